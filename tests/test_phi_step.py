"""One training step of the scheduling network on the device (fastdiff_amd.PhiStep) and its pieces: fd_phi_draw against torch's own
float32 expressions and oracle/philox.py, fd_phi_residual_forward against the reference's phi_loss (golden: gen_phi_loss) and float64
autograd, the step against a float64 evaluation on its own draws, determinism, the corpus path, phi_loss(noise_source="device").

Bars against float64 are those of tests/test_noise_predictor.py: relative to max(1, max|ref|), at most max(1e-6, K * e32) with e32 the
error of the float32 torch evaluation of the same expression on the same inputs, and never above 2e-5."""
import numpy as np
import pytest
import torch

import fastdiff_amd
import synth
from conftest import load_golden
from fastdiff_amd import lvc_op, sampler
from fastdiff_amd.corpus import TrainCorpus
from test_device_noise import Pool
from test_noise_predictor import CEIL, FLOOR, K_F32, make_predictor

pytestmark = pytest.mark.gpu
HOP, TAU = 256, 50


@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def model(gc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gc.make_model()


@pytest.fixture(scope="module")
def dh():
    return fastdiff_amd.calc_diffusion_hyperparams(1000, 1e-6, 0.01, TAU, 8, 0.5, 0.2, 1e-3)


def within(err, e32):
    return err <= min(CEIL, max(FLOOR, K_F32 * e32))


def rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def reference_phi_loss(pred, alpha, tau, ts, x_t, z, eps, dtype, beta_hat=None, delta=None):
    """util.py:340-362 on given steps, x_t, z and eps in `dtype` on the CPU; the predictor's reference_forward unless beta_hat is given;
    delta recomputed from the table in `dtype` unless given as data."""
    B = x_t.shape[0]
    alpha, x_t, z, eps = (t.detach().cpu().to(dtype) for t in (alpha, x_t, z, eps))
    ts = ts.cpu().long().view(B)
    alpha_cur = alpha.index_select(0, ts).view(B, 1, 1)
    alpha_nxt = alpha.index_select(0, ts + tau).view(B, 1, 1)
    beta_nxt = 1 - (alpha_nxt / alpha_cur) ** 2.
    delta = (1 - alpha_cur ** 2.).sqrt() if delta is None else delta.detach().cpu().to(dtype).view(B, 1, 1)
    if beta_hat is None:
        beta_hat = pred.reference_forward(x_t.view(B, -1), (beta_nxt.view(B, 1), delta.view(B, 1) ** 2.))
    loss = 1 / (2. * (delta ** 2. - beta_hat)) * (delta * z - beta_hat / delta * eps) ** 2.
    loss = loss + torch.log(1e-8 + delta ** 2. / (beta_hat + 1e-8)) / 4.
    return (torch.mean(loss, -1, keepdim=True) + beta_hat / delta ** 2 / 2.).mean()


def batch(seed, B, F):
    mel = torch.from_numpy(synth.synth_mel(seed, B, F)).cuda()
    gen = torch.Generator().manual_seed(seed)
    wav = (0.3 * torch.randn(B, 1, F * HOP, generator=gen)).cuda()
    return mel, wav


# ---- fd_phi_draw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 256), (3, 256), (5, 256), (1, 1536), (3, 1536), (5, 1536)])
def test_phi_draw_is_torch_on_the_same_draws(dh, B, L):
    import philox
    seed, it = 1234 + B, 7 + L
    alpha = dh["alpha"].cuda()
    gen = torch.Generator().manual_seed(L + B)
    x0 = (0.3 * torch.randn(B, 1, L, generator=gen)).cuda()
    x_t, z, steps, beta_nxt, delta, delta2 = lvc_op.phi_draw(x0, alpha, 1000, TAU, seed=seed, iteration=it)
    plan = lvc_op.phi_draw_plan(seed, it, B, 1000, TAU)
    assert steps.shape == (B, 1) and np.array_equal(steps.cpu().numpy().reshape(B), plan.astype(np.float32))
    # z: the generator's normal4 at stream 0xFFFFFFF9 with the step index in the id slot, to the element bar of tests/test_device_noise.py
    q = philox.normal4_f64(seed, 0xFFFFFFF9, np.arange(B * L // 4, dtype=np.uint64), uid=it).reshape(B, 1, L)
    Pool().check(z, q, f"fd_phi_draw z B={B} L={L}")
    # the rest: sampler.phi_loss's own float32 expressions (lines 261-266) on the drawn ts and z, bit for bit
    ts = torch.from_numpy(plan).cuda()
    alpha_cur = alpha.index_select(0, ts).view(B, 1, 1)
    alpha_nxt = alpha.index_select(0, ts + TAU).view(B, 1, 1)
    assert torch.equal(beta_nxt.view(B, 1, 1), 1 - (alpha_nxt / alpha_cur) ** 2.)
    d = (1 - alpha_cur ** 2.).sqrt()
    assert torch.equal(delta.view(B, 1, 1), d)
    assert torch.equal(delta2.view(B, 1), d.view(B, 1) ** 2.)
    assert torch.equal(x_t, alpha_cur * x0 + d * z)
    # a second call agrees; another iteration draws anew; the state's counter is the iteration
    again = lvc_op.phi_draw(x0, alpha, 1000, TAU, seed=seed, iteration=it)
    assert all(torch.equal(a, b) for a, b in zip(again, (x_t, z, steps, beta_nxt, delta, delta2)))
    state = lvc_op.new_train_state(x0.device)
    state[0] = it
    by_state = lvc_op.phi_draw(x0, alpha, 1000, TAU, seed=seed, iteration=0, state=state)
    assert torch.equal(by_state[0], x_t) and torch.equal(by_state[2], steps)
    assert not torch.equal(lvc_op.phi_draw(x0, alpha, 1000, TAU, seed=seed, iteration=it + 1)[1], z)


def test_phi_draw_refuses_a_table_shorter_than_two_tau(dh):
    x0 = torch.zeros(1, 1, 256).cuda()
    with pytest.raises(AssertionError, match="2 tau"):
        lvc_op.phi_draw(x0, dh["alpha"][:100].cuda().contiguous(), 100, 50)


# ---- fd_phi_residual_forward -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_draw(model, dh):
    """The golden's recorded ts and z as a draw tuple (sampler.phi_loss's float32 expressions), with the HIP eps."""
    g = load_golden("phi_loss")
    sched = load_golden("schedule")
    alpha = torch.from_numpy(sched["train_alpha"]).cuda()
    B = g["audio"].shape[0]
    ts = torch.from_numpy(g["ts"]).cuda().view(B)
    z, audio, mel = (torch.from_numpy(g[k]).cuda() for k in ("z", "audio", "mel"))
    alpha_cur = alpha.index_select(0, ts).view(B, 1, 1)
    alpha_nxt = alpha.index_select(0, ts + int(g["tau"])).view(B, 1, 1)
    beta_nxt = (1 - (alpha_nxt / alpha_cur) ** 2.).view(B, 1)
    delta = (1 - alpha_cur ** 2.).sqrt()
    x_t = alpha_cur * audio + delta * z
    draw = (x_t, z, ts.float().view(B, 1), beta_nxt, delta.view(B, 1), delta.view(B, 1) ** 2.)
    with torch.no_grad():
        eps = model((x_t, mel, draw[2]))
    return g, alpha, mel, draw, eps


def test_phi_residual_reproduces_the_reference_loss(model, golden_draw):
    g, alpha, mel, draw, eps = golden_draw
    with torch.no_grad():
        loss = sampler.phi_loss_from_draw(model, synth.stub_noise_pred_batch, mel, draw)
    ref = float(g["loss_f64"])
    print("phi loss on the HIP residual %.9f, |d| vs f64 reference %.2e (fp32 reference: %.2e)" % (loss.item(), abs(loss.item() - ref), abs(float(g["loss_f32"]) - ref)))
    assert abs(loss.item() - ref) < 2e-6 * abs(ref)
    # m and s themselves against float64 on the same eps and z, and twice the same bits
    x_t, z, _, _, delta, _ = draw
    beta_hat = synth.stub_noise_pred_batch(x_t.squeeze(1), (draw[3], draw[5])).reshape(-1).contiguous()
    B = z.shape[0]
    m, s = (torch.empty(B, device=z.device) for _ in range(2))
    m2, s2 = (torch.empty(B, device=z.device) for _ in range(2))
    for mm, ss in ((m, s), (m2, s2)):
        lvc_op._call(z.device, "fd_phi_residual_forward", "fd_phi_residual_forward", eps, z, delta.contiguous(), beta_hat, B, z.numel() // B, mm, ss)
    assert torch.equal(m, m2) and torch.equal(s, s2)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        d, bh, e, zz = (t.cpu().to(dtype).view(B, -1) for t in (delta, beta_hat, eps, z))
        r = d * zz - bh / d * e
        refs[dtype] = {"m": (r * r).mean(-1), "s": (r * e).mean(-1)}
    ref64, ref32 = refs[torch.float64], refs[torch.float32]
    for k, got in (("m", m), ("s", s)):
        e_hip, e_32 = rel(got, ref64[k]), rel(ref32[k], ref64[k])
        print(f"{k}: hip {e_hip:.2e}  f32 torch {e_32:.2e}")
        assert within(e_hip, e_32)


def test_phi_residual_backward_against_float64_autograd(model, golden_draw):
    """d loss / d beta_hat through fd_phi_residual's own backward and torch's autograd on the [B] algebra, against float64 autograd of the
    reference expression on the operator's own inputs: eps, z and the float32 delta it is handed.  At ts = 50 the stand-in predictor
    returns 0.9 delta^2, so the gradient (1.7e3) goes like (delta^2 - beta_hat)^-2 with delta^2 - beta_hat = 0.1 delta^2: a reference that
    instead recomputes delta = sqrt(1 - alpha^2) in float64 sits 3.4e-5 away from ANY float32 evaluation (HIP 3.38e-5, float32 torch
    3.37e-5 on an MI355X) -- the cancellation in 1 - alpha^2, which is an input of the operator, not its arithmetic.  That form is held
    to the float32 yardstick alone, below."""
    g, alpha, mel, draw, eps = golden_draw
    x_t, z, steps, _, delta, _ = draw
    B = z.shape[0]
    start = synth.stub_noise_pred_batch(x_t.squeeze(1), (draw[3], draw[5])).reshape(B).detach()
    leaf = start.clone().requires_grad_(True)
    loss = sampler.phi_loss_from_draw(model, lambda x, cond: leaf.view(B, 1, 1), mel, draw)
    loss.backward()
    for tag, given in (("delta as data", delta), ("delta recomputed", None)):
        refs = {}
        for dtype in (torch.float64, torch.float32):
            bh = start.cpu().to(dtype).requires_grad_(True)
            reference_phi_loss(None, alpha, int(g["tau"]), steps, x_t, z, eps, dtype, beta_hat=bh.view(B, 1, 1), delta=given).backward()
            refs[dtype] = bh.grad
        e_hip, e_32 = rel(leaf.grad, refs[torch.float64]), rel(refs[torch.float32], refs[torch.float64])
        print(f"d loss / d beta_hat ({tag}):", leaf.grad.tolist(), f"hip {e_hip:.2e}  f32 torch {e_32:.2e}")
        assert within(e_hip, e_32) if given is not None else e_hip <= max(FLOOR, K_F32 * e_32)


# ---- PhiStep -----------------------------------------------------------------------------------------------------------------------------------
def test_one_step_against_float64(model, dh):
    B, F = 3, 6
    mel, wav = batch(21, B, F)
    pred = make_predictor().cuda()
    before = {k: v.clone() for k, v in pred.state_dict().items()}
    theta = [p.detach().clone() for p in model.parameters()]
    ps = fastdiff_amd.PhiStep(model, pred, dh, seed=5)
    loss = ps.step(mel, wav)
    st = ps.state()
    assert st["applied"] == 1 and st["iter"] == 1 and st["skipped"] == 0 and st["loss"] == loss.item()
    assert all(torch.equal(a, b) for a, b in zip(theta, model.parameters())), "the denoiser is frozen"
    assert all(not torch.equal(before[k], v) for k, v in pred.state_dict().items()), "all six tensors move"
    x_t, z, steps = ps.draw[:3]
    assert np.array_equal(steps.cpu().numpy().reshape(B), lvc_op.phi_draw_plan(5, 0, B, 1000, TAU).astype(np.float32))
    with torch.no_grad():
        eps = model((x_t, mel, steps))
    refs = {}
    for dtype in (torch.float64, torch.float32):
        q = make_predictor().to(dtype)
        q.load_state_dict({k: v.cpu().to(dtype) for k, v in before.items()})
        l = reference_phi_loss(q, dh["alpha"], TAU, steps, x_t, z, eps, dtype)
        l.backward()
        refs[dtype] = dict({"loss": l.detach()}, **{"d " + k: p.grad for k, p in q.named_parameters()})
    got = dict({"loss": loss}, **{"d " + k: p.grad for k, p in pred.named_parameters()})
    bad = []
    for k, ref in refs[torch.float64].items():
        e_hip, e_32 = rel(got[k], ref), rel(refs[torch.float32][k], ref)
        print(f"{k:14s} hip {e_hip:.2e}  f32 torch {e_32:.2e}  (max |ref| {float(ref.abs().max()):.3e})")
        if not within(e_hip, e_32):
            bad.append((k, e_hip, e_32))
    assert not bad, bad
    # phi_loss(noise_source="device") is the step's loss, bit for bit, on the parameters the step started from
    pred.load_state_dict(before)
    model.noise_pred = pred
    try:
        again = fastdiff_amd.phi_loss(model, (mel, wav), dh, noise_source="device", seed=5, iteration=0)
    finally:
        del model.noise_pred
    assert torch.equal(again.detach(), loss)
    with pytest.raises(AttributeError):
        fastdiff_amd.phi_loss(model, (mel, wav), dh, noise_source="device", seed=5, iteration=0)


def test_three_steps_twice_give_the_same_parameters(model, dh):
    mel, wav = batch(22, 3, 6)
    runs = []
    for _ in range(2):
        pred = make_predictor().cuda()
        ps = fastdiff_amd.PhiStep(model, pred, dh, seed=9)
        losses = [ps.step(mel, wav).clone() for _ in range(3)]
        runs.append((losses, [p.detach().clone() for p in pred.parameters()], ps.state()))
    assert runs[0][2]["iter"] == 3 and runs[0][2] == runs[1][2]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert not torch.equal(runs[0][0][0], runs[0][0][1]), "every step draws anew"


def test_steps_cut_from_a_corpus_follow_the_plan(model, dh):
    F, lengths = 6, [9, 14, 8, 11]
    mel = synth.synth_mel(3, 1, sum(lengths))[0].T
    gen = torch.Generator().manual_seed(11)
    items, at = [], 0
    for T in lengths:
        items.append({"mel": np.ascontiguousarray(mel[at: at + T]), "wav": (0.3 * torch.randn(T * HOP, generator=gen)).numpy()})
        at += T
    corpus = TrainCorpus(items, hop_size=HOP, max_samples=F * HOP, device="cpu").to("cuda")
    pred = make_predictor().cuda()
    ps = fastdiff_amd.PhiStep(model, pred, dh, seed=3, corpus=corpus, batch_size=3)
    for it in range(2):
        loss = ps.step()
        want_items, want_starts = corpus.plan(it, 3, seed=3)
        assert np.array_equal(ps.picked.cpu().numpy(), np.stack([want_items, want_starts], 1))
        assert bool(torch.isfinite(loss))
    mels, wavs = corpus.cut(want_items, want_starts)
    assert torch.equal(ps.mel, mels) and torch.equal(ps.wav, wavs)
    # the optimizer's state in torch.optim.AdamW's layout, and back
    sd = ps.state_dict()
    assert sorted(sd["state"]) == list(range(6)) and float(sd["state"][0]["step"]) == 2.0 and sd["train_step"]["iter"] == 2
    opt = torch.optim.AdamW(pred.parameters(), lr=1e-3)
    opt.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    other = fastdiff_amd.PhiStep(model, pred, dh, seed=3, corpus=corpus, batch_size=3)
    other.load_state_dict(sd)
    assert other.state()["iter"] == 2 and all(torch.equal(a, b) for a, b in zip(other.exp_avg, ps.exp_avg))
    ps.set_lr(1e-5)
    assert ps.hyper["lr"] == 1e-5
    with pytest.raises(RuntimeError):
        fastdiff_amd.PhiStep(model, pred, dh).step()
