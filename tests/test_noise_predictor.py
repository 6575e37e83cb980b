"""fastdiff_amd.NoisePredictor -- the scheduling network of this project's own design (the reference ships none) -- and what stands next
to it on the host: calc_diffusion_hyperparams and the host twin of fd_phi_draw's step choice.

CPU: the parameter table, the range of beta_hat, the R = 1 form, the hyper-parameter dictionary, phi_draw_plan against oracle/philox.py.
GPU: the HIP operators (fd_bandpool_*, fd_npred_head_*) against reference_forward and its autograd in float64.

The bar of the GPU comparison.  For every output and gradient tensor the error is taken relative to max(1, max|ref|) and must not
exceed max(1e-6, K * e32), e32 being the error of the float32 torch evaluation of reference_forward on the same inputs (CPU), and never
2e-5.  K = twice the worst ratio HIP error / e32 measured over the case list below on an MI355X, rounded up, and refused above 8
(LABBOOK.md R16.1 holds the table).  Ratios are taken where the HIP error exceeds the 1e-6 floor, since below it the floor decides
and e32 may be 0: there the worst ratio is 1.0 (feat 1.90e-6 and d band.weight 3.01e-6 at B = 20, L = 64, F = 1 frame, the float32
evaluation at the same distance), so K = 2.  Below the floor the ratios scatter up to 11 on errors of 1e-8.
"""
import numpy as np
import pytest
import torch

import fastdiff_amd
from fastdiff_amd import lvc_op, sampler

K_F32 = 2           # twice the worst measured ratio (1.0), rounded up (module docstring)
FLOOR, CEIL = 1e-6, 2e-5
NAMES = {"band.weight": (32, 64), "band.bias": (32,), "fc1.weight": (64, 34), "fc1.bias": (64,), "fc2.weight": (1, 64), "fc2.bias": (1,)}


def make_predictor(seed=7):
    torch.manual_seed(seed)
    return fastdiff_amd.NoisePredictor()


def make_inputs(B, L, scale, zero_item, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g, dtype=torch.float64) * scale
    if zero_item is not None:
        x[zero_item] = 0.0
    beta_next = 1e-4 + 0.5 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    delta2 = torch.exp(np.log(1e-6) * torch.rand(B, 1, generator=g, dtype=torch.float64))      # log-uniform on (1e-6, 1)
    gw = torch.randn(B, generator=g, dtype=torch.float64)                                        # d loss / d beta_hat
    return x.float(), beta_next.float(), delta2.float(), gw.float()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes():
    sd = make_predictor().state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == NAMES
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert {"NoisePredictor", "PhiStep", "calc_diffusion_hyperparams"} <= set(fastdiff_amd.__all__)


def test_call_needs_a_hip_device():
    p = make_predictor()
    with pytest.raises(RuntimeError, match="HIP device"):
        p(torch.zeros(1, 64), (torch.full((1, 1), 0.1), torch.full((1, 1), 0.5)))


def test_reference_forward_stays_inside_its_range():
    p = make_predictor().double()
    with torch.no_grad():
        for i in range(100):
            B, L = 1 + i % 4, 64 + 32 * (i % 9)
            x, bn, d2, _ = (t.double() for t in make_inputs(B, L, (1.0, 0.05, 1e-3, 30.0)[i % 4], None, 1000 + i))
            if i % 5 == 0:
                d2[0] = 1e-6
            if i % 7 == 0:
                x[-1] = 0.0
            out = p.reference_forward(x, (bn, d2))
            assert out.shape == (B, 1, 1)
            top = torch.minimum(bn, d2).view(B, 1, 1)
            assert bool((out > 0).all()) and bool((out < top).all()), (i, out.flatten(), top.flatten())


def test_one_condition_for_a_batch_is_the_mean_of_the_ratios():
    p = make_predictor().double()
    x, bn, d2, _ = (t.double() for t in make_inputs(5, 256, 1.0, 2, 3))
    with torch.no_grad():
        one = p.reference_forward(x, (bn[:1], d2[:1]))
        each = p.reference_forward(x, (bn[:1].expand(5, 1), d2[:1].expand(5, 1)))
    scale = torch.minimum(bn[0], d2[0])
    ratios = each.view(5) / scale
    assert one.shape == (1, 1, 1)
    assert abs(float(one) - float(scale * ratios.mean())) <= 1e-15 * float(scale)
    with pytest.raises(ValueError):
        p.reference_forward(x, (bn[:2], d2[:2]))


def test_calc_diffusion_hyperparams():
    dh = fastdiff_amd.calc_diffusion_hyperparams(1000, 1e-6, 0.01, 50, 8, 0.5, 0.2, 1e-3)
    ref = sampler.compute_hyperparams_given_schedule(torch.linspace(1e-6, 0.01, 1000))
    assert dh["T"] == ref["T"] == 1000
    for k in ("beta", "alpha", "sigma"):
        assert torch.equal(dh[k], ref[k]) and dh[k].dtype == torch.float32
    assert (dh["tau"], dh["N"], dh["betaN"], dh["alphaN"], dh["rho"]) == (50, 8, 0.5, 0.2, 1e-3)
    assert sampler.calc_diffusion_hyperparams is fastdiff_amd.calc_diffusion_hyperparams


def test_phi_draw_plan_is_the_formula_on_the_oracle_generator():
    import philox
    rng = np.random.default_rng(5)
    for i in range(1000):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) if i % 3 else i
        it = int(rng.integers(0, 2 ** 63)) if i % 4 == 0 else int(rng.integers(0, 100000))
        B = int(rng.integers(1, 24))
        T_train, tau = ((1000, 50), (1000, 200), (7, 3), (101, 50))[i % 4]
        ts = lvc_op.phi_draw_plan(seed, it, B, T_train, tau)
        b = np.arange(B)
        w = np.stack(philox.words(seed, 0xFFFFFFFA, b >> 2, it), -1)[b, b & 3]
        ref = tau + ((w * np.uint64(T_train - 2 * tau)) >> np.uint64(32)).astype(np.int64)
        assert ts.dtype == np.int64 and np.array_equal(ts, ref), (seed, it, B)
        assert ts.min() >= tau and ts.max() < T_train - tau
    with pytest.raises(ValueError):
        lvc_op.phi_draw_plan(0, 0, 4, 100, 50)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
# F = L / 32 - 1 frames.  A thread's run is 16 frames, a workgroup takes 128, the final workgroup of the forward walks the per-workgroup
# sums in 8 strided lanes (P = 8 | 9 workgroups at F = 1024 | 1025): one frame short of, at and one past each border.
_BORDERS = [32 * (F + 1) for F in (15, 16, 17, 127, 128, 129, 1023, 1024, 1025)]
_LENGTHS = [64, 96, 256, 288, 1536, 8224, 25600]
CASES = [(B, L) for B in (1, 2, 3, 20) for L in _LENGTHS] + [(2, L) for L in _BORDERS]
_SCALES = (1.0, 0.05, 1e-3)


def _case_inputs(i, B, L):
    zero_item = (i % B) if (B > 1 and i % 2 == 0) else None
    return make_inputs(B, L, _SCALES[i % 3], zero_item, 100 + i)


def _reference(p, x, bn, d2, gw, dtype):
    """feat, beta_hat and the six gradients of sum(gw * beta_hat) by reference_forward and torch's autograd on the CPU in `dtype`."""
    q = make_predictor().to(dtype)
    q.load_state_dict({k: v.to(dtype) for k, v in p.state_dict().items()})
    x, bn, d2, gw = (t.to(dtype) for t in (x, bn, d2, gw))
    out = q.reference_forward(x, (bn, d2))
    (out.view(-1) * gw).sum().backward()
    res = {"feat": q.features(x).detach(), "beta_hat": out.detach().view(-1)}
    res.update({"d " + k: v.grad for k, v in q.named_parameters()})
    return {k: v.double() for k, v in res.items()}


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / max(1.0, float(ref.abs().max())))


@pytest.fixture(scope="module")
def cuda_predictor():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return make_predictor().cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"B{B}-L{L}" for B, L in CASES])
def test_operators_against_float64(cuda_predictor, i):
    B, L = CASES[i]
    p = cuda_predictor
    x, bn, d2, gw = _case_inputs(i, B, L)
    cpu = make_predictor()
    ref64, ref32 = _reference(cpu, x, bn, d2, gw, torch.float64), _reference(cpu, x, bn, d2, gw, torch.float32)

    def run():
        p.zero_grad(set_to_none=True)
        out = p(x.cuda(), (bn.cuda(), d2.cuda()))
        (out.view(-1) * gw.cuda()).sum().backward()
        res = {"feat": lvc_op.band_pool(x.cuda(), p.band.weight.detach(), p.band.bias.detach()), "beta_hat": out.detach().view(-1)}
        res.update({"d " + k: v.grad.clone() for k, v in p.named_parameters()})
        return res

    got, again = run(), run()
    worst = []
    for k, ref in ref64.items():
        e_hip, e_32 = _rel(got[k].cpu(), ref), _rel(ref32[k], ref)
        print(f"B={B} L={L} {k:14s} hip {e_hip:.2e}  f32 torch {e_32:.2e}  ratio {e_hip / e_32 if e_32 > 0 else float('inf'):.2f}")
        if not e_hip <= min(CEIL, max(FLOOR, K_F32 * e_32)):
            worst.append((k, e_hip, e_32))
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    assert not worst, worst


@pytest.mark.gpu
def test_items_together_equal_items_alone(cuda_predictor):
    p = cuda_predictor
    for B, L in ((3, 288), (20, 4160)):
        x, bn, d2, _ = (t.cuda() for t in _case_inputs(1, B, L))
        with torch.no_grad():
            together = p(x, (bn, d2))
            alone = torch.cat([p(x[b:b + 1], (bn[b:b + 1], d2[b:b + 1])) for b in range(B)])
        assert together.shape == (B, 1, 1) and torch.equal(together, alone)


@pytest.mark.gpu
def test_one_condition_for_a_batch_on_the_device(cuda_predictor):
    p = cuda_predictor
    x, bn, d2, _ = _case_inputs(3, 5, 1536)
    with torch.no_grad():
        one = p(x.cuda(), (bn[:1].cuda(), d2[:1].cuda()))
        each = p(x.cuda(), (bn[:1].expand(5, 1).contiguous().cuda(), d2[:1].expand(5, 1).contiguous().cuda()))
        cpu = make_predictor()
        ref64 = cpu.double().reference_forward(x.double(), (bn[:1].double(), d2[:1].double()))
        ref32 = make_predictor().reference_forward(x, (bn[:1], d2[:1]))
    assert one.shape == (1, 1, 1)
    e_hip, e_32 = _rel(one.cpu(), ref64), _rel(ref32, ref64)
    print(f"R = 1: hip {e_hip:.2e}  f32 torch {e_32:.2e}")
    assert e_hip <= min(CEIL, max(FLOOR, K_F32 * e_32))
    # the sum of the ratios in item order, divided by B, times the scale: each operation in float32
    scale = torch.minimum(bn[0], d2[0]).cuda()
    ratios = (each.view(5) / scale)
    assert abs(float(one) - float(scale * ratios.mean())) <= 16 * 2.0 ** -24 * float(scale)      # some ten float32 roundings on values <= scale
    with pytest.raises(RuntimeError, match="no_grad"):
        p(x.cuda(), (bn[:1].cuda(), d2[:1].cuda()))


@pytest.mark.gpu
def test_operators_refuse_what_they_cannot_run(cuda_predictor):
    p = cuda_predictor
    with torch.no_grad():
        with pytest.raises(ValueError):
            p(torch.zeros(2, 100).cuda(), (torch.full((2, 1), 0.1).cuda(), torch.full((2, 1), 0.5).cuda()))
        with pytest.raises(ValueError):
            p(torch.zeros(2, 32).cuda(), (torch.full((2, 1), 0.1).cuda(), torch.full((2, 1), 0.5).cuda()))
