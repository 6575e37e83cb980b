"""The whole training step on the device (fastdiff_amd.TrainStep; fd_train_draw, fd_mse_forward / _backward, fd_adamw_multi).

CPU: the new entry points are declared, exported and bound; the host twin of the step draw (`ts` over oracle/philox.py's words) is in
range, uniform and distinct per step index; the optimizer test's gradients stay clear of the clip threshold.
GPU: the draws against the twin (exact `steps`, z to the bars of tests/test_device_noise.py, x_t bit for bit what torch forms from the
returned z); the step counter lives on the device (a captured step draws it = 0, 1, 2 on three replays); the loss and its gradient
against float64; clip + guard + AdamW against clip_grad_norm_ + torch.optim.AdamW in float64; one whole TrainStep.step against the
eager composition of the same pieces.

Sums: a thread adds K_RUN = 16 elements serially (FD_STEP_RUN); everything behind that is a tree -- butterfly inside a wave, the four
waves of a workgroup, the per-workgroup results 256 at a time and then the results of that (up to 65536 workgroups, 2^28 elements) --
so an element passes through about K_RUN + log2(n / K_RUN) additions, plus the roundings of forming the square: the bound
(K_RUN + log2(n / K_RUN) + 2) * 2^-24 the issue sets.  (The norm is the square root of such a sum: half its relative error.)
"""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox   # noqa: E402
import synth    # noqa: E402

import fastdiff_amd                      # noqa: E402
from fastdiff_amd import _capi, schedules   # noqa: E402

K_RUN = 16                               # FD_STEP_RUN: the per-thread serial run length of the kernels' sums
NEW = ("fd_train_draw", "fd_mse_forward", "fd_mse_backward", "fd_adamw_multi")
TS_STREAM, Z_STREAM = 0xFFFFFFFD, 0xFFFFFFFE
SEEDS = (1234, 2 ** 32 + 7, 2 ** 63 + 7)
ITS = (0, 1, 2 ** 32 + 3)


def sum_bound(n):
    return (K_RUN + math.log2(n / K_RUN) + 2) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the twin
def ts_of_word(w, T):
    """ts = (uint64(w) * T) >> 32 for 32-bit words w."""
    return ((philox._u64(w) & philox.M32) * np.uint64(T)) >> np.uint64(32)


def ts_twin(seed, it, B, T):
    """[B] int64: item b takes output word b & 3 of the Philox call keyed (seed, stream 0xFFFFFFFD, position b >> 2, id it)."""
    b = np.arange(B, dtype=np.uint64)
    w = np.stack(philox.words(seed, TS_STREAM, b >> np.uint64(2), uid=it), axis=-1)
    return ts_of_word(w[np.arange(B), (b & np.uint64(3)).astype(np.int64)], T).astype(np.int64)


def z_twin(seed, it, B, L):
    """[B, 1, L] float64: the flat index convention of philox.z() on stream 0xFFFFFFFE with the step index in the id slot."""
    assert (B * L) % 4 == 0
    return philox.normal4_f64(seed, Z_STREAM, np.arange(B * L // 4, dtype=np.uint64), uid=it).reshape(B, 1, L)


def chi2_critical(df, tail):
    """x with P(chi2_df > x) = tail, by bisection on the regularised upper incomplete gamma function."""
    lo, hi = float(df), 4.0 * df
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        sf = float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(mid / 2.0, dtype=torch.float64)))
        lo, hi = (mid, hi) if sf > tail else (lo, mid)
    return 0.5 * (lo + hi)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_train.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert hasattr(lib, name), name
    assert inspect.isclass(fastdiff_amd.TrainStep) and "TrainStep" in fastdiff_amd.__all__
    sig = inspect.signature(fastdiff_amd.TrainStep.__init__).parameters
    assert [sig[k].default for k in ("lr", "betas", "eps", "weight_decay", "clip_grad_norm", "seed", "graph")] == [2e-4, (0.9, 0.98), 1e-8, 0.0, 1.0, 0, True]
    for method in ("step", "set_lr", "state", "state_dict", "load_state_dict"):
        assert callable(getattr(fastdiff_amd.TrainStep, method))
    p = inspect.signature(fastdiff_amd.theta_timestep_loss).parameters
    assert list(p)[:4] == ["net", "X", "diffusion_hyperparams", "reverse"]
    for name, default in (("noise_source", "reference"), ("seed", 0), ("iteration", 0)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    from fastdiff_amd import lvc_op
    import ctypes as ct
    assert ct.sizeof(lvc_op.AdamWHyper) == 48 and (lvc_op.TS_STREAM, lvc_op.Z_STREAM) == (TS_STREAM, Z_STREAM)
    assert f"#define FD_STEP_RUN {K_RUN}" in header


def test_step_draw_twin_is_in_range_uniform_and_distinct_per_step():
    for T in (1, 2, 50, 1000, 2 ** 31):
        assert int(ts_of_word(0, T)) == 0 and int(ts_of_word(2 ** 32 - 1, T)) == T - 1
    T, n = 1000, 1 << 16
    ts = ts_twin(1234, 0, n, T)
    assert ts.min() >= 0 and ts.max() < T
    counts = np.bincount(ts, minlength=T).astype(np.float64)
    chi2 = float(((counts - n / T) ** 2 / (n / T)).sum())
    crit = chi2_critical(T - 1, 1e-3)
    assert 1130.0 < crit < 1160.0, crit                     # (sanity of the bisection: 999 + 3.09 * sqrt(2 * 999) = 1137 to first order)
    print(f"chi-square of 2^16 step draws over T = 1000: {chi2:.1f} (0.1 % critical value {crit:.1f})")
    assert chi2 < crit, (chi2, crit)
    its = (0, 1, 2 ** 32)
    draws = [(ts_twin(1234, it, 64, T), z_twin(1234, it, 2, 64)) for it in its]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(draws[i][0], draws[j][0]), (its[i], its[j])
            assert not (draws[i][1] == draws[j][1]).any(), (its[i], its[j])
    # neither stream is one the sampler uses (x_T: 0xFFFFFFFF, z_k: k < 1024)
    assert not (z_twin(1234, 0, 2, 64) == philox.x_T(1234, 2, 64)).any()


# ---- the optimizer test's inputs (shared by the CPU check of the choice and the GPU test) ---------------------------------------------
MAX_NORM = 1.0
FROZEN = 5                               # the item that takes no part (g = NULL)
G_ABOVE, G_BELOW = 1e-2, 1e-5          # gradient scales: the norm well above max_norm, and the same gradients scaled by 1e-3
N_STEPS = 5


def _shapes():
    torch.manual_seed(0)
    return [tuple(p.shape) for p in fastdiff_amd.FastDiff().parameters()]


def _hash_tensors(seed, stream, shapes, scale, device):
    import gpu_common
    n = sum(int(np.prod(s)) for s in shapes)
    flat = gpu_common.hash_normal_torch(seed, stream, n, device=device) * scale
    return [t.view(s) for t, s in zip(flat.split([int(np.prod(s)) for s in shapes]), shapes)]


def test_optimizer_gradients_stay_clear_of_the_clip_threshold():
    """The float64 norm of every step's gradients is a factor of 2 away from max_norm in the clipped and in the unclipped cases (item
    FROZEN has no gradient), so no rounding decides whether a step is clipped."""
    shapes = _shapes()
    assert len(shapes) == 175
    for step in range(N_STEPS):
        g = _hash_tensors(77, 10 + step, shapes, 1.0, "cpu")
        norm = math.sqrt(sum(float((t.double() ** 2).sum()) for i, t in enumerate(g) if i != FROZEN))
        print(f"step {step}: gradient norm {norm * G_ABOVE:.3f} (above) / {norm * G_BELOW:.5f} (below)")
        assert norm * G_ABOVE > 2 * MAX_NORM and norm * G_BELOW < MAX_NORM / 2


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.mark.gpu
def test_draws_match_the_twin(gc):
    """steps exactly, z to N_ULP / P999_ULP / |z| <= 5.887 (test_device_noise.Pool), x_t bit for bit torch's expression on the returned z."""
    from test_device_noise import Pool
    from fastdiff_amd import lvc_op
    dh = schedules.training_hyperparams()
    T, alpha = dh["T"], dh["alpha"].cuda()
    pool = Pool()
    for B, L in ((20, 25600), (7, 25600), (7, 132)):
        if L == 132:
            assert (B * L // 4) % 2 == 1
        x0 = (0.3 * gc.hash_normal_torch(3, B, B * L)).view(B, 1, L)
        for seed in SEEDS:
            for it in ITS:
                x_t, z, steps = lvc_op.train_draw(x0, alpha, T, seed=seed, iteration=it)
                torch.cuda.synchronize()
                ts = ts_twin(seed, it, B, T)
                assert steps.shape == (B, 1) and steps.dtype == torch.float32
                assert np.array_equal(steps.cpu().numpy().reshape(-1), ts.astype(np.float32)), (B, L, seed, it)
                pool.check(z, z_twin(seed, it, B, L), f"B={B} L={L} seed={seed} it={it}")
                a = alpha[torch.from_numpy(ts).cuda().view(B, 1, 1)]
                want = a * x0 + (1 - a ** 2.).sqrt() * z
                assert torch.equal(x_t, want), (B, L, seed, it, float((x_t - want).abs().max()))
    pool.finish("fd_train_draw")
    # the state's counter takes the place of iter_host
    st = lvc_op.new_train_state("cuda")
    st[0] = 2 ** 32 + 3
    x0 = (0.3 * gc.hash_normal_torch(3, 7, 7 * 132)).view(7, 1, 132)
    a = lvc_op.train_draw(x0, alpha, T, seed=1234, iteration=999, state=st)
    b = lvc_op.train_draw(x0, alpha, T, seed=1234, iteration=2 ** 32 + 3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _batch(gc, B=2, T=6):
    mel = torch.from_numpy(synth.synth_mel(3, B, T)).cuda()
    wav = (0.3 * gc.hash_normal_torch(3, 1, B * T * 256)).view(B, 1, T * 256)
    return mel, wav


@pytest.mark.gpu
def test_step_counter_lives_on_the_device(gc):
    """One capture, three replays: the draws are the twin's for it = 0, 1, 2.  That the step captures is the check that nothing in it
    synchronises."""
    from test_device_noise import Pool
    dh = schedules.training_hyperparams()
    m = gc.make_model().train()
    seed = 2 ** 32 + 7
    ts = fastdiff_amd.TrainStep(m, dh, seed=seed)
    mel, wav = _batch(gc)
    B, L = wav.shape[0], wav.shape[-1]
    pool = Pool()
    graphs = set()
    for it in range(3):
        loss = ts.step(mel, wav)
        graphs.add(id(ts._graph))
        torch.cuda.synchronize()
        assert ts._graph is not None and math.isfinite(float(loss))
        assert np.array_equal(ts.steps.cpu().numpy().reshape(-1), ts_twin(seed, it, B, dh["T"]).astype(np.float32)), it
        pool.check(ts.z, z_twin(seed, it, B, L), f"replay {it}")
    assert len(graphs) == 1, "captured once, replayed three times"
    pool.finish("TrainStep replays")
    st = ts.state()
    assert st["iter"] == 3 and st["applied"] + st["skipped"] == 3 and st["applied"] == 3, st
    assert st["loss"] == float(loss) and math.isfinite(st["grad_norm"]) and st["grad_norm"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20 * 25600, 1000003])
def test_loss_and_its_gradient_against_float64(gc, n):
    """|loss - loss_f64| <= (K_RUN + log2(n / K_RUN) + 2) 2^-24 loss_f64; deps within 4 * 2^-24 relative, element-wise; bit-identical runs."""
    from fastdiff_amd import lvc_op
    assert n == 1000003 and n % 256 != 0 or n == 512000
    eps = gc.hash_normal_torch(11, 1, n).requires_grad_(True)
    z = gc.hash_normal_torch(11, 2, n)
    st = lvc_op.new_train_state("cuda")
    out = []
    for dl in (1.0, 0.37):
        for _ in range(2):
            loss = lvc_op.mse_loss(eps, z, st)
            (deps,) = torch.autograd.grad(loss, eps, grad_outputs=torch.tensor(dl, device="cuda"))
            out.append((loss.detach().clone(), deps.clone()))
        assert torch.equal(out[-1][0], out[-2][0]) and torch.equal(out[-1][1], out[-2][1])
        d64 = eps.detach().double() - z.double()
        loss64 = float((d64 ** 2).mean())
        err = abs(float(out[-1][0]) - loss64)
        print(f"n = {n}: loss {float(out[-1][0]):.9g}, float64 {loss64:.12g}, distance {err / loss64 / 2.0 ** -24:.3f} x 2^-24 (bound {sum_bound(n) / 2.0 ** -24:.1f})")
        assert err <= sum_bound(n) * loss64
        ref = float(np.float32(dl)) * 2.0 * d64 / n
        rel = ((out[-1][1].double() - ref).abs() - 4 * 2.0 ** -24 * ref.abs()).max()
        print(f"    deps (dloss = {dl}): worst distance {float(((out[-1][1].double() - ref).abs() / ref.abs().clamp_min(1e-300)).max()) / 2.0 ** -24:.3f} x 2^-24")
        assert float(rel) <= 0.0
    assert lvc_op.read_train_state(st)["loss"] == float(out[-1][0])
    # with dloss = 1 the gradient is torch's own, bit for bit (what lets TrainStep's gradients equal the eager step's)
    e2 = eps.detach().clone().requires_grad_(True)
    torch.nn.functional.mse_loss(e2, z).backward()
    assert torch.equal(e2.grad, out[0][1])


@pytest.mark.gpu
def test_a_growing_step_scratch_is_refused_inside_a_capture(gc):
    """A handle of its own has no step scratch yet: fd_mse_forward's first call inside a capture would have to allocate it and is refused
    with FD_ERR_STATE before any HIP call.  After one call outside a capture the same call captures, and replays the eager loss bit for bit."""
    import ctypes as ct
    lib = _capi.load()
    cfg = _capi.FdConfig()
    lib.fd_default_config(ct.byref(cfg))
    h = ct.c_void_p()
    _capi.check(lib, None, lib.fd_create(ct.byref(cfg), 0, ct.byref(h)), "fd_create")
    n = 8192                                               # two workgroups of 16 * 256 elements
    eps, z = gc.hash_normal_torch(13, 1, n), gc.hash_normal_torch(13, 2, n)
    loss = torch.zeros((), device="cuda")

    def call():
        return lib.fd_mse_forward(h, eps.data_ptr(), z.data_ptr(), n, loss.data_ptr(), None, torch.cuda.current_stream().cuda_stream)

    try:
        torch.cuda.synchronize()
        refused = torch.cuda.CUDAGraph()
        with torch.cuda.graph(refused):
            eps.mul_(1.0)                                  # (so that the abandoned capture is not empty)
            rc = call()
        assert rc == _capi.FD_ERR_STATE and b"stream capture" in lib.fd_last_error(h), (rc, lib.fd_last_error(h))
        assert call() == _capi.FD_OK, lib.fd_last_error(h)
        torch.cuda.synchronize()
        want = loss.clone()
        d64 = eps.double() - z.double()
        assert abs(float(want) - float((d64 ** 2).mean())) <= sum_bound(n) * float((d64 ** 2).mean())
        loss.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = call()
        assert rc == _capi.FD_OK, lib.fd_last_error(h)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, want)
    finally:
        torch.cuda.synchronize()
        lib.fd_destroy(h)


def _reference_adamw(dtype, p0, grads, hp, frozen=None):
    """clip_grad_norm_ + torch.optim.AdamW (foreach=False) on the CPU in `dtype`; returns (params, exp_avg, exp_avg_sq, norms)."""
    P = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in p0]
    opt = torch.optim.AdamW(P, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
    norms = []
    for g in grads:
        for i, (p, gi) in enumerate(zip(P, g)):
            p.grad = None if i == frozen or gi is None else gi.detach().cpu().to(dtype).clone()
        live = [p for p in P if p.grad is not None]
        norms.append(float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in live]))))
        if hp["max_norm"]:
            torch.nn.utils.clip_grad_norm_(live, hp["max_norm"], foreach=False)
        opt.step()
    zero = lambda p: torch.zeros_like(p)      # noqa: E731
    return ([p.detach() for p in P], [opt.state[p].get("exp_avg", zero(p)) if p in opt.state else zero(p) for p in P],
            [opt.state[p].get("exp_avg_sq", zero(p)) if p in opt.state else zero(p) for p in P], norms)


def _worst(a, b):
    return max(float((x.double().cpu() - y.double()).abs().max()) for x, y in zip(a, b))


def _check_against_float64(tag, got_p, p64, p32):
    """The bar of the optimizer checks: element-wise |HIP - f64| <= 2 * (worst |torch f32 - f64|) + 2^-24 |p|."""
    yard = _worst(p32, p64)
    dist = _worst(got_p, p64)
    print(f"{tag}: worst |torch float32 - float64| = {yard:.3e}, worst |HIP - float64| = {dist:.3e}")
    for i, (g, r) in enumerate(zip(got_p, p64)):
        over = (g.double().cpu() - r).abs() - (2 * yard + 2.0 ** -24 * r.abs())
        assert float(over.max()) <= 0.0, (tag, i, float(over.max()), yard)
    return yard, dist


CASES = [("above", G_ABOVE, MAX_NORM), ("below", G_BELOW, MAX_NORM), ("unclipped", G_ABOVE, 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clip_and_adamw_against_float64(gc, case, weight_decay):
    """The base model's 175 parameter shapes, hash-valued parameters and gradients, 5 steps; item FROZEN has g = NULL.

    The bar: element-wise |HIP - float64| <= 2 * max |torch float32 AdamW - float64| + 2^-24 |p|.  Both distances are printed per case
    (_check_against_float64).  FIGURES: see LABBOOK R8.1 -- the six cases passed this bar on an MI355X, but the printed yardstick and
    HIP distances of that run were not kept, so none is quoted here."""
    from fastdiff_amd import lvc_op
    _, gscale, max_norm = case
    shapes = _shapes()
    hp = dict(lr=2e-4, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=weight_decay, max_norm=max_norm)
    p0 = _hash_tensors(77, 1, shapes, 0.1, "cuda")
    grads = [_hash_tensors(77, 10 + s, shapes, gscale, "cuda") for s in range(N_STEPS)]
    p64, m64, v64, norms = _reference_adamw(torch.float64, p0, grads, hp, FROZEN)
    p32, _, _, _ = _reference_adamw(torch.float32, p0, grads, hp, FROZEN)
    for nrm in norms:
        assert max_norm == 0 or nrm > 2 * max_norm or nrm < max_norm / 2, nrm
    P = [p.clone() for p in p0]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    hyper = torch.tensor([hp[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")], dtype=torch.float64, device="cuda")
    st = lvc_op.new_train_state("cuda")
    n_live = sum(p.numel() for i, p in enumerate(P) if i != FROZEN)
    for s in range(N_STEPS):
        lvc_op.adamw_multi([(p, None if i == FROZEN else g, m, v) for i, (p, g, m, v) in enumerate(zip(P, grads[s], M, V))], hyper, st)
        got = lvc_op.read_train_state(st)
        assert (got["iter"], got["applied"], got["skipped"]) == (s + 1, s + 1, 0)
        assert abs(got["grad_norm"] - norms[s]) <= sum_bound(n_live) * norms[s], (s, got["grad_norm"], norms[s])
    assert torch.equal(P[FROZEN], p0[FROZEN]) and not M[FROZEN].any() and not V[FROZEN].any()
    _check_against_float64(f"{case[0]}, weight_decay {weight_decay}", P, p64, p32)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_a_non_finite_gradient_skips_the_step(gc, bad):
    """Two finite steps, one step with a single inf / nan in one gradient, then finite steps again: the bad step writes no p, m or v,
    counts as skipped, advances iter, and the next step uses the un-advanced t and matches float64."""
    from fastdiff_amd import lvc_op
    shapes = _shapes()
    hp = dict(lr=2e-4, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01, max_norm=MAX_NORM)
    p0 = _hash_tensors(77, 1, shapes, 0.1, "cuda")
    grads = [_hash_tensors(77, 10 + s, shapes, G_ABOVE, "cuda") for s in range(4)]
    P = [p.clone() for p in p0]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    hyper = torch.tensor([hp[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")], dtype=torch.float64, device="cuda")
    st = lvc_op.new_train_state("cuda")

    def step(g):
        lvc_op.adamw_multi([(p, None if i == FROZEN else gi, m, v) for i, (p, gi, m, v) in enumerate(zip(P, g, M, V))], hyper, st)

    step(grads[0])
    step(grads[1])
    before = [[t.clone() for t in ts] for ts in (P, M, V)]
    poisoned = [g.clone() for g in grads[2]]
    poisoned[100].view(-1)[poisoned[100].numel() // 2] = bad
    step(poisoned)
    got = lvc_op.read_train_state(st)
    assert (got["iter"], got["applied"], got["skipped"]) == (3, 2, 1), got
    assert not math.isfinite(got["grad_norm"])
    for now, was in zip((P, M, V), before):
        assert all(torch.equal(a, b) for a, b in zip(now, was))
    step(grads[2])
    step(grads[3])
    got = lvc_op.read_train_state(st)
    assert (got["iter"], got["applied"], got["skipped"]) == (5, 4, 1), got
    p64, _, _, _ = _reference_adamw(torch.float64, p0, grads, hp, FROZEN)
    p32, _, _, _ = _reference_adamw(torch.float32, p0, grads, hp, FROZEN)
    _check_against_float64(f"after a skipped step ({bad})", P, p64, p32)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_one_step_end_to_end_against_the_eager_composition(gc, graph):
    """TrainStep.step from a fixed state against: the differentiable forward on the step's x_t and ts, F.mse_loss against its z,
    backward(), float64 clip + AdamW on those gradients.  Gradients bit-equal, loss and parameters to the bars above; the optimizer
    state round-trips through torch.optim.AdamW."""
    dh = schedules.training_hyperparams()
    m = gc.make_model().train()
    twin = gc.make_model().train()          # (the same synthetic weights: a weight-normed module does not deepcopy)
    hp = dict(lr=2e-4, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01, max_norm=1.0)
    ts = fastdiff_amd.TrainStep(m, dh, weight_decay=0.01, seed=1234, graph=graph)
    mel, wav = _batch(gc)
    p0 = [p.detach().clone() for p in m.parameters()]
    loss = ts.step(mel, wav)
    torch.cuda.synchronize()
    assert (ts._graph is not None) == graph
    st = ts.state()
    assert (st["iter"], st["applied"], st["skipped"]) == (1, 1, 0), st
    # the eager composition on the same draw
    twin.zero_grad(set_to_none=True)
    eps = twin((ts.x_t.clone(), mel, ts.steps.clone()))
    loss_e = torch.nn.functional.mse_loss(eps, ts.z)
    loss_e.backward()
    names = [n for n, _ in m.named_parameters()]
    grads = []
    for n, p, q in zip(names, m.parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None), n
        assert p.grad is None or torch.equal(p.grad, q.grad), (n, float((p.grad - q.grad).abs().max()))
        grads.append(q.grad)
    n = eps.numel()
    loss64 = float(((eps.detach().double() - ts.z.double()) ** 2).mean())
    print(f"loss {float(loss):.9g} (eager {float(loss_e):.9g}, float64 {loss64:.12g})")
    assert abs(float(loss) - loss64) <= sum_bound(n) * loss64 and st["loss"] == float(loss)
    p64, m64, v64, norms = _reference_adamw(torch.float64, p0, [grads], hp)
    p32, _, _, _ = _reference_adamw(torch.float32, p0, [grads], hp)
    n_live = sum(g.numel() for g in grads if g is not None)
    assert abs(st["grad_norm"] - norms[0]) <= sum_bound(n_live) * norms[0], (st["grad_norm"], norms[0])
    _check_against_float64(f"one step ({'graph' if graph else 'eager'}), gradient norm {norms[0]:.4f}", list(m.parameters()), p64, p32)
    # state_dict -> torch.optim.AdamW -> state_dict -> TrainStep -> state_dict, bit for bit
    sd = ts.state_dict()
    opt = torch.optim.AdamW(twin.parameters(), lr=1.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 2e-4 and opt.param_groups[0]["betas"] == (0.9, 0.98) and opt.param_groups[0]["weight_decay"] == 0.01
    back = opt.state_dict()
    other = fastdiff_amd.TrainStep(twin, dh, lr=1.0, graph=False)
    other.load_state_dict(back)
    sd2 = other.state_dict()
    assert sd2["param_groups"] == sd["param_groups"] and list(sd2["state"]) == list(sd["state"]) == list(range(len(names)))
    for i in sd["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][i][k].cpu(), back["state"][i][k].cpu()) and torch.equal(sd["state"][i][k].cpu(), sd2["state"][i][k].cpu()), (i, k)
        assert float(sd["state"][i]["step"]) == 1.0
    assert other.state()["applied"] == 1 and other.hyper["lr"] == 2e-4
    # set_lr reaches the device
    ts.set_lr(1e-5)
    assert float(ts._hyper_dev[0]) == 1e-5


@pytest.mark.gpu
def test_theta_timestep_loss_with_device_noise(gc):
    """noise_source="device": the loss of the step's own draw, under autograd and under no_grad; the default path is untouched."""
    from fastdiff_amd import lvc_op
    dh = schedules.training_hyperparams()
    m = gc.make_model().train()
    mel, wav = _batch(gc)
    loss = fastdiff_amd.theta_timestep_loss(m, (mel, wav), dh, noise_source="device", seed=9, iteration=4)
    loss.backward()
    x_t, z, steps = lvc_op.train_draw(wav, dh["alpha"].cuda(), dh["T"], seed=9, iteration=4)
    eps = m((x_t, mel, steps))
    want = float(((eps.detach().double() - z.double()) ** 2).mean())
    assert abs(float(loss.detach()) - want) <= sum_bound(eps.numel()) * want
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    m.eval()
    with torch.no_grad():
        l2, x0 = fastdiff_amd.theta_timestep_loss(m, (mel, wav), dh, reverse=True, noise_source="device", seed=9, iteration=4)
    # (the inference kernels' eps is within 2e-5 of the training path's, tests/test_gpu_parity.py: 1e-3 of a loss of order 1 is far outside that)
    assert abs(float(l2) - want) <= 1e-3 * want and x0.shape == wav.shape and torch.isfinite(x0).all()
    l3 = fastdiff_amd.theta_timestep_loss(m, (mel, wav), dh, noise_source="device", seed=9, iteration=5)
    assert float(l3) != float(l2)
