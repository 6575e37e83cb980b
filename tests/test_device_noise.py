"""The on-device noise (Philox4x32-10 + Box-Muller, fdk::philox_normal4) against its host twin oracle/philox.py.

Every shipped call pattern leaves x_T and noise at None, so x_T and every z_k are drawn on the device.  The CPU tests pin the twin to
the published Random123 known-answer vectors, to the float32 uniform mapping's end values and to the distribution conditions; the GPU
tests pin every kernel that draws to the twin, element by element, and the default call (nothing injected) to the float64 oracle.

Reading a draw without rounding: with x_T = 0 injected and rows of c_eps = 0, c_div = 1, add_noise = 1 whose sigma is 1 at executed
step k and 0 elsewhere, x is exactly 0 up to step k and exactly z_k after it (the network's eps is multiplied by 0).  x_T itself is the
first entry of return_sequence=True with x_T = None.

The bar, per element:  |device - twin_f64| <= N_ULP * 2^-24 * |twin_f64| + 1e-9,  |z| <= 5.887 and finite;  and over the pooled
elements of each test the 99.9th percentile of the distance in units of 2^-24 * |twin| is at most P999_ULP.
Measured on an MI355X over 3 * 2^22 = 12.6 M draws (B = 4, T = 1024; seeds 1234, 2^32 + 7, 2^63 + 7, 99; x_T, z_0 and z_3 of N = 4;
flat and with stream ids that set both halves of the id; LABBOOK R7.1): worst distance 4.46, 99.9th percentile 2.852, median 0.547
(units of 2^-24 * |twin|; 34 draws above 4, none above 8).  N_ULP = 9 and P999_ULP = 6 are twice those, rounded up; the issue's caps are
16 and 8.  The distance is that of correctly-rounded-or-nearly logf, sqrtf, sincosf and one multiply: no approximate math function.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox   # noqa: E402
import synth    # noqa: E402

MEASURED_WORST, MEASURED_P999 = 4.46, 2.852       # MI355X, 12.6 M draws (above)
N_ULP = 9                                         # ceil(2 * MEASURED_WORST)
P999_ULP = 6                                      # ceil(2 * MEASURED_P999)
LOOP_TOL = 1e-4          # tests/test_gpu_parity.py: N <= 8 loop against the float64 oracle


# ------------------------------------------------------------------------------------------------------------------ CPU: the twin
def test_philox4x32_10_known_answer_vectors():
    """The three Random123 known-answer vectors of Philox4x32-10 (counter words, key words -> output words)."""
    pi = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    for inp, want in (((0,) * 6, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                      ((0xFFFFFFFF,) * 6, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                      (pi, (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = tuple(int(w) for w in philox.philox4x32_10(*inp))
        assert got == want, ([hex(w) for w in got], [hex(w) for w in want])
    # arrays broadcast: the three vectors in one call
    cols = [np.array([0, 0xFFFFFFFF, pi[j]], np.uint64) for j in range(6)]
    out = philox.philox4x32_10(*cols)
    assert [int(w[2]) for w in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    assert [int(w[0]) for w in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_uniform_mapping_end_values_and_normal_bound():
    """u = ((float)(r >> 8) + 0.5f) * 2^-24 in float32: the sum has 25 significant bits from r >> 8 = 2^23 on and is rounded to even, so
    u reaches exactly 1.0 (the draw is then 0) and never 0; the smallest u is 2^-25, which bounds |z| by sqrt(50 ln 2) = 5.887."""
    r = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x800001FF, 0xFFFFFEFF, 0xFFFFFFFF], np.uint64)
    u = philox.u_from_word(r)
    assert u.dtype == np.float32
    want = [2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25,
            (2 ** 24 - 1) * 2.0 ** -25,             # (2^23 - 1) + 0.5: 24 bits, exact
            0.5,                                    # 2^23 + 0.5 -> tie -> even: 2^23
            (2 ** 23 + 2) * 2.0 ** -24,             # 2^23 + 1 + 0.5 -> tie -> even: 2^23 + 2
            (2 ** 24 - 2) * 2.0 ** -24,             # 2^24 - 2 + 0.5 -> tie -> even: 2^24 - 2
            1.0]                                    # 2^24 - 1 + 0.5 -> tie -> even: 2^24
    assert [float(v) for v in u] == want
    ends = np.array([2.0 ** -25, 0.5, 1.0, (2 ** 24 - 1) * 2.0 ** -25], np.float32)
    uu = np.stack(np.meshgrid(ends, ends, ends, ends, indexing="ij"), -1).reshape(-1, 4)
    zz = philox.normal4_from_uniforms(uu)
    sup = float(np.sqrt(50.0 * np.log(2.0)))                                        # 5.8870501...
    assert philox.Z_MAX == 5.887 and 0.0 < sup - philox.Z_MAX < 6e-5
    assert np.isfinite(zz).all() and float(np.abs(zz).max()) <= sup * (1 + 1e-15)
    # 5.887 is sqrt(50 ln 2) to four figures: only the corner u0 = 2^-25 with |cos| = 1 to within 1e-5 (all four end values of u1 are
    # such angles; about 2^-24 * 3e-3 per draw) lies in the 5e-5 between the two -- the cosine components, never the sine ones
    over = np.abs(zz) > philox.Z_MAX
    assert over[:, 0].any() and over[:, 2].any() and not over[:, 1].any() and not over[:, 3].any()
    assert np.all(uu[over[:, 0], 0] == ends[0]) and np.all(uu[over[:, 2], 2] == ends[0])
    assert np.all(zz[uu[:, 0] == 1.0][:, :2] == 0.0) and np.all(zz[uu[:, 2] == 1.0][:, 2:] == 0.0)     # ln 1 = 0


def test_every_input_word_reaches_every_output():
    """Changing one bit of any single input -- seed low / high word, stream, uid low / high word, idx4 low / high word -- changes all
    four output words and all four uniforms (the twin's own argument plumbing)."""
    base = dict(seed=(0x12345678 << 32) | 0x9ABCDEF0, stream=5, idx4=(3 << 32) | 77, uid=(0x0BADF00D << 32) | 0xC0FFEE)
    w0 = [int(w) for w in philox.words(**base)]
    u0 = philox.uniforms(**base)
    seen = {tuple(w0)}
    for name, bit in (("seed", 0), ("seed", 32), ("seed", 63), ("stream", 0), ("stream", 31), ("uid", 0), ("uid", 32), ("uid", 63),
                      ("idx4", 0), ("idx4", 32), ("idx4", 63)):
        arg = dict(base)
        arg[name] ^= 1 << bit
        w = [int(x) for x in philox.words(**arg)]
        assert all(a != b for a, b in zip(w, w0)), (name, bit)
        assert np.all(philox.uniforms(**arg) != u0), (name, bit)
        assert tuple(w) not in seen or (name, bit) == ("idx4", 32), (name, bit)     # (idx4 bit 32 = uid bit 0: below)
        seen.add(tuple(w))
    # idx4's high word and uid's low word share counter word 1 by XOR (fd_device.h), so (1, 0) and (0, 1) are the same draw: positions
    # stay below 2^32 float4s (2^34 samples per utterance) for ids to be distinct streams; uid's high word has a counter word of its own
    assert [int(w) for w in philox.words(1, 2, 1 << 32, 0)] == [int(w) for w in philox.words(1, 2, 0, 1)]
    assert [int(w) for w in philox.words(1, 2, 0, 1 << 32)] != [int(w) for w in philox.words(1, 2, 0, 0)]


def test_layout_helpers_index_convention():
    """x_T() / z(): flat index over the batch without ids (a float4 straddles two utterances when L % 4 != 0), the index inside the
    utterance (+ window offset) and the id in the counter with ids."""
    seed, B, L = 99, 3, 150
    flat = philox.z(seed, 2, B, L)
    assert flat.shape == (B, 1, L)
    q = philox.normal4_f64(seed, 2, np.arange((B * L + 3) // 4, dtype=np.uint64)).reshape(-1)
    for b, t in ((0, 0), (0, 149), (1, 0), (1, 1), (1, 2), (2, 149)):
        i = b * L + t
        assert flat[b, 0, t] == q[i] == philox.normal4_f64(seed, 2, i >> 2)[i & 3]
    ids = [7, (1 << 63) + 5, 1 << 32]
    per = philox.x_T(seed, B, L, uids=ids)
    for b in range(B):
        assert np.array_equal(per[b], philox.x_T(seed, 1, L, uids=[ids[b]])[0])                  # independent of the batch position
        assert per[b, 0, 149] == philox.normal4_f64(seed, 0xFFFFFFFF, 149 >> 2, ids[b])[149 & 3]
    whole = philox.z(seed, 1, 1, 4096, uids=[9])
    win = philox.z(seed, 1, 2, 1024, uids=[9, 9], offs=[256, 512])                                # windows at samples 1024 and 2048
    assert np.array_equal(win[0, 0], whole[0, 0, 1024:2048]) and np.array_equal(win[1, 0], whole[0, 0, 2048:3072])
    assert np.array_equal(philox.x_T(seed, 2, 8), philox.z(seed, 0xFFFFFFFF, 2, 8))


def _ks_sqrt_n(v):
    """Kolmogorov-Smirnov statistic against N(0,1), times sqrt(n)."""
    s = torch.sort(torch.from_numpy(np.ascontiguousarray(v.reshape(-1)))).values
    cdf = torch.special.ndtr(s)
    n = s.numel()
    i = torch.arange(1, n + 1, dtype=torch.float64)
    d = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    return d * np.sqrt(n)


def _corr_sqrt_n(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    return float(np.corrcoef(a, b)[0, 1] * np.sqrt(a.size))


def test_reference_distribution_conditions():
    """Conditions on the twin (the device inherits them through the element-wise tests below): seed 1234, 2^20 float4s = 4.19 M normals
    per stream.  KS statistic * sqrt(n) < 1.95 (the 0.1 % critical value); correlation * sqrt(n) in [-4, 4] between the x_T stream and
    step 0, between consecutive steps, between ids 0 and 1, between seeds s and s + 2^32, and at lags 1, 2, 3, 4, 64 inside one stream.
    Fixed seeds: deterministic."""
    seed, n4 = 1234, 1 << 20
    L = 4 * n4
    x = philox.x_T(seed, 1, L)
    assert x.dtype == np.float64 and np.isfinite(x).all() and float(np.abs(x).max()) <= philox.Z_MAX
    figures = {"ks": _ks_sqrt_n(x)}
    z0, z1, z7, z8 = (philox.z(seed, k, 1, L) for k in (0, 1, 7, 8))
    figures["xT|z0"] = _corr_sqrt_n(x, z0)
    figures["z0|z1"] = _corr_sqrt_n(z0, z1)
    figures["z7|z8"] = _corr_sqrt_n(z7, z8)
    figures["z0|z8"] = _corr_sqrt_n(z0, z8)
    figures["uid0|uid1"] = _corr_sqrt_n(philox.x_T(seed, 1, L, uids=[0]), philox.x_T(seed, 1, L, uids=[1]))
    figures["uid0|uid2^32"] = _corr_sqrt_n(x, philox.x_T(seed, 1, L, uids=[1 << 32]))
    figures["seed|seed+2^32"] = _corr_sqrt_n(x, philox.x_T(seed + (1 << 32), 1, L))
    assert np.array_equal(x, philox.x_T(seed, 1, L, uids=[0]))                        # one utterance from 0: id 0 is the flat form
    flat = x.reshape(-1)
    for lag in (1, 2, 3, 4, 64):
        figures[f"lag{lag}"] = _corr_sqrt_n(flat[:-lag], flat[lag:])
    figures["ks_z8"] = _ks_sqrt_n(z8)
    print("twin, seed 1234, 2^22 normals per stream:", json.dumps({k: round(v, 3) for k, v in figures.items()}))
    assert figures["ks"] < 1.95 and figures["ks_z8"] < 1.95, figures
    for k, v in figures.items():
        if not k.startswith("ks"):
            assert -4.0 <= v <= 4.0, (k, figures)
    for v in (x, z0):                                                                  # moments, far tighter than the GPU statistics test
        assert abs(v.mean()) < 4.0 / np.sqrt(L) and abs(v.var() - 1.0) < 4.0 * np.sqrt(2.0 / L) and abs((v ** 4).mean() - 3.0) < 4.0 * np.sqrt(96.0 / L)


# ------------------------------------------------------------------------------------------------------------------ GPU: the device
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def sched():
    return load_golden("schedule")


class Pool:
    """The distances of one test's comparisons, in units of 2^-24 * |twin|, for the bulk (99.9th percentile) bound."""

    def __init__(self):
        self.d = []

    def check(self, dev, ref, tag):
        """dev: float32 tensor / array from the device; ref: the twin's float64 array of the same shape.  Whole tensors, every element."""
        dev = np.asarray(dev.detach().cpu().numpy() if torch.is_tensor(dev) else dev)
        assert dev.dtype == np.float32 and dev.shape == ref.shape and ref.dtype == np.float64, (tag, dev.dtype, dev.shape, ref.shape)
        d64 = dev.astype(np.float64)
        assert np.isfinite(d64).all(), tag
        assert float(np.abs(d64).max()) <= philox.Z_MAX, (tag, float(np.abs(d64).max()))
        err = np.abs(d64 - ref)
        unit = 2.0 ** -24 * np.abs(ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = np.where(err <= 1e-9, 0.0, (err - 1e-9) / unit)                     # a twin of exactly 0 admits 1e-9 only
        self.d.append(dist.reshape(-1))
        worst = float(dist.max())
        print(f"  {tag}: {dist.size} draws, worst {worst:.3f} x 2^-24 |twin|, max |z| {float(np.abs(d64).max()):.3f}")
        bad = np.argwhere(err > N_ULP * unit + 1e-9)
        assert bad.size == 0, (tag, f"{len(bad)} of {dist.size} elements outside {N_ULP} ulp; first at {bad[:8].tolist()}, worst {worst:.3g}")
        return worst

    def finish(self, tag):
        d = np.concatenate(self.d)
        p = float(np.percentile(d, 99.9))
        print(f"{tag}: pooled {d.size} draws, worst {float(d.max()):.3f}, 99.9th percentile {p:.3f} (x 2^-24 |twin|)")
        assert N_ULP == int(np.ceil(2 * MEASURED_WORST)) <= 16 and P999_ULP == int(np.ceil(2 * MEASURED_P999)) <= 8
        assert p <= P999_ULP, (tag, p)
        return float(d.max()), p


def probe_rows(N, k):
    """Rows whose result is exactly z_k when x_T = 0: c_eps = 0, c_div = 1, add_noise = 1 everywhere, sigma = 1 at executed step k only."""
    return [{"t": 190.0 - 9.5 * j, "c_eps": 0.0, "c_div": 1.0, "sigma": 1.0 if j == k else 0.0, "c1": 1.0, "c2": 0.0, "c3": 0.0,
             "add_noise": 1} for j in range(N)]


def read_z(m, mel, N, k, seed, **kw):
    """z_k [B,1,L] of a sample() call as the device drew it, bit for bit (module docstring); asserts the trajectory around it."""
    B, L = mel.shape[0], mel.shape[-1] * m.hop_length
    with torch.no_grad():
        seq = m.sample(mel, probe_rows(N, k), x_T=torch.zeros(B, 1, L, device=mel.device), seed=seed, return_sequence=True, **kw)
    seq = torch.stack(list(seq))
    lens = kw.get("lens")
    valid = torch.ones(B, 1, L, dtype=torch.bool, device=mel.device)
    if lens is not None:
        for b, t in enumerate(lens):
            valid[b, :, t * m.hop_length:] = False
    assert torch.isfinite(seq[:, valid]).all(), "a non-finite eps would show as NaN (0 * inf, 0 * nan)"
    for j in range(k + 1):
        assert not seq[j][valid].any(), (k, j)                       # exactly 0 until step k has run
    for j in range(k + 2, N + 1):
        assert torch.equal(seq[j][valid], seq[k + 1][valid]), (k, j)   # and exactly z_k after it
    return seq[k + 1]


def read_x_T(m, mel, seed, **kw):
    """x_T [B,1,L] of a sample() call with x_T = None: the first entry of the returned sequence."""
    with torch.no_grad():
        seq = m.sample(mel, probe_rows(1, 0), seed=seed, return_sequence=True, **kw)
    return seq[0]


def mel_of(B, T, seed=41, cond=80):
    return torch.from_numpy(synth.synth_mel(seed, B, T, cond=cond)).cuda()


@pytest.mark.gpu
def test_tuned_path_flat_index_every_step(gc):
    """B = 3, T = 33 (not a multiple of the 32-frame bucket: the library's row length differs from the caller's) and B = 1, T = 1:
    x_T and z_k for N = 4, every k, flat index over the caller's [B, L]."""
    pool = Pool()
    m = gc.make_model()
    for B, T, seed in ((3, 33, 1234), (1, 1, 77)):
        mel, L = mel_of(B, T), T * 256
        pool.check(read_x_T(m, mel, seed), philox.x_T(seed, B, L), f"x_T B={B} T={T}")
        for k in range(4):
            pool.check(read_z(m, mel, 4, k, seed), philox.z(seed, k, B, L), f"z_{k} B={B} T={T}")
    pool.finish("tuned, flat")


@pytest.mark.gpu
@pytest.mark.parametrize("graph,hoist", [("1", "auto"), ("1", "off"), ("0", "auto"), ("0", "off")])
def test_long_schedule_step_index_across_captured_pieces(gc, graph, hoist):
    """N = 19 runs as pieces of 8, 8 and 3 steps with the step index advanced on the device: step 8 (first of the second piece) draws
    stream 8, steps 16 and 17 the remainder piece's -- from the graph and launched one by one, predictor hoisted or per step."""
    pool = Pool()
    m = gc.make_model()
    m.set_option("graph", graph)
    m.set_option("hoist", hoist)
    B, T, seed, N = 2, 9, 4242, 19
    mel = mel_of(B, T)
    for k in (0, 7, 8, 9, 15, 16, 17):
        pool.check(read_z(m, mel, N, k, seed), philox.z(seed, k, B, T * 256), f"N=19 z_{k} graph={graph} hoist={hoist}")
    pool.finish(f"N=19 graph={graph} hoist={hoist}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [7, (1 << 32) + 7, (1 << 63) + 7])
def test_stream_ids_and_seeds_use_both_halves_of_both_words(gc, seed):
    """ids 0, 1, 2^32, 2^32 + 1, 2^63 + 5 in one batch, seeds with bits in the low half, the high half and the top bit; permuting the
    batch permutes the result."""
    pool = Pool()
    m = gc.make_model()
    ids = [0, 1, 1 << 32, (1 << 32) + 1, (1 << 63) + 5]
    B, T = len(ids), 3
    mel, L = mel_of(B, T), T * 256
    x = read_x_T(m, mel, seed, stream_ids=ids)
    pool.check(x, philox.x_T(seed, B, L, uids=ids), "x_T ids")
    zs = [read_z(m, mel, 4, k, seed, stream_ids=ids) for k in (0, 2)]
    for k, zk in zip((0, 2), zs):
        pool.check(zk, philox.z(seed, k, B, L, uids=ids), f"z_{k} ids")
    perm = [3, 0, 4, 2, 1]
    pmel = mel[perm].contiguous()
    pids = [ids[p] for p in perm]
    assert torch.equal(read_x_T(m, pmel, seed, stream_ids=pids), x[perm])
    assert torch.equal(read_z(m, pmel, 4, 2, seed, stream_ids=pids), zs[1][perm])
    pool.finish(f"stream ids, seed {seed:#x}")


@pytest.mark.gpu
def test_ragged_batch_draws(gc):
    """lens = [33, 5, 20], with and without stream ids: inside each valid length the draws are those of the full [B, L] layout."""
    pool = Pool()
    m = gc.make_model()
    lens, seed = [33, 5, 20], 31337
    B, T = 3, 33
    mel, L = mel_of(B, T), T * 256
    for b, t in enumerate(lens):
        mel[b, :, t:] = 0.0
    for ids in (None, [11, 1 << 40, 13]):
        kw = dict(lens=lens) if ids is None else dict(lens=lens, stream_ids=ids)
        got = [("x_T", read_x_T(m, mel, seed, **kw), philox.x_T(seed, B, L, uids=ids))]
        got += [(f"z_{k}", read_z(m, mel, 4, k, seed, **kw), philox.z(seed, k, B, L, uids=ids)) for k in (0, 3)]
        for name, dev, ref in got:
            for b, t in enumerate(lens):
                pool.check(dev[b, :, : t * 256], ref[b, :, : t * 256], f"{name} ids={ids is not None} utterance {b} ({t} frames)")
    pool.finish("ragged")


@pytest.mark.gpu
@pytest.mark.parametrize("option", [None, ("fuse_final", "0"), ("fuse_advance", "0"), ("kernels", "naive")])
def test_every_kernel_that_draws(gc, option):
    """The update fused into the last LVC layer (default), the stand-alone update kernel (fuse_final = 0), the per-step bookkeeping
    launch (fuse_advance = 0) and the naive kernel set, each on a fresh handle, each against the twin; with k_init_noise for x_T."""
    pool = Pool()
    m = gc.make_model()
    if option:
        m.set_option(*option)
    seed, B, T = 2024, 2, 33
    mel, L = mel_of(B, T), T * 256
    ids = [5, (1 << 33) + 1]
    pool.check(read_x_T(m, mel, seed), philox.x_T(seed, B, L), f"{option} x_T")
    pool.check(read_x_T(m, mel, seed, stream_ids=ids), philox.x_T(seed, B, L, uids=ids), f"{option} x_T ids")
    for k in (0, 1, 3):
        pool.check(read_z(m, mel, 4, k, seed), philox.z(seed, k, B, L), f"{option} z_{k}")
        pool.check(read_z(m, mel, 4, k, seed, stream_ids=ids), philox.z(seed, k, B, L, uids=ids), f"{option} z_{k} ids")
    pool.finish(f"option {option}")


@pytest.mark.gpu
def test_windowed_synthesis_draws_at_the_utterances_positions(gc):
    """sample_long(seed, stream_id=9, window_frames=32) at T = 100: four windows, three of them with a non-zero position offset, give
    the z_k of the whole utterance."""
    pool = Pool()
    m = gc.make_model()
    seed, T, N = 555, 100, 4
    mel, L = mel_of(1, T), T * 256
    for k in range(N):
        with torch.no_grad():
            y = m.sample_long(mel, probe_rows(N, k), x_T=torch.zeros(1, 1, L, device="cuda"), seed=seed, stream_id=9, window_frames=32)
        pool.check(y, philox.z(seed, k, 1, L, uids=[9]), f"sample_long z_{k}")
    pool.finish("windows")


CFG_B = dict(inner_channels=8, cond_channels=40, upsample_ratios=[2, 5, 3], lvc_layers_each_block=3, lvc_kernel_size=5, kpnet_hidden_channels=32,
             kpnet_conv_size=5, diffusion_step_embed_dim_in=64, diffusion_step_embed_dim_mid=256, diffusion_step_embed_dim_out=128)


@pytest.mark.gpu
def test_generic_path_draws(gc):
    """Another architecture (hop = 30) runs g_init_noise / g_update, the scalar twins: T = 5 (L = 150, L % 4 = 2: in the flat form a
    float4 straddles two utterances, with ids the last float4 of an utterance is half used) and T = 4, flat and with ids."""
    import fastdiff_amd
    pool = Pool()
    m = fastdiff_amd.FastDiff(**CFG_B)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(21, CFG_B).items()}, strict=True)
    m = m.cuda().eval()
    assert m.hop_length == 30
    seed, B = (1 << 32) + 99, 3
    ids = [4, (1 << 63) + 5, 1 << 32]
    for T in (5, 4):
        mel, L = mel_of(B, T, cond=40), T * 30
        for uids in (None, ids):
            kw = {} if uids is None else dict(stream_ids=uids)
            pool.check(read_x_T(m, mel, seed, **kw), philox.x_T(seed, B, L, uids=uids), f"generic T={T} ids={uids is not None} x_T")
            for k in range(4):
                pool.check(read_z(m, mel, 4, k, seed, **kw), philox.z(seed, k, B, L, uids=uids), f"generic T={T} ids={uids is not None} z_{k}")
    pool.finish("generic")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("ids", [None, [3, (1 << 32) + 8]])
def test_default_call_without_injected_noise_against_the_oracle(gc, sched, oracle64, N, ids):
    """model.sample(mel, rows, seed=s[, stream_ids]) with nothing injected, B = 2, T = 37, against the float64 oracle fed the twin's
    x_T and z rounded to float32: the default call pattern meets the oracle.  The twin's draws differ from the device's by a few ulp
    times sigma < 1, far below the loop tolerance."""
    m = gc.make_model()
    B, T, seed = 2, 37, 20240607
    L = T * 256
    mel = synth.synth_mel(63, B, T)
    rows, table = gc.table_rows(sched, N)
    kw = {} if ids is None else dict(stream_ids=ids)
    with torch.no_grad():
        y = m.sample(torch.from_numpy(mel).cuda(), rows, seed=seed, **kw)
    x_T = philox.x_T(seed, B, L, uids=ids).astype(np.float32)
    z = np.zeros((N, B, 1, L), np.float32)                      # z[n] is added after reverse index n = N - 1 - k (none after n = 0)
    for k in range(N - 1):
        z[N - 1 - k] = philox.z(seed, k, B, L, uids=ids).astype(np.float32)
    assert np.array_equal(gc.exec_order_noise(z)[0], philox.z(seed, 0, B, L, uids=ids).astype(np.float32))
    y_ref = oracle64.sample(mel, table, x_T, z)
    d = gc.maxdiff(y.cpu().numpy(), y_ref)
    print(f"default call N={N} ids={ids}: max|d| against the float64 oracle {d:.3e}, peak {float(np.abs(y_ref).max()):.3f}")
    assert np.isfinite(y_ref).all() and float(np.abs(y_ref).max()) > 0.1
    assert d < LOOP_TOL
