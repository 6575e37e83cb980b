"""The non-negative mel inversion on the device (fd_nnls_default_iters / fd_nnls_step_bound / fd_mel_to_linear_nnls,
griffin_lim.mel_to_linear_nnls, FastDiff.mel_to_linear(inversion="nnls") / griffin_lim_mel(inversion="nnls"),
infer.synthesize_griffin_lim(inversion=), --gl_inversion / --nnls_iters) against the oracle tests/nnls_ref.py: the header's iteration in
float64, the same iteration with every rounding in float32, and scipy.optimize.nnls for the exact optimum.

Inputs (nnls_ref.mels): "cone" (40 frames, the bank applied to |STFT| of a harmonic-plus-noise signal: a non-negative preimage exists),
"noisy" (cone times 10^(0.1 N(0, 1)); with independent noise per band 23 of its 40 frames keep a preimage, the others have an optimum of
up to 2.6e-2 of || g ||), "random" (24 frames of 10^U(-4, 0.5): none, the optimum is up to 0.13), "floor" (log10 = -6).

Bars.  No bar is tuned on the device: each is a multiple of what the float32 emulation of the same iteration does on the same input.
  * n_iters = 0: torch.equal to fd_mel_to_linear.
  * trajectories (n_iters 1, 2, 4): |amp - x_f64| per element, relative to the frame's largest amplitude, <= 10 times the emulation's
    own deviation from float64 (1.5e-7 .. 2.4e-7 here).  The margin is for a different but fixed summation order and for exp10f / expf
    against the float64 power rounded once (an ulp of g).  Measured on the device: 1.0 .. 1.4 times the emulation's.
  * 128 iterations: x itself drifts in the bank's null space (3e-5 between float32 and float64 numpy) and is not compared.  Its image:
    || A (amp - x_f64) || / || g || per frame <= 20 times the emulation's largest (6e-8 on cone, 1.1e-7 on noisy).  The residual
    recomputed on the host in float64 from the written amplitudes, per frame, <= 20 times max(the emulation's on that frame, the
    emulation's float32 floor = its largest residual over the frames that have a preimage: 6.2e-8 on cone), and its median over the
    frames <= 1 / 100 of the median of the pseudo-inverse path's (3.0e-2 on cone, 4.0e-2 on noisy).
  * 512 iterations on "random": residual minus scipy's optimum, per frame <= 2 times the float64 oracle's own largest gap (1.5e-4) plus
    20 times the float32 floor.
  * the record: resid and norm within 1e-10 relative of a float64 recomputation from the written amplitudes and from g AS THE DEVICE
    FORMED IT -- read back exactly through the pseudo-inverse path with a selection matrix for P -- on "random", where the residual is
    a tenth of || g || (on "cone" it is 1e-7 of it and the recomputation's own rounding, 1e-15 of || g ||, would be 1e-8 of the figure).
"""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import _capi, infer
from fastdiff_amd import griffin_lim as gl
import nnls_ref as ref

NEW = ("fd_nnls_default_iters", "fd_nnls_step_bound", "fd_mel_to_linear_nnls")
TILE = gl.NNLS_FRAME_TILE
BORDERS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
RAGGED = (37, 5, 18)
TIMES_TRAJ, TIMES_IMAGE, BAR_RECORD, BAR_ORACLE_GAP = 10.0, 20.0, 1e-10, 1e-3


@functools.lru_cache(maxsize=None)
def L_of(bank_id="default", variant="pwg"):
    return ref.step_bound(ref.bank(bank_id, variant))


@functools.lru_cache(maxsize=None)
def oracle(kind, n_iters, dtype="f8", bank_id="default", variant="pwg"):
    """x_n [513, T] of the restatement, float64 or the float32 emulation; computed once, shared, never changed."""
    x = ref.solve(ref.bank(bank_id, variant), ref.bank_pinv(bank_id, variant), ref.g_of(ref.mels(kind, variant, bank_id), variant), n_iters,
                  L_of(bank_id, variant), np.float64 if dtype == "f8" else np.float32)
    x.setflags(write=False)
    return x


def case(kind, bank_id="default", variant="pwg"):
    return ref.bank(bank_id, variant), ref.bank_pinv(bank_id, variant), ref.g_of(ref.mels(kind, variant, bank_id), variant)


def traj_deviation(got, x64):
    """max over the frames of max_k |got - x64| / max_k x64"""
    return float((np.abs(np.asarray(got, np.float64) - x64).max(0) / x64.max(0)).max())


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("bank_id, variant", [("default", "pwg"), ("default", "tacotron"), ("dense", "pwg")])
def test_the_step_bound_lies_above_the_largest_eigenvalue(bank_id, variant):
    fb = ref.bank(bank_id, variant)
    lam = ref.lambda_max(fb)
    L = ct.c_double()
    lib = _capi.load()
    assert lib.fd_nnls_step_bound(fb.ctypes.data, ct.byref(L)) == _capi.FD_OK
    print(f"{bank_id} {variant}: lambda_max {lam:.6g}, L / lambda_max {L.value / lam:.6f}")
    assert lam <= L.value <= 1.02 * lam
    assert abs(L.value - ref.step_bound(fb)) <= 1e-12 * lam and gl.nnls_step_bound(fb) == L.value      # deterministic, and the header's recipe
    assert lib.fd_nnls_step_bound(None, ct.byref(L)) == _capi.FD_ERR_INVALID and b"null bank_80x513" in lib.fd_last_error(None)
    bad = fb.copy()
    bad[1, 2] = np.inf
    assert lib.fd_nnls_step_bound(bad.ctypes.data, ct.byref(L)) == _capi.FD_ERR_INVALID and b"element 515 of bank_80x513" in lib.fd_last_error(None)


def test_the_entry_points_are_declared_exported_and_bound():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    api = open(os.path.join(ROOT, "fastdiff_amd", "csrc", "fd_api_ext.cpp")).read()
    for name in NEW:
        assert re.search(r"FD_API\s+[\w\s\*]+?\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTS and hasattr(lib, name) and re.search(r"\b" + name + r"\(", api), name
    assert len(lib.fd_mel_to_linear_nnls.argtypes) == 12 and len(lib.fd_nnls_step_bound.argtypes) == 2
    for name, mine in (("FD_NNLS_MAX_ITERS", gl.NNLS_MAX_ITERS), ("FD_NNLS_FRAME_TILE", gl.NNLS_FRAME_TILE)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == mine == getattr(_capi, name), name
    assert gl.NNLS_RECORD.itemsize == int(re.search(r"\}\s*fd_nnls;\s*/\*\s*(\d+) bytes", header).group(1)) == 32
    assert gl.NNLS_RECORD.names == ("resid", "norm", "frames", "iters", "status", "reserved")
    assert (gl.NNLS_OK, gl.NNLS_EMPTY, gl.NNLS_NONFINITE) == (ref.OK, ref.EMPTY, ref.NONFINITE) == (0, 1, 2)
    assert re.search(r"FD_NNLS_OK = 0, FD_NNLS_EMPTY = 1, FD_NNLS_NONFINITE = 2", header)
    assert gl.NNLS_STATUS == {0: "OK", 1: "EMPTY", 2: "NONFINITE"}
    assert lib.fd_nnls_default_iters() == gl.nnls_default_iters() == 128 <= gl.NNLS_MAX_ITERS == 4096
    assert callable(gl.mel_to_linear_nnls)
    import inspect
    for fn, names in ((fastdiff_amd.FastDiff.mel_to_linear, ("inversion", "nnls_iters", "lens", "return_record")),
                      (fastdiff_amd.FastDiff.griffin_lim_mel, ("inversion", "nnls_iters")), (infer.synthesize_griffin_lim, ("inversion", "nnls_iters"))):
        p = inspect.signature(fn).parameters
        assert all(n in p for n in names) and p["inversion"].default == "pinv" and p["nnls_iters"].default == 128, fn
    b64, b32 = ref.betas(4)
    t1 = (1 + 5 ** 0.5) / 2                                # t_0 = 1: beta_0 = 0, beta_1 = (t_1 - 1) / t_2
    assert b64[0] == 0.0 and abs(b64[1] - (t1 - 1) / ((1 + (1 + 4 * t1 * t1) ** 0.5) / 2)) < 1e-15 and b32.dtype == np.float32 and (np.diff(b64) > 0).all()


def _refusals():
    ok = dict(mel=True, bank=True, P=True, out=True, B=1, T=5, lens=None, n_iters=3, variant=0, bad=None)
    return (("a null mel", dict(ok, mel=False), b"null mel"), ("a null bank", dict(ok, bank=False), b"null bank_80x513"),
            ("a null pinv", dict(ok, P=False), b"null pinv_513x80"), ("a null amp_out", dict(ok, out=False), b"null amp_out"),
            ("B = 0", dict(ok, B=0), b"B = 0"), ("B = 4097", dict(ok, B=4097), b"B = 4097"), ("T = 0", dict(ok, T=0), b"T = 0"),
            ("T above the cap", dict(ok, T=1048577), b"T = 1048577"), ("n_iters = -1", dict(ok, n_iters=-1), b"n_iters = -1"),
            ("n_iters above the cap", dict(ok, n_iters=4097), b"n_iters = 4097"), ("variant = 2", dict(ok, variant=2), b"unknown variant 2"),
            ("a NaN in the bank", dict(ok, bad="bank"), b"element 7 of bank_80x513"), ("an infinity in P", dict(ok, bad="P"), b"element 7 of pinv_513x80"),
            ("lens[b] > T", dict(ok, lens=[6]), b"lens[0] = 6"), ("lens[b] < 0", dict(ok, lens=[-1]), b"lens[0] = -1"))


def test_refusals_name_the_value_without_a_handle():
    """The arguments are checked before the handle is looked at (host memory stands in for the device pointers, which nothing may
    touch), so every refusal is read through fd_last_error(NULL); with every argument in order the NULL handle itself is refused."""
    lib = _capi.load()
    buf, bad = (ct.c_float * (513 * 80))(), (ct.c_float * (513 * 80))()
    p = ct.addressof(buf)
    for what, c, text in _refusals():
        bad[7] = float("nan") if c["bad"] == "bank" else float("inf")
        lens = None if c["lens"] is None else (ct.c_int64 * len(c["lens"]))(*c["lens"])
        bank = None if not c["bank"] else (ct.addressof(bad) if c["bad"] == "bank" else p)
        P = None if not c["P"] else (ct.addressof(bad) if c["bad"] == "P" else p)
        rc = lib.fd_mel_to_linear_nnls(None, p if c["mel"] else None, c["B"], c["T"], lens, bank, P, c["variant"], c["n_iters"], p if c["out"] else None, None, None)
        msg = lib.fd_last_error(None)
        assert rc == _capi.FD_ERR_INVALID and text in msg and b"fd_mel_to_linear_nnls" in msg, (what, msg)
    for n_iters, lens in ((0, None), (gl.NNLS_MAX_ITERS, (ct.c_int64 * 1)(0))):                # the borders are accepted: only the handle is missing
        assert lib.fd_mel_to_linear_nnls(None, p, 1, 5, lens, p, p, 1, n_iters, p, None, None) == _capi.FD_ERR_INVALID
        assert b"null handle" in lib.fd_last_error(None)


def test_the_oracle_reaches_the_optimum_within_its_own_gap():
    fb, P, g = case("random")
    opt = ref.optimum(fb, g)
    gaps = {}
    for n in (128, 512):
        for dt in ("f8", "f4"):
            gaps[n, dt] = float((ref.residual(fb, ref.amplitudes(oracle("random", n, dt)), g) - opt).max())
    print("random: optimum up to", opt.max(), "gap to it", gaps)
    assert 0.05 < opt.max() < 0.3                                                             # no preimage
    assert -1e-9 <= gaps[512, "f8"] <= gaps[128, "f8"] and gaps[512, "f8"] <= BAR_ORACLE_GAP and gaps[512, "f4"] <= BAR_ORACLE_GAP
    fb, P, g = case("cone")
    r64, r32 = ref.residual(fb, ref.amplitudes(oracle("cone", 128)), g), ref.residual(fb, ref.amplitudes(oracle("cone", 128, "f4")), g)
    pinv_resid = ref.residual(fb, ref.amplitudes(oracle("cone", 0)), g)
    print("cone: residual after 128 iterations", r64.max(), "(float64)", r32.max(), "(float32); pseudo-inverse: median", np.median(pinv_resid))
    assert r64.max() <= 1e-7 and r32.max() <= 3e-7 and np.median(pinv_resid) >= 1e-3         # the float32 floor; the gap the feature closes
    fb, P, g = case("floor")
    assert ref.residual(fb, ref.amplitudes(oracle("floor", 128, "f4")), g).max() <= 3e-7
    # the noisy input as the docstring describes it
    fb, P, g = case("noisy")
    r = ref.residual(fb, ref.amplitudes(oracle("noisy", 512)), g)
    assert (r < 1e-9).sum() >= 20 and r.max() < 0.05


def test_the_command_line_routes_the_inversion(monkeypatch, tmp_path):
    seen = {}

    class Model:
        def cuda(self):
            return self

        def eval(self):
            return self

    def run(model, items, *a, **kw):
        seen["griffin_lim"] = (a, kw)
        return {it["item_name"]: np.zeros(256, np.int16) for it in items}

    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    monkeypatch.setattr(fastdiff_amd, "FastDiff", Model)
    monkeypatch.setattr(infer, "synthesize_griffin_lim", run)
    np.save(tmp_path / "a.npy", np.zeros((5, 80), np.float32))
    base = ["--test_input_dir", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--vocoder", "griffin_lim"]
    infer.main(base)
    a, kw = seen.pop("griffin_lim")
    assert a[0] == 60 and "inversion" not in kw and "nnls_iters" not in kw                # the default passes no new keyword
    infer.main(base + ["--gl_inversion", "pinv"])
    assert "inversion" not in seen.pop("griffin_lim")[1]
    infer.main(base + ["--gl_inversion", "nnls", "--nnls_iters", "32"])
    kw = seen.pop("griffin_lim")[1]
    assert kw["inversion"] == "nnls" and kw["nnls_iters"] == 32
    infer.main(base + ["--gl_inversion", "nnls"])
    kw = seen.pop("griffin_lim")[1]
    assert kw["inversion"] == "nnls" and kw["nnls_iters"] == 128
    infer.main(base + ["--gl_inversion", "nnls", "--nnls_iters", "0"])
    assert seen.pop("griffin_lim")[1]["nnls_iters"] == 0
    for bad in (["--gl_inversion", "lbfgs"], ["--gl_inversion", "nnls", "--nnls_iters", "-1"], ["--gl_inversion", "nnls", "--nnls_iters", "4097"]):
        with pytest.raises(SystemExit):
            infer.main(base + bad)
    assert not seen


class _StubModel:
    """What synthesize_griffin_lim touches, on the CPU: the calls are recorded, the waveform is a ramp per item"""
    hop_length = 256

    def __init__(self):
        self.calls = []

    def griffin_lim_mel(self, mels, lens=None, variant="pwg", **kw):
        self.calls.append(dict(lens=list(lens), variant=variant, **kw))
        wav = torch.zeros(mels.shape[0], 256 * (mels.shape[2] - 1))
        for b, n in enumerate(lens):
            wav[b, : 256 * (n - 1)] = torch.linspace(-1.0, 1.0, 256 * (n - 1))
        return wav

    def peak_normalize_int16(self, wav, valid=None):
        return (wav * 32767).to(torch.int16)


def test_the_baseline_driver_hands_the_inversion_to_the_model(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    rng = np.random.default_rng(0)
    items = [{"item_name": f"u{i}", "mel": torch.from_numpy(rng.standard_normal((t, 80)).astype(np.float32)), "len": t} for i, t in enumerate((9, 4, 6))]
    m = _StubModel()
    infer.synthesize_griffin_lim(m, items, n_iters=3, max_batch=2)
    assert m.calls and all("inversion" not in c and "nnls_iters" not in c for c in m.calls)
    m = _StubModel()
    infer.synthesize_griffin_lim(m, items, n_iters=3, max_batch=2, inversion="nnls", nnls_iters=17)
    assert len(m.calls) == 2 and all(c["inversion"] == "nnls" and c["nnls_iters"] == 17 and c["n_iters"] == 3 for c in m.calls)
    with pytest.raises(ValueError, match="inversion"):
        infer.synthesize_griffin_lim(m, items, inversion="lbfgs")


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.float64)


_SELECT = np.zeros((513, 80), np.float32)
_SELECT[np.arange(80), np.arange(80)] = 1.0


def device_g(mel, variant="pwg"):
    """g [80, T] float32 exactly as the kernels form it: the pseudo-inverse path with a selection matrix (a chain of exact zeros and
    one product with 1), for mels whose g is above the floor of 1e-10"""
    return gl.mel_to_linear(dev(mel)[None], _SELECT, variant)[0, :80].cpu().numpy()


def solve_dev(kind, n_iters, bank_id="default", variant="pwg", **kw):
    fb, P, _ = case(kind, bank_id, variant)
    return gl.mel_to_linear_nnls(dev(ref.mels(kind, variant, bank_id))[None], fb, P, variant, n_iters=n_iters, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["pwg", "tacotron"])
def test_zero_iterations_are_the_pseudo_inverse_path_bit_for_bit(model, variant):
    fb, used = model.mel_filterbank(variant)
    assert not used and np.abs(fb - ref.bank("default", variant)).max() <= 1e-7 * fb.max()      # the oracle's default bank is the library's
    for kind in ("cone", "random", "floor"):
        mel = dev(ref.mels(kind, variant))[None]
        want = model.mel_to_linear(mel, variant)
        got, rec = model.mel_to_linear(mel, variant, inversion="nnls", nnls_iters=0, return_record=True)
        assert got.shape == want.shape == (1, 513, mel.shape[2]) and torch.equal(got, want), (variant, kind)
        assert int(rec["status"][0]) == gl.NNLS_OK and int(rec["iters"][0]) == 0 and int(rec["frames"][0]) == mel.shape[2]
        assert torch.equal(gl.mel_to_linear_nnls(mel, fb, gl.pinv(fb, variant), variant, n_iters=0), want)


def check_trajectory(got, kind, n, bank_id="default", variant="pwg"):
    x64 = oracle(kind, n, "f8", bank_id, variant)
    emu = traj_deviation(oracle(kind, n, "f4", bank_id, variant), x64)
    d = traj_deviation(got, ref.amplitudes(x64))
    print(f"{bank_id} {variant} {kind} n_iters {n}: device {d:.3e}, float32 emulation {emu:.3e}, bar {TIMES_TRAJ * emu:.3e}")
    assert d <= TIMES_TRAJ * emu, (kind, n, d, emu)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cone", "random"])
def test_short_trajectories_follow_the_float64_oracle(kind):
    for n in (1, 2, 4):
        check_trajectory(host(solve_dev(kind, n)[0]), kind, n)


def check_image_and_residual(got, kind, n, bank_id="default", variant="pwg", medians=True):
    fb, P, g = case(kind, bank_id, variant)
    x64, x32 = oracle(kind, n, "f8", bank_id, variant), oracle(kind, n, "f4", bank_id, variant)
    img, img_emu = ref.image_gap(fb, got, ref.amplitudes(x64), g), ref.image_gap(fb, x32, x64, g)
    r, r64, r32 = ref.residual(fb, got, g), ref.residual(fb, ref.amplitudes(x64), g), ref.residual(fb, ref.amplitudes(x32), g)
    solved = r64 < 1e-6                                    # the frames that have (numerically) reached a preimage in float64
    floor32 = float(r32[solved].max()) if solved.any() else 0.0
    r_pinv = ref.residual(fb, ref.amplitudes(oracle(kind, 0, "f8", bank_id, variant)), g)
    print(f"{bank_id} {variant} {kind} n_iters {n}: image gap {img.max():.3e} (emulation {img_emu.max():.3e}); residual on the frames with a preimage "
          f"{r[solved].max() if solved.any() else float('nan'):.3e} (emulation's floor {floor32:.3e}), median {np.median(r):.3e}, "
          f"pseudo-inverse median {np.median(r_pinv):.3e}")
    assert (img <= TIMES_IMAGE * img_emu.max()).all(), (kind, img.max(), img_emu.max())
    assert (r <= TIMES_IMAGE * np.maximum(r32, floor32)).all(), (kind, (r / np.maximum(r32, floor32)).max())
    if medians:
        assert np.median(r) <= np.median(r_pinv) / 100.0, (kind, np.median(r), np.median(r_pinv))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cone", "noisy"])
def test_the_image_at_128_iterations(kind):
    amp, rec = solve_dev(kind, 128, return_record=True)
    check_image_and_residual(host(amp[0]), kind, 128)
    assert int(rec["status"][0]) == gl.NNLS_OK and int(rec["iters"][0]) == 128


@pytest.mark.gpu
def test_optimality_at_512_iterations_without_a_preimage():
    fb, P, g = case("random")
    opt = ref.optimum(fb, g)
    gap64 = float((ref.residual(fb, ref.amplitudes(oracle("random", 512)), g) - opt).max())
    fc, _, gc = case("cone")
    floor32 = float(ref.residual(fc, ref.amplitudes(oracle("cone", 128, "f4")), gc).max())
    gap = ref.residual(fb, host(solve_dev("random", 512)[0]), g) - opt
    print(f"random n_iters 512: device gap to the optimum {gap.max():.3e}, float64 oracle's {gap64:.3e}, float32 floor {floor32:.3e}")
    assert (gap <= 2.0 * gap64 + 20.0 * floor32).all() and (gap >= -20.0 * floor32).all()


@pytest.mark.gpu
def test_the_record():
    fb, P, _ = case("random")
    mel = ref.mels("random")
    g = device_g(mel)
    assert np.abs(g - ref.g_of(mel)).max() <= 4e-7 * g.max()                                  # exp10f: within a few ulp of the oracle's
    amp, rec = solve_dev("random", 24, return_record=True)
    resid, norm = ref.record(fb, host(amp[0]), g)
    print(f"record: resid {rec['resid'][0]!r} (recomputed {resid!r}), norm {rec['norm'][0]!r} (recomputed {norm!r})")
    assert abs(rec["resid"][0] - resid) <= BAR_RECORD * resid and abs(rec["norm"][0] - norm) <= BAR_RECORD * norm
    assert (int(rec["frames"][0]), int(rec["iters"][0]), int(rec["status"][0])) == (24, 24, gl.NNLS_OK)
    # a NaN, an infinity and an overflowing mel: NONFINITE, all-floor amplitudes; the neighbours are what they are alone
    batch = np.stack([mel, mel, mel, mel, mel])
    batch[1, 3, 5], batch[2, 79, 23], batch[3, 0, 0] = np.nan, -np.inf, 39.0
    lens = (24, 24, 24, 24, 0)
    got, rec = gl.mel_to_linear_nnls(dev(batch), fb, P, lens=lens, n_iters=24, return_record=True)
    assert rec["status"].tolist() == [gl.NNLS_OK, gl.NNLS_NONFINITE, gl.NNLS_NONFINITE, gl.NNLS_NONFINITE, gl.NNLS_EMPTY]
    assert rec["frames"].tolist() == list(lens) and rec["iters"].tolist() == [24] * 5
    assert np.isnan(rec["resid"][1:]).all() and np.isnan(rec["norm"][1:]).all() and np.isfinite(rec["resid"][0])
    assert torch.equal(got[0], amp[0]) and bool((got[1:] == 1e-10).all())
    assert gl.mel_to_linear_nnls(dev(batch), fb, P, lens=lens, n_iters=24).shape == (5, 513, 24)      # without a record


@pytest.mark.gpu
def test_tile_borders_and_ragged_batches():
    fb, P, _ = case("cone")
    mel = ref.mels("cone")
    long = np.concatenate([mel, mel[:, ::-1]], 1)[:, : max(BORDERS)]                          # 67 frames
    whole = gl.mel_to_linear_nnls(dev(long)[None], fb, P, n_iters=8)
    for T in BORDERS:                                      # a frame's result is a function of that frame alone
        got = gl.mel_to_linear_nnls(dev(long[:, :T])[None], fb, P, n_iters=8)
        assert got.shape == (1, 513, T) and torch.equal(got[0], whole[0, :, :T]), T
    batch = np.full((len(RAGGED), 80, max(RAGGED)), 1e30, np.float32)
    batch[:, ::2] = np.nan                                 # garbage behind each item's frames: never read
    for b, T in enumerate(RAGGED):
        batch[b, :, :T] = mel[:, :T]
    got, rec = gl.mel_to_linear_nnls(dev(batch), fb, P, lens=RAGGED, n_iters=8, return_record=True)
    again = gl.mel_to_linear_nnls(dev(batch), fb, P, lens=RAGGED, n_iters=8)
    assert torch.equal(got, again) and rec["status"].tolist() == [gl.NNLS_OK] * 3 and rec["frames"].tolist() == list(RAGGED)
    for b, T in enumerate(RAGGED):
        solo, solo_rec = gl.mel_to_linear_nnls(dev(mel[:, :T])[None], fb, P, n_iters=8, return_record=True)
        assert torch.equal(got[b, :, :T], solo[0]) and torch.equal(solo[0], whole[0, :, :T]), b
        assert bool((got[b, :, T:] == 1e-10).all()), b
        assert rec["resid"][b] == solo_rec["resid"][0] and rec["norm"][b] == solo_rec["norm"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("bank_id, variant", [("dense", "pwg"), ("dense", "tacotron"), ("default", "tacotron")])
def test_a_callers_bank_and_the_other_variant(bank_id, variant):
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: the bank is set on it
    m.set_mel_filterbank(ref.bank(bank_id, variant), variant)
    fb, used = m.mel_filterbank(variant)
    assert used and np.array_equal(fb, ref.bank(bank_id, variant))
    mel = dev(ref.mels("cone", variant, bank_id))[None]
    check_trajectory(host(m.mel_to_linear(mel, variant, inversion="nnls", nnls_iters=2)[0]), "cone", 2, bank_id, variant)
    amp, rec = m.mel_to_linear(mel, variant, inversion="nnls", return_record=True)
    assert int(rec["status"][0]) == gl.NNLS_OK and int(rec["iters"][0]) == 128
    # (the mel of a mixed-sign bank's |image| has no preimage in general: there the medians say nothing)
    check_image_and_residual(host(amp[0]), "cone", 128, bank_id, variant, medians=bank_id == "default")


@pytest.mark.gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays():
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no table, no scratch yet
    fb = m.mel_filterbank("pwg")[0]
    P = gl.pinv(fb, "pwg")
    a, b = dev(ref.mels("cone"))[None], dev(ref.mels("noisy"))[None]
    T = a.shape[2]
    mel, amp = a.clone(), torch.zeros((1, 513, T), device="cuda")
    rec = torch.zeros((1, gl.NNLS_RECORD.itemsize), device="cuda", dtype=torch.uint8)
    lib, h = m._ready(mel.device)
    args = lambda: (h, mel.data_ptr(), 1, T, None, fb.ctypes.data, P.ctypes.data, 0, 6, amp.data_ptr(), rec.data_ptr(), m._stream(mel.device))      # noqa: E731
    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        mel.mul_(1.0)                                      # (so that the capture is not empty)
        rc = lib.fd_mel_to_linear_nnls(*args())
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a = m.mel_to_linear(a, inversion="nnls", nnls_iters=6)                              # outside: the tables and the scratch buffer
    want_b = m.mel_to_linear(b, inversion="nnls", nnls_iters=6)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, lib.fd_mel_to_linear_nnls(*args()), "fd_mel_to_linear_nnls")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(amp, want_a)
    mel.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(amp, want_b) and int(gl._wave.records(rec, gl.NNLS_RECORD, gl.NNLS_RECORD.names)["status"][0]) == gl.NNLS_OK


@pytest.mark.gpu
def test_end_to_end_through_griffin_lim(model):
    mel = ref.mels("cone")
    batch = np.full((len(RAGGED), 80, max(RAGGED)), -6.0, np.float32)
    for b, T in enumerate(RAGGED):
        batch[b, :, :T] = mel[:, :T]
    d = dev(batch)
    plain, plain_rec = model.griffin_lim_mel(d, lens=RAGGED, seed=3, stream_ids=[7, 8, 9], return_record=True)
    pinv_wav, pinv_rec = model.griffin_lim_mel(d, lens=RAGGED, seed=3, stream_ids=[7, 8, 9], return_record=True, inversion="pinv")
    assert torch.equal(plain, pinv_wav) and np.array_equal(plain_rec["sc"], pinv_rec["sc"])
    wav, rec = model.griffin_lim_mel(d, lens=RAGGED, seed=3, stream_ids=[7, 8, 9], return_record=True, inversion="nnls")
    assert wav.shape == plain.shape and rec["status"].tolist() == [gl.OK] * 3 and np.isfinite(rec["sc"]).all()
    amp, nrec = model.mel_to_linear(d, inversion="nnls", lens=RAGGED, return_record=True)
    assert nrec["status"].tolist() == [gl.NNLS_OK] * 3 and nrec["iters"].tolist() == [128] * 3 and nrec["frames"].tolist() == list(RAGGED)
    # reported, not gated: the log10-mel error of the inverted amplitudes and Griffin-Lim's final sc for both inversions
    fb = ref.bank().astype(np.float64)
    err = {}
    for name, a in (("pinv", model.mel_to_linear(d)), ("nnls", amp)):
        err[name] = max(float(np.abs(np.log10(fb @ host(a[b, :, :T])) - batch[b, :, :T]).max()) for b, T in enumerate(RAGGED))
    print(f"log10-mel error of the inverted amplitudes: pinv {err['pinv']:.3e}, nnls {err['nnls']:.3e}; Griffin-Lim's final sc: pinv "
          f"{pinv_rec['sc'].tolist()}, nnls {rec['sc'].tolist()}; nnls resid {nrec['resid'].tolist()}")
