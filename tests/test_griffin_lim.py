"""Griffin-Lim on the device (fd_gl_samples / fd_gl_default_iters / fd_mel_to_linear / fd_griffin_lim, fastdiff_amd.griffin_lim,
FastDiff.griffin_lim / mel_to_linear / griffin_lim_mel, infer.synthesize_griffin_lim, --vocoder griffin_lim) against the float64 oracle
tests/gl_ref.py, which restates the header's definition in numpy and is itself confirmed here with torch.stft / torch.istft in float64.

Bars.  Inverse transform alone (n_iters = 0, given or Philox angles): |y - y_f64| <= 2e-5 S, S = max_t (1 / 1024) sum_{k < 1024} |C^[k, t]|
-- derived: every sample is four frames' worth of two nested 32-term fmaf chains over float32 table twiddles, over an envelope >= 1.25
(about 224 2^-24 / 1.25 in the worst case).  Measured on the device: at most 1.2e-7 at S = 0.84 (1.43e-7 S), about 140 times below.
Trajectories (fixed point from the true phase, n_iters 1 and 3; random start, n_iters 1 and 2): no honest a-priori bar (where |X| is
near zero the phase is ill-conditioned), so the yardstick is measured on the CPU -- the same loop in float32 through torch.stft /
torch.istft against the float64 restatement on the same inputs -- and the device bar is 10 times that, per case.  Measured: yardsticks
7.7e-8 .. 2.7e-7, the device 8.4e-8 .. 3.4e-7, at most 1.65 times its yardstick (true start, T = 2, n_iters = 3).
Record: sc within 1e-5 of the oracle's sc of the returned waveform (test_spectral.py's bar for the same quantity).  mel_to_linear: |err| <= 1e-5 sum_j |P_kj| g(mel_j) per element (an 80-term chain plus a few ulp of exp10f), plus
1e-17 where the floor is reached: the float32 nearest to 1e-10 lies 3.6e-18 from it.
"""
import ctypes as ct
import functools
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import _capi, infer
from fastdiff_amd import griffin_lim as gl
import gl_ref as ref

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox  # noqa: E402

NEW = ("fd_gl_samples", "fd_gl_default_iters", "fd_mel_to_linear", "fd_griffin_lim")
FRAMES = (2, 3, 4, 5, 9, 37)       # 2 .. 5: fewer than four frames overlap everywhere and both edge envelopes meet; 37: nine frame tiles and one frame
RAGGED = (2, 5, 37)
SEED, UID = 11, 7
BAR_ISTFT, BAR_SC, BAR_MEL, TIMES = 2e-5, 1e-5, 1e-5, 10.0


@functools.lru_cache(maxsize=None)
def signal(T):
    """float64 [256 (T - 1)]: three sinusoids and 0.01 N(0, 1) from a fixed seed, |x| <= 0.5; a shorter one is a prefix of a longer one"""
    n = 256 * (max(FRAMES) - 1)
    t = np.arange(n) / 22050.0
    x = 0.2 * np.sin(2 * np.pi * 220.0 * t) + 0.15 * np.sin(2 * np.pi * 1330.0 * t + 1.0) + 0.1 * np.sin(2 * np.pi * 3700.0 * t + 2.0)
    x = np.clip(x + 0.01 * np.random.default_rng(5).standard_normal(n), -0.5, 0.5)[: 256 * (T - 1)]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def spectrum(T):
    """(A, theta) float32 [513, T] of stft(signal(T))"""
    X = ref.stft(signal(T))
    A, th = np.abs(X).astype(np.float32), np.angle(X).astype(np.float32)
    A.setflags(write=False)
    th.setflags(write=False)
    return A, th


def scale(A):
    """S of the derived bar: max_t (1 / 1024) sum_{k < 1024} |C^[k, t]|"""
    a = np.asarray(A, np.float64)
    return float(((a.sum(0) + a[1:-1].sum(0)) / 1024.0).max())


@functools.lru_cache(maxsize=None)
def start(T, how):
    th = spectrum(T)[1] if how == "true" else ref.philox_angles(SEED, UID, T)
    th.setflags(write=False)
    return th


@functools.lru_cache(maxsize=None)
def oracle(T, how, n_iters):
    """The float64 restatement's waveform; computed once, shared, never changed."""
    y = ref.griffin_lim(spectrum(T)[0], start(T, how), n_iters)
    y.setflags(write=False)
    return y


def torch_loop_f32(A, theta0, n_iters):
    """The same loop in float32 through torch.stft / torch.istft on the CPU: the yardstick of the trajectory tests."""
    A, th = torch.from_numpy(np.array(A)), torch.from_numpy(np.array(theta0))
    w = torch.hann_window(1024, periodic=True, dtype=torch.float32)
    L = 256 * (A.shape[1] - 1)
    ist = lambda C: torch.istft(C, 1024, hop_length=256, win_length=1024, window=w, center=True, length=L)      # noqa: E731
    y = ist(torch.polar(A, th))
    for _ in range(n_iters):
        X = torch.stft(y, 1024, hop_length=256, win_length=1024, window=w, center=True, pad_mode="constant", return_complex=True)
        mag = X.abs()
        y = ist(torch.where(mag > 0, A * X / torch.where(mag > 0, mag, torch.ones_like(mag)), A.to(torch.complex64)))
    return y.numpy()


@functools.lru_cache(maxsize=None)
def yardstick(T, how, n_iters):
    return float(np.abs(torch_loop_f32(spectrum(T)[0], start(T, how), n_iters) - oracle(T, how, n_iters)).max())


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("T", FRAMES)
def test_the_oracles_transforms_are_torchs_in_float64(T):
    x = signal(T)
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    X = ref.stft(x)
    theirs = torch.stft(torch.from_numpy(x.copy()), 1024, hop_length=256, win_length=1024, window=w, center=True, pad_mode="constant", return_complex=True).numpy()
    assert X.shape == theirs.shape == (513, T)
    assert np.abs(X - theirs).max() <= 1e-12
    rng = np.random.default_rng(T)
    C = X * np.exp(1j * rng.uniform(-0.3, 0.3, X.shape))      # not a consistent spectrogram: the overlap-add and the envelope are exercised
    y = ref.istft(C)
    back = torch.istft(torch.from_numpy(C), 1024, hop_length=256, win_length=1024, window=w, center=True, length=256 * (T - 1)).numpy()
    assert y.shape == back.shape == (256 * (T - 1),) and np.abs(y - back).max() <= 1e-12
    assert np.abs(ref.istft(X) - x).max() <= 1e-12            # istft(stft(x)) == x
    assert ref.envelope(T)[512: 512 + 256 * (T - 1)].min() >= 1.25 - 1e-12
    if T >= 5:
        assert abs(ref.envelope(T)[1024] - 1.5) < 1e-12


def test_the_inconsistency_never_rises_in_float64():
    """Griffin and Lim's theorem, which confirms the restatement of the loop; and the room the GPU test's factor 0.5 asks for."""
    for T in (5, 37):
        A = spectrum(T)[0]
        _, scs = ref.griffin_lim(A, start(T, "random"), 32 if T == 37 else 16, trace=True)
        assert all(b <= a + 1e-15 for a, b in zip(scs[:17], scs[1:17])), scs
        if T == 37:
            print(f"float64 sc over 32 iterations at T = 37: sc(0) {scs[0]:.4f} sc(16) {scs[16]:.4f} sc(32) {scs[32]:.4f}")
            assert scs[32] <= 0.25 * scs[0], (scs[0], scs[32])      # at least 2 x room under sc(32) <= 0.5 sc(0)
    x = signal(9)
    assert ref.inconsistency(x, np.abs(ref.stft(x))) < 1e-14     # a consistent spectrogram is a fixed point
    assert np.abs(ref.griffin_lim(*spectrum(9), 3) - x).max() < 1e-5


def test_the_random_start_is_the_documented_philox_keying():
    T = 6
    u = ref.philox_uniforms(SEED, UID, T)
    assert u.shape == (513, T) and u.dtype == np.float32
    for t in range(T):
        for k in (0, 1, 2, 3, 4, 255, 256, 510, 511, 512):
            want = philox.uniforms(SEED, ref.PHILOX_STREAM, 129 * t + k // 4, UID)[k % 4]
            assert u[k, t].tobytes() == np.float32(want).tobytes(), (k, t)
    whole = philox.uniforms(SEED, ref.PHILOX_STREAM, np.arange(129 * T, dtype=np.uint64), UID).reshape(T, 129 * 4)[:, :513].T
    assert whole.tobytes() == np.ascontiguousarray(u).tobytes()
    th = ref.philox_angles(SEED, UID, T)
    assert th.dtype == np.float32 and th.tobytes() == (np.float32(6.283185307179586) * u).astype(np.float32).tobytes()
    assert ref.PHILOX_STREAM == gl.PHILOX_STREAM == 0xFFFFFFF8 and ref.PHILOX_STREAM != philox.X_T_STREAM
    assert not np.array_equal(ref.philox_uniforms(SEED, UID + 1, T), u) and not np.array_equal(ref.philox_uniforms(SEED + 1, UID, T), u)


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for name, mine in (("FD_GL_NFFT", gl.NFFT), ("FD_GL_HOP", gl.HOP), ("FD_GL_BINS", gl.BINS), ("FD_GL_FRAME_TILE", gl.FRAME_TILE), ("FD_GL_MAX_ITERS", gl.MAX_ITERS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == mine, name
    assert int(re.search(r"#define\s+FD_GL_PHILOX_STREAM\s+(0x[0-9A-Fa-f]+)u", header).group(1), 16) == gl.PHILOX_STREAM
    assert gl.RECORD.itemsize == int(re.search(r"\}\s*fd_gl;\s*/\*\s*(\d+) bytes", header).group(1)) == 32
    assert (gl.OK, gl.SHORT, gl.SILENT, gl.NONFINITE) == (ref.OK, ref.SHORT, ref.SILENT, ref.NONFINITE) == (0, 1, 2, 3)
    assert gl.STATUS == {0: "OK", 1: "SHORT", 2: "SILENT", 3: "NONFINITE"}
    assert "griffin_lim" in fastdiff_amd.__all__ and fastdiff_amd.griffin_lim is gl
    assert all(callable(getattr(fastdiff_amd.FastDiff, n)) for n in ("griffin_lim", "mel_to_linear", "griffin_lim_mel"))
    assert callable(infer.synthesize_griffin_lim)
    for frames in (2, 3, 87, 866):
        assert lib.fd_gl_samples(frames) == gl.samples(frames) == ref.samples(frames) == 256 * (frames - 1)
    assert lib.fd_gl_samples(1) == lib.fd_gl_samples(0) == lib.fd_gl_samples(-3) == -1
    with pytest.raises(ValueError):
        gl.samples(1)
    assert lib.fd_gl_default_iters() == gl.default_iters() == 60


def _gl_refusals():
    ok = dict(amp=True, wav=True, rec=True, B=1, T=5, lens=None, n_iters=3, pitch=1024)
    return (("a null amp", dict(ok, amp=False), b"null amp"),
            ("a null wav_out", dict(ok, wav=False), b"null wav_out"),
            ("a null record", dict(ok, rec=False), b"null rec_dev"),
            ("B = 0", dict(ok, B=0), b"B = 0"),
            ("B = 4097", dict(ok, B=4097), b"B = 4097"),
            ("T = 1", dict(ok, T=1, pitch=0), b"T = 1"),
            ("n_iters = -1", dict(ok, n_iters=-1), b"n_iters = -1"),
            ("n_iters above the cap", dict(ok, n_iters=gl.MAX_ITERS + 1), b"n_iters = 10001"),
            ("wav_pitch too small", dict(ok, pitch=1023), b"wav_pitch = 1023"),
            ("lens[b] > T", dict(ok, lens=[6]), b"lens[0] = 6"),
            ("lens[b] < 0", dict(ok, lens=[-1]), b"lens[0] = -1"))


def _gl_call(lib, h, p, case, stream=None):
    lens = None if case["lens"] is None else (ct.c_int64 * len(case["lens"]))(*case["lens"])
    return lib.fd_griffin_lim(h, p if case["amp"] else None, None, case["B"], case["T"], lens, case["n_iters"], 0, None, p if case["wav"] else None,
                              case["pitch"], p if case["rec"] else None, stream)


def _m2l_refusals():
    ok = dict(mel=True, P=True, out=True, B=1, T=5, variant=0, bad=False)
    return (("a null mel", dict(ok, mel=False), b"null mel"), ("a null pinv", dict(ok, P=False), b"null pinv_513x80"),
            ("a null amp_out", dict(ok, out=False), b"null amp_out"), ("B = 0", dict(ok, B=0), b"B = 0"), ("T = 0", dict(ok, T=0), b"T = 0"),
            ("variant = 2", dict(ok, variant=2), b"unknown variant 2"), ("a NaN in P", dict(ok, bad=True), b"element 7 of pinv_513x80"))


def test_refusals_name_the_value_without_a_handle():
    """The arguments are checked before the handle is looked at (host memory stands in for the device pointers, which nothing may
    touch), so every refusal is read through fd_last_error(NULL); with every argument in order the NULL handle itself is refused."""
    lib = _capi.load()
    buf = (ct.c_float * (513 * 80))()
    p = ct.addressof(buf)
    for what, case, text in _gl_refusals():
        assert _gl_call(lib, None, p, case) == _capi.FD_ERR_INVALID, what
        msg = lib.fd_last_error(None)
        assert text in msg and b"fd_griffin_lim" in msg, (what, msg)
    assert _gl_call(lib, None, p, dict(amp=True, wav=True, rec=True, B=1, T=5, lens=[0], n_iters=0, pitch=1024)) == _capi.FD_ERR_INVALID
    assert b"null handle" in lib.fd_last_error(None)
    bad = (ct.c_float * (513 * 80))()
    bad[7] = float("nan")
    for what, case, text in _m2l_refusals():
        P = ct.addressof(bad) if case["bad"] else p
        rc = lib.fd_mel_to_linear(None, p if case["mel"] else None, case["B"], case["T"], P if case["P"] else None, case["variant"],
                                  p if case["out"] else None, None)
        msg = lib.fd_last_error(None)
        assert rc == _capi.FD_ERR_INVALID and text in msg and b"fd_mel_to_linear" in msg, (what, msg)
    assert lib.fd_mel_to_linear(None, p, 1, 5, p, 1, p, None) == _capi.FD_ERR_INVALID and b"null handle" in lib.fd_last_error(None)
    with pytest.raises(ValueError, match="variant"):
        gl.variant_id("nnls")


def _bank(seed=0):
    """a triangular filter bank [80, 513] float32 with overlapping supports, like the front-end's"""
    rng = np.random.default_rng(seed)
    edges = np.sort(rng.uniform(2, 500, 82))
    k = np.arange(513)[None, :]
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    return np.maximum(0.0, np.minimum((k - lo) / (mid - lo), (hi - k) / (hi - mid))).astype(np.float32)


def test_the_pseudo_inverse_is_cached_and_inverts_the_bank_on_its_row_space():
    fb = _bank()
    P = gl.pinv(fb, "pwg")
    assert P.shape == (513, 80) and P.dtype == np.float32 and gl.pinv(fb.copy(), "pwg") is P            # cached per variant
    Pt = gl.pinv(fb, "tacotron")
    assert Pt is not P and np.array_equal(Pt, P) and gl.pinv(fb, "tacotron") is Pt and gl.pinv(fb, "pwg") is P
    other = gl.pinv(_bank(1), "pwg")
    assert other is not P and not np.array_equal(other, P) and gl.pinv(_bank(1), "pwg") is other        # a new bank: computed again
    assert gl.pinv(fb, "tacotron") is Pt
    with pytest.raises(ValueError):
        gl.pinv(fb[:, :512])
    with pytest.raises(ValueError):
        gl.pinv(fb, "nnls")
    rng = np.random.default_rng(3)
    A = fb.astype(np.float64).T @ rng.uniform(0.1, 1.0, (80, 6))                                          # in the bank's row space, positive
    for variant, log in (("pwg", np.log10), ("tacotron", np.log)):
        got, bound = ref.mel_to_linear(log(fb.astype(np.float64) @ A), P, variant)
        assert got.shape == (513, 6) and np.abs(got - np.maximum(A, 1e-10)).max() <= 1e-5 * A.max()      # (P is rounded to float32)
        assert (bound >= np.abs(got) - 1e-9).all()
    floor, _ = ref.mel_to_linear(np.full((80, 2), -30.0), P, "pwg")
    assert (floor == 1e-10).any() and floor.min() == 1e-10


class _StubModel:
    """What synthesize_griffin_lim touches, on the CPU: the calls are recorded, the waveform is a ramp per item"""
    hop_length = 256

    def __init__(self):
        self.calls = []

    def griffin_lim_mel(self, mels, lens=None, variant="pwg", **kw):
        self.calls.append(dict(shape=tuple(mels.shape), lens=list(lens), variant=variant, **kw))
        wav = torch.zeros(mels.shape[0], 256 * (mels.shape[2] - 1))
        for b, n in enumerate(lens):
            wav[b, : 256 * (n - 1)] = torch.linspace(-1.0, 1.0, 256 * (n - 1)) * (b + 1) / 4
        return wav

    def peak_normalize_int16(self, wav, valid=None):
        out = torch.zeros(wav.shape, dtype=torch.int16)
        for b, v in enumerate(valid):
            out[b, :v] = (wav[b, :v] / wav[b, :v].abs().max() * 32767).to(torch.int16)
        return out


def test_the_baseline_driver_uses_every_frame_and_the_items_own_streams(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    rng = np.random.default_rng(0)
    items = [{"item_name": f"u{i}", "mel": torch.from_numpy(rng.standard_normal((t, 80)).astype(np.float32)), "len": t} for i, t in enumerate((9, 1, 4, 12, 6))]
    items[3]["uid"] = 40
    m = _StubModel()
    pcm = infer.synthesize_griffin_lim(m, items, n_iters=7, max_batch=2, seed=5, variant="tacotron")
    assert {k: v.shape for k, v in pcm.items()} == {"u0": (2048,), "u2": (768,), "u3": (2816,), "u4": (1280,)}      # 256 (len - 1); the one-frame item is left out
    assert all(v.dtype == np.int16 and np.abs(v).max() == 32767 for v in pcm.values())
    assert [c["lens"] for c in m.calls] == [[12, 9], [6, 4]] and [c["shape"] for c in m.calls] == [(2, 80, 12), (2, 80, 6)]
    assert [c["stream_ids"] for c in m.calls] == [[40, 0], [4, 2]]
    assert all(c["n_iters"] == 7 and c["seed"] == 5 and c["variant"] == "tacotron" for c in m.calls)
    assert infer.synthesize_griffin_lim(m, [], n_iters=1) == {} and infer.synthesize_griffin_lim(m, items[1:2]) == {}
    with pytest.raises(ValueError, match="wav"):
        infer.synthesize_griffin_lim(m, items, stoi=True)


class _StubGenerator:
    """What synthesize_pwg touches of a ParallelWaveGAN, on the CPU: the calls are recorded, the waveform is a ramp per item"""

    def __init__(self, hop_size=256):
        self.hop_size, self.calls = hop_size, []

    def spec2wav(self, mels, lens=None, **kw):
        self.calls.append(dict(shape=tuple(mels.shape), lens=list(lens), **kw))
        wav = torch.zeros(mels.shape[0], 256 * mels.shape[2])
        for b, n in enumerate(lens):
            wav[b, : 256 * n] = torch.linspace(-1.0, 1.0, 256 * n) * (b + 1) / 4
        return wav


def _five_items():
    rng = np.random.default_rng(0)
    items = [{"item_name": f"u{i}", "mel": torch.from_numpy(rng.standard_normal((t, 80)).astype(np.float32)), "len": t} for i, t in enumerate((9, 1, 4, 12, 6))]
    items[3]["uid"] = 40
    return items


def test_the_neural_baseline_driver_drops_the_last_frame_and_uses_the_items_own_streams(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    items, m, g = _five_items(), _StubModel(), _StubGenerator()
    pcm = infer.synthesize_pwg(m, g, items, max_batch=2, seed=5)
    assert {k: v.shape for k, v in pcm.items()} == {"u0": (2048,), "u2": (768,), "u3": (2816,), "u4": (1280,)}      # 256 (len - 1); the one-frame item is left out
    assert all(v.dtype == np.int16 and np.abs(v).max() == 32767 for v in pcm.values())
    assert [c["lens"] for c in g.calls] == [[11, 8], [5, 3]] and [c["shape"] for c in g.calls] == [(2, 80, 11), (2, 80, 5)]
    assert [c["stream_ids"] for c in g.calls] == [[40, 0], [4, 2]]
    assert all(c["seed"] == 5 for c in g.calls)
    assert infer.synthesize_pwg(m, g, []) == {} and infer.synthesize_pwg(m, g, items[1:2]) == {}
    assert len(g.calls) == 2 and not m.calls


def test_the_neural_baseline_driver_keeps_every_frame_on_request(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    items, g = _five_items(), _StubGenerator()
    pcm = infer.synthesize_pwg(_StubModel(), g, items, max_batch=2, seed=5, drop_last_frame=False)
    assert {k: v.shape for k, v in pcm.items()} == {f"u{i}": (256 * t,) for i, t in enumerate((9, 1, 4, 12, 6))}
    assert all(v.dtype == np.int16 for v in pcm.values())
    assert [c["lens"] for c in g.calls] == [[12, 9], [6, 4], [1]]


def test_the_neural_baseline_driver_refuses_another_hop_and_scores_without_recordings(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    items, g = _five_items(), _StubGenerator(hop_size=300)
    with pytest.raises(ValueError, match=r"300.*256"):
        infer.synthesize_pwg(_StubModel(), g, items)
    with pytest.raises(ValueError, match=r"300.*256"):
        infer.synthesize_pwg(_StubModel(), g, [])                  # refused before the items are looked at
    with pytest.raises(ValueError, match="wav"):
        infer.synthesize_pwg(_StubModel(), _StubGenerator(), items, stoi=True)
    assert not g.calls


def test_the_two_baselines_line_up(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    items = _five_items()
    gl_pcm = infer.synthesize_griffin_lim(_StubModel(), items, n_iters=7, max_batch=2, seed=5)
    pwg_pcm = infer.synthesize_pwg(_StubModel(), _StubGenerator(), items, max_batch=2, seed=5)
    assert list(gl_pcm) == list(pwg_pcm) == ["u3", "u0", "u4", "u2"]                              # the same names, delivered in the same order
    assert {k: v.shape for k, v in gl_pcm.items()} == {k: v.shape for k, v in pwg_pcm.items()}    # with the same sample counts


def test_the_command_line_routes_the_vocoder(monkeypatch, tmp_path):
    seen = {}

    class Model:
        def cuda(self):
            return self

        def eval(self):
            return self

    def fake(which):
        def run(model, items, *a, **kw):
            seen[which] = (a, kw)
            return {it["item_name"]: np.zeros(256, np.int16) for it in items}
        return run

    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    monkeypatch.setattr(fastdiff_amd, "FastDiff", Model)
    monkeypatch.setattr(infer, "synthesize", fake("fastdiff"))
    monkeypatch.setattr(infer, "synthesize_griffin_lim", fake("griffin_lim"))
    monkeypatch.setattr(infer, "synthesize_long", fake("long"))
    np.save(tmp_path / "a.npy", np.zeros((5, 80), np.float32))
    base = ["--test_input_dir", str(tmp_path), "--out_dir", str(tmp_path / "o")]
    infer.main(base)
    assert set(seen) == {"fastdiff"}                        # the default is the model
    seen.clear()
    infer.main(base + ["--vocoder", "fastdiff"])
    assert set(seen) == {"fastdiff"}
    seen.clear()
    infer.main(base + ["--vocoder", "griffin_lim", "--seed", "9", "--max_batch", "3", "--out_sample_rate", "16000", "--loudness", "-23", "--mel_variant", "tacotron"])
    a, kw = seen.pop("griffin_lim")
    assert not seen and a == (60, 3, 9) and kw == dict(variant="tacotron", out_sample_rate=16000, loudness=-23.0, stoi=False, pitch=False, spectral=False)
    infer.main(base + ["--vocoder", "griffin_lim", "--gl_iters", "0"])
    assert seen.pop("griffin_lim")[0][0] == 0
    assert os.path.exists(tmp_path / "o" / "a.npy_pred.wav")
    # the neural baseline: the generator loaded from --pwg_dir goes in behind the model, then the items, (max_batch, seed) and the keywords
    from fastdiff_amd.pwg import ParallelWaveGAN

    def fake_pwg(model, gen, items, *a, **kw):
        seen.setdefault("pwg", []).append((gen, a, kw))
        return {it["item_name"]: np.zeros(256, np.int16) for it in items}

    monkeypatch.setattr(ParallelWaveGAN, "from_dir", classmethod(lambda cls, d: ("generator of", d)))
    monkeypatch.setattr(infer, "synthesize_pwg", fake_pwg)
    infer.main(base + ["--vocoder", "pwg", "--pwg_dir", "D", "--seed", "9", "--max_batch", "3"])
    (gen, a, kw), = seen.pop("pwg")
    assert not seen and gen == ("generator of", "D") and a == (3, 9)
    assert kw == dict(out_sample_rate=None, loudness=None, stoi=False, pitch=False, spectral=False)
    for bad in (["--vocoder", "pwg"], ["--vocoder", "pwg", "--pwg_dir", "D", "--long_form"]):
        with pytest.raises(SystemExit):
            infer.main(base + bad)
    assert not seen
    for bad in (["--vocoder", "wavenet"], ["--vocoder", "griffin_lim", "--long_form"], ["--vocoder", "griffin_lim", "--gl_iters", "-1"],
                ["--vocoder", "griffin_lim", "--gl_iters", "10001"], ["--vocoder", "griffin_lim", "--stoi"]):
        with pytest.raises(SystemExit):
            infer.main(base + bad)
    assert not seen


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ragged_batch(what):
    """[3, 513, 37] float32: item b holds the first RAGGED[b] frames of `what`(RAGGED[b]), garbage behind them"""
    out = np.full((len(RAGGED), 513, max(RAGGED)), 1e30, np.float32)
    for b, T in enumerate(RAGGED):
        out[b, :, :T] = what(T)
    return out


@pytest.mark.gpu
def test_the_inverse_transform_alone(model):
    worst = 0.0
    for T in FRAMES:
        A, th = spectrum(T)
        y, rec = model.griffin_lim(dev(A)[None], n_iters=0, angles=dev(th)[None], return_record=True)
        assert y.shape == (1, 256 * (T - 1)) and int(rec["status"][0]) == gl.OK and int(rec["frames"][0]) == T and int(rec["samples"][0]) == 256 * (T - 1)
        err = np.abs(y[0].cpu().numpy() - oracle(T, "true", 0)).max()
        worst = max(worst, err / scale(A))
        print(f"T = {T}: max |y - y_f64| {err:.2e}, bar {BAR_ISTFT * scale(A):.2e}")
        assert err <= BAR_ISTFT * scale(A), (T, err)
    y = model.griffin_lim(dev(ragged_batch(lambda T: spectrum(T)[0])), lens=RAGGED, n_iters=0, angles=dev(ragged_batch(lambda T: spectrum(T)[1])))
    for b, T in enumerate(RAGGED):
        L = 256 * (T - 1)
        err = np.abs(y[b, :L].cpu().numpy() - oracle(T, "true", 0)).max()
        assert err <= BAR_ISTFT * scale(spectrum(T)[0]) and not y[b, L:].any(), (b, T, err)
    print(f"worst error over S: {worst:.2e} (bar {BAR_ISTFT:.0e})")


@pytest.mark.gpu
def test_the_random_start_is_keyed_as_documented(model):
    for T in FRAMES:
        A = spectrum(T)[0]
        y = model.griffin_lim(dev(A)[None], n_iters=0, seed=SEED, stream_ids=[UID])
        err = np.abs(y[0].cpu().numpy() - oracle(T, "random", 0)).max()
        print(f"T = {T}: max |y - y_f64| {err:.2e}, bar {BAR_ISTFT * scale(A):.2e}")
        assert err <= BAR_ISTFT * scale(A), (T, err)
    A = spectrum(9)[0]
    default = model.griffin_lim(dev(np.stack([A, A])), n_iters=0, seed=SEED)          # without ids: item b draws from stream b
    for b in range(2):
        want = ref.griffin_lim(A, ref.philox_angles(SEED, b, 9), 0)
        assert np.abs(default[b].cpu().numpy() - want).max() <= BAR_ISTFT * scale(A)
    other = model.griffin_lim(dev(A)[None], n_iters=0, seed=SEED + 1, stream_ids=[UID])
    assert np.abs(other[0].cpu().numpy() - oracle(9, "random", 0)).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("how,iters", (("true", (1, 3)), ("random", (1, 2))))
def test_short_trajectories_stay_within_ten_times_the_float32_yardstick(model, how, iters):
    for T in FRAMES:
        A = spectrum(T)[0]
        for n in iters:
            kw = dict(angles=dev(start(T, "true"))[None]) if how == "true" else dict(seed=SEED, stream_ids=[UID])
            y = model.griffin_lim(dev(A)[None], n_iters=n, **kw)
            err, yard = np.abs(y[0].cpu().numpy() - oracle(T, how, n)).max(), yardstick(T, how, n)
            print(f"{how} start, T = {T}, n_iters = {n}: device {err:.2e}, torch float32 on the CPU {yard:.2e}")
            assert err <= TIMES * yard, (how, T, n, err, yard)
            if how == "true":
                assert np.abs(y[0].cpu().numpy() - signal(T)).max() <= 1e-5      # the result stays at x


@pytest.mark.gpu
def test_the_record(model):
    A = ragged_batch(lambda T: spectrum(T)[0])
    y, rec = model.griffin_lim(dev(A), lens=RAGGED, n_iters=4, seed=SEED, stream_ids=[1, 2, 3], return_record=True)
    assert set(rec) == set(gl.RECORD.names) and list(rec["status"]) == [gl.OK] * 3 and list(rec["iters"]) == [4] * 3
    assert list(rec["frames"]) == list(RAGGED) and list(rec["samples"]) == [256 * (T - 1) for T in RAGGED]
    for b, T in enumerate(RAGGED):
        got = y[b, : 256 * (T - 1)].cpu().numpy().astype(np.float64)
        want = ref.inconsistency(got, spectrum(T)[0])
        print(f"item {b}: sc {rec['sc'][b]:.6f}, float64 of the returned waveform {want:.6f}")
        assert abs(rec["sc"][b] - want) <= BAR_SC
        assert abs(rec["norm"][b] - np.sqrt((spectrum(T)[0].astype(np.float64) ** 2).sum())) <= 1e-9 * rec["norm"][b]
    bad = A.copy()
    bad[0, :, :2] = 0.0                                     # SILENT over its own two frames
    bad[1, 100, 3] = -1e-3                                  # NONFINITE: a negative amplitude
    lens = [2, 5, 37, 1, 37, 37]
    six = np.concatenate([bad, A[2:3], A[2:3], A[2:3]])
    six[4, 7, 30] = np.float32("nan")
    six[5, 512, 36] = np.float32("inf")
    y6, r6 = model.griffin_lim(dev(six), lens=lens, n_iters=4, seed=SEED, stream_ids=[1, 2, 3, 4, 5, 6], return_record=True)
    assert list(r6["status"]) == [gl.SILENT, gl.NONFINITE, gl.OK, gl.SHORT, gl.NONFINITE, gl.NONFINITE]
    assert [ref.status(six[b], lens[b]) for b in range(6)] == list(r6["status"])
    assert np.isnan(r6["sc"][[0, 1, 3, 4, 5]]).all() and r6["norm"][0] == 0.0 and list(r6["samples"]) == [256, 1024, 9216, 0, 9216, 9216]
    for b in (0, 1, 3, 4, 5):
        assert not y6[b].any(), b                           # the row is zeros
    assert torch.equal(y6[2], y[2]) and r6["sc"][2].tobytes() == rec["sc"][2].tobytes()      # the other items are unaffected


@pytest.mark.gpu
def test_convergence(model):
    A = dev(spectrum(37)[0])[None]
    sc = {n: float(model.griffin_lim(A, n_iters=n, seed=SEED, stream_ids=[UID], return_record=True)[1]["sc"][0]) for n in (0, 1, 2, 4, 8, 16, 32)}
    print("sc by n_iters:", {n: round(v, 5) for n, v in sc.items()})
    seq = [sc[n] for n in (0, 1, 2, 4, 8, 16)]
    assert all(b <= a + 1e-5 for a, b in zip(seq, seq[1:])), seq
    assert sc[32] <= 0.5 * sc[0], sc


@pytest.mark.gpu
def test_bit_identity_alone_in_a_batch_and_from_call_to_call(model):
    A = ragged_batch(lambda T: spectrum(T)[0])
    ids = [21, 22, 23]
    y, rec = model.griffin_lim(dev(A), lens=RAGGED, n_iters=3, seed=SEED, stream_ids=ids, return_record=True)
    for b, T in enumerate(RAGGED):
        ya, ra = model.griffin_lim(dev(spectrum(T)[0])[None], n_iters=3, seed=SEED, stream_ids=[ids[b]], return_record=True)
        assert torch.equal(ya[0], y[b, : 256 * (T - 1)]) and not y[b, 256 * (T - 1):].any(), b
        assert all(ra[k][0].tobytes() == rec[k][b].tobytes() for k in rec), b
    y2, rec2 = model.griffin_lim(dev(A), lens=RAGGED, n_iters=3, seed=SEED, stream_ids=ids, return_record=True)
    assert torch.equal(y, y2) and all(rec[k].tobytes() == rec2[k].tobytes() for k in rec)
    order = [2, 0, 1]
    y3 = model.griffin_lim(dev(A[order]), lens=[RAGGED[i] for i in order], n_iters=3, seed=SEED, stream_ids=[ids[i] for i in order])
    assert all(torch.equal(y3[b], y[src]) for b, src in enumerate(order))


@pytest.mark.gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays():
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no table, no scratch yet
    lib, h = m._ready(torch.device("cuda"))
    T = 9
    Aa, Ab = dev(spectrum(T)[0])[None], dev(spectrum(T)[0][::-1].copy())[None]
    amp = Aa.clone()
    wav = torch.zeros((1, 256 * (T - 1)), device="cuda")
    rec = torch.zeros((1, gl.RECORD.itemsize), device="cuda", dtype=torch.uint8)
    args = lambda a, B, frames, w: (h, a.data_ptr(), None, B, frames, None, 2, SEED, None, w.data_ptr(), 256 * (frames - 1), rec.data_ptr(), m._stream(a.device))      # noqa: E731
    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        amp.mul_(1.0)                                      # (so that the capture is not empty)
        rc = lib.fd_griffin_lim(*args(amp, 1, T, wav))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a, want_b = m.griffin_lim(Aa, n_iters=2, seed=SEED), m.griffin_lim(Ab, n_iters=2, seed=SEED)      # outside: the tables and the scratch buffer
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, lib.fd_griffin_lim(*args(amp, 1, T, wav)), "fd_griffin_lim")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(wav, want_a)
    amp.copy_(Ab)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(wav, want_b) and int(gl._record(rec)["status"][0]) == gl.OK
    big, big_wav = torch.zeros((3, 513, 37), device="cuda"), torch.zeros((3, 256 * 36), device="cuda")
    rec3 = torch.zeros((3, gl.RECORD.itemsize), device="cuda", dtype=torch.uint8)
    grow = torch.cuda.CUDAGraph()
    with torch.cuda.graph(grow):
        amp.mul_(1.0)
        rc = lib.fd_griffin_lim(h, big.data_ptr(), None, 3, 37, None, 2, SEED, None, big_wav.data_ptr(), 256 * 36, rec3.data_ptr(), m._stream(big.device))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"scratch buffer" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(m.griffin_lim(Ab, n_iters=2, seed=SEED), want_b)      # the handle works on


@pytest.mark.gpu
def test_mel_to_linear(model):
    rng = np.random.default_rng(9)
    mel = rng.uniform(-5.0, 0.5, (2, 80, 70)).astype(np.float32)        # 70 frames: one frame tile of 64 and a remainder
    mel[1, :, 3] = -30.0                                                # a frame at which the floor is reached everywhere
    for variant in ("pwg", "tacotron"):
        amp = model.mel_to_linear(dev(mel), variant)
        P = gl.pinv(model.mel_filterbank(variant)[0], variant)
        assert amp.shape == (2, 513, 70) and amp.dtype == torch.float32
        worst = 0.0
        for b in range(2):
            want, bound = ref.mel_to_linear(mel[b], P, variant)
            err = np.abs(amp[b].cpu().numpy() - want)
            assert (err <= BAR_MEL * bound + 1e-17).all(), (variant, b, float((err - BAR_MEL * bound).max()))
            worst = max(worst, float((err[bound > 1e-3] / bound[bound > 1e-3]).max()))      # (where the bound is not the floor's own rounding)
        print(f"{variant}: worst |err| over its bound's scale {worst:.2e} (bar {BAR_MEL:.0e})")
        assert (amp[1, :, 3] == 1e-10).all() and float(amp.min()) == np.float32(1e-10)
        assert torch.equal(amp, gl.mel_to_linear(dev(mel), P, variant))      # the module function on the operators' handle
    with pytest.raises(ValueError, match="variant"):
        model.mel_to_linear(dev(mel), "nnls")
    with pytest.raises(ValueError, match="80"):
        model.mel_to_linear(dev(mel[:, :79]))


@pytest.fixture(scope="module")
def recordings(model, tmp_path_factory):
    """two synthetic recordings of about a second (oracle/synth.py's generator, scaled into range)"""
    import synth
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("gl_corpus")
    for i, frames in enumerate((86, 61)):
        x = np.clip(0.1 * synth.synth_audio(31 + i, 1, frames).reshape(-1), -0.9, 0.9)
        wavfile.write(d / f"r{i}.wav", 22050, np.round(x * 32767.0).astype(np.int16))
    return str(d)


@pytest.mark.gpu
def test_end_to_end_next_to_the_model(model, recordings):
    items = infer.load_wav_inputs(model, recordings, keep_wav=True)
    assert [it["len"] for it in items] == [87, 62]
    mel = items[0]["mel"].transpose(0, 1).unsqueeze(0).contiguous().cuda()
    wav, rec = model.griffin_lim_mel(mel, n_iters=8, seed=3, return_record=True)
    assert wav.shape == (1, items[0]["wav"].numel()) == (1, 86 * 256) and int(rec["status"][0]) == gl.OK and 0.0 < rec["sc"][0] < 1.0
    before = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, stoi=True, spectral=True)
    pcm, report = infer.synthesize_griffin_lim(model, items, n_iters=8, max_batch=2, seed=3, stoi=True, spectral=True)
    after = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, stoi=True, spectral=True)
    assert set(pcm) == set(before[0]) == {"r0.wav", "r1.wav"}
    for name in pcm:
        assert pcm[name].dtype == np.int16 and pcm[name].shape == before[0][name].shape and np.abs(pcm[name]).max() == 32767
        assert set(report[name]) == set(before[1][name]) == {"stoi", "estoi", "status", "mr_sc", "mr_logmag", "lsd_db", "spectral_status"}
        assert report[name]["status"] == "OK" and report[name]["spectral_status"] == "OK"
        assert np.array_equal(before[0][name], after[0][name]) and before[1][name] == after[1][name]      # synthesize is untouched by the baseline run
        print(name, "synthesize sha256", hashlib.sha256(before[0][name].tobytes()).hexdigest()[:16], "griffin_lim", {k: report[name][k] for k in ("stoi", "mr_sc", "lsd_db")})
    alone = infer.synthesize_griffin_lim(model, items[1:], n_iters=8, max_batch=1, seed=3)      # uid defaults to the position: give it the job's
    assert not np.array_equal(alone["r1.wav"], pcm["r1.wav"])
    alone = infer.synthesize_griffin_lim(model, [dict(items[1], uid=1)], n_iters=8, max_batch=1, seed=3)
    assert np.array_equal(alone["r1.wav"], pcm["r1.wav"])                                      # a waveform does not depend on its micro-batch
