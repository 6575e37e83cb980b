"""Cutting long silences on the device (fd_trim_windows / _mask / _levels / _silences, FastDiff.trim_silences, infer.trim_long_sil_wav,
infer.load_wav_inputs(trim_long_sil=True), TrainCorpus.from_wav_dir(trim_long_sil=True)) against the float64 restatement
tests/trim_ref.py.

Bounds.  Levels and peak: 1e-9 dB.  Derived: a float64 sum of at most 2 W - 1 = 11519 terms moves e_w by under 1.3e-12 relative, which
is 6e-12 dB; a few ulp of log10 at 200 dB add 1e-13; the bar leaves two orders of margin for the order of summation.  Flags, out_valid,
the record's counts and status: equal -- every case first asserts on the oracle that each window lies at least 0.01 dB from the
threshold, seven orders above the level bound, so no decision can differ by rounding; no case is left out.  out: torch.equal to the
oracle's x[mask] followed by zeros (bit copies).  An utterance alone, in a ragged batch with garbage behind it, 4 bytes off alignment,
and replayed from a graph: the same bits.

The detector is an energy detector, not WebRTC's: nothing here compares with WebRTC's flags.  What IS the reference's -- the smoothing
(a cumulative-sum moving average, then np.round) and the dilation (scipy.ndimage.binary_dilation) -- is compared with the restatement
and with the library's host statement (fd_trim_mask) on the CPU.

Signals (fixed seeds): noise 80 dB down plus a DC offset of 0.003 (only the mean removal keeps it from reading -50 dB everywhere),
1 kHz sine bursts at -20, -30, -25 and -52 dB over the fractions 0.10-0.35, 0.40-0.47, 0.55-0.56 and 0.75-0.95 of the length: bursts
that the smoothing removes, gaps that the dilation bridges and gaps it does not.
"""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.io import wavfile

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import TrainCorpus, _capi, infer
from fastdiff_amd import trim as tr
import trim_ref as ref

NEW = ("fd_trim_default_params", "fd_trim_windows", "fd_trim_mask", "fd_trim_levels", "fd_trim_silences")
CHUNK = _capi.FD_TRIM_CHUNK
LEVEL_BOUND_DB = 1e-9
MARGIN_DB = 0.01
BURSTS = ((0.10, 0.35, -20.0), (0.40, 0.47, -30.0), (0.55, 0.56, -25.0), (0.75, 0.95, -52.0))


@functools.lru_cache(maxsize=None)
def signal_of(seed, rate, n, extra=()):
    """float32 [n]: noise 80 dB down + DC 0.003 + the bursts of BURSTS (a sine of level L dB has the amplitude sqrt(2) 10^(L / 20)), and
    `extra` bursts ((first sample, end sample, dB), ...)."""
    rng = np.random.default_rng([seed, rate, n])
    t = np.arange(n)
    x = 1e-4 * rng.standard_normal(n) + 0.003
    for lo, hi, db in tuple((int(a * n), int(b * n), db) for a, b, db in BURSTS) + tuple(extra):
        x[lo:hi] += np.sqrt(2.0) * 10.0 ** (db / 20.0) * np.sin(2 * np.pi * 1000.0 * t[lo:hi] / rate)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(seed, rate, n, window_ms=30, A=8, G=12, mode="long", extra=(), top_db=40.0):
    """The restatement's result for signal_of(...), computed once and shared; asserts the margin every case relies on."""
    r = ref.trim(signal_of(seed, rate, n, extra), rate, window_ms, top_db, -70.0, A, G, mode)
    assert r["margin_db"] >= MARGIN_DB, f"a window lies {r['margin_db']:.4f} dB from the threshold: the case cannot demand equal flags"
    return r


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+FD_TRIM_CHUNK\s+(\d+)", header).group(1)) == _capi.FD_TRIM_CHUNK == tr.CHUNK
    assert tr.RECORD.itemsize == 40 and ct.sizeof(_capi.FdTrimParams) == 40
    assert callable(fastdiff_amd.FastDiff.trim_silences) and "trim" in fastdiff_amd.__all__ and fastdiff_amd.trim is tr
    assert (tr.OK, tr.SILENT, tr.EMPTY) == (ref.OK, ref.SILENT, ref.EMPTY)
    assert (tr.SPEECH, tr.SMOOTH, tr.KEEP) == (ref.SPEECH, ref.SMOOTH, ref.KEEP)
    p = _capi.FdTrimParams()
    assert lib.fd_trim_default_params(22050, ct.byref(p)) == _capi.FD_OK
    assert (p.sample_rate, p.window_ms, p.average_width, p.max_silence, p.mode, p.reserved, p.top_db, p.floor_db) == (22050, 30, 8, 12, 0, 0, 40.0, -70.0)
    # a NULL handle is refused before anything is touched
    assert lib.fd_trim_silences(None, None, 1, 1, None, ct.byref(p), None, None, None, None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_trim_levels(None, None, 1, 1, None, 22050, 30, None, None) == _capi.FD_ERR_INVALID


@pytest.mark.parametrize("rate", (22050, 16000, 8000))
@pytest.mark.parametrize("window_ms", (10, 20, 30))
def test_window_counts_equal_the_restatement(rate, window_ms):
    W = window_ms * rate // 1000
    assert {(22050, 30): 661, (16000, 30): 480, (8000, 10): 80}.get((rate, window_ms), W) == W
    for n in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 13 * W + 5):
        assert tr.windows(n, rate, window_ms) == ref.windows(n, rate, window_ms), n
    b = ref.bounds(13 * W + 5, rate, window_ms)
    assert len(b) == 13 and b[0] == (0, W) and b[-1] == (12 * W, 13 * W + 5) and all(b[k][1] == b[k + 1][0] for k in range(12))


def test_bad_parameters_are_refused():
    lib = _capi.load()
    W, M = ct.c_int64(), ct.c_int64()
    for n, rate, ms in ((-1, 22050, 30), (100, 7999, 30), (100, 192001, 30), (100, 22050, 15), (100, 22050, 0)):
        assert lib.fd_trim_windows(n, rate, ms, ct.byref(W), ct.byref(M)) == _capi.FD_ERR_INVALID, (n, rate, ms)
        with pytest.raises(ValueError):
            tr.windows(n, rate, ms)
    assert lib.fd_trim_windows(100, 22050, 30, None, None) == _capi.FD_OK
    s = np.ones(5, np.uint8)
    out = np.zeros(5, np.uint8)
    for A, G, mode in ((0, 12, 0), (65, 12, 0), (8, -2, 0), (8, 13, 0), (8, 256, 0), (8, 12, 2)):
        assert lib.fd_trim_mask(s.ctypes.data, 5, A, G, mode, out.ctypes.data) == _capi.FD_ERR_INVALID, (A, G, mode)
    assert lib.fd_trim_mask(None, 5, 8, 12, 0, out.ctypes.data) == _capi.FD_ERR_INVALID
    assert lib.fd_trim_mask(s.ctypes.data, 0, 8, 12, 0, out.ctypes.data) == _capi.FD_ERR_INVALID
    with pytest.raises(ValueError, match="mode"):
        tr.mask(s, mode="both")


def _moving_average_round(flags, width):
    """The reference's smoothing as it formulates it (data_gen_utils.py:75-82): zero padding, a cumulative sum, np.round."""
    padded = np.concatenate((np.zeros((width - 1) // 2), flags, np.zeros(width // 2)))
    c = np.cumsum(padded, dtype=float)
    c[width:] = c[width:] - c[:-width]
    return np.round(c[width - 1:] / width).astype(bool)


@pytest.mark.parametrize("M", (1, 2, 7, 8, 9, 13, 100))
def test_smoothing_and_dilation_are_the_reference_s(M):
    rng = np.random.default_rng(M)
    for trial in range(12):
        s = rng.random(M) < (0.25, 0.5, 0.75)[trial % 3]
        for A in (1, 7, 8):
            sm = ref.smooth(s, A)
            assert np.array_equal(sm, _moving_average_round(s.astype(float), A)), (M, A, s)
            for G in (0, 2, 12):
                keep = ref.dilate(sm, G)
                assert np.array_equal(keep, ndimage.binary_dilation(sm, np.ones(G + 1))), (M, A, G, s)
                for mode in ("long", "edges"):      # the library's host statement of the same two steps
                    sm2, keep2 = ref.keep_mask(s, A, G, mode)
                    assert np.array_equal(tr.mask(s, A, G, mode), s * ref.SPEECH + sm2 * ref.SMOOTH + keep2 * ref.KEEP), (M, A, G, mode, s)


def test_the_signal_family_does_what_its_description_says():
    """On the oracle: the DC offset alone does not read as speech, a burst is removed by the smoothing, one gap is bridged by the
    dilation and one is not."""
    r = oracle(1, 22050, 66287)
    f = r["flags"]
    sp, sm, keep = (f & 1) > 0, (f & 2) > 0, (f & 4) > 0
    assert r["status"] == ref.OK and r["nonfinite"] == 0 and 0 < r["kept_windows"] < r["windows"] == 100
    assert not sp[:8].any() and not keep[:3].any()                      # the head: noise + DC only
    assert sp[55] and not sm[55]                                        # the 1-window burst at 0.55: smoothed away
    assert keep[36:40].all() and not sp[36:40].any()                    # the gap 0.35-0.40: bridged
    assert not keep[60:66].all()                                        # the gap 0.56-0.75: too long to survive whole
    assert r["n_out"] == len(r["out"]) == sum(hi - lo for (lo, hi), k in zip(ref.bounds(66287, 22050), keep) if k)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


WORST = {"level": 0.0}


def _check(model, x, want, rate, window_ms, A, G, mode, where, valid=None, row=0, top_db=40.0):
    """One call with flags and record + the levels, row `row` of the batch x against the oracle's dict."""
    out, ov, flags, rec = model.trim_silences(x, valid=valid, sample_rate=rate, window_ms=window_ms, top_db=top_db, average_width=A, max_silence=G,
                                              mode=mode, return_flags=True, return_record=True)
    lv = model.trim_levels(x, valid=valid, sample_rate=rate, window_ms=window_ms)[row].cpu().numpy()
    M, n_out = want["windows"], want["n_out"]
    got_lv, want_lv = lv[:M], want["levels"]
    assert np.array_equal(np.isnan(got_lv), np.isnan(want_lv)), where
    has = ~np.isnan(want_lv)
    err = float(np.abs(got_lv[has] - want_lv[has]).max()) if has.any() else 0.0
    if np.isfinite(want["peak_db"]):
        err = max(err, abs(float(rec["peak_db"][row]) - want["peak_db"]))
    else:
        assert rec["peak_db"][row] == want["peak_db"], where
    WORST["level"] = max(WORST["level"], err)
    print(f"{where}: M = {M}, n_out = {n_out}, level error {err:.2e} dB (largest so far {WORST['level']:.2e}), margin {want['margin_db']:.2f} dB")
    assert err <= LEVEL_BOUND_DB, where
    assert not lv[M:].any(), where
    assert abs(float(rec["threshold_db"][row]) - want["threshold_db"]) <= LEVEL_BOUND_DB, where
    f = flags[row].cpu().numpy()
    assert np.array_equal(f[:M], want["flags"]), (where, np.flatnonzero(f[:M] != want["flags"])[:8])
    assert not f[M:].any(), where
    for k in ("n_out", "windows", "speech", "kept_windows", "nonfinite", "status"):
        assert int(rec[k][row]) == want[k], (where, k, int(rec[k][row]), want[k])
    assert int(ov[row]) == n_out, where
    full = torch.zeros(out.shape[1])
    full[:n_out] = torch.from_numpy(want["out"].copy())
    assert torch.equal(out[row].cpu().view(torch.int32), full.view(torch.int32)), where
    return out, ov, flags, rec


SHAPE_MS = (1, 2, 7, 8, 13, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("M", SHAPE_MS)
def test_window_counts_around_the_chunk_and_every_tail(model, M, rate=8000, W=80):
    for r in (0, 1, W - 1):
        n = M * W + r
        x = torch.from_numpy(signal_of(2, rate, n).copy()).cuda()
        _check(model, x, oracle(2, rate, n, 10), rate, 10, 8, 12, "long", f"M{M}+{r}")


@pytest.mark.gpu
def test_utterances_shorter_than_a_window(model, rate=8000, W=80):
    for n in (1, W - 1):
        x = torch.from_numpy(signal_of(3, rate, n).copy()).cuda()
        _check(model, x, oracle(3, rate, n, 10), rate, 10, 8, 12, "long", f"n{n}")


@pytest.mark.gpu
@pytest.mark.parametrize("rate,window_ms,W", ((22050, 30, 661), (16000, 30, 480), (22050, 20, 441), (48000, 30, 1440), (96000, 30, 2880),
                                                (192000, 30, 5760)))
def test_native_rate_windows(model, rate, window_ms, W):
    """W = 661 and 480 at M = 100; up to 48 kHz every window is held in registers, at 96 kHz all but the last one (which takes the tail),
    at 192 kHz none."""
    n = 100 * W + (187 if rate < 96000 else W // 2 + 1)
    assert tr.windows(n, rate, window_ms) == (W, 100)
    x = torch.from_numpy(signal_of(4, rate, n).copy()).cuda()
    _check(model, x, oracle(4, rate, n, window_ms), rate, window_ms, 8, 12, "long", f"{rate}/{window_ms}")


def _border_bursts(W):
    """A 5-window burst across the first chunk border (the smoothing windows round it straddle the border) and one that ends 4 windows in
    front of the second border (its dilation reaches across)."""
    return ((CHUNK - 3) * W, (CHUNK + 2) * W, -22.0), ((2 * CHUNK - 12) * W, (2 * CHUNK - 4) * W, -24.0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("long", "edges"))
@pytest.mark.parametrize("A", (1, 8))
@pytest.mark.parametrize("G", (0, 12))
def test_modes_widths_and_bursts_across_a_chunk_border(model, mode, A, G, rate=8000, W=80):
    for M, extra in ((13, ()), (CHUNK + 1, ()), (2 * CHUNK + 5, _border_bursts(W))):
        n = M * W + 37
        x = torch.from_numpy(signal_of(5, rate, n, extra).copy()).cuda()
        want = oracle(5, rate, n, 10, A, G, mode, extra)
        _check(model, x, want, rate, 10, A, G, mode, f"{mode}-A{A}-G{G}-M{M}")
        if extra and A == 8:      # the border cases are what they claim to be
            sm, keep = (want["flags"] & 2) > 0, (want["flags"] & 4) > 0
            assert sm[CHUNK - 1] and sm[CHUNK] and (G == 0 or mode == "edges" or (keep[2 * CHUNK - 1] and keep[2 * CHUNK]))


@pytest.mark.gpu
def test_a_burst_below_the_dynamic_range_is_not_speech(model, rate=8000):
    """top_db = 30: the -52 dB burst lies under peak - 30 and is cut; at the default 40 it is kept."""
    n = 100 * 80 + 5
    x = torch.from_numpy(signal_of(6, rate, n).copy()).cuda()
    w30, w40 = oracle(6, rate, n, 10, top_db=30.0), oracle(6, rate, n, 10)
    assert not (w30["flags"][78:93] & 1).any() and (w40["flags"][78:93] & 1).all()
    _check(model, x, w30, rate, 10, 8, 12, "long", "top_db 30", top_db=30.0)
    _check(model, x, w40, rate, 10, 8, 12, "long", "top_db 40")


@pytest.mark.gpu
def test_empty_silent_nonfinite_and_all_speech_items(model, rate=8000, W=80):
    n = 40 * W + 3
    rng = np.random.default_rng(7)
    loud = (0.1 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / rate) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    bad = signal_of(7, rate, n).copy()
    w_nan, w_inf = 5, 8                                    # both inside the first burst (windows 4 .. 13)
    bad[w_nan * W + 11] = np.nan
    bad[w_inf * W + 79] = -np.inf
    rows = [signal_of(7, rate, n), (1e-4 * rng.standard_normal(n) + 0.003).astype(np.float32), np.zeros(n, np.float32), bad, loud]
    valid = [0, n, n, n, n]
    x = torch.from_numpy(np.stack(rows)).cuda()
    out, ov, flags, rec = model.trim_silences(x, valid=valid, sample_rate=rate, window_ms=10, return_flags=True, return_record=True)
    assert [tr.STATUS[s] for s in rec["status"]] == ["EMPTY", "SILENT", "SILENT", "OK", "OK"]
    assert ov.cpu().tolist()[:3] == [0, 0, 0] and not out[:3].any() and not flags[:3].any()
    assert rec["windows"].tolist() == [0, 40, 40, 40, 40] and rec["nonfinite"].tolist() == [0, 0, 0, 2, 0]
    assert rec["peak_db"][0] == -np.inf and abs(rec["peak_db"][2] + 200.0) <= LEVEL_BOUND_DB and rec["threshold_db"][2] == -70.0
    want = ref.trim(bad, rate, 10)
    assert want["margin_db"] >= MARGIN_DB and want["nonfinite"] == 2 and not (want["flags"][[w_nan, w_inf]] & 1).any()
    assert abs(want["peak_db"] - oracle(7, rate, n, 10)["peak_db"]) < 0.1          # the peak is that of the clean signal's other windows
    _check(model, x, want, rate, 10, 8, 12, "long", "nonfinite", valid=valid, row=3)
    # nothing to cut: the copy comes back bit for bit
    assert int(ov[4]) == n and rec["kept_windows"][4] == 40 and torch.equal(out[4].view(torch.int32), x[4].view(torch.int32))


@pytest.mark.gpu
def test_an_utterance_gives_the_same_bits_alone_in_a_ragged_batch_and_off_alignment(model, rate=22050):
    ns = (5949, 66287, 20011)
    rows = [signal_of(8 + k, rate, n) for k, n in enumerate(ns)]
    L = max(ns)
    g = torch.Generator().manual_seed(5)
    batch = 1e3 * torch.randn(3, L, generator=g)
    batch[:, ::7] = float("nan")                           # garbage behind every valid[b]
    for b, x in enumerate(rows):
        batch[b, :ns[b]] = torch.from_numpy(x.copy())
    out_b, ov_b, fl_b, rec_b = model.trim_silences(batch.cuda(), valid=list(ns), sample_rate=rate, return_flags=True, return_record=True)
    lv_b = model.trim_levels(batch.cuda(), valid=list(ns), sample_rate=rate)
    for b, (x, n) in enumerate(zip(rows, ns)):
        want = oracle(8 + b, rate, n)
        _check(model, batch.cuda(), want, rate, 30, 8, 12, "long", f"ragged row {b}", valid=list(ns), row=b)
        shifted = torch.empty(n + 1, device="cuda")[1:]
        shifted.copy_(torch.from_numpy(x.copy()))
        assert shifted.data_ptr() % 16 == 4
        for tag, xi in (("alone", torch.from_numpy(x.copy()).cuda()), ("off by 4 bytes", shifted)):
            out, ov, fl, rec = model.trim_silences(xi, sample_rate=rate, return_flags=True, return_record=True)
            lv = model.trim_levels(xi, sample_rate=rate)
            M = want["windows"]
            assert torch.equal(out[0].view(torch.int32), out_b[b, :n].view(torch.int32)) and not out_b[b, n:].any(), (b, tag)
            assert int(ov[0]) == int(ov_b[b]) and torch.equal(fl[0], fl_b[b, :M]), (b, tag)
            assert torch.equal(lv[0].view(torch.int64), lv_b[b, :M].view(torch.int64)), (b, tag)
            for k in rec:
                assert rec[k][0].tobytes() == rec_b[k][b].tobytes(), (b, tag, k)


@pytest.mark.gpu
def test_the_call_captures_and_replays_to_the_same_bits(model, rate=22050):
    n = 66287
    a = torch.from_numpy(signal_of(1, rate, n).copy()).cuda().reshape(1, n)
    b = torch.from_numpy(signal_of(9, rate, n).copy()).cuda().reshape(1, n)
    want_a = model.trim_silences(a, sample_rate=rate, return_flags=True)      # (also grows the scratch buffer)
    want_b = model.trim_silences(b, sample_rate=rate, return_flags=True)
    assert int(want_a[1][0]) == oracle(1, rate, n)["n_out"] and int(want_b[1][0]) == oracle(9, rate, n)["n_out"]
    x = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = model.trim_silences(x, sample_rate=rate, return_flags=True)
    for src, want in ((a, want_a), (b, want_b), (a, want_a)):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.uint8), w.view(torch.uint8))


@pytest.mark.gpu
def test_a_first_levels_call_inside_a_capture_is_refused_and_a_later_one_replays(rate=8000, window_ms=10):
    """fastdiff_hip_ext.h: the scratch buffer grows at the first call that needs more, never inside a stream capture."""
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no scratch yet
    lib, h = m._ready(torch.device("cuda"))
    n = 2 * 80 + 3                                         # two windows and three samples
    xa, xb = (torch.from_numpy(signal_of(s, rate, n).copy()).cuda().reshape(1, n) for s in (1, 9))
    x = xa.clone()
    lv = torch.zeros((1, tr.windows(n, rate, window_ms)[1]), device="cuda", dtype=torch.float64)

    def call():
        return lib.fd_trim_levels(h, x.data_ptr(), 1, n, None, rate, window_ms, lv.data_ptr(), m._stream(x.device))

    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        x.mul_(1.0)                                        # (so that the capture is not empty)
        rc = call()
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a, want_b = (m.trim_levels(t, sample_rate=rate, window_ms=window_ms) for t in (xa, xb))      # outside: the scratch buffer
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, call(), "fd_trim_levels")
    for src, want in ((xa, want_a), (xb, want_b)):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert want.shape == lv.shape and torch.equal(lv.view(torch.uint8), want.view(torch.uint8))
    assert not torch.equal(want_a, want_b)


@pytest.mark.gpu
def test_refusals_leave_a_message(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(2, 9000, device="cuda")
    y = torch.empty_like(x)
    ov = torch.empty(2, dtype=torch.int32, device="cuda")

    def call(p, wav=x, out=y, L=9000):
        return lib.fd_trim_silences(h, wav.data_ptr(), 2, L, None, ct.byref(p), out.data_ptr(), ov.data_ptr(), None, None, None)

    def params(**kw):
        p = _capi.FdTrimParams()
        lib.fd_trim_default_params(22050, ct.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for kw, text in ((dict(sample_rate=7999), b"sample rate"), (dict(sample_rate=192001), b"sample rate"), (dict(window_ms=25), b"window_ms"),
                     (dict(average_width=0), b"average_width"), (dict(average_width=65), b"average_width"), (dict(max_silence=11), b"max_silence"),
                     (dict(max_silence=256), b"max_silence"), (dict(mode=2), b"mode"), (dict(top_db=0.0), b"top_db"),
                     (dict(floor_db=float("nan")), b"floor_db"), (dict(reserved=1), b"reserved")):
        assert call(params(**kw)) == _capi.FD_ERR_INVALID, kw
        assert text in lib.fd_last_error(h), (kw, lib.fd_last_error(h))
    assert call(params(), out=x) == _capi.FD_ERR_INVALID and b"overlaps" in lib.fd_last_error(h)
    assert call(params(), out=x.view(-1)[4500:], L=4500) == _capi.FD_ERR_INVALID and b"overlaps" in lib.fd_last_error(h)      # the second half of wav
    with pytest.raises(AssertionError, match="valid"):
        model.trim_silences(x, valid=[9001, 5])
    with pytest.raises(ValueError, match="mode"):
        model.trim_silences(x, mode="both")
    out, n_out = model.trim_silences(x)                   # the handle works on
    assert n_out.tolist() == [0, 0] and not out.any()


def _recording(seed, n, rate=22050):
    """int16 PCM: speech-like bursts (an amplitude-modulated sine) with a silent head, a long pause and a silent tail."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 2e-5 * rng.standard_normal(n)
    for a, b in ((0.15, 0.40), (0.70, 0.90)):
        lo, hi = int(a * n), int(b * n)
        x[lo:hi] += 0.2 * np.sin(2 * np.pi * 180.0 * t[lo:hi] / rate) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t[lo:hi] / rate))
    return np.round(x * 32767.0).astype(np.int16)


@pytest.mark.gpu
def test_the_pipeline_trims_in_front_of_the_mel(model, tmp_path, rate=22050):
    d = tmp_path / "wavs"
    d.mkdir()
    pcm = {"a.wav": _recording(1, 40000), "b.wav": _recording(2, 52345), "c.wav": np.zeros(30000, np.int16)}
    for name, p in pcm.items():
        wavfile.write(d / name, rate, p)
    # trim_long_sil_wav = normalise to -20 LUFS, then trim, by hand
    want = {}
    for name, p in pcm.items():
        wav = torch.from_numpy(infer.pcm_to_float(p)).cuda()
        y = model.loudness_normalize(wav, -20.0, sample_rate=rate, out="float")
        out, ov = model.trim_silences(y, sample_rate=rate)
        want[name] = out[0, :int(ov[0])].clone()
        got, rec = infer.trim_long_sil_wav(model, wav, rate, name, return_record=True)
        assert torch.equal(got, want[name]) and rec["n_out"] == got.numel(), name
    assert 0 < want["a.wav"].numel() < 40000 and 0 < want["b.wav"].numel() < 52345 and want["c.wav"].numel() == 0
    with pytest.raises(ValueError, match="tiny.wav"):
        infer.trim_long_sil_wav(model, torch.zeros(4000, device="cuda"), rate, "tiny.wav")
    assert infer.trim_long_sil_wav(model, torch.zeros(4000, device="cuda"), rate, "tiny.wav", norm=False).numel() == 0
    # load_wav_inputs: the silent recording is left out, the others carry the trimmed recording and its mel
    report = []
    with pytest.warns(UserWarning, match="c.wav"):
        items = infer.load_wav_inputs(model, str(d), keep_wav=True, trim_long_sil=True, trim_report=report)
    assert [it["item_name"] for it in items] == ["a.wav", "b.wav"]
    for it in items:
        w = want[it["item_name"]]
        assert torch.equal(it["wav"], w) and it["len"] == 1 + w.numel() // 256
        assert torch.equal(it["mel"], model.mel_spectrogram(w)[0].transpose(0, 1).contiguous().cpu())
    text = infer.write_trim_report(report, str(tmp_path / "trim.tsv"))
    lines = open(tmp_path / "trim.tsv").read().splitlines()
    assert text.splitlines() == lines and lines[0].split("\t") == ["name", "samples_in", "samples_out", "windows", "kept_windows", "peak_db", "status"]
    cells = [ln.split("\t") for ln in lines[1:]]
    assert [c[0] for c in cells] == ["a.wav", "b.wav", "c.wav"] and [c[1] for c in cells] == ["40000", "52345", "30000"]
    assert [int(c[2]) for c in cells] == [want[k].numel() for k in ("a.wav", "b.wav", "c.wav")]
    assert [c[6] for c in cells] == ["OK", "OK", "SILENT"] and cells[2][3:5] == ["45", "0"]
    # the corpus: the silent recording is skipped and counted
    corpus = TrainCorpus.from_wav_dir(model, str(d), max_samples=2560, trim_long_sil=True)
    assert corpus.n_skipped == 1 and corpus.kept.tolist() == [0, 1]
    assert corpus.lengths.tolist() == [1 + want[k].numel() // 256 for k in ("a.wav", "b.wav")]
    na = want["a.wav"].numel()
    assert torch.equal(corpus.wav[:na], want["a.wav"])
    # with the argument off both are what they were
    plain = infer.load_wav_inputs(model, str(d), keep_wav=True)
    assert [it["item_name"] for it in plain] == ["a.wav", "b.wav", "c.wav"]
    for it, name in zip(plain, pcm):
        wav = infer.wav_to_device(model, pcm[name], rate, rate, name)
        assert torch.equal(it["wav"], wav) and torch.equal(it["mel"], model.mel_spectrogram(wav)[0].transpose(0, 1).contiguous().cpu())
    c0 = TrainCorpus.from_wav_dir(model, str(d), max_samples=2560)
    assert c0.n_skipped == 0 and c0.lengths.tolist() == [1 + len(p) // 256 for p in pcm.values()]
    assert torch.equal(c0.wav[:40000], torch.from_numpy(infer.pcm_to_float(pcm["a.wav"])).cuda())
