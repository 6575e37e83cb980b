"""F0 tracking and the pitch scores on the device (fd_pitch_default_config / _lags / _frames / _track / _compare, fastdiff_amd.pitch,
FastDiff.pitch, Validator(pitch=True), infer.synthesize(pitch=True), --pitch) against the float64 oracle tests/pitch_ref.py, which
restates the header's steps 1-5 and the record in numpy.

Bounds.  Integer fields and status: equal.  The voicing flag and the lag k: equal on every decided frame -- one whose oracle margins
are m_thr >= 1e-4 (the distance of d' from the threshold on the way to k0) and m_desc >= 1e-5 (the smallest step of the descent); at
most 2 % of the frames of any input may be undecided (asserted on the oracle: the 22050 Hz inputs at win 1024 and 512 have none, the 16 kHz / 63 Hz
ones one frame of 75, win 1023 and 1021 one of 103).  f0 within 1e-2 cents and aper within 1e-5 on decided frames.  A CPU emulation of the device's split
(pitch_ref.track(sums="float32"): d in float32 in the kernel's order, the rest in float64) against the oracle on these inputs:

    input                      frames  voiced  flags, k   max |f0| cents   max |aper|   max |d'| (all lags)   min m_thr   min m_desc
    22050 Hz / 80 Hz, 3 s         258      80   equal        5.7e-05        2.9e-07         5.4e-06          1.6e-04     1.5e-05
    16000 Hz / 63 Hz, 1.2 s        75      24   equal        7.2e-05        2.3e-07         2.1e-06          5.3e-05     1.3e-04
    22050 Hz, win 1023, 1.2 s     103      44   equal        4.9e-05        2.9e-07            -             4.1e-05     1.4e-05
    22050 Hz, win 1021, 1.2 s     103      44   equal        5.2e-05        2.1e-07            -             2.8e-05     2.1e-05

so 1e-2 cents and 1e-5 leave two orders of magnitude for another summation order (the emulation has to stay within 1e-3 cents and
1e-6, or the inputs change); the metric is read at 1 cent.  The record against the oracle's record from the oracle's own tracks, for
inputs without an undecided frame: rmse_cents within 1e-2 cents, gpe and vde within 1e-9 (equal counts).
fd_pitch_compare fed the oracle's float32 tracks: rmse_cents within 1e-9 relative, counts equal.  A row alone, in a ragged batch with
garbage behind it, at another row pitch and from call to call: the same bits.
"""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import _capi, infer
from fastdiff_amd import pitch as pt
import pitch_ref as ref

NEW = ("fd_pitch_default_config", "fd_pitch_lags", "fd_pitch_frames", "fd_pitch_track", "fd_pitch_compare")
FT, CHUNK, MAXL, STAGE = _capi.FD_PITCH_FRAME_TILE, _capi.FD_PITCH_LAG_CHUNK, _capi.FD_PITCH_MAX_LAGS, _capi.FD_PITCH_STAGE_FLOATS
DEGRADATIONS = ("snr20", "snr5", "sharp3", "clip")
TILE_FRAMES = (0, 1, 2, FT - 1, FT, FT + 1, 2 * FT + 3)
# (rate, f0_min) -> L = ceil(rate / f0_min) + 2: the issue's three (278, 202, 256 = 4 chunks of 64), then one below and one above 4 chunks
LAG_CASES = ((22050, 80.0, 278), (16000, 80.0, 202), (16000, 63.0, 256), (16000, 63.3, 255), (16000, 62.9, 257))
# hops at which the frames of a tile that are staged together go from 4 to 3, 3 to 2 and 2 to 1 (default lags: span = 1301):
# g = min(FT, 1 + (STAGE - span) // hop)
SPAN = 1024 + 276 + 1
STAGE_HOPS = tuple(h + d for g in (3, 2, 1) for h in ((STAGE - SPAN) // g,) for d in (0, 1))
# windows that are no multiple of the four accumulators: 1023 leaves one sample to each of a0, a1, a2; 1021 one to a0
ODD_WINS = (1023, 1021)
SHORT_S, LONG_S = 1.2, 3.0
SEED = 23
OFFSET_S = 0.33                                            # the tile cases start here: 11 frames run from voiced speech into the burst


@functools.lru_cache(maxsize=None)
def clean_of(rate, sharp=1.0):
    """float32, 3 s, from a fixed seed: harmonics 1 .. 19 of f0(t) = 170 + 90 sin(2 pi 0.7 t + 0.3) + 30 sin(2 pi 2.3 t), each
    sin(h phase + random phase) / h with its own slow amplitude modulation, times a 4 Hz syllabic envelope; in every 0.6 s: voiced
    with 0.01 N(0, 1) up to 0.38 s, a burst of 0.3 N(0, 1) up to 0.5 s, then near silence 1e-4 N(0, 1); scaled to peak 0.2.  sharp: the
    factor on the fundamental's phase (1.03: the whole voice 3 % sharp, the noise the same)."""
    rng = np.random.default_rng([SEED, rate])
    N = int(round(LONG_S * rate))
    t = np.arange(N) / rate
    f0 = 170.0 + 90.0 * np.sin(2 * np.pi * 0.7 * t + 0.3) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    phase = sharp * 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(N)
    for h in range(1, 20):
        r, ph = rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
        if h * 290.0 * 1.03 < rate / 2:
            x += (0.6 + 0.4 * np.sin(2 * np.pi * r * t)) * np.sin(h * phase + ph) / h
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)
    pos = t % 0.6
    n1, n2, n3 = (rng.standard_normal(N) for _ in range(3))
    x = np.where(pos < 0.38, x + 0.01 * n1, np.where(pos < 0.5, 0.3 * n2, 1e-4 * n3))
    x = (0.2 * x / np.abs(x).max()).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def degraded_of(rate, how):
    """clean plus white noise at 20 / 5 dB SNR; the voice 3 % sharp; a hard clip at +-0.05"""
    x = clean_of(rate).astype(np.float64)
    if how == "clip":
        y = np.clip(x, -0.05, 0.05)
    elif how == "sharp3":
        y = clean_of(rate, 1.03).astype(np.float64)
    else:
        rng = np.random.default_rng([SEED, 29, DEGRADATIONS.index(how)])
        y = x + rng.standard_normal(len(x)) * np.sqrt((x ** 2).mean() / 10.0 ** (float(how[3:]) / 10.0))
    y = y.astype(np.float32)
    y.setflags(write=False)
    return y


def signal(name, rate):
    return clean_of(rate) if name == "clean" else degraded_of(rate, name)


def piece(name, rate, start, n):
    return signal(name, rate)[start: start + n]


@functools.lru_cache(maxsize=None)
def oracle(name, rate, start, n, cfg=()):
    """The oracle's detailed track of a piece of a signal; computed once, shared, never changed."""
    out = ref.track(piece(name, rate, start, n), detail=True, rate=rate, **dict(cfg))
    for v in out.values():
        v.setflags(write=False)
    return out


def tile_cases():
    """(name, rate, start, n, cfg): F = each of TILE_FRAMES, n a multiple of the hop and hop - 1 more"""
    start = int(OFFSET_S * 22050)
    return [("clean", 22050, start, F * 256 + extra, ()) for F in TILE_FRAMES for extra in (0, 255)]


def lag_cases():
    out = []
    for rate, f0_min, L in LAG_CASES:
        n = int((LONG_S if (rate, f0_min) == (22050, 80.0) else SHORT_S) * rate)
        out.append(("clean", rate, 0, n, (("f0_min", f0_min),)))
    n = int(SHORT_S * 22050)
    out.append(("clean", 22050, 0, n, (("win", 512),)))
    out.append(("clean", 22050, 0, n, (("hop", 128),)))
    return out


def stage_group(hop, span=SPAN):
    return min(FT, 1 + (STAGE - span) // hop)


def stage_cases():
    """2 FT + 3 frames (tiles of 4, 4, 3, each split unevenly where fewer than 4 frames are staged together), n = F hop + hop - 1"""
    return [("clean", 22050, 0, (2 * FT + 3) * hop + hop - 1, (("hop", hop),)) for hop in STAGE_HOPS]


def win_cases():
    return [("clean", 22050, 0, int(SHORT_S * 22050), (("win", win),)) for win in ODD_WINS]


def measure_cases():
    return [(how, 22050, 0, int(LONG_S * 22050), ()) for how in DEGRADATIONS]


def all_cases():
    return tile_cases() + lag_cases() + stage_cases() + win_cases() + measure_cases()


def decided(o):
    return (o["m_thr"] >= 1e-4) & (o["m_desc"] >= 1e-5)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for name, value, mine in (("FD_PITCH_MAX_LAGS", MAXL, pt.MAX_LAGS), ("FD_PITCH_FRAME_TILE", FT, pt.FRAME_TILE), ("FD_PITCH_LAG_CHUNK", CHUNK, pt.LAG_CHUNK),
                              ("FD_PITCH_STAGE_FLOATS", STAGE, pt.STAGE_FLOATS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == value == mine, name
    assert MAXL == ref.MAX_LAGS == 1024
    assert pt.RECORD.itemsize == 48 and ct.sizeof(pt.FdPitchConfig) == 40
    assert callable(fastdiff_amd.FastDiff.pitch) and "pitch" in fastdiff_amd.__all__ and fastdiff_amd.pitch is pt
    assert (pt.OK, pt.SHORT, pt.UNVOICED) == (ref.OK, ref.SHORT, ref.UNVOICED) and pt.STATUS[pt.UNVOICED] == "UNVOICED"
    assert pt.default_config() == ref.DEFAULTS
    assert "YIN" in header and "not Praat" in header


def test_frames_and_lags_equal_the_oracle():
    for hop in (128, 256):
        for n in range(0, 3001):
            assert pt.frames(n, hop) == ref.frames(n, hop), (n, hop)
    assert [pt.frames(n, 256) for n in (0, 255, 256, 511, 512)] == [0, 0, 1, 1, 2]
    assert pt.lags(dict(rate=22050, f0_min=80, f0_max=750)) == (29, 276) == ref.lags()
    assert pt.lags(dict(rate=16000, f0_min=80, f0_max=750)) == (21, 200)
    assert pt.lags(dict(rate=16000, f0_min=63, f0_max=750)) == (21, 254)
    for rate, f0_min, L in LAG_CASES:
        assert pt.lags(dict(rate=rate, f0_min=f0_min)) == ref.lags(rate=rate, f0_min=f0_min) and pt.lags(dict(rate=rate, f0_min=f0_min))[1] + 2 == L
    assert pt.lags(dict(rate=48000, f0_min=50, f0_max=750)) == (64, 960) == ref.lags(rate=48000, f0_min=50.0)
    for rate in (8000, 16000, 22050, 24000, 44100, 48000):
        for f0_min in (50.0, 63.0, 80.0, 100.0):
            for f0_max in (400.0, 750.0, 1000.0):
                want = ref.lags(rate=rate, f0_min=f0_min, f0_max=f0_max)
                if want is None:
                    with pytest.raises(ValueError):
                        pt.lags(dict(rate=rate, f0_min=f0_min, f0_max=f0_max))
                else:
                    assert pt.lags(dict(rate=rate, f0_min=f0_min, f0_max=f0_max)) == want, (rate, f0_min, f0_max)


@pytest.mark.parametrize("bad", (dict(f0_max=12000.0),                      # tau_min = 1 < 2
                                 dict(f0_min=900.0),                        # tau_max = 25 <= tau_min = 29
                                 dict(rate=24000, f0_min=800.0, f0_max=800.0),      # tau_max = tau_min = 30
                                 dict(f0_min=21.5),                         # L = 1026 + 2 > 1024
                                 dict(rate=48000, f0_min=46.9),             # L = 1024 + 2
                                 dict(win=63), dict(win=2049), dict(hop=0), dict(hop=-3), dict(threshold=0.0), dict(threshold=1.0),
                                 dict(threshold=-0.1), dict(threshold=1.5)))
def test_every_refusal_of_a_configuration(bad):
    assert ref.lags(**bad) is None
    with pytest.raises(ValueError):
        pt.lags(bad)
    c = pt._config(bad)
    assert _capi.load().fd_pitch_lags(ct.byref(c), None, None) == _capi.FD_ERR_INVALID


def test_a_reserved_field_that_is_not_zero_is_refused():
    c = pt._config(None)
    c.reserved = 1
    assert _capi.load().fd_pitch_lags(ct.byref(c), None, None) == _capi.FD_ERR_INVALID
    for bad in (dict(rate=0), dict(f0_min=0.0), dict(f0_min=-80.0), dict(f0_max=0.0)):      # the refusals the header names besides the derived ones
        assert ref.lags(**bad) is None
        with pytest.raises(ValueError):
            pt.lags(bad)


def test_the_staging_cases_sit_at_the_group_boundaries():
    assert STAGE_HOPS == (1614, 1615, 2421, 2422, 4843, 4844)
    assert [stage_group(h) for h in STAGE_HOPS] == [4, 3, 3, 2, 2, 1]
    assert all(stage_group(c[4][0][1] if c[4] and c[4][0][0] == "hop" else 256) == FT for c in tile_cases() + lag_cases() + win_cases() + measure_cases())
    assert pt.lags() == (29, 276) and SPAN == 1024 + pt.lags()[1] + 1
    assert all(len(oracle(*c)["f0"]) == 2 * FT + 3 for c in stage_cases())


def test_the_limits_of_a_configuration_are_accepted():
    assert pt.lags(dict(rate=48000, f0_min=46.97)) == (64, 1022)           # L = 1024 = FD_PITCH_MAX_LAGS
    assert pt.lags(dict(win=64)) == pt.lags(dict(win=2048)) == (29, 276)
    assert pt.lags(dict(threshold=1e-6)) == pt.lags(dict(threshold=0.999999)) == (29, 276)
    assert pt.lags(dict(f0_min=760.0)) == ref.lags(f0_min=760.0) == (29, 30)        # tau_max = tau_min + 1
    assert pt.lags(dict(f0_max=11025.0)) == (2, 276)                       # tau_min = 2
    c = pt._config(None)
    assert _capi.load().fd_pitch_lags(ct.byref(c), None, None) == _capi.FD_OK      # either output may be left out


def test_null_arguments_are_refused():
    lib = _capi.load()
    assert lib.fd_pitch_default_config(None) == _capi.FD_ERR_INVALID
    assert lib.fd_pitch_lags(None, None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_pitch_frames(-1, 256) == _capi.FD_ERR_INVALID and lib.fd_pitch_frames(10, 0) == _capi.FD_ERR_INVALID
    assert lib.fd_pitch_track(None, None, 1, 1000, None, None, None, None, 3, None) == _capi.FD_ERR_INVALID
    assert lib.fd_pitch_compare(None, None, None, 1, 3, None, None, None) == _capi.FD_ERR_INVALID


def test_a_null_handle_is_refused_by_every_waveform_entry_point():
    """Every other argument is in order (host memory stands in for the device pointers, which nothing may touch): the shared host path
    -- the counts check, the settle, the scratch and the staging ring -- is not reached without a handle."""
    lib = _capi.load()
    n = 9000
    buf = (ct.c_float * n)()
    p = ct.addressof(buf)
    one = (ct.c_int64 * 1)(n)
    cfg = pt._config(None)
    calls = {
        "fd_resample": lambda: lib.fd_resample(None, p, _capi.FD_PCM_F32, 1, 1, 4000, 4000, (ct.c_int64 * 1)(4000), 22050, 16000, p, n, None),
        "fd_loudness_measure": lambda: lib.fd_loudness_measure(None, p, 1, n, one, 22050, p, None),
        "fd_loudness_normalize": lambda: lib.fd_loudness_normalize(None, p, 1, n, one, 22050, -23.0, p, None, None, None),
        "fd_stoi_measure": lambda: lib.fd_stoi_measure(None, p, p, 1, n, one, 22050, p, None),
        "fd_pitch_track": lambda: lib.fd_pitch_track(None, p, 1, n, one, ct.byref(cfg), p, p, 64, None),
        "fd_pitch_compare": lambda: lib.fd_pitch_compare(None, p, p, 1, 35, (ct.c_int64 * 1)(35), p, None),
        "fd_peak_normalize_int16_ragged": lambda: lib.fd_peak_normalize_int16_ragged(None, p, 1, n, one, p, None),
    }
    for name, call in calls.items():
        assert call() == _capi.FD_ERR_INVALID, name


def test_the_oracles_record():
    a = np.array([100.0, 0.0, 200.0, 0.0, 150.0, 300.0], np.float32)
    b = np.array([103.0, 50.0, 0.0, 0.0, 300.0, 300.0], np.float32)
    r = ref.compare(a, b)
    cents = 1200.0 * np.log2(np.array([1.03, 2.0, 1.0]))
    assert (r["frames"], r["both_voiced"], r["ref_voiced"], r["deg_voiced"], r["status"]) == (6, 3, 4, 4, ref.OK)
    assert abs(r["rmse_cents"] - np.sqrt((cents ** 2).mean())) <= 1e-9 and r["gpe"] == 1 / 3 and r["vde"] == 2 / 6
    r = ref.compare(a, np.zeros(6, np.float32))
    assert r["status"] == ref.UNVOICED and r["vde"] == 4 / 6 and np.isnan(r["rmse_cents"]) and np.isnan(r["gpe"])
    r = ref.compare(a[:0], b[:0])
    assert r["status"] == ref.SHORT and np.isnan(r["vde"])


def test_inputs_stay_clear_of_the_decisions_and_take_every_branch():
    """The condition on the test's inputs, checked on the oracle: at most 2 % of the frames of any case are undecided."""
    voiced = unvoiced = 0
    for case in all_cases():
        o = oracle(*case)
        und = int((~decided(o)).sum())
        assert und <= 0.02 * len(o["f0"]), (case, und, len(o["f0"]))
        voiced += int((o["f0"] > 0).sum())
        unvoiced += int((o["f0"] == 0).sum())
    for case in tile_cases() + lag_cases()[:1] + stage_cases() + measure_cases():      # these 22050 Hz inputs: none, so the records' counts have to be equal
        assert decided(oracle(*case)).all(), case
    assert [len(oracle(*c)["f0"]) for c in tile_cases()] == [F for F in TILE_FRAMES for _ in range(2)]
    big = oracle(*lag_cases()[0])
    assert len(big["f0"]) == 258 and 60 <= int((big["f0"] > 0).sum()) <= 200
    assert voiced > 0 and unvoiced > 0
    assert (big["k"] > big["k0"]).any() and (big["k"][big["f0"] > 0] >= 29).all()      # the descent moves; the range holds
    last = oracle(*tile_cases()[-1])
    assert (last["f0"] > 0).any() and (last["f0"] == 0).any()                            # the tile cases hold both kinds of frame


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared inputs are read-only)


def _check_track(f0, aper, o, rate, where):
    """device f0, aper [F] (numpy float32) against the oracle's detail"""
    assert f0.shape == aper.shape == o["f0"].shape, (where, f0.shape, o["f0"].shape)
    if len(f0) == 0:
        return
    ok = decided(o)
    want_v = o["f0"] > 0
    got_v = f0 > 0
    assert (got_v == want_v)[ok].all(), (where, np.nonzero((got_v != want_v) & ok)[0])
    v = ok & want_v
    # the lag: f0 = rate / (k + off), so k = rate / f0 - off with the oracle's own off (a parabola's off moves by far less than 1)
    off = rate / o["f0"][v] - o["k"][v]
    k_got = np.rint(rate / f0[v].astype(np.float64) - off)
    assert (k_got == o["k"][v]).all(), (where, k_got, o["k"][v])
    cents = np.abs(1200.0 * np.log2(f0[v].astype(np.float64) / o["f0"][v])) if v.any() else np.zeros(1)
    da = np.abs(aper[ok].astype(np.float64) - o["aper"][ok]) if ok.any() else np.zeros(1)
    print(f"{where}: frames {len(f0)} voiced {int(want_v.sum())} undecided {int((~ok).sum())} max |f0| {cents.max():.2e} cents max |aper| {da.max():.2e}")
    assert cents.max() <= 1e-2 and da.max() <= 1e-5, (where, cents.max(), da.max())


def _track_case(model, case):
    name, rate, start, n, cfg = case
    x = piece(name, rate, start, n)
    if n == 0:                                             # no sample at all: one sample of padding, none of it valid
        f0, aper = model.pitch_track(torch.zeros(1, device="cuda"), valid=[0], rate=rate, **dict(cfg))
    else:
        f0, aper = model.pitch_track(dev(x), rate=rate, **dict(cfg))
    assert f0.shape[0] == 1 and f0.dtype == torch.float32
    return f0[0].cpu().numpy(), aper[0].cpu().numpy()


@pytest.mark.gpu
def test_tracker_against_the_oracle_around_the_frame_tile(model):
    for case in tile_cases():
        f0, aper = _track_case(model, case)
        _check_track(f0, aper, oracle(*case), case[1], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lag_cases(), ids=lambda c: f"{c[1]}-{dict(c[4])}")
def test_tracker_against_the_oracle_around_the_lag_chunk(model, case):
    f0, aper = _track_case(model, case)
    _check_track(f0, aper, oracle(*case), case[1], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", stage_cases(), ids=lambda c: f"hop{c[4][0][1]}")
def test_tracker_against_the_oracle_around_the_staging_groups(model, case):
    f0, aper = _track_case(model, case)
    _check_track(f0, aper, oracle(*case), case[1], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", win_cases(), ids=lambda c: f"win{c[4][0][1]}")
def test_tracker_against_the_oracle_with_a_window_that_is_no_multiple_of_four(model, case):
    f0, aper = _track_case(model, case)
    _check_track(f0, aper, oracle(*case), case[1], case)


@pytest.mark.gpu
def test_silence_and_noise_are_unvoiced(model):
    n = 40 * 256 + 17
    f0, aper = model.pitch_track(torch.zeros(n, device="cuda"))
    assert f0.shape == (1, 40) and (f0 == 0).all() and (aper == 1).all()
    noise = np.random.default_rng(31).standard_normal(n).astype(np.float32) * 0.1
    f0, aper = model.pitch_track(dev(noise))
    assert (f0 == 0).all() and (aper > 0.15).all()
    o = ref.track(noise, detail=True)
    _check_track(f0[0].cpu().numpy(), aper[0].cpu().numpy(), o, 22050, "noise")


def _garbage(shape, seed):
    """1e30, -1e30 and signalling NaN patterns: what must never be read"""
    g = np.random.default_rng(seed).integers(0, 3, size=shape)
    out = np.where(g == 0, np.float32(1e30), np.float32(-1e30)).astype(np.float32)
    out.view(np.uint32)[g == 2] = 0x7FA00001
    return out


@pytest.mark.gpu
def test_ragged_batches_are_batch_invariant_and_deterministic(model):
    start = int(OFFSET_S * 22050)
    valid = [(2 * FT + 3) * 256 + 255, FT * 256, 255, (FT + 1) * 256 + 255, 30 * 256]
    L = max(valid) + 100
    xs = _garbage((5, L), 37)
    for b, v in enumerate(valid):
        xs[b, :v] = piece("clean", 22050, start if b != 4 else 0, v)
    xd = dev(xs)
    f0, aper = model.pitch_track(xd, valid=valid)
    F_all = L // 256
    assert f0.shape == aper.shape == (5, F_all)
    solo = []
    for b, v in enumerate(valid):
        F = v // 256
        a0, a1 = model.pitch_track(xd[b, :v].clone()) if v >= 1 else (f0[b:b + 1, :0], aper[b:b + 1, :0])
        assert a0.shape == (1, F)
        assert f0[b, :F].cpu().numpy().tobytes() == a0[0].cpu().numpy().tobytes(), b
        assert aper[b, :F].cpu().numpy().tobytes() == a1[0].cpu().numpy().tobytes(), b
        assert (f0[b, F:] == 0).all() and (aper[b, F:] == 1).all()      # behind the row's own frames
        solo.append(a0)
    _check_track(f0[0, : valid[0] // 256].cpu().numpy(), aper[0, : valid[0] // 256].cpu().numpy(), oracle(*tile_cases()[-1]), 22050, "ragged row 0")
    # another row pitch: the same rows in a wider buffer with other garbage behind them
    wide = _garbage((5, L + 333), 41)
    wide[:, :L] = xs
    for b, v in enumerate(valid):
        wide[b, v:] = _garbage((L + 333 - v,), 43 + b)
    g0, g1 = model.pitch_track(dev(wide), valid=valid)
    assert g0[:, :F_all].cpu().numpy().tobytes() == f0.cpu().numpy().tobytes() and g1[:, :F_all].cpu().numpy().tobytes() == aper.cpu().numpy().tobytes()
    h0, h1 = model.pitch_track(xd, valid=valid)
    assert h0.cpu().numpy().tobytes() == f0.cpu().numpy().tobytes() and h1.cpu().numpy().tobytes() == aper.cpu().numpy().tobytes()
    # the records: a row of a ragged comparison equals the comparison of the row alone, and a second call
    deg = xs.copy()
    for b, v in enumerate(valid):
        deg[b, :v] = piece("snr5", 22050, start if b != 4 else 0, v)
    rec = model.pitch(xd, dev(deg), valid=valid)
    assert list(rec["frames"]) == [v // 256 for v in valid] and int(rec["status"][2]) == pt.SHORT
    for b, v in enumerate(valid):
        if v >= 256:
            alone = model.pitch(xd[b, :v].clone(), dev(deg[b, :v]))
            for key in rec:
                assert rec[key][b].tobytes() == alone[key][0].tobytes(), (b, key, rec[key][b], alone[key][0])
    again = model.pitch(xd, dev(deg), valid=valid)
    assert all(again[k].tobytes() == rec[k].tobytes() for k in rec)


def _check_record(got, b, want, where, rmse_bar):
    for key in ("frames", "both_voiced", "ref_voiced", "deg_voiced", "status"):
        assert int(got[key][b]) == want[key], (where, key, {k: got[k][b] for k in got}, want)
    for key, bar in (("rmse_cents", rmse_bar), ("gpe", 1e-9), ("vde", 1e-9)):
        if np.isnan(want[key]):
            assert np.isnan(got[key][b]), (where, key, got[key][b])
        else:
            assert abs(float(got[key][b]) - want[key]) <= bar, (where, key, got[key][b], want[key])
    print(f"{where}: rmse {got['rmse_cents'][b]:.6f} oracle {want['rmse_cents']:.6f} cents; gpe {got['gpe'][b]:.6f}; vde {got['vde'][b]:.6f}; "
          f"frames {got['frames'][b]} both {got['both_voiced'][b]} ref {got['ref_voiced'][b]} deg {got['deg_voiced'][b]}")


@pytest.mark.gpu
@pytest.mark.parametrize("how", DEGRADATIONS)
def test_measure_against_the_oracles_record(model, how):
    n = int(LONG_S * 22050)
    clean, deg = oracle("clean", 22050, 0, n, (("f0_min", 80.0),)), oracle(how, 22050, 0, n)
    assert decided(clean).all() and decided(deg).all()      # (a condition on the inputs, as in the CPU test) so the counts have to be equal
    want = ref.compare(clean["f0"].astype(np.float32), deg["f0"].astype(np.float32))
    got = model.pitch(dev(clean_of(22050)), dev(degraded_of(22050, how)))
    _check_record(got, 0, want, how, 1e-2)
    if how == "sharp3":
        assert 45.0 <= got["rmse_cents"][0] <= 57.0 and got["gpe"][0] <= 0.05, got
    # the comparison alone, fed the oracle's float32 tracks
    rec = pt.compare(dev(clean["f0"].astype(np.float32)), dev(deg["f0"].astype(np.float32)))
    _check_record(rec, 0, want, how + " (oracle tracks)", 1e-9 * want["rmse_cents"])


@pytest.mark.gpu
def test_a_silent_copy_is_unvoiced_and_short_rows_are_short(model):
    x = dev(clean_of(22050))
    got = model.pitch(x, torch.zeros_like(x))
    assert int(got["status"][0]) == pt.UNVOICED and int(got["deg_voiced"][0]) == 0 and int(got["both_voiced"][0]) == 0
    assert got["vde"][0] == got["ref_voiced"][0] / got["frames"][0] and got["ref_voiced"][0] > 0
    assert np.isnan(got["rmse_cents"][0]) and np.isnan(got["gpe"][0])
    got = model.pitch(x[:255].clone(), x[:255].clone())
    assert int(got["status"][0]) == pt.SHORT and int(got["frames"][0]) == 0 and np.isnan(got["vde"][0]) and np.isnan(got["rmse_cents"][0])
    f = torch.tensor([[100.0, 0.0, 200.0, 0.0, 150.0, 300.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], device="cuda")
    g = torch.tensor([[103.0, 50.0, 0.0, 0.0, 300.0, 300.0], [110.0, 0.0, 0.0, 0.0, 0.0, 0.0]], device="cuda")
    rec = pt.compare(f, g, frames=[6, 3])
    _check_record(rec, 0, ref.compare(f[0].cpu().numpy(), g[0].cpu().numpy()), "hand-made", 1e-9)
    _check_record(rec, 1, ref.compare(f[1, :3].cpu().numpy(), g[1, :3].cpu().numpy()), "hand-made unvoiced", 1e-9)


@pytest.mark.gpu
def test_refusals_leave_a_message(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(1, 9000, device="cuda")
    out = torch.zeros(2, 64, device="cuda")
    c = pt._config(None)
    args = (ct.byref(c), out[0].data_ptr(), out[1].data_ptr(), 64, None)
    assert lib.fd_pitch_track(h, None, 1, 9000, None, *args) == _capi.FD_ERR_INVALID and b"null wav" in lib.fd_last_error(h)
    assert lib.fd_pitch_track(h, x.data_ptr(), 0, 9000, None, *args) == _capi.FD_ERR_INVALID and b"B = 0" in lib.fd_last_error(h)
    assert lib.fd_pitch_track(h, x.data_ptr(), 1, 9000, None, ct.byref(c), out[0].data_ptr(), out[1].data_ptr(), 34, None) == _capi.FD_ERR_INVALID
    assert b"out_pitch" in lib.fd_last_error(h)
    bad = pt._config(dict(win=63))
    assert lib.fd_pitch_track(h, x.data_ptr(), 1, 9000, None, ct.byref(bad), out[0].data_ptr(), out[1].data_ptr(), 64, None) == _capi.FD_ERR_INVALID
    assert b"win" in lib.fd_last_error(h)
    rec = torch.empty(48, dtype=torch.uint8, device="cuda")
    assert lib.fd_pitch_compare(h, out[0].data_ptr(), None, 1, 64, None, rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"null f0_deg" in lib.fd_last_error(h)
    with pytest.raises(Exception, match="valid"):
        model.pitch_track(x, valid=[9001])
    with pytest.raises(Exception, match="frames"):
        pt.compare(out[:1], out[1:], frames=[65])
    with pytest.raises(ValueError):
        model.pitch(x, x[:, :100])
    with pytest.raises(Exception, match="win"):
        model.pitch_track(x, win=63)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_counts_buffer_cannot_be_allocated_inside_a_capture():
    """A handle of its own, so that no earlier test has allocated the buffer of the counts: the first call that passes `valid` is
    refused inside a capture, and the handle works on afterwards."""
    import gpu_common
    m = gpu_common.make_model()
    x = torch.zeros(1, 9000, device="cuda")
    m._ready(torch.device("cuda"))                         # the handle and its weights exist; no pitch call has run on it
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(_capi.FastDiffHipError, match="stream capture"):
        with torch.cuda.graph(refused):
            x.mul_(1.0)                                    # (so that the abandoned capture is not empty)
            m.pitch_track(x, valid=[9000])
    torch.cuda.synchronize()
    f0, aper = m.pitch_track(x, valid=[9000])
    whole = m.pitch_track(x)
    assert f0.shape == (1, 35)
    assert f0.cpu().numpy().tobytes() == whole[0].cpu().numpy().tobytes() and aper.cpu().numpy().tobytes() == whole[1].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def tiny_corpus():
    import test_validation
    return test_validation.model_corpus([34, 50, 40], 33).to("cuda")


@pytest.mark.gpu
def test_validator_scores_every_batch(model, tiny_corpus):
    from fastdiff_amd import schedules
    hp = schedules.training_hyperparams()
    kw = dict(corpus=tiny_corpus, batch_size=2, sample_schedule=schedules.noise_schedule_for(4))
    val = fastdiff_amd.Validator(model, hp, pitch=True, **kw)
    first = val.run().result()
    n = tiny_corpus.n_items
    last = (n - 1) // 2 * 2                                # first item of the last batch
    rec = model.pitch(val.wav, val.sampled)
    count = n - last
    for key, name in (("rmse_cents", "f0_rmse_cents"), ("gpe", "gpe"), ("vde", "vde")):
        assert first["item_" + name][last:].tobytes() == rec[key][:count].tobytes(), name
        seen = ~np.isnan(first["item_" + name])
        want = first["item_" + name][seen].mean() if seen.any() else np.nan
        assert (np.isnan(want) and np.isnan(first[name])) or first[name] == pytest.approx(want, abs=1e-12), name
    assert not np.isnan(first["item_vde"]).any()           # 33 frames each: never SHORT
    assert first["pitch_skipped"] == int(np.isnan(first["item_f0_rmse_cents"]).sum())
    print(f"validator: f0_rmse_cents {first['f0_rmse_cents']:.2f} gpe {first['gpe']:.4f} vde {first['vde']:.4f} skipped {first['pitch_skipped']} of {n}")
    second = val.run().result()
    for k in ("item_f0_rmse_cents", "item_gpe", "item_vde", "item_mel_l1", "item_loss"):
        assert second[k].tobytes() == first[k].tobytes(), k
    plain = fastdiff_amd.Validator(model, hp, **kw).run().result()
    assert set(first) == set(plain) | {"f0_rmse_cents", "gpe", "vde", "item_f0_rmse_cents", "item_gpe", "item_vde", "pitch_skipped"}
    assert plain["item_mel_l1"].tobytes() == first["item_mel_l1"].tobytes() and plain["item_loss"].tobytes() == first["item_loss"].tobytes()
    with pytest.raises(ValueError, match="sample_schedule"):
        fastdiff_amd.Validator(model, hp, corpus=tiny_corpus, batch_size=2, pitch=True)


@pytest.mark.gpu
def test_validator_items_equal_the_measure_of_their_own_batch(model):
    """Every batch by hand, on a corpus whose recordings are voiced: the item's values are those of its slot in its own batch."""
    import test_validation as tv
    from fastdiff_amd import schedules
    F, B, lengths = 33, 2, [34, 50, 40, 45, 38]
    mel = tv.synth.synth_mel(3, 1, sum(lengths))[0].T
    items, at = [], 0
    for i, T in enumerate(lengths):
        items.append({"mel": np.ascontiguousarray(mel[at: at + T]), "wav": np.array(clean_of(22050)[2000 + 9000 * i: 2000 + 9000 * i + T * 256]) * 4.0})
        at += T
    corpus = fastdiff_amd.TrainCorpus(items, hop_size=256, max_samples=F * 256, device="cpu").to("cuda")
    val = fastdiff_amd.Validator(model, schedules.training_hyperparams(), corpus=corpus, batch_size=B, sample_schedule=schedules.noise_schedule_for(4), pitch=True)
    assert val.n_batches == 3
    was_training = model.training
    model.eval()
    val.begin()
    want = {}
    for j in range(val.n_batches):
        val.batch(j)
        rec = model.pitch(val.wav, val.sampled)
        for slot, item in enumerate(val.picked.cpu().numpy()[:, 0]):
            if item >= 0:
                want[int(item)] = {k: rec[k][slot] for k in ("rmse_cents", "gpe", "vde", "ref_voiced", "status")}
    got = val.result()
    model.train(was_training)
    assert sorted(want) == list(range(5))
    for item, w in want.items():
        for key, name in (("rmse_cents", "f0_rmse_cents"), ("gpe", "gpe"), ("vde", "vde")):
            expect = w[key] if w["status"] == pt.OK or (key == "vde" and w["status"] == pt.UNVOICED) else np.float64(np.nan)
            assert got["item_" + name][item].tobytes() == np.float64(expect).tobytes(), (item, name, got["item_" + name][item], expect)
    voiced = [int(w["ref_voiced"]) for w in want.values()]
    vde = [float(got["item_vde"][i]) for i in range(5)]
    print(f"validator by hand: ref_voiced {voiced} item_vde {vde} item_f0_rmse_cents {got['item_f0_rmse_cents'].tolist()}")
    assert min(voiced) > 0 and len(set(vde)) >= 3          # the items differ, so a wrong slot would show


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    d = tmp_path_factory.mktemp("pitch_recordings")
    x = clean_of(22050)
    for i, (start, n) in enumerate(((0, 9000), (13230, 12000))):
        wavfile.write(d / f"r{i}.wav", 22050, np.round(x[start: start + n] * 4.0 * 32767.0).astype(np.int16))
    return str(d)


@pytest.mark.gpu
def test_copy_synthesis_reports_what_the_model_measures(model, recordings, tmp_path):
    items = infer.load_wav_inputs(model, recordings, keep_wav=True)
    assert len(items) == 2
    pcm, report = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, pitch=True)
    plain = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3)
    assert set(report) == set(pcm) == set(plain) and all(np.array_equal(pcm[k], plain[k]) for k in pcm)
    rows = infer._step_rows(model, 4, None, None)
    for i, it in enumerate(items):
        t = it["len"] - 1
        mel = it["mel"][:t].transpose(0, 1).unsqueeze(0).contiguous().cuda()
        with torch.no_grad():
            wav = model.sample(mel, rows, ddim=False, seed=3, lens=[t], stream_ids=[i])
        own = model.pitch(it["wav"][: t * 256].clone(), wav.reshape(-1)[: t * 256].clone())
        r = report[it["item_name"]]
        assert set(r) == {"f0_rmse_cents", "gpe", "vde", "pitch_status"}
        assert r["pitch_status"] == pt.STATUS[int(own["status"][0])]
        for key, name in (("rmse_cents", "f0_rmse_cents"), ("gpe", "gpe"), ("vde", "vde")):
            assert np.float64(r[name]).tobytes() == own[key][0].tobytes(), (name, r[name], own[key][0])
    both_pcm, both = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, stoi=True, pitch=True)
    assert all(np.array_equal(both_pcm[k], plain[k]) for k in plain)
    for name, r in both.items():
        assert set(r) == {"stoi", "estoi", "status", "f0_rmse_cents", "gpe", "vde", "pitch_status"}
        assert all(np.float64(r[k]).tobytes() == np.float64(report[name][k]).tobytes() for k in ("f0_rmse_cents", "gpe", "vde"))
    with pytest.raises(ValueError, match="wav"):
        infer.synthesize(model, infer.load_wav_inputs(model, recordings), n_steps=4, pitch=True)
    with pytest.raises(ValueError, match="pitch"):
        infer.synthesize_long(model, items, n_steps=4, pitch=True)
    with pytest.raises(ValueError, match="pitch"):
        infer.synthesize_sharded(model, items, n_steps=4, pitch=True)
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", recordings, "--out_dir", str(tmp_path / "o"), "--pitch"])
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", recordings, "--out_dir", str(tmp_path / "o"), "--from_wav", "--pitch", "--long_form"])
    out = tmp_path / "out"
    infer.main(["--test_input_dir", recordings, "--out_dir", str(out), "--from_wav", "--pitch"])
    lines = open(out / "pitch.tsv").read().strip().split("\n")
    assert len(lines) == 1 + len(items) and lines[0].split("\t") == ["name", "f0_rmse_cents", "gpe", "vde", "status"]
    assert not os.path.exists(out / "stoi.tsv")
