"""The multi-resolution STFT distances on the device (fd_spectral_default_config / _frames / _measure, fastdiff_amd.spectral,
FastDiff.spectral, Validator(spectral=True), infer.synthesize(spectral=True), --spectral) against the float64 oracle
tests/spectral_ref.py, which restates the header's steps 1-7 in numpy and is itself confirmed here with torch.stft in float64.

Bounds against the oracle, per resolution and for the means: |sc| <= 1e-5, |logmag| <= 1e-5 nepers, |lsd| <= 1e-4 dB.  A float32
transform of N terms carries about sqrt(N) 2^-24 (2.7e-6 at N = 2048) of relative error per magnitude, there are two magnitudes per
term, the mean over more than 1e4 bins does not grow it, and one neper is 8.69 dB.  frames, n_res and status: equal.  A copy scores
exactly 0.  A pair alone, in a ragged batch with anything behind it, at another row pitch and from call to call: the same bytes.
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
from fastdiff_amd import _capi, _scores, infer
from fastdiff_amd import spectral as sp
import spectral_ref as ref

NEW = ("fd_spectral_default_config", "fd_spectral_frames", "fd_spectral_measure")
TILE, CHUNK = _capi.FD_SPECTRAL_FRAME_TILE, _capi.FD_SPECTRAL_SUM_CHUNK
RATE, SEED = 22050, 24
BAR_SC, BAR_LOGMAG, BAR_LSD = 1e-5, 1e-5, 1e-4
DEGRADATIONS = ("snr20", "snr5", "clip", "tiny")
DEFAULT = ref.DEFAULT_RES
N_FULL = 22050
# every border of the default configuration: 1024 SHORT, 1025 the smallest OK length, around 2048; the hop-240 frame count stepping at
# 240 k (k = 8: 8, 9, 9 frames = at and one above two frame tiles); 1679: 7 frames, one below; then 255, 256, 257 frames at hop 50: one
# below, at and one above the finaliser's chunk (and 64 frame tiles)
K240 = 2 * TILE
LENGTHS = (1024, 1025, 1200, 2047, 2048, 2049, 240 * K240 - 1, 240 * K240, 240 * K240 + 1, 240 * (K240 - 1) - 1,
           50 * (CHUNK - 2) + 49, 50 * (CHUNK - 1), 50 * CHUNK)
OTHER_CONFIGS = (((1024, 256, 1024),),                      # win = nfft
                 ((512, 50, 241),),                         # odd win: the offset rule
                 ((512, 300, 240),),                        # hop > win: some samples lie in no window
                 DEFAULT + ((2048, 512, 2048),))            # four resolutions
N_OTHER = 9000


@functools.lru_cache(maxsize=None)
def clean_of(n):
    """float32 [n] from a fixed seed at 22050 Hz: harmonics 1 .. 29 of f0(t) = 120 + 30 sin(2 pi 0.7 t) with amplitudes 1 / k, times the
    4 Hz envelope 0.55 + 0.45 sin(2 pi 4 t), scaled to peak 0.2, plus 1e-3 N(0, 1).  A shorter signal is a prefix of a longer one."""
    rng = np.random.default_rng([SEED, RATE])
    N = max(n, N_FULL)
    t = np.arange(N) / RATE
    phase = 2 * np.pi * np.cumsum(120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t)) / RATE
    x = sum(np.sin(k * phase) / k for k in range(1, 30)) * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t))
    x = 0.2 * x / np.abs(x).max() + 1e-3 * rng.standard_normal(N)
    x = x[:n].astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def degraded_of(n, how):
    """clean plus white noise at 20 / 5 dB SNR; a hard clip at +-0.05; 1e-5 N(0, 1) alone"""
    x = clean_of(n).astype(np.float64)
    rng = np.random.default_rng([SEED, 31, DEGRADATIONS.index(how), n])
    if how == "clip":
        y = np.clip(x, -0.05, 0.05)
    elif how == "tiny":
        y = x + 1e-5 * rng.standard_normal(n)
    else:
        y = x + rng.standard_normal(n) * np.sqrt((x ** 2).mean() / 10.0 ** (float(how[3:]) / 10.0))
    y = y.astype(np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def oracle(n, how, res=DEFAULT):
    """The oracle's record of (clean_of, degraded_of); computed once, shared, never changed."""
    out = ref.measure(clean_of(n), degraded_of(n, how), res, detail=True)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def how_for(n):
    return DEGRADATIONS[n % len(DEGRADATIONS)]


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("nfft,hop,win", DEFAULT + ((1024, 256, 1024),))
def test_the_oracles_magnitudes_are_torch_stft_in_float64(nfft, hop, win):
    x = clean_of(N_FULL)
    mine = ref.magnitudes(x, nfft, hop, win)
    spec = torch.stft(torch.from_numpy(x.astype(np.float64)), nfft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True)
    theirs = torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=ref.DEFAULT_FLOOR)).numpy().T
    assert mine.shape == theirs.shape == (ref.frames(N_FULL, hop), nfft // 2 + 1)
    err = np.abs(mine - theirs).max()
    print(f"({nfft}, {hop}, {win}): max |oracle - torch.stft| {err:.2e}")
    assert err <= 1e-12


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for name, value, mine in (("FD_SPECTRAL_MAX_RES", ref.MAX_RES, sp.MAX_RES), ("FD_SPECTRAL_FRAME_TILE", TILE, sp.FRAME_TILE),
                              ("FD_SPECTRAL_SUM_CHUNK", CHUNK, sp.SUM_CHUNK)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == value == mine, name
    stated = int(re.search(r"\}\s*fd_spectral;\s*/\*\s*(\d+) bytes", header).group(1))
    assert sp.RECORD.itemsize == stated == 144 and stated % 8 == 0
    assert ct.sizeof(sp.FdSpectralConfig) == int(re.search(r"\}\s*fd_spectral_config;\s*/\*\s*(\d+) bytes", header).group(1)) == 64
    assert callable(fastdiff_amd.FastDiff.spectral) and "spectral" in fastdiff_amd.__all__ and fastdiff_amd.spectral is sp
    assert (sp.OK, sp.SHORT) == (ref.OK, ref.SHORT) and sp.STATUS == {sp.OK: "OK", sp.SHORT: "SHORT"}
    assert sp.default_config() == {"resolutions": ref.DEFAULT_RES, "floor": ref.DEFAULT_FLOOR}
    assert lib.fd_spectral_default_config(None) == _capi.FD_ERR_INVALID
    assert lib.fd_spectral_frames(-1, 50) == _capi.FD_ERR_INVALID and lib.fd_spectral_frames(10, 0) == _capi.FD_ERR_INVALID


def test_frame_count_is_one_plus_n_over_hop():
    for hop in (16, 50, 120, 240, 256, 300):
        for k in (1, 2, 7, 93):
            for n in (hop * k - 1, hop * k, hop * k + 1):
                assert sp.frames(n, hop) == 1 + n // hop == ref.frames(n, hop), (n, hop)
    assert sp.frames(0, 50) == 1
    with pytest.raises(ValueError):
        sp.frames(100, 0)


def _refusals():
    ok = dict(B=1, L=9000, valid=None, clean=True, degraded=True, rec=True, cfg={})
    return (("a null pointer", dict(ok, degraded=False), b"null degraded"),
            ("a null record", dict(ok, rec=False), b"null rec_dev"),
            ("B = 0", dict(ok, B=0), b"B = 0"),
            ("B = 4097", dict(ok, B=4097), b"B = 4097"),
            ("L = 0", dict(ok, L=0), b"L = 0"),
            ("valid[b] > L", dict(ok, valid=[9001]), b"valid[0] = 9001"),
            ("valid[b] = 0", dict(ok, valid=[0]), b"valid[0] = 0"),
            ("nfft = 768", dict(ok, cfg=dict(resolutions=((768, 50, 240),))), b"nfft[0] = 768"),
            ("win > nfft", dict(ok, cfg=dict(resolutions=((512, 50, 240), (1024, 120, 1025)))), b"win[1] = 1025"),
            ("win = 1", dict(ok, cfg=dict(resolutions=((512, 50, 1),))), b"win[0] = 1"),
            ("hop = 8", dict(ok, cfg=dict(resolutions=((512, 8, 240),))), b"hop[0] = 8"),
            ("hop > nfft", dict(ok, cfg=dict(resolutions=((512, 513, 240),))), b"hop[0] = 513"),
            ("n_res = 5", dict(ok, cfg=dict(resolutions=((512, 50, 240),) * 5)), b"n_res = 5"),
            ("n_res = 0", dict(ok, cfg=dict(resolutions=())), b"n_res = 0"),
            ("floor = 0", dict(ok, cfg=dict(floor=0.0)), b"floor = 0"),
            ("floor = nan", dict(ok, cfg=dict(floor=float("nan"))), b"floor = nan"),
            ("floor = inf", dict(ok, cfg=dict(floor=float("inf"))), b"floor = inf"))


def _config_of(cfg):
    """As spectral._config, but a list of any length: n_res as given, the first four resolutions stored."""
    res = cfg.get("resolutions")
    c = sp._config({k: v for k, v in cfg.items() if k != "resolutions"} | ({} if res is None else {"resolutions": res[:ref.MAX_RES]}))
    if res is not None:
        c.n_res = len(res)
    return c


def _call(lib, h, p, case, stream=None):
    c = _config_of(case["cfg"])
    valid = None if case["valid"] is None else (ct.c_int64 * len(case["valid"]))(*case["valid"])
    return lib.fd_spectral_measure(h, p if case["clean"] else None, p if case["degraded"] else None, case["B"], case["L"], valid, ct.byref(c),
                                   p if case["rec"] else None, stream)


def test_refusals_name_the_value_without_a_handle():
    """The arguments are checked before the handle is looked at (host memory stands in for the device pointers, which nothing may touch),
    so every refusal is read here through fd_last_error(NULL); with every argument in order the NULL handle itself is refused."""
    lib = _capi.load()
    buf = (ct.c_float * 9000)()
    p = ct.addressof(buf)
    for what, case, text in _refusals():
        assert _call(lib, None, p, case) == _capi.FD_ERR_INVALID, what
        msg = lib.fd_last_error(None)
        assert text in msg and b"fd_spectral_measure" in msg, (what, msg)
    fine = dict(B=1, L=9000, valid=[9000], clean=True, degraded=True, rec=True, cfg={})
    assert _call(lib, None, p, fine) == _capi.FD_ERR_INVALID
    assert b"null handle" in lib.fd_last_error(None)
    assert lib.fd_spectral_measure(None, p, p, 1, 9000, None, None, p, None) == _capi.FD_ERR_INVALID      # cfg NULL = the default: fine as well
    assert b"null handle" in lib.fd_last_error(None)
    for what, case, text in _refusals():
        if case["cfg"]:
            assert not ref.accepted(case["cfg"].get("resolutions", DEFAULT), case["cfg"].get("floor", ref.DEFAULT_FLOOR)), what
    assert all(ref.accepted(res) for res in OTHER_CONFIGS + (DEFAULT, ((512, 16, 2),), ((2048, 2048, 2048),)))
    with pytest.raises(TypeError):
        sp._config({"rate": 22050})


def test_the_scores_table_has_the_entry():
    entry = _scores.enabled(spectral=True)
    assert [s.name for s in entry] == ["spectral"] and entry[0].module is sp and entry[0].status_key == "spectral_status"
    assert [(col, key, measured) for col, key, measured, _ in entry[0].columns] == [(k, k, (sp.OK,)) for k in ("mr_sc", "mr_logmag", "lsd_db")]
    assert all(col in sp.RECORD.names and sp.RECORD[col].shape == () for col, _, _, _ in entry[0].columns)
    assert [s.name for s in _scores.enabled(stoi=True, pitch=True)] == ["stoi", "pitch"]
    assert [s.name for s in _scores.enabled(stoi=True, pitch=True, spectral=False)] == ["stoi", "pitch"]
    assert [s.name for s in _scores.enabled(stoi=True, pitch=True, spectral=True)] == ["stoi", "pitch", "spectral"]
    assert _scores.enabled() == []
    with pytest.raises(ValueError, match="spectral"):
        _scores.refuse("somebody", "", spectral=True)
    assert entry[0].kwargs(22050, 256) == {}
    c = entry[0].config(22050, 256)
    assert isinstance(c, sp.FdSpectralConfig) and c.n_res == 3 and c.floor == ref.DEFAULT_FLOOR


def test_oracle_anchors_and_the_inputs_take_every_path():
    """The figures the measure was designed with (another draw of the noise: 3 %), the floor's share, and conditions on the lengths."""
    r20, r5 = oracle(N_FULL, "snr20"), oracle(N_FULL, "snr5")
    assert np.allclose(r20["sc"][:3], (0.0828, 0.0834, 0.0840), rtol=0.03) and np.allclose(r20["logmag"][:3], (1.312, 1.333, 1.399), rtol=0.03), r20
    assert np.allclose(r5["sc"][:3], (0.503, 0.508, 0.514), rtol=0.03), r5
    for how in DEGRADATIONS:
        r = oracle(N_FULL, how)
        assert r["status"] == ref.OK and r["floored"] < 1e-3 and np.isnan(r["sc"][3]) and r["frames"][3] == 0, (how, r)
        assert r["lsd_db"] >= ref.DB_PER_NEPER * r["mr_logmag"] * 0.999      # a root mean square is at least the mean
    same = ref.measure(clean_of(N_FULL), clean_of(N_FULL))
    assert same["mr_sc"] == 0.0 and same["mr_logmag"] == 0.0 and same["lsd_db"] == 0.0
    assert [oracle(n, how_for(n))["status"] for n in LENGTHS[:3]] == [ref.SHORT, ref.OK, ref.OK]
    assert np.isnan(oracle(1024, how_for(1024))["mr_sc"]) and list(oracle(1024, how_for(1024))["frames"]) == [21, 9, 5, 0]
    assert [int(oracle(n, how_for(n))["frames"][2]) for n in LENGTHS[6:10]] == [K240, K240 + 1, K240 + 1, K240 - 1]
    assert [int(oracle(n, how_for(n))["frames"][0]) for n in LENGTHS[10:]] == [CHUNK - 1, CHUNK, CHUNK + 1]
    assert K240 % TILE == 0 and CHUNK % TILE == 0


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, b, want, where):
    assert (int(got["status"][b]), int(got["n_res"][b]), list(got["frames"][b])) == (want["status"], want["n_res"], list(want["frames"])), \
        (where, {k: got[k][b] for k in got}, want)
    k = want["n_res"]
    for key in ("sc", "logmag", "lsd"):
        assert np.isnan(got[key][b][k:]).all(), (where, key, got[key][b])
    if want["status"] != ref.OK:
        assert all(np.isnan(got[key][b]).all() for key in ("sc", "logmag", "lsd", "mr_sc", "mr_logmag", "lsd_db")), (where, {k: got[k][b] for k in got})
        return
    e_sc = max(np.abs(got["sc"][b][:k] - want["sc"][:k]).max(), abs(got["mr_sc"][b] - want["mr_sc"]))
    e_lm = max(np.abs(got["logmag"][b][:k] - want["logmag"][:k]).max(), abs(got["mr_logmag"][b] - want["mr_logmag"]))
    e_lsd = max(np.abs(got["lsd"][b][:k] - want["lsd"][:k]).max(), abs(got["lsd_db"][b] - want["lsd_db"]))
    print(f"{where}: mr_sc {got['mr_sc'][b]:.6f} mr_logmag {got['mr_logmag'][b]:.6f} lsd_db {got['lsd_db'][b]:.5f}; "
          f"max |diff| sc {e_sc:.2e} logmag {e_lm:.2e} lsd {e_lsd:.2e}")
    assert e_sc <= BAR_SC and e_lm <= BAR_LOGMAG and e_lsd <= BAR_LSD, (where, e_sc, e_lm, e_lsd)


@pytest.mark.gpu
def test_every_degradation_at_the_default_configuration(model):
    for how in DEGRADATIONS:
        got = model.spectral(dev(clean_of(N_FULL)), dev(degraded_of(N_FULL, how)))
        _check(got, 0, oracle(N_FULL, how), (N_FULL, how))


@pytest.mark.gpu
def test_lengths_around_every_border(model):
    for n in LENGTHS:
        how = how_for(n)
        got = model.spectral(dev(clean_of(n)), dev(degraded_of(n, how)))
        _check(got, 0, oracle(n, how), (n, how))


@pytest.mark.gpu
@pytest.mark.parametrize("res", OTHER_CONFIGS)
def test_other_configurations(model, res):
    for how in ("snr20", "clip"):
        got = model.spectral(dev(clean_of(N_OTHER)), dev(degraded_of(N_OTHER, how)), resolutions=res)
        _check(got, 0, oracle(N_OTHER, how, res), (N_OTHER, how, res))
    got = model.spectral(dev(clean_of(N_OTHER)), dev(degraded_of(N_OTHER, "snr5")), resolutions=res[:1], floor=1e-3)      # a floor that bites
    want = ref.measure(clean_of(N_OTHER), degraded_of(N_OTHER, "snr5"), res[:1], 1e-3, detail=True)
    assert want["floored"] > 0.05
    _check(got, 0, want, (N_OTHER, "snr5", res[:1], 1e-3))


@pytest.mark.gpu
def test_a_copy_scores_exactly_zero(model):
    for n, res in ((N_FULL, DEFAULT), (1025, DEFAULT), (N_OTHER, OTHER_CONFIGS[3]), (N_OTHER, OTHER_CONFIGS[1])):
        x = dev(clean_of(n))
        got = model.spectral(x, x.clone(), resolutions=res)
        k = len(res)
        assert int(got["status"][0]) == sp.OK
        for key in ("sc", "logmag", "lsd"):
            assert (got[key][0][:k] == 0.0).all(), (n, res, key, got[key][0])
        assert got["mr_sc"][0] == 0.0 and got["mr_logmag"][0] == 0.0 and got["lsd_db"][0] == 0.0
    z = torch.zeros(3000, device="cuda")                   # silence is measured like anything else: every bin at the floor
    got = model.spectral(z, z)
    assert int(got["status"][0]) == sp.OK and got["mr_sc"][0] == 0.0 and got["lsd_db"][0] == 0.0


def _garbage(shape):
    """1e30, a quiet NaN and a signalling NaN pattern in turn"""
    bits = np.array([np.float32(1e30).view(np.uint32), 0x7FC00000, 0x7F800001], np.uint32)
    return np.resize(bits, int(np.prod(shape))).reshape(shape).view(np.float32).copy()


@pytest.mark.gpu
def test_ragged_batches_are_batch_invariant_and_deterministic(model):
    L = 12900
    valid = [L, 50 * (CHUNK - 1), 240 * K240 + 1, 1000, 2049]
    xs, ys = _garbage((5, L)), _garbage((5, L))
    for b, v in enumerate(valid):
        xs[b, :v] = clean_of(v)
        ys[b, :v] = degraded_of(v, how_for(b))
    xd, yd = dev(xs), dev(ys)
    assert xd.view(torch.int32)[3, -1].item() == xs.view(np.int32)[3, -1]      # the patterns arrive as they are
    rec = model.spectral(xd, yd, valid=valid)
    assert list(rec["status"]) == [sp.OK, sp.OK, sp.OK, sp.SHORT, sp.OK]
    for b, v in enumerate(valid):
        _check(rec, b, ref.measure(xs[b, :v], ys[b, :v]), ("ragged", b, v))
    for b, v in enumerate(valid):
        alone = model.spectral(xd[b, :v].clone(), yd[b, :v].clone())
        for key in rec:
            assert rec[key][b].tobytes() == alone[key][0].tobytes(), (b, key, rec[key][b], alone[key][0])
    wide_x, wide_y = _garbage((5, L + 37)), _garbage((5, L + 37))      # another row pitch, the rows in another order
    order = [4, 2, 0, 3, 1]
    for b, src in enumerate(order):
        wide_x[b, :valid[src]] = xs[src, :valid[src]]
        wide_y[b, :valid[src]] = ys[src, :valid[src]]
    wide = model.spectral(dev(wide_x), dev(wide_y), valid=[valid[src] for src in order])
    for b, src in enumerate(order):
        for key in rec:
            assert wide[key][b].tobytes() == rec[key][src].tobytes(), (b, src, key)
    again = model.spectral(xd, yd, valid=valid)
    assert all(again[k].tobytes() == rec[k].tobytes() for k in rec)


@pytest.mark.gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays():
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no table, no scratch yet
    n = 9000
    xa, ya = dev(clean_of(n)).reshape(1, n), dev(degraded_of(n, "snr20")).reshape(1, n)
    xb, yb = dev(clean_of(n)).reshape(1, n), dev(degraded_of(n, "clip")).reshape(1, n)
    lib, h = m._ready(torch.device("cuda"))
    x, y = xa.clone(), ya.clone()
    rec = torch.zeros((1, sp.RECORD.itemsize), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        x.mul_(1.0)                                        # (so that the capture is not empty)
        rc = lib.fd_spectral_measure(h, x.data_ptr(), y.data_ptr(), 1, n, None, None, rec.data_ptr(), m._stream(x.device))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg and b"nfft = 512" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a = m.spectral(xa, ya)                            # outside: uploads the tables and makes the scratch buffer
    want_b = m.spectral(xb, yb)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, lib.fd_spectral_measure(h, x.data_ptr(), y.data_ptr(), 1, n, None, None, rec.data_ptr(), m._stream(x.device)), "fd_spectral_measure")
    graph.replay()
    torch.cuda.synchronize()
    got = sp._record(rec)
    assert all(got[k].tobytes() == want_a[k].tobytes() for k in got)
    x.copy_(xb)
    y.copy_(yb)
    graph.replay()
    torch.cuda.synchronize()
    got = sp._record(rec)
    assert all(got[k].tobytes() == want_b[k].tobytes() for k in got)
    big = torch.zeros(4, 8 * n, device="cuda")
    grow = torch.cuda.CUDAGraph()
    with torch.cuda.graph(grow):
        x.mul_(1.0)
        rc = lib.fd_spectral_measure(h, big.data_ptr(), big.data_ptr(), 4, 8 * n, None, None, rec.data_ptr(), m._stream(x.device))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"scratch buffer" in msg, (rc, msg)
    torch.cuda.synchronize()
    after = m.spectral(xb, yb)                             # the handle works on
    assert all(after[k].tobytes() == want_b[k].tobytes() for k in after)


@pytest.mark.gpu
def test_refusals_leave_their_message_on_the_handle(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(1, 9000, device="cuda")
    rec = torch.empty(sp.RECORD.itemsize, dtype=torch.uint8, device="cuda")
    for what, case, text in _refusals():
        assert _call(lib, h, x.data_ptr(), dict(case, rec=case["rec"] and rec.data_ptr())) == _capi.FD_ERR_INVALID, what
        assert text in lib.fd_last_error(h), (what, lib.fd_last_error(h))
    with pytest.raises(Exception, match="valid"):
        model.spectral(x, x, valid=[9001])
    with pytest.raises(Exception, match="nfft"):
        model.spectral(x, x, resolutions=((768, 50, 240),))
    with pytest.raises(ValueError):
        model.spectral(x, x[:, :100])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_method_and_the_module_function_agree(model):
    n = 9000
    x, y = dev(clean_of(n)), dev(degraded_of(n, "snr5"))
    a, b = model.spectral(x, y), sp.measure(x, y)
    assert set(a) == set(sp.RECORD.names) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    res = OTHER_CONFIGS[0]
    a, b = model.spectral(x, y, resolutions=res, floor=1e-6), sp.measure(x, y, resolutions=res, floor=1e-6)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and int(a["n_res"][0]) == 1


@pytest.fixture(scope="module")
def corpus(model, tmp_path_factory):
    d = tmp_path_factory.mktemp("spectral_corpus")
    for i, n in enumerate((40000, 33000, 52000)):
        wavfile.write(d / f"r{i}.wav", 22050, np.round(clean_of(n) * 4.0 * 32767.0).astype(np.int16))
    return str(d)


@pytest.mark.gpu
def test_validator_scores_every_batch(model, corpus):
    from fastdiff_amd import schedules
    hp = schedules.training_hyperparams()
    data = fastdiff_amd.TrainCorpus.from_wav_dir(model, corpus, max_samples=25600)
    kw = dict(corpus=data, batch_size=2, sample_schedule=schedules.noise_schedule_for(4))
    val = fastdiff_amd.Validator(model, hp, spectral=True, **kw)
    first = val.run().result()
    n = data.n_items
    assert n == 3
    last = (n - 1) // 2 * 2                                # first item of the last batch
    rec = model.spectral(val.wav, val.sampled)
    for key in ("mr_sc", "mr_logmag", "lsd_db"):
        assert first["item_" + key][last:].tobytes() == rec[key][: n - last].tobytes(), key
        assert not np.isnan(first["item_" + key]).any()
        assert first[key] == pytest.approx(first["item_" + key].mean(), abs=1e-12)
    assert first["spectral_skipped"] == 0
    print(f"validator: mr_sc {first['mr_sc']:.4f} mr_logmag {first['mr_logmag']:.4f} lsd_db {first['lsd_db']:.3f}")
    plain = fastdiff_amd.Validator(model, hp, **kw).run().result()
    assert set(plain) == {"loss", "items", "nonfinite", "loss_by_t", "count_by_t", "item_loss", "mel_l1", "item_mel_l1"}
    assert set(first) == set(plain) | {"mr_sc", "mr_logmag", "lsd_db", "item_mr_sc", "item_mr_logmag", "item_lsd_db", "spectral_skipped"}
    for key in plain:
        assert np.asarray(plain[key]).tobytes() == np.asarray(first[key]).tobytes(), key
    with pytest.raises(ValueError, match="sample_schedule"):
        fastdiff_amd.Validator(model, hp, corpus=data, batch_size=2, spectral=True)
    # windows of 4 frames = 1024 samples: every item is SHORT (the windows of a corpus share one length, so either all are or none is)
    tiny = fastdiff_amd.TrainCorpus.from_wav_dir(model, corpus, max_samples=1024)
    short = fastdiff_amd.Validator(model, hp, spectral=True, **dict(kw, corpus=tiny)).run().result()
    assert short["spectral_skipped"] == 3 and np.isnan(short["item_mr_sc"]).all() and np.isnan(short["mr_sc"]) and np.isnan(short["lsd_db"])


@pytest.mark.gpu
def test_copy_synthesis_reports_what_the_model_measures(model, corpus, tmp_path):
    items = infer.load_wav_inputs(model, corpus, keep_wav=True)
    pcm, report = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, spectral=True)
    plain = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3)
    assert set(report) == set(pcm) == set(plain) and all(np.array_equal(pcm[k], plain[k]) for k in pcm)
    rows = infer._step_rows(model, 4, None, None)
    for i, it in enumerate(items):
        t = it["len"] - 1
        mel = it["mel"][:t].transpose(0, 1).unsqueeze(0).contiguous().cuda()
        with torch.no_grad():
            wav = model.sample(mel, rows, ddim=False, seed=3, lens=[t], stream_ids=[i])
        own = model.spectral(it["wav"][: t * 256].clone(), wav.reshape(-1)[: t * 256].clone())
        r = report[it["item_name"]]
        assert set(r) == {"mr_sc", "mr_logmag", "lsd_db", "spectral_status"}
        assert r["spectral_status"] == "OK" == sp.STATUS[int(own["status"][0])]
        for key in ("mr_sc", "mr_logmag", "lsd_db"):
            assert np.float64(r[key]).tobytes() == own[key][0].tobytes(), key
    with pytest.raises(ValueError, match="wav"):
        infer.synthesize(model, infer.load_wav_inputs(model, corpus), n_steps=4, spectral=True)
    with pytest.raises(ValueError, match="spectral"):
        infer.synthesize_long(model, items, n_steps=4, spectral=True)
    with pytest.raises(ValueError, match="spectral"):
        infer.synthesize_sharded(model, items, n_steps=4, spectral=True)
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", corpus, "--out_dir", str(tmp_path / "o"), "--spectral"])
    out, bare = tmp_path / "out", tmp_path / "bare"
    infer.main(["--test_input_dir", corpus, "--out_dir", str(out), "--from_wav", "--spectral"])
    infer.main(["--test_input_dir", corpus, "--out_dir", str(bare), "--from_wav"])
    lines = open(out / "spectral.tsv").read().strip().split("\n")
    assert len(lines) == 1 + len(items) and lines[0].split("\t") == ["name", "mr_sc", "mr_logmag", "lsd_db", "status"]
    assert all(len(line.split("\t")) == 5 and line.split("\t")[4] == "OK" and all(float(v) > 0 for v in line.split("\t")[1:4]) for line in lines[1:])
    assert not os.path.exists(out / "stoi.tsv") and not os.path.exists(out / "pitch.tsv")
    wavs = sorted(f for f in os.listdir(bare) if f.endswith(".wav"))
    assert len(wavs) == len(items) and sorted(os.listdir(out)) == sorted(wavs + ["spectral.tsv"])
    for f in wavs:
        assert open(out / f, "rb").read() == open(bare / f, "rb").read(), f
