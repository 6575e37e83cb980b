"""Mel-cepstral distortion with time alignment on the device (fd_mcd_default_config / fd_mcd_frames / fd_cepstra / fd_dtw /
fd_mcd_measure, fastdiff_amd.mcd, FastDiff.mcd, Validator(mcd=True), infer.synthesize(mcd=True), --mcd) against the float64 oracle
tests/mcd_ref.py, which is itself anchored here: its DCT on scipy's, its alignment on the enumeration of every monotone path.

Bounds.  fd_dtw on the same float32 features: |cost - cost64| <= g cost64 with g = (D + 2) 2^-24 -- each float32 distance (D
differences, D fused multiply-adds, one root) is within g relative of the float64 one, so every path sum is, and so is their minimum.
fd_cepstra: || c - c64 ||_2 <= sqrt(80) 2e-4 ln 10 = 4.1e-3 per frame where every log10-mel is above -4 (the front-end's own bar on such
bins, tests/test_mel_frontend.py; the orthonormal DCT is an isometry and dropping coefficients only shortens the vector).
fd_mcd_measure from the waveforms: each local cost moves by at most 2 eps (eps = that bound) and the float32 distance adds g, a path has
at most Ta + Tb cells: |cost - cost64| <= (Ta + Tb) 2 eps (1 + g) + g cost64; mcd_linear within K 2 eps (1 + g) + g mcd_linear64.
Measured on an MI355X (LABBOOK R31.1): cost 3.7e-8 .. 6.1e-8 relative, || c - c64 ||_2 at most 4.8e-6; each test prints its own figure.
"""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import ROOT, load_golden

import fastdiff_amd
from fastdiff_amd import _capi, _scores, infer
from fastdiff_amd import mcd
import mcd_ref as ref

NEW = ("fd_mcd_default_config", "fd_mcd_frames", "fd_cepstra", "fd_dtw", "fd_mcd_measure")
R, C = _capi.FD_DTW_ROWS, _capi.FD_DTW_COLS
U = 2.0 ** -24
EPS_CEP = np.sqrt(80.0) * 2e-4 * np.log(10.0)
SHAPES = tuple((ta, tb) for ta in (1, 2, R - 1, R, R + 1, 2 * R + 1) for tb in (1, 2, C - 1, C, C + 1)) + ((2 * R + 1, 300), (300, 2 * R + 1))
DIMS = (1, 13, 40)
CEP_LENGTHS = (255, 256, 257, 513, 2 * 256 * 4 + 1)


def gamma(D):
    return (D + 2) * U


@functools.lru_cache(maxsize=None)
def features(seed, T, D):
    """float32 [T, D]: a smooth random walk plus noise, so that neighbouring rows are close and the alignment has something to follow"""
    rng = np.random.default_rng([41, seed, T, D])
    x = (np.cumsum(rng.standard_normal((T, D)), 0) * 0.3 + rng.standard_normal((T, D)) * 0.1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pair_oracle(k, D):
    ta, tb = SHAPES[k]
    a, b = features(2 * k, ta, D), features(2 * k + 1, tb, D)
    c = ref.costs(a, b)
    return c, ref.dtw(c)


@functools.lru_cache(maxsize=None)
def wave(seed, n):
    """float32 [n]: white noise plus three tones, each at amplitude 0.1"""
    rng = np.random.default_rng([43, seed])
    t = np.arange(n) / 22050.0
    x = 0.1 * rng.standard_normal(n) + 0.1 * sum(np.sin(2 * np.pi * f * t + p) for f, p in ((220.0, 0.3), (1310.0, 1.1), (3700.0, 2.0)))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def warp(T, seed):
    """repeat counts 1 .. 3 per row"""
    return np.random.default_rng([47, seed]).integers(1, 4, T)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for name, value, mine in (("FD_MCD_MAX_COEF", ref.MAX_COEF, mcd.MAX_COEF), ("FD_DTW_ROWS", R, mcd.ROWS), ("FD_DTW_COLS", C, mcd.COLS),
                              ("FD_DTW_MAX_ALIGN_CELLS", 1 << 26, mcd.MAX_ALIGN_CELLS), ("FD_MCD_MAX_FRAMES", 1 << 22, mcd.MAX_FRAMES)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == value == mine, name
    assert mcd.RECORD.itemsize == int(re.search(r"\}\s*fd_mcd;\s*/\*\s*(\d+) bytes", header).group(1)) == 48
    assert mcd.DTW_RECORD.itemsize == int(re.search(r"\}\s*fd_dtw_rec;\s*/\*\s*(\d+) bytes", header).group(1)) == 32
    assert ct.sizeof(mcd.FdMcdConfig) == 8
    assert callable(fastdiff_amd.FastDiff.mcd) and "mcd" in fastdiff_amd.__all__ and fastdiff_amd.mcd is mcd
    assert (mcd.OK, mcd.SHORT, mcd.NONFINITE) == (ref.OK, ref.SHORT, ref.NONFINITE)
    assert mcd.STATUS == {mcd.OK: "OK", mcd.SHORT: "SHORT", mcd.NONFINITE: "NONFINITE"}
    assert mcd.default_config() == {"n_coef": ref.DEFAULT_COEF}
    assert lib.fd_mcd_default_config(None) == _capi.FD_ERR_INVALID and lib.fd_mcd_frames(-1) == _capi.FD_ERR_INVALID
    for n in (0, 1, 255, 256, 257, 511, 512, 513, 22050):
        assert mcd.frames(n) == ref.frames(n) == 1 + n // 256
    assert abs(mcd.K_DB - ref.K_DB) == 0 and abs(ref.K_DB - 6.141851463713754) < 1e-14


def test_refusals_name_the_value_without_a_handle():
    lib = _capi.load()
    buf = (ct.c_float * 9000)()
    p = ct.addressof(buf)

    def measure(n_coef=13, reserved=0, B=1, Lc=9000, Ld=9000, valid=None):
        c = mcd.FdMcdConfig(n_coef, reserved)
        v = None if valid is None else (ct.c_int64 * len(valid))(*valid)
        return lib.fd_mcd_measure(None, p, Lc, p, Ld, B, v, None, ct.byref(c), p, None)

    for kw, text in ((dict(n_coef=0), b"n_coef = 0"), (dict(n_coef=41), b"n_coef = 41"), (dict(reserved=7), b"reserved = 7"), (dict(B=0), b"B = 0"),
                     (dict(B=4097), b"B = 4097"), (dict(Ld=0), b"Ld = 0"), (dict(valid=[9001]), b"valid_clean[0] = 9001"), (dict(), b"null handle")):
        assert measure(**kw) == _capi.FD_ERR_INVALID, kw
        msg = lib.fd_last_error(None)
        assert text in msg and b"fd_mcd_measure" in msg, (kw, msg)
    assert measure(n_coef=1) == measure(n_coef=40) == _capi.FD_ERR_INVALID and b"null handle" in lib.fd_last_error(None)
    for n_coef, text in ((0, b"n_coef = 0"), (41, b"n_coef = 41"), (13, b"null handle")):
        assert lib.fd_cepstra(None, p, 1, 9000, None, n_coef, p, 36, None) == _capi.FD_ERR_INVALID
        assert text in lib.fd_last_error(None) and b"fd_cepstra" in lib.fd_last_error(None)
    assert lib.fd_cepstra(None, p, 1, 9000, None, 13, p, 35, None) == _capi.FD_ERR_INVALID and b"T_pitch = 35" in lib.fd_last_error(None)

    def dtw(B=1, D=13, ld=13, pa=10, pb=10, fa=None, fb=None, align=False, ap=0):
        fa = None if fa is None else (ct.c_int64 * len(fa))(*fa)
        fb = None if fb is None else (ct.c_int64 * len(fb))(*fb)
        return lib.fd_dtw(None, p, p, B, D, ld, pa, pb, fa, fb, p, p if align else None, ap, None)

    for kw, text in ((dict(D=0), b"D = 0"), (dict(D=41, ld=41), b"D = 41"), (dict(ld=12), b"ld = 12"), (dict(pa=0), b"pitch_a = 0"), (dict(fa=[11]), b"frames_a[0] = 11"),
                     (dict(fb=[0]), b"frames_b[0] = 0"), (dict(align=True, ap=9), b"align_pitch = 9"),
                     (dict(pa=8193, pb=8193, align=True, ap=8193), b"8193 x 8193 = 67125249 cells"), (dict(), b"null handle")):
        assert dtw(**kw) == _capi.FD_ERR_INVALID, kw
        msg = lib.fd_last_error(None)
        assert text in msg and b"fd_dtw" in msg, (kw, msg)
    assert dtw(pa=8192, pb=8192, align=True, ap=8192) == _capi.FD_ERR_INVALID and b"null handle" in lib.fd_last_error(None)      # 2^26 cells: accepted
    with pytest.raises(TypeError):
        mcd._config({"rate": 22050})
    with pytest.raises(ValueError):
        mcd._config({"variant": "hifigan"})


def test_the_scores_table_ends_in_the_entry():
    entry = _scores.enabled(mcd=True)
    assert [s.name for s in entry] == ["mcd"] and entry[0].module is mcd and entry[0].status_key == "mcd_status"
    assert [(col, key, measured, fmt) for col, key, measured, fmt in entry[0].columns] == [(k, k, (mcd.OK,), ".4f") for k in ("mcd_dtw", "mcd_linear")]
    assert all(col in mcd.RECORD.names for col, _, _, _ in entry[0].columns)
    assert [s.name for s in _scores.enabled(stoi=True, pitch=True, spectral=True, mcd=True)] == ["stoi", "pitch", "spectral", "mcd"]
    assert _scores.SCORES[-1].name == "mcd"
    with pytest.raises(ValueError, match="mcd"):
        _scores.refuse("somebody", "", mcd=True)
    c, variant = entry[0].config(22050, 256)
    assert isinstance(c, mcd.FdMcdConfig) and c.n_coef == 13 and variant == "pwg" and entry[0].kwargs(22050, 256) == {}


def test_the_oracles_dct_is_scipys():
    from scipy.fft import dct
    x = np.random.default_rng(1).standard_normal((80, 7))
    assert np.abs(ref.dct_matrix() @ x - dct(x, type=2, norm="ortho", axis=0)).max() <= 1e-13
    assert np.abs(ref.dct_matrix() @ ref.dct_matrix().T - np.eye(80)).max() <= 1e-13


@pytest.mark.parametrize("shape", ((4, 5), (5, 3)))
def test_the_oracles_alignment_is_the_best_of_every_monotone_path(shape):
    for seed in range(5):
        c = np.random.default_rng([3, seed]).random(shape)
        r = ref.dtw(c)
        assert r["cost"] == pytest.approx(ref.brute_force(c), rel=1e-14)
        path = ref.backtrack(r["dirs"])
        assert ref.is_monotone_path(path, *shape) and ref.path_cost(c, path) == pytest.approx(r["cost"], rel=1e-14)
        assert r["path_len"] == len(path) and r["n_diag"] == sum(1 for p, q in zip(path, path[1:]) if q[0] - p[0] == 1 and q[1] - p[1] == 1)


def test_the_oracle_follows_a_warp_exactly_in_both_orders():
    x = features(99, 37, 13)
    rep = warp(37, 1)
    y = np.repeat(x, rep, axis=0)
    assert y.shape[0] == rep.sum() and 37 < y.shape[0] <= 111
    start = np.concatenate([[0], np.cumsum(rep)[:-1]])
    r = ref.dtw(ref.costs(x, y))
    path = ref.backtrack(r["dirs"])
    assert r["cost"] == 0.0 and path == [(i, start[i] + k) for i in range(37) for k in range(rep[i])]
    assert r["path_len"] == len(y) and r["n_diag"] == 36 and list(ref.align_from_path(path, 37)) == list(start)
    t = ref.dtw(ref.costs(y, x))
    assert t["cost"] == 0.0 and ref.backtrack(t["dirs"]) == [(j, i) for i, j in path] and (t["path_len"], t["n_diag"]) == (len(y), 36)


def tie_path(ta, tb):
    """The path of the tie rule on equal costs: a trace-back from the end takes the diagonal while it can, so the path runs along row 0
    (or column 0) first and then down the diagonal into the end."""
    if tb >= ta:
        return [(0, j) for j in range(tb - ta + 1)] + [(i, tb - ta + i) for i in range(1, ta)]
    return [(i, 0) for i in range(ta - tb + 1)] + [(ta - tb + j, j) for j in range(1, tb)]


def test_the_tie_rule_on_equal_costs():
    for ta, tb in ((5, 9), (9, 5), (4, 4), (1, 3), (3, 1)):
        r = ref.dtw(np.zeros((ta, tb)))
        assert ref.backtrack(r["dirs"]) == tie_path(ta, tb), (ta, tb)
        assert (r["cost"], r["path_len"], r["n_diag"]) == (0.0, max(ta, tb), min(ta, tb) - 1)
    assert tie_path(5, 9) == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (2, 6), (3, 7), (4, 8)]


def test_the_oracle_is_the_executed_references_accumulated_matrix():
    """tests/golden/dtw_reference.npz (tools/gen_dtw_reference.py): the reference's utils/pitch_distance.py time_warp, executed with
    stand-ins for numba and matplotlib.  It never counts row 0 or column 0, so its dtw[1:, 1:] is the recurrence on costs[1:, 1:]."""
    g = load_golden("dtw_reference")
    for k in range(4):
        c, d = g[f"costs{k}"], g[f"dtw{k}"]
        assert d.shape == c.shape and d[0, 0] == 0.0 and np.isinf(d[0, 1:]).all() and np.isinf(d[1:, 0]).all()
        assert np.array_equal(ref.dtw(c[1:, 1:])["acc"], d[1:, 1:]), k


def test_the_carried_counts_are_the_back_tracked_ones():
    for k in (7, 12, 17, 30, 31):
        c, r = pair_oracle(k, 13)
        path = ref.backtrack(r["dirs"])
        assert ref.is_monotone_path(path, *c.shape) and r["path_len"] == len(path) == sum(c.shape) - 1 - r["n_diag"]
        assert r["n_diag"] == sum(1 for p, q in zip(path, path[1:]) if q[0] - p[0] == 1 and q[1] - p[1] == 1)
        assert ref.path_cost(c, path) == pytest.approx(r["cost"], rel=1e-13)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(rows, T, D, fill=np.nan):
    out = np.full((len(rows), T, D), fill, np.float32)      # what lies behind a pair's own rows is never read: NaN there would show
    for b, x in enumerate(rows):
        out[b, : len(x)] = x
    return out


def _check_alignment(where, c, want, rec, b, al, D):
    """The record and align_out of pair b against the float64 costs c and the oracle's record."""
    ta, tb = c.shape
    g = gamma(D)
    cost, plen, nd = float(rec["cost"][b]), int(rec["path_len"][b]), int(rec["n_diag"][b])
    assert (int(rec["status"][b]), int(rec["frames_a"][b]), int(rec["frames_b"][b])) == (mcd.OK, ta, tb), where
    assert abs(cost - want["cost"]) <= g * want["cost"], (where, cost, want["cost"])
    a = al[b, :ta].astype(np.int64)
    gaps = np.diff(a)
    # a monotone path from (0, 0) to the end: row i covers the columns a[i] .. e_i, the next row starts at e_i (a step in i) or e_i + 1
    # (a diagonal step).  Every such path has Ta + Tb - 1 - n_diag cells; n_diag of the transitions with a gap are diagonal.
    assert a[0] == 0 and (gaps >= 0).all() and a[-1] <= tb - 1 and (al[b, ta:] == -1).all(), (where, a)
    assert plen == ta + tb - 1 - nd and 0 <= nd <= int((gaps >= 1).sum()), (where, plen, nd)
    # the cheapest path that fits align_out, path_len and n_diag: the cells every such path has, plus the cheapest corners for the
    # transitions with a gap that are not diagonal
    base = c[ta - 1, a[-1]:].sum() + sum(c[i, a[i]: a[i + 1]].sum() for i in range(ta - 1)) + sum(c[i, a[i + 1]] for i in range(ta - 1) if gaps[i] == 0)
    corners = np.sort(np.array([c[i, a[i + 1]] for i in range(ta - 1) if gaps[i] >= 1]))
    fits = base + corners[: int((gaps >= 1).sum()) - nd].sum()
    assert fits <= want["cost"] * (1 + 2 * g) + 1e-300, (where, fits, want["cost"])
    return abs(cost - want["cost"]) / max(want["cost"], 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_dtw_against_the_oracle_at_every_block_and_tile_border(D):
    """Every shape as one pair of one ragged batch, with align_out."""
    As, Bs = [features(2 * k, ta, D) for k, (ta, tb) in enumerate(SHAPES)], [features(2 * k + 1, tb, D) for k, (ta, tb) in enumerate(SHAPES)]
    Ta, Tb = max(len(x) for x in As), max(len(x) for x in Bs)
    rec, al = mcd.dtw(dev(_padded(As, Ta, D)), dev(_padded(Bs, Tb, D)), frames_a=[len(x) for x in As], frames_b=[len(x) for x in Bs], align=True)
    al = al.cpu().numpy()
    worst = 0.0
    for k, shape in enumerate(SHAPES):
        c, want = pair_oracle(k, D)
        worst = max(worst, _check_alignment((D, shape), c, want, rec, k, al, D))
        if shape[0] == shape[1]:
            assert rec["cost"][k] <= np.trace(c) * (1 + gamma(D)), (D, shape)
    print(f"D = {D}: max |cost - cost64| / cost64 = {worst:.2e} (bound {gamma(D):.2e}) over {len(SHAPES)} shapes")
    # the arguments swapped: the same cost
    swapped = mcd.dtw(dev(_padded(Bs, Tb, D)), dev(_padded(As, Ta, D)), frames_a=[len(x) for x in Bs], frames_b=[len(x) for x in As])
    for k in range(len(SHAPES)):
        assert abs(swapped["cost"][k] - rec["cost"][k]) <= gamma(D) * rec["cost"][k], (D, SHAPES[k])
        assert (int(swapped["frames_a"][k]), int(swapped["frames_b"][k])) == SHAPES[k][::-1]


@pytest.mark.gpu
def test_dtw_follows_warps_and_the_tie_rule_exactly():
    D = 13
    x = features(99, 2 * R + 1, D)
    rep = warp(len(x), 2)
    y = np.repeat(x, rep, axis=0)
    start = np.concatenate([[0], np.cumsum(rep)[:-1]])
    rec, al = mcd.dtw(dev(x[None]), dev(y[None]), align=True)
    assert (rec["cost"][0], int(rec["path_len"][0]), int(rec["n_diag"][0]), int(rec["status"][0])) == (0.0, len(y), len(x) - 1, mcd.OK)
    assert list(al.cpu().numpy()[0]) == list(start)
    rec, al = mcd.dtw(dev(y[None]), dev(x[None]), align=True)
    assert (rec["cost"][0], int(rec["path_len"][0]), int(rec["n_diag"][0])) == (0.0, len(y), len(x) - 1)
    assert list(al.cpu().numpy()[0]) == list(np.repeat(np.arange(len(x)), rep))
    for ta, tb in ((5, 9), (9, 5), (R + 3, C + 70), (C + 70, R + 3)):                   # all rows equal: the tie-rule path
        one = np.ones((1, max(ta, tb), D), np.float32)
        rec, al = mcd.dtw(dev(one[:, :ta]), dev(one[:, :tb]), align=True)
        assert (rec["cost"][0], int(rec["path_len"][0]), int(rec["n_diag"][0])) == (0.0, max(ta, tb), min(ta, tb) - 1), (ta, tb)
        assert list(al.cpu().numpy()[0]) == list(ref.align_from_path(tie_path(ta, tb), ta)), (ta, tb)
    x = dev(features(5, R + 9, 40)[None])                                               # a copy
    rec = mcd.dtw(x, x.clone())
    assert (rec["cost"][0], int(rec["path_len"][0]), int(rec["n_diag"][0])) == (0.0, R + 9, R + 8)


@pytest.mark.gpu
def test_a_feature_that_is_not_finite_marks_its_pair_alone():
    D, ta, tb = 13, R + 5, C + 9
    As, Bs = np.stack([features(60 + b, ta, D) for b in range(3)]), np.stack([features(70 + b, tb, D) for b in range(3)])
    clean, al0 = mcd.dtw(dev(As), dev(Bs), align=True)
    for which, (i, d), bad in (("a", (0, 0), np.nan), ("a", (ta - 1, D - 1), np.inf), ("a", (R, 3), -np.inf), ("b", (C, 0), np.nan), ("b", (tb - 1, D - 1), np.inf)):
        a, b = As.copy(), Bs.copy()
        (a if which == "a" else b)[1, i, d] = bad
        rec, al = mcd.dtw(dev(a), dev(b), align=True)
        assert int(rec["status"][1]) == mcd.NONFINITE and np.isnan(rec["cost"][1]) and (rec["path_len"][1], rec["n_diag"][1]) == (0, 0), (which, i, d)
        assert (al.cpu().numpy()[1] == -1).all()
        for k in (0, 2):
            assert all(rec[key][k].tobytes() == clean[key][k].tobytes() for key in rec) and torch.equal(al[k], al0[k]), (which, i, d, k)


def _cep_check(where, got, wav, n_coef, variant="pwg", bank=None):
    lm = ref.log_mel(wav, variant, bank) / np.log(10.0)
    assert lm.min() > -4.0, (where, lm.min())
    want = ref.cepstra(wav, n_coef, variant, bank)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    err = np.sqrt(((got.astype(np.float64) - want) ** 2).sum(-1)).max()
    assert err <= EPS_CEP, (where, err)
    return err


@pytest.mark.gpu
def test_cepstra_against_the_oracle(model):
    worst = 0.0
    for n in CEP_LENGTHS:
        for n_coef in (13, 40):
            got = mcd.cepstra(dev(wave(n, n)), n_coef=n_coef).cpu().numpy()
            assert got.shape == (1, mcd.frames(n), n_coef)
            worst = max(worst, _cep_check((n, n_coef), got[0], wave(n, n), n_coef))
    L = max(CEP_LENGTHS)
    batch = np.full((len(CEP_LENGTHS), L), np.nan, np.float32)       # nothing at or behind a row's own samples is read
    for b, n in enumerate(CEP_LENGTHS):
        batch[b, :n] = wave(n, n)
    got = mcd.cepstra(dev(batch), valid=list(CEP_LENGTHS)).cpu().numpy()
    for b, n in enumerate(CEP_LENGTHS):
        T = mcd.frames(n)
        worst = max(worst, _cep_check(("ragged", n), got[b, :T], wave(n, n), 13))
        assert (got[b, T:] == 0.0).all()
        alone = mcd.cepstra(dev(wave(n, n))).cpu().numpy()
        assert alone[0].tobytes() == got[b, :T].tobytes(), n
    one = mcd.cepstra(dev(wave(3, 3000)), n_coef=1).cpu().numpy()
    assert one.tobytes() == mcd.cepstra(dev(wave(3, 3000)), n_coef=5).cpu().numpy()[:, :, :1].tobytes()
    # the tacotron front-end: 512 samples are too short (NaN rows), 513 are measured
    short = mcd.cepstra(dev(wave(4, 512)), variant="tacotron").cpu().numpy()
    assert short.shape == (1, 3, 13) and np.isnan(short).all()
    got = mcd.cepstra(dev(wave(4, 513)), variant="tacotron").cpu().numpy()
    worst = max(worst, _cep_check(("tacotron", 513), got[0], wave(4, 513), 13, "tacotron"))
    got = mcd.cepstra(dev(wave(5, 3000)), variant="tacotron", n_coef=40).cpu().numpy()
    worst = max(worst, _cep_check(("tacotron", 3000), got[0], wave(5, 3000), 40, "tacotron"))
    # a user's filter bank on the module's handle
    import mel_frontend as mf
    bank = (mf.mel_basis(fmin=0.0, fmax=11025.0) * 0.5).astype(np.float32)
    import gpu_common
    m = gpu_common.make_model()
    m.set_mel_filterbank(bank)
    got = mcd._cepstra(*m._wave_call(dev(wave(6, 3000))), dev(wave(6, 3000)), None, 13, "pwg").cpu().numpy()
    worst = max(worst, _cep_check(("bank", 3000), got[0], wave(6, 3000), 13, bank=bank))
    assert np.abs(got[0] - mcd.cepstra(dev(wave(6, 3000))).cpu().numpy()[0]).max() > 0.01
    print(f"cepstra: max ||c - c64||_2 per frame = {worst:.2e} (bound {EPS_CEP:.2e})")


def _rec_check(where, got, b, want):
    Ta, Tb = want["frames_clean"], want["frames_degraded"]
    assert (int(got["status"][b]), int(got["frames_clean"][b]), int(got["frames_degraded"][b])) == (mcd.OK, Ta, Tb), where
    g = gamma(13)
    e = 2 * EPS_CEP * (1 + g)
    assert abs(got["cost"][b] - want["cost"]) <= (Ta + Tb) * e + g * want["cost"], (where, got["cost"][b], want["cost"])
    assert abs(got["mcd_linear"][b] - want["mcd_linear"]) <= ref.K_DB * e + g * want["mcd_linear"], (where, got["mcd_linear"][b], want["mcd_linear"])
    assert int(got["path_len"][b]) == want["path_len"] and int(got["n_diag"][b]) == want["n_diag"], (where, got["path_len"][b], want["path_len"])
    assert abs(got["mcd_dtw"][b] - want["mcd_dtw"]) <= ref.K_DB * ((Ta + Tb) * e + g * want["cost"]) / want["path_len"], where
    assert got["mcd_dtw"][b] == ref.K_DB * got["cost"][b] / got["path_len"][b]


@pytest.mark.gpu
def test_measure_is_its_three_layers_and_meets_the_oracle(model):
    n = 256 * 100 + 17
    x = wave(10, n)
    cases = {"noisy": (x, (x + 0.02 * wave(11, n)).astype(np.float32)), "delayed": (x[512:], x[:-512]), "shorter": (x, (x[: n - 700] * 0.8).astype(np.float32))}
    for name, (a, b) in cases.items():
        got = model.mcd(dev(a), dev(b))
        ca, cb = mcd.cepstra(dev(a)), mcd.cepstra(dev(b))
        w = mcd.dtw(ca, cb)
        for key in ("cost", "path_len", "n_diag"):
            assert got[key][0].tobytes() == w[key][0].tobytes(), (name, key)
        T = min(ca.shape[1], cb.shape[1])
        c32 = (ca[0, :T].cpu().numpy(), cb[0, :T].cpu().numpy())
        lin = ref.K_DB * np.sqrt(((c32[0].astype(np.float64) - c32[1]) ** 2).sum(-1)).mean()
        assert abs(got["mcd_linear"][0] - lin) <= gamma(13) * lin, name
        _rec_check(name, got, 0, ref.measure(a, b))
        print(f"{name}: mcd_dtw {got['mcd_dtw'][0]:.4f} dB, mcd_linear {got['mcd_linear'][0]:.4f} dB, path_len {got['path_len'][0]}, n_diag {got['n_diag'][0]}")
    a, b = cases["delayed"]                                     # a delay of exactly two frames: the alignment takes it out
    got = model.mcd(dev(a), dev(b))
    T = mcd.frames(len(a))
    assert got["mcd_dtw"][0] < got["mcd_linear"][0] / 4 and got["n_diag"][0] >= T - 4, got
    same = model.mcd(dev(x), dev(x.copy()))
    T = mcd.frames(n)
    assert (same["mcd_dtw"][0], same["mcd_linear"][0], same["cost"][0], int(same["path_len"][0]), int(same["n_diag"][0]), int(same["status"][0])) == (0.0, 0.0, 0.0, T, T - 1, mcd.OK)
    # statuses: the tacotron front-end with at most 512 samples; a sample that is not finite
    short = model.mcd(dev(x[:512]), dev(x[:3000]), variant="tacotron")
    assert int(short["status"][0]) == mcd.SHORT and np.isnan(short["mcd_dtw"][0]) and np.isnan(short["mcd_linear"][0]) and short["path_len"][0] == 0
    y = x[:3000].copy()
    y[1000] = np.inf
    bad = model.mcd(dev(x[:3000]), dev(y))
    assert int(bad["status"][0]) == mcd.NONFINITE and np.isnan(bad["mcd_dtw"][0]) and np.isnan(bad["cost"][0])
    z = (x[:3000] + 0.05 * wave(12, 3000)).astype(np.float32)
    taco = model.mcd(dev(x[:3000]), dev(z), variant="tacotron", n_coef=20)
    want = ref.measure(x[:3000], z, 20, "tacotron")
    assert int(taco["status"][0]) == mcd.OK and abs(taco["mcd_linear"][0] - want["mcd_linear"]) <= ref.K_DB * 2 * EPS_CEP * 1.001 + gamma(20) * want["mcd_linear"]


@pytest.mark.gpu
def test_ragged_batches_are_batch_invariant_and_deterministic(model):
    Lc, Ld = 256 * 300 + 5, 256 * 280
    vc, vd = [Lc, 2049, 255, 256 * R + 1, 70000], [Ld, 1500, 700, 256 * R - 3, 256 * 270 + 1]
    xs, ys = np.full((5, Lc), np.nan, np.float32), np.full((5, Ld), np.nan, np.float32)
    for b in range(5):
        xs[b, : vc[b]] = wave(20 + b, vc[b])
        ys[b, : vd[b]] = 0.7 * wave(20 + b, max(vc[b], vd[b]))[: vd[b]] + 0.01 * wave(30 + b, vd[b])
    xd, yd = dev(xs), dev(ys)
    rec = model.mcd(xd, yd, valid=vc, valid_degraded=vd)
    assert list(rec["status"]) == [mcd.OK] * 5 and list(rec["frames_clean"]) == [mcd.frames(v) for v in vc] and list(rec["frames_degraded"]) == [mcd.frames(v) for v in vd]
    for b in range(5):
        alone = model.mcd(xd[b, : vc[b]].clone(), yd[b, : vd[b]].clone())
        for key in rec:
            assert rec[key][b].tobytes() == alone[key][0].tobytes(), (b, key, rec[key][b], alone[key][0])
    again = model.mcd(xd, yd, valid=vc, valid_degraded=vd)
    assert all(again[k].tobytes() == rec[k].tobytes() for k in rec)
    # fd_dtw: a pair alone, in a ragged batch, at a wider ld and off the 16-byte alignment: the same bytes
    D = 13
    As, Bs = [features(80 + b, t, D) for b, t in enumerate((R + 1, 7, 2 * R))], [features(90 + b, t, D) for b, t in enumerate((C + 1, 300, C))]
    fa, fb = [len(x) for x in As], [len(x) for x in Bs]
    full, al = mcd.dtw(dev(_padded(As, max(fa), D)), dev(_padded(Bs, max(fb), D)), frames_a=fa, frames_b=fb, align=True)
    for b in range(3):
        alone, al1 = mcd.dtw(dev(As[b][None]), dev(Bs[b][None]), align=True)
        assert all(full[k][b].tobytes() == alone[k][0].tobytes() for k in full) and torch.equal(al[b, : fa[b]], al1[0]), b
    ld = 24
    wa, wb = torch.full((1 + 3 * max(fa) * ld,), float("nan"), device="cuda"), torch.full((1 + 3 * max(fb) * ld,), float("nan"), device="cuda")
    va = torch.as_strided(wa, (3, max(fa), D), (max(fa) * ld, ld, 1), 1)
    vb = torch.as_strided(wb, (3, max(fb), D), (max(fb) * ld, ld, 1), 1)
    va.copy_(dev(_padded(As, max(fa), D)))
    vb.copy_(dev(_padded(Bs, max(fb), D)))
    lib, h, stream = model._wave_call(va)
    wide, alw = mcd._dtw(lib, h, stream, va, vb, fa, fb, True)
    assert va.data_ptr() % 16 == 4 and mcd._rows3(va, "a")[4] == ld
    assert all(full[k].tobytes() == wide[k].tobytes() for k in full) and torch.equal(al, alw)


@pytest.mark.gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays():
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no table, no scratch yet
    n = 9000
    xa, ya = dev(wave(1, n)).reshape(1, n), dev(0.5 * wave(2, n)).reshape(1, n)
    xb, yb = dev(wave(3, n)).reshape(1, n), dev(wave(3, n) + 0.01 * wave(4, n)).reshape(1, n)
    lib, h = m._ready(torch.device("cuda"))
    x, y = xa.clone(), ya.clone()
    rec = torch.zeros((1, mcd.RECORD.itemsize), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        x.mul_(1.0)                                        # (so that the capture is not empty)
        rc = lib.fd_mcd_measure(h, x.data_ptr(), n, y.data_ptr(), n, 1, None, None, None, rec.data_ptr(), m._stream(x.device))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a = m.mcd(xa, ya)                                 # outside: uploads the tables and makes the scratch buffer
    want_b = m.mcd(xb, yb)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, lib.fd_mcd_measure(h, x.data_ptr(), n, y.data_ptr(), n, 1, None, None, None, rec.data_ptr(), m._stream(x.device)), "fd_mcd_measure")
    graph.replay()
    torch.cuda.synchronize()
    got = mcd._record(rec)
    assert all(got[k].tobytes() == want_a[k].tobytes() for k in got)
    x.copy_(xb)
    y.copy_(yb)
    graph.replay()
    torch.cuda.synchronize()
    got = mcd._record(rec)
    assert all(got[k].tobytes() == want_b[k].tobytes() for k in got)
    big = torch.zeros(4, 8 * n, device="cuda")
    grow = torch.cuda.CUDAGraph()
    with torch.cuda.graph(grow):
        x.mul_(1.0)
        rc = lib.fd_mcd_measure(h, big.data_ptr(), 8 * n, big.data_ptr(), 8 * n, 4, None, None, None, rec.data_ptr(), m._stream(x.device))
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"scratch buffer" in msg, (rc, msg)
    torch.cuda.synchronize()
    after = m.mcd(xb, yb)                                  # the handle works on
    assert all(after[k].tobytes() == want_b[k].tobytes() for k in after)


@pytest.mark.gpu
def test_refusals_leave_their_message_on_the_handle_and_the_method_is_the_module_function(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(1, 9000, device="cuda")
    rec = torch.empty(mcd.RECORD.itemsize, dtype=torch.uint8, device="cuda")
    c = mcd.FdMcdConfig(41, 0)
    assert lib.fd_mcd_measure(h, x.data_ptr(), 9000, x.data_ptr(), 9000, 1, None, None, ct.byref(c), rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"n_coef = 41" in lib.fd_last_error(h)
    with pytest.raises(Exception, match="valid_clean"):
        model.mcd(x, x, valid=[9001])
    with pytest.raises(Exception, match="n_coef = 0"):
        model.mcd(x, x, n_coef=0)
    with pytest.raises(Exception, match="D = 41"):
        mcd.dtw(torch.zeros(1, 4, 41, device="cuda"), torch.zeros(1, 4, 41, device="cuda"))
    with pytest.raises(Exception, match="cells"):
        mcd.dtw(torch.zeros(1, 8193, 1, device="cuda"), torch.zeros(1, 8193, 1, device="cuda"), align=True)
    with pytest.raises(ValueError):
        model.mcd(x, torch.zeros(2, 9000, device="cuda"))
    torch.cuda.synchronize()
    n = 9000
    a, b = dev(wave(1, n)), dev(0.5 * wave(2, n + 300))
    p, q = model.mcd(a, b), mcd.measure(a, b)
    assert set(p) == set(mcd.FIELDS) and all(p[k].tobytes() == q[k].tobytes() for k in p)
    p, q = model.mcd(a, b, n_coef=24), mcd.measure(a, b, n_coef=24)
    assert all(p[k].tobytes() == q[k].tobytes() for k in p)


@pytest.fixture(scope="module")
def corpus(model, tmp_path_factory):
    d = tmp_path_factory.mktemp("mcd_corpus")
    for i, n in enumerate((40000, 33000)):
        wavfile.write(d / f"r{i}.wav", 22050, np.round(wave(50 + i, n) * 32767.0).astype(np.int16))
    return str(d)


@pytest.mark.gpu
def test_validator_scores_every_window(model, corpus):
    from fastdiff_amd import schedules
    hp = schedules.training_hyperparams()
    data = fastdiff_amd.TrainCorpus.from_wav_dir(model, corpus, max_samples=12800)
    kw = dict(corpus=data, batch_size=2, sample_schedule=schedules.noise_schedule_for(4))
    val = fastdiff_amd.Validator(model, hp, mcd=True, **kw)
    first = val.run().result()
    n = data.n_items
    assert n == 2 and first["mcd_skipped"] == 0
    rec = model.mcd(val.wav, val.sampled)
    for key in ("mcd_dtw", "mcd_linear"):
        assert first["item_" + key].tobytes() == rec[key][:n].tobytes(), key
        assert not np.isnan(first["item_" + key]).any() and first[key] == pytest.approx(first["item_" + key].mean(), abs=1e-12)
    assert (first["item_mcd_dtw"] <= first["item_mcd_linear"] * (1 + 1e-12)).all()      # Ta = Tb: the diagonal is one of the paths and no path has fewer cells
    with pytest.raises(ValueError, match="sample_schedule"):
        fastdiff_amd.Validator(model, hp, corpus=data, batch_size=2, mcd=True)


@pytest.mark.gpu
def test_copy_synthesis_reports_what_the_model_measures(model, corpus, tmp_path):
    items = infer.load_wav_inputs(model, corpus, keep_wav=True)
    with pytest.raises(ValueError, match="mcd"):
        infer.synthesize_long(model, items, n_steps=4, mcd=True)
    with pytest.raises(ValueError, match="mcd"):
        infer.synthesize_sharded(model, items, n_steps=4, mcd=True)
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", corpus, "--out_dir", str(tmp_path / "o"), "--mcd"])
    pcm, report = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, mcd=True)
    rows = infer._step_rows(model, 4, None, None)
    for i, it in enumerate(items):
        t = it["len"] - 1
        mel = it["mel"][:t].transpose(0, 1).unsqueeze(0).contiguous().cuda()
        with torch.no_grad():
            wav = model.sample(mel, rows, ddim=False, seed=3, lens=[t], stream_ids=[i])
        own = model.mcd(it["wav"][: t * 256].clone(), wav.reshape(-1)[: t * 256].clone())
        r = report[it["item_name"]]
        assert set(r) == {"mcd_dtw", "mcd_linear", "mcd_status"} and r["mcd_status"] == "OK" == mcd.STATUS[int(own["status"][0])]
        for key in ("mcd_dtw", "mcd_linear"):
            assert np.float64(r[key]).tobytes() == own[key][0].tobytes(), key
    # the command line: a model of its own, so the table is compared with what FastDiff.mcd gives for the files it wrote
    out = tmp_path / "out"
    infer.main(["--test_input_dir", corpus, "--out_dir", str(out), "--from_wav", "--mcd"])
    lines = open(out / "mcd.tsv").read().strip().split("\n")
    assert len(lines) == 1 + len(items) and lines[0].split("\t") == ["name", "mcd_dtw", "mcd_linear", "status"]
    for line in lines[1:]:
        name, dtw_, lin, status = line.split("\t")
        assert status == "OK" and 0.0 < float(dtw_) <= float(lin) and os.path.exists(out / f"{name}_pred.wav"), line
    assert sorted(os.listdir(out)) == sorted([f"{it['item_name']}_pred.wav" for it in items] + ["mcd.tsv"])
