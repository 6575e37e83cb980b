"""fd_cepstra, fd_dtw and fd_mcd_measure in guarded memory: the cases are registered in tests/test_guarded_memory.py's CASES, so that its
completeness test (test_every_entry_point_that_takes_a_tensor_is_reached) finds the new entry points reached, and properties (a)-(d) of
that module are asserted here through its _run.  The registry is filled when this file is imported: the completeness test knows these
cases whenever the suite is collected as a whole (python -m pytest tests -m gpu), not when the old file runs alone.  No masks: the header
leaves no region of an output unspecified (the cepstral rows behind an item's own frames are zero, align_out behind its rows is -1).
Every input ends with its last own sample or row: nothing may be read behind them.
"""
import numpy as np
import pytest
import torch

import test_guarded_memory as gm
from fastdiff_amd import mcd
import test_mcd as tm

pytestmark = pytest.mark.gpu

MINE = []
R, C = mcd.ROWS, mcd.COLS


def case(name):
    MINE.append(name)
    return gm.case(name)


def _wide(g, x, ld):
    """The rows x [T, D] ld floats apart as [1, T, D] in a guarded buffer that ends with the last row's D floats, 4 bytes off its aligned
    start."""
    T, D = x.shape
    buf = g.empty(((T - 1) * ld + D,), torch.float32, 4)
    v = torch.as_strided(buf, (1, T, D), (T * ld, ld, 1), buf.storage_offset())
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return v


def _ragged(g, rows):
    """Waveforms of different lengths as one batch that ends with the LAST row's own samples: that row is the longest but one sample."""
    L = max(len(x) for x in rows[:-1])
    assert len(rows[-1]) == L - 1
    flat = g.empty((len(rows) * L - 1,), torch.float32)
    flat.fill_(0.0 if g.fill is None else g.fill)          # what lies behind a row's own samples is never read: the poisons would show
    for b, x in enumerate(rows):                           # (flat: a [B, L] view would reach one sample behind the buffer)
        flat[b * L: b * L + len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    return flat, L, [len(x) for x in rows]


@case("cepstra-ragged-513-255-2048")
def _cepstra(g):
    v, L, valid = _ragged(g, [tm.wave(1, 513), tm.wave(2, 255), tm.wave(3, 2049), tm.wave(4, 2048)])
    # (the wrapper takes a whole [B, L] tensor; this batch lacks the one sample behind the last row, so the entry point is called as it calls it)
    lib, h, stream = mcd._wave.default_handle(v)
    T = mcd.frames(L)
    out = torch.empty((4, T, 13), device=v.device, dtype=torch.float32)
    mcd._front_end(lib, h, "pwg")
    rc = lib.fd_cepstra(h, v.data_ptr(), 4, L, mcd._wave.counts(valid, 4, "mcd"), 13, out.data_ptr(), T, stream)
    mcd._capi.check(lib, h, rc, "fd_cepstra")
    return {"cep": out}


@case("dtw-align-R+1xC+1-ld24")
def _dtw_align(g, D=13, ld=24):
    rec, al = mcd.dtw(_wide(g, tm.features(1, R + 1, D), ld), _wide(g, tm.features(2, C + 1, D), ld), align=True)
    return dict(gm.as_tensors(rec), align=al)


@case("dtw-R+1x300-D40")
def _dtw_plain(g, D=40):
    rec = mcd.dtw(_wide(g, tm.features(3, R + 1, D), D), _wide(g, tm.features(4, 300, D), D))
    return gm.as_tensors(rec)


@case("dtw-ragged-nonfinite")
def _dtw_ragged(g, D=13):
    As, Bs = [tm.features(5, 70, D), tm.features(6, R + 1, D).copy()], [tm.features(7, C + 2, D), tm.features(8, 9, D)]
    As[1][R, D - 1] = np.inf
    fill = 0.0 if g.fill is None else g.fill               # what lies behind a pair's own rows is never read: the poisons would show
    a, b = g.tensor(torch.from_numpy(tm._padded(As, R + 1, D, fill))), g.tensor(torch.from_numpy(tm._padded(Bs, C + 2, D, fill)))
    rec, al = mcd.dtw(a, b, frames_a=[70, R + 1], frames_b=[C + 2, 9], align=True)
    return dict(gm.as_tensors(rec), align=al)


@case("mcd-measure-ragged-lengths")
def _measure(g):
    x, Lc, vc = _ragged(g, [tm.wave(1, 513), tm.wave(2, 3000), tm.wave(3, 2999)])
    y, Ld, vd = _ragged(g, [tm.wave(4, 2000), tm.wave(2, 2500), tm.wave(5, 2499)])
    lib, h, stream = mcd._wave.default_handle(x)
    rec = torch.empty((3, mcd.RECORD.itemsize), device=x.device, dtype=torch.uint8)
    c, variant = mcd._config(None)
    mcd._front_end(lib, h, variant)
    import ctypes as ct
    rc = lib.fd_mcd_measure(h, x.data_ptr(), Lc, y.data_ptr(), Ld, 3, mcd._wave.counts(vc, 3, "mcd"), mcd._wave.counts(vd, 3, "mcd"), ct.byref(c), rec.data_ptr(), stream)
    mcd._capi.check(lib, h, rc, "fd_mcd_measure")
    return gm.as_tensors(mcd._record(rec))


@pytest.mark.parametrize("name", MINE)
def test_mcd_in_guarded_memory(name):
    rep = gm._run(name)
    declared = gm.CASES[name][1]
    print(f"{name}: {sum(rep.calls.values())} library calls in the two guarded runs: {dict(rep.calls)}")
    assert not rep.guard, f"(a) guard bytes changed (fill, block, shape, where): {rep.guard}"
    assert not rep.poison, f"(b) the two poisons disagree (tensor, elements, first): {rep.poison}"
    assert not rep.plain, f"(c) guarded and plain runs disagree (tensor, elements, first): {rep.plain}"
    assert set(rep.unguarded) == set(declared) == set(), f"(d) pointers outside guarded memory: {rep.unguarded}"
    want = {"cepstra": "fd_cepstra", "dtw": "fd_dtw", "mcd": "fd_mcd_measure"}[name.split("-")[0]]
    assert rep.calls[want] == 2
