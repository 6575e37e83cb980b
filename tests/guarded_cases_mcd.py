"""Cases of the guarded-memory suite (tests/guarded_suite.py): fd_cepstra, fd_dtw and fd_mcd_measure.  No masks: the header leaves no
region of an output unspecified (the cepstral rows behind an item's own frames are zero, align_out behind its rows is -1).  Every input
ends with its last own sample or row: nothing may be read behind them.
"""
import ctypes as ct

import numpy as np
import torch

from fastdiff_amd import mcd
import test_mcd as tm
from guarded_suite import _ragged, _wide, as_tensors, case

R, C = mcd.ROWS, mcd.COLS


@case("cepstra-ragged-513-255-2048", calls={"fd_cepstra": 2})
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


@case("dtw-align-R+1xC+1-ld24", calls={"fd_dtw": 2})
def _dtw_align(g, D=13, ld=24):
    rec, al = mcd.dtw(_wide(g, tm.features(1, R + 1, D), ld)[None], _wide(g, tm.features(2, C + 1, D), ld)[None], align=True)
    return dict(as_tensors(rec), align=al)


@case("dtw-R+1x300-D40", calls={"fd_dtw": 2})
def _dtw_plain(g, D=40):
    rec = mcd.dtw(_wide(g, tm.features(3, R + 1, D), D)[None], _wide(g, tm.features(4, 300, D), D)[None])
    return as_tensors(rec)


@case("dtw-ragged-nonfinite", calls={"fd_dtw": 2})
def _dtw_ragged(g, D=13):
    As, Bs = [tm.features(5, 70, D), tm.features(6, R + 1, D).copy()], [tm.features(7, C + 2, D), tm.features(8, 9, D)]
    As[1][R, D - 1] = np.inf
    fill = 0.0 if g.fill is None else g.fill               # what lies behind a pair's own rows is never read: the poisons would show
    a, b = g.tensor(torch.from_numpy(tm._padded(As, R + 1, D, fill))), g.tensor(torch.from_numpy(tm._padded(Bs, C + 2, D, fill)))
    rec, al = mcd.dtw(a, b, frames_a=[70, R + 1], frames_b=[C + 2, 9], align=True)
    return dict(as_tensors(rec), align=al)


@case("mcd-measure-ragged-lengths", calls={"fd_mcd_measure": 2})
def _measure(g):
    x, Lc, vc = _ragged(g, [tm.wave(1, 513), tm.wave(2, 3000), tm.wave(3, 2999)])
    y, Ld, vd = _ragged(g, [tm.wave(4, 2000), tm.wave(2, 2500), tm.wave(5, 2499)])
    lib, h, stream = mcd._wave.default_handle(x)
    rec = torch.empty((3, mcd.RECORD.itemsize), device=x.device, dtype=torch.uint8)
    c, variant = mcd._config(None)
    mcd._front_end(lib, h, variant)
    rc = lib.fd_mcd_measure(h, x.data_ptr(), Lc, y.data_ptr(), Ld, 3, mcd._wave.counts(vc, 3, "mcd"), mcd._wave.counts(vd, 3, "mcd"), ct.byref(c), rec.data_ptr(), stream)
    mcd._capi.check(lib, h, rc, "fd_mcd_measure")
    return as_tensors(mcd._record(rec))
