"""Cases of the guarded-memory suite (tests/guarded_suite.py): fd_trim_silences and fd_trim_levels.  No masks: the header leaves no region
of an output unspecified (out is 0 behind n_out, the flags and the levels are 0 behind an item's own windows, the record has no
padding).  The ragged batch ends with its last row's own samples: nothing may be read behind them.
"""
import ctypes as ct

import numpy as np
import torch

from fastdiff_amd import _capi, trim
import test_trim as tt
from guarded_suite import _ragged, as_tensors, case

RATE, MS, W = 8000, 10, 80
CHUNK = trim.CHUNK
SILENCES, LEVELS = {"fd_trim_silences": 2}, {"fd_trim_levels": 2}


def _rows():
    L = (CHUNK + 1) * W + 7
    return [tt.signal_of(11, RATE, 13 * W + 5), tt.signal_of(12, RATE, L), np.zeros(0, np.float32), tt.signal_of(13, RATE, W - 1), tt.signal_of(14, RATE, L - 1)]


def _call(g, v, B, L, valid, mode, with_flags, with_rec):
    lib, h, stream = trim._wave.default_handle(v)
    p = trim._params(RATE, MS, 40.0, -70.0, 8, 12, mode)
    out = torch.empty((B, L), device=v.device, dtype=torch.float32)
    ov = torch.empty((B,), device=v.device, dtype=torch.int32)
    flags = torch.empty((B, trim.windows(L, RATE, MS)[1]), device=v.device, dtype=torch.uint8) if with_flags else None
    rec = torch.empty((B, trim.RECORD.itemsize), device=v.device, dtype=torch.uint8) if with_rec else None
    rc = lib.fd_trim_silences(h, v.data_ptr(), B, L, trim._wave.counts(valid, B, "trim"), ct.byref(p), out.data_ptr(), ov.data_ptr(),
                              flags.data_ptr() if with_flags else None, rec.data_ptr() if with_rec else None, stream)
    _capi.check(lib, h, rc, "fd_trim_silences")
    ret = {"out": out, "out_valid": ov}
    if with_flags:
        ret["flags"] = flags
    if with_rec:
        ret.update(as_tensors(trim._record(rec)))
    return ret


@case("trim-ragged-long-flags-rec", calls=SILENCES)
def _ragged_long(g):
    v, L, valid = _ragged(g, _rows())
    ret = _call(g, v, 5, L, valid, "long", True, True)
    assert ret["status"].tolist() == [trim.OK, trim.OK, trim.EMPTY, trim.SILENT, trim.OK]
    return ret


@case("trim-ragged-edges-plain", calls=SILENCES)
def _ragged_edges(g):
    v, L, valid = _ragged(g, _rows())
    return _call(g, v, 5, L, valid, "edges", False, False)


@case("trim-off4-flags", calls=SILENCES)
def _off4(g):
    x = tt.signal_of(15, RATE, 2 * CHUNK * W + 5 * W + 3)
    v = g.tensor(torch.from_numpy(x.copy()).reshape(1, -1), 4)
    return _call(g, v, 1, v.shape[1], None, "long", True, False)


@case("trim-levels-ragged", calls=LEVELS)
def _levels(g):
    v, L, valid = _ragged(g, _rows())
    lib, h, stream = trim._wave.default_handle(v)
    lv = torch.empty((5, trim.windows(L, RATE, MS)[1]), device=v.device, dtype=torch.float64)
    rc = lib.fd_trim_levels(h, v.data_ptr(), 5, L, trim._wave.counts(valid, 5, "trim"), RATE, MS, lv.data_ptr(), stream)
    _capi.check(lib, h, rc, "fd_trim_levels")
    return {"levels": lv}


@case("trim-levels-off4", calls=LEVELS)
def _levels_off4(g):
    x = tt.signal_of(15, 22050, 13 * 661 + 5)
    v = g.tensor(torch.from_numpy(x.copy()).reshape(1, -1), 4)
    return {"levels": trim.levels(v, sample_rate=22050)}
