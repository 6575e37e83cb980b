"""fd_trim_silences and fd_trim_levels in guarded memory: the cases are registered in tests/test_guarded_memory.py's CASES, so that its
completeness test (test_every_entry_point_that_takes_a_tensor_is_reached) finds the new entry points reached, and properties (a)-(d) of
that module are asserted here through its _run.  The registry is filled when this file is imported: the completeness test knows these
cases whenever the suite is collected as a whole (python -m pytest tests -m gpu), not when the old file runs alone.  No masks: the header
leaves no region of an output unspecified (out is 0 behind n_out, the flags and the levels are 0 behind an item's own windows, the record
has no padding).  The ragged batch ends with its last row's own samples: nothing may be read behind them.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

import test_guarded_memory as gm
from fastdiff_amd import _capi, trim
import test_trim as tt

pytestmark = pytest.mark.gpu

MINE = []
RATE, MS, W = 8000, 10, 80
CHUNK = trim.CHUNK


def case(name):
    MINE.append(name)
    return gm.case(name)


def _ragged(g, rows):
    """Waveforms of different lengths as one batch that ends with the LAST row's own samples: that row is the longest but one sample."""
    L = max(len(x) for x in rows[:-1])
    assert len(rows[-1]) == L - 1
    flat = g.empty((len(rows) * L - 1,), torch.float32)
    flat.fill_(0.0 if g.fill is None else g.fill)          # what lies behind a row's own samples is never read: the poisons would show
    for b, x in enumerate(rows):                           # (flat: a [B, L] view would reach one sample behind the buffer)
        if len(x):
            flat[b * L: b * L + len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    return flat, L, [len(x) for x in rows]


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
        ret.update(gm.as_tensors(trim._record(rec)))
    return ret


@case("trim-ragged-long-flags-rec")
def _ragged_long(g):
    v, L, valid = _ragged(g, _rows())
    ret = _call(g, v, 5, L, valid, "long", True, True)
    assert ret["status"].tolist() == [trim.OK, trim.OK, trim.EMPTY, trim.SILENT, trim.OK]
    return ret


@case("trim-ragged-edges-plain")
def _ragged_edges(g):
    v, L, valid = _ragged(g, _rows())
    return _call(g, v, 5, L, valid, "edges", False, False)


@case("trim-off4-flags")
def _off4(g):
    x = tt.signal_of(15, RATE, 2 * CHUNK * W + 5 * W + 3)
    v = g.tensor(torch.from_numpy(x.copy()).reshape(1, -1), 4)
    return _call(g, v, 1, v.shape[1], None, "long", True, False)


@case("trim-levels-ragged")
def _levels(g):
    v, L, valid = _ragged(g, _rows())
    lib, h, stream = trim._wave.default_handle(v)
    lv = torch.empty((5, trim.windows(L, RATE, MS)[1]), device=v.device, dtype=torch.float64)
    rc = lib.fd_trim_levels(h, v.data_ptr(), 5, L, trim._wave.counts(valid, 5, "trim"), RATE, MS, lv.data_ptr(), stream)
    _capi.check(lib, h, rc, "fd_trim_levels")
    return {"levels": lv}


@case("trim-levels-off4")
def _levels_off4(g):
    x = tt.signal_of(15, 22050, 13 * 661 + 5)
    v = g.tensor(torch.from_numpy(x.copy()).reshape(1, -1), 4)
    return {"levels": trim.levels(v, sample_rate=22050)}


@pytest.mark.parametrize("name", MINE)
def test_trim_in_guarded_memory(name):
    rep = gm._run(name)
    declared = gm.CASES[name][1]
    print(f"{name}: {sum(rep.calls.values())} library calls in the two guarded runs: {dict(rep.calls)}")
    assert not rep.guard, f"(a) guard bytes changed (fill, block, shape, where): {rep.guard}"
    assert not rep.poison, f"(b) the two poisons disagree (tensor, elements, first): {rep.poison}"
    assert not rep.plain, f"(c) guarded and plain runs disagree (tensor, elements, first): {rep.plain}"
    assert set(rep.unguarded) == set(declared) == set(), f"(d) pointers outside guarded memory: {rep.unguarded}"
    want = "fd_trim_levels" if "levels" in name else "fd_trim_silences"
    assert rep.calls[want] == 2
