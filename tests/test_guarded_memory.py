"""Every operator in guarded memory (tests/guarded.py): stray stores, stray loads, unwritten output, dependence on what the output held.

The cases and what they share are in tests/guarded_suite.py and its case modules (tests/guarded_cases_*.py); importing it fills the
registry, so this file tests the same cases run alone or with the whole suite.  Each case is run plain, guarded with nan / 0x5A and
guarded with -12345.678 / 0xA5, and the test asserts
  (a) no guard byte changed in either guarded run;
  (b) the two guarded runs agree bit for bit inside the specified regions;
  (c) they agree bit for bit with the plain run (the library's sums have a fixed order) -- which ties them to the float64 comparisons
      the plain calls pass in the operators' own tests;
  (d) every device pointer the library was given lay in guarded memory, but for the arguments the case declares with a reason;
and that the entry points the case names were called as often as it says.  The last test asserts from the call log that every entry
point that takes a caller's tensor was reached.  No tolerance anywhere.
"""
import ctypes as ct

import pytest
import torch

import guarded
from fastdiff_amd import _capi
from guarded_suite import CASES, DEV, _run

pytestmark = pytest.mark.gpu


def test_a_guarded_tensor_is_aligned_like_a_plain_allocation():
    with guarded.guarded(guarded.FILLS[0], DEV) as g:
        for n, dtype in ((1, torch.float32), (37, torch.float32), (4097, torch.float32), (5, torch.int16), (3, torch.int64), (144, torch.uint8)):
            plain = g._orig["empty"](n, dtype=dtype, device=DEV)
            t = torch.empty(n, dtype=dtype, device=DEV)
            assert t.data_ptr() % guarded.GRANULE == plain.data_ptr() % guarded.GRANULE == 0, (n, dtype)
        assert g.check() == [] and len(g.blocks) == 6


def test_the_three_properties_see_a_wrong_operator_on_the_device():
    """The harness' own CPU tests (test_guarded_harness.py) on device memory, with torch operations standing in for a kernel: a store one
    element behind the output, a load one element behind the input, an element that is never written."""
    N = 37

    def wide(t):
        room = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        return torch.as_strided(t, (N + 1,), (1,), t.storage_offset()) if room > N else None

    def op(fault):
        def fn(g):
            x = g.tensor(torch.arange(1.0, N + 1))
            out = torch.empty(N, device=x.device)
            out.copy_(2 * x)
            w = wide(out if fault == "store" else x)
            if fault == "store" and w is not None:
                w[N] = 7.0
            if fault == "load" and w is not None:
                out[N - 1] += 0 * w[N]
            if fault == "skip" and g.fill is not None:
                out[N - 1] = torch.empty(N, device=x.device)[N - 1]
            return {"out": out}
        return fn

    dev = torch.device(DEV, torch.cuda.current_device())
    rep = guarded.run_case(op("store"), dev)
    assert [bad[2:] for bad in rep.guard] == [((N,), ("behind", 2)), ((N,), ("behind", 0))] and not rep.poison and not rep.plain
    for fault in ("load", "skip"):
        rep = guarded.run_case(op(fault), dev)
        assert not rep.guard and rep.poison == [("out", 1, N - 1)], (fault, rep.guard, rep.poison)
    assert guarded.run_case(op(None), dev).clean()


@pytest.mark.parametrize("name", list(CASES))
def test_operator_in_guarded_memory(name):
    rep = _run(name)
    _, declared, calls = CASES[name]
    print(f"{name}: {sum(rep.calls.values())} library calls in the two guarded runs: {dict(rep.calls)}")
    assert not rep.guard, f"(a) guard bytes changed (fill, block, shape, where): {rep.guard}"
    assert not rep.poison, f"(b) the two poisons disagree (tensor, elements, first): {rep.poison}"
    assert not rep.plain, f"(c) guarded and plain runs disagree (tensor, elements, first): {rep.plain}"
    assert set(rep.unguarded) == set(declared), f"(d) pointers outside guarded memory: {rep.unguarded}, declared: {sorted(declared)}"
    assert rep.calls, "the case called no entry point"
    assert {ep: rep.calls[ep] for ep in calls} == calls, f"calls of the entry points the case is there for: {dict(rep.calls)}, expected: {calls}"


# entry points that take a pointer but no tensor of a caller's on the device, or that have a test of their own
EXEMPT = {
    "fd_ema_multi": "tests/test_param_ema.py puts canaries round its segments",
    "fd_set_weight": "weight accessor (host data)", "fd_get_weight_image": "weight accessor (host data)",
    "fd_set_mel_filterbank": "filter-bank accessor (host data)", "fd_get_mel_filterbank": "filter-bank accessor (host data)",
    "fd_read_tap": "tap accessor (host buffer)",
    "fd_set_noise_streams": "host array of stream ids", "fd_resample_taps": "host array of taps",
    "fd_pitch_lags": "host structure and two host integers",
    "fd_sample_spans_plan": "host arrays of spans and windows, a host integer", "fd_trim_windows": "two host integers",
    "fd_get_profile": "host array of kernel statistics",
    "fd_pwg_create": "host structure and the new handle", "fd_pwg_set_weight": "weight accessor (host data)",
    "fd_pwg_set_scaler": "scaler accessor (host data)",
    "fd_pwg_generate": "tests/test_pwg.py checks pointer placement itself", "fd_pwg_draw": "tests/test_pwg.py checks pointer placement itself",
    "fd_refresh_weights_device": "reads the parameters where the module holds them; tests/test_weight_refresh.py holds the packed image to a host commit's",
}


def required_entry_points(lib):
    """The fd_* functions with a c_void_p between the handle and the stream (every pointer is bound as one: arrays of structures too)."""
    return {name for name, fn in vars(lib).items() if name.startswith("fd_") and getattr(fn, "argtypes", None) is not None and
            ct.c_void_p in fn.argtypes[1:-1]}


def test_every_entry_point_that_takes_a_tensor_is_reached():
    """From the call log of the guarded runs (a case that has not run in this process is run here): a new entry point without a case
    fails."""
    lib = _capi.load()
    need = required_entry_points(lib)
    print(f"{len(need)} entry points take a pointer between the handle and the stream: {sorted(need)}")
    assert set(EXEMPT) <= need, f"stale exemptions: {sorted(set(EXEMPT) - need)}"
    assert len(need) >= 70 and {"fd_sample_spans", "fd_mel_ring_append", "fd_forward", "fd_adamw_multi"} <= need
    reached = set()
    for name in CASES:
        reached |= set(_run(name).calls)
    missing = need - set(EXEMPT) - reached
    assert not missing, f"entry points no case reaches: {sorted(missing)}"
