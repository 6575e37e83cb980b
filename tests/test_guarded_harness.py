"""The guarded-memory helper (tests/guarded.py) on the CPU: fake operators written in torch, each wrong in one known way, must be
reported by the property they violate -- (a) a changed guard byte, (b) two poisons disagree, (c) the guarded runs differ from the
plain one, (d) a device pointer outside every guarded body -- and a correct one by none.  No tolerance: every comparison is on bytes.
"""
import ctypes as ct

import pytest
import torch

import guarded
from guarded import guarded as guarded_ctx

N = 37      # not a multiple of anything: 148 bytes of body, 364 bytes of rounding slack


def _x():
    return torch.arange(1, N + 1, dtype=torch.float32) / 8


def _beyond(t, k):
    """The N + 1 elements from k in front of t's first on, where the storage has them (a plain tensor's has not)."""
    off = t.storage_offset() - k
    room = t.untyped_storage().nbytes() // t.element_size()
    if off < 0 or off + N + 1 > room:
        return None
    return torch.as_strided(t, (N + 1,), (1,), off)


def op_correct(g):
    x = g.tensor(_x())
    out = torch.empty(N, device=x.device)
    out.copy_(2 * x)
    return {"out": out}


def op_stores_behind(g):
    ret = op_correct(g)
    wide = _beyond(ret["out"], 0)
    if wide is not None:
        wide[N] = 7.0
    return ret


def op_stores_in_front(g):
    ret = op_correct(g)
    wide = _beyond(ret["out"], 1)
    if wide is not None:
        wide[0] = 7.0
    return ret


def op_reads_behind(g):
    x = g.tensor(_x())
    out = torch.empty_like(x)
    out.copy_(2 * x)
    wide = _beyond(x, 0)
    if wide is not None:
        out[N - 1] += 0 * wide[N]
    return {"out": out}


def op_skips_the_last(g):
    x = g.tensor(_x())
    out = torch.zeros(N, device=x.device) if g.fill is None else torch.empty(N, device=x.device)      # (the plain run: "a recycled block")
    out[: N - 1] = 2 * x[: N - 1]
    if g.fill is None:
        out[N - 1] = 2 * x[N - 1]
    return {"out": out}


def op_accumulates(g):
    x = g.tensor(_x())
    out = torch.empty((N,), dtype=torch.float32, device=x.device)
    if g.fill is None:
        out.zero_()
    out += 2 * x
    return {"out": out}


def test_a_correct_operator_passes_all_three():
    rep = guarded.run_case(op_correct, "cpu")
    assert rep.clean(), (rep.guard, rep.poison, rep.plain, rep.unguarded)


@pytest.mark.parametrize("op,where", [(op_stores_behind, ("behind", 0)), (op_stores_in_front, ("front", 1))], ids=["behind", "in_front"])
def test_a_stray_store_is_seen_in_the_guard(op, where):
    rep = guarded.run_case(op, "cpu")
    # the position is a byte's: 7.0 and the NaN poison share their two low bytes, so the first changed byte may be the element's third
    assert len(rep.guard) == 2 and all(bad[2] == (N,) and bad[3][0] == where[0] and where[1] <= bad[3][1] < where[1] + 4 for bad in rep.guard), rep.guard
    assert [bad[3][1] for bad in rep.guard] == ([2, 0] if where[0] == "behind" else [1, 1])
    assert not rep.poison and not rep.plain and not rep.unguarded


def test_a_store_into_the_rounding_slack_counts_and_nan_hides_nothing():
    with guarded_ctx(float("nan"), "cpu") as g:
        out = torch.empty(N)
        assert g.check() == []
        g.blocks[0].buf[g.blocks[0].first + N + 5] = float("nan")      # a NaN of the poison's own bits: no byte changes
        assert g.check() == []
        g.blocks[0].buf.view(torch.int32)[g.blocks[0].first + N + 5] = 0x7FC00001      # another NaN
        assert g.check() == [(0, (N,), ("behind", 20))]
        g.blocks[0].buf.view(torch.int32)[3] = 0x01010101                 # bytes 12 .. 15 of the front pad
        assert g.check() == [(0, (N,), ("behind", 20)), (0, (N,), ("front", guarded.PAD - 15))]
        assert out.shape == (N,)


@pytest.mark.parametrize("op", [op_reads_behind, op_skips_the_last, op_accumulates], ids=["stray_read", "unwritten", "accumulates"])
def test_stray_reads_unwritten_elements_and_accumulation_make_the_poisons_disagree(op):
    rep = guarded.run_case(op, "cpu")
    assert not rep.guard, rep.guard
    n_bad = N if op is op_accumulates else 1
    assert rep.poison == [("out", n_bad, 0 if op is op_accumulates else N - 1)], rep.poison
    if op is not op_reads_behind:      # (0 * finite poison leaves the value: only the NaN run differs from the plain one)
        assert rep.plain == rep.poison


def test_integer_tensors_get_byte_patterns_and_zeros_zeroes_only_the_view():
    for fill, byte in zip(guarded.FILLS, (0x5A, 0xA5)):
        with guarded_ctx(fill, "cpu") as g:
            e = torch.empty((3, 5), dtype=torch.int16)
            z = torch.zeros(7, dtype=torch.int64)
            zl = torch.zeros_like(e)
            f = torch.full((4,), 3.0, dtype=torch.float64)
            u = g.tensor(torch.arange(9, dtype=torch.uint8))
            assert (e.view(torch.uint8) == byte).all() and not z.any() and not zl.any() and (f == 3).all() and u.tolist() == list(range(9))
            for b in g.blocks:
                body = b.buf.view(torch.uint8)
                lo, hi = b.first * b.buf.element_size(), (b.first + b.numel) * b.buf.element_size()
                assert lo == guarded.PAD and body.numel() % guarded.GRANULE == 0 and body.numel() >= 2 * guarded.PAD + hi - lo
                if b.buf.dtype.is_floating_point:
                    pads = torch.cat((b.buf[: b.first], b.buf[b.first + b.numel:]))
                    assert pads.isnan().all() if fill != fill else (pads == fill).all()
                else:
                    assert (body[:lo] == byte).all() and (body[hi:] == byte).all()
            assert g.check() == []


def test_a_guarded_view_is_aligned_like_a_plain_allocation():
    plain = torch.empty(1000)
    with guarded_ctx(guarded.FILLS[1], "cpu") as g:
        for dtype, n in ((torch.float32, 1), (torch.float32, 129), (torch.int16, 3), (torch.float64, 65), (torch.uint8, 513)):
            t = torch.empty(n, dtype=dtype)
            assert (t.data_ptr() - g.blocks[-1].buf.data_ptr()) % guarded.GRANULE == 0 and t.is_contiguous()
            assert t.data_ptr() % 64 == plain.data_ptr() % 64 == 0      # the CPU allocator aligns to 64 bytes; the device's to 512
        off = g.tensor(torch.arange(5, dtype=torch.int16), offset_bytes=4)
        assert (off.data_ptr() - g.blocks[-1].buf.data_ptr()) % guarded.GRANULE == 4 and off.tolist() == [0, 1, 2, 3, 4]


def test_other_devices_and_unmodelled_keywords_go_to_the_originals():
    with guarded_ctx(guarded.FILLS[0], "cpu") as g:
        torch.empty(4, device="meta")
        torch.empty(4, pin_memory=False)
        torch.empty_like(torch.ones(4, 4).t())
        torch.zeros(0)
        torch.empty(4, dtype=torch.bool)
        torch.full((4,), 1.0)
        torch.empty(4, out=torch.ones(4))
        assert g.blocks == []
        assert torch.empty(2, 3).shape == torch.empty((2, 3)).shape == torch.empty([2, 3], dtype=torch.float32, device="cpu").shape == (2, 3)
        assert len(g.blocks) == 3


def test_the_originals_are_back_after_the_context_also_after_an_exception():
    before = {k: getattr(torch, k) for k in guarded._PATCHED}
    lib = _FakeLib()
    fn = lib.fd_fake
    with guarded_ctx(guarded.FILLS[0], "cpu", lib):
        assert all(getattr(torch, k) is not before[k] for k in before) and lib.fd_fake is not fn
    assert all(getattr(torch, k) is before[k] for k in before) and lib.fd_fake is fn
    with pytest.raises(KeyError):
        with guarded_ctx(guarded.FILLS[0], "cpu", lib):
            raise KeyError("from the body")
    assert all(getattr(torch, k) is before[k] for k in before) and lib.fd_fake is fn


# ---- pointer coverage, with a fake library object -------------------------------------------------------------------------------------
class _FakeFn:
    def __init__(self, argtypes):
        self.argtypes = argtypes
        self.seen = []

    def __call__(self, *args):
        self.seen.append(args)
        return 0


class _FakeItem(ct.Structure):
    _fields_ = [("p", ct.c_void_p), ("n", ct.c_int64), ("q", ct.c_void_p)]


class _FakeLib:
    def __init__(self):
        vp, ci = ct.c_void_p, ct.c_int
        self.fd_fake = _FakeFn([vp, vp, vp, ci, vp])                     # handle, x, out, n, stream
        self.fd_fake_multi = _FakeFn([vp, ci, vp, vp, vp])               # handle, P, xs, outs, stream
        self.fd_fake_items = _FakeFn([vp, ct.POINTER(_FakeItem), ci, vp])
        self.fd_adamw_multi = _FakeFn([vp, vp, ci, vp, vp, vp])          # (a host table of guarded.HOST_TABLES)
        self.not_an_entry_point = _FakeFn([vp])
        self.fd_version = lambda: b"fake"                                 # (no argtypes: left alone)


def _double(lib, x, out):
    out.copy_(2 * x)
    lib.fd_fake(ct.c_void_p(1), x.data_ptr(), out.data_ptr(), N, ct.c_void_p(2))
    return {"out": out}


def test_outputs_allocated_some_other_way_are_reported_as_unguarded():
    lib = _FakeLib()
    rep = guarded.run_case(lambda g: _double(lib, g.tensor(_x()), torch.empty(N)), "cpu", lib)
    assert rep.clean() and rep.calls == {"fd_fake": 2}
    rep = guarded.run_case(lambda g: _double(lib, g.tensor(_x()), g.tensor(_x()).clone()), "cpu", lib)
    assert rep.unguarded == [("fd_fake", 2)] and not (rep.guard or rep.poison or rep.plain)
    rep = guarded.run_case(lambda g: _double(lib, g.tensor(_x()), g.tensor(_x()).new_empty(N)), "cpu", lib)
    assert rep.unguarded == [("fd_fake", 2)]
    rep = guarded.run_case(lambda g: _double(lib, _x(), torch.empty(N)), "cpu", lib)
    assert rep.unguarded == [("fd_fake", 1)]
    assert len(lib.fd_fake.seen) == 12, "the plain runs call the function itself"


def test_pointer_arrays_structures_and_host_tables_are_looked_into():
    import numpy as np
    lib = _FakeLib()

    def case(g):
        a, b, stray = g.tensor(_x()), torch.empty(N), _x().clone()
        b.copy_(a)
        lib.fd_fake_multi(None, 2, (ct.c_void_p * 2)(a.data_ptr(), None), (ct.c_void_p * 2)(b.data_ptr(), stray.data_ptr()), None)
        items = (_FakeItem * 2)(_FakeItem(a.data_ptr(), N, None), _FakeItem(stray.data_ptr(), N, b.data_ptr() + 4 * (N - 1)))
        lib.fd_fake_items(None, items, 2, None)
        tab = np.zeros((2, 5), dtype=np.int64)
        tab[0] = (a.data_ptr(), 0, b.data_ptr(), a.data_ptr(), N)
        tab[1] = (a.data_ptr(), b.data_ptr() + 4 * N, b.data_ptr(), a.data_ptr(), N)      # one past the end of b: outside its body
        lib.fd_adamw_multi(None, tab.ctypes.data, 2, a.data_ptr(), b.data_ptr(), None)
        lib.not_an_entry_point(stray.data_ptr())
        return {"b": b}

    rep = guarded.run_case(case, "cpu", lib)
    assert rep.unguarded == [("fd_fake_multi", 3), ("fd_fake_items", 1), ("fd_adamw_multi", 1)], rep.unguarded
    assert rep.calls == {"fd_fake_multi": 2, "fd_fake_items": 2, "fd_adamw_multi": 2}


def test_the_case_registry_is_whole_after_one_import_and_no_case_module_is_left_out():
    """tests/guarded_suite.py: importing it alone registers every case -- at least the 115 names of tests/golden/guarded_cases.txt, each
    once -- and every tests/guarded_cases_*.py on disk is in its import list, so a case module nobody imports fails here, without a GPU."""
    import glob
    import os

    from conftest import GOLD
    import guarded_suite as gs
    names = open(os.path.join(GOLD, "guarded_cases.txt")).read().split()
    assert len(names) == len(set(names)) >= 115
    assert not [n for n in names if n not in gs.CASES], "cases that are gone"
    with pytest.raises(AssertionError):                    # a name registers once
        gs.case(names[0])(lambda g: {})
    on_disk = {os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "guarded_cases_*.py"))}
    assert on_disk == set(gs.CASE_MODULES) == {fn.__module__ for fn, _, _ in gs.CASES.values()}
