"""fd_bins_pass in guarded memory: the cases are registered in tests/test_guarded_memory.py's CASES, so that its completeness test
(test_every_entry_point_that_takes_a_tensor_is_reached) finds the new entry point reached, and properties (a)-(d) of that module are
asserted here through its _run.  The registry is filled when this file is imported: the completeness test knows these cases whenever the
suite is collected as a whole (python -m pytest tests -m gpu), not when the old file runs alone.  No masks: the header leaves no region of
an output unspecified.
"""
import numpy as np
import pytest
import torch

import test_guarded_memory as gm
from fastdiff_amd import diversity as dv
import diversity_ref as ref

pytestmark = pytest.mark.gpu

MINE = []


def case(name):
    MINE.append(name)
    return gm.case(name)


def _wide(g, x, ld):
    """The rows x [N, D] ld floats apart in a guarded buffer that ends with the last row's D floats, 4 bytes off its aligned start."""
    N, D = x.shape
    buf = g.empty(((N - 1) * ld + D,), torch.float32, 4)
    v = torch.as_strided(buf, (N, D), (ld, 1), buf.storage_offset())
    v.copy_(x)
    return v


@case("bins-update-C+1x80-ld96-K33")
def _update(g, N=dv.CHUNK + 1, D=80, K=33, ld=96):
    x, shift, scale, cent = ref.gaussians(7, N, D, K, spread=0.5)
    cent[K - 1] = 100.0                                         # an empty bin: its centroid is copied
    prev = torch.from_numpy(np.random.default_rng(1).integers(-1, K, N).astype(np.int32))
    assign = g.tensor(prev)
    rec, out = dv.bins_pass(_wide(g, torch.from_numpy(x), ld), g.tensor(torch.from_numpy(cent)), g.tensor(torch.from_numpy(shift)),
                            g.tensor(torch.from_numpy(scale)), assign=assign, update=True, ld=ld)
    res = {"assign": assign, "centroids": out, "counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64)}
    res["scalars"] = torch.tensor([rec["moved"], rec["nonfinite"], rec["empty"], rec["status"]])
    return res


@case("bins-assign-1x4-K1-nulls")
def _assign_only(g):
    """Assignment only, every optional pointer NULL: the record is the one output."""
    rec, out = dv.bins_pass(g.tensor(torch.tensor([[1.0, -2.0, 0.5, 3.0]])), g.tensor(torch.tensor([[0.0, 1.0, 0.0, 1.0]])))
    assert out is None
    return {"counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64),
            "scalars": torch.tensor([rec["moved"], rec["nonfinite"], rec["empty"], rec["status"]])}


@case("bins-nonfinite-300x36-K50")
def _nonfinite(g, N=300, D=36, K=50):
    """Rows that are not finite next to the buffer's ends, update and record."""
    x, shift, scale, cent = ref.gaussians(9, N, D, K, spread=0.5)
    x[0, 0], x[N - 1, D - 1], x[130, 7] = np.nan, np.inf, -np.inf
    assign = g.tensor(torch.full((N,), -1, dtype=torch.int32))
    rec, out = dv.bins_pass(g.tensor(torch.from_numpy(x)), g.tensor(torch.from_numpy(cent)), g.tensor(torch.from_numpy(shift)),
                            g.tensor(torch.from_numpy(scale)), assign=assign, update=True)
    return {"assign": assign, "centroids": out, "counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64)}


@pytest.mark.parametrize("name", MINE)
def test_bins_pass_in_guarded_memory(name):
    rep = gm._run(name)
    declared = gm.CASES[name][1]
    print(f"{name}: {sum(rep.calls.values())} library calls in the two guarded runs: {dict(rep.calls)}")
    assert not rep.guard, f"(a) guard bytes changed (fill, block, shape, where): {rep.guard}"
    assert not rep.poison, f"(b) the two poisons disagree (tensor, elements, first): {rep.poison}"
    assert not rep.plain, f"(c) guarded and plain runs disagree (tensor, elements, first): {rep.plain}"
    assert set(rep.unguarded) == set(declared) == set(), f"(d) pointers outside guarded memory: {rep.unguarded}"
    assert rep.calls["fd_bins_pass"] == 2
