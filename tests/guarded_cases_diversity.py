"""Cases of the guarded-memory suite (tests/guarded_suite.py): fd_bins_pass.  No masks: the header leaves no region of an output
unspecified.
"""
import numpy as np
import torch

from fastdiff_amd import diversity as dv
import diversity_ref as ref
from guarded_suite import _wide, case

TWICE = {"fd_bins_pass": 2}


@case("bins-update-C+1x80-ld96-K33", calls=TWICE)
def _update(g, N=dv.CHUNK + 1, D=80, K=33, ld=96):
    x, shift, scale, cent = ref.gaussians(7, N, D, K, spread=0.5)
    cent[K - 1] = 100.0                                         # an empty bin: its centroid is copied
    prev = torch.from_numpy(np.random.default_rng(1).integers(-1, K, N).astype(np.int32))
    assign = g.tensor(prev)
    rec, out = dv.bins_pass(_wide(g, x, ld), g.tensor(torch.from_numpy(cent)), g.tensor(torch.from_numpy(shift)),
                            g.tensor(torch.from_numpy(scale)), assign=assign, update=True, ld=ld)
    res = {"assign": assign, "centroids": out, "counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64)}
    res["scalars"] = torch.tensor([rec["moved"], rec["nonfinite"], rec["empty"], rec["status"]])
    return res


@case("bins-assign-1x4-K1-nulls", calls=TWICE)
def _assign_only(g):
    """Assignment only, every optional pointer NULL: the record is the one output."""
    rec, out = dv.bins_pass(g.tensor(torch.tensor([[1.0, -2.0, 0.5, 3.0]])), g.tensor(torch.tensor([[0.0, 1.0, 0.0, 1.0]])))
    assert out is None
    return {"counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64),
            "scalars": torch.tensor([rec["moved"], rec["nonfinite"], rec["empty"], rec["status"]])}


@case("bins-nonfinite-300x36-K50", calls=TWICE)
def _nonfinite(g, N=300, D=36, K=50):
    """Rows that are not finite next to the buffer's ends, update and record."""
    x, shift, scale, cent = ref.gaussians(9, N, D, K, spread=0.5)
    x[0, 0], x[N - 1, D - 1], x[130, 7] = np.nan, np.inf, -np.inf
    assign = g.tensor(torch.full((N,), -1, dtype=torch.int32))
    rec, out = dv.bins_pass(g.tensor(torch.from_numpy(x)), g.tensor(torch.from_numpy(cent)), g.tensor(torch.from_numpy(shift)),
                            g.tensor(torch.from_numpy(scale)), assign=assign, update=True)
    return {"assign": assign, "centroids": out, "counts": torch.from_numpy(rec["counts"]), "inertia": torch.tensor([rec["inertia"]], dtype=torch.float64)}
