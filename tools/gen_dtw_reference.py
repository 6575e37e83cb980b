"""gen_dtw_reference.py -- writes tests/golden/dtw_reference.npz: a few small cost matrices and the accumulated matrix that the
reference's own alignment (utils/pitch_distance.py: time_warp) computes for them, executed, not restated.

    python tools/gen_dtw_reference.py --reference /path/to/the/reference/checkout

The reference module imports numba (for @jit) and matplotlib (for a debug plot), neither of which this project needs: both get stand-ins
here -- jit as the identity, so time_warp runs as the plain Python double loop it is written as.  Not run by the tests; the fixture it
writes is what tests/test_mcd.py reads.  The reference never counts row 0 or column 0 (it starts from dtw[0, 0] = 0 with an infinite
border), so its dtw[1:, 1:] is the textbook recurrence on costs[1:, 1:].
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np


def load_reference(root):
    numba = types.ModuleType("numba")
    numba.jit = lambda f=None, **kw: f if callable(f) else (lambda g: g)
    plt = types.ModuleType("matplotlib.pyplot")
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = plt
    for name, mod in (("numba", numba), ("matplotlib", mpl), ("matplotlib.pyplot", plt)):
        sys.modules.setdefault(name, mod)
    spec = importlib.util.spec_from_file_location("reference_pitch_distance", os.path.join(root, "utils", "pitch_distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the directory that holds utils/pitch_distance.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "dtw_reference.npz"))
    args = ap.parse_args(argv)
    ref = load_reference(args.reference)
    rng = np.random.default_rng(20)
    out = {}
    for k, shape in enumerate(((6, 8), (9, 5), (12, 12), (2, 7))):
        costs = rng.random(shape)
        if k == 2:
            costs = np.round(costs * 4.0) / 4.0            # few values: ties
        out[f"costs{k}"] = costs
        out[f"dtw{k}"] = ref.time_warp(costs.copy())
    np.savez(args.out, **out)
    print(f"wrote {os.path.normpath(args.out)}: {sorted(out)}")


if __name__ == "__main__":
    main()
