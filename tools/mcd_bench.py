"""mcd_bench.py -- times the fused alignment kernel (fd_dtw, csrc/fd_kernels_mcd.hip) against the same recurrence written in PyTorch-ROCm
eager (local costs by torch.cdist, then one anti-diagonal of the accumulated matrix after the other, each from slices of the two before
it; float64 accumulation, cost only: no path length, no alignment) on the same GPU in the same process, and fd_mcd_measure end to end.
A tool, not bench.py.

    python tools/mcd_bench.py [--pairs 8] [--frames 865] [--coef 13] [--rounds 5] [--calls 5]

Workload: 8 pairs of 865 x 865 frames of 13 coefficients (the benchmark batch's 864-frame utterances), seeded random walks; for the
end-to-end figure 8 pairs of 864 * 256 samples of noise plus tones.  Both sides are warmed up, then timed in alternating rounds of
`calls` back-to-back calls between two device events; the figure is the median round over its calls.  The two costs are compared first.
Also printed: the modelled floor of the recurrence -- Ta + Tb - 1 dependent anti-diagonal steps per pair, which the kernel takes as
blocks x (Tb + rows - 1) steps of one workgroup -- next to the measured time per step.  Prints one JSON line; without a GPU it fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fastdiff_amd import mcd  # noqa: E402


def eager_plan(Ta, Tb, dev):
    """per anti-diagonal s = i + j: the rows i it holds (the columns are s - i); shape-only, made once"""
    return [torch.arange(max(0, s - Tb + 1), min(Ta, s + 1), device=dev) for s in range(Ta + Tb - 1)]


def eager(a, b, plan):
    """the accumulated cost of every pair: D [B, Ta + 1, Tb + 1] with an infinite border, one anti-diagonal per iteration"""
    B, Ta, _ = a.shape
    Tb = b.shape[1]
    c = torch.cdist(a, b).double()
    D = torch.full((B, Ta + 1, Tb + 1), float("inf"), device=a.device, dtype=torch.float64)
    D[:, 0, 0] = 0.0
    for s, i in enumerate(plan):
        j = s - i
        best = torch.minimum(torch.minimum(D[:, i, j], D[:, i, j + 1]), D[:, i + 1, j])
        D[:, i + 1, j + 1] = c[:, i, j] + best
    return D[:, Ta, Tb]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=865)
    ap.add_argument("--coef", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mcd_bench: needs the GPU (there is no CPU path and a CPU timing would say nothing)")
    dev = torch.device("cuda")
    B, T, D = args.pairs, args.frames, args.coef
    g = torch.Generator(device=dev).manual_seed(0)
    a = (0.3 * torch.randn(B, T, D, device=dev, generator=g).cumsum(1) + 0.1 * torch.randn(B, T, D, device=dev, generator=g)).contiguous()
    b = (a + 0.2 * torch.randn(B, T, D, device=dev, generator=g)).roll(3, 1).contiguous()
    n = (T - 1) * 256
    t = torch.arange(n, device=dev) / 22050.0
    x = 0.1 * torch.randn(B, n, device=dev, generator=g) + 0.1 * torch.sin(2 * np.pi * 220.0 * t) + 0.1 * torch.sin(2 * np.pi * 1310.0 * t)
    y = (x + 0.02 * torch.randn(B, n, device=dev, generator=g)).roll(300, 1).contiguous()
    plan = eager_plan(T, T, dev)
    lib, h, stream = mcd._wave.default_handle(a)
    rec = torch.empty((B, mcd.DTW_RECORD.itemsize), device=dev, dtype=torch.uint8)
    mrec = torch.empty((B, mcd.RECORD.itemsize), device=dev, dtype=torch.uint8)
    cfg = mcd._config({"n_coef": D})

    def fused():
        mcd._capi.check(lib, h, lib.fd_dtw(h, a.data_ptr(), b.data_ptr(), B, D, D, T, T, None, None, rec.data_ptr(), None, 0, stream), "fd_dtw")

    def measure():
        mcd._enqueue(lib, h, stream, x, y, None, cfg, rec=mrec)

    plain = lambda: eager(a, b, plan)      # noqa: E731
    for _ in range(2):                     # warm-up, and the comparison
        fused(), measure()
        c_e = plain()
    torch.cuda.synchronize()
    c_f = torch.from_numpy(mcd._wave.records(rec, mcd.DTW_RECORD, mcd.DTW_FIELDS)["cost"]).to(dev)
    gap = float(((c_f - c_e).abs() / c_e).max())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    times = {"fused": [], "eager": [], "measure": []}
    for _ in range(args.rounds):           # alternating: all see the same neighbours on the machine
        times["fused"].append(timed(fused))
        times["eager"].append(timed(plain))
        times["measure"].append(timed(measure))
    f_ms, e_ms, m_ms = (float(np.median(times[k])) for k in ("fused", "eager", "measure"))
    blocks = (T + mcd.ROWS - 1) // mcd.ROWS
    steps = sum(T + min(mcd.ROWS, T - k * mcd.ROWS) - 1 for k in range(blocks))
    out = {"pairs": B, "frames": T, "coef": D, "fused_dtw_ms": f_ms, "eager_dtw_ms": e_ms, "eager_over_fused": e_ms / f_ms, "mcd_measure_ms": m_ms,
           "fused_ms_min_max": [min(times["fused"]), max(times["fused"])], "eager_ms_min_max": [min(times["eager"]), max(times["eager"])],
           "measure_ms_min_max": [min(times["measure"]), max(times["measure"])],
           "floor_dependent_steps_per_pair": 2 * T - 1, "kernel_steps_per_pair": steps, "fused_us_per_kernel_step": 1e3 * f_ms / steps,
           "largest_relative_cost_gap_to_eager": gap}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
