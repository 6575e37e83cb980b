"""bins_bench.py -- times one update pass of the fused k-means kernel (fd_bins_pass, csrc/fd_kernels_bins.hip) against the same pass
written in PyTorch-ROCm eager (cdist's expanded form as one matmul, argmin, index_add_, bincount; float32) on the same GPU in the same
process.  A tool, not bench.py.

    python tools/bins_bench.py [--rows 4194304] [--features 80] [--bins 50] [--rounds 7] [--calls 10]

Workload: 2^22 rows of 80 features (seeded overlapping Gaussians in raw units, standardised by the pass), 50 centroids.  Both sides are
warmed up, then timed in alternating rounds of `calls` back-to-back calls between two device events; the figure is the median round over
its calls.  The two assignments are compared first (rows that differ: near ties).  Also printed: the bytes of the rows over the time,
and the time those bytes take at 8 TB/s.  Prints one JSON line; without a GPU it fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fastdiff_amd import diversity as dv  # noqa: E402


def eager(x, shift, scale, cent):
    """the same pass in eager float32: standardise, scores h - z c^T, argmin, per-bin sums and counts, the quotient"""
    z = (x - shift) * scale
    s = 0.5 * (cent * cent).sum(1) - z @ cent.t()
    a = s.argmin(1)
    sums = torch.zeros_like(cent).index_add_(0, a, z)
    n = torch.bincount(a, minlength=cent.shape[0])
    return a, torch.where(n[:, None] > 0, sums / n.clamp_min(1)[:, None], cent)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--features", type=int, default=80)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bins_bench: needs the GPU (there is no CPU path and a CPU timing would say nothing)")
    dev = torch.device("cuda")
    N, D, K = args.rows, args.features, args.bins
    g = torch.Generator(device=dev).manual_seed(0)
    centres = 0.7 * torch.randn(K, D, device=dev, generator=g)
    x = centres[torch.randint(0, K, (N,), device=dev, generator=g)] + torch.randn(N, D, device=dev, generator=g)
    mu, sd = 10.0 * torch.rand(D, device=dev, generator=g) - 5.0, 0.5 + 2.5 * torch.rand(D, device=dev, generator=g)
    x = (x * sd + mu).contiguous()
    shift, scale = dv.standardization(x)
    cent = ((x[:K] - shift) * scale).contiguous()
    assign = torch.full((N,), -1, dtype=torch.int32, device=dev)

    fused = lambda: dv.bins_pass(x, cent, shift, scale, assign=assign, update=True, record=False)[1]      # noqa: E731
    plain = lambda: eager(x, shift, scale, cent)                                                          # noqa: E731
    for _ in range(2):                                                                                    # warm-up, and the comparison
        c_f, (a_e, c_e) = fused(), plain()
    torch.cuda.synchronize()
    differ = int((assign.long() != a_e).sum())
    gap = float((c_f - c_e).abs().max())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    times = {"fused": [], "eager": []}
    for _ in range(args.rounds):                                       # alternating: both see the same neighbours on the machine
        times["fused"].append(timed(fused))
        times["eager"].append(timed(plain))
    nbytes = 4.0 * N * D
    f_ms, e_ms = float(np.median(times["fused"])), float(np.median(times["eager"]))
    out = {"rows": N, "features": D, "bins": K, "fused_ms": f_ms, "eager_ms": e_ms, "fused_ms_min_max": [min(times["fused"]), max(times["fused"])],
           "eager_ms_min_max": [min(times["eager"]), max(times["eager"])], "eager_over_fused": e_ms / f_ms, "row_gbytes": nbytes / 1e9,
           "fused_tbytes_per_s": nbytes / (f_ms * 1e-3) / 1e12, "roofline_ms_at_8_tbytes_per_s": nbytes / 8e12 * 1e3,
           "rows_assigned_differently": differ, "largest_centroid_gap": gap}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
