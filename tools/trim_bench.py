"""trim_bench.py -- times fd_trim_silences (csrc/fd_kernels_trim.hip: levels, mask, gather) against the same steps written in
PyTorch-ROCm eager (unfold / var for the levels, conv1d for the count of the moving average, max_pool1d for the dilation, boolean
indexing per utterance for the compaction) on the same GPU in the same process.  A tool, not bench.py.

    python tools/trim_bench.py [--items 8] [--seconds 10] [--rate 22050] [--rounds 7] [--calls 200] [--kernels]

Workload: 8 recordings of 10 s at 22050 Hz, about a third of each silence (noise 80 dB down): a silent head, two pauses of which the
dilation bridges one, a silent tail; speech-like stretches of amplitude-modulated tones.  Both sides are warmed up, their kept counts
and outputs are compared first, then they are timed in alternating rounds of `calls` back-to-back calls between two device events; the
figure is the median round over its calls.  Also printed: the share of the memory floor -- 4 (n + 2 n_out) bytes per item (every sample
read once, every kept sample read and written once) at 8 TB/s -- that the call reaches.  The eager side stops at the windows' grid of
n - n % W samples (unfold has no tail window) and computes float32 variances; it is a timing baseline, not the oracle (tests/trim_ref.py
is).  Prints one JSON line; without a GPU it fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fastdiff_amd import trim  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def recordings(B, n, rate, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(n, device=dev, dtype=torch.float64) / rate
    x = 1e-4 * torch.randn(B, n, device=dev, generator=g, dtype=torch.float64)
    for b in range(B):
        for lo, hi in ((0.08, 0.36), (0.42, 0.60), (0.78, 0.92)):      # 60 % speech; the 6 % pause is bridged: about a third is cut
            i, j = int((lo + 0.004 * b) * n), int(hi * n)
            x[b, i:j] += 0.2 * torch.sin(2 * np.pi * (150.0 + 10 * b) * t[i:j]) * (1.0 + 0.5 * torch.sin(2 * np.pi * 3.0 * t[i:j]))
    return x.float().contiguous()


def eager(x, W, A=8, G=12, top_db=40.0, floor_db=-70.0):
    """(out [B, n] zero-padded, n_out [B]) by torch operations"""
    B, n = x.shape
    M = n // W
    win = x[:, :M * W].unfold(1, W, W)                                   # [B, M, W]
    level = 10.0 * torch.log10(win.var(dim=2, unbiased=False).clamp_min(1e-20))
    thr = torch.maximum(level.max(dim=1, keepdim=True).values - top_db, torch.full_like(level[:, :1], floor_db))
    speech = (level > thr).float().unsqueeze(1)                          # [B, 1, M]
    count = torch.nn.functional.conv1d(torch.nn.functional.pad(speech, ((A - 1) // 2, A // 2)), torch.ones(1, 1, A, device=x.device))
    smooth = (2.0 * count > A).float()
    keep = torch.nn.functional.max_pool1d(smooth, G + 1, stride=1, padding=G // 2)[:, 0] > 0      # [B, M]
    mask = keep.repeat_interleave(W, dim=1)
    out = torch.zeros_like(x)
    n_out = mask.sum(dim=1)
    for b in range(B):                                                   # ragged: one boolean index per utterance
        kept = x[b, :M * W][mask[b]]
        out[b, :kept.numel()] = kept
    return out, n_out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--kernels", action="store_true", help="also the time of each of the three kernels (the handle's profile option)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trim_bench: needs the GPU (there is no CPU path and a CPU timing would say nothing)")
    dev = torch.device("cuda")
    B, rate = args.items, args.rate
    W = trim.windows(1, rate)[0]
    n = int(args.seconds * rate) // W * W                                # a whole number of windows: both sides see the same samples
    x = recordings(B, n, rate, dev)

    fused = lambda: trim.trim(x, sample_rate=rate)      # noqa: E731
    plain = lambda: eager(x, W)                         # noqa: E731
    for _ in range(3):                                  # warm-up, and the comparison
        out_f, n_f = fused()
        out_e, n_e = plain()
    torch.cuda.synchronize()
    same_counts = bool(torch.equal(n_f.long(), n_e.long()))
    same_out = bool(torch.equal(out_f, out_e))
    n_out = n_f.long().cpu().numpy()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    times = {"fused": [], "eager": []}
    for _ in range(args.rounds):                        # alternating: both see the same neighbours on the machine
        times["fused"].append(timed(fused))
        times["eager"].append(timed(plain))
    f_ms, e_ms = (float(np.median(times[k])) for k in ("fused", "eager"))
    floor_bytes = float(sum(4 * (n + 2 * int(k)) for k in n_out))
    floor_ms = 1e3 * floor_bytes / PEAK_BYTES_PER_S
    out = {"items": B, "samples": n, "rate": rate, "window": W, "kept_share": float(n_out.sum()) / (B * n), "fused_ms": f_ms, "eager_ms": e_ms,
           "eager_over_fused": e_ms / f_ms, "fused_ms_min_max": [min(times["fused"]), max(times["fused"])],
           "eager_ms_min_max": [min(times["eager"]), max(times["eager"])], "floor_bytes": floor_bytes, "floor_ms_at_8TBps": floor_ms,
           "share_of_floor": floor_ms / f_ms, "same_counts_as_eager": same_counts, "same_output_as_eager": same_out}
    if args.kernels:                                    # per-kernel time from the library's own stamps, after the timed rounds
        from fastdiff_amd import _capi
        lib, h, _ = trim._wave.default_handle(x)
        _capi.check(lib, h, lib.fd_set_option(h, b"profile", b"1"), "fd_set_option")
        lib.fd_reset_profile(h)
        for _ in range(args.calls):
            fused()
        torch.cuda.synchronize()
        stats = (_capi.FdKernelStat * 16)()
        k = lib.fd_get_profile(h, stats, 16)
        out["kernel_ms"] = {stats[i].name.decode(): stats[i].total_ms / max(stats[i].launches, 1) for i in range(min(k, 16))}
        _capi.check(lib, h, lib.fd_set_option(h, b"profile", b"0"), "fd_set_option")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
