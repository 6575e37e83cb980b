"""Time of Griffin-Lim on the device for the benchmark batch (8 items of 865 frames = 221 184 samples, 60 iterations, everything resident
on the device) next to the same loop in PyTorch eager on the same GPU (torch.stft / angle / polar / istft, the reference's
griffin_lim_torch with zero padding):  python tools/bench_griffin_lim.py [--B 8] [--T 865] [--iters 60] [--reps 7] [--warmup 2]

Device events around each repetition, warm-up first, medians reported; one JSON line at the end.  The two loops start from the same
amplitudes; the eager one draws its own starting phase, which does not change its cost.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fastdiff_amd  # noqa: E402


def eager_griffin_lim(amp, n_iters, window):
    """amp [B, 513, T] -> [B, 256 (T - 1)]: the loop of the library's definition on torch's own transforms"""
    L = 256 * (amp.shape[-1] - 1)
    ist = lambda C: torch.istft(C, 1024, hop_length=256, win_length=1024, window=window, center=True, length=L)      # noqa: E731
    y = ist(torch.polar(amp, 6.2831855 * torch.rand_like(amp)))
    for _ in range(n_iters):
        X = torch.stft(y, 1024, hop_length=256, win_length=1024, window=window, center=True, pad_mode="constant", return_complex=True)
        y = ist(torch.polar(amp, torch.angle(X)))
    return y


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=865)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    m = fastdiff_amd.FastDiff().cuda().eval()
    window = torch.hann_window(1024, periodic=True, device="cuda")
    x = 0.3 * (torch.rand(args.B, 256 * (args.T - 1), device="cuda") * 2 - 1)
    amp = torch.stft(x, 1024, hop_length=256, win_length=1024, window=window, center=True, pad_mode="constant", return_complex=True).abs().contiguous()
    assert amp.shape == (args.B, 513, args.T)
    fused = timed(lambda: m.griffin_lim(amp, n_iters=args.iters, seed=1), args.reps, args.warmup)
    fused0 = timed(lambda: m.griffin_lim(amp, n_iters=0, seed=1), args.reps, args.warmup)
    eager = timed(lambda: eager_griffin_lim(amp, args.iters, window), args.reps, args.warmup)
    _, rec = m.griffin_lim(amp, n_iters=args.iters, seed=1, return_record=True)
    y = eager_griffin_lim(amp, args.iters, window)
    X = torch.stft(y, 1024, hop_length=256, win_length=1024, window=window, center=True, pad_mode="constant", return_complex=True).abs()
    sc_eager = float(((X - amp) ** 2).sum().sqrt() / (amp ** 2).sum().sqrt())
    f, f0, e = statistics.median(fused), statistics.median(fused0), statistics.median(eager)
    out = {"B": args.B, "T": args.T, "iters": args.iters, "reps": args.reps, "fused_ms": round(f, 3), "fused_ms_min": round(min(fused), 3),
           "fused_ms_max": round(max(fused), 3), "fused_0_iters_ms": round(f0, 3), "fused_ms_per_iter": round((f - f0) / max(args.iters, 1), 4),
           "eager_ms": round(e, 3), "eager_ms_min": round(min(eager), 3), "eager_ms_max": round(max(eager), 3),
           "eager_ms_per_iter": round(e / max(args.iters, 1), 4), "eager_over_fused": round(e / f, 3),
           "sc_fused": [round(float(v), 5) for v in rec["sc"]], "sc_eager_batch": round(sc_eager, 5), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
