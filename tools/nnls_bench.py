"""nnls_bench.py -- times the fused non-negative mel inversion (fd_mel_to_linear_nnls, csrc/fd_kernels_nnls.hip) against the same
iteration written in PyTorch-ROCm eager (torch.matmul, float32) on the same GPU in the same process.  A tool, not bench.py.

    python tools/nnls_bench.py [--items 8] [--frames 865] [--iters 128] [--rounds 7] [--calls 10]

Workload: 8 x 865 frames, 128 iterations, the default "pwg" bank; the mels are the front-end's own of a seeded harmonic-plus-noise
signal, so the timed problem is the one the baseline vocoder meets.  Both sides are warmed up (code objects, the bank's upload, the
BLAS library's choice of algorithm), then timed in alternating rounds of `calls` back-to-back calls between two device events; the
figure is the median round over its calls.  The two results are compared on their image (|| A (x_fused - x_eager) || / || g ||) first:
x itself drifts in the bank's null space.  Work counted from the shapes: 4 * 80 * 513 flop per frame and iteration.  Prints one JSON
line; without a GPU it fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fastdiff_amd import griffin_lim as gl  # noqa: E402
from fastdiff_amd import _wave  # noqa: E402


def eager(mel, A, P, step, beta, n_iters):
    """the header's iteration on [B, 80, T] in eager float32: two matmuls, a subtraction, an fma, a clamp and a lerp per iteration"""
    g = torch.pow(10.0, mel)
    x = torch.clamp_min(torch.matmul(P, g), 0.0)
    y = x
    At = A.t().contiguous()
    for k in range(n_iters):
        r = torch.matmul(A, y) - g
        xn = torch.clamp_min(y - step * torch.matmul(At, r), 0.0)
        y = xn + beta[k] * (xn - x)
        x = xn
    return torch.clamp_min(x, 1e-10)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--frames", type=int, default=865)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("nnls_bench: needs the GPU (there is no CPU path and a CPU timing would say nothing)")
    dev = torch.device("cuda")
    B, T, n = args.items, args.frames, args.iters
    rng = np.random.default_rng(0)
    L = 256 * (T - 1)
    t = np.arange(L) / 22050.0
    wav = np.stack([sum(0.3 / h * np.sin(2 * np.pi * (110.0 + 20.0 * b) * h * t + 0.7 * h) for h in range(1, 30)) + 0.01 * rng.standard_normal(L) for b in range(B)])
    wav = torch.from_numpy((wav / np.abs(wav).max() * 0.9).astype(np.float32)).to(dev)
    lib, h, stream = _wave.default_handle(wav)
    bank = np.empty((80, 513), np.float32)
    assert lib.fd_get_mel_filterbank(h, bank.ctypes.data, 80, 513) >= 0
    mel = torch.empty((B, 80, T), device=dev, dtype=torch.float32)
    assert lib.fd_mel_spectrogram(h, wav.data_ptr(), B, L, mel.data_ptr(), T, stream) == 0
    P = gl.pinv(bank, "pwg")
    Ld = gl.nnls_step_bound(bank)
    A_d, P_d = torch.from_numpy(bank).to(dev), torch.from_numpy(P.copy()).to(dev)
    tt, beta = 1.0, []
    for _ in range(max(n, 1)):
        t1 = (1.0 + (1.0 + 4.0 * tt * tt) ** 0.5) / 2.0
        beta.append(float(np.float32((tt - 1.0) / t1)))
        tt = t1
    step = float(np.float32(1.0 / Ld))

    fused = lambda: gl.mel_to_linear_nnls(mel, bank, P, n_iters=n)      # noqa: E731
    plain = lambda: eager(mel, A_d, P_d, step, beta, n)                # noqa: E731
    a_f, a_e = fused(), plain()                                        # warm-up, and the comparison
    a_f, a_e = fused(), plain()
    torch.cuda.synchronize()
    g = torch.pow(10.0, mel.double())
    img = (torch.matmul(A_d.double(), a_f.double() - a_e.double()).norm(dim=1) / g.norm(dim=1)).max().item()
    resid = {k: (torch.matmul(A_d.double(), a.double()) - g).norm(dim=1).div(g.norm(dim=1)).median().item() for k, a in (("fused", a_f), ("eager", a_e))}

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
    flop = 4.0 * 80 * 513 * B * T * n
    out = {"items": B, "frames": T, "iters": n, "fused_ms": float(np.median(times["fused"])), "eager_ms": float(np.median(times["eager"])),
           "fused_ms_min_max": [min(times["fused"]), max(times["fused"])], "eager_ms_min_max": [min(times["eager"]), max(times["eager"])],
           "gflop": flop / 1e9, "fused_tflops": flop / (np.median(times["fused"]) * 1e-3) / 1e12, "image_gap_fused_vs_eager": img,
           "median_residual": resid}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
