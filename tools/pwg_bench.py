"""Time of Parallel WaveGAN on the device for the benchmark batch (default architecture, 8 items of 864 frames = 221 184 samples, everything
resident on the device) next to the same network as a float32 PyTorch module on the same GPU in the same process (tests/pwg_ref.py:
forward, the project's own port), and next to FastDiff at N = 4 on the same mels:  python tools/pwg_bench.py [--B 8] [--T 864] [--reps 7]

Device events around each repetition, warm-up first, medians reported.  Then, in a pass of its own with the library's per-kernel
timestamps on (option profile = 1; not part of the timed repetitions), the time of the layer kernel per launch against
  * its byte floor: x in + x out + skip in and out (64 channels of float32 each) + the five conditioning coefficients + this layer's G, at
    8 TB/s (the halo is re-read from the neighbours' tiles and counted once);
  * the matrix pipe: 2 * (128 * 192 + 128 * 64) operations per sample on the exact-fp32 instruction at 157.3 TFLOP/s.
One JSON line at the end.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import fastdiff_amd  # noqa: E402
from fastdiff_amd import _capi, infer, pwg  # noqa: E402
import pwg_ref as ref  # noqa: E402

HBM_BYTES_PER_S, FP32_MATRIX_FLOPS = 8.0e12, 157.3e12


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


def profile(lib, h):
    stats = (_capi.FdKernelStat * 128)()
    n = lib.fd_get_profile(h, stats, 128)
    return {stats[i].name.decode(): (int(stats[i].launches), float(stats[i].total_ms)) for i in range(min(n, 128))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=864)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_fastdiff", action="store_true")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "pwg_bench measures on the GPU"
    cfg = ref.default_config()
    W = ref.make_weights(cfg, 1)
    m = pwg.ParallelWaveGAN(**cfg).load_state_dict(W)
    B, T, hop, layers = args.B, args.T, m.hop_size, cfg["layers"]
    L = hop * T
    mel = torch.from_numpy(ref.synth_mel(3, B, T)).cuda()
    z = m.draw_z(B, L, seed=1)
    c = torch.from_numpy(ref.pad_mel(mel.cpu().numpy(), 2).astype(np.float32)).cuda()
    Wd = {k: torch.from_numpy(v).cuda() for k, v in W.items()}

    fused = timed(lambda: m.spec2wav(mel, z=z), args.reps, args.warmup)
    fused_draw = timed(lambda: m.spec2wav(mel, seed=1), args.reps, args.warmup)
    eager = timed(lambda: ref.forward(Wd, cfg, z, c, dtype=torch.float32, device="cuda"), args.reps, args.warmup)
    y_f, y_e = m.spec2wav(mel, z=z), ref.forward(Wd, cfg, z, c, dtype=torch.float32, device="cuda")[:, 0]
    dist = float((y_f - y_e).abs().max())

    lib, h = m._lib, m._h
    _capi.check(lib, h, lib.fd_set_option(h, b"profile", b"1"), "fd_set_option")
    lib.fd_reset_profile(h)
    for _ in range(3):
        m.spec2wav(mel, z=z)
    torch.cuda.synchronize()
    prof = profile(lib, h)
    _capi.check(lib, h, lib.fd_set_option(h, b"profile", b"0"), "fd_set_option")
    per = {k: round(ms / max(n, 1), 4) for k, (n, ms) in prof.items() if k.startswith("pwg_")}
    samples = B * L
    floor_bytes = samples * (64 * 4 * 2 + 64 * 4 * 2 + 5 * 4) + B * 128 * T * 4
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    pipe_ms = samples * 2 * (128 * 192 + 128 * 64) / FP32_MATRIX_FLOPS * 1e3

    f, e = statistics.median(fused), statistics.median(eager)
    audio_s = samples / cfg["sample_rate"]
    out = {"B": B, "T": T, "samples": samples, "reps": args.reps, "fused_ms": round(f, 3), "fused_ms_min": round(min(fused), 3),
           "fused_ms_max": round(max(fused), 3), "fused_device_z_ms": round(statistics.median(fused_draw), 3), "eager_f32_ms": round(e, 3),
           "eager_f32_ms_min": round(min(eager), 3), "eager_f32_ms_max": round(max(eager), 3), "eager_over_fused": round(e / f, 3),
           "fused_vs_eager_max_abs": dist, "kernel_ms_per_launch": per, "layer_byte_floor_ms": round(floor_ms, 4),
           "layer_matrix_pipe_ms": round(pipe_ms, 4), "layer_over_byte_floor": round(per.get("pwg_layer", float("nan")) / floor_ms, 2),
           "layer_over_matrix_pipe": round(per.get("pwg_layer", float("nan")) / pipe_ms, 2), "rtf_pwg": round(f * 1e-3 / audio_s, 6),
           "device": torch.cuda.get_device_name(0)}
    if not args.no_fastdiff:
        fd = fastdiff_amd.FastDiff().cuda().eval()
        rows = infer._step_rows(fd, 4, None, None)
        with torch.no_grad():
            fd4 = timed(lambda: fd.sample(mel, rows, seed=1), args.reps, args.warmup)
        out["fastdiff_n4_ms"] = round(statistics.median(fd4), 3)
        out["rtf_fastdiff_n4"] = round(statistics.median(fd4) * 1e-3 / audio_s, 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
