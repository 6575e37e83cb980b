"""Long-form and streaming synthesis, one session: FastDiff.sample_long against the whole-utterance sample() at T = 6912, N = 4 (default
windows: 1024 frames, 896-frame centres); a 300,000-frame utterance's time and workspace_bytes; SampleStream.push time per 32-frame
chunk.  Times are host clocks around work that ends in a device synchronise, median of `--reps` after warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import torch  # noqa: E402

import fastdiff_amd  # noqa: E402
import synth  # noqa: E402
from fastdiff_amd import infer  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long_frames", type=int, default=300_000)
    ap.add_argument("--out", default=None, help="also write the numbers as JSON here")
    args = ap.parse_args()
    m = fastdiff_amd.FastDiff()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(1234).items()})
    m = m.cuda().eval()
    N = 4
    rows = infer._step_rows(m, N, None, None)
    res = {"N": N, "halo_frames": m.halo_frames(N)}
    with torch.no_grad():
        T = 6912
        mel = torch.from_numpy(synth.synth_mel(5, 1, T)).cuda()
        whole = timed(lambda: m.sample(mel, rows, seed=1, stream_ids=[0]), args.reps)
        long_ = timed(lambda: m.sample_long(mel, rows, seed=1, stream_id=0), args.reps)
        assert torch.equal(m.sample_long(mel, rows, seed=1, stream_id=0), m.sample(mel, rows, seed=1, stream_ids=[0]))
        res.update(T=T, whole_ms=whole * 1e3, sample_long_ms=long_ * 1e3, ratio=long_ / whole)
        print(f"T={T} N={N}: sample {whole * 1e3:.2f} ms, sample_long {long_ * 1e3:.2f} ms, ratio {long_ / whole:.3f}", flush=True)

        TL = args.long_frames
        g = torch.Generator(device="cuda").manual_seed(3)
        mel_l = torch.rand((1, 80, TL), device="cuda", generator=g) * 5.0 - 5.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = m.sample_long(mel_l, rows, seed=1, stream_id=0)
        torch.cuda.synchronize()
        tl = time.perf_counter() - t0
        assert torch.isfinite(y).all()
        res.update(long_frames=TL, long_s=tl, long_frames_per_s=TL / tl, workspace_bytes=m.counter("workspace_bytes"))
        print(f"T={TL}: {tl:.2f} s ({TL / tl:.0f} frames/s, {TL * 256 / 22050 / tl:.0f}x real time), "
              f"workspace_bytes {res['workspace_bytes'] / 1e9:.3f} GB", flush=True)
        del y, mel_l

        mel_s = torch.from_numpy(synth.synth_mel(7, 1, 2048)).cuda()
        s = m.stream(rows, seed=1, stream_id=0)
        per = []
        for f in range(0, 2048, 32):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = s.push(mel_s[:, :, f:f + 32])
            torch.cuda.synchronize()
            if y.numel():
                per.append(time.perf_counter() - t0)
        s.close()
        res.update(push_ms_median=statistics.median(per[2:]) * 1e3, push_ms_max=max(per[2:]) * 1e3, pushes=len(per))
        print(f"SampleStream.push per 32-frame chunk: median {res['push_ms_median']:.2f} ms, max {res['push_ms_max']:.2f} ms "
              f"({len(per)} pushes that returned samples; 32 frames = {32 * 256 / 22050 * 1e3:.0f} ms of audio)", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
