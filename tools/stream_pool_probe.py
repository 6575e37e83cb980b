"""StreamPool against S SampleStreams, and sample_long_batch against a loop of sample_long, one session (N = 4, chunk_frames = 32).

Per S in --streams: S live streams, each fed 32 frames per round; the wall time of one round (feeds included, ending in a device
synchronise), median over --rounds after --warmup.  "streams" mode pushes the chunks into S SampleStreams one after the other, "pool"
mode feeds a StreamPool and calls step() once.  "--package DIR" imports fastdiff_amd from DIR instead of this tree: a build of another
commit measured in the same session (boxes differ by up to 20 %); a package without StreamPool runs the "streams" and "long" parts only.
Second comparison: 8 utterances of 1500 frames through sample_long_batch against 8 sample_long calls.
Also reported: graph_captures / graph_evictions over the run (a pool whose number of ready streams varies captures one graph per
(windows, padded frames), and the cache holds 64)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the 8 x 1500-frame comparison")
    ap.add_argument("--package", default=None, help="directory that holds the fastdiff_amd package to measure (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the numbers as JSON here")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.package) if args.package else ROOT, os.path.join(ROOT, "oracle")]
    import torch
    import fastdiff_amd
    import synth
    from fastdiff_amd import infer

    m = fastdiff_amd.FastDiff()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(1234).items()})
    m = m.cuda().eval()
    N, chunk = 4, 32
    rows = infer._step_rows(m, N, None, None)
    H = m.halo_frames(N)
    has_pool = hasattr(m, "stream_pool")
    res = {"package": os.path.relpath(os.path.dirname(os.path.abspath(fastdiff_amd.__file__)), ROOT), "N": N, "chunk_frames": chunk, "rounds": args.rounds,
           "warmup": args.warmup, "has_pool": has_pool, "per_S": {}}
    total = H + chunk * (args.rounds + args.warmup + 1)
    counters = lambda: {k: m.counter(k) for k in ("graph_captures", "graph_evictions")}      # noqa: E731

    def rounds_of(one_round):
        ts = []
        for r in range(args.warmup + args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = one_round(H + chunk * r)
            torch.cuda.synchronize()
            if r >= args.warmup:
                ts.append(time.perf_counter() - t0)
            assert n == chunk * 256, n
        return {"median_ms": statistics.median(ts) * 1e3, "max_ms": max(ts) * 1e3, "min_ms": min(ts) * 1e3}

    with torch.no_grad():
        m.sample_long(torch.from_numpy(synth.synth_mel(1, 1, 64)).cuda(), rows)      # the handle and its weights
        for S in [int(v) for v in args.streams.split(",")]:
            mels = [torch.from_numpy(synth.synth_mel(100 + i, 1, total)).cuda() for i in range(S)]
            entry = {}
            streams = [m.stream(rows, seed=1, stream_id=i, chunk_frames=chunk) for i in range(S)]
            for s, mel in zip(streams, mels):
                assert s.push(mel[:, :, :H]).numel() == 0
            before = counters()

            def push_round(f):
                return min(s.push(mel[:, :, f:f + chunk]).numel() for s, mel in zip(streams, mels))

            entry["streams"] = rounds_of(push_round)
            entry["streams"].update({k: v - before[k] for k, v in counters().items()})
            if has_pool:
                pool = m.stream_pool(rows, seed=1, chunk_frames=chunk, max_streams=S, max_feed_frames=max(chunk, H))
                handles = [pool.open(i) for i in range(S)]
                for s, mel in zip(handles, mels):
                    pool.feed(s, mel[:, :, :H])
                assert pool.step() == {}
                before = counters()

                def pool_round(f):
                    for s, mel in zip(handles, mels):
                        pool.feed(s, mel[:, :, f:f + chunk])
                    out = pool.step()
                    assert len(out) == S
                    return min(y.numel() for y in out.values())

                entry["pool"] = rounds_of(pool_round)
                entry["pool"].update({k: v - before[k] for k, v in counters().items()})
                entry["pool_over_streams"] = entry["pool"]["median_ms"] / entry["streams"]["median_ms"]
            res["per_S"][str(S)] = entry
            print(f"S={S}: " + ", ".join(f"{k} {v['median_ms']:.3f} ms/round" for k, v in entry.items() if isinstance(v, dict)), flush=True)

        mels = [torch.from_numpy(synth.synth_mel(200 + i, 1, 1500)).cuda() for i in range(8)]

        def timed(fn):
            ts = []
            for r in range(args.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= 2:
                    ts.append(time.perf_counter() - t0)
            return statistics.median(ts) * 1e3

        res["long_8x1500"] = {"sample_long_loop_ms": timed(lambda: [m.sample_long(mel, rows, seed=1, stream_id=i) for i, mel in enumerate(mels)])}
        if hasattr(m, "sample_long_batch"):
            res["long_8x1500"]["sample_long_batch_ms"] = timed(lambda: m.sample_long_batch(mels, rows, seed=1))
            a = m.sample_long_batch(mels, rows, seed=1)
            assert all(torch.equal(y, m.sample_long(mel, rows, seed=1, stream_id=i)) for i, (y, mel) in enumerate(zip(a, mels)))
        print("8 x 1500 frames: " + ", ".join(f"{k} {v:.2f}" for k, v in res["long_8x1500"].items()), flush=True)
        res["counters_total"] = dict(counters(), graphs_resident=m.counter("graphs_resident"), workspace_bytes=m.counter("workspace_bytes"))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
