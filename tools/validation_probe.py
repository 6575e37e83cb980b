"""Time of one held-out pass, two ways:  python tools/validation_probe.py [--items 200] [--batch 20] [--frames 100] [--rounds 7]

  validator    fastdiff_amd.Validator.run() over a device-resident corpus: every batch cut, drawn, evaluated and accumulated on the
               device, nothing read back inside the pass
  host recipe  the loop a trainer wrote by hand before: per batch a window per item cut from host arrays, two copies to the device,
               sampler.theta_timestep_loss under no_grad (draws on the CPU generator), .item()
Both cover the same --items utterances once at the same batch shape on the same module; stream events around each pass, the two sides
alternating, --rounds rounds after one warm-up round.  Median and range per side, one JSON line (LABBOOK R11.1).  The point of the
Validator is the fixed, per-noise-level evaluation, not this number: no ratio is required of it.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastdiff_amd                      # noqa: E402
from fastdiff_amd import schedules       # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    torch.manual_seed(0)
    hop, F, B = 256, a.frames, a.batch
    gen = torch.Generator().manual_seed(1)
    rng = np.random.RandomState(2)
    lengths = (F + 1 + rng.randint(0, 40, size=a.items)).tolist()
    items = [{"mel": torch.randn(T, 80, generator=gen).numpy(), "wav": (0.3 * torch.randn(T * hop, generator=gen)).numpy()} for T in lengths]
    cpu = fastdiff_amd.TrainCorpus(items, hop_size=hop, max_samples=F * hop, device="cpu")
    model = fastdiff_amd.FastDiff().cuda().eval()
    dh = schedules.training_hyperparams()
    val = fastdiff_amd.Validator(model, dh, corpus=cpu.to("cuda"), batch_size=B)

    def host_recipe():
        total, n = 0.0, 0
        with torch.no_grad():
            for j in range(0, len(items), B):
                mels, wavs = [], []
                for item in items[j: j + B]:
                    s = rng.randint(0, len(item["mel"]) - F)
                    mels.append(torch.from_numpy(item["mel"][s: s + F].T.copy()))
                    wavs.append(torch.from_numpy(item["wav"][s * hop: (s + F) * hop]).view(1, -1))
                loss = fastdiff_amd.theta_timestep_loss(model, (torch.stack(mels).cuda(), torch.stack(wavs).cuda()), dh)
                total, n = total + loss.item(), n + 1
        return total / n

    def device_pass():
        val.run()

    timed(device_pass), timed(host_recipe)          # warm-up: handles, scratch buffers, the first upload of the weights
    dev_ms, host_ms = [], []
    for _ in range(a.rounds):
        dev_ms.append(timed(device_pass)[0])
        host_ms.append(timed(host_recipe)[0])
    res = val.result()
    print(json.dumps({"items": a.items, "batch": B, "frames": F, "rounds": a.rounds,
                      "validator_ms": round(statistics.median(dev_ms), 3), "validator_ms_min_max": [round(min(dev_ms), 3), round(max(dev_ms), 3)],
                      "host_recipe_ms": round(statistics.median(host_ms), 3), "host_recipe_ms_min_max": [round(min(host_ms), 3), round(max(host_ms), 3)],
                      "validator_items": res["items"], "validator_nonfinite": res["nonfinite"]}))


if __name__ == "__main__":
    main()
