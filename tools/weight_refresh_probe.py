"""Time of bringing a module's weights to its inference handle, both ways:  python tools/weight_refresh_probe.py [--reps 20]

  refresh_weights()    the packs rebuilt on the device from the live parameters (fd_refresh_weights_device), stream events around
                       one call, from enqueue to completion
  _upload_weights()    the host path (175 tensors to the CPU, fd_set_weight, fd_commit_weights: fold + pack on the host, one upload),
                       host clock around the call and a device synchronise
Medians over --reps runs after warm-up, and the bytes each refresh moves against the HBM rate.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastdiff_amd                      # noqa: E402
from fastdiff_amd import _capi            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    m = fastdiff_amd.FastDiff().cuda().eval()
    dev = next(m.parameters()).device
    lib, _ = m._ready(dev)
    read = sum(t.numel() * 4 for t in m.state_dict().values())
    written = int(m.weight_image().size)
    for _ in range(3):
        m.refresh_weights()
    torch.cuda.synchronize()
    assert m.last_refresh == "device", m.last_refresh
    dev_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.refresh_weights()
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    enq_ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        m.refresh_weights()
        enq_ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    host_ms = []
    for _ in range(a.host_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m._upload_weights(lib)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    host_ms = host_ms[1:]
    d = statistics.median(dev_ms)
    print(json.dumps({"refresh_device_ms": round(d, 4), "refresh_device_ms_min_max": [round(min(dev_ms), 4), round(max(dev_ms), 4)],
                      "refresh_enqueue_host_ms": round(statistics.median(enq_ms), 4),
                      "upload_host_ms": round(statistics.median(host_ms), 2), "upload_host_ms_all": [round(v, 2) for v in host_ms],
                      "bytes_read": read, "bytes_written": written,
                      "device_TB_per_s": round((read + written) / (d * 1e-3) / 1e12, 3), "share_of_8TBps": round((read + written) / (d * 1e-3) / 8e12, 3)}))


if __name__ == "__main__":
    main()
