"""tools/resample_probe.py -- kernel time of fd_resample for B = 8 x 10 s, both directions, from the dispatches' own timestamps (library option profile = 1),
the enqueue-to-done time of back-to-back calls from device events, and scipy.signal.resample_poly on the host for the same job."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np, torch
from scipy import signal
import gpu_common
from fastdiff_amd import resample as rs

OUT = os.environ.get("FD_SESSION_OUT", os.path.join(ROOT, "session_out"))      # the results folder of the scripts under tools/
os.makedirs(OUT, exist_ok=True)
model = gpu_common.make_model()
rng = np.random.default_rng(0)
res = []
B = 8
for name, sr_in, sr_out, dtype, C in (("48k->22.05k f32 mono", 48000, 22050, np.float32, 1), ("48k->22.05k s16 stereo", 48000, 22050, np.int16, 2),
                                      ("22.05k->48k f32 mono", 22050, 48000, np.float32, 1), ("22.05k->16k f32 mono", 22050, 16000, np.float32, 1)):
    n = 10 * sr_in
    host = rng.standard_normal((B, n, C)).astype(np.float32) * 0.1
    if dtype == np.int16:
        host = np.round(host * 32767).clip(-32768, 32767).astype(np.int16)
    x = torch.from_numpy(host if C > 1 else host[:, :, 0].copy()).cuda()
    n_out = rs.out_len(n, sr_in, sr_out)
    nbytes = B * (n * C * host.dtype.itemsize + n_out * 4)
    for _ in range(5):
        y = model.resample(x, sr_in, sr_out, channels=C)
    torch.cuda.synchronize()
    # (1) the dispatches' own begin / end timestamps
    model.set_option("profile", "1")
    model.profile(reset=True)
    for _ in range(50):
        model.resample(x, sr_in, sr_out, channels=C)
    torch.cuda.synchronize()
    prof = model.profile(reset=True)
    model.set_option("profile", "0")
    launches, total_ms = prof["resample"]
    k_us = total_ms / launches * 1e3
    # (2) back-to-back calls between two device events, profiler off
    reps = 300
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        model.resample(x, sr_in, sr_out, channels=C)
    e1.record()
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    call_us = e0.elapsed_time(e1) / reps * 1e3
    # (3) the host, same job, the same filter
    h, up, down, _ = rs.taps(sr_in, sr_out)
    mono = (host.astype(np.float32).mean(axis=2) / (32768.0 if dtype == np.int16 else 1.0)).astype(np.float32)
    t0 = time.perf_counter()
    ys = [signal.resample_poly(mono[b], up, down, window=h.astype(np.float64) / up) for b in range(B)]
    t_host = time.perf_counter() - t0
    d = float(np.abs(y.cpu().numpy() - np.stack(ys)).max())
    K = rs.ratio(sr_in, sr_out)[3]
    r = dict(case=name, B=B, n_in=n, n_out=n_out, K=K, launches=launches, kernel_us=round(k_us, 2), bytes=nbytes, GBps=round(nbytes / k_us / 1e3, 1),
             frac_of_8TBps=round(nbytes / (k_us * 1e-6) / 8e12, 4), gflops=round(2.0 * B * n_out * K / k_us / 1e3, 1),
             call_us_back_to_back=round(call_us, 2), enqueue_us_per_call=round(t_enq / reps * 1e6, 2), scipy_resample_poly_ms=round(t_host * 1e3, 1),
             max_abs_diff_vs_scipy=d)
    print(json.dumps(r), flush=True)
    res.append(r)
json.dump(res, open(os.path.join(OUT, "resample_probe.json"), "w"), indent=1)
