"""tools/loudness_probe.py -- kernel time of the loudness epilogue (FastDiff.loudness_normalize, out="int16") next to the peak epilogue
(FastDiff.peak_normalize_int16) on the same waveforms, from the dispatches' own timestamps (library option profile = 1), and the
enqueue-to-done time of back-to-back calls from device events: B = 8 x 221 184 samples (a micro-batch of 10 s utterances) and
B = 1 x 6.6 M samples (five minutes out of synthesize_long).  Also checks the device's reading against the float64 oracle once."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np, torch
import gpu_common
import loudness_ref as ref
from fastdiff_amd import loudness as ld

OUT = os.environ.get("FD_SESSION_OUT", os.path.join(ROOT, "session_out"))      # the results folder of the scripts under tools/
os.makedirs(OUT, exist_ok=True)
model = gpu_common.make_model()
rng = np.random.default_rng(0)
RATE, TARGET, res = 22050, -23.0, []
LOUD = ("loudness_pass1", "loudness_carry", "loudness_pass2", "loudness_gate", "loudness_apply")
PEAK = ("absmax", "to_int16")


def kernel_us(fn, names, reps=50):
    model.set_option("profile", "1")
    model.profile(reset=True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = model.profile(reset=True)
    model.set_option("profile", "0")
    return {k: round(prof[k][1] / reps * 1e3, 2) for k in names if k in prof}


def call_us(fn, reps=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 2), round(t_enq / reps * 1e6, 2)


for name, B, L in (("8 x 221184", 8, 221184), ("1 x 6.6M (long form)", 1, 6615000)):
    host = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    x = torch.from_numpy(host).cuda()
    loud = lambda: model.loudness_normalize(x, TARGET, sample_rate=RATE, out="int16")
    peak = lambda: model.peak_normalize_int16(x.unsqueeze(1))
    for _ in range(5):
        loud(), peak()
    torch.cuda.synchronize()
    rec = model.loudness(x, sample_rate=RATE)
    want = ref.measure(host[0], RATE)
    k_loud, k_peak = kernel_us(loud, LOUD), kernel_us(peak, PEAK)
    c_loud, c_peak = call_us(loud), call_us(peak)
    r = dict(case=name, B=B, L=L, tiles=-(-L // ld.TILE), blocks=int(rec["blocks"][0]), lufs=float(rec["lufs"][0]), lufs_oracle=want["lufs"],
             loudness_kernels_us=k_loud, loudness_sum_us=round(sum(k_loud.values()), 2), peak_kernels_us=k_peak,
             peak_sum_us=round(sum(k_peak.values()), 2), loudness_call_us_back_to_back=c_loud[0], loudness_enqueue_us=c_loud[1],
             peak_call_us_back_to_back=c_peak[0], peak_enqueue_us=c_peak[1], bytes_read_written=B * L * (3 * 4 + 2))
    print(json.dumps(r), flush=True)
    res.append(r)
json.dump(res, open(os.path.join(OUT, "loudness_probe.json"), "w"), indent=1)
