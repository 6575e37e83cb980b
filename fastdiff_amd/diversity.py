"""NDB and JSD on the device: does a sampler cover the sounds of the corpus, or does it collapse onto fewer of them?

The FastDiff paper's objective table reports the number of statistically different bins (NDB) and the Jensen-Shannon divergence (JSD) of
Richardson & Weiss, "On GANs and GMMs" (2018), next to STOI and PESQ; the reference has no code for them, and the authors' code is not
here either: this module restates the published method.  The training samples -- here the mel frames of the corpus, 80 features each --
are clustered into K bins with k-means; the generated samples are assigned to the same bins; per bin a two-proportion z-test says
whether the two sets fill it differently (NDB counts those bins), and JSD compares the two bin histograms.  The paper does not state K,
so K is a parameter (50 by default).  Every other score of the project is pairwise (one vocoded waveform against its recording); this
one is a score of a whole run against the corpus.

Lloyd's iteration is one fused kernel per pass (fd_bins_pass, include/fastdiff_hip_ext.h, which defines the arithmetic): the rows are
read once, standardised on the fly, multiplied with the centroids on the exact-fp32 matrix instruction, and the per-bin sums are a second
product on it; no [N, K] matrix reaches memory and the corpus arena is used where it lies.

    frames(mels, lens=None)      [B, 80, T] device mels -> the packed [N, 80] matrix of the valid frames
    fit(x, K=50, iters=100, n_init=3, seed=0, standardize=True, check_every=8, ld=None)      -> Bins
    Bins.counts(x) / .score(x, alpha=0.05) / .save(path) / Bins.load(path)
    ndb_jsd(ref_counts, counts, alpha=0.05)      the statistics, numpy float64 on the host
    bins_pass(x, centroids, ...)                 one pass, as the C call takes it
    python -m fastdiff_amd.diversity fit (--binary_dir D | --wav_dir D) --out bins.npz [--K 50 ...]

A record is a dict: counts (int64 [K]), inertia (float), moved, nonfinite, empty, status (int).
"""
import argparse
import math

import numpy as np
import torch

from . import _capi, _wave

CHUNK, MAX_K, MAX_D = _capi.FD_BINS_CHUNK, _capi.FD_BINS_MAX_K, _capi.FD_BINS_MAX_D
OK, NONFINITE, EMPTY = _capi.FD_BINS_OK, _capi.FD_BINS_NONFINITE, _capi.FD_BINS_EMPTY
STATUS = {OK: "OK", NONFINITE: "NONFINITE", EMPTY: "EMPTY"}
RECORD = _capi.record("fd_bins")


def ndb_jsd(ref_counts, counts, alpha=0.05):
    """The two statistics of Richardson & Weiss 2018 from two bin histograms (int arrays [K]); a restatement of the published method,
    not of the authors' code.  Per bin P = r / n_r, Q = q / n_q, the pooled p = (r + q) / (n_r + n_q), se = sqrt(p (1 - p) (1 / n_r +
    1 / n_q)); the bin is different when se > 0 and the two-sided p-value erfc(|P - Q| / se / sqrt 2) < alpha.  jsd = KL(P || M) / 2 +
    KL(Q || M) / 2 with M = (P + Q) / 2, in nats, 0 log 0 = 0.  Pure numpy float64.
    -> {"ndb", "ndb_over_k", "jsd", "z" [K] ((P - Q) / se, 0 where se = 0), "different" [K] bool, "counts" [K], "n"}"""
    r, q = np.asarray(ref_counts, np.float64).reshape(-1), np.asarray(counts, np.float64).reshape(-1)
    if r.shape != q.shape or r.size < 1:
        raise ValueError(f"ndb_jsd: histograms of {r.size} and {q.size} bins")
    if (r < 0).any() or (q < 0).any():
        raise ValueError("ndb_jsd: a negative count")
    n_r, n_q = r.sum(), q.sum()
    if n_r <= 0 or n_q <= 0:
        raise ValueError("ndb_jsd: an empty histogram")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"ndb_jsd: alpha = {alpha} outside (0, 1)")
    P, Q = r / n_r, q / n_q
    p = (r + q) / (n_r + n_q)
    se = np.sqrt(p * (1.0 - p) * (1.0 / n_r + 1.0 / n_q))
    z = np.zeros_like(P)
    np.divide(P - Q, se, out=z, where=se > 0)
    pval = np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z])
    different = (se > 0) & (pval < alpha)
    M = 0.5 * (P + Q)

    def kl(A):
        t = np.zeros_like(A)
        np.divide(A, M, out=t, where=A > 0)
        np.log(t, out=t, where=A > 0)
        return float(np.sum(A * t))

    return {"ndb": int(different.sum()), "ndb_over_k": float(different.sum()) / r.size, "jsd": 0.5 * kl(P) + 0.5 * kl(Q), "z": z,
            "different": different, "counts": np.asarray(counts).reshape(-1).astype(np.int64), "n": int(n_q)}


def frames(mels, lens=None):
    """mels [B, 80, T] (or [80, T]) on the device -> [N, 80] float32, the frames t < lens[b] of every item in batch order (lens None:
    all T).  Torch plumbing: one transposition and one gather."""
    if not isinstance(mels, torch.Tensor) or not mels.is_cuda:
        raise ValueError("diversity.frames: a tensor on the HIP device is expected (there is no CPU path)")
    if mels.dim() == 2:
        mels = mels.unsqueeze(0)
    if mels.dim() != 3:
        raise ValueError(f"diversity.frames: expected mels [B, D, T], got {list(mels.shape)}")
    B, D, T = mels.shape
    rows = mels.float().transpose(1, 2).reshape(B * T, D)
    if lens is None:
        return rows.contiguous()
    if len(lens) != B or any(not 0 <= int(v) <= T for v in lens):
        raise ValueError(f"diversity.frames: lens {list(lens)} for a batch [{B}, {D}, {T}]")
    idx = torch.cat([torch.arange(b * T, b * T + int(v)) for b, v in enumerate(lens)]).to(mels.device)
    return rows.index_select(0, idx).contiguous()


def _matrix(x, ld, who):
    """x -> (x, N, D, ld): a contiguous [N, D] matrix, or with ld a [N, D] view whose rows lie ld floats apart (the leading D of wider
    rows)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: a tensor is expected, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{who}: float32 rows are expected, got {x.dtype}")
    if ld is None:
        if x.dim() != 2 or not x.is_contiguous():
            raise ValueError(f"{who}: a contiguous [N, D] matrix is expected, got {list(x.shape)} with strides {list(x.stride())}")
        return x, int(x.shape[0]), int(x.shape[1]), int(x.shape[1])
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) != int(ld):
        raise ValueError(f"{who}: with ld = {ld} a [N, D] view whose rows lie ld floats apart is expected, got {list(x.shape)} with strides {list(x.stride())}")
    return x, int(x.shape[0]), int(x.shape[1]), int(ld)


def _need_device(x, who):
    """Last of the refusals, so that the others can be met without a device."""
    if not x.is_cuda:
        raise ValueError(f"{who}: a tensor on the HIP device is expected (there is no CPU path)")


def _check_shape(N, D, K, who):
    if N < 1:
        raise ValueError(f"{who}: no rows")
    if D < 4 or D > MAX_D or D % 4:
        raise ValueError(f"{who}: D = {D} features: a multiple of 4 in 4 .. {MAX_D} is expected")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: K = {K} bins outside 1 .. {MAX_K}")


def _pass(lib, handle, stream, x, N, D, ld, shift, scale, centroids, assign, out, rec):
    """fd_bins_pass on the stream; nothing synchronises."""
    rc = lib.fd_bins_pass(handle, x.data_ptr(), N, D, ld, shift.data_ptr() if shift is not None else None, scale.data_ptr() if scale is not None else None,
                          centroids.data_ptr(), int(centroids.shape[0]), assign.data_ptr() if assign is not None else None,
                          out.data_ptr() if out is not None else None, rec.data_ptr() if rec is not None else None, stream)
    _capi.check(lib, handle, rc, "fd_bins_pass")


def _record(rec, K):
    r = rec.cpu().numpy().view(RECORD).reshape(-1)[0]
    return {"counts": r["counts"][:K].copy(), "inertia": float(r["inertia"]), "moved": int(r["moved"]), "nonfinite": int(r["nonfinite"]),
            "empty": int(r["empty"]), "status": int(r["status"])}


def _vec(v, D, device, who, name):
    if v is None:
        return None
    v = torch.as_tensor(v, dtype=torch.float32, device=device).contiguous()
    if v.shape != (D,):
        raise ValueError(f"{who}: {name} of shape {list(v.shape)}, [{D}] expected")
    return v


def bins_pass(x, centroids, shift=None, scale=None, assign=None, update=False, ld=None, record=True):
    """One pass of Lloyd's algorithm (fd_bins_pass): x [N, D] float32 on the device (ld: see fit), centroids [K, D], shift / scale [D]
    or None, assign: an int32 [N] device tensor with the previous assignments (-1: none), overwritten with the new ones, or None.
    -> (record or None, new centroids [K, D] or None).  One synchronisation when the record is asked for."""
    who = "diversity.bins_pass"
    x, N, D, ld = _matrix(x, ld, who)
    centroids = torch.as_tensor(centroids, dtype=torch.float32, device=x.device).contiguous()
    if centroids.dim() != 2 or centroids.shape[1] != D:
        raise ValueError(f"{who}: centroids of shape {list(centroids.shape)} for rows of {D} features")
    K = int(centroids.shape[0])
    _check_shape(N, D, K, who)
    if (shift is None) != (scale is None):
        raise ValueError(f"{who}: shift and scale come together")
    shift, scale = _vec(shift, D, x.device, who, "shift"), _vec(scale, D, x.device, who, "scale")
    if assign is not None and (not isinstance(assign, torch.Tensor) or assign.dtype != torch.int32 or assign.device != x.device or assign.shape != (N,)
                               or not assign.is_contiguous()):
        raise ValueError(f"{who}: assign must be a contiguous int32 [{N}] tensor on the rows' device")
    if not update and not record and assign is None:
        raise ValueError(f"{who}: nothing is asked for")
    _need_device(x, who)
    out = torch.empty((K, D), dtype=torch.float32, device=x.device) if update else None
    rec = torch.empty((RECORD.itemsize,), dtype=torch.uint8, device=x.device) if record else None
    lib, handle, stream = _wave.default_handle(x)
    _pass(lib, handle, stream, x, N, D, ld, shift, scale, centroids, assign, out, rec)
    return (_record(rec, K) if record else None), out


def standardization(x, ld=None):
    """(shift, scale) float32 [D] on the rows' device: the per-feature mean and 1 / std (population) over the rows, computed in float64
    with torch; a feature of zero variance gets scale 1."""
    x, N, D, ld = _matrix(x, ld, "diversity.standardization")
    if N < 1:
        raise ValueError("diversity.standardization: no rows")
    x64 = x.double()
    mean = x64.mean(0)
    std = (x64 - mean).pow(2).mean(0).sqrt()
    scale = torch.where(std > 0, 1.0 / std, torch.ones_like(std))
    return mean.float().contiguous(), scale.float().contiguous()


def initial_rows(N, K, seed):
    """The rows the initial centroids of a restart are taken from: the first K entries of torch.randperm(N) drawn on the CPU from
    torch.Generator().manual_seed(seed) (seed = the fit's seed + the restart's number)."""
    return torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K]


class Bins:
    """Fitted bins: centroids [K, D], shift, scale [D] (numpy float32; shift = 0 and scale = 1 without standardisation), ref_counts [K]
    int64 (the fitting set's histogram), inertia (float), passes (int), K, D."""

    def __init__(self, centroids, shift, scale, ref_counts, inertia, passes):
        self.centroids = np.ascontiguousarray(centroids, np.float32)
        self.K, self.D = (int(v) for v in self.centroids.shape)
        self.shift, self.scale = np.ascontiguousarray(shift, np.float32).reshape(self.D), np.ascontiguousarray(scale, np.float32).reshape(self.D)
        self.ref_counts = np.ascontiguousarray(ref_counts, np.int64).reshape(self.K)
        self.inertia, self.passes = float(inertia), int(passes)
        self._dev = {}

    def _on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.centroids, self.shift, self.scale))
        return self._dev[key]

    def counts(self, x, ld=None):
        """The histogram of the rows x [N, D] over the bins (int64 [K]): one assignment pass; rows that are not finite are left out."""
        x, N, D, ld = _matrix(x, ld, "Bins.counts")
        if D != self.D:
            raise ValueError(f"Bins.counts: rows of {D} features, the bins have {self.D}")
        c, sh, sc = self._on(x.device)
        return bins_pass(x, c, sh, sc, ld=ld)[0]["counts"]

    def score(self, x, alpha=0.05, ld=None):
        """ndb_jsd of the rows x against the fitting set."""
        return ndb_jsd(self.ref_counts, self.counts(x, ld=ld), alpha)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, centroids=self.centroids, shift=self.shift, scale=self.scale, ref_counts=self.ref_counts, inertia=np.float64(self.inertia),
                     passes=np.int64(self.passes))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["centroids"], z["shift"], z["scale"], z["ref_counts"], float(z["inertia"]), int(z["passes"]))


def fit(x, K=50, iters=100, n_init=3, seed=0, standardize=True, check_every=8, ld=None):
    """K-means over the rows x [N, D] (float32 on the device, contiguous; or with ld a [N, D] view of rows that lie ld floats apart, e.g.
    buffer[:, :D] of a wider matrix -- never copied) -> Bins.
    shift / scale: standardization(x) when standardize, else 0 / 1.  Restart r of n_init starts from the rows initial_rows(N, K, seed + r)
    (standardised on the host side of the call exactly as the kernel does: two float32 roundings) and runs passes of fd_bins_pass until
    one moves no row or `iters` passes are done.  The record is read back only every check_every passes (the passes in between are only
    enqueued), so up to check_every - 1 passes beyond convergence may run: they change nothing, a pass that moves no row reproduces its
    centroids.  The restart with the lowest inertia (of its last pass' assignment against the centroids that pass started from) wins, the
    first of equal ones."""
    who = "diversity.fit"
    x, N, D, ld = _matrix(x, ld, who)
    K, iters, n_init, check_every = int(K), int(iters), int(n_init), int(check_every)
    _check_shape(N, D, K, who)
    if K > N:
        raise ValueError(f"{who}: K = {K} bins for {N} rows")
    if iters < 1 or n_init < 1 or check_every < 1:
        raise ValueError(f"{who}: iters = {iters}, n_init = {n_init}, check_every = {check_every}: each at least 1")
    _need_device(x, who)
    dev = x.device
    if standardize:
        shift, scale = standardization(x, ld)
    else:
        shift, scale = torch.zeros(D, dtype=torch.float32, device=dev), torch.ones(D, dtype=torch.float32, device=dev)
    lib, handle, stream = _wave.default_handle(x)
    best = None
    for r in range(n_init):
        rows = initial_rows(N, K, int(seed) + r).to(dev)
        cur = ((x.index_select(0, rows) - shift) * scale).contiguous()
        assign = torch.full((N,), -1, dtype=torch.int32, device=dev)
        recs = [torch.empty((RECORD.itemsize,), dtype=torch.uint8, device=dev) for _ in range(check_every)]
        passes, last = 0, None
        while passes < iters and last is None:
            n = min(check_every, iters - passes)
            kept = []
            for j in range(n):
                nxt = torch.empty((K, D), dtype=torch.float32, device=dev)
                _pass(lib, handle, stream, x, N, D, ld, shift, scale, cur, assign, nxt, recs[j])
                kept.append((cur, nxt))
                cur = nxt
            got = [_record(t, K) for t in recs[:n]]
            for j, g in enumerate(got):
                if g["moved"] == 0:
                    last = (passes + j + 1, g, kept[j][0])
                    break
            passes += n
            if last is None and passes >= iters:
                last = (passes, got[-1], kept[-1][0])
        done, rec, cent = last
        if best is None or rec["inertia"] < best[1]["inertia"]:
            best = (done, rec, cent)
    done, rec, cent = best
    return Bins(cent.cpu().numpy(), shift.cpu().numpy(), scale.cpu().numpy(), rec["counts"], rec["inertia"], done)


def score_waveforms(model, bins, wavs, variant="pwg", alpha=0.05):
    """The corpus-level score of a run: every waveform (float in [-1, 1] or int16 PCM, numpy or tensor, 22.05 kHz) goes through the mel
    front-end on the device (FastDiff.mel_spectrogram), its frames are counted in `bins`, and ndb_jsd compares the sum with the fitting
    set."""
    total = np.zeros(bins.K, np.int64)
    for w in wavs:
        t = torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w)
        t = (t.to("cuda").float() / 32768.0) if t.dtype == torch.int16 else t.to("cuda").float()
        mel = model.mel_spectrogram(t.reshape(1, -1), variant=variant)
        total += bins.counts(frames(mel))
    return ndb_jsd(bins.ref_counts, total, alpha)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fit the k-means bins of NDB / JSD on a corpus' mel frames, on the device")
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit", help="fit the bins and write them as an npz")
    src = f.add_mutually_exclusive_group(required=True)
    src.add_argument("--binary_dir", help="the reference's binarized set (train.data / train.idx / train_lengths.npy)")
    src.add_argument("--wav_dir", help="a directory of recordings: the mels are computed on the device")
    f.add_argument("--out", required=True, metavar="bins.npz")
    f.add_argument("--K", type=int, default=50)
    f.add_argument("--iters", type=int, default=100)
    f.add_argument("--n_init", type=int, default=3)
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--mel_variant", default="pwg", choices=("pwg", "tacotron"))
    f.add_argument("--no_standardize", action="store_true")
    args = ap.parse_args(argv)
    from . import FastDiff, TrainCorpus
    if args.binary_dir:
        corpus = TrainCorpus.from_binary_dir(args.binary_dir, device="cuda")
    else:
        corpus = TrainCorpus.from_wav_dir(FastDiff().cuda().eval(), args.wav_dir, mel_variant=args.mel_variant)
    bins = corpus.fit_bins(K=args.K, iters=args.iters, n_init=args.n_init, seed=args.seed, standardize=not args.no_standardize)
    bins.save(args.out)
    print(f"{args.out}: K = {bins.K} bins over {int(bins.ref_counts.sum())} frames, inertia {bins.inertia:.6g} after {bins.passes} passes, "
          f"{int((bins.ref_counts == 0).sum())} empty")


if __name__ == "__main__":
    main()
