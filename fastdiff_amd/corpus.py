"""A training corpus kept in device memory, and the host twin of the device's choice of a batch (INTEGRATION.md "Training").

What the reference builds per step on the host -- VocoderDataset.__getitem__ (unpickle an item, two FloatTensors) and collater (a random
window per item, pad, transpose: tasks/vocoder/dataset_utils.py:80-160) behind a DataLoader and a pinned copy -- is here one kernel
inside the captured step (fd_train_collate, lvc_op.train_collate): the whole set lies in two flat float32 arenas on the device, and the
utterance and the window of every slot of every step are a pure function of (seed, step index, slot, rank, world size).  TrainCorpus.plan
evaluates that function on the host in integer arithmetic, equal to the kernel's result: it is what a run logs, and what says which
batches a resumed run (TrainStep.load_state_dict restores the step index) will see.

    corpus = fastdiff_amd.TrainCorpus.from_binary_dir("data/binary/LJSpeech")
    ts = fastdiff_amd.TrainStep(model, diffusion_hyperparams, corpus=corpus, batch_size=20)
    for it in range(steps):
        loss = ts.step()                                   # no argument, no byte from the host
    items, starts = corpus.plan(it, 20)                    # the batch of step `it`

The choice (include/fastdiff_hip_train.h: fd_train_collate): slot b of step `it` stands at the global position g = (it B + b) world + rank
-- consecutive batches of EndlessDistributedSampler's indices[rank::world] -- in epoch e = g // n at place j = g % n, and takes item
pi_e(j): a keyed bijection of [0, n) evaluated per element (a 4-round balanced Feistel network over Philox4x32-10, walked along its
cycle into [0, n)).  Not torch.randperm's order.  The window starts at frame (w (T - F)) >> 32 with w a 32-bit Philox word: uniform on
[0, T - F), the range of the reference's np.random.randint(0, len(c) - F).
"""
import os
import pickle

import numpy as np
import torch

N_MELS = 80
PERM_STREAM, START_STREAM = 0xFFFFFFFB, 0xFFFFFFFC      # the Philox streams of pi's round function and of the start draw
MAX_ITEMS = 1 << 28
_M32, _M64 = np.uint64(0xFFFFFFFF), (1 << 64) - 1
_S32 = np.uint64(32)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words; returns the four output words."""
    mul0, mul1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for i in range(10):
        p0, p1 = mul0 * c0, mul1 * c2                       # 32 x 32 -> 64 bit: no overflow in uint64
        rk0, rk1 = (k0 + np.uint64(i * 0x9E3779B9)) & _M32, (k1 + np.uint64(i * 0xBB67AE85)) & _M32
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ rk0, p1 & _M32, (p0 >> _S32) ^ c3 ^ rk1, p0 & _M32
    return c0, c1, c2, c3


def _words(seed, stream, pos, uid):
    """The generator as the kernels key it: counter = (pos lo, pos hi ^ uid lo, stream, 0x5EED ^ uid hi), key = (seed lo, seed hi)."""
    seed, pos, uid = np.uint64(int(seed) & _M64), np.asarray(pos, np.uint64), np.asarray(uid, np.uint64)
    return _philox4x32_10(pos & _M32, (pos >> _S32) ^ (uid & _M32), np.uint64(stream), np.uint64(0x5EED) ^ (uid >> _S32), seed & _M32, seed >> _S32)


def _permute(j, n, seed, epoch):
    """pi_epoch(j) for uint64 arrays j < n and epoch of one shape."""
    k = 0
    while (1 << (2 * k)) < n:
        k += 1
    kk, mask = np.uint64(k), np.uint64((1 << k) - 1)
    x = np.array(j, np.uint64)
    todo = np.ones(x.shape, bool)
    while todo.any():
        v, e = x[todo], epoch[todo]
        hi, lo = v >> kk, v & mask
        for rnd in range(4):
            f = _words(seed, PERM_STREAM, lo ^ np.uint64(rnd << 28), e)[0]
            hi, lo = lo, hi ^ (f & mask)
        x[todo] = (hi << kk) | lo
        todo = x >= np.uint64(n)
    return x


def _name(i, item):
    name = item.get("item_name") if hasattr(item, "get") else None
    return f"item {i}" + (f" ({name})" if name is not None else "")


class TrainCorpus:
    """items: a sequence of mappings with "mel" ([T, 80], frame-major as the reference's binarizer writes it) and "wav" ([>= T hop]).
    Kept: the items the reference keeps (T - 2 aux_context_window > F = max_samples // hop_size, dataset_utils.py:68-72); n_skipped counts
    the others, `kept` lists the positions of the kept ones in `items`.

    wav [sum T_i hop], mel [sum T_i, 80] (float32: what torch.FloatTensor(item[...]) holds) and frame_off [n + 1] (int64 frame prefix
    sums) are tensors on `device` (None: the HIP device if there is one, else the CPU); lengths / frame_off_host are their host copies.
    A corpus on the CPU does everything but feed the kernel: .to(device) uploads it."""

    @staticmethod
    def _geometry(hop_size, max_samples, aux_context_window):
        if aux_context_window != 0:
            raise NotImplementedError("TrainCorpus: aux_context_window = 0 only (base.yaml's value; the model takes wavs of exactly T * hop samples)")
        hop, F = int(hop_size), int(max_samples) // int(hop_size)
        if hop < 4 or hop % 4 != 0:
            raise ValueError(f"TrainCorpus: hop_size = {hop_size} must be a multiple of 4 (whatever the items)")
        if F < 1:
            raise ValueError(f"TrainCorpus: max_samples = {max_samples} is shorter than one frame of {hop} samples (whatever the items)")
        return hop, F

    def __init__(self, items, hop_size=256, max_samples=25600, aux_context_window=0, device=None):
        hop, F = self._geometry(hop_size, max_samples, aux_context_window)
        mels, wavs, kept = [], [], []
        for i, item in enumerate(items):
            mel, wav = np.asarray(item["mel"]), np.asarray(item["wav"]).reshape(-1)
            if mel.ndim != 2 or mel.shape[1] != N_MELS:
                raise ValueError(f"TrainCorpus: {_name(i, item)}: mel of shape {tuple(mel.shape)}, [T, {N_MELS}] expected")
            T = mel.shape[0]
            if wav.shape[0] < T * hop:
                raise ValueError(f"TrainCorpus: {_name(i, item)}: wav of {wav.shape[0]} samples is shorter than T * hop = {T} * {hop}")
            if T > F:
                mels.append(np.ascontiguousarray(mel, np.float32))
                wavs.append(np.ascontiguousarray(wav[: T * hop], np.float32))
                kept.append(i)
        self.n_skipped = len(items) - len(kept)
        if not kept:
            raise ValueError(f"TrainCorpus: no item is longer than {F} frames: item 0 .. item {len(items) - 1} are all skipped" if len(items)
                             else "TrainCorpus: no item at all (item 0 is missing)")
        if len(kept) > MAX_ITEMS:
            raise ValueError(f"TrainCorpus: {len(kept)} items; item {kept[MAX_ITEMS]} is one too many (2^28 at most)")
        self.hop_size, self.frames, self.max_samples = hop, F, int(max_samples)
        self.kept = np.asarray(kept, np.int64)
        self.lengths = np.asarray([m.shape[0] for m in mels], np.int64)
        self.frame_off_host = np.concatenate([np.zeros(1, np.int64), np.cumsum(self.lengths)])
        self.mel = torch.from_numpy(np.concatenate(mels, axis=0))
        self.wav = torch.from_numpy(np.concatenate(wavs))
        self.frame_off = torch.from_numpy(self.frame_off_host.copy())
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self._move(torch.device(device))

    def _move(self, device):
        self.mel, self.wav, self.frame_off = (t.to(device) for t in (self.mel, self.wav, self.frame_off))
        self.device = self.wav.device

    def to(self, device):
        """This corpus with its arenas on `device` (itself when they already are there)."""
        device = torch.device(device)
        if device.type == self.device.type and (device.index is None or device.index == self.device.index):
            return self
        other = object.__new__(TrainCorpus)
        other.__dict__.update(self.__dict__)
        other._move(device)
        return other

    @property
    def n_items(self):
        return int(self.lengths.shape[0])

    def __len__(self):
        return self.n_items

    @classmethod
    def from_binary_dir(cls, data_dir, prefix="train", **kw):
        """The reference's binarized set: {prefix}_lengths.npy (frames per item), {prefix}.idx (an np.save'd dict with 'offsets': the byte
        offsets of the items) and {prefix}.data (one pickle per item with at least 'mel' and 'wav').  Items the lengths file rules out
        are not unpickled; `kept` and `n_skipped` refer to the whole set."""
        base = os.path.join(data_dir, prefix)
        lengths = np.load(base + "_lengths.npy")
        offsets = np.load(base + ".idx", allow_pickle=True).item()["offsets"]
        if len(offsets) != len(lengths) + 1:
            raise ValueError(f"TrainCorpus.from_binary_dir: {base}.idx holds {len(offsets) - 1} items, {base}_lengths.npy {len(lengths)}")
        F = int(kw.get("max_samples", 25600)) // int(kw.get("hop_size", 256))
        aux = int(kw.get("aux_context_window", 0))
        long_enough = [i for i, s in enumerate(lengths) if int(s) - 2 * aux > F]
        items = []
        with open(base + ".data", "rb") as f:
            for i in long_enough:
                f.seek(int(offsets[i]))
                item = pickle.loads(f.read(int(offsets[i + 1]) - int(offsets[i])))
                items.append({"mel": item["mel"], "wav": item["wav"], "item_name": item.get("item_name", f"{prefix}[{i}]")})
        corpus = cls(items, **kw)
        corpus.kept = np.asarray(long_enough, np.int64)[corpus.kept]
        corpus.n_skipped = len(lengths) - corpus.n_items
        return corpus

    @classmethod
    def from_wav_dir(cls, model, wav_dir, sample_rate=22050, mel_variant="pwg", hop_size=256, max_samples=25600, aux_context_window=0,
                     device=None, loud_norm=False, trim_long_sil=False):
        """A corpus straight from recordings, without the reference's binarizer (which needs librosa): every *.wav below `wav_dir`, in
        sorted order, goes through what process_utterance does per item (data_gen/tts/data_gen_utils.py:93-147), on the device of
        `model` (a FastDiff on the GPU): any rate, sample type and channel count -> float mono at `sample_rate` (infer.wav_to_device:
        FastDiff.resample), the mel of T = 1 + n // hop frames (FastDiff.mel_spectrogram), the wav zero-padded at its end to T * hop
        samples and cut there (:138-140).  One recording at a time -- peak memory is one recording plus the arenas -- and nothing comes
        back to the host.  Items the length rule drops are counted in n_skipped, `kept` lists the positions of the kept ones among the
        sorted files.  loud_norm: the reference's `loud_norm: true` -- every recording is brought to -22 LUFS (infer.loud_norm_wav) before its
        mel is taken and before the corpus keeps it; one shorter than a 400 ms block raises ValueError naming the file.  trim_long_sil: the
        reference's `trim_long_sil: true` -- the long silences of every recording are cut first (infer.trim_long_sil_wav, in front of
        loud_norm as in process_utterance, :108-120); a recording of which no window is kept is skipped and counted in n_skipped."""
        import glob
        from scipy.io import wavfile
        from . import infer
        hop, F = cls._geometry(hop_size, max_samples, aux_context_window)
        if hop != model.hop_length:
            raise ValueError(f"TrainCorpus.from_wav_dir: hop_size = {hop_size}, the model's mel front-end has {model.hop_length}")
        paths = sorted(glob.glob(f"{wav_dir}/*.wav"))
        mels, wavs, kept = [], [], []
        for i, path in enumerate(paths):
            sr, pcm = wavfile.read(path)
            wav = infer.wav_to_device(model, pcm, sr, sample_rate, path)
            if trim_long_sil:
                wav = infer.trim_long_sil_wav(model, wav, sample_rate, path)
                if wav.shape[0] == 0:                      # SILENT: no window kept
                    continue
            if loud_norm:
                wav = infer.loud_norm_wav(model, wav, sample_rate, path)
            T = 1 + wav.shape[0] // hop
            if T <= F:                                     # dataset_utils.py:68-72 would drop it: no mel computed
                continue
            mels.append(model.mel_spectrogram(wav, variant=mel_variant)[0].transpose(0, 1).contiguous())      # [T, 80] as the binarizer stores it
            wavs.append(torch.nn.functional.pad(wav, (0, T * hop - wav.shape[0])))
            kept.append(i)
        if not kept:
            raise ValueError(f"TrainCorpus.from_wav_dir: none of the {len(paths)} recordings below {wav_dir} is longer than {F} frames")
        if len(kept) > MAX_ITEMS:
            raise ValueError(f"TrainCorpus.from_wav_dir: {len(kept)} items (2^28 at most)")
        self = object.__new__(cls)
        self.n_skipped = len(paths) - len(kept)
        self.hop_size, self.frames, self.max_samples = hop, F, int(max_samples)
        self.kept = np.asarray(kept, np.int64)
        self.lengths = np.asarray([m.shape[0] for m in mels], np.int64)
        self.frame_off_host = np.concatenate([np.zeros(1, np.int64), np.cumsum(self.lengths)])
        self.mel, self.wav = torch.cat(mels, dim=0), torch.cat(wavs)
        self.frame_off = torch.from_numpy(self.frame_off_host.copy())
        self._move(torch.device(device) if device is not None else self.wav.device)
        return self

    def plan(self, iteration, batch_size, seed=0, rank=0, world_size=1):
        """(items [B], starts [B]) int64: what fd_train_collate picks for step `iteration` -- equal, not close.  Pure integer numpy."""
        B, world, rank, n = int(batch_size), int(world_size), int(rank), self.n_items
        if B < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"TrainCorpus.plan: batch_size={batch_size}, rank={rank} of world_size={world_size}")
        it = int(iteration) & _M64
        g = [((it * B + b) * world + rank) & _M64 for b in range(B)]
        items = _permute(np.array([x % n for x in g], np.uint64), n, seed, np.array([x // n for x in g], np.uint64)).astype(np.int64)
        b = np.arange(B, dtype=np.uint64)
        w = np.stack(_words(seed, START_STREAM, b >> np.uint64(2), np.uint64(it)), axis=-1)[np.arange(B), (b & np.uint64(3)).astype(np.int64)]
        starts = (w * (self.lengths[items] - self.frames).astype(np.uint64)) >> _S32
        return items, starts.astype(np.int64)

    def eval_plan(self, batch, batch_size, seed=0, fill=False):
        """picks [B, 2] int64: what fd_eval_collate reports for batch `batch` of an evaluation pass -- equal, not close.  Slot b is item
        batch B + b at start (w (T - F)) >> 32, w the start word of plan() under id = batch; a slot behind the last item is (-1, -1).
        fill=True: what the kernel CUTS instead, i.e. such a slot reads (n - 1, its start in item n - 1).  Pure integer numpy."""
        B, n, j = int(batch_size), self.n_items, int(batch) & _M64
        if B < 1:
            raise ValueError(f"TrainCorpus.eval_plan: batch_size={batch_size}")
        g = np.array([(j * B + b) & _M64 for b in range(B)], dtype=object)
        active = np.array([x < n for x in g], bool)
        items = np.array([int(x) if x < n else n - 1 for x in g], np.int64)
        b = np.arange(B, dtype=np.uint64)
        w = np.stack(_words(seed, START_STREAM, b >> np.uint64(2), np.uint64(j)), axis=-1)[np.arange(B), (b & np.uint64(3)).astype(np.int64)]
        starts = ((w * (self.lengths[items] - self.frames).astype(np.uint64)) >> _S32).astype(np.int64)
        picks = np.stack([items, starts], axis=1)
        if not fill:
            picks[~active] = -1
        return picks

    def fit_bins(self, **kw):
        """The k-means bins of NDB / JSD (fastdiff_amd.diversity.fit) over every mel frame of the corpus, on the arena where it lies:
        nothing is copied.  Keywords as diversity.fit takes them (K, iters, n_init, seed, standardize, check_every)."""
        from . import diversity
        return diversity.fit(self.mel, **kw)

    def cut(self, items, starts):
        """(mels [B, 80, F], wavs [B, 1, F hop]) by torch slicing of the arenas, on their device: the reference's collater on given
        picks.  For inspection and tests; the training path is lvc_op.train_collate."""
        F, hop = self.frames, self.hop_size
        first = [int(self.frame_off_host[i]) + int(s) for i, s in zip(items, starts)]
        mels = torch.stack([self.mel[p: p + F].t() for p in first]).contiguous()
        wavs = torch.stack([self.wav[p * hop: (p + F) * hop] for p in first]).unsqueeze(1).contiguous()
        return mels, wavs
