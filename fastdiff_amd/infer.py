"""Test-time batching / collation / sharding glue: what `tasks/run.py --infer` does around the hot path.

Reference behaviour restated (none of this is on the GPU path, so plain torch/numpy):
  * `VocoderDataset.load_mel_inputs` (tasks/vocoder/dataset_utils.py:186-204): every `*.npy` under `test_input_dir`, sorted,
    holds a mel of shape [T, 80]; item_name = path below the directory with "/" replaced by "_".
  * `VocoderDataset.collater` at test time (dataset_utils.py:100-160, `batch_max_frames = 0`): the random crop degenerates to
    frames [0, T-1) -- the LAST FRAME IS DROPPED (:116-125, interval_end = 1 so start_frame = 0); mels are zero-padded to the
    longest item of the batch (`collate_2d`, utils/__init__.py:136-150) and transposed to [B, 80, T'].
  * `DistributedSampler(shuffle=False)` (tasks/vocoder/vocoder_base.py:43-49): the index list is padded by wrap-around to a
    multiple of the world size and rank r takes r::world; every rank writes its own wavs, no collective.
  * `test_step` (modules/FastDiff/task/FastDiff.py:96-118): one `sampling_given_noise_schedule` call per batch, then per
    item `wav / wav.abs().max()` and `save_wav` = *32767 -> int16 (utils/audio.py:11-16) as `<item_name>_pred.wav`.
    The reference CLI runs B = 1 (config `max_sentences`); batching is this path's extension: the batch goes down with its
    `lens`, so every item is computed exactly as if it ran alone (and the padding costs nothing), then cropped to its length.

One job, three vocoders: synthesize, synthesize_griffin_lim and synthesize_pwg check their own arguments and hand _run_job a callable
(mels, frame counts, stream ids -> float waveform, hops per item); the job owns the score flags, the output rate, the selection
(_select: the one copy of "frames kept per item", also under collate_test_batch, synthesize_sharded and synthesize_long), the stream ids,
the micro-batches, the two legs across PCIe (pinned double buffers for synthesize, plain copies for the baselines), the level
epilogue, the scores and the delivery -- so the baselines' rows line up with the model's by construction.

Entry points: load_mel_inputs, load_wav_inputs (device resampler + mel front-end), trim_long_sil_wav (the reference's trim_long_sil on the
device), collate_test_batch, distributed_sampler_indices, synthesize,
synthesize_long (--long_form: windowed, any length, the utterances sharing window batches), synthesize_griffin_lim (--vocoder griffin_lim:
the baseline vocoder on the same items), synthesize_pwg (--vocoder pwg --pwg_dir DIR: the neural baseline on the same items), test_step
(the mirror of FastDiffTask.test_step itself), save_wavs and a small CLI
(`python -m fastdiff_amd.infer --test_input_dir D --out_dir O [--N 4] [--ckpt model.ckpt] [--from_wav] [--loud_norm] [--trim_long_sil [--trim_top_db 40] [--trim_mode long|edges]] [--out_sample_rate R]
[--loudness LUFS] [--stoi] [--pitch] [--spectral] [--mcd] [--vocoder griffin_lim [--gl_iters 60] [--gl_inversion pinv|nnls [--nnls_iters 128]]] [--vocoder pwg --pwg_dir DIR]
[--ndb_bins bins.npz]`).
"""
import argparse
import glob
import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _scores, schedules, shard
from .sampler import InferenceSchedule


def load_mel_inputs(test_input_dir: str) -> List[dict]:
    """[{item_name, mel: FloatTensor [T,80], len}] for every *.npy below the directory, in sorted path order."""
    items = []
    for path in sorted(glob.glob(f"{test_input_dir}/*.npy")):
        mel = torch.FloatTensor(np.load(path))
        if mel.dim() != 2:
            raise ValueError(f"{path}: expected a [T, n_mels] array, got shape {tuple(mel.shape)}")
        # the reference keeps the ".npy" suffix in the name (dataset_utils.py:200), so outputs are "<file>.npy_pred.wav"
        items.append({"item_name": path[len(test_input_dir) + 1:].replace("/", "_"), "mel": mel, "len": mel.shape[0]})
    return items


def pcm_to_float(pcm: np.ndarray, what: str = "wav") -> np.ndarray:
    """Samples of a RIFF file as float32 in [-1, 1), the way librosa.core.load (soundfile) hands them to process_utterance
    (data_gen/tts/data_gen_utils.py:100): every integer width is divided by its full scale (uint8 is offset binary, 24-bit PCM
    arrives from scipy left-aligned in int32), float files pass through.  Anything else is refused rather than guessed."""
    if pcm.dtype == np.uint8:
        return (pcm.astype(np.float32) - 128.0) / 128.0
    if pcm.dtype in (np.int16, np.int32):
        return pcm.astype(np.float32) / float(-int(np.iinfo(pcm.dtype).min))
    if pcm.dtype in (np.float32, np.float64):
        wav = pcm.astype(np.float32)
        if wav.size and float(np.abs(wav).max()) > 1.0 + 1e-6:
            raise ValueError(f"{what}: float samples outside [-1, 1] (peak {float(np.abs(wav).max()):.3g})")
        return wav
    raise ValueError(f"{what}: unsupported sample type {pcm.dtype}")


def wav_to_device(model, pcm: np.ndarray, sr: int, sample_rate: int = 22050, what: str = "wav") -> torch.Tensor:
    """The samples of a RIFF file ([n] or [n, C] as scipy.io.wavfile.read returns them, recorded at `sr`) as float32 mono at `sample_rate`
    on the device, [n'] -- librosa.core.load(path, sr=sample_rate).  Mono at the model's rate: pcm_to_float and an upload.  Anything
    else: the raw samples go up and FastDiff.resample converts, mixes down and resamples them there."""
    if sr == sample_rate and pcm.ndim == 1:
        return torch.from_numpy(pcm_to_float(pcm, what)).cuda()
    if pcm.ndim not in (1, 2) or (pcm.ndim == 2 and not 1 <= pcm.shape[1] <= 8):
        raise ValueError(f"{what}: expected [n] or [n, channels <= 8] samples, got shape {pcm.shape}")
    if pcm.dtype in (np.float32, np.float64):
        pcm = pcm_to_float(pcm, what)                      # float32, range checked
    elif pcm.dtype not in (np.uint8, np.int16, np.int32):
        raise ValueError(f"{what}: unsupported sample type {pcm.dtype}")
    if pcm.shape[0] < 1:
        raise ValueError(f"{what}: no samples")
    raw = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    return model.resample(raw, sr, sample_rate, channels=1 if pcm.ndim == 1 else pcm.shape[1])[0]


LOUD_NORM_LUFS = -22.0      # process_utterance(loud_norm=True): pyln.normalize.loudness(wav, loudness, -22.0) (data_gen_utils.py:118)


def loud_norm_wav(model, wav: torch.Tensor, sample_rate: int = 22050, what: str = "wav") -> torch.Tensor:
    """The loud_norm branch of process_utterance (data_gen/tts/data_gen_utils.py:115-120) on a device waveform [n]: normalised to
    -22 LUFS in float32, or divided by its new peak where that would exceed 1.  Shorter than one 400 ms block: ValueError, as
    pyloudnorm raises; nothing to measure (silence): left unchanged, with a warning."""
    from . import loudness as _loudness
    y, rec = model.loudness_normalize(wav, LOUD_NORM_LUFS, sample_rate=sample_rate, out="float", return_record=True)
    status = int(rec["status"][0])
    if status == _loudness.SHORT:
        raise ValueError(f"{what}: {wav.shape[-1]} samples at {sample_rate} Hz are shorter than one 400 ms block: loudness cannot be measured")
    if status == _loudness.SILENT:
        import warnings
        warnings.warn(f"{what}: no block passes the loudness gates (silence?): left as it is", stacklevel=2)
    return y


TRIM_NORM_LUFS = -20.0      # trim_long_silences(norm=True): pyln.normalize.loudness(wav_raw, loudness, -20.0) (data_gen_utils.py:45)


def trim_long_sil_wav(model, wav: torch.Tensor, sample_rate: int = 22050, what: str = "wav", norm: bool = True, top_db: float = 40.0,
                      mode: str = "long", return_record: bool = False):
    """The trim_long_sil branch of process_utterance (data_gen/tts/data_gen_utils.py:108-109 -> trim_long_silences, :27-90) on a device
    waveform [n]: with norm, first brought to -20 LUFS (or divided by its new peak where that would exceed 1, :42-47; shorter than one
    400 ms block: ValueError naming `what`, as loud_norm_wav raises), then the long silences cut (FastDiff.trim_silences: an energy
    detector in place of WebRTC's, the reference's smoothing and dilation).  Returns the device waveform cut to its n_out samples -- empty
    for a recording without a kept window, as the reference's wav_raw[audio_mask] is; with return_record also the record (a dict of
    scalars)."""
    from . import loudness as _loudness
    wav = wav.reshape(-1)
    if norm:
        wav, rec = model.loudness_normalize(wav, TRIM_NORM_LUFS, sample_rate=sample_rate, out="float", return_record=True)
        if int(rec["status"][0]) == _loudness.SHORT:
            raise ValueError(f"{what}: {wav.shape[-1]} samples at {sample_rate} Hz are shorter than one 400 ms block: loudness cannot be measured")
    out, _, rec = model.trim_silences(wav, sample_rate=sample_rate, top_db=top_db, mode=mode, return_record=True)
    rec = {k: v[0].item() for k, v in rec.items()}
    cut = out[0, :rec["n_out"]].contiguous()
    return (cut, rec) if return_record else cut


def write_trim_report(report, path: str) -> str:
    """The (item_name, samples in, record) rows of load_wav_inputs(trim_report=...) as <out_dir>/trim.tsv; returns the text."""
    from . import trim as _trim
    lines = ["\t".join(["name", "samples_in", "samples_out", "windows", "kept_windows", "peak_db", "status"])]
    for name, n_in, r in report:
        lines.append("\t".join([name, str(n_in), str(r["n_out"]), str(r["windows"]), str(r["kept_windows"]), format(r["peak_db"], ".2f"),
                                _trim.STATUS[r["status"]]]))
    text = "\n".join(lines)
    with open(path, "w") as f:
        f.write(text + "\n")
    return text


def load_wav_inputs(model, test_input_dir: str, sample_rate: int = 22050, mel_variant: str = "pwg", loud_norm: bool = False,
                    keep_wav: bool = False, trim_long_sil: bool = False, trim_top_db: float = 40.0, trim_mode: str = "long",
                    trim_report: list = None) -> List[dict]:
    """Copy-synthesis inputs (`test_input_dir` with recordings, tasks/vocoder/dataset_utils.py:162-184): every *.wav below the
    directory, in sorted order, through the device mel front-end (`FastDiff.mel_spectrogram` = process_utterance of
    data_gen/tts/data_gen_utils.py:93-147, or with mel_variant="tacotron" the TacotronSTFT of vocoder_binarizer_tacotron.py:110-116
    for models trained on FastDiff_tacotron.yaml features).  Integer PCM is scaled by its full range as librosa.core.load does
    (pcm_to_float).  A recording at another rate, or with several channels, first goes through the device resampler as the file holds
    it (FastDiff.resample: sample type, down-mix and rate in one launch -- librosa.core.load(path, sr=sample_rate),
    data_gen_utils.py:111); a mono recording at the model's rate takes the direct path, bit for bit as before.
    loud_norm: the reference's `loud_norm: true` configurations -- every recording is brought to -22 LUFS before its mel is taken
    (loud_norm_wav: FastDiff.loudness_normalize).
    trim_long_sil: the reference's `trim_long_sil: true` -- the long silences of every recording are cut before anything else sees it
    (trim_long_sil_wav, in front of loud_norm as in process_utterance): the mel, the vocoder and every score's reference get the trimmed
    recording.  A recording without a kept window is left out with a warning (the reference would hand an empty array on).  trim_report: a list that receives one
    (item_name, samples in, record) per recording.
    keep_wav: every item also carries "wav", its device waveform [n] at the model's rate as the mel was taken from it (what
    synthesize(stoi=True), synthesize(pitch=True) and synthesize(spectral=True) score the vocoded waveform against)."""
    from scipy.io import wavfile
    items = []
    for path in sorted(glob.glob(f"{test_input_dir}/*.wav")):
        sr, pcm = wavfile.read(path)
        wav = wav_to_device(model, pcm, sr, sample_rate, path)
        name = path[len(test_input_dir) + 1:].replace("/", "_")
        if trim_long_sil:
            n_in = wav.numel()
            wav, rec = trim_long_sil_wav(model, wav, sample_rate, path, top_db=trim_top_db, mode=trim_mode, return_record=True)
            if trim_report is not None:
                trim_report.append((name, n_in, rec))
            if rec["n_out"] == 0:
                import warnings
                warnings.warn(f"{path}: no window of the recording is kept (silence?): left out", stacklevel=2)
                continue
        if loud_norm:
            wav = loud_norm_wav(model, wav, sample_rate, path)
        mel = model.mel_spectrogram(wav, variant=mel_variant)[0].transpose(0, 1).contiguous().cpu()      # [T, 80] as on disk
        items.append({"item_name": name, "mel": mel, "len": mel.shape[0]})
        if keep_wav:
            items[-1]["wav"] = wav.reshape(-1)
    return items


def _select(items: Sequence[dict], drop_last_frame: bool):
    """The test-time collater's selection, the one copy of the rule: (mels, frames kept per item, item_names, positions in `items`) of
    the items that yield a hop.  With drop_last_frame every mel loses its last frame (dataset_utils.py:116-125), and a one-frame item
    is left out: the reference cannot collate it (dataset_utils.py:110 squeezes it away)."""
    mels, lens, names, where = [], [], [], []
    for i, it in enumerate(items):
        t = it["mel"].shape[0] - (1 if drop_last_frame else 0)
        if t >= 1:
            mels.append(it["mel"])
            lens.append(t)
            names.append(it["item_name"])
            where.append(i)
    return mels, lens, names, where


def _pad_on_host(mels, lens, out: "np.ndarray" = None) -> "np.ndarray":
    """[T, 80] mels, the first lens[b] frames of each -> the zero-padded [B, 80, max lens] batch, in `out` (flat float32) if given.
    The padding and the [T, 80] -> [80, T] transposition are plain numpy slice copies (torch's CPU kernels wake a whole OpenMP team
    for these few hundred KB, which on a 256-core host now and then costs tens of milliseconds)."""
    B, C, T = len(mels), mels[0].shape[1], max(lens)
    buf = np.empty(B * C * T, np.float32) if out is None else out[: B * C * T]
    batch = buf.reshape(B, C, T)
    for b, (c, t) in enumerate(zip(mels, lens)):
        a = c.numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        batch[b, :, :t] = a[:t].T
        batch[b, :, t:] = 0.0
    return batch


def collate_test_batch(items: Sequence[dict], drop_last_frame: bool = True, out: "np.ndarray" = None):
    """mels [B, 80, T'] zero-padded, lens [B] (frames kept per item), item_names -- the test-time collater (_select, _pad_on_host).
    `out`: optional flat float32 buffer (e.g. pinned memory) that receives the batch; the returned tensor is then a view of it."""
    mels, lens, names, _ = _select(items, drop_last_frame)
    return (torch.from_numpy(_pad_on_host(mels, lens, out)), lens, names) if mels else (None, [], [])


def distributed_sampler_indices(n_items: int, rank: int, world_size: int) -> List[int]:
    """Indices torch's DistributedSampler(shuffle=False, drop_last=False) hands to `rank`."""
    if n_items == 0:
        return []
    total = -(-n_items // world_size) * world_size
    idx = list(range(n_items))
    while len(idx) < total:                   # padded by repeating from the start (possibly several times)
        idx += idx[: total - len(idx)]
    return idx[rank:total:world_size]


def _job_cache(model) -> dict:
    """Per-model cache of what a synthesis job needs besides the weights: the step table of each schedule (host arithmetic that
    depends on the schedule only: ~6 ms for N = 6) and the pinned staging buffers (a pinned allocation costs more than vocoding a
    micro-batch).  Lives on the module, so it is released with it."""
    cache = getattr(model, "_infer_cache", None)
    if cache is None:
        cache = {"rows": {}, "pin": None}
        try:
            model._infer_cache = cache
        except AttributeError:          # a stand-in without attributes (tests): no caching
            pass
    return cache


def _step_rows(model, n_steps, noise_schedule, diffusion_hyperparams):
    if diffusion_hyperparams is not None:          # caller-owned tables: derived as given, not cached
        if noise_schedule is None:
            noise_schedule = schedules.noise_schedule_for(n_steps)
        return InferenceSchedule(diffusion_hyperparams, noise_schedule, verbose=False).rows()
    if noise_schedule is None:
        noise_schedule = schedules.noise_schedule_for(n_steps)
    key = tuple(float(v) for v in torch.as_tensor(noise_schedule).reshape(-1).tolist())
    rows_of = _job_cache(model)["rows"]
    if key not in rows_of:
        rows_of[key] = InferenceSchedule(schedules.training_hyperparams(), noise_schedule, verbose=False).rows()
    return rows_of[key]


def _pinned_staging(model, n_mel: int, n_pcm: int):
    """Two mel and two PCM pinned buffers of at least the given element counts, kept on the model between jobs."""
    cache = _job_cache(model)
    pin = cache["pin"]
    if pin is None or pin[0][0].numel() < n_mel or pin[1][0].numel() < n_pcm:
        n_mel = max(n_mel, pin[0][0].numel() if pin else 0)
        n_pcm = max(n_pcm, pin[1][0].numel() if pin else 0)
        pin = ([torch.empty(n_mel, dtype=torch.float32).pin_memory() for _ in range(2)],
               [torch.empty(n_pcm, dtype=torch.int16).pin_memory() for _ in range(2)])
        cache["pin"] = pin
    return pin


def _pad_on_device(mels, lens) -> torch.Tensor:
    """_pad_on_host for mels that already live on the GPU (the RCCL scatter of synthesize_sharded delivers them there): the same
    padded [B, 80, max lens] batch, built with device copies -- no round trip over PCIe."""
    batch = torch.zeros(len(mels), mels[0].shape[1], max(lens), dtype=torch.float32, device=mels[0].device)
    for b, (c, t) in enumerate(zip(mels, lens)):
        batch[b, :, :t] = c[:t].transpose(0, 1)
    return batch


def _level_epilogue(model, out_sample_rate, sample_rate, loudness):
    """(n_of, epilogue) of a synthesis job: n_of(t) = the PCM samples of t hops (at R = out_sample_rate where that is another rate than
    `sample_rate`); epilogue(wav, lens) = the float waveforms of a micro-batch (item b: lens[b] hops) -> int16 PCM [B, n]: resampled to
    R first, then peak-normalised, or with loudness = LUFS loudness-normalised, each item over its own samples."""
    from . import resample as _resample
    hop = model.hop_length
    R = None if out_sample_rate is None or int(out_sample_rate) == int(sample_rate) else int(out_sample_rate)
    n_of = (lambda t: t * hop) if R is None else (lambda t: _resample.out_len(t * hop, sample_rate, R))      # PCM samples of t frames

    def to_pcm(wav, valid, rate):
        if loudness is None:
            return model.peak_normalize_int16(wav, valid=valid)
        return model.loudness_normalize(wav.reshape(wav.shape[0], -1), float(loudness), valid=valid, sample_rate=rate, out="int16")

    def epilogue(wav, lens):
        if R is None:
            return to_pcm(wav, [t * hop for t in lens], sample_rate)
        y = model.resample(wav.reshape(wav.shape[0], -1), sample_rate, R, valid=[t * hop for t in lens])
        return to_pcm(y, [n_of(t) for t in lens], R)

    return n_of, epilogue


def _scorer(model, items, scored, report, sample_rate, who):
    """score(wav, names, lens) of a synthesis job: every enabled score of the micro-batch's float waveforms against
    the items' recordings, cut to the vocoded length (lens hops), into report[name]."""
    hop = model.hop_length

    def score(wav, names, lens):
        # the recordings of the micro-batch next to its float waveform: one padded batch, one call and one record read per score
        wav_of = {it["item_name"]: it["wav"] for it in items}
        B, n = wav.shape[0], wav.shape[-1]
        clean = torch.zeros((B, n), device=wav.device, dtype=torch.float32)
        for b, (name, t) in enumerate(zip(names, lens)):
            if wav_of[name].numel() < t * hop:
                raise ValueError(f"{who}: the recording of {name} has {wav_of[name].numel()} samples, fewer than the {t * hop} vocoded")
            clean[b, : t * hop] = wav_of[name][: t * hop]
        valid = [t * hop for t in lens]
        for sc in scored:
            rec = getattr(model, sc.name)(clean, wav.reshape(B, n), valid=valid, **sc.kwargs(sample_rate, hop))
            for b, name in enumerate(names):
                report.setdefault(name, {}).update({key: float(rec[col][b]) for col, key, _, _ in sc.columns})
                report[name][sc.status_key] = sc.module.STATUS[int(rec["status"][b])]

    return score


def _run_job(who, model, items, vocode, max_batch, sort, drop_last_frame, out_sample_rate, sample_rate, loudness, scores,
             all_frames_in=False, pinned=False, return_device=False):
    """The synthesis job of synthesize, synthesize_griffin_lim and synthesize_pwg (`who`: the one named in a refusal): item_name -> int16
    PCM, with scores=dict(stoi=, pitch=, spectral=, mcd=) enabled (pcm, report).  The items that yield a hop (_select) go longest first
    (sort) into padded micro-batches; each is collated where its mels live, vocoded, taken through the level epilogue and the scores,
    and unpacked to n_of(hops) samples per item.  An item's noise-stream id is its "uid", by default its position in `items`.
    vocode(mels [B, 80, T'] on the device, frames [B], stream_ids [B]) is the only per-vocoder part: it returns (float waveform, hops
    per item) -- all_frames_in: it is given every frame of a mel and returns one hop less, as the selection counts them -- and may add
    settle(), which is True when the call has been run again since (FastDiff's option fallback = "host"): the epilogue and the scores
    of that micro-batch are then redone, when the batch is collected on the host or, with return_device, one batch late.
    pinned: the two legs across PCIe go through pinned double buffers (_pinned_staging) -- the collater writes into one, one
    asynchronous copy per micro-batch each way, and the previous batch is unpacked on the host while this one runs; otherwise
    mels.cuda() and pcm.cpu().  return_device: the values are int16 device tensors, nothing comes back."""
    scored = _scores.enabled(**scores)
    if scored and not all(isinstance(it.get("wav"), torch.Tensor) and it["wav"].is_cuda for it in items):
        raise ValueError(f"{who}: {scored[0].name}=True needs items that carry their device waveform as 'wav' (load_wav_inputs(keep_wav=True))")
    report: Dict[str, dict] = {}
    out: Dict[str, np.ndarray] = {}
    job_mels, frames, job_names, picked = _select(items, drop_last_frame)
    if not picked:
        return (out, report) if scored else out
    n_of, epilogue = _level_epilogue(model, out_sample_rate, sample_rate, loudness)
    score = _scorer(model, items, scored, report, sample_rate, who)
    uids = [int(items[i].get("uid", i)) for i in picked]
    if all_frames_in:
        frames = [t + 1 for t in frames]           # selected by its hops, collated with every frame
    on_device = isinstance(job_mels[0], torch.Tensor) and job_mels[0].is_cuda
    # pinned staging, two mel and two PCM buffers used alternately -- buffer k & 1 is free again once micro-batch k - 2 has been
    # collected, which happens in iteration k - 1.  Only the legs that cross PCIe need it.
    if pinned and not (on_device and return_device):
        t_max, b_max = max(frames), min(max_batch, len(picked))
        mel_pin, pcm_pin = _pinned_staging(model, 0 if on_device else b_max * job_mels[0].shape[1] * t_max, 0 if return_device else b_max * n_of(t_max))
        mel_np = [m.numpy() for m in mel_pin]      # the collater writes the batch straight into the pinned buffer
    mel_up = [None, None]          # event behind the upload that last read mel_pin[i]: the collater waits for it before writing there again
    pending = None                 # pinned: the micro-batch still on its way to the host, as collect() takes it
    unsettled = None               # return_device: (settle, wav, names, lens) of the micro-batch nobody has settled yet

    def finish(wav, names, lens):
        pcm = epilogue(wav, lens)
        if scored:
            score(wav, names, lens)
        return pcm

    def collect(done, host, names, lens, wav, settle):
        if done is not None:
            done.synchronize()
        if settle is not None and settle():      # an operand left the fp16 range: the call was run again on fp32 -- so is its epilogue
            host.copy_(finish(wav, names, lens), non_blocking=True)
            torch.cuda.current_stream().synchronize()
        rows = host.numpy()
        for b, (name, t) in enumerate(zip(names, lens)):
            out[name] = rows[b, : n_of(t)].copy()

    def keep_on_device(pcm, names, lens):
        for b, (name, t) in enumerate(zip(names, lens)):
            out[name] = pcm[b, : n_of(t)]

    def resettle(p):
        if p is not None and p[0]():             # run again on fp32: so is its epilogue
            keep_on_device(finish(*p[1:]), *p[2:])

    # (the frames kept are the full counts or one less for every item, so longest first is the order of the full counts)
    for k, idx in enumerate(shard.micro_batches(range(len(picked)), frames, max_batch, sort=sort)):
        mels, lens, names = [job_mels[i] for i in idx], [frames[i] for i in idx], [job_names[i] for i in idx]
        if on_device:
            mels = _pad_on_device(mels, lens)
        elif pinned:
            if mel_up[k & 1] is not None:            # the upload of micro-batch k - 2 read this pinned buffer
                mel_up[k & 1].synchronize()
            batch = _pad_on_host(mels, lens, out=mel_np[k & 1])
            mels = mel_pin[k & 1][: batch.size].view(batch.shape).cuda(non_blocking=True)
            mel_up[k & 1] = torch.cuda.Event()
            mel_up[k & 1].record()
        else:
            mels = torch.from_numpy(_pad_on_host(mels, lens)).cuda()
        with torch.no_grad():
            wav, lens, *settle = vocode(mels, lens, [uids[i] for i in idx])
        settle = settle[0] if settle else None
        # one epilogue call and one asynchronous copy per micro-batch; the previous batch is unpacked on the host while this one runs
        pcm = finish(wav, names, lens)
        if return_device:
            keep_on_device(pcm, names, lens)
            # the library remembers a bounded number of redone tickets (fd_sample_settle), so a micro-batch is settled as soon as the
            # next call has looked at it (no wait by then) and not at the end of the job
            resettle(unsettled)
            unsettled = (settle, wav, names, lens) if settle is not None else None
        elif pinned:
            host = pcm_pin[k & 1][: pcm.numel()].view(pcm.shape)
            host.copy_(pcm, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            if pending is not None:
                collect(*pending)
            pending = (done, host, names, lens, wav, settle)
        else:
            collect(None, pcm.cpu(), names, lens, wav, settle)
    if pending is not None:
        collect(*pending)
    resettle(unsettled)
    return (out, report) if scored else out


def synthesize(model, items: Sequence[dict], n_steps: int = 4, max_batch: int = 8, seed: int = 0, drop_last_frame: bool = True,
               noise_schedule=None, diffusion_hyperparams=None, return_device: bool = False, sort: bool = True, out_sample_rate: int = None,
               sample_rate: int = 22050, loudness: float = None, stoi: bool = False, pitch: bool = False,
               spectral: bool = False, mcd: bool = False) -> Dict[str, np.ndarray]:
    """item_name -> int16 PCM of its own length (hop 256 x frames), through length-sorted padded micro-batches.
    Noise: utterance `it` draws x_T and z from Philox stream (seed, it["uid"]) over its own samples (fd_set_noise_streams); "uid"
    defaults to the item's position in `items`, callers that shard a job put the utterance's index in the WHOLE job there, so a
    waveform does not depend on the micro-batch, rank or world size that produced it.
    Mels may live on the host ([T, 80] tensors or arrays: collated in numpy straight into pinned memory) or on the GPU (collated
    there).  return_device: the values are int16 device tensors instead of host arrays (no device-to-host copy at all: what
    synthesize_sharded hands to the RCCL gather).  sort=False: micro-batches in the order of arrival instead of longest first.
    out_sample_rate = R (None: the model's `sample_rate`, every byte as without the argument): the float waveform of each micro-batch is
    resampled on the device (FastDiff.resample, ragged: valid = lens * hop) and THEN peak-normalised over its out_len(lens * hop) samples,
    so the filter's overshoot cannot clip; an item's PCM is what it would get alone.
    loudness = LUFS (None: peak normalisation, every byte as without the argument): the loudness epilogue instead of the peak epilogue
    (FastDiff.loudness_normalize, out="int16"): every utterance is measured as it is delivered -- after the resampling, at that rate,
    over its own samples -- and scaled to that BS.1770 loudness; one that cannot be measured, or that the gain would clip, is
    peak-normalised as before.
    stoi=True (copy synthesis: every item carries "wav", its recording on the device at `sample_rate`, load_wav_inputs(keep_wav=True)):
    returns (pcm, report) with report[name] = {"stoi", "estoi", "status"} (FastDiff.stoi; status by name, the values NaN unless "OK"),
    measured on the float waveform of each micro-batch before the level epilogue and before any out_sample_rate, the recording cut to
    the vocoded length (lens * hop).
    pitch=True (copy synthesis, items as for stoi=True): returns (pcm, report) with report[name] = {"f0_rmse_cents", "gpe", "vde",
    "pitch_status"} (FastDiff.pitch at `sample_rate`, one F0 per mel frame; status by name), measured on the same waveforms as STOI.
    With stoi=True as well, report[name] holds both sets of keys.
    spectral=True (copy synthesis, items as for stoi=True): returns (pcm, report) with report[name] = {"mr_sc", "mr_logmag", "lsd_db",
    "spectral_status"} (FastDiff.spectral at the default resolutions: the means over them of the spectral convergence, the log-magnitude
    distance in nepers and the log-spectral distance in dB; status by name), measured on the same waveforms, next to the other sets.
    mcd=True (copy synthesis, items as for stoi=True): returns (pcm, report) with report[name] = {"mcd_dtw", "mcd_linear", "mcd_status"}
    (FastDiff.mcd with 13 coefficients of the pwg front-end: the mel-cepstral distortion in dB along the time-warped path and frame by
    frame; status by name), measured on the same waveforms, next to the other sets."""
    # the step table depends on the schedule only: derived once per schedule and model (sampling_given_noise_schedule derives it on
    # every call, as the reference does), the same rows then drive every micro-batch
    rows = _step_rows(model, n_steps, noise_schedule, diffusion_hyperparams)
    # library option fallback = "host": the range check of a sample call is looked at by the NEXT call, after that one has enqueued
    # itself (FastDiff.settle); until then the waveform and everything computed from it is provisional
    host_check = getattr(model, "_options", {}).get("fallback") == "host"

    def vocode(mels, lens, stream_ids):
        wav = model.sample(mels, rows, ddim=False, seed=seed, lens=lens, stream_ids=stream_ids, defer_check=host_check)
        ticket = getattr(model, "last_ticket", 0)
        return (wav, lens, lambda: model.settle(ticket)) if host_check else (wav, lens)

    return _run_job("synthesize", model, items, vocode, max_batch, sort, drop_last_frame, out_sample_rate, sample_rate, loudness,
                    dict(stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd), pinned=True, return_device=return_device)


def synthesize_griffin_lim(model, items: Sequence[dict], n_iters: int = 60, max_batch: int = 8, seed: int = 0, variant: str = "pwg",
                           sort: bool = True, out_sample_rate: int = None, sample_rate: int = 22050, loudness: float = None,
                           stoi: bool = False, pitch: bool = False, spectral: bool = False, inversion: str = "pinv",
                           mcd: bool = False,
                           nnls_iters: int = 128) -> Dict[str, np.ndarray]:
    """The baseline next to synthesize(): item_name -> int16 PCM from Griffin-Lim on the device (FastDiff.griffin_lim_mel: the mel
    inverted with the front-end's filter bank -- inversion="pinv", the default: its pseudo-inverse; inversion="nnls": the non-negative
    least squares of the reference's GLMel, vocoders/gl_mel.py, in nnls_iters steps -- then n_iters projections), through the same
    length-sorted padded micro-batches.  ALL frames of an item's mel are used: its
    `len` frames give 256 (len - 1) samples, exactly what synthesize() produces from the same item after dropping the last frame, so
    the two waveforms and their scores line up.  An item of fewer than 2 frames is left out, as synthesize() leaves out what it cannot
    collate.  The starting phase of item `it` is drawn from Philox stream (seed, it["uid"], frame, bin); "uid" defaults to the item's
    position in `items`, so a waveform does not depend on its micro-batch.  variant: the front-end the mels come from ("pwg": log10,
    "tacotron": ln).  out_sample_rate, loudness, stoi, pitch, spectral, mcd: as in synthesize() -- the same level epilogue, the same scores
    into the same report keys, measured on the float waveform before the epilogue."""
    if inversion not in ("pinv", "nnls"):
        raise ValueError(f"synthesize_griffin_lim: inversion must be 'pinv' or 'nnls', got {inversion!r}")
    how = {} if inversion == "pinv" else dict(inversion=inversion, nnls_iters=int(nnls_iters))      # (the default passes no new keyword)

    def vocode(mels, frames, stream_ids):              # all frames in, in hops: 256 (frames - 1) samples out
        wav = model.griffin_lim_mel(mels, lens=frames, variant=variant, n_iters=n_iters, seed=seed, stream_ids=stream_ids, **how)
        return wav, [f - 1 for f in frames]

    return _run_job("synthesize_griffin_lim", model, items, vocode, max_batch, sort, drop_last_frame=True, all_frames_in=True,
                    out_sample_rate=out_sample_rate, sample_rate=sample_rate, loudness=loudness,
                    scores=dict(stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd))


def synthesize_pwg(model, pwg, items: Sequence[dict], max_batch: int = 8, seed: int = 0, drop_last_frame: bool = True, sort: bool = True,
                   out_sample_rate: int = None, sample_rate: int = 22050, loudness: float = None, stoi: bool = False, pitch: bool = False,
                   spectral: bool = False, mcd: bool = False) -> Dict[str, np.ndarray]:
    """The neural baseline next to synthesize(): item_name -> int16 PCM from Parallel WaveGAN on the device (`pwg`: a loaded
    fastdiff_amd.pwg.ParallelWaveGAN; its spec2wav applies the scaler and the edge padding, as the reference's vocoders/pwg.py), through
    the same length-sorted padded micro-batches.  As in synthesize() the last frame of a mel is dropped, so the two waveforms and their
    scores line up.  The network is convolutional and takes any length up to FD_PWG_MAX_FRAMES: there is no windowed variant.  z of
    item `it` is drawn from Philox stream (seed, it["uid"], sample); "uid" defaults to the item's position in `items`, so a waveform does
    not depend on its micro-batch.  `model` (a FastDiff) supplies the level epilogue and the scores: out_sample_rate, loudness, stoi,
    pitch, spectral, mcd as in synthesize() -- the same report keys, measured on the float waveform before the epilogue."""
    if pwg.hop_size != model.hop_length:
        raise ValueError(f"synthesize_pwg: the generator's hop {pwg.hop_size} is not the {model.hop_length} samples of the mels' frames")
    return _run_job("synthesize_pwg", model, items, lambda mels, lens, stream_ids: (pwg.spec2wav(mels, lens=lens, seed=seed, stream_ids=stream_ids), lens),
                    max_batch, sort, drop_last_frame, out_sample_rate, sample_rate, loudness, dict(stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd))


def synthesize_sharded(model, items, n_steps: int = 4, max_batch: int = 8, seed: int = 0, drop_last_frame: bool = True, src: int = 0,
                       device=None, force_collectives: int = 0, gather: str = "src", balance: str = "time", out_sample_rate: int = None,
                       sample_rate: int = 22050, loudness: float = None, stoi: bool = False, pitch: bool = False,
                       spectral: bool = False, mcd: bool = False) -> Dict[str, np.ndarray]:
    """BASELINE config 4 as north_star words it: rank `src` holds all utterances (items; None elsewhere) -> length-balanced
    partition (shard.partition_utterances) -> scatter of the mels -> every rank vocodes its share in padded micro-batches on its
    own GPU -> gather of the int16 PCM on `src`, which returns item_name -> PCM (the other ranks return {}).  The process group
    must be initialised; `device` is where the messages are staged (the GPU for RCCL, None = host for gloo).  Without a process
    group (one process) this is synthesize().
    With `device` set the data crosses PCIe exactly twice: the mels go up once on `src` (inside the scatter), the scattered mels are
    collated on the GPU they arrive on, the PCM stays on the device through the gather, and `src` brings the whole job back with ONE
    device-to-host copy.
    force_collectives = R > 1 in a process group of ONE rank (a box with a single GPU): the job still takes the multi-rank route --
    the broadcast of names / ids / lengths, a partition into R parts, and parts 1 .. R-1 scattered and gathered as packed messages
    from this rank to itself through the backend (shard loopback) -- so every line a real peer would execute runs on RCCL too.
    gather = "none": the job ends the way the reference's does (FastDiff.py:107-118: every rank writes the wavs of its own
    utterances, nothing is collected): each rank returns item_name -> PCM of ITS share, brought to its own host behind its own
    micro-batches; no message travels back and `src` does no work the other ranks do not do.
    balance = "time" (default): the partition weighs an utterance as frames + a per-utterance constant (shard.utterance_cost);
    "frames": by frames alone (rounds 1-5).
    out_sample_rate, loudness: as in synthesize() -- every rank resamples and normalises its own share, the gathered PCM is at that rate.
    stoi=True, pitch=True, spectral=True and mcd=True are refused: the recordings are not scattered (score with synthesize(stoi=True,
    pitch=True, spectral=True, mcd=True))."""
    _scores.refuse("synthesize_sharded", " (the recordings are not scattered): use synthesize({name}=True)", stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd)
    if gather not in ("src", "none"):
        raise ValueError(f"synthesize_sharded: gather must be 'src' or 'none', got {gather!r}")
    if balance not in ("time", "frames"):
        raise ValueError(f"synthesize_sharded: balance must be 'time' or 'frames', got {balance!r}")
    import torch.distributed as dist
    loop = int(force_collectives) if (dist.is_available() and dist.is_initialized() and dist.get_world_size() == 1) else 0
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and loop < 2):
        return synthesize(model, items, n_steps, max_batch, seed, drop_last_frame, out_sample_rate=out_sample_rate, sample_rate=sample_rate, loudness=loudness)
    rank, world = dist.get_rank(), dist.get_world_size()
    meta = [None]
    if rank == src:      # the collater's view of every item: the on-disk [T', 80] rows with the last frame dropped (a view: no copy, no
        mels, lens, names, kept = _select(items, drop_last_frame)                                             # transposition on the host)
        mels = [m[:t] for m, t in zip(mels, lens)]
        meta = [(names, [int(items[i].get("uid", i)) for i in kept], lens)]
    dist.broadcast_object_list(meta, src=src)          # names, noise-stream ids and lengths in one message
    names, uids, lens = meta[0]
    parts = shard.partition_utterances(lens, loop or world, cost="time" if balance == "time" else None)
    mine, _ = shard.scatter_utterances(mels if rank == src else None, parts, src=src, device=device, lens=lens, frames_first=True, loopback=bool(loop))
    on_gpu = device is not None and torch.device(device).type == "cuda"
    local = [{"item_name": str(i), "mel": m, "len": m.shape[0], "uid": uids[i]} for i, m in mine]
    if gather == "none":      # the reference's own ending: this rank's waveforms on this rank's host, nothing sent back
        pcm = synthesize(model, local, n_steps, max_batch, seed, drop_last_frame=False, out_sample_rate=out_sample_rate, sample_rate=sample_rate, loudness=loudness)
        return {names[i]: pcm[str(i)] for i, _ in mine}
    pcm = synthesize(model, local, n_steps, max_batch, seed, drop_last_frame=False, return_device=on_gpu, out_sample_rate=out_sample_rate,
                     sample_rate=sample_rate, loudness=loudness)
    wavs = [(i, pcm[str(i)] if on_gpu else torch.from_numpy(pcm[str(i)])) for i, _ in mine]
    # the gather sizes its messages as lens * hop: hand it the sample counts the epilogue delivered, with a hop of 1
    n_of = _level_epilogue(model, out_sample_rate, sample_rate, loudness)[0]
    out = shard.gather_waveforms(wavs, [n_of(t) for t in lens], parts, hop=1, dst=src, device=device, dtype=torch.int16, loopback=bool(loop))
    if rank != src:
        return {}
    if not on_gpu:
        return {names[i]: out[i].numpy() for i in range(len(names))}
    sizes = [int(o.numel()) for o in out]
    # one device-to-host copy for the whole job, into pageable memory the caller owns (through a pinned buffer it measured 9 ms for
    # the 27 MB of BASELINE config 4 against 1 ms: reading pinned memory back on the host is slow)
    flat = torch.cat([o.reshape(-1) for o in out]).cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return {names[i]: flat[offs[i]: offs[i + 1]] for i in range(len(names))}


def test_step(model, sample: dict, hparams: dict, diffusion_hyperparams=None, gen_dir: str = None, noise_source: str = "device",
              seed=None) -> Dict[str, np.ndarray]:
    """`FastDiffTask.test_step(sample, batch_idx)` (modules/FastDiff/task/FastDiff.py:60-119) around the HIP sampler, statement for
    statement: the schedule is hparams['noise_schedule'] when set (a list becomes a FloatTensor, :65-68), else picked by
    hparams['N'] (:70-93: 1000 / 200 linspaces, the literal lists for 8 / 6 / 4 / 3, a missing N -> 4 with the reference's message,
    anything else NotImplementedError); ONE sampling_given_noise_schedule call of size (1, 1, T * hop_size) on sample['mels'] (:98-103);
    every predicted waveform divided by its own peak (:110,115) and written through save_wav = * 32767 -> int16 (utils/audio.py:11-16)
    as `<gen_dir>/<item_name>_pred.wav`; with ground-truth waveforms in sample['wavs'] also `<item_name>_gt.wav`, normalised the same
    way (:113-117).  Returns item_name -> int16 PCM of the prediction.
    sample: {"mels": [1, 80, T] tensor, "wavs": [] or [1, 1, L] tensor, "item_name": [name]}, as the test-time collater builds it
    (collate_test_batch; the reference CLI runs max_sentences = 1, base.yaml:53, and the size above is only valid for one item).
    gen_dir: where the files go (the reference derives it from work_dir / global_step / gen_dir_name, :104; None = write nothing).
    noise_source "device" (Philox on the GPU, `seed`) or "reference" (std_normal on the CPU generator in the reference's order: a
    seeded run then draws the reference's random stream)."""
    from . import sampler
    mels, y = sample["mels"], sample["wavs"]
    schedule = schedules.noise_schedule_for(hparams.get("N"), hparams.get("noise_schedule", ""))
    if isinstance(schedule, list):
        schedule = torch.FloatTensor(schedule)
    if diffusion_hyperparams is None:
        diffusion_hyperparams = schedules.training_hyperparams()
    audio_length = mels.shape[-1] * hparams["hop_size"]
    y_ = sampler.sampling_given_noise_schedule(model, (1, 1, audio_length), diffusion_hyperparams, schedule, condition=mels.cuda(), ddim=False,
                                               return_sequence=False, noise_source=noise_source, seed=seed)
    if gen_dir is not None:
        os.makedirs(gen_dir, exist_ok=True)
    out: Dict[str, np.ndarray] = {}
    pcm = model.peak_normalize_int16(y_).cpu().numpy()            # wav_pred / wav_pred.abs().max(), then save_wav's * 32767 -> int16
    gts = y if len(y) else [None] * len(sample["item_name"])
    for idx, (wav_gt, item_name) in enumerate(zip(gts, sample["item_name"])):
        out[item_name] = pcm[idx].reshape(-1)
        if gen_dir is None:
            continue
        from scipy.io import wavfile
        if wav_gt is not None:
            gt = model.peak_normalize_int16(wav_gt.reshape(1, 1, -1).cuda().float()).cpu().numpy().reshape(-1)
            wavfile.write(f"{gen_dir}/{item_name}_gt.wav", hparams["audio_sample_rate"], gt)
        wavfile.write(f"{gen_dir}/{item_name}_pred.wav", hparams["audio_sample_rate"], out[item_name])
    return out


LONG_FORM_GROUP_FRAMES = 1 << 16      # mel frames per sample_long_batch call: 64 MiB of float32 output (an utterance longer than that goes alone)


def synthesize_long(model, items: Sequence[dict], n_steps: int = 4, seed: int = 0, drop_last_frame: bool = True, noise_schedule=None,
                    diffusion_hyperparams=None, window_frames=None, group_frames: int = LONG_FORM_GROUP_FRAMES, loudness: float = None,
                    sample_rate: int = 22050, stoi: bool = False, pitch: bool = False, spectral: bool = False,
                    mcd: bool = False) -> Dict[str, np.ndarray]:
    """item_name -> int16 PCM through FastDiff.sample_long_batch (windowed: any length, device memory of one window batch): the
    utterances are taken in order in groups of up to group_frames mel frames, so their outputs fit, and the windows of a group share the
    sampler's batches.  Utterance `it` draws its noise from Philox stream (seed, it["uid"]) as in synthesize(), so the PCM is the same,
    byte for byte; peak normalisation runs on each whole utterance afterwards (FastDiff.py:110) -- or, with loudness = LUFS, the
    loudness epilogue as in synthesize(): the filter runs over the whole utterance in tiles, however long it is.
    stoi=True, pitch=True, spectral=True and mcd=True are refused (score the result with FastDiff.stoi, FastDiff.pitch, FastDiff.spectral and FastDiff.mcd, which
    take any length)."""
    _scores.refuse("synthesize_long", ": score the waveforms with FastDiff.{name}", stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd)
    rows = _step_rows(model, n_steps, noise_schedule, diffusion_hyperparams)
    hop = model.hop_length
    out: Dict[str, np.ndarray] = {}
    group, frames = [], 0

    def run():
        with torch.no_grad():
            wavs = model.sample_long_batch([m for _, _, m in group], rows, ddim=False, seed=seed, stream_ids=[u for _, u, _ in group],
                                           window_frames=window_frames)
        for (name, _, m), wav in zip(group, wavs):
            if loudness is None:
                pcm = model.peak_normalize_int16(wav)
            else:
                pcm = model.loudness_normalize(wav.reshape(1, -1), float(loudness), sample_rate=sample_rate, out="int16")
            out[name] = pcm[0, : m.shape[-1] * hop].cpu().numpy()

    for c, t, name, i in zip(*_select(items, drop_last_frame)):
        if group and frames + t > group_frames:
            run()
            group, frames = [], 0
        group.append((name, int(items[i].get("uid", i)), torch.as_tensor(c)[:t].to(device="cuda", dtype=torch.float32).transpose(0, 1).contiguous()))
        frames += t
    if group:
        run()
    return out


def save_wavs(pcm: Dict[str, np.ndarray], out_dir: str, sample_rate: int = 22050) -> List[str]:
    from scipy.io import wavfile
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, data in pcm.items():
        path = os.path.join(out_dir, f"{name}_pred.wav")
        wavfile.write(path, sample_rate, data)
        paths.append(path)
    return paths


def _write_table(rows, out_dir: str, stem: str, rank: int = 0, world: int = 1) -> str:
    """Prints a table (rows of cells, the header first) tab-separated and writes it as <out_dir>/<stem>.tsv, one process per job, or as
    <stem>.rank<r>.tsv where several ranks each write their own; returns the text."""
    text = "\n".join("\t".join(row) for row in rows)
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{stem}.tsv" if world == 1 else f"{stem}.rank{rank}.tsv"), "w") as f:
        f.write(text + "\n")
    return text


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--test_input_dir", required=True, help="directory of [T,80] .npy mels, or of .wav recordings with --from_wav")
    ap.add_argument("--from_wav", action="store_true", help="inputs are recordings: compute the mels on the device first")
    ap.add_argument("--mel_variant", default="pwg", choices=("pwg", "tacotron"), help="front-end for --from_wav (base.yaml / FastDiff_tacotron.yaml features)")
    ap.add_argument("--mel_basis", default=None, metavar="FILE.npy",
                    help="with --from_wav: an [80, 513] float32 filter bank to use instead of the library's restated default, e.g. saved "
                         "from librosa.filters.mel(sr=22050, n_fft=1024, n_mels=80, fmin=80, fmax=7600) (data_gen_utils.py:122-134)")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--N", type=int, default=4, help="reverse steps: 3, 4, 6, 8, 200 or 1000 (FastDiff.py:76-93)")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (state_dict under ['state_dict']['model'])")
    ap.add_argument("--max_batch", type=int, default=16, help="utterances per padded micro-batch (16: 6 % faster than 8 on a 64-utterance job)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out_sample_rate", type=int, default=None, metavar="R",
                    help="write the wavs at R Hz (e.g. 16000, 24000, 44100, 48000) instead of the model's 22050: resampled on the device, then normalised")
    ap.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                    help="normalise every wav to this BS.1770 integrated loudness (e.g. -23) on the device instead of to its peak; an utterance "
                         "too short or too quiet to measure, or that the gain would clip, is peak-normalised")
    ap.add_argument("--loud_norm", action="store_true",
                    help="with --from_wav: bring every recording to -22 LUFS before its mel is taken (the reference's loud_norm: true)")
    ap.add_argument("--stoi", action="store_true",
                    help="with --from_wav (copy synthesis): score every vocoded waveform against its recording with STOI and ESTOI on the "
                         "device, print the table and write <out_dir>/stoi.tsv")
    ap.add_argument("--pitch", action="store_true",
                    help="with --from_wav (copy synthesis): track F0 of every recording and vocoded waveform with YIN on the device and score "
                         "the pitch (F0 RMSE in cents, gross pitch error, voicing decision error), print the table and write <out_dir>/pitch.tsv")
    ap.add_argument("--spectral", action="store_true",
                    help="with --from_wav (copy synthesis): measure the multi-resolution STFT distances of every vocoded waveform against its "
                         "recording on the device (spectral convergence, log-magnitude distance, log-spectral distance in dB; the means over "
                         "512 / 1024 / 2048-point transforms), print the table and write <out_dir>/spectral.tsv")
    ap.add_argument("--mcd", action="store_true",
                    help="with --from_wav (copy synthesis): measure the mel-cepstral distortion of every vocoded waveform against its recording "
                         "on the device (13 mel-filter-bank cepstral coefficients; in dB along the time-warped path and frame by frame), print "
                         "the table and write <out_dir>/mcd.tsv")
    ap.add_argument("--vocoder", default="fastdiff", choices=("fastdiff", "griffin_lim", "pwg"),
                    help="pwg: the neural baseline instead of the model -- Parallel WaveGAN on the device from --pwg_dir; griffin_lim: the baseline instead of the model -- every mel inverted with the filter bank (--gl_inversion) and "
                         "run through --gl_iters Griffin-Lim iterations on the device; the same <name>_pred.wav files and, with --stoi / "
                         "--pitch / --spectral / --mcd, the same TSVs, so a baseline row is one command next to the model's")
    ap.add_argument("--pwg_dir", default=None, metavar="DIR",
                    help="with --vocoder pwg: the directory of the generator (config.yaml, the newest model_ckpt_steps_*.ckpt or "
                         "checkpoint-*steps.pkl, and for the latter the scaler's stats.npy / stats.h5), as the reference's vocoder_ckpt")
    ap.add_argument("--gl_iters", type=int, default=60, help="with --vocoder griffin_lim: iterations (griffin_lim_iters of base.yaml: 60)")
    ap.add_argument("--gl_inversion", default="pinv", choices=("pinv", "nnls"),
                    help="with --vocoder griffin_lim: how the mel is inverted -- pinv: the pseudo-inverse of the filter bank, floored (the "
                         "default); nnls: the non-negative least squares of the reference's GLMel, solved on the device in --nnls_iters steps")
    ap.add_argument("--nnls_iters", type=int, default=128, help="with --gl_inversion nnls: accelerated projected-gradient steps per frame")
    ap.add_argument("--long_form", action="store_true",
                    help="vocode window by window, the utterances sharing window batches (FastDiff.sample_long_batch): any length, the same PCM")
    ap.add_argument("--ndb_bins", default=None, metavar="bins.npz",
                    help="the k-means bins of `python -m fastdiff_amd.diversity fit`: the run's output waveforms go through the mel front-end on "
                         "the device, their frames are counted in the bins, and the run's NDB and JSD against the corpus (Richardson & Weiss "
                         "2018) are printed and written to <out_dir>/diversity.tsv -- one row for the run, not one per utterance")
    ap.add_argument("--trim_long_sil", action="store_true",
                    help="with --from_wav: cut the long silences of every recording on the device before its mel is taken (the reference's "
                         "trim_long_sil: true, with an energy detector in place of WebRTC's); the mel, the vocoder and every score's reference "
                         "get the trimmed recording, and <out_dir>/trim.tsv lists what was cut")
    ap.add_argument("--trim_top_db", type=float, default=40.0, help="with --trim_long_sil: a window is speech within this many dB of the loudest")
    ap.add_argument("--trim_mode", default="long", choices=("long", "edges"),
                    help="with --trim_long_sil: long = the reference's mask (pauses of more than 12 windows shortened); edges = only leading and "
                         "trailing silence")
    args = ap.parse_args(argv)
    if args.trim_long_sil and not args.from_wav:
        ap.error("--trim_long_sil cuts recordings: it needs --from_wav")
    if args.ndb_bins and args.out_sample_rate not in (None, 22050):
        ap.error("--ndb_bins takes the mel of the output waveforms at 22050 Hz: it is not available with --out_sample_rate")
    scored = _scores.enabled(stoi=args.stoi, pitch=args.pitch, spectral=args.spectral, mcd=args.mcd)
    for sc in scored:
        if not args.from_wav:
            ap.error(f"--{sc.name} scores the vocoded waveform against its recording: it needs --from_wav")
        if args.long_form:
            ap.error(f"--{sc.name} is not available with --long_form")
    if args.vocoder == "griffin_lim":
        if args.long_form:
            ap.error("--vocoder griffin_lim is not available with --long_form")
        if not 0 <= args.gl_iters <= 10000:
            ap.error(f"--gl_iters {args.gl_iters} outside 0 .. 10000")
        if not 0 <= args.nnls_iters <= 4096:
            ap.error(f"--nnls_iters {args.nnls_iters} outside 0 .. 4096")
    if args.vocoder == "pwg":
        if args.long_form:
            ap.error("--vocoder pwg is not available with --long_form (the network takes any length in one call)")
        if not args.pwg_dir:
            ap.error("--vocoder pwg needs --pwg_dir")
    from . import FastDiff
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:      # one process per GPU (utils/trainer.py:94-107): each on its own slice of the cores next to its GPU
        from . import affinity
        affinity.bind_rank(int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    torch.manual_seed(args.seed)
    model = FastDiff().cuda().eval()
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu")["state_dict"]["model"], strict=True)
    if args.mel_basis:
        model.set_mel_filterbank(np.load(args.mel_basis), variant=args.mel_variant)
    trimmed = [] if args.trim_long_sil else None
    more_in = dict(trim_long_sil=True, trim_top_db=args.trim_top_db, trim_mode=args.trim_mode, trim_report=trimmed) if args.trim_long_sil else {}      # (the default passes no new keyword)
    items = load_wav_inputs(model, args.test_input_dir, mel_variant=args.mel_variant, loud_norm=args.loud_norm, keep_wav=bool(scored), **more_in) if args.from_wav else load_mel_inputs(args.test_input_dir)
    if trimmed is not None and rank == 0:                  # (every rank trims every recording; one of them writes the table)
        os.makedirs(args.out_dir, exist_ok=True)
        print(write_trim_report(trimmed, os.path.join(args.out_dir, "trim.tsv")))
    mine = [dict(items[i], uid=i) for i in sorted(set(distributed_sampler_indices(len(items), rank, world)))]
    more = dict(mcd=True) if args.mcd else {}              # (the default passes no new keyword)
    if args.vocoder == "griffin_lim":
        how = {} if (args.gl_inversion, args.nnls_iters) == ("pinv", 128) else dict(inversion=args.gl_inversion, nnls_iters=args.nnls_iters)
        pcm = synthesize_griffin_lim(model, mine, args.gl_iters, args.max_batch, args.seed, variant=args.mel_variant, out_sample_rate=args.out_sample_rate,
                                     loudness=args.loudness, stoi=args.stoi, pitch=args.pitch, spectral=args.spectral, **how, **more)
    elif args.vocoder == "pwg":
        from .pwg import ParallelWaveGAN
        pcm = synthesize_pwg(model, ParallelWaveGAN.from_dir(args.pwg_dir), mine, args.max_batch, args.seed, out_sample_rate=args.out_sample_rate,
                             loudness=args.loudness, stoi=args.stoi, pitch=args.pitch, spectral=args.spectral, **more)
    elif args.long_form:
        if args.out_sample_rate is not None:
            ap.error("--out_sample_rate is not available with --long_form (resample its output whole with FastDiff.resample)")
        pcm = synthesize_long(model, mine, args.N, args.seed, loudness=args.loudness)
    else:
        pcm = synthesize(model, mine, args.N, args.max_batch, args.seed, out_sample_rate=args.out_sample_rate, loudness=args.loudness, stoi=args.stoi, pitch=args.pitch,
                         spectral=args.spectral, **more)
    if scored:
        pcm, report = pcm
        rows = [(it["item_name"], report[it["item_name"]]) for it in mine if it["item_name"] in report]
        for sc in scored:
            _write_table([["name"] + [key for _, key, _, _ in sc.columns] + ["status"]]
                  + [[name] + [format(r[key], fmt) for _, key, _, fmt in sc.columns] + [r[sc.status_key]] for name, r in rows], args.out_dir, sc.name, rank, world)
    if args.ndb_bins:      # a score of the whole run against the corpus the bins were fitted on (not a row of _scores.SCORES, which are per utterance)
        from . import diversity
        d = diversity.score_waveforms(model, diversity.Bins.load(args.ndb_bins), [pcm[it["item_name"]] for it in mine if it["item_name"] in pcm],
                                      variant=args.mel_variant)
        _write_table([["n", "ndb", "ndb_over_k", "jsd"], [str(d["n"]), str(d["ndb"]), format(d["ndb_over_k"], ".4f"), format(d["jsd"], ".6f")]], args.out_dir, "diversity", rank, world)
    paths = save_wavs(pcm, args.out_dir, sample_rate=args.out_sample_rate or 22050)
    print(f"rank {rank}/{world}: wrote {len(paths)} files to {args.out_dir}")


if __name__ == "__main__":
    main()
