"""One validation pass of the denoiser on the device (INTEGRATION.md "Validating and sampling during training").

What FastDiffTask.validation_step / validation_end report (FastDiff.py:52-57: theta_timestep_loss under no_grad on every batch of the
held-out loader, the batch means averaged) -- but over FIXED draws, per noise level, and without the host:

    valid = fastdiff_amd.TrainCorpus.from_binary_dir(dir, prefix="valid")
    val = fastdiff_amd.Validator(model, diffusion_hyperparams, corpus=valid, batch_size=20)
    ...
    val.run()              # enqueues ceil(n / B) batches; reads no loss value back
    print(val.result())    # synchronises once

Every item of the corpus is evaluated exactly once per pass, in order (the held-out loader is not shuffled: vocoder_base.py:29).  The
window of every item and the draws of `ts` and `z` are a pure function of (seed, batch index): the pass owns an fd_train_state whose
`iter` is the batch index, zeroed when a pass begins, and runs lvc_op.eval_collate and lvc_op.train_draw on it under its own seed -- so
two passes over unchanged weights give the same bits, and a curve over checkpoints shows the model and nothing else.  The forward runs
on the fused inference kernels (FastDiff.forward under no_grad; the module refreshes its operand packs on the device first when
TrainStep has written the parameters), the per-item MSE comes from lvc_op.item_distance, and lvc_op.eval_accumulate adds it, in slot
order and in double precision, to the pass total and to the bin of the item's diffusion step.

With sample_schedule (an inference noise schedule, e.g. schedules.noise_schedule_for(4)) every batch is also vocoded from its mel
(FastDiff.sample with the item ids as noise streams: an item's noise does not depend on the batch size) and compared with the ground
truth as the mean |difference| of the two log-mel spectrograms, both from the library's own front end ('pwg' variant), so that edge
frames affect the two alike.  sample() looks at its range check before returning: this mode waits for the device once per batch.
With stoi=True on top of it, the vocoded window is also scored against the ground truth with STOI and ESTOI (FastDiff.stoi's kernels,
fastdiff_amd/stoi.py) at the corpus' sample rate: the records of every batch stay on the device until result() reads them.
With pitch=True on top of it, both are tracked with YIN on the mel frame grid and the vocoded pitch is scored against the ground truth's
(FastDiff.pitch's kernels, fastdiff_amd/pitch.py: F0 RMSE in cents, gross pitch error, voicing decision error), likewise.
With spectral=True on top of it, the vocoded window's spectrum is scored against the ground truth's with the multi-resolution STFT
distances at the default resolutions (FastDiff.spectral's kernels, fastdiff_amd/spectral.py), likewise.
With mcd=True on top of it, the vocoded window is scored against the ground truth's with the mel-cepstral distortion, along the
time-warped path and frame by frame (FastDiff.mcd's kernels, fastdiff_amd/mcd.py), likewise.

The default seed differs from TrainStep's (0), so that batch j of a pass does not repeat the noise of training step j.  The operators
share the per-device step scratch with TrainStep (lvc_op._handle): a pass asks for far less of it than an optimizer step over the
model, so a pass between two replays of a captured step leaves the capture valid; a Validator used BEFORE a TrainStep exists is
followed by that TrainStep's own warm-up, which happens outside its capture.
"""
import numpy as np
import torch

from . import _scores, lvc_op

DEFAULT_SEED = 0x56414C      # "VAL"


class Validator:
    def __init__(self, model, diffusion_hyperparams, *, corpus, batch_size, seed=DEFAULT_SEED, bins=10, sample_schedule=None, weights=None, stoi=False, sample_rate=22050,
                 pitch=False, spectral=False, mcd=False):
        if int(batch_size) < 1:
            raise ValueError(f"Validator: batch_size={batch_size} (at least 1)")
        if not 1 <= int(bins) <= lvc_op.EVAL_MAX_BINS:
            raise ValueError(f"Validator: bins={bins} (1..{lvc_op.EVAL_MAX_BINS})")
        params = list(model.parameters())
        if not params or not all(p.is_cuda for p in params):
            raise RuntimeError("fastdiff_amd.Validator needs the module's parameters on a HIP device (no CPU fallback)")
        self.model, self.device = model, params[0].device
        # what run() computes with: None = whatever the module uses (the live parameters unless its use_weights said otherwise), else a
        # source as FastDiff.use_weights takes it (a ParamEMA, a mapping name -> tensor), chosen for the pass and handed back after it
        self.weights = weights
        if weights is not None:
            model.check_weights_source(weights)      # names and shapes: refused now, not inside a pass
        if corpus.device != self.device:
            raise RuntimeError(f"Validator: the corpus lies on {corpus.device}, the module on {self.device} (corpus.to(device) uploads it)")
        if corpus.hop_size != model.hop_length:
            raise ValueError(f"Validator: the corpus' hop_size ({corpus.hop_size}) is not the module's ({model.hop_length})")
        self.corpus, self.batch_size, self.seed, self.bins = corpus, int(batch_size), int(seed), int(bins)
        self.T_train = int(diffusion_hyperparams["T"])
        self.alpha = diffusion_hyperparams["alpha"].detach().to(self.device, torch.float32).contiguous()
        self.n_batches = (corpus.n_items + self.batch_size - 1) // self.batch_size
        self.table = None
        if sample_schedule is not None:
            from .sampler import InferenceSchedule
            self.table = InferenceSchedule(diffusion_hyperparams, torch.as_tensor(sample_schedule, dtype=torch.float32), verbose=False).rows()
        B, F, L, dev = self.batch_size, corpus.frames, corpus.frames * corpus.hop_size, self.device
        self._state = lvc_op.new_train_state(dev)             # fd_train_state: iter = the batch index
        self._acc = lvc_op.new_eval_state(dev)                # fd_eval_state of the loss
        self._acc_mel = lvc_op.new_eval_state(dev) if self.table is not None else None
        # the buffers of the current batch (those of the last one after a pass)
        self.mel = torch.empty((B, 80, F), device=dev, dtype=torch.float32)
        self.wav, self.x_t, self.z = (torch.empty((B, 1, L), device=dev, dtype=torch.float32) for _ in range(3))
        self.steps = torch.empty((B, 1), device=dev, dtype=torch.float32)
        self.picked = torch.empty((B, 2), device=dev, dtype=torch.int64)
        self.values = torch.empty(B, device=dev, dtype=torch.float32)
        self.item_loss = torch.zeros(corpus.n_items, device=dev, dtype=torch.float32)
        self.eps = self.sampled = self.mel_sampled = self.mel_target = None
        self.values_mel = torch.empty(B, device=dev, dtype=torch.float32) if self.table is not None else None
        self.item_mel_l1 = torch.zeros(corpus.n_items, device=dev, dtype=torch.float32) if self.table is not None else None
        self.sample_rate = int(sample_rate)                    # the rate of the corpus' waveforms
        self._scored = []                                      # (score, its configuration, its records: slot b of batch j is row j B + b)
        for sc in _scores.enabled(stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd):
            if self.table is None:
                raise ValueError(f"Validator: {sc.name}=True scores the vocoded windows, which needs sample_schedule")
            cfg = sc.config(self.sample_rate, corpus.hop_size)      # refused now, not inside a pass
            self._scored.append((sc, cfg, torch.zeros((self.n_batches * B, sc.module.RECORD.itemsize), device=dev, dtype=torch.uint8)))

    def state(self):
        """The pass's fd_train_state as a dict (`iter` = batches done).  Synchronises."""
        return lvc_op.read_train_state(self._state)

    def begin(self):
        """Start a pass: the batch index, the accumulators and the per-item outputs go back to zero (on the current stream)."""
        for t in (self._state, self._acc, self._acc_mel, self.item_loss, self.item_mel_l1):
            if t is not None:
                t.zero_()

    @torch.no_grad()
    def batch(self, j):
        """Batch j of the pass begun last; the batches of a pass are called in order, j = 0 .. n_batches - 1 (the device counts them
        itself: j only names the items' noise streams of the sampled metric).  run() is begin() and these calls."""
        B, F, m = self.batch_size, self.corpus.frames, self.model
        lvc_op.eval_collate(self.corpus, B, seed=self.seed, state=self._state, out=(self.mel, self.wav, self.picked))
        lvc_op.train_draw(self.wav, self.alpha, self.T_train, seed=self.seed, state=self._state, out=(self.x_t, self.z, self.steps))
        self.eps = m((self.x_t, self.mel, self.steps))
        lvc_op.item_distance(self.eps, self.z, 0, out=self.values)
        if self.table is not None:
            self.sampled = m.sample(self.mel, self.table, seed=self.seed, stream_ids=[j * B + b for b in range(B)])
            self.mel_sampled = m.mel_spectrogram(self.sampled.view(B, -1), n_frames=F, variant="pwg")
            self.mel_target = m.mel_spectrogram(self.wav.view(B, -1), n_frames=F, variant="pwg")
            lvc_op.item_distance(self.mel_sampled, self.mel_target, 1, out=self.values_mel)
            lvc_op.eval_accumulate(self.values_mel, self.picked, self._acc_mel, item_out=self.item_mel_l1)
            for sc, cfg, rec in self._scored:
                lib, h = m._ready(self.device)
                sc.module._enqueue(lib, h, m._stream(self.device), self.wav, self.sampled, None, cfg, rec=rec[j * B: (j + 1) * B])
        # last: it advances the batch index, behind every read of it
        lvc_op.eval_accumulate(self.values, self.picked, self._acc, steps=self.steps, T_train=self.T_train, bins=self.bins,
                               item_out=self.item_loss, advance=self._state)

    def run(self):
        """One pass: ceil(n / B) batches enqueued on the current stream, nothing read back (with sample_schedule: one wait per batch).
        The module's `training` flag is as before afterwards.  With weights= the module computes from that source during the pass and
        from its previous one after it; its packs are marked stale, so the next inference call builds them again from that one."""
        was_training = self.model.training
        self.model.eval()
        switched = self.weights is not None
        previous = self.model.use_weights(self.weights) if switched else None
        try:
            self.begin()
            for j in range(self.n_batches):
                self.batch(j)
        finally:
            if switched:
                self.model.use_weights(previous)
            self.model.train(was_training)
        return self

    def result(self):
        """{"loss", "items", "nonfinite", "loss_by_t" [bins], "count_by_t" [bins], "item_loss" [n]} of the last pass, plus "mel_l1" and
        "item_mel_l1" [n] with sample_schedule, plus "stoi", "estoi" (the means over the items with status OK), "item_stoi", "item_estoi"
        [n] (NaN where not OK) and "stoi_skipped" (the items not OK) with stoi=True, plus "f0_rmse_cents", "gpe" (the means over the items
        with status OK), "vde" (over the items OK or UNVOICED), "item_f0_rmse_cents", "item_gpe", "item_vde" [n] (NaN where not measured) and
        "pitch_skipped" (the items not OK) with pitch=True, plus "mr_sc", "mr_logmag", "lsd_db" (the means over the items with status OK),
        "item_mr_sc", "item_mr_logmag", "item_lsd_db" [n] (NaN where not OK) and "spectral_skipped" (the items not OK: windows of at most
        1024 samples) with spectral=True, plus "mcd_dtw", "mcd_linear" (the means over the items with status OK), "item_mcd_dtw",
        "item_mcd_linear" [n] (NaN where not OK) and "mcd_skipped" (the items not OK) with mcd=True.  loss = the mean over the items (the reference's validation_end averages batch means:
        the two differ only through a short last batch); loss_by_t[k] = the mean over the items whose step fell into
        [k T / bins, (k + 1) T / bins), NaN where none did.  Synchronises once."""
        acc = lvc_op.read_eval_state(self._acc, self.bins)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {"loss": acc["sum"] / acc["count"] if acc["count"] else float("nan"), "items": acc["count"], "nonfinite": acc["nonfinite"],
                   "loss_by_t": acc["bin_sum"] / acc["bin_count"], "count_by_t": acc["bin_count"], "item_loss": self.item_loss.cpu().numpy()}
        if self._acc_mel is not None:
            mel = lvc_op.read_eval_state(self._acc_mel, 1)
            out["mel_l1"] = mel["sum"] / mel["count"] if mel["count"] else float("nan")
            out["item_mel_l1"] = self.item_mel_l1.cpu().numpy()
        n = self.corpus.n_items
        for sc, _, dev_rec in self._scored:
            rec = sc.module._record(dev_rec)                 # slot b of batch j is item j B + b: the first n rows are the items
            status = rec["status"][:n]
            for key, name, measured, _ in sc.columns:
                use = np.isin(status, measured)
                item = np.where(use, rec[key][:n], np.nan)
                out["item_" + name] = item
                out[name] = float(item[use].mean()) if use.any() else float("nan")
            out[sc.name + "_skipped"] = int(n - (status == sc.module.OK).sum())
        return out
