"""One training step of the scheduling network phi on the device (INTEGRATION.md "A schedule for your own weights").

The twin of TrainStep for phi_loss (util.py:328-362): the denoiser theta is frozen -- it runs under no_grad on the fused inference
kernels and follows FastDiff.use_weights, so phi can be trained against the averaged weights -- and only the six tensors of a
fastdiff_amd.NoisePredictor are optimized.  Per step: the batch (from the host, or cut from a device-resident corpus by
lvc_op.train_collate), the draws (lvc_op.phi_draw: ts in [tau, T - tau), z, x_t, beta_next, delta), eps_theta, beta_hat with autograd
(lvc_op.band_pool / npred_head), the residual's means on fixed-order sums (lvc_op.phi_residual), the reference's algebra on [B] tensors,
backward, and clip + non-finite guard + AdamW (lvc_op.adamw_multi).  Every per-step quantity lives in device memory and nothing waits
for the device:

    pred = fastdiff_amd.NoisePredictor().cuda()
    ps = fastdiff_amd.PhiStep(model, pred, dh, corpus=corpus, batch_size=20)        # dh: calc_diffusion_hyperparams(...): T, alpha, tau
    for it in range(steps):
        loss = ps.step()                                                             # a device tensor; ps.state() synchronises
    model.noise_pred = pred

The step runs eagerly (a dozen small launches around one denoiser evaluation); no graph is captured.  Two runs from the same seed give
the same parameters bit for bit.  state(), set_lr, state_dict and load_state_dict are TrainStep's, over the predictor's six tensors.
"""
import torch

from . import lvc_op
from .sampler import phi_loss_from_draw
from .trainstep import TrainStep


class PhiStep(TrainStep):
    def __init__(self, model, predictor, diffusion_hyperparams, lr=2e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0, clip_grad_norm=1.0,
                 seed=0, *, corpus=None, batch_size=None, rank=0, world_size=1):
        self.model, self.predictor = model, predictor
        self._init_optimizer(list(predictor.parameters()), lr, betas, eps, weight_decay, clip_grad_norm)
        if any(p.device != self.device for p in model.parameters()):
            raise RuntimeError(f"PhiStep: the denoiser and the predictor must lie on one device ({self.device})")
        dh = diffusion_hyperparams
        self.T_train, self.tau = int(dh["T"]), int(dh["tau"])
        if self.tau < 0 or self.T_train <= 2 * self.tau:
            raise ValueError(f"PhiStep: T={self.T_train} must exceed 2 tau={2 * self.tau}")
        self.alpha = dh["alpha"].detach().to(self.device, torch.float32).contiguous()
        self.seed = int(seed)
        self._state_loss = lvc_op.state_field(self._state, "fd_train_state", "loss")
        self.ema = None                                                                  # (no average: state_dict() asks)
        self._init_batch_source(corpus, batch_size, rank, world_size)
        self.mel = self.wav = self.draw = None      # the buffers of the current batch shape

    def _prepare(self, mel_shape, wav_shape):
        B, L = wav_shape[0], wav_shape[-1]
        if len(wav_shape) != 3 or wav_shape[1] != 1 or L % 32 != 0 or L < 64:
            raise ValueError("PhiStep.step: wavs [B, 1, L] with L a multiple of 32, at least 64")
        dev = self.device
        self.mel = torch.empty(tuple(mel_shape), device=dev, dtype=torch.float32)
        self.wav = torch.empty((B, 1, L), device=dev, dtype=torch.float32)
        # x_t, z, steps, beta_nxt, delta, delta2
        self.draw = tuple(torch.empty((B, 1, L), device=dev, dtype=torch.float32) for _ in range(2)) + \
            tuple(torch.empty((B, 1), device=dev, dtype=torch.float32) for _ in range(4))

    def step(self, mels=None, wavs=None):
        """One step of phi on the batch (mels [B, 80, T], wavs [B, 1, T * hop]), or, without arguments, on a batch cut from the
        constructor's corpus inside the step (`picked` = corpus.plan(state()["iter"], batch_size, seed, rank, world_size)).  Returns the
        loss as a device tensor and does not synchronise.  No parameter of the denoiser is written."""
        if not torch.is_grad_enabled():
            raise RuntimeError("PhiStep.step needs gradients enabled")
        collate, shapes = self._batch_of(mels, wavs)
        if shapes != self._key:
            self._prepare(*shapes)
            self._key = shapes
        if collate:
            self._collate()
        else:
            self.mel.copy_(mels, non_blocking=True)
            self.wav.copy_(wavs, non_blocking=True)
        lvc_op.phi_draw(self.wav, self.alpha, self.T_train, self.tau, seed=self.seed, state=self._state, out=self.draw)
        self.predictor.zero_grad(set_to_none=True)
        loss = phi_loss_from_draw(self.model, self.predictor, self.mel, self.draw)
        loss.backward()
        self._state_loss.copy_(loss.detach().view(1))
        grads = [None if p.grad is None else p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in self.params]
        lvc_op.adamw_multi(list(zip(self.params, grads, self.exp_avg, self.exp_avg_sq)), self._hyper_dev, self._state)
        self.loss = loss.detach()
        return self.loss
