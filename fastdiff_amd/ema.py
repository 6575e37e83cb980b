"""An exponential moving average of a module's parameters, kept on the device (INTEGRATION.md "Training").

The reference has no EMA: this is an addition, off by default.  The average lives in one flat float32 buffer (the "shadow"), one segment
per entry of state_dict() -- weight_g and weight_v of a weight-normed layer are averaged separately, as an EMA over a state_dict does --
and moves by one call of lvc_op.ema_multi (fd_ema_multi) behind the optimizer:

    e = e + w * (p - e),   w = float32(1 - decay_t),   decay_t = min(decay, (1 + updates) / (10 + updates))  (warmup) or decay

Whether it moves is decided on the device: only when the optimizer's `applied` counter went up since the last update, so a step that
the non-finite guard skipped leaves the average alone, and the host never has to read the train state to know.

    ts = fastdiff_amd.TrainStep(model, diffusion_hyperparams, ema_decay=0.999)      # ts.ema: updated inside the captured step
    model.use_weights(ts.ema)                                                      # inference from the average (FastDiff.use_weights)
    ts.ema.copy_to(export_model)                                                   # ... or write it over a module's parameters
"""
from collections import OrderedDict

import torch

from . import lvc_op

ALIGN = 4      # floats: every segment of the shadow starts 16-byte aligned (fd_ema_multi's 16-byte path)


def decay_at(updates, decay, warmup=True):
    """The decay of the update that follows `updates` earlier ones: the host twin of fd_ema_multi's decision, in Python floats."""
    n = int(updates)
    return min(float(decay), (1 + n) / (10 + n)) if warmup else float(decay)


class ParamEMA:
    def __init__(self, model, decay=0.999, warmup=True):
        named = list(model.named_parameters())
        params = [p for _, p in named]
        if not params or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params):
            raise RuntimeError("fastdiff_amd.ParamEMA needs the module's parameters as contiguous float32 tensors on a HIP device (no CPU fallback)")
        by_name = dict(named)
        keys = list(model.state_dict().keys())
        if set(keys) != set(by_name) or len(keys) != len(named):
            raise RuntimeError("fastdiff_amd.ParamEMA: the module's state_dict() keys must be its named parameters (no buffers, no shared tensors)")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ParamEMA: decay={decay} (0..1)")
        self.model, self.device = model, params[0].device
        self.decay, self.warmup = float(decay), bool(warmup)
        self.names = keys
        self.params = [by_name[k] for k in keys]
        offsets, at = [], 0
        for p in self.params:
            offsets.append(at)
            at += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.shadow = torch.zeros(at, device=self.device, dtype=torch.float32)
        self.tensors = OrderedDict((k, self.shadow[o: o + p.numel()].view(p.shape)) for k, o, p in zip(keys, offsets, self.params))
        self._hyper_dev = lvc_op.new_state("fd_ema_hyper", self.device, torch.float64)
        self._write_hyper()
        self._state = lvc_op.new_ema_state(self.device)                                 # fd_ema_state
        self.reset()

    def _write_hyper(self):
        self._hyper_dev.copy_(lvc_op.pack_state("fd_ema_hyper", torch.float64, decay=self.decay, warmup=1.0 if self.warmup else 0.0))

    def reset(self, seen_applied=0):
        """The shadow := the parameters as they are now, no update counted; seen_applied: the optimizer's `applied` count that the
        average is taken to have seen (it moves again once the count exceeds it)."""
        with torch.no_grad():
            for e, p in zip(self.tensors.values(), self.params):
                e.copy_(p)
        self._state.copy_(lvc_op.pack_state("fd_ema_state", seen_applied=int(seen_applied)))

    def update(self, train_state, ema_state=None):
        """One lvc_op.ema_multi call on the current stream, behind the optimizer that advances `train_state` (a new_train_state
        tensor, only read).  Does not synchronise.  ema_state: another fd_ema_state than the average's own (TrainStep's warm-up)."""
        lvc_op.ema_multi(list(zip(self.params, self.tensors.values())), self._hyper_dev, train_state,
                         self._state if ema_state is None else ema_state)

    def set_decay(self, decay):
        """The decay of the following updates: a copy of 8 bytes into device memory, between two replays."""
        self.decay = float(decay)
        lvc_op.state_field(self._hyper_dev, "fd_ema_hyper", "decay").copy_(torch.tensor([self.decay], dtype=torch.float64))

    def state(self):
        """{"updates", "seen_applied"} of the device's fd_ema_state.  Synchronises."""
        st = lvc_op.read_ema_state(self._state)
        return {"updates": st["updates"], "seen_applied": st["seen_applied"]}

    def state_dict(self):
        """{"decay", "warmup", "updates", "seen_applied", "shadow": {name: tensor}} (copies).  Synchronises."""
        st = self.state()
        return {"decay": self.decay, "warmup": self.warmup, "updates": st["updates"], "seen_applied": st["seen_applied"],
                "shadow": OrderedDict((k, t.detach().clone()) for k, t in self.tensors.items())}

    def load_state_dict(self, sd):
        shadow = sd["shadow"]
        if set(shadow) != set(self.tensors):
            odd = sorted(set(shadow) ^ set(self.tensors))
            raise ValueError(f"ParamEMA.load_state_dict: the shadow's names are not the module's (first differences: {odd[:3]})")
        for k, t in self.tensors.items():
            if tuple(shadow[k].shape) != tuple(t.shape):
                raise ValueError(f"ParamEMA.load_state_dict: {k}: shape {list(shadow[k].shape)}, expected {list(t.shape)}")
        with torch.no_grad():
            for k, t in self.tensors.items():
                t.copy_(shadow[k])
        self.decay, self.warmup = float(sd["decay"]), bool(sd["warmup"])
        self._write_hyper()
        self._state.copy_(lvc_op.pack_state("fd_ema_state", updates=int(sd["updates"]), seen_applied=int(sd["seen_applied"])))

    def copy_to(self, module):
        """Write the shadow over the parameters of `module` (this one or another of the same architecture) with torch's copy_: for
        export.  The parameters' versions move as usual, so a FastDiff notices and uploads them before its next inference call."""
        target = dict(module.named_parameters())
        if set(target) != set(self.tensors):
            odd = sorted(set(target) ^ set(self.tensors))
            raise ValueError(f"ParamEMA.copy_to: the module's parameter names are not the shadow's (first differences: {odd[:3]})")
        for k, t in self.tensors.items():
            if tuple(target[k].shape) != tuple(t.shape):
                raise ValueError(f"ParamEMA.copy_to: {k}: shape {list(target[k].shape)}, expected {list(t.shape)}")
        with torch.no_grad():
            for k, t in self.tensors.items():
                target[k].copy_(t)
