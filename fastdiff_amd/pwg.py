"""Parallel WaveGAN on the device: the reference's neural baseline vocoder behind the interface of the other two.

The reference registers PWG next to FastDiff and Griffin-Lim (vocoders/pwg.py over modules/parallel_wavegan: ParallelWaveGANGenerator, a
30-layer non-causal WaveNet at the sample rate, conditioned on the up-sampled mel).  Here it is one call (fd_pwg_generate,
include/fastdiff_hip_ext.h, which defines the computation and says how the device runs it: the conditioning projected to every layer's
gate channels at the frame rate, one kernel per residual block on the exact-fp32 matrix instruction, a tail kernel).

    ParallelWaveGAN(**generator_params)     the reference generator's constructor arguments; what the specialised path does not build
                                            (causal, pitch embedding, NSF, MelGANGenerator, an activation in the up-sampler, other widths)
                                            is refused here, with the field and its value
    .load_state_dict(state)                 a plain state dict, the official checkpoint (["models"]["generator"]) or the reference's own
                                            (["state_dict"]["model_gen"]); weight_g / weight_v pairs are folded on the host in float64
    ParallelWaveGAN.from_dir(dir)           config.yaml + the newest checkpoint + the scaler's statistics, as vocoders/pwg.py reads them
    .set_scaler(mean, scale)                a StandardScaler's statistics ([80] each), or None, None
    .forward(z, c)                          z [B, 1, hop T], c [B, 80, T + 2 w] (padded) -> [B, 1, hop T]: the reference module's call
    .spec2wav(mel, lens=None, seed=0, stream_ids=None, z=None)   mel [B, 80, T] -> wav [B, hop T]: PWG.spec2wav, batched
    .draw_z(B, L, seed, stream_ids)         the z a spec2wav call draws: [B, L]
    samples(frames), receptive_field         hop * frames; 2 * (the sum of the dilations) + 1

Tensors live on the HIP device; there is no CPU path.  Calls run on the current stream, on the per-device handle of the operators
(lvc_op), and are capturable once a call of the same shape has grown the scratch buffer.
"""
import ctypes as ct
import glob
import os
import re

import numpy as np
import torch

from . import _capi, _wave

TILE, PHILOX_STREAM, MELS = _capi.FD_PWG_TILE, _capi.FD_PWG_PHILOX_STREAM, 80
_UPSAMPLE_NETS = {"ConvInUpsampleNetwork": _capi.FD_PWG_CONV_IN_UPSAMPLE, "UpsampleNetwork": _capi.FD_PWG_UPSAMPLE,
                  "MelGANGenerator": _capi.FD_PWG_MELGAN}
_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128,
                 skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True,
                 use_causal_conv=False, upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork",
                 upsample_params=None, use_pitch_embed=False, use_nsf=False, sample_rate=22050)
# what the reference's constructor itself writes into upsample_params, and the up-sampler's own arguments with the only values built
_UPSAMPLE_PARAMS = {"upsample_scales", "nonlinear_activation", "nonlinear_activation_params", "interpolate_mode", "freq_axis_kernel_size",
                    "aux_channels", "aux_context_window", "use_causal_conv"}


def config_struct(**kw):
    """The reference generator's constructor arguments -> fd_pwg_config.  Arguments the C structure has no field for are refused here
    (NotImplementedError, the field and its value in the message); every other refusal is fd_pwg_create's."""
    unknown = sorted(set(kw) - set(_DEFAULTS))
    if unknown:
        raise TypeError(f"ParallelWaveGAN: unexpected argument {unknown[0]!r}")
    a = dict(_DEFAULTS, **kw)
    up = dict(a["upsample_params"] or {"upsample_scales": [4, 4, 4, 4]})
    extra = sorted(set(up) - _UPSAMPLE_PARAMS)
    if extra:
        raise NotImplementedError(f"ParallelWaveGAN: upsample_params[{extra[0]!r}] = {up[extra[0]]!r} is not built")
    if a["upsample_net"] not in _UPSAMPLE_NETS:
        raise NotImplementedError(f"ParallelWaveGAN: upsample_net = {a['upsample_net']!r} is not built")
    if up.get("interpolate_mode", "nearest") != "nearest":
        raise NotImplementedError(f"ParallelWaveGAN: interpolate_mode = {up['interpolate_mode']!r}: only 'nearest' is built")
    for k in ("aux_channels", "aux_context_window", "use_causal_conv"):
        if k in up and up[k] != a[k]:
            raise ValueError(f"ParallelWaveGAN: upsample_params[{k!r}] = {up[k]!r} contradicts {k} = {a[k]!r}")
    scales = [int(s) for s in up.get("upsample_scales", [])]
    if len(scales) > 8:
        raise NotImplementedError(f"ParallelWaveGAN: upsample_scales = {scales}: at most {_capi.FD_PWG_MAX_SCALES} scales are built")
    c = _capi.FdPwgConfig()
    for k in ("in_channels", "out_channels", "kernel_size", "layers", "stacks", "residual_channels", "gate_channels", "skip_channels",
              "aux_channels", "aux_context_window", "bias", "use_causal_conv", "upsample_conditional_features", "use_pitch_embed", "use_nsf"):
        setattr(c, k, int(a[k]))
    c.upsample_net = _UPSAMPLE_NETS[a["upsample_net"]]
    c.n_scales = len(scales)
    for i, s in enumerate(scales):
        c.upsample_scales[i] = s
    c.upsample_activation = 0 if up.get("nonlinear_activation") is None else 1
    c.interpolate_nearest = 1
    c.freq_axis_kernel_size = int(up.get("freq_axis_kernel_size", 1))
    return c, a, up


def _refuse(lib, c):
    """fd_pwg_create's refusal of a configuration without a device: NotImplementedError with the field and its value."""
    if lib.fd_pwg_samples(ct.byref(c), 0) >= 0:
        return
    out = ct.c_void_p()
    _capi.check(lib, None, lib.fd_pwg_create(None, ct.byref(c), ct.byref(out)), "fd_pwg_create")


def samples(frames, **kw):
    """hop * frames of a configuration (fd_pwg_samples)."""
    lib = _capi.load()
    c = config_struct(**kw)[0]
    _refuse(lib, c)
    return int(lib.fd_pwg_samples(ct.byref(c), int(frames)))


def receptive_field(**kw):
    """2 * (the sum of the layers' dilations) + 1 (fd_pwg_receptive_field): 6139 for the default."""
    lib = _capi.load()
    c = config_struct(**kw)[0]
    _refuse(lib, c)
    return int(lib.fd_pwg_receptive_field(ct.byref(c)))


def fold_weight_norm(state):
    """A state dict with weight_g / weight_v pairs -> name -> float32 numpy array with weight = g v / |v|, the norm over all but the
    first axis, in float64, rounded once.  Tensors without weight norm pass through."""
    out = {}
    for name, v in state.items():
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if name.endswith(".weight_g"):
            continue
        if name.endswith(".weight_v"):
            g = state[name[:-2] + "_g"]
            g64 = (g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)).astype(np.float64)
            v64 = v.astype(np.float64)
            norm = np.sqrt((v64.reshape(v64.shape[0], -1) ** 2).sum(1)).reshape(g64.shape)
            out[name[:-2]] = (v64 * (g64 / norm)).astype(np.float32)
        else:
            out[name] = v.astype(np.float32)
    return out


def unwrap_checkpoint(obj):
    """A plain state dict, the official checkpoint or the reference's own -> (the generator's state dict, True if it was the official one)."""
    if isinstance(obj, dict) and "state_dict" in obj and isinstance(obj["state_dict"], dict) and "model_gen" in obj["state_dict"]:
        return obj["state_dict"]["model_gen"], False
    if isinstance(obj, dict) and "models" in obj and "generator" in obj["models"]:
        return obj["models"]["generator"], True
    return obj, False


def read_stats(path):
    """(mean, scale) [80] each from a scaler's statistics: .npy ([2, 80]: mean, scale) or .h5 (datasets mean, scale; needs h5py)."""
    if path.endswith(".npy"):
        s = np.load(path)
        return np.asarray(s[0], np.float32), np.asarray(s[1], np.float32)
    if path.endswith(".h5"):
        try:
            import h5py
        except ImportError as e:
            raise ImportError(f"ParallelWaveGAN: {path} holds the scaler's statistics in HDF5, which needs h5py; "
                              "store them as a .npy ([2, 80]: mean, scale) instead") from e
        with h5py.File(path, "r") as f:
            return np.asarray(f["mean"][()], np.float32), np.asarray(f["scale"][()], np.float32)
    raise ValueError(f"ParallelWaveGAN: statistics {path}: only .npy and .h5 are read")


class ParallelWaveGAN:
    def __init__(self, device=None, **generator_params):
        self._lib = _capi.load()
        self._p = None
        cfg, self.params, self.upsample_params = config_struct(**generator_params)
        _refuse(self._lib, cfg)
        self.cfg = cfg
        self.layers, self.stacks, self.aux_context_window = cfg.layers, cfg.stacks, cfg.aux_context_window
        self.upsample_scales = [cfg.upsample_scales[i] for i in range(cfg.n_scales)]
        self.hop_size = int(np.prod(self.upsample_scales))
        self.receptive_field_size = int(self._lib.fd_pwg_receptive_field(ct.byref(cfg)))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ParallelWaveGAN: a HIP device is expected (there is no CPU path)")
        _, self._h = _wave.default_handle(torch.empty(0, device=self.device))[:2]
        p = ct.c_void_p()
        _capi.check(self._lib, self._h, self._lib.fd_pwg_create(self._h, ct.byref(cfg), ct.byref(p)), "fd_pwg_create")
        self._p = p
        self.scaler = None
        self.committed = False

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.fd_pwg_destroy(self._p)
            self._p = None

    def _check(self, rc, what):
        return _capi.check(self._lib, self._h, rc, what)

    # ------------------------------------------------------------------------------------------------------------------- weights
    def load_state_dict(self, state):
        """Every tensor of the configuration must be there (KeyError names the first that is not); others are refused."""
        state = fold_weight_norm(unwrap_checkpoint(state)[0])
        for name, v in state.items():
            v = np.ascontiguousarray(v, dtype=np.float32)
            self._check(self._lib.fd_pwg_set_weight(self._p, name.encode(), v.ctypes.data, v.size), "fd_pwg_set_weight")
        self._check(self._lib.fd_pwg_commit(self._p), "fd_pwg_commit")
        self.committed = True
        return self

    def set_scaler(self, mean, scale):
        if mean is None and scale is None:
            self._check(self._lib.fd_pwg_set_scaler(self._p, None, None), "fd_pwg_set_scaler")
            self.scaler = None
            return self
        mean, scale = np.ascontiguousarray(mean, dtype=np.float32), np.ascontiguousarray(scale, dtype=np.float32)
        if mean.shape != (MELS,) or scale.shape != (MELS,):
            raise ValueError(f"ParallelWaveGAN: expected mean and scale [80], got {list(mean.shape)} and {list(scale.shape)}")
        self._check(self._lib.fd_pwg_set_scaler(self._p, mean.ctypes.data, scale.ctypes.data), "fd_pwg_set_scaler")
        self.scaler = (mean, scale)
        return self

    @classmethod
    def from_dir(cls, base_dir, device=None):
        """config.yaml + the newest checkpoint of `base_dir`, as vocoders/pwg.py: the reference's own model_ckpt_steps_*.ckpt (no scaler),
        else the official checkpoint-*steps.pkl with the scaler's statistics (stats.npy, or stats.h5 if h5py imports)."""
        import yaml
        with open(os.path.join(base_dir, "config.yaml")) as f:
            config = yaml.safe_load(f)

        def newest(pattern, rx):
            found = [(int(re.search(rx, os.path.basename(p)).group(1)), p) for p in glob.glob(os.path.join(base_dir, pattern))]
            return max(found)[1] if found else None

        ckpt = newest("model_ckpt_steps_*.ckpt", r"model_ckpt_steps_(\d+)\.ckpt") or newest("checkpoint-*steps.pkl", r"checkpoint-(\d+)steps\.pkl")
        if ckpt is None:
            raise FileNotFoundError(f"ParallelWaveGAN: no model_ckpt_steps_*.ckpt or checkpoint-*steps.pkl in {base_dir}")
        m = cls(device=device, **config["generator_params"])
        state, official = unwrap_checkpoint(torch.load(ckpt, map_location="cpu"))
        m.load_state_dict(state)
        if official:
            npy, h5 = os.path.join(base_dir, "stats.npy"), os.path.join(base_dir, "stats.h5")
            m.set_scaler(*read_stats(npy if os.path.exists(npy) or not os.path.exists(h5) else h5))
        m.config = config
        return m

    # ------------------------------------------------------------------------------------------------------------------- calls
    def _generate(self, src, padded, lens, z, seed, stream_ids, wav=None):
        if not self.committed:
            raise RuntimeError("ParallelWaveGAN: load_state_dict has not run")
        if not isinstance(src, torch.Tensor) or not src.is_cuda:
            raise ValueError("ParallelWaveGAN: a tensor on the HIP device is expected (there is no CPU path)")
        src = src.contiguous().float()
        if src.dim() == 2:
            src = src.unsqueeze(0)
        w = self.aux_context_window
        T = src.shape[-1] - (2 * w if padded else 0)
        if src.dim() != 3 or src.shape[1] != MELS or T < 1:
            raise ValueError(f"ParallelWaveGAN: expected {'c [B, 80, T + %d]' % (2 * w) if padded else 'a mel [B, 80, T]'}, got {list(src.shape)}")
        B, L = src.shape[0], self.hop_size * T
        if z is not None:
            if not isinstance(z, torch.Tensor) or z.device != src.device:
                raise ValueError("ParallelWaveGAN: z must be a tensor on the conditioning's device")
            z = z.contiguous().float()
            if z.numel() != B * L:
                raise ValueError(f"ParallelWaveGAN: z {list(z.shape)} does not hold {B} x {L} samples")
        if wav is None:
            wav = torch.empty((B, L), device=src.device, dtype=torch.float32)
        ids = None
        if stream_ids is not None:
            if len(stream_ids) != B:
                raise ValueError(f"ParallelWaveGAN: stream_ids has {len(stream_ids)} entries for {B} items")
            ids = (ct.c_uint64 * B)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids])
        from . import lvc_op
        rc = self._lib.fd_pwg_generate(self._p, src.data_ptr(), int(padded), B, T, _wave.counts(lens, B, "ParallelWaveGAN"),
                                       None if z is None else z.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, ids, wav.data_ptr(), wav.stride(0),
                                       lvc_op._stream(src.device))
        self._check(rc, "fd_pwg_generate")
        return wav

    def forward(self, z, c):
        """The reference module's call: z [B, 1, hop T] noise, c [B, 80, T + 2 w] padded conditioning -> [B, 1, hop T]."""
        return self._generate(c, True, None, z, 0, None).unsqueeze(1)

    __call__ = forward

    def spec2wav(self, mel, lens=None, seed=0, stream_ids=None, z=None, out=None):
        """mel [B, 80, T] (or [80, T]) -> wav [B, hop T]: the scaler if one is set, w frames of edge replication, z ~ N(0, 1) drawn on the
        device keyed on (seed, stream_ids[b] or b, sample) unless given.  lens: [B] frame counts of a padded batch; item b fills its first
        hop lens[b] samples, the rest of its row is 0.  out: a float32 tensor [B, >= hop T] whose rows (of any pitch) receive the result."""
        return self._generate(mel, False, lens, z, seed, stream_ids, out)

    def draw_z(self, B, L, seed=0, stream_ids=None):
        z = torch.empty((B, L), device=self.device, dtype=torch.float32)
        ids = None if stream_ids is None else (ct.c_uint64 * B)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids])
        from . import lvc_op
        self._check(self._lib.fd_pwg_draw(self._h, B, L, int(seed) & 0xFFFFFFFFFFFFFFFF, ids, z.data_ptr(), L, lvc_op._stream(self.device)), "fd_pwg_draw")
        return z
