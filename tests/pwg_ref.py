"""Parallel WaveGAN's generator restated from include/fastdiff_hip_ext.h ("Parallel WaveGAN"), for the tests and tools/pwg_bench.py.

    default_config()                              the reference's constructor defaults, as a dict
    weight_shapes(cfg)                            name -> shape of the state dict after weight-norm removal, in the reference's order
    make_weights(cfg, seed)                       name -> float32 array, from oracle/philox.py's integer words only: its bits depend on no
                                                  library version, so the default architecture's 1.33 M parameters are not stored
    with_weight_norm(weights, seed)               the same network before removal: every conv's weight as a weight_g / weight_v pair
    forward(weights, cfg, z, c, dtype, device)    z [B, 1, hop T], c [B, 80, T + 2 w] (padded) -> [B, 1, hop T]: the direct form
    forward_projected(...)                        the form the device runs: conditioning projected to every layer's 128 gate channels at
                                                  the frame rate, then up-sampled per layer
    pad_mel(mel, w, mean, scale)                  what PWG.spec2wav does in front: (mel - mean) / scale, w frames of edge replication
    draw_z(seed, ids, L)                          the host twin of the device's z: float64 [B, L]

Every step is written out with torch's elementary operations so that the same code runs in float64 on the CPU (the oracle) and in float32
on the device (the eager baseline of the benchmark).  Nothing here is taken from the reference's text.
"""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import philox   # noqa: E402

RES, GATE, SKIP, AUX = 64, 128, 64, 80
PHILOX_STREAM = 0xFFFFFFF7            # FD_PWG_PHILOX_STREAM: the word of z
WEIGHT_STREAM = 0x50574700            # make_weights' own: never a word the library draws on


def default_config():
    return dict(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=RES, gate_channels=GATE,
                skip_channels=SKIP, aux_channels=AUX, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True,
                use_causal_conv=False, upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork",
                upsample_params={"upsample_scales": [4, 4, 4, 4]}, use_pitch_embed=False, use_nsf=False, sample_rate=22050)


def config(**kw):
    """The default configuration with fields replaced; upsample_scales=[...] is a shorthand for upsample_params."""
    cfg = default_config()
    if "upsample_scales" in kw:
        cfg["upsample_params"] = {"upsample_scales": list(kw.pop("upsample_scales"))}
    cfg.update(kw)
    return cfg


def scales_of(cfg):
    return [int(s) for s in cfg["upsample_params"]["upsample_scales"]]


def hop_of(cfg):
    return int(np.prod(scales_of(cfg)))


def dilation(cfg, layer):
    return 2 ** (layer % (cfg["layers"] // cfg["stacks"]))


def receptive_field(cfg):
    return (cfg["kernel_size"] - 1) * sum(dilation(cfg, l) for l in range(cfg["layers"])) + 1


def weight_shapes(cfg):
    w, out = cfg["aux_context_window"], OrderedDict()
    out["first_conv.weight"] = (RES, 1, 1)
    out["first_conv.bias"] = (RES,)
    out["upsample_net.conv_in.weight"] = (AUX, AUX, 2 * w + 1)
    for i, s in enumerate(scales_of(cfg)):
        out[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"] = (1, 1, 1, 2 * s + 1)
    for l in range(cfg["layers"]):
        p = f"conv_layers.{l}."
        out[p + "conv.weight"] = (GATE, RES, 3)
        out[p + "conv.bias"] = (GATE,)
        out[p + "conv1x1_aux.weight"] = (GATE, AUX, 1)
        out[p + "conv1x1_out.weight"] = (RES, GATE // 2, 1)
        out[p + "conv1x1_out.bias"] = (RES,)
        out[p + "conv1x1_skip.weight"] = (SKIP, GATE // 2, 1)
        out[p + "conv1x1_skip.bias"] = (SKIP,)
    out["last_conv_layers.1.weight"] = (SKIP, SKIP, 1)
    out["last_conv_layers.1.bias"] = (SKIP,)
    out["last_conv_layers.3.weight"] = (1, SKIP, 1)
    out["last_conv_layers.3.bias"] = (1,)
    return out


def _signed_unit(seed, uid, n):
    """n values in [-1, 1) from Philox words alone: (word - 2^31) / 2^31, exact in float64."""
    idx = np.arange((n + 3) // 4, dtype=np.uint64)
    w = np.stack(philox.words(seed, WEIGHT_STREAM, idx, uid), -1).reshape(-1)[:n]
    return (w.astype(np.float64) - 2147483648.0) / 2147483648.0


def make_weights(cfg, seed=1):
    """Weights of the size a trained network has: uniform with the variance of the He initialisation (amplitude sqrt(6 / fan_in)) for the
    convolutions, biases in +-0.1, and the up-sampler's taps at their initial 1 / (2 s + 1) times (1 + 0.5 u): all-equal taps would hide
    a wrong phase.  Every value is a float32 (rounded once from exact float64 arithmetic and one correctly rounded sqrt)."""
    out = OrderedDict()
    for uid, (name, shape) in enumerate(weight_shapes(cfg).items()):
        n = int(np.prod(shape))
        u = _signed_unit(seed, uid, n)
        if name.endswith(".bias"):
            v = 0.1 * u
        elif ".up_layers." in name:
            v = (1.0 + 0.5 * u) / float(n)
        else:
            v = math.sqrt(6.0 / float(np.prod(shape[1:]))) * u
        out[name] = v.reshape(shape).astype(np.float32)
    return out


def with_weight_norm(weights, seed=2):
    """The state dict before weight-norm removal: each convolution weight w becomes weight_v = w * r (r > 0 per output channel, from Philox
    words) and weight_g = |w|_2 per output channel, so that g v / |v| is w up to rounding.  The up-sampler's Conv2d carry it too."""
    out = OrderedDict()
    for uid, (name, w) in enumerate(weights.items()):
        if not name.endswith(".weight"):
            out[name] = w
            continue
        w64 = w.astype(np.float64)
        rows = w64.reshape(w64.shape[0], -1)
        r = 1.5 + 0.5 * _signed_unit(seed, uid, rows.shape[0])
        ones = (1,) * (w64.ndim - 1)
        out[name + "_g"] = np.sqrt((rows * rows).sum(1)).reshape((-1,) + ones).astype(np.float32)
        out[name + "_v"] = (w64 * r.reshape((-1,) + ones)).astype(np.float32)
    return out


def fold_weight_norm(state):
    """weight_g / weight_v pairs -> weight = g v / |v| in float64 (the norm over all but the first axis), rounded to float32."""
    out = OrderedDict()
    for name, v in state.items():
        if name.endswith(".weight_g"):
            continue
        if name.endswith(".weight_v"):
            v64, g64 = np.asarray(v, np.float64), np.asarray(state[name[:-2] + "_g"], np.float64)
            norm = np.sqrt((v64.reshape(v64.shape[0], -1) ** 2).sum(1)).reshape(g64.shape)
            out[name[:-2]] = (v64 * (g64 / norm)).astype(np.float32)
        else:
            out[name] = np.asarray(v)
    return out


def _t(weights, dtype, device):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in weights.items()}


def _upsample(u, W, cfg):
    """[B, C, n] at the frame rate -> [B, C, hop n]: per scale s a nearest stretch by s, then the 2 s + 1 taps with zero padding s."""
    B, C, _ = u.shape
    for i, s in enumerate(scales_of(cfg)):
        u = u.repeat_interleave(s, dim=-1)
        taps = W[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"].reshape(1, 1, 2 * s + 1)
        u = F.conv1d(u.reshape(B * C, 1, -1), taps, padding=s).reshape(B, C, -1)
    return u


def _stack(W, cfg, z, cond_of_layer):
    """first_conv, the residual blocks (cond_of_layer(l) -> [B, 128, L]) and the output layers."""
    x = z * W["first_conv.weight"].reshape(1, RES, 1) + W["first_conv.bias"].reshape(1, RES, 1)
    skips = None
    for l in range(cfg["layers"]):
        p, d = f"conv_layers.{l}.", dilation(cfg, l)
        g = F.conv1d(x, W[p + "conv.weight"], W[p + "conv.bias"], padding=d, dilation=d) + cond_of_layer(l)
        h = torch.tanh(g[:, :GATE // 2]) * torch.sigmoid(g[:, GATE // 2:])
        s = F.conv1d(h, W[p + "conv1x1_skip.weight"], W[p + "conv1x1_skip.bias"])
        skips = s if skips is None else skips + s
        x = (F.conv1d(h, W[p + "conv1x1_out.weight"], W[p + "conv1x1_out.bias"]) + x) * math.sqrt(0.5)
    y = torch.relu(skips * math.sqrt(1.0 / cfg["layers"]))
    y = torch.relu(F.conv1d(y, W["last_conv_layers.1.weight"], W["last_conv_layers.1.bias"]))
    return F.conv1d(y, W["last_conv_layers.3.weight"], W["last_conv_layers.3.bias"])


def _prepare(weights, z, c, dtype, device):
    W = weights if isinstance(next(iter(weights.values())), torch.Tensor) else _t(weights, dtype, device)
    z = torch.as_tensor(np.asarray(z) if not isinstance(z, torch.Tensor) else z, dtype=dtype, device=device)
    c = torch.as_tensor(np.asarray(c) if not isinstance(c, torch.Tensor) else c, dtype=dtype, device=device)
    if z.dim() == 2:
        z = z.unsqueeze(1)
    return W, z, c


def forward(weights, cfg, z, c, dtype=torch.float64, device="cpu"):
    """The direct form: conv_in, the up-sampling network on its 80 channels, every layer's own 128 x 80 projection at the sample rate."""
    W, z, c = _prepare(weights, z, c, dtype, device)
    with torch.no_grad():
        cu = _upsample(F.conv1d(c, W["upsample_net.conv_in.weight"]), W, cfg)
        assert cu.shape[-1] == z.shape[-1], (cu.shape, z.shape)
        return _stack(W, cfg, z, lambda l: F.conv1d(cu, W[f"conv_layers.{l}.conv1x1_aux.weight"]))


def forward_projected(weights, cfg, z, c, dtype=torch.float64, device="cpu"):
    """The device's form: G_l = W_aux_l conv_in(c) at the frame rate, up-sampled per layer (the up-sampler is linear and acts per channel
    along time, so it commutes with the projection, zero padding of every stage included)."""
    W, z, c = _prepare(weights, z, c, dtype, device)
    with torch.no_grad():
        ci = F.conv1d(c, W["upsample_net.conv_in.weight"])
        return _stack(W, cfg, z, lambda l: _upsample(F.conv1d(ci, W[f"conv_layers.{l}.conv1x1_aux.weight"]), W, cfg))


def pad_mel(mel, w, mean=None, scale=None):
    """mel [B, 80, T] (numpy) -> the padded c [B, 80, T + 2 w]: the optional (mel - mean) / scale per channel, then edge replication."""
    c = np.asarray(mel, np.float64)
    if mean is not None:
        c = (c - np.asarray(mean, np.float64).reshape(1, -1, 1)) / np.asarray(scale, np.float64).reshape(1, -1, 1)
    return np.pad(c, ((0, 0), (0, 0), (w, w)), mode="edge")


def draw_z(seed, ids, L):
    """float64 [B, L]: sample t of item b is component t & 3 of the generator's float4 t >> 2 on stream word PHILOX_STREAM, id ids[b]."""
    n4 = (int(L) + 3) // 4
    return np.stack([philox.normal4_f64(seed, PHILOX_STREAM, np.arange(n4, dtype=np.uint64), int(i)).reshape(-1)[:L] for i in ids])


def synth_mel(seed, B, T):
    """A mel-like [B, 80, T] float32 from Philox words: log-magnitudes in [-4, 1], smooth along neither axis (a harder input than speech)."""
    u = _signed_unit(seed, 0xC0FFEE, B * AUX * T).reshape(B, AUX, T)
    return (2.5 * u - 1.5).astype(np.float32)
