"""gen_pwg_reference.py -- writes tests/golden/pwg_reference.npz, pwg_reference_net.npz and pwg_reference_net_removed.npz: what the reference's own Parallel WaveGAN
generator (modules/parallel_wavegan/models/parallel_wavegan.py: ParallelWaveGANGenerator) computes, executed on the CPU, not restated.

    python tools/gen_pwg_reference.py --reference /path/to/the/reference/checkout

The reference's utils/__init__ imports chardet, which this project does not need: `utils` and `utils.hparams` get stand-ins here (the
generator reads nothing from hparams).  Not run by the tests; tests/test_pwg_host.py and tests/test_pwg.py read the fixtures.

pwg_reference.npz, per case NAME (tests/pwg_ref.py: make_weights(config, seed) gives the weights, so they are not stored):
    NAME/config     the constructor's kwargs as JSON          NAME/seed      of make_weights
    NAME/c          the padded conditioning [B, 80, T + 2 w]  NAME/z         the noise [B, 1, hop T]   (float32 values)
    NAME/mel, NAME/mean, NAME/scale   where the case has a scaler: c = pad((mel - mean) / scale), as PWG.spec2wav forms it
    NAME/out        the reference module's float64 output [B, 1, hop T]
    NAME/e32        [B]: per item the max abs distance of the reference module's own float32 run from that output
pwg_reference_net.npz is the state dict, BEFORE weight-norm removal, of one small network built by the reference's own constructor (layers
4, stacks 2, aux_context_window 1); pwg_reference_net_removed.npz holds its weights/NAME after the reference's remove_weight_norm, and
config, c, z, out, e32 of one run of it (two files: each stays below the size limit of a committed file).
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import pwg_ref   # noqa: E402

DEFAULT_FRAMES = (1, 2, 3, 4, 5)


def load_reference(root):
    utils = types.ModuleType("utils")
    utils.__path__ = []
    hp = types.ModuleType("utils.hparams")
    hp.hparams = {}
    utils.hparams = hp
    sys.modules["utils"], sys.modules["utils.hparams"] = utils, hp
    sys.path.insert(0, root)
    from modules.parallel_wavegan.models import ParallelWaveGANGenerator
    return ParallelWaveGANGenerator


def run_both(model, z, c):
    """-> (the float64 output, per item the max abs distance of the float32 run from it)"""
    model = model.eval()
    with torch.no_grad():
        y32 = model.float()(torch.from_numpy(z).float(), torch.from_numpy(c).float()).double().numpy()
        y64 = model.double()(torch.from_numpy(z).double(), torch.from_numpy(c).double()).numpy()
    return y64, np.abs(y32 - y64).reshape(y64.shape[0], -1).max(1)


def inputs(cfg, seed, B, T):
    w, hop = cfg["aux_context_window"], pwg_ref.hop_of(cfg)
    mel = pwg_ref.synth_mel(seed, B, T)
    z = pwg_ref.draw_z(seed, range(100, 100 + B), hop * T).astype(np.float32).reshape(B, 1, hop * T)
    return mel, z, w


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the directory that holds modules/parallel_wavegan)")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    args = ap.parse_args(argv)
    Gen = load_reference(args.reference)
    torch.set_num_threads(8)
    out = {}

    cases = [(f"default_T{T}", pwg_ref.config(), 10 + T, 3, T, False) for T in DEFAULT_FRAMES]
    cases += [("l6s2", pwg_ref.config(layers=6, stacks=2), 21, 2, 3, False),
              ("l6s3", pwg_ref.config(layers=6, stacks=3), 22, 2, 3, False),
              ("w0", pwg_ref.config(layers=6, stacks=2, aux_context_window=0), 23, 2, 3, False),
              ("w4", pwg_ref.config(layers=6, stacks=2, aux_context_window=4), 24, 2, 3, True),
              ("s884", pwg_ref.config(layers=6, stacks=3, upsample_scales=[8, 8, 4]), 25, 2, 3, False),
              ("s2816", pwg_ref.config(layers=6, stacks=2, upsample_scales=[2, 8, 16]), 26, 2, 3, True),
              ("scaler", pwg_ref.config(), 27, 2, 2, True)]
    for name, cfg, seed, B, T, scaler in cases:
        weights = pwg_ref.make_weights(cfg, seed)
        kw = copy.deepcopy(cfg)
        kw["use_weight_norm"] = False
        model = Gen(**kw)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
        mel, z, w = inputs(cfg, seed, B, T)
        if scaler:
            u = pwg_ref._signed_unit(seed, 0x5CA1E, 160)
            mean, scale = (-1.5 + 0.5 * u[:80]).astype(np.float32), (1.25 + 0.75 * u[80:]).astype(np.float32)
            out[f"{name}/mel"], out[f"{name}/mean"], out[f"{name}/scale"] = mel, mean, scale
            c = pwg_ref.pad_mel(mel, w, mean, scale).astype(np.float32)
        else:
            c = pwg_ref.pad_mel(mel, w).astype(np.float32)
        y64, e32 = run_both(model, z, c)
        out[f"{name}/config"], out[f"{name}/seed"] = np.array(json.dumps(cfg)), np.int64(seed)
        out[f"{name}/c"], out[f"{name}/z"], out[f"{name}/out"], out[f"{name}/e32"] = c, z, y64, e32
        print(f"{name}: B {B} T {T} max |out| {np.abs(y64).max():.3f} e32 {e32.max():.3g}")

    # one small network from the reference's own constructor, with weight norm
    cfg = pwg_ref.config(layers=4, stacks=2, aux_context_window=1)
    torch.manual_seed(0)
    model = Gen(**copy.deepcopy(cfg))
    with torch.no_grad():
        for uid, (n, p) in enumerate(model.named_parameters()):
            u = torch.from_numpy(pwg_ref._signed_unit(3, uid, p.numel()).reshape(tuple(p.shape))).float()
            if n.endswith("bias"):
                p.copy_(0.1 * u)
            elif n.endswith("weight_g"):
                p.mul_(1.0 + 0.25 * u)
            elif ".up_layers." in n:
                p.mul_(1.0 + 0.5 * u)
    before = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    model.remove_weight_norm()
    mel, z, w = inputs(cfg, 31, 2, 3)
    c = pwg_ref.pad_mel(mel, w).astype(np.float32)
    after = {f"weights/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}
    y64, e32 = run_both(model, z, c)
    after["config"], after["c"], after["z"], after["out"], after["e32"] = np.array(json.dumps(cfg)), c, z, y64, e32
    print(f"net: max |out| {np.abs(y64).max():.3f} e32 {e32.max():.3g}")

    for fn, d in (("pwg_reference.npz", out), ("pwg_reference_net.npz", before), ("pwg_reference_net_removed.npz", after)):
        path = os.path.normpath(os.path.join(args.out, fn))
        np.savez_compressed(path, **d)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
