"""Parallel WaveGAN, the host side (no GPU): the float64 restatement tests/pwg_ref.py against what the executed reference computed
(tests/golden/pwg_reference*.npz, tools/gen_pwg_reference.py), the identity the device path rests on, the loader's weight-norm folding,
the configuration's refusals and the pure-host entry points.
"""
import ctypes as ct
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

from fastdiff_amd import _capi, pwg
import pwg_ref as ref

GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixtures():
    fx = np.load(os.path.join(GOLDEN, "pwg_reference.npz"))
    return fx, sorted({k.split("/")[0] for k in fx.files})


def case_of(fx, name):
    cfg = json.loads(str(fx[name + "/config"]))
    return cfg, ref.make_weights(cfg, int(fx[name + "/seed"]))


def test_weight_recipe_bits_are_pinned():
    """make_weights uses Philox words, exact float64 arithmetic and one correctly rounded sqrt per tensor: its bytes are the same under
    every library version, which is why the default architecture's 1.33 M parameters are not stored."""
    W = ref.make_weights(ref.default_config(), 11)
    assert sum(v.size for v in W.values()) == 1334309
    h = hashlib.sha256()
    for k, v in W.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, "<f4").tobytes())
    assert h.hexdigest() == PINNED_SHA256
    taps = W["upsample_net.upsample.up_layers.1.weight"].reshape(-1)
    assert len(set(taps.tolist())) == taps.size, "all-equal taps would hide a wrong phase"


PINNED_SHA256 = "11abdfecf130b43d349334a86fc0d441a0cb96e280c453b83db5be467e54ac0c"


def test_restatement_equals_every_fixture():
    fx, names = fixtures()
    assert len(names) == 12
    for name in names:
        cfg, W = case_of(fx, name)
        out = ref.forward(W, cfg, fx[name + "/z"], fx[name + "/c"]).numpy()
        err = float(np.abs(out - fx[name + "/out"]).max())
        print(f"{name}: max abs distance from the executed reference {err:.3g}, e32 {fx[name + '/e32'].max():.3g}")
        assert out.shape == fx[name + "/out"].shape and err <= 1e-12, (name, err)
        if name + "/mel" in fx.files:           # the scaler and the edge replication, as PWG.spec2wav forms c
            c = ref.pad_mel(fx[name + "/mel"], cfg["aux_context_window"], fx[name + "/mean"], fx[name + "/scale"]).astype(np.float32)
            assert np.array_equal(c, fx[name + "/c"]), name


def test_projected_form_equals_direct_form():
    """conv1x1_aux(upsample(conv_in(c))) == upsample(conv1x1_aux(conv_in(c))), the zero padding of every stage included: looked at over
    the whole output and, by themselves, over the first and the last two frames, where the padding acts."""
    fx, names = fixtures()
    for name in names:
        cfg, W = case_of(fx, name)
        a = ref.forward(W, cfg, fx[name + "/z"], fx[name + "/c"]).numpy()
        b = ref.forward_projected(W, cfg, fx[name + "/z"], fx[name + "/c"]).numpy()
        hop = ref.hop_of(cfg)
        edge = min(2 * hop, a.shape[-1])
        for what, sl in (("all", slice(None)), ("first two frames", slice(0, edge)), ("last two frames", slice(a.shape[-1] - edge, None))):
            err = float(np.abs(a[..., sl] - b[..., sl]).max())
            assert err <= 1e-12, (name, what, err)


def test_weight_norm_folding_reproduces_the_stored_network():
    before = dict(np.load(os.path.join(GOLDEN, "pwg_reference_net.npz")))
    after = np.load(os.path.join(GOLDEN, "pwg_reference_net_removed.npz"))
    cfg = json.loads(str(after["config"]))
    assert any(k.endswith(".weight_g") for k in before) and not any(k.endswith(".weight") for k in before)
    for wrap in (lambda s: s, lambda s: {"models": {"generator": s}}, lambda s: {"state_dict": {"model_gen": s, "model_disc": {}}}):
        state, official = pwg.unwrap_checkpoint(wrap({k: torch.from_numpy(v) for k, v in before.items()}))
        folded = pwg.fold_weight_norm(state)
        assert sorted(folded) == sorted(ref.weight_shapes(cfg)) == sorted(k[len("weights/"):] for k in after.files if k.startswith("weights/"))
        for k, v in folded.items():
            want = after["weights/" + k]
            assert v.dtype == np.float32 and v.shape == want.shape == tuple(ref.weight_shapes(cfg)[k]), k
            # the reference folds in float32 (g * v / |v|, three roundings), this loader in float64 rounded once: a few ulp of the largest
            assert float(np.abs(v - want).max()) <= 4 * 2.0 ** -24 * float(np.abs(want).max()), k
    assert pwg.unwrap_checkpoint({"models": {"generator": {}}})[1] and not official
    out = ref.forward(folded, cfg, after["z"], after["c"]).numpy()
    err, e32 = np.abs(out - after["out"]).reshape(out.shape[0], -1).max(1), after["e32"]
    print(f"folded network against the reference's float64 run: {err.max():.3g}, e32 {e32.max():.3g}, ratio {float((err / e32).max()):.2f}")
    assert (err <= 10 * e32).all()       # weights a float32 rounding apart: the distance of a float32 run, with the margin of the parity tests
    assert np.array_equal(ref.fold_weight_norm(before)["first_conv.weight"], folded["first_conv.weight"])


def _struct(**kw):
    return pwg.config_struct(**kw)[0]


REFUSED = [
    (dict(use_causal_conv=True), "use_causal_conv = 1"), (dict(use_pitch_embed=True), "use_pitch_embed = 1"), (dict(use_nsf=True), "use_nsf = 1"),
    (dict(upsample_net="MelGANGenerator", aux_context_window=0), "upsample_net = 2"), (dict(upsample_net="UpsampleNetwork"), "upsample_net = 1"),
    (dict(upsample_params={"upsample_scales": [4, 4, 4, 4], "nonlinear_activation": "ReLU"}), "upsample_activation = 1"),
    (dict(upsample_params={"upsample_scales": [4, 4, 4, 4], "interpolate_mode": "linear"}), "interpolate_mode = 'linear'"),
    (dict(upsample_params={"upsample_scales": [4, 4, 4, 4], "freq_axis_kernel_size": 3}), "freq_axis_kernel_size = 3"),
    (dict(upsample_conditional_features=False), "upsample_conditional_features = 0"),
    (dict(residual_channels=32), "residual_channels = 32"), (dict(gate_channels=64), "gate_channels = 64"), (dict(skip_channels=128), "skip_channels = 128"),
    (dict(aux_channels=40), "aux_channels = 40"), (dict(kernel_size=5), "kernel_size = 5"), (dict(in_channels=2), "in_channels = 2"),
    (dict(out_channels=2), "out_channels = 2"), (dict(bias=False), "bias = 0"),
    (dict(layers=0), "layers = 0"), (dict(layers=31, stacks=1), "layers = 31"), (dict(layers=30, stacks=4), "stacks = 4"),
    (dict(layers=22, stacks=2), "stacks = 2 with layers = 22: dilation 1024"), (dict(aux_context_window=5), "aux_context_window = 5"),
    (dict(aux_context_window=-1), "aux_context_window = -1"),
    (dict(upsample_params={"upsample_scales": []}), "0 scales"), (dict(upsample_params={"upsample_scales": [2] * 5}), "5 scales"),
    (dict(upsample_params={"upsample_scales": [4, 1, 4]}), "upsample_scales[1] = 1"), (dict(upsample_params={"upsample_scales": [17, 4]}), "upsample_scales[0] = 17"),
    (dict(upsample_params={"upsample_scales": [16, 16, 4]}), "hop = 1024"),
]


@pytest.mark.parametrize("kw,text", REFUSED, ids=[t for _, t in REFUSED])
def test_what_is_not_built_is_refused_with_the_field_named(kw, text):
    with pytest.raises(NotImplementedError, match="ParallelWaveGAN|fd_pwg_create") as e:
        pwg.ParallelWaveGAN(**kw)
    assert text in str(e.value), str(e.value)
    with pytest.raises(NotImplementedError):
        pwg.samples(1, **kw)


def test_constructor_arguments():
    with pytest.raises(TypeError, match="diffusion_step_embed_dim_in"):
        pwg.ParallelWaveGAN(diffusion_step_embed_dim_in=128)       # ParallelWaveGANGenerator_Diffusion is not this class
    with pytest.raises(ValueError, match="contradicts"):
        pwg.config_struct(upsample_params={"upsample_scales": [4, 4], "aux_context_window": 0})
    # what the reference's constructor writes into upsample_params itself is accepted
    c = _struct(upsample_params={"upsample_scales": [8, 8, 4], "use_causal_conv": False, "aux_channels": 80, "aux_context_window": 2}, dropout=0.1)
    assert [c.upsample_scales[i] for i in range(c.n_scales)] == [8, 8, 4] and ct.sizeof(c) == 112
    d = _capi.FdPwgConfig()
    _capi.load().fd_pwg_default_config(ct.byref(d))
    assert bytes(d) == bytes(_struct())


def test_samples_and_receptive_field():
    lib = _capi.load()
    assert pwg.receptive_field() == ref.receptive_field(ref.default_config()) == 6139
    for kw in (dict(layers=6, stacks=2), dict(layers=6, stacks=3), dict(layers=10, stacks=1), dict(layers=1, stacks=1)):
        assert pwg.receptive_field(**kw) == ref.receptive_field(ref.config(**kw)) == 2 * sum(ref.dilation(ref.config(**kw), l) for l in range(kw["layers"])) + 1
    assert pwg.samples(0) == 0 and pwg.samples(864) == 864 * 256
    assert pwg.samples(3, upsample_params={"upsample_scales": [2, 8, 16]}) == 768 and pwg.samples(3, upsample_params={"upsample_scales": [3, 5]}) == 45
    c = _struct()
    assert lib.fd_pwg_samples(ct.byref(c), -1) == -1 and lib.fd_pwg_samples(None, 1) == -1 and lib.fd_pwg_receptive_field(None) == -1
    bad = _struct(layers=31, stacks=1)
    assert lib.fd_pwg_samples(ct.byref(bad), 1) == -1 and lib.fd_pwg_receptive_field(ct.byref(bad)) == -1


def test_arguments_are_refused_before_a_handle_is_looked_at():
    lib = _capi.load()
    out = ct.c_void_p()
    assert lib.fd_pwg_create(None, None, ct.byref(out)) == _capi.FD_ERR_INVALID and b"null cfg" in lib.fd_last_error(None)
    c = _struct()
    assert lib.fd_pwg_create(None, ct.byref(c), ct.byref(out)) == _capi.FD_ERR_INVALID and b"null handle" in lib.fd_last_error(None)
    some = ct.cast(256, ct.POINTER(ct.c_float))             # (an address that is never read: every call below is refused first)
    args = lambda **kw: [kw.get("p"), kw.get("mel", some), kw.get("padded", 0), kw.get("B", 1), kw.get("T", 4), None, None, 0, None, kw.get("wav", some), 1024, None]  # noqa: E731
    for kw, text in ((dict(mel=None), b"null mel_or_c"), (dict(wav=None), b"null wav_out"), (dict(padded=2), b"padded = 2"), (dict(B=0), b"B = 0"),
                     (dict(B=4097), b"B = 4097"), (dict(T=0), b"T = 0"), (dict(T=32769), b"T = 32769"), (dict(), b"null generator")):
        assert lib.fd_pwg_generate(*args(**kw)) == _capi.FD_ERR_INVALID
        assert text in lib.fd_last_error(None), (kw, lib.fd_last_error(None))
    lens = (ct.c_int64 * 1)(5)
    a = args()
    a[5] = lens
    assert lib.fd_pwg_generate(*a) == _capi.FD_ERR_INVALID and b"lens[0] = 5" in lib.fd_last_error(None)
    assert lib.fd_pwg_draw(None, 1, 0, 0, None, some, 0, None) == _capi.FD_ERR_INVALID and b"L = 0" in lib.fd_last_error(None)
    assert lib.fd_pwg_set_weight(None, b"x", some, 1) == _capi.FD_ERR_INVALID and lib.fd_pwg_commit(None) == _capi.FD_ERR_INVALID
    assert lib.fd_pwg_destroy(None) == _capi.FD_OK


def test_constants_follow_the_header():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    for name in ("FD_PWG_TILE", "FD_PWG_MAX_LAYERS", "FD_PWG_MAX_DILATION", "FD_PWG_MAX_CONTEXT", "FD_PWG_MAX_SCALES", "FD_PWG_MAX_SCALE", "FD_PWG_MAX_HOP",
                 "FD_PWG_MAX_FRAMES"):
        assert f"#define {name} {getattr(_capi, name)} " in header or f"#define {name} {getattr(_capi, name)}\n" in header, name
    assert "#define FD_PWG_PHILOX_STREAM 0xFFFFFFF7u" in header and _capi.FD_PWG_PHILOX_STREAM == ref.PHILOX_STREAM == 0xFFFFFFF7
    assert "0xFFFFFFF7" in open(os.path.join(ROOT, "DESIGN.md")).read(), "the stream word is documented next to the others"
    assert _capi.FD_PWG_TILE % 256 == 0 and _capi.FD_PWG_TILE // 256 - 1 >= 1


def test_stats_files(tmp_path):
    mean, scale = np.arange(80, dtype=np.float32), 1.0 + np.arange(80, dtype=np.float32)
    np.save(tmp_path / "stats.npy", np.stack([mean, scale]))
    m, s = pwg.read_stats(str(tmp_path / "stats.npy"))
    assert np.array_equal(m, mean) and np.array_equal(s, scale)
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            pwg.read_stats(str(tmp_path / "stats.h5"))
    with pytest.raises(ValueError, match="only .npy and .h5"):
        pwg.read_stats(str(tmp_path / "stats.txt"))
