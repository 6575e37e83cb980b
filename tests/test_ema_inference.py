"""Inference from another weight source (FastDiff.use_weights, Validator(weights=...)) -- the averaged weights of a TrainStep run.

One sequence, run once (the `story` fixture): a module is committed through the host, trained for three steps with ema_decay = 0.5, and
then asked for its weight image, a forward and a validation pass from the average and from the live parameters in turn.  The
references are modules that received the same tensors through the host: `from_ema` by ParamEMA.copy_to, `from_live` by load_state_dict.
Both sides are deterministic (tests/test_weight_refresh.py), so every comparison is byte for byte.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import synth    # noqa: E402

import fastdiff_amd                                    # noqa: E402
from fastdiff_amd import TrainCorpus, schedules       # noqa: E402

HOP, F, B = 256, 7, 3
STEPS = 3


def model_corpus(lengths, frames):
    """The smallest corpus and window tests/test_validation.py runs the model on."""
    mel = synth.synth_mel(3, 1, sum(lengths))[0].T
    gen = torch.Generator().manual_seed(11)
    items, at = [], 0
    for T in lengths:
        items.append({"mel": np.ascontiguousarray(mel[at: at + T]), "wav": (0.3 * torch.randn(T * HOP, generator=gen)).numpy()})
        at += T
    return TrainCorpus(items, hop_size=HOP, max_samples=frames * HOP, device="cpu")


def same(a, b):
    """Two result() dictionaries, bit for bit (NaN of an empty bin included)."""
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def trained(gc, dh, mel, wav, steps):
    m = gc.make_model()
    with torch.no_grad():
        m((wav, mel, torch.tensor([[37.0], [512.0]], device="cuda")))      # the handle's first weights go through the host
    assert m.last_refresh.startswith("host")
    m.train()
    ts = fastdiff_amd.TrainStep(m, dh, lr=1e-2, seed=7, graph=False, ema_decay=0.5)
    for _ in range(steps):
        ts.step(mel, wav)
    return m, ts


@pytest.fixture(scope="module")
def story():
    import gpu_common as gc
    dh = schedules.training_hyperparams()
    mel = torch.from_numpy(synth.synth_mel(3, 2, 6)).cuda()
    wav = (0.3 * gc.hash_normal_torch(3, 1, 2 * 6 * HOP)).view(2, 1, 6 * HOP)
    audio = 0.5 * gc.hash_normal_torch(5, 9, 2 * 6 * HOP).view(2, 1, 6 * HOP)
    steps = torch.tensor([[37.0], [512.0]], device="cuda")
    held_out = model_corpus([8, 19, 9, 12], F).to("cuda")
    s = {"dh": dh, "mel": mel, "wav": wav, "held_out": held_out}

    def forward(net):
        was = net.training
        net.eval()
        with torch.no_grad():
            y = net((audio, mel, steps)).clone()
        net.train(was)
        return y

    m, ts = trained(gc, dh, mel, wav, STEPS)
    assert ts.state()["applied"] == STEPS and ts.ema.state()["updates"] == STEPS
    s["m"], s["ts"] = m, ts
    # the references, through the host
    from_ema = gc.make_model()
    ts.ema.copy_to(from_ema)
    s["ema_forward"] = forward(from_ema)
    s["ema_image"], s["from_ema_refresh"] = from_ema.weight_image(), from_ema.last_refresh
    s["ema_pass"] = fastdiff_amd.Validator(from_ema, dh, corpus=held_out, batch_size=B).run().result()
    from_live = fastdiff_amd.FastDiff()
    from_live.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    from_live = from_live.cuda().eval()
    s["live_forward"] = forward(from_live)
    s["live_image"] = from_live.weight_image()
    s["live_pass"] = fastdiff_amd.Validator(from_live, dh, corpus=held_out, batch_size=B).run().result()
    s["forward"] = forward
    return s


@pytest.mark.gpu
def test_the_image_follows_the_source(story):
    m, ts = story["m"], story["ts"]
    assert not np.array_equal(story["ema_image"], story["live_image"]), "lr = 1e-2, decay 0.5: the average lags the parameters"
    assert story["from_ema_refresh"].startswith("host")
    assert m.use_weights(ts.ema) is None and m.weights_source is ts.ema
    y = story["forward"](m)
    assert m.last_refresh.startswith("device") and "ParamEMA" in m.last_refresh, m.last_refresh
    assert np.array_equal(m.weight_image(), story["ema_image"])
    assert torch.equal(bits(y), bits(story["ema_forward"]))
    # back to the live parameters
    assert m.use_weights(None) is ts.ema
    y = story["forward"](m)
    assert m.last_refresh == "device", m.last_refresh
    assert np.array_equal(m.weight_image(), story["live_image"])
    assert torch.equal(bits(y), bits(story["live_forward"]))
    # a plain mapping of device tensors is a source as well
    m.use_weights({k: v.clone() for k, v in ts.ema.tensors.items()})
    story["forward"](m)
    assert m.last_refresh.startswith("device") and np.array_equal(m.weight_image(), story["ema_image"])
    m.use_weights(None)
    # the differentiable forward reads the live parameters whatever the source is
    m.use_weights(ts.ema)
    x = (story["wav"], story["mel"], torch.tensor([[37.0], [512.0]], device="cuda"))
    with_source = m(x).detach().clone()
    m.use_weights(None)
    assert m.training and torch.equal(bits(with_source), bits(m(x).detach()))
    m.zero_grad(set_to_none=True)


@pytest.mark.gpu
def test_a_validation_pass_from_the_average(story):
    m, ts, dh, held_out = story["m"], story["ts"], story["dh"], story["held_out"]
    val = fastdiff_amd.Validator(m, dh, corpus=held_out, batch_size=B, weights=ts.ema)
    assert m.weights_source is None, "the constructor only checks the source"
    got = val.run().result()
    assert m.training and m.weights_source is None and m._weights_dirty
    assert got["items"] == 4 and got["nonfinite"] == 0 and math.isfinite(got["loss"])
    first = next((k for k in got if np.asarray(got[k]).tobytes() != np.asarray(story["ema_pass"][k]).tobytes()), None)
    assert first is None, (first, got[first], story["ema_pass"][first])
    assert np.array_equal(got["item_loss"], story["ema_pass"]["item_loss"])
    live = fastdiff_amd.Validator(m, dh, corpus=held_out, batch_size=B).run().result()
    assert same(live, story["live_pass"])
    assert not np.array_equal(got["item_loss"], live["item_loss"]) and got["loss"] != live["loss"]
    assert np.array_equal(got["count_by_t"], live["count_by_t"]), "the draws are the same: only the weights differ"
    # after a pass from the average the module is back on its own source, and its next forward is the live weights'
    val.run()
    y = story["forward"](m)
    assert m.weights_source is None and m.last_refresh == "device"
    assert torch.equal(bits(y), bits(story["live_forward"]))
    # a pass hands back whatever source the module had
    m.use_weights(ts.ema)
    fastdiff_amd.Validator(m, dh, corpus=held_out, batch_size=B, weights={k: v for k, v in m.state_dict().items()}).run()
    assert m.weights_source is ts.ema
    m.use_weights(None)
    with pytest.raises(ValueError, match="names"):
        fastdiff_amd.Validator(m, dh, corpus=held_out, batch_size=B, weights={"fc_t1.bias": torch.zeros(512, device="cuda")})


@pytest.mark.gpu
def test_training_goes_on_as_if_never_validated(story):
    """(runs after the passes above) one more step on the module that validated from the average equals the fourth step of a run
    that never did; and the module then repacks from the moved shadow while the average is its source."""
    import gpu_common as gc
    m, ts = story["m"], story["ts"]
    m.use_weights(ts.ema)
    ts.step(story["mel"], story["wav"])
    assert m._weights_dirty
    other, ts_other = trained(gc, story["dh"], story["mel"], story["wav"], STEPS + 1)
    torch.cuda.synchronize()
    assert ts.state()["applied"] == ts_other.state()["applied"] == STEPS + 1
    for (k, a), b in zip(m.state_dict().items(), other.state_dict().values()):
        assert torch.equal(bits(a), bits(b)), k
    for (k, a), b in zip(ts.ema.tensors.items(), ts_other.ema.tensors.values()):
        assert torch.equal(bits(a), bits(b)), k
    story["forward"](m)
    assert m.last_refresh.startswith("device") and "ParamEMA" in m.last_refresh
    moved = m.weight_image()
    assert not np.array_equal(moved, story["ema_image"])
    ref = gc.make_model()
    ts_other.ema.copy_to(ref)
    story["forward"](ref)
    assert np.array_equal(moved, ref.weight_image())
    m.use_weights(None)
