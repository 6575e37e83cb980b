"""Parallel WaveGAN on the device (fd_pwg_generate, fastdiff_amd/pwg.py) against the executed reference's float64 output
(tests/golden/pwg_reference.npz; weights from tests/pwg_ref.py: make_weights), and the properties of a batched call.

The parity bar: per item the max abs error against the reference's float64 output is at most 10 times that item's e32, the distance
of the reference's own float32 run from the same output (0.9e-6 .. 1.8e-6 on outputs of order 1): the margin the Griffin-Lim and NNLS
tests give a float32 emulation.  Every test prints the ratio.  Measured on an MI355X: the largest ratio is 1.45 over the default architecture (B = 3, 2 frames) and
1.66 over the other configurations (aux_context_window 4).

The z the device draws: its position and key are pinned bit for bit -- a call with z = None equals, bit for bit, the call given the
output of fd_pwg_draw, alone and inside a batch -- and fd_pwg_draw's values are held to the host twin (oracle/philox.py, float64
Box-Muller on the same float32 uniforms) within the N_ULP of tests/test_device_noise.py: logf, sqrtf and sincosf of the device have no
bit-exact host restatement.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

from fastdiff_amd import _capi, pwg
import guarded
import pwg_ref as ref

GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE_FRAMES = _capi.FD_PWG_TILE // 256
FRAMES = (1, 2, 3, 4, 5)
BAR = 10.0
N_ULP = 9                      # tests/test_device_noise.py: twice the worst distance measured over 12.6 M draws of the same generator


@functools.lru_cache(maxsize=None)
def fixture_file():
    return np.load(os.path.join(GOLDEN, "pwg_reference.npz"))


@functools.lru_cache(maxsize=16)
def network(cfg_json, seed):
    cfg = json.loads(cfg_json)
    return pwg.ParallelWaveGAN(**cfg).load_state_dict(ref.make_weights(cfg, seed))


def case(name):
    fx = fixture_file()
    cfg_json = str(fx[name + "/config"])
    d = {k.split("/", 1)[1]: fx[k] for k in fx.files if k.startswith(name + "/")}
    return json.loads(cfg_json), network(cfg_json, int(fx[name + "/seed"])), d


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ratios(got, d, items, tag):
    """per item: max abs error against the float64 fixture over its e32; printed, then held to the bar"""
    got = got.double().cpu().numpy().reshape(len(items), -1)
    want = d["out"].reshape(d["out"].shape[0], -1)[list(items)]
    err = np.abs(got - want).max(1)
    r = err / d["e32"][list(items)]
    print(f"{tag}: max abs error {err.max():.3g}, e32 {d['e32'][list(items)].max():.3g}, ratio {r.max():.2f} (bar {BAR:g})")
    assert np.isfinite(got).all() and (r <= BAR).all(), (tag, r.tolist())
    return float(r.max())


@pytest.mark.gpu
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("B", (1, 3))
def test_parity_default_architecture(B, T):
    """1 frame: every tap of dilation >= 256 lies outside the item; 2 frames equal the largest dilation; 3 and 5: a tile and one frame,
    two tiles and one frame."""
    assert {1, 2, 3, 4, 5, TILE_FRAMES - 1, TILE_FRAMES, TILE_FRAMES + 1, 2 * TILE_FRAMES + 1} == set(FRAMES)
    cfg, m, d = case(f"default_T{T}")
    items = range(B)
    y = m.forward(dev(d["z"][:B]), dev(d["c"][:B]))
    assert y.shape == (B, 1, 256 * T)
    ratios(y, d, items, f"forward B={B} T={T}")
    mel = d["c"][:B, :, 2:-2]                                   # (these cases have no scaler: c is the mel, edge padded)
    ratios(m.spec2wav(dev(mel), z=dev(d["z"][:B])), d, items, f"spec2wav B={B} T={T}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("l6s2", "l6s3", "w0", "w4", "s884", "s2816", "scaler"))
def test_parity_other_configurations(name):
    cfg, m, d = case(name)
    w, B = cfg["aux_context_window"], d["z"].shape[0]
    assert m.hop_size == ref.hop_of(cfg) and m.receptive_field_size == ref.receptive_field(cfg)
    ratios(m.forward(dev(d["z"]), dev(d["c"])), d, range(B), f"{name}: forward")
    if "mel" in d:                                              # with the scaler: the mel goes in, (mel - mean) / scale and the padding happen inside
        m.set_scaler(d["mean"], d["scale"])
        try:
            ratios(m.spec2wav(dev(d["mel"]), z=dev(d["z"])), d, range(B), f"{name}: spec2wav with the scaler")
            ratios(m.forward(dev(d["z"]), dev(d["c"])), d, range(B), f"{name}: forward with a scaler set (it does not apply to a padded c)")
        finally:
            m.set_scaler(None, None)
    else:
        mel = d["c"][:, :, w:d["c"].shape[-1] - w]
        ratios(m.spec2wav(dev(mel), z=dev(d["z"])), d, range(B), f"{name}: spec2wav")


def ragged_inputs(m, garbage):
    lens, T = [5, 1, 3], 5
    mel = ref.synth_mel(77, 3, T)
    z = ref.draw_z(5, [7, 8, 9], m.hop_size * T).astype(np.float32)
    if garbage is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = garbage
            z[b, m.hop_size * t:] = garbage
    return lens, T, mel, z


@pytest.mark.gpu
def test_ragged_batch_is_bit_identical_to_each_item_alone():
    cfg, m, _ = case("default_T5")
    lens, T, mel, z = ragged_inputs(m, float("nan"))
    L = m.hop_size * T
    out = torch.full((3, L + 1), float("nan"), device="cuda")           # rows at a pitch 4 bytes off alignment
    wav = m.spec2wav(dev(mel), lens=lens, z=dev(z), out=out)
    assert wav.data_ptr() == out.data_ptr() and torch.isnan(out[:, L]).all(), "the column behind the rows is not the call's"
    for b, t in enumerate(lens):
        alone = m.spec2wav(dev(mel[b:b + 1, :, :t]), z=dev(z[b:b + 1, :m.hop_size * t]))
        assert torch.isfinite(alone).all() and alone.abs().max() > 0.01
        assert torch.equal(out[b, :m.hop_size * t], alone[0]), b
        assert not out[b, m.hop_size * t:L].any(), "zeros from L_b to the row's end"
    # the padded c of forward(), ragged: item b's frames are its first lens[b] + 2 w columns
    c = np.full((3, 80, T + 4), np.nan, np.float32)
    for b, t in enumerate(lens):
        c[b, :, :t + 4] = ref.pad_mel(mel[b:b + 1, :, :t], 2)[0]
    again = m._generate(dev(c), True, lens, dev(z), 0, None)
    assert torch.equal(again, out[:, :L])


@pytest.mark.gpu
def test_device_drawn_z():
    cfg, m, _ = case("default_T5")
    lens, T, mel, _ = ragged_inputs(m, None)
    ids, seed, L = [2 ** 63 + 5, 1, 2 ** 32 + 3], 2 ** 40 + 17, m.hop_size * T
    batch = m.spec2wav(dev(mel), lens=lens, seed=seed, stream_ids=ids)
    zd = m.draw_z(3, L, seed, ids)
    for b, t in enumerate(lens):
        alone = m.spec2wav(dev(mel[b:b + 1, :, :t]), seed=seed, stream_ids=[ids[b]])
        assert torch.equal(batch[b, :m.hop_size * t], alone[0]), "an item's noise does not depend on the batch it sits in"
        given = m.spec2wav(dev(mel[b:b + 1, :, :t]), z=zd[b:b + 1, :m.hop_size * t].contiguous())
        assert torch.equal(alone, given), "a call without z draws exactly what fd_pwg_draw writes, halo included"
    assert not torch.equal(batch, m.spec2wav(dev(mel), lens=lens, seed=seed + 1, stream_ids=ids))
    # without ids the id is the item's position in the batch
    assert torch.equal(m.spec2wav(dev(mel), seed=seed), m.spec2wav(dev(mel), seed=seed, stream_ids=[0, 1, 2]))
    # the drawn values against the host twin
    twin = ref.draw_z(seed, ids, L)
    got = zd.double().cpu().numpy()
    err, unit = np.abs(got - twin), 2.0 ** -24 * np.abs(twin)
    worst = float(((err - 1e-9).clip(0) / unit).max())
    print(f"fd_pwg_draw against the host twin: {got.size} draws, worst {worst:.3f} x 2^-24 |twin|, std {got.std():.4f}")
    assert (err <= N_ULP * unit + 1e-9).all() and abs(got.std() - 1.0) < 0.05
    odd = m.draw_z(2, 1023, seed, ids[:2])                               # a row that ends inside a float4
    assert torch.equal(odd, zd[:2, :1023])


@pytest.mark.gpu
def test_graph_replay_equals_the_eager_call():
    cfg, m, d = case("l6s2")
    mel_a, mel_b = dev(ref.synth_mel(81, 2, 3)), dev(ref.synth_mel(82, 2, 3))
    want_a, want_b = m.spec2wav(mel_a, seed=3), m.spec2wav(mel_b, seed=3)      # (the eager calls also grow the scratch buffer)
    mel, out = mel_a.clone(), torch.zeros_like(want_a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.spec2wav(mel, seed=3, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    mel.copy_(mel_b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b) and not torch.equal(want_a, want_b)


@pytest.mark.gpu
def test_forward_equals_spec2wav():
    cfg, m, d = case("default_T3")
    mel, z = d["c"][:, :, 2:-2], dev(d["z"])
    assert np.array_equal(ref.pad_mel(mel, 2).astype(np.float32), d["c"])
    assert torch.equal(m.forward(z, dev(d["c"]))[:, 0], m.spec2wav(dev(mel), z=z))
    assert torch.equal(m(z, dev(d["c"])), m.forward(z, dev(d["c"])))


@pytest.mark.gpu
def test_guarded_memory_ragged_call():
    """No stray read or write, and every output sample is written (below L_b by the network, behind it with zeros): the call at a
    ragged shape in guarded memory, with two poisons and plain."""
    cfg, m, _ = case("default_T5")
    lens, T, mel, z = ragged_inputs(m, None)
    L = m.hop_size * T

    def fn(g, with_z):
        fill = 0.0 if g.fill is None else g.fill
        mel_g, z_g = mel.copy(), z.copy()
        for b, t in enumerate(lens):                                     # what lies behind an item's frames is the poison
            mel_g[b, :, t:] = fill
            z_g[b, m.hop_size * t:] = fill
        out = g.empty((3, L + 1), torch.float32)
        mel_t, z_t = g.tensor(torch.from_numpy(mel_g), 4), g.tensor(torch.from_numpy(z_g)) if with_z else None
        if g.fill is not None:                                           # (the entry point declares float pointers, which the harness does not look at)
            assert all(g._inside(t.data_ptr()) for t in (mel_t, z_t, out) if t is not None)
        m.spec2wav(mel_t, lens=lens, z=z_t, seed=9, stream_ids=[4, 5, 6], out=out)
        mask = torch.ones((3, L + 1), dtype=torch.bool)
        mask[:, L] = False
        return {"wav": out}, {"wav": mask}

    for with_z in (True, False):
        rep = guarded.run_case(functools.partial(fn, with_z=with_z), "cuda")
        assert rep.clean(), (with_z, rep.guard, rep.poison, rep.plain, rep.unguarded)
        assert rep.calls == {"fd_pwg_generate": 2}, rep.calls


@pytest.mark.gpu
def test_states_and_refusals_on_the_device():
    cfg = ref.config(layers=2, stacks=1)
    m = pwg.ParallelWaveGAN(**cfg)
    mel = dev(ref.synth_mel(1, 1, 2))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.spec2wav(mel)
    W = ref.make_weights(cfg, 1)
    with pytest.raises(KeyError, match="last_conv_layers.3.bias was never set"):
        m.load_state_dict({k: v for k, v in W.items() if k != "last_conv_layers.3.bias"})
    with pytest.raises(KeyError, match="conv_layers.2.conv.weight"):
        m.load_state_dict(dict(W, **{"conv_layers.2.conv.weight": W["conv_layers.1.conv.weight"]}))
    with pytest.raises(AssertionError, match="first_conv.bias has 64 elements, got 63"):
        m.load_state_dict(dict(W, **{"first_conv.bias": W["first_conv.bias"][:63]}))
    m.load_state_dict(W)
    want = ref.forward(W, cfg, ref.draw_z(1, [0], 512).astype(np.float32), ref.pad_mel(mel.cpu().numpy(), 2).astype(np.float32))
    got = m.spec2wav(mel, z=dev(ref.draw_z(1, [0], 512)))
    assert float((got.double().cpu() - want[:, 0]).abs().max()) < 1e-5
    with pytest.raises(AssertionError, match="wav_pitch = 100"):
        m.spec2wav(mel, out=torch.empty((1, 100), device="cuda"))
    with pytest.raises(AssertionError, match=r"lens\[0\] = 3"):
        m.spec2wav(mel, lens=[3])
    with pytest.raises(AssertionError, match="scale 0"):
        m.set_scaler(np.zeros(80), np.zeros(80))


def write_dir(path, cfg, state, official, stats=None):
    import yaml
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.yaml"), "w") as f:
        yaml.safe_dump({"generator_params": cfg, "hop_size": ref.hop_of(cfg), "format": "npy"}, f)
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    for steps in (1000, 20000, 3000):                                     # the newest by its number, not by its name's order
        blob = {"models": {"generator": state}} if official else {"state_dict": {"model_gen": state}}
        if steps != 20000:
            blob = {"models": {"generator": {}}} if official else {"state_dict": {"model_gen": {}}}
        torch.save(blob, os.path.join(path, f"checkpoint-{steps}steps.pkl" if official else f"model_ckpt_steps_{steps}.ckpt"))
    if stats is not None:
        np.save(os.path.join(path, "stats.npy"), np.stack(stats))


@pytest.mark.gpu
def test_from_dir_reads_both_checkpoint_formats(tmp_path):
    cfg, m, d = case("scaler")
    W = ref.make_weights(cfg, int(d["seed"]))
    write_dir(str(tmp_path / "own"), cfg, ref.with_weight_norm(W), False)
    write_dir(str(tmp_path / "official"), cfg, ref.with_weight_norm(W), True, (d["mean"], d["scale"]))
    own, official = pwg.ParallelWaveGAN.from_dir(str(tmp_path / "own")), pwg.ParallelWaveGAN.from_dir(str(tmp_path / "official"))
    assert own.scaler is None and np.array_equal(official.scaler[0], d["mean"])
    # (weights folded from g and v are a float32 rounding away from W: the bar of the parity tests holds for them too)
    ratios(official.spec2wav(dev(d["mel"]), z=dev(d["z"])), d, range(2), "from_dir, official checkpoint with stats.npy")
    ratios(own.forward(dev(d["z"]), dev(d["c"])), d, range(2), "from_dir, the reference's own checkpoint")
    with pytest.raises(FileNotFoundError):
        os.makedirs(tmp_path / "empty")
        open(tmp_path / "empty" / "config.yaml", "w").write("generator_params: {}\n")
        pwg.ParallelWaveGAN.from_dir(str(tmp_path / "empty"))


@pytest.fixture(scope="module")
def job():
    """infer.synthesize_pwg's two models and a small job: a generator of 6 layers in 2 stacks, a FastDiff for the epilogue, mels of
    2, 3, 9 and 1 frames (item 2 with a stream id of its own)"""
    import gpu_common
    from fastdiff_amd import infer
    cfg = ref.config(layers=6, stacks=2)
    gen = pwg.ParallelWaveGAN(**cfg).load_state_dict(ref.make_weights(cfg, 5))
    mels = [torch.from_numpy(np.ascontiguousarray(ref.synth_mel(50 + i, 1, t)[0].T, dtype=np.float32)) for i, t in enumerate((2, 3, 9, 1))]
    items = [{"item_name": f"u{i}", "mel": m, "len": m.shape[0]} for i, m in enumerate(mels)]
    items[2]["uid"] = 40
    return infer, gpu_common.make_model(), gen, items


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("host", "device"))
def test_synthesize_pwg_equals_direct_calls_item_by_item(job, where):
    infer, model, gen, items = job
    if where == "device":
        items = [dict(it, mel=it["mel"].cuda()) for it in items]
    pcm = infer.synthesize_pwg(model, gen, items, max_batch=2, seed=7)
    assert sorted(pcm) == ["u0", "u1", "u2"]                              # the one-frame item is absent
    for i, it in enumerate(items[:3]):
        t = it["mel"].shape[0] - 1                                        # spec2wav on the item's frames but the last, alone, then its own peak
        mel = it["mel"].T.unsqueeze(0).contiguous().cuda()
        want = model.peak_normalize_int16(gen.spec2wav(mel[:, :, :t].contiguous(), seed=7, stream_ids=[int(it.get("uid", i))])).cpu().numpy().reshape(-1)
        got = pcm[it["item_name"]]
        assert got.dtype == np.int16 and got.shape == (256 * t,) and np.abs(got).max() == 32767
        assert np.array_equal(got, want), it["item_name"]


@pytest.mark.gpu
def test_synthesize_pwg_at_another_rate_equals_each_item_alone(job):
    from fastdiff_amd import resample
    infer, model, gen, items = job
    pcm = infer.synthesize_pwg(model, gen, items, max_batch=2, seed=7, out_sample_rate=16000)
    assert sorted(pcm) == ["u0", "u1", "u2"]
    for i, it in enumerate(items[:3]):
        one = infer.synthesize_pwg(model, gen, [dict(it, uid=int(it.get("uid", i)))], max_batch=2, seed=7, out_sample_rate=16000)
        assert list(one) == [it["item_name"]] and np.array_equal(pcm[it["item_name"]], one[it["item_name"]])
        assert pcm[it["item_name"]].shape == (resample.out_len(256 * (it["mel"].shape[0] - 1), 22050, 16000),)


@pytest.mark.gpu
def test_synthesize_pwg_scores_into_the_models_report_keys(job, tmp_path):
    import synth
    from scipy.io import wavfile
    infer, model, gen, _ = job
    for i, frames in enumerate((86, 61)):                                  # two recordings, as tests/test_griffin_lim.py makes them
        x = np.clip(0.1 * synth.synth_audio(31 + i, 1, frames).reshape(-1), -0.9, 0.9)
        wavfile.write(tmp_path / f"r{i}.wav", 22050, np.round(x * 32767.0).astype(np.int16))
    items = infer.load_wav_inputs(model, str(tmp_path), keep_wav=True)
    assert [it["len"] for it in items] == [87, 62]
    _, theirs = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, stoi=True, spectral=True)
    pcm, report = infer.synthesize_pwg(model, gen, items, max_batch=2, seed=3, stoi=True, spectral=True)
    plain = infer.synthesize_pwg(model, gen, items, max_batch=2, seed=3)
    assert set(pcm) == set(report) == set(plain) == {"r0.wav", "r1.wav"}
    for name in pcm:
        assert set(report[name]) == set(theirs[name])
        assert report[name]["status"] == "OK" and report[name]["spectral_status"] == "OK"
        assert np.array_equal(pcm[name], plain[name])


@pytest.mark.gpu
def test_cli_vocoder_pwg(tmp_path):
    """infer --vocoder pwg on two tiny recordings writes the wavs and a score table."""
    import synth
    from scipy.io import wavfile
    src, out = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    for i, frames in enumerate((86, 61)):
        x = np.clip(0.1 * synth.synth_audio(31 + i, 1, frames).reshape(-1), -0.9, 0.9)
        wavfile.write(str(src / f"utt{i}.wav"), 22050, (x * 32767).astype(np.int16))
    cfg = ref.config(layers=6, stacks=2)
    write_dir(str(tmp_path / "pwg"), cfg, ref.with_weight_norm(ref.make_weights(cfg, 5)), False)
    cmd = [sys.executable, "-m", "fastdiff_amd.infer", "--test_input_dir", str(src), "--from_wav", "--out_dir", str(out), "--vocoder", "pwg",
           "--pwg_dir", str(tmp_path / "pwg"), "--spectral", "--max_batch", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    wavs = sorted(f for f in os.listdir(out) if f.endswith(".wav"))
    assert len(wavs) == 2, os.listdir(out)
    for f in wavs:
        rate, pcm = wavfile.read(str(out / f))
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.size % 256 == 0 and pcm.size >= 59 * 256 and np.abs(pcm).max() > 1000
    rows = open(out / "spectral.tsv").read().strip().split("\n")
    assert len(rows) == 3 and rows[0].split("\t")[0] == "name" and all(r.split("\t")[-1] == "OK" for r in rows[1:]), rows
    bad = subprocess.run([a for a in cmd if a != "--spectral"] + ["--long_form"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--vocoder pwg is not available with --long_form" in bad.stderr
