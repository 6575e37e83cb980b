"""STOI and ESTOI on the device (fd_stoi_bands / _frames / _measure, fastdiff_amd.stoi, FastDiff.stoi, Validator(stoi=True),
infer.synthesize(stoi=True), --stoi) against the float64 oracle tests/stoi_ref.py, which restates the header's steps 1-9 in numpy.

Bounds.  frames, kept, segments, status: equal.  stoi, estoi: 1e-6 -- a float32 emulation on the CPU of steps 2-5 with float64 segments
stays within 3e-8 of the oracle on these inputs, so 1e-6 leaves more than an order of magnitude for another transform order, and the
metric is read at 1e-2.  An utterance alone, in a ragged batch with garbage behind it, and from call to call: the same bits.  The
inputs keep every frame energy at least 0.01 dB from the silence threshold (asserted on the oracle; float32 energy rounding is about
1e-6 dB), so the mask cannot differ by rounding.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import _capi, infer
from fastdiff_amd import stoi as st
import stoi_ref as ref

NEW = ("fd_stoi_bands", "fd_stoi_frames", "fd_stoi_measure")
LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
HI = [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]
SCAN, SEGT = _capi.FD_STOI_SCAN_TILE, _capi.FD_STOI_SEG_TILE
DEGRADATIONS = ("snr30", "snr10", "snr0", "snr-5", "clip")
STEADY_LENGTHS = (256, 257, 4096, 4097, 4225)
# (on top of the lengths above: kept = frames = 30 + J, so these put J one below, at and one above the segment tile)
STEADY_LENGTHS += tuple(256 + 128 * (30 + SEGT + d) for d in (-1, 0, 1))
GAP_LENGTHS = (6000, 11610) + tuple(128 * T + d for T in (SEGT, SCAN) for d in (-1, 0, 257)) + (128 * (2 * SCAN + 300) + 77,)
RESAMPLED = ((22050, 25600), (22050, 14001), (16000, 18575), (16000, 9999))


@functools.lru_cache(maxsize=None)
def clean_of(kind, n, rate=10000):
    """float32 [n] from a fixed seed.  gap: 29 harmonics of a slowly varying 90-150 Hz fundamental, each with its own slow amplitude
    modulation, times a 4 Hz syllabic envelope, plus 0.02 N(0, 1), a 120 ms gap at -70 dB every 0.5 s, scaled to peak 0.2; steady: the
    same without gaps."""
    rng = np.random.default_rng([7, rate])                 # (not on n: a shorter signal is a prefix of a longer one up to the scale)
    N = max(n, 2 * rate)
    t = np.arange(N) / rate
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.31 * t + 0.4)
    phase = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(N)
    for h in range(1, 30):
        am = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0) * t + rng.uniform(0, 2 * np.pi))
        x += am * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)
    x += 0.02 * rng.standard_normal(N) * np.abs(x).max()
    if kind == "gap":
        pos = (t % 0.5)
        x = np.where((pos >= 0.3) & (pos < 0.42), x * 10.0 ** (-70.0 / 20.0), x)
    x = x[:n]
    x = (0.2 * x / np.abs(x).max()).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def degraded_of(kind, n, how, rate=10000):
    """clean plus white noise at 30, 10, 0, -5 dB SNR, or a hard clip at +-0.03"""
    x = clean_of(kind, n, rate).astype(np.float64)
    if how == "clip":
        y = np.clip(x, -0.03, 0.03)
    else:
        snr = float(how[3:])
        rng = np.random.default_rng([11, DEGRADATIONS.index(how), n])
        y = x + rng.standard_normal(n) * np.sqrt((x ** 2).mean() / 10.0 ** (snr / 10.0))
    y = y.astype(np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def oracle(kind, n, how, rate=10000):
    """The oracle's record of (clean_of, degraded_of); computed once, shared, never changed."""
    return ref.measure(clean_of(kind, n, rate), degraded_of(kind, n, how, rate), rate, detail=True)


def how_for(n):
    return DEGRADATIONS[n % len(DEGRADATIONS)]


def all_cases():
    cases = [("steady", n, how_for(n), 10000) for n in STEADY_LENGTHS] + [("gap", n, how_for(n), 10000) for n in GAP_LENGTHS]
    cases += [("gap", 11610, how, 10000) for how in DEGRADATIONS]
    cases += [("gap", n, how_for(n), rate) for rate, n in RESAMPLED]
    return cases


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+FD_STOI_SCAN_TILE\s+(\d+)", header).group(1)) == SCAN == st.SCAN_TILE
    assert int(re.search(r"#define\s+FD_STOI_SEG_TILE\s+(\d+)", header).group(1)) == SEGT == st.SEG_TILE
    assert st.RECORD.itemsize == 32
    assert callable(fastdiff_amd.FastDiff.stoi) and "stoi" in fastdiff_amd.__all__ and fastdiff_amd.stoi is st
    assert (st.OK, st.SHORT, st.SILENT) == (ref.OK, ref.SHORT, ref.SILENT) and st.STATUS[st.SHORT] == "SHORT"
    assert lib.fd_stoi_measure(None, None, None, 1, 1000, None, 10000, None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_stoi_bands(None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_stoi_frames(-1) == _capi.FD_ERR_INVALID
    assert "as recalled" in header.lower() and header.count("DEVIATION") >= 2


def test_band_table_is_the_pinned_one_and_the_oracles():
    lo, hi = st.bands()
    assert list(lo) == LO and list(hi) == HI
    assert ref.bands() == (LO, HI)


def test_frame_count_equals_the_oracle():
    for n in list(range(250, 701)) + list(range(4090, 4104)):
        assert st.frames(n) == ref.frames(n), n
    assert [st.frames(n) for n in (256, 257, 4096, 4097)] == [0, 1, 30, 31]
    assert st.frames(0) == 0


def test_oracle_anchors():
    """No outside number is available offline (pystoi is not installed and nothing can be fetched), so the oracle is anchored on the
    measure's own properties: identical signals score 1, the score falls with the SNR, and it does not depend on the level of y."""
    n = 11610
    x = clean_of("gap", n)
    same = ref.measure(x, x)
    assert same["status"] == ref.OK and abs(same["stoi"] - 1.0) <= 1e-12 and abs(same["estoi"] - 1.0) <= 1e-12, same
    rows = [oracle("gap", n, how) for how in ("snr30", "snr10", "snr0", "snr-5")]
    for a, b in zip(rows, rows[1:]):
        assert a["stoi"] > b["stoi"] and a["estoi"] > b["estoi"], rows
    assert all(r["estoi"] < r["stoi"] for r in rows)
    assert (rows[0]["frames"], rows[0]["kept"], rows[0]["segments"]) == (89, rows[0]["kept"], rows[0]["kept"] - 30)
    for how in ("snr10", "clip"):
        y = degraded_of("gap", n, how)
        half = ref.measure(x, y * np.float32(0.5))
        assert abs(half["stoi"] - oracle("gap", n, how)["stoi"]) <= 1e-12 and abs(half["estoi"] - oracle("gap", n, how)["estoi"]) <= 1e-12


def test_inputs_stay_clear_of_the_threshold_and_take_every_branch():
    """A condition on the test's inputs, checked on the oracle."""
    clipped = 0.0
    for kind, n, how, rate in all_cases():
        r = oracle(kind, n, how, rate)
        assert r["margin"] >= 0.01, (kind, n, how, rate, r)
        if kind == "steady":
            assert r["kept"] == r["frames"], (n, r)
        clipped = max(clipped, r.get("clipped", 0.0))
    r = oracle("gap", 11610, "snr10")
    assert r["status"] == ref.OK and 30 < r["kept"] < r["frames"] == 89, r
    assert clipped > 0.0
    assert [oracle("steady", n, how_for(n))["status"] for n in STEADY_LENGTHS[:5]] == [ref.SHORT, ref.SHORT, ref.SHORT, ref.OK, ref.OK]
    assert [oracle("steady", n, how_for(n))["segments"] for n in STEADY_LENGTHS[5:]] == [SEGT - 1, SEGT, SEGT + 1]
    assert oracle("steady", 4097, how_for(4097))["segments"] == 1


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, b, want, where):
    assert (int(got["frames"][b]), int(got["kept"][b]), int(got["segments"][b]), int(got["status"][b])) == \
        (want["frames"], want["kept"], want["segments"], want["status"]), (where, {k: got[k][b] for k in got}, want)
    if want["status"] != ref.OK:
        assert np.isnan(got["stoi"][b]) and np.isnan(got["estoi"][b]), (where, got["stoi"][b], got["estoi"][b])
        return 0.0
    e1, e2 = abs(float(got["stoi"][b]) - want["stoi"]), abs(float(got["estoi"][b]) - want["estoi"])
    print(f"{where}: stoi {got['stoi'][b]:.9f} oracle {want['stoi']:.9f} |diff| {e1:.2e}; estoi {got['estoi'][b]:.9f} oracle {want['estoi']:.9f} |diff| {e2:.2e}")
    assert e1 <= 1e-6 and e2 <= 1e-6, (where, got["stoi"][b], want["stoi"], got["estoi"][b], want["estoi"])
    return max(e1, e2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lengths", (("steady", STEADY_LENGTHS), ("gap", GAP_LENGTHS)))
def test_measure_against_the_oracle_at_10_khz(model, kind, lengths):
    worst = 0.0
    for n in lengths:
        how = how_for(n)
        got = model.stoi(dev(clean_of(kind, n)), dev(degraded_of(kind, n, how)), sample_rate=10000)
        worst = max(worst, _check(got, 0, oracle(kind, n, how), (kind, n, how)))
    print(f"{kind}: max |diff| {worst:.2e}")


@pytest.mark.gpu
def test_every_degradation_at_the_validation_window(model):
    n = 11610
    for how in DEGRADATIONS:
        got = model.stoi(dev(clean_of("gap", n)), dev(degraded_of("gap", n, how)), sample_rate=10000)
        _check(got, 0, oracle("gap", n, how), ("gap", n, how))


@pytest.mark.gpu
@pytest.mark.parametrize("rate,n", RESAMPLED)
def test_measure_through_the_internal_resample(model, rate, n):
    how = how_for(n)
    got = model.stoi(dev(clean_of("gap", n, rate)), dev(degraded_of("gap", n, how, rate)), sample_rate=rate)
    _check(got, 0, oracle("gap", n, how, rate), ("gap", rate, n, how))


@pytest.mark.gpu
def test_silent_and_short_rows(model):
    n = 6000
    z = torch.zeros(n, device="cuda")
    got = model.stoi(z, dev(degraded_of("gap", n, "snr10")), sample_rate=10000)
    assert int(got["status"][0]) == st.SILENT and int(got["frames"][0]) == ref.frames(n) and int(got["kept"][0]) == 0
    assert np.isnan(got["stoi"][0]) and np.isnan(got["estoi"][0])
    x = np.stack([clean_of("steady", 4097)] * 3)
    got = model.stoi(dev(x), dev(x), valid=[4097, 4096, 200], sample_rate=10000)
    assert list(got["status"]) == [st.OK, st.SHORT, st.SHORT] and list(got["frames"]) == [31, 30, 0] and list(got["segments"]) == [1, 0, 0]
    assert abs(got["stoi"][0] - 1.0) <= 1e-9 and np.isnan(got["stoi"][1:]).all() and np.isnan(got["estoi"][1:]).all()
    got = model.stoi(z[:8000], z[:8000], sample_rate=16000)                 # through the resampler: still exact zeros
    assert int(got["status"][0]) == st.SILENT


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (10000, 22050))
def test_ragged_batches_are_batch_invariant_and_deterministic(model, rate):
    L = 128 * (SCAN + 40) + 99 if rate == 10000 else 30000
    valid = [L, 11610, 256 + 128 * (30 + SEGT + 9) + 5, 6000, 300] if rate == 10000 else [L, 25600, 14001, 18000, 500]
    rng = np.random.default_rng(5)
    xs, ys = (rng.standard_normal((5, L)).astype(np.float32) * 3.0 for _ in range(2))      # garbage behind every utterance
    for b, v in enumerate(valid):
        xs[b, :v] = clean_of("gap", v, rate)
        ys[b, :v] = degraded_of("gap", v, how_for(b), rate)
    xd, yd = dev(xs), dev(ys)
    rec = model.stoi(xd, yd, valid=valid, sample_rate=rate)
    assert list(rec["status"]) == [st.OK, st.OK, st.OK, st.OK, st.SHORT]
    for b, v in enumerate(valid):
        _check(rec, b, ref.measure(xs[b, :v], ys[b, :v], rate), ("ragged", rate, b, v))
    for b, v in enumerate(valid):
        alone = model.stoi(xd[b, :v].clone(), yd[b, :v].clone(), sample_rate=rate)
        for key in rec:
            assert rec[key][b].tobytes() == alone[key][0].tobytes(), (b, key, rec[key][b], alone[key][0])
    again = model.stoi(xd, yd, valid=valid, sample_rate=rate)
    assert all(again[k].tobytes() == rec[k].tobytes() for k in rec)


@pytest.mark.gpu
def test_the_call_captures_and_a_growing_scratch_is_refused_inside_a_capture():
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no scratch yet
    n = 11610
    xa, ya = dev(clean_of("gap", n)).reshape(1, n), dev(degraded_of("gap", n, "snr10")).reshape(1, n)
    xb, yb = dev(clean_of("steady", n)).reshape(1, n), dev(degraded_of("steady", n, "snr0")).reshape(1, n)
    want_a = m.stoi(xa, ya, sample_rate=10000)             # (also grows the scratch buffer)
    want_b = m.stoi(xb, yb, sample_rate=10000)
    lib, h = m._ready(torch.device("cuda"))
    x, y = xa.clone(), ya.clone()
    rec = torch.zeros((1, 32), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, lib.fd_stoi_measure(h, x.data_ptr(), y.data_ptr(), 1, n, None, 10000, rec.data_ptr(), m._stream(x.device)), "fd_stoi_measure")
    graph.replay()
    torch.cuda.synchronize()
    got = st._record(rec)
    assert all(got[k].tobytes() == want_a[k].tobytes() for k in got)
    x.copy_(xb)
    y.copy_(yb)
    graph.replay()
    torch.cuda.synchronize()
    got = st._record(rec)
    assert all(got[k].tobytes() == want_b[k].tobytes() for k in got)
    big = torch.zeros(4, 64 * n, device="cuda")
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(_capi.FastDiffHipError, match="stream capture"):
        with torch.cuda.graph(refused):
            x.mul_(1.0)                                    # (so that the abandoned capture is not empty)
            m.stoi(big, big, sample_rate=10000)
    torch.cuda.synchronize()
    after = m.stoi(xa, ya, sample_rate=10000)              # the handle works on
    assert all(after[k].tobytes() == want_a[k].tobytes() for k in after)


@pytest.mark.gpu
def test_refusals_leave_a_message(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(1, 9000, device="cuda")
    rec = torch.empty(32, dtype=torch.uint8, device="cuda")
    assert lib.fd_stoi_measure(h, x.data_ptr(), x.data_ptr(), 1, 9000, None, 7999, rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"sample rate" in lib.fd_last_error(h)
    assert lib.fd_stoi_measure(h, x.data_ptr(), x.data_ptr(), 0, 9000, None, 10000, rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"B = 0" in lib.fd_last_error(h)
    assert lib.fd_stoi_measure(h, x.data_ptr(), None, 1, 9000, None, 10000, rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"null degraded" in lib.fd_last_error(h)
    with pytest.raises(Exception, match="valid"):
        model.stoi(x, x, valid=[9001], sample_rate=10000)
    with pytest.raises(Exception, match="valid"):
        model.stoi(x, x, valid=[0], sample_rate=10000)
    with pytest.raises(ValueError):
        model.stoi(x, x[:, :100], sample_rate=10000)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def corpus(model, tmp_path_factory):
    d = tmp_path_factory.mktemp("stoi_corpus")
    for i, n in enumerate((40000, 33000, 52000)):
        x = clean_of("gap", n, 22050)
        wavfile.write(d / f"r{i}.wav", 22050, np.round(x * 4.0 * 32767.0).astype(np.int16))
    return fastdiff_amd.TrainCorpus.from_wav_dir(model, str(d), max_samples=25600), str(d)


@pytest.mark.gpu
def test_validator_scores_every_batch(model, corpus):
    from fastdiff_amd import schedules
    hp = schedules.training_hyperparams()
    kw = dict(corpus=corpus[0], batch_size=2, sample_schedule=schedules.noise_schedule_for(4))
    val = fastdiff_amd.Validator(model, hp, stoi=True, **kw)
    first = val.run().result()
    n = corpus[0].n_items
    last = (n - 1) // 2 * 2                                # first item of the last batch
    rec = model.stoi(val.wav, val.sampled, sample_rate=22050)
    count = n - last
    assert first["item_stoi"][last:].tobytes() == rec["stoi"][:count].tobytes()
    assert first["item_estoi"][last:].tobytes() == rec["estoi"][:count].tobytes()
    ok = ~np.isnan(first["item_stoi"])
    assert first["stoi_skipped"] == int((~ok).sum()) and ok.any()
    assert first["stoi"] == pytest.approx(first["item_stoi"][ok].mean(), abs=1e-12)
    assert first["estoi"] == pytest.approx(first["item_estoi"][ok].mean(), abs=1e-12)
    print(f"validator: stoi {first['stoi']:.4f} estoi {first['estoi']:.4f} skipped {first['stoi_skipped']} of {n}")
    second = val.run().result()
    for k in ("item_stoi", "item_estoi", "item_mel_l1", "item_loss"):
        assert second[k].tobytes() == first[k].tobytes(), k
    assert second["stoi"] == first["stoi"] and second["estoi"] == first["estoi"]
    plain = fastdiff_amd.Validator(model, hp, **kw).run().result()
    assert set(plain) == {"loss", "items", "nonfinite", "loss_by_t", "count_by_t", "item_loss", "mel_l1", "item_mel_l1"}
    assert set(first) == set(plain) | {"stoi", "estoi", "item_stoi", "item_estoi", "stoi_skipped"}
    assert plain["item_mel_l1"].tobytes() == first["item_mel_l1"].tobytes() and plain["item_loss"].tobytes() == first["item_loss"].tobytes()
    with pytest.raises(ValueError, match="sample_schedule"):
        fastdiff_amd.Validator(model, hp, corpus=corpus[0], batch_size=2, stoi=True)


@pytest.mark.gpu
def test_copy_synthesis_reports_what_the_model_measures(model, corpus, tmp_path):
    items = infer.load_wav_inputs(model, corpus[1], keep_wav=True)
    assert all(it["wav"].is_cuda and it["wav"].dim() == 1 for it in items)
    assert "wav" not in infer.load_wav_inputs(model, corpus[1])[0]
    pcm, report = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3, stoi=True)
    plain = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=3)
    assert set(report) == set(pcm) == set(plain) and all(np.array_equal(pcm[k], plain[k]) for k in pcm)
    rows = infer._step_rows(model, 4, None, None)
    for i, it in enumerate(items):
        t = it["len"] - 1
        mel = it["mel"][:t].transpose(0, 1).unsqueeze(0).contiguous().cuda()
        with torch.no_grad():
            wav = model.sample(mel, rows, ddim=False, seed=3, lens=[t], stream_ids=[i])
        own = model.stoi(it["wav"][: t * 256].clone(), wav.reshape(-1)[: t * 256].clone(), sample_rate=22050)
        r = report[it["item_name"]]
        assert set(r) == {"stoi", "estoi", "status"}
        assert r["status"] == st.STATUS[int(own["status"][0])]
        assert np.float64(r["stoi"]).tobytes() == own["stoi"][0].tobytes() and np.float64(r["estoi"]).tobytes() == own["estoi"][0].tobytes()
    with pytest.raises(ValueError, match="wav"):
        infer.synthesize(model, infer.load_wav_inputs(model, corpus[1]), n_steps=4, stoi=True)
    with pytest.raises(ValueError, match="stoi"):
        infer.synthesize_long(model, items, n_steps=4, stoi=True)
    with pytest.raises(ValueError, match="stoi"):
        infer.synthesize_sharded(model, items, n_steps=4, stoi=True)
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", corpus[1], "--out_dir", str(tmp_path / "o"), "--stoi"])
    out = tmp_path / "out"
    infer.main(["--test_input_dir", corpus[1], "--out_dir", str(out), "--from_wav", "--stoi"])
    lines = open(out / "stoi.tsv").read().strip().split("\n")
    assert len(lines) == 1 + len(items) and lines[0].split("\t") == ["name", "stoi", "estoi", "status"]
