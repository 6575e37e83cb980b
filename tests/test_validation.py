"""The held-out pass on the device (fastdiff_amd.Validator; fd_eval_collate, fd_item_distance, fd_eval_accumulate; TrainCorpus.eval_plan).

CPU: the host twin of the pass's choice -- every item exactly once over ceil(n / B) batches, surplus slots (-1, -1), the starts in range
and equal to oracle/philox.py's words; the constructor's refusals; the symbols.
GPU: the collated batches EQUAL torch slicing of the arenas at the twin's picks; the per-item distances against float64 within the
forward error bound of the fixed-order sum, bit-identical between two calls, an inf in one item leaving the others alone; the
accumulators EQUAL a float64 numpy evaluation in slot order; validate - train - validate end to end without a tolerance (two passes
agree bit for bit, a pass after a TrainStep step runs on device-refreshed packs and equals a fresh module that loaded the trained
weights through the host); the loss against the reference formula on the Validator's own buffers; the sampled mel metric.

The bound of fd_item_distance, from the code (csrc/fd_kernels_step.hip): a thread adds at most FD_STEP_RUN = 16 terms serially, the 256
threads of a workgroup are added by an 8-level tree, the P = ceil(slots / 1024) workgroups of an item by a tree of ceil(log2 P) levels
(adding a zero is exact) -- an element passes through at most 16 + ceil(log2(n / 16)) + 1 <= RUN + ceil(log2 n) - 3 roundings; the
term itself carries 2 (the rounded difference, squared) or 1 (its absolute value), the final division by n one more: no deeper than
the issue's (RUN + ceil(log2 n) + 4) * 2^-24 * value, which is therefore used as stated.
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox   # noqa: E402
import synth    # noqa: E402

import fastdiff_amd                                      # noqa: E402
from fastdiff_amd import TrainCorpus, _capi, schedules   # noqa: E402

NEW = ("fd_eval_collate", "fd_item_distance", "fd_eval_accumulate")
RUN = 16
HOP = 256


def bar(n):
    return (RUN + math.ceil(math.log2(n)) + 4) * 2.0 ** -24


def blank_corpus(n, F, hop=4):
    """n items of F + 1 .. F + 40 frames, zeros."""
    lengths = [F + 1 + (13 * i) % 40 for i in range(n)]
    return TrainCorpus([{"mel": np.zeros((T, 80), np.float32), "wav": np.zeros(T * hop, np.float32)} for T in lengths], hop_size=hop,
                       max_samples=F * hop, device="cpu")


def start_words(seed, batch, B):
    b = np.arange(B, dtype=np.uint64)
    w = philox.words(seed, 0xFFFFFFFC, b >> np.uint64(2), uid=batch)
    return np.stack(w, axis=-1)[np.arange(B), (b & np.uint64(3)).astype(np.int64)].astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_train.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    assert "Validator" in fastdiff_amd.__all__ and callable(TrainCorpus.eval_plan)
    from fastdiff_amd import lvc_op
    for name in ("eval_collate", "item_distance", "eval_accumulate"):
        assert callable(getattr(lvc_op, name))
    assert fastdiff_amd.validate.DEFAULT_SEED != 0, "TrainStep's default seed is 0: batch j must not repeat training step j's noise"


@pytest.mark.parametrize("n", [1, 4, 7])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_eval_plan_takes_every_item_once(n, B):
    F = 6
    c = blank_corpus(n, F)
    batches = (n + B - 1) // B
    for seed in (0x56414C, 2 ** 63 + 7):
        seen = []
        for j in range(batches):
            picks = c.eval_plan(j, B, seed=seed)
            assert picks.shape == (B, 2) and picks.dtype == np.int64
            w = start_words(seed, j, B)
            for b in range(B):
                g = j * B + b
                if g >= n:
                    assert picks[b].tolist() == [-1, -1], (n, B, j, b)
                    continue
                item, start = picks[b].tolist()
                assert item == g
                rng = int(c.lengths[item]) - F
                assert 0 <= start < rng
                assert start == (int(w[b]) * rng) >> 32, (n, B, j, b)
                seen.append(item)
            fill = c.eval_plan(j, B, seed=seed, fill=True)
            for b in range(B):
                if j * B + b >= n:
                    assert fill[b].tolist() == [n - 1, (int(w[b]) * (int(c.lengths[n - 1]) - F)) >> 32]
                else:
                    assert fill[b].tolist() == picks[b].tolist()
        assert seen == list(range(n)), (n, B, seed)
        assert all(np.array_equal(c.eval_plan(j, B, seed=seed), c.eval_plan(j, B, seed=seed)) for j in range(batches))
    # two seeds differ somewhere over a corpus with room to move (40 frames of range, 64 slots)
    wide = TrainCorpus([{"mel": np.zeros((F + 40, 80), np.float32), "wav": np.zeros((F + 40) * 4, np.float32)}] * 64, hop_size=4,
                       max_samples=F * 4, device="cpu")
    assert not np.array_equal(wide.eval_plan(0, 64, seed=1), wide.eval_plan(0, 64, seed=2))
    assert not np.array_equal(wide.eval_plan(0, 32, seed=1)[:, 1], wide.eval_plan(1, 32, seed=1)[:, 1])
    with pytest.raises(ValueError):
        c.eval_plan(0, 0)


def test_the_constructor_refuses_what_it_cannot_run():
    c = blank_corpus(3, 6, hop=HOP)
    dh = schedules.training_hyperparams()
    cpu_model = fastdiff_amd.FastDiff()
    for bad in (0, 65):
        with pytest.raises(ValueError, match="bins"):
            fastdiff_amd.Validator(cpu_model, dh, corpus=c, batch_size=2, bins=bad)
    with pytest.raises(ValueError, match="batch_size"):
        fastdiff_amd.Validator(cpu_model, dh, corpus=c, batch_size=0)
    with pytest.raises(RuntimeError, match="HIP device"):
        fastdiff_amd.Validator(cpu_model, dh, corpus=c, batch_size=2)


# ------------------------------------------------------------------------------------------------------------------ GPU
def host_batch(cpu, picks):
    """The reference's collater on given picks: torch slicing of the host arenas."""
    F, hop = cpu.frames, cpu.hop_size
    first = [int(cpu.frame_off_host[i]) + int(s) for i, s in picks]
    mels = torch.stack([cpu.mel[p: p + F].transpose(0, 1) for p in first])
    wavs = torch.stack([cpu.wav[p * hop: (p + F) * hop].view(1, -1) for p in first])
    return mels.contiguous(), wavs.contiguous()


def random_corpus(n, F, seed):
    gen = torch.Generator().manual_seed(seed)
    lengths = [F + 1 + (13 * i + seed) % 40 for i in range(n)]
    return TrainCorpus([{"mel": torch.randn(T, 80, generator=gen).numpy(), "wav": torch.randn(T * HOP, generator=gen).numpy()} for T in lengths],
                       hop_size=HOP, max_samples=F * HOP, device="cpu")


def model_corpus(lengths, F):
    """Items with mels of the range the model is fed in the other tests and waveforms of speech-like level."""
    mel = synth.synth_mel(3, 1, sum(lengths))[0].T
    gen = torch.Generator().manual_seed(11)
    items, at = [], 0
    for T in lengths:
        items.append({"mel": np.ascontiguousarray(mel[at: at + T]), "wav": (0.3 * torch.randn(T * HOP, generator=gen)).numpy()})
        at += T
    return TrainCorpus(items, hop_size=HOP, max_samples=F * HOP, device="cpu")


@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def dh():
    return schedules.training_hyperparams()


@pytest.fixture(scope="module")
def model(gc):
    return gc.make_model()


def same(a, b):
    """Two result() dictionaries, bit for bit (NaN of an empty bin included)."""
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [7, 33, 65])
def test_collated_batches_are_exact(F):
    from fastdiff_amd import lvc_op
    for n in (1, 4, 7):
        cpu = random_corpus(n, F, seed=F + n)
        dev = cpu.to("cuda")
        for B in (1, 3, 5):
            seed = 0x56414C + B
            state = lvc_op.new_train_state("cuda")
            seen = []
            for j in range((n + B - 1) // B):
                state[0] = j
                mels, wavs, picked = lvc_op.eval_collate(dev, B, seed=seed, iteration=99, state=state)      # (the state wins)
                tag = (F, n, B, j)
                got = picked.cpu().numpy()
                assert np.array_equal(got, cpu.eval_plan(j, B, seed=seed)), (tag, got.tolist())
                want_mels, want_wavs = host_batch(cpu, cpu.eval_plan(j, B, seed=seed, fill=True))
                assert torch.equal(mels.cpu(), want_mels), tag
                assert torch.equal(wavs.cpu(), want_wavs), tag
                seen += [int(i) for i in got[:, 0] if i >= 0]
                assert (got[:, 0] >= 0).sum() == min(B, n - j * B)
            assert seen == list(range(n)), (F, n, B)
            by_host = lvc_op.eval_collate(dev, B, seed=seed, iteration=0)
            assert np.array_equal(by_host[2].cpu().numpy(), cpu.eval_plan(0, B, seed=seed))


@pytest.mark.gpu
def test_the_pass_counts_its_batches_on_the_device(model, dh):
    cpu = model_corpus([8, 19, 9, 12], 7)
    val = fastdiff_amd.Validator(model, dh, corpus=cpu.to("cuda"), batch_size=3)
    assert val.n_batches == 2
    val.run()
    assert val.state()["iter"] == 2
    val.begin()
    assert val.state()["iter"] == 0
    for j in range(2):
        val.batch(j)
        assert val.state()["iter"] == j + 1
        assert np.array_equal(val.picked.cpu().numpy(), cpu.eval_plan(j, 3, seed=val.seed)), j
        want_mels, want_wavs = host_batch(cpu, cpu.eval_plan(j, 3, seed=val.seed, fill=True))
        assert torch.equal(val.mel.cpu(), want_mels) and torch.equal(val.wav.cpu(), want_wavs), j
    model.train()
    val.run()
    assert model.training and val.state()["iter"] == 2
    model.eval()
    val.run()
    assert not model.training
    with pytest.raises(RuntimeError, match="corpus lies on"):
        fastdiff_amd.Validator(model, dh, corpus=cpu, batch_size=3)


DIST_N = (1, 15, 16, 17, 4095, 4096, 4097, 7 * 256)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B", [1, 5])
def test_item_distance_against_float64(kind, B):
    from fastdiff_amd import lvc_op
    gen = torch.Generator().manual_seed(100 * B + kind)
    for n in DIST_N:
        a, b = (torch.randn(B, n, generator=gen).cuda() for _ in range(2))
        got = lvc_op.item_distance(a, b, kind)
        again = lvc_op.item_distance(a, b, kind)
        d = a.double() - b.double()
        want = (d * d if kind == 0 else d.abs()).mean(dim=1)
        rel = ((got.double() - want).abs() / want).max().item()
        print(f"kind {kind} B {B} n {n}: max rel err {rel:.3e} (bar {bar(n):.3e})")
        assert torch.equal(got, again), (kind, B, n)
        assert rel <= bar(n), (kind, B, n, rel, bar(n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_a_non_finite_item_is_counted_and_spoils_no_other(kind):
    from fastdiff_amd import lvc_op
    gen = torch.Generator().manual_seed(7)
    B, n = 5, 4097                       # (item borders inside 16-byte slots: items 1 .. 4 start at an odd offset)
    a, b = (torch.randn(B, n, generator=gen).cuda() for _ in range(2))
    clean = lvc_op.item_distance(a, b, kind).clone()
    a[2, 0], a[2, n - 1] = float("inf"), float("nan")
    got = lvc_op.item_distance(a, b, kind)
    others = [0, 1, 3, 4]
    assert torch.equal(got[others], clean[others])
    assert not torch.isfinite(got[2])
    picked = torch.tensor([[i, 0] for i in range(B)], dtype=torch.int64, device="cuda")
    acc, item_out = lvc_op.new_eval_state("cuda"), torch.zeros(B, device="cuda")
    steps = torch.tensor([3.0, 500.0, 501.0, 999.0, 0.0], device="cuda")
    lvc_op.eval_accumulate(got, picked, acc, steps=steps, T_train=1000, bins=10, item_out=item_out)
    res = lvc_op.read_eval_state(acc, 10)
    vals = clean.cpu().numpy().astype(np.float64)
    total = 0.0
    for i in others:
        total += vals[i]
    assert res["nonfinite"] == 1 and res["count"] == 4 and res["sum"] == total
    assert res["bin_count"].tolist() == [2, 0, 0, 0, 0, 1, 0, 0, 0, 1] and res["bin_sum"][5] == vals[1] and res["bin_sum"][0] == vals[0] + vals[4]
    assert torch.equal(item_out[others], clean[others])


@pytest.mark.gpu
@pytest.mark.parametrize("T_train", [7, 1000])
@pytest.mark.parametrize("bins", [1, 10])
def test_accumulators_equal_float64_in_slot_order(T_train, bins):
    from fastdiff_amd import lvc_op
    n_items = 9
    batches = [  # (values, steps, items): -1 = an inactive slot
        ([0.1, 1e-7, 3.5, 2e4, 0.25], [0, T_train - 1, T_train // 2, 1, T_train - 1], [0, 1, -1, 2, 3]),
        ([7.0, 1.0 / 3.0, 9e-5, 0.5, 0.75], [T_train - 1, 0, 3 % T_train, 2 % T_train, 5 % T_train], [4, -1, 5, 6, -1]),
        ([1e3, 2.0, 3.0, 4.0, 5.0], [T_train // 3, 0, 0, 0, 0], [7, 8, -1, -1, -1]),
    ]
    acc = lvc_op.new_eval_state("cuda")
    state = lvc_op.new_train_state("cuda")
    item_out = torch.full((n_items,), -1.0, device="cuda")
    want_sum, want_count = 0.0, 0
    want_bin, want_bin_count, want_items = np.zeros(bins), np.zeros(bins, np.int64), np.full(n_items, -1.0, np.float32)
    for values, steps, items in batches:
        v32 = np.asarray(values, np.float32)
        picked = torch.tensor([[i, 2 if i >= 0 else -1] for i in items], dtype=torch.int64, device="cuda")
        lvc_op.eval_accumulate(torch.from_numpy(v32).cuda(), picked, acc, steps=torch.tensor(steps, dtype=torch.float32, device="cuda"),
                               T_train=T_train, bins=bins, item_out=item_out, advance=state)
        for v, ts, i in zip(v32, steps, items):
            if i < 0:
                continue
            want_sum += np.float64(v)
            want_count += 1
            want_bin[(ts * bins) // T_train] += np.float64(v)
            want_bin_count[(ts * bins) // T_train] += 1
            want_items[i] = v
    res = lvc_op.read_eval_state(acc, bins)
    assert res["sum"] == want_sum and res["count"] == want_count == 9 and res["nonfinite"] == 0
    assert np.array_equal(res["bin_sum"], want_bin) and np.array_equal(res["bin_count"], want_bin_count)
    assert np.array_equal(item_out.cpu().numpy(), want_items)
    assert lvc_op.read_train_state(state)["iter"] == 3
    if T_train == 7 and bins == 10:
        assert (res["bin_count"] == 0).any(), "7 steps cannot fill 10 bins"
    # without steps nothing is binned, without advance nothing counted
    acc2 = lvc_op.new_eval_state("cuda")
    lvc_op.eval_accumulate(torch.ones(2, device="cuda"), torch.tensor([[0, 0], [-1, -1]], device="cuda"), acc2)
    res2 = lvc_op.read_eval_state(acc2)
    assert res2["sum"] == 1.0 and res2["count"] == 1 and not res2["bin_count"].any()


@pytest.mark.gpu
def test_validate_train_validate_end_to_end(gc, dh):
    """(a) two passes agree bit for bit; (b) a pass after one TrainStep step runs on packs refreshed on the device and sees the step;
    (c) a fresh module that loaded the trained weights through the host gives (b)'s result bit for bit."""
    F, B = 7, 3
    held_out = model_corpus([8, 19, 9, 12], F).to("cuda")
    train = model_corpus([9, 14, 30], F).to("cuda")
    m = gc.make_model().train()
    val = fastdiff_amd.Validator(m, dh, corpus=held_out, batch_size=B)
    a1 = val.run().result()
    a2 = val.run().result()
    assert m.training
    assert a1["items"] == 4 and a1["nonfinite"] == 0 and math.isfinite(a1["loss"]) and a1["count_by_t"].sum() == 4
    assert same(a1, a2), (a1, a2)
    ts = fastdiff_amd.TrainStep(m, dh, lr=1e-2, graph=False, corpus=train, batch_size=2)
    ts.step()
    b = val.run().result()
    assert m.last_refresh == "device", m.last_refresh
    assert ts.state()["applied"] == 1
    assert b["items"] == 4 and math.isfinite(b["loss"]) and b["loss"] != a1["loss"], (a1["loss"], b["loss"])
    assert np.array_equal(b["count_by_t"], a1["count_by_t"]), "the draws are those of (a): only the weights moved"
    fresh = fastdiff_amd.FastDiff()
    fresh.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    fresh = fresh.cuda().eval()
    c = fastdiff_amd.Validator(fresh, dh, corpus=held_out, batch_size=B).run().result()
    assert fresh.last_refresh.startswith("host"), fresh.last_refresh
    first = next((k for k in b if np.asarray(b[k]).tobytes() != np.asarray(c[k]).tobytes()), None)
    assert first is None, (first, b[first], c[first])


@pytest.mark.gpu
def test_the_loss_is_the_reference_formula_on_the_pass_buffers(model, dh):
    F, B, bins = 7, 4, 10
    cpu = model_corpus([8, 19, 9], F)
    val = fastdiff_amd.Validator(model, dh, corpus=cpu.to("cuda"), batch_size=B, bins=bins)      # one batch, its last slot inactive
    res = val.run().result()
    eps, z, steps = val.eps.double().cpu(), val.z.double().cpu(), val.steps.cpu().view(-1).numpy()
    assert val.picked.cpu().numpy()[:, 0].tolist() == [0, 1, 2, -1]
    want = ((eps - z) ** 2).mean(dim=(1, 2)).numpy()[:3]
    rel = np.abs(res["item_loss"].astype(np.float64) - want) / want
    print(f"item_loss {res['item_loss'].tolist()} rel err {rel.tolist()} bar {bar(F * HOP):.3e}")
    assert (rel <= bar(F * HOP)).all(), (rel, bar(F * HOP))
    assert ((steps >= 0) & (steps < 1000) & (steps == np.floor(steps))).all()
    sums, counts, total = np.zeros(bins), np.zeros(bins, np.int64), 0.0
    for v, ts in zip(res["item_loss"][:3], steps[:3]):
        k = (int(ts) * bins) // 1000
        sums[k] += np.float64(v)
        counts[k] += 1
        total += np.float64(v)
    assert np.array_equal(res["count_by_t"], counts) and res["items"] == 3 and res["loss"] == total / 3
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res["loss_by_t"], sums / counts, equal_nan=True)
    # the draws are train_draw's under the pass's seed and batch index: the twin of the step draw says the same
    w = philox.words(val.seed, 0xFFFFFFFD, np.arange(B, dtype=np.uint64) >> np.uint64(2), uid=0)
    ts_twin = [(int(np.stack(w, axis=-1)[b, b & 3]) * 1000) >> 32 for b in range(B)]
    assert steps.astype(np.int64).tolist() == ts_twin


@pytest.mark.gpu
def test_the_sampled_mel_metric(model, dh):
    F, B = 33, 2
    cpu = model_corpus([34, 50, 40], F)
    val = fastdiff_amd.Validator(model, dh, corpus=cpu.to("cuda"), batch_size=B, sample_schedule=schedules.noise_schedule_for(4))
    val.begin()
    want = np.zeros(3)
    for j in range(2):
        val.batch(j)
        d = (val.mel_sampled.double() - val.mel_target.double()).abs().mean(dim=(1, 2)).cpu().numpy()
        assert val.mel_sampled.shape == val.mel_target.shape == (B, 80, F)
        for slot, item in enumerate(val.picked.cpu().numpy()[:, 0]):
            if item >= 0:
                want[item] = d[slot]
    first = val.result()
    rel = np.abs(first["item_mel_l1"].astype(np.float64) - want) / want
    print(f"item_mel_l1 {first['item_mel_l1'].tolist()} rel err {rel.tolist()} bar {bar(80 * F):.3e}")
    assert (rel <= bar(80 * F)).all(), (rel, bar(80 * F))
    total = 0.0
    for v in first["item_mel_l1"]:
        total += np.float64(v)
    assert first["mel_l1"] == total / 3 and first["items"] == 3
    second = val.run().result()
    assert same(first, second)
