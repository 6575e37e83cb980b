"""The device-resident training corpus and its on-device collater (fastdiff_amd.TrainCorpus, lvc_op.train_collate / fd_train_collate,
TrainStep(corpus=...)).

CPU: the host twin of the choice (TrainCorpus.plan) -- pi is a bijection per epoch and differs between epochs, the start frames lie in
[0, T - F) and reach both ends; the filter, the reader of the reference's binarized format, the error cases, the host arenas.
GPU: the kernel's picks EQUAL the twin's and its batches EQUAL torch slicing of the host arenas (copies: no tolerance anywhere); the
step index comes from the device state; a captured TrainStep cuts plan(0), plan(1), plan(2) on three replays; a step fed by the corpus
equals, bit for bit, the step fed the same batch by hand.
"""
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox   # noqa: E402
import synth    # noqa: E402

import fastdiff_amd                                   # noqa: E402
from fastdiff_amd import TrainCorpus, _capi, schedules   # noqa: E402
from fastdiff_amd import corpus as corpus_mod         # noqa: E402

SEEDS = (1234, 2 ** 32 + 7, 2 ** 63 + 7)
ITS = (0, 1, 2 ** 32 + 3)
BATCHES = (1, 5, 20)
RANKS = ((0, 1), (2, 3))


def make_items(lengths, hop, seed=0, extra_wav=0):
    """Items of the given frame counts filled with torch.randn (float32), as the binarizer lays them out: mel [T, 80], wav [T hop (+ extra)]."""
    gen = torch.Generator().manual_seed(seed)
    return [{"item_name": f"utt{i:03d}", "mel": torch.randn(T, 80, generator=gen).numpy(), "wav": torch.randn(T * hop + extra_wav, generator=gen).numpy()}
            for i, T in enumerate(lengths)]


def blank_corpus(lengths, F=4, hop=4):
    return TrainCorpus([{"mel": np.zeros((T, 80), np.float32), "wav": np.zeros(T * hop, np.float32)} for T in lengths], hop_size=hop,
                       max_samples=F * hop, device="cpu")


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_train.h")).read()
    assert "fd_train_collate" in set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    assert "fd_train_collate" in _capi.EXPORTS and hasattr(_capi.load(), "fd_train_collate")
    assert "TrainCorpus" in fastdiff_amd.__all__ and (corpus_mod.PERM_STREAM, corpus_mod.START_STREAM) == (0xFFFFFFFB, 0xFFFFFFFC)
    p = inspect.signature(fastdiff_amd.TrainStep.__init__).parameters
    for name, default in (("corpus", None), ("batch_size", None), ("rank", 0), ("world_size", 1)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    assert list(p)[-4:] == ["corpus", "batch_size", "rank", "world_size"]
    q = inspect.signature(fastdiff_amd.TrainStep.step).parameters
    assert q["mels"].default is None and q["wavs"].default is None
    c = inspect.signature(TrainCorpus.__init__).parameters
    assert [c[k].default for k in ("hop_size", "max_samples", "aux_context_window", "device")] == [256, 25600, 0, None]
    from fastdiff_amd import lvc_op
    t = inspect.signature(lvc_op.train_collate).parameters
    assert list(t) == ["corpus", "batch_size", "seed", "iteration", "state", "rank", "world_size", "out"]


def test_the_twins_generator_is_the_kernels():
    """corpus.py carries its own Philox4x32-10 (the product imports nothing from oracle/): the same words as oracle/philox.py, which
    tests/test_device_noise.py pins to the published vectors and to the device."""
    pos = np.array([0, 1, 5, 2 ** 32 + 9, 2 ** 63 + 1], np.uint64)
    for seed in SEEDS:
        for uid in ITS:
            for stream in (corpus_mod.PERM_STREAM, corpus_mod.START_STREAM):
                got = corpus_mod._words(seed, stream, pos, np.uint64(uid))
                want = philox.words(seed, stream, pos, uid=uid)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (seed, uid, stream)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 1000])
def test_the_item_order_is_a_bijection_per_epoch(n):
    """The items at positions g in [e n, (e + 1) n), gathered from plan() over the ranks, are a permutation of range(n) for e = 0, 1, 2;
    from n = 5 on the three orders differ pairwise.  The order does not depend on how the positions are dealt out (B, world)."""
    c = blank_corpus([5] * n)
    for seed in SEEDS if n < 1000 else SEEDS[:1]:                      # (3 n plans per seed at B = 1: one seed at the largest n keeps the test short)
        seen = []
        for B in (1, 4):
            for world in (1, 3):
                got, it = {}, 0
                while len(got) < 3 * n + B * world:
                    for rank in range(world):
                        items, starts = c.plan(it, B, seed=seed, rank=rank, world_size=world)
                        assert items.dtype == starts.dtype == np.int64 and items.shape == starts.shape == (B,)
                        for b in range(B):
                            got[(it * B + b) * world + rank] = int(items[b])
                    it += 1
                orders = [[got[e * n + j] for j in range(n)] for e in range(3)]
                for e, order in enumerate(orders):
                    assert sorted(order) == list(range(n)), (n, seed, B, world, e)
                if n >= 5:
                    assert orders[0] != orders[1] and orders[1] != orders[2] and orders[0] != orders[2], (n, seed)
                seen.append(orders)
        assert all(o == seen[0] for o in seen[1:]), (n, seed)


@pytest.mark.parametrize("span", [1, 3, 1000])
def test_the_start_frames_stay_in_range_and_reach_both_ends(span):
    """T - F = span: every start in [0, span); span 3 reaches 0 and 2 within 4096 draws; span 1 always gives 0."""
    F = 4
    c = blank_corpus([F + span], F=F)
    for seed in SEEDS:
        starts = np.concatenate([c.plan(it, 64, seed=seed)[1] for it in range(64)])
        assert starts.shape == (4096,) and starts.min() >= 0 and starts.max() < span, (seed, span)
        if span == 3:
            assert set(starts.tolist()) == {0, 1, 2}, seed
        if span == 1:
            assert not starts.any()
    # the top of the range at a large step index: the word is a full 32 bits wide
    big = blank_corpus([F + 1000], F=F).plan(2 ** 63 + 11, 64, seed=2 ** 63 + 7)[1]
    assert big.min() >= 0 and big.max() < 1000 and big.max() > 500


def test_the_filter_keeps_what_the_reference_keeps():
    F, hop = 6, 4
    lengths = [F, F + 1, F - 1, F + 9, 1, F + 1]
    c = TrainCorpus(make_items(lengths, hop), hop_size=hop, max_samples=F * hop + 3, device="cpu")      # (F = max_samples // hop)
    assert c.frames == F and c.n_skipped == 3 and c.n_items == len(c) == 3
    assert c.kept.tolist() == [1, 3, 5] and c.lengths.tolist() == [F + 1, F + 9, F + 1]
    assert c.frame_off_host.tolist() == [0, F + 1, 2 * F + 10, 3 * F + 11] and c.frame_off.tolist() == c.frame_off_host.tolist()


def test_the_host_arenas_hold_what_was_given():
    hop, F = 8, 3
    lengths = [4, 9, 3, 5]
    items = make_items(lengths, hop, seed=3, extra_wav=5)          # (every wav 5 samples longer than T hop: trimmed)
    items[1]["mel"] = items[1]["mel"].astype(np.float64)           # (converted like torch.FloatTensor(item["mel"]))
    c = TrainCorpus(items, hop_size=hop, max_samples=F * hop, device="cpu")
    assert c.device.type == "cpu" and c.to("cpu") is c
    assert c.mel.dtype == c.wav.dtype == torch.float32 and c.frame_off.dtype == torch.int64
    assert c.mel.shape == (18, 80) and c.wav.shape == (18 * hop,)
    for k, i in enumerate(c.kept.tolist()):
        lo, hi = int(c.frame_off_host[k]), int(c.frame_off_host[k + 1])
        assert hi - lo == lengths[i]
        assert np.array_equal(c.mel[lo:hi].numpy(), items[i]["mel"].astype(np.float32))
        assert np.array_equal(c.wav[lo * hop: hi * hop].numpy(), items[i]["wav"][: lengths[i] * hop])
    mels, wavs = c.cut(*c.plan(0, 4, seed=1))
    assert mels.shape == (4, 80, F) and wavs.shape == (4, 1, F * hop)


def write_binary_set(folder, prefix, items):
    """The reference's binarized format (utils/indexed_datasets.py): concatenated pickles, an np.save'd dict of byte offsets, the lengths."""
    offsets = [0]
    with open(os.path.join(folder, prefix + ".data"), "wb") as f:
        for item in items:
            offsets.append(offsets[-1] + f.write(pickle.dumps(item)))
    with open(os.path.join(folder, prefix + ".idx"), "wb") as f:
        np.save(f, {"offsets": offsets})
    np.save(os.path.join(folder, prefix + "_lengths.npy"), np.array([len(item["mel"]) for item in items]))


def test_from_binary_dir_reads_the_reference_format(tmp_path):
    hop, F = 4, 5
    lengths = [9, 5, 6, 2, 14]
    items = make_items(lengths, hop, seed=5, extra_wav=3)
    for item in items:
        item["pitch"] = np.zeros(len(item["mel"]), np.int64)       # (fields the vocoder set also carries)
    write_binary_set(str(tmp_path), "train", items)
    write_binary_set(str(tmp_path), "valid", items[:1])
    c = TrainCorpus.from_binary_dir(str(tmp_path), hop_size=hop, max_samples=F * hop, device="cpu")
    assert c.n_items == 3 and c.n_skipped == 2 and c.kept.tolist() == [0, 2, 4] and c.lengths.tolist() == [9, 6, 14]
    direct = TrainCorpus(items, hop_size=hop, max_samples=F * hop, device="cpu")
    assert torch.equal(c.mel, direct.mel) and torch.equal(c.wav, direct.wav) and torch.equal(c.frame_off, direct.frame_off)
    assert c.wav.numel() == 29 * hop                                # (the 3 extra samples of every wav are gone)
    v = TrainCorpus.from_binary_dir(str(tmp_path), prefix="valid", hop_size=hop, max_samples=F * hop, device="cpu")
    assert v.n_items == 1 and v.n_skipped == 0


def test_wrong_inputs_raise_and_name_the_item():
    hop, F = 4, 3
    kw = dict(hop_size=hop, max_samples=F * hop, device="cpu")
    good = make_items([5, 6, 7], hop)
    with pytest.raises(NotImplementedError, match="aux_context_window"):
        TrainCorpus(good, aux_context_window=2, **kw)
    short = make_items([5, 6, 7], hop)
    short[1]["wav"] = short[1]["wav"][:-1]
    with pytest.raises(ValueError, match=r"item 1 \(utt001\).*wav"):
        TrainCorpus(short, **kw)
    for bad in (np.zeros((6, 79), np.float32), np.zeros((80,), np.float32), np.zeros((80, 6), np.float32)):
        wrong = make_items([5, 6, 7], hop)
        wrong[2]["mel"] = bad
        with pytest.raises(ValueError, match=r"item 2 \(utt002\).*mel"):
            TrainCorpus(wrong, **kw)
    with pytest.raises(ValueError, match="hop_size"):
        TrainCorpus(good, hop_size=6, max_samples=18, device="cpu")
    with pytest.raises(ValueError, match="item 0"):
        TrainCorpus(make_items([3, 2], hop), **kw)                  # (T == F and T < F: nothing left)
    with pytest.raises(ValueError, match="item 0"):
        TrainCorpus([], **kw)
    c = TrainCorpus(good, **kw)
    for bad_plan in (dict(batch_size=0), dict(batch_size=2, rank=3, world_size=3), dict(batch_size=2, world_size=0)):
        with pytest.raises(ValueError):
            c.plan(0, **bad_plan)
    from fastdiff_amd import lvc_op
    with pytest.raises(RuntimeError, match="HIP device"):
        lvc_op.train_collate(c, 2)                                  # (a corpus on the CPU does everything but feed the kernel)


# ------------------------------------------------------------------------------------------------------------------ GPU
SHAPES = ((256, 1), (256, 7), (256, 100), (4, 7))                  # (hop, F): a tile tail of every kind; hop 4 = the smallest vector copy
KINDS = ("one", "three", "many")


def _lengths(kind, F):
    if kind == "one":
        return [F + 1]
    if kind == "three":
        return [F + 1, F + 23, F + 4]
    rng = np.random.RandomState(F)
    return (F + 1 + rng.randint(0, 40, size=65)).tolist()


def _cases():
    """Two calls per (shape, corpus): 24 of the product, every value of every axis several times over."""
    out = []
    for s, (hop, F) in enumerate(SHAPES):
        for k, kind in enumerate(KINDS):
            for v in range(2):
                c = 2 * (3 * s + k) + v
                out.append((hop, F, kind, BATCHES[(c + s + 1) % 3], ITS[(c // 2 + v) % 3], SEEDS[(c // 3 + k) % 3], RANKS[(c + k + s) % 2]))
    return out


def test_the_gpu_cases_cover_every_axis():
    cases = _cases()
    assert len(cases) == 24
    for axis, values in ((3, BATCHES), (4, ITS), (5, SEEDS), (6, RANKS)):
        for hop, F in SHAPES:                                       # ... at every shape
            assert {c[axis] for c in cases if c[:2] == (hop, F)} == set(values), (axis, hop, F)
    assert (256, 100, "many", 20) in {c[:4] for c in cases}          # the training shape itself


def host_batch(cpu, items, starts):
    """The reference's collater on given picks: torch slicing of the host arenas."""
    F, hop = cpu.frames, cpu.hop_size
    first = [int(cpu.frame_off_host[i]) + int(s) for i, s in zip(items, starts)]
    mels = torch.stack([cpu.mel[p: p + F].transpose(0, 1) for p in first])
    wavs = torch.stack([cpu.wav[p * hop: (p + F) * hop].view(1, -1) for p in first])
    return mels.contiguous(), wavs.contiguous()


@pytest.fixture(scope="module")
def corpora():
    made = {}

    def get(hop, F, kind):
        if (hop, F, kind) not in made:
            cpu = TrainCorpus(make_items(_lengths(kind, F), hop, seed=F), hop_size=hop, max_samples=F * hop, device="cpu")
            made[(hop, F, kind)] = (cpu, cpu.to("cuda"))
        return made[(hop, F, kind)]
    return get


@pytest.mark.gpu
def test_batches_are_exact(corpora):
    from fastdiff_amd import lvc_op
    for hop, F, kind, B, it, seed, (rank, world) in _cases():
        cpu, dev = corpora(hop, F, kind)
        assert dev.device.type == "cuda" and dev.wav.is_cuda and dev.n_items == cpu.n_items and cpu.device.type == "cpu"
        tag = (hop, F, kind, B, it, seed, rank, world)
        mels, wavs, picked = lvc_op.train_collate(dev, B, seed=seed, iteration=it, rank=rank, world_size=world)
        items, starts = cpu.plan(it, B, seed=seed, rank=rank, world_size=world)
        assert picked.shape == (B, 2) and picked.dtype == torch.int64
        got = picked.cpu().numpy()
        assert np.array_equal(got[:, 0], items) and np.array_equal(got[:, 1], starts), (tag, got.tolist(), items.tolist(), starts.tolist())
        assert (starts >= 0).all() and (starts + F <= cpu.lengths[items]).all()
        want_mels, want_wavs = host_batch(cpu, items, starts)
        assert mels.shape == (B, 80, F) and wavs.shape == (B, 1, F * hop)
        assert torch.equal(wavs.cpu(), want_wavs), tag
        assert torch.equal(mels.cpu(), want_mels), tag
    # into given buffers, and twice the same
    cpu, dev = corpora(256, 100, "many")
    out = (torch.zeros(20, 80, 100, device="cuda"), torch.zeros(20, 1, 25600, device="cuda"), torch.zeros(20, 2, dtype=torch.int64, device="cuda"))
    back = lvc_op.train_collate(dev, 20, seed=5, iteration=9, out=out)
    assert all(a is b for a, b in zip(back, out))
    again = lvc_op.train_collate(dev, 20, seed=5, iteration=9)
    assert all(torch.equal(a, b) for a, b in zip(back, again))
    other = lvc_op.train_collate(dev, 20, seed=5, iteration=10)
    assert not torch.equal(other[2], back[2])


@pytest.mark.gpu
def test_the_device_state_beats_the_host_iteration(corpora):
    from fastdiff_amd import lvc_op
    cpu, dev = corpora(256, 7, "many")
    st = lvc_op.new_train_state("cuda")
    st[0] = 5
    mels, wavs, picked = lvc_op.train_collate(dev, 5, seed=1234, iteration=0, state=st)
    items, starts = cpu.plan(5, 5, seed=1234)
    assert np.array_equal(picked.cpu().numpy(), np.stack([items, starts], axis=1))
    want_mels, want_wavs = host_batch(cpu, items, starts)
    assert torch.equal(mels.cpu(), want_mels) and torch.equal(wavs.cpu(), want_wavs)
    assert not np.array_equal(np.stack(cpu.plan(0, 5, seed=1234), axis=1), picked.cpu().numpy())
    assert lvc_op.read_train_state(st)["iter"] == 5                  # only read


# ---- TrainStep: the smallest batch shape of tests/test_train_step.py's end-to-end case (B = 2, 6 frames of 256 samples)
STEP_B, STEP_F, STEP_HOP = 2, 6, 256


def step_corpus():
    lengths = [7, 19, 8, 12, 30]
    mel = synth.synth_mel(3, 1, sum(lengths))[0].T                   # [sum T, 80]: values of the range the model is fed in the other tests
    gen = torch.Generator().manual_seed(11)
    items, at = [], 0
    for T in lengths:
        items.append({"mel": np.ascontiguousarray(mel[at: at + T]), "wav": (0.3 * torch.randn(T * STEP_HOP, generator=gen)).numpy()})
        at += T
    return TrainCorpus(items, hop_size=STEP_HOP, max_samples=STEP_F * STEP_HOP, device="cpu")


@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.mark.gpu
def test_a_captured_step_cuts_a_new_batch_on_every_replay(gc):
    import math
    cpu = step_corpus()
    dh = schedules.training_hyperparams()
    seed = 2 ** 32 + 7
    ts = fastdiff_amd.TrainStep(gc.make_model().train(), dh, seed=seed, corpus=cpu.to("cuda"), batch_size=STEP_B, graph=True)
    assert ts.picked.shape == (STEP_B, 2) and ts.picked.dtype == torch.int64 and ts.picked.is_cuda
    graphs, plans = set(), []
    for k in range(3):
        loss = ts.step()
        graphs.add(id(ts._graph))
        torch.cuda.synchronize()
        assert ts._graph is not None and math.isfinite(float(loss))
        items, starts = cpu.plan(k, STEP_B, seed=seed)
        assert np.array_equal(ts.picked.cpu().numpy(), np.stack([items, starts], axis=1)), k
        want_mels, want_wavs = host_batch(cpu, items, starts)
        assert torch.equal(ts.mel.cpu(), want_mels) and torch.equal(ts.wav.cpu(), want_wavs), k
        plans.append(ts.picked.cpu().numpy().tolist())
    assert len(graphs) == 1, "captured once, replayed three times"
    assert plans[0] != plans[1] and plans[1] != plans[2] and plans[0] != plans[2]
    st = ts.state()
    assert st["iter"] == 3 and st["applied"] == 3 and st["skipped"] == 0, st


@pytest.mark.gpu
def test_a_step_from_the_corpus_equals_the_step_fed_by_hand(gc):
    """Same kernels on the same bits with fixed-order sums: the loss and every parameter are equal, not close."""
    cpu = step_corpus()
    dh = schedules.training_hyperparams()
    a = fastdiff_amd.TrainStep(gc.make_model().train(), dh, seed=1234, graph=False, corpus=cpu.to("cuda"), batch_size=STEP_B)
    b = fastdiff_amd.TrainStep(gc.make_model().train(), dh, seed=1234, graph=False)
    before = [p.detach().clone() for p in a.params]
    loss_a = a.step().clone()
    mels, wavs = host_batch(cpu, *cpu.plan(0, STEP_B, seed=1234))
    loss_b = b.step(mels.cuda(), wavs.cuda()).clone()
    torch.cuda.synchronize()
    assert torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    names = [n for n, _ in a.model.named_parameters()]
    for n, p, q in zip(names, a.params, b.params):
        assert torch.equal(p, q), (n, float((p - q).abs().max()))
    assert any(not torch.equal(p, q) for p, q in zip(a.params, before)), "the step moved the parameters"
    assert a.state() == b.state()


@pytest.mark.gpu
def test_wrong_calls_and_the_unchanged_path(gc):
    cpu = step_corpus()
    dh = schedules.training_hyperparams()
    plain = fastdiff_amd.TrainStep(gc.make_model().train(), dh, seed=7, graph=False)
    with pytest.raises(RuntimeError, match="corpus"):
        plain.step()
    with pytest.raises(ValueError, match="batch_size"):
        fastdiff_amd.TrainStep(plain.model, dh, corpus=cpu.to("cuda"))
    with pytest.raises(RuntimeError, match="corpus lies on"):
        fastdiff_amd.TrainStep(plain.model, dh, corpus=cpu, batch_size=STEP_B)
    both = fastdiff_amd.TrainStep(gc.make_model().train(), dh, seed=7, graph=False, corpus=cpu.to("cuda"), batch_size=STEP_B)
    with pytest.raises(TypeError):
        both.step(torch.zeros(2, 80, 6, device="cuda"))
    mel = torch.from_numpy(synth.synth_mel(3, 2, 6)).cuda()
    wav = (0.3 * gc.hash_normal_torch(3, 1, 2 * 6 * 256)).view(2, 1, 6 * 256)
    for k in range(2):                                               # the second call as well: the existing path's result
        la, lb = both.step(mel, wav).clone(), plain.step(mel, wav).clone()
        assert torch.equal(la, lb), k
    for p, q in zip(both.params, plain.params):
        assert torch.equal(p, q)
    assert both.state() == plain.state() and both.state()["iter"] == 2
    both.step()                                                      # and the two modes alternate on one TrainStep
    assert np.array_equal(both.picked.cpu().numpy(), np.stack(cpu.plan(2, STEP_B, seed=7), axis=1))
