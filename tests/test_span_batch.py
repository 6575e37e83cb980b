"""Many utterances per window batch (fd_sample_spans_plan, fd_sample_spans, fd_mel_ring_append; FastDiff.sample_long_batch, stream_pool).

CPU: the planner that fd_sample_spans runs equals a twin written here on a few hundred random span sets, and refuses per span what
fd_sample_span refuses.  GPU: every comparison is torch.equal -- an utterance vocoded in a batch shared with others, or a stream of a
pool fed through a ring, gets the bits of its own single-utterance call."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 256
MAX_WINDOWS, BATCH_FRAMES = 32, 16384


def _capi():
    from fastdiff_amd import _capi
    return _capi


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound():
    import fastdiff_amd
    capi = _capi()
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = capi.load()
    for name in ("fd_sample_spans_plan", "fd_sample_spans", "fd_mel_ring_append"):
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    for struct in ("fd_span", "fd_span_window", "fd_ring_chunk"):
        assert re.search(r"typedef struct %s\b" % struct, header), struct
    assert lib.fd_sample_spans(None, None, 0, None, 4, 0, 0, 0, None) == capi.FD_ERR_INVALID
    assert lib.fd_mel_ring_append(None, None, 0, None) == capi.FD_ERR_INVALID
    for method in ("sample_long_batch", "stream_pool"):
        assert callable(getattr(fastdiff_amd.FastDiff, method)), method
    for method in ("open", "feed", "close", "step"):
        assert callable(getattr(fastdiff_amd.StreamPool, method)), method
    for text in ("distinct stream_ids", "must not overlap", "redone as a whole", "calls_redone", "span_batches", "span_windows"):
        assert text in header, text


def test_struct_sizes_match_the_header():
    """fd_span: 2 pointers + 8 x 64 bit; fd_span_window: 4 x int32 + 2 x int64; fd_ring_chunk: 2 pointers + 5 x int64."""
    capi = _capi()
    assert ct.sizeof(capi.FdSpan) == 80 and capi.FdSpan.stream_id.offset == 64 and capi.FdSpan.out.offset == 72
    assert ct.sizeof(capi.FdSpanWindow) == 32 and capi.FdSpanWindow.start.offset == 16 and capi.FdSpanWindow.c0.offset == 24
    assert ct.sizeof(capi.FdRingChunk) == 56 and capi.FdRingChunk.src.offset == 32 and capi.FdRingChunk.frames.offset == 48


def _ceil32(v):
    return (v + 31) // 32 * 32


def _twin_plan(spans, N, wf):
    """The plan as the header states it: [(span, batch, len, clen, start, c0)], Wp."""
    H = 16 * N
    C = wf if wf else _ceil32(max(1024, 4 * H)) - 2 * H
    Wp = _ceil32(_ceil32(H) + min(C, _ceil32(max(s["t1"] - s["t0"] for s in spans))) + H)
    Bw = min(MAX_WINDOWS, max(1, BATCH_FRAMES // Wp))
    wins = []
    for i, s in enumerate(spans):
        for c0 in range(s["t0"], s["t1"], C):
            ce = min(c0 + C, s["t1"])
            ws = max(0, (c0 - H) // 32 * 32)
            we = min(s["utt_frames"], ce + H) if s["utt_frames"] >= 0 else ce + H
            wins.append((i, len(wins) // Bw, we - ws, ce - c0, ws, c0))
    return wins, Wp


def _c_spans(spans):
    capi = _capi()
    arr = (capi.FdSpan * max(1, len(spans)))()
    for i, s in enumerate(spans):
        cap = s.get("mel_cap", 0)
        arr[i] = capi.FdSpan(None, s.get("mel_pitch", cap or s["mel_frames"]), cap, s["mel_first"], s["mel_frames"], s["utt_frames"], s["t0"], s["t1"],
                             i, None)
    return arr


def _c_plan(spans, N, wf, room=None):
    """fd_sample_spans_plan: ([(span, batch, len, clen, start, c0)], Wp), or its negative status."""
    capi = _capi()
    lib = capi.load()
    arr = _c_spans(spans)
    wp = ct.c_int(-7)
    n = lib.fd_sample_spans_plan(arr, len(spans), N, wf, None, 0, ct.byref(wp))
    if n < 0:
        return n
    wins = (capi.FdSpanWindow * max(1, n))()
    assert lib.fd_sample_spans_plan(arr, len(spans), N, wf, wins, n if room is None else room, ct.byref(wp)) == n
    return [(w.span, w.batch, w.len, w.clen, w.start, w.c0) for w in wins[:n if room is None else min(n, room)]], wp.value


def _random_span(rng, N):
    H = 16 * N
    t0 = 0 if rng.integers(3) == 0 else 32 * int(rng.integers(1, 60))
    if rng.integers(2):                                     # the utterance's length is known
        utt = t0 + int(rng.integers(1, 3000 if rng.integers(4) else 40))
        t1 = utt if rng.integers(2) or utt - t0 < 32 else t0 + 32 * int(rng.integers(1, (utt - t0) // 32 + 1))
        need_hi = min(utt, t1 + H)
        hi = int(rng.integers(need_hi, utt + 1))
    else:
        utt = -1
        t1 = t0 + 32 * int(rng.integers(1, 90 if rng.integers(4) else 3))
        need_hi = t1 + H
        hi = need_hi + int(rng.integers(0, 100))
    need_lo = max(0, t0 - H)
    lo = int(rng.integers(0, need_lo + 1)) if rng.integers(2) else need_lo
    s = {"mel_first": lo, "mel_frames": hi - lo, "utt_frames": utt, "t0": t0, "t1": t1}
    if rng.integers(2):
        s["mel_cap"] = hi - lo + int(rng.integers(0, 64))
    return s


def test_plan_equals_its_python_twin_on_random_span_sets():
    rng = np.random.default_rng(20240917)
    seen_second_batch = seen_short = seen_ragged_end = seen_t0 = 0
    for trial in range(400):
        N = int(rng.choice((1, 3, 4, 8)))
        wf = int(rng.choice((32, 64, 256, 0)))
        H = 16 * N
        spans = [_random_span(rng, N) for _ in range(int(rng.integers(1, 12)))]
        got = _c_plan(spans, N, wf)
        assert not isinstance(got, int), (trial, got, spans)
        wins, Wp = got
        twin, twin_Wp = _twin_plan(spans, N, wf)
        assert (wins, Wp) == (twin, twin_Wp), (trial, N, wf)
        C = wf if wf else _ceil32(max(1024, 4 * H)) - 2 * H
        # every frame of every span lies in exactly one centre
        for i, s in enumerate(spans):
            mine = [w for w in wins if w[0] == i]
            pos = s["t0"]
            for _, _, _, clen, _, c0 in mine:
                assert c0 == pos and 0 < clen <= C
                pos += clen
            assert pos == s["t1"]
            seen_short += s["t1"] - s["t0"] < C
            seen_ragged_end += s["t1"] % 32 != 0
            seen_t0 += s["t0"] > 0
        per_batch = {}
        last = 0
        for span, batch, ln, clen, start, c0 in wins:
            assert start % 32 == 0 and start == max(0, (c0 - H) // 32 * 32)
            assert 0 < ln <= Wp and c0 - start + clen <= ln
            assert batch in (last, last + 1)                # non-decreasing, none left out
            last = batch
            per_batch[batch] = per_batch.get(batch, 0) + 1
        assert wins[0][1] == 0
        assert Wp % 32 == 0 and Wp <= _ceil32(_ceil32(H) + C + H)
        for n in per_batch.values():
            assert n <= MAX_WINDOWS and (n * Wp <= BATCH_FRAMES or n == 1)
        seen_second_batch += len(per_batch) > 1
    assert min(seen_second_batch, seen_short, seen_ragged_end, seen_t0) > 20


def test_plan_wp_follows_the_centre_needed():
    """32 one-chunk stream windows at N = 4 are 160 padded frames each, not the default's 1024."""
    spans = [{"mel_first": 0, "mel_frames": 96, "utt_frames": -1, "t0": 0, "t1": 32} for _ in range(32)]
    wins, Wp = _c_plan(spans, 4, 0)
    assert Wp == 64 + 32 + 64 and len(wins) == 32 and {w[1] for w in wins} == {0}
    spans[5] = {"mel_first": 0, "mel_frames": 5000, "utt_frames": 5000, "t0": 0, "t1": 5000}
    wins, Wp = _c_plan(spans, 4, 0)
    assert Wp == 1024 and max(w[1] for w in wins) == (len(wins) - 1) // 16


def test_plan_fills_no_more_than_the_room_given():
    spans = [{"mel_first": 0, "mel_frames": 700, "utt_frames": 700, "t0": 0, "t1": 700}]
    full, Wp = _c_plan(spans, 4, 32)
    part, Wp2 = _c_plan(spans, 4, 32, room=5)
    assert len(full) == 22 and part == full[:5] and Wp == Wp2


GOOD = {"mel_first": 0, "mel_frames": 400, "utt_frames": 400, "t0": 0, "t1": 400}
REFUSED = {
    "t0 misaligned": dict(GOOD, t0=16),
    "t1 misaligned and not the end": dict(GOOD, t1=100),
    "t1 past the utterance": dict(GOOD, mel_frames=400, t1=432),
    "empty": dict(GOOD, t0=64, t1=64),
    "negative t0": dict(GOOD, t0=-32),
    "utt_frames 0": dict(GOOD, utt_frames=0),
    "utt_frames -2": dict(GOOD, utt_frames=-2),
    "mel_first negative": dict(GOOD, mel_first=-1),
    "no mel": dict(GOOD, mel_frames=0),
    "mel past the utterance": dict(GOOD, mel_frames=401),
    "mel starts inside the halo of t0": {"mel_first": 100, "mel_frames": 300, "utt_frames": 400, "t0": 128, "t1": 256},
    "mel ends inside the halo of t1": {"mel_first": 0, "mel_frames": 300, "utt_frames": 400, "t0": 0, "t1": 256},
    "streaming: t1 + H past the mel": {"mel_first": 0, "mel_frames": 400, "utt_frames": -1, "t0": 0, "t1": 352},
    "ring smaller than its frames": dict(GOOD, mel_cap=399),
    "negative ring": dict(GOOD, mel_cap=-1, mel_pitch=400),
    "pitch shorter than a row": dict(GOOD, mel_pitch=399),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_plan_refuses_per_span(why):
    capi = _capi()
    bad = REFUSED[why]
    assert not isinstance(_c_plan([GOOD, GOOD, GOOD], 4, 0), int)
    assert _c_plan([bad], 4, 0) == capi.FD_ERR_INVALID
    assert _c_plan([GOOD, GOOD, bad], 4, 0) == capi.FD_ERR_INVALID
    assert _c_plan([GOOD, bad, GOOD], 4, 32) == capi.FD_ERR_INVALID


def test_plan_refuses_bad_call_parameters_and_takes_no_spans():
    capi = _capi()
    for N, wf in ((0, 0), (1025, 0), (4, 48), (4, -32)):
        assert _c_plan([GOOD], N, wf) == capi.FD_ERR_INVALID
    assert _c_plan([], 4, 0) == ([], 0)
    assert capi.load().fd_sample_spans_plan(None, 0, 4, 0, None, 0, None) == 0
    assert capi.load().fd_sample_spans_plan(None, 2, 4, 0, None, 0, None) == capi.FD_ERR_INVALID


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def model(gc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gc.make_model()


@pytest.fixture(scope="module")
def sched():
    return load_golden("schedule")


@pytest.fixture(scope="module")
def rows4(gc, sched):
    return gc.table_rows(sched, 4)[0]


def _mel(seed, T):
    import synth
    return torch.from_numpy(synth.synth_mel(seed, 1, T)).cuda()


def _no_handover(model, redone_before):
    assert model.counter("calls_redone") == redone_before
    assert model.counter("pieces_redone") == 0
    assert not model.read_tap("range_flags_call").view(np.int32).any()


def _span_of(mel, first, last, utt, t0, t1, sid, out=None):
    """A plain-buffer span over mel[:, :, first:last] of an utterance (a dict for longform.sample_spans)."""
    out = torch.empty(((t1 - t0) * HOP,), device="cuda") if out is None else out
    return {"mel": mel[0, :, first:last].contiguous(), "out": out, "mel_first": first, "mel_frames": last - first, "utt_frames": utt,
            "t0": t0, "t1": t1, "stream_id": sid}


def _alone(model, s, rows, **kw):
    """The span's own fd_sample_span call."""
    from fastdiff_amd import longform
    return longform.sample_span(model, s["mel"], s["mel_first"], s["utt_frames"], s["t0"], s["t1"], rows, stream_id=s["stream_id"], **kw).reshape(-1)


LENGTHS = (1, 70, 333, 700, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("N,wf,ddim", [(4, 32, False), (4, 32, True), (3, None, False)], ids=["ddpm_w32", "ddim_w32", "N3_default"])
def test_sample_long_batch_equals_sample_long_per_utterance(model, gc, sched, N, wf, ddim):
    """One frame, ragged last windows, an exact multiple of the centre; at 32-frame centres the five utterances make 39 windows, so an
    utterance continues in a second batch.  span_batches rises by the plan's batch count -- not by one call or more per utterance."""
    from fastdiff_amd import longform
    rows, _ = gc.table_rows(sched, N)
    mels = [_mel(50 + i, T) for i, T in enumerate(LENGTHS)]
    sids = [900 + 7 * i for i in range(len(mels))]
    plan, _ = _c_plan([{"mel_first": 0, "mel_frames": T, "utt_frames": T, "t0": 0, "t1": T} for T in LENGTHS], N, wf or 0)
    n_batches = plan[-1][1] + 1
    assert n_batches == (2 if wf == 32 else 1)
    with torch.no_grad():
        refs = [model.sample_long(m, rows, ddim=ddim, seed=5, stream_id=sid, window_frames=wf) for m, sid in zip(mels, sids)]
        redone = model.counter("calls_redone")
        batches, windows = model.counter("span_batches"), model.counter("span_windows")
        ys = model.sample_long_batch([mels[0][0]] + mels[1:], rows, ddim=ddim, seed=5, stream_ids=sids, window_frames=wf)
    assert model.counter("span_batches") - batches == n_batches and model.counter("span_windows") - windows == len(plan)
    assert len(ys) == len(refs)
    for T, y, ref in zip(LENGTHS, ys, refs):
        assert y.shape == ref.shape == (1, 1, T * HOP)
        assert torch.equal(y, ref), (T, float((y - ref).abs().max()))
    _no_handover(model, redone)
    assert longform.sample_long_batch(model, [], rows) == []


@pytest.mark.gpu
def test_mixed_raw_spans_in_one_call(model, rows4):
    """A first span whose utterance's end is not known, a middle span whose mel starts at frame 32, a closing span up to
    utt_frames = 205: each equals its own fd_sample_span call."""
    from fastdiff_amd import longform
    a, b, c = _mel(61, 300), _mel(62, 400), _mel(63, 205)
    spans = [_span_of(a, 0, 192, -1, 0, 128, 11), _span_of(b, 32, 300, -1, 96, 224, 12), _span_of(c, 64, 205, 205, 128, 205, 13)]
    with torch.no_grad():
        refs = [_alone(model, s, rows4, seed=9) for s in spans]
        redone = model.counter("calls_redone")
        longform.sample_spans(model, spans, rows4, seed=9)
    for s, ref in zip(spans, refs):
        assert torch.equal(s["out"], ref), (s["t0"], s["t1"])
    _no_handover(model, redone)


@pytest.mark.gpu
def test_a_span_does_not_depend_on_what_shares_its_call(model, rows4):
    from fastdiff_amd import longform
    mel = _mel(64, 333)
    others = [_mel(70 + i, T) for i, T in enumerate((40, 517, 96, 150))]

    def run(position):
        mine = _span_of(mel, 0, 333, 333, 0, 333, 77)
        rest = [_span_of(m, 0, m.shape[-1], m.shape[-1], 0, m.shape[-1], 200 + i) for i, m in enumerate(others)]
        spans = {"alone": [mine], "first": [mine] + rest, "last": rest + [mine]}[position]
        with torch.no_grad():
            longform.sample_spans(model, spans, rows4, seed=4, window_frames=64)
        return mine["out"]

    redone = model.counter("calls_redone")
    alone, first, last = run("alone"), run("first"), run("last")
    assert torch.equal(alone, first) and torch.equal(alone, last)
    with torch.no_grad():
        assert torch.equal(alone, model.sample_long(mel, rows4, seed=4, stream_id=77).reshape(-1))
    _no_handover(model, redone)


def _drive_pool(model, pool, rows, plan, seed, rng, max_chunk, H, chunk=32):
    """plan: [(open at round, stream id, mel)].  Every round: open what is due (when a slot is free), feed each open stream one chunk
    of 1..max_chunk frames, close the ones fed completely, step().  Returns {stream id: concatenated pieces} and, per stream id, (its
    slot, the round it was opened in, whether a closed stream had left that slot)."""
    live, pieces, fed, got, slots, left = {}, {}, {}, {}, {}, set()
    waiting = list(plan)
    rnd = 0
    while waiting or live:
        for item in [w for w in waiting if w[0] <= rnd]:
            if not pool._free:
                break
            _, sid, mel = item
            waiting.remove(item)
            s = pool.open(sid)
            live[s] = (sid, mel)
            pieces[sid], fed[s], got[s] = [], 0, 0
            slot = pool._streams[s].slot
            assert slot not in [pool._streams[o].slot for o in live if o != s]
            slots[sid] = (slot, rnd, slot in left)
        for s, (sid, mel) in live.items():
            T = mel.shape[-1]
            if fed[s] < T:
                t = int(min(T - fed[s], rng.integers(1, max_chunk + 1)))
                pool.feed(s, mel[0, :, fed[s]:fed[s] + t] if rng.integers(2) else mel[:, :, fed[s]:fed[s] + t])
                fed[s] += t
                if fed[s] == T:
                    pool.close(s)
        res = pool.step()
        for s, y in res.items():
            assert y.dim() == 1 and y.numel() % HOP == 0 and y.numel() > 0
            pieces[live[s][0]].append(y)
            got[s] += y.numel() // HOP
        for s in list(live):
            T = live[s][1].shape[-1]
            if fed[s] == T:                                   # closed: this step returned its rest and freed its slot
                assert got[s] == T and s not in pool._streams
                left.add(slots[live[s][0]][0])
                del live[s]
            else:
                assert got[s] % chunk == 0 and got[s] >= fed[s] - H - chunk + 1, (live[s][0], fed[s], got[s])
        rnd += 1
        assert rnd < 1000
    return {sid: torch.cat(p) for sid, p in pieces.items()}, slots


@pytest.mark.gpu
def test_stream_pool_rings_equal_sample_long(model, rows4):
    """Five streams of 1, 63, 64, 301 and 777 frames through three ring slots of 224 columns, fed in random chunks of 1..64 frames
    between steps; later streams are opened into the slots that closed ones left, and the longest wraps its ring three times."""
    H = model.halo_frames(4)
    pool = model.stream_pool(rows4, seed=21, chunk_frames=32, max_streams=3, max_feed_frames=64)
    assert pool.cap == 224 and 777 // pool.cap >= 3
    lengths = {301: 1, 302: 63, 303: 777, 304: 64, 305: 301}
    mels = {sid: _mel(sid % 89, T) for sid, T in lengths.items()}
    plan = [(0, 301, mels[301]), (0, 302, mels[302]), (1, 303, mels[303]), (2, 304, mels[304]), (3, 305, mels[305])]
    with torch.no_grad():
        refs = {sid: model.sample_long(m, rows4, seed=21, stream_id=sid).reshape(-1) for sid, m in mels.items()}
        redone = model.counter("calls_redone")
        out, slots = _drive_pool(model, pool, rows4, plan, 21, np.random.default_rng(77), 64, H)
    assert len({rnd for _, rnd, _ in slots.values()}) >= 3                 # opened at different steps
    assert sum(reopened for _, _, reopened in slots.values()) >= 2         # ... two or more into slots that closed streams just left
    for sid in lengths:
        assert torch.equal(out[sid], refs[sid]), (sid, lengths[sid])
    _no_handover(model, redone)
    assert not pool._streams and len(pool._free) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 3])
def test_a_reused_slot_shows_nothing_of_the_stream_before(model, gc, sched, N):
    """The only slot first holds a stream of mel at +1.5 everywhere, then a shorter stream: the columns behind the second stream's
    frames, and (N = 3: window starts 16 frames in front of the frames still held) the columns in front of them, count as zeros."""
    rows, _ = gc.table_rows(sched, N)
    H = model.halo_frames(N)
    pool = model.stream_pool(rows, seed=2, chunk_frames=32, max_streams=1, max_feed_frames=64)
    hot = torch.full((1, 80, 300), 1.5, device="cuda")
    mel = _mel(31, 150)
    with torch.no_grad():
        ref = model.sample_long(mel, rows, seed=2, stream_id=8).reshape(-1)
        redone = model.counter("calls_redone")
        rng = np.random.default_rng(5)
        out, slots = _drive_pool(model, pool, rows, [(0, 7, hot), (1, 8, mel)], 2, rng, 64, H)      # 8 waits for the only slot
        assert bool((pool.arena[0, :, 150:] == 1.5).all())      # the columns that 8 did not write are still stale
    assert slots[8][0] == 0 and slots[8][2] and torch.equal(out[8], ref)
    _no_handover(model, redone)


@pytest.mark.gpu
def test_one_call_per_pool_step(gc, rows4):
    """Eight streams with one 32-frame chunk ready each: one fd_sample of eight windows between one gather and one scatter launch."""
    m = gc.make_model()
    m.set_option("graph", "0")
    H = m.halo_frames(4)
    pool = m.stream_pool(rows4, seed=1, chunk_frames=32, max_streams=8)
    mels = [_mel(80 + i, H + 32) for i in range(8)]
    with torch.no_grad():
        handles = [pool.open(40 + i) for i in range(8)]
        for s, mel in zip(handles, mels):
            pool.feed(s, mel)
        pool._flush()
        m.set_option("profile", "1")
        try:
            m.profile(reset=True)
            batches, windows = m.counter("span_batches"), m.counter("span_windows")
            res = pool.step()
            launched = m.profile(reset=True)
        finally:
            m.set_option("profile", "0")
        assert m.counter("span_batches") - batches == 1 and m.counter("span_windows") - windows == 8
        assert launched["spans_gather"][0] == 1 and launched["spans_scatter"][0] == 1
        assert "span_gather" not in launched and "span_scatter" not in launched
        assert sorted(res) == sorted(handles)
        for i, s in enumerate(handles):
            assert torch.equal(res[s], m.stream(rows4, seed=1, stream_id=40 + i).push(mels[i]))
        assert pool.step() == {}                              # nothing became ready: no call
        assert m.counter("span_batches") - batches == 1 + 8   # (the eight SampleStream pushes above)


@pytest.mark.gpu
def test_unaligned_output_goes_element_by_element(model, rows4):
    from fastdiff_amd import longform
    mel = _mel(66, 205)
    big = torch.full((205 * HOP + 8,), -7.0, device="cuda")
    aligned = _span_of(mel, 0, 205, 205, 0, 205, 3)
    shifted = _span_of(mel, 0, 205, 205, 0, 205, 3, out=big[1:1 + 205 * HOP])
    assert aligned["out"].data_ptr() % 16 == 0 and shifted["out"].data_ptr() % 16 == 4
    with torch.no_grad():
        redone = model.counter("calls_redone")
        longform.sample_spans(model, [aligned, shifted], rows4, seed=6, window_frames=64)
    assert torch.equal(aligned["out"], shifted["out"])
    assert float(big[0]) == -7.0 and bool((big[1 + 205 * HOP:] == -7.0).all())
    _no_handover(model, redone)


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable(model, gc, rows4):
    import fastdiff_amd
    from fastdiff_amd import longform
    capi = _capi()
    mel = _mel(3, 400)
    good = lambda: [_span_of(mel, 0, 400, 400, 0, 400, i) for i in range(3)]      # noqa: E731

    def works():
        spans = good()
        longform.sample_spans(model, spans, rows4, window_frames=256)
        assert torch.equal(spans[0]["out"], model.sample_long(mel, rows4, stream_id=0).reshape(-1))

    with torch.no_grad():
        works()
        g = fastdiff_amd.FastDiff(upsample_ratios=[8, 8, 2, 2]).cuda().eval()
        with pytest.raises(NotImplementedError, match="architecture"):
            g.sample_long_batch([mel], rows4)
        model.set_option("kernels.lvc", "naive")
        try:
            with pytest.raises(NotImplementedError, match="naive"):
                model.sample_long_batch([mel], rows4)
        finally:
            model.set_option("kernels", "fast")
        works()
        spans = good()
        spans[1].update(mel_cap=399)
        with pytest.raises(AssertionError, match="ring of mel_cap=399 columns of span 1"):
            longform.sample_spans(model, spans, rows4)
        spans = good()
        spans[2] = _span_of(mel, 0, 400, 400, 16, 400, 2)
        with pytest.raises(AssertionError, match="of span 2 must be non-empty with t0 a multiple of 32"):
            longform.sample_spans(model, spans, rows4)
        spans = good()
        spans[1] = _span_of(mel, 100, 400, 400, 128, 256, 1)
        with pytest.raises(AssertionError, match="of span 1 need mel"):
            longform.sample_spans(model, spans, rows4)
        works()
        pool = model.stream_pool(rows4, max_streams=2, max_feed_frames=64)
        s = pool.open(1)
        pool.feed(s, mel[:, :, :200])
        with pytest.raises(AssertionError, match=r"cap = 224 .*step\(\) first"):
            pool.feed(s, mel[:, :, 200:225])
        assert pool.step()[s].numel() == 128 * HOP            # the refused feed changed nothing: 200 frames, 136 ready, four chunks
        lib, h = model._ready(mel.device)
        ring = torch.zeros((80, 64), device="cuda")
        chunk = capi.FdRingChunk(ring.data_ptr(), 64, 64, 0, mel.data_ptr(), 400, 65)
        assert lib.fd_mel_ring_append(h, ct.byref(chunk), 1, None) == capi.FD_ERR_INVALID
        assert b"the ring holds 64" in lib.fd_last_error(h)
        works()


@pytest.mark.gpu
def test_ring_append_alone(model):
    """Three chunks into two rings in one launch, one of them wrapping; the rest of the rings untouched."""
    capi = _capi()
    lib, h = model._ready(torch.device("cuda", torch.cuda.current_device()))
    g = torch.Generator(device="cuda").manual_seed(3)
    rings = torch.rand((2, 80, 96), device="cuda", generator=g)          # pitch 96, cap 80 and 96
    srcs = [torch.rand((80, n + 3), device="cuda", generator=g) for n in (50, 7, 33)]
    want = rings.clone()
    jobs = [(0, 80, 60, srcs[0], 50), (1, 96, 5, srcs[1], 7), (1, 96, 96 + 20, srcs[2], 33)]      # (ring, cap, first_frame, src, frames)
    chunks = (capi.FdRingChunk * 3)()
    for i, (r, cap, first, src, n) in enumerate(jobs):
        chunks[i] = capi.FdRingChunk(rings[r].data_ptr(), 96, cap, first, src.data_ptr(), src.stride(0), n)
        want[r][:, (first + torch.arange(n, device="cuda")) % cap] = src[:, :n]
    assert (60 + 50) > 80                                                 # the first chunk wraps
    rc = lib.fd_mel_ring_append(h, chunks, 3, model._stream(rings.device))
    capi.check(lib, h, rc, "fd_mel_ring_append")
    assert torch.equal(rings, want)
    assert lib.fd_mel_ring_append(h, chunks, 0, None) == 0
