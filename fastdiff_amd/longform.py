"""Long-form and streaming synthesis on top of fd_sample_span (include/fastdiff_hip_ext.h).

One utterance of any length is vocoded window by window: each window is a batch item of the ordinary sampler, and the part of it kept
lies at least H = fd_sample_halo_frames(N) frames (16 per reverse step) from every window edge that is not an edge of the utterance.
The network's receptive field is finite, so the result is bit-identical to the whole-utterance call (FastDiff.sample with
stream_ids=[stream_id]) while the device memory stays that of one window batch.  FastDiff.sample_long is the whole-utterance form;
SampleStream the streaming one, for mel that arrives in chunks.  sample_long_batch and StreamPool do the same for many utterances
at once (fd_sample_spans): the windows of all of them share the sampler's batches, and every utterance still gets the bits of its own
single-utterance call.

Streaming latency: a frame is final once H frames of mel beyond it have arrived -- 64 frames (0.74 s at 22.05 kHz) for N = 4.
"""
import ctypes as ct

import torch

from . import _capi

HOP = 256


def halo_frames(N):
    """Frames of halo per side for an N-step schedule (fd_sample_halo_frames); raises for N outside 1..1024."""
    h = _capi.load().fd_sample_halo_frames(int(N))
    if h < 0:
        raise AssertionError(f"halo_frames: N={N} outside 1..1024")
    return h


def _steps(table):
    steps = getattr(table, "fd_steps", None)      # sampler.StepRows: the ctypes table built once per schedule
    if steps is None or len(steps) != len(table):
        steps = _capi.step_table(table)
    return steps


def sample_span(model, mel, mel_first, utt_frames, t0, t1, table, ddim=False, x_T=None, noise=None, seed=0, stream_id=0,
                window_frames=None):
    """x_0 [1,1,(t1-t0)*256] on frames [t0, t1) of one utterance, from mel [1,80,F] = its frames [mel_first, mel_first + F) (fd_sample_span).
    utt_frames: the utterance's length, or -1 while it is not known (streaming).  x_T [1,1,F*256] / noise [N,1,1,F*256] (execution
    order, N <= 8) cover the same frames as mel; None = Philox (seed, stream_id) at the utterance's absolute sample positions."""
    model._require_inference(mel, mel)
    mel = mel.to(dtype=torch.float32).reshape(1, mel.shape[-2], mel.shape[-1]).contiguous()
    assert mel.shape[1] == model.cond_channels
    F = mel.shape[-1]
    N = len(table)
    dev = mel.device
    if x_T is not None:
        x_T = x_T.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(x_T.shape) == (1, 1, F * HOP)
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(noise.shape) == (N, 1, 1, F * HOP)
    out = torch.empty((1, 1, max(0, int(t1) - int(t0)) * HOP), device=dev, dtype=torch.float32)
    lib, h = model._ready(dev)
    rc = lib.fd_sample_span(h, mel.data_ptr(), int(mel_first), F, int(utt_frames), int(t0), int(t1), _steps(table), N, int(bool(ddim)),
                            None if x_T is None else x_T.data_ptr(), None if noise is None else noise.data_ptr(),
                            ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ct.c_uint64(int(stream_id) & 0xFFFFFFFFFFFFFFFF),
                            int(window_frames or 0), out.data_ptr(), model._stream(dev))
    _capi.check(lib, h, rc, "fd_sample_span")
    return out


class SampleStream:
    """Streaming vocoder of one utterance (FastDiff.stream).  push(mel_chunk) takes [80, t] or [1, 80, t] and returns the samples that
    became final, a [n*256] float32 device tensor (possibly empty); close() returns the rest.  The concatenation of all returned pieces
    equals FastDiff.sample_long on the whole mel, bit for bit.

    Latency: after a push that brings the mel to F frames, every frame below F - H - chunk_frames + 1 has been returned (H =
    halo_frames(N): 64 frames = 0.74 s at N = 4); the stream computes in steps of chunk_frames (a multiple of 32) and keeps only the mel
    frames it still needs (the last H + chunk_frames or so)."""

    def __init__(self, model, table, ddim=False, seed=0, stream_id=0, chunk_frames=32):
        if chunk_frames <= 0 or chunk_frames % 32:
            raise AssertionError(f"SampleStream: chunk_frames={chunk_frames} must be a positive multiple of 32")
        self.model, self.table, self.ddim, self.seed, self.stream_id = model, table, ddim, seed, stream_id
        self.chunk = int(chunk_frames)
        self.H = halo_frames(len(table))
        self.mel = None            # [1, 80, kept] device: utterance frames [self.first, self.frames)
        self.first = 0
        self.frames = 0            # F: mel frames pushed so far
        self.done = 0              # frames returned so far (a multiple of 32 until close())
        self.closed = False

    def _span(self, t1, utt_frames):
        y = sample_span(self.model, self.mel, self.first, utt_frames, self.done, t1, self.table, ddim=self.ddim, seed=self.seed,
                        stream_id=self.stream_id)
        self.done = t1
        keep_from = max(0, t1 - self.H)          # the next span needs mel from max(0, t0 - H) on
        if keep_from > self.first:
            self.mel = self.mel[:, :, keep_from - self.first:].contiguous()
            self.first = keep_from
        return y.reshape(-1)

    def push(self, mel_chunk):
        if self.closed:
            raise AssertionError("SampleStream.push after close()")
        c = mel_chunk.reshape(-1, mel_chunk.shape[-2], mel_chunk.shape[-1]) if mel_chunk.dim() == 3 else mel_chunk.unsqueeze(0)
        assert c.shape[0] == 1 and c.shape[1] == self.model.cond_channels, f"SampleStream.push: expected [80, t] mel, got {list(mel_chunk.shape)}"
        c = c.to(dtype=torch.float32)
        self.mel = c.contiguous() if self.mel is None else torch.cat((self.mel, c.to(self.mel.device)), dim=-1)
        self.frames += c.shape[-1]
        ready = self.frames - self.H - self.done       # frames past `done` with a full halo of mel behind them
        if ready < self.chunk:
            return torch.empty(0, device=self.mel.device, dtype=torch.float32)
        return self._span(self.done + ready // self.chunk * self.chunk, -1)

    def close(self):
        """The rest of the utterance (its length is now known: the last window ends at the utterance's end)."""
        self.closed = True
        if self.mel is None or self.done >= self.frames:
            dev = self.mel.device if self.mel is not None else "cuda"
            return torch.empty(0, device=dev, dtype=torch.float32)
        return self._span(self.frames, self.frames)


def _u64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF


def plan_spans(spans, N, window_frames=None):
    """fd_sample_spans_plan on an array of _capi.FdSpan: ([FdSpanWindow], Wp) -- the windows fd_sample_spans would run, batch by batch."""
    lib = _capi.load()
    n = len(spans)
    wp = ct.c_int(0)
    count = lib.fd_sample_spans_plan(spans, n, int(N), int(window_frames or 0), None, 0, ct.byref(wp))
    if count < 0:
        raise AssertionError(f"fd_sample_spans_plan refused the spans (status {count})")
    wins = (_capi.FdSpanWindow * max(1, count))()
    lib.fd_sample_spans_plan(spans, n, int(N), int(window_frames or 0), wins, count, ct.byref(wp))
    return [wins[i] for i in range(count)], wp.value


def sample_spans(model, spans, table, ddim=False, seed=0, window_frames=None):
    """One fd_sample_spans call.  spans: dicts with mel (a device float32 tensor whose last two dimensions are [80, columns]), out (a
    device float32 tensor of (t1 - t0) * 256 elements, written in place), mel_first, mel_frames, utt_frames, t0, t1, stream_id and
    mel_cap (0 / absent: a plain buffer; else the ring's columns)."""
    if not spans:
        return
    dev = spans[0]["mel"].device
    arr = (_capi.FdSpan * len(spans))()
    for i, s in enumerate(spans):
        mel, out = s["mel"], s["out"]
        model._require_inference(mel, out)
        assert mel.dtype == torch.float32 and out.dtype == torch.float32 and mel.stride(-1) == 1 and out.is_contiguous()
        assert mel.shape[-2] == model.cond_channels and mel.device == dev and out.device == dev
        assert out.numel() == (int(s["t1"]) - int(s["t0"])) * HOP, f"span {i}: out has {out.numel()} elements for frames [{s['t0']}, {s['t1']})"
        arr[i] = _capi.FdSpan(mel.data_ptr(), mel.stride(-2), int(s.get("mel_cap", 0)), int(s["mel_first"]), int(s["mel_frames"]),
                              int(s["utt_frames"]), int(s["t0"]), int(s["t1"]), _u64(s.get("stream_id", 0)), out.data_ptr())
    lib, h = model._ready(dev)
    rc = lib.fd_sample_spans(h, arr, len(spans), _steps(table), len(table), int(bool(ddim)), ct.c_uint64(_u64(seed)),
                             int(window_frames or 0), model._stream(dev))
    _capi.check(lib, h, rc, "fd_sample_spans")


def sample_long_batch(model, mels, table, ddim=False, seed=0, stream_ids=None, window_frames=None):
    """[x_0 [1,1,T_i*256]] of the utterances mels[i] ([80,T_i] or [1,80,T_i]) in ONE fd_sample_spans call, one span per utterance:
    element i equals sample_long(mels[i], ..., stream_id=stream_ids[i]) bit for bit.  stream_ids default to range(len(mels))."""
    ids = list(range(len(mels))) if stream_ids is None else [int(v) for v in stream_ids]
    assert len(ids) == len(mels), f"sample_long_batch: {len(ids)} stream ids for {len(mels)} utterances"
    spans, outs = [], []
    for m, sid in zip(mels, ids):
        assert m.dim() in (2, 3) and m.shape[-2] == model.cond_channels and (m.dim() == 2 or m.shape[0] == 1), \
            f"sample_long_batch: expected [80, T] or [1, 80, T] mel, got {list(m.shape)}"
        model._require_inference(m)
        m = m.to(dtype=torch.float32).reshape(m.shape[-2], m.shape[-1]).contiguous()
        T = m.shape[-1]
        out = torch.empty((1, 1, T * HOP), device=m.device, dtype=torch.float32)
        spans.append({"mel": m, "out": out, "mel_first": 0, "mel_frames": T, "utt_frames": T, "t0": 0, "t1": T, "stream_id": sid})
        outs.append(out)
    sample_spans(model, spans, table, ddim=ddim, seed=seed, window_frames=window_frames)
    return outs


class StreamPool:
    """Many live streams vocoded together (FastDiff.stream_pool).  s = open(stream_id) takes a slot of a device arena
    [max_streams, 80, cap] of mel rings; feed(s, mel_chunk) appends [80, t] or [1, 80, t] frames to its ring (fd_mel_ring_append; the
    feeds between two steps go out in one launch); close(s) marks the utterance's end; step() makes ONE fd_sample_spans call over
    every open stream with at least chunk_frames ready frames (SampleStream's rule: a frame is ready once H = halo_frames(N) frames
    of mel lie beyond it) and over every closed stream's rest, and returns {s: float32 device tensor of the samples that became
    final}.  A stream with nothing ready is absent from the result; a closed stream's slot is free after the step that returned its
    rest.  The concatenation of a stream's pieces equals SampleStream with the same (seed, stream_id, chunk_frames) on the same
    chunks, hence sample_long, bit for bit.

    cap = ceil32(2 H + chunk_frames + max_feed_frames): after a step() a stream still needs fewer than 2 H + chunk_frames frames, so
    up to max_feed_frames may be fed to it before the next step(); feed() raises when a stream would hold more."""

    def __init__(self, model, table, ddim=False, seed=0, chunk_frames=32, max_streams=64, max_feed_frames=256):
        if chunk_frames <= 0 or chunk_frames % 32:
            raise AssertionError(f"StreamPool: chunk_frames={chunk_frames} must be a positive multiple of 32")
        if max_streams < 1 or max_feed_frames < 1:
            raise AssertionError(f"StreamPool: max_streams={max_streams} and max_feed_frames={max_feed_frames} must be positive")
        self.model, self.table, self.ddim, self.seed = model, table, ddim, seed
        self.chunk = int(chunk_frames)
        self.H = halo_frames(len(table))
        self.cap = (2 * self.H + self.chunk + int(max_feed_frames) + 31) // 32 * 32
        model._require_device(*model.parameters())
        self.device = next(model.parameters()).device
        self.arena = torch.zeros((int(max_streams), model.cond_channels, self.cap), device=self.device, dtype=torch.float32)
        self._free = list(range(int(max_streams) - 1, -1, -1))      # slot 0 first
        self._streams = {}        # handle -> state
        self._next = 0
        self._feeds = []          # (ring row tensor, first_frame, chunk): appended by the next _flush

    class _State:
        __slots__ = ("slot", "stream_id", "frames", "done", "closed")

    def open(self, stream_id):
        if not self._free:
            raise RuntimeError(f"StreamPool.open: all {self.arena.shape[0]} slots are in use (max_streams)")
        st = self._State()
        st.slot, st.stream_id, st.frames, st.done, st.closed = self._free.pop(), int(stream_id), 0, 0, False
        s, self._next = self._next, self._next + 1
        self._streams[s] = st
        return s

    def _first(self, st):
        return max(0, st.done - self.H)       # the oldest frame the stream still needs

    def feed(self, s, mel_chunk):
        st = self._streams[s]
        if st.closed:
            raise AssertionError("StreamPool.feed after close()")
        c = mel_chunk.reshape(-1, mel_chunk.shape[-2], mel_chunk.shape[-1]) if mel_chunk.dim() == 3 else mel_chunk.unsqueeze(0)
        assert c.shape[0] == 1 and c.shape[1] == self.model.cond_channels, f"StreamPool.feed: expected [80, t] mel, got {list(mel_chunk.shape)}"
        t = c.shape[-1]
        if t == 0:
            return
        held = st.frames + t - self._first(st)
        if held > self.cap:
            raise AssertionError(f"StreamPool.feed: the stream would hold {held} frames, its ring holds cap = {self.cap} "
                                 f"(2 * {self.H} halo + chunk_frames + max_feed_frames, rounded up to 32): call step() first")
        self._feeds.append((st.slot, st.frames, c[0].to(device=self.device, dtype=torch.float32).contiguous()))
        st.frames += t

    def close(self, s):
        self._streams[s].closed = True

    def _flush(self):
        if not self._feeds:
            return
        lib = self.model._ensure_handle(self.device)
        h = self.model._handle
        chunks = (_capi.FdRingChunk * len(self._feeds))()
        for i, (slot, first, c) in enumerate(self._feeds):
            chunks[i] = _capi.FdRingChunk(self.arena[slot].data_ptr(), self.cap, self.cap, first, c.data_ptr(), c.stride(0), c.shape[-1])
        rc = lib.fd_mel_ring_append(h, chunks, len(self._feeds), self.model._stream(self.device))
        self._feeds = []      # (the copies are enqueued on the current stream: the allocator keeps the chunks until they have run)
        _capi.check(lib, h, rc, "fd_mel_ring_append")

    def step(self):
        self._flush()
        spans, result, freed = [], {}, []
        for s, st in self._streams.items():
            if st.closed:
                freed.append(s)
                if st.done >= st.frames:
                    continue
                t1, utt = st.frames, st.frames
            else:
                ready = st.frames - self.H - st.done
                if ready < self.chunk:
                    continue
                t1, utt = st.done + ready // self.chunk * self.chunk, -1
            first = self._first(st)
            out = torch.empty(((t1 - st.done) * HOP,), device=self.device, dtype=torch.float32)
            spans.append({"mel": self.arena[st.slot], "mel_cap": self.cap, "out": out, "mel_first": first, "mel_frames": st.frames - first,
                          "utt_frames": utt, "t0": st.done, "t1": t1, "stream_id": st.stream_id})
            result[s] = (out, st, t1)
        sample_spans(self.model, spans, self.table, ddim=self.ddim, seed=self.seed)      # (a refusal leaves the pool as it was)
        for s in freed:
            self._free.append(self._streams.pop(s).slot)
        for s, (out, st, t1) in list(result.items()):
            st.done = t1
            result[s] = out
        return result
