"""Long-form and streaming synthesis on top of fd_sample_span (include/fastdiff_hip_ext.h).

One utterance of any length is vocoded window by window: each window is a batch item of the ordinary sampler, and the part of it kept
lies at least H = fd_sample_halo_frames(N) frames (16 per reverse step) from every window edge that is not an edge of the utterance.
The network's receptive field is finite, so the result is bit-identical to the whole-utterance call (FastDiff.sample with
stream_ids=[stream_id]) while the device memory stays that of one window batch.  FastDiff.sample_long is the whole-utterance form;
SampleStream the streaming one, for mel that arrives in chunks.

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
