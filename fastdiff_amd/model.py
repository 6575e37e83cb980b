"""Host-side mirror of the reference denoiser module, backed by libfastdiff_hip.so.

`FastDiff` keeps the reference's constructor signature, parameter names / shapes / registration order
(so `state_dict()`, `load_state_dict(ckpt['state_dict']['model'])`, `.cuda()`, `.eval()` behave as for
modules/FastDiff/module/FastDiff_model.py:10-122) and the `forward(data)` contract
(FastDiff_model.py:74-102).  On the inference path the torch.nn sub-modules below are parameter holders only: no
PyTorch op runs there -- forward() hands raw device pointers to the C ABI (include/fastdiff_hip.h).  Under autograd
(train() mode, or an input that requires a gradient) forward() records the same network as autograd nodes with the
location-variable convolutions on the HIP operator, forward and backward (fastdiff_amd/train.py).
There is no CPU fallback: without the HIP library or a HIP device it raises.
"""
import ctypes as ct

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _wave


class _DBlockParams(nn.Module):
    """Parameters of DiffusionDBlock (modules.py:116-125)."""

    def __init__(self, input_size, hidden_size, factor):
        super().__init__()
        self.factor = factor
        self.residual_dense = nn.Conv1d(input_size, hidden_size, 1)
        self.conv = nn.ModuleList([
            nn.Conv1d(input_size, hidden_size, 3, dilation=1, padding=1),
            nn.Conv1d(hidden_size, hidden_size, 3, dilation=2, padding=2),
            nn.Conv1d(hidden_size, hidden_size, 3, dilation=4, padding=4),
        ])


class _KernelPredictorParams(nn.Module):
    """Parameters of KernelPredictor (modules.py:257-318)."""

    def __init__(self, cond_channels, conv_in_channels, conv_out_channels, conv_layers, conv_kernel_size,
                 hidden, kp_conv_size, dropout):
        super().__init__()
        l_w = conv_in_channels * conv_out_channels * conv_kernel_size * conv_layers
        l_b = conv_out_channels * conv_layers
        pad = (kp_conv_size - 1) // 2
        act = lambda: nn.LeakyReLU(negative_slope=0.1)  # noqa: E731
        self.input_conv = nn.Sequential(nn.Conv1d(cond_channels, hidden, 5, padding=2, bias=True), act())
        layers = []
        for _ in range(3):
            layers += [nn.Dropout(dropout),
                       nn.Conv1d(hidden, hidden, kp_conv_size, padding=pad, bias=True), act(),
                       nn.Conv1d(hidden, hidden, kp_conv_size, padding=pad, bias=True), act()]
        self.residual_conv = nn.Sequential(*layers)
        self.kernel_conv = nn.Conv1d(hidden, l_w, kp_conv_size, padding=pad, bias=True)
        self.bias_conv = nn.Conv1d(hidden, l_b, kp_conv_size, padding=pad, bias=True)


class _LVCBlockParams(nn.Module):
    """Parameters of TimeAware_LVCBlock (modules.py:141-187), registered and constructed in the reference's order."""

    def __init__(self, in_channels, cond_channels, upsample_ratio, conv_layers, conv_kernel_size, cond_hop_length,
                 kpnet_hidden_channels, kpnet_conv_size, kpnet_dropout, noise_scale_embed_dim_out):
        super().__init__()
        self.cond_hop_length = cond_hop_length
        self.convs = nn.ModuleList()
        r = upsample_ratio
        self.upsample = nn.ConvTranspose1d(in_channels, in_channels, kernel_size=2 * r, stride=r,
                                           padding=r // 2 + r % 2, output_padding=r % 2)
        self.kernel_predictor = _KernelPredictorParams(cond_channels, in_channels, 2 * in_channels, conv_layers,
                                                       conv_kernel_size, kpnet_hidden_channels, kpnet_conv_size,
                                                       kpnet_dropout)
        self.fc_t = nn.Linear(noise_scale_embed_dim_out, cond_channels)
        for i in range(conv_layers):
            pad = (3 ** i) * int((conv_kernel_size - 1) / 2)
            self.convs.append(nn.Conv1d(in_channels, in_channels, kernel_size=conv_kernel_size, padding=pad,
                                        dilation=3 ** i))


class FastDiff(nn.Module):
    """Drop-in for `modules.FastDiff.module.FastDiff_model.FastDiff` on an MI355X."""

    def __init__(self, audio_channels=1, inner_channels=32, cond_channels=80, upsample_ratios=[8, 8, 4],
                 lvc_layers_each_block=4, lvc_kernel_size=3, kpnet_hidden_channels=64, kpnet_conv_size=3,
                 dropout=0.0, diffusion_step_embed_dim_in=128, diffusion_step_embed_dim_mid=512,
                 diffusion_step_embed_dim_out=512, use_weight_norm=True):
        super().__init__()
        if dropout != 0.0:
            raise NotImplementedError("fastdiff_amd is the inference path: dropout must be 0.0 (base.yaml:29)")
        self.diffusion_step_embed_dim_in = diffusion_step_embed_dim_in
        self.audio_channels = audio_channels
        self.cond_channels = cond_channels
        self.lvc_block_nums = len(upsample_ratios)
        self._cfg = dict(audio_channels=audio_channels, inner_channels=inner_channels, cond_channels=cond_channels,
                         upsample_ratios=list(upsample_ratios), lvc_layers_each_block=lvc_layers_each_block,
                         lvc_kernel_size=lvc_kernel_size, kpnet_hidden_channels=kpnet_hidden_channels,
                         kpnet_conv_size=kpnet_conv_size, diffusion_step_embed_dim_in=diffusion_step_embed_dim_in,
                         diffusion_step_embed_dim_mid=diffusion_step_embed_dim_mid,
                         diffusion_step_embed_dim_out=diffusion_step_embed_dim_out, use_weight_norm=use_weight_norm)
        self.hop_length = int(np.prod(upsample_ratios))

        self.first_audio_conv = nn.Conv1d(1, inner_channels, kernel_size=7, padding=3, dilation=1, bias=True)
        self.lvc_blocks = nn.ModuleList()
        self.downsample = nn.ModuleList()
        self.fc_t = nn.ModuleList()
        self.fc_t1 = nn.Linear(diffusion_step_embed_dim_in, diffusion_step_embed_dim_mid)
        self.fc_t2 = nn.Linear(diffusion_step_embed_dim_mid, diffusion_step_embed_dim_out)
        hop = 1
        for n in range(self.lvc_block_nums):
            hop *= upsample_ratios[n]
            self.lvc_blocks.append(_LVCBlockParams(inner_channels, cond_channels, upsample_ratios[n],
                                                   lvc_layers_each_block, lvc_kernel_size, hop, kpnet_hidden_channels,
                                                   kpnet_conv_size, dropout, diffusion_step_embed_dim_out))
            self.downsample.append(_DBlockParams(inner_channels, inner_channels,
                                                 upsample_ratios[self.lvc_block_nums - n - 1]))
        self.final_conv = nn.Sequential(nn.Conv1d(inner_channels, audio_channels, kernel_size=7, padding=3,
                                                  dilation=1, bias=True))
        if use_weight_norm:
            self.apply_weight_norm()
        # HIP side
        self._handle = None
        self._handle_device = None
        self._synced_state = None
        self._keepalive = None
        self.last_ticket = 0
        # Library options of this module's handle.  "fallback": "host" -- the range check of a sample() call is read on the host
        # instead of trailing every fp16x2 kernel with an early-exit fp32 launch (21 launches per reverse step less: -3 % at B=8,
        # -7 % at B=1).  "defer_check": "1" -- the library does not settle that check inside fd_sample (its default for a C caller,
        # include/fastdiff_hip.h): sample() / check() / settle() below do it, which lets sample(..., defer_check=True) pipeline calls.
        self._options = {"fallback": "host", "defer_check": "1"}
        self._param_list = None                # the parameter tensors _state_signature last walked (see there)
        self._sig_calls = 0
        # Set by whoever writes the parameters behind torch's back (TrainStep.step: its optimizer kernel takes raw pointers, so neither
        # data_ptr nor _version moves): the next inference call then refreshes the handle's weights first (refresh_weights).
        self._weights_dirty = False
        self.last_refresh = None               # how the weights last reached the handle: "device", or "host: <why>"
        # Where the inference handle's weights come from (use_weights): None = the live parameters, else a mapping name -> tensor
        self._weights_source = None
        self._weights_label = None

    # ---- reference API --------------------------------------------------------------------------------
    def apply_weight_norm(self):
        def _apply(m):
            if isinstance(m, (nn.Conv1d, nn.Conv2d)):
                torch.nn.utils.weight_norm(m)
        self.apply(_apply)
        self.__dict__["_param_list"] = None

    def remove_weight_norm(self):
        def _remove(m):
            try:
                torch.nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        self.apply(_remove)
        self._invalidate_params()

    def forward(self, data, lens=None):
        """eps = net((audio [B,1,L], c [B,80,T] or [80,T], diffusion_steps [B,1])) -- FastDiff_model.py:74-102.
        lens (extension, optional): valid frames per utterance of a zero-padded batch, see sample()."""
        audio, c, diffusion_steps = data
        if torch.is_grad_enabled() and (self.training or audio.requires_grad or c.requires_grad):
            # training (FastDiff.py:44-49): the same network as autograd nodes, the location-variable convolutions forward and
            # backward on the HIP operator (fastdiff_amd/train.py)
            if lens is not None:
                raise NotImplementedError("lens is an extension of the inference path; under autograd pass whole utterances")
            self._require_device(audio, c)
            if not getattr(self, "_warned_autograd_path", False) and not (audio.requires_grad or c.requires_grad):
                # nn.Module starts in train() mode: a freshly built model called outside no_grad lands here, not on the fused kernels
                import warnings
                warnings.warn("fastdiff_amd.FastDiff.forward is recording an autograd graph (module in train() mode with gradients "
                              "enabled): the fused inference kernels run under torch.no_grad() or after .eval()", stacklevel=2)
                self._warned_autograd_path = True
            from .train import differentiable_forward
            return differentiable_forward(self, (audio.float(), self._prep_condition(c, audio.shape[0], audio.device), diffusion_steps))
        self._require_inference(audio, c)
        audio = audio.contiguous().float()
        B, ch, L = audio.shape
        c = self._prep_condition(c, B, audio.device)
        T = c.shape[-1]
        # the reference's check is `in_length == kernel_length * hop_size` (modules.py:236)
        assert ch == 1 and L == T * self.hop_length, "length of (x, kernel) is not matched"
        steps = diffusion_steps.to(device=audio.device, dtype=torch.float32).reshape(-1).contiguous()
        assert steps.numel() == B
        out = torch.empty_like(audio)
        lib, h = self._ready(audio.device)
        lens_arr = None if lens is None else (ct.c_int * B)(*[int(v) for v in lens])
        rc = lib.fd_forward(h, audio.data_ptr(), c.data_ptr(), steps.data_ptr(), B, T, lens_arr, out.data_ptr(),
                            self._stream(audio.device))
        _capi.check(lib, h, rc, "fd_forward")
        return out

    # ---- HIP-side entry used by fastdiff_amd.util.sampling_given_noise_schedule ---------------------------
    def sample(self, condition, table, ddim=False, x_T=None, noise=None, seed=0, return_sequence=False, lens=None, stream_ids=None,
               defer_check=False):
        """Run the N-step reverse loop on the device.

        table: list of dicts with keys t, c_eps, c_div, sigma, c1, c2, c3, add_noise (executed first -> last).
        x_T [B,1,L] / noise [N,B,1,L] optional device tensors (None -> on-device Philox keyed by `seed`).
        lens: optional valid frames per utterance of a zero-padded batch: utterance b is then computed as if it were alone
        and lens[b] frames long (its first lens[b]*256 samples are exactly that result; the rest of its row is unspecified).
        stream_ids: optional [B] integers (fd_set_noise_streams): utterance b draws its noise from Philox stream (seed, stream_ids[b])
        over its own samples, i.e. independently of its place in the batch.
        defer_check: this class runs the library with option fallback = "host" (self._options; also the C ABI's default): a
        result is final only after its range check has been looked at (fd_sample_check: one stream synchronisation and, rarely, a
        second pass on the fp32 kernels).  sample() does that before returning unless told to defer.  A deferred call is settled ONLY by
        check(), settle(ticket), forward(), the next sample() (which looks at it after enqueuing itself), set_option and a weight
        upload -- NOT by peak_normalize_int16 / mel_spectrogram, which run on a provisional waveform without waiting: read their output
        only after check() / settle(last_ticket) returned False, and compute it again when they returned True."""
        B = condition.shape[0]
        self._require_inference(condition, condition)
        condition = condition.contiguous().float()
        T = condition.shape[-1]
        L = T * self.hop_length
        N = len(table)
        steps = getattr(table, "fd_steps", None)      # sampler.StepRows: the ctypes table built once per schedule
        if steps is None or len(steps) != N:
            steps = _capi.step_table(table)
        dev = condition.device
        out = torch.empty((B, 1, L), device=dev, dtype=torch.float32)
        seq = torch.empty((N + 1, B, 1, L), device=dev, dtype=torch.float32) if return_sequence else None
        if x_T is not None:
            x_T = x_T.to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(x_T.shape) == (B, 1, L)
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(noise.shape) == (N, B, 1, L)
        lib, h = self._ready(dev)
        lens_arr = None if lens is None else (ct.c_int * B)(*[int(v) for v in lens])
        if stream_ids is not None:
            assert len(stream_ids) == B
            ids = (ct.c_uint64 * B)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids])
            _capi.check(lib, h, lib.fd_set_noise_streams(h, ids, B), "fd_set_noise_streams")
        rc = lib.fd_sample(h, condition.data_ptr(), B, T, lens_arr, steps, N, int(bool(ddim)),
                           None if x_T is None else x_T.data_ptr(), None if noise is None else noise.data_ptr(),
                           ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), out.data_ptr(),
                           None if seq is None else seq.data_ptr(), self._stream(dev))
        _capi.check(lib, h, rc, "fd_sample")
        # inputs (and outputs) of the calls a deferred check may still run again: this one and, under the pipelined host check,
        # the one before it (looked at only after this call was enqueued)
        self._keepalive = ((condition, x_T, noise, out, seq), self._keepalive[0] if self._keepalive else None)
        self.last_ticket = int(lib.fd_sample_ticket(h))
        if not defer_check:
            self.check()
        if return_sequence:
            return [seq[k] for k in range(N + 1)]
        return out

    def sample_long(self, condition, table, ddim=False, x_T=None, noise=None, seed=0, stream_id=0, window_frames=None):
        """x_0 [1,1,T*256] of ONE utterance of any length T, window by window (fd_sample_span; fastdiff_amd/longform.py): bit-identical
        to sample(condition, table, ddim, seed=seed, stream_ids=[stream_id]) -- also past the length sample() refuses -- while the
        device memory stays that of one window batch.  condition [1,80,T] or [80,T]; x_T [1,1,T*256] / noise [N,1,1,T*256] (N <= 8)
        as in sample(); window_frames: centre frames per window (a multiple of 32), None = the library's default."""
        from . import longform
        c = condition if condition.dim() == 3 else condition.unsqueeze(0)
        assert c.shape[0] == 1, "sample_long vocodes one utterance: condition [1,80,T]"
        T = c.shape[-1]
        return longform.sample_span(self, c, 0, T, 0, T, table, ddim=ddim, x_T=x_T, noise=noise, seed=seed, stream_id=stream_id,
                                    window_frames=window_frames)

    def stream(self, table, ddim=False, seed=0, stream_id=0, chunk_frames=32):
        """A SampleStream (fastdiff_amd/longform.py) of one utterance whose mel arrives in chunks: push([80,t]) returns the samples
        that became final, close() the rest; together they equal sample_long on the whole mel.  Lookahead: H = halo_frames(N)
        frames of mel beyond a frame before it is final (64 frames = 0.74 s at N = 4)."""
        from . import longform
        return longform.SampleStream(self, table, ddim=ddim, seed=seed, stream_id=stream_id, chunk_frames=chunk_frames)

    def sample_long_batch(self, mels, table, ddim=False, seed=0, stream_ids=None, window_frames=None):
        """A list of x_0 [1,1,T_i*256], one per utterance of `mels` (a list of [80,T_i] or [1,80,T_i] tensors of any lengths), from ONE
        fd_sample_spans call: the windows of all utterances share the sampler's batches.  Element i equals
        sample_long(mels[i], table, ddim, seed=seed, stream_id=stream_ids[i], window_frames=window_frames) bit for bit; stream_ids
        default to range(len(mels)).  Distinct utterances need distinct stream ids."""
        from . import longform
        return longform.sample_long_batch(self, mels, table, ddim=ddim, seed=seed, stream_ids=stream_ids, window_frames=window_frames)

    def stream_pool(self, table, ddim=False, seed=0, chunk_frames=32, max_streams=64, max_feed_frames=256):
        """A StreamPool (fastdiff_amd/longform.py): up to max_streams live streams whose mel lies in device rings; open / feed / close
        per stream, and one step() vocodes whatever became ready on all of them in one fd_sample_spans call.  A stream's pieces
        equal stream(table, ddim, seed, stream_id, chunk_frames) on the same chunks, hence sample_long, bit for bit."""
        from . import longform
        return longform.StreamPool(self, table, ddim=ddim, seed=seed, chunk_frames=chunk_frames, max_streams=max_streams,
                                   max_feed_frames=max_feed_frames)

    @staticmethod
    def halo_frames(N):
        """Frames of halo per side that sample_long / stream add for an N-step schedule (fd_sample_halo_frames)."""
        from . import longform
        return longform.halo_frames(N)

    def check(self):
        """Settle the last sample() under fallback = "host" (no-op otherwise).  Returns True if it had to be redone."""
        if self._handle is None:
            return False
        lib = _capi.load()
        rc = lib.fd_sample_check(self._handle)
        _capi.check(lib, self._handle, rc, "fd_sample_check")
        self._keepalive = None
        return rc == 1

    def settle(self, ticket):
        """Pipelined host check (option fallback = "host", sample(..., defer_check=True)): make the sample() call whose `last_ticket`
        was `ticket` final -- waiting for it only if nothing has looked at it yet; the next sample() on the module does so after
        enqueuing itself -- and return True if it had to be run again on the fp32 kernels: whatever the caller computed from its
        output in the meantime (epilogue, copies) must then be computed again.  With in-graph fallbacks (option fallback = "graph"): False."""
        if self._handle is None:
            return False
        lib = _capi.load()
        rc = lib.fd_sample_settle(self._handle, int(ticket))
        _capi.check(lib, self._handle, rc, "fd_sample_settle")
        return rc == 1

    def peak_normalize_int16(self, wav, valid=None):
        """wav [B,1,L] float32 -> int16 PCM [B,L]: wav/abs(wav).max() * 32767 (FastDiff.py:110; utils/audio.py:11-16).
        valid (optional, [B] sample counts of a zero-padded batch): each utterance's peak is searched over its own samples only
        and the PCM behind them is 0 -- one call and one device-to-host copy per micro-batch instead of one per utterance."""
        lib, h, stream = self._wave_call(wav)
        wav, B, L = _wave.rows(wav, "peak_normalize_int16")
        pcm = torch.empty((B, L), device=wav.device, dtype=torch.int16)
        rc = lib.fd_peak_normalize_int16_ragged(h, wav.data_ptr(), B, L, _wave.counts(valid, B, "peak_normalize_int16"), pcm.data_ptr(), stream)
        _capi.check(lib, h, rc, "fd_peak_normalize_int16")
        return pcm

    def mel_spectrogram(self, wav, n_frames=None, variant="pwg"):
        """wav [B, n] float32 in [-1, 1] (int16 PCM / 32768) -> log-mel [B, 80, T], T = 1 + n // 256 by default, on the device.
        variant "pwg": the reference's process_utterance(..., vocoder='pwg') (data_gen/tts/data_gen_utils.py:93-147): zero padding,
        filters 80-7600 Hz, log10(max(1e-6, .)).  variant "tacotron": TacotronSTFT.mel_spectrogram (data_gen/tts/tacotron/layers.py:
        42-80): reflect padding, filters 0-8000 Hz, ln(clamp(., 1e-5)); asserts the range [-1, 1] like the reference (layers.py:70-71)."""
        if variant not in ("pwg", "tacotron"):
            raise ValueError(f"mel_spectrogram: variant must be 'pwg' or 'tacotron', got {variant!r}")
        self._require_inference(wav, wav)
        wav = wav.contiguous().float()
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        B, n = wav.shape
        if variant == "tacotron":
            assert torch.min(wav) >= -1
            assert torch.max(wav) <= 1
        T = 1 + n // self.hop_length if n_frames is None else int(n_frames)
        mel = torch.empty((B, 80, T), device=wav.device, dtype=torch.float32)
        lib, h = self._ready(wav.device)
        _capi.check(lib, h, lib.fd_set_option(h, b"mel", variant.encode()), "fd_set_option")
        _capi.check(lib, h, lib.fd_mel_spectrogram(h, wav.data_ptr(), B, n, mel.data_ptr(), T, self._stream(wav.device)), "fd_mel_spectrogram")
        return mel

    def resample(self, x, sr_in, sr_out, valid=None, channels=1):
        """Sample-rate conversion on the device (fastdiff_amd/resample.py; the reference's librosa.core.load(path, sr=...),
        data_gen/tts/data_gen_utils.py:111): x [n] / [B, n], or interleaved [n, C] / [B, n, C] with channels = C, float32 / int16 /
        int32 / uint8 as a RIFF file holds them -> float32 mono [B, out_len(n, sr_in, sr_out)].  valid: [B] frame counts of a
        zero-padded batch; each item's result is what it gets alone, and 0 behind its own length."""
        from . import resample as _resample
        return _resample._run(*self._wave_call(x), x, sr_in, sr_out, valid, channels)

    def loudness(self, wav, valid=None, sample_rate=22050):
        """BS.1770 integrated loudness on the device (fastdiff_amd/loudness.py; the reference's pyloudnorm.Meter(rate), data_gen/tts/
        data_gen_utils.py:115-117): wav [n] / [B, n] / [B, 1, n] float32 -> a dict of numpy arrays over the batch: lufs, gain (1 here),
        peak, blocks, gated, status (loudness.OK / SHORT / SILENT / CLIPPED).  valid: [B] sample counts of a padded batch.  Synchronises
        once, for the records."""
        from . import loudness as _loudness
        return _loudness._measure(*self._wave_call(wav), wav, valid, sample_rate)

    def loudness_normalize(self, wav, target, valid=None, sample_rate=22050, out="float", return_record=False):
        """wav scaled to `target` LUFS on the device (pyloudnorm.normalize.loudness with the reference's guard, data_gen_utils.py:118-120):
        out="float": float32 in the shape of wav; out="int16": PCM [B, n] = (int16)(wav gain 32767).  An utterance that cannot be
        measured (SHORT, SILENT) or whose peak the gain would push over 1 (CLIPPED) is peak-normalised instead in int16 mode, bit for bit
        as peak_normalize_int16 does it; in float mode it is left unchanged (SHORT, SILENT) or divided by its peak (CLIPPED).
        return_record: (output, record as FastDiff.loudness returns it, with the gain applied); without it nothing synchronises."""
        from . import loudness as _loudness
        return _loudness._normalize(*self._wave_call(wav), wav, target, valid, sample_rate, out, return_record)

    def trim_silences(self, wav, valid=None, sample_rate=22050, window_ms=30, top_db=40., floor_db=-70., average_width=8, max_silence=12,
                      mode="long", return_flags=False, return_record=False):
        """Long silences cut on the device (fastdiff_amd/trim.py; the reference's trim_long_silences, data_gen/tts/data_gen_utils.py:27-90,
        with an energy detector in place of WebRTC's): wav [n] / [B, n] / [B, 1, n] -> (out [B, n] float32: each utterance's kept samples in
        order, 0 behind them; out_valid device int32 [B]), then the window flags and the record on request.  Nothing synchronises without
        return_record."""
        from . import trim as _trim
        return _trim._trim(*self._wave_call(wav), wav, valid, sample_rate, window_ms, top_db, floor_db, average_width, max_silence, mode,
                           return_flags, return_record)

    def trim_levels(self, wav, valid=None, sample_rate=22050, window_ms=30):
        """The level of every window of trim_silences, dB re full scale: device float64 [B, Mmax] (fastdiff_amd/trim.py: levels)."""
        from . import trim as _trim
        return _trim._levels(*self._wave_call(wav), wav, valid, sample_rate, window_ms)

    def stoi(self, clean, degraded, valid=None, sample_rate=22050):
        """STOI and ESTOI of `degraded` against `clean` on the device (fastdiff_amd/stoi.py; what people run pystoi for over the reference's
        *_gt.wav / *_pred.wav pairs, FastDiff.py:113-117): two tensors [n] / [B, n] / [B, 1, n] of one shape at `sample_rate` -> a dict of
        numpy arrays over the batch: stoi, estoi (NaN unless OK), frames, kept, segments, status (stoi.OK / SHORT / SILENT).  valid: [B]
        sample counts of a padded batch.  Synchronises once, for the records."""
        from . import stoi as _stoi
        return _stoi._measure(*self._wave_call(clean, degraded), clean, degraded, valid, sample_rate)

    def pitch(self, clean, degraded, valid=None, **cfg):
        """The pitch scores of `degraded` against `clean` on the device (fastdiff_amd/pitch.py): both are tracked with YIN on the mel
        frame grid (one F0 per hop, where the reference's data_gen_utils.get_pitch runs Praat / WORLD) and the tracks compared.  Two
        tensors [n] / [B, n] / [B, 1, n] of one shape -> a dict of numpy arrays over the batch: rmse_cents, gpe (NaN unless OK), vde,
        frames, both_voiced, ref_voiced, deg_voiced, status (pitch.OK / SHORT / UNVOICED).  valid: [B] sample counts of a padded batch;
        cfg: rate, hop, win, f0_min, f0_max, threshold.  Synchronises once, for the records."""
        from . import pitch as _pitch
        return _pitch._measure(*self._wave_call(clean, degraded), clean, degraded, valid, cfg)

    def spectral(self, clean, degraded, valid=None, **cfg):
        """The multi-resolution STFT distances of `degraded` against `clean` on the device (fastdiff_amd/spectral.py; what people compute
        with torch.stft over the reference's *_gt.wav / *_pred.wav pairs): two tensors [n] / [B, n] / [B, 1, n] of one shape -> a dict of
        numpy arrays over the batch: sc, logmag, lsd [B, 4] per resolution, their means mr_sc, mr_logmag, lsd_db (NaN unless OK), frames
        [B, 4], n_res, status (spectral.OK / SHORT).  valid: [B] sample counts of a padded batch; cfg: resolutions, floor.  Synchronises
        once, for the records."""
        from . import spectral as _spectral
        return _spectral._measure(*self._wave_call(clean, degraded), clean, degraded, valid, cfg)

    def mcd(self, clean, degraded, valid=None, valid_degraded=None, **cfg):
        """The mel-cepstral distortion of `degraded` against `clean` on the device, with and without time alignment (fastdiff_amd/mcd.py):
        two tensors [n] / [B, n] / [B, 1, n] whose lengths may differ -> a dict of numpy arrays over the batch: mcd_dtw, mcd_linear (dB,
        NaN unless OK), cost, path_len, n_diag, frames_clean, frames_degraded, status (mcd.OK / SHORT / NONFINITE).  valid,
        valid_degraded: [B] sample counts of the padded batches (valid_degraded=None: valid counts for both); cfg: n_coef, variant.
        Synchronises once, for the records."""
        from . import mcd as _mcd
        return _mcd._measure(*self._wave_call(clean, degraded), clean, degraded, valid, cfg, valid_degraded=valid_degraded)

    def mel_to_linear(self, mel, variant="pwg", inversion="pinv", nnls_iters=128, lens=None, return_record=False):
        """Mel inversion on the device (fastdiff_amd/griffin_lim.py; utils/audio.py:91-95 _mel_to_linear): mel [B, 80, T] as front-end
        `variant` produces it (log10 for "pwg", ln for "tacotron") -> amplitudes [B, 513, T], with the bank this module's front-end
        uses (mel_filterbank) and its pseudo-inverse from numpy.linalg.pinv in float64, cached per variant.  inversion="pinv" (the
        default): max(1e-10, pinv(bank) @ g(mel)).  inversion="nnls": the non-negative least squares of GLMel's
        librosa.feature.inverse.mel_to_stft (librosa.util.nnls) -- nnls_iters accelerated projected-gradient steps from the clipped
        pseudo-inverse in one fused kernel; lens: [B] frame counts of a padded batch; return_record: (amp, record with resid, norm,
        frames, iters, status per item), which synchronises once.  Otherwise nothing synchronises."""
        from . import griffin_lim as _gl
        _gl.variant_id(variant)
        if inversion not in ("pinv", "nnls"):
            raise ValueError(f"mel_to_linear: inversion must be 'pinv' or 'nnls', got {inversion!r}")
        lib, h, stream = self._wave_call(mel)
        bank = self.mel_filterbank(variant, device=mel.device)[0]
        P = _gl.pinv(bank, variant)
        if inversion == "nnls":
            return _gl._mel_to_linear_nnls(lib, h, stream, mel, bank, P, variant, lens, nnls_iters, return_record)
        if return_record:
            raise ValueError("mel_to_linear: only inversion='nnls' has a record")
        return _gl._mel_to_linear(lib, h, stream, mel, P, variant)

    def griffin_lim(self, amp, lens=None, n_iters=60, angles=None, seed=0, stream_ids=None, return_record=False):
        """Griffin-Lim on the device (fastdiff_amd/griffin_lim.py; the reference's GLLinear, vocoders/gl_linear.py over utils/audio.py:
        35-63): amplitudes [B, 513, T] of a 1024-point STFT at hop 256 -> wav [B, 256 (T - 1)] after n_iters projections.  lens: [B] frame
        counts of a padded batch (item b: 256 (lens[b] - 1) samples, zeros behind them).  angles [B, 513, T]: the starting phase
        (n_iters = 0: the inverse STFT alone); None: Philox angles keyed on (seed, stream_ids[b] or b, frame, bin), so with ids an item's
        waveform does not depend on its batch.  return_record: (wav, record) with sc = || |stft(wav)| - amp || / || amp ||, norm, frames,
        samples, iters, status (griffin_lim.OK / SHORT / SILENT / NONFINITE) per item; without it nothing synchronises."""
        from . import griffin_lim as _gl
        return _gl._run(*self._wave_call(amp), amp, lens, n_iters, angles, seed, stream_ids, return_record)

    def griffin_lim_mel(self, mel, lens=None, variant="pwg", inversion="pinv", nnls_iters=128, **kw):
        """mel_to_linear, then griffin_lim: mel [B, 80, T] -> wav [B, 256 (T - 1)] (the reference's GLMel).  inversion="pinv" (the
        default) inverts the mel with the pseudo-inverse, inversion="nnls" with GLMel's own non-negative least squares (nnls_iters
        steps).  kw: n_iters, seed, stream_ids, return_record (Griffin-Lim's record)."""
        if inversion == "pinv":
            return self.griffin_lim(self.mel_to_linear(mel, variant), lens=lens, **kw)
        return self.griffin_lim(self.mel_to_linear(mel, variant, inversion=inversion, nnls_iters=nnls_iters, lens=lens), lens=lens, **kw)

    def pitch_track(self, wav, valid=None, **cfg):
        """(f0, aper) of `wav` on the device, float32 [B, n // hop] (fastdiff_amd/pitch.py: track); does not synchronise."""
        from . import pitch as _pitch
        return _pitch._track(*self._wave_call(wav), wav, valid, cfg)

    def set_mel_filterbank(self, fb, variant="pwg", device=None):
        """Use `fb` [80, 513] (numpy / tensor, float32; librosa.filters.mel's own layout) as the filter bank of front-end `variant`
        instead of the library's restated default -- what a deployment that has librosa passes
        (`librosa.filters.mel(sr=22050, n_fft=1024, n_mels=80, fmin=80, fmax=7600)`; Tacotron: fmin 0, fmax 8000;
        data_gen/tts/data_gen_utils.py:122-134, tacotron/layers.py:42-60).  The weights are used bit for bit.  fb None: back to the default."""
        import numpy as np
        if variant not in ("pwg", "tacotron"):
            raise ValueError(f"set_mel_filterbank: variant must be 'pwg' or 'tacotron', got {variant!r}")
        dev = device if device is not None else next(self.parameters()).device
        lib, h = self._ready(torch.device(dev))
        _capi.check(lib, h, lib.fd_set_option(h, b"mel", variant.encode()), "fd_set_option")
        banks = self.__dict__.setdefault("_mel_banks", {})
        if fb is None:
            banks.pop(variant, None)
            _capi.check(lib, h, lib.fd_set_mel_filterbank(h, None, 80, 513), "fd_set_mel_filterbank")
            return
        a = np.ascontiguousarray(fb.detach().cpu().numpy() if torch.is_tensor(fb) else fb, dtype=np.float32)
        if a.shape != (80, 513):
            raise ValueError(f"set_mel_filterbank: expected [80, 513] (80 mel filters over the bins of a 1024-point FFT), got {list(a.shape)}")
        _capi.check(lib, h, lib.fd_set_mel_filterbank(h, a.ctypes.data, 80, 513), "fd_set_mel_filterbank")
        banks[variant] = a.copy()

    def mel_filterbank(self, variant="pwg", device=None):
        """(bank [80, 513] float32 numpy, supplied_by_caller) of front-end `variant` as the library uses it."""
        import numpy as np
        dev = device if device is not None else next(self.parameters()).device
        lib, h = self._ready(torch.device(dev))
        _capi.check(lib, h, lib.fd_set_option(h, b"mel", variant.encode()), "fd_set_option")
        out = np.empty((80, 513), np.float32)
        rc = lib.fd_get_mel_filterbank(h, out.ctypes.data, 80, 513)
        if rc < 0:
            _capi.check(lib, h, rc, "fd_get_mel_filterbank")
        return out, bool(rc)

    # ---- options / introspection (tests, bench) ---------------------------------------------------------
    def set_option(self, key, value):
        self._options[key] = str(value)
        if self._handle is not None:
            lib = _capi.load()
            _capi.check(lib, self._handle, lib.fd_set_option(self._handle, key.encode(), str(value).encode()), "fd_set_option")

    def read_tap(self, name):
        lib = _capi.load()
        n = lib.fd_read_tap(self._handle, name.encode(), None, 0)
        _capi.check(lib, self._handle, n, "fd_read_tap")
        buf = np.empty(n, np.float32)
        _capi.check(lib, self._handle, lib.fd_read_tap(self._handle, name.encode(), buf.ctypes.data, n), "fd_read_tap")
        return buf

    def counter(self, name):
        """fd_get_counter: "pieces" / "pieces_redone" / "pieces_fp32" / "fp32_mask" of the last long sample() call, "calls_redone", "span_batches", "span_windows", ...."""
        lib = _capi.load()
        return int(_capi.check(lib, self._handle, lib.fd_get_counter(self._handle, name.encode()), "fd_get_counter"))

    def profile(self, reset=False):
        lib = _capi.load()
        stats = (_capi.FdKernelStat * 128)()
        n = lib.fd_get_profile(self._handle, stats, 128)
        res = {stats[i].name.decode(): (int(stats[i].launches), float(stats[i].total_ms)) for i in range(min(n, 128))}
        if reset:
            lib.fd_reset_profile(self._handle)
        return res

    @staticmethod
    def kernel_index(layer, in_ch, out_ch, tap):
        return _capi.load().fd_kernel_index(layer, in_ch, out_ch, tap)

    @staticmethod
    def bias_index(layer, out_ch):
        return _capi.load().fd_bias_index(layer, out_ch)

    # ---- internals ----------------------------------------------------------------------------------------
    @staticmethod
    def _require_device(*tensors):
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("fastdiff_amd.FastDiff runs only on a HIP device (no CPU fallback): move the module "
                                   "and its inputs to cuda")

    def _require_inference(self, *tensors):
        self._require_device(*tensors)
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            raise NotImplementedError("this entry point is the inference pipeline (no saved activations): only FastDiff.forward "
                                      "records an autograd graph (fastdiff_amd/train.py)")

    def _wave_call(self, *tensors):
        """(lib, handle, stream) of a waveform method: the tensors lie on one device and carry no autograd graph, the weights are synced."""
        self._require_inference(*tensors)
        device = tensors[0].device
        return (*self._ready(device), self._stream(device))

    def _prep_condition(self, c, B, device):
        c = c.to(device=device, dtype=torch.float32)
        if c.dim() == 2:                      # egs/demo.ipynb feeds [80,T]; the reference broadcasts it (modules.py:203)
            c = c.unsqueeze(0)
        if c.shape[0] != B:
            c = c.expand(B, -1, -1)
        assert c.shape[1] == self.cond_channels
        return c.contiguous()

    @staticmethod
    def _stream(device):
        return ct.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    _SIG_WALK_EVERY = 64

    def _state_signature(self):
        # (storage, version) of every parameter: changes when a tensor is moved (.cuda()), loaded (load_state_dict copies in place) or
        # written in place.  The walk over the module tree that finds the tensors (named_parameters(): ~150-250 us for 175 parameters,
        # a sixth of what a one-utterance sample call takes on the GPU) is done when the set of parameters can have changed
        # (_invalidate_params: _apply, load_state_dict, apply / remove_weight_norm) and otherwise on every 64th call, which catches a
        # parameter object replaced behind the module's back (torch.nn.utils.remove_weight_norm on a sub-module, an assignment);
        # in between only the known tensors are looked at (~30 us).
        self._sig_calls += 1
        if self._param_list is None or self._sig_calls % self._SIG_WALK_EVERY == 0:
            named = list(self.named_parameters())
            self._param_names = tuple(k for k, _ in named)
            self._param_list = [v for _, v in named]
        return self._param_names, tuple((v.data_ptr(), v._version) for v in self._param_list)

    def _invalidate_params(self):
        self._param_list = None

    def _apply(self, fn, *args, **kwargs):
        self._invalidate_params()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._invalidate_params()
        return super().load_state_dict(*args, **kwargs)

    def _ensure_handle(self, device):
        """The library and this module's context on `device`, created if needed (weights not looked at)."""
        lib = _capi.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._handle is None or self._handle_device != idx:
            self._release()
            cfg = _capi.FdConfig()
            lib.fd_default_config(ct.byref(cfg))
            c = self._cfg
            if len(c["upsample_ratios"]) > 8:
                raise NotImplementedError("at most 8 upsample stages")
            cfg.audio_channels, cfg.inner_channels, cfg.cond_channels = c["audio_channels"], c["inner_channels"], c["cond_channels"]
            cfg.n_upsample = len(c["upsample_ratios"])
            for i in range(8):
                cfg.upsample_ratios[i] = c["upsample_ratios"][i] if i < cfg.n_upsample else 0
            cfg.lvc_layers_each_block, cfg.lvc_kernel_size = c["lvc_layers_each_block"], c["lvc_kernel_size"]
            cfg.kpnet_hidden_channels, cfg.kpnet_conv_size = c["kpnet_hidden_channels"], c["kpnet_conv_size"]
            cfg.diffusion_step_embed_dim_in = c["diffusion_step_embed_dim_in"]
            cfg.diffusion_step_embed_dim_mid = c["diffusion_step_embed_dim_mid"]
            cfg.diffusion_step_embed_dim_out = c["diffusion_step_embed_dim_out"]
            cfg.use_weight_norm = int(bool(c["use_weight_norm"]))
            h = ct.c_void_p()
            rc = lib.fd_create(ct.byref(cfg), idx, ct.byref(h))
            _capi.check(lib, None, rc, "fd_create")
            self._handle, self._handle_device, self._synced_state = h, idx, None
            for k, v in self._options.items():
                _capi.check(lib, h, lib.fd_set_option(h, k.encode(), v.encode()), "fd_set_option")
            for variant, a in self.__dict__.get("_mel_banks", {}).items():      # caller-supplied filter banks follow the module to a new device
                _capi.check(lib, h, lib.fd_set_option(h, b"mel", variant.encode()), "fd_set_option")
                _capi.check(lib, h, lib.fd_set_mel_filterbank(h, a.ctypes.data, 80, 513), "fd_set_mel_filterbank")
        return lib

    def _ready(self, device):
        """Create the context on `device` if needed and (re)upload weights when any parameter changed."""
        lib = self._ensure_handle(device)
        sig = self._state_signature()
        if sig != self._synced_state:
            self._upload_weights(lib)
            self._synced_state = sig
            self._weights_dirty = False
            self.last_refresh = "host: a parameter tensor was moved, loaded or written in place" + self._source_suffix()
        elif self._weights_dirty:
            self.refresh_weights()
        return lib, self._handle

    def use_weights(self, source=None):
        """Choose what the inference entry points (forward under no_grad, sample, ...) compute with: None = the live parameters, or a
        fastdiff_amd.ParamEMA, or a mapping from every name of state_dict() to a tensor of that shape (device tensors are packed on the
        device like the parameters, anything else goes through the host).  Wrong names or shapes raise here.  The call only records the
        source and marks the handle's weights as stale: the next inference call repacks them (refresh_weights), and so does the first
        one after every TrainStep.step -- a ParamEMA's shadow has moved by then.  The differentiable forward (train() mode with
        gradients enabled) reads the live parameters whatever the source is.  Returns the previous source."""
        previous = self._weights_source
        self._weights_label = self.check_weights_source(source)
        self._weights_source = source
        self._weights_dirty = True
        return previous

    def check_weights_source(self, source):
        """Raise ValueError unless `source` is something use_weights takes for this module; returns its label for `last_refresh`."""
        if source is None:
            return None
        tensors = getattr(source, "tensors", source)
        if not hasattr(tensors, "keys"):
            raise ValueError(f"FastDiff.use_weights: a ParamEMA or a mapping from name to tensor is expected, got {type(source).__name__}")
        want = self.state_dict()
        missing = [k for k in want if k not in tensors]
        extra = [k for k in tensors.keys() if k not in want]
        if missing or extra:
            raise ValueError(f"FastDiff.use_weights: the source's names are not the module's (missing {missing[:3]}, unexpected {extra[:3]})")
        for k, t in want.items():
            if not torch.is_tensor(tensors[k]) or tuple(tensors[k].shape) != tuple(t.shape):
                raise ValueError(f"FastDiff.use_weights: {k}: expected a tensor of shape {list(t.shape)}, got "
                                 f"{list(tensors[k].shape) if torch.is_tensor(tensors[k]) else type(tensors[k]).__name__}")
        return type(source).__name__

    @property
    def weights_source(self):
        """What use_weights recorded last (None: the live parameters)."""
        return self._weights_source

    def _source_suffix(self):
        return "" if self._weights_source is None else f" (source: {self._weights_label})"

    def _weight_tensors(self):
        """name -> tensor of the recorded source, in state_dict() order."""
        sd = self.state_dict()
        src = self._weights_source
        if src is None:
            return sd
        tensors = getattr(src, "tensors", src)
        return {k: tensors[k].detach() for k in sd}

    def refresh_weights(self, stream=None):
        """Bring the inference handle's weights up to date with the parameters as they are NOW, on the device: the operand packs are
        rebuilt in place from the live tensors (fd_refresh_weights_device), asynchronously on `stream` (a torch.cuda.Stream; None = the
        current one), and the captured graphs stay valid.  For whoever writes parameters without torch noticing -- TrainStep.step sets
        the module's dirty flag, and the next forward() / sample() calls this by itself; call it directly after writing parameters through
        raw pointers of your own.  `last_refresh` says what happened: "device", or "host: <why>" when the weights went through
        fd_set_weight / fd_commit_weights instead (the module's parameters are not on a HIP device; an architecture other than
        base.yaml's; the handle's first weights, which lay the arena out; a parameter that is not contiguous float32).  With a source
        chosen by use_weights the tensors are that source's, and both strings end in " (source: <its type>)"."""
        p = next(self.parameters())
        if not p.is_cuda:
            if self._handle is None:       # nothing holds weights yet: the first inference call uploads them
                self.last_refresh = "host: the parameters are not on a HIP device (no handle yet: uploaded by the first inference call)"
                return
            lib, why = _capi.load(), "the parameters are not on a HIP device"
        else:
            lib, why = self._ensure_handle(p.device), None
            sd = self._weight_tensors()
            if self._synced_state is None:
                why = "the handle's first weights (fd_commit_weights lays the arena out)"
            elif not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in sd.values()):
                why = "a parameter is not a contiguous float32 tensor on the device"
            else:
                names = [k.encode() for k in sd]
                dims = [(ct.c_int64 * t.dim())(*t.shape) for t in sd.values()]
                items = (_capi.FdWeightRef * len(sd))(*[_capi.FdWeightRef(k, t.data_ptr(), ct.addressof(d), t.dim(), 0)
                                                        for k, t, d in zip(names, sd.values(), dims)])
                s = self._stream(p.device) if stream is None else ct.c_void_p(getattr(stream, "cuda_stream", stream))
                rc = lib.fd_refresh_weights_device(self._handle, items, len(sd), s)
                if rc == _capi.FD_ERR_UNSUPPORTED:
                    why = lib.fd_last_error(self._handle).decode()
                else:
                    _capi.check(lib, self._handle, rc, "fd_refresh_weights_device")
        if why is not None:
            self._upload_weights(lib)
        self.last_refresh = ("device" if why is None else "host: " + why) + self._source_suffix()
        self._synced_state = self._state_signature()
        self._weights_dirty = False

    def weight_image(self):
        """The handle's committed weight image as bytes (numpy uint8; fd_get_weight_image).  Synchronises.  For tests."""
        lib, n = _capi.load(), ct.c_size_t(0)
        _capi.check(lib, self._handle, lib.fd_get_weight_image(self._handle, None, ct.byref(n)), "fd_get_weight_image")
        buf = np.empty(n.value, np.uint8)
        _capi.check(lib, self._handle, lib.fd_get_weight_image(self._handle, buf.ctypes.data, ct.byref(n)), "fd_get_weight_image")
        return buf

    def weight_flags(self):
        """The six fp16-range flags of the handle's weights as bits (fd_get_weight_flags); waits for a pending refresh.  For tests."""
        lib, m = _capi.load(), ct.c_uint(0)
        _capi.check(lib, self._handle, lib.fd_get_weight_flags(self._handle, ct.byref(m)), "fd_get_weight_flags")
        return int(m.value)

    def _upload_weights(self, lib):
        h = self._handle
        for name, t in self._weight_tensors().items():
            a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            dims = (ct.c_int64 * a.ndim)(*a.shape)
            rc = lib.fd_set_weight(h, name.encode(), a.ctypes.data, dims, a.ndim)
            _capi.check(lib, h, rc, f"fd_set_weight({name})")
        _capi.check(lib, h, lib.fd_commit_weights(h), "fd_commit_weights")

    def _release(self):
        if self._handle is not None:
            try:
                _capi.load().fd_destroy(self._handle)
            finally:
                self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass
