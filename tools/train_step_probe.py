"""Training-side timing: the reference's training shape -- max_sentences 20 x max_samples 25600 (base.yaml:50-51),
i.e. B = 20 utterance crops of T = 100 frames -- through FastDiff.forward in train() mode + loss.backward(), with the location-variable
convolution (a) on the HIP operator (fd_lvc_forward / fd_lvc_backward) and (b) as the reference states it, pad + unfold + einsum on
PyTorch-ROCm (modules.py:220-253 with dilation 1), on the same GPU; then the operator alone, forward and backward, per hop size.
The corpus rows: the replayed step fed from a device-resident TrainCorpus against the same step fed by a host loop that cuts the same
windows with numpy and copies them up.
Usage: python tools/train_step_probe.py [B] [T] [corpus]      (corpus: only the corpus rows)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

import fastdiff_amd
from fastdiff_amd import train


def lvc_unfold_einsum(x, kernel, bias, dilation, hop):
    """out[b,o,l*hop+s] = bias[b,o,l] + sum_{i,k} xpad[b,i,l*hop+s+k] kernel[b,i,o,k,l] the way eager PyTorch runs it."""
    B, _, L = x.shape
    win = F.pad(x, (1, 1)).unfold(2, hop + 2, hop).unfold(3, 3, 1)           # [B, in, T, hop, 3]
    out = torch.einsum("bithk,biokt->both", win, kernel) + bias.unsqueeze(-1)
    return out.reshape(B, -1, L)


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def full_step_row(B, T, rounds=7, reps=10):
    """A real training step both ways, alternating within one call, device-synchronised wall time per step (median and range over
    `rounds` rounds of `reps` steps):
      (a) fastdiff_amd.TrainStep.step: batch copy + one graph replay (draws, forward, loss, backward, clip, guard, AdamW on the device);
      (b) the recipe without it: CPU randint + std_normal + copy, x_t on the device, replay of the forward + backward graph,
          clip_grad_norm_, the reference's NaN scan (trainer.py:320-327), torch.optim.AdamW.step();
      (c) the forward + backward graph of (b) alone (the figure the rows above report)."""
    import statistics
    from fastdiff_amd import schedules, sampler
    dh = schedules.training_hyperparams()
    alpha = dh["alpha"].cuda()
    mel = (torch.rand(B, 80, T) * 7.5 - 6.0).cuda()
    wav = (0.3 * torch.randn(B, 1, T * 256)).cuda()
    try:
        ma, mb = fastdiff_amd.FastDiff().cuda().train(), fastdiff_amd.FastDiff().cuda().train()
        mb.load_state_dict(ma.state_dict())
        # (a)
        ts = fastdiff_amd.TrainStep(ma, dh, seed=1)
        ts.step(mel, wav)
        torch.cuda.synchronize()
        # (b): static inputs of the captured forward + backward
        x_s, z_s, st_s = torch.empty_like(wav), torch.empty_like(wav), torch.empty(B, 1, device="cuda")
        opt = torch.optim.AdamW(mb.parameters(), lr=2e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0)

        def draw():
            t = torch.randint(dh["T"], size=(B, 1, 1)).cuda()
            z = sampler.std_normal(wav.shape)
            a = alpha[t]
            x_s.copy_(a * wav + (1 - a ** 2.).sqrt() * z)
            z_s.copy_(z)
            st_s.copy_(t.view(B, 1))

        def fb():
            eps = train.differentiable_forward(mb, (x_s, mel, st_s), lvc=None)
            F.mse_loss(eps, z_s).backward()

        draw()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                mb.zero_grad(set_to_none=True)
                fb()
        torch.cuda.current_stream().wait_stream(side)
        mb.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fb()

        def recipe():
            draw()
            graph.replay()
            torch.nn.utils.clip_grad_norm_(mb.parameters(), 1.0)
            for _, p in mb.named_parameters():
                if (p.grad is not None) and torch.isnan(p.grad.float()).any():
                    raise RuntimeError("NaN gradient")
            opt.step()

        runs = {"(a) TrainStep.step, replayed": lambda: ts.step(mel, wav), "(b) draws on the CPU + forward/backward replay + clip + NaN scan + torch AdamW": recipe,
                "(c) forward + backward replay alone": graph.replay}
        times = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                times[k].append(timed(fn, warm=2, reps=reps))
        print(f"  a real training step at B={B} T={T}, {rounds} alternating rounds of {reps} steps (ms per step: median [min .. max]):")
        for k, v in times.items():
            print(f"    {k}: {statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]")
        st = ts.state()
        print(f"    TrainStep state after the run: {st}")
        # launches of one step: the kernels of the same calls run eagerly, counted by the profiler (the graph holds the same launches)
        from torch.profiler import profile, ProfilerActivity
        eager = fastdiff_amd.TrainStep(ma, dh, seed=1, graph=False)
        eager.step(mel, wav)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            eager.step(mel, wav)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        ours = [n for n in names if any(k in n for k in ("k_train_draw", "k_mse_", "k_adamw_"))]
        print(f"    kernel launches of one full step (eager, profiler): {len(names)}, of them draw / loss / optimizer: {len(ours)}")
    except Exception:      # noqa: BLE001 -- the rows behind this one still run; the probe then ends non-zero
        import traceback
        traceback.print_exc()
        print("  the full-step row FAILED (traceback above)")
        return False
    return True


def corpus_rows(B, T, rounds=7, reps=10, n_items=200):
    """Where the batch comes from, alternating within one call (device-synchronised wall time per step, median and range over `rounds`
    rounds of `reps` steps), on a synthetic corpus of `n_items` utterances of T + 1 .. 8 T frames:
      (a) TrainStep.step(): the batch cut inside the replayed step from the corpus in device memory;
      (b) TrainStep.step(mels, wavs): a single-process host loop computes the same picks (corpus.plan), cuts them out of the host arenas
          with numpy (slice, transpose, stack) and hands pageable tensors to the step, which copies them up and replays;
      (host) the host part of (b) alone, no device work."""
    import statistics
    import numpy as np
    from fastdiff_amd import schedules
    try:
        dh = schedules.training_hyperparams()
        rng = np.random.RandomState(0)
        lengths = rng.randint(T + 1, 8 * T + 1, size=n_items)
        items = [{"mel": (rng.rand(n, 80) * 7.5 - 6.0).astype(np.float32), "wav": (0.3 * rng.randn(n * 256)).astype(np.float32)} for n in lengths]
        cpu = fastdiff_amd.TrainCorpus(items, hop_size=256, max_samples=T * 256, device="cpu")
        dev = cpu.to("cuda")
        mel_h, wav_h, off = cpu.mel.numpy(), cpu.wav.numpy(), cpu.frame_off_host
        ma, mb = fastdiff_amd.FastDiff().cuda().train(), fastdiff_amd.FastDiff().cuda().train()
        mb.load_state_dict(ma.state_dict())
        ta = fastdiff_amd.TrainStep(ma, dh, seed=1, corpus=dev, batch_size=B)
        tb = fastdiff_amd.TrainStep(mb, dh, seed=1)
        count = [0]

        def host_cut():
            picks, starts = cpu.plan(count[0], B, seed=1)
            count[0] += 1
            first = off[picks] + starts
            mels = np.stack([mel_h[p: p + T].T for p in first])
            wavs = np.stack([wav_h[p * 256: (p + T) * 256] for p in first])[:, None, :]
            return torch.from_numpy(np.ascontiguousarray(mels)), torch.from_numpy(np.ascontiguousarray(wavs))

        ta.step()
        tb.step(*host_cut())
        torch.cuda.synchronize()
        same = torch.equal(ta.mel, tb.mel) and torch.equal(ta.wav, tb.wav)
        runs = {"(a) step() from the device-resident corpus, replayed": ta.step, "(b) step(mels, wavs) fed by a host loop (plan + numpy cut + copy), replayed": lambda: tb.step(*host_cut()),
                "(host) plan + numpy cut alone": host_cut}
        times = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                times[k].append(timed(fn, warm=2, reps=reps))
        print(f"  the batch source at B={B} T={T}, corpus of {cpu.n_items} items ({cpu.wav.numel() * 4 / 1e6:.0f} MB of waveform), {rounds} alternating rounds of {reps} steps (ms per step: median [min .. max]):")
        for k, v in times.items():
            print(f"    {k}: {statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]")
        print(f"    first batch of (a) and (b) identical: {same};  state of (a): {ta.state()}")
    except Exception:      # noqa: BLE001
        import traceback
        traceback.print_exc()
        print("  the corpus rows FAILED (traceback above)")
        return False
    return True


def main():
    if len(sys.argv) > 3 and sys.argv[3] == "corpus":
        return corpus_rows(int(sys.argv[1]), int(sys.argv[2]))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    torch.manual_seed(0)
    m = fastdiff_amd.FastDiff().cuda().train()
    mel = (torch.rand(B, 80, T) * 7.5 - 6.0).cuda()
    x = (0.3 * torch.randn(B, 1, T * 256)).cuda()
    z = torch.randn(B, 1, T * 256).cuda()
    steps = torch.randint(1000, (B, 1)).float().cuda()

    def step(lvc):
        m.zero_grad(set_to_none=True)
        eps = train.differentiable_forward(m, (x, mel, steps), lvc=lvc)
        F.mse_loss(eps, z).backward()

    def fwd(lvc):
        with torch.no_grad():
            train.differentiable_forward(m, (x, mel, steps), lvc=lvc)

    if os.environ.get("FD_LVC_DX"):      # gather (default) | copy: how the frames path's dx kernel gets its operands
        from fastdiff_amd import lvc_op
        lib, h = lvc_op._handle(torch.device("cuda"))
        assert lib.fd_set_option(h, b"lvc_dx", os.environ["FD_LVC_DX"].encode()) == 0
    print(f"training shape B={B} T={T} ({B * T * 256} samples)" + (f", lvc_dx = {os.environ['FD_LVC_DX']}" if os.environ.get("FD_LVC_DX") else ""))
    # frames: kernel_conv hands the LVC operator its frame-major operands (the product path); reference tensor: through the reference's
    # [B, layers, 32, 64, 3, T] kernels and the operator's transposes (module._train_frames = False)
    for name, lvc, frames in (("HIP operator, frames", None, True), ("HIP operator, reference tensor", None, False),
                              ("unfold+einsum (PyTorch-ROCm eager)", lvc_unfold_einsum, True)):
        try:
            m._train_frames = frames
            print(f"  forward + backward, LVC = {name}: {timed(lambda: step(lvc)):8.2f} ms   forward only (no_grad): {timed(lambda: fwd(lvc)):8.2f} ms")
        except Exception as e:      # noqa: BLE001 -- e.g. out of memory in the unfold view's backward
            print(f"  LVC = {name}: failed: {e!r}")
    m._train_frames = True
    # the same step captured once in a hipGraph (torch.cuda.graph) and replayed: what is left when the ~500 kernel launches of a step
    # cost no host time.  Variants: FD_TRAIN_VARIANTS=1 also replays the step without frames / without the fused predictor activations
    def graph_run(label, **attrs):
        try:
            for k, v in attrs.items():
                setattr(m, k, v)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step(None)
            torch.cuda.current_stream().wait_stream(side)
            m.zero_grad(set_to_none=True)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                eps = train.differentiable_forward(m, (x, mel, steps), lvc=None)
                loss = F.mse_loss(eps, z)
                loss.backward()
            graph.replay()
            torch.cuda.synchronize()
            g_graph = {n: p.grad.clone() for n, p in m.named_parameters()}
            loss_graph = float(loss.detach())
            step(None)
            torch.cuda.synchronize()
            worst = max(float((g_graph[n] - p.grad).abs().max()) / max(float(p.grad.abs().max()), 1e-20) for n, p in m.named_parameters())
            print(f"  forward + backward, LVC = HIP operator{label}, replayed from a hipGraph: {timed(graph.replay):8.2f} ms   eager: {timed(lambda: step(None)):8.2f} ms   (loss {loss_graph:.6f}; gradients vs the eager step: max relative difference {worst:.1e})")
        except Exception as e:      # noqa: BLE001
            print(f"  hipGraph capture of the training step{label} failed: {e!r}")
        finally:
            m._train_frames, m._train_fuse_act, m._train_skip_fan, m._train_stack, m._train_wn_all, m._train_fronts = True, True, True, True, True, True

    graph_run("")
    if os.environ.get("FD_TRAIN_VARIANTS"):
        graph_run(" [predictor front ends one by one]", _train_fronts=False)
        graph_run(" [weight-norm: one operator per convolution]", _train_wn_all=False)
        graph_run(" [residual stack: one node per pair]", _train_stack=False)
        graph_run(" [skip fan-out by autograd]", _train_skip_fan=False)
        graph_run(" [predictor activations as torch nodes]", _train_fuse_act=False)
        graph_run(" [reference kernel tensor + transposes]", _train_frames=False)
        graph_run("")
    full_ok = full_step_row(B, T)
    full_ok = corpus_rows(B, T) and full_ok
    for hop in (8, 64, 256):
        L = T * hop
        y = torch.randn(B, 32, L, device="cuda", requires_grad=True)
        k = (0.1 * torch.randn(B, 32, 64, 3, T, device="cuda")).requires_grad_(True)
        b = torch.randn(B, 64, T, device="cuda", requires_grad=True)
        d = torch.randn(B, 64, L, device="cuda")
        for name, op in (("HIP", fastdiff_amd.location_variable_convolution), ("unfold+einsum", lvc_unfold_einsum)):
            def f():
                with torch.no_grad():
                    op(y, k, b, 1, hop)

            def fb():
                y.grad = k.grad = b.grad = None
                op(y, k, b, 1, hop).backward(d)
            tf, tfb = timed(f), timed(fb)
            flops = 2.0 * B * L * 64 * 96
            print(f"  hop {hop:3d} {name:14s}: forward {tf:7.3f} ms ({flops / tf / 1e9:6.1f} TFLOP/s)   forward+backward {tfb:7.3f} ms ({3 * flops / tfb / 1e9:6.1f} TFLOP/s)")
    return full_ok


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
