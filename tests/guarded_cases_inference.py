"""Cases of the guarded-memory suite (tests/guarded_suite.py): forward, the sampler, long-form and streaming synthesis.
"""
import numpy as np
import torch

from guarded_suite import case, model, rows2

# =====================================================================================================================================
# Inference
# =====================================================================================================================================
def _sample_mask(B, T, lens):
    """True on the samples sample() / forward() specify: behind lens[b] * 256 a row is unspecified (FastDiff.sample)."""
    mask = torch.zeros(B, 1, T * 256, dtype=torch.bool)
    for b in range(B):
        mask[b, :, : (T if lens is None else lens[b]) * 256] = True
    return mask


def _infer(B, T):
    import synth
    lens_sets = [("", None)] + ([] if B == 1 else [("-short-first", sorted(range(T, T - B, -1))), ("-short-last", sorted(range(T, T - B, -1))[::-1])])
    if B > 1:
        lens_sets[1][1][0] = 1          # (the shortest item: one frame)
        lens_sets[2][1][-1] = 1

    def inputs(g, lens):
        mel = torch.from_numpy(synth.synth_mel(3, B, T).copy())
        x = torch.from_numpy(synth.hash_normal(3, 1, B * T * 256).reshape(B, 1, T * 256).copy())
        for b, v in enumerate(lens or []):
            mel[b, :, v:] = 0
            x[b, :, v * 256:] = 0
        return g.tensor(mel), g.tensor(x)

    @case(f"forward-{B}x{T}")
    def fwd(g):
        m, out, masks = model(), {}, {}
        for tag, lens in lens_sets:
            mel, x = inputs(g, lens)
            steps = g.tensor(torch.full((B, 1), 7.4132))
            with torch.no_grad():
                out["eps" + tag] = m((x, mel, steps), lens=lens)
            masks["eps" + tag] = _sample_mask(B, T, lens)
        return out, masks

    @case(f"sample-{B}x{T}")
    def smp(g):
        m, out, masks = model(), {}, {}
        for tag, lens in lens_sets:
            mel, x = inputs(g, lens)
            z = torch.from_numpy(np.stack([synth.hash_normal(3, 2 + n, B * T * 256).reshape(B, 1, T * 256) for n in range(2)]))
            with torch.no_grad():
                out["injected" + tag] = m.sample(mel, rows2(), x_T=x, noise=g.tensor(z), lens=lens)
                out["device-noise" + tag] = m.sample(mel, rows2(), seed=7, lens=lens)
            masks["injected" + tag] = masks["device-noise" + tag] = _sample_mask(B, T, lens)
        return out, masks


_infer(1, 1)
_infer(2, 17)
_infer(3, 49)


@case("sample-exact-T-buffers")
def _t_bucket(g, B=2, T=17):
    """Option t_bucket = 0: the library's buffers are laid out for T itself, not for T rounded up to 32 frames."""
    import synth
    m = model()
    m.set_option("t_bucket", "0")
    try:
        with torch.no_grad():
            y = m.sample(g.tensor(torch.from_numpy(synth.synth_mel(3, B, T).copy())), rows2(), seed=7, return_sequence=True)
    finally:
        m.set_option("t_bucket", "32")
    return {f"x{k}": t for k, t in enumerate(y)}


@case("sample-span-window")
def _span(g, T=200):
    """One window of tests/test_long_form.py's utterances: frames [64, 96) of 200, from the whole mel and from the part that holds its halo."""
    import synth
    from fastdiff_amd import longform
    m = model()
    mel = torch.from_numpy(synth.synth_mel(8, 1, T).copy())
    H = longform.halo_frames(2)
    lo, hi = max(0, 64 - H), min(T, 96 + H)
    with torch.no_grad():
        whole = longform.sample_span(m, g.tensor(mel), 0, T, 64, 96, rows2(), seed=5, stream_id=7)
        part = longform.sample_span(m, g.tensor(mel[:, :, lo:hi].contiguous()), lo, T, 64, 96, rows2(), seed=5, stream_id=7)
    return {"whole": whole, "part": part}


@case("sample-spans")
def _spans(g):
    """fd_sample_spans: two utterances in one call; outputs the caller places (the header promises any alignment: one 4 bytes off); and a
    stream pool, whose mel reaches its ring through fd_mel_ring_append."""
    import synth
    from fastdiff_amd import longform
    m = model()
    mels = [g.tensor(torch.from_numpy(synth.synth_mel(8 + i, 1, T).copy())) for i, T in enumerate((40, 70))]
    with torch.no_grad():
        ys = m.sample_long_batch(mels, rows2(), seed=5, stream_ids=[3, 4])
        outs = [g.empty((1, 1, 40 * 256), torch.float32, 4), g.empty((1, 1, 32 * 256), torch.float32, 0)]
        longform.sample_spans(m, [{"mel": mels[0][0], "out": outs[0], "mel_first": 0, "mel_frames": 40, "utt_frames": 40, "t0": 0, "t1": 40, "stream_id": 3},
                                  {"mel": mels[1][0], "out": outs[1], "mel_first": 0, "mel_frames": 70, "utt_frames": 70, "t0": 32, "t1": 64, "stream_id": 4}],
                              rows2(), seed=5)
        pool = m.stream_pool(rows2(), seed=5, max_streams=2, max_feed_frames=64)
        s = pool.open(3)
        pool.feed(s, g.tensor(mels[0][:, :, :25]))
        pool.feed(s, g.tensor(mels[0][:, :, 25:]))
        pool.close(s)
        piece = pool.step()[s]
    return {"long0": ys[0], "long1": ys[1], "placed0": outs[0], "placed1": outs[1], "pool": piece, "arena": pool.arena}
