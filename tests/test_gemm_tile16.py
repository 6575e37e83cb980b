"""The Winograd predictor GEMM on 16-row matrix tiles (option gemm_tile = 16, the default) against the float64 oracle at ITS borders
(run with -m gpu on an MI355X).

k_kp_gemm_w<16> builds a 64-frame item from two row tiles of 16 pairs (32 frames): a row tile that begins behind the utterance's end is
skipped, one that lies inside it stores through the buffer descriptor behind a 16-lane row exchange, one that straddles the end stores
lane by lane.  tests/test_tile_borders.py has the 64-frame item border; the frame counts here sit one short of, at and one past the
32-frame row tile inside the first and the second item, with an utterance boundary behind it in the persistent walk, and in a ragged
batch.  gemm_tile = 32 (the 32 x 32 x 16 body) runs the same cases.

The bar is the one of tests/test_tile_borders.py: FWD_TOL on every predicted tap, and below it K_PREDICTED x the float32 ORACLE's own
distance from float64 on the same tap and input -- never another run of the library.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5            # tests/test_tile_borders.py
K_PREDICTED = 3.0         # ... K["predicted"]
TAPS = ("kernels0", "kernels1", "kernels2", "bias0", "bias1", "bias2")
ARMS = ("16", "32")
# (B, T, lens): the row-tile border of the first item (32) and of the second (96); two utterances; a ragged batch whose first utterance
# ends one frame into a row tile and whose second ends in the middle of one, the two neighbours in the persistent walk
SHAPES = [(1, t, None) for t in (31, 32, 33, 95, 96, 97)] + [(2, 33, None), (2, 97, (97, 80))]
CASES = [(arm, B, T, lens) for (B, T, lens) in SHAPES for arm in ARMS]      # shape-major: one reference, both arms

_refs = {}       # (B, T, lens) -> inputs and, per segment (utterances, frames), float64 taps + the float32 oracle's gap per tap
_worst = {}      # arm -> (ratio, tap, B, T)


def _inputs(B, T):
    import synth
    seed = 1000 + 8 * T + B
    steps = np.array([(61.75 * T + 999.0 * b / B) % 999.0 for b in range(B)], np.float32)
    return synth.synth_audio(seed, B, T), synth.synth_mel(seed, B, T), steps


def _reference(oracle64, oracle32, B, T, lens):
    """Computed once per shape and left unchanged.  A ragged batch: each utterance alone at its own length (what `lens` promises)."""
    key = (B, T, lens)
    if key not in _refs:
        import gpu_common
        audio, mel, steps = _inputs(B, T)
        segments = []
        if lens is None:
            pieces = [(slice(0, B), T)]
        else:
            pieces = [(slice(b, b + 1), t) for b, t in enumerate(lens)]
            for b, t in enumerate(lens):
                mel[b, :, t:] = 0.0
                audio[b, :, t * 256:] = 0.0
        for sl, t in pieces:
            a, c, s = np.ascontiguousarray(audio[sl, :, : t * 256]), np.ascontiguousarray(mel[sl, :, :t]), steps[sl]
            _, ref64 = oracle64.forward(a, c, s, taps=True)
            _, ref32 = oracle32.forward(a, c, s, taps=True)
            gap32 = {k: gpu_common.maxdiff(ref32[k], ref64[k]) for k in TAPS}
            for k in TAPS:
                ref64[k].setflags(write=False)
            segments.append((sl, t, {k: ref64[k] for k in TAPS}, gap32))
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        _refs[key] = (audio, mel, steps, segments)
    return _refs[key]


def _model(tile, taps):
    import gpu_common
    m = gpu_common.make_model()
    m.set_option("gemm_tile", tile)
    m.set_option("taps", "1" if taps else "0")
    return m


@pytest.fixture(scope="module")
def handles():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(arm):
        if arm not in made:
            made[arm] = _model(arm, taps=True)
        return made[arm]

    yield get
    for m in made.values():
        m._release()
    for arm in ARMS:
        if arm in _worst:
            r, tap, B, T = _worst[arm]
            print(f"\ngemm_tile={arm}: worst err / gap32 = {r:.2f} ({tap} at B={B}, T={T})")


@pytest.mark.parametrize("arm,B,T,lens", [pytest.param(a, B, T, lens, id=f"tile{a}-B{B}-T{T}" + ("-ragged" if lens else ""))
                                          for a, B, T, lens in CASES])
def test_predicted_taps_against_float64_at_the_row_tile_borders(handles, oracle64, oracle32, arm, B, T, lens):
    import gpu_common as gc
    audio, mel, steps, segments = _reference(oracle64, oracle32, B, T, lens)
    m = handles(arm)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.no_grad():
        m((cu(audio), cu(mel), cu(steps.reshape(-1, 1))), lens=None if lens is None else list(lens))
    torch.cuda.synchronize()
    taps = gc.read_taps(m, B, T)
    flags = m.read_tap("range_flags").view(np.int32)
    failures = []
    for sl, t, ref64, gap32 in segments:
        for tap in TAPS:
            err = gc.maxdiff(taps[tap][sl, :, :t], ref64[tap])
            ratio = err / gap32[tap]
            if ratio > _worst.get(arm, (0.0,))[0]:
                _worst[arm] = (ratio, tap, B, T)
            bar = min(FWD_TOL, K_PREDICTED * gap32[tap])
            print(f"gemm_tile={arm} B={B} T={T} utterances {sl.start}..{sl.stop - 1} ({t} frames) {tap}: err {err:.3e}  gap32 {gap32[tap]:.3e}  "
                  f"ratio {ratio:.2f}  bar {bar:.3e}")
            if not err <= bar:
                d = np.abs(np.asarray(taps[tap][sl, :, :t], np.float64) - ref64[tap])
                idx = np.unravel_index(int(d.argmax()), d.shape)
                failures.append(f"gemm_tile={arm} {tap}: err {err:.3e} > bar {bar:.3e} (gap32 {gap32[tap]:.3e}, ratio {ratio:.2f}) at utterance "
                                f"{sl.start + idx[0]}, row {idx[1]}, frame {idx[2]} of {t}")
    assert not failures, "\n".join(failures)
    assert not flags.any(), (arm, np.flatnonzero(flags))


def _rows(N):
    return [{"t": 700.0 - 450.0 * k, "c_eps": 0.03, "c_div": 0.995, "sigma": 0.1, "c1": 1.0, "c2": 0.0, "c3": 0.0, "add_noise": int(k < N - 1)}
            for k in range(N)]


def test_hoisted_predictor_on_16_row_tiles_equals_the_stepwise_one():
    """hoist = on batches (step, utterance) entries along the axis the row tiles run over: N = 2 steps of B = 2 utterances of 33 frames,
    one frame past the first row tile; the waveform is the one of hoist = off, bit for bit."""
    import synth
    B, T, N = 2, 33, 2
    mel = torch.from_numpy(synth.synth_mel(91, B, T)).cuda()
    out = {}
    for hoist in ("on", "off"):
        m = _model("16", taps=False)
        m.set_option("hoist", hoist)
        try:
            with torch.no_grad():
                out[hoist] = m.sample(mel, _rows(N), seed=7)
            assert not m.read_tap("range_flags_call").view(np.int32).any(), hoist
        finally:
            m._release()
    assert torch.isfinite(out["on"]).all() and float(out["on"].abs().max()) > 0.0
    assert torch.equal(out["on"], out["off"])


def test_flipping_gemm_tile_on_a_warm_handle():
    """The option is part of the graph key: a handle that has run under one value runs the other value's kernel after a flip, and the
    first one's again after flipping back -- each result that of a fresh handle under the same value."""
    import synth
    B, T, N = 1, 33, 2
    mel = torch.from_numpy(synth.synth_mel(92, B, T)).cuda()
    fresh = {}
    for arm in ARMS:
        m = _model(arm, taps=False)
        try:
            with torch.no_grad():
                fresh[arm] = m.sample(mel, _rows(N), seed=9)
        finally:
            m._release()
    m = _model("16", taps=False)
    try:
        with torch.no_grad():
            for arm in ("16", "32", "16"):
                m.set_option("gemm_tile", arm)
                assert torch.equal(m.sample(mel, _rows(N), seed=9), fresh[arm]), arm
    finally:
        m._release()
