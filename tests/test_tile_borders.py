"""Every shipped kernel variant, tap by tap, against the float64 oracle one frame to either side of each tile or window border
(run with -m gpu on an MI355X).

tests/test_gpu_parity.py holds the intermediates to float64 at frame counts that straddle no border, and holds the border lengths to
`eps` alone or to the fp32 kernel set, which shares the tiling, the halo logic and lvc_tile_of_workgroup with the default set.  Here
the frame counts are the smallest ones a frame short of, at, and a frame past each border in the code (SHAPES), the variants are the
ones an option or a fallback can select (VARIANTS), and every tap of every (variant, shape) is compared with the float64 oracle.

The bar.  FWD_TOL is the hard absolute bar on every tap.  Below it sits a bar per tap, proportional to the float32 ORACLE's own
distance from float64 on the same input and tap:  err <= K[family] * maxdiff(ref32[tap], ref64[tap]).  The yardstick is the reference
computed in float32, never another run of the library.  An error of order 2^-11 relative in a few predicted coefficients or in one
halo column vanishes inside FWD_TOL on eps; in the tap where it arises it is tens of times the float32 rounding noise.  K was measured
(LABBOOK R13.1: the worst ratio over all variants and shapes, doubled because the maximum over 1e5 .. 1e7 elements moves by tens of
percent between seeds, rounded up to one digit) and is not to be raised to make a failing kernel pass.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5          # tests/test_gpu_parity.py: one forward against the oracle
LOOP_TOL = 1e-4         # ... and an N <= 8 loop with injected noise

# frames per border: the 128-column tile of DBlock 2 (8 columns a frame); KPF_VALID, the predictor front's tile; the 64-frame item of
# both fp16x2 GEMM forms (32 Winograd pairs, 2 frame tiles) and the 64-tile period of lvc_tile_of_workgroup at hop 256; the fp32
# GEMM's 128-frame chunk (GEMM_CT * 32) and the 128-column tile of DBlock 3.  T = 1, 2, 3, 5: one frame, a Winograd pair whose second
# frame is outside, T % 4 for the 4-frame workgroups of the hop-8 and hop-64 LVC layers, the two-frame tiles of DBlock 1.
BORDERS = (16, 48, 64, 128)
SHAPES = [(1, t) for t in (1, 2, 3, 5, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129)]
SHAPES += [(2, 65), (3, 49)]      # the same borders with an utterance boundary right behind them: neighbours in the persistent walk
SHAPES += [(2, 193)]              # three whole GEMM items plus one frame
NAIVE_MAX_T = 17                  # the one-thread-per-output set: the yardstick of test_each_fast_stage_against_oracle, held to the taps here

VARIANTS = {
    "default": {},
    "direct": {"gemm_form": "direct"},      # k_kp_gemm_h2, the image write of k_kp_front_h2, k_h_split: also the library's own fall-back
    "valu": {"lvc_h8": "valu"},             # k_lvc_h8: the all-VALU hop-8 layer, the fp32 twin of k_lvc_h8m
    "fp32": {"gemm": "fp32", "lvc": "fp32", "conv": "fp32"},
    "naive": {"kernels": "naive"},
}
CASES = [(v, B, T) for (B, T) in SHAPES for v in VARIANTS if v != "naive" or T <= NAIVE_MAX_T]      # shape-major: one reference, all variants

TAPS = ("a0", "a1", "a2", "a3", "kernels0", "kernels1", "kernels2", "bias0", "bias1", "bias2", "x0", "x1", "x2", "y")
# err_hip / gap32, twice the worst measured ratio per family, rounded up to one digit (LABBOOK R13.1)
K = {"a": 4.0, "predicted": 3.0, "x": 4.0, "y": 4.0}


def _family(tap):
    return "predicted" if tap.startswith(("kernels", "bias")) else tap[0]


_refs = {}       # (B, T) -> inputs, float64 taps, float32 oracle's gap per tap; the last two shapes (the cases run shape-major)
_worst = {}      # (variant, tap) -> (ratio, B, T): the table behind K, printed when the module's handles are destroyed


def _inputs(B, T):
    import synth
    seed = 1000 + 8 * T + B
    steps = np.array([(61.75 * T + 999.0 * b / B) % 999.0 for b in range(B)], np.float32)      # spread over [0, 999]
    return synth.synth_audio(seed, B, T), synth.synth_mel(seed, B, T), steps


def _reference(oracle64, oracle32, B, T):
    """The float64 oracle's taps and the float32 oracle's distance from them, computed once per shape and left unchanged."""
    if (B, T) not in _refs:
        audio, mel, steps = _inputs(B, T)
        y64, ref64 = oracle64.forward(audio, mel, steps, taps=True)
        y32, ref32 = oracle32.forward(audio, mel, steps, taps=True)
        ref64["y"], ref32["y"] = y64, y32
        import gpu_common
        gap32 = {k: gpu_common.maxdiff(ref32[k], ref64[k]) for k in TAPS}
        for a in ref64.values():
            a.setflags(write=False)
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        _refs[(B, T)] = (audio, mel, steps, {k: ref64[k] for k in TAPS}, gap32)
    return _refs[(B, T)]


@pytest.fixture(scope="module")
def handles():
    """One handle per variant, made on first use with its options set once and taps = 1; all destroyed at the end of the module."""
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(variant):
        if variant not in made:
            m = gpu_common.make_model()
            for k, v in VARIANTS[variant].items():
                m.set_option(k, v)
            m.set_option("hoist", "on")       # (the sampler cases; a forward has no steps to hoist over)
            m.set_option("taps", "1")
            made[variant] = m
        return made[variant]

    yield get
    for m in made.values():
        m._release()
    if _worst:
        print("\nworst err / gap32 per variant and tap (B, T of the worst shape):")
        for variant in VARIANTS:
            row = [f"{tap} {_worst[(variant, tap)][0]:.2f}@{_worst[(variant, tap)][1]}x{_worst[(variant, tap)][2]}"
                   for tap in TAPS if (variant, tap) in _worst]
            if row:
                print(f"  {variant:8s}" + "  ".join(row))


def _where(got, ref, T):
    """The worst element of a tap: its utterance and frame, and where that frame lies relative to the borders of the table."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    idx = np.unravel_index(int(d.argmax()), d.shape)
    f = int(idx[-1]) // (d.shape[-1] // T)
    near = min(((abs(f - m), -w, m) for w in BORDERS for m in range(w, T + 1, w)), default=None)      # a tie: the widest border
    txt = f"utterance {idx[0]}, channel/row {idx[1]}, frame {f} of {T} ({f - T:+d} from the end, frame % 4 = {f % 4}"
    if near is not None:
        txt += f", {f - near[2]:+d} from the {-near[1]}-frame border at frame {near[2]}"
    return txt + ")"


def _launched(m, audio, mel, steps):
    """Labels of the kernels one eager forward launches (the scheme of test_weight_out_of_fp16_range_...: graph = 0, profile = 1)."""
    import gpu_common
    m.set_option("graph", "0")
    m.set_option("profile", "1")
    try:
        m.profile(reset=True)
        y = gpu_common.run_forward(m, audio, mel, steps)
        launched = m.profile(reset=True)
    finally:
        m.set_option("profile", "0")
        m.set_option("graph", "1")
    return launched, y


def _check_launches(variant, launched):
    names = sorted(launched)
    if variant == "default":
        assert "h_wino" in launched and "kp_gemm_f16x2" in launched and "kp_gemm" not in launched, names
        assert launched["lvc_fp32_fallback"][0] == 12, launched      # a forward enqueues the fp32 twin behind every fp16 LVC layer
    elif variant == "direct":
        assert "kp_gemm_f16x2" in launched and "h_wino" not in launched and "kp_gemm" not in launched, names
    elif variant == "valu":
        # k_lvc_h8 as the layer itself carries the layer's label and has no twin behind it: of the 12 lvc_fp32_fallback launches of
        # the default set, the 8 of the hop-64 and hop-256 layers remain (the test tells the two hop-8 kernels apart by their bits too)
        assert all(launched.get(f"lvc_layer_h8_d{d}", (0,))[0] == 1 for d in (1, 3, 9, 27)), launched
        assert launched["lvc_fp32_fallback"][0] == 8 and "h_wino" in launched, launched
    elif variant == "fp32":
        assert "kp_gemm" in launched and "kp_gemm_f16x2" not in launched and "h_wino" not in launched, names
        assert not any(n.endswith("fp32_fallback") for n in launched), names
    else:
        assert "naive_lvc_conv" in launched and "naive_kp_res" in launched and "kp_gemm_f16x2" not in launched, names


@pytest.mark.parametrize("variant,B,T", [pytest.param(v, B, T, id=f"{v}-B{B}-T{T}") for v, B, T in CASES])
def test_every_tap_against_float64_at_a_border(handles, oracle64, oracle32, variant, B, T):
    import gpu_common as gc
    audio, mel, steps, ref64, gap32 = _reference(oracle64, oracle32, B, T)
    m = handles(variant)
    y = gc.run_forward(m, audio, mel, steps)
    taps = gc.read_taps(m, B, T)
    taps["y"] = y
    flags = m.read_tap("range_flags").view(np.int32)
    launched, y_eager = _launched(m, audio, mel, steps)
    failures = []
    for tap in TAPS:
        err = gc.maxdiff(taps[tap], ref64[tap])
        ratio = err / gap32[tap]
        if ratio > _worst.get((variant, tap), (0.0,))[0]:
            _worst[(variant, tap)] = (ratio, B, T)
        bar = min(FWD_TOL, K[_family(tap)] * gap32[tap])
        print(f"{variant} B={B} T={T} {tap}: err {err:.3e}  gap32 {gap32[tap]:.3e}  ratio {ratio:.2f}  bar {bar:.3e}")
        if not err <= bar:
            failures.append(f"{variant} {tap}: err {err:.3e} > bar {bar:.3e} (gap32 {gap32[tap]:.3e}, ratio {ratio:.2f}) at "
                            + _where(taps[tap], ref64[tap], T))
    assert not failures, "\n".join(failures)
    assert not flags.any(), (variant, np.flatnonzero(flags))
    _check_launches(variant, launched)
    assert np.array_equal(y_eager, y), variant          # the profiled eager call ran the same kernels on the same input
    if variant == "valu":                                # ... and those are not k_lvc_h8m: same predictor bits, other hop-8 bits
        d = handles("default")
        gc.run_forward(d, audio, mel, steps)
        x0 = d.read_tap("x0").reshape(B, 32, T * 8)
        assert np.array_equal(d.read_tap("kpack0"), m.read_tap("kpack0")) and not np.array_equal(x0, taps["x0"])


@pytest.mark.parametrize("variant", ["default", "direct"])
def test_hoisted_sampler_at_the_gemm_item_border(handles, oracle64, variant):
    """The hoisted predictor batches (step, utterance) entries along the axis the Winograd pairs and the direct form's frame tiles run
    over: N = 3 steps of a ragged batch whose utterances end one frame past and one frame short of the 64-frame item, each against
    the float64 oracle's loop on that utterance alone at its own length."""
    import gpu_common as gc
    import synth
    B, T, N = 2, 65, 3
    lens = [65, 63]
    rows, table = gc.table_rows(load_golden("schedule"), N)
    mel = synth.synth_mel(71, B, T)
    for b, t in enumerate(lens):
        mel[b, :, t:] = 0.0
    x_T = synth.hash_normal(71, 1, B * T * 256).reshape(B, 1, T * 256)
    z = gc.noise_from_seed(71, B, T, N)
    m = handles(variant)
    m.set_option("taps", "0")          # a call that keeps taps does not hoist
    args = dict(x_T=torch.from_numpy(x_T).cuda(), noise=torch.from_numpy(gc.exec_order_noise(z)).cuda(), lens=lens)
    try:
        with torch.no_grad():
            y = m.sample(torch.from_numpy(mel).cuda(), rows, **args).cpu().numpy()
            flags = m.read_tap("range_flags_call").view(np.int32)
            m.set_option("graph", "0")      # the same call launched one by one: its profile shows ONE predictor for the three steps
            m.set_option("profile", "1")
            m.profile(reset=True)
            y_eager = m.sample(torch.from_numpy(mel).cuda(), rows, **args).cpu().numpy()
            launched = m.profile(reset=True)
    finally:
        m.set_option("profile", "0")
        m.set_option("graph", "1")
        m.set_option("taps", "1")
    assert not flags.any(), (variant, np.flatnonzero(flags))
    assert launched["kp_gemm_f16x2"][0] == 1 and launched["kp_front"][0] == 1, launched
    assert ("h_wino" in launched) == (variant == "default"), sorted(launched)
    for b, t in enumerate(lens):
        n = t * 256
        assert np.array_equal(y_eager[b, :, :n], y[b, :, :n]), (variant, b)
        ref = oracle64.sample(mel[b:b + 1, :, :t], table, x_T[b:b + 1, :, :n], np.ascontiguousarray(z[:, b:b + 1, :, :n]))
        d = gc.maxdiff(y[b:b + 1, :, :n], ref)
        print(f"{variant} hoisted N={N} utterance {b} (T={t}): max|d| = {d:.3e}")
        assert d < LOOP_TOL, (variant, b, t, d)
