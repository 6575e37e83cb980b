"""Which kernels a denoiser step launches, and how often, under every option that changes the choice: the labels and counts of
m.profile() after one forward and three sample calls per option set, compared with the recorded table tests/step_launches.json.

The table is recorded by this file itself through the public Python API only:
    python tests/test_step_launches.py [--digests] [--out PATH]
writes {case: {label: launches}} (with --digests also a SHA-256 of every call's output bytes under "<case>#sha256", for a one-off
comparison of two builds; the committed table holds no digests)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "step_launches.json")
B, T = 2, 5

OPTION_SETS = [
    ("default", {}),
    ("fallback=graph", {"fallback": "graph"}),
    ("hoist=off", {"hoist": "off"}),
    ("gemm_form=direct", {"gemm_form": "direct"}),
    ("gemm_tile=32", {"gemm_tile": "32"}),
    ("gemm=fp32", {"gemm": "fp32"}),
    ("lvc=fp32", {"lvc": "fp32"}),
    ("conv=fp32", {"conv": "fp32"}),
    ("lvc_h8=valu", {"lvc_h8": "valu"}),
    ("fuse_up=0", {"fuse_up": "0"}),
    ("fuse_final=0", {"fuse_final": "0"}),
    ("fuse_advance=0", {"fuse_advance": "0"}),
    ("taps=1", {"taps": "1"}),
    ("kernels=naive", {"kernels": "naive"}),
    ("kernels.first=naive", {"kernels.first": "naive"}),
    ("kernels.convt=naive", {"kernels.convt": "naive"}),
    ("kernels.lvc=naive", {"kernels.lvc": "naive"}),
    ("kernels.final=naive", {"kernels.final": "naive"}),
    ("kernels.kp_gemm=naive", {"kernels.kp_gemm": "naive"}),
]
# (name, reverse steps or None = a forward, lens): N = 2 is hoisted as one piece, N = 9 an 8-step piece plus a 1-step piece (hoist_chunk
# and the host check between the pieces)
CALLS = [("forward", None, None), ("sample_n2", 2, None), ("sample_n9", 9, None), ("sample_n2_ragged", 2, [5, 3])]
OVERFLOW = "default/sample_n2_overflow"      # x_T scaled out of the fp16 range: the host-checked redo with a non-zero fp32 mask


def _rows(N):
    return [{"t": float(3 + 5 * k), "c_eps": 0.05, "c_div": 1.0 + 0.01 * k, "sigma": 0.02, "c1": 1.0, "c2": 0.0, "c3": 0.0,
             "add_noise": int(k < N - 1)} for k in range(N)]


def _inputs():
    import synth
    import torch
    mel = torch.from_numpy(synth.synth_mel(17, B, T)).cuda()
    x = torch.from_numpy(synth.hash_normal(17, 1, B * T * 256).reshape(B, 1, T * 256)).cuda()
    steps = torch.tensor([[3.0], [40.0]], dtype=torch.float32).cuda()
    return mel, x, steps


def _model(options):
    import gpu_common
    m = gpu_common.make_model()
    for k, v in options.items():
        m.set_option(k, v)
    m.set_option("graph", "0")      # the scheme of test_tile_borders._launched: every launch one by one, with its label
    m.set_option("profile", "1")
    return m


def _one_call(m, N, lens, mel, x, steps, scale=1.0):
    """({label: launches}, SHA-256 of the output bytes) of one call."""
    import torch
    m.profile(reset=True)
    with torch.no_grad():
        if N is None:
            y = m((x * scale, mel, steps), lens=lens)
        else:
            y = m.sample(mel, _rows(N), x_T=x * scale, seed=7, lens=lens)
    torch.cuda.synchronize()
    launched = {k: v[0] for k, v in sorted(m.profile(reset=True).items())}
    return launched, hashlib.sha256(np.ascontiguousarray(y.cpu().numpy()).tobytes()).hexdigest()


def _run_set(name, options, digests=False):
    """{case: {label: launches}} of one option set (and its digests)."""
    mel, x, steps = _inputs()
    m = _model(options)
    out = {}
    for call, N, lens in CALLS:
        try:
            launched, sha = _one_call(m, N, lens, mel, x, steps)
        except NotImplementedError:      # a ragged batch with any stage on the naive set is refused: the table says so
            assert lens is not None and any(k.startswith("kernels") for k in options)
            launched, sha = {"refused": 1}, ""
        out[f"{name}/{call}"] = launched
        if digests:
            out[f"{name}/{call}#sha256"] = sha
    if name == "default":
        launched, sha = _one_call(_model(options), 2, None, mel, x, steps, scale=3.0e5)
        out[OVERFLOW] = launched
        if digests:
            out[OVERFLOW + "#sha256"] = sha
    return out


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", OPTION_SETS, ids=[n for n, _ in OPTION_SETS])
def test_launches_match_the_recorded_table(name, options, table):
    got = _run_set(name, options)
    want = {k: v for k, v in table.items() if k.split("/")[0] == name}
    assert sorted(got) == sorted(want)
    for case in sorted(got):
        assert got[case] == want[case], (case, {k: (got[case].get(k), want[case].get(k))
                                                for k in sorted(set(got[case]) | set(want[case])) if got[case].get(k) != want[case].get(k)})
    if name == "default":      # the overflow case is in the table only if it does run the second pass with stages on fp32
        assert want[OVERFLOW] != want["default/sample_n2"]


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else TABLE
    rec = {}
    for set_name, opts in OPTION_SETS:
        rec.update(_run_set(set_name, opts, digests="--digests" in sys.argv))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:      # one case per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(rec[k], sort_keys=True)}" for k in sorted(rec)) + "\n}\n")
    print(f"{len(rec)} entries -> {path}")
