"""The binding is read from the three public headers (fastdiff_amd/_capi.py: read_headers).  Pinned here from outside the reader: the
C compiler's sizeof / offsetof of every struct and the value of every constant; the derived prototypes of a handful of entry points that
together hold every mapping of the rule, spelled out; that nothing in the headers is passed over and that a declaration outside the
grammar is refused by name; and the consumers that read C structs by field (lvc_op's state readers, its item tables, the view of one
field) on bytes laid out with struct.pack at the compiler's offsets."""
import ctypes as ct
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from fastdiff_amd import _capi, lvc_op

INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def cc_says(tmp_path_factory):
    """{"sizeof": {struct: bytes}, "offsetof": {(struct, field): bytes}, "value": {constant: int}} as a C99 compiler sees the headers."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("needs a C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + ['#include "%s"' % h for h in _capi.HEADERS] + ["int main(void) {"]
    for s in _capi.STRUCTS:
        lines.append('    printf("sizeof %s - %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['    printf("offsetof %s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in _capi.record(s).names]
    lines += ['    printf("value %s - %%lld\\n", (long long)%s);' % (c, c) for c in _capi.CONSTANTS if c != "FD_BINS_RECORD_BYTES"]
    lines += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("capi")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-I" + INCLUDE, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {"sizeof": {}, "offsetof": {}, "value": {}}
    for kind, a, b, n in (ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()):
        out[kind][a if b == "-" else (a, b)] = int(n)
    return out


def _stripped():
    return [_capi._COMMENT.sub(" ", open(os.path.join(INCLUDE, h)).read()) for h in _capi.HEADERS]


def test_every_struct_is_laid_out_as_the_compiler_lays_it_out(cc_says):
    assert len(cc_says["sizeof"]) == len(_capi.STRUCTS) == sum(len(re.findall(r"\btypedef\s+struct\s+\w+\s*\{", t)) for t in _stripped())
    n = 0
    for s in _capi.STRUCTS:
        rec, cls = _capi.record(s), _capi.struct(s)
        assert rec.itemsize == ct.sizeof(cls) == cc_says["sizeof"][s], s
        assert list(rec.names) == [f[0] for f in cls._fields_]
        for f in rec.names:
            assert rec.fields[f][1] == getattr(cls, f).offset == cc_says["offsetof"][s, f], (s, f)
            assert rec.fields[f][0].itemsize == getattr(cls, f).size, (s, f)
            n += 1
    assert n == len(cc_says["offsetof"])


def test_every_constant_has_the_compiler_s_value(cc_says):
    assert cc_says["value"] == {k: v for k, v in _capi.CONSTANTS.items() if k != "FD_BINS_RECORD_BYTES"}
    assert _capi.FD_BINS_RECORD_BYTES == cc_says["sizeof"]["fd_bins"]
    for k, v in _capi.CONSTANTS.items():
        assert getattr(_capi, k) == v
    assert (_capi.FD_OK, _capi.FD_ERR_INVALID, _capi.FD_ERR_MISSING, _capi.FD_GL_PHILOX_STREAM, _capi.FD_PCM_U8) == (0, -1, -5, 0xFFFFFFF8, 3)


def test_prototypes_spelled_out():
    vp, ci, i64, u64, cf, cd, cs = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_uint64, ct.c_float, ct.c_double, ct.c_char_p
    expected = {
        "fd_version": (cs, []),
        "fd_sample_ticket": (i64, [vp]),
        "fd_sample": (ci, [vp, vp, ci, ci, vp, vp, ci, ci, vp, vp, u64, vp, vp, vp]),
        "fd_loudness_normalize": (ci, [vp, vp, ci, i64, vp, ci, cd, vp, vp, vp, vp]),
        "fd_dtw": (ci, [vp, vp, vp, ci, ci, i64, i64, i64, vp, vp, vp, vp, i64, vp]),
        "fd_kconv_backward_w_multi": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, cf, vp, vp, vp]),
        "fd_pwg_default_config": (None, [vp]),
        "fd_get_weight_image": (ci, [vp, vp, vp]),
        "fd_create": (ci, [vp, ci, vp]),
        "fd_set_weight": (ci, [vp, cs, vp, vp, ci]),
    }
    for name, want in expected.items():
        assert _capi.PROTOTYPES[name] == want, name
    # the scalars no prototype passes by value, through a fragment
    _, structs, protos = _capi.read_headers([("f.h", "typedef struct fd_c *fd_h;\nFD_API double fd_f(fd_h h, unsigned a, size_t b, int32_t c, "
                                                     "const char *const *d, char *e, fd_h *f);")])
    assert protos == {"fd_f": (cd, [vp, ct.c_uint, ct.c_size_t, ct.c_int32, vp, vp, vp])} and structs == {}


def test_nothing_in_the_headers_is_passed_over():
    texts = _stripped()
    assert len(_capi.EXPORTS) == len(set(_capi.EXPORTS)) == sum(len(re.findall(r"\bFD_API\b", t)) for t in texts) - 1      # (its own #define)
    assert sum(len(re.findall(r"\btypedef\s+struct\b", t)) for t in texts) == len(_capi.STRUCTS) + 2                       # (the two handles)
    assert sum(len(re.findall(r"#\s*define\s+FD_\w+[ \t]+[\d(-]", t)) for t in texts) + \
        sum(len(re.findall(r"\bFD_\w+\s*(?:=[^,}]*)?[,}]", body)) for t in texts for body in re.findall(r"\benum\b[^{;]*(\{[^}]*\})", t)) == \
        len(_capi.CONSTANTS) - 1                                                                                           # (FD_BINS_RECORD_BYTES)
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libfastdiff_hip.so is not built")
    lib = _capi.load()
    for name in _capi.EXPORTS:
        fn = vars(lib)[name]
        assert (fn.restype, list(fn.argtypes)) == _capi.PROTOTYPES[name], name


_HANDLE = "typedef struct fd_context *fd_handle;\n"


@pytest.mark.parametrize("fragment, declaration, token", [
    (_HANDLE + "FD_API int fd_f(fd_handle h,\n    const foo_t *x);", "FD_API int fd_f(fd_handle h, const foo_t *x);", "foo_t"),
    ("typedef struct fd_a { int32_t n; float v[FD_NOPE]; } fd_a;", "typedef struct fd_a { int32_t n; float v[FD_NOPE]; } fd_a;", "FD_NOPE"),
    ("typedef struct fd_a { int32_t n; } fd_a;\nFD_API int fd_f(fd_a a);", "FD_API int fd_f(fd_a a);", "fd_a"),
    ("FD_API int fd_f(int v[4]);", "FD_API int fd_f(int v[4]);", "v[4]"),
    ("FD_API int fd_f(int (*cb)(int));", "FD_API int fd_f", "FD_API"),
    ("enum { FD_A = 1, FD_B = FD_A + 1 };", "enum { FD_A = 1, FD_B = FD_A + 1 };", "FD_A + 1"),
    ("#define FD_N (3 * 4)", "#define FD_N (3 * 4)", "3 * 4"),
    ("int fd_hidden(void);", "int fd_hidden(void)", "int"),
    ("FD_API int fd_f(void);\nFD_API int fd_f(void);", "FD_API int fd_f(void);", "fd_f"),
    ("FD_API int fd_f(int FD_API);", "FD_API", "2"),
])
def test_a_declaration_outside_the_grammar_is_refused_by_name(fragment, declaration, token):
    with pytest.raises(_capi.HeaderError) as e:
        _capi.read_headers([("fragment.h", fragment)])
    msg = str(e.value)
    assert msg.startswith("fragment.h: ") and declaration in msg and token in msg, msg


def test_the_grammar_s_corners():
    consts, structs, _ = _capi.read_headers([("f.h", """
        #define FD_A 0x10u   /* hex */
        #define FD_B (1 << 4)
        #define FD_C FD_API_TEXT(x)
        #define FD_D 7UL
        enum fd_e { FD_E0, FD_E1, FD_E5 = 5, FD_E6, FD_EM = -2, FD_EN };   // running values
        typedef struct fd_s { const float *v, *g; int32_t cols, reserved; char name[FD_A]; double s[FD_D]; const char *text; } fd_s;
    """)])
    assert consts == {"FD_A": 16, "FD_B": 16, "FD_D": 7, "FD_E0": 0, "FD_E1": 1, "FD_E5": 5, "FD_E6": 6, "FD_EM": -2, "FD_EN": -1}
    assert [(f, k[0], n) for f, k, n in structs["fd_s"]] == [("v", ct.c_void_p, None), ("g", ct.c_void_p, None), ("cols", ct.c_int32, None),
                                                            ("reserved", ct.c_int32, None), ("name", ct.c_char, 16), ("s", ct.c_double, 7),
                                                            ("text", ct.c_char_p, None)]


# ---- the consumers that read structs by field, on bytes this file lays out ------------------------------------------------------------
def _packed(cc_says, name, dtype, **fields):
    """struct `name` as a CPU tensor of `dtype` words: every field packed at the compiler's offset with the format given for it."""
    buf = bytearray(cc_says["sizeof"][name])
    assert {f for s, f in cc_says["offsetof"] if s == name} >= set(fields)
    for f, (fmt, *values) in fields.items():
        struct.pack_into("<" + fmt, buf, cc_says["offsetof"][name, f], *values)
    return torch.frombuffer(buf, dtype=dtype)


def test_state_readers_read_the_compiler_s_layout(cc_says):
    t = _packed(cc_says, "fd_train_state", torch.int64, iter=("Q", 2 ** 63 + 5), applied=("Q", 11), skipped=("Q", 3), grad_norm=("f", 1.5), loss=("f", 0.375))
    assert lvc_op.read_train_state(t) == {"iter": 2 ** 63 + 5, "applied": 11, "skipped": 3, "grad_norm": 1.5, "loss": 0.375}
    assert t.shape == lvc_op.new_train_state("cpu").shape and t.dtype == lvc_op.new_train_state("cpu").dtype
    t = _packed(cc_says, "fd_ema_state", torch.int64, updates=("Q", 7), seen_applied=("Q", 2 ** 40 + 1), w=("f", 0.125), apply=("i", 1))
    assert lvc_op.read_ema_state(t) == {"updates": 7, "seen_applied": 2 ** 40 + 1, "w": 0.125, "apply": 1}
    assert t.shape == lvc_op.new_ema_state("cpu").shape
    sums, counts = [0.5 * k + 1 for k in range(64)], [1000 + k for k in range(64)]
    t = _packed(cc_says, "fd_eval_state", torch.int64, sum=("d", 123.25), count=("Q", 77), nonfinite=("Q", 4), reserved=("Q", 99),
                bin_sum=("64d", *sums), bin_count=("64Q", *counts))
    got = lvc_op.read_eval_state(t, bins=3)
    assert (got["sum"], got["count"], got["nonfinite"]) == (123.25, 77, 4) and set(got) == {"sum", "count", "nonfinite", "bin_sum", "bin_count"}
    assert got["bin_sum"].dtype == np.float64 and got["bin_sum"].tolist() == sums[:3]
    assert got["bin_count"].dtype == np.int64 and got["bin_count"].tolist() == counts[:3]
    assert t.shape == lvc_op.new_eval_state("cpu").shape
    found = [0.25 * k + 0.5 for k in range(64)]
    t = _packed(cc_says, "fd_sched_state", torch.int32, alpha_cur=("f", 0.75), beta_cur=("f", 0.0625), stopped=("i", 1), n_found=("i", 5),
                found=("64f", *found), step=("f", 17.0), ddim=("i", 1), coef=("4f", 9.0, 10.0, 11.0, 12.0), cond=("2f", 13.0, 14.0))
    got = lvc_op.read_sched_state(t)
    assert got.pop("found").tolist() == found[:5]
    assert got == {"alpha_cur": 0.75, "beta_cur": 0.0625, "stopped": 1, "n_found": 5, "step": 17.0}
    assert (lvc_op.EVAL_MAX_BINS, lvc_op.SCHED_MAX_STEPS) == (cc_says["value"]["FD_EVAL_MAX_BINS"], cc_says["value"]["FD_SCHED_MAX_STEPS"])


def test_one_field_of_a_state_is_found_by_name(cc_says):
    """PhiStep copies the loss out of its fd_train_state through this view: float32 word 7."""
    state = lvc_op.new_train_state("cpu")
    loss = lvc_op.state_field(state, "fd_train_state", "loss")
    assert loss.dtype == torch.float32 and loss.shape == (1,) and loss.data_ptr() - state.data_ptr() == cc_says["offsetof"]["fd_train_state", "loss"] == 4 * 7
    state.view(torch.float32)[7] = 2.5
    assert float(loss) == 2.5
    hyper = lvc_op.pack_state("fd_adamw_hyper", torch.float64, lr=1.0, beta1=2.0, beta2=3.0, eps=4.0, weight_decay=5.0, max_norm=6.0)
    assert bytes(hyper.numpy().tobytes()) == bytes(_packed(cc_says, "fd_adamw_hyper", torch.float64, lr=("d", 1.0), beta1=("d", 2.0), beta2=("d", 3.0),
                                                           eps=("d", 4.0), weight_decay=("d", 5.0), max_norm=("d", 6.0)).numpy().tobytes())
    lr = lvc_op.state_field(hyper, "fd_adamw_hyper", "lr")
    assert lr.dtype == torch.float64 and lr.data_ptr() - hyper.data_ptr() == cc_says["offsetof"]["fd_adamw_hyper", "lr"]
    ema = lvc_op.pack_state("fd_ema_state", seen_applied=9)
    assert lvc_op.read_ema_state(ema) == {"updates": 0, "seen_applied": 9, "w": 0.0, "apply": 0}


class _AsIfOnDevice(torch.Tensor):
    """ema_multi refuses a host fd_ema_state; nothing is launched in this file."""
    is_cuda = property(lambda self: True)


def test_item_tables_are_filled_as_the_compiler_lays_them_out(cc_says, monkeypatch):
    """One row of each host table, as the operator itself builds it (the library call is caught and the table's bytes read there)."""
    seen = {}

    def caught(dev, fn, label, table, n, *rest):
        seen[fn] = ct.string_at(table, n * cc_says["sizeof"][{"fd_adamw_multi": "fd_adamw_item", "fd_ema_multi": "fd_ema_item"}.get(fn, "fd_wn_item")])

    def row(name, **fields):
        return bytes(_packed(cc_says, name, torch.uint8, **fields).numpy().tobytes())

    monkeypatch.setattr(lvc_op, "_call", caught)
    p, g, m, v = (torch.zeros(6) for _ in range(4))
    lvc_op.adamw_multi([(p, g, m, v)], None, lvc_op.new_train_state("cpu"))
    assert seen["fd_adamw_multi"] == row("fd_adamw_item", p=("Q", p.data_ptr()), g=("Q", g.data_ptr()), m=("Q", m.data_ptr()), v=("Q", v.data_ptr()),
                                         numel=("q", 6))
    e = torch.zeros(6)
    lvc_op.ema_multi([(p, e)], lvc_op.pack_state("fd_ema_hyper", torch.float64), lvc_op.new_train_state("cpu"),
                     lvc_op.new_ema_state("cpu").as_subclass(_AsIfOnDevice))
    assert seen["fd_ema_multi"] == row("fd_ema_item", p=("Q", p.data_ptr()), e=("Q", e.data_ptr()), numel=("q", 6))
    wv, wg = torch.ones(3, 5, 2, requires_grad=True), torch.ones(3, 1, 1, requires_grad=True)
    (w,) = lvc_op._WeightNormAll.apply(wv, wg)
    fwd = seen["fd_weight_norm_multi_forward"]
    w_at, norm_at = (struct.unpack_from("<Q", fwd, cc_says["offsetof"]["fd_wn_item", f])[0] for f in ("w", "norm"))
    assert w_at == w.data_ptr()
    assert fwd == row("fd_wn_item", v=("Q", wv.data_ptr()), g=("Q", wg.data_ptr()), w=("Q", w_at), norm=("Q", norm_at), rows=("q", 3), cols=("i", 10))
    dw = torch.ones_like(w)
    w.backward(dw)
    bwd = seen["fd_weight_norm_multi_backward"]
    dw_at, dv_at, dg_at = (struct.unpack_from("<Q", bwd, cc_says["offsetof"]["fd_wn_item", f])[0] for f in ("dw", "dv", "dg"))
    assert dw_at and dv_at and dg_at and len({w_at, norm_at, dw_at, dv_at, dg_at}) == 5
    assert bwd == row("fd_wn_item", v=("Q", wv.data_ptr()), g=("Q", wg.data_ptr()), w=("Q", w_at), norm=("Q", norm_at), dw=("Q", dw_at),
                      dv=("Q", dv_at), dg=("Q", dg_at), rows=("q", 3), cols=("i", 10))


def test_the_tools_name_what_the_binding_has():
    tools = os.path.join(ROOT, "tools")
    named = {m for f in os.listdir(tools) if f.endswith(".py") for m in re.findall(r"\b_capi\.(\w+)", open(os.path.join(tools, f)).read())}
    assert {"check", "FdKernelStat"} <= named and not [m for m in named if not hasattr(_capi, m)]
