"""The registry of the guarded-memory suite (tests/test_guarded_memory.py) and what its cases share.  Not a test module.

A case builds its inputs from seeded host tensors with Guard.tensor, calls the public Python wrapper and returns the tensors the caller
gets back (outputs, gradients, records), with a mask where the header leaves a region unspecified.  The cases live in the modules of
CASE_MODULES, one per area, which define nothing but cases; this module imports them all at its end, so the registry is whole after
`import guarded_suite` whichever test file asked for it.  Shapes: the smallest at which the access pattern changes, taken from the border
tables of the operators' own tests.
"""
import importlib

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository and oracle/ on sys.path)
import guarded

DEV = "cuda"
CASES = {}          # id -> (function, {(entry point, argument index): reason}, {entry point: calls in the two guarded runs})
REPORTS = {}        # id -> guarded.Report of the cases that have run in this process
CASE_MODULES = ("guarded_cases_training", "guarded_cases_wave", "guarded_cases_inference", "guarded_cases_diversity", "guarded_cases_mcd",
                "guarded_cases_trim")


def case(name, declared=None, calls=None):
    """declared: the arguments that may lie outside guarded memory, each with its reason; calls: the entry points the case is there for,
    with the number of calls the two guarded runs must log."""
    def put(fn):
        assert name not in CASES, name
        CASES[name] = (fn, declared or {}, calls or {})
        return fn
    return put


def rnd(seed, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def leaf(g, t):
    return g.tensor(t).requires_grad_(True)


def grads(outs, inputs, gouts):
    return torch.autograd.grad(outs, inputs, gouts)


def as_tensors(record, prefix=""):
    return {prefix + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in record.items()}


_model = None


def model():
    """The inference module of the parity tests, made (and its weights uploaded) outside every guarded context: a case's plain run
    comes first."""
    global _model
    if _model is None:
        import gpu_common
        _model = gpu_common.make_model()
    return _model


_rows = None


def rows2():
    """A two-step schedule (the last two betas of the reference's N = 4 list)."""
    global _rows
    if _rows is None:
        from fastdiff_amd import sampler, schedules
        _rows = sampler.InferenceSchedule(schedules.training_hyperparams(), torch.FloatTensor([2.5376e-02, 7.0414e-01]), verbose=False).rows()
    return _rows


def _wide(g, x, ld):
    """The rows x [N, D] (tensor or array) ld floats apart in a guarded buffer that ends with the last row's D floats, 4 bytes off its
    aligned start."""
    N, D = x.shape
    buf = g.empty(((N - 1) * ld + D,), torch.float32, 4)
    v = torch.as_strided(buf, (N, D), (ld, 1), buf.storage_offset())
    v.copy_(torch.as_tensor(np.ascontiguousarray(x)))
    return v


def _ragged(g, rows):
    """Waveforms of different lengths as one batch that ends with the LAST row's own samples: that row is the longest but one sample.
    -> (the flat buffer, L, the lengths)"""
    L = max(len(x) for x in rows[:-1])
    assert len(rows[-1]) == L - 1
    flat = g.empty((len(rows) * L - 1,), torch.float32)
    flat.fill_(0.0 if g.fill is None else g.fill)          # what lies behind a row's own samples is never read: the poisons would show
    for b, x in enumerate(rows):                           # (flat: a [B, L] view would reach one sample behind the buffer)
        if len(x):
            flat[b * L: b * L + len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    return flat, L, [len(x) for x in rows]


def _run(name):
    if name not in REPORTS:
        try:
            REPORTS[name] = guarded.run_case(CASES[name][0], torch.device(DEV, torch.cuda.current_device()))
        except RuntimeError as e:
            if "illegal memory access" in str(e) or "HIP error" in str(e):      # the device is gone for this process: start nothing more on it
                pytest.exit(f"{name}: {e}", returncode=3)
            raise
    return REPORTS[name]


for _m in CASE_MODULES:          # last: the case modules import the names above from this module
    importlib.import_module(_m)
