"""Guarded memory for operator tests (a helper module like gpu_common.py, not a conftest).

`with guarded(fill, device) as g:` makes every tensor that a wrapper allocates on `device` with torch.empty / empty_like / zeros /
zeros_like / full, and every tensor the test copies in with g.tensor(t), a view into a larger block [pad | body | pad] that is filled
with a poison before the view is handed out.  Three properties of an operator can then be checked without a device sanitizer:

  (a) no guard byte changed: g.check() compares the pads (and the slack that rounds the body up to 512 bytes) byte by byte with
      the poison, so NaN hides nothing, and says where the first changed byte lies relative to the tensor's ends;
  (b) two runs with different poisons agree bit for bit: a load past the end of an input, an output element that is never
      written and a result that depends on what the output held all make them differ;
  (c) the guarded runs agree bit for bit with a plain run.

While the context is active the fd_* functions of the library object are wrapped as well: every device pointer that crosses ctypes
(a c_void_p argument that is a non-zero int, every element of a (c_void_p * n) array, every c_void_p field of an array of
structures, and the pointer columns of the host tables in HOST_TABLES) must lie inside a guarded body; the others are recorded and
g.unguarded() returns them, so an operator cannot escape the check by allocating some other way (x.clone(), x.new_empty(...)).
The handle (first argument) and the stream (last argument) are not looked at.  g.calls counts the calls per function.

The pad is 1024 bytes: a multiple of the caching allocator's 512-byte granule, so a guarded tensor starts with the alignment of a
plain allocation and the kernels take the same code path; it is also what one wavefront of 64 lanes moves with 16-byte accesses.
Poison: floating types get `fill` (nan, or -12345.678, the canary of test_param_ema.py); integer and byte types get the byte
0x5A for a nan fill and 0xA5 otherwise.  check() synchronises the device once; nothing else is added to the stream.
"""
import contextlib
import ctypes as ct
import math
from collections import Counter

import torch

from fastdiff_amd import _capi

PAD = 1024
GRANULE = 512
FILLS = (float("nan"), -12345.678)

# host tables of structures whose columns hold device pointers: function -> (index of the table argument, index of the count argument,
# 8-byte words per item, the pointer columns): the words and columns are those of the item structure as the header declares it


def _host_table(item, at, n_at, looked=None):
    """looked: the pointer fields the call reads or writes (None: all of them)."""
    rec = _capi.record(item)
    pointers = [name for name, typ in _capi.struct(item)._fields_ if typ is ct.c_void_p]
    assert rec.itemsize % 8 == 0 and set(looked or ()) <= set(pointers)
    return at, n_at, rec.itemsize // 8, tuple(rec.fields[name][1] // 8 for name in pointers if looked is None or name in looked)


HOST_TABLES = {
    "fd_adamw_multi": _host_table("fd_adamw_item", 1, 2),
    "fd_ema_multi": _host_table("fd_ema_item", 1, 2),
    "fd_weight_norm_multi_forward": _host_table("fd_wn_item", 1, 2, ("v", "g", "w", "norm")),
    "fd_weight_norm_multi_backward": _host_table("fd_wn_item", 1, 2),
}

_FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
_INTS = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
_PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "full")


def _itemsize(dtype):
    return (torch.finfo(dtype) if dtype.is_floating_point else torch.iinfo(dtype)).bits // 8


class _Unmodelled(Exception):
    """A call the replacements do not model: it goes to the original."""


class _Block:
    def __init__(self, buf, first, numel, view):
        self.buf, self.first, self.numel, self.view = buf, first, numel, view
        isz = buf.element_size()
        self.lo = buf.data_ptr() + first * isz          # the body: [lo, hi)
        self.hi = self.lo + numel * isz


class Guard:
    def __init__(self, fill, device, originals):
        self.fill = float(fill)
        self.byte = 0x5A if math.isnan(self.fill) else 0xA5
        self.device = torch.device(device)
        self._orig = originals
        self.blocks = []
        self.calls = Counter()
        self._unguarded = []

    # ---- allocation -------------------------------------------------------------------------------------------------------------
    def _matches(self, device):
        d = torch.device("cpu") if device is None else torch.device(device)
        if d.type != self.device.type:
            return False
        if d.type == "cpu":
            return True
        cur = torch.cuda.current_device()
        return (cur if d.index is None else d.index) == (cur if self.device.index is None else self.device.index)

    def _poison(self, n, dtype):
        if dtype in _FLOATS:
            return self._orig["full"]((n,), self.fill, dtype=dtype, device=self.device)
        isz = _itemsize(dtype)
        return self._orig["full"]((n * isz,), self.byte, dtype=torch.uint8, device=self.device).view(dtype)

    def empty(self, shape, dtype=torch.float32, offset_bytes=0):
        """A poisoned tensor of `shape` inside a block of its own.  offset_bytes (a multiple of the element size): how far behind the
        aligned position the tensor starts, for the entry points whose header promises any alignment."""
        if dtype not in _FLOATS + _INTS:
            raise _Unmodelled(dtype)
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        if numel == 0:
            raise _Unmodelled("empty tensor")
        isz = _itemsize(dtype)
        assert offset_bytes % isz == 0 and 0 <= offset_bytes < GRANULE
        body = -(-(numel * isz + offset_bytes) // GRANULE) * GRANULE
        buf = self._poison((2 * PAD + body) // isz, dtype)
        first = (PAD + offset_bytes) // isz
        view = buf[first: first + numel].view(shape)
        self.blocks.append(_Block(buf, first, numel, view))
        return view

    def tensor(self, t, offset_bytes=0):
        """A copy of the host or device tensor `t` in guarded memory (contiguous)."""
        out = self.empty(t.shape, t.dtype, offset_bytes)
        out.copy_(t.detach())
        return out

    # ---- the checks -------------------------------------------------------------------------------------------------------------
    def check(self):
        """[(block index, shape, where)] for every block with a changed guard byte; where = ("behind", k): the first changed byte is
        byte k behind the tensor's end (k >= 0), or ("front", k): the changed byte nearest to the tensor is k bytes in front of its
        start (k >= 1).  An empty list: no guard byte changed.  One device synchronisation."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        bad = []
        for i, b in enumerate(self.blocks):
            isz = b.buf.element_size()
            got = b.buf.view(torch.uint8)
            want = self._poison(1, b.buf.dtype).view(torch.uint8).repeat(b.buf.numel())
            diff = got != want
            lo, hi = b.first * isz, (b.first + b.numel) * isz
            front, behind = diff[:lo], diff[hi:]
            if bool(behind.any()):
                bad.append((i, tuple(b.view.shape), ("behind", int(behind.nonzero()[0]))))
            if bool(front.any()):
                bad.append((i, tuple(b.view.shape), ("front", lo - int(front.nonzero()[-1]))))
        return bad

    def unguarded(self):
        """The (function, argument index) pairs whose address lay outside every guarded body, each once, in call order."""
        seen, out = set(), []
        for k in self._unguarded:
            if k not in seen:
                seen.add(k)
                out.append(k)
        return out

    def _inside(self, addr):
        return any(b.lo <= addr < b.hi for b in self.blocks)

    def _look(self, fn, i, addr):
        if addr and not self._inside(int(addr)):
            self._unguarded.append((fn, i))

    def _inspect(self, fn, argtypes, args):
        self.calls[fn] += 1
        last = len(args) - 1
        for i, a in enumerate(args):
            if i == 0 or i == last:
                continue
            if isinstance(a, ct.Array):
                if a._type_ is ct.c_void_p:
                    for v in a:
                        self._look(fn, i, v)
                elif issubclass(a._type_, ct.Structure):
                    for item in a:
                        for name, typ in item._fields_:
                            if typ is ct.c_void_p:
                                self._look(fn, i, getattr(item, name))
                continue
            if i < len(argtypes) and argtypes[i] is ct.c_void_p and isinstance(a, int) and not isinstance(a, bool) and a != 0:
                table = HOST_TABLES.get(fn)
                if table is not None and table[0] == i:
                    _, n_at, words, cols = table
                    raw = (ct.c_int64 * (int(args[n_at]) * words)).from_address(a)
                    for r in range(int(args[n_at])):
                        for c in cols:
                            self._look(fn, i, raw[r * words + c] & 0xFFFFFFFFFFFFFFFF)
                else:
                    self._look(fn, i, a)


class _Wrapped:
    """An fd_* function with the guard looking at its arguments first."""

    def __init__(self, name, fn, guard):
        self._name, self._fn, self._guard = name, fn, guard

    def __call__(self, *args):
        self._guard._inspect(self._name, self._fn.argtypes or (), args)
        return self._fn(*args)

    def __getattr__(self, k):
        return getattr(self._fn, k)


def _replacements(g, orig):
    def plain(kw, allowed=("dtype", "device")):
        if any(k not in allowed for k in kw) or kw.get("dtype", torch.float32) is None:
            raise _Unmodelled(kw)

    def size_of(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if not all(isinstance(s, int) and not isinstance(s, bool) for s in size):
            raise _Unmodelled(size)
        return size

    def new(size, kw):
        plain(kw)
        if not g._matches(kw.get("device")):
            raise _Unmodelled("another device")
        return g.empty(size_of(size), kw.get("dtype", torch.get_default_dtype()))

    def like(x, kw):
        plain(kw)
        if not isinstance(x, torch.Tensor) or not x.is_contiguous() or not g._matches(kw.get("device", x.device)):
            raise _Unmodelled("another device or layout")
        return g.empty(x.shape, kw.get("dtype", x.dtype))

    def empty(*size, **kw):
        try:
            return new(size, kw)
        except _Unmodelled:
            return orig["empty"](*size, **kw)

    def zeros(*size, **kw):
        try:
            return new(size, kw).zero_()
        except _Unmodelled:
            return orig["zeros"](*size, **kw)

    def empty_like(x, **kw):
        try:
            return like(x, kw)
        except _Unmodelled:
            return orig["empty_like"](x, **kw)

    def zeros_like(x, **kw):
        try:
            return like(x, kw).zero_()
        except _Unmodelled:
            return orig["zeros_like"](x, **kw)

    def full(size, value, **kw):
        try:
            if not isinstance(value, (int, float)) or isinstance(value, bool) or "dtype" not in kw:
                raise _Unmodelled(value)
            return new((size,), kw).fill_(value)
        except _Unmodelled:
            return orig["full"](size, value, **kw)

    return {"empty": empty, "empty_like": empty_like, "zeros": zeros, "zeros_like": zeros_like, "full": full}


@contextlib.contextmanager
def guarded(fill, device, lib=None):
    """The context of the module's text.  lib: the library object whose fd_* functions are wrapped (default: the one
    fastdiff_amd._capi.load() returns, when its file exists; a test may pass a fake object carrying functions with `argtypes`)."""
    if lib is None:
        from fastdiff_amd import _capi
        import os
        lib = _capi.load() if os.path.exists(_capi.LIB_PATH) else None
    orig = {k: getattr(torch, k) for k in _PATCHED}
    g = Guard(fill, device, orig)
    wrapped = {}
    if lib is not None:
        for name, fn in list(vars(lib).items()):
            if name.startswith("fd_") and callable(fn) and getattr(fn, "argtypes", None) is not None:
                wrapped[name] = fn
    try:
        for k, f in _replacements(g, orig).items():
            setattr(torch, k, f)
        for name, fn in wrapped.items():
            setattr(lib, name, _Wrapped(name, fn, g))
        yield g
    finally:
        for k, f in orig.items():
            setattr(torch, k, f)
        for name, fn in wrapped.items():
            setattr(lib, name, fn)


class Plain:
    """What a case gets for its plain run: Guard's allocation interface on ordinary tensors."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.fill = None

    def tensor(self, t, offset_bytes=0):
        return t.detach().to(self.device).clone()

    def empty(self, shape, dtype=torch.float32, offset_bytes=0):
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)


class Report:
    """What run_case found: guard = [(fill, block, shape, where)], poison = [(name, differing elements, first index)] between the two
    guarded runs, plain = the same between the first guarded run and the plain one, unguarded = [(function, argument index)],
    calls = Counter of the library functions the guarded runs called."""

    def __init__(self):
        self.guard, self.poison, self.plain, self.unguarded, self.calls = [], [], [], [], Counter()

    def clean(self):
        return not (self.guard or self.poison or self.plain or self.unguarded)


def _snapshot(ret):
    outs, masks = ret if isinstance(ret, tuple) else (ret, {})
    assert outs and all(isinstance(t, torch.Tensor) for t in outs.values()), "a case returns a dict of the tensors the caller gets back"
    return {k: t.detach().cpu().clone() for k, t in outs.items()}, {k: m.detach().cpu().clone() for k, m in (masks or {}).items()}


def run_case(fn, device, lib=None):
    """Run the case `fn(guard) -> {name: tensor}` or `({name: tensor}, {name: mask of the specified elements})` three times -- plain, and
    guarded with each of FILLS -- and report on the three properties and the pointer coverage (the module's text)."""
    rep = Report()
    plain, masks = _snapshot(fn(Plain(device)))
    runs = []
    for fill in FILLS:
        with guarded(fill, device, lib) as g:
            ret = fn(g)
            rep.guard += [(fill,) + bad for bad in g.check()]
        runs.append(_snapshot(ret)[0])
        rep.unguarded += [k for k in g.unguarded() if k not in rep.unguarded]
        rep.calls.update(g.calls)
    for name in plain:
        mask = masks.get(name)
        for other, found in ((runs[1], rep.poison), (plain, rep.plain)):
            a, b = runs[0][name], other[name]
            if a.shape != b.shape or a.dtype != b.dtype:
                found.append((name, "shape or type", None))
                continue
            n, first = first_difference(a, b, mask)
            if n:
                found.append((name, n, first))
    return rep


def first_difference(a, b, mask=None):
    """(count, index of the first) of the elements whose bytes differ, inside `mask` where one is given; (0, None): none."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    isz = a.element_size()
    d = (a.reshape(-1).view(torch.uint8).view(-1, isz) != b.reshape(-1).view(torch.uint8).view(-1, isz)).any(1)
    if mask is not None:
        d &= mask.detach().cpu().reshape(-1).bool()
    n = int(d.sum())
    return n, (int(d.nonzero()[0]) if n else None)
