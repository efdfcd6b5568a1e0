"""Poisoned, guarded buffers for the memory contract under the arithmetic.

Two conventions carry every ``torch.empty`` of the product code and no arithmetic test sees either of them:
outputs are fully written, and workspaces are never read before they are written.  The caching allocator hides a
violation (a freed block comes back with the previous, correct, answer), so this module takes the allocation
functions away for the length of a ``with`` block:

``poisoned(float_fill, int_fill)`` replaces ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
``torch.Tensor.new_empty`` (and wraps ``torch.zeros`` / ``torch.full``).  Every tensor they hand out is the middle of
a flat byte buffer ``guard | interior (rounded up to 256 bytes) | guard``: the interior is filled with the poison, the
guards (the rounding slack belongs to the back guard) with a fixed byte pattern, and base, view and the caller's
``file:line`` inside ``deadtrees_amd`` are recorded.  ``check_guards()`` compares every guard byte for byte and names
the allocation site of any that changed; the block calls it on the way out.

Poison shows as a wrong VALUE, never as a wild address: floating tensors get NaN in one run and the finite sentinel
``SENTINEL`` in another, integer and bool tensors the element values 0 and 1 in their own dtype, and a ``uint8``
buffer that a kernel reads as wider integers (named by ``wide_u8``) 0 or 1 per 8-byte word.  The guards of floating
buffers read as NaN in bf16, fp32 and fp64; those of integer buffers hold 1 per 8-byte word where the poison is 0 and
zeros where it is 1, so a stray integer store of either value changes one of the two runs.

What this does NOT see: an out-of-bounds write farther than ``guard_bytes`` from the buffer, a read past an input
that reaches no result, and anything under HIP-graph capture (an allocation while the stream captures raises).

``run_three`` is the comparison every case goes through: plain, ``poisoned(NaN, 0)``, ``poisoned(SENTINEL, 1)``, on
identical ``guarded`` inputs; every returned tensor must be ``same_bytes`` across the three runs, no floating result
may hold a NaN (the guards of the inputs are NaN: a read past an input that reaches a result shows there), and no
guard may have changed.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "deadtrees_amd") + os.sep
SENTINEL = 1.0e30
NAN = float("nan")
ALIGN = 256

# allocation sites reached under ``poisoned`` since import: "relative/path.py:line" -> count (the coverage test reads it)
reached: dict = {}
# guarded buffers handed out since import (inputs included)
stats = {"buffers": 0, "bytes": 0}


class GuardError(AssertionError):
    """a guard changed: something wrote outside the buffer it was given"""


class PoisonError(AssertionError):
    """results differ between plain and poisoned memory, or hold a NaN that only a guard or a poison can have put there"""


_FLOAT_GUARD = (0xC0, 0x7F)                       # bf16 0x7FC0, fp32 0x7FC07FC0, fp64 0x7FC07FC07FC07FC0: NaN in each
_WORD_ONE = (1, 0, 0, 0, 0, 0, 0, 0)
_pattern_cache: dict = {}


def _pattern(kind: str, n: int, device) -> torch.Tensor:
    """n guard bytes of ``kind`` ("float", "one" = 1 per 8-byte word, "zero") on ``device``; cached, never written"""
    key = (kind, n, str(device))
    t = _pattern_cache.get(key)
    if t is None:
        unit = {"float": _FLOAT_GUARD, "one": _WORD_ONE, "zero": (0,)}[kind]
        t = torch.tensor(unit, dtype=torch.uint8).repeat(-(-n // len(unit)))[:n].to(device)
        _pattern_cache[key] = t
    return t


def _is_float(dtype) -> bool:
    return dtype.is_floating_point or dtype.is_complex


def _site(depth: int = 2) -> str:
    """the innermost caller inside deadtrees_amd as "path:line" relative to the repository; without one, the caller of
    the allocation function itself"""
    f = sys._getframe(depth)
    first = f
    while f is not None:
        name = f.f_code.co_filename
        if os.path.abspath(name).startswith(PACKAGE):
            return f"{os.path.relpath(os.path.abspath(name), ROOT)}:{f.f_lineno}"
        f = f.f_back
    return f"{os.path.relpath(os.path.abspath(first.f_code.co_filename), ROOT)}:{first.f_lineno}"


class _Record:
    __slots__ = ("base", "front", "back", "kind", "site", "view", "is_input")

    def __init__(self, base, front, back, kind, site, view):
        self.base, self.front, self.back, self.kind, self.site, self.view = base, front, back, kind, site, view
        self.is_input = False

    def holds(self, t: torch.Tensor) -> bool:
        lo = self.base.data_ptr()
        return t.numel() > 0 and t.device == self.base.device and lo <= t.data_ptr() < lo + self.base.numel()


class _State:
    def __init__(self, float_fill, int_fill, guard_bytes, wide_u8):
        if int_fill not in (0, 1):
            raise ValueError("integer poison is the element value 0 or 1, never a byte pattern")
        if guard_bytes <= 0 or guard_bytes % ALIGN:
            raise ValueError(f"guard_bytes must be a positive multiple of {ALIGN}")
        self.float_fill, self.int_fill, self.guard, self.wide_u8 = float_fill, int_fill, guard_bytes, tuple(wide_u8)
        self.records = []
        self.orig = {}


_active: list = []          # the stack of open ``poisoned`` blocks (one in practice)
_input_records: list = []   # guards of ``guarded`` inputs made outside a block; checked and dropped by run_three


def _raw_empty(*a, **k):
    return (_active[-1].orig["empty"] if _active else torch.empty)(*a, **k)


def _carve(nbytes: int, dtype, device, guard: int, kind: str, site: str):
    """-> (flat view of ``nbytes`` bytes as ``dtype`` at a 256-byte aligned address, record)"""
    device = torch.device(device if device is not None else "cpu")
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"poison: allocation at {site} while a HIP graph is captured; capture is out of scope")
    room = -(-nbytes // ALIGN) * ALIGN
    base = _raw_empty(guard + room + guard + ALIGN, dtype=torch.uint8, device=device)
    off = (-base.data_ptr()) % ALIGN
    lo, hi = off + guard, off + guard + nbytes
    front, back = base[off:lo], base[hi:off + guard + room + guard]
    front.copy_(_pattern(kind, front.numel(), device))
    back.copy_(_pattern(kind, back.numel(), device))
    flat = base[lo:hi].view(dtype) if nbytes else _raw_empty(0, dtype=dtype, device=device)
    rec = _Record(base, front, back, kind, site, flat)
    stats["buffers"] += 1
    stats["bytes"] += nbytes
    return flat, rec


def _fill(flat: torch.Tensor, state: _State, site_fn: str):
    """poison the interior: floats the fill value, integers the element value int_fill written through the bytes (works
    for every integer dtype), a wide-read uint8 workspace int_fill per 8-byte word"""
    if flat.numel() == 0:
        return
    if _is_float(flat.dtype):
        flat.fill_(state.float_fill)
        return
    raw = flat.view(torch.uint8)
    raw.zero_()
    if state.int_fill:
        k = flat.element_size()
        if flat.dtype == torch.uint8 and any(name in site_fn for name in state.wide_u8):
            k = 8
        raw[::k] = 1                                   # little endian: the low byte of every element / word


def _guard_kind(dtype, state: _State = None) -> str:
    if _is_float(dtype):
        return "float"
    if state is None:
        return "zero"                                  # an integer input: guards of 0
    return "zero" if state.int_fill else "one"


def _numel(size) -> int:
    n = 1
    for s in size:
        n *= int(s)
    return n


def _size_of(args):
    if len(args) == 1 and not isinstance(args[0], (int, torch.SymInt)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


_PLAIN_KW = {"dtype", "device", "requires_grad", "memory_format", "layout", "pin_memory"}


def _plain(kw) -> bool:
    """keyword arguments the guarded path reproduces (anything else goes to the original function, unguarded)"""
    return (set(kw) <= _PLAIN_KW and not kw.get("pin_memory") and not kw.get("requires_grad")
            and kw.get("layout", torch.strided) is torch.strided
            and kw.get("memory_format", torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format))


def _alloc(state: _State, size, dtype, device, site, site_fn, poison=True, strides=None):
    dtype = dtype if dtype is not None else torch.get_default_dtype()
    item = torch.tensor([], dtype=dtype).element_size()
    if strides is None:
        elems = _numel(size)
    else:
        elems = 0 if _numel(size) == 0 else 1 + sum((int(s) - 1) * int(st) for s, st in zip(size, strides))
    flat, rec = _carve(elems * item, dtype, device, state.guard, _guard_kind(dtype, state), site)
    state.records.append(rec)
    reached[site] = reached.get(site, 0) + 1
    if poison:
        _fill(flat, state, site_fn)
    return flat.view(size) if strides is None else flat.as_strided(size, strides)


def _caller_fn(depth: int = 2) -> str:
    """names of the functions on the stack above the allocation (for ``wide_u8``), innermost first, joined"""
    f, names = sys._getframe(depth), []
    while f is not None and len(names) < 16:
        names.append(f.f_code.co_name)
        f = f.f_back
    return " ".join(names)


def _install(state: _State):
    o = state.orig
    o["empty"], o["empty_like"], o["empty_strided"] = torch.empty, torch.empty_like, torch.empty_strided
    o["zeros"], o["full"] = torch.zeros, torch.full
    o["new_empty"] = torch.Tensor.__dict__.get("new_empty")            # None: inherited from the C base class
    o["new_empty_fn"] = torch.Tensor.new_empty

    def empty(*args, **kw):
        if not _plain(kw) or kw.get("out") is not None:
            return o["empty"](*args, **kw)
        return _alloc(state, _size_of(args), kw.get("dtype"), kw.get("device"), _site(), _caller_fn())

    def empty_like(t, **kw):
        if not _plain(kw):
            return o["empty_like"](t, **kw)
        return _alloc(state, tuple(t.shape), kw.get("dtype") or t.dtype, kw.get("device") or t.device, _site(), _caller_fn())

    def empty_strided(size, stride, **kw):
        if not _plain(kw):
            return o["empty_strided"](size, stride, **kw)
        return _alloc(state, tuple(size), kw.get("dtype"), kw.get("device"), _site(), _caller_fn(),
                      strides=tuple(int(s) for s in stride))

    def new_empty(self, *args, **kw):
        if not _plain(kw):
            return o["new_empty_fn"](self, *args, **kw)
        return _alloc(state, _size_of(args), kw.get("dtype") or self.dtype, kw.get("device") or self.device, _site(),
                      _caller_fn())

    def zeros(*args, **kw):
        if not _plain(kw) or kw.get("out") is not None:
            return o["zeros"](*args, **kw)
        return _alloc(state, _size_of(args), kw.get("dtype"), kw.get("device"), _site(), "", poison=False).zero_()

    def full(size, fill_value, **kw):
        if not _plain(kw) or kw.get("out") is not None:
            return o["full"](size, fill_value, **kw)
        dtype = kw.get("dtype")
        if dtype is None:
            dtype = o["full"]((), fill_value).dtype
        return _alloc(state, tuple(size), dtype, kw.get("device"), _site(), "", poison=False).fill_(fill_value)

    torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
    torch.zeros, torch.full = zeros, full
    torch.Tensor.new_empty = new_empty


def _remove(state: _State):
    o = state.orig
    torch.empty, torch.empty_like, torch.empty_strided = o["empty"], o["empty_like"], o["empty_strided"]
    torch.zeros, torch.full = o["zeros"], o["full"]
    if o["new_empty"] is None:
        del torch.Tensor.new_empty
    else:
        torch.Tensor.new_empty = o["new_empty"]


def _check(records) -> None:
    bad = []
    for r in records:
        for side, g in (("before", r.front), ("behind", r.back)):
            want = _pattern(r.kind, g.numel(), g.device)
            if not torch.equal(g, want):
                where = torch.nonzero(g != want).view(-1)
                first = int(where[0]) if side == "behind" else int(g.numel() - 1 - where[-1])
                bad.append(f"{r.site}: {int(where.numel())} guard byte(s) changed {side} the buffer "
                           f"({r.view.numel()} x {r.view.dtype}), the nearest {first} byte(s) away")
    if bad:
        raise GuardError("write outside an allocation:\n  " + "\n  ".join(bad))


def check_guards() -> None:
    """every guard of the open ``poisoned`` block and of the ``guarded`` inputs, byte for byte; GuardError names the
    allocation site of each that changed"""
    if any(r.base.is_cuda for s in _active for r in s.records) or any(r.base.is_cuda for r in _input_records):
        torch.cuda.synchronize()
    _check([r for s in _active for r in s.records] + _input_records)


@contextlib.contextmanager
def poisoned(float_fill, int_fill, guard_bytes: int = 4096, wide_u8=()):
    """see the module docstring.  ``wide_u8``: names of functions (anywhere on the stack of the allocation) whose ``uint8`` allocations a kernel
    reads as wider integers.  Yields the block's state (``.records``); the guards are checked on a clean way out, the
    four functions are restored on every way out"""
    if _active:
        raise RuntimeError("poisoned blocks do not nest")
    state = _State(float_fill, int_fill, guard_bytes, wide_u8)
    _install(state)
    _active.append(state)
    try:
        yield state
        check_guards()
    finally:
        _active.pop()
        _remove(state)
        state.records.clear()


def guarded(t: torch.Tensor, guard_bytes: int = 4096, site: str = None) -> torch.Tensor:
    """a copy of the input ``t`` (contiguous, same shape, dtype and device) in guarded storage: NaN guards around a
    floating tensor, zeros around an integer one.  A read past it that reaches a result turns that result into NaN;
    a write past it is what ``check_guards`` reports, under ``site`` (default: the line that called ``guarded``;
    ``run_three`` passes the line that called it, with the input's position)"""
    if t is None:
        return None
    flat, rec = _carve(t.numel() * t.element_size(), t.dtype, t.device, guard_bytes, _guard_kind(t.dtype), site or _site())
    rec.is_input = True
    (_active[-1].records if _active else _input_records).append(rec)
    out = flat.view(t.shape)
    out.copy_(t)
    return out


def release_inputs() -> None:
    """forget the guards of the ``guarded`` inputs made outside a block (after they were checked)"""
    _input_records.clear()


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equality of the bytes: NaN equals NaN, -0.0 differs from 0.0"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def flatten(out, path="out"):
    """(path, tensor) of every tensor / array / number in a nested result; None is skipped"""
    if out is None:
        return
    if isinstance(out, torch.Tensor):
        yield path, out.detach()
    elif isinstance(out, np.ndarray):
        yield path, torch.from_numpy(np.array(out))          # a copy: host results may be read-only
    elif isinstance(out, (bool, int, float, np.generic)):
        yield path, torch.tensor(out)
    elif isinstance(out, (str, bytes)):
        return
    elif isinstance(out, dict):
        for k in out:
            yield from flatten(out[k], f"{path}[{k!r}]")
    elif hasattr(out, "_fields"):
        for k in out._fields:
            yield from flatten(getattr(out, k), f"{path}.{k}")
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            yield from flatten(v, f"{path}[{i}]")
    elif hasattr(out, "__dict__"):
        for k, v in vars(out).items():
            yield from flatten(v, f"{path}.{k}")
    else:
        raise TypeError(f"{path}: cannot compare a {type(out).__name__}")


def _first_difference(a, b) -> str:
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    a, b = a.contiguous().view(-1).cpu(), b.contiguous().view(-1).cpu()
    ne = (a.view(torch.uint8).view(a.numel(), -1) != b.view(torch.uint8).view(b.numel(), -1)).any(1)
    idx = torch.nonzero(ne).view(-1)
    i = int(idx[0])
    return f"{int(idx.numel())} of {a.numel()} elements, first at flat index {i}: {a[i].item()!r} against {b[i].item()!r}"


RUNS = (("plain", None), ("poisoned(nan, 0)", (NAN, 0)), ("poisoned(1e30, 1)", (SENTINEL, 1)))


def run_three(make_inputs, call, cut=None, wide_u8=(), guard_bytes: int = 4096, nan_ok: bool = False, ref=None):
    """the three-run comparison.  ``make_inputs()`` -> a tuple / dict of inputs, built once; every run gets its own
    ``guarded`` copies (so tensors the op writes in place start from the same bytes each time).  ``call(*inputs)`` (or
    ``call(**inputs)``) -> the result; tensors of the inputs the op may have written can be returned with it.  ``cut``
    maps a result to the part that is defined (a table with fewer live rows than capacity).  Raises PoisonError /
    GuardError; returns the plain run's flattened result [(path, tensor)].  ``ref(inputs, {path: tensor})``, when given, is
    called once with the inputs as built and the plain run's result: the place for a comparison with a reference."""
    inputs = make_inputs()
    caller = _site()
    names = []
    results, owners, sites = [], {}, set()
    for name, fills in RUNS:
        def copies(v, path="input"):
            if isinstance(v, torch.Tensor):
                names.append(f"{path} ({v.numel()} x {v.dtype})")
                return guarded(v, guard_bytes, site=f"{caller} [{path}]")
            if isinstance(v, (tuple, list)):
                return type(v)(copies(x, f"{path}[{i}]") for i, x in enumerate(v))
            if isinstance(v, dict):
                return {k: copies(x, f"{path}[{k!r}]") for k, x in v.items()}
            return v
        try:
            if fills is None:
                args = copies(inputs)
                out = call(**args) if isinstance(args, dict) else call(*args)
                check_guards()
            else:
                with poisoned(fills[0], fills[1], guard_bytes, wide_u8) as state:
                    args = copies(inputs)
                    out = call(**args) if isinstance(args, dict) else call(*args)
                    out = list(flatten(cut(out) if cut is not None else out))
                    fresh = [r for r in state.records if not r.is_input]
                    owners.update({p: r.site for p, t in out for r in fresh if r.holds(t)})
                    sites.update(r.site for r in fresh)
                    out = [(p, t.clone()) for p, t in out]
            if fills is None:
                out = [(p, t.clone()) for p, t in flatten(cut(out) if cut is not None else out)]
        except GuardError as e:
            raise GuardError(f"{name}: {e}") from None
        finally:
            release_inputs()
        results.append((name, out))
    plain = results[0][1]
    for name, out in results[1:]:
        if [p for p, _ in out] != [p for p, _ in plain]:
            raise PoisonError(f"{name}: result structure {[p for p, _ in out]} against plain {[p for p, _ in plain]}")
        for (p, a), (_, b) in zip(plain, out):
            if not same_bytes(a, b):
                raise PoisonError(f"{p}: plain against {name}: {_first_difference(a, b)} — an output element that is "
                                  "never written, or a workspace read before it is written; the result was allocated at "
                                  f"{owners.get(p, 'a place outside the block')}, the allocations of the run: "
                                  f"{', '.join(sorted(sites))}")
    if not nan_ok:
        for p, a in plain:
            if _is_float(a.dtype) and bool(torch.isnan(a).any()):
                raise PoisonError(f"{p}: NaN in the result of finite inputs: a read outside an input reached it; the inputs "
                                  f"were guarded at {caller}: {', '.join(sorted(set(names)))}")
    if ref is not None:
        ref(inputs, dict(plain))
    return plain
