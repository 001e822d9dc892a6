"""Guarded allocator for the Python binding: where did a kernel write, and what did it read?  (plain helper module, like conv_shapes.py)

The parity tests ask whether a number is right.  They cannot see a kernel that writes past the buffer a size query promised (the
stray bytes land in memory torch's caching allocator happens to own) or one that leaves a ragged tail of its output unwritten / reads
a workspace slot before writing it (a `torch.empty` block usually still holds the previous, correct result of the same shape).  The
GPU address sanitizer is not available on the shared MI355X machines, so the check lives here:

  Arena        hands out tensors from flat uint8 blocks [guard | payload | guard]: guards hold a canary byte, `empty` payloads a poison
               byte (0xFF: NaN in bf16 / fp32, -1 in int32; 0x7F: 3.39e38 in bf16 / fp32, 0x7F7F7F7F in int32), `zeros` payloads zero.
  guarded()    replaces the name `torch` inside cd360.ops / cd360.nerf / cd360.grad with a proxy whose empty / empty_like / zeros /
               zeros_like allocate from the arena, and cd360._lib.load() with a recorder of the cd360_* entry points called.
  run_twice()  runs a callable under both poisons and asserts
                 P1  no guard byte changed (no stray write),
                 P2  every result is bit-equal between the two runs and finite in the first (fully written, nothing uninitialised read),
                 P3  every operand is bit-equal to its clone from before the call (read-only), named in/out arguments excepted,
                 P4  every entry point the case declares was called.
No tolerance anywhere: canary equality and bit equality only.  Not for use under hipGraph capture (allocations there happen once, before
the capture; the same kernels are covered eagerly)."""
from __future__ import annotations

import contextlib
import os
import sys
import types

import torch

GUARD_MIN, GUARD_MAX, ALIGN = 4096, 1 << 20, 256
POISONS = (0xFF, 0x7F)
MODULES = ("cd360.ops", "cd360.nerf", "cd360.grad")
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


def guard_bytes(nbytes: int) -> int:
    """Each guard: the payload rounded up to 256 bytes, at least 4 KiB, at most 1 MiB -- a write of up to twice the promised size lands
    in a guard for every payload up to 1 MiB."""
    return min(max(GUARD_MIN, (nbytes + ALIGN - 1) // ALIGN * ALIGN), GUARD_MAX)


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} in {f.f_code.co_name}"


class _Block:
    __slots__ = ("raw", "front", "nbytes", "site", "shape", "dtype", "kind")

    def describe(self, index: int) -> str:
        return f"allocation #{index} ({self.kind}) at {self.site}, shape {tuple(self.shape)}, dtype {self.dtype}, {self.nbytes} bytes"


class Arena:
    def __init__(self, poison: int, canary: int = 0xA5):
        assert 0 <= poison < 256 and 0 <= canary < 256 and poison != canary
        self.poison, self.canary, self.blocks = poison, canary, []

    def alloc(self, shape, dtype, device, zero: bool = False, kind: str = "empty", strides=None) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        n = 1
        for s in shape:
            assert s >= 0
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        pad = guard_bytes(nbytes)
        raw = torch.full((pad + ALIGN + nbytes + pad,), self.canary, dtype=torch.uint8, device=device)
        front = pad + (-(raw.data_ptr() + pad)) % ALIGN  # payload start 256-byte aligned whatever the allocator returned
        pay = raw[front:front + nbytes]
        assert nbytes == 0 or pay.data_ptr() % ALIGN == 0
        pay.fill_(0 if zero else self.poison)
        blk = _Block()
        blk.raw, blk.front, blk.nbytes, blk.site, blk.shape, blk.dtype, blk.kind = raw, front, nbytes, _call_site(), shape, dtype, kind
        self.blocks.append(blk)
        t = pay.view(dtype)
        return t.view(shape) if strides is None else t.as_strided(shape, strides)

    def damage(self):
        """[(block index, block, side, first, last)]: first / last damaged byte as an offset from the payload's first byte (front guard:
        negative) or from the first byte behind the payload (back guard: >= 0)."""
        if any(b.raw.is_cuda for b in self.blocks):
            torch.cuda.synchronize()
        out = []
        for i, b in enumerate(self.blocks):
            for side, g, base in (("front", b.raw[:b.front], -b.front), ("back", b.raw[b.front + b.nbytes:], 0)):
                bad = g != self.canary
                if bool(bad.any()):
                    idx = bad.nonzero().flatten()
                    out.append((i, b, side, base + int(idx[0]), base + int(idx[-1])))
        return out

    def check(self) -> None:
        dmg = self.damage()
        if dmg:
            lines = [f"{b.describe(i)}: {side} guard damaged, bytes {first:+d} .. {last:+d} relative to the payload's "
                     f"{'start' if side == 'front' else 'end'}" for i, b, side, first, last in dmg]
            raise GuardError(f"P1 stray write (poison 0x{self.poison:02X}): " + "; ".join(lines))


def _is_cuda(device) -> bool:
    return device is not None and torch.device(device).type == "cuda"


def _size_args(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        return tuple(size[0])
    return tuple(size)


class TorchProxy(types.ModuleType):
    """Stands in for the module `torch` inside the binding: every attribute is torch's, except the allocation routes."""

    def __init__(self, arena: Arena):
        super().__init__("torch")
        self.__dict__["_arena"] = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _kw(kw, what):
        kw = dict(kw)
        dtype, device = kw.pop("dtype", None), kw.pop("device", None)
        if kw.pop("requires_grad", False) or kw.pop("pin_memory", False):
            raise NotImplementedError(f"guarded torch.{what}: requires_grad / pin_memory allocations are not modelled")
        if what.endswith("_like"):
            kw.pop("memory_format", None)  # honoured through the strides torch itself would choose (_like below)
        if kw:
            raise NotImplementedError(f"guarded torch.{what}: unexpected arguments {sorted(kw)}")
        return dtype, device

    def empty(self, *size, **kw):
        dtype, device = self._kw(kw, "empty")
        return self._arena.alloc(_size_args(size), dtype, device, zero=False, kind="empty")

    def zeros(self, *size, **kw):
        dtype, device = self._kw(kw, "zeros")
        return self._arena.alloc(_size_args(size), dtype, device, zero=True, kind="zeros")

    def _like(self, x, kw, what, zero):
        strides = torch.empty_like(x, device="meta", **{k: v for k, v in kw.items() if k != "device"}).stride()  # torch's own layout rule
        dtype, device = self._kw(kw, what)
        return self._arena.alloc(x.shape, x.dtype if dtype is None else dtype, x.device if device is None else device, zero=zero, kind=what,
                                 strides=strides)

    def empty_like(self, x, **kw):
        return self._like(x, kw, "empty_like", False)

    def zeros_like(self, x, **kw):
        return self._like(x, kw, "zeros_like", True)

    def _refuse(self, name, args, kw):
        if _is_cuda(kw.get("device")):
            raise GuardError(f"guarded torch.{name}(..., device={kw['device']!r}): an allocation route on the GPU that the arena does not "
                             "intercept -- use empty / empty_like / zeros / zeros_like, or teach tests/guarded.py the new route")
        return getattr(torch, name)(*args, **kw)

    def empty_strided(self, *a, **kw):
        return self._refuse("empty_strided", a, kw)

    def full(self, *a, **kw):
        return self._refuse("full", a, kw)

    def ones(self, *a, **kw):
        return self._refuse("ones", a, kw)


class Recorder:
    """The object cd360._lib.load() returns, noting which cd360_* symbols are called."""

    def __init__(self, lib):
        self.__dict__["_lib"], self.__dict__["called"] = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cd360_"):
            return fn
        called = self.called

        def call(*args):
            called.append(name)
            return fn(*args)
        return call


class Guard:
    def __init__(self, arena, torch_proxy, lib):
        self.arena, self.torch, self.lib = arena, torch_proxy, lib

    @property
    def called(self):
        return set(() if self.lib is None else self.lib.called)


@contextlib.contextmanager
def guarded(arena: Arena, modules=None, lib=None):
    """Inside the context the binding modules allocate from `arena` and their library calls are recorded.  `modules`: module objects to
    patch (default: cd360.ops, cd360.nerf, cd360.grad); `lib`: the library object to record (default: cd360._lib.load()'s) -- the
    self-test passes fakes for both and needs no library."""
    L = None
    if modules is None:
        import importlib
        modules = [importlib.import_module(m) for m in MODULES]
        L = importlib.import_module("cd360._lib")
        lib = L.load() if lib is None else lib
    proxy = TorchProxy(arena)
    rec = None if lib is None else Recorder(lib)
    saved = [(m, m.__dict__["torch"]) for m in modules]
    saved_load = None if L is None else L.load
    try:
        for m, _ in saved:
            m.torch = proxy
        if L is not None:
            L.load = lambda check_symbols=True: rec
        yield Guard(arena, proxy, rec)
    finally:
        for m, t in saved:
            m.torch = t
        if L is not None:
            L.load = saved_load


@contextlib.contextmanager
def recorded(guard, module):
    """Inside guarded()'s context: record the entry points of `module`'s library as well (guarded() records cd360._lib.load()'s library;
    cd360.ops reaches the others through cd360._edit.load(), cd360._optim.load(), cd360._text.load()), into the same list P4 reads."""
    rec = Recorder(module.load())
    saved = module.load
    module.load = lambda: rec
    try:
        yield rec
    finally:
        module.load = saved
        guard.lib.called.extend(rec.called)


def _flatten(x, out=None, path="result"):
    out = [] if out is None else out
    if isinstance(x, torch.Tensor):
        out.append((path, x))
    elif isinstance(x, dict):
        for k, v in x.items():
            _flatten(v, out, f"{path}[{k!r}]")
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flatten(v, out, f"{path}[{i}]")
    return out


def _same_bits(a, b) -> bool:
    """P3 compares BITS (an operand rewritten as -0.0 for +0.0, or a NaN payload changed, is a write); P2 compares with torch.equal after
    the finiteness check, so there +0.0 == -0.0 passes and a NaN never reaches the comparison."""
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def _call(fn, inputs, guard):
    kw = {"guard": guard} if getattr(fn, "wants_guard", False) else {}
    if isinstance(inputs, dict):
        return fn(**inputs, **kw)
    return fn(*inputs, **kw)


def run_twice(fn, inputs, declares=(), inout=(), valid=None, bit_equal=True, modules=None, lib=None):
    """Run fn(*inputs) (fn(**inputs) for a dict) under guarded(Arena(0xFF)), then under guarded(Arena(0x7F)); assert P1 - P4; return both
    results.
      declares   cd360_* entry points the call must reach (P4)
      inout      positions / names in `inputs` the header documents as in/out: restored before the second run, compared between the runs
                 like a result instead of against their clone.  They are the caller's tensors, NOT arena blocks: P1 sees no stray write
                 around them and they are not poisoned -- only their final bits are compared.  (Every input is outside the arena; P1
                 covers what the binding, or a case through guard.torch, allocates.)
      valid      results -> the tensors (slices of the valid region) P2 compares, for outputs whose remainder include/cd360_hip.h leaves
                 unspecified; default: every tensor of the result.  P1 has no exemptions.
      bit_equal  False only for the fp32-atomic scatter form: P2 keeps finiteness, drops the bit comparison
      fn.wants_guard = True: fn also receives guard=<Guard> (guard.torch / guard.lib) for entry points the binding does not wrap."""
    items = list(inputs.items()) if isinstance(inputs, dict) else list(enumerate(inputs))
    before = {k: v.clone() for k, v in items if isinstance(v, torch.Tensor)}
    for k in inout:
        assert k in before, f"in/out argument {k!r} is not a tensor input"
    results, finals, name = [], [], getattr(fn, "__name__", "case")
    for run, poison in enumerate(POISONS):
        if run:
            for k in inout:
                dict(items)[k].copy_(before[k])
        arena = Arena(poison)
        with guarded(arena, modules=modules, lib=lib) as g:
            res = _call(fn, inputs, g)
        arena.check()  # P1
        missing = sorted(set(declares) - g.called)
        if missing:
            raise GuardError(f"P4 entry point not called: {name} declares {missing}, the recorder saw {sorted(g.called)}")
        for k, v in before.items():
            if k not in inout and not _same_bits(dict(items)[k], v):
                raise GuardError(f"P3 operand modified: input {k!r} of {name} (shape {tuple(v.shape)}, {v.dtype}) differs from its clone "
                                 f"taken before the call (poison 0x{poison:02X})")
        results.append(res)
        finals.append({k: dict(items)[k].clone() for k in inout})
    cmp = []
    for res, fin in zip(results, finals):
        flat = _flatten(res if valid is None else valid(res))
        cmp.append(flat + [(f"in/out input {k!r}", v) for k, v in fin.items()])
    assert len(cmp[0]) == len(cmp[1])
    for (path, a), (_, b) in zip(*cmp):
        if a.is_floating_point() and not bool(torch.isfinite(a).all()):
            bad = (~torch.isfinite(a)).flatten().nonzero().flatten()
            raise GuardError(f"P2 not fully written / uninitialised read: {path} of {name} (shape {tuple(a.shape)}, {a.dtype}) holds "
                             f"{bad.numel()} non-finite elements under poison 0xFF, flat index {int(bad[0])} .. {int(bad[-1])}")
        if bit_equal and not (a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)):
            diff = (a != b).flatten().nonzero().flatten() if a.shape == b.shape else torch.zeros(1, dtype=torch.long)
            raise GuardError(f"P2 not fully written / uninitialised read: {path} of {name} (shape {tuple(a.shape)}, {a.dtype}) differs between "
                             f"the 0xFF and the 0x7F run in {diff.numel()} elements, flat index {int(diff[0])} .. {int(diff[-1])}")
    return results[0], results[1]
