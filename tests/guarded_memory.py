"""Guard-band memory for the kernel tests (test-only; nothing in the product knows about it).

One byte arena filled with 0xFF (NaN as fp32 / bf16, -1 as an integer).  Every tensor it hands out starts at an address = 16 (mod 512) -- the
least the C ABI promises, never the 512 torch's allocator always gives -- and has at least 64 KiB of poison on either side; nothing is handed
out within 1 MiB of the arena's ends.  `guarded(arena)` routes, for the duration of a `with` block,

  * `kernels.workspace(nbytes, device)` to an arena slice of EXACTLY `nbytes` bytes (re-poisoned before every call; the launcher is told `nbytes`,
    not the size of a grown-and-kept buffer),
  * the allocations `iseg_amd/kernels.py` makes through its module global `torch` (empty / empty_like / zeros / zeros_like / full / ... on the
    arena's device type) to the arena: empty ones stay poison, zeros / full / ones keep their values,
  * the `q()` operand helper of tests/test_kernels_gpu.py (and the copies other test modules imported) to the arena.

`arena.check()` then asserts, on the device and on the stream the kernels ran on, that every byte NOT inside a handed-out tensor is still 0xFF.

What this cannot see: a read out of range whose value is discarded (a read that is multiplied by a zero mask instead of skipped does show: the
band is NaN, and the caller's parity check fails), and a stray access farther away than the arena reaches.
"""
import contextlib
import functools
import inspect
import sys

import torch

POISON = 0xFF
MARGIN = 1 << 20            # nothing is handed out this close to either end of the arena
BAND = 64 << 10             # untouched poison on either side of every handed-out tensor
DEFAULT_BYTES = 128 << 20
ALIGN_MODULUS = 512         # torch's own allocations are = 0 (mod 512); the arena's are = align (mod 512)


class GuardViolation(AssertionError):
    """a byte outside every handed-out tensor changed.  offset: arena byte offset of the first such byte; record: the nearest handed-out tensor;
    side / distance: ("after", d): the byte is d bytes past the tensor's end (0 = the byte right behind it); ("before", d): d bytes in front of its first byte"""

    def __init__(self, msg, offset, record, side, distance):
        super().__init__(msg)
        self.offset, self.record, self.side, self.distance = offset, record, side, distance


class Record:
    def __init__(self, start, end, role, shape, dtype, name):
        self.start, self.end, self.role, self.shape, self.dtype, self.name = start, end, role, tuple(shape), dtype, name

    def __repr__(self):
        return f"{self.role} '{self.name}' shape {self.shape} {self.dtype} at arena bytes [{self.start}, {self.end})"


class Arena:
    def __init__(self, device, nbytes=DEFAULT_BYTES, margin=MARGIN, band=BAND):
        self.device = torch.device(device)
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.nbytes, self.margin, self.band = int(nbytes), int(margin), int(band)
        self.records = []
        self.reset()

    # ---- allocation ---------------------------------------------------------------------------------------------------------------------
    def reset(self):
        """start of a test: all poison, nothing handed out"""
        self.buf.fill_(POISON)
        self.records = []
        self._top = self.margin
        self._count = 0

    def alloc(self, shape, dtype, role, *, align=16, name=None):
        """a contiguous tensor of poison inside the arena; role is one of "workspace", "output", "operand" """
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = n * item
        if nbytes == 0:
            return torch.empty(shape, dtype=dtype, device=self.device)
        base = self.buf.data_ptr()
        start = self._top + self.band
        start += (align % ALIGN_MODULUS - (base + start)) % ALIGN_MODULUS
        end = start + nbytes
        if end + self.band > self.nbytes - self.margin:
            raise MemoryError(f"guard arena exhausted: {nbytes} more bytes after {self._top} of {self.nbytes}")
        self._top = end
        self._count += 1
        rec = Record(start, end, role, shape, dtype, name or f"{role}#{self._count}")
        self.records.append(rec)
        # a tensor of its own over the arena's storage, not a view of self.buf: a custom autograd Function may return it, and the re-poisoning
        # fill_ of the buffer does not count as an in-place change of it
        t = torch.empty(0, dtype=dtype, device=self.device)
        return t.set_(self.buf.untyped_storage(), (self.buf.storage_offset() + start) // item, shape)

    def offset_of(self, t):
        return t.data_ptr() - self.buf.data_ptr()

    # ---- the check ----------------------------------------------------------------------------------------------------------------------
    def check(self):
        """every arena byte not inside a handed-out tensor is still poison (device-side compare on the current stream, one host read)"""
        bad = self.buf != POISON
        for r in self.records:
            bad[r.start:r.end] = False
        if not bool(bad.any().item()):
            return
        offset = int(torch.nonzero(bad)[0].item())
        value = int(self.buf[offset].item())
        if not self.records:
            raise GuardViolation(f"arena byte {offset} changed to 0x{value:02x} and nothing was handed out", offset, None, None, None)
        best = None
        for r in self.records:
            side, dist = ("before", r.start - offset) if offset < r.start else ("after", offset - r.end)
            if best is None or dist < best[2]:
                best = (r, side, dist)
        r, side, dist = best
        where = f"{dist} bytes past the end of" if side == "after" else f"{dist} bytes before the start of"
        count = int(bad.sum().item())
        raise GuardViolation(f"guard band broken: arena byte {offset} is 0x{value:02x} ({count} bytes changed in all); the first is {where} {r!r}",
                             offset, r, side, dist)

    def untouched(self, role="output", since=0):
        """the handed-out tensors of a role (None: of every role), from record index `since` on, that are still all poison -> (untouched, total)"""
        recs = [r for r in self.records[since:] if role is None or r.role == role]
        if not recs:
            return 0, 0
        flags = torch.stack([(self.buf[r.start:r.end] == POISON).all() for r in recs])
        return int(flags.sum().item()), len(recs)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scoped patching
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _TorchProxy:
    """stands in for the module global `torch` of iseg_amd/kernels.py: allocation functions carve from the arena, everything else is torch's"""

    def __init__(self, arena, align):
        self._arena, self._align = arena, align

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    @staticmethod
    def _size(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def _new(self, size, dtype):
        return self._arena.alloc(size, dtype or torch.get_default_dtype(), "output", align=self._align)

    def _like(self, t, dtype):
        out = self._arena.alloc(t.numel(), dtype or t.dtype, "output", align=self._align)
        span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
        if t.is_contiguous() or span != t.numel() or len(set(t.stride())) != t.dim():
            return out.view(t.shape)
        return out.as_strided(t.shape, t.stride())      # (torch.empty_like keeps the strides of a dense permuted tensor)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._new(self._size(size), dtype)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._new(self._size(size), dtype).zero_()

    def ones(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.ones(*size, dtype=dtype, device=device, **kw)
        return self._new(self._size(size), dtype).fill_(1)

    def full(self, size, fill_value, *, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.get_default_dtype() if isinstance(fill_value, float) else (torch.bool if isinstance(fill_value, bool) else torch.int64)
        return self._new(self._size((size,)), dtype).fill_(fill_value)

    def empty_like(self, t, *, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, dtype)

    def zeros_like(self, t, *, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, dtype).zero_()

    def ones_like(self, t, *, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.ones_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, dtype).fill_(1)

    def full_like(self, t, fill_value, *, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.full_like(t, fill_value, dtype=dtype, device=device, **kw)
        return self._like(t, dtype).fill_(fill_value)


class Scope:
    """what `guarded` yields.  refused_from: with short_workspace, the arena's record count when the innermost kernels.py function that raised
    HipCallError was entered -- every record from there on belongs to the refused call"""

    def __init__(self, arena):
        self.arena, self.refused_from, self.short_from = arena, None, None


def _noting_refusals(f, scope, error):
    @functools.wraps(f)
    def call(*a, **kw):
        mark = len(scope.arena.records)
        try:
            return f(*a, **kw)
        except error:
            if scope.refused_from is None:
                scope.refused_from = mark
            raise

    return call


def _restore_dict(d, saved):
    d.clear()
    d.update(saved)


@contextlib.contextmanager
def guarded(arena, *, align=16, short_workspace=0, kernels=None):
    """inside the block: kernels.workspace, the allocations of kernels.py and the q() operand helper of the test modules use the arena.
    short_workspace = n hands every launcher n bytes less than it asked for (and says so): the launcher has to refuse, and the scope notes
    which records the refused call owns (refused_from) and where its short workspace is (short_from)."""
    if kernels is None:
        from iseg_amd import kernels
    slices = {}
    scope = Scope(arena)

    def workspace(nbytes, device):
        nbytes = int(nbytes)
        if nbytes <= 0:
            return None, 0
        give = nbytes - int(short_workspace)
        if give <= 0:
            return None, 0
        ws = slices.get(give)
        if ws is None:
            if short_workspace and scope.short_from is None:
                scope.short_from = len(arena.records)
            ws = slices[give] = arena.alloc(give, torch.uint8, "workspace", align=align)
        ws.fill_(POISON)        # no launcher may count on what an earlier call left behind
        return ws, give

    def q(t, dtype):
        s = t.to(dtype)
        d = arena.alloc(s.shape, s.dtype, "operand", align=align)
        d.copy_(s)
        return d, s.to(torch.float64)

    saved_q = [(m, m.q) for name, m in list(sys.modules.items())
               if name.startswith("tests.") and m is not None and callable(getattr(m, "q", None))]
    saved = (kernels.workspace, kernels.torch)
    # module-level buffers that outlive a call must not end up inside an arena that the next test poisons again
    keep = [(d, type(d)(d)) for d in (getattr(kernels, n, None) for n in ("_WS", "_DCN_SIDE", "_DEFER")) if isinstance(d, dict)]
    dirty = set(getattr(kernels, "_DCN_SIDE_DIRTY", ()))
    wrapped = {}
    if short_workspace:
        from iseg_amd import _hip

        wrapped = {n: f for n, f in vars(kernels).items() if inspect.isfunction(f) and f.__module__ == kernels.__name__
                   and n not in ("workspace", "stream", "ptr", "dt", "_require_cuda")}
        for n, f in wrapped.items():
            setattr(kernels, n, _noting_refusals(f, scope, _hip.HipCallError))
    kernels.workspace, kernels.torch = workspace, _TorchProxy(arena, align)
    for m, _ in saved_q:
        m.q = q
    try:
        yield scope
    finally:
        kernels.workspace, kernels.torch = saved
        for n, f in wrapped.items():
            setattr(kernels, n, f)
        for m, old in saved_q:
            m.q = old
        for d, old in keep:
            _restore_dict(d, old)
        if hasattr(kernels, "_DCN_SIDE_DIRTY"):
            kernels._DCN_SIDE_DIRTY.clear()
            kernels._DCN_SIDE_DIRTY.update(dirty)
