"""Guard bands, poisoned outputs and exact workspaces for the ops layer (test-side only).

    with guarded(ops, ops16) as g:
        dw = ops.conv2d_wgrad(x, dy, 3, out=g.place(slab_view, offset_elems=3))
        damage = g.verify()          # [] when nothing was written outside a tensor

Inside the block the name `torch` of each given module is a forwarding proxy: everything goes to the real torch except
`empty`, `zeros`, `empty_like` and `zeros_like`, the four allocation idioms `sivae_hip.ops`, `ops16` and `pointcloud`
use.  Those allocate ONE uint8 buffer `guard | body | guard` filled with the byte 0xFF and return the body viewed as the
requested dtype and shape (contiguous; `zeros*` then zero the body).  GUARD_BYTES is a multiple of 512, so the body keeps
the caching allocator's 512-byte alignment and the 16-byte-path predicates of the library choose what they choose in
production.  A module's `workspace` (ops' own and every copy imported by name) returns a FRESH guarded uint8 buffer of
EXACTLY the requested size — production never allocates less than 1 MiB, which satisfies every `*_workspace_bytes()`
whatever it returns.  The one exception is a request for 0 bytes: an empty tensor has no address and the entry points
refuse a null workspace, so it gets a view of ONE byte of the guard (the library is told 1 byte, not 0; writing that
byte is reported as damage).  The modules' caches of unguarded buffers
(`_workspaces`, `_counters`, `_bn_states`) are swapped for empty dicts, so the counter / barrier states come from the
proxy's `zeros`.  Everything is put back when the block ends, also after an exception.

0xFF everywhere is NaN as fp32, bf16 and fp64, -1 as int32 and 255 as uint8: an output element no kernel wrote turns the
checks' error figure into inf (they reject non-finite values) or fails their exact integer comparisons; no tolerance is
involved.

`place(t, offset_elems)` copies a caller-made tensor into a guarded body `offset_elems` elements behind its start (the
elements in front stay 0xFF and are verified like a guard): a destination for `out=` / `accumulate=` / `pg_out=` the
way optim.FlatAdam's slab views sit in their flat buffer, at any element offset and next to other tensors' bytes.

`verify()` synchronises, compares every guard with 0xFF, releases the allocations and returns one record per damaged
allocation: the allocating function and line in the patched module, shape, dtype, the first and last damaged byte
relative to the returned tensor (negative: in front of it) and the number of damaged bytes.

What this does not see:
  * a store whose address wraps inside the kernel's own buffer window (an out-of-range marker that is not 16 bytes below
    2^32 under a 16-byte store lands INSIDE the tensor: wrong values, which only the value checks can find);
  * reads past the end of an input (over-reads return guard bytes, i.e. NaN, only where the input itself came from the
    proxy);
  * anything farther away than GUARD_BYTES, and anything written with the byte 0xFF.
HIP-graph capture does not mix with it (the pattern fills would be captured).
"""
import contextlib
import sys

import torch as _torch

PATTERN = 0xFF
GUARD_BYTES = 256 * 1024  # the largest plane among the check shapes (256 x 256 fp32); raise it if a shape needs more
_CACHES = ("_workspaces", "_counters", "_bn_states")
# allocations / workspaces / placed destinations whose guards verify() has compared, over the whole process
TOTALS = {"allocations": 0, "workspaces": 0, "placed": 0, "damaged": 0}


class _Record:
    __slots__ = ("raw", "front", "nbytes", "site", "shape", "dtype", "kind")

    def __init__(self, raw, front, nbytes, site, shape, dtype, kind):
        self.raw, self.front, self.nbytes, self.site = raw, front, nbytes, site
        self.shape, self.dtype, self.kind = tuple(shape), dtype, kind


def _site(depth):
    f = sys._getframe(depth)
    return "%s:%s:%d" % (f.f_globals.get("__name__", "?"), f.f_code.co_name, f.f_lineno)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class _TorchProxy:
    """stands in for the module-level name `torch` of a patched module"""

    def __init__(self, guard):
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        return getattr(_torch, name)

    # (dtype and device are the only keywords the ops layer passes; another one — pin_memory, memory_format,
    # requires_grad — would be ignored here and change what the guarded run does: a TypeError instead)
    def empty(self, *size, dtype=None, device=None):
        return self._guard._alloc(_shape_of(size), dtype, device, False, "alloc")

    def zeros(self, *size, dtype=None, device=None):
        return self._guard._alloc(_shape_of(size), dtype, device, True, "alloc")

    def empty_like(self, t, dtype=None, device=None):
        return self._guard._alloc(t.shape, dtype or t.dtype, device or t.device, False, "alloc")

    def zeros_like(self, t, dtype=None, device=None):
        return self._guard._alloc(t.shape, dtype or t.dtype, device or t.device, True, "alloc")


class Guard:
    check_front = check_back = True  # (which guards verify() compares: switched off by hand to see the host test fail)

    def __init__(self, guard_bytes=GUARD_BYTES):
        if guard_bytes <= 0 or guard_bytes % 512:
            raise ValueError("guard_bytes must be a positive multiple of 512 (the body keeps the allocator's alignment)")
        self.guard_bytes = int(guard_bytes)
        self.records = []
        self.proxy = _TorchProxy(self)

    # ---------------------------------------------------------------------------------------------- allocation
    def _alloc(self, shape, dtype, device, zero, kind, front_elems=0):
        dtype = dtype or _torch.get_default_dtype()
        device = _torch.device(device if device is not None else "cpu")
        item = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        front = self.guard_bytes + front_elems * item
        nbytes = numel * item
        raw = _torch.empty(front + nbytes + self.guard_bytes, dtype=_torch.uint8, device=device)
        raw.fill_(PATTERN)
        # (guard_bytes is a multiple of 512 and front_elems whole elements: the view below is aligned for its dtype)
        body = raw[front:front + nbytes].view(dtype).view(shape)
        if zero:
            body.zero_()
        self.records.append(_Record(raw, front, nbytes, _site(3), shape, dtype, kind))
        return body

    def workspace(self, nbytes, device):
        """replacement of ops.workspace: a fresh buffer of exactly nbytes.  A 0-byte request gets a view of ONE byte of the
        guard behind it (an empty tensor has no address, and the entry points refuse a null workspace): that byte is
        verified like the rest of the guard."""
        ws = self._alloc((int(nbytes),), _torch.uint8, device, False, "workspace")
        if nbytes == 0:
            r = self.records[-1]
            ws = r.raw[r.front:r.front + 1]
        return ws

    def place(self, t, offset_elems=0):
        """t copied into a guarded body, offset_elems elements behind its start -> the view (contiguous, t's shape)"""
        view = self._alloc(t.shape, t.dtype, t.device, False, "placed", front_elems=int(offset_elems))
        view.copy_(t)
        return view

    # ---------------------------------------------------------------------------------------------- verification
    def verify(self):
        """-> [] or one dict per damaged allocation; the allocations are released"""
        recs, self.records = self.records, []
        if not recs:
            return []
        if any(r.raw.is_cuda for r in recs):
            _torch.cuda.synchronize()

        def parts(r):  # the verified regions of one allocation: (bytes, offset of their first byte from the tensor)
            end = r.front + r.nbytes
            return ([(r.raw[:r.front], -r.front)] if self.check_front else []) + \
                   ([(r.raw[end:], r.nbytes)] if self.check_back else [])

        dev = recs[0].raw.device
        counts = _torch.stack([sum(((p != PATTERN).sum() for p, _ in parts(r)), _torch.zeros((), dtype=_torch.int64,
                                                                                             device=r.raw.device)).to(dev)
                               for r in recs]).tolist()  # (one read-back for all of them)
        damage = []
        for r, n in zip(recs, counts):
            TOTALS[{"alloc": "allocations", "workspace": "workspaces", "placed": "placed"}[r.kind]] += 1
            if not n:
                continue
            pos = _torch.cat([(p != PATTERN).nonzero().flatten().cpu() + off for p, off in parts(r)])
            TOTALS["damaged"] += 1
            damage.append(dict(site=r.site, kind=r.kind, shape=r.shape, dtype=str(r.dtype).replace("torch.", ""),
                               first_byte=int(pos.min()), last_byte=int(pos.max()), damaged_bytes=int(n)))
        return damage


@contextlib.contextmanager
def guarded(*modules, guard_bytes=GUARD_BYTES):
    """patch `modules` (sivae_hip.ops, ops16, pointcloud — anything written in their style) for the block -> Guard"""
    g = Guard(guard_bytes)
    saved = []  # (module, name, value)
    originals = {id(m.__dict__["workspace"]): True for m in modules
                 if "_workspaces" in m.__dict__ and callable(m.__dict__.get("workspace"))}
    try:
        for m in modules:
            d = m.__dict__
            saved.append((m, "torch", d["torch"]))
            setattr(m, "torch", g.proxy)
            # the module's own workspace() and the copies other modules imported by name
            if callable(d.get("workspace")) and ("_workspaces" in d or id(d["workspace"]) in originals):
                saved.append((m, "workspace", d["workspace"]))
                setattr(m, "workspace", g.workspace)
            for name in _CACHES:
                if name in d:
                    saved.append((m, name, d[name]))
                    setattr(m, name, {})
        yield g
    finally:
        for m, name, value in reversed(saved):
            setattr(m, name, value)
        g.records = []


def describe(damage):
    """damage records -> one line each (assertion messages)"""
    return "\n".join("  %(kind)s %(dtype)s%(shape)s from %(site)s: %(damaged_bytes)d byte(s) damaged, offsets "
                     "%(first_byte)d .. %(last_byte)d relative to the tensor" % d for d in damage) or "  (none)"
