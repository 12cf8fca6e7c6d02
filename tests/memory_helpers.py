"""The harness of the memory-bounds tests (tests/test_memory_bounds_gpu.py): every entry point of
include/ffn_hip.h writes only through its non-``const`` pointers and only inside those buffers,
writes every output word, and reads its inputs only inside their extents.

torch's caching allocator hides all three kinds of error: a block is rounded up to 512 bytes and
shares a segment with unrelated tensors (a write past an output lands in slack), a freed block
comes back holding the previous right answer (an unwritten word passes), and what lies beyond an
input is whatever torch left there.  Here every buffer a case makes is GUARDED instead:

* a guarded buffer is the middle of a ``uint8`` allocation of its own, ``left + nbytes + right``
  bytes: the payload starts 512-byte aligned, as ``torch.empty`` memory does, and ends exactly
  where the right red zone begins, so that an overrun of one element lands in the zone.  A zone is
  ``max(4096, nbytes rounded up to 512)`` bytes: 4096 covers a block of 256 threads that stores
  16 bytes a lane, the proportional part a doubled count or stride;
* the zones, and the payload of what stands in for ``torch.empty``, hold one of two fills (FILLS):
  finite floats in [0, 1] that are exact in bf16, and the integers 1 and 0, which are in range as
  an index, a flag or a count of every array of the cases (tests/stream_helpers.py argues this for
  its mark).  A stray read computes a wrong answer from in-range data, never a wild access;
* a registry keeps every buffer made, so that the address of a pointer argument finds its owner.

A case runs under fill A and under fill B: the zones must come back untouched, and the outputs
must be the same bits both times and the bits of a run on plain torch memory."""

import re

import torch

from tests.stream_helpers import HEADER

# torch's own factories, taken before any guard stands in for them
_RAW = {name: getattr(torch, name)
        for name in ("empty", "zeros", "empty_like", "zeros_like", "full")}
raw_clone = torch.Tensor.clone

ALIGN = 512                      # what torch.empty gives on the device
MIN_ZONE = 4096                  # 256 threads x 16 bytes
FILLS = {"A": (0.37109375, 1), "B": (0.62890625, 0)}    # (floats, integers)


# ------------------------------------------------------------------------------------ the header
class Param:
    def __init__(self, text):
        self.text = " ".join(text.split())
        self.pointer = "*" in self.text
        self.name = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", self.text)[-1]
        self.const = self.pointer and bool(re.match(r"const\b", self.text))

    def __repr__(self):
        return "Param(%r)" % self.text


def signatures():
    """Every entry point of include/ffn_hip.h that takes a ``stream`` -> its ordered parameters
    (the trailing ``stream`` included), each with ``name``, ``pointer`` and ``const``; parsed as
    ``stream_helpers.stream_entry_points`` parses the header."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        if not re.search(r"\bstream\b", params):
            continue
        parsed = [Param(p) for p in params.split(",")]
        assert parsed[-1].name == "stream" and not parsed[-1].const, name
        out[name] = parsed
    return out


def written(name, sigs=None):
    """The names of the pointers ``name`` may write through (``stream`` is not one)."""
    return [p.name for p in (sigs or signatures())[name][:-1] if p.pointer and not p.const]


# ------------------------------------------------------------------------------------ placement
def zone_bytes(nbytes):
    return max(MIN_ZONE, -(-nbytes // ALIGN) * ALIGN)


def _plain(t):
    """``t`` as a type of its width that fills and compares everywhere (uint32 does not)."""
    signed = {"torch.uint16": torch.int16, "torch.uint32": torch.int32, "torch.uint64": torch.int64,
              "torch.bool": torch.uint8}
    return t.view(signed[str(t.dtype)]) if str(t.dtype) in signed else t


class Buffer:
    """One guarded buffer: ``base`` (uint8, 1-D) = left zone | payload | right zone."""

    def __init__(self, base, offset, shape, dtype, kind, fill):
        self.base, self.offset, self.shape, self.dtype, self.kind = base, offset, shape, dtype, kind
        self.nbytes = _itemsize(dtype) * _numel(shape)
        self.zone = zone_bytes(self.nbytes)
        self.start = base.data_ptr() + offset
        self.end = self.start + self.nbytes
        self.fill = fill[0] if dtype.is_floating_point else fill[1]
        self.users = set()          # the entry points whose arguments pointed into the payload
        self.tensor = self.bytes().view(dtype).view(shape)
        for zone in self.zones():
            zone.fill_(self.fill)

    def bytes(self):
        return self.base[self.offset:self.offset + self.nbytes]

    def zones(self):
        """(left, right) as 1-D tensors of the payload's element type."""
        lo, hi = self.offset - self.zone, self.offset + self.nbytes
        return [_plain(self.base[a:a + self.zone].view(self.dtype)) for a in (lo, hi)]

    def owns(self, address):
        return self.start <= address < self.end

    def damage(self):
        """None, or the text that reports what was written into the zones."""
        size = self.tensor.element_size()
        found = []
        for side, zone in zip(("left", "right"), self.zones()):
            changed = (zone != self.fill).nonzero().reshape(-1)
            if changed.numel():
                first, last = int(changed[0]), int(changed[-1])
                if side == "left":      # bytes before the payload's start
                    span = "%d .. %d bytes before the payload's start" % (
                        (zone.numel() - first) * size, (zone.numel() - 1 - last) * size + 1)
                else:
                    span = "%d .. %d bytes past the payload's end" % (first * size,
                                                                      (last + 1) * size - 1)
                found.append("%d elements of the %s zone changed, %s" % (changed.numel(), side, span))
        if not found:
            return None
        return "%s %s buffer (%s), arguments of %s: %s" % (
            tuple(self.shape), self.dtype, self.kind, sorted(self.users) or "no call",
            "; ".join(found))


def _itemsize(dtype):
    return _RAW["empty"]((), dtype=dtype).element_size()


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Guard:
    """The guarded placement of one run: ``fill`` is "A" or "B", ``device_type`` the kind of device
    whose tensors are guarded ("cuda" in the GPU test, "cpu" in the test of the harness itself)."""

    def __init__(self, fill, device_type="cuda"):
        self.name, self.fill, self.device_type = fill, FILLS[fill], device_type
        self.buffers = []
        self.problems = []              # what the call hook found (tests/test_memory_bounds_gpu.py)
        self.const_seen, self.const_guarded = 0, 0
        self.const_moved = 0            # ... moved into a guarded copy for the call (Hook)
        self.const_unguarded = set()    # (entry point, parameter) of those the call saw unguarded
        self.unguarded_written = set()  # (entry point, parameter) written through, not guarded
        self.reached = []

    # -- making buffers
    def buffer(self, shape, dtype, device, kind):
        """A guarded buffer -> its Buffer.  ``kind``: "empty" (the payload holds the fill), "zeros"
        or "input" (the caller copies into it)."""
        shape = tuple(int(s) for s in shape)
        nbytes = _itemsize(dtype) * _numel(shape)
        zone = zone_bytes(nbytes)
        base = _RAW["empty"]((zone + nbytes + zone,), dtype=torch.uint8, device=device)
        offset = zone
        if base.data_ptr() % ALIGN:     # host memory: the allocation carries its own slack
            base = _RAW["empty"]((zone + nbytes + zone + ALIGN,), dtype=torch.uint8, device=device)
            offset = zone + (-(base.data_ptr() + zone)) % ALIGN
        buf = Buffer(base, offset, shape, dtype, kind, self.fill)
        if kind == "zeros":
            buf.bytes().zero_()
        elif kind == "empty" and nbytes:
            _plain(buf.tensor).fill_(buf.fill)
        self.buffers.append(buf)
        return buf

    def place(self, t):
        """``t`` (contiguous) moved into a guarded buffer of its own; other tensors as they are."""
        if not self._ours(t.device) or not t.is_contiguous() or t.numel() == 0 or t.requires_grad:
            return t
        buf = self.buffer(t.shape, t.dtype, t.device, "input")
        buf.bytes().copy_(t.reshape(-1).view(torch.uint8))
        return buf.tensor

    def _ours(self, device):
        return device is not None and torch.device(device).type == self.device_type

    # -- the registry
    def find(self, address):
        for buf in self.buffers:
            if buf.owns(address):
                return buf
        return None

    def damage(self):
        return [d for d in (buf.damage() for buf in self.buffers) if d]

    # -- standing in for torch
    def patch(self, patch):
        """From here to the end of ``patch`` (a pytest ``monkeypatch`` or one of its contexts)
        ``torch.empty``, ``torch.empty_like``, ``torch.zeros``, ``torch.zeros_like`` and, because
        the in-place entry points write through them, ``Tensor.clone`` and ``torch.full`` (the
        z-buffer of the rasteriser) give guarded buffers for tensors of this guard's device type;
        every other form (CPU tensors, ``pin_memory``, ``out=``, ``memory_format=``, empty shapes,
        ...) passes through to torch."""
        def shape_of(size):
            if len(size) == 1 and not isinstance(size[0], int):
                size = tuple(size[0])
            if not all(isinstance(s, int) and not isinstance(s, bool) for s in size):
                raise TypeError
            return tuple(size)

        def maker(raw, kind):
            def make(*size, dtype=None, device=None, **other):
                try:
                    shape = shape_of(size)
                except TypeError:
                    return raw(*size, dtype=dtype, device=device, **other)
                if other or not self._ours(device) or _numel(shape) == 0:
                    return raw(*size, dtype=dtype, device=device, **other)
                return self.buffer(shape, dtype or torch.get_default_dtype(), device, kind).tensor
            return make

        def maker_like(raw, kind):
            def make(t, dtype=None, device=None, **other):
                device_ = t.device if device is None else device
                if (other or not self._ours(device_) or t.numel() == 0 or not t.is_contiguous()
                        or t.layout != torch.strided):
                    return raw(t, dtype=dtype, device=device, **other)
                return self.buffer(t.shape, dtype or t.dtype, device_, kind).tensor
            return make

        def full(size, fill_value, dtype=None, device=None, **other):
            try:
                shape = shape_of((size,))
            except TypeError:
                return _RAW["full"](size, fill_value, dtype=dtype, device=device, **other)
            if (other or not self._ours(device) or _numel(shape) == 0
                    or not isinstance(fill_value, (int, float))):
                return _RAW["full"](size, fill_value, dtype=dtype, device=device, **other)
            dtype = dtype or _RAW["full"]((), fill_value).dtype
            buf = self.buffer(shape, dtype, device, "input")
            buf.tensor.fill_(fill_value)
            return buf.tensor

        def clone(t, *args, **kwargs):
            if (args or kwargs or type(t) is not torch.Tensor or t.layout != torch.strided
                    or t.requires_grad or t.numel() == 0 or not t.is_contiguous()
                    or not self._ours(t.device)):
                return raw_clone(t, *args, **kwargs)
            return self.place(t)

        patch.setattr(torch, "empty", maker(_RAW["empty"], "empty"))
        patch.setattr(torch, "zeros", maker(_RAW["zeros"], "zeros"))
        patch.setattr(torch, "empty_like", maker_like(_RAW["empty_like"], "empty"))
        patch.setattr(torch, "zeros_like", maker_like(_RAW["zeros_like"], "zeros"))
        patch.setattr(torch, "full", full)
        patch.setattr(torch.Tensor, "clone", clone)
        # ``_dev`` hands the tensor on with its pointer: the call hook moves an input that torch made
        # (a sort, a linspace, an uploaded table, a parameter) into a guarded copy for the call
        from fourier_feature_nets_amd import mlp_engine, ops
        raw_dev = ops._dev

        def dev(t, *args, **kwargs):
            ptr = raw_dev(t, *args, **kwargs)
            ptr.tensor = t
            return ptr

        patch.setattr(ops, "_dev", dev)
        patch.setattr(mlp_engine, "_dev", dev)
        # the builders' ``_t`` (tests/stream_order_cases.py) makes nearly every input of the cases
        from tests import stream_order_cases
        patch.setattr(stream_order_cases, "PLACE", self.place)


# ------------------------------------------------------------------------------------ the hook
def _extent(ptr):
    """The addresses [lo, hi) of the tensor behind a device pointer (one byte where none is known)."""
    t = getattr(ptr, "tensor", None)
    return ptr.value, ptr.value + max(1, 0 if t is None else t.numel() * t.element_size())


class Hook:
    """Stands in for ``_lib.call``: records every entry point and, while a Guard is ``active``,
    looks every device pointer of the call up in its registry.  A ``const`` pointer that no guarded
    buffer owns, and whose tensor overlaps nothing the call may write, is replaced for the call by
    a guarded copy of its tensor: the entry point only reads it, so nothing else changes."""

    def __init__(self, call):
        self.call, self.sigs = call, signatures()
        self.names, self.active = [], None

    def __call__(self, name, *args):
        from fourier_feature_nets_amd.ops import _DevPtr
        self.names.append(name)
        guard = self.active
        if guard is None:
            return self.call(name, *args)
        guard.reached.append(name)
        params = self.sigs[name]
        assert len(args) == len(params), (     # both counts less the trailing ``stream``
            "%s is given %d arguments before the stream, the header declares %d"
            % (name, len(args) - 1, len(params) - 1))
        read, wrote = {}, {}
        args = list(args)
        targets = [_extent(arg) for param, arg in zip(params[:-1], args[:-1])
                   if isinstance(arg, _DevPtr) and arg.value and not param.const]
        for k, (param, arg) in enumerate(zip(params[:-1], args[:-1])):
            if not isinstance(arg, _DevPtr) or not arg.value:
                continue
            assert param.pointer, "%s: a device pointer for %r" % (name, param.text)
            buf = guard.find(arg.value)
            if param.const:
                guard.const_seen += 1
                guard.const_guarded += buf is not None
                t = getattr(arg, "tensor", None)
                lo, hi = _extent(arg)
                if buf is None and t is not None and not any(lo < w_hi and w_lo < hi
                                                             for w_lo, w_hi in targets):
                    placed = guard.place(t)
                    buf = guard.find(placed.data_ptr())
                    if buf is not None:
                        args[k] = _DevPtr(placed.data_ptr())
                        args[k].device = arg.device
                        guard.const_moved += 1
                if buf is None:
                    guard.const_unguarded.add((name, param.name))
            else:
                if buf is None:
                    guard.unguarded_written.add((name, param.name))
            if buf is not None:
                buf.users.add(name)
                (read if param.const else wrote)[id(buf)] = (buf, param.name)
        inputs = [pair for key, pair in read.items() if key not in wrote]
        before = [raw_clone(buf.bytes()) for buf, _ in inputs]
        out = self.call(name, *args)
        torch.cuda.synchronize()
        for (buf, pname), snapshot in zip(inputs, before):
            if not torch.equal(buf.bytes(), snapshot):
                changed = (buf.bytes() != snapshot).nonzero().reshape(-1)
                guard.problems.append(
                    "%s wrote through its const parameter %s: %d bytes of the %s %s buffer changed, "
                    "payload bytes %d .. %d" % (name, pname, changed.numel(), tuple(buf.shape),
                                                buf.dtype, int(changed[0]), int(changed[-1])))
        return out
