"""The harness of the stream-order tests (tests/test_stream_order_gpu.py): every entry point of
include/ffn_hip.h that takes a ``stream`` must put ALL its launches, memsets and copies on it.

The GPU tests elsewhere run on the default stream, the legacy null stream, where a launch that was
given stream 0 instead of the caller's is ordered by accident.  Here the caller's stream is a torch
pool stream (``side``; those do not block against the null stream) and one of the two streams is
held back by a calibrated delay:

* scenario A, the caller delayed: the live inputs hold a DECOY; on ``side`` go the delay, the copy
  of the real values into the live inputs, the operation and the clones of its outputs.  Whatever
  the entry point put on the null stream runs at once and reads the decoy.
* scenario B, the null stream delayed: the live inputs hold the real values, the delay goes on the
  default stream, the operation and the clones on ``side``.  Whatever was put on the null stream
  runs after its consumers and after the clones.

The clones are compared bit for bit with the same operation on the default stream.  A decoy is a
valid input (the real tensor flipped along its batch dimension, or a second valid tensor of the
same shape), structural arrays stay live from the start, and fresh ``torch.empty`` memory is
filled with a finite sentinel (floats) or ones (integers): a mis-ordered run computes a wrong
answer from in-range data, never an out-of-range access.

The streams of a process share a few hardware queues.  A side stream that shares the null stream's
queue is ordered against it by the hardware, and a stray launch would pass by accident: every case
first shows, with two torch copies, that ITS side stream runs past a held-back null stream's
neighbour (``side_stream``), and takes another pool stream if it does not."""

import os
import re
import time

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "ffn_hip.h")
FLOOR_MS = 10.0                 # three orders of magnitude above a launch's enqueue time
SENTINEL = 0.37109375           # finite, exact in f32 and bf16: safe as a position, a density, a weight


def stream_entry_points():
    """The entry points of include/ffn_hip.h whose parameter list names ``stream`` (parsed as
    ``_lib.declared_symbols`` parses it; needs neither a GPU nor the library)."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    found = re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text)
    return sorted({name for name, params in found if re.search(r"\bstream\b", params)})


# ------------------------------------------------------------------------------------ the delay
class Delay:
    """``issue(stream)`` holds ``stream`` back for at least FLOOR_MS (measured once a session)."""

    def __init__(self):
        import torch
        self.kind, self.count, self.ms = "torch.cuda._sleep", 1 << 20, 0.0
        if hasattr(torch.cuda, "_sleep"):
            while self.count <= 1 << 36:
                self.ms = self._measure()
                if self.ms >= FLOOR_MS:
                    break
                self.count *= 2
        if self.ms < FLOOR_MS:          # missing, or it does not delay on this device
            self.kind, self.count = "matmul chain", 1
            self._a = torch.randn(1024, 1024, device="cuda") * 0.01
            while self.count <= 1 << 16:
                self.ms = self._measure()
                if self.ms >= FLOOR_MS:
                    break
                self.count *= 2
        assert self.ms >= FLOOR_MS, "no delay of %.0f ms could be made on this device" % FLOOR_MS
        print("stream order: delay = %s(%d), measured %.2f ms" % (self.kind, self.count, self.ms))

    def _enqueue(self):
        import torch
        if self.kind == "torch.cuda._sleep":
            torch.cuda._sleep(self.count)
        else:
            x = self._a
            for _ in range(self.count):
                x = x @ self._a

    def _measure(self):
        import torch
        self._enqueue()                 # the first use pays for code loading
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self._enqueue()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def issue(self, stream):
        """The delay on ``stream`` -> an event recorded behind it (``query()``: has it drained)."""
        import torch
        with torch.cuda.stream(stream):
            self._enqueue()
            released = torch.cuda.Event()
            released.record(stream)
        return released


_DELAY = None


def delay():
    global _DELAY
    if _DELAY is None:
        _DELAY = Delay()
    return _DELAY


# ------------------------------------------------------------------------------------ the streams
_SIDE, _PROBE = None, None


def overlaps(side):
    """Whether work on the null stream runs past a held-back ``side``: control A in small."""
    import torch
    global _PROBE
    if _PROBE is None:
        real = torch.arange(1024, dtype=torch.float32, device="cuda")
        _PROBE = (real, real.flip(0).contiguous(), torch.empty_like(real), torch.empty_like(real))
    real, decoy, live, early = _PROBE
    with torch.cuda.stream(side):           # the copy kernels have run once on both streams
        live.copy_(real)
    early.copy_(live)
    live.copy_(decoy)
    torch.cuda.synchronize()
    released = delay().issue(side)
    with torch.cuda.stream(side):
        live.copy_(real)
    early.copy_(live)
    pending = not released.query()
    torch.cuda.synchronize()
    return pending and bool(torch.equal(early, decoy))


def side_stream():
    """A torch pool stream that does run concurrently with the null stream, probed before every
    use; the pool's streams are tried in turn."""
    import torch
    global _SIDE
    for _ in range(32):
        if _SIDE is None:
            _SIDE = torch.cuda.Stream()
        if overlaps(_SIDE):
            return _SIDE
        print("stream order: pool stream %#x is ordered against the null stream; the next is tried"
              % _SIDE.cuda_stream)
        _SIDE = None
    raise AssertionError("the harness is blind: no pool stream runs past the null stream")


# ------------------------------------------------------------------------------------ memory
def mark_empties(patch):
    """From here to the end of ``patch`` (a pytest ``monkeypatch`` or one of its contexts)
    ``torch.empty`` / ``torch.empty_like`` memory starts as SENTINEL (floats) or 1 (integers),
    filled on the current stream: the wrappers' outputs and scratch arrays.  A launch that runs
    too late, a clearing memset among them, leaves the mark where the answer belongs (0 would hide
    a missing clear), and a 1 read as a flag, a count or an index is in range of every array of the
    cases, which hold hundreds of elements.  Memory from ``new_empty``, ``torch.zeros``,
    ``torch.full`` and from torch operations is NOT marked: it is either initialised by torch on
    the current stream or not an output of a kernel of this library."""
    import torch
    empty, empty_like = torch.empty, torch.empty_like

    def mark(t):
        if t.numel():
            t.fill_(SENTINEL if t.dtype.is_floating_point else 1)
        return t

    patch.setattr(torch, "empty", lambda *a, **k: mark(empty(*a, **k)))
    patch.setattr(torch, "empty_like", lambda *a, **k: mark(empty_like(*a, **k)))


def is_mark(t):
    """Whether every element of ``t`` still holds the mark of ``mark_empties``."""
    if t is None or t.numel() == 0:
        return False
    return bool((t == (SENTINEL if t.dtype.is_floating_point else 1)).all())


def clones(outputs):
    return [None if o is None else o.clone() for o in outputs]


def same_bits(a, b):
    import torch
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                       b.contiguous().reshape(-1).view(torch.uint8))


def differing(got, want):
    """The numbers of the outputs that are not the same bits."""
    assert len(got) == len(want)
    return [k for k, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]


# ------------------------------------------------------------------------------------ the hook
class Inconclusive(AssertionError):
    """The delay drained where it had to be pending: the run proves nothing."""


class Hook:
    """Stands in for ``_lib.call``: records every entry point, and holds the delay to its word
    around every call (module docstring of tests/test_stream_order_gpu.py)."""

    def __init__(self, call):
        self.call = call
        self.names = []
        self.scenario, self.released, self.armed_at = None, None, 0.0
        self.rearms, self.refreshed, self.calls_in_scenario = 0, 0, 0

    def arm(self, scenario, stream):
        self.scenario, self.stream = scenario, stream
        self.released = delay().issue(stream)
        self.armed_at = time.perf_counter()
        self.rearms, self.refreshed, self.calls_in_scenario = 0, 0, 0

    def disarm(self):
        self.scenario = None

    def pending(self):
        return not self.released.query()

    def __call__(self, name, *args):
        self.names.append(name)
        if self.scenario == "A" and self.calls_in_scenario == 0 and not self.pending():
            raise Inconclusive("inconclusive: the caller's delay drained before the first call (%s)"
                               % name)
        if self.scenario == "B":
            # behind a host round trip the delay may have drained: a fresh one goes on (a re-arm).
            # One also goes on when the last is older than a third of its length (a refresh, counted
            # apart), so that no call starts with a delay about to end
            drained = not self.pending()
            if drained or (time.perf_counter() - self.armed_at) * 1e3 > delay().ms / 3:
                self.released = delay().issue(self.stream)
                self.armed_at = time.perf_counter()
                self.rearms += drained
                self.refreshed += not drained
        self.calls_in_scenario += 1
        out = self.call(name, *args)
        if self.scenario == "B" and not self.pending():
            raise Inconclusive("inconclusive: the null stream's delay of %.1f ms drained during %s"
                               % (delay().ms, name))
        return out


# ------------------------------------------------------------------------------------ one case
def take_extras(live):
    """Takes what is not a tensor out of a builder's ``live`` -> (decoys, kept, check_reference)
    (tests/stream_order_cases.py, module docstring)."""
    return live.pop("_decoys", {}), live.pop("_kept", {}), live.pop("_check_reference", None)


def keep_answers(patch, kept):
    """The wrappers' host-side checks named in ``kept`` give their recorded answers (``_keep_answer``
    of tests/stream_order_cases.py) to the end of ``patch``."""
    from fourier_feature_nets_amd import ops
    for name, answer in kept.items():
        patch.setattr(ops, name, lambda *args, _answer=answer, **kwargs: _answer)


def run_case(case, scenario, hook, monkeypatch):
    """Runs ``case`` (tests/stream_order_cases.py) in ``scenario`` "A" or "B" -> the entry points
    it reached.  Raises AssertionError naming the outputs that differ and the call sequence."""
    import torch
    assert scenario in ("A", "B")
    delay()
    null, side = torch.cuda.default_stream(), side_stream()
    assert null.cuda_stream == 0 and side.cuda_stream != 0
    live, run = case.build(torch.device("cuda:0"))
    custom, kept, check_reference = take_extras(live)
    real = {k: live[k].clone() for k in case.decoy}
    decoy = {k: (custom[k] if k in custom else real[k].flip(0)).contiguous() for k in case.decoy}
    for k in case.decoy:
        assert decoy[k].shape == real[k].shape and decoy[k].dtype == real[k].dtype

    def put(values):
        for k in case.decoy:
            live[k].copy_(values[k])

    with monkeypatch.context() as patch:
        mark_empties(patch)
        keep_answers(patch, kept)
        put(real)
        want = clones(run(live))
        torch.cuda.synchronize()
        if check_reference is not None:
            check_reference(want)
        if case.clear_only:
            # no input changes the answer of a path that only clears: the marks are the teeth
            marked = [k for k, o in enumerate(want) if is_mark(o)]
            assert not marked, "%s: outputs %s equal the mark: no teeth" % (case.name, marked)
        else:
            put(decoy)
            other = clones(run(live))
            torch.cuda.synchronize()
            assert differing(other, want), ("%s: the decoy gives the real answer: no teeth"
                                            % case.name)
        # warm-up on the caller's stream, with the decoy: packing, grow-only workspaces and the
        # allocator's growth happen here, and every cached workspace holds decoy-derived values
        with torch.cuda.stream(side):
            clones(run(live))
        torch.cuda.synchronize()
        first = len(hook.names)
        try:
            if scenario == "A":
                hook.arm("A", side)
                with torch.cuda.stream(side):
                    put(real)
                    got = clones(run(live))
            else:
                put(real)
                torch.cuda.synchronize()
                hook.arm("B", null)
                with torch.cuda.stream(side):
                    got = clones(run(live))
                if not hook.pending():
                    raise Inconclusive("inconclusive: the null stream's delay drained before the "
                                       "outputs were cloned")
        finally:
            hook.disarm()
            torch.cuda.synchronize()
            put(real)
            torch.cuda.synchronize()
    reached = hook.names[first:]
    print("stream order: %s [%s] reached %s; re-arms behind a drained delay %d, refreshes %d"
          % (case.name, scenario, ", ".join(sorted(set(reached))), hook.rearms, hook.refreshed))
    missing = sorted(set(case.reaches) - set(reached))
    assert not missing, "%s does not reach %s" % (case.name, missing)
    wrong = differing(got, want)
    assert not wrong, (
        "%s, scenario %s (%s): outputs %s differ from the default-stream run.  Something behind one "
        "of these calls did not go onto the caller's stream: %s"
        % (case.name, scenario, "caller delayed" if scenario == "A" else "null stream delayed",
           wrong, " -> ".join(reached)))
    return set(reached)
