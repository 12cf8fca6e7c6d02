"""Every kernel entry point runs on the caller's stream: ``ops._call`` hands torch's current
stream to each of them, and every launch, memset and copy behind it must be given that stream.

Each case of tests/stream_order_cases.py runs twice on a side stream (tests/stream_helpers.py):
in scenario A the side stream is held back and the inputs still hold a decoy, in scenario B the
null stream is held back.  Either way the clones of the outputs must be the bits of the same
operation on the default stream -- which the float64 tests of each family hold to its
restatement, so nothing is re-derived here.  A hook on ``_lib.call`` records the entry points a
case reaches, re-arms the null stream's delay behind host round trips and fails a case as
inconclusive when a delay drained where it had to be pending.

The two controls show, with torch operations alone, that a mis-ordered consumer or producer IS
seen on this machine; if they fail, the cases prove nothing."""

import pytest
import torch

from tests import stream_helpers as sh
from tests.stream_order_cases import CASES

pytestmark = pytest.mark.gpu

_REACHED, _RAN = set(), set()


def test_control_a_a_consumer_on_the_null_stream_reads_the_decoy():
    side = sh.side_stream()
    real = torch.arange(4096, dtype=torch.float32, device="cuda")
    decoy = real.flip(0).contiguous()
    live = decoy.clone()
    torch.cuda.synchronize()
    released = sh.delay().issue(side)
    with torch.cuda.stream(side):
        live.copy_(real)                    # the producer, behind the delay
    early = live.clone()                    # the consumer, on the default stream
    assert not released.query(), "inconclusive: the delay drained before the consumer was issued"
    torch.cuda.synchronize()
    assert torch.equal(early, decoy), "the harness is blind: the null stream waited for the side stream"
    assert torch.equal(live, real)


def test_control_b_a_step_on_the_delayed_null_stream_is_missed():
    side = sh.side_stream()
    x = torch.arange(4096, dtype=torch.float32, device="cuda")
    # every buffer is made before the delay: a fresh allocation may wait for the whole device
    y, z, w, seen = (torch.zeros_like(x) for _ in range(4))
    # and every kernel has run once: loading its code may wait for the device too
    with torch.cuda.stream(side):
        torch.add(x, 1, out=y)
        torch.mul(y, 2, out=z)
        torch.add(z, 3, out=w)
        seen.copy_(w)
        for t in (y, z, w, seen):
            t.zero_()
    torch.cuda.synchronize()
    released = sh.delay().issue(torch.cuda.default_stream())
    with torch.cuda.stream(side):
        torch.add(x, 1, out=y)
    torch.mul(y, 2, out=z)                  # the stray step, on the delayed default stream
    with torch.cuda.stream(side):
        torch.add(z, 3, out=w)
        seen.copy_(w)
    assert not released.query(), "inconclusive: the delay drained before the clone was issued"
    torch.cuda.synchronize()
    assert torch.equal(z, (x + 1) * 2)
    assert not torch.equal(seen, (x + 1) * 2 + 3), \
        "the harness is blind: the side stream waited for the null stream"
    assert torch.equal(seen, torch.full_like(x, 3))


@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_launch_is_on_the_callers_stream(case, scenario, monkeypatch):
    from fourier_feature_nets_amd import _lib
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    hook = sh.Hook(_lib.call)
    monkeypatch.setattr(_lib, "call", hook)
    _REACHED.update(sh.run_case(case, scenario, hook, monkeypatch))
    _RAN.add((case.name, scenario))


def test_the_cases_reached_every_stream_taking_entry_point():
    """Judged only when every case has run in both scenarios in this session (the last test of
    the module); a selection of cases (-k, --lf, a single rerun) cannot show it and is skipped:
    tests/test_stream_order_cpu.py holds the table to the header on every run."""
    if len(_RAN) < 2 * len(CASES):
        pytest.skip("only %d of %d case runs in this session" % (len(_RAN), 2 * len(CASES)))
    missing = sorted(set(sh.stream_entry_points()) - _REACHED)
    assert not missing, "no case reached %s" % missing
