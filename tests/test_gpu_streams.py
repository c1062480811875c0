"""Every entry point of the C ABI on a held side stream (tests/stream_cases.py: the protocol, its reasons and its one blind
spot).  The header's contract: a call only enqueues work on the caller's stream and does not wait for the device; the
documented exceptions (``stream_cases.SYNCHRONISING``) read flags on the host.

The hold is a chain of ``busy = busy @ busy * 1e-3`` on a 4096 x 4096 fp32 tensor on the side stream.  Its length is chosen
once per module by doubling the repeat count until two events on the side stream measure at least
max(30 ms, 20 x the largest host wall time of a non-synchronising case on an idle side stream); the factor 20 is margin for
scheduling noise on a shared host, a choice and not a measurement.  The two ``hold_done.query()`` checks are the condition:
a hold that is too short fails loudly.  profiles/streams/README.md records the numbers of one run.

The premise test and the two self-tests of the protocol come first: without them a pass of the cases would say nothing."""
import time

import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MIN_HOLD_MS, HOLD_FACTOR, MAX_REPEATS = 30.0, 20.0, 4096


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


@pytest.fixture(scope="module")
def instances(dev):
    """name -> the built case (or the exception its builder raised), built once and shared."""
    built = {}

    def get(name):
        if name not in built:
            try:
                built[name] = sc.CASES[name].build(dev)
            except Exception as error:   # noqa: BLE001 (kept for the test of that case, which raises it)
                built[name] = error
            torch.cuda.synchronize()
        if isinstance(built[name], Exception):
            raise built[name]
        return built[name]
    return get


class Hold:
    def __init__(self, dev):
        self.base = torch.randn(4096, 4096, device=dev)
        self.repeats, self.measured_ms, self.target_ms, self.host_ms = 1, 0.0, MIN_HOLD_MS, {}

    def __call__(self):
        busy = self.base
        for _ in range(self.repeats):
            busy = busy @ busy * 1e-3

    def measure(self):
        """Milliseconds of one hold between two events on an idle side stream."""
        side = torch.cuda.Stream()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            start.record(side)
            self()
            end.record(side)
        side.synchronize()
        return start.elapsed_time(end)


@pytest.fixture(scope="module")
def hold(dev, instances):
    h = Hold(dev)
    h.measure()   # (the first product loads its kernel)
    for name, case in sc.CASES.items():
        if case.synchronising:
            continue
        try:
            h.host_ms[name] = 1e3 * sc.host_time_on_idle_side_stream(instances(name))
        except Exception:   # noqa: BLE001 (the case's own test reports it)
            continue
    h.target_ms = max(MIN_HOLD_MS, HOLD_FACTOR * max(h.host_ms.values(), default=0.0))
    while True:
        h.measured_ms = h.measure()
        if h.measured_ms >= h.target_ms or h.repeats >= MAX_REPEATS:
            break
        h.repeats *= 2
    for name, ms in sorted(h.host_ms.items(), key=lambda kv: -kv[1]):
        print(f"host time {name}: {ms:.3f} ms")
    print(f"hold: target {h.target_ms:.1f} ms, {h.repeats} products, measured {h.measured_ms:.1f} ms")
    assert h.measured_ms >= h.target_ms, "the hold cannot be made long enough"
    return h


def test_premise_side_streams_do_not_block_against_stream_0(dev, hold):
    """With the side stream held, a trivial op on the default stream and its read-back complete while the hold still runs."""
    side = torch.cuda.Stream()
    hold_done = torch.cuda.Event()
    x = torch.arange(1000, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert side.cuda_stream != 0
        hold()
        hold_done.record(side)
    assert torch.cuda.current_stream().cuda_stream == 0
    total = float((x * 2.0).sum().cpu())
    still_held = not hold_done.query()
    side.synchronize()
    assert total == 999000.0
    assert still_held, "a default-stream op waited for the held side stream: the protocol could detect nothing on this runtime"


class TwoSteps:
    """A test-local computation in plain torch, no library code: step 1 writes an intermediate from ``In``, step 2 writes
    ``Out`` from the intermediate.  ``stray``: step 2 is issued on the default stream, as a launch with a lost stream argument
    would be.  ``wait``: the call ends in a read-back."""

    def __new__(cls, dev, stray=False, wait=False):
        i = sc.Inst(dev)
        rng = torch.Generator().manual_seed(1)
        x = i.inp(torch.rand(4096, generator=rng, dtype=torch.float64), torch.rand(4096, generator=rng, dtype=torch.float64))
        mid = i.work(8 * 4096).view(torch.float64)
        out = i.out("out", (4096,), torch.float64)

        def call():
            torch.mul(x, 3.0, out=mid)
            if stray:
                with torch.cuda.stream(torch.cuda.default_stream()):
                    torch.add(mid, 1.0, out=out)
            else:
                torch.add(mid, 1.0, out=out)
            if wait:
                out.cpu()
        i.call = call
        return i


def test_the_protocol_catches_a_step_on_the_wrong_stream(dev, hold):
    sc.run_protocol(TwoSteps(dev), hold)   # wholly on the caller's stream: passes
    with pytest.raises(sc.ProtocolFailure, match="step 6.*'out'.*still hold scene A"):
        sc.run_protocol(TwoSteps(dev, stray=True), hold)


def test_the_protocol_catches_a_host_wait(dev, hold):
    with pytest.raises(sc.ProtocolFailure, match="step 5: the hold had ended when the call returned"):
        sc.run_protocol(TwoSteps(dev, wait=True), hold)
    sc.run_protocol(TwoSteps(dev, wait=True), hold, synchronising=True)   # what a documented exception is held to


def test_the_protocol_rejects_a_vacuous_case(dev, hold):
    i = TwoSteps(dev)
    i.B[0].copy_(i.A[0])
    with pytest.raises(sc.ProtocolFailure, match="step 3"):
        sc.run_protocol(i, hold)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_entry_point_on_a_held_side_stream(name, instances, hold):
    case = sc.CASES[name]
    report = {}
    started = time.perf_counter()
    try:
        sc.run_protocol(instances(name), hold, synchronising=case.synchronising, report=report)
    finally:
        print(f"{name}: {case.entries} host {1e3 * report.get('host_time', float('nan')):.3f} ms, held before "
              f"{report.get('held_before')} after {report.get('held_after')}, protocol {time.perf_counter() - started:.2f} s")
