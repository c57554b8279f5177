"""Hold a torch stream back for a bounded time, so that a test can tell on which stream a library call enqueued.

    ev = stream_gate.gate(side)          # `side` now runs a spin kernel of some tens of milliseconds
    ... enqueue the work under test ...
    assert not ev.query()                # the gate was still closed when the enqueue returned

Work enqueued on the gated stream cannot start before the gate ends; work that went to another stream by mistake runs at
once and reads whatever its inputs held then.  The gate is torch.cuda._sleep(cycles) (a kernel that spins on the
device clock for a fixed count, nothing the host could leave waiting for ever), calibrated once per process by timing
a fixed count between two events; where that helper does not spin on this runtime, a chain of large torch.mm's.
No kernel here waits for a host flag.
"""
import torch

GATE_MS = 60.0                    # some tens of milliseconds: longer than enqueueing a whole chain takes the host
_SLEEP_PROBE_CYCLES = 1 << 20
_MM_N = 4096

_calibration = None               # ("sleep", cycles per ms) or ("mm", ms per product, (a, b, out))


def _time_on(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate():
    """The gate's mechanism and its rate on this device, measured once: ("sleep", cycles per ms) or ("mm", ms each)."""
    global _calibration
    if _calibration is not None:
        return _calibration
    s = torch.cuda.Stream()
    try:
        torch.cuda._sleep(1000)                      # loads the kernel
        torch.cuda.synchronize()
        cycles, ms = _SLEEP_PROBE_CYCLES, 0.0
        for _ in range(8):                           # grow the count until it is long enough to time: at most 2^34 cycles
            ms = _time_on(s, lambda: torch.cuda._sleep(cycles))
            if ms >= 5.0:
                break
            cycles *= 4
        if ms >= 5.0:
            _calibration = ("sleep", cycles / ms)
    except (AttributeError, RuntimeError):
        pass
    if _calibration is None:                         # the spin helper does not hold the stream here: matrix products
        a = torch.rand((_MM_N, _MM_N), device="cuda:0")
        b = torch.rand((_MM_N, _MM_N), device="cuda:0")
        out = torch.empty_like(a)
        torch.mm(a, b, out=out)
        torch.cuda.synchronize()
        ms = _time_on(s, lambda: [torch.mm(a, b, out=out) for _ in range(8)]) / 8
        _calibration = ("mm", ms, (a, b, out))
    print(f"\nstream gate: {describe()}")
    return _calibration


def describe(ms: float = GATE_MS) -> str:
    c = calibrate()
    if c[0] == "sleep":
        return f"torch.cuda._sleep, {c[1]:.0f} cycles per ms, {int(c[1] * ms)} cycles for a {ms:.0f} ms gate"
    return f"torch.mm {_MM_N}x{_MM_N}, {c[1]:.3f} ms each, {max(1, round(ms / c[1]))} products for a {ms:.0f} ms gate"


def gate(stream, ms: float = GATE_MS):
    """Enqueue about `ms` milliseconds of device-side waiting on `stream`; returns an event recorded right after it
    (event.query() is False until the gate has ended)."""
    c = calibrate()
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        if c[0] == "sleep":
            torch.cuda._sleep(int(c[1] * ms))
        else:
            a, b, out = c[2]
            for _ in range(max(1, round(ms / c[1]))):
                torch.mm(a, b, out=out)
        ev.record()
    return ev


def measure(ms: float = GATE_MS) -> float:
    """How long a gate of `ms` really holds an otherwise idle side stream, in milliseconds."""
    calibrate()
    s = torch.cuda.Stream()
    return _time_on(s, lambda: gate(s, ms))


def control_side_gate(side):
    """A gate on `side` does not hold the default stream back: the default stream's copy sees the old value."""
    x = torch.zeros(1 << 16, device="cuda:0")
    y = torch.full_like(x, 2)
    torch.cuda.synchronize()
    ev = gate(side)
    with torch.cuda.stream(side):
        x.fill_(1)
    y.copy_(x)                                       # on the default stream
    open_at_enqueue = not ev.query()
    side.synchronize()
    torch.cuda.synchronize()
    return {"gate open at enqueue": open_at_enqueue, "early copy": y.cpu(), "late value": x.cpu()}


def control_null_gate(side):
    """The roles exchanged: a gate on the default stream does not hold `side` back."""
    default = torch.cuda.default_stream()
    x = torch.zeros(1 << 16, device="cuda:0")
    y = torch.full_like(x, 2)
    torch.cuda.synchronize()
    ev = gate(default)
    x.fill_(1)                                       # on the default stream, behind the gate
    with torch.cuda.stream(side):
        y.copy_(x)
    open_at_enqueue = not ev.query()
    side.synchronize()
    torch.cuda.synchronize()
    return {"gate open at enqueue": open_at_enqueue, "early copy": y.cpu(), "late value": x.cpu(),
            "default handle": default.cuda_stream, "side handle": side.cuda_stream}


def control_problems(res) -> list:
    """What of a control's result does not hold (empty: the control holds)."""
    bad = []
    if not res["gate open at enqueue"]:
        bad.append("the gate had ended before the enqueues returned")
    if not bool((res["early copy"] == 0).all()):
        bad.append("the other stream's copy did not see the value from before the gated write: it holds "
                   f"{sorted(set(res['early copy'].tolist()))}")
    if not bool((res["late value"] == 1).all()):
        bad.append("the gated stream's write did not land")
    if res.get("default handle", 0) != 0:
        bad.append("torch's default stream is not stream 0")
    if res.get("side handle", 1) == 0:
        bad.append("torch's side stream is stream 0")
    return bad


_picked = None


def side_stream(k: int = 0):
    """The k-th (0 or 1) of two side streams on which both controls hold, picked once per process.  AssertionError
    naming the control where this machine has none: a test that needs the gate fails then, it does not skip."""
    streams, problems = picked()
    for control, bad in problems.items():
        assert not bad, f"precondition: the control '{control}' holds on no side stream of this machine: {bad}"
    return streams[k]


def picked():
    """pick_side_streams(2), once per process."""
    global _picked
    if _picked is None:
        _picked = pick_side_streams(2)
    return _picked


def pick_side_streams(n: int = 2, tries: int = 32):
    """n side streams for which both controls hold, and what was seen on the way: (streams, {control: problems}).

    The runtime maps its streams onto a few hardware queues (GPU_MAX_HW_QUEUES), and two streams that share a queue run
    one after the other although nothing orders them: a gate on one of them holds the other back as well, and a test
    cannot tell the two apart.  torch.cuda.Stream() hands out the streams of a pool in turn, so the controls are tried
    on one after the other until n of them run beside the default stream.  Fewer than n: the problems of the last one tried."""
    streams, seen, last = [], set(), {}
    for _ in range(tries):
        s = torch.cuda.Stream()
        if s.cuda_stream in seen:
            break                                    # the pool has come round
        seen.add(s.cuda_stream)
        last = {"side gate (test_control_side_gate)": control_problems(control_side_gate(s)),
                "null gate (test_control_null_gate)": control_problems(control_null_gate(s))}
        if not any(last.values()):
            streams.append(s)
            if len(streams) == n:
                break
    print(f"\nstream gate: {len(streams)} of {len(seen)} side streams tried run beside the default stream")
    return streams, ({} if len(streams) == n else last)
