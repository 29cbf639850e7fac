"""What tests/test_gpu_streams.py rests on: a device-side delay of a stated length, two torch side streams that are PROVEN to
overtake one another in this process, inputs that arrive late on a stream, and the fresh child process every test body runs
in.  Nothing here calls the library.

  delay(stream, ms)       a busy wait on `stream` (torch.cuda._sleep, its cycles calibrated once per process with two events;
                          without _sleep: in-place arithmetic on a large tensor, calibrated the same way)
  side_streams()          (A, B, log): two side streams (hipStreamNonBlocking) for which work enqueued on one runs in front of
                          delayed work on the other, in both directions -- the control of every ordering assertion.  Pairs of
                          torch's pool are tried, at most eight: two streams that share a hardware queue cannot overtake.  No
                          pair: RuntimeError (the test fails; it never skips).
  late(stream, ...)       tensors that hold a DECOY (another valid batch) until, behind a delay on `stream`, the real values
                          are copied in; returns the event recorded right behind the delay
  run_child(script, ...)  one test body in a fresh interpreter, with a time limit; after a child that ended in a signal or at
                          its time limit no further child is started
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_CAL = {}          # "cycles_per_ms" (torch.cuda._sleep) or "reps_per_ms" + "tensor" (the fallback), measured once
CONTROL_MS = 20.0  # the delay of the overtaking control
MAX_PAIRS = 8


def _torch():
    import torch

    return torch


def _timed_ms(stream, enqueue):
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        enqueue()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(stream=None):
    """Measure what one millisecond of busy wait costs (once per process) -> the dict of the measurement."""
    torch = _torch()
    if _CAL:
        return _CAL
    stream = stream or torch.cuda.current_stream()
    if hasattr(torch.cuda, "_sleep"):
        _timed_ms(stream, lambda: torch.cuda._sleep(1_000_000))                  # (first launch: not measured)
        cycles = 20_000_000
        ms = _timed_ms(stream, lambda: torch.cuda._sleep(cycles))
        _CAL.update(kind="_sleep", cycles_per_ms=cycles / ms, probe_ms=ms)
    else:
        t = torch.zeros(1 << 24, dtype=torch.float32, device="cuda")

        def spin(reps):
            for _ in range(reps):
                t.mul_(1.0000001)

        _timed_ms(stream, lambda: spin(4))
        ms = _timed_ms(stream, lambda: spin(64))
        _CAL.update(kind="arithmetic", reps_per_ms=64 / ms, probe_ms=ms, tensor=t)
    return _CAL


def delay(stream, ms):
    """Enqueue a device-side busy wait of `ms` milliseconds on `stream`."""
    torch = _torch()
    cal = calibrate()
    with torch.cuda.stream(stream):
        if cal["kind"] == "_sleep":
            torch.cuda._sleep(int(cal["cycles_per_ms"] * ms))
        else:
            for _ in range(max(1, int(cal["reps_per_ms"] * ms))):
                cal["tensor"].mul_(1.0000001)


def overtakes(fast, slow, ms=CONTROL_MS):
    """True when work enqueued on `fast` AFTER delayed work on `slow` runs in front of it: behind a delay on `slow`, src is
    copied into dst; at once src is overwritten on `fast`; dst then holds the overwritten values.  A benign race on two
    tensors of this function's own."""
    torch = _torch()
    src = torch.full((4096,), 1.0, dtype=torch.float32, device="cuda")
    dst = torch.zeros(4096, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    delay(slow, ms)
    with torch.cuda.stream(slow):
        dst.copy_(src)
    with torch.cuda.stream(fast):
        src.fill_(2.0)
    with torch.cuda.stream(slow):
        got = dst.cpu()
    fast.synchronize()
    slow.synchronize()
    return bool((got == 2.0).all())


def side_streams():
    """(A, B, log) -- see the module's docstring.  `log`: one line per pair tried, for the test's output."""
    torch = _torch()
    calibrate()
    log = []
    A = torch.cuda.Stream()
    for k in range(MAX_PAIRS):
        B = torch.cuda.Stream()
        if B.cuda_stream == A.cuda_stream or 0 in (A.cuda_stream, B.cuda_stream):
            log.append(f"pair {k}: the pool handed out the same stream twice")
            continue
        ab, ba = overtakes(B, A), overtakes(A, B)
        log.append(f"pair {k}: B in front of delayed A: {ab}, A in front of delayed B: {ba}")
        if ab and ba:
            return A, B, log
    raise RuntimeError("no pair of torch side streams overtakes in this process (%d pairs tried): %s -- without that control "
                       "every ordering assertion would pass vacuously" % (MAX_PAIRS, "; ".join(log)))


def late(stream, tensors, real, decoy, ms):
    """`tensors` (the device tensors a call is about to be handed) hold `decoy` now; behind a delay of `ms` on `stream` the
    `real` values are copied in (device staging, filled and synchronised by the caller beforehand).  The three are sequences
    of equal length (None entries are skipped).  Returns the event recorded on `stream` right behind the delay: while it is
    pending, nothing enqueued on `stream` after this call can have run."""
    torch = _torch()
    for t, d in zip(tensors, decoy):
        if t is not None:
            t.copy_(d)
    torch.cuda.synchronize()          # (before anything is enqueued: the decoy is in place)
    delay(stream, ms)
    with torch.cuda.stream(stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        for t, r in zip(tensors, real):
            if t is not None:
                t.copy_(r, non_blocking=True)
    return ev


def delay_ms_for(serial_wall_s):
    """the delay that covers the host time between the first enqueue and the second call's kernels: max(50 ms, 20 x the warm
    serial wall time of the calls)"""
    return max(50.0, 20.0 * 1000.0 * serial_wall_s)


# ---- the child process of a test body ---------------------------------------------------------------------------------------

_STOPPED = []      # why no further child is started (a child ended in a signal or at its time limit)


def run_child(script, args, timeout=120.0):
    """Run `script` (a path) with `args` in a fresh interpreter -> (its last JSON line as a dict, stdout).  AssertionError when
    the child fails; after a child that ended in a signal or at its time limit every later call fails at once."""
    if _STOPPED:
        raise AssertionError("no further child is started: " + _STOPPED[0])
    cmd = [sys.executable, script, *[str(a) for a in args]]
    t0 = time.time()
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _STOPPED.append("%s ran into its time limit of %d s" % (" ".join(cmd[1:]), timeout))
        raise AssertionError(_STOPPED[0] + "\n" + str(e.stdout or "")[-2000:] + str(e.stderr or "")[-2000:])
    if p.returncode < 0 or p.returncode in (134, 139):
        _STOPPED.append("%s ended with status %d" % (" ".join(cmd[1:]), p.returncode))
    print(p.stdout[-6000:])
    print("child wall time: %.1f s" % (time.time() - t0))
    assert p.returncode == 0, "%s: exit status %d\n%s\n%s" % (" ".join(cmd[1:]), p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, "the child printed no result line:\n" + p.stdout[-2000:]
    return json.loads(lines[-1]), p.stdout
