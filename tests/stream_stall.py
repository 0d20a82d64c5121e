"""A stalled stream for the cross-stream hand-off tests (tests/test_stream_order_gpu.py).

On an idle GPU a producer on one stream finishes long before the host has enqueued the consumer on another, so a
missing edge between the two never shows.  Here the producer's stream is kept busy first:

    stall(stream, ms)         enqueue about `ms` of work on `stream`; -> an event recorded after it
    independent_streams(k)    k non-default streams that do not order each other by sharing a hardware queue, as
                              measured: with a stall on A, a one-element kernel on B completes while A's stall is pending
    Case(name, stalled)       one case: warm-up on throw-away handles, the stall, the sequence under test with no
                              synchronisation of any kind, `outlived` read right after the last enqueue, then the sync

The stall is torch.cuda._sleep(cycles), its cycles per millisecond calibrated once per process against events; if that
does not scale linearly (10x the cycles within 8..12x the time) the stall is a chain of dependent fp32 matmuls on a
fixed 4096 x 4096 operand, counted the same way.  It is a bounded delay (at most MAX_MS), never a wait on a condition.

The length of a case's stall is max(50 ms, 20 x the host time its warm-up took to enqueue the same sequence), capped
at MAX_MS.  Every case prints one JSON line (the calibration, the enqueue times, the length), and appends it to the
file STREAM_STALL_OUT names (profiles/stream_stall.jsonl was recorded that way).
"""
import gc
import json
import os
import time

MIN_MS, MAX_MS, FACTOR = 50.0, 500.0, 20.0

_cal = None            # {"mode": "sleep" | "matmul", "per_ms": units per ms, "ratio": t(10 u) / t(u), "timed_ms": ...}
_mat = None
_streams = []


def _timed(stream, fn):
    """Milliseconds `fn` keeps `stream` busy (events; synchronises)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _matmul_chain(n):
    x = _mat[1]
    for _ in range(int(n)):
        x = _mat[0] @ x               # (each product reads the one before: the chain cannot overlap itself)
    return x


def calibration():
    """Once per process: the unit of the stall (sleep cycles or matmuls) per millisecond.  Synchronises."""
    global _cal, _mat
    if _cal is not None:
        return _cal
    import torch
    s = torch.cuda.Stream()
    _timed(s, lambda: torch.cuda._sleep(1000))                            # (the kernel's first launch)
    t1 = _timed(s, lambda: torch.cuda._sleep(2_000_000))
    t10 = _timed(s, lambda: torch.cuda._sleep(20_000_000))
    ratio = t10 / max(t1, 1e-6)
    if 8.0 <= ratio <= 12.0 and t10 > 0.5:
        _cal = {"mode": "sleep", "per_ms": 20_000_000 / t10, "ratio": ratio}
    else:
        with torch.cuda.stream(s):
            g = torch.Generator(device="cuda").manual_seed(1)
            _mat = (torch.rand((4096, 4096), device="cuda", generator=g) / 2048.0,        # (row sums ~1: no overflow)
                    torch.rand((4096, 4096), device="cuda", generator=g))
        _timed(s, lambda: _matmul_chain(2))
        m1 = _timed(s, lambda: _matmul_chain(4))
        m10 = _timed(s, lambda: _matmul_chain(40))
        _cal = {"mode": "matmul", "per_ms": 40 / m10, "ratio": m10 / max(m1, 1e-6), "sleep_ratio": ratio}
    torch.cuda.synchronize()
    _cal["timed_ms"] = _timed(s, lambda: stall(s, MIN_MS))                # the final stall, timed once
    _cal["asked_ms"] = MIN_MS
    print("stream_stall calibration:", json.dumps(_cal))
    return _cal


def stall(stream, ms):
    """Keep `stream` busy for about `ms` (at most MAX_MS); -> an event recorded on it after that work."""
    import torch
    cal = calibration()
    ms = min(float(ms), MAX_MS)
    with torch.cuda.stream(stream):
        if cal["mode"] == "sleep":
            torch.cuda._sleep(int(ms * cal["per_ms"]))
        else:
            _matmul_chain(max(1, round(ms * cal["per_ms"])))
        ev = torch.cuda.Event()
        ev.record()
    return ev


def _independent(a, b, ms=20.0):
    """With `a` stalled, does a one-element kernel on `b` complete while the stall is still pending?"""
    import torch
    x = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    pending = stall(a, ms)
    with torch.cuda.stream(b):
        x.add_(1.0)
        done = torch.cuda.Event()
        done.record()
    done.synchronize()
    ok = not pending.query()
    pending.synchronize()
    return ok


def independent_streams(k):
    """k non-default torch streams, pairwise independent in both directions as measured (two torch streams can share
    one of the process's hardware queues, and a stall then orders them by accident: every stalled case would pass
    vacuously), none of which holds up the null stream either.  Drawn from a pool of at most 8; kept for the process.
    Fails -- never skips -- when there are not k."""
    import torch
    calibration()
    tried = len(_streams)
    pool = []
    while len(_streams) < k and tried + len(pool) < 8:
        c = torch.cuda.Stream()
        pool.append(c)
        # (the null stream too: the library's blocking hipMemcpy calls run there, and one that shares its queue with a
        # stalled stream holds the host until the stall is over)
        if (c.cuda_stream != 0 and _independent(c, torch.cuda.default_stream())
                and all(_independent(c, s) and _independent(s, c) for s in _streams)):
            _streams.append(c)
    assert len(_streams) >= k, "stream_stall: %d pairwise independent streams among %d tried, %d wanted" % (
        len(_streams), tried + len(pool), k)
    return _streams[:k]


class Case:
    """One stalled case.

        case = Case("name", stalled=C)
        case.warm(lambda: sequence(throw_away_handles))     # timed on the host, then synchronised
        out = case.run(lambda: sequence(handles))           # stall armed, enqueue, `outlived`, synchronise

    outlived: the stall was still pending right after the last enqueue of the sequence -- the consumer was enqueued
    while the producer's stream had not yet run the producer.  host_ms: the sequence's host time under the stall."""

    def __init__(self, name, stalled):
        self.name, self.stalled = name, stalled
        self.warm_ms = self.host_ms = self.stall_ms = None
        self.outlived = None

    def warm(self, fn):
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.warm_ms = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        del out
        gc.collect()                     # (a handle freed later would synchronise the device under the stall)
        torch.cuda.synchronize()
        return self

    def run(self, fn):
        import torch
        assert self.warm_ms is not None, "Case.run: warm() the sequence on throw-away handles first"
        self.stall_ms = min(MAX_MS, max(MIN_MS, FACTOR * self.warm_ms))
        gc.collect()
        torch.cuda.synchronize()
        gc.disable()
        try:
            pending = stall(self.stalled, self.stall_ms)
            t0 = time.perf_counter()
            out = fn()
            self.host_ms = 1e3 * (time.perf_counter() - t0)
            self.outlived = not pending.query()
        finally:
            gc.enable()
        torch.cuda.synchronize()
        rec = {"case": self.name, "warm_enqueue_ms": round(self.warm_ms, 3), "enqueue_ms": round(self.host_ms, 3),
               "stall_ms": round(self.stall_ms, 1), "outlived": self.outlived, "calibration": calibration()}
        print(json.dumps(rec))
        if os.environ.get("STREAM_STALL_OUT"):
            with open(os.environ["STREAM_STALL_OUT"], "a") as f:
                f.write(json.dumps(rec) + "\n")
        return out
