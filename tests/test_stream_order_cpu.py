"""mfrl_amd.policy.StreamOrder, the record of which streams have seen a handle's current state, with fake streams and
events: who waits for what, how often, and that the producer's own stream -- the default path -- never records or
waits for an event.  The GPU side is tests/test_stream_order_gpu.py."""
from mfrl_amd.policy import StreamOrder


class Log:
    def __init__(self):
        self.recorded, self.waited = [], []

    def record(self, stream):
        self.recorded.append(stream)
        return ("event", len(self.recorded), stream)

    def wait(self, stream, event):
        self.waited.append((stream, event))

    def order(self):
        return StreamOrder(record=self.record, wait=self.wait)


def test_producer_stream_never_records_or_waits():
    log = Log()
    o = log.order()
    assert o.ready(7, "s7") is False and o.gen == 0          # before any state: nothing to wait for, nothing marked
    assert o.seen == set()
    for gen in (1, 2, 3):
        o.produced(7, "s7")
        assert o.gen == gen and o.seen == {7}
        for _ in range(3):
            assert o.ready(7, "s7") is False
    assert log.recorded == [] and log.waited == []


def test_foreign_stream_waits_once_per_generation():
    log = Log()
    o = log.order()
    o.produced(1, "C")
    assert o.ready(2, "S1") is True
    assert log.recorded == ["C"] and log.waited == [("S1", ("event", 1, "C"))]
    for _ in range(5):                                       # the steady state: a set lookup
        assert o.ready(2, "S1") is False and 2 in o.seen
    assert len(log.recorded) == 1 and len(log.waited) == 1
    # a second engine's stream waits too (on the same event: one record per generation), the producer's never
    assert o.ready(3, "S2") is True and o.ready(1, "C") is False
    assert log.recorded == ["C"] and log.waited[1] == ("S2", ("event", 1, "C"))
    # the state moves again, now on another stream: everyone else waits again, once, on a new event from that stream
    o.produced(3, "S2")
    assert o.gen == 2 and o.seen == {3}
    assert o.ready(2, "S1") is True and o.ready(1, "C") is True and o.ready(3, "S2") is False
    assert log.recorded == ["C", "S2"]
    assert log.waited[2:] == [("S1", ("event", 2, "S2")), ("C", ("event", 2, "S2"))]
    assert o.ready(2, "S1") is False and o.ready(1, "C") is False
    assert len(log.waited) == 4


def test_stream_object_is_fetched_only_when_waiting():
    log = Log()
    o = log.order()
    calls = []

    def get():
        calls.append(1)
        return "S"

    o.produced(1, "C")
    assert o.ready(1, get) is False and calls == []
    assert o.ready(2, get) is True and calls == [1]
    assert o.ready(2, get) is False and calls == [1]
    assert log.waited == [("S", ("event", 1, "C"))]


def test_a_producer_that_extends_the_state_keeps_the_order_transitive():
    """Weights on C, then the support image -- which gathers from the weights -- on T: T waits for C before it
    produces, so a consumer that waits for T's event alone is behind both."""
    log = Log()
    o = log.order()
    o.produced(1, "C")
    assert o.ready(5, "T") is True                           # (ACNetHIP._extend)
    o.produced(5, "T")
    assert o.ready(2, "S") is True
    assert log.waited == [("T", ("event", 1, "C")), ("S", ("event", 2, "T"))]
    assert log.recorded == ["C", "T"]


def test_a_reused_stream_id_waits_in_the_next_generation():
    """`seen` is rebuilt at every production: an id kept from an earlier generation never passes for ordered."""
    log = Log()
    o = log.order()
    o.produced(1, "C")
    o.ready(2, "S")
    o.produced(1, "C")
    assert 2 not in o.seen and o.ready(2, "S-again") is True
    assert log.waited[-1] == ("S-again", ("event", 2, "C"))
