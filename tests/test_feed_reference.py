"""The scheduler model of the feed (``tests/feed_reference.py``): hand-worked cases and the invariants the GPU tests lean on.
No GPU: the model is what decides, in those tests, what the twin handle is told through ``hold`` / ``resume`` / ``push``."""
import numpy as np
import pytest

from feed_reference import FeedModel, Refused

H = 256


def model(S=3, cap=4 * H):
    m = FeedModel(S, H)
    m.enable_feed(cap)
    return m


def test_hand_worked_tick():
    m = model()
    m.feed([0, 1, 2], 300, [300, 255, 0])
    t = m.tick()
    assert t.ready == {0} and t.starved == {1, 2}
    assert sorted(t.writes) == [(1, "hold"), (2, "hold")]
    assert t.taken[0] == list(range(256)) and m.queued() == [44, 255, 0]
    assert m.P == H and m.last_consumed == [True, False, False]
    # slot 1 gets its missing sample, slot 0 is short now: one resume, one hold, slot 2 costs nothing
    m.feed(1, 1)
    t = m.tick()
    assert t.ready == {1} and t.starved == {0, 2}
    assert sorted(t.writes) == [(0, "hold"), (1, "resume")]
    assert t.taken[1] == list(range(256)) and m.queued() == [44, 0, 0]
    # two hops at once: the oldest 512 of slot 0, in order
    m.feed(0, 3 * H)
    t = m.tick(2)
    assert t.ready == {0} and t.taken[0] == list(range(256, 768)) and m.queued(0) == 44 + 256
    assert m.P == 4 * H


def test_a_slot_starved_over_ten_ticks_costs_two_entries():
    m = model(2)
    writes = []
    for k in range(10):
        m.feed(0, H)
        writes += m.tick().writes
    m.feed([0, 1], H)
    writes += m.tick().writes
    assert writes == [(1, "hold"), (1, "resume")] and m.writes == 2


def test_nobody_ready_changes_nothing():
    m = model()
    m.feed([0, 1], 100)
    m.hold(2)
    before = (m.P, m.queued(), list(m.starved), list(m.on_device), m.writes)
    assert m.tick() is None
    assert (m.P, m.queued(), list(m.starved), list(m.on_device), m.writes) == before
    assert m.last_consumed == [False] * 3
    # a held slot with a full queue is not ready either
    m.feed(2, 2 * H)
    assert m.tick() is None and m.queued(2) == 2 * H


def test_caller_holds():
    m = model(2)
    assert m.hold(1) == [(1, "hold")]
    m.feed([0, 1], H)
    t = m.tick()
    assert t.ready == {0} and t.starved == set() and t.writes == []
    assert m.held(1) and not m.held(0) and m.queued(1) == H
    assert m.resume(1) == [(1, "resume")]
    m.feed(0, H)
    t = m.tick()
    assert t.ready == {0, 1} and t.writes == []
    # the resume of a starved slot writes nothing: it stays held on the device until it is ready
    m.feed(0, H)
    assert m.tick().writes == [(1, "hold")]
    assert not m.held(1)
    assert m.hold(1) == [] and m.held(1)
    assert m.resume(1) == [] and 1 in m.device_held()
    m.feed([0, 1], H)
    assert m.tick().writes == [(1, "resume")]


def test_pad_feed():
    m = model(3, 3 * H)
    m.release(2)
    m.feed([0, 1], 300, [300, 256])
    assert m.pad_feed() == [212, 0, 0] and m.queued() == [512, 256, 0]
    m.feed(1, 1)
    assert m.pad_feed(1) == 255 and m.queued(1) == 512
    assert m.pad_feed([0, 1]) == [0, 0]
    with pytest.raises(Refused):
        m.pad_feed(2)                           # an idle slot, named


def test_refusals_change_nothing():
    m = FeedModel(3, H)
    with pytest.raises(Refused):
        m.feed(0, 10)                           # before enable_feed
    with pytest.raises(Refused):
        m.tick()
    with pytest.raises(Refused):
        m.enable_feed(H - 1)
    m.enable_feed(2 * H)
    with pytest.raises(Refused):
        m.enable_feed(2 * H)                    # once
    m.release(2)
    m.feed([0, 1], 100)

    def state():
        return (m.P, m.queued(), list(m.serial), list(m.starved), list(m.on_device), list(m.caller_held), m.writes)

    before = state()
    for call in (lambda: m.feed([0, 1], 2 * H - 99, [0, 2 * H - 99]),    # overflow of slot 1 alone
                 lambda: m.feed([0, 2], 10),                            # an idle slot
                 lambda: m.feed([0, 0], 10),                            # a slot named twice
                 lambda: m.feed([0, 1], 10, [10, 11]),                  # a count above n
                 lambda: m.feed([0, 1], 10, [-1, 1]),
                 lambda: m.feed(3, 10),                                 # out of range
                 lambda: m.push(H),                                     # a push with a queue
                 lambda: m.finish_stream(0),
                 lambda: m.finish(),
                 lambda: m.tick(0)):
        with pytest.raises(Refused):
            call()
        assert state() == before
    m.clear_feed()
    m.push(100)
    with pytest.raises(Refused):
        m.tick()                                # off the hop grid
    with pytest.raises(Refused):
        m.hold(0)
    m.push(H - 100)
    m.finish()
    with pytest.raises(Refused):
        m.feed(0, 1)


def test_push_after_ticks_resumes_the_starved():
    m = model(3)
    m.feed(0, H)
    assert sorted(m.tick().writes) == [(1, "hold"), (2, "hold")]
    assert sorted(m.push(100)) == [(1, "resume"), (2, "resume")] and m.device_held() == set()
    assert m.push(H - 100) == []


def test_restart_release_and_finish_stream_empty_the_inbox():
    m = model(3)
    m.feed([0, 1, 2], 100)
    m.restart(0)
    m.release(1)
    assert m.queued() == [0, 0, 100] and m.cleared[:2] == [100, 100]
    with pytest.raises(Refused):
        m.feed(1, 1)
    m.clear_feed(2)
    m.finish_stream(2)
    assert not m.live[2]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_invariants_of_a_seeded_run(seed):
    rs = np.random.RandomState(seed)
    S, cap = 5, 5 * H
    m = model(S, cap)
    expect = [0] * S                            # the serial number each slot's next consumed sample has
    for step in range(600):
        r = rs.rand()
        if r < 0.55:
            slots = [s for s in range(S) if rs.rand() < 0.6 and m.live[s]]
            n = int(rs.randint(0, 700))
            counts = [int(rs.randint(0, n + 1)) for _ in slots]
            try:
                m.feed(slots, n, counts)
            except Refused:
                assert any(m.queued(s) + k > cap for s, k in zip(slots, counts))
        elif r < 0.9:
            hops = int(rs.randint(1, 4))
            before = (m.P, m.queued(), list(m.on_device), m.writes)
            t = m.tick(hops)
            if t is None:
                assert (m.P, m.queued(), list(m.on_device), m.writes) == before
                assert not any(m.last_consumed)
                continue
            assert m.P == before[0] + hops * H
            for s in range(S):
                took = s in t.ready
                assert m.last_consumed[s] == took
                assert took == (m.live[s] and not m.caller_held[s] and before[1][s] >= hops * H)
                if took:                        # every consumption is hops * H samples, and the oldest ones
                    assert t.taken[s] == list(range(expect[s], expect[s] + hops * H))
                    expect[s] += hops * H
                else:
                    assert m.queued(s) == before[1][s]
            # the table was written exactly where held-by-either changed
            now = [m.caller_held[s] or m.starved[s] for s in range(S)]
            assert now == m.on_device
            assert sorted(s for s, _ in t.writes) == [s for s in range(S) if now[s] != before[2][s]]
            assert m.writes == before[3] + len(t.writes)
        elif r < 0.94:
            s = int(rs.randint(S))
            if m.live[s]:
                (m.resume if m.caller_held[s] else m.hold)(s)
        elif r < 0.97:
            s = int(rs.randint(S))
            expect[s] += m.queued(s)            # what is cleared is never consumed
            m.clear_feed(s)
        else:
            m.pad_feed()
            assert all(q % H == 0 for q in m.queued())
        for s in range(S):                      # fed = consumed + queued + cleared
            assert m.fed[s] == m.consumed[s] + m.queued(s) + m.cleared[s]
            assert m.queued(s) <= cap
    assert m.P > 100 * H and min(m.consumed) > 20 * H and m.writes > 10
