"""A pure-Python model of the feed scheduler of ``repet.online_streams`` (``enable_feed`` / ``feed`` / ``tick``): queues and their
capacity, who is ready and who is starved at a tick, the hold / resume entries a tick writes to the device table, ``pad_feed``,
``clear_feed`` and every refusal. No audio: a queue holds the serial numbers of the samples a slot was fed (0, 1, 2, ... per
stream), so a test can say which samples a tick consumed. The GPU tests drive a twin handle through ``hold`` / ``resume`` /
``push`` with what this model decides.

The rules (H the hop, P the samples pushed, in samples):
  ready    a live slot the caller does not hold whose queue has at least hops * H samples
  starved  a live slot the caller does not hold that is not ready, at a tick at which somebody is
  a tick with nobody ready changes nothing
  a slot is held ON THE DEVICE while the caller holds it or it is starved; the table is written only where that changes
  a slot the caller holds keeps its starved flag until a tick looks at it again (so a resume of a starved slot writes nothing)
"""


class Refused(ValueError):
    """what the library answers with ValueError / REPET_ERR_BAD_ARG; the model is unchanged"""


class Tick:
    """what one tick did: the slots that were consumed and starved, the table entries written ((slot, "hold" | "resume")) and the
    serial numbers each ready slot's share was made of"""

    def __init__(self, ready, starved, writes, taken):
        self.ready, self.starved, self.writes, self.taken = frozenset(ready), frozenset(starved), list(writes), dict(taken)


class FeedModel:
    def __init__(self, n_slots, hop):
        self.S, self.H = int(n_slots), int(hop)
        self.capacity = 0
        self.P = 0
        self.finished = False
        self.live = [True] * self.S
        self.caller_held = [False] * self.S
        self.starved = [False] * self.S
        self.on_device = [False] * self.S           # what the device table says: held by either
        self.queue = [[] for _ in range(self.S)]
        self.serial = [0] * self.S                  # next serial number of each slot's stream
        self.fed = [0] * self.S
        self.consumed = [0] * self.S
        self.cleared = [0] * self.S
        self.last_consumed = [False] * self.S
        self.writes = 0                             # table entries written so far

    # ---- the table ----
    def _sync(self, slots):
        out = []
        for s in slots:
            want = self.caller_held[s] or self.starved[s]
            if want != self.on_device[s]:
                self.on_device[s] = want
                out.append((s, "hold" if want else "resume"))
        self.writes += len(out)
        return out

    def device_held(self):
        """the live slots a twin handle has to hold for the push that mirrors the next emission"""
        return {s for s in range(self.S) if self.on_device[s]}

    def _slots(self, slots):
        slots = [slots] if isinstance(slots, int) else list(slots)
        for s in slots:
            if not 0 <= s < self.S:
                raise Refused("slot out of range")
        return slots

    def _need_feed(self):
        if self.capacity <= 0:
            raise Refused("no inboxes")
        if self.finished:
            raise Refused("finished")

    # ---- inboxes ----
    def enable_feed(self, capacity):
        if self.finished or self.capacity > 0 or capacity < self.H or self.P % self.H:
            raise Refused("enable_feed")
        self.capacity = int(capacity)

    def queued(self, slot=None):
        return [len(q) for q in self.queue] if slot is None else len(self.queue[slot])

    def feed(self, slots, n, counts=None):
        """rows of n samples for the named slots, of which row i brings counts[i] (None: n). Returns the serial numbers fed per
        slot. All or nothing."""
        self._need_feed()
        slots = self._slots(slots)
        counts = [n] * len(slots) if counts is None else list(counts)
        if len(counts) != len(slots) or len(set(slots)) != len(slots) or n < 0:
            raise Refused("duplicate slot or bad counts")
        for s, k in zip(slots, counts):
            if not self.live[s]:
                raise Refused("idle slot")
            if not 0 <= k <= n:
                raise Refused("count outside [0, n]")
            if len(self.queue[s]) + k > self.capacity:
                raise Refused("overflow")
        fed = {}
        for s, k in zip(slots, counts):
            fed[s] = list(range(self.serial[s], self.serial[s] + k))
            self.queue[s] += fed[s]
            self.serial[s] += k
            self.fed[s] += k
        return fed

    def pad_feed(self, slots=None):
        """the pad counts; the zeros get serial numbers like any sample"""
        self._need_feed()
        named = [s for s in range(self.S) if self.live[s]] if slots is None else self._slots(slots)
        pads = [(-len(self.queue[s])) % self.H for s in named]
        self.feed(named, self.H, pads)
        if slots is None:
            out = [0] * self.S
            for s, k in zip(named, pads):
                out[s] = k
            return out
        return pads[0] if isinstance(slots, int) else pads

    def clear_feed(self, slots=None):
        if self.capacity <= 0:
            raise Refused("no inboxes")
        for s in (range(self.S) if slots is None else self._slots(slots)):
            self.cleared[s] += len(self.queue[s])
            self.queue[s] = []

    # ---- the push ----
    def tick(self, hops=1):
        """None where nobody is ready (nothing changes), else the Tick"""
        self._need_feed()
        if hops < 1 or self.P % self.H:
            raise Refused("off the hop grid")
        n = hops * self.H
        free = [s for s in range(self.S) if self.live[s] and not self.caller_held[s]]
        ready = [s for s in free if len(self.queue[s]) >= n]
        if not ready:
            self.last_consumed = [False] * self.S
            return None
        changed = []
        for s in free:
            want = s not in ready
            if self.starved[s] != want:
                self.starved[s] = want
                changed.append(s)
        writes = self._sync(changed)
        taken = {}
        for s in ready:
            taken[s], self.queue[s] = self.queue[s][:n], self.queue[s][n:]
            self.consumed[s] += n
        self.P += n
        self.last_consumed = [s in ready for s in range(self.S)]
        return Tick(ready, [s for s in free if s not in ready], writes, taken)

    def push(self, n):
        """a plain lockstep push: refused while an inbox holds samples; the starved slots are resumed first"""
        if self.finished or n < 0:
            raise Refused("push")
        if any(self.queue[s] for s in range(self.S)):
            raise Refused("an inbox holds samples")
        if any(self.caller_held) and n % self.H:
            raise Refused("held slots need whole hops")
        was = [s for s in range(self.S) if self.starved[s]]
        for s in was:
            self.starved[s] = False
        writes = self._sync(was)
        self.P += n
        return writes

    # ---- the slots ----
    def hold(self, slots):
        slots = self._slots(slots)
        if self.finished or self.P % self.H or any(not self.live[s] for s in slots):
            raise Refused("hold")
        for s in slots:
            self.caller_held[s] = True
        return self._sync(slots)

    def resume(self, slots):
        slots = self._slots(slots)
        if self.finished or self.P % self.H:
            raise Refused("resume")
        for s in slots:
            self.caller_held[s] = False
        return self._sync(slots)

    def held(self, slot):
        return self.caller_held[slot]

    def _reset(self, slots, live):
        for s in slots:
            self.cleared[s] += len(self.queue[s])
            self.queue[s] = []
            self.live[s] = live
            self.caller_held[s] = self.starved[s] = self.on_device[s] = False     # (the reset launch writes the table itself)

    def restart(self, slots):
        slots = self._slots(slots)
        if self.finished or self.P % self.H:
            raise Refused("restart")
        self._reset(slots, True)

    def release(self, slots):
        slots = self._slots(slots)
        if self.finished:
            raise Refused("release")
        self._reset(slots, False)

    def finish_stream(self, slot):
        (slot,) = self._slots(slot)
        if self.finished or not self.live[slot]:
            raise Refused("idle slot")
        if self.queue[slot]:
            raise Refused("queued samples: clear_feed or pad_feed first")
        self.caller_held[slot] = self.starved[slot] = False
        writes = self._sync([slot])
        self._reset([slot], False)
        return writes

    def finish(self):
        if self.finished:
            raise Refused("finished")
        if any(self.queue[s] for s in range(self.S)):
            raise Refused("queued samples: clear_feed or pad_feed first")
        was = [s for s in range(self.S) if self.on_device[s]]
        for s in was:
            self.caller_held[s] = self.starved[s] = False
        writes = self._sync(was)
        self.finished = True
        return writes
