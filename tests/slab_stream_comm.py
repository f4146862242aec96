"""A stream-ordered, in-process transport for the slab engine: a test double for slab.TorchComm
that behaves like RCCL rather than like host-staged gloo.

The W ranks of a test run as W threads of ONE process on one GPU.  A rank's host never waits
for device work: an operation only waits, on the host, until the neighbour thread has POSTED
the matching operation.  Posted operations are matched first-in first-out per edge, direction
and traffic class (causal states, anticausal states, stencil planes).  Data dependencies travel
as HIP events only:

  * a send records an event on the sender's current stream (the sweep that wrote the buffer);
  * a receive records an event on the receiver's current stream (the engine posts receives
    from its `post[d]` streams, behind the sweep that last read the buffer);
  * the copy runs on a stream owned by the transport, after both events;
  * `_Xfer.wait()` of either side makes the caller's CURRENT stream wait for the copy's event --
    the receive before its sweep reads the state, the send before a sweep rewrites the buffer.

`halo()` exchanges its planes the same way and waits for its transfers at once, on the caller's
stream: the engine's halo contract is blocking with respect to the bulk stream.

Why this cannot deadlock on the device, whatever the number of hardware queues.  No stream is
ever made to wait for an event before the work that records it has been enqueued: the sender's
and the receiver's events are recorded before their operation is posted, the copy is enqueued
only once both are posted, and a waiter blocks its host until the copy (and its event) has been
enqueued.  So every wait refers to work submitted EARLIER in host time.  Each hardware queue runs
in submission order, hence the oldest unfinished piece of work never waits for anything
unfinished, and all work completes however the runtime maps streams onto shared in-order
queues.  (HIP treats a wait on an event that has not been recorded yet as a no-op; the rule also
keeps the double itself free of that race.)  Nothing here sets a runtime variable.

A failure must not become a hang: every host-side wait for a match times out with a message that
names the rank, the direction and the item, and `abort()` wakes every waiter at once.

On CPU tensors (no events) the copy runs on the host when the match is made, and a wait returns
once it has.
"""
import collections
import threading


class TransportError(RuntimeError):
    pass


class Hub:
    """The mailboxes shared by the rank threads of one run."""

    def __init__(self, world, timeout=30.0):
        self.world, self.timeout = world, timeout
        self.cv = threading.Condition()
        self.sends = collections.defaultdict(collections.deque)   # (src, dst, cls) -> posted sends
        self.recvs = collections.defaultdict(collections.deque)   # (src, dst, cls) -> posted receives
        self.counts = collections.Counter()                       # operations posted per (side, key)
        self.copy_streams = {}
        self.failed = None

    def abort(self, exc):
        with self.cv:
            if self.failed is None:
                self.failed = exc
            self.cv.notify_all()

    def _stream(self, key, device):
        import torch
        s = self.copy_streams.get(key)
        if s is None:
            s = self.copy_streams[key] = torch.cuda.Stream(device)
        return s

    def post(self, side, key, op):
        """side 'send' or 'recv'; op an _Op.  Matches FIFO with the other side's queue."""
        with self.cv:
            op.item = self.counts[(side, key)]
            self.counts[(side, key)] += 1
            mine, other = (self.sends, self.recvs) if side == "send" else (self.recvs, self.sends)
            if other[key]:
                peer = other[key].popleft()
                snd, rcv = (op, peer) if side == "send" else (peer, op)
                if snd.item != rcv.item:
                    raise TransportError("%s: send %d matched with receive %d" % (key, snd.item, rcv.item))
                self._copy(key, snd, rcv)
                self.cv.notify_all()
            else:
                mine[key].append(op)

    def _copy(self, key, snd, rcv):
        if snd.buf.shape != rcv.buf.shape or snd.buf.dtype != rcv.buf.dtype:
            raise TransportError("%s item %d: sent %s %s into %s %s" % (key, snd.item, tuple(snd.buf.shape),
                                                                       snd.buf.dtype, tuple(rcv.buf.shape),
                                                                       rcv.buf.dtype))
        if snd.event is None:          # CPU tensors: nothing runs ahead
            rcv.buf.copy_(snd.buf)
            done = True
        else:
            import torch
            s = self._stream(key, snd.buf.device)
            s.wait_event(snd.event)
            s.wait_event(rcv.event)
            with torch.cuda.stream(s):
                rcv.buf.copy_(snd.buf, non_blocking=True)
            done = torch.cuda.Event()
            done.record(s)
        snd.done = rcv.done = done

    def wait_match(self, op, what):
        with self.cv:
            self.cv.wait_for(lambda: op.done is not None or self.failed is not None, self.timeout)
            if op.done is None:
                if self.failed is not None:
                    raise TransportError("%s: aborted (%s)" % (what, self.failed))
                raise TransportError("%s: no matching operation posted within %g s" % (what, self.timeout))
            return op.done


class _Op:
    def __init__(self, buf, event):
        self.buf, self.event, self.done, self.item = buf, event, None, None


class _StreamXfer:
    """slab._Xfer's interface: wait() makes the current stream wait for the copy."""

    def __init__(self, hub, op, what):
        self.hub, self.op, self.what = hub, op, what

    def wait(self):
        if self.op is None:
            return
        done = self.hub.wait_match(self.op, self.what + " item %d" % self.op.item)
        if done is not True:
            import torch
            torch.cuda.current_stream(self.op.buf.device).wait_event(done)
        self.op = None


class StreamComm:
    """The per-rank face of a Hub, with slab.TorchComm's interface."""

    per_class = True

    def __init__(self, hub, rank):
        self.hub, self.rank, self.world = hub, rank, hub.world

    def _event(self, buf):
        if buf.device.type != "cuda":
            return None
        import torch
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(buf.device))
        return e

    def _post(self, side, buf, peer, cls):
        key = (self.rank, peer, cls) if side == "send" else (peer, self.rank, cls)
        op = _Op(buf, self._event(buf))
        self.hub.post(side, key, op)
        return _StreamXfer(self.hub, op, "rank %d %s %s rank %d (%s)" % (
            self.rank, side, "to" if side == "send" else "from", peer, cls))

    # causal states travel up (r -> r+1), anticausal states down (r -> r-1)
    def isend_up(self, buf):
        return self._post("send", buf, self.rank + 1, "causal")

    def irecv_up(self, buf):
        return self._post("recv", buf, self.rank - 1, "causal")

    def isend_down(self, buf):
        return self._post("send", buf, self.rank - 1, "anticausal")

    def irecv_down(self, buf):
        return self._post("recv", buf, self.rank + 1, "anticausal")

    def halo(self, first_planes, last_planes, lo_halos, hi_halos):
        xs = []
        for nb, snd, rcv in ((self.rank - 1, first_planes, lo_halos),
                             (self.rank + 1, last_planes, hi_halos)):
            if nb < 0 or nb >= self.world:
                continue
            for s, r in zip(snd, rcv):
                xs.append(self._post("send", s, nb, "halo"))
                xs.append(self._post("recv", r, nb, "halo"))
        for x in xs:
            x.wait()


def run_threads(world, body, join_timeout=90.0, hub_timeout=30.0):
    """body(rank, hub) in one thread per rank; re-raises the first failure, never hangs."""
    hub = Hub(world, hub_timeout)
    errors = [None] * world

    def main(r):
        try:
            body(r, hub)
        except BaseException as exc:  # noqa: BLE001 -- handed to the test thread
            errors[r] = exc
            hub.abort("rank %d failed: %r" % (r, exc))

    threads = [threading.Thread(target=main, args=(r,), daemon=True, name="rank%d" % r) for r in range(world)]
    import time
    for t in threads:
        t.start()
    deadline = time.monotonic() + join_timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    first = next((e for e in errors if e is not None and not isinstance(e, TransportError)), None)
    first = first or next((e for e in errors if e is not None), None)
    if first is not None:
        raise first
    if alive:
        hub.abort("join timed out")
        raise TransportError("rank threads still running after %g s: %s" % (join_timeout, alive))
    return hub
