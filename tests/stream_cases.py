"""Harness of tests/test_gpu_streams.py: every stream-taking entry point on a
stream the caller created -- TEST INFRASTRUCTURE ONLY.

On the legacy null stream an internal launch that forgets its stream
argument, a graph launched on the wrong stream, a fork event recorded on the
wrong stream and a missing wait on the handle's last event all give the right
answer, because everything is ordered there anyway.  The tests therefore run
each call on a torch.cuda.Stream() of their own, behind work that keeps that
stream busy while the call is issued:

  delayed(stream, ms)   a chain of matmuls on `stream` lasting about `ms`
                        (calibrated once per stream with events recorded on
                        it); returns an event recorded behind the chain
  streams()             two user streams for which the control holds: while
                        delayed(s1, ...) is pending, a trivial kernel on the
                        null stream and one on s2 both complete.  With few
                        hardware queues two streams can share one and then
                        serialise by accident, so up to four streams are
                        tried; no passing pair is a failure that names this
                        cause, never a skip and never a pass
  behind_delay(...)     the pattern of every test: synchronise, enqueue the
                        delay, enqueue the copies that produce the real
                        inputs (into buffers that hold NaN until then) on the
                        user stream, issue the library call at once, assert
                        that the delay was still pending (conclusiveness),
                        wait for the stream

The delay of a call is at least FACTOR times the host wall clock of the same
call on the idle null stream (call_ms, measured by the test on a twin handle
in the same state), and at least MIN_DELAY_MS: host enqueue time jitters on a
shared machine, and a case whose delay ran out before the call returned would
prove nothing (it fails as inconclusive).  LOG keeps (label, call ms, delay
ms) of every call for the records in DESIGN.md.

Only public torch API is used (streams, events, torch.mm).
"""
import math
import time

FACTOR = 5.0            # delay >= FACTOR x the call's host time on the idle null stream
MIN_DELAY_MS = 20.0     # ... and at least this: >= FACTOR x any call below 4 ms
CONTROL_MS = 20.0       # the delay the control runs behind
MAT_N = 2048            # one link of the chain: a 2048^3 fp32 matmul
LOG = []                # (label, call_ms, delay_ms)

_state = {}


class Inconclusive(AssertionError):
    """The delay had run out when the call was issued / returned."""


class NoIndependentStreams(AssertionError):
    """No pair of user streams passed the control."""


def _torch():
    import torch
    return torch


def _chain(stream):
    """(a, b, out, ms per matmul) of `stream`: operands shared, one output per
    stream, the time per link measured with events on that stream."""
    torch = _torch()
    key = ('chain', stream.cuda_stream)
    if key not in _state:
        if 'ab' not in _state:
            g = torch.Generator(device='cuda').manual_seed(1)
            _state['ab'] = tuple(torch.rand(MAT_N, MAT_N, device='cuda', dtype=torch.float32, generator=g) / MAT_N
                                 for _ in range(2))
        a, b = _state['ab']
        out = torch.empty_like(a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            for _ in range(4):                      # library start-up, workspace of this stream
                torch.mm(a, b, out=out)
            stream.synchronize()
            e0.record(stream)
            for _ in range(16):
                torch.mm(a, b, out=out)
            e1.record(stream)
        e1.synchronize()
        _state[key] = (a, b, out, max(e0.elapsed_time(e1) / 16.0, 1e-3))
    return _state[key]


def delayed(stream, ms):
    """Keep `stream` busy for about `ms`; the event recorded behind that work."""
    torch = _torch()
    a, b, out, per = _chain(stream)
    n = max(1, int(math.ceil(ms / per)))
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(n):
            torch.mm(a, b, out=out)
        ev.record(stream)
    return ev


def _control(s1, s2, ms=CONTROL_MS):
    """While delayed(s1, ms) is pending, a trivial kernel on the null stream
    and one on s2 both complete."""
    torch = _torch()
    t0, t2 = _state.setdefault('ticks', tuple(torch.zeros(8, device='cuda') for _ in range(2)))
    torch.cuda.synchronize()
    null = torch.cuda.default_stream()
    ev = delayed(s1, ms)
    e0, e2 = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(null):
        t0.add_(1.0)
        e0.record(null)
    with torch.cuda.stream(s2):
        t2.add_(1.0)
        e2.record(s2)
    ok = False
    while not ev.query():
        if e0.query() and e2.query():
            ok = not ev.query()
            break
    torch.cuda.synchronize()
    return ok


def streams():
    """(s1, s2): user streams that pass the control in both directions, chosen
    once per session out of up to four and checked again (s1 busy, s2 and the
    null stream free) at every call."""
    torch = _torch()
    if 'pair' not in _state:
        cands = [torch.cuda.Stream() for _ in range(4)]
        for s in cands:
            _chain(s)
        found = None
        for i in range(len(cands)):
            for j in range(i + 1, len(cands)):
                if found is None and _control(cands[i], cands[j]) and _control(cands[j], cands[i]):
                    found = (cands[i], cands[j])
        _state['pair'] = found
    pair = _state['pair']
    if pair is None or not _control(pair[0], pair[1]):
        raise NoIndependentStreams(
            'stream control failed: no two of four torch.cuda.Stream() objects ran independently of each other and '
            'of the null stream (a kernel behind a %g ms delay on one held up the others; streams sharing a '
            'hardware queue?) -- the stream tests cannot tell a mis-streamed launch from a right one here'
            % CONTROL_MS)
    return pair


def host_ms(call):
    """Host wall clock of call() on an idle device, in ms (the device is
    synchronised before and after; the time is the call's own)."""
    torch = _torch()
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    dt = (time.perf_counter() - t) * 1e3
    torch.cuda.synchronize()
    return dt


def delay_for(call_ms):
    return max(FACTOR * call_ms, MIN_DELAY_MS)


def behind_delay(label, stream, call_ms, fill, call, sync_inside=False, wait=True):
    """The pattern: device idle; delay on `stream`; fill() enqueues the copies
    that produce the inputs, on `stream`; call() follows at once.  The delay's
    event must still be unfinished when an asynchronous call returns, or
    immediately before a call that synchronises inside (sync_inside).
    Returns the delay's event; wait=False leaves the stream running."""
    torch = _torch()
    ms = delay_for(call_ms)
    LOG.append((label, call_ms, ms))
    print('STREAMS %-44s call %8.3f ms  delay %8.1f ms' % (label, call_ms, ms))
    torch.cuda.synchronize()
    ev = delayed(stream, ms)
    with torch.cuda.stream(stream):
        fill()
    if sync_inside:
        pending = not ev.query()
        call()
    else:
        call()
        pending = not ev.query()
    if wait:
        stream.synchronize()
    if not pending:
        raise Inconclusive('%s: the %.1f ms delay (%.1f x the call\'s %.3f ms on the idle null stream) was over %s: '
                           'the call was not issued behind pending work, the case proves nothing'
                           % (label, ms, ms / max(call_ms, 1e-9), call_ms,
                              'before the call' if sync_inside else 'when the call returned'))
    return ev
