"""A harness that runs device entries the way they are advertised: on a side stream, captured into a graph, and
replayed over new contents of the same arrays and a workspace another batch left behind.

``replay(run, X, Y, works)`` takes a callable ``run(a)`` that makes the calls under test on torch's current stream
(``a``: name -> tensor for every input, in-place array, output and workspace) and two batches of
stream_pairs_helper that agree in every by-value argument and array size.  It then

1. allocates every array once, between guards (gpu_guard.Guarded); a workspace of its ``*_work`` size plus 16 bytes
   that the call is not told about;
2. loads X, fills the outputs and the workspaces with poison;
3. runs ``run`` eagerly on a side stream ``s``, synchronises ``s`` alone and compares everything with X's reference
   (this is the side-stream test, and it loads the code objects before any capture);
4. captures ``run`` once on ``s`` (one stream, no fork or join; capture_error_mode "thread_local", as bench.py does);
5. loads Y into the same arrays, poisons the outputs again and the workspaces with another byte, replays,
   synchronises ``s`` and compares everything with Y's reference;
6. loads X again and poisons the outputs only — the workspaces stay as Y's replay left them — replays and
   compares with X's reference.

Every comparison is over whole arrays, byte for byte, the only bytes left out those a family's own mask_slack rule
leaves out (``Batch.slack``); the guards, the 16 bytes behind every workspace and the inputs must be unchanged.

Why this finds what the default stream hides:
* a launch or memset that went to another stream than the one it was given is not part of the capture (in
  thread_local mode the null stream is not captured and does not wait for ``s``), so a replay over poisoned outputs
  leaves poison, a stale table or a stale count behind; in the eager step it races the side stream;
* a synchronisation or a read of device memory on the host is not permitted while a stream captures: the capture
  itself fails;
* a value the host baked into the launch sequence from X's data (a count, a grid size, an id) is wrong under Y, whose
  every array and counter differs from X's (test_stream_pairs_ref.py);
* state a call needs from its workspace but does not initialise itself is Y's in step 6, and poison of another
  byte than the first run's in step 5.

Tensors a wrapper allocates during the capture (``run`` returns them, name -> tensor) belong to the graph's pool:
the harness keeps them for the graph's lifetime and poisons them before each replay.  Their memory may be that of
a temporary the wrapper freed earlier in the same capture (a workspace of an earlier call of a chain), which the
replay writes again after the poison, and in the eager step they start as whatever ``torch.empty`` gave: so of
such a tensor the bytes the reference leaves at poison are not compared, every other byte is.
"""
import numpy as np
import torch

from gpu_guard import DEV, FILL, Guarded
from stream_pairs_helper import POISON

assert POISON == FILL
WORK_POISON = (0xEE, 0x5A)  # the workspaces' fill before the eager run, and before Y's replay
TAIL = 16                   # bytes behind a workspace that the call is not told about
_TORCH = {np.dtype("<u2"): torch.int16, np.dtype("<u4"): torch.int32, np.dtype("<u8"): torch.int64, np.dtype("<i8"): torch.int64}


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _flat(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


class Arrays:
    """The device arrays of one pair of batches, allocated once: ``ins`` / ``io`` / ``out`` / ``work`` hold a Guarded
    each, ``stage`` the two batches' inputs and in-place arrays on the device (so that loading one is a copy on the
    stream, nothing the host waits for)."""

    def __init__(self, X, Y, works, held=()):
        assert X.args == Y.args, "the batches differ in a by-value argument"
        self.batches = (X, Y)
        mk = lambda a: Guarded(a.nbytes, dtype=_TORCH.get(a.dtype, torch.uint8))  # noqa: E731
        for role in ("ins", "io", "want"):
            assert {k: a.nbytes for k, a in getattr(X, role).items()} == {k: a.nbytes for k, a in getattr(Y, role).items()}, role
        self.ins = {k: mk(a) for k, a in X.ins.items()}
        self.io = {k: mk(a) for k, a in X.io.items()}
        self.out = {k: mk(a) for k, a in X.want.items() if k not in X.io and k not in held}
        self.work = {k: Guarded(-(-n // 8) * 8 + TAIL) for k, n in works.items()}
        self.work_bytes = {k: -(-n // 8) * 8 for k, n in works.items()}
        self.work_fill = WORK_POISON[0]
        self.stage = [{k: torch.from_numpy(_bytes(a).copy()).to(DEV) for k, a in {**b.ins, **b.io}.items()} for b in (X, Y)]
        torch.cuda.synchronize()                      # the allocations and their fills ran on the default stream

    def tensors(self):
        """name -> tensor, as ``run`` gets them: typed like the batch's arrays (records as uint8), the workspaces
        uint8 and without their tail (their sizes rounded up to 8 bytes, for the wrappers that take int64)."""
        a = {k: g.t for d in (self.ins, self.io, self.out) for k, g in d.items()}
        for k, g in self.work.items():
            a[k] = g.t[:self.work_bytes[k]]
        return a

    @staticmethod
    def _inner(g):
        return g.big[g.g:g.g + g.n]

    def load(self, which, work_fill=None, held=None):
        """Batch ``which`` (0: X, 1: Y) into the inputs and in-place arrays, poison into every output (and into the
        workspaces with ``work_fill``), all on the current stream."""
        for k, g in {**self.ins, **self.io}.items():
            self._inner(g).copy_(self.stage[which][k], non_blocking=True)
        for g in self.out.values():
            self._inner(g).fill_(POISON)
        for t in (held or {}).values():
            _flat(t).fill_(POISON)
        if work_fill is not None:
            self.work_fill = work_fill
            for g in self.work.values():
                self._inner(g).fill_(work_fill)

    def snapshot(self, held=None):
        """Copies of everything a check reads, made on the current stream."""
        snap = {k: g.big.clone() for d in (self.ins, self.io, self.out, self.work) for k, g in d.items()}
        return snap, {k: _flat(t).clone() for k, t in (held or {}).items()}, self.work_fill

    def check(self, which, tag, held=None, snap=None):
        """Everything against batch ``which``: outputs and in-place arrays against its reference, the inputs
        unchanged, every guard and workspace tail intact.  ``snap``: a snapshot to check in place of the arrays."""
        b = self.batches[which]
        bigs, held, work_fill = snap if snap is not None else ({k: g.big for d in (self.ins, self.io, self.out, self.work)
                                                                for k, g in d.items()},
                                                               {k: _flat(t) for k, t in (held or {}).items()}, self.work_fill)
        host = {}
        for d in (self.ins, self.io, self.out, self.work):
            for k, g in d.items():
                big = bigs[k].cpu().numpy()
                assert (big[:g.g] == FILL).all() and (big[g.g + g.n:] == FILL).all(), f"{tag}: written outside {k}"
                host[k] = big[g.g:g.g + g.n]
        for k, n in self.work_bytes.items():
            assert (host[k][n:] == work_fill).all(), f"{tag}: written behind the {n} bytes of {k}"
        for k, a in b.ins.items():
            assert np.array_equal(host[k], _bytes(a)), f"{tag}: input {k} was written"
        for k, w in b.want.items():
            w = _bytes(w)
            if k in held:
                got = held[k].cpu().numpy()[:w.size]
                skip = w == POISON                      # (what the call leaves unwritten: see the module docstring)
            else:
                got, skip = host[k], np.zeros(w.size, bool)
            assert got.size == w.size, (tag, k, got.size, w.size)
            if k in b.slack:
                skip = skip | b.slack[k]
            bad = np.flatnonzero((got != w) & ~skip)
            assert bad.size == 0, (tag, k, bad.size, [(int(i), int(got[i]), int(w[i])) for i in bad[:6]])


def replay(run, X, Y, works, held=()):
    """Steps 1-6 of the module docstring for ``run`` over the pair (X, Y).  ``works``: name -> bytes of each
    workspace (the entry's own ``*_work`` size); ``held``: the outputs a wrapper allocates itself (``run`` returns
    them)."""
    arr = Arrays(X, Y, works, held)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        arr.load(0, WORK_POISON[0])
        got = run(arr.tensors()) or {}
    s.synchronize()
    assert set(got) == set(held), (sorted(got), sorted(held))
    arr.check(0, "eager on a side stream", got)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        kept = run(arr.tensors()) or {}            # allocated from the graph's pool: alive as long as `kept` and `graph`
    for which, tag, work_fill in ((1, "replay over Y", WORK_POISON[1]), (0, "replay over X and the workspace Y left", None)):
        with torch.cuda.stream(s):
            arr.load(which, work_fill, kept)
            graph.replay()
        s.synchronize()
        arr.check(which, tag, kept)
    del graph, kept


def concurrent(lanes, rounds=4):
    """Eager runs of several families at once.  ``lanes``: one list of jobs ``(run, X, Y, works)`` per side stream, all
    of the same length; job p of every lane runs X, Y, X, ... for ``rounds`` rounds on its lane's stream with arrays of
    its own, the lanes taking turns to enqueue, then job p + 1.  Every round's results are copied aside on the
    lane's stream.  One synchronize at the end; then every copy is compared with its reference."""
    streams = [torch.cuda.Stream() for _ in lanes]
    arrays = [[Arrays(X, Y, works) for _, X, Y, works in jobs] for jobs in lanes]
    snaps = {}
    for p in range(len(lanes[0])):
        for r in range(rounds):
            for j, jobs in enumerate(lanes):
                arr = arrays[j][p]
                with torch.cuda.stream(streams[j]):
                    arr.load(r & 1, WORK_POISON[r & 1] if r < 2 else None)   # later rounds: over what the round before left
                    got = jobs[p][0](arr.tensors())
                    assert not got, "pass every output in: the results are copied aside"
                    snaps[j, p, r] = arr.snapshot()
    torch.cuda.synchronize()
    for (j, p, r), snap in snaps.items():
        arrays[j][p].check(r & 1, f"stream {j}, job {p}, round {r}", snap=snap)
