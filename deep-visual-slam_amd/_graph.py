"""What every captured HIP graph and every asynchronous host copy in this package shares:

    CapturedStep(step, nets, state, derived)   one graph of step(), and everything that decides whether replaying it is still right
    HostRing()                                 two alternating slots of pinned host tensors, addressed by name, an event each
"""
import weakref

import torch

from . import nn_ops
from ._lib import DvsError


def _fold_snapshot():
    """(generation, references to every folded-BatchNorm tensor currently cached).  A captured graph holds raw pointers to
    those tensors; nn_ops._fold_cache may replace an entry later (new weights, optimiser step) and the old tensors would
    be freed under the graph -- the holder keeps them alive, the generation tells a replay that they are stale."""
    return nn_ops.generation(), [(w, b) for (_, w, b) in nn_ops._fold_cache.values()]


class _WeightsWatch:
    """torch-visible modification state of every parameter / buffer of some networks (in-place torch updates,
    load_state_dict bump `_version`).  One attribute read per tensor and replay: ~25 us for both networks."""

    def __init__(self, *nets):
        self.tensors = [t for net in nets for t in list(net.parameters()) + list(net.buffers())]
        self.seen = self.versions()

    def versions(self):
        return sum(t._version for t in self.tensors)

    def changed(self):
        return self.versions() != self.seen


def _weakly(fn):
    """`fn`, held weakly where it is a bound method (None: nothing to name).  An owner keeps its CapturedStep and hands it its own
    methods; held strongly that is a reference cycle, which only the cyclic collector frees, at a time of its choosing -- inside
    a later capture, where destroying a graph aborts the process."""
    if fn is None:
        return lambda: []
    if not (hasattr(fn, "__self__") and hasattr(fn, "__func__")):           # a function, a closure, a builtin's method
        return fn
    ref, name = weakref.WeakMethod(fn), fn.__qualname__

    def call():
        method = ref()
        if method is None:
            raise DvsError("CapturedStep: the owner of %s is gone; the holder keeps its owner's methods weakly" % name)
        return method()
    return call


class CapturedStep:
    """step() -- no arguments, issues the launches, returns the static outputs -- as one HIP graph.  nets: the networks whose
    weights and buffers the graph reads; state(): the persistent tensors step() advances in place; derived(): objects the graph
    points into and that their owner may re-make (cached operands).  Knows nothing of frames, shapes or static inputs: the caller
    fills its own static buffers, then replay()s and reads `out`."""

    def __init__(self, step, nets, state=None, derived=None):
        self.step, self.nets = _weakly(step), tuple(nets)
        self.state, self.derived = _weakly(state), _weakly(derived)
        self.graph, self.out = None, None

    @torch.no_grad()
    def capture(self, runs):
        """`runs` warm-up steps on a side stream (lazy initialisation, the fold cache), then the capture.  Neither advances
        anything: what state() names is put back."""
        saved = [t.clone() for t in self.state()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(runs):
                self.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self.step()
        self._gen, self._held = _fold_snapshot()
        self._watch = _WeightsWatch(*self.nets)
        self._derived = self.derived()                      # the graph points into these: kept alive, compared in stale()
        for t, s in zip(self.state(), saved):
            t.copy_(s)

    def stale(self):
        """True when the library's raw-pointer writers ran (nn_ops.generation()), a weight or buffer changed under torch, or a
        derived object was re-made since the capture: the graph must be captured again, never replayed."""
        return (self._gen != nn_ops.generation() or self._watch.changed()
                or any(a is not b for a, b in zip(self.derived(), self._derived)))

    def replay(self):
        self.graph.replay()


class HostSlot(dict):
    """name -> pinned host tensor (None for a tensor that was None), and "event", recorded behind the copies."""

    def wait(self):
        self["event"].synchronize()
        return self


class HostRing:
    """Two HostSlots used in turn, so that the host views of one put stay valid until the put after next.  Allocated from the
    device tensors it is first given, and again when a shape or dtype changes."""

    def __init__(self):
        self._slots, self._like, self._n = None, None, 0

    def next(self, **tensors):
        """The next slot, shaped like `tensors`, for a caller that copies by hand and records slot["event"] itself."""
        like = {k: None if t is None else (tuple(t.shape), t.dtype) for k, t in tensors.items()}
        if like != self._like:
            pin = lambda d: None if d is None else torch.zeros(d[0], dtype=d[1], pin_memory=True)
            self._slots = [HostSlot({k: pin(d) for k, d in like.items()}, event=torch.cuda.Event()) for _ in range(2)]
            self._like = like
        self._n += 1
        return self._slots[self._n & 1]

    def put(self, **tensors):
        """Copy every tensor that is not None into the next slot (non_blocking), record its event, return the slot."""
        slot = self.next(**tensors)
        for k, t in tensors.items():
            if t is not None:
                slot[k].copy_(t, non_blocking=True)
        slot["event"].record()
        return slot
