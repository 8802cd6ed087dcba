"""_graph.CapturedStep without a device: an owner that keeps its holder and hands it its own methods must die by reference count.
A dead cycle that holds a captured graph is freed by the cyclic collector whenever that runs -- on the MI355X it ran inside a later
stream's capture, where destroying a graph aborts the process -- so the holder keeps bound methods weakly."""
import gc
import weakref

import pytest
import torch

from deep_visual_slam_amd import _graph, inference, raft, raft_video


class Owner:
    def __init__(self):
        self.calls = []
        self.captured = _graph.CapturedStep(self.step, (), state=self.state, derived=self.derived)

    def step(self):
        self.calls.append("step")
        return 7

    def state(self):
        return []

    def derived(self):
        return [self]


@pytest.fixture
def no_collector():
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


def test_the_holder_calls_its_owners_methods_and_does_not_keep_the_owner_alive(no_collector):
    owner = Owner()
    held = owner.captured
    assert held.step() == 7 and held.state() == [] and held.derived() == [owner] and owner.calls == ["step"]
    ref = weakref.ref(owner)
    del owner
    assert ref() is None                                                    # no collector ran: the reference count alone


def test_plain_callables_and_defaults_are_kept_as_they_are():
    step = lambda: 3
    held = _graph.CapturedStep(step, ())
    assert held.step is step and held.state() == [] and held.derived() == [] and held.graph is None and held.out is None


def test_a_dead_owner_a_builtins_method_and_a_closure(no_collector):
    held = _graph.CapturedStep(Owner().step, ())                            # nobody keeps the owner
    with pytest.raises(_graph.DvsError, match="Owner.step is gone"):
        held.step()
    items = [3, 1]
    held = _graph.CapturedStep(items.copy, (), derived=items.copy)          # __self__ without __func__: kept as it is
    assert held.step() == [3, 1] and held.derived() == [3, 1]


def test_the_streams_hand_the_holder_bound_methods_only(no_collector):
    """Every user builds its holder where a device is needed (a first push, a constructor that captures), so this reads the
    source of those places -- every argument of CapturedStep( is an attribute of self, no lambda, no partial -- and then pins, on
    objects made by hand, that holders built from exactly those methods leave no cycle."""
    import inspect
    import re
    for fn in (raft_video.FlowStream._allocate, inference.Graphed.__init__, inference.FramePredictor.__init__):
        calls = re.findall(r"CapturedStep\((.*)\)", inspect.getsource(fn))
        assert len(calls) == 1, fn.__qualname__
        step, _, rest = calls[0].partition(", (")
        assert re.fullmatch(r"self\._\w+", step), (fn.__qualname__, step)
        assert re.findall(r"(\w+)=([^,]+)", rest) == [(k, v) for k, v in re.findall(r"(state|derived)=(self\._\w+)", rest)], rest
        assert "lambda" not in calls[0] and "partial" not in calls[0]
    assert "CapturedStep(" not in inspect.getsource(inference.CloudPredictor)   # it is FramePredictor's
    stream = raft_video.FlowStream(raft.SmallRAFT())
    held = _graph.CapturedStep(stream._graph_step, (stream.model,), state=stream._state, derived=stream._derived)
    stream._captured = held
    ref = weakref.ref(stream)
    del stream
    assert ref() is None
    for cls in (inference.Graphed, inference.FramePredictor, inference.CloudPredictor):
        assert callable(cls._step) and "lambda" not in cls._step.__qualname__
        obj = cls.__new__(cls)
        obj._captured = _graph.CapturedStep(obj._step, (), state=getattr(obj, "_state", None))
        ref = weakref.ref(obj)
        del obj
        assert ref() is None, cls.__name__
