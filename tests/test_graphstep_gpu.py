"""_graph.CapturedStep and _graph.HostRing on the GPU, on a toy step: one 8-element parameter p, the persistent state acc [8],
step: acc += x * p, out = acc * 2.  Every value is a small integer, so every comparison is exact.  The graph is one chain of
launches on one stream."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _graph
    return _graph


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.arange(1.0, 9.0))


def make(G, dev):
    toy = Toy().to(dev)
    t = dict(x=torch.full((8,), 3.0, device=dev), acc=torch.arange(8.0, device=dev), operand=[object()], steps=0)

    def step():
        t["steps"] += 1
        t["acc"].add_(t["x"] * toy.p)
        return t["acc"] * 2

    captured = G.CapturedStep(step, (toy,), state=lambda: [t["acc"]], derived=lambda: t["operand"])
    return toy, t, captured


def test_a_capture_advances_nothing_and_a_replay_advances_once(G, gpu_device):
    toy, t, captured = make(G, gpu_device)
    assert captured.graph is None and captured.out is None
    before = t["acc"].clone()
    captured.capture(3)
    torch.cuda.synchronize()
    assert t["steps"] == 4                                                  # three warm-up runs and the captured one
    assert torch.equal(t["acc"], before) and isinstance(captured.graph, torch.cuda.CUDAGraph) and not captured.stale()
    p = toy.p.detach()
    for n in (1, 2):
        captured.replay()
        assert torch.equal(t["acc"], before + n * 3.0 * p) and torch.equal(captured.out, 2 * (before + n * 3.0 * p))
    t["x"].fill_(5.0)                                                       # the caller's own static input
    captured.replay()
    assert torch.equal(t["acc"], before + 11.0 * p) and t["steps"] == 4 and not captured.stale()


def test_each_of_the_three_conditions_makes_it_stale_and_a_capture_clears_it(G, gpu_device):
    from deep_visual_slam_amd import nn_ops
    toy, t, captured = make(G, gpu_device)
    captured.capture(1)
    first = captured.graph

    def recapture():
        acc, graph = t["acc"].clone(), captured.graph
        captured.capture(1)
        assert captured.graph is not graph and not captured.stale() and torch.equal(t["acc"], acc)

    assert not captured.stale()
    with torch.no_grad():
        toy.p.add_(1)                                                       # torch's version counter
    assert captured.stale()
    recapture()
    nn_ops.bump_generation()                                                # the library's raw-pointer writers
    assert captured.stale()
    recapture()
    kept = t["operand"][0]
    t["operand"] = [object()]                                               # a derived operand re-made
    assert captured.stale()
    recapture()
    assert captured._derived[0] is t["operand"][0] is not kept and captured.graph is not first
    before = t["acc"].clone()
    captured.replay()                                                       # the new graph reads the new weights
    assert torch.equal(t["acc"], before + 3.0 * toy.p.detach()) and float(toy.p.detach()[0]) == 2.0


def test_without_state_or_derived_objects_only_the_weights_count(G, gpu_device):
    toy = Toy().to(gpu_device)
    x = torch.ones(8, device=gpu_device)
    captured = G.CapturedStep(lambda: x * toy.p, (toy,))
    captured.capture(1)
    captured.replay()
    assert torch.equal(captured.out, toy.p.detach()) and not captured.stale()
    toy.load_state_dict({"p": torch.zeros(8)})
    assert captured.stale()


def test_the_ring_alternates_two_pinned_slots_by_name(G, gpu_device):
    ring = G.HostRing()
    a = torch.arange(6.0, device=gpu_device).view(2, 3)
    b = torch.arange(4, device=gpu_device, dtype=torch.uint8)
    slots = [ring.put(a=a + i, b=b + i, c=None) for i in range(3)]
    for i, slot in enumerate(slots):
        assert slot["a"].is_pinned() and slot["b"].is_pinned() and slot["c"] is None and slot.wait() is slot
        assert slot["a"].dtype == torch.float32 and slot["b"].dtype == torch.uint8 and tuple(slot["a"].shape) == (2, 3)
    assert slots[0] is not slots[1] and slots[2] is slots[0] and slots[0]["event"] is not slots[1]["event"]
    assert torch.equal(slots[1]["a"], a.cpu() + 1) and torch.equal(slots[1]["b"], b.cpu() + 1)       # untouched by the put after it
    assert torch.equal(slots[2]["a"], a.cpu() + 2) and torch.equal(slots[2]["b"], b.cpu() + 2)       # put 0's slot, used again
    again = ring.put(a=a, b=b, c=None)
    assert again is slots[1]
    wide = ring.put(a=torch.zeros(2, 4, device=gpu_device), b=b, c=None)                             # a changed shape: a new ring
    assert all(wide is not s for s in slots) and tuple(wide["a"].shape) == (2, 4) and tuple(slots[1]["a"].shape) == (2, 3)
    other = ring.put(a=torch.zeros(2, 4, device=gpu_device), b=b.int(), c=None)                      # a changed dtype too
    assert other is not wide and other["b"].dtype == torch.int32
    filled = ring.put(a=torch.zeros(2, 4, device=gpu_device), b=b.int(), c=b)                        # None no longer
    assert filled.wait()["c"].is_pinned() and torch.equal(filled["c"], b.cpu())


def test_a_slot_taken_by_hand_is_the_next_in_turn(G, gpu_device):
    ring = G.HostRing()
    count = torch.tensor([2, 1], device=gpu_device, dtype=torch.int32)
    rows = torch.arange(12.0, device=gpu_device).view(2, 3, 2)
    first = ring.put(count=count, rows=rows)
    slot = ring.next(count=count, rows=rows)
    assert slot is not first
    slot["count"].copy_(count, non_blocking=True)
    slot["event"].record()
    for i, c in enumerate(slot.wait()["count"].tolist()):
        slot["rows"][i, :c].copy_(rows[i, :c], non_blocking=True)
    slot["event"].record()
    want = rows.cpu()
    want[0, 2:], want[1, 1:] = 0, 0
    assert torch.equal(slot.wait()["rows"], want) and torch.equal(first.wait()["rows"], rows.cpu())
    assert ring.put(count=count, rows=rows) is first
