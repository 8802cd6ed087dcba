"""tests/golden/conv_small_cases.json is the right list: one tiny case per launch sequence, proven without a GPU.

tests/test_conv_sequences_gpu.py runs the entries of that file on the GPU and compares numbers; this file proves that the
entries stand for what they claim.  For every entry, conv.conv2d and its backward are driven at the SMALL shape with the
recorders of tests/test_conv_routes_cpu.py, and

  * the log equals, string for string, the golden log of the full-size case the entry names (`stands_for`);
  * the union over the entries is exactly the set of deterministic-off logs of conv_routes.json: UNREACHABLE lists what could not
    be reached, with the reason, and is empty;
  * the C entry points, which choose kernels by shape as well, choose at the small shape what they choose at the product's
    (tests/conv_cases.py spells their rules out as plain arithmetic, read from csrc/conv_thin.hip and csrc/conv_fwd.hip): the
    same thin-kernel instance, the split-K form the entry declares -- with a second entry at an unsplit size for every sequence
    whose product-size launch at batch 12 does not split --, a padded-domain data gradient only where it has its three rows and
    columns, a Winograd general gather only where it has two;
  * an entry is marked `refused` exactly where dvs_conv2d_fwd rejects the operands (the ragged concat layer's direct forward,
    which conv.supported() excludes from the product): the GPU test asserts the refusal there, every other entry the numbers.
"""
import pytest

import conv_cases as C
import test_conv_routes_cpu as R

CASES = C.load()
UNREACHABLE = {}            # log -> reason; must stay empty for the fp32 mode (it is empty for both)
_GOLDEN = None


def _golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = C.golden_det0()
    return _GOLDEN


def _twin_batch(e):
    return int(e["stands_for"].split("|")[1][1:])


@pytest.mark.parametrize("e", CASES, ids=[C.entry_id(e) for e in CASES])
def test_entry_runs_the_sequence_it_stands_for(e, monkeypatch):
    golden = _golden()
    layer, batch, precision, det, switch, grads, sink = e["stands_for"].split("|")
    # the full-size case is the same layer in the same mode; only the size and the batch differ
    assert (layer, precision, det, switch, grads, sink) == (e["layer"], e["precision"], "det0", e["switch"], e["grads"], "sink%d" % e["sink"])
    assert e["stands_for"] in golden
    log = C.run_entry(monkeypatch, e)
    assert log == golden[e["stands_for"]]

    cfg, full, fb = C.entry_cfg(e), R.LAYERS[e["layer"]], _twin_batch(e)
    assert cfg["x"][0] == full["x"][0] and (cfg["x2"] == full["x2"] or cfg["x2"][0] == full["x2"][0])     # channels stay
    # thin decoder kernels: the same instance as at the product's size
    assert C.thin_forms(cfg, e["batch"], log) == C.thin_forms(full, fb, log)
    # split-K of the LDS-DMA launches: as declared; an unsplit double runs every launch in the product's batch-12 form
    forms = C.splitk_forms(cfg, e["batch"], precision, log)
    assert forms == e["splitk"]
    if e["double"]:
        assert fb == 12 and forms == C.splitk_forms(full, 12, precision, log) and any(f.endswith(":unsplit") for f in forms)
        assert max(full["w"][:2]) <= 128
        for what, fused in C.direct_launches(cfg, log):
            small, big = C.dma_launch(cfg, e["batch"], precision, what, fused), C.dma_launch(full, 12, precision, what, fused)
            if small is not None and not small["ksplit"] and not (cfg["stats"] & 3 and what == "fwd"):
                assert small["tiles"] >= C.SPLITK_TILES and big["tiles"] >= C.SPLITK_TILES
    # a launch the C entry point refuses: only where conv.supported() keeps the product from ever planning it
    assert e["refused"] == C.refused(cfg, log)
    if e["refused"]:
        import torch
        from deep_visual_slam_amd import conv
        assert not conv.supported(torch.empty((1,) + cfg["x"]), torch.empty(cfg["w"]), x2=torch.empty((1,) + cfg["x2"]))
        assert e["layer"] == "ragged_skip"
    B, ci, H, W, c1, up = C._logical(cfg, e["batch"])
    h, w = cfg["x"][1:]
    if "conv2d_dgrad_padded(" in log:
        assert (h >= 3 and w >= 3) or (up and h >= 2)
    if "wino_gen(" in log or "wino_wgrad_gen(" in log:
        assert H >= 2 and W >= 2


def test_the_entries_cover_every_deterministic_off_sequence_once():
    golden = _golden()
    logs = set(golden.values())
    firsts = [e for e in CASES if not e["double"]]
    reached = [golden[e["stands_for"]] for e in firsts]
    assert len(reached) == len(set(reached)), "two entries for one sequence"
    assert set(reached) | set(UNREACHABLE) == logs and not set(reached) & set(UNREACHABLE)
    assert not [log for log in UNREACHABLE if "conv3x3_p16" not in log], "an fp32 sequence may not be unreachable"
    assert not UNREACHABLE
    print("%d entries for %d sequences, %d unsplit-K doubles, %d unreachable"
          % (len(firsts), len(logs), len(CASES) - len(firsts), len(UNREACHABLE)))


def test_every_sequence_that_runs_unsplit_at_the_products_size_has_an_unsplit_double():
    """A sequence with an LDS-DMA launch that splits K at the tiny size but not in some batch-12 product case on a layer of at
    most 128 channels must have a double, and every double must be such a sequence."""
    golden = _golden()
    tiny = {golden[e["stands_for"]]: e for e in CASES if not e["double"]}
    doubles = {golden[e["stands_for"]] for e in CASES if e["double"]}
    need = set()
    for cid, log in golden.items():
        layer, batch, precision = cid.split("|")[:3]
        full = R.LAYERS[layer]
        if batch != "b12" or max(full["w"][:2]) > 128 or not any(f.endswith(":split") for f in tiny[log]["splitk"]):
            continue
        if any(f.endswith(":unsplit") for f in C.splitk_forms(full, 12, precision, log)):
            need.add(log)
    assert need == doubles, (len(need), len(doubles))
