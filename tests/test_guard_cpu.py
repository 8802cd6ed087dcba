"""tests/guard.py proves itself on the CPU: a clean use passes, and each kind of stray access -- made here with plain
torch indexing into the backing buffer, never by a kernel -- is caught and located."""
import types

import pytest
import torch

import guard


def _raw(band, dtype):
    """The whole backing buffer as `dtype` words plus the index of the tensor's first element (front is a multiple of 256)."""
    size = torch.empty((), dtype=dtype).element_size()
    return band.buf[:band.buf.numel() // size * size].view(dtype), band.front // size


def test_clean_use_passes_and_layout_is_kept():
    t, band = guard.guarded_empty((2, 5, 3, 7), torch.float32, "cpu", memory_format=torch.channels_last)
    assert t.shape == (2, 5, 3, 7) and t.is_contiguous(memory_format=torch.channels_last)
    assert t.data_ptr() % 16 == 0 and band.front % 256 == 0
    assert band.front >= guard.MIN_PAD and band.back >= guard.MIN_PAD
    t.copy_(torch.randn(2, 5, 3, 7))
    t += 1.0
    band.check()
    src = torch.randn(3, 4, 6, 5).contiguous(memory_format=torch.channels_last)
    p, b2 = guard.place(src, guard.POISON)
    assert p.stride() == src.stride() and p.dtype == src.dtype and torch.equal(p, src)
    b2.check()
    perm = torch.randn(2, 3, 4, 5).permute(0, 2, 3, 1)              # a dense layout that is neither
    p, b3 = guard.place(perm)
    assert p.stride() == perm.stride() and torch.equal(p, perm)
    b3.check()
    e, b4 = guard.guarded_empty((0, 4), torch.float32)
    assert e.numel() == 0
    b4.check()


def test_band_width_is_two_rows_or_64k():
    t, band = guard.guarded_empty((1, 512, 4, 100), torch.float32, "cpu", memory_format=torch.channels_last)
    assert band.back >= 2 * 100 * 512 * 4 and band.front >= 2 * 100 * 512 * 4
    t, band = guard.guarded_empty((7,), torch.uint8)
    assert band.back == guard.MIN_PAD and band.front == guard.MIN_PAD


def test_store_one_float_past_the_end():
    t, band = guard.guarded_empty((1, 3, 5, 7), torch.float32, "cpu", memory_format=torch.channels_last, pattern=guard.CANARY)
    t.zero_()
    assert t.numel() % 4 != 0
    raw, first = _raw(band, torch.float32)
    raw[first + t.numel()] = 2.5
    with pytest.raises(guard.GuardError) as e:
        band.check()
    assert e.value.side == "back" and e.value.offset == t.numel() * 4 and 1 <= e.value.count <= 4


def test_add_one_float_before_the_start():
    t, band = guard.guarded_empty((33,), torch.float32, pattern=guard.CANARY)
    t.zero_()
    raw, first = _raw(band, torch.float32)
    raw[first - 1] += 1e-6                                         # what an atomic add of a small gradient does
    with pytest.raises(guard.GuardError) as e:
        band.check()
    assert e.value.side == "front" and -4 <= e.value.offset <= -1 and e.value.count >= 1


def test_nan_band_would_miss_the_add_the_canary_sees():
    """Why accumulated operands get CANARY: NaN + x keeps the NaN's bits."""
    nan = torch.tensor([guard.POISON], dtype=torch.int32).view(torch.float32)
    assert torch.equal((nan + 1.0).view(torch.int32), nan.view(torch.int32))
    can = torch.tensor([guard.CANARY], dtype=torch.int32).view(torch.float32)
    assert not torch.equal((can + 1e-36).view(torch.int32), can.view(torch.int32))


def test_one_byte_past_an_odd_uint8_tensor():
    t, band = guard.guarded_empty((3, 7, 5), torch.uint8, pattern=guard.CANARY)
    t.zero_()
    assert t.numel() % 4 == 1
    band.check()
    band.buf[band.front + t.numel()] = 0                            # a 32-bit store that rounds the byte count up does this
    with pytest.raises(guard.GuardError) as e:
        band.check()
    assert e.value.side == "back" and e.value.offset == 105 and e.value.count == 1


def test_store_at_the_far_edge_of_each_band():
    t, band = guard.guarded_empty((5, 5), torch.float32, pattern=guard.CANARY)
    band.buf[band.buf.numel() - 1] ^= 0xFF
    with pytest.raises(guard.GuardError) as e:
        band.check()
    assert e.value.side == "back" and e.value.offset == 100 + band.back - 1 and e.value.count == 1
    t, band = guard.guarded_empty((5, 5), torch.float32, pattern=guard.CANARY)
    band.buf[0] ^= 0xFF
    with pytest.raises(guard.GuardError) as e:
        band.check()
    assert e.value.side == "front" and e.value.offset == -band.front


def test_poison_reaches_arithmetic():
    x, band = guard.place(torch.ones(4, 6), guard.POISON)
    raw, first = _raw(band, torch.float32)
    assert torch.isfinite(x).all() and torch.isfinite(x.sum())
    halo = raw[first - 1:first + x.numel() + 1]                     # a read one element too wide on each side
    assert not torch.isfinite(halo.sum())
    assert not torch.isfinite((halo * 0.0).sum())                   # a multiply-by-zero mask does not save it
    band.check()                                                    # reading leaves the bands alone


def _fake_module(name):
    m = types.ModuleType(name)
    m.torch = torch
    exec("def run(f, *a, **k):\n    return getattr(torch, f)(*a, **k)\n", m.__dict__)
    return m


def test_proxy_intercepts_every_allocation_form():
    inside, outside = _fake_module("pkg.inside"), _fake_module("pkg.outside")
    like = torch.randn(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    with guard.allocations(inside) as rec:
        assert inside.torch is not torch and outside.torch is torch
        outs = [
            (inside.run("empty", 3, 4), (3, 4), torch.float32, None),
            (inside.run("empty", (2, 3, 4, 5), dtype=torch.bfloat16, memory_format=torch.channels_last), (2, 3, 4, 5), torch.bfloat16, None),
            (inside.run("empty_like", like), (2, 3, 4, 5), torch.float32, None),
            (inside.run("empty_like", like, memory_format=torch.contiguous_format), (2, 3, 4, 5), torch.float32, None),
            (inside.run("zeros", (7,), dtype=torch.int32), (7,), torch.int32, 0),
            (inside.run("zeros", 2, 3, device="cpu"), (2, 3), torch.float32, 0),
            (inside.run("zeros_like", like, dtype=torch.uint8), (2, 3, 4, 5), torch.uint8, 0),
            (inside.run("full", (3, 3), 2.5), (3, 3), torch.float32, 2.5),
            (inside.run("full", (5,), 7, dtype=torch.uint8), (5,), torch.uint8, 7),
            (inside.run("ones", 4), (4,), torch.float32, 1),
        ]
        assert rec.count == len(outs)
        for (t, shape, dtype, fill), band in zip(outs, rec.bands):
            assert tuple(t.shape) == shape and t.dtype == dtype
            assert band.buf.data_ptr() + band.front == t.data_ptr() and band.nbytes == t.numel() * t.element_size()
            if fill is not None:
                assert bool((t == fill).all())
        assert outs[1][0].is_contiguous(memory_format=torch.channels_last)
        assert outs[2][0].stride() == like.stride() and outs[6][0].stride() == like.stride()
        assert outs[3][0].is_contiguous()
        assert inside.run("empty", 3, requires_grad=True).requires_grad
        # everything else is torch's own
        assert inside.run("arange", 4).tolist() == [0, 1, 2, 3] and inside.torch.float32 is torch.float32
        # a module that was not named allocates as always
        before = rec.count
        outside.run("zeros", 8)
        torch.zeros(8)
        assert rec.count == before
    assert inside.torch is torch


def test_allocations_checks_on_exit_and_restores_after_an_error():
    inside = _fake_module("pkg.inside")
    with pytest.raises(guard.GuardError) as e:
        with guard.allocations(inside) as rec:
            t = inside.run("zeros", 9)
            rec.bands[0].buf[rec.bands[0].front + 36] = 1          # the float right behind a 9-element tensor
    assert e.value.side == "back" and e.value.offset == 36
    assert inside.torch is torch
    with pytest.raises(KeyError):
        with guard.allocations(inside):
            raise KeyError("x")
    assert inside.torch is torch


def test_zeropool_is_routed_to_the_guarded_path():
    from deep_visual_slam_amd import zeropool
    orig = zeropool.zeros
    with guard.allocations(zeropool) as rec:
        dw = zeropool.zeros((6, 5, 3, 3), torch.device("cpu"), channels_last=True)
        st = zeropool.zeros((2, 2, 5), torch.device("cpu"), pooled=False)
        assert rec.count == 2
        ref = torch.zeros(6 * 9 * 5).view(6, 3, 3, 5).permute(0, 3, 1, 2)      # the pool's view (zeropool.py)
        assert dw.shape == ref.shape and dw.stride() == ref.stride() and dw.dtype == torch.float32
        assert st.shape == (2, 2, 5) and st.is_contiguous()
        assert float(dw.abs().sum()) == 0.0 and float(st.abs().sum()) == 0.0
    assert zeropool.zeros == orig and zeropool.torch is torch


def test_appends_from_other_threads_are_kept():
    import threading
    rec = guard.Bands("cpu")
    ts = [threading.Thread(target=lambda: [rec.empty((3,)) for _ in range(50)]) for _ in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(rec) == 200
    rec.check()
