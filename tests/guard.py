"""Guard bands: where does a kernel read and write?

The value tests compare what a kernel returns; this helper checks that it stays inside its buffers.  A tensor is
carved out of one larger buffer whose every other byte holds a known pattern (a "band" in front of the tensor and
one behind it).  After the kernel ran, the bands are compared byte for byte with the pattern:

  POISON  0x7FC0BEEF  a quiet NaN.  Around buffers a kernel only READS: a halo or tail read that reaches arithmetic
                      turns the result NaN, which the caller's finiteness check sees.
  CANARY  0x0DEADBEF  1.447e-30, a normal fp32.  Around buffers a kernel WRITES or ADDS into: NaN + x keeps the
                      NaN's payload bit for bit, so a NaN band cannot see an atomic add; the canary changes under
                      any add with |x| >~ 1e-37 and under any store of another value.

The front band is a multiple of 256 bytes (the tensor keeps the 16-byte alignment the C ABI requires); the back band
starts at the tensor's exact last byte, without rounding, so a one-element overrun of a tensor whose size is not a
multiple of 16 bytes -- or of a uint8 tensor -- is seen.  Each band is at least max(64 KiB, 2 rows of the tensor), so
an off-by-one-row halo access (row -1, row H) lands inside it.

`allocations(*modules)` guards what the package allocates itself (outputs, workspaces, weight packs): while it is
active the module-level name `torch` of the named package modules is a forwarding proxy whose allocation functions
return guarded tensors, and `zeropool.zeros` is routed to it.  `torch` itself is untouched.

This is a plain module (imported like cloud_ref), not a conftest: it changes no pytest behaviour.
"""
import contextlib
import threading

import torch

POISON = 0x7FC0BEEF
CANARY = 0x0DEADBEF
MIN_PAD = 64 * 1024


class GuardError(AssertionError):
    """A band was touched.  side: "front" / "back"; offset: first changed byte relative to the tensor's first byte
    (negative in the front band, >= the tensor's byte size in the back band); count: number of changed bytes."""

    def __init__(self, name, side, offset, count, nbytes):
        self.side, self.offset, self.count, self.nbytes = side, offset, count, nbytes
        where = ("%d bytes before the tensor's first byte" % -offset if side == "front"
                 else "%d bytes past the tensor's last byte" % (offset - nbytes))
        super().__init__("guard band violated: %s band of %s, first changed byte at tensor offset %d (%s), %d bytes changed"
                         % (side, name, offset, where, count))


def _filled(nbytes, pattern, device):
    """uint8[nbytes] holding the 4 bytes of `pattern` (little endian) repeated from byte 0."""
    words = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    words.fill_(pattern if pattern < 1 << 31 else pattern - (1 << 32))
    return words.view(torch.uint8)[:nbytes]


def _dense_strides(t):
    """The strides of `t` if it covers its memory exactly once (contiguous in some dimension order), else None."""
    if t.numel() == 0:
        return None
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return None
        expect *= size
    return tuple(t.stride())


def _strides_for(shape, memory_format):
    return tuple(torch.empty(shape, device="meta", memory_format=memory_format).stride())


def default_pad(shape, itemsize):
    """max(64 KiB, 2 x W x C x itemsize): two rows of an image tensor [.., C, H, W] whatever its layout."""
    row = 1
    if len(shape) >= 3:
        row = int(shape[-1]) * int(shape[-3])
    elif len(shape) >= 1:
        row = int(shape[-1])
    return max(MIN_PAD, 2 * row * itemsize)


class Band:
    def __init__(self, buf, front, nbytes, pattern, name):
        self.buf, self.front, self.nbytes, self.pattern, self.name = buf, front, nbytes, pattern, name

    @property
    def back(self):
        return self.buf.numel() - self.front - self.nbytes

    def violations(self):
        """[(side, first offset relative to the tensor, changed bytes)] -- raw byte comparison, never as floats."""
        want = _filled(self.buf.numel(), self.pattern, self.buf.device)
        out = []
        end = self.front + self.nbytes
        for side, lo, hi in (("front", 0, self.front), ("back", end, self.buf.numel())):
            diff = self.buf[lo:hi] != want[lo:hi]
            count = int(diff.sum())
            if count:
                first = int(diff.nonzero()[0]) + lo
                out.append((side, first - self.front, count))
        return out

    def check(self):
        for side, offset, count in self.violations():
            raise GuardError(self.name, side, offset, count, self.nbytes)


def guarded_empty(shape, dtype=torch.float32, device="cpu", memory_format=None, strides=None, pattern=CANARY,
                  pad_bytes=None, name=None):
    """(tensor, band): an uninitialised tensor (it holds the pattern) between two bands.  `strides` (a dense layout)
    or `memory_format` choose the layout; default contiguous."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    itemsize = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    if strides is None:
        strides = _strides_for(shape, memory_format or torch.contiguous_format)
    strides = tuple(int(s) for s in strides)
    span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if numel else 0
    if span != numel:
        raise ValueError("guarded_empty: layout %s / %s does not cover its memory exactly once" % (shape, strides))
    pad = default_pad(shape, itemsize) if pad_bytes is None else int(pad_bytes)
    front = (pad + 255) // 256 * 256
    nbytes = span * itemsize
    buf = _filled(front + nbytes + pad, pattern, device)
    assert buf.data_ptr() % 16 == 0
    body = buf[front:front + nbytes].view(dtype)
    t = body.as_strided(shape, strides) if numel else body.view(shape)
    band = Band(buf, front, nbytes, pattern, name or "%s%s" % (str(dtype).replace("torch.", ""), list(shape)))
    return t, band


def place(t, pattern=POISON, device=None, pad_bytes=None, name=None):
    """(copy, band): `t` copied into a guarded buffer with its shape, dtype and strides (channels_last stays
    channels_last; a layout that is not dense becomes contiguous).  The copy is a leaf without requires_grad."""
    t = t.detach()
    dst, band = guarded_empty(t.shape, t.dtype, device if device is not None else t.device, strides=_dense_strides(t),
                              pattern=pattern, pad_bytes=pad_bytes, name=name)
    dst.copy_(t)
    return dst, band


class Bands:
    """A list of bands with the constructors attached: `g = Bands(dev); x = g.place(t); ...; g.check()`."""

    def __init__(self, device=None):
        self.device = device
        self.bands = []
        self._lock = threading.Lock()

    def add(self, band):
        with self._lock:                       # autograd's device thread appends too
            self.bands.append(band)

    def place(self, t, pattern=POISON, **kw):
        out, band = place(t, pattern, device=self.device, **kw)
        self.add(band)
        return out

    def empty(self, shape, dtype=torch.float32, pattern=CANARY, **kw):
        out, band = guarded_empty(shape, dtype, self.device if self.device is not None else "cpu", pattern=pattern, **kw)
        self.add(band)
        return out

    def zeros(self, shape, dtype=torch.float32, pattern=CANARY, **kw):
        out = self.empty(shape, dtype, pattern, **kw)
        out.zero_()
        return out

    def __len__(self):
        return len(self.bands)

    def check(self):
        with self._lock:
            bands = list(self.bands)
        if any(b.buf.is_cuda for b in bands):
            torch.cuda.synchronize()
        for b in bands:
            b.check()


# ---- the package's own allocations ------------------------------------------------------------------------------------

def _shape_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(args[0])
    return tuple(args)


class _TorchProxy:
    """Stands in for the name `torch` inside a package module: everything is forwarded to torch except the allocation
    functions, which return guarded tensors of the same shape, dtype, device, strides and requires_grad."""

    def __init__(self, bands, pad_bytes):
        self.__dict__["_bands"] = bands
        self.__dict__["_pad"] = pad_bytes

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _new(self, shape, fill, dtype=None, device=None, memory_format=None, strides=None, requires_grad=False,
             layout=None, pin_memory=False, out=None):
        if out is not None or (layout is not None and layout != torch.strided) or pin_memory:
            raise NotImplementedError("guarded allocation with out= / layout= / pin_memory=")
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t, band = guarded_empty(shape, dtype, device, memory_format=memory_format, strides=strides, pattern=CANARY,
                                pad_bytes=self._pad)
        self._bands.add(band)
        if fill is not None:
            t.fill_(fill)                       # the interior only: the bands keep the canary
        if requires_grad:
            t.requires_grad_(True)
        return t

    def _like(self, t, fill, dtype=None, device=None, memory_format=torch.preserve_format, **kw):
        strides = None
        if memory_format == torch.preserve_format:
            strides, memory_format = _dense_strides(t), None
        return self._new(tuple(t.shape), fill, dtype=dtype if dtype is not None else t.dtype,
                         device=device if device is not None else t.device, memory_format=memory_format, strides=strides, **kw)

    def empty(self, *size, **kw):
        return self._new(_shape_of(size), None, **kw)

    def zeros(self, *size, **kw):
        return self._new(_shape_of(size), 0, **kw)

    def ones(self, *size, **kw):
        return self._new(_shape_of(size), 1, **kw)

    def full(self, size, fill_value, **kw):
        if kw.get("dtype") is None:
            kw["dtype"] = (torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int)
                           else torch.get_default_dtype())
        return self._new(tuple(size), fill_value, **kw)

    def empty_like(self, t, **kw):
        return self._like(t, None, **kw)

    def zeros_like(self, t, **kw):
        return self._like(t, 0, **kw)

    def ones_like(self, t, **kw):
        return self._like(t, 1, **kw)

    def full_like(self, t, fill_value, **kw):
        return self._like(t, fill_value, **kw)


class Allocations(Bands):
    """What `allocations()` yields: the bands of every allocation guarded so far; `count` is their number."""

    @property
    def count(self):
        return len(self.bands)


@contextlib.contextmanager
def allocations(*modules, pad_bytes=None):
    """While active, every torch.empty / empty_like / zeros / zeros_like / full (and ones / ones_like / full_like) call
    made through the module-level name `torch` of `modules`, and every zeropool.zeros hand-out, returns a tensor between
    two CANARY bands.  All bands are checked on a clean exit (after a device synchronise); the yielded object's `count`
    says how many allocations were guarded -- assert on it, so that a refactor that bypasses the proxy is noticed."""
    rec = Allocations()
    proxy = _TorchProxy(rec, pad_bytes)
    saved = []
    zp, zp_zeros = None, None
    try:
        for m in modules:
            if getattr(m, "torch", None) is torch:
                saved.append(m)
                m.torch = proxy
            if m.__name__.endswith(".zeropool") and hasattr(m, "zeros"):
                zp, zp_zeros = m, m.zeros

                def zeros(shape, device, channels_last=False, pooled=True):
                    if channels_last:           # logical [Cout,Cin,kh,kw], physical [Cout][kh][kw][Cin], as the pool's view
                        return proxy.zeros(tuple(shape), device=device, dtype=torch.float32, memory_format=torch.channels_last)
                    return proxy.zeros(tuple(shape), device=device, dtype=torch.float32)
                m.zeros = zeros
        yield rec
    finally:
        for m in saved:
            m.torch = torch
        if zp is not None:
            zp.zeros = zp_zeros
    rec.check()
