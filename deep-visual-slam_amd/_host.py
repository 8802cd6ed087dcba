"""What every Python wrapper in front of a kernel shares: the one argument check, the one shape refusal, the one alignment
rule and the one rule for reading a view in place.  Depends on torch and _lib alone, so ops.py and the RAFT family (_raft_host)
can both import it."""
import torch

from ._lib import DvsError

CL = torch.channels_last


def gpu_arg(who, t, want=None, rank=4, ok=None, no_cpu=DvsError, fp32_note=""):
    """Refuse `t` unless it is a GPU tensor, fp32 and, where `want` ("[N,2,h,w] expected") says what is, of a rank in `rank` with
    ok(t.shape).  Every message starts with `who`; `no_cpu` is the class raised for what is not on the GPU.  Reads is_cuda, dtype,
    dim(), shape and device only, so a stand-in that has those passes as far as a tensor would."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise no_cpu("%s: GPU tensors only (got %s); this package has no CPU path" % (who, getattr(t, "device", type(t))))
    if t.dtype != torch.float32:
        raise DvsError("%s: fp32 only, got %s%s" % (who, t.dtype, fp32_note))
    if want is not None and (t.dim() not in (rank if isinstance(rank, tuple) else (rank,)) or (ok is not None and not ok(t.shape))):
        raise DvsError("%s: %s, got %s" % (who, want, tuple(t.shape)))


def shaped(op, name, t, what, *shapes, like=None):
    """Refuse `t` unless its shape is one of `shapes`: "<op>: <name> must be <what> = <shapes>, got <shape>".  `like` is a tensor
    whose device `t` has to share."""
    if tuple(t.shape) not in shapes:
        raise DvsError("%s: %s must be %s = %s, got %s" % (op, name, what, " or ".join(str(s) for s in shapes), tuple(t.shape)))
    if like is not None and t.device != like.device:
        raise DvsError("%s: %s is on %s, not on %s" % (op, name, t.device, like.device))


def not_negative(who, **values):
    """The values as floats; refuses, naming all of them, unless every one is finite and not negative."""
    got = tuple(float(v) for v in values.values())
    if not all(0.0 <= v < float("inf") for v in got):
        raise DvsError("%s: %s must be finite and not negative" % (who, ", ".join("%s=%r" % kv for kv in values.items())))
    return got


def dense_view(t, inner=1):
    """(tensor, stride in elements of every dim in front of the innermost run, outermost first, ...) with which a kernel that takes
    those strides reads `t`: `t` itself where the innermost run is dense and nothing overlaps, else ONE dense copy -- a layout a
    kernel does not address is never read as if it were dense.  inner=1: the run is the last dim, with unit stride; inner=3: the
    last two dims, a last dim of size 3 with stride 1 behind a dim of stride 3 (uint8 pixels).  Walking outwards from the run, a
    dim of size 1 takes the extent of what lies inside it as its stride (whatever torch reports for it), and any other dim must
    have a stride of at least that extent.  So a dense tensor, a batch or channel slice, a crop and a view at a storage offset are
    read in place; a transposed, an expanded or an overlapping one is copied.  Stride arithmetic only: any device."""
    n, shape, strides, extent = t.dim(), t.shape, list(t.stride()), 1
    front = n - (1 if inner == 1 else 2)
    for d in reversed(range(n)):
        if shape[d] == 1:
            strides[d] = extent
        elif strides[d] < extent or (d >= front and strides[d] != extent):
            t = t.contiguous()
            return (t,) + tuple(t.stride()[:front])
        extent += (shape[d] - 1) * strides[d]
    return (t,) + tuple(strides[:front])


def aligned(t, memory_format=torch.contiguous_format, bytes=16):
    """A tensor a kernel only READS, dense in `memory_format` and with its first byte on a `bytes` boundary as the vector loads
    of the entries demand: t itself where it is both, else a copy.  (A batch slice of a tensor of odd images, a row slice of a
    Linear's weight and a view at a storage offset are dense and misaligned.)"""
    if not t.is_contiguous(memory_format=memory_format):
        return t.contiguous(memory_format=memory_format)       # a fresh allocation: aligned
    return t if t.data_ptr() % bytes == 0 else t.clone(memory_format=memory_format)
