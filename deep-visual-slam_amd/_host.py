"""What every Python wrapper in front of a kernel shares: the one argument check, the one shape refusal and the one alignment
rule.  Depends on torch and _lib alone, so ops.py and the RAFT family (_raft_host) can both import it."""
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


def aligned(t, memory_format=torch.contiguous_format, bytes=16):
    """A tensor a kernel only READS, dense in `memory_format` and with its first byte on a `bytes` boundary as the vector loads
    of the entries demand: t itself where it is both, else a copy.  (A batch slice of a tensor of odd images, a row slice of a
    Linear's weight and a view at a storage offset are dense and misaligned.)"""
    if not t.is_contiguous(memory_format=memory_format):
        return t.contiguous(memory_format=memory_format)       # a fresh allocation: aligned
    return t if t.data_ptr() % bytes == 0 else t.clone(memory_format=memory_format)
