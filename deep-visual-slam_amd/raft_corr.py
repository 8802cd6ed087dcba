"""RAFT correlation block on the device (csrc/corr.hip): all-pairs volume, pooling pyramid, windowed bilinear lookup.

The surface of the reference's model/raft/core/corr.py:12-60:

    block = CorrBlock(fmap1, fmap2, num_levels=4, radius=4)      # raft.py:89-92
    for _ in range(iters):
        corr = block(coords1.detach())                           # raft.py:100-102 -> [B, L * (2r+1)^2, h, w]

Memory.  The pyramid is ONE buffer (level i a contiguous [B*h*w, h_i*w_i] matrix inside it, `corr_pyramid[i]` a view).  The
backward of the N lookups of a block adds into ONE gradient pyramid of the same size: every lookup node takes a one-element
token that the build node produced, so autograd runs all lookup backwards (each accumulates in place and hands a zero back for
the token) before the build node's backward, which turns the accumulated gradient into dfmap1 / dfmap2 and frees it.
Coordinates are constants (raft.py:101 detaches them).  fp32 only, GPU only; the process-wide precision mode has no effect.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import CorrCfg, DvsError, check, ptr

CL = torch.channels_last


def _cfg(B, Cn, H, W, num_levels, radius, nchw1=0, nchw2=0):
    cfg = CorrCfg()
    cfg.B, cfg.C, cfg.H, cfg.W, cfg.num_levels, cfg.radius = int(B), int(Cn), int(H), int(W), int(num_levels), int(radius)
    cfg.fmap1_nchw, cfg.fmap2_nchw = int(nchw1), int(nchw2)
    return cfg


def _check_fmap(name, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise DvsError("%s: GPU tensors only (got %s); this package has no CPU path" % (name, getattr(t, "device", type(t))))
    if t.dtype != torch.float32:
        raise DvsError("%s: fp32 only, got %s (the reference casts with .float() at raft.py:82-83 even under autocast)"
                       % (name, t.dtype))
    if t.dim() != 4:
        raise DvsError("%s: [B,C,h,w] expected, got %s" % (name, tuple(t.shape)))


def _sizes(cfg):
    """(pyramid floats, level offsets, workspace bytes) of dvs_corr_sizes, which is also where every limit of the kernels is
    checked (C % 4, levels, radius, >= 2 rows and columns per level, (h*w)^2 < 2^31): one place, no copy of them here."""
    floats, ws = C.c_size_t(), C.c_size_t()
    offs = (C.c_size_t * max(int(cfg.num_levels), 1))()
    check(_lib.lib().dvs_corr_sizes(C.byref(cfg), C.byref(floats), offs, C.byref(ws)), "dvs_corr_sizes")
    return floats.value, list(offs), ws.value


def _layout(t):
    """(tensor whose memory the kernels read in place, nchw flag): channels_last memory is position-major already."""
    if t.is_contiguous(memory_format=CL):
        return t.permute(0, 2, 3, 1), 0
    if t.is_contiguous():
        return t, 1
    return t.contiguous(memory_format=CL).permute(0, 2, 3, 1), 0


class _State:
    """What the lookups of one block share: geometry, the pyramid buffer, and (during a backward) the gradient pyramid.
    `grad` lives from the first lookup backward of a pass to the build node's backward; a pass that an exception cut short
    leaves it behind, so every new lookup in the forward direction drops it (CorrBlock.__call__)."""

    def __init__(self, cfg, pyramid, offsets, sizes):
        self.cfg, self.pyramid, self.offsets, self.sizes = cfg, pyramid, offsets, sizes
        self.grad = None

    def grad_pyramid(self):
        if self.grad is None:
            self.grad = torch.zeros_like(self.pyramid)
        return self.grad


class _Build(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels, radius, holder):
        ctx.set_materialize_grads(False)                # an unused pyramid output must not become a dense zero gradient
        B, Cn, H, W = fmap1.shape
        f1, n1 = _layout(fmap1.detach())
        f2, n2 = _layout(fmap2.detach())
        cfg = _cfg(B, Cn, H, W, num_levels, radius, n1, n2)
        floats, offs, ws = _sizes(cfg)
        pyramid = torch.empty(floats, device=fmap1.device, dtype=torch.float32)
        workspace = torch.empty(ws, device=fmap1.device, dtype=torch.uint8)
        check(_lib.lib().dvs_corr_build(C.byref(cfg), ptr(f1), ptr(f2), ptr(pyramid), ptr(workspace), _lib.stream()), "dvs_corr_build")
        sizes = [(H >> i, W >> i) for i in range(num_levels)]
        state = _State(cfg, pyramid.detach(), offs, sizes)           # detached: the state must not own the graph that owns it
        holder.append(state)
        # The backward reads the feature maps again (in place when they are channels_last) and the pooled rows derived from
        # them: saved through autograd, so that an in-place change between forward and backward is an error, not a wrong
        # gradient.  A layout copy made here (neither NCHW- nor channels_last-contiguous input) is kept instead of remade.
        ctx.save_for_backward(fmap1, fmap2)
        ctx.copies = tuple(c if c.data_ptr() != t.data_ptr() else None for c, t in ((f1, fmap1), (f2, fmap2)))
        ctx.state, ctx.workspace = state, workspace
        token = torch.zeros(1, device=fmap1.device, dtype=torch.float32)
        return pyramid, token

    @staticmethod
    def backward(ctx, dpyramid, dtoken):
        st = ctx.state
        g = st.grad
        st.grad = None                                  # a second backward through a retained graph starts from zero again
        if dpyramid is not None:                        # somebody differentiated through corr_pyramid itself
            g = dpyramid.contiguous() if g is None else g.add_(dpyramid)
        if g is None:
            g = torch.zeros_like(st.pyramid)
        cfg = st.cfg
        N = cfg.H * cfg.W
        f1, f2 = (c if c is not None else _layout(t.detach())[0] for c, t in zip(ctx.copies, ctx.saved_tensors))
        d1 = torch.empty(cfg.B, N, cfg.C, device=g.device, dtype=torch.float32)
        d2 = torch.empty(cfg.B, N, cfg.C, device=g.device, dtype=torch.float32)
        check(_lib.lib().dvs_corr_volume_bwd(C.byref(cfg), ptr(g), ptr(f1), ptr(f2), ptr(ctx.workspace), ptr(d1), ptr(d2),
                                             _lib.stream()), "dvs_corr_volume_bwd")
        as_map = lambda d: d.view(cfg.B, cfg.H, cfg.W, cfg.C).permute(0, 3, 1, 2)       # [B,C,h,w] in channels_last memory
        return (as_map(d1) if ctx.needs_input_grad[0] else None, as_map(d2) if ctx.needs_input_grad[1] else None, None, None, None)


class _Lookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, coords, state, channels_last):
        ctx.state, ctx.coords = state, coords
        return _lookup_raw(state, coords, channels_last)

    @staticmethod
    def backward(ctx, dout):
        st = ctx.state
        cfg = st.cfg
        nhwc = int(dout.is_contiguous(memory_format=CL) and not dout.is_contiguous())
        dout = dout.permute(0, 2, 3, 1) if nhwc else dout.contiguous()
        check(_lib.lib().dvs_corr_lookup_bwd(C.byref(cfg), ptr(ctx.coords), ptr(dout), nhwc, ptr(st.grad_pyramid()), _lib.stream()),
              "dvs_corr_lookup_bwd")
        return torch.zeros(1, device=dout.device, dtype=torch.float32), None, None, None


def _lookup_raw(state, coords, channels_last):
    cfg = state.cfg
    ch = cfg.num_levels * (2 * cfg.radius + 1) ** 2
    out = torch.empty(cfg.B, ch, cfg.H, cfg.W, device=coords.device, dtype=torch.float32,
                      memory_format=CL if channels_last else torch.contiguous_format)
    check(_lib.lib().dvs_corr_lookup_fwd(C.byref(cfg), ptr(state.pyramid), ptr(coords),
                                         ptr(out.permute(0, 2, 3, 1) if channels_last else out), int(bool(channels_last)),
                                         _lib.stream()), "dvs_corr_lookup_fwd")
    return out


def _memory_format_flag(memory_format):
    if memory_format in (None, torch.contiguous_format):
        return False
    if memory_format == CL:
        return True
    raise DvsError("corr_lookup: memory_format must be torch.contiguous_format or torch.channels_last")


class CorrBlock:
    """model/raft/core/corr.py:12-60.  `corr_pyramid[i]` is a [B*h*w, 1, h>>i, w>>i] view of the one pyramid buffer."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        _check_fmap("CorrBlock: fmap1", fmap1)
        _check_fmap("CorrBlock: fmap2", fmap2)
        if fmap1.shape != fmap2.shape:
            raise DvsError("CorrBlock: fmap1 %s and fmap2 %s differ" % (tuple(fmap1.shape), tuple(fmap2.shape)))
        if fmap2.device != fmap1.device:
            raise DvsError("CorrBlock: fmap1 on %s, fmap2 on %s" % (fmap1.device, fmap2.device))
        B, Cn, H, W = fmap1.shape
        _sizes(_cfg(B, Cn, H, W, num_levels, radius))               # every shape limit, before anything is allocated
        self.num_levels, self.radius = int(num_levels), int(radius)
        holder = []
        pyramid, self._token = _Build.apply(fmap1, fmap2, self.num_levels, self.radius, holder)
        self._state = holder[0]
        self._flat = pyramid
        N = H * W
        self.corr_pyramid = []
        for i, (hi, wi) in enumerate(self._state.sizes):
            o = self._state.offsets[i]
            self.corr_pyramid.append(pyramid[o:o + B * N * hi * wi].view(B * N, 1, hi, wi))

    def __call__(self, coords, memory_format=None):
        st = self._state
        cfg = st.cfg
        if not torch.is_tensor(coords) or not coords.is_cuda:
            raise DvsError("CorrBlock: GPU coordinates only; this package has no CPU path")
        if coords.device != st.pyramid.device:
            raise DvsError("CorrBlock: coords on %s, the block on %s" % (coords.device, st.pyramid.device))
        if coords.requires_grad:
            raise DvsError("CorrBlock: coordinates are constants -- model/raft/core/raft.py:101 detaches them before the lookup "
                           "(coords1 = coords1.detach()); pass coords.detach()")
        if tuple(coords.shape) != (cfg.B, 2, cfg.H, cfg.W):
            raise DvsError("CorrBlock: coords must be [%d,2,%d,%d], got %s" % (cfg.B, cfg.H, cfg.W, tuple(coords.shape)))
        if coords.dtype != torch.float32:
            raise DvsError("CorrBlock: fp32 coordinates only, got %s" % coords.dtype)
        coords = coords.contiguous()
        cl = _memory_format_flag(memory_format)
        if self._token.requires_grad and torch.is_grad_enabled():
            st.grad = None                              # left behind only by a backward pass that did not finish
            return _Lookup.apply(self._token, coords, st, cl)
        return _lookup_raw(st, coords, cl)

    @staticmethod
    def corr(fmap1, fmap2):
        """corr.py:52-60: the level-0 volume [B, h, w, 1, h, w]."""
        block = CorrBlock(fmap1, fmap2, num_levels=1, radius=0)
        B, _, H, W = fmap1.shape
        return block.corr_pyramid[0].view(B, H, W, 1, H, W)


def corr_pyramid(fmap1, fmap2, num_levels=4, radius=4):
    """The block whose lookups share one pyramid (functional spelling of CorrBlock(...))."""
    return CorrBlock(fmap1, fmap2, num_levels, radius)


def corr_lookup(block, coords, memory_format=None):
    """[B, L * (2r+1)^2, h, w] correlation features of `block` at `coords` [B,2,h,w] (x, y)."""
    return block(coords, memory_format=memory_format)


def pyramid_bytes(B, H, W, num_levels=4):
    return 4 * B * H * W * sum((H >> i) * (W >> i) for i in range(num_levels))


def build_flops(B, Cn, H, W, num_levels=4):
    """2 * (h*w) * (sum of level sizes) * C per sample: what the one-GEMM pyramid spends."""
    return 2.0 * B * H * W * sum((H >> i) * (W >> i) for i in range(num_levels)) * Cn
