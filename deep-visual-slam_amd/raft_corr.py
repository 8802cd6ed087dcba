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

AlternateCorrBlock (corr.py:63-91 over alt_cuda_corr) is the same function without the volume: every lookup computes the
(2r+2)^2 correlations per pixel and level that its taps touch from the feature maps and the pooled rows of fmap2, and its
backward sends their gradient straight to the feature maps.  Nothing of size (h*w)^2 exists, so there is no (h*w)^2 < 2^31
limit; a lookup costs more (it re-reads the rows of fmap2 through the caches).  Outputs and dfmap1 repeat bit for bit; dfmap2
is summed with float atomics and does not.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import CorrCfg, DvsError, check, ptr
from ._raft_host import CL, aligned, gpu_arg


def _cfg(B, Cn, H, W, num_levels, radius, nchw1=0, nchw2=0):
    cfg = CorrCfg()
    cfg.B, cfg.C, cfg.H, cfg.W, cfg.num_levels, cfg.radius = int(B), int(Cn), int(H), int(W), int(num_levels), int(radius)
    cfg.fmap1_nchw, cfg.fmap2_nchw = int(nchw1), int(nchw2)
    return cfg


class NoCpuPath(DvsError, NotImplementedError):
    """What AlternateCorrBlock raises for anything that is not a GPU tensor: a DvsError like every input error of this package,
    and a NotImplementedError because that is what the alternate block of this package answered before it existed."""


def _check_fmaps(who, fmap1, fmap2, no_cpu=DvsError):
    for name, t in (("fmap1", fmap1), ("fmap2", fmap2)):
        gpu_arg("%s: %s" % (who, name), t, "[B,C,h,w] expected", no_cpu=no_cpu,
                fp32_note=" (the reference casts with .float() at raft.py:82-83 even under autocast)")
    if fmap1.shape != fmap2.shape:
        raise DvsError("%s: fmap1 %s and fmap2 %s differ" % (who, tuple(fmap1.shape), tuple(fmap2.shape)))
    if fmap2.device != fmap1.device:
        raise DvsError("%s: fmap1 on %s, fmap2 on %s" % (who, fmap1.device, fmap2.device))


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
        return aligned(t, CL).permute(0, 2, 3, 1), 0
    if t.is_contiguous():
        return aligned(t), 1
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
        dout = dout.permute(0, 2, 3, 1) if nhwc else aligned(dout, bytes=4)      # the lookups read single floats
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


def _check_coords(name, coords, cfg, device):
    gpu_arg(name + ": coords", coords, "[B,2,h,w] expected")
    if coords.device != device:
        raise DvsError("%s: coords on %s, the block on %s" % (name, coords.device, device))
    if coords.requires_grad:
        raise DvsError("%s: coordinates are constants -- model/raft/core/raft.py:101 detaches them before the lookup "
                       "(coords1 = coords1.detach()); pass coords.detach()" % name)
    if tuple(coords.shape) != (cfg.B, 2, cfg.H, cfg.W):
        raise DvsError("%s: coords must be [%d,2,%d,%d], got %s" % (name, cfg.B, cfg.H, cfg.W, tuple(coords.shape)))
    return aligned(coords, bytes=4)


def _memory_format_flag(memory_format):
    if memory_format in (None, torch.contiguous_format):
        return False
    if memory_format == CL:
        return True
    raise DvsError("corr_lookup: memory_format must be torch.contiguous_format or torch.channels_last")


class CorrBlock:
    """model/raft/core/corr.py:12-60.  `corr_pyramid[i]` is a [B*h*w, 1, h>>i, w>>i] view of the one pyramid buffer."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        _check_fmaps("CorrBlock", fmap1, fmap2)
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
        coords = _check_coords("CorrBlock", coords, cfg, st.pyramid.device)
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


# ---- the on-the-fly form ---------------------------------------------------------------------------------------------------
def _alt_sizes(cfg):
    """(pooled-row floats, workspace bytes) of dvs_altcorr_sizes, where every limit of the on-the-fly kernels is checked."""
    floats, ws = C.c_size_t(), C.c_size_t()
    check(_lib.lib().dvs_altcorr_sizes(C.byref(cfg), C.byref(floats), C.byref(ws)), "dvs_altcorr_sizes")
    return floats.value, ws.value


class _AltState:
    """What the lookups of one alternate block share: geometry, the memory the kernels read the feature maps from (the
    tensors themselves when they are channels_last, else layout copies / the workspace's transposed copies)."""

    def __init__(self, cfg, f1, f2, workspace):
        self.cfg, self.f1, self.f2, self.workspace = cfg, f1, f2, workspace


class _AltPool(torch.autograd.Function):
    """fmap2 -> the pooled rows of levels 1 .. L-1 (and, on the way, the transposed copies of NCHW maps in the workspace)."""

    @staticmethod
    def forward(ctx, fmap2, state, floats):
        ctx.set_materialize_grads(False)                # one level: the rows are never read and get no gradient
        pooled = torch.empty(floats, device=fmap2.device, dtype=torch.float32)
        check(_lib.lib().dvs_altcorr_pool(C.byref(state.cfg), ptr(state.f1), ptr(state.f2), ptr(pooled), ptr(state.workspace),
                                          _lib.stream()), "dvs_altcorr_pool")
        ctx.state = state
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        if dpooled is None:
            return None, None, None
        cfg = ctx.state.cfg
        d2 = torch.zeros(cfg.B, cfg.H * cfg.W, cfg.C, device=dpooled.device, dtype=torch.float32)
        check(_lib.lib().dvs_altcorr_unpool(C.byref(cfg), ptr(dpooled.contiguous()), ptr(d2), _lib.stream()), "dvs_altcorr_unpool")
        return d2.view(cfg.B, cfg.H, cfg.W, cfg.C).permute(0, 3, 1, 2), None, None


def _alt_lookup_raw(state, pooled, coords, channels_last):
    cfg = state.cfg
    ch = cfg.num_levels * (2 * cfg.radius + 1) ** 2
    out = torch.empty(cfg.B, ch, cfg.H, cfg.W, device=coords.device, dtype=torch.float32,
                      memory_format=CL if channels_last else torch.contiguous_format)
    check(_lib.lib().dvs_altcorr_fwd(C.byref(cfg), ptr(state.f1), ptr(state.f2), ptr(pooled), ptr(state.workspace), ptr(coords),
                                     ptr(out.permute(0, 2, 3, 1) if channels_last else out), int(bool(channels_last)),
                                     _lib.stream()), "dvs_altcorr_fwd")
    return out


class _AltLookup(torch.autograd.Function):
    """One lookup.  Its backward returns dfmap1, dfmap2 and the gradient of the pooled rows; autograd sums those of the N
    lookups of a block, and _AltPool's backward turns the summed pooled-row gradient into the rest of dfmap2."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, pooled, coords, state, channels_last):
        # saved through autograd, so that an in-place change between forward and backward is an error, not a wrong gradient
        ctx.save_for_backward(fmap1, fmap2, pooled)
        ctx.state, ctx.coords = state, coords
        return _alt_lookup_raw(state, pooled.detach(), coords, channels_last)

    @staticmethod
    def backward(ctx, dout):
        st = ctx.state
        cfg = st.cfg
        _, _, pooled = ctx.saved_tensors                # (reading them is what checks their versions)
        nhwc = int(dout.is_contiguous(memory_format=CL) and not dout.is_contiguous())
        dout = dout.permute(0, 2, 3, 1) if nhwc else aligned(dout, bytes=4)      # the lookups read single floats
        N = cfg.H * cfg.W
        d1 = torch.empty(cfg.B, N, cfg.C, device=dout.device, dtype=torch.float32)
        d2 = torch.zeros(cfg.B, N, cfg.C, device=dout.device, dtype=torch.float32)
        dpooled = torch.zeros_like(pooled)
        check(_lib.lib().dvs_altcorr_bwd(C.byref(cfg), ptr(st.f1), ptr(st.f2), ptr(pooled), ptr(st.workspace), ptr(ctx.coords),
                                         ptr(dout), nhwc, ptr(d1), ptr(d2), ptr(dpooled), _lib.stream()), "dvs_altcorr_bwd")
        as_map = lambda d: d.view(cfg.B, cfg.H, cfg.W, cfg.C).permute(0, 3, 1, 2)       # [B,C,h,w] in channels_last memory
        return (as_map(d1) if ctx.needs_input_grad[0] else None, as_map(d2) if ctx.needs_input_grad[1] else None,
                dpooled if ctx.needs_input_grad[2] and cfg.num_levels > 1 else None, None, None, None)


class AlternateCorrBlock:
    """model/raft/core/corr.py:63-91 (alternate_corr=True), differentiable in both feature maps.  Holds the feature maps and
    the pooled rows of fmap2 -- (1 + 1/4 + ...) feature maps, not a volume."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        _check_fmaps("AlternateCorrBlock", fmap1, fmap2, NoCpuPath)
        B, Cn, H, W = fmap1.shape
        self.num_levels, self.radius = int(num_levels), int(radius)
        _alt_sizes(_cfg(B, Cn, H, W, self.num_levels, self.radius))    # every shape limit, before anything is allocated
        f1, n1 = _layout(fmap1.detach())
        f2, n2 = _layout(fmap2.detach())
        cfg = _cfg(B, Cn, H, W, self.num_levels, self.radius, n1, n2)
        floats, ws = _alt_sizes(cfg)
        workspace = torch.empty(ws, device=fmap1.device, dtype=torch.uint8)
        self._state = _AltState(cfg, f1, f2, workspace)
        self._fmap1, self._fmap2 = fmap1, fmap2
        self._pooled = _AltPool.apply(fmap2, self._state, floats)

    def __call__(self, coords, memory_format=None):
        st = self._state
        coords = _check_coords("AlternateCorrBlock", coords, st.cfg, self._fmap1.device)
        return _AltLookup.apply(self._fmap1, self._fmap2, self._pooled, coords, st, _memory_format_flag(memory_format))


def altcorr_bytes(B, Cn, H, W, num_levels=4, radius=4):
    """Bytes an AlternateCorrBlock holds beside its inputs -- the pooled rows of fmap2 -- plus one lookup's output: the
    counterpart of pyramid_bytes.  (NCHW inputs add one position-major copy of each map, 4 * B * C * H * W bytes.)"""
    pooled = 4 * B * Cn * sum((H >> i) * (W >> i) for i in range(1, num_levels))
    return pooled + 4 * B * num_levels * (2 * radius + 1) ** 2 * H * W


def pyramid_bytes(B, H, W, num_levels=4):
    return 4 * B * H * W * sum((H >> i) * (W >> i) for i in range(num_levels))


def build_flops(B, Cn, H, W, num_levels=4):
    """2 * (h*w) * (sum of level sizes) * C per sample: what the one-GEMM pyramid spends."""
    return 2.0 * B * H * W * sum((H >> i) * (W >> i) for i in range(num_levels)) * Cn
