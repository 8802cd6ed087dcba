"""The view zoo: one tensor's values in every memory layout a caller can hand an operator.

The value tests hand the operators dense, freshly allocated tensors.  Real callers hand them crops, channel slices (what torch.split
returns), batch slices, tensors at a storage offset, and autograd hands the backwards expanded (stride 0) and channels_last
cotangents.  Every kernel here takes raw pointers, so the Python wrapper in front of it decides what memory the pointer names and
whether to copy; `views(t)` yields the layouts that decision has to cope with:

  planar         a contiguous clone                                                  the baseline
  cl             4-D: a channels_last clone                                          NCHW assumed
  offset         dense, starting 1 element into its storage                          is_contiguous() true, data_ptr() % 16 == 4
  offset_cl      4-D: the same in channels_last form
  batch_slice    big[1:1+N] of [N+2, ..]                                             a per-image offset, misaligned for odd images
  chan_slice     big[:, 1:1+C] of [N, C+2, ..]                                       torch.split / chunk outputs
  chan_slice_cl  4-D: the same of a channels_last parent                             contiguous in neither format
  crop           big[..., 1:1+H, 2:2+W] of a padded parent                           InputPadder.unpad: a row stride > W
  transposed     the last two dims swapped in memory                                 unit stride on the wrong axis
  expanded       stride 0 along every dim (of size > 1) along which t is constant    the cotangent of .sum() / .mean()
  size1          stride 999 on every dim of size 1                                   code that reads t.stride()

A kind is produced only where it applies (rank, sizes, constancy).

Safety: every view lives in ONE allocation of its own, at least numel() elements of that allocation lie behind the view's first
element, and what the view does not cover holds SENTINEL (finite).  A wrapper that wrongly reads the view as dense from data_ptr()
therefore computes wrong values -- it never touches foreign memory -- and shows up as a failed comparison.

`dense(v)` is the twin in a fresh allocation; `relayout(y, kind)` is an identity whose backward re-makes the incoming gradient as
`kind`, so that the backward of the operator in front of it receives a cotangent of a chosen layout.

A plain module (imported like guard.py), not a conftest: it changes no pytest behaviour.
"""
import torch

CL = torch.channels_last
SENTINEL = {torch.float32: 12345.0, torch.uint8: 201}
KINDS = ("planar", "cl", "offset", "offset_cl", "batch_slice", "chan_slice", "chan_slice_cl", "crop", "transposed", "expanded", "size1")
CL_KINDS = ("cl", "offset_cl", "chan_slice_cl")
# what a stride-blind reader (numel elements from data_ptr()) gets wrong; the others are dense in their own format
NOT_DENSE = ("chan_slice", "chan_slice_cl", "crop", "transposed", "expanded")
SIZE1_STRIDE = 999


def _strides(shape, memory_format=torch.contiguous_format):
    return tuple(torch.empty(shape, device="meta", memory_format=memory_format).stride())


def _carve(t, strides, offset):
    """t's values at (strides, offset) of a fresh flat allocation full of the sentinel, with the slack the module promises."""
    n = t.numel()
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, strides)) if n else 0
    buf = torch.full((offset + max(span, n) + n,), SENTINEL[t.dtype], dtype=t.dtype, device=t.device)
    v = buf.as_strided(tuple(t.shape), strides, offset)
    v.copy_(t)
    return v


def _sub(t, parent_shape, memory_format, index):
    """The strides and offset of parent[index] for a parent of `parent_shape` in `memory_format`."""
    probe = torch.empty(parent_shape, device="meta", memory_format=memory_format)[index]
    assert tuple(probe.shape) == tuple(t.shape)
    return _carve(t, tuple(probe.stride()), probe.storage_offset())


def constant_dims(t):
    """The dims of size > 1 along which t does not vary."""
    return tuple(d for d in range(t.dim()) if t.shape[d] > 1 and bool((t == t.narrow(d, 0, 1)).all()))


def make(t, kind):
    """The `kind` view of the dense tensor t (on t's device), or None where the kind does not apply to t."""
    if t.dtype not in SENTINEL:
        raise TypeError("layouts: fp32 or uint8 tensors, got %s" % t.dtype)
    t = t.detach()
    shape, r = tuple(t.shape), t.dim()
    if t.numel() == 0 or (r == 0 and kind not in ("planar", "offset")):
        return None
    if kind == "planar":
        return _carve(t, _strides(shape), 0)
    if kind == "cl":
        return _carve(t, _strides(shape, CL), 0) if r == 4 else None
    if kind == "offset":
        return _carve(t, _strides(shape), 1)
    if kind == "offset_cl":
        return _carve(t, _strides(shape, CL), 1) if r == 4 else None
    if kind == "batch_slice":
        return _sub(t, (shape[0] + 2,) + shape[1:], torch.contiguous_format, slice(1, 1 + shape[0]))
    if kind in ("chan_slice", "chan_slice_cl"):
        if r < 2 or (kind == "chan_slice_cl" and r != 4):
            return None
        fmt = CL if kind == "chan_slice_cl" else torch.contiguous_format
        return _sub(t, (shape[0], shape[1] + 2) + shape[2:], fmt, (slice(None), slice(1, 1 + shape[1])))
    if kind == "crop":
        if r < 2:
            return None
        H, W = shape[-2:]
        return _sub(t, shape[:-2] + (H + 2, W + 4), torch.contiguous_format, (Ellipsis, slice(1, 1 + H), slice(2, 2 + W)))
    if kind == "transposed":
        if r < 2 or shape[-1] == 1 or shape[-2] == 1:
            return None
        st = _strides(shape[:-2] + (shape[-1], shape[-2]))
        return _carve(t, st[:-2] + (st[-1], st[-2]), 0)
    if kind == "expanded":
        dims = constant_dims(t)
        if not dims:
            return None
        small = t
        for d in dims:
            small = small.narrow(d, 0, 1)
        st = _strides(tuple(small.shape))
        buf = torch.full((2 * t.numel(),), SENTINEL[t.dtype], dtype=t.dtype, device=t.device)
        buf.as_strided(tuple(small.shape), st).copy_(small)
        return buf.as_strided(shape, tuple(0 if d in dims else s for d, s in enumerate(st)))
    if kind == "size1":
        if 1 not in shape:
            return None
        st = _strides(shape)
        return _carve(t, tuple(SIZE1_STRIDE if n == 1 else s for n, s in zip(shape, st)), 0)
    raise ValueError("layouts: no kind %r" % (kind,))


def views(t, kinds=KINDS):
    """(kind, view) for every kind that applies to the dense fp32 / uint8 tensor t: t's shape and values, other memory."""
    for kind in kinds:
        v = make(t, kind)
        if v is not None:
            yield kind, v


def kinds_for(t, kinds=KINDS):
    return [kind for kind, _ in views(t, kinds)]


def is_cl(v):
    """Whether v's memory is ordered channels-last (a channels_last tensor or a slice of one)."""
    return v.dim() == 4 and v.shape[1] > 1 and v.stride(1) == 1 and (v.shape[3] == 1 or v.stride(3) > 1)


def dense(v):
    """The twin: v's values in a fresh allocation, channels_last if v came from a channels_last kind, else contiguous.
    (.contiguous() would be a no-op for `offset` and `batch_slice`.)"""
    return v.detach().clone(memory_format=CL if is_cl(v) else torch.contiguous_format)


def storage_flat(v):
    """The whole allocation v lives in, as a flat tensor of v's dtype."""
    return torch.empty(0, dtype=v.dtype, device=v.device).set_(v.untyped_storage())


def read_as_dense(v):
    """What a stride-blind reader sees: numel() elements from v's first one."""
    return storage_flat(v)[v.storage_offset():v.storage_offset() + v.numel()]


class _Relayout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, kind):
        ctx.kind = kind
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        v = make(g.contiguous(), ctx.kind)
        if v is None:
            raise ValueError("layouts.relayout: kind %r does not apply to a gradient of shape %s" % (ctx.kind, tuple(g.shape)))
        return v, None


def relayout(y, kind):
    """y itself; in the backward pass the gradient arrives at y's producer re-made as `kind`."""
    return _Relayout.apply(y, kind)


# ---- the matrix: one operator, one argument, one kind ------------------------------------------------------------------------
class Case:
    """One operator at one shape.  fn(**tensors) -> a tensor or a tuple of tensors; `inputs` name -> dense CPU tensor (fp32 or
    uint8), every one of them a pure input; `grads` the inputs whose gradient is compared; ref(**inputs as fp64) -> the same outputs
    computed plainly.  exact: the view run must equal the dense run bit for bit (torch.equal), forward and gradients ("forward": the outputs
    alone, the gradients against the reference); otherwise (operators that add with float atomics) both runs are judged against the
    fp64 reference.  judge(what, got, want) asserts one
    fp32 result `got` close to the fp64 `want` with the tolerance of the operator's own value test; `what` is "out<i>" or
    "d_<name>".  kinds: {name: kinds} narrows the kinds of an argument (default: every kind that applies)."""

    def __init__(self, fn, inputs, ref, judge, grads=(), exact=True, kinds=None, outputs=None, with32=False):
        self.fn, self.inputs, self.ref, self.judge = fn, dict(inputs), ref, judge
        self.grads, self.exact, self.kinds = tuple(grads), exact, dict(kinds or {})
        self.outputs = outputs                 # indices of the differentiable fp32 outputs (default: all)
        self.with32 = with32                   # judge(what, got, want, want32): also the reference's fp32 run on the CPU
        self._ref = {}

    def arg_kinds(self, name):
        return self.kinds.get(name) or kinds_for(self.inputs[name])

    def _cots(self, outs, constant):
        g = torch.Generator().manual_seed(1234)
        return [torch.full(tuple(o.shape), 0.5, dtype=torch.float64) if constant
                else torch.randn(tuple(o.shape), generator=g, dtype=torch.float64) for o in outs]

    def diff_outputs(self, outs):
        return [outs[i] for i in (self.outputs if self.outputs is not None else range(len(outs)))]

    def reference(self, constant=False, dtype=torch.float64):
        """(outputs, gradients by name) in fp64 (or the same formulas in fp32), for the random or the constant (expanded)
        cotangent; computed once."""
        key = constant
        constant = bool(constant)
        if dtype != torch.float64:
            key = (constant, dtype)
        if key not in self._ref:
            args = {k: (v.to(dtype) if v.dtype == torch.float32 else v.clone()) for k, v in self.inputs.items()}
            for k in self.grads:
                args[k].requires_grad_(True)
            outs = _tuple(self.ref(**args))
            grads = {}
            if self.grads:
                d = self.diff_outputs(outs)
                gs = torch.autograd.grad(d, [args[k] for k in self.grads], [c.to(dtype) for c in self._cots(d, constant)], allow_unused=True)
                grads = {k: (g if g is not None else torch.zeros_like(args[k])) for k, g in zip(self.grads, gs)}
            self._ref[key] = ([o.detach() for o in outs], grads)
        return self._ref[key]

    def out_kinds(self):
        """The cotangent kinds: every kind that applies to some differentiable output (`expanded` always does: the cotangent
        is then constant, as the one of .sum() is)."""
        outs = self.diff_outputs(self.reference()[0])
        found = []
        for kind in KINDS:
            probe = [torch.full(tuple(o.shape), 0.5) if kind == "expanded" else torch.randn(tuple(o.shape)) for o in outs]
            if any(make(p, kind) is not None for p in probe) and kind not in found:
                found.append(kind)
        return found

    def run(self, dev, replace=None, cot_kind=None, constant=False):
        """(outputs, gradients by name) on `dev`, as CPU tensors read logically.  replace: name -> device tensor to hand in
        instead of a fresh dense copy; cot_kind: the layout in which the backward receives every cotangent (constant: of 0.5
        everywhere, which `expanded` needs)."""
        replace = replace or {}
        args = {}
        for k, v in self.inputs.items():
            t = replace[k] if k in replace else v.to(dev)
            args[k] = t.detach().requires_grad_(True) if k in self.grads else t
        outs = _tuple(self.fn(**args))
        grads = {}
        if self.grads:
            d = self.diff_outputs(outs)
            cots = [c.float().to(dev) for c in self._cots(d, constant)]
            if cot_kind is not None:
                d = [relayout(o, cot_kind) if make(c, cot_kind) is not None else o for o, c in zip(d, cots)]
            gs = torch.autograd.grad(d, [args[k] for k in self.grads], cots, allow_unused=True)
            grads = {k: (g.detach().cpu() if g is not None else torch.zeros_like(self.inputs[k])) for k, g in zip(self.grads, gs)}
        return [o.detach().cpu() for o in outs], grads

    def compare(self, dev, replace, twins, cot_kind=None):
        """The cell: the run with `replace` against the run with `twins` and against the fp64 reference."""
        constant = cot_kind == "expanded"
        ref_outs, ref_grads = self.reference(constant)
        outs32, grads32 = self.reference(constant, torch.float32) if self.with32 else (None, None)
        extra = lambda r, k: (r[k],) if self.with32 else ()
        got = self.run(dev, replace, cot_kind, constant)
        base = self.run(dev, twins, None if cot_kind is None else "planar", constant)
        for label, (outs, grads) in (("dense", base), ("view", got)):
            if label == "view" and self.exact:
                for i, (a, b) in enumerate(zip(outs, base[0])):
                    assert a.shape == b.shape and torch.equal(a, b), "out%d differs from the dense run" % i
                for k in self.grads:
                    if self.exact == "forward":         # the backward adds with float atomics: against the reference
                        self.judge("d_" + k, grads[k], ref_grads[k], *extra(grads32, k))
                    else:
                        assert grads[k].shape == base[1][k].shape and torch.equal(grads[k], base[1][k]), "d_%s differs from the dense run" % k
                continue
            for i, (a, b) in enumerate(zip(outs, ref_outs)):
                assert tuple(a.shape) == tuple(b.shape), (label, i, a.shape, b.shape)
                self.judge("out%d" % i, a, b, *extra(outs32, i))
            for k in self.grads:
                assert tuple(grads[k].shape) == tuple(ref_grads[k].shape), (label, k)
                self.judge("d_" + k, grads[k], ref_grads[k], *extra(grads32, k))

    def check_input(self, dev, name, kind):
        v = make(self.inputs[name].to(dev), kind)
        assert v is not None, "kind %s does not apply to %s" % (kind, name)
        self.compare(dev, {name: v}, {name: dense(v)})

    def check_cotangent(self, dev, kind):
        self.compare(dev, {}, {}, cot_kind=kind)

    def check_all_at_once(self, dev):
        """Every argument a view, a different kind each (as far as the kinds go round), and the cotangents channels_last or
        at an offset."""
        replace = {}
        for i, name in enumerate(self.inputs):
            kinds = [k for k in self.arg_kinds(name) if k != "planar"]
            replace[name] = make(self.inputs[name].to(dev), kinds[(2 * i + 1) % len(kinds)])
        assert len({tuple(v.stride()) + (v.storage_offset(),) for v in replace.values()}) > 1 or len(replace) == 1
        cot = None
        if self.grads:
            cot = "offset_cl" if "offset_cl" in self.out_kinds() else "offset"
        self.compare(dev, replace, {k: dense(v) for k, v in replace.items()}, cot_kind=cot)


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def input_cells(cases):
    """[(case, argument, kind)] of a dict of cases: the parametrisation of the input half of the matrix."""
    return [(c, name, kind) for c, case in cases.items() for name in case.inputs for kind in case.arg_kinds(name)]


def cotangent_cells(cases):
    return [(c, kind) for c, case in cases.items() if case.grads for kind in case.out_kinds()]
