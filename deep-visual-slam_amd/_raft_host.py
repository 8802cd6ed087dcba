"""What the host layer of the RAFT family shares (raft, raft_corr, raft_encoder, raft_update, raft_video, posenet_single): the one
argument check and the one cache of operands derived from parameters."""
import weakref

import torch

from . import nn_ops
from ._host import CL, aligned, gpu_arg                 # noqa: F401  (the family imports them from here)


def _drop_on_gradient(owner_ref):
    def hook(grad):
        owner = owner_ref()
        if owner is not None:
            owner._drop()
    return hook


class DerivedOperands:
    """Mixin of an nn.Module whose launches read operands made from its parameters by differentiable torch ops (sliced, stacked,
    zero-padded, channels_last), so that gradients land on the parameters themselves.  The class provides _operands() ->
    (operands, the derived tensors among them) and, to use _hoisted, _context_terms(inp, operands).

    _weights   (stamp, operands), served by _derive() while the stamp holds
    _context   (weakref(inp), (inp._version, inp.requires_grad), terms), served by _hoisted() while `inp` is that object in that
               state and _weights stands
    Under autograd both hold graph nodes; a hook on each drops both slots when its gradient arrives, because the backward pass that
    delivers it frees their graph."""

    def _drop(self):
        self._weights = self._context = None

    def _stamp(self):
        """conv._p16_stamp's rule over every parameter (dp.FusedAdam writes weights behind torch's back and bumps
        nn_ops.generation()), plus what decides whether the derived tensors are graph nodes."""
        return (torch.is_grad_enabled(), nn_ops.generation()) + tuple((id(p), p._version, p.requires_grad) for p in self.parameters())

    def _derive(self):
        stamp = self._stamp()
        if self._weights is not None and self._weights[0] == stamp:
            return self._weights[1]
        w, tensors = self._operands()
        self._weights, self._context = (stamp, w), None
        if torch.is_grad_enabled():
            hook = _drop_on_gradient(weakref.ref(self))
            for t in tensors:
                if t.requires_grad and not t.is_leaf:       # a leaf is the parameter itself: nothing of its graph is freed
                    t.register_hook(hook)
        return w

    def _hoisted(self, inp, w):
        ent = self._context
        key = (inp._version, inp.requires_grad)
        if ent is not None and ent[0]() is inp and ent[1] == key:
            return ent[2]
        c = self._context_terms(inp, w)
        hook = _drop_on_gradient(weakref.ref(self))
        for t in (c if isinstance(c, tuple) else (c,)):
            if t.requires_grad:
                t.register_hook(hook)
        self._context = (weakref.ref(inp), key, c)
        return c
