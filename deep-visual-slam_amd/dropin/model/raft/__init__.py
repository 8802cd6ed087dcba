"""Namespace shim, one level down from model/__init__.py: `core/corr.py` here shadows the reference's, everything else of
model/raft falls through to the reference's own directory further down sys.path (model/__init__.py has already put the
reference's model/ on the parent's __path__)."""
import os
import sys

_here = os.path.dirname(os.path.abspath(__file__))
_parent = sys.modules[__name__.rpartition(".")[0]]
for _p in _parent.__path__:
    _cand = os.path.join(_p, os.path.basename(_here))
    if os.path.isdir(_cand) and os.path.abspath(_cand) != _here and _cand not in __path__:
        __path__.append(_cand)
