"""Namespace shim: `corr.py` here shadows the reference's model/raft/core/corr.py; raft.py, update.py, extractor.py and utils/
still come from the reference's own directory (found through the parent package's __path__)."""
import os
import sys

_here = os.path.dirname(os.path.abspath(__file__))
_parent = sys.modules[__name__.rpartition(".")[0]]
for _p in _parent.__path__:
    _cand = os.path.join(_p, os.path.basename(_here))
    if os.path.isdir(_cand) and os.path.abspath(_cand) != _here and _cand not in __path__:
        __path__.append(_cand)
