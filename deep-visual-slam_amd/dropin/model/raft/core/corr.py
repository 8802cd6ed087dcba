"""model/raft/core/corr.py of the reference, backed by csrc/corr.hip: `from .corr import CorrBlock, AlternateCorrBlock`
(model/raft/core/raft.py:8) resolves here.  AlternateCorrBlock is the on-the-fly form (alternate_corr=True, raft.py:204-205):
the same function as CorrBlock without the all-pairs volume."""
import os as _os
import sys as _sys

_root = _os.path.abspath(__file__)
for _ in range(6):
    _root = _os.path.dirname(_root)
if _root not in _sys.path:
    _sys.path.insert(0, _root)
from deep_visual_slam_amd.raft_corr import AlternateCorrBlock, CorrBlock  # noqa: F401,E402
