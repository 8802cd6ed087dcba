"""model/raft/core/corr.py of the reference, backed by csrc/corr.hip: `from .corr import CorrBlock, AlternateCorrBlock`
(model/raft/core/raft.py:8) resolves here."""
import os as _os
import sys as _sys

_root = _os.path.abspath(__file__)
for _ in range(6):
    _root = _os.path.dirname(_root)
if _root not in _sys.path:
    _sys.path.insert(0, _root)
from deep_visual_slam_amd.raft_corr import CorrBlock  # noqa: F401,E402


class AlternateCorrBlock:
    """The on-the-fly form (model/raft/core/corr.py:63-91 over model/raft/alt_cuda_corr/): not implemented.  The reference
    constructs its networks with alternate_corr=False (model/posenet_single.py), so CorrBlock is the one in use."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("AlternateCorrBlock (alt_cuda_corr) is not implemented; use CorrBlock (alternate_corr=False)")
