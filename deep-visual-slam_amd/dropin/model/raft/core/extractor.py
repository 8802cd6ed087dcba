"""model/raft/core/extractor.py of the reference, backed by csrc/inorm.hip, the BatchNorm kernels and the convolution kernels:
`from .extractor import BasicEncoder, SmallEncoder` (model/raft/core/raft.py:7) resolves here."""
import os as _os
import sys as _sys

_root = _os.path.abspath(__file__)
for _ in range(6):
    _root = _os.path.dirname(_root)
if _root not in _sys.path:
    _sys.path.insert(0, _root)
from deep_visual_slam_amd.raft_encoder import BasicEncoder, SmallEncoder  # noqa: F401,E402
