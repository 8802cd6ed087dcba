"""model/raft/core/raft.py of the reference, backed by raft.py of this package: `from model.raft.core.raft import SmallRAFT`
(model/posenet_single.py:103, model/raft/raft.py:47) and `from model.raft.core.raft import RAFT` resolve here, with the names the
reference's module carries (CorrBlock, AlternateCorrBlock, BasicEncoder, SmallEncoder, BasicUpdateBlock, SmallUpdateBlock,
coords_grid, upflow8).  RAFT is the full-size model (BasicEncoder, SepConvGRU on the shift-stack kernels, the mask head and the
fused convex upsampling).  `update.py` is not shadowed: `model.raft.core.update` stays the reference's file, and the two models
take their update blocks from this package directly."""
import os as _os
import sys as _sys

_root = _os.path.abspath(__file__)
for _ in range(6):
    _root = _os.path.dirname(_root)
if _root not in _sys.path:
    _sys.path.insert(0, _root)
from deep_visual_slam_amd.raft import (RAFT, AlternateCorrBlock, BasicEncoder, BasicUpdateBlock, CorrBlock,  # noqa: F401,E402
                                       SmallEncoder, SmallRAFT, SmallUpdateBlock, coords_grid, upflow8, upsample_flow)
