"""model/raft/core/raft.py of the reference, backed by raft.py of this package: `from model.raft.core.raft import SmallRAFT`
(model/posenet_single.py:103, model/raft/raft.py:47) resolves here, with the names the reference's module carries (CorrBlock,
AlternateCorrBlock, SmallEncoder, SmallUpdateBlock, coords_grid, upflow8).  RAFT, the full-size model, is a name whose
constructor raises NotImplementedError: BasicEncoder, SepConvGRU and the mask head are not built.  `update.py` is not shadowed:
`model.raft.core.update` stays the reference's file, and SmallRAFT takes its update block from this package directly."""
import os as _os
import sys as _sys

_root = _os.path.abspath(__file__)
for _ in range(6):
    _root = _os.path.dirname(_root)
if _root not in _sys.path:
    _sys.path.insert(0, _root)
from deep_visual_slam_amd.raft import (RAFT, AlternateCorrBlock, CorrBlock, SmallEncoder, SmallRAFT,  # noqa: F401,E402
                                       SmallUpdateBlock, coords_grid, upflow8)
