"""fovealseg -- MI355X-native FovealSeg forward/backward hot path.

Host side mirrors the reference plugin surface (`ModelBuilder`, `DeformSegmentationModule`;
/root/reference/models/models.py:476-1230); every op below that surface is a hand-written HIP
kernel for gfx950 reached through the C-ABI library declared in include/fovealseg.h.
"""
from . import config, weights, hip, frames, masks, gaze, overlay, unwarp, ops, modules, models, data, session  # noqa: F401
from .models import ModelBuilder, DeformSegmentationModule  # noqa: F401
from .config import lvis50_cfg  # noqa: F401
from .session import GazeSession  # noqa: F401

__all__ = ["config", "weights", "hip", "frames", "masks", "gaze", "overlay", "unwarp", "ops", "modules", "models", "data", "session",
           "ModelBuilder", "DeformSegmentationModule", "GazeSession", "lvis50_cfg"]
