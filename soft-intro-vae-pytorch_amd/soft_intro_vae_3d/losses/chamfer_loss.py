"""ChamferLoss of the reference's soft_intro_vae_3d/losses/chamfer_loss.py on the HIP Chamfer kernels."""
import os
import sys

import torch.nn as nn

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (where sivae_hip lies)
if _PKG not in sys.path:
    sys.path.append(_PKG)
from sivae_hip import pointcloud as PC  # noqa: E402


class ChamferLoss(nn.Module):
    """forward(preds [B, M, 3], gts [B, N, 3]) -> [B]: sum of squared nearest-neighbour distances, both directions
    (reference :11-17).  Distances are formed directly (dx^2 + dy^2 + dz^2), not by the reference's expansion."""

    def __init__(self):
        super().__init__()
        self.use_cuda = True

    def forward(self, preds, gts):
        return PC.chamfer_distance(preds, gts)
