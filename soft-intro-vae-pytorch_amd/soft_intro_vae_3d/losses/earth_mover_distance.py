"""EMD: the 'earth_mover' reconstruction loss that the reference's soft_intro_vae_3d/train_soft_intro_vae_3d.py:171-176
names (the project it derives from trains with losses/earth_mover_distance.py::EMD on the approxmatch / matchcost /
matchcostgrad extension), on the HIP kernel of csrc/pc_emd.hip."""
import os
import sys

import torch.nn as nn

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (where sivae_hip lies)
if _PKG not in sys.path:
    sys.path.append(_PKG)
from sivae_hip import pointcloud as PC  # noqa: E402


class EMD(nn.Module):
    """forward(preds [B, N, 3], gts [B, M, 3]) -> [B]: the cost of the approximate matching of Fan, Su and Guibas with
    preds on the matching's left side and gts on its right, unnormalised like ChamferLoss (the loop's
    scale = 1 / (3 n_points) applies unchanged).  The gradients are matchcostgrad's: the plan is held constant, so
    torch.autograd.gradcheck does not apply.  At most 4096 points a cloud."""

    def __init__(self):
        super().__init__()
        self.use_cuda = True

    def forward(self, preds, gts):
        return PC.emd_distance(preds, gts)
