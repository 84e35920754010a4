"""Drop-in for the reference's style_soft_intro_vae/custom_adam.py: with this directory in front of the reference's on
PYTHONPATH, the training script's `from custom_adam import LREQAdam` gets the optimizer whose step is one multi-tensor HIP
launch per network instead of five element-wise launches per tensor (sivae_hip/lreq_adam.py).

`lerp_parameters` is the weight average: in the reference's model.py, replace lines 328-329 (the loop over the two zipped
parameter lists and its per-tensor `lerp_`) with

    lerp_parameters(params, other_param, 1.0 - betta)

after `from custom_adam import lerp_parameters`.
"""
from sivae_hip.lreq_adam import LREQAdam, lerp_parameters

__all__ = ["LREQAdam", "lerp_parameters"]
