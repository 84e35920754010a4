"""CPU-side checks of the fused last encoder stage (ReLU -> BatchNorm1d -> max over the points): the argument validation
of sivae_relu_bn_max_fwd / _bwd (every call returns before any launch), the Python surface of
sivae_hip.pointcloud.relu_bn_max, the module switch and the encoder's route."""
import ctypes
import inspect

import pytest
import torch

from sivae_hip import lib


class _St:
    """what functional.BNState carries"""

    def __init__(self, C, training=True):
        self.running_mean, self.running_var = torch.zeros(C), torch.ones(C)
        self.num_batches_tracked = torch.zeros((), dtype=torch.int64)
        self.training, self.eps, self.momentum = training, 1e-5, 0.1


def test_relu_bn_max_entry_points_validate_arguments():
    """null pointers, non-positive sizes, B C N >= 2^31 - 1: the documented codes, in the manner of
    test_pointcloud_host.py::test_pointcloud_entry_points_validate_arguments"""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    f = L.sivae_relu_bn_max_fwd
    ok = [one] * 7
    for i in range(7):  # a, mean, invstd, gamma, beta, vals, arg
        args = list(ok)
        args[i] = null
        assert f(*args, 2, 4, 8, null) == -1, i
    for shape in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (-1, 4, 8)):
        assert f(*ok, *shape, null) == -2, shape
    assert f(*ok, 1 << 12, 1 << 12, 1 << 12, null) == -5
    assert f(*ok, 1, 1, 0x7fffffff, null) == -5        # (the bound itself is refused)
    b = L.sivae_relu_bn_max_bwd
    ok = [one] * 9
    for i in range(9):  # g, arg, a, mean, invstd, gamma, da, dgamma, dbeta
        args = list(ok)
        args[i] = null
        assert b(*args, 2, 4, 8, null) == -1, i
    for shape in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (2, 4, -3)):
        assert b(*ok, *shape, null) == -2, shape
    assert b(*ok, 1 << 12, 1 << 12, 1 << 12, null) == -5
    assert b(*ok, 0x7fffffff, 1, 1, null) == -5
    assert L.sivae_abi_version() == 1


def test_relu_bn_max_rejects_cpu_tensors_and_wrong_ranks():
    from sivae_hip import pointcloud as PC
    w, b = torch.ones(4), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.relu_bn_max(torch.zeros(2, 4, 8), w, b, _St(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.relu_bn_max_fwd(torch.zeros(2, 4, 8), b, w, w, b)
    with pytest.raises(ValueError, match=r"\[B, C, N\]"):  # (a 2-D input: the shape is checked before the device)
        PC.relu_bn_max(torch.zeros(4, 8), w, b, _St(4))
    for fn in (PC.relu_bn_max_fwd, PC.relu_bn_max_bwd):  # (the neighbours' checks)
        src = inspect.getsource(fn)
        assert "_require_f32(" in src and "_bcn(a)" in src and "timer_end(" in src and "torch.empty" in src
    assert "_require_i32(arg)" in inspect.getsource(PC.relu_bn_max_bwd)


def test_switch_and_encoder_route():
    import soft_intro_vae_3d.models.vae as V
    from sivae_hip import pointcloud as PC
    assert PC.RELU_BN_MAX is True
    src = inspect.getsource(V.Encoder.forward)
    assert "relu_bn_max" in src and "RELU_BN_MAX" in src
    assert "relu_bn_max" not in inspect.getsource(V.EncoderNoBatchNorm.forward)
    assert callable(PC.relu_bn_max) and issubclass(PC.ReluBnMaxFn, torch.autograd.Function)
    assert "relu_bn_max(a [B, C, N], weight, bias, BNState)" in PC.__doc__
