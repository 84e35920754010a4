"""GPU checks of the style variant's fused_scale convolutions on every route a layer can take: the rows EDGE of
tests/test_style_scale_conv_host.py (tests/test_style_scale_edges_host.py says what each is for and holds them to the
route functions), through the checks of tests/test_style_scale_conv_gpu.py.

The rows whose property depends on the number of CUs (the 64-row maps: one work item of the pooled F(4x4,3x3) kernel per
CU, or one image less) take their batch size from the device, B = cdiv(CUs, 32), which is the table's 8 at 256 CUs.  Every
test asserts the family ops.conv2d_up_dgrad_route gives on the device before it compares anything.

Tolerances.  Against the float64 CPU formula of the reference's form, kernel_checks._err: the tensor the pooled
F(4x4,3x3) kernel writes (dx of "up", y of "down" on a wino4_pool row) is held to kernel_checks.WINO4_TOL, the figure
that kernel is held to with a plain weight; everything else, dw on every row included, to kernel_checks.WINO_TOL.
Networks: test_style_model_gpu.CLASS_GRAD_GATE, as in test_style_scale_conv_gpu.py.

Measured on an MI355X (256 CUs), worst over the rows of a route and both kinds (y, dx, dw):
    wino4_pool (conv_wino4_pool_kernel<false>)                      4.18e-06  4.10e-06  6.43e-07
    wino_up_dgrad (conv_wino_up_dgrad_kernel<1,4>)                  5.73e-07  6.30e-07  7.38e-07
    wino_up_dgrad (conv_wino_up_dgrad_kernel<2,3>)                  2.52e-07  2.81e-07  5.36e-07
    wino_up_dgrad_splitk (conv_wino_up_dgrad_kernel<1,4>)           8.17e-07  9.22e-07  6.33e-07
    wino_up_dgrad_splitk (conv_wino_up_dgrad_kernel<2,3>)           7.92e-07  9.08e-07  8.63e-07
On (8, 16, 16, 64, 64) the pooled kernel is at 3.65e-06 (dx of "up") and 3.08e-06 (y of "down") where the phase form of the
same call is at 3.78e-07 and 4.17e-07: ten times the phase form's error, inside WINO_TOL here and a tenth of WINO4_TOL.
The networks whose fused_scale layer takes the pooled kernel, switch on against off: Generator 2.75e-06, Encoder 4.84e-06
(gate 1e-04)."""
import pytest
import torch

import kernel_checks as K
import test_style_model_gpu as TM
import test_style_scale_conv_gpu as C
from test_style_scale_conv_gpu import case, conv_module, module_run, oracle, put, run, torch_lines  # noqa: F401
from test_style_scale_conv_host import EDGE
from test_style_scale_edges_host import cdiv, wgrad_slices

pytestmark = pytest.mark.gpu

KINDS = C.KINDS
blocks = C.blocks
POOL_ROW, WIDE_SPLIT, CAP_SPLIT, TWO_SLICES = (8, 16, 16, 64, 64), (1, 128, 128, 8, 32), (1, 128, 512, 8, 16), (5, 4, 6, 10, 40)
NET_CFG = dict(startf=16, maxf=16, layer_count=6, latent_size=8)  # one fused_scale layer, 16 channels at 128 x 128
ids = lambda s: "x".join(map(str, s))  # noqa: E731
WORST = {}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_device(shape):
    """the row as the device at hand needs it: the 64-row maps are sized so that B = 8 is one work item of the pooled
    kernel per CU at 256 CUs"""
    B = shape[0] + (cdiv(cus(), 32) - 8 if shape[3] == 64 else 0)
    assert B > 0
    return (B,) + tuple(shape[1:])


def held(kind, row):
    """asserts the property the row is in the table for, on this device -> (the row as run, its family)"""
    from sivae_hip import ops
    conv_key, adj_key, family, split, slices = EDGE[row]
    shape = on_device(row)
    B, Cl, Cf, h, w = shape
    adj = ops.conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, has_wp1=True)
    assert (adj.family, adj.key, adj.split) == (family, adj_key, split), (row, shape, cus())
    r = ops.scale_conv_routes(kind, *C.layer_args(kind, shape))
    assert r.refused is None and adj == (r.dgrad if kind == "up" else r.forward)
    assert (r.dgrad if kind == "down" else r.forward).key == conv_key
    got = wgrad_slices(r.wgrad, shape)
    assert (got > 1) == (slices > 1) and (got == slices or cus() != 256), (row, got)
    return shape, family


def gates(kind, family):
    """(y, dx, dw): WINO4_TOL for what the pooled kernel writes, WINO_TOL for the rest"""
    g = dict(y=K.WINO_TOL, dx=K.WINO_TOL, dw=K.WINO_TOL)
    if family == "wino4_pool":
        g["dx" if kind == "up" else "y"] = K.WINO4_TOL
    return g


# ------------------------------------------------------------------------------------------------ the functions
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", list(EDGE), ids=ids)
def test_functions_against_the_reference_form(row, kind):
    shape, family = held(kind, row)
    (x, w, gy), (y_ref, dx_ref, dw_ref) = case(kind, shape)
    y, dx, dw, wg = run(kind, x, w, gy)
    errs = dict(y=K._err(y, y_ref), dx=K._err(dx, dx_ref), dw=K._err(dw, dw_ref))
    gate = gates(kind, family)
    print("conv_%sscale %s %s: %s" % (kind, shape, family, ", ".join("%s %.2e (gate %.0e)" % (k, e, gate[k])
                                                                       for k, e in errs.items())))
    worst = WORST.setdefault(family + " / " + EDGE[row][1], dict(y=0.0, dx=0.0, dw=0.0))
    for k, e in errs.items():
        worst[k] = max(worst[k], e)
    print("worst so far: " + "; ".join("%s: %s" % (f, ", ".join("%s %.2e" % kv for kv in v.items()))
                                       for f, v in sorted(WORST.items())))
    assert dw.shape == wg.shape and dx.shape == x.shape
    for k, e in errs.items():
        assert e <= gate[k], (k, e)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [POOL_ROW, WIDE_SPLIT, TWO_SLICES], ids=ids)
def test_the_function_is_the_three_ops(row, kind):
    from sivae_hip import ops
    shape, family = held(kind, row)
    (y, dx, dw), (xg, gyg, wp0, wp1) = C.three_ops(kind, shape)
    if family != "wino4_pool":
        return
    # the same call without the mode-1 pack: the phase-form kernel, right too, and not the pooled one's bits (a pooled
    # route that silently stops being taken shows here)
    B, Cl, Cf, h, w = shape
    assert ops.conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, has_wp1=False).family == "wino_up_dgrad"
    _, ref = case(kind, shape)
    pooled, want, src = (dx, ref[1], gyg) if kind == "up" else (y, ref[0], xg)
    plain = ops.conv2d_up_dgrad(src, wp0, Cl)
    assert torch.equal(pooled, ops.conv2d_up_dgrad(src, wp0, Cl, wp1=wp1))
    print("%s %s: pooled %.2e, phase form %.2e" % (kind, shape, K._err(pooled, want), K._err(plain, want)))
    assert K._err(plain, want) <= K.WINO_TOL and K._err(pooled, want) <= K.WINO4_TOL
    assert not torch.equal(plain, pooled)


# ------------------------------------------------------------------------------------------------ the cache
@pytest.mark.parametrize("kind", KINDS)
def test_a_stale_mode1_pack_would_show(blocks, kind):
    """after an in-place edit, an LREQAdam step and a weight average: "down" reads the mode-1 pack in the forward, "up" in
    the data gradient, which is held to the current weight's as well"""
    shape, family = held(kind, POOL_ROW)
    assert family == "wino4_pool"
    g = gates(kind, family)
    C.stale_weight(blocks, kind, shape, tol=g["y"], dx_tol=g["dx"])


# ------------------------------------------------------------------------------------------------ guarded
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [POOL_ROW, CAP_SPLIT, TWO_SLICES], ids=ids)
def test_guarded(row, kind):
    C.guarded_run(held(kind, row)[0], (kind,))


# ------------------------------------------------------------------------------------------------ slabs, wanted gradients
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_slabs(kind):
    C.gradient_slabs(kind, held(kind, POOL_ROW)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_only_wanted_gradients_are_launched(monkeypatch, kind):
    C.wanted_gradients(monkeypatch, kind, held(kind, POOL_ROW)[0])


# ------------------------------------------------------------------------------------------------ _Conv3x3
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [POOL_ROW, WIDE_SPLIT], ids=ids)
def test_the_module_calls_no_torch_convolution(blocks, monkeypatch, row, kind):
    shape, family = held(kind, row)
    g = gates(kind, family)
    C.no_torch_convolution(blocks, monkeypatch, kind, shape, tols=(g["y"], g["dx"], g["dw"]))


# ------------------------------------------------------------------------------------------------ the networks
@pytest.mark.parametrize("cls", ["Generator", "Encoder"])
def test_networks_on_the_pooled_route_with_the_switch_on_against_off(blocks, monkeypatch, cls):
    """test_style_scale_conv_gpu's criterion and gate on networks whose one fused_scale layer (16 -> 16 channels, 64 x 64
    and 128 x 128) takes the pooled kernel: in the backward of the Generator, in the forward of the Encoder"""
    from sivae_hip import ops
    batch = cdiv(cus(), 32)
    route, seen = ops.conv2d_up_dgrad_route, []

    def spy(*a, **k):
        r = route(*a, **k)
        if "dx_al8" in k:  # (the launch's own question; scale_conv_routes asks without it)
            # (inside the engine's run of a graph, i.e. a backward pass, or outside one)
            seen.append((r.family, "forward" if torch._C._current_graph_task_id() == -1 else "backward", a))
        return r

    ops.conv2d_up_dgrad_route = spy
    try:
        errs, layer = C.switch_on_against_off(blocks, monkeypatch, cls, NET_CFG, batch)
    finally:
        ops.conv2d_up_dgrad_route = route
    conv = layer.conv_1 if cls == "Generator" else layer.conv_2
    assert tuple(conv.weight.shape) == (16, 16, 3, 3)
    assert [s[:2] for s in seen] == [("wino4_pool", "backward" if cls == "Generator" else "forward")], seen
    assert seen[0][2] == (batch, 16, 16, 128, 128)
    assert max(errs.values()) <= TM.CLASS_GRAD_GATE
