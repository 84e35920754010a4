"""Keeps the rows of the fused_scale convolution tests in step with the route functions, without a GPU (the library's
predicates answer for 256 CUs where there is no device): every kernel signature ops.scale_conv_routes can choose over a
grid of layers must have a row in TAKEN or EDGE of tests/test_style_scale_conv_host.py (which test_style_scale_conv_gpu.py
and test_style_scale_edges_gpu.py run), and the thresholds the rows straddle are read out of the sources, so that a
moved one fails here with the name of the kind of row that is missing; a reformatted predicate fails with "not in the
shape this test reads".

A shape is (B, Cl, Cf, h, w) as in test_style_scale_conv_host.py.  What the EDGE rows are for:
    (8, 16, 16, 64, 64)    wino4_pool (the pooled F(4x4,3x3) kernel, the only reader of the mode-1 pack of the effective
                           weight) with exactly one work item per CU; Cl = Cf, so that the mode-0 and mode-1 operands have
                           one size; a weight gradient of 512 stages in 32 slices
    (8, 5, 24, 64, 64)     wino4_pool with ragged channels on both sides
    (8, 3, 65, 64, 64)     wino4_pool behind three output-channel tiles of conv_wino_up_kernel<1,4>: 768 work items, more
                           than its persistent grid of 2 x CUs blocks
    (8, 64, 16, 64, 64), (8, 65, 16, 64, 64)    the two sides of N <= 64: pool, and the phase form <1,4> unsplit
    (7, 16, 16, 64, 64)    one image short of one item per CU: the same layer on wino_up_dgrad
    (8, 16, 15, 64, 64), (8, 16, 16, 64, 72)    C < 16, and a full-resolution width of no whole tiles: not pool
    (1, 128, 128, 8, 32)   split-K of the phase data gradient on the wide tile, S = 2 (the ffhq256 layers at B = 4)
    (1, 128, 256, 8, 16), (1, 128, 512, 8, 16)    S = 4 and S = 8 (the cap)
    (5, 4, 6, 10, 40)      wide tile, partial in both directions; 45 stages in 2 slices of 23 and 22
    (1, 3, 5, 9, 18)       odd low-resolution height
    the nine rows below them    the other combinations of tile, split and one / several slices the sweep meets"""
import functools
import os
import re

import pytest

from test_style_scale_conv_host import EDGE, FFHQ256, TAKEN, layer_args

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd")
CUS = 256  # what the library assumes without a device, and what an MI355X has
FAMILIES = {"wino_up", "wino_up_dgrad", "wino_up_dgrad_splitk", "wino4_pool", "wino_up_wgrad"}
READS = "is not in the shape this test reads"
KINDS = ("up", "down")
ROWS = {**TAKEN, **EDGE}


def cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def source(*path):
    with open(os.path.join(PKG, *path)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def defines(text):
    return {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\b", text, re.M)}


def found(pattern, text, what):
    m = re.search(pattern, text, re.S)
    assert m, "%s %s" % (what, READS)
    return [int(g) for g in m.groups()]


@pytest.fixture(scope="module")
def consts():
    """the numbers the route predicates compare with, read out of the sources"""
    c = {}
    w4 = source("csrc", "conv_wino4.hip")
    d = defines(w4)
    assert {"W4_PXH", "W4_PXW", "W4_TCO"} <= set(d), "the tile constants of conv_wino4.hip " + READS
    c.update(pxh=d["W4_PXH"], pxw=d["W4_PXW"], tco=d["W4_TCO"])
    c["c_min"], c["n_max"] = found(
        r"int sivae_conv2d_wino4_dgrad_pool_pays\(int B, int C, int N, int H, int W\) \{\s*"
        r"if \(B <= 0 \|\| C < (\d+) \|\| N <= 0 \|\| N > (\d+) \|\| sivae_conv2d_wino4_supported\(H, W\) != 1\) return 0;\s*"
        r"return w4_px_tiles\(B, H, W\) \* \(\(N \+ W4_TCO - 1\) / W4_TCO\) >= sivae_num_cus\(\) \? 1 : 0;",
        w4, "sivae_conv2d_wino4_dgrad_pool_pays")
    assert "return (H >= 16 && W >= 32 && (H % W4_PXH) == 0 && (W % W4_PXW) == 0) ? 1 : 0;" in w4, \
        "sivae_conv2d_wino4_supported " + READS
    assert "return ipi > 1 ? B / ipi : (long long)B * (H / W4_PXH) * (W / W4_PXW);" in w4, "w4_px_tiles " + READS
    wud = source("csrc", "conv_wino_up_dgrad.hip")
    d = defines(wud)
    assert {"WUD_TN", "WUD_CK"} <= set(d), "the tile constants of conv_wino_up_dgrad.hip " + READS
    c.update(tn=d["WUD_TN"], ck=d["WUD_CK"])
    (c["split_n"], c["wide_w"], c["wide_h"], c["narrow_h"], c["wide_pw"], c["narrow_pw"], c["min_chunks"], c["per_slice"],
     per_slice2, cap, cap2) = found(
        r"if \(!enabled \|\| N <= (\d+) \|\| \(\(Hs \* Ws\) & 3\)\) return 1;\s*"
        r"const int pxh = Ws >= (\d+) \? (\d+) : (\d+), pxw = Ws >= \d+ \? (\d+) : (\d+);\s*"
        r"const long long items = \(long long\)B \* cdiv\(Hs, pxh\) \* cdiv\(Ws, pxw\) \* cdiv\(N, WUD_TN\);\s*"
        r"const int nch = wud_cpad\(C\) / WUD_CK;[^\n]*\s*"
        r"const int cus = wud_grid_blocks\(\) / 2;\s*"
        r"if \(items > cus \|\| nch < (\d+)\) return 1;\s*"
        r"int S = \(int\)\(2 \* cus / items\);\s*"
        r"if \(S > nch / (\d+)\) S = nch / (\d+);[^\n]*\s*"
        r"if \(S > (\d+)\) S = (\d+);\s*"
        r"return S < 2 \? 1 : S;", wud, "sivae_conv2d_wino_up_dgrad_splitk")
    assert per_slice2 == c["per_slice"] and cap2 == cap, "sivae_conv2d_wino_up_dgrad_splitk " + READS
    c["cap"] = cap
    assert "g = 2 * cus;" in wud, "wud_grid_blocks " + READS
    wuw = source("csrc", "conv_wino_up_wgrad.hip")
    d = defines(wuw)
    assert {"WUW_CIT", "WUW_COT"} <= set(d), "the tile constants of conv_wino_up_wgrad.hip " + READS
    c.update(cit=d["WUW_CIT"], cot=d["WUW_COT"])
    c["sh"], c["sw"], c["blocks"], c["stages"], stages2 = found(
        r"p->nrh = cdiv\(Hs, (\d+)\);\s*p->nrw = cdiv\(Ws, (\d+)\);.*?"
        r"int n_slices = cdiv\((\d+), ntiles\);\s*"
        r"const int max_slices = p->nstages / (\d+) > 0 \? p->nstages / (\d+) : 1;\s*"
        r"if \(n_slices > max_slices\) n_slices = max_slices;\s*"
        r"p->sps = cdiv\(p->nstages, n_slices\);\s*"
        r"p->n_slices = cdiv\(p->nstages, p->sps\);", wuw, "wuw_plan")
    assert stages2 == c["stages"], "wuw_plan " + READS
    assert "return (size_t)p.n_slices * 16 * p.Co_pad * p.Ci_pad * sizeof(float);" in wuw, \
        "sivae_conv2d_wino_up_wgrad_workspace_bytes " + READS
    wup = source("csrc", "conv_wino_up.hip")
    d = defines(wup)
    assert "WUP_TCO" in d and "g = 2 * cus;" in wup, "the grid of conv_wino_up.hip " + READS
    assert "static inline bool wup_wide(int W) { return (W >> 1) >= %d; }" % c["wide_w"] in wup, "wup_wide " + READS
    c["up_tco"] = d["WUP_TCO"]
    ops_py = source("sivae_hip", "ops.py")
    assert 'key="conv_wino_up_kernel<%s,%s>" % ("1,4" if W >= ' + str(2 * c["wide_w"]) + ' else "2,3", _tf(pro))' in ops_py \
        and 'key = "conv_wino_up_dgrad_kernel<%s>" % ("1,4" if W // 2 >= ' + str(c["wide_w"]) + ' else "2,3")' in ops_py, \
        "the kernel keys of ops.conv2d_fwd_route / conv2d_up_dgrad_route are " + READS[3:]
    return c


def wgrad_slices(route, shape):
    """slices of the upsample weight gradient, from the workspace its route asks for (16 floats per weight and slice)"""
    d = defines(source("csrc", "conv_wino_up_wgrad.hip"))
    _, Cl, Cf, _, _ = shape
    per = 16 * cdiv(Cl, d["WUW_CIT"]) * d["WUW_CIT"] * cdiv(Cf, d["WUW_COT"]) * d["WUW_COT"] * 4
    assert route.family == "wino_up_wgrad" and route.ws_bytes % per == 0
    return route.ws_bytes // per


def plan_slices(c, shape):
    """wuw_plan restated with the constants read: (stages, stages per slice, slices, which bound held)"""
    B, Cl, Cf, h, w = shape
    stages = B * cdiv(h, c["sh"]) * cdiv(w, c["sw"])
    by_blocks, by_stages = cdiv(c["blocks"], cdiv(Cl, c["cit"]) * cdiv(Cf, c["cot"])), max(stages // c["stages"], 1)
    sps = cdiv(stages, min(by_blocks, by_stages))
    return stages, sps, cdiv(stages, sps), "blocks" if by_blocks < by_stages else "stages"


def taken(kind, shape):
    """-> (the routes, the upsample convolution's, its phase data gradient's: the same two ops in either kind)"""
    from sivae_hip import ops
    r = ops.scale_conv_routes(kind, *layer_args(kind, shape))
    if r.refused:
        return r, None, None
    return (r, r.forward, r.dgrad) if kind == "up" else (r, r.dgrad, r.forward)


def signature(kind, shape):
    """what a layer runs, reduced to what a row can stand for (None: refused)"""
    r, conv, adj = taken(kind, shape)
    if r.refused:
        return None
    for x in (conv, adj, r.wgrad):
        assert x.family in FAMILIES, "%s of %s %s is not a route this test knows" % (x.family, kind, shape)
    assert conv.family == "wino_up" and r.wgrad.family == "wino_up_wgrad" and adj.family not in ("wino_up", "wino_up_wgrad"), \
        "%s %s: %s / %s / %s is not a route this test knows" % (kind, shape, conv.family, adj.family, r.wgrad.family)
    split = {1: "1", 2: "2", 8: "8"}.get(adj.split, "3-7")
    assert 1 <= adj.split <= 8
    return "%s + %s %s split %s + %s slices %s" % (conv.key, adj.family, adj.key, split, r.wgrad.family,
                                                    "1" if wgrad_slices(r.wgrad, shape) == 1 else ">1")


# ------------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(EDGE), ids=lambda s: "x".join(map(str, s)))
def test_routes_of_the_edge_shapes(shape, kind):
    from sivae_hip import ops
    conv_key, adj_key, adj_family, split, slices = EDGE[shape]
    r, conv, adj = taken(kind, shape)
    assert r.refused is None
    assert (conv.family, conv.key, conv.ws_bytes) == ("wino_up", conv_key, 0)
    assert (adj.family, adj.key, adj.split) == (adj_family, adj_key, split)
    assert (adj.ws_bytes > 0) == (split > 1)
    B, Cl, Cf, h, w = shape
    if split > 1:  # (the exact workspace: S partial results)
        assert adj.ws_bytes == split * B * Cl * h * w * 4
    assert (adj.operand, adj.entry) == (("wino4", "sivae_conv2d_wino4_dgrad_pool") if adj_family == "wino4_pool" else
                                        ("wino_up_dgrad", "sivae_conv2d_wino_up_dgrad" + ("_splitk_run" if split > 1 else "")))
    assert (r.wgrad.family, r.wgrad.key) == ("wino_up_wgrad", "wino_up_wgrad_kernel")
    assert wgrad_slices(r.wgrad, shape) == slices
    assert all(x.error is None for x in (r.forward, r.dgrad, r.wgrad))
    assert conv == ops.conv2d_fwd_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)
    assert adj == ops.conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, has_wp1=True)
    assert r.wgrad == ops.conv2d_wgrad_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)
    # without the mode-1 pack, or into a destination that is not 8-byte aligned, the same call is a phase-form one
    for flags in (dict(has_wp1=False), dict(has_wp1=True, dx_al8=False)):
        assert ops.conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, **flags).family in ("wino_up_dgrad", "wino_up_dgrad_splitk")


def test_taken_rows_have_one_slice():
    """(what EDGE adds to TAKEN's layout is 1 in every row of TAKEN)"""
    for shape in TAKEN:
        for kind in KINDS:
            assert wgrad_slices(taken(kind, shape)[0].wgrad, shape) == 1


def test_the_rows_say_what_the_docstring_says(consts):
    """the properties the rows were chosen for that are no part of a route: counts of work items, slices and tiles"""
    c = consts
    pool_items = lambda s: s[0] * (2 * s[3] // c["pxh"]) * (2 * s[4] // c["pxw"]) * cdiv(s[1], c["tco"])  # noqa: E731
    up_items = lambda s: s[0] * cdiv(s[3], c["wide_h"]) * cdiv(s[4], c["wide_pw"]) * cdiv(s[2], c["up_tco"])  # noqa: E731
    assert pool_items((8, 16, 16, 64, 64)) == CUS and pool_items((7, 16, 16, 64, 64)) == CUS - 32
    assert plan_slices(c, (8, 16, 16, 64, 64))[:3] == (512, 16, 32)
    assert up_items((8, 3, 65, 64, 64)) == 768 > 2 * CUS >= max(up_items(s) for s in ROWS if s != (8, 3, 65, 64, 64))
    assert plan_slices(c, (5, 4, 6, 10, 40))[:3] == (45, 23, 2)
    assert (10 % c["wide_h"], 40 % c["wide_pw"]) == (2, 8) and 40 >= c["wide_w"]  # (partial in both directions)
    # the ffhq256 signature: 256 work items on the wide tile over 8 channel chunks, S = 2
    for kind, Ci, Co, side in (FFHQ256[0], FFHQ256[3]):
        Cl, Cf, h = (Ci, Co, side) if kind == "up" else (Co, Ci, side // 2)
        _, _, adj = taken(kind, (4, Cl, Cf, h, h))
        assert (adj.family, adj.key, adj.split) == ("wino_up_dgrad_splitk", "conv_wino_up_dgrad_kernel<1,4>", 2)
        assert 4 * cdiv(h, c["wide_h"]) * cdiv(h, c["wide_pw"]) * cdiv(Cl, c["tn"]) == 256 and cdiv(Cf, c["ck"]) == 8
    _, _, adj = taken("up", (1, 128, 128, 8, 32))
    assert (adj.family, adj.key, adj.split) == ("wino_up_dgrad_splitk", "conv_wino_up_dgrad_kernel<1,4>", 2)


# ------------------------------------------------------------------------------------------------ closure
GRID_B = (1, 2, 4, 7, 8, 16)
GRID_C = (3, 15, 16, 64, 65, 128, 256, 512)
GRID_HW = ((8, 16), (9, 18), (10, 40), (16, 32), (64, 64), (64, 72), (128, 128))


def covered():
    return {signature(kind, shape) for shape in ROWS for kind in KINDS}


def test_every_signature_of_the_grid_has_a_row(consts):
    have, missing, n = covered(), {}, 0
    assert None not in have
    for B in GRID_B:
        for Cl in GRID_C:
            for Cf in GRID_C:
                for hw in GRID_HW:
                    for kind in KINDS:
                        shape = (B, Cl, Cf) + hw
                        sig = signature(kind, shape)
                        assert sig is not None, (kind, shape)  # (no layer of the grid is refused)
                        n += 1
                        if sig not in have:
                            missing.setdefault(sig, (kind, shape))
                        r = taken(kind, shape)[0]
                        assert wgrad_slices(r.wgrad, shape) == plan_slices(consts, shape)[2], (kind, shape)
    print("%d layers, %d signatures, %d of them among the rows" % (n, len(have | set(missing)), len(have)))
    assert not missing, "no row of TAKEN or EDGE runs: " + "; ".join("%s (as %s %s does)" % (k, v[0], v[1])
                                                                      for k, v in sorted(missing.items()))


@pytest.mark.parametrize("B", [4, 8])
def test_the_ffhq256_layers_have_rows(B):
    have = covered()
    for kind, Ci, Co, side in FFHQ256:
        shape = (B, Ci, Co, side, side) if kind == "up" else (B, Co, Ci, side // 2, side // 2)
        assert layer_args(kind, shape) == (B, Ci, Co, side, side)
        assert signature(kind, shape) in have, (kind, Ci, Co, side, signature(kind, shape))


def test_an_unknown_family_is_named(monkeypatch):
    from sivae_hip import ops
    new = ops.Route("wino8_pool", "sivae_conv2d_wino8", "wino4", "a", key="k")
    monkeypatch.setattr(ops, "conv2d_up_dgrad_route", lambda *a, **k: new)
    with pytest.raises(AssertionError, match="not a route this test knows"):
        signature("up", (2, 8, 6, 8, 16))
    monkeypatch.undo()
    assert signature("up", (2, 8, 6, 8, 16)) in covered()


# ------------------------------------------------------------------------------------------------ the thresholds
def family(kind, shape):
    return taken(kind, shape)[2].family


def test_every_threshold_has_a_row_on_each_side(consts):
    """the numbers read out of the sources against the rows: a moved threshold leaves one side without a row"""
    c = consts
    assert CUS % 32 == 0
    pool = [s for s in ROWS if ROWS[s][2] == "wino4_pool"]
    rest = [s for s in ROWS if ROWS[s][2] != "wino4_pool"]
    whole = lambda s: (2 * s[3]) % c["pxh"] == 0 and (2 * s[4]) % c["pxw"] == 0  # noqa: E731
    items = lambda s: s[0] * (2 * s[3] // c["pxh"]) * (2 * s[4] // c["pxw"]) * cdiv(s[1], c["tco"])  # noqa: E731
    takes = lambda s, but=None: [but == k or ok for k, ok in (("n", s[1] <= c["n_max"]), ("c", s[2] >= c["c_min"]),  # noqa: E731
                                                               ("tiles", whole(s)), ("items", items(s) >= CUS))]
    for s in ROWS:  # (the predicate restated with the numbers read is the route)
        for kind in KINDS:
            assert (family(kind, s) == "wino4_pool") == all(takes(s)) == (s in pool), (kind, s)
    assert any(s[1] == c["n_max"] for s in pool), "no wino4_pool row with N = %d low-resolution channels" % c["n_max"]
    assert any(s[1] == c["n_max"] + 1 and all(takes(s, "n")) for s in rest), \
        "no row that only N > %d keeps off wino4_pool" % c["n_max"]
    assert any(s[2] == c["c_min"] for s in pool), "no wino4_pool row with C = %d full-resolution channels" % c["c_min"]
    assert any(s[2] == c["c_min"] - 1 and all(takes(s, "c")) for s in rest), \
        "no row that only C < %d keeps off wino4_pool" % c["c_min"]
    assert any(not whole(s) and all(takes(s, "tiles")) for s in rest), \
        "no row that only a map of no whole %d x %d tiles keeps off wino4_pool" % (c["pxh"], c["pxw"])
    assert any(items(s) == CUS for s in pool), "no wino4_pool row with exactly one work item per CU"
    assert any(items(s) < CUS and all(takes(s, "items")) for s in rest), \
        "no row that only too few work items keep off wino4_pool"
    assert any(s[1] % c["tco"] and s[2] % c["ck"] for s in pool), "no wino4_pool row with ragged channels on both sides"
    # the split of the phase data gradient: every S up to the cap, on both tiles, and N on both sides of the bound
    split = {s: v[3] for s, v in ROWS.items()}
    assert c["split_n"] == c["n_max"] and c["tn"] == 2 * c["split_n"]
    for name, wide in (("wide", True), ("narrow", False)):
        mine = {s: S for s, S in split.items() if (s[4] >= c["wide_w"]) == wide}
        assert all((ROWS[s][1] == "conv_wino_up_dgrad_kernel<1,4>") == wide for s in mine if ROWS[s][2] != "wino4_pool")
        assert 2 in mine.values(), "no row with S = 2 on the %s tile" % name
        assert any(2 < S < c["cap"] for S in mine.values()), "no row with 2 < S < %d on the %s tile" % (c["cap"], name)
        assert c["cap"] in mine.values(), "no row with S = %d, the cap, on the %s tile" % (c["cap"], name)
        assert any(S == 1 and s[1] > c["split_n"] for s, S in mine.items()), \
            "no unsplit row with N > %d on the %s tile" % (c["split_n"], name)
    for s, S in split.items():  # (the predicate restated: few items, at least min_chunks chunks, per_slice chunks a slice)
        B, Cl, Cf, h, w = s
        wide = w >= c["wide_w"]
        n = B * cdiv(h, c["wide_h"] if wide else c["narrow_h"]) * cdiv(w, c["wide_pw"] if wide else c["narrow_pw"]) \
            * cdiv(Cl, c["tn"])
        nch = cdiv(Cf, c["ck"])
        want = 1
        if ROWS[s][2] != "wino4_pool" and Cl > c["split_n"] and not (h * w) & 3 and n <= CUS and nch >= c["min_chunks"]:
            want = max(min(2 * CUS // n, nch // c["per_slice"], c["cap"]), 1)
        assert S == want, s
    # the slices of the weight gradient
    plans = {s: plan_slices(c, s) for s in ROWS}
    assert all(plans[s][2] == (ROWS[s][4] if s in EDGE else 1) for s in ROWS)
    assert any(p[2] > 1 and p[0] % p[1] for p in plans.values()), "no row with a ragged last slice of the weight gradient"
    assert any(p[2] == 2 for p in plans.values()) and any(p[2] > 2 and p[0] % p[1] == 0 for p in plans.values()), \
        "no row with two, or with many whole, slices of the weight gradient"
    assert any(p[0] // c["stages"] == 0 for p in plans.values()), "no row with fewer than %d stages" % c["stages"]
    # (the other bound, cdiv(blocks, tiles), holds from 2^30 products of B h w Cl Cf up: no row is that large, the sweep's
    # largest layers are, and there the restated plan is held to the library's workspace size)
    assert all(p[3] == "stages" for p in plans.values())
    assert plan_slices(c, (16, 512, 512, 128, 128))[3] == "blocks"
    # the tiles of the two phase-form kernels: partial tiles and odd sizes on both
    for name, wide, ph, pw in (("wide", True, c["wide_h"], c["wide_pw"]), ("narrow", False, c["narrow_h"], c["narrow_pw"])):
        mine = [s for s in ROWS if (s[4] >= c["wide_w"]) == wide]
        assert any(s[3] % ph and s[4] % pw for s in mine), "no row of partial %s tiles in both directions" % name
        assert any(s[3] % ph == 0 and s[4] % pw == 0 for s in mine), "no row of whole %s tiles" % name
    assert any(s[3] % 2 for s in ROWS), "no row with an odd low-resolution height"
    up_items = lambda s: s[0] * cdiv(s[3], c["wide_h"]) * cdiv(s[4], c["wide_pw"]) * cdiv(s[2], c["up_tco"])  # noqa: E731
    assert any(s[4] >= c["wide_w"] and up_items(s) > 2 * CUS for s in ROWS), \
        "no row with more work items than the %d resident blocks of conv_wino_up_kernel<1,4>" % (2 * CUS)

