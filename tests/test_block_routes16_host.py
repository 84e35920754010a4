"""Host-only checks that tie the bf16 mode's dispatch to its tests (library predicates only: no GPU needed).  The route
classes come from the route functions of sivae_hip.ops16 (conv2d_route, bn_bwd_route, the block plan's pooled data
gradient) — the code that launches —, which tests/test_conv_routes_host.py holds to a recording of the dispatch.

* every route class a block / stem / predict call of the benchmarked bf16 iterations takes (pixel tile or split-K plan
  of both 3x3 convs, pooled data gradient, one-launch BatchNorm backward, expansion conv, upsampled input, fused
  neighbour, segmented batch) is covered by a case of tests/block_checks16.py;
* nn.segments_supported(..., "bf16") never admits a segmented batch whose conv-epilogue statistics rows would mix two
  passes.
"""
import pytest

import block_checks16 as bc


def test_every_benchmarked_bf16_route_has_a_block_referee():
    """reads nn.main_plan of the Encoder / Decoder of config 3 (128x128, batch 128), celeb256_bf16_bs128 and the
    16-image 256x256 shard, unpaired and as segmented pairs, and requires each route class to be the class of a
    block_checks16 case at that case's own (smaller) batch — the classes are asked of ops16's route functions in both
    places, so a dispatch change that opens a new route fails here until a case covers it"""
    prod = bc.production_routes()
    assert len(prod) >= 20, len(prod)  # (sanity: the walk saw the networks)
    cov = bc.covered_routes()
    missing = {r: where[:3] for r, where in prod.items() if r not in cov}
    assert not missing, "bf16 routes without a block referee case: %s" % missing


def test_block_cases_take_the_routes_they_are_named_for():
    """the case names promise routes (split-K, big pixel tiles, no pooled data gradient, three-launch BatchNorm):
    hold them to it at their own batch"""
    for cs in bc.BLOCK_CASES:
        r = bc.case_route(cs)
        name = cs["name"]
        if name.startswith("splitk"):
            assert r[4] == r[5] == "splitk", (name, r)
        if name.startswith("big"):
            assert r[4] == r[5] == "big", (name, r)
        if name.startswith("small"):
            assert r[4] == r[5] == "small", (name, r)
        if "no pooled dgrad" in name or "pooled dgrad off" in name:
            assert r[6] is False, (name, r)
        if "(pooled dgrad)" in name:
            assert r[6] is True, (name, r)
        if "3-launch BN" in name:
            assert r[7] is False and r[8] is False, (name, r)


def _nets():
    """BASELINE's networks (image_size = 4 * 2^levels) and narrow-channel nets of the same depths, down to 8 channels"""
    base = [64, 128, 256, 512, 512, 512]
    out = []
    for size in (32, 64, 128, 256):
        n = {32: 3, 64: 4, 128: 5, 256: 6}[size]
        for ch in (base[:n], [8 * 2 ** i for i in range(n)], [8] * n, [16] * n, [24, 40, 72, 136, 264, 520][:n],
                   [64] * n, [512] * n):
            out.append((size, list(ch)))
    return out


@pytest.mark.parametrize("size,channels", _nets(), ids=lambda v: str(v))
def test_bf16_segments_supported_never_mixes_two_passes(size, channels):
    """Wherever nn.segments_supported(size, seg_images, "bf16") admits a pair (nseg = 2), every conv whose epilogue
    writes BatchNorm statistics — at 2 * seg_images images, the statistics rows of its route (ops16.conv2d_route: one
    row per image for a split-K plan, else one per pixel tile) — must be cut into the two passes without a row holding images of both (the rule ops.bn_stats_from_conv enforces,
    ops.stats_rows_fit_segments).

    The predicate's hard-coded `seg_images % 16 == 0` holds because of a bound in bf16_conv.hip px_tile_3x3: a tile
    holds several images only on maps smaller than it, and the big tile is refused when `2 * plane > 5 * 256` (plane =
    images x (TH + 2) x (TW + 2)) — which keeps every tile of the 4 x 4 maps (the smallest map of these nets) at <= 16
    images (the 64-channel big tile there would hold 32 images with a 1152-element plane).  Tiles of the 8 x 8 / 16 x 16
    maps hold fewer; the stem's 5x5 tiles stay inside one image.  A tile change that breaks that bound fails here."""
    from sivae_hip import ops, ops16
    from sivae_hip import nn as N
    convs = []
    bc.walk_routes(channels, size, 2, nseg=1, convs=convs)
    shapes = sorted(set(convs))
    admitted = 0
    for seg in range(1, 513):
        if not N.segments_supported(size, seg, "bf16"):
            continue
        admitted += 1
        B = 2 * seg
        for Ci, Co, H, W, ks in shapes:
            rows = ops16.conv2d_route(B, Ci, Co, H, W, ks, want_stats=True).stats_rows
            assert rows > 0, (Ci, Co, H, W, ks, rows)
            assert ops.stats_rows_fit_segments(rows, B, 2), \
                "segments_supported(%d, %d, 'bf16') but conv %s has %d statistics rows at %d images" % (
                    size, seg, (Ci, Co, H, W, ks), rows, B)
    assert admitted == 32, admitted  # (seg_images 16, 32, ..., 512)
