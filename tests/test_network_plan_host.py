"""Host-only checks of sivae_hip.nn.main_plan: the layer groups nn._run_main dispatches, each group's fused neighbour
(`post`), upsample addressing (`x_up`), channels and resolution, asserted as values (no GPU, nothing runs: the networks
are built on the meta device).  tests/test_block_launches_host.py holds the execution of the plan to a recording."""
import contextlib
import gc
import weakref

import pytest
import torch

from sivae_hip import nn as N

CELEB256 = [64, 128, 256, 512, 512, 512]
CIFAR10 = [64, 128, 256]


def _nets(channels, size):
    with torch.device("meta"), contextlib.redirect_stdout(None):  # (the constructors print their shapes)
        enc = N.Encoder(3, 8, channels, size)
        dec = N.Decoder(3, 8, channels, size, conv_input_size=enc.conv_output_size)
    return enc, dec


def _rows(plan):
    return [(s.kind, s.post, s.x_up, s.Ci, s.Cm, s.Co, (s.H, s.W), (s.Ho, s.Wo)) for s in plan]


def _check_indices(main, plan):
    """every step starts at its `index` in `main` with the modules it names, and the steps tile the Sequential"""
    mods = list(main.children())
    at = 0
    for s in plan:
        assert s.index == at, (s.index, at)
        if s.kind == "block":
            assert mods[at] is s.block and s.conv is None and s.bn is None
            at += 1 if s.post is None else 2
        elif s.kind == "stem":
            assert mods[at] is s.conv and mods[at + 1] is s.bn and s.block is None
            at += 4
        else:
            assert s.kind == "predict" and mods[at] is s.conv and s.block is None and s.bn is None
            at += 1
    assert at == len(mods)


def test_celeb256_decoder_defers_every_upsample(monkeypatch):
    monkeypatch.setattr(N, "DEFER_UPSAMPLE", True)
    dec = _nets(CELEB256, 256)[1]
    plan = N.main_plan(dec.main, (4, 4))
    chans = [(512, 512), (512, 512), (512, 512), (512, 256), (256, 128), (128, 64)]
    want = [("block", "up_deferred", i > 0, ci, co, co, (4 << i, 4 << i), (4 << i, 4 << i))
            for i, (ci, co) in enumerate(chans)]
    want.append(("block", None, True, 64, 64, 64, (256, 256), (256, 256)))
    want.append(("predict", None, False, 64, None, 3, (256, 256), (256, 256)))
    assert _rows(plan) == want
    assert [s.index for s in plan] == [0, 2, 4, 6, 8, 10, 12, 13]
    _check_indices(dec.main, plan)
    assert N.main_plan(dec.main, (4, 4)) is plan  # (memoised: a forward pass parses nothing)


def test_defer_upsample_switch_takes_effect_on_a_planned_decoder(monkeypatch):
    monkeypatch.setattr(N, "DEFER_UPSAMPLE", True)
    dec = _nets(CELEB256, 256)[1]
    before = N.main_plan(dec.main, (4, 4))
    assert [s.post for s in before].count("up_deferred") == 6
    monkeypatch.setattr(N, "DEFER_UPSAMPLE", False)
    plan = N.main_plan(dec.main, (4, 4))
    assert [s.post for s in plan] == ["up"] * 6 + [None, None]
    assert not any(s.x_up for s in plan)
    assert [(s.H, s.W) for s in plan] == [(4 << i, 4 << i) for i in range(7)] + [(256, 256)]
    assert [(s.Ho, s.Wo) for s in plan] == [(8 << i, 8 << i) for i in range(6)] + [(256, 256)] * 2
    _check_indices(dec.main, plan)
    N.DEFER_UPSAMPLE = True  # (plain assignment; monkeypatch puts the session's own value back at the end)
    assert N.main_plan(dec.main, (4, 4)) is before
    N.DEFER_UPSAMPLE = False
    assert N.main_plan(dec.main, (4, 4)) is plan


@pytest.mark.parametrize("channels,size", [(CELEB256, 256), (CIFAR10, 32)], ids=["celeb256", "cifar10"])
def test_encoder_is_a_stem_then_pooled_blocks(channels, size):
    enc = _nets(channels, size)[0]
    plan = N.main_plan(enc.main, (size, size))
    want = [("stem", "pool", False, 3, None, channels[0], (size, size), (size // 2, size // 2))]
    s = size // 2
    for ci, co in zip(channels, channels[1:]):
        want.append(("block", "pool", False, ci, co, co, (s, s), (s // 2, s // 2)))
        s //= 2
    want.append(("block", None, False, channels[-1], channels[-1], channels[-1], (s, s), (s, s)))
    assert _rows(plan) == want
    assert (plan[-1].Co, plan[-1].Ho, plan[-1].Wo) == tuple(enc.conv_output_size)
    assert [st.index for st in plan] == [0] + [4 + 2 * i for i in range(len(channels))]
    _check_indices(enc.main, plan)


def test_an_odd_width_does_not_defer(monkeypatch):
    monkeypatch.setattr(N, "DEFER_UPSAMPLE", True)
    with torch.device("meta"):
        main = torch.nn.Sequential(N.ResidualBlock(8, 8), torch.nn.Upsample(scale_factor=2, mode="nearest"),
                                   N.ResidualBlock(8, 8))
    even, odd = N.main_plan(main, (6, 6)), N.main_plan(main, (7, 7))
    assert _rows(even) == [("block", "up_deferred", False, 8, 8, 8, (6, 6), (6, 6)),
                           ("block", None, True, 8, 8, 8, (12, 12), (12, 12))]
    assert _rows(odd) == [("block", "up", False, 8, 8, 8, (7, 7), (14, 14)),
                          ("block", None, False, 8, 8, 8, (14, 14), (14, 14))]
    for plan in (even, odd):
        assert [s.index for s in plan] == [0, 2]
        _check_indices(main, plan)


def test_an_edited_sequential_is_planned_anew():
    with torch.device("meta"):
        main = torch.nn.Sequential(N.ResidualBlock(8, 8), torch.nn.AvgPool2d(2), N.ResidualBlock(8, 8))
        first = N.main_plan(main, (8, 8))
        main[2] = N.ResidualBlock(8, 16)
        main.append(torch.nn.Conv2d(16, 3, 5, 1, 2))
    plan = N.main_plan(main, (8, 8))
    assert [s.kind for s in first] == ["block", "block"] and first[1].Co == 8
    assert [(s.kind, s.Co, s.index) for s in plan] == [("block", 8, 0), ("block", 16, 2), ("predict", 3, 3)]
    _check_indices(main, plan)
    main[1] = torch.nn.ReLU()
    with pytest.raises(RuntimeError):
        N.main_plan(main, (8, 8))


def test_an_unexpected_layer_is_refused():
    with torch.device("meta"):
        main = torch.nn.Sequential(N.ResidualBlock(8, 8), torch.nn.ReLU(), N.ResidualBlock(8, 8))
    with pytest.raises(RuntimeError) as e:
        N.main_plan(main, (8, 8))
    assert str(e.value) == "sivae_hip: unexpected layer ReLU in network"
    with pytest.raises(RuntimeError) as e:
        N._run_main(main, torch.empty(2, 8, 8, 8, device="meta"))
    assert str(e.value) == "sivae_hip: unexpected layer ReLU in network"


def test_a_stem_without_its_pool_is_refused():
    with torch.device("meta"):
        main = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 5, 1, 2, bias=False), torch.nn.BatchNorm2d(8),
                                   torch.nn.LeakyReLU(0.2), N.ResidualBlock(8, 8))
    with pytest.raises(AssertionError):
        N.main_plan(main, (8, 8))


def test_the_plan_does_not_keep_the_model_alive():
    enc, dec = _nets(CIFAR10, 32)
    N.main_plan(enc.main, (32, 32))
    N.main_plan(dec.main, tuple(enc.conv_output_size[1:]))
    refs = [weakref.ref(enc.main), weakref.ref(dec.main)]
    del enc, dec
    gc.collect()
    assert [r() for r in refs] == [None, None]
