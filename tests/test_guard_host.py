"""tests/support/guard.py against a toy module on CPU tensors: what the guard must see (a byte next to the tensor on either
side, a byte at the far edge of either guard, an element nobody wrote, a workspace one byte too small) and what it must
put back.  No GPU."""
import types

import pytest
import torch

from support import guard as G

TOY_SOURCE = '''
import torch

_workspaces = {}
_counters = {"stale": 1}
_bn_states = {"stale": 2}


def workspace(nbytes, device):
    buf = _workspaces.get("k")
    if buf is None or buf.numel() < nbytes:
        buf = _workspaces["k"] = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
    return buf


def counters(device):
    buf = _counters.get("k")
    if buf is None:
        buf = _counters["k"] = torch.zeros(64, dtype=torch.int32, device=device)
    return buf


def make(shape, dtype):
    return torch.empty(shape, dtype=dtype, device="cpu")


def make_like(t, zero=False):
    return torch.zeros_like(t) if zero else torch.empty_like(t)


def make_flat(n):
    return torch.empty(n, dtype=torch.float32, device=torch.device("cpu"))


def scratch(nbytes):
    return workspace(nbytes, torch.device("cpu"))


def make_pinned(n):
    return torch.empty(n, dtype=torch.float32, device="cpu", pin_memory=False)
'''
USER_SOURCE = '''
import torch
from toy_ops import workspace


def scratch(nbytes):
    return workspace(nbytes, torch.device("cpu"))
'''


@pytest.fixture
def toy(monkeypatch):
    import sys
    m = types.ModuleType("toy_ops")
    exec(compile(TOY_SOURCE, "toy_ops.py", "exec"), m.__dict__)
    monkeypatch.setitem(sys.modules, "toy_ops", m)
    u = types.ModuleType("toy_user")  # (a module that imported workspace by name, as pointcloud does)
    exec(compile(USER_SOURCE, "toy_user.py", "exec"), u.__dict__)
    return m, u


def _raw(g, t):
    """the whole guard | body | guard buffer of the allocation that returned t"""
    r = [r for r in g.records if r.raw.data_ptr() + r.front == t.data_ptr()][-1]
    return r.raw, r.front, r.nbytes


def test_intact_allocations_verify_empty(toy):
    m, _ = toy
    with G.guarded(m) as g:
        a = m.make((3, 5), torch.float32)
        a.fill_(1.0)
        m.make_flat(7).zero_()
        m.scratch(100).zero_()
        assert g.verify() == []
        assert g.verify() == []  # (released: nothing left to look at)


@pytest.mark.parametrize("where", ["just_past", "just_before", "far_edge_back", "far_edge_front"])
def test_one_damaged_byte_is_reported(toy, where):
    m, _ = toy
    with G.guarded(m, guard_bytes=1024) as g:
        t = m.make((3, 5), torch.float32)
        t.zero_()
        raw, front, nbytes = _raw(g, t)
        at = {"just_past": front + nbytes, "just_before": front - 1, "far_edge_back": raw.numel() - 1,
              "far_edge_front": 0}[where]
        raw[at] = 0
        other = m.make((2,), torch.int32)  # (an intact neighbour is not reported)
        other.zero_()
        damage = g.verify()
    assert len(damage) == 1, damage
    d = damage[0]
    assert d["site"] == "toy_ops:make:%d" % (TOY_SOURCE.split("\n").index('    return torch.empty(shape, dtype=dtype, device="cpu")') + 1)
    assert d["shape"] == (3, 5) and d["dtype"] == "float32" and d["damaged_bytes"] == 1
    assert d["first_byte"] == d["last_byte"] == at - front  # (relative to the tensor: negative in front of it)
    assert (d["first_byte"] < 0) == (where in ("just_before", "far_edge_front"))
    assert "toy_ops:make" in G.describe(damage)


def test_damage_on_both_sides_is_one_record_with_the_range(toy):
    m, _ = toy
    with G.guarded(m, guard_bytes=512) as g:
        t = m.make_flat(4)
        raw, front, nbytes = _raw(g, t)
        raw[front - 3:front] = 7
        raw[front + nbytes:front + nbytes + 2] = 7
        (d,) = g.verify()
    assert (d["first_byte"], d["last_byte"], d["damaged_bytes"]) == (-3, nbytes + 1, 5)


def test_unwritten_elements_read_back_as_poison_and_zeros_are_zero(toy):
    m, _ = toy
    with G.guarded(m) as g:
        assert torch.isnan(m.make((4, 3), torch.float32)).all()
        assert torch.isnan(m.make((4, 3), torch.float64)).all()
        assert torch.isnan(m.make((4, 8), torch.bfloat16).float()).all()
        assert (m.make((5,), torch.int32) == -1).all()
        assert (m.make((5,), torch.uint8) == 255).all()
        assert torch.isnan(m.make((), torch.float32))  # (0-dim: one element)
        like = m.make_like(torch.ones(2, 3, dtype=torch.float64))
        assert like.shape == (2, 3) and like.dtype == torch.float64 and torch.isnan(like).all()
        z = m.make_like(torch.ones(6, dtype=torch.float32), zero=True)
        assert (z == 0).all()
        c = m.counters(torch.device("cpu"))
        assert c.dtype == torch.int32 and c.shape == (64,) and (c == 0).all()
        for t in (like, z, c, m.make((7, 3), torch.float32)):
            assert t.is_contiguous()
        assert g.verify() == []


def test_a_keyword_the_proxy_does_not_model_is_an_error(toy):
    """pin_memory / memory_format / requires_grad would be dropped silently: the guarded run would differ from production"""
    m, _ = toy
    assert m.make_pinned(3).shape == (3,)
    with G.guarded(m):
        with pytest.raises(TypeError, match="pin_memory"):
            m.make_pinned(3)


def test_body_keeps_the_512_byte_alignment(toy):
    m, _ = toy
    with pytest.raises(ValueError):
        G.Guard(guard_bytes=1000)
    with G.guarded(m) as g:
        for shape, dtype in (((3,), torch.float32), ((5, 7), torch.bfloat16), ((1,), torch.uint8)):
            t = m.make(shape, dtype)
            raw, front, _ = _raw(g, t)
            assert front == G.GUARD_BYTES and front % 512 == 0 and t.data_ptr() - raw.data_ptr() == front
        # a placed destination starts offset_elems ELEMENTS behind the aligned start
        for k in range(4):
            src = torch.arange(6, dtype=torch.float32).view(2, 3)
            v = g.place(src, offset_elems=k)
            raw, front, _ = _raw(g, v)
            assert front == G.GUARD_BYTES + 4 * k and torch.equal(v, src) and v.is_contiguous()
            assert (raw[G.GUARD_BYTES:front] == 0xFF).all()
        assert g.verify() == []


def test_the_elements_in_front_of_a_placed_tensor_are_verified(toy):
    m, _ = toy
    with G.guarded(m, guard_bytes=512) as g:
        v = g.place(torch.zeros(5), offset_elems=3)
        raw, front, _ = _raw(g, v)
        raw[front - 12] = 0  # (the first byte of the three unused elements)
        (d,) = g.verify()
    assert d["kind"] == "placed" and (d["first_byte"], d["last_byte"]) == (-12, -12)


def test_workspace_is_fresh_exact_and_never_null(toy):
    m, u = toy
    with G.guarded(m, u) as g:
        a, b = m.scratch(1000), m.scratch(1000)
        assert a.numel() == b.numel() == 1000 and a.dtype == torch.uint8 and a.data_ptr() != b.data_ptr()
        assert (a == 255).all()
        assert u.scratch(77).numel() == 77  # (the copy another module imported by name)
        assert m._workspaces == {}          # (the module's cache of unguarded buffers is not used)
        raw, front, nbytes = _raw(g, a)
        raw[front + 1000] = 1               # byte 1000 of a 1000-byte workspace
        z = m.scratch(0)
        assert z.data_ptr() != 0 and z.numel() <= 1
        damage = g.verify()
        assert [(d["kind"], d["first_byte"]) for d in damage] == [("workspace", 1000)]
        z = m.scratch(0)
        z.zero_()                           # whatever a 0-byte workspace is given, writing it is damage
        assert [(d["kind"], d["first_byte"], d["damaged_bytes"]) for d in g.verify()] == [("workspace", 0, 1)]


def test_everything_is_restored_after_an_exception(toy):
    m, u = toy
    before = {k: m.__dict__[k] for k in ("torch", "workspace", "_workspaces", "_counters", "_bn_states")}
    user_ws = u.workspace
    with pytest.raises(RuntimeError, match="boom"):
        with G.guarded(m, u):
            assert m.torch is not torch and u.torch is not torch and m._counters == {} and m._bn_states == {}
            assert u.workspace is not user_ws and m.workspace is not before["workspace"]
            m.make((2,), torch.float32)
            raise RuntimeError("boom")
    for k, v in before.items():
        assert m.__dict__[k] is v, k
    assert m.torch is torch and u.torch is torch and u.workspace is user_ws
    assert m._counters == {"stale": 1} and m._bn_states == {"stale": 2}
    assert not torch.isnan(m.make((2,), torch.float32).fill_(0)).any() and m.scratch(8).numel() == 1 << 20


def test_the_real_modules_use_only_the_four_idioms_the_proxy_replaces():
    """a new allocation idiom in the ops layer (torch.full, new_empty, ...) would escape the guard: extend the proxy"""
    import os
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "soft-intro-vae-pytorch_amd", "sivae_hip")
    makers = re.compile(r"torch\.(full|ones|full_like|ones_like|rand\w*|tensor|arange|empty_strided)\(|\.new_(empty|zeros|full|ones|tensor)\(")
    for name in ("ops.py", "ops16.py", "pointcloud.py"):
        with open(os.path.join(pkg, name)) as f:
            hits = [line.strip() for line in f if makers.search(line)]
        assert not hits, (name, hits)
