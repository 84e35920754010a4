"""Reader of tests/golden/style_model.npz (written by tests/golden/make_golden_style_model.py, which documents the entries)."""
import contextlib
import os
import random

import torch

import style_net_fixture as NF

PATH = os.path.join(NF.HERE, "golden", "style_model.npz")
LAST = ("last_rec_loss", "last_real_kl", "last_fake_kl", "last_kl_diff", "last_expelbo_fake", "last_expelbo_rec")
LAST_IN = dict(last_fake_kl=0.75, last_real_kl=0.25)


class Fixture(NF.Fixture):
    def __init__(self, path=PATH):
        super().__init__(path)

    def runs(self, kind):
        return [k[:-len("/meta")] for k in self.files if k.startswith(kind + "/") and k.endswith("/meta")]

    def draws(self, run):
        """the recorded draws of a run in call order, float32"""
        shapes = self.json(run + "/meta")["draw_shapes"]
        return list(self.split(self[run + "/draws"], [[str(i), s] for i, s in enumerate(shapes)]).values())


def import_model():
    """the drop-in model.py, imported as `model` with its directory on the path (it does `from net import *`)"""
    import importlib
    import sys
    sys.path.insert(0, NF.NET_DIR)
    try:
        return importlib.import_module("model")
    finally:
        sys.path.remove(NF.NET_DIR)


@contextlib.contextmanager
def replay(draws, seed, batch):
    """torch.randn / torch.randn_like return the recorded draws in order (on the device asked for) and `random` is seeded as
    the generator seeded it.  Shapes must agree, except that a recorded [1, 1, 4, 4] stands for the [batch, 1, 4, 4] noise
    of the first decoder layer (the drop-in Generator expands its constant to the batch, the reference leaves it at one
    sample: net.py's documented difference).  On exit every draw must have been used."""
    left = list(draws)
    real = (torch.randn, torch.randn_like)

    def take(shape, device):
        assert left, "more draws than the reference made"
        t = left.pop(0)
        shape = tuple(shape)
        if tuple(t.shape) != shape:
            assert tuple(t.shape) == (1, 1, 4, 4) and shape == (batch, 1, 4, 4), (tuple(t.shape), shape)
            t = t.expand(batch, 1, 4, 4).contiguous()
        return t.to(device=device, dtype=torch.float32)

    def randn(*size, device=None, **kw):
        size = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        return take(size, device)

    def randn_like(t, **kw):
        return take(t.shape, t.device)

    random.seed(seed)
    torch.randn, torch.randn_like = randn, randn_like
    try:
        yield left
    finally:
        torch.randn, torch.randn_like = real
    assert not left, "%d recorded draws were not used" % len(left)
