"""bf16-mode autograd blocks (functional16: ResidualBlock in every dispatch branch, stem, predict) against the fp64
"rounded-where-stored" referee of tests/block_checks16.py (pytest -m gpu)."""
import pytest
import torch

import block_checks16 as bc

CHECKS = bc.all_checks()


@pytest.mark.gpu
@pytest.mark.parametrize("label,thunk", CHECKS, ids=[c[0] for c in CHECKS])
def test_block16(label, thunk):
    results = thunk()
    torch.cuda.synchronize()
    bad = [(n, e, t) for (n, e, t) in results if not e <= t]
    assert not bad, "bf16 block referee failures: %s" % bad
