"""CPU side of the step gate: `NativeScalerWithGradNormCount.__call__` keeps the reference's precedence
(egom2p/utils/native_scaler.py:30-40: `if clip_grad is not None ... elif skip_grad is not None`), and the committed fixture of
the reference run is what the GPU tests expect it to be."""
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from egom2p_amd.optim import NativeScalerWithGradNormCount


class _StubOptimizer:
    def __init__(self):
        self.calls = []

    def step(self, **kw):
        self.calls.append(kw)
        return torch.tensor(1.0)


def _loss():
    w = torch.ones(3, requires_grad=True)
    return (w * 2.0).sum(), w


def test_scaler_precedence_is_the_reference_one():
    scaler = NativeScalerWithGradNormCount(enabled=False)
    opt = _StubOptimizer()
    loss, w = _loss()
    norm = scaler(loss, opt, clip_grad=1.0, skip_grad=5.0, parameters=[w], update_grad=True)      # clip set: skip_grad is ignored
    assert norm is not None and w.grad is not None
    assert opt.calls == [{"clip_grad": 1.0}]
    loss, w = _loss()
    scaler(loss, opt, clip_grad=None, skip_grad=5.0, parameters=[w], update_grad=True)           # skip_grad alone: forwarded, unclipped
    assert opt.calls[-1] == {"clip_grad": None, "skip_grad": 5.0}
    loss, w = _loss()
    assert scaler(loss, opt, clip_grad=None, skip_grad=5.0, parameters=[w], update_grad=False) is None
    assert len(opt.calls) == 2 and w.grad is not None                                             # accumulation micro-step: backward only
    loss, w = _loss()
    scaler(loss, opt, parameters=[w])                                                             # neither: the norm-only call of before
    assert opt.calls[-1] == {"clip_grad": 1e30}


def test_scaler_guard_is_a_constructor_option():
    scaler = NativeScalerWithGradNormCount(enabled=False, skip_nonfinite=True)
    opt = _StubOptimizer()
    loss, w = _loss()
    scaler(loss, opt, clip_grad=1.0, skip_grad=5.0, parameters=[w])                               # the production recipe + guard
    assert opt.calls[-1] == {"clip_grad": 1.0, "skip_nonfinite": True}
    loss, w = _loss()
    scaler(loss, opt, skip_grad=5.0, parameters=[w])
    assert opt.calls[-1] == {"clip_grad": None, "skip_grad": 5.0, "skip_nonfinite": True}


def test_skip_grad_fixture_is_the_reference_run():
    f = np.load(os.path.join(GOLDEN_DIR, "skip_grad.npz"), allow_pickle=False)
    assert f["decisions"].tolist() == [0, 0, 1, 0, 1, 0, 0]
    steps = f["steps"]
    assert steps.shape == (7, 4) and steps[-1].tolist() == [5, 5, 5, 5]
    assert steps[:, 0].tolist() == [1, 2, 2, 3, 3, 4, 5]                  # a skipped call does not advance state["step"]
    norms = f["norms"]
    assert np.isinf(norms[4]) and np.isnan(norms[6]) and norms[2] > 200.0 and all(norms[k] < 200.0 for k in (0, 1, 3, 5))
    for n, k in (("decay0", 1027), ("decay1", 64), ("nodecay0", 4099), ("nodecay1", 3)):
        assert f[f"p0.{n}"].shape == (k,) and f[f"g6.{n}"].shape == (k,)
        for call in (2, 4):                                               # skipped: the parameters keep their bits
            assert np.array_equal(f[f"p{call + 1}.{n}"], f[f"p{call}.{n}"])
        assert not np.array_equal(f[f"p1.{n}"], f[f"p0.{n}"])
    assert np.isnan(f["p7.nodecay0"]).sum() == 1 and not np.isnan(f["p6.nodecay0"]).any()
