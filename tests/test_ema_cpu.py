"""Host side of the model EMA (egom2p_amd/ema.py; ModelEmaV2, egom2p/utils/timm/model_ema.py:84-149): the decay rule, the
constructor's refusals and the command-line surface.  Nothing here launches a kernel."""
import importlib.util
import os
import types

import pytest
import torch

from egom2p_amd.ema import ModelEma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_engine(n=8):
    return types.SimpleNamespace(P=torch.arange(n, dtype=torch.float32), weights_dirty=False, params_swapped=False)


def test_decay_at_with_and_without_warmup():
    d = 0.9999
    e = ModelEma(_fake_engine(), decay=d, warmup=True)
    assert [e.decay_at(k) for k in range(3)] == [0.1, 2.0 / 11.0, 3.0 / 12.0]
    # (1 + k) / (10 + k) >= d  <=>  k >= (10 d - 1) / (1 - d): the first such k takes the configured decay, the one before does not
    cross = next(k for k in range(200_000) if (1.0 + k) / (10.0 + k) >= d)
    assert cross == 89_990
    assert e.decay_at(cross) == d and e.decay_at(cross + 1) == d and e.decay_at(10 ** 9) == d
    assert e.decay_at(cross - 1) == (1.0 + cross - 1) / (10.0 + cross - 1) < d
    vals = [e.decay_at(k) for k in range(0, cross + 10, 997)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))                       # never decreases
    small = ModelEma(_fake_engine(), decay=0.5, warmup=True)                 # cross-over at k = 8: 9 / 18
    assert [small.decay_at(k) for k in (7, 8, 9)] == [8.0 / 17.0, 0.5, 0.5]
    flat = ModelEma(_fake_engine(), decay=d, warmup=False)
    assert {flat.decay_at(k) for k in (0, 1, 2, 10, 89_989, 10 ** 9)} == {d}
    assert isinstance(e.decay_at(5), float)


def test_constructor_copies_the_flat_buffer_and_refuses_bad_decays():
    eng = _fake_engine()
    e = ModelEma(eng)
    assert e.decay == 0.9999 and e.warmup is False and e.num_updates == 0
    assert torch.equal(e.ema, eng.P) and e.ema.data_ptr() != eng.P.data_ptr() and e.ema.dtype == torch.float32
    assert ModelEma(_fake_engine(), decay=0.0).decay == 0.0 and ModelEma(_fake_engine(), decay=1.0).decay == 1.0
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ModelEma(_fake_engine(), decay=bad)
    holder = types.SimpleNamespace(engine=eng)                               # a model: the engine is taken from it
    assert ModelEma(holder).engine is eng


def _script():
    spec = importlib.util.spec_from_file_location("run_training_egom2p_ema_cpu", os.path.join(ROOT, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    return R


def test_training_script_flags():
    R = _script()
    a = R.get_args([])
    assert a.model_ema is False and a.model_ema_decay == 0.9999 and a.model_ema_warmup is False
    a = R.get_args(["--model_ema", "--model_ema_decay", "0.99", "--model_ema_warmup"])
    assert a.model_ema is True and a.model_ema_decay == 0.99 and a.model_ema_warmup is True


def test_generation_parser_knows_use_ema():
    from egom2p_amd import eval_generation as E
    for task in E.TASKS:
        ap = E.get_parser(task)
        assert ap.parse_args([]).use_ema is False
        assert ap.parse_args(["--use-ema", "--ckpt", "x.pth"]).use_ema is True


def test_generation_refuses_a_checkpoint_without_the_average(tmp_path):
    from egom2p_amd import eval_generation as E
    path = str(tmp_path / "plain.pth")
    torch.save({"model": {}}, path)
    with pytest.raises(SystemExit) as ei:
        E.load_weights(None, path, use_ema=True)
    assert "state_dict_ema" in str(ei.value)
    with pytest.raises(SystemExit):
        E.main("rgb2cam", ["--use-ema"])                                      # no checkpoint at all: refused before a model is built
