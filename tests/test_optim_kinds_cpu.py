"""Host side of the optimisers other than AdamW (Adam, SGD with momentum, Nesterov): the fp64 restatement of their update rules
(tests/_optim_ref.py, which the GPU tests compare the kernel against) held to torch.optim.SGD / Adam in float64, the dispatch of
`create_optimizer` on `args.opt` as the reference has it (optim_factory.py:214-229), and the entry lists of the new header."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import _optim_ref as R
from egom2p_amd import _lib as L
from egom2p_amd import ops
from egom2p_amd import optim as O
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = ("tok_cam", "tok_gaze")


def tiny_model(device="cpu"):
    """dim 128, 2 + 2 layers, 2 heads, tok_cam + tok_gaze (parameters only: no kernel runs on the CPU)."""
    from functools import partial
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}
    return EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in MODS}, dim=128, encoder_depth=2, decoder_depth=2, num_heads=2,
                  qkv_bias=False, proj_bias=False, mlp_bias=False, norm_layer=partial(LayerNorm, eps=1e-6, bias=False),
                  act_layer=torch.nn.SiLU, gated_mlp=True, device=device)


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("kind,momentum", [("momentum", 0.0), ("momentum", 0.9), ("nesterov", 0.9), ("adam", 0.0), ("adam", 0.9)])
def test_restatement_equals_torch_in_float64(kind, momentum, wd):
    """5 steps on random tensors, to 1e-12 relative (both sides are float64: the orders of operations differ by roundings of
    2^-53 per term).  Adam takes no momentum: its two cases are two draws of the data."""
    gen = torch.Generator().manual_seed(7 + int(momentum * 10))
    lr, b1, b2, eps = 1e-2, 0.9, 0.95, 1e-8
    q = torch.randn(3, 257, dtype=torch.float64, generator=gen).requires_grad_(True)
    if kind == "adam":
        topt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    else:
        topt = torch.optim.SGD([q], lr=lr, momentum=momentum, nesterov=kind == "nesterov", weight_decay=wd)
    p = q.detach().numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 6):
        g = torch.randn(3, 257, dtype=torch.float64, generator=gen)
        q.grad = g.clone()
        topt.step()
        p, m, v = R.step(kind, p, g.numpy(), m, v, lr, wd, t=t, momentum=momentum, b1=b1, b2=b2, eps=eps)
        want = q.detach().numpy()
        assert np.abs(p - want).max() <= 1e-12 * np.abs(want).max(), (kind, t)
        st = topt.state[q]
        if kind == "adam":
            assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 * np.abs(m).max()
            assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(v).max()
        elif momentum:
            assert np.abs(m - st["momentum_buffer"].numpy()).max() <= 1e-12 * np.abs(m).max()


@pytest.mark.parametrize("kind", ["momentum", "nesterov"])
def test_exact_case_stays_in_float32(kind):
    """The inputs of the GPU exact case: three steps in float64 during which nothing the kernel rounds leaves float32."""
    p, gs, buf = R.exact_inputs()
    assert R.fits_fp32(p, buf, *gs)
    states, exact = R.exact_run(kind, p, gs, buf)
    assert exact and len(states) == 3
    lo, hi = R.EXACT_ROWS[3][:2]
    assert np.array_equal(states[-1][0][lo:], p[lo:]) and np.array_equal(states[-1][1][lo:], buf[lo:])     # frozen and stray: untouched
    assert not np.array_equal(states[-1][0][:lo], p[:lo])
    assert sum(hi - lo for lo, hi, *_ in R.EXACT_ROWS) + 4 == R.EXACT_N
    # the two SGD kinds differ on these inputs
    other, _ = R.exact_run("nesterov" if kind == "momentum" else "momentum", p, gs, buf)
    assert not np.array_equal(other[-1][0], states[-1][0])


def _args(opt, **kw):
    return types.SimpleNamespace(opt=opt, lr=1e-3, weight_decay=0.05, opt_betas=(0.9, 0.95), opt_eps=1e-8, momentum=0.9, **kw)


@pytest.mark.parametrize("opt,kind", [("sgd", "nesterov"), ("nesterov", "nesterov"), ("momentum", "momentum"), ("adam", "adam"),
                                      ("fused_adam", "adam"), ("adamw", "adamw"), ("SGD", "nesterov")])
def test_create_optimizer_dispatch(opt, kind):
    model = tiny_model()
    o = O.create_optimizer(_args(opt), model)
    assert o.kind == kind
    if kind == "adamw":
        assert type(o) is O.FusedAdamW and not o.segmented and o.v is not None
        return
    assert isinstance(o, O.FusedOptimizer) and o.segmented                       # the new kinds always step on the segmented launch
    assert [g["name"] for g in o.param_groups] == ["decay", "no_decay"] and [g["weight_decay"] for g in o.param_groups] == [0.05, 0.0]
    assert sum(len(g["params"]) for g in o.param_groups) == len(list(model.named_parameters()))
    sd = o.state_dict()
    assert sd["kind"] == kind
    if kind == "adam":
        assert o.v is not None and "v" in sd and "momentum" not in sd
    else:
        assert o.v is None and "v" not in sd and sd["momentum"] == 0.9 and o.momentum == 0.9      # one state buffer
    assert o.m.shape == model.engine.P.shape


def test_create_optimizer_refusals_and_groups():
    model = tiny_model()
    with pytest.raises(ValueError):
        O.create_optimizer(_args("lamb"), model)
    a = _args("nesterov")
    a.momentum = 0.0
    with pytest.raises(ValueError, match="[Nn]esterov"):
        O.create_optimizer(a, model)
    with pytest.raises(ValueError, match="[Nn]esterov"):
        O.create_optimizer(types.SimpleNamespace(**dict(vars(a), opt="sgd")), model)
    a.opt = "momentum"                                                          # momentum 0 with --opt momentum: plain SGD
    assert O.create_optimizer(a, model).momentum == 0.0
    # the group logic is AdamW's: layer functions, decoder_decay and no_lr_scale_list for every kind
    from functools import partial
    layer_fn = partial(O.get_num_layer_for_fm, num_enc_layers=2, num_dec_layers=2)
    scale_fn = O.LayerDecayValueAssigner(O.layer_decay_values(0.75, 4)).get_scale
    extra = dict(decoder_decay=0.01, no_lr_scale_list="encoder.0.attn.qkv.weight-decoder_norm.weight")
    ref = O.create_optimizer(_args("adamw", **extra), model, get_num_layer=layer_fn, get_layer_scale=scale_fn)
    strip = lambda o: [{k: v for k, v in g.items() if k != "params"} for g in o.param_groups]
    for opt in ("sgd", "momentum", "adam"):
        o = O.create_optimizer(_args(opt, **extra), model, get_num_layer=layer_fn, get_layer_scale=scale_fn)
        assert strip(o) == strip(ref) and o.segments() == ref.segments()
    # without filter_bias_and_bn: one group, the decay on every tensor (optim_factory.py:184-186)
    o = O.create_optimizer(_args("sgd"), model, filter_bias_and_bn=False)
    assert [g["name"] for g in o.param_groups] == ["all"] and o.param_groups[0]["weight_decay"] == 0.05
    # a state of another kind does not load, and the message names both
    sgd, adam, adamw = (O.create_optimizer(_args(k), model) for k in ("sgd", "adam", "adamw"))
    for dst, src in ((adam, sgd), (sgd, adam), (adamw, sgd), (sgd, adamw), (adam, adamw)):
        with pytest.raises(RuntimeError, match=f"'{src.kind}'.*'{dst.kind}'"):
            dst.load_state_dict(src.state_dict())
    with pytest.raises(ValueError):
        O.FusedOptimizer(model.engine, "adamw", named_parameters=model.named_parameters())


def test_sgd_segments_ignore_step_offsets():
    """A tensor that sat steps out splits a segment only where a bias correction depends on the step count."""
    model = tiny_model()
    sgd, adam = (O.create_optimizer(_args(k), model) for k in ("momentum", "adam"))
    key = model.engine._canon_key("encoder.0.attn.qkv.weight")
    base = len(sgd.segments())
    sgd.skipped[key] = adam.skipped[key] = 2
    assert len(sgd.segments()) == base and all(sk == 0 for _, _, _, sk, _ in sgd.segments())
    assert len(adam.segments()) > base and any(sk == 2 for _, _, _, sk, _ in adam.segments())


def test_new_symbol_is_declared_bound_and_exported():
    """include/egom2p_hip_optim_kinds.h, its binding table (_lib.EXPORTS_OPTIM_KINDS) and the library's dynamic symbols agree; the
    entry is in neither of the two pinned lists, the core header includes the new one, and the ABI version stands."""
    core = open(os.path.join(ROOT, "include", "egom2p_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "egom2p_hip_optim_kinds.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s+(ego_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(L.EXPORTS_OPTIM_KINDS) == {"ego_optim_step_seg"}
    assert not declared & set(L.EXPORTS) and not declared & set(L.EXPORTS_OPTIM)
    assert '#include "egom2p_hip_optim_kinds.h"' in core and L.ABI_VERSION == 12
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert declared <= set(re.findall(r" T (ego_\w+)", out))
    assert "optim_factory.py:217-224" in hdr
    for name, val in (("EGO_OPT_ADAM", L.OPT_ADAM), ("EGO_OPT_SGD", L.OPT_SGD), ("EGO_OPT_NESTEROV", L.OPT_NESTEROV)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
    assert ops.OPT_KINDS == {"adam": L.OPT_ADAM, "momentum": L.OPT_SGD, "nesterov": L.OPT_NESTEROV}
    assert hasattr(L.load(), "ego_optim_step_seg") and callable(ops.optim_step_seg)
    # the new entry takes ego_adamw_step_seg's arguments, then the kind and the momentum in front of the stream
    assert L._SIGS_OPTIM_KINDS["ego_optim_step_seg"] == L._SIGS_OPTIM["ego_adamw_step_seg"][:-1] + [L.i32, L.f32, L.vp]


def test_entry_script_switches_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_training_optim_kinds", os.path.join(ROOT, "run_training_egom2p.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    a = rt.get_args([])
    assert a.opt == "adamw" and a.momentum == 0.9
    a = rt.get_args(["--opt", "sgd", "--momentum", "0.8"])
    assert a.opt == "sgd" and a.momentum == 0.8
