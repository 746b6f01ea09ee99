"""CPU-side checks of the QK-norm family: the configuration, the fixtures and the fp64 restatement the kernel tests compare against
(no kernel is launched)."""
import dataclasses

import numpy as np
import torch

import _qknorm_ref as QR
from conftest import load_golden
from egom2p_amd import synth
from egom2p_amd.config import MODEL_CFGS, ModelCfg

SITES = ([f"encoder.{i}.attn" for i in range(2)] + [f"decoder.{i}.{s}" for i in range(2) for s in ("self_attn", "cross_attn")])
HEAD_NORMS = [f"{s}.{n}_norm.weight" for s in SITES for n in ("q", "k")]


def test_model_cfg_qk_norm_flag():
    d = {f.name: f.default for f in dataclasses.fields(ModelCfg)}
    assert d["qk_norm"] is False
    assert not MODEL_CFGS["egom2p_base_12e_12d_swiglu_nobias"].qk_norm
    c = MODEL_CFGS["ego_384_2e_2d_qknorm"]
    assert c.qk_norm is True and (c.dim, c.num_heads, c.head_dim, c.encoder_depth, c.decoder_depth) == (384, 6, 64, 2, 2)
    g = MODEL_CFGS["ego_gen_384_2e_2d_qknorm"]
    assert g.qk_norm and g.modalities == ("tok_rgb", "tok_depth")
    b = MODEL_CFGS["ego_b_qknorm"]
    assert b.qk_norm and dataclasses.replace(b, name="x", qk_norm=False) == dataclasses.replace(MODEL_CFGS["egom2p_base_12e_12d_swiglu_nobias"], name="x")


def test_synthetic_state_dict_draws_the_head_norm_weights():
    sd = synth.build_state_dict(MODEL_CFGS["ego_384_2e_2d_qknorm"], 43, posemb=False)
    plain = synth.build_state_dict(MODEL_CFGS["ego_384_2e_2d_causal"], 43, posemb=False)
    assert set(sd) - set(plain) == set(HEAD_NORMS) | {k[:-len("weight")] + "bias" for k in HEAD_NORMS}
    for k in HEAD_NORMS:
        w = sd[k]
        assert w.shape == (64,) and abs(w.mean().item() - 1.0) < 0.05 and 0.05 < w.std().item() < 0.2
        assert sd[k[:-len("weight")] + "bias"].shape == (64,) and not bool(sd[k[:-len("weight")] + "bias"].any())
    for k in plain:                                  # every other tensor is what the flag-free configuration draws
        assert torch.equal(sd[k], plain[k]), k


def test_fixtures_load_and_record_nonzero_head_norm_gradients():
    g, meta = load_golden("b2_qknorm")
    assert meta["cfg"] == "ego_384_2e_2d_qknorm" and (meta["batch"], meta["n_enc"], meta["n_dec"]) == (2, 256, 320)
    names = [str(n) for n in g["grad_names"]]
    sq = dict(zip(names, g["grad_sqnorm_all"]))
    assert len(HEAD_NORMS) == 2 * (2 + 2 * 2) == 12
    assert sorted(n for n in names if "q_norm" in n or "k_norm" in n) == sorted(HEAD_NORMS)
    for n in HEAD_NORMS:
        assert sq[n] > 0.0, n
    assert int(g["dec_pad"].sum()) == 97 and np.isfinite(float(g["loss"]))
    gg, gmeta = load_golden("gen_rgb2depth_qknorm")
    assert gmeta["cfg"] == "ego_gen_384_2e_2d_qknorm" and int(gg["n_steps"]) == 3 and gg["final_tokens"].shape == (1, 5120)
    assert float(gg["s0.cfg"][2]) == 2.0


def test_fp64_restatement_agrees_with_torch_layer_norm_autograd_on_a_strided_view():
    gen = torch.Generator().manual_seed(5)
    B, n, H, A = 2, 7, 3, 192
    buf = torch.randn(B * n * 3 * A + 40, generator=gen, dtype=torch.float64)
    w = (1.0 + 0.1 * torch.randn(64, generator=gen, dtype=torch.float64)).requires_grad_(True)
    src = buf.clone().requires_grad_(True)
    xv = QR.head_view(src, 40 + A, n * 3 * A, 3 * A, B, n, H)           # the k slot of a [rows, 3A] buffer that starts 40 elements in
    y = torch.nn.functional.layer_norm(xv, (64,), w, None, 1e-6)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy)
    y2, mean, rstd = QR.headnorm_fwd(xv.detach(), w.detach())
    assert torch.allclose(y2, y.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, xv.detach().mean(-1)) and torch.allclose(rstd, (xv.detach().var(-1, unbiased=False) + 1e-6).rsqrt())
    dx, dw = QR.headnorm_bwd(dy, xv.detach(), w.detach())
    gx = QR.head_view(src.grad, 40 + A, n * 3 * A, 3 * A, B, n, H)
    assert torch.allclose(dx, gx, rtol=1e-10, atol=1e-12) and torch.allclose(dw, w.grad, rtol=1e-10, atol=1e-12)
    mask = torch.ones_like(src.grad, dtype=torch.bool)
    QR.head_view(mask, 40 + A, n * 3 * A, 3 * A, B, n, H).fill_(False)
    assert not bool(src.grad[mask].any())            # nothing outside the addressed slices carries a gradient
