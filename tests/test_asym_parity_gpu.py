"""Parity of the asymmetric (b2_asym), no-separation (b2_nosep, three decoder modalities: the staircase is real) and unshared
(b2_unshared) variants against outputs of the REAL reference model (tests/golden/b2_*.npz, made by tools/make_goldens_asym.py):
integer outputs and the decoder mask bit-exact, taps and gradients at the bars of tests/test_engine_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _asym_bars import held  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL, ACT_TOL, GRAD_TOL = 1e-3, 2e-2, 4e-2          # tests/test_engine_gpu.py:20-22

_spec = importlib.util.spec_from_file_location("make_goldens_asym_parity", os.path.join(ROOT, "tools", "make_goldens_asym.py"))
TOOL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(TOOL)                            # the cases' configurations, weights and budgets: one statement of them


@pytest.mark.parametrize("case", ["b2_asym", "b2_nosep", "b2_unshared"])
def test_variant_matches_reference(case):
    g, meta = load_golden(case)
    cfg = TOOL.CFGS[case]
    B, N, M, D = meta["batch"], meta["n_enc"], meta["n_dec"], cfg.dim
    sd = TOOL.state_dict_for(cfg)
    md = synth.make_clip_batch(cfg, B, meta["budgets"], meta["seed"])
    md = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}
    eng = Engine(cfg, "cuda:0", max_batch=B, n_enc=N, n_dec=M)
    eng.load_state_dict(sd)
    order = [str(x) for x in g["dec_order"]]
    loss, mod_loss = eng.forward(md, dec_order=order)
    torch.cuda.synchronize()

    # ---- integer outputs: bit-exact (ids_keep indexes the concatenation of the side's own modalities, as in the reference)
    for ours, key in ((eng.ce["ids_keep"], "enc_ids_keep"), (eng.cd["ids_keep"], "dec_ids_keep"), (eng.ce["mod_mask"], "enc_mod_mask"),
                      (eng.cd["mod_mask"], "dec_mod_mask"), (eng.cd["tok"], "target_ids")):
        assert np.array_equal(ours[:B].cpu().numpy(), g[key]), key
    assert np.array_equal(eng.ce["pad"][:B].cpu().numpy().astype(bool), g["enc_pad"])
    assert np.array_equal(eng.cd["pad"][:B].cpu().numpy().astype(bool), g["dec_pad"])
    assert eng.cd["err"].item() == 0
    blocked = np.unpackbits(g["dec_attn_mask_packed"], axis=-1)[:, :, :M].astype(bool)
    ks, ke = eng.cd["ks"][:B].cpu().numpy(), eng.cd["ke"][:B].cpu().numpy()
    j = np.arange(M)[None, None, :]
    allowed = (j >= ks[:, :, None]) & (j < ke[:, :, None])
    valid = ~g["dec_pad"]                                 # (padding rows are consumed by nobody: theirs is the engine's own interval)
    assert np.array_equal(allowed[valid], ~blocked[valid])
    if case == "b2_nosep":                                # the staircase: later modalities see the earlier ones' keys
        assert (ks[valid] == 0).all() and len(np.unique(ke[0][valid[0]])) == 3 and eng._dec_groups() == {}

    # ---- taps
    def tap(key, t, n, rows_ok=None):
        t = t[:B * n].view(B, n, -1)[..., :D].float().cpu()
        e1 = rel_l2(t[:, :6, :24].numpy(), g[f"tap_head.{key}"])
        rn, ref = t.double().norm(dim=-1).numpy(), g[f"tap_rownorm.{key}"]
        if rows_ok is not None:
            rn, ref = rn[rows_ok], ref[rows_ok]
        return max(e1, rel_l2(rn, ref))
    assert tap("enc_x0", eng.enc[0]["x"], N) < 1e-6                      # exact fp32 gather + adds
    assert tap("dec_y0", eng.dec[0]["x"], M) < 1e-6                      # (the decoder's own mod_emb where there is one)
    held(f"{case}.tap.enc_out", tap("enc_out", eng.xe, N), hard=ACT_TOL)
    held(f"{case}.tap.context", tap("context", eng.ctx, N), hard=ACT_TOL)
    # decoder_norm output: written modality-grouped (eng.perm); valid rows only (the reference never reads the padding rows)
    vt = torch.from_numpy(valid).cuda()
    perm = eng.perm[:B * M].view(B, M)[vt].long()
    got = eng.yn[perm][:, :D].float().double().norm(dim=-1).cpu().numpy()
    held(f"{case}.tap.dec_out", rel_l2(got, g["tap_rownorm.dec_out"][valid]), hard=ACT_TOL)

    # ---- loss
    ref_loss = float(g["loss"])
    assert abs(loss.item() - ref_loss) < LOSS_RTOL * abs(ref_loss), (loss.item(), ref_loss)
    assert sorted(mod_loss) == sorted(m.name for m in cfg.dec_mods)
    for m in mod_loss:
        r = float(g[f"mod_loss.{m}"])
        assert abs(mod_loss[m].item() - r) < LOSS_RTOL * max(abs(r), 1.0), (m, mod_loss[m].item(), r)

    # ---- gradients: one norm per reference parameter, the mod_emb gradients element by element
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    worst = ("", 0.0)
    names = [str(n) for n in g["grad_names"]]
    assert names == meta["param_names"]
    for n, ref_sq in zip(names, g["grad_sqnorm_all"]):
        got_sq = eng.grad_of(n).double().pow(2).sum().item()
        if ref_sq < 0:
            assert got_sq == 0.0, n
            continue
        err = abs(got_sq ** 0.5 - ref_sq ** 0.5) / max(ref_sq ** 0.5, 1e-12)
        worst = max(worst, (n, err), key=lambda t: t[1])
    held(f"{case}.worst_grad_norm", worst[1], hard=GRAD_TOL)
    total = sum(eng.grad_of(n).double().pow(2).sum().item() for n in names) ** 0.5
    assert abs(total - float(g["grad_total_norm"])) < 1e-2 * float(g["grad_total_norm"])
    embs = [k[5:] for k in g.files if k.startswith("grad.")]
    assert any(n.startswith("decoder_embeddings") for n in embs) == (case != "b2_nosep")
    held(f"{case}.worst_mod_emb_grad", max(rel_l2(eng.grad_of(n).float().cpu().numpy(), g[f"grad.{n}"]) for n in embs), hard=GRAD_TOL)
