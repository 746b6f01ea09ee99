"""The causal decoder variant (`decoder_causal_mask=True`, egom2p_model.py:459-463, 1029-1051) and modality-subset batches
(:706-714) on the GPU: compaction, the attention kernels on causal intervals, and `EgoM2P.forward` / backward against fixtures
made from the real reference (tools/make_goldens_variants.py: tests/golden/b2_causal.npz, b2_subset.npz).

Tolerances are the ones of the tests these extend: `ATT_FWD_TOL` / `ATT_BWD_TOL` of tests/test_kernels_gpu.py for the attention
kernels' per-row-interval cases, `ACT_TOL` / `GRAD_TOL` / `LOSS_RTOL` of tests/test_engine_gpu.py for the fp32 reference fixtures."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_engine_gpu as TE  # noqa: E402
import test_kernels_gpu as TK  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.masking import causal_decoder_intervals  # noqa: E402
from egom2p_amd.model import MODALITY_INFO, create_model  # noqa: E402

DEV = "cuda"
CAUSAL_NAME = "egom2p_base_12e_12d_swiglu_nobias_causal"
MODS = ["tok_rgb", "tok_depth", "tok_cam", "tok_gaze"]
_CACHE = {}


def _case(name):
    """fixture + the seeded weights and clips it was made from (built once, left unchanged)"""
    if name not in _CACHE:
        g, meta = load_golden(name)
        cfg = MODEL_CFGS[meta["cfg"]]
        key = ("inputs", meta["cfg"], meta["seed"], repr(meta["budgets"]))
        if key not in _CACHE:
            sd = synth.build_state_dict(cfg, meta["seed"])
            md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
            _CACHE[key] = (sd, {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()})
        _CACHE[name] = (g, meta, cfg) + _CACHE[key]
    return _CACHE[name]


def _model(name, **kw):
    """the registered variant `name` at the fixtures' width and depth (dim 384, 6 heads, 2 + 2 layers)"""
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}
    return create_model(name, encoder_embeddings=enc, decoder_embeddings=dec, modality_info=MODALITY_INFO, dim=384, num_heads=6,
                        encoder_depth=2, decoder_depth=2, **kw)


def _causal_model():
    if "model" not in _CACHE:
        g, meta, cfg, sd, md = _case("b2_causal")
        model = _model(CAUSAL_NAME)
        assert model.decoder_causal_mask and model.cfg.decoder_causal_mask
        assert set(model.state_dict().keys()) == set(sd.keys())
        model.load_state_dict(sd)
        _CACHE["model"] = model
    return _CACHE["model"]


# ---------------------------------------------------------------------------------------------- compaction
def _side(B, n, n_mods):
    def e(*s, dt=torch.int32):
        return torch.zeros(*s, device=DEV, dtype=dt)
    return dict(ids_keep=e(B, n, dt=torch.int64), pad=e(B, n, dt=torch.uint8), mod_mask=e(B, n, dt=torch.int16), slot=e(B, n), local=e(B, n),
                tok=e(B, n), ks=e(B, n), ke=e(B, n), n_valid=e(B), seg=e(B, n_mods, 2), err=e(1), seg_bad=e(B))


def test_compaction_in_causal_mode():
    g, meta, cfg, sd, md = _case("b2_causal")
    B, M = meta["batch"], meta["n_dec"]
    byname = {m.name: m for m in cfg.mods}
    dmods = [byname[str(n)] for n in g["dec_order"]]
    args = ([md[m.name]["target_mask"] for m in dmods], [md[m.name]["tensor"].reshape(B, -1).contiguous() for m in dmods],
            [md[m.name]["decoder_attention_mask"] for m in dmods], [m.max_tokens for m in dmods], [m.id for m in dmods], M, True)
    plain, causal = _side(B, M, len(dmods)), _side(B, M, len(dmods))
    ops.compact(*args, plain, B)
    ops.compact(*args, causal, B, causal=True)
    torch.cuda.synchronize()
    ks, ke = causal_decoder_intervals(g["dec_mod_mask"])
    assert np.array_equal(causal["ks"].cpu().numpy(), ks) and np.array_equal(causal["ke"].cpu().numpy(), ke)
    assert causal["err"].item() == 0 and plain["err"].item() == 0
    for k in ("n_valid", "ids_keep", "pad", "mod_mask", "slot", "local", "tok", "seg"):
        assert torch.equal(causal[k], plain[k]), k
    assert np.array_equal(causal["ids_keep"].cpu().numpy(), g["dec_ids_keep"])
    assert np.array_equal(causal["mod_mask"].cpu().numpy(), g["dec_mod_mask"])
    # both samples have a group of more than one row: neither may take the uniform row-group path of the attention kernels
    assert causal["seg_bad"].bool().all() and not plain["seg_bad"].bool().any()
    # groups of at most one row share their interval trivially: such a sample keeps the group path
    one = {n: {"tensor": d["tensor"][:1], "decoder_attention_mask": d["decoder_attention_mask"][:1],
               "target_mask": torch.ones_like(d["target_mask"][:1])} for n, d in md.items()}
    for n in one:
        one[n]["target_mask"][0, 3] = False
    s1 = _side(1, 8, len(dmods))
    ops.compact([one[m.name]["target_mask"] for m in dmods], [one[m.name]["tensor"].reshape(1, -1).contiguous() for m in dmods],
                [one[m.name]["decoder_attention_mask"] for m in dmods], [m.max_tokens for m in dmods], [m.id for m in dmods], 8, True,
                s1, 1, causal=True)
    assert s1["seg_bad"].item() == 0 and s1["n_valid"].item() == 4 and s1["err"].item() == 0
    assert s1["ks"][0].tolist() == [0, 1, 2, 3, 0, 0, 0, 0] and s1["ke"][0].tolist() == [1, 2, 3, 4, 4, 4, 4, 4]
    # the encoder side has no causal mode
    with pytest.raises(Exception):
        ops.compact(args[0], args[1], None, args[3], args[4], M, False, _side(B, M, len(dmods)), B, causal=True)


# ---------------------------------------------------------------------------------------------- attention kernels
@pytest.mark.parametrize("N,groups", [(320, (200, 120)), (97, (60, 37))])
def test_attention_kernels_on_causal_intervals(N, groups):
    """ego_attn_fwd_d64 / ego_attn_bwd_d64 (the per-row interval class) on ks = g0, ke = r + 1 against fp32 torch attention under
    the dense mask: 320 rows = a group across two 128-row query tiles and four 64-key tiles with the diagonal inside tiles, 97
    rows = a ragged last tile.  Error measure and bars: those of test_kernels_gpu.test_attention_fwd_bwd."""
    torch.manual_seed(1234)
    B, H, D = 2, 2, 128
    qb = TK._bf(torch.randn(B, N, D, device=DEV))
    kvb = TK._bf(torch.randn(B, N, 2, D, device=DEV))
    mm = np.concatenate([np.full(c, i + 1) for i, c in enumerate(groups)])[None].repeat(B, 0)
    ks_h, ke_h = causal_decoder_intervals(mm)
    ks, ke = torch.from_numpy(ks_h).to(DEV), torch.from_numpy(ke_h).to(DEV)
    scale = 64 ** -0.5
    q = qb.view(B, N, H, 64).permute(0, 2, 1, 3).float().requires_grad_(True)
    k = kvb[:, :, 0].reshape(B, N, H, 64).permute(0, 2, 1, 3).float().requires_grad_(True)
    v = kvb[:, :, 1].reshape(B, N, H, 64).permute(0, 2, 1, 3).float().requires_grad_(True)
    blocked = torch.ones(N, N, dtype=torch.bool, device=DEV).triu(1)[None] | (torch.from_numpy(mm).to(DEV)[:, None, :] != torch.from_numpy(mm).to(DEV)[:, :, None])
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(blocked[:, None], -torch.finfo(torch.float32).max)
    ref = s.softmax(-1) @ v
    o = torch.empty(B, N, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=DEV)
    kp, vp = kvb.data_ptr(), kvb.data_ptr() + D * 2
    ops.attn_fwd(qb.data_ptr(), N * D, D, kp, N * 2 * D, 2 * D, vp, N * 2 * D, 2 * D, o.data_ptr(), N * D, D, lse, ks, ke, N, 1, B, H, N, N, scale)
    e_fwd = TK._rel(o.view(B, N, H, 64).permute(0, 2, 1, 3).float(), ref)
    do = TK._bf(torch.randn(B, N, D, device=DEV))
    ref.backward(do.view(B, N, H, 64).permute(0, 2, 1, 3).float())
    runs = []
    for _ in range(2):
        dq = torch.zeros(B, N, D, device=DEV, dtype=torch.bfloat16)
        dkv = torch.zeros(B, N, 2, D, device=DEV, dtype=torch.bfloat16)
        delta = torch.empty(B, H, N, device=DEV)
        ops.attn_bwd(qb.data_ptr(), N * D, D, kp, N * 2 * D, 2 * D, vp, N * 2 * D, 2 * D, o.data_ptr(), N * D, D, do.data_ptr(), N * D, D, lse, delta,
                     dq.data_ptr(), N * D, D, dkv.data_ptr(), N * 2 * D, 2 * D, dkv.data_ptr() + D * 2, N * 2 * D, 2 * D, ks, ke, N, 1, B, H, N, N, scale)
        runs.append((dq, dkv))
    torch.cuda.synchronize()
    dq, dkv = runs[0]
    e_dq = TK._rel(dq.view(B, N, H, 64).permute(0, 2, 1, 3).float(), q.grad)
    e_dk = TK._rel(dkv[:, :, 0].reshape(B, N, H, 64).permute(0, 2, 1, 3).float(), k.grad)
    e_dv = TK._rel(dkv[:, :, 1].reshape(B, N, H, 64).permute(0, 2, 1, 3).float(), v.grad)
    print(f"causal attention N={N}: fwd {e_fwd:.3e} dq {e_dq:.3e} dk {e_dk:.3e} dv {e_dv:.3e}")
    assert e_fwd < TK.ATT_FWD_TOL
    assert e_dq < TK.ATT_BWD_TOL and e_dk < TK.ATT_BWD_TOL and e_dv < TK.ATT_BWD_TOL
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # dQ, dK, dV bit for bit


# ---------------------------------------------------------------------------------------------- module against the fixtures
def _dec_tap_err(g, key, t, valid):
    """decoder taps: the fixture's head slice (rows 0..5 of each sample: valid) and the row norms of the VALID rows (padding rows
    are consumed by nothing in the reference: mod_mask -1)"""
    t = t.float().cpu()
    e1 = rel_l2(t[:, :6, :24].numpy(), g[f"tap_head.{key}"])
    e2 = rel_l2(t.double().norm(dim=-1).numpy()[valid], g[f"tap_rownorm.{key}"][valid])
    return max(e1, e2)


def _check_against_fixture(model, case, present, zero_grad=True):
    g, meta, cfg, sd, md = _case(case)
    eng = model.engine
    B, N, M, D = meta["batch"], meta["n_enc"], meta["n_dec"], cfg.dim
    random.seed(meta["py_seed"])                       # the golden run's python-random state -> the same decoder order (:312)
    if zero_grad:
        eng.zero_grad()
    loss, mod_loss = model({n: md[n] for n in present}, N, M, loss_type="mod")
    torch.cuda.synchronize()
    assert [m.name for m in eng.dmods] == [str(x) for x in g["dec_order"]]
    assert set(mod_loss.keys()) == set(present)
    # integer outputs: bit-exact
    assert np.array_equal(eng.ce["ids_keep"][:B].cpu().numpy(), g["enc_ids_keep"])
    assert np.array_equal(eng.cd["ids_keep"][:B].cpu().numpy(), g["dec_ids_keep"])
    assert np.array_equal(eng.ce["pad"][:B].cpu().numpy().astype(bool), g["enc_pad"])
    assert np.array_equal(eng.cd["pad"][:B].cpu().numpy().astype(bool), g["dec_pad"])
    assert np.array_equal(eng.ce["mod_mask"][:B].cpu().numpy(), g["enc_mod_mask"])
    assert np.array_equal(eng.cd["mod_mask"][:B].cpu().numpy(), g["dec_mod_mask"])
    assert np.array_equal(eng.cd["tok"][:B].cpu().numpy(), g["target_ids"])
    assert eng.cd["err"].item() == 0
    valid = ~g["dec_pad"]
    blocked = np.unpackbits(g["dec_attn_mask_packed"], axis=-1)[:, :, :M].astype(bool)
    ks, ke = eng.cd["ks"][:B].cpu().numpy(), eng.cd["ke"][:B].cpu().numpy()
    j = np.arange(M)[None, None, :]
    assert np.array_equal(((j >= ks[:, :, None]) & (j < ke[:, :, None]))[valid], ~blocked[valid])
    # taps
    RN, RM = B * N, B * M
    act = lambda t, rows, n: t[:rows].view(B, n, D)      # noqa: E731
    assert TE._tap(g, "enc_x0", act(eng.enc[0]["x"], RN, N)) < 1e-6
    assert TE._tap(g, "enc_block0", act(eng.enc[1]["x"], RN, N)) < TE.ACT_TOL
    assert TE._tap(g, "enc_out", act(eng.xe, RN, N)) < TE.ACT_TOL
    assert TE._tap(g, "context", act(eng.ctx, RN, N)) < TE.ACT_TOL
    assert _dec_tap_err(g, "dec_y0", act(eng.dec[0]["x"], RM, M), valid) < 1e-6
    e_blk = _dec_tap_err(g, "dec_block0", act(eng.dec[1]["x"], RM, M), valid)
    vt = torch.from_numpy(valid).cuda()
    perm = eng.perm[:RM].view(B, M)[vt].long()
    e_out = rel_l2(eng.yn[perm][:, :D].float().norm(dim=-1).cpu().numpy(), g["tap_rownorm.dec_out"][valid])
    print(f"{case}: dec_block0 {e_blk:.3e} dec_out row norms {e_out:.3e} loss {loss.item():.6f} (reference {float(g['loss']):.6f})")
    assert e_blk < TE.ACT_TOL and e_out < TE.ACT_TOL
    # loss
    ref_loss = float(g["loss"])
    assert abs(loss.item() - ref_loss) < TE.LOSS_RTOL * abs(ref_loss), (loss.item(), ref_loss)
    for n in present:
        r = float(g[f"mod_loss.{n}"])
        assert abs(mod_loss[n].item() - r) < TE.LOSS_RTOL * max(abs(r), 1.0), (n, mod_loss[n].item(), r)
    # gradients: one norm per tensor (the reference's None = exactly zero here), the recorded slices after the clip
    loss.backward()
    torch.cuda.synchronize()
    worst = ("", 0.0)
    for n, ref_sq in zip([str(x) for x in g["grad_names"]], g["grad_sqnorm_all"]):
        got_sq = eng.grad_of(n).double().pow(2).sum().item()
        if ref_sq < 0:
            assert got_sq == 0.0, n
            continue
        err = abs(got_sq ** 0.5 - ref_sq ** 0.5) / max(ref_sq ** 0.5, 1e-12)
        worst = max(worst, (n, err), key=lambda x: x[1])
    print(f"{case}: worst gradient norm error {worst}")
    assert worst[1] < TE.GRAD_TOL, worst
    coef = min(1.0, 1.0 / (float(g["clip_total_norm"]) + 1e-6))
    for key in g.files:
        if key.startswith("grad_head."):
            gr = eng.grad_of(key[10:]) * coef
            e = rel_l2(gr.reshape(-1, gr.shape[-1])[:4, :32].float().cpu().numpy(), g[key])
            assert e < 2 * TE.GRAD_TOL, (key, e)
    return g, eng, valid


def test_causal_model_matches_the_reference_fixture():
    model = _causal_model()
    g, eng, valid = _check_against_fixture(model, "b2_causal", MODS)
    # the mask matters: the same weights through the standard (non-causal) variant leave the fixture's decoder tap
    _, meta, cfg, sd, md = _case("b2_causal")
    plain = _model("egom2p_tiny_6e_6d_swiglu_nobias")
    plain.load_state_dict(sd)
    random.seed(meta["py_seed"])
    with torch.no_grad():
        plain(md, meta["n_enc"], meta["n_dec"])
    B, M = meta["batch"], meta["n_dec"]
    e = _dec_tap_err(g, "dec_block0", plain.engine.dec[1]["x"][:B * M].view(B, M, cfg.dim), valid)
    print(f"non-causal model against the causal fixture: dec_block0 {e:.3e}")
    assert e > TE.ACT_TOL, e


def test_modality_subset_matches_the_reference_fixture():
    model = _causal_model()
    present = ["tok_rgb", "tok_cam"]
    g, eng, _ = _check_against_fixture(model, "b2_subset", present)
    # gradients of everything that belongs to an absent modality: exactly zero
    for n in ("tok_depth", "tok_gaze"):
        for key in (f"encoder_embeddings.{n}.token_emb.weight", f"decoder_embeddings.{n}.token_emb.weight", f"encoder_embeddings.{n}.mod_emb"):
            assert not bool(eng.grad_of(key).any()), key
    # the same subset under no_grad and with return_logits
    _, meta, cfg, sd, md = _case("b2_subset")
    sub = {n: md[n] for n in present}
    B, N, M = meta["batch"], meta["n_enc"], meta["n_dec"]
    random.seed(meta["py_seed"])
    with torch.no_grad():
        l2, ml2 = model(sub, N, M)
        assert not l2.requires_grad and set(ml2) == set(present)
        assert abs(l2.item() - float(g["loss"])) < TE.LOSS_RTOL * float(g["loss"])
        random.seed(meta["py_seed"])
        logits = model(sub, N, M, return_logits=True)
    assert set(logits) == set(present)
    assert logits["tok_rgb"].shape == (B, M, 64000) and logits["tok_cam"].shape == (B, M, 256)
    assert torch.isfinite(logits["tok_cam"].float()).all()
    # reuse across changing subsets: all four modalities through the same module still match the full fixture
    _check_against_fixture(model, "b2_causal", MODS)
    # what the reference's embedding lookup refuses
    with pytest.raises((KeyError, ValueError)):
        model({**sub, "tok_audio": md["tok_cam"]}, N, M)
    with pytest.raises(ValueError):
        model({}, N, M)


def test_sparse_table_exchange_with_an_untouched_table():
    """a step in which a modality is absent touches no row of its encoder table: the row-list exchange moves an empty list"""
    from egom2p_amd.dp import SparseTableExchange
    torch.manual_seed(3)
    g0, g1 = torch.randn(300, 128, device=DEV), torch.randn(300, 128, device=DEV)
    t0, t1 = torch.zeros(300, device=DEV, dtype=torch.uint8), torch.zeros(300, device=DEV, dtype=torch.uint8)
    t1[[5, 77, 299]] = 1
    want0, want1 = g0.clone(), g1.clone()
    ex = SparseTableExchange([(g0, t0), (g1, t1)], cap_rows=64)
    ex.exchange()
    torch.cuda.synchronize()
    assert not ex.overflowed()
    assert ex.tables[0]["count"].item() == 0 and ex.tables[1]["count"].item() == 3
    assert torch.equal(g0, want0) and torch.equal(g1, want1) and not bool(t1.any())
