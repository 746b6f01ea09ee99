"""Activation checkpointing (`Engine(act_checkpoint=True)`, `EgoM2P(use_act_checkpoint=True)`, `--act_checkpoint`): every layer keeps its
fp32 input, the blocks of a stack run in one shared buffer set, the backward rebuilds a block in front of the block's backward.

The training path has no float atomics and the rebuild issues the forward's own launches on the forward's own operands, so the
acceptance test has NO tolerance: two engines from the same seeded weights, flag off and on, see the same batches and must agree with
`torch.equal` on the losses, on the whole flat gradient and, after a FusedAdamW step, on the whole flat parameter buffer - for every
place a rebuild can go wrong (depth, ragged rows, masks, model families, drop path, step structure).  The surface, the data-parallel
bucket order and the workspace accounting are checked beside it, and one reference fixture runs end to end through the checkpointing
engine.
"""
import dataclasses
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_engine_gpu as TE  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.model import MODALITY_INFO, create_model  # noqa: E402
from egom2p_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda:0"
TINY = MODEL_CFGS["ego_tiny_2e_2d"]                 # dim 128, 2 heads, cam + gaze (30 positions each): N = M = 30
MODS4 = ["tok_rgb", "tok_depth", "tok_cam", "tok_gaze"]
# two clips of the four modalities at N = 256, M = 320: a full one and a ragged one - pad rows on both sides, an EMPTY modality
# (depth), a modality without targets (cam), skewed segments
B2_BUDGETS = {"tok_rgb": [(140, 200), (60, 150)], "tok_depth": [(100, 90), (0, 0)], "tok_cam": [(10, 20), (30, 0)], "tok_gaze": [(6, 10), (5, 25)]}
B2_N, B2_M = 256, 320


def _depth(cfg, le, ld, **kw):
    return dataclasses.replace(cfg, encoder_depth=le, decoder_depth=ld, **kw)


def _pair(cfg, B, N, M, seed=3, **kw):
    """(plain, checkpointing) engines over the same seeded weights"""
    a = Engine(cfg, DEV, max_batch=B, n_enc=N, n_dec=M, **kw)
    b = Engine(cfg, DEV, max_batch=B, n_enc=N, n_dec=M, act_checkpoint=True, **kw)
    assert not a.act_checkpoint and b.act_checkpoint
    assert a.layout_tag() == b.layout_tag() and a.buckets == b.buckets and a.opt_runs == b.opt_runs and list(a.offsets.items()) == list(b.offsets.items())
    a.init_random(seed)
    b.P.copy_(a.P)
    b.weights_dirty = True
    # the checkpointing engine really shares: two layers of a stack name the same buffers, except their inputs
    for stack in (b.enc, b.dec):
        if len(stack) > 1:
            assert stack[0]["ln1"] is stack[1]["ln1"] and stack[0]["ab"] is stack[1]["ab"] and stack[0]["x"] is not stack[1]["x"]
    for stack in (a.enc, a.dec):
        if len(stack) > 1:
            assert stack[0]["ln1"] is not stack[1]["ln1"]
    return a, b


def _tiny_batch(cfg, B, seed, ragged=True):
    bud = synth.dirichlet_budgets(cfg, B, 30, 30, seed) if ragged else {m.name: (15, 15) for m in cfg.mods}
    return synth.make_clip_batch_device(cfg, B, bud, seed=seed, sample_offset=0, device=DEV)


def _b2_batch(cfg, seed=5, mods=None):
    md = synth.make_clip_batch(cfg, 2, {m.name: B2_BUDGETS[m.name] for m in cfg.mods}, seed)
    return {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items() if mods is None or k in mods}


def _run(eng, steps, opt=None, before=None, calls=None):
    """steps: optimiser steps, each a list of micro-batches (mod_dict, decoder order, loss_grad or None, training).  Returns every
    tensor the two engines must agree on, in order: per micro-batch the losses, per step the flat gradient and the flat parameters."""
    opt = opt or FusedAdamW(eng, lr=1e-3, weight_decay=0.05)
    out = []
    eng.zero_grad()
    for mbs in steps:
        for j, (md, order, lg, training) in enumerate(mbs):
            if before is not None:
                before(eng, j)
            loss, mod_loss = eng.forward(md, dec_order=order, loss_grad=lg, training=training)
            out.append(torch.stack([loss] + [mod_loss[n] for n in sorted(mod_loss)]).clone())
            eng.backward(lg if lg is not None else 1.0 / len(mbs), bucket_done=None if calls is None else (lambda *a: calls.append(a)))
        out.append(eng.G.clone())
        assert bool(torch.isfinite(eng.G).all()) and bool(eng.G.any())
        opt.step(clip_grad=1.0, zero_grad=True)
        out.append(eng.P.clone())
    torch.cuda.synchronize()
    return out


def _same(ra, rb):
    assert len(ra) == len(rb)
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert torch.equal(x, y), (k, tuple(x.shape), float((x.double() - y.double()).abs().max()))


def _names(cfg):
    return [m.name for m in cfg.mods]


# ---------------------------------------------------------------------------------------------- 1. depth, 2. ragged rows
@pytest.mark.parametrize("le,ld", [(3, 3), (1, 1), (2, 0), (0, 2)])
def test_depth(le, ld):
    """depth 3: a middle layer whose shared buffers were last written by its neighbour; depth 1: only the block the forward left
    resident; an empty stack.  Ragged Dirichlet budgets, 30 rows per sample (no tile multiple), a batch of 3 in a workspace of 4,
    two steps (the second over the first's stale shared buffers)."""
    cfg = _depth(TINY, le, ld)
    a, b = _pair(cfg, 4, 30, 30)
    order = _names(cfg)
    steps = [[(_tiny_batch(cfg, 3, 11), order, None, False)], [(_tiny_batch(cfg, 4, 12), order[::-1], 1.0, True)]]
    _same(_run(a, steps), _run(b, steps))


# ---------------------------------------------------------------------------------------------- 3. decoder masks, 4. families
FAMILIES = {
    "b2_standard_mask": ("ego_b_2e_2d", {}, {}, None),
    "per_row_launches": ("ego_384_2e_2d_causal", dict(decoder_causal_mask=False), {}, None),        # the round-3 per-row interval launches
    "causal_decoder": ("ego_384_2e_2d_causal", {}, {}, None),
    "qk_norm": ("ego_384_2e_2d_qknorm", {}, {}, None),
    "gelu_biased": ("ego_384_2e_2d_gelu", {}, {}, None),
    "register_tokens": ("ego_b_2e_2d_reg4", {}, {}, None),
    "modality_subset": ("ego_384_2e_2d_causal", dict(decoder_causal_mask=False), {}, ("tok_rgb", "tok_cam")),
    "padded_1020": ("ego_L_1020_2e_2d", {}, {}, None),
    "fp8_forward": ("ego_b_2e_2d", {}, dict(fp8_forward=True), None),
    "fp8_forward_backward": ("ego_b_2e_2d", {}, dict(fp8_forward=True, fp8_backward=True), None),
    "attn_o_residual_all": ("ego_384_2e_2d_causal", dict(decoder_causal_mask=False), dict(attn_o_residual="all"), None),
    "ctx_ln_per_layer": ("ego_384_2e_2d_causal", dict(decoder_causal_mask=False), {}, None),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_families_and_masks(family, monkeypatch):
    """the four modalities at B = 2 (a full clip and a ragged one), 3 + 3 layers so that a middle layer is rebuilt: the standard
    block-diagonal decoder mask by row groups and by per-row launches, the causal decoder, the head norms (their statistics must be
    rebuilt before their backward reads them), the biased family, register tokens, a modality subset, padded storage, the fp8 side
    buffers, every site's rounding residual, the chained context LayerNorm.  Two steps: plain CE, then the fused CE on a smaller batch."""
    name, repl, kw, subset = FAMILIES[family]
    if family == "ctx_ln_per_layer":
        monkeypatch.setenv("EGOM2P_CTX_LN_FUSED", "0")
    cfg = _depth(dataclasses.replace(MODEL_CFGS[name], **repl), 3, 3)
    a, b = _pair(cfg, 2, B2_N, B2_M, **kw)
    if family == "per_row_launches":
        a.attn_groups = b.attn_groups = False
    assert a.ctx_ln_fused == b.ctx_ln_fused == (family not in ("ctx_ln_per_layer", "fp8_forward", "fp8_forward_backward", "gelu_biased"))
    md = _b2_batch(cfg, mods=subset)
    order = [n for n in MODS4 if n in md]
    one = {k: {kk: vv[1:].contiguous() for kk, vv in v.items()} for k, v in md.items()}          # the ragged clip alone: B below the workspace batch
    steps = [[(md, order, None, False)], [(one, order[::-1], 1.0, True)]]
    _same(_run(a, steps), _run(b, steps))


# ---------------------------------------------------------------------------------------------- 5. drop path
def _dp_cfg():
    # per-stack linspace over 3 layers: rates 0, 0.1, 0.2 | 0, 0.2, 0.4 - a rebuilt middle layer that drops, a resident last one
    return _depth(MODEL_CFGS["ego_384_2e_2d_causal"], 3, 3, decoder_causal_mask=False, drop_path_rate_encoder=0.2, drop_path_rate_decoder=0.4)


def test_drop_path_injected_tables():
    """a sample dropped in every site kind, in the rebuilt layer and in the resident one: the rebuild reads the forward's keep table"""
    cfg = _dp_cfg()
    a, b = _pair(cfg, 2, B2_N, B2_M)
    assert len(b.dp_sites) == 2 * 2 + 2 * 3
    enc_t, dec_t = torch.ones(3, 2, 2, dtype=torch.bool), torch.ones(3, 3, 2, dtype=torch.bool)
    enc_t[1, :, 0] = False
    enc_t[2, :, 1] = False
    dec_t[1, :, 1] = False
    dec_t[2, :, 0] = False

    def before(eng, j):
        eng.inject_drop_path(enc_t, dec_t)

    md = _b2_batch(cfg)
    steps = [[(md, MODS4, 1.0, True)]]
    ra, rb = _run(a, steps, before=before), _run(b, steps, before=before)
    _same(ra, rb)
    # (sites in dp_sites order: encoder.1 attn / mlp, encoder.2 ..., decoder.1 self / cross / mlp, decoder.2 ...)
    assert torch.equal(a.drop_path_table(), b.drop_path_table())
    assert b.drop_path_table().cpu().tolist() == [[0, 1]] * 2 + [[1, 0]] * 2 + [[1, 0]] * 3 + [[0, 1]] * 3


def test_drop_path_drawn_table_and_counter():
    """the rebuild draws nothing: both engines used the table of (seed, counter) and advanced the counter once per forward"""
    cfg = _dp_cfg()
    a, b = _pair(cfg, 2, B2_N, B2_M)
    md = _b2_batch(cfg)
    tabs = {}

    def before(eng, j):
        if j == 0:
            eng.set_drop_path_seed(77, counter=3)

    steps = [[(md, MODS4, 0.5, True), (md, MODS4[::-1], 0.5, True)]]
    ra, rb = _run(a, steps, before=before), _run(b, steps, before=before)
    _same(ra, rb)
    for eng in (a, b):
        assert eng.dp_last == (77, 4) and eng._dp_counter == 5
        tabs[eng] = eng.drop_path_table()
    assert torch.equal(tabs[a], tabs[b])


# ---------------------------------------------------------------------------------------------- 6. step structure
def test_step_structure():
    """two micro-batches accumulated into G before one optimiser step, with the fused CE and without; a further step on the same
    engines; `resize_workspaces` to another (B, N, M), then a step"""
    cfg = _depth(TINY, 3, 3)
    a, b = _pair(cfg, 4, 30, 30)
    order = _names(cfg)
    steps = [[(_tiny_batch(cfg, 4, 21), order, 0.5, True), (_tiny_batch(cfg, 2, 22), order[::-1], 0.5, True)],
             [(_tiny_batch(cfg, 4, 23), order, None, False), (_tiny_batch(cfg, 3, 24), order, None, False)]]
    oa, ob = FusedAdamW(a, lr=1e-3), FusedAdamW(b, lr=1e-3)
    _same(_run(a, steps, opt=oa), _run(b, steps, opt=ob))
    wb = b.workspace_bytes()
    for eng in (a, b):
        eng.resize_workspaces(2, 24, 28)
    assert b.workspace_bytes()["total"] < wb["total"] and b.dcn is None and b.dec[0]["qkv"] is b.dec[2]["qkv"]
    bud = {m.name: [(12, 14), (9, 3)] for m in cfg.mods}
    md = synth.make_clip_batch_device(cfg, 2, bud, seed=25, sample_offset=0, device=DEV)
    steps = [[(md, order, 1.0, True)]]
    _same(_run(a, steps, opt=oa), _run(b, steps, opt=ob))
    # a backward needs a forward, as before
    with pytest.raises(AssertionError):
        b.backward(1.0)


# ---------------------------------------------------------------------------------------------- 7. data parallel, world 1
def test_bucket_done_sequence_is_unchanged():
    cfg = _depth(TINY, 3, 3)
    a, b = _pair(cfg, 2, 30, 30)
    md, order = _tiny_batch(cfg, 2, 31), _names(cfg)
    ca, cb = [], []
    _same(_run(a, [[(md, order, 1.0, True)]], calls=ca), _run(b, [[(md, order, 1.0, True)]], calls=cb))
    assert ca == cb and len(ca) == len(a.buckets) and {c[0] for c in ca} == {n for n, _, _ in a.buckets}


# ---------------------------------------------------------------------------------------------- 8. surface
def _model(**kw):
    mods = ["tok_cam", "tok_gaze"]
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}
    return create_model("egom2p_tiny_6e_6d_swiglu_nobias", encoder_embeddings=enc, decoder_embeddings=dec,
                        modality_info={m: MODALITY_INFO[m] for m in mods}, encoder_depth=3, decoder_depth=3, **kw)


def test_constructor_keyword_and_state_across_the_flag():
    """(fails on the parent: no `act_checkpoint` attribute) - and a model / optimiser state written with the flag off loads with it on
    and continues to the same bits"""
    import random
    plain, ck = _model(), _model(use_act_checkpoint=True)
    assert plain.engine.act_checkpoint is False and ck.engine.act_checkpoint is True
    assert plain.cfg.use_act_checkpoint is False and ck.cfg.use_act_checkpoint is True and ck.use_act_checkpoint is True
    assert list(plain.state_dict()) == list(ck.state_dict())
    cfg = plain.cfg
    mds = [_tiny_batch(cfg, 2, s) for s in (41, 42)]
    op, oc = FusedAdamW(plain.engine, lr=1e-3), FusedAdamW(ck.engine, lr=1e-3)

    def step(model, opt, md, seed):
        random.seed(seed)                      # the decoder-order shuffle
        model.train()
        loss, _ = model(md, 30, 30)
        loss.backward()
        opt.step(clip_grad=1.0, zero_grad=True)
        return loss.detach().clone()

    step(plain, op, mds[0], 1)
    ck.load_state_dict({k: v.clone() for k, v in plain.state_dict().items()})
    oc.load_state_dict({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in op.state_dict().items()})
    assert ck.engine.act_checkpoint is True
    lp, lc = step(plain, op, mds[1], 2), step(ck, oc, mds[1], 2)
    torch.cuda.synchronize()
    assert torch.equal(lp, lc) and torch.equal(plain.engine.P, ck.engine.P) and torch.equal(op.m, oc.m) and torch.equal(op.v, oc.v)
    # the engine flag alone, without the configuration's
    assert Engine(TINY, DEV, max_batch=1, n_enc=30, n_dec=30, act_checkpoint=True).act_checkpoint is True
    assert Engine(dataclasses.replace(TINY, use_act_checkpoint=True), DEV, max_batch=1, n_enc=30, n_dec=30).act_checkpoint is True


def test_training_script_writes_the_same_checkpoint(tmp_path):
    """(fails on the parent: the parser rejects --act_checkpoint) two optimiser steps of run_training_egom2p.py with and without
    the flag leave the same checkpoint-0.pth tensors"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_training_egom2p_amd_ck", os.path.join(root, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    common = ["--model", "egom2p_tiny_6e_6d_swiglu_nobias", "--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze",
              "--num_input_tokens", "32", "--num_target_tokens", "32", "--batch_size", "4", "--epochs", "1", "--epoch_size", "8",
              "--clip_grad", "1.0", "--blr", "1e-3", "--print_freq", "100", "--seed", "3"]
    env_keys = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") if k in os.environ}
    seen = []
    real = R.get_model

    def spy(args):
        model = real(args)
        seen.append(model.engine.act_checkpoint)
        return model

    R.get_model = spy
    try:
        a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
        R.main(R.get_args(common + ["--output_dir", a_dir]))
        R.main(R.get_args(common + ["--output_dir", b_dir, "--act_checkpoint"]))
    finally:
        os.environ.update(env_keys)
    assert seen == [False, True]
    ca = torch.load(os.path.join(a_dir, "checkpoint-0.pth"), map_location="cpu", weights_only=True)
    cb = torch.load(os.path.join(b_dir, "checkpoint-0.pth"), map_location="cpu", weights_only=True)
    assert ca["optimizer"]["t"] == cb["optimizer"]["t"] == 2 and ca["args"]["act_checkpoint"] is False and cb["args"]["act_checkpoint"] is True
    assert list(ca["model"]) == list(cb["model"])
    for k, v in ca["model"].items():
        assert torch.equal(v, cb["model"][k]), k
    for k in ("m", "v"):
        assert torch.equal(ca["optimizer"][k], cb["optimizer"][k]), k


# ---------------------------------------------------------------------------------------------- 9. memory
def _nbytes(d, skip=()):
    return sum(t.numel() * t.element_size() for k, t in d.items() if t is not None and k not in skip)


@pytest.mark.parametrize("name,kw", [("ego_tiny_2e_2d", {}), ("ego_384_2e_2d_qknorm", dict(attn_o_residual="all"))])
def test_workspace_bytes(name, kw):
    """(fails on the parent: no `workspace_bytes`) under the flag a layer saves rows * D * 4 bytes, the shared sets are one encoder and
    one decoder layer's buffers, and at depth 3 the total falls by two layers' buffers per stack - all from the plain engine's shapes"""
    cfg = _depth(MODEL_CFGS[name], 3, 3)
    B, N, M = 3, 30, 30
    a = Engine(cfg, DEV, max_batch=B, n_enc=N, n_dec=M, **kw)
    b = Engine(cfg, DEV, max_batch=B, n_enc=N, n_dec=M, act_checkpoint=True, **kw)
    wa, wb = a.workspace_bytes(), b.workspace_bytes()
    assert set(wa) == set(wb) == {"saved", "shared", "other", "backward", "total"}
    for w in (wa, wb):
        assert w["total"] == w["saved"] + w["shared"] + w["other"] + w["backward"]
    enc_rest, dec_rest = _nbytes(a.enc[0], skip=("x",)), _nbytes(a.dec[0], skip=("x",))
    assert enc_rest > 0 and dec_rest > 0
    assert wa["shared"] == 0 and wa["saved"] == 3 * (_nbytes(a.enc[0]) + _nbytes(a.dec[0]))
    assert wb["saved"] == 3 * (B * N * a.D * 4) + 3 * (B * M * a.D * 4)
    assert wb["shared"] == enc_rest + dec_rest
    assert set(b.enc_sh) == set(a.enc[0]) - {"x"} and set(b.dec_sh) == set(a.dec[0]) - {"x"}
    for k in b.enc_sh:
        assert (b.enc_sh[k] is None) == (a.enc[0][k] is None) and (b.enc_sh[k] is None or (b.enc_sh[k].shape, b.enc_sh[k].dtype) == (a.enc[0][k].shape, a.enc[0][k].dtype)), k
    for k in b.dec_sh:
        assert (b.dec_sh[k] is None) == (a.dec[0][k] is None) and (b.dec_sh[k] is None or (b.dec_sh[k].shape, b.dec_sh[k].dtype) == (a.dec[0][k].shape, a.dec[0][k].dtype)), k
    assert wb["other"] == wa["other"] and wb["backward"] == wa["backward"]
    assert wa["total"] - wb["total"] == 2 * enc_rest + 2 * dec_rest > 0
    # the fused context LayerNorm's per-layer gradient buffers appear once a backward made them: the same in both engines
    md = _tiny_batch(cfg, B, 51) if name == "ego_tiny_2e_2d" else None
    if md is not None:
        for eng in (a, b):
            eng.init_random(1)
            eng.forward(md, dec_order=_names(cfg))
            eng.backward(1.0)
        assert a.workspace_bytes()["backward"] == b.workspace_bytes()["backward"] == wa["backward"] + 3 * a.Bmax * a.Ne * a.D * 2


# ---------------------------------------------------------------------------------------------- 10. reference
def test_reference_fixture_through_the_checkpointing_engine(monkeypatch):
    """tests/golden/b2.npz end to end - integer outputs, taps, losses, logits, gradients, AdamW, the recorded parity bars - with every
    engine of the existing parity test built checkpointing"""
    built = []

    def make(*a, **k):
        built.append(Engine(*a, act_checkpoint=True, **k))
        return built[-1]

    monkeypatch.setattr(TE, "Engine", make)
    TE.test_engine_matches_reference("b2")
    assert len(built) == 1 and built[0].act_checkpoint and built[0].enc[0]["qkv"] is built[0].enc[1]["qkv"]
