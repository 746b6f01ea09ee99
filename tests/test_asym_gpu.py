"""Asymmetric models on the GPU: `ego_compact_nosep` against a numpy restatement of adapt_decoder_attention_mask without its
separation term (exact integers), the engine identities that tie an asymmetric / unshared / no-separation model to the symmetric
shared one on the same weights, training through run_training_egom2p.py, generation with an rgb -> depth specialist, and the device
masking under zero alphas.  Model scale: dim 384, 6 heads, 2 + 2 layers, B <= 3."""
import importlib.util
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _asym_bars import held  # noqa: E402
from conftest import rel_l2  # noqa: E402
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODALITIES, ModelCfg  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.masking import nosep_decoder_intervals  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FP32_TOL = 2e-5          # the project's fp32 bar (tests/test_oracle_vs_goldens.py): the same sum in another fp32 order

SYM = ModelCfg("sym3", 384, 2, 2, 6, modalities=("tok_rgb", "tok_depth", "tok_cam"))
ASYM = replace(SYM, name="asym", encoder_modalities=("tok_rgb", "tok_cam"), decoder_modalities=("tok_depth", "tok_cam"))


# ------------------------------------------------------------------------------------------------ 1. ego_compact_nosep, exact
MODS = [MODALITIES[n] for n in ("tok_rgb", "tok_cam", "tok_gaze")]            # T = 5180: 21 groups of 256 positions, all 8 CP_SPLIT parts
T = sum(m.max_tokens for m in MODS)


def _decoder_side(counts, dam_rule, seed):
    """target masks with counts[b][m] random target positions per sample and modality, and a decoder_attention_mask per rule:
    'first' - the data contract (the target count at the modality's first target position, masking.py:262-264); 'ones' - 1 on every
    target (strictly autoregressive); 'over' - the contract plus 5 on the first count (a pad key becomes visible: err)."""
    rng = np.random.RandomState(seed)
    B = len(counts)
    masks, ids, dams = [], [], []
    for j, m in enumerate(MODS):
        mk = np.ones((B, m.max_tokens), bool)
        dm = np.zeros((B, m.max_tokens), np.int32)
        for b in range(B):
            pos = np.sort(rng.permutation(m.max_tokens)[:counts[b][j]])
            mk[b, pos] = False
            rule = dam_rule[b]
            if len(pos):
                if rule == "ones":
                    dm[b, pos] = 1
                else:
                    dm[b, pos[0]] = len(pos) + (5 if rule == "over" and j == 0 else 0)
        masks.append(torch.from_numpy(mk).to(DEV))
        ids.append(torch.from_numpy(rng.randint(0, m.vocab_size, (B, m.max_tokens)).astype(np.int64)).to(DEV))
        dams.append(torch.from_numpy(dm).to(DEV))
    return masks, ids, dams


def _compact(masks, ids, dams, n_keep, B, **kw):
    i32 = dict(device=DEV, dtype=torch.int32)
    out = {k: torch.full((B, n_keep), -77, device=DEV, dtype=dt) for k, dt in (
        ("ids_keep", torch.int64), ("pad", torch.uint8), ("mod_mask", torch.int16), ("slot", torch.int32), ("local", torch.int32),
        ("tok", torch.int32), ("ks", torch.int32), ("ke", torch.int32))}
    out.update(n_valid=torch.zeros(B, **i32), seg=torch.zeros(B, len(MODS), 2, **i32), err=torch.zeros(1, **i32), seg_bad=torch.zeros(B, **i32))
    ops.compact(masks, ids, dams, [m.max_tokens for m in MODS], [m.id for m in MODS], n_keep, True, out, B, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# per sample (rgb, cam, gaze) target counts: 300 valid (rgb spans two query tiles), 200 valid with NO gaze target, 41 valid
COUNTS = [[250, 20, 30], [180, 20, 0], [1, 30, 10]]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("n_keep", [256, 512])         # 256: sample 0 is cut inside cam (250 + 6 rows), no padding there; 512: padding everywhere
@pytest.mark.parametrize("rules", [("first", "ones", "first"), ("first", "over", "ones")])
def test_compact_nosep_is_the_reference_mask_without_separation(causal, n_keep, rules):
    B = len(COUNTS)
    masks, ids, dams = _decoder_side(COUNTS, rules, seed=11)
    sep = _compact(masks, ids, dams, n_keep, B, causal=causal)
    got = _compact(masks, ids, dams, n_keep, B, causal=causal, sep=False)
    for k in ("ids_keep", "pad", "mod_mask", "slot", "local", "tok", "n_valid", "seg"):       # everything but the intervals: ego_compact's
        assert np.array_equal(got[k], sep[k]), k
    # adapt_decoder_attention_mask (egom2p_model.py:446-481 without :476-479) on the gathered rows, in numpy
    dam_all = np.concatenate([d.cpu().numpy() for d in dams], axis=1)
    dam_keep = np.take_along_axis(dam_all, got["ids_keep"], axis=1)
    j = np.arange(n_keep)
    if causal:
        blocked = np.broadcast_to(np.triu(np.ones((n_keep, n_keep), bool), 1), (B, n_keep, n_keep))
    else:
        blocked = j[None, None, :] >= np.cumsum(dam_keep, axis=1)[:, :, None]
    allowed = (j[None, None, :] >= got["ks"][:, :, None]) & (j[None, None, :] < got["ke"][:, :, None])
    valid = got["pad"] == 0
    assert valid.sum(1).tolist() == [min(sum(c), n_keep) for c in COUNTS]
    assert np.array_equal(allowed[valid], ~blocked[valid])                                   # every kept row: exactly [ks, ke)
    assert (got["ks"] == 0).all()
    for b in range(B):                                                                        # padding rows: every valid key
        assert (got["ke"][b][~valid[b]] == got["n_valid"][b]).all()
    ks, ke = nosep_decoder_intervals(got["mod_mask"], dam_keep, causal=causal)               # the host restatement agrees
    assert np.array_equal(ks, got["ks"]) and np.array_equal(ke, got["ke"])
    # seg_bad: raised exactly for the samples with a kept row whose interval is not its slot's segment
    want_bad = []
    for b in range(B):
        bad = False
        for r in np.nonzero(valid[b])[0]:
            s0, c = got["seg"][b, got["slot"][b, r]]
            bad |= (got["ks"][b, r], got["ke"][b, r]) != (s0, s0 + c)
        want_bad.append(int(bad))
    assert (got["seg_bad"] != 0).astype(int).tolist() == want_bad and sum(want_bad) > 0
    # err: the cumsum mode's "a padding key would be visible" rule, as ego_compact raises it; never under the causal mask
    over = any(r == "over" and sum(c) < n_keep for r, c in zip(rules, COUNTS))
    assert int(got["err"][0]) == int(sep["err"][0]) == (0 if causal else int(over))


def test_compact_nosep_single_modality_needs_no_per_row_path():
    """one non-empty slot under the data contract: every row's interval IS the segment - seg_bad stays clear, intervals equal ego_compact's"""
    masks, ids, dams = _decoder_side([[140, 0, 0], [0, 0, 25]], ("first", "first"), seed=3)
    sep, got = _compact(masks, ids, dams, 160, 2), _compact(masks, ids, dams, 160, 2, sep=False)
    assert got["seg_bad"].tolist() == [0, 0] and int(got["err"][0]) == 0
    valid = got["pad"] == 0
    assert np.array_equal(got["ks"][valid], sep["ks"][valid]) and np.array_equal(got["ke"][valid], sep["ke"][valid])


def test_compact_nosep_rejects_the_encoder_side():
    masks, ids, dams = _decoder_side([[5, 5, 5]], ("first",), seed=1)
    from egom2p_amd import _lib as L
    i32 = dict(device=DEV, dtype=torch.int32)
    out = {k: torch.zeros(1, 8, device=DEV, dtype=dt) for k, dt in (("ids_keep", torch.int64), ("pad", torch.uint8), ("mod_mask", torch.int16),
           ("slot", torch.int32), ("local", torch.int32), ("tok", torch.int32), ("ks", torch.int32), ("ke", torch.int32))}
    out.update(n_valid=torch.zeros(1, **i32), seg=torch.zeros(1, 3, 2, **i32), err=torch.zeros(1, **i32))
    with pytest.raises(L.EgoHipError):
        ops.compact(masks, ids, None, [m.max_tokens for m in MODS], [m.id for m in MODS], 8, False, out, 1, sep=False)


# ------------------------------------------------------------------------------------------------ 2. engine identities
N_ENC, N_DEC = 192, 200
# sample 0 / 1 (inputs, targets): rgb is input only, depth target only - the batch an asymmetric {rgb, cam} -> {depth, cam} model sees
BUDGETS = {"tok_rgb": [(100, 0), (120, 0)], "tok_depth": [(0, 130), (0, 90)], "tok_cam": [(12, 10), (15, 8)]}
FULL = {"tok_rgb": [(80, 70), (60, 50)], "tok_depth": [(50, 90), (70, 60)], "tok_cam": [(12, 10), (15, 8)]}


def _engine(cfg, sd):
    eng = Engine(cfg, DEV, max_batch=2, n_enc=N_ENC, n_dec=N_DEC)
    eng.load_state_dict(sd)
    return eng


def _batch(budgets, seed=5):
    md = synth.make_clip_batch(SYM, 2, budgets, seed)
    return {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in md.items()}


def _step(eng, md, order, loss_type="mod"):
    eng.zero_grad()
    loss, mod_loss = eng.forward(md, dec_order=order, loss_type=loss_type)
    eng.backward(1.0)
    torch.cuda.synchronize()
    return loss.clone(), {k: v.clone() for k, v in mod_loss.items()}


def test_asymmetric_model_equals_the_symmetric_one_on_its_batch():
    """(a) encoder {rgb, cam} / decoder {depth, cam} against the symmetric {rgb, depth, cam} model on a batch where rgb has no targets
    and depth no inputs, loss_type 'token' (an empty modality weighs 0): the same rows in the same order through kernels without
    atomics - per-modality losses, the total and every gradient both models own, bit for bit."""
    sd = synth.build_state_dict(SYM, seed=4)
    sym, asym = _engine(SYM, sd), _engine(ASYM, sd)
    assert "decoder_embeddings.tok_depth.mod_emb" in asym.p and "encoder_embeddings.tok_depth.mod_emb" not in asym.p
    md = _batch(BUDGETS)
    ls, ms = _step(sym, md, ["tok_depth", "tok_cam", "tok_rgb"], "token")
    la, ma = _step(asym, md, ["tok_depth", "tok_cam"], "token")
    assert sorted(ma) == ["tok_cam", "tok_depth"]
    assert torch.isfinite(la) and torch.equal(la, ls), (la.item(), ls.item())
    for m in ma:
        assert torch.equal(ma[m], ms[m]), m
    for name in asym.p:
        twin = name if name in sym.p else name.replace("decoder_embeddings", "encoder_embeddings")     # depth's mod_emb: shared there
        assert torch.equal(asym.g[name], sym.g[twin]), name
    assert bool(asym.g["decoder_embeddings.tok_depth.mod_emb"].any())
    # tensors only the symmetric model owns saw no row
    for name in ("encoder_embeddings.tok_depth.token_emb.weight", "decoder_embeddings.tok_rgb.token_emb.weight"):
        assert not bool(sym.g[name].any()), name
    # a key in neither set is refused, a batch without a decoder modality too
    with pytest.raises(KeyError):
        asym.forward(dict(md, tok_gaze=md["tok_cam"]))
    with pytest.raises(ValueError):
        asym.forward({"tok_rgb": md["tok_rgb"]})


def test_unshared_modality_embeddings_split_the_shared_gradient():
    """(b) share_modality_embeddings=False with the decoder mod_emb copied from the encoder's: the forward adds the same numbers - the
    same loss - and the shared mod_emb gradient is the sum of the two unshared ones up to fp32 summation order."""
    sd = synth.build_state_dict(SYM, seed=4)
    sym, uns = _engine(SYM, sd), _engine(replace(SYM, share_modality_embeddings=False), sd)
    md, order = _batch(FULL), ["tok_cam", "tok_rgb", "tok_depth"]
    ls, ms = _step(sym, md, order)
    lu, mu = _step(uns, md, order)
    assert torch.equal(ls, lu) and all(torch.equal(ms[m], mu[m]) for m in ms)
    for m in SYM.modalities:
        e, d = uns.g[f"encoder_embeddings.{m}.mod_emb"], uns.g[f"decoder_embeddings.{m}.mod_emb"]
        assert bool(e.any()) and bool(d.any())
        held(f"asym.unshared_mod_emb_grad.{m}", rel_l2((e.double() + d.double()).cpu().numpy(), sym.g[f"encoder_embeddings.{m}.mod_emb"].cpu().numpy()),
             hard=FP32_TOL)
    for name in sym.p:
        if not name.endswith("mod_emb"):
            assert torch.equal(sym.g[name], uns.g[name]), name


@pytest.mark.parametrize("causal", [False, True])
def test_no_separation_with_one_decoder_modality_equals_separation(causal):
    """(c) with a single decoder modality in the batch the separation term masks nothing: decoder_sep_mask=False gives the same bits"""
    base = replace(SYM, decoder_causal_mask=causal)
    sd = synth.build_state_dict(base, seed=4)
    sep, nosep = _engine(base, sd), _engine(replace(base, decoder_sep_mask=False), sd)
    assert nosep._dec_groups() == {}
    md = _batch({"tok_rgb": [(100, 0), (120, 0)], "tok_depth": [(40, 130), (30, 90)], "tok_cam": [(12, 0), (15, 0)]})
    md = {k: v for k, v in md.items()}
    sub = {"tok_rgb": md["tok_rgb"], "tok_cam": md["tok_cam"], "tok_depth": md["tok_depth"]}
    order = ["tok_depth", "tok_rgb", "tok_cam"]                      # (rgb and cam hold no target: one non-empty decoder slot)
    l1, m1 = _step(sep, sub, order)
    l2, m2 = _step(nosep, sub, order)
    assert torch.isfinite(l1) and torch.equal(l1, l2) and torch.equal(m1["tok_depth"], m2["tok_depth"])
    assert torch.equal(sep.G, nosep.G)


def test_no_separation_changes_the_mask_with_several_decoder_modalities():
    """three decoder modalities: rows see the earlier modalities' keys too (the staircase) - another loss than under separation, finite,
    and every sample on the per-row path"""
    sd = synth.build_state_dict(SYM, seed=4)
    sep, nosep = _engine(SYM, sd), _engine(replace(SYM, decoder_sep_mask=False), sd)
    md, order = _batch(FULL), ["tok_cam", "tok_rgb", "tok_depth"]
    l1, _ = _step(sep, md, order)
    l2, _ = _step(nosep, md, order)
    assert torch.isfinite(l2) and not torch.equal(l1, l2)
    assert nosep.cd["seg_bad"][:2].tolist() == [1, 1] and int(nosep.cd["err"].item()) == 0
    ke = nosep.cd["ke"][:2].cpu().numpy()
    seg = nosep.cd["seg"].view(-1)[:2 * 3 * 2].view(2, 3, 2).cpu().numpy()
    for b in range(2):
        for s in range(3):
            s0, c = seg[b, s]
            assert (ke[b, s0:s0 + c] == s0 + c).all() and (nosep.cd["ks"][b, s0:s0 + c] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the module surface
def _module(enc, dec, **kw):
    from egom2p_amd.model import MODALITY_INFO, create_model
    return create_model("egom2p_tiny_6e_6d_swiglu_nobias", encoder_depth=2, decoder_depth=2,
                        encoder_embeddings={m: MODALITY_INFO[m]["encoder_embedding"]() for m in enc},
                        decoder_embeddings={m: MODALITY_INFO[m]["decoder_embedding"]() for m in dec},
                        modality_info={m: MODALITY_INFO[m] for m in set(enc) | set(dec)}, **kw)


def test_the_three_formerly_refused_models_build_and_train():
    """(raises NotImplementedError on the commit before) different modality sets, decoder_sep_mask=False and unshared modality
    embeddings through the constructor: the reference's parameter names, a finite loss, gradients where the reference has them"""
    md = _batch(FULL)
    for kw, enc, dec in ((dict(), ("tok_rgb", "tok_cam"), ("tok_depth", "tok_cam")),
                         (dict(decoder_sep_mask=False), ("tok_rgb", "tok_depth", "tok_cam"), ("tok_rgb", "tok_depth", "tok_cam")),
                         (dict(share_modality_embeddings=False), ("tok_rgb", "tok_cam"), ("tok_rgb", "tok_cam"))):
        torch.manual_seed(0)
        model = _module(enc, dec, **kw)
        names = {n for n, _ in model.named_parameters()}
        keys = set(model.state_dict())
        for m in dec:
            own = m not in enc or kw.get("share_modality_embeddings") is False
            assert (f"decoder_embeddings.{m}.mod_emb" in names) == own and f"decoder_embeddings.{m}.mod_emb" in keys
        assert not any(n.startswith("encoder_embeddings.") and n.split(".")[1] not in enc for n in keys)
        assert not any(n.startswith("decoder_embeddings.") and n.split(".")[1] not in dec for n in keys)
        loss, mod_loss = model({k: v for k, v in md.items() if k in set(enc) | set(dec)}, 128, 128, loss_type="mod")
        loss.backward()
        assert torch.isfinite(loss) and sorted(mod_loss) == sorted(dec)
        for n, p in model.named_parameters():
            if n.endswith("mod_emb"):
                assert p.grad is not None and bool(p.grad.any()), n
        with pytest.raises(KeyError):
            model(dict(md, tok_gaze=md["tok_cam"]), 128, 128)
    # freeze_params_except_specific_embeddings walks both sets (egom2p_model.py:748-811)
    model = _module(("tok_rgb", "tok_cam"), ("tok_depth", "tok_cam"))
    model.freeze_params_except_specific_embeddings("tok_depth")
    grads = {n: p.requires_grad for n, p in model.named_parameters()}
    assert not grads["decoder_embeddings.tok_depth.mod_emb"] and not grads["decoder_embeddings.tok_depth.token_emb.weight"]
    assert grads["encoder_embeddings.tok_rgb.token_emb.weight"] and not grads["encoder.0.attn.qkv.weight"]
    model.unfreeze_all()
    assert all(p.requires_grad for p in model.parameters())


def test_training_script_trains_an_asymmetric_model(tmp_path):
    """run_training_egom2p.py --in_domains tok_rgb-tok_cam --out_domains tok_depth-tok_cam: two AdamW steps with a finite loss, a
    checkpoint that reloads, and a second identical run that is bitwise equal"""
    spec = importlib.util.spec_from_file_location("run_training_egom2p_asym", os.path.join(ROOT, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    common = ["--model", "egom2p_tiny_6e_6d_swiglu_nobias", "--in_domains", "tok_rgb-tok_cam", "--out_domains", "tok_depth-tok_cam",
              "--num_input_tokens", "96", "--num_target_tokens", "96", "--batch_size", "2", "--epochs", "1", "--epoch_size", "4",
              "--blr", "1e-3", "--print_freq", "1", "--seed", "3", "--max_steps", "2"]
    cks = []
    for run in ("a", "b"):
        R.main(R.get_args(common + ["--output_dir", str(tmp_path / run)]))
        cks.append(torch.load(tmp_path / run / "checkpoint-0.pth", map_location="cpu", weights_only=True))
        log = open(tmp_path / run / "log.txt").read()
        assert np.isfinite(float(json.loads(log.splitlines()[-1])["loss"]))
    a, b = cks[0]["model"], cks[1]["model"]
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert "decoder_embeddings.tok_depth.mod_emb" in a and "encoder_embeddings.tok_depth.mod_emb" not in a
    args = R.get_args(common)
    model = R.get_model(args)
    model.load_state_dict(a, strict=True)
    back = model.state_dict()
    assert all(torch.equal(back[k].cpu(), a[k]) for k in a)
    # the weights moved: both embeddings of the asymmetric pair trained
    fresh = R.get_model(args).state_dict()
    assert not torch.equal(fresh["decoder_embeddings.tok_depth.mod_emb"].cpu(), a["decoder_embeddings.tok_depth.mod_emb"])


# ------------------------------------------------------------------------------------------------ 4. generation: an rgb -> depth specialist
def test_rgb_to_depth_specialist_generates_eager_graphed_and_whole_schedule():
    """encoder {rgb}, decoder {depth}: 3 ROAR steps + one MaskGIT step; the decoded depth tokens never re-enter the encoder (it has no
    depth embedding, generate.py:749-751) - the same tokens from generate, use_graphs=True and generate_graphed for one seed"""
    from egom2p_amd.generate import GenerationSampler, build_chained_generation_schedules, init_empty_target_modality, init_full_input_modality
    from egom2p_amd.model import MODALITY_INFO
    cfg = ModelCfg("rgb2depth", 384, 2, 2, 6, modalities=("tok_rgb", "tok_depth"), encoder_modalities=("tok_rgb",),
                   decoder_modalities=("tok_depth",))
    eng = Engine(cfg, DEV, max_batch=2, n_enc=64, n_dec=64)
    eng.init_random(3)
    B, n_open, known = 2, 128, 5120 - 128

    def kw(scheme, steps, tokens):
        return build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [tokens], [scheme], [steps], ["linear"], [1.0], ["constant"],
                                                  [2.0], ["constant"], cfg_grow_conditioning=True)
    sch = kw("roar", 3, 96) + kw("maskgit", 1, 32)
    assert [s["scheme"] for s in sch] == ["roar"] * 3 + ["maskgit"] and sum(s["num_tokens"] for s in sch) == n_open
    sample = {"tok_rgb": {"tensor": synth.randint("spec.rgb", (B, 5, 32, 32), 64000, seed=2).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", B, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    sample["tok_rgb"]["input_mask"][:, 600:] = True                      # 600 rgb tokens condition the pass
    d = sample["tok_depth"]
    d["tensor"][:, :known] = synth.randint("spec.depth", (B, known), 64000, seed=2).to(DEV)
    d["input_mask"][:, :known] = False
    d["target_mask"][:, :known] = True
    outs = [GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=9),
            GenerationSampler(eng, use_graphs=True).generate(sample, sch, top_p=0.8, seed=9),
            GenerationSampler(eng).generate_graphed(sample, sch, top_p=0.8, seed=9)]
    t = outs[0]["tok_depth"]["tensor"]
    assert outs[0]["tok_depth"]["target_mask"].all() and int(t.min()) >= 0 and int(t.max()) < 64000
    assert torch.equal(t[:, :known], d["tensor"][:, :known])
    for o in outs[1:]:
        assert torch.equal(o["tok_depth"]["tensor"], t)
    # the target must be a decoder modality, an encoder pass takes encoder modalities only
    pos = torch.zeros(B, 4, dtype=torch.int64, device=DEV)
    ids, msk = sample["tok_rgb"]["tensor"].reshape(B, -1), sample["tok_rgb"]["input_mask"]
    with pytest.raises(KeyError):
        eng.infer_logits({"tok_rgb": (ids, msk)}, 600, "tok_rgb", pos)
    with pytest.raises(KeyError):
        eng.infer_logits({"tok_depth": (ids, msk)}, 600, "tok_depth", pos)


# ------------------------------------------------------------------------------------------------ 5. device masking under zero alphas
def test_device_masking_gives_a_zero_alpha_modality_no_tokens():
    """4096 draws of the device sampler with one zero input alpha (depth) and one zero target alpha (rgb): that modality's budget is 0 on
    that side in every draw - the zero pattern of the reference's own sampler on the same dataset, recorded in
    tests/golden/zero_alpha_budgets.npz and asserted of it in tests/test_asym_layout_cpu.py.  The other invariants of the device
    masking hold - budgets stay inside the token counts and the modalities, inputs and targets are disjoint and the
    decoder_attention_mask carries the target count on the targets."""
    from egom2p_amd.masking import UnifiedMasking, sampling_mod_info
    from egom2p_amd.model import MODALITY_INFO
    info = sampling_mod_info(["tok_rgb", "tok_cam"], ["tok_depth", "tok_cam"], MODALITY_INFO)
    um = UnifiedMasking(info, None, 256, 256, seed=5, device=DEV)
    names = um.names
    assert names == ["tok_rgb", "tok_cam", "tok_depth"]
    n_in, n_tg = {n: [] for n in names}, {n: [] for n in names}
    B = 512
    for call in range(8):
        toks = {n: torch.zeros(B, MODALITIES[n].max_tokens, dtype=torch.int64, device=DEV) for n in names}
        out = um(toks)
        for n in names:
            o = out[n]
            inp, tgt = ~o["input_mask"], ~o["target_mask"]
            assert not bool((inp & tgt).any())
            n_in[n].append(inp.sum(1)); n_tg[n].append(tgt.sum(1))
            dam = o["decoder_attention_mask"]
            assert torch.equal(dam.sum(1), tgt.sum(1).to(dam.dtype)) and not bool((dam != 0)[~tgt].any())
    n_in = {n: torch.cat(v).cpu().numpy() for n, v in n_in.items()}
    n_tg = {n: torch.cat(v).cpu().numpy() for n, v in n_tg.items()}
    assert len(n_in["tok_rgb"]) == 4096
    assert (n_in["tok_depth"] == 0).all() and (n_tg["tok_rgb"] == 0).all()
    # ... exactly the sides the reference's sampler leaves empty on this dataset (and no other)
    g = np.load(os.path.join(ROOT, "tests", "golden", "zero_alpha_budgets.npz"), allow_pickle=False)
    for j, n in enumerate(str(x) for x in g["names"]):
        assert bool((g["k_in"][j] == 0).all()) == bool((n_in[n] == 0).all()) and bool((g["k_tgt"][j] == 0).all()) == bool((n_tg[n] == 0).all()), n
    # cam holds 30 positions: what a draw gives it beyond them is cut (masking.py:199, 228), so the sums are bounded, not fixed
    tot_in, tot_tg = sum(n_in.values()), sum(n_tg.values())
    assert (tot_in <= 256).all() and (tot_in >= 256 - 226).all() and (tot_tg <= 256).all()
    assert (n_in["tok_rgb"] + n_in["tok_cam"] == tot_in).all() and (n_in["tok_cam"] + n_tg["tok_cam"] <= 30).all()
    assert n_in["tok_rgb"].max() > 200 and n_in["tok_cam"].max() > 0 and n_tg["tok_depth"].max() > 200 and n_tg["tok_cam"].max() > 0
