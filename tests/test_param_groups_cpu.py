"""Host side of parameter-group AdamW (layer-wise lr decay): the groups against the reference's own `get_parameter_groups` /
`get_num_layer_for_fm` (tests/golden/param_groups.json, tools/make_goldens_param_groups.py), the layer numbering's quirk, the
segment construction of the one-launch step on hand-made flat layouts, and the default optimiser left as it was."""
import json
import os
import re
from functools import partial

import pytest
import torch

from egom2p_amd import _lib as L
from egom2p_amd import ops
from egom2p_amd import optim as O
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "param_groups.json")))
MODS = ("tok_cam", "tok_gaze")
CASES = [(c, v) for c in sorted(GOLD) for v in sorted(GOLD[c]["variants"])]


def tiny_model(gelu=False, device="cpu", **kw):
    """The fixture's geometry: dim 128, 2 + 2 layers, 2 heads, tok_cam + tok_gaze (parameters only: no kernel runs on the CPU)."""
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}
    norm = partial(torch.nn.LayerNorm, eps=1e-6) if gelu else partial(LayerNorm, eps=1e-6, bias=False)
    return EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in MODS}, dim=128, encoder_depth=2, decoder_depth=2, num_heads=2,
                  qkv_bias=gelu, proj_bias=gelu, mlp_bias=gelu, norm_layer=norm, act_layer=torch.nn.GELU if gelu else torch.nn.SiLU,
                  gated_mlp=not gelu, device=device, **kw)


def groups_for(model, args):
    layer_fn = partial(O.get_num_layer_for_fm, num_enc_layers=2, num_dec_layers=2)
    scale_fn = O.LayerDecayValueAssigner(O.layer_decay_values(args["layer_decay"], 4)).get_scale
    return O.get_parameter_groups(model, 0.05, (), layer_fn, scale_fn, args["decoder_decay"], (), args["no_lr_scale_list"].split("-"))


@pytest.mark.parametrize("cname,vname", CASES)
def test_groups_equal_the_reference(cname, vname):
    entry = GOLD[cname]
    model = tiny_model(**entry["model"])
    names = {n for n, _ in model.named_parameters()}
    want = entry["variants"][vname]["params"]
    assert names == set(want) | set(entry["frozen"])               # the same tensors under the same names, nothing left out
    for n, p in model.named_parameters():
        if n in entry["frozen"]:
            p.requires_grad = False
    got = {}
    for g in groups_for(model, entry["variants"][vname]["args"]):
        assert len(g["params"]) == len(g["param_names"])
        for n in g["param_names"]:
            assert n not in got
            got[n] = [g["name"], g["lr_scale"], g["weight_decay"]]
    assert set(got) == set(want)
    for n in want:
        assert got[n][0] == want[n][0] and got[n][1] == want[n][1] and got[n][2] == want[n][2], (n, got[n], want[n])


def test_layer_numbering_keeps_the_reference_quirk():
    f = partial(O.get_num_layer_for_fm, num_enc_layers=2, num_dec_layers=2)
    # the reference compares whole names with ("encoder_norm", "decoder_proj_context", "mask_token"): only the bare name matches
    assert f("mask_token") == 2
    assert f("encoder_norm.weight") == f("decoder_proj_context.weight") == f("decoder_proj_context.bias") == 5
    assert f("encoder_embeddings.tok_cam.token_emb.weight") == 0 and f("encoder.1.mlp.fc1.weight") == 2
    assert f("decoder_embeddings.tok_cam.mod_emb") == 2 and f("decoder.0.norm1.weight") == 3 and f("decoder.1.mlp.fc2.weight") == 4
    assert f("decoder_embeddings.tok_cam.token_emb.weight") == f("decoder_norm.weight") == f("register_tokens") == 5
    assert O.get_num_layer_for_fm("decoder_embeddings.tok_cam.mod_emb", 2, 2, last_layer_mod_emb=True) == 5
    gold = GOLD["swiglu_nobias"]["variants"]["ld"]["params"]
    for n in ("encoder_norm.weight", "decoder_proj_context.weight", "decoder_proj_context.bias"):
        assert gold[n][0].startswith("layer_5_") and gold[n][1] == 1.0
    assert O.layer_decay_values(0.75, 4) == [0.75 ** (5 - i) for i in range(6)]


def _offsets(sizes):
    offs, o = {}, 0
    for name, n in sizes:
        offs[name] = (o, n, (n,))
        o += (n + 3) // 4 * 4
    return offs, o


def _check_segments(segs, offs, never):
    prev = 0
    for lo, hi, grp, sk, fro in segs:
        assert lo >= prev and hi > lo and lo % 4 == 0 and hi % 4 == 0
        prev = hi
    covered = sorted((lo, hi) for lo, hi, *_ in segs)
    want = sorted((o, o + (n + 3) // 4 * 4) for k, (o, n, _) in offs.items() if k not in never)
    flat = lambda rs: [x for lo, hi in rs for x in range(lo, hi, 4)]
    assert flat(covered) == flat(want)                             # exactly the tensors that can have a gradient


def test_segments_on_a_hand_made_layout():
    offs, total = _offsets([("a", 10), ("b", 4), ("c", 4096), ("never", 7), ("d", 5000), ("e", 3), ("f", 8), ("g", 8), ("h", 12)])
    group_of = {"a": 0, "b": 0, "c": 1, "d": 1, "e": 1, "f": 2, "g": 2, "h": 2, "never": 3}
    segs = O.build_segments(offs, {"never"}, group_of, {"e": 2}, {"g"})
    _check_segments(segs, offs, {"never"})
    keys = [(grp, sk, fro) for _, _, grp, sk, fro in segs]
    # a | b merge (same group); c stands alone (the never_grad gap behind it); d and e differ in step offset; g is frozen between f and h
    assert keys == [(0, 0, False), (1, 0, False), (1, 0, False), (1, 2, False), (2, 0, False), (0, 0, True), (2, 0, False)]
    assert segs[0][:2] == (0, 16) and segs[1][:2] == (16, 16 + 4096) and segs[2][0] == 16 + 4096 + 8
    for x, y in zip(segs, segs[1:]):
        assert x[1] != y[0] or x[2:] != y[2:]                      # whatever touches and agrees was merged
    # a tensor in no group (requires_grad=False when the groups were built) is a frozen segment for good
    segs2 = O.build_segments(offs, {"never"}, {k: v for k, v in group_of.items() if k != "c"}, {}, set())
    assert [s for s in segs2 if s[4]] == [(16, 16 + 4096, 0, 0, True)]
    (rows, slots), = O.plan_launches(segs)
    assert slots == [(0, 0), (1, 0), (1, 2), (2, 0)] and [r[2] for r in rows] == [0, 1, 1, 2, 3, 0, 3] and [r[3] for r in rows] == [0, 0, 0, 0, 0, 1, 0]
    first, n_chunks = ops.seg_chunks(rows)
    assert first[0] == 0 and n_chunks == sum(-(-(hi - lo) // L.ADAMW_CHUNK) for lo, hi, _, _ in rows)
    for s in range(len(rows) - 1):
        assert first[s + 1] - first[s] == -(-(rows[s][1] - rows[s][0]) // L.ADAMW_CHUNK) >= 1
    assert [first[s + 1] - first[s] for s in (0, 1, 2)] == [1, 1, 2]      # 16, 4096 and 5000 floats


def test_129_combinations_take_two_launches():
    offs, _ = _offsets([(f"t{i}", 8) for i in range(129)])
    segs = O.build_segments(offs, set(), {f"t{i}": i for i in range(129)}, {}, set())
    assert len(segs) == 129
    launches = O.plan_launches(segs, L.ADAMW_MAX_GROUPS)
    assert [len(rows) for rows, _ in launches] == [128, 1] and [len(slots) for _, slots in launches] == [128, 1]
    assert launches[1][0] == [(128 * 8, 129 * 8, 0, 0)] and launches[1][1] == [(128, 0)]
    assert all(0 <= r[2] < L.ADAMW_MAX_GROUPS for rows, _ in launches for r in rows)
    # the same group under two step offsets is two combinations
    segs = O.build_segments(offs, set(), {f"t{i}": 0 for i in range(129)}, {f"t{i}": i % 2 for i in range(129)}, set())
    (rows, slots), = O.plan_launches(segs)
    assert slots == [(0, 0), (0, 1)] and len(rows) == 129


def test_engine_segments_of_the_tiny_model():
    model = tiny_model()
    eng = model.engine
    opt = O.FusedAdamW(eng, named_parameters=model.named_parameters(),
                       param_groups=groups_for(model, GOLD["swiglu_nobias"]["variants"]["ld"]["args"]))
    assert opt.segmented and len(opt.param_groups) == 11
    segs = opt.segments()
    _check_segments(segs, eng.offsets, eng.never_grad)
    assert not any(s[4] for s in segs) and segs[0][0] == 0 and segs[-1][1] == eng.n_flat
    model.freeze_encoder()
    segs = opt.segments()
    _check_segments(segs, eng.offsets, eng.never_grad)
    frozen = [s for s in segs if s[4]]
    assert frozen and sum(hi - lo for lo, hi, *_ in frozen) == sum((n + 3) // 4 * 4 for k, (o, n, _) in eng.offsets.items()
                                                                     if k.startswith(("encoder.", "encoder_norm", "encoder_embeddings")))
    with pytest.raises(ValueError):
        O.FusedAdamW(eng, named_parameters=model.named_parameters(), param_groups=[{"params": [torch.nn.Parameter(torch.zeros(4))],
                                                                                   "param_names": ["no.such.tensor"]}])


def test_create_optimizer_called_as_before_builds_the_two_groups():
    model = tiny_model()
    args = type("A", (), {"opt": "adamw", "lr": 1e-3, "weight_decay": 0.05, "opt_betas": (0.9, 0.95), "opt_eps": None})()
    opt = O.create_optimizer(args, model)
    assert not opt.segmented and [g["name"] for g in opt.param_groups] == ["decay", "no_decay"]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.05, 0.0] and all(g["lr_scale"] == 1.0 for g in opt.param_groups)
    assert len(opt.param_groups[0]["params"]) + len(opt.param_groups[1]["params"]) == len(list(model.named_parameters()))
    same = O.create_optimizer(args, model, get_num_layer=None, get_layer_scale=None, filter_bias_and_bn=True, skip_list=None)
    assert not same.segmented and [g["name"] for g in same.param_groups] == ["decay", "no_decay"]
    # the reference's signature: the layer functions give one group per (layer, weight-decay class), args carry the rest
    layer_fn = partial(O.get_num_layer_for_fm, num_enc_layers=2, num_dec_layers=2)
    args.decoder_decay, args.no_lr_scale_list = 0.01, "encoder.0.attn.qkv.weight-decoder_norm.weight"
    ld = O.create_optimizer(args, model, get_num_layer=layer_fn, get_layer_scale=O.LayerDecayValueAssigner(O.layer_decay_values(0.75, 4)).get_scale)
    want = GOLD["swiglu_nobias"]["variants"]["ld_dd"]["params"]
    assert ld.segmented and {g["name"] for g in ld.param_groups} == {v[0] for v in want.values()}
    assert [g["name"] for g in ld.state_dict()["param_groups"]] == [g["name"] for g in ld.param_groups]
    sd = ld.state_dict()
    with pytest.raises(RuntimeError, match="parameter groups"):
        opt.load_state_dict(sd)
    args.weight_decay = 0.0
    with pytest.raises(ValueError):
        O.create_optimizer(args, model, get_num_layer=layer_fn)


def test_new_symbol_is_declared_bound_and_exported():
    """The extension header (include/egom2p_hip_optim.h), its binding table and the library's dynamic symbols agree - what
    tests/test_cabi_exports.py holds for the core header - and the core header includes the extension."""
    import subprocess
    core = open(os.path.join(ROOT, "include", "egom2p_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "egom2p_hip_optim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s+(ego_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(L.EXPORTS_OPTIM) == {"ego_adamw_step_seg"} and not declared & set(L.EXPORTS)
    assert '#include "egom2p_hip_optim.h"' in core
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert declared <= set(re.findall(r" T (ego_\w+)", out))
    assert "optim_factory.py:97-154, 226" in hdr and "run_training_egom2p.py:707-713" in hdr
    for name, val in (("EGO_ADAMW_MAX_GROUPS", L.ADAMW_MAX_GROUPS), ("EGO_ADAMW_CHUNK", L.ADAMW_CHUNK), ("EGO_SEG_FROZEN", L.SEG_FROZEN)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
    import ctypes as C
    assert C.sizeof(L.AdamwSeg) == 24 and C.sizeof(L.AdamwHp) == 5 * 4 * L.ADAMW_MAX_GROUPS + 4
    assert hasattr(L.load(), "ego_adamw_step_seg") and callable(ops.adamw_step_seg)


def test_entry_script_switches_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_training_layer_decay", os.path.join(ROOT, "run_training_egom2p.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    a = rt.get_args([])
    assert a.layer_decay is None and a.decoder_decay is None and a.no_lr_scale_list == "" and a.finetune == ""
    a = rt.get_args(["--layer_decay", "0.75", "--decoder_decay", "0.01", "--no_lr_scale_list", "a-b", "--finetune", "x.pth"])
    assert (a.layer_decay, a.decoder_decay, a.no_lr_scale_list, a.finetune) == (0.75, 0.01, "a-b", "x.pth")
    with pytest.raises(ValueError, match="local"):
        rt.load_finetune("https://example.org/weights.pth", None)
