"""MaskGIT generation on the GPU: the two device kernels (`ego_maskgit_positions`, `ego_maskgit_select`) against torch, the
sampler's reported probability against torch, `GenerationSampler.maskgit_step` against fixtures made by the REAL reference
(tests/golden/maskgit_rgb2cam.npz, maskgit_rgb2depth.npz: tools/make_goldens_maskgit.py), and whole schedules eager / graphed."""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR, rel_l2  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.generate import (GenerationSampler, build_chained_generation_schedules, init_empty_target_modality,  # noqa: E402
                                 init_full_input_modality)
from egom2p_amd.model import MODALITY_INFO  # noqa: E402

DEV = "cuda"


def _fixture(name):
    """a missing fixture FAILS (conftest.load_golden would skip)"""
    path = os.path.join(GOLDEN_DIR, f"{name}.npz")
    assert os.path.exists(path), f"tests/golden/{name}.npz is missing (tools/make_goldens_maskgit.py)"
    g = np.load(path, allow_pickle=False)
    return g, ast.literal_eval(str(g["meta"]))


# ------------------------------------------------------------------------------------------------------------ 1. positions
def _ref_positions(mask, M):
    T = mask.shape[1]
    return torch.argsort(mask + torch.arange(T, device=mask.device).unsqueeze(0) * 1e-6, dim=1)[:, :M]      # generate.py:463-467


@pytest.mark.parametrize("T", [30, 37, 5120])
def test_positions_equal_the_argsort_formula(T):
    g = torch.Generator().manual_seed(T)
    n0 = T // 2 + 1                                           # open positions of row 0 (sets M); row 1 has fewer, row 2 more
    mask = torch.ones(3, T, dtype=torch.bool)
    for b, n in enumerate((n0, n0 - 3, min(T, n0 + 5))):
        mask[b, torch.randperm(T, generator=g)[:n]] = False
    mask = mask.to(DEV)
    for M in (0, 1, n0):
        got = ops.maskgit_positions(mask, M)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, M)
        assert torch.equal(got, _ref_positions(mask, M)), (T, M)
    # every position, all open, all closed
    assert torch.equal(ops.maskgit_positions(mask, T), _ref_positions(mask, T))
    for m in (torch.zeros_like(mask), torch.ones_like(mask)):
        assert torch.equal(ops.maskgit_positions(m, T), torch.arange(T, device=DEV).expand(3, T))
    with pytest.raises(L.EgoHipError):
        ops.maskgit_positions(mask, T + 1)


# ------------------------------------------------------------------------------------------------------------ 2./3. select
def _select_case(probs, K, seed):
    """random tokens / distinct positions / random initial state for `probs` [B, M]; runs the kernel; returns everything"""
    B, M = probs.shape
    T = M + 7
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, 64000, (B, M), generator=g, dtype=torch.int32).to(DEV)
    pos = torch.stack([torch.randperm(T, generator=g)[:M] for _ in range(B)]).to(DEV)
    tensor0 = torch.randint(0, 64000, (B, T), generator=g).to(DEV)
    im0 = (torch.rand(B, T, generator=g) < 0.5).to(DEV)
    tm0 = (torch.rand(B, T, generator=g) < 0.5).to(DEV)
    tensor, im, tm = tensor0.clone(), im0.clone(), tm0.clone()
    Kc = min(K, M)
    idx = torch.full((B, Kc), -1, device=DEV, dtype=torch.int64)
    ops.maskgit_select(tokens, probs, pos, K, tensor, im, tm, out_idx=idx)
    return dict(tokens=tokens, pos=pos, init=(tensor0, im0, tm0), out=(tensor, im, tm), idx=idx, Kc=Kc)


def _check_against(c, chosen):
    """the kernel's state equals torch.scatter's over the rows `chosen` [B, Kc] (any order); every other element is untouched"""
    top_pos = torch.gather(c["pos"], -1, chosen)
    top_tok = torch.gather(c["tokens"].long(), -1, chosen)
    t0, i0, m0 = c["init"]
    assert torch.equal(c["out"][0], torch.scatter(t0, -1, top_pos, top_tok))
    assert torch.equal(c["out"][1], torch.scatter(i0, -1, top_pos, torch.zeros_like(top_tok, dtype=torch.bool)))
    assert torch.equal(c["out"][2], torch.scatter(m0, -1, top_pos, torch.ones_like(top_tok, dtype=torch.bool)))
    assert torch.equal(c["idx"], torch.sort(chosen, -1).values)                  # the chosen rows, ascending


@pytest.mark.parametrize("M", [1, 30, 1000, 5120, 8192])
def test_select_distinct_probabilities_equal_topk(M):
    B = 4
    g = torch.Generator().manual_seed(M)
    # a scaled random permutation: ties are impossible by construction
    probs = torch.stack([(torch.randperm(M, generator=g) + 1).float() / (M + 1) for _ in range(B)]).to(DEV)
    for K in sorted({1, M // 3, M - 1, M, M + 5}):
        c = _select_case(probs, K, seed=K)
        if c["Kc"] == 0:                                                          # nothing to commit: nothing is touched
            assert all(torch.equal(a, b) for a, b in zip(c["init"], c["out"]))
            continue
        _check_against(c, torch.topk(probs, c["Kc"], dim=-1)[1])


def test_select_refuses_more_than_8192_rows():
    probs = torch.rand(1, 8193, device=DEV)
    with pytest.raises(L.EgoHipError, match="bad arguments"):
        _select_case(probs, 5, seed=0)


@pytest.mark.parametrize("M", [37, 5120])
@pytest.mark.parametrize("case", ["all_one", "block", "zeros"])
def test_select_ties_go_to_the_lower_rows_and_are_reproducible(case, M):
    """the tie rule (include/egom2p_hip.h): strictly larger first, equal ones in ascending decoder-row order = a
    STABLE descending sort"""
    B = 3
    g = torch.Generator().manual_seed(M)
    if case == "all_one":                                     # temperature 0: every probability is 1
        probs, K = torch.ones(B, M), M // 3
    elif case == "block":                                     # a block of equal values straddles the K-th place
        probs = torch.stack([(torch.randperm(M, generator=g) + 1).float() / (M + 1) for _ in range(B)])
        K = M // 2
        srt = torch.sort(probs, -1, descending=True).values
        lo, hi = srt[:, K + M // 5], srt[:, K - M // 5]
        probs = torch.where((probs >= lo[:, None]) & (probs <= hi[:, None]), hi[:, None].expand(B, M), probs)
    else:                                                     # zeros present, K larger than the number of positive values
        probs = torch.rand(B, M, generator=g)
        probs[torch.rand(B, M, generator=g) < 0.7] = 0.0
        K = int((probs > 0).sum(-1).max()) + 3
        assert K < M
    probs = probs.to(DEV)
    want = torch.sort(probs, dim=-1, descending=True, stable=True).indices[:, :K]
    a = _select_case(probs, K, seed=1)
    _check_against(a, want)
    b = _select_case(probs, K, seed=1)                        # a second launch: identical bits
    assert torch.equal(a["idx"], b["idx"]) and all(torch.equal(x, y) for x, y in zip(a["out"], b["out"]))


# ------------------------------------------------------------------------------------------------------------ 4. sampler probability
def _ref_filter(logits, top_p):
    """the reference's top_k_top_p_filtering (generate.py:348-357) restated with torch ops"""
    sl, si = torch.sort(logits, dim=1, descending=True)
    cp = torch.cumsum(torch.softmax(sl, -1), -1)
    rm = cp > top_p
    rm[:, 1:] = rm[:, :-1].clone()
    rm[:, 0] = False
    return torch.gather(rm, -1, torch.argsort(si, -1))


def test_sampler_reports_the_probability_of_the_sampled_token():
    """`out_prob` of ego_sample_cfg_topp (what MaskGIT ranks by) against `softmax(filtered mixed / T)[token]` (generate.py:367-370)
    in fp32 torch.  The kernel uses __expf and its own summation order, and its nucleus can differ from torch's by the tokens AT the
    cut: logits that tie there are kept or dropped together (csrc/sample.hip; 2c - u of bf16 logits lies on a coarse grid: ties are
    common), and torch's fp32 cumsum over 64000 sorted tokens decides a token within rounding of top_p either way.  Such a token
    moves the normaliser by its share of the kept mass - these rows' logits have a standard deviation of 6.7, a few dozen tokens
    carry the nucleus - which is what the largest difference shows; the other rows agree to fp32 rounding (printed).
    Measured on MI355X (first run, this seed): largest relative difference 1.55e-02, in the ONE row of 64 that differs by more than
    1e-5 (median 0.0); the bounds are 2x the two figures, so that a shift of every row does not hide behind the outlier."""
    torch.manual_seed(0)
    rows, V, s, top_p, temp = 64, 64000, 2.0, 0.8, 1.0
    cond = (torch.randn(rows, V, device=DEV) * 3).bfloat16()
    unc = (torch.randn(rows, V, device=DEV) * 3).bfloat16()
    mixed = unc.float() + (cond.float() - unc.float()) * s
    removed = _ref_filter(mixed.clone(), top_p)
    p = torch.softmax(mixed.masked_fill(removed, float("-inf")) / temp, -1)
    tok = torch.empty(rows, device=DEV, dtype=torch.int32)
    prob = torch.empty(rows, device=DEV)
    ops.sample_cfg_topp(cond, unc, V, s, top_p, temp, torch.rand(rows, device=DEV), tok, prob, ld=V)
    want = p.gather(1, tok.long()[:, None])[:, 0]
    assert bool((want > 0).all())                             # every sample lies inside the reference's nucleus
    rels = (prob - want).abs() / want
    rel = rels.max().item()
    print("sampler out_prob vs torch, largest relative difference:", rel, "median:", rels.median().item(),
          "rows above 1e-5:", int((rels > 1e-5).sum()), "of", rows)
    assert rel < 2 * 1.55e-02, rel
    assert int((rels > 1e-5).sum()) <= 2 * 1, rels


# ------------------------------------------------------------------------------------------------------------ 5. reference parity
@pytest.mark.parametrize("fixture", ["maskgit_rgb2cam", "maskgit_rgb2depth"])
def test_maskgit_cfg_generation_matches_reference(fixture):
    """Per step of the reference's guided MaskGIT run: our decoder row order equals its `mod_pos` bit for bit; the conditional /
    unconditional logits are held to the flat-head bars of test_roar_cfg_generation_matches_reference (the same pass over a
    different row set); with the reference's tokens and probabilities forced, the committed rows are its `top_indices` and the
    state after the step is its state."""
    g, meta = _fixture(fixture)
    cfg = MODEL_CFGS[meta["cfg"]]
    cond, target, B = meta["cond"], meta["target"], int(meta["batch"])
    eng = Engine(cfg, "cuda:0", max_batch=B, n_enc=64, n_dec=64)
    eng.load_state_dict(synth.build_state_dict(cfg, meta["seed"]))
    sampler = GenerationSampler(eng)
    md = {cond: {"tensor": torch.from_numpy(g["rgb_ids"].astype(np.int64)).to(DEV)}}
    md = init_empty_target_modality(md, MODALITY_INFO, target, B, int(meta["tokens"]), DEV)
    md = init_full_input_modality(md, MODALITY_INFO, cond, DEV)
    known = int(meta["known"])                               # target tokens given from the start: the rgb ids stand in (the fixture's note)
    init = np.zeros((B, int(meta["tokens"])), dtype=np.int64)
    init[:, :known] = g["rgb_ids"].reshape(B, -1)[:, :known]
    md[target] = {"tensor": torch.from_numpy(init).to(DEV),
                  "input_mask": torch.from_numpy(g["init.input_mask"]).to(DEV), "target_mask": torch.from_numpy(g["init.target_mask"]).to(DEV)}
    assert int(g["n_steps"]) == meta["steps"] == 3
    for step in range(int(g["n_steps"])):
        num_select, temp, cfg_scale = g[f"s{step}.cfg"]
        ref_pos = torch.from_numpy(g[f"s{step}.mod_pos"].astype(np.int64)).to(DEV)
        M = ref_pos.shape[1]
        assert torch.equal(ops.maskgit_positions(md[target]["target_mask"], M), ref_pos), step
        md, info = sampler.maskgit_step(md, target, int(num_select), float(temp), 0.0, meta["top_p"], conditioning=[cond],
                                        guidance_scale=float(cfg_scale), seed=step, return_logits=True,
                                        forced_samples=torch.from_numpy(g[f"s{step}.samples"].astype(np.int64)),
                                        forced_probs=torch.from_numpy(g[f"s{step}.probs"]))
        assert torch.equal(info["mod_pos"], ref_pos), step
        for nm, lg in (("cond", info["logits_cond"]), ("uncond", info["logits_uncond"])):
            lg = lg.float()
            assert tuple(lg.shape[:2]) == (B, M)
            assert rel_l2(lg[:, :6, :48].cpu().numpy(), g[f"s{step}.{nm}.head"]) < 3e-2, (step, nm)
            assert rel_l2(lg.norm(dim=-1).cpu().numpy(), g[f"s{step}.{nm}.rownorm"]) < 1e-2, (step, nm)
            lse_scale = max(1.0, float(np.abs(g[f"s{step}.{nm}.max"]).max()))
            assert np.abs(torch.logsumexp(lg, -1).cpu().numpy() - g[f"s{step}.{nm}.lse"]).max() < 5e-2 * lse_scale, (step, nm)
            am = (lg.argmax(-1).cpu().numpy() == g[f"s{step}.{nm}.argmax"]).mean()
            print(fixture, "step", step, nm, "arg-max agreement", round(float(am), 4))
            assert am > 0.9, (step, nm, am)
        # the kernel's own draws are tokens of the vocabulary with a probability in (0, 1]
        assert int(info["samples"].min()) >= 0 and int(info["samples"].max()) < 64000
        assert bool((info["probs"] > 0).all()) and bool((info["probs"] <= 1).all())
        want = np.sort(g[f"s{step}.top_indices"].astype(np.int64), -1)
        assert np.array_equal(info["top_indices"].cpu().numpy(), want), step
        state = md[target]["tensor"].cpu().numpy()
        assert np.array_equal(state[:, :known], init[:, :known]) and np.array_equal(state[:, known:].astype(np.int32), g[f"s{step}.tensor"]), step
        assert np.array_equal(md[target]["input_mask"].cpu().numpy(), g[f"s{step}.input_mask"]), step
        assert np.array_equal(md[target]["target_mask"].cpu().numpy(), g[f"s{step}.target_mask"]), step
    assert np.array_equal(md[target]["tensor"].cpu().numpy().astype(np.int32), g["final_tokens"])
    assert md[target]["target_mask"].all() and not md[target]["input_mask"].any()


# ------------------------------------------------------------------------------------------------------------ 6. end to end
N_KNOWN, N_OPEN = 3072, 2048


def _depth_sample(B, tag, seed, known=N_KNOWN):
    """rgb clip -> depth with the first `known` depth tokens given"""
    sample = {"tok_rgb": {"tensor": synth.randint(f"{tag}.rgb", (B, 5, 32, 32), 64000, seed=seed).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", B, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    d = sample["tok_depth"]
    d["tensor"][:, :known] = synth.randint(f"{tag}.depth", (B, known), 64000, seed=seed).to(DEV)
    d["input_mask"][:, :known] = False
    d["target_mask"][:, :known] = True
    return sample


def _depth_schedule(scheme="maskgit"):
    return build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [N_OPEN], [scheme], [3], ["cosine"], [1.0], ["constant"],
                                              [2.0], ["constant"], cfg_grow_conditioning=True)


@pytest.fixture(scope="module")
def eng384():
    eng = Engine(MODEL_CFGS["ego_gen_384_2e_2d"], "cuda:0", max_batch=2, n_enc=64, n_dec=64)
    eng.init_random(3)
    return eng


def test_maskgit_end_to_end_eager_and_graphed(eng384):
    eng = eng384
    sch = _depth_schedule()
    assert [s["num_tokens"] for s in sch] == [512, 1024, 512] and all(s["scheme"] == "maskgit" for s in sch)
    eager, graphed = GenerationSampler(eng, use_graphs=False), GenerationSampler(eng)
    for trial in range(2):                                    # the first graphed call captures, the second replays on new inputs
        sample = _depth_sample(2, f"mg{trial}", seed=trial)
        before = {k: v.clone() for k, v in sample["tok_depth"].items()}
        # step by step, as generate() seeds them: the filled count follows the schedule
        md = {k: dict(v) for k, v in sample.items()}
        filled = N_KNOWN
        for step, s in enumerate(sch):
            md = eager.maskgit_step(md, "tok_depth", s["num_tokens"], s["temperature"], 0.0, 0.8, conditioning=s["cfg_cond_domains"],
                                    guidance_scale=s["cfg_scale"], seed=20 + trial + step)
            filled += s["num_tokens"]
            assert md["tok_depth"]["target_mask"].sum(1).tolist() == [filled, filled]
            assert torch.equal(md["tok_depth"]["target_mask"], ~md["tok_depth"]["input_mask"])
        a = eager.generate(sample, sch, top_p=0.8, seed=20 + trial)
        t = a["tok_depth"]["tensor"]
        assert torch.equal(t, md["tok_depth"]["tensor"])
        assert t.shape == (2, 5120) and int(t.min()) >= 0 and int(t.max()) < 64000
        assert a["tok_depth"]["target_mask"].all() and not a["tok_depth"]["input_mask"].any()
        assert torch.equal(t[:, :N_KNOWN], before["tensor"][:, :N_KNOWN])                     # known tokens stay
        assert all(torch.equal(sample["tok_depth"][k], before[k]) for k in before)            # the caller's dict is untouched
        b = graphed.generate_graphed(sample, sch, top_p=0.8, seed=20 + trial)
        assert torch.equal(t, b["tok_depth"]["tensor"]), trial
        assert torch.equal(a["tok_depth"]["input_mask"], b["tok_depth"]["input_mask"]) and b["tok_depth"]["target_mask"].all()
        assert all(torch.equal(sample["tok_depth"][k], before[k]) for k in before)
    keys = [k for k in eng._graphs if k[0] == "generate"]
    assert len(keys) == 1 and keys[0][-1] == ("maskgit",) * 3                                # one graph, its key names the schemes
    # the same counts under ROAR are another graph
    graphed.generate_graphed(sample, _depth_schedule("roar")[:1], top_p=0.8, seed=1)
    assert sum(1 for k in eng._graphs if k[0] == "generate") == 2


def test_maskgit_unequal_open_counts_raise_on_the_graphed_path_only(eng384):
    sample = _depth_sample(2, "uneq", seed=5)
    d = sample["tok_depth"]
    d["input_mask"][1, N_KNOWN] = False                       # clip 1 knows one token more: 2047 open
    d["target_mask"][1, N_KNOWN] = True
    sch = _depth_schedule()
    with pytest.raises(ValueError, match="same number of open"):
        GenerationSampler(eng384).generate_graphed(sample, sch, top_p=0.8, seed=0)
    out = GenerationSampler(eng384, use_graphs=False).generate(sample, sch, top_p=0.8, seed=0)     # the reference's sample-0 rule
    assert out["tok_depth"]["target_mask"].all()
    bad = [dict(sch[0], scheme="beam")]
    for run in (GenerationSampler(eng384, use_graphs=False).generate, GenerationSampler(eng384).generate_graphed):
        with pytest.raises(ValueError, match="Invalid sampling scheme"):
            run(_depth_sample(2, "bad", seed=6), bad, top_p=0.8, seed=0)


def test_chained_roar_then_maskgit_schedule_eager_equals_graphed():
    cfg = MODEL_CFGS["ego_b_2e_2d"]
    eng = Engine(cfg, "cuda:0", max_batch=2, n_enc=64, n_dec=64)
    eng.init_random(6)
    sch = build_chained_generation_schedules(["tok_rgb"], ["tok_depth", "tok_cam"], [5120, 30], ["roar", "maskgit"], [3, 3],
                                             ["linear", "cosine"], [0.01, 1.0], ["constant", "constant"], [2.0, 2.0],
                                             ["constant", "constant"], cfg_grow_conditioning=True)
    assert [s["scheme"] for s in sch] == ["roar"] * 3 + ["maskgit"] * 3
    sample = {"tok_rgb": {"tensor": synth.randint("chain.rgb", (2, 5, 32, 32), 64000, seed=2).to(DEV)}}
    for tg, n in (("tok_depth", 5120), ("tok_cam", 30)):
        sample = init_empty_target_modality(sample, MODALITY_INFO, tg, 2, n, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    a = GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=7)
    b = GenerationSampler(eng).generate_graphed(sample, sch, top_p=0.8, seed=7)
    for tg, vocab in (("tok_depth", 64000), ("tok_cam", 256)):
        assert torch.equal(a[tg]["tensor"], b[tg]["tensor"]), tg
        assert a[tg]["target_mask"].all() and b[tg]["target_mask"].all() and not b[tg]["input_mask"].any()
        assert int(a[tg]["tensor"].min()) >= 0 and int(a[tg]["tensor"].max()) < vocab
