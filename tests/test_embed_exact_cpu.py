"""What tests/test_embed_exact_gpu.py relies on, proven on the host (no GPU):
  * every generator of tests/_embed_ref.py delivers the geometry its GPU case claims - run lengths per owner workgroup, the 2048 / 2049
    pair totals, the keys a flush of the fallback cuts (the collect-and-flush rule is simulated here), the width templates, the one-wave
    threshold, the slot patterns;
  * every exact case's sums stay below 2^24 in magnitude in any order;
  * the bound gamma(n + 1) (|init| + sum |x_i|) admits plain fp32 evaluations on the host in sequential, reversed and pairwise order;
  * the numpy loss_perm and row-list references agree with brute-force restatements on small inputs."""
import numpy as np
import pytest
import torch

import _embed_ref as E


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_scan_cases_sit_on_the_row_scan_seams():
    assert [E.scan_quarter(r) for r in E.SCAN_ROWS] == [512] * 7 + [1024, 1024]          # 2048 -> 2049: the quarter doubles
    assert {r % 4 for r in E.SCAN_ROWS} == {0, 1, 3} and E.SCAN_MISALIGNED % 4 != 0
    for rows in E.SCAN_ROWS:
        c = E.scan_case(rows)
        assert c["slot"].numel() == rows and c["D"] == 128 and c["V"] == [1024, 600]
        assert E.max_owner_pairs(c) <= E.ET_CAP                                       # fast path
        keep = c["slot"] >= 0
        assert int(c["slot"][0]) >= 0 and bool((c["tok"][keep].long() < torch.tensor(c["V"])[c["slot"][keep].long()]).all())
        if rows >= 511:
            frac = 1.0 - float(keep.float().mean())
            assert 0.02 < frac < 0.09 and bool((c["tok"][~keep] == E.GARBAGE).all())
    assert E.scan_case(E.SCAN_MISALIGNED, True)["misalign"]


def test_runs_case_has_the_run_lengths_in_one_owner():
    c = E.runs_case()
    n = E.key_counts(c, E.RUN_OWNER)
    toks = [E.RUN_OWNER + E.ET_WGS * k for k in range(len(E.RUN_LENGTHS))]
    assert [n[t] for t in toks] == list(E.RUN_LENGTHS)                                # slot 0: key = token id
    assert [n[(1 << 16) | t] for t in toks] == [2] * len(toks) and len(n) == 2 * len(toks)   # the same token ids in table 1
    assert sum(n.values()) == 1130 and E.max_owner_pairs(c) == 1130 <= E.ET_CAP       # fast path
    assert {E.ET_HEAVY - 1, E.ET_HEAVY, E.ET_HEAVY + 1} <= set(E.RUN_LENGTHS)
    heavy = [x for x in E.RUN_LENGTHS if x >= E.ET_HEAVY]
    assert {x % 4 for x in heavy} == {0, 1, 2, 3}                                     # (cnt + 3) / 4 differs from cnt / 4 for three of them
    # the rows of a key are scattered among the others: no key's rows are consecutive
    rows, keys = E.owner_pairs(c, E.RUN_OWNER)
    r257 = rows[keys == toks[-1]]
    assert int(r257[-1] - r257[0]) > 4 * 257


@pytest.mark.parametrize("pairs", [2048, 2049])
def test_cap_cases_hit_the_fast_path_limit(pairs):
    c = E.cap_case(pairs)
    n = E.key_counts(c, E.CAP_OWNER)
    assert sum(n.values()) == pairs == E.max_owner_pairs(c)
    assert sorted(n.values(), reverse=True)[0] == 700 and 63 in n.values() and 64 in n.values() and 65 in n.values()
    others = torch.bincount(c["tok"][c["slot"] >= 0].long() % E.ET_WGS, minlength=E.ET_WGS)
    others[E.CAP_OWNER] = 0
    assert int(others.max()) < 64                                                    # every other owner stays on the fast path
    segs = E.fallback_segments(c, E.CAP_OWNER)
    assert all(len(s) <= E.ET_CAP for s in segs)
    if pairs > E.ET_CAP:                                                              # the first fallback: a flush cuts runs
        assert len(segs) == 2 and E.cut_keys(c, E.CAP_OWNER)


def test_flush_case_cuts_a_heavy_and_a_light_run():
    c = E.flush_case()
    assert c["slot"].numel() == 6000
    n = E.key_counts(c, E.CAP_OWNER)
    heavy = c["meta"]["heavy"]
    assert n[heavy] == E.FLUSH_HEAVY_ROWS and len(n) == 1 + E.FLUSH_LIGHT_KEYS
    assert all(v == E.FLUSH_LIGHT_ROWS < E.ET_HEAVY for k, v in n.items() if k != heavy)
    segs = E.fallback_segments(c, E.CAP_OWNER)
    assert len(segs) >= 3 and all(E.ET_CAP - 256 < len(s) <= E.ET_CAP for s in segs[:-1]) and len(segs[-1]) <= E.ET_CAP
    cut = E.cut_keys(c, E.CAP_OWNER)
    assert heavy in cut and len(cut - {heavy}) >= 1
    assert all(s.count(heavy) >= E.ET_HEAVY for s in segs)                            # the heavy key takes the whole-workgroup path in every flush
    assert any(0 < s.count(k) < E.ET_HEAVY for s in segs for k in cut - {heavy})


def test_width_and_one_wave_cases_sit_on_the_thresholds():
    assert [E.maxc(D) for D in E.WIDTHS] == [3, 3, 4, 4, 6, 6, 8, 8]                   # both sides of every MAXC boundary
    assert all(D % 4 == 0 and D <= 2048 for D in E.WIDTHS)
    assert 4 * (4 + 1) * 2048 * 4 == E.ES_LDS_BYTES and E.es_waves(4, 2048) == 4      # the exact-fit four-wave case
    assert [E.es_waves(m, D) for m, D in E.ONEWAVE_SHAPES] == [1, 1, 1, 4]
    assert (8 + 1) * 1136 <= 10240 < (8 + 1) * 1152 and E.es_waves(8, 1140) == 1      # 1136: the largest four-wave width of 8 modalities
    assert [r % 32 for r in E.ONEWAVE_ROWS] == [1, 1, 12] and [r % 128 for r in E.ONEWAVE_ROWS] == [33, 1, 44]
    assert (E.TWO_LEVEL_ROWS + 31) // 32 > 64
    for D in E.WIDTHS:
        c = E.width_case(D)
        assert len(c["V"]) == 4 and c["slot"].numel() == 300 and set(c["slot"].tolist()) == {-1, 0, 1, 2, 3}
    for (m, D), rows in zip(E.ONEWAVE_SHAPES, E.ONEWAVE_ROWS):
        c = E.onewave_case(m, D, rows)
        assert int(c["slot"].max()) == m - 1 and c["slot"].numel() == rows


@pytest.mark.parametrize("D", [128, 1152])
def test_slot_patterns_are_what_they_claim(D):
    P = {p: E.pattern_case(p, D) for p in E.SLOT_PATTERNS}
    s = P["runs"]["slot"]
    change = (s[1:] != s[:-1]).nonzero().flatten() + 1
    assert np.diff([0] + change.tolist() + [s.numel()]).tolist() == [1, 2, 31, 32, 33, 40, 5, 16]
    s = P["alternate"]["slot"]
    assert bool((s[1:] != s[:-1]).all()) and int(s.min()) == 0
    s = P["pad32"]["slot"]
    assert bool((s[64:96] == -1).all()) and 64 % 32 == 0 and bool((s[32:64] >= 0).any()) and bool((s[96:128] >= 0).any())
    s = P["reg"]["slot"]
    assert int((s == -2).sum()) == 16 and bool((s[:4] == -2).all())
    s = P["empty_mod"]["slot"]
    assert not bool((s == 1).any()) and bool((s == 0).any()) and bool((s == 2).any())
    assert P["no_table"]["has_table"] == [True, False, True] and bool((P["no_table"]["slot"] == 1).any())
    c = P["tok_edges"]
    assert set(c["tok"][c["slot"] >= 0].tolist()) == {0, 63}
    c = E.slot7_case()
    assert len(c["V"]) == 8 and c["V"][7] == 65536
    k7 = c["tok"][c["slot"] == 7].tolist()
    assert k7.count(65535) == 5 and 0 in k7 and 65535 - E.ET_WGS in k7
    assert (7 << 16) | 65535 == 0x7FFFF                                               # the largest key the kernel forms


def test_every_bwd_case_respects_the_entry_points_limits():
    for name, (build, _) in E.BWD_CASES.items():
        c = build()
        assert c["name"] == name
        slot, tok = c["slot"].long(), c["tok"].long()
        keep = slot >= 0
        assert int(slot.max()) < len(c["V"]) <= E.MAX_MODS and int(slot.min()) >= -2
        assert bool((tok[keep] >= 0).all()) and bool((tok[keep] < torch.tensor(c["V"])[slot[keep]]).all())
        assert max(c["V"]) <= 65536 and c["D"] % 4 == 0 and c["D"] <= 2048
        for j in {E.RUN_OWNER, E.CAP_OWNER}:                                          # no flush ever holds more than the LDS lists do
            assert all(len(s) <= E.ET_CAP for s in E.fallback_segments(c, j))
    assert set(E.BWD_NUMERIC) == {"runs", "cap2048", "cap2049", "flush"} | {k for k in E.BWD_CASES if k.startswith("sums")}


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", E.BWD_EXACT)
def test_exact_cases_stay_below_2_24(name):
    """|init| + the sum of |dx| + |d2| over ALL rows, twice (two accumulating calls), bounds every partial sum of every output in
    every order"""
    c = E.BWD_CASES[name][0]()
    d = E.bwd_data(c, True)
    for t in [d["dx"], d["d2"], d["base"]] + d["mod"] + [t for t in d["tab"] if t is not None]:
        assert t.dtype == torch.float32 and bool((t == t.round()).all()) and float(t.abs().max()) <= 8
    worst = 4 + 2 * float((d["dx"].abs() + d["d2"].abs()).sum(0).max())
    assert worst < 2 ** 24
    want = E.bwd_expect_exact(c, d, 2)
    for t in want["mod"] + [want["base"]] + [t for t in want["tab"] if t is not None]:
        assert float(t.abs().max()) <= worst


def test_reg_grad_cases_are_exact_and_need_a_second_workgroup():
    assert [(D // 4 + 255) // 256 for D in E.REG_DS] == [1, 1, 2, 2]
    for B in E.REG_BS:
        for n_reg in E.REG_NS:
            c = E.reg_case(B, n_reg, 1028, True)
            dx = c["dx"].reshape(B, c["rps"], -1)
            assert bool(torch.isnan(dx[:, n_reg:]).all()) and not bool(torch.isnan(dx[:, :n_reg]).any())
            want = c["init"].long() + 2 * dx[:, :n_reg].long().sum(0)
            assert torch.equal(E.reg_ref(c, 2), want.float())


# ---------------------------------------------------------------------------------------------------------------- the bound
def _sum32(x, order):
    """fp32 sum of the rows of x [n, D] from zero"""
    x = x.astype(np.float32)
    if order == "reversed":
        x = x[::-1]
    if order == "pairwise":
        while x.shape[0] > 1:
            if x.shape[0] % 2:
                x = np.concatenate([x, np.zeros((1, x.shape[1]), np.float32)])
            x = x[0::2] + x[1::2]
        return x[0] if x.shape[0] else np.zeros(x.shape[1], np.float32)
    acc = np.zeros(x.shape[1], np.float32)
    for r in x:
        acc = acc + r
    return acc


@pytest.mark.parametrize("name", ["runs", "flush", "sums8x1152r129"])
def test_gamma_bound_admits_fp32_sums_in_three_orders(name):
    c = E.BWD_CASES[name][0]()
    d = E.bwd_data(c, False)
    ref, bound = E.bwd_expect_numeric(c, d)
    slot, tok = c["slot"].long(), c["tok"].long()
    dx, y = d["dx"].numpy(), (d["dx"] + d["d2"]).numpy()                              # dx + d2: one fp32 rounding per term, as in the kernel
    worst = 0.0
    for order in ("sequential", "reversed", "pairwise"):
        items = [(ref["base"], bound["base"], d["base"].numpy() + _sum32(dx[(slot >= 0).numpy()], order))]
        for m in range(len(c["V"])):
            sel = (slot == m).numpy()
            items.append((ref["mod"][m], bound["mod"][m], d["mod"][m].numpy() + _sum32(y[sel], order)))
            cnt = torch.bincount(tok[slot == m], minlength=c["V"][m])
            for t in torch.argsort(cnt, descending=True)[:6].tolist():                # the longest runs of this table
                rows = ((slot == m) & (tok == t)).numpy()
                items.append((ref["tab"][m][t], bound["tab"][m][t], d["tab"][m][t].numpy() + _sum32(dx[rows], order)))
        for r, b, got in items:
            err = np.abs(got.astype(np.float64) - r.numpy())
            assert (err <= b.numpy()).all(), (name, order)
            worst = max(worst, float((err / np.maximum(b.numpy(), 1e-300)).max()))
    print(f"{name}: worst |fp32 - ref| / bound over three orders = {worst:.4f}")
    # the bound of an element nothing contributes to is zero
    m0 = next(m for m in range(len(c["V"])) if ref["tab"][m] is not None)
    idle = torch.bincount(tok[slot == m0], minlength=c["V"][m0]) == 0
    assert bool(idle.any()) and bool((bound["tab"][m0][idle] == 0).all()) and torch.equal(ref["tab"][m0][idle], d["tab"][m0][idle].double())


def test_gamma():
    assert E.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and E.gamma(2501) < 1.5e-4


# ---------------------------------------------------------------------------------------------------------------- forward cases
def test_fwd_cases_cover_the_row_kinds():
    for D in E.FWD_DS:
        for rows in E.FWD_ROWS:
            for v in E.FWD_VARIANTS:
                c = E.fwd_case(D, rows, v)
                s = c["slot"]
                assert s.numel() == rows and int(s[0]) == 7
                if rows >= 3:
                    assert int(s[1]) == -1 and int(s[2]) == -2
                assert bool((c["tok"][s == -1] == E.GARBAGE).all()) and bool((c["local"][s == -1] == E.GARBAGE).all())
                assert bool((c["local"][s == -2] < E.FWD_NREG).all())
                x, emb = E.fwd_ref(c)
                assert not bool(x[s == -1].any()) and (emb is None) == (v == "noemb")
                if emb is not None:
                    assert not bool(emb[s < 0].any())
                if v == "enc_noreg":
                    assert not bool(x[s == -2].any())
                elif rows >= 3:
                    assert torch.equal(x[2], c["reg"][int(c["local"][2])])
                assert (c["tables"] is None) == (v == "dec") == (c["base_vec"] is not None)
    c = E.fwd_case(260, 301, "enc")
    assert set(c["slot"].tolist()) == set(range(-2, 8))


# ---------------------------------------------------------------------------------------------------------------- row lists
def test_row_list_references_agree_with_brute_force():
    for V in E.ROWS_VS:
        for p in E.ROWS_PATTERNS:
            f = E.compact_flags(V, p)
            count = int(np.count_nonzero(f))
            for cap in E.compact_caps(count):
                rows, word = E.compact_ref(f, cap)
                want = [i for i in range(V) if f[i]]
                assert rows.tolist() == (want[:cap] + [-1] * cap)[:cap]
                assert word == min(count, cap) + (E.TRUNC if count > cap else 0)
    assert int(np.count_nonzero(E.compact_flags(5000, "seams"))) == 5 and set(np.unique(E.compact_flags(1025, "random"))) == {0, 1, 255}
    assert int(np.count_nonzero(E.compact_flags(1024, "none"))) == 0 and E.compact_flags(1, "last")[0] == 255
    for D in (4, 260):
        for cap in E.ROWS_CAPS:
            for n in range(cap + 1):
                for word in (n, n | E.TRUNC):
                    table, rows, src = E.rowlist_case(D, cap, n, "cpu")
                    assert len(set(rows.tolist()) - {-1}) == cap - (1 if n >= 3 else 0)
                    assert all(np.isnan(table[r]).all() for r in rows[n:]) and (n < 3 or rows[1] == -1)
                    g = np.zeros((cap, D), np.float32)
                    for i in range(n):
                        if rows[i] >= 0:
                            g[i] = table[rows[i]]
                    assert np.array_equal(E.gather_ref(table, rows, word, cap), g) and not np.isnan(g).any()
                    for add in (0, 1):
                        for s in (src, None):
                            t = table.copy()
                            for i in range(n):
                                if rows[i] >= 0:
                                    t[rows[i]] = (t[rows[i]] if add else 0) + (0 if s is None else s[i])
                            got = E.scatter_ref(table, rows, word, cap, s, add)
                            assert np.array_equal(got.view(np.int32), t.view(np.int32))
                            assert not np.isnan(got[rows[:n][rows[:n] >= 0]]).any()


# ---------------------------------------------------------------------------------------------------------------- loss_perm
def _lp_brute(c):
    B, M, n = c["B"], c["M"], c["n_mods"]
    kept = sorted((int(c["canon"][c["slot"][r]]), r) for r in range(B * M) if c["slot"][r] >= 0)
    perm = [-1] * (B * M)
    for g, (_, r) in enumerate(kept):
        perm[r] = g
    ranges = [[sum(1 for cm, _ in kept if cm < k), sum(1 for cm, _ in kept if cm == k)] for k in range(n)]
    base = [[ranges[c["canon"][s]][0] + sum(1 for cm, r in kept if cm == c["canon"][s] and r // M < b) for s in range(n)] for b in range(B)]
    return perm, [int(c["tok"][r]) for _, r in kept], ranges, base


def test_loss_perm_reference_agrees_with_brute_force():
    cases = [E.lp_case(2, 30, 4, o, "orders") for o in E.LP_ORDERS[::5]]
    cases += [E.lp_case(3, 40, 1, (0,), "counts"), E.lp_case(3, 40, 8, (5, 0, 7, 2, 1, 6, 3, 4), "counts"), E.lp_case(1, 1, 4, (1, 3, 0, 2), "shapes"),
              E.lp_case(3, 30, 4, (2, 0, 3, 1), "empty", empty=2, pad_sample=1)]
    for c in cases:
        # the compaction contract: one contiguous run per sample and slot, -1 elsewhere
        slot = c["slot"].reshape(c["B"], c["M"])
        for b in range(c["B"]):
            want = np.full(c["M"], -1)
            for s in range(c["n_mods"]):
                st, n = c["seg"][b, s]
                want[st:st + n] = s
            assert np.array_equal(slot[b], want)
        ref = E.lp_ref(c)
        perm, tgt, ranges, base = _lp_brute(c)
        assert ref["perm"].tolist() == perm and ref["tgt"].tolist() == tgt and ref["total"] == len(tgt)
        assert ref["ranges"].tolist() == ranges and ref["base"].tolist() == base
    e = cases[-1]
    assert (e["seg"][:, 2, 1] == 0).all() and (e["slot"].reshape(3, 30)[1] == -1).all() and (e["seg"][1, :, 1] == 0).all()


def test_loss_perm_shapes_reach_the_grid_stride_loop_and_the_lds_limit():
    assert 37 * 7100 > 256 * 1024 and (37 * 7100 + 1023) // 1024 > 256
    assert (3 * 511 * 8 + 8) * 4 <= 48 * 1024 < (3 * 512 * 8 + 8) * 4
    assert len(E.LP_ORDERS) == 24
