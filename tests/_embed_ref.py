"""Shared pieces of the token front-end conformance tests (tests/test_embed_exact_gpu.py, tests/test_embed_exact_cpu.py): case
generators and host references for the kernels of egom2p_amd/csrc/embed.hip - ego_embed_fwd, ego_embed_bwd, ego_reg_grad,
ego_rows_compact / _gather / _scatter and ego_loss_perm.  Nothing in this module needs a GPU.

How a result is judged
----------------------
* Exact cases: dx and d2 are integers in [-8, 8], the accumulators start from integers in [-4, 4]; every partial sum of every order
  stays below 2^24 in magnitude (tests/test_embed_exact_cpu.py proves it per case), so fp32 is exact and the result must equal an
  int64 index_add_ / column sum bit for bit.
* Numeric cases: randn inputs, fp64 reference.  A sum of n fp32 terms taken in ANY order and added to an existing value obeys
  |got - ref| <= gamma(n + 1) (|init| + sum |x_i|), gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of
  Numerical Algorithms, section 4.2): every operand passes through at most n additions, and a term dx + d2 carries one more rounding.
  n is the number of rows that contribute to the element - an element no row contributes to has bound 0.  No factor is applied.
* ego_embed_fwd and ego_reg_grad state their order of evaluation (token + (pos + mod); b ascending): fp32 torch on the host in that
  order gives the expected bits.
"""
import itertools

import numpy as np
import torch

from _rowops_ref import NAN_F32, SENT_F32, SENT_U8, gen, ibits, sbits  # noqa: F401  (the frame helpers, shared with the GPU half)

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
U = 2.0 ** -24                          # unit roundoff of fp32
SENT_I32 = 0x7FA55AA5                   # output frames of int32 buffers (no row index, count or token is that large)
GARBAGE = 0x7FFFFFFF                    # `local` / `tok` of rows that must not be looked up
MAX_MODS = 8

# the constants of embed_tables_kernel / embed_sums_kernel the generators aim at
ET_WGS, ET_CAP, ET_HEAVY = 512, 2048, 64
ES_LDS_BYTES = 160 * 1024


def gamma(k):
    return k * U / (1.0 - k * U)


def es_waves(n_mods, D):
    """waves per workgroup of embed_sums_kernel: four row sets of (n_mods + 1) x D floats in 160 KiB of LDS, else one"""
    return 4 if 4 * (n_mods + 1) * D * 4 <= ES_LDS_BYTES else 1


def maxc(D):
    """the width template (16-byte chunks per lane) ego_embed_bwd picks"""
    return 3 if D <= 768 else 4 if D <= 1024 else 6 if D <= 1536 else 8


def scan_quarter(rows):
    """rows each wave of embed_tables_kernel scans on the fast path"""
    return ((rows + 3) // 4 + 511) // 512 * 512


# ================================================================================================================ ego_embed_bwd
def _case(name, D, V, slot, tok, has_table=None, misalign=False, **meta):
    return dict(name=name, D=D, V=list(V), slot=slot.to(I32).contiguous(), tok=tok.to(I32).contiguous(),
                has_table=[True] * len(V) if has_table is None else list(has_table), misalign=misalign, meta=meta)


def random_rows(rows, V, key, pad=0.05):
    """random slots and token ids; `pad` of the rows (never row 0) are padding: slot -1 and a token id that must not be used"""
    g = gen("embed rows", *key)
    slot = torch.randint(0, len(V), (rows,), generator=g)
    tok = (torch.rand(rows, generator=g, dtype=F64) * torch.tensor(V, dtype=F64)[slot]).long()
    padm = torch.rand(rows, generator=g) < pad
    padm[0] = False
    slot[padm], tok[padm] = -1, GARBAGE
    return slot, tok


def _filler(n, V, j, key):
    """random rows none of which belongs to owner workgroup j (j < 511)"""
    slot, tok = random_rows(n, V, key)
    hit = (slot >= 0) & (tok % ET_WGS == j)
    tok[hit] += 1
    return slot, tok


def _shuffled(slot, tok, key):
    p = torch.randperm(slot.numel(), generator=gen("embed shuffle", *key))
    return slot[p], tok[p]


def _keyed(pairs):
    """[(slot, tok, count)] -> the rows, key after key"""
    slot = torch.cat([torch.full((n,), s, dtype=I64) for s, _, n in pairs])
    tok = torch.cat([torch.full((n,), t, dtype=I64) for _, t, n in pairs])
    return slot, tok


# ---- 1. row-scan seams
SCAN_ROWS = (1, 3, 511, 512, 513, 2047, 2048, 2049, 2051)
SCAN_MISALIGNED = 2049


def scan_case(rows, misalign=False):
    V = [1024, 600]
    slot, tok = random_rows(rows, V, ("scan", rows))
    return _case(f"scan{rows}{'m' if misalign else ''}", 128, V, slot, tok, misalign=misalign)


# ---- 2. run lengths in one owner workgroup
RUN_LENGTHS = (1, 3, 4, 5, 63, 64, 65, 66, 67, 255, 256, 257)
RUN_OWNER = 37


def runs_case():
    V, j = [8192, 8192], RUN_OWNER
    keys = [(0, j + ET_WGS * k, n) for k, n in enumerate(RUN_LENGTHS)]
    keys += [(1, j + ET_WGS * k, 2) for k in range(len(RUN_LENGTHS))]          # the same token ids in another table
    s0, t0 = _keyed(keys)
    s1, t1 = _filler(1500, V, j, ("runs",))
    slot, tok = _shuffled(torch.cat([s0, s1]), torch.cat([t0, t1]), ("runs",))
    return _case("runs", 128, V, slot, tok, owner=j, keys=keys)


# ---- 3. fast-path limit and fallback flushes
CAP_OWNER = 5


def cap_case(pairs):
    """owner CAP_OWNER receives exactly `pairs` (key, row) pairs: 22 keys, run lengths 700, 64, 63 and a spread round 64"""
    V, j = [8192, 8192], CAP_OWNER
    ids = [(s, j + ET_WGS * k) for k in range(16) for s in range(2)]
    keys = [(*ids[0], 700), (*ids[1], 64), (*ids[2], 63)]
    rest, nk = pairs - 827, 19
    keys += [(*ids[3 + i], rest // nk + (1 if i < rest % nk else 0)) for i in range(nk)]
    s0, t0 = _keyed(keys)
    s1, t1 = _filler(1000, V, j, ("cap", pairs))
    slot, tok = _shuffled(torch.cat([s0, s1]), torch.cat([t0, t1]), ("cap", pairs))
    return _case(f"cap{pairs}", 128, V, slot, tok, owner=j, keys=keys)


FLUSH_HEAVY_ROWS, FLUSH_LIGHT_KEYS, FLUSH_LIGHT_ROWS = 2500, 40, 50


def flush_case():
    """6000 rows: one key of owner CAP_OWNER has 2500 rows, 40 more keys of the same owner 50 each, 1500 rows of other owners"""
    V, j = [8192, 8192, 8192], CAP_OWNER
    ids = [(s, j + ET_WGS * k) for k in range(16) for s in range(3)]
    heavy = ids.pop(9)
    keys = [(*heavy, FLUSH_HEAVY_ROWS)] + [(*ids[i], FLUSH_LIGHT_ROWS) for i in range(FLUSH_LIGHT_KEYS)]
    s0, t0 = _keyed(keys)
    s1, t1 = _filler(1500, V, j, ("flush",))
    slot, tok = _shuffled(torch.cat([s0, s1]), torch.cat([t0, t1]), ("flush",))
    return _case("flush", 128, V, slot, tok, owner=j, keys=keys, heavy=(heavy[0] << 16) | heavy[1])


def owner_pairs(case, j):
    """(rows, keys) of the pairs owner workgroup j collects, in row order"""
    slot, tok = case["slot"].long(), case["tok"].long()
    has = torch.tensor(case["has_table"] + [False])[slot.clamp(-1, len(case["V"]) - 1)]
    mine = (slot >= 0) & has & (tok % ET_WGS == j)
    rows = mine.nonzero().flatten()
    return rows, (slot[rows] << 16) | tok[rows]


def max_owner_pairs(case):
    slot, tok = case["slot"].long(), case["tok"].long()
    has = torch.tensor(case["has_table"] + [False])[slot.clamp(-1, len(case["V"]) - 1)]
    mine = (slot >= 0) & has
    return int(torch.bincount(tok[mine] % ET_WGS, minlength=ET_WGS).max()) if bool(mine.any()) else 0


def key_counts(case, j):
    _, keys = owner_pairs(case, j)
    k, n = torch.unique(keys, return_counts=True)
    return dict(zip(k.tolist(), n.tolist()))


def fallback_segments(case, j):
    """the collect-and-flush rule of embed_tables_kernel's fallback for owner j: 256 rows per step, a flush as soon as more than
    ET_CAP - 256 pairs are held, one at the end.  Returns the key lists of the flushes."""
    rows, keys = owner_pairs(case, j)
    rows, keys = rows.tolist(), keys.tolist()
    segs, cur, p = [], [], 0
    for base in range(0, case["slot"].numel(), 256):
        while p < len(rows) and rows[p] < base + 256:
            cur.append(keys[p])
            p += 1
        if len(cur) > ET_CAP - 256:
            segs.append(cur)
            cur = []
    if cur:
        segs.append(cur)
    return segs


def cut_keys(case, j):
    """keys of owner j whose rows are spread over more than one flush"""
    seen = {}
    for i, seg in enumerate(fallback_segments(case, j)):
        for k in set(seg):
            seen.setdefault(k, []).append(i)
    return {k for k, v in seen.items() if len(v) > 1}


# ---- 4. width templates, 5. the one-wave path of embed_sums_kernel
WIDTHS = (4, 768, 772, 1024, 1028, 1536, 1540, 2048)


def width_case(D):
    V = [1024] * 4
    slot, tok = random_rows(300, V, ("width", D))
    return _case(f"width{D}", D, V, slot, tok)


ONEWAVE_SHAPES = ((5, 2048), (8, 1152), (8, 1280), (8, 1136))
ONEWAVE_ROWS = (33, 129, 300)
TWO_LEVEL_ROWS = 2100                   # one-wave path: 66 partial rows, more than one 64-row chunk of the ordered column sum


def onewave_case(n_mods, D, rows):
    V = [64] * n_mods
    slot, tok = random_rows(rows, V, ("onewave", n_mods, D, rows))
    return _case(f"sums{n_mods}x{D}r{rows}", D, V, slot, tok)


# ---- 6. slot patterns
SLOT_PATTERNS = ("runs", "alternate", "pad32", "reg", "empty_mod", "no_table", "tok_edges")


def pattern_case(pattern, D):
    V, rows = [64, 64, 64], 160
    slot, tok = random_rows(rows, V, ("pattern", pattern, D))
    has = None
    if pattern == "runs":                                    # runs of one modality: lengths round a wave's 32 rows
        lens = [1, 2, 31, 32, 33, 40, 5, 16]
        slot = torch.cat([torch.full((n,), i % 3, dtype=I64) for i, n in enumerate(lens)])[:rows]
        slot = torch.cat([slot, torch.full((rows - slot.numel(),), 1, dtype=I64)])
        tok = torch.randint(0, 64, (rows,), generator=gen("pattern runs", D))
    elif pattern == "alternate":
        slot = torch.arange(rows) % 3
        tok = torch.randint(0, 64, (rows,), generator=gen("pattern alt", D))
    elif pattern == "pad32":
        slot[64:96], tok[64:96] = -1, GARBAGE
    elif pattern == "reg":                                   # 4 register rows in front of every 40-row sample
        r = torch.arange(rows) % 40 < 4
        slot[r], tok[r] = -2, 0
    elif pattern == "empty_mod":
        keep = slot >= 0
        slot[keep] = slot[keep] // 2 * 2                     # modality 1 owns no row
    elif pattern == "no_table":
        has = [True, False, True]
    elif pattern == "tok_edges":
        keep = slot >= 0
        tok[keep] = torch.where(torch.arange(rows)[keep] % 3 == 0, 0, 63)
    return _case(f"{pattern}{D}", D, V, slot, tok, has_table=has)


def slot7_case():
    """eight modalities; slot 7 has V = 65536 and rows with token 65535, the largest 16-bit key, beside 0 and 65023 (same owner)"""
    V = [16] * 7 + [65536]
    slot, tok = random_rows(200, V, ("slot7",), pad=0.05)
    for i, t in enumerate([65535] * 5 + [0] * 2 + [65535 - ET_WGS] * 3 + [65534]):
        slot[3 + 7 * i], tok[3 + 7 * i] = 7, t
    return _case("slot7", 128, V, slot, tok)


def options_case():
    V = [1024, 600]
    slot, tok = random_rows(300, V, ("options",))
    return _case("options", 128, V, slot, tok)


def bwd_cases():
    """name -> (builder, also run numeric)"""
    c = {}
    for rows in SCAN_ROWS:
        c[f"scan{rows}"] = (lambda rows=rows: scan_case(rows), False)
    c[f"scan{SCAN_MISALIGNED}m"] = (lambda: scan_case(SCAN_MISALIGNED, True), False)
    c["runs"] = (runs_case, True)
    c["cap2048"] = (lambda: cap_case(2048), True)
    c["cap2049"] = (lambda: cap_case(2049), True)
    c["flush"] = (flush_case, True)
    for D in WIDTHS:
        c[f"width{D}"] = (lambda D=D: width_case(D), False)
    for (m, D), rows in itertools.product(ONEWAVE_SHAPES, ONEWAVE_ROWS):
        c[f"sums{m}x{D}r{rows}"] = (lambda m=m, D=D, rows=rows: onewave_case(m, D, rows), True)
    for D, p in itertools.product((128, 1152), SLOT_PATTERNS):
        c[f"{p}{D}"] = (lambda p=p, D=D: pattern_case(p, D), False)
    c["slot7"] = (slot7_case, False)
    return c


BWD_CASES = bwd_cases()
BWD_EXACT = list(BWD_CASES)
BWD_NUMERIC = [k for k, (_, num) in BWD_CASES.items() if num]


def bwd_data(case, exact):
    """dx, d2 and the values the accumulators start from; touched flags: 3 % already set"""
    rows, D = case["slot"].numel(), case["D"]
    g = gen("embed bwd data", case["name"], exact)

    def draw(shape, lim):
        return torch.randint(-lim, lim + 1, shape, generator=g).float() if exact else torch.randn(shape, generator=g)
    d = dict(dx=draw((rows, D), 8), d2=draw((rows, D), 8), base=draw((D,), 4), mod=[draw((D,), 4) for _ in case["V"]],
             tab=[draw((v, D), 4) if h else None for v, h in zip(case["V"], case["has_table"])])
    d["touched"] = [(torch.rand(v, generator=g) < 0.03).to(U8) if h else None for v, h in zip(case["V"], case["has_table"])]
    return d


def _bwd_sums(case, dx, d2, dtype):
    """per table, modality and base: the sums of one call in `dtype` (int64: exact; fp64: reference), and the contributing rows"""
    slot, tok = case["slot"].long(), case["tok"].long()
    D = case["D"]
    x = dx.to(dtype)
    y = x if d2 is None else x + d2.to(dtype)
    tab, mod, cnt_tab, cnt_mod = [], [], [], []
    for m, v in enumerate(case["V"]):
        sel = slot == m
        mod.append(y[sel].sum(0))
        cnt_mod.append(int(sel.sum()))
        if case["has_table"][m]:
            tab.append(torch.zeros(v, D, dtype=dtype).index_add_(0, tok[sel], x[sel]))
            cnt_tab.append(torch.bincount(tok[sel], minlength=v))
        else:
            tab.append(None)
            cnt_tab.append(None)
    keep = slot >= 0
    return dict(tab=tab, mod=mod, base=x[keep].sum(0), cnt_tab=cnt_tab, cnt_mod=cnt_mod, cnt_base=int(keep.sum()))


def bwd_expect_exact(case, data, calls, d2=True, dbase=True):
    """the fp32 tensors `calls` accumulating calls must leave, from int64 sums; flags = row received a contribution"""
    s = _bwd_sums(case, data["dx"], data["d2"] if d2 else None, I64)
    out = dict(tab=[None if t is None else (i.to(I64) + calls * t).float() for t, i in zip(s["tab"], data["tab"])],
               mod=[(i.to(I64) + calls * t).float() for t, i in zip(s["mod"], data["mod"])],
               base=(data["base"].to(I64) + calls * s["base"]).float() if dbase else data["base"].clone(),
               got_row=[None if c is None else c > 0 for c in s["cnt_tab"]])
    return out


def bwd_expect_numeric(case, data, d2=True, dbase=True):
    """one call: (fp64 reference, per-element bound gamma(n + 1) (|init| + sum |x_i|)) for every table, modality sum and the base"""
    s = _bwd_sums(case, data["dx"], data["d2"] if d2 else None, F64)
    a = _bwd_sums(case, data["dx"].abs() if not d2 else (data["dx"].double() + data["d2"].double()).abs(), None, F64)
    at = _bwd_sums(case, data["dx"].abs(), None, F64)         # tables and base sum dx alone
    ref, bound = dict(tab=[], mod=[]), dict(tab=[], mod=[])
    for m in range(len(case["V"])):
        if s["tab"][m] is None:
            ref["tab"].append(None)
            bound["tab"].append(None)
        else:
            i = data["tab"][m].double()
            ref["tab"].append(i + s["tab"][m])
            n = s["cnt_tab"][m].double()[:, None]
            bound["tab"].append(torch.where(n > 0, gamma(n + 1) * (i.abs() + at["tab"][m]), torch.zeros_like(i)))
        i = data["mod"][m].double()
        ref["mod"].append(i + s["mod"][m])
        n = s["cnt_mod"][m]
        bound["mod"].append(gamma(n + 1) * (i.abs() + a["mod"][m]) if n else torch.zeros_like(i))
    i = data["base"].double()
    ref["base"] = i + s["base"] if dbase else i
    bound["base"] = gamma(s["cnt_base"] + 1) * (i.abs() + at["base"]) if dbase else torch.zeros_like(i)
    return ref, bound


# ================================================================================================================ ego_embed_fwd
FWD_DS = (4, 128, 260, 1024, 2048)
FWD_ROWS = (1, 3, 4, 5, 301)
FWD_VARIANTS = ("enc", "enc_noreg", "dec", "noemb")
FWD_NREG = 3


def fwd_case(D, rows, variant):
    """eight modalities (table m: 11 + m rows, 9 + m positions), rows led by slot 7, a padding row, a register row; padding rows
    carry GARBAGE in local and tok, register rows in tok"""
    g = gen("embed fwd", D, rows, variant)
    lead = torch.tensor([7, -1, -2, 0, 3])
    slot = torch.cat([lead, torch.randint(-2, MAX_MODS, (max(0, rows - 5),), generator=g)])[:rows]
    sc = slot.clamp_min(0)
    tok = (torch.rand(rows, generator=g) * (11 + sc)).long()
    local = (torch.rand(rows, generator=g) * (9 + sc)).long()
    local[slot == -2] = torch.randint(0, FWD_NREG, (int((slot == -2).sum()),), generator=g)
    tok[slot < 0] = GARBAGE
    local[slot == -1] = GARBAGE
    c = dict(D=D, rows=rows, variant=variant, slot=slot.to(I32), tok=tok.to(I32), local=local.to(I32),
             tables=[torch.randn(11 + m, D, generator=g) for m in range(MAX_MODS)],
             pos=[torch.randn(9 + m, D, generator=g) for m in range(MAX_MODS)],
             mod=[torch.randn(D, generator=g) for m in range(MAX_MODS)],
             base_vec=torch.randn(D, generator=g), reg=torch.randn(FWD_NREG, D, generator=g))
    if variant == "dec":
        c["tables"] = None
    else:
        c["base_vec"] = None
    if variant == "enc_noreg":
        c["reg"] = None
    return c


def fwd_ref(c):
    """x = tab + (pos + mod) in fp32 in that order, emb = pos + mod; padding rows zeros; register rows x = reg[local], emb = 0"""
    x = torch.zeros(c["rows"], c["D"])
    emb = torch.zeros(c["rows"], c["D"])
    slot, tok, local = c["slot"].long(), c["tok"].long(), c["local"].long()
    for m in range(MAX_MODS):
        sel = slot == m
        e = c["pos"][m][local[sel]] + c["mod"][m]
        t = c["base_vec"].expand_as(e) if c["tables"] is None else c["tables"][m][tok[sel]]
        emb[sel] = e
        x[sel] = t + e
    if c["reg"] is not None:
        sel = slot == -2
        x[sel] = c["reg"][local[sel]]
    return x, (None if c["variant"] == "noemb" else emb)


# ================================================================================================================ ego_reg_grad
REG_BS, REG_NS, REG_DS = (1, 3), (1, 4), (4, 1024, 1028, 2048)


def reg_case(B, n_reg, D, exact):
    """dx [B (n_reg + 5), D]: the rows that are not register rows hold NaN; dreg starts from values"""
    rps = n_reg + 5
    g = gen("reg grad", B, n_reg, D, exact)
    dx = torch.full((B, rps, D), float("nan"))
    if exact:
        dx[:, :n_reg] = torch.randint(-8, 9, (B, n_reg, D), generator=g).float()
        init = torch.randint(-4, 5, (n_reg, D), generator=g).float()
    else:
        dx[:, :n_reg] = torch.randn(B, n_reg, D, generator=g)
        init = torch.randn(n_reg, D, generator=g)
    return dict(B=B, n_reg=n_reg, rps=rps, D=D, dx=dx.reshape(B * rps, D), init=init)


def reg_ref(c, calls=1):
    """dreg += (sum over b ascending, from zero) in fp32, once per call"""
    dx = c["dx"].reshape(c["B"], c["rps"], c["D"])
    acc = torch.zeros(c["n_reg"], c["D"])
    for b in range(c["B"]):
        acc = acc + dx[b, :c["n_reg"]]
    out = c["init"].clone()
    for _ in range(calls):
        out = out + acc
    return out


# ================================================================================================================ ego_rows_*
ROWS_VS = (1, 1023, 1024, 1025, 5000)
ROWS_PATTERNS = ("none", "all", "last", "seams", "random")
ROWS_DS = (4, 252, 256, 260, 768)
ROWS_CAPS = (1, 5, 8)
TRUNC = 0x40000000


def compact_flags(V, pattern):
    """uint8 flags; set flags are 1 or 255 (any non-zero value counts)"""
    f = np.zeros(V, np.uint8)
    if pattern == "all":
        f[:] = 1
        f[1::2] = 255
    elif pattern == "last":
        f[V - 1] = 255
    elif pattern == "seams":                                 # wave (64) and pass (1024) seams of rows_compact_kernel
        for i in (63, 64, 65, 1023, 1024):
            if i < V:
                f[i] = 1 if i % 2 else 255
    elif pattern == "random":
        r = torch.rand(V, generator=gen("rows flags", V)).numpy()
        f[r < 0.3] = 1
        f[r < 0.15] = 255
    return f


def compact_caps(count):
    return (count - 1, count, count + 1) if count > 1 else (1, 2)


def compact_ref(flags, cap):
    """(rows [cap]: ascending set flags, -1 behind them; count word with bit 30 when the list is truncated)"""
    idx = np.flatnonzero(flags).astype(np.int32)
    rows = np.full(cap, -1, np.int32)
    n = min(idx.size, cap)
    rows[:n] = idx[:n]
    return rows, n | (TRUNC if idx.size > cap else 0)


def gather_ref(table, rows, count, cap):
    n = count & 0x3FFFFFFF
    out = np.zeros((cap, table.shape[1]), np.float32)
    use = (np.arange(cap) < n) & (rows[:cap] >= 0)
    out[use] = table[rows[:cap][use]]
    return out


def scatter_ref(table, rows, count, cap, src, add):
    n = min(count & 0x3FFFFFFF, cap)
    out = table.copy()
    use = (np.arange(cap) < n) & (rows[:cap] >= 0)
    r = rows[:cap][use]
    v = np.zeros((r.size, table.shape[1]), np.float32) if src is None else src[:cap][use]
    out[r] = (table[r] + v) if add else v
    return out


def rowlist_case(D, cap, count, key):
    """a 24-row table of small integers whose rows that are not listed hold NaN; rows: `count` distinct listed rows in ascending
    order with one -1 among them (count >= 3), and in-range rows of NaN behind `count` that must not be used"""
    V = 24
    g = gen("rowlist", D, cap, count, key)
    listed = np.sort(torch.randperm(V, generator=g)[:cap].numpy()).astype(np.int32)
    rows = listed.copy()
    live = rows[:count].copy()
    if count >= 3:
        rows[1] = -1
        live = np.delete(live, 1)
    table = np.full((V, D), np.nan, np.float32)
    table[live] = torch.randint(-8, 9, (live.size, D), generator=g).numpy().astype(np.float32)
    src = torch.randint(-8, 9, (cap, D), generator=g).numpy().astype(np.float32)
    src[count:] = np.nan
    if count >= 3:
        src[1] = np.nan
    return table, rows, src


# ================================================================================================================ ego_loss_perm
def lp_case(B, M, n_mods, canon, key, empty=None, pad_sample=None):
    """host statement of the compaction contract: per sample the decoder slots in order, one contiguous [start, start + count) run
    each, padding (slot -1, garbage token) behind them.  canon: decoder slot -> canonical modality."""
    g = gen("loss perm", B, M, n_mods, tuple(canon), key)
    seg = np.zeros((B, n_mods, 2), np.int32)
    slot = np.full((B, M), -1, np.int32)
    tok = np.full((B, M), GARBAGE, np.int32)
    for b in range(B):
        kept = M if M < 4 else int(torch.randint(M // 2, M + 1, (1,), generator=g))
        if pad_sample == b:
            kept = 0
        cuts = np.sort(torch.randint(0, kept + 1, (n_mods - 1,), generator=g).numpy())
        cnt = np.diff(np.concatenate([[0], cuts, [kept]])).astype(np.int64)
        if empty is not None:
            cnt[empty] = 0
        start = 0
        for s in range(n_mods):
            seg[b, s] = (start, cnt[s])
            slot[b, start:start + cnt[s]] = s
            start += cnt[s]
        tok[b, :start] = torch.randint(0, 64000, (int(start),), generator=g).numpy()
    return dict(B=B, M=M, n_mods=n_mods, canon=np.asarray(canon, np.int32), seg=seg, slot=slot.reshape(-1), tok=tok.reshape(-1))


def lp_ref(c):
    """the row order of y[decoder_mod_mask == id], modality after modality in canonical order: perm, tgt_perm[:total], ranges, base"""
    slot, canon, n_mods = c["slot"], c["canon"], c["n_mods"]
    mm = np.where(slot >= 0, canon[np.clip(slot, 0, None)], -1)
    perm = np.full(slot.size, -1, np.int32)
    ranges = np.zeros((n_mods, 2), np.int32)
    tgt, off = [], 0
    for cm in range(n_mods):
        rows = np.flatnonzero(mm == cm)
        perm[rows] = off + np.arange(rows.size)
        tgt.append(c["tok"][rows])
        ranges[cm] = (off, rows.size)
        off += rows.size
    cnt = c["seg"][:, :, 1].astype(np.int64)
    before = np.cumsum(cnt, 0) - cnt                          # rows of the same slot in earlier samples
    base = (ranges[canon, 0][None, :] + before).astype(np.int32)
    return dict(perm=perm, tgt=np.concatenate(tgt).astype(np.int32), total=off, ranges=ranges, base=base)


LP_ORDERS = list(itertools.permutations(range(4)))
LP_SHAPES = ((1, 1), (3, 1025), (37, 7100))
