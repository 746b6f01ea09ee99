"""Shared pieces of the attention conformance tests (tests/test_attention_exact_gpu.py, tests/test_attention_exact_cpu.py).

Two kinds of input.  EXACT cases have Q = 0 and 0/1 codes of the key index in V (of the query index in dO): every score is 0,
every allowed p is 1 (1 / n after the normalisation), every sum is a small integer, so the set of keys a query row used - and
the set of queries a key was used by - can be read off the outputs as integers.  The other cases are checked row by row against
`ref64` (the operation in fp64) inside an envelope that `model64` (fp64 plus the roundings the kernels document) sets.
Nothing in this module needs a GPU; tests/test_attention_exact_cpu.py proves what the GPU test relies on."""
import functools
import math
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

LOG2E_F32 = np.float32(1.4426950408889634)
LN2 = math.log(2.0)
U_BF16 = 2.0 ** -8                      # largest relative error of one round-to-nearest bf16 rounding (8 significant bits)
S_FWD_MAX, S_BWD_MAX = 127, 40          # largest code counts the recoveries are proven for (forward O, backward dV)


def bf16r(x):
    """fp32 then round-to-nearest-even bf16 (what a kernel's store does), back in fp64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def randn_bf16(shape, *key):
    return torch.randn(shape, generator=gen(*key)).to(torch.bfloat16).to(torch.float64)


def code(n):
    """[n, 64] 0/1 code of the index: column i % 32 among 0..31, column 32 + (i // 32) % 32 among 32..63"""
    i = torch.arange(n)
    c = torch.zeros(n, 64, dtype=torch.float64)
    c[i, i % 32] = 1
    c[i, 32 + (i // 32) % 32] = 1
    return c


def pow2_scale(c=0.125):
    """an fp32 `scale` whose fp32 product with log2(e) is exactly the power of two c: the kernels' operand pre-scaling
    (bf16(x * scale * log2e)) is then exact, and the exp2-domain scores are c * q . k"""
    s = np.float32(c / float(LOG2E_F32))
    for cand in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))):
        if np.float32(cand * LOG2E_F32) == np.float32(c):
            return float(cand)
    raise AssertionError("no fp32 scale gives an exact power-of-two pre-scale")


def intervals(ks, ke, Nq, Nk):
    """allowed[b, q, j] and flat[b, q] of the kernels' interval semantics: ke is clamped to Nk, an empty interval (ke <= ks after
    the clamp, which covers ks >= Nk) attends all Nk keys uniformly"""
    ks, ke = torch.as_tensor(ks).long(), torch.as_tensor(ke).long()
    if ks.dim() == 1:
        ks, ke = ks[:, None].expand(-1, Nq), ke[:, None].expand(-1, Nq)
    ke = ke.clamp(max=Nk)
    flat = ke <= ks
    j = torch.arange(Nk)
    allowed = ((j >= ks[..., None]) & (j < ke[..., None])) | flat[..., None]
    return allowed, flat


# ---- the two references ------------------------------------------------------------------------------------------------------
def ref64(q, k, v, do, ks, ke, scale):
    """The operation in fp64 on the (bf16-valued) inputs [B, H, N, d]; masked-fill semantics: an empty row attends all keys
    uniformly and has dS = 0.  lse is the natural-log log-sum-exp of the scaled scores."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    A, flat = intervals(ks, ke, q.shape[2], k.shape[2])
    fl = flat[:, None, :, None]
    s = (q @ k.transpose(-1, -2)) * scale
    s = torch.where(fl, torch.zeros_like(s), s).masked_fill(~A[:, None], -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    delta = (do * o).sum(-1)
    ds = p * (do @ v.transpose(-1, -2) - delta[..., None])
    ds = torch.where(fl, torch.zeros_like(ds), ds)
    return dict(o=o, lse=lse, delta=delta, dq=ds @ k * scale, dk=ds.transpose(-1, -2) @ q * scale, dv=p.transpose(-1, -2) @ do)


def model64(q, k, v, do, ks, ke, scale, o_lo=False, fwd=None):
    """ref64 with the roundings the kernels document, and nothing else (`fwd`: see the end):
      * the forward and the dQ kernel contract bf16(Q * scale * log2e) with K, the dK / dV kernel Q with bf16(K * scale * log2e)
        (the factor is the fp32 product of the fp32 scale and the fp32 log2e), p = exp2(score - lse2);
      * P (forward: relative to the row maximum, the sum l from the unrounded values) and dS are rounded to bf16 before their
        second products;
      * O, dQ, dK, dV are rounded to bf16; O_lo = bf16(o - O);
      * delta = rowsum(dO o O), or rowsum(dO o (O + O_lo)) when o_lo is given.
    The backward's operands include what the forward stored - O, O_lo and the log2-domain lse2.  With fwd = dict(o, olo, lse2) the
    backward half is modelled on exactly those (the forward half is unchanged): delta and p then differ from a kernel's only by
    fp32 summation, not by which way a stored O element or a P element happened to round in the forward.  That matters for a dK
    row whose error is carried by a handful of large dS (the 100 x dO rows): one dS rounding the other way moves such a row by
    more than the factor 2 allows, and a 1e-5 difference in delta flips about one dS in 400."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    A, flat = intervals(ks, ke, q.shape[2], k.shape[2])
    fl, Am = flat[:, None, :, None], A[:, None]
    c_sc, sc32 = float(np.float32(scale) * LOG2E_F32), float(np.float32(scale))
    qs = bf16r(q.float() * np.float32(c_sc))
    qs = torch.where(fl, torch.zeros_like(qs), qs)
    s2 = (qs @ k.transpose(-1, -2)).masked_fill(~Am, -math.inf)
    m = s2.max(-1, keepdim=True).values
    pu = torch.exp2(s2 - m)
    l = pu.sum(-1, keepdim=True)
    lse2 = (m + torch.log2(l))[..., 0]
    o_full = (bf16r(pu) @ v) / l
    o = bf16r(o_full)
    olo = bf16r(o_full - o) if o_lo else torch.zeros_like(o)
    delta = (do * (o + olo)).sum(-1)
    if fwd is not None:
        d = q.shape[-1]
        delta, lse2 = (do * (fwd["o"] + fwd["olo"])[..., :d].double()).sum(-1), fwd["lse2"].double()
    dp = do @ v.transpose(-1, -2) - delta[..., None]
    zero = torch.zeros_like(dp)
    ds = torch.where(fl | ~Am, zero, torch.exp2(s2 - lse2[..., None]) * dp)
    dq = torch.where(fl, torch.zeros_like(q), bf16r((bf16r(ds) @ k) * sc32))
    kk = bf16r(k.float() * np.float32(c_sc))
    s2k = torch.where(fl, zero, q @ kk.transpose(-1, -2)).masked_fill(~Am, -math.inf)
    pk = torch.exp2(s2k - lse2[..., None])
    dsk = torch.where(fl | ~Am, zero, pk * dp)
    dv = bf16r(bf16r(pk).transpose(-1, -2) @ do)
    dk = bf16r((bf16r(dsk).transpose(-1, -2) @ q) * sc32)
    return dict(o=o, olo=olo, lse=lse2 * LN2, delta=delta, dq=dq, dk=dk, dv=dv)


def naive(q, k, v, do, ks, ke, scale):
    """the same operation by explicit loops over (b, h, row) in fp64 - the CPU test's independent restatement of ref64"""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    B, H, Nq, d = q.shape
    Nk = k.shape[2]
    ks, ke = torch.as_tensor(ks).long(), torch.as_tensor(ke).long()
    out = dict(o=torch.zeros(B, H, Nq, d, dtype=torch.float64), lse=torch.zeros(B, H, Nq, dtype=torch.float64),
               delta=torch.zeros(B, H, Nq, dtype=torch.float64), dq=torch.zeros(B, H, Nq, d, dtype=torch.float64),
               dk=torch.zeros(B, H, Nk, d, dtype=torch.float64), dv=torch.zeros(B, H, Nk, d, dtype=torch.float64))
    for b in range(B):
        for i in range(Nq):
            a, e = (int(ks[b]), int(ke[b])) if ks.dim() == 1 else (int(ks[b, i]), int(ke[b, i]))
            e = min(e, Nk)
            empty = e <= a
            if empty:
                a, e = 0, Nk
            for h in range(H):
                s = torch.zeros(e - a, dtype=torch.float64) if empty else (k[b, h, a:e] @ q[b, h, i]) * scale
                p = torch.softmax(s, 0)
                o = p @ v[b, h, a:e]
                out["o"][b, h, i] = o
                out["lse"][b, h, i] = torch.logsumexp(s, 0)
                dl = (do[b, h, i] * o).sum()
                out["delta"][b, h, i] = dl
                out["dv"][b, h, a:e] += p[:, None] * do[b, h, i]
                if not empty:
                    ds = p * (v[b, h, a:e] @ do[b, h, i] - dl)
                    out["dq"][b, h, i] = ds @ k[b, h, a:e] * scale
                    out["dk"][b, h, a:e] += ds[:, None] * q[b, h, i] * scale
    return out


def row_rms(x):
    return x.double().pow(2).mean(-1).sqrt()


def envelope(model, ref, factor):
    """per output row (the values of one head): factor x RMS(model - ref) + 2^-9 x RMS(ref)"""
    return factor * row_rms(model - ref) + 2.0 ** -9 * row_rms(ref)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    q: torch.Tensor                     # [B, H, Nq, d] fp64 holding bf16 values (d: the head's real dimension)
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor
    ks: torch.Tensor                    # int64 [B] (one interval per sample) or [B, Nq]
    ke: torch.Tensor
    scale: float
    exact: bool = False                 # Q = 0 and index codes in V / dO
    o_lo: bool = False
    seg: Optional[list] = None          # row groups per sample [[(first, count), ...], ...]
    seg_bad: Optional[list] = None
    splits: tuple = ()                  # also run through the split-key forward with these kv_splits
    hd: Optional[tuple] = None          # (pitch, real dimension given in the upper bits?) for the other-head-dim entries
    group: str = ""

    @property
    def dims(self):
        B, H, Nq, d = self.q.shape
        return B, H, Nq, self.k.shape[2], d


def mask(kind, B, Nq, Nk, g):
    """(ks, ke) int64 of a mask kind; per-sample kinds return [B], the others [B, Nq].  0 <= ks; ke any value >= 0."""
    ri = lambda lo, hi, shape=(B, Nq): torch.randint(lo, max(hi, lo + 1), shape, generator=g)
    if kind == "full":
        return torch.zeros(B, dtype=torch.int64), torch.full((B,), Nk, dtype=torch.int64)
    if kind == "sample":                                          # full | ks > 0 | one key
        ks = torch.tensor([0, min(5, Nk - 1), Nk // 2])[:B]
        return ks, torch.tensor([Nk, Nk, Nk // 2 + 1])[:B]
    if kind == "sample_edge":                                     # ke > Nk (clamped) | ks >= Nk (empty) | ends one short of Nk
        return torch.tensor([0, Nk, min(1, Nk - 1)])[:B], torch.tensor([Nk + 9, Nk + 5, max(Nk - 1, 1)])[:B]
    if kind == "sample_empty":
        return torch.full((B,), 3, dtype=torch.int64), torch.full((B,), 3, dtype=torch.int64)
    if kind == "ragged":
        ks = ri(0, Nk)
        ke = ks + ri(0, Nk + 1)                                   # some run past Nk, some are empty
    elif kind.startswith("align"):
        a = int(kind[5:])
        nt = (Nk + a - 1) // a
        ks = a * ri(0, nt)
        ke = ks + a * ri(1, nt + 1)
    elif kind == "one_tile":                                      # wholly inside one 64-key tile
        t = ri(0, (Nk + 63) // 64)
        lo = ri(0, 63)
        ks = (64 * t + lo).clamp(max=Nk - 1)
        ke = torch.minimum(ks + 1 + ri(0, 64), 64 * (ks // 64) + 64)
    elif kind == "edges":                                         # both ends on a tile edge, or one key either side of it
        nt = (Nk + 63) // 64
        ks = (64 * ri(0, nt) + ri(-1, 2)).clamp(min=0)
        ke = (64 * ri(1, nt + 1) + ri(-1, 2)).clamp(min=0)
    elif kind.startswith("window"):                               # equal-length sliding windows: every row has n keys
        n = min(int(kind[6:]), Nk)
        ks = (torch.arange(Nq) * 7 % (Nk - n + 1))[None].expand(B, -1).clone()
        ke = ks + n
    elif kind == "beyond":
        ks = ri(0, Nk + 20)                                       # ks >= Nk: empty
        ke = ks + ri(1, Nk + 40)                                  # ke > Nk: clamped
    elif kind == "all_empty":
        ks = ri(0, Nk + 3)
        ke = ks.clone()
    else:
        raise KeyError(kind)
    return ks, ke


def empties(ks, ke, where):
    """empty intervals at rows: 'iso' (isolated), 'wave' (rows 32..63), 'wg' (rows 128..255), applied in place"""
    Nq = ks.shape[1]
    if "iso" in where:
        ke[:, 5 % Nq::11] = ks[:, 5 % Nq::11]
    if "wave" in where and Nq >= 64:
        ke[:, 32:64] = ks[:, 32:64]
    if "wg" in where and Nq >= 256:
        ke[0, 128:256] = ks[0, 128:256]
        ke[1:, 0:128] = ks[1:, 0:128]
    return ks, ke


def exact_case(name, B, H, Nq, Nk, kind, empty="", d=64, **kw):
    g = gen("exact", name)
    ks, ke = mask(kind, B, Nq, Nk, g)
    if empty:
        ks, ke = empties(ks, ke, empty)
    q = torch.zeros(B, H, Nq, d, dtype=torch.float64)
    k = randn_bf16((B, H, Nk, d), "k", name)
    v = torch.zeros(B, H, Nk, d, dtype=torch.float64)
    do = torch.zeros(B, H, Nq, d, dtype=torch.float64)
    v[..., :64] = code(Nk)
    do[..., :64] = code(Nq)
    return Case(name, q, k, v, do, ks, ke, d ** -0.5, exact=True, **kw)


def spike_do(do):
    """input (c): a few rows 100 x larger than the rest, and rows of zeros"""
    do = do.clone()
    do[:, :, 3::17] = bf16r(do[:, :, 3::17] * 100)
    do[:, :, 5::13] = 0
    return do


def no_single_key(ks, ke, Nk):
    """Widen one-key intervals to two keys.  A one-key row has dS = p (dP - delta) = 0 in exact arithmetic, so its reference dQ
    row is zero and its envelope empty, while a kernel's fp32 dP - delta leaves summation-order noise there: the float cases
    keep such rows out (the exact cases cover them)."""
    one = (ke.clamp(max=Nk) - ks) == 1
    return torch.where(one & (ks > 0), ks - 1, ks), torch.where(one & (ks == 0), ke + 1, ke)


def random_case(name, B, H, Nq, Nk, kind, empty="", d=64, **kw):
    g = gen("random", name)
    ks, ke = mask(kind, B, Nq, Nk, g)
    if empty:
        ks, ke = empties(ks, ke, empty)
    ks, ke = no_single_key(ks, ke, Nk)
    q, k, v = (randn_bf16((B, H, n, d), t, name) for t, n in (("q", Nq), ("k", Nk), ("v", Nk)))
    return Case(name, q, k, v, spike_do(randn_bf16((B, H, Nq, d), "do", name)), ks, ke, d ** -0.5, **kw)


DYNAMICS = ("ascend", "descend", "late_jump", "early_jump", "offset_pos", "offset_neg", "offset_pos_var", "offset_neg_var", "halves")
SCORE_COL = 5


def dynamics_targets(kind, Nk):
    """exp2-domain score of key j for a query whose only non-zero entry is 1"""
    j = torch.arange(Nk, dtype=torch.float64)
    t = torch.div(j, 64, rounding_mode="floor")
    jump0 = 64 * (max(Nk - 48, 0) // 64) + 7                   # 7 keys into the last tile that has at least 48 keys behind it
    if kind == "ascend":
        return 10 * t + 0.0625 * (j % 64)
    if kind == "descend":
        return -10 * t - 0.0625 * (j % 64)
    if kind == "late_jump":                       # flat, then + 40 part-way through a late tile (after the fast path began)
        return torch.where(j >= jump0, 40.0, 0.0)
    if kind == "early_jump":                      # behind every partial interval's start, so every row sees all eight keys
        return torch.where((j >= 40) & (j < 48), 40.0, 0.0)
    if kind.startswith("offset"):
        off = 150.0 if "pos" in kind else -150.0
        return off + (1.0 * (j % 3) if kind.endswith("var") else 0 * j)
    if kind == "halves":                          # the two 32-key halves of a tile differ by 12 > FWD_TAU, alternating per tile
        return torch.where(((j % 64) >= 32) ^ (t % 2 == 1), 12.0, 0.0)
    raise KeyError(kind)


def dynamics_case(name, B, H, Nq, Nk, dyn, kind, **kw):
    """input (b): Q rows with one non-zero column (64, 64, 32, -64 by row: the negative rows see the mirrored dynamics), K's entry
    in that column 1/8 of the target score (at most ~19: a K column of 1200 would put the whole dQ row error into the one scalar
    1200 x sum of the dS roundings, and a row-wise RMS criterion on one random scalar is a coin toss), scale chosen so that
    scale * log2e = 1/8 exactly in fp32: the pre-scaling is exact."""
    g = gen("dyn", name)
    ks, ke = mask(kind, B, Nq, Nk, g)
    q = torch.zeros(B, H, Nq, 64, dtype=torch.float64)
    q[..., SCORE_COL] = torch.tensor([64.0, 64.0, 32.0, -64.0], dtype=torch.float64)[torch.arange(Nq) % 4]
    k = randn_bf16((B, H, Nk, 64), "k", name)
    k[..., SCORE_COL] = bf16r(dynamics_targets(dyn, Nk) / 8)
    v = randn_bf16((B, H, Nk, 64), "v", name)
    return Case(name, q, k, v, spike_do(randn_bf16((B, H, Nq, 64), "do", name)), ks, ke, pow2_scale(0.125), **kw)


def partial_ends(B, Nq, Nk, g):
    """per-row intervals that start inside the first key tile and end inside the last one: the forward's seeded / fast path
    switches on after a partial tile"""
    ks = torch.randint(0, min(40, Nk), (B, Nq), generator=g)
    ke = Nk - torch.randint(0, min(40, Nk), (B, Nq), generator=g)
    return ks, ke


def seg_intervals(groups, N, g, bad=None):
    """per-row (ks, ke) of row groups: a group's rows attend the group; tail rows get a group's interval, an empty one or a random
    one; samples flagged in `bad` get ragged intervals that are NOT their groups"""
    B = len(groups)
    ks, ke = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, dtype=torch.int64)
    for b in range(B):
        end = 0
        for s0, c in groups[b]:
            ks[b, s0:s0 + c], ke[b, s0:s0 + c] = s0, s0 + c
            end = max(end, s0 + c)
        for i in range(end, N):
            j = int(torch.randint(0, len(groups[b]) + 2, (1,), generator=g))
            if j < len(groups[b]) and groups[b][j][1] > 0:
                ks[b, i], ke[b, i] = groups[b][j][0], groups[b][j][0] + groups[b][j][1]
            elif j == len(groups[b]):
                ks[b, i], ke[b, i] = 7, 7
            else:
                ks[b, i], ke[b, i] = 3, max(end, 4)
        if bad and bad[b]:
            ks[b] = torch.randint(0, N, (N,), generator=g)
            ke[b] = ks[b] + torch.randint(0, N // 2, (N,), generator=g)
    return ks, ke


def seg_case(name, H, N, groups, bad=None, exact=True):
    B = len(groups)
    base = (exact_case if exact else random_case)(name, B, H, N, N, "ragged")
    base.ks, base.ke = seg_intervals(groups, N, gen("seg", name), bad)
    if not exact:
        assert not ((base.ke.clamp(max=N) - base.ks) == 1).any()
    base.seg, base.seg_bad = groups, bad
    return base


# (Nq, Nk, mask kind, empty rows): Nq from {1, 31, 32, 33, 127, 128, 129, 257}, Nk from {1, 63, 64, 65, 127, 128, 129, 191, 192,
# 193, 257, 321} - 1 to 6 key tiles (the forward ring has 3 stages, the dK / dV ring 4, over 64-row tiles of the other axis),
# partial last tiles on both axes, every mask kind on at least one multi-tile shape
GEOMETRY = [
    (1, 1, "sample", ""), (1, 64, "ragged", ""), (1, 321, "edges", ""), (31, 63, "ragged", "iso"), (31, 129, "sample", ""),
    (32, 64, "sample_edge", ""), (32, 65, "edges", ""), (32, 192, "align32", ""), (33, 1, "ragged", ""), (33, 127, "one_tile", ""),
    (33, 193, "ragged", "iso"), (33, 257, "window33", ""), (127, 63, "window17", ""), (127, 128, "align64", "iso"),
    (127, 191, "edges", "wave"), (127, 321, "sample", ""), (128, 64, "full", ""), (128, 128, "window64", ""),
    (128, 129, "beyond", ""), (128, 192, "one_tile", "wave"), (128, 257, "align128", ""), (128, 321, "ragged", "wave"),
    (129, 65, "sample_edge", ""), (129, 127, "ragged", "iso wave"), (129, 193, "window129", ""), (129, 257, "edges", ""),
    (129, 321, "all_empty", ""), (257, 1, "sample", ""), (257, 63, "beyond", ""), (257, 128, "sample_empty", ""),
    (257, 191, "align32", "wg"), (257, 192, "ragged", "wg iso"), (257, 257, "window40", ""), (257, 321, "one_tile", "wg"),
    (257, 321, "full", ""), (64, 257, "window1", ""),
]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, (Nq, Nk, kind, empty) in enumerate(GEOMETRY):
        B = 3 if kind.startswith("sample") else 2
        c = exact_case(f"geo-{Nq}x{Nk}-{kind}{'-' + empty.replace(' ', '+') if empty else ''}", B, 2 + i % 2, Nq, Nk, kind, empty,
                       o_lo=i % 2 == 0, group="geometry")
        if (Nq, Nk, kind) in ((33, 257, "window33"), (129, 65, "sample_edge"), (128, 321, "ragged"), (257, 192, "ragged"), (1, 321, "edges")):
            c.splits = (2, 3, 5, 16)
        out.append(c)
    # row groups: groups of 1, 127, 128, 129 and 0 rows, with and without a tail, seg_bad samples, one group over everything
    out += [
        seg_case("seg-385-notail", 2, 385, [[(0, 1), (1, 127), (128, 128), (256, 129)], [(0, 129), (129, 0), (129, 128), (257, 128)]]),
        seg_case("seg-300-tail", 3, 300, [[(0, 127), (127, 0), (127, 129)], [(0, 1), (1, 128), (129, 127)]]),
        seg_case("seg-257-one", 2, 257, [[(0, 257)], [(0, 257)]]),
        seg_case("seg-300-bad", 2, 300, [[(0, 127), (127, 129)], [(0, 128), (128, 100)], [(0, 300), (300, 0)]], bad=[0, 1, 0]),
        seg_case("seg-300-random", 2, 300, [[(0, 127), (127, 0), (127, 129)], [(0, 2), (2, 128), (130, 126)]], exact=False),
    ]
    for c in out[-5:]:
        c.group = "seg"
    # other head dimensions: 32-row tiles, so 31 / 32 / 33 on the key axis too
    for j, (Nq, Nk, kind, empty) in enumerate([(33, 31, "ragged", "iso"), (129, 32, "sample", ""), (128, 33, "edges", ""),
                                                (257, 193, "ragged", "wave wg"), (127, 129, "window31", ""), (32, 65, "beyond", "")]):
        for d, pitch, real in ((68, 96, True), (68, 128, False), (96, 96, False), (68, 128, True)):
            if real and d == 68 and pitch == 128 and j % 2:
                continue
            B = 3 if kind.startswith("sample") else 2
            out.append(exact_case(f"hd{d}p{pitch}{'r' if real else ''}-{Nq}x{Nk}-{kind}", B, 2, Nq, Nk, kind, empty, d=d,
                                  hd=(pitch, real), o_lo=j % 2 == 0, group="hd"))
    for d, pitch, real in ((68, 96, True), (68, 128, False), (96, 96, False)):
        out.append(random_case(f"hd{d}p{pitch}{'r' if real else ''}-129x193-random", 2, 2, 129, 193, "ragged", "iso", d=d,
                               hd=(pitch, real), o_lo=True, group="hd"))
    # (a) N(0, 1) with ragged, block and per-sample masks, (c) folded into every dO
    for i, (Nq, Nk, kind, empty) in enumerate([(129, 193, "ragged", "iso"), (257, 321, "align64", "wave"), (128, 257, "sample", ""),
                                                (33, 65, "edges", ""), (257, 129, "ragged", "wg"), (127, 191, "full", ""),
                                                (1, 127, "ragged", ""), (129, 63, "sample", "")]):
        out.append(random_case(f"rand-{Nq}x{Nk}-{kind}", 3 if kind.startswith("sample") else 2, 2, Nq, Nk, kind, empty,
                               o_lo=i % 2 == 0, splits=(2, 5) if i < 3 else (), group="random"))
    # (b) softmax dynamics, on a full mask and on per-row masks with partial first / last tiles, also through the split forward
    for i, dyn in enumerate(DYNAMICS):
        for Nq, Nk, kind in ((129, 321, "partial"), (33, 257, "full"), (128, 192, "partial")):
            c = dynamics_case(f"dyn-{dyn}-{Nq}x{Nk}-{kind}", 2, 2, Nq, Nk, dyn, "full", o_lo=i % 2 == 1, group="dynamics",
                              splits=(3,) if Nk == 321 else ())
            if kind == "partial":
                c.ks, c.ke = partial_ends(2, Nq, Nk, gen("partial", c.name))
            out.append(c)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_names(pred=lambda c: True):
    return [c.name for c in cases() if pred(c)]


def get(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref64, model64) of a case, computed once and shared by every test that needs it (read-only)"""
    c = get(name)
    return ref64(c.q, c.k, c.v, c.do, c.ks, c.ke, c.scale), model64(c.q, c.k, c.v, c.do, c.ks, c.ke, c.scale, c.o_lo)


# ---- what the exact cases must show ----------------------------------------------------------------------------------------------
def exact_counts(c):
    """integer truths of an exact case: n[b, q] keys per row, fwd[b, q, 64] = attended keys per code column, bwd[b, j, 64] =
    attending queries per code column (all rows of a key share n where `n_uniform`), dv[b, j, 64] = sum_i code_i / n_i"""
    B, H, Nq, Nk, _ = c.dims
    A, _ = intervals(c.ks, c.ke, Nq, Nk)
    Ad = A.double()
    n = A.sum(-1)
    fwd = Ad @ code(Nk)
    bwd = Ad.transpose(-1, -2) @ code(Nq)
    dv = (Ad / n[..., None].double()).transpose(-1, -2) @ code(Nq)
    return dict(n=n, fwd=fwd, bwd=bwd, dv=dv, n_uniform=bool((n == n.flatten()[0]).all()))
