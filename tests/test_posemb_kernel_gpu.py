"""ego_posemb_grad - the gradient of learned positional tables - against torch references on the GPU.

dpos[m][p, :D] (+)= sum over the samples b, ascending, of (dx + d2)[row of sample b with slot m, local p].  An exact case (integer
data: every partial sum is exact in fp32, so the result is THE sum, bit for bit), an fp64 case held per element to the bound of a
B-term fp32 sum of two-term addends, (B + 1) * 2^-24 * sum |terms| (derived: one rounding per addend dx + d2, one per addition of the
running sum, each at most 2^-24 of a partial sum that is at most sum |terms|), padded pitch, skipped modality / NULL d2, the
summation order (the batch's), and the refusals of include/egom2p_hip.h."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda:0"
B, RPS, NPOS = 3, 40, (30, 64)


def _geometry(sets, seed=0, rps=RPS):
    """slot / local [B * rps] from sets[b][m] = positions sample b holds of modality m: a register row (slot -2) in front, the
    kept rows in a seeded random order with padding rows (slot -1) between them."""
    g = torch.Generator().manual_seed(seed)
    slot = torch.full((len(sets), rps), -1, dtype=torch.int32)
    local = torch.zeros(len(sets), rps, dtype=torch.int32)
    for b, per_mod in enumerate(sets):
        pairs = [(m, p) for m, ps in enumerate(per_mod) for p in ps]
        assert len(pairs) < rps
        where = (torch.randperm(rps - 1, generator=g)[:len(pairs)] + 1).tolist()
        slot[b, 0], local[b, 0] = -2, 0
        for (m, p), r in zip(pairs, where):
            slot[b, r], local[b, r] = m, p
    local[slot == -1] = 7                          # whatever a padding row holds: it is skipped
    return slot.reshape(-1).to(DEV), local.reshape(-1).to(DEV)


# overlapping (mod 0: samples 0 and 1 share 5..9), disjoint (mod 1: samples 0 and 1) and empty (sample 2 holds nothing of mod 0)
SETS = [[list(range(0, 10)), list(range(0, 20))],
        [list(range(5, 15)), list(range(40, 60))],
        [[], list(range(10, 15)) + list(range(50, 55))]]


def _ref64(dx, d2, slot, local, D, n_pos=NPOS, rps=RPS):
    """fp64 index_add_ per modality, the samples' terms added in ascending b; also sum |terms| and the held positions"""
    out, mag, held = [], [], []
    for m, n in enumerate(n_pos):
        r = torch.zeros(n, D, dtype=torch.float64, device=dx.device)
        a = torch.zeros_like(r)
        h = torch.zeros(n, dtype=torch.bool, device=dx.device)
        for b in range(slot.numel() // rps):
            rows = torch.arange(b * rps, (b + 1) * rps, device=dx.device)
            rows = rows[slot[rows] == m]
            term = dx[rows, :D].double() + (d2[rows, :D].double() if d2 is not None else 0.0)
            tabs = dx[rows, :D].double().abs() + (d2[rows, :D].double().abs() if d2 is not None else 0.0)
            r.index_add_(0, local[rows].long(), term)
            a.index_add_(0, local[rows].long(), tabs)
            h[local[rows].long()] = True
        out.append(r); mag.append(a); held.append(h)
    return out, mag, held


def _run(dpos, dx, d2, slot, local, D, accumulate, rps=RPS, nb=B):
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    ops.posemb_grad(dpos, dx, d2, slot, local, slot.numel(), rps, nb, D, err, accumulate=accumulate)
    torch.cuda.synchronize()
    return int(err.item())


def test_posemb_grad_exact():
    D = 128
    slot, local = _geometry(SETS)
    g = torch.Generator(device=DEV).manual_seed(1)
    dx = torch.randint(-8, 9, (B * RPS, D), device=DEV, generator=g).float()
    d2 = torch.randint(-8, 9, (B * RPS, D), device=DEV, generator=g).float()
    ref, _, held = _ref64(dx, d2, slot, local, D)
    for acc in (0, 1):
        prior = [torch.randint(-8, 9, (n, D), device=DEV, generator=g).float() + 0.5 for n in NPOS]
        dpos = [p.clone() for p in prior]
        assert _run(dpos, dx, d2, slot, local, D, acc) == 0
        for m in range(2):
            want = ref[m] + (prior[m].double() if acc else 0.0)
            assert torch.equal(dpos[m].double(), want), (acc, m)
            assert (~held[m]).any() and held[m].any()
            if acc:
                assert torch.equal(dpos[m][~held[m]], prior[m][~held[m]])       # untouched positions keep their value
            else:
                assert float(dpos[m][~held[m]].abs().max()) == 0.0                  # ... or are written as zero


def test_posemb_grad_fp64_bound_and_reproducible():
    D = 128
    slot, local = _geometry(SETS)
    g = torch.Generator(device=DEV).manual_seed(2)
    dx = torch.randn(B * RPS, D, device=DEV, generator=g)
    d2 = torch.randn(B * RPS, D, device=DEV, generator=g)
    ref, mag, _ = _ref64(dx, d2, slot, local, D)
    runs = []
    for _ in range(2):
        dpos = [torch.full((n, D), 3.0, device=DEV) for n in NPOS]
        assert _run(dpos, dx, d2, slot, local, D, 0) == 0
        runs.append(dpos)
    worst = 0.0
    for m in range(2):
        assert torch.equal(runs[0][m], runs[1][m])
        bound = (B + 1) * 2.0 ** -24 * mag[m]
        diff = (runs[0][m].double() - ref[m]).abs()
        worst = max(worst, float((diff / bound.clamp_min(1e-300)).max()))
        assert bool((diff <= bound).all()), m
    print("posemb fp64: worst |got - ref| / bound =", worst)


@pytest.mark.parametrize("D,ld", [(1020, 1024), (126, 128), (2046, 2048), (129, 132), (3, 4)])
def test_posemb_grad_padded_pitch(D, ld):
    """D columns of an ld-pitch row; D need not be a multiple of 4 (dim 2046 in rows of 2048): the columns behind D & ~3 are a
    scalar tail"""
    slot, local = _geometry(SETS)
    g = torch.Generator(device=DEV).manual_seed(3)
    dx = torch.randint(-8, 9, (B * RPS, ld), device=DEV, generator=g).float()
    d2 = torch.randint(-8, 9, (B * RPS, ld), device=DEV, generator=g).float()
    ref, _, _ = _ref64(dx, d2, slot, local, D)
    for acc in (0, 1):
        dpos = [torch.full((n, ld), -77.0, device=DEV) for n in NPOS]
        assert _run(dpos, dx, d2, slot, local, D, acc) == 0
        for m in range(2):
            assert torch.equal(dpos[m][:, :D].double(), ref[m] + (-77.0 if acc else 0.0))
            assert bool((dpos[m][:, D:] == -77.0).all())                            # columns [D, ld) stay as they were


def test_posemb_grad_skipped_modality_and_null_d2():
    D = 128
    slot, local = _geometry(SETS)
    g = torch.Generator(device=DEV).manual_seed(4)
    dx = torch.randint(-8, 9, (B * RPS, D), device=DEV, generator=g).float()
    ref, _, _ = _ref64(dx, None, slot, local, D)
    for fixed in (0, 1):
        dpos = [torch.full((n, D), 5.0, device=DEV) for n in NPOS]
        arg = [NPOS[m] if m == fixed else dpos[m] for m in range(2)]               # a fixed table: its position count only
        assert _run(arg, dx, None, slot, local, D, 0) == 0
        assert torch.equal(dpos[1 - fixed].double(), ref[1 - fixed])
        assert bool((dpos[fixed] == 5.0).all())
    assert _run([NPOS[0], NPOS[1]], dx, None, slot, local, D, 0) == 0              # every table fixed: nothing to do


def test_posemb_grad_sums_in_batch_order():
    """every sample holds every position of modality 0: a three-term sum per element, whose bits depend on the order"""
    D = 128
    sets = [[list(range(30)), []] for _ in range(B)]
    slot, local = _geometry(sets, seed=5)
    g = torch.Generator(device=DEV).manual_seed(5)
    dx = torch.randn(B * RPS, D, device=DEV, generator=g) * torch.tensor([1.0, 1e3, 1e-3], device=DEV).repeat_interleave(RPS)[:, None]

    def run(order):
        rows = torch.cat([torch.arange(b * RPS, (b + 1) * RPS, device=DEV) for b in order])
        dpos = [torch.zeros(n, D, device=DEV) for n in NPOS]
        assert _run(dpos, dx[rows].contiguous(), None, slot[rows].contiguous(), local[rows].contiguous(), D, 0) == 0
        return dpos[0]

    first, other, again = run([0, 1, 2]), run([2, 0, 1]), run([0, 1, 2])
    assert torch.equal(first, again)
    assert not torch.equal(first, other)
    # the stated order itself: ((0 + t0) + t1) + t2 in fp32
    rows = [torch.arange(b * RPS, (b + 1) * RPS, device=DEV) for b in range(B)]
    want = torch.zeros(30, D, device=DEV)
    for b in range(B):
        r = rows[b][slot[rows[b]] == 0]
        want[local[r].long()] = want[local[r].long()] + dx[r]
    assert torch.equal(first, want)


def _call(**over):
    """ego_posemb_grad on a valid descriptor with fields replaced; returns (rc, err word, tensors kept alive)"""
    D = over.pop("_D", 128)
    slot, local = over.pop("_geo", None) or _geometry(SETS)
    dx = torch.ones(B * RPS + 1, D, device=DEV)
    d2 = torch.ones(B * RPS + 1, D, device=DEV)
    dpos = [torch.zeros(n + 1, D, device=DEV) for n in NPOS]
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    n = ops.posemb_grad_work_ints(B, 2, NPOS)
    assert n == B * sum(NPOS)
    work = torch.empty(n, device=DEV, dtype=torch.int32)
    d = L.PosembGradDesc()
    d.dx, d.d2, d.slot, d.local = dx.data_ptr(), d2.data_ptr(), slot.data_ptr(), local.data_ptr()
    d.rows, d.rows_per_sample, d.B, d.D, d.ld, d.n_mods, d.accumulate = B * RPS, RPS, B, D, D, 2, 0
    for m in range(2):
        d.n_pos[m], d.dpos[m] = NPOS[m], dpos[m].data_ptr()
    d.work, d.work_ints, d.err = work.data_ptr(), n, err.data_ptr()
    for k, v in over.items():
        if k.startswith("dpos"):
            d.dpos[int(k[4:])] = v(dpos[int(k[4:])].data_ptr())
        elif k.startswith("n_pos"):
            d.n_pos[int(k[5:])] = v
        else:
            setattr(d, k, v(getattr(d, k)) if callable(v) else v)
    rc = L.load().ego_posemb_grad(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(err.item()), dpos


def test_posemb_grad_refusals():
    assert _call()[0] == 0
    bad = [dict(dx=None), dict(dx=lambda p: p + 4), dict(d2=lambda p: p + 8), dict(dpos0=lambda p: p + 4), dict(dpos1=lambda p: p + 12),
           dict(slot=None), dict(local=None), dict(work=None), dict(err=None),
           dict(ld=124), dict(ld=130), dict(D=126, ld=126), dict(D=2052, ld=2052), dict(D=0), dict(n_mods=L.MAX_MODS + 1), dict(n_mods=0), dict(n_pos1=0),
           dict(rows=B * RPS + 1), dict(rows=0), dict(B=0), dict(rows_per_sample=0), dict(work_ints=B * sum(NPOS) - 1)]
    for over in bad:
        rc, err, dpos = _call(**over)
        assert rc == 1, over                                   # EGO_ERR_ARG
        assert err == 0 and all(float(t.abs().max()) == 0.0 for t in dpos), over      # a refused call has written nothing
    assert ops.posemb_grad_work_ints(0, 2, NPOS) == 0 and ops.posemb_grad_work_ints(B, L.MAX_MODS + 1, NPOS * 5) == 0


def test_posemb_grad_contract_breaks_raise_err():
    """what the host cannot see: a local outside its table, a slot outside the modalities, one (m, p) twice in a sample - err is
    raised, the offending row (of a duplicate pair: one of the two) is left out, every other position is the sum it should be"""
    D = 128
    for kind in ("local_high", "local_negative", "slot_high", "duplicate"):
        slot, local = _geometry(SETS)
        s2, l2 = slot.clone(), local.clone()
        r = int((slot[:RPS] == 1).nonzero()[0])                # a row of sample 0, modality 1
        if kind == "local_high":
            l2[r] = NPOS[1]
        elif kind == "local_negative":
            l2[r] = -3
        elif kind == "slot_high":
            s2[r] = 2
        else:
            r2 = int((slot[:RPS] == 1).nonzero()[1])
            l2[r2] = l2[r]                                    # sample 0 now holds (1, local[r]) twice
        rc, err, dpos = _call(_geo=(s2, l2))
        assert rc == 0 and err == 2, kind
        keep = torch.ones(B * RPS, dtype=torch.bool, device=DEV)
        keep[r] = False
        if kind == "duplicate":
            keep[r2] = False
        sk = torch.where(keep, s2, torch.full_like(s2, -1))
        ones = torch.ones(B * RPS, D, device=DEV)
        ref, _, _ = _ref64(ones, ones, sk, l2, D)
        for m in range(2):
            got = dpos[m][:NPOS[m]].double()
            if kind == "duplicate" and m == 1:
                p = int(l2[r])
                assert float(got[p, 0]) == float(ref[m][p, 0]) + 2.0       # exactly one of the two rows took part
                got = got.clone(); got[p] = ref[m][p]
            assert torch.equal(got, ref[m]), (kind, m)
            assert float(dpos[m][NPOS[m]:].abs().max()) == 0.0             # nothing behind the table
