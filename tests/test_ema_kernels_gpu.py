"""`ego_ema_update` / `ego_swap_f32` (csrc/optim.hip) through `ops`: exact cases against a host result, a per-element bound
for general decays against fp64 on the same fp32 operands, bit-for-bit exchange, refusals.

Every buffer under test sits between guard elements of a sentinel; guards and the read-only operand must come back unchanged.
Sizes: the issue's list (empty, below / at / above one 16-byte vector, around one 256-thread block of vectors, three blocks
plus a tail element) and one size past the capped grid (4096 blocks x 256 threads x 4 elements), where a thread walks more than
one vector."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from egom2p_amd import ops  # noqa: E402

DEV = "cuda:0"
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 + 1]
STRIDED = 2 * 4096 * 256 * 4 + 5          # twice the capped grid's reach, plus a vector and a tail element
SENT_BITS = 0x7FC00ABC                    # a NaN with a payload, compared as int32
BACK = 64


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _ranged(n, seed):
    """random floats with magnitude in [2^-10, 2^10): (1 + u) * 2^k, k in [-10, 9], random sign"""
    g = _gen(seed)
    m = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    k = torch.randint(-10, 10, (n,), generator=g).double()
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (s * m * torch.pow(torch.tensor(2.0, dtype=torch.float64), k)).float()


def _ints(n, seed):
    return torch.randint(-4096, 4097, (n,), generator=_gen(seed)).float()


def _guarded(values, front):
    """values (host fp32) between `front` and BACK sentinel elements on the device: (whole, view).  front = 64: the view starts 256
    bytes into the allocation; front = 4: 16 bytes into it."""
    n = values.numel()
    whole = torch.full((front + n + BACK,), SENT_BITS, dtype=torch.int32, device=DEV)
    whole[front:front + n].copy_(_bits(values).to(DEV))                  # an integer copy: every bit pattern arrives as it is
    return whole, whole[front:front + n].view(torch.float32)


def _guards_intact(whole, front, n):
    g = torch.cat([whole[:front], whole[front + n:]])
    return bool((g == SENT_BITS).all().item()) and g.numel() == front + BACK


def _bits(t):
    return t.contiguous().view(torch.int32)


EXACT = {
    # decay: (operand maker, host result).  0.5: both products are exact, the fp64 sum of the halves is exact (exponents differ
    # by at most 20), so the correctly rounded fp32 sum is unique - with or without a contracted fma.  0.75: integer operands up
    # to 4096, every intermediate is exact in fp32.  0 / 1: a copy of p / no change.
    0.5: (_ranged, lambda e, p: (0.5 * e.double() + 0.5 * p.double()).float()),
    0.75: (_ints, lambda e, p: 0.75 * e + 0.25 * p),
    0.0: (_ranged, lambda e, p: p.clone()),
    1.0: (_ranged, lambda e, p: e.clone()),
}


@pytest.mark.parametrize("decay", sorted(EXACT))
def test_ema_update_exact_cases(decay):
    make, host = EXACT[decay]
    for n in SIZES + [STRIDED]:
        for front in ((64, 4) if n != STRIDED else (4,)):
            e0, p0 = make(n, 100 + n % 977), make(n, 200 + n % 977)
            we, e = _guarded(e0, front)
            wp, p = _guarded(p0, front)
            assert e.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
            ops.ema_update(e, p, decay)
            want = host(e0, p0)
            assert torch.equal(e.cpu(), want), (decay, n, front)
            assert torch.equal(_bits(p).cpu(), _bits(p0)), (decay, n, front)          # p is read-only
            assert _guards_intact(we, front, n) and _guards_intact(wp, front, n), (decay, n, front)


@pytest.mark.parametrize("decay", [0.9, 0.999, 0.9999])
def test_ema_update_general_decay_within_the_rounding_bound(decay):
    """Reference: fp64 arithmetic on the same fp32 operands and the same two fp32 factors.  Two product roundings and one sum
    rounding (or one product and one fma rounding) give |err| <= 2^-23 (|d e| + |omd p|); 1.01 x that is allowed."""
    n = 4 * 256 * 3 + 1
    d32 = torch.tensor(decay, dtype=torch.float32)                       # the factors as ops.ema_update hands them over
    omd32 = torch.tensor(1.0 - decay, dtype=torch.float32)
    e0, p0 = _ranged(n, 7), _ranged(n, 8)
    we, e = _guarded(e0, 64)
    wp, p = _guarded(p0, 64)
    ops.ema_update(e, p, decay)
    de, op = d32.double() * e0.double(), omd32.double() * p0.double()
    err = (e.cpu().double() - (de + op)).abs()
    bound = 1.01 * 2.0 ** -23 * (de.abs() + op.abs())
    worst = float((err / bound).max())
    print(f"decay {decay}: worst error / bound {worst:.3f}")
    assert (err <= bound).all(), worst
    assert torch.equal(_bits(p).cpu(), _bits(p0)) and _guards_intact(we, 64, n) and _guards_intact(wp, 64, n)


@pytest.mark.parametrize("decay", [0.9, 0.999, 0.9999])
def test_ema_update_chain_stays_within_the_accumulated_bound(decay):
    """200 updates from 0 toward a constant p against the fp64 recursion with the same fp32 factors.  Accumulated bound:
    B' = d B + 1.01 x 2^-23 (d (|r| + B) + omd |p|), the per-update bound at the largest value the average can have.  The start
    at 0 keeps the average - and so the bound - small against p: a kernel that forms 1 - decay itself in fp32 is off by
    1.7e-4 x (1 - decay) |p| per update at 0.9999 and leaves the bound (checked below on the host)."""
    n, steps = 1025, 200
    d = float(torch.tensor(decay, dtype=torch.float32))
    omd = float(torch.tensor(1.0 - decay, dtype=torch.float32))
    p0 = _ranged(n, 21)
    we, e = _guarded(torch.zeros(n), 64)
    wp, p = _guarded(p0, 64)
    r, B = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    naive = torch.zeros(n)                                                # fp32 recursion with the factor formed in fp32
    omd_naive = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(decay, dtype=torch.float32)
    for _ in range(steps):
        ops.ema_update(e, p, decay)
        B = d * B + 1.01 * 2.0 ** -23 * (d * (r.abs() + B) + omd * p0.double().abs())
        r = d * r + omd * p0.double()
        naive = torch.tensor(decay, dtype=torch.float32) * naive + omd_naive * p0
    err = (e.cpu().double() - r).abs()
    print(f"decay {decay}: worst chained error / bound {float((err / B).max()):.3f}")
    assert (err <= B).all()
    assert torch.equal(_bits(p).cpu(), _bits(p0)) and _guards_intact(we, 64, n) and _guards_intact(wp, 64, n)
    if decay == 0.9999:
        assert ((naive.double() - r).abs() > B).all()                    # the check has the power the issue asks of it


def _patterns(n, seed):
    """random 32-bit patterns; the special ones (quiet / signalling NaNs with payloads, infinities, -0.0, denormals) lead"""
    t = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=_gen(seed), dtype=torch.int64).to(torch.int32)
    special = [0x7FC00001, 0x7F800001, -0x400000 + 5, 0x7F800000, -0x800000, -2 ** 31, 0x00000001, -2 ** 31 + 0x7FFFFF, 0]
    k = min(n, len(special))
    t[:k] = torch.tensor(special[:k], dtype=torch.int64).to(torch.int32)
    return t


def test_swap_moves_bit_patterns_and_twice_is_the_identity():
    for n in SIZES + [STRIDED]:
        for front in ((64, 4) if n != STRIDED else (4,)):
            a0, b0 = _patterns(n, 300 + n % 977), _patterns(n, 400 + n % 977).flip(0)
            wa, a = _guarded(a0.view(torch.float32), front)
            wb, b = _guarded(b0.view(torch.float32), front)
            assert torch.equal(_bits(a).cpu(), a0)                       # the copy in kept the bits
            ops.swap_f32(a, b)
            assert torch.equal(_bits(a).cpu(), b0) and torch.equal(_bits(b).cpu(), a0), (n, front)
            assert _guards_intact(wa, front, n) and _guards_intact(wb, front, n), (n, front)
            ops.swap_f32(a, b)
            assert torch.equal(_bits(a).cpu(), a0) and torch.equal(_bits(b).cpu(), b0), (n, front)
            assert _guards_intact(wa, front, n) and _guards_intact(wb, front, n), (n, front)


def test_refusals_leave_the_buffers_alone():
    n = 1024
    buf0 = _ranged(2 * n + 8, 5)
    buf = buf0.to(DEV)
    other0 = _ranged(n, 6)
    other = other0.to(DEV)
    bad = [
        ("misaligned ema", lambda: ops.ema_update(buf[1:1 + n], other, 0.5)),
        ("misaligned p", lambda: ops.ema_update(other, buf[1:1 + n], 0.5)),
        ("ema is p", lambda: ops.ema_update(other, other, 0.5)),
        ("overlap", lambda: ops.ema_update(buf[:n], buf[n // 2:n // 2 + n], 0.5)),
        ("overlap by one vector", lambda: ops.ema_update(buf[n - 4:2 * n - 4], buf[:n], 0.5)),
        ("decay 1.5", lambda: ops.ema_update(buf[:n], other, 1.5)),
        ("decay -0.1", lambda: ops.ema_update(buf[:n], other, -0.1)),
        ("decay nan", lambda: ops.ema_update(buf[:n], other, float("nan"))),
        ("swap misaligned", lambda: ops.swap_f32(buf[1:1 + n], other)),
        ("swap a is b", lambda: ops.swap_f32(other, other)),
        ("swap overlap", lambda: ops.swap_f32(buf[:n], buf[n // 2:n // 2 + n])),
        ("lengths differ", lambda: ops.ema_update(buf[:n], other[:n - 4], 0.5)),
    ]
    for what, call in bad:
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf).cpu(), _bits(buf0)) and torch.equal(_bits(other).cpu(), _bits(other0)), what
    ops.ema_update(buf[:n], buf[n:2 * n], 0.5)                            # adjacent ranges are fine
    assert torch.equal(buf[:n].cpu(), (0.5 * buf0[:n].double() + 0.5 * buf0[n:2 * n].double()).float())
