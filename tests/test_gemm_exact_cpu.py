"""Host-side proof that the REFERENCE of tests/test_gemm_exact_gpu.py is exact, so that a mismatch there is the kernel's:
the value ranges keep every intermediate below 2^24, an fp32 sum of the products is the fp64 product in any order, and the torch
epilogue formulas are the documented roundings (round-to-nearest-even bfloat16, ties included).  No GPU."""
import torch

import _gemm_exact as X


def test_value_ranges_keep_every_intermediate_exact_in_fp32():
    assert X.ACC_MAX == 16 * X.K_MAX == 32768
    assert 16 * X.K_MAX + 64 + 64 == X.WORST < 2 ** 24
    # fp8: sa * sb * acc with power-of-two scales 2^-3 .. 2^3 is n * 2^e with |n| <= 2^15 and -6 <= e <= 6.  In units of
    # min(2^e, 1) the sum with a bias and a residual of at most 64 each is an integer of at most 2^21 + 2^13: below 2^24
    assert X.ACC_MAX * 64 + 128 * 64 < 2 ** 24
    for lo, hi in ((X.OPERAND_LO, X.OPERAND_HI), (X.ADDEND_LO, X.ADDEND_HI)):
        t = X.ints((257, 130), lo, hi, torch.float32, seed=3)
        assert t.min().item() == lo and t.max().item() == hi and torch.equal(t, t.round())
        assert torch.equal(t, X.ints((257, 130), lo, hi, torch.float32, seed=3))           # seeded
        assert not torch.equal(t, X.ints((257, 130), lo, hi, torch.float32, seed=4))
        assert torch.equal(t.to(torch.bfloat16).float(), t)                               # exact in the operand format
    p = X.pitched(X.ints((5, 16), -4, 4, torch.bfloat16), 24, float("nan"))
    assert p.shape == (5, 16) and p.stride(0) == 24 and p._base.shape == (5, 24) and p._base[:, 16:].isnan().all()
    assert not p.isnan().any()


def test_fp32_sums_of_integer_products_equal_fp64_in_any_order():
    M, N, K = 37, 29, X.K_MAX
    A = X.ints((M, K), X.OPERAND_LO, X.OPERAND_HI, torch.float32, seed=1)
    B = X.ints((N, K), X.OPERAND_LO, X.OPERAND_HI, torch.float32, seed=2)
    A[0], B[0] = 4.0, 4.0                       # the worst case: K products of +16 ...
    A[1], B[1] = -4.0, 4.0                      # ... and of -16
    ref = A.double() @ B.double().t()
    assert ref[0, 0].item() == X.ACC_MAX and ref[1, 0].item() == -X.ACC_MAX

    def exact(c32):
        assert c32.dtype == torch.float32
        return torch.equal(c32.double(), ref)

    assert exact(A @ B.t())                                                    # whatever order the host BLAS takes
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(5))
    assert exact(A[:, perm] @ B[:, perm].t())                                  # permuted K
    for step in (32, 64, 128):                                                 # MFMA depth, K-step, fp8 K-tile
        blocks = [A[:, k:k + step] @ B[:, k:k + step].t() for k in range(0, K, step)]
        fwd = torch.zeros(M, N)
        for b in blocks:
            fwd = fwd + b
        assert exact(fwd)
        rev = torch.zeros(M, N)
        for b in reversed(blocks):
            rev = rev + b
        assert exact(rev)
        for splits in (2, 3, 8):                                               # split-K slabs summed afterwards, some of them empty
            per = -(-len(blocks) // splits)
            slabs = [sum(blocks[s * per:(s + 1) * per], torch.zeros(M, N)) for s in range(splits)]
            assert exact(sum(slabs, torch.zeros(M, N)))
    # one product at a time, in fp32, for the worst-case elements
    acc = torch.zeros((), dtype=torch.float32)
    for k in range(K):
        acc = acc + A[0, k] * B[0, k]
    assert acc.item() == X.ACC_MAX


def test_torch_epilogues_are_the_documented_roundings_ties_included():
    # every accumulator value the ranges allow, which holds every tie of every binade (odd integers in [256, 512), 4 n + 2 in
    # [512, 1024), ...), with R and bias cycling through their range
    acc = torch.arange(-X.ACC_MAX, X.ACC_MAX + 1, dtype=torch.float64)
    n = acc.numel()
    R = ((torch.arange(n) * 7) % 129 - 64).to(torch.float32)
    bias = ((torch.arange(n) * 11) % 129 - 64).to(torch.float32)
    got = [f(acc, R, bias).to(torch.float64).tolist() for f in X.EPILOGUES]
    rne, f32 = X.bf16_rne_scalar, X.f32_scalar
    ties = 0
    for i, (a, r, b) in enumerate(zip(acc.tolist(), R.tolist(), bias.tolist())):
        want = (rne(a), a, f32(r + rne(a)), f32(r + rne(f32(a + rne(b)))))
        for e in range(4):
            assert got[e][i] == want[e], (e, a, r, b, got[e][i], want[e])
        ties += int(abs(a) >= 256 and rne(a) != a and abs(rne(a) - a) * 2 == _ulp_bf16(a))
    assert ties > 1000
    # the tie rule itself, on hand-written cases: round half to EVEN
    for x, want in ((257.0, 256.0), (259.0, 260.0), (261.0, 260.0), (263.0, 264.0), (-257.0, -256.0), (-259.0, -260.0),
                    (514.0, 512.0), (518.0, 520.0), (32704.0, 32768.0), (32512.0 + 64.0, 32512.0), (255.0, 255.0), (1.3359375, 1.3359375)):
        assert rne(x) == want, (x, rne(x), want)
        assert X.bf16_rne(torch.tensor([x], dtype=torch.float64)).item() == want


def _ulp_bf16(a):
    e = 0
    a = abs(a)
    while 2 ** (e + 1) <= a:
        e += 1
    return 2.0 ** (e - 7)
