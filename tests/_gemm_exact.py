"""Shared pieces of the exact-arithmetic GEMM conformance tests (tests/test_gemm_exact_gpu.py, tests/test_gemm_exact_cpu.py).

Operands are small integers, so every product is exact in the MFMA and every partial sum is an integer far below 2^24: the fp32
accumulator of a kernel equals the fp64 product in ANY summation order, and every epilogue is one or two deterministic roundings
of it.  The value ranges are fixed here so that the reference stays exact; tests/test_gemm_exact_cpu.py proves that on the host.
Nothing in this module needs a GPU."""
import struct
import zlib

import torch

OPERAND_LO, OPERAND_HI = -4, 4          # GEMM operand elements
ADDEND_LO, ADDEND_HI = -64, 64          # R, bias and the preloaded C0 / C1
K_MAX = 2048                            # longest contraction (NT: K, TN: M)
ACC_MAX = OPERAND_HI * OPERAND_HI * K_MAX                 # |acc| <= 32768
WORST = ACC_MAX + ADDEND_HI + ADDEND_HI                   # acc + bias + R: the largest intermediate of any epilogue


def ints(shape, lo, hi, dtype, seed=0, device="cpu"):
    """Integer-valued tensor, uniform in [lo, hi], from a generator seeded by (shape, range, seed): the same call gives the same
    tensor in every test and on every run."""
    g = torch.Generator(device=device)
    g.manual_seed(zlib.crc32(repr((tuple(shape), lo, hi, seed)).encode()))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=device, dtype=torch.int32).to(dtype)


def pitched(t, ld, fill):
    """View of t's shape into a fresh [rows, ld] buffer whose pad columns [width, ld) hold `fill` (`view._base` is the buffer).
    The base address is whatever torch allocates."""
    rows, width = t.shape
    assert ld >= width
    buf = torch.full((rows, ld), fill, dtype=t.dtype, device=t.device)
    buf[:, :width] = t
    return buf[:, :width]


# ---- the four epilogues of include/egom2p_hip.h, on an exact accumulator (any float dtype holding integers / dyadics) ----------
def bf16_rne(x):
    """round-to-nearest-even to bfloat16, returned as fp32"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def epi_f32(acc, R=None, bias=None):
    return acc.to(torch.float32)


def epi_bf16(acc, R=None, bias=None):
    return acc.to(torch.float32).to(torch.bfloat16)


def epi_resid(acc, R, bias=None):
    return R + bf16_rne(acc)


def epi_bias_resid(acc, R, bias):
    return R + bf16_rne(acc.to(torch.float32) + bf16_rne(bias))


EPILOGUES = (epi_bf16, epi_f32, epi_resid, epi_bias_resid)      # indexed by EGO_EPI_*


# ---- scalar round-to-nearest-even bfloat16 (the CPU test's independent restatement) ----------------------------------------------
def f32_scalar(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bf16_rne_scalar(x):
    """bf16 RNE of a finite Python float that is exactly representable in fp32; returns a Python float"""
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    assert struct.unpack("<f", struct.pack("<I", bits))[0] == x, "not an fp32 value"
    low, keep = bits & 0xFFFF, bits >> 16
    if low > 0x8000 or (low == 0x8000 and (keep & 1)):
        keep += 1                                            # a carry into the exponent is the right result
    return struct.unpack("<f", struct.pack("<I", (keep << 16) & 0xFFFFFFFF))[0]
