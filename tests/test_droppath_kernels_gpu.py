"""The drop-path kernels (egom2p_amd/csrc/droppath.hip) against their host restatements (tests/_droppath_ref.py): the draw bit for bit
against splitmix64 in Python integers, the residual add and the gradient scale bitwise against torch's `R + where(keep, (branch.float()
/ keep_prob).bfloat16().float(), 0)` - the correctly rounded fp32 divide and one bf16 rounding, nothing else."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _droppath_ref as R  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
KPS = [R.keep_prob(r) for r in R.rates(0.1, 0.3, 2, 2, True)[1]] + [R.keep_prob(R.f32(0.1))]      # fp32(1 - rate.item()): 0.8, 0.7, 0.9


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_draw_matches_the_host_restatement_bit_for_bit():
    kps = [R.f32(0.9), R.f32(0.7), R.f32(0.7), R.f32(0.8), 1.0, R.f32(0.5), R.f32(0.7), R.f32(0.9)]
    kp_dev = torch.tensor(kps, dtype=torch.float32, device=DEV)
    seed = 1234567
    tabs = {}
    for counter in (0, 5):
        for B in (1, 3, 64):
            keep = torch.full((8 * B + 16,), 7, dtype=torch.uint8, device=DEV)
            ops.droppath_draw(kp_dev, seed, counter, keep, B)
            got = keep[:8 * B].view(8, B).cpu().tolist()
            assert got == R.draw(kps, B, seed, counter), (counter, B)
            assert bool((keep[8 * B:] == 7).all())                            # nothing behind the table is written
            tabs[counter, B] = got
        # sample b's decision does not depend on the batch size
        assert [row[:3] for row in tabs[counter, 64]] == tabs[counter, 3] and [row[:1] for row in tabs[counter, 64]] == tabs[counter, 1]
    assert tabs[0, 64] != tabs[5, 64]
    assert all(tabs[0, 64][4])                                                # keep_prob 1 keeps every sample
    # a 64-bit seed and counter pass whole
    keep = torch.zeros(8 * 3, dtype=torch.uint8, device=DEV)
    ops.droppath_draw(kp_dev, 2 ** 63 + 11, 2 ** 40 + 3, keep, 3)
    assert keep.view(8, 3).cpu().tolist() == R.draw(kps, 3, 2 ** 63 + 11, 2 ** 40 + 3)


def _keep_tables(B):
    gen = torch.Generator().manual_seed(B)
    mixed = torch.rand(B, generator=gen) < 0.5
    if B > 1:
        mixed[0], mixed[1] = True, False
    return {"mixed": mixed, "all_kept": torch.ones(B, dtype=torch.bool), "all_dropped": torch.zeros(B, dtype=torch.bool)}


@pytest.mark.parametrize("width,ld", [(384, 384), (1020, 1024)])
@pytest.mark.parametrize("rps", [1, 5, 320])
@pytest.mark.parametrize("B", [1, 4])
def test_resid_and_scale_are_bitwise_the_torch_restatement(width, ld, rps, B):
    rows = B * rps
    gen = torch.Generator(device=DEV).manual_seed(width + 7 * rps + B)
    Rm = torch.zeros(rows, ld, device=DEV)
    Rm[:, :width] = torch.randn(rows, width, device=DEV, generator=gen)
    br = torch.zeros(rows, ld, device=DEV, dtype=torch.bfloat16)
    br[:, :width] = (torch.randn(rows, width, device=DEV, generator=gen) * 3).bfloat16()
    for kp in (KPS[2], KPS[1]):                                               # 0.9, 0.7
        for tag, keep in _keep_tables(B).items():
            keep_d = keep.to(DEV).to(torch.uint8)
            keep_rows = keep.to(DEV).repeat_interleave(rps)
            src = br.clone()
            src[~keep_rows] = float("nan")                                    # a dropped sample's branch is not read
            want = torch.zeros(rows, ld, device=DEV)
            want[:, :width] = R.resid(Rm[:, :width], br[:, :width], keep_rows, kp)
            out = torch.full((rows + 1, ld), 3.0, device=DEV)
            ops.droppath_resid(Rm, src, out, keep_d, rows, rps, width, kp)
            assert torch.equal(_bits(out[:rows]), _bits(want)), (tag, kp)
            assert bool((out[:rows, width:] == 0).all()) and bool((out[rows] == 3.0).all())        # pad columns 0, the next row untouched
            # out aliasing R
            alias = Rm.clone()
            ops.droppath_resid(alias, src, alias, keep_d, rows, rps, width, kp)
            assert torch.equal(_bits(alias), _bits(want)), (tag, kp, "alias")
            # the gradient scale: the bf16 form
            wants = torch.zeros(rows, ld, device=DEV, dtype=torch.bfloat16)
            wants[:, :width] = R.scaled(br[:, :width], keep_rows, kp)
            dst = torch.full((rows + 1, ld), 3.0, device=DEV, dtype=torch.bfloat16)
            ops.droppath_scale(src, dst, keep_d, rows, rps, width, kp)
            assert torch.equal(_bits(dst[:rows]), _bits(wants)), (tag, kp, "scale")
            assert bool((dst[:rows, width:] == 0).all()) and bool((dst[rows] == 3.0).all())
            if tag == "all_dropped":
                assert torch.equal(out[:rows], Rm) and not bool(dst[:rows].any())
            if tag == "all_kept":
                assert not torch.equal(out[:rows], Rm)


def test_divide_is_correctly_rounded_over_every_normal_bf16_value():
    """every bf16 value of magnitude in [2^-120, max] through the scale kernel at keep_prob 0.7 and 0.9: the same bits as torch's fp32
    divide + bf16 rounding (quotients stay normal; the largest values overflow to inf in both)"""
    allv = torch.arange(0, 65536, dtype=torch.int32, device=DEV).to(torch.int16).view(torch.bfloat16)
    allv = allv[torch.isfinite(allv.float()) & (allv.float().abs() >= 2.0 ** -120)]
    n = allv.numel() // 8 * 8
    br = allv[:n].view(-1, 8).contiguous()
    rows = br.shape[0]
    keep = torch.ones(1, dtype=torch.uint8, device=DEV)
    rows_kept = torch.ones(rows, dtype=torch.bool, device=DEV)
    for kp in (KPS[1], KPS[2]):
        dst = torch.empty_like(br)
        ops.droppath_scale(br, dst, keep, rows, rows, 8, kp)
        assert torch.equal(_bits(dst), _bits(R.scaled(br, rows_kept, kp)))


def test_arguments_are_checked():
    lib = L.load()
    R_ = torch.zeros(8, 16, device=DEV)
    b = torch.zeros(8, 16, device=DEV, dtype=torch.bfloat16)
    keep = torch.ones(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.EgoHipError):                 # more rows than samples x rows per sample: the keep lookup would leave the table
        ops.droppath_resid(R_, b, R_, keep, 8, 3, 16, 0.9)
    with pytest.raises(L.EgoHipError):
        ops.droppath_scale(b, b.clone(), keep, 8, 3, 16, 0.9)
    with pytest.raises(L.EgoHipError):                 # keep_prob outside (0, 1]
        ops.droppath_resid(R_, b, R_, keep, 8, 4, 16, 0.0)
    with pytest.raises(L.EgoHipError):                 # a pitch below the width rounded up to 8
        ops.droppath_scale(b, torch.zeros(8, 8, device=DEV, dtype=torch.bfloat16), keep, 8, 4, 12, 0.9)
    assert lib.ego_abi_version() == 12
