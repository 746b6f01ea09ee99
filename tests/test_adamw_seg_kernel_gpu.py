"""`ops.adamw_step_seg` (ego_adamw_step_seg): every segment of the flat buffers with its own lr, weight decay and step count in ONE
launch.  The reference is torch.optim.AdamW on clones, one optimiser per segment; the bar is this kernel family's
(tests/test_step_gate_gpu.py: rel_l2 < 1e-6 per segment), the measured values held to their recorded baselines
(tests/_adamw_seg_bars.py).  The kernel is a trivially parallel stream: what can go wrong is the attribution of a vector to a
segment, so neighbours differ up to 100 x in lr - one misattributed vector misses the bar by orders of magnitude."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _adamw_seg_bars import held  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
B1, B2, EPS = 0.9, 0.95, 1e-8
BAR = 1e-6

# (size, lr, wd, first step, frozen, gap in front): the first segment starts at 0; 4 | 8 and 4092 | 4096 touch; gaps of 4 and of
# 4100 floats; sizes around one chunk (4096), 3 x 4096 + 4 laid across chunk boundaries, one frozen segment between two live ones
BOUNDARY = [
    (4, 1e-2, 0.0, 1, False, 0), (8, 1e-4, 0.05, 2, False, 0), (4092, 3e-3, 0.0, 7, False, 4), (4096, 1e-4, 0.1, 1000, False, 0),
    (4100, 1e-2, 0.0, 1, False, 4100), (8200, 5e-3, 0.05, 3, True, 0), (100004, 2e-4, 0.05, 2, False, 0),
    (3 * 4096 + 4, 1e-2, 0.0, 7, False, 0), (1150004, 1e-4, 0.1, 1000, False, 0),
]


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Case:
    """Buffers p, g, m, v with random contents EVERYWHERE (gaps and the frozen segment included), the segment table, and one torch
    optimiser per live segment whose state starts at the segment's moments and step count."""

    def __init__(self, layout, seed=0, tail=8):
        self.rows, self.meta, o = [], [], 0
        for k, (n, lr, wd, t0, frozen, gap) in enumerate(layout):
            o += gap
            self.rows.append((o, o + n, k, L.SEG_FROZEN if frozen else 0))
            self.meta.append((lr, wd, t0, frozen))
            o += n
        self.n = o + tail                                            # (a gap behind the last segment too)
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.p = torch.randn(self.n, device=DEV, generator=gen)
        self.g = torch.randn(self.n, device=DEV, generator=gen)
        self.m = torch.randn(self.n, device=DEV, generator=gen) * 0.1
        self.v = torch.rand(self.n, device=DEV, generator=gen) * 0.01
        self.gen = gen
        self.table = ops.AdamwSegTable(self.rows, DEV)
        self.calls = 0
        self.live = torch.zeros(self.n, device=DEV, dtype=torch.bool)
        self.frozen = torch.zeros(self.n, device=DEV, dtype=torch.bool)
        self.ref = []
        for (lo, hi, _, fl), (lr, wd, t0, fro) in zip(self.rows, self.meta):
            (self.frozen if fro else self.live)[lo:hi] = True
            if fro:
                self.ref.append(None)
                continue
            q = self.p[lo:hi].clone().requires_grad_(True)
            opt = torch.optim.AdamW([q], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
            opt.state[q] = {"step": torch.tensor(float(t0 - 1)), "exp_avg": self.m[lo:hi].clone(), "exp_avg_sq": self.v[lo:hi].clone()}
            self.ref.append((q, opt))
        self.gap = ~(self.live | self.frozen)

    def hp(self, extra=None):
        extra = self.calls if extra is None else extra
        return [(lr, wd, t0 + extra) for lr, wd, t0, _ in self.meta]

    def fresh_grads(self, scale=1.0):
        self.g.copy_(torch.randn(self.n, device=DEV, generator=self.gen) * scale)

    def ref_step(self, coef=1.0):
        for (lo, hi, _, _), r in zip(self.rows, self.ref):
            if r is not None:
                r[0].grad = self.g[lo:hi].clone() * coef
                r[1].step()

    def check(self, tag):
        worst = 0.0
        for k, ((lo, hi, _, _), r) in enumerate(zip(self.rows, self.ref)):
            if r is None:
                continue
            q, opt = r
            for what, a, b in (("p", self.p[lo:hi], q.detach()), ("m", self.m[lo:hi], opt.state[q]["exp_avg"]),
                               ("v", self.v[lo:hi], opt.state[q]["exp_avg_sq"])):
                e = _rel(a, b)
                assert e < BAR, (tag, k, what, hi - lo, e)
                worst = max(worst, e)
        return worst


@pytest.fixture(scope="module")
def boundary():
    """Four calls with fresh gradients on the boundary layout; the tests below read what it kept."""
    c = Case(BOUNDARY, seed=1)
    assert 1.2e6 < c.n < 1.4e6 and c.rows[0][0] == 0
    keep = {"worst": 0.0}
    for call in range(4):
        if call:
            c.fresh_grads()
        before = {k: getattr(c, k).clone() for k in "pgmv"}
        c.ref_step()
        zero = call != 2                                             # (the third call leaves the gradients in place)
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp(), B1, B2, EPS, zero_grad=zero)
        c.calls += 1
        keep["worst"] = max(keep["worst"], c.check(f"call {call}"))
        keep[call] = (before, {k: getattr(c, k).clone() for k in "pgmv"}, zero)
    keep["case"] = c
    return keep


def test_boundary_segments_match_torch(boundary):
    print(f"boundary layout, 4 calls: worst per-segment rel_l2 of p / m / v = {boundary['worst']:.3e}")
    held("adamw_seg.boundary.rel_l2", boundary["worst"], hard=BAR)


def test_gaps_and_frozen_segment_are_left_alone(boundary):
    c = boundary["case"]
    assert int(c.gap.sum()) == 4 + 4100 + 8 and int(c.frozen.sum()) == 8200
    for call in range(4):
        before, after, zero = boundary[call]
        for k in "pgmv":                                             # elements in no segment: neither read nor written
            assert torch.equal(before[k][c.gap].view(torch.int32), after[k][c.gap].view(torch.int32)), (call, k)
        for k in "pmv":
            assert torch.equal(before[k][c.frozen].view(torch.int32), after[k][c.frozen].view(torch.int32)), (call, k)
        if zero:
            assert not bool(after["g"][c.frozen].any()) and not bool(after["g"][c.live].any()), call
        else:
            assert torch.equal(before["g"].view(torch.int32), after["g"].view(torch.int32)), call
        assert not torch.equal(before["p"][c.live], after["p"][c.live])


def test_past_the_grid_cap():
    """4096 * 4096 + 8196 floats in 3 segments: 4099 chunks for a grid of 4096 workgroups - the first three workgroups take a
    second chunk, and chunk 4096 lies inside the third segment."""
    total = 4096 * 256 * 4 * 4 + 8196
    layout = [(6000004, 1e-2, 0.0, 1, False, 0), (10000000, 1e-4, 0.05, 7, False, 0), (total - 16000004, 1e-2, 0.1, 2, False, 0)]
    c = Case(layout, seed=2, tail=0)
    first, n_chunks = ops.seg_chunks(c.rows)
    assert c.n == total and n_chunks == 4099 and first[2] < 4096 < n_chunks
    c.ref_step()
    ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp(), B1, B2, EPS, zero_grad=True)
    worst = c.check("grid cap")
    assert not bool(c.g.any())
    print(f"grid-cap case: worst per-segment rel_l2 = {worst:.3e}")
    held("adamw_seg.grid_cap.rel_l2", worst, hard=BAR)


def test_clip_and_gscale_against_clip_grad_norm():
    c = Case(BOUNDARY[:8], seed=3)
    sq = torch.zeros(1, device=DEV, dtype=torch.float64)
    worst = 0.0
    for call, max_norm in enumerate((50.0, 1e4)):                    # the first clips (norm ~ 0.5 * sqrt(133 k) = 180), the second does not
        if call:
            c.fresh_grads()
        sq.zero_()
        for (lo, hi, _, _), r in zip(c.rows, c.ref):
            if r is not None:
                ops.grad_sqnorm(c.g[lo:hi], sq)                      # the union of the live segments, as the optimiser forms it
        for (lo, hi, _, _), r in zip(c.rows, c.ref):
            if r is not None:
                r[0].grad = c.g[lo:hi].clone() * 0.5
        norm = torch.nn.utils.clip_grad_norm_([r[0] for r in c.ref if r is not None], max_norm, foreach=False)
        assert (float(norm) > max_norm) == (call == 0)
        for r in c.ref:
            if r is not None:
                r[1].step()
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp(), B1, B2, EPS, gscale=0.5, max_norm=max_norm, sqnorm=sq, zero_grad=True)
        c.calls += 1
        worst = max(worst, c.check(f"clip call {call}"))
    print(f"clip + gscale: worst per-segment rel_l2 = {worst:.3e}")
    held("adamw_seg.clip.rel_l2", worst, hard=BAR)


def test_gate_sequence_step_gated_step_step():
    """The plan of test_gated_pass_shapes_against_torch, per segment: the host counts every call, the device takes the gated one
    out of every segment's step count."""
    c = Case(BOUNDARY[:8], seed=4)
    gate = torch.zeros(ops.GATE_WORDS, device=DEV, dtype=torch.int32)
    sq = torch.zeros(1, device=DEV, dtype=torch.float64)
    worst = 0.0
    for call in range(4):
        c.fresh_grads(scale=1000.0 if call == 1 else 1.0)
        sq.zero_()
        ops.grad_sqnorm(c.g, sq)
        ops.adamw_gate(sq, gate, skip_norm=1e4)                      # norm ~ 366 on plain calls, 3.7e5 on the scaled one
        before = {k: getattr(c, k).clone() for k in "pgmv"}
        if call != 1:
            c.ref_step()
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp(), B1, B2, EPS, sqnorm=sq, zero_grad=True, gate=gate)
        c.calls += 1
        if call == 1:
            assert gate.tolist()[:3] == [1, 1, 1]
            for k in "pmv":
                assert torch.equal(before[k].view(torch.int32), getattr(c, k).view(torch.int32)), k
            assert not bool(c.g[c.live | c.frozen].any())
            assert torch.equal(before["g"][c.gap].view(torch.int32), c.g[c.gap].view(torch.int32))
        else:
            worst = max(worst, c.check(f"gate call {call}"))
    assert gate.tolist()[:3] == [0, 1, 1]
    for (lr, wd, t0, fro), r in zip(c.meta, c.ref):
        if r is not None:
            assert int(r[1].state[r[0]]["step"]) == t0 - 1 + 3
    print(f"gate sequence: worst per-segment rel_l2 = {worst:.3e}")
    held("adamw_seg.gate.rel_l2", worst, hard=BAR)


def test_bitwise_equal_to_the_per_run_kernel():
    """The same state through ops.adamw_step once per segment: the same expression and the same host-rounded coefficients."""
    c = Case(BOUNDARY, seed=5)
    sq = torch.zeros(1, device=DEV, dtype=torch.float64)
    worst = 0.0
    for call in range(3):
        if call:
            c.fresh_grads()
        sq.zero_()
        ops.grad_sqnorm(c.g, sq)
        ref = {k: getattr(c, k).clone() for k in "pgmv"}
        for (lo, hi, _, _), (lr, wd, t0, fro) in zip(c.rows, c.meta):
            if fro:
                ref["g"][lo:hi].zero_()
                continue
            ops.adamw_step(ref["p"][lo:hi], ref["g"][lo:hi], ref["m"][lo:hi], ref["v"][lo:hi], lr, wd, t0 + call, B1, B2, EPS,
                           gscale=0.5, max_norm=100.0, sqnorm=sq, zero_grad=True)
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp(call), B1, B2, EPS, gscale=0.5, max_norm=100.0, sqnorm=sq, zero_grad=True)
        for k in "pgmv":
            worst = max(worst, float((getattr(c, k) - ref[k]).abs().max()))
            assert torch.equal(getattr(c, k).view(torch.int32), ref[k].view(torch.int32)), (call, k, worst)
    print(f"segmented vs per-run kernel over 3 calls: largest element difference {worst:.3e}")


def test_refusals_launch_nothing():
    c = Case(BOUNDARY[:3], seed=6)
    before = {k: getattr(c, k).clone() for k in "pgmv"}
    off = torch.randn(c.n + 1, device=DEV)
    with pytest.raises(L.EgoHipError):                               # a pointer that is not 16-byte aligned
        ops.adamw_step_seg(off[1:], c.g, c.m, c.v, c.table, c.hp(), B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError):                               # segment 2 names slot 2 of a block with two slots
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, c.hp()[:2], B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError):                               # step 0 in the slot of a live segment
        ops.adamw_step_seg(c.p, c.g, c.m, c.v, c.table, [(lr, wd, 0) for lr, wd, _ in c.hp()], B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError):                               # a segment behind the end of the buffers
        ops.adamw_step_seg(c.p[:4096], c.g[:4096], c.m[:4096], c.v[:4096], c.table, c.hp(), B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError):
        ops.AdamwSegTable([(0, 8, 0, 0), (4, 12, 1, 0)], DEV)        # overlapping segments never reach the device
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(before[k].view(torch.int32), getattr(c, k).view(torch.int32)), k
    # a frozen segment's slot may hold any step: it is never read
    rows = [(0, 8, 0, L.SEG_FROZEN), (8, 16, 1, 0)]
    ops.adamw_step_seg(c.p, c.g, c.m, c.v, ops.AdamwSegTable(rows, DEV), [(1e-3, 0.0, 0), (1e-3, 0.0, 1)], B1, B2, EPS, zero_grad=True)
    assert not bool(c.g[:16].any()) and torch.equal(before["p"][:8], c.p[:8]) and not torch.equal(before["p"][8:16], c.p[8:16])
