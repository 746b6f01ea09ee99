"""The AdamW step gate at kernel level (ops.adamw_gate + ops.adamw_step_gated): `skip_grad` of the reference loop
(egom2p/utils/native_scaler.py:34-40) and the opt-in non-finite guard, decided on the device.

tests/golden/skip_grad.npz is the real reference scaler driving torch.optim.AdamW on the CPU (tools/make_goldens_skip_grad.py):
calls 0, 1, 3, 5 stepped, 2 (norm x 40) and 4 (an inf element) skipped, 6 (a NaN element) STEPPED - `nan >= thr` is false."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
LR, WD = 1e-3, 0.05


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _state(n):
    return tuple(torch.zeros(n, device=DEV) for _ in range(3))          # g, m, v


def _gate():
    return torch.zeros(ops.GATE_WORDS, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV, dtype=torch.float64)


def _call(p, g, m, v, step, gate, sq, skip_norm=0.0, guard=False, gscale=1.0, max_norm=0.0, wd=WD, runs=None):
    """norm, gate, gated pass over every run [(lo, hi, wd)]; returns the norm the gate saw"""
    sq.zero_()
    ops.grad_sqnorm(g, sq)
    ops.adamw_gate(sq, gate, gscale=gscale, skip_norm=skip_norm, skip_nonfinite=guard)
    for lo, hi, w in (runs or [(0, p.numel(), wd)]):
        ops.adamw_step_gated(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], LR, w, step, gate, gscale=gscale, max_norm=max_norm, sqnorm=sq,
                             zero_grad=True)
    return float(sq.sqrt().to(torch.float32).item()) * gscale


def test_fixture_replay_matches_the_reference_scaler():
    f = np.load(os.path.join(GOLDEN_DIR, "skip_grad.npz"), allow_pickle=False)
    sizes = {"decay0": 1027, "decay1": 64, "nodecay0": 4099, "nodecay1": 3}
    off, o = {}, 0
    for n, k in sizes.items():                                          # 4-aligned offsets, as the engine lays tensors out
        off[n] = o
        o += (k + 3) // 4 * 4
    total = o
    runs = [(0, off["nodecay0"], WD), (off["nodecay0"], total, 0.0)]
    P = torch.zeros(total, device=DEV)
    G, M, V = _state(total)
    gate, sq = _gate()

    def put(buf, prefix):
        buf.zero_()
        for n, k in sizes.items():
            buf[off[n]:off[n] + k] = torch.from_numpy(f[f"{prefix}.{n}"]).to(DEV)

    put(P, "p0")
    dec, norms = f["decisions"].tolist(), f["norms"]
    for k in range(6):
        put(G, f"g{k}")
        before = (P.clone(), M.clone(), V.clone())
        norm = _call(P, G, M, V, k + 1, gate, sq, skip_norm=200.0, runs=runs)
        print(f"call {k}: norm {norm} (fixture {norms[k]}), gate {gate.tolist()}")
        assert int(gate[0]) == dec[k], (k, gate.tolist())
        if math.isfinite(float(norms[k])):
            assert abs(norm - float(norms[k])) <= 1e-5 * float(norms[k]), (k, norm, float(norms[k]))
        else:
            assert norm == float(norms[k])                               # call 4: inf on both sides
        assert float(G.abs().max()) == 0.0
        if dec[k]:
            for a, b in zip((P, M, V), before):
                assert torch.equal(a, b), k
        else:
            for n, sz in sizes.items():
                r = _rel(P[off[n]:off[n] + sz], torch.from_numpy(f[f"p{k + 1}.{n}"]).to(DEV))
                print(f"  {n}: rel_l2 {r:.3e}")
                assert r < 1e-6, (k, n, r)
    assert gate.tolist()[:3] == [0, 2, 2]
    # call 6 holds a NaN: the reference steps it (nan >= thr is false) - so does the gate with the guard off
    pre = (P.clone(), M.clone(), V.clone(), gate.clone())
    put(G, "g6")
    _call(P, G, M, V, 7, gate, sq, skip_norm=200.0, runs=runs)
    assert gate.tolist()[:3] == [0, 2, 2]
    for n, sz in sizes.items():
        got, want = P[off[n]:off[n] + sz], torch.from_numpy(f[f"p7.{n}"]).to(DEV)
        assert torch.equal(got.isnan(), want.isnan()), n
    assert bool(P.isnan().any())
    # the same call from the same pre-state with the guard on: gated, nothing moves
    P.copy_(pre[0]); M.copy_(pre[1]); V.copy_(pre[2]); gate.copy_(pre[3])
    put(G, "g6")
    _call(P, G, M, V, 7, gate, sq, skip_norm=200.0, guard=True, runs=runs)
    assert gate.tolist()[:3] == [1, 3, 3]
    assert torch.equal(P, pre[0]) and torch.equal(M, pre[1]) and torch.equal(V, pre[2]) and float(G.abs().max()) == 0.0


def test_gate_boundary_is_greater_or_equal():
    """[3, 4, 0, ...] has norm exactly 5.0 (25.0 and its root are exact): threshold 5.0 gates (`norm >= skip_grad`), the next
    float32 above steps; with gscale 0.5 (world_size 2) the gate sees 2.5."""
    up = float(np.nextafter(np.float32(5.0), np.float32(np.inf)))
    for gscale, thr, want in ((1.0, 5.0, 1), (1.0, up, 0), (0.5, 2.5, 1)):
        p = torch.ones(8, device=DEV)
        g, m, v = _state(8)
        g[0], g[1] = 3.0, 4.0
        gate, sq = _gate()
        norm = _call(p, g, m, v, 1, gate, sq, skip_norm=thr, gscale=gscale)
        assert norm == 5.0 * gscale
        assert int(gate[0]) == want, (gscale, thr, gate.tolist())
        assert bool(torch.equal(p, torch.ones(8, device=DEV))) == bool(want)
        assert float(g.abs().max()) == 0.0


# n = 3: no vector part; 100003: vector part + tail; the last: past the 4096-workgroup cap (the grid-stride loop runs twice for
# some threads) with a tail
@pytest.mark.parametrize("n", [3, 100003, 4096 * 256 * 4 + 4099])
def test_gated_pass_shapes_against_torch(n):
    gen = torch.Generator(device=DEV).manual_seed(n % 1000)
    p0 = torch.randn(n, device=DEV, generator=gen)
    pr = p0.clone().requires_grad_(True)
    topt = torch.optim.AdamW([pr], lr=LR, betas=(0.9, 0.95), eps=1e-8, weight_decay=WD)
    p = p0.clone()
    g, m, v = _state(n)
    gate, sq = _gate()
    for k, skip in enumerate((False, True, False, False)):              # step, skip, step, step
        gk = torch.randn(n, device=DEV, generator=gen) * (k + 1)
        g.copy_(gk)
        before = (p.clone(), m.clone(), v.clone())
        _call(p, g, m, v, k + 1, gate, sq, skip_norm=1e-9 if skip else 1e9)
        assert int(gate[0]) == int(skip)
        assert float(g.abs().max()) == 0.0
        if skip:
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
        else:
            pr.grad = gk
            topt.step()
            r = _rel(p, pr.detach())
            print(f"n {n} call {k}: rel_l2 {r:.3e}")
            assert r < 1e-6, (n, k, r)
    assert gate.tolist()[:3] == [0, 1, 1] and int(topt.state[pr]["step"]) == 3


def test_ungated_calls_match_the_plain_kernel():
    """No gated call ever: the gated pass beside ops.adamw_step on the same inputs.  The device's pow feeding the two float bias
    corrections is the only difference between the kernels; the largest element difference is printed (DESIGN records it)."""
    n = 100003
    gen = torch.Generator(device=DEV).manual_seed(7)
    p0 = torch.randn(n, device=DEV, generator=gen)
    pa, pb = p0.clone(), p0.clone()
    ga, ma, va = _state(n)
    gb, mb, vb = _state(n)
    gate, sq = _gate()
    worst = 0.0
    for k in range(5):
        gk = torch.randn(n, device=DEV, generator=gen) * 3
        ga.copy_(gk); gb.copy_(gk)
        _call(pa, ga, ma, va, k + 1, gate, sq, guard=True, max_norm=1.0)
        sq.zero_()
        ops.grad_sqnorm(gb, sq)
        ops.adamw_step(pb, gb, mb, vb, LR, WD, k + 1, gscale=1.0, max_norm=1.0, sqnorm=sq, zero_grad=True)
        worst = max(worst, float((pa - pb).abs().max()), float((ma - mb).abs().max()), float((va - vb).abs().max()))
        assert _rel(pa, pb) < 1e-6 and _rel(ma, mb) < 1e-6 and _rel(va, vb) < 1e-6, k
    print(f"largest element difference gated vs plain over 5 steps: {worst:.3e}")
    assert gate.tolist()[:3] == [0, 0, 0]


def test_clip_with_nonfinite_guard():
    """The production recipe (clip_grad 1.0) with the guard: an inf element makes clip_grad_norm_'s coefficient 0 and inf * 0 a
    NaN in the reference; here the call moves nothing, and the next finite call is torch's SECOND step."""
    n = 4099
    gen = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.randn(n, device=DEV, generator=gen)
    pr = p0.clone().requires_grad_(True)
    topt = torch.optim.AdamW([pr], lr=LR, betas=(0.9, 0.95), eps=1e-8, weight_decay=WD)
    p = p0.clone()
    g, m, v = _state(n)
    gate, sq = _gate()
    for k, bad in enumerate((False, True, False)):
        gk = torch.randn(n, device=DEV, generator=gen) * 2
        if bad:
            gk[1234] = float("inf")
        g.copy_(gk)
        before = (p.clone(), m.clone(), v.clone())
        _call(p, g, m, v, k + 1, gate, sq, guard=True, max_norm=1.0)
        assert int(gate[0]) == int(bad) and float(g.abs().max()) == 0.0
        if bad:
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
        else:
            pr.grad = gk.clone()
            torch.nn.utils.clip_grad_norm_([pr], 1.0)
            topt.step()
            assert _rel(p, pr.detach()) < 1e-6, k
        assert bool(torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all())
    assert int(topt.state[pr]["step"]) == 2 and gate.tolist()[:3] == [0, 1, 1]
