"""`ops.optim_step_seg` (ego_optim_step_seg): Adam, SGD with momentum and Nesterov on the segmented flat-buffer launch, and the
optimiser object / `create_optimizer` / training script on top of it.

Kernel level, one layout throughout (tests/_optim_ref.py): 8200 floats - segments of 4, 4092 and 4096 floats (the last one whole
chunk), a frozen segment of 4 and 4 floats in no segment - two groups, 64 sentinel floats on either side of every buffer.
  * the SGD kinds on operands in eighths: three steps equal the fp64 restatement BIT FOR BIT (nothing rounds);
  * Adam against the fp64 restatement, held to twice what the parent's `ops.adamw_step_seg` measures against ITS fp64 restatement
    on the same inputs (tests/golden/parity_bars_optim_kinds.json; the coupled decay adds one rounding to d);
  * the gate, and the argument errors that launch nothing.
Object level: three training steps of `ego_tiny_2e_2d` per kind beside torch.optim.SGD / Adam fed the engine's own gradients
(the pattern and the 2e-6 of tests/test_step_gate_optim_gpu.py / tests/test_layer_decay_engine_gpu.py)."""
import importlib.util
import json
import os
import random
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _optim_ref as R  # noqa: E402
from conftest import GOLDEN_DIR, bar, load_golden, rel_l2  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm  # noqa: E402
from egom2p_amd.optim import create_optimizer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
B1, B2, EPS = 0.9, 0.95, 1e-8
BAR = 1e-6                                          # this kernel family's stated tolerance (tests/test_adamw_seg_kernel_gpu.py)
PAD = 64                                            # sentinel floats on either side
N = R.EXACT_N
ROWS = [(lo, hi, grp, L.SEG_FROZEN if fro else 0) for lo, hi, grp, fro in R.EXACT_ROWS]
_BARS_PATH = os.path.join(GOLDEN_DIR, "parity_bars_optim_kinds.json")
RECORDED = json.load(open(_BARS_PATH)) if os.path.exists(_BARS_PATH) else {}


def _mask(which):
    m = np.zeros(N, dtype=bool)
    for lo, hi, _, fl in ROWS:
        if (which == "frozen") == bool(fl):
            m[lo:hi] = True
    return m


LIVE, FROZEN = _mask("live"), _mask("frozen")
STRAY = ~(LIVE | FROZEN)
assert LIVE.sum() == 8192 and FROZEN.sum() == 4 and STRAY.sum() == 4


class Buf:
    """A flat fp32 buffer of N floats inside an allocation with PAD sentinel floats on either side (16-byte aligned view)."""

    def __init__(self, values):
        rng = np.random.default_rng(99)
        self.whole = torch.from_numpy(rng.standard_normal(N + 2 * PAD).astype(np.float32)).to(DEV)
        self.t = self.whole[PAD:PAD + N]
        assert self.t.data_ptr() % 16 == 0
        self.set(values)
        self.guard = self.whole.clone()

    def set(self, values):
        self.t.copy_(torch.from_numpy(np.asarray(values, dtype=np.float64).astype(np.float32)))

    def np(self):
        return self.t.cpu().numpy()

    def sentinels_intact(self):
        w, g = self.whole.view(torch.int32), self.guard.view(torch.int32)
        return torch.equal(w[:PAD], g[:PAD]) and torch.equal(w[PAD + N:], g[PAD + N:])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@pytest.fixture(scope="module")
def table():
    return ops.AdamwSegTable(ROWS, DEV)


# ---- 4. exact cases, SGD kinds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["momentum", "nesterov"])
def test_sgd_kinds_exact_against_the_restatement(kind, table):
    p0, gs, buf0 = R.exact_inputs()
    want, exact = R.exact_run(kind, p0, gs, buf0)
    assert exact                                                     # (held on the CPU too: test_exact_case_stays_in_float32)
    p, g, buf = Buf(p0), Buf(gs[0]), Buf(buf0)
    hp = [(lr, wd, 0) for lr, wd in R.EXACT_HP]                      # step counts are not read by the SGD kinds: 0 is no error
    for s in range(R.EXACT_STEPS):
        g.set(gs[s])
        ops.optim_step_seg(kind, p.t, g.t, buf.t, None, table, hp, momentum=R.EXACT_MOMENTUM, zero_grad=True)
        gp, gb, gg = p.np(), buf.np(), g.np()
        assert np.array_equal(bits(gp), bits(want[s][0])), (kind, s, np.abs(gp - want[s][0]).max())
        assert np.array_equal(bits(gb), bits(want[s][1])), (kind, s, np.abs(gb - want[s][1]).max())
        assert not gg[LIVE | FROZEN].any()                           # gradients zeroed, the frozen segment's too
        assert np.array_equal(bits(gg[STRAY]), bits(gs[s][STRAY]))   # elements in no segment are not written
    rest = FROZEN | STRAY
    assert np.array_equal(bits(p.np()[rest]), bits(p0[rest])) and np.array_equal(bits(buf.np()[rest]), bits(buf0[rest]))
    assert not np.array_equal(bits(p.np()[LIVE]), bits(p0[LIVE]))
    assert p.sentinels_intact() and g.sentinels_intact() and buf.sentinels_intact()
    # the two groups took their own lr / wd: one element of each group by hand, first step
    for i in (0, 4):
        lr, wd = R.EXACT_HP[0 if i < 4 else 1]
        d = gs[0][i] + wd * p0[i]
        b = R.EXACT_MOMENTUM * buf0[i] + d
        assert want[0][0][i] == p0[i] - lr * (d + R.EXACT_MOMENTUM * b if kind == "nesterov" else b)


# ---- 5. Adam against fp64, the bar measured on the parent's kernel -------------------------------------------------------------
ADAM_HP = [(1e-2, 0.05, 1), (1e-3, 0.1, 7)]         # (lr, wd, first step) of the two groups


def _adam_inputs(seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    p, m = f32(rng.standard_normal(N)), f32(0.1 * rng.standard_normal(N))
    v = f32(m * m + 0.01 * rng.random(N))                            # v >= m^2: a second moment this first moment could have
    gs = [f32(rng.standard_normal(N)) for _ in range(3)]
    return p, gs, m, v


def _run_against_fp64(kind, max_norm, table):
    """Three calls of the kernel (kind "adamw": the parent's ops.adamw_step_seg) beside the fp64 restatement run from the same
    fp32 inputs; returns the worst rel_l2 of p / m / v over the live elements and over each live segment."""
    p0, gs, m0, v0 = _adam_inputs(5)
    p, g, m, v = Buf(p0), Buf(gs[0]), Buf(m0), Buf(v0)
    rp, rm, rv = p0.copy(), m0.copy(), v0.copy()
    sq = torch.zeros(1, device=DEV, dtype=torch.float64)
    worst_all = worst_seg = 0.0
    for s in range(3):
        g.set(gs[s])
        sq.zero_()
        for lo, hi, _, fl in ROWS:
            if not fl:
                ops.grad_sqnorm(g.t[lo:hi], sq)                      # the live segments, as the optimiser forms the norm
        sqv = float(sq.item())
        norm = float(np.sqrt(sqv)) * 0.5
        assert (norm > max_norm) == (max_norm < 50.0)                # ~ 0.5 * sqrt(8192) = 45: the small max_norm clips, the large does not
        coef = R.clip_coef(sqv, 0.5, max_norm)
        hp = [(lr, wd, t0 + s) for lr, wd, t0 in ADAM_HP]
        kw = dict(gscale=0.5, max_norm=max_norm, sqnorm=sq, zero_grad=True)
        if kind == "adamw":
            ops.adamw_step_seg(p.t, g.t, m.t, v.t, table, hp, B1, B2, EPS, **kw)
        else:
            ops.optim_step_seg(kind, p.t, g.t, m.t, v.t, table, hp, B1, B2, EPS, **kw)
        for lo, hi, grp, fl in ROWS:
            if fl:
                continue
            lr, wd, t0 = ADAM_HP[grp]
            sl = slice(lo, hi)
            rp[sl], rm[sl], rv[sl] = R.step(kind, rp[sl], gs[s][sl], rm[sl], rv[sl], lr, wd, t=t0 + s, b1=B1, b2=B2,
                                            eps=EPS, coef=coef)
        for got, want in ((p.np(), rp), (m.np(), rm), (v.np(), rv)):
            worst_all = max(worst_all, rel_l2(got[LIVE], want[LIVE]))
            for lo, hi, _, fl in ROWS:
                if not fl:
                    worst_seg = max(worst_seg, rel_l2(got[lo:hi], want[lo:hi]))
            assert np.array_equal(bits(got[~LIVE]), bits(want[~LIVE]))                   # frozen and stray: bit patterns kept
        assert not g.np()[LIVE | FROZEN].any() and np.array_equal(bits(g.np()[STRAY]), bits(gs[s][STRAY]))
    assert all(b.sentinels_intact() for b in (p, g, m, v))
    return worst_all, worst_seg


@pytest.mark.parametrize("case,max_norm", [("clip", 10.0), ("noclip", 1e4)])
def test_adam_against_fp64_within_twice_the_parents_error(case, max_norm, table):
    """Measured on MI355X (tests/golden/parity_bars_optim_kinds.json), clip / no clip: adamw_seg 1.03e-7 / 1.76e-7, adam
    1.19e-7 / 1.82e-7 - the new kernel is held to 2 x the parent's recorded value."""
    base, base_seg = _run_against_fp64("adamw", max_norm, table)
    mine, mine_seg = _run_against_fp64("adam", max_norm, table)
    print(f"{case}: rel_l2 against fp64 over 3 steps, worst of p / m / v - parent adamw_seg {base:.3e} (per segment {base_seg:.3e}), "
          f"adam {mine:.3e} (per segment {mine_seg:.3e})")
    bar(f"optim_kinds.adamw_seg.fp64.{case}", base, hard=BAR)
    bar(f"optim_kinds.adam.fp64.{case}", mine, hard=BAR)
    assert mine_seg < BAR and base_seg < BAR                         # a misattributed vector misses this by orders of magnitude
    if not os.environ.get("EGOM2P_RECORD_BARS"):
        rec = RECORDED[f"optim_kinds.adamw_seg.fp64.{case}"]
        assert base <= rec * 1.30, ("the yardstick moved", base, rec)              # conftest.bar's margin: the record still describes the parent
        assert mine <= 2.0 * rec, (mine, "recorded parent error", rec)


# ---- 6. gate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "momentum", "nesterov"])
def test_gated_call_writes_nothing_but_zeroed_gradients(kind, table):
    p0, gs, m0, v0 = _adam_inputs(6)
    p, g, m = Buf(p0), Buf(gs[0]), Buf(m0)
    v = Buf(v0) if kind == "adam" else None
    gate = torch.tensor([1, 0, 0, 0], device=DEV, dtype=torch.int32)
    hp = [(lr, wd, t0) for lr, wd, t0 in ADAM_HP]
    for zero in (False, True):
        ops.optim_step_seg(kind, p.t, g.t, m.t, v.t if v else None, table, hp, B1, B2, EPS, momentum=0.5, zero_grad=zero, gate=gate)
        for b, want in ((p, p0), (m, m0)) + (((v, v0),) if v else ()):
            assert np.array_equal(bits(b.np()), bits(want)) and b.sentinels_intact()
        if zero:
            assert not g.np()[LIVE | FROZEN].any() and np.array_equal(bits(g.np()[STRAY]), bits(gs[0][STRAY]))
        else:
            assert np.array_equal(bits(g.np()), bits(gs[0]))
    assert g.sentinels_intact() and gate.tolist() == [1, 0, 0, 0]


def test_gate_count_moves_the_adam_bias_corrections(table):
    """gate[1] = 2: a slot's corrections are those of step - 2 (formed on the device); the restatement at the unshifted step
    is far away (bc1 of step 3 against step 1: a factor 2.7 on the first group's update)."""
    gate = torch.tensor([0, 2, 2, 0], device=DEV, dtype=torch.int32)
    hp_shift = [(lr, wd, t0 + 2) for lr, wd, t0 in ADAM_HP]
    p0, gs, m0, v0 = _adam_inputs(5)
    p, g, m, v = Buf(p0), Buf(gs[0]), Buf(m0), Buf(v0)
    ops.optim_step_seg("adam", p.t, g.t, m.t, v.t, table, hp_shift, B1, B2, EPS, zero_grad=True, gate=gate)
    worst = far = 0.0
    for lo, hi, grp, fl in ROWS:
        if fl:
            continue
        lr, wd, t0 = ADAM_HP[grp]
        sl = slice(lo, hi)
        rp, rm, rv = R.step("adam", p0[sl], gs[0][sl], m0[sl], v0[sl], lr, wd, t=t0, b1=B1, b2=B2, eps=EPS)
        wrong, _, _ = R.step("adam", p0[sl], gs[0][sl], m0[sl], v0[sl], lr, wd, t=t0 + 2, b1=B1, b2=B2, eps=EPS)
        worst = max(worst, rel_l2(p.np()[sl], rp), rel_l2(m.np()[sl], rm), rel_l2(v.np()[sl], rv))
        if grp == 0:
            far = max(far, rel_l2(p.np()[sl], wrong))
    print(f"gate[1] = 2: worst per-segment rel_l2 against the restatement at step - 2: {worst:.3e}; against the unshifted step {far:.3e}")
    assert worst < BAR and far > 100 * BAR
    assert gate.tolist() == [0, 2, 2, 0]
    # the floor at 1: step 2 behind two gated calls is step 1, not step 0
    p.set(p0); g.set(gs[0]); m.set(m0); v.set(v0)
    ops.optim_step_seg("adam", p.t, g.t, m.t, v.t, table, [(lr, wd, 2) for lr, wd, _ in ADAM_HP], B1, B2, EPS, gate=gate)
    lr, wd, _ = ADAM_HP[0]
    rp, _, _ = R.step("adam", p0[:4], gs[0][:4], m0[:4], v0[:4], lr, wd, t=1, b1=B1, b2=B2, eps=EPS)
    assert rel_l2(p.np()[:4], rp) < BAR


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(table):
    p0, gs, m0, v0 = _adam_inputs(7)
    p, g, m, v = Buf(p0), Buf(gs[0]), Buf(m0), Buf(v0)
    hp = [(lr, wd, t0) for lr, wd, t0 in ADAM_HP]
    off = torch.zeros(N + 1, device=DEV)[1:]
    bad_table = ops.AdamwSegTable(ROWS, DEV)
    bad_table.host[2].hi = 8190                                      # the host copy is what the entry checks: not a multiple of 4
    calls = {
        "misaligned p": lambda k, vv: ops.optim_step_seg(k, off, g.t, m.t, vv, table, hp, B1, B2, EPS, momentum=0.5, zero_grad=True),
        "misaligned m": lambda k, vv: ops.optim_step_seg(k, p.t, g.t, off, vv, table, hp, B1, B2, EPS, momentum=0.5, zero_grad=True),
        "segment % 4": lambda k, vv: ops.optim_step_seg(k, p.t, g.t, m.t, vv, bad_table, hp, B1, B2, EPS, momentum=0.5, zero_grad=True),
        "group out of range": lambda k, vv: ops.optim_step_seg(k, p.t, g.t, m.t, vv, table, hp[:1], B1, B2, EPS, momentum=0.5, zero_grad=True),
    }
    for kind in ("adam", "momentum", "nesterov"):
        for what, call in calls.items():
            with pytest.raises(L.EgoHipError, match="bad arguments"):
                call(kind, v.t if kind == "adam" else None)
    with pytest.raises(L.EgoHipError, match="bad arguments"):       # an unknown kind
        ops.optim_step_seg(7, p.t, g.t, m.t, v.t, table, hp, B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="bad arguments"):
        ops.optim_step_seg(0, p.t, g.t, m.t, v.t, table, hp, B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="unknown optimiser kind"):
        ops.optim_step_seg("lamb", p.t, g.t, m.t, v.t, table, hp, B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="bad arguments"):       # Adam without its second moment
        ops.optim_step_seg("adam", p.t, g.t, m.t, None, table, hp, B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="bad arguments"):       # misaligned v counts for Adam only
        ops.optim_step_seg("adam", p.t, g.t, m.t, off, table, hp, B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="bad arguments"):       # step 0 in a live slot: an error for Adam ...
        ops.optim_step_seg("adam", p.t, g.t, m.t, v.t, table, [(lr, wd, 0) for lr, wd, _ in ADAM_HP], B1, B2, EPS, zero_grad=True)
    with pytest.raises(L.EgoHipError, match="bad arguments"):
        ops.optim_step_seg("nesterov", p.t, g.t, m.t, None, table, hp, momentum=-0.5, zero_grad=True)
    torch.cuda.synchronize()
    for b, want in ((p, p0), (g, gs[0]), (m, m0), (v, v0)):
        assert np.array_equal(bits(b.np()), bits(want)) and b.sentinels_intact()
    # ... and none for the SGD kinds, which do not read it
    ops.optim_step_seg("momentum", p.t, g.t, m.t, None, table, [(lr, wd, 0) for lr, wd, _ in ADAM_HP], momentum=0.5, zero_grad=True)
    assert not np.array_equal(bits(p.np()[LIVE]), bits(p0[LIVE])) and np.array_equal(bits(v.np()), bits(v0))


# ---- 8. the optimiser object ---------------------------------------------------------------------------------------------------
LR, WD, MOM, CLIP = 1e-2, 0.05, 0.9, 0.1
LATE = "encoder.0.attn.qkv.weight"                  # frozen for the first step, thawed for the second


def _args(opt):
    return types.SimpleNamespace(opt=opt, lr=LR, weight_decay=WD, opt_betas=(0.9, 0.95), opt_eps=1e-8, momentum=MOM)


def tiny_model():
    from functools import partial
    mods = ["tok_cam", "tok_gaze"]
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}
    return EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in mods}, dim=128, encoder_depth=2, decoder_depth=2, num_heads=2,
                  mlp_ratio=4, qkv_bias=False, proj_bias=False, mlp_bias=False,
                  norm_layer=partial(LayerNorm, eps=1e-6, bias=False), act_layer=torch.nn.SiLU, gated_mlp=True)


class Setup:
    def __init__(self, opt):
        _, meta = load_golden("tiny")
        cfg = MODEL_CFGS[meta["cfg"]]
        self.meta = meta
        md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
        self.mdg = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}
        self.model = tiny_model()
        self.model.load_state_dict(synth.build_state_dict(cfg, meta["seed"]))
        self.opt = create_optimizer(_args(opt), self.model)
        self.named = dict(self.model.named_parameters())

    def backward(self, step):
        random.seed(self.meta["py_seed"] + step)
        loss, _ = self.model(self.mdg, self.meta["n_enc"], self.meta["n_dec"])
        loss.backward()
        return float(loss.item())

    def freeze_for(self, step):
        self.named[LATE].requires_grad = step >= 1

    def run(self, steps=3):
        for step in range(steps):
            self.freeze_for(step)
            self.backward(step)
            self.opt.step(clip_grad=CLIP)
        eng = self.model.engine
        return eng.P.clone(), self.opt.m.clone(), None if self.opt.v is None else self.opt.v.clone()


@pytest.mark.parametrize("opt", ["sgd", "momentum", "adam"])
def test_optimiser_object_against_torch(opt):
    s = Setup(opt)
    kind = s.opt.kind
    assert kind == {"sgd": "nesterov", "momentum": "momentum", "adam": "adam"}[opt] and s.opt.segmented
    assert (s.opt.v is None) == (kind != "adam")
    named, eng = s.named, s.model.engine
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in named.items()}
    nd = lambda n: ("norm." in n or ".norm" in n or n.endswith(".bias"))
    groups = [{"params": [ref[n] for n in named if not nd(n)], "weight_decay": WD}, {"params": [ref[n] for n in named if nd(n)], "weight_decay": 0.0}]
    if kind == "adam":
        topt = torch.optim.Adam(groups, lr=LR, betas=(0.9, 0.95), eps=1e-8)
    else:
        topt = torch.optim.SGD(groups, lr=LR, momentum=MOM, nesterov=kind == "nesterov")
    key = eng._canon_key
    worst = worst_state = 0.0
    compared = clipped = 0
    for step in range(3):
        s.freeze_for(step)
        live =[n for n, p in named.items() if p.requires_grad]
        assert (LATE in live) == (step >= 1)
        s.backward(step)
        for n in named:
            ref[n].grad = named[n].grad.detach().clone() if n in live else None
        before = {n: p.detach().clone() for n, p in named.items()}
        tnorm = torch.nn.utils.clip_grad_norm_([ref[n] for n in live], CLIP)
        clipped += int(float(tnorm) > CLIP)
        topt.step()
        norm = s.opt.step(clip_grad=CLIP)
        assert abs(norm.item() - tnorm.item()) < 1e-5 * tnorm.item()  # (the frozen tensor's gradient is left out of the norm)
        for n, p in named.items():
            e = rel_l2(p.detach().float().cpu().numpy(), ref[n].detach().float().cpu().numpy())
            worst = max(worst, e)
            assert e < 2e-6, (opt, step, n, e)
        if step == 0:
            assert torch.equal(named[LATE].detach(), before[LATE]) and any(f for *_, f in s.opt.segments())
        assert any(not torch.equal(named[n].detach(), before[n]) for n in live)
        assert float(eng.G.abs().max().item()) == 0.0                # the frozen range cleared in the same launch
        # the state buffers: linear in the clip coefficient, which the two sides form from norms that agree to 1e-5 (above)
        for n in live:
            o, cnt, _ = eng.offsets[key(n)]
            st = topt.state[ref[n]]
            pairs = [(s.opt.m, st["exp_avg"]), (s.opt.v, st["exp_avg_sq"])] if kind == "adam" else [(s.opt.m, st["momentum_buffer"])]
            if not (named[n].numel() == cnt and named[n].is_contiguous() and named[n].data_ptr() == eng.P.data_ptr() + 4 * o):
                continue                                             # (stored in another element order: covered through its parameters)
            compared += 1
            for mine, theirs in pairs:
                e = rel_l2(mine[o:o + cnt].cpu().numpy(), theirs.detach().reshape(-1).cpu().numpy())
                worst_state = max(worst_state, e)
                assert e < 2e-5, (opt, step, n, e)
    print(f"--opt {opt}: worst per-tensor rel_l2 against torch over 3 steps: parameters {worst:.3e}, state {worst_state:.3e}")
    if kind == "adam":                                               # the thawed tensor's bias correction starts at step 1
        early = next(n for n in named if n != LATE and named[n].numel() > 4)
        assert topt.state[ref[LATE]]["step"].item() == 2 == s.opt.t - s.opt.skipped[key(LATE)]
        assert topt.state[ref[early]]["step"].item() == 3 == s.opt.t - s.opt.skipped.get(key(early), 0)
        assert any(sk == 1 for _, _, _, sk, fro in s.opt.segments() if not fro)
    assert clipped >= 1                                              # clipping is on, and clips
    assert len(s.opt._launches) == 1 and compared > 3 * len(named) // 2
    Pa, ma, va = eng.P.clone(), s.opt.m.clone(), None if s.opt.v is None else s.opt.v.clone()

    # two runs from the same seed are bitwise equal
    Pb, mb, vb = Setup(opt).run()
    assert torch.equal(Pa, Pb) and torch.equal(ma, mb) and (va is None or torch.equal(va, vb))

    # state_dict -> new optimiser -> load_state_dict continues bitwise
    st = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.opt.state_dict().items()}
    assert st["kind"] == kind and ("v" in st) == (kind == "adam") and st["t"] == 3
    opt2 = create_optimizer(_args(opt), s.model)
    opt2.load_state_dict(st)
    assert opt2.t == s.opt.t and opt2.skipped == s.opt.skipped
    s.backward(3)
    P0, G0 = eng.P.clone(), eng.G.clone()
    s.opt.step(clip_grad=CLIP)
    Pc, mc, vc = eng.P.clone(), s.opt.m.clone(), None if s.opt.v is None else s.opt.v.clone()
    eng.P.copy_(P0); eng.G.copy_(G0)
    opt2.step(clip_grad=CLIP)
    assert not torch.equal(Pc, P0)
    assert torch.equal(eng.P, Pc) and torch.equal(opt2.m, mc) and (vc is None or torch.equal(opt2.v, vc))

    # a state of another kind does not load
    other = create_optimizer(_args("adam" if kind != "adam" else "sgd"), s.model)
    with pytest.raises(RuntimeError, match=f"'{kind}'.*'{other.kind}'"):
        other.load_state_dict(st)
    with pytest.raises(RuntimeError, match=f"'{kind}'.*'adamw'"):
        create_optimizer(_args("adamw"), s.model).load_state_dict(st)


def test_skip_grad_gates_one_call_of_sgd():
    """`step(skip_grad=)` through the gate on an SGD kind: the gated call moves neither parameters nor the momentum buffer."""
    s = Setup("sgd")
    for step in range(3):
        s.backward(step)
        P0, m0 = s.model.engine.P.clone(), s.opt.m.clone()
        s.opt.step(skip_grad=1e-9 if step == 1 else 1e9)
        moved = not torch.equal(s.model.engine.P, P0)
        assert moved == (step != 1) and torch.equal(s.opt.m, m0) == (step == 1)
        assert float(s.model.engine.G.abs().max().item()) == 0.0
    assert s.opt.state_dict()["gated_total"] == 1 and s.opt.state_dict()["t"] == 2


# ---- 9. the training script ----------------------------------------------------------------------------------------------------
def test_training_script_sgd_layer_decay_ema_and_resume(tmp_path, capsys):
    """`run_training_egom2p.py --opt sgd --momentum 0.9 --layer_decay 0.75` (with --model_ema), 2 steps on synthetic clips: the
    log lists the groups and names the optimiser, the loss is finite; --resume restores the momentum buffer."""
    spec = importlib.util.spec_from_file_location("run_training_egom2p_kinds", os.path.join(ROOT, "run_training_egom2p.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    common = ["--model", "egom2p_tiny_6e_6d_swiglu_nobias", "--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze",
              "--num_input_tokens", "32", "--num_target_tokens", "32", "--batch_size", "4", "--epoch_size", "12",
              "--blr", "1e-1", "--print_freq", "1", "--seed", "3", "--max_steps", "2", "--opt", "sgd", "--momentum", "0.9",
              "--layer_decay", "0.75", "--model_ema", "--output_dir", str(tmp_path)]
    env_keys = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") if k in os.environ}
    seen = {}
    real = T.train_one_epoch

    def spy(model, loader, optimizer, *rest):
        seen["m_at_start"] = optimizer.m.clone()
        seen["opt"] = optimizer
        return real(model, loader, optimizer, *rest)

    try:
        T.main(T.get_args(common + ["--epochs", "1"]))
        out = capsys.readouterr().out
        ck = os.path.join(str(tmp_path), "checkpoint-0.pth")
        assert os.path.exists(ck)
        T.train_one_epoch = spy
        T.main(T.get_args(common + ["--epochs", "2", "--resume", ck]))
        out2 = capsys.readouterr().out
    finally:
        T.train_one_epoch = real
        os.environ.update(env_keys)
    line = next(ln for ln in out.splitlines() if ln.startswith("Param groups"))
    assert "optimizer nesterov" in line and "momentum 0.9" in line and "layer_13_decay" in line and "layer_0_decay" in line
    logged = [ln for ln in out.splitlines() if " group_lrs " in ln]
    assert len(logged) == 2
    lrs = dict(re.findall(r"(layer_\d+_\w+)=([0-9.e+-]+)", logged[0].split(" group_lrs ")[1]))
    assert len(lrs) == 2 * 14 - 1
    losses = [float(x) for x in re.findall(r"step \d+ loss ([0-9.eE+-]+|nan|inf)", out)]
    assert len(losses) == 2 and all(np.isfinite(losses))
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["optimizer"]["kind"] == "nesterov" and "v" not in saved["optimizer"] and saved["optimizer"]["t"] == 2
    assert "state_dict_ema" in saved and bool(saved["optimizer"]["m"].any())
    opt = seen["opt"]
    assert opt.kind == "nesterov" and opt.v is None and opt.t == 4
    assert torch.equal(seen["m_at_start"].cpu(), saved["optimizer"]["m"])        # the resumed run started from the saved buffer
    assert "resumed " in out2 and len(re.findall(r"step \d+ loss", out2)) == 2
