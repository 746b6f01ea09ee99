"""fp64 numpy restatement of the per-element update rules of `ops.optim_step_seg` (ego_optim_step_seg) and, as the yardstick of its
arithmetic class, of `ops.adamw_step_seg`.  tests/test_optim_kinds_cpu.py holds the three new rules to torch.optim.SGD / Adam in
float64; the GPU tests (tests/test_optim_kinds_gpu.py) compare the kernels against it.

    adam      d = g coef + wd p;  m = b1 m + (1 - b1) d;  v = b2 v + (1 - b2) d d;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
    momentum  d = g coef + wd p;  m = momentum m + d;  p -= lr m
    nesterov  d, m as momentum;   p -= lr (d + momentum m)
    adamw     p *= 1 - lr wd;  m, v from g coef alone;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)      (decoupled decay)
"""
import numpy as np

KINDS = ("adam", "momentum", "nesterov")


def clip_coef(sqnorm, gscale=1.0, max_norm=0.0):
    """The factor the kernels put on every raw gradient: gscale * min(1, max_norm / (sqrt(sqnorm) * gscale + 1e-6))."""
    coef = float(gscale)
    if max_norm > 0.0 and sqnorm is not None:
        coef *= min(1.0, max_norm / (float(np.sqrt(sqnorm)) * gscale + 1e-6))
    return coef


def step(kind, p, g, m, v, lr, wd, t=1, momentum=0.0, b1=0.9, b2=0.999, eps=1e-8, coef=1.0):
    """One step in float64 on arrays of any shape: returns the new (p, m, v); v passes through (None allowed) for the SGD kinds,
    whose `m` is the momentum buffer.  t: the step count of the bias corrections (Adam kinds)."""
    p, g, m = (np.asarray(x, dtype=np.float64) for x in (p, g, m))
    ge = g * coef
    if kind in ("momentum", "nesterov"):
        d = ge + wd * p
        m = momentum * m + d
        u = d + momentum * m if kind == "nesterov" else m
        return p - lr * u, m, v
    v = np.asarray(v, dtype=np.float64)
    bc1, bc2_sqrt = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    if kind == "adamw":
        p = p * (1.0 - lr * wd)
        d = ge
    elif kind == "adam":
        d = ge + wd * p
    else:
        raise ValueError(kind)
    m = b1 * m + (1.0 - b1) * d
    v = b2 * v + (1.0 - b2) * d * d
    return p - (lr / bc1) * (m / (np.sqrt(v) / bc2_sqrt + eps)), m, v


def fits_fp32(*arrays):
    """Every value of every fp64 array is a float32 number (the exact cases: no step may round)."""
    return all(np.array_equal(np.asarray(a, np.float64), np.asarray(a, np.float64).astype(np.float32).astype(np.float64)) for a in arrays)


# ---- the exact case of the SGD kinds: 8200 floats, five segments, operands in eighths ------------------------------------------
# (lo, hi, group, frozen): 4 | 4092 | 4096 (one whole chunk) | 4 frozen | 4 in no segment
EXACT_N = 8200
EXACT_ROWS = [(0, 4, 0, False), (4, 4096, 1, False), (4096, 8192, 0, False), (8192, 8196, 1, True)]
EXACT_HP = [(0.25, 0.5), (0.5, 0.25)]              # (lr, wd) of group 0 and 1
EXACT_MOMENTUM, EXACT_STEPS = 0.5, 3


def exact_inputs(seed=0):
    """p, buf: k / 8 with |k| <= 8; g[step]: k / 8 with |k| <= 8 - float64 arrays that hold fp32-exact values."""
    rng = np.random.default_rng(seed)
    draw = lambda: rng.integers(-8, 9, EXACT_N).astype(np.float64) / 8.0
    return draw(), [draw() for _ in range(EXACT_STEPS)], draw()


def exact_run(kind, p, gs, buf):
    """The restatement over the exact case: [(p, buf) after step 1, 2, 3] and whether every intermediate that the kernel rounds
    (d, the new buffer, the Nesterov sum, the new p) stayed a float32 number."""
    p, buf = p.copy(), buf.copy()
    out, exact = [], True
    for g in gs:
        for lo, hi, grp, frozen in EXACT_ROWS:
            if frozen:
                continue
            lr, wd = EXACT_HP[grp]
            s = slice(lo, hi)
            d = g[s] + wd * p[s]
            nb = EXACT_MOMENTUM * buf[s] + d
            u = d + EXACT_MOMENTUM * nb
            np_, nm, _ = step(kind, p[s], g[s], buf[s], None, lr, wd, momentum=EXACT_MOMENTUM)
            exact = exact and fits_fp32(d, nb, u, np_, nm)
            p[s], buf[s] = np_, nm
        out.append((p.copy(), buf.copy()))
    return out, exact
