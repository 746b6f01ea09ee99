"""Golden vectors for the AdamW step gate from the REAL reference `NativeScalerWithGradNormCount`
(egom2p/utils/native_scaler.py:21-47, the `elif skip_grad is not None` branch :34-40) driving `torch.optim.AdamW` on the CPU in
fp32, `GradScaler(enabled=False)` as run_training_egom2p.py:518 makes it for bf16.

The reference's file is loaded by path (as tools/make_goldens_maskgit.py loads generate.py); only the data it produces is written.

Optimiser: lr 1e-3, betas (0.9, 0.95), eps 1e-8; a decay group (weight decay 0.05) of tensors with 1027 and 64 elements, a
no-decay group of tensors with 4099 and 3 elements.  The loss of call k is sum(p * g_k), so the gradient of call k is the seeded
g_k whatever the parameters are.  skip_grad = 200 in every call:

    calls 0, 1, 3, 5   g_k as drawn (norm 71-73)              stepped
    call 2             g_k * 40 (norm ~2900)                  skipped
    call 4             one element set to inf                 skipped (inf >= thr)
    call 6             one element set to NaN                 STEPPED (nan >= thr is false): the weights become NaN

The generator asserts these decisions and that a skipped call leaves parameters, moments and state["step"] untouched.

    python tools/make_goldens_skip_grad.py [path of the reference checkout]

Writes data only, to tests/golden/skip_grad.npz.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SIZES = {"decay0": 1027, "decay1": 64, "nodecay0": 4099, "nodecay1": 3}     # group = the name without its digit
LR, BETAS, EPS, WD, SKIP = 1e-3, (0.9, 0.95), 1e-8, 0.05, 200.0
N_CALLS, SEED = 7, 20
SCALED, INF_CALL, NAN_CALL = {2: 40.0}, 4, 6


def load_scaler(ref):
    spec = importlib.util.spec_from_file_location("ref_native_scaler", os.path.join(ref, "egom2p", "utils", "native_scaler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EGOM2P_REFERENCE", "/root/reference")
    NS = load_scaler(ref)
    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(SEED)
    params = {n: torch.randn(k, generator=gen, dtype=torch.float32).requires_grad_(True) for n, k in SIZES.items()}
    grads = []
    for k in range(N_CALLS):
        g = {n: torch.randn(sz, generator=gen, dtype=torch.float32) * SCALED.get(k, 1.0) for n, sz in SIZES.items()}
        if k == INF_CALL:
            g["decay0"][517] = float("inf")
        if k == NAN_CALL:
            g["nodecay0"][4097] = float("nan")
        grads.append(g)
    opt = torch.optim.AdamW([{"params": [params["decay0"], params["decay1"]], "weight_decay": WD},
                             {"params": [params["nodecay0"], params["nodecay1"]], "weight_decay": 0.0}], lr=LR, betas=BETAS, eps=EPS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaler = NS.NativeScalerWithGradNormCount(enabled=False)

    gold = {f"p0.{n}": p.detach().numpy().copy() for n, p in params.items()}
    norms, decisions, steps = [], [], []
    for k in range(N_CALLS):
        before = {n: p.detach().clone() for n, p in params.items()}
        state0 = {n: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in opt.state.get(p, {}).items()} for n, p in params.items()}
        loss = sum((p * grads[k][n]).sum() for n, p in params.items())
        norm = scaler(loss, opt, clip_grad=None, skip_grad=SKIP, parameters=list(params.values()), update_grad=True)
        for n, p in params.items():
            assert torch.equal(p.grad.isnan(), grads[k][n].isnan()) and torch.equal(p.grad.nan_to_num(0.0, 1.0, -1.0), grads[k][n].nan_to_num(0.0, 1.0, -1.0))
        step_now = [int(opt.state[p]["step"]) if p in opt.state and "step" in opt.state[p] else 0 for p in params.values()]
        skipped = all(torch.equal(p.detach(), before[n]) for n, p in params.items())
        if skipped:                                                # a skipped call leaves the whole optimiser state as it was
            for n, p in params.items():
                for kk, vv in state0[n].items():
                    assert torch.equal(torch.as_tensor(opt.state[p][kk]), torch.as_tensor(vv)), (k, n, kk)
        opt.zero_grad()                                            # run_training_egom2p.py:740-741
        norms.append(float(norm))
        decisions.append(int(skipped))
        steps.append(step_now)
        for n, p in params.items():
            gold[f"g{k}.{n}"] = grads[k][n].numpy().copy()
            gold[f"p{k + 1}.{n}"] = p.detach().numpy().copy()
        print(f"[goldens] call {k}: norm {float(norm):.4f} -> {'skipped' if skipped else 'stepped'}, state['step'] {step_now}", flush=True)
    assert decisions == [0, 0, 1, 0, 1, 0, 0], decisions
    assert all(s == 5 for s in steps[-1])
    assert any(bool(p.isnan().any()) for p in params.values())      # the NaN call was stepped
    gold["norms"] = np.array(norms, dtype=np.float32)
    gold["decisions"] = np.array(decisions, dtype=np.int32)
    gold["steps"] = np.array(steps, dtype=np.int32)                # [call, parameter] in the order of SIZES
    gold["meta"] = np.array(repr(dict(sizes=SIZES, lr=LR, betas=BETAS, eps=EPS, wd=WD, skip_grad=SKIP, calls=N_CALLS, seed=SEED)))
    path = os.path.join(GOLDEN, "skip_grad.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


if __name__ == "__main__":
    main()
