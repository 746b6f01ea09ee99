"""Write the flat parameter layout of symmetric, shared-embedding configurations to tests/golden/layout_symmetric.json:
offsets, all-reduce buckets, optimiser runs and the layout tag, as `Engine._build_params` lays them out.  Run on the commit whose
layout is to be pinned (tests/test_asym_layout_cpu.py compares the current code against the file); needs no GPU.

    python tools/snapshot_layout.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egom2p_amd.config import MODEL_CFGS      # noqa: E402
from egom2p_amd.engine import Engine          # noqa: E402

NAMES = ("ego_384_2e_2d_causal", "ego_b_2e_2d_untied", "ego_gen_384_2e_2d_reg4", "ego_384_2e_2d_gelu", "ego_384_2e_2d_qknorm",
         "ego_tiny8_2e_2d", "ego_L_1020_2e_2d")


def layout(name):
    eng = Engine(MODEL_CFGS[name], device="cpu", max_batch=1, n_enc=8, n_dec=8)
    return {"offsets": {k: [int(o), int(n), list(s)] for k, (o, n, s) in eng.offsets.items()},
            "buckets": [[n, int(a), int(b)] for n, a, b in eng.buckets],
            "opt_runs": [[int(a), int(b), bool(nd)] for a, b, nd in eng.opt_runs],
            "layout_tag": list(eng.layout_tag()),
            "never_grad": sorted(eng.never_grad),
            "state_dict_keys": list(eng.state_dict().keys())}


if __name__ == "__main__":
    out = {n: layout(n) for n in NAMES}
    path = os.path.join(ROOT, "tests", "golden", "layout_symmetric.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
