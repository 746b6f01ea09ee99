"""Optimiser side of the train loop over the engine's flat buffers.

Mirrors, for the hot path, `create_optimizer` / `get_parameter_groups` (egom2p/utils/optim_factory.py:97-230:
AdamW betas (0.9, 0.95), eps 1e-8, two groups - `no_decay` iff the name contains "norm." / ".norm" or
ends with ".bias") and `NativeScalerWithGradNormCount` (egom2p/utils/native_scaler.py:21-52: backward,
clip_grad_norm_, step).  The clip coefficient, the data-parallel 1/world factor and zero_grad are folded
into the AdamW kernel: gradients are read once and written once per step.  `skip_grad` (native_scaler.py:34-40)
and the opt-in guard against non-finite gradients are decided on the device (ops.adamw_gate): no host read.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops


def is_no_decay(name: str, skip_list=()) -> bool:
    """optim_factory.py:113"""
    return "norm." in name or ".norm" in name or name.endswith(".bias") or name in skip_list


def get_num_layer_for_fm(var_name: str, num_enc_layers: int, num_dec_layers: int, last_layer_mod_emb: bool = False) -> int:
    """Layer id of a parameter for layer-wise lr decay (optim_factory.py:62-79): 0 = the encoder embeddings, i + 1 = encoder block
    i, num_enc + j + 1 = decoder block j, num_enc + num_dec + 1 = everything behind the decoder.

    Restated as the reference BEHAVES on real parameter names, not as its docstring reads: it compares the whole name with
    ("encoder_norm", "decoder_proj_context", "mask_token"), so `encoder_norm.weight`, `decoder_proj_context.weight` and
    `decoder_proj_context.bias` never match and fall through to the LAST layer id; only `mask_token` (a bare name) gets
    num_enc.  `register_tokens` and the decoder embeddings' tables fall through as well.  Kept on purpose: a model fine-tuned here
    takes the lr scales it would take there."""
    if var_name.startswith("encoder_embeddings"):
        return 0
    if var_name.startswith("encoder."):
        return int(var_name.split(".")[1]) + 1
    if var_name in ("encoder_norm", "decoder_proj_context", "mask_token"):
        return num_enc_layers
    if not last_layer_mod_emb and var_name.startswith("decoder_embeddings.") and "mod_emb" in var_name:
        return num_enc_layers
    if var_name.startswith("decoder."):
        return num_enc_layers + int(var_name.split(".")[1]) + 1
    return num_enc_layers + num_dec_layers + 1


class LayerDecayValueAssigner:
    """optim_factory.py:82-88: `values[layer_id]` is the layer's lr scale."""

    def __init__(self, values):
        self.values = list(values)

    def get_scale(self, layer_id: int) -> float:
        return self.values[layer_id]


def layer_decay_values(layer_decay: float, num_layers: int) -> List[float]:
    """The scales of `--layer_decay`: layer_decay ** (L + 1 - i) for i in 0 .. L + 1 (the last layer id has scale 1)."""
    return [layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)]


def get_parameter_groups(model, weight_decay=1e-5, skip_list=(), get_num_layer=None, get_layer_scale=None, decoder_decay=None,
                         decoder_list=(), no_lr_scale_list=()):
    """The groups of optim_factory.py:97-154, in the order of first appearance: one per (layer id, weight-decay class), named
    `layer_%d_{decay,no_decay,decoder_decay}[_no_lr_scale]` (without a layer function: the bare class).  A group's lr_scale is the
    layer's (1.0 without a scale function and for `no_lr_scale_list` names).  Tensors with requires_grad=False are left out.
    Every group also lists its parameters' names (`param_names`), which the flat-buffer optimiser needs."""
    groups: Dict[str, Dict] = {}
    for name, param in model.named_parameters():
        name = name.replace("_fsdp_wrapped_module.", "")
        if not param.requires_grad:
            continue
        if is_no_decay(name, skip_list) or name.endswith((".lookup_table_weight", ".gamma")):
            cls, wd = "no_decay", 0.0
        elif decoder_decay is not None and (name.startswith("decoder.") or name in decoder_list):
            cls, wd = "decoder_decay", decoder_decay
        else:
            cls, wd = "decay", weight_decay
        layer_id, unscaled = None, False
        if get_num_layer is not None:
            layer_id = get_num_layer(name)
            cls = "layer_%d_%s" % (layer_id, cls)
            if name in no_lr_scale_list:
                unscaled = True
                cls += "_no_lr_scale"
        if cls not in groups:
            scale = get_layer_scale(layer_id) if get_layer_scale is not None and not unscaled else 1.0
            groups[cls] = {"name": cls, "weight_decay": wd, "params": [], "param_names": [], "lr_scale": scale}
        groups[cls]["params"].append(param)
        groups[cls]["param_names"].append(name)
    return list(groups.values())


def build_segments(offsets, never_grad, group_of, skipped, frozen):
    """Pure host logic of the segmented step.  offsets: engine key -> (offset, numel, shape) in flat order; group_of: engine key ->
    group index (a tensor in no group never steps); skipped: key -> optimiser steps the tensor sat out; frozen: keys that sit this
    phase out.  Returns segments (lo, hi, group, step offset, frozen): every tensor outside `never_grad` is covered exactly (padded
    to 4 floats, as the engine lays it out), ascending; neighbours merge only when they touch and agree in (group, offset, frozen)."""
    segs: List[List] = []
    for name, (o, n, _) in offsets.items():
        if name in never_grad:
            continue
        n4 = (n + 3) // 4 * 4
        fro = name in frozen or name not in group_of
        key = (0, 0, True) if fro else (group_of[name], skipped.get(name, 0), False)
        if segs and segs[-1][1] == o and tuple(segs[-1][2:]) == key:
            segs[-1][1] = o + n4
        else:
            segs.append([o, o + n4, *key])
    return [tuple(s) for s in segs]


def plan_launches(segments, max_groups: int = 128):
    """Segments -> launches: [(table rows (lo, hi, slot, flags), slots [(group, step offset), ...])].  A launch holds at most
    `max_groups` distinct (group, step offset) combinations - the kernel's hyper-parameter block; a frozen segment takes slot 0."""
    launches, rows, slots = [], [], {}
    for lo, hi, grp, sk, fro in segments:
        if not fro and (grp, sk) not in slots and len(slots) == max_groups:
            launches.append((rows, list(slots)))
            rows, slots = [], {}
        if fro:
            rows.append((lo, hi, 0, 1))
        else:
            rows.append((lo, hi, slots.setdefault((grp, sk), len(slots)), 0))
    if rows:
        launches.append((rows, list(slots)))
    return launches


class FusedAdamW:
    """Duck-types the torch optimiser surface the reference loop touches: `param_groups` (with "lr",
    "weight_decay", "lr_scale"), `step`, `zero_grad`, `state_dict`, `load_state_dict`.

    `param_groups` (optional): the groups of `get_parameter_groups` - any number, each with its own weight decay and lr_scale.
    Without it the optimiser has the two groups `decay` / `no_decay` and steps one launch per run of equal weight-decay class;
    with it every group, step offset and frozen range is a segment of ONE `ops.adamw_step_seg` launch."""

    kind = "adamw"                                 # `FusedOptimizer` below: "adam", "momentum", "nesterov"

    def __init__(self, engine, lr: float = 1e-4, weight_decay: float = 0.05, betas=(0.9, 0.95), eps: float = 1e-8,
                 named_parameters=None, world_size: int = 1, param_groups=None):
        self.engine = engine
        self.betas, self.eps = betas, eps
        self.world_size = world_size
        self.m = torch.zeros_like(engine.P)
        self.v = torch.zeros_like(engine.P) if self.kind not in ops.SGD_KINDS else None     # (SGD: `m` is the momentum buffer)
        self.sqnorm = torch.zeros(1, device=engine.dev, dtype=torch.float64)
        self.t = 0
        named = list(named_parameters) if named_parameters is not None else []
        self._named = named
        decay = [p for n, p in named if not is_no_decay(n)]
        nodecay = [p for n, p in named if is_no_decay(n)]
        self.param_groups: List[Dict] = [
            {"params": decay, "weight_decay": weight_decay, "lr": lr, "lr_scale": 1.0, "name": "decay"},
            {"params": nodecay, "weight_decay": 0.0, "lr": lr, "lr_scale": 1.0, "name": "no_decay"},
        ]
        self.segmented = param_groups is not None
        self._launches: List = []                  # segmented path: [(ops.AdamwSegTable, [(group index, step offset), ...])]
        if self.segmented:
            if not named:
                raise ValueError("FusedAdamW: parameter groups need named_parameters (tensors are placed by name)")
            name_of = {id(p): n for n, p in named}
            self.param_groups, self._group_of = [], {}
            for gi, src in enumerate(param_groups):
                names = list(src.get("param_names") or [name_of[id(p)] for p in src["params"]])
                grp = {"params": list(src["params"]), "param_names": names, "weight_decay": float(src.get("weight_decay", weight_decay)),
                       "lr": float(src.get("lr", lr)), "lr_scale": float(src.get("lr_scale", 1.0)), "name": src.get("name", f"group_{gi}")}
                self.param_groups.append(grp)
                for n in names:
                    key = engine._canon_key(n)
                    if key not in engine.offsets:
                        raise ValueError(f"FusedAdamW: parameter '{n}' of group '{grp['name']}' is not a tensor of this engine")
                    if self._group_of.setdefault(key, gi) != gi:
                        raise ValueError(f"FusedAdamW: parameter '{n}' is in two groups")
            known = {engine._canon_key(n) for n, _ in named} | set(engine.never_grad)
            stray = [k for k in engine.offsets if k not in known]
            if stray:
                raise ValueError(f"FusedAdamW: engine tensors without a named parameter: {stray[:4]}")
        self._frozen_sig = None
        self._runs = [(lo, hi, nd, 0) for lo, hi, nd in engine.opt_runs]
        self._frozen_ranges: List = []          # [lo, hi) ranges of the flat buffers that belong to frozen tensors
        self._frozen_names: List[str] = []
        # torch.optim.AdamW keeps state["step"] PER PARAMETER and skips parameters without a gradient (requires_grad=False), so a
        # tensor that is unfrozen after k steps (run_training_egom2p.py --frozen_model_epochs) starts its bias correction at 1,
        # not at k + 1: `skipped[name]` = optimiser steps the tensor sat out; its effective step is t - skipped[name]
        self.skipped: Dict[str, int] = {}
        self.last_grad_norm: Optional[torch.Tensor] = None
        # step gate (skip_grad / skip_nonfinite): the device counts the calls it gated (ops.GATE_WORDS int32, made at the first
        # gated-path call); `t` and `skipped` count EVERY call until `_fold_gated` subtracts the device's count from both
        self.gate: Optional[torch.Tensor] = None
        self._gate_pending = False                 # gated-path calls were issued since the last fold
        self._gated_base = 0                       # gated calls of a restored state (the device total restarts at 0)

    def _fold_gated(self):
        """One host read: take the calls the device gated since the last fold out of `t` and out of `skipped` of the tensors
        that were frozen meanwhile (a gated call counts for nobody, as torch's per-parameter state["step"] would have it).
        The frozen set is constant between two folds, so the arithmetic is exact.  Called only where a sync is harmless."""
        if not self._gate_pending:
            return
        c = int(self.gate[1].item())
        if c:
            self.t -= c
            for name in self._frozen_names:
                self.skipped[name] = self.skipped.get(name, 0) - c
            self.gate[1].zero_()
        self._gate_pending = False

    def gated_total(self) -> int:
        """Calls gated so far (one host read)."""
        return self._gated_base + (int(self.gate[2].item()) if self.gate is not None else 0)

    def _active_runs(self):
        """Honour requires_grad=False (freeze_* methods of the model): frozen tensors are left untouched."""
        if not self._named and not any(self.skipped.values()):
            return self._runs                       # (no tensor to freeze and none that sat steps out: the engine's own runs)
        sig = tuple(p.requires_grad for _, p in self._named)
        if sig != self._frozen_sig:
            self._fold_gated()                      # with the OLD frozen names, before the runs take their step offsets
            self._frozen_sig = sig
            if all(sig) and not any(self.skipped.values()):
                self._runs = [(lo, hi, nd, 0) for lo, hi, nd in self.engine.opt_runs]
                self._frozen_ranges, self._frozen_names = [], []
            else:
                eng, runs, fro, fnames = self.engine, [], [], []
                frozen = {eng._canon_key(n) for (n, p) in self._named if not p.requires_grad} | set(eng.never_grad)
                for name, (o, n, _) in eng.offsets.items():
                    n4 = (n + 3) // 4 * 4
                    if name in frozen:
                        fnames.append(name)
                        if fro and fro[-1][1] == o:
                            fro[-1][1] = o + n4
                        else:
                            fro.append([o, o + n4])
                        continue
                    nd, sk = is_no_decay(name), self.skipped.get(name, 0)
                    if runs and runs[-1][2] == nd and runs[-1][3] == sk and runs[-1][1] == o:
                        runs[-1][1] = o + n4
                    else:
                        runs.append([o, o + n4, nd, sk])
                self._runs = [tuple(r) for r in runs]
                self._frozen_ranges = [tuple(r) for r in fro]
                self._frozen_names = [n for n in fnames if n not in eng.never_grad]
        return self._runs

    def segments(self):
        """The segmented path's (lo, hi, group, step offset, frozen) runs for the present frozen set and step offsets."""
        eng = self.engine
        frozen = {eng._canon_key(n) for n, p in self._named if not p.requires_grad}
        return build_segments(eng.offsets, eng.never_grad, self._group_of, self.skipped, frozen)

    def _plan(self):
        """Segment tables of the segmented path, rebuilt (and uploaded) only when the frozen signature changes."""
        sig = tuple(p.requires_grad for _, p in self._named)
        if sig != self._frozen_sig:
            self._fold_gated()                      # with the OLD frozen names, before the segments take their step offsets
            self._frozen_sig = sig
            segs = self.segments()
            self._launches = [(ops.AdamwSegTable(rows, self.engine.dev), slots) for rows, slots in plan_launches(segs, ops.L.ADAMW_MAX_GROUPS)]
            self._runs = [(lo, hi, grp, sk) for lo, hi, grp, sk, fro in segs if not fro]
            self._frozen_ranges = [(lo, hi) for lo, hi, _, _, fro in segs if fro]
            eng = self.engine
            frozen = {eng._canon_key(n) for n, p in self._named if not p.requires_grad}
            self._frozen_names = [k for k in eng.offsets if k in frozen and k in self._group_of and k not in eng.never_grad]
        return self._launches

    @torch.no_grad()
    def step(self, clip_grad: Optional[float] = None, zero_grad: bool = True, skip_grad: Optional[float] = None,
             skip_nonfinite: bool = False):
        """One AdamW step on every (unfrozen) parameter.  Returns the global gradient norm (device tensor,
        of the world-averaged gradients, as clip_grad_norm_ would report it) if clipping or a gate was requested.

        skip_grad (native_scaler.py:34-40): the call updates nothing when norm >= skip_grad; skip_nonfinite: nor when the norm is
        inf or NaN (the reference steps on a NaN norm: `nan >= thr` is false).  Both are decided on the device; a gated call
        leaves parameters, moments and every tensor's step count as they were and still clears the gradients."""
        eng = self.engine
        if getattr(eng, "params_swapped", False):
            raise RuntimeError("FusedAdamW.step inside ModelEma.applied(): the flat buffer holds the averaged weights, "
                               "a step here would train the average")
        gated = skip_grad is not None or bool(skip_nonfinite)
        if skip_grad is not None and not skip_grad > 0:
            raise ValueError(f"skip_grad must be positive, got {skip_grad}")
        self.t += 1
        gscale = 1.0 / self.world_size
        norm = None
        launches = self._plan() if self.segmented else None
        runs = self._runs if self.segmented else self._active_runs()
        if clip_grad is not None or gated:
            # clip_grad_norm_ of the reference (native_scaler.py:33) sees only tensors that have a gradient: the engine's
            # backward writes every tensor's gradient, so frozen ranges are left out of the norm here
            self.sqnorm.zero_()
            if not self._frozen_ranges:
                ops.grad_sqnorm(eng.G, self.sqnorm)
            else:
                for lo, hi, _, _ in runs:
                    ops.grad_sqnorm(eng.G[lo:hi], self.sqnorm)
            norm = self.sqnorm.sqrt().to(torch.float32) * gscale
        if gated:
            if self.gate is None:
                self.gate = torch.zeros(ops.GATE_WORDS, device=eng.dev, dtype=torch.int32)
            ops.adamw_gate(self.sqnorm, self.gate, gscale=gscale, skip_norm=float(skip_grad) if skip_grad is not None else 0.0,
                           skip_nonfinite=skip_nonfinite)
            self._gate_pending = True
        if zero_grad and not self.segmented:
            for lo, hi in self._frozen_ranges:      # never consumed: must not accumulate from step to step
                eng.G[lo:hi].zero_()
        for name in self._frozen_names:             # this step passes them by, as torch's per-parameter step counter would
            self.skipped[name] = self.skipped.get(name, 0) + 1
        if self.segmented:
            # one launch (or the few the block's 128 slots force): frozen ranges are segments too, their gradients zeroed in-kernel
            for table, slots in launches:
                hp = [(float(self.param_groups[gi]["lr"]), float(self.param_groups[gi]["weight_decay"]), self.t - sk)
                      for gi, sk in slots] or [(0.0, 0.0, 1)]
                self._launch_seg(table, hp, gscale=gscale, max_norm=float(clip_grad) if clip_grad else 0.0,
                                 sqnorm=self.sqnorm if (clip_grad or gated) else None, zero_grad=zero_grad,
                                 gate=self.gate if gated else None)
            eng.weights_dirty = True
            self.last_grad_norm = norm
            return norm
        decay, nodecay = self.param_groups
        for lo, hi, nd, sk in runs:
            grp = nodecay if nd else decay
            if gated:
                ops.adamw_step_gated(eng.P[lo:hi], eng.G[lo:hi], self.m[lo:hi], self.v[lo:hi], float(grp["lr"]),
                                     float(grp["weight_decay"]), self.t - sk, self.gate, self.betas[0], self.betas[1], self.eps,
                                     gscale=gscale, max_norm=float(clip_grad) if clip_grad else 0.0, sqnorm=self.sqnorm,
                                     zero_grad=zero_grad)
                continue
            ops.adamw_step(eng.P[lo:hi], eng.G[lo:hi], self.m[lo:hi], self.v[lo:hi], float(grp["lr"]), float(grp["weight_decay"]),
                           self.t - sk, self.betas[0], self.betas[1], self.eps, gscale=gscale,
                           max_norm=float(clip_grad) if clip_grad else 0.0, sqnorm=self.sqnorm if clip_grad else None,
                           zero_grad=zero_grad)
        eng.weights_dirty = True
        self.last_grad_norm = norm
        return norm

    def _launch_seg(self, table, hp, **kw):
        eng = self.engine
        ops.adamw_step_seg(eng.P, eng.G, self.m, self.v, table, hp, self.betas[0], self.betas[1], self.eps, **kw)

    def zero_grad(self, set_to_none: bool = False):
        self.engine.G.zero_()

    def state_dict(self):
        # m / v are the engine's PHYSICAL flat layout (padded heads, padded F): `layout` names it so that a resume under another
        # layout (EGOM2P_HEAD_PAD, a round-3 ego-L checkpoint) fails with a message instead of a size mismatch or, worse, a fit
        self._fold_gated()                          # `t` and `skipped` leave as applied-step counts
        return {"m": self.m, "v": self.v, "t": self.t, "skipped": dict(self.skipped), "layout": self.engine.layout_tag(),
                "gated_total": self.gated_total(),
                "param_groups": [{k: v for k, v in g.items() if k not in ("params", "param_names")} for g in self.param_groups]}

    def load_state_dict(self, sd):
        if sd.get("kind", "adamw") != self.kind:
            raise RuntimeError(f"optimizer state was saved by the optimiser kind '{sd.get('kind', 'adamw')}', this optimiser is "
                               f"'{self.kind}' (--opt): their state buffers mean different things; build it with the same --opt, "
                               "or restart the optimizer state")
        moments = ("m",) if self.v is None else ("m", "v")
        have, want = sd.get("layout"), self.engine.layout_tag()
        if have is None:
            # (before round 5 the state carried no tag, and round 5 moved the decoder's context_norm weights inside the flat buffers:
            #  the element counts agree, the element ORDER does not - copying would misalign every moment behind `bridge` silently)
            raise RuntimeError("optimizer state without a storage-layout tag (saved before round 5): the flat parameter order changed since; "
                               "restart the optimizer state (the model state dict, keyed by name, still loads)")
        body = int(getattr(self.engine, "n_flat_body", want[1]))
        if (tuple(have) != tuple(want) and tuple(have[:1]) + tuple(have[2:]) == tuple(want[:1]) + tuple(want[2:])
                and int(have[1]) == body < int(want[1]) and sd["m"].numel() == body):
            # a run with fixed positional tables continued with learned ones: the learned tables lie behind everything the saved
            # state covers, so the saved moments are the head of this engine's; the tables start like any parameter new to AdamW -
            # zero moments, bias correction from step 1 (`skipped`, as for a tensor unfrozen later)
            for k in moments:
                getattr(self, k).zero_()
                getattr(self, k)[:body].copy_(sd[k])
            sd = dict(sd, layout=want, **{k: getattr(self, k) for k in moments},
                      skipped=dict(sd.get("skipped", {}), **{n: int(sd["t"]) for n in self.engine.offsets if n.endswith("pos_emb")}))
            have = want
        if tuple(have) != tuple(want):
            raise RuntimeError(f"optimizer state was saved for storage layout {tuple(have)}, this engine uses {tuple(want)} "
                               "(layout version, n_flat, D, heads stored, head pitch, padded F): resume with the same EGOM2P_HEAD_PAD / model, "
                               "or restart the optimizer state")
        if sd["m"].numel() != self.m.numel():
            raise RuntimeError(f"optimizer state has {sd['m'].numel()} moments, this engine {self.m.numel()} parameters")
        saved, mine = [s.get("name") for s in sd["param_groups"]], [g["name"] for g in self.param_groups]
        if saved != mine:
            raise RuntimeError(f"optimizer state was saved with the parameter groups {saved[:4]}{'...' if len(saved) > 4 else ''} "
                               f"({len(saved)}), this optimiser has {mine[:4]}{'...' if len(mine) > 4 else ''} ({len(mine)}): build it "
                               "with the same layer_decay / decoder_decay / no_lr_scale_list, or restart the optimizer state")
        for k in moments:
            getattr(self, k).copy_(sd[k])
        self.t = int(sd["t"])
        self.skipped = {str(k): int(v) for k, v in sd.get("skipped", {}).items()}
        # the restored counts are folded ones: whatever this optimiser's device block counted belongs to the state it replaces
        if self.gate is not None:
            self.gate.zero_()
        self._gate_pending = False
        self._gated_base = int(sd.get("gated_total", 0))
        self._frozen_sig = None                     # runs are rebuilt with the restored per-tensor step offsets
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)


class FusedOptimizer(FusedAdamW):
    """The other optimisers of the reference's `--opt` (optim_factory.py:217-224) on the segmented launch, `ops.optim_step_seg`:
    kind "adam" (torch.optim.Adam: the weight decay is added to the gradient), "momentum" (torch.optim.SGD with momentum) and
    "nesterov" (the same with nesterov=True).  Everything around the per-element rule is `FusedAdamW`'s: groups with lr /
    weight_decay / lr_scale, frozen ranges (out of the clip norm, gradients zeroed), the step gate, and for Adam the per-tensor
    step offsets.  Without `param_groups` the segment table is the two-group (decay / no_decay) one.
    State: Adam keeps `m` and `v`; the SGD kinds keep `m` alone - the momentum buffer - and allocate no `v` (4 B per parameter
    less).  A tensor that sat steps out starts from its zero buffer, as torch's SGD starts a parameter without state."""

    def __init__(self, engine, kind: str, lr: float = 1e-4, weight_decay: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 momentum: float = 0.9, named_parameters=None, world_size: int = 1, param_groups=None):
        if kind not in ops.OPT_KINDS:
            raise ValueError(f"FusedOptimizer: unknown kind '{kind}' (one of {sorted(ops.OPT_KINDS)}; AdamW is FusedAdamW)")
        if kind in ops.SGD_KINDS:
            if not momentum >= 0.0:                 # torch.optim.SGD's own refusals
                raise ValueError(f"Invalid momentum value: {momentum}")
            if kind == "nesterov" and momentum <= 0:
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.kind = kind
        self.momentum = float(momentum)
        named = list(named_parameters) if named_parameters is not None else []
        if param_groups is None:                    # FusedAdamW's default grouping, as a segment table
            if not named:
                raise ValueError("FusedOptimizer needs named_parameters (tensors are placed by name)")
            param_groups = [
                {"name": "decay", "weight_decay": weight_decay, "lr_scale": 1.0,
                 "params": [p for n, p in named if not is_no_decay(n)], "param_names": [n for n, _ in named if not is_no_decay(n)]},
                {"name": "no_decay", "weight_decay": 0.0, "lr_scale": 1.0,
                 "params": [p for n, p in named if is_no_decay(n)], "param_names": [n for n, _ in named if is_no_decay(n)]},
            ]
        super().__init__(engine, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, named_parameters=named,
                         world_size=world_size, param_groups=param_groups)

    def segments(self):
        if self.kind not in ops.SGD_KINDS:
            return super().segments()
        eng = self.engine                           # (no bias correction: a step offset does not split a segment)
        frozen = {eng._canon_key(n) for n, p in self._named if not p.requires_grad}
        return build_segments(eng.offsets, eng.never_grad, self._group_of, {}, frozen)

    def _launch_seg(self, table, hp, **kw):
        eng = self.engine
        ops.optim_step_seg(self.kind, eng.P, eng.G, self.m, self.v, table, hp, self.betas[0], self.betas[1], self.eps,
                           momentum=self.momentum, **kw)

    def state_dict(self):
        sd = super().state_dict()
        sd["kind"] = self.kind
        if self.v is None:                          # one buffer: `m`, the momentum buffer
            del sd["v"]
            sd["momentum"] = self.momentum
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)                 # (refuses a state of another kind)
        if self.v is None and "momentum" in sd:
            self.momentum = float(sd["momentum"])


def create_optimizer(args, model, get_num_layer=None, get_layer_scale=None, filter_bias_and_bn=True, skip_list=None):
    """`create_optimizer` of the reference (optim_factory.py:157-230).  `args.opt` picks the optimiser as there (:214-229, the part
    behind the last "_"): `sgd` / `nesterov` -> SGD with Nesterov momentum, `momentum` -> SGD with plain momentum (both read
    `args.momentum` and drop eps), `adam` -> Adam, `adamw` -> AdamW; anything else is a ValueError.  `get_num_layer` (name -> layer
    id) and `get_layer_scale` (layer id -> lr scale) give layer-wise lr decay; `args.decoder_decay` (a weight decay of its own for
    names starting `decoder.`) and `args.no_lr_scale_list` ("a-b-c": names that keep scale 1) are read as the reference reads them
    (:163-170).  With none of them AdamW is the two-group optimiser on its per-run launches; the other kinds always step on the
    segmented launch, over the same two groups."""
    opt = getattr(args, "opt", "adamw").lower().split("_")[-1]
    kind = {"sgd": "nesterov", "nesterov": "nesterov", "momentum": "momentum", "adam": "adam", "adamw": "adamw"}.get(opt)
    if kind is None:
        raise ValueError(f"Invalid optimizer '{args.opt}': one of sgd, nesterov, momentum, adam, adamw (optim_factory.py:217-229)")
    betas = tuple(args.opt_betas) if getattr(args, "opt_betas", None) else (0.9, 0.999)
    eps = args.opt_eps if getattr(args, "opt_eps", None) else 1e-8
    world = torch.distributed.get_world_size() if torch.distributed.is_available() and torch.distributed.is_initialized() else 1
    decoder_decay = getattr(args, "decoder_decay", None)
    no_lr_scale = getattr(args, "no_lr_scale_list", None)
    no_lr_scale = no_lr_scale.split("-") if isinstance(no_lr_scale, str) else []
    groups = None
    if not (args.weight_decay and filter_bias_and_bn):
        if get_num_layer is not None or get_layer_scale is not None or decoder_decay is not None:
            # (the reference hands AdamW the bare parameter list here, :183-186, and the layer functions are silently dropped)
            raise ValueError("layer-wise lr decay / decoder_decay need weight_decay > 0 and filter_bias_and_bn=True: "
                             "the reference builds no parameter groups otherwise")
        if not filter_bias_and_bn:                 # (:184-186: one group, the weight decay on every tensor)
            kept = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
            groups = [{"name": "all", "params": [p for _, p in kept], "param_names": [n for n, _ in kept],
                       "weight_decay": args.weight_decay, "lr_scale": 1.0}]
    elif get_num_layer is not None or get_layer_scale is not None or decoder_decay is not None or skip_list:
        skip = skip_list if skip_list is not None else (model.no_weight_decay() if hasattr(model, "no_weight_decay") else ())
        dec = model.decoder_weight_decay() if hasattr(model, "decoder_weight_decay") else ()
        groups = get_parameter_groups(model, args.weight_decay, skip, get_num_layer, get_layer_scale, decoder_decay, dec, no_lr_scale)
    if kind != "adamw":
        return FusedOptimizer(model.engine, kind, lr=args.lr, weight_decay=args.weight_decay, betas=betas, eps=eps,
                              momentum=getattr(args, "momentum", 0.9), named_parameters=model.named_parameters(), world_size=world,
                              param_groups=groups)
    return FusedAdamW(model.engine, lr=args.lr, weight_decay=args.weight_decay, betas=betas, eps=eps,
                      named_parameters=model.named_parameters(), world_size=world, param_groups=groups)


class NativeScalerWithGradNormCount:
    """bf16 needs no loss scaling (GradScaler disabled at run_training_egom2p.py:518); same call surface."""
    state_dict_key = "amp_scaler"

    def __init__(self, enabled: bool = False, skip_nonfinite: bool = False):
        self.enabled = enabled
        self.skip_nonfinite = bool(skip_nonfinite)     # not in the reference: pass a call whose gradient norm is inf / NaN by

    def __call__(self, loss, optimizer, clip_grad=None, skip_grad=None, parameters=None, create_graph=False,
                 update_grad=True, compute_grad_norm=True):
        loss.backward()
        norm = None
        if update_grad:
            kw = {}
            if clip_grad is None and skip_grad is not None:       # native_scaler.py:30-40: clip_grad set -> skip_grad is ignored
                kw["skip_grad"] = skip_grad
            if self.skip_nonfinite:
                kw["skip_nonfinite"] = True
            norm = optimizer.step(clip_grad=clip_grad if clip_grad is not None else (1e30 if compute_grad_norm and not kw else None), **kw)
        return norm

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass
