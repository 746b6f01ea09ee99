"""Moving average of the model weights on the device: `ModelEmaV2` of the reference (egom2p/utils/timm/model_ema.py:84-149:
`ema = decay * ema + (1 - decay) * model` after every optimiser step, `state_dict_ema` in the checkpoint) over the engine's
flat fp32 parameter buffer.

The reference deep-copies the module and evaluates the copy.  Here parameters are views of ONE buffer (`engine.P`), the bf16 /
fp8 weight copies are derived from it, and captured generation graphs hold raw pointers into both: the average is a second
flat buffer, one kernel updates it (`ops.ema_update`, 12 B per parameter), and evaluating with it means EXCHANGING the
contents of the two buffers in place (`ops.swap_f32`) - no pointer changes, so views and graphs stay valid.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict

import torch

from . import ops


def host_copy(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A state dict cloned to the host.  Entries that are one tensor on the device (tied `token_emb` / `to_logits`, a shared
    `mod_emb`, the zero norm biases) stay one tensor: torch.save then writes them once, as it does for the model's own."""
    seen, out = {}, {}
    for k, v in sd.items():
        ident = (v.data_ptr(), tuple(v.shape), tuple(v.stride()))
        if ident not in seen:
            seen[ident] = v.detach().to("cpu", copy=True)
        out[k] = seen[ident]
    return out


class ModelEma:
    def __init__(self, model_or_engine, decay: float = 0.9999, warmup: bool = False):
        decay = float(decay)
        if math.isnan(decay) or not 0.0 <= decay <= 1.0:
            raise ValueError(f"ModelEma: decay must lie in [0, 1], got {decay}")
        self.model = model_or_engine if hasattr(model_or_engine, "engine") else None
        self.engine = model_or_engine.engine if self.model is not None else model_or_engine
        self.decay, self.warmup = decay, bool(warmup)
        self.num_updates = 0
        if getattr(self.engine, "params_swapped", False):
            raise RuntimeError("ModelEma: the engine's parameters are exchanged with another average (inside applied())")
        self.ema = self.engine.P.clone()                 # the reference's deepcopy(model) (model_ema.py:111)
        self._applied = False

    def decay_at(self, k: int) -> float:
        """The decay of update number k (k updates done so far); host arithmetic in double.  With warm-up: timm's later rule
        min(decay, (1 + k) / (10 + k)), so that a short run does not keep its initial weights."""
        if not self.warmup:
            return self.decay
        return min(self.decay, (1.0 + k) / (10.0 + k))

    @torch.no_grad()
    def update(self):
        """model_ema.py:128-129, one launch over the flat buffer (pads are 0 in both buffers and stay 0; a frozen tensor's average
        stays at its value).  Called after every optimiser call, also one the step gate passed by: no host read."""
        if self._applied:
            raise RuntimeError("ModelEma.update inside applied(): the buffers are exchanged")
        ops.ema_update(self.ema, self.engine.P, self.decay_at(self.num_updates))
        self.num_updates += 1

    @torch.no_grad()
    def set(self):
        """model_ema.py:131-132"""
        if self._applied:
            raise RuntimeError("ModelEma.set inside applied(): the buffers are exchanged")
        self.ema.copy_(self.engine.P)

    @contextlib.contextmanager
    def applied(self):
        """The model computes with the averaged weights inside: the contents of `engine.P` and of the average are exchanged on
        entry and exchanged back on exit; the bf16 / fp8 copies are rebuilt at the next forward (`weights_dirty`)."""
        eng = self.engine
        if self._applied or getattr(eng, "params_swapped", False):
            raise RuntimeError("ModelEma.applied() does not nest: the averaged weights are already applied")
        ops.swap_f32(eng.P, self.ema)
        eng.weights_dirty = True
        eng.params_swapped = self._applied = True
        try:
            yield self
        finally:
            ops.swap_f32(eng.P, self.ema)
            eng.weights_dirty = True
            eng.params_swapped = self._applied = False

    def _holder(self):
        return self.model if self.model is not None else self.engine

    @torch.no_grad()
    def state_dict(self) -> Dict:
        """`state_dict_ema`: the keys and shapes of the model's own state dict (name-keyed: loadable under another storage
        layout), on the host; and the three scalars."""
        with self.applied():
            sd = host_copy(self._holder().state_dict())
        return {"state_dict_ema": sd, "decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict):
        with self.applied():
            self._holder().load_state_dict(sd["state_dict_ema"])
        self.decay, self.warmup = float(sd.get("decay", self.decay)), bool(sd.get("warmup", self.warmup))
        self.num_updates = int(sd.get("num_updates", 0))
