"""ROAR / MaskGIT + classifier-free-guidance generation over the HIP engine (BASELINE config 4).

Mirrors the part of `egom2p/models/generate.py` the reference's eval scripts use
(`eval_model_rgb2depth.py:43-96`): `build_chained_generation_schedules` (:197-322),
`init_empty_target_modality` (:83-115), `init_full_input_modality` (:117-151), `empty_img_modality`
(:30-37) and `GenerationSampler.generate` (:1031-1099) for token modalities with the two parallel-decoding schemes
'roar' (`roar_step_batched` :768-783, `guided_roar_step_batched` :785-817) and 'maskgit' (`maskgit_step_batched` :652-665,
`guided_maskgit_step_batched` :667-705), with or without guidance; chained schedules may mix the two.  Autoregressive text
and multi-guided generation are outside the hot-path scope and raise.

Per schedule step: two encoder-decoder passes on the engine (conditional / unconditional; the
unconditional one sees an empty context on the first step), then ONE HIP kernel per step does the CFG
mix, nucleus filtering, temperature softmax and sampling for all rows (`ego_sample_cfg_topp`).  The
random ROAR order and the sampling uniforms come from torch's generator seeded with `seed + step`
like the reference (:1050, :484-485); they are explicit inputs of the kernels, so a test can pin them.

A MaskGIT step decodes ALL open target positions (`ego_maskgit_positions`: open positions ascending, :463-467), samples a token
for each with the same sampler kernel - which also returns the sampled token's probability - and commits the `num_tokens`
rows of largest probability (`ego_maskgit_select`: no sort; ties go to the lower decoder row).  Its only random
numbers are the sampling uniforms.

A model with `decoder_causal_mask=True` generates exactly like a standard one: the reference's ROAR and MaskGIT passes hand
`forward_decoder` no self-attention mask (`sa_mask=None`, :644, :761; `forward_mask_decoder_{maskgit,roar}` :447-516 build none),
so the flag only shapes the training forward.
"""
from __future__ import annotations

import copy
import math
from typing import List, Optional

import numpy as np
import torch

from . import ops


# ---------------------------------------------------------------------------------------------- schedules
def linear_schedule(num_steps: int, total_tokens: int) -> np.ndarray:
    """egom2p/utils/generation.py: tokens per step, descending, zeros trimmed."""
    edges = np.linspace(0, total_tokens, num_steps + 1, dtype=int)
    steps = np.sort(np.diff(edges))[::-1]
    return np.trim_zeros(steps, "b")


def cosine_schedule(num_steps: int, total_tokens: int) -> np.ndarray:
    s = np.array([0.5 * (1 + math.cos(math.pi * i / num_steps)) for i in range(num_steps)])
    toks = [round(total_tokens * d) for d in (s[:-1] - s[1:])]
    toks.append(total_tokens - sum(toks))
    return np.array(toks)


def linear_temp_schedule(temp: float, token_schedule: np.ndarray) -> np.ndarray:
    """egom2p/utils/generation.py:97-99: the temperature decays with the share of tokens still to decode"""
    return np.concatenate([np.array([temp * 1.0]), (temp * (token_schedule.sum() - token_schedule.cumsum()) / token_schedule.sum())[:-1]]).clip(min=1e-9)


def onex_temp_schedule(max_t: float, min_t: float, token_schedule: np.ndarray, power: float = 0.5, min_linspace: float = 1,
                       max_linspace: float = 100) -> np.ndarray:
    """egom2p/utils/generation.py:83-94 (`onex:{min_t}:{power}`): 1 / x^power over the token count, rescaled to [0, 1], times the
    share of tokens still to decode after each step"""
    x = np.linspace(min_linspace, max_linspace, num=sum(token_schedule))
    y = 1 / (x ** power)
    y = y - min(y)
    y = y / max(y)
    cs = np.cumsum(token_schedule) / np.sum(token_schedule)
    unscaled = [(1 - c) * u for u, c in zip(y, cs)]
    return np.array([min_t + (max_t - min_t) * u for u in unscaled]).clip(min=1e-9)


def build_chained_generation_schedules(cond_domains: List[str], target_domains: List[str], tokens_per_target: List[int],
                                       autoregression_schemes: List[str], decoding_steps: List[int],
                                       token_decoding_schedules: List[str], temps: List[float], temp_schedules: List[str],
                                       cfg_scales: List[float], cfg_schedules: List[str], cfg_grow_conditioning: bool = False,
                                       modality_info: Optional[dict] = None) -> List[dict]:
    out, cond = [], list(cond_domains)
    for i, target in enumerate(target_domains):
        scheme, ntoks = autoregression_schemes[i], tokens_per_target[i]
        if scheme == "roar":
            sched = linear_schedule(decoding_steps[i], ntoks)
        elif scheme == "maskgit":
            if token_decoding_schedules[i] == "cosine":
                sched = cosine_schedule(decoding_steps[i], ntoks)
            elif token_decoding_schedules[i] == "linear":
                sched = linear_schedule(decoding_steps[i], ntoks)
            else:
                raise ValueError(f"Illegal MaskGIT token schedule {token_decoding_schedules[i]}")      # the reference's messages (:271, :277)
        elif scheme == "autoregressive":
            raise NotImplementedError(f"scheme {scheme} is outside the hot-path scope")
        else:
            raise ValueError(f"Illegal decoding scheme {scheme}")
        if temp_schedules[i] == "constant":
            t_s = temps[i] * np.ones(decoding_steps[i])
        elif temp_schedules[i] == "linear":
            t_s = linear_temp_schedule(temps[i], sched)
        elif "onex" in temp_schedules[i]:
            # formatted like onex:{min_t}:{power} (:284-287)
            min_t, power = [float(f) for f in temp_schedules[i].split(":")[1:]]
            t_s = onex_temp_schedule(max_t=temps[i], min_t=min_t, token_schedule=sched, power=power)
        else:
            raise ValueError(f"Illegal temperature schedule {temp_schedules[i]}")                        # (:289)
        if cfg_schedules[i] == "cosine":
            raise NotImplementedError(f"guidance schedule {cfg_schedules[i]}")                          # the reference raises too (:298)
        if cfg_schedules[i] != "constant":
            raise ValueError(f"Illegal guidance schedule {cfg_schedules[i]}")                           # (:300)
        c_s = cfg_scales[i] * np.ones(decoding_steps[i])
        for tok, t, c in zip(sched, t_s, c_s):
            out.append({"target_domain": target, "scheme": scheme, "num_tokens": int(tok), "temperature": float(t),
                        "cfg_scale": float(c), "cfg_cond_domains": list(cond)})
        if cfg_grow_conditioning:
            cond.append(target)
    return out


# ---------------------------------------------------------------------------------------------- mod_dict helpers
def empty_img_modality(mod_dict, key):
    mod_dict[key]["input_mask"][:] = True
    mod_dict[key]["target_mask"][:] = False
    return mod_dict


def init_empty_target_modality(mod_dict, modality_info, domain, batch_size, num_tokens, device):
    if modality_info[domain]["type"] not in ("img", "gaze", "cam", "keypoints"):
        raise NotImplementedError("sequence modalities are outside the hot-path scope")
    mod_dict[domain] = {"tensor": torch.zeros((batch_size, num_tokens), dtype=torch.int64, device=device),
                        "input_mask": torch.ones((batch_size, num_tokens), dtype=torch.bool, device=device),
                        "target_mask": torch.zeros((batch_size, num_tokens), dtype=torch.bool, device=device)}
    return empty_img_modality(mod_dict, domain)


def init_full_input_modality(mod_dict, modality_info, domain, device, eos_id=3):
    if modality_info[domain]["type"] not in ("img", "gaze", "cam", "keypoints"):
        raise NotImplementedError("sequence modalities are outside the hot-path scope")
    d = mod_dict[domain]
    shape = (d["tensor"].shape[0], int(np.prod(d["tensor"].shape[1:])))
    d.setdefault("input_mask", torch.zeros(shape, dtype=torch.bool, device=device))
    d.setdefault("target_mask", torch.ones(shape, dtype=torch.bool, device=device))
    d.setdefault("decoder_attention_mask", torch.zeros(shape, dtype=torch.bool, device=device))
    d["input_mask"][:] = False
    d["target_mask"][:] = True
    return mod_dict


# ---------------------------------------------------------------------------------------------- sampler
class GenerationSampler:
    def __init__(self, model, use_graphs: bool = False):
        self.model = model
        self.engine = model.engine if hasattr(model, "engine") else model
        self.use_graphs = use_graphs           # replay each encoder-decoder pass from a captured hipGraph

    # one encoder-decoder pass (forward_enc_dec_roar_batched, generate.py:747-766) ---------------------
    def _enc_inputs(self, mod_dict, n_enc: Optional[int] = None):
        eng = self.engine
        enc = {}
        for m in eng.enc_mods:                 # (encoder modalities only, generate.py:749-751: a decoder-only target never re-enters)
            if m.name not in mod_dict:
                continue
            d = mod_dict[m.name]
            B = d["tensor"].shape[0]
            ids = d["tensor"].reshape(B, -1).to(eng.dev, torch.int64)
            mask = d["input_mask"].reshape(B, -1).to(eng.dev, torch.bool)
            enc[m.name] = (ids, mask)
        # rows kept by forward_mask_encoder_generation = max unmasked count over the batch (:413-415)
        if n_enc is None:
            n_enc = int(torch.stack([(~v[1]).sum(1) for v in enc.values()]).sum(0).max().item()) if enc else 0
        return enc, n_enc

    def _logits(self, mod_dict, target_mod, mod_pos, n_enc: Optional[int] = None, ws: Optional[dict] = None):
        """n_enc given: no host sync (the caller knows the kept-row count, e.g. from the schedule); ws: workspace to use."""
        eng = self.engine
        enc, n_enc = self._enc_inputs(mod_dict, n_enc)
        if ws is not None:
            return eng.infer_logits(enc, n_enc, target_mod, mod_pos, ws=ws)
        if self.use_graphs:
            return eng.infer_logits_graphed(enc, n_enc, target_mod, mod_pos).clone()
        return eng.infer_logits(enc, n_enc, target_mod, mod_pos)

    def roar_order(self, target_mask: torch.Tensor, num_select: int, seed: Optional[int], noise: Optional[torch.Tensor] = None,
                   n_dec: Optional[int] = None) -> torch.Tensor:
        """Positions decoded in this step (forward_mask_decoder_roar, :481-516): unmasked targets in a random
        order shared by the batch, the first `num_select` of them.  `noise` ([T] uniforms) / `n_dec` given: nothing
        is drawn or read back here (graph capture)."""
        dev = target_mask.device
        if noise is None:
            if seed is not None:
                torch.manual_seed(seed)
            noise = torch.rand(target_mask.shape[1], device=dev)
        if n_dec is None:
            n_dec = min(int(num_select), int((~target_mask[0]).sum().item()))
        ids_shuffle = torch.argsort(target_mask.float() + noise.unsqueeze(0) * 1e-6, dim=1)
        return ids_shuffle[:, :n_dec]

    def _step_logits(self, mod_dict, target_mod, mod_pos, conditioning, guidance_scale, static: Optional[dict]):
        """The encoder-decoder passes of one schedule step over the decoder rows `mod_pos`: the conditional pass and, when
        guided, the unconditional one (conditioning modalities emptied) - as one paired decoder pass where the engine allows."""
        eng = self.engine
        st = static or {}
        guided = guidance_scale != 1.0 and len(conditioning) > 0
        uncond = None
        if guided:
            uncond = {k: {kk: vv.clone() for kk, vv in v.items()} for k, v in mod_dict.items()}
            for mod in conditioning:
                uncond = empty_img_modality(uncond, mod)
        ws = st.get("ws")
        pair = guided and getattr(eng, "cfg_pair", False) and (ws is None or ws.get("groups", 1) >= 2)
        logits_uncond = None
        if pair:
            # the two passes of a guided step decode the same rows: one decoder pass over both contexts (engine.infer_logits_cfg)
            enc_c, n_c = self._enc_inputs(mod_dict, st.get("n_enc_cond"))
            enc_u, n_u = self._enc_inputs(uncond, st.get("n_enc_uncond"))
            pair = n_c > 0
        if pair and ws is None and self.use_graphs:
            logits_cond, logits_uncond = (t.clone() for t in eng.infer_logits_cfg_graphed(enc_c, n_c, enc_u, n_u, target_mod, mod_pos))
        elif pair:
            logits_cond, logits_uncond = eng.infer_logits_cfg(enc_c, n_c, enc_u, n_u, target_mod, mod_pos, ws=ws)
        else:
            logits_cond = self._logits(mod_dict, target_mod, mod_pos, n_enc=st.get("n_enc_cond"), ws=ws)
            if static is not None:
                logits_cond = logits_cond.clone()
            if guided:
                logits_uncond = self._logits(uncond, target_mod, mod_pos, n_enc=st.get("n_enc_uncond"), ws=ws)
        return logits_cond, logits_uncond

    def roar_step(self, mod_dict, target_mod, num_select, temperature, top_k, top_p, conditioning=(), guidance_scale=1.0,
                  seed=None, mod_pos: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
                  return_logits: bool = False, forced_samples: Optional[torch.Tensor] = None,
                  static: Optional[dict] = None):
        """static (graph capture): {"noise", "n_dec", "n_enc_cond", "n_enc_uncond", "ws"} - every count comes from the
        schedule, every random number from a buffer filled before the replay: no host sync, no generator call."""
        eng = self.engine
        st = static or {}
        d = mod_dict[target_mod]
        if mod_pos is None:
            mod_pos = self.roar_order(d["target_mask"].to(eng.dev), num_select, seed, noise=st.get("noise"), n_dec=st.get("n_dec"))
        mod_pos = mod_pos.to(eng.dev)
        logits_cond, logits_uncond = self._step_logits(mod_dict, target_mod, mod_pos, conditioning, guidance_scale, static)
        B, M, V = logits_cond.shape
        if uniforms is None:
            uniforms = torch.rand(B * M, device=eng.dev)
        samples = torch.empty(B * M, device=eng.dev, dtype=torch.int32)
        ops.sample_cfg_topp(logits_cond.view(B * M, V), None if logits_uncond is None else logits_uncond.view(B * M, V), V,
                            float(guidance_scale), float(top_p), float(temperature), uniforms, samples, ld=V,
                            top_k=ops.top_k_count(top_k, V))          # int: a count, float: a share of V (generate.py:335-342)
        samples = samples.view(B, M).to(torch.int64)
        drawn = samples
        if forced_samples is not None:             # teacher forcing for parity tests: scatter the given tokens instead
            samples = forced_samples.to(eng.dev, torch.int64).view(B, M)
        d["tensor"] = torch.scatter(d["tensor"].reshape(B, -1).to(eng.dev), -1, mod_pos, samples)
        d["input_mask"] = torch.scatter(d["input_mask"].to(eng.dev), -1, mod_pos, torch.zeros_like(samples, dtype=torch.bool))
        d["target_mask"] = torch.scatter(d["target_mask"].to(eng.dev), -1, mod_pos, torch.ones_like(samples, dtype=torch.bool))
        if return_logits:
            return mod_dict, dict(logits_cond=logits_cond, logits_uncond=logits_uncond, mod_pos=mod_pos, samples=drawn)
        return mod_dict

    def maskgit_step(self, mod_dict, target_mod, num_select, temperature, top_k, top_p, conditioning=(), guidance_scale=1.0,
                     seed=None, mod_pos: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
                     return_logits: bool = False, forced_samples: Optional[torch.Tensor] = None,
                     forced_probs: Optional[torch.Tensor] = None, static: Optional[dict] = None):
        """One MaskGIT step (maskgit_step_batched :652-665, guided_maskgit_step_batched :667-705): every open target position is
        decoded (`ego_maskgit_positions`: open positions ascending, as many rows as sample 0 has open, :460-467), a token is
        sampled for each, and the `num_select` rows of largest token probability are committed (`ego_maskgit_select`).
        The only random numbers are the sampling uniforms: `torch.manual_seed(seed); torch.rand(B * M)`.
        forced_samples / forced_probs ([B, M], teacher forcing for parity tests): the selection runs on the given pair.
        static (graph capture): {"n_dec", "n_enc_cond", "n_enc_uncond", "ws"} - every count comes from the schedule."""
        eng = self.engine
        st = static or {}
        d = mod_dict[target_mod]
        B = d["tensor"].shape[0]
        # (the step updates its three tensors through the select kernel: work on copies, like roar_step's functional scatters)
        tensor = d["tensor"].reshape(B, -1).to(eng.dev, torch.int64).clone()
        input_mask = d["input_mask"].reshape(B, -1).to(eng.dev, torch.bool).clone()
        target_mask = d["target_mask"].reshape(B, -1).to(eng.dev, torch.bool).clone()
        if mod_pos is None:
            n_dec = st.get("n_dec")
            if n_dec is None:
                n_dec = int((~target_mask[0]).sum().item())            # sample 0 sets the row count of the batch (:460)
            mod_pos = ops.maskgit_positions(target_mask, n_dec)
        mod_pos = mod_pos.to(eng.dev, torch.int64).contiguous()
        M = mod_pos.shape[1]
        info = dict(logits_cond=None, logits_uncond=None, mod_pos=mod_pos, samples=None, probs=None, top_indices=None)
        if M > 0:
            logits_cond, logits_uncond = self._step_logits(mod_dict, target_mod, mod_pos, conditioning, guidance_scale, static)
            V = logits_cond.shape[-1]
            if uniforms is None:
                if seed is not None:
                    torch.manual_seed(seed)
                uniforms = torch.rand(B * M, device=eng.dev)
            samples = torch.empty(B, M, device=eng.dev, dtype=torch.int32)
            probs = torch.empty(B, M, device=eng.dev, dtype=torch.float32)
            ops.sample_cfg_topp(logits_cond.view(B * M, V), None if logits_uncond is None else logits_uncond.view(B * M, V), V,
                                float(guidance_scale), float(top_p), float(temperature), uniforms, samples, probs, ld=V,
                                top_k=ops.top_k_count(top_k, V))
            info.update(logits_cond=logits_cond, logits_uncond=logits_uncond, samples=samples.to(torch.int64), probs=probs)
            if forced_samples is not None:
                samples = forced_samples.to(eng.dev, torch.int32).reshape(B, M).contiguous()
            if forced_probs is not None:
                probs = forced_probs.to(eng.dev, torch.float32).reshape(B, M).contiguous()
            K = min(int(num_select), M)
            top = torch.empty(B, K, device=eng.dev, dtype=torch.int64) if return_logits else None
            ops.maskgit_select(samples, probs, mod_pos, K, tensor, input_mask, target_mask, out_idx=top)
            info["top_indices"] = top
        d["tensor"], d["input_mask"], d["target_mask"] = tensor, input_mask, target_mask
        if return_logits:
            return mod_dict, info
        return mod_dict

    def _step(self, mod_dict, info, top_k, top_p, **kw):
        scheme = info["scheme"].lower()
        if scheme not in ("roar", "maskgit"):
            raise ValueError("Invalid sampling scheme")                  # the reference's message (:1081)
        step = self.roar_step if scheme == "roar" else self.maskgit_step
        return step(mod_dict, info["target_domain"], info["num_tokens"], info["temperature"], top_k, top_p,
                    conditioning=info.get("cfg_cond_domains", []), guidance_scale=info.get("cfg_scale", 1.0), **kw)

    @torch.no_grad()
    def generate(self, mod_dict, schedule, top_k=0.0, top_p=0.0, text_tokenizer=None, verbose=False, seed=None):
        mod_dict = copy.deepcopy(mod_dict)
        for step, info in enumerate(schedule):
            mod_dict = self._step(mod_dict, info, top_k, top_p, seed=None if seed is None else seed + step)
        return mod_dict

    # ---- the whole schedule as ONE hipGraph (BASELINE config 4: "hipGraph-captured decode") ---------------------------
    @torch.no_grad()
    def generate_graphed(self, mod_dict, schedule, top_k=0.0, top_p=0.0, seed: int = 0):
        """`generate` with every encoder-decoder pass, the device sampler and the token scatters of ALL schedule steps
        replayed from one captured graph: one host call per clip batch, one host read (the initial mask counts) per call.

        What makes that possible: with ROAR the kept-row counts of every pass follow from the schedule and the initial
        number of unmasked inputs (conditional pass of step s: inputs + tokens decoded so far; unconditional: tokens
        decoded so far, 0 on the first step), and the random ROAR order / sampling uniforms are drawn BEFORE the replay
        with torch's generator seeded `seed + step` exactly as the eager path does - same tokens, bit for bit.
        MaskGIT steps are planned from the schedule alone as well: a step decodes every target still open (open targets -
        tokens committed so far) and commits K = min(num_tokens, rows) of them; kept rows as above with "committed" for
        "decoded".  That needs the same open count in every batch row (the eager path follows the reference's sample-0 rule,
        :460): unequal counts raise ValueError here.
        One graph per (batch, schedule, initial counts, top_p), kept in the engine's bounded graph cache."""
        eng = self.engine
        names = [m.name for m in eng.mods if m.name in mod_dict]
        B = mod_dict[names[0]]["tensor"].shape[0]
        flat = {n: {"tensor": mod_dict[n]["tensor"].reshape(B, -1).to(eng.dev, torch.int64),
                    "input_mask": mod_dict[n]["input_mask"].reshape(B, -1).to(eng.dev, torch.bool),
                    "target_mask": mod_dict[n]["target_mask"].reshape(B, -1).to(eng.dev, torch.bool)} for n in names}
        # the one host read: unmasked inputs and open targets per sample and modality (ROAR uses sample 0's open count, like
        # :498-500; MaskGIT needs every row's)
        cnt = torch.stack([torch.cat([(~flat[n]["input_mask"]).sum(1), (~flat[n]["target_mask"]).sum(1)]) for n in names]).cpu().numpy()
        n_in = {n: cnt[i, :B].astype(np.int64) for i, n in enumerate(names)}            # [B] each
        n_open = {n: int(cnt[i, B]) for i, n in enumerate(names)}
        schemes = [info["scheme"].lower() for info in schedule]
        if any(sc not in ("roar", "maskgit") for sc in schemes):
            raise ValueError("Invalid sampling scheme")                                 # the reference's message (:1081)
        for i, n in enumerate(names):
            if any(sc == "maskgit" and info["target_domain"] == n for sc, info in zip(schemes, schedule)) and len(set(cnt[i, B:].tolist())) > 1:
                raise ValueError(f"MaskGIT from one captured graph needs the same number of open {n} targets in every batch row, "
                                 f"got {cnt[i, B:].tolist()}: use generate()")
        plan, dec_so_far = [], {n: 0 for n in names}
        for info, scheme in zip(schedule, schemes):
            t = info["target_domain"]
            # decoder rows of the step / tokens it commits: ROAR decodes what it commits, MaskGIT decodes every open target
            rows = n_open[t] - dec_so_far[t]
            n_dec = min(int(info["num_tokens"]), rows)
            n_rows = n_dec if scheme == "roar" else rows
            cond = list(info.get("cfg_cond_domains", []))
            guided = info.get("cfg_scale", 1.0) != 1.0 and len(cond) > 0
            # rows kept by a pass = max over the batch of the unmasked inputs of all its modalities (:413-415)
            enc_names = [n for n in names if n in {m.name for m in eng.enc_mods}]
            total = int(sum(n_in[n] + dec_so_far[n] for n in enc_names).max()) if enc_names else 0
            unc = [n for n in enc_names if n not in cond]
            total_u = int(sum(n_in[n] + dec_so_far[n] for n in unc).max()) if unc else 0
            plan.append(dict(target=t, n_dec=n_dec, n_rows=n_rows, scheme=scheme, n_enc_cond=total, guided=guided, n_enc_uncond=total_u, info=info))
            dec_so_far[t] += n_dec
        key = ("generate", bool(eng.cfg_pair), B, tuple(names), tuple((n, tuple(int(x) for x in n_in[n])) for n in names), tuple(sorted(n_open.items())), float(top_p), (type(top_k).__name__, float(top_k or 0)),
               tuple((p["target"], p["n_dec"], p["info"]["temperature"], p["info"].get("cfg_scale", 1.0),
                      tuple(p["info"].get("cfg_cond_domains", []))) for p in plan))
        # (the key holds every step's committed count and the initial open counts; a MaskGIT step's decoder rows - open targets
        #  minus what earlier steps committed - follow from those two, so they need no entry of their own)
        if "maskgit" in schemes:                                # (ROAR-only schedules keep the key they always had)
            key = key + (tuple(schemes),)

        def make_state():
            n_max = max(max(p["n_enc_cond"] for p in plan), 1) + eng.R
            m_max = max(p["n_rows"] for p in plan)
            return {"in": {n: {k: v.clone() for k, v in flat[n].items()} for n in names},
                    "noise": [torch.zeros(flat[p["target"]]["target_mask"].shape[1], device=eng.dev) for p in plan],
                    "uni": [torch.zeros(B * p["n_rows"], device=eng.dev) for p in plan],
                    "ws": eng._alloc_infer(B, n_max, m_max, fresh=True,
                                           groups=2 if (eng.cfg_pair and any(p["guided"] for p in plan)) else 1), "out": None}

        def run(st):
            md = {n: {k: v.clone() for k, v in st["in"][n].items()} for n in names}
            for i, p in enumerate(plan):
                info = p["info"]
                step = self.roar_step if p["scheme"] == "roar" else self.maskgit_step
                md = step(md, p["target"], p["n_dec"], info["temperature"], top_k, top_p,
                          conditioning=info.get("cfg_cond_domains", []), guidance_scale=info.get("cfg_scale", 1.0),
                          uniforms=st["uni"][i],
                          static=dict(noise=st["noise"][i], n_dec=p["n_rows"], n_enc_cond=p["n_enc_cond"],
                                      n_enc_uncond=p["n_enc_uncond"], ws=st["ws"]))
            st["out"] = md                                      # (the capture's run comes last: its tensors are the graph's)

        graph, st = eng._graphed(key, make_state, run)
        for n in names:
            for k in ("tensor", "input_mask", "target_mask"):
                st["in"][n][k].copy_(flat[n][k])
        for i, p in enumerate(plan):                            # the eager path's draws, in its order (roar_order, then roar_step;
            torch.manual_seed(seed + i)                         #  a MaskGIT step draws its uniforms only)
            if p["scheme"] == "roar":
                st["noise"][i].copy_(torch.rand(st["noise"][i].shape[0], device=eng.dev))
            st["uni"][i].copy_(torch.rand(st["uni"][i].shape[0], device=eng.dev))
        graph.replay()
        out = copy.deepcopy({n: dict(mod_dict[n]) for n in mod_dict if n not in names})
        for n in names:
            out[n] = {k: v.clone() for k, v in st["out"][n].items()}
            for k, v in mod_dict[n].items():
                out[n].setdefault(k, v)
        return out
