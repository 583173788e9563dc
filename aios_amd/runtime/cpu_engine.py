"""CPU inference engine: the runtime's no-GPU backend (BASELINE config #1 -- "TinyLlama Q4_0 greedy
decode via the runtime on CPU, plumbing, no GPU"; the reference's default deployment is
llama-server with `gpu_layers: 0`, `runtime/src/main.rs:108-115`).

Same Python surface as the native `Engine` (prefill / decode / config / weight_bytes / kv_bytes /
close), so the scheduler, the AIRuntime gRPC service and the OpenAI HTTP endpoint run unchanged
on it.  Numerics are the fp32 reference forward (`aios_amd.models.reference`) over the exact
dequantised GGUF weights with a per-slot KV cache; sampling uses the host sampler (same
semantics as the device sampler, incl. the JSON-grammar bitmask).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np
import torch

from ..models.reference import ReferenceModel
from . import embedding as host_embedding
from . import sampler as host_sampler
from . import scoring as host_scoring


@dataclasses.dataclass
class CpuEngineConfig:
    max_ctx: int
    max_slots: int
    max_batch: int
    vocab_size: int
    n_layers: int
    device: str = "cpu"


class CpuEngine:
    def __init__(self, model: ReferenceModel, max_ctx: int = 2048, max_slots: int = 4, max_batch: int = 4,
                 threads: int = 0):
        if threads > 0:
            torch.set_num_threads(threads)
        self.model = model
        self.cfg = model.cfg
        self.config = CpuEngineConfig(max_ctx=max_ctx, max_slots=max_slots, max_batch=max_batch,
                                      vocab_size=model.cfg.vocab_size, n_layers=model.cfg.n_layers)
        self.caches: Dict[int, dict] = {}
        self.weight_bytes = int(sum(t.numel() * t.element_size() for t in model.w.values()))
        c = model.cfg
        self.kv_bytes = 2 * c.n_layers * max_slots * max_ctx * c.n_kv_heads * c.head_dim * 4
        self.last: Optional[np.ndarray] = None
        self._proc = None  # set_sample_processors: per-row processors of the next sampler call only
        self._lp = None    # set_logprobs: per-row top_n of the next sampler call only
        self._lp_out = ()  # last_logprobs: what the last sampler call reported
        self._emb: Dict[int, dict] = {}  # embed_prefill: per-slot pooling state (pos, pooling, sum, rows)
        self._emb_tokens = 0

    @classmethod
    def from_gguf(cls, path: str, max_ctx: int = 2048, max_slots: int = 4, max_batch: int = 4,
                  threads: int = 0) -> "CpuEngine":
        return cls(ReferenceModel.from_gguf(path, kv_bf16=False), max_ctx, max_slots, max_batch, threads)

    # ------------------------------------------------------------------ cache
    def _cache_at(self, slot: int, start: int) -> dict:
        if not 0 <= slot < self.config.max_slots:
            raise ValueError(f"bad slot {slot}")
        c = self.caches.get(slot)
        if c is None or start == 0:
            c = self.model.new_cache()
            self.caches[slot] = c
        if start > c["len"]:
            raise ValueError(f"slot {slot}: position {start} beyond the cached {c['len']} tokens")
        if start < c["len"]:  # prefix reuse: drop the cached tail
            for l in range(self.cfg.n_layers):
                c["k"][l] = c["k"][l][:start]
                c["v"][l] = c["v"][l][:start]
            c["len"] = start
        return c

    def copy_slot(self, src: int, dst: int, n: int):
        s = self.caches.get(src)
        if s is None:
            return
        self.caches[dst] = {"k": [k[:n].clone() for k in s["k"]], "v": [v[:n].clone() for v in s["v"]], "len": n}

    # ------------------------------------------------------------------ inference
    def prefill(self, slot: int, ids: List[int], start: int = 0, want_logits: bool = True):
        if start + len(ids) > self.config.max_ctx:
            raise ValueError("prefill: context overflow")
        c = self._cache_at(slot, start)
        logits = self.model.forward(list(ids), c)[-1].numpy()
        self.last = logits[None]
        return logits if want_logits else []

    def embed_prefill(self, slot: int, ids: List[int], start: int = 0, pooling: int = 1, final: bool = True):
        """The native Engine's embed_prefill (runtime/embedding.py: the rule): prefill `ids` into the slot
        and fold their final hidden rows into the slot's pooling state.  start == 0 resets it; a later call
        must continue where the last one ended ("last" keeps no state and may start at a cached prefix).
        final: the unit vector [d] (pooling 1 mean, 3 last) or the normed rows [tokens, d] (0 none); else an
        empty array."""
        pooling = host_embedding.pooling_code(pooling)
        if not ids:
            raise ValueError("embed_prefill: empty prompt")
        if start + len(ids) > self.config.max_ctx:
            raise ValueError("embed_prefill: context overflow")
        st = self._emb.get(slot)
        last = pooling == host_embedding.POOLING["last"]
        if start == 0 or last:
            st = dict(pos=start, pooling=pooling, sum=0.0, rows=[])
        elif st is None or st["pos"] != start or st["pooling"] != pooling:
            raise ValueError(f"embed_prefill: start_pos {start} does not continue the slot's pooled positions "
                             f"({st['pos'] if st else -1})")
        self._emb.pop(slot, None)  # (a call that throws leaves no state to continue)
        c = self._cache_at(slot, start)
        x = self.model.hidden(list(ids), c).double().cpu().numpy()
        g = self.model.w["output_norm.weight"].double().cpu().numpy()
        eps = self.cfg.norm_eps
        if pooling == host_embedding.POOLING["none"]:
            st["rows"].append(host_embedding.normed_rows(x, g, eps))
        elif last:
            st["sum"] = host_embedding.normed_rows(x[-1], g, eps)
        else:  # the sum of x / rms; g is applied once at the end, as on the device
            st["sum"] = st["sum"] + host_embedding.normed_rows(x, np.ones_like(g), eps).sum(0)
        st["pos"] = start + len(ids)
        self._emb[slot] = st
        if not final:
            return np.zeros(0, np.float32)
        self._emb_tokens = st["pos"]
        if pooling == host_embedding.POOLING["none"]:
            return np.concatenate(st["rows"]).astype(np.float32)
        p = st["sum"] if last else st["sum"] / st["pos"] * g
        return host_embedding.unit(p).astype(np.float32)

    def embed_tokens(self) -> int:
        return self._emb_tokens

    def score_prefill(self, slot: int, ids: List[int], start: int = 0, next_token: int = -1, top_n: int = 0,
                      want_logits: bool = False) -> dict:
        """The native Engine's score_prefill (runtime/scoring.py: the rule): prefill `ids` into the slot and
        score every row against the token after it, the last row against next_token (-1: none).  The same
        dict of arrays; want_logits: the last row's logits are kept for sample_first, as after prefill."""
        if not ids:
            raise ValueError("score_prefill: empty prompt")
        if start + len(ids) > self.config.max_ctx:
            raise ValueError("score_prefill: context overflow")
        if not -1 <= int(next_token) < self.config.vocab_size:
            raise ValueError("score_prefill: next_token out of range")
        c = self._cache_at(slot, start)
        logits = self.model.forward(list(ids), c).numpy()
        if want_logits:
            self.last = logits[-1][None]
        return host_scoring.score_rows(logits, [int(t) for t in ids[1:]] + [int(next_token)], top_n)

    def set_sample_processors(self, min_p, repeat_penalty, presence_penalty, frequency_penalty, recent,
                              bias_ids=(), bias_vals=()):
        """Per-row min-p, penalties and penalty windows (the rows' recent token ids) for the NEXT
        sampler call (decode or sample_first), then dropped -- the native Engine's contract.
        bias_ids / bias_vals: the rows' logit-bias lists (both empty: none), applied in front of the
        penalties."""
        B = len(recent)
        if not (len(min_p) == len(repeat_penalty) == len(presence_penalty) == len(frequency_penalty) == B):
            raise ValueError("set_sample_processors: size mismatch")
        V = self.config.vocab_size
        for w in recent:
            if len(w) > host_sampler.PEN_MAX:
                raise ValueError(f"set_sample_processors: window longer than {host_sampler.PEN_MAX}")
            if any(t >= V for t in w):
                raise ValueError("set_sample_processors: token out of range")
        if len(bias_ids) or len(bias_vals):
            if len(bias_ids) != B or len(bias_vals) != B:
                raise ValueError("set_sample_processors: size mismatch")
            for ids, vals in zip(bias_ids, bias_vals):
                host_sampler.check_logit_bias(ids, vals, V)
        self._proc = (list(min_p), list(repeat_penalty), list(presence_penalty), list(frequency_penalty),
                      [list(w) for w in recent], [list(i) for i in bias_ids], [list(v) for v in bias_vals])

    def set_logprobs(self, top_n):
        """Per-row alternatives wanted (0..LOGPROB_MAX_TOP, < 0: row off) from the NEXT sampler call
        (decode or sample_first), then dropped -- the native Engine's contract."""
        top_n = [int(n) for n in top_n]
        if not 1 <= len(top_n) <= self.config.max_batch:
            raise ValueError("set_logprobs: batch out of range")
        if any(n > host_sampler.LOGPROB_MAX_TOP for n in top_n):
            raise ValueError(f"set_logprobs: top_n above {host_sampler.LOGPROB_MAX_TOP}")
        self._lp = top_n

    def _take_logprobs(self, rows, toks):
        """after a sampler call over the raw logits `rows` that chose `toks`: the staged report"""
        top_n, self._lp = self._lp, None
        self._lp_out = ()
        if top_n is None:
            return
        if len(top_n) != len(toks):
            raise ValueError("logprobs staged for another batch size")
        K = host_sampler.LOGPROB_MAX_TOP
        lp = np.full(len(toks), np.nan, np.float64)
        ids = np.full((len(toks), K), -1, np.int32)
        lps = np.full((len(toks), K), -np.inf, np.float64)
        for b, n in enumerate(top_n):
            if n < 0:
                continue
            lp[b], i, x = host_sampler.logprobs(rows[b], toks[b], n)
            ids[b, :len(i)] = i
            lps[b, :len(x)] = x
        self._lp_out = (lp, ids, lps)

    def last_logprobs(self):
        """() when the last sampler call had none staged, else (token logprob [B], ids [B][20], logprobs
        [B][20]); rows that were off: NaN, -1, -inf -- the native Engine's shape"""
        return self._lp_out

    def _sample(self, proc, b, logits, t, k, tp, m, rng):
        if proc is None or b >= len(proc[4]):
            return host_sampler.sample(logits, t, k, tp, m, rng)
        mp, rp, pp, fp, recent, bias_ids, bias_vals = proc
        if bias_ids:
            logits = host_sampler.apply_logit_bias(logits, bias_ids[b], bias_vals[b])
        logits = host_sampler.apply_penalties(logits, recent[b], rp[b], pp[b], fp[b])
        return host_sampler.sample(logits, t, k, tp, m, rng, min_p=float(mp[b]))

    def decode(self, slots, toks, pos, temps, topk, seed, mask: bytes = b"", top_p=None, seeds=None):
        V = self.config.vocab_size
        row = (V + 7) // 8
        out, rows = [], []
        proc, self._proc = self._proc, None
        for b, (slot, tok, p) in enumerate(zip(slots, toks, pos)):
            if p >= self.config.max_ctx:
                raise ValueError("decode: position out of range")
            c = self._cache_at(slot, p)
            logits = self.model.forward([int(tok)], c)[-1].numpy()
            rows.append(logits)
            m = mask[b * row:(b + 1) * row] if mask else None
            t = float(temps[b]) if b < len(temps) else 0.0
            k = int(topk[b]) if b < len(topk) else 0
            # per-row seed: the row's stream depends on (seed, position) only, as on the GPU
            rng = (np.random.default_rng([int(seeds[b]) & 0xFFFFFFFF, p]) if seeds else
                   np.random.default_rng((int(seed) << 20) ^ (slot << 12) ^ p))
            tp = float(top_p[b]) if top_p is not None and b < len(top_p) else 1.0
            out.append(self._sample(proc, b, logits, t, k, tp, m, rng))
        self.last = np.stack(rows) if rows else None
        self._take_logprobs(rows, out)
        return out

    def sample_first(self, pos, temperature, top_k, top_p, seed, mask: bytes = b""):
        """the token after a prefill, from its last logits, with the decode steps' RNG stream"""
        logits = self.last[0]
        rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(pos)])
        proc, self._proc = self._proc, None
        tok = self._sample(proc, 0, logits, float(temperature), int(top_k), float(top_p), mask or None, rng)
        self._take_logprobs([logits], [tok])
        return tok

    def last_logits(self, B: int):
        return self.last[:B].reshape(-1) if self.last is not None else np.zeros(0, np.float32)

    def synchronize(self):
        pass

    def close(self):
        self.caches.clear()
