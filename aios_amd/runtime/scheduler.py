"""Continuous-batching generation scheduler for one model.

Replaces the per-request HTTP round trip to llama-server (`runtime/src/inference.rs:94-186`)
with an in-process worker per model that owns the native Engine:

* admission: a waiting request takes a free KV slot and inherits the longest cached prefix of
  ANY slot -- free or still decoding: the engine's paged KV shares that prefix's full blocks
  with the new slot (refcounted, no copy; csrc/engine.hip copy_slot) and only the remainder is
  prefilled (the autonomy loop resends the tool catalogue and format rules every round, with up
  to 3 concurrent loops);
* chunked prefill interleaved with decode: while sequences are decoding, a new prompt is
  prefilled AIOS_PREFILL_CHUNK tokens (default 512) per scheduler iteration between batched
  decode steps, so a 3k-token admission does not stall every running stream for its whole
  prefill; with nothing decoding the prompt goes through in one call;
* each iteration runs ONE batched decode step (hipGraph replay) for every decoding sequence, so
  concurrent agents/reasoning loops share each weight pass;
* JSON mode (the reference's `response_format: json_object`) builds the allowed-token mask per
  row with the native JsonGrammar and the device sampler applies it; generation stops as soon as
  the top-level object is complete;
* true token streaming: every step pushes text deltas to the request's callback (the reference
  buffered the whole SSE body, App. A #2).

The worker is a thread: engine calls release the GIL, asyncio callers get results through
thread-safe callbacks.
"""
from __future__ import annotations

import collections
import concurrent.futures
import dataclasses
import logging
import os
import threading
import time
from typing import Callable, Deque, Dict, List, Optional

import numpy as np

from . import embedding as host_embedding
from . import json_schema
from . import kv_snapshot
from . import sampler as host_sampler
from . import speculative as speculative_mod

log = logging.getLogger("aios.runtime.scheduler")


NEUTRAL_PROCESSORS = dict(min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)


def _fresh_seed() -> int:
    return int.from_bytes(os.urandom(8), "little") | 1


@dataclasses.dataclass
class GenRequest:
    prompt_ids: List[int]
    max_tokens: int = 512
    temperature: float = 0.0
    top_k: int = 40
    top_p: float = 0.95
    json_mode: bool = False
    # a JSON schema the finished answer must validate against (runtime/json_schema.py: the accepted subset, the
    # forced property order, the whitespace rule); it takes the place of json_mode's "one JSON object".  The
    # request ends "grammar" where nothing can follow, "stop" at an end-of-sequence token (allowed only where the
    # text is complete) and "length" where max_tokens cuts the value short.  min_tokens is ignored and the row
    # takes no speculative steps.  On a single-GPU tier the mask comes from the device (Engine.set_grammar_rows)
    # unless the request also bans tokens; elsewhere from the host grammar
    json_schema: Optional[dict] = None
    # JSON mode: the grammar may not close the object before this many tokens (bench runs pin the
    # plan length with it: random weights close a JSON object at arbitrary points)
    min_tokens: int = 0
    seed: int = 0
    # logit processors (runtime/sampler.py: apply_penalties, min-p).  None = the tier's default
    # (Scheduler.sampling_defaults, neutral unless the node config sets it); neutral values are
    # min_p 0, repeat_penalty 1, presence_penalty 0, frequency_penalty 0
    min_p: Optional[float] = None
    repeat_penalty: Optional[float] = None
    repeat_last_n: int = 64           # penalty window: the row's last n tokens, prompt tail included (< 0 or > 256: 256)
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    # logit bias (runtime/sampler.py: apply_logit_bias, in front of the penalties): token id -> a finite bias
    # or -inf (a ban), at most 512 entries.  ignore_eos bans the tier's end-of-sequence ids (over a finite
    # bias on them): the request ends by max_tokens, its other stop ids or the context window.  In JSON mode
    # the grammar wins: at a step where no token is both allowed by the grammar and unbanned, the bans are
    # left out for that step (stats["bias_overridden"])
    logit_bias: Optional[Dict[int, float]] = None
    ignore_eos: bool = False
    # per-token log-probabilities of the model's RAW distribution (before penalties, the grammar mask and
    # temperature; runtime/sampler.py: logprobs): the chosen token's, and its top_logprobs (0..20) best
    # alternatives -- GenResult.logprobs.  The stream callback carries text only.
    logprobs: bool = False
    top_logprobs: int = 0
    # text embedding instead of generation (runtime/embedding.py: the rule): "mean" | "last" | "none".  The
    # prompt is prefilled like any other (admission, slot, chunks between decode steps) through the engine's
    # embed_prefill and the request ends with it -- GenResult.embedding, finish_reason "embedding";
    # max_tokens, json_mode, the sampling fields and logprobs are ignored
    embed: Optional[str] = None
    # logprobs of the PROMPT's tokens (runtime/scoring.py: the rule; the engine's score_prefill): None = off,
    # else the number of alternatives per prompt token, 0..20 -- GenResult.prompt_logprobs.  The prompt is
    # prefilled from position 0 (cached positions have no logits) and generation proceeds as usual; with
    # such a request max_tokens may be 0: it then finishes "length" with no sampled token
    prompt_logprobs: Optional[int] = None
    # speculative decoding from prompt-lookup drafts (runtime/speculative.py: the rule): None = the tier's
    # default, True / False = on / off for this request.  The tokens are the ones plain decode would emit;
    # only the number of engine steps changes.  prediction_ids: the tokens of a text the caller expects in
    # the output (OpenAI's Predicted Outputs), searched for drafts before the prompt itself
    speculative: Optional[bool] = None
    prediction_ids: Optional[List[int]] = None
    # context shift (llama-server's n_keep / context shift; the engine's shift_context): when the slot reaches the
    # context window and max_tokens is not, the oldest part of the conversation behind the first n_keep prompt
    # tokens is dropped -- n_discard = (n_past - n_keep) // 2 tokens, llama.cpp's numbers -- the rest moves down
    # with its keys re-rotated, and generation goes on; max_tokens is then not clamped to the window.  n_keep:
    # -1 = the whole prompt; any value is clamped to the prompt length.  The tier's default (node config
    # context_shift) applies to requests that leave the flag off
    context_shift: bool = False
    n_keep: int = -1
    stop_ids: Optional[List[int]] = None
    on_delta: Optional[Callable[[str], None]] = None
    on_done: Optional[Callable[["GenResult"], None]] = None
    deadline: float = 0.0             # absolute time.time(); 0 = none
    cancelled: bool = False
    submitted_at: float = dataclasses.field(default_factory=time.time)


@dataclasses.dataclass
class GenResult:
    text: str
    token_ids: List[int]
    prompt_tokens: int
    completion_tokens: int
    finish_reason: str                # stop | length | grammar | cancelled | error | deadline | embedding
    ttft_ms: float = 0.0
    latency_ms: float = 0.0
    cached_prompt_tokens: int = 0
    error: str = ""
    # requests with logprobs=True: one (token id, logprob, [(alternative id, logprob), ...]) per entry of
    # token_ids, best alternative first; None otherwise
    logprobs: Optional[list] = None
    # requests with embed set: the unit vector [d] ("mean", "last") or the normed rows [tokens, d] ("none")
    embedding: Optional[np.ndarray] = None
    # requests with prompt_logprobs set: one (token id, logprob | None, rank | None, [(alternative id,
    # logprob), ...]) per prompt token; rank 0 = the token was the model's argmax, the alternatives are the
    # best tokens AT that position, best first; the first token has no distribution: None, None, []
    prompt_logprobs: Optional[list] = None
    # speculative decoding: draft tokens handed to the engine for verification, and how many of them it
    # accepted (both 0 when nothing was drafted)
    draft_tokens: int = 0
    accepted_draft_tokens: int = 0
    context_shifts: int = 0           # context shifts the request went through


# the tier's speculative-decoding settings (node config: speculative, spec_draft_max, spec_ngram_min / _max,
# spec_max_context, spec_multi); draft_max and max_context are measured values (profiles/spec_decode.txt), as is
# multi (profiles/spec_decode_multi.txt): speculative steps while 2..8 sequences decode
SPEC_DEFAULTS = dict(mode="off", draft_max=7, ngram_min=2, ngram_max=3, max_context=4096, multi=1)


class SlotBusy(RuntimeError):
    """a slot action (save / restore / erase) on a slot that is decoding or prefilling"""


class SlotsUnsupported(RuntimeError):
    """slot actions on a tier whose engine has no kv_save / kv_restore (a tensor-parallel or CPU tier)"""


class _Seq:
    __slots__ = ("req", "slot", "pos", "last", "out", "grammar_state", "emitted", "t_first", "cached", "todo",
                 "p_off", "r_off", "seed", "proc", "pen_n", "bias", "bias_soft", "lp_n", "lps", "embedding", "plp_n", "plps",
                 "spec", "drafter", "drafted", "draft_hits", "shift", "n_keep", "shifts", "grammar", "schema", "dev_grammar")

    def __init__(self, req, slot):
        self.req, self.slot = req, slot
        # the request's sampling seed; unseeded requests draw a fresh one (llama-server does the
        # same), so two identical T > 0 requests do not return identical "samples"
        self.seed = int(req.seed) & 0xFFFFFFFFFFFFFFFF if req.seed else _fresh_seed()
        self.pos = 0                 # next position to write (prefill cursor, then decode position)
        self.last = 0
        self.out: List[int] = []
        self.grammar_state = None
        self.grammar = None          # the row's grammar object: the tier's JsonGrammar or its schema's SchemaGrammar
        self.schema = None           # its compiled schema (json_schema.SchemaCache.Entry), held until the row finishes
        self.dev_grammar = False     # the device computes the row's mask from (schema.gid, grammar_state.s)
        self.emitted = ""
        self.t_first = 0.0
        self.cached = 0
        self.todo: List[int] = []    # prompt tokens still to prefill
        self.proc = None             # (min_p, repeat, presence, frequency penalty), None when all neutral
        self.pen_n = 0               # penalty window length
        self.bias = None             # logit bias (ids, vals), built once at admission; None when empty
        self.bias_soft = None        # the same without its -inf entries (a step where the grammar wins)
        self.lp_n = int(req.top_logprobs) if req.logprobs else -1  # alternatives per token; -1: no logprobs
        self.lps: List[tuple] = []   # one entry per token of `out`
        self.embedding = None        # an embedding request's result
        self.plp_n = -1              # prompt logprobs: alternatives per prompt token; -1: not asked
        self.plps: List[tuple] = []  # one entry per prompt token prefilled so far
        self.spec = False            # speculative decoding on for this request (set at admission)
        self.drafter = None          # its LookupDrafter over prompt + out, built when decoding starts
        self.drafted = 0             # draft tokens verified / accepted so far
        self.draft_hits = 0
        self.shift = False           # context shift on for this request (set at admission)
        self.n_keep = 0              # its n_keep, clamped to the prompt
        self.shifts = 0              # shifts so far; from the first on the slot's cached tokens stay cut to n_keep
        self.p_off = 0              # incremental detokenization window [p_off, r_off) already emitted
        self.r_off = 0


class Scheduler:
    def __init__(self, engine, tokenizer, max_batch: int, max_slots: int, max_ctx: int, grammar=None,
                 name: str = "model", sampling_defaults: Optional[Dict[str, float]] = None,
                 speculative: Optional[dict] = None, context_shift: bool = False):
        self.engine = engine
        # context shift (GenRequest.context_shift; this is the tier's default for requests that leave it off); it
        # needs the engine's shift_context, which the CPU and tensor-parallel tiers lack
        self.context_shift = bool(context_shift)
        self.can_shift = hasattr(engine, "shift_context")
        self._warned_no_shift = False
        # KV snapshots (save_slot / restore_slot / erase_slot / slots): they need the engine's kv_save and
        # kv_restore, which the CPU and tensor-parallel tiers lack.  Actions wait here for the worker, which owns
        # the engine and runs them between two iterations
        self.can_snapshot = hasattr(engine, "kv_save") and hasattr(engine, "kv_restore")
        self._ops: Deque = collections.deque()
        # speculative decoding (SPEC_DEFAULTS; off unless the tier or a request turns it on); it needs the
        # engine's spec_decode, which the CPU and tensor-parallel tiers lack: they decode plainly and say so once
        self.spec = dict(SPEC_DEFAULTS)
        for k, v in (speculative or {}).items():
            if k not in SPEC_DEFAULTS:
                raise ValueError(f"unknown speculative setting {k!r}")
            self.spec[k] = v if k == "mode" else int(v)
        if self.spec["mode"] not in ("off", "lookup"):
            raise ValueError(f"speculative mode {self.spec['mode']!r} is neither 'off' nor 'lookup'")
        if not (1 <= self.spec["draft_max"] <= speculative_mod.DRAFT_MAX_LIMIT and self.spec["max_context"] >= 1 and
                self.spec["multi"] in (0, 1) and
                1 <= self.spec["ngram_min"] <= self.spec["ngram_max"] <= speculative_mod.NGRAM_MAX_LIMIT):
            raise ValueError("speculative settings out of range")
        self.can_spec = hasattr(engine, "spec_decode")
        self.can_spec_multi = self.can_spec and hasattr(engine, "spec_decode_multi")
        # schema rows whose mask the device computes need the engine's grammar calls (the CPU and tensor-parallel
        # tiers lack them and serve such rows through the host grammar); the cache is built by the first schema
        self.can_device_grammar = all(hasattr(engine, n) for n in ("grammar_vocab", "grammar_load", "set_grammar_rows"))
        self._schemas: Optional[json_schema.SchemaCache] = None
        self._warned_no_spec = False
        # the tier's logit-processor defaults for requests that leave a field unset (the only way a
        # gRPC caller, whose contract has no such fields, gets them)
        self.sampling_defaults = dict(NEUTRAL_PROCESSORS)
        for k, v in (sampling_defaults or {}).items():
            if k not in NEUTRAL_PROCESSORS:
                raise ValueError(f"unknown sampling default {k!r}")
            self.sampling_defaults[k] = float(v)
        self._warned_no_processors = False
        # a logit bias needs the engine's set_sample_processors (a tensor-parallel tier hides the call)
        self.can_bias = hasattr(engine, "set_sample_processors")
        # per-token logprobs need the engine's set_logprobs / last_logprobs (a tensor-parallel tier has
        # neither: its lm_head is vocab-parallel)
        self.can_logprobs = hasattr(engine, "set_logprobs") and hasattr(engine, "last_logprobs")
        # text embeddings need the engine's embed_prefill (a tensor-parallel tier hides it)
        self.can_embed = hasattr(engine, "embed_prefill")
        # prompt logprobs need the engine's score_prefill (a tensor-parallel tier has none)
        self.can_score = hasattr(engine, "score_prefill")
        self.tok = tokenizer
        self.max_batch = max_batch
        self.max_ctx = max_ctx
        self.grammar = grammar
        self.name = name
        self.vocab = tokenizer.vocab_size
        self.eos = {tokenizer.eos_id}
        for extra in ("<|eot_id|>", "<|im_end|>", "<|end|>"):
            if extra in tokenizer.vocab:
                self.eos.add(tokenizer.vocab[extra])
        self.slot_cache: Dict[int, List[int]] = {s: [] for s in range(max_slots)}
        self.free_slots = list(range(max_slots))
        self.queue: Deque[GenRequest] = collections.deque()
        self.active: List[_Seq] = []          # decoding
        self.prefilling: List[_Seq] = []      # admitted, prompt not fully prefilled yet
        self.prefill_chunk = int(os.environ.get("AIOS_PREFILL_CHUNK", "512"))
        self._full_mask = None
        # host-side cost breakdown of the decode loop (bench_serving / HealthCheck)
        self.timing = dict(mask_s=0.0, engine_decode_s=0.0, accept_s=0.0, prefill_s=0.0)
        self.step_log: Deque = collections.deque(maxlen=4096)  # (end time, batch) per decode step
        self.share_prefix = hasattr(engine, "copy_slot")
        self.min_shared_prefix = int(os.environ.get("AIOS_MIN_SHARED_PREFIX", "128"))
        self.cv = threading.Condition()
        self.stop_flag = False
        self.stats = dict(requests=0, tokens=0, prefill_tokens=0, cached_tokens=0, steps=0, batch_sum=0, errors=0,
                          embeddings=0, prompt_scores=0, spec_steps=0, spec_drafted=0, spec_accepted=0,
                          spec_multi_steps=0, bias_overridden=0, context_shifts=0, shifted_tokens=0, slot_saves=0, slot_restores=0,
                          slot_erases=0, schema_requests=0, schema_compiles=0)
        # health / metrics (ModelManager.supervise and HealthCheck details)
        self.max_slots = max_slots
        self.last_progress = time.time()   # last completed admission or decode step
        self.failed = ""                   # last engine error (a device fault leaves the engine unusable)
        self._ttft = collections.deque(maxlen=256)
        self._step_ms = collections.deque(maxlen=256)
        self._tok_times = collections.deque(maxlen=4096)
        # pipelined decode (Engine.decode_submit / decode_sample / decode_collect): the forward of step
        # t+1 is queued before the host has seen step t's token, so the host's per-token work (grammar
        # mask, accept, detokenize, callbacks) overlaps the device step instead of adding to it
        self.pipeline = hasattr(engine, "decode_submit") and os.environ.get("AIOS_DECODE_PIPELINE", "1") != "0"
        self._pending: Optional[List[_Seq]] = None  # rows whose sampled step is in flight
        self.thread = threading.Thread(target=self._run, name=f"sched-{name}", daemon=True)
        self.thread.start()

    # ------------------------------------------------------------------ public
    def submit(self, req: GenRequest):
        with self.cv:
            self.queue.append(req)
            self.stats["requests"] += 1
            self.cv.notify()

    def close(self):
        with self.cv:
            self.stop_flag = True
            self.cv.notify()
        self.thread.join(timeout=10)
        if self._schemas is not None and not self.thread.is_alive():  # (the worker owned the engine until now)
            try:
                self._schemas.clear()
            except Exception:  # noqa: BLE001 - a failed engine
                log.exception("freeing the compiled schemas failed")

    @property
    def load(self) -> int:
        return len(self.queue) + len(self.active) + len(self.prefilling)

    # ------------------------------------------------------------------ slot actions (KV snapshots)
    def _slot_op(self, fn, timeout: float):
        """Run fn() on the worker thread between two iterations and return its result (or raise its error)."""
        fut: concurrent.futures.Future = concurrent.futures.Future()
        with self.cv:
            if self.stop_flag:
                raise RuntimeError(f"{self.name}: the scheduler is closed")
            self._ops.append((fn, fut))
            self.cv.notify()
        return fut.result(timeout)

    def _free_slot(self, slot) -> int:
        if isinstance(slot, bool) or not isinstance(slot, int) or slot not in self.slot_cache:
            raise ValueError(f"unknown slot {slot!r}")
        if slot not in self.free_slots:
            raise SlotBusy("slot busy")
        return slot

    def _need_snapshots(self):
        if not self.can_snapshot:
            raise SlotsUnsupported("slots: single-GPU engines only")

    def save_slot(self, slot: int, path: str, timeout: float = 120.0) -> dict:
        """Save a free slot's cache to `path` (runtime/kv_snapshot.py): exactly the tokens its cache record holds
        -- the positions _pick_slot would trust, so nothing behind a context shift's n_keep and nothing a dropped
        pipelined step wrote.  {"n_saved": tokens, "n_written": bytes}.  SlotBusy for a slot that is decoding or
        prefilling, ValueError for an unknown slot or an empty record."""
        def op():
            self._need_snapshots()
            s = self._free_slot(slot)
            n, written = kv_snapshot.save_slot(self.engine, s, list(self.slot_cache[s]), path, self.name)
            self.stats["slot_saves"] += 1
            return {"n_saved": n, "n_written": written}
        return self._slot_op(op, timeout)

    def restore_slot(self, slot: int, path: str, timeout: float = 120.0) -> dict:
        """Restore `path` into a free slot and set its cache record to the file's tokens: the next request with that
        prefix reuses it through the ordinary admission path.  {"n_restored": tokens, "n_read": bytes}.
        FileNotFoundError, kv_snapshot.SnapshotError (naming the field) and SlotBusy change nothing."""
        def op():
            self._need_snapshots()
            s = self._free_slot(slot)
            tokens, size = kv_snapshot.restore_slot(self.engine, s, path, self.name, self.max_ctx)
            self.slot_cache[s] = list(tokens)
            self.stats["slot_restores"] += 1
            return {"n_restored": len(tokens), "n_read": size}
        return self._slot_op(op, timeout)

    def erase_slot(self, slot: int, timeout: float = 120.0) -> dict:
        """Release a free slot's blocks and clear its cache record.  {"n_erased": tokens the record held}."""
        def op():
            self._need_snapshots()
            s = self._free_slot(slot)
            n = len(self.slot_cache[s])
            self.engine.release_slot(s)
            self.slot_cache[s] = []
            self.stats["slot_erases"] += 1
            return {"n_erased": n}
        return self._slot_op(op, timeout)

    def slots(self, timeout: float = 120.0) -> List[dict]:
        """One entry per slot: id, is_processing (decoding or prefilling) and n_cached (its cache record's length)."""
        def op():
            return [{"id": s, "is_processing": s not in self.free_slots, "n_cached": len(self.slot_cache[s])}
                    for s in sorted(self.slot_cache)]
        return self._slot_op(op, timeout)

    def _run_ops(self, ops):
        for fn, fut in ops:
            if not fut.set_running_or_notify_cancel():
                continue
            try:
                fut.set_result(fn())
            except BaseException as e:  # noqa: BLE001 - the caller's to handle
                fut.set_exception(e)

    # ------------------------------------------------------------------ worker
    def _run(self):
        while True:
            with self.cv:
                while (not self.stop_flag and not self.queue and not self.active and not self.prefilling and
                       not self._ops):
                    self.cv.wait(timeout=1.0)
                ops = list(self._ops)
                self._ops.clear()
                if self.stop_flag:
                    for _fn, fut in ops:
                        fut.set_exception(RuntimeError(f"{self.name}: the scheduler is closed"))
                    self._discard_pending()
                    for s in list(self.active) + list(self.prefilling):
                        self._finish(s, "cancelled")
                    while self.queue:
                        r = self.queue.popleft()
                        self._done(r, GenResult("", [], len(r.prompt_ids), 0, "cancelled"))
                    return
                admit = []
                while (self.queue and self.free_slots and
                       len(self.active) + len(self.prefilling) + len(admit) < self.max_batch):
                    admit.append(self.queue.popleft())
            if admit or self.prefilling or ops:
                self._drain()  # (no other engine call while a pipelined step is in flight)
            if ops:
                self._run_ops(ops)
            for r in admit:
                try:
                    self._admit(r)
                    self.last_progress = time.time()
                except ValueError as e:  # request error (e.g. prompt too long): the engine is fine
                    self._done(r, GenResult("", [], len(r.prompt_ids), 0, "error", error=str(e)))
                except Exception as e:  # noqa: BLE001 - engine failure: reported to the caller
                    log.exception("admission failed")
                    self._engine_failed(e)
                    self._done(r, GenResult("", [], len(r.prompt_ids), 0, "error", error=str(e)))
            if self.prefilling:
                seq = self.prefilling[0]
                try:
                    self._prefill_chunk(seq)
                    self.last_progress = time.time()
                except ValueError as e:
                    self._finish(seq, "error", str(e))
                except Exception as e:  # noqa: BLE001
                    log.exception("prefill failed")
                    self._engine_failed(e)
                    self._finish(seq, "error", str(e))
            if self.active:
                try:
                    t0 = time.time()
                    self._step()
                    self.last_progress = time.time()
                    self._step_ms.append((self.last_progress - t0) * 1e3)
                except Exception as e:  # noqa: BLE001
                    log.exception("decode step failed")
                    self._engine_failed(e)
                    self._pending = None
                    for s in list(self.active):
                        self._finish(s, "error", str(e))

    @staticmethod
    def _common(c: List[int], ids: List[int]) -> int:
        n, lim = 0, min(len(c), len(ids) - 1)  # >= 1 token is always prefilled (its logits)
        while n < lim and c[n] == ids[n]:
            n += 1
        return n

    def _pick_slot(self, ids: List[int]):
        """(slot, reused tokens): the free slot whose own cache matches best, or -- when another
        slot (free or decoding) holds a longer matching prefix -- the free slot with the least
        cached content, which then shares that prefix through the paged KV."""
        best, best_len = None, -1
        for s in self.free_slots:
            n = self._common(self.slot_cache[s], ids)
            if n > best_len:
                best, best_len = s, n
        best_len = max(best_len, 0)
        if self.share_prefix:
            src, src_len = None, best_len
            for s, c in self.slot_cache.items():
                if s != best:
                    n = self._common(c, ids)
                    if n > src_len:
                        src, src_len = s, n
            if src is not None and src_len >= best_len + self.min_shared_prefix:
                dst = min(self.free_slots, key=lambda f: len(self.slot_cache[f]))
                self.engine.copy_slot(src, dst, src_len)
                self.slot_cache[dst] = list(ids[:src_len])
                self.stats["shared_prefix_tokens"] = self.stats.get("shared_prefix_tokens", 0) + src_len
                return dst, src_len
        return best, best_len

    def _admit_embedding(self, r: GenRequest):
        """An embedding request: admitted like a prompt, prefilled by _prefill_chunk through embed_prefill."""
        ids = r.prompt_ids
        host_embedding.pooling_code(r.embed)  # (ValueError: unknown pooling)
        if not self.can_embed:
            raise ValueError(f"{self.name}: this tier's engine cannot compute embeddings")
        if not ids:
            raise ValueError("embedding input is empty")
        if len(ids) > self.max_ctx:  # (no token is generated: the whole window may be prompt)
            raise ValueError(f"prompt of {len(ids)} tokens exceeds the context window ({self.max_ctx})")
        if r.embed == "none" and any(q.req.embed == "none" for q in self.prefilling):
            # the engine stages "none" rows in one buffer for all slots: one such prompt at a time; this one
            # waits at the head of the queue until the other's last chunk is through
            with self.cv:
                self.queue.appendleft(r)
            return
        if r.embed == "last":
            slot, common = self._pick_slot(ids)  # a cached prefix serves: only the last row is pooled
        else:  # cached positions have no hidden rows to pool: from position 0, in the least useful slot
            slot, common = min(self.free_slots, key=lambda f: len(self.slot_cache[f])), 0
        self.free_slots.remove(slot)
        seq = _Seq(r, slot)
        seq.lp_n = -1
        self._begin_prefill(seq, common)

    def _begin_prefill(self, seq: _Seq, common: int):
        """An admitted sequence whose slot holds its first `common` prompt tokens: queue the rest for
        prefill, and with nothing decoding (no stream to protect) prefill it right away."""
        ids, slot = seq.req.prompt_ids, seq.slot
        seq.cached = common
        seq.pos = common
        seq.todo = list(ids[common:])
        self.slot_cache[slot] = list(ids[:common])
        self.stats["cached_tokens"] += common
        self.prefilling.append(seq)
        if not self.active:
            try:
                self._prefill_chunk(seq, whole=True)
            except Exception:
                if seq in self.prefilling:  # the caller reports the error; the slot goes back
                    self.prefilling.remove(seq)
                    self.free_slots.append(slot)
                raise

    def _admit(self, r: GenRequest):
        if r.embed is not None:
            return self._admit_embedding(r)
        ids = r.prompt_ids
        score = r.prompt_logprobs is not None
        if score:
            if isinstance(r.prompt_logprobs, bool) or not 0 <= int(r.prompt_logprobs) <= host_sampler.LOGPROB_MAX_TOP:
                raise ValueError(f"prompt_logprobs outside 0..{host_sampler.LOGPROB_MAX_TOP}")
            if not self.can_score:
                raise ValueError(f"{self.name}: this tier's engine cannot score prompts")
            if not ids:
                raise ValueError("prompt is empty")
        # (a pure scoring request generates nothing: the whole window may be prompt)
        if len(ids) >= self.max_ctx and not (score and r.max_tokens <= 0 and len(ids) == self.max_ctx):
            raise ValueError(f"prompt of {len(ids)} tokens exceeds the context window ({self.max_ctx})")
        if r.logprobs:
            if not 0 <= int(r.top_logprobs) <= host_sampler.LOGPROB_MAX_TOP:
                raise ValueError(f"top_logprobs outside 0..{host_sampler.LOGPROB_MAX_TOP}")
            if not self.can_logprobs:
                raise ValueError(f"{self.name}: this tier's engine cannot report logprobs")
        bias = self._bias_of(r)
        schema = self._schema_of(r)  # (json_schema.SchemaError, a ValueError, names the path)
        try:
            return self._admit_checked(r, ids, score, bias, schema)
        except BaseException:
            if schema is not None and not any(q.req is r for q in self.active + self.prefilling):
                self._schemas.release(schema)
            raise

    def _schema_of(self, r: GenRequest):
        """The request's compiled schema out of the tier's cache (None without one); the first schema builds the
        cache, and on a tier whose engine computes masks uploads the vocabulary's byte strings."""
        if r.json_schema is None:
            return None
        if self._schemas is None:
            tokens = self.tok.all_token_bytes()
            eos = sorted(self.eos)
            if self.can_device_grammar:
                try:
                    self.engine.grammar_vocab(tokens, eos)
                except RuntimeError as e:
                    # (more end-of-sequence ids than the kernel takes, say): the engine is fine, the tier serves
                    # schemas through the host grammar like one whose engine lacks the calls
                    self.can_device_grammar = False
                    log.warning("%s: no device grammar masks (%s); schema rows use host masks", self.name, e)
            self._schemas = json_schema.SchemaCache(json_schema.Vocab(tokens, eos),
                                                    self.engine if self.can_device_grammar else None)
        self.stats["schema_requests"] += 1
        try:
            return self._schemas.acquire(r.json_schema)
        finally:
            self.stats["schema_compiles"] = self._schemas.compiles

    def _admit_checked(self, r: GenRequest, ids, score, bias, schema):
        shift = bool(r.context_shift)
        if shift and not self.can_shift:
            raise ValueError(f"{self.name}: context_shift: single-GPU engines only")
        if not shift and self.context_shift:  # the tier's default
            shift = self.can_shift
            if not shift and not self._warned_no_shift:
                self._warned_no_shift = True
                log.warning("%s: the engine has no shift_context; context shift is off on this tier", self.name)
        # (a request that shifts is not bounded by the window)
        r.max_tokens = max(0 if score else 1, r.max_tokens if shift else min(r.max_tokens, self.max_ctx - len(ids)))
        r.min_tokens = min(r.min_tokens, r.max_tokens)
        if score:  # cached positions have no logits to score: from position 0, in the least useful slot
            slot, common = min(self.free_slots, key=lambda f: len(self.slot_cache[f])), 0
        else:
            slot, common = self._pick_slot(ids)
        self.free_slots.remove(slot)
        seq = _Seq(r, slot)
        seq.shift = shift
        seq.n_keep = len(ids) if int(r.n_keep) < 0 else min(int(r.n_keep), len(ids))
        if score:
            seq.plp_n = int(r.prompt_logprobs)
        d = self.sampling_defaults
        proc = tuple(float(d[k] if getattr(r, k) is None else getattr(r, k)) for k in NEUTRAL_PROCESSORS)
        if proc != tuple(NEUTRAL_PROCESSORS.values()):
            seq.proc = proc
            seq.pen_n = host_sampler.penalty_window(r.repeat_last_n)
        if bias is not None:
            seq.bias = bias
            keep = [j for j, v in enumerate(bias[1]) if v != -np.inf]
            seq.bias_soft = ([bias[0][j] for j in keep], [bias[1][j] for j in keep])
        seq.spec = self.spec["mode"] == "lookup" if r.speculative is None else bool(r.speculative)
        if schema is not None:
            seq.schema, seq.grammar = schema, schema.grammar
            seq.spec = False  # (schema rows take no speculative steps)
            # a row that bans tokens needs its mask bytes on the host (_bias_lists: the grammar wins)
            bans = seq.bias is not None and len(seq.bias_soft[0]) < len(seq.bias[0])
            seq.dev_grammar = schema.gid >= 0 and not bans
        elif r.json_mode:
            seq.grammar = self.grammar
        if seq.spec and not self.can_spec:
            seq.spec = False
            if not self._warned_no_spec:
                self._warned_no_spec = True
                log.warning("%s: the engine has no spec_decode; speculative decoding is off on this tier", self.name)
        self._begin_prefill(seq, common)

    def _bias_of(self, r: GenRequest):
        """The request's logit-bias list (ids, vals), or None when it has none; ValueError for a list the
        sampler does not take or a tier that cannot apply one (a ban silently dropped is worse than a
        refusal: unlike the penalties, which such a tier ignores with a log line)."""
        bias = {}
        for t, v in (r.logit_bias or {}).items():
            if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
                raise ValueError("logit_bias: token ids must be integers")
            bias[int(t)] = float(v)
        if r.ignore_eos:
            for t in self.eos:
                bias[int(t)] = -np.inf
        if not bias:
            return None
        ids, vals = list(bias), list(bias.values())
        host_sampler.check_logit_bias(ids, vals, self.vocab)
        if not self.can_bias:
            raise ValueError(f"{self.name}: logit_bias: single-GPU engines only")
        return ids, vals

    def _bias_lists(self, rows, masks: bytes = b""):
        """The rows' bias lists for one sampler launch (masks: the launch's grammar masks, b"" for none).
        The grammar wins: a row whose mask allows no unbanned token gets its list without the bans for
        this step, so the sampler never sees a row with nothing left."""
        nb = (self.vocab + 7) // 8
        ids, vals = [], []
        for b, s in enumerate(rows):
            bias = s.bias or ((), ())
            if s.bias is not None and masks and s.grammar_state is not None and len(s.bias_soft[0]) < len(bias[0]):
                m = masks[b * nb:(b + 1) * nb]
                allowed = int.from_bytes(m, "little").bit_count()
                hit = sum(1 for t, v in zip(*bias) if v == -np.inf and (m[t >> 3] >> (t & 7)) & 1)
                if allowed and hit >= allowed:
                    bias = s.bias_soft
                    self.stats["bias_overridden"] += 1
            ids.append(list(bias[0]))
            vals.append(list(bias[1]))
        return ids, vals

    def _prefill_chunk(self, seq: _Seq, whole: bool = False):
        """Prefill the next chunk of seq's prompt; the last chunk samples the first token and
        moves the sequence to the decoding set."""
        r = seq.req
        if r.cancelled:
            self._finish(seq, "cancelled")
            return
        n = len(seq.todo) if (whole or not self.active) else min(len(seq.todo), max(1, self.prefill_chunk))
        chunk, last = seq.todo[:n], n == len(seq.todo)
        tp0 = time.perf_counter()
        if r.embed is not None:
            emb = self.engine.embed_prefill(seq.slot, chunk, seq.pos, host_embedding.POOLING[r.embed], last)
        elif seq.plp_n >= 0:
            # the last row's target is the next chunk's first token; the prompt's last row has none
            sc = self.engine.score_prefill(seq.slot, chunk, seq.pos, -1 if last else int(seq.todo[n]), seq.plp_n,
                                           last and r.max_tokens > 0)
            self._take_scores(seq, chunk, sc, last)
        else:
            logits = self.engine.prefill(seq.slot, chunk, seq.pos, last)
        self.timing["prefill_s"] += time.perf_counter() - tp0
        self.step_log.append((time.perf_counter(), -n))  # a prefill chunk between decode steps
        seq.todo = seq.todo[n:]
        seq.pos += n
        self.slot_cache[seq.slot].extend(chunk)
        self.stats["prefill_tokens"] += n
        if not last:
            return
        if r.embed is not None:  # the request ends here; the slot keeps the prompt's KV for a later chat
            seq.embedding = np.asarray(emb, np.float32)
            self.stats["embeddings"] += 1
            self._finish(seq, "embedding")
            return
        if seq.plp_n >= 0:
            self.stats["prompt_scores"] += 1
            if r.max_tokens <= 0:  # a pure scoring request: no token is sampled
                self._finish(seq, "length")
                return
            if not hasattr(self.engine, "sample_first"):
                logits = np.asarray(self.engine.last_logits(1), np.float32)
        self.prefilling.remove(seq)
        mask = None
        if seq.grammar is not None:
            seq.grammar_state = seq.grammar.initial()
            if not seq.dev_grammar:
                mask = self._mask(seq)
        topk = int(r.top_k) if r.temperature > 0 else 0
        topp = float(r.top_p) if 0.0 < r.top_p < 1.0 else 1.0
        if hasattr(self.engine, "sample_first"):
            # on the device, the decode steps' sampler and RNG stream (seed, position)
            self._processors([seq], bytes(mask) if mask is not None else b"")
            self._stage_logprobs([seq])
            self._stage_grammar([seq])
            tok = int(self.engine.sample_first(seq.pos - 1, float(r.temperature), topk, topp, seq.seed,
                                               bytes(mask) if mask is not None else b""))
            lp = self._read_logprobs([seq])[0]
        else:
            rng = np.random.default_rng([seq.seed & 0xFFFFFFFF, seq.pos - 1])
            min_p = 0.0
            raw = logits
            if seq.bias is not None:
                bi, bv = self._bias_lists([seq], bytes(mask) if mask is not None else b"")
                logits = host_sampler.apply_logit_bias(logits, bi[0], bv[0])
            if seq.proc is not None:
                min_p = seq.proc[0]
                logits = host_sampler.apply_penalties(logits, self._window(seq), *seq.proc[1:])
            tok = host_sampler.sample(logits, r.temperature, r.top_k, r.top_p, mask, rng, min_p=min_p)
            lp = None
            if seq.lp_n >= 0:  # (`raw`: the prefill's logits, before the penalties above)
                x, ids, xs = host_sampler.logprobs(raw, tok, seq.lp_n)
                lp = (x, list(zip(ids, xs)))
        seq.t_first = time.time()
        self.active.append(seq)
        if seq.spec:  # (before the first token: _accept appends every emitted token to the drafter's context)
            sp = self.spec
            seq.drafter = speculative_mod.LookupDrafter(r.prompt_ids, r.prediction_ids, sp["ngram_min"], sp["ngram_max"],
                                                        sp["draft_max"])
        self._accept(seq, tok, lp)

    @staticmethod
    def _take_scores(seq: _Seq, chunk: List[int], sc: dict, last: bool):
        """Append a score_prefill result to seq.plps: row i of the chunk scored the token after it."""
        if seq.pos == 0:
            seq.plps.append((int(chunk[0]), None, None, []))
        targets = list(chunk[1:]) + ([] if last else [int(seq.todo[len(chunk)])])
        lp, rank = sc["lp"], sc["rank"]
        ids, lps = (sc["ids"], sc["lps"]) if seq.plp_n > 0 else (None, None)
        for i, t in enumerate(targets):
            top = [(int(a), float(x)) for a, x in zip(ids[i], lps[i]) if a >= 0] if ids is not None else []
            seq.plps.append((int(t), float(lp[i]), int(rank[i]), top))

    def _accept(self, seq: _Seq, tok: int, lp=None) -> bool:
        """Record a sampled token (lp: its logprob entry, kept only with a token that is emitted);
        returns False when the sequence finished."""
        r = seq.req
        if r.cancelled:
            self._finish(seq, "cancelled")
            return False
        if tok in self.eos or (r.stop_ids and tok in r.stop_ids):
            self._finish(seq, "stop")
            return False
        if seq.grammar_state is not None:
            if not seq.grammar.accept_token(seq.grammar_state, tok):
                self._finish(seq, "stop")
                return False
        seq.out.append(tok)
        if seq.drafter is not None:
            seq.drafter.append(tok)
        if seq.lp_n >= 0:
            seq.lps.append((int(tok), lp[0], lp[1]))
        seq.last = tok
        self.stats["tokens"] += 1
        self._tok_times.append(time.time())
        if r.on_delta is not None:
            # incremental detokenization over a short window (decoding the whole output every
            # token is O(n^2) per stream and dominated the host side of a step)
            prev = self.tok.decode(seq.out[seq.p_off:seq.r_off])
            text = self.tok.decode(seq.out[seq.p_off:])
            if len(text) > len(prev) and not text.endswith("�"):
                delta = text[len(prev):]
                seq.emitted += delta
                seq.p_off, seq.r_off = seq.r_off, len(seq.out)
                r.on_delta(delta)
        if seq.grammar_state is not None and seq.grammar.complete(seq.grammar_state):
            self._finish(seq, "grammar")
            return False
        if len(seq.out) >= r.max_tokens or (seq.pos + 1 >= self.max_ctx and not (seq.shift and self._shift(seq))):
            self._finish(seq, "length")
            return False
        if r.deadline and time.time() > r.deadline:
            self._finish(seq, "deadline")
            return False
        return True

    def _shift(self, seq: _Seq) -> bool:
        """The slot reached the window: drop n_discard = (n_past - n_keep) // 2 tokens behind the first n_keep
        (llama.cpp's numbers) through the engine's shift_context and go on at the new position; the next step of
        the row is host-fed (no forward of it is queued: _can_speculate refuses a row this close to the window).
        False: nothing can be dropped, or the pool has no block for the un-sharing -- the request ends "length"."""
        self._drain()  # (no other engine call while a pipelined step is in flight)
        n_past = seq.pos
        n_discard = (n_past - seq.n_keep) // 2
        if n_discard < 1:
            return False
        try:
            seq.pos = int(self.engine.shift_context(seq.slot, n_past, seq.n_keep, n_discard))
        except RuntimeError as e:
            if "pool exhausted" not in str(e):
                raise
            return False
        # the moved keys are not what a prefill of those tokens would write: never inherited as a prefix
        seq.shifts += 1
        del self.slot_cache[seq.slot][seq.n_keep:]
        self.stats["context_shifts"] += 1
        self.stats["shifted_tokens"] += n_past - seq.n_keep - n_discard
        return True

    def _advance(self, s: _Seq):
        """The row's token went in at s.pos: the position moves on, and so does the slot's record of cached tokens
        (until the first context shift: behind it the slot no longer holds what a prefill would write)."""
        s.pos += 1
        if not s.shifts:
            self.slot_cache[s.slot].append(s.last)

    def _engine_failed(self, e: BaseException):
        self.stats["errors"] += 1
        self.failed = f"{type(e).__name__}: {e}"

    def stalled(self, timeout_s: float) -> bool:
        """Work is pending but nothing completed for timeout_s (a hung device call)."""
        return bool(self.active or self.queue) and time.time() - self.last_progress > timeout_s

    def metrics(self) -> dict:
        now = time.time()
        while self._tok_times and now - self._tok_times[0] > 10.0:
            self._tok_times.popleft()
        ttft = sorted(self._ttft)
        st = self.stats
        return {"tokens_per_s": len(self._tok_times) / 10.0,
                "ttft_p50_ms": ttft[len(ttft) // 2] if ttft else 0.0,
                "itl_ms": sum(self._step_ms) / len(self._step_ms) if self._step_ms else 0.0,
                # a sequence mid chunked-prefill holds a slot and is work in flight: it
                # counts as active for idle-unload and replica routing
                "active": len(self.active) + len(self.prefilling), "decoding": len(self.active),
                "prefilling": len(self.prefilling), "queued": len(self.queue),
                "kv_slot_util": (len(self.active) + len(self.prefilling)) / max(1, self.max_slots),
                "avg_batch": st["batch_sum"] / st["steps"] if st["steps"] else 0.0,
                "prefix_hit_tokens": st["cached_tokens"], "errors": st["errors"],
                # accepted / verified draft tokens of the speculative steps so far (0 when none ran)
                "spec_accept_rate": st["spec_accepted"] / st["spec_drafted"] if st["spec_drafted"] else 0.0}

    def _mask(self, seq: _Seq) -> bytes:
        # the next token may not complete the object (schema rows ignore min_tokens)
        if seq.schema is None and len(seq.out) + 1 < seq.req.min_tokens:
            return seq.grammar.mask_open(seq.grammar_state)
        return seq.grammar.mask(seq.grammar_state)

    def _drain(self):
        """Collect and accept a pipelined step still in flight (before any other engine call)."""
        rows = self._pending
        if rows is None:
            return
        self._pending = None
        try:
            out = self.engine.decode_collect()
        except Exception as e:  # noqa: BLE001
            log.exception("decode step failed")
            self._engine_failed(e)
            for s in list(self.active):
                self._finish(s, "error", str(e))
            return
        self._take(rows, out)

    def _discard_pending(self):
        if self._pending is not None:
            self._pending = None
            try:
                self.engine.decode_collect()
            except Exception:  # noqa: BLE001
                pass

    def _take(self, rows, out):
        self.stats["steps"] += 1
        self.stats["batch_sum"] += len(rows)
        lps = self._read_logprobs(rows)
        for s, t, lp in zip(rows, out, lps):
            self._advance(s)
            self._accept(s, int(t), lp)

    def _can_speculate(self, rows) -> bool:
        """Whether step t+1 of the same rows can be queued before step t's tokens are known: no
        admission or prefill will interleave, and no row is certain to finish at step t."""
        if self.prefilling or (self.queue and self.free_slots and
                               len(self.active) + len(self.prefilling) < self.max_batch):
            return False
        now = time.time()
        for s in rows:
            r = s.req
            if r.cancelled or len(s.out) + 1 >= r.max_tokens or s.pos + 2 >= self.max_ctx:
                return False
            if r.deadline and now > r.deadline:
                return False
        return True

    def _submit(self, rows, first: bool):
        """Queue the forward of the rows' next step: `first` with the host's tokens at s.pos, else
        with the tokens the in-flight sampler leaves on the device, at s.pos + 1."""
        self.engine.decode_submit([s.slot for s in rows], [s.last for s in rows] if first else [],
                                  [s.pos + (0 if first else 1) for s in rows],
                                  [float(s.req.temperature) for s in rows],
                                  [int(s.req.top_k) if s.req.temperature > 0 else 0 for s in rows], 0,
                                  [float(s.req.top_p) if 0.0 < s.req.top_p < 1.0 else 1.0 for s in rows],
                                  [s.seed for s in rows])

    @staticmethod
    def _window(s: _Seq, extra=()) -> List[int]:
        """the row's penalty window: its last pen_n tokens, prompt tail included (extra: draft tokens that
        stand behind `out` for a row of a speculative step)"""
        n = s.pen_n
        if n <= 0:
            return []
        out = s.out + list(extra) if extra else s.out
        return (s.req.prompt_ids[-(n - len(out)):] if len(out) < n else []) + out[-n:]

    def _processors(self, rows, masks: bytes = b"", windows=None):
        """Before a sampler launch: hand the engine the rows' min-p / penalties and penalty windows
        (every token of a row is on the host at this point) and their logit-bias lists (masks: the
        launch's grammar masks, for _bias_lists).  All rows neutral: no call at all.  windows: the rows'
        penalty windows where they are not the sequences' own (a speculative step's rows stand behind drafts)."""
        biased = any(s.bias is not None for s in rows)
        if not biased and not any(s.proc is not None for s in rows):
            return
        setp = getattr(self.engine, "set_sample_processors", None)
        if setp is None:
            if not self._warned_no_processors:
                self._warned_no_processors = True
                log.warning("%s: the engine has no set_sample_processors; min_p and penalties are ignored", self.name)
            return
        neutral = tuple(NEUTRAL_PROCESSORS.values())
        cols = list(zip(*[s.proc or neutral for s in rows]))
        if windows is None:
            windows = [self._window(s) if s.proc is not None else [] for s in rows]
        if biased:
            setp(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), windows, *self._bias_lists(rows, masks))
        else:
            setp(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), windows)

    def _stage_logprobs(self, rows):
        """Before a sampler launch, after _processors: the rows' top_logprobs for the engine's logprob
        launch behind it.  No row asks: no call at all."""
        if any(s.lp_n >= 0 for s in rows):
            self.engine.set_logprobs([s.lp_n for s in rows])

    def _read_logprobs(self, rows) -> list:
        """After the rows' sampled tokens reached the host: one entry per row, (the token's logprob,
        [(alternative id, logprob), ...]) or None for a row that did not ask."""
        if not any(s.lp_n >= 0 for s in rows):
            return [None] * len(rows)
        got = self.engine.last_logprobs()
        if len(got) != 3 or len(got[0]) != len(rows):
            raise RuntimeError("the engine returned no logprobs for a step that staged them")
        lp, ids, lps = got
        out = []
        for b, s in enumerate(rows):
            if s.lp_n < 0:
                out.append(None)
                continue
            top = [(int(i), float(x)) for i, x in zip(ids[b][:s.lp_n], lps[b][:s.lp_n]) if i >= 0]
            out.append((float(lp[b]), top))
        return out

    def _masks(self, rows) -> bytes:
        """The launch's host masks: b"" when no row needs one; else one per row, all ones for a free row and for a
        row whose mask the device writes over it (_stage_grammar)."""
        if not any(s.grammar_state is not None and not s.dev_grammar for s in rows):
            return b""
        if self._full_mask is None:
            self._full_mask = host_sampler.all_allowed(self.vocab)
        return b"".join(self._mask(s) if s.grammar_state is not None and not s.dev_grammar else self._full_mask
                        for s in rows)

    def _stage_grammar(self, rows):
        """Before a sampler launch: the (grammar id, state) of the rows whose mask the device computes.  No such
        row: no call at all."""
        if any(s.dev_grammar for s in rows):
            self.engine.set_grammar_rows([s.schema.gid if s.dev_grammar else -1 for s in rows],
                                         [s.grammar_state.s if s.dev_grammar else 0 for s in rows])

    def _step_pipelined(self):
        t0 = time.perf_counter()
        rows = self._pending
        if rows is None:  # a batch's first step (or after an admission / finish): host tokens
            rows = list(self.active)
            self._submit(rows, True)
            masks = self._masks(rows)
            self._processors(rows, masks)
            self._stage_logprobs(rows)
            self._stage_grammar(rows)
            self.engine.decode_sample(masks)
        self._pending = None
        spec = self._can_speculate(rows)
        if spec:
            self._submit(rows, False)
        t1 = time.perf_counter()
        out = self.engine.decode_collect()
        t2 = time.perf_counter()
        self._take(rows, out)
        t2b = time.perf_counter()
        if spec and self.active == rows:
            # nobody finished or joined: sample the queued forward with the masks of the new tokens
            masks = self._masks(rows)
            self._processors(rows, masks)
            self._stage_logprobs(rows)
            self._stage_grammar(rows)
            self.engine.decode_sample(masks)
            self._pending = rows
        # (spec and a row finished: the queued forward is dropped -- its KV writes at the next
        # position are rewritten by whatever runs there next)
        t3 = time.perf_counter()
        tm = self.timing
        tm["mask_s"] += (t3 - t2b) + (t1 - t0)   # masks + submit / sampler enqueue
        tm["engine_decode_s"] += t2 - t1          # waiting for the device
        tm["accept_s"] += t2b - t2
        self.step_log.append((t3, len(rows)))

    def _spec_draft(self, s: _Seq):
        """The draft of s's next speculative step and its rows' masks: the drafter's proposal, trimmed so
        that no row can run past the request's end -- to max_tokens and the context window, before the first
        EOS / stop id, and for a grammar row before the first token the grammar rejects or that would
        complete the value (row i's mask is the grammar's after drafts 0..i-1)."""
        r = s.req
        rows_max = min(self.max_batch, speculative_mod.DRAFT_MAX_LIMIT + 1)
        lim = min(r.max_tokens - len(s.out) - 1, self.max_ctx - s.pos - 2, rows_max - 1)
        draft = list(s.drafter.draft(lim)) if lim > 0 else []
        for i, t in enumerate(draft):
            if t in self.eos or (r.stop_ids and t in r.stop_ids):
                draft = draft[:i]
                break
        masks = b""
        if draft and s.grammar_state is not None:
            st = s.grammar_state.copy()
            ms = [self._mask(s)]
            for i, t in enumerate(draft):
                if not s.grammar.accept_token(st, t) or s.grammar.complete(st):
                    draft = draft[:i]
                    break
                open_ = len(s.out) + i + 2 < r.min_tokens  # (_mask's rule for the row behind draft i)
                ms.append(s.grammar.mask_open(st) if open_ else s.grammar.mask(st))
            masks = b"".join(ms[:len(draft) + 1])
        return draft, masks

    def _spec_step(self) -> bool:
        """A speculative step instead of a plain one, when exactly one sequence decodes, speculation is on
        for it, nothing is prefilling and its drafter proposes something: the last token and the draft go
        through the engine as consecutive rows of one step (Engine.spec_decode), and every token it emits
        is accepted in order, as if each came from a step of its own.  Several sequences decoding: the
        multi-sequence step below.  False: nothing ran, the caller takes a plain step."""
        if len(self.active) > 1:
            return self._spec_step_multi()
        if len(self.active) != 1 or self.prefilling or not self.active[0].spec:
            return False
        s = self.active[0]
        if self._pending is not None:
            # The draft needs the in-flight step's token, and collecting it early gives up that step's
            # overlap of host and device work.  So only when a draft can follow: the context is short enough
            # and the text in front of the unknown token has occurred before with two tokens behind it (the
            # drafter's necessary condition; text that does not repeat stays fully pipelined).
            if s.pos + 2 > self.spec["max_context"] or not s.drafter.may_draft_after_next():
                return False
            self._drain()
            if self.active != [s]:  # (the collected token finished the request, or the step failed)
                return False
        if s.pos + 1 > self.spec["max_context"]:  # every row re-reads the slot's K/V: no gain past this
            return False
        t0 = time.perf_counter()
        draft, masks = self._spec_draft(s)
        if not draft:
            return False
        r, R = s.req, len(draft) + 1
        rows = [s] * R
        if s.bias is not None:  # the same list on each of the R rows (the grammar-wins test is per row's mask)
            proc = s.proc or tuple(NEUTRAL_PROCESSORS.values())
            self.engine.set_sample_processors(*[[v] * R for v in proc],
                                              [self._window(s, draft[:i]) if s.proc is not None else [] for i in range(R)],
                                              *self._bias_lists(rows, masks))
        elif s.proc is not None and hasattr(self.engine, "set_sample_processors"):
            self.engine.set_sample_processors(*[[v] * R for v in s.proc], [self._window(s, draft[:i]) for i in range(R)])
        self._stage_logprobs(rows)
        t1 = time.perf_counter()
        acc, out = self.engine.spec_decode(s.slot, [s.last] + draft, s.pos, float(r.temperature),
                                           int(r.top_k) if r.temperature > 0 else 0,
                                           float(r.top_p) if 0.0 < r.top_p < 1.0 else 1.0, s.seed, masks)
        t2 = time.perf_counter()
        st = self.stats
        st["steps"] += 1
        st["batch_sum"] += 1
        st["spec_steps"] += 1
        st["spec_drafted"] += len(draft)
        st["spec_accepted"] += int(acc)
        s.drafted += len(draft)
        s.draft_hits += int(acc)
        lps = self._read_logprobs(rows)
        for i, t in enumerate(out):  # stops at the first token that finishes the request: the rest is dropped
            self._advance(s)
            if not self._accept(s, int(t), lps[i]):
                break
        t3 = time.perf_counter()
        tm = self.timing
        tm["mask_s"] += t1 - t0
        tm["engine_decode_s"] += t2 - t1
        tm["accept_s"] += t3 - t2
        self.step_log.append((t3, 1))
        return True

    def _spec_step_multi(self) -> bool:
        """A speculative step while 2..8 sequences decode (Engine.spec_decode_multi): every active sequence goes
        in as one segment, its last token and its draft -- no draft (speculation off for it, nothing proposed, a
        schema-grammar row, a context past spec_max_context): a one-row segment that rides along -- and each
        sequence's emitted tokens are accepted in order, as if each came from a step of its own.  The drafts
        are trimmed longest-first until the rows fit min(max_batch, 32).  False: nothing ran (no sequence
        brought a draft, or the tier does not take such steps), the caller takes a plain step."""
        S = len(self.active)
        cap = min(self.max_batch, speculative_mod.MULTI_ROWS_MAX)
        if (not self.spec["multi"] or not self.can_spec_multi or self.prefilling or S > speculative_mod.MULTI_SEQS_MAX or
                S >= cap or not any(s.spec for s in self.active)):
            return False
        ctx = self.spec["max_context"]
        if self._pending is not None:
            # _spec_step's rule: the in-flight step is collected early only if some sequence may then draft
            if not any(s.spec and s.pos + 2 <= ctx and s.drafter.may_draft_after_next() for s in self.active):
                return False
            self._drain()
            if len(self.active) < 2 or self.prefilling:  # (collected tokens finished sequences, or the step failed)
                return self._spec_step() if len(self.active) == 1 else False
            S = len(self.active)
        t0 = time.perf_counter()
        seqs = list(self.active)
        parts = [self._spec_draft(s) if s.spec and s.pos + 1 <= ctx else ([], b"") for s in seqs]
        drafts = [list(d) for d, _ in parts]
        if not any(drafts):
            return False
        while S + sum(len(d) for d in drafts) > cap:  # the longest draft gives up its last token (first among equals)
            max(drafts, key=len).pop()
        rows = [s for s, d in zip(seqs, drafts) for _ in range(len(d) + 1)]
        masks = b""
        if any(s.grammar_state is not None and not s.dev_grammar for s in seqs):
            if self._full_mask is None:
                self._full_mask = host_sampler.all_allowed(self.vocab)
            nb = len(self._full_mask)
            ms = []
            for s, d, (_, m) in zip(seqs, drafts, parts):
                if s.grammar_state is not None and not s.dev_grammar:
                    ms.append((m or self._mask(s))[:(len(d) + 1) * nb])  # (row i: the grammar after drafts 0..i-1)
                else:
                    ms.append(self._full_mask * (len(d) + 1))
            masks = b"".join(ms)
        # the rows' processors as _spec_step stages them for its R rows, segment after segment: row i of a
        # segment has the drafts before it behind the sequence's own tokens in its penalty window
        self._processors(rows, masks, windows=[self._window(s, d[:i]) if s.proc is not None else []
                                               for s, d in zip(seqs, drafts) for i in range(len(d) + 1)])
        self._stage_logprobs(rows)
        self._stage_grammar(rows)
        t1 = time.perf_counter()
        res = self.engine.spec_decode_multi(
            [s.slot for s in seqs], [[s.last] + d for s, d in zip(seqs, drafts)], [s.pos for s in seqs],
            [float(s.req.temperature) for s in seqs], [int(s.req.top_k) if s.req.temperature > 0 else 0 for s in seqs],
            [float(s.req.top_p) if 0.0 < s.req.top_p < 1.0 else 1.0 for s in seqs], [s.seed for s in seqs], masks)
        t2 = time.perf_counter()
        st = self.stats
        st["steps"] += 1
        st["batch_sum"] += S
        st["spec_steps"] += 1
        st["spec_multi_steps"] += 1
        lps = self._read_logprobs(rows)
        r0 = 0
        for s, d, (acc, out) in zip(seqs, drafts, res):
            st["spec_drafted"] += len(d)
            st["spec_accepted"] += int(acc)
            s.drafted += len(d)
            s.draft_hits += int(acc)
            for i, t in enumerate(out):  # stops at the first token that finishes the request: the rest is dropped
                self._advance(s)
                if not self._accept(s, int(t), lps[r0 + i]):
                    break
            r0 += len(d) + 1
        t3 = time.perf_counter()
        tm = self.timing
        tm["mask_s"] += t1 - t0
        tm["engine_decode_s"] += t2 - t1
        tm["accept_s"] += t3 - t2
        self.step_log.append((t3, S))
        return True

    def _step(self):
        if self._spec_step():
            return
        if not self.active:  # (_spec_step collected a pipelined step whose token finished the last sequence)
            return
        if self.pipeline:
            return self._step_pipelined()
        B = len(self.active)
        slots = [s.slot for s in self.active]
        toks = [s.last for s in self.active]
        pos = [s.pos for s in self.active]
        temps = [float(s.req.temperature) for s in self.active]
        topk = [int(s.req.top_k) if s.req.temperature > 0 else 0 for s in self.active]
        seeds = [s.seed for s in self.active]  # per row: a request samples the same at any batch row
        t0 = time.perf_counter()
        mask = self._masks(self.active)
        topp = [float(s.req.top_p) if 0.0 < s.req.top_p < 1.0 else 1.0 for s in self.active]
        rows = list(self.active)
        self._processors(rows, mask)
        self._stage_logprobs(rows)
        self._stage_grammar(rows)
        t1 = time.perf_counter()
        out = self.engine.decode(slots, toks, pos, temps, topk, 0, mask, topp, seeds)
        t2 = time.perf_counter()
        self.stats["steps"] += 1
        self.stats["batch_sum"] += B
        lps = self._read_logprobs(rows)
        for s, t, lp in zip(rows, out, lps):
            self._advance(s)
            self._accept(s, int(t), lp)
        t3 = time.perf_counter()
        tm = self.timing
        tm["mask_s"] += t1 - t0
        tm["engine_decode_s"] += t2 - t1
        tm["accept_s"] += t3 - t2
        self.step_log.append((t3, B))

    def _finish(self, seq: _Seq, reason: str, error: str = ""):
        if seq in self.active:
            self.active.remove(seq)
        if seq in self.prefilling:
            self.prefilling.remove(seq)
        self.free_slots.append(seq.slot)
        if seq.schema is not None:  # (an evicted schema's device tables go with its last row)
            self._schemas.release(seq.schema)
            seq.schema = None
        r = seq.req
        text = self.tok.decode(seq.out)
        if r.on_delta is not None and len(text) > len(seq.emitted) and text.startswith(seq.emitted):
            r.on_delta(text[len(seq.emitted):])
        now = time.time()
        if seq.t_first:
            self._ttft.append((seq.t_first - r.submitted_at) * 1e3)
        self._done(r, GenResult(
            text=text, token_ids=list(seq.out), prompt_tokens=len(r.prompt_ids), completion_tokens=len(seq.out),
            finish_reason=reason, ttft_ms=(seq.t_first - r.submitted_at) * 1e3 if seq.t_first else 0.0,
            latency_ms=(now - r.submitted_at) * 1e3, cached_prompt_tokens=seq.cached, error=error,
            logprobs=list(seq.lps) if seq.lp_n >= 0 else None, embedding=seq.embedding,
            prompt_logprobs=list(seq.plps) if seq.plp_n >= 0 else None,
            draft_tokens=seq.drafted, accepted_draft_tokens=seq.draft_hits, context_shifts=seq.shifts))

    @staticmethod
    def _done(r: GenRequest, res: GenResult):
        if r.on_done is not None:
            try:
                r.on_done(res)
            except Exception:  # noqa: BLE001
                log.exception("on_done callback failed")
