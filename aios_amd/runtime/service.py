"""AIRuntime gRPC service (:50055) + per-model OpenAI-compatible HTTP endpoints.

RPC semantics follow the reference (`runtime/src/grpc_service.rs:28-178`,
`runtime/src/inference.rs:94-186`): unary Infer always uses JSON mode, max_tokens <= 0 -> 512,
temperature == 0 -> 0.7 (API-compatible default; a *negative* temperature requests greedy
decoding, App. A #3), tokens_used = prompt + completion, latency_ms = wall time.  StreamInfer
streams real token deltas as they are generated (App. A #2).

HTTP (per loaded model on its `ModelStatus.port`, like llama-server): POST /v1/chat/completions
(+ `stream: true` SSE, `response_format: {"type":"json_object"}`), POST /v1/completions, POST
/v1/embeddings and GET /health -- so the
gateway's `local` provider (`LOCAL_LLM_URL`, default :8082) can reach the local strategic tier.
"""
from __future__ import annotations

import asyncio
import json
import logging
import math
import os
import time
from typing import Dict, List, Optional

import grpc
import numpy as np

from ..rpc.schema import pb
from . import json_schema
from .chat_template import build_messages
from .embedding import MAX_INPUTS as MAX_EMBED_INPUTS
from .model_manager import ModelManager, RoutingError
from .sampler import BIAS_MAX, LOGPROB_MAX_TOP
from .scheduler import GenRequest, GenResult

log = logging.getLogger("aios.runtime.service")


def _gen_params(temperature: float, max_tokens: int):
    if max_tokens <= 0:
        max_tokens = 512
    if temperature < 0:
        temperature = 0.0
    elif temperature == 0:
        temperature = 0.7
    return float(temperature), int(max_tokens)


def _json_min_tokens(max_tokens: int) -> int:
    """AIOS_JSON_MIN_TOKENS (benchmarks only): JSON-mode generations run to this many tokens before
    the grammar lets the object close ("max": to max_tokens) -- a fixed plan length, since
    random-init weights close a JSON object at arbitrary points."""
    v = os.environ.get("AIOS_JSON_MIN_TOKENS", "").strip()
    if not v:
        return 0
    return max_tokens if v == "max" else min(max_tokens, int(v))


# request-body fields of /v1/chat/completions that map onto GenRequest fields of the same name
SAMPLING_FIELDS = {"top_p": float, "top_k": int, "seed": int, "min_p": float, "repeat_penalty": float,
                   "presence_penalty": float, "frequency_penalty": float}


def sampling_from_body(body: dict) -> dict:
    """the sampling fields an OpenAI / llama-server client sent (absent or null ones stay the
    request's and the tier's defaults)"""
    return {k: cast(body[k]) for k, cast in SAMPLING_FIELDS.items() if body.get(k) is not None}


LOGPROB_NEG_INF = -9999.0  # -inf is not valid JSON; OpenAI reports it as -9999.0


def logprobs_from_body(body: dict, scheduler) -> Optional[int]:
    """`logprobs` / `top_logprobs` of a /v1/chat/completions body: None (not asked) or the number of
    alternatives per token; ValueError (-> 400) for what OpenAI rejects and what this runtime cannot serve"""
    want, top = body.get("logprobs"), body.get("top_logprobs")
    if want is not None and not isinstance(want, bool):
        raise ValueError("logprobs must be a boolean")
    if top is not None:
        if not want:
            raise ValueError("top_logprobs requires logprobs: true")
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= LOGPROB_MAX_TOP:
            raise ValueError(f"top_logprobs must be an integer in 0..{LOGPROB_MAX_TOP}")
    if not want:
        return None
    if body.get("stream"):
        raise ValueError("logprobs are not available with stream: true")
    if not getattr(scheduler, "can_logprobs", False):  # (a tensor-parallel tier: vocab-parallel lm_head)
        raise ValueError("this model's engine cannot report logprobs")
    return int(top or 0)


def bias_from_body(body: dict, scheduler):
    """`logit_bias` and `ignore_eos` of a chat or completions body: (GenRequest.logit_bias, GenRequest.ignore_eos).
    logit_bias: OpenAI's map {"<token id>": number} or llama-server's list [[id, number | false], ...] (false:
    a ban, as -inf is); values outside OpenAI's [-100, 100] are taken as they are.  ValueError (-> 400) for a
    malformed field and on a tier whose engine cannot apply one (a tensor-parallel tier)."""
    raw, ieos = body.get("logit_bias"), body.get("ignore_eos")
    if ieos is not None and not isinstance(ieos, bool):
        raise ValueError("ignore_eos must be a boolean")
    if raw is None and not ieos:  # (a body without the fields asks nothing of the tier)
        return None, False
    vocab = scheduler.vocab
    bias = {}

    def entry(tid, v):
        if isinstance(tid, str):
            try:
                tid = int(tid.strip())
            except ValueError:
                raise ValueError(f"logit_bias: key {tid!r} is not an integer token id") from None
        if isinstance(tid, bool) or not isinstance(tid, int) or not 0 <= tid < vocab:
            raise ValueError(f"logit_bias: token id {tid!r} outside [0, {vocab})")
        if v is False:
            v = -math.inf
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"logit_bias: the bias of token {tid} must be a number (or false: a ban)")
        v = float(v)
        if v != v or v == math.inf:
            raise ValueError(f"logit_bias: the bias of token {tid} must be finite or -inf")
        if tid in bias:
            raise ValueError(f"logit_bias: duplicate token id {tid}")
        bias[tid] = v

    if isinstance(raw, dict):
        for k, v in raw.items():
            entry(k, v)
    elif isinstance(raw, list):
        for it in raw:
            if not isinstance(it, (list, tuple)) or len(it) != 2 or isinstance(it[0], str):
                raise ValueError("logit_bias: the list form takes [token id, bias] pairs")
            entry(it[0], it[1])
    elif raw is not None:
        raise ValueError("logit_bias must be a map of token ids to biases or a list of [token id, bias] pairs")
    if len(bias) > BIAS_MAX:
        raise ValueError(f"logit_bias: more than {BIAS_MAX} entries")
    if (bias or ieos) and not getattr(scheduler, "can_bias", False):
        raise ValueError("logit_bias: single-GPU engines only" if bias else "ignore_eos: single-GPU engines only")
    return (bias or None), bool(ieos)


def schema_from_body(body: dict):
    """The JSON schema a chat or completions body asks the answer to validate against, or None: OpenAI's
    `response_format: {"type": "json_schema", "json_schema": {"name", "schema", "strict"}}`, llama-server's
    `response_format: {"type": "json_object", "schema": {...}}` and its top-level `json_schema: {...}`.  The schema
    is compiled here (runtime/json_schema.py: compile_cached, where the scheduler's cache then finds the table;
    a pure-Python compile, so the handlers call this in an executor, off the event loop): ValueError
    (-> 400) for a malformed field and for a schema outside the accepted subset, naming the JSON path."""
    rf, where, schema = body.get("response_format"), None, None
    if rf is not None and not isinstance(rf, dict):
        raise ValueError("response_format must be an object")
    if rf and rf.get("type") == "json_schema":
        js = rf.get("json_schema")
        if not isinstance(js, dict):
            raise ValueError("response_format.json_schema must be an object")
        where, schema = "response_format.json_schema.schema", js.get("schema")
    elif rf and rf.get("type") == "json_object" and "schema" in rf:
        where, schema = "response_format.schema", rf["schema"]
    if "json_schema" in body and body["json_schema"] is not None:
        if where is not None:
            raise ValueError(f"json_schema: the body also names {where}")
        where, schema = "json_schema", body["json_schema"]
    if where is None:
        return None
    if not isinstance(schema, dict):
        raise ValueError(f"{where} must be an object")
    try:
        json_schema.compile_cached(schema)
    except json_schema.SchemaError as e:
        raise ValueError(f"{where}: {e}") from None
    return schema


def shift_from_body(body: dict, scheduler):
    """`context_shift` (a boolean) and `n_keep` (an integer >= -1; -1: the whole prompt) of a chat or completions
    body, llama-server's fields: (GenRequest.context_shift, GenRequest.n_keep, whether usage reports
    context_shifts -- the body names one of the fields or the tier shifts by default).  ValueError (-> 400) for a
    malformed field and on a tier whose engine cannot shift (a tensor-parallel or CPU tier)."""
    flag, keep = body.get("context_shift"), body.get("n_keep")
    if flag is not None and not isinstance(flag, bool):
        raise ValueError("context_shift must be a boolean")
    if keep is not None and (isinstance(keep, bool) or not isinstance(keep, int) or keep < -1):
        raise ValueError("n_keep must be an integer >= -1")
    if flag and not getattr(scheduler, "can_shift", False):
        raise ValueError("context_shift: single-GPU engines only")
    named = "context_shift" in body or "n_keep" in body
    return bool(flag), -1 if keep is None else int(keep), named or bool(getattr(scheduler, "context_shift", False))


def prediction_from_body(body: dict, tokenizer):
    """`prediction` (OpenAI's Predicted Outputs) and `speculative` (a boolean, an extension) of a chat or
    completions body: (GenRequest.speculative, GenRequest.prediction_ids).  A prediction turns prompt-lookup
    speculation on for the request unless `speculative` says otherwise; its text is only a source of drafts,
    the output is what the model samples.  ValueError (-> 400) for a malformed field."""
    spec, pred = body.get("speculative"), body.get("prediction")
    if spec is not None and not isinstance(spec, bool):
        raise ValueError("speculative must be a boolean")
    if pred is None:
        return spec, None
    if not isinstance(pred, dict) or pred.get("type") != "content":
        raise ValueError('prediction must be an object of type "content"')
    content = pred.get("content")
    if isinstance(content, list) and content and all(
            isinstance(p, dict) and p.get("type") == "text" and isinstance(p.get("text"), str) for p in content):
        content = "".join(p["text"] for p in content)
    if not isinstance(content, str) or not content:
        raise ValueError('prediction.content must be a non-empty string or a list of {"type": "text", "text": ...} parts')
    ids = [int(t) for t in tokenizer.encode(content, add_bos=False, parse_special=False)]
    return (True if spec is None else spec), ids


def prediction_usage(res) -> dict:
    """usage.completion_tokens_details: the draft tokens the engine verified, accepted and not (0 / 0 when
    nothing was drafted -- speculation off, a tier whose engine cannot speculate, or no draft found)"""
    acc = int(getattr(res, "accepted_draft_tokens", 0) or 0)
    return {"accepted_prediction_tokens": acc,
            "rejected_prediction_tokens": max(int(getattr(res, "draft_tokens", 0) or 0) - acc, 0)}


def logprobs_content(tokenizer, entries) -> list:
    """GenResult.logprobs as OpenAI's choices[0].logprobs.content: per token its piece (`bytes`: the
    piece's raw bytes, `token`: their UTF-8 decoding, U+FFFD where the piece alone is not valid UTF-8),
    its logprob and the alternatives, best first"""
    def item(tid, lp):
        raw = tokenizer.token_bytes(int(tid))
        finite = lp == lp and lp not in (float("inf"), float("-inf"))
        return {"token": raw.decode("utf-8", errors="replace"), "logprob": float(lp) if finite else LOGPROB_NEG_INF,
                "bytes": list(raw)}

    out = []
    for tid, lp, top in entries or []:
        it = item(tid, lp)
        it["top_logprobs"] = [item(i, x) for i, x in top]
        out.append(it)
    return out


def embedding_inputs(body: dict, tokenizer, max_ctx: int) -> List[List[int]]:
    """The `input` of a /v1/embeddings body as token lists: a string, a list of strings, one tokenised input
    (a list of ints) or a list of them.  Strings get BOS and no chat template.  ValueError: a 400."""
    inp = body.get("input")

    def is_id(v):
        return isinstance(v, int) and not isinstance(v, bool)

    if isinstance(inp, str):
        items = [inp]
    elif isinstance(inp, list) and inp and all(is_id(v) for v in inp):
        items = [inp]
    elif isinstance(inp, list) and inp and all(isinstance(v, str) or (isinstance(v, list) and all(is_id(t) for t in v))
                                                for v in inp):
        items = inp
    else:
        raise ValueError("input must be a non-empty string, a list of strings, a list of token ids or a list of "
                         "token-id lists")
    if len(items) > MAX_EMBED_INPUTS:
        raise ValueError(f"at most {MAX_EMBED_INPUTS} inputs per request, got {len(items)}")
    out = []
    for i, it in enumerate(items):
        if len(it) == 0:
            raise ValueError(f"input {i} is empty")
        ids = tokenizer.encode(it, add_bos=True, parse_special=False) if isinstance(it, str) else [int(t) for t in it]
        if any(not 0 <= t < tokenizer.vocab_size for t in ids):
            raise ValueError(f"input {i}: token id outside [0, {tokenizer.vocab_size})")
        if len(ids) > max_ctx:
            raise ValueError(f"input {i}: {len(ids)} tokens exceed the context window ({max_ctx})")
        out.append(ids)
    return out


COMPLETION_MAX_TOKENS = 16  # OpenAI's default for /v1/completions


def completion_request(body: dict, tokenizer, scheduler) -> dict:
    """A /v1/completions body, checked: dict(ids, prompt_text, max_tokens, temperature, echo, logprobs (None or
    the number of alternatives), stream, sampling, repeat_last_n).  A string prompt gets BOS and no chat
    template.  ValueError (-> 400) for what this endpoint does not serve."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)

    if not isinstance(body, dict):
        raise ValueError("the body must be a JSON object")
    for k, why in (("best_of", "best_of is not supported"), ("suffix", "suffix is not supported")):
        if body.get(k) is not None:
            raise ValueError(why)
    if body.get("n") not in (None, 1):
        raise ValueError("n > 1 is not supported")
    prompt = body.get("prompt")
    if isinstance(prompt, str):
        if not prompt:
            raise ValueError("prompt is empty")
        ids = tokenizer.encode(prompt, add_bos=True, parse_special=False)
        text = prompt
    elif isinstance(prompt, list) and prompt and all(is_int(t) for t in prompt):
        ids = [int(t) for t in prompt]
        if any(not 0 <= t < tokenizer.vocab_size for t in ids):
            raise ValueError(f"prompt: token id outside [0, {tokenizer.vocab_size})")
        text = tokenizer.decode(ids)
    elif isinstance(prompt, list) and prompt:
        raise ValueError("one prompt per request: a string or a list of token ids (lists of prompts are not supported)")
    else:
        raise ValueError("prompt must be a non-empty string or a non-empty list of token ids")
    max_tokens = body.get("max_tokens")
    max_tokens = COMPLETION_MAX_TOKENS if max_tokens is None else max_tokens
    if not is_int(max_tokens) or max_tokens < 0:
        raise ValueError("max_tokens must be a non-negative integer")
    echo = body.get("echo")
    if echo is not None and not isinstance(echo, bool):
        raise ValueError("echo must be a boolean")
    lp = body.get("logprobs")
    if lp is not None and (not is_int(lp) or not 0 <= lp <= LOGPROB_MAX_TOP):
        raise ValueError(f"logprobs must be null or an integer in 0..{LOGPROB_MAX_TOP}")
    stream = bool(body.get("stream"))
    if stream and lp is not None:
        raise ValueError("logprobs are not available with stream: true")
    if max_tokens == 0 and not (echo and lp is not None):
        raise ValueError("max_tokens: 0 scores the prompt: it needs echo: true and logprobs")
    if len(ids) > scheduler.max_ctx or (max_tokens > 0 and len(ids) >= scheduler.max_ctx):
        raise ValueError(f"prompt of {len(ids)} tokens exceeds the context window ({scheduler.max_ctx})")
    if lp is not None:  # (a tensor-parallel tier: vocab-parallel lm_head)
        if max_tokens > 0 and not getattr(scheduler, "can_logprobs", False):
            raise ValueError("this model's engine cannot report logprobs")
        if echo and not getattr(scheduler, "can_score", False):
            raise ValueError("this model's engine cannot score prompts (single-GPU tiers only)")
    try:
        sampling = sampling_from_body(body)
        temperature = float(body.get("temperature", 1.0) if body.get("temperature") is not None else 1.0)
        rln = body.get("repeat_last_n")
        rln = None if rln is None else int(rln)
    except (TypeError, ValueError) as e:
        raise ValueError(f"bad sampling field: {e}") from None
    speculative, prediction_ids = prediction_from_body(body, tokenizer)
    logit_bias, ignore_eos = bias_from_body(body, scheduler)
    context_shift, n_keep, shift_usage = shift_from_body(body, scheduler)
    return dict(json_schema=schema_from_body(body), context_shift=context_shift, n_keep=n_keep, shift_usage=shift_usage,
                logit_bias=logit_bias, ignore_eos=ignore_eos, ids=ids, prompt_text=text, max_tokens=int(max_tokens), temperature=max(temperature, 0.0),
                echo=bool(echo), logprobs=lp, stream=stream, sampling=sampling, repeat_last_n=rln,
                speculative=speculative, prediction_ids=prediction_ids)


def completion_logprobs(tokenizer, entries) -> dict:
    """OpenAI's text_completion `logprobs` object from (token id, logprob | None, [(alternative id, logprob),
    ...]) entries: tokens, token_logprobs, top_logprobs (one {token text: logprob} dict per token; colliding
    token texts keep the better one) and text_offset (each token's offset in the tokens' concatenation).  An
    entry whose logprob is None (a prompt's first token) reports null for both."""
    def num(lp):
        finite = lp == lp and lp not in (float("inf"), float("-inf"))
        return float(lp) if finite else LOGPROB_NEG_INF

    def piece(tid):
        return tokenizer.token_bytes(int(tid)).decode("utf-8", errors="replace")

    out = {"tokens": [], "token_logprobs": [], "top_logprobs": [], "text_offset": []}
    off = 0
    for tid, lp, top in entries:
        s = piece(tid)
        out["tokens"].append(s)
        out["text_offset"].append(off)
        off += len(s)
        if lp is None:
            out["token_logprobs"].append(None)
            out["top_logprobs"].append(None)
            continue
        out["token_logprobs"].append(num(lp))
        alts: Dict[str, float] = {}
        for i, x in top:
            k, v = piece(i), num(x)
            if k not in alts or v > alts[k]:
                alts[k] = v
        out["top_logprobs"].append(alts)
    return out


async def complete(m, c: dict, on_delta=None, timeout: float = 120.0) -> GenResult:
    """Submit a checked /v1/completions request (completion_request) to the model's scheduler."""
    loop = asyncio.get_running_loop()
    fut = loop.create_future()
    delta_cb = None
    if on_delta is not None:
        def delta_cb(d):
            loop.call_soon_threadsafe(on_delta, d)
    req = GenRequest(prompt_ids=c["ids"], max_tokens=c["max_tokens"], temperature=c["temperature"], on_delta=delta_cb,
                     on_done=lambda res: loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(res)),
                     deadline=time.time() + timeout)
    for k, v in c["sampling"].items():
        setattr(req, k, v)
    if c["repeat_last_n"] is not None:
        req.repeat_last_n = c["repeat_last_n"]
    if c["logprobs"] is not None:
        if c["max_tokens"] > 0:
            req.logprobs, req.top_logprobs = True, int(c["logprobs"])
        if c["echo"]:
            req.prompt_logprobs = int(c["logprobs"])
    req.speculative, req.prediction_ids = c.get("speculative"), c.get("prediction_ids")
    req.logit_bias, req.ignore_eos = c.get("logit_bias"), bool(c.get("ignore_eos"))
    req.context_shift, req.n_keep = bool(c.get("context_shift")), int(c.get("n_keep", -1))
    req.json_schema = c.get("json_schema")
    m.scheduler.submit(req)
    try:
        return await asyncio.wait_for(fut, timeout + 5)
    except asyncio.TimeoutError:
        req.cancelled = True
        raise


async def embed(m, inputs: List[List[int]], pooling: str, timeout: float = 120.0) -> List[GenResult]:
    """Submit the inputs to the model's scheduler together; their results in input order."""
    loop = asyncio.get_running_loop()
    futs, reqs = [], []
    for ids in inputs:
        fut = loop.create_future()
        reqs.append(GenRequest(prompt_ids=ids, embed=pooling, deadline=time.time() + timeout,
                               on_done=lambda res, fut=fut: loop.call_soon_threadsafe(
                                   lambda: fut.done() or fut.set_result(res))))
        futs.append(fut)
    for r in reqs:
        m.scheduler.submit(r)
    try:
        return list(await asyncio.wait_for(asyncio.gather(*futs), timeout + 5))
    except asyncio.TimeoutError:
        for r in reqs:
            r.cancelled = True
        raise


async def generate(m, messages, max_tokens: int, temperature: float, json_mode: bool, on_delta=None,
                   timeout: float = 120.0, seed: int = 0, sampling: Optional[dict] = None,
                   top_logprobs: Optional[int] = None, speculative: Optional[bool] = None,
                   prediction_ids: Optional[List[int]] = None, logit_bias: Optional[Dict[int, float]] = None,
                   ignore_eos: bool = False, context_shift: bool = False, n_keep: int = -1,
                   schema: Optional[dict] = None) -> GenResult:
    """sampling: further GenRequest fields by name (top_p, top_k, seed, min_p, the penalties);
    top_logprobs: None, or per-token logprobs with that many alternatives (GenResult.logprobs);
    speculative / prediction_ids: GenRequest's (prediction_from_body); logit_bias / ignore_eos:
    GenRequest's (bias_from_body); context_shift / n_keep: GenRequest's (shift_from_body); schema:
    GenRequest.json_schema (schema_from_body), in place of json_mode"""
    loop = asyncio.get_running_loop()
    fut = loop.create_future()
    prompt = m.template.render(messages, add_generation_prompt=True)
    ids = m.tokenizer.encode(prompt)

    def done(res):
        loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(res))

    delta_cb = None
    if on_delta is not None:
        def delta_cb(d):
            loop.call_soon_threadsafe(on_delta, d)
    req = GenRequest(prompt_ids=ids, max_tokens=max_tokens, temperature=temperature, json_mode=json_mode,
                     min_tokens=_json_min_tokens(max_tokens) if json_mode else 0, seed=seed, on_delta=delta_cb, on_done=done, deadline=time.time() + timeout)
    for k, v in (sampling or {}).items():
        if k not in SAMPLING_FIELDS:
            raise ValueError(f"unknown sampling field {k!r}")
        setattr(req, k, v)
    if top_logprobs is not None:
        req.logprobs, req.top_logprobs = True, int(top_logprobs)
    req.speculative, req.prediction_ids = speculative, prediction_ids
    req.logit_bias, req.ignore_eos = logit_bias, ignore_eos
    req.context_shift, req.n_keep = context_shift, n_keep
    if schema is not None:
        req.json_schema, req.json_mode, req.min_tokens = schema, False, 0
    m.scheduler.submit(req)
    try:
        return await asyncio.wait_for(fut, timeout + 5)
    except asyncio.TimeoutError:
        req.cancelled = True
        raise


class AIRuntimeService:
    def __init__(self, manager: ModelManager, http: bool = True):
        self.mgr = manager
        self.http = http
        self._http_runners: Dict[str, object] = {}
        manager.unload_hooks.append(self._drop_http)

    async def _drop_http(self, name: str):
        runner = self._http_runners.pop(name, None)
        if runner is not None:
            await runner.cleanup()

    async def _route(self, request):
        """Resolve (loading an on-demand tier when needed) and expose a freshly loaded model's
        OpenAI-compatible endpoint."""
        m = await self.mgr.resolve_async(request.model, request.intelligence_level)
        if self.http and m.name not in self._http_runners:
            await self.start_http(m)
        return m

    async def _abort(self, context, e: RoutingError):
        await context.abort(getattr(grpc.StatusCode, e.code), str(e))

    @staticmethod
    def _status(m) -> object:
        return pb.runtime.ModelStatus(model_name=m.name, status=m.status_string(), port=m.port, loaded_at=m.loaded_at,
                                      last_used=m.last_used, request_count=m.request_count)

    async def LoadModel(self, request, context):
        name = request.model_name or (request.model_path.split("/")[-1].rsplit(".", 1)[0] if request.model_path else "")
        if not name or not request.model_path:
            await context.abort(grpc.StatusCode.INVALID_ARGUMENT, "model_name and model_path are required")
        m = await self.mgr.load_model(name, request.model_path, request.context_length, request.port)
        if m.status == "ready" and self.http:
            await self.start_http(m)
        return self._status(m)

    async def UnloadModel(self, request, context):
        ok = await self.mgr.unload_model(request.model_name)
        return pb.common.Status(success=ok, message="unloaded" if ok else f"model {request.model_name} not found")

    async def ListModels(self, request, context):
        return pb.runtime.ModelList(models=[self._status(m) for m in self.mgr.list_models()])

    def _engine_failed(self, m) -> bool:
        """The model's engine (not the request) failed: take it out of routing."""
        sch = m.scheduler
        if sch is not None and sch.failed:
            self.mgr.fail_model(m, f"engine failure: {sch.failed}")
            return True
        return m.status != "ready"

    async def Infer(self, request, context):
        try:
            m = await self._route(request)
        except RoutingError as e:
            await self._abort(context, e)
        temperature, max_tokens = _gen_params(request.temperature, request.max_tokens)
        t0 = time.time()
        msgs = build_messages(request.prompt, request.system_prompt)
        res = await generate(m, msgs, max_tokens, temperature, json_mode=True)
        if res.finish_reason == "error" and self._engine_failed(m):
            # e.g. a TP rank timed out: the tier is torn down and the request re-routed once to
            # the next ready model of its level (strategic -> tactical ...)
            log.warning("model %s failed (%s); re-routing the request", m.name, res.error)
            try:
                m = await self._route(request)
            except RoutingError as e:
                await self._abort(context, e)
            res = await generate(m, msgs, max_tokens, temperature, json_mode=True)
        if res.finish_reason == "error":
            await context.abort(grpc.StatusCode.INTERNAL, f"inference failed: {res.error}")
        return pb.runtime.InferResponse(text=res.text, tokens_used=res.prompt_tokens + res.completion_tokens,
                                        latency_ms=int((time.time() - t0) * 1000), model_used=m.name)

    async def StreamInfer(self, request, context):
        try:
            m = await self._route(request)
        except RoutingError as e:
            await self._abort(context, e)
            return
        temperature, max_tokens = _gen_params(request.temperature, request.max_tokens)
        q: asyncio.Queue = asyncio.Queue()
        task = asyncio.ensure_future(generate(m, build_messages(request.prompt, request.system_prompt), max_tokens,
                                              temperature, json_mode=False, on_delta=q.put_nowait))
        task.add_done_callback(lambda _t: q.put_nowait(None))
        while True:
            d = await q.get()
            if d is None:
                break
            yield pb.runtime.InferChunk(text=d, done=False)
        res = task.result()
        if res.finish_reason == "error":
            await context.abort(grpc.StatusCode.INTERNAL, res.error)
        yield pb.runtime.InferChunk(text="", done=True)

    async def HealthCheck(self, request, context):
        models = self.mgr.list_models()
        ready = sum(1 for m in models if m.status == "ready")
        h = pb.common.HealthStatus(healthy=True, service="aios-runtime",
                                   message=f"{ready}/{len(models)} models ready",
                                   uptime_seconds=int(time.time() - self.mgr.started))
        for k, v in self.mgr.health().items():
            h.details[k] = v
        try:  # amdgpu RAS / thermal verdict (uncorrectable HBM ECC or xGMI errors -> unhealthy)
            from ..utils import sysinfo

            gh = sysinfo.gpu_health()
            h.details["gpu_ecc_uncorrectable"] = str(gh["ecc_ue_total"])
            h.details["gpu_ecc_correctable"] = str(gh["ecc_ce_total"])
            if not gh["healthy"]:
                h.details["gpu_problems"] = json.dumps(gh["problems"])
                h.message += f"; GPU problems on {len(gh['problems'])} counter(s)"
        except Exception:  # pragma: no cover - no GPU sysfs
            pass
        return h

    # ------------------------------------------------------------------ HTTP (OpenAI-compatible)
    async def start_http(self, m, host: str = "127.0.0.1"):
        from aiohttp import web

        if m.name in self._http_runners:
            return
        app = web.Application()
        app["model"] = m
        app.router.add_get("/health", self._http_health)
        app.router.add_post("/v1/chat/completions", self._http_chat)
        app.router.add_get("/v1/models", self._http_models)
        app.router.add_post("/v1/embeddings", self._http_embeddings)
        app.router.add_post("/v1/completions", self._http_completions)
        app.router.add_get("/slots", self._http_slots)
        app.router.add_post("/slots/{id}", self._http_slot_action)
        runner = web.AppRunner(app, access_log=None)
        await runner.setup()
        try:
            await web.TCPSite(runner, host, m.port).start()
            self._http_runners[m.name] = runner
        except OSError as e:
            log.warning("HTTP endpoint for %s on :%d unavailable: %s", m.name, m.port, e)
            await runner.cleanup()

    async def _http_health(self, request):
        from aiohttp import web

        m = request.app["model"]
        return web.json_response({"status": "ok" if m.status == "ready" else m.status})

    async def _http_models(self, request):
        from aiohttp import web

        m = request.app["model"]
        return web.json_response({"object": "list", "data": [{"id": m.name, "object": "model"}]})

    async def _http_chat(self, request):
        from aiohttp import web

        m = request.app["model"]
        body = await request.json()
        messages = body.get("messages") or []
        max_tokens = int(body.get("max_tokens") or 512)
        temperature = float(body.get("temperature", 0.7))
        try:
            schema = await asyncio.get_running_loop().run_in_executor(None, schema_from_body, body)
        except ValueError as e:
            return web.json_response({"error": {"message": str(e), "type": "invalid_request_error"}}, status=400)
        json_mode = (body.get("response_format") or {}).get("type") == "json_object"
        try:
            sampling = sampling_from_body(body)
        except (TypeError, ValueError) as e:
            return web.json_response({"error": {"message": f"bad sampling field: {e}", "type": "invalid_request_error"}},
                                     status=400)
        try:
            top_logprobs = logprobs_from_body(body, m.scheduler)
            speculative, prediction_ids = prediction_from_body(body, m.tokenizer)
            logit_bias, ignore_eos = bias_from_body(body, m.scheduler)
            context_shift, n_keep, shift_usage = shift_from_body(body, m.scheduler)
        except ValueError as e:
            return web.json_response({"error": {"message": str(e), "type": "invalid_request_error"}}, status=400)
        created = int(time.time())
        rid = f"chatcmpl-{created}{id(request) & 0xffff:04x}"
        if body.get("stream"):
            resp = web.StreamResponse(headers={"Content-Type": "text/event-stream"})
            await resp.prepare(request)
            q: asyncio.Queue = asyncio.Queue()
            task = asyncio.ensure_future(generate(m, messages, max_tokens, temperature, json_mode, on_delta=q.put_nowait,
                                                  sampling=sampling, speculative=speculative,
                                                  prediction_ids=prediction_ids, logit_bias=logit_bias,
                                                  ignore_eos=ignore_eos, context_shift=context_shift, n_keep=n_keep,
                                                  schema=schema))
            task.add_done_callback(lambda _t: q.put_nowait(None))
            while True:
                d = await q.get()
                if d is None:
                    break
                chunk = {"id": rid, "object": "chat.completion.chunk", "created": created, "model": m.name,
                         "choices": [{"index": 0, "delta": {"content": d}, "finish_reason": None}]}
                await resp.write(f"data: {json.dumps(chunk)}\n\n".encode())
            res = task.result()
            end = {"id": rid, "object": "chat.completion.chunk", "created": created, "model": m.name,
                   "choices": [{"index": 0, "delta": {}, "finish_reason": "stop" if res.finish_reason != "length" else "length"}]}
            await resp.write(f"data: {json.dumps(end)}\n\ndata: [DONE]\n\n".encode())
            await resp.write_eof()
            return resp
        res = await generate(m, messages, max_tokens, temperature, json_mode, sampling=sampling,
                             top_logprobs=top_logprobs, speculative=speculative, prediction_ids=prediction_ids,
                             logit_bias=logit_bias, ignore_eos=ignore_eos, context_shift=context_shift, n_keep=n_keep,
                             schema=schema)
        choice = {"index": 0, "message": {"role": "assistant", "content": res.text},
                  "finish_reason": "length" if res.finish_reason == "length" else "stop"}
        if top_logprobs is not None:  # (bodies of requests that did not ask stay as they were)
            choice["logprobs"] = {"content": logprobs_content(m.tokenizer, res.logprobs)}
        usage = {"prompt_tokens": res.prompt_tokens, "completion_tokens": res.completion_tokens,
                 "total_tokens": res.prompt_tokens + res.completion_tokens,
                 "completion_tokens_details": prediction_usage(res)}
        if shift_usage:  # (a body that names neither field on a tier that does not shift stays as it was)
            usage["context_shifts"] = int(res.context_shifts)
        return web.json_response({
            "id": rid, "object": "chat.completion", "created": created, "model": m.name,
            "choices": [choice],
            "usage": usage,
            "timings": {"ttft_ms": res.ttft_ms, "latency_ms": res.latency_ms,
                        "cached_prompt_tokens": res.cached_prompt_tokens},
        })

    async def _http_completions(self, request):
        """OpenAI's /v1/completions: a raw prompt (a string, which gets BOS and no chat template, or one token
        list), optionally `echo` and `logprobs` (an integer: alternatives per token, 0..20) -- with both the
        prompt's tokens are scored too (runtime/scoring.py: the rule), and max_tokens: 0 only scores."""
        from aiohttp import web

        m = request.app["model"]

        def bad(msg):
            return web.json_response({"error": {"message": msg, "type": "invalid_request_error"}}, status=400)

        try:
            body = await request.json()
        except ValueError:
            return bad("the body is not JSON")
        try:
            if isinstance(body, dict):  # (compiles a schema off the loop; completion_request then finds it cached)
                await asyncio.get_running_loop().run_in_executor(None, schema_from_body, body)
            c = completion_request(body, m.tokenizer, m.scheduler)
        except ValueError as e:
            return bad(str(e))
        created = int(time.time())
        rid = f"cmpl-{created}{id(request) & 0xffff:04x}"

        def chunk(text, finish):
            return {"id": rid, "object": "text_completion", "created": created, "model": m.name,
                    "choices": [{"text": text, "index": 0, "logprobs": None, "finish_reason": finish}]}

        if c["stream"]:
            resp = web.StreamResponse(headers={"Content-Type": "text/event-stream"})
            await resp.prepare(request)
            q: asyncio.Queue = asyncio.Queue()
            task = asyncio.ensure_future(complete(m, c, on_delta=q.put_nowait))
            task.add_done_callback(lambda _t: q.put_nowait(None))
            if c["echo"]:
                await resp.write(f"data: {json.dumps(chunk(c['prompt_text'], None))}\n\n".encode())
            while True:
                d = await q.get()
                if d is None:
                    break
                await resp.write(f"data: {json.dumps(chunk(d, None))}\n\n".encode())
            res = task.result()
            end = chunk("", "length" if res.finish_reason == "length" else "stop")
            await resp.write(f"data: {json.dumps(end)}\n\ndata: [DONE]\n\n".encode())
            await resp.write_eof()
            return resp
        res = await complete(m, c)
        if res.finish_reason == "error":
            return web.json_response({"error": {"message": res.error or "inference failed", "type": "server_error"}},
                                     status=500)
        lp = None
        if c["logprobs"] is not None:
            entries = [(t, x, top) for t, x, _rank, top in (res.prompt_logprobs or [])] if c["echo"] else []
            entries += list(res.logprobs or [])
            lp = completion_logprobs(m.tokenizer, entries)
        choice = {"text": (c["prompt_text"] if c["echo"] else "") + res.text, "index": 0, "logprobs": lp,
                  "finish_reason": "length" if res.finish_reason == "length" else "stop"}
        usage = {"prompt_tokens": res.prompt_tokens, "completion_tokens": res.completion_tokens,
                 "total_tokens": res.prompt_tokens + res.completion_tokens}
        # (the usage of a body that names neither field on a tier that does not speculate stays as it was)
        if c["speculative"] is not None or getattr(m.scheduler, "spec", {}).get("mode", "off") != "off":
            usage["completion_tokens_details"] = prediction_usage(res)
        if c["shift_usage"]:  # (likewise)
            usage["context_shifts"] = int(res.context_shifts)
        return web.json_response({
            "id": rid, "object": "text_completion", "created": created, "model": m.name, "choices": [choice],
            "usage": usage,
        })

    async def _http_embeddings(self, request):
        """OpenAI's /v1/embeddings (runtime/embedding.py: the rule).  `pooling`: "mean" | "last", an extension;
        its default is the model's (ModelConfig.pooling).  `dimensions` is refused."""
        import base64

        from aiohttp import web

        m = request.app["model"]

        def bad(msg):
            return web.json_response({"error": {"message": msg, "type": "invalid_request_error"}}, status=400)

        try:
            body = await request.json()
        except ValueError:
            return bad("the body is not JSON")
        if not isinstance(body, dict):
            return bad("the body must be a JSON object")
        if body.get("dimensions") is not None:
            return bad("dimensions is not supported: this model is not trained for truncated embeddings")
        fmt = body.get("encoding_format", "float")
        if fmt not in ("float", "base64"):
            return bad('encoding_format must be "float" or "base64"')
        pooling = body.get("pooling", getattr(getattr(m, "config", None), "pooling", "mean"))
        if pooling not in ("mean", "last"):
            return bad('pooling must be "mean" or "last"')
        if not getattr(m.scheduler, "can_embed", False):  # (a tensor-parallel tier)
            return bad("this model's engine cannot compute embeddings (single-GPU tiers only)")
        try:
            inputs = embedding_inputs(body, m.tokenizer, m.scheduler.max_ctx)
        except ValueError as e:
            return bad(str(e))
        results = await embed(m, inputs, pooling)
        for res in results:
            if res.finish_reason != "embedding":
                return web.json_response({"error": {"message": res.error or res.finish_reason, "type": "server_error"}},
                                         status=500)
        data = []
        for i, res in enumerate(results):
            v = np.asarray(res.embedding, "<f4")
            data.append({"object": "embedding", "index": i,
                         "embedding": base64.b64encode(v.tobytes()).decode() if fmt == "base64" else v.tolist()})
        n = sum(len(ids) for ids in inputs)
        return web.json_response({"object": "list", "data": data, "model": m.name,
                                  "usage": {"prompt_tokens": n, "total_tokens": n}})

    async def _http_slots(self, request):
        """llama-server's GET /slots: one entry per slot -- id, is_processing, n_cached (the tokens of its cache
        record, what a save would write)."""
        from aiohttp import web

        m = request.app["model"]
        return web.json_response(await asyncio.to_thread(m.scheduler.slots))

    async def _http_slot_action(self, request):
        """llama-server's POST /slots/{id}?action=save|restore|erase with body {"filename": "..."} (runtime/
        kv_snapshot.py: the file; Scheduler.save_slot / restore_slot / erase_slot).  Files live in the tier's
        slot_save_path and nowhere else; without one the actions answer 501, as llama-server does without
        --slot-save-path."""
        from aiohttp import web

        from . import kv_snapshot
        from .scheduler import SlotBusy, SlotsUnsupported

        m = request.app["model"]

        def err(status, msg, kind="invalid_request_error"):
            return web.json_response({"error": {"message": msg, "type": kind, "code": status}}, status=status)

        action = request.query.get("action", "")
        if action not in ("save", "restore", "erase"):
            return err(400, f"action: must be save, restore or erase, not {action!r}")
        directory = getattr(m, "slot_save_path", "")
        if not directory:
            return err(501, "this server does not support slot actions: no slot_save_path is configured",
                       "not_supported_error")
        if not getattr(m.scheduler, "can_snapshot", False):
            return err(400, "slots: single-GPU engines only")
        try:
            slot = int(request.match_info["id"])
        except ValueError:
            return err(400, f"unknown slot {request.match_info['id']!r}")
        sch = m.scheduler
        t0 = time.perf_counter()
        try:
            if action == "erase":
                got = await asyncio.to_thread(sch.erase_slot, slot)
                return web.json_response({"id_slot": slot, "n_erased": got["n_erased"]})
            try:
                body = await request.json()
            except ValueError:
                return err(400, "the body is not JSON")
            if not isinstance(body, dict):
                return err(400, "the body must be a JSON object")
            filename = body.get("filename")
            path = kv_snapshot.snapshot_path(directory, filename)
            if action == "save":
                try:
                    got = await asyncio.to_thread(sch.save_slot, slot, path)
                except kv_snapshot.SnapshotError as e:  # (a slot with nothing cached)
                    return err(400, str(e))
                return web.json_response({"id_slot": slot, "filename": filename, "n_saved": got["n_saved"],
                                          "n_written": got["n_written"],
                                          "timings": {"save_ms": (time.perf_counter() - t0) * 1e3}})
            got = await asyncio.to_thread(sch.restore_slot, slot, path)
            return web.json_response({"id_slot": slot, "filename": filename, "n_restored": got["n_restored"],
                                      "n_read": got["n_read"],
                                      "timings": {"restore_ms": (time.perf_counter() - t0) * 1e3}})
        except SlotBusy as e:
            return err(409, str(e))
        except SlotsUnsupported as e:
            return err(400, str(e))
        except FileNotFoundError:
            return err(404, f"filename: no snapshot {body.get('filename')!r}", "not_found_error")
        except kv_snapshot.SnapshotError as e:  # the file does not fit this engine, or is damaged: the field is named
            return err(409, f"snapshot mismatch: {e}")
        except ValueError as e:  # an unknown slot, a malformed filename
            return err(400, str(e))
        except Exception as e:  # noqa: BLE001 - e.g. a pool without the blocks the restore needs
            return err(500, f"{type(e).__name__}: {e}", "server_error")

    async def close(self):
        for r in self._http_runners.values():
            await r.cleanup()
        self._http_runners.clear()
        for m in list(self.mgr.list_models()):
            await self.mgr.unload_model(m.name)
