"""fp8 KV-cache calibration at load (Engine.calibrate_kv_scales).

With `kv_dtype = "fp8_e4m3"` every layer stores K and V as OCP e4m3 codes times a per-layer scale.
At scale 1.0 e4m3 loses mantissa bits below 2^-6, flushes to zero below 2^-9 and saturates at 448,
and a checkpoint's post-RoPE keys or its values can leave that window layer by layer.  So the loader
runs one short prefill with the KV writers' observer on, takes per layer the largest |K| and |V|
over the heads, and installs scale = amax x 2 / 448 (one e4m3 binade of headroom for tokens the
prompt did not contain).

The scales are per layer, static and derived from ONE prompt.  Per-head and per-token scales are not
built; `engine.kv_amax` (n_layers x 2 x n_kv_heads) shows how far the heads of a layer differ.
"""
from __future__ import annotations

import logging
from typing import Callable, List, Optional, Sequence, Union

log = logging.getLogger("aios.runtime.kv_calibration")

KV_CALIBRATE_MODES = ("auto", "off")
AUTO_MAX_TOKENS = 256

# The "auto" prompt: the shape of the requests this runtime serves -- a system preamble, an excerpt
# of a JSON tool catalogue and a goal to plan for.
CALIBRATION_PROMPT = """\
You are the planning agent of an autonomous operating system node. You receive a goal, break it \
into steps, pick one tool per step from the catalogue below and answer with a single JSON object. \
Never invent a tool. Prefer read-only tools until the cause of a problem is known. Report what you \
did, what you found and what is still open.

Tool catalogue (excerpt):
[
  {"name": "fs.read", "description": "Read a text file", "input": {"path": "string", "max_bytes": "integer"}},
  {"name": "fs.list", "description": "List a directory", "input": {"path": "string", "recursive": "boolean"}},
  {"name": "process.list", "description": "Running processes with cpu and memory use", "input": {"sort_by": "string"}},
  {"name": "service.status", "description": "State of a system service", "input": {"name": "string"}},
  {"name": "service.restart", "description": "Restart a system service", "input": {"name": "string", "reason": "string"}},
  {"name": "monitor.disk", "description": "Disk usage per mount point", "input": {}},
  {"name": "net.check", "description": "Check that a host and port answer", "input": {"host": "string", "port": "integer"}},
  {"name": "log.search", "description": "Search the system logs", "input": {"pattern": "string", "since_minutes": "integer"}},
  {"name": "package.install", "description": "Install a package", "input": {"name": "string", "version": "string"}},
  {"name": "security.scan", "description": "Scan open ports and file permissions", "input": {"scope": "string"}}
]

Goal: the health report shows the disk of the data partition at 91 percent and the log service \
restarting every few minutes. Find out which process writes the most data, check whether the log \
service fails because the disk is full, free space without deleting anything younger than seven \
days, restart the service once and confirm that its status is healthy.

Answer format: {"reasoning": "...", "steps": [{"tool": "...", "input": {...}, "why": "..."}], \
"tools_needed": ["..."], "done": false}
"""


def normalize_mode(kv_calibrate) -> Union[str, List[int]]:
    """None / "off" -> "off"; "auto" -> "auto"; a sequence of token ids -> that list."""
    if kv_calibrate is None:
        return "off"
    if isinstance(kv_calibrate, str):
        k = kv_calibrate.strip().lower()
        if k not in KV_CALIBRATE_MODES:
            raise ValueError(f"kv_calibrate must be one of {KV_CALIBRATE_MODES} or a list of token ids, "
                             f"not {kv_calibrate!r}")
        return k
    return [int(t) for t in kv_calibrate]


def auto_token_limit(max_ctx: int) -> int:
    return max(1, min(AUTO_MAX_TOKENS, int(max_ctx) // 2))


def auto_tokens(tokenizer, max_ctx: int) -> List[int]:
    """The built-in prompt in the model's own tokenizer, cut to min(256, max_ctx // 2) tokens."""
    ids = [int(t) for t in tokenizer.encode(CALIBRATION_PROMPT)]
    return ids[:auto_token_limit(max_ctx)]


def calibrate(eng, kv_calibrate, tokenizer: Optional[Callable[[], object]] = None,
              headroom: float = 2.0) -> Optional[Sequence[float]]:
    """Calibrate `eng`'s fp8 KV scales as `kv_calibrate` says ("auto": `tokenizer()` supplies the
    model's tokenizer).  Nothing happens -- and nothing is an error -- for "off" / None or a bf16 KV
    cache.  Returns the installed scales, or None when nothing was done."""
    mode = normalize_mode(kv_calibrate)
    if mode == "off" or not getattr(eng, "kv_fp8", 0):
        return None
    if mode == "auto":
        if tokenizer is None:
            raise ValueError('kv_calibrate="auto" needs the model\'s tokenizer')
        mode = auto_tokens(tokenizer(), eng.config.max_ctx)
    if not mode:
        raise ValueError("kv_calibrate: empty calibration prompt")
    scales = eng.calibrate_kv_scales(mode, headroom)
    log.info("fp8 KV calibrated on %d tokens: K scales %.3g..%.3g, V scales %.3g..%.3g", len(mode),
             min(scales[0::2]), max(scales[0::2]), min(scales[1::2]), max(scales[1::2]))
    return scales
