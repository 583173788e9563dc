"""KV snapshot files: one slot's cached positions [0, n) on disk (llama-server's --slot-save-path).

Layout:  MAGIC (8 bytes) | version (u32 LE) | header length (u32 LE) | header (UTF-8 JSON) | payload

The payload is what `Engine.kv_save(slot, n)` returns -- `Engine.kv_read`'s bytes, [layer][K, V][kv_head][token]
[head_dim] in the cache's own element type (csrc/ops.h KvSnapArgs).  The header names the n token ids and
everything the bytes depend on: the cache shape, the KV dtype, the per-layer fp8 K / V scales (as fp32 bit
patterns: codes under other scales are other values, so they are compared bit for bit), the RoPE base and pairing
(cached keys are rotated), the model name with `weight_type_summary()` / `weight_bytes` as a fingerprint of the
weights, and the payload's size and CRC32.

A save writes a temporary file beside the target and renames it.  A restore reads the whole file, checks it, and
compares every header field with the engine before the engine is touched: each refusal is a SnapshotError that
names the field, and changes nothing.
"""
from __future__ import annotations

import json
import os
import struct
import zlib
from typing import List, Tuple

import numpy as np

MAGIC = b"AIOSKVSN"
VERSION = 1
_PREFIX = struct.Struct("<8sII")
MAX_HEADER = 64 << 20

# header fields a restore compares with the engine, in the order they are checked
ENGINE_FIELDS = ("n_layers", "n_kv_heads", "head_dim", "kv_dtype", "kv_scales_bits", "rope_theta", "rope_mode", "model",
                 "weight_types", "weight_bytes")


class SnapshotError(ValueError):
    """A snapshot file that cannot be used; `field` names what is wrong with it ("magic", "version", "truncated",
    "crc32", "header", "tokens", or one of ENGINE_FIELDS)."""

    def __init__(self, field: str, message: str):
        super().__init__(f"{field}: {message}")
        self.field = field


def snapshot_path(directory: str, filename) -> str:
    """The path of snapshot `filename` inside `directory`.  filename must be a bare file name: ValueError naming
    the field for anything else (empty, a path separator, '..', a NUL), so nothing outside the directory is ever
    opened."""
    if not isinstance(filename, str) or not filename:
        raise ValueError("filename: must be a non-empty string")
    if any(c in filename for c in ("\0", "/", "\\", os.sep, "..")) or filename == ".":
        raise ValueError("filename: must be a bare file name (no path separator, '..' or NUL)")
    return os.path.join(directory, filename)


def scales_bits(scales) -> List[int]:
    return [int(v) for v in np.asarray(list(scales), np.float32).view(np.uint32)]


def engine_header(engine, model: str) -> dict:
    """the header fields that describe `engine` (ENGINE_FIELDS)"""
    cfg = engine.config
    fp8 = bool(getattr(engine, "kv_fp8", False))
    wb = engine.weight_bytes
    return {
        "n_layers": int(cfg.n_layers), "n_kv_heads": int(cfg.n_kv_heads), "head_dim": int(cfg.head_dim),
        "kv_dtype": "fp8_e4m3" if fp8 else "bf16",
        "kv_scales_bits": scales_bits(engine.kv_scales) if fp8 else [],
        "rope_theta": float(cfg.rope_theta), "rope_mode": "neox" if cfg.rope_neox else "norm",
        "model": str(model), "weight_types": str(engine.weight_type_summary()),
        "weight_bytes": int(wb() if callable(wb) else wb),
    }


def payload_bytes(header: dict) -> int:
    es = 1 if header["kv_dtype"] == "fp8_e4m3" else 2
    return int(header["n_layers"]) * 2 * int(header["n_kv_heads"]) * int(header["n_tokens"]) * int(header["head_dim"]) * es


def write(path: str, header: dict, payload) -> int:
    """Write header + payload to `path` through a temporary file beside it; returns the file's size."""
    head = dict(header)
    head["version"] = VERSION
    head["payload_bytes"] = len(payload)
    head["payload_crc32"] = zlib.crc32(payload) & 0xFFFFFFFF
    hj = json.dumps(head, separators=(",", ":")).encode()
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(_PREFIX.pack(MAGIC, VERSION, len(hj)))
            f.write(hj)
            f.write(payload)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return _PREFIX.size + len(hj) + len(payload)


def read(path: str) -> Tuple[dict, bytes, int]:
    """(header, payload, file size) of a snapshot file, checked for magic, version, length and CRC.
    FileNotFoundError when there is no such file; SnapshotError otherwise."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        pre = f.read(_PREFIX.size)
        if len(pre) < _PREFIX.size:
            raise SnapshotError("truncated", f"{size} bytes hold no header")
        magic, version, hlen = _PREFIX.unpack(pre)
        if magic != MAGIC:
            raise SnapshotError("magic", "not a KV snapshot file")
        if version != VERSION:
            raise SnapshotError("version", f"file version {version}, this build reads {VERSION}")
        if hlen > MAX_HEADER or _PREFIX.size + hlen > size:
            raise SnapshotError("truncated", f"{size} bytes end inside the header")
        try:
            header = json.loads(f.read(hlen).decode())
            n = int(header["n_tokens"])
            tokens = header["tokens"]
            want, crc = int(header["payload_bytes"]), int(header["payload_crc32"])
            for k in ENGINE_FIELDS:
                header[k]
            shape_bytes = payload_bytes(header)
        except (ValueError, KeyError, TypeError) as e:
            raise SnapshotError("header", f"unreadable ({type(e).__name__}: {e})") from None
        if n < 1 or not isinstance(tokens, list) or len(tokens) != n:
            raise SnapshotError("tokens", f"{len(tokens) if isinstance(tokens, list) else 'no'} token ids for {n} positions")
        if want != shape_bytes:
            raise SnapshotError("header", f"payload_bytes {want} is not the size of its shape ({shape_bytes})")
        have = size - _PREFIX.size - hlen
        if have != want:
            raise SnapshotError("truncated", f"payload of {have} bytes, the header says {want}")
        payload = f.read(want)
    if len(payload) != want:
        raise SnapshotError("truncated", f"payload of {len(payload)} bytes, the header says {want}")
    if zlib.crc32(payload) & 0xFFFFFFFF != crc:
        raise SnapshotError("crc32", "payload checksum mismatch")
    return header, payload, size


def check_engine(header: dict, engine, model: str, max_ctx: int):
    """SnapshotError naming the first header field that differs from the engine (or a token count beyond its
    window)."""
    mine = engine_header(engine, model)
    for k in ENGINE_FIELDS:
        if header[k] != mine[k]:
            raise SnapshotError(k, f"file has {_short(header[k])}, the engine {_short(mine[k])}")
    if int(header["n_tokens"]) > int(max_ctx):
        raise SnapshotError("tokens", f"{header['n_tokens']} positions exceed the context window ({max_ctx})")


def _short(v) -> str:
    s = repr(v)
    return s if len(s) <= 80 else s[:77] + "..."


def save_slot(engine, slot: int, tokens: List[int], path: str, model: str) -> Tuple[int, int]:
    """Save positions [0, len(tokens)) of `slot` to `path`; returns (tokens saved, bytes written)."""
    n = len(tokens)
    if n < 1:
        raise SnapshotError("tokens", "the slot holds no cached tokens")
    header = engine_header(engine, model)
    header["n_tokens"] = n
    header["tokens"] = [int(t) for t in tokens]
    payload = engine.kv_save(int(slot), n)
    return n, write(path, header, payload)


def restore_slot(engine, slot: int, path: str, model: str, max_ctx: int) -> Tuple[List[int], int]:
    """Restore `path` into `slot`; returns (the file's token ids, bytes read).  Nothing changes on a refusal."""
    header, payload, size = read(path)
    check_engine(header, engine, model, max_ctx)
    engine.kv_restore(int(slot), payload, int(header["n_tokens"]))
    return [int(t) for t in header["tokens"]], size
