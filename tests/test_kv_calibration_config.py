"""fp8 KV calibration, control plane (no GPU): the tier key kv_calibrate, its way through the model
spec fragment and the model manager to the loader, the built-in prompt, and write_synthetic_gguf's
tensor_scale leaving files written without it byte-identical."""
import hashlib
import inspect

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.utils import config as node_config


def _cfg(tmp_path, body: str):
    p = tmp_path / "config.toml"
    p.write_text(body)
    return node_config.load(str(p), env={})


def test_tier_key_parses_and_defaults_to_auto(tmp_path):
    cfg = _cfg(tmp_path, """
[models.a]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
[models.b]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
kv_calibrate = "off"
[models.c]
file = "synthetic:test-small"
kv_calibrate = "Auto"
[models.d]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
kv_calibrate = "sometimes"
""")
    t = cfg.models.tiers
    assert node_config.ModelTier().kv_calibrate == "auto"
    assert (t["a"].kv_calibrate, t["b"].kv_calibrate, t["c"].kv_calibrate) == ("auto", "off", "auto")
    assert t["d"].kv_calibrate == "auto" and any("models.d.kv_calibrate" in w for w in cfg.warnings)
    assert not any("models.a" in w or "models.b" in w or "models.c" in w for w in cfg.warnings)


def test_spec_fragment_round_trip(tmp_path):
    from aios_amd.parallel.tp import parse_spec, spec_kv_calibrate, spec_kv_dtype

    cfg = _cfg(tmp_path, """
[models.a]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
always_loaded = true
[models.b]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
kv_calibrate = "off"
always_loaded = true
[models.c]
file = "synthetic:test-small"
kv_calibrate = "off"
always_loaded = true
""")
    specs = {n: s for n, s, _ in cfg.model_specs()}
    plan = {p["name"]: p["spec"] for p in cfg.tier_plan()}
    assert specs == plan
    assert specs["a"] == "synthetic:test-small#kv=fp8_e4m3"          # the default adds nothing
    assert specs["b"] == "synthetic:test-small#kv=fp8_e4m3&kvcal=off"  # next to kv=
    assert specs["c"] == "synthetic:test-small"                       # no effect on a bf16 tier
    assert (spec_kv_dtype(specs["a"]), spec_kv_calibrate(specs["a"])) == ("fp8_e4m3", "auto")
    assert (spec_kv_dtype(specs["b"]), spec_kv_calibrate(specs["b"])) == ("fp8_e4m3", "off")
    assert spec_kv_calibrate(specs["c"]) == "auto"
    assert parse_spec(specs["b"]) == ("synthetic:test-small", 1, True)
    assert spec_kv_calibrate("m.gguf#tp=2&kv=fp8_e4m3&kvcal=off&q8=0") == "off"
    with pytest.raises(ValueError):
        spec_kv_calibrate("m.gguf#kv=fp8_e4m3&kvcal=maybe")


class _Stop(Exception):
    pass


@pytest.mark.parametrize("spec,want_dtype,want_cal", [
    ("synthetic:test-small#kv=fp8_e4m3", "fp8_e4m3", "auto"),
    ("synthetic:test-small#kv=fp8_e4m3&kvcal=off", "fp8_e4m3", "off"),
    ("synthetic:test-small", "bf16", "auto"),
    ("FILE#kv=fp8_e4m3", "fp8_e4m3", "auto"),
    ("FILE#kv=fp8_e4m3&kvcal=off", "fp8_e4m3", "off"),
])
def test_model_manager_hands_it_to_the_loader(tmp_path, monkeypatch, spec, want_dtype, want_cal):
    """_load_blocking with stub loaders: both the GGUF and the synthetic branch pass kv_calibrate (and
    the synthetic one the tokenizer "auto" needs)."""
    from aios_amd.runtime import loader, model_manager, native

    f = tmp_path / "m.gguf"
    f.write_bytes(b"x")
    spec = spec.replace("FILE", str(f))
    seen = {}

    def stub(name):
        def fn(*a, **kw):
            seen[name] = kw
            raise _Stop()
        return fn

    monkeypatch.delenv("AIOS_KV_DTYPE", raising=False)
    monkeypatch.delenv("AIOS_RUNTIME_DEVICE", raising=False)
    monkeypatch.setattr(native, "require", lambda: object())
    monkeypatch.setattr(native, "gpu_available", lambda: True)
    monkeypatch.setattr(loader, "load_engine", stub("load_engine"))
    monkeypatch.setattr(loader, "random_engine", stub("random_engine"))
    mm = model_manager.ModelManager()
    m = model_manager.ManagedModel(name="t", path=spec, status="loading", port=0)
    with pytest.raises(_Stop):
        mm._load_blocking(m, 256)
    (name, kw), = seen.items()
    assert name == ("random_engine" if spec.startswith("synthetic:") else "load_engine")
    assert kw["kv_dtype"] == want_dtype and kw["kv_calibrate"] == want_cal
    if name == "random_engine":
        assert kw["tokenizer"] is not None


class _FakeEngine:
    def __init__(self, kv_fp8, max_ctx=256):
        self.kv_fp8 = kv_fp8
        self.config = type("C", (), {"max_ctx": max_ctx})()
        self.calls = []

    def calibrate_kv_scales(self, tokens, headroom):
        self.calls.append((list(tokens), headroom))
        return [0.5, 0.25]


def test_calibrate_modes_and_bf16_ignored():
    from aios_amd.runtime import kv_calibration as kc
    from aios_amd.runtime.tokenizer import SpmTokenizer

    toks, scores, types = synthetic_vocab(1024)
    tok = SpmTokenizer(toks, scores, types, 1, 2)
    for mode in ("auto", "off", None, [1, 2, 3]):  # a bf16 KV cache: ignored, no error
        e = _FakeEngine(0)
        assert kc.calibrate(e, mode, lambda: tok) is None and e.calls == []
    for mode in ("off", None):
        e = _FakeEngine(1)
        assert kc.calibrate(e, mode, lambda: tok) is None and e.calls == []
    e = _FakeEngine(1)
    assert kc.calibrate(e, [1, 7, 9]) == [0.5, 0.25] and e.calls == [([1, 7, 9], 2.0)]
    # "auto": the built-in prompt in the model's tokenizer, cut to min(256, max_ctx // 2)
    full = tok.encode(kc.CALIBRATION_PROMPT)
    assert len(full) > 256 and full[0] == 1
    for ctx, n in ((256, 128), (4096, 256), (64, 32)):
        e = _FakeEngine(1, ctx)
        kc.calibrate(e, "auto", lambda: tok)
        assert e.calls == [(full[:n], 2.0)]
    with pytest.raises(ValueError):
        kc.calibrate(_FakeEngine(1), "sometimes", lambda: tok)
    with pytest.raises(ValueError):
        kc.calibrate(_FakeEngine(1), "auto")  # no tokenizer
    # the prompt is what the runtime serves: a preamble, a JSON tool catalogue, a goal
    assert '"name": "fs.read"' in kc.CALIBRATION_PROMPT and "Goal:" in kc.CALIBRATION_PROMPT


def test_loader_signatures():
    from aios_amd.runtime import loader

    assert inspect.signature(loader.load_engine).parameters["kv_calibrate"].default is None
    assert inspect.signature(loader.random_engine).parameters["kv_calibrate"].default is None


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_tensor_scale_leaves_plain_files_byte_identical(tmp_path):
    """Without tensor_scale (the parent's call) and with tensor_scale=None / {}: the same bytes; a
    multiplier changes its tensor alone, exactly (power of two, BF16) and not the random stream."""
    from aios_amd.gguf.reader import GGUFReader

    cfg = get_preset("test-tiny")
    a = write_synthetic_gguf(str(tmp_path / "a.gguf"), cfg, "Q4_K_M", seed=5)
    b = write_synthetic_gguf(str(tmp_path / "b.gguf"), cfg, "Q4_K_M", seed=5, tensor_scale=None)
    c = write_synthetic_gguf(str(tmp_path / "c.gguf"), cfg, "Q4_K_M", seed=5, tensor_scale={})
    assert _sha(a) == _sha(b) == _sha(c)
    p = write_synthetic_gguf(str(tmp_path / "p.gguf"), cfg, "BF16", seed=5)
    s = write_synthetic_gguf(str(tmp_path / "s.gguf"), cfg, "BF16", seed=5,
                             tensor_scale={"blk.1.attn_k.weight": 2.0 ** -10})
    rp, rs = GGUFReader(p), GGUFReader(s)
    for name in rp.tensors:
        x, y = rp.dequantize(name), rs.dequantize(name)
        if name == "blk.1.attn_k.weight":
            assert np.array_equal(x * np.float32(2.0 ** -10), y) and np.abs(x).max() > 0
        else:
            assert np.array_equal(x, y), name
