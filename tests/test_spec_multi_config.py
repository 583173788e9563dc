"""The node key spec_multi on its way to the scheduler: ModelTier.spec_multi -> the model spec's specmulti
fragment (only where speculative = "lookup", only when it differs from the default) -> parallel.tp.spec_speculative's
`multi` -> Scheduler.spec["multi"]; and the tensor-parallel proxy hides Engine.spec_decode_multi as it hides
spec_decode, so such a tier takes no multi-sequence steps."""
import pytest

from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.parallel.tp import TPEngine, spec_speculative
from aios_amd.runtime.scheduler import SPEC_DEFAULTS, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer
from aios_amd.utils import config as C
from aios_amd.utils.config import ModelTier


def test_default_and_round_trip():
    dflt = ModelTier().spec_multi
    assert isinstance(dflt, bool) and SPEC_DEFAULTS["multi"] == int(dflt)
    assert ModelTier(speculative="lookup").speculative_frag() == ["spec=lookup"]            # the default is not spelled out
    t = ModelTier(speculative="lookup", spec_multi=not dflt)
    assert t.speculative_frag() == ["spec=lookup", f"specmulti={int(not dflt)}"]
    assert spec_speculative("m.gguf#kv=fp8_e4m3&" + "&".join(t.speculative_frag())) == dict(mode="lookup", multi=int(not dflt))
    # read only where speculation is on: an "off" tier says nothing about it
    assert ModelTier(speculative="off", spec_multi=not dflt).speculative_frag() == []
    assert spec_speculative("m.gguf#spec=lookup&specmulti=1") == dict(mode="lookup", multi=1)
    assert spec_speculative("m.gguf#spec=lookup&specmulti=0") == dict(mode="lookup", multi=0)
    # a malformed or out-of-range fragment keeps the default
    assert spec_speculative("m.gguf#spec=lookup&specmulti=2") == dict(mode="lookup")
    assert spec_speculative("m.gguf#spec=lookup&specmulti=yes") == dict(mode="lookup")


def test_node_config_key(tmp_path):
    p = tmp_path / "node.toml"
    p.write_text('[models.operational]\nspeculative = "lookup"\nspec_multi = false\n'
                 '[models.tactical]\nspeculative = "lookup"\nspec_multi = true\n[models.strategic]\nspec_multi = false\n')
    tiers = C.load(str(p)).models.tiers
    assert (tiers["operational"].spec_multi, tiers["tactical"].spec_multi, tiers["strategic"].spec_multi) == (False, True, False)
    frags = {k: spec_speculative("m.gguf#" + "&".join(t.speculative_frag())) for k, t in tiers.items()}
    assert frags["operational"].get("multi", SPEC_DEFAULTS["multi"]) == 0
    assert frags["tactical"].get("multi", SPEC_DEFAULTS["multi"]) == 1
    assert frags["strategic"] == {}


class _Eng:
    def spec_decode(self, *a):
        raise AssertionError

    def spec_decode_multi(self, *a):
        raise AssertionError


def test_scheduler_setting_and_the_tensor_parallel_proxy():
    t, s, ty = synthetic_vocab(512)
    tok = SpmTokenizer(t, s, ty, 1, 2)
    for spec, want in ((dict(mode="lookup", multi=0), 0), (dict(mode="lookup", multi=1), 1),
                       (dict(mode="lookup"), SPEC_DEFAULTS["multi"])):
        sched = Scheduler(_Eng(), tok, max_batch=8, max_slots=2, max_ctx=64, speculative=spec)
        try:
            assert sched.spec["multi"] == want and sched.can_spec and sched.can_spec_multi
        finally:
            sched.close()
    with pytest.raises(ValueError):
        Scheduler(_Eng(), tok, max_batch=8, max_slots=2, max_ctx=64, speculative=dict(multi=2)).close()
    eng = TPEngine(_Eng(), comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "spec_decode") and not hasattr(eng, "spec_decode_multi")
    sched = Scheduler(eng, tok, max_batch=8, max_slots=2, max_ctx=64, speculative=dict(mode="lookup"))
    try:
        assert not sched.can_spec and not sched.can_spec_multi
    finally:
        sched.close()
