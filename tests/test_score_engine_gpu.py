"""Engine.score_prefill on the GPU against the fp32 reference model of the same synthetic GGUF and the float64
scoring oracle (tests/score_oracle.py), plus its call contract.

Bound: for every row, |lp - oracle(ref.forward(prompt)[i], target)| <= 2 x 2e-2 x max(scale, 1), scale =
max |ref logits| over the prompt.  tests/test_engine_gpu.py bounds the engine's logits error by
2e-2 x max(scale, 1), and lp = l[t] - lse carries that error at most twice (lse is 1-Lipschitz in the
max norm).  best_lp = max l - lse is held to the same bound for the same reason.  The fp8-KV engine is
compared with the reference built with the same fp8 K / V rounding, under the same bound.

Prompts: 1, 3 and 4 tokens (the GEMV path), 5 and 41 (the GEMMs), and for the 151,936-token vocabulary one
that spans two lm_head groups of the scoring buffer.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import score_oracle as O
from aios_amd.models.config import get_preset

pytestmark = pytest.mark.gpu

CONFIGS = [("test-tiny", "Q4_K_M", "bf16"), ("test-tiny", "BF16", "bf16"), ("test-qwen3-shape", "Q4_K_M", "bf16"),
           ("test-tiny", "Q4_K_M", "fp8_e4m3")]
LENGTHS = [1, 3, 4, 5, 41]


def prompt(cfg, T, seed=11):
    ids = np.random.default_rng(seed + T).integers(3, cfg.vocab_size, T)
    ids[0] = cfg.bos_id
    return [int(t) for t in ids]


class Setup:
    def __init__(self, name, recipe, kv, tmp):
        from aios_amd.models.reference import ReferenceModel
        from aios_amd.models.synthetic import write_synthetic_gguf

        self.cfg = get_preset(name)
        self.kv = kv
        self.path = write_synthetic_gguf(str(tmp / f"{name}_{recipe}.gguf"), self.cfg, recipe, seed=13)
        self.scales = [0.05 if i % 2 == 0 else 0.02 for i in range(2 * self.cfg.n_layers)]
        self.eng = self.load()
        if kv == "bf16":
            self.ref = ReferenceModel.from_gguf(self.path, kv_bf16=True, act_q8=False)
        else:
            self.ref = ReferenceModel.from_gguf(self.path, kv_fp8=True, kv_scales=self.scales)
        self._want = {}

    def load(self):
        from aios_amd.runtime.loader import load_engine

        eng, _, _ = load_engine(self.path, max_ctx=256, max_slots=3, max_batch=2, act_q8=False, kv_dtype=self.kv)
        if self.kv != "bf16":
            eng.set_kv_scales(self.scales)
        return eng

    def want(self, ids, next_token=-1):
        """the reference's (lp, rank, best, best_lp, bound) for the prompt, computed once and kept"""
        key = (tuple(ids), next_token)
        if key not in self._want:
            rl = self.ref.forward(list(ids)).double().numpy()
            bound = 2 * 2e-2 * max(float(np.abs(rl).max()), 1.0)
            self._want[key] = O.score_rows(rl, list(ids[1:]) + [next_token]) + (bound,)
        return self._want[key]


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda p: "-".join(p))
def S(request, tmp_path_factory):
    return Setup(*request.param, tmp_path_factory.mktemp("score"))


def consistent(name, sc, targets, top_n):
    """what must hold on every row whatever the numerics"""
    T = len(targets)
    for k in ("lp", "best_lp", "rank", "best"):
        assert sc[k].shape == (T,), f"{name}: {k} shape {sc[k].shape}"
    for i, t in enumerate(targets):
        if t < 0:
            assert math.isnan(sc["lp"][i]) and sc["rank"][i] == -1, f"{name}: row {i} without a target"
        else:
            assert np.isfinite(sc["lp"][i]) and sc["rank"][i] >= 0, f"{name}: row {i} not scored"
            assert (sc["rank"][i] == 0) == (sc["best"][i] == t), f"{name}: row {i} rank / best disagree"
            assert sc["best_lp"][i] >= sc["lp"][i], f"{name}: row {i} best_lp below lp"
        assert np.isfinite(sc["best_lp"][i]) and sc["best_lp"][i] <= 0.0
    if top_n > 0:
        assert sc["ids"].shape == sc["lps"].shape == (T, top_n)
        for i in range(T):
            assert sc["ids"][i][0] == sc["best"][i], f"{name}: row {i} first alternative is not best"
            assert sc["lps"][i][0] == sc["best_lp"][i] or abs(sc["lps"][i][0] - sc["best_lp"][i]) < 1e-5
            assert np.all(np.diff(sc["lps"][i]) <= 0), f"{name}: row {i} alternatives not descending"
    else:
        assert "ids" not in sc and "lps" not in sc


def against_reference(name, S, sc, ids, next_token, rows=None):
    """rows: (first, count) of the prompt's rows that sc covers (default all)"""
    lp, _rank, _best, best_lp, bound = S.want(ids, next_token)
    a, n = rows or (0, len(ids))
    worst = 0.0
    for i in range(n):
        if not math.isnan(lp[a + i]):
            worst = max(worst, abs(float(sc["lp"][i]) - lp[a + i]))
        worst = max(worst, abs(float(sc["best_lp"][i]) - best_lp[a + i]))
    print(f"score engine {name}: max |lp - reference| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound, f"{name}: {worst:.3e} above {bound:.3e}"


@pytest.mark.parametrize("T", LENGTHS)
def test_rows_match_the_reference(S, T):
    ids = prompt(S.cfg, T)
    name = f"{S.cfg.name} {S.kv} T={T}"
    sc = S.eng.score_prefill(0, ids, 0, -1, 5, False)
    consistent(name, sc, ids[1:] + [-1], 5)
    against_reference(name, S, sc, ids, -1)
    # the last row with a token: scored; without alternatives: the same values, no ids / lps
    nt = int(ids[0] + 1) % S.cfg.vocab_size
    sc2 = S.eng.score_prefill(0, ids, 0, nt, 0, False)
    consistent(name + " next", sc2, ids[1:] + [nt], 0)
    against_reference(name + " next", S, sc2, ids, nt)


def test_prompt_spanning_two_lm_head_groups(S):
    g = S.eng.score_group_rows()
    if g + 20 > 256:
        # (the small vocabularies' groups hold the whole window: one group is all there is to test)
        assert S.cfg.vocab_size < 100000
        return
    ids = prompt(S.cfg, g + 20)
    name = f"{S.cfg.name} {S.kv} T={len(ids)} (groups of {g})"
    sc = S.eng.score_prefill(1, ids, 0, -1, 5, False)
    consistent(name, sc, ids[1:] + [-1], 5)
    against_reference(name, S, sc, ids, -1)


def test_seam_between_two_calls(S):
    ids = prompt(S.cfg, 41)
    name = f"{S.cfg.name} {S.kv} 20+21"
    a = S.eng.score_prefill(2, ids[:20], 0, ids[20], 5, False)
    b = S.eng.score_prefill(2, ids[20:], 20, -1, 5, False)
    consistent(name + " a", a, ids[1:21], 5)
    consistent(name + " b", b, ids[21:] + [-1], 5)
    assert np.isfinite(a["lp"][19]) and a["rank"][19] >= 0  # the seam row
    against_reference(name + " a", S, a, ids, -1, (0, 20))
    against_reference(name + " b", S, b, ids, -1, (20, 21))


def continue_greedy(eng, T, n=8):
    toks = [int(eng.sample_first(T - 1, 0.0, 0, 1.0, 7))]
    for i in range(n):
        toks.append(int(eng.decode([0], [toks[-1]], [T + i])[0]))
    return toks


@pytest.mark.parametrize("T", [4, 41])
def test_generation_continues_as_after_prefill(S, T):
    ids = prompt(S.cfg, T, seed=3)
    one, two = S.load(), S.load()  # two engines in the same state: the block tables can be compared
    one.score_prefill(0, ids, 0, -1, 3, True)
    got = continue_greedy(one, T)
    two.prefill(0, ids, 0, True)
    want = continue_greedy(two, T)
    assert got == want
    assert list(one.block_table(0)) == list(two.block_table(0))
    assert one.kv_blocks_free == two.kv_blocks_free


_DET_PROC = r"""
import numpy as np
from aios_amd.models.config import get_preset
from aios_amd.runtime.loader import random_engine
cfg = get_preset("test-tiny")
eng = random_engine(cfg, "Q4_K_M", seed=3, max_ctx=256, max_slots=2, max_batch=2)
ids = [cfg.bos_id] + [int(t) for t in np.random.default_rng(5).integers(3, cfg.vocab_size, 40)]
a = eng.score_prefill(0, ids, 0, 9, 5, False)
b = eng.score_prefill(0, ids, 0, 9, 5, False)
assert sorted(a) == sorted(b) == ["best", "best_lp", "ids", "lp", "lps", "rank"]
for k in a:
    assert a[k].tobytes() == b[k].tobytes(), k
assert np.isfinite(a["lp"]).all()
print("identical")
"""


def test_two_calls_give_identical_bytes_without_split_k():
    env = dict(os.environ, AIOS_GEMM_PF_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", _DET_PROC], env=env, capture_output=True, text=True, timeout=240,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "identical"


def test_limits_throw():
    from aios_amd.runtime import native
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-tiny")
    eng = random_engine(cfg, "Q4_K_M", seed=1, max_ctx=64, max_slots=2, max_batch=2)
    ids = prompt(cfg, 6)
    for top_n in (-1, native.require().LOGPROB_MAX_TOP + 1):
        with pytest.raises(RuntimeError, match="top_n"):
            eng.score_prefill(0, ids, 0, -1, top_n, False)
    with pytest.raises(RuntimeError, match="next_token"):
        eng.score_prefill(0, ids, 0, cfg.vocab_size, 0, False)
    with pytest.raises(RuntimeError, match="empty"):
        eng.score_prefill(0, [], 0, -1, 0, False)
    with pytest.raises(RuntimeError, match="context"):
        eng.score_prefill(0, prompt(cfg, eng.config.max_ctx + 1), 0, -1, 0, False)  # (the engine's own window)
    # (nothing above ran a forward: the engine still scores)
    assert eng.score_prefill(0, ids, 0, -1, 0, False)["lp"].shape == (6,)
    # one rank's shard of a tensor-parallel engine (vocab-parallel lm_head): refused before anything runs
    shard = random_engine(get_preset("test-tp8-shape"), "Q4_K_M", seed=1, max_ctx=64, max_slots=2, max_batch=2,
                          tp_rank=0, tp_size=2)
    assert shard.config.tp_size == 2 and shard.config.vocab_parallel == 1
    with pytest.raises(RuntimeError, match="single-GPU"):
        shard.score_prefill(0, ids, 0, -1, 0, False)
