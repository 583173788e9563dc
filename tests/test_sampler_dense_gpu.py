"""The device sampler's filtered path (top-k, top-p, min-p: sample_kernel in csrc/kernels/elementwise.hip) on
dense logits and large vocabularies, against the float64 oracle of its contract (tests/sampler_oracle.py):
nuclei of tens to hundreds of survivors, slices that fill their 256 candidate slots, a merge with more
candidates than its table holds (V > 65536), tied values at a slice's cap, different settings per row in
one launch.  Everything goes through the raw op `_engine.sample` with ldl = 0: every row reads the same
logits row, so 4096 rows (independent RNG streams) cost one row of memory.

What these cases found (MI355X, n = 16384, sampled frequency vs oracle mass) in the kernel whose merge cut the
slices' candidates to its table's first 4096 and whose slices handed out their 256 slots in thread order:
  test_merge_capacity, all three vocabularies, every setting with K = 256 (top_k 0 / 256 / 1000): the best
    token (V - 2) never sampled, the upper slices empty, tokens outside the oracle's support sampled --
    V = 128256, top_p 0.9: rank 1 0.00000 vs 0.08825, slice quartiles 0.626 / 0.374 / 0 / 0 vs 0.326 / 0.192 /
    0.221 / 0.260; V = 262144, top_k 256: rank 1 0 vs 0.12798, quartiles 1 / 0 / 0 / 0 vs 0.413 / 0.191 /
    0.158 / 0.238; V = 69640, min_p 0.05: rank 1 0 vs 0.20192, last quartile 0.197 vs 0.360.
    top_k = 40 and top_k = 64 passed: 64 slices * 64 candidates still fit the table.
  test_large_vocabulary_argmax_equalities, all three vocabularies: top_p = 1e-6 returned token 1234 (the
    second best, in slice 0) in every row.
  test_tie_overflow_keeps_the_values_above_the_ties: 1.0 and 0.5 sampled 0 and 0 times; 256 distinct tokens,
    all of them ties.
The V = 9000 cases, the mixed launch, the few-allowed mask and the re-arm case passed there too.
"""
import math

import numpy as np
import pytest
import torch

import sampler_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def per_row(x, B, dtype):
    return torch.from_numpy(np.resize(np.asarray(x, dtype), B)).cuda()


def device_tokens(E, cases, rows=O.N_ROWS, seeds=O.SEEDS):
    """[len(seeds)][B] tokens of B = rows * len(cases) rows, row b under cases[b % len(cases)], all reading
    one logits row (ldl = 0); pos = arange(B).  min-p and the penalties are passed only if a case has them
    (so the cases without run the kernel instantiation without logit processors)."""
    nc, V = len(cases), cases[0].logits.shape[0]
    B = rows * nc
    assert all(c.logits is cases[0].logits for c in cases)
    logits = torch.from_numpy(np.array(cases[0].logits)).cuda()  # (a copy: the shared input is read-only)
    temp = per_row([c.T for c in cases], B, np.float32)
    tk = per_row([c.top_k for c in cases], B, np.int32)
    tp = per_row([c.top_p for c in cases], B, np.float32)
    pos = torch.arange(B, dtype=torch.int32, device="cuda")
    tok = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    keep = []  # (device buffers stay alive over the launches)
    kw, mask = {}, 0
    if any(c.min_p > 0 for c in cases):
        keep.append(per_row([c.min_p for c in cases], B, np.float32))
        kw["min_p"] = keep[-1].data_ptr()
    if any(c.window for c in cases):
        stride = max(len(c.window or []) for c in cases)
        w = np.full((nc, stride), -1, np.int32)
        for i, c in enumerate(cases):
            w[i, :len(c.window or [])] = c.window or []
        keep += [torch.from_numpy(np.ascontiguousarray(np.resize(w, (B, stride)))).cuda(),
                 per_row([c.repeat for c in cases], B, np.float32), per_row([c.presence for c in cases], B, np.float32),
                 per_row([c.frequency for c in cases], B, np.float32)]
        kw.update(pen_tokens=keep[-4].data_ptr(), pen_stride=stride, repeat_penalty=keep[-3].data_ptr(),
                  presence_penalty=keep[-2].data_ptr(), frequency_penalty=keep[-1].data_ptr())
    if any(c.mask is not None for c in cases):
        assert nc == 1
        keep.append(torch.from_numpy(np.tile(np.frombuffer(cases[0].mask, np.uint8), (B, 1))).cuda())
        mask = keep[-1].data_ptr()
    out = []
    for seed in seeds:
        tok.fill_(-1)
        E.sample(logits.data_ptr(), 0, B, V, temp.data_ptr(), tk.data_ptr(), seed, tok.data_ptr(), pos.data_ptr(), mask,
                 stream(), tp.data_ptr(), **kw)
        torch.cuda.synchronize()
        out.append(tok.cpu().numpy().copy())
    return np.stack(out)


def check_case(E, c):
    assert O.ambiguous_of(c) == set()  # (a condition on the input, before the device is touched)
    p = O.oracle_of(c)
    t = device_tokens(E, [c])
    assert t.min() >= 0 and t.max() < p.shape[0]
    O.check_bins(np.bincount(t.reshape(-1), minlength=p.shape[0]), p, t.size, c.name)
    return t


@pytest.mark.parametrize("i", range(18), ids=[c.name for c in O.dense_cases()])
def test_dense(E, i):
    """V = 9000, three temperatures x six settings; top_k = 1000 behaves as 256 (the documented clamp)"""
    check_case(E, O.dense_cases()[i])


def test_dense_clamp_is_exact(E):
    a, b = O.dense_cases()[8], O.dense_cases()[9]
    assert (a.top_k, b.top_k) == (256, 1000)
    assert np.array_equal(device_tokens(E, [a], seeds=O.SEEDS[:1]), device_tokens(E, [b], seeds=O.SEEDS[:1]))


def test_dense_masked_penalised(E):
    """every second token banned, the top five of the rest in the penalty window"""
    c = O.masked_penalised_case()
    t = check_case(E, c)
    assert (t % 2 == 0).all()


@pytest.mark.parametrize("setting", range(6), ids=[f"k{k}-p{p}-m{m}" for k, p, m in O.SETTINGS])
@pytest.mark.parametrize("V", O.V_CAPACITY)
def test_merge_capacity(E, V, setting):
    """more than 16 slices: the slices publish more candidates than the merge's table holds.  The best token
    sits in the last slice, the second best in the first."""
    check_case(E, O.capacity_cases(V)[setting])


@pytest.mark.parametrize("V", O.V_CAPACITY)
def test_large_vocabulary_argmax_equalities(E, V):
    """top_k = 1, top_p = 1e-6 and min_p = 1.0 each leave the argmax alone -- no statistics"""
    x = O.capacity_logits(V)
    for k, p, m in [(1, 1.0, 0.0), (0, 1e-6, 0.0), (0, 1.0, 1.0)]:
        t = device_tokens(E, [O.Case("argmax", x, 0.8, k, p, m)], rows=512, seeds=O.SEEDS[:1])
        assert (t == V - 2).all(), (k, p, m, np.unique(t)[:8])


def test_tie_overflow_keeps_the_values_above_the_ties(E):
    """top_k = 3 over 1.0, 0.5 and 400 tokens at exactly 0.0 in one slice; the two planted tokens sit at the
    slice's last thread positions, 256 ties come before them in slot order.  A token strictly above the K-th
    value is never displaced by tokens tied at it (ops.h); how many of the ties appear is not asserted."""
    c = O.tie_case()
    t = device_tokens(E, [c]).reshape(-1)
    n1, n05 = int((t == O.TIE_HI).sum()), int((t == O.TIE_MID).sum())
    print(f"tie overflow: 1.0 sampled {n1}, 0.5 sampled {n05}, distinct tokens {np.unique(t).size}")
    assert t.min() >= 0 and (c.logits[t] >= 0.0).all()
    assert n1 > 0 and n05 > 0
    r = math.exp(0.5 / 0.8)
    q, n2 = r / (1 + r), n1 + n05
    assert abs(n1 / n2 - q) <= 5 * math.sqrt(q * (1 - q) / n2), (n1, n05, q)


def test_mixed_rows_in_one_launch(E):
    """row b uses setting b % 6: greedy, temperature, top-k, top-p, min-p, all three with penalties"""
    cases = O.mixed_cases()
    for c in cases:
        assert O.ambiguous_of(c) == set()
    t = device_tokens(E, cases, rows=1024)
    V = cases[0].logits.shape[0]
    assert t.min() >= 0 and t.max() < V
    assert (t[:, 0::6] == int(np.argmax(cases[0].logits))).all()
    for i, c in enumerate(cases[1:], 1):
        ti = t[:, i::6]
        assert ti.size == 4096
        O.check_bins(np.bincount(ti.reshape(-1), minlength=V), O.oracle_of(c), ti.size, c.name)


def test_few_allowed_tokens(E):
    """three allowed tokens, all in the last slice: the other slices publish no candidates"""
    t = check_case(E, O.few_allowed_case())
    assert set(np.unique(t).tolist()) == set(O.FEW_ALLOWED[1:])


def test_rearm_same_tokens(E):
    """the same launches twice on the same counters and workspace: identical, token for token"""
    c = O.capacity_cases(128256)[0]
    a = device_tokens(E, [c], seeds=O.SEEDS[:2])
    b = device_tokens(E, [c], seeds=O.SEEDS[:2])
    assert np.array_equal(a, b)
    assert np.unique(a).size > 8
