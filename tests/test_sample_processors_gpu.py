"""Device sampler logit processors (min-p, repeat / presence / frequency penalties) against the host
sampler's rule (aios_amd.runtime.sampler: apply_penalties in fp32, probabilities in fp64), through the
raw op `_engine.sample` and through Engine.set_sample_processors."""
import numpy as np
import pytest
import torch

from aios_amd.runtime import sampler as host

pytestmark = pytest.mark.gpu

V3 = 9000  # three 4096-token slices, the last one partial: the smallest shape with a slice boundary and a tail


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def windows(rows, stride):
    """[B][stride] int32 penalty windows, -1 = empty entry"""
    w = np.full((len(rows), stride), -1, np.int32)
    for b, r in enumerate(rows):
        w[b, :len(r)] = r
    return torch.from_numpy(w).cuda()


def test_greedy_penalties_exact(E):
    B, V = 4, V3
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, V, generator=g)
    # row 0: the unpenalised argmax (4096) and the runners-up at the slice edges are penalised away
    logits[0, 4096], logits[0, 4095], logits[0, 8999], logits[0, 100] = 20.0, 15.0, 14.0, 13.0
    # row 1: every logit negative (the multiply branch); the best token appears three times (frequency)
    logits[1] -= 10.0
    logits[1, 7], logits[1, 5000] = -1.0, -1.5
    # row 3: its five best tokens and the slice-edge ids, some of them repeated
    top3 = torch.topk(logits[3], 5).indices.tolist()
    rows = [[4096, 4095, 8999], [7, 7, 7], [], top3 + [4095, 4096, 8999, top3[0], 4096, top3[0]]]
    rp, pp, fp = [1.5, 1.2, 1.7, 1.3], [0.5, 0.0, 1.0, 0.7], [0.25, 0.5, 0.3, 0.4]
    want = [int(np.argmax(host.apply_penalties(logits[b].numpy(), rows[b], rp[b], pp[b], fp[b]))) for b in range(B)]
    assert want[0] == 100 and want[1] == 5000 and want[2] == int(logits[2].argmax())  # the construction holds
    assert want[3] != int(logits[3].argmax())
    d = logits.cuda()
    w = windows(rows, 12)
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    drp, dpp, dfp = f32(rp), f32(pp), f32(fp)
    for _ in range(2):  # (twice: the tickets re-arm and the count table is rebuilt)
        tok.zero_()
        E.sample(d.data_ptr(), V, B, V, 0, 0, 0, tok.data_ptr(), 0, 0, stream(), pen_tokens=w.data_ptr(), pen_stride=12,
                 repeat_penalty=drp.data_ptr(), presence_penalty=dpp.data_ptr(), frequency_penalty=dfp.data_ptr())
        torch.cuda.synchronize()
        assert tok.cpu().tolist() == want


SPIKES = [5, 4097, 8500, 4000, 8998]  # logits 1.0 / 0.5 / 0 / -0.5 / -1.0 over -30, in all three slices


def spike_logits():
    base = torch.full((V3,), -30.0)
    for j, i in enumerate(SPIKES):
        base[i] = 1.0 - 0.5 * j
    return base


def device_counts(E, base, top_k, top_p, min_p, mask=None, window=None, presence=0.0):
    """512 rows (independent RNG streams) x 8 seeds of the device sampler at T = 0.8"""
    B, V = 512, base.shape[0]
    logits = base.repeat(B, 1).cuda()
    temp = torch.full((B,), 0.8, device="cuda")
    tk = torch.full((B,), top_k, dtype=torch.int32, device="cuda")
    tp = torch.full((B,), top_p, device="cuda")
    mp = torch.full((B,), min_p, device="cuda")
    pos = torch.arange(B, dtype=torch.int32, device="cuda")
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    m = torch.from_numpy(np.tile(np.frombuffer(mask, np.uint8), (B, 1))).cuda() if mask is not None else None
    kw = {}
    if window is not None:
        w = windows([window] * B, len(window))
        pres = torch.full((B,), presence, device="cuda")
        kw = dict(pen_tokens=w.data_ptr(), pen_stride=len(window), presence_penalty=pres.data_ptr())
    counts = {}
    for rep in range(8):
        E.sample(logits.data_ptr(), V, B, V, temp.data_ptr(), tk.data_ptr(), 77 + rep, tok.data_ptr(), pos.data_ptr(),
                 m.data_ptr() if m is not None else 0, stream(), tp.data_ptr(), min_p=mp.data_ptr(), **kw)
        torch.cuda.synchronize()
        for t in tok.cpu().tolist():
            counts[t] = counts.get(t, 0) + 1
    return counts


def check_distribution(counts, p):
    n = sum(counts.values())
    allowed = set(np.nonzero(p > 1e-9)[0].tolist())
    assert set(counts) <= allowed, (set(counts) - allowed)
    for i in allowed:
        print(f"token {i}: device {counts.get(i, 0) / n:.4f} host {p[i]:.4f}")
    for i in allowed:
        assert abs(counts.get(i, 0) / n - float(p[i])) < 0.04, (i, counts.get(i, 0) / n, float(p[i]))


@pytest.mark.parametrize("top_k,top_p,masked", [(0, 1.0, False), (4, 0.9, False), (0, 1.0, True)])
def test_min_p_distribution(E, top_k, top_p, masked):
    """min_p = 0.2 at T = 0.8: the spikes' ratios to the best are 1, 0.54, 0.29, 0.15, 0.08 -- three
    survive, none near the cut (with the top spike masked, the next three)."""
    base = spike_logits()
    mask = None
    if masked:
        bits = np.ones(V3, np.uint8)
        bits[SPIKES[0]] = 0
        mask = np.packbits(bits, bitorder="little").tobytes()
    p = host.probabilities(base.numpy(), 0.8, top_k, top_p, mask, min_p=0.2)
    assert set(np.nonzero(p)[0].tolist()) == set(SPIKES[1:4] if masked else SPIKES[:3])
    check_distribution(device_counts(E, base, top_k, top_p, 0.2, mask), p)


def test_penalties_then_min_p_distribution(E):
    """the top spike in the window with presence_penalty 1.0 (1.0 -> 0.0): min-p's M is the second spike"""
    base = spike_logits()
    pen = host.apply_penalties(base.numpy(), [SPIKES[0]], 1.0, 1.0, 0.0)
    p = host.probabilities(pen, 0.8, 0, 1.0, None, min_p=0.2)
    assert set(np.nonzero(p)[0].tolist()) == set(SPIKES[:4])
    check_distribution(device_counts(E, base, 0, 1.0, 0.2, window=[SPIKES[0]], presence=1.0), p)


def test_neutral_equals_absent(E):
    B, V = 64, 32000
    logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(5)) * 2).cuda()
    temp = torch.full((B,), 0.8, device="cuda")
    tk = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    tp = torch.full((B,), 0.95, device="cuda")
    pos = torch.arange(B, dtype=torch.int32, device="cuda")
    a = torch.zeros(B, dtype=torch.int32, device="cuda")
    b = torch.zeros(B, dtype=torch.int32, device="cuda")
    args = (logits.data_ptr(), V, B, V, temp.data_ptr(), tk.data_ptr(), 4242)
    E.sample(*args, a.data_ptr(), pos.data_ptr(), 0, stream(), tp.data_ptr())
    zeros, ones, w = f32([0.0] * B), f32([1.0] * B), windows([[]] * B, 4)
    E.sample(*args, b.data_ptr(), pos.data_ptr(), 0, stream(), tp.data_ptr(), min_p=zeros.data_ptr(),
             pen_tokens=w.data_ptr(), pen_stride=4, repeat_penalty=ones.data_ptr(), presence_penalty=zeros.data_ptr(),
             frequency_penalty=zeros.data_ptr())
    torch.cuda.synchronize()
    assert len(set(a.cpu().tolist())) > 8  # (it samples: not one token everywhere)
    assert torch.equal(a, b)


def test_vocabulary_limit(E):
    V = 262144  # 64 slices: the most the merge's slice table holds
    logits = torch.randn(1, V + 1, generator=torch.Generator().manual_seed(6))
    logits[0, V - 3] = 9.0
    d = logits.cuda()
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    E.sample(d.data_ptr(), V + 1, 1, V, 0, 0, 0, tok.data_ptr(), 0, 0, stream())
    torch.cuda.synchronize()
    assert int(tok.item()) == V - 3
    with pytest.raises(RuntimeError, match="vocabulary"):
        E.sample(d.data_ptr(), V + 1, 1, V + 1, 0, 0, 0, tok.data_ptr(), 0, 0, stream())


@pytest.fixture(scope="module")
def small_engine(tmp_path_factory):
    from aios_amd.models.config import get_preset
    from aios_amd.models.synthetic import write_synthetic_gguf
    from aios_amd.runtime.loader import load_engine

    path = write_synthetic_gguf(str(tmp_path_factory.mktemp("proc") / "small.gguf"), get_preset("test-small"), "Q4_K_M",
                                seed=7)
    eng, cfg, _ = load_engine(path, max_ctx=256, max_slots=2, max_batch=2)
    return eng, cfg


@pytest.mark.parametrize("pipelined", [False, True])
def test_engine_processors_one_shot(small_engine, pipelined):
    """8 greedy steps of B = 2 with frequency_penalty 2.0 over the rows' true recent tokens: every token
    is the argmax of the penalised logits of its step; a following step without the call is the plain
    argmax (the processors are one-shot).  That step is then run once more, from the same tokens and
    positions, with the token it produced added to the window: the penalty has to move it."""
    eng, cfg = small_engine
    V, B = cfg.vocab_size, 2
    prompts = [[1, 30, 40, 50, 60, 70, 80], [1, 31, 41, 51, 61]]
    seqs = []
    for s, p in enumerate(prompts):
        logits = np.asarray(eng.prefill(s, p, 0, True))
        seqs.append(list(p) + [int(np.argmax(logits))])

    def step(wins, host_tokens):
        """one decode step from the rows' last tokens; wins: the penalty windows, or None for no call"""
        last, pos = [s[-1] for s in seqs], [len(s) - 1 for s in seqs]
        if wins is not None:
            eng.set_sample_processors([0.0] * B, [1.0] * B, [0.0] * B, [2.0] * B, wins)
        if pipelined:
            eng.decode_submit([0, 1], last if host_tokens else [], pos, [0.0] * B, [0] * B, 0)
            eng.decode_sample(b"")
            out = eng.decode_collect()
        else:
            out = eng.decode([0, 1], last, pos, [0.0] * B, [0] * B, 0, b"")
        lg = np.asarray(eng.last_logits(B)).reshape(B, V)
        for b in range(B):
            want = lg[b] if wins is None else host.apply_penalties(lg[b], wins[b], 1.0, 0.0, 2.0)
            assert int(out[b]) == int(np.argmax(want)), (b, wins is not None)
        return [int(t) for t in out]

    for i in range(8):
        out = step([s[-64:] for s in seqs], i == 0)
        for b in range(B):
            seqs[b].append(out[b])
    plain = step(None, False)
    moved = step([s[-61:] + [plain[b]] * 3 for b, s in enumerate(seqs)], True)
    assert all(moved[b] != plain[b] for b in range(B))
    assert step(None, True) == plain


def test_engine_processors_resample_and_first(small_engine):
    """the other two sampler launches take the staged processors too, once"""
    eng, cfg = small_engine
    logits = np.asarray(eng.prefill(0, [1, 33, 44, 55], 0, True))
    best = int(np.argmax(logits))
    second = int(np.argmax(host.apply_penalties(logits, [best], 1.0, 1e4, 0.0)))
    assert second != best
    eng.set_sample_processors([0.0], [1.0], [1e4], [0.0], [[best]])
    assert eng.sample_first(3, 0.0, 0, 1.0, 1, b"") == second
    assert eng.sample_first(3, 0.0, 0, 1.0, 1, b"") == best
    tok = eng.decode([0], [best], [4], [0.0], [0], 0, b"")[0]
    lg = np.asarray(eng.last_logits(1)).reshape(-1)
    assert tok == int(np.argmax(lg))
    eng.set_sample_processors([0.0], [1.0], [1e4], [0.0], [[tok]])
    assert eng.resample(1, [0.0], [0], 0, b"")[0] == int(np.argmax(host.apply_penalties(lg, [tok], 1.0, 1e4, 0.0))) != tok
    assert eng.resample(1, [0.0], [0], 0, b"")[0] == tok
    # staged for two rows, launched with one: refused, and dropped
    eng.set_sample_processors([0.0] * 2, [1.0] * 2, [0.0] * 2, [0.0] * 2, [[1], [2]])
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.resample(1, [0.0], [0], 0, b"")
    assert eng.resample(1, [0.0], [0], 0, b"")[0] == tok


def test_engine_processors_validation(small_engine):
    eng, cfg = small_engine
    with pytest.raises(RuntimeError, match="size mismatch"):
        eng.set_sample_processors([0.0], [1.0, 1.0], [0.0], [0.0], [[1]])
    with pytest.raises(RuntimeError, match="window longer"):
        eng.set_sample_processors([0.0], [1.0], [0.0], [0.0], [[1] * 257])
    with pytest.raises(RuntimeError, match="token out of range"):
        eng.set_sample_processors([0.0], [1.0], [0.0], [0.0], [[cfg.vocab_size]])
    with pytest.raises(RuntimeError, match="batch out of range"):
        eng.set_sample_processors([0.0] * 3, [1.0] * 3, [0.0] * 3, [0.0] * 3, [[1]] * 3)


def ban(V, tok):
    """a one-row grammar mask that allows every token but tok"""
    bits = np.ones(V, np.uint8)
    bits[tok] = 0
    return np.packbits(bits, bitorder="little").tobytes()


def greedy_step(eng):
    """prefill slot 0, then the decode step (token t0 at position 4) the staging tests repeat: its token t0,
    its logits and their argmax"""
    t0 = int(np.argmax(np.asarray(eng.prefill(0, [1, 33, 44, 55], 0, True))))
    tok = eng.decode([0], [t0], [4], [0.0], [0], 0, b"")[0]
    lg = np.asarray(eng.last_logits(1)).reshape(-1)
    assert tok == int(np.argmax(lg))
    return t0, lg, tok


@pytest.mark.parametrize("with_logprobs", [False, True])
def test_throwing_call_drops_processors(small_engine, with_logprobs):
    """a decode that is refused (position out of range) drops the staged processors, and the staged logprobs
    beside them: the next valid decode of the row is the plain argmax and reports no logprobs"""
    eng, cfg = small_engine
    t0, lg, tok = greedy_step(eng)
    assert int(np.argmax(host.apply_penalties(lg, [tok], 1.0, 1e4, 0.0))) != tok   # (the penalty would move it)
    eng.set_sample_processors([0.0], [1.0], [1e4], [0.0], [[tok]])
    if with_logprobs:
        eng.set_logprobs([5])
    with pytest.raises(RuntimeError, match="position out of range"):
        eng.decode([0], [t0], [10 ** 6], [0.0], [0], 0, b"")
    assert eng.decode([0], [t0], [4], [0.0], [0], 0, b"")[0] == tok
    if with_logprobs:
        assert len(eng.last_logprobs()) == 0


def test_decode_loop_run_drops_processors(small_engine):
    """the graph-replayed loop carries no processors: staged ones are dropped there, not kept for the resample"""
    eng, cfg = small_engine
    t0, lg, tok = greedy_step(eng)
    assert int(np.argmax(host.apply_penalties(lg, [tok], 1.0, 1e4, 0.0))) != tok
    eng.set_sample_processors([0.0], [1.0], [1e4], [0.0], [[tok]])
    eng.decode_loop_prepare([0], [t0], [4])
    eng.decode_loop_run(1, 1, True)
    eng.synchronize()
    assert eng.resample(1, [0.0], [0], 0, b"")[0] == tok


@pytest.mark.parametrize("masked_first", [True, False])
def test_mask_argument_carries_no_state(small_engine, masked_first):
    """a masked and an unmasked decode of the same row, token and position on one engine, in either order,
    with and without capture_graphs between them: the mask bans the argmax in the one and nothing in the other"""
    eng, cfg = small_engine
    t0, lg, best = greedy_step(eng)
    rest = lg.copy()
    rest[best] = -np.inf
    calls = [(ban(cfg.vocab_size, best), int(np.argmax(rest))), (b"", best)]
    first, second = calls if masked_first else calls[::-1]
    for capture in (False, True):
        assert eng.decode([0], [t0], [4], [0.0], [0], 0, first[0])[0] == first[1]
        if capture:   # every graph of max_batch = 2: the unmasked and the masked step and the forward, per batch size
            assert eng.capture_graphs(2) == 6
        assert eng.decode([0], [t0], [4], [0.0], [0], 0, second[0])[0] == second[1]


def test_sampler_only_calls_leave_the_step_rows_alone(small_engine):
    """resample / sample_first between two pipelined steps upload sampling parameters only: the next
    decode_submit(tokens = {}) continues from the slots, tokens, positions and lengths on the device, and gives
    what the same steps give without the call in between"""
    eng, cfg = small_engine
    V, B = cfg.vocab_size, 2
    prompts = [[1, 30, 40, 50, 60, 70, 80], [1, 31, 41, 51, 61]]

    def run(between):
        first = [int(np.argmax(np.asarray(eng.prefill(s, p, 0, True)))) for s, p in enumerate(prompts)]
        pos = [len(p) for p in prompts]
        eng.decode_submit([0, 1], first, pos, [0.0] * B, [0] * B, 0)
        eng.decode_sample(b"")
        out1 = [int(t) for t in eng.decode_collect()]
        if between == "resample":
            assert [int(t) for t in eng.resample(2, [0.0] * B, [0] * B, 0, b"")] == out1
        elif between == "sample_first":   # (row 0 of the step's logits: the same greedy token)
            assert eng.sample_first(pos[0], 0.0, 0, 1.0, 1, b"") == out1[0]
        eng.decode_submit([0, 1], [], [p + 1 for p in pos], [0.0] * B, [0] * B, 0)
        eng.decode_sample(b"")
        out2 = [int(t) for t in eng.decode_collect()]
        lg = np.asarray(eng.last_logits(B)).reshape(B, V)
        assert out2 == [int(np.argmax(lg[b])) for b in range(B)]
        return out1, out2, lg

    want = run(None)
    for between in ("resample", "sample_first"):
        got = run(between)
        assert got[:2] == want[:2], between
        assert [int(np.argmax(r)) for r in got[2]] == [int(np.argmax(r)) for r in want[2]], between
