"""The device sampler's logit bias (SampleArgs::bias_ids / bias_vals, csrc/ops.h) through the raw op
`_engine.sample`.  The rule defines the result as exactly what the sampler returns for logits to which the host
added the bias in fp32 beforehand, so the core test runs every mode both ways -- the list on the device, and the
host-biased logits with no list -- with the same seeds and positions and asks for identical tokens."""
import numpy as np
import pytest
import torch

from aios_amd.runtime import sampler as host

pytestmark = pytest.mark.gpu

V3 = 9000    # three 4096-token slices, the last one partial (test_sample_processors_gpu.py's shape)
V1 = 1000    # one partial slice
VL = 151936  # 38 slices
B = 32
STRIDES = (1, 300, 512)
EDGES = (0, 4095, 4096, 8191, 8192)


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def tables(rows, stride):
    """rows: per row a list of (id, bias) or None (an empty entry) -> [B][stride] ids (-1 = empty) and biases"""
    ids = np.full((len(rows), stride), -1, np.int32)
    vals = np.zeros((len(rows), stride), np.float32)
    for b, r in enumerate(rows):
        assert len(r) <= stride
        for j, e in enumerate(r):
            if e is not None:
                ids[b, j], vals[b, j] = e
    return torch.from_numpy(ids).cuda(), torch.from_numpy(vals).cuda()


def host_biased(logits, rows):
    out = logits.clone()
    for b, r in enumerate(rows):
        ent = [e for e in r if e is not None]
        out[b] = torch.from_numpy(host.apply_logit_bias(logits[b].numpy(), [e[0] for e in ent], [e[1] for e in ent]))
    return out


def bias_rows(logits, stride, seed):
    """Per-row lists of at most `stride` entries, ids distinct within a row: the slice-edge ids and V - 1, a ban on
    the row's argmax, a +50 that makes a tail token the argmax, an empty row between biased ones, a row with empty
    entries in the middle, and rows that differ from one another."""
    nb, V = logits.shape
    rng = np.random.default_rng(seed)
    edges = [i for i in EDGES + (V - 1,) if i < V]
    rows = []
    for b in range(nb):
        best = int(logits[b].argmax())
        if b % 8 == 3:
            rows.append([])  # neutral, between biased rows
            continue
        if b % 8 == 1:
            head = [(best, -np.inf)]
        elif b % 8 == 2:
            head = [(V - 1 if best != V - 1 else V - 2, 50.0)]
        else:
            head = [(edges[(b + j) % len(edges)], float(rng.uniform(-6, 6))) for j in range(len(edges))]
            head = list(dict(head).items())
        head = head[:stride]
        n = int(rng.integers(len(head), stride + 1)) if b % 8 != 0 else stride  # (rows 0, 8, ..: the full stride)
        used = {i for i, _ in head}
        fill = [int(i) for i in rng.permutation(V) if int(i) not in used][:n - len(head)]
        row = head + [(i, float(rng.choice([-np.inf, rng.uniform(-6, 6)], p=[0.05, 0.95]))) for i in fill]
        if b % 8 == 4 and len(row) >= 3:  # empty entries in the middle of the row
            row[1] = None
            row[len(row) // 2] = None
        rows.append(row)
    return rows


MODES = {
    "greedy": dict(),
    "temperature": dict(temp=0.8),
    "top_k": dict(temp=0.8, top_k=40),
    "top_p": dict(temp=0.8, top_p=0.9),
    "top_k_top_p": dict(temp=0.8, top_k=40, top_p=0.9),
    "min_p": dict(temp=0.8, min_p=0.05),
    "penalties": dict(temp=0.8, top_k=40, pen=True),
}


def run_mode(E, d_logits, mode, seed, bias=None, pen_rows=None):
    """one sampler launch over d_logits [B][V]; bias: (ids, vals, stride) device tables or None"""
    nb, V = d_logits.shape
    tok = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    pos = torch.arange(nb, dtype=torch.int32, device="cuda") + 3
    keep = [tok, pos]
    temp = tk = tp = 0
    kw = {}
    if "temp" in mode:
        t, k, p = f32([mode["temp"]] * nb), i32([mode.get("top_k", 0)] * nb), f32([mode.get("top_p", 1.0)] * nb)
        keep += [t, k, p]
        temp, tk, tp = t.data_ptr(), k.data_ptr(), p.data_ptr()
    if "min_p" in mode:
        mp = f32([mode["min_p"]] * nb)
        keep.append(mp)
        kw["min_p"] = mp.data_ptr()
    if mode.get("pen"):
        w = np.full((nb, 12), -1, np.int32)
        for b, r in enumerate(pen_rows):
            w[b, :len(r)] = r
        w = torch.from_numpy(w).cuda()
        rp, pp, fp = f32([1.3] * nb), f32([0.5] * nb), f32([0.25] * nb)
        keep += [w, rp, pp, fp]
        kw.update(pen_tokens=w.data_ptr(), pen_stride=12, repeat_penalty=rp.data_ptr(), presence_penalty=pp.data_ptr(),
                  frequency_penalty=fp.data_ptr())
    if bias is not None:
        kw.update(bias_ids=bias[0].data_ptr(), bias_vals=bias[1].data_ptr(), bias_stride=bias[2])
    E.sample(d_logits.data_ptr(), V, nb, V, temp, tk, seed, tok.data_ptr(), pos.data_ptr(), 0, stream(), tp, **kw)
    torch.cuda.synchronize()
    return tok.cpu().tolist()


@pytest.fixture(scope="module")
def cases():
    """per vocabulary: the logits, and per stride the rows, the device tables and the host-biased logits (built
    once, shared by every mode, never written again)"""
    out = {}
    for V in (V3, V1):
        logits = torch.randn(B, V, generator=torch.Generator().manual_seed(11 + V)) * 2
        per = {}
        for s in STRIDES:
            rows = bias_rows(logits, s, seed=s)
            ids, vals = tables(rows, s)
            per[s] = (rows, (ids, vals, s), host_biased(logits, rows).cuda())
        pen_rows = [[int(logits[b].argmax()), 0, V - 1, 4095 % V, 4096 % V, int(logits[b].argmax())] for b in range(B)]
        out[V] = (logits, logits.cuda(), per, pen_rows)
    return out


@pytest.mark.parametrize("V", [V3, V1])
@pytest.mark.parametrize("name", list(MODES))
def test_device_bias_equals_host_biased_logits(E, cases, name, V):
    logits, d_logits, per, pen_rows = cases[V]
    mode = MODES[name]
    for s in STRIDES:
        rows, bias, d_biased = per[s]
        plain = run_mode(E, d_logits, mode, 99, None, pen_rows)
        for rep in range(2):  # (twice: the tickets re-arm and the table is rebuilt)
            got = run_mode(E, d_logits, mode, 99 + rep, bias, pen_rows)
            want = run_mode(E, d_biased, mode, 99 + rep, None, pen_rows)
            assert all(0 <= t < V for t in got)
            assert got == want, (name, V, s, rep, [b for b in range(B) if got[b] != want[b]])
        # the lists matter: with them the launch answers differently, and the neutral rows do not
        first = run_mode(E, d_logits, mode, 99, bias, pen_rows)
        assert first != plain, (name, V, s)
        assert all(first[b] == plain[b] for b in range(B) if not rows[b])
        if name == "greedy":
            for b in range(B):
                best = int(logits[b].argmax())
                if b % 8 == 1:
                    assert first[b] != best          # the ban on the argmax
                if b % 8 == 2:
                    assert first[b] in (V - 1, V - 2) and first[b] != best  # +50 made a tail token the argmax
        for b in range(B):  # no banned token anywhere
            assert first[b] not in {e[0] for e in rows[b] if e is not None and e[1] == -np.inf}


def test_large_vocabulary_last_slice(E):
    """V = 151,936 (38 slices), B = 2, once: the entries that decide the rows lie in the last slice"""
    V, nb = VL, 2
    logits = torch.randn(nb, V, generator=torch.Generator().manual_seed(4)) * 2
    last = 37 * 4096
    logits[0, last + 5] = 30.0   # row 0: the argmax, in the last slice, banned; V - 1 lifted to second place
    logits[1, last + 7] = -40.0  # row 1: a tail token of the last slice lifted to the top
    rows = [[(last + 5, -np.inf), (V - 1, 20.0), (0, -3.0), (4096, 1.5)],
            [(last + 7, 90.0), None, (V - 1, -np.inf), (8191, 2.0)]]
    ids, vals = tables(rows, 4)
    d, db = logits.cuda(), host_biased(logits, rows).cuda()
    assert run_mode(E, d, MODES["greedy"], 5, (ids, vals, 4)) == [V - 1, last + 7]
    for name in ("greedy", "temperature", "top_k_top_p"):
        assert run_mode(E, d, MODES[name], 5, (ids, vals, 4)) == run_mode(E, db, MODES[name], 5), name


def test_greedy_order_against_the_host_rule(E):
    """bias, then penalties: logit +0.5, bias -1.0, repeat_penalty 2.0, token in the window -> -0.5 * 2 = -1.0, below
    a rival at -0.9; penalty first would give 0.25 - 1 = -0.75, above it.  Further rows: random lists and windows
    against apply_logit_bias + apply_penalties + argmax."""
    nb, V = 8, V3
    rng = np.random.default_rng(21)
    logits = torch.randn(nb, V, generator=torch.Generator().manual_seed(8))
    logits[0] = -5.0
    logits[0, 4097], logits[0, 8999] = 0.5, -0.9
    rows = [[(4097, -1.0)]]
    wins = [[4097]]
    for b in range(1, nb):
        top = torch.topk(logits[b], 6).indices.tolist()
        rows.append([(t, float(rng.uniform(-3, 3))) for t in top[:4]] + [(int(i), -np.inf) for i in (top[4],)])
        wins.append(top[1:6] + [top[1]])
    rp, pp, fp = [2.0] + [1.4] * (nb - 1), [0.0] + [0.3] * (nb - 1), [0.0] + [0.2] * (nb - 1)
    want = []
    for b in range(nb):
        ent = rows[b]
        l = host.apply_logit_bias(logits[b].numpy(), [e[0] for e in ent], [e[1] for e in ent])
        want.append(int(np.argmax(host.apply_penalties(l, wins[b], rp[b], pp[b], fp[b]))))
    assert want[0] == 8999
    ids, vals = tables(rows, 5)
    w = np.full((nb, 6), -1, np.int32)
    for b, r in enumerate(wins):
        w[b, :len(r)] = r
    w = torch.from_numpy(w).cuda()
    d, drp, dpp, dfp = logits.cuda(), f32(rp), f32(pp), f32(fp)
    tok = torch.zeros(nb, dtype=torch.int32, device="cuda")
    for _ in range(2):
        tok.fill_(-1)
        E.sample(d.data_ptr(), V, nb, V, 0, 0, 0, tok.data_ptr(), 0, 0, stream(), pen_tokens=w.data_ptr(), pen_stride=6,
                 repeat_penalty=drp.data_ptr(), presence_penalty=dpp.data_ptr(), frequency_penalty=dfp.data_ptr(),
                 bias_ids=ids.data_ptr(), bias_vals=vals.data_ptr(), bias_stride=5)
        torch.cuda.synchronize()
        assert tok.cpu().tolist() == want


SPIKES = [5, 4097, 8500, 4000, 8998]  # logits 1.0 / 0.5 / 0 / -0.5 / -1.0 over -30, in all three slices


def test_bans_under_sampling_are_never_drawn(E):
    nb, V = 512, V3
    base = torch.full((V,), -30.0)
    for j, i in enumerate(SPIKES):
        base[i] = 1.0 - 0.5 * j
    banned = [SPIKES[0], SPIKES[2]]
    logits = base.repeat(nb, 1).cuda()
    ids, vals = tables([[(banned[0], -np.inf), None, (banned[1], -np.inf)]] * nb, 3)
    temp = torch.full((nb,), 0.8, device="cuda")
    pos = torch.arange(nb, dtype=torch.int32, device="cuda")
    tok = torch.zeros(nb, dtype=torch.int32, device="cuda")
    counts = {}
    for rep in range(4):
        E.sample(logits.data_ptr(), V, nb, V, temp.data_ptr(), 0, 300 + rep, tok.data_ptr(), pos.data_ptr(), 0, stream(),
                 bias_ids=ids.data_ptr(), bias_vals=vals.data_ptr(), bias_stride=3)
        torch.cuda.synchronize()
        for t in tok.cpu().tolist():
            counts[t] = counts.get(t, 0) + 1
    print("draws:", sorted(counts.items()))
    assert not set(counts) & set(banned)
    assert set(counts) == set(SPIKES) - set(banned)  # (2048 draws: each remaining spike has mass > 0.1)


def test_launcher_refuses_strides_outside_the_limit(E):
    assert E.SAMPLE_BIAS_MAX == host.BIAS_MAX == 512
    logits = torch.zeros(1, V1, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    ids, vals = tables([[(3, 1.0)]], 513)
    for stride in (0, 513, -1):
        with pytest.raises(RuntimeError, match="logit bias stride"):
            E.sample(logits.data_ptr(), V1, 1, V1, 0, 0, 0, tok.data_ptr(), 0, 0, stream(), bias_ids=ids.data_ptr(),
                     bias_vals=vals.data_ptr(), bias_stride=stride)
    E.sample(logits.data_ptr(), V1, 1, V1, 0, 0, 0, tok.data_ptr(), 0, 0, stream(), bias_ids=ids.data_ptr(),
             bias_vals=vals.data_ptr(), bias_stride=512)
    torch.cuda.synchronize()
    assert int(tok.item()) == 3
