"""GPU: the work the batched-decode / short-prefill GEMMs fold into their epilogues -- RoPE + q store +
paged K/V write (GEPI_QKV), the RMSNorm split across two GEMMs (GEPI_ACCUM_NORM -> nrm_in), add_norm,
get_rows_step -- and the qkv_post / swiglu kernels, each against the float64 oracle (fused_oracle.py).

A fused GEMM epilogue is compared with host post-processing of the SAME launch's GEPI_STORE result (same
kernel, same split: asserted through gemm_route), so the tolerances are those of the epilogue arithmetic
alone.  Every GEMM launches twice into freshly sentinel-filled outputs: the second launch runs on the
split-K tickets the first one re-armed."""
import numpy as np
import pytest
import torch

import fused_oracle as O
from aios_amd.gguf.quants import GGMLType, dequantize, quantize

pytestmark = pytest.mark.gpu

Q4, Q5, Q6, Q8 = GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K, GGMLType.Q8_0
MAX_CTX, SLOTS, THETA = 512, 6, 10000.0
SENT16, SENT8, SENT32 = 0x5A5A, 0xA5, 0x5A5A5A5A  # untouched-cell bit patterns (bf16 / fp8 / fp32 buffers)
INV_K, INV_V = 8.0, 20.0  # fp8: code = value * inv; different, so a K / V swap fails


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


_mats = {}


def stack(E, segs, K, std=0.02):
    """[(type, rows)] -> (QMatrix list, dequantised [N, K] fp32), built once per module"""
    key = (tuple(segs), K, std)
    if key not in _mats:
        ms, refs = [], []
        for i, (t, n) in enumerate(segs):
            x = np.random.default_rng(500 + 13 * i + K + n).standard_normal((n, K)).astype(np.float32) * std
            raw = quantize(x, t)
            refs.append(torch.from_numpy(dequantize(raw, t).reshape(n, K).copy()))
            ms.append(E.QMatrix(int(t), n, K, raw))
        _mats[key] = (ms, torch.cat(refs, 0))
    return _mats[key]


def sent(shape, dtype, bits):
    """a device buffer of `dtype` with every element's bit pattern = bits"""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
    return torch.full(shape, bits, dtype=it, device="cuda").view(dtype)


def bits(t):
    t = t.detach().cpu().contiguous()
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.view(it)


def is_sent(t, b):
    return bits(t) == torch.tensor(b, dtype=torch.int64).to(bits(t).dtype)


_tables = {}


def rope_table(hd):
    if hd not in _tables:
        t = O.rope_table(MAX_CTX, hd, THETA)
        _tables[hd] = (t, t.cuda().contiguous())
    return _tables[hd]


class Rows:
    """M rows' (pos, slot) and a shuffled block table: slots drawn from {5, 0, 3, 1} (a non-identity
    order with gaps), positions including 128, 511, 0, 127 (block edges, first / last), all (slot, pos)
    distinct"""

    def __init__(self, M, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        special = [(3, 128), (5, 511), (1, 0), (0, 127)][:M]
        rest = [(s, p) for s in (5, 0, 3, 1) for p in range(MAX_CTX) if (s, p) not in special]
        pick = torch.randperm(len(rest), generator=g)[:M - len(special)].tolist()
        cells = special + [rest[i] for i in pick]
        assert len(set(cells)) == M
        slot, pos = torch.tensor([c[0] for c in cells]), torch.tensor([c[1] for c in cells])
        self.pos, self.slot = pos.int(), slot.int()
        self.bt = torch.randperm(SLOTS * MAX_CTX // O.KVB, generator=g).view(SLOTS, -1).int()
        self.dpos, self.dslot, self.dbt = self.pos.cuda(), self.slot.cuda(), self.bt.cuda()


def caches(Hkv, hd, fp8):
    n = (SLOTS * MAX_CTX // O.KVB, Hkv, O.KVB, hd)
    if fp8:
        return sent(n, torch.uint8, SENT8), sent(n, torch.uint8, SENT8)
    return sent(n, torch.bfloat16, SENT16), sent(n, torch.bfloat16, SENT16)


def check_qkv(v, geo, rows, q_out, kc, vc, fp8=False, neox=False, q_rel=2.0 ** -22, exact_v=True):
    """v [M, q_dim + 2 kv_dim]: the packed values before RoPE (fp32: what the epilogue holds, or float64 when
    a scale was applied on the host).  q_out rows < M and the cache cells of kv_targets against the oracle;
    every other element of q_out and of both caches must still hold its sentinel."""
    H, Hkv, hd = geo
    M, qd, kvd = v.shape[0], H * hd, Hkv * hd
    table = rope_table(hd)[0]
    vq, vk, vv = v[:, :qd].reshape(M, H, hd), v[:, qd:qd + kvd].reshape(M, Hkv, hd), v[:, qd + kvd:].reshape(M, Hkv, hd)
    q_ref = O.rope_pairs(vq, rows.pos, table, neox)
    k_ref = O.rope_pairs(vk, rows.pos, table, neox)
    # q: two products and one add in fp32 per element (contraction only tightens it)
    got_q = q_out.cpu()
    err = (got_q[:M].view(M, H, hd).double() - q_ref).abs()
    bound = q_rel * O.rope_pair_mag(vq, neox)
    assert bool((err <= bound).all()), ("q_out", float((err - bound).max()), float(err.max()))
    assert bool(is_sent(got_q[M:], SENT32).all()), "q_out rows >= M written"
    off = O.kv_targets(rows.pos, rows.slot, rows.bt, Hkv, hd, MAX_CTX).reshape(-1)
    mask = torch.zeros(kc.numel(), dtype=torch.bool)
    mask[off] = True
    assert int(mask.sum()) == off.numel()
    for name, cache, ref, inv in (("k", kc, k_ref, INV_K), ("v", vc, vv, INV_V)):
        flat = cache.cpu().reshape(-1)
        stray = ~is_sent(flat, SENT8 if fp8 else SENT16) & ~mask
        assert not bool(stray.any()), (name, "cells outside kv_targets written", int(stray.sum()),
                                       torch.nonzero(stray).flatten()[:8].tolist())
        got = flat[off].view(M, Hkv, hd)
        if fp8:
            assert float((ref.double() * inv).abs().max()) < 200
            val = got.view(torch.float8_e4m3fn).float().double() / inv
            e = (val - ref.double()).abs()
            b = O.fp8_bound(ref, 1.0 / inv)
            assert bool((e <= b).all()), (name, "fp8", float((e - b).max()))
        elif name == "v" and exact_v:  # no arithmetic between the accumulator and the store
            assert torch.equal(bits(got), bits(ref.to(torch.float32).to(torch.bfloat16))), "v not bit-equal"
        else:
            st = O.bf16_steps(got, ref.double())
            assert int(st.max()) <= 1, (name, "bf16 steps", int(st.max()))


# ---------------------------------------------------------------------------------------- GEPI_QKV
GEOS = [(4, 2, 64), (2, 1, 128)]  # q_dim 256, kv_dim 128, N 512 for both
K_QKV = 2048
# ksplit = 3 is not clamped at K = 2048: sk_qt limits S to nchunk = ceil(ceil(K / W / 4) / 4) X chunks, which
# is 4 for the 32-weight chunks of Q4_K / Q5_K / Q6_K and 8 for Q8_0's 16; the ring limits it to K / 256 = 8
STACKS = {
    "q4k": [(Q4, 512)],
    "q4k_m": [(Q4, 256), (Q4, 128), (Q6, 128)],      # the Q4_K_M QKV stack, 128-row segments
    "q4k_64": [(Q4, 192), (Q4, 320)],                # 64-row aligned seams: the ring and pf decline
    "q4k_m_64": [(Q4, 192), (Q4, 192), (Q6, 128)],   # ... the mixed launch of the skinny kernel
    "q8_0": [(Q8, 512)],
    "q5k": [(Q5, 512)],
    "q5k_m": [(Q5, 256), (Q5, 128), (Q6, 128)],      # Q5_K_M: no mixed launch below M = 33 -> two launches
}
PF_TILES = ["256x256", "128x256", "64x256", "256x128", "128x128", "64x128"]  # as test_gemm_pf_vs_unquantized


def _qkv_cases():
    c = []  # (stack, M, ksplit, fp8, tile, expected route)
    for st in ("q4k", "q4k_m"):
        for M in (5, 16, 17, 32):
            for ks in (0, 1):  # the ring's automatic split-K (last arriver) and its direct path
                c.append((st, M, ks, 0, None, [(0, "ring")]))
        for ks in (1, 3):
            c.append((st, 1, ks, 0, None, [(0, "skinny")]))
    for st, Ms in (("q4k_m_64", (1, 5, 16, 17, 32, 33, 64)), ("q4k_64", (5, 33)), ("q8_0", (1, 5, 16, 17, 32)),
                   ("q5k", (1, 5, 16, 17, 32))):
        for M in Ms:
            for ks in (1, 3):
                c.append((st, M, ks, 0, None, [(0, "skinny")]))
    for M in (1, 5, 32):  # format-split launches: the V launch starts at col0 = q_dim + kv_dim
        for ks in (1, 3):
            c.append(("q5k_m", M, ks, 0, None, [(0, "skinny"), (384, "ring" if M >= 2 else "skinny")]))
    for tile in PF_TILES:
        for st in (("q4k", "q5k") if tile.endswith("x256") else ("q4k_m", "q5k_m")):
            for M in (33, 64):
                c.append((st, M, 1, 0, tile, [(0, "pf")]))
    for st in ("q4k_m", "q8_0"):  # fp8 cache: pf declines it, so 33 and 64 run the skinny kernel at MT = 4
        for M in (5, 33, 64):
            for ks in (1, 3):
                c.append((st, M, ks, 1, None, [(0, "ring" if st == "q4k_m" and M <= 32 else "skinny")]))
    return c


def _case_id(c):
    st, M, ks, fp8, tile, route = c
    return f"{st}-M{M}-S{ks}-{'fp8' if fp8 else 'bf16'}-{tile or 'auto'}-{'+'.join(k for _, k in route)}"


def store_reference(E, monkeypatch, A, mats, M, N, ksplit, want, **kw):
    """the same launch with GEPI_STORE -> [M, N] fp32 on the host; it must take the route `want` (a STORE
    launch the prefill GEMM would serve where the fused one runs the skinny kernel is sent there too)"""
    K = A.shape[1]
    r = E.gemm_route(K, mats, M, N, E.GEPI_STORE, ksplit, **kw)
    if r != want:
        monkeypatch.setenv("AIOS_GEMM_PF", "0")
        r = E.gemm_route(K, mats, M, N, E.GEPI_STORE, ksplit, **kw)
    assert r == want, (r, want)
    C = torch.zeros(M, N, device="cuda")
    E.gemm_q(A.data_ptr(), K, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE, stream(), ksplit, **kw)
    torch.cuda.synchronize()
    monkeypatch.delenv("AIOS_GEMM_PF", raising=False)
    return C.cpu()


def qkv_kw(geo, rows, q_out, kc, vc, fp8):
    H, Hkv, hd = geo
    return dict(head_dim=hd, q_dim=H * hd, kv_dim=Hkv * hd, n_kv_heads=Hkv, max_ctx=MAX_CTX,
                rope_cs=rope_table(hd)[1].data_ptr(), pos=rows.dpos.data_ptr(), slot=rows.dslot.data_ptr(),
                block_table=rows.dbt.data_ptr(), q_out=q_out.data_ptr(), k_cache=kc.data_ptr(), v_cache=vc.data_ptr(),
                kv_fp8=int(fp8), kv_inv_k=INV_K, kv_inv_v=INV_V)


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "H%d_%d_%d" % g)
@pytest.mark.parametrize("case", _qkv_cases(), ids=_case_id)
def test_gemm_qkv_epilogue(E, monkeypatch, geo, case):
    """RoPE + q_out + paged K/V write of sk_epilogue (skinny / ring, direct and last-arriver paths) and
    pf_qkv_out (pf4 / pf8 / pf8c bodies) == the host post-processing of the same launch's fp32 product."""
    st, M, ks, fp8, tile, want = case
    H, Hkv, hd = geo
    if tile:
        monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    mats, _ = stack(E, STACKS[st], K_QKV)
    N = (H + 2 * Hkv) * hd
    A = torch.randn(M, K_QKV, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).cuda()
    rows = Rows(M, seed=M)
    for _ in range(2):
        q_out = sent((64, H * hd), torch.float32, SENT32)
        kc, vc = caches(Hkv, hd, fp8)
        kw = qkv_kw(geo, rows, q_out, kc, vc, fp8)
        assert E.gemm_route(K_QKV, mats, M, N, E.GEPI_QKV, ks, **kw) == want
        E.gemm_q(A.data_ptr(), K_QKV, mats, M, 0, 0, N, E.GEPI_QKV, stream(), ks, **kw)
        torch.cuda.synchronize()
    v = store_reference(E, monkeypatch, A, mats, M, N, ks, want)
    check_qkv(v, geo, rows, q_out, kc, vc, fp8=bool(fp8))


# ------------------------------------------------------------------- split RMSNorm: the producer
K_NRM = 1024


def _producer_cases():
    c = []  # (type, M, ksplit, rb4, expected kernel)
    for M in (3, 16, 20):
        c.append((Q4, M, 0, 0, "ring"))
        c.append((Q4, M, 1, 0, "ring"))
    for M in (3, 16, 20, 48):
        for ks in (1, 3):
            for rb4 in (0, 1):
                c.append((Q8, M, ks, rb4, "skinny"))
    for ks in (1, 3):
        for rb4 in (0, 1):
            c.append((Q4, 48, ks, rb4, "skinny"))
    return c


@pytest.mark.parametrize("N", [512, 1024])
@pytest.mark.parametrize("case", _producer_cases(),
                         ids=lambda c: f"{c[0].name}-M{c[1]}-S{c[2]}-{'rb4' if c[3] else 'rb8'}-{c[4]}")
def test_gemm_accum_norm_producer(E, monkeypatch, N, case):
    """GEPI_ACCUM_NORM: C += v bit-exactly, nrm_out16 = bf16(C_new * g), one sum of squares per output tile
    (128 columns, 64 under AIOS_SKINNY_RB=4) from the S == 1 wave / LDS reduction and the split-K last
    arriver's shuffle reduction; nothing written past row M."""
    t, M, ks, rb4, kern = case
    if rb4:
        monkeypatch.setenv("AIOS_SKINNY_RB", "4")
    mats, _ = stack(E, [(t, N)], K_NRM)
    parts = E.gemm_skinny_ntile(mats, M)
    tile = 64 if rb4 else 128
    assert parts == N // tile
    g = torch.Generator().manual_seed(N + M)
    A = torch.randn(M, K_NRM, generator=g).to(torch.bfloat16).cuda()
    C0 = torch.randn(M, N, generator=g)
    gw = (torch.rand(N, generator=g) + 0.5).cuda()
    want = [(0, kern)]
    for _ in range(2):
        C = sent((64, N), torch.float32, SENT32)
        C[:M] = C0.cuda()
        o16 = sent((64, N), torch.bfloat16, SENT16)
        part = sent((64, parts), torch.float32, SENT32)
        kw = dict(nrm_g=gw.data_ptr(), nrm_out16=o16.data_ptr(), nrm_part=part.data_ptr(), nrm_parts=parts)
        assert E.gemm_route(K_NRM, mats, M, N, E.GEPI_ACCUM_NORM, ks, **kw) == want
        E.gemm_q(A.data_ptr(), K_NRM, mats, M, C.data_ptr(), 0, N, E.GEPI_ACCUM_NORM, stream(), ks, **kw)
        torch.cuda.synchronize()
    v = store_reference(E, monkeypatch, A, mats, M, N, ks, want)
    Cn = C0 + v  # fp32, one add
    assert torch.equal(bits(C[:M]), bits(Cn)), "residual not the fp32 add"
    assert torch.equal(bits(o16[:M]), bits((Cn * gw.cpu()).to(torch.bfloat16))), "nrm_out16"
    ref = O.split_norm_parts(Cn, tile)
    rel = ((part[:M].cpu().double() - ref).abs() / ref).max().item()
    print("producer partial rel err", rel)
    assert rel <= (tile + 8) * 2.0 ** -24, rel
    for name, buf, b in (("C", C, SENT32), ("nrm_out16", o16, SENT16), ("nrm_part", part, SENT32)):
        assert bool(is_sent(buf[M:], b).all()), name + " rows >= M written"


# ------------------------------------------------------------------- split RMSNorm: the consumer
NRM_EPS = 1e-5
# Largest relative deviation of an fp32 consumer output from (same launch without nrm_in) x the float64
# rsqrt(sum / K + eps), over every parametrization below; the assertion allows 4x.
# Measured on an MI355X: 1.61e-7 (the largest of the 20 STORE cases, which lie in 0.9e-7 .. 1.61e-7) -- the
# fp32 sum of the partials, the divide, rsqrtf and the product, about 1.3 ulp together.  A dropped or doubled
# part moves the scale by >= 3e-3, four orders of magnitude above the bound.
CONSUMER_MEASURED = 1.61e-7
CONSUMER_TOL = 4 * CONSUMER_MEASURED
assert CONSUMER_TOL <= 1e-5  # a larger bound could not tell rounding from a mis-summed part


def _consumer_setup(E, t, M, nparts, N):
    mats, _ = stack(E, [(t, N)], K_NRM)
    g = torch.Generator().manual_seed(7 * M + nparts)
    A = torch.randn(M, K_NRM, generator=g).to(torch.bfloat16).cuda()
    # in [0.5, 1.5]: dropping or doubling one of <= 64 parts moves the scale by >= 0.3 %
    parts = torch.rand(64, nparts, generator=g) + 0.5
    return mats, A, parts, O.rsqrt_scale(parts[:M], K_NRM, NRM_EPS)


CONSUMER_ROUTES = [(Q4, 5, "ring"), (Q4, 20, "ring"), (Q8, 5, "skinny"), (Q8, 20, "skinny"), (Q8, 48, "skinny")]
_cons_ids = lambda c: f"{c[0].name}-M{c[1]}-{c[2]}"


@pytest.mark.parametrize("nparts", [4, 12, 32, 64])
@pytest.mark.parametrize("route", CONSUMER_ROUTES, ids=_cons_ids)
@pytest.mark.parametrize("epi", ["store", "swiglu"])
def test_gemm_nrm_in_consumer(E, monkeypatch, nparts, route, epi):
    """nrm_in: output row m of any epilogue is scaled by rsqrt(sum of the row's nrm_parts partials / K +
    eps); 12 parts: the lane guard of the non-power-of-two reduction."""
    t, M, kern = route
    N = 512
    mats, A, parts, scale = _consumer_setup(E, t, M, nparts, N)
    dparts = parts.cuda()
    want = [(0, kern)]
    kw = dict(nrm_in=dparts.data_ptr(), nrm_parts=nparts, nrm_eps=NRM_EPS)
    v = store_reference(E, monkeypatch, A, mats, M, N, 0, want).double()
    ref = v * scale[:, None]
    for _ in range(2):
        if epi == "store":
            C = sent((64, N), torch.float32, SENT32)
            assert E.gemm_route(K_NRM, mats, M, N, E.GEPI_STORE, 0, **kw) == want
            E.gemm_q(A.data_ptr(), K_NRM, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE, stream(), 0, **kw)
        else:
            C = sent((64, N // 2), torch.bfloat16, SENT16)
            assert E.gemm_route(K_NRM, mats, M, N // 2, E.GEPI_SWIGLU_BF16, 0, **kw) == want
            E.gemm_q(A.data_ptr(), K_NRM, mats, M, 0, C.data_ptr(), N // 2, E.GEPI_SWIGLU_BF16, stream(), 0, **kw)
        torch.cuda.synchronize()
    assert bool(is_sent(C[M:], SENT32 if epi == "store" else SENT16).all())
    if epi == "store":
        dev = ((C[:M].cpu().double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
        print("consumer rel dev", dev)
        assert dev <= CONSUMER_TOL, dev  # 4 x the measured 1.61e-7 (CONSUMER_MEASURED above)
    else:
        sw = torch.nn.functional.silu(ref[:, 0::2]) * ref[:, 1::2]
        assert int(O.bf16_steps(C[:M].cpu(), sw).max()) <= 1


@pytest.mark.parametrize("nparts", [4, 12, 32, 64])
@pytest.mark.parametrize("route", [(Q4, 5, "ring"), (Q8, 20, "skinny"), (Q8, 48, "skinny")], ids=_cons_ids)
def test_gemm_nrm_in_consumer_qkv(E, monkeypatch, nparts, route):
    """the consumer scale in front of the GEPI_QKV epilogue (the engine's batched-decode QKV launch)"""
    t, M, kern = route
    geo = GEOS[0]
    H, Hkv, hd = geo
    N = (H + 2 * Hkv) * hd
    mats, A, parts, scale = _consumer_setup(E, t, M, nparts, N)
    dparts = parts.cuda()
    want = [(0, kern)]
    rows = Rows(M, seed=nparts)
    v = store_reference(E, monkeypatch, A, mats, M, N, 0, want).double() * scale[:, None]
    for _ in range(2):
        q_out = sent((64, H * hd), torch.float32, SENT32)
        kc, vc = caches(Hkv, hd, False)
        kw = dict(qkv_kw(geo, rows, q_out, kc, vc, 0), nrm_in=dparts.data_ptr(), nrm_parts=nparts, nrm_eps=NRM_EPS)
        assert E.gemm_route(K_NRM, mats, M, N, E.GEPI_QKV, 0, **kw) == want
        E.gemm_q(A.data_ptr(), K_NRM, mats, M, 0, 0, N, E.GEPI_QKV, stream(), 0, **kw)
        torch.cuda.synchronize()
    # q: the scale's deviation on both pair members, then the RoPE arithmetic; V is scaled, so one bf16 step
    check_qkv(v, geo, rows, q_out, kc, vc, q_rel=CONSUMER_TOL + 2.0 ** -22, exact_v=False)


def test_gemm_nrm_in_bad_parts_raises(E):
    """nrm_parts = 6 (not a multiple of 4): no kernel takes it and launch_gemm_q must say so, not compute"""
    mats, A, parts, _ = _consumer_setup(E, Q4, 5, 6, 512)
    dparts = parts.cuda()
    C = sent((64, 512), torch.float32, SENT32)
    kw = dict(nrm_in=dparts.data_ptr(), nrm_parts=6, nrm_eps=NRM_EPS)
    with pytest.raises(RuntimeError, match="need the skinny"):
        E.gemm_route(K_NRM, mats, 5, 512, E.GEPI_STORE, 0, **kw)
    with pytest.raises(RuntimeError, match="need the skinny"):
        E.gemm_q(A.data_ptr(), K_NRM, mats, 5, C.data_ptr(), 0, 512, E.GEPI_STORE, stream(), 0, **kw)
    torch.cuda.synchronize()
    assert bool(is_sent(C, SENT32).all())


# ------------------------------------------------------------------- add_norm and the chained contract
def _chain_consumer(E, monkeypatch, x16, ld16, part, nparts, resid, gw, rows, d):
    """consumer GEMM (Q4_K, N = 256) on the producer's bf16(x * g) + partials against rmsnorm_bf16 followed by
    the plain GEMM on the same residual: g is applied before the bf16 rounding in one path and after the
    scale in the other, so the two differ by operand rounding -- relative L2 <= 6e-3, the bf16-operand
    bound of test_gemm_error_vs_unquantized_product"""
    N = 256
    mats, _ = stack(E, [(Q4, N)], d)
    want = [(0, "ring" if rows >= 2 else "skinny")]
    kw = dict(nrm_in=part.data_ptr(), nrm_parts=nparts, nrm_eps=NRM_EPS)
    for _ in range(2):
        Y = sent((64, N), torch.float32, SENT32)
        assert E.gemm_route(ld16, mats, rows, N, E.GEPI_STORE, 0, **kw) == want
        E.gemm_q(x16.data_ptr(), ld16, mats, rows, Y.data_ptr(), 0, N, E.GEPI_STORE, stream(), 0, **kw)
        torch.cuda.synchronize()
    xn = torch.zeros(rows, d, dtype=torch.bfloat16, device="cuda")
    E.rmsnorm_bf16(resid.data_ptr(), resid.stride(0), gw.data_ptr(), xn.data_ptr(), d, rows, d, NRM_EPS, stream())
    Yr = torch.zeros(rows, N, device="cuda")
    assert E.gemm_route(d, mats, rows, N, E.GEPI_STORE, 0) == want
    E.gemm_q(xn.data_ptr(), d, mats, rows, Yr.data_ptr(), 0, N, E.GEPI_STORE, stream(), 0)
    torch.cuda.synchronize()
    got, ref = Y[:rows].cpu().double(), Yr.cpu().double()
    rel = float((got - ref).norm() / ref.norm())
    assert rel <= 6e-3, rel
    assert bool(is_sent(Y[rows:], SENT32).all())


@pytest.mark.parametrize("d", [1024, 2048, 5120])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("with_data", [False, True])
def test_add_norm_and_chain(E, monkeypatch, d, rows, with_data):
    """launch_add_norm, the TP path's producer: residual += data (or as is), bf16(x * g), one partial per
    1024 columns, the padding partials (5120: 5 live of 8) written as exact zeros; then the chain."""
    nparts = E.resid_norm_parts(d)
    assert nparts == ((d // 1024 + 3) & ~3)
    g = torch.Generator().manual_seed(d + rows)
    r0 = torch.randn(rows, d, generator=g)
    data = torch.randn(rows, d, generator=g) if with_data else None
    gw = (torch.rand(d, generator=g) + 0.5).cuda()
    resid = r0.cuda()
    ddata = data.cuda() if with_data else None
    ld16 = d + 8
    o16 = sent((rows + 1, ld16), torch.bfloat16, SENT16)
    part = sent((rows + 1, nparts), torch.float32, SENT32)
    E.add_norm(resid.data_ptr(), ddata.data_ptr() if with_data else 0, rows, d, gw.data_ptr(), o16.data_ptr(), ld16,
               part.data_ptr(), nparts, stream())
    torch.cuda.synchronize()
    xn = r0 + data if with_data else r0
    assert torch.equal(bits(resid), bits(xn)), "residual not the fp32 add"
    assert int(O.bf16_steps(o16[:rows, :d].cpu(), (xn * gw.cpu()).double()).max()) <= 1
    live = d // 1024
    ref = O.split_norm_parts(xn, 1024)
    p = part.cpu()
    rel = ((p[:rows, :live].double() - ref).abs() / ref).max().item()
    assert rel <= (1024 + 8) * 2.0 ** -24, rel
    assert bool((bits(p[:rows, live:]) == 0).all()), "tail partials must be exact zeros"
    assert bool(is_sent(o16[:rows, d:], SENT16).all()) and bool(is_sent(o16[rows:], SENT16).all())
    assert bool(is_sent(part[rows:], SENT32).all())
    _chain_consumer(E, monkeypatch, o16, ld16, part, nparts, resid, gw, rows, d)


@pytest.mark.parametrize("M,kern", [(5, "ring"), (48, "skinny")])
def test_accum_norm_chain(E, monkeypatch, M, kern):
    """the same chain with a GEPI_ACCUM_NORM GEMM as the producer (the single-GPU batched decode)"""
    d, Kp = 1024, 512
    mats, _ = stack(E, [(Q4, d)], Kp)
    nparts = E.gemm_skinny_ntile(mats, M)
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, Kp, generator=g).to(torch.bfloat16).cuda()
    resid = torch.randn(M, d, generator=g).cuda()
    gw = (torch.rand(d, generator=g) + 0.5).cuda()
    o16 = torch.zeros(M, d, dtype=torch.bfloat16, device="cuda")
    part = torch.zeros(M, nparts, device="cuda")
    kw = dict(nrm_g=gw.data_ptr(), nrm_out16=o16.data_ptr(), nrm_part=part.data_ptr(), nrm_parts=nparts)
    assert E.gemm_route(Kp, mats, M, d, E.GEPI_ACCUM_NORM, 0, **kw) == [(0, kern)]
    E.gemm_q(A.data_ptr(), Kp, mats, M, resid.data_ptr(), 0, d, E.GEPI_ACCUM_NORM, stream(), 0, **kw)
    torch.cuda.synchronize()
    N = 256
    cm, _ = stack(E, [(Q4, N)], d)
    want = [(0, "ring" if M <= 32 else "skinny")]
    ckw = dict(nrm_in=part.data_ptr(), nrm_parts=nparts, nrm_eps=NRM_EPS)
    Y = torch.zeros(M, N, device="cuda")
    assert E.gemm_route(d, cm, M, N, E.GEPI_STORE, 0, **ckw) == want
    E.gemm_q(o16.data_ptr(), d, cm, M, Y.data_ptr(), 0, N, E.GEPI_STORE, stream(), 0, **ckw)
    xn = torch.zeros(M, d, dtype=torch.bfloat16, device="cuda")
    E.rmsnorm_bf16(resid.data_ptr(), d, gw.data_ptr(), xn.data_ptr(), d, M, d, NRM_EPS, stream())
    Yr = torch.zeros(M, N, device="cuda")
    monkeypatch.setenv("AIOS_GEMM_PF", "0")  # (M = 48: the reference product on the skinny kernel as well)
    assert E.gemm_route(d, cm, M, N, E.GEPI_STORE, 0) == want
    E.gemm_q(xn.data_ptr(), d, cm, M, Yr.data_ptr(), 0, N, E.GEPI_STORE, stream(), 0)
    torch.cuda.synchronize()
    rel = float((Y.cpu().double() - Yr.cpu().double()).norm() / Yr.cpu().double().norm())
    assert rel <= 6e-3, rel


# ----------------------------------------------------------------------------------------- qkv_post
def run_qkv_post(E, qkv, geo, rows, fp8, neox=0, bias=None, amax=None, use_table=True):
    H, Hkv, hd = geo
    T = qkv.shape[0]
    q_out = sent((T + 2, H * hd), torch.float32, SENT32)
    kc, vc = caches(Hkv, hd, fp8)
    E.qkv_post(qkv.data_ptr(), qkv.stride(0), T, H, Hkv, hd, 0, 0, 1e-6, neox, THETA, rows.dpos.data_ptr(),
               rows.dslot.data_ptr(), q_out.data_ptr(), kc.data_ptr(), vc.data_ptr(), MAX_CTX, stream(),
               block_table=rows.dbt.data_ptr(), rope_cs=rope_table(hd)[1].data_ptr() if use_table else 0,
               bias=bias.data_ptr() if bias is not None else 0, kv_fp8=int(fp8), kv_inv_k=INV_K, kv_inv_v=INV_V,
               amax=amax.data_ptr() if amax is not None else 0)
    torch.cuda.synchronize()
    return q_out, kc, vc


@pytest.mark.parametrize("geo", [(4, 2, 64), (32, 8, 128)], ids=lambda g: "H%d_%d_%d" % g)
@pytest.mark.parametrize("fp8", [0, 1])
def test_qkv_post_row_kernel(E, geo, fp8):
    """qkv_post_row_kernel (table RoPE, no norm, no bias: the Llama / Mistral path); (32, 8, 128) has 3072
    pairs per row, so the 2048-pair outer loop runs a second, partial pass"""
    H, Hkv, hd = geo
    T = 3
    qkv = torch.randn(T, (H + 2 * Hkv) * hd + 8, generator=torch.Generator().manual_seed(H))[:, :(H + 2 * Hkv) * hd]
    rows = Rows(T, seed=40 + H)
    dq = torch.empty(T, (H + 2 * Hkv) * hd + 8, device="cuda")[:, :(H + 2 * Hkv) * hd]
    dq.copy_(qkv)
    q_out, kc, vc = run_qkv_post(E, dq, geo, rows, fp8)
    check_qkv(qkv.contiguous(), geo, rows, q_out, kc, vc, fp8=bool(fp8))


@pytest.mark.parametrize("mode", ["bias", "neox_fp8", "neox_bias_fp8"])
def test_qkv_post_head_kernel(E, mode):
    """qkv_post_kernel (one wave per head): the bias add in front of RoPE, and NeoX pairs (i, i + hd / 2)
    into an fp8 cache -- the non-adjacent byte stores of kv_store_pair"""
    geo = (4, 2, 64)
    H, Hkv, hd = geo
    T, W = 3, (H + 2 * Hkv) * hd
    g = torch.Generator().manual_seed(len(mode))
    qkv = torch.randn(T, W, generator=g)
    bias = torch.randn(W, generator=g) if "bias" in mode else None
    neox, fp8 = int("neox" in mode), int("fp8" in mode)
    rows = Rows(T, seed=50)
    q_out, kc, vc = run_qkv_post(E, qkv.cuda(), geo, rows, fp8, neox=neox, bias=bias.cuda() if bias is not None else None)
    v = qkv + bias if bias is not None else qkv  # one fp32 add, as the kernel's
    if neox:  # V is never rotated: its reference pairs stay adjacent, only q / k use the NeoX pairing
        check_qkv(v, geo, rows, q_out, kc, vc, fp8=bool(fp8), neox=True)
    else:
        check_qkv(v, geo, rows, q_out, kc, vc, fp8=bool(fp8))


@pytest.mark.parametrize("kernel", ["row", "head"])
def test_qkv_post_amax(E, kernel):
    """the fp8 calibration observer of both kernels: per KV head the running max |value| about to be stored
    (K after RoPE, V as is) as float bit patterns; a NaN stays visible; a later, smaller launch changes
    nothing"""
    geo = (4, 2, 64)
    H, Hkv, hd = geo
    T, W, qd, kvd = 3, (H + 2 * Hkv) * hd, H * hd, Hkv * hd
    qkv = torch.randn(T, W, generator=torch.Generator().manual_seed(77))
    rows = Rows(T, seed=60)
    neox = 0 if kernel == "row" else 1  # NeoX takes the per-head kernel
    amax = torch.zeros(2, Hkv, dtype=torch.int32, device="cuda")
    run_qkv_post(E, qkv.cuda(), geo, rows, 0, neox=neox, amax=amax)
    tab = amax.cpu().view(torch.float32)
    vmax = qkv[:, qd + kvd:].view(T, Hkv, hd).abs().amax((0, 2))
    assert torch.equal(bits(tab[1]), bits(vmax)), "V row must be max |v| bit for bit"
    kref = O.rope_pairs(qkv[:, qd:qd + kvd].view(T, Hkv, hd), rows.pos, rope_table(hd)[0], bool(neox)).abs().amax((0, 2))
    assert bool(((tab[0].double() - kref).abs() <= 2.0 ** -22 * kref).all())
    before = amax.clone()
    run_qkv_post(E, (qkv * 0.5).cuda(), geo, rows, 0, neox=neox, amax=amax)
    assert torch.equal(amax, before), "the table is a running max"
    bad = qkv.clone()
    bad[1, qd + kvd + hd + 3] = float("nan")  # V, head 1
    run_qkv_post(E, bad.cuda(), geo, rows, 0, neox=neox, amax=amax)
    tab = amax.cpu().view(torch.float32)
    assert bool(torch.isnan(tab[1, 1])) and torch.equal(bits(tab[1, 0]), bits(vmax[0]))
    assert torch.equal(amax.cpu()[0], before.cpu()[0])


# --------------------------------------------------------------------------- get_rows_step, swiglu
@pytest.mark.parametrize("null_slot", [False, True])
def test_get_rows_step(E, null_slot):
    """get_rows plus the step's lookups: kv[b] = (pos[b], physical block of (slot[b], pos[b])), rope[b] = the
    table row of pos[b], bit for bit.  A null slot means ROW b's slot here (the first launch of a step has
    one row per slot) -- unlike the GEMM / qkv_post epilogues, where a null slot is slot 0."""
    V, K, B, hd = 96, 512, 4, 64
    mats, _ = stack(E, [(Q4, V)], K, std=0.05)
    m = mats[0]
    rows = Rows(B, seed=70)
    ids = torch.tensor([7, 95, 0, 33], dtype=torch.int32, device="cuda")
    ld = K + 4
    a = sent((B, ld), torch.float32, SENT32)
    b = sent((B, ld), torch.float32, SENT32)
    kv = sent((B + 1, 2), torch.int32, SENT32)
    rope = sent((B + 1, hd // 2, 2), torch.float32, SENT32)
    m.get_rows(ids.data_ptr(), B, a.data_ptr(), ld, stream())
    m.get_rows_step(ids.data_ptr(), B, b.data_ptr(), ld, stream(), rows.dpos.data_ptr(),
                    slot=0 if null_slot else rows.dslot.data_ptr(), block_table=rows.dbt.data_ptr(),
                    maxb=MAX_CTX // O.KVB, rope_cs=rope_table(hd)[1].data_ptr(), half=hd // 2, kv=kv.data_ptr(),
                    rope=rope.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))
    slot = torch.arange(B) if null_slot else rows.slot.long()
    blk = rows.bt[slot, rows.pos.long() // O.KVB]
    assert torch.equal(kv[:B].cpu(), torch.stack([rows.pos, blk], 1))
    assert torch.equal(bits(rope[:B]), bits(rope_table(hd)[0][rows.pos.long()]))
    assert bool(is_sent(kv[B:], SENT32).all()) and bool(is_sent(rope[B:], SENT32).all())


@pytest.mark.parametrize("n", [64, 1000, 20000])
def test_swiglu(E, n):
    """out[r][i] = silu(gu[r][2i]) * gu[r][2i + 1]: fp32 elementwise, the bound of test_rmsnorm"""
    rowsn, ldo = 3, n + 4
    gu = torch.randn(rowsn, 2 * n, generator=torch.Generator().manual_seed(n)) * 3
    out = sent((rowsn, ldo), torch.float32, SENT32)
    dgu = gu.cuda()
    E.swiglu(dgu.data_ptr(), 2 * n, out.data_ptr(), ldo, rowsn, n, stream())
    torch.cuda.synchronize()
    d = gu.double()
    ref = torch.nn.functional.silu(d[:, 0::2]) * d[:, 1::2]
    assert torch.allclose(out[:, :n].cpu().double(), ref, atol=1e-5, rtol=1e-5)
    assert bool(is_sent(out[:, n:], SENT32).all())
