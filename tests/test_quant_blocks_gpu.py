"""Every weight decoder on raw blocks the quantizer never emits (quant_block_oracle.py), against float64.

Element decode: get_rows within 3 x 2^-24 s_k of the float64 value (two fp32 roundings, with or without FMA
contraction); the bf16 outputs (QMatrix.dequant_bf16, legacy_to_bf16) within one bf16 ulp of bf16(float64 value)
everywhere and bit-equal to it outside the boundary band |w - boundary| <= 2^-22 s_k (a zero may carry either
sign: the sign of a float64 zero depends on the order its terms are subtracted in).

Products: reference W64 @ x64, error scale S = sum_k s_k |x_k| over the unfolded form (s_k = |d sc| q + |dmin m|):
  fp32-activation GEMV        (K + 8) 2^-24 S
  int8-activation GEMV        the same with x = ReferenceModel.q8(x); the 1e-40 run (127 / amax overflows) adds
                              sum |w_k| amax of that run
  bf16-operand GEMM / GEMV    sum_k h_k |a_k| + (K + 8) 2^-24 S', h_k = half a bf16 ulp of w_k, S' = sum |w_k| |a_k|,
                              a already bf16; + 2^-23 |C_prev| (accum)
Every output finite; the all-zero activation row gives exactly 0 through a store epilogue.

Two bounds follow the kernels' arithmetic instead of the first guess (measured misses: 1.2 - 1.9 x, never 2 x):
  * The GEMV decoders (qweight.h QStream / QFmt, gemv_q8.h) treat the symmetric formats as affine too: the codes are
    re-biased to unsigned u and the row computes d sc sum(u x) - bias d sc sum(x), bias 8 (Q4_0), 32 (Q6_K), 128
    (Q8_0, fp32 paths only; the int8 path keeps signed codes).  A 1e4 outlier channel under a code next to the
    bias has |w| = |d| but terms of 9e4 |d| and 8e4 |d|: the unfolded form of THAT arithmetic is
    s_k = |d sc| (u_k + bias) (oracle: s_fold), and S uses it for these formats.
  * One round-to-nearest bf16 rounding of w errs by up to half an ulp, which is 2^-8 |w| at the bottom of a
    binade and 2^-9 |w| only at its top; 2^-9 S' is not an upper bound of it (saturated blocks x offset
    activations: every error has the same sign).  h_k is the exact half ulp of each w_k.

Shapes: rows 128, K 512.  The LDS engines (kernel_sel 3) decline K = 512 and 2304 (K / 32 must be a multiple of 64):
K = 2048; the ring GEMM takes every 128-row Q4_K / Q6_K launch of M <= 32, so the skinny cases use 192 rows.
Each case asserts its route (gemv_plan family / gemv_bf16_engine_fits / gemm_route / gemm_pf_plan).

Largest error / bound seen on an MI355X, per path and format (measurements against the float64 reference, printed
again at the end of every run; they show headroom and are not asserted):
  get_rows          Q4_K 0.333  Q5_K 0.332  Q6_K / Q4_0 / Q8_0 / F16 / BF16 0 (bit-exact)
  gemv v1           Q4_K 0.0107  Q5_K 0.0094  Q6_K 0.0062  Q4_0 0.0057  Q8_0 0.0087  F16 0.0077  BF16 0.0065
  gemv v2           Q4_K 0.0107  Q5_K 0.0094  Q6_K 0.0062  Q4_0 0.0057  Q8_0 0.0082  F16 0.0077  BF16 (engine) 0.00011
  gemv q8           Q4_K 0.0079  Q5_K 0.0081  Q6_K 0.0055  Q4_0 0.0045  Q8_0 0.0066
  batch-1 sel 2     Q4_K 0.0091  Q5_K 0.0068  Q6_K 0.0031  Q4_0 0.0027  Q8_0 0.0045
  batch-1 sel 3     Q4_K 0.0020  Q5_K 0.0016  Q6_K 0.0012  Q4_0 0.0009  Q8_0 0.0017
  batched LDS       Q4_K 0.0019  Q5_K 0.0019  Q6_K 0.0020  Q4_0 0.0014  Q8_0 0.0016
  BF16 engine       BF16 0.00015
  gemm big          Q4_K 0.978  Q5_K 0.963  Q6_K 0.960  Q4_0 0.937  Q8_0 0.967  F16 0.00038  BF16 0.00033
  gemm skinny       Q4_K 0.948  Q5_K 0.978  Q6_K 0.965  Q4_0 0.949  Q8_0 0.970  F16 0.00035  BF16 0.00041
  gemm ring         Q4_K 0.978  Q6_K 0.960  mixed 0.978
  gemm pf           q4k 0.978  q5k 0.963  q6k 0.960  q8_0 0.968  q4_0 0.935  mixed 0.978  q5k_mixed 0.963  bf16 0.00033
  gemm pf split-K   Q4_K 0.978
(the quantized GEMM rows sit just under 1: the 1e4 outlier channel makes one weight's bf16 rounding the whole
error, and the half-ulp term is exact for it)
"""
import numpy as np
import pytest
import torch

import quant_block_oracle as O
from aios_amd.gguf.quants import GGMLType as T
from test_kernels_gpu import B1_SELS, PF_SEGS, PF_TILES, bf16_engine, q8_ref, stream

pytestmark = pytest.mark.gpu

ROWS, K = 128, 512
NATIVE = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q4_0, T.Q8_0, T.F16, T.BF16]
QUANT = NATIVE[:5]
LEGACY = [T.Q2_K, T.Q3_K, T.IQ4_NL, T.IQ4_XS, T.Q4_1, T.Q5_0, T.Q5_1, T.F32]


def cases(types):
    c = [(t, f) for t in types for f in O.families(t)]
    return dict(argnames="t,family", argvalues=c, ids=[f"{t.name}-{f}" for t, f in c])


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    print("\nlargest error / bound per path and format")
    for (path, fmt), r in sorted(RATIOS.items()):
        print(f"  {path:<16} {fmt:<7} {r:.3g}")


_qm = {}


def qmat(E, t, family, rows=ROWS, k=K):
    key = (int(t), family, rows, k)
    if key not in _qm:
        m = O.matrix(t, rows, k, family)
        _qm[key] = (E.QMatrix(int(t), rows, k, m.raw), m)
    return _qm[key]


def judge(path, t, tag, got, ref, bound, fails):
    """|got - ref| <= bound element-wise (bound 0: exactly equal); records the largest ratio"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        fails.append(f"{tag}: non-finite output")
        return
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    r = float(ratio.max())
    name = t if isinstance(t, str) else t.name
    RATIOS[(path, name)] = max(RATIOS.get((path, name), 0.0), r)
    if r > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        fails.append(f"{tag}: error / bound {r:.3g} at {i} (got {got[i]:.9g}, ref {ref[i]:.9g}, bound {bound[i]:.3g})")


def bf16_half_ulp(w):
    """the largest error of one round-to-nearest bf16 rounding of each w: between 2^-9 |w| and 2^-8 |w|"""
    return O.bf16_round(w)[1] / 2


# ------------------------------------------------------------------------------------------ element decode
def check_bf16(out, m, fails, tag):
    """out: int16 view of the bf16 output [rows, K]"""
    bits = out.cpu().numpy().view(np.uint16)
    val = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    r, ulp, _ = O.bf16_round(m.w)
    if not np.isfinite(val).all():
        fails.append(f"{tag}: non-finite")
        return
    if not (np.abs(val - r) <= ulp).all():
        fails.append(f"{tag}: {int((np.abs(val - r) > ulp).sum())} elements more than one bf16 ulp off")
    band = O.boundary_band(m.w, m.s)
    assert band.mean() <= 1e-3
    want = O.bf16_bits(r)
    same = (bits == want) | ((r == 0) & ((bits & 0x7FFF) == 0))
    bad = ~same & ~band
    if bad.any():
        i = np.unravel_index(int(bad.argmax()), bad.shape)
        fails.append(f"{tag}: {int(bad.sum())} elements not bit-equal outside the band, first {i}: got {bits[i]:#06x} "
                     f"want {want[i]:#06x} (w {m.w[i]!r})")


@pytest.mark.parametrize(**cases(NATIVE))
def test_decode_native(E, t, family):
    qm, m = qmat(E, t, family)
    fails = []
    out = torch.zeros(ROWS, K, dtype=torch.bfloat16, device="cuda")
    qm.dequant_bf16(out.data_ptr(), stream())
    torch.cuda.synchronize()
    check_bf16(out.view(torch.int16), m, fails, "dequant_bf16")
    perm = np.random.default_rng(1).permutation(ROWS).astype(np.int32)
    rows = torch.from_numpy(perm).cuda()
    g = torch.full((ROWS, K), 7.0, device="cuda")
    qm.get_rows(rows.data_ptr(), ROWS, g.data_ptr(), K, stream())
    torch.cuda.synchronize()
    judge("get_rows", t, "get_rows", g.cpu().numpy(), m.w[perm], 3 * 2.0 ** -24 * m.s[perm], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize(**cases(LEGACY))
def test_decode_legacy_to_bf16(E, t, family):
    m = O.matrix(t, ROWS, K, family)
    out = torch.zeros(ROWS, K, dtype=torch.bfloat16, device="cuda")
    E.legacy_to_bf16(int(t), m.raw, ROWS * K, out.data_ptr(), stream())
    torch.cuda.synchronize()
    fails = []
    check_bf16(out.view(torch.int16), m, fails, "legacy_to_bf16")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ GEMV
def gemv_case(E, path, t, family, B, fails, k=K, mode="v2", sel=0, grid=0, want_family=None):
    qm, m = qmat(E, t, family, ROWS, k)
    q8 = mode == "q8"
    if want_family:
        p = E.gemv_plan([int(t)], [ROWS], k, B, act_q8=int(q8), force_v1=int(mode == "v1"), kernel_sel=sel,
                        tune_grid=grid, cus=E.device_cu_count())
        assert p["family"] == want_family, (p["family"], want_family)
    b16 = t == T.BF16 and mode != "v1" and bf16_engine(E, [qm], B)
    for kind in O.ACTS:
        x = O.activations(kind, B, k, int8=q8)
        xt = torch.from_numpy(x)
        extra = 0.0
        if b16:  # the BF16 engine's operand: hand it bf16 values
            xt = xt.to(torch.bfloat16).float()
        xd = xt.cuda()
        y = torch.full((B, ROWS), 7.0, device="cuda")
        E.gemv([qm], B, xd.data_ptr(), k, 0, 1e-5, y.data_ptr(), ROWS, E.EPI_STORE, stream(), int(mode == "v1"), int(q8),
               grid, kernel_sel=sel)
        torch.cuda.synchronize()
        xr = (q8_ref(xt) if q8 else xt).numpy().astype(np.float64)
        if q8 and kind == "tiny":
            run, _ = O.TINY_RUNS[1]
            sl = slice(32 * run, 32 * run + 32)
            extra = np.abs(x[:, sl]).max(1)[:, None].astype(np.float64) * np.abs(m.w[:, sl]).sum(1)[None, :]
        ref = xr @ m.w.T
        if b16:
            bound = np.abs(xr) @ bf16_half_ulp(m.w).T + (k + 8) * 2.0 ** -24 * (np.abs(xr) @ np.abs(m.w).T)
        else:
            sk = m.s if (q8 and t == T.Q8_0) else m.s_fold  # (the int8 Q8_0 path keeps signed codes: no fold)
            bound = (k + 8) * 2.0 ** -24 * (np.abs(xr) @ sk.T) + extra
        tag = f"{path} {t.name}-{family} B{B} {kind}"
        got = y.cpu().numpy()
        judge(path, t, tag, got, ref, bound, fails)
        if kind == "sparse" and B > 1 and got[1].any():
            fails.append(f"{tag}: the all-zero row gave {np.abs(got[1]).max()}")


MODE_CASES = [(t, f, mode) for t in NATIVE for f in O.families(t) for mode in ("v1", "v2", "q8")
              if mode != "q8" or t in QUANT]  # (no int8 path for the 16-bit formats)


@pytest.mark.parametrize("t,family,mode", MODE_CASES, ids=[f"{t.name}-{f}-{mode}" for t, f, mode in MODE_CASES])
def test_gemv_modes(E, t, family, mode):
    fails = []
    for B in (1, 3):
        path = "gemv_" + mode + ("_bf16eng" if t == T.BF16 and mode == "v2" else "")
        gemv_case(E, path, t, family, B, fails, mode=mode,
                  want_family={"v1": "v1", "q8": "q8"}.get(mode) if t in QUANT else None)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("grid", [0, 3])
@pytest.mark.parametrize("sel", B1_SELS)
@pytest.mark.parametrize(**cases(QUANT))
def test_gemv_b1_engines(E, t, family, sel, grid):
    fails = []
    gemv_case(E, f"b1_sel{sel}", t, family, 1, fails, k=K if sel == 2 else 2048, mode="q8", sel=sel, grid=grid,
              want_family={2: "cu", 3: "lds"}[sel])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize(**cases(QUANT))
def test_gemv_lds_batched(E, t, family, B):
    fails = []
    gemv_case(E, "lds_batched", t, family, B, fails, k=2048, mode="q8", sel=3, want_family="lds")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("family", O.families(T.BF16))
def test_gemv_bf16_engine(E, family, B):
    qm, _ = qmat(E, T.BF16, family)
    assert bf16_engine(E, [qm], B)
    fails = []
    gemv_case(E, "bf16_engine", T.BF16, family, B, fails, mode="v2", want_family="lds16")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ GEMM
def gemm_case(E, path, name, mats, ms, M, fails, epi="store", ksplit=0, via_gemm=False):
    """mats / ms: the segments' QMatrix / oracle matrices; one launch per activation kind"""
    W = np.concatenate([m.w for m in ms], 0)
    N, k = W.shape
    for kind in O.ACTS:
        a = torch.from_numpy(O.activations(kind, M, k)).to(torch.bfloat16)
        A = a.cuda()
        prev = torch.from_numpy(np.random.default_rng(M).standard_normal((M, N)).astype(np.float32))
        C = (prev.clone() if epi == "accum" else torch.full((M, N), 5.0)).cuda()
        if via_gemm:
            E.gemm(A.data_ptr(), k, mats[0], M, C.data_ptr(), N, int(epi == "accum"), stream())
        else:
            E.gemm_q(A.data_ptr(), k, mats, M, C.data_ptr(), 0, N, E.GEPI_ACCUM if epi == "accum" else E.GEPI_STORE,
                     stream(), ksplit)
        torch.cuda.synchronize()
        a64 = a.float().numpy().astype(np.float64)
        ref = a64 @ W.T
        bound = np.abs(a64) @ bf16_half_ulp(W).T + (k + 8) * 2.0 ** -24 * (np.abs(a64) @ np.abs(W).T)
        if epi == "accum":
            ref = ref + prev.numpy().astype(np.float64)
            bound = bound + 2.0 ** -23 * np.abs(prev.numpy().astype(np.float64))
        tag = f"{path} {name} M{M} {epi} S{ksplit} {kind}"
        got = C.cpu().numpy()
        judge(path, name, tag, got, ref, bound, fails)
        if kind == "sparse" and epi == "store" and got[1].any():
            fails.append(f"{tag}: the all-zero row gave {np.abs(got[1]).max()}")


@pytest.mark.parametrize(**cases(NATIVE))
def test_gemm_big(E, monkeypatch, t, family):
    monkeypatch.setenv("AIOS_GEMM_PF", "0")
    qm, m = qmat(E, t, family)
    assert E.gemm_route(K, [qm], 100, ROWS, E.GEPI_STORE, 0) == [(0, "big")]
    fails = []
    for epi in ("store", "accum"):
        gemm_case(E, "gemm_big", t.name, [qm], [m], 100, fails, epi=epi, via_gemm=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize(**cases(NATIVE))
def test_gemm_skinny(E, t, family, ksplit):
    qm, m = qmat(E, t, family, rows=192)
    fails = []
    for epi in ("store", "accum"):
        assert E.gemm_route(K, [qm], 16, 192, E.GEPI_ACCUM if epi == "accum" else E.GEPI_STORE, ksplit) == [(0, "skinny")]
        gemm_case(E, "gemm_skinny", t.name, [qm], [m], 16, fails, epi=epi, ksplit=ksplit)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize(**cases([T.Q4_K, T.Q6_K]))
def test_gemm_ring(E, t, family):
    qm, m = qmat(E, t, family)
    fails = []
    for epi in ("store", "accum"):
        assert E.gemm_route(K, [qm], 8, ROWS, E.GEPI_ACCUM if epi == "accum" else E.GEPI_STORE, 0) == [(0, "ring")]
        gemm_case(E, "gemm_ring", t.name, [qm], [m], 8, fails, epi=epi)
    assert not fails, "\n".join(fails)


# one 128-column tile per format file of the prefill GEMM: (PF_SEGS stack, tile, file)
PF_CASES = [("q4k", "64x128", "q4k"), ("q5k", "128x128", "q5k"), ("q6k", "64x128", "q6k"), ("q8_0", "128x128", "q8q4"),
            ("q4_0", "256x128", "q8q4"), ("mixed", "128x128", "mix"), ("q5k_mixed", "64x128", "mix"),
            ("bf16", "64x128", "bf16")]


def pf_stack(E, stack, shift=0):
    """the stack's formats at 128 rows per segment, segment i from block family (i + shift)"""
    out = []
    for i, (t, _) in enumerate(PF_SEGS[stack]):
        fam = O.families(t)
        out.append(qmat(E, t, fam[(i + shift) % len(fam)]))
    return [q for q, _ in out], [m for _, m in out]


PF_PARAMS = [c + (sh,) for c in PF_CASES for sh in range(len(O.families(PF_SEGS[c[0]][0][0])))]


@pytest.mark.parametrize("stack,tile,file,shift", PF_PARAMS, ids=[f"{c[0]}-{c[3]}" for c in PF_PARAMS])
def test_gemm_pf(E, monkeypatch, stack, tile, file, shift):
    assert tile in PF_TILES
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    mats, ms = pf_stack(E, stack, shift)
    N = ROWS * len(mats)
    fails = []
    for epi in ("store", "accum"):
        ge = E.GEPI_ACCUM if epi == "accum" else E.GEPI_STORE
        assert E.gemm_route(K, mats, 33, N, ge, 1) == [(0, "pf")]
        assert E.gemm_pf_plan(mats, 33, ge, 1)[:2] == tuple(int(v) for v in tile.split("x"))
        gemm_case(E, "gemm_pf_" + file, stack, mats, ms, 33, fails, epi=epi, ksplit=1)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize(**cases([T.Q4_K]))
def test_gemm_pf_split_k(E, monkeypatch, t, family):
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", "64x128")
    qm, m = qmat(E, t, family)
    fails = []
    for epi in ("store", "accum"):
        ge = E.GEPI_ACCUM if epi == "accum" else E.GEPI_STORE
        assert E.gemm_route(K, [qm], 33, ROWS, ge, 2) == [(0, "pf")] and E.gemm_pf_plan([qm], 33, ge, 2)[2] == 2
        gemm_case(E, "gemm_pf_splitk", t.name, [qm], [m], 33, fails, epi=epi, ksplit=2)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_gemm_mixed_segments_ring(E, shift):
    """Q4_K + Q4_K + Q6_K in one ring launch, each segment from a different block family"""
    mats, ms = pf_stack(E, "mixed", shift)
    assert len({(m.t, m.family) for m in ms}) == 3
    assert E.gemm_route(K, mats, 8, 3 * ROWS, E.GEPI_STORE, 0) == [(0, "ring")]
    fails = []
    gemm_case(E, "gemm_ring_mixed", "mixed", mats, ms, 8, fails)
    assert not fails, "\n".join(fails)
