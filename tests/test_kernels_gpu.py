"""GPU numerics: every HIP kernel against a plain PyTorch fp32 reference of the same op."""
import math

import numpy as np
import pytest
import torch

from aios_amd.gguf.quants import GGMLType, dequantize, quantize
from attention_oracle import paged as paged_cache, unpaged  # noqa: F401  (one definition: the oracle's)

pytestmark = pytest.mark.gpu

QTS = [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q5_K, GGMLType.Q4_0, GGMLType.Q8_0, GGMLType.F16, GGMLType.BF16]


KVB = 128  # paged KV block (E.KV_BLOCK)


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def q8_ref(x):
    from aios_amd.models.reference import ReferenceModel

    return ReferenceModel.q8(x)


def bf16_ref(x):
    """the BF16 engine's activation operand (kernels/gemv_lds16.h): x (times the norm weight) rounded
    to bf16; the 1 / rms scale is applied to the fp32 row sums"""
    return x.to(torch.bfloat16).float()


def bf16_engine(E, segs, B, epi=0):
    return bool(getattr(E, "gemv_bf16_engine_fits", None)) and E.gemv_bf16_engine_fits(segs, B, epi)


def qmat(E, t, rows, cols, seed=0, std=0.05):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, cols)).astype(np.float32) * std
    raw = quantize(x, t)
    ref = torch.from_numpy(dequantize(raw, t).reshape(rows, cols).copy())
    return E.QMatrix(int(t), rows, cols, raw), ref


@pytest.mark.parametrize("t", QTS)
def test_dequant_exact(E, t):
    m, ref = qmat(E, t, 16, 512, seed=1)
    out = torch.empty(16, 512, dtype=torch.bfloat16, device="cuda")
    m.dequant_bf16(out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.to(torch.bfloat16))


@pytest.mark.parametrize("t", QTS)
def test_get_rows(E, t):
    m, ref = qmat(E, t, 32, 256, seed=2)
    rows = torch.tensor([3, 0, 31, 7], dtype=torch.int32, device="cuda")
    out = torch.empty(4, 256, device="cuda")
    m.get_rows(rows.data_ptr(), 4, out.data_ptr(), 256, stream())
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu(), ref[rows.cpu().long()], atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("t", QTS)
@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("K", [512, 2304])
@pytest.mark.parametrize("mode", ["v1", "v2", "q8"])
@pytest.mark.parametrize("N", [264, 4098])
def test_gemv_store(E, t, B, K, mode, N):
    m, W = qmat(E, t, N, K, seed=3)
    x = torch.randn(B, K, device="cuda")
    y = torch.zeros(B, N, device="cuda")
    q8 = mode == "q8" and t not in (GGMLType.F16, GGMLType.BF16)
    E.gemv([m], B, x.data_ptr(), K, 0, 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), int(mode == "v1"), int(q8))
    torch.cuda.synchronize()
    xr = q8_ref(x.cpu()) if q8 else x.cpu()
    if t == GGMLType.BF16 and mode != "v1" and bf16_engine(E, [m], B):
        xr = bf16_ref(x.cpu())
    ref = xr @ W.T
    # q8: an activation exactly on a rounding tie may land one int8 step away from the oracle's
    tol = 6e-3 if q8 else 2e-3
    assert torch.allclose(y.cpu(), ref, atol=tol, rtol=2e-3), (y.cpu() - ref).abs().max()


@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0])
@pytest.mark.parametrize("outliers", [False, True])
def test_gemv_q8_error_vs_unquantized_product(E, t, outliers):
    """The int8-activation (q8_1-style, per-32 block) GEMV against the UNQUANTIZED fp32 product
    of the same dequantized weights -- not a q8-emulating oracle: the activation rounding costs
    < 1.5 % relative L2 error of the outputs (< 3 % with 20x outlier channels, which inflate their
    blocks' scales), and the fp32-activation path stays at fp32 summation noise."""
    N, K = 512, 4096
    m, W = qmat(E, t, N, K, seed=21, std=0.02)
    x = torch.randn(1, K)
    if outliers:
        x[0, ::97] *= 20.0
    xd = x.cuda()
    out = {}
    for q8 in (0, 1):
        y = torch.zeros(1, N, device="cuda")
        E.gemv([m], 1, xd.data_ptr(), K, 0, 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), 0, q8)
        torch.cuda.synchronize()
        out[q8] = y.cpu().double()
    ref = x.double() @ W.double().T
    rel = lambda y: float((y - ref).norm() / ref.norm())  # noqa: E731
    assert rel(out[0]) < 1e-5, rel(out[0])
    assert rel(out[1]) < (0.03 if outliers else 0.015), rel(out[1])


@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0, GGMLType.BF16])
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("q8", [0, 1])
@pytest.mark.parametrize("ksplit", [0, 1])
def test_gemv_long_k(E, t, B, q8, ksplit):
    # K = 14336: fp32 persistent kernel / int8 k-split / int8 row kernels / v1 K-tiles (B = 4, fp32)
    N, K = 200, 14336
    m, W = qmat(E, t, N, K, seed=4, std=0.02)
    x = torch.randn(B, K, device="cuda")
    nw = torch.rand(K, device="cuda") + 0.5
    y = torch.zeros(B, N, device="cuda")
    q8 = q8 and t != GGMLType.BF16
    E.gemv([m], B, x.data_ptr(), K, nw.data_ptr(), 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), 0, q8, 0, 0, ksplit)
    torch.cuda.synchronize()
    xc = x.cpu()
    xn = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5) * nw.cpu()
    if q8:
        xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    if t == GGMLType.BF16 and bf16_engine(E, [m], B):
        xn = bf16_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    ref = xn @ W.T
    assert torch.allclose(y.cpu(), ref, atol=5e-3, rtol=5e-3)


def test_gemv_norm_resid_swiglu(E):
    K, F, B = 512, 256, 2
    gate, Wg = qmat(E, GGMLType.Q4_K, F, K, seed=5)
    up, Wu = qmat(E, GGMLType.Q4_K, F, K, seed=6)
    # interleave rows on the host through raw re-quantization of the dequantized values
    inter = torch.empty(2 * F, K)
    inter[0::2], inter[1::2] = Wg, Wu
    gu = E.QMatrix(int(GGMLType.BF16), 2 * F, K, inter.to(torch.bfloat16).view(torch.int16).numpy())
    Wgu = inter.to(torch.bfloat16).float()
    x = torch.randn(B, K, device="cuda") * 3
    nw = torch.rand(K, device="cuda") + 0.5
    out = torch.zeros(B, F, device="cuda")
    E.gemv([gu], B, x.data_ptr(), K, nw.data_ptr(), 1e-5, out.data_ptr(), F, E.EPI_SWIGLU, stream())
    torch.cuda.synchronize()
    xc = x.cpu()
    eng = bf16_engine(E, [gu], B)  # (BF16 weights: the BF16 engine rounds its x operand to bf16)
    xr = bf16_ref if eng else (lambda v: v)
    xn = xr(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    h = xn @ Wgu.T
    ref = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
    assert torch.allclose(out.cpu(), ref, atol=2e-3, rtol=2e-3)
    # residual epilogue
    y0 = torch.randn(B, 2 * F, device="cuda")
    y = y0.clone()
    E.gemv([gu], B, x.data_ptr(), K, 0, 1e-5, y.data_ptr(), 2 * F, E.EPI_RESID, stream())
    torch.cuda.synchronize()
    assert torch.allclose(y.cpu(), y0.cpu() + xr(xc) @ Wgu.T, atol=2e-3, rtol=2e-3)


def bf16_mat(rows, cols, seed, std=0.02):
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32) * std).to(torch.bfloat16)
    return w


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", ["tinyllama", "mistral"])
def test_gemv_bf16_engine_vs_unquantized(E, B, shape):
    """BF16 weights on the LDS-DMA engine (kernels/gemv_lds16.h), the decode projections of the BF16
    tiers (TinyLlama d 2048 / ff 5632; Mistral-size d 4096 / ff 14336): gate/up with the SwiGLU bf16
    hand-off, then down reading it, against the fp64 product of the UNROUNDED fp32 activations (< 0.6 %
    relative L2 error: bf16 rounding of x) and against fp64 of the kernel's own bf16 operands (fp32
    summation noise only)."""
    d, ff = (2048, 5632) if shape == "tinyllama" else (4096, 14336)
    gu16 = bf16_mat(2 * ff, d, 41)
    dn16 = bf16_mat(d, ff, 42)
    gu = E.QMatrix(int(GGMLType.BF16), 2 * ff, d, gu16.view(torch.int16).numpy())
    dn = E.QMatrix(int(GGMLType.BF16), d, ff, dn16.view(torch.int16).numpy())
    if not (bf16_engine(E, [gu], B) and bf16_engine(E, [dn], B)):
        assert shape == "mistral" and B >= 3, "the engine must take every TinyLlama shape at B <= 4"
        pytest.skip("long-K staging does not fit LDS at this batch (register kernels serve it)")
    gen = torch.Generator().manual_seed(43)
    x = (torch.randn(B, d, generator=gen) * 2).cuda()
    nw = (torch.rand(d, generator=gen) + 0.5).cuda()
    h16 = torch.zeros(B, ff, dtype=torch.bfloat16, device="cuda")
    E.gemv([gu], B, x.data_ptr(), d, nw.data_ptr(), 1e-5, 0, ff, E.EPI_SWIGLU, stream(), y16=h16.data_ptr())
    y0 = torch.randn(B, d, generator=gen).cuda()
    y = y0.clone()
    E.gemv([dn], B, 0, ff, 0, 1e-5, y.data_ptr(), d, E.EPI_RESID, stream(), x16=h16.data_ptr())
    torch.cuda.synchronize()
    xc = x.cpu().double()
    inv = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    Wgu, Wdn = gu16.double(), dn16.double()
    # unrounded activations
    h = (xc * inv * nw.cpu().double()) @ Wgu.T
    hs = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
    rel = lambda a, r: float((a - r).norm() / r.norm())  # noqa: E731
    assert rel(h16.cpu().double(), hs) < 6e-3, rel(h16.cpu().double(), hs)
    # the kernel's own operands: bf16(x * g), fp32 sums, then the rms scale; bf16 hand-off
    hk = (bf16_ref(x.cpu() * nw.cpu()).double() * inv) @ Wgu.T
    hks = torch.nn.functional.silu(hk[:, 0::2]) * hk[:, 1::2]
    assert torch.allclose(h16.cpu().double(), hks, atol=1e-2, rtol=8e-3)  # (bf16 output rounding)
    ref_dn = h16.cpu().double() @ Wdn.T
    assert rel(y.cpu().double() - y0.cpu().double(), ref_dn) < 1e-4
    assert rel(y.cpu().double() - y0.cpu().double(), hs @ Wdn.T) < 1.2e-2


@pytest.mark.parametrize("B", [1, 3])
def test_gemv_bf16_engine_qkv(E, B):
    """BF16 QKV (three segments, the TinyLlama heads) through the BF16 engine's RoPE + paged KV
    epilogue, batch 1 (the prefetched pos / block / rope path) and 3 (the generic epilogue)"""
    d, H, Hkv, hd, max_ctx, slots = 2048, 32, 4, 64, 256, 3
    mats = [bf16_mat(n, d, 50 + i) for i, n in enumerate((H * hd, Hkv * hd, Hkv * hd))]
    segs = [E.QMatrix(int(GGMLType.BF16), w.shape[0], d, w.view(torch.int16).numpy()) for w in mats]
    assert bf16_engine(E, segs, B, E.EPI_QKV)
    gen = torch.Generator().manual_seed(54)
    x = torch.randn(B, d, generator=gen).cuda()
    nw = (torch.rand(d, generator=gen) + 0.5).cuda()
    pos = torch.tensor([141, 7, 200][:B], dtype=torch.int32, device="cuda")
    slot = torch.tensor([1, 2, 0][:B], dtype=torch.int32, device="cuda")
    kp, bt = paged_cache(torch.zeros(slots, Hkv, max_ctx, hd, dtype=torch.bfloat16), shuffle=True, seed=5)
    kp, bt = kp.cuda(), bt.cuda()
    vp = torch.zeros_like(kp)
    q = torch.zeros(B, H * hd, device="cuda")
    E.gemv_qkv(segs, B, x.data_ptr(), d, nw.data_ptr(), 1e-5, q.data_ptr(), 0, hd, H, Hkv, max_ctx, 0, 10000.0,
               pos.data_ptr(), slot.data_ptr(), kp.data_ptr(), vp.data_ptr(), stream(), 0, block_table=bt.data_ptr())
    torch.cuda.synchronize()
    kc, vc = unpaged(kp, slots, max_ctx, bt), unpaged(vp, slots, max_ctx, bt)
    xc = x.cpu()
    xn = bf16_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    Wq, Wk, Wv = (w.float() for w in mats)
    qr = rope_ref((xn @ Wq.T).view(B, H, hd), pos.cpu(), 10000.0)
    kr = rope_ref((xn @ Wk.T).view(B, Hkv, hd), pos.cpu(), 10000.0)
    vr = (xn @ Wv.T).view(B, Hkv, hd)
    assert torch.allclose(q.cpu().view(B, H, hd), qr, atol=2e-3, rtol=2e-3), (q.cpu().view(B, H, hd) - qr).abs().max()
    for b in range(B):
        s_, p_ = int(slot[b]), int(pos[b])
        assert torch.allclose(kc[s_, :, p_].float().cpu(), kr[b], atol=2e-2, rtol=1e-2)
        assert torch.allclose(vc[s_, :, p_].float().cpu(), vr[b], atol=2e-2, rtol=1e-2)
    assert int((kc != 0).sum()) == B * Hkv * hd and int((vc != 0).sum()) == B * Hkv * hd


def rope_ref(x, pos, theta, neox=False):
    hd = x.shape[-1]
    p = torch.arange(hd // 2, dtype=torch.float32)
    freq = torch.pow(torch.tensor(theta), -2.0 * p / hd)
    ang = pos.float()[:, None] * freq[None]
    c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
    out = torch.empty_like(x)
    if neox:
        a, b = x[..., :hd // 2], x[..., hd // 2:]
        return torch.cat([a * c - b * s, a * s + b * c], -1)
    a, b = x[..., 0::2], x[..., 1::2]
    out[..., 0::2] = a * c - b * s
    out[..., 1::2] = a * s + b * c
    return out


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("q8", [0, 1])
def test_gemv_qkv_rope_kv(E, mixed, q8):
    d, H, Hkv, hd, max_ctx, slots = 256, 4, 2, 64, 128, 3
    B = 3
    wq, Wq = qmat(E, GGMLType.Q4_K, H * hd, d, seed=7)
    wk, Wk = qmat(E, GGMLType.Q4_K, Hkv * hd, d, seed=8)
    wv, Wv = qmat(E, GGMLType.Q6_K if mixed else GGMLType.Q4_K, Hkv * hd, d, seed=9)
    x = torch.randn(B, d, device="cuda")
    nw = torch.rand(d, device="cuda") + 0.5
    pos = torch.tensor([5, 17, 100], dtype=torch.int32, device="cuda")
    slot = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    kp, bt = paged_cache(torch.zeros(slots, Hkv, max_ctx, hd, dtype=torch.bfloat16), shuffle=True, seed=3)
    kp, bt = kp.cuda(), bt.cuda()
    vp = torch.zeros_like(kp)
    q = torch.zeros(B, H * hd, device="cuda")
    E.gemv_qkv([wq, wk, wv], B, x.data_ptr(), d, nw.data_ptr(), 1e-5, q.data_ptr(), 0, hd, H, Hkv, max_ctx, 0,
               10000.0, pos.data_ptr(), slot.data_ptr(), kp.data_ptr(), vp.data_ptr(), stream(), q8,
               block_table=bt.data_ptr())
    torch.cuda.synchronize()
    kc, vc = unpaged(kp, slots, max_ctx, bt), unpaged(vp, slots, max_ctx, bt)
    xc = x.cpu()
    xn = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5) * nw.cpu()
    if q8:
        xn = q8_ref(xn)
    qr = rope_ref((xn @ Wq.T).view(B, H, hd), pos.cpu(), 10000.0)
    kr = rope_ref((xn @ Wk.T).view(B, Hkv, hd), pos.cpu(), 10000.0)
    vr = (xn @ Wv.T).view(B, Hkv, hd)
    assert torch.allclose(q.cpu().view(B, H, hd), qr, atol=2e-3, rtol=2e-3)
    for b in range(B):
        s, p = int(slot[b]), int(pos[b])
        assert torch.allclose(kc[s, :, p].float().cpu(), kr[b], atol=2e-2, rtol=1e-2)
        assert torch.allclose(vc[s, :, p].float().cpu(), vr[b], atol=2e-2, rtol=1e-2)


# ---- one-workgroup-per-CU batch-1 GEMVs: sel 2 = register-streaming (kernels/gemv_cu.h), 3 = the
# LDS-DMA loader/consumer engine (kernels/gemv_lds.h; needs K / chunk % 64 == 0, else it falls back);
# pair ranges split over workgroups, tune_grid forces the workgroup count (ragged splits, > 64 pairs
# per workgroup so the epilogue wave takes a second pass, rows straddling two waves / two slots)
B1_SELS = [2, 3]


@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q5_K, GGMLType.Q4_0, GGMLType.Q8_0])
@pytest.mark.parametrize("K", [2304, 4096, 14336])
@pytest.mark.parametrize("grid", [0, 3, 37])
@pytest.mark.parametrize("sel", B1_SELS)
def test_gemv_b1_cu_store(E, t, K, grid, sel):
    N = 1030
    m, W = qmat(E, t, N, K, seed=31, std=0.02)
    x = torch.randn(1, K, device="cuda")
    nw = torch.rand(K, device="cuda") + 0.5
    y = torch.zeros(1, N, device="cuda")
    E.gemv([m], 1, x.data_ptr(), K, nw.data_ptr(), 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), 0, 1, grid,
           kernel_sel=sel)
    torch.cuda.synchronize()
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    ref = xn @ W.T
    assert torch.allclose(y.cpu(), ref, atol=5e-3, rtol=5e-3), (y.cpu() - ref).abs().max()


@pytest.mark.parametrize("grid", [0, 2, 11])
@pytest.mark.parametrize("sel", B1_SELS)
def test_gemv_b1_cu_swiglu_resid(E, grid, sel):
    K, F = 4096, 600
    gate, Wg = qmat(E, GGMLType.Q4_K, F, K, seed=32, std=0.02)
    up, Wu = qmat(E, GGMLType.Q4_K, F, K, seed=33, std=0.02)
    # interleaved (gate_i, up_i) rows in one Q4_K matrix, as the loader repacks ffn_gate/ffn_up
    inter = torch.empty(2 * F, K)
    inter[0::2], inter[1::2] = Wg, Wu
    raw = quantize(inter.numpy(), GGMLType.Q4_K)
    Wgu = torch.from_numpy(dequantize(raw, GGMLType.Q4_K).reshape(2 * F, K).copy())
    gu = E.QMatrix(int(GGMLType.Q4_K), 2 * F, K, raw)
    x = torch.randn(1, K, device="cuda") * 3
    nw = torch.rand(K, device="cuda") + 0.5
    out = torch.zeros(1, F, device="cuda")
    E.gemv([gu], 1, x.data_ptr(), K, nw.data_ptr(), 1e-5, out.data_ptr(), F, E.EPI_SWIGLU, stream(), 0, 1, grid,
           kernel_sel=sel)
    torch.cuda.synchronize()
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    h = xn @ Wgu.T
    ref = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
    assert torch.allclose(out.cpu(), ref, atol=5e-3, rtol=5e-3), (out.cpu() - ref).abs().max()
    y0 = torch.randn(1, 2 * F, device="cuda")
    y = y0.clone()
    E.gemv([gu], 1, x.data_ptr(), K, 0, 1e-5, y.data_ptr(), 2 * F, E.EPI_RESID, stream(), 0, 1, grid,
           kernel_sel=sel)
    torch.cuda.synchronize()
    ref = y0.cpu() + q8_ref(xc) @ Wgu.T
    assert torch.allclose(y.cpu(), ref, atol=5e-3, rtol=5e-3), (y.cpu() - ref).abs().max()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("grid", [0, 1, 5])
@pytest.mark.parametrize("sel", B1_SELS)
def test_gemv_b1_cu_qkv(E, mixed, table, grid, sel):
    d, H, Hkv, hd, max_ctx, slots = 2048, 8, 2, 64, 256, 2
    wq, Wq = qmat(E, GGMLType.Q4_K, H * hd, d, seed=34)
    wk, Wk = qmat(E, GGMLType.Q4_K, Hkv * hd, d, seed=35)
    wv, Wv = qmat(E, GGMLType.Q6_K if mixed else GGMLType.Q4_K, Hkv * hd, d, seed=36)
    # seeded: an unseeded x put a q element 0.0035 off once in ~600 runs (an int8 activation that
    # rounds the other way on the device flips one per-32 product)
    gen = torch.Generator().manual_seed(37)
    x = torch.randn(1, d, generator=gen).cuda()
    nw = (torch.rand(d, generator=gen) + 0.5).cuda()
    pos = torch.tensor([141], dtype=torch.int32, device="cuda")
    slot = torch.tensor([1], dtype=torch.int32, device="cuda")
    kp, bt = paged_cache(torch.zeros(slots, Hkv, max_ctx, hd, dtype=torch.bfloat16), shuffle=True, seed=4)
    kp, bt = kp.cuda(), bt.cuda()
    vp = torch.zeros_like(kp)
    q = torch.zeros(1, H * hd, device="cuda")
    cs = 0
    if table:
        p = torch.arange(hd // 2, dtype=torch.float64)
        ang = torch.arange(max_ctx, dtype=torch.float64)[:, None] * torch.pow(10000.0, -2.0 * p / hd)[None]
        rope_t = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous().cuda()
        cs = rope_t.data_ptr()
    E.gemv_qkv([wq, wk, wv], 1, x.data_ptr(), d, nw.data_ptr(), 1e-5, q.data_ptr(), 0, hd, H, Hkv, max_ctx, 0,
               10000.0, pos.data_ptr(), slot.data_ptr(), kp.data_ptr(), vp.data_ptr(), stream(), 1,
               block_table=bt.data_ptr(), rope_cs=cs, tune_grid=grid, kernel_sel=sel)
    torch.cuda.synchronize()
    kc, vc = unpaged(kp, slots, max_ctx, bt), unpaged(vp, slots, max_ctx, bt)
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    qr = rope_ref((xn @ Wq.T).view(1, H, hd), pos.cpu(), 10000.0)
    kr = rope_ref((xn @ Wk.T).view(1, Hkv, hd), pos.cpu(), 10000.0)
    vr = (xn @ Wv.T).view(1, Hkv, hd)
    assert torch.allclose(q.cpu().view(1, H, hd), qr, atol=5e-3, rtol=5e-3), (q.cpu().view(1, H, hd) - qr).abs().max()
    assert torch.allclose(kc[1, :, 141].float().cpu(), kr[0], atol=2e-2, rtol=1e-2)
    assert torch.allclose(vc[1, :, 141].float().cpu(), vr[0], atol=2e-2, rtol=1e-2)
    # nothing else in the cache was written
    assert int((kc != 0).sum()) == Hkv * hd and int((vc != 0).sum()) == Hkv * hd


@pytest.mark.parametrize("hd,H,Hkv", [(64, 8, 1), (128, 32, 8), (64, 32, 4), (128, 40, 8),
                                       (64, 4, 4), (128, 12, 6)])  # (the last two: G = 1 and G = 2)
@pytest.mark.parametrize("lens,max_ctx", [([1], 256), ([37, 200], 256), ([64, 65, 129, 1], 256),
                                          ([256, 255, 192], 256),
                                          # several 512-key splits: exercises the cross-workgroup combine
                                          ([1500, 513, 512, 2048], 2048), ([1025, 3], 1280)])
@pytest.mark.parametrize("split", [0, 64, 192])  # 0 = the launcher's choice
@pytest.mark.parametrize("paging", ["identity", "slot_table", "row_table"])
@pytest.mark.parametrize("grouped", ["", "1"])  # "1": AIOS_ATTN_GROUPED_MIN=1, the batched grouped mode
def test_attention_decode(E, hd, H, Hkv, lens, max_ctx, split, paging, grouped, monkeypatch):
    if grouped:
        if split not in (0, 64):
            pytest.skip("grouped mode: launcher and one-pass splits cover it")
        monkeypatch.setenv("AIOS_ATTN_GROUPED_MIN", grouped)
    B = len(lens)
    slots = B + 1
    kc = (torch.randn(slots, Hkv, max_ctx, hd) * 0.5).to(torch.bfloat16)
    vc = torch.randn(slots, Hkv, max_ctx, hd).to(torch.bfloat16)
    kp, bt = paged_cache(kc, shuffle=paging != "identity", seed=11)
    vp, _ = paged_cache(vc, shuffle=paging != "identity", seed=11)
    kp, vp = kp.cuda(), vp.cuda()
    bt_rows = 0
    if paging == "row_table":  # table indexed by batch row (the engine's decode rows)
        bt = torch.stack([bt[b + 1] for b in range(B)])
        bt_rows = 1
    bt_dev = bt.cuda() if bt is not None else None
    q = torch.randn(B, H, hd, device="cuda")
    seq = torch.tensor(lens, dtype=torch.int32, device="cuda")
    slot = torch.tensor(list(range(1, B + 1)), dtype=torch.int32, device="cuda")
    nch = max_ctx // E.ATTN_CHUNK
    opart = torch.empty(B, H, nch, hd, device="cuda")
    ml = torch.empty(B, H, nch, 2, device="cuda")
    out = torch.empty(B, H * hd, device="cuda")
    cnt = torch.zeros(B, H, dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(hd)
    for _ in range(2):  # second launch checks the counters re-armed themselves
        out.zero_()
        E.attn_decode(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), seq.data_ptr(), slot.data_ptr(), B, H, Hkv, hd,
                      max_ctx, nch, scale, opart.data_ptr(), ml.data_ptr(), out.data_ptr(), cnt.data_ptr(), stream(),
                      split, bt_dev.data_ptr() if bt_dev is not None else 0, bt_rows)
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0
    G = H // Hkv
    log2e = 1.4426950408889634
    for b in range(B):
        L, s = lens[b], b + 1
        k = kc[s, :, :L].float().cpu().repeat_interleave(G, 0)
        v = vc[s, :, :L].float().cpu().repeat_interleave(G, 0)
        # the op as the kernel defines it: q * scale * log2(e) rounded to bf16 (v_dot2_f32_bf16
        # scores, as the MFMA prefill rounds q), then an fp32 base-2 softmax and fp32 P.V
        qs = (q[b].cpu() * (scale * log2e)).to(torch.bfloat16).float()
        att = torch.softmax(torch.einsum("hd,hsd->hs", qs, k) * math.log(2.0), -1)
        ref = torch.einsum("hs,hsd->hd", att, v).reshape(-1)
        assert torch.allclose(out[b].cpu(), ref, atol=2e-4, rtol=2e-3), (b, (out[b].cpu() - ref).abs().max())
        # and against unrounded fp32 attention: the bf16 q costs < 1e-2 absolute here
        att32 = torch.softmax(torch.einsum("hd,hsd->hs", q[b].cpu(), k) * scale, -1)
        ref32 = torch.einsum("hs,hsd->hd", att32, v).reshape(-1)
        assert (out[b].cpu() - ref32).abs().max() < 1e-2


def fp8_codes(x, scale):
    """logical values -> (OCP e4m3 codes as uint8, their dequantised fp32 values) at one scale"""
    c = (x.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    return c.view(torch.uint8), c.float() * scale


@pytest.mark.parametrize("hd,H,Hkv", [(128, 32, 8), (64, 32, 4)])
@pytest.mark.parametrize("lens,max_ctx", [([1], 256), ([37, 200], 256), ([700], 1024), ([3000, 129], 4096),
                                          ([20000, 9000], 32768)])
@pytest.mark.parametrize("grouped", ["", "1"])
def test_attention_decode_fp8_kv(E, hd, H, Hkv, lens, max_ctx, grouped, monkeypatch):
    """fp8 e4m3 KV pool (EngineConfig::kv_fp8): the decode attention reads 1-byte codes, K converted to
    bf16 pairs for v_dot2 with the layer's K scale folded into q, V to fp32 with its scale on the output
    -- against fp32 attention over the dequantised codes (the op as defined), short / long / grouped
    modes with a shuffled block table; 32k keys: several passes per long-mode workgroup"""
    if grouped:
        monkeypatch.setenv("AIOS_ATTN_GROUPED_MIN", grouped)
    B = len(lens)
    slots = B + 1
    sk, sv = 0.02, 0.05  # per-layer scales (value = code x scale)
    kc = torch.randn(slots, Hkv, max_ctx, hd) * 0.5
    vc = torch.randn(slots, Hkv, max_ctx, hd)
    k8, kdq = fp8_codes(kc, sk)
    v8, vdq = fp8_codes(vc, sv)
    kp, bt = paged_cache(k8, shuffle=True, seed=12)
    vp, _ = paged_cache(v8, shuffle=True, seed=12)
    kp, vp, bt_dev = kp.cuda(), vp.cuda(), bt.cuda()
    q = torch.randn(B, H, hd, device="cuda")
    seq = torch.tensor(lens, dtype=torch.int32, device="cuda")
    slot = torch.tensor(list(range(1, B + 1)), dtype=torch.int32, device="cuda")
    nch = max_ctx // E.ATTN_CHUNK
    opart = torch.empty(B, H, nch, hd, device="cuda")
    ml = torch.empty(B, H, nch, 2, device="cuda")
    out = torch.empty(B, H * hd, device="cuda")
    cnt = torch.zeros(B, H, dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(hd)
    E.attn_decode(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), seq.data_ptr(), slot.data_ptr(), B, H, Hkv, hd,
                  max_ctx, nch, scale, opart.data_ptr(), ml.data_ptr(), out.data_ptr(), cnt.data_ptr(), stream(),
                  0, bt_dev.data_ptr(), 0, kv_fp8=1, k_scale=sk, v_scale=sv)
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0
    G = H // Hkv
    log2e = 1.4426950408889634
    for b in range(B):
        L, s_ = lens[b], b + 1
        k = kdq[s_, :, :L].repeat_interleave(G, 0)
        v = vdq[s_, :, :L].repeat_interleave(G, 0)
        # q * scale * log2(e) * k_scale rounded to bf16, dot with the codes (exact in bf16), fp32 softmax
        qs = (q[b].cpu() * (scale * log2e * sk)).to(torch.bfloat16).float()
        att = torch.softmax(torch.einsum("hd,hsd->hs", qs, k / sk) * math.log(2.0), -1)
        ref = torch.einsum("hs,hsd->hd", att, v).reshape(-1)
        assert torch.allclose(out[b].cpu(), ref, atol=5e-4, rtol=5e-3), (b, (out[b].cpu() - ref).abs().max())


@pytest.mark.parametrize("H,Hkv,hd", [(32, 8, 128), (32, 4, 64)])
@pytest.mark.parametrize("start,T", [(0, 37), (70, 130), (0, 300)])
def test_attention_prefill_fp8_kv(E, H, Hkv, hd, start, T):
    """the prefill flash attention over an fp8 e4m3 KV pool: tiles converted to bf16 with the layer's
    scales while staging, then the bf16 MFMA math -- against fp32 attention over the dequantised codes"""
    max_ctx = 512
    slot, slots = 1, 2
    G = H // Hkv
    sk, sv = 0.03, 0.04
    k8, kdq = fp8_codes(torch.randn(slots, Hkv, max_ctx, hd) * 0.5, sk)
    v8, vdq = fp8_codes(torch.randn(slots, Hkv, max_ctx, hd), sv)
    kp, bt = paged_cache(k8, True, seed=6)
    vp, _ = paged_cache(v8, True, seed=6)
    kp, vp, bt_dev = kp.cuda(), vp.cuda(), bt.cuda()
    q = torch.randn(T, H, hd, device="cuda")
    out = torch.zeros(T, H * hd, dtype=torch.bfloat16, device="cuda")
    scale = 1 / math.sqrt(hd)
    E.attn_prefill(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), slot, start, T, H, Hkv, hd, max_ctx, scale,
                   out.data_ptr(), H * hd, stream(), bt_dev.data_ptr(), kv_fp8=1, k_scale=sk, v_scale=sv)
    torch.cuda.synchronize()
    L = start + T
    k = kdq[slot, :, :L].repeat_interleave(G, 0)
    v = vdq[slot, :, :L].repeat_interleave(G, 0)
    # q * scale * log2(e) * k_scale rounded to bf16 against the codes (exact in bf16)
    qq = (q.cpu() * (scale * 1.4426950408889634 * sk)).to(torch.bfloat16).float() / (1.4426950408889634 * sk)
    s_ = torch.einsum("thd,hld->htl", qq, k)
    pos = torch.arange(start, L)[:, None]
    s_ = s_.masked_fill(torch.arange(L)[None, :] > pos, float("-inf"))
    ref = torch.einsum("htl,hld->thd", torch.softmax(s_, -1), v).reshape(T, H * hd)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 3e-2, err


@pytest.mark.parametrize("n", [2048, 4096, 8192, 6000])
@pytest.mark.parametrize("y_off", [0, 1])
def test_rmsnorm(E, n, y_off):
    """register kernel (n <= 4096: NV = 4; <= 8192: NV = 8 -- Llama-3-70B's d 8192) and the scalar
    kernel (n % 4 != 0 or a misaligned output: y_off shifts y by one element)"""
    x = torch.randn(5, n, device="cuda") * 2
    w = torch.rand(n, device="cuda")
    ld = n + 4
    ybuf = torch.zeros(5 * ld + 8, device="cuda")
    y = ybuf[y_off:y_off + 5 * ld].view(5, ld)
    E.rmsnorm(x.data_ptr(), n, w.data_ptr(), y.data_ptr(), ld, 5, n, 1e-5, stream())
    ybb = torch.zeros(5 * ld + 8, dtype=torch.bfloat16, device="cuda")
    yb = ybb[y_off:y_off + 5 * ld].view(5, ld)
    E.rmsnorm_bf16(x.data_ptr(), n, w.data_ptr(), yb.data_ptr(), ld, 5, n, 1e-5, stream())
    torch.cuda.synchronize()
    ref = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5) * w
    assert torch.allclose(y[:, :n], ref, atol=1e-5, rtol=1e-5)
    assert torch.allclose(yb[:, :n].float(), ref, atol=2e-2, rtol=1e-2)
    assert not y[:, n:].any() and not yb[:, n:].float().any()  # nothing past each row


@pytest.mark.parametrize("neox", [0, 1])
def test_qkv_post_qknorm(E, neox):
    T, H, Hkv, hd, max_ctx = 4, 4, 2, 128, 128
    qkv = torch.randn(T, (H + 2 * Hkv) * hd, device="cuda")
    qn = torch.rand(hd, device="cuda") + 0.5
    kn = torch.rand(hd, device="cuda") + 0.5
    pos = torch.tensor([0, 1, 9, 33], dtype=torch.int32, device="cuda")
    kp = torch.zeros(max_ctx // KVB, Hkv, KVB, hd, dtype=torch.bfloat16, device="cuda")
    vp = torch.zeros_like(kp)
    q = torch.empty(T, H * hd, device="cuda")
    E.qkv_post(qkv.data_ptr(), qkv.shape[1], T, H, Hkv, hd, qn.data_ptr(), kn.data_ptr(), 1e-6, neox, 1e6,
               pos.data_ptr(), 0, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), max_ctx, stream())
    torch.cuda.synchronize()
    kc = unpaged(kp, 1, max_ctx)
    c = qkv.cpu()
    rms = lambda x, w: x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w
    qr = rope_ref(rms(c[:, :H * hd].view(T, H, hd), qn.cpu()), pos.cpu(), 1e6, bool(neox))
    kr = rope_ref(rms(c[:, H * hd:(H + Hkv) * hd].view(T, Hkv, hd), kn.cpu()), pos.cpu(), 1e6, bool(neox))
    assert torch.allclose(q.cpu().view(T, H, hd), qr, atol=1e-4, rtol=1e-4)
    for t in range(T):
        assert torch.allclose(kc[0, :, int(pos[t])].float().cpu(), kr[t], atol=2e-2, rtol=1e-2)
    # V: no norm, no RoPE -- the input rounded to bf16, bit for bit, at (head, pos[t]) and nowhere else
    vc = unpaged(vp, 1, max_ctx).cpu()
    vr = c[:, (H + Hkv) * hd:].view(T, Hkv, hd).to(torch.bfloat16)
    for t in range(T):
        assert torch.equal(vc[0, :, int(pos[t])].view(torch.int16), vr[t].view(torch.int16))
    other = torch.ones(max_ctx, dtype=torch.bool)
    other[pos.cpu().long()] = False
    assert not vc[0][:, other].view(torch.int16).any()


def test_sample_greedy_and_mask(E):
    B, V = 3, 32000
    logits = torch.randn(B, V, device="cuda")
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    E.sample(logits.data_ptr(), V, B, V, 0, 0, 0, tok.data_ptr(), 0, 0, stream())
    torch.cuda.synchronize()
    assert torch.equal(tok.cpu().long(), logits.argmax(-1).cpu())
    # grammar mask: allow only tokens 10..19
    mask = np.zeros((B, V // 8), np.uint8)
    for b in range(B):
        for i in range(10, 20):
            mask[b, i >> 3] |= 1 << (i & 7)
    m = torch.from_numpy(mask).cuda()
    E.sample(logits.data_ptr(), V, B, V, 0, 0, 0, tok.data_ptr(), 0, m.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(tok.cpu().long(), logits[:, 10:20].argmax(-1).cpu() + 10)


def test_sample_temperature_topk_distribution(E):
    V = 1000
    logits = torch.full((1, V), -10.0, device="cuda")
    logits[0, 3], logits[0, 7], logits[0, 11] = 2.0, 1.0, 0.0
    temp = torch.tensor([1.0], device="cuda")
    topk = torch.tensor([2], dtype=torch.int32, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = {}
    for i in range(400):
        pos = torch.tensor([i], dtype=torch.int32, device="cuda")
        E.sample(logits.data_ptr(), V, 1, V, temp.data_ptr(), topk.data_ptr(), 1234, tok.data_ptr(), pos.data_ptr(),
                 0, stream())
        counts[int(tok.item())] = counts.get(int(tok.item()), 0) + 1
    assert set(counts) <= {3, 7}
    p3 = counts.get(3, 0) / 400
    assert abs(p3 - math.e / (math.e + 1)) < 0.08


@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_sample_greedy_multi_slice(E, V):
    """Greedy argmax through the two-phase sampler (V/4096 slice workgroups + last-arriver merge),
    repeated to check the per-row tickets re-arm."""
    B = 5
    logits = torch.randn(B, V, device="cuda")
    logits[1, V - 1] = 50.0  # winner in the last (partial) slice
    logits[2, 0] = 50.0
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    for _ in range(3):
        tok.zero_()
        E.sample(logits.data_ptr(), V, B, V, 0, 0, 0, tok.data_ptr(), 0, 0, stream())
        torch.cuda.synchronize()
        assert torch.equal(tok.cpu().long(), logits.argmax(-1).cpu())


@pytest.mark.parametrize("top_k,top_p,V", [(0, 0.7, 32000), (3, 0.9, 32000), (4, 1.0, 128256), (0, 1.0, 5000)])
def test_sample_topk_topp_distribution(E, top_k, top_p, V):
    """Empirical distribution of the device sampler (B rows = independent RNG streams) against
    the host sampler's exact top-k -> softmax -> nucleus distribution."""
    B = 512
    base = torch.full((V,), -30.0)
    idx = [5, 4097, 9000 % V, 20001 % V, V - 2]
    for j, i in enumerate(idx):
        base[i] = 1.0 - 0.5 * j
    logits = base.repeat(B, 1).cuda()
    temp = torch.full((B,), 0.8, device="cuda")
    tk = torch.full((B,), top_k, dtype=torch.int32, device="cuda")
    tp = torch.full((B,), top_p, device="cuda")
    pos = torch.arange(B, dtype=torch.int32, device="cuda")
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    counts = {}
    for rep in range(8):
        E.sample(logits.data_ptr(), V, B, V, temp.data_ptr(), tk.data_ptr(), 77 + rep, tok.data_ptr(), pos.data_ptr(),
                 0, stream(), tp.data_ptr())
        torch.cuda.synchronize()
        for t in tok.cpu().tolist():
            counts[t] = counts.get(t, 0) + 1
    # exact distribution
    l = base.double() / 0.8
    if top_k:
        kth = torch.topk(l, top_k).values[-1]
        l[l < kth] = -float("inf")
    p = torch.softmax(l, 0)
    if top_p < 1.0:
        order = torch.argsort(-p)
        cum = torch.cumsum(p[order], 0)
        before = cum - p[order]
        drop = order[before >= top_p]
        p[drop] = 0
        p /= p.sum()
    n = sum(counts.values())
    allowed = set(torch.nonzero(p > 1e-9).flatten().tolist())
    assert set(counts) <= allowed, (set(counts) - allowed)
    for i in allowed:
        assert abs(counts.get(i, 0) / n - float(p[i])) < 0.04, (i, counts.get(i, 0) / n, float(p[i]))


@pytest.mark.parametrize("t", QTS)
@pytest.mark.parametrize("M", [1, 64, 100])
def test_gemm_mfma(E, t, M):
    N, K = 192, 512
    m, W = qmat(E, t, N, K, seed=11)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.zeros(M, N, device="cuda")
    E.gemm(A.data_ptr(), K, m, M, C.data_ptr(), N, 0, stream())
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.to(torch.bfloat16).float().T
    assert torch.allclose(C.cpu(), ref, atol=2e-3, rtol=2e-3), (C.cpu() - ref).abs().max()
    C2 = C.clone()
    E.gemm(A.data_ptr(), K, m, M, C2.data_ptr(), N, 1, stream())
    torch.cuda.synchronize()
    assert torch.allclose(C2.cpu(), 2 * ref, atol=4e-3, rtol=2e-3)


# ---- prefill path: multi-segment MFMA GEMM with fused epilogues + causal flash attention ----------
@pytest.mark.parametrize("segs", [[(GGMLType.Q4_K, 128), (GGMLType.Q4_K, 64), (GGMLType.Q6_K, 64)],
                                  [(GGMLType.Q8_0, 64)], [(GGMLType.BF16, 192), (GGMLType.Q5_K, 64)],
                                  [(GGMLType.Q4_0, 128), (GGMLType.F16, 128)]])
@pytest.mark.parametrize("M", [1, 100, 300])
@pytest.mark.parametrize("ksplit", [0, 1, 3])
def test_gemm_q_segments(E, segs, M, ksplit):
    K = 512
    mats, refs = zip(*[qmat(E, t, n, K, seed=20 + i) for i, (t, n) in enumerate(segs)])
    W = torch.cat(refs, 0)
    N = W.shape[0]
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.zeros(M, N, device="cuda")
    C.fill_(7.0)  # STORE must overwrite (split-K zeroes first)
    E.gemm_q(A.data_ptr(), K, list(mats), M, C.data_ptr(), 0, N, E.GEPI_STORE, stream(), ksplit)
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.to(torch.bfloat16).float().T
    assert torch.allclose(C.cpu(), ref, atol=2e-3, rtol=2e-3), (C.cpu() - ref).abs().max()
    E.gemm_q(A.data_ptr(), K, list(mats), M, C.data_ptr(), 0, N, E.GEPI_ACCUM, stream(), ksplit)
    torch.cuda.synchronize()
    assert torch.allclose(C.cpu(), 2 * ref, atol=4e-3, rtol=2e-3)


@pytest.mark.parametrize("M,N,K", [(1024, 4096, 256), (200, 2048, 1024)])
def test_gemm_q_large_tiles(E, M, N, K):
    # shapes that select the 128x128 and 64x128 workgroup tiles (XCD-remapped grid)
    m, W = qmat(E, GGMLType.Q4_K, N, K, seed=5)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.zeros(M, N, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_STORE, stream())
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.to(torch.bfloat16).float().T
    assert torch.allclose(C.cpu(), ref, atol=3e-3, rtol=3e-3), (C.cpu() - ref).abs().max()


@pytest.mark.parametrize("M", [7, 130])
def test_gemm_q_swiglu_epilogue(E, M):
    K, F = 256, 192  # interleaved gate/up rows: 2F weight rows -> F bf16 outputs
    m, W = qmat(E, GGMLType.Q4_K, 2 * F, K, seed=8, std=0.2)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    out = torch.zeros(M, F, dtype=torch.bfloat16, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, 0, out.data_ptr(), F, E.GEPI_SWIGLU_BF16, stream())
    torch.cuda.synchronize()
    y = A.float().cpu() @ W.to(torch.bfloat16).float().T
    ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
    assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2), (out.float().cpu() - ref).abs().max()


@pytest.mark.parametrize("H,Hkv,hd", [(32, 8, 128), (32, 4, 64), (8, 8, 64), (16, 8, 128), (64, 8, 128)])
@pytest.mark.parametrize("start,T", [(0, 1), (0, 37), (70, 130), (0, 300)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_attention_prefill_causal(E, H, Hkv, hd, start, T, shuffle):
    max_ctx = 512
    slot, slots = 1, 2
    G = H // Hkv
    kc = (torch.randn(slots, Hkv, max_ctx, hd) * 0.5).to(torch.bfloat16)
    vc = torch.randn(slots, Hkv, max_ctx, hd).to(torch.bfloat16)
    kp, bt = paged_cache(kc, shuffle, seed=5)
    vp, _ = paged_cache(vc, shuffle, seed=5)
    kp, vp = kp.cuda(), vp.cuda()
    bt_dev = bt.cuda() if bt is not None else None
    q = torch.randn(T, H, hd, device="cuda")
    out = torch.zeros(T, H * hd, dtype=torch.bfloat16, device="cuda")
    scale = 1 / math.sqrt(hd)
    E.attn_prefill(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), slot, start, T, H, Hkv, hd, max_ctx, scale,
                   out.data_ptr(), H * hd, stream(), bt_dev.data_ptr() if bt_dev is not None else 0)
    torch.cuda.synchronize()
    L = start + T
    k = kc[slot, :, :L].float().cpu().repeat_interleave(G, 0)  # [H, L, hd]
    v = vc[slot, :, :L].float().cpu().repeat_interleave(G, 0)
    qq = q.cpu().to(torch.bfloat16).float()
    s = torch.einsum("thd,hld->htl", qq, k) * scale
    pos = torch.arange(start, L)[:, None]
    s = s.masked_fill(torch.arange(L)[None, :] > pos, float("-inf"))
    ref = torch.einsum("htl,hld->thd", torch.softmax(s, -1), v).reshape(T, H * hd)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 3e-2, err


# ---- skinny (M <= 64) batched-decode GEMM: weights streamed into MFMA operands ---------------------
@pytest.mark.parametrize("t", QTS)
@pytest.mark.parametrize("M", [2, 16, 33, 64])
@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("epi", ["store", "accum", "swiglu"])
def test_gemm_skinny(E, t, M, ksplit, epi):
    N, K = 256, 2048
    m, W = qmat(E, t, N, K, seed=31, std=0.05)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    y = A.float().cpu() @ W.to(torch.bfloat16).float().T
    if epi == "swiglu":
        out = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
        E.gemm_q(A.data_ptr(), K, [m], M, 0, out.data_ptr(), N // 2, E.GEPI_SWIGLU_BF16, stream(), ksplit)
        torch.cuda.synchronize()
        ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
        assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2), (out.float().cpu() - ref).abs().max()
        return
    C = torch.full((M, N), 3.0, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N,
             E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM, stream(), ksplit)
    torch.cuda.synchronize()
    ref = y if epi == "store" else y + 3.0
    assert torch.allclose(C.cpu(), ref, atol=3e-3, rtol=3e-3), (C.cpu() - ref).abs().max()


@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K])
@pytest.mark.parametrize("M", [8, 40])
@pytest.mark.parametrize("ksplit", [9, 16])
def test_gemm_skinny_wide_split(E, t, M, ksplit):
    # K = 14336 over 9 / 16 slices: the last arriver sums the slabs in batches of 8 (fixed order)
    N, K = 256, 14336
    m, W = qmat(E, t, N, K, seed=61, std=0.01)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.full((M, N), 1.0, device="cuda")
    for _ in range(2):  # the second launch re-uses the re-armed tickets
        C.fill_(1.0)
        E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_ACCUM, stream(), ksplit)
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.to(torch.bfloat16).float().T + 1.0
    assert torch.allclose(C.cpu(), ref, atol=5e-3, rtol=5e-3), (C.cpu() - ref).abs().max()


@pytest.mark.parametrize("M", [4, 32])
def test_gemm_skinny_mixed_segments_long_k(E, M):
    # Q4_K_M-style QKV (Q4_K q/k + Q6_K v, one mixed-format launch) and a K = 14336 down projection with the
    # automatic split: every tile's last arriver reduces the slabs (tickets re-armed per launch)
    K = 4096
    segs = [(GGMLType.Q4_K, 512), (GGMLType.Q4_K, 128), (GGMLType.Q6_K, 128)]
    mats, refs = zip(*[qmat(E, t, n, K, seed=40 + i, std=0.02) for i, (t, n) in enumerate(segs)])
    W = torch.cat(refs, 0)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.zeros(M, W.shape[0], device="cuda")
    for _ in range(2):  # second call re-uses the re-armed tickets
        E.gemm_q(A.data_ptr(), K, list(mats), M, C.data_ptr(), 0, W.shape[0], E.GEPI_STORE, stream())
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.to(torch.bfloat16).float().T
    assert torch.allclose(C.cpu(), ref, atol=3e-3, rtol=3e-3), (C.cpu() - ref).abs().max()
    m, Wd = qmat(E, GGMLType.Q6_K, 256, 14336, seed=50, std=0.01)
    X = torch.randn(M, 14336, device="cuda").to(torch.bfloat16)
    D = torch.ones(M, 256, device="cuda")
    E.gemm_q(X.data_ptr(), 14336, [m], M, D.data_ptr(), 0, 256, E.GEPI_ACCUM, stream())
    torch.cuda.synchronize()
    refd = X.float().cpu() @ Wd.to(torch.bfloat16).float().T + 1.0
    assert torch.allclose(D.cpu(), refd, atol=4e-3, rtol=4e-3), (D.cpu() - refd).abs().max()


@pytest.mark.parametrize("M,N,K", [(512, 1024, 4096), (2048, 512, 1024), (300, 384, 2048)])
@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K])
def test_gemm_big_tiles_match(E, M, N, K, t):
    # 256-row and 128-row workgroup tiles (AIOS_GEMM_BM picks by grid size), partial last M tile
    m, W = qmat(E, t, N, K, seed=60, std=0.02)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    C = torch.zeros(M, N, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_STORE, stream())
    torch.cuda.synchronize()
    ref = A.float() @ W.to(torch.bfloat16).float().cuda().T
    assert torch.allclose(C, ref, atol=3e-3, rtol=3e-3), (C - ref).abs().max()


@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0])
@pytest.mark.parametrize("M,ksplit", [(2, 1), (8, 3), (32, 1), (64, 4), (512, 0)])
def test_gemm_error_vs_unquantized_product(E, t, M, ksplit):
    """The MFMA paths (skinny GEMM for M <= 64: batched decode / short prefill; the dequant-fused
    big GEMM beyond: prefill) against the UNQUANTIZED fp32 product -- exact dequantised weights x
    the fp32 activations before their bf16 rounding -- not against an oracle that rounds W to bf16
    as the kernel does: the bf16 operand rounding (weights and activations, 8 significant bits)
    costs < 0.6 % relative L2 error of the outputs, fp32 accumulation over K = 4096 nothing
    measurable on top."""
    N, K = 256, 4096
    m, W = qmat(E, t, N, K, seed=71, std=0.02)
    x = torch.randn(M, K)
    A = x.to(torch.bfloat16).cuda()
    C = torch.zeros(M, N, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_STORE, stream(), ksplit)
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T
    rel = float((C.cpu().double() - ref).norm() / ref.norm())
    assert rel < 6e-3, rel
    # the same bound row by row: no batch row (M position) is treated differently
    per_row = ((C.cpu().double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    assert per_row < 1e-2, per_row


# ---- the LDS-DMA ring GEMM (gemm_ring.hip): batched decode M = 5..32 on Q4_K / Q6_K / mixed stacks ----
@pytest.mark.parametrize("M", [5, 8, 13, 16, 17, 24, 32])
@pytest.mark.parametrize("segs,K", [([(GGMLType.Q4_K, 384)], 4096), ([(GGMLType.Q6_K, 256)], 14336),
                                    ([(GGMLType.Q4_K, 256), (GGMLType.Q4_K, 128), (GGMLType.Q6_K, 128)], 4096),
                                    ([(GGMLType.Q4_K, 128)], 1024)])
@pytest.mark.parametrize("epi", ["store", "accum"])
def test_gemm_ring_vs_unquantized(E, M, segs, K, epi):
    """Against the UNQUANTIZED fp32 product (exact dequantised weights x the fp32 activations): ring
    slots of one 256-k superblock, the automatic split-K (one dispatch round) reduced by the tile's
    last arriver, padded activation rows (M not a multiple of 16), the mixed-format QKV launch"""
    mats, refs = zip(*[qmat(E, t, n, K, seed=80 + i, std=0.02) for i, (t, n) in enumerate(segs)])
    W = torch.cat(refs, 0)
    N = W.shape[0]
    x = torch.randn(M, K)
    A = x.to(torch.bfloat16).cuda()
    C = torch.full((M, N), 2.0, device="cuda")
    for _ in range(2):  # the second launch re-uses the re-armed tickets
        C.fill_(2.0)
        E.gemm_q(A.data_ptr(), K, list(mats), M, C.data_ptr(), 0, N,
                 E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM, stream())
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T + (0.0 if epi == "store" else 2.0)
    got = C.cpu().double()
    rel = float((got - ref).norm() / (ref - (0.0 if epi == "store" else 2.0)).norm())
    assert rel < 6e-3, rel


@pytest.mark.parametrize("M", [6, 16, 32])
def test_gemm_ring_swiglu(E, M):
    N, K = 512, 4096
    m, W = qmat(E, GGMLType.Q4_K, N, K, seed=91, std=0.05)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    out = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, 0, out.data_ptr(), N // 2, E.GEPI_SWIGLU_BF16, stream())
    torch.cuda.synchronize()
    y = A.float().cpu() @ W.to(torch.bfloat16).float().T
    ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
    assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2), (out.float().cpu() - ref).abs().max()


# ---- the LDS-DMA engine serving B = 2..4 rows from one weight stream (small-batch decode) --------
@pytest.mark.parametrize("t", [GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q5_K, GGMLType.Q8_0])
@pytest.mark.parametrize("K", [4096, 14336])
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("grid", [0, 37])
def test_gemv_lds_batched_store(E, t, K, B, grid):
    N = 1030
    m, W = qmat(E, t, N, K, seed=41, std=0.02)
    x = torch.randn(B, K, device="cuda")
    x[1] *= 4.0  # rows with different norms / scales
    nw = torch.rand(K, device="cuda") + 0.5
    y = torch.full((B, N), 7.0, device="cuda")
    E.gemv([m], B, x.data_ptr(), K, nw.data_ptr(), 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), 0, 1, grid,
           kernel_sel=3)
    torch.cuda.synchronize()
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    ref = xn @ W.T
    assert torch.allclose(y.cpu(), ref, atol=5e-3, rtol=5e-3), (y.cpu() - ref).abs().max()


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("grid", [0, 11])
def test_gemv_lds_batched_swiglu_resid(E, B, grid):
    K, F = 4096, 600
    gu, Wgu = qmat(E, GGMLType.Q4_K, 2 * F, K, seed=42, std=0.02)
    x = torch.randn(B, K, device="cuda") * 3
    nw = torch.rand(K, device="cuda") + 0.5
    out = torch.zeros(B, F, device="cuda")
    E.gemv([gu], B, x.data_ptr(), K, nw.data_ptr(), 1e-5, out.data_ptr(), F, E.EPI_SWIGLU, stream(), 0, 1, grid,
           kernel_sel=3)
    torch.cuda.synchronize()
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    h = xn @ Wgu.T
    ref = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
    assert torch.allclose(out.cpu(), ref, atol=5e-3, rtol=5e-3), (out.cpu() - ref).abs().max()
    y0 = torch.randn(B, 2 * F, device="cuda")
    y = y0.clone()
    E.gemv([gu], B, x.data_ptr(), K, 0, 1e-5, y.data_ptr(), 2 * F, E.EPI_RESID, stream(), 0, 1, grid, kernel_sel=3)
    torch.cuda.synchronize()
    ref = y0.cpu() + q8_ref(xc) @ Wgu.T
    assert torch.allclose(y.cpu(), ref, atol=5e-3, rtol=5e-3), (y.cpu() - ref).abs().max()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("B", [2, 4])
def test_gemv_lds_batched_qkv(E, mixed, B):
    d, H, Hkv, hd, max_ctx, slots = 2048, 8, 2, 64, 256, 4
    wq, Wq = qmat(E, GGMLType.Q4_K, H * hd, d, seed=44)
    wk, Wk = qmat(E, GGMLType.Q4_K, Hkv * hd, d, seed=45)
    wv, Wv = qmat(E, GGMLType.Q6_K if mixed else GGMLType.Q4_K, Hkv * hd, d, seed=46)
    x = torch.randn(B, d, device="cuda")
    nw = torch.rand(d, device="cuda") + 0.5
    pos = torch.tensor([141, 17, 200, 3][:B], dtype=torch.int32, device="cuda")
    slot = torch.tensor([1, 0, 3, 2][:B], dtype=torch.int32, device="cuda")
    kp, bt = paged_cache(torch.zeros(slots, Hkv, max_ctx, hd, dtype=torch.bfloat16), shuffle=True, seed=6)
    kp, bt = kp.cuda(), bt.cuda()
    vp = torch.zeros_like(kp)
    q = torch.zeros(B, H * hd, device="cuda")
    E.gemv_qkv([wq, wk, wv], B, x.data_ptr(), d, nw.data_ptr(), 1e-5, q.data_ptr(), 0, hd, H, Hkv, max_ctx, 0,
               10000.0, pos.data_ptr(), slot.data_ptr(), kp.data_ptr(), vp.data_ptr(), stream(), 1,
               block_table=bt.data_ptr(), kernel_sel=3)
    torch.cuda.synchronize()
    kc, vc = unpaged(kp, slots, max_ctx, bt), unpaged(vp, slots, max_ctx, bt)
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    for b in range(B):
        pb = pos[b:b + 1].cpu()
        qr = rope_ref((xn[b:b + 1] @ Wq.T).view(1, H, hd), pb, 10000.0)
        kr = rope_ref((xn[b:b + 1] @ Wk.T).view(1, Hkv, hd), pb, 10000.0)
        vr = (xn[b:b + 1] @ Wv.T).view(1, Hkv, hd)
        assert torch.allclose(q[b].cpu().view(1, H, hd), qr, atol=3e-3, rtol=3e-3)
        s, p = int(slot[b]), int(pos[b])
        assert torch.allclose(kc[s, :, p].float().cpu(), kr[0], atol=2e-2, rtol=1e-2)
        assert torch.allclose(vc[s, :, p].float().cpu(), vr[0], atol=2e-2, rtol=1e-2)
    assert int((kc != 0).sum()) == B * Hkv * hd and int((vc != 0).sum()) == B * Hkv * hd


# ---- the prefill GEMM (gemm_pf.hip): LDS-DMA slots, weights dequantised once per workgroup tile ------
PF_TILES = ["256x256", "128x256", "64x256", "256x128", "128x128", "64x128"]
PF_SEGS = {
    "q4k": [(GGMLType.Q4_K, 512)],
    "q6k": [(GGMLType.Q6_K, 512)],
    "mixed": [(GGMLType.Q4_K, 256), (GGMLType.Q4_K, 256), (GGMLType.Q6_K, 256)],  # Q4_K_M QKV stack
    "bf16": [(GGMLType.BF16, 512)],
    # round 6 (verdict r5 missing #4): the Q5_K_M / Q4_0 / Q8_0 recipes' stacks (pf4, and pf8_body for 256 columns)
    "q5k": [(GGMLType.Q5_K, 512)],
    "q5k_mixed": [(GGMLType.Q5_K, 256), (GGMLType.Q5_K, 256), (GGMLType.Q6_K, 256)],  # Q5_K_M QKV stack
    "q4_0": [(GGMLType.Q4_0, 512)],
    "q8_0": [(GGMLType.Q8_0, 512)],
}
_pf_cache = {}


def pf_mats(E, name, K):
    key = (name, K)
    if key not in _pf_cache:
        mats, refs = zip(*[qmat(E, t, n, K, seed=100 + 7 * i + K, std=0.02) for i, (t, n) in enumerate(PF_SEGS[name])])
        _pf_cache[key] = (list(mats), torch.cat(refs, 0))
    return _pf_cache[key]


@pytest.mark.parametrize("tile", PF_TILES)
@pytest.mark.parametrize("fmt", list(PF_SEGS))
@pytest.mark.parametrize("M", [33, 200, 512])
@pytest.mark.parametrize("epi", ["store", "accum"])
def test_gemm_pf_vs_unquantized(E, monkeypatch, tile, fmt, M, epi):
    """Against the UNQUANTIZED fp32 product (exact dequantised weights x the fp32 activations): every
    tile shape, partial last row tile (M = 33, 200), mixed-format segment stacks in one launch."""
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    K = 1024
    mats, W = pf_mats(E, fmt, K)
    N = W.shape[0]
    if N % int(tile.split("x")[1]):
        pytest.skip("tile does not divide N")
    assert E.gemm_pf_plan(mats, M, E.GEPI_STORE, 1)[0] == int(tile.split("x")[0])
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M))
    A = x.to(torch.bfloat16).cuda()
    base = 0.0 if epi == "store" else 2.0
    C = torch.full((M, N), 5.0 if epi == "store" else 2.0, device="cuda")
    E.gemm_q(A.data_ptr(), K, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM,
             stream(), 1)
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T
    got = C.cpu().double() - base
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 6e-3, rel
    per_row = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    assert per_row < 1e-2, per_row


@pytest.mark.parametrize("fmt", ["q4k", "mixed", "bf16", "q5k_mixed", "q8_0"])
@pytest.mark.parametrize("M,S", [(64, 2), (100, 3), (300, 4)])
@pytest.mark.parametrize("epi", ["store", "accum"])
def test_gemm_pf_split_k(E, monkeypatch, fmt, M, S, epi):
    """split-K (gridDim.y slices, fp32 atomic adds; STORE zeroes its target first), K = 4096"""
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", "128x128" if fmt == "q8_0" else "128x256")
    K = 4096
    mats, W = pf_mats(E, fmt, K)
    N = W.shape[0]
    assert E.gemm_pf_plan(mats, M, E.GEPI_ACCUM, S)[2] == S
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(S))
    A = x.to(torch.bfloat16).cuda()
    C = torch.full((M, N), 1.0, device="cuda")
    E.gemm_q(A.data_ptr(), K, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM,
             stream(), S)
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T + (0.0 if epi == "store" else 1.0)
    rel = float((C.cpu().double() - ref).norm() / ref.norm())
    assert rel < 6e-3, rel


@pytest.mark.parametrize("epi", ["store", "accum", "swiglu"])
@pytest.mark.parametrize("tile,N", [("256x256", 16384), ("256x128", 8192)])
@pytest.mark.parametrize("fmt", [GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q8_0])
def test_gemm_pf_tail_split(E, monkeypatch, epi, tile, N, fmt):
    """256-row plan whose last round is at most half full (M = 1280: 320 tiles on 256 CUs): the last
    64 tiles run as two 128-row workgroups each (gemm_pft_kernel, 256- and 128-column tiles).  Against the
    unquantized product and bit-identical to the plain launch (same per-element accumulation order)."""
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    M, K = 1280, 512
    m, W = qmat(E, fmt, N, K, seed=131, std=0.02)
    assert E.gemm_pf_plan([m], M, E.GEPI_ACCUM, 1)[:2] == tuple(int(v) for v in tile.split("x"))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(9))
    A = x.to(torch.bfloat16).cuda()
    outs = []
    for tail in ("1", "0"):
        monkeypatch.setenv("AIOS_GEMM_PF_TAIL", tail)
        if epi == "swiglu":
            C = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
            E.gemm_q(A.data_ptr(), K, [m], M, 0, C.data_ptr(), N // 2, E.GEPI_SWIGLU_BF16, stream(), 1)
        else:
            C = torch.full((M, N), 0.5, device="cuda")
            E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM,
                     stream(), 1)
        torch.cuda.synchronize()
        outs.append(C.float().cpu())
    assert torch.equal(outs[0], outs[1])
    y = x.double() @ W.double().T
    if epi == "swiglu":
        ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
        assert torch.allclose(outs[0].double(), ref, atol=2e-2, rtol=2e-2), (outs[0].double() - ref).abs().max()
    else:
        ref = y + (0.0 if epi == "store" else 0.5)
        rel = float((outs[0].double() - ref).norm() / ref.norm())
        assert rel < 6e-3, rel


@pytest.mark.parametrize("segs,M", [([(GGMLType.Q4_K, 8192)], 2100),
                                    ([(GGMLType.Q4_K, 4096), (GGMLType.Q4_K, 1024), (GGMLType.Q6_K, 1024)], 2800),
                                    ([(GGMLType.Q5_K, 4096), (GGMLType.Q5_K, 1024), (GGMLType.Q6_K, 1024)], 2800)])
@pytest.mark.parametrize("epi", ["store", "accum"])
def test_gemm_pf_tail_split_ragged(E, monkeypatch, segs, M, epi):
    """the tail split with M NOT a multiple of 256 (the last row tile partial, its second
    128-row half entirely past M) and on the mixed Q4_K|Q6_K QKV stack (Mistral's 4096 + 1024 + 1024
    rows: the segment branch runs per half; the Q5_K|Q6_K stack takes it on the pf8 body, the Q4_K one
    on pf8c): bit-identical to the plain launch, and against the unquantized product"""
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", "256x256")
    K = 512
    mats, refs = zip(*[qmat(E, t, n, K, seed=140 + i, std=0.02) for i, (t, n) in enumerate(segs)])
    mats, W = list(mats), torch.cat(refs, 0)
    N = W.shape[0]
    tiles = -(-M // 256) * (N // 256)
    assert tiles % E.device_cu_count() <= E.device_cu_count() // 2 < tiles  # (a half-full last round)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M))
    A = x.to(torch.bfloat16).cuda()
    outs = []
    for tail in ("1", "0"):
        monkeypatch.setenv("AIOS_GEMM_PF_TAIL", tail)
        C = torch.full((M, N), 0.25, device="cuda")
        E.gemm_q(A.data_ptr(), K, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM,
                 stream(), 1)
        torch.cuda.synchronize()
        outs.append(C.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = x.double() @ W.double().T + (0.0 if epi == "store" else 0.25)
    rel = float((outs[0].double() - ref).norm() / ref.norm())
    assert rel < 6e-3, rel


@pytest.mark.parametrize("fmt,N,K", [(GGMLType.Q4_K, 512, 4096), (GGMLType.Q6_K, 256, 14336), (GGMLType.BF16, 256, 4096),
                                     (GGMLType.Q5_K, 256, 4096), (GGMLType.Q8_0, 256, 4096), (GGMLType.Q4_0, 256, 4096)])
@pytest.mark.parametrize("split", [0, 4])
def test_gemm_pf_production_shapes_vs_unquantized(E, monkeypatch, fmt, N, K, split):
    """a 2048-token prefill chunk (M = 2048) at the production K of the Mistral
    projections -- K = 4096 (QKV / O / gate-up) and K = 14336 (the Q6_K down) -- through the
    launcher's own plan and a split-K plan, against the unquantized fp64 product"""
    if split:
        monkeypatch.setenv("AIOS_GEMM_PF_SPLIT", str(split))
    M = 2048
    m, W = qmat(E, fmt, N, K, seed=150 + K, std=0.02)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K))
    A = x.to(torch.bfloat16).cuda()
    C = torch.zeros(M, N, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, C.data_ptr(), 0, N, E.GEPI_ACCUM, stream(), split or 0)
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T
    got = C.cpu().double()
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 6e-3, rel
    per_row = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    assert per_row < 1e-2, per_row


@pytest.mark.parametrize("fmt,N,K", [("mixed6144", 6144, 4096), ("q4k", 4096, 4096), ("q6k", 4096, 14336),
                                     ("bf16", 2048, 2048), ("q5k", 4096, 4096), ("q8_0", 4096, 4096),
                                     ("mixed5k", 6144, 4096)])
@pytest.mark.parametrize("tile", ["128x128", "128x256", "256x256"])
@pytest.mark.parametrize("epi", ["store", "accum"])
def test_gemm_pf_stream_k(E, monkeypatch, fmt, N, K, tile, epi):
    """Stream-K (AIOS_GEMM_PF_SPLIT=-1): one workgroup per CU over an equal share of the (tile, K-step)
    iterations, partial tiles added atomically -- the 512-token shapes of Mistral's QKV stack, O and
    Q6_K down, and a bf16 matrix, every body (pf4 128-column, pf8c 256-column K-quant, pf8 bf16),
    against the unquantized fp64 product"""
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    monkeypatch.setenv("AIOS_GEMM_PF_SPLIT", "-1")
    segs = {"mixed6144": [(GGMLType.Q4_K, 4096), (GGMLType.Q4_K, 1024), (GGMLType.Q6_K, 1024)],
            "q4k": [(GGMLType.Q4_K, N)], "q6k": [(GGMLType.Q6_K, N)], "bf16": [(GGMLType.BF16, N)],
            "q5k": [(GGMLType.Q5_K, N)], "q8_0": [(GGMLType.Q8_0, N)],
            "mixed5k": [(GGMLType.Q5_K, 4096), (GGMLType.Q5_K, 1024), (GGMLType.Q6_K, 1024)]}[fmt]
    key = ("sk", fmt, K)
    if key not in _pf_cache:
        mats, refs = zip(*[qmat(E, t, n, K, seed=170 + i, std=0.02) for i, (t, n) in enumerate(segs)])
        _pf_cache[key] = (list(mats), torch.cat(refs, 0))
    mats, W = _pf_cache[key]
    M = 512
    if E.gemm_pf_plan(mats, M, E.GEPI_ACCUM, 0)[2] != -1:
        pytest.skip("stream-K not eligible for this tile / shape")
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K + N))
    A = x.to(torch.bfloat16).cuda()
    C = torch.full((M, N), 0.5, device="cuda")
    E.gemm_q(A.data_ptr(), K, mats, M, C.data_ptr(), 0, N, E.GEPI_STORE if epi == "store" else E.GEPI_ACCUM, stream(), 0)
    torch.cuda.synchronize()
    ref = x.double() @ W.double().T + (0.0 if epi == "store" else 0.5)
    got = C.cpu().double()
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 6e-3, rel
    per_row = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    assert per_row < 1e-2, per_row


@pytest.mark.parametrize("tile", ["256x256", "128x256", "64x128"])
@pytest.mark.parametrize("M", [40, 300])
def test_gemm_pf_swiglu(E, monkeypatch, tile, M):
    monkeypatch.setenv("AIOS_GEMM_PF_TILE", tile)
    K, N = 1024, 512
    m, W = qmat(E, GGMLType.Q4_K, N, K, seed=93, std=0.05)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    out = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
    E.gemm_q(A.data_ptr(), K, [m], M, 0, out.data_ptr(), N // 2, E.GEPI_SWIGLU_BF16, stream())
    torch.cuda.synchronize()
    y = A.float().cpu() @ W.to(torch.bfloat16).float().T
    ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
    assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2), (out.float().cpu() - ref).abs().max()


def test_gemm_pf_serves_prefill_shapes(E):
    """The default plan takes every prefill launch of the Q4_K_M / Q5_K_M / Q4_0 / Q8_0 / bf16 stacks (no
    fallback kernel)."""
    for fmt in PF_SEGS:
        mats, _ = pf_mats(E, fmt, 1024)
        for M in (33, 64, 128, 512, 2048):
            bm, bn, s = E.gemm_pf_plan(mats, M, E.GEPI_ACCUM, 0)
            assert bm in (64, 128, 256) and bn in (128, 256) and (s >= 1 or s == -1), (fmt, M, bm, bn, s)
