"""The one-workgroup-per-CU batch-1 GEMVs (kernel_sel 2 register kernel, 3 LDS-DMA engine) reading
their work split from the cached host-built descriptors (csrc/gemv_desc.h): same fp32 references and
tolerances as test_kernels_gpu.test_gemv_b1_cu_store / _qkv, every case launched twice (the second
launch hits the cache and must reproduce the first bit for bit)."""
import pytest
import torch

from aios_amd.gguf.quants import GGMLType
from aios_amd.runtime import native

pytestmark = pytest.mark.gpu

Q4, Q6 = GGMLType.Q4_K, GGMLType.Q6_K
_mats = {}


@pytest.fixture(scope="module")
def E():
    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def q8_ref(x):
    from aios_amd.models.reference import ReferenceModel

    return ReferenceModel.q8(x)


def qmat(E, t, rows, cols, seed, std=0.02):
    """(device matrix, dequantised fp32 reference), built once per shape and shared, never modified"""
    import numpy as np

    from aios_amd.gguf.quants import dequantize, quantize

    key = (int(t), rows, cols, seed)
    if key not in _mats:
        w = np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32) * std
        raw = quantize(w, t)
        _mats[key] = (E.QMatrix(int(t), rows, cols, raw), torch.from_numpy(dequantize(raw, t).reshape(rows, cols).copy()))
    return _mats[key]


def store_case(E, t, N, K, grid, sel, seed=31):
    m, W = qmat(E, t, N, K, seed)
    gen = torch.Generator().manual_seed(1000 + K)
    x = torch.randn(1, K, generator=gen).cuda()
    nw = (torch.rand(K, generator=gen) + 0.5).cuda()
    outs = []
    for _ in range(2):
        y = torch.zeros(1, N, device="cuda")
        E.gemv([m], 1, x.data_ptr(), K, nw.data_ptr(), 1e-5, y.data_ptr(), N, E.EPI_STORE, stream(), 0, 1, grid,
               kernel_sel=sel)
        torch.cuda.synchronize()
        outs.append(y.cpu())
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    return outs, xn @ W.T


@pytest.mark.parametrize("t", [Q4, Q6])
@pytest.mark.parametrize("K", [2304, 4096])
@pytest.mark.parametrize("grid", [0, 1, 3, 37])
@pytest.mark.parametrize("sel", [2, 3])
def test_desc_store(E, t, K, grid, sel):
    (y0, y1), ref = store_case(E, t, 1030, K, grid, sel)
    assert torch.allclose(y0, ref, atol=5e-3, rtol=5e-3), (y0 - ref).abs().max()
    assert torch.equal(y0, y1)


@pytest.mark.parametrize("t", [Q4, Q6])
@pytest.mark.parametrize("sel", [2, 3])
def test_desc_down_shape(E, t, sel):
    # K = 14336: 7 groups per row, rows straddle consumer waves and ring slots.  The row sums of this
    # shape are LDS float atomics whose order may vary between launches: both launches are held to the
    # reference, not to each other
    (y0, y1), ref = store_case(E, t, 64, 14336, 0, sel, seed=41)
    assert torch.allclose(y0, ref, atol=5e-3, rtol=5e-3), (y0 - ref).abs().max()
    assert torch.allclose(y1, ref, atol=5e-3, rtol=5e-3), (y1 - ref).abs().max()


def test_desc_key_has_grid(E):
    # the same matrix launched with two grids, alternating: a cache keyed without the grid would hand
    # the second launch the first one's records (other rows per workgroup, other record count)
    res = [store_case(E, Q4, 1030, 4096, grid, 3) for grid in (3, 37, 3, 37)]
    for (y0, y1), ref in res:
        assert torch.allclose(y0, ref, atol=5e-3, rtol=5e-3), (y0 - ref).abs().max()
        assert torch.equal(y0, y1)
    assert torch.equal(res[0][0][0], res[2][0][0]) and torch.equal(res[1][0][0], res[3][0][0])


@pytest.mark.parametrize("grid", [0, 1, 5])
@pytest.mark.parametrize("sel", [2, 3])
def test_desc_qkv_mixed(E, grid, sel):
    from test_kernels_gpu import paged_cache, rope_ref, unpaged

    d, H, Hkv, hd, max_ctx, slots = 2048, 8, 2, 64, 256, 2
    wq, Wq = qmat(E, Q4, H * hd, d, 34, std=0.05)
    wk, Wk = qmat(E, Q4, Hkv * hd, d, 35, std=0.05)
    wv, Wv = qmat(E, Q6, Hkv * hd, d, 36, std=0.05)
    gen = torch.Generator().manual_seed(37)
    x = torch.randn(1, d, generator=gen).cuda()
    nw = (torch.rand(d, generator=gen) + 0.5).cuda()
    pos = torch.tensor([141], dtype=torch.int32, device="cuda")
    slot = torch.tensor([1], dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(2):
        kp, bt = paged_cache(torch.zeros(slots, Hkv, max_ctx, hd, dtype=torch.bfloat16), shuffle=True, seed=4)
        kp, bt = kp.cuda(), bt.cuda()
        vp = torch.zeros_like(kp)
        q = torch.zeros(1, H * hd, device="cuda")
        E.gemv_qkv([wq, wk, wv], 1, x.data_ptr(), d, nw.data_ptr(), 1e-5, q.data_ptr(), 0, hd, H, Hkv, max_ctx, 0,
                   10000.0, pos.data_ptr(), slot.data_ptr(), kp.data_ptr(), vp.data_ptr(), stream(), 1,
                   block_table=bt.data_ptr(), rope_cs=0, tune_grid=grid, kernel_sel=sel)
        torch.cuda.synchronize()
        outs.append((q.cpu(), unpaged(kp, slots, max_ctx, bt).cpu(), unpaged(vp, slots, max_ctx, bt).cpu()))
    (q0, kc, vc), (q1, kc1, vc1) = outs
    xc = x.cpu()
    xn = q8_ref(xc * nw.cpu()) * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    qr = rope_ref((xn @ Wq.T).view(1, H, hd), pos.cpu(), 10000.0)
    kr = rope_ref((xn @ Wk.T).view(1, Hkv, hd), pos.cpu(), 10000.0)
    vr = (xn @ Wv.T).view(1, Hkv, hd)
    assert torch.allclose(q0.view(1, H, hd), qr, atol=5e-3, rtol=5e-3), (q0.view(1, H, hd) - qr).abs().max()
    assert torch.allclose(kc[1, :, 141].float(), kr[0], atol=2e-2, rtol=1e-2)
    assert torch.allclose(vc[1, :, 141].float(), vr[0], atol=2e-2, rtol=1e-2)
    assert int((kc != 0).sum()) == Hkv * hd and int((vc != 0).sum()) == Hkv * hd
    assert torch.equal(q0, q1) and torch.equal(kc, kc1) and torch.equal(vc, vc1)
