"""The float64 attention oracle (tests/attention_oracle.py) against torch.softmax attention, and the
conditions its input families promise -- asserted on the reference alone, for every family, layout and
number format tests/test_attention_gpu.py runs.  CPU only."""
import math

import pytest
import torch

import attention_oracle as O


@pytest.mark.parametrize("H,Hkv,hd", [(4, 4, 64), (12, 6, 128), (20, 4, 128)])
@pytest.mark.parametrize("p_bf16", [False, True])
def test_attn_ref_matches_torch_softmax(H, Hkv, hd, p_bf16):
    """Random input, a causal and a ragged mask: attn_ref against float64 torch.softmax attention over
    the same bf16-rounded q (both sides).  Unrounded P: float64 agreement.  bf16 P: each term moves by
    at most 2^-8 relative (bf16's unit roundoff), so the output by at most 2^-8 * mag."""
    g = torch.Generator().manual_seed(1)
    R, L, G = 7, 200, H // Hkv
    q = torch.randn(R, H, hd, generator=g)
    k = (torch.randn(Hkv, L, hd, generator=g) * 0.5).to(torch.bfloat16).float()
    v = torch.randn(Hkv, L, hd, generator=g).to(torch.bfloat16).float()
    scale = 1 / math.sqrt(hd)
    for visible in (torch.arange(L)[None, :] <= (L - R + torch.arange(R))[:, None],
                    torch.arange(L)[None, :] < torch.tensor([1, 2, 64, 65, 128, 199, 200])[:, None]):
        out, mag = O.attn_ref(q, k, v, visible, scale, p_bf16=p_bf16)
        qs = (q * (torch.tensor(scale) * torch.tensor(O.LOG2E))).to(torch.bfloat16).double()
        s = torch.einsum("rhd,hld->rhl", qs, k.double().repeat_interleave(G, 0)) * math.log(2.0)
        att = torch.softmax(s.masked_fill(~visible[:, None, :], float("-inf")), -1)
        ref = torch.einsum("rhl,hld->rhd", att, v.double().repeat_interleave(G, 0))
        refmag = torch.einsum("rhl,hld->rhd", att, v.double().abs().repeat_interleave(G, 0))
        assert torch.allclose(mag, refmag, rtol=1e-12, atol=0)
        bound = (2.0 ** -8 if p_bf16 else 1e-12) * refmag
        assert bool(((out - ref).abs() <= bound).all())
        if p_bf16:
            assert (out - ref).abs().max() > 0  # the flag does something


def test_attn_ref_fp8_scales():
    """k_scale folds into q and divides out of K; v_scale is part of the value: the fp8 form of a case
    equals the plain form over the dequantised values up to q's bf16 rounding point (a power-of-two
    scale moves no rounding at all)."""
    g = torch.Generator().manual_seed(2)
    q = torch.randn(3, 8, 64, generator=g)
    codes_k = torch.randn(2, 50, 64, generator=g).to(torch.float8_e4m3fn).float()
    codes_v = torch.randn(2, 50, 64, generator=g).to(torch.float8_e4m3fn).float()
    vis = torch.ones(3, 50, dtype=torch.bool)
    sk, sv = 2.0 ** -5, 0.37
    a, _ = O.attn_ref(q, codes_k * sk, codes_v * sv, vis, 0.125, k_scale=sk, v_scale=sv)
    b, _ = O.attn_ref(q * sk, codes_k, codes_v * sv, vis, 0.125)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-14)


def test_paged_roundtrip_and_live_mask():
    x = torch.randn(3, 2, 384, 8, generator=torch.Generator().manual_seed(3))
    for shuffle in (False, True):
        phys, bt = O.paged(x, shuffle, seed=4)
        assert torch.equal(O.unpaged(phys, 3, 384, bt), x)
        live = O.live_mask([0, 129, 384], 384, bt)
        tag = O.unpaged(live[:, None, :, None].expand(-1, 2, -1, 8).contiguous(), 3, 384, bt)
        want = torch.arange(384)[None, :] < torch.tensor([0, 129, 384])[:, None]
        assert torch.equal(tag, want[:, None, :, None].expand(3, 2, 384, 8))


@pytest.mark.parametrize("fp8", [False, True])
def test_poison_and_decoy_keep_live_bits(fp8):
    c = O.decode_case("peaked-last", 64, 4, 4, [1, 129, 200], 256, fp8, seed=5)
    for shuffle in (False, True):
        kp, vp, bt, live = O.pools(c, shuffle, seed=6, mode="clean")
        m = live[:, None, :, None].expand(kp.shape)
        bits = (lambda t: t) if fp8 else (lambda t: t.view(torch.int16))
        for clean, bad in ((kp, O.poison(kp, live)), (vp, O.poison(vp, live))):
            assert torch.equal(bits(bad)[m], bits(clean)[m])
            dead = bad[~m].view(torch.float8_e4m3fn).float() if fp8 else bad[~m].float()
            assert dead.numel() > 0 and not bool(torch.isfinite(dead).any())
            if not fp8:  # NaN and both infinities all occur
                assert bool(dead.isnan().any()) and bool((dead == math.inf).any()) and bool((dead == -math.inf).any())
        # the logical view: exactly the first n_live keys of every slot survive
        lg = O.unpaged(O.poison(kp, live), 4, 256, bt)
        lg = lg.view(torch.float8_e4m3fn).float() if fp8 else lg.float()
        fin = torch.isfinite(lg).all(-1).all(1)  # [S, C]
        assert torch.equal(fin, torch.arange(256)[None, :] < torch.tensor(c.n_live)[:, None])
        dk, dv = O.decoy(kp, vp, live, c.kraw[1, :, 0], 100.0 if not fp8 else 448.0)
        assert torch.equal(bits(dk)[m], bits(kp)[m]) and torch.equal(bits(dv)[m], bits(vp)[m])
        dvf = dv[~m].view(torch.float8_e4m3fn).float() if fp8 else dv[~m].float()
        assert bool((dvf == (448.0 if fp8 else 100.0)).all())
        assert torch.equal(bits(dk)[~m], bits(c.kraw[1, :, 0])[None, :, None, :].expand(kp.shape)[~m])


def _probs(c, rows, s, L):
    raw = O.attn_scores(c.q[rows], c.k(s, L), c.scale, c.sk)
    masked = raw.masked_fill(~c.visible[rows][:, None, :L], float("-inf"))
    return raw, torch.softmax(masked * math.log(2.0), -1)


DECODE_SHAPES = [lay + lc + (f8,) for lay in O.DECODE_LAYOUTS for lc in O.DECODE_LENS for f8 in (False, True)]
DECODE_SHAPES += [w + (False,) for w in O.DECODE_WIDE] + [O.DECODE_KNOB + (False,)]  # (bf16 only on the GPU too)


@pytest.mark.parametrize("hd,H,Hkv,lens,max_ctx,fp8", DECODE_SHAPES)
def test_decode_families_hold_their_conditions(hd, H, Hkv, lens, max_ctx, fp8):
    for family in O.DECODE_FAMILIES:
        c = O.decode_case(family, hd, H, Hkv, lens, max_ctx, fp8, seed=7)
        for b, n in enumerate(lens):
            raw, p = _probs(c, slice(b, b + 1), c.slot[b], n)
            assert float(raw.abs().max()) <= 128.0
            if family.startswith("peaked"):
                # the needle holds >= 0.99 of the mass
                mass = p[0].gather(-1, c.needle[b][:, None])[:, 0]
                assert float(mass.min()) >= 0.99, (family, b, float(mass.min()))
                continue
            # per-128-key-pass maximum of the live keys, every head
            pm = torch.stack([raw[0, :, j:j + O.KVB].max(-1).values for j in range(0, n, O.KVB)], -1)  # [H, passes]
            d = pm[:, 1:] - pm[:, :-1]
            if family == "ascending":
                assert bool((d > 0).all())
            elif family == "descending":
                assert bool((d < 0).all())
            else:  # flat but for one key of the last pass, which then holds all the mass
                j = c.spike[c.slot[b]]
                assert j // O.KVB == (n - 1) // O.KVB and j < n
                others = torch.cat([raw[0, :, :j], raw[0, :, j + 1:]], -1)
                if others.numel():
                    assert float((others.max(-1).values - others.min(-1).values).max()) < 0.5
                    assert float((raw[0, :, j] - others.max(-1).values).min()) > 30
                assert float(p[0, :, j].min()) >= 0.99


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("start,T", O.PREFILL_CASES + [(0, 70), (0, 150), (70, 80)])
@pytest.mark.parametrize("H,Hkv,hd", O.PREFILL_LAYOUTS)
def test_prefill_families_hold_their_conditions(H, Hkv, hd, start, T, fp8):
    L = start + T
    c = O.prefill_case("peaked", H, Hkv, hd, start, T, fp8, seed=8)
    # scores over one key more than is live: the first masked key of the last row (when the context has it)
    Lx = min(L + 1, c.max_ctx)
    raw = O.attn_scores(c.q, c.k(1, Lx), c.scale, c.sk)
    assert float(raw.abs().max()) <= 128.0
    _, p = _probs(c, slice(0, T), 1, L)
    diag = (start + torch.arange(T))[:, None, None].expand(T, H, 1)
    assert float(p.gather(-1, diag).min()) >= 0.99
    rows = torch.arange(T)[start + torch.arange(T) + 1 < Lx]
    gap = raw[rows].gather(-1, diag[rows] + 1) - raw[rows].gather(-1, diag[rows])
    assert rows.numel() == 0 or float(gap.min()) >= 8.0
    c = O.prefill_case("ascending", H, Hkv, hd, start, T, fp8, seed=8)
    raw = O.attn_scores(c.q[-1:], c.k(1, L), c.scale, c.sk)
    assert float(raw.abs().max()) <= 128.0
    # per 64-key tile of the last row (hence per 128-key pass too)
    pm = torch.stack([raw[0, :, j:j + 64].max(-1).values for j in range(0, L, 64)], -1)
    assert bool((pm[:, 1:] - pm[:, :-1] > 0).all())
