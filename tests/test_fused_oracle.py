"""The float64 oracle of the fused-epilogue tests (tests/fused_oracle.py) against the references the
suite already trusts.  CPU only: this is the part of the oracle that can be checked without a GPU."""
import pytest
import torch

import fused_oracle as O
from test_kernels_gpu import KVB, paged_cache, rope_ref, unpaged


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("neox", [False, True])
def test_rope_pairs_matches_rope_ref(hd, neox):
    """rope_ref rounds the frequency and the angle pos * freq to fp32 (relative 2^-24 each, so the angle
    is off by <= pos * 2^-23) and its cos / sin and three fp32 operations add 2^-24-sized terms; the
    table is exact angles rounded once.  Per element: <= (pos * 2^-23 + 2^-21) * (|v0| + |v1|)."""
    theta, max_ctx = 10000.0, 512
    g = torch.Generator().manual_seed(3)
    pos = torch.tensor([0, 1, 127, 128, 300, 511])
    x = torch.randn(len(pos), 3, hd, generator=g)
    got = O.rope_pairs(x, pos, O.rope_table(max_ctx, hd, theta), neox)
    ref = rope_ref(x, pos, theta, neox).double()
    bound = (pos.double() * 2.0 ** -23 + 2.0 ** -21)[:, None, None] * O.rope_pair_mag(x, neox)
    assert bool(((got - ref).abs() <= bound).all()), ((got - ref).abs() / bound).max()
    # position 0 is the identity, exactly
    assert torch.equal(got[0], x[0].double())


def test_rope_pairs_matches_reference_model():
    from aios_amd.models.config import get_preset
    from aios_amd.models.reference import ReferenceModel

    cfg = get_preset("test-mistral-shape")
    rm = ReferenceModel.__new__(ReferenceModel)  # _rope reads cfg only
    rm.cfg = cfg
    hd = 64
    pos = torch.tensor([0, 5, 127, 128])
    x = torch.randn(len(pos), 2, hd, generator=torch.Generator().manual_seed(4))
    from aios_amd.models.reference import ROPE_NEOX

    neox = cfg.rope_mode == ROPE_NEOX
    got = O.rope_pairs(x, pos, O.rope_table(256, hd, cfg.rope_theta), neox)
    ref = rm._rope(x, pos).double()
    bound = (pos.double() * 2.0 ** -23 + 2.0 ** -21)[:, None, None] * O.rope_pair_mag(x, neox)
    assert bool(((got - ref).abs() <= bound).all())


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("Hkv,hd", [(2, 64), (1, 128)])
def test_kv_targets_matches_paged_cache(shuffle, Hkv, hd):
    """Scatter row tags through kv_targets into a flat pool; unpaged() must find tag t at the logical
    (slot[t], head, pos[t]) and nothing anywhere else."""
    S, C = 6, 512
    pos = torch.tensor([0, 127, 128, 511, 300, 128])
    slot = torch.tensor([4, 1, 5, 2, 2, 0])
    phys0, bt = paged_cache(torch.zeros(S, Hkv, C, hd), shuffle=shuffle, seed=9)
    off = O.kv_targets(pos, slot, bt, Hkv, hd, C)
    assert off.shape == (len(pos), Hkv, hd) and off.unique().numel() == off.numel()
    pool = torch.zeros(phys0.numel())
    tag = (torch.arange(len(pos))[:, None, None] * 1000 + torch.arange(Hkv)[None, :, None] * 200 +
           torch.arange(hd)[None, None, :] + 1).float()
    pool[off.reshape(-1)] = tag.reshape(-1)
    logical = unpaged(pool.view_as(phys0), S, C, bt)
    expect = torch.zeros(S, Hkv, C, hd)
    for t in range(len(pos)):
        expect[slot[t], :, pos[t]] = tag[t]
    assert torch.equal(logical, expect)


def test_kv_targets_null_slot_is_slot_zero():
    pos = torch.tensor([3, 130])
    off = O.kv_targets(pos, None, None, 2, 64, 256)
    assert torch.equal(off, O.kv_targets(pos, torch.zeros(2, dtype=torch.long), None, 2, 64, 256))
    assert int(off[1, 0, 0]) == ((1 * 2 + 0) * KVB + 2) * 64


def test_split_norm_parts_and_helpers():
    x = torch.randn(5, 512, generator=torch.Generator().manual_seed(1))
    p = O.split_norm_parts(x, 128)
    assert p.shape == (5, 4)
    assert torch.allclose(p.sum(-1), (x.double() ** 2).sum(-1), rtol=1e-14, atol=0)
    assert torch.equal(p[:, 1], (x[:, 128:256].double() ** 2).sum(-1))
    s = O.rsqrt_scale(p, 512, 1e-5)
    assert torch.allclose(s, torch.rsqrt((x.double() ** 2).mean(-1) + 1e-5), rtol=1e-14, atol=0)
    # bf16 step distance: the rounded value itself, its neighbours, across zero and across a binade
    v = torch.tensor([1.0, 1.0078125, -1.0, 0.0, 2.0])
    b = v.to(torch.bfloat16)
    assert O.bf16_steps(b, v.double()).tolist() == [0, 0, 0, 0, 0]
    nxt = torch.tensor([1.0078125, 1.015625, -1.0078125, 9.183549615799121e-41, 1.9921875]).to(torch.bfloat16)
    assert O.bf16_steps(nxt, v.double()).tolist() == [1, 1, 1, 1, 1]
