"""csrc/kernels/kv_snapshot.hip through the raw binding, against tests/kv_snapshot_oracle.py, bit for bit.

2 layers; head_dim 64 and 128; 1 and 2 KV heads; element size 2 and 1; n in {1, 127, 128, 129, 300}.  The pool holds
7 blocks and the null block; the slot's table row is a permutation of physical blocks placed among another slot's,
and every byte of the pool is random (kv_snapshot_oracle.poison_pool), so a row taken from a dead row of the last
block, a foreign block or the null block shows.  Pack must equal the oracle.  Unpack is checked on a whole-pool copy
before and after: the target rows equal the payload and every other byte of the pool is unchanged.
"""
import numpy as np
import pytest

import kv_snapshot_oracle as O

pytestmark = pytest.mark.gpu

LAYERS, BLOCKS, MAXB = 2, 7, 4
NS = [1, 127, 128, 129, 300]
# slot 1 is the one under test: a permutation, among slot 0's and slot 2's blocks; unmapped entries name the null block
TABLE = np.array([[1, 6, BLOCKS, BLOCKS], [5, 0, 3, BLOCKS], [2, 4, BLOCKS, BLOCKS]], np.int32)
SLOT = 1


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.load(build_if_missing=False)


def run(E, torch, pool_np, buf, n, hd, heads, es, unpack, table=TABLE, slot=SLOT):
    """one launch over both layers on a device copy of the pool; returns the pool afterwards (numpy)"""
    pool = torch.from_numpy(pool_np).cuda()  # [layer][K, V][block][head][128][hd * es]
    k, v = pool[:, 0].contiguous(), pool[:, 1].contiguous()
    tab = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    layer_bytes = (BLOCKS + 1) * heads * O.KV_BLOCK * hd * es
    assert k[0].numel() == layer_bytes
    E.kv_snapshot(k.data_ptr(), v.data_ptr(), layer_bytes, buf.data_ptr(), tab.data_ptr(), MAXB, BLOCKS, slot, n,
                  LAYERS, heads, hd, es, unpack, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return torch.stack([k, v], 1).cpu().numpy()


@pytest.mark.parametrize("es", [2, 1], ids=["bf16", "fp8"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("hd", [64, 128])
def test_pack_and_unpack_match_the_oracle(E, hd, heads, es):
    import torch

    pool = O.poison_pool(LAYERS, BLOCKS, heads, hd, es, seed=hd + heads + es)
    for n in NS:
        shape = O.payload_shape(LAYERS, heads, n, hd, es)
        # pack: a poisoned buffer with a guard behind it
        buf = torch.full((int(np.prod(shape)) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        after = run(E, torch, pool, buf, n, hd, heads, es, False)
        got = buf.cpu().numpy()
        assert (got[-64:] == 0xA5).all(), f"n={n}: pack wrote behind the payload"
        assert (got[:-64].reshape(shape) == O.pack(pool, TABLE, SLOT, n)).all(), f"n={n}: pack differs from the oracle"
        assert (after == pool).all(), f"n={n}: pack changed the pool"

        # unpack: another payload into the same rows, whole pool compared
        payload = np.random.default_rng(1000 + n).integers(0, 256, shape, dtype=np.uint8)
        buf = torch.from_numpy(payload.reshape(-1)).cuda()
        after = run(E, torch, pool, buf, n, hd, heads, es, True)
        want = O.unpack(pool, TABLE, SLOT, payload)
        m = O.touched_mask(pool.shape, TABLE, SLOT, n)
        assert (after[m] == want[m]).all(), f"n={n}: the target rows differ from the payload"
        assert (after[~m] == pool[~m]).all(), f"n={n}: unpack changed a byte outside the slot's live rows"
        assert (buf.cpu().numpy().reshape(shape) == payload).all()


def test_one_layer_of_two_and_table_entries_outside_the_pool(E):
    import torch

    hd, heads, es, n = 64, 2, 2, 200
    pool = O.poison_pool(LAYERS, BLOCKS, heads, hd, es, seed=9)
    shape1 = O.payload_shape(1, heads, n, hd, es)
    # layer0 = 1, one layer: the engine's per-layer launch
    pool_t = torch.from_numpy(pool).cuda()
    k, v = pool_t[:, 0].contiguous(), pool_t[:, 1].contiguous()
    tab = torch.from_numpy(TABLE).cuda()
    buf = torch.zeros(int(np.prod(shape1)), dtype=torch.uint8, device="cuda")
    E.kv_snapshot(k.data_ptr(), v.data_ptr(), k[0].numel(), buf.data_ptr(), tab.data_ptr(), MAXB, BLOCKS, SLOT, n, 1, heads,
                  hd, es, False, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().reshape(shape1) == O.pack(pool, TABLE, SLOT, n)[1:2]).all()

    # an unmapped entry (the null block) and an entry outside the pool: unpack writes neither, pack reads the null
    # block (Engine.kv_read's rule) and skips the other
    table = TABLE.copy()
    table[SLOT, 0], table[SLOT, 1] = BLOCKS, BLOCKS + 5
    shape = O.payload_shape(LAYERS, heads, n, hd, es)
    payload = np.random.default_rng(4).integers(0, 256, shape, dtype=np.uint8)
    after = run(E, torch, pool, torch.from_numpy(payload.reshape(-1)).cuda(), n, hd, heads, es, True, table=table)
    assert (after == pool).all()
    buf = torch.full((int(np.prod(shape)),), 0xA5, dtype=torch.uint8, device="cuda")
    run(E, torch, pool, buf, n, hd, heads, es, False, table=table)
    got = buf.cpu().numpy().reshape(shape)
    assert (got[:, :, :, :128] == pool[:, :, BLOCKS, :, :128]).all() and (got[:, :, :, 128:] == 0xA5).all()


def test_launch_refusals(E):
    import torch

    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    tab = torch.from_numpy(TABLE).cuda()
    lb = (BLOCKS + 1) * 2 * O.KV_BLOCK * 64 * 2

    def call(**kw):
        a = dict(k_cache=buf.data_ptr(), v_cache=buf.data_ptr(), layer_bytes=lb, buf=buf.data_ptr(),
                 block_table=tab.data_ptr(), max_blocks=MAXB, n_blocks=BLOCKS, slot=SLOT, n_tokens=1, n_layers=1,
                 n_kv_heads=2, head_dim=64, elem_bytes=2, unpack=False)
        a.update(kw)
        E.kv_snapshot(**a)

    for kw, msg in [(dict(n_tokens=0), "n_tokens"), (dict(n_tokens=MAXB * 128 + 1), "n_tokens"),
                    (dict(elem_bytes=4), "element size"), (dict(head_dim=60), "head_dim"), (dict(buf=0), "null"),
                    (dict(buf=buf.data_ptr() + 8), "aligned"), (dict(layer_bytes=lb - 16), "layer stride"),
                    (dict(slot=-1), "bad shape")]:
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
