"""KV snapshot rule in numpy (csrc/ops.h KvSnapArgs): a paged pool, a block table, pack and unpack.

A pool is uint8 [layer][K, V][block][kv_head][KV_BLOCK][head_dim * elem_bytes]; block `n_blocks` (the last) is the
null block.  A table is int [slots][max_blocks].  The payload of a slot's first n positions is
[layer][K, V][kv_head][token][head_dim * elem_bytes], what Engine.kv_read returns.
"""
import numpy as np

KV_BLOCK = 128


def payload_shape(n_layers, n_kv_heads, n, head_dim, elem_bytes):
    return (n_layers, 2, n_kv_heads, n, head_dim * elem_bytes)


def pack(pool, table, slot, n):
    """payload of positions [0, n) of `slot`; reads only the live rows of the row's first ceil(n / KV_BLOCK) blocks"""
    L, _, _, H, _, rb = pool.shape
    out = np.zeros((L, 2, H, n, rb), np.uint8)
    for j in range((n + KV_BLOCK - 1) // KV_BLOCK):
        rows = min(KV_BLOCK, n - j * KV_BLOCK)
        b = int(table[slot, j])
        out[:, :, :, j * KV_BLOCK:j * KV_BLOCK + rows] = pool[:, :, b, :, :rows]
    return out


def unpack(pool, table, slot, payload):
    """a copy of `pool` with the payload written to positions [0, n) of `slot`; nothing else changes"""
    n = payload.shape[3]
    out = pool.copy()
    for j in range((n + KV_BLOCK - 1) // KV_BLOCK):
        rows = min(KV_BLOCK, n - j * KV_BLOCK)
        b = int(table[slot, j])
        out[:, :, b, :, :rows] = payload[:, :, :, j * KV_BLOCK:j * KV_BLOCK + rows]
    return out


def touched_mask(pool_shape, table, slot, n):
    """bool array of pool_shape: the bytes pack reads and unpack writes"""
    m = np.zeros(pool_shape, bool)
    for j in range((n + KV_BLOCK - 1) // KV_BLOCK):
        rows = min(KV_BLOCK, n - j * KV_BLOCK)
        m[:, :, int(table[slot, j]), :, :rows] = True
    return m


def poison_pool(n_layers, n_blocks, n_kv_heads, head_dim, elem_bytes, seed):
    """a pool (null block included) where every byte depends on its address: equal bytes at two addresses are a
    1-in-256 accident per byte, a whole misplaced row never goes unseen"""
    shape = (n_layers, 2, n_blocks + 1, n_kv_heads, KV_BLOCK, head_dim * elem_bytes)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8)
