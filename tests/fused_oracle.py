"""Plain float64 references for what the GEMM epilogues fuse (RoPE, the paged KV write, the split
RMSNorm): CPU torch only, no kernel code.  tests/test_fused_oracle.py checks these functions against
the project's older references; tests/test_fused_epilogues_gpu.py checks the kernels against them."""
import torch

KVB = 128  # paged KV block (KV_BLOCK in csrc/common.h)


def rope_table(max_ctx, hd, theta):
    """The engine's (cos, sin) table [max_ctx][hd / 2][2]: angles in float64, entries rounded to fp32."""
    p = torch.arange(hd // 2, dtype=torch.float64)
    ang = torch.arange(max_ctx, dtype=torch.float64)[:, None] * torch.pow(torch.tensor(float(theta), dtype=torch.float64),
                                                                          -2.0 * p / hd)[None]
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).to(torch.float32)


def rope_pairs(x, pos, cs_table, neox=False):
    """x [T, heads, hd] rotated at pos [T] with the fp32 table the kernel reads, in float64.  Pairs are
    (2i, 2i + 1) -- or (i, i + hd / 2) for neox -- and pair i of a head uses table entry i."""
    x = x.double()
    cs = cs_table.double()[pos.long()]  # [T, hd / 2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    hd = x.shape[-1]
    if neox:
        a, b = x[..., :hd // 2], x[..., hd // 2:]
        return torch.cat([a * c - b * s, a * s + b * c], -1)
    a, b = x[..., 0::2], x[..., 1::2]
    out = torch.empty_like(x)
    out[..., 0::2] = a * c - b * s
    out[..., 1::2] = a * s + b * c
    return out


def rope_pair_mag(x, neox=False):
    """|v0| + |v1| of the pair each element of x [.., hd] belongs to (the scale of its fp32 rounding)."""
    x = x.double().abs()
    hd = x.shape[-1]
    if neox:
        m = x[..., :hd // 2] + x[..., hd // 2:]
        return torch.cat([m, m], -1)
    m = x[..., 0::2] + x[..., 1::2]
    return m.repeat_interleave(2, -1)


def kv_targets(pos, slot, block_table, n_kv_heads, hd, max_ctx):
    """Element offsets [T, n_kv_heads, hd] into a layer's pool [blocks][n_kv_heads][KVB][hd] that row t
    writes (kv_offset, csrc/common.h).  slot None: slot 0 for every row (the epilogues' null-slot rule);
    block_table None: the identity map block = slot * (max_ctx / KVB) + pos / KVB."""
    pos = pos.long()
    T = pos.shape[0]
    slot = torch.zeros(T, dtype=torch.long) if slot is None else slot.long()
    maxb = max_ctx // KVB
    j = pos // KVB
    blk = slot * maxb + j if block_table is None else block_table.long().reshape(-1, maxb)[slot, j]
    head = torch.arange(n_kv_heads)[None, :, None]
    e = torch.arange(hd)[None, None, :]
    return ((blk[:, None, None] * n_kv_heads + head) * KVB + (pos % KVB)[:, None, None]) * hd + e


def split_norm_parts(x, tile):
    """[M, N] -> [M, N / tile]: the sum of squares of each tile-column block of every row, float64."""
    M, N = x.shape
    assert N % tile == 0
    return (x.double() ** 2).reshape(M, N // tile, tile).sum(-1)


def bf16_steps(got, ref):
    """How many bf16 steps the bf16 tensor `got` lies from bf16(ref), ref float64: 0 = the correctly
    rounded value, 1 = its neighbour.  Codes compared as sign-magnitude integers (monotone in value)."""
    def key(t):
        b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(b >= 0x8000, 0x8000 - b, b)
    return (key(got) - key(ref.to(torch.float32).to(torch.bfloat16))).abs()


def fp8_bound(ref, scale):
    """|code * scale - ref| allowed for an e4m3 store of ref / scale: half a step of a 3-bit mantissa
    (2^-4 relative, with the 1e-3 slack for the fp32 product ref * inv) plus half the smallest subnormal
    step (2^-9 / 2) in units of the scale."""
    return 2.0 ** -4 * ref.double().abs() * (1 + 1e-3) + 2.0 ** -10 * scale


def rsqrt_scale(parts, K, eps):
    """The consumer's row scale rsqrt(sum_t parts[m][t] / K + eps), float64."""
    return 1.0 / torch.sqrt(parts.double().sum(-1) / K + eps)
