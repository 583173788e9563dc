"""Plain float64 reference of the two attention kernels (decode and prefill) and the adversarial inputs
their tests run on: CPU torch only, no kernel code.  tests/test_attention_oracle.py checks the reference
and the conditions every input family promises; tests/test_attention_gpu.py checks the kernels.

Why not randn: i.i.d. K / q give a flat softmax (every key weighs about 1 / L), under which a swapped
key pair, a causal mask off by one or a head mix-up moves the output by less than the tolerance, and the
running maximum hardly moves, so the rescale paths only ever see alpha = 1.  The families here:

peaked      q and K are RoPE rotations of one constant vector, so score(key j) depends on j - target
            only and peaks sharply at the target: one key (the needle) holds >= 0.99 of the mass and V
            rows are independent randn, so any wrong key is an O(1) error.
ramp        scores monotone in the key index over the whole context, about 60 log2 units end to end:
            ascending makes every pass raise the running maximum (every pass rescales), descending never
            after the first, late_spike is flat but for one key of the last pass.
poison      every element of the physical pools that no live key owns becomes NaN / +-Inf.
decoy       the same region, finite: K the best-scoring row of the case, V a constant 100.
"""
import math

import torch

KVB = 128  # paged KV block (KV_BLOCK in csrc/common.h)
LOG2E = 1.4426950408889634


# ---------------------------------------------------------------------------------- paged pools
def paged(x, shuffle=False, seed=0):
    """Logical KV [S, Hkv, C, hd] -> (physical pool [S*C/KVB, Hkv, KVB, hd], block table [S, C/KVB] or
    None for the identity map).  shuffle scatters the logical blocks over a random permutation."""
    S, Hk, C, D = x.shape
    nb = C // KVB
    blocks = x.reshape(S, Hk, nb, KVB, D).permute(0, 2, 1, 3, 4).reshape(S * nb, Hk, KVB, D)
    if not shuffle:
        return blocks.contiguous(), None
    perm = torch.randperm(S * nb, generator=torch.Generator().manual_seed(seed))
    phys = torch.empty_like(blocks)
    phys[perm] = blocks
    return phys.contiguous(), perm.view(S, nb).to(torch.int32)


def unpaged(phys, S, C, bt=None):
    """Inverse of paged: physical pool (+ table) -> logical [S, Hkv, C, hd]."""
    nb = C // KVB
    blocks = phys if bt is None else phys[bt.reshape(-1).long().to(phys.device)]
    Hk, D = phys.shape[1], phys.shape[3]
    return blocks.reshape(S, nb, Hk, KVB, D).permute(0, 2, 1, 3, 4).reshape(S, Hk, C, D)


def live_mask(n_live, C, bt=None):
    """[S*C/KVB, KVB] bool over the physical pool: True where a key position belongs to the first
    n_live[s] keys of slot s (bt: the table paged() returned, None for the identity map)."""
    S, nb = len(n_live), C // KVB
    live = torch.zeros(S * nb, KVB, dtype=torch.bool)
    for s in range(S):
        for j in range(nb):
            blk = s * nb + j if bt is None else int(bt[s, j])
            live[blk] = j * KVB + torch.arange(KVB) < n_live[s]
    return live


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def quantise(x, fp8):
    """Logical values -> (storage tensor, the exact value of every stored element as fp32, scale).
    bf16: RNE, scale 1.  fp8: OCP e4m3 codes (uint8) at scale amax / 448; value = code * scale."""
    if not fp8:
        s = x.to(torch.bfloat16)
        return s, s.float(), 1.0
    scale = _f32(float(x.abs().max()) / 448.0) or 1.0
    c = (x.double() / scale).clamp(-448, 448).float().to(torch.float8_e4m3fn)
    return c.view(torch.uint8), c.float(), scale


# ---------------------------------------------------------------------------------- reference
def attn_scores(q, k, scale, k_scale=1.0):
    """Raw base-2 scores [R, H, L], float64, as both kernels define them: q * (scale * log2 e * k_scale)
    -- the factor and the product formed in fp32 -- rounded to bf16, against the stored K (k / k_scale:
    bf16 values, or fp8 codes).  q [R, H, hd] fp32; k [Hkv, L, hd]; head h reads KV head h // G."""
    H, Hkv = q.shape[1], k.shape[0]
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    c = c * torch.tensor(k_scale, dtype=torch.float32)
    qs = (q.float() * c).to(torch.bfloat16).double()
    kk = (k.double() / k_scale)[torch.arange(H) // (H // Hkv)]
    return torch.einsum("rhd,hld->rhl", qs, kk)


def attn_ref(q, k, v, visible, scale, k_scale=1.0, v_scale=1.0, p_bf16=False):
    """Attention as the kernels define it, float64.  k, v [Hkv, L, hd]: the logical values the cache
    holds (bf16 values, or fp8 code * scale); visible [R, L] bool (decode: key < len; prefill:
    key <= start + t).  p_bf16 rounds every 2^(s - max) to bf16 before P.V (the prefill MFMA's operand)
    while the denominator keeps the unrounded sum, as the kernel does.
    Returns out [R, H, hd] and mag = sum_k p_k |v_kd| / sum_k p_k, the scale of its rounding error."""
    H, Hkv = q.shape[1], k.shape[0]
    s = attn_scores(q, k, scale, k_scale).masked_fill(~visible[:, None, :], float("-inf"))
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    den = p.sum(-1)[..., None]
    vv = v.double()[torch.arange(H) // (H // Hkv)]  # (already scaled: v_scale is part of the value)
    pv = p.float().to(torch.bfloat16).double() if p_bf16 else p
    out = torch.einsum("rhl,hld->rhd", pv, vv) / den
    mag = torch.einsum("rhl,hld->rhd", p, vv.abs()) / den
    return out, mag


# ---------------------------------------------------------------------------------- input families
def rope_rows(pos, amp):
    """[..., hd] float64: pair i of the row at position p is amp[i] * (cos, sin)(p * theta_i), the RoPE
    rotation of the constant vector (amp[i], 0) over the hd / 2 geometric frequencies of base 10000."""
    n = amp.shape[0]
    th = 10000.0 ** (-torch.arange(n, dtype=torch.float64) / n)
    ang = pos.double()[..., None] * th
    return torch.stack([amp * torch.cos(ang), amp * torch.sin(ang)], -1).flatten(-2)


def peak_amp(hd, peak, ratio=0.8):
    """Per-pair amplitudes: score(j) = sum_i amp_i^2 cos((j - target) theta_i), so the peak is
    sum amp^2 = `peak` log2 units (<= 128).  Weights fall geometrically with the frequency index: the
    fast pairs carry the weight, so the score drops by tens of units one key off the target (equal
    weights would need a peak of about 240 for an 8-unit drop) and by more everywhere further."""
    assert peak <= 128
    w = ratio ** torch.arange(hd // 2, dtype=torch.float64)
    return torch.sqrt(w / w.sum() * peak)


DECODE_PEAK, PREFILL_PEAK = 64.0, 96.0  # the smaller decode peak keeps its fp32 scores finer (2^-18 ulp)


def peaked(seed, S, Hkv, C, hd, target, scale, peak):
    """q [R, H, hd] fp32 pointing at key position target [R, H]; K [S, Hkv, C, hd] float64 whose row j
    is the constant vector rotated to j (every slot and head alike: V tells them apart); V randn."""
    amp = peak_amp(hd, peak)
    k = rope_rows(torch.arange(C), amp).expand(S, Hkv, C, hd)
    q = (rope_rows(target, amp) / (scale * LOG2E)).float()
    v = torch.randn(S, Hkv, C, hd, generator=torch.Generator().manual_seed(seed))
    return q, k, v


RAMP_SPAN = 60.0
SPIKE = 40.0


def ramp(seed, S, Hkv, C, hd, R, H, scale, kind, spike=None):
    """Scores t_j along a random unit direction per KV head: ascending t_j = -30 .. +30 over the C keys
    of the context, descending the reverse; late_spike: -5 everywhere but +SPIKE at key spike[s] of
    slot s.  Query head h scales the span by 1 - 0.1 * (h % 3), so the heads of a group differ.
    Half of the rise is a slope, half a step at every 64th key (the prefill tile; every other one a
    decode pass edge): a pass that holds one live key still beats the pass before it by more than the
    storage format's rounding of K moves a score (fp8: about 0.2 units at |t| = 30)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(Hkv, hd, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    half = RAMP_SPAN / 2
    j = torch.arange(C, dtype=torch.float64)
    t = (-half + half * (j / (C - 1) + (j // 64) / (C // 64 - 1))).expand(S, C).clone()
    if kind == "descending":
        t = -t
    elif kind == "late_spike":
        t[:] = -5.0
        for s, j in enumerate(spike):
            if j is not None:
                t[s, j] = SPIKE
    else:
        assert kind == "ascending"
    root = math.sqrt(half)
    k = t[:, None, :, None] / root * u[None, :, None, :]
    gain = 1.0 - 0.1 * (torch.arange(H) % 3).double()
    q = (root * gain[None, :, None] * u[torch.arange(H) // (H // Hkv)][None] / (scale * LOG2E)).expand(R, H, hd).float()
    v = torch.randn(S, Hkv, C, hd, generator=g)
    return q.contiguous(), k, v


_BF16_BAD = torch.tensor([0x7FC0, 0x7F80, 0x7FC0, 0xFF80 - 0x10000], dtype=torch.int16)  # NaN, +Inf, NaN, -Inf
_FP8_BAD = torch.tensor([0x7F, 0xFF], dtype=torch.uint8)  # e4m3 has no Inf: both NaN codes


def poison(pool, live):
    """A copy of the physical pool [NB, Hkv, KVB, hd] (bf16 or e4m3 codes as uint8) in which every
    element of a key position outside live [NB, KVB] holds a non-finite pattern: dead positions of a
    last block, whole unused blocks, other slots.  Live elements keep their bits."""
    bad = _FP8_BAD if pool.dtype == torch.uint8 else _BF16_BAD.view(torch.bfloat16)
    fill = bad[torch.arange(pool.numel()) % bad.numel()].view(pool.shape)
    return torch.where(live[:, None, :, None], pool, fill)


def decoy(kpool, vpool, live, krow, v_const=100.0):
    """Copies of the pools whose dead positions are finite and tempting: K = krow [Hkv, hd] (the row
    of the case with the highest score, in the pool's storage type), V = v_const in storage units
    (bf16: the value; fp8: the code's value, 448 the largest)."""
    m = live[:, None, :, None]
    kfill = krow[None, :, None, :].expand(kpool.shape)
    if vpool.dtype == torch.uint8:
        vfill = torch.full(vpool.shape, v_const).to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        vfill = torch.full(vpool.shape, v_const, dtype=vpool.dtype)
    return torch.where(m, kpool, kfill), torch.where(m, vpool, vfill)


# ---------------------------------------------------------------------------------- the tested cases
# decode: (hd, H, Hkv) -- G = 1, G = 2 with n_heads & 7 != 0, G = 5 (non-XCD mapping), G = 4 (control)
DECODE_LAYOUTS = [(64, 4, 4), (128, 12, 6), (128, 20, 4), (128, 32, 8)]
# (lens, max_ctx): the last live key at pass / lane-group edges, 512|513 the short|long boundary; every
# context leaves at least one whole unused block in some row
DECODE_LENS = [([1], 256), ([127, 128, 129], 256), ([512, 513], 768), ([1025, 3], 1280)]
DECODE_FAMILIES = ["peaked-first", "peaked-last", "peaked-127", "peaked-128", "ascending", "descending", "late_spike"]
# prefill: (H, Hkv, hd) and (start, T) at max_ctx 512
PREFILL_LAYOUTS = [(8, 8, 64), (16, 8, 128), (32, 8, 128), (64, 8, 128), (32, 4, 64)]
PREFILL_CASES = [(0, 1), (200, 1), (0, 63), (0, 64), (0, 65), (0, 127), (0, 129), (70, 130), (61, 7), (384, 128),
                 (1, 300)]
PREFILL_FAMILIES = ["peaked", "ascending"]
PREFILL_CTX = 512
# more than 32 partials for the two-trip combine: (hd, H, Hkv, lens, max_ctx) at split 4096
DECODE_WIDE = [(64, 4, 1, [4225], 8192), (64, 4, 1, [8192], 8192)]
DECODE_KNOB = (128, 32, 8, [129, 700], 1024)  # one row per mode: short (<= 512 keys) and long


class Case:
    """One launch's inputs.  q fp32; kraw / vraw the logical caches [S, Hkv, C, hd] in storage type
    (bf16, or uint8 e4m3 codes); kval / vval the exact value of every stored element / scale, fp32;
    sk / sv the scales; n_live[s] the live keys of slot s; slot[r] / visible[r] per query row."""

    def k(self, s, L):
        return self.kval[s, :, :L].double() * self.sk

    def v(self, s, L):
        return self.vval[s, :, :L].double() * self.sv

    def ref(self, rows, s, L, p_bf16=False):
        """(out, mag) of query rows `rows` (a slice or index list) against the first L keys of slot s."""
        return attn_ref(self.q[rows], self.k(s, L), self.v(s, L), self.visible[rows][:, :L], self.scale, self.sk,
                        self.sv, p_bf16)


def _finish(c, q, k, v, fp8, scale):
    c.q, c.scale, c.fp8 = q, scale, fp8
    c.kraw, c.kval, c.sk = quantise(k, fp8)
    c.vraw, c.vval, c.sv = quantise(v, fp8)
    return c


def decode_needles(family, lens, H):
    """needle [B, H] of a peaked decode family: the named key (first / last / 127 / 128, clamped to the
    row's live keys) moved back by h % 4 keys for head h, so the heads of a GQA group differ."""
    name = family.split("-")[1]
    base = [0 if name == "first" else n - 1 if name == "last" else min(int(name), n - 1) for n in lens]
    return torch.tensor([[max(0, b - (h % 4)) for h in range(H)] for b in base])


def spike_keys(lens):
    """late_spike: the middle live key of each row's last 128-key pass"""
    return [(n - 1) // KVB * KVB + ((n - 1) % KVB) // 2 for n in lens]


def decode_case(family, hd, H, Hkv, lens, max_ctx, fp8, seed=0, needle=None):
    """Row b reads slot b + 1 (slot 0 stays unused).  needle [B, H] overrides the family's."""
    c = Case()
    B, S = len(lens), len(lens) + 1
    scale = 1 / math.sqrt(hd)
    if family.startswith("peaked"):
        c.needle = decode_needles(family, lens, H) if needle is None else needle
        q, k, v = peaked(seed, S, Hkv, max_ctx, hd, c.needle, scale, DECODE_PEAK)
    else:
        c.spike = [None] + spike_keys(lens)
        q, k, v = ramp(seed, S, Hkv, max_ctx, hd, B, H, scale, family, c.spike)
    c.lens, c.n_live, c.slot, c.max_ctx = lens, [0] + list(lens), list(range(1, S)), max_ctx
    c.visible = torch.arange(max_ctx)[None, :] < torch.tensor(lens)[:, None]
    return _finish(c, q, k, v, fp8, scale)


def prefill_case(family, H, Hkv, hd, start, T, fp8, seed=0, max_ctx=PREFILL_CTX):
    """T query rows at positions start .. start + T - 1 of slot 1 (of 2).  peaked: row t points at key
    start + t + 1, its first masked key, so the diagonal is the needle and the best raw score of every
    row is a key the causal mask must hide."""
    c = Case()
    scale = 1 / math.sqrt(hd)
    qpos = start + torch.arange(T)
    if family == "peaked":
        q, k, v = peaked(seed, 2, Hkv, max_ctx, hd, (qpos + 1)[:, None].expand(T, H), scale, PREFILL_PEAK)
    else:
        q, k, v = ramp(seed, 2, Hkv, max_ctx, hd, T, H, scale, family)
    c.start, c.T, c.n_live, c.slot, c.max_ctx = start, T, [0, start + T], [1] * T, max_ctx
    c.visible = torch.arange(max_ctx)[None, :] <= qpos[:, None]
    return _finish(c, q, k, v, fp8, scale)


def pools(c, shuffle, seed=0, mode="poison", krow=None, n_live=None):
    """The physical K and V pools of a case and its block table: mode "poison" / "decoy" / "clean"
    decides what the dead key positions hold (clean: the family's own finite values)."""
    kp, bt = paged(c.kraw, shuffle, seed)
    vp, _ = paged(c.vraw, shuffle, seed)
    live = live_mask(c.n_live if n_live is None else n_live, c.max_ctx, bt)
    if mode == "poison":
        kp, vp = poison(kp, live), poison(vp, live)
    elif mode == "decoy":
        kp, vp = decoy(kp, vp, live, krow, 100.0 if not c.fp8 else 448.0)
    return kp, vp, bt, live
