"""Raw GGUF weight blocks that no quantizer emits, and their float64 decode (numpy only).

`build(t, rows, K, family, seed)` writes block bytes directly from BLOCK_INFO: the fp16 fields (d, dmin, m)
get independent signs, zeros, -0.0 and a subnormal; the code / scale bytes are random, saturated or split
(a sub-block scale of 0 next to a nonzero min and the reverse).  `decode(t, raw, rows, K)` is an element-wise
float64 decoder written from the public block layouts, independent of aios_amd.gguf.quants (the CPU test
holds the two against each other).  It returns, per element, the value w and the magnitudes of the unfolded
form: a = |d sc| q and b = |dmin m| (|m| for Q4_1 / Q5_1) for the affine formats, a = |w|, b = 0 otherwise;
s = a + b is the error scale of one element.

The random fp16 fields are +-2^-e x (1 + mant / 1024) with an ODD 10-bit mant: an odd 11-bit integer times
any nonzero integer code has at least 11 significant bits, so no product d x code is a bf16 value or an
exact bf16 rounding tie.  The exponent range is 4..12, narrowed per format so that max|w| <= 8; the two fields
of an affine format draw from disjoint parts of it (E_RANGE: the min field is the finer one), because sums of
two products on the same binary grid land on exact bf16 ties far too often for the boundary-band cap (0.27 %
of a Q4_K matrix, 0.9 % of Q4_1, with both fields on 4..12).
"""
import numpy as np

from aios_amd.gguf.quants import BLOCK_INFO, GGMLType as T

IQ4 = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float64)

ELEMENT_TYPES = (T.F32, T.F16, T.BF16)
# byte offset of each fp16 field (first = d, second = dmin / m)
FP16 = {
    T.Q4_0: (0,), T.Q4_1: (0, 2), T.Q5_0: (0,), T.Q5_1: (0, 2), T.Q8_0: (0,), T.IQ4_NL: (0,), T.IQ4_XS: (0,),
    T.Q2_K: (80, 82), T.Q3_K: (108,), T.Q4_K: (0, 2), T.Q5_K: (0, 2), T.Q6_K: (208,),
}
# the other bytes: scale fields, code (quant) bits, separate high bits
REGIONS = {
    T.Q4_0: {"quant": (2, 18)}, T.Q4_1: {"quant": (4, 20)},
    T.Q5_0: {"high": (2, 6), "quant": (6, 22)}, T.Q5_1: {"high": (4, 8), "quant": (8, 24)},
    T.Q8_0: {"quant": (2, 34)}, T.IQ4_NL: {"quant": (2, 18)}, T.IQ4_XS: {"scale": (2, 8), "quant": (8, 136)},
    T.Q2_K: {"scale": (0, 16), "quant": (16, 80)},
    T.Q3_K: {"high": (0, 32), "quant": (32, 96), "scale": (96, 108)},
    T.Q4_K: {"scale": (4, 16), "quant": (16, 144)},
    T.Q5_K: {"scale": (4, 16), "high": (16, 48), "quant": (48, 176)},
    T.Q6_K: {"quant": (0, 128), "high": (128, 192), "scale": (192, 208)},
}
# smallest e of |field| < 2^(1-e) that keeps max|w| <= 8: the largest |code x scale| (+ min) per format is
# Q4_K 63 (15 + 1) = 1008, Q5_K 63 (31 + 1) = 2016, Q6_K 128 x 32 = 4096, Q8_0 128, IQ4_NL 127, IQ4_XS 32 x 127,
# Q3_K 32 x 4, Q2_K 15 (3 + 1), Q5_1 31 + 1, Q4_1 15 + 1, Q5_0 16, Q4_0 8
E_MIN = {T.Q4_K: 8, T.Q5_K: 9, T.Q6_K: 10, T.Q8_0: 5, T.IQ4_NL: 5, T.IQ4_XS: 10, T.Q3_K: 5}
E_MAX = 12
# (d, second field) exponent ranges of the affine formats
E_RANGE = {T.Q4_K: ((8, 9), (11, 12)), T.Q5_K: ((9, 10), (11, 12)), T.Q2_K: ((4, 7), (9, 12)),
           T.Q4_1: ((4, 8), (9, 12)), T.Q5_1: ((4, 8), (9, 12))}
AFFINE = (T.Q4_K, T.Q5_K, T.Q2_K, T.Q4_1, T.Q5_1)
SPLIT_TYPES = (T.Q4_K, T.Q5_K, T.Q2_K)
F16_SUBNORMAL = 0x0010  # 2^-20
F16_NEG_ZERO = 0x8000


def families(t):
    if t in ELEMENT_TYPES:
        return ["random", "zeros"]
    return ["random", "zeros", "saturated"] + (["split"] if t in SPLIT_TYPES else [])


def _rand_f16_bits(rng, n, t, field=0):
    lo, hi = E_RANGE[t][field] if t in E_RANGE else (E_MIN.get(t, 4), E_MAX)
    e = rng.integers(lo, hi + 1, n)
    mant = rng.integers(0, 512, n) * 2 + 1
    sign = rng.integers(0, 2, n)
    return ((sign << 15) | ((15 - e) << 10) | mant).astype(np.uint16)


def _put_f16(b, off, bits, sel=slice(None)):
    bits = np.asarray(bits, np.uint16)
    b[sel, off] = (bits & 0xFF).astype(np.uint8)
    b[sel, off + 1] = (bits >> 8).astype(np.uint8)


def _variant(nblk, nbr, nv):
    """variant of block i (row i // nbr): the variants in turn, shifted by one after every nbr * nv blocks so
    that every variant meets every block position of a row"""
    i = np.arange(nblk)
    return (i + i // (nbr * nv)) % nv


def _kq_pack(sc, mn):
    """[nb, 8] 6-bit scales / mins -> the 12-byte Q4_K / Q5_K table (sub-blocks 0..3: low 6 bits of bytes j /
    j + 4; 4..7: low 4 bits in byte j + 4 (scale low nibble, min high), top 2 in bits 6..7 of bytes j - 4 / j)"""
    out = np.zeros((sc.shape[0], 12), np.int64)
    for j in range(4):
        out[:, j] |= sc[:, j]
        out[:, j + 4] |= mn[:, j]
    for j in range(4, 8):
        out[:, j + 4] |= (sc[:, j] & 15) | ((mn[:, j] & 15) << 4)
        out[:, j - 4] |= (sc[:, j] >> 4) << 6
        out[:, j] |= (mn[:, j] >> 4) << 6
    return out.astype(np.uint8)


def _build_elements(t, n, family, rng):
    e = rng.integers(4, E_MAX + 1, n)
    v = np.ldexp(1.0 + (rng.integers(0, 64, n) * 2 + 1) / 128.0, -e) * rng.choice([-1.0, 1.0], n)  # 8-bit mantissas
    if family == "zeros":
        k = np.arange(n) % 4
        v = np.where(k == 0, 0.0, np.where(k == 1, -0.0, np.where(k == 2, np.copysign(2.0 ** -20, v), v)))
    v32 = v.astype(np.float32)
    if t == T.F32:
        return v32.view(np.uint8)
    if t == T.F16:
        return v32.astype(np.float16).view(np.uint8)
    return (v32.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)  # (exact: 8 significant bits)


def build(t, rows, K, family, seed):
    """raw bytes (uint8, flat) of a [rows, K] matrix of type t from one block family"""
    t = T(t)
    assert family in families(t), (t, family)
    rng = np.random.default_rng([seed, int(t), families(t).index(family)])
    if t in ELEMENT_TYPES:
        return np.ascontiguousarray(_build_elements(t, rows * K, family, rng))
    blk, nbytes = BLOCK_INFO[t]
    nbr = K // blk
    nblk = rows * nbr
    b = rng.integers(0, 256, (nblk, nbytes), dtype=np.uint8)
    fields = FP16[t]
    for k, off in enumerate(fields):
        _put_f16(b, off, _rand_f16_bits(rng, nblk, t, k))
    if family == "zeros":
        # d = 0 | second field = 0 | both 0 | d = -0.0 | second = -0.0 | both -0.0; a few blocks: subnormal d
        two = len(fields) == 2
        v = _variant(nblk, nbr, 6 if two else 3)  # (one-field formats: every third block keeps its random d)
        for k, (zd, zs, bits) in enumerate([(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, F16_NEG_ZERO), (0, 1, F16_NEG_ZERO),
                                            (1, 1, F16_NEG_ZERO)] if two else [(1, 0, 0), (1, 0, F16_NEG_ZERO)]):
            if zd:
                _put_f16(b, fields[0], bits, v == k)
            if zs:
                _put_f16(b, fields[1], bits, v == k)
        # one subnormal d per 64 Ki elements of the 256-formats (whose d x scale x code products can be exact
        # bf16 ties: they count against the boundary-band cap), eight for the 32-formats; signs alternate
        nsub = 1 if blk == 256 else 8
        idx = (np.arange(nsub) * 2 + 1) * nblk // (2 * nsub) + np.arange(nsub) % nbr
        _put_f16(b, fields[0], F16_SUBNORMAL | ((np.arange(nsub) & 1) << 15), idx)
    elif family == "saturated":
        # every combination of {all bits clear, all bits set} over the regions; Q6_K scales also 0x7F / 0x80
        # (+127 / -128), Q8_0 codes also 0x7F / 0x80 (+127 / -128) and the two alternating
        regs = list(REGIONS[t].items())
        fills = []
        for name, _ in regs:
            f = [0x00, 0xFF]
            if (t == T.Q6_K and name == "scale") or (t == T.Q8_0 and name == "quant"):
                f += [0x7F, 0x80]
            if t == T.Q8_0:
                f += ["alt"]
            fills.append(f)
        combos = [[]]
        for f in fills:
            combos = [c + [x] for c in combos for x in f]
        v = _variant(nblk, nbr, len(combos))
        for k, combo in enumerate(combos):
            sel = v == k
            for (name, (lo, hi)), fill in zip(regs, combo):
                if fill == "alt":
                    b[sel, lo:hi] = np.where(np.arange(hi - lo) % 2 == 0, 0x80, 0x7F).astype(np.uint8)
                else:
                    b[sel, lo:hi] = fill
    elif family == "split":
        # per sub-block: (scale 0, min != 0) or (scale != 0, min 0); the pattern alternates, reversed on odd
        # blocks, random on every third
        nsb, top = (16, 15) if t == T.Q2_K else (8, 63)
        sc = rng.integers(1, top + 1, (nblk, nsb))
        mn = rng.integers(1, top + 1, (nblk, nsb))
        pat = (np.arange(nsb)[None, :] + np.arange(nblk)[:, None]) % 2
        rnd = rng.integers(0, 2, (nblk, nsb))
        pat = np.where((np.arange(nblk) % 3 == 2)[:, None], rnd, pat)
        sc = np.where(pat == 0, 0, sc)
        mn = np.where(pat == 1, 0, mn)
        if t == T.Q2_K:
            b[:, 0:16] = (sc | (mn << 4)).astype(np.uint8)
        else:
            b[:, 4:16] = _kq_pack(sc, mn)
    return np.ascontiguousarray(b.reshape(-1))


# ------------------------------------------------------------------------------------------ decode
def _f16(b, off):
    return np.ascontiguousarray(b[:, off:off + 2]).view(np.float16).astype(np.float64)  # [nb, 1]


def _nibbles32(qs):
    """16 bytes -> 32 codes: element j < 16 low nibble of byte j, else high nibble of byte j - 16"""
    return np.concatenate([qs & 15, qs >> 4], axis=-1).astype(np.int64)


def _decode_blocks(t, b):
    """b [nb, block bytes] uint8 -> (w, a, bm) float64 [nb, block elements]"""
    nb = b.shape[0]
    bi = b.astype(np.int64)
    if t in (T.Q4_0, T.IQ4_NL, T.Q4_1):
        hdr = 4 if t == T.Q4_1 else 2
        code = _nibbles32(bi[:, hdr:hdr + 16])
        d = _f16(b, 0)
        if t == T.Q4_0:
            w = d * (code - 8)
            return w, np.abs(w), np.zeros_like(w), np.abs(d) * (code + 8)
        elif t == T.IQ4_NL:
            w = d * IQ4[code]
        else:
            m = _f16(b, 2)
            return d * code + m, np.abs(d) * code, np.abs(m) + 0.0 * code
        return w, np.abs(w), np.zeros_like(w)
    if t in (T.Q5_0, T.Q5_1):
        hdr = 2 if t == T.Q5_0 else 4
        qh = bi[:, hdr] | (bi[:, hdr + 1] << 8) | (bi[:, hdr + 2] << 16) | (bi[:, hdr + 3] << 24)
        code = _nibbles32(bi[:, hdr + 4:hdr + 20]) | (((qh[:, None] >> np.arange(32)[None, :]) & 1) << 4)
        d = _f16(b, 0)
        if t == T.Q5_0:
            w = d * (code - 16)
            return w, np.abs(w), np.zeros_like(w)
        m = _f16(b, 2)
        return d * code + m, np.abs(d) * code, np.abs(m) + 0.0 * code
    if t == T.Q8_0:
        code = b[:, 2:34].view(np.int8).astype(np.float64)
        w = _f16(b, 0) * code
        return w, np.abs(w), np.zeros_like(w), np.abs(_f16(b, 0)) * (code + 256)
    j = np.arange(256)
    if t == T.IQ4_XS:
        ib = np.arange(8)
        sh = bi[:, 2] | (bi[:, 3] << 8)
        ls = ((bi[:, 4 + ib // 2] >> (4 * (ib % 2))) & 15) | (((sh[:, None] >> (2 * ib)) & 3) << 4)
        idx = _nibbles32(bi[:, 8:136].reshape(nb, 8, 16)).reshape(nb, 256)
        w = _f16(b, 0) * (ls - 32)[:, j >> 5] * IQ4[idx]
        return w, np.abs(w), np.zeros_like(w)
    if t in (T.Q2_K, T.Q3_K):
        base = 16 if t == T.Q2_K else 32
        low2 = (bi[:, base + 32 * (j >> 7) + (j & 31)] >> (2 * ((j >> 5) & 3))) & 3
        if t == T.Q2_K:
            d, dmin = _f16(b, 80), _f16(b, 82)
            sb = bi[:, j >> 4]
            sc, mn = sb & 15, sb >> 4
            return d * sc * low2 - dmin * mn, np.abs(d * sc) * low2, np.abs(dmin * mn)
        s = j >> 4
        g, k = s >> 2, s & 3
        low4 = (bi[:, 96 + np.where(g & 1, 4, 0) + k] >> np.where(g & 2, 4, 0)) & 15
        sc = (low4 | (((bi[:, 104 + k] >> (2 * g)) & 3) << 4)) - 32
        hb = (bi[:, j & 31] >> (j >> 5)) & 1
        w = _f16(b, 108) * sc * (low2 - 4 * (1 - hb))
        return w, np.abs(w), np.zeros_like(w)
    if t in (T.Q4_K, T.Q5_K):
        q = bi[:, 4:16]
        sc = np.empty((nb, 8), np.int64)
        mn = np.empty((nb, 8), np.int64)
        for s in range(8):
            if s < 4:
                sc[:, s], mn[:, s] = q[:, s] & 63, q[:, s + 4] & 63
            else:
                sc[:, s] = (q[:, s + 4] & 15) | ((q[:, s - 4] >> 6) << 4)
                mn[:, s] = (q[:, s + 4] >> 4) | ((q[:, s] >> 6) << 4)
        sub, i = j >> 5, j & 31
        qs0 = 16 if t == T.Q4_K else 48
        code = (bi[:, qs0 + 32 * (sub >> 1) + i] >> (4 * (sub & 1))) & 15
        if t == T.Q5_K:
            code = code | (((bi[:, 16 + i] >> sub) & 1) << 4)
        d, dmin = _f16(b, 0), _f16(b, 2)
        return d * sc[:, sub] * code - dmin * mn[:, sub], np.abs(d * sc[:, sub]) * code, np.abs(dmin * mn[:, sub])
    if t == T.Q6_K:
        n, r = j >> 7, j & 127
        k4, l_ = r >> 5, r & 31
        nib = (bi[:, 64 * n + 32 * (k4 & 1) + l_] >> (4 * (k4 >> 1))) & 15
        h2 = (bi[:, 128 + 32 * n + l_] >> (2 * k4)) & 3
        sc = b[:, 192:208].view(np.int8).astype(np.int64)[:, 8 * n + 2 * k4 + (l_ >> 4)]
        code = nib | (h2 << 4)
        w = _f16(b, 208) * sc * (code - 32)
        return w, np.abs(w), np.zeros_like(w), np.abs(_f16(b, 208) * sc) * (code + 32)
    raise ValueError(t)


def decode(t, raw, rows, K):
    """(w, a, bm): float64 [rows, K] value and unfolded magnitudes of every element"""
    t = T(t)
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if t in ELEMENT_TYPES:
        if t == T.F32:
            w = raw.view(np.float32).astype(np.float64)
        elif t == T.F16:
            w = raw.view(np.float16).astype(np.float64)
        else:
            w = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        w = w.reshape(rows, K)
        return w, np.abs(w), np.zeros_like(w)
    blk, nbytes = BLOCK_INFO[t]
    w, a, bm = _decode_blocks(t, raw.reshape(-1, nbytes))[:3]
    return w.reshape(rows, K), (a + 0.0).reshape(rows, K), (bm + 0.0).reshape(rows, K)


def rebias_scale(t, raw, rows, K):
    """error scale of the kernels' folded form of the symmetric formats they re-bias to unsigned codes u:
    d sc u x - (bias d sc) x, bias 8 (Q4_0), 32 (Q6_K), 128 (Q8_0): |d sc| (u + bias) per element; the other
    formats: a + bm"""
    t = T(t)
    if t not in (T.Q4_0, T.Q6_K, T.Q8_0):
        _, a, bm = decode(t, raw, rows, K)
        return a + bm
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, BLOCK_INFO[t][1])
    return (_decode_blocks(t, raw)[3] + 0.0).reshape(rows, K)


class Matrix:
    """one family's matrix: raw bytes, float64 values, error scale s = a + bm"""

    def __init__(self, t, rows, K, family, seed=0):
        self.t, self.rows, self.K, self.family = T(t), rows, K, family
        self.raw = build(t, rows, K, family, seed)
        self.w, self.a, self.bm = decode(t, self.raw, rows, K)
        self.s = self.a + self.bm
        self.s_fold = rebias_scale(t, self.raw, rows, K)


_cache = {}


def matrix(t, rows, K, family, seed=0):
    key = (int(t), rows, K, family, seed)
    if key not in _cache:
        _cache[key] = Matrix(t, rows, K, family, seed)
    return _cache[key]


# ------------------------------------------------------------------------------------------ bf16
def bf16_round(w):
    """float64 -> (nearest-even bf16 value as float64, its ulp, distance of w to the nearest rounding boundary)"""
    w = np.asarray(w, np.float64)
    aw = np.abs(w)
    _, e = np.frexp(aw)  # aw = m 2^e, m in [0.5, 1)
    ulp = np.ldexp(1.0, e - 8)  # 8 significant bits
    t = aw / ulp
    r = np.copysign(np.rint(t) * ulp, w)
    frac = t - np.floor(t)
    dist = np.where(aw > 0, np.abs(frac - 0.5) * ulp, np.inf)
    return r, ulp, dist


def bf16_bits(v):
    """float64 values that are bf16 values -> their 16 bits"""
    return (np.asarray(v, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def boundary_band(w, s):
    """elements whose float64 value lies within 2^-22 s of a bf16 rounding boundary (fp32 evaluation may round
    them either way)"""
    return bf16_round(w)[2] <= 2.0 ** -22 * s


# ------------------------------------------------------------------------------------------ activations
ACTS = ("randn", "offset", "sparse", "tiny")
TINY_RUNS = ((3, 1e-30), (9, 1e-40))  # (32-run index, factor); 1e-40 is an fp32 subnormal


def _q8_units(x):
    """x [B, K] fp32 -> value of every entry in int8 units of its 32-block (fp32 arithmetic, as the kernels and
    ReferenceModel.q8 compute it), and the blocks whose 127 / amax overflows"""
    xb = x.reshape(-1, 32)
    amax = np.abs(xb).max(-1, keepdims=True)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = np.where(amax > 0, np.float32(127.0) / amax, np.float32(0)).astype(np.float32)
        v = (xb * inv).astype(np.float32)
    return v, ~np.isfinite(inv)


def activations(kind, B, K, seed=0, int8=False):
    """[B, K] fp32.  int8: entries within 1e-3 of a .5 rounding tie in the int8 units of their 32-block are redrawn
    (shrunk by a random factor: the block's amax stays), so ReferenceModel.q8 is unambiguous."""
    assert kind in ACTS and K % 32 == 0 and K >= 320
    rng = np.random.default_rng([seed, ACTS.index(kind), B, K])
    x = rng.standard_normal((B, K)).astype(np.float32)
    if kind == "offset":
        x += np.float32(8.0)
    elif kind == "sparse":
        x[:, 64:96] = 0
        x[:, K - 32:] = 0
        x[:, 37] = 1e4
        if B > 1:
            x[1] = 0
    elif kind == "tiny":
        for run, f in TINY_RUNS:
            x[:, 32 * run:32 * run + 32] *= np.float32(f)
    if int8:
        for _ in range(100):
            v, over = _q8_units(x)
            v = np.where(over, 0, v)
            bad = np.abs(np.abs(v - np.floor(v)) - 0.5) < 1e-3
            if not bad.any():
                break
            xb = x.reshape(-1, 32)
            xb[bad] *= rng.uniform(0.5, 0.95, int(bad.sum())).astype(np.float32)
        else:
            raise AssertionError("int8 ties left")
    return x
