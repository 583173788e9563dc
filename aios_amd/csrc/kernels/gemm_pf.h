// Prefill GEMM on the CDNA4 matrix cores, dequantising the packed weights ONCE per workgroup tile:
//   C[M][N] (epilogue) = A[M][K] (bf16 activations) x W[N][K]^T (the GEMV engines' quantised planes, or bf16)
// -- the work llama.cpp's mul_mat_q does -- without any resident dequantised copy of a weight and
// without a vendor GEMM.
//
// Common to the three bodies.  A workgroup owns a BM x BN tile (BM = 256 / 128 / 64); each wave owns
// ALL BM rows and 32 columns, dequantises exactly its own columns' weights (each weight byte decoded
// once per workgroup, straight into MFMA B fragments in registers -- no bf16 LDS image of the
// weights, no LDS write pass) and shares the activation tile with the other waves through LDS (BM
// rows x 128 B per 64-deep K-step, 16-B units XOR-swizzled by row so a ds_read_b128 lane group hits
// distinct banks).  Everything is staged by global_load_lds (LDS-DMA: no VGPR staging, no ds_write)
// in compile-time pieces, a wave fetching its own columns, so each wave waits with one counted
// s_waitcnt vmcnt immediate -- the only vector-memory operations inside the loops are these DMAs, so
// the counts are exact.  One raw s_barrier per K-step (in-flight LDS-DMA survives it), placed between
// the two halves of the step's last MFMA phase; the next step's B fragments are decoded inside this
// step's phases; the loops are branch-free.
//
// The bodies and the launches they serve (PfTile, pf_launch below):
//   pf4_body   128-column tiles of every format: 4 waves (one per SIMD), v_mfma_f32_32x32x16_bf16,
//              a ring of per-K-step slots (Pf4Layout / Pf4Dma).
//   pf8_body   256-column tiles of bf16 and of the Q5_K / Q4_0 / Q8_0 stacks (their Q6_K segments
//              too): 8 waves (two per SIMD), v_mfma_f32_16x16x32_bf16, the same slot ring.
//   pf8c_body  256-column tiles of the K-quant stacks (Q4_K, Q6_K, their mix): pf8 with the weight
//              planes staged coalesced per half block / block (PfcLayout / PfcDma).
// Each runs as a plain launch (grid = tiles x K slices), with the tail split (256-row tiles) or as
// stream-K; one kernel per mode, pf_run_tile picking the body and the segment's format.
//
// Weight k order: chunk h (16 B) of a 64-weight Q4_K group holds weights 16h + i (low nibble of byte
// i) and 32 + 16h + i (high nibble).  Lane quarter q of the 16x16x32 B fragment reads bytes
// 8(q&1) .. 8(q&1)+7 of chunk q>>1: its low nibbles are k = 8q .. 8q+7 (fragment of k-substep 0)
// and its high nibbles k = 32 + 8q .. (substep 1) -- exactly the MFMA's natural k layout, so the A
// fragments are plain 16-B row reads at unit 4s + q.  Q6_K is repacked into the same chunk order
// (qweight.h), its 2 high bits and int8 sub-block scales riding beside the codes.
#pragma once
#include <cstdlib>

#include "gemm_common.h"

namespace aios {

// GEPI_QKV (prefill chunks, non-NeoX RoPE, no QK-norm / bias, S = 1): the accumulator element
// (m, n) of this lane goes to the attention inputs directly -- RoPE'd q fp32 to q_out[m][q_dim], RoPE'd
// k and v as bf16 into the paged KV cache at (slot[m], pos[m]) -- the qkv_post launch and the fp32
// QKV round trip folded into the epilogue.  The RoPE partner (column n ^ 1) is the lane ^ 1 in both
// accumulator layouts (column = lane mod 16 / 32); every lane runs the DPP, the even one stores the pair.
__device__ __forceinline__ void pf_qkv_out(const GemmQArgs& a, int m, int n, float v, bool even) {
  const float w = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
  if (!even || m >= a.M) return;
  const int hd = a.head_dim, pos = a.pos[m], slot = a.slot ? a.slot[m] : 0;
  float v0 = v, v1 = w;
  const int part = n < a.q_dim ? 0 : (n < a.q_dim + a.kv_dim ? 1 : 2);
  const int r = n - (part == 0 ? 0 : (part == 1 ? a.q_dim : a.q_dim + a.kv_dim));
  const int head = r / hd, lr = r - head * hd;
  if (part < 2) {
    const float2 t = a.rope_cs[(size_t)pos * (hd >> 1) + (lr >> 1)];
    const float o0 = v0 * t.x - v1 * t.y, o1 = v0 * t.y + v1 * t.x;
    v0 = o0;
    v1 = o1;
  }
  if (part == 0) {
    *(float2*)(a.q_out + (size_t)m * a.q_dim + n) = make_float2(v0, v1);
  } else {
    bf16_t* cache = part == 1 ? a.k_cache : a.v_cache;
    const size_t base = kv_offset(a.block_table, a.max_ctx / KV_BLOCK, slot, a.n_kv_heads, head, pos, hd);
    *(uint32_t*)(cache + base + lr) = pk_bf16(v0, v1);
  }
}

// The epilogue of one accumulator element (m, n) = v; `even`: this lane's column is even (its pair
// partner, column n ^ 1, is the lane ^ 1).  S > 1: a split-K / stream-K partial, added atomically.
template <int EPI>
__device__ __forceinline__ void pf_store(const GemmQArgs& a, int m, int n, float v, bool even, int S) {
  if constexpr (EPI == GEPI_SWIGLU_BF16) {
    // interleaved gate/up columns: even lane = gate, odd lane = its up partner
    const float up = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
    if (m < a.M && even) a.C16[(size_t)m * a.ldc + (n >> 1)] = f32_to_bf16(v / (1.f + __expf(-v)) * up);
  } else if constexpr (EPI == GEPI_QKV) {
    pf_qkv_out(a, m, n, v, even);
  } else if (m < a.M) {
    float* cp = a.C + (size_t)m * a.ldc + n;
    if (S > 1) unsafeAtomicAdd(cp, v);
    else if constexpr (EPI == GEPI_ACCUM) *cp += v;
    else *cp = v;
  }
}

__device__ __forceinline__ void pf_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <int N>
__device__ __forceinline__ void pf_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS-DMA through inline asm: hipcc's waitcnt pass then does not see the DMA, so it no longer puts
// an `s_waitcnt vmcnt(0)` in front of the first ds_read after every issue (it cannot prove the read
// misses the DMA's target slot -- measured: that drain serialised every K-step).  The counted
// pf_vmcnt waits below are the only ordering these loads need.  M0 is set and restored inside the
// statement (CDNA guide §5.7, LDS-DMA recipe).
__device__ __forceinline__ uint32_t pf_lds_addr(const uint8_t* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)p;
}
__device__ __forceinline__ void pf_glds16(const void* src, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds)
               : "memory");
}
__device__ __forceinline__ void pf_glds4(const void* src, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds)
               : "memory");
}

// 8 codes (bytes of w0 then w1) -> bf16x8 fragment of sc * q - of
__device__ __forceinline__ gbf16x8 pf_dq8(uint32_t w0, uint32_t w1, float sc, float of) {
  asm volatile("" : "+v"(w0), "+v"(w1));  // one v_cvt_f32_ubyteN per byte
  uint32_t p[4];
  p[0] = pk_bf16(fmaf(sc, (float)(w0 & 0xff), -of), fmaf(sc, (float)((w0 >> 8) & 0xff), -of));
  p[1] = pk_bf16(fmaf(sc, (float)((w0 >> 16) & 0xff), -of), fmaf(sc, (float)(w0 >> 24), -of));
  p[2] = pk_bf16(fmaf(sc, (float)(w1 & 0xff), -of), fmaf(sc, (float)((w1 >> 8) & 0xff), -of));
  p[3] = pk_bf16(fmaf(sc, (float)((w1 >> 16) & 0xff), -of), fmaf(sc, (float)(w1 >> 24), -of));
  gbf16x8 r;
  __builtin_memcpy(&r, p, 16);
  return r;
}

// Raw weight bytes of one tile column for this lane's quarter q (LDS reads), then the decode of
// fragment s (k 8q.. for s = 0, 32 + 8q.. for s = 1) -- split so the decode can sit between MFMAs.
struct PfBRaw {
  uint2 cw;       // 8 code bytes: low nibbles = fragment 0, high nibbles = fragment 1
  uint4 mt;       // Q4_K scale record | bf16: fragment 0
  uint2 hb;       // Q6_K high bits {run 0, run 1}
  uint32_t scw;   // Q6_K int8 scale pairs
  uint32_t dw;    // Q6_K dword holding d
  uint4 b1;       // bf16: fragment 1
};

template <int QT, int S>
__device__ __forceinline__ gbf16x8 pf_bdec(const PfBRaw& r, int q, int kt, int dpar) {
  gbf16x8 f;
  if constexpr (QT == QT_BF16) {
    const uint4 v = S == 0 ? r.mt : r.b1;
    __builtin_memcpy(&f, &v, 16);
  } else if constexpr (QT == QT_Q8_0) {  // (pf8 body) fragment S = the K-step's 32-block S: cw / b1.xy
    const uint32_t w0 = (S == 0 ? r.cw.x : r.b1.x) ^ 0x80808080u, w1 = (S == 0 ? r.cw.y : r.b1.y) ^ 0x80808080u;
    const float d = h2f((uint16_t)(r.scw >> (16 * S)));
    f = pf_dq8(w0, w1, d, 128.f * d);
  } else if constexpr (QT == QT_Q4_0) {  // block S: weights 8q.. = low nibbles (q < 2) / high (q >= 2)
    const int sh = 4 * (q >> 1);
    const uint32_t w0 = ((S == 0 ? r.cw.x : r.b1.x) >> sh) & 0x0f0f0f0fu, w1 = ((S == 0 ? r.cw.y : r.b1.y) >> sh) & 0x0f0f0f0fu;
    const float d = h2f((uint16_t)(r.scw >> (16 * S)));
    f = pf_dq8(w0, w1, d, 8.f * d);
  } else if constexpr (QT == QT_Q6_K) {
    const float d = h2f((uint16_t)(r.dw >> (16 * dpar)));
    const float ds = d * (float)(int8_t)((r.scw >> (16 * (q >> 1) + 8 * S)) & 0xff);
    const uint32_t hv = S == 0 ? r.hb.x : r.hb.y;
    const int j0 = 2 * (q & 1);  // code words j0, j0 + 1 of the chunk
    const uint32_t c0 = S == 0 ? (r.cw.x & 0x0f0f0f0fu) : ((r.cw.x >> 4) & 0x0f0f0f0fu);
    const uint32_t c1 = S == 0 ? (r.cw.y & 0x0f0f0f0fu) : ((r.cw.y >> 4) & 0x0f0f0f0fu);
    f = pf_dq8(c0 | (((hv >> (2 * j0)) & 0x03030303u) << 4), c1 | (((hv >> (2 * j0 + 2)) & 0x03030303u) << 4), ds,
               32.f * ds);
  } else {  // Q4_K
    const float d = h2f((uint16_t)(r.mt.x & 0xffff)), dmin = h2f((uint16_t)(r.mt.x >> 16));
    const uint32_t fl = kq_field(r.mt.y, r.mt.z, r.mt.w, kt & 3);
    const float ds = d * (float)((fl >> (6 * S)) & 63), dm = dmin * (float)((fl >> (12 + 6 * S)) & 63);
    uint32_t c0 = S == 0 ? (r.cw.x & 0x0f0f0f0fu) : ((r.cw.x >> 4) & 0x0f0f0f0fu);
    uint32_t c1 = S == 0 ? (r.cw.y & 0x0f0f0f0fu) : ((r.cw.y >> 4) & 0x0f0f0f0fu);
    if constexpr (QT == QT_Q5_K) {  // (pf8 body) qh bytes 8q.. in hb: bit 2g + S
      const int sh = 2 * (kt & 3) + S;
      c0 |= ((r.hb.x >> sh) & 0x01010101u) << 4;
      c1 |= ((r.hb.y >> sh) & 0x01010101u) << 4;
    }
    f = pf_dq8(c0, c1, ds, dm);
  }
  return f;
}

// ---- 32x32x16 fragments (pf4): a wave's BM rows x 32 columns are BM/32 accumulators of
// v_mfma_f32_32x32x16_bf16.  Per 64-deep K-step four k16 substeps s = 0..3 at k = 16s + 8h + j
// (h = lane >> 5): chunk (s & 1)'s bytes 8h .. 8h+7, low nibbles for s < 2, high nibbles for s >= 2 --
// again the MFMA's natural k layout, so A fragments are 16-B row reads at unit 2s + h.  Per MFMA (32
// cycles, vector issue held for 8) there is room for ~6 fillers against ~2 on 16x16x32.
struct PfBRaw32 {
  uint2 c0, c1;   // 8 code bytes of chunk 0 / chunk 1
  uint4 mt;       // Q4_K scale record | Q6_K high bits {c0 run0, c0 run1, c1 run0, c1 run1} | bf16 fragment 0
  uint32_t scw;   // Q6_K int8 scales {c0 run0, c0 run1, c1 run0, c1 run1}
  uint32_t dw;    // Q6_K dword holding d
  uint4 b1, b2, b3;  // bf16 fragments 1..3
};

template <int QT, int S>
__device__ __forceinline__ gbf16x8 pf_bdec32(const PfBRaw32& r, int h, int kt, int dpar) {
  gbf16x8 f;
  if constexpr (QT == QT_BF16) {
    const uint4 v = S == 0 ? r.mt : (S == 1 ? r.b1 : (S == 2 ? r.b2 : r.b3));
    __builtin_memcpy(&f, &v, 16);
  } else if constexpr (QT == QT_Q8_0) {  // int8 codes (+128 -> the unsigned decode), d of block S >> 1
    const uint32_t w0 = (S == 0 ? r.c0.x : (S == 1 ? r.c1.x : (S == 2 ? r.b1.x : r.b1.z))) ^ 0x80808080u;
    const uint32_t w1 = (S == 0 ? r.c0.y : (S == 1 ? r.c1.y : (S == 2 ? r.b1.y : r.b1.w))) ^ 0x80808080u;
    const float d = h2f((uint16_t)(r.scw >> (16 * (S >> 1))));
    f = pf_dq8(w0, w1, d, 128.f * d);
  } else if constexpr (QT == QT_Q4_0) {  // block S >> 1: low nibbles = weights 0..15, high = 16..31
    const uint2 cw = (S >> 1) ? r.c1 : r.c0;
    const uint32_t w0 = (S & 1) ? ((cw.x >> 4) & 0x0f0f0f0fu) : (cw.x & 0x0f0f0f0fu);
    const uint32_t w1 = (S & 1) ? ((cw.y >> 4) & 0x0f0f0f0fu) : (cw.y & 0x0f0f0f0fu);
    const float d = h2f((uint16_t)(r.scw >> (16 * (S >> 1))));
    f = pf_dq8(w0, w1, d, 8.f * d);
  } else {
    const uint2 cw = (S & 1) ? r.c1 : r.c0;
    const uint32_t w0 = (S < 2) ? (cw.x & 0x0f0f0f0fu) : ((cw.x >> 4) & 0x0f0f0f0fu);
    const uint32_t w1 = (S < 2) ? (cw.y & 0x0f0f0f0fu) : ((cw.y >> 4) & 0x0f0f0f0fu);
    if constexpr (QT == QT_Q6_K) {
      // run (S >> 1) of chunk (S & 1): high-bit word and int8 scale
      constexpr int idx = 2 * (S & 1) + (S >> 1);
      const uint32_t hv = idx == 0 ? r.mt.x : (idx == 1 ? r.mt.y : (idx == 2 ? r.mt.z : r.mt.w));
      const float d = h2f((uint16_t)(r.dw >> (16 * dpar)));
      const float ds = d * (float)(int8_t)((r.scw >> (8 * idx)) & 0xff);
      const int j0 = 2 * h;  // code words 2h, 2h + 1 of the chunk
      f = pf_dq8(w0 | (((hv >> (2 * j0)) & 0x03030303u) << 4), w1 | (((hv >> (2 * j0 + 2)) & 0x03030303u) << 4), ds,
                 32.f * ds);
    } else {  // Q4_K / Q5_K: sub-block 2g (S < 2) or 2g + 1
      const float d = h2f((uint16_t)(r.mt.x & 0xffff)), dmin = h2f((uint16_t)(r.mt.x >> 16));
      const uint32_t fl = kq_field(r.mt.y, r.mt.z, r.mt.w, kt & 3);
      constexpr int sb = S >> 1;
      const float ds = d * (float)((fl >> (6 * sb)) & 63), dm = dmin * (float)((fl >> (12 + 6 * sb)) & 63);
      if constexpr (QT == QT_Q5_K) {  // + bit (2g + hi) of the weights' qh bytes as bit 4
        const int sh = 2 * (kt & 3) + sb;
        const uint32_t h0 = (S & 1) ? r.b1.z : r.b1.x, h1 = (S & 1) ? r.b1.w : r.b1.y;
        f = pf_dq8(w0 | (((h0 >> sh) & 0x01010101u) << 4), w1 | (((h1 >> sh) & 0x01010101u) << 4), ds, dm);
      } else {
        f = pf_dq8(w0, w1, ds, dm);
      }
    }
  }
  return f;
}


// ==== pf4: 4 waves (one per SIMD) x WC columns each, 32x32x16 MFMA, accumulators in AGPRs ============
// Measured in round 5 (timing probes + rocprofv3 PMC, gate/up M = 2048) on the first bodies, which
// shared one DMA among 8 waves and decoded at the step head: the two waves of a SIMD raced for its
// matrix pipe, the leader then idled at every per-step barrier (SQ_WAIT_ANY 148M vs 55M quad-cycles
// without the barrier) while the step head -- fragment reads and the B decode -- ran with the pipe
// idle; the runtime piece selection of the shared DMA added ~68 SALU per wave-step.  Here each wave
// owns its SIMD, DMAs its OWN weight columns (so it can wait for, read and decode step t+1's B
// fragments with its own vmcnt, before the barrier, inside step t's last phases) and every DMA
// piece is compile-time: one vmcnt immediate per wave.
//
// Formats beyond Q4_K / Q6_K / bf16 read the GEMV engines' planes
// (quant_pack.hip) in place -- no second copy of any weight:
//   Q5_K  = the Q4_K codes + record, plus the block's 32 qh bytes (bit 2g + hi of byte l = high bit of
//           weight 64g + 32hi + l) fetched with every K-step as one more 1 KB piece;
//   Q4_0  = 32-weight blocks: the K-step's two 16-B code blocks (the Q4_K code reads, a different
//           nibble <-> fragment map) + the dword holding both blocks' f16 d (4-B piece, as Q6_K's scales);
//   Q8_0  = row-major int8 codes, 64 B per column per K-step (two 1 KB pieces) + the d-pair dword.
template <int QT>
struct PfFmt {
  static constexpr bool Q6 = QT == QT_Q6_K, BF = QT == QT_BF16, Q5 = QT == QT_Q5_K, L0 = QT == QT_Q4_0,
                        L8 = QT == QT_Q8_0, KREC = QT == QT_Q4_K || QT == QT_Q5_K;
};
#ifndef AIOS_PF4_NS
#define AIOS_PF4_NS 3
#endif
template <int QT, int BM, int WC, int NW = 4>
struct Pf4Layout {
  using F = PfFmt<QT>;
  static constexpr bool Q6 = F::Q6, BF = F::BF, Q5 = F::Q5, L0 = F::L0, L8 = F::L8;
  static constexpr int A_BYTES = BM * 128;
  // per wave: bf16 rows / Q8_0 bytes / 2 code chunks per column
  static constexpr int CODE = BF ? WC * 128 : (L8 ? WC * 64 : WC * 32);
  static constexpr int META = (F::KREC || Q6) ? (WC * 16 > 1024 ? WC * 16 : 1024) : 0;  // K record / Q6_K high bits
  static constexpr int HB = Q5 ? WC * 32 : 0;                                             // Q5_K qh bytes
  static constexpr int SC = (Q6 || L0 || L8) ? 256 : 0;  // Q6_K int8 scales / Q4_0, Q8_0 d pair (4-B pieces)
  static constexpr int DW = Q6 ? 256 : 0;                // Q6_K d dword
  static constexpr int OFF_META = CODE, OFF_HB = OFF_META + META, OFF_SC = OFF_HB + HB, OFF_DW = OFF_SC + SC;
  static constexpr int WB = OFF_DW + DW;                 // one wave's weight bytes per slot
  static constexpr int OFF_B = A_BYTES;
  static constexpr int SLOT = (A_BYTES + NW * WB + 255) / 256 * 256;
  // ring depth: as many slots as 160 KB of LDS holds, up to AIOS_PF4_NS (deeper rings keep more K-steps of
  // DMA in flight for the one workgroup per CU; the counted waits are (NS - 1) / (NS - 2) x PW)
  static constexpr int NS_FIT = (160 * 1024) / SLOT;
  static constexpr int NS = NS_FIT < AIOS_PF4_NS ? NS_FIT : AIOS_PF4_NS;
  static constexpr int NA = BM / (8 * NW), NCODE = CODE / 1024, NMETA = META / 1024, NHB = HB / 1024,
                       NSC = SC / 256, ND = DW / 256;
  static constexpr int PW = NA + NCODE + NMETA + NHB + NSC + ND;  // DMA instructions per wave per slot
  static_assert(CODE % 1024 == 0 && HB % 1024 == 0 && WC * 4 <= 256 && PW <= 31 && NA * 8 * NW == BM, "pf4 slot");
  static_assert(NS >= 2 && (NS - 1) * PW <= 63, "pf4 ring depth / vmcnt immediate");
};

template <int QT, int BM, int WC, int NW = 4>
struct Pf4Dma {
  using L = Pf4Layout<QT, BM, WC, NW>;
  uint32_t off[L::PW];

  __device__ __forceinline__ void init(const GemmQArgs& a, int wcol0, int m0, int wv) {
    const int lane = threadIdx.x & 63;
    const uint32_t nbk = (uint32_t)a.K >> 8;
    static_for<L::PW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      uint32_t o;
      if constexpr (i < L::NA) {  // A piece j = NW i + wv: unit p -> row p>>3, logical unit (p&7) ^ ((row>>1)&7)
        const int p = 64 * (NW * i + wv) + lane, row = p >> 3, c = (p & 7) ^ ((row >> 1) & 7);
        const int m = min(m0 + row, a.M - 1);
        o = ((uint32_t)m * (uint32_t)a.lda + (uint32_t)(c * 8)) * 2u;
      } else if constexpr (i < L::NA + L::NCODE) {
        const int p = 64 * (i - L::NA) + lane;
        if constexpr (L::BF) {
          const int col = p >> 3, c = (p & 7) ^ ((col >> 1) & 7);
          o = ((uint32_t)(wcol0 + col) * (uint32_t)a.K + (uint32_t)(c * 8)) * 2u;
        } else if constexpr (L::L8) {  // 4 x 16 B per column
          const int col = p >> 2, u = p & 3;
          o = (uint32_t)(wcol0 + col) * nbk * 256u + (uint32_t)u * 16u;
        } else {
          const int col = p >> 1, hh = p & 1;
          o = (uint32_t)(wcol0 + col) * nbk * 128u + (uint32_t)hh * 16u;
        }
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA) {
        const uint32_t row = (uint32_t)(wcol0 + (lane & (WC - 1)));
        o = L::Q6 ? row * nbk * 64u : row * nbk * 16u;
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA + L::NHB) {  // Q5_K qh: 2 x 16 B per column
        o = (uint32_t)(wcol0 + (lane >> 1)) * nbk * 32u + (uint32_t)(lane & 1) * 16u;
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA + L::NHB + L::NSC) {
        o = (uint32_t)(wcol0 + (lane & (WC - 1))) * nbk * 16u;  // (Q4_0 / Q8_0: K / 16 bytes of d per row)
      } else {
        o = (uint32_t)(wcol0 + (lane & (WC - 1))) * nbk;
      }
      off[i] = o;
    });
  }

  // K-step kt into the slot at LDS byte address dst (wave-uniform)
  __device__ __forceinline__ void issue(const GemmQArgs& a, const QWeight& w, int kt, uint32_t dst, int wv) const {
    const uint32_t wb = dst + L::OFF_B + (uint32_t)wv * L::WB;
    static_for<L::PW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if constexpr (i < L::NA) {
        pf_glds16((const uint8_t*)a.A + kt * 128 + off[i], dst + (NW * i + wv) * 1024);
      } else if constexpr (i < L::NA + L::NCODE) {
        pf_glds16(w.p0 + (L::BF ? kt * 128 : (L::L8 ? kt * 64 : kt * 32)) + off[i], wb + (i - L::NA) * 1024);
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA) {
        pf_glds16(w.p1 + (L::Q6 ? kt * 16 : (kt >> 2) * 16) + off[i], wb + L::OFF_META);
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA + L::NHB) {
        pf_glds16(w.p2 + (kt >> 2) * 32 + off[i], wb + L::OFF_HB);
      } else if constexpr (i < L::NA + L::NCODE + L::NMETA + L::NHB + L::NSC) {
        pf_glds4((L::Q6 ? w.p2 : w.p1) + kt * 4 + off[i], wb + L::OFF_SC);
      } else {
        pf_glds4(w.p3 + (((off[i] + (uint32_t)(kt >> 2)) >> 1) << 2), wb + L::OFF_DW);
      }
    });
  }
};

// raw B bytes of tile column cl (0..WC-1 of this wave) for lane half h
template <int QT, int BM, int WC>
__device__ __forceinline__ void pf4_braw(const uint8_t* wbase, int cl, int h, PfBRaw32& r) {
  using L = Pf4Layout<QT, BM, WC>;
  if constexpr (L::BF) {
    const uint8_t* row = wbase + cl * 128;
    const int x = (cl >> 1) & 7;
    r.mt = *(const uint4*)(row + (((0 + h) ^ x) << 4));
    r.b1 = *(const uint4*)(row + (((2 + h) ^ x) << 4));
    r.b2 = *(const uint4*)(row + (((4 + h) ^ x) << 4));
    r.b3 = *(const uint4*)(row + (((6 + h) ^ x) << 4));
  } else if constexpr (L::L8) {  // fragment s: bytes 16 s + 8 h .. of the column's 64
    const uint8_t* row = wbase + cl * 64 + 8 * h;
    r.c0 = *(const uint2*)(row);
    r.c1 = *(const uint2*)(row + 16);
    const uint2 c2 = *(const uint2*)(row + 32), c3 = *(const uint2*)(row + 48);
    r.b1 = make_uint4(c2.x, c2.y, c3.x, c3.y);
    r.scw = *(const uint32_t*)(wbase + L::OFF_SC + cl * 4);
  } else {
    r.c0 = *(const uint2*)(wbase + cl * 32 + 8 * h);
    r.c1 = *(const uint2*)(wbase + cl * 32 + 16 + 8 * h);
    if constexpr (L::META > 0) r.mt = *(const uint4*)(wbase + L::OFF_META + cl * 16);
    if constexpr (L::Q5) {  // qh bytes 8 h .. and 16 + 8 h .. of the block's 32
      const uint2 q0 = *(const uint2*)(wbase + L::OFF_HB + cl * 32 + 8 * h);
      const uint2 q1 = *(const uint2*)(wbase + L::OFF_HB + cl * 32 + 16 + 8 * h);
      r.b1 = make_uint4(q0.x, q0.y, q1.x, q1.y);
    }
    if constexpr (L::SC > 0) r.scw = *(const uint32_t*)(wbase + L::OFF_SC + cl * 4);
    if constexpr (L::Q6) r.dw = *(const uint32_t*)(wbase + L::OFF_DW + cl * 4);
  }
}

template <int QT, int BM, int WC, int EPI>
__device__ __forceinline__ void pf4_body(const GemmQArgs& a, int m0, int n0, int seg, int kt0, int kt1, int S) {
  using L = Pf4Layout<QT, BM, WC>;
  constexpr int MT = BM / 32, CT = WC / 32, NS = L::NS, PW = L::PW;
  extern __shared__ __attribute__((aligned(16))) uint8_t pf_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  QWeight w;  // field-wise uniform selects (a dynamically indexed struct copy goes to scratch)
  w.qtype = QT;
  w.rows = seg == 0 ? a.seg[0].rows : (seg == 1 ? a.seg[1].rows : a.seg[2].rows);
  w.cols = a.K;
  w.pad_ = 0;
  w.p0 = seg == 0 ? a.seg[0].p0 : (seg == 1 ? a.seg[1].p0 : a.seg[2].p0);
  w.p1 = seg == 0 ? a.seg[0].p1 : (seg == 1 ? a.seg[1].p1 : a.seg[2].p1);
  w.p2 = seg == 0 ? a.seg[0].p2 : (seg == 1 ? a.seg[1].p2 : a.seg[2].p2);
  w.p3 = seg == 0 ? a.seg[0].p3 : (seg == 1 ? a.seg[1].p3 : a.seg[2].p3);
  const int wcol0 = n0 - (seg == 0 ? a.seg_n0[0] : (seg == 1 ? a.seg_n0[1] : a.seg_n0[2])) + wv * WC;
  const uint32_t nbk = (uint32_t)a.K >> 8;
  const int r32 = lane & 31, h = lane >> 5;

  gf32x16 acc[MT][CT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][c][e] = 0.f;

  const int nk = kt1 - kt0;
  Pf4Dma<QT, BM, WC> dma;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(pf_lds_addr(pf_smem));
  dma.init(a, wcol0, m0, wv);
  // Pipeline: NS slots, all NS filled ahead.  The barrier B(t+1) sits inside step t's last phase,
  // between its two MFMA halves: by then every wave has waited for its own step-(t+1) pieces
  // (phase 1) and holds step t's last fragments in registers, so slot t is free for DMA(t + NS) and
  // step t+1's first A reads fly under the remaining MFMAs.  The loop is branch-free (a branch splits
  // the scheduling region and, here, made the allocator shuttle accumulators between AGPRs and
  // VGPRs): past the last step the DMA re-loads step nk-1 into the free slot and the decode reads a
  // stale slot, neither ever consumed; every DMA is drained before the epilogue.
  const int klast = kt1 - 1;
#pragma unroll
  for (int p = 0; p < NS; ++p) dma.issue(a, w, min(kt0 + p, klast), lds0 + p * L::SLOT, wv);

  // B fragments: bf[c][s] is consumed by phase s; the next step's fragment s is decoded into it in
  // the phase after (s = 0..2 in phases 1..3 of this step, s = 3 in phase 0 of the next), from raw
  // bytes read once per column in phase 1 -- one fragment per column per phase, no second set.
  gbf16x8 bf[CT][4], fa[MT], fb[MT];
  PfBRaw32 raw[CT];
  int rkt = kt0;  // K-step of raw
  auto read_raw = [&](const uint8_t* sl, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CT; ++c) pf4_braw<QT, BM, WC>(sl + L::OFF_B + wv * L::WB, 32 * c + r32, h, raw[c]);
    rkt = kt;
  };
  auto dec = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S4 = decltype(sc)::value;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int cl = 32 * c + r32;
      const int dpar = L::Q6 ? (int)(((uint32_t)(wcol0 + cl) * nbk + (uint32_t)(rkt >> 2)) & 1u) : 0;
      bf[c][S4] = pf_bdec32<QT, S4>(raw[c], h, rkt, dpar);
      // pinned here: LLVM otherwise sinks the arithmetic to its first use (the next step, past the
      // barrier), where it ran serially with the matrix pipe idle
      asm volatile("" : "+v"(bf[c][S4]));
    }
  };
  auto ldA = [&](const uint8_t* sl, gbf16x8(&f)[MT], int sp) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int row = 32 * i + r32;
      const uint4 av = *(const uint4*)(sl + row * 128 + (((2 * sp + h) ^ ((row >> 1) & 7)) << 4));
      __builtin_memcpy(&f[i], &av, 16);
    }
  };
  auto mfma_range = [&](const gbf16x8(&f)[MT], int sp, int k0, int k1) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < MT * CT; ++k) {
      if (k < k0 || k >= k1) continue;
      const int c = k / MT, i = k % MT;
      acc[i][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[i], bf[c][sp], acc[i][c], 0, 0, 0);
    }
  };
  constexpr int NMF = MT * CT, HALF = NMF / 2;
  // step kt0's own pieces (NS - 1 younger steps in flight)
  pf_vmcnt<(NS - 1) * PW>();
  read_raw(pf_smem, kt0);
  dec(std::integral_constant<int, 0>{});
  dec(std::integral_constant<int, 1>{});
  dec(std::integral_constant<int, 2>{});
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  pf_barrier();
  ldA(pf_smem, fa, 0);

  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    const uint8_t* slot = pf_smem + cur * L::SLOT;
    const int nxt = cur == NS - 1 ? 0 : cur + 1;
    __builtin_amdgcn_sched_barrier(0);
    // phase 0: step t's fragment 3
    ldA(slot, fb, 1);
    dec(std::integral_constant<int, 3>{});
    mfma_range(fa, 0, 0, NMF);
    __builtin_amdgcn_sched_barrier(0);
    // phase 1: own step-(t+1) pieces landed (NS - 2 younger steps in flight) -> raw bytes, fragment 0
    ldA(slot, fa, 2);
    pf_vmcnt<(NS - 2) * PW>();
    read_raw(pf_smem + nxt * L::SLOT, kt0 + t + 1);
    dec(std::integral_constant<int, 0>{});
    mfma_range(fb, 1, 0, NMF);
    __builtin_amdgcn_sched_barrier(0);
    // phase 2
    ldA(slot, fb, 3);
    dec(std::integral_constant<int, 1>{});
    mfma_range(fa, 2, 0, NMF);
    __builtin_amdgcn_sched_barrier(0);
    // phase 3: half the MFMAs; B(t+1); step t+1's first reads, DMA(t + NS) into slot t, fragment 2
    // of step t+1, under the other half
    mfma_range(fb, 3, 0, HALF);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pf_barrier();
    ldA(pf_smem + nxt * L::SLOT, fa, 0);
    dma.issue(a, w, min(kt0 + t + NS, klast), lds0 + cur * L::SLOT, wv);
    dec(std::integral_constant<int, 2>{});
    mfma_range(fb, 3, HALF, NMF);
    cur = nxt;
  }
  pf_vmcnt<0>();  // no LDS-DMA may land after this workgroup's LDS is released

  // epilogue -- C/D map of the 32x32 accumulator: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int n = n0 + wv * WC + 32 * c + r32;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        pf_store<EPI>(a, m0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h, n, acc[i][c][e], !(r32 & 1), S);
  }
}

// ==== pf8: 8 waves (two per SIMD) x 32 columns, 16x16x32 MFMA ======================================
// With the DMA taken out, 8 waves on 16x16x32 ran at 1.33 PF per busy CU against 1.16 for pf4's one
// wave per SIMD (measured in round 5: the SIMD's second wave covers the first's LDS latencies); this
// is that geometry with pf4's structure: compile-time own-column DMA pieces, the next step's B decode inside this
// step's phases, the barrier between the two halves of the last phase, a branch-free loop.
template <int QT, int BM, int EPI>
__device__ __forceinline__ void pf8_body(const GemmQArgs& a, int m0, int n0, int seg, int kt0, int kt1, int S) {
  constexpr int NW = 8, WC = 32;
  using L = Pf4Layout<QT, BM, WC, NW>;
  constexpr int MT = BM / 16, GR = MT < 8 ? MT : 8, NG = MT / GR, NPH = 2 * NG, NS = L::NS, PW = L::PW;
  extern __shared__ __attribute__((aligned(16))) uint8_t pf_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  QWeight w;  // field-wise uniform selects (a dynamically indexed struct copy goes to scratch)
  w.qtype = QT;
  w.rows = seg == 0 ? a.seg[0].rows : (seg == 1 ? a.seg[1].rows : a.seg[2].rows);
  w.cols = a.K;
  w.pad_ = 0;
  w.p0 = seg == 0 ? a.seg[0].p0 : (seg == 1 ? a.seg[1].p0 : a.seg[2].p0);
  w.p1 = seg == 0 ? a.seg[0].p1 : (seg == 1 ? a.seg[1].p1 : a.seg[2].p1);
  w.p2 = seg == 0 ? a.seg[0].p2 : (seg == 1 ? a.seg[1].p2 : a.seg[2].p2);
  w.p3 = seg == 0 ? a.seg[0].p3 : (seg == 1 ? a.seg[1].p3 : a.seg[2].p3);
  const int wcol0 = n0 - (seg == 0 ? a.seg_n0[0] : (seg == 1 ? a.seg_n0[1] : a.seg_n0[2])) + wv * WC;
  const uint32_t nbk = (uint32_t)a.K >> 8;
  const int r16 = lane & 15, q = lane >> 4;

  gf32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[i][c] = gf32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = kt1 - kt0, klast = kt1 - 1;
  Pf4Dma<QT, BM, WC, NW> dma;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(pf_lds_addr(pf_smem));
  dma.init(a, wcol0, m0, wv);
#pragma unroll
  for (int p = 0; p < NS; ++p) dma.issue(a, w, min(kt0 + p, klast), lds0 + p * L::SLOT, wv);

  gbf16x8 bf[2][2], fa[GR], fb[GR];
  PfBRaw raw[2];
  int rkt = kt0;
  auto read_raw = [&](const uint8_t* sl, int kt) __attribute__((always_inline)) {
    const uint8_t* wb = sl + L::OFF_B + wv * L::WB;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cl = 16 * c + r16;
      PfBRaw& r = raw[c];
      if constexpr (L::BF) {
        r.mt = *(const uint4*)(wb + cl * 128 + (((0 + q) ^ ((cl >> 1) & 7)) << 4));
        r.b1 = *(const uint4*)(wb + cl * 128 + (((4 + q) ^ ((cl >> 1) & 7)) << 4));
      } else if constexpr (L::L8 || L::L0) {  // the K-step's two 32-blocks: bytes of fragment 0 / 1
        const int bs = L::L8 ? 32 : 16, o = L::L8 ? 8 * q : 8 * (q & 1);
        r.cw = *(const uint2*)(wb + cl * (2 * bs) + o);
        const uint2 c1 = *(const uint2*)(wb + cl * (2 * bs) + bs + o);
        r.b1.x = c1.x;
        r.b1.y = c1.y;
        r.scw = *(const uint32_t*)(wb + L::OFF_SC + cl * 4);
      } else {
        r.cw = *(const uint2*)(wb + cl * 32 + 8 * q);
        if constexpr (L::Q5) r.hb = *(const uint2*)(wb + L::OFF_HB + cl * 32 + 8 * q);
        if constexpr (L::Q6) {
          r.hb = *(const uint2*)(wb + L::CODE + cl * 16 + 8 * (q >> 1));
          r.scw = *(const uint32_t*)(wb + L::CODE + L::META + cl * 4);
          r.dw = *(const uint32_t*)(wb + L::OFF_DW + cl * 4);
        } else {
          r.mt = *(const uint4*)(wb + L::OFF_META + cl * 16);
        }
      }
    }
    rkt = kt;
  };
  auto dec = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S2 = decltype(sc)::value;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cl = 16 * c + r16;
      const int dpar = L::Q6 ? (int)(((uint32_t)(wcol0 + cl) * nbk + (uint32_t)(rkt >> 2)) & 1u) : 0;
      bf[c][S2] = pf_bdec<QT, S2>(raw[c], q, rkt, dpar);
      asm volatile("" : "+v"(bf[c][S2]));  // keep the decode in this phase (else sunk past the barrier)
    }
  };
  auto ldA = [&](const uint8_t* sl, gbf16x8(&f)[GR], int p) __attribute__((always_inline)) {
    const int sp = p / NG, g = p % NG;
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      const int row = 16 * (g * GR + i) + r16;
      const uint4 av = *(const uint4*)(sl + row * 128 + (((4 * sp + q) ^ ((row >> 1) & 7)) << 4));
      __builtin_memcpy(&f[i], &av, 16);
    }
  };
  auto mfma_range = [&](const gbf16x8(&f)[GR], int p, int k0, int k1) __attribute__((always_inline)) {
    const int sp = p / NG, g = p % NG;
#pragma unroll
    for (int k = 0; k < 2 * GR; ++k) {
      if (k < k0 || k >= k1) continue;
      const int c = k / GR, i = k % GR;
      acc[g * GR + i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[i], bf[c][sp], acc[g * GR + i][c], 0, 0, 0);
    }
  };
  pf_vmcnt<(NS - 1) * PW>();
  read_raw(pf_smem, kt0);
  dec(std::integral_constant<int, 0>{});
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  pf_barrier();
  ldA(pf_smem, fa, 0);

  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    const uint8_t* slot = pf_smem + cur * L::SLOT;
    const int nxt = cur == NS - 1 ? 0 : cur + 1;
    static_for<NPH>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      __builtin_amdgcn_sched_barrier(0);
      auto& cf = (p % 2 == 0) ? fa : fb;
      auto& nf = (p % 2 == 0) ? fb : fa;
      if constexpr (p + 1 < NPH) ldA(slot, nf, p + 1);
      if constexpr (p == 0) dec(std::integral_constant<int, 1>{});  // this step's fragment 1
      if constexpr (p == NG) {
        // own pieces of step t+1 landed (NS - 2 younger steps in flight): its raw bytes, fragment 0
        pf_vmcnt<(NS - 2) * PW>();
        read_raw(pf_smem + nxt * L::SLOT, kt0 + t + 1);
        dec(std::integral_constant<int, 0>{});
      }
      if constexpr (p + 1 < NPH) {
        mfma_range(cf, p, 0, 2 * GR);
      } else {
        // last phase: half the MFMAs; B(t+1); the next step's first reads and DMA(t + NS) into slot t
        // under the other half
        mfma_range(cf, p, 0, GR);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pf_barrier();
        ldA(pf_smem + nxt * L::SLOT, nf, 0);
        dma.issue(a, w, min(kt0 + t + NS, klast), lds0 + cur * L::SLOT, wv);
        mfma_range(cf, p, GR, 2 * GR);
      }
    });
    if constexpr (NPH % 2 == 1) {
#pragma unroll
      for (int i = 0; i < GR; ++i) fa[i] = fb[i];
    }
    cur = nxt;
  }
  pf_vmcnt<0>();  // no LDS-DMA may land after this workgroup's LDS is released

  // epilogue -- C/D map of the 16x16 accumulator: col = lane & 15, row = 4 * (lane >> 4) + e
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int n = n0 + wv * WC + 16 * c + r16;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) pf_store<EPI>(a, m0 + 16 * i + 4 * q + e, n, acc[i][c][e], !(r16 & 1), S);
  }
}

// ==== pf8c: pf8 with the K-quant weight planes staged coalesced ==================================
// Measured in round 5: pf8's per-step weight pieces -- each column's 32 B of codes and its 16-B scale
// record, i.e. 32-64 separate rows per DMA instruction -- cost 13-18 % of the kernel against
// contiguous pieces.  (The same staging on v_mfma_f32_32x32x16_bf16 was tried and dropped: 611 vs
// 484 us at gate/up M = 2048.)  Here a wave stages, per HALF block (2 K-steps), 64
// contiguous bytes of codes per column (16 rows x 64 B per DMA: 4 lanes per row, the 16-B units
// XOR-swizzled by (row >> 2) & 3 on the source side so the 8-byte fragment reads are conflict-free),
// per 256-block the scale records (Q4_K meta / Q6_K int8 scales: 16 B per row) and Q6_K d, and the
// Q6_K high bits per half block (32 B per row); double buffers by half-block / block parity.
// Every step issues the same group (so one vmcnt immediate): the per-block / per-half-block planes
// go as partial-lane pieces, one per step (records: 8 rows = 32 lanes x 4 B; Q6_K d: 8 lanes).
// Group G(s), issued at the end of step s (after the barrier B(s+1)), s relative to the slice:
//   A(s + 3); code piece (s & 1) [+ Q6_K high-bit piece (s & 1)] of half block (s + 4) / 2;
//   record piece (s + 6) % 4 [+ Q6_K d piece] of block (s + 6) / 4.
// Every target buffer is free by then (its previous contents were last decoded during step s); the
// data is needed by the decode of the first step using it, at least 1.25 steps later.
template <int QT, int BM>
struct PfcLayout {
  static constexpr int NW = 8, WC = 32, NSA = 3;
  static constexpr bool Q6 = QT == QT_Q6_K;
  static constexpr int A_BYTES = BM * 128;
  static constexpr int OFF_CB = NSA * A_BYTES, CB_W = WC * 64;
  static constexpr int OFF_HB = OFF_CB + 2 * NW * CB_W, HB_W = Q6 ? WC * 32 : 0;  // Q6_K high bits
  static constexpr int OFF_RB = OFF_HB + 2 * NW * HB_W, RB_W = WC * 16;           // records
  static constexpr int OFF_D = OFF_RB + 2 * NW * RB_W, D_W = Q6 ? WC * 4 : 0;
  static constexpr int TOTAL = OFF_D + 2 * NW * D_W;
  static constexpr int NA = BM / 64;
  static constexpr int PW = NA + 2 + (Q6 ? 2 : 0);     // DMA instructions per wave per step
  static constexpr int PRE = NA + 6 + (Q6 ? 6 : 0);    // prologue group: step 0's A, half block 0, block 0
};

template <int QT, int BM>
struct PfcDma {
  using L = PfcLayout<QT, BM>;
  static constexpr int NW = 8;
  uint32_t offA[L::NA], offC[2], offR, offH, offD;

  __device__ __forceinline__ void init(const GemmQArgs& a, int wcol0, int m0, int wv) {
    const int lane = threadIdx.x & 63;
    const uint32_t nbk = (uint32_t)a.K >> 8;
#pragma unroll
    for (int i = 0; i < L::NA; ++i) {
      const int p = 64 * (NW * i + wv) + lane, row = p >> 3, c = (p & 7) ^ ((row >> 1) & 7);
      const int m = min(m0 + row, a.M - 1);
      offA[i] = ((uint32_t)m * (uint32_t)a.lda + (uint32_t)(c * 8)) * 2u;
    }
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int row = 16 * pc + (lane >> 2), u = (lane & 3) ^ ((row >> 2) & 3);
      offC[pc] = (uint32_t)(wcol0 + row) * nbk * 128u + 16u * (uint32_t)u;
    }
    const int l32 = lane & 31;
    offR = (uint32_t)(wcol0 + (l32 >> 2)) * nbk * 16u + 4u * (uint32_t)(l32 & 3);  // + 8 rows per piece
    offH = (uint32_t)(wcol0 + (l32 >> 1)) * nbk * 64u + 16u * (uint32_t)(l32 & 1);  // + 16 rows per piece
    offD = (uint32_t)(wcol0 + (lane & 7)) * nbk;                                      // + 8 rows per piece
  }

  __device__ __forceinline__ void A(const GemmQArgs& a, int kt, uint32_t dst, int wv) const {
#pragma unroll
    for (int i = 0; i < L::NA; ++i) pf_glds16((const uint8_t*)a.A + kt * 128 + offA[i], dst + (NW * i + wv) * 1024);
  }
  // the A pieces i with i % NP == P
  template <int P, int NP>
  __device__ __forceinline__ void A_part(const GemmQArgs& a, int kt, uint32_t dst, int wv) const {
#pragma unroll
    for (int i = 0; i < L::NA; ++i)
      if (i % NP == P) pf_glds16((const uint8_t*)a.A + kt * 128 + offA[i], dst + (NW * i + wv) * 1024);
  }
  // code piece pc of half block hsrc into the wave's half-block buffer at dst
  __device__ __forceinline__ void code(const QWeight& w, int hsrc, int pc, uint32_t dst) const {
    // (a register select: offC[pc] with a runtime pc puts the array in scratch, and the scratch
    // load's vmcnt(0) drained every in-flight DMA)
    pf_glds16(w.p0 + hsrc * 64 + (pc ? offC[1] : offC[0]), dst + pc * 1024);
  }
  // record piece pr (rows 8 pr .. 8 pr + 7) of block bsrc; lanes 0..31
  __device__ __forceinline__ void rec(const QWeight& w, int bsrc, int pr, uint32_t nbk, uint32_t dst) const {
    if ((threadIdx.x & 63) < 32) pf_glds4((L::Q6 ? w.p2 : w.p1) + bsrc * 16 + offR + pr * 128 * nbk, dst + pr * 128);
  }
  // Q6_K high-bit piece pc (rows 16 pc ..) of half block hsrc; lanes 0..31
  __device__ __forceinline__ void hi(const QWeight& w, int hsrc, int pc, uint32_t nbk, uint32_t dst) const {
    if ((threadIdx.x & 63) < 32) pf_glds16(w.p1 + hsrc * 32 + offH + pc * 1024 * nbk, dst + pc * 512);
  }
  // Q6_K d piece pr (rows 8 pr ..) of block bsrc: the dword holding each row's f16 d; lanes 0..7
  __device__ __forceinline__ void dq(const QWeight& w, int bsrc, int pr, uint32_t nbk, uint32_t dst) const {
    if ((threadIdx.x & 63) < 8) pf_glds4(w.p3 + (((offD + pr * 8 * nbk + (uint32_t)bsrc) * 2u) & ~3u), dst + pr * 32);
  }
};

template <int QT, int BM, int EPI>
__device__ __forceinline__ void pf8c_body(const GemmQArgs& a, int m0, int n0, int seg, int kt0, int kt1, int S) {
  using L = PfcLayout<QT, BM>;
  constexpr int NW = 8, WC = 32, NSA = L::NSA, PW = L::PW;
  // row tiles per phase: 4 at BM = 256 (8 phases; 8 ran out of registers once the DMA is spread)
  constexpr int MT = BM / 16, GR = MT >= 16 ? 4 : MT, NG = MT / GR, NPH = 2 * NG;
  extern __shared__ __attribute__((aligned(16))) uint8_t pf_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  QWeight w;  // field-wise uniform selects (a dynamically indexed struct copy goes to scratch)
  w.qtype = QT;
  w.rows = seg == 0 ? a.seg[0].rows : (seg == 1 ? a.seg[1].rows : a.seg[2].rows);
  w.cols = a.K;
  w.pad_ = 0;
  w.p0 = seg == 0 ? a.seg[0].p0 : (seg == 1 ? a.seg[1].p0 : a.seg[2].p0);
  w.p1 = seg == 0 ? a.seg[0].p1 : (seg == 1 ? a.seg[1].p1 : a.seg[2].p1);
  w.p2 = seg == 0 ? a.seg[0].p2 : (seg == 1 ? a.seg[1].p2 : a.seg[2].p2);
  w.p3 = seg == 0 ? a.seg[0].p3 : (seg == 1 ? a.seg[1].p3 : a.seg[2].p3);
  const int wcol0 = n0 - (seg == 0 ? a.seg_n0[0] : (seg == 1 ? a.seg_n0[1] : a.seg_n0[2])) + wv * WC;
  const uint32_t nbk = (uint32_t)a.K >> 8;
  const int r16 = lane & 15, q = lane >> 4;

  gf32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[i][c] = gf32x4{0.f, 0.f, 0.f, 0.f};

  // kt0, kt1 are multiples of 4 (block-aligned slices)
  const int nk = kt1 - kt0, klast = kt1 - 1, hlast = (kt1 >> 1) - 1, blast = (kt1 >> 2) - 1;
  PfcDma<QT, BM> dma;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(pf_lds_addr(pf_smem));
  dma.init(a, wcol0, m0, wv);
  constexpr uint32_t CBS = NW * L::CB_W, HBS = NW * L::HB_W, RBS = NW * L::RB_W, DBS = NW * L::D_W;
  const uint32_t cb = lds0 + L::OFF_CB + wv * L::CB_W, hb = lds0 + L::OFF_HB + wv * L::HB_W;
  const uint32_t rb = lds0 + L::OFF_RB + wv * L::RB_W, db = lds0 + L::OFF_D + wv * L::D_W;
  // G(s): phase-split -- A pieces in the first phases (longest lead), then code (+ high bits), then
  // records (+ d); PH_ALL = every phase (prologue)
  constexpr int PH_ALL = -1;
  auto group = [&](int s, auto phc) __attribute__((always_inline)) {
    constexpr int ph = decltype(phc)::value;
    // A piece i in phase i % NG (all before the decode wait at phase NG)
    if constexpr (ph == PH_ALL) {
      dma.A(a, min(kt0 + s + NSA, klast), lds0 + (uint32_t)(((s + 3 * NSA) % NSA) * L::A_BYTES), wv);
    } else if constexpr (ph < NG) {
      dma.template A_part<(ph < 0 ? 0 : ph), NG>(a, min(kt0 + s + NSA, klast),
                                                 lds0 + (uint32_t)(((s + 3 * NSA) % NSA) * L::A_BYTES), wv);
    }
    const int H = (kt0 >> 1) + ((s + 4) >> 1), B = (kt0 >> 2) + ((s + 6) >> 2), pr = (s + 6) & 3;
    if constexpr (ph == PH_ALL || ph == NPH - 2 || (NPH == 2 && ph == 0)) {
      dma.code(w, min(H, hlast), s & 1, cb + (uint32_t)(H & 1) * CBS);
      if constexpr (L::Q6) dma.hi(w, min(H, hlast), s & 1, nbk, hb + (uint32_t)(H & 1) * HBS);
    }
    if constexpr (ph == PH_ALL || ph == NPH - 1) {
      dma.rec(w, min(B, blast), pr, nbk, rb + (uint32_t)(B & 1) * RBS);
      if constexpr (L::Q6) dma.dq(w, min(B, blast), pr, nbk, db + (uint32_t)(B & 1) * DBS);
    }
  };
  // DMA instructions of G(s-1) issued in step s's phases before the decode wait (phase NG)
  constexpr int NB = 1 + (L::Q6 ? 1 : 0);  // code pieces (+ high bits)
  constexpr int PRE_WAIT = NPH == 2 ? L::NA + NB : L::NA;
  {  // prologue: step 0's A, half block 0, block 0 (PRE instructions), then G(-2), G(-1)
    const int H0 = kt0 >> 1, B0 = kt0 >> 2;
    dma.A(a, kt0, lds0, wv);
    dma.code(w, H0, 0, cb + (uint32_t)(H0 & 1) * CBS);
    dma.code(w, H0, 1, cb + (uint32_t)(H0 & 1) * CBS);
    if constexpr (L::Q6) {
      dma.hi(w, H0, 0, nbk, hb + (uint32_t)(H0 & 1) * HBS);
      dma.hi(w, H0, 1, nbk, hb + (uint32_t)(H0 & 1) * HBS);
    }
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      dma.rec(w, B0, pr, nbk, rb + (uint32_t)(B0 & 1) * RBS);
      if constexpr (L::Q6) dma.dq(w, B0, pr, nbk, db + (uint32_t)(B0 & 1) * DBS);
    }
    group(-2, std::integral_constant<int, PH_ALL>{});
  }

  gbf16x8 bf[2][2], fa[GR], fb[GR];
  PfBRaw raw[2];
  int rkt = kt0;
  // raw bytes of (absolute) K-step kt for this lane's two columns
  auto read_raw = [&](int kt) __attribute__((always_inline)) {
    const int H = kt >> 1, j = kt & 1, B = kt >> 2;
    const uint8_t* cbp = pf_smem + L::OFF_CB + (H & 1) * CBS + wv * L::CB_W;
    const uint8_t* rbp = pf_smem + L::OFF_RB + (B & 1) * RBS + wv * L::RB_W;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int row = 16 * c + r16;
      PfBRaw& r = raw[c];
      r.cw = *(const uint2*)(cbp + row * 64 + (((2 * j + (q >> 1)) ^ ((row >> 2) & 3)) << 4) + 8 * (q & 1));
      if constexpr (L::Q6) {
        r.hb = *(const uint2*)(pf_smem + L::OFF_HB + (H & 1) * HBS + wv * L::HB_W + row * 32 + (2 * j + (q >> 1)) * 8);
        r.scw = *(const uint32_t*)(rbp + row * 16 + 4 * (kt & 3));
        r.dw = *(const uint32_t*)(pf_smem + L::OFF_D + (B & 1) * DBS + wv * L::D_W + row * 4);
      } else {
        r.mt = *(const uint4*)(rbp + row * 16);
      }
    }
    rkt = kt;
  };
  auto dec = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S2 = decltype(sc)::value;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cl = 16 * c + r16;
      const int dpar = L::Q6 ? (int)(((uint32_t)(wcol0 + cl) * nbk + (uint32_t)(rkt >> 2)) & 1u) : 0;
      bf[c][S2] = pf_bdec<QT, S2>(raw[c], q, rkt, dpar);
      asm volatile("" : "+v"(bf[c][S2]));  // keep the decode in this phase (else sunk past the barrier)
    }
  };
  auto ldA = [&](const uint8_t* sl, gbf16x8(&f)[GR], int p) __attribute__((always_inline)) {
    const int sp = p / NG, g = p % NG;
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      const int row = 16 * (g * GR + i) + r16;
      const uint4 av = *(const uint4*)(sl + row * 128 + (((4 * sp + q) ^ ((row >> 1) & 7)) << 4));
      __builtin_memcpy(&f[i], &av, 16);
    }
  };
  auto mfma_range = [&](const gbf16x8(&f)[GR], int p, int k0, int k1) __attribute__((always_inline)) {
    const int sp = p / NG, g = p % NG;
#pragma unroll
    for (int k = 0; k < 2 * GR; ++k) {
      if (k < k0 || k >= k1) continue;
      const int c = k / GR, i = k % GR;
      acc[g * GR + i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[i], bf[c][sp], acc[g * GR + i][c], 0, 0, 0);
    }
  };
  pf_vmcnt<PW>();  // the prologue group landed (G(-2) in flight)
  read_raw(kt0);
  dec(std::integral_constant<int, 0>{});
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  pf_barrier();
  ldA(pf_smem, fa, 0);

  int cur = 0;
  for (int s = 0; s < nk; ++s) {
    const uint8_t* slot = pf_smem + cur * L::A_BYTES;
    const int nxt = cur == NSA - 1 ? 0 : cur + 1;
    static_for<NPH>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      __builtin_amdgcn_sched_barrier(0);
      auto& cf = (p % 2 == 0) ? fa : fb;
      auto& nf = (p % 2 == 0) ? fb : fa;
      if constexpr (p + 1 < NPH) ldA(slot, nf, p + 1);
      if constexpr (p == 0) dec(std::integral_constant<int, 1>{});
      if constexpr (p == NG) {
        // G(s-2) landed -- step s+1's codes / records and this wave's A pieces of it -- with only
        // G(s-1)'s first-phase pieces younger
        pf_vmcnt<PRE_WAIT>();
        read_raw(kt0 + s + 1);  // (past the last step: stale buffers, unused)
        dec(std::integral_constant<int, 0>{});
      }
      // G(s-1): its slot / buffers were released by B(s) (past the end: clamped re-loads, unused)
      group(s - 1, pc);
      if constexpr (p + 1 < NPH) {
        mfma_range(cf, p, 0, 2 * GR);
      } else {
        mfma_range(cf, p, 0, GR);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pf_barrier();
        ldA(pf_smem + nxt * L::A_BYTES, nf, 0);
        mfma_range(cf, p, GR, 2 * GR);
      }
    });
    if constexpr (NPH % 2 == 1) {
#pragma unroll
      for (int i = 0; i < GR; ++i) fa[i] = fb[i];
    }
    cur = nxt;
  }
  pf_vmcnt<0>();  // no LDS-DMA may land after this workgroup's LDS is released

#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int n = n0 + wv * WC + 16 * c + r16;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) pf_store<EPI>(a, m0 + 16 * i + 4 * q + e, n, acc[i][c][e], !(r16 & 1), S);
  }
}

// ==== tiles -> bodies, kernels, launch ============================================================
// stacks whose 256-column tiles run pf8_body (64-weight K-steps, Pf4Layout planes) instead of pf8c:
// bf16, and the Q5_K / Q4_0 / Q8_0 recipes' stacks (their Q6_K segments too)
constexpr bool pf8_generic(int QT0) { return QT0 == QT_BF16 || QT0 == QT_Q5_K || QT0 == QT_Q4_0 || QT0 == QT_Q8_0; }

// The BN-column tiles of a (possibly mixed-format) segment stack: tiles of the last segment run as
// QT1 (the Q4_K_M QKV stack: Q|K Q4_K, V Q6_K), the others as QT0.
template <int QT0_, int QT1_, int BN_>
struct PfTile {
  static constexpr int QT0 = QT0_, QT1 = QT1_, BN = BN_;
  static constexpr int NW = BN / 32, NT = 64 * NW;            // waves of 32 columns; threads per workgroup
  static constexpr bool C = BN == 256 && !pf8_generic(QT0);   // pf8c_body
  static constexpr int KG = C ? 4 : 1;                        // K-steps per slice unit (pf8c slices on 256-blocks)
  static constexpr bool TAIL = BN == 128 || QT0 != QT_BF16;   // 256-row launches may take the tail split
  template <int QT, int BM>
  static constexpr int lds_of() {
    if constexpr (C) return PfcLayout<QT, BM>::TOTAL;
    else return Pf4Layout<QT, BM, 32, NW>::NS * Pf4Layout<QT, BM, 32, NW>::SLOT;
  }
  template <int BM>
  static constexpr int lds() {  // (the larger format's)
    return lds_of<QT0, BM>() > lds_of<QT1, BM>() ? lds_of<QT0, BM>() : lds_of<QT1, BM>();
  }
};

// tile L (column-fastest) of a launch with BM x BN tiles: its first row and column, its segment
struct PfAt {
  int m0, n0, seg;
};
__device__ __forceinline__ PfAt pf_tile(const GemmQArgs& a, int L, int BM, int BN) {
  const int nN = a.N / BN, tn = L % nN, tm = L / nN;
  PfAt t{tm * BM, tn * BN, 0};
  if (a.nseg > 1 && t.n0 >= a.seg_n0[1]) t.seg = 1;
  if (a.nseg > 2 && t.n0 >= a.seg_n0[2]) t.seg = 2;
  return t;
}

// K-steps [kt0, kt1) of tile t on the family's body, as format QT
template <class T, int QT, int BM, int EPI>
__device__ __forceinline__ void pf_body(const GemmQArgs& a, PfAt t, int kt0, int kt1, int S) {
  if constexpr (T::BN == 128) pf4_body<QT, BM, 32, EPI>(a, t.m0, t.n0, t.seg, kt0, kt1, S);
  else if constexpr (T::C) pf8c_body<QT, BM, EPI>(a, t.m0, t.n0, t.seg, kt0, kt1, S);
  else pf8_body<QT, BM, EPI>(a, t.m0, t.n0, t.seg, kt0, kt1, S);
}
// ... in its segment's format.  HALVES (the tail split, BM = 256): half >= 0 runs the 128-row body
// (the choice sits inside the segment branch: the other nesting cost the mixed stacks registers).
template <class T, int BM, int EPI, bool HALVES = false, int QT = T::QT0>
__device__ __forceinline__ void pf_run_tile(const GemmQArgs& a, PfAt t, int kt0, int kt1, int S, int half = -1) {
  if constexpr (QT != T::QT1) {
    if (t.seg == a.nseg - 1) {
      pf_run_tile<T, BM, EPI, HALVES, T::QT1>(a, t, kt0, kt1, S, half);
      return;
    }
  }
  if constexpr (HALVES) {
    if (half < 0) pf_body<T, QT, BM, EPI>(a, t, kt0, kt1, S);
    else pf_body<T, QT, 128, EPI>(a, t, kt0, kt1, S);
  } else {
    pf_body<T, QT, BM, EPI>(a, t, kt0, kt1, S);
  }
}

// One launch for every tile of the stack; gridDim.y = K slices (S > 1: atomic adds).
template <class T, int BM, int EPI>
__global__ void __launch_bounds__(T::NT) gemm_pf_kernel(GemmQArgs a) {
  const int total = (a.N / T::BN) * ((a.M + BM - 1) / BM);
  const PfAt t = pf_tile(a, xcd_remap(blockIdx.x, total), BM, T::BN);
  const int S = gridDim.y, nu = a.K / (64 * T::KG);
  const int kt0 = T::KG * (int)((long)blockIdx.y * nu / S), kt1 = T::KG * (int)((long)(blockIdx.y + 1) * nu / S);
  pf_run_tile<T, BM, EPI>(a, t, kt0, kt1, S);
}

// Tail split (round 5).  A 256-row-tile launch of T tiles runs one workgroup per CU (LDS), so it
// takes ceil(T / CUs) rounds; when the last round is at most half full (R = T mod CUs <= CUs / 2)
// the other CUs idle through it -- Mistral's gate/up at 2048 rows is 896 tiles = 3.5 rounds of 256
// that cost 4.  Here the first F = T - R tiles run as usual and each of the last R runs as TWO
// 128-row workgroups (the BM = 128 body on its half), dispatched last: the final round puts
// half-size work on every CU.  S = 1 (plans with split-K fill the chip their own way).
template <class T, int EPI>
__global__ void __launch_bounds__(T::NT) gemm_pft_kernel(GemmQArgs a, int F) {
  int L, half = -1;
  if ((int)blockIdx.x < F) {
    L = xcd_remap(blockIdx.x, F);
  } else {
    const int j = xcd_remap(blockIdx.x - F, gridDim.x - F);
    L = F + (j >> 1);
    half = j & 1;
  }
  PfAt t = pf_tile(a, L, 256, T::BN);
  t.m0 += half > 0 ? 128 : 0;
  pf_run_tile<T, 256, EPI, true>(a, t, 0, T::KG * (a.K / (64 * T::KG)), 1, half);
}

// full tiles before the tail of a 256 x BN launch, or -1 (no tail split for this shape / plan)
inline int pf_tail_full(const GemmQArgs& a, int BN, int S) {
  const char* e = std::getenv("AIOS_GEMM_PF_TAIL");  // (read per call: tests compare both)
  if ((e && std::atoi(e) == 0) || S != 1 || a.epi == GEPI_QKV) return -1;
  const int T = (a.N / BN) * ((a.M + 255) / 256), C = device_cu_count(), R = T % C;
  return (T > C && R > 0 && 2 * R <= C) ? T - R : -1;
}

// Stream-K (round 6): a launch whose output tiles do not fill the chip -- the N = 4096-6144
// projections of a 512-token chunk have 32-192 tiles for 256 CUs -- runs one workgroup per CU over an
// equal share of the flattened (tile, K unit) iteration space instead of split-K's equal slices of
// every tile: workgroup w takes iterations [w * ipw, (w + 1) * ipw), i.e. the tail of one tile and the
// head of the next, and adds each partial tile into C with the split-K atomics (STORE targets zeroed
// first).  A unit is KG K-steps.  A workgroup that runs a second segment barriers first: the previous
// body's last LDS reads against its prologue DMA.
template <class T, int BM, int EPI>
__global__ void __launch_bounds__(T::NT) gemm_pfsk_kernel(GemmQArgs a, int ipw) {
  const int nN = a.N / T::BN, nM = (a.M + BM - 1) / BM, nk = a.K / (64 * T::KG);
  const long total = (long)nN * nM * nk;
  long it = (long)blockIdx.x * ipw;
  const long end = it + ipw < total ? it + ipw : total;
  bool first = true;
  while (it < end) {
    const int L = (int)(it / nk), k0 = (int)(it - (long)L * nk);
    const int k1 = (int)(k0 + (end - it) < nk ? k0 + (end - it) : nk);
    const PfAt t = pf_tile(a, L, BM, T::BN);
    if (!first) __syncthreads();
    // S: 1 when this workgroup owns the whole tile (plain epilogue), else atomic partials
    pf_run_tile<T, BM, EPI>(a, t, k0 * T::KG, k1 * T::KG, (k0 == 0 && k1 == nk) ? 1 : 2);
    it += k1 - k0;
    first = false;
  }
}

// iterations per workgroup of a stream-K launch over the device's CUs (workgroups = its grid)
inline int pf_sk_ipw(const GemmQArgs& a, int BM, int BN, int KG, int& grid) {
  const long total = (long)(a.N / BN) * ((a.M + BM - 1) / BM) * (a.K / (64 * KG));
  const int cus = device_cu_count();
  // (even: with an even K-step count per tile every segment is >= 2 units, as the split-K slices)
  const int ipw = (int)(((total + cus - 1) / cus + 1) & ~1L);
  grid = (int)((total + ipw - 1) / ipw);
  return ipw;
}

// host: one plan of one tile family.  S < 0: stream-K (STORE / ACCUM only: partial tiles are atomic
// adds); S = 1 at BM = 256 takes the tail split where pf_tail_full says so (never QKV); else tiles x S.
template <class T, int BM>
void pf_launch(const GemmQArgs& a, int S, hipStream_t st) {
  constexpr int lds = T::template lds<BM>();
  static_assert(lds <= 160 * 1024, "LDS");
  const dim3 block(T::NT);
  if (S < 0) {
    int grid = 0;
    const int ipw = pf_sk_ipw(a, BM, T::BN, T::KG, grid);
    if (a.epi == GEPI_STORE) hipLaunchKernelGGL((gemm_pfsk_kernel<T, BM, GEPI_STORE>), dim3(grid), block, lds, st, a, ipw);
    else hipLaunchKernelGGL((gemm_pfsk_kernel<T, BM, GEPI_ACCUM>), dim3(grid), block, lds, st, a, ipw);
    return;
  }
  if constexpr (BM == 256 && T::TAIL) {
    const int F = pf_tail_full(a, T::BN, S);
    if (F >= 0) {
      constexpr int ldst = lds > T::template lds<128>() ? lds : T::template lds<128>();
      const int tiles = (a.N / T::BN) * ((a.M + 255) / 256);
      const dim3 grid(F + 2 * (tiles - F));
      switch (a.epi) {
        case GEPI_STORE: hipLaunchKernelGGL((gemm_pft_kernel<T, GEPI_STORE>), grid, block, ldst, st, a, F); break;
        case GEPI_ACCUM: hipLaunchKernelGGL((gemm_pft_kernel<T, GEPI_ACCUM>), grid, block, ldst, st, a, F); break;
        default: hipLaunchKernelGGL((gemm_pft_kernel<T, GEPI_SWIGLU_BF16>), grid, block, ldst, st, a, F); break;
      }
      return;
    }
  }
  const dim3 grid((a.N / T::BN) * ((a.M + BM - 1) / BM), S);
  switch (a.epi) {
    case GEPI_STORE: hipLaunchKernelGGL((gemm_pf_kernel<T, BM, GEPI_STORE>), grid, block, lds, st, a); break;
    case GEPI_ACCUM: hipLaunchKernelGGL((gemm_pf_kernel<T, BM, GEPI_ACCUM>), grid, block, lds, st, a); break;
    case GEPI_QKV: hipLaunchKernelGGL((gemm_pf_kernel<T, BM, GEPI_QKV>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((gemm_pf_kernel<T, BM, GEPI_SWIGLU_BF16>), grid, block, lds, st, a); break;
  }
}

// the tile set of one format pair (one translation unit each, compiled in parallel)
template <int QT0, int QT1>
bool pf_launch_fmt(const GemmQArgs& a, int BM, int BN, int S, hipStream_t st) {
#define PF_GO(bm, bn)                                \
  if (BM == bm && BN == bn) {                        \
    pf_launch<PfTile<QT0, QT1, bn>, bm>(a, S, st);   \
    return true;                                     \
  }
  PF_GO(256, 256) PF_GO(128, 256) PF_GO(64, 256) PF_GO(256, 128) PF_GO(128, 128) PF_GO(64, 128)
#undef PF_GO
  return false;
}

}  // namespace aios
