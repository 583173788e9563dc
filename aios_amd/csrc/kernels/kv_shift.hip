// Context shift (ops.h KvShiftArgs): move one slot's cached positions [n_keep + n_discard, n) down by
// n_discard, in place, through the slot's row of the device block table.  V rows move as bytes; K rows, which
// are stored with RoPE applied, are rotated by -n_discard positions on the way (fp32, the engine's (cos, sin)
// table row n_discard with the sine negated) and rounded back to the cache type: bf16 round-to-nearest-even,
// fp8 e4m3 decoded and re-encoded with the layer's K scale by the KV writers' own conversion.
//
//  - One launch for every layer: workgroup (kv head, K or V, layer) owns that column of the slot and walks the
//    destination positions [n_keep, n - n_discard) in ascending order, one tile at a time.  Workgroups never
//    touch each other's bytes.
//  - A thread's unit is one 16-byte piece of a row's lower half and the piece at the same offset in its upper
//    half: two 16-byte loads, two 16-byte stores.  For ROPE_NEOX those hold both halves of its pairs (i,
//    i + head_dim / 2); for ROPE_NORM each piece holds whole adjacent pairs.  The piece is fixed per thread, so
//    its (cos, sin) values are loaded once; a thread holds KVS_ROWS rows of a tile in registers.
//  - In place: inside a tile position p's destination is position p - n_discard's source whenever n_discard
//    is smaller than the tile, so every load of a tile has returned (vmcnt(0)) in every wave (workgroup
//    barrier) before any of its stores is issued.  The next tile's sources lie above everything stored so far
//    (n_discard >= 1), so its loads are issued right behind the barrier, in front of this tile's stores.
// No LDS, no scratch, no atomics, no workspace.
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int KVS_THREADS = 256;
constexpr int KVS_ROWS = 2;  // rows (positions) of a tile per thread (two tiles are held: this one and the next)

struct KvsTile {
  uint4 lo[KVS_ROWS], hi[KVS_ROWS];
};

__device__ __forceinline__ void kvs_rot(float& x, float& y, float2 cs) {  // by -angle: (c, -s)
  const float nx = x * cs.x + y * cs.y;
  const float ny = y * cs.x - x * cs.y;
  x = nx;
  y = ny;
}

// 8 bf16 of the lower piece in a, of the upper piece in b; cs: NORM 4 pairs of a then 4 of b, NEOX 8 pairs (a[j], b[j])
template <bool NEOX>
__device__ __forceinline__ void kvs_rotate_bf16(uint4& a, uint4& b, const float2* cs) {
  uint32_t* aw = (uint32_t*)&a;
  uint32_t* bw = (uint32_t*)&b;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float a0 = bf16_to_f32(aw[w] & 0xffffu), a1 = bf16_to_f32(aw[w] >> 16);
    float b0 = bf16_to_f32(bw[w] & 0xffffu), b1 = bf16_to_f32(bw[w] >> 16);
    if (NEOX) {
      kvs_rot(a0, b0, cs[2 * w]);
      kvs_rot(a1, b1, cs[2 * w + 1]);
    } else {
      kvs_rot(a0, a1, cs[w]);
      kvs_rot(b0, b1, cs[4 + w]);
    }
    aw[w] = (uint32_t)f32_to_bf16(a0) | ((uint32_t)f32_to_bf16(a1) << 16);
    bw[w] = (uint32_t)f32_to_bf16(b0) | ((uint32_t)f32_to_bf16(b1) << 16);
  }
}

typedef float kvs_f32x2 __attribute__((ext_vector_type(2)));

// 16 fp8 codes per piece; cs: NORM 8 pairs of a then 8 of b, NEOX 16 pairs (a[j], b[j])
template <bool NEOX>
__device__ __forceinline__ void kvs_rotate_fp8(uint4& a, uint4& b, const float2* cs, float scale, float inv) {
  uint32_t* aw = (uint32_t*)&a;
  uint32_t* bw = (uint32_t*)&b;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const kvs_f32x2 al = __builtin_amdgcn_cvt_pk_f32_fp8((int)aw[w], false);
    const kvs_f32x2 ah = __builtin_amdgcn_cvt_pk_f32_fp8((int)aw[w], true);
    const kvs_f32x2 bl = __builtin_amdgcn_cvt_pk_f32_fp8((int)bw[w], false);
    const kvs_f32x2 bh = __builtin_amdgcn_cvt_pk_f32_fp8((int)bw[w], true);
    float av[4] = {al[0] * scale, al[1] * scale, ah[0] * scale, ah[1] * scale};
    float bv[4] = {bl[0] * scale, bl[1] * scale, bh[0] * scale, bh[1] * scale};
    if (NEOX) {
#pragma unroll
      for (int j = 0; j < 4; ++j) kvs_rot(av[j], bv[j], cs[4 * w + j]);
    } else {
      kvs_rot(av[0], av[1], cs[2 * w]);
      kvs_rot(av[2], av[3], cs[2 * w + 1]);
      kvs_rot(bv[0], bv[1], cs[8 + 2 * w]);
      kvs_rot(bv[2], bv[3], cs[8 + 2 * w + 1]);
    }
    aw[w] = f32x2_to_fp8x2(av[0] * inv, av[1] * inv) | (f32x2_to_fp8x2(av[2] * inv, av[3] * inv) << 16);
    bw[w] = f32x2_to_fp8x2(bv[0] * inv, bv[1] * inv) | (f32x2_to_fp8x2(bv[2] * inv, bv[3] * inv) << 16);
  }
}

template <bool FP8, bool NEOX>
__global__ __launch_bounds__(KVS_THREADS) void kv_shift_kernel(KvShiftArgs a) {
  constexpr int ES = FP8 ? 1 : 2;       // bytes per element
  constexpr int EPP = 16 / ES;          // elements per 16-byte piece
  constexpr int NCS = FP8 ? 16 : 8;     // (cos, sin) pairs a thread applies
  const int kvh = blockIdx.x, is_v = blockIdx.y, layer = blockIdx.z;
  const int hd = a.head_dim, half = hd / 2;
  const int ppr = half / EPP;           // pieces per half row = threads per row
  const int rpp = KVS_THREADS / ppr;    // rows per pass of the workgroup
  const int piece = threadIdx.x % ppr, prow = threadIdx.x / ppr;
  const bool active = prow < rpp;       // (ppr need not divide the workgroup)
  char* pool = (char*)(is_v ? a.v_cache : a.k_cache) + (size_t)layer * a.layer_elems * ES;
  const int e_lo = piece * EPP, e_hi = half + piece * EPP;  // the thread's first elements in a row

  float2 cs[NCS];
  float scale = 1.f, inv = 1.f;
  if (!is_v) {
    const float2* t = a.rope_cs + (size_t)a.n_discard * half;
    if (NEOX) {
#pragma unroll
      for (int j = 0; j < NCS; ++j) cs[j] = t[e_lo + j];
    } else {
#pragma unroll
      for (int j = 0; j < NCS / 2; ++j) {
        cs[j] = t[e_lo / 2 + j];
        cs[NCS / 2 + j] = t[e_hi / 2 + j];
      }
    }
    if (FP8) {
      scale = a.k_scale[layer];
      inv = 1.f / scale;
    }
  }

  const int end = a.n_tokens - a.n_discard;  // destinations are [n_keep, end)
  const int tile = rpp * KVS_ROWS;
  auto offset = [&](int pos) {  // byte offset of the row's first element in the layer pool
    return kv_offset(a.block_table, a.max_blocks, a.slot, a.n_kv_heads, kvh, pos, hd) * ES;
  };
  auto load = [&](KvsTile& t, int p0) {
#pragma unroll
    for (int u = 0; u < KVS_ROWS; ++u) {
      const int p = p0 + u * rpp + prow;
      if (active && p < end) {
        const char* src = pool + offset(p + a.n_discard);
        t.lo[u] = *(const uint4*)(src + e_lo * ES);
        t.hi[u] = *(const uint4*)(src + e_hi * ES);
      }
    }
  };

  KvsTile cur, nxt;
  load(cur, a.n_keep);
  for (int p0 = a.n_keep; p0 < end; p0 += tile) {
    // every load of this tile has returned, in every wave, before any of its stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (p0 + tile < end) load(nxt, p0 + tile);
#pragma unroll
    for (int u = 0; u < KVS_ROWS; ++u) {
      const int p = p0 + u * rpp + prow;
      if (active && p < end) {
        uint4 lo = cur.lo[u], hi = cur.hi[u];
        if (!is_v) {
          if (FP8) kvs_rotate_fp8<NEOX>(lo, hi, cs, scale, inv);
          else kvs_rotate_bf16<NEOX>(lo, hi, cs);
        }
        char* dst = pool + offset(p);
        *(uint4*)(dst + e_lo * ES) = lo;
        *(uint4*)(dst + e_hi * ES) = hi;
      }
    }
    cur = nxt;
  }
}

void launch_kv_shift(const KvShiftArgs& a, hipStream_t st) {
  if (!a.k_cache || !a.v_cache || !a.block_table || !a.rope_cs) throw std::runtime_error("kv_shift: null argument");
  if (a.kv_fp8 && !a.k_scale) throw std::runtime_error("kv_shift: an fp8 cache needs the K scales");
  if (a.n_layers < 1 || a.n_kv_heads < 1 || a.slot < 0 || a.max_blocks < 1)
    throw std::runtime_error("kv_shift: bad shape");
  // a half row is a whole number of 16-byte pieces, at most one workgroup of them
  const int piece = a.kv_fp8 ? 32 : 16;  // elements of a row per thread
  if (a.head_dim < piece || a.head_dim % piece || a.head_dim / piece > KVS_THREADS)
    throw std::runtime_error("kv_shift: head_dim " + std::to_string(a.head_dim) + " is not a multiple of " +
                             std::to_string(piece));
  if (a.n_keep < 0 || a.n_discard < 1 || a.n_keep + a.n_discard > a.n_tokens || a.n_tokens > a.max_blocks * KV_BLOCK)
    throw std::runtime_error("kv_shift: positions out of range");
  if (a.n_keep + a.n_discard == a.n_tokens) return;  // nothing moves
  if (a.n_discard >= a.rope_rows) throw std::runtime_error("kv_shift: n_discard beyond the rotation table");
  const dim3 grid(a.n_kv_heads, 2, a.n_layers);
  auto k = a.kv_fp8 ? (a.rope_neox ? kv_shift_kernel<true, true> : kv_shift_kernel<true, false>)
                    : (a.rope_neox ? kv_shift_kernel<false, true> : kv_shift_kernel<false, false>);
  hipLaunchKernelGGL(k, grid, dim3(KVS_THREADS), 0, st, a);
}

}  // namespace aios
