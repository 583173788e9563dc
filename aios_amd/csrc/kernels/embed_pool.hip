// Text-embedding pooling (ops.h EmbedPoolArgs): fold a chunk of residual rows x[n][ldx] into a running
// per-slot accumulator, in the sampler's / logprob kernel's shape -- 256 threads, slab partials published
// with write-through stores + a ticket, a last-arriver merge.  ONE launch:
//  A) workgroup w takes the contiguous band of rows [w * band, (w + 1) * band), band = ceil(n / 64) (so at
//     most EMBED_MAX_WG = 64 workgroups: one row each up to n = 64, 32 rows each at n = 2048).  It holds one
//     row at a time in registers (PER = ceil(d / 256) floats per lane, column c = j * 256 + tid), reduces the
//     row's sum of squares over the workgroup, and adds x * rsqrt(mean(x^2) + eps) into per-lane column
//     accumulators -- the norm weight g commutes with the sum and is applied once, at the end.  The band's
//     [d] partial goes to slab w of the workspace.
//  B) the last arriving workgroup sums the slabs IN WORKGROUP-INDEX ORDER onto acc (zero when `first`) and
//     adds n to the count.  No float atomics anywhere: the same input gives the same bits on every run.
//     On `final` it also writes out = normalise(acc / count * g): scaled by its largest |component| first
//     (so neither tiny nor huge g leaves fp32's range when squared), then divided by its L2 norm; a result
//     that is exactly zero stays the zero vector (no 0 / 0).
// Chunking: acc after (first, n1) + (n - n1) rows is ((band sums of chunk 1) + (band sums of chunk 2)), a
// different association from one launch of n rows (whose bands differ), so the two agree to fp32 rounding
// of the sum (tests/embed_oracle.py GPU_TOL), NOT bit for bit; each of them is deterministic.
// EMBED_LAST is the single-row case: the launcher passes the chunk's last row with first = 1.
// EMBED_NONE pools nothing: phase A writes h = x * inv_rms * g for its rows to out[n][d] and returns (the
// fp32 rmsnorm launch computes the same, but its float4 loads want 16-byte aligned rows, which a raw-op
// caller's ldx need not give; here every access is a coalesced dword).
// (every register array is indexed by unrolled constants only, and no kernel argument is chosen by a
// pointer select: elementwise.hip's notes on scratch)
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int EP_THREADS = 256;

size_t embed_pool_ws_bytes(int d) { return (size_t)EMBED_MAX_WG * d * 4; }

__device__ __forceinline__ float ep_block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <int PER>
__global__ void __launch_bounds__(EP_THREADS) embed_pool_kernel(EmbedPoolArgs a) {
  __shared__ float red[16];
  __shared__ int s_last;
  const unsigned tid = threadIdx.x, d = a.d;
  const int wg = blockIdx.x, G = gridDim.x;
  const int r0 = wg * a.band, r1 = min(a.n, r0 + a.band);

  // ---- A) this band, one row in registers at a time
  float sum[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) sum[j] = 0.f;
#pragma unroll 1
  for (int r = r0; r < r1; ++r) {
    const float* xr = a.x + (size_t)r * a.ldx;
    float v[PER];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const unsigned c = j * EP_THREADS + tid;
      const float t = xr[c < d ? c : 0];
      v[j] = c < d ? t : 0.f;
      ss += v[j] * v[j];
    }
    ss = block_sum(ss, red);
    const float ir = rsqrtf(ss / (float)d + a.eps);
    if (a.mode == EMBED_NONE) {
      float* orow = a.out + (size_t)r * d;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const unsigned c = j * EP_THREADS + tid;
        if (c < d) orow[c] = v[j] * ir * a.g[c];
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) sum[j] += v[j] * ir;
    }
  }
  if (a.mode == EMBED_NONE) return;

  float* slab = a.ws + (size_t)wg * d;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const unsigned c = j * EP_THREADS + tid;
    if (c < d) __hip_atomic_store(slab + c, sum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(a.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == G - 1);
  }
  __syncthreads();
  if (!s_last) return;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);

  // ---- B) the last arriver: slabs in workgroup order onto acc, then (final) the unit vector
  const int count = (a.first ? 0 : *a.count) + a.n;
  // Slab by slab, a row of PER independent loads in flight.  Plain loads: the slabs were written through to
  // L2 before their tickets, and the acquire fence above dropped this CU's L1.  Lanes past d read column 0
  // (their sums are never used), so no load sits behind a guard and waits for the one before it.
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const unsigned c = j * EP_THREADS + tid;
    sum[j] = 0.f;
    if (c < d && !a.first) sum[j] = a.acc[c];
  }
#pragma unroll 2
  for (int w = 0; w < G; ++w) {
    const float* slab_w = a.ws + (size_t)w * d;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const unsigned c = j * EP_THREADS + tid;
      sum[j] += slab_w[c < d ? c : 0];
    }
  }
  float o[PER];
  float big = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const unsigned c = j * EP_THREADS + tid;
    o[j] = 0.f;
    if (c < d) {
      a.acc[c] = sum[j];
      o[j] = sum[j] / (float)count * a.g[c];
    }
    big = fmaxf(big, fabsf(o[j]));
  }
  if (tid == 0) {
    *a.count = count;
    __hip_atomic_store(a.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  }
  if (!a.final) return;
  big = ep_block_max(big, red);
  float n2 = 0.f;
  if (big > 0.f) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      o[j] /= big;
      n2 += o[j] * o[j];
    }
  }
  n2 = block_sum(n2, red);
  const float nrm = sqrtf(n2);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const unsigned c = j * EP_THREADS + tid;
    if (c < d) a.out[c] = big > 0.f ? o[j] / nrm : 0.f;
  }
}

void launch_embed_pool(const EmbedPoolArgs& args, hipStream_t st) {
  EmbedPoolArgs a = args;
  if (a.d < 64 || a.d > EMBED_MAX_D || a.d % 64)
    throw std::runtime_error("embed_pool: d must be a multiple of 64 in 64.." + std::to_string(EMBED_MAX_D) + ", got " +
                             std::to_string(a.d));
  if (a.n < 1 || a.n > EMBED_MAX_ROWS)
    throw std::runtime_error("embed_pool: rows outside 1.." + std::to_string(EMBED_MAX_ROWS));
  if (a.ldx < a.d) throw std::runtime_error("embed_pool: row stride below d");
  if (a.mode != EMBED_NONE && a.mode != EMBED_MEAN && a.mode != EMBED_LAST)
    throw std::runtime_error("embed_pool: pooling must be 0 (none), 1 (mean) or 3 (last)");
  if (!a.x || !a.g) throw std::runtime_error("embed_pool: null argument");
  if (a.mode == EMBED_NONE) {
    if (!a.out) throw std::runtime_error("embed_pool: none needs the [n][d] output");
  } else {
    if (!a.acc || !a.count || !a.ws || !a.counter) throw std::runtime_error("embed_pool: accumulator, count, workspace and counter required");
    if (a.final && !a.out) throw std::runtime_error("embed_pool: final needs the [d] output");
    if (a.ws_bytes < embed_pool_ws_bytes(a.d)) throw std::runtime_error("embed_pool: workspace too small");
  }
  if (a.mode == EMBED_LAST) {  // the single-row case, on the chunk's last row
    a.x += (size_t)(a.n - 1) * a.ldx;
    a.n = 1;
    a.first = 1;
  }
  a.band = (a.n + EMBED_MAX_WG - 1) / EMBED_MAX_WG;
  const dim3 grid((a.n + a.band - 1) / a.band), block(EP_THREADS);
  const int per = (a.d + EP_THREADS - 1) / EP_THREADS;
  if (per <= 1) hipLaunchKernelGGL(embed_pool_kernel<1>, grid, block, 0, st, a);
  else if (per <= 2) hipLaunchKernelGGL(embed_pool_kernel<2>, grid, block, 0, st, a);
  else if (per <= 4) hipLaunchKernelGGL(embed_pool_kernel<4>, grid, block, 0, st, a);
  else if (per <= 8) hipLaunchKernelGGL(embed_pool_kernel<8>, grid, block, 0, st, a);
  else if (per <= 16) hipLaunchKernelGGL(embed_pool_kernel<16>, grid, block, 0, st, a);
  else if (per <= 20) hipLaunchKernelGGL(embed_pool_kernel<20>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(embed_pool_kernel<32>, grid, block, 0, st, a);
}

}  // namespace aios
