// Per-token log-probabilities of the raw logits row (ops.h LogprobArgs), in the sampler's shape: grid
// (NS = ceil(V / 4096), B), 256 threads, ONE launch of two phases.
//  A) every workgroup holds a 4096-logit slice in registers (16 per thread): the slice maximum m, the sum
//     s = sum exp(l - m), and its local top n = top_n[b] logits ordered by (value desc, id asc) -- n rounds
//     of a block argmax, the winner's owner dropping it from its registers -- published with write-through
//     stores + a ticket, as the sampler's slices are;
//  B) the row's last arriving workgroup merges: M = max m_i, S = sum s_i exp(m_i - M), lse = M + log S; the
//     NS x n candidates (at most 1280, 5 per thread) go through the same n rounds -- the global top n is a
//     subset of the union of the slices' top n, the order being total; then l[tokens[b]] - lse, the
//     alternatives' l - lse, and the counter is re-armed.
// Selection only compares fp32 values, so the ids match a float64 oracle exactly, ties included.  Entries
// past V carry (-inf, INT_MAX): a real -inf logit sorts before them, by its id.
// (kernel arguments are never chosen between by a pointer select, and every register array is indexed by
// unrolled constants only: elementwise.hip's notes on SGPR spills and argument copies in scratch)
#include <climits>
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int LP_THREADS = 256;
constexpr int LP_PER_THREAD = 16;
constexpr int LP_SLICE = LP_THREADS * LP_PER_THREAD;
constexpr int LP_MAX_SLICES = SAMPLE_MAX_V / LP_SLICE;
constexpr int LP_MERGE_PER_THREAD = (LP_MAX_SLICES * LOGPROB_MAX_TOP + LP_THREADS - 1) / LP_THREADS;
static_assert(LP_MAX_SLICES <= LP_THREADS, "the merge reads one slice partial per thread");
static_assert(LOGPROB_MAX_TOP <= LP_THREADS, "thread r keeps the r-th winner");

static inline int lp_slices(int V) { return (V + LP_SLICE - 1) / LP_SLICE; }

size_t logprob_ws_bytes(int B, int V) {
  return (size_t)B * lp_slices(V) * (8 + (size_t)LOGPROB_MAX_TOP * 8) + 256;
}

struct LpWs {
  float* part_m; float* part_s; float* cand_v; int* cand_i;
};
__device__ __forceinline__ LpWs lp_ws(void* base, int B, int NS) {
  LpWs w;
  char* p = (char*)base;
  w.part_m = (float*)p; p += (size_t)B * NS * 4;
  w.part_s = (float*)p; p += (size_t)B * NS * 4;
  w.cand_v = (float*)p; p += (size_t)B * NS * LOGPROB_MAX_TOP * 4;
  w.cand_i = (int*)p;
  return w;
}

struct LpKey {
  float v;
  int i;
};
// the order of the reported list: value descending, ties by the lower id
__device__ __forceinline__ LpKey lp_better(LpKey a, LpKey b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ float lp_block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The n best of the block's N-per-thread (value, id) pairs, in order: thread r < n returns the r-th, the
// others (-inf, -1).  The real ids are distinct; the pads' INT_MAX never is removed and fills the list when
// fewer than n real pairs exist.  One barrier per round: the waves' winners alternate between two LDS rows.
template <int N>
__device__ __forceinline__ LpKey lp_block_topn(const float (&v)[N], const int (&id)[N], int n, float (*s_v)[4],
                                               int (*s_i)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned taken = 0;
  auto best_left = [&]() __attribute__((always_inline)) {
    LpKey m{-INFINITY, INT_MAX};
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (!((taken >> j) & 1u)) m = lp_better(m, LpKey{v[j], id[j]});
    return m;
  };
  LpKey mine = best_left();
  LpKey keep{-INFINITY, -1};
#pragma unroll 1
  for (int r = 0; r < n; ++r) {
    LpKey w = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      LpKey t;
      t.v = __shfl_xor(w.v, o, 64);
      t.i = __shfl_xor(w.i, o, 64);
      w = lp_better(w, t);
    }
    if (lane == 0) { s_v[r & 1][wid] = w.v; s_i[r & 1][wid] = w.i; }
    __syncthreads();
    LpKey g{s_v[r & 1][0], s_i[r & 1][0]};
#pragma unroll
    for (int k = 1; k < LP_THREADS / 64; ++k) g = lp_better(g, LpKey{s_v[r & 1][k], s_i[r & 1][k]});
    if (tid == r) keep = g;
    if (g.i == mine.i && g.i != INT_MAX) {  // this thread's pair won: drop it
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (id[j] == g.i) taken |= 1u << j;
      mine = best_left();
    }
  }
  return keep;
}

__global__ void __launch_bounds__(LP_THREADS) logprob_kernel(LogprobArgs a) {
  __shared__ float red[16];
  __shared__ float s_v[2][4];
  __shared__ int s_i[2][4];
  __shared__ int s_last;
  const int b = blockIdx.y, slice = blockIdx.x, NS = gridDim.x, tid = threadIdx.x;
  const int want = a.top_n[b];
  if (want < 0) return;  // row off (uniform over the row's workgroups: no ticket is taken)
  const int n = min(want, LOGPROB_MAX_TOP);
  const float* l = a.logits + (size_t)b * a.ldl;

  // ---- A) this slice in registers
  float v[LP_PER_THREAD];
  int id[LP_PER_THREAD];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < LP_PER_THREAD; ++j) {
    const int i = slice * LP_SLICE + j * LP_THREADS + tid;
    const bool in = i < a.V;
    v[j] = in ? l[i] : -INFINITY;
    id[j] = in ? i : INT_MAX;
    m = fmaxf(m, v[j]);
  }
  m = lp_block_max(m, red);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) s += expf(v[j] - m);
  }
  s = block_sum(s, red);
  const LpKey c = lp_block_topn(v, id, n, s_v, s_i);
  const LpWs w = lp_ws(a.ws, a.B, NS);
  const size_t sl = (size_t)b * NS + slice;
  if (tid < n) {
    __hip_atomic_store(w.cand_v + sl * LOGPROB_MAX_TOP + tid, c.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w.cand_i + sl * LOGPROB_MAX_TOP + tid, c.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) {
    __hip_atomic_store(w.part_m + sl, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w.part_s + sl, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(a.counters + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == NS - 1);
  }
  __syncthreads();
  if (!s_last) return;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);

  // ---- B) the row's last arriver merges
  auto ldf = [](const float* p) { return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto ldi = [](const int* p) { return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  float pm = -INFINITY, ps = 0.f;
  if (tid < NS) {
    pm = ldf(w.part_m + (size_t)b * NS + tid);
    ps = ldf(w.part_s + (size_t)b * NS + tid);
  }
  const float M = lp_block_max(pm, red);
  const float S = block_sum(pm > -INFINITY ? ps * expf(pm - M) : 0.f, red);
  const float lse = M + logf(S);
  float cv[LP_MERGE_PER_THREAD];
  int ci[LP_MERGE_PER_THREAD];
  const int total = NS * n;  // <= LP_MAX_SLICES * LOGPROB_MAX_TOP
#pragma unroll
  for (int j = 0; j < LP_MERGE_PER_THREAD; ++j) {
    const int o = j * LP_THREADS + tid;
    cv[j] = -INFINITY;
    ci[j] = INT_MAX;
    if (o < total) {
      const int sc = o / n;
      const size_t g = ((size_t)b * NS + sc) * LOGPROB_MAX_TOP + (o - sc * n);
      cv[j] = ldf(w.cand_v + g);
      ci[j] = ldi(w.cand_i + g);
    }
  }
  const LpKey g = lp_block_topn(cv, ci, n, s_v, s_i);
  float* olp = a.out_lp + (size_t)b * LOGPROB_ROW;
  int* oid = a.out_id + (size_t)b * LOGPROB_ROW;
  if (tid < LOGPROB_MAX_TOP) {
    const bool real = tid < n && g.i != INT_MAX;
    oid[1 + tid] = real ? g.i : -1;
    olp[1 + tid] = real ? g.v - lse : -INFINITY;
  }
  if (tid == 0) {
    const int tok = min(max(a.tokens[b], 0), a.V - 1);
    oid[0] = tok;
    olp[0] = l[tok] - lse;
    __hip_atomic_store(a.counters + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  }
}

void launch_logprobs(const LogprobArgs& a, hipStream_t st) {
  if (!a.ws || !a.counters) throw std::runtime_error("logprobs: workspace and counters required");
  if (!a.logits || !a.tokens || !a.top_n || !a.out_lp || !a.out_id)
    throw std::runtime_error("logprobs: null argument");
  if (a.B < 1 || a.ldl < a.V) throw std::runtime_error("logprobs: bad batch or row stride");
  if (a.V < 1 || a.V > SAMPLE_MAX_V)
    throw std::runtime_error("logprobs: vocabulary outside 1.." + std::to_string(SAMPLE_MAX_V));
  if (a.ws_bytes < logprob_ws_bytes(a.B, a.V)) throw std::runtime_error("logprobs: workspace too small");
  hipLaunchKernelGGL(logprob_kernel, dim3(lp_slices(a.V), a.B), dim3(LP_THREADS), 0, st, a);
}

}  // namespace aios
