// Prompt scoring (ops.h ScoreArgs): for each of R raw logits rows and its target id, the target's logprob and
// rank and the row's argmax with its logprob.  The shape is the opposite of logprobs.hip's (few rows, each
// split over many workgroups): MANY rows, so ONE 256-thread workgroup per row, a grid stride over rows, one
// streaming pass over V per row.
//  - the row base is 16-byte aligned or not per row (ldl and V may be odd): a scalar head of up to 3 logits, the
//    body as 16-byte loads (four in flight per thread), a scalar tail of up to 3; nothing in [V, ldl) is read;
//  - per thread: an online (m, s) with s = sum exp(l - m), rescaled only when m grows; the argmax key (value
//    desc, id asc); the count of logits ordered before the target's l[t], which is loaded once up front;
//  - one block reduction per row (wave shuffles, then the four waves through LDS), in a fixed order.
// No workspace, no tickets, no atomics: the same input gives the same bits.  Selection compares the fp32
// values as they are, so rank and best match a float64 oracle exactly, ties included.
// (kernel arguments are never chosen between by a pointer select, and every register array is indexed by
// unrolled constants only: elementwise.hip's notes on SGPR spills and argument copies in scratch)
#include <algorithm>
#include <climits>
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_UNROLL = 4;        // 16-byte loads in flight per thread
constexpr int SC_MAX_GRID = 2048;   // workgroups per launch at most (8 per CU of 256 threads); more rows stride

struct ScState {
  float m, s;  // running maximum and sum exp(l - m)
  float bv;    // argmax key: value, then the lower id
  int bi;
  int cnt;     // logits ordered before the target
};

__device__ __forceinline__ void sc_take(ScState& st, float v, int i, bool has, float lt, int t) {
  if (v > st.m) {
    st.s = st.s * expf(st.m - v) + 1.f;  // (m = -inf: s is 0 and stays finite)
    st.m = v;
  } else if (v > -INFINITY) {
    st.s += expf(v - st.m);
  }
  if (v > st.bv || (v == st.bv && i < st.bi)) { st.bv = v; st.bi = i; }
  st.cnt += (has && (v > lt || (v == lt && i < t))) ? 1 : 0;
}

// a and b cover disjoint id sets
__device__ __forceinline__ ScState sc_merge(const ScState& a, const ScState& b) {
  ScState r;
  r.m = fmaxf(a.m, b.m);
  const float sa = a.m > -INFINITY ? a.s * expf(a.m - r.m) : 0.f;
  const float sb = b.m > -INFINITY ? b.s * expf(b.m - r.m) : 0.f;
  r.s = sa + sb;
  const bool tb = b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi);
  r.bv = tb ? b.bv : a.bv;
  r.bi = tb ? b.bi : a.bi;
  r.cnt = a.cnt + b.cnt;
  return r;
}

__global__ void __launch_bounds__(SC_THREADS) score_rows_kernel(ScoreArgs a) {
  __shared__ float s_m[SC_WAVES], s_s[SC_WAVES], s_bv[SC_WAVES];
  __shared__ int s_bi[SC_WAVES], s_cnt[SC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = a.V;
  for (int row = blockIdx.x; row < a.R; row += gridDim.x) {
    const float* l = a.logits + (size_t)row * a.ldl;
    const int t = a.targets[row];
    const bool has = t >= 0 && t < V;  // (an id past V is reported as no target: the read stays in the row)
    const float lt = has ? l[t] : 0.f;
    ScState st{-INFINITY, 0.f, -INFINITY, INT_MAX, 0};

    // scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
    const int mis = (int)(((uintptr_t)l >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int nvec = (V - head) >> 2;
    const int tail0 = head + 4 * nvec;
    if (tid < head) sc_take(st, l[tid], tid, has, lt, t);
    if (tid < V - tail0) sc_take(st, l[tail0 + tid], tail0 + tid, has, lt, t);
    const float4* l4 = (const float4*)(l + head);
    int k = tid;
    for (; k + (SC_UNROLL - 1) * SC_THREADS < nvec; k += SC_UNROLL * SC_THREADS) {
      float4 v[SC_UNROLL];
#pragma unroll
      for (int u = 0; u < SC_UNROLL; ++u) v[u] = l4[k + u * SC_THREADS];
#pragma unroll
      for (int u = 0; u < SC_UNROLL; ++u) {
        const int i = head + 4 * (k + u * SC_THREADS);
        sc_take(st, v[u].x, i, has, lt, t);
        sc_take(st, v[u].y, i + 1, has, lt, t);
        sc_take(st, v[u].z, i + 2, has, lt, t);
        sc_take(st, v[u].w, i + 3, has, lt, t);
      }
    }
    for (; k < nvec; k += SC_THREADS) {
      const float4 v = l4[k];
      const int i = head + 4 * k;
      sc_take(st, v.x, i, has, lt, t);
      sc_take(st, v.y, i + 1, has, lt, t);
      sc_take(st, v.z, i + 2, has, lt, t);
      sc_take(st, v.w, i + 3, has, lt, t);
    }

    // the row's one reduction: lanes by shuffles, then the waves through LDS, both in a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ScState p;
      p.m = __shfl_xor(st.m, o, 64);
      p.s = __shfl_xor(st.s, o, 64);
      p.bv = __shfl_xor(st.bv, o, 64);
      p.bi = __shfl_xor(st.bi, o, 64);
      p.cnt = __shfl_xor(st.cnt, o, 64);
      // (both lanes of a pair merge in the same operand order, so they hold the same bits)
      st = (lane & o) ? sc_merge(p, st) : sc_merge(st, p);
    }
    __syncthreads();  // (the previous row's readers are done with the LDS rows)
    if (lane == 0) { s_m[wid] = st.m; s_s[wid] = st.s; s_bv[wid] = st.bv; s_bi[wid] = st.bi; s_cnt[wid] = st.cnt; }
    __syncthreads();
    if (tid == 0) {
      ScState g{s_m[0], s_s[0], s_bv[0], s_bi[0], s_cnt[0]};
#pragma unroll
      for (int w = 1; w < SC_WAVES; ++w) g = sc_merge(g, ScState{s_m[w], s_s[w], s_bv[w], s_bi[w], s_cnt[w]});
      const float lse = g.m + logf(g.s);
      a.out_f[(size_t)row * 2] = has ? lt - lse : __builtin_nanf("");
      a.out_f[(size_t)row * 2 + 1] = g.bv - lse;
      a.out_i[(size_t)row * 2] = has ? g.cnt : -1;
      a.out_i[(size_t)row * 2 + 1] = g.bi;
    }
  }
}

void launch_score_rows(const ScoreArgs& a, hipStream_t st) {
  if (!a.logits || !a.targets || !a.out_f || !a.out_i) throw std::runtime_error("score_rows: null argument");
  if (a.R < 1 || a.V < 1 || a.ldl < a.V) throw std::runtime_error("score_rows: bad rows, vocabulary or row stride");
  if ((uintptr_t)a.logits & 3) throw std::runtime_error("score_rows: logits not 4-byte aligned");
  const int cap = a.max_grid > 0 ? std::min(a.max_grid, SC_MAX_GRID) : SC_MAX_GRID;
  hipLaunchKernelGGL(score_rows_kernel, dim3(std::min(a.R, cap)), dim3(SC_THREADS), 0, st, a);
}

}  // namespace aios
