// Speculative decoding's accept step (ops.h SpecAcceptArgs): after the R-row sampler launch of one request's
// R consecutive positions, find how many drafts the sampler agreed with, pack what the host needs into one
// record and turn row 0 of the step state into the sequence advanced by n + 1 tokens.
//  - one workgroup of one wave: lane i < R holds out[i] and in[i + 1]; a ballot of the mismatching lanes gives
//    n as its lowest set bit (lane R - 1 always counts as one: there is no draft behind the last row);
//  - every out[i] is in a register before anything is stored, so out may be the state's own token array;
//  - lanes 0..n store their token into the record and row 0's history, lanes above store the record's -1
//    padding, lane 0 stores n and row 0's {token, pos, seq_len} -- plain vector stores, nothing else.
// No workspace, no atomics, no LDS.
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

__global__ __launch_bounds__(64) void spec_accept_kernel(SpecAcceptArgs a) {
  const int lane = threadIdx.x;
  const int R = a.R;
  int o = -1, d = -2;  // (never equal: lanes at or past R - 1 mismatch)
  if (lane < R) o = a.out[lane];
  if (lane + 1 < R) d = a.in[lane + 1];
  const unsigned long long miss = __ballot(o != d);  // bit R - 1 is set, so miss != 0
  const int n = __ffsll((long long)miss) - 1;        // 0..R-1
  const int last = __shfl(o, n, 64);
  if (lane < SPEC_MAX_ROWS) a.record[1 + lane] = lane <= n ? o : -1;
  if (lane <= n && a.history) {
    const int h = a.pos0 + 1 + lane;
    if (h < a.hist_stride) a.history[h] = o;
  }
  if (lane == 0) {
    a.record[0] = n;
    a.tokens[0] = last;
    a.pos[0] = a.pos0 + n + 1;
    a.seq_len[0] = a.pos0 + n + 2;
  }
}

void launch_spec_accept(const SpecAcceptArgs& a, hipStream_t st) {
  if (!a.in || !a.out || !a.record || !a.tokens || !a.pos || !a.seq_len)
    throw std::runtime_error("spec_accept: null argument");
  if (a.R < 2 || a.R > SPEC_MAX_ROWS) throw std::runtime_error("spec_accept: rows outside 2.." + std::to_string(SPEC_MAX_ROWS));
  if (a.pos0 < 0 || (a.history && a.hist_stride < 1)) throw std::runtime_error("spec_accept: bad position or history stride");
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, st, a);
}

// The segmented step (ops.h SpecAcceptMultiArgs): S sequences' rows side by side, each segment judged alone.
//  - still one wave: lane r < Rt holds out[r] and, unless r is its segment's last row, in[r + 1]; one ballot of
//    the mismatching lanes serves every segment, n_s being its lowest set bit at or above seg[s] (a segment's
//    last row always counts as a mismatch, so the search never leaves the segment);
//  - seg[] and pos0[] sit in the argument block and are read with constant indices in unrolled loops (scalar
//    loads, no private segment); lane s < S keeps its sequence's {seg[s], pos0[s], n_s}, the record lanes fetch
//    them with shuffles;
//  - the S records are S * SPEC_RECORD <= 72 ints: two passes of the wave, both computed before anything is
//    stored, as is every other value -- out may be the state's own token array, which rows 0..S-1 overwrite.
__global__ __launch_bounds__(64) void spec_accept_multi_kernel(SpecAcceptMultiArgs a) {
  const int lane = threadIdx.x;
  const int S = a.S;
  // the segment of flat row `lane` (none at or past Rt) and, for lane s < S, sequence s's segment
  int seg_b = 0, seg_e = 0, seg_i = -1, seg_p0 = 0;  // row `lane`'s segment: [seg_b, seg_e), index, pos0
  int sq_b = 0, sq_p0 = 0;                           // sequence `lane`'s
#pragma unroll
  for (int t = 0; t < SPEC_MULTI_MAX_SEQS; ++t) {
    if (t < S) {
      const int b = a.seg[t], e = a.seg[t + 1], p = a.pos0[t];
      if (lane >= b && lane < e) { seg_b = b; seg_e = e; seg_i = t; seg_p0 = p; }
      if (lane == t) { sq_b = b; sq_p0 = p; }
    }
  }
  int o = -1, d = -2;  // (never equal: a segment's last row and the lanes past Rt mismatch)
  if (seg_i >= 0) o = a.out[lane];
  if (lane + 1 < seg_e) d = a.in[lane + 1];
  const unsigned long long miss = __ballot(o != d);  // every bit seg[s + 1] - 1 is set
  const int n_row = __ffsll((long long)(miss >> seg_b)) - 1;  // row `lane`'s segment's n
  const int sq_n = __ffsll((long long)(miss >> sq_b)) - 1;    // sequence `lane`'s n (lane < S)
  const int sq_last = __shfl(o, (sq_b + sq_n) & 63, 64);
  // the records: entry idx = s * SPEC_RECORD + j, j = 0: n_s, j >= 1: out[seg[s] + j - 1] or -1
  int rec[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int idx = lane + 64 * k;
    const int s = min(idx / SPEC_RECORD, SPEC_MULTI_MAX_SEQS - 1), j = idx % SPEC_RECORD;
    const int b = __shfl(sq_b, s, 64), n = __shfl(sq_n, s, 64);
    const int v = __shfl(o, (b + j - 1) & 63, 64);
    rec[k] = j == 0 ? n : (j - 1 <= n ? v : -1);
  }
  // ---- stores only from here on ----
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (lane + 64 * k < S * SPEC_RECORD) a.record[lane + 64 * k] = rec[k];
  if (seg_i >= 0 && lane - seg_b <= n_row && a.history) {
    const int h = seg_p0 + 1 + (lane - seg_b);
    if (h < a.hist_stride) a.history[(size_t)seg_i * a.hist_stride + h] = o;
  }
  if (lane < S) {
    a.tokens[lane] = sq_last;
    a.pos[lane] = sq_p0 + sq_n + 1;
    a.seq_len[lane] = sq_p0 + sq_n + 2;
  }
}

void launch_spec_accept_multi(const SpecAcceptMultiArgs& a, hipStream_t st) {
  if (!a.in || !a.out || !a.record || !a.tokens || !a.pos || !a.seq_len)
    throw std::runtime_error("spec_accept_multi: null argument");
  if (a.S < 1 || a.S > SPEC_MULTI_MAX_SEQS)
    throw std::runtime_error("spec_accept_multi: sequences outside 1.." + std::to_string(SPEC_MULTI_MAX_SEQS));
  if (a.seg[0] != 0) throw std::runtime_error("spec_accept_multi: the first segment does not start at row 0");
  for (int s = 0; s < a.S; ++s) {
    const int rows = a.seg[s + 1] - a.seg[s];
    if (rows < 1 || rows > SPEC_MAX_ROWS)
      throw std::runtime_error("spec_accept_multi: a segment's rows outside 1.." + std::to_string(SPEC_MAX_ROWS));
    if (a.pos0[s] < 0) throw std::runtime_error("spec_accept_multi: bad position");
  }
  if (a.seg[a.S] > SPEC_MULTI_MAX_ROWS)
    throw std::runtime_error("spec_accept_multi: more than " + std::to_string(SPEC_MULTI_MAX_ROWS) + " rows");
  if (a.history && a.hist_stride < 1) throw std::runtime_error("spec_accept_multi: bad history stride");
  hipLaunchKernelGGL(spec_accept_multi_kernel, dim3(1), dim3(64), 0, st, a);
}

}  // namespace aios
