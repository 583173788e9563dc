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

}  // namespace aios
