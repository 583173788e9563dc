// Allowed-token masks of DFA grammars (ops.h GrammarMaskArgs): row b's mask is computed on the device from
// (grammar id, DFA state) instead of being walked, memoised and uploaded by the host.
//
//  - One thread per token, one workgroup of GM_THREADS tokens per (token tile, row).  The thread walks its token's
//    bytes through the row's table: class = byte_class[byte], state = trans[state][class], out at the dead state 0.
//    The byte and class loads do not depend on the state, so the next byte's class is requested before the
//    transition load that is in flight is waited for: the dependent chain is one u16 load per byte.
//  - An empty token (a control token) is not allowed; the end-of-sequence ids are allowed exactly when the row's
//    state is accepting, whatever their bytes.
//  - A wave's 64 verdicts are one ballot = 8 mask bytes in the sampler's layout (bit t % 8 of byte t / 8).  Lanes
//    0..7 store one byte each, bounded by the row's ceil(V / 8) bytes: rows need not be 8-byte aligned or padded,
//    and bits past V in the last byte are zero (those lanes vote false).
//  - A row with gid < 0 is filled with ones when fill_free is set (the launch has no host mask), else left alone.
// No LDS, no scratch, no atomics, no workspace.
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int GM_THREADS = 256;

__global__ __launch_bounds__(GM_THREADS) void grammar_mask_kernel(GrammarMaskArgs a) {
  const int b = blockIdx.y;
  const int gid = a.gid[b];
  if (gid < 0 && !a.fill_free) return;  // (the whole workgroup: the row is the host's)
  const int t = blockIdx.x * GM_THREADS + threadIdx.x;
  bool ok = false;
  if (gid < 0) {
    ok = t < a.V;
  } else if (t < a.V && gid < a.n_grammars) {
    const GrammarTable g = a.grammars[gid];
    unsigned s = (unsigned)a.state[b];
    if (s >= (unsigned)g.n_states) s = 0;  // (a state outside the table allows nothing)
    bool eos = false;
#pragma unroll
    for (int j = 0; j < GRAMMAR_MAX_EOS; ++j) eos |= j < a.n_eos && t == a.eos[j];
    if (eos) {
      ok = s != 0 && g.accept[s] != 0;
    } else {
      int i = a.tok_off[t];
      const int e = a.tok_off[t + 1];
      if (i < e && s != 0) {
        const unsigned C = (unsigned)g.n_classes;
        unsigned c = g.byte_class[a.tok_bytes[i]];
        for (;;) {
          ++i;
          const unsigned cn = i < e ? g.byte_class[a.tok_bytes[i]] : 0u;
          s = g.trans[s * C + c];
          if (i >= e || s == 0) break;
          c = cn;
        }
        ok = s != 0;
      }
    }
  }
  const unsigned long long word = __ballot(ok);
  const int lane = threadIdx.x & 63;
  const int nb = (a.V + 7) >> 3;
  const int byte = ((t >> 6) << 3) + lane;  // (t >> 6 is the wave's word: a wave's tokens start at a multiple of 64)
  if (lane < 8 && byte < nb) a.mask[(size_t)b * nb + byte] = (uint8_t)(word >> (8 * lane));
}

void launch_grammar_mask(const GrammarMaskArgs& a, hipStream_t st) {
  if (!a.tok_off || !a.tok_bytes || !a.gid || !a.state || !a.mask) throw std::runtime_error("grammar_mask: null argument");
  if (a.V < 1 || a.B < 1 || a.B > 65535) throw std::runtime_error("grammar_mask: bad shape");
  if (a.n_grammars < 0 || (a.n_grammars > 0 && !a.grammars)) throw std::runtime_error("grammar_mask: no grammar table");
  if (a.n_eos < 0 || a.n_eos > GRAMMAR_MAX_EOS)
    throw std::runtime_error("grammar_mask: more than " + std::to_string(GRAMMAR_MAX_EOS) + " end-of-sequence ids");
  const dim3 grid((a.V + GM_THREADS - 1) / GM_THREADS, a.B);
  hipLaunchKernelGGL(grammar_mask_kernel, grid, dim3(GM_THREADS), 0, st, a);
}

}  // namespace aios
