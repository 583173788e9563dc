// Host-built launch descriptors of the one-workgroup-per-CU batch-1 GEMVs (kernels/gemv_lds.h,
// kernels/gemv_cu.h).
//
// Which row pairs a workgroup owns, how many ring slots it runs and where its first slots lie in
// the weight planes are pure functions of (segment shapes and formats, K, grid): constant for the
// life of a weight set and across graph replays.  The kernels used to recompute them in every wave
// of every launch (two 64-bit divisions, the mixed-format split, a segment search per prologue
// slot) before the first weight byte was requested.  They are now built here once per
// (shape, grid, kernel variant), cached in device memory for the life of the process
// (gemv_desc_device, kernels/gemv_dispatch.hip) and read by the kernel with one scalar load.
//
// A descriptor holds row / group indices only, never a pointer: every weight set of one shape (all
// layers of a model, every engine in the process) shares it.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "qweight.h"

namespace aios {

struct GemvWgDesc;

struct CuPlan {
  int g0;      // workgroups serving format-0 pairs [0, np0)
  int np0;     // pairs of format 0; pairs [np0, N/2) use the last segment's format
  int racc_n;  // LDS row accumulators: 2 x the most pairs any workgroup owns, rounded to 4
  const GemvWgDesc* desc;  // [grid] device records (null: the BF16 engine, which splits in-kernel)
};

constexpr int GD_PRO = 8;                   // engine prologue slots described per workgroup
constexpr int GD_OFF_BITS = 26;             // pro word: slot's first group within its segment ...
constexpr int GD_SEG_SHIFT = GD_OFF_BITS;   // ... the segment (2 bits) ...
constexpr int GD_FAST = 1 << 28;            // ... whole slot inside one segment and the workgroup's groups
constexpr int GD_SEAM = 1 << 29;            // ... whole slot inside the workgroup's groups but across a segment seam

// one workgroup's record: 64 B, read with one scalar load
struct alignas(64) GemvWgDesc {
  int r0;        // first row
  int nrows;     // rows (0: the workgroup owns nothing and returns before any barrier)
  int ngroups;   // nrows x 64-chunk groups per row
  int T;         // engine ring slots: ceil(ngroups / groups per slot of the workgroup's format)
  int fmt1;      // 1: the rows are in the last segment's format (mixed launches)
  int nfast;     // leading prologue slots that are GD_FAST (<= GD_PRO)
  int rsv[2];
  int pro[GD_PRO];  // slot s < min(T, GD_PRO)
};
static_assert(sizeof(GemvWgDesc) == 64, "one 16-dword scalar load");

// what a descriptor depends on (the cache key, with the device)
struct GemvDescShape {
  int nseg;
  int qtype[3];
  int seg_row0[3];
  int N, K;
  int grid;     // workgroups asked for (CU count, CU-mask budget or tune_grid), before the clamp to N / 2
  int variant;  // GemvArgs::kernel_sel of the kernel served: 2 register kernel, 3 LDS-DMA engine
};

inline int gd_chunk_w(int qt) { return qt == QT_Q8_0 ? 16 : ((qt == QT_F16 || qt == QT_BF16) ? 8 : 32); }
// groups per engine ring slot (LgLayout::NGS): 14 consumer waves x 1 (Q6_K, Q5_K) or 2 groups
constexpr int gd_slot_groups(int qt) { return (qt == QT_Q6_K || qt == QT_Q5_K) ? 14 : 28; }

inline int cu_fmt_bytes_per_256(int qt) {
  switch (qt) {
    case QT_Q4_K: return 144;
    case QT_Q5_K: return 176;
    case QT_Q6_K: return 210;
    case QT_Q4_0: return 144;
    case QT_Q8_0: return 272;
  }
  return 256;
}

// the launch plan: grid G and the format split; false when the shape cannot be split (then the
// row-pair kernel runs)
inline bool gemv_desc_plan(const GemvDescShape& s, CuPlan& pl, int& G) {
  const int npairs = s.N / 2;
  G = std::min(s.grid, npairs);
  if (G < 1 || s.nseg < 1 || s.nseg > 3) return false;
  auto rup = [](int n, int g) { return (n + g - 1) / g; };
  pl = CuPlan{G, npairs, (2 * rup(npairs, G) + 3) & ~3, nullptr};
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  if (qt0 != qt1 && s.nseg > 1) {
    const int np0 = s.seg_row0[s.nseg - 1] / 2;
    if (G < 2 || np0 < 1 || np0 >= npairs) return false;
    const double b0 = (double)np0 * cu_fmt_bytes_per_256(qt0), b1 = (double)(npairs - np0) * cu_fmt_bytes_per_256(qt1);
    int g0 = (int)(G * b0 / (b0 + b1) + 0.5);
    g0 = std::max(1, std::min(G - 1, g0));
    const int most = std::max(rup(np0, g0), rup(npairs - np0, G - g0));
    pl = CuPlan{g0, np0, (2 * most + 3) & ~3, nullptr};
  }
  return true;
}

// the G records of a plan
inline std::vector<GemvWgDesc> gemv_desc_build(const GemvDescShape& s, const CuPlan& pl, int G) {
  std::vector<GemvWgDesc> out((size_t)G);
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  const bool mixed = qt0 != qt1;
  const int npairs = s.N / 2;
  const int nch = s.K / gd_chunk_w(qt0);
  const int nit = (nch + 63) >> 6;
  const long G1 = s.nseg > 1 ? (long)s.seg_row0[1] * nit : LONG_MAX;
  const long G2 = s.nseg > 2 ? (long)s.seg_row0[2] * nit : LONG_MAX;
  for (int g = 0; g < G; ++g) {
    GemvWgDesc d{};
    const bool fmt1 = mixed && g >= pl.g0;
    int pb, pe;
    if (!fmt1) {
      const int np = mixed ? pl.np0 : npairs, Gd = mixed ? pl.g0 : G;
      pb = (int)((long)g * np / Gd);
      pe = (int)((long)(g + 1) * np / Gd);
    } else {
      const int np = npairs - pl.np0, Gd = G - pl.g0, gg = g - pl.g0;
      pb = pl.np0 + (int)((long)gg * np / Gd);
      pe = pl.np0 + (int)((long)(gg + 1) * np / Gd);
    }
    d.fmt1 = fmt1;
    if (pb < pe) {
      d.r0 = 2 * pb;
      d.nrows = 2 * (pe - pb);
      d.ngroups = d.nrows * nit;
      const int ngs = gd_slot_groups(fmt1 ? qt1 : qt0);
      d.T = (d.ngroups + ngs - 1) / ngs;
      const long gfirst = (long)d.r0 * nit, glast = gfirst + d.ngroups - 1;
      bool lead = true;
      for (int sl = 0; sl < std::min(d.T, GD_PRO); ++sl) {
        const long g0 = gfirst + (long)sl * ngs, gend = g0 + ngs - 1;
        const int sg = g0 >= G2 ? 2 : (g0 >= G1 ? 1 : 0);
        const long Gs = sg == 0 ? 0 : (sg == 1 ? G1 : G2), Gn = sg == 0 ? G1 : (sg == 1 ? G2 : LONG_MAX);
        const long off = g0 - Gs;
        const bool whole = gend <= glast && off < (1L << GD_OFF_BITS);
        const bool fast = whole && gend < Gn;
        d.pro[sl] = (int)(off & ((1L << GD_OFF_BITS) - 1)) | (sg << GD_SEG_SHIFT) | (fast ? GD_FAST : 0) |
                    (whole && !fast ? GD_SEAM : 0);
        lead = lead && fast;
        if (lead) d.nfast = sl + 1;
      }
    }
    out[(size_t)g] = d;
  }
  return out;
}

// the cached device copy of a plan's records for the current device (kernels/gemv_dispatch.hip);
// built and uploaded on the first use of (shape, grid, variant), then shared by every launch, stream,
// engine and captured graph of the process.  Safe to call while the calling thread captures a graph.
const GemvWgDesc* gemv_desc_device(const GemvDescShape& s, const CuPlan& pl, int G);
// allocate the first descriptor arena of the current device now (engines call it at construction,
// so no allocation happens inside a graph capture)
void gemv_desc_reserve();

}  // namespace aios
