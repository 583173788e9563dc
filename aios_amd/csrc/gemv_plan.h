// The host-side launch plan of the decode GEMVs: which kernel family serves a launch, with which
// template parameters, grid, workgroup size and LDS bytes.  Pure arithmetic on the shape: no HIP
// call, no pointer, no allocation, so it is pinned on the CPU (tests/test_gemv_plan.py through the
// gemv_plan binding).  The launchers (kernels/gemv_impl.h) map a plan onto the compiled
// instantiations and decide nothing; the engine's questions (gemv_engine_fits,
// gemv_bf16_engine_fits, the dry mode of launch_gemv_tp_fused) ask the plan and launch nothing.
//
// A new kernel variant is one more plan_* function and one rung of gemv_plan's cascade.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "gemv.h"
#include "gemv_desc.h"

namespace aios {

// ---------------------------------------------------------------------------------------- knobs
// Process-wide tuning knobs of the GEMV launch choice (environment, read once: gemv_knobs()).  The
// engine's per-projection AIOS_GEMV_{U,GRID}_{QKV,...} knobs are not here: they arrive per launch
// as GemvArgs::tune_u / tune_grid.
struct GemvKnobs {
  // AIOS_GEMV_LDS: the LDS-DMA engine (gemv_lds.h): 0 = off, 1 = projections from lds_min_kb per
  // CU at batch 1 and every batched shape (default), 2 = every shape.
  // Small projections (O: <= ~40 KB per CU) stay on the row-pair kernel: the engine's fixed
  // start-up (first slot lands ~3-4 us after issue, behind the CU's whole prologue burst) and its
  // barrier steps cost more than the row kernel's x-staging stall there (tools/gemv_cu_probe.py:
  // O 6.96 vs 5.60 us, QKV 8.73 vs 8.38; gate_up 17.35 vs 19.39, down 13.8 vs 15.2, lm_head 24.8
  // vs 25.9).  Batched launches (B >= 2) take the engine for every shape: the row-pair kernels
  // re-read the B x vectors per wave and measured 2-3x slower there (B = 2 QKV 26 us vs 9.6 at
  // B = 1).
  int lds = 1;
  // AIOS_GEMV_LDS_MAXB: batch rows the engine serves (1..4, default 4; whether B = 3 / 4 decode
  // takes this path or the skinny MFMA GEMM is the engine's dec_gemm_min_b_,
  // profiles/lds_batched_r3.txt).  kernel_sel = 3 serves up to 4 whatever this says.
  int lds_maxb = 4;
  // AIOS_GEMV_LDS_MIN_KB: per-CU weight bytes from which the engine serves a batch-1 shape.
  // Round 5 (same box, tools/ab.sh): 40 instead of 96 -- the Mistral QKV (59 KB per CU) and the
  // TinyLlama gate/up (50 KB) move to the engine: Mistral 668.2 / 668.1 -> 672.6 / 671.5 tok/s,
  // TinyLlama 1500.7 / 1500.5 -> 1530.8 / 1535.3 (O, 37 KB, stays on the row kernel).
  double lds_min_kb = 40.0;
  // AIOS_LDS_B1_RSUB: ring slots fewer than LgLayout's depth at batch 1 (1 or 2; anything else:
  // the full depth).  A smaller prologue burst (~64 instead of ~96 KB per CU, 16 MB chip-wide)
  // lands the first slot sooner, and R - 1 slots in flight still cover the stream's latency:
  // 649.4 -> 662.9 tok/s same box (tools/gpu_r4_ab5.sh,
  // profiles/decode_mistral_rocprof_r4_final.txt).
  int lds_b1_rsub = 1;
  // AIOS_LDS_B1_RSUB_Q6: Q6_K matrices' own value (negative: lds_b1_rsub).  Default 2: their
  // 23.5 KB slots cover the latency with one slot fewer still -- Mistral B=1 670.7 / 670.9 ->
  // 672.6 / 672.0 tok/s, profiles/decode_b1_experiments_r6.txt.
  int lds_b1_rsub_q6 = 2;
  // AIOS_GEMV_CU: the register-streaming one-workgroup-per-CU kernel (gemv_cu.h), kept for probes
  // (kernel_sel 2 / AIOS_GEMV_CU=4|8 = items in flight per wave): slower than the LDS-DMA engine
  // because its weight stream stalls during the x staging.  0 = off (default).
  int cu = 0;
  // AIOS_Q8_BALANCE: the row-pair kernel's batch-1 launch sized to one workgroup per CU (see
  // plan_q8); 0 = the 8-wave grid and the double-buffered U.
  int q8_balance = 1;
  // AIOS_GEMV_BF16_LDS: the BF16 LDS-DMA engine (gemv_lds16.h); 0 = the round-1 persistent
  // register GEMV instead (A/B runs).
  int bf16_lds = 1;
  // AIOS_LB_CFG (BF16 engine, batch 1 only): slot geometry x ring depth -- 23 = 28 KB slots x 3
  // (default), 24 = 28 KB x 4, 14 = 14 KB x 4, 16 = 14 KB x 6
  // (profiles/decode_tinyllama_bf16_rocprof_r6.txt).
  int lb_cfg = 23;
};

inline const GemvKnobs& gemv_knobs() {
  static const GemvKnobs k = [] {
    GemvKnobs v;
    auto geti = [](const char* name, int& dst) {
      if (const char* e = std::getenv(name)) dst = std::atoi(e);
    };
    geti("AIOS_GEMV_LDS", v.lds);
    geti("AIOS_GEMV_LDS_MAXB", v.lds_maxb);
    v.lds_maxb = std::max(1, std::min(4, v.lds_maxb));
    if (const char* e = std::getenv("AIOS_GEMV_LDS_MIN_KB")) v.lds_min_kb = std::atof(e);
    geti("AIOS_LDS_B1_RSUB", v.lds_b1_rsub);
    geti("AIOS_LDS_B1_RSUB_Q6", v.lds_b1_rsub_q6);
    geti("AIOS_GEMV_CU", v.cu);
    geti("AIOS_Q8_BALANCE", v.q8_balance);
    geti("AIOS_GEMV_BF16_LDS", v.bf16_lds);
    geti("AIOS_LB_CFG", v.lb_cfg);
    return v;
  }();
  return k;
}

// ---------------------------------------------------------------------------------------- shape
// What the choice depends on, and nothing else (no pointer: two launches of one shape share a plan)
struct GemvShape {
  int nseg;
  int qtype[GEMV_MAX_SEGS];
  int seg_row0[GEMV_MAX_SEGS];
  int seg_rows[GEMV_MAX_SEGS];
  int k_ok;  // every segment's column count is K
  int N, K, B, epi;
  int act_q8, force_v1, kernel_sel, tune_grid, tune_u, tune_dbg;
  int x16, y16;  // the bf16 input / SwiGLU output hand-off is set
  int grid_cap;
};

inline GemvShape gemv_shape(const GemvArgs& a) {
  GemvShape s{};
  s.nseg = a.nseg;
  s.k_ok = 1;
  for (int k = 0; k < a.nseg && k < GEMV_MAX_SEGS; ++k) {
    s.qtype[k] = a.seg[k].qtype;
    s.seg_row0[k] = a.seg_row0[k];
    s.seg_rows[k] = a.seg[k].rows;
    if (a.seg[k].cols != a.K) s.k_ok = 0;
  }
  s.N = a.N; s.K = a.K; s.B = a.B; s.epi = a.epi;
  s.act_q8 = a.act_q8; s.force_v1 = a.force_v1; s.kernel_sel = a.kernel_sel;
  s.tune_grid = a.tune_grid; s.tune_u = a.tune_u; s.tune_dbg = a.tune_dbg;
  s.x16 = a.x16 != nullptr; s.y16 = a.y16 != nullptr;
  s.grid_cap = a.grid_cap;
  return s;
}

// ----------------------------------------------------------------------------------------- plan
enum GemvFamily : int {
  GF_NONE = 0,     // nothing serves the shape (only from the fused-TP question, plan_tp_fused)
  GF_LDS,          // LDS-DMA engine, gemv_lds_b1<QT0, QT1, B, RSUB>
  GF_LDS16,        // BF16 LDS-DMA engine, gemv_lds16<B, R, GPW>
  GF_CU,           // CU register kernel, gemv_cu_b1<QT0, QT1, D>
  GF_Q8,           // q8 row-pair kernel, gemv_q8_rows<QT0, QT1, B, U, PIPE>
  GF_PERSISTENT,   // persistent fp32 kernel, gemv_persistent<QT0, QT1, B, U>
  GF_V1,           // v1 fp32 kernel, gemv_kernel<QT0, QT1, B, U>
};
inline const char* gemv_family_name(int f) {
  static const char* const n[] = {"none", "lds", "lds16", "cu", "q8", "persistent", "v1"};
  return f >= 0 && f <= GF_V1 ? n[f] : "?";
}

struct GemvPlan {
  int family;
  int B;             // batch rows as instantiated (>= the launch's B)
  int U, PIPE;       // q8 / persistent / v1: chunks per lane per item; q8: item buffers
  int RSUB;          // LDS engine: ring slots fewer than LgLayout's depth
  int R, GPW;        // BF16 engine: ring depth, groups per consumer wave per step
  int D;             // CU kernel: items in flight per wave
  int grid, threads;
  size_t lds;        // dynamic LDS bytes
  int kt_max;        // GemvArgs::kt_max of the launch (0: the family does not read it)
  CuPlan cu;         // LDS / BF16 / CU families (desc stays null until the launch)
  GemvDescShape desc;  // LDS / CU families: the launch descriptor to fetch at the launch
  bool occ_grid;     // the grid came from the occupancy query
};

// flag of a format pair's entry point (gemv_pair, kernels/gemv_impl.h): the plan of
// launch_gemv_tp_fused instead of launch_gemv's cascade
constexpr int GEMV_TP_FUSED = 1;

// compile-time constants of the kernels, asserted where the kernels define them (gemv_impl.h)
constexpr int PLAN_V1_THREADS = 256, PLAN_V1_ROWS_PER_BLOCK = 8, PLAN_V1_LDS_FLOATS = 16384;
constexpr int PLAN_GP_THREADS = 256, PLAN_GP_WAVES = 4;
constexpr int PLAN_Q8_WAVES = 8;
constexpr int PLAN_ONE_WG_THREADS = 1024;  // LDS engines and the CU kernel: one workgroup per CU
constexpr int PLAN_LG_DBG_RING = 0x10000;
constexpr int PLAN_TPF_SLOTS = 256, PLAN_TPF_CAP = 1024;  // comm.h
constexpr size_t PLAN_LDS_MAX = 160 * 1024;

constexpr bool plan_is16(int qt) { return qt == QT_F16 || qt == QT_BF16; }
constexpr int plan_w(int qt) { return qt == QT_Q8_0 ? 16 : (plan_is16(qt) ? 8 : 32); }     // QFmt::W
constexpr int plan_runs(int qt) { return (qt == QT_Q8_0 || plan_is16(qt)) ? 1 : 2; }       // QFmt::RUNS
constexpr bool plan_kq(int qt) { return qt == QT_Q4_K || qt == QT_Q5_K || qt == QT_Q6_K; }
constexpr bool plan_same_xlayout(int a, int b) { return a == b || (plan_kq(a) && plan_kq(b)); }
constexpr int plan_qtype_block(int qt) { return plan_kq(qt) ? 256 : (plan_is16(qt) ? 8 : 32); }
constexpr bool plan_lg_supported(int qt) { return plan_kq(qt) || qt == QT_Q4_0 || qt == QT_Q8_0; }
// LDS engine ring per format: bytes per slot and LgLayout's depth before RSUB (gemv_lds.h)
constexpr int plan_lg_slot_bytes(int qt) {
  return qt == QT_Q5_K ? 20480 : (qt == QT_Q6_K ? 23808 : (qt == QT_Q8_0 ? 30720 : 32768));
}
constexpr int plan_lg_depth(int qt) { return qt == QT_Q5_K ? 6 : (qt == QT_Q6_K ? 5 : 4); }
// up to 16 waves per workgroup for the register-light variants (U <= 2 single-buffered: the batch-1
// QKV / O shapes).  The double-buffered ones keep 8: at 16 waves (128 VGPRs) they spilled 12-230 B
// per lane to scratch (tools/kernel_resources.py)
constexpr int plan_q8_max_threads(int U, int PIPE) { return U <= 2 && PIPE == 1 ? 1024 : PLAN_Q8_WAVES * 64; }

// the format pairs with compiled kernels: (every segment but the last, the last segment)
struct GemvPair {
  int qt0, qt1;
};
constexpr GemvPair GEMV_PAIRS[] = {{QT_Q4_K, QT_Q4_K}, {QT_Q4_K, QT_Q6_K}, {QT_Q6_K, QT_Q6_K}, {QT_Q5_K, QT_Q5_K},
                                   {QT_Q5_K, QT_Q6_K}, {QT_Q4_0, QT_Q4_0}, {QT_Q8_0, QT_Q8_0}, {QT_F16, QT_F16},
                                   {QT_BF16, QT_BF16}};
constexpr int GEMV_NPAIRS = sizeof(GEMV_PAIRS) / sizeof(GEMV_PAIRS[0]);
inline int gemv_pair_index(int qt0, int qt1) {
  for (int i = 0; i < GEMV_NPAIRS; ++i)
    if (GEMV_PAIRS[i].qt0 == qt0 && GEMV_PAIRS[i].qt1 == qt1) return i;
  return -1;
}

// what launch_gemv refuses outright
inline void gemv_check(const GemvShape& s) {
  if (s.nseg < 1 || s.nseg > GEMV_MAX_SEGS) throw std::runtime_error("gemv: bad segment count");
  if (s.B < 1 || s.B > 8) throw std::runtime_error("gemv: batch must be 1..8");
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  for (int k = 0; k + 1 < s.nseg; ++k)
    if (s.qtype[k] != qt0) throw std::runtime_error("gemv: only the last segment may differ in format");
  if (!s.k_ok) throw std::runtime_error("gemv: segment K mismatch");
  for (int k = 0; k < s.nseg; ++k)
    if (s.seg_row0[k] % 8) throw std::runtime_error("gemv: segment boundary must be a multiple of 8 rows");
  if (s.N % 2) throw std::runtime_error("gemv: N must be even");
  if (s.K % 16) throw std::runtime_error("gemv: K must be a multiple of 16");
  if (gemv_pair_index(qt0, qt1) < 0)
    throw std::runtime_error("gemv: unsupported format pair " + std::to_string(qt0) + "/" + std::to_string(qt1));
}

inline GemvDescShape plan_desc_shape(const GemvShape& s, int grid, int variant) {
  GemvDescShape d{};
  d.nseg = s.nseg;
  for (int k = 0; k < s.nseg; ++k) {
    d.qtype[k] = s.qtype[k];
    d.seg_row0[k] = s.seg_row0[k];
  }
  d.N = s.N;
  d.K = s.K;
  d.grid = grid;
  d.variant = variant;
  return d;
}

// ---- the LDS-DMA engine (B = 1..4, int8 activations); false: the shape does not fit
inline bool plan_lds(const GemvShape& s, const GemvKnobs& kn, int cus, GemvPlan& p) {
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  if (!plan_same_xlayout(qt0, qt1) || !plan_lg_supported(qt0) || !plan_lg_supported(qt1)) return false;
  // (tune_dbg LG_DBG_RING: the probe's ring-only mode; every other microbenchmark bit -> row kernels)
  if (!kn.lds || s.B < 1 || s.B > (s.kernel_sel == 3 ? 4 : kn.lds_maxb) || (s.tune_dbg & ~PLAN_LG_DBG_RING) ||
      (s.kernel_sel != 0 && s.kernel_sel != 3))
    return false;
  const int W = plan_w(qt0), R = plan_runs(qt0);
  const int nch = s.K / W;
  if (nch % 64) return false;  // a ring group is 64 chunks of one row
  GemvPlan q{};
  q.desc = plan_desc_shape(s, s.tune_grid > 0 ? s.tune_grid : cus, 3);
  if (!gemv_desc_plan(q.desc, q.cu, q.grid)) return false;
  if (kn.lds != 2 && s.kernel_sel != 3 && s.B == 1) {  // the size floor (GemvKnobs::lds, lds_min_kb)
    double bytes = 0;
    for (int k = 0; k < s.nseg; ++k) bytes += (double)s.seg_rows[k] * s.K / 256.0 * cu_fmt_bytes_per_256(s.qtype[k]);
    if (bytes / q.grid < kn.lds_min_kb * 1024) return false;
  }
  auto bytes = [&](int B, int rsub) {
    const size_t head = (64 + (size_t)B * q.cu.racc_n) * 4 + (size_t)B * nch * R * 8 + (size_t)B * s.K;
    const size_t ring = std::max((plan_lg_depth(qt0) - rsub) * plan_lg_slot_bytes(qt0),
                                 (plan_lg_depth(qt1) - rsub) * plan_lg_slot_bytes(qt1));
    return (head + 255) / 256 * 256 + ring;
  };
  q.family = GF_LDS;
  q.B = s.B;  // (B = 3 has its own instantiation: no idle fourth row in the dot work / staging)
  q.threads = PLAN_ONE_WG_THREADS;
  if (s.B == 1) {
    const int rsub = (qt0 == QT_Q6_K && kn.lds_b1_rsub_q6 >= 0) ? kn.lds_b1_rsub_q6 : kn.lds_b1_rsub;
    q.RSUB = (rsub == 1 || rsub == 2) ? rsub : 0;
  } else {
    // long K (the d_ff-wide down projection): three / four staged x rows leave room for a shallower ring
    q.RSUB = (s.B >= 3 && bytes(s.B, 1) > PLAN_LDS_MAX) ? 2 : 1;
  }
  q.lds = bytes(s.B, q.RSUB);
  if (q.lds > PLAN_LDS_MAX) return false;
  p = q;
  return true;
}

// ---- the BF16 LDS-DMA engine (B = 1..4); false: shape / epilogue outside it
inline bool plan_lds16(const GemvShape& s, const GemvKnobs& kn, int cus, GemvPlan& p) {
  if (!kn.bf16_lds || s.B < 1 || s.B > 4 || s.K % 512 || s.N % 2 || s.epi == EPI_TP_RESID || s.tune_dbg ||
      (s.kernel_sel != 0 && s.kernel_sel != 3) || !s.k_ok)
    return false;
  for (int k = 0; k < s.nseg; ++k)
    if (s.qtype[k] != QT_BF16 || (k > 0 && s.seg_row0[k] % 2)) return false;
  const int npairs = s.N / 2;
  GemvPlan q{};
  q.family = GF_LDS16;
  q.B = s.B;
  q.threads = PLAN_ONE_WG_THREADS;
  q.grid = std::min(s.tune_grid > 0 ? s.tune_grid : cus, npairs);
  q.cu = CuPlan{q.grid, npairs, (2 * ((npairs + q.grid - 1) / q.grid) + 3) & ~3, nullptr};
  auto fits = [&](int R, int GPW) {
    const size_t head = (64 + (size_t)s.B * q.cu.racc_n) * 4 + (size_t)s.B * s.K * 2;
    q.R = R;
    q.GPW = GPW;
    q.lds = (head + 255) / 256 * 256 + (size_t)R * (14 * GPW * 1024);
    return q.lds <= PLAN_LDS_MAX;
  };
  // R = 3 (two 28 KB slots in flight per CU, the quantised engine's batch-1 depth), R = 2 where the
  // staged x rows leave no room (long K at B = 3..4); GemvKnobs::lb_cfg: batch 1's other geometries
  const bool ok = (s.B == 1 && kn.lb_cfg == 24 && fits(4, 2)) || (s.B == 1 && kn.lb_cfg == 14 && fits(4, 1)) ||
                  (s.B == 1 && kn.lb_cfg == 16 && fits(6, 1)) || fits(3, 2) || fits(2, 2);
  if (ok) p = q;
  return ok;
}

// ---- the CU register kernel (batch 1, probes); false: off, or the shape does not fit
inline bool plan_cu(const GemvShape& s, const GemvKnobs& kn, int cus, GemvPlan& p) {
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  if (!plan_same_xlayout(qt0, qt1)) return false;
  const int mode = s.kernel_sel == 2 ? 8 : (s.kernel_sel == 0 ? kn.cu : 0);
  if (!mode || s.B != 1 || s.tune_dbg) return false;
  GemvPlan q{};
  // tune_grid > 0: that many workgroups (tests: ragged splits, > 64 pairs per workgroup)
  q.desc = plan_desc_shape(s, s.tune_grid > 0 ? s.tune_grid : cus, 2);
  if (!gemv_desc_plan(q.desc, q.cu, q.grid)) return false;
  q.lds = (64 + (size_t)q.cu.racc_n) * 4 + (size_t)(s.K / plan_w(qt0)) * plan_runs(qt0) * 8 + (size_t)s.K + 16;
  if (q.lds > PLAN_LDS_MAX) return false;
  q.lds = std::max(q.lds, (size_t)(81 * 1024));  // one workgroup per CU
  q.family = GF_CU;
  q.B = 1;
  q.D = mode <= 4 ? 4 : 8;
  q.threads = PLAN_ONE_WG_THREADS;
  p = q;
  return true;
}

// ---- the q8 row-pair kernel (int8 activations, any B).  false: the staged x does not fit, or an
// EPI_TP_RESID launch whose rows do not fit the fused stage within the co-residency cap (the
// caller takes the separate all-reduce instead).  occupancy(plan): resident workgroups per CU of
// the plan's instantiation, asked only for the grid of the non-balanced launch.
template <class Occ>
bool plan_q8(const GemvShape& s, const GemvKnobs& kn, int cus, Occ&& occupancy, GemvPlan& p) {
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  if (!plan_same_xlayout(qt0, qt1)) return false;
  GemvPlan q{};
  q.family = GF_Q8;
  q.B = s.B == 1 ? 1 : (s.B == 2 ? 2 : (s.B <= 4 ? 4 : 8));
  const int nch = s.K / plan_w(qt0), npairs = s.N / 2;
  q.lds = 64 * 4 + (size_t)q.B * nch * plan_runs(qt0) * 8 + (size_t)q.B * s.K + 2048 + 16;
  if (q.lds > 128 * 1024) return false;
  q.kt_max = s.K;
  if (q.B == 1) {
    int u = s.tune_u;
    if (u <= 0 || (u > 8 && u != 11 && u != 12 && u != 13 && u != 14 && u != 21 && u != 22 && u != 31)) {
      // MI355X sweep (tools/gemv_probe.py --sweep): one chunk per lane per item for short K,
      // except the mid-sized Q4_K/Q5_K projections; the whole K slice in flight for long K
      // (U = 1 for the small/huge-N shapes won in the eager sweep but lost 2-3 % inside the
      // captured decode step, so the whole-K-slice rule stays)
      // (re-swept in the captured step, tools/gemv_knob_sweep.sh: U = 1 for K = 4096 gate/up
      // +1.8 %, QKV +1 %, O / lm_head neutral)
      u = nch <= 128 ? 1 : (nch <= 512 ? (nch + 63) / 64 : 2);
      // Round 4 (tools/gemv_cu_probe.py row-kernel stamps): when the balanced launch gives every
      // wave exactly ONE row pair, the double-buffered U = 1 pipeline issued the pair's second K
      // half only after the x-staging barrier -- a second memory round trip on the critical path
      // (O: barrier 1.9 us, pair computed 3.6 us).  The pair's whole K slice in one single-buffered
      // item instead: QKV 8.27 -> 7.36 us, O 5.71 -> 5.05 (profiles/qkv_prologue_r4.txt).
      if (kn.q8_balance && s.tune_grid <= 0 && npairs <= 16 * cus && nch <= 128) u = nch <= 64 ? 11 : 12;
    }
    switch (u) {
      case 11: q.U = 1; q.PIPE = 1; break;  // one pair per wave: the K slice in
      case 12: q.U = 2; q.PIPE = 1; break;  // one single-buffered item
      case 13: q.U = 3; q.PIPE = 2; break;  // tuning: U = 3/4 double-buffered
      case 14: q.U = 4; q.PIPE = 2; break;
      case 21: q.U = 1; q.PIPE = 3; break;  // tuning: triple / quad buffers
      case 22: q.U = 2; q.PIPE = 3; break;
      case 31: q.U = 1; q.PIPE = 4; break;
      case 1: q.U = 1; q.PIPE = 2; break;
      case 2: q.U = 2; q.PIPE = 2; break;
      default: q.U = (u >= 3 && u <= 7) ? u : 8; q.PIPE = 1; break;
    }
  } else {
    q.U = q.B == 8 ? 1 : 2;
    q.PIPE = 2;
  }
  // Batch 1, one pair per wave: 8-wave workgroups leave CUs unequal whenever npairs / 8 is not a
  // multiple of the CU count (Mistral QKV: 3072 pairs = 384 workgroups on 256 CUs -> half the CUs
  // stream 16 pairs, half 8).  Instead size the workgroup to ceil(npairs / CUs) waves (<= 16) and
  // launch one per CU: every CU streams the same bytes (GemvKnobs::q8_balance = 0: the 8-wave grid).
  int nw = PLAN_Q8_WAVES;
  int blocks = 0;
  if (q.B == 1 && kn.q8_balance && s.tune_grid <= 0 && npairs >= 2 * cus) {
    // round 4: also for the register-heavy U >= 3 variants (<= 8 waves) and for shapes with more
    // pairs than waves (ppw pairs per wave, one workgroup per CU): TinyLlama's down (1024 pairs,
    // U = 3) ran 128 8-wave workgroups on half the chip, its gate/up (5632 pairs) 512 workgroups with
    // 1 or 2 pairs per wave
    const int maxw = plan_q8_max_threads(q.U, q.PIPE) / 64;
    const int ppw = (npairs + cus * maxw - 1) / (cus * maxw);
    int want = (npairs + cus * ppw - 1) / (cus * ppw);
    bool mixed = false;
    int np0 = 0;
    if (qt0 != qt1 && s.nseg > 1 && ppw == 1) {
      // mixed formats: whole waves per format in every workgroup (the kernel splits nw by pair
      // counts), e.g. TinyLlama's QKV 1152 Q4_K + 128 Q6_K pairs -> 5 + 1 waves, not 4 + 1
      np0 = s.seg_row0[s.nseg - 1] / 2;
      want = (np0 + cus - 1) / cus + (npairs - np0 + cus - 1) / cus;
      mixed = true;
    }
    // several pairs per wave only for the long-K (U >= 3) shapes: TinyLlama's 5632-pair gate/up at
    // U = 1 went 6.96 -> 9.15 us as 3 pairs per wave on one 8-wave workgroup per CU
    // (profiles/decode_tinyllama_rocprof_r4.txt)
    if (want >= 2 && want <= maxw && (ppw == 1 || q.U >= 3)) {
      nw = want;
      blocks = std::min(cus, (npairs + nw - 1) / nw);
      if (mixed) {
        // the grid must cover each format's pairs with ITS waves (the kernel's split):
        // 214 blocks x 5 Q4_K waves left 82 of TinyLlama's 1152 Q|K pairs to a second pass (9.5 us)
        int nw0 = (int)(((long)nw * np0 + npairs / 2) / npairs);
        nw0 = std::max(1, std::min(nw - 1, nw0));
        const int nw1 = nw - nw0;
        blocks = std::min(cus, std::max((np0 + nw0 - 1) / nw0, (npairs - np0 + nw1 - 1) / nw1));
      }
    }
  }
  if (!blocks) {
    int per_cu = s.tune_grid;  // tune_grid > 0: workgroups per CU
    if (per_cu <= 0) {
      per_cu = std::min(std::max(1, (int)occupancy(q)), 2);
      q.occ_grid = true;
    }
    blocks = std::min((npairs + nw - 1) / nw, cus * per_cu);
  }
  if (s.epi == EPI_TP_RESID) {
    // fused all-reduce: at most grid_cap workgroups (every rank sharing a GPU resident at once --
    // spinning workgroups past it could wait on peers that cannot be scheduled), at most
    // TPF_SLOTS, and each workgroup's pairs inside its stage slot (TPF_CAP values)
    const int cap = s.grid_cap > 0 ? std::min(s.grid_cap, PLAN_TPF_SLOTS) : PLAN_TPF_SLOTS;
    blocks = std::min(blocks, cap);
    auto per_wg = [&](int g) { return 2 * nw * ((npairs + g * nw - 1) / (g * nw)); };
    while (per_wg(blocks) > PLAN_TPF_CAP && blocks < cap) ++blocks;
    if (per_wg(blocks) > PLAN_TPF_CAP) return false;
  }
  q.grid = blocks;
  q.threads = nw * 64;
  p = q;
  return true;
}

// ---- the persistent fp32 kernel (B <= 4); false: B * K floats of x (+ run sums) exceed 96 KB
template <class Occ>
bool plan_persistent(const GemvShape& s, int cus, Occ&& occupancy, GemvPlan& p) {
  if (s.B > 4) return false;
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  GemvPlan q{};
  q.family = GF_PERSISTENT;
  q.B = s.B == 1 ? 1 : (s.B == 2 ? 2 : 4);
  q.U = q.B == 4 ? 1 : 2;
  const size_t xfl = (size_t)q.B * s.K + (size_t)q.B * s.K / 16;
  q.lds = (64 + xfl * (plan_same_xlayout(qt0, qt1) ? 1 : 2) + 4) * sizeof(float);
  if (q.lds > 96 * 1024) return false;
  // grid = min(row groups, CUs x resident workgroups per CU (VGPR + LDS limited))
  const int per_cu = std::max(1, std::min(std::max(1, (int)occupancy(q)), (int)(PLAN_LDS_MAX / q.lds)));
  q.occ_grid = true;
  q.grid = std::min((s.N / 2 + PLAN_GP_WAVES - 1) / PLAN_GP_WAVES, cus * per_cu);
  q.threads = PLAN_GP_THREADS;
  q.kt_max = s.K;
  p = q;
  return true;
}

// ---- the v1 fp32 kernel: serves every checked shape (K tiles of x in LDS)
inline void plan_v1(const GemvShape& s, GemvPlan& p) {
  GemvPlan q{};
  q.family = GF_V1;
  q.B = s.B == 1 ? 1 : (s.B == 2 ? 2 : (s.B <= 4 ? 4 : 8));
  const int chunks_per_lane = (s.K / plan_w(s.qtype[0]) + 63) / 64;
  q.U = q.B == 1 ? (chunks_per_lane >= 4 ? 4 : 2) : (q.B == 8 ? 1 : 2);
  int kt = (PLAN_V1_LDS_FLOATS / q.B) / 256 * 256;
  if (kt >= s.K) kt = s.K;
  int blk = 8;
  for (int k = 0; k < s.nseg; ++k) blk = std::max(blk, plan_qtype_block(s.qtype[k]));
  if (kt < blk) kt = blk;
  q.kt_max = kt;
  q.lds = (64 + (size_t)q.B * kt + (size_t)q.B * kt / 16 + 4) * sizeof(float);
  q.grid = (s.N + PLAN_V1_ROWS_PER_BLOCK - 1) / PLAN_V1_ROWS_PER_BLOCK;
  q.threads = PLAN_V1_THREADS;
  p = q;
}

// The plan of launch_gemv: the cascade of the families, in order.  Throws where launch_gemv does.
// check = false skips gemv_check (tests: format pairs no kernel is compiled for).
template <class Occ>
GemvPlan gemv_plan(const GemvShape& s, const GemvKnobs& kn, int cus, Occ&& occupancy, bool check = true) {
  if (check) gemv_check(s);
  const int qt0 = s.qtype[0], qt1 = s.qtype[s.nseg - 1];
  GemvPlan p{};
  if (!plan_is16(qt0) && !s.force_v1 && s.act_q8) {
    if (s.B <= 4 && plan_lds(s, kn, cus, p)) return p;  // B = 1..4: the LDS-DMA engine
    if (plan_cu(s, kn, cus, p)) return p;
    if (plan_q8(s, kn, cus, occupancy, p)) return p;
  }
  if (qt0 == QT_BF16 && qt1 == QT_BF16 && !s.force_v1 && plan_lds16(s, kn, cus, p)) return p;
  if (s.epi == EPI_TP_RESID)  // only the row-pair int8 kernel does the fused all-reduce epilogue
    throw std::runtime_error("gemv: EPI_TP_RESID launch not taken by the row-pair kernel (use launch_gemv_tp_fused)");
  if (s.x16 || s.y16) throw std::runtime_error("bf16 GEMV input / SwiGLU output: int8-activation kernels only");
  if (!s.force_v1 && plan_persistent(s, cus, occupancy, p)) return p;
  plan_v1(s, p);
  return p;
}

// The plan of launch_gemv_tp_fused (EPI_TP_RESID, batch 1): the row-pair kernel, or GF_NONE
// (format, shape or stage capacity outside it: the caller runs the plain GEMV and an all-reduce)
template <class Occ>
GemvPlan plan_tp_fused(const GemvShape& s, const GemvKnobs& kn, int cus, Occ&& occupancy) {
  GemvPlan p{};
  if (s.nseg != 1 || s.epi != EPI_TP_RESID || s.B != 1 || !s.act_q8) return p;
  if (plan_is16(s.qtype[0]) || gemv_pair_index(s.qtype[0], s.qtype[0]) < 0) return p;
  if (!plan_q8(s, kn, cus, occupancy, p)) p = GemvPlan{};
  return p;
}

// ---- questions that launch nothing.  The family never depends on occupancy.
// GF_NONE where gemv_plan would throw.
inline int gemv_plan_family(const GemvShape& s, const GemvKnobs& kn, int cus, bool tp_fused = false) {
  auto one = [](const GemvPlan&) { return 1; };
  try {
    return tp_fused ? plan_tp_fused(s, kn, cus, one).family : gemv_plan(s, kn, cus, one).family;
  } catch (const std::runtime_error&) {
    return GF_NONE;
  }
}
// Whether the B-row LDS-DMA engine serves the int8-activation launch of this shape (B = 1..4, the
// LDS plan fits 160 KB).  16-bit weights never take the engine and report true (their B-row kernels
// are the only GEMV path).  The engine's batched-decode path choice asks this per projection, about
// the shape: an fp32-activation engine gets the same answer.
inline bool gemv_engine_fits(GemvShape s, const GemvKnobs& kn, int cus) {
  if (plan_is16(s.qtype[0])) return true;
  s.act_q8 = 1;
  s.force_v1 = 0;
  return gemv_plan_family(s, kn, cus) == GF_LDS;
}
inline bool gemv_bf16_engine_fits(const GemvShape& s, const GemvKnobs& kn, int cus) {
  return gemv_plan_family(s, kn, cus) == GF_LDS16;
}

}  // namespace aios
