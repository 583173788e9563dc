// Host dispatcher: (segment-0 format, last-segment format) -> kernel instantiation.
#include <array>
#include <utility>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "../gemv.h"
#include "../gemv_desc.h"
#include "../gemv_plan.h"

namespace aios {

// ---- launch descriptor cache (gemv_desc.h): process-wide, one arena list per device, nothing is
// ever freed or moved, so a pointer handed to a captured graph stays valid for the process' life.
// Allocation and upload run in relaxed capture mode on a private non-blocking stream: neither
// touches a capturing stream, and a first use inside an engine's graph capture is legal.
namespace {
struct DescArena {
  GemvWgDesc* dev = nullptr;
  size_t cap = 0, used = 0;  // records
};
struct DescDevice {
  std::vector<DescArena> arenas;
  hipStream_t st = nullptr;
  std::map<std::array<int, 14>, const GemvWgDesc*> cache;
};
std::mutex g_desc_mu;
std::map<int, DescDevice> g_desc_dev;
constexpr size_t DESC_ARENA_RECORDS = 32768;  // 2 MB: 128 whole-chip descriptors

struct RelaxedCapture {  // this thread's capture mode -> relaxed for the scope
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
  ~RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
};

GemvWgDesc* desc_alloc(DescDevice& d, size_t n) {
  if (d.arenas.empty() || d.arenas.back().used + n > d.arenas.back().cap) {
    DescArena a;
    a.cap = std::max(n, DESC_ARENA_RECORDS);
    HIP_CHECK(hipMalloc((void**)&a.dev, a.cap * sizeof(GemvWgDesc)));
    d.arenas.push_back(a);
  }
  DescArena& a = d.arenas.back();
  GemvWgDesc* p = a.dev + a.used;
  a.used += n;
  return p;
}
}  // namespace

void gemv_desc_reserve() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_desc_mu);
  DescDevice& d = g_desc_dev[dev];
  RelaxedCapture rc;
  if (!d.st) HIP_CHECK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  if (d.arenas.empty()) {
    desc_alloc(d, 1);
    d.arenas.back().used = 0;
  }
}

const GemvWgDesc* gemv_desc_device(const GemvDescShape& s, const CuPlan& pl, int G) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  // (g0 / np0 / G follow from the shape and the grid: the key needs only those)
  const std::array<int, 14> key = {s.nseg, s.qtype[0], s.qtype[1], s.qtype[2], s.seg_row0[0], s.seg_row0[1],
                                   s.seg_row0[2], s.N, s.K, s.grid, s.variant, G, pl.g0, pl.np0};
  std::lock_guard<std::mutex> lk(g_desc_mu);
  DescDevice& d = g_desc_dev[dev];
  auto it = d.cache.find(key);
  if (it != d.cache.end()) return it->second;
  const std::vector<GemvWgDesc> host = gemv_desc_build(s, pl, G);
  RelaxedCapture rc;
  if (!d.st) HIP_CHECK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  GemvWgDesc* p = desc_alloc(d, host.size());
  HIP_CHECK(hipMemcpyAsync(p, host.data(), host.size() * sizeof(GemvWgDesc), hipMemcpyHostToDevice, d.st));
  HIP_CHECK(hipStreamSynchronize(d.st));
  d.cache.emplace(key, p);
  return p;
}

// ---- one table of the compiled format pairs (GEMV_PAIRS, gemv_plan.h) -> their entry points
template <int QT0, int QT1>
GemvPlan gemv_pair(const GemvArgs&, hipStream_t, int);  // kernels/gemv_impl.h, instantiated per pair
namespace {
using PairFn = GemvPlan (*)(const GemvArgs&, hipStream_t, int);
template <size_t... I>
constexpr std::array<PairFn, GEMV_NPAIRS> pair_table(std::index_sequence<I...>) {
  return {&gemv_pair<GEMV_PAIRS[I].qt0, GEMV_PAIRS[I].qt1>...};
}
constexpr auto PAIR_FN = pair_table(std::make_index_sequence<GEMV_NPAIRS>{});
}  // namespace

bool gemv_supports(int qt0, int qt1) { return gemv_pair_index(qt0, qt1) >= 0; }

bool gemv_engine_fits(const GemvArgs& a) { return gemv_engine_fits(gemv_shape(a), gemv_knobs(), device_cu_count()); }
bool gemv_bf16_engine_fits(const GemvArgs& a) {
  return gemv_bf16_engine_fits(gemv_shape(a), gemv_knobs(), device_cu_count());
}

// EPI_TP_RESID (the TP all-reduce in the GEMV epilogue): launched by the row-pair kernel, or false
// with nothing launched (format, shape or stage capacity outside it) -- the caller then runs the
// plain GEMV and a separate all-reduce.  a.dry: only whether it would launch.
bool launch_gemv_tp_fused(const GemvArgs& a, hipStream_t st) {
  if (a.dry) return gemv_plan_family(gemv_shape(a), gemv_knobs(), device_cu_count(), true) == GF_Q8;
  const int i = a.nseg == 1 ? gemv_pair_index(a.seg[0].qtype, a.seg[0].qtype) : -1;
  return i >= 0 && PAIR_FN[i](a, st, GEMV_TP_FUSED).family == GF_Q8;  // (GF_NONE: nothing launched)
}

void launch_gemv(const GemvArgs& a, hipStream_t st) {
  const GemvShape s = gemv_shape(a);
  gemv_check(s);  // (throws: segment count, batch range, alignment, unsupported pair)
  PAIR_FN[gemv_pair_index(s.qtype[0], s.qtype[s.nseg - 1])](a, st, 0);
}
}  // namespace aios
