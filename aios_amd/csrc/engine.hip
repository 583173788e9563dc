// Engine implementation -- see engine.h.
#include "engine.h"
#include <hip/hip_ext.h>

#include <set>
#include "comm.h"
#include <cstdlib>
#include <map>

#include <algorithm>
#include <cstring>
#include <cmath>
#include <limits>
#include <regex>
#include <sstream>

#include <rocprofiler-sdk-roctx/roctx.h>

namespace aios {

static bool trace_enabled() {
  static const int on = [] {
    const char* e = std::getenv("AIOS_TRACE");
    return e && std::atoi(e) == 0 ? 0 : 1;
  }();
  return on != 0;
}
TraceRange::TraceRange(const char* name) : on(trace_enabled()) {
  if (on) roctxRangePushA(name);
}
TraceRange::~TraceRange() {
  if (on) roctxRangePop();
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static bool is_kquant(int qt) { return qt == QT_Q4_K || qt == QT_Q5_K || qt == QT_Q6_K; }
static int block_elems(int qt) {
  if (is_kquant(qt) || qt == QT_Q2_K || qt == QT_Q3_K || qt == QT_IQ4_XS) return 256;
  if (qt == QT_F32 || qt == QT_F16 || qt == QT_BF16) return 1;
  return 32;
}
static int block_bytes(int qt) {
  switch (qt) {
    case QT_Q4_K: return 144;
    case QT_Q5_K: return 176;
    case QT_Q6_K: return 210;
    case QT_Q4_0: return 18;
    case QT_Q4_1: return 20;
    case QT_Q5_0: return 22;
    case QT_Q5_1: return 24;
    case QT_Q8_0: return 34;
    case QT_Q2_K: return 84;
    case QT_Q3_K: return 110;
    case QT_IQ4_NL: return 18;
    case QT_IQ4_XS: return 136;
    case QT_F16:
    case QT_BF16: return 2;
    case QT_F32: return 4;
  }
  throw std::runtime_error("unsupported ggml type " + std::to_string(qt));
}
// formats the GEMV streams natively; others are expanded to BF16 at load
static bool native_qtype(int qt) {
  return qt == QT_Q4_K || qt == QT_Q5_K || qt == QT_Q6_K || qt == QT_Q4_0 || qt == QT_Q8_0 || qt == QT_F16 ||
         qt == QT_BF16;
}

Engine::Engine(const EngineConfig& cfg) : cfg_(cfg) {
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (!cfg_.cu_mask.empty()) {
    int n = 0, dev_cus = 0;
    for (uint32_t w : cfg_.cu_mask) n += __builtin_popcount(w);
    HIP_CHECK(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, cfg_.device));
    if (n <= 0) throw std::runtime_error("cu_mask selects no CU");
    HIP_CHECK(hipExtStreamCreateWithCUMask(&stream_, (uint32_t)cfg_.cu_mask.size(), cfg_.cu_mask.data()));
    cus_ = std::min(n, dev_cus);
  } else if (cfg_.stream_priority != 0) {
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int pr = std::max(greatest, std::min(least, cfg_.stream_priority));
    HIP_CHECK(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, pr));
  } else {
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  }
  gemv_desc_reserve();  // the GEMV launch descriptors' device arena: allocated outside any graph capture

  layers_.resize(cfg_.n_layers);
  // B <= 8 decodes through the fused GEMVs; larger batches (up to 64) through the MFMA GEMM path
  if (cfg_.max_batch < 1 || cfg_.max_batch > 64) throw std::runtime_error("max_batch must be 1..64");
  if (cfg_.max_slots < cfg_.max_batch) cfg_.max_slots = cfg_.max_batch;
  if (cfg_.tp_size <= 1 || cfg_.tie_embeddings) cfg_.vocab_parallel = 0;
  if (cfg_.vocab_parallel && cfg_.vocab_size % cfg_.tp_size)
    throw std::runtime_error("vocab_parallel: vocab_size not divisible by tp_size");
}

Engine::~Engine() {
  try {
    stage_release();
  } catch (...) {
  }
  for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  for (void* p : allocs_) hipFree(p);
  if (h_par_) hipHostFree(h_par_);
  if (h_tok_out_) hipHostFree(h_tok_out_);
  if (h_mask_) hipHostFree(h_mask_);
  if (h_proc_) hipHostFree(h_proc_);
  if (h_lp_) hipHostFree(h_lp_);
  if (h_gr_) hipHostFree(h_gr_);
  if (d_tok_bytes_) hipFree(d_tok_bytes_);
  for (auto& g : grammars_)
    if (g.buf) hipFree(g.buf);
  if (h_spec_) hipHostFree(h_spec_);
  if (h_specm_) hipHostFree(h_specm_);
  if (snap_dev_) hipFree(snap_dev_);
  for (void* h : snap_host_)
    if (h) hipHostFree(h);
  for (hipEvent_t e : snap_ev_)
    if (e) hipEventDestroy(e);
  if (pipe_ev_) hipEventDestroy(pipe_ev_);
  if (stream_) hipStreamDestroy(stream_);
}

void* Engine::dmalloc(size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
  allocs_.push_back(p);
  return p;
}

QMat Engine::alloc_qmat(int qt, int rows, int cols) {
  if (cols % block_elems(qt)) throw std::runtime_error("matrix cols not a multiple of the quant block");
  QMat m;
  m.w.qtype = qt;
  m.w.rows = rows;
  m.w.cols = cols;
  const size_t nb = (size_t)rows * (cols / block_elems(qt));
  size_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  switch (qt) {
    case QT_Q4_K: s0 = nb * 128; s1 = nb * 16; break;
    case QT_Q5_K: s0 = nb * 128; s1 = nb * 16; s2 = nb * 32; break;
    case QT_Q6_K: s0 = nb * 128; s1 = nb * 64; s2 = nb * 16; s3 = nb * 2; break;
    case QT_Q4_0: s0 = nb * 16; s1 = nb * 2; break;
    case QT_Q8_0: s0 = nb * 32; s1 = nb * 2; break;
    case QT_F16:
    case QT_BF16: s0 = (size_t)rows * cols * 2; break;
    default: throw std::runtime_error("alloc_qmat: non-native type");
  }
  const size_t a = 256;
  const size_t o1 = align_up(s0, a), o2 = o1 + align_up(s1, a), o3 = o2 + align_up(s2, a);
  m.bytes = o3 + align_up(s3, a) + 64;
  m.buf = dmalloc(m.bytes);
  uint8_t* base = (uint8_t*)m.buf;
  m.w.p0 = base;
  m.w.p1 = s1 ? base + o1 : nullptr;
  m.w.p2 = s2 ? base + o2 : nullptr;
  m.w.p3 = s3 ? base + o3 : nullptr;
  weight_bytes_ += m.bytes;
  return m;
}

// Load path (one hipMalloc + pageable copy + stream sync + hipFree per tensor).
// Now: the GGUF bytes (mmap'd by the loader) are copied in 64 MB chunks through two pinned host
// buffers into one of two device staging buffers (DMA from pinned memory, the next chunk's host
// memcpy overlapping the previous chunk's transfer), and the repack kernel of tensor i runs while
// tensor i+1 is being staged into the other buffer.  No per-tensor allocation or device sync.
void Engine::stage_upload(const void* host, size_t nbytes, void*& dev_staging) {
  constexpr size_t CHUNK = 64ull << 20;
  const int k = stage_next_;
  stage_next_ ^= 1;
  if (stage_ev_[k]) HIP_CHECK(hipEventSynchronize(stage_ev_[k]));  // repack of the tensor two back is done
  if (stage_dev_bytes_[k] < nbytes) {
    if (stage_dev_[k]) HIP_CHECK(hipFree(stage_dev_[k]));
    stage_dev_bytes_[k] = std::max(nbytes, (size_t)256 << 20);
    HIP_CHECK(hipMalloc(&stage_dev_[k], stage_dev_bytes_[k]));
  }
  for (int i = 0; i < 2; ++i)
    if (!stage_host_[i]) {
      HIP_CHECK(hipHostMalloc(&stage_host_[i], CHUNK, hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&stage_host_ev_[i], hipEventDisableTiming));
      HIP_CHECK(hipEventRecord(stage_host_ev_[i], stream_));
    }
  for (size_t off = 0; off < nbytes; off += CHUNK) {
    const size_t n = std::min(CHUNK, nbytes - off);
    const int h = stage_host_next_;
    stage_host_next_ ^= 1;
    HIP_CHECK(hipEventSynchronize(stage_host_ev_[h]));  // this pinned buffer's last transfer is done
    std::memcpy(stage_host_[h], (const uint8_t*)host + off, n);
    HIP_CHECK(hipMemcpyAsync((uint8_t*)stage_dev_[k] + off, stage_host_[h], n, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipEventRecord(stage_host_ev_[h], stream_));
  }
  dev_staging = stage_dev_[k];
  stage_cur_ = k;
}

void Engine::stage_done() {
  const int k = stage_cur_;
  if (!stage_ev_[k]) HIP_CHECK(hipEventCreateWithFlags(&stage_ev_[k], hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(stage_ev_[k], stream_));
}

void Engine::stage_release() {
  HIP_CHECK(hipStreamSynchronize(stream_));
  for (int i = 0; i < 2; ++i) {
    if (stage_dev_[i]) HIP_CHECK(hipFree(stage_dev_[i]));
    if (stage_host_[i]) HIP_CHECK(hipHostFree(stage_host_[i]));
    if (stage_ev_[i]) HIP_CHECK(hipEventDestroy(stage_ev_[i]));
    if (stage_host_ev_[i]) HIP_CHECK(hipEventDestroy(stage_host_ev_[i]));
    stage_dev_[i] = stage_host_[i] = nullptr;
    stage_ev_[i] = stage_host_ev_[i] = nullptr;
    stage_dev_bytes_[i] = 0;
  }
}

QMat Engine::upload_qmat(int qt, int rows, int cols, const void* host, size_t nbytes) {
  const size_t expect = (size_t)rows * (cols / block_elems(qt)) * block_bytes(qt);
  if (nbytes != expect)
    throw std::runtime_error("tensor byte size mismatch: got " + std::to_string(nbytes) + " expected " +
                             std::to_string(expect));
  QMat m;
  if ((qt == QT_F16 || qt == QT_BF16)) {  // final layout == file layout: straight into place
    m = alloc_qmat(qt, rows, cols);
    void* staging = nullptr;
    stage_upload(host, nbytes, staging);
    HIP_CHECK(hipMemcpyAsync(m.buf, staging, nbytes, hipMemcpyDeviceToDevice, stream_));
    stage_done();
    return m;
  }
  void* staging = nullptr;
  stage_upload(host, nbytes, staging);
  if (native_qtype(qt)) {
    m = alloc_qmat(qt, rows, cols);
    launch_repack(qt, staging, (size_t)rows * (cols / block_elems(qt)), m.w, stream_);
  } else {
    m = alloc_qmat(QT_BF16, rows, cols);
    launch_legacy_to_bf16(qt, staging, (size_t)rows * cols, m.buf, stream_);
  }
  stage_done();
  return m;
}

float* Engine::upload_f32(const void* host, size_t n, int qt) {
  std::vector<float> tmp(n);
  if (qt == QT_F32) {
    std::memcpy(tmp.data(), host, n * 4);
  } else if (qt == QT_F16 || qt == QT_BF16) {
    const uint16_t* h = (const uint16_t*)host;
    for (size_t i = 0; i < n; ++i) {
      if (qt == QT_BF16) {
        uint32_t u = (uint32_t)h[i] << 16;
        std::memcpy(&tmp[i], &u, 4);
      } else {
        // IEEE half -> float
        const uint32_t s = (h[i] >> 15) & 1, e = (h[i] >> 10) & 31, f = h[i] & 1023;
        float v;
        if (e == 0) v = std::ldexp((float)f, -24);
        else if (e == 31) v = f ? NAN : INFINITY;
        else v = std::ldexp((float)(f | 1024), (int)e - 25);
        tmp[i] = s ? -v : v;
      }
    }
  } else {
    throw std::runtime_error("norm/bias tensors must be F32/F16/BF16");
  }
  float* d = (float*)dmalloc(n * 4);
  HIP_CHECK(hipMemcpy(d, tmp.data(), n * 4, hipMemcpyHostToDevice));
  weight_bytes_ += n * 4;
  return d;
}

// rows of a and b interleaved: out row 2i = a row i, 2i+1 = b row i (gate/up -> SwiGLU pairs)
QMat Engine::interleave_rows(const QMat& a, const QMat& b) {
  if (a.w.qtype != b.w.qtype || a.w.rows != b.w.rows || a.w.cols != b.w.cols)
    throw std::runtime_error("gate/up shape or format mismatch");
  QMat m = alloc_qmat(a.w.qtype, 2 * a.w.rows, a.w.cols);
  const int rows = a.w.rows;
  const size_t nbr = a.w.cols / block_elems(a.w.qtype);  // blocks per row
  auto copy_stream = [&](const uint8_t* dst, const uint8_t* sa, const uint8_t* sb, size_t row_bytes) {
    if (!dst) return;
    HIP_CHECK(hipMemcpy2DAsync((void*)dst, 2 * row_bytes, sa, row_bytes, row_bytes, rows, hipMemcpyDeviceToDevice,
                               stream_));
    HIP_CHECK(hipMemcpy2DAsync((void*)(dst + row_bytes), 2 * row_bytes, sb, row_bytes, row_bytes, rows,
                               hipMemcpyDeviceToDevice, stream_));
  };
  size_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
  switch (a.w.qtype) {
    case QT_Q4_K: r0 = nbr * 128; r1 = nbr * 16; break;
    case QT_Q5_K: r0 = nbr * 128; r1 = nbr * 16; r2 = nbr * 32; break;
    case QT_Q6_K: r0 = nbr * 128; r1 = nbr * 64; r2 = nbr * 16; r3 = nbr * 2; break;
    case QT_Q4_0: r0 = nbr * 16; r1 = nbr * 2; break;
    case QT_Q8_0: r0 = nbr * 32; r1 = nbr * 2; break;
    default: r0 = (size_t)a.w.cols * 2; break;
  }
  copy_stream(m.w.p0, a.w.p0, b.w.p0, r0);
  if (r1) copy_stream(m.w.p1, a.w.p1, b.w.p1, r1);
  if (r2) copy_stream(m.w.p2, a.w.p2, b.w.p2, r2);
  if (r3) copy_stream(m.w.p3, a.w.p3, b.w.p3, r3);
  HIP_CHECK(hipStreamSynchronize(stream_));
  return m;
}

void Engine::set_tensor(const std::string& name, int qt, int rows, int cols, const void* host, size_t nbytes) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (finalized_) throw std::runtime_error("set_tensor after finalize");
  HIP_CHECK(hipSetDevice(cfg_.device));
  static const std::regex blk_re(R"(blk\.(\d+)\.(.+))");
  std::smatch m;
  if (name == "token_embd.weight") {
    tok_embd_ = upload_qmat(qt, rows, cols, host, nbytes);
    return;
  }
  if (name == "output.weight") {
    if (cfg_.vocab_parallel && rows != cfg_.vocab_size / cfg_.tp_size)
      throw std::runtime_error("vocab-parallel output.weight: expected " +
                               std::to_string(cfg_.vocab_size / cfg_.tp_size) + " rows (this rank's shard)");
    output_ = upload_qmat(qt, rows, cols, host, nbytes);
    return;
  }
  if (name == "output_norm.weight") {
    out_norm_ = upload_f32(host, (size_t)rows * cols, qt);
    return;
  }
  if (!std::regex_match(name, m, blk_re)) throw std::runtime_error("unknown tensor " + name);
  const int l = std::stoi(m[1]);
  if (l < 0 || l >= cfg_.n_layers) throw std::runtime_error("layer index out of range in " + name);
  const std::string t = m[2];
  LayerW& L = layers_[l];
  const size_t n = (size_t)rows * cols;
  if (t == "attn_norm.weight") L.attn_norm = upload_f32(host, n, qt);
  else if (t == "ffn_norm.weight") L.ffn_norm = upload_f32(host, n, qt);
  else if (t == "attn_q_norm.weight") L.q_norm = upload_f32(host, n, qt);
  else if (t == "attn_k_norm.weight") L.k_norm = upload_f32(host, n, qt);
  else if (t == "attn_q.weight") L.wq = upload_qmat(qt, rows, cols, host, nbytes);
  else if (t == "attn_k.weight") L.wk = upload_qmat(qt, rows, cols, host, nbytes);
  else if (t == "attn_v.weight") L.wv = upload_qmat(qt, rows, cols, host, nbytes);
  else if (t == "attn_output.weight") L.wo = upload_qmat(qt, rows, cols, host, nbytes);
  else if (t == "ffn_down.weight") L.wdown = upload_qmat(qt, rows, cols, host, nbytes);
  else if (t == "ffn_gate.weight" || t == "ffn_up.weight") {
    const std::string other = (t == "ffn_gate.weight") ? "ffn_up.weight" : "ffn_gate.weight";
    const std::string key = "blk." + std::to_string(l) + ".";
    QMat q = upload_qmat(qt, rows, cols, host, nbytes);
    auto it = pending_.find(key + other);
    if (it == pending_.end()) {
      pending_[key + t] = q;
    } else {
      const QMat& g = (t == "ffn_gate.weight") ? q : it->second;
      const QMat& u = (t == "ffn_gate.weight") ? it->second : q;
      L.wgu = interleave_rows(g, u);
      // the separate copies are no longer needed
      for (const QMat* mm : {&q, &it->second}) {
        auto pos = std::find(allocs_.begin(), allocs_.end(), mm->buf);
        if (pos != allocs_.end()) allocs_.erase(pos);
        weight_bytes_ -= mm->bytes;
        HIP_CHECK(hipFree(mm->buf));
      }
      pending_.erase(it);
    }
  } else if (t == "attn_q.bias" || t == "attn_k.bias" || t == "attn_v.bias") {
    const int qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
    if (!L.bqkv) {
      L.bqkv = (float*)dmalloc((size_t)(qd + 2 * kvd) * 4);
      HIP_CHECK(hipMemset(L.bqkv, 0, (size_t)(qd + 2 * kvd) * 4));
    }
    const int off = t == "attn_q.bias" ? 0 : (t == "attn_k.bias" ? qd : qd + kvd);
    float* tmp = upload_f32(host, n, qt);
    HIP_CHECK(hipMemcpy(L.bqkv + off, tmp, n * 4, hipMemcpyDeviceToDevice));
  } else {
    throw std::runtime_error("unknown layer tensor " + name);
  }
}

void Engine::init_random(const std::string& recipe_in, uint64_t seed) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  TraceRange tr("aios.init_random");
  HIP_CHECK(hipSetDevice(cfg_.device));
  std::string r = recipe_in;
  std::transform(r.begin(), r.end(), r.begin(), ::toupper);
  const int d = cfg_.d_model, qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
  const int ff = cfg_.d_ff, V = cfg_.vocab_size, NL = cfg_.n_layers;
  auto more_bits = [&](int i) { return i < NL / 8 || i >= 7 * NL / 8 || (i - NL / 8) % 3 == 2; };
  auto type_for = [&](const std::string& t, int layer) -> int {
    if (r == "Q4_K_M") {
      if (t == "output") return QT_Q6_K;
      if (t == "attn_v" || t == "ffn_down") return more_bits(layer) ? QT_Q6_K : QT_Q4_K;
      return QT_Q4_K;
    }
    if (r == "Q5_K_M") {
      if (t == "output") return QT_Q6_K;
      if (t == "attn_v" || t == "ffn_down") return more_bits(layer) ? QT_Q6_K : QT_Q5_K;
      return QT_Q5_K;
    }
    if (r == "Q4_K") return QT_Q4_K;
    if (r == "Q6_K") return QT_Q6_K;
    if (r == "Q4_0") return t == "output" ? QT_Q6_K : QT_Q4_0;
    if (r == "Q8_0") return QT_Q8_0;
    if (r == "F16") return QT_F16;
    if (r == "BF16") return QT_BF16;
    // recipes whose formats the loader expands to bf16 (Q2_K / Q3_K / IQ4 / legacy 32-blocks): in HBM
    // their matrices ARE bf16, next to the native K-quants the mix keeps (models/config.py tensor_type)
    if (r == "Q3_K_M") {
      if (t == "output") return QT_Q6_K;
      if (t == "attn_v" || t == "ffn_down") return more_bits(layer) ? QT_Q5_K : QT_Q4_K;
      return t == "attn_output" ? QT_Q4_K : QT_BF16;
    }
    if (r == "Q2_K") {
      if (t == "output") return QT_Q6_K;
      return (t == "attn_v" || t == "ffn_down") && more_bits(layer) ? QT_Q4_K : QT_BF16;
    }
    if (r == "IQ4_NL" || r == "IQ4_XS" || r == "Q4_1" || r == "Q5_0" || r == "Q5_1") return t == "output" ? QT_Q6_K : QT_BF16;
    throw std::runtime_error("unknown recipe " + recipe_in);
  };
  uint64_t s = seed * 1000003ULL;
  auto mk = [&](int qt, int rows, int cols, float amp) {
    QMat m = alloc_qmat(qt, rows, cols);
    fill_random_weight(m.w, ++s, amp, stream_);
    return m;
  };
  auto vec = [&](int n, float base, float amp) {
    float* p = (float*)dmalloc((size_t)n * 4);
    weight_bytes_ += (size_t)n * 4;
    fill_random_f32(p, n, ++s, base, amp, stream_);
    return p;
  };
  const float amp = 0.02f;
  tok_embd_ = mk(type_for("token_embd", 0), V, d, 1.0f);
  if (!cfg_.tie_embeddings) output_ = mk(type_for("output", 0), cfg_.vocab_parallel ? V / cfg_.tp_size : V, d, amp);
  out_norm_ = vec(d, 1.f, 0.1f);
  for (int l = 0; l < NL; ++l) {
    LayerW& L = layers_[l];
    L.attn_norm = vec(d, 1.f, 0.1f);
    L.ffn_norm = vec(d, 1.f, 0.1f);
    if (cfg_.qk_norm) {
      L.q_norm = vec(cfg_.head_dim, 1.f, 0.1f);
      L.k_norm = vec(cfg_.head_dim, 1.f, 0.1f);
    }
    if (cfg_.qkv_bias) L.bqkv = vec(qd + 2 * kvd, 0.f, 0.02f);
    L.wq = mk(type_for("attn_q", l), qd, d, amp);
    L.wk = mk(type_for("attn_k", l), kvd, d, amp);
    L.wv = mk(type_for("attn_v", l), kvd, d, amp);
    L.wo = mk(type_for("attn_output", l), d, qd, amp);
    L.wgu = mk(type_for("ffn_gate", l), 2 * ff, d, amp);
    L.wdown = mk(type_for("ffn_down", l), d, ff, amp);
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
}

std::vector<std::string> Engine::missing_tensors() const {
  std::vector<std::string> miss;
  if (!tok_embd_.valid()) miss.push_back("token_embd.weight");
  if (!out_norm_) miss.push_back("output_norm.weight");
  for (int l = 0; l < cfg_.n_layers; ++l) {
    const LayerW& L = layers_[l];
    const std::string p = "blk." + std::to_string(l) + ".";
    if (!L.attn_norm) miss.push_back(p + "attn_norm.weight");
    if (!L.ffn_norm) miss.push_back(p + "ffn_norm.weight");
    if (!L.wq.valid()) miss.push_back(p + "attn_q.weight");
    if (!L.wk.valid()) miss.push_back(p + "attn_k.weight");
    if (!L.wv.valid()) miss.push_back(p + "attn_v.weight");
    if (!L.wo.valid()) miss.push_back(p + "attn_output.weight");
    if (!L.wgu.valid()) miss.push_back(p + "ffn_gate.weight/ffn_up.weight");
    if (!L.wdown.valid()) miss.push_back(p + "ffn_down.weight");
    if (cfg_.qk_norm && (!L.q_norm || !L.k_norm)) miss.push_back(p + "attn_q_norm/attn_k_norm");
  }
  return miss;
}

std::string Engine::weight_type_summary() const {
  std::map<int, size_t> cnt;
  auto add = [&](const QMat& m) { if (m.valid()) cnt[m.w.qtype] += (size_t)m.w.rows * m.w.cols; };
  add(tok_embd_);
  add(output_);
  for (const LayerW& L : layers_) { add(L.wq); add(L.wk); add(L.wv); add(L.wo); add(L.wgu); add(L.wdown); }
  std::ostringstream os;
  for (auto& kv : cnt) os << kv.first << ":" << kv.second << " ";
  return os.str();
}

static std::vector<std::vector<const QMat*>> qkv_groups(const LayerW& L);

void Engine::finalize() {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  TraceRange tr("aios.finalize");
  HIP_CHECK(hipSetDevice(cfg_.device));
  stage_release();  // weights are in place: drop the load-time staging buffers
  auto miss = missing_tensors();
  if (!miss.empty()) throw std::runtime_error("missing tensors, first: " + miss[0]);
  if (!output_.valid()) {
    if (!cfg_.tie_embeddings) cfg_.tie_embeddings = 1;
    cfg_.vocab_parallel = 0;  // the tied table is the full vocabulary
    output_ = tok_embd_;  // tied embeddings (GGUF files without output.weight)
  }
  const int d = cfg_.d_model, hd = cfg_.head_dim, H = cfg_.n_heads, Hkv = cfg_.n_kv_heads;
  const int qd = H * hd, kvd = Hkv * hd, V = cfg_.vocab_size, Bm = cfg_.max_batch;
  if (cfg_.max_ctx % KV_BLOCK) cfg_.max_ctx = (int)align_up(cfg_.max_ctx, KV_BLOCK);  // whole KV blocks
  // paged KV pool: max_slots * max_ctx / KV_BLOCK blocks always suffice (a mapping or
  // un-sharing step never needs more distinct blocks than there are table entries) + one null
  // block that unmapped table entries point to on the device
  kv_maxb_ = cfg_.max_ctx / KV_BLOCK;
  kv_nblocks_ = cfg_.max_slots * kv_maxb_;
  bt_.assign((size_t)cfg_.max_slots * kv_maxb_, -1);
  refcnt_.assign(kv_nblocks_, 0);
  free_blocks_.clear();
  for (int b = kv_nblocks_ - 1; b >= 0; --b) free_blocks_.push_back(b);
  row_bt_host_.assign((size_t)Bm * kv_maxb_, kv_nblocks_);
  layer_kv_elems_ = (size_t)(kv_nblocks_ + 1) * Hkv * KV_BLOCK * hd;
  kv_es_ = cfg_.kv_fp8 ? 1 : 2;  // bytes per cached element (fp8 e4m3 or bf16)
  kv_bytes_ = 2 * layer_kv_elems_ * cfg_.n_layers * kv_es_;
  if (kv_scale_.size() != (size_t)2 * cfg_.n_layers) kv_scale_.assign((size_t)2 * cfg_.n_layers, 1.f);
  k_cache_ = (bf16_t*)dmalloc(kv_bytes_ / 2);
  v_cache_ = (bf16_t*)dmalloc(kv_bytes_ / 2);
  HIP_CHECK(hipMemset(k_cache_, 0, kv_bytes_ / 2));
  HIP_CHECK(hipMemset(v_cache_, 0, kv_bytes_ / 2));
  if (cfg_.kv_fp8) d_kv_amax_ = (unsigned*)dmalloc((size_t)cfg_.n_layers * 2 * Hkv * sizeof(unsigned));
  n_chunks_ = (cfg_.max_ctx + ATTN_CHUNK - 1) / ATTN_CHUNK;
  {
    const size_t nc = (size_t)std::max(prefill_rows_, Bm) * H;  // decode attention tickets [row][head]
    attn_cnt_ = (int*)dmalloc(nc * 4);
    HIP_CHECK(hipMemset(attn_cnt_, 0, nc * 4));
  }
  {
    const int half = hd / 2;
    std::vector<float> tab((size_t)cfg_.max_ctx * half * 2);
    for (int pos = 0; pos < cfg_.max_ctx; ++pos)
      for (int p = 0; p < half; ++p) {
        const double th = (double)pos * std::pow((double)cfg_.rope_theta, -2.0 * p / (double)hd);
        tab[((size_t)pos * half + p) * 2] = (float)std::cos(th);
        tab[((size_t)pos * half + p) * 2 + 1] = (float)std::sin(th);
      }
    rope_cs_ = (float2*)dmalloc(tab.size() * 4);
    HIP_CHECK(hipMemcpy(rope_cs_, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  }

  size_t ws = 0;
  auto fbuf = [&](size_t n) { ws += n * 4; return (float*)dmalloc(n * 4); };
  auto ibuf = [&](size_t n) { ws += n * 4; int* p = (int*)dmalloc(n * 4); HIP_CHECK(hipMemset(p, 0, n * 4)); return p; };
  x_ = fbuf((size_t)Bm * d);
  q_ = fbuf((size_t)Bm * qd);
  qkv_ = fbuf((size_t)Bm * (qd + 2 * kvd));
  attn_ = fbuf((size_t)Bm * std::max(qd, d));
  ff_ = fbuf((size_t)Bm * std::max(cfg_.d_ff, d));
  // (the BF16 engine stages its x as bf16 whatever act_q8 says: the hand-off serves it too)
  if ((cfg_.act_q8 || layers_[0].wgu.w.qtype == QT_BF16) && cfg_.d_ff % 8 == 0 &&
      !(std::getenv("AIOS_FF16") && std::atoi(std::getenv("AIOS_FF16")) == 0)) {
    gv_ff16_ = (bf16_t*)dmalloc((size_t)Bm * cfg_.d_ff * 2);
    ws += (size_t)Bm * cfg_.d_ff * 2;
  }
  opart_ = fbuf((size_t)Bm * H * n_chunks_ * hd);
  ml_ = fbuf((size_t)Bm * H * n_chunks_ * 2);
  logits_ = fbuf((size_t)Bm * V);
  {
    // per-step decode parameters + grammar masks in ONE device block mirrored by a pinned host
    // block: a scheduler decode() uploads all of them with a single async copy (round 1 issued 8
    // pageable copies per step)
    const size_t mb = (size_t)Bm * ((V + 7) / 8);
    par_seeds_off_ = align_up(par_off(PAR_ROWS), 8);  // per-row seeds after the row arrays
    par_mask_off_ = align_up(par_seeds_off_ + (size_t)Bm * 8, 256);
    par_bytes_ = par_mask_off_ + mb;
    d_par_ = (char*)dmalloc(par_bytes_);
    ws += par_bytes_;
    // two halves: the pipelined decode writes step t+1's parameters while step t's copy may still be
    // queued (decode_submit); every upload through the block writes the half the last one did not (next_par)
    HIP_CHECK(hipHostMalloc(&h_par_, 2 * par_bytes_, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&h_mask_, mb, hipHostMallocDefault));
    // logit processors (set_sample_processors): scalars, penalty windows, bias ids and values
    const size_t pb = (size_t)Bm * (4 * 4 + (size_t)SAMPLE_PEN_MAX * 4 + (size_t)SAMPLE_BIAS_MAX * 8);
    HIP_CHECK(hipHostMalloc((void**)&h_proc_, pb, hipHostMallocDefault));
    d_proc_ = (char*)dmalloc(pb);
    ws += pb;
    HIP_CHECK(hipEventCreateWithFlags(&pipe_ev_, hipEventDisableTiming));
    HIP_CHECK(hipHostMalloc((void**)&h_tok_out_, (size_t)Bm * 4, hipHostMallocDefault));
    std::memset(h_par_, 0, 2 * par_bytes_);
    d_seed_ = (uint64_t*)d_par_;
    d_slot_ = (int*)(d_par_ + par_off(PAR_SLOT));
    d_tokens_ = (int*)(d_par_ + par_off(PAR_TOKEN));
    d_pos_ = (int*)(d_par_ + par_off(PAR_POS));
    d_seqlen_ = (int*)(d_par_ + par_off(PAR_SEQLEN));
    d_topk_ = (int*)(d_par_ + par_off(PAR_TOPK));
    d_temp_ = (float*)(d_par_ + par_off(PAR_TEMP));
    d_topp_ = (float*)(d_par_ + par_off(PAR_TOPP));
    d_seeds_ = (uint64_t*)(d_par_ + par_seeds_off_);
    d_mask_ = (uint8_t*)(d_par_ + par_mask_off_);
    float* htp = (float*)(h_par_ + par_off(PAR_TOPP));
    for (int b = 0; b < Bm; ++b) htp[b] = 1.f;
    HIP_CHECK(hipMemcpy(d_par_, h_par_, par_bytes_, hipMemcpyHostToDevice));
  }
  d_bt_ = ibuf((size_t)cfg_.max_slots * kv_maxb_);
  d_row_bt_ = ibuf((size_t)Bm * kv_maxb_);
  {
    std::vector<int> nul((size_t)cfg_.max_slots * kv_maxb_, kv_nblocks_);
    HIP_CHECK(hipMemcpy(d_bt_, nul.data(), nul.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_row_bt_, nul.data(), (size_t)Bm * kv_maxb_ * 4, hipMemcpyHostToDevice));
  }
  attn_bt_ = d_row_bt_;
  attn_bt_rows_ = 1;
  d_step_ = ibuf(4);
  d_step_kv_ = ibuf((size_t)Bm * 2);
  d_step_rope_ = (float2*)fbuf((size_t)Bm * hd);
  d_fpos_ = ibuf(4);
  sample_ws_bytes_ = sample_ws_bytes(Bm, V);
  sample_ws_ = dmalloc(sample_ws_bytes_);
  ws += sample_ws_bytes_;
  sample_cnt_ = ibuf(Bm);
  {
    // per-token logprobs (set_logprobs): slice workspace + tickets, and per row LOGPROB_ROW floats and ids,
    // device block [Bm rows of floats | Bm rows of ids] mirrored by a pinned one ([top_n | floats | ids])
    lp_ws_bytes_ = logprob_ws_bytes(Bm, V);
    lp_ws_ = dmalloc(lp_ws_bytes_);
    ws += lp_ws_bytes_;
    lp_cnt_ = ibuf(Bm);
    d_lp_topn_ = ibuf(Bm);
    const size_t ob = (size_t)Bm * LOGPROB_ROW * 8;
    d_lp_out_ = (char*)dmalloc(ob);
    ws += ob;
    HIP_CHECK(hipHostMalloc((void**)&h_lp_, (size_t)Bm * 4 + ob, hipHostMallocDefault));
  }
  d_history_ = ibuf((size_t)Bm * (cfg_.max_ctx + 1));
  d_spec_ = ibuf(SPEC_MAX_ROWS + SPEC_RECORD);
  HIP_CHECK(hipHostMalloc((void**)&h_spec_, (size_t)(SPEC_MAX_ROWS + SPEC_RECORD) * 4, hipHostMallocDefault));
  const int R = prefill_rows_;
  pf_x_ = fbuf((size_t)R * d);
  pf_q_ = fbuf((size_t)R * qd);
  pf_qkv_ = fbuf((size_t)R * (qd + 2 * kvd));
  pf_attn_ = fbuf((size_t)R * std::max(qd, d));
  pf_ff_ = fbuf((size_t)R * std::max(cfg_.d_ff, d));
  pf_opart_ = fbuf((size_t)R * H * n_chunks_ * hd);
  pf_ml_ = fbuf((size_t)R * H * n_chunks_ * 2);
  pf_a16_ = (bf16_t*)dmalloc((size_t)R * std::max({d, qd, cfg_.d_ff}) * 2);
  pf_tokens_ = ibuf(R);
  pf_pos_ = ibuf(R);
  pf_seqlen_ = ibuf(R);
  pf_slot_ = ibuf(R);
  // GEMM prefill path: supported when every projection is a GEMM format with 64-aligned shapes
  // and the head layout has a flash-attention instantiation
  {
    if (const char* e = std::getenv("AIOS_PREFILL_GEMM_MIN")) gm_min_rows_ = std::max(1, std::atoi(e));
    // one chunk per prompt up to 2048 tokens: the M tile count, not the chunk count, fills the chip
    gm_rows_ = std::min(cfg_.max_ctx, 2048);
    if (const char* e = std::getenv("AIOS_PREFILL_GEMM_ROWS")) gm_rows_ = std::max(64, std::atoi(e));
    bool ok = attn_prefill_supports(H, Hkv, hd) && d % 64 == 0 && cfg_.d_ff % 64 == 0 && qd % 64 == 0 && kvd % 64 == 0;
    for (const auto& L : layers_) {
      for (const QMat* m : {&L.wq, &L.wk, &L.wv, &L.wo, &L.wgu, &L.wdown})
        if (!gemm_supports(m->w.qtype) || m->w.rows % 64 || m->w.cols % 64) ok = false;
    }
    if (const char* e = std::getenv("AIOS_PREFILL_GEMM"))
      if (std::atoi(e) == 0) ok = false;
    gm_ok_ = ok;
    if (ok) {
      const int G = gm_rows_;
      gm_x_ = fbuf((size_t)G * d);
      gm_qkv_ = fbuf((size_t)G * (qd + 2 * kvd));
      gm_q_ = fbuf((size_t)G * qd);
      gm_part_ = fbuf((size_t)G * d);
      gm_a16_ = (bf16_t*)dmalloc((size_t)G * d * 2);
      gm_ff16_ = (bf16_t*)dmalloc((size_t)G * cfg_.d_ff * 2);
      gm_attn16_ = (bf16_t*)dmalloc((size_t)G * qd * 2);
      ws += (size_t)G * (d + cfg_.d_ff + qd) * 2;
      gm_tokens_ = ibuf(G);
      gm_pos_ = ibuf(G);
      gm_slot_ = ibuf(G);
      if (const char* e = std::getenv("AIOS_DECODE_GEMM_MIN_B")) {
        dec_gemm_min_b_ = std::atoi(e);
      } else {
        // B rows go through the B-row LDS-DMA engine only if EVERY projection's LDS plan fits at that
        // B; where one does not (e.g. a 28672-wide down projection at B = 4: 115 KB of staged x), the
        // row-pair fallback is 2-3x slower than the skinny GEMM, so that B takes the GEMM path
        // (ADVICE r3).  Also bounds the short-prompt prefill rows that use the GEMV path.
        for (int b = 2; b < dec_gemm_min_b_ && b <= Bm; ++b) {
          bool ok = true;
          for (int l = 0; l < cfg_.n_layers && ok; ++l) {
            const LayerW& L = layers_[l];
            for (auto& grp : qkv_groups(L)) {
              int n = 0;
              for (auto* m : grp) n += m->w.rows;
              ok = ok && gemv_engine_fits(gemv_args(grp, n, d, b, x_, d, L.attn_norm, q_, n, EPI_STORE, l));
            }
            ok = ok && gemv_engine_fits(gemv_args({&L.wo}, d, qd, b, attn_, qd, nullptr, x_, d, EPI_RESID, l)) &&
                 gemv_engine_fits(gemv_args({&L.wgu}, 2 * cfg_.d_ff, d, b, x_, d, L.ffn_norm, ff_, cfg_.d_ff,
                                            EPI_SWIGLU, l)) &&
                 gemv_engine_fits(gemv_args({&L.wdown}, d, cfg_.d_ff, b, ff_, cfg_.d_ff, nullptr, x_, d, EPI_RESID, l));
          }
          if (!ok) {
            dec_gemm_min_b_ = b;
            gm_min_rows_ = std::min(gm_min_rows_, b);
          }
        }
      }
      // split-K slabs + tickets for every skinny-GEMM call: batched decode (M <= max_batch, the
      // lm_head included) AND prefill chunks of 16-64 tokens (no lm_head) -- sized for the batch
      // only, a 32-token prompt ran its projections unsplit (32 workgroups for N = d_model)
      const int maxN = std::max({qd + 2 * kvd, d, 2 * cfg_.d_ff, V});
      const int maxN_pf = std::max({qd + 2 * kvd, d, 2 * cfg_.d_ff});
      gk_ws_bytes_ = std::max(Bm >= 2 ? gemm_skinny_ws_bytes(std::min(Bm, 64), maxN) : (size_t)0,
                              gemm_skinny_ws_bytes(64, maxN_pf));
      gk_ws_ = (float*)dmalloc(gk_ws_bytes_);
      ws += gk_ws_bytes_;
      gk_cnt_len_ = gemm_skinny_cnt_len(maxN);
      gk_cnt_ = ibuf(gk_cnt_len_);
      if (const char* e = std::getenv("AIOS_GEMM_NORM_FUSE")) nrm_fuse_ = std::atoi(e);
      {  // split-RMSNorm operands of short (<= 64-row) prefill chunks, independent of max_batch
        GemmQArgs p;
        std::memset(&p, 0, sizeof(p));
        p.M = 64; p.N = d; p.K = d; p.nseg = 1; p.seg[0] = layers_[0].wo.w;
        const int parts = gemm_skinny_ntile(p);
        if (nrm_fuse_ && parts > 0 && parts % 4 == 0 && parts <= 64 && d % 128 == 0) {
          const int Gs = std::min(G, 64);
          gm_nparts_ = parts;
          gm_xn16_ = (bf16_t*)dmalloc((size_t)Gs * d * 2);
          gm_npart_ = fbuf((size_t)Gs * parts);
          ws += (size_t)Gs * d * 2;
        }
      }
      if (Bm >= 2) {
        dec_a16_ = (bf16_t*)dmalloc((size_t)Bm * std::max(d, qd) * 2);
        dec_ff16_ = (bf16_t*)dmalloc((size_t)Bm * cfg_.d_ff * 2);
        ws += (size_t)Bm * (std::max(d, qd) + cfg_.d_ff) * 2;
        GemmQArgs p;  // the residual producer's shape (O / down: N = d_model, one segment)
        std::memset(&p, 0, sizeof(p));
        p.M = std::min(Bm, 64); p.N = d; p.K = d; p.nseg = 1; p.seg[0] = layers_[0].wo.w;
        const int parts = gemm_skinny_ntile(p);
        if (nrm_fuse_ && Bm <= 64 && parts > 0 && parts % 4 == 0 && parts <= 64 && d % 128 == 0) {
          nrm_parts_ = parts;
          dec_xn16_ = (bf16_t*)dmalloc((size_t)Bm * d * 2);
          nrm_part_ = fbuf((size_t)Bm * parts);
          ws += (size_t)Bm * d * 2;
        }
        // TP: the all-reduce after O / down writes the next GEMM's split-norm operand itself
        if (cfg_.tp_size > 1 && dec_xn16_ && resid_norm_parts(d) > 0 && resid_norm_parts(d) <= 64) {
          tpn_parts_ = resid_norm_parts(d);
          tpn_part_ = fbuf((size_t)Bm * tpn_parts_);
        }
      }
    }
  }
  ws_bytes_ = ws;
  HIP_CHECK(hipDeviceSynchronize());
  tune_prefill_gemm();
  finalized_ = true;
}

// Measured prefill-GEMM plans (kernels/gemm_pf.hip): every distinct projection launch of this model
// -- QKV stack, O, gate/up (SwiGLU), down, per weight-format signature -- timed over its candidate
// tiles / K splits at M = 64 .. gm_rows_ (powers of two), the fastest kept per M bucket in the
// process-wide plan cache (one tuning per shape per process; ~0.3 s for Mistral-7B).  Activations
// are random bf16 (a zero fill clocks the chip differently).  AIOS_GEMM_PF_TUNE=0: model plans only.
void Engine::tune_prefill_gemm() {
  if (!gm_ok_ || cfg_.n_layers == 0) return;
  if (const char* e = std::getenv("AIOS_GEMM_PF_TUNE"))
    if (std::atoi(e) == 0) return;
  const int d = cfg_.d_model, hd = cfg_.head_dim, qd = cfg_.n_heads * hd, kvd = cfg_.n_kv_heads * hd;
  const int ff = cfg_.d_ff, G = gm_rows_, ldqkv = qd + 2 * kvd;
  const bool tp = cfg_.tp_size > 1;
  const size_t n = (size_t)G * std::max({d, qd, ff});
  float* tmp = nullptr;
  HIP_CHECK(hipMalloc(&tmp, n * 4));
  fill_random_f32(tmp, n, 0x7u, 0.f, 1.f, stream_);
  launch_f32_to_bf16(tmp, gm_a16_, (size_t)G * d, stream_);
  launch_f32_to_bf16(tmp, gm_attn16_, (size_t)G * qd, stream_);
  launch_f32_to_bf16(tmp, gm_ff16_, (size_t)G * ff, stream_);
  std::set<std::string> seen;
  for (int M = 64; M <= G; M *= 2) {
    for (const LayerW& L : layers_) {
      auto tune = [&](GemmQArgs& g, const char* what) {
        std::string sig = std::string(what) + ":" + std::to_string(M);
        for (int s = 0; s < g.nseg; ++s) sig += "," + std::to_string(g.seg[s].qtype);
        if (!seen.insert(sig).second) return;
        gemm_pf_autotune(g, stream_);
      };
      GemmQArgs g;
      std::memset(&g, 0, sizeof(g));
      g.A = gm_a16_; g.lda = d; g.M = M; g.K = d; g.nseg = 3;
      g.seg[0] = L.wq.w; g.seg[1] = L.wk.w; g.seg[2] = L.wv.w;
      g.seg_n0[0] = 0; g.seg_n0[1] = qd; g.seg_n0[2] = qd + kvd;
      g.N = ldqkv; g.C = gm_qkv_; g.ldc = ldqkv; g.epi = GEPI_STORE;
      tune(g, "qkv");
      std::memset(&g, 0, sizeof(g));
      g.A = gm_attn16_; g.lda = qd; g.M = M; g.K = qd; g.nseg = 1; g.seg[0] = L.wo.w; g.N = d; g.ldc = d;
      if (tp) { g.C = gm_part_; g.epi = GEPI_STORE; } else { g.C = gm_x_; g.epi = GEPI_ACCUM; }
      tune(g, "o");
      std::memset(&g, 0, sizeof(g));
      g.A = gm_a16_; g.lda = d; g.M = M; g.K = d; g.nseg = 1; g.seg[0] = L.wgu.w; g.N = 2 * ff;
      g.C16 = gm_ff16_; g.ldc = ff; g.epi = GEPI_SWIGLU_BF16;
      tune(g, "gu");
      std::memset(&g, 0, sizeof(g));
      g.A = gm_ff16_; g.lda = ff; g.M = M; g.K = ff; g.nseg = 1; g.seg[0] = L.wdown.w; g.N = d; g.ldc = d;
      if (tp) { g.C = gm_part_; g.epi = GEPI_STORE; } else { g.C = gm_x_; g.epi = GEPI_ACCUM; }
      tune(g, "down");
    }
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  HIP_CHECK(hipFree(tmp));
}

// TP: sum the row-parallel partials in `p` over the ranks and add the total into `residual`
// (one fused launch: xGMI one-shot all-reduce + residual add, aios_amd/csrc/comm.h)
void Engine::allreduce(float* p, size_t n, float* residual) {
  if (cfg_.tp_size > 1) {
    if (!allreduce_) throw std::runtime_error("tensor-parallel engine without an all-reduce hook");
    allreduce_(allreduce_ctx_, p, n, residual, stream_);
  }
}

// decode GEMV tuning knobs from the environment (read once): AIOS_GEMV_{U,GRID}_{QKV,O,GU,DOWN,LM}
// -- in-situ sweeps of the captured decode step (tools/gemv_knob_sweep.sh); 0 = the launcher's choice
static int gemv_knob(const char* what, const char* kind) {
  static std::map<std::string, int> cache;
  const std::string key = std::string("AIOS_GEMV_") + what + "_" + kind;
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const char* e = std::getenv(key.c_str());
  const int v = e ? std::atoi(e) : 0;
  cache[key] = v;
  return v;
}
static void apply_knobs(GemvArgs& a, const char* kind) {
  a.tune_u = gemv_knob("U", kind);
  a.tune_grid = gemv_knob("GRID", kind);
}

void Engine::gemv(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx,
                  const float* norm_w, float* y, int ldy, int epi, int layer) {
  launch_gemv(gemv_args(segs, N, K, B, x, ldx, norm_w, y, ldy, epi, layer), stream_);
}

GemvArgs Engine::gemv_args(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx,
                           const float* norm_w, float* y, int ldy, int epi, int layer) {
  GemvArgs a = gemv_base(segs, N, K, B, x, ldx, norm_w, y, ldy, epi, layer);
  apply_knobs(a, K == cfg_.d_ff ? "DOWN" : (N == 2 * cfg_.d_ff ? "GU" : (N == cfg_.vocab_size ? "LM" : "O")));
  return a;
}

GemvArgs Engine::gemv_base(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx,
                           const float* norm_w, float* y, int ldy, int epi, int layer) const {
  GemvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.act_q8 = cfg_.act_q8;
  a.nseg = (int)segs.size();
  int row = 0;
  for (int s = 0; s < a.nseg; ++s) {
    a.seg[s] = segs[s]->w;
    a.seg_row0[s] = row;
    row += segs[s]->w.rows;
  }
  a.N = N;
  a.K = K;
  a.B = B;
  a.row_base = 0;
  a.x = x;
  a.ldx = ldx;
  a.norm_w = norm_w;
  a.eps = cfg_.norm_eps;
  a.y = y;
  a.ldy = ldy;
  a.epi = epi;
  if (epi == EPI_QKV) {
    const LayerW& L = layers_[layer];
    a.bias = L.bqkv;
    a.head_dim = cfg_.head_dim;
    a.q_dim = cfg_.n_heads * cfg_.head_dim;
    a.kv_dim = cfg_.n_kv_heads * cfg_.head_dim;
    a.n_kv_heads = cfg_.n_kv_heads;
    a.max_ctx = cfg_.max_ctx;
    a.rope_neox = cfg_.rope_neox;
    a.rope_base = cfg_.rope_theta;
    a.rope_cs = rope_cs_;
    a.k_cache = kv_layer(k_cache_, layer);
    a.v_cache = kv_layer(v_cache_, layer);
    kv_write_args(a, layer);
  }
  return a;
}

// QKV segments: group into launches where only the last segment may differ in format
static std::vector<std::vector<const QMat*>> qkv_groups(const LayerW& L) {
  const QMat* s[3] = {&L.wq, &L.wk, &L.wv};
  if (s[0]->w.qtype == s[1]->w.qtype && gemv_supports(s[0]->w.qtype, s[2]->w.qtype)) return {{s[0], s[1], s[2]}};
  if (s[0]->w.qtype == s[1]->w.qtype) return {{s[0], s[1]}, {s[2]}};
  return {{s[0]}, {s[1]}, {s[2]}};
}

void Engine::gemm(GemmQArgs& g) {
  g.ws = gk_ws_;
  g.ws_bytes = gk_ws_bytes_;
  g.cnt = gk_cnt_;
  g.cnt_len = gk_cnt_len_;
  launch_gemm_q(g, stream_);
}

GemvArgs Engine::qkv_gemv_args(int l, const std::vector<const QMat*>& grp, int row0, int B, const float* x, bool fused,
                               float* q, float* qkv, const int* pos, const int* slot) {
  const int d = cfg_.d_model, qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
  int n = 0;
  for (auto* m : grp) n += m->w.rows;
  GemvArgs a = gemv_base(grp, n, d, B, x, d, layers_[l].attn_norm, fused ? q : qkv, fused ? qd : qd + 2 * kvd,
                         fused ? EPI_QKV : EPI_STORE, l);
  a.row_base = row0;
  if (fused) { a.pos = pos; a.slot = slot; a.block_table = d_bt_; }
  return a;
}

QkvPostArgs Engine::qkv_post_args(int l, const float* qkv, int ldqkv, int T, const int* pos, const int* slot,
                                  float* q_out, const float* bias, unsigned* amax) const {
  const LayerW& L = layers_[l];
  QkvPostArgs p;
  p.qkv = qkv; p.ldqkv = ldqkv; p.T = T;
  p.n_heads = cfg_.n_heads; p.n_kv_heads = cfg_.n_kv_heads; p.head_dim = cfg_.head_dim;
  p.bias = bias; p.q_norm = L.q_norm; p.k_norm = L.k_norm; p.eps = cfg_.norm_eps;
  p.rope_neox = cfg_.rope_neox; p.rope_base = cfg_.rope_theta; p.rope_cs = rope_cs_;
  p.pos = pos; p.slot = slot; p.q_out = q_out;
  p.k_cache = kv_layer(k_cache_, l); p.v_cache = kv_layer(v_cache_, l);
  p.max_ctx = cfg_.max_ctx; p.block_table = d_bt_;
  kv_write_args(p, l);
  p.amax = amax;
  return p;
}

AttnDecodeArgs Engine::attn_decode_args(int l, int B, const float* q, float* out, const int* seq_len, const int* slot,
                                        const int* block_table, int bt_rows, float* o_part, float* ml,
                                        bf16_t* out16) const {
  AttnDecodeArgs a;
  a.split = 0;
  a.q = q; a.k_cache = kv_layer(k_cache_, l); a.v_cache = kv_layer(v_cache_, l);
  kv_read_args(a, l);
  a.seq_len = seq_len; a.slot = slot; a.block_table = block_table; a.bt_rows = bt_rows;
  a.B = B; a.n_heads = cfg_.n_heads; a.n_kv_heads = cfg_.n_kv_heads; a.head_dim = cfg_.head_dim;
  a.max_ctx = cfg_.max_ctx; a.n_chunks = n_chunks_; a.scale = 1.f / std::sqrt((float)cfg_.head_dim);
  a.o_part = o_part; a.ml = ml; a.out = out; a.out16 = out16; a.counters = attn_cnt_;
  return a;
}

GemmQArgs Engine::gemm_args(const bf16_t* A, int lda, int M, int K, const QWeight& w, int N, int ldc, float* C, int epi) {
  GemmQArgs g;
  std::memset(&g, 0, sizeof(g));
  g.A = A; g.lda = lda; g.M = M; g.K = K; g.nseg = 1; g.seg[0] = w; g.N = N; g.C = C; g.ldc = ldc; g.epi = epi;
  return g;
}

GemmQArgs Engine::qkv_gemm_args(int l, const bf16_t* A, int M, float* C) const {
  const LayerW& L = layers_[l];
  const int d = cfg_.d_model, qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
  GemmQArgs g = gemm_args(A, d, M, d, L.wq.w, qd + 2 * kvd, qd + 2 * kvd, C, GEPI_STORE);
  g.nseg = 3; g.seg[1] = L.wk.w; g.seg[2] = L.wv.w;
  g.seg_n0[0] = 0; g.seg_n0[1] = qd; g.seg_n0[2] = qd + kvd;
  return g;
}
void Engine::qkv_gemm_epi(GemmQArgs& g, int l, const int* pos, const int* slot, float* q_out) const {
  g.epi = GEPI_QKV; g.col0 = 0;
  g.head_dim = cfg_.head_dim; g.q_dim = cfg_.n_heads * cfg_.head_dim; g.kv_dim = cfg_.n_kv_heads * cfg_.head_dim;
  g.n_kv_heads = cfg_.n_kv_heads; g.max_ctx = cfg_.max_ctx;
  g.rope_cs = rope_cs_; g.pos = pos; g.slot = slot; g.block_table = d_bt_;
  g.q_out = q_out; g.k_cache = kv_layer(k_cache_, l); g.v_cache = kv_layer(v_cache_, l);
  kv_write_args(g, l);
}

void Engine::nrm_consume(GemmQArgs& g, const SplitNorm& n) const {
  g.A = n.xn16; g.nrm_in = n.part; g.nrm_parts = n.parts; g.nrm_eps = cfg_.norm_eps;
}
void Engine::nrm_produce(GemmQArgs& g, const SplitNorm& n, const float* g_next) {
  g.epi = GEPI_ACCUM_NORM; g.nrm_g = g_next; g.nrm_out16 = n.xn16; g.nrm_part = n.part; g.nrm_parts = n.parts;
}

// one transformer block for the B rows staged in x_ (decode).
// Batched decode (B >= dec_gemm_min_b_): the int8 GEMV's dot work grows with B while the weight
// stream does not, so from two concurrent sequences on the projections go through the skinny
// MFMA GEMM (weights dequantised once per step into MFMA operands, split-K reduced in-launch),
// with explicit RMSNorm -> bf16 and RoPE/KV-write launches in place of the GEMV prologue /
// epilogue fusions.  SwiGLU runs in the gate/up GEMM's epilogue (bf16 out for the down GEMM).
bool Engine::nrm_on(int B) const { return nrm_parts_ > 0 && dec_xn16_ && cfg_.tp_size == 1 && B <= 64; }
// AIOS_TP_NORM_FUSE=0 restores the separate RMSNorm launches after C1 / C2 (A/B and tests)
bool Engine::tpn_on(int B) const {
  static const bool on = !(std::getenv("AIOS_TP_NORM_FUSE") && std::atoi(std::getenv("AIOS_TP_NORM_FUSE")) == 0);
  return on && tpn_parts_ > 0 && allreduce_norm_ && cfg_.tp_size > 1 && B <= 64;
}

void Engine::layer_decode_gemm(int l, int B) {
  const LayerW& L = layers_[l];
  const int d = cfg_.d_model, ff = cfg_.d_ff, qd = cfg_.n_heads * cfg_.head_dim;
  const int ldqkv = qd + 2 * cfg_.n_kv_heads * cfg_.head_dim;
  const bool tp = cfg_.tp_size > 1;
  const bool fn = nrm_on(B);
  const bool tpn = tp && tpn_on(B);  // (fn and tpn are exclusive: fn needs tp_size 1)
  // the split RMSNorm's operands: written by the residual GEMMs, or (TP) by the fused all-reduce (C1 / C2)
  const SplitNorm sn = tpn ? SplitNorm{dec_xn16_, tpn_part_, tpn_parts_} : SplitNorm{dec_xn16_, nrm_part_, nrm_parts_};
  auto tp_reduce = [&](float* part, const float* g_next) {
    if (tpn) allreduce_norm_(allreduce_norm_ctx_, part, B, d, x_, ResidNorm{g_next, dec_xn16_, d, tpn_part_, tpn_parts_},
                             stream_);
    else allreduce(part, (size_t)B * d, x_);
  };
  if (!((fn || tpn) && l > 0)) launch_rmsnorm_bf16(x_, d, L.attn_norm, dec_a16_, d, B, d, cfg_.norm_eps, stream_);
  GemmQArgs g = qkv_gemm_args(l, dec_a16_, B, qkv_);
  if ((fn || tpn) && l > 0) nrm_consume(g, sn);
  // RoPE + q store + KV-cache write in the GEMM epilogue (one launch per layer less) whenever
  // qkv_post would only do that (non-NeoX pairs, no QK-norm, no QKV bias)
  static const int qkv_epi_max_b = [] {
    const char* e = std::getenv("AIOS_GEMM_QKV_EPI_MAX_B");
    return e ? std::atoi(e) : 64;
  }();
  const bool qkv_epi = !cfg_.qk_norm && !cfg_.rope_neox && !L.bqkv && rope_cs_ && B <= qkv_epi_max_b;
  if (qkv_epi) qkv_gemm_epi(g, l, d_pos_, d_slot_, q_);
  gemm(g);
  static const bool attn_out16 = !(std::getenv("AIOS_ATTN_OUT16") && std::atoi(std::getenv("AIOS_ATTN_OUT16")) == 0);
  if (!qkv_epi) launch_qkv_post(qkv_post_args(l, qkv_, ldqkv, B, d_pos_, d_slot_, q_, L.bqkv, nullptr), stream_);
  // (out16: bf16 straight from the attention epilogue, no conversion launch)
  launch_attn_decode(attn_decode_args(l, B, q_, attn_, d_seqlen_, d_slot_, attn_bt_, attn_bt_rows_, opart_, ml_,
                                      attn_out16 ? dec_a16_ : nullptr),
                     stream_);
  if (!attn_out16) launch_f32_to_bf16(attn_, dec_a16_, (size_t)B * qd, stream_);
  g = gemm_args(dec_a16_, qd, B, qd, L.wo.w, d, d, tp ? ff_ : x_, tp ? GEPI_STORE : GEPI_ACCUM);
  if (fn) nrm_produce(g, sn, L.ffn_norm);
  gemm(g);
  if (tp) tp_reduce(ff_, L.ffn_norm);
  if (!fn && !tpn) launch_rmsnorm_bf16(x_, d, L.ffn_norm, dec_a16_, d, B, d, cfg_.norm_eps, stream_);
  g = gemm_args(dec_a16_, d, B, d, L.wgu.w, 2 * ff, ff, nullptr, GEPI_SWIGLU_BF16);
  g.C16 = dec_ff16_;
  if (fn || tpn) nrm_consume(g, sn);
  gemm(g);
  g = gemm_args(dec_ff16_, ff, B, ff, L.wdown.w, d, d, tp ? attn_ : x_, tp ? GEPI_STORE : GEPI_ACCUM);
  // the next consumer: layer l + 1's QKV, or the lm_head after the last layer
  const float* g_next = l + 1 < cfg_.n_layers ? layers_[l + 1].attn_norm : out_norm_;
  if (fn) nrm_produce(g, sn, g_next);
  nrm_lm_ = (fn || tpn) && l + 1 == cfg_.n_layers;
  lm_nrm_ = sn;
  gemm(g);
  if (tp) tp_reduce(attn_, g_next);
}

void Engine::layer_decode(int l, int B) {
  if (dec_a16_ && ((dec_gemm_min_b_ > 0 && B >= dec_gemm_min_b_) || B > 8)) {
    layer_decode_gemm(l, B);
    return;
  }
  if (B > 8) throw std::runtime_error("decode: batches above 8 need the GEMM path (GEMM-capable weights)");
  const LayerW& L = layers_[l];
  const int d = cfg_.d_model, hd = cfg_.head_dim, qd = cfg_.n_heads * hd, kvd = cfg_.n_kv_heads * hd;
  const bool fused_qkv = !cfg_.qk_norm && !cfg_.rope_neox;
  // ---- QKV (+RMSNorm prologue, RoPE + KV-cache epilogue)
  {
    int row0 = 0;
    for (auto& grp : qkv_groups(L)) {
      GemvArgs a = qkv_gemv_args(l, grp, row0, B, x_, fused_qkv, q_, qkv_, d_pos_, d_slot_);
      if (fused_qkv && step_prep_on_ && B == 1) { a.step_kv = d_step_kv_; a.step_rope = d_step_rope_; }
      apply_knobs(a, "QKV");
      static const int qkv_dbg = [] {  // probes only (AIOS_QKV_DBG=0x20000: epilogue lookups skipped)
        const char* e = std::getenv("AIOS_QKV_DBG");
        return e ? (int)std::strtol(e, nullptr, 0) : 0;
      }();
      a.tune_dbg = qkv_dbg;
      launch_gemv(a, stream_);
      row0 += a.N;
    }
    if (!fused_qkv) {
      if (L.bqkv) throw std::runtime_error("qkv bias with unfused QKV path not supported yet");
      launch_qkv_post(qkv_post_args(l, qkv_, qd + 2 * kvd, B, d_pos_, d_slot_, q_, nullptr, nullptr), stream_);
    }
  }
  // ---- attention (fp32 output: a bf16 hand-off to O measured neutral, 544.0-544.5 vs 545.0-545.7 tok/s)
  launch_attn_decode(attn_decode_args(l, B, q_, attn_, d_seqlen_, d_slot_, attn_bt_, attn_bt_rows_, opart_, ml_), stream_);
  // ---- O projection (+ residual; TP: partial -> all-reduce -> add, fused into the GEMV epilogue
  // when the comm provides it)
  {
    const bool tp = cfg_.tp_size > 1;
    if (!(tp && tp_fuse_gemv(gemv_args({&L.wo}, d, qd, B, attn_, qd, nullptr, x_, d, EPI_TP_RESID, l)))) {
      GemvArgs a = gemv_args({&L.wo}, d, qd, B, attn_, qd, nullptr, tp ? ff_ : x_, d, tp ? EPI_STORE : EPI_RESID, l);
      launch_gemv(a, stream_);
      if (tp) allreduce(ff_, (size_t)B * d, x_);
    }
  }
  // ---- gate/up (+RMSNorm, SwiGLU; bf16 out when the down GEMV stages int8 activations, i.e. both
  // matrices take the int8-activation kernels: quantised formats, not F16 / BF16)
  auto q8k = [](int qt) { return qt != QT_F16 && qt != QT_BF16 && qt != QT_F32; };
  bf16_t* ff16 = (gv_ff16_ && q8k(L.wgu.w.qtype) && q8k(L.wdown.w.qtype)) ? gv_ff16_ : nullptr;
  if (gv_ff16_ && L.wgu.w.qtype == QT_BF16 && L.wdown.w.qtype == QT_BF16 &&
      gemv_bf16_engine_fits(gemv_args({&L.wgu}, 2 * cfg_.d_ff, d, B, x_, d, L.ffn_norm, ff_, cfg_.d_ff, EPI_SWIGLU, l)) &&
      gemv_bf16_engine_fits(gemv_args({&L.wdown}, d, cfg_.d_ff, B, ff_, cfg_.d_ff, nullptr, x_, d, EPI_RESID, l)))
    ff16 = gv_ff16_;  // BF16 weights: both GEMVs on the BF16 engine, which reads / writes the bf16 hand-off
  {
    GemvArgs a = gemv_args({&L.wgu}, 2 * cfg_.d_ff, d, B, x_, d, L.ffn_norm, ff_, cfg_.d_ff, EPI_SWIGLU, l);
    a.y16 = ff16;
    launch_gemv(a, stream_);
  }
  // ---- down (+ residual)
  {
    const bool tp = cfg_.tp_size > 1;
    GemvArgs f = gemv_args({&L.wdown}, d, cfg_.d_ff, B, ff_, cfg_.d_ff, nullptr, x_, d, EPI_TP_RESID, l);
    f.x16 = ff16;
    if (!(tp && tp_fuse_gemv(f))) {
      GemvArgs a = gemv_args({&L.wdown}, d, cfg_.d_ff, B, ff_, cfg_.d_ff, nullptr, tp ? attn_ : x_, d,
                             tp ? EPI_STORE : EPI_RESID, l);
      a.x16 = ff16;
      launch_gemv(a, stream_);
      if (tp) allreduce(attn_, (size_t)B * d, x_);
    }
  }
}


// EPI_TP_RESID (the O / down all-reduce in the GEMV epilogue, gemv_q8.h) when the comm provides the
// fused context
bool Engine::tp_fuse_gemv(GemvArgs a) {
  // batch 1 only, through the row-pair kernel (any K; a TP rank's O / down shares sit below the LDS
  // engine's size floor anyway); B = 2..4 keep separate all-reduce launches
  if (!tp_fuse_ || a.B != 1 || !a.act_q8 || a.force_v1 || a.nseg != 1) return false;  // (int8-activation kernel)
  const int qt0 = a.seg[0].qtype;
  if (!(qt0 == QT_Q4_K || qt0 == QT_Q5_K || qt0 == QT_Q6_K || qt0 == QT_Q4_0 || qt0 == QT_Q8_0)) return false;
  a.tp = tp_fuse_;
  a.kernel_sel = 1;
  a.tune_grid = 0;
  a.tune_u = 0;
  a.grid_cap = tp_fuse_grid_;  // ranks sharing a GPU: every rank's workgroups resident together
  // (false: the row-pair kernel did not take it -- stage capacity within grid_cap, LDS plan -- and
  // nothing was launched; the caller runs the plain GEMV + all-reduce)
  return launch_gemv_tp_fused(a, stream_);
}

std::vector<int> Engine::tp_fuse_fits() {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  std::vector<int> out;
  if (!tp_fuse_) return out;
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int d = cfg_.d_model, qd = cfg_.n_heads * cfg_.head_dim;
  for (int l = 0; l < cfg_.n_layers; ++l) {
    const LayerW& L = layers_[l];
    GemvArgs o = gemv_args({&L.wo}, d, qd, 1, attn_, qd, nullptr, x_, d, EPI_TP_RESID, l);
    GemvArgs f = gemv_args({&L.wdown}, d, cfg_.d_ff, 1, ff_, cfg_.d_ff, nullptr, x_, d, EPI_TP_RESID, l);
    o.dry = f.dry = 1;
    out.push_back(tp_fuse_gemv(o) ? 1 : 0);
    out.push_back(tp_fuse_gemv(f) ? 1 : 0);
  }
  return out;
}

// logits_[B][V] = rmsnorm(x) . output^T.  Vocab-parallel TP: this rank holds V/tp rows of
// output.weight, writes its column slice of every logits row, and the xGMI all-gather completes the
// rows on every rank, so the sampler and the grammar mask run identically everywhere -- 1/tp of
// the largest single matrix per GPU instead of a replica (Llama-3 70B: 128256 x 8192 Q6_K).
void Engine::lm_head(int B, const float* x, int ldx) {
  const int d = cfg_.d_model, V = cfg_.vocab_size;
  const bool vp = cfg_.vocab_parallel != 0;
  const int Vl = vp ? V / cfg_.tp_size : V;
  float* y = logits_ + (vp ? (size_t)cfg_.tp_rank * Vl : 0);
  if (dec_a16_ && ((dec_gemm_min_b_ > 0 && B >= dec_gemm_min_b_) || B > 8) && Vl % 64 == 0 &&
      gemm_supports(output_.w.qtype)) {
    const bool fused = nrm_lm_ && x == x_ && ldx == d;  // normalised by the last down GEMM
    nrm_lm_ = false;  // one use: a later lm_head (prefill) normalises for itself
    if (!fused) launch_rmsnorm_bf16(x, ldx, out_norm_, dec_a16_, d, B, d, cfg_.norm_eps, stream_);
    GemmQArgs g = gemm_args(dec_a16_, d, B, d, output_.w, Vl, V, y, GEPI_STORE);
    if (fused) nrm_consume(g, lm_nrm_);
    gemm(g);
  } else {
    gemv({&output_}, Vl, d, B, x, ldx, out_norm_, y, V, EPI_STORE, 0);
  }
  if (vp) {
    if (!allgather_) throw std::runtime_error("vocab-parallel engine without an all-gather hook");
    allgather_(allgather_ctx_, logits_, B, Vl, V, stream_);
  }
}

void Engine::enqueue_decode_step(int B, bool masked) {
  enqueue_decode_forward(B);
  enqueue_sample(B, masked);
}

void Engine::enqueue_decode_forward(int B) {
  const int d = cfg_.d_model;
  {
    StepPrep sp{d_pos_, d_slot_, d_bt_, kv_maxb_, rope_cs_, cfg_.head_dim / 2, d_step_kv_, d_step_rope_};
    launch_get_rows_step(tok_embd_.w, d_tokens_, B, x_, d, 1.f, sp, stream_);
  }
  static const bool step_prep = !(std::getenv("AIOS_STEP_PREP") && std::atoi(std::getenv("AIOS_STEP_PREP")) == 0);
  step_prep_on_ = step_prep && rope_cs_ != nullptr;
  nrm_lm_ = false;
  for (int l = 0; l < cfg_.n_layers; ++l) layer_decode(l, B);
  step_prep_on_ = false;
  lm_head(B, x_, d);
  nrm_lm_ = false;
}

void Engine::set_sample_processors(const std::vector<float>& min_p, const std::vector<float>& repeat_penalty,
                                   const std::vector<float>& presence_penalty,
                                   const std::vector<float>& frequency_penalty,
                                   const std::vector<std::vector<int>>& recent,
                                   const std::vector<std::vector<int>>& bias_ids,
                                   const std::vector<std::vector<float>>& bias_vals) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("set_sample_processors: not available on a tensor-parallel engine");
  const int B = (int)recent.size(), Bm = cfg_.max_batch;
  if (B < 1 || B > Bm) throw std::runtime_error("set_sample_processors: batch out of range");
  if ((int)min_p.size() != B || (int)repeat_penalty.size() != B || (int)presence_penalty.size() != B ||
      (int)frequency_penalty.size() != B)
    throw std::runtime_error("set_sample_processors: size mismatch");
  int stride = 1;
  for (const auto& w : recent) {
    if ((int)w.size() > SAMPLE_PEN_MAX)
      throw std::runtime_error("set_sample_processors: window longer than " + std::to_string(SAMPLE_PEN_MAX));
    for (int t : w)
      if (t < 0 || t >= cfg_.vocab_size) throw std::runtime_error("set_sample_processors: token out of range");
    stride = std::max(stride, (int)w.size());
  }
  int bstride = 0;
  if (!bias_ids.empty() || !bias_vals.empty()) {
    if ((int)bias_ids.size() != B || (int)bias_vals.size() != B)
      throw std::runtime_error("set_sample_processors: size mismatch");
    std::vector<int> seen;
    for (int b = 0; b < B; ++b) {
      const auto& ids = bias_ids[b];
      if (ids.size() != bias_vals[b].size()) throw std::runtime_error("set_sample_processors: size mismatch");
      if ((int)ids.size() > SAMPLE_BIAS_MAX)
        throw std::runtime_error("set_sample_processors: logit bias longer than " + std::to_string(SAMPLE_BIAS_MAX));
      int bans = 0;
      for (size_t j = 0; j < ids.size(); ++j) {
        const float v = bias_vals[b][j];
        if (ids[j] < 0 || ids[j] >= cfg_.vocab_size)
          throw std::runtime_error("set_sample_processors: logit bias token out of range");
        if (std::isnan(v) || (std::isinf(v) && v > 0.f))
          throw std::runtime_error("set_sample_processors: logit bias must be finite or -inf");
        bans += std::isinf(v) ? 1 : 0;
      }
      seen.assign(ids.begin(), ids.end());
      std::sort(seen.begin(), seen.end());
      if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
        throw std::runtime_error("set_sample_processors: duplicate logit bias token");
      if (bans >= cfg_.vocab_size) throw std::runtime_error("set_sample_processors: logit bias bans every token");
      bstride = std::max(bstride, (int)ids.size());
    }
  }
  // (one pinned buffer, h_mask_'s rule: the previous processors' copy ran before the sampler whose
  // token the host already collected -- the caller stages a step's processors from that token)
  float* hf = (float*)h_proc_;
  int* hw = (int*)(h_proc_ + (size_t)Bm * 16);
  for (int b = 0; b < B; ++b) {
    hf[b] = min_p[b]; hf[Bm + b] = repeat_penalty[b]; hf[2 * Bm + b] = presence_penalty[b];
    hf[3 * Bm + b] = frequency_penalty[b];
    for (int j = 0; j < stride; ++j) hw[(size_t)b * stride + j] = j < (int)recent[b].size() ? recent[b][j] : -1;
  }
  int* hb = hw + (size_t)B * stride;
  float* hv = (float*)(hb + (size_t)B * bstride);
  for (int b = 0; b < B && bstride; ++b)
    for (int j = 0; j < bstride; ++j) {
      const bool in = j < (int)bias_ids[b].size();
      hb[(size_t)b * bstride + j] = in ? bias_ids[b][j] : -1;
      hv[(size_t)b * bstride + j] = in ? bias_vals[b][j] : 0.f;
    }
  proc_rows_ = B;
  proc_stride_ = stride;
  proc_bias_stride_ = bstride;
}

void Engine::take_processors(SampleArgs& s, int B) {
  if (!proc_rows_) return;
  const int Bm = cfg_.max_batch;
  proc_rows_ = 0;  // one shot (the caller's SampleStage checked the rows)
  const size_t wbytes = (size_t)Bm * 16 + (size_t)B * proc_stride_ * 4;
  const size_t nbytes = wbytes + (size_t)B * proc_bias_stride_ * 8;
  HIP_CHECK(hipMemcpyAsync(d_proc_, h_proc_, nbytes, hipMemcpyHostToDevice, stream_));
  const float* df = (const float*)d_proc_;
  s.min_p = df; s.repeat_penalty = df + Bm; s.presence_penalty = df + 2 * Bm; s.frequency_penalty = df + 3 * Bm;
  s.pen_tokens = (const int*)(d_proc_ + (size_t)Bm * 16);
  s.pen_stride = proc_stride_;
  if (proc_bias_stride_) {
    s.bias_ids = (const int*)(d_proc_ + wbytes);
    s.bias_vals = (const float*)(s.bias_ids + (size_t)B * proc_bias_stride_);
    s.bias_stride = proc_bias_stride_;
  }
}

void Engine::set_logprobs(const std::vector<int>& top_n) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("set_logprobs: not available on a tensor-parallel engine");
  const int B = (int)top_n.size();
  if (B < 1 || B > cfg_.max_batch) throw std::runtime_error("set_logprobs: batch out of range");
  for (int n : top_n)
    if (n > LOGPROB_MAX_TOP) throw std::runtime_error("set_logprobs: top_n above " + std::to_string(LOGPROB_MAX_TOP));
  // (one pinned buffer, h_proc_'s rule: the previous step's upload ran before the sampler whose token the
  // host already collected)
  int* hn = (int*)h_lp_;
  for (int b = 0; b < B; ++b) hn[b] = top_n[b] < 0 ? -1 : top_n[b];
  lp_rows_ = B;
}

// after a B-row sampler launch: the staged logprob launch over the tokens it wrote and the copy of its
// outputs to pinned memory (valid once the stream reaches the caller's synchronisation point); nothing
// staged: last_logprobs() is empty
void Engine::take_logprobs(int B) {
  lp_last_.clear();
  if (!lp_rows_) return;
  const int Bm = cfg_.max_batch;
  lp_rows_ = 0;  // one shot (the caller's SampleStage checked the rows)
  const int* hn = (const int*)h_lp_;
  HIP_CHECK(hipMemcpyAsync(d_lp_topn_, hn, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  LogprobArgs a;
  std::memset(&a, 0, sizeof(a));
  a.logits = logits_; a.ldl = cfg_.vocab_size; a.B = B; a.V = cfg_.vocab_size;
  a.tokens = d_tokens_; a.top_n = d_lp_topn_;
  a.out_lp = (float*)d_lp_out_; a.out_id = (int*)(d_lp_out_ + (size_t)Bm * LOGPROB_ROW * 4);
  a.ws = lp_ws_; a.ws_bytes = lp_ws_bytes_; a.counters = lp_cnt_;
  launch_logprobs(a, stream_);
  // one copy: every row of floats and the first B rows of ids
  HIP_CHECK(hipMemcpyAsync(h_lp_ + (size_t)Bm * 4, d_lp_out_, (size_t)(Bm + B) * LOGPROB_ROW * 4, hipMemcpyDeviceToHost,
                           stream_));
  lp_last_.assign(hn, hn + B);
}

Engine::Logprobs Engine::last_logprobs() const {
  Logprobs r;
  const int B = (int)lp_last_.size(), Bm = cfg_.max_batch;
  if (!B) return r;
  const float* hl = (const float*)(h_lp_ + (size_t)Bm * 4);
  const int* hi = (const int*)(hl + (size_t)Bm * LOGPROB_ROW);
  r.top_n = lp_last_;
  r.token_lp.assign(B, std::numeric_limits<float>::quiet_NaN());
  r.ids.assign((size_t)B * LOGPROB_MAX_TOP, -1);
  r.lps.assign((size_t)B * LOGPROB_MAX_TOP, -std::numeric_limits<float>::infinity());
  for (int b = 0; b < B; ++b) {
    if (lp_last_[b] < 0) continue;  // row off: the kernel wrote nothing
    r.token_lp[b] = hl[(size_t)b * LOGPROB_ROW];
    std::copy(hi + (size_t)b * LOGPROB_ROW + 1, hi + (size_t)(b + 1) * LOGPROB_ROW, r.ids.begin() + (size_t)b * LOGPROB_MAX_TOP);
    std::copy(hl + (size_t)b * LOGPROB_ROW + 1, hl + (size_t)(b + 1) * LOGPROB_ROW, r.lps.begin() + (size_t)b * LOGPROB_MAX_TOP);
  }
  return r;
}

// ---- DFA grammars ------------------------------------------------------------------------------
void Engine::grammar_vocab(const std::vector<std::string>& tokens, const std::vector<int>& eos_ids) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("grammar_vocab: not available on a tensor-parallel engine");
  const int V = cfg_.vocab_size;
  if ((int)tokens.size() != V) throw std::runtime_error("grammar_vocab: " + std::to_string(V) + " tokens expected");
  if ((int)eos_ids.size() > GRAMMAR_MAX_EOS)
    throw std::runtime_error("grammar_vocab: more than " + std::to_string(GRAMMAR_MAX_EOS) + " end-of-sequence ids");
  for (int e : eos_ids)
    if (e < 0 || e >= V) throw std::runtime_error("grammar_vocab: end-of-sequence id out of range");
  std::vector<int> off(V + 1, 0);
  size_t total = 0;
  for (int t = 0; t < V; ++t) {
    total += tokens[t].size();
    if (total > (size_t)INT32_MAX) throw std::runtime_error("grammar_vocab: vocabulary bytes overflow");
    off[t + 1] = (int)total;
  }
  std::vector<uint8_t> bytes(std::max<size_t>(total, 1), 0);
  for (int t = 0; t < V; ++t) std::memcpy(bytes.data() + off[t], tokens[t].data(), tokens[t].size());
  HIP_CHECK(hipSetDevice(cfg_.device));
  HIP_CHECK(hipStreamSynchronize(stream_));  // (a launch reading the old table may be queued)
  if (!d_grammars_) {
    const int Bm = cfg_.max_batch;
    grammars_.assign(GRAMMAR_MAX, GrammarSlot{});
    d_grammars_ = (GrammarTable*)dmalloc(sizeof(GrammarTable) * GRAMMAR_MAX);
    HIP_CHECK(hipMemset(d_grammars_, 0, sizeof(GrammarTable) * GRAMMAR_MAX));
    d_gr_ = (int*)dmalloc((size_t)2 * Bm * 4);
    d_tok_off_ = (int*)dmalloc((size_t)(V + 1) * 4);
    HIP_CHECK(hipHostMalloc((void**)&h_gr_, (size_t)4 * Bm * 4, hipHostMallocDefault));
  }
  if (d_tok_bytes_) HIP_CHECK(hipFree(d_tok_bytes_));
  d_tok_bytes_ = nullptr;
  HIP_CHECK(hipMalloc((void**)&d_tok_bytes_, bytes.size()));
  HIP_CHECK(hipMemcpy(d_tok_bytes_, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_tok_off_, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  gr_n_eos_ = (int)eos_ids.size();
  for (int j = 0; j < GRAMMAR_MAX_EOS; ++j) gr_eos_[j] = j < gr_n_eos_ ? eos_ids[j] : -1;
}

int Engine::grammars_loaded() const {
  int n = 0;
  for (const auto& g : grammars_) n += g.buf != nullptr;
  return n;
}

GrammarMaskArgs Engine::grammar_args(int B, const int* gid, const int* state, uint8_t* mask, bool fill_free) const {
  GrammarMaskArgs a;
  std::memset(&a, 0, sizeof(a));
  a.tok_off = d_tok_off_; a.tok_bytes = d_tok_bytes_; a.V = cfg_.vocab_size;
  a.grammars = d_grammars_; a.n_grammars = GRAMMAR_MAX;
  a.gid = gid; a.state = state; a.mask = mask; a.B = B;
  a.fill_free = fill_free ? 1 : 0;
  for (int j = 0; j < GRAMMAR_MAX_EOS; ++j) a.eos[j] = gr_eos_[j];
  a.n_eos = gr_n_eos_;
  return a;
}

int Engine::grammar_load(const uint8_t* byte_class, const uint16_t* trans, const uint8_t* accept, int n_states,
                         int n_classes) {
  if (!d_tok_bytes_) throw std::runtime_error("grammar_load: no vocabulary (grammar_vocab first)");
  const int S = n_states, C = n_classes;
  if (S < 2 || S > 65535 || C < 1 || C > 256) throw std::runtime_error("grammar_load: table shape out of range");
  for (int c = 0; c < 256; ++c)
    if (byte_class[c] >= C) throw std::runtime_error("grammar_load: byte class out of range");
  for (size_t i = 0; i < (size_t)S * C; ++i) {
    if (trans[i] >= S) throw std::runtime_error("grammar_load: transition out of range");
    if (i < (size_t)C && trans[i] != 0) throw std::runtime_error("grammar_load: the dead state 0 has a way out");
  }
  int gid = -1;
  for (int i = 0; i < GRAMMAR_MAX && gid < 0; ++i)
    if (!grammars_[i].buf) gid = i;
  if (gid < 0) throw std::runtime_error("grammar_load: " + std::to_string(GRAMMAR_MAX) + " grammars already loaded");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t t_off = 256, a_off = t_off + (size_t)S * C * 2;
  std::vector<uint8_t> host(a_off + S);
  std::memcpy(host.data(), byte_class, 256);
  std::memcpy(host.data() + t_off, trans, (size_t)S * C * 2);
  std::memcpy(host.data() + a_off, accept, S);
  GrammarSlot& g = grammars_[gid];
  HIP_CHECK(hipMalloc(&g.buf, host.size()));
  g.n_states = S;
  g.n_classes = C;
  const char* base = (const char*)g.buf;
  const GrammarTable tab{(const uint8_t*)base, (const uint16_t*)(base + t_off), (const uint8_t*)(base + a_off), S, C};
  try {
    HIP_CHECK(hipMemcpy(g.buf, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_grammars_ + gid, &tab, sizeof(tab), hipMemcpyHostToDevice));
    // every live state that is not terminal must allow a token
    std::vector<int> states;
    for (int s = 1; s < S; ++s) {
      bool way_on = false;
      for (int c = 0; c < C && !way_on; ++c) way_on = trans[(size_t)s * C + c] != 0;
      if (way_on || !accept[s]) states.push_back(s);
    }
    const size_t nb = (size_t)((cfg_.vocab_size + 7) / 8);
    for (size_t i0 = 0; i0 < states.size(); i0 += GRAMMAR_MASK_ROWS) {
      const size_t n = std::min(states.size() - i0, (size_t)GRAMMAR_MASK_ROWS);
      const std::vector<uint8_t> m = grammar_masks(gid, std::vector<int>(states.begin() + i0, states.begin() + i0 + n));
      for (size_t r = 0; r < n; ++r) {
        bool any = false;
        for (size_t j = 0; j < nb && !any; ++j) any = m[r * nb + j] != 0;
        if (!any)
          throw std::runtime_error("grammar_load: state " + std::to_string(states[i0 + r]) +
                                   " allows no token of this vocabulary");
      }
    }
  } catch (...) {
    // (the descriptor first, as grammar_free does: nothing on the device names the freed buffer)
    const GrammarTable none{nullptr, nullptr, nullptr, 0, 0};
    hipStreamSynchronize(stream_);
    hipMemcpy(d_grammars_ + gid, &none, sizeof(none), hipMemcpyHostToDevice);
    hipFree(g.buf);
    g = GrammarSlot{};
    throw;
  }
  return gid;
}

void Engine::grammar_free(int gid) {
  if (gid < 0 || gid >= (int)grammars_.size() || !grammars_[gid].buf) throw std::runtime_error("grammar_free: unknown grammar");
  HIP_CHECK(hipSetDevice(cfg_.device));
  HIP_CHECK(hipStreamSynchronize(stream_));  // (a launch reading the tables may be queued)
  const GrammarTable none{nullptr, nullptr, nullptr, 0, 0};
  HIP_CHECK(hipMemcpy(d_grammars_ + gid, &none, sizeof(none), hipMemcpyHostToDevice));
  HIP_CHECK(hipFree(grammars_[gid].buf));
  grammars_[gid] = GrammarSlot{};
}

std::vector<uint8_t> Engine::grammar_masks(int gid, const std::vector<int>& states) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (gid < 0 || gid >= (int)grammars_.size() || !grammars_[gid].buf) throw std::runtime_error("grammar_masks: unknown grammar");
  for (int s : states)
    if (s < 0 || s >= grammars_[gid].n_states) throw std::runtime_error("grammar_masks: state out of range");
  const size_t n = states.size(), nb = (size_t)((cfg_.vocab_size + 7) / 8);
  std::vector<uint8_t> out(n * nb);
  if (!n) return out;
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t rows = std::min(n, (size_t)GRAMMAR_MASK_ROWS);
  char* dev = nullptr;  // [rows] gid | [rows] state | [rows][nb] masks
  HIP_CHECK(hipMalloc((void**)&dev, rows * 8 + rows * nb));
  try {
    std::vector<int> rs(2 * rows);
    for (size_t i0 = 0; i0 < n; i0 += rows) {
      const size_t k = std::min(rows, n - i0);
      for (size_t r = 0; r < k; ++r) {
        rs[r] = gid;
        rs[rows + r] = states[i0 + r];
      }
      HIP_CHECK(hipMemcpyAsync(dev, rs.data(), rows * 8, hipMemcpyHostToDevice, stream_));
      launch_grammar_mask(grammar_args((int)k, (const int*)dev, (const int*)dev + rows, (uint8_t*)dev + rows * 8, true),
                          stream_);
      HIP_CHECK(hipMemcpyAsync(out.data() + i0 * nb, dev + rows * 8, k * nb, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
  } catch (...) {
    hipFree(dev);
    throw;
  }
  HIP_CHECK(hipFree(dev));
  return out;
}

void Engine::set_grammar_rows(const std::vector<int>& gids, const std::vector<int>& states) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (!d_tok_bytes_) throw std::runtime_error("set_grammar_rows: no vocabulary (grammar_vocab first)");
  const int B = (int)gids.size(), Bm = cfg_.max_batch;
  if (B < 1 || B > Bm) throw std::runtime_error("set_grammar_rows: batch out of range");
  if ((int)states.size() != B) throw std::runtime_error("set_grammar_rows: size mismatch");
  for (int b = 0; b < B; ++b) {
    if (gids[b] < 0) continue;
    if (gids[b] >= (int)grammars_.size() || !grammars_[gids[b]].buf)
      throw std::runtime_error("set_grammar_rows: unknown grammar");
    if (states[b] < 1 || states[b] >= grammars_[gids[b]].n_states)
      throw std::runtime_error("set_grammar_rows: state out of range");
  }
  gr_buf_ ^= 1;
  int* h = h_gr_ + (size_t)gr_buf_ * 2 * Bm;
  for (int b = 0; b < B; ++b) {
    h[b] = gids[b] < 0 ? -1 : gids[b];
    h[Bm + b] = gids[b] < 0 ? 0 : states[b];
  }
  gr_rows_ = B;
}

bool Engine::take_grammar(int B, bool host_mask) {
  if (!gr_rows_) return false;
  gr_rows_ = 0;  // one shot (the caller's SampleStage checked the rows)
  const int Bm = cfg_.max_batch;
  HIP_CHECK(hipMemcpyAsync(d_gr_, h_gr_ + (size_t)gr_buf_ * 2 * Bm, (size_t)2 * Bm * 4, hipMemcpyHostToDevice, stream_));
  launch_grammar_mask(grammar_args(B, d_gr_, d_gr_ + Bm, d_mask_, !host_mask), stream_);
  return true;
}

SampleArgs Engine::sample_args(int B, bool masked) const {
  SampleArgs s;
  std::memset(&s, 0, sizeof(s));
  s.logits = logits_; s.ldl = cfg_.vocab_size; s.B = B; s.V = cfg_.vocab_size;
  s.temperature = d_temp_; s.top_k = d_topk_; s.top_p = d_topp_; s.seeds = d_seeds_;
  s.tokens = d_tokens_;
  s.mask = masked ? d_mask_ : nullptr;
  s.ws = sample_ws_; s.ws_bytes = sample_ws_bytes_; s.counters = sample_cnt_;
  return s;
}

void Engine::enqueue_sample(int B, bool masked, SampleKind kind, bool staged) {
  SampleArgs s = sample_args(B, masked);
  // FIRST: no seed_dev, the key is the row seed and pos alone; AGAIN: pos was advanced by the step, so the RNG
  // key differs from the first sample's
  if (kind != SAMPLE_FIRST) s.seed_dev = d_seed_;
  s.pos = kind == SAMPLE_FIRST ? d_fpos_ : d_pos_;
  if (kind == SAMPLE_STEP) {
    s.seq_len = d_seqlen_;
    s.history = d_history_; s.hist_stride = cfg_.max_ctx + 1;
    s.advance = 1;
  }
  if (staged) take_processors(s, B);
  launch_sample(s, stream_);
  if (staged) take_logprobs(B);
}

bool Engine::gemm_prefill_ok(int T) const { return gm_ok_ && T >= gm_min_rows_; }

// Prefill through the matrix cores: per chunk of <= gm_rows_ tokens and per layer
//   RMSNorm -> bf16 | QKV GEMM (Q4_K/Q6_K dequant fused, one launch per format run) | RoPE + KV
//   write | causal flash attention (MFMA) -> bf16 | O GEMM (+= residual) | RMSNorm -> bf16 |
//   gate/up GEMM with the SwiGLU epilogue -> bf16 | down GEMM (+= residual)
// so every weight byte is dequantised once per chunk (not once per 8 rows as on the GEMV path).
// TP: the row-parallel O / down outputs go through the all-reduce hook into the residual.
void Engine::prefill_gemm(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits,
                          const ChunkHook& hook) {
  TraceRange tr("aios.prefill_gemm");
  const int T = (int)tokens.size();
  const int d = cfg_.d_model, hd = cfg_.head_dim, H = cfg_.n_heads, Hkv = cfg_.n_kv_heads, ff = cfg_.d_ff;
  const int qd = H * hd, ldqkv = qd + 2 * Hkv * hd;
  const bool tp = cfg_.tp_size > 1;
  const SplitNorm sn{gm_xn16_, gm_npart_, gm_nparts_};  // (as in layer_decode_gemm, on a short chunk's rows)
  std::vector<int> hp(gm_rows_), hs(gm_rows_, slot);
  // short chunks (n <= max_batch, the batched-decode GEMMs' shapes): the decode step's fusions --
  // RoPE + KV write in the QKV GEMM's epilogue and the split RMSNorm (the residual GEMMs write
  // bf16(x * g_next) + per-tile sums, the next GEMM scales its rows) -- 3 launches per layer fewer
  static const bool short_fuse = !(std::getenv("AIOS_PREFILL_SHORT_FUSE") && std::atoi(std::getenv("AIOS_PREFILL_SHORT_FUSE")) == 0);
  for (int r0 = 0; r0 < T; r0 += gm_rows_) {
    const int n = std::min(gm_rows_, T - r0);
    // (the fused epilogues are the ring GEMM's: chunks of <= 32 rows; longer chunks take the prefill
    // GEMM, kernels/gemm_pf.hip, with the plain epilogues)
    const bool sh = short_fuse && !tp && n <= 32;
    const bool fnp = sh && gm_nparts_ > 0;
    // The prefill GEMM's split-K and stream-K plans add their partial tiles with fp32 atomics, in arrival
    // order, so two prefills of one prompt differ in the low bits (up to 9e-05 on the pooled unit vector
    // of a bf16 model).  A deterministic call's chunks that reach it (more than 32 rows) ask for its best
    // plan without them (ksplit < 0), so the same tokens pool to the same bytes; prefill() keeps its plans.
    const bool no_split = hook.deterministic && n > 32;
    auto run = [&](GemmQArgs& g) {
      if (no_split) g.ksplit = -1;
      gemm(g);
    };
    for (int i = 0; i < n; ++i) hp[i] = start_pos + r0 + i;
    HIP_CHECK(hipMemcpyAsync(gm_tokens_, tokens.data() + r0, n * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(gm_pos_, hp.data(), n * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(gm_slot_, hs.data(), n * 4, hipMemcpyHostToDevice, stream_));
    launch_get_rows(tok_embd_.w, gm_tokens_, n, gm_x_, d, 1.f, stream_);
    for (int l = 0; l < cfg_.n_layers; ++l) {
      const LayerW& L = layers_[l];
      if (!(fnp && l > 0)) launch_rmsnorm_bf16(gm_x_, d, L.attn_norm, gm_a16_, d, n, d, cfg_.norm_eps, stream_);
      GemmQArgs g = qkv_gemm_args(l, gm_a16_, n, gm_qkv_);
      if (fnp && l > 0) nrm_consume(g, sn);
      // the RoPE / KV-cache epilogue: short chunks (ring / skinny GEMMs); the prefill GEMM's chunks
      // (>= 33 rows) only with AIOS_PREFILL_QKV_EPI=1 -- it needs S = 1 plans, and at 2048 tokens
      // the QKV GEMM then took 212.7 us against 115.7 (split-K) + 32 us of qkv_post (64 tokens:
      // 5.77 vs 4.6 ms per prompt), profiles/prefill_r5.txt
      // (calibration: K / V go through qkv_post, where the observer sits)
      const bool qepi_ok = !cfg_.qk_norm && !cfg_.rope_neox && !L.bqkv && rope_cs_ && !tp && !kv_obs_;
      bool qepi = false;
      if (qepi_ok) {
        GemmQArgs q = g;
        qkv_gemm_epi(q, l, gm_pos_, gm_slot_, gm_q_);
        static const int pf_qkv = [] { const char* e = std::getenv("AIOS_PREFILL_QKV_EPI"); return e ? std::atoi(e) : 0; }();
        qepi = sh || (pf_qkv && gemm_pf_serves(q));
        if (qepi) g = q;
      }
      run(g);
      if (!qepi)
        launch_qkv_post(qkv_post_args(l, gm_qkv_, ldqkv, n, gm_pos_, gm_slot_, gm_q_, L.bqkv, kv_obs_table(l)), stream_);
      AttnPrefillArgs at;
      at.q = gm_q_; at.k_cache = kv_layer(k_cache_, l); at.v_cache = kv_layer(v_cache_, l); at.block_table = d_bt_;
      kv_read_args(at, l);
      at.slot = slot; at.start = start_pos + r0; at.T = n;
      at.n_heads = H; at.n_kv_heads = Hkv; at.head_dim = hd; at.max_ctx = cfg_.max_ctx;
      at.scale = 1.f / std::sqrt((float)hd);
      at.out = gm_attn16_; at.ldo = qd;
      launch_attn_prefill(at, stream_);
      // O projection (+ residual)
      g = gemm_args(gm_attn16_, qd, n, qd, L.wo.w, d, d, tp ? gm_part_ : gm_x_, tp ? GEPI_STORE : GEPI_ACCUM);
      if (fnp) nrm_produce(g, sn, L.ffn_norm);
      run(g);
      if (tp) allreduce(gm_part_, (size_t)n * d, gm_x_);
      // FFN
      if (!fnp) launch_rmsnorm_bf16(gm_x_, d, L.ffn_norm, gm_a16_, d, n, d, cfg_.norm_eps, stream_);
      g = gemm_args(gm_a16_, d, n, d, L.wgu.w, 2 * ff, ff, nullptr, GEPI_SWIGLU_BF16);
      g.C16 = gm_ff16_;
      if (fnp) nrm_consume(g, sn);
      run(g);
      g = gemm_args(gm_ff16_, ff, n, ff, L.wdown.w, d, d, tp ? gm_part_ : gm_x_, tp ? GEPI_STORE : GEPI_ACCUM);
      if (fnp && l + 1 < cfg_.n_layers) nrm_produce(g, sn, layers_[l + 1].attn_norm);  // (lm_head normalises its row)
      run(g);
      if (tp) allreduce(gm_part_, (size_t)n * d, gm_x_);
    }
    if (r0 + n == T && want_logits) lm_head(1, gm_x_ + (size_t)(n - 1) * d, d);
    if (hook.fn) hook.fn(gm_x_, n, r0, r0 + n == T);
  }
}

// Prefill through the GEMVs: chunks of prefill_rows_ rows, per layer the projections in sub-batches of <= 8
// rows and the decode attention once over the chunk's rows (causal by per-row seq_len).  Works on the pf_*
// buffers through local pointers: the decode workspace (x_, q_, ..., d_pos_) is neither read nor written.
// The decode step's extras stay off here: no QKV knobs / step-prep lookups, no bf16 SwiGLU hand-off, no
// fused TP all-reduce epilogue.
void Engine::prefill_gemv(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits,
                          const ChunkHook& hook) {
  const int T = (int)tokens.size(), R = prefill_rows_;
  const int d = cfg_.d_model, ff = cfg_.d_ff, qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
  const int ldqkv = qd + 2 * kvd;
  const bool tp = cfg_.tp_size > 1;
  // (calibration: EPI_STORE + qkv_post, where the observer sits)
  const bool fused_qkv = !cfg_.qk_norm && !cfg_.rope_neox && !kv_obs_;
  std::vector<int> hp(R), hs(R, slot), hsl(R);
  for (int r0 = 0; r0 < T; r0 += R) {
    const int n = std::min(R, T - r0);
    for (int i = 0; i < n; ++i) { hp[i] = start_pos + r0 + i; hsl[i] = hp[i] + 1; }
    HIP_CHECK(hipMemcpyAsync(pf_tokens_, tokens.data() + r0, n * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(pf_pos_, hp.data(), n * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(pf_seqlen_, hsl.data(), n * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(pf_slot_, hs.data(), n * 4, hipMemcpyHostToDevice, stream_));
    launch_get_rows(tok_embd_.w, pf_tokens_, n, pf_x_, d, 1.f, stream_);
    for (int l = 0; l < cfg_.n_layers; ++l) {
      const LayerW& L = layers_[l];
      // every projection: sub-batches of <= 8 rows, rows [o, o + bn) of the chunk
      auto each_sub = [&](auto&& body) {
        for (int o = 0; o < n; o += 8) body(o, std::min(8, n - o));
      };
      each_sub([&](int o, int bn) {
        float *x = pf_x_ + (size_t)o * d, *q = pf_q_ + (size_t)o * qd, *qkv = pf_qkv_ + (size_t)o * ldqkv;
        const int *pos = pf_pos_ + o, *slt = pf_slot_ + o;
        int row0 = 0;
        for (auto& grp : qkv_groups(L)) {
          const GemvArgs a = qkv_gemv_args(l, grp, row0, bn, x, fused_qkv, q, qkv, pos, slt);
          launch_gemv(a, stream_);
          row0 += a.N;
        }
        // (bias and observer only while calibrating, in place of the fused epilogue's bias)
        if (!fused_qkv)
          launch_qkv_post(qkv_post_args(l, qkv, ldqkv, bn, pos, slt, q, kv_obs_ ? L.bqkv : nullptr, kv_obs_table(l)),
                          stream_);
      });
      // attention for all n rows: one slot, the slot-indexed table
      launch_attn_decode(attn_decode_args(l, n, pf_q_, pf_attn_, pf_seqlen_, pf_slot_, d_bt_, 0, pf_opart_, pf_ml_),
                         stream_);
      // O (+ residual; TP: partials into pf_ff_, all-reduced into the residual)
      each_sub([&](int o, int bn) {
        gemv({&L.wo}, d, qd, bn, pf_attn_ + (size_t)o * qd, qd, nullptr, (tp ? pf_ff_ : pf_x_) + (size_t)o * d, d,
             tp ? EPI_STORE : EPI_RESID, l);
      });
      if (tp) allreduce(pf_ff_, (size_t)n * d, pf_x_);
      each_sub([&](int o, int bn) {
        gemv({&L.wgu}, 2 * ff, d, bn, pf_x_ + (size_t)o * d, d, L.ffn_norm, pf_ff_ + (size_t)o * ff, ff, EPI_SWIGLU, l);
      });
      // down (+ residual; TP: partials into pf_attn_)
      each_sub([&](int o, int bn) {
        gemv({&L.wdown}, d, ff, bn, pf_ff_ + (size_t)o * ff, ff, nullptr, (tp ? pf_attn_ : pf_x_) + (size_t)o * d, d,
             tp ? EPI_STORE : EPI_RESID, l);
      });
      if (tp) allreduce(pf_attn_, (size_t)n * d, pf_x_);
    }
    // (lm_head normalises the row itself: x is not x_, and nrm_lm_ is false outside a decode step)
    if (r0 + n == T && want_logits) lm_head(1, pf_x_ + (size_t)(n - 1) * d, d);
    if (hook.fn) hook.fn(pf_x_, n, r0, r0 + n == T);
  }
}

std::vector<float> Engine::prefill(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits) {
  return prefill_run(slot, tokens, start_pos, want_logits, ChunkHook{});
}

std::vector<float> Engine::prefill_run(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits,
                                       const ChunkHook& hook) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  TraceRange tr("aios.prefill");
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int T = (int)tokens.size();
  if (T == 0) throw std::runtime_error("prefill: empty prompt");
  if (start_pos + T > cfg_.max_ctx) throw std::runtime_error("prefill: context overflow");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("prefill: bad slot");
  for (int t : tokens)
    if (t < 0 || t >= cfg_.vocab_size) throw std::runtime_error("prefill: token id out of range");
  kv_prepare_write(slot, start_pos, start_pos + T);
  kv_sync(0);
  if (gemm_prefill_ok(T)) prefill_gemm(slot, tokens, start_pos, want_logits, hook);
  else prefill_gemv(slot, tokens, start_pos, want_logits, hook);
  std::vector<float> out;
  if (want_logits) {
    out.resize(cfg_.vocab_size);
    HIP_CHECK(hipMemcpyAsync(out.data(), logits_, (size_t)cfg_.vocab_size * 4, hipMemcpyDeviceToHost, stream_));
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

// ---- text embeddings (engine.h embed_prefill) -----------------------------------------------------
void Engine::embed_buffers(bool rows) {
  // First use, not finalize: an engine that never embeds allocates what it always did.  All or nothing:
  // the members are set only once every allocation of a group succeeded (a failed dmalloc throws; what it
  // got before stays in allocs_ and is freed with the engine).
  const size_t d = cfg_.d_model;
  if (!emb_acc_) {
    float* acc = (float*)dmalloc((size_t)cfg_.max_slots * d * 4);
    float* out = (float*)dmalloc(d * 4);
    float* ws = (float*)dmalloc(embed_pool_ws_bytes((int)d));
    int* count = (int*)dmalloc((size_t)cfg_.max_slots * 4);
    int* cnt = (int*)dmalloc(4);
    HIP_CHECK(hipMemset(count, 0, (size_t)cfg_.max_slots * 4));
    HIP_CHECK(hipMemset(cnt, 0, 4));
    HIP_CHECK(hipStreamSynchronize(nullptr));  // (the memsets ran on the null stream, the kernel runs on ours)
    emb_pos_.assign(cfg_.max_slots, -1);
    emb_mode_.assign(cfg_.max_slots, -1);
    emb_out_ = out; emb_ws_ = ws; emb_count_ = count; emb_cnt_ = cnt;
    emb_acc_ = acc;
    ws_bytes_ += ((size_t)cfg_.max_slots * d + d) * 4 + embed_pool_ws_bytes((int)d) + (size_t)cfg_.max_slots * 4 + 4;
  }
  if (rows && !emb_rows_) {  // max_ctx x d floats, by the first EMBED_NONE call only
    emb_rows_ = (float*)dmalloc((size_t)cfg_.max_ctx * d * 4);
    ws_bytes_ += (size_t)cfg_.max_ctx * d * 4;
  }
}

void Engine::embed_fold(const EmbedFold& f, const float* x, int n, int pos0, bool last) {
  if (f.pooling == EMBED_LAST && !(f.final && last)) return;  // only the prompt's last row counts
  EmbedPoolArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = x; a.ldx = cfg_.d_model; a.n = n; a.d = cfg_.d_model;
  a.g = out_norm_; a.eps = cfg_.norm_eps;
  a.acc = emb_acc_ + (size_t)f.slot * cfg_.d_model; a.count = emb_count_ + f.slot;
  a.mode = f.pooling; a.first = pos0 == 0; a.final = f.final && last;
  a.out = f.pooling == EMBED_NONE ? emb_rows_ + (size_t)pos0 * cfg_.d_model : emb_out_;
  a.ws = emb_ws_; a.ws_bytes = embed_pool_ws_bytes(cfg_.d_model); a.counter = emb_cnt_;
  launch_embed_pool(a, stream_);
}

std::vector<float> Engine::embed_prefill(int slot, const std::vector<int>& tokens, int start_pos, int pooling,
                                         bool final) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("embeddings: single-GPU engines only");
  if (pooling != EMBED_NONE && pooling != EMBED_MEAN && pooling != EMBED_LAST)
    throw std::runtime_error("embed_prefill: pooling must be 0 (none), 1 (mean) or 3 (last)");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("embed_prefill: bad slot");
  if (start_pos < 0) throw std::runtime_error("embed_prefill: bad start_pos");
  const int d = cfg_.d_model, T = (int)tokens.size();
  if (d % 64 || d > EMBED_MAX_D) throw std::runtime_error("embeddings: d_model must be a multiple of 64 up to 8192");
  HIP_CHECK(hipSetDevice(cfg_.device));
  embed_buffers(pooling == EMBED_NONE);
  if (pooling != EMBED_LAST && start_pos != 0 && (emb_pos_[slot] != start_pos || emb_mode_[slot] != pooling))
    throw std::runtime_error("embed_prefill: start_pos " + std::to_string(start_pos) + " does not continue the slot's " +
                             "pooled positions (" + std::to_string(emb_pos_[slot]) + ")");
  if (pooling == EMBED_NONE) {
    // one staging buffer for every slot: a NONE call on another slot overwrites its first rows, so the
    // prompt that was being staged there cannot be continued any more
    if (emb_rows_slot_ >= 0 && emb_rows_slot_ != slot && emb_mode_[emb_rows_slot_] == EMBED_NONE) emb_pos_[emb_rows_slot_] = -1;
    emb_rows_slot_ = slot;
  }
  emb_pos_[slot] = -1;  // (a call that throws leaves no state to continue)
  const EmbedFold fold{slot, pooling, final};
  ChunkHook hook;
  hook.fn = [&](const float* x, int n, int row0, bool last) { embed_fold(fold, x, n, start_pos + row0, last); };
  hook.deterministic = true;  // the same tokens pool to the same bytes (engine.h)
  prefill_run(slot, tokens, start_pos, false, hook);
  emb_pos_[slot] = start_pos + T;
  emb_mode_[slot] = pooling;
  if (!final) return {};
  emb_tokens_ = start_pos + T;
  std::vector<float> out(pooling == EMBED_NONE ? (size_t)emb_tokens_ * d : (size_t)d);
  HIP_CHECK(hipMemcpyAsync(out.data(), pooling == EMBED_NONE ? emb_rows_ : emb_out_, out.size() * 4,
                           hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

// ---- prompt scoring (engine.h score_prefill) --------------------------------------------------------
int Engine::score_group_rows() const {
  const size_t rows = SCORE_LOGITS_BYTES / ((size_t)cfg_.vocab_size * 4);
  // (at most the prefill chunk: gm_a16_ holds the group's normed rows; the GEMV path's chunks are shorter)
  return (int)std::min<size_t>(std::max<size_t>(rows, SCORE_MIN_ROWS), (size_t)std::max(gm_ok_ ? gm_rows_ : prefill_rows_, 1));
}

void Engine::score_buffers() {
  // First use, not finalize, and all or nothing, as embed_buffers
  if (sc_logits_) return;
  const int V = cfg_.vocab_size, rows = score_group_rows();
  const size_t ctx = (size_t)cfg_.max_ctx;
  float* lg = (float*)dmalloc((size_t)rows * V * 4);
  int* tg = (int*)dmalloc(ctx * 4);
  const size_t ob = ctx * (16 + (size_t)LOGPROB_ROW * 8);
  char* out = (char*)dmalloc(ob);
  int* tn = (int*)dmalloc((size_t)rows * 4);
  size_t lpb = 0;
  void* lpw = nullptr;
  int* lpc = nullptr;
  if (V <= SAMPLE_MAX_V) {
    lpb = logprob_ws_bytes(rows, V);
    lpw = dmalloc(lpb);
    lpc = (int*)dmalloc((size_t)rows * 4);
    HIP_CHECK(hipMemset(lpc, 0, (size_t)rows * 4));
    HIP_CHECK(hipStreamSynchronize(nullptr));  // (the memset ran on the null stream, the kernel runs on ours)
  }
  sc_rows_ = rows; sc_targets_ = tg; sc_out_ = out; sc_topn_ = tn; sc_topn_val_ = -1;
  sc_lp_ws_ = lpw; sc_lp_ws_bytes_ = lpb; sc_lp_cnt_ = lpc;
  sc_logits_ = lg;
  ws_bytes_ += (size_t)rows * V * 4 + ctx * 4 + ob + (size_t)rows * 4 + lpb + (lpc ? (size_t)rows * 4 : 0);
}

// sc_logits_[n][V] = rmsnorm(x) . output^T for n <= sc_rows_ rows: lm_head with an output pointer and a row
// count.  Five rows or more go through the GEMMs (the ring GEMM up to 32, the prefill GEMM above) where the
// prefill does, shorter groups and engines without the GEMM path through the GEMV in sub-batches of 8.
void Engine::score_lm_head(int n, const float* x, int ldx) {
  const int d = cfg_.d_model, V = cfg_.vocab_size;
  if (gm_ok_ && n >= 5 && n <= gm_rows_ && V % 64 == 0 && gemm_supports(output_.w.qtype)) {
    launch_rmsnorm_bf16(x, ldx, out_norm_, gm_a16_, d, n, d, cfg_.norm_eps, stream_);
    GemmQArgs g = gemm_args(gm_a16_, d, n, d, output_.w, V, V, sc_logits_, GEPI_STORE);
    gemm(g);
    return;
  }
  for (int o = 0; o < n; o += 8)
    gemv({&output_}, V, d, std::min(8, n - o), x + (size_t)o * ldx, ldx, out_norm_, sc_logits_ + (size_t)o * V, V,
         EPI_STORE, 0);
}

void Engine::score_fold(const ScoreFold& f, const float* x, int n, int row0) {
  const int d = cfg_.d_model, V = cfg_.vocab_size;
  const size_t T = (size_t)f.T;
  float* out_f = (float*)sc_out_;
  int* out_i = (int*)(sc_out_ + T * 8);
  float* alt_lp = (float*)(sc_out_ + T * 16);
  int* alt_id = (int*)(sc_out_ + T * 16 + T * LOGPROB_ROW * 4);
  for (int g0 = 0; g0 < n; g0 += sc_rows_) {
    const int m = std::min(sc_rows_, n - g0);
    const size_t r = (size_t)row0 + g0;
    score_lm_head(m, x + (size_t)g0 * d, d);
    ScoreArgs a;
    std::memset(&a, 0, sizeof(a));
    a.logits = sc_logits_; a.ldl = V; a.R = m; a.V = V;
    a.targets = sc_targets_ + r; a.out_f = out_f + r * 2; a.out_i = out_i + r * 2;
    launch_score_rows(a, stream_);
    if (f.top_n > 0) {
      LogprobArgs p;
      std::memset(&p, 0, sizeof(p));
      p.logits = sc_logits_; p.ldl = V; p.B = m; p.V = V;
      p.tokens = sc_targets_ + r;  // (the kernel clamps a -1; only the alternatives are read back)
      p.top_n = sc_topn_;
      p.out_lp = alt_lp + r * LOGPROB_ROW; p.out_id = alt_id + r * LOGPROB_ROW;
      p.ws = sc_lp_ws_; p.ws_bytes = sc_lp_ws_bytes_; p.counters = sc_lp_cnt_;
      launch_logprobs(p, stream_);
    }
  }
}

Engine::PromptScores Engine::score_prefill(int slot, const std::vector<int>& tokens, int start_pos, int next_token,
                                           int top_n, bool want_logits) {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("score_prefill: single-GPU engines only");
  if (top_n < 0 || top_n > LOGPROB_MAX_TOP)
    throw std::runtime_error("score_prefill: top_n outside 0.." + std::to_string(LOGPROB_MAX_TOP));
  const int V = cfg_.vocab_size, T = (int)tokens.size();
  if (top_n > 0 && V > SAMPLE_MAX_V)
    throw std::runtime_error("score_prefill: alternatives need a vocabulary up to " + std::to_string(SAMPLE_MAX_V));
  if (next_token < -1 || next_token >= V) throw std::runtime_error("score_prefill: next_token out of range");
  if (T == 0) throw std::runtime_error("score_prefill: empty prompt");
  if (start_pos < 0 || start_pos + T > cfg_.max_ctx) throw std::runtime_error("score_prefill: context overflow");
  for (int t : tokens)
    if (t < 0 || t >= V) throw std::runtime_error("score_prefill: token id out of range");
  HIP_CHECK(hipSetDevice(cfg_.device));
  score_buffers();
  std::vector<int> tg(T);
  for (int i = 0; i + 1 < T; ++i) tg[i] = tokens[i + 1];
  tg[T - 1] = next_token;
  HIP_CHECK(hipMemcpyAsync(sc_targets_, tg.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream_));
  if (top_n > 0 && sc_topn_val_ != top_n) {
    const std::vector<int> tn(sc_rows_, top_n);
    HIP_CHECK(hipMemcpyAsync(sc_topn_, tn.data(), tn.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));  // (tn leaves scope)
    sc_topn_val_ = top_n;
  }
  const ScoreFold sf{top_n, T};
  ChunkHook hook;
  hook.fn = [&](const float* x, int n, int row0, bool) { score_fold(sf, x, n, row0); };
  prefill_run(slot, tokens, start_pos, want_logits, hook);
  // one copy of what the call staged: [T][2] floats | [T][2] ints (| [T][LOGPROB_ROW] floats | ... ints)
  const size_t nbytes = (size_t)T * (16 + (top_n > 0 ? (size_t)LOGPROB_ROW * 8 : 0));
  std::vector<char> host(nbytes);
  HIP_CHECK(hipMemcpyAsync(host.data(), sc_out_, nbytes, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  const float* hf = (const float*)host.data();
  const int* hi = (const int*)(host.data() + (size_t)T * 8);
  PromptScores r;
  r.lp.resize(T); r.best_lp.resize(T); r.rank.resize(T); r.best.resize(T);
  for (int i = 0; i < T; ++i) {
    r.lp[i] = hf[2 * i]; r.best_lp[i] = hf[2 * i + 1];
    r.rank[i] = hi[2 * i]; r.best[i] = hi[2 * i + 1];
  }
  if (top_n > 0) {
    const float* al = (const float*)(host.data() + (size_t)T * 16);
    const int* ai = (const int*)(host.data() + (size_t)T * 16 + (size_t)T * LOGPROB_ROW * 4);
    r.ids.resize((size_t)T * top_n);
    r.lps.resize((size_t)T * top_n);
    for (int i = 0; i < T; ++i)
      for (int j = 0; j < top_n; ++j) {
        r.ids[(size_t)i * top_n + j] = ai[(size_t)i * LOGPROB_ROW + 1 + j];
        r.lps[(size_t)i * top_n + j] = al[(size_t)i * LOGPROB_ROW + 1 + j];
      }
  }
  return r;
}

std::vector<int> Engine::decode(const std::vector<int>& slots, const std::vector<int>& tokens,
                                const std::vector<int>& pos, const std::vector<float>& temperature,
                                const std::vector<int>& top_k, uint64_t seed, const std::vector<uint8_t>& mask,
                                const std::vector<float>& top_p, const std::vector<uint64_t>& seeds) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int B = (int)slots.size();
  const SampleStage stage(*this, B, "decode");  // (before the step changes any state)
  check_step("decode", slots, tokens, pos, seeds, true);
  bool masked = !mask.empty();
  if (masked && mask.size() != (size_t)B * ((cfg_.vocab_size + 7) / 8))
    throw std::runtime_error("decode: mask size mismatch");
  row_slots_ = slots;
  row_pos_ = pos;
  // one pinned staging block -> one async copy; the device-resident seed lets one captured graph per
  // (B, masked) serve every request
  upload_step_params(slots, tokens, pos, temperature, top_k, top_p, seed, seeds, mask);
  if (take_grammar(B, masked)) masked = true;  // (behind the mask's copy, in front of the graph that samples)
  if (proc_rows_ || lp_rows_) {
    // staged logit processors / logprobs: the forward graph and an eager sampler (and logprob launch), as
    // the pipelined path runs a step -- the captured (B, masked) step graphs never see them
    advance_rows(B, 1);
    HIP_CHECK(hipGraphLaunch(forward_graph(B), stream_));
    enqueue_sample(B, masked, SAMPLE_STEP, true);
  } else {
    decode_loop_body(B, 1, true, masked);
  }
  HIP_CHECK(hipMemcpyAsync(h_tok_out_, d_tokens_, B * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return std::vector<int>(h_tok_out_, h_tok_out_ + B);
}

Engine::SpecResult Engine::spec_decode(int slot, const std::vector<int>& tokens, int pos0, float temperature, int top_k,
                                       float top_p, uint64_t seed, const std::vector<uint8_t>& masks) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int R = (int)tokens.size();
  const SampleStage stage(*this, R, "spec_decode");  // (before the step changes any state)
  if (cfg_.tp_size > 1) throw std::runtime_error("spec_decode: not available on a tensor-parallel engine");
  if (pipe_sampled_) throw std::runtime_error("spec_decode: a pipelined step is in flight");
  if (R < 2 || R > std::min(cfg_.max_batch, SPEC_MAX_ROWS)) throw std::runtime_error("spec_decode: rows out of range");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("spec_decode: bad slot");
  if (pos0 < 0 || pos0 + R > cfg_.max_ctx) throw std::runtime_error("spec_decode: positions out of range");
  for (int t : tokens)
    if (t < 0 || t >= cfg_.vocab_size) throw std::runtime_error("spec_decode: token out of range");
  if (!masks.empty() && masks.size() != (size_t)R * ((cfg_.vocab_size + 7) / 8))
    throw std::runtime_error("spec_decode: mask size mismatch");
  // the rows of decode(): one slot, consecutive positions, the request's parameters and seed on every row
  row_slots_.assign(R, slot);
  row_pos_.resize(R);
  for (int i = 0; i < R; ++i) row_pos_[i] = pos0 + i;
  upload_step_params(row_slots_, tokens, row_pos_, std::vector<float>(R, temperature), std::vector<int>(R, top_k),
                     std::vector<float>(R, top_p), seed, std::vector<uint64_t>(R, seed), masks);
  // the input tokens once more, apart from d_tokens_ (the sampler overwrites those)
  std::copy(tokens.begin(), tokens.end(), h_spec_);
  HIP_CHECK(hipMemcpyAsync(d_spec_, h_spec_, (size_t)R * 4, hipMemcpyHostToDevice, stream_));
  advance_rows(R, 1);  // (the host rows become the one row behind the accepted tokens below)
  HIP_CHECK(hipGraphLaunch(forward_graph(R), stream_));
  enqueue_sample(R, !masks.empty(), SAMPLE_STEP, true);
  SpecAcceptArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in = d_spec_; a.out = d_tokens_; a.pos0 = pos0; a.R = R;
  a.record = d_spec_ + SPEC_MAX_ROWS;
  a.tokens = d_tokens_; a.pos = d_pos_; a.seq_len = d_seqlen_;
  a.history = d_history_; a.hist_stride = cfg_.max_ctx + 1;
  launch_spec_accept(a, stream_);
  int* h_rec = h_spec_ + SPEC_MAX_ROWS;
  HIP_CHECK(hipMemcpyAsync(h_rec, d_spec_ + SPEC_MAX_ROWS, (size_t)SPEC_RECORD * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  SpecResult r;
  r.accepted = std::min(std::max(h_rec[0], 0), R - 1);
  r.tokens.assign(h_rec + 1, h_rec + 2 + r.accepted);
  // the step state is one row now: the sequence at pos0 + accepted + 1
  row_slots_.assign(1, slot);
  row_pos_.assign(1, pos0 + r.accepted + 1);
  return r;
}

std::vector<Engine::SpecResult> Engine::spec_decode_multi(const std::vector<int>& slots,
                                                          const std::vector<std::vector<int>>& tokens,
                                                          const std::vector<int>& pos0, const std::vector<float>& temperature,
                                                          const std::vector<int>& top_k, const std::vector<float>& top_p,
                                                          const std::vector<uint64_t>& seeds,
                                                          const std::vector<uint8_t>& masks) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int S = (int)slots.size();
  size_t total = 0;
  for (const auto& t : tokens) total += t.size();
  // (clamped only so that the stage below can be taken before the arguments are checked: a call that throws
  // must drop what was staged; a total past max_batch is refused further down, before Rt is used)
  const int Rt = (int)std::min<size_t>(total, (size_t)cfg_.max_batch + 1);
  const SampleStage stage(*this, Rt, "spec_decode_multi");  // (before the step changes any state)
  if (cfg_.tp_size > 1) throw std::runtime_error("spec_decode_multi: not available on a tensor-parallel engine");
  if (pipe_sampled_) throw std::runtime_error("spec_decode_multi: a pipelined step is in flight");
  if (S < 1 || S > SPEC_MULTI_MAX_SEQS) throw std::runtime_error("spec_decode_multi: sequences out of range");
  if ((int)tokens.size() != S || (int)pos0.size() != S || (int)temperature.size() != S || (int)top_k.size() != S ||
      (int)top_p.size() != S || (int)seeds.size() != S)
    throw std::runtime_error("spec_decode_multi: size mismatch");
  for (const auto& t : tokens)
    if (t.empty() || (int)t.size() > SPEC_MAX_ROWS) throw std::runtime_error("spec_decode_multi: a segment's rows out of range");
  if (total > (size_t)std::min(cfg_.max_batch, SPEC_MULTI_MAX_ROWS)) throw std::runtime_error("spec_decode_multi: rows out of range");
  for (int s = 0; s < S; ++s) {
    if (slots[s] < 0 || slots[s] >= cfg_.max_slots) throw std::runtime_error("spec_decode_multi: bad slot");
    for (int t = 0; t < s; ++t)
      if (slots[t] == slots[s]) throw std::runtime_error("spec_decode_multi: a slot named twice");
    if (pos0[s] < 0 || pos0[s] + (int)tokens[s].size() > cfg_.max_ctx)
      throw std::runtime_error("spec_decode_multi: positions out of range");
    for (int t : tokens[s])
      if (t < 0 || t >= cfg_.vocab_size) throw std::runtime_error("spec_decode_multi: token out of range");
  }
  if (!masks.empty() && masks.size() != (size_t)Rt * ((cfg_.vocab_size + 7) / 8))
    throw std::runtime_error("spec_decode_multi: mask size mismatch");
  if (!d_specm_) {
    // first use, not finalize (as embed_buffers): an engine that never takes such a step allocates what it always did
    const size_t n = SPEC_MULTI_MAX_ROWS + SPEC_MULTI_MAX_SEQS * SPEC_RECORD;
    // (the pinned mirror first: if it fails nothing is held, and if the device buffer fails the mirror is kept
    // for the next call -- neither leaves a second device buffer behind)
    if (!h_specm_) HIP_CHECK(hipHostMalloc((void**)&h_specm_, n * 4, hipHostMallocDefault));
    d_specm_ = (int*)dmalloc(n * 4);
    ws_bytes_ += n * 4;
  }
  // the rows of decode(), segment after segment: a sequence's slot, consecutive positions, parameters and seed
  SpecAcceptMultiArgs a;
  std::memset(&a, 0, sizeof(a));
  std::vector<int> flat(Rt), rtk(Rt);
  std::vector<float> rT(Rt), rP(Rt);
  std::vector<uint64_t> rs(Rt);
  row_slots_.resize(Rt);
  row_pos_.resize(Rt);
  for (int s = 0, r = 0; s < S; ++s) {
    a.seg[s] = r; a.pos0[s] = pos0[s];
    for (int i = 0; i < (int)tokens[s].size(); ++i, ++r) {
      row_slots_[r] = slots[s]; row_pos_[r] = pos0[s] + i; flat[r] = tokens[s][i];
      rT[r] = temperature[s]; rtk[r] = top_k[s]; rP[r] = top_p[s]; rs[r] = seeds[s];
    }
  }
  a.seg[S] = Rt; a.S = S;
  upload_step_params(row_slots_, flat, row_pos_, rT, rtk, rP, seeds[0], rs, masks);
  // the input tokens once more, apart from d_tokens_ (the sampler overwrites those)
  std::copy(flat.begin(), flat.end(), h_specm_);
  HIP_CHECK(hipMemcpyAsync(d_specm_, h_specm_, (size_t)Rt * 4, hipMemcpyHostToDevice, stream_));
  const bool masked = take_grammar(Rt, !masks.empty()) || !masks.empty();
  advance_rows(Rt, 1);  // (the host rows become the S rows behind the accepted tokens below)
  HIP_CHECK(hipGraphLaunch(forward_graph(Rt), stream_));
  enqueue_sample(Rt, masked, SAMPLE_STEP, true);
  a.in = d_specm_; a.out = d_tokens_;
  a.record = d_specm_ + SPEC_MULTI_MAX_ROWS;
  a.tokens = d_tokens_; a.pos = d_pos_; a.seq_len = d_seqlen_;
  a.history = d_history_; a.hist_stride = cfg_.max_ctx + 1;
  launch_spec_accept_multi(a, stream_);
  int* h_rec = h_specm_ + SPEC_MULTI_MAX_ROWS;
  HIP_CHECK(hipMemcpyAsync(h_rec, d_specm_ + SPEC_MULTI_MAX_ROWS, (size_t)S * SPEC_RECORD * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  std::vector<SpecResult> res(S);
  // the step state is S rows now: sequence s at pos0[s] + accepted_s + 1
  row_slots_ = slots;
  row_pos_.resize(S);
  for (int s = 0; s < S; ++s) {
    const int* rec = h_rec + (size_t)s * SPEC_RECORD;
    res[s].accepted = std::min(std::max(rec[0], 0), (int)tokens[s].size() - 1);
    res[s].tokens.assign(rec + 1, rec + 2 + res[s].accepted);
    row_pos_[s] = pos0[s] + res[s].accepted + 1;
  }
  return res;
}

std::vector<int> Engine::resample(int B, const std::vector<float>& temperature, const std::vector<int>& top_k,
                                  uint64_t seed, const std::vector<uint8_t>& mask, const std::vector<float>& top_p) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  // re-run only the sampler on the logits of the last step (grammar fast path: the unmasked
  // sample was rejected on the host)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  const SampleStage stage(*this, B, "resample");  // (before the sampler is enqueued)
  if (B < 1 || B > cfg_.max_batch) throw std::runtime_error("resample: batch out of range");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t mbytes = (size_t)B * ((cfg_.vocab_size + 7) / 8);
  if (!mask.empty() && mask.size() != mbytes) throw std::runtime_error("resample: mask size mismatch");
  upload_sample_params(B, temperature, top_k, top_p, seed, {}, true);
  if (!mask.empty()) HIP_CHECK(hipMemcpyAsync(d_mask_, mask.data(), mbytes, hipMemcpyHostToDevice, stream_));
  const bool gm = take_grammar(B, !mask.empty());
  enqueue_sample(B, gm || !mask.empty(), SAMPLE_AGAIN, true);
  std::vector<int> out(B);
  HIP_CHECK(hipMemcpyAsync(out.data(), d_tokens_, B * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

// rows without their own seed keep the shared seed decorrelated by row (the round-2 stream keyed
// (seed, row, pos)); rows with one (a request's own seed) sample independently of their row
void Engine::fill_row_seeds(uint64_t* hs, int B, uint64_t seed, const std::vector<uint64_t>& seeds) {
  for (int b = 0; b < B; ++b) hs[b] = seeds.empty() ? seed ^ (0x9E3779B97F4A7C15ULL * (uint64_t)(b + 1)) : seeds[b];
}

int Engine::sample_first(int pos, float temperature, int top_k, float top_p, uint64_t seed,
                         const std::vector<uint8_t>& mask) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  const SampleStage stage(*this, 1, "sample_first");  // (before the sampler is enqueued)
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t mbytes = (size_t)((cfg_.vocab_size + 7) / 8);
  if (!mask.empty() && mask.size() != mbytes) throw std::runtime_error("sample_first: mask size mismatch");
  // row 0 of the parameter block (its row seed: the request's own): the next decode() re-uploads every row it uses
  upload_sample_params(1, {temperature}, {top_k}, {top_p}, seed, {seed}, false);
  HIP_CHECK(hipMemcpyAsync(d_fpos_, &pos, 4, hipMemcpyHostToDevice, stream_));
  if (!mask.empty()) HIP_CHECK(hipMemcpyAsync(d_mask_, mask.data(), mbytes, hipMemcpyHostToDevice, stream_));
  const bool gm = take_grammar(1, !mask.empty());
  enqueue_sample(1, gm || !mask.empty(), SAMPLE_FIRST, true);
  int out = 0;
  HIP_CHECK(hipMemcpyAsync(&out, d_tokens_, 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

std::vector<float> Engine::last_logits(int B) {
  std::vector<float> out((size_t)B * cfg_.vocab_size);
  HIP_CHECK(hipMemcpyAsync(out.data(), logits_, out.size() * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

void Engine::decode_loop_prepare(const std::vector<int>& slots, const std::vector<int>& tokens,
                                 const std::vector<int>& pos) {
  const int B = (int)slots.size();
  if (B < 1 || B > cfg_.max_batch || (int)pos.size() != B || (int)tokens.size() != B)
    throw std::runtime_error("decode_loop_prepare: bad batch");
  std::vector<int> sl(B);
  for (int b = 0; b < B; ++b) sl[b] = pos[b] + 1;
  row_slots_ = slots;
  row_pos_ = pos;
  std::vector<float> temps(B, 0.f);
  std::vector<int> tks(B, 0);
  HIP_CHECK(hipMemcpyAsync(d_slot_, slots.data(), B * 4, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_tokens_, tokens.data(), B * 4, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_pos_, pos.data(), B * 4, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_seqlen_, sl.data(), B * 4, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_temp_, temps.data(), B * 4, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_topk_, tks.data(), B * 4, hipMemcpyHostToDevice, stream_));
  std::vector<float> ones(B, 1.f);
  HIP_CHECK(hipMemcpyAsync(d_topp_, ones.data(), B * 4, hipMemcpyHostToDevice, stream_));
  const uint64_t zero = 0;
  HIP_CHECK(hipMemcpyAsync(d_seed_, &zero, 8, hipMemcpyHostToDevice, stream_));
  std::vector<uint64_t> hs(B);
  fill_row_seeds(hs.data(), B, 0, {});
  HIP_CHECK(hipMemcpyAsync(d_seeds_, hs.data(), (size_t)B * 8, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::decode_loop_run(int B, int n_steps, bool use_graph) { decode_loop_body(B, n_steps, use_graph, false); }

void Engine::decode_loop_body(int B, int n_steps, bool use_graph, bool masked) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  TraceRange tr(use_graph ? "aios.decode_graph_replay" : "aios.decode_eager");
  HIP_CHECK(hipSetDevice(cfg_.device));
  if ((int)row_slots_.size() < B) throw std::runtime_error("decode_loop_run: rows not prepared");
  // (these steps never carry staged processors or a logprob launch: a staging is dropped, not kept for later)
  lp_last_.clear();
  proc_rows_ = lp_rows_ = gr_rows_ = 0;
  advance_rows(B, n_steps);
  if (!use_graph) {
    for (int i = 0; i < n_steps; ++i) enqueue_decode_step(B, masked);
    return;
  }
  hipGraphExec_t ge = step_graph(B, masked);
  for (int i = 0; i < n_steps; ++i) HIP_CHECK(hipGraphLaunch(ge, stream_));
}

void Engine::advance_rows(int B, int n) {
  for (int b = 0; b < B; ++b) {
    const int to = std::min(row_pos_[b] + n, cfg_.max_ctx);
    kv_prepare_write(row_slots_[b], row_pos_[b], to);
    row_pos_[b] = to;
  }
  kv_sync(B);
}

hipGraphExec_t Engine::graph_for(int key, const std::function<void()>& enqueue) {
  auto it = graphs_.find(key);
  if (it == graphs_.end()) {
    hipGraph_t g;
    HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    try {
      enqueue();
    } catch (...) {
      hipStreamEndCapture(stream_, &g);
      throw;
    }
    HIP_CHECK(hipStreamEndCapture(stream_, &g));
    hipGraphExec_t ge;
    HIP_CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(g));
    it = graphs_.emplace(key, ge).first;
  }
  return it->second;
}

// the captured decode step for (B, masked): captured once, replayed for every request --
// the kernels read tokens / positions / slots / sampling parameters from device arrays
hipGraphExec_t Engine::step_graph(int B, bool masked) {
  return graph_for(B * 4 + (masked ? 1 : 0), [&] { enqueue_decode_step(B, masked); });
}

// the forward of a decode step without its sampler (the pipelined decode's graph)
hipGraphExec_t Engine::forward_graph(int B) {
  return graph_for(B * 4 + 2, [&] { enqueue_decode_forward(B); });
}

void Engine::write_step_params(char* hpar, const std::vector<int>& slots, const std::vector<int>& tokens,
                               const std::vector<int>& pos, const std::vector<float>& temperature,
                               const std::vector<int>& top_k, const std::vector<float>& top_p, uint64_t seed,
                               const std::vector<uint64_t>& seeds) {
  const int B = (int)slots.size();
  int *hs = (int*)(hpar + par_off(PAR_SLOT)), *ht = (int*)(hpar + par_off(PAR_TOKEN));
  int *hp = (int*)(hpar + par_off(PAR_POS)), *hl = (int*)(hpar + par_off(PAR_SEQLEN));
  for (int b = 0; b < B; ++b) {
    hs[b] = slots[b]; hp[b] = pos[b]; hl[b] = pos[b] + 1;
    if (!tokens.empty()) ht[b] = tokens[b];
  }
  write_sample_params(hpar, B, temperature, top_k, top_p, seed, seeds);
}

void Engine::write_sample_params(char* hpar, int B, const std::vector<float>& temperature, const std::vector<int>& top_k,
                                 const std::vector<float>& top_p, uint64_t seed, const std::vector<uint64_t>& seeds) {
  *(uint64_t*)hpar = seed;
  int* hk = (int*)(hpar + par_off(PAR_TOPK));
  float *hT = (float*)(hpar + par_off(PAR_TEMP)), *hP = (float*)(hpar + par_off(PAR_TOPP));
  for (int b = 0; b < B; ++b) {
    hk[b] = b < (int)top_k.size() ? top_k[b] : 0;
    hT[b] = b < (int)temperature.size() ? temperature[b] : 0.f;
    hP[b] = b < (int)top_p.size() ? top_p[b] : 1.f;
  }
  fill_row_seeds((uint64_t*)(hpar + par_seeds_off_), B, seed, seeds);
}

void Engine::par_copy(const char* hpar, size_t from, size_t to) {
  HIP_CHECK(hipMemcpyAsync(d_par_ + from, hpar + from, to - from, hipMemcpyHostToDevice, stream_));
}

void Engine::upload_step_params(const std::vector<int>& slots, const std::vector<int>& tokens,
                                const std::vector<int>& pos, const std::vector<float>& temperature,
                                const std::vector<int>& top_k, const std::vector<float>& top_p, uint64_t seed,
                                const std::vector<uint64_t>& seeds, const std::vector<uint8_t>& mask) {
  // the other half: the copy of the previous upload may not have run yet (a pipelined step's, or that of a
  // forward the scheduler queued and dropped)
  char* hpar = next_par();
  write_step_params(hpar, slots, tokens, pos, temperature, top_k, top_p, seed, seeds);
  size_t from = 0, end = par_seeds_off_ + (size_t)cfg_.max_batch * 8;
  if (!mask.empty()) {
    std::memcpy(hpar + par_mask_off_, mask.data(), mask.size());
    end = par_mask_off_ + mask.size();
  }
  if (tokens.empty()) {  // every row array but the tokens the previous sampler left on the device
    par_copy(hpar, 0, par_off(PAR_TOKEN));
    from = par_off(PAR_TOKEN + 1);
  }
  par_copy(hpar, from, end);
}

void Engine::upload_sample_params(int B, const std::vector<float>& temperature, const std::vector<int>& top_k,
                                  const std::vector<float>& top_p, uint64_t seed, const std::vector<uint64_t>& seeds,
                                  bool dev_seed) {
  char* hpar = next_par();
  write_sample_params(hpar, B, temperature, top_k, top_p, seed, seeds);
  if (dev_seed) par_copy(hpar, 0, 8);
  par_copy(hpar, par_off(PAR_TOPK), par_off(PAR_TOPP) + (size_t)B * 4);  // (rows past B of top_k / temperature too)
  par_copy(hpar, par_seeds_off_, par_seeds_off_ + (size_t)B * 8);
}

void Engine::check_step(const std::string& who, const std::vector<int>& slots, const std::vector<int>& tokens,
                        const std::vector<int>& pos, const std::vector<uint64_t>& seeds, bool need_tokens) const {
  const int B = (int)slots.size();
  const bool host_tokens = need_tokens || !tokens.empty();
  if (B < 1 || B > cfg_.max_batch) throw std::runtime_error(who + ": batch out of range");
  if ((int)pos.size() != B || (host_tokens && (int)tokens.size() != B))
    throw std::runtime_error(who + ": size mismatch");
  if (!seeds.empty() && (int)seeds.size() != B) throw std::runtime_error(who + ": seeds size mismatch");
  for (int b = 0; b < B; ++b) {
    if (pos[b] < 0 || pos[b] >= cfg_.max_ctx) throw std::runtime_error(who + ": position out of range");
    if (slots[b] < 0 || slots[b] >= cfg_.max_slots) throw std::runtime_error(who + ": bad slot");
    if (host_tokens && (tokens[b] < 0 || tokens[b] >= cfg_.vocab_size))
      throw std::runtime_error(who + ": token out of range");
  }
}

void Engine::decode_submit(const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
                           const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
                           const std::vector<float>& top_p, const std::vector<uint64_t>& seeds) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int B = (int)slots.size();
  check_step("decode_submit", slots, tokens, pos, seeds, false);
  upload_step_params(slots, tokens, pos, temperature, top_k, top_p, seed, seeds);  // (no mask: decode_sample's)
  row_slots_ = slots;
  row_pos_ = pos;
  advance_rows(B, 1);
  HIP_CHECK(hipGraphLaunch(forward_graph(B), stream_));
  pipe_B_ = B;
}

void Engine::decode_sample(const std::vector<uint8_t>& mask) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  const int B = pipe_B_;
  if (B < 1) throw std::runtime_error("decode_sample: no submitted step");
  const SampleStage stage(*this, B, "decode_sample");  // (before the sampler is enqueued)
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t mbytes = (size_t)B * ((cfg_.vocab_size + 7) / 8);
  if (!mask.empty()) {
    if (mask.size() != mbytes) throw std::runtime_error("decode_sample: mask size mismatch");
    // (one pinned buffer: the previous mask's copy ran before the sampler whose token the host
    // already collected)
    std::memcpy(h_mask_, mask.data(), mbytes);
    HIP_CHECK(hipMemcpyAsync(d_mask_, h_mask_, mbytes, hipMemcpyHostToDevice, stream_));
  }
  const bool gm = take_grammar(B, !mask.empty());
  enqueue_sample(B, gm || !mask.empty(), SAMPLE_STEP, true);
  HIP_CHECK(hipMemcpyAsync(h_tok_out_, d_tokens_, B * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipEventRecord(pipe_ev_, stream_));
  pipe_sampled_ = true;
}

std::vector<int> Engine::decode_collect() {
  const int B = pipe_B_;
  if (B < 1) throw std::runtime_error("decode_collect: no sampled step");
  HIP_CHECK(hipEventSynchronize(pipe_ev_));
  pipe_sampled_ = false;
  return std::vector<int>(h_tok_out_, h_tok_out_ + B);
}

// capture (without running) the decode-step graphs of every batch size up to max_b, masked and
// unmasked, so a serving scheduler whose batch grows and shrinks never stalls a step on a capture
// (a 160-launch capture + instantiate costs milliseconds); returns the graphs held
int Engine::capture_graphs(int max_b) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  HIP_CHECK(hipSetDevice(cfg_.device));
  for (int B = 1; B <= std::min(max_b, cfg_.max_batch); ++B) {
    step_graph(B, false);
    forward_graph(B);  // (the pipelined decode's forward)
    step_graph(B, true);
  }
  return (int)graphs_.size();
}

std::vector<int> Engine::decode_loop_history(int B, int from_pos, int n) {
  std::vector<int> out((size_t)B * n);
  for (int b = 0; b < B; ++b)
    HIP_CHECK(hipMemcpyAsync(out.data() + (size_t)b * n, d_history_ + (size_t)b * (cfg_.max_ctx + 1) + from_pos,
                             n * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

void Engine::synchronize() {
  HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::set_kv_scales(const std::vector<float>& s) {
  if (s.size() != (size_t)2 * cfg_.n_layers) throw std::runtime_error("set_kv_scales: need 2 x n_layers values");
  for (float v : s)
    if (!(v > 0.f) || !std::isfinite(v)) throw std::runtime_error("set_kv_scales: scales must be positive");
  if (finalized_) HIP_CHECK(hipStreamSynchronize(stream_));  // (no replay of the old graphs in flight)
  kv_scale_ = s;
  reset_graphs();
}

std::vector<float> kv_scales_from_amax(const std::vector<float>& amax, int n_layers, int n_kv_heads, float headroom) {
  if (n_layers < 0 || n_kv_heads < 1 || amax.size() != (size_t)n_layers * 2 * n_kv_heads)
    throw std::runtime_error("kv_scales_from_amax: need n_layers x 2 x n_kv_heads values");
  if (!(headroom >= 1.f) || !std::isfinite(headroom)) throw std::runtime_error("kv_scales_from_amax: headroom must be >= 1");
  std::vector<float> s((size_t)2 * n_layers, 1.f);
  for (int l = 0; l < n_layers; ++l)
    for (int kv = 0; kv < 2; ++kv) {
      float m = 0.f;
      for (int h = 0; h < n_kv_heads; ++h) {
        const float v = amax[((size_t)l * 2 + kv) * n_kv_heads + h];
        if (!std::isfinite(v))
          throw std::runtime_error("fp8 KV calibration: non-finite " + std::string(kv ? "V" : "K") + " maximum in layer " +
                                   std::to_string(l) + " (head " + std::to_string(h) + ")");
        m = std::max(m, std::fabs(v));
      }
      const float sc = (m * headroom) / 448.f;
      // (all zeros -- or a product that leaves fp32's range -- keeps 1.0: set_kv_scales wants positive finite values)
      if (sc > 0.f && std::isfinite(sc)) s[(size_t)2 * l + kv] = sc;
    }
  return s;
}

std::vector<float> Engine::calibrate_kv_scales(const std::vector<int>& tokens, float headroom) {
  if (!finalized_) throw std::runtime_error("calibrate_kv_scales: engine not finalized");
  if (!cfg_.kv_fp8) throw std::runtime_error("calibrate_kv_scales: the KV cache is not fp8");
  if (tokens.empty()) throw std::runtime_error("calibrate_kv_scales: empty prompt");
  if (!(headroom >= 1.f) || !std::isfinite(headroom)) throw std::runtime_error("calibrate_kv_scales: headroom must be >= 1");
  int slot = -1;
  for (int s = 0; s < cfg_.max_slots && slot < 0; ++s) {
    bool empty = true;
    for (int j = 0; j < kv_maxb_; ++j) empty = empty && bt_[(size_t)s * kv_maxb_ + j] < 0;
    if (empty) slot = s;
  }
  if (slot < 0) throw std::runtime_error("calibrate_kv_scales: no free slot (every slot holds KV blocks)");
  HIP_CHECK(hipSetDevice(cfg_.device));
  const size_t n = (size_t)cfg_.n_layers * 2 * cfg_.n_kv_heads;
  HIP_CHECK(hipMemsetAsync(d_kv_amax_, 0, n * sizeof(unsigned), stream_));
  kv_obs_ = true;
  try {
    prefill(slot, tokens, 0, false);
  } catch (...) {
    kv_obs_ = false;
    release_slot(slot);
    throw;
  }
  kv_obs_ = false;
  release_slot(slot);  // (the codes of this pass were written with the old scales)
  std::vector<float> tab(n);
  HIP_CHECK(hipMemcpyAsync(tab.data(), d_kv_amax_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  kv_amax_ = tab;
  const std::vector<float> s = kv_scales_from_amax(tab, cfg_.n_layers, cfg_.n_kv_heads, headroom);
  set_kv_scales(s);
  return s;
}

void Engine::reset_graphs() {
  for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  graphs_.clear();
}

// ---- paged KV ----------------------------------------------------------------------------------
int Engine::kv_alloc() {
  if (free_blocks_.empty()) throw std::runtime_error("paged KV: pool exhausted");  // cannot happen, see finalize
  const int b = free_blocks_.back();
  free_blocks_.pop_back();
  refcnt_[b] = 1;
  return b;
}

void Engine::kv_unref(int blk) {
  if (blk < 0) return;
  if (--refcnt_[blk] == 0) free_blocks_.push_back(blk);
}

// one block of every layer's K and V pool: [n_kv_heads][KV_BLOCK][hd] contiguous
void Engine::kv_copy_block(int src, int dst) {
  const size_t blk = (size_t)cfg_.n_kv_heads * KV_BLOCK * cfg_.head_dim * kv_es_;  // bytes
  for (int l = 0; l < cfg_.n_layers; ++l)
    for (bf16_t* base : {k_cache_, v_cache_}) {
      char* lb = (char*)kv_layer(base, l);
      HIP_CHECK(hipMemcpyAsync(lb + (size_t)dst * blk, lb + (size_t)src * blk, blk, hipMemcpyDeviceToDevice, stream_));
    }
}

void Engine::kv_prepare_write(int slot, int from, int to) {
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("paged KV: bad slot");
  if (to <= from) return;
  int* row = bt_.data() + (size_t)slot * kv_maxb_;
  for (int j = from / KV_BLOCK; j <= (to - 1) / KV_BLOCK && j < kv_maxb_; ++j) {
    if (row[j] < 0) {
      row[j] = kv_alloc();
      bt_dirty_ = true;
    } else if (refcnt_[row[j]] > 1) {  // shared prefix block about to be written: un-share
      const int nb = kv_alloc();
      kv_copy_block(row[j], nb);
      kv_unref(row[j]);
      row[j] = nb;
      bt_dirty_ = true;
    }
  }
}

// Upload the slot table (when dirty) and the row table of decode rows 0..B-1 (when it changed).
// Blocking uploads with the stream drained first: the captured decode graph reads the tables in
// place, and a table changes only every KV_BLOCK tokens of a sequence or when rows change.
void Engine::kv_sync(int B) {
  bool rows_changed = false;
  std::vector<int> rows((size_t)B * kv_maxb_);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < kv_maxb_; ++j) {
      const int v = bt_[(size_t)row_slots_[b] * kv_maxb_ + j];
      rows[(size_t)b * kv_maxb_ + j] = v < 0 ? kv_nblocks_ : v;
    }
  if (B > 0 && std::memcmp(rows.data(), row_bt_host_.data(), rows.size() * 4) != 0) rows_changed = true;
  if (!bt_dirty_ && !rows_changed) return;
  HIP_CHECK(hipStreamSynchronize(stream_));
  if (bt_dirty_) {
    std::vector<int> dev(bt_.size());
    for (size_t i = 0; i < bt_.size(); ++i) dev[i] = bt_[i] < 0 ? kv_nblocks_ : bt_[i];
    // (on the engine's stream, not the null stream: a co-resident tier's CU-masked stream is a
    // blocking stream, and a null-stream copy would wait for the other tier's queued steps)
    HIP_CHECK(hipMemcpyAsync(d_bt_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    bt_dirty_ = false;
  }
  if (rows_changed) {
    std::copy(rows.begin(), rows.end(), row_bt_host_.begin());
    HIP_CHECK(hipMemcpyAsync(d_row_bt_, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
}

void Engine::copy_slot(int src, int dst, int n) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (src < 0 || src >= cfg_.max_slots || dst < 0 || dst >= cfg_.max_slots) throw std::runtime_error("copy_slot: bad slot");
  if (src == dst) return;
  HIP_CHECK(hipSetDevice(cfg_.device));
  n = std::min(n, cfg_.max_ctx);
  int* s = bt_.data() + (size_t)src * kv_maxb_;
  int* d = bt_.data() + (size_t)dst * kv_maxb_;
  for (int j = 0; j < kv_maxb_; ++j) {  // dst's old content is dropped
    kv_unref(d[j]);
    d[j] = -1;
  }
  const int full = std::max(n, 0) / KV_BLOCK;
  for (int j = 0; j < full; ++j) {
    d[j] = s[j];
    if (d[j] >= 0) ++refcnt_[d[j]];
  }
  if (n > 0 && n % KV_BLOCK && s[full] >= 0) {  // the partial block: private copy
    d[full] = kv_alloc();
    kv_copy_block(s[full], d[full]);
  }
  bt_dirty_ = true;
  kv_sync(0);
  HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::release_slot(int slot) {
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("release_slot: bad slot");
  int* row = bt_.data() + (size_t)slot * kv_maxb_;
  for (int j = 0; j < kv_maxb_; ++j) {
    if (row[j] >= 0) bt_dirty_ = true;
    kv_unref(row[j]);
    row[j] = -1;
  }
}

int Engine::shift_context(int slot, int n_tokens, int n_keep, int n_discard) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error("shift_context: not available on a tensor-parallel engine");
  if (pipe_sampled_) throw std::runtime_error("shift_context: a pipelined step is in flight");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("shift_context: bad slot");
  if (n_tokens < 1 || n_tokens > cfg_.max_ctx) throw std::runtime_error("shift_context: n_tokens out of range");
  if (n_keep < 0) throw std::runtime_error("shift_context: n_keep is negative");
  if (n_discard < 1) throw std::runtime_error("shift_context: n_discard below 1");
  if (n_keep > n_tokens - n_discard) throw std::runtime_error("shift_context: n_keep + n_discard beyond n_tokens");
  const int n_new = n_tokens - n_discard;
  int* row = bt_.data() + (size_t)slot * kv_maxb_;
  {
    // the blocks kv_prepare_write will take, counted first: a throw half way would leave the tables changed
    size_t need = 0;
    if (n_new > n_keep)
      for (int j = n_keep / KV_BLOCK; j <= (n_new - 1) / KV_BLOCK; ++j) need += row[j] < 0 || refcnt_[row[j]] > 1;
    if (need > free_blocks_.size()) throw std::runtime_error("paged KV: pool exhausted");
  }
  HIP_CHECK(hipSetDevice(cfg_.device));
  TraceRange tr("aios.shift_context");
  kv_prepare_write(slot, n_keep, n_new);
  kv_sync(0);
  if (n_new > n_keep) {
    KvShiftArgs a;
    std::memset(&a, 0, sizeof(a));
    a.k_cache = k_cache_; a.v_cache = v_cache_; a.layer_elems = layer_kv_elems_;
    a.block_table = d_bt_; a.max_blocks = kv_maxb_; a.slot = slot;
    a.n_layers = cfg_.n_layers; a.n_kv_heads = cfg_.n_kv_heads; a.head_dim = cfg_.head_dim;
    a.n_tokens = n_tokens; a.n_keep = n_keep; a.n_discard = n_discard;
    a.rope_cs = rope_cs_; a.rope_rows = cfg_.max_ctx; a.rope_neox = cfg_.rope_neox; a.kv_fp8 = cfg_.kv_fp8;
    if (cfg_.kv_fp8) {
      if (!d_shift_kscale_) d_shift_kscale_ = (float*)dmalloc((size_t)cfg_.n_layers * 4);
      std::vector<float> ks(cfg_.n_layers);
      for (int l = 0; l < cfg_.n_layers; ++l) ks[l] = kv_scale_[2 * l];
      HIP_CHECK(hipMemcpyAsync(d_shift_kscale_, ks.data(), ks.size() * 4, hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));  // (ks is pageable and leaves scope)
      a.k_scale = d_shift_kscale_;
    }
    launch_kv_shift(a, stream_);
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  for (int j = (n_new + KV_BLOCK - 1) / KV_BLOCK; j < kv_maxb_; ++j) {
    kv_unref(row[j]);
    row[j] = -1;
  }
  // decode rows of the slot: their host positions are not beyond the new length (advance_rows maps from there)
  for (size_t b = 0; b < row_slots_.size(); ++b)
    if (row_slots_[b] == slot) row_pos_[b] = std::min(row_pos_[b], n_new);
  bt_dirty_ = true;
  kv_sync((int)std::min(row_slots_.size(), (size_t)cfg_.max_batch));
  return n_new;
}

// ---- KV snapshots ------------------------------------------------------------------------------
size_t Engine::kv_snapshot_bytes(int n_tokens) const {
  return (size_t)cfg_.n_layers * 2 * cfg_.n_kv_heads * (size_t)std::max(n_tokens, 0) * cfg_.head_dim * kv_es_;
}

void Engine::snap_check(const char* who, int slot, int n_tokens, size_t bytes) const {
  const std::string w(who);
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (cfg_.tp_size > 1) throw std::runtime_error(w + ": not available on a tensor-parallel engine");
  if (pipe_sampled_) throw std::runtime_error(w + ": a pipelined step is in flight");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error(w + ": bad slot");
  if (n_tokens < 1 || n_tokens > cfg_.max_ctx) throw std::runtime_error(w + ": n_tokens out of range");
  if (bytes != kv_snapshot_bytes(n_tokens))
    throw std::runtime_error(w + ": payload of " + std::to_string(bytes) + " bytes, " + std::to_string(n_tokens) +
                             " tokens are " + std::to_string(kv_snapshot_bytes(n_tokens)));
}

void Engine::snap_reserve(size_t layer_bytes) {
  for (auto& e : snap_ev_)
    if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (layer_bytes <= snap_cap_) return;
  HIP_CHECK(hipStreamSynchronize(stream_));
  if (snap_dev_) HIP_CHECK(hipFree(snap_dev_));
  snap_dev_ = nullptr;
  for (auto& h : snap_host_) {
    if (h) HIP_CHECK(hipHostFree(h));
    h = nullptr;
  }
  snap_cap_ = 0;
  HIP_CHECK(hipMalloc(&snap_dev_, layer_bytes));
  for (auto& h : snap_host_) HIP_CHECK(hipHostMalloc(&h, layer_bytes, hipHostMallocDefault));
  snap_cap_ = layer_bytes;
}

void Engine::snap_launch(int slot, int layer, int n_tokens, bool unpack) {
  KvSnapArgs a;
  std::memset(&a, 0, sizeof(a));
  a.k_cache = k_cache_; a.v_cache = v_cache_; a.layer_bytes = layer_kv_elems_ * kv_es_;
  a.buf = snap_dev_; a.block_table = d_bt_; a.max_blocks = kv_maxb_; a.n_blocks = kv_nblocks_; a.slot = slot;
  a.layer0 = layer; a.n_layers = 1; a.n_kv_heads = cfg_.n_kv_heads; a.head_dim = cfg_.head_dim;
  a.n_tokens = n_tokens; a.elem_bytes = kv_es_; a.unpack = unpack ? 1 : 0;
  launch_kv_snapshot(a, stream_);
}

void Engine::kv_save(int slot, int n_tokens, void* out, size_t out_bytes) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  snap_check("kv_save", slot, n_tokens, out_bytes);
  if (!out) throw std::runtime_error("kv_save: null buffer");
  HIP_CHECK(hipSetDevice(cfg_.device));
  TraceRange tr("aios.kv_save");
  const size_t lb = out_bytes / cfg_.n_layers;  // one layer's K and V
  snap_reserve(lb);
  kv_sync(0);  // (the device table is the host's)
  // layer l: pack into the device staging, copy to pinned buffer l % 2; the host copies layer l - 1 out of the
  // other pinned buffer meanwhile.  The stream orders the staging's reuse; the host's own order a pinned buffer's.
  auto drain = [&](int l) {
    HIP_CHECK(hipEventSynchronize(snap_ev_[l & 1]));
    std::memcpy((char*)out + (size_t)l * lb, snap_host_[l & 1], lb);
  };
  for (int l = 0; l < cfg_.n_layers; ++l) {
    snap_launch(slot, l, n_tokens, false);
    HIP_CHECK(hipMemcpyAsync(snap_host_[l & 1], snap_dev_, lb, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(snap_ev_[l & 1], stream_));
    if (l > 0) drain(l - 1);
  }
  drain(cfg_.n_layers - 1);
}

void Engine::kv_restore(int slot, const void* data, size_t data_bytes, int n_tokens) {
  const CuScope cu_scope(cus_);  // (grids sized to this engine's CU mask)
  snap_check("kv_restore", slot, n_tokens, data_bytes);
  if (!data) throw std::runtime_error("kv_restore: null buffer");
  int* row = bt_.data() + (size_t)slot * kv_maxb_;
  const int nb = (n_tokens + KV_BLOCK - 1) / KV_BLOCK;
  {
    // the blocks kv_prepare_write will take, counted first: a throw half way would leave the tables changed
    size_t need = 0;
    for (int j = 0; j < nb; ++j) need += row[j] < 0 || refcnt_[row[j]] > 1;
    if (need > free_blocks_.size()) throw std::runtime_error("paged KV: pool exhausted");
  }
  HIP_CHECK(hipSetDevice(cfg_.device));
  TraceRange tr("aios.kv_restore");
  const size_t lb = data_bytes / cfg_.n_layers;
  snap_reserve(lb);  // (may throw: nothing has changed yet)
  kv_prepare_write(slot, 0, n_tokens);
  for (int j = nb; j < kv_maxb_; ++j) {
    kv_unref(row[j]);
    row[j] = -1;
  }
  bt_dirty_ = true;
  kv_sync(0);
  for (int l = 0; l < cfg_.n_layers; ++l) {
    if (l >= 2) HIP_CHECK(hipEventSynchronize(snap_ev_[l & 1]));  // this pinned buffer's last upload is done
    std::memcpy(snap_host_[l & 1], (const char*)data + (size_t)l * lb, lb);
    HIP_CHECK(hipMemcpyAsync(snap_dev_, snap_host_[l & 1], lb, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipEventRecord(snap_ev_[l & 1], stream_));
    snap_launch(slot, l, n_tokens, true);
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  // decode rows of the slot: their host positions are not beyond the restored length (advance_rows maps from there)
  for (size_t b = 0; b < row_slots_.size(); ++b)
    if (row_slots_[b] == slot) row_pos_[b] = std::min(row_pos_[b], n_tokens);
  bt_dirty_ = true;
  kv_sync((int)std::min(row_slots_.size(), (size_t)cfg_.max_batch));
}

std::vector<int> Engine::block_table(int slot) const {
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("block_table: bad slot");
  return std::vector<int>(bt_.begin() + (size_t)slot * kv_maxb_, bt_.begin() + (size_t)(slot + 1) * kv_maxb_);
}

std::vector<uint8_t> Engine::kv_read(int slot, int n_tokens) const {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (slot < 0 || slot >= cfg_.max_slots) throw std::runtime_error("kv_read: bad slot");
  if (n_tokens < 0 || n_tokens > cfg_.max_ctx) throw std::runtime_error("kv_read: token count out of range");
  HIP_CHECK(hipSetDevice(cfg_.device));
  HIP_CHECK(hipStreamSynchronize(stream_));
  const size_t row = (size_t)cfg_.head_dim * kv_es_;                 // one position of one head, bytes
  const size_t blk = (size_t)cfg_.n_kv_heads * KV_BLOCK * row;       // one block of one pool, bytes
  std::vector<uint8_t> out((size_t)cfg_.n_layers * 2 * cfg_.n_kv_heads * n_tokens * row);
  uint8_t* o = out.data();
  for (int l = 0; l < cfg_.n_layers; ++l)
    for (bf16_t* base : {k_cache_, v_cache_}) {
      const char* lb = (const char*)kv_layer(base, l);
      for (int h = 0; h < cfg_.n_kv_heads; ++h)
        for (int t0 = 0; t0 < n_tokens; t0 += KV_BLOCK) {
          const int b = bt_[(size_t)slot * kv_maxb_ + t0 / KV_BLOCK];
          const size_t n = (size_t)std::min(KV_BLOCK, n_tokens - t0) * row;
          const char* src = lb + (size_t)(b < 0 ? kv_nblocks_ : b) * blk + (size_t)h * KV_BLOCK * row;
          HIP_CHECK(hipMemcpyAsync(o, src, n, hipMemcpyDeviceToHost, stream_));
          o += n;
        }
    }
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

std::vector<int> Engine::kv_device_tables(int B) const {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (B < 0 || B > cfg_.max_batch) throw std::runtime_error("kv_device_tables: rows out of range");
  HIP_CHECK(hipSetDevice(cfg_.device));
  HIP_CHECK(hipStreamSynchronize(stream_));
  const size_t ns = bt_.size(), nr = (size_t)B * kv_maxb_;
  std::vector<int> out(ns + nr);
  HIP_CHECK(hipMemcpyAsync(out.data(), d_bt_, ns * 4, hipMemcpyDeviceToHost, stream_));
  if (nr) HIP_CHECK(hipMemcpyAsync(out.data() + ns, d_row_bt_, nr * 4, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

std::vector<uint8_t> Engine::kv_read_block(int block) const {
  if (!finalized_) throw std::runtime_error("engine not finalized");
  if (block < 0 || block > kv_nblocks_) throw std::runtime_error("kv_read_block: bad block");
  HIP_CHECK(hipSetDevice(cfg_.device));
  HIP_CHECK(hipStreamSynchronize(stream_));
  const size_t blk = (size_t)cfg_.n_kv_heads * KV_BLOCK * cfg_.head_dim * kv_es_;
  std::vector<uint8_t> out((size_t)cfg_.n_layers * 2 * blk);
  uint8_t* o = out.data();
  for (int l = 0; l < cfg_.n_layers; ++l)
    for (bf16_t* base : {k_cache_, v_cache_}) {
      HIP_CHECK(hipMemcpyAsync(o, (const char*)kv_layer(base, l) + (size_t)block * blk, blk, hipMemcpyDeviceToHost, stream_));
      o += blk;
    }
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

}  // namespace aios
