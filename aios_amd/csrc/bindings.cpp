// pybind11 bindings: the Engine (runtime) plus raw-pointer op entry points used by the kernel
// numerics tests (torch tensors pass data_ptr() and torch.cuda.current_stream().cuda_stream).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "comm.h"
#include "rccl_comm.h"
#include "engine.h"
#include "gemv_desc.h"
#include "gemv_plan.h"
#include "grammar.h"
#include "ops.h"

namespace py = pybind11;
using namespace aios;

namespace aios {
double bench_launch_chain(int n_kernels, int blocks, int use_graph, int reps);
double bench_stream_read(size_t bytes, int nbuf, int wg_per_cu, int u, int threads, int reps);
double bench_stream_read_part(size_t bytes, int nbuf, int mode, int threads, int reps);
}

namespace {

hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// split-K workspace for GEMM calls from Python (tests / tools): grown on demand, never freed;
// tickets zeroed once (the kernel's last arriver re-arms them)
struct GemmWs {
  float* ws = nullptr;
  size_t bytes = 0;
  int* cnt = nullptr;
  int cnt_len = 0;
};
GemmWs& gemm_ws(int M, int N) {
  static GemmWs g;
  const size_t need = gemm_skinny_ws_bytes(std::min(M, 64), N);
  const int need_cnt = gemm_skinny_cnt_len(N);
  if (need > g.bytes) {
    HIP_CHECK(hipDeviceSynchronize());
    if (g.ws) HIP_CHECK(hipFree(g.ws));
    HIP_CHECK(hipMalloc(&g.ws, need));
    g.bytes = need;
  }
  if (need_cnt > g.cnt_len) {
    HIP_CHECK(hipDeviceSynchronize());
    if (g.cnt) HIP_CHECK(hipFree(g.cnt));
    HIP_CHECK(hipMalloc(&g.cnt, need_cnt * 4));
    HIP_CHECK(hipMemset(g.cnt, 0, need_cnt * 4));
    g.cnt_len = need_cnt;
  }
  return g;
}

struct PyQMatrix;
// GemmQArgs from the arguments gemm_q / gemm_route / gemm_skinny_ntile share; kw: every other field by
// name (device pointers as integers), an unknown name throws
void gemm_q_args(GemmQArgs& a, const std::vector<PyQMatrix*>& segs, int lda, int M, int ldc, int epi, int ksplit,
                 const py::kwargs& kw);

// Owning device matrix in the repacked layout (tests / tools)
struct PyQMatrix {
  QWeight w{};
  void* buf = nullptr;
  size_t bytes = 0;
  PyQMatrix(int qt, int rows, int cols, py::buffer raw) {
    py::buffer_info bi = raw.request();
    const size_t nbytes = (size_t)bi.size * bi.itemsize;
    // engine-less allocation mirroring Engine::alloc_qmat
    EngineConfig cfg;
    cfg.n_layers = 0;
    (void)cfg;
    const int be = (qt == QT_Q4_K || qt == QT_Q5_K || qt == QT_Q6_K) ? 256 : ((qt == QT_F16 || qt == QT_BF16) ? 1 : 32);
    const size_t nb = (size_t)rows * (cols / be);
    size_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    switch (qt) {
      case QT_Q4_K: s0 = nb * 128; s1 = nb * 16; break;
      case QT_Q5_K: s0 = nb * 128; s1 = nb * 16; s2 = nb * 32; break;
      case QT_Q6_K: s0 = nb * 128; s1 = nb * 64; s2 = nb * 16; s3 = nb * 2; break;
      case QT_Q4_0: s0 = nb * 16; s1 = nb * 2; break;
      case QT_Q8_0: s0 = nb * 32; s1 = nb * 2; break;
      case QT_F16:
      case QT_BF16: s0 = nb * 2; break;
      default: throw std::runtime_error("QMatrix: unsupported type");
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o1 = al(s0), o2 = o1 + al(s1), o3 = o2 + al(s2);
    bytes = o3 + al(s3) + 64;
    HIP_CHECK(hipMalloc(&buf, bytes));
    uint8_t* base = (uint8_t*)buf;
    w.qtype = qt;
    w.rows = rows;
    w.cols = cols;
    w.p0 = base;
    w.p1 = s1 ? base + o1 : nullptr;
    w.p2 = s2 ? base + o2 : nullptr;
    w.p3 = s3 ? base + o3 : nullptr;
    void* staging = nullptr;
    HIP_CHECK(hipMalloc(&staging, nbytes));
    HIP_CHECK(hipMemcpy(staging, bi.ptr, nbytes, hipMemcpyHostToDevice));
    if (qt == QT_F16 || qt == QT_BF16) HIP_CHECK(hipMemcpy(buf, staging, nbytes, hipMemcpyDeviceToDevice));
    else launch_repack(qt, staging, nb, w, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipFree(staging));
  }
  ~PyQMatrix() {
    if (buf) hipFree(buf);
  }
};

void gemm_q_args(GemmQArgs& a, const std::vector<PyQMatrix*>& segs, int lda, int M, int ldc, int epi, int ksplit,
                 const py::kwargs& kw) {
  std::memset(&a, 0, sizeof(a));
  if (segs.empty() || segs.size() > 3) throw std::runtime_error("gemm_q: 1..3 segments");
  a.lda = lda; a.nseg = (int)segs.size();
  int n0 = 0;
  for (int s = 0; s < a.nseg; ++s) { a.seg[s] = segs[s]->w; a.seg_n0[s] = n0; n0 += segs[s]->w.rows; }
  a.M = M; a.N = n0; a.K = segs[0]->w.cols; a.ldc = ldc; a.epi = epi; a.ksplit = ksplit;
  a.kv_inv_k = a.kv_inv_v = 1.f;
  for (auto kv : kw) {
    const std::string k = py::cast<std::string>(kv.first);
    auto ptr = [&]() { return py::cast<uintptr_t>(kv.second); };
    int* fi = k == "col0" ? &a.col0 : k == "head_dim" ? &a.head_dim : k == "q_dim" ? &a.q_dim : k == "kv_dim" ? &a.kv_dim
            : k == "n_kv_heads" ? &a.n_kv_heads : k == "max_ctx" ? &a.max_ctx : k == "kv_fp8" ? &a.kv_fp8
            : k == "nrm_parts" ? &a.nrm_parts : nullptr;
    float* ff = k == "kv_inv_k" ? &a.kv_inv_k : k == "kv_inv_v" ? &a.kv_inv_v : k == "nrm_eps" ? &a.nrm_eps : nullptr;
    if (fi) *fi = py::cast<int>(kv.second);
    else if (ff) *ff = py::cast<float>(kv.second);
    else if (k == "rope_cs") a.rope_cs = (const float2*)ptr();
    else if (k == "pos") a.pos = (const int*)ptr();
    else if (k == "slot") a.slot = (const int*)ptr();
    else if (k == "block_table") a.block_table = (const int*)ptr();
    else if (k == "q_out") a.q_out = (float*)ptr();
    else if (k == "k_cache") a.k_cache = (bf16_t*)ptr();
    else if (k == "v_cache") a.v_cache = (bf16_t*)ptr();
    else if (k == "nrm_g") a.nrm_g = (const float*)ptr();
    else if (k == "nrm_out16") a.nrm_out16 = (bf16_t*)ptr();
    else if (k == "nrm_part") a.nrm_part = (float*)ptr();
    else if (k == "nrm_in") a.nrm_in = (const float*)ptr();
    else throw std::runtime_error("gemm_q: unknown argument " + k);
  }
}

}  // namespace

PYBIND11_MODULE(_engine, m) {
  m.doc() = "aiOS-MI355X native inference engine (gfx950 HIP kernels + C++ runtime)";
  m.attr("QT_F32") = (int)QT_F32;
  m.attr("QT_F16") = (int)QT_F16;
  m.attr("QT_BF16") = (int)QT_BF16;
  m.attr("QT_Q4_0") = (int)QT_Q4_0;
  m.attr("QT_Q8_0") = (int)QT_Q8_0;
  m.attr("QT_Q4_K") = (int)QT_Q4_K;
  m.attr("QT_Q5_K") = (int)QT_Q5_K;
  m.attr("QT_Q6_K") = (int)QT_Q6_K;
  m.attr("EPI_STORE") = (int)EPI_STORE;
  m.attr("EPI_RESID") = (int)EPI_RESID;
  m.attr("EPI_SWIGLU") = (int)EPI_SWIGLU;
  m.attr("EPI_QKV") = (int)EPI_QKV;
  m.attr("KV_BLOCK") = KV_BLOCK;
  m.attr("ATTN_CHUNK") = (int)ATTN_CHUNK;

  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
  });
  m.def("device_name", [](int dev) {
    hipDeviceProp_t p;
    HIP_CHECK(hipGetDeviceProperties(&p, dev));
    return std::string(p.name) + " / " + p.gcnArchName;
  });
  m.def("synchronize", []() { HIP_CHECK(hipDeviceSynchronize()); });
  m.def("resid_norm_parts", &resid_norm_parts, py::arg("d"));

  py::class_<EngineConfig>(m, "EngineConfig")
      .def(py::init<>())
      .def_readwrite("name", &EngineConfig::name)
      .def_readwrite("vocab_size", &EngineConfig::vocab_size)
      .def_readwrite("d_model", &EngineConfig::d_model)
      .def_readwrite("n_layers", &EngineConfig::n_layers)
      .def_readwrite("n_heads", &EngineConfig::n_heads)
      .def_readwrite("n_kv_heads", &EngineConfig::n_kv_heads)
      .def_readwrite("head_dim", &EngineConfig::head_dim)
      .def_readwrite("d_ff", &EngineConfig::d_ff)
      .def_readwrite("rope_theta", &EngineConfig::rope_theta)
      .def_readwrite("rope_neox", &EngineConfig::rope_neox)
      .def_readwrite("norm_eps", &EngineConfig::norm_eps)
      .def_readwrite("max_ctx", &EngineConfig::max_ctx)
      .def_readwrite("max_slots", &EngineConfig::max_slots)
      .def_readwrite("max_batch", &EngineConfig::max_batch)
      .def_readwrite("tie_embeddings", &EngineConfig::tie_embeddings)
      .def_readwrite("qk_norm", &EngineConfig::qk_norm)
      .def_readwrite("qkv_bias", &EngineConfig::qkv_bias)
      .def_readwrite("act_q8", &EngineConfig::act_q8)
      .def_readwrite("tp_rank", &EngineConfig::tp_rank)
      .def_readwrite("tp_size", &EngineConfig::tp_size)
      .def_readwrite("vocab_parallel", &EngineConfig::vocab_parallel)
      .def_readwrite("device", &EngineConfig::device)
      .def_readwrite("cu_mask", &EngineConfig::cu_mask)
      .def_readwrite("kv_fp8", &EngineConfig::kv_fp8)
      .def_readwrite("stream_priority", &EngineConfig::stream_priority);

  py::class_<Engine>(m, "Engine")
      .def(py::init<const EngineConfig&>())
      .def("set_tensor",
           [](Engine& e, const std::string& name, int qt, int rows, int cols, py::buffer raw) {
             py::buffer_info bi = raw.request();
             const size_t nbytes = (size_t)bi.size * bi.itemsize;
             py::gil_scoped_release nogil;
             e.set_tensor(name, qt, rows, cols, bi.ptr, nbytes);
           })
      .def("init_random", &Engine::init_random, py::call_guard<py::gil_scoped_release>())
      .def("finalize", &Engine::finalize, py::call_guard<py::gil_scoped_release>())
      .def("missing_tensors", &Engine::missing_tensors)
      .def("weight_type_summary", &Engine::weight_type_summary)
      .def_property_readonly("ready", &Engine::ready)
      .def_property_readonly("weight_bytes", &Engine::weight_bytes)
      .def_property_readonly("kv_bytes", &Engine::kv_bytes)
      .def_property_readonly("workspace_bytes", &Engine::workspace_bytes)
      .def_property_readonly("config", &Engine::config)
      .def("prefill",
           [](Engine& e, int slot, const std::vector<int>& tokens, int start_pos, bool want_logits) {
             std::vector<float> out;
             {
               py::gil_scoped_release nogil;
               out = e.prefill(slot, tokens, start_pos, want_logits);
             }
             return py::array_t<float>(out.size(), out.data());
           },
           py::arg("slot"), py::arg("tokens"), py::arg("start_pos") = 0, py::arg("want_logits") = true)
      .def("embed_prefill",
           [](Engine& e, int slot, const std::vector<int>& tokens, int start_pos, int pooling, bool final) -> py::object {
             // final: the [d] unit vector, or for pooling 0 (none) the [tokens][d] normed rows; else an empty array
             std::vector<float> out;
             {
               py::gil_scoped_release nogil;
               out = e.embed_prefill(slot, tokens, start_pos, pooling, final);
             }
             py::array_t<float> a(out.size(), out.data());
             if (final && pooling == EMBED_NONE)
               return a.reshape({(py::ssize_t)e.embed_tokens(), (py::ssize_t)e.config().d_model});
             return a;
           },
           py::arg("slot"), py::arg("tokens"), py::arg("start_pos") = 0, py::arg("pooling") = (int)EMBED_MEAN,
           py::arg("final") = true)
      .def("embed_tokens", &Engine::embed_tokens)
      .def("score_prefill",
           [](Engine& e, int slot, const std::vector<int>& tokens, int start_pos, int next_token, int top_n,
              bool want_logits) {
             // dict of numpy arrays: lp, best_lp (float32 [T]), rank, best (int32 [T]) and, when top_n > 0,
             // ids (int32 [T][top_n]) and lps (float32 [T][top_n])
             Engine::PromptScores r;
             {
               py::gil_scoped_release nogil;
               r = e.score_prefill(slot, tokens, start_pos, next_token, top_n, want_logits);
             }
             const py::ssize_t T = (py::ssize_t)r.lp.size();
             py::dict d;
             d["lp"] = py::array_t<float>(T, r.lp.data());
             d["best_lp"] = py::array_t<float>(T, r.best_lp.data());
             d["rank"] = py::array_t<int>(T, r.rank.data());
             d["best"] = py::array_t<int>(T, r.best.data());
             if (top_n > 0) {
               d["ids"] = py::array_t<int>({T, (py::ssize_t)top_n}, r.ids.data());
               d["lps"] = py::array_t<float>({T, (py::ssize_t)top_n}, r.lps.data());
             }
             return d;
           },
           py::arg("slot"), py::arg("tokens"), py::arg("start_pos") = 0, py::arg("next_token") = -1,
           py::arg("top_n") = 0, py::arg("want_logits") = false)
      .def("score_group_rows", &Engine::score_group_rows)
      .def("decode",
           [](Engine& e, const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
              const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed, py::bytes mask,
              const std::vector<float>& top_p, const std::vector<uint64_t>& seeds) {
             std::string m = mask;  // packed allowed-token bitmask, B rows of ceil(V/8) bytes (or empty)
             std::vector<uint8_t> mv(m.begin(), m.end());
             py::gil_scoped_release nogil;
             return e.decode(slots, tokens, pos, temperature, top_k, seed, mv, top_p, seeds);
           },
           py::arg("slots"), py::arg("tokens"), py::arg("pos"), py::arg("temperature") = std::vector<float>{},
           py::arg("top_k") = std::vector<int>{}, py::arg("seed") = 0, py::arg("mask") = py::bytes(),
           py::arg("top_p") = std::vector<float>{}, py::arg("seeds") = std::vector<uint64_t>{})
      .def("spec_decode",
           [](Engine& e, int slot, const std::vector<int>& tokens, int pos0, float temperature, int top_k, float top_p,
              uint64_t seed, py::bytes masks) {
             // (accepted, tokens): the accepted drafts and the accepted + 1 emitted tokens
             std::string m = masks;  // R rows of ceil(V/8) bytes (or empty)
             std::vector<uint8_t> mv(m.begin(), m.end());
             Engine::SpecResult r;
             {
               py::gil_scoped_release nogil;
               r = e.spec_decode(slot, tokens, pos0, temperature, top_k, top_p, seed, mv);
             }
             return py::make_tuple(r.accepted, r.tokens);
           },
           py::arg("slot"), py::arg("tokens"), py::arg("pos0"), py::arg("temperature") = 0.f, py::arg("top_k") = 0,
           py::arg("top_p") = 1.f, py::arg("seed") = 0, py::arg("masks") = py::bytes())
      .def("spec_decode_multi",
           [](Engine& e, const std::vector<int>& slots, const std::vector<std::vector<int>>& tokens,
              const std::vector<int>& pos0, const std::vector<float>& temperature, const std::vector<int>& top_k,
              const std::vector<float>& top_p, const std::vector<uint64_t>& seeds, py::bytes masks) {
             // one (accepted, tokens) per sequence; empty temperature / top_k / top_p / seeds: greedy, 1.0, 0
             const size_t n = slots.size();
             std::string m = masks;  // Rt rows of ceil(V/8) bytes (or empty), in segment order
             std::vector<uint8_t> mv(m.begin(), m.end());
             std::vector<Engine::SpecResult> r;
             {
               py::gil_scoped_release nogil;
               r = e.spec_decode_multi(slots, tokens, pos0, temperature.empty() ? std::vector<float>(n, 0.f) : temperature,
                                       top_k.empty() ? std::vector<int>(n, 0) : top_k,
                                       top_p.empty() ? std::vector<float>(n, 1.f) : top_p,
                                       seeds.empty() ? std::vector<uint64_t>(n, 0) : seeds, mv);
             }
             py::list out;
             for (const auto& x : r) out.append(py::make_tuple(x.accepted, x.tokens));
             return out;
           },
           py::arg("slots"), py::arg("tokens"), py::arg("pos0"), py::arg("temperature") = std::vector<float>{},
           py::arg("top_k") = std::vector<int>{}, py::arg("top_p") = std::vector<float>{},
           py::arg("seeds") = std::vector<uint64_t>{}, py::arg("masks") = py::bytes())
      .def("decode_submit",
           [](Engine& e, const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
              const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
              const std::vector<float>& top_p, const std::vector<uint64_t>& seeds) {
             py::gil_scoped_release nogil;
             e.decode_submit(slots, tokens, pos, temperature, top_k, seed, top_p, seeds);
           },
           py::arg("slots"), py::arg("tokens"), py::arg("pos"), py::arg("temperature") = std::vector<float>{},
           py::arg("top_k") = std::vector<int>{}, py::arg("seed") = 0, py::arg("top_p") = std::vector<float>{},
           py::arg("seeds") = std::vector<uint64_t>{})
      .def("decode_sample",
           [](Engine& e, py::bytes mask) {
             std::string m = mask;
             std::vector<uint8_t> mv(m.begin(), m.end());
             py::gil_scoped_release nogil;
             e.decode_sample(mv);
           },
           py::arg("mask") = py::bytes())
      .def("decode_collect", &Engine::decode_collect, py::call_guard<py::gil_scoped_release>())
      .def("set_sample_processors", &Engine::set_sample_processors, py::arg("min_p"), py::arg("repeat_penalty"),
           py::arg("presence_penalty"), py::arg("frequency_penalty"), py::arg("recent"),
           py::arg("bias_ids") = std::vector<std::vector<int>>{},
           py::arg("bias_vals") = std::vector<std::vector<float>>{}, py::call_guard<py::gil_scoped_release>())
      .def("set_logprobs", &Engine::set_logprobs, py::arg("top_n"))
      .def("grammar_vocab",
           [](Engine& e, const std::vector<py::bytes>& toks, const std::vector<int>& eos_ids) {
             std::vector<std::string> t;
             t.reserve(toks.size());
             for (auto& b : toks) t.push_back(std::string(b));
             py::gil_scoped_release nogil;
             e.grammar_vocab(t, eos_ids);
           },
           py::arg("tokens"), py::arg("eos_ids"))
      .def("grammar_load",
           [](Engine& e, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> byte_class,
              py::array_t<uint16_t, py::array::c_style | py::array::forcecast> trans,
              py::array_t<uint8_t, py::array::c_style | py::array::forcecast> accept) {
             if (byte_class.ndim() != 1 || byte_class.shape(0) != 256 || trans.ndim() != 2 || accept.ndim() != 1 ||
                 accept.shape(0) != trans.shape(0))
               throw std::runtime_error("grammar_load: byte_class[256], trans[S][C], accept[S] expected");
             const uint8_t* bc = byte_class.data();
             const uint16_t* tr = trans.data();
             const uint8_t* ac = accept.data();
             const int S = (int)trans.shape(0), C = (int)trans.shape(1);
             py::gil_scoped_release nogil;
             return e.grammar_load(bc, tr, ac, S, C);
           },
           py::arg("byte_class"), py::arg("trans"), py::arg("accept"))
      .def("grammar_free", &Engine::grammar_free, py::arg("gid"), py::call_guard<py::gil_scoped_release>())
      .def("grammar_masks",
           [](Engine& e, int gid, const std::vector<int>& states) {
             std::vector<uint8_t> m;
             {
               py::gil_scoped_release nogil;
               m = e.grammar_masks(gid, states);
             }
             return py::bytes((const char*)m.data(), m.size());
           },
           py::arg("gid"), py::arg("states"))
      .def("set_grammar_rows", &Engine::set_grammar_rows, py::arg("gids"), py::arg("states"))
      .def_property_readonly("grammars_loaded", &Engine::grammars_loaded)
      .def("last_logprobs",
           [](const Engine& e) -> py::object {
             // () when the last sampler launch had none staged, else (token_lp [B], ids [B][LOGPROB_MAX_TOP],
             // lps [B][LOGPROB_MAX_TOP]); rows that were off: NaN, -1, -inf
             const Engine::Logprobs r = e.last_logprobs();
             if (r.top_n.empty()) return py::tuple(0);
             const py::ssize_t B = (py::ssize_t)r.top_n.size();
             py::array_t<float> lp(B);
             py::array_t<int> ids({B, (py::ssize_t)LOGPROB_MAX_TOP});
             py::array_t<float> lps({B, (py::ssize_t)LOGPROB_MAX_TOP});
             std::memcpy(lp.mutable_data(), r.token_lp.data(), r.token_lp.size() * 4);
             std::memcpy(ids.mutable_data(), r.ids.data(), r.ids.size() * 4);
             std::memcpy(lps.mutable_data(), r.lps.data(), r.lps.size() * 4);
             return py::make_tuple(lp, ids, lps);
           })
      .def("sample_first",
           [](Engine& e, int pos, float temperature, int top_k, float top_p, uint64_t seed, py::bytes mask) {
             std::string m = mask;
             std::vector<uint8_t> mv(m.begin(), m.end());
             py::gil_scoped_release nogil;
             return e.sample_first(pos, temperature, top_k, top_p, seed, mv);
           },
           py::arg("pos"), py::arg("temperature") = 0.f, py::arg("top_k") = 0, py::arg("top_p") = 1.f,
           py::arg("seed") = 0, py::arg("mask") = py::bytes())
      .def("resample",
           [](Engine& e, int B, const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
              py::bytes mask, const std::vector<float>& top_p) {
             std::string m = mask;
             std::vector<uint8_t> mv(m.begin(), m.end());
             py::gil_scoped_release nogil;
             return e.resample(B, temperature, top_k, seed, mv, top_p);
           },
           py::arg("B"), py::arg("temperature") = std::vector<float>{}, py::arg("top_k") = std::vector<int>{},
           py::arg("seed") = 0, py::arg("mask") = py::bytes(), py::arg("top_p") = std::vector<float>{})
      .def("last_logits",
           [](Engine& e, int B) {
             std::vector<float> v;
             {
               py::gil_scoped_release nogil;
               v = e.last_logits(B);
             }
             py::array_t<float> a({(py::ssize_t)B, (py::ssize_t)e.config().vocab_size});
             std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
             return a;
           })
      .def("decode_loop_prepare", &Engine::decode_loop_prepare, py::call_guard<py::gil_scoped_release>())
      .def("decode_loop_run", &Engine::decode_loop_run, py::arg("B"), py::arg("n_steps"), py::arg("use_graph") = true,
           py::call_guard<py::gil_scoped_release>())
      .def("decode_loop_history", &Engine::decode_loop_history, py::call_guard<py::gil_scoped_release>())
      .def("synchronize", &Engine::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("reset_graphs", &Engine::reset_graphs)
      .def("copy_slot", &Engine::copy_slot, py::call_guard<py::gil_scoped_release>())
      .def("release_slot", &Engine::release_slot)
      .def("shift_context", &Engine::shift_context, py::call_guard<py::gil_scoped_release>(), py::arg("slot"),
           py::arg("n_tokens"), py::arg("n_keep"), py::arg("n_discard"))
      .def("kv_snapshot_bytes", &Engine::kv_snapshot_bytes, py::arg("n_tokens"))
      .def("kv_save",
           [](Engine& e, int slot, int n_tokens) {
             // the snapshot payload of a slot's first n_tokens positions, kv_read's bytes (written straight into
             // the bytes object: no second copy of the slot on the host either)
             // (an n_tokens out of range: no allocation by it, the engine's refusal instead)
             const size_t n = n_tokens <= e.config().max_ctx ? e.kv_snapshot_bytes(n_tokens) : 0;
             PyObject* o = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)n);
             if (!o) throw py::error_already_set();
             py::bytes out = py::reinterpret_steal<py::bytes>(o);
             char* p = PyBytes_AS_STRING(o);
             {
               py::gil_scoped_release nogil;
               e.kv_save(slot, n_tokens, p, n);
             }
             return out;
           },
           py::arg("slot"), py::arg("n_tokens"))
      .def("kv_restore",
           [](Engine& e, int slot, py::buffer data, int n_tokens) {
             py::buffer_info bi = data.request();
             const size_t n = (size_t)bi.size * bi.itemsize;
             if (bi.ndim > 1 || (bi.ndim == 1 && bi.strides[0] != bi.itemsize))
               throw std::runtime_error("kv_restore: data must be contiguous");
             py::gil_scoped_release nogil;
             e.kv_restore(slot, bi.ptr, n, n_tokens);
           },
           py::arg("slot"), py::arg("data"), py::arg("n_tokens"))
      .def("block_table", &Engine::block_table)
      .def("kv_read",
           [](const Engine& e, int slot, int n_tokens) {
             // raw cache bytes of a slot's first n_tokens positions: [layer][K, V][kv_head][token][head_dim]
             std::vector<uint8_t> v;
             {
               py::gil_scoped_release nogil;
               v = e.kv_read(slot, n_tokens);
             }
             return py::bytes((const char*)v.data(), v.size());
           },
           py::arg("slot"), py::arg("n_tokens"))
      .def("kv_read_block",
           [](const Engine& e, int block) {
             // one physical block of every layer: [layer][K, V][kv_head][KV_BLOCK][head_dim]
             std::vector<uint8_t> v;
             {
               py::gil_scoped_release nogil;
               v = e.kv_read_block(block);
             }
             return py::bytes((const char*)v.data(), v.size());
           },
           py::arg("block"))
      .def("kv_device_tables", &Engine::kv_device_tables, py::arg("B"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("kv_blocks_free", &Engine::kv_blocks_free)
      .def_property_readonly("kv_blocks_total", &Engine::kv_blocks_total)
      .def_property_readonly("norm_fused_parts", &Engine::norm_fused_parts)
      .def("capture_graphs", &Engine::capture_graphs, py::arg("max_b"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("stream", &Engine::stream_handle)
      .def_property_readonly("k_cache_ptr", &Engine::kv_cache_k)
      .def_property_readonly("v_cache_ptr", &Engine::kv_cache_v)
      .def("set_allreduce_ptr", [](Engine& e, uintptr_t fn, uintptr_t ctx) {
        e.set_allreduce(reinterpret_cast<AllReduceFn>(fn), reinterpret_cast<void*>(ctx));
      })
      .def("set_comm", [](Engine& e, XgmiComm& c) {
        // the comm must outlive the engine's use of it (the Python wrapper keeps a reference)
        e.set_allreduce(&XgmiComm::hook, &c);
        e.set_allgather(&XgmiComm::gather_hook, &c);
        e.set_allreduce_norm(&XgmiComm::norm_hook, &c);
        e.set_tp_fuse(c.fuse_ctx(), c.fuse_grid());
      })
      .def("set_comm", [](Engine& e, RcclComm& c) {
        e.set_allreduce(&RcclComm::hook, &c);
        e.set_allgather(&RcclComm::gather_hook, &c);
        e.set_allreduce_norm(&RcclComm::norm_hook, &c);
      })
      .def_property_readonly("vocab_parallel", &Engine::vocab_parallel)
      .def_property_readonly("tp_fused", &Engine::tp_fused)
      .def("tp_fuse_fits", &Engine::tp_fuse_fits)
      .def("set_kv_scales", &Engine::set_kv_scales)
      .def_property_readonly("kv_scales", &Engine::kv_scales)
      .def("calibrate_kv_scales", &Engine::calibrate_kv_scales, py::arg("tokens"), py::arg("headroom") = 2.f,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("kv_amax", &Engine::kv_amax)
      .def_property_readonly("kv_fp8", &Engine::kv_fp8)
      .def("disable_tp_fuse", &Engine::disable_tp_fuse);

  // ------------------------------------------------------------------ TP collectives (xGMI)
  py::class_<XgmiComm>(m, "XgmiComm")
      .def(py::init<int, int, int, size_t>(), py::arg("rank"), py::arg("world"), py::arg("device"),
           py::arg("cap_floats"))
      .def("ipc_handle", [](const XgmiComm& c) { return py::bytes(c.ipc_handle()); })
      .def("set_ranks_per_gpu", &XgmiComm::set_ranks_per_gpu)
      .def_property_readonly("fuse_grid", &XgmiComm::fuse_grid)
      .def_property_readonly("fuse_eligible", &XgmiComm::fuse_eligible)
      .def_property_readonly("uncached", &XgmiComm::uncached)
      .def("disable_fuse", &XgmiComm::disable_fuse)
      .def_property_readonly("fused", [](const XgmiComm& c) { return c.fuse_ctx() != nullptr; })
      // one batch-1 EPI_TP_RESID GEMV through this comm's fused context (the TP init self-test of the
      // O / down all-reduce epilogue): y[n] += sum over ranks of (W x)[n]; false = not launched (no
      // fused context, or the shape does not fit the stage) -- dry: only whether it would launch
      .def("fused_gemv",
           [](XgmiComm& c, PyQMatrix& w, uintptr_t x, uintptr_t y, uintptr_t st, bool dry) {
             if (!c.fuse_ctx()) return false;
             GemvArgs a;
             std::memset(&a, 0, sizeof(a));
             a.nseg = 1; a.seg[0] = w.w; a.N = w.w.rows; a.K = w.w.cols; a.B = 1;
             a.x = (const float*)x; a.ldx = a.K; a.y = (float*)y; a.ldy = a.N;
             a.epi = EPI_TP_RESID; a.act_q8 = 1; a.tp = c.fuse_ctx(); a.kernel_sel = 1; a.grid_cap = c.fuse_grid();
             a.dry = dry ? 1 : 0;
             return launch_gemv_tp_fused(a, S(st));
           },
           py::arg("w"), py::arg("x"), py::arg("y"), py::arg("stream") = 0, py::arg("dry") = false)
      .def("connect", [](XgmiComm& c, const std::vector<py::bytes>& hs) {
        std::vector<std::string> v;
        for (auto& h : hs) v.push_back(std::string(h));
        c.connect(v);
      })
      .def("allreduce", [](XgmiComm& c, uintptr_t data, size_t n, uintptr_t residual, uintptr_t st) {
        c.allreduce((float*)data, n, (float*)residual, S(st));
      }, py::arg("data"), py::arg("n"), py::arg("residual") = 0, py::arg("stream") = 0)
      .def("allreduce_norm",
           [](XgmiComm& c, uintptr_t data, int rows, int d, uintptr_t residual, uintptr_t g, uintptr_t out16, int ld16,
              uintptr_t part, int parts, uintptr_t st) {
             c.allreduce_norm((float*)data, rows, d, (float*)residual,
                              ResidNorm{(const float*)g, (bf16_t*)out16, ld16, (float*)part, parts}, S(st));
           },
           py::arg("data"), py::arg("rows"), py::arg("d"), py::arg("residual"), py::arg("g"), py::arg("out16"),
           py::arg("ld16"), py::arg("part"), py::arg("parts"), py::arg("stream") = 0)
      .def("allgather_cols", [](XgmiComm& c, uintptr_t data, int rows, int slice, int ld, uintptr_t st) {
        c.allgather_cols((float*)data, rows, slice, ld, S(st));
      }, py::arg("data"), py::arg("rows"), py::arg("slice"), py::arg("ld"), py::arg("stream") = 0)
      .def_property("two_shot_min", &XgmiComm::two_shot_min, &XgmiComm::set_two_shot_min)
      .def_property("call_wg", &XgmiComm::call_wg, &XgmiComm::set_call_wg)
      .def_property("bf16_payload", &XgmiComm::bf16_payload, &XgmiComm::set_bf16_payload)
      .def("error", &XgmiComm::error)
      .def("reset_error", &XgmiComm::reset_error)
      .def_property_readonly("rank", &XgmiComm::rank)
      .def_property_readonly("world", &XgmiComm::world)
      .def_property_readonly("capacity", &XgmiComm::capacity)
      .def_property_readonly("connected", &XgmiComm::connected);

  // ------------------------------------------------------------------ TP collectives (RCCL, dlopen'd)
  py::class_<RcclComm>(m, "RcclComm")
      // the id arrives as std::string (converted under the GIL); only the collective init runs
      // without it (ncclCommInitRank blocks until every rank has joined)
      .def(py::init([](int rank, int world, int device, const std::string& id) {
             py::gil_scoped_release nogil;
             return new RcclComm(rank, world, device, id);
           }),
           py::arg("rank"), py::arg("world"), py::arg("device"), py::arg("unique_id"))
      .def_static("unique_id", []() { return py::bytes(RcclComm::unique_id()); })
      .def_static("available", &RcclComm::available)
      .def("allreduce", [](RcclComm& c, uintptr_t data, size_t n, uintptr_t residual, uintptr_t st) {
        c.allreduce((float*)data, n, (float*)residual, S(st));
      }, py::arg("data"), py::arg("n"), py::arg("residual") = 0, py::arg("stream") = 0)
      .def("allreduce_norm",
           [](RcclComm& c, uintptr_t data, int rows, int d, uintptr_t residual, uintptr_t g, uintptr_t out16, int ld16,
              uintptr_t part, int parts, uintptr_t st) {
             c.allreduce_norm((float*)data, rows, d, (float*)residual,
                              ResidNorm{(const float*)g, (bf16_t*)out16, ld16, (float*)part, parts}, S(st));
           },
           py::arg("data"), py::arg("rows"), py::arg("d"), py::arg("residual"), py::arg("g"), py::arg("out16"),
           py::arg("ld16"), py::arg("part"), py::arg("parts"), py::arg("stream") = 0)
      .def("allgather_cols", [](RcclComm& c, uintptr_t data, int rows, int slice, int ld, uintptr_t st) {
        c.allgather_cols((float*)data, rows, slice, ld, S(st));
      }, py::arg("data"), py::arg("rows"), py::arg("slice"), py::arg("ld"), py::arg("stream") = 0)
      .def("error", &RcclComm::error)
      .def("reset_error", &RcclComm::reset_error)
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("world", &RcclComm::world);

  // ------------------------------------------------------------------ raw ops (tests / tools)
  py::class_<PyQMatrix>(m, "QMatrix")
      .def(py::init<int, int, int, py::buffer>())
      .def_property_readonly("qtype", [](const PyQMatrix& q) { return q.w.qtype; })
      .def_property_readonly("rows", [](const PyQMatrix& q) { return q.w.rows; })
      .def_property_readonly("cols", [](const PyQMatrix& q) { return q.w.cols; })
      .def_property_readonly("nbytes", [](const PyQMatrix& q) { return q.bytes; })
      .def("dequant_bf16", [](PyQMatrix& q, uintptr_t out, uintptr_t st) { launch_dequant_bf16(q.w, (void*)out, S(st)); })
      .def("get_rows", [](PyQMatrix& q, uintptr_t rows, int n, uintptr_t out, int ldo, uintptr_t st) {
        launch_get_rows(q.w, (const int*)rows, n, (float*)out, ldo, 1.f, S(st));
      })
      // get_rows + the per-step lookups of the batch-1 QKV epilogue (StepPrep, ops.h)
      .def("get_rows_step",
           [](PyQMatrix& q, uintptr_t rows, int n, uintptr_t out, int ldo, uintptr_t st, uintptr_t pos, uintptr_t slot,
              uintptr_t block_table, int maxb, uintptr_t rope_cs, int half, uintptr_t kv, uintptr_t rope) {
             const StepPrep sp{(const int*)pos, (const int*)slot, (const int*)block_table, maxb, (const float2*)rope_cs,
                               half, (int*)kv, (float2*)rope};
             launch_get_rows_step(q.w, (const int*)rows, n, (float*)out, ldo, 1.f, sp, S(st));
           },
           py::arg("rows"), py::arg("n"), py::arg("out"), py::arg("ldo"), py::arg("st"), py::arg("pos"),
           py::arg("slot") = 0, py::arg("block_table") = 0, py::arg("maxb") = 0, py::arg("rope_cs") = 0,
           py::arg("half") = 0, py::arg("kv") = 0, py::arg("rope") = 0)
      .def("fill_random", [](PyQMatrix& q, uint64_t seed, float amp) {
        fill_random_weight(q.w, seed, amp, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
      });

  // the load-time expansion of the formats no kernel streams (Engine::upload_qmat): n elements of raw
  // GGUF blocks staged on the device -> bf16 at out
  m.def("legacy_to_bf16",
        [](int qt, py::buffer raw, size_t n, uintptr_t out, uintptr_t st) {
          size_t be = 0, bb = 0;  // block elements / bytes
          switch (qt) {
            case QT_F32: be = 1; bb = 4; break;
            case QT_Q4_1: be = 32; bb = 20; break;
            case QT_Q5_0: be = 32; bb = 22; break;
            case QT_Q5_1: be = 32; bb = 24; break;
            case QT_IQ4_NL: be = 32; bb = 18; break;
            case QT_IQ4_XS: be = 256; bb = 136; break;
            case QT_Q2_K: be = 256; bb = 84; break;
            case QT_Q3_K: be = 256; bb = 110; break;
            default: throw std::runtime_error("legacy_to_bf16: not a load-time expanded type");
          }
          py::buffer_info bi = raw.request();
          const size_t nbytes = (size_t)bi.size * bi.itemsize;
          if (n % be || nbytes != n / be * bb) throw std::runtime_error("legacy_to_bf16: byte size does not match n");
          void* staging = nullptr;
          HIP_CHECK(hipMalloc(&staging, nbytes));
          HIP_CHECK(hipMemcpy(staging, bi.ptr, nbytes, hipMemcpyHostToDevice));
          launch_legacy_to_bf16(qt, staging, n, (void*)out, S(st));
          HIP_CHECK(hipStreamSynchronize(S(st)));
          HIP_CHECK(hipFree(staging));
        },
        py::arg("qtype"), py::arg("raw_bytes"), py::arg("n"), py::arg("out_ptr"), py::arg("stream"));
  m.def("gemv",
        [](std::vector<PyQMatrix*> segs, int B, uintptr_t x, int ldx, uintptr_t norm_w, float eps, uintptr_t y,
           int ldy, int epi, uintptr_t st, int force_v1, int act_q8, int tune_grid, int tune_u, int tune_ksplit, int tune_dbg,
           int kernel_sel, uintptr_t dbg_ts, uintptr_t x16, uintptr_t y16) {
          (void)tune_ksplit;  // (accepted and ignored: no kernel has a K-split decomposition)
          GemvArgs a;
          std::memset(&a, 0, sizeof(a));
          a.nseg = (int)segs.size();
          int r = 0;
          for (int s = 0; s < a.nseg; ++s) { a.seg[s] = segs[s]->w; a.seg_row0[s] = r; r += segs[s]->w.rows; }
          a.N = r; a.K = segs[0]->w.cols; a.B = B;
          a.x = (const float*)x; a.ldx = ldx; a.norm_w = (const float*)norm_w; a.eps = eps;
          a.y = (float*)y; a.ldy = ldy; a.epi = epi; a.force_v1 = force_v1; a.act_q8 = act_q8;
          a.tune_grid = tune_grid; a.tune_u = tune_u; a.tune_dbg = tune_dbg;
          a.kernel_sel = kernel_sel; a.dbg_ts = (unsigned long long*)dbg_ts;
          a.x16 = (const bf16_t*)x16; a.y16 = (bf16_t*)y16;  // bf16 input / SwiGLU output (hand-off kernels)
          launch_gemv(a, S(st));
        },
        py::arg("segs"), py::arg("B"), py::arg("x"), py::arg("ldx"), py::arg("norm_w"), py::arg("eps"), py::arg("y"),
        py::arg("ldy"), py::arg("epi"), py::arg("stream"), py::arg("force_v1") = 0, py::arg("act_q8") = 0,
        py::arg("tune_grid") = 0, py::arg("tune_u") = 0, py::arg("tune_ksplit") = 0, py::arg("tune_dbg") = 0,
        py::arg("kernel_sel") = 0, py::arg("dbg_ts") = 0, py::arg("x16") = 0, py::arg("y16") = 0);
  m.def("gemv_bf16_engine_fits",
        [](std::vector<PyQMatrix*> segs, int B, int epi) {
          GemvArgs a;
          std::memset(&a, 0, sizeof(a));
          a.nseg = (int)segs.size();
          int r = 0;
          for (int s = 0; s < a.nseg; ++s) { a.seg[s] = segs[s]->w; a.seg_row0[s] = r; r += segs[s]->w.rows; }
          a.N = r; a.K = segs[0]->w.cols; a.B = B; a.epi = epi;
          return gemv_bf16_engine_fits(a);
        },
        py::arg("segs"), py::arg("B"), py::arg("epi") = 0);
  m.def("gemv_qkv",
        [](std::vector<PyQMatrix*> segs, int B, uintptr_t x, int ldx, uintptr_t norm_w, float eps, uintptr_t q_out,
           uintptr_t bias, int head_dim, int n_heads, int n_kv_heads, int max_ctx, int rope_neox, float rope_base,
           uintptr_t pos, uintptr_t slot, uintptr_t k_cache, uintptr_t v_cache, uintptr_t st, int act_q8,
           uintptr_t block_table, uintptr_t rope_cs, int tune_grid, int kernel_sel) {
          GemvArgs a;
          std::memset(&a, 0, sizeof(a));
          a.nseg = (int)segs.size();
          int r = 0;
          for (int s = 0; s < a.nseg; ++s) { a.seg[s] = segs[s]->w; a.seg_row0[s] = r; r += segs[s]->w.rows; }
          a.N = r; a.K = segs[0]->w.cols; a.B = B;
          a.x = (const float*)x; a.ldx = ldx; a.norm_w = (const float*)norm_w; a.eps = eps;
          a.y = (float*)q_out; a.ldy = n_heads * head_dim; a.epi = EPI_QKV;
          a.bias = (const float*)bias; a.head_dim = head_dim; a.q_dim = n_heads * head_dim;
          a.kv_dim = n_kv_heads * head_dim; a.n_kv_heads = n_kv_heads; a.max_ctx = max_ctx;
          a.rope_neox = rope_neox; a.rope_base = rope_base; a.rope_cs = (const float2*)rope_cs; a.pos = (const int*)pos; a.slot = (const int*)slot;
          a.k_cache = (bf16_t*)k_cache; a.v_cache = (bf16_t*)v_cache; a.act_q8 = act_q8;
          a.block_table = (const int*)block_table;
          a.tune_grid = tune_grid;
          a.kernel_sel = kernel_sel;
          launch_gemv(a, S(st));
        },
        py::arg("segs"), py::arg("B"), py::arg("x"), py::arg("ldx"), py::arg("norm_w"), py::arg("eps"),
        py::arg("q_out"), py::arg("bias"), py::arg("head_dim"), py::arg("n_heads"), py::arg("n_kv_heads"),
        py::arg("max_ctx"), py::arg("rope_neox"), py::arg("rope_base"), py::arg("pos"), py::arg("slot"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("stream"), py::arg("act_q8") = 0,
        py::arg("block_table") = 0, py::arg("rope_cs") = 0, py::arg("tune_grid") = 0, py::arg("kernel_sel") = 0);
  m.def("attn_decode",
        [](uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t seq_len, uintptr_t slot, int B, int H, int Hkv, int hd,
           int max_ctx, int n_chunks, float scale, uintptr_t opart, uintptr_t ml, uintptr_t out, uintptr_t counters,
           uintptr_t st, int split, uintptr_t block_table, int bt_rows, uintptr_t ts, int kv_fp8, float k_scale,
           float v_scale, uintptr_t out16, int out_wt, int short_len, int kv_tail, int kv_nt, int combine_trips) {
          AttnDecodeArgs a;
          a.split = split;
          a.out16 = (bf16_t*)out16; a.out_wt = out_wt; a.short_len = short_len; a.kv_tail = kv_tail; a.kv_nt = kv_nt;
          a.combine_trips = combine_trips;
          a.kv_fp8 = kv_fp8; a.kv_scale_k = k_scale; a.kv_scale_v = v_scale;
          a.ts = (unsigned long long*)ts;
          a.block_table = (const int*)block_table; a.bt_rows = bt_rows;
          a.q = (const float*)q; a.k_cache = (const bf16_t*)k; a.v_cache = (const bf16_t*)v;
          a.seq_len = (const int*)seq_len; a.slot = (const int*)slot;
          a.B = B; a.n_heads = H; a.n_kv_heads = Hkv; a.head_dim = hd; a.max_ctx = max_ctx; a.n_chunks = n_chunks;
          a.scale = scale; a.o_part = (float*)opart; a.ml = (float*)ml; a.out = (float*)out;
          a.counters = (int*)counters;
          launch_attn_decode(a, S(st));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("seq_len"), py::arg("slot"), py::arg("B"), py::arg("H"),
        py::arg("Hkv"), py::arg("hd"), py::arg("max_ctx"), py::arg("n_chunks"), py::arg("scale"), py::arg("opart"),
        py::arg("ml"), py::arg("out"), py::arg("counters"), py::arg("st"), py::arg("split") = 0,
        py::arg("block_table") = 0, py::arg("bt_rows") = 0, py::arg("ts") = 0, py::arg("kv_fp8") = 0,
        py::arg("k_scale") = 1.f, py::arg("v_scale") = 1.f, py::arg("out16") = 0, py::arg("out_wt") = 0,
        py::arg("short_len") = -1, py::arg("kv_tail") = -1, py::arg("kv_nt") = -1, py::arg("combine_trips") = 0);
  m.def("attn_decode_split", &attn_decode_split);
  // physical identity of a device (PCI bus id): ranks that share a GPU see the same string
  // the host-built launch descriptor of the one-workgroup-per-CU GEMVs (gemv_desc.h; no GPU needed):
  // None when the shape cannot be split, else {"G", "g0", "np0", "racc_n", "wgs": [per-workgroup dicts]}
  m.def("gemv_desc_build",
        [](std::vector<int> qtypes, std::vector<int> rows, int K, int grid, int variant) -> py::object {
          if (qtypes.empty() || qtypes.size() > 3 || rows.size() != qtypes.size())
            throw std::runtime_error("gemv_desc_build: 1..3 segments");
          GemvDescShape s{};
          s.nseg = (int)qtypes.size();
          int r = 0;
          for (int k = 0; k < s.nseg; ++k) { s.qtype[k] = qtypes[k]; s.seg_row0[k] = r; r += rows[k]; }
          s.N = r;
          s.K = K;
          s.grid = grid;
          s.variant = variant;
          CuPlan pl;
          int G = 0;
          if (!gemv_desc_plan(s, pl, G)) return py::none();
          py::list wgs;
          for (const GemvWgDesc& d : gemv_desc_build(s, pl, G)) {
            py::dict w;
            w["r0"] = d.r0; w["nrows"] = d.nrows; w["ngroups"] = d.ngroups; w["T"] = d.T; w["fmt1"] = d.fmt1;
            w["nfast"] = d.nfast;
            py::list pro;
            for (int i = 0; i < GD_PRO; ++i) {
              py::dict p;
              p["off"] = d.pro[i] & ((1 << GD_OFF_BITS) - 1);
              p["seg"] = (d.pro[i] >> GD_SEG_SHIFT) & 3;
              p["fast"] = (d.pro[i] & GD_FAST) != 0;
              p["seam"] = (d.pro[i] & GD_SEAM) != 0;
              pro.append(p);
            }
            w["pro"] = pro;
            wgs.append(w);
          }
          py::dict out;
          out["G"] = G; out["g0"] = pl.g0; out["np0"] = pl.np0; out["racc_n"] = pl.racc_n; out["wgs"] = wgs;
          return out;
        },
        py::arg("qtypes"), py::arg("rows"), py::arg("K"), py::arg("grid"), py::arg("variant") = 3);
  // the launch plan of a GEMV (gemv_plan.h; no GPU needed, no HIP call): which kernel family, template
  // parameters, grid, workgroup size and LDS bytes serve the shape on a device of `cus` CUs whose
  // occupancy query answers `occupancy`.  Raises exactly where launch_gemv would.  knobs: GemvKnobs
  // fields by name (the process environment is not read).  tp_fused: launch_gemv_tp_fused's plan
  // (family "none": it would not launch).  "engine_fits" / "bf16_engine_fits": the engine's questions.
  m.def("gemv_plan",
        [](std::vector<int> qtypes, std::vector<int> rows, int K, int B, int epi, int act_q8, int force_v1,
           int kernel_sel, int tune_grid, int tune_u, int tune_dbg, bool x16, bool y16, int grid_cap, int cus,
           int occupancy, py::dict knobs, bool tp_fused, bool check) {
          GemvShape s{};
          s.nseg = (int)qtypes.size();
          if (rows.size() != qtypes.size()) throw std::runtime_error("gemv_plan: one row count per segment");
          if (s.nseg < 1 || s.nseg > GEMV_MAX_SEGS) throw std::runtime_error("gemv: bad segment count");  // (check = false too)
          int r = 0;
          for (int k = 0; k < s.nseg && k < GEMV_MAX_SEGS; ++k) {
            s.qtype[k] = qtypes[k]; s.seg_row0[k] = r; s.seg_rows[k] = rows[k]; r += rows[k];
          }
          s.k_ok = 1; s.N = r; s.K = K; s.B = B; s.epi = epi; s.act_q8 = act_q8; s.force_v1 = force_v1;
          s.kernel_sel = kernel_sel; s.tune_grid = tune_grid; s.tune_u = tune_u; s.tune_dbg = tune_dbg;
          s.x16 = x16; s.y16 = y16; s.grid_cap = grid_cap;
          GemvKnobs kn;
          for (auto kv : knobs) {
            const std::string name = py::cast<std::string>(kv.first);
            int* f = name == "lds" ? &kn.lds : name == "lds_maxb" ? &kn.lds_maxb : name == "lds_b1_rsub" ? &kn.lds_b1_rsub
                   : name == "lds_b1_rsub_q6" ? &kn.lds_b1_rsub_q6 : name == "cu" ? &kn.cu
                   : name == "q8_balance" ? &kn.q8_balance : name == "bf16_lds" ? &kn.bf16_lds
                   : name == "lb_cfg" ? &kn.lb_cfg : nullptr;
            if (f) *f = py::cast<int>(kv.second);
            else if (name == "lds_min_kb") kn.lds_min_kb = py::cast<double>(kv.second);
            else throw std::runtime_error("gemv_plan: unknown knob " + name);
          }
          int asked = 0;
          auto occ = [&](const GemvPlan&) { ++asked; return occupancy; };
          const GemvPlan p = tp_fused ? plan_tp_fused(s, kn, cus, occ) : gemv_plan(s, kn, cus, occ, check);
          py::dict d;
          d["family"] = gemv_family_name(p.family);
          d["B"] = p.B; d["U"] = p.U; d["PIPE"] = p.PIPE; d["RSUB"] = p.RSUB; d["R"] = p.R; d["GPW"] = p.GPW; d["D"] = p.D;
          d["grid"] = p.grid; d["threads"] = p.threads; d["lds"] = p.lds; d["kt_max"] = p.kt_max;
          d["occ_grid"] = p.occ_grid; d["occupancy_asked"] = asked;
          d["g0"] = p.cu.g0; d["np0"] = p.cu.np0; d["racc_n"] = p.cu.racc_n;
          d["engine_fits"] = gemv_engine_fits(s, kn, cus);
          d["bf16_engine_fits"] = gemv_bf16_engine_fits(s, kn, cus);
          return d;
        },
        py::arg("qtypes"), py::arg("rows"), py::arg("K"), py::arg("B"), py::arg("epi") = 0, py::arg("act_q8") = 1,
        py::arg("force_v1") = 0, py::arg("kernel_sel") = 0, py::arg("tune_grid") = 0, py::arg("tune_u") = 0,
        py::arg("tune_dbg") = 0, py::arg("x16") = false, py::arg("y16") = false, py::arg("grid_cap") = 0,
        py::arg("cus") = 256, py::arg("occupancy") = 2, py::arg("knobs") = py::dict(), py::arg("tp_fused") = false,
        py::arg("check") = true);
  m.def("device_cu_count", [](int dev) {
    int n = 0;
    HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    return n;
  }, py::arg("device") = 0);
  m.def("device_pci_bus_id", [](int dev) {
    char buf[64] = {0};
    HIP_CHECK(hipDeviceGetPCIBusId(buf, (int)sizeof(buf), dev));
    return std::string(buf);
  });
  m.def("rmsnorm", [](uintptr_t x, int ldx, uintptr_t w, uintptr_t y, int ldy, int rows, int n, float eps, uintptr_t st) {
    launch_rmsnorm((const float*)x, ldx, (const float*)w, (float*)y, ldy, rows, n, eps, S(st));
  });
  m.def("rmsnorm_bf16", [](uintptr_t x, int ldx, uintptr_t w, uintptr_t y, int ldy, int rows, int n, float eps, uintptr_t st) {
    launch_rmsnorm_bf16((const float*)x, ldx, (const float*)w, (bf16_t*)y, ldy, rows, n, eps, S(st));
  });
  m.def("swiglu", [](uintptr_t gu, int ldg, uintptr_t out, int ldo, int rows, int n, uintptr_t st) {
    launch_swiglu_interleaved((const float*)gu, ldg, (float*)out, ldo, rows, n, S(st));
  });
  m.def("qkv_post",
        [](uintptr_t qkv, int ldqkv, int T, int H, int Hkv, int hd, uintptr_t q_norm, uintptr_t k_norm, float eps,
           int rope_neox, float rope_base, uintptr_t pos, uintptr_t slot, uintptr_t q_out, uintptr_t k_cache,
           uintptr_t v_cache, int max_ctx, uintptr_t st, uintptr_t block_table, uintptr_t rope_cs, uintptr_t bias,
           int kv_fp8, float kv_inv_k, float kv_inv_v, uintptr_t amax) {
          QkvPostArgs a;
          a.bias = (const float*)bias; a.kv_fp8 = kv_fp8; a.kv_inv_k = kv_inv_k; a.kv_inv_v = kv_inv_v;
          a.amax = (unsigned*)amax;
          a.block_table = (const int*)block_table;
          a.qkv = (const float*)qkv; a.ldqkv = ldqkv; a.T = T; a.n_heads = H; a.n_kv_heads = Hkv; a.head_dim = hd;
          a.q_norm = (const float*)q_norm; a.k_norm = (const float*)k_norm; a.eps = eps; a.rope_neox = rope_neox;
          a.rope_base = rope_base; a.rope_cs = (const float2*)rope_cs; a.pos = (const int*)pos; a.slot = (const int*)slot; a.q_out = (float*)q_out;
          a.k_cache = (bf16_t*)k_cache; a.v_cache = (bf16_t*)v_cache; a.max_ctx = max_ctx;
          launch_qkv_post(a, S(st));
        },
        py::arg("qkv"), py::arg("ldqkv"), py::arg("T"), py::arg("H"), py::arg("Hkv"), py::arg("hd"), py::arg("q_norm"),
        py::arg("k_norm"), py::arg("eps"), py::arg("rope_neox"), py::arg("rope_base"), py::arg("pos"), py::arg("slot"),
        py::arg("q_out"), py::arg("k_cache"), py::arg("v_cache"), py::arg("max_ctx"), py::arg("st"),
        py::arg("block_table") = 0, py::arg("rope_cs") = 0, py::arg("bias") = 0, py::arg("kv_fp8") = 0,
        py::arg("kv_inv_k") = 1.f, py::arg("kv_inv_v") = 1.f, py::arg("amax") = 0);
  // host side of the fp8 KV calibration: observed table -> per-layer (K, V) scales
  m.def("kv_scales_from_amax", &kv_scales_from_amax, py::arg("amax"), py::arg("n_layers"), py::arg("n_kv_heads"),
        py::arg("headroom") = 2.f);
  m.def("sample",
        [](uintptr_t logits, int ldl, int B, int V, uintptr_t temperature, uintptr_t top_k, uint64_t seed,
           uintptr_t tokens, uintptr_t pos, uintptr_t mask, uintptr_t st, uintptr_t top_p, uintptr_t ts,
           uintptr_t min_p, uintptr_t pen_tokens, int pen_stride, uintptr_t repeat_penalty, uintptr_t presence_penalty,
           uintptr_t frequency_penalty, uintptr_t bias_ids, uintptr_t bias_vals, int bias_stride) {
          // grow-on-demand scratch for the raw-op binding (the engine owns its own)
          static void* ws = nullptr;
          static size_t ws_bytes = 0;
          static int* cnt = nullptr;
          static int cnt_len = 0;
          const size_t need = sample_ws_bytes(B, V);
          if (need > ws_bytes) {
            if (ws) HIP_CHECK(hipFree(ws));
            HIP_CHECK(hipMalloc(&ws, need));
            ws_bytes = need;
          }
          if (B > cnt_len) {
            if (cnt) HIP_CHECK(hipFree(cnt));
            HIP_CHECK(hipMalloc(&cnt, (size_t)B * 4));
            HIP_CHECK(hipMemset(cnt, 0, (size_t)B * 4));
            cnt_len = B;
          }
          SampleArgs a;
          std::memset(&a, 0, sizeof(a));
          a.logits = (const float*)logits; a.ldl = ldl; a.B = B; a.V = V;
          a.temperature = (const float*)temperature; a.top_k = (const int*)top_k; a.seed = seed;
          a.tokens = (int*)tokens; a.pos = (int*)pos; a.mask = (const uint8_t*)mask;
          a.top_p = (const float*)top_p; a.ws = ws; a.ws_bytes = ws_bytes; a.counters = cnt;
          a.ts = (long long*)ts;
          a.min_p = (const float*)min_p; a.pen_tokens = (const int*)pen_tokens; a.pen_stride = pen_stride;
          a.repeat_penalty = (const float*)repeat_penalty; a.presence_penalty = (const float*)presence_penalty;
          a.frequency_penalty = (const float*)frequency_penalty;
          a.bias_ids = (const int*)bias_ids; a.bias_vals = (const float*)bias_vals; a.bias_stride = bias_stride;
          launch_sample(a, S(st));
        },
        py::arg("logits"), py::arg("ldl"), py::arg("B"), py::arg("V"), py::arg("temperature"), py::arg("top_k"),
        py::arg("seed"), py::arg("tokens"), py::arg("pos"), py::arg("mask"), py::arg("st"), py::arg("top_p") = 0,
        py::arg("ts") = 0, py::arg("min_p") = 0, py::arg("pen_tokens") = 0, py::arg("pen_stride") = 0,
        py::arg("repeat_penalty") = 0, py::arg("presence_penalty") = 0, py::arg("frequency_penalty") = 0,
        py::arg("bias_ids") = 0, py::arg("bias_vals") = 0, py::arg("bias_stride") = 0);
  m.attr("SAMPLE_BIAS_MAX") = SAMPLE_BIAS_MAX;
  m.attr("LOGPROB_MAX_TOP") = LOGPROB_MAX_TOP;
  m.def("logprobs",
        [](uintptr_t logits, int ldl, int B, int V, uintptr_t tokens, uintptr_t top_n, uintptr_t out_lp, uintptr_t out_id,
           uintptr_t st) {
          // grow-on-demand scratch for the raw-op binding (the engine owns its own); out_lp / out_id:
          // [B][LOGPROB_MAX_TOP + 1]
          static void* ws = nullptr;
          static size_t ws_bytes = 0;
          static int* cnt = nullptr;
          static int cnt_len = 0;
          if (B < 1 || V < 1 || V > SAMPLE_MAX_V)  // (before the sizes below are taken from them)
            throw std::runtime_error("logprobs: batch or vocabulary out of range (V <= " + std::to_string(SAMPLE_MAX_V) + ")");
          const size_t need = logprob_ws_bytes(B, V);
          if (need > ws_bytes) {
            if (ws) HIP_CHECK(hipFree(ws));
            ws = nullptr;
            ws_bytes = 0;
            HIP_CHECK(hipMalloc(&ws, need));
            ws_bytes = need;
          }
          if (B > cnt_len) {
            if (cnt) HIP_CHECK(hipFree(cnt));
            cnt = nullptr;
            cnt_len = 0;
            HIP_CHECK(hipMalloc(&cnt, (size_t)B * 4));
            HIP_CHECK(hipMemset(cnt, 0, (size_t)B * 4));
            cnt_len = B;
          }
          LogprobArgs a;
          std::memset(&a, 0, sizeof(a));
          a.logits = (const float*)logits; a.ldl = ldl; a.B = B; a.V = V;
          a.tokens = (const int*)tokens; a.top_n = (const int*)top_n;
          a.out_lp = (float*)out_lp; a.out_id = (int*)out_id;
          a.ws = ws; a.ws_bytes = ws_bytes; a.counters = cnt;
          launch_logprobs(a, S(st));
        },
        py::arg("logits"), py::arg("ldl"), py::arg("B"), py::arg("V"), py::arg("tokens"), py::arg("top_n"),
        py::arg("out_lp"), py::arg("out_id"), py::arg("st"));
  m.def("score_rows",
        [](uintptr_t logits, int ldl, int R, int V, uintptr_t targets, uintptr_t out_f, uintptr_t out_i, uintptr_t st,
           int max_grid) {
          // out_f / out_i: [R][2]; max_grid: workgroups at most (0: the launcher's cap), for the grid stride
          ScoreArgs a;
          std::memset(&a, 0, sizeof(a));
          a.logits = (const float*)logits; a.ldl = ldl; a.R = R; a.V = V;
          a.targets = (const int*)targets; a.out_f = (float*)out_f; a.out_i = (int*)out_i; a.max_grid = max_grid;
          launch_score_rows(a, S(st));
        },
        py::arg("logits"), py::arg("ldl"), py::arg("R"), py::arg("V"), py::arg("targets"), py::arg("out_f"),
        py::arg("out_i"), py::arg("st"), py::arg("max_grid") = 0);
  m.attr("SPEC_MAX_ROWS") = SPEC_MAX_ROWS;
  m.attr("SPEC_RECORD") = SPEC_RECORD;
  m.def("spec_accept",
        [](uintptr_t in, uintptr_t out, int pos0, int R, uintptr_t record, uintptr_t tokens, uintptr_t pos,
           uintptr_t seq_len, uintptr_t history, int hist_stride, uintptr_t st) {
          // in / out: [R] ints; record: [SPEC_RECORD]; tokens / pos / seq_len: the step state (row 0 written);
          // history: row 0's [hist_stride] or 0
          SpecAcceptArgs a;
          std::memset(&a, 0, sizeof(a));
          a.in = (const int*)in; a.out = (const int*)out; a.pos0 = pos0; a.R = R; a.record = (int*)record;
          a.tokens = (int*)tokens; a.pos = (int*)pos; a.seq_len = (int*)seq_len;
          a.history = (int*)history; a.hist_stride = hist_stride;
          launch_spec_accept(a, S(st));
        },
        py::arg("in_tokens"), py::arg("out_tokens"), py::arg("pos0"), py::arg("R"), py::arg("record"), py::arg("tokens"),
        py::arg("pos"), py::arg("seq_len"), py::arg("history"), py::arg("hist_stride"), py::arg("st"));
  m.attr("SPEC_MULTI_MAX_SEQS") = SPEC_MULTI_MAX_SEQS;
  m.attr("SPEC_MULTI_MAX_ROWS") = SPEC_MULTI_MAX_ROWS;
  m.def("spec_accept_multi",
        [](uintptr_t in, uintptr_t out, const std::vector<int>& seg, const std::vector<int>& pos0, uintptr_t record,
           uintptr_t tokens, uintptr_t pos, uintptr_t seq_len, uintptr_t history, int hist_stride, uintptr_t st) {
          // in / out: [Rt] ints; seg: S + 1 row offsets, pos0: S; record: [S][SPEC_RECORD]; tokens / pos / seq_len:
          // the step state (rows 0..S-1 written); history: [S][hist_stride] or 0
          if (seg.empty() || seg.size() > (size_t)SPEC_MULTI_MAX_SEQS + 1 || pos0.size() + 1 != seg.size())
            throw std::runtime_error("spec_accept_multi: seg needs 2.." + std::to_string(SPEC_MULTI_MAX_SEQS + 1) +
                                     " entries and pos0 one fewer");
          SpecAcceptMultiArgs a;
          std::memset(&a, 0, sizeof(a));
          a.in = (const int*)in; a.out = (const int*)out; a.S = (int)pos0.size();
          std::copy(seg.begin(), seg.end(), a.seg);
          std::copy(pos0.begin(), pos0.end(), a.pos0);
          a.record = (int*)record; a.tokens = (int*)tokens; a.pos = (int*)pos; a.seq_len = (int*)seq_len;
          a.history = (int*)history; a.hist_stride = hist_stride;
          launch_spec_accept_multi(a, S(st));
        },
        py::arg("in_tokens"), py::arg("out_tokens"), py::arg("seg"), py::arg("pos0"), py::arg("record"), py::arg("tokens"),
        py::arg("pos"), py::arg("seq_len"), py::arg("history"), py::arg("hist_stride"), py::arg("st"));
  m.attr("GRAMMAR_MAX") = GRAMMAR_MAX;
  m.attr("GRAMMAR_MAX_EOS") = GRAMMAR_MAX_EOS;
  m.def("grammar_tables",
        [](const std::vector<std::tuple<uintptr_t, uintptr_t, uintptr_t, int, int>>& grammars) {
          // the bytes of a GrammarTable array for grammar_mask's `grammars` (the caller copies them to the device):
          // one (byte_class[256] u8, trans[S][C] u16, accept[S] u8, S, C) of device pointers per grammar
          std::vector<GrammarTable> host;
          for (const auto& g : grammars)
            host.push_back(GrammarTable{(const uint8_t*)std::get<0>(g), (const uint16_t*)std::get<1>(g),
                                        (const uint8_t*)std::get<2>(g), std::get<3>(g), std::get<4>(g)});
          return py::bytes((const char*)host.data(), host.size() * sizeof(GrammarTable));
        },
        py::arg("grammars"));
  m.def("grammar_mask",
        [](uintptr_t tok_off, uintptr_t tok_bytes, int V, uintptr_t grammars, int n_grammars, uintptr_t gid,
           uintptr_t state, uintptr_t mask, int B, bool fill_free, const std::vector<int>& eos, uintptr_t st) {
          // tok_off: [V + 1] ints, tok_bytes: u8; grammars: the caller's device copy of grammar_tables(...), whose
          // tables' entries the caller has checked (ops.h); gid / state: [B] ints; mask: [B][ceil(V / 8)]
          if (n_grammars > GRAMMAR_MAX || eos.size() > (size_t)GRAMMAR_MAX_EOS)
            throw std::runtime_error("grammar_mask: too many grammars or end-of-sequence ids");
          GrammarMaskArgs a;
          std::memset(&a, 0, sizeof(a));
          a.tok_off = (const int*)tok_off; a.tok_bytes = (const uint8_t*)tok_bytes; a.V = V;
          a.grammars = (const GrammarTable*)grammars; a.n_grammars = n_grammars;
          a.gid = (const int*)gid; a.state = (const int*)state; a.mask = (uint8_t*)mask; a.B = B;
          a.fill_free = fill_free ? 1 : 0;
          a.n_eos = (int)eos.size();
          for (int j = 0; j < GRAMMAR_MAX_EOS; ++j) a.eos[j] = j < a.n_eos ? eos[j] : -1;
          launch_grammar_mask(a, S(st));
        },
        py::arg("tok_off"), py::arg("tok_bytes"), py::arg("V"), py::arg("grammars"), py::arg("n_grammars"), py::arg("gid"),
        py::arg("state"), py::arg("mask"), py::arg("B"), py::arg("fill_free"), py::arg("eos"), py::arg("st"));
  m.def("kv_snapshot",
        [](uintptr_t k_cache, uintptr_t v_cache, size_t layer_bytes, uintptr_t buf, uintptr_t block_table, int max_blocks,
           int n_blocks, int slot, int n_tokens, int n_layers, int n_kv_heads, int head_dim, int elem_bytes, bool unpack,
           int layer0, uintptr_t st) {
          // k_cache / v_cache: [layer] pools of layer_bytes each, [n_blocks + 1][n_kv_heads][KV_BLOCK][head_dim];
          // buf: [n_layers][2][n_kv_heads][n_tokens][head_dim]; block_table: [slots][max_blocks] ints
          KvSnapArgs a;
          std::memset(&a, 0, sizeof(a));
          a.k_cache = (void*)k_cache; a.v_cache = (void*)v_cache; a.layer_bytes = layer_bytes; a.buf = (void*)buf;
          a.block_table = (const int*)block_table; a.max_blocks = max_blocks; a.n_blocks = n_blocks; a.slot = slot;
          a.layer0 = layer0; a.n_layers = n_layers; a.n_kv_heads = n_kv_heads; a.head_dim = head_dim;
          a.n_tokens = n_tokens; a.elem_bytes = elem_bytes; a.unpack = unpack ? 1 : 0;
          launch_kv_snapshot(a, S(st));
        },
        py::arg("k_cache"), py::arg("v_cache"), py::arg("layer_bytes"), py::arg("buf"), py::arg("block_table"),
        py::arg("max_blocks"), py::arg("n_blocks"), py::arg("slot"), py::arg("n_tokens"), py::arg("n_layers"),
        py::arg("n_kv_heads"), py::arg("head_dim"), py::arg("elem_bytes"), py::arg("unpack"), py::arg("layer0") = 0,
        py::arg("st") = 0);
  m.attr("EMBED_NONE") = (int)EMBED_NONE;
  m.attr("EMBED_MEAN") = (int)EMBED_MEAN;
  m.attr("EMBED_LAST") = (int)EMBED_LAST;
  m.attr("EMBED_MAX_D") = EMBED_MAX_D;
  m.attr("EMBED_MAX_WG") = EMBED_MAX_WG;
  m.def("embed_pool_ws_bytes", &embed_pool_ws_bytes);
  m.def("embed_pool",
        [](uintptr_t x, int ldx, int n, int d, uintptr_t g, float eps, uintptr_t acc, uintptr_t count, int mode, int first,
           int final, uintptr_t out, uintptr_t ws, size_t ws_bytes, uintptr_t counter, uintptr_t st) {
          // every buffer is the caller's: ws of embed_pool_ws_bytes(d) bytes, counter one zeroed int
          EmbedPoolArgs a;
          std::memset(&a, 0, sizeof(a));
          a.x = (const float*)x; a.ldx = ldx; a.n = n; a.d = d; a.g = (const float*)g; a.eps = eps;
          a.acc = (float*)acc; a.count = (int*)count; a.mode = mode; a.first = first; a.final = final;
          a.out = (float*)out; a.ws = (float*)ws; a.ws_bytes = ws_bytes; a.counter = (int*)counter;
          launch_embed_pool(a, S(st));
        },
        py::arg("x"), py::arg("ldx"), py::arg("n"), py::arg("d"), py::arg("g"), py::arg("eps"), py::arg("acc"),
        py::arg("count"), py::arg("mode"), py::arg("first"), py::arg("final"), py::arg("out"), py::arg("ws"),
        py::arg("ws_bytes"), py::arg("counter"), py::arg("st"));
  m.def("gemm",
        [](uintptr_t A, int lda, PyQMatrix* w, int M, uintptr_t C, int ldc, int accumulate, uintptr_t st) {
          GemmArgs a;
          a.A = (const bf16_t*)A; a.lda = lda; a.w = w->w; a.M = M; a.N = w->w.rows; a.K = w->w.cols;
          a.C = (float*)C; a.ldc = ldc; a.accumulate = accumulate;
          GemmWs& g = gemm_ws(M, a.N);
          a.ws = g.ws; a.ws_bytes = g.bytes; a.cnt = g.cnt; a.cnt_len = g.cnt_len;
          launch_gemm(a, S(st));
        });
  m.def("gemm_supports", &gemm_supports);
  m.def(
      "gemm_q",
      // kw: the GemmQArgs fields of the fused epilogues, each defaulting to 0 / null (kv_inv_* to 1) --
      // GEPI_QKV: col0, head_dim, q_dim, kv_dim, n_kv_heads, max_ctx, rope_cs, pos, slot, block_table,
      // q_out, k_cache, v_cache, kv_fp8, kv_inv_k, kv_inv_v; the split RMSNorm: nrm_g, nrm_out16,
      // nrm_part, nrm_in, nrm_parts, nrm_eps
      [](uintptr_t A, int lda, std::vector<PyQMatrix*> segs, int M, uintptr_t C, uintptr_t C16, int ldc, int epi,
         uintptr_t st, int ksplit, uintptr_t dbg_ts, py::kwargs kw) {
        GemmQArgs a;
        gemm_q_args(a, segs, lda, M, ldc, epi, ksplit, kw);
        a.A = (const bf16_t*)A; a.C = (float*)C; a.C16 = (bf16_t*)C16;
        a.dbg_ts = (unsigned long long*)dbg_ts;
        GemmWs& g = gemm_ws(M, a.N);
        a.ws = g.ws; a.ws_bytes = g.bytes; a.cnt = g.cnt; a.cnt_len = g.cnt_len;
        launch_gemm_q(a, S(st));
      },
      py::arg("A"), py::arg("lda"), py::arg("segs"), py::arg("M"), py::arg("C"), py::arg("C16"), py::arg("ldc"),
      py::arg("epi"), py::arg("stream"), py::arg("ksplit") = 0, py::arg("dbg_ts") = 0);
  // which kernel launch_gemm_q would hand each format-split launch of the same call to (no launch):
  // [(col0, "ring" | "pf" | "skinny" | "big")].  gemm_q's arguments minus the buffers: A, C / C16 count
  // as present and aligned; the keyword pointers are only tested for null, pass what gemm_q gets
  m.def(
      "gemm_route",
      [](int lda, std::vector<PyQMatrix*> segs, int M, int ldc, int epi, int ksplit, py::kwargs kw) {
        GemmQArgs a;
        gemm_q_args(a, segs, lda, M, ldc, epi, ksplit, kw);
        a.A = (const bf16_t*)(uintptr_t)256;
        if (epi == GEPI_SWIGLU_BF16) a.C16 = (bf16_t*)(uintptr_t)256;
        else a.C = (float*)(uintptr_t)256;
        GemmWs& g = gemm_ws(M, a.N);  // (the split-K workspace gemm_q would pass)
        a.ws = g.ws; a.ws_bytes = g.bytes; a.cnt = g.cnt; a.cnt_len = g.cnt_len;
        static const char* names[] = {"ring", "pf", "skinny", "big"};
        py::list out;
        for (const GemmRoute& r : gemm_route(a)) out.append(py::make_tuple(r.col0, names[r.kernel]));
        return out;
      },
      py::arg("lda"), py::arg("segs"), py::arg("M"), py::arg("ldc"), py::arg("epi"), py::arg("ksplit") = 0);
  // output tiles of the skinny kernel for a stack at M rows (AIOS_SKINNY_RB is read per call): the
  // nrm_parts of a GEPI_ACCUM_NORM producer, as the engine sizes it
  m.def(
      "gemm_skinny_ntile",
      [](std::vector<PyQMatrix*> segs, int M) {
        GemmQArgs a;
        gemm_q_args(a, segs, segs.empty() ? 0 : segs[0]->w.cols, M, 0, GEPI_STORE, 0, py::kwargs());
        return gemm_skinny_ntile(a);
      },
      py::arg("segs"), py::arg("M"));
  // residual[m][:] += data[m][:] (data 0: residual holds the sum) + the split-RMSNorm producer outputs
  m.def(
      "add_norm",
      [](uintptr_t residual, uintptr_t data, int rows, int d, uintptr_t g, uintptr_t out16, int ld16, uintptr_t part,
         int parts, uintptr_t st) {
        launch_add_norm((float*)residual, (const float*)data, rows, d,
                        ResidNorm{(const float*)g, (bf16_t*)out16, ld16, (float*)part, parts}, S(st));
      },
      py::arg("residual"), py::arg("data"), py::arg("rows"), py::arg("d"), py::arg("g"), py::arg("out16"),
      py::arg("ld16"), py::arg("part"), py::arg("parts"), py::arg("st") = 0);
  m.def(
      "gemm_pf_plan",
      [](std::vector<PyQMatrix*> segs, int M, int epi, int ksplit) {
        GemmQArgs a;
        std::memset(&a, 0, sizeof(a));
        if (segs.empty() || segs.size() > 3) throw std::runtime_error("gemm_pf_plan: 1..3 segments");
        a.nseg = (int)segs.size();
        int n0 = 0;
        for (int s = 0; s < a.nseg; ++s) { a.seg[s] = segs[s]->w; a.seg_n0[s] = n0; n0 += segs[s]->w.rows; }
        a.M = M; a.N = n0; a.K = segs[0]->w.cols; a.epi = epi; a.ksplit = ksplit;
        int bm = 0, bn = 0, sp = 0;
        gemm_pf_plan(a, bm, bn, sp);
        return py::make_tuple(bm, bn, sp);
      },
      py::arg("segs"), py::arg("M"), py::arg("epi"), py::arg("ksplit") = 0);
  m.attr("GEPI_STORE") = (int)GEPI_STORE;
  m.attr("GEPI_ACCUM") = (int)GEPI_ACCUM;
  m.attr("GEPI_SWIGLU_BF16") = (int)GEPI_SWIGLU_BF16;
  m.attr("GEPI_QKV") = (int)GEPI_QKV;
  m.attr("GEPI_ACCUM_NORM") = (int)GEPI_ACCUM_NORM;
  m.def(
      "attn_prefill",
      [](uintptr_t q, uintptr_t k, uintptr_t v, int slot, int start, int T, int H, int Hkv, int hd, int max_ctx,
         float scale, uintptr_t out, int ldo, uintptr_t st, uintptr_t block_table, int kv_fp8, float k_scale,
         float v_scale) {
        AttnPrefillArgs a;
        a.kv_fp8 = kv_fp8; a.kv_scale_k = k_scale; a.kv_scale_v = v_scale;
        a.block_table = (const int*)block_table;
        a.q = (const float*)q; a.k_cache = (const bf16_t*)k; a.v_cache = (const bf16_t*)v;
        a.slot = slot; a.start = start; a.T = T; a.n_heads = H; a.n_kv_heads = Hkv; a.head_dim = hd;
        a.max_ctx = max_ctx; a.scale = scale; a.out = (bf16_t*)out; a.ldo = ldo;
        launch_attn_prefill(a, S(st));
      },
      py::arg("q"), py::arg("k"), py::arg("v"), py::arg("slot"), py::arg("start"), py::arg("T"), py::arg("H"),
      py::arg("Hkv"), py::arg("hd"), py::arg("max_ctx"), py::arg("scale"), py::arg("out"), py::arg("ldo"),
      py::arg("st"), py::arg("block_table") = 0, py::arg("kv_fp8") = 0, py::arg("k_scale") = 1.f,
      py::arg("v_scale") = 1.f);
  m.def("attn_prefill_supports", &attn_prefill_supports);

  // ------------------------------------------------------------------ JSON-mode grammar (K10)
  py::class_<JsonState>(m, "JsonState")
      .def(py::init<>())
      .def("copy", [](const JsonState& s) { return JsonState(s); })
      .def_property_readonly("depth", [](const JsonState& s) { return (int)s.depth; })
      .def_property_readonly("mode", [](const JsonState& s) { return (int)s.mode; });
  py::class_<JsonGrammar>(m, "JsonGrammar")
      .def(py::init([](const std::vector<py::bytes>& toks, int eos, int max_ws, bool require_object) {
             std::vector<std::string> t;
             t.reserve(toks.size());
             for (auto& b : toks) t.push_back(std::string(b));
             return new JsonGrammar(t, eos, max_ws, require_object);
           }),
           py::arg("tokens"), py::arg("eos_id"), py::arg("max_ws") = 20, py::arg("require_object") = true)
      .def("initial", &JsonGrammar::initial)
      .def("accept_token", &JsonGrammar::accept_token)
      .def("accept_bytes", [](const JsonGrammar& g, JsonState& s, py::bytes b) { return g.accept_bytes(s, std::string(b)); })
      .def("complete", &JsonGrammar::complete)
      .def("mask",
           [](JsonGrammar& g, const JsonState& s) {
             const std::vector<uint8_t>* m;
             {
               py::gil_scoped_release nogil;
               m = &g.mask(s);
             }
             return py::bytes((const char*)m->data(), m->size());
           })
      .def("mask_open",
           [](JsonGrammar& g, const JsonState& s) {
             const std::vector<uint8_t>* m;
             {
               py::gil_scoped_release nogil;
               m = &g.mask_open(s);
             }
             return py::bytes((const char*)m->data(), m->size());
           })
      .def_property_readonly("vocab_size", &JsonGrammar::vocab_size)
      .def_property_readonly("cache_size", &JsonGrammar::cache_size);
  m.def("gemm_pf_export", &gemm_pf_export);
  m.def("gemm_pf_import", &gemm_pf_import, py::arg("plans"));
  m.def("bench_stream_read_part", &aios::bench_stream_read_part, py::arg("bytes"), py::arg("nbuf"), py::arg("mode"),
        py::arg("threads") = 512, py::arg("reps") = 20);
  m.def("bench_stream_read", &aios::bench_stream_read, py::arg("bytes"), py::arg("nbuf"), py::arg("wg_per_cu"),
        py::arg("u"), py::arg("threads"), py::arg("reps"));
  m.def("bench_launch_chain", &aios::bench_launch_chain, py::arg("n_kernels"), py::arg("blocks"), py::arg("use_graph"),
        py::arg("reps"), py::call_guard<py::gil_scoped_release>());
}
