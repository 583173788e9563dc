// In-process inference engine for Llama-family GGUF models on one MI355X (gfx950).
//
// Replaces the reference's per-model llama-server child process
// (`runtime/src/model_manager.rs:185-204`, HTTP at `runtime/src/inference.rs:94-186`):
// weights live in HBM in the repacked GEMV layout, the KV cache is a bf16 slab
// [layer][slot][kv_head][max_ctx][head_dim], and the whole decode step (embed -> L x {QKV+RoPE+KV,
// attention, O+residual, gate/up+SwiGLU, down+residual} -> norm+lm_head -> sample) is one
// stream-ordered sequence of launches that is captured once per batch size into a hipGraph and
// replayed (SURVEY.md §2.7 fusion targets, §7.6 hard part 2).  Sampled tokens are fed back on
// device, so N decode steps need no host round trip.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"
#include "ops.h"

namespace aios {

struct EngineConfig {
  std::string name = "model";
  int vocab_size = 32000;
  int d_model = 2048;
  int n_layers = 22;
  int n_heads = 32;
  int n_kv_heads = 4;
  int head_dim = 64;
  int d_ff = 5632;
  float rope_theta = 10000.f;
  int rope_neox = 0;
  float norm_eps = 1e-5f;
  int max_ctx = 2048;
  int max_slots = 4;
  int max_batch = 8;
  int tie_embeddings = 0;
  int qk_norm = 0;
  int qkv_bias = 0;
  int act_q8 = 1;  // int8 activations (v_dot4) in the quantised GEMVs, as llama.cpp's q8_1 path
  // tensor parallel (the engine holds this rank's shard; collectives via the comm hook)
  int tp_rank = 0;
  int tp_size = 1;
  // vocab-parallel lm_head under TP: output.weight holds rows [rank*V/tp, (rank+1)*V/tp) and the
  // logits are completed by the all-gather hook (ignored for tp_size 1 / tied embeddings)
  int vocab_parallel = 0;
  int device = 0;
  // KV cache element type: 0 = bf16, 1 = fp8 e4m3 (OCP) with a per-layer K / V scale (value = code x
  // scale) -- half the cache bytes and the decode attention's K / V reads (bf16 or fp8
  // on MI355X).  The scales are 1.0 until Engine::calibrate_kv_scales or set_kv_scales installs others;
  // at 1.0 a layer whose keys / values leave e4m3's window (below 2^-9, above 448) is stored wrong
  int kv_fp8 = 0;
  // CU mask of the engine's stream (hipExtStreamCreateWithCUMask; 32 CUs per word, empty = every CU):
  // co-resident tiers each get their own CUs, and the engine sizes its grids to the mask's CU count
  std::vector<uint32_t> cu_mask;
  // stream priority (co-resident tiers, unmasked streams): 0 = normal, < 0 = higher (the range of
  // hipDeviceGetStreamPriorityRange; the hardware queue's dispatcher serves it first)
  int stream_priority = 0;
};

// device matrix in repacked layout (owns its buffer)
struct QMat {
  QWeight w{};
  void* buf = nullptr;
  size_t bytes = 0;
  bool valid() const { return buf != nullptr; }
};

struct LayerW {
  float* attn_norm = nullptr;
  float* ffn_norm = nullptr;
  float* q_norm = nullptr;
  float* k_norm = nullptr;
  float* bqkv = nullptr;  // [q_dim + 2 kv_dim]
  QMat wq, wk, wv, wo, wgu, wdown;
};

// all-reduce hook (TP): sum `n` floats of `data` over the TP ranks on `stream` and add the
// total into `residual` (or into `data` when residual is null); installed by aios_amd/parallel.
using AllReduceFn = void (*)(void* ctx, float* data, size_t n, float* residual, hipStream_t stream);
// all-gather hook (vocab-parallel lm_head): rank r owns columns [r*slice, (r+1)*slice) of the
// rows x ld fp32 matrix `data`; afterwards every rank holds all of them
using AllGatherFn = void (*)(void* ctx, float* data, int rows, int slice, int ld, hipStream_t stream);
// fused all-reduce + split-RMSNorm producer hook (batched TP decode, C1 / C2): residual ([rows][d]) +=
// sum of partials, then the ResidNorm outputs (ops.h) the next skinny GEMM consumes -- no RMSNorm launch
using AllReduceNormFn = void (*)(void* ctx, float* data, int rows, int d, float* residual, const ResidNorm& nm,
                                 hipStream_t stream);

class Engine {
 public:
  explicit Engine(const EngineConfig& cfg);
  ~Engine();

  const EngineConfig& config() const { return cfg_; }

  // --- weights -------------------------------------------------------------------------------
  // raw GGUF bytes (host pointer) of a named tensor; names follow GGUF ("blk.3.attn_q.weight").
  void set_tensor(const std::string& name, int ggml_type, int rows, int cols, const void* host, size_t nbytes);
  // random-init synthetic weights generated in HBM (recipe: "Q4_K_M", "Q4_0", "Q8_0", "BF16", ...)
  void init_random(const std::string& recipe, uint64_t seed);
  void finalize();  // checks completeness, allocates KV cache + workspace
  bool ready() const { return finalized_; }
  size_t weight_bytes() const { return weight_bytes_; }
  size_t kv_bytes() const { return kv_bytes_; }
  size_t workspace_bytes() const { return ws_bytes_; }
  std::vector<std::string> missing_tensors() const;
  std::string weight_type_summary() const;

  // --- inference -----------------------------------------------------------------------------
  // Prefill `tokens` into `slot` starting at position `start_pos`.  Returns logits of the last
  // token (host copy) if want_logits, and leaves the slot ready to decode.
  std::vector<float> prefill(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits);
  // Text embedding of a prompt (ops.h EmbedPoolArgs: the rule).  Runs the forward and KV writes of
  // prefill(slot, tokens, start_pos, false) -- the slot afterwards holds valid KV for those positions --
  // and after each internal chunk folds that chunk's hidden rows into the slot's pooling state.  One
  // difference from prefill: chunks that reach the prefill GEMM (more than 32 rows) ask for its best plan
  // without split-K / stream-K (GemmQArgs::ksplit < 0), whose fp32 atomics make two prefills of one prompt
  // differ in the low bits.  With that, calls of 5 tokens or more give the same bytes every time; shorter
  // ones take the GEMV path, whose bf16 kernels sum with LDS float atomics, and may differ in the last bits.
  // A prompt
  // may come in several calls (the scheduler's chunked prefill): start_pos == 0 resets the slot's state, a
  // later call must start where the last one ended, with the same pooling (else it throws: a chunk was
  // skipped or repeated); EMBED_LAST keeps no state and may start anywhere (a cached prefix).  EMBED_NONE
  // stages its rows in ONE device buffer (max_ctx x d floats, allocated by the first such call): a NONE call
  // on another slot ends the prompt being staged, whose next call then throws.  final ==
  // false returns nothing; final == true returns the d floats of the unit vector, or for EMBED_NONE the
  // (start_pos + T) x d normed rows, staged on the device and copied out once.  Single-GPU engines only.
  std::vector<float> embed_prefill(int slot, const std::vector<int>& tokens, int start_pos, int pooling, bool final);
  int embed_tokens() const { return emb_tokens_; }  // tokens pooled by the last final embed_prefill
  // Prompt scoring (ops.h ScoreArgs: the rule).  Runs exactly the forward and KV writes of
  // prefill(slot, tokens, start_pos, want_logits) and after each internal chunk scores that chunk's hidden
  // rows in groups: output_norm + lm_head of the group into a scoring logits buffer [group rows][V], the
  // row-scoring kernel, and, when top_n > 0, the logprob kernel over the same rows for the alternatives.
  // Row i's target is tokens[i + 1]; the call's last row takes next_token (-1: none -- lp NaN, rank -1; a
  // chunked caller passes the next chunk's first token).  The scoring buffer is allocated by the first call
  // and bounded independently of the chunk: SCORE_LOGITS_BYTES of logits, i.e. that many bytes / (4 V) rows
  // per group (at least SCORE_MIN_ROWS, at most the prefill chunk).  The call's results are staged on the
  // device and copied out once.  want_logits: the last row's logits are also left in logits_ row 0 by the
  // lm_head(1, ...) call prefill makes, so sample_first and the decode steps behave as after prefill (the
  // host copy of that row is not returned).  top_n in 0..LOGPROB_MAX_TOP; a vocabulary above SAMPLE_MAX_V is
  // refused only when top_n > 0.  Single-GPU engines only: a vocab-parallel lm_head shards the row.
  static constexpr size_t SCORE_LOGITS_BYTES = (size_t)64 << 20;
  static constexpr int SCORE_MIN_ROWS = 64;
  struct PromptScores {
    std::vector<float> lp, best_lp;  // [T]
    std::vector<int> rank, best;     // [T]
    std::vector<int> ids;            // [T][top_n], only when top_n > 0
    std::vector<float> lps;          // [T][top_n], only when top_n > 0
  };
  PromptScores score_prefill(int slot, const std::vector<int>& tokens, int start_pos, int next_token, int top_n,
                             bool want_logits);
  int score_group_rows() const;  // rows per lm_head group for this model
  // One decode step for B sequences: input token ids at positions pos[b] in slots[b].  Samples
  // with per-row temperature/top_k (0 = greedy) and optional grammar bitmasks; returns tokens.
  std::vector<int> decode(const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
                          const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
                          const std::vector<uint8_t>& mask, const std::vector<float>& top_p = {},
                          const std::vector<uint64_t>& seeds = {});
  // sample the token after a prefill from its last logits (logits_ row 0) on the device, with the
  // same sampler and RNG stream (seed, pos) as the decode steps -- pos: the prompt's last position
  int sample_first(int pos, float temperature, int top_k, float top_p, uint64_t seed, const std::vector<uint8_t>& mask);
  // re-sample the last step's logits (no state advance), e.g. with a grammar mask
  std::vector<int> resample(int B, const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
                            const std::vector<uint8_t>& mask, const std::vector<float>& top_p = {});
  // logits of the last decode (B x V) -- host copy
  std::vector<float> last_logits(int B);

  // Speculative decoding (ops.h SpecAcceptArgs: the rule): one request's R consecutive positions as the R
  // rows of one decode step.  tokens[0] is the request's last accepted token (at pos0), tokens[1..R) a draft
  // of what follows; rows are (slot, tokens[i], pos0 + i), every row samples with the request's parameters
  // and seeds[i] = seed, so row i draws what a one-row step at pos0 + i would.  Runs the B = R forward graph
  // (the same graph key as decode's), the eager sampler with the rows' masks (R rows or empty), the staged
  // processors / logprobs with decode()'s contract (staged for R rows, one shot; last_logprobs() reports R
  // rows, the caller uses the first accepted + 1), then the accept kernel, and returns after one copy of its
  // record.  Afterwards: the slot holds valid K/V for [0, pos0 + accepted + 1) -- the positions behind hold
  // the rejected rows' K/V, which nothing reads and the next write there replaces (the pipelined scheduler's
  // rule for its dropped forward), and their blocks stay mapped to the slot; the step state is one row at
  // pos0 + accepted + 1 whose token is on the device, so a B = 1 decode_submit(tokens = {}) continues from
  // it; logits_ keeps the R rows (last_logits(R)).  Throws before any state changes on: R outside
  // 2..min(max_batch, SPEC_MAX_ROWS), pos0 + R > max_ctx, a token out of range, a mask that is not R rows, a
  // tensor-parallel engine, a pipelined step in flight (sampled by decode_sample and not yet collected; a
  // forward that was submitted and never sampled -- the scheduler's dropped forward -- does not count).
  struct SpecResult {
    int accepted = 0;
    std::vector<int> tokens;  // accepted + 1 of them
  };
  SpecResult spec_decode(int slot, const std::vector<int>& tokens, int pos0, float temperature, int top_k, float top_p,
                         uint64_t seed, const std::vector<uint8_t>& masks);
  // The same step for S sequences at once (ops.h SpecAcceptMultiArgs: the rule).  Sequence s brings tokens[s]:
  // its last accepted token (at pos0[s]) and a draft of 0..SPEC_MAX_ROWS - 1 tokens; the step's Rt rows are the
  // segments one after another, (slots[s], tokens[s][i], pos0[s] + i), every row of segment s sampling with
  // temperature[s], top_k[s], top_p[s] and seeds[i] = seeds[s].  Runs the B = Rt forward graph (decode's graph
  // key), the eager sampler with the rows' masks (Rt rows or empty), the staged processors / logprobs / grammar
  // rows with decode()'s contract (staged for Rt rows, one shot; last_logprobs() reports Rt rows in segment
  // order), then the segmented accept kernel, and returns after one copy of its S records: one result per
  // sequence.  Afterwards: slot s holds valid K/V for [0, pos0[s] + accepted_s + 1), the rejected rows' K/V
  // behind it as after spec_decode; the step state is S rows, row s the sequence at pos0[s] + accepted_s + 1
  // whose token is on the device, so a B = S decode_submit(tokens = {}) with the slots in segment order
  // continues from them; logits_ keeps the Rt rows.  Throws before any state changes on: S outside
  // 1..SPEC_MULTI_MAX_SEQS (or per-sequence arguments of another length), a segment empty or longer than
  // SPEC_MAX_ROWS, Rt > min(max_batch, SPEC_MULTI_MAX_ROWS), a bad slot or one named twice, pos0[s] + rows_s >
  // max_ctx, a token out of range, masks that are neither empty nor Rt rows, a tensor-parallel engine, a
  // pipelined step in flight.
  std::vector<SpecResult> spec_decode_multi(const std::vector<int>& slots, const std::vector<std::vector<int>>& tokens,
                                            const std::vector<int>& pos0, const std::vector<float>& temperature,
                                            const std::vector<int>& top_k, const std::vector<float>& top_p,
                                            const std::vector<uint64_t>& seeds, const std::vector<uint8_t>& masks);

  // Pipelined decode (the serving scheduler's fast path): decode() split so that the forward of step
  // t+1 is enqueued before the host has seen step t's token -- the rows' tokens are the ones step t's
  // sampler left on the device -- and only the sampler waits for the host's grammar mask:
  //   decode_submit(..., tokens = {})   forward graph of the next step (tokens from the device)
  //   decode_sample(mask)               mask upload + sampler + token copy, one event
  //   decode_collect()                  waits for that event: the sampled tokens
  // The stream holds sample(t), forward(t+1) while the host turns token t into mask t+1.
  // decode_submit with tokens: the host's tokens (a batch's first step).
  void decode_submit(const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
                     const std::vector<float>& temperature, const std::vector<int>& top_k, uint64_t seed,
                     const std::vector<float>& top_p = {}, const std::vector<uint64_t>& seeds = {});
  void decode_sample(const std::vector<uint8_t>& mask);
  std::vector<int> decode_collect();

  // Logit processors (ops.h SampleArgs: min-p, repeat / presence / frequency penalties) of the NEXT
  // sampler launch only -- decode, decode_sample, sample_first or resample, whichever comes first --
  // and dropped after it, so a row's values never reach another batch.  Dropped as well by a sampler-launching
  // call that throws before its launch (a refused argument, say) and by decode_loop_run: they never wait
  // for a later, unrelated launch with the same row count.  One entry per row of that launch; recent[b]:
  // the row's penalty window, at most SAMPLE_PEN_MAX token ids, each in [0, vocab).
  // decode() with processors staged replays the forward graph and enqueues the sampler eagerly, like
  // the pipelined path (no graph of its own).  Single-GPU engines only: the ranks of a tensor-parallel
  // engine sample in lock step from arguments this call does not broadcast.
  // bias_ids / bias_vals (both empty: none): the rows' logit-bias lists (ops.h, applied in front of the
  // penalties), one list per row, at most SAMPLE_BIAS_MAX entries each, a row's ids distinct and in
  // [0, vocab), a bias finite or -inf (a ban), fewer bans than the vocabulary has tokens; a row with an
  // empty list is neutral.
  void set_sample_processors(const std::vector<float>& min_p, const std::vector<float>& repeat_penalty,
                             const std::vector<float>& presence_penalty, const std::vector<float>& frequency_penalty,
                             const std::vector<std::vector<int>>& recent,
                             const std::vector<std::vector<int>>& bias_ids = {},
                             const std::vector<std::vector<float>>& bias_vals = {});

  // Per-token log-probabilities (ops.h LogprobArgs: the RAW distribution, before penalties, mask and
  // temperature) of the NEXT sampler launch only -- decode, decode_sample, sample_first or resample,
  // whichever comes first -- and dropped after it: set_sample_processors' contract.  One entry per row of
  // that launch: the alternatives wanted, 0..LOGPROB_MAX_TOP, or < 0 for a row that reports nothing.
  // The logprob launch follows the sampler on the stream, reads the tokens it wrote, and its outputs
  // reach pinned memory before the step's tokens do; decode() with logprobs staged runs the forward
  // graph and an eager sampler, as with staged processors.  Single-GPU engines only: a vocab-parallel
  // lm_head shards the row.
  void set_logprobs(const std::vector<int>& top_n);
  // what the last sampler launch reported (call after its tokens were returned / collected); every vector
  // empty when that launch had nothing staged.  Rows that were off: token_lp NaN, ids -1, lps -inf.
  struct Logprobs {
    std::vector<int> top_n;       // [B] as staged
    std::vector<float> token_lp;  // [B] logprob of the sampled token
    std::vector<int> ids;         // [B][LOGPROB_MAX_TOP] alternatives, best first; -1 past the row's top_n
    std::vector<float> lps;       // [B][LOGPROB_MAX_TOP]
  };
  Logprobs last_logprobs() const;

  // DFA grammars (ops.h GrammarMaskArgs: the rule): a row's allowed-token mask computed on the device from
  // (grammar id, state) -- no host walk, no memo, no per-step mask upload.
  // grammar_vocab: the vocabulary's byte strings (vocab_size of them, empty for a control token: what JsonGrammar
  // receives) and its end-of-sequence ids, uploaded once; calling it again drops nothing but replaces the table.
  // grammar_load: uploads one grammar's tables and returns its id (ids of freed grammars are reused).  Refuses,
  // before anything is kept: a table that is not [n_states][n_classes] with 2 <= n_states <= 65535 and 1 <=
  // n_classes <= 256, a class or transition out of range, a dead state 0 with a way out, GRAMMAR_MAX grammars
  // already loaded, no vocabulary, and -- after one grammar_masks pass over every state -- a live state that is
  // not terminal (accepting with no way on) and allows no token: no tokenizer path leads on from there.
  // grammar_free: waits for the stream, then frees the tables.  grammar_masks: the masks of `states`, one row
  // each, ceil(V / 8) bytes per row (one launch per GRAMMAR_MASK_ROWS rows, into a buffer of its own).
  // set_grammar_rows: the rows' (grammar id or -1, state) for the NEXT sampler launch only -- decode,
  // decode_sample, sample_first or resample -- with set_sample_processors' lifetime: one shot, refused and dropped
  // when staged for another row count, dropped by a call that throws before its launch, by decode_loop_run and
  // by spec_decode (grammar rows take no speculative steps).  At that launch the mask kernel goes on the
  // stream behind the host mask's copy, if the call has one, and in front of the sampler (or of the step graph
  // that holds it), and the sampler runs masked: rows with id -1 keep the host's mask bytes, or are set to all
  // ones when the call passed no mask.  A state must be a live state of its grammar.  Single-GPU engines only.
  static constexpr int GRAMMAR_MASK_ROWS = 1024;
  void grammar_vocab(const std::vector<std::string>& tokens, const std::vector<int>& eos_ids);
  int grammar_load(const uint8_t* byte_class, const uint16_t* trans, const uint8_t* accept, int n_states, int n_classes);
  void grammar_free(int gid);
  std::vector<uint8_t> grammar_masks(int gid, const std::vector<int>& states);
  void set_grammar_rows(const std::vector<int>& gids, const std::vector<int>& states);
  int grammars_loaded() const;

  // Device-resident greedy generation for benchmarking: runs n_steps decode steps for B
  // sequences without host synchronisation (tokens fed back on device, graph replay when
  // use_graph).  Sequences must already be prefilled to positions pos[b].
  void decode_loop_prepare(const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos);
  void decode_loop_run(int B, int n_steps, bool use_graph);
  std::vector<int> decode_loop_history(int B, int from_pos, int n);

  void synchronize();
  uintptr_t stream_handle() const { return (uintptr_t)stream_; }
  void set_allreduce(AllReduceFn fn, void* ctx) { allreduce_ = fn; allreduce_ctx_ = ctx; }
  void set_allgather(AllGatherFn fn, void* ctx) { allgather_ = fn; allgather_ctx_ = ctx; }
  void set_allreduce_norm(AllReduceNormFn fn, void* ctx) { allreduce_norm_ = fn; allreduce_norm_ctx_ = ctx; }
  // TP: the O / down all-reduces fused into the B <= 4 GEMV engine's epilogue (EPI_TP_RESID);
  // ctx null = separate all-reduce launches; grid = engine workgroups per launch (0: one per CU)
  void set_tp_fuse(const ArDevCtx* ctx, int grid) { tp_fuse_ = ctx; tp_fuse_grid_ = grid; }
  bool tp_fused() const { return tp_fuse_ != nullptr; }
  // TP init: for every layer's O and down projection at batch 1, whether the fused all-reduce
  // epilogue would launch on THIS rank (row kernel stage fit under the co-residency cap, which
  // depends on the device's CU count); the ranks all-gather it and turn fusion off everywhere unless
  // every rank fits every shape (a rank falling back alone would leave its peers waiting on flags)
  std::vector<int> tp_fuse_fits();
  void disable_tp_fuse() { tp_fuse_ = nullptr; }
  // fp8 KV: the per-layer (K, V) scales, 2 x n_layers values (value = code x scale; captured decode
  // graphs are dropped, they hold the old ones).  1.0 until set, which is NOT adequate in general:
  // at 1.0 e4m3 loses mantissa bits below 2^-6, flushes to zero below 2^-9 and saturates at 448, and a
  // checkpoint's post-RoPE keys or its values can leave that window layer by layer.  The runtime
  // loader therefore calibrates (calibrate_kv_scales) unless the config turns it off.
  void set_kv_scales(const std::vector<float>& s);
  std::vector<float> kv_scales() const { return kv_scale_; }
  // fp8 KV calibration at load: prefill `tokens` into a free slot (throws when every slot holds
  // blocks; nothing is evicted) with the KV writers' observer on -- every prefill path routes K / V
  // through launch_qkv_post meanwhile -- which records max |value| per (layer, K / V, KV head) on the
  // device.  Per layer: scale = max over heads x headroom / 448 (headroom 2: one e4m3 binade kept
  // free for tokens the prompt did not contain); a layer that saw only zeros keeps 1.0, a non-finite
  // maximum throws and names the layer.  The codes written meanwhile used the old scales: the slot is
  // released again.  Installs the scales through set_kv_scales and returns them.  Static, per layer,
  // from one prompt: no per-head or per-token scales.
  std::vector<float> calibrate_kv_scales(const std::vector<int>& tokens, float headroom = 2.f);
  // the table the last calibration observed, n_layers x 2 x n_kv_heads (empty before any)
  std::vector<float> kv_amax() const { return kv_amax_; }
  int kv_fp8() const { return cfg_.kv_fp8; }
  bool vocab_parallel() const { return cfg_.vocab_parallel != 0; }
  void reset_graphs();
  int capture_graphs(int max_b);  // pre-capture the decode-step graphs of B = 1..max_b (masked + unmasked)
  // ---- paged KV (block table per slot; see kv_offset in common.h) --------------------------------
  // prefix sharing: dst's positions [0, n) become src's -- full blocks shared (refcounted, never
  // written again by either slot: writes un-share first), the partial last block copied
  void copy_slot(int src, int dst, int n_tokens);
  void release_slot(int slot);         // drop every block reference of the slot
  // Context shift (ops.h KvShiftArgs: the rule): the slot's positions [n_keep + n_discard, n_tokens) move down
  // by n_discard, K re-rotated, in place; returns the new length n_tokens - n_discard.  The blocks of
  // [n_keep, new length) are mapped and un-shared first (a shared prefix block is never written through; the
  // blocks above are only read), the blocks wholly above the new length are unreferenced and unmapped
  // afterwards, and the device tables are uploaded again, the decode rows' included, before the call returns
  // (the captured decode graphs read them in place).  n_keep + n_discard == n_tokens only truncates.  Decode
  // rows of the slot are moved back to the new length: the slot's next step must be host-fed (explicit token
  // and position).  Throws before any table, refcount or cache byte changes on: a bad slot, n_tokens outside
  // [1, max_ctx], n_keep < 0, n_discard < 1, n_keep + n_discard > n_tokens, a pipelined step in flight
  // (sampled by decode_sample and not yet collected), an engine that is not finalized or is tensor-parallel,
  // a pool without the free blocks the un-sharing needs.
  int shift_context(int slot, int n_tokens, int n_keep, int n_discard);
  // KV snapshots (ops.h KvSnapArgs: the payload).  kv_snapshot_bytes: the exact payload size of n_tokens
  // positions.  kv_save: the slot's positions [0, n_tokens) into out, byte for byte what kv_read returns, one
  // pack launch and one device-to-host copy per layer.  Staging is bounded: one layer's K and V on the device and
  // two pinned host buffers of that size, grown on demand and kept; never a second copy of the slot.
  // kv_restore: the blocks of [0, n_tokens) are mapped and un-shared first (a shared prefix block is never
  // written through), the slot's blocks above ceil(n_tokens / KV_BLOCK) are unreferenced and unmapped, the data
  // is unpacked layer by layer and the device tables are uploaded again, the decode rows' included (the captured
  // decode graphs read them in place).  Decode rows of the slot are moved back to n_tokens: the slot's next step
  // must be host-fed.  Both throw before any table, refcount or cache byte changes on: a bad slot, n_tokens
  // outside [1, max_ctx], a size other than kv_snapshot_bytes(n_tokens), a pipelined step in flight, an engine
  // that is not finalized or is tensor-parallel, (restore) a pool without the free blocks the mapping needs.
  size_t kv_snapshot_bytes(int n_tokens) const;
  void kv_save(int slot, int n_tokens, void* out, size_t out_bytes);
  void kv_restore(int slot, const void* data, size_t data_bytes, int n_tokens);
  int kv_blocks_free() const { return (int)free_blocks_.size(); }
  int kv_blocks_total() const { return kv_nblocks_; }
  int norm_fused_parts() const { return nrm_parts_; }  // 0: batched-decode RMSNorm not split into the GEMMs
  std::vector<int> block_table(int slot) const;
  // read-only views of the cache for tests (host copies after a stream synchronise; raw bf16 / fp8 bytes):
  // kv_read: positions [0, n_tokens) of a slot gathered through its host table, [layer][K, V][kv_head][token]
  // [head_dim] (an unmapped block reads as the null block); kv_read_block: one physical block, [layer][K, V]
  // [kv_head][KV_BLOCK][head_dim] (block == kv_blocks_total: the null block)
  std::vector<uint8_t> kv_read(int slot, int n_tokens) const;
  std::vector<uint8_t> kv_read_block(int block) const;
  // the tables as the kernels see them, read back from the device: the slot table [max_slots][max_ctx / KV_BLOCK],
  // then the first B rows of the decode batch's row table (unmapped entries: kv_blocks_total).  They are what
  // kv_sync last uploaded: release_slot alone uploads nothing
  std::vector<int> kv_device_tables(int B) const;

  // raw device pointers for tests / custom kernels
  uintptr_t kv_cache_k() const { return (uintptr_t)k_cache_; }
  uintptr_t kv_cache_v() const { return (uintptr_t)v_cache_; }

 private:
  void enqueue_decode_step(int B, bool masked);  // uses device arrays d_tokens_/d_pos_/d_seqlen_/d_slot_
  void enqueue_decode_forward(int B);            // ... up to the logits (no sampler)
  // what every sampler launch shares: logits_, the parameter block's row arrays, workspace and tickets
  // (mask: d_mask_ or null)
  SampleArgs sample_args(int B, bool masked) const;
  // the fields the launches differ in -- STEP (decode, decode_sample, spec_decode): the device seed, d_pos_,
  // sequence lengths and history, advancing; AGAIN (resample): the device seed and d_pos_, no advance; FIRST
  // (sample_first): d_fpos_ and the row seed alone, no advance
  enum SampleKind { SAMPLE_STEP, SAMPLE_AGAIN, SAMPLE_FIRST };
  // THE sampler launch.  staged: the staged processors go in front of it and the staged logprob launch
  // behind it; the captured step graph passes false and holds the sampler alone
  void enqueue_sample(int B, bool masked, SampleKind kind = SAMPLE_STEP, bool staged = false);
  // the staged logit processors of a B-row sampler launch: uploads them, points s at them and
  // un-stages them (no-op when nothing is staged)
  void take_processors(SampleArgs& s, int B);
  char* h_proc_ = nullptr;               // pinned staging: [4][max_batch] floats | [rows][stride] window ints
  char* d_proc_ = nullptr;               // | [rows][bias stride] bias ids | [rows][bias stride] bias floats
  int proc_rows_ = 0, proc_stride_ = 0;  // rows staged (0: none) and their window stride
  int proc_bias_stride_ = 0;             // the staged rows' bias-list stride (0: no row has a bias)
  void take_logprobs(int B);             // after a B-row sampler launch: the staged logprob launch + its copy
  int lp_rows_ = 0;                      // rows staged by set_logprobs (0: none)
  // A sampler-launching call's hold on the staged processors and logprobs, taken before it changes any
  // state: refuses (and drops both) when either was staged for another batch size, and drops both when the
  // call ends, however it ends -- a call that throws half way never leaves them to a later, unrelated launch.
  struct SampleStage {
    Engine& e;
    SampleStage(Engine& eng, int B, const char* who) : e(eng) {
      const char* bad = e.proc_rows_ && e.proc_rows_ != B ? "sample processors"
                        : e.lp_rows_ && e.lp_rows_ != B   ? "logprobs"
                        : e.gr_rows_ && e.gr_rows_ != B   ? "grammar rows" : nullptr;
      if (!bad) return;
      e.proc_rows_ = e.lp_rows_ = e.gr_rows_ = 0;
      throw std::runtime_error(std::string(who) + ": " + bad + " staged for another batch size");
    }
    ~SampleStage() { e.proc_rows_ = e.lp_rows_ = e.gr_rows_ = 0; }
  };
  // DFA grammars: the vocabulary table, the loaded grammars (one device buffer each) and their device descriptors,
  // the staged rows (pinned, two halves: a staging may follow one whose copy is still queued)
  struct GrammarSlot {
    void* buf = nullptr;  // byte_class[256] | trans | accept
    int n_states = 0, n_classes = 0;
  };
  std::vector<GrammarSlot> grammars_;
  GrammarTable* d_grammars_ = nullptr;   // [GRAMMAR_MAX]
  int* d_tok_off_ = nullptr;             // [V + 1]
  uint8_t* d_tok_bytes_ = nullptr;
  int gr_eos_[GRAMMAR_MAX_EOS] = {0};
  int gr_n_eos_ = 0;
  int* h_gr_ = nullptr;                  // pinned [2][2][max_batch]: gid | state
  int* d_gr_ = nullptr;                  // [2][max_batch]
  int gr_rows_ = 0, gr_buf_ = 0;         // rows staged by set_grammar_rows (0: none) and the half they are in
  GrammarMaskArgs grammar_args(int B, const int* gid, const int* state, uint8_t* mask, bool fill_free) const;
  // the staged grammar rows of a B-row sampler launch: their upload and the mask kernel, un-staged; false when
  // nothing is staged (host_mask: the call copied mask bytes of its own into d_mask_)
  bool take_grammar(int B, bool host_mask);
  std::vector<int> lp_last_;             // top_n of the rows the last sampler launch reported (empty: none)
  char* h_lp_ = nullptr;                 // pinned: [max_batch] top_n | the device output block's mirror
  char* d_lp_out_ = nullptr;             // [max_batch][LOGPROB_ROW] floats | [max_batch][LOGPROB_ROW] ids
  int* d_lp_topn_ = nullptr;
  void* lp_ws_ = nullptr;
  size_t lp_ws_bytes_ = 0;
  int* lp_cnt_ = nullptr;
  hipGraphExec_t forward_graph(int B);
  hipGraphExec_t graph_for(int key, const std::function<void()>& enqueue);  // captured once per key
  int cus_ = 0;                          // CUs of the stream's mask (0: the whole device)
  int kv_es_ = 2;                        // bytes per KV element (2 bf16, 1 fp8)
  std::vector<float> kv_scale_;          // [n_layers][K, V] fp8 scales (value = code * scale)
  std::vector<float> kv_amax_;           // [n_layers][K, V][n_kv_heads] of the last calibration
  unsigned* d_kv_amax_ = nullptr;        // its device table (float bit patterns; fp8 engines only)
  bool kv_obs_ = false;                  // calibration prefill running: observer on, K / V via qkv_post
  unsigned* kv_obs_table(int l) const { return kv_obs_ ? d_kv_amax_ + (size_t)l * 2 * cfg_.n_kv_heads : nullptr; }
  bf16_t* kv_layer(bf16_t* base, int l) const {  // layer l's pool (element indices as bf16, bytes as kv_es_)
    return (bf16_t*)((char*)base + (size_t)l * layer_kv_elems_ * kv_es_);
  }
  template <typename T>
  void kv_write_args(T& a, int l) const {
    a.kv_fp8 = cfg_.kv_fp8;
    a.kv_inv_k = 1.f / kv_scale_[2 * l];
    a.kv_inv_v = 1.f / kv_scale_[2 * l + 1];
  }
  template <typename T>
  void kv_read_args(T& a, int l) const {
    a.kv_fp8 = cfg_.kv_fp8;
    a.kv_scale_k = kv_scale_[2 * l];
    a.kv_scale_v = kv_scale_[2 * l + 1];
  }
  int pipe_B_ = 0;                       // rows of the last submitted step (decode_sample's rows; never reset)
  bool pipe_sampled_ = false;            // decode_sample ran and decode_collect has not: a step is in flight
  int par_buf_ = 0;                      // which half of the double-buffered pinned parameter block
  uint8_t* h_mask_ = nullptr;            // pinned staging of the pipelined sampler's masks
  hipEvent_t pipe_ev_ = nullptr;         // the pipelined sampler's token copy
  bool gemm_prefill_ok(int T) const;
  // what embed_prefill / score_prefill do with each chunk's hidden rows (embed_fold / score_fold)
  struct EmbedFold {
    int slot, pooling;
    bool final;
  };
  struct ScoreFold {
    int top_n;
    int T;  // rows of the call (the staged results' layout)
  };
  // A prefill call's per-chunk consumer, run on the host after each chunk's layers were enqueued.
  struct ChunkHook {
    // x[n][d]: the chunk's hidden rows, rows [row0, row0 + n) of the call; last: the call's last chunk
    // (null: plain prefill, nothing is enqueued for it)
    std::function<void(const float* x, int n, int row0, bool last)> fn;
    // chunks that reach the prefill GEMM (more than 32 rows) ask for its plans without split-K / stream-K
    bool deterministic = false;
  };
  // prefill()'s body: validate, map the KV blocks, one of the two bodies below, the logits' copy-out
  std::vector<float> prefill_run(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits,
                                 const ChunkHook& hook);
  void prefill_gemm(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits, const ChunkHook& hook);
  // short prompts / engines without the GEMM path: sub-batches of <= 8 rows through the GEMVs, on the pf_*
  // buffers only (no decode workspace member is read or written)
  void prefill_gemv(int slot, const std::vector<int>& tokens, int start_pos, bool want_logits, const ChunkHook& hook);
  // n hidden rows x[n][d], rows [row0, row0 + n) of the call being scored
  void score_fold(const ScoreFold& f, const float* x, int n, int row0);
  void score_lm_head(int n, const float* x, int ldx);  // sc_logits_[n][V] = rmsnorm(x) . output^T
  void score_buffers();                    // allocated by the first score_prefill
  int sc_rows_ = 0;                        // rows of the scoring logits buffer = rows per lm_head group
  float* sc_logits_ = nullptr;             // [sc_rows_][V]
  int* sc_targets_ = nullptr;              // [max_ctx] the call's targets
  char* sc_out_ = nullptr;                 // the call's staged results: [T][2] f | [T][2] i | [T][LOGPROB_ROW] f | ... i
  int* sc_topn_ = nullptr;                 // [sc_rows_] the logprob launch's per-row top_n
  void* sc_lp_ws_ = nullptr;               // its workspace and tickets for sc_rows_ rows (vocabularies it takes)
  size_t sc_lp_ws_bytes_ = 0;
  int* sc_lp_cnt_ = nullptr;
  int sc_topn_val_ = -1;                   // the value sc_topn_ holds
  // n hidden rows x[n][d] of positions [pos0, pos0 + n) of f.slot; last: the call's last chunk
  void embed_fold(const EmbedFold& f, const float* x, int n, int pos0, bool last);
  void embed_buffers(bool rows);           // allocated by the first embed_prefill (rows: by the first EMBED_NONE)
  float* emb_acc_ = nullptr;               // [max_slots][d] running sums of x / rms
  int* emb_count_ = nullptr;               // [max_slots] rows folded (device; the kernel's count)
  float* emb_out_ = nullptr;               // [d] the unit vector of a final call
  float* emb_rows_ = nullptr;              // [max_ctx][d] EMBED_NONE's staged rows, one buffer for every slot
  int emb_rows_slot_ = -1;                 // the slot whose rows it holds
  float* emb_ws_ = nullptr;                // embed_pool_ws_bytes(d)
  int* emb_cnt_ = nullptr;                 // the pool kernel's ticket
  std::vector<int> emb_pos_, emb_mode_;    // [max_slots] position reached (-1: no state) and its pooling
  int emb_tokens_ = 0;
  void layer_decode(int l, int B);
  // ---- launch descriptors: one builder each, from (layer, rows, explicit buffers) ----
  // one QKV group (qkv_groups) of layer l for B rows of x[B][d]: fused = RoPE + KV write in the epilogue
  // (q out, pos / slot read), else the packed rows into qkv for qkv_post.  No knobs: the caller's.
  GemvArgs qkv_gemv_args(int l, const std::vector<const QMat*>& grp, int row0, int B, const float* x, bool fused,
                         float* q, float* qkv, const int* pos, const int* slot);
  QkvPostArgs qkv_post_args(int l, const float* qkv, int ldqkv, int T, const int* pos, const int* slot, float* q_out,
                            const float* bias, unsigned* amax) const;
  AttnDecodeArgs attn_decode_args(int l, int B, const float* q, float* out, const int* seq_len, const int* slot,
                                  const int* block_table, int bt_rows, float* o_part, float* ml,
                                  bf16_t* out16 = nullptr) const;
  // single-matrix skinny / prefill GEMM: C[M][N] (ldc) = A[M][K] . w^T with epilogue epi
  static GemmQArgs gemm_args(const bf16_t* A, int lda, int M, int K, const QWeight& w, int N, int ldc, float* C, int epi);
  // the stacked Q / K / V GEMM of layer l, and its RoPE + q store + KV-write epilogue (GEPI_QKV)
  GemmQArgs qkv_gemm_args(int l, const bf16_t* A, int M, float* C) const;
  void qkv_gemm_epi(GemmQArgs& g, int l, const int* pos, const int* slot, float* q_out) const;
  // RMSNorm split across two GEMMs: the residual GEMM (O, down) also writes bf16(x * g_next) to xn16 and
  // per-tile row sums of squares to part; the next GEMM reads xn16 as A and scales its rows by the inverse RMS
  struct SplitNorm {
    bf16_t* xn16;
    float* part;
    int parts;
  };
  void nrm_consume(GemmQArgs& g, const SplitNorm& n) const;
  static void nrm_produce(GemmQArgs& g, const SplitNorm& n, const float* g_next);
  // the step parameter block: 8 bytes of seed, PAR_ROWS arrays of max_batch 4-byte entries, the per-row
  // seeds (par_seeds_off_), the masks (par_mask_off_) -- finalize points the d_* members at the same offsets
  enum { PAR_SLOT, PAR_TOKEN, PAR_POS, PAR_SEQLEN, PAR_TOPK, PAR_TEMP, PAR_TOPP, PAR_ROWS };
  size_t par_off(int array) const { return 8 + (size_t)array * cfg_.max_batch * 4; }
  size_t par_seeds_off_ = 0;
  char* next_par() { return h_par_ + (size_t)(par_buf_ ^= 1) * par_bytes_; }  // flips to the other pinned half
  void par_copy(const char* hpar, size_t from, size_t to);  // bytes [from, to) of that half to the device block
  // decode's and decode_submit's checks of a step's rows (tokens may be empty only when !need_tokens)
  void check_step(const std::string& who, const std::vector<int>& slots, const std::vector<int>& tokens,
                  const std::vector<int>& pos, const std::vector<uint64_t>& seeds, bool need_tokens) const;
  // B rows' sampling parameters into the pinned block at hpar: the seed, top_k / temperature / top_p (missing
  // entries: 0 / 0 / 1) and the row seeds
  void write_sample_params(char* hpar, int B, const std::vector<float>& temperature, const std::vector<int>& top_k,
                           const std::vector<float>& top_p, uint64_t seed, const std::vector<uint64_t>& seeds);
  // those and a step's rows (tokens empty: that array is left alone)
  void write_step_params(char* hpar, const std::vector<int>& slots, const std::vector<int>& tokens,
                         const std::vector<int>& pos, const std::vector<float>& temperature,
                         const std::vector<int>& top_k, const std::vector<float>& top_p, uint64_t seed,
                         const std::vector<uint64_t>& seeds);
  // a step's upload: write_step_params into the next pinned half, the mask behind it when there is one, one
  // copy (tokens empty: two, around the array the last sampler left on the device)
  void upload_step_params(const std::vector<int>& slots, const std::vector<int>& tokens, const std::vector<int>& pos,
                          const std::vector<float>& temperature, const std::vector<int>& top_k,
                          const std::vector<float>& top_p, uint64_t seed, const std::vector<uint64_t>& seeds,
                          const std::vector<uint8_t>& mask = {});
  // a sampler-only call's upload (resample, sample_first): write_sample_params into the next pinned half, one
  // copy of top_k .. top_p (up to row B of top_p), one of the row seeds, one of the seed when dev_seed -- never
  // slot / token / pos / seq_len, which a pipelined decode_submit(tokens = {}) continues from
  void upload_sample_params(int B, const std::vector<float>& temperature, const std::vector<int>& top_k,
                            const std::vector<float>& top_p, uint64_t seed, const std::vector<uint64_t>& seeds,
                            bool dev_seed);
  // map (and un-share) the blocks the B rows' next n positions write, before anything that writes them is
  // enqueued, and move the rows' host positions there
  void advance_rows(int B, int n);
  void gemv(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx, const float* norm_w,
            float* y, int ldy, int epi, int layer);
  GemvArgs gemv_args(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx,
                     const float* norm_w, float* y, int ldy, int epi, int layer);  // gemv_base + the shape's knobs
  GemvArgs gemv_base(const std::vector<const QMat*>& segs, int N, int K, int B, const float* x, int ldx,
                     const float* norm_w, float* y, int ldy, int epi, int layer) const;
  QMat alloc_qmat(int qt, int rows, int cols);
  QMat upload_qmat(int qt, int rows, int cols, const void* host, size_t nbytes);
  // load-time staging: two device buffers (tensor i repacks while i+1 uploads) fed through two
  // pinned 64 MB host chunks
  void stage_upload(const void* host, size_t nbytes, void*& dev_staging);
  void stage_done();
  void stage_release();
  void* stage_dev_[2] = {nullptr, nullptr};
  size_t stage_dev_bytes_[2] = {0, 0};
  hipEvent_t stage_ev_[2] = {nullptr, nullptr};
  void* stage_host_[2] = {nullptr, nullptr};
  hipEvent_t stage_host_ev_[2] = {nullptr, nullptr};
  int stage_next_ = 0, stage_host_next_ = 0, stage_cur_ = 0;
  float* upload_f32(const void* host, size_t n, int qt);
  QMat interleave_rows(const QMat& a, const QMat& b);
  void* dmalloc(size_t bytes);
  void tune_prefill_gemm();  // measured prefill-GEMM plans for this model's projection shapes
  void allreduce(float* p, size_t n, float* residual);
  void lm_head(int B, const float* x, int ldx);  // logits_[B][V] (vocab-parallel aware)

  EngineConfig cfg_;
  hipStream_t stream_ = nullptr;

  bool finalized_ = false;
  std::vector<void*> allocs_;
  size_t weight_bytes_ = 0, kv_bytes_ = 0, ws_bytes_ = 0;

  QMat tok_embd_, output_;
  float* out_norm_ = nullptr;
  std::vector<LayerW> layers_;
  std::map<std::string, QMat> pending_;  // gate/up waiting for their partner

  bf16_t* k_cache_ = nullptr;
  bf16_t* v_cache_ = nullptr;
  size_t layer_kv_elems_ = 0;

  // workspace
  float *x_ = nullptr, *q_ = nullptr, *attn_ = nullptr, *ff_ = nullptr, *qkv_ = nullptr;
  // the GEMV path's SwiGLU hand-off in bf16 (gate/up epilogue -> down staging: half the bytes every
  // down workgroup re-reads; AIOS_FF16=0 keeps fp32), [max_batch][d_ff]
  bf16_t* gv_ff16_ = nullptr;
  float *opart_ = nullptr, *ml_ = nullptr, *logits_ = nullptr;
  int *d_tokens_ = nullptr, *d_pos_ = nullptr, *d_seqlen_ = nullptr, *d_slot_ = nullptr, *d_history_ = nullptr;
  int *d_topk_ = nullptr, *d_step_ = nullptr;
  float* d_temp_ = nullptr;
  float* d_topp_ = nullptr;
  char* d_par_ = nullptr;          // per-step parameter block (seed, slot, token, pos, seq_len, top_k, T, top_p | masks)
  char* h_par_ = nullptr;          // pinned mirror
  int* h_tok_out_ = nullptr;       // pinned sampled tokens
  int* d_spec_ = nullptr;          // spec_decode: [SPEC_MAX_ROWS] input tokens | [SPEC_RECORD] the accept record
  int* h_spec_ = nullptr;          // its pinned mirror
  int* d_specm_ = nullptr;         // spec_decode_multi: [SPEC_MULTI_MAX_ROWS] input tokens | [SPEC_MULTI_MAX_SEQS] records
  int* h_specm_ = nullptr;         // its pinned mirror
  size_t par_bytes_ = 0, par_mask_off_ = 0;
  void* sample_ws_ = nullptr;
  size_t sample_ws_bytes_ = 0;
  int* sample_cnt_ = nullptr;
  uint64_t* d_seed_ = nullptr;
  uint64_t* d_seeds_ = nullptr;    // [max_batch] per-row sampling seeds (in the parameter block)
  int* d_fpos_ = nullptr;          // sample_first's RNG position
  // StepPrep outputs of the decode step's embedding launch: [max_batch][2] {pos, KV block} and
  // [max_batch][head_dim / 2] rope rows, read by the batch-1 QKV epilogue while step_prep_on_
  int* d_step_kv_ = nullptr;
  float2* d_step_rope_ = nullptr;
  bool step_prep_on_ = false;
  void fill_row_seeds(uint64_t* host_seeds, int B, uint64_t seed, const std::vector<uint64_t>& seeds);
  uint8_t* d_mask_ = nullptr;
  int n_chunks_ = 0;
  int* attn_cnt_ = nullptr;  // [max(prefill_rows, max_batch)][n_kv_heads] combine tickets
  float2* rope_cs_ = nullptr;  // [max_ctx][head_dim/2] cos/sin computed in double on the host
  int prefill_rows_ = 64;  // rows of the prefill workspace
  float *pf_x_ = nullptr, *pf_q_ = nullptr, *pf_attn_ = nullptr, *pf_ff_ = nullptr, *pf_qkv_ = nullptr;
  float *pf_opart_ = nullptr, *pf_ml_ = nullptr;
  bf16_t* pf_a16_ = nullptr;
  // GEMM prefill workspace (chunks of gm_rows_ tokens through MFMA GEMMs + flash attention)
  int gm_rows_ = 512;
  // prompts shorter than this take the GEMV path, whose batched LDS-DMA engine serves up to 4 rows
  // (tools/bench_prefill.py, round 3: 2 / 3 / 4 tokens 1.85 / 2.02 / 2.29 ms there vs 3.25 ms for 4 through
  // the skinny GEMM; from 5 rows the GEMV falls back to the row kernels, 8.5 ms, the GEMM 3.25)
  int gm_min_rows_ = 5;
  bool gm_ok_ = false;    // every layer's weights / head shape supported
  float *gm_x_ = nullptr, *gm_qkv_ = nullptr, *gm_q_ = nullptr, *gm_part_ = nullptr;
  bf16_t *gm_a16_ = nullptr, *gm_ff16_ = nullptr, *gm_attn16_ = nullptr;
  int *gm_tokens_ = nullptr, *gm_pos_ = nullptr, *gm_slot_ = nullptr;
  // chunks of <= 64 rows: the residual GEMMs' bf16(x * g_next) + per-tile sums (split RMSNorm)
  bf16_t* gm_xn16_ = nullptr;
  float* gm_npart_ = nullptr;
  int gm_nparts_ = 0;
  const ArDevCtx* tp_fuse_ = nullptr;
  int tp_fuse_grid_ = 0;
  bool tp_fuse_gemv(GemvArgs a);  // EPI_TP_RESID launch when the engine serves the shape (else false)
  // batched decode through the skinny MFMA GEMM (B >= dec_gemm_min_b_): bf16 activation buffers
  // (MI355X, Mistral-7B Q4_K_M, tools/gpu_batch_ab.sh: B=2 GEMV 2.41 ms vs GEMM 3.25 ms, B=4 3.31 vs 3.26,
  // B=8 5.80 vs 3.37 -- the skinny GEMM's per-step dequant floor lost below 4 rows; after the split
  // RMSNorm / mixed-QKV / split-K work, tools/gpu_minb_ab.sh: B=3 GEMV 956 vs GEMM 1065 tok/s, B=2 829 vs 712)
  // round 3: the LDS-DMA GEMV engine serves B = 2..4 from one weight stream (gemv_lds.h):
  // B = 2 / 3 / 4 1.82 / 2.29 / 2.45 ms vs the skinny GEMM's 3.25 / 2.83 / 2.84 (profiles/lds_batched_r3.txt)
  int dec_gemm_min_b_ = 5;
  bf16_t *dec_a16_ = nullptr, *dec_ff16_ = nullptr;
  // split-K slabs + arrival tickets of the skinny GEMM (shared by every decode GEMM of a step)
  float* gk_ws_ = nullptr;
  size_t gk_ws_bytes_ = 0;
  int* gk_cnt_ = nullptr;
  int gk_cnt_len_ = 0;
  void gemm(GemmQArgs& g);  // launch_gemm_q with the engine's split-K workspace
  // RMSNorm split across the skinny GEMMs (AIOS_GEMM_NORM_FUSE, default on): the residual GEMMs
  // (O, down) also write bf16(x * g_next) to dec_xn16_ and per-tile row sums of squares to
  // nrm_part_; the next GEMM (gate/up, next layer's QKV, lm_head) scales its rows by the inverse
  // RMS in the epilogue -- two normalisation launches per layer less
  bf16_t* dec_xn16_ = nullptr;
  float* nrm_part_ = nullptr;
  int nrm_fuse_ = 1;
  int nrm_parts_ = 0;  // tiles of the d_model-wide producer GEMM (0: fusion unavailable)
  bool nrm_on(int B) const;
  bool tpn_on(int B) const;  // batched TP decode: C1 / C2 fused with the next RMSNorm
  void layer_decode_gemm(int l, int B);
  hipGraphExec_t step_graph(int B, bool masked);
  void decode_loop_body(int B, int n_steps, bool use_graph, bool masked);  // decode_loop_run, with the steps' mask flag
  bool nrm_lm_ = false;  // the last layer's down GEMM prepared dec_xn16_ / nrm_part_ for lm_head(x_)
  int *pf_tokens_ = nullptr, *pf_pos_ = nullptr, *pf_seqlen_ = nullptr, *pf_slot_ = nullptr;

  // paged KV state: host tables are the truth, device copies uploaded (stream idle) when dirty
  int kv_maxb_ = 0;                // blocks per slot = max_ctx / KV_BLOCK
  int kv_nblocks_ = 0;             // allocatable blocks per layer pool (+1 null block at the end)
  std::vector<int> bt_;            // [max_slots][kv_maxb_], -1 = unmapped
  std::vector<int> refcnt_;        // [kv_nblocks_]
  std::vector<int> free_blocks_;
  std::vector<int> row_bt_host_;   // [max_batch][kv_maxb_] as last uploaded
  int* d_bt_ = nullptr;            // [max_slots][kv_maxb_] slot-indexed (unmapped -> null block)
  int* d_row_bt_ = nullptr;        // [max_batch][kv_maxb_] rows of the decode batch
  bool bt_dirty_ = false;
  std::vector<int> row_slots_, row_pos_;  // decode rows: slot and host-tracked next position
  const int* attn_bt_ = nullptr;   // table the decode attention reads (rows / slot indexed)
  int attn_bt_rows_ = 1;
  int kv_alloc();
  void kv_unref(int blk);
  void kv_copy_block(int src, int dst);
  void kv_prepare_write(int slot, int from, int to);  // map + un-share the blocks of [from, to)
  void kv_sync(int B);                                 // upload dirty tables (rows 0..B-1)
  float* d_shift_kscale_ = nullptr;                    // [n_layers] the K scales shift_context's launch reads (fp8)
  // kv_save / kv_restore staging: one layer's K and V on the device, two pinned host buffers of that size
  void* snap_dev_ = nullptr;
  void* snap_host_[2] = {nullptr, nullptr};
  hipEvent_t snap_ev_[2] = {nullptr, nullptr};
  size_t snap_cap_ = 0;
  void snap_check(const char* who, int slot, int n_tokens, size_t bytes) const;
  void snap_reserve(size_t layer_bytes);
  void snap_launch(int slot, int layer, int n_tokens, bool unpack);

  std::map<int, hipGraphExec_t> graphs_;
  AllReduceFn allreduce_ = nullptr;
  void* allreduce_ctx_ = nullptr;
  AllGatherFn allgather_ = nullptr;
  AllReduceNormFn allreduce_norm_ = nullptr;
  void* allreduce_norm_ctx_ = nullptr;
  // batched TP decode: the fused all-reduce's split-norm partials [max_batch][tpn_parts_] (0: off)
  int tpn_parts_ = 0;
  float* tpn_part_ = nullptr;
  SplitNorm lm_nrm_{};  // the split-norm operands the lm_head consumes when nrm_lm_ is set (nrm_part_ or tpn_part_)
  void* allgather_ctx_ = nullptr;
};

}  // namespace aios
