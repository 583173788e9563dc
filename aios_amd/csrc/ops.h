// Host launchers for every device op of the engine (one header so the engine, the bindings and
// the tests see the same signatures).  All launchers are stream-ordered and capture-safe: no
// allocation, no synchronisation (CDNA guide §6 Guideline 9), so the decode step can be captured
// into a hipGraph.
#pragma once
#include "common.h"
#include <vector>
#include "gemv.h"
#include "qweight.h"

namespace aios {

// ---- weights -------------------------------------------------------------------------------
void launch_repack(int qt, const void* raw, size_t nblocks, const QWeight& w, hipStream_t st);
void launch_get_rows(const QWeight& w, const int* rows, int nrows, float* out, int ldo, float scale,
                     hipStream_t st);
// Per-step lookups the batch-1 QKV epilogue needs, done by the step's first (embedding) launch while
// it gathers the rows: kv[b] = {pos[b], physical KV block of (slot[b], pos[b])}, rope[b][:] = the
// (cos, sin) row of pos[b].  Every layer's QKV GEMV then loads them with no dependent round trip.
struct StepPrep {
  const int* pos;          // [B]
  const int* slot;         // [B] or null (row b)
  const int* block_table;  // [slots][maxb] or null (identity)
  int maxb;
  const float2* rope_cs;   // [max_ctx][half] or null (no rope rows)
  int half;
  int* kv;                 // out [B][2]
  float2* rope;            // out [B][half]
};
void launch_get_rows_step(const QWeight& w, const int* rows, int nrows, float* out, int ldo, float scale,
                          const StepPrep& prep, hipStream_t st);
void launch_dequant_bf16(const QWeight& w, void* out, hipStream_t st);
void launch_legacy_to_bf16(int qt, const void* raw, size_t n, void* out, hipStream_t st);
void fill_random_weight(const QWeight& w, uint64_t seed, float amp, hipStream_t st);
void fill_random_f32(float* p, size_t n, uint64_t seed, float base, float amp, hipStream_t st);
bool gemv_supports(int qt0, int qt1);

// ---- elementwise / norms ---------------------------------------------------------------------
// y[b] = x[b] * rsqrt(mean(x^2)+eps) * w     (rows of length n, row strides ldx/ldy)
void launch_rmsnorm(const float* x, int ldx, const float* w, float* y, int ldy, int rows, int n, float eps,
                    hipStream_t st);
// same, bf16 output (GEMM A operand)
void launch_rmsnorm_bf16(const float* x, int ldx, const float* w, bf16_t* y, int ldy, int rows, int n, float eps,
                         hipStream_t st);
void launch_f32_to_bf16(const float* x, bf16_t* y, size_t n, hipStream_t st);
void launch_add(float* y, const float* x, size_t n, hipStream_t st);

// Producer side of the split RMSNorm after a TP all-reduce (the skinny GEMM's nrm_in contract,
// GemmQArgs below): out16[m][:] = bf16(x_new[m][:] * g) and part[m * parts + j] = sum of x_new^2 over
// the j-th 1024-column block of row m (parts = round_up(d / 1024, 4) <= 64, the tail parts zero).
constexpr int RNORM_COLS = 1024;
struct ResidNorm {
  const float* g;   // [d] RMSNorm weight of the consumer
  bf16_t* out16;    // [rows][ld16]
  int ld16;
  float* part;      // [rows][parts]
  int parts;
};
inline int resid_norm_parts(int d) { return d % RNORM_COLS ? 0 : ((d / RNORM_COLS + 3) & ~3); }
// residual[m][:] += data[m][:] (data may be null: residual already holds the sum), then the outputs above
void launch_add_norm(float* residual, const float* data, int rows, int d, const ResidNorm& nm, hipStream_t st);

// out[b][i] = silu(gu[b][2i]) * gu[b][2i+1]
void launch_swiglu_interleaved(const float* gu, int ldg, float* out, int ldo, int rows, int n, hipStream_t st);
void launch_swiglu_interleaved_bf16(const float* gu, int ldg, bf16_t* out, int ldo, int rows, int n, hipStream_t st);

// Per-head: optional RMSNorm(q/k heads) + RoPE + Q store + K/V cache write, from a packed
// qkv row [B][q_dim + 2 kv_dim] (used for Qwen3 QK-norm and the prefill GEMM path).
struct QkvPostArgs {
  const float* qkv;  // [T][ldqkv]
  int ldqkv;
  int T;
  int n_heads, n_kv_heads, head_dim;
  const float* bias = nullptr;  // [q_dim + 2 kv_dim] or null (added before norm / RoPE)
  const float* q_norm;  // [head_dim] or null
  const float* k_norm;
  float eps;
  int rope_neox;
  float rope_base;
  const float2* rope_cs;  // [max_ctx][head_dim/2] table or null
  const int* pos;    // [T]
  const int* slot;   // [T] or null (0)
  float* q_out;      // [T][n_heads*head_dim]
  bf16_t* k_cache;   // layer base of the paged pool [blocks][n_kv][KV_BLOCK][hd]
  bf16_t* v_cache;
  int max_ctx;
  const int* block_table = nullptr;  // [slots][max_ctx / KV_BLOCK] or null (identity)
  int kv_fp8 = 0;    // fp8 e4m3 pool: code = value * kv_inv_{k,v}
  float kv_inv_k = 1.f, kv_inv_v = 1.f;
  // fp8 calibration observer (null: off): the layer's [2][n_kv_heads] table of max |value| about to
  // be stored (K row 0, V row 1; after bias / QK-norm / RoPE, before the fp8 conversion), kept as the
  // bit patterns of the non-negative floats (they order like unsigned integers; a NaN sorts above
  // every finite value and so stays visible) -- the launch takes the observing kernel variants
  unsigned* amax = nullptr;
};
void launch_qkv_post(const QkvPostArgs& a, hipStream_t st);
// fp8 KV calibration: per-layer (K, V) scales, 2 x n_layers values, from an observed table
// amax[n_layers][2][n_kv_heads]: scale = max over heads x headroom / 448 (e4m3's largest finite
// value); a layer / part that saw only zeros keeps 1.0; a non-finite entry throws, naming the layer
std::vector<float> kv_scales_from_amax(const std::vector<float>& amax, int n_layers, int n_kv_heads, float headroom);

// ---- attention ---------------------------------------------------------------------------------
struct AttnDecodeArgs {
  const float* q;          // [B][n_heads][head_dim]
  const bf16_t* k_cache;   // layer base of the paged pool [blocks][n_kv][KV_BLOCK][hd]
  const bf16_t* v_cache;
  const int* block_table = nullptr;  // [slots][max_ctx / KV_BLOCK] or null (identity)
  int bt_rows = 0;         // block_table indexed by row b instead of slot[b]
  const int* seq_len;      // [B] number of valid keys (pos+1); >= 1 -- an empty row (0) is never passed: its
                           // output is 0/0 (other rows and the counters are unaffected)
  const int* slot;         // [B] or null
  int B, n_heads, n_kv_heads, head_dim, max_ctx;
  int n_chunks;            // grid chunks (>= ceil(max_len / ATTN_CHUNK))
  int split;               // keys per workgroup (multiple of ATTN_CHUNK); 0 -> chosen by the launcher
  float scale;
  float* o_part;           // [B][n_heads][n_chunks][hd]
  float* ml;               // [B][n_heads][n_chunks][2]
  float* out;              // [B][n_heads*hd]
  bf16_t* out16 = nullptr; // if set: the output as bf16 instead (the batched-decode GEMM's A operand)
  int short_len = -1;      // contexts up to this many keys split by query head (-1: launcher decides)
  int* counters;           // [B][n_kv_heads] arrival tickets, zero-initialised, self re-arming
  unsigned long long* ts = nullptr;  // probes: [grid][8] s_memrealtime phase stamps (tools/attn_probe.py --stamps)
  int kv_nt = -1;          // long mode: K/V loads with the streaming (nt) policy (-1: AIOS_ATTN_NT, default 1)
  int kv_tail = -1;        // last partial block: loads only for live keys (-1: AIOS_ATTN_TAIL, default 1)
                           // (0 requires finite dead keys: their V is loaded and multiplied by p = 0)
  int combine_trips = 0;   // split-K combine: 0 = launcher (AIOS_ATTN_COMBINE, default one round trip), 2 = two
  int out_wt = 0;          // fp32 out with write-through (agent-scope) stores
  int kv_fp8 = 0;          // fp8 e4m3 pool: value = code * kv_scale_{k,v}
  float kv_scale_k = 1.f, kv_scale_v = 1.f;
};
constexpr int ATTN_CHUNK = 64;
void launch_attn_decode(const AttnDecodeArgs& a, hipStream_t st);
struct GemvArgs;
int attn_decode_split(int max_ctx, int B, int n_kv_heads);

// causal flash attention for a prefill chunk of T tokens at positions [start, start+T) of one
// slot, over the cached keys [0, start+T) (MFMA; kernels/attention_prefill.hip)
struct AttnPrefillArgs {
  const float* q;          // [T][n_heads][head_dim] (RoPE applied)
  const bf16_t* k_cache;   // layer base of the paged pool [blocks][n_kv][KV_BLOCK][hd]
  const bf16_t* v_cache;
  const int* block_table = nullptr;  // [slots][max_ctx / KV_BLOCK] or null (identity)
  int slot, start, T;
  int n_heads, n_kv_heads, head_dim, max_ctx;
  float scale;
  bf16_t* out;             // [T][ldo] bf16
  int ldo;
  int kv_fp8 = 0;          // fp8 e4m3 pool: value = code * kv_scale_{k,v}
  float kv_scale_k = 1.f, kv_scale_v = 1.f;
};
void launch_attn_prefill(const AttnPrefillArgs& a, hipStream_t st);
bool attn_prefill_supports(int n_heads, int n_kv_heads, int head_dim);  // keys per workgroup the launcher picks

// ---- sampling ---------------------------------------------------------------------------------
// per row b: token[b] = argmax(logits[b])   (temperature[b] > 0 -> Gumbel-max sample from
// softmax(logits / T) restricted to the top-k (top_k[b] > 0, <= 256) and the nucleus top_p[b]
// (< 1; over the top-256 when top-k is off)); then pos[b] += 1, seq_len[b] = pos[b] + 1,
// history[b][step] = token.
// Logit processors (min_p or pen_tokens non-null selects the kernel instantiation that has them), in
// this order per row: penalties over the window pen_tokens[b] -- for every distinct token t with
// c >= 1 occurrences, l[t] = l[t] > 0 ? l[t] / repeat_penalty : l[t] * repeat_penalty, then
// l[t] -= c * frequency_penalty + presence_penalty (llama.cpp's rule) -- then the mask, then greedy
// argmax, or top-k / top-p as above followed by min-p: a survivor i stays only if
// exp((l_i - M) / T) >= min_p[b], M the largest allowed penalised logit (a ratio test on the tempered
// distribution: it intersects with the nucleus, nothing is renormalised before it; <= 0: off; greedy
// ignores it).  min-p with top-k and top-p both off works on the top-256 logits, like top-p alone.
// Top-K, K = min(top_k, 256) or 256: a token stays if l >= the K-th largest allowed logit, compared on a
// grid of (30 T + 1) * 2^-24 (values within a cell of the K-th count as tied with it and stay).  Ties: a
// token strictly above the K-th value is never displaced by tokens tied at it -- a 4096-token slice
// publishes at most 256 candidates and the merge carries at most 3840 from round to round, and what either
// drops beyond that comes from the group tied at the threshold only (the last of it in thread order).
// Capacity: every V up to SAMPLE_MAX_V with every K up to 256 -- the merge folds the slices' candidates (up
// to 256 * V / 4096) through its 4096-entry table in rounds (one round up to 4096 candidates, i.e. every
// V <= 65536), in a fixed order: the same logits, settings and RNG key give the same token on every run.
// tests/sampler_oracle.py is this rule in float64.
// Logit bias (bias_ids non-null selects the processor instantiation too): per row a sparse list of at most
// SAMPLE_BIAS_MAX entries (id, bias) -- ids distinct and in [0, V), -1 = empty entry, bias a finite fp32 or
// -inf (a ban; +inf and NaN are refused by every layer that builds a list).  Order per row: bias, then the
// penalties, then the mask, then everything above.  l[id] = l[id] + bias is ONE fp32 add (single rounding,
// no contraction), so the penalty rule sees the biased logit, a masked token stays -inf whatever its bias,
// and greedy argmax, the Gumbel path, the top-k threshold and its span, the nucleus and min-p's M all see
// biased, penalised logits: the result is exactly what the sampler returns for logits to which the host
// added the bias in fp32 beforehand.  runtime/sampler.py apply_logit_bias is the same rule on the host.
// Logprobs and prompt scoring keep reporting the RAW distribution, before the bias.
constexpr int SAMPLE_PEN_MAX = 256;  // longest penalty window (one entry per sampler thread)
constexpr int SAMPLE_BIAS_MAX = 512; // longest logit-bias list (two entries per sampler thread)
constexpr int SAMPLE_MAX_V = 262144; // largest vocabulary launch_sample takes (64 slices of 4096)
struct SampleArgs {
  const float* logits;
  int ldl;
  int B, V;
  const float* temperature;  // [B] or null (greedy)
  const int* top_k;          // [B] or null
  uint64_t seed;             // RNG key = (seed, row, pos[row])
  const uint64_t* seed_dev;  // if non-null, the seed is read from device memory (graph-replay safe)
  const uint64_t* seeds;     // [B] per-row seeds or null: RNG key = (seeds[b], pos[b]) -- a request's
                             // samples then depend on its seed and positions only, not its batch row
  int* tokens;               // [B] out
  int* pos;                  // [B] in/out (incremented when advance != 0)
  int* seq_len;              // [B] out (pos+1) or null
  int* history;              // [B][hist_stride] or null
  int hist_stride;
  int advance;
  const uint8_t* mask;       // [B][ceil(V/8)] allowed-token bitmask or null
  const float* top_p;        // [B] nucleus mass (>= 1: off) or null
  void* ws;                  // sample_ws_bytes(B, V) scratch (slice partials + candidates)
  size_t ws_bytes;
  int* counters;             // [B] arrival tickets, zero-initialised, self re-arming
  long long* ts;             // probe stamps [B][slices][16] (tools/sample_probe.py --stamps) or null
  const float* min_p;              // [B] or null (off)
  const float* repeat_penalty;     // [B] or null (1)
  const float* presence_penalty;   // [B] or null (0)
  const float* frequency_penalty;  // [B] or null (0)
  const int* pen_tokens;           // [B][pen_stride] penalty windows, -1 = empty entry; or null
  int pen_stride;                  // <= SAMPLE_PEN_MAX
  const int* bias_ids;             // [B][bias_stride] logit-bias ids, -1 = empty entry; or null (off)
  const float* bias_vals;          // [B][bias_stride] their biases (finite or -inf)
  int bias_stride;                 // <= SAMPLE_BIAS_MAX
};
void launch_sample(const SampleArgs& a, hipStream_t st);
size_t sample_ws_bytes(int B, int V);

// Per-token log-probabilities of the model's RAW distribution (before penalties, the grammar mask and
// temperature), for the tokens a sampler launch just wrote.  Per row b with top_n[b] >= 0:
//   lse = log sum_i exp(l[b][i]) over i in [0, V);  out_lp[b][0] = l[b][t] - lse, out_id[b][0] = t, t = tokens[b]
//   clamped to [0, V);
//   out_id[b][1..n], out_lp[b][1..n], n = min(top_n[b], V): the n largest logits, value descending, ties by
//   the lower token id, each as l - lse; the entries behind them get id -1 and logprob -inf.
// Selection compares the fp32 values as they are (no arithmetic), so the ids are exact; a -inf logit has
// logprob -inf and may close the list.  A row that is all -inf or holds a NaN is unspecified.
// top_n[b] < 0: row off -- its outputs are not written.  tokens[] lives on the device, written by the sampler
// launch in front (which only writes ids in [0, V)); no launcher sees it on the host, so nothing throws for
// an id outside [0, V): only the kernel's clamp keeps the read in bounds, and out_id[b][0] shows the id used.
// The host rule (runtime/sampler.py: logprobs), which has the token, raises.  kernels/logprobs.hip; tests/logprob_oracle.py is this rule in float64.
constexpr int LOGPROB_MAX_TOP = 20;  // alternatives per token (OpenAI's top_logprobs cap)
constexpr int LOGPROB_ROW = LOGPROB_MAX_TOP + 1;  // entries per output row: the token, then the alternatives
struct LogprobArgs {
  const float* logits;
  int ldl;
  int B, V;              // V <= SAMPLE_MAX_V
  const int* tokens;     // [B] the sampled tokens
  const int* top_n;      // [B] alternatives wanted, 0..LOGPROB_MAX_TOP; < 0: row off
  float* out_lp;         // [B][LOGPROB_ROW]
  int* out_id;           // [B][LOGPROB_ROW]
  void* ws;              // logprob_ws_bytes(B, V) scratch (slice maxima, sums and candidates)
  size_t ws_bytes;
  int* counters;         // [B] arrival tickets, zero-initialised, self re-arming
};
void launch_logprobs(const LogprobArgs& a, hipStream_t st);
size_t logprob_ws_bytes(int B, int V);

// Prompt scoring: the same RAW distribution for MANY rows, one target id each (a prompt's next tokens).
// Per row r, l = logits[r][0..V), t = targets[r], lse = log sum_i exp(l_i):
//   out_f[r] = {lp, best_lp}, out_i[r] = {rank, best};  lp = l[t] - lse;
//   rank = #{ i : l_i > l_t, or l_i == l_t and i < t } (0: the target is the argmax);
//   best = the lowest id among the maxima, best_lp = l[best] - lse.
// t < 0 (or, on the device, t >= V): no target -- lp NaN, rank -1, best / best_lp still reported.  A -inf logit
// has logprob -inf; a row that is all -inf or holds a NaN is unspecified.  Any V >= 1 (the kernel loops: no
// SAMPLE_MAX_V limit), any ldl >= V (nothing in [V, ldl) is read), any R.  No workspace, no atomics: the same
// input gives the same bits.  kernels/score_rows.hip; tests/score_oracle.py is this rule in float64.
struct ScoreArgs {
  const float* logits;  // [R][ldl]
  int ldl;
  int R, V;
  const int* targets;   // [R]
  float* out_f;         // [R][2]
  int* out_i;           // [R][2]
  int max_grid = 0;     // workgroups at most (0: the launcher's cap); more rows take a grid stride
};
void launch_score_rows(const ScoreArgs& a, hipStream_t st);

// ---- speculative decoding: accept a draft ---------------------------------------------------------
// One request ran R consecutive positions pos0 .. pos0 + R - 1 as the R rows of one decode step: in[0] is its
// last accepted token, in[1..R) a draft of the tokens that follow, and the R-row sampler launch in front (on
// the same stream, advance = 1) wrote out[i], the token after in[0..i].  Row i saw the right context only if
// the drafts before it were right, so
//   n = the largest k <= R - 1 with out[i] == in[i + 1] for every i < k  (a match behind the first mismatch
//   does not count), and the request emits out[0..n]: what n + 1 one-row steps would have sampled, because
//   the sampler's RNG is keyed (seeds[b], pos[b]) and not by step.
// Writes: record[SPEC_RECORD] = {n, out[0..n], -1 ...} for one copy to the host, and row 0 of the step state
// as if the sequence had advanced by n + 1 one-row steps: tokens[0] = out[n], pos[0] = pos0 + n + 1,
// seq_len[0] = pos0 + n + 2, history[pos0 + 1 + i] = out[i] for i <= n (row 0's history; entries at or past
// hist_stride are not written).  Rows 1..R-1 of the state are left as the sampler wrote them: the next step's
// upload overwrites them.  out may be tokens (every out[i] is read before tokens[0] is written).  One
// workgroup of one wave, no workspace, no atomics.  kernels/spec_accept.hip; tests/spec_oracle.py is the rule.
constexpr int SPEC_MAX_ROWS = 8;                  // rows of a speculative step: the last token + 7 drafts
constexpr int SPEC_RECORD = SPEC_MAX_ROWS + 1;    // ints of the packed record
struct SpecAcceptArgs {
  const int* in;    // [R] the step's input tokens (a copy of its own: the sampler overwrites tokens[])
  const int* out;   // [R] what the sampler wrote
  int pos0, R;      // R in 2..SPEC_MAX_ROWS
  int* record;      // [SPEC_RECORD]
  int* tokens;      // step state, row 0 written
  int* pos;
  int* seq_len;
  int* history;     // row 0's history or null
  int hist_stride;
};
void launch_spec_accept(const SpecAcceptArgs& a, hipStream_t st);

// ---- speculative decoding: accept the drafts of several sequences ---------------------------------
// One decode step carried S sequences, segment after segment: rows seg[s] .. seg[s + 1] - 1 (seg[0] = 0,
// seg[S] = Rt) are sequence s's 1 + d_s consecutive positions pos0[s] .. pos0[s] + d_s, in[seg[s]] its last
// accepted token and the d_s >= 0 rows behind it its draft.  The Rt-row sampler launch in front (same stream,
// advance = 1) wrote out[r].  Each segment is judged by the rule above on its own:
//   n_s = the largest k <= d_s with out[seg[s] + i] == in[seg[s] + i + 1] for every i < k; a segment's last row
//   has no draft behind it, so a match across a segment boundary never counts and d_s = 0 gives n_s = 0.
// Writes: record[s][SPEC_RECORD] = {n_s, out[seg[s] .. seg[s] + n_s], -1 ...} (S records, one copy to the
// host) and rows 0..S-1 of the step state, compacted in place, as if sequence s had advanced by n_s + 1 one-row
// steps in row s: tokens[s] = out[seg[s] + n_s], pos[s] = pos0[s] + n_s + 1, seq_len[s] = pos0[s] + n_s + 2,
// history[s * hist_stride + pos0[s] + 1 + i] = out[seg[s] + i] for i <= n_s (row s's history; an entry whose
// index pos0[s] + 1 + i is at or past hist_stride is not written).  Nothing else in the history is written
// here; what the sampler in front wrote stays: its one entry per row r, history[r * hist_stride + (position of
// row r) + 1] = out[r].  For r = 0 that entry is one of the above.  In a row 1 <= r < S flat row r belongs to
// another sequence (or to a later position of sequence 0), so its entry is a stray one in row r's history: it is
// overwritten where it falls into the range above, and stays otherwise -- beyond the range, or BELOW pos0[r] + 1,
// where it replaces an older entry of row r.  Row r >= 1 is therefore guaranteed from pos0[r] + 1 on only, not
// over its whole history as row 0 is; rows S..Rt-1 keep theirs as after the single-sequence kernel.
// Rows S..Rt-1 of tokens / pos / seq_len are left as the sampler wrote them: the next step's upload overwrites
// them.  out may be tokens: the one wave holds every out[r], in[r] and segment value in registers before its
// first store.  seg and pos0 travel in the argument block, so the launcher checks them: S in
// 1..SPEC_MULTI_MAX_SEQS, every segment 1..SPEC_MAX_ROWS rows, Rt <= SPEC_MULTI_MAX_ROWS.  One workgroup of
// one wave, no workspace, no atomics, no LDS.  kernels/spec_accept.hip; tests/spec_multi_oracle.py is the rule.
constexpr int SPEC_MULTI_MAX_SEQS = 8;   // sequences of one step
constexpr int SPEC_MULTI_MAX_ROWS = 32;  // rows of one step, all segments together
struct SpecAcceptMultiArgs {
  const int* in;    // [Rt] the step's input tokens (a copy of its own: the sampler overwrites tokens[])
  const int* out;   // [Rt] what the sampler wrote
  int S;            // sequences, 1..SPEC_MULTI_MAX_SEQS
  int seg[SPEC_MULTI_MAX_SEQS + 1];  // seg[0] = 0 < seg[1] < ... < seg[S] = Rt
  int pos0[SPEC_MULTI_MAX_SEQS];
  int* record;      // [S][SPEC_RECORD]
  int* tokens;      // step state, rows 0..S-1 written
  int* pos;
  int* seq_len;
  int* history;     // [S][hist_stride] at least, or null
  int hist_stride;
};
void launch_spec_accept_multi(const SpecAcceptMultiArgs& a, hipStream_t st);

// ---- text embeddings ---------------------------------------------------------------------------
// Pooled embedding of hidden rows x[t] (the residual stream before output_norm), llama.cpp's --embedding
// rule for a causal model:  h[t] = x[t] * g * rsqrt(mean(x[t]^2) + eps)  (the model's final RMSNorm);
//   EMBED_MEAN: p = (1 / T) sum_t h[t];  EMBED_LAST: p = h[T - 1];  result p / ||p||_2, a p that is exactly
//   zero giving the zero vector;  EMBED_NONE: the rows h[t] themselves, not L2-normalised.
// One launch folds a chunk of n rows into the running state of one sequence: acc[d] = sum of x[t] / rms[t]
// (g is applied once, at the end) and count = rows folded.  `first` zeroes both before folding; `final`
// also writes the unit vector to out[d].  EMBED_LAST folds only the chunk's last row (as first);
// EMBED_NONE touches no state and writes h for the chunk's rows to out[n][d].  Fixed summation order, no
// float atomics: bit-identical from run to run; a sum split over several launches differs from the single
// launch by fp32 rounding only.  kernels/embed_pool.hip; tests/embed_oracle.py is this rule in float64.
// The codes are GGUF's {arch}.pooling_type.
enum EmbedPooling { EMBED_NONE = 0, EMBED_MEAN = 1, EMBED_LAST = 3 };
constexpr int EMBED_MAX_D = 8192;     // widest row (a multiple of 64 from 64 up)
constexpr int EMBED_MAX_ROWS = 2048;  // most rows per launch (the prefill chunk)
constexpr int EMBED_MAX_WG = 64;      // workgroups per launch = slabs of the workspace
struct EmbedPoolArgs {
  const float* x;  // [n][ldx]
  int ldx;
  int n, d;
  const float* g;  // [d] output_norm weight
  float eps;
  float* acc;      // [d] in/out
  int* count;      // [1] in/out
  int mode;        // EmbedPooling
  int first, final;
  float* out;      // mean / last: [d], written when final; none: [n][d]
  float* ws;       // embed_pool_ws_bytes(d): one [d] slab per workgroup
  size_t ws_bytes;
  int* counter;    // [1] arrival ticket, zero-initialised, self re-arming
  int band = 0;    // rows per workgroup (set by the launcher)
};
void launch_embed_pool(const EmbedPoolArgs& a, hipStream_t st);
size_t embed_pool_ws_bytes(int d);

// ---- context shift -----------------------------------------------------------------------------
// A slot holds positions [0, n_tokens).  Positions [0, n_keep) stay, [n_keep, n_keep + n_discard) are
// forgotten, every position p at or above n_keep + n_discard becomes p - n_discard (llama.cpp's context
// shift; the new length is n_tokens - n_discard).  A moved V row is the same bytes.  A moved K row is the
// stored (RoPE'd) row rotated by -n_discard positions: pair i with stored (x, y) and (c, s) = rope_cs
// [n_discard][i] becomes (x c + y s, -x s + y c) in fp32, rounded to the cache type (bf16 nearest-even; fp8:
// decoded with the layer's K scale and re-encoded with it by the KV writers' conversion).  Pairs are
// (2i, 2i + 1), or (i, i + head_dim / 2) when rope_neox.  In place, through row `slot` of the block table:
// every block of the destination range must be mapped and private, every block of the source range mapped
// (Engine::shift_context).  n_keep + n_discard == n_tokens moves nothing.  One launch for every layer;
// kernels/kv_shift.hip, tests/context_shift_oracle.py is this rule in float64.
struct KvShiftArgs {
  bf16_t* k_cache;         // layer 0's pools (element indices as bf16, bytes when kv_fp8)
  bf16_t* v_cache;
  size_t layer_elems;      // elements from one layer's pool to the next
  const int* block_table;  // [slots][max_blocks], unmapped entries: the null block
  int max_blocks;
  int slot;
  int n_layers, n_kv_heads, head_dim;
  int n_tokens, n_keep, n_discard;
  const float2* rope_cs;   // [rope_rows][head_dim / 2] (cos, sin)
  int rope_rows;
  int rope_neox;
  int kv_fp8;
  const float* k_scale;    // [n_layers] on the device (fp8 only): value = code * scale
};
void launch_kv_shift(const KvShiftArgs& a, hipStream_t st);

// ---- KV snapshot -------------------------------------------------------------------------------
// pack: positions [0, n_tokens) of a slot, read through row `slot` of the block table, written to one contiguous
// buffer [layer][K, V][kv_head][token][head_dim] in the cache's own element type -- the layout Engine::kv_read
// returns, which is the definition of the payload (tests/kv_snapshot_oracle.py is this rule in numpy).  unpack:
// the reverse, into the slot's mapped blocks (Engine::kv_restore maps and un-shares them first).  Bytes move
// verbatim, 16 at a time.  A (block, kv head) tile of a pool is contiguous and so is its place in the buffer, so
// workgroup (block j, kv head, K or V, layer) copies min(KV_BLOCK, n_tokens - j * KV_BLOCK) rows from one to the
// other: rows at or above n_tokens and blocks outside the row's [0, ceil(n_tokens / KV_BLOCK)) are neither read
// nor written.  A table entry outside the pool is skipped: pack reads blocks [0, n_blocks] (n_blocks: the null
// block an unmapped entry names), unpack writes blocks [0, n_blocks) only.  One launch covers layers
// [layer0, layer0 + n_layers); the buffer starts at layer0.  kernels/kv_snapshot.hip.
struct KvSnapArgs {
  void* k_cache;           // layer 0's pools
  void* v_cache;
  size_t layer_bytes;      // bytes from one layer's pool to the next
  void* buf;               // [n_layers][2][n_kv_heads][n_tokens][head_dim], 16-byte aligned
  const int* block_table;  // [slots][max_blocks]
  int max_blocks;
  int n_blocks;            // allocatable blocks of a layer pool (block n_blocks: the null block)
  int slot;
  int layer0, n_layers, n_kv_heads, head_dim;
  int n_tokens;
  int elem_bytes;          // 2 (bf16) or 1 (fp8)
  int unpack;              // 0: pool -> buf, 1: buf -> pool
};
void launch_kv_snapshot(const KvSnapArgs& a, hipStream_t st);

// ---- DFA grammar masks -------------------------------------------------------------------------
// A grammar is a byte-level DFA (runtime/json_schema.py compiles a JSON schema into one): byte_class[256],
// trans[n_states][n_classes] (u16), accept[n_states]; state 0 is dead (its row is zero), every entry of trans is
// below n_states and every entry of byte_class below n_classes -- the loader checks that, the kernel does not.
// Row b of the launch has grammar gid[b] in state state[b]; token t is allowed when it is not empty and its bytes
// tok_bytes[tok_off[t] .. tok_off[t + 1]) lead from that state to a state other than 0; the ids in eos are
// allowed exactly when accept[state[b]].  mask row b (ceil(V / 8) bytes, bit t % 8 of byte t / 8: SampleArgs::mask)
// is written whole, bits past V zero.  gid[b] < 0: the row has no device grammar -- with fill_free it is set to
// all ones (bits past V zero), without it is not touched (the host's mask bytes stay).  gid[b] >= n_grammars or a
// state outside the table: nothing is allowed.  kernels/grammar_mask.hip; runtime/json_schema.py SchemaGrammar.mask
// is this rule in numpy.
constexpr int GRAMMAR_MAX = 64;      // grammars an engine holds at once
constexpr int GRAMMAR_MAX_EOS = 8;   // end-of-sequence ids of a vocabulary
struct GrammarTable {
  const uint8_t* byte_class;  // [256]
  const uint16_t* trans;      // [n_states][n_classes]
  const uint8_t* accept;      // [n_states]
  int n_states, n_classes;
};
struct GrammarMaskArgs {
  const int* tok_off;         // [V + 1] offsets into tok_bytes
  const uint8_t* tok_bytes;
  int V;
  const GrammarTable* grammars;  // [n_grammars] on the device
  int n_grammars;
  const int* gid;             // [B]
  const int* state;           // [B]
  uint8_t* mask;              // [B][ceil(V / 8)]
  int B;
  int fill_free;
  int eos[GRAMMAR_MAX_EOS];
  int n_eos;
};
void launch_grammar_mask(const GrammarMaskArgs& a, hipStream_t st);

// ---- MFMA GEMM (prefill) ----------------------------------------------------------------------
// C[M][N] (fp32, epilogue) = A[M][K] (bf16) x W[N][K]^T (quantized, dequantized tile-wise in LDS)
struct GemmArgs {
  const bf16_t* A;
  int lda;
  QWeight w;
  int M, N, K;
  float* C;
  int ldc;
  int accumulate;  // C += result
  float* ws = nullptr;  // split-K workspace of the skinny (M <= 64) kernel, see GemmQArgs
  size_t ws_bytes = 0;
  int* cnt = nullptr;
  int cnt_len = 0;
};
void launch_gemm(const GemmArgs& a, hipStream_t st);
bool gemm_supports(int qt);

// multi-segment GEMM with fused epilogues (the prefill path): C = A x [W0; W1; W2]^T
enum GemmEpi { GEPI_STORE = 0, GEPI_ACCUM = 1, GEPI_SWIGLU_BF16 = 2, GEPI_QKV = 3, GEPI_ACCUM_NORM = 4 };
struct GemmQArgs {
  const bf16_t* A;   // [M][lda] bf16
  int lda;
  QWeight seg[3];    // weight segments stacked along N (rows of each a multiple of 64)
  int seg_n0[3];     // first output column of each segment
  int nseg;
  int M, N, K;
  float* C;          // [M][ldc] fp32 (STORE / ACCUM)
  bf16_t* C16;       // [M][ldc] bf16 (SWIGLU_BF16: column n/2 = silu(col n) * col n+1)
  int ldc;
  int epi;
  int ksplit;        // K split over workgroups: 0 = auto, 1 = off, < 0 = auto among the plans whose sums are
                     // reproducible (no fp32-atomic split-K / stream-K partials: the prefill GEMM's tuned
                     // S = 1 plan; the ring and skinny GEMMs' slab splits already are)
  // skinny (M <= 64) split-K: fp32 partial slabs [S][tiles][16*Mt][rows] + per-tile arrival
  // tickets (zero-initialised, re-armed by each tile's last arriver).  Null -> no split.
  float* ws;
  size_t ws_bytes;
  int* cnt;
  int cnt_len;
  // GEPI_QKV (skinny kernel, batched decode; non-NeoX RoPE, no QK-norm / bias): global column
  // col0 + n of the packed [q | k | v] product -> RoPE'd q to q_out[M][q_dim], RoPE'd k / v as bf16
  // into the paged KV cache at (slot[m], pos[m]) -- the qkv_post launch folded into the epilogue
  int col0;
  int head_dim, q_dim, kv_dim, n_kv_heads, max_ctx;
  const float2* rope_cs;  // [max_ctx][head_dim / 2] (cos, sin)
  const int* pos;
  const int* slot;
  const int* block_table;
  float* q_out;
  bf16_t* k_cache;
  bf16_t* v_cache;
  int kv_fp8;        // fp8 e4m3 pool: code = value * kv_inv_{k,v}
  float kv_inv_k, kv_inv_v;
  // RMSNorm split across two skinny GEMMs (batched decode: no normalisation launch).
  //  producer (GEPI_ACCUM_NORM = residual add): also writes bf16(x_new * nrm_g) to nrm_out16
  //    [M][ldc] and, per output tile t, sum_n x_new[m][n]^2 to nrm_part[m * nrm_parts + t]
  //    (nrm_parts = gemm_skinny_ntile(producer args); fixed-order reductions, no atomics)
  //  consumer (any epilogue, nrm_in set): A is that bf16(x * g); output row m is scaled by
  //    rsqrt(sum_t nrm_in[m * nrm_parts + t] / K + nrm_eps) before the epilogue
  const float* nrm_g;
  bf16_t* nrm_out16;
  float* nrm_part;
  const float* nrm_in;
  int nrm_parts;
  float nrm_eps;
  unsigned long long* dbg_ts;  // probes (skinny kernel): [grid][8] s_memrealtime phase stamps or null
};
// bytes of split-K workspace / ticket count the skinny GEMM may use for an M x N output
size_t gemm_skinny_ws_bytes(int M, int N);
int gemm_skinny_cnt_len(int N);
// output tiles of the skinny kernel for these args (0: not served by the skinny kernel)
int gemm_skinny_ntile(const GemmQArgs& a);
void launch_gemm_q(const GemmQArgs& a, hipStream_t st);
// Which kernel launch_gemm_q hands each of its format-split launches to, without launching: one
// entry per launch, col0 = the launch's first global column.  Asks the launchers' own predicates in
// launch_gemm_q's order and throws where it would (bindings / tests: a test asserts the kernel it
// means to exercise).
enum GemmKernel { GK_RING = 0, GK_PF = 1, GK_SKINNY = 2, GK_BIG = 3 };
struct GemmRoute {
  int col0;
  int kernel;
};
std::vector<GemmRoute> gemm_route(const GemmQArgs& a);
bool gemm_ring_serves(const GemmQArgs& a);    // launch_gemm_ring would take a (gemm_ring.hip)
bool gemm_skinny_serves(const GemmQArgs& a);  // launch_gemm_skinny would take a (gemm_skinny.hip)
// the prefill GEMM (kernels/gemm_pf.hip): true if it took the launch; its tile / split plan for a shape
bool launch_gemm_pf(const GemmQArgs& a, hipStream_t st);
bool gemm_pf_serves(const GemmQArgs& a);  // launch_gemm_pf would take a (gemm_pf.hip)
void gemm_pf_plan(const GemmQArgs& a, int& bm, int& bn, int& s);
// time every prefill-GEMM plan for these args (buffers overwritten) and keep the fastest for their M
// bucket; returns the number of plans timed
int gemm_pf_autotune(const GemmQArgs& a, hipStream_t st);
std::vector<int> gemm_pf_export();              // the process's tuned prefill plans (flat ints)
void gemm_pf_import(const std::vector<int>& v);  // ... installed (TP: the leader's; persisted sets)

}  // namespace aios
