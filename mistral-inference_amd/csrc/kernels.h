// Internal (non-ABI) declarations shared by the kernel translation units and the runner.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mistral_hip.h"

typedef uint16_t bf16_t;

// ---------------------------------------------------------------------------------------------- GEMV
enum GemvMode {
  GEMV_STORE = 0,
  GEMV_RESIDUAL = 1,
  GEMV_SWIGLU = 2,
  GEMV_LOGITS = 3,
  GEMV_QKV_ROPE = 4,  // fused q|k|v projection + RoPE (+ ring write at decode)
  GEMV_MOE_W13 = 5,   // per (token, slot) expert gate/up projection + SwiGLU
  GEMV_MOE_W2 = 6     // per token: expert down projections, weighted bf16 combine, residual
};

constexpr int GEMV_MAX_T = 8;
// LDS a GEMV block may use for its T activation rows.  Round 5: up to 144 KiB (opt-in above 64 KiB per function) instead of 64:
// with hidden_dim 14336 a row is 28 KiB, and a batch of three sequences (mistral-demo) ran the W2 GEMV as TWO passes - the
// weights streamed twice per decode step (+24 us per layer).  Above 80 KiB one block fits a CU: the grid is one block per CU.
constexpr size_t GEMV_LDS_BUDGET = 144 * 1024;

struct GemvArgs {
  int mode;
  int T;                // tokens in this launch
  int K;                // contraction length (multiple of 8)
  int N;                // output rows (SWIGLU: hidden_dim)
  const bf16_t* x;      // [T, ldx]
  int ldx;
  const bf16_t* norm_w; // fused RMSNorm weight [K] or nullptr
  float eps;
  const bf16_t* w0;     // rows [0, n0)
  const bf16_t* w1;     // rows [n0, n1)   (SWIGLU: W3)
  const bf16_t* w2;     // rows [n1, N)
  int n0, n1;
  void* out;            // bf16 [T, ldo] (fp32 for LOGITS)
  int ldo;
  const bf16_t* residual;
  // QKV_ROPE
  const float* rope_cs; // fp32 [rope_len, head_dim/2, 2]
  const int32_t* tok_pos;
  const int32_t* tok_seq;  // nullptr: sequence id == seq0 + token index
  int head_dim;
  int write_kv;
  void* cache_k;
  void* cache_v;
  int W;
  int kv_layout;  // MI_KV_SLOT_MAJOR / MI_KV_HEAD_MAJOR (common.cuh)
  // MoE
  const void* const* expert_tab;  // device [E][3]
  const int32_t* sel_idx;         // device [T*top_k]
  const float* sel_w;             // device [T*top_k]
  int top_k;
  int seq0;  // QKV_ROPE without tok_seq: the sequence of this launch's token 0 (the first row of a later pass, gemv_pass_loop)
};

int gemv_max_tokens(int K);
hipError_t launch_gemv(const GemvArgs& a, hipStream_t s);
// gemv.hip compiled with -DGEMV_F16=1 (element ElemF16, common.cuh): the same kernels on fp16 payloads (mi_forward_generic: decode steps of fp16 models)
int gemv_max_tokens_f16(int K);
hipError_t launch_gemv_f16(const GemvArgs& a, hipStream_t s);

// The same launches on quantised weight rows with their scales (weight-only formats).  GemvArgs is the bf16 kernels' kernarg and
// stays as it is: the scales ride beside it.  w0 / w1 / w2 point to bytes, modes STORE / RESIDUAL / SWIGLU / QKV_ROPE / LOGITS; scale[i]
// belongs to segment i (SWIGLU: scale[0] = W1's, scale[1] = W3's).
template <class scale_t>
struct GemvScaledArgs {
  GemvArgs g;
  const scale_t* scale[3];
};
// The dequantised image of the N rows of up to three matrices side by side (segment ends n0, n1 as in GemvArgs), dense [N, K]
// bf16: what the MFMA GEMMs read at more than 8 rows
template <class scale_t>
struct DequantArgs {
  const uint8_t* w[3];
  const scale_t* scale[3];
  int n0, n1, N, K;
  bf16_t* out;
};
// gemv_w8.hip: OCP e4m3 bytes [rows, K], K % 16 == 0; scale[i] holds one fp32 per row.  out[r, k] = bf16(scale[r] * e4m3(W[r, k]))
typedef GemvScaledArgs<float> GemvW8Args;
typedef DequantArgs<float> DequantW8Args;
hipError_t launch_gemv_w8(const GemvW8Args& a, hipStream_t s);
hipError_t launch_dequant_w8(const DequantW8Args& a, hipStream_t s);
// gemv_w4.hip: OCP MXFP4, e2m1 code bytes [rows, K / 2] (two codes per byte, the low nibble at the even k), K % 32 == 0; scale[i]
// holds the e8m0 block scales [rows, K / 32] (byte b: 2^(b - 127)).  out[r, k] = 2^(scale[r, k / 32] - 127) * e2m1(code[r, k]),
// exact in bf16
typedef GemvScaledArgs<uint8_t> GemvW4Args;
typedef DequantArgs<uint8_t> DequantW4Args;
hipError_t launch_gemv_w4(const GemvW4Args& a, hipStream_t s);
hipError_t launch_dequant_w4(const DequantW4Args& a, hipStream_t s);
int gemv_w4_row_pairs(int npairs, int cus);  // row pairs per unit the launcher picks at one token

// ---------------------------------------------------------------------------------------------- GEMM
enum GemmEpi { GEMM_STORE = 0, GEMM_RESIDUAL = 1, GEMM_SWIGLU = 2, GEMM_LOGITS = 3, GEMM_LOGPROB = 4 };

struct GemmArgs {
  int epi;
  int M, N, K;          // N: output columns (SWIGLU: hidden_dim)
  const bf16_t* a;      // [M, lda]
  int lda;
  const bf16_t* w0;     // row segments as in GemvArgs (SWIGLU: w0 = W1, w1 = W3)
  const bf16_t* w1;
  const bf16_t* w2;
  int n0, n1;
  void* out;
  int ldo;
  const bf16_t* residual;
  // Token-grouped form (MoE prefill, moe.py:28-32): ONE launch covers every expert.  Compact rows are the (token,
  // slot) pairs sorted by expert; tile i of `tile_tab` is {expert, first compact row, valid rows (<= tile_rows), 0}.
  const int32_t* tile_tab;        // device [max_m_tiles][4] or nullptr (plain GEMM)
  const int32_t* n_tiles_ptr;     // device: number of valid entries in tile_tab
  int max_m_tiles;                // host upper bound (grid sizing)
  int tile_rows;                  // rows per m-tile the table was built for: 128 (gemm.hip) or 256 (gemm256.hip)
  const void* const* expert_tab;  // device [E][3] (w1, w2, w3) pointers
  int w_sel0, w_sel1;             // which of the three matrices feed w0 / w1 (w_sel1 < 0: unused)
  const int32_t* a_gather;        // device: A row of compact row r is a[a_gather[r]] (nullptr: a[r])
  // GEMM_LOGPROB (gemm256 only): nothing is stored; per (row, 256-column tile) the max and sum-exp of the bf16-rounded
  // logits go to lp_partial[row][n_tile] and the logit of column lp_target[row] to lp_tgt[row]
  const int32_t* lp_target;       // device [M], -1: none
  float2* lp_partial;             // device [M][ceil(N / 256)]
  float* lp_tgt;                  // device [M]
  // GEMM_STORE only: rotary embedding in the epilogue (transformer_layers.py:70 apply_rotary_emb on the bf16 q, k).  Output
  // columns n < rope_cols are (re, im) pairs of heads of rope_dh columns; pair i of a head is turned by the table entry
  // rope_cs[tok_pos[row]][i] = (cos, sin), exactly as rope_kernel does in a separate pass.  nullptr: plain store.
  const float* rope_cs;           // device fp32 [rope_len][rope_dh / 2][2]
  const int32_t* tok_pos;         // device [M]
  int rope_cols, rope_dh;         // rope_cols % rope_dh == 0, rope_dh % 4 == 0
  int rope_col0;                  // column of the whole problem at which this (column-sliced) launch starts (% rope_dh == 0)
  // GEMM_LOGPROB of a launch that is columns [lp_col0, lp_col0 + N) of a wider head (a quantised LM head dequantised in slices of
  // vocabulary rows, api.hip): lp_target holds columns of the whole head and lp_partial is [M][lp_tiles] with this launch's tiles
  // from lp_col0 / 256 on, so that the slices leave exactly the partials of the one launch.  lp_col0 % 256 == 0; lp_tiles 0:
  // ceil(N / 256).  (Behind everything else: no other field moves, so no other kernel's instruction stream changes.)
  int lp_col0, lp_tiles;
};
// weight row r of up to three matrices side by side (the MFMA GEMMs' DMA sources)
__device__ __forceinline__ const bf16_t* seg_row(const GemmArgs& g, int r) {
  if (r < g.n0) return g.w0 + (size_t)r * g.K;
  if (r < g.n1) return g.w1 + (size_t)(r - g.n0) * g.K;
  return g.w2 + (size_t)(r - g.n1) * g.K;
}
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
// Which kernel computes which column of launch_gemm(g), plain form: columns [0, c256) on the 256-tile kernel (0: none, g.N: all),
// the rest on the 128-tile kernel - or, with `half`, on the 256 kernel's half-height tiles.  A caller that runs the problem in column
// slices (a quantised LM head, api.hip) keeps every column on the kernel the one launch gives it: same kernel, same bits.
struct GemmPlan {
  int c256;
  bool half;
};
GemmPlan gemm_plan(const GemmArgs& g);
hipError_t launch_gemm128(const GemmArgs& g, hipStream_t s);  // the 128-tile kernel, whatever the shape
bool gemm256_applicable(const GemmArgs& g);  // gemm256.hip: 256x256 tile for the large prefill shapes
hipError_t launch_gemm256(const GemmArgs& g, hipStream_t s);
bool gemm256_half_applicable(const GemmArgs& g);  // 128x256 tiles of the same kernel: the columns of a half-filled last round
hipError_t launch_gemm256_half(const GemmArgs& g, hipStream_t s);
void gemm_set_tail_mode(int mode);  // mi_debug_set_prefill_kernels
// gemm256.hip compiled with -DG256_F16=1 (element ElemF16): the same kernel on fp16 payloads (generic.hip: prefills of fp16 models; gemm256_applicable is the predicate for both elements)
hipError_t launch_gemm256_f16(const GemmArgs& g, hipStream_t s);

// The 256-tile GEMM on e4m3 activation bytes (prefills of quantised models, opt-in).  gemm256.hip, gemm256_w8a8.hip and
// gemm256_w4a8.hip share their tile map, K loop, epilogue and launcher pieces through gemm256_core.cuh; GemmArgs is the bf16
// kernel's kernarg and stays as it is, the scales ride beside it (as GemvScaledArgs above).  g.a points to e4m3 bytes, g.lda is in
// bytes; sx [M] are the activation rows' scales (launch_act_quant_e4m3), sw[i] the scales of weight segment i (SWIGLU: sw[0] =
// W1's, sw[1] = W3's).  Epilogues STORE (with RoPE) / RESIDUAL / SWIGLU; plain form only (no tile table, no gather).
template <class scale_t>
struct GemmA8Args {
  GemmArgs g;
  const float* sx;
  const scale_t* sw[3];
};
// gemm256_w8a8.hip: e4m3 bytes for BOTH operands (FP8 models): out = epilogue((A_q . W_q^T)[m, n] * sx[m] * sw[n]).
// g.w0 / g.w1 / g.w2 point to e4m3 bytes [rows, K], sw[i] holds one fp32 per weight row.
typedef GemmA8Args<float> GemmW8A8Args;
bool gemm256_w8a8_applicable(int M, int K);  // M >= 256 && K % 128 == 0 && K <= 16384 (the quantiser's limit): the route's one shape predicate
hipError_t launch_gemm256_w8a8(const GemmW8A8Args& a, hipStream_t s);

// gemm256_w4a8.hip: the same on MXFP4 weights (MXFP4 models): e2m1 codes meet e4m3 activations on the mixed form of the
// block-scaled MFMA, which applies the e8m0 block scales itself:
// out = epilogue((sum_k A_q[m, k] * e2m1(C[n, k]) * 2^(S[n, k / 32] - 127)) * sx[m]).  g.w0 / g.w1 / g.w2 point to code bytes
// [rows, K / 2]; sw[i] are the block scale bytes [rows, K / 32] of segment i, 4-byte aligned.
typedef GemmA8Args<uint8_t> GemmW4A8Args;
bool gemm256_w4a8_applicable(int M, int K);  // gemm256_w8a8_applicable: one quantiser, one K tile
hipError_t launch_gemm256_w4a8(const GemmW4A8Args& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------- attention
struct AttnDecodeArgs {
  void* out;            // [B, H*Dh]
  const bf16_t* q;      // [B, ldq]
  int ldq;
  const bf16_t* cache_k;  // [maxB, W, Hkv*Dh] (kv_layout 0) or [maxB, Hkv, W, Dh] (1)
  const bf16_t* cache_v;
  int kv_layout;           // with MI_KV_E4M3: cache_k / cache_v point to e4m3 bytes (launch_attn_decode picks the kernels' Ring argument)
  int W, B, H, Hkv, Dh;    // Hkv: kv heads AS SCHEDULED = real kv heads x kv_groups (launch_attn_decode sets both)
  int kv_groups;           // query-head groups per real kv head (1 unless the GQA ratio is split, see launch_attn_decode)
  const int32_t* tok_pos;  // [B]
  float* partial;          // scratch
  int32_t* tickets;        // reserved: first 4 KiB of the scratch (arrival counters of a removed in-kernel combine)
  int n_splits;
};
int attn_decode_splits(int W);
int attn_decode_group(int R);  // query heads served per block: the largest of {8, 6, 4, 2, 1} dividing the GQA ratio
size_t attn_decode_partial_floats(int B, int H, int Hkv, int Dh, int W);
hipError_t launch_attn_decode(const AttnDecodeArgs& a, hipStream_t s);

struct AttnPrefillArgs {
  void* out;            // [T, H*Dh]
  const bf16_t* qkv;    // [T, ld]  q | k | v (post-RoPE)
  int ld;
  const bf16_t* cache_k;
  const bf16_t* cache_v;
  int kv_layout;  // MI_KV_SLOT_MAJOR / MI_KV_HEAD_MAJOR (common.cuh)
  int W, B, max_q_len, H, Hkv, Dh;
  const int32_t* q_start;    // [B+1]
  const int32_t* kv_before;  // [B]
  int causal;
  float scale;  // softmax scale (already validated: > 0)
};
hipError_t launch_attn_prefill(const AttnPrefillArgs& a, hipStream_t s);
void attn_prefill_set_mode(int waves);  // mi_debug_set_prefill_kernels (negative: keep)
hipError_t launch_attn_prefill_f16(const AttnPrefillArgs& a, hipStream_t s);  // attn_prefill.hip compiled with -DATTN_F16=1

// Verify step (attn_verify.hip): sequence b brings rows q_start[b] .. q_start[b + 1] (at most 8, at positions kv_before[b] + i)
// that are NOT in its ring; mask of the prefill attention, split geometry of the decode attention.
struct AttnVerifyArgs {
  void* out;            // [T, H*Dh]
  const bf16_t* qkv;    // [T, ld]  q | k | v (post-RoPE)
  int ld;
  const bf16_t* cache_k;  // bf16 rings in kv_layout
  const bf16_t* cache_v;
  int kv_layout;
  int W, T, B, H, Hkv, Dh;
  const int32_t* q_start;    // [B+1]
  const int32_t* kv_before;  // [B]
  float* partial;            // attn_verify_partial_floats(T, H, Dh, W) floats
  bf16_t* stash;             // [T, 2 * Hkv * Dh] K | V of the step's rows, or nullptr
  int n_splits;              // launch_attn_verify sets it
};
int attn_verify_splits(int W);  // blocks of 128 slots; more than 32 of them: launch_attn_verify declines (hipErrorInvalidValue)
size_t attn_verify_partial_floats(int T, int H, int Dh, int W);
hipError_t launch_attn_verify(const AttnVerifyArgs& a, hipStream_t s);

// Verify step, behind the LM head (elementwise.hip).  accept: n_accept[b] = the number of leading drafts ids[q_start[b] + i]
// (i >= 1) that equal the argmax tok[q_start[b] + i - 1] of the row before them.  commit: for every layer l, rows 0 .. n_accept[b]
// of sequence b go from the stash [n_layers, T, 2 * kv_dim] (K | V) to slot (kv_before[b] + i) % W_l of its rings, then
// kv_seqlens[b] += n_accept[b] + 1.  The ring table travels in the kernel arguments, VERIFY_COMMIT_LAYERS layers per launch.
constexpr int VERIFY_COMMIT_LAYERS = 128;
struct VerifyCommitArgs {
  bf16_t* k[VERIFY_COMMIT_LAYERS];
  bf16_t* v[VERIFY_COMMIT_LAYERS];
  int32_t W[VERIFY_COMMIT_LAYERS];
  const bf16_t* stash;  // of the first layer of this launch
  int n_layers, T, B, kv_dim, Dh, kv_layout;
  const int32_t *q_start, *kv_before, *tok_seq, *n_accept;
  int64_t* kv_seqlens;  // advanced by this launch, or nullptr (every launch of a step but the last)
};
hipError_t launch_verify_accept(const int64_t* ids, const int64_t* tok, const int32_t* q_start, int B, int32_t* n_accept, hipStream_t s);
hipError_t launch_verify_commit(const VerifyCommitArgs& a, hipStream_t s);

// Compute units of the current device (256 on a full MI355X; fewer in partitioned modes).  Grid-shaping heuristics
// (rounds of blocks, tail splitting) use it; results never depend on it.
inline int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      cus = 256;
  }
  return cus;
}

// ---------------------------------------------------------------------------------------------- workspace control words
// The first 32-bit words of a workspace (mi_forward's and the generic path's alike), shared by the launch path's kernels, the
// persistent decode engine and the host (mi_decode_engine_status copies the eight words below CTRL_CENSUS0).  mistral_inference/_hip.py names them in
// the same order (CTRL_WORDS; tests/test_ctrl_words.py holds the two together).
enum : int {
  CTRL_EPOCH = 0,     // step epoch of the persistent decode engine (granule tags), bumped by the step's first kernel
  CTRL_STATUS = 1,    // sticky engine status: the code of the first timed-out wait (mi_decode_engine_reset clears it)
  CTRL_ABORT = 2,     // per-step abort broadcast
  CTRL_BAD_ID = 3,    // 1 + the index of an out-of-range token id (atomic max)
  CTRL_LAUNCHES = 4,  // engine launches completed
  CTRL_STEPS = 5,     // decode steps committed (index + 1 into the greedy history ring)
  CTRL_ARRIVE = 6,    // workgroup arrivals of the running engine launch
  CTRL_SABOTAGE = 7,  // test hook: engine launches that shall fail their residency gate (mi_debug_engine_sabotage)
  CTRL_CENSUS0 = 8,   // two spare words that the engine's residency census borrows
  CTRL_CENSUS1 = 9
};

// ---------------------------------------------------------------------------------------------- elementwise
hipError_t launch_gelu(void* x, int ldx, int T, int N, hipStream_t s);
// log-softmax gather: out[m] = x_t - logsumexp(row m), from per-tile (max, sum-exp) partials or from a full logits row
hipError_t launch_logprob_finalize(float* out, const float2* partial, const float* tgt, int M, int n_tiles, hipStream_t s);
hipError_t launch_logprob_rows(float* out, const float* logits, int ld, const int32_t* target, int M, int V, hipStream_t s);
// bad_id (nullable): receives 1 + the index of an out-of-range token id (atomic max); such ids read row 0 / vocab-1
hipError_t launch_embedding(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, uint32_t* bad_id,
                            hipStream_t s);
hipError_t launch_rmsnorm(void* out, const void* x, const void* w, int T, int D, float eps, hipStream_t s);
hipError_t launch_rope(void* qkv, int ld, int T, int H, int Hkv, int Dh, const float* rope_cs, const int32_t* tok_pos,
                       hipStream_t s);
// Per-row (per-token) e4m3 quantisation of bf16 rows x [M, K] (row stride ldx elements): xq [M, K] bytes, sx [M] fp32, by the rule
// of mistral_inference.quant.quantize_rows - sx = 2^ceil(log2(amax / 448)) (an all-zero row: 1), byte = e4m3_rne(clamp(x / sx,
// +-448)), never a NaN code.  norm_w != nullptr: the row quantised is the bf16 row launch_rmsnorm would have written.
// K % 8 == 0, K <= 16384, ldx % 8 == 0.
hipError_t launch_act_quant_e4m3(void* xq, float* sx, const void* x, int ldx, int M, int K, const void* norm_w, float eps,
                                 hipStream_t s);
hipError_t launch_kv_write(void* ck, void* cv, int W, const void* k, const void* v, int ld, int T, int kv_dim,
                           const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_start, int kv_layout, int Dh, hipStream_t s);
// kv_layout with MI_KV_E4M3 (launch_kv_write): bf16 rows in, e4m3 bytes to the ring.  launch_kv_dequant: n_elems e4m3 bytes of
// each of sk / sv -> bf16 in dk / dv (n_elems % 16 == 0)
hipError_t launch_kv_dequant(void* dk, void* dv, const void* sk, const void* sv, size_t n_elems, hipStream_t s);
// engine_ctrl (nullable): control words of the workspace - CTRL_EPOCH and CTRL_STEPS are incremented here, CTRL_ABORT is cleared
// here, CTRL_BAD_ID receives the out-of-range token id flag (launch_embedding)
hipError_t launch_decode_prep(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before, int32_t* tok_seq,
                              int32_t* tok_pos, int B, uint32_t* engine_ctrl, hipStream_t s);
hipError_t launch_decode_prep_embedding(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before, int32_t* tok_seq,
                                        int32_t* tok_pos, int B, void* out, const void* table, const int64_t* ids, int D,
                                        int vocab, uint32_t* engine_ctrl, hipStream_t s);
hipError_t launch_add_rows(void* out, const void* a, const void* b, size_t n, hipStream_t s);
// Greedy sampling of B logits rows (generate.py:124-136 at temperature 0): tok[b] = first index of the row maximum
// (torch.argmax), lp[b] = log_softmax(row)[tok[b]]; also stored at entry (ctrl[CTRL_STEPS] - 1) % hist_len of the
// [hist_len, B] history rings when given (CTRL_STEPS = decode steps started on this workspace, advanced by decode_prep).
hipError_t launch_greedy_rows(const float* logits, int ld, int B, int V, int64_t* tok, float* lp, int64_t* hist_tok,
                              float* hist_lp, int hist_len, const uint32_t* ctrl, hipStream_t s);
// Nucleus sampling of B logits rows (generate.py:151-170 + the logprob of :134-136), csrc/sampling.hip: tok[b] drawn from
// softmax(row / temperature) restricted to the top-p prefix; uniforms (nullable): u[b] in [0, 1) instead of the Philox draw
// keyed by (seed; offset + ctrl[CTRL_STEPS], b); history rings as launch_greedy_rows.
hipError_t launch_sample_top_p(const float* logits, int ld, int B, int V, float temperature, float top_p, uint64_t seed,
                               uint64_t offset, const float* uniforms, int64_t* tok, float* lp, int64_t* hist_tok, float* hist_lp,
                               int hist_len, const uint32_t* ctrl, hipStream_t s);
// Sampled verification of T logits rows in B sequences (mi_verify_sample), csrc/sampling.hip: one block per row decides accept /
// residual draw / plain draw against ids[t + 1], then one thread per sequence scans its rows - tok[T], lp[T], n_accept[B].
// uniforms (nullable): (u_acc, u_draw)[t] instead of the Philox draw keyed by (seed; offset, t).  Two launches.
hipError_t launch_verify_sample(const float* logits, int ld, int T, int B, int V, const int64_t* ids, const int32_t* q_start,
                                float temperature, float top_p, uint64_t seed, uint64_t offset, const float* uniforms, int64_t* tok,
                                float* lp, int32_t* n_accept, hipStream_t s);
// control words of a workspace after a raised engine status: status / abort / arrivals cleared, epoch advanced
hipError_t launch_engine_ctrl_reset(uint32_t* ctrl, hipStream_t s);

// ---------------------------------------------------------------------------------------------- MoE
hipError_t launch_moe_router(int32_t* sel_idx, float* sel_w, const void* x, int ldx, int T, int D, const void* gate,
                             int E, int top_k, const void* norm_w, float eps, hipStream_t s);
// Sort the (token, slot) pairs by expert: tok_of[r] = token of compact row r, row_of[t*top_k + kk] = compact row of
// that pair, tile_tab / n_tiles = the grouped GEMM's m-tile table (128 rows per tile, tiles never span experts).
hipError_t launch_moe_lists(const int32_t* sel_idx, int T, int E, int top_k, int32_t* tok_of, int32_t* row_of,
                            int32_t* tile_tab, int32_t* n_tiles, int tile_rows, hipStream_t s);
// out[t] = bf16(h[t] + R_t), R_t = sum over the token's experts in ascending id of bf16(w * y[row]), accumulated in
// bf16 from zero (moe.py:28-32 + transformer_layers.py:168)
hipError_t launch_moe_combine(void* out, const void* h, const void* y, const int32_t* sel_idx, const float* sel_w,
                              const int32_t* row_of, int T, int D, int top_k, hipStream_t s);


// ---------------------------------------------------------------------------------------------- persistent decode engine
// decode_engine.hip: one launch per (up to ENG_MAXL) layers of a batch-1 decode step on a dense model.
constexpr int ENG_MAXL = 32;  // layers per launch: bounded by the 4 KiB kernel-argument segment

struct EngLayer {
  const bf16_t *an, *wq, *wk, *wv, *wo, *fn, *w1, *w2, *w3;
  bf16_t *ck, *cv;
  int W, n_splits, chunk, kv_layout;  // kv_layout: MI_KV_SLOT_MAJOR / MI_KV_HEAD_MAJOR (common.cuh)
};

struct EngArgs {
  int n_layers, D, H, Hkv, F, V;
  int R, kv_groups, Hs;   // query heads per scheduled kv head; groups per real kv head; scheduled kv heads
  int NB, ring_fills;
  int seq_base;           // global index of this launch's first layer (tag sequence)
  int first, head;
  int thin, depth;        // loader knobs (A/B): during hand-off sweeps 0 stream / 1 one fill in flight / 2 stop; fills in flight (2 or 3)
  int holders;            // 1: holder waves take the last W1|W3 units of every CU's slab (A/B: MI_ENGINE_HOLDERS=0)
  int commit;             // 1: this launch ends the decode step: workgroup 0 advances kv_seqlens / epoch / step counter
  int hist_len;           // entries of the greedy history ring (0: none)
  float eps;
  bf16_t* h;              // [D] residual stream, in (first layer, unless emb) / out (last layer)
  const bf16_t* emb;      // token embedding table [V, D]: the first layer's input is row ids[0] (nullptr: read h)
  const int64_t* ids;     // [1] token id of this step (may alias greedy_tok: it is read before anything is committed)
  int64_t* kv_seqlens;    // [1] position of this step's token; + 1 at commit (cache.py:193-195)
  int32_t *q_start, *kv_before, *tok_seq, *tok_pos;  // the step's metadata words, written at commit for callers (launch-path layout)
  int64_t* greedy_tok;    // [1] argmax of the logits (first maximal index), or nullptr
  float* greedy_lp;       // [1] log_softmax(logits)[argmax]
  int64_t* hist_tok;      // [hist_len] ring indexed by the step counter (CTRL_STEPS) or nullptr
  float* hist_lp;
  const float* rope_cs;
  const bf16_t* final_norm;
  const bf16_t* output;
  float* logits;
  uint64_t* gran;         // granule regions
  uint32_t* ctrl;         // the workspace control words (CTRL_*)
  uint32_t g_h, g_qkv, g_att, g_h1, g_hid, g_hid2, g_part, g_amax;
  int E;                  // experts (0: dense).  MoE layers: EngLayer.w1 = gate [E, D], .w2 = device table [E][3] of (w1, w2, w3)
  unsigned long long* trace;  // optional timeline buffer (debug)
  EngLayer L[ENG_MAXL];
};

struct EngProblem {
  int D, H, Hkv, F, V, n_layers, NB;
  int E, top_k;              // MoE (0, 0: dense)
  float eps;
  const mi_layer_t* layers;  // host
  void* const* cache_k;      // host [n_layers]
  void* const* cache_v;
  const int32_t* W;          // host [n_layers]
  int kv_layout;             // layout of every ring (common.cuh)
  void* h;
  const float* rope_cs;
  const void* emb;           // nullptr: h holds the step's input
  const int64_t* ids;
  int64_t* kv_seqlens;
  int32_t *q_start, *kv_before, *tok_seq, *tok_pos;  // decode metadata words (kept consistent for callers)
  const void* final_norm;
  const void* output;
  float* logits;             // nullptr: no LM head
  int64_t* greedy_tok;       // optional fused greedy sampling (needs logits)
  float* greedy_lp;
  int64_t* hist_tok;
  float* hist_lp;
  int hist_len;
  void* granules;
  size_t granule_bytes;
  uint32_t* ctrl;
  int forced;                // set by the routing (variant 1): take shapes that measured slower than the launch path too (traces, tests)
  int lora_rank;             // > 0: the model carries un-merged LoRA adapters - no engine build takes it (engine_route)
  int quant;                 // != 0: the layers' linears are quantised (mi_forward_w8 / _w4) - no engine build reads them
};
static_assert(sizeof(EngArgs) <= 4096, "EngArgs must fit the kernel-argument segment");
// The same in every build, read by the kernels and by the host side alike:
constexpr int TR_CONS = 18, TR_EVENTS = 26;  // timeline events per layer: consumer wave 0 writes [0, TR_CONS), the loader the rest
constexpr uint32_t ARRIVE_POLLS = 1u << 16;  // ~50 ms: far beyond the ~1 us over which a resident grid starts
constexpr int AMAX_MAX_NB = 1024;            // workgroups the greedy-sampling edge is sized for (decode_engine_applicable: NB <= 1024)

// decode_engine.hip holds the kernels and is compiled once per build below (build_native.py: VARIANT_OBJECTS); every compile
// exports one accessor to this descriptor and nothing else (tests/test_engine_objects.py).  The descriptor holds what only the
// build's own compile knows: its name, the constants its kernels were compiled with, and which kernels it instantiates.
// Everything else about the engine - granule layout, residency census, knobs, applicability, launch, routing - is
// decode_engine_host.hip, compiled once.  Same EngProblem, same granule layout, bit-identical results in every build.
struct EngineBuild {
  const char* name;  // "default", "next", "nemo", "wide", "moe"; "x<N>": a slot of an experiment library
  int wide, headline_only, all4;       // ENG_WIDE, ENG_HEADLINE_ONLY, ENG_ALL4
  int ring_fills, fill, piece;         // the LDS ring: fills, pieces per fill, bytes per piece
  int lds_total, xs_off, res_bytes;    // dynamic LDS per workgroup; offset of the activation region; bytes of the residual slab
  int nthreads;                        // threads per workgroup
  // the instantiation for (query heads per scheduled kv head, MoE, every row a multiple of 4 pieces); nullptr: not instantiated
  const void* (*kernel)(int R, bool moe, bool all4);
};
// frozen since round 3: every dense shape the others decline; MI_ENGINE_VARIANT=2 routes the headline to it for A/B
const EngineBuild& decode_engine_build();
// build_native.ENGINE_NEXT_FLAGS: the dense GQA-4 shapes with rows of 4-piece groups, i.e. the headline model
const EngineBuild& decode_engine_build_next();
// build_native.ENGINE_NEMO_FLAGS: dense GQA-4 models of a large dim whose rows are not multiples of 4 pieces (Mistral-Nemo, dim
// 5120), every DMA from inline asm (the wide build's dense kernels drain the builtin-DMA queue: scripts/engine_loader_waits.py)
const EngineBuild& decode_engine_build_nemo();
// -DENG_WIDE=1: GQA ratio 6 with a 32 KiB hid vector (Mixtral-8x22B: 7-fill ring), rows of an even number of pieces that is not
// a multiple of 4 (contiguous units)
const EngineBuild& decode_engine_build_wide();
// -DENG_WIDE=2: the wide build's additions on the 8-fill ring, for MoE models whose hid vector fits beside it (Mixtral-8x7B)
const EngineBuild& decode_engine_build_moe();

// ---- decode_engine_host.hip
size_t decode_engine_granule_bytes(int D, int H, int Hkv, int F, int maxW);
size_t decode_engine_trace_bytes(int NB);
// A batch-1 decode step on the first build of the route (engine_route) that takes it.
struct EngStep {
  bool ran;          // the step's launches are enqueued, or one of them failed (err); false: take the launch path
  hipError_t err;
  const char* what;  // names the launch for an error message
  bool declined;     // a shipped build was asked and its residency census had failed: decode_engine_census_detail() says why
};
EngStep decode_engine_step(const EngProblem& pr, hipStream_t s);
// the whole chain of builds a step of this shape would try, as "name,name" (every ring of cache_size slots); returns the length
// the list needs, out_len or more if it was cut
size_t decode_engine_route_names(int D, int H, int Hkv, int F, int V, int E, int top_k, int n_layers, int cache_size, int NB,
                                 int variant, bool nemo_opt_in, char* out, size_t out_len);
const char* decode_engine_census_detail();
void decode_engine_forget_census();               // tests: the next launch probes again
void decode_engine_set_trace(void* dev_buffer);   // debug: nullptr disables
void decode_engine_set_knobs(int thin, int depth);  // debug / tuning
void decode_engine_set_holders(int on);           // debug / A/B: -1 = environment default
int decode_engine_set_variant(int variant);       // mi_debug_set_engine_variant; returns the previous one

// ---------------------------------------------------------------------------------------------- un-merged LoRA (lora.hip)
// lora.py:71-74 around a base product that the tuned GEMV / GEMM has already written:  t = bf16(A x),
// d = bf16(bf16(B t) * s), y = bf16(base + d), out = epilogue(y).  Up to three adapters share an input (q|k|v, w1|w3).
//
// Adapter banks (ABI v9): with bank.seq_slot != nullptr every A[i] / B[i] is the base of a contiguous per-slot array
// ([slots, r, K] / [slots, n_rows, r]) and row m runs through slot seq_slot[tok_seq[m]] (tok_seq == nullptr: seq_slot[m]); -1 = no
// adapter on that row (d = 0), any other value is clamped into the bank.  The bank is a compile-time mode of the same kernels:
// for one (row, column) both modes run one loop, the same fp32 operations in the same order.  seq_slot == nullptr: the
// single-adapter mode on the pointers as given (slot 0).
struct LoraBank {
  int slots;                // >= 1 (read with seq_slot only)
  const int32_t* tok_seq;   // [T] sequence of a row, or nullptr: row m is sequence m
  const int32_t* seq_slot;  // [B] slot of a sequence, -1 .. slots - 1; nullptr: no bank
};
inline LoraBank lora_bank(int slots, const int32_t* tok_seq, const int32_t* seq_slot) {
  return {slots > 1 ? slots : 1, tok_seq, seq_slot};  // (0 slots: a model or a caller that never asked for a bank)
}
inline bool lora_rank_ok(int rank) { return rank >= 8 && rank <= 64 && rank % 8 == 0; }
struct LoraDownArgs {
  const bf16_t* x;      // [T, ldx] the linear's input (already normalised)
  int ldx, T, K;
  const bf16_t* A[3];   // [r, K] each; nullptr: the segment has no adapter (its slice of t is neither written nor read)
  int nseg, r;
  bf16_t* t;            // [T, nseg * r]; a row on slot -1 is not written
  LoraBank bank;
  int64_t a_stride;     // elements between two slots of a segment's A: r * K
};
struct LoraUpArgs {
  int epi;              // MI_EPI_STORE / MI_EPI_RESIDUAL / MI_EPI_SWIGLU
  int T, N;             // N: output columns (SWIGLU: hidden_dim; the base then holds 2 N columns, W1's then W3's)
  const void* base;     // [T, ldb] bf16(W x): bf16, or fp32 holding bf16 values (base_f32: the GEMV's LOGITS form)
  int ldb, base_f32;
  const bf16_t* t;      // [T, nseg * r]
  const bf16_t* B[3];   // [n_rows of the segment, r] each; nullptr: d = 0
  int n0, n1;           // segment ends as in GemvArgs (STORE / RESIDUAL)
  int nseg, r;
  float scaling;
  bf16_t* out;          // [T, ldo]; may alias a bf16 base (STORE / RESIDUAL) or the residual
  int ldo;
  const bf16_t* residual;  // [T, ldo]
  int fast_silu;        // SiLU as the MFMA GEMM's epilogue evaluates it (swiglu_bf_fast) instead of the GEMV's (swiglu_bf)
  int64_t b_stride[3];  // elements between two slots of a segment's B: n_rows of the segment * r
  LoraBank bank;
};
hipError_t launch_lora_down(const LoraDownArgs& a, hipStream_t s);
hipError_t launch_lora_up(const LoraUpArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------- generic storage dtype
// generic.hip: the operator sequence of the hot path for fp32 / fp16 storage (and for bf16 shapes the tuned kernels
// decline), every rounding point in the storage dtype as the reference executes it.  mi_forward_generic (api.hip).
enum { G_DT_BF16 = 0, G_DT_FP16 = 1, G_DT_FP32 = 2 };
enum { G_EPI_STORE = 0, G_EPI_RESIDUAL = 1, G_EPI_LOGITS = 2, G_EPI_SWIGLU = 3 };
struct GLinearArgs {
  const void* x;         // [M, K], row stride ldx
  int ldx;
  const void* w;         // [N, K] dense
  // --- the forms below exist on the M <= 8 kernel only (launch_g_linear refuses them otherwise; g_gemv_takes())
  const void* w1;        // optional second / third weight matrix: output columns [n0, n1) are rows of w1, [n1, N) rows of w2
  const void* w2;        //   (q | k | v in one launch).  G_EPI_SWIGLU: out[m, n] = silu(x . w[n]) * (x . w1[n]), N rows each
  int n0, n1;
  const void* norm_w;    // optional fused RMSNorm of x ([K] weights, `eps`): the contraction runs on round(round(x inv) w)
  float eps;
  void* out;             // [M, N] storage dtype (fp32 for G_EPI_LOGITS), row stride ldo
  int ldo;
  const void* residual;  // G_EPI_RESIDUAL: [M, N], row stride ldr (may alias out)
  int ldr;
  int M, N, K;
  int epi;
  const int32_t* active; // optional [M]: MoE row mask (nothing is done when no row of a tile is active)
};
struct GAttnArgs {
  void* out;             // [T, H * Dh]
  int ldo;
  const void* qkv;       // [T, ld]: q | k | v after RoPE
  int ld;
  const void* cache_k;   // rings [max_batch, W, Hkv, Dh] or head-major [max_batch, Hkv, W, Dh] (nullptr: cache=None call)
  const void* cache_v;
  int kv_layout;
  int W, T, H, Hkv, Dh;
  const int32_t* q_start;
  const int32_t* kv_before;
  const int32_t* tok_seq;
  const int32_t* tok_pos;
  int causal;            // 0: the cache=None call (every token sees every token, transformer_layers.py:165)
  float scale;
  float* partial;        // scratch of g_attn_partial_floats(T, H, Dh) floats: launches with few (token, head) pairs split the keys
  int B, max_q_len;      // sequences / longest new-token run of the forward (0: unknown - the MFMA prefill route is not taken)
};
size_t g_elem_bytes(int dt);
size_t g_attn_partial_floats(int T, int H, int Dh);
bool g_gemv_takes(int M, int K, int ldx);  // the M <= 8 kernel (fused norm / multi-matrix / SwiGLU forms) applies
bool g_linear_fused_ok(int dt, const GLinearArgs& g);  // a multi-matrix / SwiGLU request has a kernel (M <= 8 rows, or fp16 with >= 256 rows)
hipError_t launch_g_embedding(int dt, void* out, const void* table, const int64_t* ids, int T, int D, int vocab, uint32_t* bad_id,
                              hipStream_t s);
hipError_t launch_g_rmsnorm(int dt, void* out, const void* x, const void* w, int T, int D, float eps, hipStream_t s);
hipError_t launch_g_linear(int dt, const GLinearArgs& g, hipStream_t s);
hipError_t launch_g_rope(int dt, void* qkv, int ld, int T, int n_rot_cols, int Dh, const float* rope_cs, const int32_t* tok_pos,
                         hipStream_t s);
hipError_t launch_g_kv_write(int dt, void* ck, void* cv, int W, const void* k, const void* v, int ld, int T, int kv_dim,
                             const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_start, int kv_layout, int Dh, hipStream_t s);
hipError_t launch_g_attention(int dt, const GAttnArgs& a, hipStream_t s);
hipError_t launch_g_swiglu(int dt, void* a, const void* b, int T, int F, const int32_t* active, hipStream_t s);
hipError_t launch_g_moe_topk(int dt, const void* logits, int T, int E, int k, int32_t* sel_idx, float* sel_w, hipStream_t s);
hipError_t launch_g_moe_mask(const int32_t* sel_idx, const float* sel_w, int T, int k, int e, int32_t* active, float* wt, hipStream_t s);
hipError_t launch_g_moe_accum(int dt, void* results, const void* y, const int32_t* active, const float* wt, int T, int D, hipStream_t s);
hipError_t launch_g_add(int dt, void* out, const void* a, const void* b, size_t n, hipStream_t s);
hipError_t launch_g_zero(int dt, void* p, size_t n, hipStream_t s);
hipError_t launch_g_gelu(int dt, void* x, int ldx, int T, int N, hipStream_t s);
