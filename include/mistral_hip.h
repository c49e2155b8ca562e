/*
 * mistral_hip.h -- C ABI of libmistral_hip.so: the MI355X (gfx950) implementation of
 * mistral-inference's `Transformer.forward_partial` hot path.
 *
 * The reference (mistralai/mistral-inference v1.6.0) has NO FFI/plugin layer of its own: its hot
 * path calls torch/xformers kernels from Python.  This header is therefore the boundary a
 * maintainer would bind (ctypes stub in INTEGRATION.md); every entry point names the reference
 * lines whose work it replaces.  Paths are relative to src/mistral_inference/ of the reference.
 *
 * Conventions
 *   - plain C types only; all tensor arguments are raw DEVICE pointers unless marked "host";
 *   - storage dtype is bf16 (uint16 payload), row-major, innermost dimension contiguous;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates,
 *     frees or synchronises, and keeps no state between calls (scratch comes from the caller);
 *   - return value: 0 = ok, >0 = hipError_t of a failed launch, <0 = MI_ERR_* argument check;
 *     `mi_error_string` turns any of them into text.  The Python host raises RuntimeError.
 *   - numerics contract (rounding points): SURVEY.md Appendix A / DESIGN.md section 4.
 */
#ifndef MISTRAL_HIP_H
#define MISTRAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 9

#define MI_OK 0
#define MI_ERR_ARG (-1)        /* null pointer / non-positive size                        */
#define MI_ERR_SHAPE (-2)      /* shape not supported by the gfx950 kernels (see message) */
#define MI_ERR_WORKSPACE (-3)  /* caller workspace too small                              */
#define MI_ERR_UNSUPPORTED (-4)
#define MI_ERR_RCCL (-5)       /* a RCCL call failed: text in mi_rccl_last_error()        */

typedef void* mi_stream_t; /* hipStream_t */

int mi_abi_version(void);
const char* mi_error_string(int code);
/* text of the last MI_ERR_* raised on this thread (empty string if none) */
const char* mi_last_error_detail(void);

/* ------------------------------------------------------------------------------------------------
 * Leaf operators (each replaces one group of torch/xformers launches of the reference)
 * ---------------------------------------------------------------------------------------------- */

/* transformer.py:193  h = tok_embeddings(input_ids).  out[T,D] = table[ids[t], :].  ids must lie in [0, vocab): the
 * reference raises IndexError otherwise, which a kernel cannot - this leaf reads row 0 / vocab-1 for such an id (callers
 * validate; mi_forward additionally records the offending token index in the workspace, see mi_decode_engine_status). */
int mi_embedding(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, mi_stream_t stream);

/* transformer_layers.py:115-120 RMSNorm.forward: out = bf16(bf16(x_f32 * rsqrt(mean(x^2)+eps)) * w).
 * In-place (out == x) is allowed. */
int mi_rmsnorm(void* out, const void* x, const void* w, int T, int D, float eps, mi_stream_t stream);

/* rope.py:13-23 apply_rotary_emb, in place on the q and k column blocks of a fused activation
 * buffer qkv[T, ld] = [ q (n_heads*Dh) | k (n_kv_heads*Dh) | v ... ].
 * rope_cs: fp32 [rope_len, Dh/2, 2] = (cos, sin), i.e. view_as_real of the reference's complex64
 * freqs_cis table (rope.py:6-10, transformer.py:113-116); tok_pos[T] absolute positions. */
int mi_rope_inplace(void* qkv, int ld, int T, int n_heads, int n_kv_heads, int head_dim, const float* rope_cs,
                    int rope_len, const int32_t* tok_pos, mi_stream_t stream);

/* cache.py:83-92 CacheView.update with to_cache_mask / cache_positions of cache.py:226-235:
 * token t (sequence b = tok_seq[t], index i = t - q_start[b] of s_b = q_start[b+1]-q_start[b] new
 * tokens) is stored iff i >= s_b - W, into ring slot tok_pos[t] % W of row b.
 * k/v: [T, ld] activation views (already at the k / v column), cache_k/v: one layer's rings in `kv_layout` (below). */
int mi_kv_write(void* cache_k, void* cache_v, int W, const void* k, const void* v, int ld, int T, int kv_dim,
                const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_start, int kv_layout, int head_dim,
                mi_stream_t stream);

/* ABI v7 - layout of a layer's K/V rings in HBM.  A kv head's head_dim elements are contiguous in both:
 *   MI_KV_SLOT_MAJOR  [max_batch, W, n_kv_heads, head_dim]: the reference's torch.empty shape (cache.py:163-167)
 *   MI_KV_HEAD_MAJOR  [max_batch, n_kv_heads, W, head_dim]: the slots of ONE kv head are contiguous, so the keys a decode work
 *                     item (kv head, range of slots) reads are a single run - 4-KiB runs that the persistent engine streams at
 *                     its weight rate; the strided form costs it 1.2 us per 16 KiB against 0.66.  What
 *                     mistral_inference.cache.BufferCache allocates (exposed to Python as a permuted view of the reference's shape).
 * Every entry point that touches a ring takes the layout; all rings of one mi_forward call share it (mi_batch_t.kv_layout). */
#define MI_KV_SLOT_MAJOR 0
#define MI_KV_HEAD_MAJOR 1
/* FP8 K/V rings (additive to ABI v9: the presence of mi_kv_dequant is the feature test).  OR-ed into a layout code: the rings hold
 * OCP e4m3 bytes (torch.float8_e4m3fn) instead of bf16 elements, same shapes and layouts, no scales.
 *   write rule  byte = e4m3_rne(clamp(float(x), -448, 448)) of every bf16 x: +-inf saturates to +-448, NaN stays an e4m3 NaN
 *   read rule   bf16(e4m3(byte)), exact
 * so that an attention result on an e4m3 ring is, bit for bit, the bf16 kernel's on a bf16 ring holding the dequantised values.
 * The valid layout codes are 0, 1, 0x10 and 0x11.  With the flag: mi_kv_write takes bf16 rows and writes bytes; mi_attn_decode
 * reads bytes (the same split geometry and visit order as on bf16 rings); mi_qkv_rope_kvwrite[_w8/_w4] run the GEMV without its
 * fused ring write, then the e4m3 ring write; mi_attn_prefill returns MI_ERR_UNSUPPORTED (mi_kv_dequant the rings first);
 * mi_forward / _w8 / _w4 run on such rings (below); mi_forward_generic refuses them.  Scales are not implemented. */
#define MI_KV_E4M3 0x10

/* e4m3 rings of B sequences -> bf16 rings of the same layout: dst[i] = bf16(e4m3(src[i])) over B * W * n_kv_heads * head_dim
 * elements each of K and V.  kv_layout: with or without MI_KV_E4M3 (the source is e4m3 either way; an element-wise pass, so the
 * layout does not enter).  The element count per ring must be a multiple of 16. */
int mi_kv_dequant(void* dst_k, void* dst_v, const void* src_k, const void* src_v, int W, int B, int n_kv_heads, int head_dim,
                  int kv_layout, mi_stream_t stream);

/* Epilogues of the dense contractions */
enum mi_epilogue {
  MI_EPI_STORE = 0,    /* out = bf16(acc)                                  nn.Linear                       */
  MI_EPI_RESIDUAL = 1, /* out = bf16(residual + bf16(acc))                 transformer_layers.py:166,168   */
  MI_EPI_SWIGLU = 2,   /* out = bf16(bf16(silu(bf16(acc1))) * bf16(acc3))  transformer_layers.py:105-106   */
  MI_EPI_LOGITS = 3    /* out_f32 = float(bf16(acc))                       transformer.py:235,239-242      */
};

/* out[M,N] = epilogue(x[M,K] @ W^T).  W is given as up to three row blocks (w[i] has n_rows[i]
 * rows of K bf16; used for the fused Wq|Wk|Wv projection, transformer_layers.py:66) except for
 * MI_EPI_SWIGLU where w[0]=W1, w[1]=W3 (both [N,K]).  M <= 8 runs the weight-streaming GEMV kernels
 * (HBM-bound), M > 8 the MFMA GEMM.  norm_w != NULL fuses RMSNorm(x; norm_w, eps) in front
 * (GEMV path only; the GEMM path requires norm_w == NULL).
 * residual: [M, ldo] (may alias out).  out is bf16 [M, ldo] (fp32 for MI_EPI_LOGITS). */
int mi_linear(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
              int epilogue, const void* residual, const void* norm_w, float eps, mi_stream_t stream);

/* ABI v8 - lora.py:71-74 LoRALinear.forward on a bf16 model: mi_linear with un-merged adapters beside the frozen weight.
 * Segment i (w[i], n_rows[i]) has the adapter A[i] [rank, K], B[i] [n_rows[i], rank]; a NULL pair = no adapter.  With fp32
 * accumulation in each product:
 *     t = bf16(A x)      d = bf16(bf16(B t) * scaling)      y = bf16(bf16(W x) + d)      out = epilogue(y)
 * where y stands exactly where bf16(acc) stands in mi_linear's epilogues (MI_EPI_STORE, MI_EPI_RESIDUAL, MI_EPI_SWIGLU:
 * w[0] = W1, w[1] = W3 with their own adapters; MI_EPI_LOGITS has no adapter form: the LM head carries none).  The base
 * product bf16(W x) is mi_linear's own GEMV (M <= 8) or MFMA GEMM pass; two more launches form t and apply the rest.
 * rank: a multiple of 8 up to 64 (MI_ERR_SHAPE otherwise).  x is the linear's input; norm_w != NULL (M <= 8 only, as
 * mi_linear) puts RMSNorm(x; norm_w, eps) in front of W and of A.  ldx must be a multiple of 8.
 * scratch: device memory of at least mi_lora_linear_scratch_bytes(M, K, n_rows, epilogue, rank, norm_w != NULL) bytes. */
size_t mi_lora_linear_scratch_bytes(int M, int K, const int n_rows[3], int epilogue, int rank, int fused_norm);
int mi_lora_linear(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const void* const A[3],
                   const void* const B[3], int rank, float scaling, void* scratch, size_t scratch_bytes, mi_stream_t stream);

/* ABI v9 - mi_lora_linear with one adapter PER ROW out of a bank of `slots` adapter sets.  The reference has one adapter set per
 * model (lora.py:52-61); row m here is what lora.py:71-74 computes for that row with the adapters of slot row_slot[m] loaded,
 * with the rounding points of mi_lora_linear - bit for bit the row of an mi_lora_linear call on that slot's A / B.
 * A[i] / B[i]: bases of contiguous per-slot arrays [slots, rank, K] / [slots, n_rows[i], rank] (a NULL pair: no adapter in any
 * slot).  row_slot: device int32 [M], values -1 .. slots - 1; -1 = the row has no adapter (y = bf16(bf16(W x) + 0)); a value
 * outside the range is the caller's error - the kernels clamp it into the bank.  row_slot == NULL: every row on slot 0, on
 * mi_lora_linear's own kernels.  scratch: mi_lora_linear_scratch_bytes, unchanged. */
int mi_lora_linear_slots(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                         int epilogue, const void* residual, const void* norm_w, float eps, const void* const A[3],
                         const void* const B[3], int rank, float scaling, int slots, const int32_t* row_slot, void* scratch,
                         size_t scratch_bytes, mi_stream_t stream);

/* generate.py:101-118 needs, of the prompt's [T, vocab] logits (transformer.py:235-242), only log_softmax(logits)[t, next
 * token]: logprob[m] = l[m, target[m]] - logsumexp(l[m, :]) with l = float(bf16(x @ W^T)), computed in ONE pass over the
 * LM head without materialising the logits (per-tile max / sum-exp partials in `scratch`).  M < 256 rows take the plain
 * logits + row-reduction route inside the same call.  target[m] outside [0, vocab) yields -logsumexp. */
size_t mi_lm_head_logprobs_scratch_bytes(int M, int vocab);
int mi_lm_head_logprobs(float* logprob, const void* x, int ldx, int M, int K, const void* w, int vocab,
                        const int32_t* target, void* scratch, size_t scratch_bytes, mi_stream_t stream);

/* generate.py:124 + :134-136 at temperature 0 for B rows of fp32 logits [B, ld]: token[b] = FIRST index of the row maximum
 * (torch.argmax), logprob[b] = log_softmax(row)[token[b]] - one block per row.  mi_forward fuses the same reduction
 * behind its LM head (mi_batch_t.greedy_token). */
int mi_greedy_sample(const float* logits, int ld, int B, int vocab, int64_t* token, float* logprob, mi_stream_t stream);

/* generate.py:151-170 `sample` / `sample_top_p` at temperature > 0 for B rows of fp32 logits [B, ld], ONE launch (the
 * reference: softmax, a sort of the whole vocabulary, cumsum, masked fill, renormalise, torch.multinomial, gathers):
 *   probs = softmax(row / temperature); the tokens kept are the prefix of the descending order whose mass BEFORE the token
 *   is <= top_p (generate.py:165-167; ties in probability are ordered by ascending index - torch.sort leaves them
 *   unspecified); token[b] is drawn from the renormalised kept masses by inverse CDF in that order;
 *   logprob[b] = log_softmax(row)[token[b]] of the UNSCALED logits (generate.py:134-136).
 * The uniform variate is Philox4x32-10(seed; counter = offset, row b) unless `uniforms` (device fp32 [B], each in [0, 1))
 * is given - which is how tests pin a draw.  Masses are 40-bit fixed point: the result is bit-reproducible for a given
 * seed/offset (torch.multinomial's own stream cannot be reproduced; parity is distributional, tests/test_gpu_sampling.py).
 * mi_forward fuses the same kernel behind its LM head (mi_batch_t.sample_temperature > 0). */
int mi_sample_top_p(const float* logits, int ld, int B, int vocab, float temperature, float top_p, uint64_t seed,
                    uint64_t offset, const float* uniforms, int64_t* token, float* logprob, mi_stream_t stream);

/* Decode-branch attention (transformer_layers.py:77-89 with the mask of cache.py:249-254):
 * one query per sequence, keys = ring slots [0, min(pos+1, W)) of its row, GQA by kv = h / (H/Hkv)
 * (replaces repeat_kv, transformer_layers.py:16-19,84).  q: [B, ldq] (H*Dh used), out: [B, H*Dh].
 * tok_pos[b] = position of the new token (already written to the ring).  scratch: fp32, at least
 * mi_attn_decode_scratch_bytes(...) bytes; its first `B*Hkv` int32 words are arrival counters that
 * must be zero at the first call (the kernel leaves them zero). */
size_t mi_attn_decode_scratch_bytes(int B, int n_heads, int n_kv_heads, int head_dim, int W);
int mi_attn_decode(void* out, const void* q, int ldq, const void* cache_k, const void* cache_v, int W, int B,
                   int n_heads, int n_kv_heads, int head_dim, const int32_t* tok_pos, void* scratch, int kv_layout,
                   mi_stream_t stream);

/* Prefill-branch attention (transformer_layers.py:74-76,84-89; keys of cache.py:94-117 interleave_kv;
 * masks of cache.py:238-248).  For sequence b with s_b new tokens (rows q_start[b]..) and p_b =
 * kv_before[b] tokens already seen, key position kp is visible to query position qp iff
 * qp - W < kp <= qp; keys kp < p_b are read from the ring (slot kp % W, only the last min(p_b,W)
 * exist), keys kp >= p_b from the activation rows.  qkv: [T, ld] fused buffer (post-RoPE).
 * causal == 0 is the cache=None quirk (transformer_layers.py:165): one segment, no mask - also what one image of the
 * vision tower's block-diagonal mask is (vision_encoder.py:96-99).
 * softmax_scale <= 0 selects head_dim^-1/2 (the xformers default the reference relies on, transformer_layers.py:48,88);
 * the vision tower runs its 64-wide heads zero-padded to 128 and passes 64^-1/2.
 * out: [T, H*Dh]. */
int mi_attn_prefill(void* out, const void* qkv, int ld, const void* cache_k, const void* cache_v, int W, int B,
                    int max_q_len, int n_heads, int n_kv_heads, int head_dim, const int32_t* q_start,
                    const int32_t* kv_before, int causal, float softmax_scale, int kv_layout, mi_stream_t stream);

/* nn.GELU() of the vision-language adapter (vision_encoder.py:112-116; exact erf form): x <- bf16(gelu(x)) in place
 * over [T, N] bf16 rows with row pitch ldx. */
int mi_gelu(void* x, int ldx, int T, int N, mi_stream_t stream);

/* moe.py:25-27: logits = bf16(x @ Wg^T); top-k on them; fp32 softmax over the k picked, rounded to
 * bf16.  x is [T, D] (norm_w != NULL fuses the RMSNorm).  sel_idx int32 [T, k], sel_w fp32 [T, k]
 * (bf16-rounded values).  Ties: the lowest expert id wins (torch.topk leaves tie order unspecified). */
int mi_moe_router(int32_t* sel_idx, float* sel_w, const void* x, int ldx, int T, int D, const void* gate, int E,
                  int top_k, const void* norm_w, float eps, mi_stream_t stream);

/* transformer_layers.py:66-70,165 + rope.py:13-23 + cache.py:83-92 for T <= 8 tokens (the decode step) in ONE launch:
 * qkv[t] = [ rope(Wq xn) | rope(Wk xn) | Wv xn ] with xn = RMSNorm(x[t]; norm_w, eps) (norm_w == NULL: xn = x), every
 * projection rounded to bf16 before the rotation; when cache_k/cache_v are given the new K/V rows are also stored into
 * ring slot tok_pos[t] % W of row tok_seq[t] (tok_seq == NULL: row t) - CacheView.update at decode.
 * qkv: [T, ldo] bf16, ldo >= (n_heads + 2 n_kv_heads) * head_dim.  T > 8: MI_ERR_UNSUPPORTED (the prefill path is
 * mi_rmsnorm + mi_linear + mi_rope_inplace + mi_kv_write). */
int mi_qkv_rope_kvwrite(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                        const void* wv, int n_heads, int n_kv_heads, int head_dim, const void* norm_w, float eps,
                        const float* rope_cs, int rope_len, const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k,
                        void* cache_v, int W, int kv_layout, mi_stream_t stream);

/* moe.py:28-32 (+ the residual add of transformer_layers.py:168) for T <= 8 tokens, two launches, no host sync:
 * out[t] = bf16(residual[t] + R_t), R_t = sum over the token's picked experts in ascending expert id of
 * bf16(w * bf16(W2_e . bf16(silu(W1_e xn) * W3_e xn))), accumulated in bf16 from zero; xn = RMSNorm(x[t]) when norm_w is
 * given.  expert_w_dev: DEVICE array [E][3] of (w1, w2, w3) pointers; sel_idx/sel_w: mi_moe_router's output [T, top_k];
 * hidden_scratch: bf16 [T * top_k, F].  out may alias residual. */
int mi_moe_experts_decode(void* out, const void* residual, const void* x, int ldx, int T, int D, int F,
                          const void* const* expert_w_dev, const int32_t* sel_idx, const float* sel_w, int top_k,
                          const void* norm_w, float eps, void* hidden_scratch, mi_stream_t stream);

/* The same layer for any T (prefill): (token, slot) pairs sorted by expert ON THE DEVICE (the reference does one
 * torch.where host sync per expert per layer, moe.py:30), ONE token-grouped MFMA GEMM launch per projection over all
 * experts, then the ordered bf16 combine + residual.  x: dense [T, D] (already ffn-normalised), ldx == D. */
size_t mi_moe_grouped_gemm_scratch_bytes(int T, int D, int F, int E, int top_k);
int mi_moe_grouped_gemm(void* out, const void* residual, const void* x, int ldx, int T, int D, int F, int E, int top_k,
                        const void* const* expert_w_dev, const int32_t* sel_idx, const float* sel_w, void* scratch,
                        size_t scratch_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole local layer stack: Transformer.forward_partial (transformer.py:163-219) + the LM head of
 * Transformer.forward (transformer.py:229-242)
 * ---------------------------------------------------------------------------------------------- */
/* ABI v8 - un-merged LoRA adapters of one layer (lora.py:52-61): A [rank, in], B [out, rank], bf16, for each of the seven
 * linears.  A NULL pair: that linear has no adapter.  The MoE gate and the LM head never have one.
 * ABI v9 - with mi_model_t.lora_slots > 1 every non-NULL pointer is the base of a contiguous per-slot array:
 * A [lora_slots, rank, in], B [lora_slots, out, rank]; slot 0 is what ABI v8 pointed to. */
typedef struct mi_lora_layer {
  const void *wq_a, *wq_b, *wk_a, *wk_b, *wv_a, *wv_b, *wo_a, *wo_b;
  const void *w1_a, *w1_b, *w2_a, *w2_b, *w3_a, *w3_b;
} mi_lora_layer_t;

typedef struct mi_layer {
  const void* attention_norm; /* [D]            transformer_layers.py:143 */
  const void* wq;             /* [H*Dh, D]      transformer_layers.py:51  */
  const void* wk;             /* [Hkv*Dh, D]                         :52  */
  const void* wv;             /* [Hkv*Dh, D]                         :53  */
  const void* wo;             /* [D, H*Dh]                           :54  */
  const void* ffn_norm;       /* [D]                                 :144 */
  const void* w1;             /* [F, D]  dense FFN (NULL when MoE)   :101 */
  const void* w2;             /* [D, F]                              :102 */
  const void* w3;             /* [F, D]                              :103 */
  const void* gate;           /* [E, D]  MoE router (NULL when dense) moe.py:20 */
  const void* const* expert_w_dev;  /* DEVICE array [E][3] of (w1,w2,w3) pointers, moe.py:19 */
  const void* const* expert_w_host; /* the same table in host memory */
  const mi_lora_layer_t* lora;      /* ABI v8: host pointer, read when mi_model_t.lora_rank > 0 (NULL: no adapter in this layer) */
} mi_layer_t;

typedef struct mi_model {
  int32_t dim, n_heads, n_kv_heads, head_dim, hidden_dim, vocab_size;
  int32_t n_layers;               /* layers local to this pipeline rank (transformer.py:94-98) */
  int32_t num_experts, top_k;     /* 0,0 for dense */
  float norm_eps;
  const void* tok_embeddings;     /* [V, D] or NULL when pipeline_rank > 0 (transformer.py:56-57) */
  const void* final_norm;         /* [D]    or NULL when not the last rank (transformer.py:77-79) */
  const void* output;             /* [V, D] or NULL */
  const float* rope_cs;           /* fp32 [rope_len, Dh/2, 2] */
  int32_t rope_len;
  const mi_layer_t* layers;       /* host array [n_layers] */
  /* ABI v8 - un-merged LoRA (params.json `lora`, lora.py:12-19).  0 / 0.0 (a zero-initialised struct): none.  rank > 0:
   * every linear of every layer runs as mi_lora_linear describes, on the launch path for every T (the persistent engine
   * declines such a model); dense bf16 models only - a MoE model and mi_forward_generic return MI_ERR_UNSUPPORTED. */
  int32_t lora_rank;              /* multiple of 8 up to 64 */
  float lora_scaling;
  /* ABI v9 - adapter bank: lora_slots adapter sets (lora.py:52-61 each) beside ONE set of frozen weights, one of them chosen per
   * sequence by mi_batch_t.seq_adapter.  0 and 1 both mean one slot: the ABI v8 behaviour.  Needs lora_rank > 0 (MI_ERR_ARG). */
  int32_t lora_slots;
} mi_model_t;

enum mi_branch {
  MI_BRANCH_NOCACHE = 0, /* cache=None: positions restart per sequence, attention unmasked         */
  MI_BRANCH_PREFILL = 1, /* first or subsequent prefill chunk (cache.py:236-248)                   */
  MI_BRANCH_DECODE = 2   /* all seqlens == 1 and tokens already cached (cache.py:249-254)          */
};

typedef struct mi_batch {
  int32_t T, B, branch;
  int32_t max_q_len;            /* host: max(seqlens) */
  const int64_t* input_ids;     /* dev [T]; embedded into h when model->tok_embeddings != NULL; NULL: h is the input */
  /* sequence metadata, device int32.  PREFILL/NOCACHE: written by the host (one H2D copy per
   * forward -- the reference rebuilds five tensors per LAYER, cache.py:226-263).
   * DECODE: filled on the device from kv_seqlens by the first kernel of the step. */
  int32_t* q_start;             /* [B+1] */
  int32_t* kv_before;           /* [B]   */
  int32_t* tok_seq;             /* [T]   */
  int32_t* tok_pos;             /* [T]   */
  int64_t* kv_seqlens;          /* dev [B] BufferCache.kv_seqlens (cache.py:170,193-195); DECODE reads
                                   positions from it and adds 1 on the device; NULL for NOCACHE */
  void* const* cache_k;         /* host array [n_layers] of dev rings: [max_batch, W_l, Hkv, Dh] (cache.py:163-167) or head-major
                                   [max_batch, Hkv, W_l, Dh], as kv_layout (last field) says */
  void* const* cache_v;
  const int32_t* cache_sizes;   /* host [n_layers] W_l (cache.py:13-24) */
  void* h;                      /* dev [T, D] bf16, in/out: the residual stream.  rank 0: overwritten by
                                   the embedding; rank>0: holds the received activations.  On return: the
                                   block-stack output, RMS-normalised when final_norm != NULL and
                                   logits == NULL (transformer.py:213-219) */
  float* logits;                /* dev [T, V] fp32 or NULL (transformer.py:235-242) */
  void* workspace;              /* dev scratch, >= mi_workspace_bytes(model, T, B, max W) */
  size_t workspace_bytes;
  /* ABI v4 - greedy sampling fused behind the LM head (generate.py:124 `torch.argmax(logits)` and :134-136
   * `log_softmax(logits)[token]` at temperature 0).  Optional (NULL: not computed); DECODE branch with `logits` only.
   *   greedy_token[b]   = first index of the maximum of logits[b, :]            (torch.argmax's tie rule)
   *   greedy_logprob[b] = log_softmax(logits[b, :])[greedy_token[b]]
   * `input_ids` MAY ALIAS `greedy_token`: the ids are consumed before the outputs are written, so a caller can chain
   * steps (the next step's input is this step's sample) without any copy between two mi_forward calls - the shape of
   * generate()'s greedy loop, and of a captured hipGraph that is replayed once per token.
   * hist_token / hist_logprob: optional rings [hist_len, B]; the step's sample is also stored at row
   * (steps % hist_len), `steps` being the number of decode steps this workspace has run before this one
   * (mi_decode_engine_status word 5; the caller may zero that word) - so a generation loop reads its tokens back in
   * ONE copy at the end instead of one per step (generate.py:137 `generated_tensors.append`). */
  int64_t* greedy_token;        /* dev [B] or NULL */
  float* greedy_logprob;        /* dev [B] */
  int64_t* hist_token;          /* dev [hist_len, B] or NULL */
  float* hist_logprob;          /* dev [hist_len, B] or NULL */
  int32_t hist_len;
  /* ABI v5 - nucleus sampling instead of the argmax (generate.py:126 `sample(logits, temperature, top_p=0.8)`): with
   * sample_temperature > 0 the token written to greedy_token / the history ring is DRAWN as mi_sample_top_p describes
   * (one more small kernel behind the LM head, inside the same captured step), greedy_logprob is its log-probability under
   * the unscaled logits.  The variate of a step, row b is Philox(sample_seed; sample_offset + n, b) with n = the workspace's
   * decode-step counter (mi_decode_engine_status word 5) - a device value, so hipGraph replays draw fresh numbers; a caller
   * that wants the stream of a generation to start at the same point every time passes sample_offset = -(counter at its
   * start).  sample_temperature == 0: the ABI v4 behaviour (argmax). */
  float sample_temperature;
  float sample_top_p;
  uint64_t sample_seed;
  uint64_t sample_offset;
  /* ABI v7 */
  int32_t kv_layout;            /* MI_KV_SLOT_MAJOR (0, the reference's shape) or MI_KV_HEAD_MAJOR: layout of EVERY ring in cache_k / cache_v */
  /* ABI v9 - one LoRA adapter set per sequence (lora.py:71-74 per row): the rows of sequence b are what the reference computes
   * for that sequence with the adapters of slot seq_adapter[b] loaded.  Values -1 .. lora_slots - 1; -1 = the base model for that
   * sequence.  Read on all three branches through tok_seq (NOCACHE: tok_seq[t] must then name the row's entry of seq_adapter).
   * NULL: every sequence on slot 0, the ABI v8 launches.  Non-NULL with lora_rank == 0: MI_ERR_ARG.  The pointer, not the
   * values, is what a captured step holds: a caller may rewrite the array between replays. */
  const int32_t* seq_adapter;   /* dev [B] or NULL */
} mi_batch_t;

size_t mi_workspace_bytes(const mi_model_t* model, int T, int B, int max_cache_size);
/* The workspace must be ZERO-FILLED once after allocation (the first 4 KiB hold the control words of the persistent
 * decode engine - step epoch, status - and the engine's hand-off granules carry tags that must never match garbage). */
int mi_forward(const mi_model_t* model, const mi_batch_t* batch, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight-only FP8 (OCP e4m3, what torch.float8_e4m3fn and safetensors F8_E4M3 store) on dense bf16 models.  Additive to ABI
 * v9: no struct above changes and no entry point above changes meaning; the presence of these symbols is the feature test.
 * The reference has no quantised linear: a quantised linear here stands for the nn.Linear of transformer_layers.py:51-54,
 * 101-103 on the real-valued weight  W[r, k] = scale[r] * e4m3(w[r, k])  (w: bytes [out, in]; scale: fp32 [out], positive, finite).
 *   M <= 8:  acc[r] = sum_k e4m3(w[r, k]) * x[k] in fp32, y = acc * scale[r] in fp32, and y enters the epilogues of mi_linear /
 *            mi_qkv_rope_kvwrite exactly where acc enters them there (csrc/gemv_w8.hip; activations, norms and rings stay bf16);
 *   M  > 8:  W' = bf16(scale[r] * e4m3(w[r, k])) is written into a scratch and mi_linear's MFMA GEMM runs on W'.
 * With power-of-two scales W' is exact and both forms are the bf16 model on the dequantised weights up to fp32 summation order;
 * with other scales the two forms differ by one bf16 rounding of each weight.  K must be a multiple of 16 (MI_ERR_SHAPE).
 * Embeddings, norms, the LM head, the MoE gate and the K/V rings stay bf16.
 * ---------------------------------------------------------------------------------------------- */
#define MI_W8_FP8_E4M3 1

/* mi_linear (nn.Linear, transformer_layers.py:66,93,105-106) with w[i] read as e4m3 bytes [n_rows[i], K] and scale[i] their fp32
 * row scales [n_rows[i]].  MI_EPI_STORE / MI_EPI_RESIDUAL / MI_EPI_SWIGLU (MI_EPI_LOGITS: MI_ERR_UNSUPPORTED - the LM head is
 * not quantised).  M > 8 needs `scratch` of at least mi_linear_w8_scratch_bytes(M, K, n_rows, epilogue) bytes (0 for M <= 8,
 * where scratch may be NULL); norm_w as mi_linear (M <= 8 only). */
size_t mi_linear_w8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue);
int mi_linear_w8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                 int epilogue, const void* residual, const void* norm_w, float eps, const float* const scale[3], void* scratch,
                 size_t scratch_bytes, mi_stream_t stream);

/* mi_qkv_rope_kvwrite (transformer_layers.py:66-70,165 + rope.py:13-23 + cache.py:83-92, T <= 8) with wq / wk / wv read as e4m3
 * bytes and sq / sk / sv their fp32 row scales. */
int mi_qkv_rope_kvwrite_w8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                           const void* wv, const float* sq, const float* sk, const float* sv, int n_heads, int n_kv_heads,
                           int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                           const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k, void* cache_v, int W, int kv_layout,
                           mi_stream_t stream);

/* Row scales of the seven linears of one layer (transformer_layers.py:51-54,101-103): DEVICE fp32 [rows of that linear]. */
typedef struct mi_w8_layer {
  const float *wq, *wk, *wv, *wo, *w1, *w2, *w3;
} mi_w8_layer_t;
/* The quantisation of a model's layers: beside an mi_model_t whose seven linear pointers per layer then point to e4m3 bytes. */
typedef struct mi_w8_model {
  int32_t format;               /* MI_W8_FP8_E4M3 */
  const mi_w8_layer_t* layers;  /* host array [n_layers] */
} mi_w8_model_t;

/* mi_workspace_bytes / mi_forward (Transformer.forward_partial, transformer.py:163-219, + the LM head, :229-242) on a model
 * whose linears are quantised as `w8` describes.  w8 == NULL: exactly mi_workspace_bytes / mi_forward.  T <= 8: the six launches
 * per layer of mi_forward on the e4m3 GEMV kernels.  T > 8: per linear group (q|k|v, wo, w1|w3, w2) one dequantisation launch
 * into a scratch carved behind everything else in the workspace (the largest group, only for such a model and such a T), then
 * mi_forward's GEMM launch.  Always the launch path: the persistent engine declines.  Dense models without un-merged LoRA only
 * (num_experts > 0 or lora_rank > 0: MI_ERR_UNSUPPORTED); dim, hidden_dim and n_heads * head_dim multiples of 16. */
size_t mi_workspace_bytes_w8(const mi_model_t* model, const mi_w8_model_t* w8, int T, int B, int max_cache_size);
int mi_forward_w8(const mi_model_t* model, const mi_w8_model_t* w8, const mi_batch_t* batch, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight-only MXFP4 (OCP microscaling: e2m1 codes in blocks of 32 along K, one e8m0 scale byte per block; 4.25 bits per
 * weight) on dense bf16 models.  Additive to ABI v9 like the FP8 block above: the presence of these symbols is the feature test;
 * mi_forward_w8 keeps refusing every format value other than MI_W8_FP8_E4M3.
 * The reference has no quantised linear: a quantised linear here stands for the nn.Linear of transformer_layers.py:51-54,
 * 101-103 on the real-valued weight  W[r, k] = 2^(s[r, k / 32] - 127) * e2m1(c[r, k])  where
 *   c: bytes [out, in / 2], two codes per byte, the LOW nibble at the even k; code & 7 indexes {0, .5, 1, 1.5, 2, 3, 4, 6}, code & 8
 *      is the sign;   s: bytes [out, in / 32], e8m0 (255, its NaN, must not occur).
 * Every such W is exact in bf16.  Numerics contract: at any M the result is what mi_linear / mi_qkv_rope_kvwrite compute on the
 * bf16 matrix W, up to the order of the fp32 summation -
 *   M <= 8:  each code pair becomes a scaled bf16 pair in registers (v_cvt_scalef32_pk_bf16_fp4) and enters the bf16 kernels' dot
 *            products and epilogues (csrc/gemv_w4.hip; activations, norms and rings stay bf16);
 *   M  > 8:  W is written into a scratch as bf16 and mi_linear's MFMA GEMM runs on it.
 * K must be a multiple of 32 (MI_ERR_SHAPE).  Scale bytes below 3 give bf16 subnormals, which the dot product may flush to zero.
 * Embeddings, norms, the LM head, the MoE gate and the K/V rings stay bf16.
 * ---------------------------------------------------------------------------------------------- */
#define MI_W4_MXFP4 2

/* mi_linear (nn.Linear, transformer_layers.py:66,93,105-106) with w[i] read as MXFP4 code bytes [n_rows[i], K / 2] and scale[i]
 * their e8m0 block scales [n_rows[i], K / 32], row-major.  MI_EPI_STORE / MI_EPI_RESIDUAL / MI_EPI_SWIGLU (MI_EPI_LOGITS:
 * MI_ERR_UNSUPPORTED - the LM head is not quantised).  M > 8 needs `scratch` of at least mi_linear_w4_scratch_bytes(M, K, n_rows,
 * epilogue) bytes (0 for M <= 8, where scratch may be NULL); norm_w as mi_linear (M <= 8 only). */
size_t mi_linear_w4_scratch_bytes(int M, int K, const int n_rows[3], int epilogue);
int mi_linear_w4(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                 int epilogue, const void* residual, const void* norm_w, float eps, const uint8_t* const scale[3], void* scratch,
                 size_t scratch_bytes, mi_stream_t stream);

/* mi_qkv_rope_kvwrite (transformer_layers.py:66-70,165 + rope.py:13-23 + cache.py:83-92, T <= 8) with wq / wk / wv read as MXFP4
 * code bytes and sq / sk / sv their e8m0 block scales. */
int mi_qkv_rope_kvwrite_w4(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                           const void* wv, const uint8_t* sq, const uint8_t* sk, const uint8_t* sv, int n_heads, int n_kv_heads,
                           int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                           const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k, void* cache_v, int W, int kv_layout,
                           mi_stream_t stream);

/* Block scales of the seven linears of one layer (transformer_layers.py:51-54,101-103): DEVICE bytes [rows, K / 32], row-major. */
typedef struct mi_w4_layer {
  const uint8_t *wq, *wk, *wv, *wo, *w1, *w2, *w3;
} mi_w4_layer_t;
/* The quantisation of a model's layers: beside an mi_model_t whose seven linear pointers per layer then point to MXFP4 code bytes. */
typedef struct mi_w4_model {
  int32_t format;               /* MI_W4_MXFP4 */
  const mi_w4_layer_t* layers;  /* host array [n_layers] */
} mi_w4_model_t;

/* mi_workspace_bytes / mi_forward (Transformer.forward_partial, transformer.py:163-219, + the LM head, :229-242) on a model
 * whose linears are quantised as `w4` describes; w4 == NULL: exactly mi_workspace_bytes / mi_forward.  Launches, scratch and
 * refusals as mi_forward_w8: T <= 8 the six launches per layer on the MXFP4 GEMV kernels; T > 8 one dequantisation launch per linear
 * group into the scratch behind everything else in the workspace, then mi_forward's GEMM launch.  Always the launch path: the
 * persistent engine declines.  Dense models without un-merged LoRA only (num_experts > 0 or lora_rank > 0: MI_ERR_UNSUPPORTED,
 * naming MXFP4); dim, hidden_dim and n_heads * head_dim multiples of 32. */
size_t mi_workspace_bytes_w4(const mi_model_t* model, const mi_w4_model_t* w4, int T, int B, int max_cache_size);
int mi_forward_w4(const mi_model_t* model, const mi_w4_model_t* w4, const mi_batch_t* batch, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Speculative greedy decoding: one verify step scores up to 8 consecutive rows of a sequence.  Additive to ABI v9 like the blocks
 * above: no struct or entry point above changes, the presence of these symbols is the feature test.  The reference has no
 * speculative decoding; what a verify step emits is what generate.py:120-137 emits at temperature 0, token by token.
 *
 * Sequence b has p_b = kv_seqlens[b] cached positions and brings m_b rows (1 <= m_b <= 8, T = sum m_b <= 8): row 0 is its last
 * emitted token, not yet cached, rows 1 .. m_b - 1 are drafted tokens; row i sits at position p_b + i.  Per layer the step runs the
 * launches of a T-row prefill chunk (the T <= 8 GEMV kernels, same bits) except that NO row enters the rings: the post-RoPE K | V
 * rows go to a per-layer stash in the workspace, and the attention (mi_attn_verify) reads ring keys below p_b and the step's own
 * rows j <= i.  Behind the LM head: g_i = first argmax of row i, lp_i its log-softmax; a_b = the largest a with
 * ids[i] == g_(i-1) for all 1 <= i <= a; the emitted tokens of sequence b are g_0 .. g_(a_b).  The last launch of the call
 * commits: stash rows 0 .. a_b go to ring slots (p_b + i) % W_l of every layer, kv_seqlens[b] += a_b + 1, no other ring byte
 * changes - a rejected draft leaves no trace, also on a wrapped ring where its slot still holds a position that earlier rows see.
 * ---------------------------------------------------------------------------------------------- */

/* The attention of a verify step, a leaf like mi_attn_decode / mi_attn_prefill.  qkv: [T, ld] fused post-RoPE rows, sequence b's
 * are q_start[b] .. q_start[b + 1]; kv_before[b] = p_b.  Key position kp is visible to row i iff p_b + i - W < kp <= p_b + i;
 * kp < p_b is read from ring slot kp % W, kp >= p_b from the rows; the rings are not written.  Split geometry of the decode
 * attention (blocks of 128 slots of one kv head, streamed once for all rows and query heads); bf16 rings of either layout, W up
 * to 4096 (more, or MI_KV_E4M3: MI_ERR_UNSUPPORTED), T <= 8, B <= T.  scratch: mi_attn_verify_scratch_bytes, no initialisation.
 * out: [T, H*Dh]. */
size_t mi_attn_verify_scratch_bytes(int T, int n_heads, int head_dim, int W);
int mi_attn_verify(void* out, const void* qkv, int ld, const void* cache_k, const void* cache_v, int W, int T, int B, int n_heads,
                   int n_kv_heads, int head_dim, const int32_t* q_start, const int32_t* kv_before, void* scratch, int kv_layout,
                   mi_stream_t stream);

typedef struct mi_verify_out {
  int64_t* tokens;    /* dev [T]  g_i of every row; the first n_accept[b] + 1 of sequence b's rows are its emitted tokens */
  float* logprobs;    /* dev [T]  lp_i */
  int32_t* n_accept;  /* dev [B]  a_b */
} mi_verify_out_t;

/* Workspace of mi_forward_verify: mi_workspace_bytes_kv(model, quantised, T, T, max_cache_size, kv_layout) - the split partials
 * of the attention are per row, so T stands where the batch size stands - plus exactly the stash,
 * n_layers * T * 2 * n_kv_heads * head_dim bf16, behind everything else.  0 for T > 8 or a layout with MI_KV_E4M3. */
size_t mi_workspace_bytes_verify(const mi_model_t* model, int quantised, int T, int max_cache_size, int kv_layout);

/* One verify step on `model` - with w8 or w4 (at most one; both NULL: a bf16 model) as mi_forward_w8 / mi_forward_w4.  batch: the
 * PREFILL branch with a cache - q_start, kv_before, tok_seq, tok_pos written by the host, kv_before[b] == kv_seqlens[b],
 * tok_pos = kv_before[tok_seq[t]] + (t - q_start[tok_seq[t]]) - input_ids, logits [T, vocab] (all T rows are written) and a
 * workspace of mi_workspace_bytes_verify; greedy_token NULL.  Refused before any launch: lora_rank > 0 and MI_KV_E4M3 rings
 * (MI_ERR_UNSUPPORTED), T > 8 (MI_ERR_UNSUPPORTED), B > T or a max_q_len that leaves some sequence without a row, no cache or
 * kv_seqlens, no input_ids / logits (MI_ERR_ARG), a ring above 4096 slots (MI_ERR_UNSUPPORTED), and whatever mi_forward_w8 / _w4
 * refuse of a quantised model.  Always the launch path. */
int mi_forward_verify(const mi_model_t* model, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_batch_t* batch,
                      const mi_verify_out_t* out, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sampled verify steps: speculative decoding at temperature > 0.  Additive like the block above: one new symbol whose presence is
 * the feature test, no struct changes.  THE RULE (this is its definition; DESIGN.md section 0 restates it):
 *
 * Drafts are deterministic, so the proposal for a position is a point mass on the drafted token.  One sequence brings rows
 * 0 .. m-1: row 0 its last emitted token, rows 1 .. m-1 the drafts d_1 .. d_(m-1).  P_i is exactly the distribution mi_sample_top_p
 * draws from on row i's logits: softmax(logits / temperature); kept set = the prefix of the descending order whose mass BEFORE the
 * token is <= top_p, ties by ascending token id; renormalised; 40-bit fixed-point masses.  M_i is the kept mass, mass_i(d) the mass
 * of d if d is kept and 0 otherwise - also for a token tied at the cut value that the ascending-id rule leaves out.
 *   - for i = 0 .. m-2 in order: d_(i+1) is ACCEPTED iff u_acc[i] * M_i < mass_i(d_(i+1)); then token[i] = d_(i+1), the scan goes on;
 *   - at the first rejection token[i] is drawn by inverse CDF with u_draw[i] from P_i with d_(i+1) removed and renormalised (same
 *     order, same tie rule; the removed token's mass leaves the running sums), n_accept = i, and later rows emit nothing
 *     (token -1, logprob 0);
 *   - if every draft is accepted (n_accept = m-1, also m = 1), token[m-1] is the plain mi_sample_top_p draw from P_(m-1) with
 *     u_draw[m-1];
 *   - logprob[i] = log_softmax(UNSCALED logits_i)[token[i]] (generate.py:134-136), as mi_sample_top_p reports it;
 *   - a sole-survivor nucleus has mass(d) == M and is always accepted (u < 1): the residual is never empty when drawn from.
 * Accepting has probability P_i(d) and a rejection draws from P_i without d, so each emitted token is distributed as P_i: the
 * generation has the plain sampler's distribution - not its tokens for a given seed.
 * Variates: (w0, w1, w2, w3) = Philox4x32-10(seed; counter = offset, row t), t = the row's index in the step;
 * u_draw = (w0 * 2^32 + w1) / 2^64 - the words mi_sample_top_p uses - and u_acc = (w2 * 2^32 + w3) / 2^64.
 *
 * mi_verify_sample applies the rule to T rows of fp32 logits [T, ld] in B sequences (rows q_start[b] .. q_start[b + 1], q_start
 * device int32 [B + 1] with q_start[B] == T; ids device int64 [T]: the step's input ids, ids[t + 1] is row t's draft).  T is not
 * limited to 8 here.  uniforms: device fp32 [T][2] = (u_acc, u_draw) per row in place of the Philox words, or NULL.  An id
 * outside [0, vocab) has mass 0 (it is rejected; nothing is read for it).  Two launches, no scratch.  MI_ERR_ARG: a NULL
 * pointer but uniforms, B > T, temperature <= 0, top_p outside [0, 1].
 * mi_forward_verify with batch->sample_temperature > 0 runs it behind the LM head in place of argmax + acceptance, with
 * sample_top_p (checked as mi_forward checks it), sample_seed and counter = sample_offset (the host passes the index of the verify
 * step within the generation); the commit is unchanged.  sample_temperature == 0 is launch for launch the greedy step. */
int mi_verify_sample(const float* logits, int ld, int T, int B, int vocab, const int64_t* ids, const int32_t* q_start,
                     float temperature, float top_p, uint64_t seed, uint64_t offset, const float* uniforms, int64_t* tokens,
                     float* logprobs, int32_t* n_accept, mi_stream_t stream);

/* ABI v6 - storage dtypes other than bf16 (reference transformer.py:303,338: `from_folder(dtype=...)` keeps the dtype the
 * caller asks for; the reference's own tests build fp32 models, tests/test_generate.py:51,100) and bf16 models of a shape
 * mi_forward declines with MI_ERR_SHAPE (head_dim != 128, more than 16 experts, top_k = 3).  Same structs, same metadata
 * protocol, same sample epilogue; every weight / activation / cache pointer is to `dtype` elements, `logits` stays fp32.
 * Rounding points are the reference's in that dtype (csrc/generic.hip); with MI_DTYPE_FP32 nothing is rounded.  Launch by
 * launch (capturable in a hipGraph by the caller), not tuned to the roofline: BASELINE's configurations are bf16. */
enum mi_dtype { MI_DTYPE_BF16 = 0, MI_DTYPE_FP16 = 1, MI_DTYPE_FP32 = 2 };
/* Workspace of mi_forward (quantised == 0) or of mi_forward_w8 / _w4 (quantised != 0) for rings of layout code `kv_layout`.  Without
 * MI_KV_E4M3 exactly mi_workspace_bytes / mi_workspace_bytes_w8 / _w4.  With it, larger by the prefill scratch of one layer's
 * dequantised rings - 2 * B * n_kv_heads * max_cache_size * head_dim bf16 elements, rounded up to 256 bytes, behind everything else
 * - which a forward with MI_KV_E4M3 in mi_batch_t.kv_layout requires.  Such a forward runs, per layer: decode steps of T <= 8 the
 * q|k|v GEMV without its ring write, mi_kv_write's e4m3 kernel and the decode attention on bytes (one launch more than on bf16
 * rings); T > 8 the existing ring write call site; prefill with a cache one dequantisation of the layer's rings into the scratch,
 * the bf16 prefill attention on the scratch, then the e4m3 ring write.  The chunk's own rows are read from the activations,
 * unrounded; a decode step's own row goes through the ring, rounded (transformer_layers.py:72-81).  The persistent engine declines. */
size_t mi_workspace_bytes_kv(const mi_model_t* model, int quantised, int T, int B, int max_cache_size, int kv_layout);

/* ------------------------------------------------------------------------------------------------
 * FP8 prefill GEMMs (W8A8) for models whose weights are MI_W8_FP8_E4M3: opt-in, additive to ABI v9 like the blocks above (the
 * presence of these symbols is the feature test; nothing above changes meaning).  A linear group of M >= 256 rows and K % 128 == 0
 * quantises its bf16 input rows per row (per token) to e4m3 and contracts bytes with bytes on the block-scaled FP8 MFMA
 * (csrc/gemm256_w8a8.hip):
 *     s_x[m] = 2^ceil(log2(amax_k |x[m, k]| / 448))  (an all-zero row: 1),   x_q[m, k] = e4m3_rne(clamp(x[m, k] / s_x[m], +-448)),
 *     y[m, n] = (sum_k e4m3(x_q[m, k]) * e4m3(w[n, k])) * (s_x[m] * scale[n])   in fp32,
 * and y enters the epilogues exactly where the fp32 accumulator of mi_linear's GEMM enters them (same rounding points).  There is
 * no dequantisation launch and no bf16 image of the weights.  Activations keep three mantissa bits: on inputs that e4m3 holds
 * exactly under the row's power-of-two scale the route is lossless, on anything else it is NOT the weight-only model, and no claim
 * about model quality is made.  Anything else - M < 256, K % 128 != 0, K > 16384 (the quantiser holds a row in registers), a row
 * stride of x that is no multiple of 8, x or a weight matrix not 16-byte aligned - is not an error: it takes mi_linear_w8's routes,
 * bit for bit.
 * ---------------------------------------------------------------------------------------------- */
/* xq [M, K] e4m3 bytes and sx [M] fp32 from bf16 rows x [M, K] (row stride ldx elements) by the rule above - the rule of
 * mistral_inference.quant.quantize_rows, the same bytes as the CPU gives; never a NaN code; a code whose dequantised value would
 * pass the largest bf16 steps down.  norm_w != NULL: the rows quantised are bf16(mi_rmsnorm(x, norm_w, eps)), i.e. what mi_rmsnorm
 * writes.  K and ldx multiples of 8, K <= 16384 (MI_ERR_SHAPE). */
int mi_act_quant_e4m3(void* xq, float* sx, const void* x, int ldx, int M, int K, const void* norm_w, float eps, mi_stream_t stream);
/* mi_linear_w8 with the W8A8 route where it applies (M >= 256 && K % 128 == 0 && K <= 16384, operands as above): `scratch` then holds
 * x_q | s_x, and norm_w is taken where the route is (fused into the quantisation).  Outside that shape it IS mi_linear_w8, scratch size
 * included; inside it mi_linear_w8a8_scratch_bytes is the larger of the two routes' needs (x_q | s_x, or mi_linear_w8's bf16 image),
 * since operands that the 16-byte accesses cannot read still take mi_linear_w8's route.  MI_EPI_LOGITS: MI_ERR_UNSUPPORTED, as there. */
size_t mi_linear_w8a8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue);
int mi_linear_w8a8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const float* const scale[3], void* scratch,
                   size_t scratch_bytes, mi_stream_t stream);
/* The q|k|v group of a prefill as mi_forward_w8a8 runs it, as a leaf: qkv[T, ldo] = rope(bf16((x_q . [wq; wk; wv]^T) * s_x * s_w))
 * with RoPE in the GEMM's epilogue on the q | k columns (rope.py:13-23 on the bf16-rounded projection, as mi_rope_inplace) and no
 * ring write.  The route's shape and operands only (T >= 256, D % 128 == 0, D <= 16384, ldx % 8 == 0, x and the weights 16-byte
 * aligned; MI_ERR_UNSUPPORTED otherwise: fewer rows are mi_qkv_rope_kvwrite_w8's); head_dim 128; scratch of
 * mi_linear_w8a8_scratch_bytes(T, D, ...) bytes. */
int mi_qkv_rope_w8a8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                     const float* sq, const float* sk, const float* sv, int n_heads, int n_kv_heads, int head_dim, const void* norm_w,
                     float eps, const float* rope_cs, int rope_len, const int32_t* tok_pos, void* scratch, size_t scratch_bytes,
                     mi_stream_t stream);
/* mi_workspace_bytes_kv(model, 1, ...) / mi_forward_w8 with the W8A8 route in the four linear groups of every layer (q|k|v and
 * w1|w3 with the RMSNorm fused into the quantisation, q|k|v with RoPE in the GEMM's epilogue).  The workspace is larger by
 * x_q (T * max(dim, n_heads * head_dim, hidden_dim) bytes) and s_x (T floats), each rounded up to 256 bytes, behind everything else.
 * A group outside the route (hidden_dim > 16384: w2) runs as in mi_forward_w8.
 * Same refusals as mi_forward_w8 (w8 == NULL: MI_ERR_ARG).  Every forward of T < 256 rows - decode steps, short chunks - is launch
 * for launch mi_forward_w8; rings of e4m3 bytes (MI_KV_E4M3) are independent of it. */
size_t mi_workspace_bytes_w8a8(const mi_model_t* model, const mi_w8_model_t* w8, int T, int B, int max_cache_size, int kv_layout);
int mi_forward_w8a8(const mi_model_t* model, const mi_w8_model_t* w8, const mi_batch_t* batch, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MXFP4 x FP8 prefill GEMMs (W4A8) for models whose weights are MI_W4_MXFP4: opt-in, additive to ABI v9 like the block above.  A
 * linear group of M >= 256 rows and K % 128 == 0 quantises its bf16 input rows per row (per token) to e4m3 - mi_act_quant_e4m3,
 * the rule above - and contracts them with the e2m1 codes on the mixed form of the block-scaled MFMA, which applies the e8m0 block
 * scale bytes itself (csrc/gemm256_w4a8.hip):
 *     y[m, n] = (sum_k e4m3(x_q[m, k]) * e2m1(c[n, k]) * 2^(s[n, k / 32] - 127)) * s_x[m]   in fp32,
 * and y enters the epilogues exactly where the fp32 accumulator of mi_linear's GEMM enters them (same rounding points).  There is
 * no dequantisation launch and no bf16 image of the weights.  On inputs that e4m3 holds exactly under the row's power-of-two scale
 * the route is the weight-only route up to fp32 summation order (lossless); on anything else it is NOT the weight-only model, and
 * no claim about model quality is made.  For block scale bytes below 3 (weights under 2^-124) the weight-only route's bf16 image
 * holds subnormals, which it may flush and this route does not.  Anything else - M < 256, K % 128 != 0, K > 16384, a row stride of
 * x that is no multiple of 8, x or a code matrix not 16-byte aligned, a block scale matrix not 4-byte aligned (the GEMM stages the
 * scale bytes of a K tile by 4-byte DMA) - is not an error: it takes mi_linear_w4's routes, bit for bit.
 * ---------------------------------------------------------------------------------------------- */
/* mi_linear_w4 with the W4A8 route where it applies: `scratch` then holds x_q | s_x, and norm_w is taken where the route is (fused
 * into the quantisation).  Outside the route's shape it IS mi_linear_w4, scratch size included; inside it
 * mi_linear_w4a8_scratch_bytes is the larger of the two routes' needs (x_q | s_x, or mi_linear_w4's bf16 image).  MI_EPI_LOGITS:
 * MI_ERR_UNSUPPORTED, as there. */
size_t mi_linear_w4a8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue);
int mi_linear_w4a8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const uint8_t* const scale[3], void* scratch,
                   size_t scratch_bytes, mi_stream_t stream);
/* mi_qkv_rope_w8a8 on MXFP4 code matrices and their block scale bytes: the q|k|v group of a prefill as mi_forward_w4a8 runs it,
 * RoPE in the GEMM's epilogue, no ring write.  The route's shape and operands only, the 4-byte alignment of sq / sk / sv included
 * (MI_ERR_UNSUPPORTED otherwise: fewer rows are mi_qkv_rope_kvwrite_w4's); head_dim 128; scratch of mi_linear_w4a8_scratch_bytes(T, D, ...) bytes. */
int mi_qkv_rope_w4a8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                     const uint8_t* sq, const uint8_t* sk, const uint8_t* sv, int n_heads, int n_kv_heads, int head_dim,
                     const void* norm_w, float eps, const float* rope_cs, int rope_len, const int32_t* tok_pos, void* scratch,
                     size_t scratch_bytes, mi_stream_t stream);
/* mi_workspace_bytes_kv(model, 1, ...) / mi_forward_w4 with the W4A8 route in the four linear groups of every layer (q|k|v and
 * w1|w3 with the RMSNorm fused into the quantisation, q|k|v with RoPE in the GEMM's epilogue).  The workspace is larger by
 * x_q (T * max(dim, n_heads * head_dim, hidden_dim) bytes) and s_x (T floats), each rounded up to 256 bytes, behind everything else.
 * A group outside the route (hidden_dim > 16384: w2) runs as in mi_forward_w4.  Same refusals as mi_forward_w4 (w4 == NULL:
 * MI_ERR_ARG).  Every forward of T < 256 rows - decode steps, short chunks - is launch for launch mi_forward_w4. */
size_t mi_workspace_bytes_w4a8(const mi_model_t* model, const mi_w4_model_t* w4, int T, int B, int max_cache_size, int kv_layout);
int mi_forward_w4a8(const mi_model_t* model, const mi_w4_model_t* w4, const mi_batch_t* batch, mi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A quantised LM head for MI_W8_FP8_E4M3 and MI_W4_MXFP4 models: opt-in, additive to ABI v9 like the blocks above (the presence of
 * these symbols is the feature test; no struct or entry point above changes - mi_linear_w8 / _w4 keep answering MI_EPI_LOGITS with
 * MI_ERR_UNSUPPORTED).  The head (transformer.py:235, `output`) is then stored in the format of the model's layers: w [vocab, K]
 * e4m3 bytes with fp32 row scales [vocab], or MXFP4 code bytes [vocab, K / 2] with e8m0 block scales [vocab, K / 32]; K = dim.
 *   M <= 8:  the weight-streaming GEMV of the format with the bf16 head's epilogue (csrc/gemv_w8.hip, gemv_w4.hip; the final
 *            RMSNorm fused as there): logit = float(bf16(acc * scale[r])) for FP8, float(bf16(acc)) for MXFP4 - one bf16 rounding
 *            of the fp32 value, then widened, exactly where the bf16 head rounds;
 *   M  > 8:  the bf16 image of the head (as mi_linear_w8 / _w4 define it) is written into a scratch in slices of
 *            MI_LM_HEAD_SLICE_ROWS vocabulary rows - one dequantisation launch and the GEMM launch(es) of mi_linear /
 *            mi_lm_head_logprobs per slice - so the scratch is min(vocab, MI_LM_HEAD_SLICE_ROWS) * K bf16 (84 MB at K = 5120),
 *            rounded up to 256 bytes, whatever the vocabulary.  Every column runs on the GEMM kernel that one launch on the whole
 *            image gives it: logits and log-probabilities are those of mi_linear(MI_EPI_LOGITS) / mi_lm_head_logprobs on the
 *            dequantised head, bit for bit.
 * Nothing is claimed about model quality (MXFP4's relative rms weight error is 0.12).  The embedding table stays bf16.
 * ---------------------------------------------------------------------------------------------- */
#define MI_LM_HEAD_SLICE_ROWS 8192

/* The quantisation of the LM head: beside an mi_model_t whose `output` then points to the quantised bytes. */
typedef struct mi_lm_head_quant {
  int32_t format;     /* MI_W8_FP8_E4M3 / MI_W4_MXFP4: the format of the model's layers */
  const void* scale;  /* DEVICE: fp32 [vocab] (FP8) or e8m0 bytes [vocab, dim / 32], row-major (MXFP4) */
} mi_lm_head_quant_t;

/* The head as a leaf: logits[M, ldo] (fp32) = bf16-rounded (rmsnorm(x) or x)[M, K] @ W^T, W as `head` describes `w`.  M > 8 needs
 * `scratch` of mi_lm_head_q_scratch_bytes(M, K, vocab) bytes (0 for M <= 8, where scratch may be NULL); norm_w as mi_linear (M <= 8
 * only).  K a multiple of 16 (FP8) / 32 (MXFP4): MI_ERR_SHAPE; another format value: MI_ERR_UNSUPPORTED. */
size_t mi_lm_head_q_scratch_bytes(int M, int K, int vocab);
int mi_lm_head_q(float* logits, int ldo, const void* x, int ldx, int M, int K, const void* w, int vocab, const mi_lm_head_quant_t* head,
                 const void* norm_w, float eps, void* scratch, size_t scratch_bytes, mi_stream_t stream);
/* mi_lm_head_logprobs on a quantised head.  scratch: mi_lm_head_logprobs_scratch_bytes(M, vocab) rounded up to 256 bytes, and for
 * M > 8 the slice of mi_lm_head_q_scratch_bytes behind it.  The fused route reduces over the whole vocabulary: the slices write
 * the per-tile partials of the one launch, so the result does not depend on the slicing. */
size_t mi_lm_head_logprobs_q_scratch_bytes(int M, int K, int vocab);
int mi_lm_head_logprobs_q(float* logprob, const void* x, int ldx, int M, int K, const void* w, int vocab, const mi_lm_head_quant_t* head,
                          const int32_t* target, void* scratch, size_t scratch_bytes, mi_stream_t stream);

/* ONE forward entry for a model with a quantised head.  It covers mi_forward (w8 == w4 == NULL), mi_forward_w8 / _w4 (one of them),
 * mi_forward_w8a8 / _w4a8 (a8 != 0) and mi_forward_verify (verify_out != NULL); with head == NULL it is, launch for launch, those
 * entries, error codes included.  head != NULL: the LM head launch reads model->output as quantised bytes with head->scale; at T <= 8
 * (decode steps, verify steps, short chunks) the format's GEMV, above the sliced route - the a8 routes leave the head on it, as they
 * leave the bf16 head alone.  Refused before any launch: a head format that is not the layers' (MI_ERR_UNSUPPORTED), a head on a
 * model without quantised layers (MI_ERR_UNSUPPORTED), a NULL scale (MI_ERR_ARG), and whatever those entries refuse - dim not a
 * multiple of 16 / 32 among it.
 * Workspace: mi_workspace_bytes_q with the same w8 / w4 / head / a8 and verify = (verify_out != NULL).  With head == NULL it is
 * mi_workspace_bytes_kv / _w8a8 / _w4a8 / _verify (verify: B is not read, T stands for it); with a head and T > 8 it is larger by
 * exactly the slice, min(vocab, MI_LM_HEAD_SLICE_ROWS) * dim * 2 bytes rounded up to 256, behind everything else. */
size_t mi_workspace_bytes_q(const mi_model_t* model, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_lm_head_quant_t* head,
                            int T, int B, int max_cache_size, int kv_layout, int a8, int verify);
int mi_forward_q(const mi_model_t* model, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_lm_head_quant_t* head,
                 const mi_batch_t* batch, const mi_verify_out_t* verify_out, int a8, mi_stream_t stream);

size_t mi_workspace_bytes_generic(const mi_model_t* model, int T, int dtype);
int mi_forward_generic(const mi_model_t* model, const mi_batch_t* batch, int dtype, mi_stream_t stream);
/* Leaf operators in any storage dtype - what module-level callers of an fp16 / fp32 model bind (the Pixtral tower of
 * vision_encoder.py:76-204, RMSNorm / FeedForward used stand-alone); argument meaning as the bf16 entry points above.
 * mi_linear_generic: one launch per weight matrix, epilogues STORE / RESIDUAL / LOGITS (SwiGLU = two calls +
 * mi_swiglu_generic: a <- silu(a) * b).  mi_attention_nocache_generic: the cache=None attention, every token sees every
 * token (transformer_layers.py:72-73,165), any head_dim <= 256, softmax_scale <= 0 = head_dim^-1/2. */
int mi_embedding_generic(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, int dtype, mi_stream_t stream);
int mi_rmsnorm_generic(void* out, const void* x, const void* w, int T, int D, float eps, int dtype, mi_stream_t stream);
int mi_linear_generic(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                      int epilogue, const void* residual, int dtype, mi_stream_t stream);
int mi_rope_inplace_generic(void* qkv, int ld, int T, int n_rot_cols, int head_dim, const float* rope_cs, const int32_t* tok_pos,
                            int dtype, mi_stream_t stream);
int mi_attention_nocache_generic(void* out, const void* qkv, int ld, int T, int n_heads, int n_kv_heads, int head_dim,
                                 float softmax_scale, int dtype, mi_stream_t stream);
int mi_swiglu_generic(void* a, const void* b, int T, int F, int dtype, mi_stream_t stream);
int mi_gelu_generic(void* x, int ldx, int T, int N, int dtype, mi_stream_t stream);

/* Persistent decode engine (csrc/decode_engine.hip).  A DECODE-branch mi_forward with T == B == 1 on a dense model runs
 * all local layers - TransformerBlock.forward (transformer_layers.py:158-169) x n_layers, the ring write (cache.py:83-92)
 * and the LM head (transformer.py:235) - as ONE persistent launch when the shapes allow it (dim, hidden_dim and
 * n_heads*128 multiples of 512, dim <= 8192, at most one attention work item per CU); bit-identical to the launch path.
 * mi_set_decode_engine(0) forces the launch path (A/B measurements, tests); returns the previous setting.  Initial value:
 * environment MI_DECODE_ENGINE (default 1). */
int mi_set_decode_engine(int enabled);
/* Residency.  The engine's workgroups wait for each other, so all of them (one per CU) must be resident at once; a plain
 * launch checks nothing.  Two guards: (1) before its first use on a device the library runs a census kernel with the
 * engine's launch shape (one stream synchronisation, outside any capture): if the workgroups do not all meet - a CU mask, a
 * partition mode, a co-tenant - the engine is not used on that device and mi_forward takes the launch path;
 * mi_decode_engine_census(1) forgets the verdicts (tests, or after the device's situation changed).  (2) Every engine
 * launch repeats the census on itself before its first side effect; if it fails, the launch ends having written NOTHING
 * (no ring row, no position advance, no sample), raises status word 1 = 0x700, and every later engine launch on that
 * workspace leaves at once until the caller has run mi_decode_engine_reset - the device state stays exactly that of the
 * first failed step, which the caller can therefore re-run on the launch path (mi_set_decode_engine(0)); the number of
 * steps that did complete is status word 5.  Timeouts AFTER the census (codes 0x100-0x600) should not exist; they poison
 * the workspace the same way but may leave a half-written step. */
int mi_decode_engine_census(int forget);
int mi_decode_engine_reset(void* workspace, mi_stream_t stream);
/* Copies the engine's control words out of a workspace and synchronises `stream` (a health check, NOT part of the hot
 * path): status[0] = step epoch, status[1] = 0 or the code of the first bounded wait that ever timed out
 * (0x100 loader / 0x200 ring / 0x300 consumer barrier / 0x400 hand-off sweep / 0x500-0x600 holder waves / 0x700 residency
 * census of a step: nothing was written), status[2] = abort flag of the last step,
 * status[3] = 0 or 1 + the index of a token whose id was outside [0, vocab) in some mi_forward call (sticky until the
 * caller zeroes the word: the host raises the reference's IndexError from it), status[4] = launches completed by the
 * engine since the workspace was zeroed (one per <= 32 layers of a decode step; unchanged when the launch path ran),
 * status[5] = decode steps run on this workspace (engine: completed; launch path: started) = next row of the greedy
 * history ring, status[6] = workgroup arrivals of the current engine step, status[7] reserved. */
int mi_decode_engine_status(const void* workspace, mi_stream_t stream, uint32_t status[8]);
/* Engine diagnostics (timeline trace, loader knobs, residency-gate test hook) are NOT part of the product boundary:
 * include/mistral_hip_debug.h. */

/* ------------------------------------------------------------------------------------------------
 * Pipeline-parallel exchange steps over RCCL (xGMI between the GPUs of a node)
 *
 * Replaces the reference's torch.distributed calls on the hot path: recv of the previous stage's activations
 * (transformer.py:196), send to the next stage (:214), logits broadcast from the last stage (:237); process-group
 * set-up of main.py:110-118.  One communicator per process (one process per GPU).  Every transfer is enqueued on the
 * caller's HIP stream - no host synchronisation, and capturable in a hipGraph with the decode step.  librccl is
 * dlopen()ed at the first call (MI_RCCL_LIB overrides the name): MI_ERR_UNSUPPORTED when it is absent.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mi_rccl_comm* mi_rccl_t;
#define MI_RCCL_ID_BYTES 128
/* rank 0 creates the 128-byte rendezvous id; the host distributes it to the other ranks (any side channel:
 * torch.distributed object broadcast, a file, MPI) before each rank calls mi_rccl_init with the same id. */
int mi_rccl_unique_id(void* id128);
int mi_rccl_init(mi_rccl_t* comm, int world_size, int rank, const void* id128);
int mi_rccl_destroy(mi_rccl_t comm);
/* point-to-point: `bytes` from/to device memory, matched by the peer's recv/send on ITS stream */
int mi_rccl_send(mi_rccl_t comm, const void* buf, size_t bytes, int peer, mi_stream_t stream);
int mi_rccl_recv(mi_rccl_t comm, void* buf, size_t bytes, int peer, mi_stream_t stream);
/* in-place broadcast of `bytes` from `root` */
int mi_rccl_bcast(mi_rccl_t comm, void* buf, size_t bytes, int root, mi_stream_t stream);
/* ncclGroupStart / ncclGroupEnd: a send and a recv that must progress together (a rank exchanging with itself or with
 * both neighbours at once) are issued between the two */
int mi_rccl_group_start(void);
int mi_rccl_group_end(void);
const char* mi_rccl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MISTRAL_HIP_H */
