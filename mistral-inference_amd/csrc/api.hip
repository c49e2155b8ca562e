// C-ABI entry points of libmistral_hip.so (include/mistral_hip.h) and the layer-stack runner.
//
// mi_forward sequences, for every local layer, the launches that replace TransformerBlock.forward
// (reference transformer_layers.py:158-169) and, around the stack, Transformer.forward_partial /
// forward (transformer.py:163-242).  Per decode token and dense layer that is 6 launches:
//   [RMSNorm + Wq|Wk|Wv GEMV + RoPE + ring write] [split-KV GQA attention] [split combine] [Wo GEMV + residual]
//   [RMSNorm + W1|W3 GEMV + SiLU*mul] [W2 GEMV + residual]
// (rings of e4m3 bytes, MI_KV_E4M3: the GEMV without its ring write + the e4m3 ring write = 7 launches, and at prefill one
// dequantisation of the layer's rings into a scratch in front of the attention)
// with no host synchronisation and no per-step host metadata (positions come from the device-resident
// kv_seqlens), so a decode step can also be captured in a hipGraph by the caller.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/mistral_hip.h"
#include "../../include/mistral_hip_debug.h"
#include "kernels.h"

namespace {

thread_local char g_detail[512] = "";

// a layout code: MI_KV_SLOT_MAJOR / MI_KV_HEAD_MAJOR, alone or with MI_KV_E4M3 (rings of e4m3 bytes)
bool kv_layout_ok(int layout) { return (layout & ~MI_KV_E4M3) == MI_KV_SLOT_MAJOR || (layout & ~MI_KV_E4M3) == MI_KV_HEAD_MAJOR; }
bool kv_e4m3(int layout) { return (layout & MI_KV_E4M3) != 0; }
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_detail, sizeof(g_detail), fmt, ap);
  va_end(ap);
  return code;
}

inline int hip_rc(hipError_t e, const char* what) {
  if (e == hipSuccess) return MI_OK;
  snprintf(g_detail, sizeof(g_detail), "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

#define MI_TRY(expr)          \
  do {                        \
    int _rc = (expr);         \
    if (_rc != MI_OK) return _rc; \
  } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

constexpr size_t TICKET_BYTES = 4096;  // first words: control block of the persistent decode engine (epoch, status, abort)

// 1 (default): batch-1 decode steps of dense models run on the persistent engine (decode_engine.hip) when the shapes
// allow it; 0: always the launch path.  MI_DECODE_ENGINE sets the initial value, mi_set_decode_engine changes it.
int g_engine_mode = -1;
int engine_mode() {
  if (g_engine_mode < 0) {
    const char* e = getenv("MI_DECODE_ENGINE");
    g_engine_mode = e ? (atoi(e) != 0) : 1;
  }
  return g_engine_mode;
}

// MI_FUSE_ROPE=0: RoPE as a separate pass after the prefill q|k|v GEMM instead of in its epilogue (A/B testing)
bool fuse_rope_enabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("MI_FUSE_ROPE");
    v = e ? (atoi(e) != 0) : 1;
  }
  return v != 0;
}

struct Workspace {
  int32_t* tickets;
  bf16_t* xn;       // [T, D]
  bf16_t* qkv;      // [T, (H + 2 Hkv) Dh]
  bf16_t* attn;     // [T, H Dh]
  bf16_t* hid;      // [T * max(1, top_k), F]
  float* partial;   // decode attention partials
  int32_t* sel_idx; // MoE: router picks [T, top_k]
  float* sel_w;
  int32_t* tok_of;   // token of compact row r            [T * top_k]
  int32_t* row_of;   // compact row of (token, slot)      [T * top_k]
  int32_t* tile_tab; // grouped-GEMM m-tile table         [max_tiles][4]
  int32_t* n_tiles;
  bf16_t* moe_y;     // expert outputs, compact rows      [T * top_k, D]
  void* gran;        // decode-engine granule regions (dense models)
  size_t gran_bytes;
  int max_tiles;
  bf16_t* lora_t;    // un-merged LoRA (lora_rank > 0 only, behind everything else): t = bf16(A x)   [T, 3 * rank]
  void* lora_base;   // ... and the base products of q|k|v and w1|w3  [T, max(qkv cols, 2 F)]: fp32 holding bf16 values for T <= 8
  bf16_t* deq;       // quantised models at T > 8 (behind everything else, such models only): the dequantised weights of one linear
  bf16_t* kv_deq;    // e4m3 K/V rings (behind everything else, such forwards only): one layer's rings of the batch as bf16, K then V,
                     //     for the prefill attention (kv_scratch_elems).  (deq: deq_scratch_elems.  lora_base: the GEMV's LOGITS form, see
                     //     linear_group; bf16 above 8 rows.  Wo's and W2's base product goes to xn.)
  bf16_t* stash;     // verify steps (behind everything else, such steps only): the step's post-RoPE K | V rows of every layer
                     //     [n_layers, T, 2 * n_kv_heads * head_dim], which enter the rings once acceptance is known
  uint8_t* x_q;      // FP8 prefill GEMMs (mi_forward_w8a8 / mi_forward_w4a8 only, behind everything else): the e4m3 rows of a linear group's input
  float* s_x;        //     [T, max(dim, n_heads * head_dim, hidden_dim)] and their scales [T]
  bf16_t* head_deq;  // a quantised LM head at T > 8 (mi_forward_q with a head struct only, behind everything else): one slice of
                     //     lm_head_slice_rows(vocab) dequantised vocabulary rows
  size_t total;
};

// A quantised LM head at more than 8 rows is dequantised and multiplied in slices of this many vocabulary rows (the last one
// shorter), so that its bf16 image never exists as a whole: 1.34 GB at vocab 131072 x dim 5120, against 84 MB for a slice.  8192
// rows are 32 column tiles of the 256-tile GEMM: from 2048 prompt rows on, a slice still fills the 256 CUs, and a slice's
// dequantisation moves tens of megabytes, far above the cost of a launch.  A multiple of 256, so that every slice starts on a tile
// boundary of either GEMM kernel and of the fused log-prob partials.
constexpr int LM_HEAD_SLICE_ROWS = MI_LM_HEAD_SLICE_ROWS;
static_assert(LM_HEAD_SLICE_ROWS % 256 == 0, "slices start on tile boundaries");
inline size_t lm_head_slice_rows(int vocab) { return (size_t)(vocab < LM_HEAD_SLICE_ROWS ? vocab : LM_HEAD_SLICE_ROWS); }
inline size_t lm_head_slice_bytes(int vocab, int K) { return lm_head_slice_rows(vocab) * (size_t)K * sizeof(bf16_t); }

// bf16 elements of the largest linear group a prefill dequantises at once: q|k|v, wo, w1|w3, w2
size_t deq_scratch_elems(const mi_model_t* m) {
  const size_t D = m->dim, F = m->hidden_dim, nq = (size_t)m->n_heads * m->head_dim, nkv = (size_t)m->n_kv_heads * m->head_dim;
  const size_t a = (nq + 2 * nkv) * D, b = 2 * F * D;
  return a > b ? a : b;  // (wo: D * nq <= a; w2: D * F <= b)
}

// bf16 elements of ONE dequantised ring (K or V) of B sequences of a layer
size_t kv_scratch_elems(const mi_model_t* m, int B, int maxW) { return (size_t)B * m->n_kv_heads * maxW * m->head_dim; }

// bytes of a verify step's stash: K | V rows of T tokens in every layer (a multiple of 256 at head_dim 128)
size_t verify_stash_bytes(const mi_model_t* m, int T) { return (size_t)m->n_layers * T * 2 * m->n_kv_heads * m->head_dim * sizeof(bf16_t); }

// quant: the linears are quantised (any format: the same scratch of one dequantised linear group); kv8: the rings hold e4m3 bytes
// verify: a verify step (mi_forward_verify) - its attention keeps split partials per ROW, so the caller passes B = T, and the stash
// a8: the entry is mi_forward_w8a8 / mi_forward_w4a8 - the activation rows of its FP8-activation GEMMs
// qhead: the LM head is quantised (mi_forward_q) - the slice of its bf16 image at T > 8
Workspace carve(const mi_model_t* m, int T, int B, int maxW, char* base, bool quant = false, bool kv8 = false, bool verify = false,
                bool a8 = false, bool qhead = false) {
  Workspace w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  const int qkv_cols = (m->n_heads + 2 * m->n_kv_heads) * m->head_dim;
  const int slots = m->top_k > 0 ? m->top_k : 1;
  w.tickets = (int32_t*)take(TICKET_BYTES);
  // engine granules at a FIXED offset (independent of T): nothing else ever writes them, so a stale word can never
  // look like a valid {value, tag} granule
  w.gran_bytes = (m->n_kv_heads > 0 && m->n_heads % m->n_kv_heads == 0)
                     ? decode_engine_granule_bytes(m->dim, m->n_heads, m->n_kv_heads, m->hidden_dim, maxW) : 0;
  w.gran = take(w.gran_bytes);
  w.xn = (bf16_t*)take((size_t)T * m->dim * 2);
  w.qkv = (bf16_t*)take((size_t)T * qkv_cols * 2);
  w.attn = (bf16_t*)take((size_t)T * m->n_heads * m->head_dim * 2);
  w.hid = (bf16_t*)take((size_t)T * slots * m->hidden_dim * 2);
  size_t partial_floats = attn_decode_partial_floats(B, m->n_heads, m->n_kv_heads, m->head_dim, maxW);
  if (verify) {  // (the same figure while the decode attention's split geometry is its default one)
    const size_t v = attn_verify_partial_floats(T, m->n_heads, m->head_dim, maxW);
    partial_floats = v > partial_floats ? v : partial_floats;
  }
  w.partial = (float*)take(partial_floats * sizeof(float));
  w.sel_idx = (int32_t*)take((size_t)T * slots * 4);
  w.sel_w = (float*)take((size_t)T * slots * 4);
  w.max_tiles = (T * slots + 127) / 128 + (m->num_experts > 0 ? m->num_experts : 0);
  w.tok_of = (int32_t*)take((size_t)T * slots * 4);
  w.row_of = (int32_t*)take((size_t)T * slots * 4);
  w.tile_tab = (int32_t*)take((size_t)w.max_tiles * 16);
  w.n_tiles = (int32_t*)take(256);
  w.moe_y = (bf16_t*)take(m->num_experts > 0 ? (size_t)T * slots * m->dim * 2 : 0);
  w.lora_t = nullptr;
  w.lora_base = nullptr;
  if (m->lora_rank > 0) {  // (lora_rank == 0: the layout and the total are exactly those of ABI v7)
    const size_t wide = (size_t)(qkv_cols > 2 * m->hidden_dim ? qkv_cols : 2 * m->hidden_dim);
    w.lora_t = (bf16_t*)take((size_t)T * 3 * m->lora_rank * 2);
    w.lora_base = take((size_t)T * wide * (T <= GEMV_MAX_T ? 4 : 2));
  }
  w.deq = (quant && T > GEMV_MAX_T) ? (bf16_t*)take(deq_scratch_elems(m) * 2) : nullptr;  // (a plain model: layout and total as ever)
  w.kv_deq = kv8 ? (bf16_t*)take(2 * kv_scratch_elems(m, B, maxW) * 2) : nullptr;          // (bf16 rings: layout and total as ever)
  w.stash = verify ? (bf16_t*)take(verify_stash_bytes(m, T)) : nullptr;                      // (any other forward: layout and total as ever)
  w.x_q = nullptr;
  w.s_x = nullptr;
  if (a8) {  // (any other forward: layout and total as ever)
    const size_t nq = (size_t)m->n_heads * m->head_dim, k1 = (size_t)m->dim > nq ? (size_t)m->dim : nq;
    w.x_q = (uint8_t*)take((size_t)T * (k1 > (size_t)m->hidden_dim ? k1 : (size_t)m->hidden_dim));
    w.s_x = (float*)take((size_t)T * sizeof(float));
  }
  // (any other forward: layout and total as ever)
  w.head_deq = (qhead && T > GEMV_MAX_T) ? (bf16_t*)take(lm_head_slice_bytes(m->vocab_size, m->dim)) : nullptr;
  w.total = off;
  return w;
}

// ---- GemvArgs of the fused modes, one builder each, for mi_forward_generic's fp16 rows (every bf16 / quantised linear goes
// through linear_group below).  Pointers are to 2-byte elements of either compile of gemv.hip; T is set per pass below.
GemvArgs gemv_common(const void* x, int ldx, int K, int N, const void* norm_w, float eps, void* out, int ldo) {
  GemvArgs a;
  memset(&a, 0, sizeof(a));
  a.K = K; a.N = N; a.x = (const bf16_t*)x; a.ldx = ldx; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.out = out; a.ldo = ldo;
  return a;
}
struct RingWrite {  // the K/V ring of one layer, for the launch whose epilogue writes it
  void *k, *v;
  int W, layout;
};
// qkv[T, ldo] = rope(rmsnorm(x) @ [wq; wk; wv]^T); ring != nullptr: the k | v columns also go to slot tok_pos % W of tok_seq's ring.
// Without a ring the four ring fields stay 0: the kernel reads them only under write_kv (gemv_core.cuh), so there is no pos % 0.
GemvArgs gemv_qkv_rope(const void* x, int ldx, int D, const void* norm_w, float eps, const void* wq, const void* wk, const void* wv,
                       int nq, int nkv, void* qkv, int ldo, const float* rope_cs, const int32_t* tok_pos, const int32_t* tok_seq,
                       int head_dim, const RingWrite* ring) {
  GemvArgs a = gemv_common(x, ldx, D, nq + 2 * nkv, norm_w, eps, qkv, ldo);
  a.mode = GEMV_QKV_ROPE;
  a.w0 = (const bf16_t*)wq; a.w1 = (const bf16_t*)wk; a.w2 = (const bf16_t*)wv; a.n0 = nq; a.n1 = nq + nkv;
  a.rope_cs = rope_cs; a.tok_pos = tok_pos; a.tok_seq = tok_seq; a.head_dim = head_dim;
  if (ring) { a.write_kv = 1; a.cache_k = ring->k; a.cache_v = ring->v; a.W = ring->W; a.kv_layout = ring->layout; }
  return a;
}
// h[T, D] += x[T, K] @ w^T   (Wo, W2)
GemvArgs gemv_residual(const void* x, int K, const void* w, void* h, int D) {
  GemvArgs a = gemv_common(x, K, K, D, nullptr, 0.f, h, D);
  a.mode = GEMV_RESIDUAL;
  a.w0 = (const bf16_t*)w; a.n0 = a.n1 = D; a.residual = (const bf16_t*)h;
  return a;
}
// hid[T, F] = silu(xn @ w1^T) * (xn @ w3^T), xn = rmsnorm(h[T, D])
GemvArgs gemv_swiglu(const void* h, int D, const void* norm_w, float eps, const void* w1, const void* w3, void* hid, int F) {
  GemvArgs a = gemv_common(h, D, D, F, norm_w, eps, hid, F);
  a.mode = GEMV_SWIGLU;
  a.w0 = (const bf16_t*)w1; a.w1 = (const bf16_t*)w3; a.n0 = a.n1 = F;
  return a;
}
// logits[T, V] (fp32) = rmsnorm(h[T, D]) @ w^T
GemvArgs gemv_logits(const void* h, int D, const void* norm_w, float eps, const void* w, float* logits, int V) {
  GemvArgs a = gemv_common(h, D, D, V, norm_w, eps, logits, V);
  a.mode = GEMV_LOGITS;
  a.w0 = (const bf16_t*)w; a.n0 = a.n1 = V;
  return a;
}

// The two compiles of gemv.hip: bf16 payloads (mi_forward, the bf16 leaves) and fp16 payloads (mi_forward_generic).
struct GemvKernels {
  int (*max_tokens)(int K);
  hipError_t (*launch)(const GemvArgs&, hipStream_t);
};
constexpr GemvKernels kGemvBf16 = {gemv_max_tokens, launch_gemv}, kGemvF16 = {gemv_max_tokens_f16, launch_gemv_f16};

// GEMV over T <= 8 tokens, in passes of at most `cap` rows when T * K does not fit the LDS budget.
template <class Launch>
int gemv_pass_loop(int cap, const GemvArgs& a, int T, const char* what, Launch&& launch) {
  const size_t out_elt = (a.mode == GEMV_LOGITS) ? 4 : 2;
  for (int t0 = 0; t0 < T; t0 += cap) {
    GemvArgs p = a;
    p.T = (T - t0 < cap) ? T - t0 : cap;
    p.x = a.x + (size_t)t0 * a.ldx;
    p.out = (char*)a.out + (size_t)t0 * a.ldo * out_elt;
    if (a.residual) p.residual = a.residual + (size_t)t0 * a.ldo;
    if (a.tok_pos) p.tok_pos = a.tok_pos + t0;
    if (a.tok_seq) p.tok_seq = a.tok_seq + t0;
    else p.seq0 = a.seq0 + t0;  // (no tok_seq: token t is sequence t, in every pass)
    MI_TRY(hip_rc(launch(p), what));
  }
  return MI_OK;
}
int gemv_passes(const GemvKernels& k, const GemvArgs& a, int T, hipStream_t s, const char* what) {
  return gemv_pass_loop(k.max_tokens(a.K), a, T, what, [&](const GemvArgs& p) { return k.launch(p, s); });
}
// The weight-only formats: the same launches with the weight pointers read as quantised bytes and the scales beside the arguments
// (activation rows are bf16 there too: the bf16 kernels' row budget).  A format is one trait: its scale element, K modulus, names
// and the two launchers of its file.
template <class scale_t>
struct Scales {
  const scale_t* s[3];
};
struct QuantW8 {  // gemv_w8.hip: e4m3 bytes, one fp32 scale per row
  typedef float scale_t;
  static constexpr int kFormat = MI_W8_FP8_E4M3, kMod = 16;
  static constexpr const char *kFormatName = "MI_W8_FP8_E4M3 = 1", *kArg = "w8", *kName = "FP8", *kScales = "row scales";
  static constexpr const char* kWhy = "a 16-byte piece is 16 e4m3 weights";
  static constexpr const char *kLinear = "mi_linear_w8", *kQkv = "mi_qkv_rope_kvwrite_w8", *kGemv = "gemv (w8)", *kDequant = "dequant (w8)",
                              *kQkvGemv = "qkv gemv (w8)", *kLinearA8 = "mi_linear_w8a8", *kQkvA8 = "mi_qkv_rope_w8a8",
                              *kPrior = "mi_qkv_rope_kvwrite_w8", *kGemmA8 = "FP8 prefill GEMM",
                              *kOperandsA8 = "x and the weights 16-byte aligned";
  static constexpr auto launch_gemv = launch_gemv_w8;
  static constexpr auto launch_dequant = launch_dequant_w8;
  static size_t row_bytes(int K) { return (size_t)K; }  // of a weight row; scale elements of a row
  static size_t row_scales(int) { return 1; }
};
struct QuantW4 {  // gemv_w4.hip: MXFP4 code bytes, one e8m0 scale byte per block of 32
  typedef uint8_t scale_t;
  static constexpr int kFormat = MI_W4_MXFP4, kMod = 32;
  static constexpr const char *kFormatName = "MI_W4_MXFP4 = 2", *kArg = "w4", *kName = "MXFP4", *kScales = "block scales";
  static constexpr const char* kWhy = "one e8m0 scale per block of 32 MXFP4 weights";
  static constexpr const char *kLinear = "mi_linear_w4", *kQkv = "mi_qkv_rope_kvwrite_w4", *kGemv = "gemv (w4)", *kDequant = "dequant (w4)",
                              *kQkvGemv = "qkv gemv (w4)", *kLinearA8 = "mi_linear_w4a8", *kQkvA8 = "mi_qkv_rope_w4a8",
                              *kPrior = "mi_qkv_rope_kvwrite_w4", *kGemmA8 = "MXFP4 x FP8 prefill GEMM",
                              *kOperandsA8 = "x and the code matrices 16-byte aligned, the block scale matrices 4-byte aligned";
  static constexpr auto launch_gemv = launch_gemv_w4;
  static constexpr auto launch_dequant = launch_dequant_w4;
  static size_t row_bytes(int K) { return (size_t)K >> 1; }
  static size_t row_scales(int K) { return (size_t)K >> 5; }
};
template <class Q>
int gemv_passes_quant(const GemvArgs& a, const Scales<typename Q::scale_t>& sc, int T, hipStream_t s, const char* what) {
  return gemv_pass_loop(gemv_max_tokens(a.K), a, T, what, [&](const GemvArgs& p) {
    const GemvScaledArgs<typename Q::scale_t> w = {p, {sc.s[0], sc.s[1], sc.s[2]}};
    return Q::launch_gemv(w, s);
  });
}
// Dequantise up to three matrices of K columns side by side into `out` (dense [sum of rows, K] bf16); w[i] then points at the
// bf16 rows of matrix i.
template <class Q>
int dequant_group(const void* w[3], const Scales<typename Q::scale_t>& sc, const int n_rows[3], int K, bf16_t* out, hipStream_t s, const char* what) {
  DequantArgs<typename Q::scale_t> d;
  memset(&d, 0, sizeof(d));
  int n = 0;
  for (int i = 0; i < 3; ++i) {
    const int rows = w[i] ? n_rows[i] : 0;
    d.w[i] = (const uint8_t*)w[i]; d.scale[i] = sc.s[i];
    if (i == 0) d.n0 = rows;
    if (i == 1) d.n1 = d.n0 + rows;
    w[i] = w[i] ? (const void*)(out + (size_t)n * K) : nullptr;
    n += rows;
  }
  if (!d.w[1]) d.n1 = d.n0;
  d.N = n; d.K = K; d.out = out;
  return hip_rc(Q::launch_dequant(d, s), what);
}
struct PlainBf16 {  // no format: what the q|k|v leaf that the formats share reads of a trait, for bf16 weights (no scales)
  typedef float scale_t;
  static constexpr int kFormat = 0;
  static constexpr const char *kLinear = "mi_linear", *kQkv = "mi_qkv_rope_kvwrite", *kQkvGemv = "qkv gemv";
};
// The quantisation that forward_body runs a model under: what mi_forward_w8 / mi_forward_w4 were handed, as one argument.
struct QuantModel {
  int entry_format;  // the format of the entry point that was called: MI_W8_FP8_E4M3 / MI_W4_MXFP4
  int format;        // the format the caller's struct names (check_quant: must be the entry's)
  const mi_w8_layer_t* l8;  // host [n_layers]; the table of entry_format, the other one nullptr
  const mi_w4_layer_t* l4;
  const mi_lm_head_quant_t* head;  // mi_forward_q: the LM head is quantised too (m->output: its bytes), or nullptr - a bf16 head
};
// f(trait of the format)
template <class Fn>
int with_format(int format, Fn&& f) { return format == MI_W4_MXFP4 ? f(QuantW4{}) : f(QuantW8{}); }
inline const mi_w8_layer_t* layers_of(const QuantModel& q, QuantW8) { return q.l8; }
inline const mi_w4_layer_t* layers_of(const QuantModel& q, QuantW4) { return q.l4; }
// of the one struct that an entry point was handed (neither: not read)
QuantModel quant_model(const mi_w8_model_t* w8, const mi_w4_model_t* w4) {
  if (w8) return {MI_W8_FP8_E4M3, w8->format, w8->layers, nullptr, nullptr};
  return w4 ? QuantModel{MI_W4_MXFP4, w4->format, nullptr, w4->layers, nullptr} : QuantModel{};
}

// ---- MoE FFN of T <= 8 tokens: per (token, slot) gate | up + SwiGLU into hid [T * top_k, F], then per token the down
// projections, the weighted combine and the residual
int moe_decode(void* out, const void* residual, const void* x, int ldx, int T, int D, int F, const void* const* expert_tab,
               const int32_t* sel_idx, const float* sel_w, int top_k, const void* norm_w, float eps, void* hid, hipStream_t s) {
  GemvArgs a = gemv_common(x, ldx, D, F, norm_w, eps, hid, F);
  a.mode = GEMV_MOE_W13; a.T = T;
  a.expert_tab = expert_tab; a.sel_idx = sel_idx; a.sel_w = sel_w; a.top_k = top_k;
  MI_TRY(hip_rc(launch_gemv(a, s), "moe w13 gemv"));
  a = gemv_common(hid, F, F, D, nullptr, 0.f, out, D);
  a.mode = GEMV_MOE_W2; a.T = T; a.residual = (const bf16_t*)residual;
  a.expert_tab = expert_tab; a.sel_idx = sel_idx; a.sel_w = sel_w; a.top_k = top_k;
  return hip_rc(launch_gemv(a, s), "moe w2 gemv");
}

struct MoeScratch {
  bf16_t* hid;       // [T * top_k, F]
  bf16_t* y;         // expert outputs, compact rows      [T * top_k, D]
  int32_t* tok_of;   // token of compact row r            [T * top_k]
  int32_t* row_of;   // compact row of (token, slot)      [T * top_k]
  int32_t* tile_tab; // grouped-GEMM m-tile table         [max_tiles][4]
  int32_t* n_tiles;
  int max_tiles;
  size_t total;
};
// ---- MoE FFN of a prefill: x [T, D] dense rows (already normed).  One token-grouped launch per projection covers all experts
// (tile table built on the device: no host sync), then the weighted combine and the residual.
int moe_grouped(void* out, const void* residual, const void* x, int T, int D, int F, int E, int k, const void* const* expert_tab,
                const int32_t* sel_idx, const float* sel_w, const MoeScratch& w, hipStream_t s) {
  // 256-row m-tiles (gemm256.hip) once an expert averages a few of them, else 128-row tiles (gemm.hip)
  const int tile_rows = ((long)T * k >= 512L * E && D % 64 == 0 && F % 64 == 0) ? 256 : 128;
  const int max_m_tiles = (T * k + tile_rows - 1) / tile_rows + E;  // <= the scratch's max_tiles (sized for 128-row tiles)
  MI_TRY(hip_rc(launch_moe_lists(sel_idx, T, E, k, w.tok_of, w.row_of, w.tile_tab, w.n_tiles, tile_rows, s), "moe_lists"));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.epi = GEMM_SWIGLU; g.M = T * k; g.N = F; g.K = D; g.a = (const bf16_t*)x; g.lda = D; g.n0 = g.n1 = F;
  g.out = w.hid; g.ldo = F;
  g.tile_tab = w.tile_tab; g.n_tiles_ptr = w.n_tiles; g.max_m_tiles = max_m_tiles; g.tile_rows = tile_rows;
  g.expert_tab = expert_tab; g.w_sel0 = 0; g.w_sel1 = 2; g.a_gather = w.tok_of;
  MI_TRY(hip_rc(launch_gemm(g, s), "moe w13 grouped gemm"));
  memset(&g, 0, sizeof(g));
  g.epi = GEMM_STORE; g.M = T * k; g.N = D; g.K = F; g.a = w.hid; g.lda = F; g.n0 = g.n1 = D;
  g.out = w.y; g.ldo = D;
  g.tile_tab = w.tile_tab; g.n_tiles_ptr = w.n_tiles; g.max_m_tiles = max_m_tiles; g.tile_rows = tile_rows;
  g.expert_tab = expert_tab; g.w_sel0 = 1; g.w_sel1 = -1;
  MI_TRY(hip_rc(launch_gemm(g, s), "moe w2 grouped gemm"));
  return hip_rc(launch_moe_combine(out, residual, w.y, sel_idx, sel_w, w.row_of, T, D, k, s), "moe combine");
}

// ---- scratch of the un-merged LoRA leaf (mi_lora_linear; the launches: linear_group below)
struct LoraScratch {
  void* base;
  bf16_t* t;
  bf16_t* xn;
  size_t total;
};
LoraScratch lora_carve(int M, int K, int n_total, int nseg, int rank, bool base_f32, bool fused_norm, char* p) {
  LoraScratch w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off += align_up(bytes);
    return q;
  };
  w.base = take((size_t)M * n_total * (base_f32 ? 4 : 2));
  w.t = (bf16_t*)take((size_t)M * nseg * rank * 2);
  w.xn = (bf16_t*)take(fused_norm ? (size_t)M * K * 2 : 0);
  w.total = off;
  return w;
}
// what the leaf derives from its arguments (0 segments: refused)
struct LoraShape {
  int nseg, n_total;
  bool base_f32;
};
LoraShape lora_shape(const int n_rows[3], int epilogue, bool fused_norm) {
  LoraShape sh = {0, 0, false};
  if (epilogue == MI_EPI_SWIGLU) {
    sh.nseg = 2;
    sh.n_total = 2 * n_rows[0];
  } else {
    for (int i = 0; i < 3 && n_rows[i] > 0; ++i) {
      ++sh.nseg;
      sh.n_total += n_rows[i];
    }
  }
  // the plain linear a fused-norm SwiGLU compares with is the GEMV's norm mode; store / residual with a fused norm are not
  sh.base_f32 = fused_norm && epilogue == MI_EPI_SWIGLU;
  return sh;
}

// ---- attention arguments (scratch = the tickets block and the split partials behind it)
AttnDecodeArgs attn_decode_args(void* out, const void* q, int ldq, const void* cache_k, const void* cache_v, int kv_layout, int W,
                                int B, int H, int Hkv, int Dh, const int32_t* tok_pos, int32_t* tickets, float* partial) {
  AttnDecodeArgs a = {};  // (kv_groups: launch_attn_decode sets it)
  a.out = out; a.q = (const bf16_t*)q; a.ldq = ldq; a.cache_k = (const bf16_t*)cache_k; a.cache_v = (const bf16_t*)cache_v;
  a.kv_layout = kv_layout;
  a.W = W; a.B = B; a.H = H; a.Hkv = Hkv; a.Dh = Dh; a.tok_pos = tok_pos;
  a.tickets = tickets; a.partial = partial; a.n_splits = attn_decode_splits(W);
  return a;
}
// softmax_scale <= 0: 1 / sqrt(head_dim)
AttnPrefillArgs attn_prefill_args(void* out, const void* qkv, int ld, const void* cache_k, const void* cache_v, int kv_layout, int W,
                                  int B, int max_q_len, int H, int Hkv, int Dh, const int32_t* q_start, const int32_t* kv_before,
                                  int causal, float softmax_scale) {
  AttnPrefillArgs a = {};
  a.out = out; a.qkv = (const bf16_t*)qkv; a.ld = ld; a.cache_k = (const bf16_t*)cache_k; a.cache_v = (const bf16_t*)cache_v;
  a.kv_layout = kv_layout;
  a.W = W; a.B = B; a.max_q_len = max_q_len; a.H = H; a.Hkv = Hkv; a.Dh = Dh;
  a.q_start = q_start; a.kv_before = kv_before; a.causal = causal;
  a.scale = softmax_scale > 0.f ? softmax_scale : 1.0f / sqrtf((float)Dh);
  return a;
}

// The ring write as a launch of its own: the k | v columns of qkv [T, ldo] (behind nq columns of q) go to slot tok_pos % W of
// sequence tok_seq (nullptr: the row index) - of bf16 rings or, by the layout, of e4m3 rings.  q_start == nullptr: no window drop.
int ring_write(const RingWrite& ring, const void* qkv, int ldo, int T, int nq, int nkv, int head_dim, const int32_t* tok_pos,
               const int32_t* tok_seq, const int32_t* q_start, hipStream_t s, const char* what) {
  const bf16_t* k = (const bf16_t*)qkv + nq;
  return hip_rc(launch_kv_write(ring.k, ring.v, ring.W, k, k + nkv, ldo, T, nkv, tok_seq, tok_pos, q_start, ring.layout, head_dim, s), what);
}

// ---- One linear group: up to three weight matrices of K columns read side by side (q|k|v, wo, w1|w3, w2, the LM head) in one
// weight format, with or without un-merged LoRA adapters (lora.py:71-74).  Every linear of the leaves and of forward_body is this
// description, a LinearCall and linear_group(): the one place that picks and sequences the launches.
struct LinearGroup {
  const void* w[3];     // weight segments (SwiGLU: W1, W3); nullptr: no such segment
  int n_rows[3];
  int nseg, K;
  int format;           // 0: bf16; MI_W8_FP8_E4M3 / MI_W4_MXFP4: w[] are quantised bytes with the scales of that format's type
  Scales<float> s8;
  Scales<uint8_t> s4;
  // adapters (rank > 0): A[i] [rank, K] and B[i] [n_rows[i], rank] per segment, or both nullptr.  bank.seq_slot != nullptr (ABI v9):
  // A[i] / B[i] are the bases of [slots, rank, K] / [slots, n_rows[i], rank] arrays and row m runs through slot
  // seq_slot[tok_seq[m]] (kernels.h); all zero: one adapter set, the kernels' single-adapter mode
  const void *A[3], *B[3];
  int rank;
  float scaling;
  LoraBank bank;
};
LinearGroup group_of(int K, const void* w0, int r0, const void* w1 = nullptr, int r1 = 0, const void* w2 = nullptr, int r2 = 0) {
  LinearGroup g;
  memset(&g, 0, sizeof(g));
  g.w[0] = w0; g.w[1] = w1; g.w[2] = w2; g.n_rows[0] = r0; g.n_rows[1] = r1; g.n_rows[2] = r2;
  g.nseg = !w0 ? 0 : !w1 ? 1 : !w2 ? 2 : 3;
  g.K = K;
  return g;
}
inline void set_scales(LinearGroup& g, QuantW8, const float* s0, const float* s1 = nullptr, const float* s2 = nullptr) {
  g.format = QuantW8::kFormat; g.s8 = {{s0, s1, s2}};
}
inline void set_scales(LinearGroup& g, QuantW4, const uint8_t* s0, const uint8_t* s1 = nullptr, const uint8_t* s2 = nullptr) {
  g.format = QuantW4::kFormat; g.s4 = {{s0, s1, s2}};
}
inline const Scales<float>& scales_of(const LinearGroup& g, QuantW8) { return g.s8; }
inline const Scales<uint8_t>& scales_of(const LinearGroup& g, QuantW4) { return g.s4; }
inline void set_adapters(LinearGroup& g, int rank, float scaling, const LoraBank& bank, const void* a0, const void* b0,
                         const void* a1 = nullptr, const void* b1 = nullptr, const void* a2 = nullptr, const void* b2 = nullptr) {
  g.rank = rank; g.scaling = scaling; g.bank = bank; g.A[0] = a0; g.A[1] = a1; g.A[2] = a2; g.B[0] = b0; g.B[1] = b1; g.B[2] = b2;
}

// What the 16-byte accesses of the W8A8 route need of a call beside its shape (gemm256_w8a8_applicable): the quantiser loads 16
// bytes of x per lane, the GEMM's DMA 16 bytes of a weight row.  A call that does not meet it takes the weight-only routes.
inline bool w8a8_operands_ok(const void* x, int ldx, const void* const w[3]) {
  return ldx % 8 == 0 && ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(w[0]) | reinterpret_cast<size_t>(w[1]) |
                           reinterpret_cast<size_t>(w[2])) & 15) == 0;
}

// The route's one shape predicate, by the group's format (kernels.h): the runner, the leaves and the scratch queries all ask here
inline bool a8_applicable(int format, int M, int K) {
  return format == MI_W4_MXFP4 ? gemm256_w4a8_applicable(M, K) : gemm256_w8a8_applicable(M, K);
}
// The operands' needs for a group of either format: the W4A8 GEMM also stages the block scale bytes by 4-byte DMA (rows are K / 32 = 4 k bytes)
inline bool a8_operands_ok(const LinearGroup& G, const void* x, int ldx) {
  if (G.format == MI_W4_MXFP4 &&
      ((reinterpret_cast<size_t>(G.s4.s[0]) | reinterpret_cast<size_t>(G.s4.s[1]) | reinterpret_cast<size_t>(G.s4.s[2])) & 3))
    return false;
  return w8a8_operands_ok(x, ldx, G.w);
}

constexpr int EPI_QKV_ROPE = 100;  // beside the public MI_EPI_* codes: the fused q|k|v + RoPE (+ ring write)
struct LinearLabels {  // the `what` of each launch (error details name it); nullptr: the caller cannot reach that launch
  const char *gemv, *gemm, *dequant, *norm;
  // the separate ring write behind a GEMV that could not fuse it (e4m3 rings) / behind the GEMM or LoRA route: two labels because
  // forward_body's error details have always told the two apart ("kv_write (decode, e4m3)" / "kv_write (decode)")
  const char *ring_gemv, *ring;
};
struct LinearCall {
  const void* x;         // [M, ldx]; pre-norm when norm_w is given
  int ldx;
  const void* norm_w;    // fused RMSNorm (eps) in front of the product, or nullptr
  float eps;
  void* out;             // [M, ldo] bf16 (fp32: EPI_LOGITS)
  int ldo;
  const void* residual;
  int epi;               // MI_EPI_* (the leaves pass validated codes only) or EPI_QKV_ROPE
  // EPI_QKV_ROPE: the segments are wq | wk | wv over heads of head_dim.  ring != nullptr: the k | v columns also go to the ring
  // (a separate launch reads ring_q_start: nullptr, no window drop)
  const float* rope_cs;
  const int32_t *tok_pos, *tok_seq;
  int head_dim;
  const RingWrite* ring;
  const int32_t* ring_q_start;
  // scratch of the routes; nullptr: the route is not open to this caller
  bf16_t* xn;            // [M, K]: the RMSNorm as a launch of its own (M > 8, and whatever lora_down reads)
  bf16_t* deq;           // the bf16 image of the group's quantised weights (M > 8)
  void* lora_base;       // [M, sum of n_rows]: the base product of a group with adapters - bf16, or with lora_base_f32 fp32 holding
  bf16_t* lora_t;        //     bf16 values (below);  lora_t [M, nseg * rank]: t = bf16(A xn)
  // the base GEMV (M <= 8) in its LOGITS form: its fused RMSNorm is the one of the fused q|k|v and W1|W3 modes (gemv_core.cuh
  // kNormMode: same staging, same order of the sum of squares), so that a model whose adapters are zero reproduces the plain model
  // bit for bit.  forward_body asks for it at q|k|v and W1|W3, the leaf only for a fused-norm SwiGLU (lora_shape)
  bool lora_base_f32;
  LinearLabels what;
  // FP8 prefill GEMMs (opt-in: mi_linear_w8a8, mi_forward_w8a8; on MXFP4 weights mi_linear_w4a8, mi_forward_w4a8): a quantised group
  // of M >= 256 rows and K % 128 == 0 quantises its input rows into x_q [M, K] e4m3 bytes / s_x [M] and runs the W8A8 GEMM (the W4A8
  // GEMM) on the weight bytes as they are
  bool a8;
  uint8_t* x_q;
  float* s_x;
};

// A quantised LM head (one matrix, G.format != 0) at more than 8 rows.  g: the GEMM of the whole head on its bf16 image (GEMM_LOGITS
// or GEMM_LOGPROB; g.w0 is not read).  Per slice of LM_HEAD_SLICE_ROWS vocabulary rows: one dequantisation launch into `deq`
// (lm_head_slice_bytes), then the GEMM on the slice's columns.  Every column runs on the kernel that the one launch on the whole
// image would give it (gemm_plan), with the same K loop on the same bf16 weights: the logits are those of the unsliced launch, bit
// for bit.  The fused log-prob partials of a slice go to the slice's tiles of the whole head's [M][tiles] array (lp_col0, lp_tiles).
int head_gemm_sliced(const LinearGroup& G, const GemmArgs& g, bf16_t* deq, hipStream_t s, const char* what_dequant, const char* what_gemm) {
  GemmArgs whole = g;
  whole.w0 = deq; whole.w1 = whole.w2 = nullptr; whole.n0 = whole.n1 = g.N;
  const int c256 = g.epi == GEMM_LOGPROB ? g.N : gemm_plan(whole).c256;  // (the logits' tail is the 128-tile kernel's: no half tiles)
  for (int r0 = 0; r0 < g.N; r0 += LM_HEAD_SLICE_ROWS) {
    const int r1 = g.N - r0 < LM_HEAD_SLICE_ROWS ? g.N : r0 + LM_HEAD_SLICE_ROWS;
    MI_TRY(with_format(G.format, [&](auto Q) {
      typedef decltype(Q) F;
      const void* w[3] = {(const uint8_t*)G.w[0] + (size_t)r0 * F::row_bytes(G.K), nullptr, nullptr};
      Scales<typename F::scale_t> sc = {{scales_of(G, Q).s[0] + (size_t)r0 * F::row_scales(G.K), nullptr, nullptr}};
      const int nr[3] = {r1 - r0, 0, 0};
      return dequant_group<F>(w, sc, nr, G.K, deq, s, what_dequant);
    }));
    const int cut = c256 < r0 ? r0 : (c256 > r1 ? r1 : c256);  // columns [r0, cut) on the 256-tile kernel, [cut, r1) on the 128-tile one
    const int part[2][2] = {{r0, cut}, {cut, r1}};
    for (int i = 0; i < 2; ++i) {
      const int a = part[i][0], b = part[i][1];
      if (b <= a) continue;
      GemmArgs p = whole;
      p.N = p.n0 = p.n1 = b - a;
      p.w0 = deq + (size_t)(a - r0) * G.K;
      if (g.epi == GEMM_LOGPROB) {
        p.lp_col0 = a; p.lp_tiles = (g.N + 255) / 256;
      } else {
        p.out = reinterpret_cast<float*>(g.out) + a;
      }
      MI_TRY(hip_rc(i == 0 ? launch_gemm256(p, s) : launch_gemm128(p, s), what_gemm));
    }
  }
  return MI_OK;
}

// M <= GEMV_MAX_T rows: weight-streaming GEMV passes with the RMSNorm, RoPE and (bf16 rings) the ring write fused.  More rows: the
// RMSNorm into xn, the bf16 image of quantised weights into deq, then the MFMA GEMM (RoPE in its epilogue when it takes the heads).
// Quantised groups with C.a8 at M >= 256 rows and K % 128 == 0: the per-token e4m3 quantisation of the input rows (the RMSNorm fused
// into it) and the format's FP8-activation MFMA GEMM on the weight bytes (gemm256_w8a8.hip / gemm256_w4a8.hip) - no xn, no deq, no
// dequantisation launch; any other shape takes the routes above.
// Adapters: the RMSNorm into xn at any M (lora_down reads it), the base product by the same two routes in plain store form,
// lora_down, lora_up with the epilogue, then RoPE and the ring write as passes of their own (bit-equal to the fused epilogues:
// same arithmetic on the same bf16 values).
int linear_group(const LinearGroup& G, const LinearCall& C, int M, hipStream_t s) {
  const bool gemv = M <= GEMV_MAX_T, swiglu = C.epi == MI_EPI_SWIGLU, qkv = C.epi == EPI_QKV_ROPE;
  const int K = G.K, n0 = G.n_rows[0], n1 = n0 + (G.w[1] ? G.n_rows[1] : 0), n2 = n1 + (G.w[2] ? G.n_rows[2] : 0);
  const bool fused_ring = C.ring && gemv && G.rank == 0 && !kv_e4m3(C.ring->layout);  // (the GEMV epilogue stores bf16 only)
  // RoPE rides on the GEMV's epilogue, and on the GEMM's (same arithmetic as rope_kernel on the same bf16-rounded values; it was a
  // separate 20 us pass over q|k per layer at 4096 tokens) unless the heads are of a size that epilogue does not take
  const bool fused_rope = qkv && G.rank == 0 && (gemv || (fuse_rope_enabled() && C.head_dim % 16 == 0));  // (either GEMM's epilogue)
  const bool a8 = C.a8 && C.x_q && C.s_x && G.format != 0 && G.rank == 0 && C.epi != MI_EPI_LOGITS && a8_applicable(G.format, M, K) &&
                  a8_operands_ok(G, C.x, C.ldx);
  if (C.norm_w && !C.xn && !a8 && (!gemv || G.rank > 0)) return fail(MI_ERR_UNSUPPORTED, "linear group: fused RMSNorm only on the M <= 8 path");
  if (G.rank > 0) {
    const void* xn = C.x;
    int ldxn = C.ldx;
    if (C.norm_w) {
      MI_TRY(hip_rc(launch_rmsnorm(C.xn, C.x, C.norm_w, M, K, C.eps, s), C.what.norm));
      xn = C.xn; ldxn = K;
    }
    LinearGroup base = G;
    base.rank = 0;
    LinearCall bc = C;
    bc.epi = C.lora_base_f32 ? MI_EPI_LOGITS : MI_EPI_STORE; bc.out = C.lora_base; bc.ldo = n2; bc.residual = nullptr; bc.ring = nullptr;
    bc.what.gemv = "lora base gemv"; bc.what.gemm = "lora base gemm";
    if (!gemv) { bc.x = xn; bc.ldx = ldxn; bc.norm_w = nullptr; }  // (M <= 8: the GEMV fuses the norm on x itself)
    MI_TRY(linear_group(base, bc, M, s));
    bool any = false;
    for (int i = 0; i < G.nseg; ++i) any = any || (G.A[i] && G.B[i]);
    if (any) {
      LoraDownArgs d;
      memset(&d, 0, sizeof(d));
      d.x = (const bf16_t*)xn; d.ldx = ldxn; d.T = M; d.K = K; d.nseg = G.nseg; d.r = G.rank; d.t = C.lora_t;
      d.a_stride = (int64_t)G.rank * K; d.bank = G.bank;
      for (int i = 0; i < G.nseg; ++i) d.A[i] = (G.A[i] && G.B[i]) ? (const bf16_t*)G.A[i] : nullptr;
      MI_TRY(hip_rc(launch_lora_down(d, s), "lora_down"));
    }
    LoraUpArgs u;
    memset(&u, 0, sizeof(u));
    u.epi = qkv ? MI_EPI_STORE : C.epi;
    u.T = M; u.N = swiglu ? n0 : n2; u.base = C.lora_base; u.ldb = n2; u.base_f32 = C.lora_base_f32 ? 1 : 0;
    u.t = C.lora_t; u.n0 = n0; u.n1 = n1; u.nseg = G.nseg; u.r = G.rank; u.scaling = G.scaling;
    u.bank = G.bank;
    for (int i = 0; i < G.nseg; ++i) u.b_stride[i] = (int64_t)G.n_rows[i] * G.rank;
    for (int i = 0; i < G.nseg; ++i) u.B[i] = (G.A[i] && G.B[i]) ? (const bf16_t*)G.B[i] : nullptr;
    u.out = (bf16_t*)C.out; u.ldo = C.ldo; u.residual = (const bf16_t*)C.residual;
    u.fast_silu = !gemv;  // (the SiLU of the path that a plain linear of this M takes: gemv_core.cuh / gemm.hip)
    MI_TRY(hip_rc(launch_lora_up(u, s), "lora_up"));
  } else if (gemv) {
    GemvArgs a = gemv_common(C.x, C.ldx, K, swiglu ? n0 : n2, C.norm_w, C.eps, C.out, C.ldo);
    a.mode = swiglu ? GEMV_SWIGLU : qkv ? GEMV_QKV_ROPE : C.epi == MI_EPI_STORE ? GEMV_STORE : C.epi == MI_EPI_RESIDUAL ? GEMV_RESIDUAL : GEMV_LOGITS;
    a.w0 = (const bf16_t*)G.w[0]; a.w1 = (const bf16_t*)G.w[1]; a.w2 = (const bf16_t*)G.w[2]; a.n0 = n0; a.n1 = swiglu ? n0 : n1;
    a.residual = (const bf16_t*)C.residual;
    if (qkv) { a.rope_cs = C.rope_cs; a.tok_pos = C.tok_pos; a.tok_seq = C.tok_seq; a.head_dim = C.head_dim; }
    // (without a fused write the four ring fields stay 0: the kernel reads them only under write_kv, so there is no pos % 0)
    if (fused_ring) { a.write_kv = 1; a.cache_k = C.ring->k; a.cache_v = C.ring->v; a.W = C.ring->W; a.kv_layout = C.ring->layout; }
    if (G.format)
      MI_TRY(with_format(G.format, [&](auto Q) { return gemv_passes_quant<decltype(Q)>(a, scales_of(G, Q), M, s, C.what.gemv); }));
    else
      MI_TRY(gemv_passes(kGemvBf16, a, M, s, C.what.gemv));
  } else if (a8) {
    MI_TRY(hip_rc(launch_act_quant_e4m3(C.x_q, C.s_x, C.x, C.ldx, M, K, C.norm_w, C.eps, s), "act_quant_e4m3"));
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.epi = swiglu ? GEMM_SWIGLU : (C.epi == MI_EPI_STORE || qkv) ? GEMM_STORE : GEMM_RESIDUAL;
    g.M = M; g.N = swiglu ? n0 : n2; g.K = K; g.a = (const bf16_t*)C.x_q; g.lda = K;
    g.w0 = (const bf16_t*)G.w[0]; g.w1 = (const bf16_t*)G.w[1]; g.w2 = (const bf16_t*)G.w[2]; g.n0 = n0; g.n1 = swiglu ? n0 : n1;
    g.out = C.out; g.ldo = C.ldo; g.residual = (const bf16_t*)C.residual;
    if (fused_rope) { g.rope_cs = C.rope_cs; g.tok_pos = C.tok_pos; g.rope_cols = n1; g.rope_dh = C.head_dim; }
    if (G.format == MI_W4_MXFP4) {  // e2m1 codes x e4m3 bytes, the block scales inside the MFMA
      const GemmW4A8Args a = {g, C.s_x, {G.s4.s[0], G.s4.s[1], G.s4.s[2]}};
      MI_TRY(hip_rc(launch_gemm256_w4a8(a, s), "w4a8 gemm"));
    } else {  // e4m3 bytes x e4m3 bytes, the row scales in the epilogue
      const GemmW8A8Args a = {g, C.s_x, {G.s8.s[0], G.s8.s[1], G.s8.s[2]}};
      MI_TRY(hip_rc(launch_gemm256_w8a8(a, s), "w8a8 gemm"));
    }
  } else {
    const bf16_t* x = (const bf16_t*)C.x;
    int ldx = C.ldx;
    if (C.norm_w) {
      MI_TRY(hip_rc(launch_rmsnorm(C.xn, C.x, C.norm_w, M, K, C.eps, s), C.what.norm));
      x = C.xn; ldx = K;
    }
    const void* w[3] = {G.w[0], G.w[1], G.w[2]};
    const bool head_slices = G.format && C.epi == MI_EPI_LOGITS;  // a quantised LM head: its bf16 image slice by slice
    if (G.format) {
      if (!C.deq) return fail(MI_ERR_WORKSPACE, "linear group: no scratch for the dequantised weights");
      const int nr[3] = {n0, n1 - n0, n2 - n1};
      if (!head_slices)
        MI_TRY(with_format(G.format, [&](auto Q) { return dequant_group<decltype(Q)>(w, scales_of(G, Q), nr, K, C.deq, s, C.what.dequant); }));
    }
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.epi = swiglu ? GEMM_SWIGLU : (C.epi == MI_EPI_STORE || qkv) ? GEMM_STORE : C.epi == MI_EPI_RESIDUAL ? GEMM_RESIDUAL : GEMM_LOGITS;
    g.M = M; g.N = swiglu ? n0 : n2; g.K = K; g.a = x; g.lda = ldx;
    g.w0 = (const bf16_t*)w[0]; g.w1 = (const bf16_t*)w[1]; g.w2 = (const bf16_t*)w[2]; g.n0 = n0; g.n1 = swiglu ? n0 : n1;
    g.out = C.out; g.ldo = C.ldo; g.residual = (const bf16_t*)C.residual;
    if (fused_rope) { g.rope_cs = C.rope_cs; g.tok_pos = C.tok_pos; g.rope_cols = n1; g.rope_dh = C.head_dim; }
    if (head_slices) MI_TRY(head_gemm_sliced(G, g, C.deq, s, C.what.dequant, C.what.gemm));
    else MI_TRY(hip_rc(launch_gemm(g, s), C.what.gemm));
  }
  if (qkv && !fused_rope)
    MI_TRY(hip_rc(launch_rope(C.out, C.ldo, M, n0 / C.head_dim, (n1 - n0) / C.head_dim, C.head_dim, C.rope_cs, C.tok_pos, s), "rope"));
  // the ring write must precede the attention (cache.py:83-92 `update` then read, transformer_layers.py:77-81)
  if (C.ring && !fused_ring)
    MI_TRY(ring_write(*C.ring, C.out, C.ldo, M, n0, n1 - n0, C.head_dim, C.tok_pos, C.tok_seq, C.ring_q_start, s,
                      (gemv && G.rank == 0) ? C.what.ring_gemv : C.what.ring));
  return MI_OK;
}

// ---- what mi_forward and mi_forward_generic check of a batch, in the order the checks fire
struct BatchInfo {
  int T, B, branch, kv_layout;
  bool has_cache;
  bool want_sample;  // the step's token is picked on the device behind the LM head ...
  bool want_topp;    // ... by a nucleus draw instead of the argmax (ABI v5; generate.py:126 at temperature > 0)
};
// The checks before the workspace is sized.  attn_rows: mi_forward's decode attention keeps one word per (sequence, kv head)
// in the TICKET_BYTES block.
int check_batch(const char* entry, const mi_model_t* m, const mi_batch_t* bt, bool attn_rows, BatchInfo* info) {
  if (!bt || bt->T <= 0 || bt->B <= 0 || !bt->h || !bt->workspace) return fail(MI_ERR_ARG, "%s: batch", entry);
  if (!bt->q_start || !bt->kv_before || !bt->tok_seq || !bt->tok_pos) return fail(MI_ERR_ARG, "%s: metadata", entry);
  BatchInfo& b = *info;
  b.T = bt->T; b.B = bt->B; b.branch = bt->branch; b.kv_layout = bt->kv_layout;
  b.has_cache = b.branch != MI_BRANCH_NOCACHE;
  if (b.has_cache && (!bt->cache_k || !bt->cache_v || !bt->cache_sizes)) return fail(MI_ERR_ARG, "%s: cache", entry);
  if (!kv_layout_ok(bt->kv_layout)) return fail(MI_ERR_ARG, "%s: kv_layout", entry);
  if (b.branch == MI_BRANCH_DECODE && (b.T != b.B || !bt->kv_seqlens)) return fail(MI_ERR_ARG, "%s: decode needs T == B", entry);
  if (attn_rows && (size_t)b.B * m->n_kv_heads * 4 > TICKET_BYTES) return fail(MI_ERR_SHAPE, "B * n_kv_heads > 1024");
  if (bt->logits && (!m->final_norm || !m->output)) return fail(MI_ERR_ARG, "%s: logits on a rank without LM head", entry);
  if (bt->seq_adapter && m->lora_rank <= 0) return fail(MI_ERR_ARG, "%s: seq_adapter on a model without un-merged LoRA (lora_rank 0)", entry);
  return MI_OK;
}
// The checks behind it: the entry's carved size against the caller's, then the sample request.
int check_workspace_and_sample(const char* entry, const mi_batch_t* bt, size_t required, BatchInfo* info) {
  if (required > bt->workspace_bytes) return fail(MI_ERR_WORKSPACE, "workspace %zu < required %zu", bt->workspace_bytes, required);
  BatchInfo& b = *info;
  b.want_sample = b.branch == MI_BRANCH_DECODE && bt->logits && bt->greedy_token && bt->greedy_logprob;
  if (bt->greedy_token && !b.want_sample)
    return fail(MI_ERR_ARG, "%s: greedy_token needs the DECODE branch, logits and greedy_logprob", entry);
  if (b.want_sample && bt->hist_len > 0 && (!bt->hist_token || !bt->hist_logprob))
    return fail(MI_ERR_ARG, "%s: hist_len > 0 without history buffers", entry);
  b.want_topp = b.want_sample && bt->sample_temperature > 0.f;
  if (bt->sample_temperature < 0.f || (b.want_topp && !(bt->sample_top_p >= 0.f && bt->sample_top_p <= 1.f)))
    return fail(MI_ERR_ARG, "%s: sample_temperature %g / sample_top_p %g", entry, (double)bt->sample_temperature, (double)bt->sample_top_p);
  return MI_OK;
}

// The step's sample behind the LM head of either entry (generate.py:124-136; one block per sequence); ctrl: the control words
// of the workspace - it reads the step counter the step advanced.
int sample_step(const mi_batch_t* bt, const mi_model_t* m, bool topp, const uint32_t* ctrl, hipStream_t s) {
  if (topp)
    return hip_rc(launch_sample_top_p(bt->logits, m->vocab_size, bt->B, m->vocab_size, bt->sample_temperature, bt->sample_top_p,
                                      bt->sample_seed, bt->sample_offset, nullptr, bt->greedy_token, bt->greedy_logprob, bt->hist_token,
                                      bt->hist_logprob, bt->hist_len, ctrl, s), "top-p sample");
  return hip_rc(launch_greedy_rows(bt->logits, m->vocab_size, bt->B, m->vocab_size, bt->greedy_token, bt->greedy_logprob,
                                   bt->hist_token, bt->hist_logprob, bt->hist_len, ctrl, s), "greedy sample");
}

bool dtype_ok(int dtype) { return dtype == G_DT_BF16 || dtype == G_DT_FP16 || dtype == G_DT_FP32; }

int check_model(const mi_model_t* m) {
  if (!m || !m->layers) return fail(MI_ERR_ARG, "null model");
  if (m->head_dim != 128) return fail(MI_ERR_SHAPE, "head_dim %d: kernels are built for 128", m->head_dim);
  if (m->n_heads % m->n_kv_heads) return fail(MI_ERR_SHAPE, "n_heads %% n_kv_heads != 0");
  if (m->dim % 8 || m->hidden_dim % 8) return fail(MI_ERR_SHAPE, "dim/hidden_dim must be multiples of 8");
  if (m->dim > 16384) return fail(MI_ERR_SHAPE, "dim > 16384");
  if (m->num_experts > 16 || m->top_k > 4 || (m->top_k == 3)) return fail(MI_ERR_SHAPE, "MoE: E <= 16, top_k in {1,2,4}");
  if (m->num_experts > 0 && (size_t)m->top_k * m->hidden_dim * 2 > 65536)
    return fail(MI_ERR_SHAPE, "MoE: top_k * hidden_dim too large for the decode combine kernel");
  if (m->lora_rank < 0 || (m->lora_rank > 0 && !lora_rank_ok(m->lora_rank)))
    return fail(MI_ERR_SHAPE, "LoRA rank %d: the kernels take multiples of 8 up to 64", m->lora_rank);
  if (m->lora_rank > 0 && m->num_experts > 0)
    return fail(MI_ERR_UNSUPPORTED, "un-merged LoRA on a MoE model is not implemented (adapters inside the experts); merge the adapter");
  if (m->lora_rank > 0 && !(m->lora_scaling > 0.f)) return fail(MI_ERR_ARG, "lora_scaling %g must be > 0 (lora.py:19)", (double)m->lora_scaling);
  if (m->lora_slots < 0 || (m->lora_slots > 1 && m->lora_rank == 0))
    return fail(MI_ERR_ARG, "lora_slots %d: an adapter bank needs lora_rank > 0 and at least one slot", m->lora_slots);
  return MI_OK;
}

}  // namespace

// mi_qkv_rope_kvwrite and its _w8 / _w4 forms (PlainBf16: no scales, D a multiple of 8)
template <class Q>
static int qkv_rope_kvwrite(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                            const typename Q::scale_t* sq, const typename Q::scale_t* sk, const typename Q::scale_t* sv, int n_heads,
                            int n_kv_heads, int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                            const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k, void* cache_v, int W, int kv_layout,
                            mi_stream_t stream) {
  const char* me = Q::kQkv;
  constexpr bool quant = Q::kFormat != 0;
  if (!qkv || !x || !wq || !wk || !wv || (quant ? (!sq || !sk || !sv) : D % 8 != 0) || !rope_cs || !tok_pos || T <= 0 || D <= 0 ||
      rope_len <= 0 || !kv_layout_ok(kv_layout))
    return fail(MI_ERR_ARG, "%s", me);
  if constexpr (quant)
    if (D % Q::kMod) return fail(MI_ERR_SHAPE, "%s: D = %d must be a multiple of %d (%s)", me, D, Q::kMod, Q::kWhy);
  if (head_dim != 128) return fail(MI_ERR_SHAPE, "head_dim must be 128");
  if ((cache_k == nullptr) != (cache_v == nullptr) || (cache_k && W <= 0)) return fail(MI_ERR_ARG, "%s: cache", me);
  if (T > GEMV_MAX_T)
    return fail(MI_ERR_UNSUPPORTED, "%s: T = %d > %d (the prefill path is mi_rmsnorm + %s + mi_rope_inplace + mi_kv_write)", me, T, GEMV_MAX_T,
                Q::kLinear);
  // rings of e4m3 bytes: an e4m3 store in the GEMV epilogue would change every GEMV kernel, so the GEMV runs without its fused write
  // and the k | v columns of its output go through the e4m3 ring-write kernel - every row to the slot the fused write picks
  const RingWrite ring = {cache_k, cache_v, W, kv_layout};
  LinearGroup g = group_of(D, wq, n_heads * head_dim, wk, n_kv_heads * head_dim, wv, n_kv_heads * head_dim);
  if constexpr (quant) set_scales(g, Q{}, sq, sk, sv);
  LinearCall c = {x, ldx, norm_w, eps, qkv, ldo, nullptr, EPI_QKV_ROPE, rope_cs, tok_pos, tok_seq, head_dim, cache_k ? &ring : nullptr};
  c.what = {Q::kQkvGemv, nullptr, nullptr, nullptr, "kv_write (e4m3)"};
  return linear_group(g, c, T, (hipStream_t)stream);
}

extern "C" {

int mi_abi_version(void) { return MI_ABI_VERSION; }

const char* mi_last_error_detail(void) { return g_detail; }

const char* mi_error_string(int code) {
  switch (code) {
    case MI_OK: return "ok";
    case MI_ERR_ARG: return "invalid argument";
    case MI_ERR_SHAPE: return "shape not supported by the gfx950 kernels";
    case MI_ERR_WORKSPACE: return "workspace too small";
    case MI_ERR_UNSUPPORTED: return "unsupported";
    case MI_ERR_RCCL: return "RCCL call failed (see mi_rccl_last_error)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int mi_embedding(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, mi_stream_t stream) {
  if (!out || !table || !ids || T <= 0 || D <= 0 || D % 8) return fail(MI_ERR_ARG, "mi_embedding");
  return hip_rc(launch_embedding(out, table, ids, T, D, vocab, nullptr, (hipStream_t)stream), "embedding");
}

int mi_rmsnorm(void* out, const void* x, const void* w, int T, int D, float eps, mi_stream_t stream) {
  if (!out || !x || !w || T <= 0 || D <= 0 || D % 8) return fail(MI_ERR_ARG, "mi_rmsnorm");
  return hip_rc(launch_rmsnorm(out, x, w, T, D, eps, (hipStream_t)stream), "rmsnorm");
}

int mi_rope_inplace(void* qkv, int ld, int T, int n_heads, int n_kv_heads, int head_dim, const float* rope_cs,
                    int rope_len, const int32_t* tok_pos, mi_stream_t stream) {
  if (!qkv || !rope_cs || !tok_pos || T <= 0 || head_dim % 8 || rope_len <= 0) return fail(MI_ERR_ARG, "mi_rope_inplace");
  return hip_rc(launch_rope(qkv, ld, T, n_heads, n_kv_heads, head_dim, rope_cs, tok_pos, (hipStream_t)stream), "rope");
}

int mi_kv_write(void* cache_k, void* cache_v, int W, const void* k, const void* v, int ld, int T, int kv_dim,
                const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_start, int kv_layout, int head_dim,
                mi_stream_t stream) {
  if (!cache_k || !cache_v || !k || !v || !tok_seq || !tok_pos || !q_start || W <= 0 || T <= 0 || kv_dim % 8)
    return fail(MI_ERR_ARG, "mi_kv_write");
  if (!kv_layout_ok(kv_layout) || head_dim <= 0 || head_dim % 8 || kv_dim % head_dim) return fail(MI_ERR_ARG, "mi_kv_write: layout / head_dim");
  return hip_rc(launch_kv_write(cache_k, cache_v, W, k, v, ld, T, kv_dim, tok_seq, tok_pos, q_start, kv_layout, head_dim,
                                (hipStream_t)stream), "kv_write");
}

int mi_kv_dequant(void* dst_k, void* dst_v, const void* src_k, const void* src_v, int W, int B, int n_kv_heads, int head_dim,
                  int kv_layout, mi_stream_t stream) {
  if (!dst_k || !dst_v || !src_k || !src_v || W <= 0 || B <= 0 || n_kv_heads <= 0 || head_dim <= 0 || !kv_layout_ok(kv_layout))
    return fail(MI_ERR_ARG, "mi_kv_dequant");
  const size_t n = (size_t)B * W * n_kv_heads * head_dim;
  if (n % 16) return fail(MI_ERR_SHAPE, "mi_kv_dequant: %zu elements per ring, not a multiple of 16", n);
  return hip_rc(launch_kv_dequant(dst_k, dst_v, src_k, src_v, n, (hipStream_t)stream), "kv_dequant");
}

int mi_linear(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
              int epilogue, const void* residual, const void* norm_w, float eps, mi_stream_t stream) {
  if (!out || !x || !w || !n_rows || !w[0] || M <= 0 || K <= 0 || K % 8) return fail(MI_ERR_ARG, "mi_linear");
  if (epilogue == MI_EPI_RESIDUAL && !residual) return fail(MI_ERR_ARG, "mi_linear: residual epilogue without residual");
  if (epilogue == MI_EPI_SWIGLU && (!w[1] || n_rows[0] != n_rows[1])) return fail(MI_ERR_ARG, "mi_linear: swiglu needs W1, W3");
  if (norm_w && M > GEMV_MAX_T) return fail(MI_ERR_UNSUPPORTED, "mi_linear: fused RMSNorm only on the M <= 8 path");
  const LinearGroup g = group_of(K, w[0], n_rows[0], w[1], n_rows[1], w[2], n_rows[2]);
  // (any code but the three: LOGITS, as ever - and the internal EPI_QKV_ROPE is out of a caller's reach)
  const int epi = (epilogue == MI_EPI_STORE || epilogue == MI_EPI_RESIDUAL || epilogue == MI_EPI_SWIGLU) ? epilogue : MI_EPI_LOGITS;
  LinearCall c = {x, ldx, norm_w, eps, out, ldo, residual, epi};
  c.what = {"gemv", "gemm"};
  return linear_group(g, c, M, (hipStream_t)stream);
}

/* lora.py:71-74 */
size_t mi_lora_linear_scratch_bytes(int M, int K, const int n_rows[3], int epilogue, int rank, int fused_norm) {
  if (M <= 0 || K <= 0 || !n_rows || !lora_rank_ok(rank)) return 0;
  const LoraShape sh = lora_shape(n_rows, epilogue, fused_norm != 0);
  if (sh.nseg == 0) return 0;
  return lora_carve(M, K, sh.n_total, sh.nseg, rank, sh.base_f32, fused_norm != 0, nullptr).total;
}

/* lora.py:71-74; slots / row_slot: the adapter bank of mi_lora_linear_slots (1 / NULL: one adapter set) */
static int lora_linear_leaf(const char* entry, void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3],
                            const int n_rows[3], int epilogue, const void* residual, const void* norm_w, float eps,
                            const void* const A[3], const void* const B[3], int rank, float scaling, int slots, const int32_t* row_slot,
                            void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  if (!out || !x || !w || !n_rows || !w[0] || !A || !B || !scratch || M <= 0 || K <= 0 || K % 8 || ldx % 8 || n_rows[0] <= 0)
    return fail(MI_ERR_ARG, "%s", entry);
  if (epilogue != MI_EPI_STORE && epilogue != MI_EPI_RESIDUAL && epilogue != MI_EPI_SWIGLU)
    return fail(MI_ERR_ARG, "%s: epilogue %d (store, residual and swiglu carry adapters; the LM head has none)", entry, epilogue);
  if (epilogue == MI_EPI_RESIDUAL && !residual) return fail(MI_ERR_ARG, "%s: residual epilogue without residual", entry);
  if (epilogue == MI_EPI_SWIGLU && (!w[1] || n_rows[0] != n_rows[1])) return fail(MI_ERR_ARG, "%s: swiglu needs W1, W3", entry);
  if (!lora_rank_ok(rank)) return fail(MI_ERR_SHAPE, "%s: LoRA rank %d: the kernels take multiples of 8 up to 64", entry, rank);
  if (!(scaling > 0.f)) return fail(MI_ERR_ARG, "%s: scaling %g must be > 0 (lora.py:19)", entry, (double)scaling);
  if (norm_w && M > GEMV_MAX_T) return fail(MI_ERR_UNSUPPORTED, "%s: fused RMSNorm only on the M <= 8 path", entry);
  const LoraShape sh = lora_shape(n_rows, epilogue, norm_w != nullptr);
  LinearGroup g = group_of(K, nullptr, 0);  // filled by hand: each segment is checked before it is taken, and the messages are pinned
  g.nseg = sh.nseg; g.rank = rank; g.scaling = scaling;
  if (slots < 1) return fail(MI_ERR_ARG, "%s: slots %d", entry, slots);
  g.bank = lora_bank(slots, nullptr, row_slot);  // (tok_seq == nullptr: row m is its own sequence)
  for (int i = 0; i < sh.nseg; ++i) {
    if (!w[i]) return fail(MI_ERR_ARG, "%s: n_rows[%d] without a weight", entry, i);
    if ((A[i] == nullptr) != (B[i] == nullptr)) return fail(MI_ERR_ARG, "%s: adapter %d needs both A and B (or neither)", entry, i);
    g.w[i] = w[i]; g.A[i] = A[i]; g.B[i] = B[i]; g.n_rows[i] = epilogue == MI_EPI_SWIGLU ? n_rows[0] : n_rows[i];
  }
  const LoraScratch sc = lora_carve(M, K, sh.n_total, sh.nseg, rank, sh.base_f32, norm_w != nullptr, (char*)scratch);
  if (sc.total > scratch_bytes) return fail(MI_ERR_WORKSPACE, "%s: scratch %zu < required %zu", entry, scratch_bytes, sc.total);
  LinearCall c = {x, ldx, norm_w, eps, out, ldo, residual, epilogue};
  c.xn = sc.xn; c.lora_base = sc.base; c.lora_t = sc.t; c.lora_base_f32 = sh.base_f32; c.what.norm = "lora rmsnorm";
  return linear_group(g, c, M, (hipStream_t)stream);
}

/* lora.py:71-74 */
int mi_lora_linear(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const void* const A[3],
                   const void* const B[3], int rank, float scaling, void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  return lora_linear_leaf("mi_lora_linear", out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, A, B, rank, scaling, 1,
                          nullptr, scratch, scratch_bytes, stream);
}

/* lora.py:71-74, one adapter per row out of a bank of `slots` */
int mi_lora_linear_slots(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                         int epilogue, const void* residual, const void* norm_w, float eps, const void* const A[3],
                         const void* const B[3], int rank, float scaling, int slots, const int32_t* row_slot, void* scratch,
                         size_t scratch_bytes, mi_stream_t stream) {
  return lora_linear_leaf("mi_lora_linear_slots", out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, A, B, rank,
                          scaling, slots, row_slot, scratch, scratch_bytes, stream);
}

namespace {
constexpr int LOGPROB_ROW_CHUNK = 128;  // rows per pass of the unfused route (bounds its scratch)
MoeScratch moe_carve(int T, int D, int F, int E, int top_k, char* base) {
  MoeScratch w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  const size_t rows = (size_t)T * top_k;
  w.hid = (bf16_t*)take(rows * F * 2);
  w.y = (bf16_t*)take(rows * D * 2);
  w.tok_of = (int32_t*)take(rows * 4);
  w.row_of = (int32_t*)take(rows * 4);
  w.max_tiles = (int)((rows + 127) / 128) + E;
  w.tile_tab = (int32_t*)take((size_t)w.max_tiles * 16);
  w.n_tiles = (int32_t*)take(256);
  w.total = off;
  return w;
}
}

size_t mi_lm_head_logprobs_scratch_bytes(int M, int vocab) {
  if (M <= 0 || vocab <= 0) return 0;
  const size_t n_tiles = (size_t)(vocab + 255) / 256;
  const size_t fused = align_up((size_t)M * n_tiles * sizeof(float2)) + align_up((size_t)M * sizeof(float));
  const size_t rows = (size_t)(M < LOGPROB_ROW_CHUNK ? M : LOGPROB_ROW_CHUNK) * vocab * sizeof(float);
  return fused > rows ? fused : rows;  // either route may be taken (the fused one needs M >= 256 and K % 64 == 0)
}

// mi_lm_head_logprobs, and mi_lm_head_logprobs_q on a quantised head (head.format != 0: deq holds a slice of its bf16 image).
// The arguments have been checked; scratch: mi_lm_head_logprobs_scratch_bytes.
static int lm_head_logprobs(float* logprob, const void* x, int ldx, int M, int K, const LinearGroup& head, const int32_t* target, void* scratch,
                            bf16_t* deq, hipStream_t s) {
  const int vocab = head.n_rows[0];
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.epi = GEMM_LOGPROB; g.M = M; g.N = vocab; g.K = K; g.a = (const bf16_t*)x; g.lda = ldx;
  g.w0 = (const bf16_t*)head.w[0]; g.n0 = g.n1 = vocab;
  if (M >= 256 && gemm256_applicable(g)) {
    // one pass over the LM head: per-tile (max, sum-exp) partials + the target logit, then one wave per row
    const int n_tiles = (vocab + 255) / 256;
    g.lp_target = target;
    g.lp_partial = (float2*)scratch;
    g.lp_tgt = (float*)((char*)scratch + align_up((size_t)M * n_tiles * sizeof(float2)));
    MI_TRY(hip_rc(hipMemsetAsync(g.lp_tgt, 0, (size_t)M * sizeof(float), s), "logprob target memset"));
    if (head.format) MI_TRY(head_gemm_sliced(head, g, deq, s, "dequant lm head", "lm head logprob gemm"));
    else MI_TRY(hip_rc(launch_gemm256(g, s), "lm head logprob gemm"));
    return hip_rc(launch_logprob_finalize(logprob, g.lp_partial, g.lp_tgt, M, n_tiles, s), "logprob finalize");
  }
  // few rows (or a K the 256-tile kernel does not take): fp32 logits of up to 128 rows at a time into the scratch
  // (GEMV / 128-tile GEMM), then a row-wise log-softmax gather
  for (int r0 = 0; r0 < M; r0 += LOGPROB_ROW_CHUNK) {
    const int rows = (M - r0 < LOGPROB_ROW_CHUNK) ? M - r0 : LOGPROB_ROW_CHUNK;
    LinearCall c = {(const bf16_t*)x + (size_t)r0 * ldx, ldx, nullptr, 0.f, scratch, vocab, nullptr, MI_EPI_LOGITS};
    c.deq = deq;
    c.what = {"gemv", "gemm", "dequant lm head"};
    MI_TRY(linear_group(head, c, rows, s));
    MI_TRY(hip_rc(launch_logprob_rows(logprob + r0, (const float*)scratch, vocab, target + r0, rows, vocab, s), "logprob rows"));
  }
  return MI_OK;
}

int mi_lm_head_logprobs(float* logprob, const void* x, int ldx, int M, int K, const void* w, int vocab,
                        const int32_t* target, void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  if (!logprob || !x || !w || !target || !scratch || M <= 0 || K <= 0 || K % 8 || vocab <= 0)
    return fail(MI_ERR_ARG, "mi_lm_head_logprobs");
  if (scratch_bytes < mi_lm_head_logprobs_scratch_bytes(M, vocab))
    return fail(MI_ERR_WORKSPACE, "mi_lm_head_logprobs: scratch %zu < required %zu", scratch_bytes,
                mi_lm_head_logprobs_scratch_bytes(M, vocab));
  return lm_head_logprobs(logprob, x, ldx, M, K, group_of(K, w, vocab), target, scratch, nullptr, (hipStream_t)stream);
}

/* a quantised LM head as leaves (include/mistral_hip.h: mi_lm_head_quant_t) */
static int check_head_quant(const char* me, const mi_lm_head_quant_t* head, int K, LinearGroup* g) {
  if (!head || !head->scale) return fail(MI_ERR_ARG, "%s: head (format and scales)", me);
  if (head->format != MI_W8_FP8_E4M3 && head->format != MI_W4_MXFP4)
    return fail(MI_ERR_UNSUPPORTED, "%s: LM head format %d (MI_W8_FP8_E4M3 = 1 and MI_W4_MXFP4 = 2 are the formats)", me, head->format);
  return with_format(head->format, [&](auto Q) {
    typedef decltype(Q) F;
    if (K % F::kMod) return fail(MI_ERR_SHAPE, "%s: K = %d must be a multiple of %d (%s)", me, K, F::kMod, F::kWhy);
    set_scales(*g, Q, (const typename F::scale_t*)head->scale);
    return (int)MI_OK;
  });
}

size_t mi_lm_head_q_scratch_bytes(int M, int K, int vocab) {
  if (M <= GEMV_MAX_T || K <= 0 || vocab <= 0) return 0;
  return align_up(lm_head_slice_bytes(vocab, K));
}

int mi_lm_head_q(float* logits, int ldo, const void* x, int ldx, int M, int K, const void* w, int vocab, const mi_lm_head_quant_t* head,
                 const void* norm_w, float eps, void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  const char* me = "mi_lm_head_q";
  if (!logits || !x || !w || M <= 0 || K <= 0 || vocab <= 0 || ldo < vocab) return fail(MI_ERR_ARG, "%s", me);
  LinearGroup g = group_of(K, w, vocab);
  MI_TRY(check_head_quant(me, head, K, &g));
  if (M > GEMV_MAX_T) {
    if (norm_w) return fail(MI_ERR_UNSUPPORTED, "%s: fused RMSNorm only on the M <= 8 path", me);
    const size_t need = mi_lm_head_q_scratch_bytes(M, K, vocab);
    if (!scratch || scratch_bytes < need) return fail(MI_ERR_WORKSPACE, "%s: scratch %zu < required %zu", me, scratch ? scratch_bytes : (size_t)0, need);
  }
  LinearCall c = {x, ldx, norm_w, eps, logits, ldo, nullptr, MI_EPI_LOGITS};
  c.deq = (bf16_t*)scratch;
  c.what = {"lm head gemv", "lm head gemm", "dequant lm head"};
  return linear_group(g, c, M, (hipStream_t)stream);
}

size_t mi_lm_head_logprobs_q_scratch_bytes(int M, int K, int vocab) {
  if (M <= 0 || K <= 0 || vocab <= 0) return 0;
  return align_up(mi_lm_head_logprobs_scratch_bytes(M, vocab)) + mi_lm_head_q_scratch_bytes(M, K, vocab);
}

int mi_lm_head_logprobs_q(float* logprob, const void* x, int ldx, int M, int K, const void* w, int vocab, const mi_lm_head_quant_t* head,
                          const int32_t* target, void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  const char* me = "mi_lm_head_logprobs_q";
  if (!logprob || !x || !w || !target || !scratch || M <= 0 || K <= 0 || vocab <= 0) return fail(MI_ERR_ARG, "%s", me);
  LinearGroup g = group_of(K, w, vocab);
  MI_TRY(check_head_quant(me, head, K, &g));
  const size_t need = mi_lm_head_logprobs_q_scratch_bytes(M, K, vocab);
  if (scratch_bytes < need) return fail(MI_ERR_WORKSPACE, "%s: scratch %zu < required %zu", me, scratch_bytes, need);
  bf16_t* deq = (bf16_t*)((char*)scratch + align_up(mi_lm_head_logprobs_scratch_bytes(M, vocab)));
  return lm_head_logprobs(logprob, x, ldx, M, K, g, target, scratch, M > GEMV_MAX_T ? deq : nullptr, (hipStream_t)stream);
}

size_t mi_attn_decode_scratch_bytes(int B, int n_heads, int n_kv_heads, int head_dim, int W) {
  return TICKET_BYTES + align_up(attn_decode_partial_floats(B, n_heads, n_kv_heads, head_dim, W) * sizeof(float));
}

int mi_attn_decode(void* out, const void* q, int ldq, const void* cache_k, const void* cache_v, int W, int B,
                   int n_heads, int n_kv_heads, int head_dim, const int32_t* tok_pos, void* scratch, int kv_layout,
                   mi_stream_t stream) {
  if (!out || !q || !cache_k || !cache_v || !tok_pos || !scratch || W <= 0 || B <= 0 || !kv_layout_ok(kv_layout))
    return fail(MI_ERR_ARG, "mi_attn_decode");
  if (head_dim != 128) return fail(MI_ERR_SHAPE, "head_dim must be 128");
  if ((size_t)B * n_kv_heads * 4 > TICKET_BYTES) return fail(MI_ERR_SHAPE, "B * n_kv_heads > 1024");
  const AttnDecodeArgs a = attn_decode_args(out, q, ldq, cache_k, cache_v, kv_layout, W, B, n_heads, n_kv_heads, head_dim, tok_pos,
                                            (int32_t*)scratch, (float*)((char*)scratch + TICKET_BYTES));
  return hip_rc(launch_attn_decode(a, (hipStream_t)stream), "attn_decode");
}

int mi_attn_prefill(void* out, const void* qkv, int ld, const void* cache_k, const void* cache_v, int W, int B,
                    int max_q_len, int n_heads, int n_kv_heads, int head_dim, const int32_t* q_start,
                    const int32_t* kv_before, int causal, float softmax_scale, int kv_layout, mi_stream_t stream) {
  if (!out || !qkv || B <= 0 || max_q_len <= 0 || W <= 0 || !kv_layout_ok(kv_layout)) return fail(MI_ERR_ARG, "mi_attn_prefill");
  if (causal && (!q_start || !kv_before)) return fail(MI_ERR_ARG, "mi_attn_prefill: metadata");
  if (kv_e4m3(kv_layout))
    return fail(MI_ERR_UNSUPPORTED, "mi_attn_prefill: rings of e4m3 bytes (MI_KV_E4M3) are not read here; mi_kv_dequant them into bf16 rings first");
  if (head_dim != 128) return fail(MI_ERR_SHAPE, "head_dim must be 128");
  // the kernel forms 32-bit element offsets inside one ring (W * kv_dim) and inside the activation matrix (rows * ld)
  if ((size_t)W * n_kv_heads * head_dim >= (1ull << 31) || (size_t)B * max_q_len * (size_t)ld >= (1ull << 31))
    return fail(MI_ERR_UNSUPPORTED, "mi_attn_prefill: ring or activation matrix larger than 2^31 elements");
  const AttnPrefillArgs a = attn_prefill_args(out, qkv, ld, cache_k, cache_v, kv_layout, W, B, max_q_len, n_heads, n_kv_heads, head_dim,
                                              q_start, kv_before, causal, softmax_scale);
  return hip_rc(launch_attn_prefill(a, (hipStream_t)stream), "attn_prefill");
}

size_t mi_attn_verify_scratch_bytes(int T, int n_heads, int head_dim, int W) {
  if (T <= 0 || n_heads <= 0 || W <= 0) return 0;
  return align_up(attn_verify_partial_floats(T, n_heads, head_dim, W) * sizeof(float));
}

int mi_attn_verify(void* out, const void* qkv, int ld, const void* cache_k, const void* cache_v, int W, int T, int B, int n_heads,
                   int n_kv_heads, int head_dim, const int32_t* q_start, const int32_t* kv_before, void* scratch, int kv_layout,
                   mi_stream_t stream) {
  if (!out || !qkv || !cache_k || !cache_v || !q_start || !kv_before || !scratch || W <= 0 || T <= 0 || B <= 0 || n_heads <= 0 ||
      n_kv_heads <= 0 || !kv_layout_ok(kv_layout))
    return fail(MI_ERR_ARG, "mi_attn_verify");
  if (kv_e4m3(kv_layout)) return fail(MI_ERR_UNSUPPORTED, "mi_attn_verify: rings of e4m3 bytes (MI_KV_E4M3) are not implemented");
  if (head_dim != 128) return fail(MI_ERR_SHAPE, "mi_attn_verify: head_dim must be 128");
  if (n_heads % n_kv_heads) return fail(MI_ERR_SHAPE, "mi_attn_verify: n_heads %% n_kv_heads != 0");
  if (T > GEMV_MAX_T) return fail(MI_ERR_UNSUPPORTED, "mi_attn_verify: T = %d rows; a verify step takes at most %d", T, GEMV_MAX_T);
  if (B > T) return fail(MI_ERR_ARG, "mi_attn_verify: every sequence brings m_b >= 1 rows (T %d, B %d)", T, B);
  if (ld < (n_heads + 2 * n_kv_heads) * head_dim) return fail(MI_ERR_ARG, "mi_attn_verify: ld %d below the q | k | v columns", ld);
  if (attn_verify_splits(W) > 32) return fail(MI_ERR_UNSUPPORTED, "mi_attn_verify: a ring of %d slots; the verify attention takes 1 .. 4096", W);
  AttnVerifyArgs a = {};
  a.out = out; a.qkv = (const bf16_t*)qkv; a.ld = ld; a.cache_k = (const bf16_t*)cache_k; a.cache_v = (const bf16_t*)cache_v;
  a.kv_layout = kv_layout; a.W = W; a.T = T; a.B = B; a.H = n_heads; a.Hkv = n_kv_heads; a.Dh = head_dim;
  a.q_start = q_start; a.kv_before = kv_before; a.partial = (float*)scratch; a.stash = nullptr;
  return hip_rc(launch_attn_verify(a, (hipStream_t)stream), "attn_verify");
}

int mi_gelu(void* x, int ldx, int T, int N, mi_stream_t stream) {
  if (!x || T <= 0 || N <= 0 || ldx < N) return fail(MI_ERR_ARG, "mi_gelu");
  return hip_rc(launch_gelu(x, ldx, T, N, (hipStream_t)stream), "gelu");
}

int mi_moe_router(int32_t* sel_idx, float* sel_w, const void* x, int ldx, int T, int D, const void* gate, int E,
                  int top_k, const void* norm_w, float eps, mi_stream_t stream) {
  if (!sel_idx || !sel_w || !x || !gate || T <= 0 || D % 8) return fail(MI_ERR_ARG, "mi_moe_router");
  if (E > 16 || top_k > 4 || top_k > E || top_k < 1) return fail(MI_ERR_SHAPE, "router: E <= 16, top_k <= 4");
  return hip_rc(launch_moe_router(sel_idx, sel_w, x, ldx, T, D, gate, E, top_k, norm_w, eps, (hipStream_t)stream), "moe_router");
}

int mi_qkv_rope_kvwrite(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                        const void* wv, int n_heads, int n_kv_heads, int head_dim, const void* norm_w, float eps,
                        const float* rope_cs, int rope_len, const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k,
                        void* cache_v, int W, int kv_layout, mi_stream_t stream) {
  return qkv_rope_kvwrite<PlainBf16>(qkv, ldo, x, ldx, T, D, wq, wk, wv, nullptr, nullptr, nullptr, n_heads, n_kv_heads, head_dim, norm_w, eps,
                                     rope_cs, rope_len, tok_pos, tok_seq, cache_k, cache_v, W, kv_layout, stream);
}

/* weight-only FP8 leaves (include/mistral_hip.h: MI_W8_FP8_E4M3) */
static size_t linear_w8_rows(const int n_rows[3], const void* const w[3], int epilogue) {
  if (epilogue == MI_EPI_SWIGLU) return 2 * (size_t)n_rows[0];
  size_t n = 0;
  for (int i = 0; i < 3 && (i == 0 || !w || w[i]); ++i) n += n_rows[i] > 0 ? n_rows[i] : 0;
  return n;
}
size_t mi_linear_w8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue) {
  if (M <= GEMV_MAX_T || K <= 0 || !n_rows) return 0;
  return align_up(linear_w8_rows(n_rows, nullptr, epilogue) * (size_t)K * 2);
}

}  // extern "C"

static size_t w8a8_scratch_bytes(int M, int K) { return align_up((size_t)M * K) + align_up((size_t)M * sizeof(float)); }  // x_q | s_x

// mi_linear_w8 / mi_linear_w4; a8 (mi_linear_w8a8 / mi_linear_w4a8): the format's FP8-activation GEMM where it applies, whose scratch is x_q | s_x
template <class Q>
static int linear_quant(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3], int epilogue,
                        const void* residual, const void* norm_w, float eps, const typename Q::scale_t* const scale[3], void* scratch,
                        size_t scratch_bytes, mi_stream_t stream, bool a8 = false) {
  const char* me = a8 ? Q::kLinearA8 : Q::kLinear;
  if (!out || !x || !w || !n_rows || !scale || !w[0] || !scale[0] || M <= 0 || K <= 0 || n_rows[0] <= 0) return fail(MI_ERR_ARG, "%s", me);
  for (int i = 1; i < 3; ++i)
    if (w[i] && (!scale[i] || n_rows[i] <= 0 || !w[i - 1])) return fail(MI_ERR_ARG, "%s: segment %d needs rows, a scale and its predecessor", me, i);
  if (K % Q::kMod) return fail(MI_ERR_SHAPE, "%s: K = %d must be a multiple of %d (%s)", me, K, Q::kMod, Q::kWhy);
  if (epilogue != MI_EPI_STORE && epilogue != MI_EPI_RESIDUAL && epilogue != MI_EPI_SWIGLU)
    return fail(MI_ERR_UNSUPPORTED, "%s: epilogue %d (store, residual and swiglu; the LM head is not quantised)", me, epilogue);
  if (epilogue == MI_EPI_RESIDUAL && !residual) return fail(MI_ERR_ARG, "%s: residual epilogue without residual", me);
  if (epilogue == MI_EPI_SWIGLU && (!w[1] || n_rows[0] != n_rows[1])) return fail(MI_ERR_ARG, "%s: swiglu needs W1, W3", me);
  const bool swiglu = epilogue == MI_EPI_SWIGLU;  // (W1 | W3: a third segment is not read)
  LinearGroup g = group_of(K, w[0], n_rows[0], w[1], w[1] ? n_rows[1] : 0, swiglu ? nullptr : w[2], (!swiglu && w[2]) ? n_rows[2] : 0);
  set_scales(g, Q{}, scale[0], w[1] ? scale[1] : nullptr, (!swiglu && w[2]) ? scale[2] : nullptr);
  // (outside the route's shape the leaf is mi_linear_w8; inside it linear_group still takes the weight-only route for operands the
  // 16-byte accesses cannot read, so the scratch is sized for either: mi_linear_w8a8_scratch_bytes)
  a8 = a8 && a8_applicable(Q::kFormat, M, K);
  if (M > GEMV_MAX_T) {
    if (norm_w && !(a8 && a8_operands_ok(g, x, ldx))) return fail(MI_ERR_UNSUPPORTED, "%s: fused RMSNorm only on the M <= 8 path", me);
    size_t need = align_up((size_t)(g.n_rows[0] + g.n_rows[1] + g.n_rows[2]) * K * 2);
    if (a8 && need < w8a8_scratch_bytes(M, K)) need = w8a8_scratch_bytes(M, K);
    if (!scratch || scratch_bytes < need) return fail(MI_ERR_WORKSPACE, "%s: scratch %zu < required %zu", me, scratch ? scratch_bytes : (size_t)0, need);
  }
  LinearCall c = {x, ldx, norm_w, eps, out, ldo, residual, epilogue};
  if (a8) {
    c.a8 = true; c.x_q = (uint8_t*)scratch; c.s_x = (float*)((char*)scratch + align_up((size_t)M * K));
  }
  c.deq = (bf16_t*)scratch;
  c.what = {Q::kGemv, "gemm", Q::kDequant};
  return linear_group(g, c, M, (hipStream_t)stream);
}

// mi_qkv_rope_w8a8 / mi_qkv_rope_w4a8
template <class Q>
static int qkv_rope_a8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                       const typename Q::scale_t* sq, const typename Q::scale_t* sk, const typename Q::scale_t* sv, int n_heads,
                       int n_kv_heads, int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                       const int32_t* tok_pos, void* scratch, size_t scratch_bytes, mi_stream_t stream) {
  const char* me = Q::kQkvA8;
  if (!qkv || !x || !wq || !wk || !wv || !sq || !sk || !sv || !rope_cs || !tok_pos || T <= 0 || D <= 0 || rope_len <= 0 || n_heads <= 0 ||
      n_kv_heads <= 0)
    return fail(MI_ERR_ARG, "%s", me);
  if (head_dim != 128) return fail(MI_ERR_SHAPE, "head_dim must be 128");
  LinearGroup g = group_of(D, wq, n_heads * head_dim, wk, n_kv_heads * head_dim, wv, n_kv_heads * head_dim);
  set_scales(g, Q{}, sq, sk, sv);
  if (!a8_applicable(Q::kFormat, T, D) || !a8_operands_ok(g, x, ldx))
    return fail(MI_ERR_UNSUPPORTED, "%s: T = %d, D = %d, ldx = %d (this leaf is the %s only: T >= 256, D %% 128 == 0, D <= 16384, "
                "ldx %% 8 == 0, %s; fewer rows are %s's)", me, T, D, ldx, Q::kGemmA8, Q::kOperandsA8, Q::kPrior);
  const size_t need = w8a8_scratch_bytes(T, D);
  if (!scratch || scratch_bytes < need) return fail(MI_ERR_WORKSPACE, "%s: scratch %zu < required %zu", me, scratch ? scratch_bytes : (size_t)0, need);
  LinearCall c = {x, ldx, norm_w, eps, qkv, ldo, nullptr, EPI_QKV_ROPE, rope_cs, tok_pos, nullptr, head_dim, nullptr};
  c.a8 = true; c.x_q = (uint8_t*)scratch; c.s_x = (float*)((char*)scratch + align_up((size_t)T * D));
  c.what = {Q::kQkvGemv, "qkv gemm", "dequant q|k|v", "attention_norm"};
  return linear_group(g, c, T, (hipStream_t)stream);
}

extern "C" {

int mi_linear_w8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                 int epilogue, const void* residual, const void* norm_w, float eps, const float* const scale[3], void* scratch,
                 size_t scratch_bytes, mi_stream_t stream) {
  return linear_quant<QuantW8>(out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, scale, scratch, scratch_bytes, stream);
}

int mi_qkv_rope_kvwrite_w8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                           const void* wv, const float* sq, const float* sk, const float* sv, int n_heads, int n_kv_heads,
                           int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                           const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k, void* cache_v, int W, int kv_layout,
                           mi_stream_t stream) {
  return qkv_rope_kvwrite<QuantW8>(qkv, ldo, x, ldx, T, D, wq, wk, wv, sq, sk, sv, n_heads, n_kv_heads, head_dim, norm_w, eps, rope_cs,
                                   rope_len, tok_pos, tok_seq, cache_k, cache_v, W, kv_layout, stream);
}

/* FP8 prefill GEMMs (include/mistral_hip.h: W8A8) */
int mi_act_quant_e4m3(void* xq, float* sx, const void* x, int ldx, int M, int K, const void* norm_w, float eps, mi_stream_t stream) {
  if (!xq || !sx || !x || M <= 0 || K <= 0 || ldx < K) return fail(MI_ERR_ARG, "mi_act_quant_e4m3");
  if (K % 8 || ldx % 8 || K > 16384)
    return fail(MI_ERR_SHAPE, "mi_act_quant_e4m3: K = %d and ldx = %d must be multiples of 8 (16-byte loads), K at most 16384", K, ldx);
  return hip_rc(launch_act_quant_e4m3(xq, sx, x, ldx, M, K, norm_w, eps, (hipStream_t)stream), "act_quant_e4m3");
}

size_t mi_linear_w8a8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue) {
  if (M <= 0 || K <= 0 || !n_rows) return 0;
  const size_t w8 = mi_linear_w8_scratch_bytes(M, K, n_rows, epilogue);
  if (!a8_applicable(MI_W8_FP8_E4M3, M, K)) return w8;
  return w8 > w8a8_scratch_bytes(M, K) ? w8 : w8a8_scratch_bytes(M, K);  // (either route of such a call: linear_quant)
}

int mi_linear_w8a8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const float* const scale[3], void* scratch,
                   size_t scratch_bytes, mi_stream_t stream) {
  return linear_quant<QuantW8>(out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, scale, scratch, scratch_bytes, stream, true);
}

int mi_qkv_rope_w8a8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                     const float* sq, const float* sk, const float* sv, int n_heads, int n_kv_heads, int head_dim, const void* norm_w,
                     float eps, const float* rope_cs, int rope_len, const int32_t* tok_pos, void* scratch, size_t scratch_bytes,
                     mi_stream_t stream) {
  return qkv_rope_a8<QuantW8>(qkv, ldo, x, ldx, T, D, wq, wk, wv, sq, sk, sv, n_heads, n_kv_heads, head_dim, norm_w, eps, rope_cs, rope_len,
                              tok_pos, scratch, scratch_bytes, stream);
}

/* MXFP4 x FP8 prefill GEMMs (include/mistral_hip.h: W4A8) */
size_t mi_linear_w4a8_scratch_bytes(int M, int K, const int n_rows[3], int epilogue) {
  if (M <= 0 || K <= 0 || !n_rows) return 0;
  const size_t w4 = mi_linear_w4_scratch_bytes(M, K, n_rows, epilogue);
  if (!a8_applicable(MI_W4_MXFP4, M, K)) return w4;
  return w4 > w8a8_scratch_bytes(M, K) ? w4 : w8a8_scratch_bytes(M, K);  // (either route of such a call: linear_quant)
}

int mi_linear_w4a8(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                   int epilogue, const void* residual, const void* norm_w, float eps, const uint8_t* const scale[3], void* scratch,
                   size_t scratch_bytes, mi_stream_t stream) {
  return linear_quant<QuantW4>(out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, scale, scratch, scratch_bytes, stream, true);
}

int mi_qkv_rope_w4a8(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk, const void* wv,
                     const uint8_t* sq, const uint8_t* sk, const uint8_t* sv, int n_heads, int n_kv_heads, int head_dim, const void* norm_w,
                     float eps, const float* rope_cs, int rope_len, const int32_t* tok_pos, void* scratch, size_t scratch_bytes,
                     mi_stream_t stream) {
  return qkv_rope_a8<QuantW4>(qkv, ldo, x, ldx, T, D, wq, wk, wv, sq, sk, sv, n_heads, n_kv_heads, head_dim, norm_w, eps, rope_cs, rope_len,
                              tok_pos, scratch, scratch_bytes, stream);
}

/* weight-only MXFP4 leaves (include/mistral_hip.h: MI_W4_MXFP4) */
size_t mi_linear_w4_scratch_bytes(int M, int K, const int n_rows[3], int epilogue) { return mi_linear_w8_scratch_bytes(M, K, n_rows, epilogue); }

int mi_linear_w4(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                 int epilogue, const void* residual, const void* norm_w, float eps, const uint8_t* const scale[3], void* scratch,
                 size_t scratch_bytes, mi_stream_t stream) {
  return linear_quant<QuantW4>(out, ldo, x, ldx, M, K, w, n_rows, epilogue, residual, norm_w, eps, scale, scratch, scratch_bytes, stream);
}

int mi_qkv_rope_kvwrite_w4(void* qkv, int ldo, const void* x, int ldx, int T, int D, const void* wq, const void* wk,
                           const void* wv, const uint8_t* sq, const uint8_t* sk, const uint8_t* sv, int n_heads, int n_kv_heads,
                           int head_dim, const void* norm_w, float eps, const float* rope_cs, int rope_len,
                           const int32_t* tok_pos, const int32_t* tok_seq, void* cache_k, void* cache_v, int W, int kv_layout,
                           mi_stream_t stream) {
  return qkv_rope_kvwrite<QuantW4>(qkv, ldo, x, ldx, T, D, wq, wk, wv, sq, sk, sv, n_heads, n_kv_heads, head_dim, norm_w, eps, rope_cs,
                                   rope_len, tok_pos, tok_seq, cache_k, cache_v, W, kv_layout, stream);
}

int mi_moe_experts_decode(void* out, const void* residual, const void* x, int ldx, int T, int D, int F,
                          const void* const* expert_w_dev, const int32_t* sel_idx, const float* sel_w, int top_k,
                          const void* norm_w, float eps, void* hidden_scratch, mi_stream_t stream) {
  if (!out || !residual || !x || !expert_w_dev || !sel_idx || !sel_w || !hidden_scratch || T <= 0 || D % 8 || F % 8)
    return fail(MI_ERR_ARG, "mi_moe_experts_decode");
  if (T > GEMV_MAX_T) return fail(MI_ERR_UNSUPPORTED, "mi_moe_experts_decode: T = %d > %d (use mi_moe_grouped_gemm)", T, GEMV_MAX_T);
  if (!(top_k == 1 || top_k == 2 || top_k == 4)) return fail(MI_ERR_SHAPE, "MoE: top_k in {1,2,4}");
  if ((size_t)top_k * F * 2 > 65536) return fail(MI_ERR_SHAPE, "MoE: top_k * hidden_dim too large for the decode combine kernel");
  return moe_decode(out, residual, x, ldx, T, D, F, expert_w_dev, sel_idx, sel_w, top_k, norm_w, eps, hidden_scratch, (hipStream_t)stream);
}

size_t mi_moe_grouped_gemm_scratch_bytes(int T, int D, int F, int E, int top_k) {
  if (T <= 0 || D <= 0 || F <= 0 || E <= 0 || top_k <= 0) return 0;
  return moe_carve(T, D, F, E, top_k, nullptr).total;
}

int mi_moe_grouped_gemm(void* out, const void* residual, const void* x, int ldx, int T, int D, int F, int E, int top_k,
                        const void* const* expert_w_dev, const int32_t* sel_idx, const float* sel_w, void* scratch,
                        size_t scratch_bytes, mi_stream_t stream) {
  if (!out || !residual || !x || !expert_w_dev || !sel_idx || !sel_w || !scratch || T <= 0 || D % 8 || F % 8 || ldx != D)
    return fail(MI_ERR_ARG, "mi_moe_grouped_gemm (x must be dense [T, D])");
  if (E > 16 || top_k > 4 || top_k > E || top_k < 1) return fail(MI_ERR_SHAPE, "MoE: E <= 16, top_k <= 4");
  MoeScratch w = moe_carve(T, D, F, E, top_k, (char*)scratch);
  if (w.total > scratch_bytes) return fail(MI_ERR_WORKSPACE, "mi_moe_grouped_gemm: scratch %zu < required %zu", scratch_bytes, w.total);
  return moe_grouped(out, residual, x, T, D, F, E, top_k, expert_w_dev, sel_idx, sel_w, w, (hipStream_t)stream);
}

int mi_set_decode_engine(int enabled) {
  const int prev = engine_mode();
  g_engine_mode = enabled != 0;
  return prev;
}

int mi_decode_engine_reset(void* workspace, mi_stream_t stream) {
  if (!workspace) return fail(MI_ERR_ARG, "mi_decode_engine_reset");
  hipStream_t s = (hipStream_t)stream;
  // a raised status poisons the workspace (every later engine launch leaves at once): clear it, clear the abort broadcast
  // and the arrival count, and move to an epoch whose tags no granule of the failed step can carry
  MI_TRY(hip_rc(launch_engine_ctrl_reset(reinterpret_cast<uint32_t*>(workspace), s), "engine reset"));
  return MI_OK;
}

int mi_greedy_sample(const float* logits, int ld, int B, int vocab, int64_t* token, float* logprob, mi_stream_t stream) {
  if (!logits || !token || !logprob || B <= 0 || vocab <= 0 || ld < vocab) return fail(MI_ERR_ARG, "mi_greedy_sample");
  return hip_rc(launch_greedy_rows(logits, ld, B, vocab, token, logprob, nullptr, nullptr, 0, nullptr, (hipStream_t)stream),
                "greedy sample");
}

int mi_sample_top_p(const float* logits, int ld, int B, int vocab, float temperature, float top_p, uint64_t seed,
                    uint64_t offset, const float* uniforms, int64_t* token, float* logprob, mi_stream_t stream) {
  if (!logits || !token || !logprob || B <= 0 || vocab <= 0 || ld < vocab) return fail(MI_ERR_ARG, "mi_sample_top_p");
  if (!(temperature > 0.f) || !(top_p >= 0.f && top_p <= 1.f))
    return fail(MI_ERR_ARG, "mi_sample_top_p: temperature %g must be > 0 and top_p %g in [0, 1] (generate.py:163)", (double)temperature,
                (double)top_p);
  return hip_rc(launch_sample_top_p(logits, ld, B, vocab, temperature, top_p, seed, offset, uniforms, token, logprob, nullptr,
                                    nullptr, 0, nullptr, (hipStream_t)stream),
                "top-p sample");
}

int mi_verify_sample(const float* logits, int ld, int T, int B, int vocab, const int64_t* ids, const int32_t* q_start,
                     float temperature, float top_p, uint64_t seed, uint64_t offset, const float* uniforms, int64_t* tokens,
                     float* logprobs, int32_t* n_accept, mi_stream_t stream) {
  if (!logits || !ids || !q_start || !tokens || !logprobs || !n_accept || T <= 0 || B <= 0 || B > T || vocab <= 0 || ld < vocab)
    return fail(MI_ERR_ARG, "mi_verify_sample: logits, ids, q_start and the three outputs; 1 <= B <= T (T %d, B %d), ld >= vocab > 0", T, B);
  if (!(temperature > 0.f) || !(top_p >= 0.f && top_p <= 1.f))
    return fail(MI_ERR_ARG, "mi_verify_sample: temperature %g must be > 0 and top_p %g in [0, 1] (generate.py:163)", (double)temperature,
                (double)top_p);
  return hip_rc(launch_verify_sample(logits, ld, T, B, vocab, ids, q_start, temperature, top_p, seed, offset, uniforms, tokens,
                                     logprobs, n_accept, (hipStream_t)stream),
                "verify sample");
}

int mi_debug_engine_sabotage(void* workspace, int launches, mi_stream_t stream) {
  if (!workspace || launches < 0) return fail(MI_ERR_ARG, "mi_debug_engine_sabotage");
  static thread_local uint32_t v;
  v = (uint32_t)launches;
  MI_TRY(hip_rc(hipMemcpyAsync((uint32_t*)workspace + CTRL_SABOTAGE, &v, 4, hipMemcpyHostToDevice, (hipStream_t)stream), "sabotage word"));
  return hip_rc(hipStreamSynchronize((hipStream_t)stream), "sabotage sync");
}

int mi_decode_engine_census(int forget) {
  if (forget) decode_engine_forget_census();
  return MI_OK;
}

int mi_decode_engine_status(const void* workspace, mi_stream_t stream, uint32_t status[8]) {
  if (!workspace || !status) return fail(MI_ERR_ARG, "mi_decode_engine_status");
  MI_TRY(hip_rc(hipMemcpyAsync(status, workspace, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream), "status copy"));
  return hip_rc(hipStreamSynchronize((hipStream_t)stream), "status sync");
}

size_t mi_debug_engine_trace_bytes(void) { return decode_engine_trace_bytes(device_cus()); }
int mi_debug_set_engine_knobs(int thin, int depth) {
  decode_engine_set_knobs(thin, depth);
  return MI_OK;
}
int mi_debug_set_engine_holders(int on) {
  decode_engine_set_holders(on);
  return MI_OK;
}
int mi_debug_set_engine_variant(int variant) { return decode_engine_set_variant(variant); }
int mi_debug_engine_route(int dim, int n_heads, int n_kv_heads, int hidden_dim, int vocab, int num_experts, int top_k, int n_layers,
                          int cache_size, int n_cus, int variant, int nemo_opt_in, char* out, size_t out_len) {
  if (!out || !out_len || n_layers <= 0 || n_layers > 4096 || n_cus <= 0) return fail(MI_ERR_ARG, "mi_debug_engine_route");
  const size_t n = decode_engine_route_names(dim, n_heads, n_kv_heads, hidden_dim, vocab, num_experts, top_k, n_layers, cache_size, n_cus,
                                             variant, nemo_opt_in != 0, out, out_len);
  return n < out_len ? MI_OK : fail(MI_ERR_ARG, "mi_debug_engine_route: out_len %zu", out_len);
}
int mi_debug_gemv_w4_row_pairs(int n_pairs, int n_cus) { return gemv_w4_row_pairs(n_pairs, n_cus); }
int mi_debug_set_prefill_kernels(int attn_waves, int gemm_tail) {
  attn_prefill_set_mode(attn_waves);
  if (gemm_tail >= 0) gemm_set_tail_mode(gemm_tail);
  return MI_OK;
}
int mi_debug_set_engine_trace(void* dev_buffer) {
  decode_engine_set_trace(dev_buffer);
  return MI_OK;
}

size_t mi_workspace_bytes(const mi_model_t* model, int T, int B, int max_cache_size) {
  if (!model || T <= 0 || B <= 0) return 0;
  return carve(model, T, B, max_cache_size > 0 ? max_cache_size : 1, nullptr).total;
}

static size_t workspace_bytes_quant(const mi_model_t* model, bool quant, int T, int B, int max_cache_size) {
  if (!model || T <= 0 || B <= 0) return 0;
  return carve(model, T, B, max_cache_size > 0 ? max_cache_size : 1, nullptr, quant).total;
}
size_t mi_workspace_bytes_w8(const mi_model_t* model, const mi_w8_model_t* w8, int T, int B, int max_cache_size) {
  return workspace_bytes_quant(model, w8 != nullptr, T, B, max_cache_size);
}
size_t mi_workspace_bytes_w4(const mi_model_t* model, const mi_w4_model_t* w4, int T, int B, int max_cache_size) {
  return workspace_bytes_quant(model, w4 != nullptr, T, B, max_cache_size);
}

size_t mi_workspace_bytes_kv(const mi_model_t* model, int quantised, int T, int B, int max_cache_size, int kv_layout) {
  if (!model || T <= 0 || B <= 0 || !kv_layout_ok(kv_layout)) return 0;
  return carve(model, T, B, max_cache_size > 0 ? max_cache_size : 1, nullptr, quantised != 0, kv_e4m3(kv_layout)).total;
}

size_t mi_workspace_bytes_w8a8(const mi_model_t* model, const mi_w8_model_t* w8, int T, int B, int max_cache_size, int kv_layout) {
  if (!model || !w8 || T <= 0 || B <= 0 || !kv_layout_ok(kv_layout)) return 0;
  return carve(model, T, B, max_cache_size > 0 ? max_cache_size : 1, nullptr, true, kv_e4m3(kv_layout), false, true).total;
}

size_t mi_workspace_bytes_w4a8(const mi_model_t* model, const mi_w4_model_t* w4, int T, int B, int max_cache_size, int kv_layout) {
  if (!model || !w4 || T <= 0 || B <= 0 || !kv_layout_ok(kv_layout)) return 0;
  return carve(model, T, B, max_cache_size > 0 ? max_cache_size : 1, nullptr, true, kv_e4m3(kv_layout), false, true).total;
}

// what a quantised model must be, by name, before any launch
static int check_quant(const char* entry, const mi_model_t* m, const QuantModel& q) {
  return with_format(q.entry_format, [&](auto Q) {
    typedef decltype(Q) F;
    if (q.format != F::kFormat) return fail(MI_ERR_UNSUPPORTED, "%s: weight format %d (%s is the only one)", entry, q.format, F::kFormatName);
    if (!layers_of(q, Q)) return fail(MI_ERR_ARG, "%s: %s without layer scales", entry, F::kArg);
    if (m->num_experts > 0) return fail(MI_ERR_UNSUPPORTED, "%s: %s weights on a MoE model are not implemented (the experts stay bf16)", entry, F::kName);
    if (m->lora_rank > 0)
      return fail(MI_ERR_UNSUPPORTED, "%s: un-merged LoRA on an %s base is not implemented; merge the adapter before quantising", entry, F::kName);
    if (m->dim % F::kMod || m->hidden_dim % F::kMod || (m->n_heads * m->head_dim) % F::kMod)
      return fail(MI_ERR_SHAPE, "%s: dim, hidden_dim and n_heads * head_dim must be multiples of %d (%s)", entry, F::kMod, F::kWhy);
    if (q.head) {  // (its K is dim: the multiple of kMod above)
      if (q.head->format != F::kFormat)
        return fail(MI_ERR_UNSUPPORTED, "%s: LM head format %d on layers of format %s (a quantised LM head is in the layers' format)", entry,
                    q.head->format, F::kFormatName);
      if (!q.head->scale) return fail(MI_ERR_ARG, "%s: quantised LM head without %s", entry, F::kScales);
    }
    return (int)MI_OK;
  });
}

// what a verify step must be, by name, before any launch (mi_forward_verify; the batch has passed check_batch)
static int check_verify(const char* entry, const mi_model_t* m, const mi_batch_t* bt, const mi_verify_out_t* vo) {
  if (!vo->tokens || !vo->logprobs || !vo->n_accept) return fail(MI_ERR_ARG, "%s: outputs (tokens, logprobs, n_accept)", entry);
  if (m->lora_rank > 0) return fail(MI_ERR_UNSUPPORTED, "%s: un-merged LoRA (lora_rank %d) in a verify step is not implemented; merge the adapter", entry, m->lora_rank);
  if (bt->branch != MI_BRANCH_PREFILL || !bt->kv_seqlens)
    return fail(MI_ERR_ARG, "%s: a verify step needs a cache: the PREFILL branch with kv_seqlens (branch %d)", entry, bt->branch);
  if (kv_e4m3(bt->kv_layout)) return fail(MI_ERR_UNSUPPORTED, "%s: rings of e4m3 bytes (MI_KV_E4M3) in a verify step are not implemented", entry);
  // sample_temperature > 0: the step verifies by sampling (mi_verify_sample); top_p as mi_forward checks it
  if (bt->sample_temperature > 0.f && !(bt->sample_top_p >= 0.f && bt->sample_top_p <= 1.f))
    return fail(MI_ERR_ARG, "%s: sample_temperature %g / sample_top_p %g", entry, (double)bt->sample_temperature, (double)bt->sample_top_p);
  if (bt->T > GEMV_MAX_T) return fail(MI_ERR_UNSUPPORTED, "%s: T = %d rows; a verify step takes at most %d", entry, bt->T, GEMV_MAX_T);
  if (bt->B > bt->T || bt->max_q_len < 1 || bt->max_q_len > bt->T - bt->B + 1)
    return fail(MI_ERR_ARG, "%s: every sequence brings m_b >= 1 rows (T %d, B %d, max_q_len %d)", entry, bt->T, bt->B, bt->max_q_len);
  if (!bt->input_ids || !m->tok_embeddings || !bt->logits)
    return fail(MI_ERR_ARG, "%s: input_ids, the embedding table and a logits buffer [T, vocab] are needed (one pipeline stage)", entry);
  for (int l = 0; l < m->n_layers; ++l)
    if (bt->cache_sizes[l] <= 0 || attn_verify_splits(bt->cache_sizes[l]) > 32)
      return fail(MI_ERR_UNSUPPORTED, "%s: layer %d has a ring of %d slots; the verify attention takes 1 .. 4096", entry, l, bt->cache_sizes[l]);
  return MI_OK;
}

// mi_forward, mi_forward_w8 and mi_forward_w4.  q == nullptr: exactly the launches of mi_forward as they always were.
// vo != nullptr: a verify step (mi_forward_verify) - the T <= 8 launches of a prefill chunk with the verify attention in place of
// the prefill attention and NO ring write, then argmax and acceptance (sample_temperature > 0: the sampled verification) and the
// commit of the accepted rows.
// a8 (mi_forward_w8a8, mi_forward_w4a8): x_q | s_x behind the workspace, and the quantised groups of a forward of 256 rows or more
// take the format's FP8-activation route (W8A8 / W4A8).
static int forward_body(const char* entry, const mi_model_t* m, const QuantModel* q, const mi_batch_t* bt, mi_stream_t stream,
                        const mi_verify_out_t* vo = nullptr, bool a8 = false) {
  MI_TRY(check_model(m));
  if (q) MI_TRY(check_quant(entry, m, *q));
  BatchInfo bi;
  MI_TRY(check_batch(entry, m, bt, true, &bi));
  if (vo) MI_TRY(check_verify(entry, m, bt, vo));
  int maxW = 1;
  if (bi.has_cache)
    for (int l = 0; l < m->n_layers; ++l) maxW = bt->cache_sizes[l] > maxW ? bt->cache_sizes[l] : maxW;
  const bool kv8 = bi.has_cache && kv_e4m3(bi.kv_layout);  // rings of e4m3 bytes: written by the e4m3 ring-write kernel only
  const Workspace ws = carve(m, bi.T, vo ? bi.T : bi.B, maxW, (char*)bt->workspace, q != nullptr, kv8, vo != nullptr, a8, q && q->head);
  MI_TRY(check_workspace_and_sample(entry, bt, ws.total, &bi));
  const int T = bi.T, B = bi.B, branch = bi.branch, kvl = bi.kv_layout;  // (kvl keeps MI_KV_E4M3: the ring write and the decode attention pick their e4m3 kernels by it)
  const bool has_cache = bi.has_cache, want_greedy = bi.want_sample, want_topp = bi.want_topp;
  hipStream_t s = (hipStream_t)stream;

  const int D = m->dim, H = m->n_heads, Hkv = m->n_kv_heads, Dh = m->head_dim, F = m->hidden_dim;
  const int nq = H * Dh, nkv = Hkv * Dh, qkv_cols = nq + 2 * nkv;
  const bool gemv = T <= GEMV_MAX_T;
  const bool lora = m->lora_rank > 0;
  bf16_t* h = (bf16_t*)bt->h;

  // input_ids == NULL: h already holds this stage's input - received from the previous pipeline rank, or the multimodal
  // embeddings of transformer.py:190-191 (text rows from mi_embedding, image rows from the vision tower)
  const bool embed = m->tok_embeddings && bt->input_ids;
  uint32_t* engine_ctrl = reinterpret_cast<uint32_t*>(ws.tickets);

  // ---- batch-1 decode step of a dense model: every layer (and the LM head) in ONE persistent launch, which also does
  // the step's bookkeeping (position, embedding row, greedy sample): nothing else is enqueued for the token
  if (branch == MI_BRANCH_DECODE && T == 1 && B == 1 && m->n_layers > 0 && engine_mode()) {
    EngProblem pr;
    memset(&pr, 0, sizeof(pr));
    pr.D = D; pr.H = H; pr.Hkv = Hkv; pr.F = F; pr.V = m->vocab_size; pr.n_layers = m->n_layers; pr.NB = device_cus();
    pr.eps = m->norm_eps; pr.layers = m->layers; pr.cache_k = bt->cache_k; pr.cache_v = bt->cache_v; pr.W = bt->cache_sizes; pr.kv_layout = kvl;
    pr.h = h; pr.rope_cs = m->rope_cs;
    pr.emb = embed ? m->tok_embeddings : nullptr; pr.ids = bt->input_ids; pr.kv_seqlens = bt->kv_seqlens;
    pr.q_start = bt->q_start; pr.kv_before = bt->kv_before; pr.tok_seq = bt->tok_seq; pr.tok_pos = bt->tok_pos;
    pr.final_norm = m->final_norm; pr.output = m->output; pr.logits = bt->logits;
    if (want_greedy && !want_topp) {  // (a nucleus draw is its own small kernel behind the engine launch, below)
      pr.greedy_tok = bt->greedy_token; pr.greedy_lp = bt->greedy_logprob;
      pr.hist_tok = bt->hist_token; pr.hist_lp = bt->hist_logprob; pr.hist_len = bt->hist_len;
    }
    pr.granules = ws.gran; pr.granule_bytes = ws.gran_bytes; pr.ctrl = engine_ctrl;
    pr.E = m->num_experts; pr.top_k = m->top_k; pr.lora_rank = m->lora_rank; pr.quant = q != nullptr;
    const EngStep step = decode_engine_step(pr, s);  // the builds of the route in turn: the first that takes the step ran it
    if (step.declined) snprintf(g_detail, sizeof(g_detail), "decode engine declined: %s", decode_engine_census_detail());  // informational
    if (step.ran) {
      int rc = hip_rc(step.err, step.what);
      if (rc == MI_OK && m->final_norm && !bt->logits) rc = hip_rc(launch_rmsnorm(h, h, m->final_norm, T, D, m->norm_eps, s), "final norm");
      if (rc == MI_OK && want_topp) rc = sample_step(bt, m, true, engine_ctrl, s);
      return rc;
    }
  }

  if (branch == MI_BRANCH_DECODE && embed) {
    MI_TRY(hip_rc(launch_decode_prep_embedding(bt->kv_seqlens, bt->q_start, bt->kv_before, bt->tok_seq, bt->tok_pos, B, h,
                                               m->tok_embeddings, bt->input_ids, D, m->vocab_size, engine_ctrl, s),
                  "decode_prep+embedding"));
  } else {
    if (branch == MI_BRANCH_DECODE)
      MI_TRY(hip_rc(launch_decode_prep(bt->kv_seqlens, bt->q_start, bt->kv_before, bt->tok_seq, bt->tok_pos, B, engine_ctrl, s),
                    "decode_prep"));
    if (embed)
      MI_TRY(hip_rc(launch_embedding(h, m->tok_embeddings, bt->input_ids, T, D, m->vocab_size, engine_ctrl + CTRL_BAD_ID, s), "embedding"));
  }

  // what every linear group of the step shares: the scratch of its routes, and (un-merged LoRA, ABI v8 / v9) the adapter bank -
  // the pointers of a layer's adapters are bank bases and bt->seq_adapter picks a slot per sequence; without it every row runs
  // through slot 0 in the kernels' single-adapter mode
  LinearCall call;
  memset(&call, 0, sizeof(call));
  call.xn = ws.xn; call.deq = ws.deq; call.lora_base = ws.lora_base; call.lora_t = ws.lora_t;
  call.a8 = a8; call.x_q = ws.x_q; call.s_x = ws.s_x;
  const LoraBank bank = lora_bank(m->lora_slots, bt->tok_seq, bt->seq_adapter);
  static const mi_lora_layer_t kNoAdapters = {};

  for (int l = 0; l < m->n_layers; ++l) {
    const mi_layer_t& L = m->layers[l];
    const int W = has_cache ? bt->cache_sizes[l] : 1;
    void* ck = has_cache ? bt->cache_k[l] : nullptr;
    void* cv = has_cache ? bt->cache_v[l] : nullptr;
    const RingWrite ring = {ck, cv, W, kvl};

    // ---- the layer's four linear groups: weights, then the scales of a quantised model or the adapters of an un-merged LoRA
    LinearGroup qkv = group_of(D, L.wq, nq, L.wk, nkv, L.wv, nkv), wo = group_of(nq, L.wo, D), w13 = group_of(D, L.w1, F, L.w3, F),
                w2 = group_of(F, L.w2, D);
    if (q) {
      MI_TRY(with_format(q->entry_format, [&](auto Q) {
        const auto& S = layers_of(*q, Q)[l];
        if (!(S.wq && S.wk && S.wv && S.wo && S.w1 && S.w2 && S.w3))
          return fail(MI_ERR_ARG, "%s: layer %d has a linear without %s", entry, l, decltype(Q)::kScales);
        set_scales(qkv, Q, S.wq, S.wk, S.wv); set_scales(wo, Q, S.wo); set_scales(w13, Q, S.w1, S.w3); set_scales(w2, Q, S.w2);
        return (int)MI_OK;
      }));
    }
    if (lora) {
      if (!L.w1 || !L.w2 || !L.w3) return fail(MI_ERR_ARG, "mi_forward: dense layer without w1/w2/w3");
      const mi_lora_layer_t& A = L.lora ? *L.lora : kNoAdapters;
      const int r = m->lora_rank;
      const float ls = m->lora_scaling;
      set_adapters(qkv, r, ls, bank, A.wq_a, A.wq_b, A.wk_a, A.wk_b, A.wv_a, A.wv_b); set_adapters(wo, r, ls, bank, A.wo_a, A.wo_b);
      set_adapters(w13, r, ls, bank, A.w1_a, A.w1_b, A.w3_a, A.w3_b); set_adapters(w2, r, ls, bank, A.w2_a, A.w2_b);
    }

    // ---- qkv = rope(attention_norm(h) @ [Wq; Wk; Wv]^T); on the DECODE branch the k | v rows also enter the ring here (bf16
    // rings at T <= 8: in the GEMV's epilogue; else one launch more per layer).  A verify step has no ring write at all.
    LinearCall c = call;
    c.x = h; c.ldx = D; c.norm_w = L.attention_norm; c.eps = m->norm_eps; c.out = ws.qkv; c.ldo = qkv_cols; c.epi = EPI_QKV_ROPE;
    c.rope_cs = m->rope_cs; c.tok_pos = bt->tok_pos; c.tok_seq = bt->tok_seq; c.head_dim = Dh;
    c.ring = branch == MI_BRANCH_DECODE ? &ring : nullptr; c.ring_q_start = bt->q_start;
    c.lora_base_f32 = gemv;
    c.what = {"qkv gemv", "qkv gemm", "dequant q|k|v", "attention_norm", "kv_write (decode, e4m3)", "kv_write (decode)"};
    MI_TRY(linear_group(qkv, c, T, s));

    // ---- attention
    if (branch == MI_BRANCH_DECODE) {
      const AttnDecodeArgs a = attn_decode_args(ws.attn, ws.qkv, qkv_cols, ck, cv, kvl, W, B, H, Hkv, Dh, bt->tok_pos, ws.tickets, ws.partial);
      MI_TRY(hip_rc(launch_attn_decode(a, s), "attn_decode"));
    } else if (vo) {
      // verify step: ring keys below kv_before, the step's own rows from ws.qkv (and into the layer's stash); no ring write
      AttnVerifyArgs a = {};
      a.out = ws.attn; a.qkv = ws.qkv; a.ld = qkv_cols; a.cache_k = (const bf16_t*)ck; a.cache_v = (const bf16_t*)cv; a.kv_layout = kvl;
      a.W = W; a.T = T; a.B = B; a.H = H; a.Hkv = Hkv; a.Dh = Dh; a.q_start = bt->q_start; a.kv_before = bt->kv_before;
      a.partial = ws.partial; a.stash = ws.stash + (size_t)l * T * 2 * nkv;
      MI_TRY(hip_rc(launch_attn_verify(a, s), "attn_verify"));
    } else {
      // e4m3 rings: the keys older than this forward are read from the bf16 image of the layer's rings in the scratch (exact); the
      // chunk's own rows come from the activations, unrounded, as ever (transformer_layers.py:72-76)
      const void *pk = ck, *pv = cv;
      if (kv8) {
        const size_t n = (size_t)B * Hkv * W * Dh;
        pk = ws.kv_deq; pv = ws.kv_deq + n;
        MI_TRY(hip_rc(launch_kv_dequant(ws.kv_deq, ws.kv_deq + n, ck, cv, n, s), "kv_dequant"));
      }
      const AttnPrefillArgs a = attn_prefill_args(ws.attn, ws.qkv, qkv_cols, pk, pv, kvl & 1, has_cache ? W : T, B, has_cache ? bt->max_q_len : T,
                                                  H, Hkv, Dh, bt->q_start, bt->kv_before, has_cache ? 1 : 0, 0.f);
      MI_TRY(hip_rc(launch_attn_prefill(a, s), "attn_prefill"));
      if (has_cache) MI_TRY(ring_write(ring, ws.qkv, qkv_cols, T, nq, nkv, Dh, bt->tok_pos, bt->tok_seq, bt->q_start, s, "kv_write"));
    }

    // ---- h = h + attn @ Wo^T   (adapters: the base product goes to xn, which nothing holds here)
    c = call;
    c.x = ws.attn; c.ldx = nq; c.out = h; c.ldo = D; c.residual = h; c.epi = MI_EPI_RESIDUAL; c.lora_base = ws.xn;
    c.what = {"wo gemv", "wo gemm", "dequant wo"};
    MI_TRY(linear_group(wo, c, T, s));

    // ---- h = h + FFN(ffn_norm(h))
    if (m->num_experts == 0) {
      c = call;
      c.x = h; c.ldx = D; c.norm_w = L.ffn_norm; c.eps = m->norm_eps; c.out = ws.hid; c.ldo = F; c.epi = MI_EPI_SWIGLU; c.lora_base_f32 = gemv;
      c.what = {"w13 gemv", "w13 gemm", "dequant w1|w3", "ffn_norm"};
      MI_TRY(linear_group(w13, c, T, s));
      c = call;
      c.x = ws.hid; c.ldx = F; c.out = h; c.ldo = D; c.residual = h; c.epi = MI_EPI_RESIDUAL; c.lora_base = ws.xn;
      c.what = {"w2 gemv", "w2 gemm", "dequant w2"};
      MI_TRY(linear_group(w2, c, T, s));
    } else {
      const int E = m->num_experts, k = m->top_k;
      if (!L.gate || !L.expert_w_dev || !L.expert_w_host) return fail(MI_ERR_ARG, "mi_forward: MoE layer tables");
      if (gemv) {
        MI_TRY(hip_rc(launch_moe_router(ws.sel_idx, ws.sel_w, h, D, T, D, L.gate, E, k, L.ffn_norm, m->norm_eps, s), "moe_router"));
        MI_TRY(moe_decode(h, h, h, D, T, D, F, L.expert_w_dev, ws.sel_idx, ws.sel_w, k, L.ffn_norm, m->norm_eps, ws.hid, s));
      } else {
        MI_TRY(hip_rc(launch_rmsnorm(ws.xn, h, L.ffn_norm, T, D, m->norm_eps, s), "ffn_norm"));
        MI_TRY(hip_rc(launch_moe_router(ws.sel_idx, ws.sel_w, ws.xn, D, T, D, L.gate, E, k, nullptr, 0.f, s), "moe_router"));
        const MoeScratch sc = {ws.hid, ws.moe_y, ws.tok_of, ws.row_of, ws.tile_tab, ws.n_tiles, ws.max_tiles, 0};
        MI_TRY(moe_grouped(h, h, ws.xn, T, D, F, E, k, L.expert_w_dev, ws.sel_idx, ws.sel_w, sc, s));
      }
    }
  }

  // ---- final norm (+ LM head; + the step's sample: generate.py:124-136 fused behind the LM head)
  if (m->final_norm && !bt->logits) {
    MI_TRY(hip_rc(launch_rmsnorm(h, h, m->final_norm, T, D, m->norm_eps, s), "final norm"));
  } else if (m->final_norm) {
    // the LM head carries no adapters; it is bf16 unless the entry was handed its quantisation (mi_forward_q), and then it stays on
    // the weight-only routes also where the layers take the FP8-activation GEMMs (linear_group: never a8 on MI_EPI_LOGITS)
    LinearCall c = call;
    c.x = h; c.ldx = D; c.norm_w = m->final_norm; c.eps = m->norm_eps; c.out = bt->logits; c.ldo = m->vocab_size; c.epi = MI_EPI_LOGITS;
    c.deq = ws.head_deq;
    c.what = {"lm head gemv", "lm head gemm", "dequant lm head", "final norm"};
    LinearGroup head = group_of(D, m->output, m->vocab_size);
    if (q && q->head) {
      if (q->entry_format == MI_W4_MXFP4) set_scales(head, QuantW4{}, (const uint8_t*)q->head->scale);
      else set_scales(head, QuantW8{}, (const float*)q->head->scale);
    }
    MI_TRY(linear_group(head, c, T, s));
    if (want_greedy) MI_TRY(sample_step(bt, m, want_topp, engine_ctrl, s));
  }
  if (vo) {
    if (bt->sample_temperature > 0.f) {  // sampled verification: accept / residual draw per row, then the scan (mi_verify_sample)
      MI_TRY(hip_rc(launch_verify_sample(bt->logits, m->vocab_size, T, B, m->vocab_size, bt->input_ids, bt->q_start, bt->sample_temperature,
                                         bt->sample_top_p, bt->sample_seed, bt->sample_offset, nullptr, vo->tokens, vo->logprobs,
                                         vo->n_accept, s), "verify sample"));
    } else {
      MI_TRY(hip_rc(launch_greedy_rows(bt->logits, m->vocab_size, T, m->vocab_size, vo->tokens, vo->logprobs, nullptr, nullptr, 0, nullptr, s),
                    "verify argmax"));
      MI_TRY(hip_rc(launch_verify_accept(bt->input_ids, vo->tokens, bt->q_start, B, vo->n_accept, s), "verify accept"));
    }
    for (int l0 = 0; l0 < m->n_layers; l0 += VERIFY_COMMIT_LAYERS) {  // (one launch up to 128 layers)
      VerifyCommitArgs c;
      memset(&c, 0, sizeof(c));
      c.n_layers = m->n_layers - l0 < VERIFY_COMMIT_LAYERS ? m->n_layers - l0 : VERIFY_COMMIT_LAYERS;
      for (int l = 0; l < c.n_layers; ++l) {
        c.k[l] = (bf16_t*)bt->cache_k[l0 + l]; c.v[l] = (bf16_t*)bt->cache_v[l0 + l]; c.W[l] = bt->cache_sizes[l0 + l];
      }
      c.stash = ws.stash + (size_t)l0 * T * 2 * nkv;
      c.T = T; c.B = B; c.kv_dim = nkv; c.Dh = Dh; c.kv_layout = kvl & 1;
      c.q_start = bt->q_start; c.kv_before = bt->kv_before; c.tok_seq = bt->tok_seq; c.n_accept = vo->n_accept;
      c.kv_seqlens = (l0 + VERIFY_COMMIT_LAYERS >= m->n_layers) ? bt->kv_seqlens : nullptr;
      MI_TRY(hip_rc(launch_verify_commit(c, s), "verify commit"));
    }
  }
  return MI_OK;
}

int mi_forward(const mi_model_t* m, const mi_batch_t* bt, mi_stream_t stream) { return forward_body("mi_forward", m, nullptr, bt, stream); }

int mi_forward_w8(const mi_model_t* m, const mi_w8_model_t* w8, const mi_batch_t* bt, mi_stream_t stream) {
  const QuantModel q = quant_model(w8, nullptr);
  return forward_body(w8 ? "mi_forward_w8" : "mi_forward", m, w8 ? &q : nullptr, bt, stream);
}

int mi_forward_w4(const mi_model_t* m, const mi_w4_model_t* w4, const mi_batch_t* bt, mi_stream_t stream) {
  const QuantModel q = quant_model(nullptr, w4);
  return forward_body(w4 ? "mi_forward_w4" : "mi_forward", m, w4 ? &q : nullptr, bt, stream);
}

int mi_forward_w8a8(const mi_model_t* m, const mi_w8_model_t* w8, const mi_batch_t* bt, mi_stream_t stream) {
  if (!w8) return fail(MI_ERR_ARG, "mi_forward_w8a8: w8 (the FP8 prefill GEMMs read FP8 weights)");
  const QuantModel q = quant_model(w8, nullptr);
  return forward_body("mi_forward_w8a8", m, &q, bt, stream, nullptr, true);
}

int mi_forward_w4a8(const mi_model_t* m, const mi_w4_model_t* w4, const mi_batch_t* bt, mi_stream_t stream) {
  if (!w4) return fail(MI_ERR_ARG, "mi_forward_w4a8: w4 (the MXFP4 x FP8 prefill GEMMs read MXFP4 weights)");
  const QuantModel q = quant_model(nullptr, w4);
  return forward_body("mi_forward_w4a8", m, &q, bt, stream, nullptr, true);
}

size_t mi_workspace_bytes_verify(const mi_model_t* model, int quantised, int T, int max_cache_size, int kv_layout) {
  if (!model || T <= 0 || T > GEMV_MAX_T || !kv_layout_ok(kv_layout) || kv_e4m3(kv_layout)) return 0;
  return carve(model, T, T, max_cache_size > 0 ? max_cache_size : 1, nullptr, quantised != 0, false, true).total;
}

int mi_forward_verify(const mi_model_t* m, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_batch_t* bt,
                      const mi_verify_out_t* out, mi_stream_t stream) {
  if (!out) return fail(MI_ERR_ARG, "mi_forward_verify: outputs");
  if (w8 && w4) return fail(MI_ERR_ARG, "mi_forward_verify: both w8 and w4 given; a model has at most one weight format");
  const QuantModel q = quant_model(w8, w4);
  return forward_body("mi_forward_verify", m, (w8 || w4) ? &q : nullptr, bt, stream, out);
}

/* a quantised LM head (include/mistral_hip.h: mi_lm_head_quant_t) */
size_t mi_workspace_bytes_q(const mi_model_t* model, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_lm_head_quant_t* head,
                            int T, int B, int max_cache_size, int kv_layout, int a8, int verify) {
  if (!model || T <= 0 || B <= 0 || !kv_layout_ok(kv_layout) || (w8 && w4)) return 0;
  if (a8 && !w8 && !w4) return 0;
  if (verify && (T > GEMV_MAX_T || kv_e4m3(kv_layout))) return 0;
  if (head && !w8 && !w4) return 0;
  return carve(model, T, verify ? T : B, max_cache_size > 0 ? max_cache_size : 1, nullptr, w8 || w4, kv_e4m3(kv_layout), verify != 0, a8 != 0,
               head != nullptr).total;
}

int mi_forward_q(const mi_model_t* m, const mi_w8_model_t* w8, const mi_w4_model_t* w4, const mi_lm_head_quant_t* head,
                 const mi_batch_t* bt, const mi_verify_out_t* verify_out, int a8, mi_stream_t stream) {
  // head == NULL: the old entries, under their own names in the error details
  const char* me = head ? "mi_forward_q" : verify_out ? "mi_forward_verify" : a8 ? (w4 ? "mi_forward_w4a8" : "mi_forward_w8a8")
                   : w8 ? "mi_forward_w8" : w4 ? "mi_forward_w4" : "mi_forward";
  if (w8 && w4) return fail(MI_ERR_ARG, "%s: both w8 and w4 given; a model has at most one weight format", me);
  if (a8 && !w8 && !w4) return fail(MI_ERR_ARG, "%s: a8 without w8 or w4 (the FP8-activation prefill GEMMs read quantised weights)", me);
  if (head && !w8 && !w4)
    return fail(MI_ERR_UNSUPPORTED, "%s: a quantised LM head on a model without quantised layers (the head is quantised in the layers' format)", me);
  QuantModel q = quant_model(w8, w4);
  q.head = head;
  return forward_body(me, m, (w8 || w4) ? &q : nullptr, bt, stream, verify_out, a8 != 0);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- generic storage dtype
// mi_forward for fp32 / fp16 storage (and for bf16 models of a shape check_model declines): launch by launch over the
// kernels of generic.hip.  Same mi_model_t / mi_batch_t contract (pointers are to `dtype` elements), same metadata
// protocol (DECODE: positions from kv_seqlens on the device), same sample epilogue behind the LM head.
namespace {

struct GWorkspace {
  uint32_t* ctrl;
  char *xn, *qkv, *attn, *a, *b, *y, *res, *glog;
  int32_t *sel_idx, *active;
  float *sel_w, *wt, *attn_partial;
  size_t total;
};

GWorkspace carve_generic(const mi_model_t* m, int T, size_t es, char* base) {
  GWorkspace w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  const size_t qkv_cols = (size_t)(m->n_heads + 2 * m->n_kv_heads) * m->head_dim;
  const bool moe = m->num_experts > 0;
  w.ctrl = (uint32_t*)take(TICKET_BYTES);  // same control words as mi_forward (step counter, bad-id flag)
  w.xn = take((size_t)T * m->dim * es);
  w.qkv = take((size_t)T * qkv_cols * es);
  w.attn = take((size_t)T * m->n_heads * m->head_dim * es);
  w.a = take((size_t)T * m->hidden_dim * es);
  w.b = take((size_t)T * m->hidden_dim * es);
  w.y = take(moe ? (size_t)T * m->dim * es : 0);
  w.res = take(moe ? (size_t)T * m->dim * es : 0);
  w.glog = take(moe ? (size_t)T * m->num_experts * es : 0);
  w.sel_idx = (int32_t*)take(moe ? (size_t)T * m->top_k * 4 : 0);
  w.sel_w = (float*)take(moe ? (size_t)T * m->top_k * 4 : 0);
  w.active = (int32_t*)take(moe ? (size_t)T * 4 : 0);
  w.wt = (float*)take(moe ? (size_t)T * 4 : 0);
  w.attn_partial = (float*)take(g_attn_partial_floats(T, m->n_heads, m->head_dim) * sizeof(float));
  w.total = off;
  return w;
}

int check_model_generic(const mi_model_t* m, int dtype) {
  if (!m || !m->layers) return fail(MI_ERR_ARG, "null model");
  if (m->lora_rank != 0)
    return fail(MI_ERR_UNSUPPORTED, "un-merged LoRA on fp16 / fp32 storage (mi_forward_generic) is not implemented; merge the adapter");
  if (!dtype_ok(dtype)) return fail(MI_ERR_ARG, "storage dtype %d", dtype);
  if (m->head_dim <= 0 || m->head_dim > 256 || m->head_dim % 8) return fail(MI_ERR_SHAPE, "head_dim %d: multiple of 8, <= 256", m->head_dim);
  if (m->n_kv_heads <= 0 || m->n_heads % m->n_kv_heads) return fail(MI_ERR_SHAPE, "n_heads %% n_kv_heads != 0");
  if (m->dim % 8 || m->hidden_dim % 8) return fail(MI_ERR_SHAPE, "dim/hidden_dim must be multiples of 8");
  if (m->num_experts > 0 && (m->top_k <= 0 || m->top_k > m->num_experts)) return fail(MI_ERR_SHAPE, "MoE: 0 < top_k <= num_experts");
  return MI_OK;
}
int check_dt(int dtype, const char* what) {
  return dtype_ok(dtype) ? MI_OK : fail(MI_ERR_ARG, "%s: storage dtype %d", what, dtype);
}

}  // namespace

extern "C" {

// ---- leaf operators in any storage dtype (ABI v6): what module-level callers of an fp16 / fp32 model bind - the Pixtral tower
// (vision_encoder.py), RMSNorm / FeedForward modules used stand-alone.  Same kernels as mi_forward_generic.
int mi_embedding_generic(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_embedding_generic"));
  if (!out || !table || !ids || T <= 0 || D <= 0) return fail(MI_ERR_ARG, "mi_embedding_generic");
  return hip_rc(launch_g_embedding(dtype, out, table, ids, T, D, vocab, nullptr, (hipStream_t)stream), "embedding");
}

int mi_rmsnorm_generic(void* out, const void* x, const void* w, int T, int D, float eps, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_rmsnorm_generic"));
  if (!out || !x || !w || T <= 0 || D <= 0) return fail(MI_ERR_ARG, "mi_rmsnorm_generic");
  return hip_rc(launch_g_rmsnorm(dtype, out, x, w, T, D, eps, (hipStream_t)stream), "rmsnorm");
}

/* out[:, columns of w[i]] = epilogue(x @ w[i]^T), i < 3 (w[i] == NULL ends the list): MI_EPI_STORE, MI_EPI_RESIDUAL (residual
 * [M, N] with row stride ldo) or MI_EPI_LOGITS (fp32 out).  One launch per matrix. */
int mi_linear_generic(void* out, int ldo, const void* x, int ldx, int M, int K, const void* const w[3], const int n_rows[3],
                      int epilogue, const void* residual, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_linear_generic"));
  if (!out || !x || !w || !n_rows || !w[0] || M <= 0 || K <= 0) return fail(MI_ERR_ARG, "mi_linear_generic");
  int epi;
  switch (epilogue) {
    case MI_EPI_STORE: epi = G_EPI_STORE; break;
    case MI_EPI_RESIDUAL: epi = G_EPI_RESIDUAL; break;
    case MI_EPI_LOGITS: epi = G_EPI_LOGITS; break;
    default: return fail(MI_ERR_UNSUPPORTED, "mi_linear_generic: epilogue %d (SwiGLU: two calls + mi_swiglu_generic)", epilogue);
  }
  if (epi == G_EPI_RESIDUAL && !residual) return fail(MI_ERR_ARG, "mi_linear_generic: residual");
  const size_t es = g_elem_bytes(dtype), oes = epi == G_EPI_LOGITS ? 4 : es;
  int col = 0;
  for (int i = 0; i < 3 && w[i]; ++i) {
    if (n_rows[i] <= 0) return fail(MI_ERR_ARG, "mi_linear_generic: n_rows[%d]", i);
    GLinearArgs g;
    memset(&g, 0, sizeof(g));
    g.x = x; g.ldx = ldx; g.w = w[i]; g.out = (char*)out + (size_t)col * oes; g.ldo = ldo;
    g.residual = residual ? (const char*)residual + (size_t)col * es : nullptr; g.ldr = ldo;
    g.M = M; g.N = n_rows[i]; g.K = K; g.epi = epi;
    MI_TRY(hip_rc(launch_g_linear(dtype, g, (hipStream_t)stream), "linear"));
    col += n_rows[i];
  }
  return MI_OK;
}

/* rope.py:13-23 in place on the first n_rot_cols columns (heads of head_dim): pair i of a head turns by rope_cs[tok_pos[t], i] */
int mi_rope_inplace_generic(void* qkv, int ld, int T, int n_rot_cols, int head_dim, const float* rope_cs, const int32_t* tok_pos,
                            int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_rope_inplace_generic"));
  if (!qkv || !rope_cs || !tok_pos || T <= 0 || head_dim <= 0 || head_dim % 2 || n_rot_cols % head_dim || n_rot_cols > ld)
    return fail(MI_ERR_ARG, "mi_rope_inplace_generic");
  return hip_rc(launch_g_rope(dtype, qkv, ld, T, n_rot_cols, head_dim, rope_cs, tok_pos, (hipStream_t)stream), "rope");
}

/* the cache=None attention (transformer_layers.py:72-73,165: every token sees every token): qkv [T, ld] = q | k | v after RoPE */
int mi_attention_nocache_generic(void* out, const void* qkv, int ld, int T, int n_heads, int n_kv_heads, int head_dim,
                                 float softmax_scale, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_attention_nocache_generic"));
  if (!out || !qkv || T <= 0 || n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads || head_dim <= 0 || head_dim > 256)
    return fail(MI_ERR_ARG, "mi_attention_nocache_generic");
  GAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.out = out; a.ldo = n_heads * head_dim; a.qkv = qkv; a.ld = ld; a.W = T; a.T = T; a.H = n_heads; a.Hkv = n_kv_heads; a.Dh = head_dim;
  a.causal = 0;
  a.scale = softmax_scale > 0.f ? softmax_scale : 1.0f / sqrtf((float)head_dim);
  return hip_rc(launch_g_attention(dtype, a, (hipStream_t)stream), "attention");
}

/* a <- silu(a) * b on [T, F] dense rows (transformer_layers.py:106) */
int mi_swiglu_generic(void* a, const void* b, int T, int F, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_swiglu_generic"));
  if (!a || !b || T <= 0 || F <= 0) return fail(MI_ERR_ARG, "mi_swiglu_generic");
  return hip_rc(launch_g_swiglu(dtype, a, b, T, F, nullptr, (hipStream_t)stream), "swiglu");
}

int mi_gelu_generic(void* x, int ldx, int T, int N, int dtype, mi_stream_t stream) {
  MI_TRY(check_dt(dtype, "mi_gelu_generic"));
  if (!x || T <= 0 || N <= 0 || ldx < N) return fail(MI_ERR_ARG, "mi_gelu_generic");
  return hip_rc(launch_g_gelu(dtype, x, ldx, T, N, (hipStream_t)stream), "gelu");
}

size_t mi_workspace_bytes_generic(const mi_model_t* model, int T, int dtype) {
  if (!model || T <= 0) return 0;
  return carve_generic(model, T, g_elem_bytes(dtype), nullptr).total;
}

int mi_forward_generic(const mi_model_t* m, const mi_batch_t* bt, int dtype, mi_stream_t stream) {
  MI_TRY(check_model_generic(m, dtype));
  const int dt = dtype;
  const size_t es = g_elem_bytes(dt);
  BatchInfo bi;
  MI_TRY(check_batch("mi_forward_generic", m, bt, false, &bi));
  if (kv_e4m3(bi.kv_layout))
    return fail(MI_ERR_UNSUPPORTED, "mi_forward_generic: K/V rings of e4m3 bytes (MI_KV_E4M3) are not implemented for fp16 / fp32 storage or "
                "on the generic route; use rings of the model's dtype");
  const GWorkspace ws = carve_generic(m, bi.T, es, (char*)bt->workspace);
  MI_TRY(check_workspace_and_sample("mi_forward_generic", bt, ws.total, &bi));
  const int T = bi.T, B = bi.B, branch = bi.branch, kvl = bi.kv_layout;
  const bool has_cache = bi.has_cache;
  hipStream_t s = (hipStream_t)stream;

  const int D = m->dim, H = m->n_heads, Hkv = m->n_kv_heads, Dh = m->head_dim, F = m->hidden_dim;
  const int nq = H * Dh, nkv = Hkv * Dh, qkv_cols = nq + 2 * nkv;
  char* h = (char*)bt->h;

  auto linear = [&](const void* x, int ldx, const void* w, void* out, int ldo, int N, int K, int epi, const void* residual,
                    const int32_t* active, const char* what) -> int {
    GLinearArgs g;
    memset(&g, 0, sizeof(g));
    g.x = x; g.ldx = ldx; g.w = w; g.out = out; g.ldo = ldo; g.residual = residual; g.ldr = ldo;
    g.M = T; g.N = N; g.K = K; g.epi = epi; g.active = active;
    return hip_rc(launch_g_linear(dt, g, s), what);
  };
  // launch_g_linear's fused forms on x [T, D]: an RMSNorm prologue (norm_w), up to three matrices side by side (w1 / w2 from
  // columns n0 / n1 on), or w and w1 through SiLU * mul (G_EPI_SWIGLU)
  auto fused = [&](const void* x, const void* norm_w, const void* w, const void* w1, const void* w2, int n0, int n1, void* out, int N,
                   int epi) {
    GLinearArgs g;
    memset(&g, 0, sizeof(g));
    g.x = x; g.ldx = D; g.w = w; g.w1 = w1; g.w2 = w2; g.n0 = n0; g.n1 = n1; g.norm_w = norm_w; g.eps = norm_w ? m->norm_eps : 0.f;
    g.out = out; g.ldo = N; g.M = T; g.N = N; g.K = D; g.epi = epi;
    return g;
  };
  // T <= 8 (decode steps, tiny prompts): the row kernel's fused forms - RMSNorm in the prologue, q | k | v in one launch,
  // gate / up / SiLU / product in one launch: 8 launches per dense layer instead of 13
  const bool rows = g_gemv_takes(T, D, D);
  // ... and for fp16 those launches are the TUNED weight-streaming kernels themselves (gemv.hip compiled for fp16 payloads,
  // launch_gemv_f16): RMSNorm + q | k | v + RoPE in one launch, Wo / W2 with the residual, RMSNorm + gate | up + SiLU, the LM
  // head - the launch path of mi_forward minus its bf16 attention kernels.  MI_GENERIC_GEMV_TUNED=0: the generic row kernel.
  static int tuned_rows = -1;
  if (tuned_rows < 0) {
    const char* e = getenv("MI_GENERIC_GEMV_TUNED");
    tuned_rows = e ? atoi(e) : 1;
  }
  const bool rows16 = rows && dt == G_DT_FP16 && tuned_rows != 0 && Dh % 2 == 0;

  if (branch == MI_BRANCH_DECODE)
    MI_TRY(hip_rc(launch_decode_prep(bt->kv_seqlens, bt->q_start, bt->kv_before, bt->tok_seq, bt->tok_pos, B, ws.ctrl, s), "decode_prep"));
  if (m->tok_embeddings && bt->input_ids)
    MI_TRY(hip_rc(launch_g_embedding(dt, h, m->tok_embeddings, bt->input_ids, T, D, m->vocab_size, ws.ctrl + CTRL_BAD_ID, s), "embedding"));

  for (int l = 0; l < m->n_layers; ++l) {
    const mi_layer_t& L = m->layers[l];
    const int W = has_cache ? bt->cache_sizes[l] : T;
    void* ck = has_cache ? bt->cache_k[l] : nullptr;
    void* cv = has_cache ? bt->cache_v[l] : nullptr;
    // ---- attention_norm, q | k | v, RoPE (transformer_layers.py:66-70)
    if (rows16) {
      // (no ring write in the epilogue: it follows the attention here, g_kv_write below)
      MI_TRY(gemv_passes(kGemvF16, gemv_qkv_rope(h, D, D, L.attention_norm, m->norm_eps, L.wq, L.wk, L.wv, nq, nkv, ws.qkv, qkv_cols,
                                                 m->rope_cs, bt->tok_pos, bt->tok_seq, Dh, nullptr),
                         T, s, "norm + q|k|v + rope (fp16 gemv)"));
    } else if (rows) {
      const GLinearArgs g = fused(h, L.attention_norm, L.wq, L.wk, L.wv, nq, nq + nkv, ws.qkv, qkv_cols, G_EPI_STORE);
      MI_TRY(hip_rc(launch_g_linear(dt, g, s), "norm + q|k|v"));
    } else {
      MI_TRY(hip_rc(launch_g_rmsnorm(dt, ws.xn, h, L.attention_norm, T, D, m->norm_eps, s), "attention_norm"));
      const GLinearArgs g = fused(ws.xn, nullptr, L.wq, L.wk, L.wv, nq, nq + nkv, ws.qkv, qkv_cols, G_EPI_STORE);
      if (g_linear_fused_ok(dt, g)) {  // (fp16, at least 256 rows: one launch of the 256-tile kernel)
        MI_TRY(hip_rc(launch_g_linear(dt, g, s), "q|k|v"));
      } else {
        MI_TRY(linear(ws.xn, D, L.wq, ws.qkv, qkv_cols, nq, D, G_EPI_STORE, nullptr, nullptr, "wq"));
        MI_TRY(linear(ws.xn, D, L.wk, ws.qkv + (size_t)nq * es, qkv_cols, nkv, D, G_EPI_STORE, nullptr, nullptr, "wk"));
        MI_TRY(linear(ws.xn, D, L.wv, ws.qkv + (size_t)(nq + nkv) * es, qkv_cols, nkv, D, G_EPI_STORE, nullptr, nullptr, "wv"));
      }
    }
    if (!rows16) MI_TRY(hip_rc(launch_g_rope(dt, ws.qkv, qkv_cols, T, nq + nkv, Dh, m->rope_cs, bt->tok_pos, s), "rope"));
    // ---- attention over [surviving ring entries ++ this forward's keys], then the ring write (cache.py:83-117)
    GAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.out = ws.attn; a.ldo = nq; a.qkv = ws.qkv; a.ld = qkv_cols; a.cache_k = ck; a.cache_v = cv; a.kv_layout = kvl;
    a.W = W; a.T = T; a.H = H; a.Hkv = Hkv; a.Dh = Dh;
    a.q_start = bt->q_start; a.kv_before = bt->kv_before; a.tok_seq = bt->tok_seq; a.tok_pos = bt->tok_pos;
    a.causal = has_cache ? 1 : 0;
    a.scale = 1.0f / sqrtf((float)Dh);
    a.partial = ws.attn_partial;
    a.B = has_cache ? B : 1; a.max_q_len = has_cache ? bt->max_q_len : T;
    MI_TRY(hip_rc(launch_g_attention(dt, a, s), "attention"));
    if (has_cache)
      MI_TRY(hip_rc(launch_g_kv_write(dt, ck, cv, W, ws.qkv + (size_t)nq * es, ws.qkv + (size_t)(nq + nkv) * es, qkv_cols, T, nkv,
                                      bt->tok_seq, bt->tok_pos, bt->q_start, kvl, Dh, s), "kv_write"));
    // ---- h = h + wo(attn)
    if (rows16)
      MI_TRY(gemv_passes(kGemvF16, gemv_residual(ws.attn, nq, L.wo, h, D), T, s, "wo (fp16 gemv)"));
    else
      MI_TRY(linear(ws.attn, nq, L.wo, h, D, D, nq, G_EPI_RESIDUAL, h, nullptr, "wo"));
    // ---- h = h + FFN(ffn_norm(h))
    if (m->num_experts == 0) {
      if (!L.w1 || !L.w2 || !L.w3) return fail(MI_ERR_ARG, "mi_forward_generic: dense layer without w1/w2/w3");
      if (rows16) {
        MI_TRY(gemv_passes(kGemvF16, gemv_swiglu(h, D, L.ffn_norm, m->norm_eps, L.w1, L.w3, ws.a, F), T, s, "norm + w1|w3 + swiglu (fp16 gemv)"));
        MI_TRY(gemv_passes(kGemvF16, gemv_residual(ws.a, F, L.w2, h, D), T, s, "w2 (fp16 gemv)"));
      } else if (rows) {
        const GLinearArgs g = fused(h, L.ffn_norm, L.w1, L.w3, nullptr, 0, 0, ws.a, F, G_EPI_SWIGLU);
        MI_TRY(hip_rc(launch_g_linear(dt, g, s), "norm + w1|w3 + swiglu"));
      } else {
        MI_TRY(hip_rc(launch_g_rmsnorm(dt, ws.xn, h, L.ffn_norm, T, D, m->norm_eps, s), "ffn_norm"));
        const GLinearArgs g = fused(ws.xn, nullptr, L.w1, L.w3, nullptr, 0, 0, ws.a, F, G_EPI_SWIGLU);
        if (g_linear_fused_ok(dt, g)) {
          MI_TRY(hip_rc(launch_g_linear(dt, g, s), "w1|w3 + swiglu"));
        } else {
          MI_TRY(linear(ws.xn, D, L.w1, ws.a, F, F, D, G_EPI_STORE, nullptr, nullptr, "w1"));
          MI_TRY(linear(ws.xn, D, L.w3, ws.b, F, F, D, G_EPI_STORE, nullptr, nullptr, "w3"));
          MI_TRY(hip_rc(launch_g_swiglu(dt, ws.a, ws.b, T, F, nullptr, s), "swiglu"));
        }
      }
      if (!rows16) MI_TRY(linear(ws.a, F, L.w2, h, D, D, F, G_EPI_RESIDUAL, h, nullptr, "w2"));
    } else {
      MI_TRY(hip_rc(launch_g_rmsnorm(dt, ws.xn, h, L.ffn_norm, T, D, m->norm_eps, s), "ffn_norm"));
      // moe.py:24-32: experts in ascending id, each adding round(weight * expert(x)) for the rows that picked it
      const int E = m->num_experts, k = m->top_k;
      if (!L.gate || !L.expert_w_host) return fail(MI_ERR_ARG, "mi_forward_generic: MoE layer tables");
      MI_TRY(linear(ws.xn, D, L.gate, ws.glog, E, E, D, G_EPI_STORE, nullptr, nullptr, "gate"));
      MI_TRY(hip_rc(launch_g_moe_topk(dt, ws.glog, T, E, k, ws.sel_idx, ws.sel_w, s), "moe top-k"));
      MI_TRY(hip_rc(launch_g_zero(dt, ws.res, (size_t)T * D, s), "moe zero"));
      for (int e = 0; e < E; ++e) {
        const void* w1 = L.expert_w_host[e * 3 + 0];
        const void* w2 = L.expert_w_host[e * 3 + 1];
        const void* w3 = L.expert_w_host[e * 3 + 2];
        MI_TRY(hip_rc(launch_g_moe_mask(ws.sel_idx, ws.sel_w, T, k, e, ws.active, ws.wt, s), "moe mask"));
        MI_TRY(linear(ws.xn, D, w1, ws.a, F, F, D, G_EPI_STORE, nullptr, ws.active, "expert w1"));
        MI_TRY(linear(ws.xn, D, w3, ws.b, F, F, D, G_EPI_STORE, nullptr, ws.active, "expert w3"));
        MI_TRY(hip_rc(launch_g_swiglu(dt, ws.a, ws.b, T, F, ws.active, s), "expert swiglu"));
        MI_TRY(linear(ws.a, F, w2, ws.y, D, D, F, G_EPI_STORE, nullptr, ws.active, "expert w2"));
        MI_TRY(hip_rc(launch_g_moe_accum(dt, ws.res, ws.y, ws.active, ws.wt, T, D, s), "moe accumulate"));
      }
      MI_TRY(hip_rc(launch_g_add(dt, h, h, ws.res, (size_t)T * D, s), "moe residual"));
    }
  }

  if (m->final_norm) {
    if (bt->logits) {
      if (rows16) {
        MI_TRY(gemv_passes(kGemvF16, gemv_logits(h, D, m->final_norm, m->norm_eps, m->output, bt->logits, m->vocab_size), T, s,
                           "final norm + lm head (fp16 gemv)"));
      } else if (rows) {
        const GLinearArgs g = fused(h, m->final_norm, m->output, nullptr, nullptr, 0, 0, bt->logits, m->vocab_size, G_EPI_LOGITS);
        MI_TRY(hip_rc(launch_g_linear(dt, g, s), "final norm + lm head"));
      } else {
        MI_TRY(hip_rc(launch_g_rmsnorm(dt, ws.xn, h, m->final_norm, T, D, m->norm_eps, s), "final norm"));
        MI_TRY(linear(ws.xn, D, m->output, bt->logits, m->vocab_size, m->vocab_size, D, G_EPI_LOGITS, nullptr, nullptr, "lm head"));
      }
      if (bi.want_sample) MI_TRY(sample_step(bt, m, bi.want_topp, ws.ctrl, s));
    } else {
      MI_TRY(hip_rc(launch_g_rmsnorm(dt, h, h, m->final_norm, T, D, m->norm_eps, s), "final norm"));
    }
  }
  return MI_OK;
}

}  // extern "C"
