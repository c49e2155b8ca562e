// Host side of the persistent decode engine, compiled once: everything about the engine that is not a kernel body.
//
// decode_engine.hip is compiled once per build (kernels.h: EngineBuild) because the kernels' speed depends on their exact
// instruction stream; each of those objects exports one descriptor.  What a build accepts, how it is launched, the residency
// census, the debug knobs and the order in which a decode step tries the builds are plain host code on those descriptors, and
// live here - one copy of every piece of state, whatever the number of builds in the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "attn_decode_core.cuh"
#include "kernels.h"

// ------------------------------------------------------------------------------------------------ granule layout
namespace {
struct GranLayout {
  uint32_t g_h, g_qkv, g_att, g_h1, g_hid, g_hid2, g_part, g_amax, total;
};
GranLayout gran_layout(int D, int H, int Hkv, int F, int max_splits) {
  using attn_core::DH;
  const int Rtot = H / Hkv, R = attn_decode_group(Rtot), Hs = Hkv * (Rtot / R);
  GranLayout g;
  uint32_t off = 0;
  g.g_h = off;    off += D / 2;
  g.g_qkv = off;  off += (H + 2 * Hkv) * DH / 2;
  g.g_att = off;  off += H * DH / 2;
  g.g_h1 = off;   off += D / 2;
  g.g_hid = off;  off += F / 2;
  g.g_hid2 = off; off += F / 2;  // MoE: hid of the second expert
  g.g_part = off; off += (uint32_t)((size_t)Hs * max_splits * R * (DH + 2));
  g.g_amax = off; off += 4 * AMAX_MAX_NB;  // (max logit, argmax, sum exp, pad) per workgroup
  g.total = off;
  return g;
}
}  // namespace

size_t decode_engine_granule_bytes(int D, int H, int Hkv, int F, int maxW) {
  if (Hkv <= 0 || H % Hkv) return 0;
  (void)maxW;  // sized for the maximum of 32 splits so that the layout depends on the model only
  return (size_t)gran_layout(D, H, Hkv, F, 32).total * 8;
}
size_t decode_engine_trace_bytes(int NB) { return (size_t)NB * ENG_MAXL * TR_EVENTS * sizeof(uint64_t); }

// ------------------------------------------------------------------------------------------------ applicability
// whether the build's kernels take the problem; why (nullable) receives the reason when they do not
static bool decode_engine_applicable(const EngineBuild& b, const EngProblem& pr, char* why, size_t why_len) {
  auto no = [&](const char* m) {
    if (why) snprintf(why, why_len, "%s", m);
    return false;
  };
  using attn_core::DH;
  if (pr.D % 512 || pr.F % 512 || (pr.H * DH) % 512) return no("dim / hidden_dim / n_heads*128 not a multiple of 512");
  if (pr.D > 8192) return no("dim > 8192 (fused RMSNorm holds 4 pieces per thread)");
  // Large dims that are not a multiple of 2048 (Mistral-Nemo: 5120 = rows of 10 pieces, streamed in 2-piece groups, no holder
  // waves): 7.6-8.0 ms per step on the engine against 5.0 ms on the launch path (profiles/EXPERIMENTS.md) - such models
  // take the launch path.  Small dims (the parity tests) stay on the engine.
  // The wide builds stream such rows as contiguous units (Loader::unit) - the third form tried for the Nemo dims, and still
  // slower than the launch path there: 5.47 vs 4.94 ms per step at an 8192-token context (profiles/EXPERIMENTS.md round 4;
  // 2-piece groups: 7.6-8.0 ms, 4 + 4 + 2 groups: 5.62 ms).  Declined unless the caller forces the wide build (traces, tests).
  // (headline_only 2: the `nemo` build exists for exactly these dims)
  if (b.headline_only != 2 && pr.D > 3072 && ((pr.D >> 9) & 3) != 0 && !(b.wide && pr.forced))
    return no("dim > 3072 and not a multiple of 2048: the launch path is faster (Nemo dims)");
  if (b.wide && ((pr.D >> 9) & 1) && pr.D > 3072) return no("odd number of 512-element pieces per row at a large dim");
  if (pr.V % 2) return no("odd vocab");
  if (b.headline_only == 1) {
    if (pr.E || pr.H != 4 * pr.Hkv || pr.D % 2048 || (pr.H * DH) % 2048 || pr.F % 2048)
      return no("this build instantiates the dense GQA-4 kernel for rows of 4-piece groups only");
  } else if (b.headline_only == 2) {
    if (pr.E || pr.H != 4 * pr.Hkv || !(pr.D % 2048 || (pr.H * DH) % 2048 || pr.F % 2048) || pr.D <= 3072)
      return no("this build instantiates the dense GQA-4 kernel for large dims whose rows are not all 4-piece groups only (Mistral-Nemo)");
  } else if (b.wide == 2) {
    if (!pr.E) return no("the 8-fill MoE build takes MoE models only");
  }
  const int kmax = pr.D > pr.F ? (pr.D > pr.H * DH ? pr.D : pr.H * DH) : (pr.F > pr.H * DH ? pr.F : pr.H * DH);
  const size_t region = (size_t)b.lds_total - b.ring_fills * b.fill * b.piece - b.xs_off;  // activation vector / attention scratch
  if ((size_t)kmax * 2 > region) return no("activation vector does not fit beside the 8-fill ring");
  if (pr.E) {
    if (pr.E > 16 || pr.top_k != 2) return no("MoE: at most 16 experts, top-2 routing");
    if (b.wide) {
      if ((size_t)pr.D * 6 > region) return no("MoE: normalised + raw + router-normalised activation vector");
    } else {
      if ((size_t)pr.D * 4 > region) return no("MoE: normalised + raw activation vector");
    }
    if ((size_t)pr.F * 2 + (size_t)((pr.D / 2 + pr.NB - 1) / pr.NB) * 8 > region) return no("MoE: hid vector + per-unit partial sums");
  }
  if ((size_t)pr.D * 2 + (size_t)((pr.V / 2 + pr.NB - 1) / pr.NB) * 8 + 16 + (size_t)pr.NB * 16 > region)
    return no("LM-head logits stash + greedy reduction staging");
  const int NB = pr.NB;
  if (NB < 8 || NB > 1024) return no("CU count");
  if (((pr.D / 2 + NB - 1) / NB) * 2 * 2 > b.res_bytes) return no("residual slab");
  if (pr.Hkv <= 0 || pr.H % pr.Hkv) return no("heads");
  const int Rtot = pr.H / pr.Hkv;
  const int R = attn_decode_group(Rtot);
  if (b.wide == 2) {
    if (R != 4) return no("GQA group size (the 8-fill MoE build instantiates 4)");
  } else if (b.wide) {
    if (R != 4 && R != 6) return no("GQA group size (the wide build instantiates 4 and 6)");
  } else {
    if (R != 1 && R != 2 && R != 4 && R != 8) return no("GQA group size");
  }
  const int Hs = pr.Hkv * (Rtot / R);
  const int ne_max = ((pr.H * DH / 2 + NB - 1) / NB) * 2;
  if (ne_max > 64) return no("split-merge slab");
  if (b.wide) {
    // q (R*64 words) | k, v of this step (128 words) | m, l (8R floats) | acc (4 R DH floats) | merge staging (3 * 32 * ne words)
    if ((size_t)R * 256 + 512 + (size_t)R * 32 + (size_t)4 * R * DH * 4 + (size_t)3 * 32 * ne_max * 4 > region) return no("attention scratch");
  } else {
    if ((size_t)R * (256 + 2 * DH * 16 + 32) + 512 + (size_t)3 * 32 * ne_max * 4 > region) return no("attention scratch");
  }
  for (int l = 0; l < pr.n_layers; ++l) {
    const int ns = attn_decode_splits(pr.W[l]);
    if (ns > 32 || Hs * ns > NB) return no("more attention work items than CUs");
    // ratio 6 serves its heads in two passes over K/V pieces that must all sit in the LDS ring (run_consumer)
    if (b.wide && R == 6 && 2 * ((attn_core::split_chunk(pr.W[l], ns) + 3) >> 2) > (b.ring_fills - 2) * b.fill)
      return no("GQA ratio 6: ring longer than 5120 slots");
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ knobs
namespace {
std::mutex g_mu;  // the two tables below (census verdicts, LDS opt-ins)
uint64_t* g_trace = nullptr;
int g_thin = -1, g_depth = -1, g_holders = -1;  // -1: not read yet (the environment, then the default)

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
}  // namespace

void decode_engine_set_holders(int on) { g_holders = on; }
void decode_engine_set_knobs(int thin, int depth) {
  g_thin = thin;
  g_depth = depth;
}
void decode_engine_set_trace(void* dev_buffer) { g_trace = (uint64_t*)dev_buffer; }

// ---- residency census (once per device, launch shape and process, outside any stream capture) -----------------------------
// The engine's hand-offs need all NB workgroups resident at once.  hipOccupancy... answers for an empty device; a CU mask,
// a partition mode or a co-tenant kernel changes the real answer, and a plain launch applies no check (MI355X_MICROARCH.md
// "Residency and cooperative launch").  So before the engine is used on a device the first time, a probe kernel with the
// engine's exact launch shape (512 threads, 160 KiB LDS - the same for every shipped build, so one probe answers for all) is
// run: every workgroup counts itself in and waits (bounded) for the others.  A failed census disables the engine for this
// device - the launch path is bit-identical and needs nothing.
// The per-step residency gate in the kernel covers what changes later (run_consumer).
__global__ __launch_bounds__(1024, 1) void engine_census_kernel(uint32_t* words, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  (void)smem;
  if (threadIdx.x != 0) return;
  __hip_atomic_fetch_add(words, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t polls = 0; polls < ARRIVE_POLLS; ++polls) {
    if (__hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (uint32_t)nb) return;
    __builtin_amdgcn_s_sleep(8);
  }
  __hip_atomic_store(words + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // somebody never showed up
}

namespace {
struct Census {
  int dev, threads, lds;
  int verdict;  // 1 passed, -1 failed
};
std::vector<Census> g_census;
char g_census_why[160] = "";

// 1 passed, -1 failed, 0 unknown (cannot probe now)
int engine_census(int dev, int threads, int lds, int nb, uint32_t* ctrl, hipStream_t s) {
  if (dev < 0 || dev >= 64) return -1;
  std::lock_guard<std::mutex> lock(g_mu);
  for (const Census& c : g_census)
    if (c.dev == dev && c.threads == threads && c.lds == lds) return c.verdict;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return 0;  // cannot probe now
  auto verdict = [&](int v) {
    g_census.push_back({dev, threads, lds, v});
    return v;
  };
  const void* fn = (const void*)engine_census_kernel;
  int per_cu = 0;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu < 1) {
    snprintf(g_census_why, sizeof(g_census_why), "occupancy query: %d workgroups of %d threads + %d B LDS per CU", per_cu, threads, lds);
    return verdict(-1);
  }
  uint32_t* words = ctrl + CTRL_CENSUS0;  // two spare control words of the caller's workspace (the ABI never allocates)
  uint32_t host[2] = {0, 0};
  bool ok = hipMemsetAsync(words, 0, 8, s) == hipSuccess;
  if (ok) {
    void* params[] = {(void*)&words, (void*)&nb};
    ok = hipLaunchKernel(fn, dim3(nb), dim3(threads), params, lds, s) == hipSuccess &&
         hipMemcpyAsync(host, words, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  if (!ok || host[1] != 0 || host[0] != (uint32_t)nb) {
    snprintf(g_census_why, sizeof(g_census_why), "census: %u of %d workgroups resident together (CU mask / partition / co-tenant?)",
             host[0], nb);
    return verdict(-1);
  }
  return verdict(1);
}
}  // namespace

const char* decode_engine_census_detail() { return g_census_why; }
void decode_engine_forget_census() {
  std::lock_guard<std::mutex> lock(g_mu);
  g_census.clear();
}

// ------------------------------------------------------------------------------------------------ launch
// *declined = true (and nothing enqueued): the residency census failed on this device - the caller takes the launch path
static hipError_t launch_decode_engine(const EngineBuild& b, const EngProblem& pr, hipStream_t s, bool* declined) {
  if (declined) *declined = false;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (engine_census(dev, b.nthreads, b.lds_total, pr.NB, pr.ctrl, s) < 0) {  // not all workgroups can be resident
    if (declined) *declined = true;
    return hipSuccess;
  }
  EngArgs a;
  memset(&a, 0, sizeof(a));
  a.trace = (unsigned long long*)g_trace;
  if (g_thin < 0) g_thin = env_int("MI_ENGINE_THIN", 2);     // 0 stream through sweeps, 1 one fill in flight, 2 stop (measured best)
  if (g_depth < 0) g_depth = env_int("MI_ENGINE_DEPTH", 2);  // measured: 2 fills in flight (plus the one being issued) beats 3
  if (g_holders < 0) g_holders = env_int("MI_ENGINE_HOLDERS", 1) != 0;
  a.thin = g_thin;
  a.depth = g_depth;
  a.holders = g_holders;
  a.D = pr.D; a.H = pr.H; a.Hkv = pr.Hkv; a.F = pr.F; a.V = pr.V; a.eps = pr.eps; a.NB = pr.NB;
  const int Rtot = pr.H / pr.Hkv;
  a.R = attn_decode_group(Rtot);
  a.kv_groups = Rtot / a.R;
  a.Hs = pr.Hkv * a.kv_groups;
  a.ring_fills = b.ring_fills;
  a.h = (bf16_t*)pr.h; a.rope_cs = pr.rope_cs;
  a.kv_seqlens = pr.kv_seqlens; a.q_start = pr.q_start; a.kv_before = pr.kv_before; a.tok_seq = pr.tok_seq; a.tok_pos = pr.tok_pos;
  a.final_norm = (const bf16_t*)pr.final_norm; a.output = (const bf16_t*)pr.output; a.logits = pr.logits;
  a.gran = (uint64_t*)pr.granules; a.ctrl = pr.ctrl;
  const GranLayout gl = gran_layout(pr.D, pr.H, pr.Hkv, pr.F, 32);
  a.g_h = gl.g_h; a.g_qkv = gl.g_qkv; a.g_att = gl.g_att; a.g_h1 = gl.g_h1; a.g_hid = gl.g_hid; a.g_part = gl.g_part;
  a.g_amax = gl.g_amax; a.g_hid2 = gl.g_hid2; a.E = pr.E;
  if ((size_t)gl.total * 8 > pr.granule_bytes || !pr.kv_seqlens) return hipErrorInvalidValue;

  const bool moe = pr.E > 0;
  const bool all4 = b.all4 && pr.D % 2048 == 0 && (pr.H * attn_core::DH) % 2048 == 0 && pr.F % 2048 == 0;
  const void* fn = b.kernel(a.R, moe, all4);
  if (!fn) return hipErrorInvalidValue;
  {  // 160 KiB of dynamic LDS is an opt-in per function AND per device
    static std::vector<std::pair<int, const void*>> opted_in;
    std::lock_guard<std::mutex> lock(g_mu);
    bool have = false;
    for (const auto& o : opted_in) have = have || (o.first == dev && o.second == fn);
    if (!have) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, b.lds_total);
      if (e != hipSuccess) return e;
      opted_in.push_back({dev, fn});
    }
  }
  for (int l0 = 0; l0 < pr.n_layers; l0 += ENG_MAXL) {
    const int nl = pr.n_layers - l0 < ENG_MAXL ? pr.n_layers - l0 : ENG_MAXL;
    const bool last = l0 + nl == pr.n_layers;
    a.n_layers = nl;
    a.seq_base = l0;
    a.first = 1;  // every launch starts from the residual stream in global memory (the first one: or the embedding row)
    a.emb = l0 == 0 ? (const bf16_t*)pr.emb : nullptr;
    a.ids = pr.ids;
    a.commit = last;
    a.head = last && pr.logits != nullptr;
    const bool greedy = a.head && pr.greedy_tok && pr.greedy_lp;
    a.greedy_tok = greedy ? pr.greedy_tok : nullptr;
    a.greedy_lp = greedy ? pr.greedy_lp : nullptr;
    a.hist_tok = greedy && pr.hist_lp ? pr.hist_tok : nullptr;
    a.hist_lp = greedy && pr.hist_tok ? pr.hist_lp : nullptr;
    a.hist_len = pr.hist_len;
    for (int l = 0; l < nl; ++l) {
      const mi_layer_t& M = pr.layers[l0 + l];
      EngLayer& L = a.L[l];
      L.an = (const bf16_t*)M.attention_norm; L.wq = (const bf16_t*)M.wq; L.wk = (const bf16_t*)M.wk;
      L.wv = (const bf16_t*)M.wv; L.wo = (const bf16_t*)M.wo; L.fn = (const bf16_t*)M.ffn_norm;
      if (pr.E) {  // MoE layers: the gate in the w1 slot, the DEVICE table [E][3] of expert matrices in the w2 slot
        L.w1 = (const bf16_t*)M.gate; L.w2 = (const bf16_t*)M.expert_w_dev; L.w3 = nullptr;
      } else {
        L.w1 = (const bf16_t*)M.w1; L.w2 = (const bf16_t*)M.w2; L.w3 = (const bf16_t*)M.w3;
      }
      L.ck = (bf16_t*)pr.cache_k[l0 + l]; L.cv = (bf16_t*)pr.cache_v[l0 + l];
      L.W = pr.W[l0 + l];
      L.kv_layout = pr.kv_layout;
      L.n_splits = attn_decode_splits(L.W);
      L.chunk = attn_core::split_chunk(L.W, L.n_splits);
    }
    void* params[] = {(void*)&a};
    hipError_t e = hipLaunchKernel(fn, dim3(pr.NB), dim3(b.nthreads), params, b.lds_total, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ routing
// Every compile of the kernel source (kernels.h: EngineBuild).  Experiment libraries (scripts/build_variants.py engine_slots ->
// -DMI_SLOT_LIST="X(0) X(1) ..." on this file) append further compiles under the names *_x<N>, selected at run time by
// mi_debug_set_engine_slot (scripts/engine_ab.py: one process, one set of weights, every slot timed in turn on the same box).
#ifdef MI_SLOT_LIST
#define X(n) const EngineBuild& decode_engine_build_x##n();
MI_SLOT_LIST
#undef X
#define X(n) &decode_engine_build_x##n(),
#define ENGINE_SLOTS MI_SLOT_LIST
#else
#define ENGINE_SLOTS
#endif

namespace {
enum { B_DEFAULT, B_NEXT, B_NEMO, B_WIDE, B_MOE, N_SHIPPED };
const EngineBuild* const kBuilds[] = {&decode_engine_build(), &decode_engine_build_next(), &decode_engine_build_nemo(),
                                      &decode_engine_build_wide(), &decode_engine_build_moe(), ENGINE_SLOTS};
constexpr int N_SLOTS = (int)(sizeof(kBuilds) / sizeof(kBuilds[0])) - N_SHIPPED;
int g_slot = -1;  // experiment slot that a step tries first (-1: none)

bool nemo_engine_enabled() {
  // measured (round 6): 5.15-5.17 ms per step against 4.94-4.95 on the launch path at the Nemo-12B dims
  static const bool on = env_int("MI_ENGINE_NEMO", 0) != 0;
  return on;
}
int g_engine_variant = -1;  // 0 (default): the shipped engine build first (MoE: the wide build first); 1: wide first; 2: shipped first
int engine_variant() {
  if (g_engine_variant < 0) g_engine_variant = env_int("MI_ENGINE_VARIANT", 0);
  return g_engine_variant;
}

// Which builds a batch-1 decode step tries, in order: calls try_build(build) for each applicable one until it returns true (the
// step is finished, or failed); a build whose launch declined (residency census) returns false and the next stage is asked.
// Lazy: on the headline model `next` is the only applicable build asked per step.  variant: mi_debug_set_engine_variant.
// Returns whether a try_build returned true (false: take the launch path).
template <class Try>
bool engine_route(int variant, bool nemo_opt_in, const EngineBuild* slot, EngProblem pr, Try&& try_build) {
  const bool moe = pr.E > 0;
  pr.forced = variant == 1;
  if (pr.lora_rank > 0) return false;  // un-merged LoRA adapters: no engine build carries them, the launch path does (lora.hip)
  if (pr.quant) return false;          // quantised weight bytes: no engine build reads them, the launch path does (gemv_w8.hip, gemv_w4.hip)
  if (pr.kv_layout & MI_KV_E4M3) return false;  // K/V rings of e4m3 bytes: no engine build reads them, the launch path does (attn_decode.hip)
  auto takes = [&](int b) { return decode_engine_applicable(*kBuilds[b], pr, nullptr, 0); };
  auto run = [&](const EngineBuild& b) { return try_build(b, pr); };
  if (slot && decode_engine_applicable(*slot, pr, nullptr, 0) && run(*slot)) return true;
  // the dense GQA-4 headline shapes: the `next` compile (build_native.ENGINE_NEXT_FLAGS)
  if (!moe && variant == 0 && takes(B_NEXT) && run(*kBuilds[B_NEXT])) return true;
  // large dims whose rows are not multiples of 4 pieces (Mistral-Nemo): the `nemo` compile - bit-equal, in a clean regime
  // (scripts/engine_loader_waits.py) and still 4 % slower than the launch path at those dims (contiguous 20- / 40-piece units:
  // four consumer waves cannot all hold one in the 128-piece ring), so it is opt-in: MI_ENGINE_NEMO=1 or engine variant 3 (tests)
  if (!moe && (variant == 3 || (variant == 0 && nemo_opt_in)) && takes(B_NEMO) && run(*kBuilds[B_NEMO])) return true;
  // Exactly one of the rest.  MoE models: the 8-fill MoE build where the model fits it (Mixtral-8x7B), else the 7-fill wide build
  // (Mixtral-8x22B) wherever it applies - both carry the round-4 router (two experts per wave, batched loads: -8..-11 us per
  // layer), which the default object - frozen, see decode_engine.hip - does not.  Dense models: the default build, and the wide
  // one for what it declines (GQA ratio 6; rows of 10 pieces when forced).  Variant 1 (tests) prefers the wide build wherever
  // it applies, so that its code paths can be compared bit for bit at small sizes; variant 2 = default build first for every model.
  const bool wide_first = variant == 1 || (variant == 0 && moe);
  const int last = (moe && variant == 0 && takes(B_MOE)) ? B_MOE
                   : (wide_first && takes(B_WIDE))       ? B_WIDE
                   : takes(B_DEFAULT)                    ? B_DEFAULT
                   : (!wide_first && takes(B_WIDE))      ? B_WIDE
                                                         : -1;
  return last >= 0 && run(*kBuilds[last]);
}
}  // namespace

EngStep decode_engine_step(const EngProblem& pr, hipStream_t s) {
  EngStep r = {false, hipSuccess, "decode engine", false};
  for (int l = 0; l < pr.n_layers; ++l) {  // every layer carries the weights the kernels read
    const mi_layer_t& M = pr.layers[l];
    if (!(pr.E ? (M.gate && M.expert_w_dev) : (M.w1 && M.w2 && M.w3))) return r;
  }
  const EngineBuild* slot = g_slot >= 0 ? kBuilds[N_SHIPPED + g_slot] : nullptr;
  r.ran = engine_route(engine_variant(), nemo_engine_enabled(), slot, pr, [&](const EngineBuild& b, const EngProblem& p) {
    bool declined = false;  // true: the step is finished, r.err says how; false: the build declined
    r.err = launch_decode_engine(b, p, s, &declined);
    r.what = &b == slot ? "decode engine (experiment slot)" : "decode engine";
    if (r.err == hipSuccess && declined) {
      if (&b != slot) r.declined = true;
      return false;
    }
    return true;
  });
  return r;
}

size_t decode_engine_route_names(int D, int H, int Hkv, int F, int V, int E, int top_k, int n_layers, int cache_size, int NB,
                                 int variant, bool nemo_opt_in, char* out, size_t out_len) {
  const std::vector<int32_t> W(n_layers, cache_size);
  EngProblem pr;
  memset(&pr, 0, sizeof(pr));
  pr.D = D; pr.H = H; pr.Hkv = Hkv; pr.F = F; pr.V = V; pr.n_layers = n_layers; pr.NB = NB;
  pr.E = E; pr.top_k = top_k; pr.W = W.data();
  size_t n = 0;
  out[0] = 0;
  engine_route(variant, nemo_opt_in, nullptr, pr, [&](const EngineBuild& b, const EngProblem&) {  // "declined": the whole chain is listed
    if (n < out_len) n += snprintf(out + n, out_len - n, "%s%s", n ? "," : "", b.name);
    return false;
  });
  return n;
}

int decode_engine_set_variant(int variant) {
  const int prev = engine_variant();
  g_engine_variant = variant < 0 || variant > 3 ? 0 : variant;
  return prev;
}

#ifdef MI_SLOT_LIST
extern "C" int mi_debug_set_engine_slot(int slot) {  // -1: the library's own routing; returns the number of slots
  g_slot = slot < 0 || slot >= N_SLOTS ? -1 : slot;
  return N_SLOTS;
}
#endif
