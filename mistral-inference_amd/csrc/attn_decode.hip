// Decode-branch attention: one query per sequence against its rotating K/V ring.
//
// Replaces transformer_layers.py:77-89 at decode: `repeat_kv` (the reference materialises R copies of
// the whole padded ring per token, :16-19,84) plus xformers FMHA under
// BlockDiagonalCausalWithOffsetPaddedKeysMask (cache.py:249-254): sequence b sees ring slots
// [0, min(pos_b + 1, W)) of its own row; slot order is irrelevant (RoPE applied before caching).
//
// HBM-bound (K and V of the ring are read exactly once): grid = (splits, kv_head, sequence); each
// block streams a contiguous slot range for ONE kv head and serves all R = H/Hkv query heads from
// the same registers.  A wave-load covers 4 slots x 256 B; 16 lanes share a slot, scores are reduced
// with DPP row rotations; online softmax is kept per 16-lane group (no cross-lane sync in the loop)
// and merged once at the end: lanes -> waves (LDS) -> splits (global fp32 partials, merged by a second, tiny
// launch: the kernel boundary is the cross-XCD visibility point.  An in-kernel "last block combines" variant with an
// agent-scope release/acquire ticket measured slower than that boundary and was dropped).
//
// The ring element is the kernels' first template argument (attn_split.cuh: RingBf16 / RingE4m3); the block coordinates, the ring
// loads, the partial's store and the merge of the splits are attn_split.cuh's, shared with attn_verify.hip.
#include <cstdlib>

#include "attn_split.cuh"
#include "kernels.h"

namespace {

using namespace attn_split;

// The block's partial in the scratch: acc [b, kvh][split][R][Dh], then (m, l) [b, kvh][split][R][2]
template <int R, class FP>
__device__ __forceinline__ void store_block_partial(float* partial, int B, int Hkv, int n_splits, int b, int kvh, int split, int tid, FP sm_m,
                                                    FP sm_l, FP sm_acc) {
  const int bh = b * Hkv + kvh;
  float* p_acc = partial + ((size_t)bh * n_splits + split) * R * DH;
  float* p_ml = partial + (size_t)B * Hkv * n_splits * R * DH + ((size_t)bh * n_splits + split) * R * 2;
  store_split_partial<R>(tid, sm_m, sm_l, sm_acc, p_acc, p_ml, R);
}

// SMALL (round 5, batches of >= 3 sequences - mistral-demo decodes three): the kernel sits at 170 VGPRs = 2 blocks per CU, so
// 3 x 256 blocks ran as 1.5 rounds of the grid (20.7 us per layer against 9.0 at batch 1).  With half-size load sets (UK = 2:
// 8 instead of 16 KiB in flight per wave) it fits 3 blocks per CU without spilling and the batch is ONE round.  A lane group
// still visits its slots in ascending order: bit-identical results.
template <class Ring, int R, bool SMALL>
__global__ __launch_bounds__(256, SMALL ? 3 : 1) void attn_decode_kernel(AttnDecodeArgs a) {
  typedef typename Ring::raw raw_t;
  __shared__ float sm_m[4 * R];
  __shared__ float sm_l[4 * R];
  __shared__ float sm_acc[4 * R * DH];

  const Coords c(a.Hkv, a.W, a.n_splits);
  const int pos = a.tok_pos[c.b];
  const int kv_len = min(pos + 1, a.W);
  const int s_end = min(c.s_begin + c.chunk, kv_len);

  float qf[R][8];
  {
    u32x4 qraw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) qraw[r] = ld16(a.q + (size_t)c.b * a.ldq + (size_t)(c.kvh * R + r) * DH + c.dl * 8);
    load_q<R>(qf, qraw);
  }
  State<R> st;
  init_state<R>(st);

  const RingSlice<Ring> ring(a.cache_k, a.cache_v, a.kv_layout, a.W, a.Hkv, a.kv_groups, c.b, c.kvh, c.dl);

  // Each lane group walks slots s_begin + wid*4 + g + 16*j, UK slots (K and V rows = 2*UK loads) per step, two
  // steps in flight (ping-pong register sets A/B refilled in place, 16 KiB per wave outstanding): the kernel is pure
  // HBM latency/bandwidth, so depth is what matters.
  constexpr int UK = (R <= 4 && !SMALL) ? 4 : 2;  // R >= 6 needs the registers for its accumulators: half-size sets, no AGPR spills
  const int s_clamp = max(kv_len - 1, 0);
  const int n_steps = (s_end > c.s_begin) ? (s_end - c.s_begin + 16 * UK - 1) / (16 * UK) : 0;  // block-uniform
  // [0, UK): K rows, [UK, 2UK): V rows.  (ONE array per set: with the K and the V rows in arrays of their own, <4, true> came out
  // at 168 VGPRs and 28 bytes of scratch instead of 148 and none.)
  raw_t setA[2 * UK], setB[2 * UK];
  // slots past the block's range are clamped to a valid slot (RingSlice::load) and masked in reduce_step
  auto load_step = [&](int it, raw_t (&kv)[2 * UK]) { ring.template load<UK>(c.s_first + it * 16 * UK, s_clamp, kv, kv + UK); };
  auto reduce_step = [&](int it, const raw_t (&kv)[2 * UK]) {
    const int s0 = c.s_first + it * 16 * UK;
#pragma unroll
    for (int u = 0; u < UK; ++u) reduce_slot<R>(st, qf, Ring::pairs(kv[u]), Ring::pairs(kv[UK + u]), (s0 + 16 * u) < s_end);
  };
  // Two sets in flight.  Steps beyond n_steps reduce nothing (every slot is masked).
  load_step(0, setA);
  load_step(1, setB);
  for (int it = 0; it < n_steps; it += 2) {
    reduce_step(it, setA);
    load_step(it + 2, setA);
    reduce_step(it + 1, setB);
    load_step(it + 3, setB);
  }

  // 4 lane groups -> wave -> LDS
  wave_state_to_lds<R>(st, c.wid, c.lane, sm_m, sm_l, sm_acc);
  __syncthreads();

  // 4 waves -> block partial in global scratch
  store_block_partial<R>(a.partial, a.B, a.Hkv, a.n_splits, c.b, c.kvh, c.split, c.tid, sm_m, sm_l, sm_acc);
}

// ALL-IN form (round 6; batches of >= 3 sequences on rings of <= 4096 slots: 128 slots per block = 8 per lane group): the block's
// whole K/V share - 16 loads per lane - is issued at once and the query heads are served in passes of two over the SAME registers
// (heads do not interact in reduce_slot, a lane group still visits its slots in ascending order: bit-identical results).  The
// SMALL form above walks the same slots in four dependent steps with two in flight: three memory round trips where this has
// one (batch 3: 16.9 us per layer for 50 MB).  Fits 3 blocks per CU.
template <class Ring, int R>
__global__ __launch_bounds__(256, 3) void attn_decode_allin_kernel(AttnDecodeArgs a) {
  static_assert(R == 2 || R == 4, "passes of two query heads");
  __shared__ float sm_m[4 * R];
  __shared__ float sm_l[4 * R];
  __shared__ float sm_acc[4 * R * DH];
  constexpr int NS = 8;  // slots per lane group: 4 waves x 4 groups x 8 = 128 slots per block

  const Coords c(a.Hkv, a.W, a.n_splits);  // chunk <= 128 (decode_form)
  const int pos = a.tok_pos[c.b];
  const int kv_len = min(pos + 1, a.W);
  const int s_end = min(c.s_begin + c.chunk, kv_len);

  u32x4 qraw[R];
#pragma unroll
  for (int r = 0; r < R; ++r) qraw[r] = ld16(a.q + (size_t)c.b * a.ldq + (size_t)(c.kvh * R + r) * DH + c.dl * 8);

  const RingSlice<Ring> ring(a.cache_k, a.cache_v, a.kv_layout, a.W, a.Hkv, a.kv_groups, c.b, c.kvh, c.dl);
  typename Ring::raw kk[NS], vv[NS];  // (slots past the block's range: clamped, masked below)
  ring.template load<NS>(c.s_first, max(kv_len - 1, 0), kk, vv);
#pragma unroll
  for (int rp = 0; rp < R; rp += 2) {
    if (rp > 0) {  // the passes run one after the other on the RAW rows: shared, hipcc keeps every row's 16 converted floats live (145 spills)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NS; ++j) asm volatile("" : "+v"(kk[j]), "+v"(vv[j]));
    }
    float qf[2][8];
    const u32x4 qpair[2] = {qraw[rp], qraw[rp + 1]};
    load_q<2>(qf, qpair);
    State<2> st;
    init_state<2>(st);
#pragma unroll
    for (int j = 0; j < NS; ++j) reduce_slot<2>(st, qf, Ring::pairs(kk[j]), Ring::pairs(vv[j]), (c.s_first + 16 * j) < s_end);
    wave_state_to_lds_heads<2, R>(st, c.wid, c.lane, rp, sm_m, sm_l, sm_acc);
  }
  __syncthreads();

  store_block_partial<R>(a.partial, a.B, a.Hkv, a.n_splits, c.b, c.kvh, c.split, c.tid, sm_m, sm_l, sm_acc);
}

// Second launch: one block per (sequence, q head), one thread per output element (attn_split.cuh: combine_pair).
template <int NS>  // upper bound on n_splits held in registers
__global__ __launch_bounds__(128) void attn_decode_combine_kernel(AttnDecodeArgs a) {
  const int d = threadIdx.x, b = blockIdx.y;
  const int R = a.H / a.Hkv, kvh = blockIdx.x % a.Hkv, r = blockIdx.x / a.Hkv, h = kvh * R + r;  // same XCD as the splits
  const int bh = b * a.Hkv + kvh;
  const float* all_acc = a.partial + (size_t)bh * a.n_splits * R * DH + (size_t)r * DH + d;
  const float* all_ml = a.partial + (size_t)a.B * a.Hkv * a.n_splits * R * DH + (size_t)bh * a.n_splits * R * 2 + r * 2;
  const float o = combine_pair<NS>(all_acc, all_ml, R, a.n_splits);
  reinterpret_cast<bf16_t*>(a.out)[(size_t)b * a.H * DH + (size_t)h * DH + d] = f_to_bf(o);
}

bool allin_enabled() {  // MI_ATTN_ALLIN=0: the stepping form for batches >= 3 (A/B testing)
  static const bool on = [] {
    const char* e = getenv("MI_ATTN_ALLIN");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

// Which kernel serves R query heads per block at batch B with `chunk` slots per block.
enum class Form { STEP, STEP_SMALL, ALLIN };
Form decode_form(int R, int B, int chunk) {
  if (B < 3 || R > 4) return Form::STEP;  // (R >= 6 has no SMALL form: its load sets are half-size already)
  if ((R == 2 || R == 4) && chunk <= 128 && allin_enabled()) return Form::ALLIN;
  return Form::STEP_SMALL;
}

template <class Ring, int R>
void launch_r(const AttnDecodeArgs& a, hipStream_t s) {
  dim3 grid(a.n_splits * a.Hkv, a.B), block(256);
  switch (decode_form(R, a.B, split_chunk(a.W, a.n_splits))) {
    case Form::ALLIN:
      if constexpr (R == 2 || R == 4) hipLaunchKernelGGL((attn_decode_allin_kernel<Ring, R>), grid, block, 0, s, a);
      break;
    case Form::STEP_SMALL: hipLaunchKernelGGL((attn_decode_kernel<Ring, R, (R <= 4)>), grid, block, 0, s, a); break;
    case Form::STEP: hipLaunchKernelGGL((attn_decode_kernel<Ring, R, false>), grid, block, 0, s, a); break;
  }
  if (a.n_splits <= 16) hipLaunchKernelGGL((attn_decode_combine_kernel<16>), dim3(a.H, a.B), dim3(128), 0, s, a);
  else hipLaunchKernelGGL((attn_decode_combine_kernel<32>), dim3(a.H, a.B), dim3(128), 0, s, a);  // n_splits <= 32
}

template <class Ring>
hipError_t launch_ring(const AttnDecodeArgs& a, int R, hipStream_t s) {
  switch (R) {
    case 1: launch_r<Ring, 1>(a, s); break;
    case 2: launch_r<Ring, 2>(a, s); break;
    case 4: launch_r<Ring, 4>(a, s); break;
    case 6: launch_r<Ring, 6>(a, s); break;
    case 8: launch_r<Ring, 8>(a, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

int attn_decode_splits(int W) {
  static int slots = 0;  // minimum ring slots per block; MI_ATTN_SPLIT_SLOTS overrides (tuning)
  if (slots == 0) {
    const char* e = getenv("MI_ATTN_SPLIT_SLOTS");
    slots = e ? atoi(e) : 128;
    if (slots < 16) slots = 128;
  }
  // at most 32 splits (the one-round-trip combine holds 32 partials per thread): widen the blocks beyond that
  int per = slots;
  if ((W + per - 1) / per > 32) per = (((W + 31) / 32) + 15) & ~15;
  int n = (W + per - 1) / per;
  if (n < 1) n = 1;
  return n;
}

size_t attn_decode_partial_floats(int B, int H, int Hkv, int Dh, int W) {
  const int R = H / Hkv;
  return (size_t)B * Hkv * attn_decode_splits(W) * R * (Dh + 2);
}

// Largest per-block query-head count in {8, 6, 4, 2, 1} that divides the GQA ratio: 12 (Mistral-Large) -> 2 groups of 6,
// 16 -> 2 x 8, 3 -> 3 x 1.  Each group is scheduled as a kv head of its own.
int attn_decode_group(int R) {
  for (int g : {8, 6, 4, 2}) if (R % g == 0) return g;
  return 1;
}

hipError_t launch_attn_decode(const AttnDecodeArgs& a_in, hipStream_t s) {
  if (a_in.Dh != DH || a_in.H % a_in.Hkv != 0) return hipErrorInvalidValue;
  AttnDecodeArgs a = a_in;
  const int R = attn_decode_group(a.H / a.Hkv);
  a.kv_groups = (a.H / a.Hkv) / R;
  a.Hkv = a_in.Hkv * a.kv_groups;
  a.kv_layout = a_in.kv_layout & 1;  // the kernels index with the layout bit; the element bit picks their ring
  return (a_in.kv_layout & MI_KV_E4M3) ? launch_ring<RingE4m3>(a, R, s) : launch_ring<RingBf16>(a, R, s);
}
