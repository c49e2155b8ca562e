// What the split-KV kernels (attn_decode.hip: stepping and all-in form; attn_verify.hip) share around the arithmetic of
// attn_decode_core.cuh: the ring element, a block's coordinates, its slice of the K/V ring with the clamped loads, the store of a
// split's partial and the merge of the splits.  The decode engine has its own block structure and does not include this file.
#pragma once
#include "attn_decode_core.cuh"
#include "gemv_core.cuh"  // cvt4_e4m3: e4m3 bytes -> exact bf16 pairs

namespace attn_split {

using namespace attn_core;

// The ring element (MI_KV_E4M3, include/mistral_hip.h).  A lane's piece of a ring row is its 8 head dims: 16 bytes of a bf16 ring,
// 8 bytes of an e4m3 ring, which expand - exactly, every e4m3 value is a bf16 value - to the four bf16 pair words that reduce_slot
// takes.  Everything else (split geometry, slot-to-lane-group mapping, ascending visit order, the arithmetic) does not depend on the
// element, so the result on an e4m3 ring is bit for bit the result on a bf16 ring holding the dequantised values.
struct RingBf16 {
  typedef bf16_t elem;
  typedef u32x4 raw;
  static __device__ __forceinline__ raw load(const elem* p) { return ld16_nt(p); }
  static __device__ __forceinline__ u32x4 pairs(raw r) { return r; }
};
struct RingE4m3 {
  typedef uint8_t elem;
  typedef u32x2 raw;
  static __device__ __forceinline__ raw load(const elem* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)); }
  static __device__ __forceinline__ u32x4 pairs(raw r) {
    uint32_t p[4];
    gemv_core::cvt4_e4m3(r[0], p[0], p[1]);
    gemv_core::cvt4_e4m3(r[1], p[2], p[3]);
    return u32x4{p[0], p[1], p[2], p[3]};
  }
};

// Lane and block coordinates of a split launch: grid (n_splits * Hkv, B), 256 threads.  Lane group g (16 lanes, 8 head dims each)
// of wave wid takes slots s_first + 16 * j of the block's range [s_begin, s_begin + chunk).
struct Coords {
  int tid, lane, wid, g, dl;
  int kvh, split, b;
  int chunk, s_begin, s_first;
  __device__ __forceinline__ Coords(int Hkv, int W, int n_splits) {
    tid = threadIdx.x, lane = tid & 63;
    wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform -> scalar control flow
    g = lane >> 4, dl = lane & 15;
    // Workgroup i runs on XCD i % 8: consecutive ids cycle through the kv heads, so (Hkv = 8) every split of a kv head
    // - and the combine block that merges them - sits on ONE XCD and the fp32 partials are re-read from that XCD's L2.
    kvh = blockIdx.x % Hkv, split = blockIdx.x / Hkv, b = blockIdx.y;
    chunk = split_chunk(W, n_splits);
    s_begin = split * chunk;
    s_first = s_begin + wid * 4 + g;
  }
};

// A lane's view of the K and V ring of (sequence b, kv head kvh): its 8 head dims of slot 0, and the distance between slots.
template <class Ring>
struct RingSlice {
  const typename Ring::elem *k, *v;
  size_t row_stride;
  // `kvh` is a SCHEDULED kv head: when a GQA ratio is split into groups, kv_groups consecutive scheduled heads read the
  // same real head's K/V (the repeat hits the XCD's L2) and own consecutive slices of its query heads.
  __device__ __forceinline__ RingSlice(const void* cache_k, const void* cache_v, int kv_layout, int W, int Hkv, int kv_groups, int b, int kvh,
                                       int dl) {
    const int kv_real = kvh / kv_groups;
    // elements between consecutive slots: a whole row of kv heads in the reference's layout, ONE head row in the head-major
    // layout (common.cuh) - there the four lane groups of a wave read four consecutive slots = one contiguous KiB per load
    const int hkv_real = Hkv / kv_groups;
    row_stride = kv_layout ? (size_t)DH : (size_t)hkv_real * DH;
    const size_t ring0 = kv_offset(kv_layout, W, hkv_real * DH, DH, (size_t)b, 0, kv_real * DH) + dl * 8;
    k = reinterpret_cast<const typename Ring::elem*>(cache_k) + ring0;
    v = reinterpret_cast<const typename Ring::elem*>(cache_v) + ring0;
  }
  // ALWAYS exactly 2 * N unconditional loads (slots past s_clamp are clamped to it, and the caller masks what they hold): no
  // branch around a load, so hipcc's wait for one set leaves another set's loads in flight.
  template <int N>
  __device__ __forceinline__ void load(int s0, int s_clamp, typename Ring::raw* kr, typename Ring::raw* vr) const {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int sl = min(s0 + 16 * j, s_clamp);
      kr[j] = Ring::load(k + (size_t)sl * row_stride);
      vr[j] = Ring::load(v + (size_t)sl * row_stride);
    }
  }
};

// 4 waves (LDS image of wave_state_to_lds) -> the split's partial of N pairs in global fp32: acc [N][DH] at p_acc, (m, l) [N][2]
// at p_ml; pairs from `live` on are not written.
template <int N, class FP>
__device__ __forceinline__ void store_split_partial(int tid, FP sm_m, FP sm_l, FP sm_acc, float* p_acc, float* p_ml, int live) {
  for (int idx = tid; idx < N * DH; idx += 256) {
    const int r = idx / DH;
    if (r >= live) continue;
    float A, M, L;
    split_partial<N>(idx, sm_m, sm_l, sm_acc, A, M, L);
    p_acc[idx] = A;
    if (idx % DH == 0) {
      p_ml[r * 2] = M;
      p_ml[r * 2 + 1] = L;
    }
  }
}

// splits -> one output element of one pair.  All of a thread's loads (the pair's (m, l) - same address across the block, so one
// transaction each - and its own accumulator column) are independent and issued together: one memory round trip instead of a
// chain.  all_acc / all_ml point to split 0; consecutive splits lie `pairs` pairs apart ([pairs][DH] and [pairs][2] floats).
template <int MAXS>  // upper bound on n_splits held in registers
__device__ __forceinline__ float combine_pair(const float* all_acc, const float* all_ml, size_t pairs, int n_splits) {
  float m[MAXS], l[MAXS], v[MAXS];
#pragma unroll
  for (int sp = 0; sp < MAXS; ++sp) {
    const int s2 = min(sp, n_splits - 1);  // clamped, never a conditional load
    const float2 ml = *reinterpret_cast<const float2*>(all_ml + (size_t)s2 * pairs * 2);
    m[sp] = (sp < n_splits) ? ml.x : -1e30f;
    l[sp] = (sp < n_splits) ? ml.y : 0.f;
    v[sp] = all_acc[(size_t)s2 * pairs * DH];
  }
  return combine_splits<MAXS>(m, l, v, n_splits);
}

}  // namespace attn_split
