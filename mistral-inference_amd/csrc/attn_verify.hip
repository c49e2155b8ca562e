// Verify-step attention: m <= 8 consecutive query rows of one sequence against its K/V ring plus the step's own rows.
//
// The mask is mi_attn_prefill's (cache.py:236-248): query row i of sequence b sits at position p_b + i and sees key positions
// kp with p_b + i - W < kp <= p_b + i; kp < p_b come from ring slot kp % W, the rows j <= i of the step from the activations.
// The step's rows are NOT in the ring (a verify step writes them only after acceptance is known), so on a wrapped ring slot
// (p_b + j) % W still holds position p_b + j - W: rows before j read it, rows from j on must not - masking is per (head, row).
//
// Geometry of the decode attention (attn_decode.hip): grid = (splits x kv head, sequence), a block streams its slot range of
// ONE kv head once - slot s_begin + 4 * (wave + 4 j) + lane group, 8 slots per lane group, issued as two unconditional sets of
// eight 16-byte non-temporal loads before anything else (clamped addresses, masked values: no branch around a load) - and
// serves all R * m (query head, row) pairs from those registers in passes of four pairs: 32 accumulator sets do not fit the
// register file, four do, beside the 16 raw rows.  A pass is a lane group's softmax over its nine rows with one validity bit per
// (pair, row), merged as attn_decode_core.cuh merges: lanes -> waves (LDS, double-buffered: one barrier per pass) -> split
// partial (global fp32).
// The last split also folds in the step's own rows (lane group f of the block takes row f) and copies them, K then V, into the
// per-layer stash that the commit kernel (elementwise.hip) reads.  A second launch merges the splits as the decode combine does.
// The block coordinates, the ring loads (through the RingBf16 element: bf16 rings only), the partial's store and the merge of the
// splits are attn_split.cuh's, shared with attn_decode.hip.
#include "attn_split.cuh"
#include "kernels.h"

namespace {

using namespace attn_split;

constexpr int NS = 8;  // ring slots per lane group: 4 waves x 4 groups x 8 = 128 slots per block (launch_attn_verify keeps chunks <= 128)
constexpr int P = 4;   // pairs per pass
typedef float f32x2 __attribute__((ext_vector_type(2)));

// A pass starts from an empty state and sees all of the lane group's slots at once, so its softmax needs no running maximum:
// scores of every slot first (independent chains: one wave per SIMD has nothing else to hide a DPP or v_exp latency behind), the
// exact maximum per pair, then the weights and the p.v sums - no rescale branch.  The sums run on PAIRS of head dims (v_pk_fma_f32).
// Even and odd dims accumulate apart and meet once per score; nothing here has to match another kernel's bits.
__device__ __forceinline__ void unpack(f32x2 (&f)[4], const u32x4 raw) {
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = f32x2{bf_lo(raw[i]), bf_hi(raw[i])};
}
__device__ __forceinline__ float score(const f32x2 (&q)[4], const f32x2 (&k)[4]) {
  f32x2 t = q[0] * k[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) t = q[i] * k[i] + t;
  return row16_sum(t[0] + t[1]);
}

// a row nobody may see (a slot the ring never filled can hold NaN bits, and 0 * NaN is NaN): zeros
__device__ __forceinline__ u32x4 keep_if(u32x4 v, bool keep) {
  return u32x4{keep ? v[0] : 0u, keep ? v[1] : 0u, keep ? v[2] : 0u, keep ? v[3] : 0u};
}

// (one block per CU: 32 splits x 8 kv heads is the grid of a 4096-slot ring at the 7B dims, and the 16 raw rows, the 36 scores and
//  four accumulator sets want more than the 256 registers that two blocks per CU would leave - 53 spills when it was tried)
__global__ __launch_bounds__(256, 1) void attn_verify_kernel(AttnVerifyArgs a) {
  __shared__ float sm_m[2][4 * P];
  __shared__ float sm_l[2][4 * P];
  __shared__ float sm_acc[2][4 * P * DH];

  const Coords c(a.Hkv, a.W, a.n_splits);  // chunk <= 128
  const int R = a.H / a.Hkv;
  const int q0 = a.q_start[c.b], m = a.q_start[c.b + 1] - q0, p = a.kv_before[c.b];
  const int n_pairs = R * m;
  const int s_end = min(c.s_begin + c.chunk, a.W);
  const bool fresh_split = c.split == a.n_splits - 1;

  // ---- the block's whole K/V share, then the step's own rows: every load is issued before the first use
  const RingSlice<RingBf16> ring(a.cache_k, a.cache_v, a.kv_layout, a.W, a.Hkv, 1, c.b, c.kvh, c.dl);
  u32x4 kk[NS], vv[NS];  // set A: j < 4, set B: j >= 4
  ring.load<NS>(c.s_first, a.W - 1, kk, vv);  // every slot of a ring is allocated; what a clamped or unfilled slot holds is masked below
  const int f = c.wid * 4 + c.g;  // the step's own row this lane group takes (rows f >= m: clamped, masked)
  const bf16_t* frow = a.qkv + (size_t)min(q0 + max(min(f, m - 1), 0), a.T - 1) * a.ld + (size_t)a.H * DH + (size_t)c.kvh * DH + c.dl * 8;
  u32x4 fk = ld16(frow), fv = ld16(frow + (size_t)a.Hkv * DH);
  if (fresh_split && f < m && a.stash) {  // K | V of the step's rows, [T, 2 * Hkv * Dh]
    bf16_t* dst = a.stash + (size_t)(q0 + f) * 2 * a.Hkv * DH + (size_t)c.kvh * DH + c.dl * 8;
    st16(dst, fk);
    st16(dst + (size_t)a.Hkv * DH, fv);
  }

  // position held by slot s of a ring whose last written position is p - 1 (negative: never written)
  const int last_slot = (p > 0) ? (p - 1) % a.W : -1;
  const int base_pos = p - 1 - last_slot;
  int kp[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int sl = c.s_first + 16 * j;
    kp[j] = (sl < s_end && p > 0) ? ((sl <= last_slot) ? base_pos + sl : base_pos - a.W + sl) : -1;
    kk[j] = keep_if(kk[j], kp[j] >= 0);
    vv[j] = keep_if(vv[j], kp[j] >= 0);
  }
  const bool f_ok = fresh_split && f < m;
  fk = keep_if(fk, f_ok);
  fv = keep_if(fv, f_ok);

  // q of pair pi = (row pi / R, head kvh * R + pi % R); pairs past n_pairs: clamped, masked
  auto load_q_raw = [&](int pp, u32x4 (&qraw)[P]) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
      const int pi = max(min(pp + r, n_pairs - 1), 0);
      qraw[r] = ld16(a.qkv + (size_t)min(q0 + pi / R, a.T - 1) * a.ld + (size_t)(c.kvh * R + pi % R) * DH + c.dl * 8);
    }
  };
  u32x4 qnext[P];
  load_q_raw(0, qnext);

  const size_t pair0 = (size_t)q0 * R;  // first pair of the sequence among the T * R pairs of this kv head
  const size_t n_all = (size_t)a.T * R;
  float* p_acc = a.partial + (((size_t)c.kvh * a.n_splits + c.split) * n_all + pair0) * DH;
  float* p_ml = a.partial + (size_t)a.Hkv * a.n_splits * n_all * DH + (((size_t)c.kvh * a.n_splits + c.split) * n_all + pair0) * 2;

  int buf = 0;
  for (int pp = 0; pp < n_pairs; pp += P, buf ^= 1) {
    // the passes run on the RAW rows: without this hipcc hoists every row's 16 converted floats out of the loop and spills
#pragma unroll
    for (int j = 0; j < NS; ++j) asm volatile("" : "+v"(kk[j]), "+v"(vv[j]));
    asm volatile("" : "+v"(fk), "+v"(fv));
    f32x2 qf[P][4];  // pre-scaled by Dh^-1/2 * log2(e), as load_q does
    {
      const float sc = rsqrtf((float)DH) * LOG2E;
#pragma unroll
      for (int r = 0; r < P; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) qf[r][i] = f32x2{bf_lo(qnext[r][i]), bf_hi(qnext[r][i])} * f32x2{sc, sc};
    }
    load_q_raw(pp + P, qnext);  // the next pass's q rides behind this pass's arithmetic
    int lo[P], row[P];          // the pair's window: kp > lo; its row among the step's own
#pragma unroll
    for (int r = 0; r < P; ++r) {
      const bool live = pp + r < n_pairs;
      row[r] = live ? (pp + r) / R : -1;
      lo[r] = live ? p + row[r] - a.W : 0x7fffffff;
    }
    // ---- scores of the NS ring slots and of the step's own row, masked per pair
    float d[NS + 1][P];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      f32x2 kf[4];
      unpack(kf, kk[j]);
#pragma unroll
      for (int r = 0; r < P; ++r) {
        const float sc = score(qf[r], kf);  // (unconditional: the DPP sum runs with every lane of the row active)
        d[j][r] = (kp[j] >= 0 && kp[j] > lo[r]) ? sc : -1e30f;
      }
    }
    {
      f32x2 kf[4];
      unpack(kf, fk);
#pragma unroll
      for (int r = 0; r < P; ++r) {
        const float sc = score(qf[r], kf);
        d[NS][r] = (f_ok && f <= row[r] && f > row[r] - a.W) ? sc : -1e30f;
      }
    }
    State<P> st;  // (m, l, acc) of the lane group; the merges are attn_decode_core.cuh's
    f32x2 acc[P][4];
#pragma unroll
    for (int r = 0; r < P; ++r) {
      float mx = d[0][r];
#pragma unroll
      for (int j = 1; j <= NS; ++j) mx = fmaxf(mx, d[j][r]);
      st.m[r] = mx;
      st.l[r] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][i] = f32x2{0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j <= NS; ++j) {
      f32x2 vf[4];
      unpack(vf, j < NS ? vv[j < NS ? j : 0] : fv);  // (j is a compile-time constant here)
#pragma unroll
      for (int r = 0; r < P; ++r) {
        const float p = (d[j][r] > -1e30f) ? ex2(d[j][r] - st.m[r]) : 0.f;  // (a masked score: weight 0, also when every score is masked)
        st.l[r] += p;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][i] = f32x2{p, p} * vf[i] + acc[r][i];
      }
    }
#pragma unroll
    for (int r = 0; r < P; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        st.acc[r][2 * i] = acc[r][i][0];
        st.acc[r][2 * i + 1] = acc[r][i][1];
      }
    wave_state_to_lds<P>(st, c.wid, c.lane, sm_m[buf], sm_l[buf], sm_acc[buf]);
    __syncthreads();
    store_split_partial<P>(c.tid, sm_m[buf], sm_l[buf], sm_acc[buf], p_acc + (size_t)pp * DH, p_ml + (size_t)pp * 2, n_pairs - pp);
  }
}

// Second launch: one block per (row, q head), one thread per output element - the decode combine on the pair's partials.
__global__ __launch_bounds__(128) void attn_verify_combine_kernel(AttnVerifyArgs a) {
  const int d = threadIdx.x, h = blockIdx.x, t = blockIdx.y;
  const int R = a.H / a.Hkv, kvh = h / R, r = h % R;
  const size_t n_all = (size_t)a.T * R, pair = (size_t)t * R + r;
  const float* all_acc = a.partial + ((size_t)kvh * a.n_splits * n_all + pair) * DH + d;
  const float* all_ml = a.partial + (size_t)a.Hkv * a.n_splits * n_all * DH + ((size_t)kvh * a.n_splits * n_all + pair) * 2;
  const float o = combine_pair<32>(all_acc, all_ml, n_all, a.n_splits);  // launch_attn_verify: n_splits <= 32
  reinterpret_cast<bf16_t*>(a.out)[(size_t)t * a.H * DH + (size_t)h * DH + d] = f_to_bf(o);
}

}  // namespace

// 128-slot blocks whatever the ring (the decode attention's default geometry up to 4096 slots); rings beyond 32 such blocks are declined
int attn_verify_splits(int W) { return W > 0 ? (W + 127) / 128 : 1; }

size_t attn_verify_partial_floats(int T, int H, int Dh, int W) { return (size_t)T * H * attn_verify_splits(W) * (Dh + 2); }

hipError_t launch_attn_verify(const AttnVerifyArgs& a_in, hipStream_t s) {
  if (a_in.Dh != DH || a_in.Hkv <= 0 || a_in.H % a_in.Hkv != 0 || a_in.T <= 0 || a_in.B <= 0 || a_in.B > a_in.T) return hipErrorInvalidValue;
  AttnVerifyArgs a = a_in;
  a.kv_layout = a_in.kv_layout & 1;
  a.n_splits = attn_verify_splits(a.W);
  if (a.n_splits > 32 || split_chunk(a.W, a.n_splits) > 16 * NS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_verify_kernel, dim3(a.n_splits * a.Hkv, a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(attn_verify_combine_kernel, dim3(a.H, a.T), dim3(128), 0, s, a);
  return hipGetLastError();
}
