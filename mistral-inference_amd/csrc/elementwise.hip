// Memory-bound elementwise / row kernels of the hot path.  All bf16 traffic is 16 bytes per lane.
#include "common.cuh"
#include "gemv_core.cuh"  // cvt4_e4m3: e4m3 bytes -> exact bf16 pairs
#include "kernels.h"

namespace {

// transformer.py:193
// An id outside [0, vocab) makes nn.Embedding raise (reference transformer.py:193).  A kernel cannot raise: it records
// 1 + the token index in *bad_id (when given), reads row 0 / vocab-1 instead of faulting, and the host turns the flag
// into the IndexError at its next synchronisation point (ids that live on the host are checked before the launch).
__device__ __forceinline__ long checked_id(long id, int vocab, int t, uint32_t* bad_id) {
  if (id < 0 || id >= vocab) {
    if (bad_id && threadIdx.x == 0) atomicMax(bad_id, (uint32_t)t + 1u);
    id = id < 0 ? 0 : vocab - 1;
  }
  return id;
}

__global__ __launch_bounds__(256) void embedding_kernel(bf16_t* out, const bf16_t* table, const int64_t* ids, int D,
                                                        int vocab, uint32_t* bad_id) {
  const int t = blockIdx.x;
  const long id = checked_id(ids[t], vocab, t, bad_id);
  const bf16_t* src = table + (size_t)id * D;
  bf16_t* dst = out + (size_t)t * D;
  for (int p = threadIdx.x; p < (D >> 3); p += 256) st16(dst + p * 8, ld16(src + p * 8));
}

// transformer_layers.py:115-120.  One WAVE per row (4 rows per block): the row sits in registers between the two passes,
// the sum of squares is a wave reduction - no LDS, no barrier - and every lane's NP 16-byte loads are issued
// unconditionally from clamped addresses before anything waits (a `p < np ? load : 0` form costs a branch and a full
// vmcnt drain per load, cdna_hip_programming.md ".s-level traps" (c)).
template <int NP>  // 16-byte pieces per lane: D <= 64 * 8 * NP
__global__ __launch_bounds__(256) void rmsnorm_kernel(bf16_t* out, const bf16_t* x, const bf16_t* w, int T, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= T) return;
  const bf16_t* xr = x + (size_t)t * D;
  const int np = D >> 3;
  u32x4 v[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) v[j] = ld16(xr + min(lane + j * 64, np - 1) * 8);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = bf_lo(v[j][i]), b = bf_hi(v[j][i]);
      s = fmaf(a, a, s);
      s = fmaf(b, b, s);
    }
    ss += (lane + j * 64 < np) ? s : 0.f;
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / sqrtf(ss / (float)D + eps);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + j * 64;
    if (p < np) {
      const u32x4 wv = ld16(w + p * 8);
      u32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = pack_bf2(bf_round(bf_lo(v[j][i]) * inv) * bf_lo(wv[i]), bf_round(bf_hi(v[j][i]) * inv) * bf_hi(wv[i]));
      st16(out + (size_t)t * D + p * 8, o);
    }
  }
}

// ---- per-token e4m3 quantisation of activation rows (W8A8 prefill, kernels.h launch_act_quant_e4m3): the rule of
// mistral_inference.quant.quantize_rows in the same integer-exponent arithmetic, so the CPU and the device give the same bytes.
// One wave per row as rmsnorm_kernel, the row in registers: one pass over the row, 16-byte loads, 8-byte stores.  NORM: the row
// quantised is the bf16 row rmsnorm_kernel writes (the same operations in the same order, then pack_bf2's rounding).
__device__ __forceinline__ float aq_clamp(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
__device__ __forceinline__ uint32_t aq_stepdown(uint32_t w) {  // codes of magnitude >= 256 step down (a scale of 2^120 only)
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (((w >> (8 * b)) & 0x7fu) >= 0x78u) w -= 1u << (8 * b);
  return w;
}
template <int NP, bool NORM>
__global__ __launch_bounds__(256) void act_quant_e4m3_kernel(uint8_t* xq, float* sx, const bf16_t* x, int ldx, const bf16_t* w, int T,
                                                             int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= T) return;
  const bf16_t* xr = x + (size_t)t * ldx;
  const int np = D >> 3;
  u32x4 v[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) v[j] = ld16(xr + min(lane + j * 64, np - 1) * 8);
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = bf_lo(v[j][i]), b = bf_hi(v[j][i]);
        s = fmaf(a, a, s);
        s = fmaf(b, b, s);
      }
      ss += (lane + j * 64 < np) ? s : 0.f;
    }
    ss = wave_sum(ss);
    const float inv = 1.0f / sqrtf(ss / (float)D + eps);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const u32x4 wv = ld16(w + min(lane + j * 64, np - 1) * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[j][i] = pack_bf2(bf_round(bf_lo(v[j][i]) * inv) * bf_lo(wv[i]), bf_round(bf_hi(v[j][i]) * inv) * bf_hi(wv[i]));
    }
  }
  // amax over bf16 magnitudes is a maximum over their 15-bit patterns
  uint32_t am = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m = max(m, max(v[j][i] & 0x7fffu, (v[j][i] >> 16) & 0x7fffu));
    am = max(am, (lane + j * 64 < np) ? m : 0u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  const float amax = __uint_as_float(am << 16);
  // amax = mant * 2^ex, mant in [0.5, 1);  amax / 448 = (2 mant / 1.75) * 2^(ex - 9)
  int ex = 0;
  const float mant = frexpf(amax, &ex);
  const int e = am == 0 ? 0 : ex - 9 + (mant > 0.875f ? 1 : 0);
  if (lane == 0) sx[t] = ldexpf(1.0f, e);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + j * 64;
    if (p < np) {
      u32x2 o;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t p0 = v[j][2 * i], p1 = v[j][2 * i + 1];
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(aq_clamp(ldexpf(bf_lo(p0), -e)), aq_clamp(ldexpf(bf_hi(p0), -e)), 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(aq_clamp(ldexpf(bf_lo(p1), -e)), aq_clamp(ldexpf(bf_hi(p1), -e)), c, true);
        o[i] = e >= 120 ? aq_stepdown((uint32_t)c) : (uint32_t)c;
      }
      *reinterpret_cast<u32x2*>(xq + (size_t)t * D + p * 8) = o;
    }
  }
}

// rope.py:13-23, in place on the q|k columns of the fused buffer.  One thread rotates 4 adjacent pairs.
__global__ __launch_bounds__(256) void rope_kernel(bf16_t* qkv, int ld, int T, int n_rot_cols, int Dh,
                                                   const float* rope_cs, const int32_t* tok_pos) {
  const int pieces_per_row = n_rot_cols >> 3;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)T * pieces_per_row) return;
  const int t = (int)(gid / pieces_per_row), p = (int)(gid % pieces_per_row);
  const int col = p * 8;
  const int i0 = (col % Dh) >> 1;
  bf16_t* ptr = qkv + (size_t)t * ld + col;
  const u32x4 v = ld16(ptr);
  const float* cs = rope_cs + ((size_t)tok_pos[t] * (Dh >> 1) + i0) * 2;
  const f32x4 c01 = *reinterpret_cast<const f32x4*>(cs);
  const f32x4 c23 = *reinterpret_cast<const f32x4*>(cs + 4);
  const float cc[4] = {c01[0], c01[2], c23[0], c23[2]};
  const float sn[4] = {c01[1], c01[3], c23[1], c23[3]};
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = bf_lo(v[i]), b = bf_hi(v[i]);
    float re, im;
    rope_pair(a, b, cc[i], sn[i], re, im);
    o[i] = pack_bf2(re, im);
  }
  st16(ptr, o);
}

// cache.py:83-92 + 226-235
__global__ __launch_bounds__(256) void kv_write_kernel(bf16_t* ck, bf16_t* cv, int W, const bf16_t* k, const bf16_t* v,
                                                       int ld, int T, int kv_dim, const int32_t* tok_seq,
                                                       const int32_t* tok_pos, const int32_t* q_start, int layout, int Dh) {
  const int pieces = kv_dim >> 3;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)T * pieces) return;
  const int t = (int)(gid / pieces), p = (int)(gid % pieces);
  const int b = tok_seq[t];
  const int i = t - q_start[b];
  const int s = q_start[b + 1] - q_start[b];
  if (i < s - W) return;  // to_cache_mask: only the last W tokens of the chunk are stored
  const size_t off = kv_offset(layout, W, kv_dim, Dh, (size_t)b, tok_pos[t] % W, p * 8);  // (Dh % 8 == 0: a piece stays inside a head)
  st16(ck + off, ld16(k + (size_t)t * ld + p * 8));
  st16(cv + off, ld16(v + (size_t)t * ld + p * 8));
}

// ---- FP8 K/V rings (include/mistral_hip.h: MI_KV_E4M3).  Write rule: byte = e4m3_rne(clamp(float(x), -448, 448)), a NaN stays a
// NaN - in torch x.float().clamp(-448, 448).to(torch.float8_e4m3fn), mistral_inference.cache.kv_quantize.
// v_max / v_min drop a NaN operand (IEEE maxNum), so the NaN code (0x7f under the input's sign, what torch's cast gives) is set
// on the converted bytes.
__device__ __forceinline__ float kv8_clamp(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
__device__ __forceinline__ uint32_t kv8_nan_fix(uint32_t w, uint32_t pair, int byte) {
  const uint32_t lo = pair << 16, hi = pair & 0xffff0000u;  // the two bf16 values as fp32 bits
  if ((lo & 0x7fffffffu) > 0x7f800000u) w = (w & ~(0xffu << (8 * byte))) | ((0x7fu | (lo >> 24 & 0x80u)) << (8 * byte));
  if ((hi & 0x7fffffffu) > 0x7f800000u) w = (w & ~(0xff00u << (8 * byte))) | ((0x7f00u | (hi >> 16 & 0x8000u)) << (8 * byte));
  return w;
}
// eight bf16 (four pair words) -> eight e4m3 bytes
__device__ __forceinline__ u32x2 kv8_pack(u32x4 v) {
  u32x2 o;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t p0 = v[2 * i], p1 = v[2 * i + 1];
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(bf_lo(p0)), kv8_clamp(bf_hi(p0)), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(bf_lo(p1)), kv8_clamp(bf_hi(p1)), w, true);
    o[i] = kv8_nan_fix(kv8_nan_fix((uint32_t)w, p0, 0), p1, 2);
  }
  return o;
}
// kv_write_kernel with e4m3 rings: 16 bytes in, 8 bytes out per lane; the same window-drop rule
__global__ __launch_bounds__(256) void kv_write_e4m3_kernel(uint8_t* ck, uint8_t* cv, int W, const bf16_t* k, const bf16_t* v,
                                                            int ld, int T, int kv_dim, const int32_t* tok_seq,
                                                            const int32_t* tok_pos, const int32_t* q_start, int layout, int Dh) {
  const int pieces = kv_dim >> 3;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)T * pieces) return;
  const int t = (int)(gid / pieces), p = (int)(gid % pieces);
  const int b = tok_seq ? tok_seq[t] : t;
  if (q_start) {  // (nullptr: every row is stored - the q|k|v leaves, whose fused write has no window rule either)
    const int i = t - q_start[b];
    const int s = q_start[b + 1] - q_start[b];
    if (i < s - W) return;  // to_cache_mask: only the last W tokens of the chunk are stored
  }
  const size_t off = kv_offset(layout, W, kv_dim, Dh, (size_t)b, tok_pos[t] % W, p * 8);  // in elements = bytes; a multiple of 8
  *reinterpret_cast<u32x2*>(ck + off) = kv8_pack(ld16(k + (size_t)t * ld + p * 8));
  *reinterpret_cast<u32x2*>(cv + off) = kv8_pack(ld16(v + (size_t)t * ld + p * 8));
}

// e4m3 rings -> bf16 rings, element by element (the layout does not enter): one 16-byte load and two 16-byte stores per lane
// and ring; blockIdx.y picks K or V.  n16: 16-element pieces per ring.
__global__ __launch_bounds__(256) void kv_dequant_kernel(bf16_t* dk, bf16_t* dv, const uint8_t* sk, const uint8_t* sv, size_t n16) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n16) return;
  const uint8_t* src = (blockIdx.y ? sv : sk) + idx * 16;
  bf16_t* dst = (blockIdx.y ? dv : dk) + idx * 16;
  const u32x4 w = ld16_nt(src);
  u32x4 o[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t p01, p23;
    gemv_core::cvt4_e4m3(w[i], p01, p23);
    o[i >> 1][2 * (i & 1)] = p01;
    o[i >> 1][2 * (i & 1) + 1] = p23;
  }
  st16(dst, o[0]);
  st16(dst + 8, o[1]);
}

// Decode step metadata from the device-resident kv_seqlens (no host round trip), then
// kv_seqlens += 1 (cache.py:193-195 update_seqlens for seqlens = [1]*B).
__global__ void decode_prep_kernel(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before, int32_t* tok_seq,
                                   int32_t* tok_pos, int B, uint32_t* engine_ctrl) {
  const int b = threadIdx.x;
  if (b == 0 && engine_ctrl) {
    engine_ctrl[CTRL_EPOCH] += 1;
    engine_ctrl[CTRL_ABORT] = 0;
    engine_ctrl[CTRL_STEPS] += 1;  // decode steps started on this workspace (index + 1 into the greedy history ring)
  }
  if (b < B) {
    const int p = (int)kv_seqlens[b];
    kv_before[b] = p;
    tok_pos[b] = p;
    tok_seq[b] = b;
    q_start[b] = b;
    kv_seqlens[b] = p + 1;
  }
  if (b == 0) q_start[B] = B;
}

// Decode step on the rank that owns the embedding: decode_prep + embedding gather in ONE launch (block t = sequence t;
// T == B at decode).  Saves a launch per token; the metadata words are consumed only by later launches.
__global__ __launch_bounds__(256) void decode_prep_embedding_kernel(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before,
                                                                    int32_t* tok_seq, int32_t* tok_pos, int B, bf16_t* out,
                                                                    const bf16_t* table, const int64_t* ids, int D, int vocab,
                                                                    uint32_t* engine_ctrl) {
  const int t = blockIdx.x;
  if (threadIdx.x == 0) {
    if (t == 0 && engine_ctrl) {
      engine_ctrl[CTRL_EPOCH] += 1;
      engine_ctrl[CTRL_ABORT] = 0;
      engine_ctrl[CTRL_STEPS] += 1;
    }
    const int p = (int)kv_seqlens[t];
    kv_before[t] = p;
    tok_pos[t] = p;
    tok_seq[t] = t;
    q_start[t] = t;
    kv_seqlens[t] = p + 1;
    if (t == 0) q_start[B] = B;
  }
  const long id = checked_id(ids[t], vocab, t, engine_ctrl ? engine_ctrl + CTRL_BAD_ID : nullptr);
  const bf16_t* src = table + (size_t)id * D;
  bf16_t* dst = out + (size_t)t * D;
  for (int p = threadIdx.x; p < (D >> 3); p += 256) st16(dst + p * 8, ld16(src + p * 8));
}

// Greedy sampling behind the LM head on the launch path (the persistent engine does the same in its own epilogue,
// decode_engine.hip): block b reduces logits row b to (max, FIRST index of the max, sum exp(x - max)) - generate.py:124
// `torch.argmax` and :134-136 `log_softmax(...)[token]`, which at the argmax is -log(sum).  Logits of -inf (a masked vocabulary
// tail) add nothing to the sum, as in log_softmax; a row of nothing but -inf has no defined result.
__global__ __launch_bounds__(1024) void greedy_rows_kernel(const float* logits, int ld, int B, int V, int64_t* tok, float* lp,
                                                           int64_t* hist_tok, float* hist_lp, int hist_len,
                                                           const uint32_t* ctrl) {
  __shared__ float s_m[16], s_s[16];
  __shared__ int s_i[16];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* row = logits + (size_t)b * ld;
  float M = -INFINITY, S = 0.f;
  // What the sum subtracts: M once the thread has met a finite logit, 0 until then - x - M would be -inf + inf = NaN for a thread that
  // starts on -inf logits (a masked vocabulary tail), exp(-inf - 0) is the 0 such a logit adds.  Set where M is: no work per trip.
  float Ms = 0.f;
  int I = 0x7fffffff;
  int i0 = threadIdx.x;
  if ((V & 3) == 0 && (reinterpret_cast<size_t>(row) & 15) == 0) {
    // 16 logits per trip from four independent 16-byte loads (round 6: the scalar loop below was one dependent 4-byte load per
    // trip - V / 1024 L2 round trips: 46.6 us per step at Mistral-Nemo's 131072 logits, 14.4 at 32768).  Ascending indices per
    // thread, `>` on the trip's maximum and the first position holding it: the FIRST maximum, as before.
    const int V4 = V >> 2;
    for (int q = threadIdx.x; q < V4; q += 4096) {
      float x[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int qk = q + k * 1024;
        const float4 v = *reinterpret_cast<const float4*>(row + (size_t)min(qk, V4 - 1) * 4);  // (unconditional load, masked value)
        const bool in = qk < V4;
        x[4 * k + 0] = in ? v.x : -INFINITY;
        x[4 * k + 1] = in ? v.y : -INFINITY;
        x[4 * k + 2] = in ? v.z : -INFINITY;
        x[4 * k + 3] = in ? v.w : -INFINITY;
      }
      float cm = x[0];
#pragma unroll
      for (int e = 1; e < 16; ++e) cm = fmaxf(cm, x[e]);
      if (cm > M) {
        S *= __expf(M - cm);  // (M = -inf at the start: exp(-inf) = 0 and S = 0)
        M = Ms = cm;
        int first = 15;
#pragma unroll
        for (int e = 14; e >= 0; --e) first = (x[e] == cm) ? e : first;
        I = (q + (first >> 2) * 1024) * 4 + (first & 3);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) S += __expf(x[e] - Ms);
    }
    i0 = V;  // nothing left for the scalar loop
  }
  for (int i = i0; i < V; i += 1024) {  // ascending indices per thread: `>` keeps the first maximum
    const float x = row[i];
    if (x > M) {
      S = S * __expf(M - x) + 1.f;
      M = Ms = x;
      I = i;
    } else {
      S += __expf(x - Ms);
    }
  }
  auto merge = [&](float m2, int i2, float s2) {
    const bool take = m2 > M || (m2 == M && i2 < I);
    const float Mn = take ? m2 : M;
    S = S * (M == Mn ? 1.f : __expf(M - Mn)) + s2 * (m2 == Mn ? 1.f : __expf(m2 - Mn));
    M = Mn;
    I = take ? i2 : I;
  };
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) merge(__shfl_xor(M, o, 64), __shfl_xor(I, o, 64), __shfl_xor(S, o, 64));
  if (lane == 0) {
    s_m[w] = M;
    s_i[w] = I;
    s_s[w] = S;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 16; ++j) merge(s_m[j], s_i[j], s_s[j]);
    const float l = -__logf(S);
    tok[b] = I;
    lp[b] = l;
    if (hist_tok && hist_len > 0) {
      const uint32_t step = (ctrl[CTRL_STEPS] - 1u) % (uint32_t)hist_len;
      hist_tok[(size_t)step * B + b] = I;
      hist_lp[(size_t)step * B + b] = l;
    }
  }
}

// Verify step: thread b counts the leading drafts of sequence b that the model's own argmaxes confirm.
__global__ void verify_accept_kernel(const int64_t* ids, const int64_t* tok, const int32_t* q_start, int B, int32_t* n_accept) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int q0 = q_start[b], m = q_start[b + 1] - q0;
  int a = 0;
  while (a + 1 < m && ids[q0 + a + 1] == tok[q0 + a]) ++a;
  n_accept[b] = a;
}

// Verify step: the accepted rows of the per-layer stash enter the rings - block (row t, layer l), one 16-byte piece of K and of V
// per thread and trip; rejected rows are not read.  Block (0, 0) advances kv_seqlens when the launch carries it.
__global__ __launch_bounds__(256) void verify_commit_kernel(VerifyCommitArgs a) {
  const int t = blockIdx.x, l = blockIdx.y;
  const int b = a.tok_seq[t];
  const int i = t - a.q_start[b];
  if (t == 0 && l == 0 && a.kv_seqlens)
    for (int s = threadIdx.x; s < a.B; s += 256) a.kv_seqlens[s] += a.n_accept[s] + 1;
  if (i > a.n_accept[b]) return;
  const int W = a.W[l];
  const bf16_t* src = a.stash + ((size_t)l * a.T + t) * 2 * a.kv_dim;
  for (int p = threadIdx.x; p < (a.kv_dim >> 3); p += 256) {
    const size_t off = kv_offset(a.kv_layout, W, a.kv_dim, a.Dh, (size_t)b, (a.kv_before[b] + i) % W, p * 8);
    st16(a.k[l] + off, ld16(src + p * 8));
    st16(a.v[l] + off, ld16(src + a.kv_dim + p * 8));
  }
}

__global__ void engine_ctrl_reset_kernel(uint32_t* ctrl) {
  ctrl[CTRL_EPOCH] += 16;  // tags of the failed step (epoch + 1) can never match again
  ctrl[CTRL_STATUS] = 0;
  ctrl[CTRL_ABORT] = 0;
  ctrl[CTRL_ARRIVE] = 0;
}

// out = bf16(a + b) (transformer_layers.py:168 for the MoE prefill path)
__global__ __launch_bounds__(256) void add_rows_kernel(bf16_t* out, const bf16_t* a, const bf16_t* b, size_t npieces) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npieces) return;
  const u32x4 x = ld16(a + p * 8), y = ld16(b + p * 8);
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack_bf2(bf_lo(x[i]) + bf_lo(y[i]), bf_hi(x[i]) + bf_hi(y[i]));
  st16(out + p * 8, o);
}

// moe.py:25-27.  One block per token, one wave per expert: logit_e = bf16(x . Wg[e]) ; top-k ; softmax over the k ;
// bf16.  (A single wave per token serialises E dot products behind one another: 30 us per decode layer.)
constexpr int MOE_MAX_E = 16;
__global__ __launch_bounds__(1024) void moe_router_kernel(int32_t* sel_idx, float* sel_w, const bf16_t* x, int ldx, int D,
                                                          const bf16_t* gate, int E, int top_k, const bf16_t* norm_w,
                                                          float eps) {
  __shared__ float s_logit[MOE_MAX_E];
  const int t = blockIdx.x, lane = threadIdx.x & 63, e = threadIdx.x >> 6;  // wave e <-> expert e
  const bf16_t* xr = x + (size_t)t * ldx;
  const bf16_t* gr = gate + (size_t)e * D;
  const int np = D >> 3;
  float ss = 0.f;
  if (norm_w) {  // every wave needs the same 1/rms: recomputing it (8 KB from L2) is cheaper than a block reduction
    for (int p = lane; p < np; p += 64) {
      const u32x4 v = ld16(xr + p * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = bf_lo(v[i]), b = bf_hi(v[i]);
        ss = fmaf(a, a, ss);
        ss = fmaf(b, b, ss);
      }
    }
    ss = wave_sum(ss);
  }
  const float inv = norm_w ? 1.0f / sqrtf(ss / (float)D + eps) : 1.f;
  float acc = 0.f;
  for (int p = lane; p < np; p += 64) {
    const u32x4 v = ld16(xr + p * 8);
    const u32x4 g = ld16(gr + p * 8);
    const u32x4 wv = norm_w ? ld16(norm_w + p * 8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x0 = bf_lo(v[i]), x1 = bf_hi(v[i]);
      if (norm_w) {
        x0 = bf_round(bf_round(x0 * inv) * bf_lo(wv[i]));
        x1 = bf_round(bf_round(x1 * inv) * bf_hi(wv[i]));
      }
      acc = fmaf(bf_lo(g[i]), x0, acc);
      acc = fmaf(bf_hi(g[i]), x1, acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s_logit[e] = bf_round(acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    float tw[4];
    int ti[4];
    unsigned taken = 0;
    for (int k = 0; k < top_k; ++k) {
      int best = -1;
      float bv = -INFINITY;
      for (int j = 0; j < E; ++j)
        if (!((taken >> j) & 1u) && (best < 0 || s_logit[j] > bv)) {  // ties: lowest expert id
          best = j;
          bv = s_logit[j];
        }
      taken |= 1u << best;
      ti[k] = best;
      tw[k] = bv;
    }
    float den = 0.f, ex[4];
    for (int k = 0; k < top_k; ++k) {
      ex[k] = expf(tw[k] - tw[0]);
      den += ex[k];
    }
    for (int k = 0; k < top_k; ++k) {
      sel_idx[t * top_k + k] = ti[k];
      sel_w[t * top_k + k] = bf_round(ex[k] / den);
    }
  }
}

// Sort the T*top_k (token, slot) pairs by expert for the token-grouped prefill GEMMs (moe.py:29-31 `torch.where` per
// expert, which costs the reference one host sync per expert per layer).  Single block: LDS histogram, exclusive
// scan, LDS-cursor scatter.  Row order inside an expert is arbitrary (it only decides which MFMA tile a row lands
// in, never its value); the bf16 accumulation ORDER of moe.py is reproduced later by moe_combine_kernel.
__global__ __launch_bounds__(1024) void moe_lists_kernel(const int32_t* sel_idx, int T, int E, int top_k, int32_t* tok_of,
                                                         int32_t* row_of, int32_t* tile_tab, int32_t* n_tiles, int tile_rows) {
  __shared__ int cnt[MOE_MAX_E];
  __shared__ int off[MOE_MAX_E + 1];
  __shared__ int cur[MOE_MAX_E];
  const int tid = threadIdx.x, n = T * top_k;
  if (tid < MOE_MAX_E) cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) atomicAdd(&cnt[sel_idx[i]], 1);
  __syncthreads();
  if (tid == 0) {
    int o = 0, nt = 0;
    for (int e = 0; e < E; ++e) {
      off[e] = o;
      cur[e] = o;
      for (int r = 0; r < cnt[e]; r += tile_rows) {  // m-tiles of this expert
        tile_tab[nt * 4 + 0] = e;
        tile_tab[nt * 4 + 1] = o + r;
        tile_tab[nt * 4 + 2] = min(tile_rows, cnt[e] - r);
        tile_tab[nt * 4 + 3] = 0;
        ++nt;
      }
      o += cnt[e];
    }
    off[E] = o;
    *n_tiles = nt;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int r = atomicAdd(&cur[sel_idx[i]], 1);
    tok_of[r] = i / top_k;
    row_of[i] = r;
  }
}

// moe.py:28-32 accumulation + transformer_layers.py:168: per token, experts in ascending id, bf16 running sum from 0.
__global__ __launch_bounds__(256) void moe_combine_kernel(bf16_t* out, const bf16_t* h, const bf16_t* y, const int32_t* sel_idx,
                                                          const float* sel_w, const int32_t* row_of, int D, int top_k) {
  const int t = blockIdx.x;
  int eid[4], row[4];
  float w[4];
  for (int k = 0; k < top_k; ++k) {
    eid[k] = sel_idx[t * top_k + k];
    row[k] = row_of[t * top_k + k];
    w[k] = sel_w[t * top_k + k];
  }
  for (int i = 0; i < top_k; ++i)
    for (int j = i + 1; j < top_k; ++j)
      if (eid[j] < eid[i]) {
        int te = eid[i]; eid[i] = eid[j]; eid[j] = te;
        te = row[i]; row[i] = row[j]; row[j] = te;
        const float tw = w[i]; w[i] = w[j]; w[j] = tw;
      }
  for (int p = threadIdx.x; p < (D >> 3); p += 256) {
    float r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = 0.f;
    for (int k = 0; k < top_k; ++k) {
      const u32x4 v = ld16(y + (size_t)row[k] * D + p * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        r[2 * i] = bf_round(r[2 * i] + bf_round(w[k] * bf_lo(v[i])));
        r[2 * i + 1] = bf_round(r[2 * i + 1] + bf_round(w[k] * bf_hi(v[i])));
      }
    }
    const u32x4 hv = ld16(h + (size_t)t * D + p * 8);
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_bf2(bf_lo(hv[i]) + r[2 * i], bf_hi(hv[i]) + r[2 * i + 1]);
    st16(out + (size_t)t * D + p * 8, o);
  }
}

// nn.GELU() (exact erf form) on a bf16 tensor: evaluated in fp32, rounded once (vision_encoder.py:112-116).
__global__ __launch_bounds__(256) void gelu_kernel(bf16_t* x, int ldx, int N) {
  bf16_t* row = x + (size_t)blockIdx.x * ldx;
  for (int i = threadIdx.x; i < N; i += 256) {
    const float v = bf_to_f(row[i]);
    row[i] = f_to_bf(0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)));
  }
}

// logprob[m] = x_t - (M + log sum_j s_j exp(m_j - M)) from the per-tile partials of GEMM_LOGPROB: one wave per row.
__global__ __launch_bounds__(64) void logprob_finalize_kernel(float* out, const float2* partial, const float* tgt, int n_tiles) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const float2* p = partial + (size_t)m * n_tiles;
  float M = -INFINITY;
  for (int j = lane; j < n_tiles; j += 64) M = fmaxf(M, p[j].x);
  M = wave_max(M);
  float S = 0.f;
  for (int j = lane; j < n_tiles; j += 64) S += p[j].y * __expf(p[j].x - M);
  S = wave_sum(S);
  if (lane == 0) out[m] = tgt[m] - (M + logf(S));
}

// Same result from a full fp32 logits row (small-M path): one block per row.
__global__ __launch_bounds__(256) void logprob_rows_kernel(float* out, const float* logits, int ld, const int32_t* target, int V) {
  __shared__ float red[8];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* x = logits + (size_t)m * ld;
  float M = -INFINITY;
  for (int j = tid; j < V; j += 256) M = fmaxf(M, x[j]);
  M = wave_max(M);
  if (lane == 0) red[wid] = M;
  __syncthreads();
  M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float S = 0.f;
  for (int j = tid; j < V; j += 256) S += __expf(x[j] - M);
  S = wave_sum(S);
  if (lane == 0) red[4 + wid] = S;
  __syncthreads();
  if (tid == 0) {
    const int t = target[m];
    out[m] = (t >= 0 && t < V ? x[t] : 0.f) - (M + logf(red[4] + red[5] + red[6] + red[7]));
  }
}

}  // namespace

hipError_t launch_logprob_finalize(float* out, const float2* partial, const float* tgt, int M, int n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(logprob_finalize_kernel, dim3(M), dim3(64), 0, s, out, partial, tgt, n_tiles);
  return hipGetLastError();
}
hipError_t launch_logprob_rows(float* out, const float* logits, int ld, const int32_t* target, int M, int V, hipStream_t s) {
  hipLaunchKernelGGL(logprob_rows_kernel, dim3(M), dim3(256), 0, s, out, logits, ld, target, V);
  return hipGetLastError();
}

hipError_t launch_gelu(void* x, int ldx, int T, int N, hipStream_t s) {
  hipLaunchKernelGGL(gelu_kernel, dim3(T), dim3(256), 0, s, (bf16_t*)x, ldx, N);
  return hipGetLastError();
}

hipError_t launch_embedding(void* out, const void* table, const int64_t* ids, int T, int D, int vocab, uint32_t* bad_id,
                            hipStream_t s) {
  hipLaunchKernelGGL(embedding_kernel, dim3(T), dim3(256), 0, s, (bf16_t*)out, (const bf16_t*)table, ids, D, vocab, bad_id);
  return hipGetLastError();
}
hipError_t launch_rmsnorm(void* out, const void* x, const void* w, int T, int D, float eps, hipStream_t s) {
  const dim3 grid((T + 3) / 4), block(256);
  bf16_t* o = (bf16_t*)out;
  const bf16_t *xx = (const bf16_t*)x, *ww = (const bf16_t*)w;
  if (D % 8 || D > 16384) return hipErrorInvalidValue;
  if (D <= 4096) hipLaunchKernelGGL((rmsnorm_kernel<8>), grid, block, 0, s, o, xx, ww, T, D, eps);
  else if (D <= 6144) hipLaunchKernelGGL((rmsnorm_kernel<12>), grid, block, 0, s, o, xx, ww, T, D, eps);
  else if (D <= 8192) hipLaunchKernelGGL((rmsnorm_kernel<16>), grid, block, 0, s, o, xx, ww, T, D, eps);
  else hipLaunchKernelGGL((rmsnorm_kernel<32>), grid, block, 0, s, o, xx, ww, T, D, eps);
  return hipGetLastError();
}
template <bool NORM>
static hipError_t launch_act_quant(uint8_t* q, float* sx, const bf16_t* x, int ldx, const bf16_t* w, int M, int K, float eps, hipStream_t s) {
  const dim3 grid((M + 3) / 4), block(256);
  if (K <= 4096) hipLaunchKernelGGL((act_quant_e4m3_kernel<8, NORM>), grid, block, 0, s, q, sx, x, ldx, w, M, K, eps);
  else if (K <= 6144) hipLaunchKernelGGL((act_quant_e4m3_kernel<12, NORM>), grid, block, 0, s, q, sx, x, ldx, w, M, K, eps);
  else if (K <= 8192) hipLaunchKernelGGL((act_quant_e4m3_kernel<16, NORM>), grid, block, 0, s, q, sx, x, ldx, w, M, K, eps);
  else hipLaunchKernelGGL((act_quant_e4m3_kernel<32, NORM>), grid, block, 0, s, q, sx, x, ldx, w, M, K, eps);
  return hipGetLastError();
}
hipError_t launch_act_quant_e4m3(void* xq, float* sx, const void* x, int ldx, int M, int K, const void* norm_w, float eps,
                                 hipStream_t s) {
  if (M <= 0 || K <= 0 || K % 8 || K > 16384 || ldx < K || ldx % 8) return hipErrorInvalidValue;
  return norm_w ? launch_act_quant<true>((uint8_t*)xq, sx, (const bf16_t*)x, ldx, (const bf16_t*)norm_w, M, K, eps, s)
                : launch_act_quant<false>((uint8_t*)xq, sx, (const bf16_t*)x, ldx, nullptr, M, K, eps, s);
}
hipError_t launch_rope(void* qkv, int ld, int T, int H, int Hkv, int Dh, const float* rope_cs, const int32_t* tok_pos,
                       hipStream_t s) {
  const int cols = (H + Hkv) * Dh;
  const long n = (long)T * (cols >> 3);
  hipLaunchKernelGGL(rope_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (bf16_t*)qkv, ld, T, cols, Dh,
                     rope_cs, tok_pos);
  return hipGetLastError();
}
hipError_t launch_kv_write(void* ck, void* cv, int W, const void* k, const void* v, int ld, int T, int kv_dim,
                           const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_start, int kv_layout, int Dh, hipStream_t s) {
  if (Dh <= 0 || Dh % 8 || kv_dim % Dh) return hipErrorInvalidValue;
  const long n = (long)T * (kv_dim >> 3);
  if (kv_layout & MI_KV_E4M3) {
    hipLaunchKernelGGL(kv_write_e4m3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint8_t*)ck, (uint8_t*)cv, W,
                       (const bf16_t*)k, (const bf16_t*)v, ld, T, kv_dim, tok_seq, tok_pos, q_start, kv_layout & 1, Dh);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(kv_write_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (bf16_t*)ck, (bf16_t*)cv, W,
                     (const bf16_t*)k, (const bf16_t*)v, ld, T, kv_dim, tok_seq, tok_pos, q_start, kv_layout, Dh);
  return hipGetLastError();
}
hipError_t launch_kv_dequant(void* dk, void* dv, const void* sk, const void* sv, size_t n_elems, hipStream_t s) {
  if (n_elems % 16) return hipErrorInvalidValue;
  const size_t n16 = n_elems / 16;
  if (n16 == 0) return hipSuccess;
  hipLaunchKernelGGL(kv_dequant_kernel, dim3((unsigned)((n16 + 255) / 256), 2), dim3(256), 0, s, (bf16_t*)dk, (bf16_t*)dv,
                     (const uint8_t*)sk, (const uint8_t*)sv, n16);
  return hipGetLastError();
}
hipError_t launch_decode_prep(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before, int32_t* tok_seq,
                              int32_t* tok_pos, int B, uint32_t* engine_ctrl, hipStream_t s) {
  if (B > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(decode_prep_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, s, kv_seqlens, q_start, kv_before,
                     tok_seq, tok_pos, B, engine_ctrl);
  return hipGetLastError();
}
hipError_t launch_decode_prep_embedding(int64_t* kv_seqlens, int32_t* q_start, int32_t* kv_before, int32_t* tok_seq,
                                        int32_t* tok_pos, int B, void* out, const void* table, const int64_t* ids, int D,
                                        int vocab, uint32_t* engine_ctrl, hipStream_t s) {
  hipLaunchKernelGGL(decode_prep_embedding_kernel, dim3(B), dim3(256), 0, s, kv_seqlens, q_start, kv_before, tok_seq, tok_pos, B,
                     (bf16_t*)out, (const bf16_t*)table, ids, D, vocab, engine_ctrl);
  return hipGetLastError();
}
hipError_t launch_greedy_rows(const float* logits, int ld, int B, int V, int64_t* tok, float* lp, int64_t* hist_tok,
                              float* hist_lp, int hist_len, const uint32_t* ctrl, hipStream_t s) {
  hipLaunchKernelGGL(greedy_rows_kernel, dim3(B), dim3(1024), 0, s, logits, ld, B, V, tok, lp, hist_tok, hist_lp, hist_len, ctrl);
  return hipGetLastError();
}
hipError_t launch_verify_accept(const int64_t* ids, const int64_t* tok, const int32_t* q_start, int B, int32_t* n_accept, hipStream_t s) {
  hipLaunchKernelGGL(verify_accept_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ids, tok, q_start, B, n_accept);
  return hipGetLastError();
}
hipError_t launch_verify_commit(const VerifyCommitArgs& a, hipStream_t s) {
  if (a.n_layers <= 0 || a.n_layers > VERIFY_COMMIT_LAYERS || a.T <= 0 || a.Dh <= 0 || a.Dh % 8 || a.kv_dim % a.Dh || (a.kv_layout & ~1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(verify_commit_kernel, dim3(a.T, a.n_layers), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_engine_ctrl_reset(uint32_t* ctrl, hipStream_t s) {
  hipLaunchKernelGGL(engine_ctrl_reset_kernel, dim3(1), dim3(1), 0, s, ctrl);
  return hipGetLastError();
}
hipError_t launch_add_rows(void* out, const void* a, const void* b, size_t n, hipStream_t s) {
  const size_t np = n >> 3;
  hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, (bf16_t*)out,
                     (const bf16_t*)a, (const bf16_t*)b, np);
  return hipGetLastError();
}
hipError_t launch_moe_router(int32_t* sel_idx, float* sel_w, const void* x, int ldx, int T, int D, const void* gate,
                             int E, int top_k, const void* norm_w, float eps, hipStream_t s) {
  if (E > MOE_MAX_E || top_k > 4 || top_k > E) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_router_kernel, dim3(T), dim3(64 * E), 0, s, sel_idx, sel_w, (const bf16_t*)x, ldx, D,
                     (const bf16_t*)gate, E, top_k, (const bf16_t*)norm_w, eps);
  return hipGetLastError();
}
hipError_t launch_moe_lists(const int32_t* sel_idx, int T, int E, int top_k, int32_t* tok_of, int32_t* row_of,
                            int32_t* tile_tab, int32_t* n_tiles, int tile_rows, hipStream_t s) {
  hipLaunchKernelGGL(moe_lists_kernel, dim3(1), dim3(1024), 0, s, sel_idx, T, E, top_k, tok_of, row_of, tile_tab, n_tiles,
                     tile_rows);
  return hipGetLastError();
}
hipError_t launch_moe_combine(void* out, const void* h, const void* y, const int32_t* sel_idx, const float* sel_w,
                              const int32_t* row_of, int T, int D, int top_k, hipStream_t s) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3(T), dim3(256), 0, s, (bf16_t*)out, (const bf16_t*)h, (const bf16_t*)y,
                     sel_idx, sel_w, row_of, D, top_k);
  return hipGetLastError();
}
