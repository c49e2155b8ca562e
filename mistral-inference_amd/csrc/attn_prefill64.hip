// Non-causal, cache-less attention for 64-wide heads on MFMA: the Pixtral vision tower's attention (vision_encoder.py), where all
// patches of all images attend to each other.  One sequence of T rows, n_heads == n_kv_heads, qkv [T, ld] post-RoPE with q at
// column h*64, k at (H + h)*64, v at (2H + h)*64; out [T, H*64].
//
// Not attn_prefill.hip with DH = 64: there is no causal path, no ring and no per-sequence metadata, and the halved head width moves
// the balance - per score the MFMA work halves while the softmax VALU work (scale, exp2, max, sum, pack) does not.  What the
// narrower head frees is spent on fewer barriers and fewer LDS fragment reads per score:
//   * Block = (query tile, head), NW waves x QS sets of 32 queries.  S^T = K . Q^T, so a lane owns ONE query per set: the row
//     reductions are in-lane plus one permlane32_swap.  With QS = 2 both sets are multiplied against every K and V^T fragment a
//     wave reads: the accumulator budget attn_prefill.hip spends on one set of 128-wide rows (O^T is two f32x16 per set here,
//     not four), and half the LDS fragment traffic per score.
//   * A staged tile is 128 keys (the bytes of the 128 kernel's 64-key tile): one barrier and one staging pass per 128 keys.  The
//     softmax runs on 64-key halves of it, so the live scores stay at 32 registers per set.  Double-buffered: the next tile's
//     global loads are issued before this tile's math and written to the other buffer after it.
//   * K tile: [128 rows][8 slots of 16 B].  A row is 128 B = half of the 64 banks, so the row index decides the upper half of the
//     bank: key k lives in row swap_bits_0_3(k) and its slot s at s ^ (k & 7).  The 32 keys x 2 slots a wave reads for one MFMA
//     then fall on bank group (key & 15) ^ slot - the conflict-free pattern of the 128 kernel's 256-byte rows - and the 16 lanes
//     that stage two consecutive rows cover all 64 banks.
//   * V^T tile: two 64-key halves, each [64 d][144 B] with the 128 kernel's quad order 0, 2, 1, 3 inside every 16 keys: a lane's
//     8 keys of one MFMA are one ds_read_b128, conflict-free at the 144-byte stride.
// Masks: keys at or past T in the last tile score -inf (their loads are clamped to row T - 1); query rows at or past T are
// computed on clamped rows and never stored.  Numerics are attn_prefill.hip's: raw fp32 scores, base-2 softmax with the scale
// folded into the exponent's fma, deferred rescale (threshold 8), P rounded to bf16 for V^T . P^T, fp32 row sum and O, one rounding
// of O / l.
#include <cstdlib>

#include "common.cuh"
#include "kernels.h"

using E = Elem16<false>;  // (an fp16 compile would pick Elem16<true>; fp16 / fp32 towers run on generic.hip)

namespace {

constexpr int DH = 64;
constexpr int KT = 128;                        // keys per staged tile
constexpr int KS_BYTES = KT * DH * 2;          // 16 KiB
constexpr int VT_STRIDE = 144;                 // bytes per d row of a 64-key V^T half
constexpr int VT_HALF = DH * VT_STRIDE;        // 9 KiB
constexpr int BUF_BYTES = KS_BYTES + 2 * VT_HALF;  // 34 KiB; two buffers
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int swap_bits_0_3(int k) { return (k & ~9) | ((k & 1) << 3) | ((k >> 3) & 1); }

template <int NW, int QS>
__global__ __launch_bounds__(NW * 64, 2) void attn_prefill64_kernel(AttnPrefillArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x BUF_BYTES
  constexpr int NT = NW * 64, QW = 32 * QS, QB = NW * QW;      // threads, queries per wave, queries per block

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);    // provably wave-uniform: scalar control flow below
  const int hf = lane >> 5, ql = lane & 31;
  // consecutive block ids go to consecutive XCDs: head fastest, so the blocks of one head meet in one XCD's L2 (H % 8 == 0)
  const int h = blockIdx.x % a.H, qt = blockIdx.x / a.H;
  const int T = a.max_q_len, ld = a.ld;
  const int n_tiles = (T + KT - 1) / KT;
  const int q0 = qt * QB + wid * QW;                           // this wave's first query
  const bool wave_active = q0 < T;

  E::x8 qf[QS][4];
#pragma unroll
  for (int s = 0; s < QS; ++s) {
    const bf16_t* qrow = a.qkv + (size_t)min(q0 + s * 32 + ql, T - 1) * ld + h * DH + hf * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[s][kk] = __builtin_bit_cast(E::x8, ld16(qrow + kk * 16));
  }

  f32x16 acc[QS][2];
  float m_run[QS], l_run[QS];
#pragma unroll
  for (int s = 0; s < QS; ++s) {
    m_run[s] = -1e30f;
    l_run[s] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][dt][r] = 0.f;
  }
  const float sc = a.scale * LOG2E;

  // ---- staging.  K: 16-byte piece p = tid + NT*j -> LDS row p >> 3 (which holds key swap_bits_0_3(row)), slot p & 7.
  // V: a thread takes the same 16-byte d slice of PPT consecutive keys and transposes them in registers, four keys at a time.
  constexpr int PPT = 1024 / NT;  // K pieces and V keys per thread (4 or 8)
  const int k_slot = tid & 7, k_row0 = tid >> 3;
  const int v_kg = tid % (KT / PPT), v_ds = tid / (KT / PPT);
  const bf16_t* kbase = a.qkv + (size_t)(a.H + h) * DH + k_slot * 8;
  const bf16_t* vbase = a.qkv + (size_t)(2 * a.H + h) * DH + v_ds * 8;
  u32x4 rk[PPT], rv[PPT];
  // rows are clamped to T - 1 (in bounds; the duplicates are masked in the softmax); row * ld < 2^31 is checked on the host
  auto gload = [&](int it) {
    const int t_lo = it * KT;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int kk = min(t_lo + swap_bits_0_3(k_row0 + (NT / 8) * j), T - 1);
      rk[j] = ld16(kbase + (uint32_t)(kk * ld));
      const int kv = min(t_lo + v_kg * PPT + j, T - 1);
      rv[j] = ld16(vbase + (uint32_t)(kv * ld));
    }
  };
  auto lstore = [&](char* Ks, char* Vt) {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int row = k_row0 + (NT / 8) * j, key = swap_bits_0_3(row);
      st16(Ks + row * (DH * 2) + ((k_slot ^ (key & 7)) << 4), rk[j]);
    }
#pragma unroll
    for (int g = 0; g < PPT / 4; ++g) {
      const int vk0 = v_kg * PPT + 4 * g, k6 = vk0 & 63;  // first of four keys; they share a 16-key group of one half
      // byte offset inside a V^T row: the quads of every 16 keys in the order 0, 2, 1, 3
      const int v_pos = ((k6 & ~15) | (((k6 >> 2) & 1) << 3) | (((k6 >> 3) & 1) << 2)) * 2;
      char* vt = Vt + (vk0 >> 6) * VT_HALF + v_pos;
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // d = v_ds*8 + 2c (low halves) and 2c + 1 (high halves)
        u32x2 lo, hi;
        lo[0] = (rv[4 * g][c] & 0xffffu) | (rv[4 * g + 1][c] << 16);
        lo[1] = (rv[4 * g + 2][c] & 0xffffu) | (rv[4 * g + 3][c] << 16);
        hi[0] = (rv[4 * g][c] >> 16) | (rv[4 * g + 1][c] & 0xffff0000u);
        hi[1] = (rv[4 * g + 2][c] >> 16) | (rv[4 * g + 3][c] & 0xffff0000u);
        *reinterpret_cast<u32x2*>(vt + (v_ds * 8 + 2 * c) * VT_STRIDE) = lo;
        *reinterpret_cast<u32x2*>(vt + (v_ds * 8 + 2 * c + 1) * VT_STRIDE) = hi;
      }
    }
  };

  gload(0);
  lstore(smem, smem + KS_BYTES);
  __syncthreads();
  for (int it = 0; it < n_tiles; ++it) {
    if (it + 1 < n_tiles) gload(it + 1);
    const char* Kt = smem + (it & 1) * BUF_BYTES;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      const int k_lo = it * KT + hb * 64;       // first key of this 64-key half
      if (!wave_active || k_lo >= T) continue;  // (scalar)
      const char* Ks = Kt + hb * 64 * (DH * 2);
      const char* Vt = Kt + KS_BYTES + hb * VT_HALF;
      // ---- S^T = K . Q^T: the 8 fragments of both 32-key groups are read ahead of the MFMAs and serve every query set
      f32x16 st[QS][2];
#pragma unroll
      for (int s = 0; s < QS; ++s)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int r = 0; r < 16; ++r) st[s][mb][r] = 0.f;
      {
        E::x8 kf[4][2];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) {
            const int key = mb * 32 + ql, slot = k4 * 2 + hf;
            kf[k4][mb] = __builtin_bit_cast(
                E::x8, *reinterpret_cast<const u32x4*>(Ks + swap_bits_0_3(key) * (DH * 2) + ((slot ^ (key & 7)) << 4)));
          }
        __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of the MFMAs
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int s = 0; s < QS; ++s) st[s][mb] = E::mfma32(kf[k4][mb], qf[s][k4], st[s][mb]);
      }
      // ---- the one mask: keys at or past T (last tile only; one scalar branch)
      if (k_lo + 63 >= T) {
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int kp = k_lo + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
              st[s][mb][r] = kp < T ? st[s][mb][r] : -INFINITY;
            }
      }
      // ---- online softmax per query set (this lane: query ql of the set, the keys of its half-wave)
      uint32_t pb[QS][2][2][4];
#pragma unroll
      for (int s = 0; s < QS; ++s) {
        float mx = -INFINITY;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[s][mb][r]);
        {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
          mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        // deferred rescale: the old maximum stays while no lane's grew by more than 2^8 (P <= 256: no loss in bf16 / fp32);
        // wave-uniform, taken before this half's V^T . P^T; l and O see the same factor
        const float m_cand = fmaxf(m_run[s], mx);
        float alpha = 1.0f;
        if (__any((m_cand - m_run[s]) * sc > 8.0f)) {
          alpha = fast_exp2((m_run[s] - m_cand) * sc);
          m_run[s] = m_cand;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[s][dt][r] *= alpha;
        }
        const float nm = -m_run[s] * sc;
        float psum = 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float p0 = fast_exp2(fmaf(st[s][mb][r], sc, nm)), p1 = fast_exp2(fmaf(st[s][mb][r + 1], sc, nm));
            psum += p0 + p1;
            pb[s][mb][r >> 3][(r & 7) >> 1] = E::pack2_fast(p0, p1);
          }
        l_run[s] = l_run[s] * alpha + psum;
      }
      // ---- O^T += V^T . P^T: P^T straight from the S^T registers (keys {0..3, 8..11} + 4*hf of every 16), V^T read in the same order
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            const u32x4 vw = *reinterpret_cast<const u32x4*>(Vt + (dt * 32 + ql) * VT_STRIDE + (mb * 32 + kb * 16 + 8 * hf) * 2);
#pragma unroll
            for (int s = 0; s < QS; ++s) {
              const u32x4 pw = {pb[s][mb][kb][0], pb[s][mb][kb][1], pb[s][mb][kb][2], pb[s][mb][kb][3]};
              acc[s][dt] = E::mfma32(__builtin_bit_cast(E::x8, vw), __builtin_bit_cast(E::x8, pw), acc[s][dt]);
            }
          }
    }
    if (it + 1 < n_tiles) {
      char* nb = smem + ((it + 1) & 1) * BUF_BYTES;
      lstore(nb, nb + KS_BYTES);
    }
    __syncthreads();
  }

  // ---- epilogue: O^T[d][q] / l -> out[q][h*64 + d]
#pragma unroll
  for (int s = 0; s < QS; ++s) {
    const float l_tot = l_run[s] + __shfl_xor(l_run[s], 32, 64);
    const int qi = q0 + s * 32 + ql;
    if (qi < T) {
      const float inv = 1.0f / l_tot;
      bf16_t* orow = reinterpret_cast<bf16_t*>(a.out) + (size_t)qi * (a.H * DH) + h * DH;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          u32x2 o;
          o[0] = E::pack2(acc[s][dt][4 * g] * inv, acc[s][dt][4 * g + 1] * inv);
          o[1] = E::pack2(acc[s][dt][4 * g + 2] * inv, acc[s][dt][4 * g + 3] * inv);
          *reinterpret_cast<u32x2*>(orow + dt * 32 + 8 * g + 4 * hf) = o;
        }
    }
  }
}

template <int NW, int QS>
hipError_t launch_shape(const AttnPrefillArgs& a, hipStream_t s) {
  // 2 x 34 KiB of dynamic LDS: above the 64 KiB default limit.  The opt-in is per function AND per device.
  static bool attr_set[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_prefill64_kernel<NW, QS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BUF_BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  constexpr int QB = NW * 32 * QS;
  hipLaunchKernelGGL((attn_prefill64_kernel<NW, QS>), dim3(((a.max_q_len + QB - 1) / QB) * a.H), dim3(NW * 64), 2 * BUF_BYTES, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_attn_prefill64(const AttnPrefillArgs& a, hipStream_t s) {
  if (a.Dh != DH || a.H != a.Hkv || a.causal || a.cache_k || a.cache_v || a.max_q_len <= 0) return hipErrorInvalidValue;
  // Blocks against CUs (two blocks fit a CU's LDS).  256-query blocks (4 waves x 2 query sets) once every CU gets one: at 16
  // heads x 4096 patches (256 blocks on 256 CUs) they measured 110-112 us against 114-116 as 128-query blocks, at 16384 patches
  // 1353 against 1564.  Else 128-query blocks (4 waves x 1 set) down to half the CUs: one 1024-patch image is 128 of them and
  // measured 19.7 us, against 20.4 as 256 two-wave 64-query blocks - a block on every CU does not pay for the halved K/V reuse
  // there - and 26.8 as 64 blocks of 256.  Below that, 64-query blocks (2 waves) spread what little work there is over twice the
  // CUs.  (scripts/vision_attn_probe.py, profiles/vision_attn_probe.json.log.)
  // MI_ATTN64_QUERIES = 64 | 128 | 256 pins the shape (A/B runs and the tests of the shapes small inputs never choose); it is
  // read on every launch.
  const char* e = getenv("MI_ATTN64_QUERIES");
  int qb = e ? atoi(e) : 0;
  if (qb != 64 && qb != 128 && qb != 256) {
    const long cus = device_cus(), T = a.max_q_len;
    qb = (T + 255) / 256 * a.H >= cus ? 256 : (T + 127) / 128 * a.H * 2 >= cus ? 128 : 64;
  }
  return qb == 256 ? launch_shape<4, 2>(a, s) : qb == 128 ? launch_shape<4, 1>(a, s) : launch_shape<2, 1>(a, s);
}
