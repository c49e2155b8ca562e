// Weight-streaming GEMV launches for M <= 8 tokens (decode) on bf16 weight rows, and the MoE down-projection kernel.
//
// Replaces, per decode token and layer, the reference's separate launches for RMSNorm
// (transformer_layers.py:115-120), the q/k/v/o and w1/w2/w3 nn.Linear GEMVs (:66,:93,:105-106), RoPE
// (rope.py:13-23), the ring write (cache.py:83-92), the residual adds (:166,:168) and silu*mul.
//
// The kernels are gemv_core::gemv_body on the W16 format; the design notes are in gemv_core.cuh.
#include <cstdlib>

#include "common.cuh"
#include "gemv_core.cuh"

// A second compile with -DGEMV_F16=1 (build_native.py: gemv_f16.o) is the same weight-streaming kernel for fp16 storage: the
// element E (common.cuh) is ElemF16 - v_dot2_f32_f16 for v_dot2c_f32_bf16, half conversions and rounding points - and the entry
// points are launch_gemv_f16 / gemv_max_tokens_f16 (api.hip: decode steps of fp16 models in mi_forward_generic).  gemv_core.cuh
// takes the element from the weight format W16<E>; nothing in it depends on this file's switch.
#ifndef GEMV_F16
#define GEMV_F16 0
#endif
using E = Elem16<GEMV_F16>;

namespace {

using namespace gemv_core;
typedef W16<E> W;  // the weight format: 16-bit rows of the activations' element

// ROWS: rows per unit, always 2; DMA: the activation rows go to LDS by LDS-DMA (instantiated for 2..8 tokens, picked when they do
// not fit the registers)
template <int TT, int MODE, int ROWS, bool DMA>
__global__ __launch_bounds__(256, (TT == 1 ? 4 : (TT <= 3 ? 3 : 2))) void gemv_kernel(GemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<W, TT, MODE, ROWS, DMA>(a, nullptr, smem, blockIdx.x, gridDim.x, blockIdx.y);
}

// Blocks of 5 .. 7 waves for the plain modes at one token (gemv_core.cuh NWV): row counts that 4-wave blocks cannot split evenly
// over the CUs.
template <int MODE, int NWV>
__global__ __launch_bounds__(NWV * 64, 4) void gemv_kernel_nw(GemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<W, 1, MODE, 2, false, NWV>(a, nullptr, smem, blockIdx.x, gridDim.x, blockIdx.y);
}

// MoE down-projection + combine for one token per blockIdx.y (moe.py:28-32 at decode):
// out[t] = bf16(h[t] + R),  R = sum over the token's experts in ascending id of bf16(w_e * bf16(W2_e . g_e)),
// accumulated in bf16 starting from zero.
template <int TOPK>
__global__ __launch_bounds__(256) void moe_w2_kernel(GemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [TOPK][K]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.y;
  const int nwaves = gridDim.x * 4;
  const int units = (a.N + 1) >> 1;
  constexpr int U = BATCH / 2;
  const int nch = (a.K + (1 << W::SHIFT) - 1) >> W::SHIFT;
  const int nb = (nch + U - 1) / U;

  int eid[TOPK];
  float ew[TOPK];
  const bf16_t* w2[TOPK];
#pragma unroll
  for (int k = 0; k < TOPK; ++k) {
    eid[k] = a.sel_idx[t * TOPK + k];
    ew[k] = a.sel_w[t * TOPK + k];
  }
  // visit experts in ascending id (moe.py:29 loop order)
#pragma unroll
  for (int i = 0; i < TOPK; ++i)
#pragma unroll
    for (int j = i + 1; j < TOPK; ++j)
      if (eid[j] < eid[i]) {
        const int te = eid[i]; eid[i] = eid[j]; eid[j] = te;
        const float tw = ew[i]; ew[i] = ew[j]; ew[j] = tw;
      }
  int slot_of[TOPK];  // which hidden row belongs to sorted position k
#pragma unroll
  for (int k = 0; k < TOPK; ++k) {
    slot_of[k] = 0;
#pragma unroll
    for (int s = 0; s < TOPK; ++s)
      if (a.sel_idx[t * TOPK + s] == eid[k]) slot_of[k] = s;
    w2[k] = reinterpret_cast<const bf16_t*>(a.expert_tab[eid[k] * 3 + 1]);
  }

  // flattened load cursor over (unit, expert, batch)
  int u = blockIdx.x * 4 + wid;
  int ul = u, kl = 0, jl = 0;
  u32x4 bufA[BATCH], bufB[BATCH];
  auto issue = [&](u32x4 (&buf)[BATCH]) {  // branch-free around the loads (see gemv_core.cuh)
    const bool live = ul < units;
    const bf16_t* base = w2[0];
#pragma unroll
    for (int k = 1; k < TOPK; ++k) base = (kl == k) ? w2[k] : base;
    const int ue = live ? ul : 0;
    Rows<W, 2> r;
    r.p[0] = live ? base + (size_t)(2 * ue) * a.K : a.x;
    r.p[1] = live ? ((2 * ue + 1 < a.N) ? base + (size_t)(2 * ue + 1) * a.K : r.p[0]) : a.x;
    load_batch<W, 2>(r, live ? jl * U : 0, live ? a.K : 8, live ? lane : 0, buf);
    if (live && ++jl == nb) {
      jl = 0;
      if (++kl == TOPK) {
        kl = 0;
        ul += nwaves;
      }
    }
  };
  // stage the TOPK hidden rows of this token (rows of a.x are [T*TOPK, K], slot-major per token) by LDS-DMA, one row per sorted
  // position: all pieces in flight at once (it was a load -> store loop of K / 2048 L2 round trips), issued BEFORE the two weight
  // batches so that vmcnt(16) = "the rows have landed" leaves the weights in flight
#pragma unroll
  for (int k = 0; k < TOPK; ++k)
    dma_rows_to_lds(a.x + ((size_t)t * TOPK + slot_of[k]) * a.ldx, 0, 1, 1, a.K >> 3, reinterpret_cast<char*>(xs + (size_t)k * a.K));
  issue(bufA);
  issue(bufB);
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __syncthreads();

  float acc[2][1] = {{0.f}, {0.f}};
  int jc = 0, kc = 0;
  float r0 = 0.f, r1 = 0.f;
  auto step = [&](u32x4 (&buf)[BATCH]) {
    fma_batch<W, 1, 2>(buf, jc * U, xs + (size_t)kc * a.K, a.K, lane, acc);
    issue(buf);
    if (++jc == nb) {
      jc = 0;
      const float y0 = wave_sum(acc[0][0]), y1 = wave_sum(acc[1][0]);
      acc[0][0] = acc[1][0] = 0.f;
      float w = ew[0];
#pragma unroll
      for (int k = 1; k < TOPK; ++k) w = (kc == k) ? ew[k] : w;
      r0 = E::round(r0 + E::round(w * E::round(y0)));
      r1 = E::round(r1 + E::round(w * E::round(y1)));
      if (++kc == TOPK) {
        kc = 0;
        if (lane == 0 && u < units) {
          const int n = 2 * u;
          const bf16_t* rs = a.residual + (size_t)t * a.ldo + n;
          bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + (size_t)t * a.ldo + n;
          o[0] = E::from_f(E::to_f(rs[0]) + r0);
          if (n + 1 < a.N) o[1] = E::from_f(E::to_f(rs[1]) + r1);
        }
        r0 = r1 = 0.f;
        u += nwaves;
      }
    }
  };
  if (u < units) {  // both steps per trip: see gemv_core.cuh (a step past the last unit stores nothing)
    do {
      step(bufA);
      step(bufB);
    } while (u < units);
  }
}

template <int MODE>
hipError_t launch_mode(const GemvArgs& a, int TT, dim3 grid, size_t lds, hipStream_t s) {
  return for_tt(TT, [&](auto tt) {
    constexpr int T = decltype(tt)::value;
    if constexpr (T > 1) {
      if (stage_by_dma(MODE, T, a.K)) return launch_lds<gemv_kernel<T, MODE, 2, true>>(a, grid, lds, s);
    }
    return launch_lds<gemv_kernel<T, MODE, 2, false>>(a, grid, lds, s);
  });
}

template <int MODE>
hipError_t launch_nw(const GemvArgs& a, int nw, dim3 grid, size_t lds, hipStream_t s) {
  switch (nw) {
    case 5: hipLaunchKernelGGL((gemv_kernel_nw<MODE, 5>), grid, dim3(320), lds, s, a); break;
    case 6: hipLaunchKernelGGL((gemv_kernel_nw<MODE, 6>), grid, dim3(384), lds, s, a); break;
    case 7: hipLaunchKernelGGL((gemv_kernel_nw<MODE, 7>), grid, dim3(448), lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

#if GEMV_F16
int gemv_max_tokens_f16(int K) {
#else
int gemv_max_tokens(int K) {
#endif
  int t = (int)(GEMV_LDS_BUDGET / ((size_t)K * 2));
  if (t == 5 || t == 7) --t;  // (5 and 7 rows run on the 6- and 8-row instantiations, which stage 6 / 8 rows in LDS)
  return t < 1 ? 1 : (t > GEMV_MAX_T ? GEMV_MAX_T : t);
}

// One launch; a.T must be <= gemv_max_tokens(K).
#if GEMV_F16
hipError_t launch_gemv_f16(const GemvArgs& a, hipStream_t s) {
#else
hipError_t launch_gemv(const GemvArgs& a, hipStream_t s) {
#endif
  const bool pair_mode = !(a.mode == GEMV_SWIGLU || a.mode == GEMV_MOE_W13);
  const int units = pair_mode ? (a.N + 1) / 2 : a.N;
  const int cus = device_cus();
  int blocks = even_blocks(units, cus);
  int nw = 4;  // waves per block
  if (!blocks) {
    // No even split over 4-wave blocks (Mistral-Nemo's Wo / W2: 5120 rows = 2560 pairs = 256 CUs x 10).  spread_blocks
    // gives 320 blocks - 64 CUs with two blocks, 192 with one - and the doubly loaded CUs set the kernel's time at their own
    // ingest rate (W2: 30 us for 147 MB).  One token, plain modes: blocks of 5 .. 7 waves that DO split evenly, all resident.
    static int nw_ok = -1;  // MI_GEMV_NW=0: 4-wave blocks only (A/B testing)
    if (nw_ok < 0) {
      const char* e = getenv("MI_GEMV_NW");
      nw_ok = e ? atoi(e) : 1;
    }
    const bool plain1 = nw_ok && a.T == 1 && (a.mode == GEMV_STORE || a.mode == GEMV_RESIDUAL) && a.norm_w == nullptr &&
                        (size_t)a.K * 2 <= 48 * 1024;
    for (int w = 5; plain1 && w <= 7 && nw == 4; ++w)
      for (int k = 1; k <= 16 && nw == 4; ++k) {
        const int b = units / (w * k);
        if (b >= cus && b % cus == 0 && b * w * k == units && b * w <= 16 * cus) {
          nw = w;
          blocks = b;
        }
      }
  }
  if (!blocks) blocks = spread_blocks(units, max_blocks(cus));
  if (a.mode == GEMV_MOE_W2) {
    const size_t lds = (size_t)a.top_k * a.K * 2;
    dim3 grid(blocks, a.T);
    switch (a.top_k) {
      case 1: hipLaunchKernelGGL((moe_w2_kernel<1>), grid, dim3(256), lds, s, a); break;
      case 2: hipLaunchKernelGGL((moe_w2_kernel<2>), grid, dim3(256), lds, s, a); break;
      case 4: hipLaunchKernelGGL((moe_w2_kernel<4>), grid, dim3(256), lds, s, a); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  const int TT = a.mode == GEMV_MOE_W13 ? 1 : round_tt(a.T);
  const size_t lds = lds_bytes(TT, a.K, a.norm_w != nullptr);
  dim3 grid(blocks_for_lds(blocks, units, cus, lds), a.mode == GEMV_MOE_W13 ? a.T * a.top_k : 1);
  if (nw != 4) return a.mode == GEMV_STORE ? launch_nw<GEMV_STORE>(a, nw, grid, lds, s) : launch_nw<GEMV_RESIDUAL>(a, nw, grid, lds, s);
  switch (a.mode) {
    case GEMV_STORE: return launch_mode<GEMV_STORE>(a, TT, grid, lds, s);
    case GEMV_RESIDUAL: return launch_mode<GEMV_RESIDUAL>(a, TT, grid, lds, s);
    case GEMV_LOGITS: return launch_mode<GEMV_LOGITS>(a, TT, grid, lds, s);
    case GEMV_SWIGLU: return launch_mode<GEMV_SWIGLU>(a, TT, grid, lds, s);
    case GEMV_QKV_ROPE: return launch_mode<GEMV_QKV_ROPE>(a, TT, grid, lds, s);
    case GEMV_MOE_W13: return launch_mode<GEMV_MOE_W13>(a, 1, grid, lds, s);
    default: return hipErrorInvalidValue;
  }
}
