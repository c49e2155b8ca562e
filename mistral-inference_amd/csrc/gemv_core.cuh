// Core of the weight-streaming GEMV for M <= 8 tokens (decode): HBM-bound, one pass over the weights.  One unit loop
// (gemv_body) for 16-bit weight rows (gemv.hip: W16<ElemBf16>, and W16<ElemF16> in its -DGEMV_F16=1 compile) and for e4m3 rows
// with fp32 row scales (gemv_w8.hip) and for MXFP4 rows, e2m1 codes with one e8m0 scale byte per block of 32 (gemv_w4.hip); the MoE
// down-projection (gemv.hip) uses the same batch loads and FMAs.  Host side: the launch plan.
//
// Structure (cdna_hip_programming.md "GEMV / M<=16 decode weights"): weights go straight HBM -> VGPR with 16-byte
// non-temporal loads in batches of 8 per lane; a wave always has two batches (16 KiB) in flight, across the prologue and
// across unit boundaries (the load cursor runs over the flattened (unit, batch) sequence, two batches ahead of the FMAs).
// The (optionally RMS-normalised) activation rows live in LDS; their loads are issued before the first weight batch so the
// prologue finishes under the HBM latency of the weights.  A wave owns "units" (one or two pairs of weight rows) strided over
// the whole grid, so at any instant the chip streams one contiguous weight region.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "common.cuh"
#include "kernels.h"

namespace gemv_core {

constexpr int BATCH = 8;  // 16-byte loads per lane per batch (NR rows x BATCH/NR chunks); two batches in flight

// ---- weight formats.  PIECE: weights per 16-byte piece; a chunk is one wave instruction = 64 pieces = 1 << SHIFT weights.
// VLOADS: vector loads per batch (x_finish counts two batches of them behind the LDS-DMAs); BLOCK: block-scaled (below).
// act: the element (common.cuh) of the activation rows, norm weights, residual and outputs: the prologue and the epilogue convert and round through it.
template <class A>
struct W16 {  // 16-bit rows of the activations' own element, which is also the dot product's
  typedef A act;
  typedef uint16_t elem;
  typedef float scale_t;
  static constexpr int PIECE = 8, SHIFT = 9;
  static constexpr bool SCALED = false, BLOCK = false;
  static constexpr int VLOADS = 8;
};
// OCP e4m3 bytes; the real-valued weight is scale[r] * e4m3(W[r, k]).  Per output row acc = sum_k e4m3(W[r, k]) * x[k] in fp32
// and y = acc * scale[r] in fp32 enters the epilogue where acc enters it for 16-bit rows.  K % 16 == 0.
struct WE4m3 {
  typedef ElemBf16 act;
  typedef uint8_t elem;
  typedef float scale_t;
  static constexpr int PIECE = 16, SHIFT = 10;
  static constexpr bool SCALED = true, BLOCK = false;
  static constexpr int VLOADS = 8;
};
// OCP MXFP4: e2m1 codes, two per byte with the low nibble at the even k, and one e8m0 scale byte per block of 32 along K (scale
// rows [rows, K / 32] beside the weight rows); the weight entering the dot product is 2^(b - 127) * e2m1(code), exact in bf16.  A
// 16-byte piece is 32 weights = exactly one scale block: every piece load of a batch has one scale-byte load beside it (block-
// scaled, as opposed to SCALED per row: nothing is applied in the epilogue).  K % 32 == 0.  Element offsets k of this format are
// byte offsets k / 2 (wofs).
struct WMxfp4 {
  typedef ElemBf16 act;
  typedef uint8_t elem;
  typedef uint8_t scale_t;
  static constexpr int PIECE = 32, SHIFT = 11;
  static constexpr bool SCALED = false, BLOCK = true;
  static constexpr int VLOADS = 16;
};
// offset of weight k of a row, in F::elem
template <class F>
__device__ __forceinline__ size_t wofs(size_t k) {
  if constexpr (F::BLOCK) return k >> 1;
  else return k;
}

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// four e4m3 bytes (k .. k + 3) -> fp32 (k, k + 1) and (k + 2, k + 3): v_cvt_pk_f32_fp8 on either half of the dword
__device__ __forceinline__ void cvt4_e4m3_f32(uint32_t w, f32x2_t& lo, f32x2_t& hi) {
  lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
}
// ... -> the bf16 pairs (k, k + 1) and (k + 2, k + 3).  Every finite e4m3 value is exact in bf16, so the high halves of the two
// fp32 results, packed by v_perm_b32, are an exact bf16 pair for v_dot2c_f32_bf16.  Per dword of weights: 2 converts + 2 perms
// (shared by all tokens) + 2 dot2 per token, against 4 unpacks + 4 FMAs per token for the plain-fp32 form.
__device__ __forceinline__ void cvt4_e4m3(uint32_t w, uint32_t& p01, uint32_t& p23) {
  f32x2_t lo, hi;
  cvt4_e4m3_f32(w, lo, hi);
  // bytes 2, 3 of the first operand's partner (S1) below bytes 2, 3 of S0: (S1 >> 16) | (S0 & 0xffff0000)
  p01 = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
  p23 = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
}

template <class F, int NR, bool BLK = F::BLOCK>
struct Rows {
  const typename F::elem* p[NR];
};
template <class F, int NR>
struct Rows<F, NR, true> {
  const typename F::elem* p[NR];
  const uint8_t* s[NR];  // the rows of block scales, [K / 32] bytes each
};
// the scale bytes of a batch beside its pieces (block-scaled formats; nothing otherwise)
template <class F>
struct ScaleBuf {};
template <>
struct ScaleBuf<WMxfp4> {
  uint32_t b[BATCH];
};

// byte SEL of w = two e2m1 codes (k, k + 1), the low nibble first -> the bf16 pair scaled by 2^(b - 127), sc = the float b << 23:
// one v_cvt_scalef32_pk_bf16_fp4 (op_sel picks the byte).  Exact: 8 magnitudes x a power of two.
template <int SEL>
__device__ __forceinline__ uint32_t cvt2_e2m1(uint32_t w, float sc) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
}

// One batch = chunks [c0, c0 + BATCH/NR) of each of the unit's NR rows: always exactly BATCH unconditional loads.
// Chunk offsets past K are clamped to the row's last 16 bytes (fma_batch skips them) and a missing last row aliases
// its partner (the epilogue drops it).  Never a `cond ? load : 0`: that makes hipcc branch around each load and wait
// vmcnt(0) after it (cdna_hip_programming.md, ".s-level traps" (c)).
template <class F, int NR>
__device__ __forceinline__ void load_batch(const Rows<F, NR>& r, int c0, int K, int lane, u32x4 (&buf)[BATCH]) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = min(((c0 + u) * 64 + lane) * F::PIECE, K - F::PIECE);
#pragma unroll
    for (int i = 0; i < NR; ++i) buf[i * U + u] = ld16_nt(r.p[i] + wofs<F>(e));
  }
}
// ... and the scale bytes of the same (clamped) pieces: BATCH more unconditional loads, 64 consecutive bytes per wave instruction
template <class F, int NR>
__device__ __forceinline__ void load_scales(const Rows<F, NR>& r, int c0, int K, int lane, ScaleBuf<F>& sb) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = min(((c0 + u) * 64 + lane) * F::PIECE, K - F::PIECE);
#pragma unroll
    for (int i = 0; i < NR; ++i) sb.b[i * U + u] = r.s[i][e >> 5];
  }
}

// xs: the activation rows in LDS, [TT][K] 16-bit
template <class F, int TT, int NR>
__device__ __forceinline__ void fma_batch(const u32x4 (&buf)[BATCH], int c0, const bf16_t* xs, int K, int lane, float (&acc)[NR][TT]) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = ((c0 + u) * 64 + lane) * F::PIECE;
    if (e < K) {
      if constexpr (F::PIECE == 8) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + e);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < NR; ++i) acc[i][t] = F::act::dot2(buf[i * U + u][c], xv[c], acc[i][t]);
        }
      } else {
        static_assert(std::is_same<typename F::act, ElemBf16>::value, "cvt4_e4m3 makes bf16 pairs");
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // halves of the piece: 8 weights = 2 dwords against one 16-byte piece of x
          uint32_t p[NR][4];
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            cvt4_e4m3(buf[i * U + u][2 * h], p[i][0], p[i][1]);
            cvt4_e4m3(buf[i * U + u][2 * h + 1], p[i][2], p[i][3]);
          }
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + e + 8 * h);
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[i][t] = ElemBf16::dot2(p[i][c], xv[c], acc[i][t]);
          }
        }
      }
    }
  }
}

// MXFP4: a piece is 32 weights against 64 bytes of x.  Per quarter of the piece (one dword = 8 weights): 4 converts per row, shared
// by all tokens, then 4 dot2 per row and token.
template <int TT, int NR>
__device__ __forceinline__ void fma_batch_w4(const u32x4 (&buf)[BATCH], const ScaleBuf<WMxfp4>& sb, int c0, const bf16_t* xs, int K,
                                             int lane, float (&acc)[NR][TT]) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = ((c0 + u) * 64 + lane) * 32;
    if (e < K) {
      float sc[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) sc[i] = __uint_as_float(sb.b[i * U + u] << 23);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        uint32_t p[NR][4];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const uint32_t w = buf[i * U + u][h];
          p[i][0] = cvt2_e2m1<0>(w, sc[i]);
          p[i][1] = cvt2_e2m1<1>(w, sc[i]);
          p[i][2] = cvt2_e2m1<2>(w, sc[i]);
          p[i][3] = cvt2_e2m1<3>(w, sc[i]);
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + e + 8 * h);
#pragma unroll
          for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][t] = ElemBf16::dot2(p[i][c], xv[c], acc[i][t]);
        }
      }
    }
  }
}

// ---- activation staging.  x[T, K] (rows t >= T are zero) goes to LDS, optionally RMS-normalised:
// bf16( bf16(x * rsqrt(mean(x^2) + eps)) * w )   (transformer_layers.py:115-120).
// Split in two so that the x (and norm weight) loads are the FIRST loads the wave issues - they are L2 hits and
// return long before the HBM weight batches issued right after them, so the whole prologue runs under the
// weight latency instead of in front of it.
// Activation pieces (16 B) a thread holds in registers while the weight batches are issued.  Modes that fuse the
// RMSNorm (K = model dim <= 8192 for one token) hold NX = 4 x pieces + NW = 4 norm-weight pieces; the plain modes
// (Wo, W2: K up to 16384) hold NX = 8 x pieces and no norm weights.  Anything larger takes the in-loop path.
template <int NX, int NW>
struct XRegs {
  u32x4 x[NX];
  u32x4 w[NW > 0 ? NW : 1];
};

// Activations that do not fit the register set (batches of >= 3 tokens; W2 rows of >= 2 tokens) go to LDS by LDS-DMA
// (global_load_lds_dwordx4: a wave-instruction moves 64 consecutive 16-byte pieces, no registers, all of them in flight at
// once), the norm weights behind them; x_finish waits ONCE and runs the RMSNorm passes on LDS.  Before round 6 this case was
// a load -> wait -> store loop per 256 pieces: up to 21 dependent L2 round trips in front of the first FMA of every GEMV of a
// batch-3 decode step (q|k|v 19.3 us against 13.0 at batch 1).  Piece q of `rows` rows goes to dst + q * 16; rows >= T are zeros.
__device__ __forceinline__ void dma_rows_to_lds(const bf16_t* src, int ld, int rows, int T, int npieces, char* dst) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int total = rows * npieces;
  for (int q0 = wid * 64; q0 < total; q0 += 256) {
    const int q = q0 + lane;
    const int t = q / npieces, pc = q - t * npieces;
    if (q < total) {
      if (t < T) {
        // from inline asm (M0 = the wave's LDS base, saved and restored): hipcc does not track it, so it neither drains the
        // weight loads at the prologue's barriers (as it does behind the builtin) nor counts it - the waits behind these DMAs are
        // the caller's (x_finish: vmcnt(16) with exactly the two weight batches issued after them)
        unsigned keep;
        const bf16_t* sp = src + (size_t)t * ld + pc * 8;
        const uint32_t lds_addr = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)(dst + (size_t)q0 * 16);
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off\n\t"
                     "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(sp), "s"(lds_addr) : "memory");
      } else {
        st16(dst + (size_t)q * 16, u32x4{0u, 0u, 0u, 0u});
      }
    }
  }
}

// Issues exactly NX + NW loads (clamped / dummy where there is nothing to load); when the rows do not fit them, the DMAs above.
// xs: the LDS image [TT][K]; ws: K norm weights behind it (used by the DMA path of the norm modes only).
// DMA is a property of the INSTANTIATION (launch_gemv picks it when the rows cannot fit the registers): with an LDS-DMA anywhere in
// a function hipcc waits vmcnt(0) at every barrier and gives up the counted waits of the register path.
template <int TT, int NX, int NW, bool DMA, int NT = 256>
__device__ __forceinline__ bool x_issue(XRegs<NX, NW>& xr, const bf16_t* x, int ldx, int T, int K, const bf16_t* norm_w, bf16_t* xs,
                                        bf16_t* ws) {
  const int npieces = K >> 3;
  const int total = TT * npieces;
  if constexpr (DMA) {
    dma_rows_to_lds(x, ldx, TT, T, npieces, reinterpret_cast<char*>(xs));
    if (norm_w) dma_rows_to_lds(norm_w, 0, 1, 1, npieces, reinterpret_cast<char*>(ws));
    return false;
  }
  const bool fits = total <= NX * NT && (norm_w == nullptr || total <= NW * NT);
  const bf16_t* wsrc = norm_w ? norm_w : x;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int q = min((int)threadIdx.x + i * NT, total - 1);
    const int t = q / npieces, p = q - t * npieces;
    xr.x[i] = ld16(x + (size_t)min(t, T - 1) * ldx + p * 8);
    if (i < NW) xr.w[i] = ld16(wsrc + p * 8);
  }
  return fits;
}

// A: the rows' element (F::act); VMW: the vector loads issued behind the DMAs = two weight batches of the format (F::VLOADS each).
template <class A, int TT, int NX, int NW, bool DMA, int NT = 256, int VMW = 2 * BATCH>
__device__ __forceinline__ void x_finish(bool in_regs, XRegs<NX, NW>& xr, bf16_t* xs, float* red, const bf16_t* ws,
                                         const bf16_t* x, int ldx, int T, int K, const bf16_t* norm_w, float eps) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int npieces = K >> 3;
  float ss[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) ss[t] = 0.f;
  if (in_regs) {
    const int total = TT * npieces;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int q = tid + i * NT;
      if (q < total) {
        const int t = q / npieces;
        if (t >= T) xr.x[i] = u32x4{0u, 0u, 0u, 0u};
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float a = A::lo(xr.x[i][c]), b = A::hi(xr.x[i][c]);
          s = fmaf(a, a, s);
          s = fmaf(b, b, s);
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) ss[tt] += (tt == t) ? s : 0.f;
        if (!norm_w) st16(xs + (size_t)q * 8, xr.x[i]);  // [t][K] row-major == q * 8
      }
    }
  } else if constexpr (DMA) {
    // the rows (and norm weights) were sent to LDS by x_issue's DMAs.  vmcnt retires in order and EXACTLY the two weight batches
    // (2 x BATCH unconditional loads: gemv_body, moe_w2_kernel; a block-scaled format has as many scale-byte loads again) were issued
    // behind them: vmcnt(VMW) = the DMAs have landed, the weights stay in flight under the passes below, which read LDS only.
    static_assert(BATCH == 8 && (VMW == 16 || VMW == 32), "the wait below counts the two weight batches");
    if constexpr (VMW == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    __syncthreads();
    if (norm_w != nullptr) {
      for (int p = tid; p < npieces; p += 256) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + p * 8);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float a = A::lo(v[c]), b = A::hi(v[c]);
            ss[t] = fmaf(a, a, ss[t]);
            ss[t] = fmaf(b, b, ss[t]);
          }
        }
      }
    }
  } else {
    for (int p = tid; p < npieces; p += NT) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const u32x4 ld = ld16(x + (size_t)min(t, T - 1) * ldx + p * 8);
        const u32x4 z = {0u, 0u, 0u, 0u};
        const u32x4 v = (t < T) ? ld : z;
        st16(xs + (size_t)t * K + p * 8, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float a = A::lo(v[c]), b = A::hi(v[c]);
          ss[t] = fmaf(a, a, ss[t]);
          ss[t] = fmaf(b, b, ss[t]);
        }
      }
    }
  }
  if (norm_w == nullptr) {
    if (!DMA) __syncthreads();  // (the DMA path has had its barrier)
    return;
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float s = wave_sum(ss[t]);
    if (lane == 0) red[wid * TT + t] = s;
  }
  __syncthreads();
  float inv[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float s = red[t] + red[TT + t] + red[2 * TT + t] + red[3 * TT + t];
    inv[t] = 1.0f / sqrtf(s / (float)K + eps);
  }
  if (in_regs) {
    if constexpr (NW > 0) {
      const int total = TT * npieces;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int q = tid + i * 256;
        if (q < total) {
          const int t = q / npieces;
          float iv = 0.f;
#pragma unroll
          for (int tt = 0; tt < TT; ++tt) iv = (tt == t) ? inv[tt] : iv;
          u32x4 o;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            o[c] = A::pack2(A::round(A::lo(xr.x[i][c]) * iv) * A::lo(xr.w[i < NW ? i : 0][c]),
                            A::round(A::hi(xr.x[i][c]) * iv) * A::hi(xr.w[i < NW ? i : 0][c]));
          st16(xs + (size_t)q * 8, o);
        }
      }
    }
  } else {
    for (int p = tid; p < npieces; p += 256) {
      const u32x4 wv = DMA ? *reinterpret_cast<const u32x4*>(ws + p * 8) : ld16(norm_w + p * 8);
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + p * 8);
        u32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          o[c] = A::pack2(A::round(A::lo(v[c]) * inv[t]) * A::lo(wv[c]), A::round(A::hi(v[c]) * inv[t]) * A::hi(wv[c]));
        st16(xs + (size_t)t * K + p * 8, o);
      }
    }
  }
  __syncthreads();
}

// Row r of up to three matrices side by side (segment ends n0, n1) picks the expression of its own matrix.  A macro, so that
// only the picked expression is evaluated: the e4m3 kernels then keep scalar branches around the three forms; a function
// taking the three pointers by value makes s_cselect chains there and a slower Wo kernel (profiles/EXPERIMENTS.md).
#define GEMV_SEG_PICK(r, n0, n1, e0, e1, e2) ((r) < (n0) ? (e0) : ((r) < (n1) ? (e1) : (e2)))

template <class Wt>
__device__ __forceinline__ const Wt* seg_row(const GemvArgs& a, int r) {
  return GEMV_SEG_PICK(r, a.n0, a.n1, reinterpret_cast<const Wt*>(a.w0) + (size_t)r * a.K,
                       reinterpret_cast<const Wt*>(a.w1) + (size_t)(r - a.n0) * a.K, reinterpret_cast<const Wt*>(a.w2) + (size_t)(r - a.n1) * a.K);
}
// ... of MXFP4 rows (K / 2 bytes each), and the row's block scales (K / 32 bytes)
__device__ __forceinline__ const uint8_t* seg_row_w4(const GemvArgs& a, int r) {
  const size_t rb = (size_t)(a.K >> 1);
  return GEMV_SEG_PICK(r, a.n0, a.n1, reinterpret_cast<const uint8_t*>(a.w0) + (size_t)r * rb,
                       reinterpret_cast<const uint8_t*>(a.w1) + (size_t)(r - a.n0) * rb, reinterpret_cast<const uint8_t*>(a.w2) + (size_t)(r - a.n1) * rb);
}
__device__ __forceinline__ const uint8_t* seg_scale_row_w4(const GemvArgs& a, const uint8_t* const* scale, int r) {
  const size_t rb = (size_t)(a.K >> 5);
  return GEMV_SEG_PICK(r, a.n0, a.n1, scale[0] + (size_t)r * rb, scale[1] + (size_t)(r - a.n0) * rb, scale[2] + (size_t)(r - a.n1) * rb);
}

// the modes that fuse the RMSNorm into the prologue
constexpr bool norm_mode(int mode) { return mode == GEMV_QKV_ROPE || mode == GEMV_SWIGLU || mode == GEMV_LOGITS || mode == GEMV_MOE_W13; }

// F: weight format; TT: token rows staged in LDS; NR = rows per unit: one row pair, or two for e4m3 rows, which are half the
// bytes, so that the fixed cost of a unit (wave reductions, epilogue, loop bookkeeping) weighs twice as much (launch_gemv_w8).
// Row pair q: SWIGLU / MOE_W13 = (W1 row q, W3 row q), else output rows (2 q, 2 q + 1).
// scale: the fp32 row scales of the (up to) three matrices, read by the SCALED formats only; the block-scale rows of the BLOCK ones.
// Order: activation loads first (L2 hits), then two weight batches, and the prologue finishes under them.
// NWV = waves per block: 4; 5 .. 8 for the plain modes (no fused RMSNorm: its passes are written for 256 threads) when the row
// count has no even split over 4-wave blocks - Mistral-Nemo's 5120 rows are 2560 pairs = 256 CUs x 10 (launch_gemv).
template <class F, int TT, int MODE, int NR, bool DMA, int NWV = 4>
__device__ __forceinline__ void gemv_body(const GemvArgs& a, const typename F::scale_t* const* scale, char* smem, int block_id, int n_blocks,
                                          int problem) {
  typedef typename F::elem Wt;  // weight storage
  typedef typename F::act A;    // activations and outputs
  constexpr int RP = NR / 2, U = BATCH / NR;
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + (size_t)TT * a.K * 2);
  bf16_t* ws = reinterpret_cast<bf16_t*>(smem + (size_t)TT * a.K * 2 + 16 * TT);  // (lds_bytes reserves it for TT > 1)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: unit loops become scalar
  const int nwaves = n_blocks * NWV;
  constexpr bool kPairOut = !(MODE == GEMV_SWIGLU || MODE == GEMV_MOE_W13);
  const int npairs = kPairOut ? (a.N + 1) >> 1 : a.N;
  const int units = (npairs + RP - 1) / RP;
  const int nch = (a.K + (1 << F::SHIFT) - 1) >> F::SHIFT;
  const int nb = (nch + U - 1) / U;  // batches per unit

  // MoE: blockIdx.y is the problem (token, slot); pick this problem's expert and input row
  const bf16_t* x = a.x;
  const Wt *e1 = nullptr, *e3 = nullptr;
  char* outp = reinterpret_cast<char*>(a.out);
  if (MODE == GEMV_MOE_W13) {
    const int prob = problem;
    const int e = a.sel_idx[prob];
    e1 = reinterpret_cast<const Wt*>(a.expert_tab[e * 3 + 0]);
    e3 = reinterpret_cast<const Wt*>(a.expert_tab[e * 3 + 2]);
    x = a.x + (size_t)(prob / a.top_k) * a.ldx;
    outp += (size_t)prob * a.ldo * 2;
  }
  const int T = (MODE == GEMV_MOE_W13) ? 1 : a.T;

  // 1. activation (and norm weight) loads first, 2. two weight batches, 3. finish the prologue under them
  constexpr bool kNormMode = norm_mode(MODE);
  constexpr int NX = kNormMode ? 4 : 8, NW = kNormMode ? 4 : 0;
  static_assert(NWV == 4 || (!kNormMode && !DMA), "other block sizes: plain modes on the register staging path");
  XRegs<NX, NW> xr;
  bool in_regs = false;
  // q|k|v epilogue operands that depend on nothing: the token's position (RoPE row, ring slot) and its sequence (ring row) are the
  // FIRST loads of the wave.  Loaded behind the weight batches (rounds 1-6), the position - which the first RoPE prefetch needs
  // for its address - made hipcc wait vmcnt(0) in front of the first FMA: both weight batches drained, then two dependent L2
  // round trips (position, RoPE entry), and a third per unit for the sequence in the epilogue.  As the oldest loads they are
  // waited for with a counted vmcnt that leaves the weights in flight.
  const int tl = lane < T ? lane : 0;
  int ep_pos = 0, ep_seq = 0;
  if (MODE == GEMV_QKV_ROPE) {
    ep_pos = a.tok_pos[tl];
    ep_seq = a.tok_seq ? a.tok_seq[tl] : a.seq0 + tl;
  }
  in_regs = x_issue<TT, NX, NW, DMA, NWV * 64>(xr, x, a.ldx, T, a.K, a.norm_w, xs, ws);

  auto unit_rows = [&](int uu) {
    Rows<F, NR> r;
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      // a unit's missing second pair repeats the last one.  Two-row e4m3 units keep the clamp although it changes nothing: without
      // it hipcc lays the Wo kernel out 120 ns slower per call (profiles/EXPERIMENTS.md); the 16-bit rows never had it.
      const int q = (RP == 1 && !F::SCALED) ? uu : min(uu * RP + p, npairs - 1);
      if constexpr (F::BLOCK) {  // (STORE / RESIDUAL / SWIGLU / QKV_ROPE)
        if (MODE == GEMV_SWIGLU) {
          r.p[2 * p] = reinterpret_cast<const Wt*>(a.w0) + (size_t)q * (a.K >> 1);
          r.p[2 * p + 1] = reinterpret_cast<const Wt*>(a.w1) + (size_t)q * (a.K >> 1);
          r.s[2 * p] = scale[0] + (size_t)q * (a.K >> 5);
          r.s[2 * p + 1] = scale[1] + (size_t)q * (a.K >> 5);
        } else {
          const int r1 = (2 * q + 1 < a.N) ? 2 * q + 1 : 2 * q;  // odd N: alias, result dropped in the epilogue
          r.p[2 * p] = seg_row_w4(a, 2 * q);
          r.p[2 * p + 1] = seg_row_w4(a, r1);
          r.s[2 * p] = seg_scale_row_w4(a, scale, 2 * q);
          r.s[2 * p + 1] = seg_scale_row_w4(a, scale, r1);
        }
      } else if (MODE == GEMV_SWIGLU) {
        r.p[2 * p] = reinterpret_cast<const Wt*>(a.w0) + (size_t)q * a.K;
        r.p[2 * p + 1] = reinterpret_cast<const Wt*>(a.w1) + (size_t)q * a.K;
      } else if (MODE == GEMV_MOE_W13) {
        r.p[2 * p] = e1 + (size_t)q * a.K;
        r.p[2 * p + 1] = e3 + (size_t)q * a.K;
      } else {
        r.p[2 * p] = seg_row<Wt>(a, 2 * q);
        r.p[2 * p + 1] = (2 * q + 1 < a.N) ? seg_row<Wt>(a, 2 * q + 1) : r.p[2 * p];  // odd N: alias, result dropped in the epilogue
      }
    }
    return r;
  };

  // load cursor over the flattened (unit, batch) sequence of this wave: always two batches ahead of the math
  int u = block_id * NWV + wid;
  int ul = u, jl = 0;
  Rows<F, NR> rpl = unit_rows(min(ul, units - 1));
  u32x4 bufA[BATCH], bufB[BATCH];
  ScaleBuf<F> sbA, sbB;  // (block-scaled formats: the scale bytes of the two batches)
  // Past the wave's last unit `issue` loads BATCH times one L2-resident line instead of branching around the loads:
  // the row pointers and chunk offset are SELECTED (real rows, or one dummy line) and the BATCH loads are issued
  // unconditionally, which keeps the loop body one basic block and the compiler's wait for one buffer at
  // "the other buffer's BATCH loads may stay in flight".  The trailing loads are never consumed.
  const Wt* dummy = reinterpret_cast<const Wt*>(x);
  auto issue = [&](u32x4 (&buf)[BATCH], ScaleBuf<F>& sb) {
    const bool live = ul < units;
    Rows<F, NR> r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.p[i] = live ? rpl.p[i] : dummy;
    load_batch<F, NR>(r, live ? jl * U : 0, live ? a.K : F::PIECE, live ? lane : 0, buf);
    if constexpr (F::BLOCK) {
#pragma unroll
      for (int i = 0; i < NR; ++i) r.s[i] = live ? rpl.s[i] : reinterpret_cast<const uint8_t*>(dummy);
      load_scales<F, NR>(r, live ? jl * U : 0, live ? a.K : F::PIECE, live ? lane : 0, sb);
    }
    if (live && ++jl == nb) {
      jl = 0;
      ul += nwaves;
      if (ul < units) rpl = unit_rows(ul);
    }
  };
  issue(bufA, sbA);
  issue(bufB, sbB);
  x_finish<A, TT, NX, NW, DMA, NWV * 64, 2 * F::VLOADS>(in_regs, xr, xs, red, ws, x, a.ldx, T, a.K, a.norm_w, a.eps);

  float acc[NR][TT];
#pragma unroll
  for (int i = 0; i < NR; ++i)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;
  int jc = 0;

  // Epilogue operands are fetched EARLY (token position once; the unit's row scales, RoPE entries / residual pairs when the
  // unit starts) so that the end of a unit is arithmetic + one store instead of a chain of dependent loads.
  float ep_s[NR];
  float2 ep_cs[RP];
  uint32_t ep_res[RP];
#pragma unroll
  for (int p = 0; p < RP; ++p) {
    ep_s[2 * p] = ep_s[2 * p + 1] = 1.f;
    ep_cs[p] = make_float2(1.f, 0.f);
    ep_res[p] = 0;
  }
  auto seg_scale = [&](int r) { return GEMV_SEG_PICK(r, a.n0, a.n1, scale[0][r], scale[1][r - a.n0], scale[2][r - a.n1]); };
  auto prefetch_epilogue = [&](int uu) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const int q = (RP == 1 && !F::SCALED) ? uu : min(uu * RP + p, npairs - 1);  // (as unit_rows)
      const int r0 = 2 * q;
      const bool two = r0 + 1 < a.N;
      if constexpr (F::SCALED) {
        if (!kPairOut) {
          ep_s[2 * p] = scale[0][q];
          ep_s[2 * p + 1] = scale[1][q];
        } else {
          ep_s[2 * p] = seg_scale(r0);
          ep_s[2 * p + 1] = seg_scale(two ? r0 + 1 : r0);
        }
      }
      if (MODE == GEMV_QKV_ROPE && r0 < a.n1) {
        const int i = (r0 % a.head_dim) >> 1;
        ep_cs[p] = *reinterpret_cast<const float2*>(a.rope_cs + ((size_t)ep_pos * (a.head_dim >> 1) + i) * 2);
      }
      if (MODE == GEMV_RESIDUAL) {
        const bf16_t* rs = a.residual + (size_t)tl * a.ldo + r0;
        if (two) ep_res[p] = *reinterpret_cast<const uint32_t*>(rs);
        else ep_res[p] = rs[0];
      }
    }
  };
  if (u < units) prefetch_epilogue(u);

  auto finish_unit = [&]() {
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i][t] = wave_sum(acc[i][t]);
    // ---- epilogue: lane t finishes token t
    float v[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] = 0.f;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (lane == t) {
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = acc[i][t];
      }
    }
    if (lane < T) {
      const int t = lane;
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        const int q = u * RP + p;
        if (RP == 1 || q < npairs) {
          float v0 = v[2 * p], v1 = v[2 * p + 1];
          if constexpr (F::SCALED) {  // y = acc * scale, fp32, before the first rounding
            v0 *= ep_s[2 * p];
            v1 *= ep_s[2 * p + 1];
          }
          if (!kPairOut) {
            bf16_t* o = reinterpret_cast<bf16_t*>(outp) + (size_t)t * a.ldo + q;
            *o = A::from_f(A::swiglu(v0, v1));
          } else {
            const int r0 = 2 * q;
            const bool two = r0 + 1 < a.N;
            if (MODE == GEMV_LOGITS) {
              float* o = reinterpret_cast<float*>(outp) + (size_t)t * a.ldo + r0;
              o[0] = A::round(v0);
              if (two) o[1] = A::round(v1);
            } else {
              float y0 = A::round(v0), y1 = A::round(v1);
              bf16_t* o = reinterpret_cast<bf16_t*>(outp) + (size_t)t * a.ldo + r0;
              if (MODE == GEMV_RESIDUAL) {
                y0 = A::lo(ep_res[p]) + y0;
                if (two) y1 = A::hi(ep_res[p]) + y1;
              }
              if (MODE == GEMV_QKV_ROPE) {
                if (r0 < a.n1) {  // q or k rows: rotate the adjacent pair (rope.py:13-23)
                  float re, im;
                  rope_pair(y0, y1, ep_cs[p].x, ep_cs[p].y, re, im);
                  y0 = re;
                  y1 = im;
                }
                if (a.write_kv && r0 >= a.n0) {  // cache.py:83-92: ring slot pos % W of this sequence's row
                  const int kv_dim = a.n1 - a.n0;
                  const size_t off = kv_offset(a.kv_layout, a.W, kv_dim, a.head_dim, (size_t)ep_seq, ep_pos % a.W,
                                               (r0 < a.n1) ? r0 - a.n0 : r0 - a.n1);
                  bf16_t* ring = ((r0 < a.n1) ? reinterpret_cast<bf16_t*>(a.cache_k) : reinterpret_cast<bf16_t*>(a.cache_v)) + off;
                  *reinterpret_cast<uint32_t*>(ring) = A::pack2(y0, y1);
                }
              }
              if (two) {
                *reinterpret_cast<uint32_t*>(o) = A::pack2(y0, y1);
              } else {
                o[0] = A::from_f(y0);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;
  };

  // One step = consume the oldest batch, refill the same registers with the batch two ahead (ping-pong between
  // bufA and bufB: no register copies, so the compiler's wait for bufA leaves bufB's eight loads in flight).
  auto step = [&](u32x4 (&buf)[BATCH], ScaleBuf<F>& sb) {
    if constexpr (F::BLOCK) fma_batch_w4<TT, NR>(buf, sb, jc * U, xs, a.K, lane, acc);
    else fma_batch<F, TT, NR>(buf, jc * U, xs, a.K, lane, acc);
    issue(buf, sb);
    if (++jc == nb) {
      jc = 0;
      if (u < units) finish_unit();
      u += nwaves;
      if (u < units) prefetch_epilogue(u);
    }
  };
  // ALWAYS both steps per trip (a step past the wave's last unit multiplies dummy lines and stores nothing).  With the second
  // step under `if (u < units)` - rounds 1-6 - hipcc's wait-count pass merged the skip edge into the loop header and guarded
  // the FIRST step's operands with vmcnt(6..0) instead of vmcnt(14..8): every trip drained both batches before its first FMA
  // and the "two batches in flight" of the design was one.
  if (u < units) {
    do {
      step(bufA, sbA);
      step(bufB, sbB);
    } while (u < units);
  }
}

// ---- the launch plan (host), shared by launch_gemv and launch_gemv_scaled (gemv_w8.hip, gemv_w4.hip)

// 5 and 7 rows run on the 6- and 8-row instantiations, which stage 6 / 8 rows in LDS
inline int round_tt(int T) { return T == 5 ? 6 : (T == 7 ? 8 : T); }

// [TT][K] activations, 4 x TT partial sums, and (norm modes at TT > 1: the DMA staging path) K norm weights
inline size_t lds_bytes(int TT, int K, bool norm) { return (size_t)TT * K * 2 + 4 * TT * sizeof(float) + ((TT > 1 && norm) ? (size_t)K * 2 : 0); }

// Rows that fit the prologue's register set (4 x 256 pieces with a fused RMSNorm, 8 x 256 without) are staged through registers;
// 2..8 rows that do not, by LDS-DMA.
inline bool stage_by_dma(int mode, int TT, int K) { return TT > 1 && (size_t)TT * (K >> 3) > (norm_mode(mode) ? 4u : 8u) * 256u; }

// MI_GEMV_MAX_BLOCKS; default 2 blocks per CU (of the first caller's device), measured best on MI355X.  Read once.
inline int max_blocks(int cus) {
  static int v = 0;
  if (v == 0) {
    const char* e = getenv("MI_GEMV_MAX_BLOCKS");
    v = e ? atoi(e) : 2 * cus;
    if (v <= 0) v = 2 * cus;
  }
  return v;
}

// Persistent-style grid: every wave gets the same number k of units (no partially filled last round of blocks; the two-batch
// load pipeline runs across a wave's units).  even_blocks: the smallest k for which the block count is a multiple of the CUs
// (even load per CU), at most 4 per CU, and divides the units exactly - e.g. W1|W3: 14336 units -> 512 blocks x 4 waves x 7
// units; q|k|v: 3072 units -> 768 blocks x 1; 0 when there is none.  spread_blocks: the smallest k that fits `cap` blocks.
inline int even_blocks(int units, int cus) {
  for (int k = 1; k <= 64; ++k) {
    const int b = (units + 4 * k - 1) / (4 * k);
    if (b <= 4 * cus && b % cus == 0 && b * 4 * k == units && (b <= max_blocks(cus) || k == 1)) return b;
  }
  return 0;
}
inline int spread_blocks(int units, int cap) {
  const int k = (units + 4 * cap - 1) / (4 * cap);
  const int b = (units + 4 * k - 1) / (4 * k);
  return b < 1 ? 1 : b;
}
// above 80 KiB of LDS one block fits a CU: one block per CU, every wave the same number of units
inline int blocks_for_lds(int blocks, int units, int cus, size_t lds) { return (lds > 80 * 1024 && blocks > cus) ? spread_blocks(units, cus) : blocks; }

// Launch of a 256-thread kernel with `lds` bytes of dynamic LDS; more than the default limit of 64 KiB is an opt-in per function
// AND per device.
template <auto KERNEL, class Args>
hipError_t launch_lds(const Args& a, dim3 grid, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024) {
    static bool attr_set[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)GEMV_LDS_BUDGET + 1024);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, s, a);
  return hipGetLastError();
}

// f(std::integral_constant<int, TT>) for the instantiated row counts
template <class Fn>
hipError_t for_tt(int TT, Fn&& f) {
  switch (TT) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// ---- the launch of a GEMV on scaled weight rows (host), once for every weight format.  F names what a format's file owns:
//   F::kernel<TT, MODE, RP, DMA>   its __global__ kernel (gemv_body on its WFormat, under its own launch bounds)
//   F::row_pairs(npairs, cus)      its rule for the row pairs per unit at one token
//   F::kRpEnv                      the environment variable that overrides the rule (A/B): 1 / 2; 0 or unset: the rule
template <class F, int MODE, class Args>
hipError_t launch_mode(const Args& a, int TT, int rp, dim3 grid, size_t lds, hipStream_t s) {
  return for_tt(TT, [&](auto tt) {
    constexpr int T = decltype(tt)::value;
    if constexpr (T == 1) {
      return rp == 2 ? launch_lds<F::template kernel<1, MODE, 2, false>>(a, grid, lds, s) : launch_lds<F::template kernel<1, MODE, 1, false>>(a, grid, lds, s);
    } else {
      return stage_by_dma(MODE, T, a.g.K) ? launch_lds<F::template kernel<T, MODE, 1, true>>(a, grid, lds, s)
                                          : launch_lds<F::template kernel<T, MODE, 1, false>>(a, grid, lds, s);
    }
  });
}

// One launch; a.g.T must be <= gemv_max_tokens(K) (the activation rows are bf16 as in gemv.hip: the same LDS budget).
template <class F, class Args>
hipError_t launch_gemv_scaled(const Args& a, hipStream_t s) {
  const GemvArgs& g = a.g;
  static int rp_env = -1;  // (one per format: a static of this instantiation)
  const int cus = device_cus();
  if (rp_env < 0) {
    const char* e = getenv(F::kRpEnv);
    rp_env = e ? atoi(e) : 0;
  }
  const int npairs = g.mode == GEMV_SWIGLU ? g.N : (g.N + 1) / 2;
  int rp = g.T == 1 ? F::row_pairs(npairs, cus) : 1;
  if (g.T == 1 && (rp_env == 1 || rp_env == 2)) rp = rp_env;
  const int units = (npairs + rp - 1) / rp;
  int blocks = even_blocks(units, cus);
  if (!blocks) blocks = spread_blocks(units, max_blocks(cus));
  const int TT = round_tt(g.T);
  const size_t lds = lds_bytes(TT, g.K, g.norm_w != nullptr);
  const dim3 grid(blocks_for_lds(blocks, units, cus, lds));
  switch (g.mode) {
    case GEMV_STORE: return launch_mode<F, GEMV_STORE>(a, TT, rp, grid, lds, s);
    case GEMV_RESIDUAL: return launch_mode<F, GEMV_RESIDUAL>(a, TT, rp, grid, lds, s);
    case GEMV_SWIGLU: return launch_mode<F, GEMV_SWIGLU>(a, TT, rp, grid, lds, s);
    case GEMV_QKV_ROPE: return launch_mode<F, GEMV_QKV_ROPE>(a, TT, rp, grid, lds, s);
    case GEMV_LOGITS: return launch_mode<F, GEMV_LOGITS>(a, TT, rp, grid, lds, s);  // a quantised LM head (opt-in, mi_forward_q)
    default: return hipErrorInvalidValue;
  }
}

}  // namespace gemv_core
