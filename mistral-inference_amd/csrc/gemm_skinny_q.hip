// Weight-streaming MFMA GEMM for 9 .. 64 rows on QUANTISED weight rows (weight-only FP8 e4m3 with fp32 row scales, MXFP4 with e8m0
// block scales): out[M,N] = epilogue(A[M,K] . W[N,K]^T) with bf16 activations, the STORE (+ RoPE) / RESIDUAL / SWIGLU epilogues.
// The weight bytes go HBM -> VGPR once and become bf16 MFMA operands in registers; no bf16 image of the weights is written.
//
// The frame is gemm_skinny.hip's: one block of 4 waves per 16 weight rows (or 32, below), the K range split over the waves in
// interleaved batches of CH chunks, a register ring of NB batches with unconditional clamped loads (a chunk past the end of K loads
// the last chunk again and multiplies nothing), no LDS and no barrier inside the loop, the reduce ((w0 + w1) + w2) + w3 through LDS
// by wave 0, G = ceil(M / 16) token groups as a template parameter.  What is new is the operand path:
//
//   chunk      a lane (row l % 16, k-slot l / 16) owns 32 CONTIGUOUS BYTES of its weight row per chunk - two 16-byte non-temporal
//              loads - so that the four slots of a chunk cover one whole 128-byte line of each of the 16 rows, as at bf16.  That is a
//              chunk of 128 weights at e4m3 (32 per lane: four MFMAs of k = 32) and of 256 at MXFP4 (64 per lane = exactly two scale
//              blocks of 32: eight MFMAs).  MFMA j of a chunk takes the lane's weights 8 j .. 8 j + 7; the k label of a slot is free
//              as long as both operands agree on it, so the token fragment of MFMA j is the 16-byte piece j of the lane's 64 / 128
//              contiguous bytes of its token row at the same k offset.
//   scales     MXFP4: the lane's two e8m0 bytes of a chunk (blocks 2 s, 2 s + 1 of the chunk at slot s) are adjacent in the scale
//              row: ONE aligned 16-bit load per chunk and row, beside the weight loads in the ring (gemv_core.cuh loads a byte per
//              piece).  e4m3: the four row scales of a lane's output columns are loaded by wave 0 in front of the loop.
//   convert    e4m3 -> bf16 is exact: v_cvt_pk_f32_fp8 on either half of a dword and a v_perm_b32 that keeps the high halves
//              (gemv_core::cvt4_e4m3): 4 VALU per 4 weights, shared by all token groups.  MXFP4: v_cvt_scalef32_pk_bf16_fp4 with the
//              block's scale as a float, one per byte (gemv_core::cvt2_e2m1), exact as well.  The MFMA stays
//              v_mfma_f32_16x16x32_bf16 on bf16 activations: this is the weight-only route.
//   L2 side    every block reads all of x: 32 K bytes per token group against 16 K (e4m3) or 8.5 K (MXFP4) weight bytes per unit -
//              at four groups 8 x and 15 x the weight bytes.  Both forms are built: U = 1 unit per block, and U = 2 units (32 rows)
//              that share every x fragment, which halves the L2 traffic for 8 (+1) more ring registers per chunk - the x fragments
//              are the ring, not the weights.  The launcher takes U = 2 when ceil(N / 32) blocks still give every CU one
//              (ceil(N / 32) >= CUs: W1|W3 of a 7B model and larger), else U = 1 so that the weight stream is spread over all CUs.
//   registers  the ring shape (CH, NB) is computed per instantiation from the registers a chunk takes (ring_shape below): about 176
//              ring VGPRs where two chunks fit that, never fewer than two chunks in flight.  Every instantiation builds without
//              scratch (checked at build time with -Rpass-analysis=kernel-resource-usage).
//   numerics   e4m3: acc runs on the codes' values, y = acc * scale[row] in fp32 enters the epilogue where acc enters it at bf16 (the
//              rule of the e4m3 GEMV; NOT the bf16(scale * w) rounding of the dequantisation pass).  MXFP4: the block scale is applied
//              in the conversion, the product is the bf16 kernel's on the exact dequantised weights up to summation order.
//   epilogue   the accumulator layout, rounding points, RoPE arithmetic, fast SiLU and edge handling (clamp on load, mask on store,
//              8-byte stores only when aligned) are gemm_skinny.hip's.
#include "common.cuh"
#include "gemv_core.cuh"
#include "kernels.h"

namespace {

struct FmtE4m3 {
  typedef float scale_t;
  static constexpr int BK = 128, XP = 4;  // K chunk; MFMAs (= 16-byte x pieces per lane and token group) per chunk
  static constexpr bool BLOCK = false;
  __host__ __device__ static size_t row_bytes(int K) { return (size_t)K; }
};
struct FmtMxfp4 {
  typedef uint8_t scale_t;
  static constexpr int BK = 256, XP = 8;
  static constexpr bool BLOCK = true;
  __host__ __device__ static size_t row_bytes(int K) { return (size_t)K >> 1; }
};

constexpr int SQ_MAX_G = 4;  // token groups of 16 a launch takes

// one ring entry: CH chunks of NM weight matrices (two 16-byte pieces each, and the two block scale bytes) and G token groups
template <class F, int NM, int G, int CH>
struct QBatch {
  u32x4 w[NM][CH][2];
  uint32_t sc[NM][CH];
  u32x4 x[G][CH][F::XP];
};
// (CH, NB): as many chunks in flight as fit about 176 ring registers, at least two; three batches when there are six chunks
template <class F, int NM, int G>
struct ring_shape {
  static constexpr int per = 8 * NM + (F::BLOCK ? NM : 0) + 4 * F::XP * G;
  static constexpr int tot = 176 / per < 2 ? 2 : 176 / per;
  static constexpr int NB = tot >= 6 ? 3 : 2;
  static constexpr int CH = tot / NB > 4 ? 4 : tot / NB;
};

// MFMA j's eight bf16 weights of a lane's 32 bytes (w[0] | w[1]) of a chunk
template <class F>
__device__ __forceinline__ bf16x8 operand(const u32x4 (&w)[2], uint32_t sc, int j) {
  u32x4 p;
  if constexpr (F::BLOCK) {  // dword j: 8 codes of block j / 4
    const uint32_t d = w[j >> 2][j & 3];
    const float s = __uint_as_float(((j < 4) ? (sc & 0xffu) : ((sc >> 8) & 0xffu)) << 23);
    p = u32x4{gemv_core::cvt2_e2m1<0>(d, s), gemv_core::cvt2_e2m1<1>(d, s), gemv_core::cvt2_e2m1<2>(d, s), gemv_core::cvt2_e2m1<3>(d, s)};
  } else {  // dwords 2 j, 2 j + 1: 8 bytes
    uint32_t a, b, c, d;
    gemv_core::cvt4_e4m3(w[j >> 1][(2 * j) & 3], a, b);
    gemv_core::cvt4_e4m3(w[j >> 1][(2 * j + 1) & 3], c, d);
    p = u32x4{a, b, c, d};
  }
  return __builtin_bit_cast(bf16x8, p);
}

// F: weight format; U: units of 16 rows per block; matrix m = u * NW + (0: W / W1, 1: W3) of the block
template <class F, int EPI, int G, int U>
__global__ __launch_bounds__(256) void gemm_skinny_q_kernel(GemmScaledArgs<typename F::scale_t> a) {
  constexpr int NW = (EPI == GEMM_SWIGLU) ? 2 : 1, NM = U * NW;
  constexpr int CH = ring_shape<F, NM, G>::CH, NB = ring_shape<F, NM, G>::NB;
  typedef QBatch<F, NM, G, CH> Batch;
  const GemmArgs& g = a.g;
  __shared__ f32x4 red[3][NM * G][64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, ls = lane >> 4;
  const int unit0 = blockIdx.x * U;

  // weight row n of matrix w (0 .. 2 of the arguments), in bytes, and where its scales start
  auto seg_of = [&](int n, int& w, int& r) {
    if (EPI == GEMM_SWIGLU || n < g.n0) { w = 0; r = n; }
    else if (n < g.n1) { w = 1; r = n - g.n0; }
    else { w = 2; r = n - g.n1; }
  };
  auto wbase = [&](int w) { return reinterpret_cast<const uint8_t*>(w == 0 ? g.w0 : w == 1 ? g.w1 : g.w2); };

  // ---- row pointers at this lane's k-slot.  Rows past the edge repeat the last valid one (dropped in the epilogue).
  const uint8_t* wrow[NM];
  const uint8_t* srow[NM];  // (block-scaled formats: the row's scale bytes at this lane's pair)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int n = min((unit0 + u) * 16 + lr, g.N - 1);
#pragma unroll
    for (int v = 0; v < NW; ++v) {
      int w, r;
      seg_of(n, w, r);
      if (EPI == GEMM_SWIGLU) w = v;
      wrow[u * NW + v] = wbase(w) + (size_t)r * F::row_bytes(g.K) + ls * 32;
      if constexpr (F::BLOCK) srow[u * NW + v] = reinterpret_cast<const uint8_t*>(a.sw[w]) + (size_t)r * (g.K >> 5) + ls * 2;
      else srow[u * NW + v] = nullptr;
    }
  }
  const bf16_t* xrow[G];
#pragma unroll
  for (int gg = 0; gg < G; ++gg) xrow[gg] = g.a + (size_t)min(gg * 16 + lr, g.M - 1) * g.lda + ls * (F::BK / 4);

  // epilogue operands that depend on nothing are the first loads of wave 0: the token positions of RoPE, the row scales of the
  // lane's four output columns (per-row formats)
  const bool rope = EPI == GEMM_STORE && g.rope_cs != nullptr;
  int tpos[G];
#pragma unroll
  for (int gg = 0; gg < G; ++gg) tpos[gg] = (rope && wid == 0) ? g.tok_pos[min(gg * 16 + lr, g.M - 1)] : 0;
  float rs[NM][4];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[m][r] = 1.f;
  if constexpr (!F::BLOCK) {
    if (wid == 0) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = min((unit0 + u) * 16 + ls * 4 + r, g.N - 1);
          int w, q;
          seg_of(n, w, q);
#pragma unroll
          for (int v = 0; v < NW; ++v) rs[u * NW + v][r] = a.sw[EPI == GEMM_SWIGLU ? v : w][q];
        }
    }
  }

  const int nk = g.K / F::BK;                               // chunks
  const int nbat = (nk + CH - 1) / CH;                      // batches of the block
  const int mine = wid < nbat ? (nbat - wid + 3) >> 2 : 0;  // batches of this wave: wid, wid + 4, ..

  Batch ring[NB];
  auto issue = [&](Batch& b, int i) {
    const int c0 = (wid + 4 * i) * CH;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int c = min(c0 + u, nk - 1);
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const uint8_t* p = wrow[m] + (size_t)c * 128;  // (a chunk is 128 bytes of a row in either format)
        b.w[m][u][0] = ld16_nt(p);
        b.w[m][u][1] = ld16_nt(p + 16);
        if constexpr (F::BLOCK) b.sc[m][u] = *reinterpret_cast<const uint16_t*>(srow[m] + c * 8);
      }
      const int koff = c * F::BK;
#pragma unroll
      for (int gg = 0; gg < G; ++gg)
#pragma unroll
        for (int j = 0; j < F::XP; ++j) b.x[gg][u][j] = ld16(xrow[gg] + koff + 8 * j);
    }
  };

  f32x4 acc[NM][G];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int gg = 0; gg < G; ++gg) acc[m][gg] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto consume = [&](const Batch& b, int i) {
    const int c0 = (wid + 4 * i) * CH;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      if (c0 + u < nk) {  // (wave-uniform; a chunk past the end of K holds the last chunk again)
#pragma unroll
        for (int j = 0; j < F::XP; ++j)
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            const bf16x8 wv = operand<F>(b.w[m][u], F::BLOCK ? b.sc[m][u] : 0u, j);
#pragma unroll
            for (int gg = 0; gg < G; ++gg)
              acc[m][gg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, __builtin_bit_cast(bf16x8, b.x[gg][u][j]), acc[m][gg], 0, 0, 0);
          }
      }
    }
  };

#pragma unroll
  for (int sl = 0; sl < NB; ++sl) issue(ring[sl], sl);
  // ALWAYS all NB steps per trip (gemm_skinny.hip): a step past the wave's last batch multiplies nothing and loads the last chunk again
  for (int i = 0; i < mine; i += NB) {
#pragma unroll
    for (int sl = 0; sl < NB; ++sl) {
      consume(ring[sl], i + sl);
      issue(ring[sl], i + sl + NB);
    }
  }

  // ---- the four partial sums, in wave order
  if (wid > 0) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int gg = 0; gg < G; ++gg) red[wid - 1][m * G + gg][lane] = acc[m][gg];
  }
  __syncthreads();
  if (wid > 0) return;
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int gg = 0; gg < G; ++gg)
#pragma unroll
      for (int w = 0; w < 3; ++w) acc[m][gg] += red[w][m * G + gg][lane];

  // ---- epilogue.  acc[u * NW + .][gg][r] is token gg * 16 + lr, output column (unit0 + u) * 16 + 4 ls + r
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int n0 = (unit0 + u) * 16 + ls * 4;
    if (n0 >= g.N) continue;
    const bool full = n0 + 3 < g.N;
    const int m0 = u * NW, m1 = u * NW + NW - 1;
#pragma unroll
    for (int gg = 0; gg < G; ++gg) {
      const int t = gg * 16 + lr;
      if (t >= g.M) continue;
      const size_t o = (size_t)t * g.ldo + n0;
      bf16_t* op = reinterpret_cast<bf16_t*>(g.out) + o;
      float y[4];
      if (EPI == GEMM_SWIGLU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = swiglu_bf_fast(acc[m0][gg][r] * rs[m0][r], acc[m1][gg][r] * rs[m1][r]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = bf_round(acc[m0][gg][r] * rs[m0][r]);
        if (EPI == GEMM_STORE && rope && n0 < g.rope_cols) {
          // (rope_cols is a multiple of rope_dh, rope_dh of 4: the lane's two pairs are both inside or both outside)
          const int i0 = ((n0 + g.rope_col0) % g.rope_dh) >> 1;
          const f32x4 cs = *reinterpret_cast<const f32x4*>(g.rope_cs + ((size_t)tpos[gg] * (g.rope_dh >> 1) + i0) * 2);
          float re, im;
          rope_pair(y[0], y[1], cs[0], cs[1], re, im);
          y[0] = bf_round(re);
          y[1] = bf_round(im);
          rope_pair(y[2], y[3], cs[2], cs[3], re, im);
          y[2] = bf_round(re);
          y[3] = bf_round(im);
        }
        if (EPI == GEMM_RESIDUAL) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + r < g.N) y[r] = bf_to_f(g.residual[o + r]) + y[r];
        }
      }
      if (full && (reinterpret_cast<uintptr_t>(op) & 7) == 0) {
        *reinterpret_cast<u32x2*>(op) = u32x2{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3])};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < g.N) op[r] = f_to_bf(y[r]);
      }
    }
  }
}

// Two units per block where that still gives every CU a block (the header's "L2 side")
template <class F, int EPI, int G>
hipError_t launch_g(const GemmScaledArgs<typename F::scale_t>& a, hipStream_t s) {
  const int pairs = (a.g.N + 31) / 32;
  if (pairs >= device_cus()) hipLaunchKernelGGL((gemm_skinny_q_kernel<F, EPI, G, 2>), dim3((unsigned)pairs), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_skinny_q_kernel<F, EPI, G, 1>), dim3((unsigned)((a.g.N + 15) / 16)), dim3(256), 0, s, a);
  return hipGetLastError();
}
template <class F, int EPI>
hipError_t launch_epi(const GemmScaledArgs<typename F::scale_t>& a, hipStream_t s) {
  switch ((a.g.M + 15) / 16) {
    case 1: return launch_g<F, EPI, 1>(a, s);
    case 2: return launch_g<F, EPI, 2>(a, s);
    case 3: return launch_g<F, EPI, 3>(a, s);
    default: return launch_g<F, EPI, 4>(a, s);
  }
}

inline bool aligned(const void* p, size_t n) { return (reinterpret_cast<size_t>(p) & (n - 1)) == 0; }

// shape and operands of the kernel itself (any bound on M above 0 is the caller's)
template <class F>
bool takes(const GemmScaledArgs<typename F::scale_t>& a) {
  const GemmArgs& g = a.g;
  if (g.tile_tab || g.a_gather || g.M <= 0 || g.M > 16 * SQ_MAX_G || g.N <= 0 || g.K <= 0 || g.K % F::BK != 0) return false;
  if (g.epi != GEMM_STORE && g.epi != GEMM_RESIDUAL && g.epi != GEMM_SWIGLU) return false;
  if (!g.w0 || !a.sw[0] || (g.epi == GEMM_SWIGLU && (!g.w1 || !a.sw[1]))) return false;
  if (g.lda % 8 != 0 || !aligned(g.a, 16) || !aligned(g.w0, 16) || !aligned(g.w1, 16) || !aligned(g.w2, 16)) return false;
  const size_t sa = F::BLOCK ? 2 : 4;  // the 16-bit load of a lane's scale pair (rows of K / 32 bytes: even); fp32 row scales
  return aligned(a.sw[0], sa) && aligned(a.sw[1], sa) && aligned(a.sw[2], sa);
}

template <class F>
hipError_t launch(const GemmScaledArgs<typename F::scale_t>& a, hipStream_t s) {
  if (!takes<F>(a)) return hipErrorInvalidValue;
  switch (a.g.epi) {
    case GEMM_STORE: return launch_epi<F, GEMM_STORE>(a, s);
    case GEMM_RESIDUAL: return launch_epi<F, GEMM_RESIDUAL>(a, s);
    default: return launch_epi<F, GEMM_SWIGLU>(a, s);
  }
}

}  // namespace

// The largest M the route gives to this kernel for a format and epilogue (0: none): the switch of gemm_skinny.hip, with the
// formats' own shipped bounds at mode 1
int gemm_skinny_q_max_rows(int format, int epi) {
  if (gemm_skinny_set_mode(-1) != 1) return gemm_skinny_max_rows(epi);  // off, or a mode above 1: every epilogue up to that many rows
  return format == MI_W4_MXFP4 ? GEMM_SKINNY_Q_MAX_M_W4 : GEMM_SKINNY_Q_MAX_M_W8;
}

bool gemm_skinny_w8_applicable(const GemmSkinnyW8Args& a) {
  return a.g.M > GEMV_MAX_T && a.g.M <= gemm_skinny_q_max_rows(MI_W8_FP8_E4M3, a.g.epi) && takes<FmtE4m3>(a);
}
bool gemm_skinny_w4_applicable(const GemmSkinnyW4Args& a) {
  return a.g.M > GEMV_MAX_T && a.g.M <= gemm_skinny_q_max_rows(MI_W4_MXFP4, a.g.epi) && takes<FmtMxfp4>(a);
}
hipError_t launch_gemm_skinny_w8(const GemmSkinnyW8Args& a, hipStream_t s) { return launch<FmtE4m3>(a, s); }
hipError_t launch_gemm_skinny_w4(const GemmSkinnyW4Args& a, hipStream_t s) { return launch<FmtMxfp4>(a, s); }
