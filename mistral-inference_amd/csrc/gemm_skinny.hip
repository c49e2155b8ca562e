// bf16 weight-streaming MFMA GEMM for 9 .. 64 rows (batched decode steps, short prompts, last prompt chunks):
// out[M,N] = epilogue(A[M,K] . W[N,K]^T), the plain form of GemmArgs with the STORE (+ RoPE) / RESIDUAL / SWIGLU / LOGITS epilogues.
//
// At these row counts the product is a stream of the weights, as the GEMVs of M <= 8 are, but with enough rows to feed the matrix
// cores.  The 128 x 128 tile kernel (gemm.hip) splits it over ceil(M / 128) * ceil(N / 128) blocks - 32 for Wo of a 7B model on
// 256 CUs - and fills 7/8 of every A tile with clamped rows.  Here:
//
//   unit     16 weight rows = the A operand of v_mfma_f32_16x16x32_bf16; the tokens are the B operand, 16 per group, G = ceil(M / 16)
//            groups (template parameter) reuse every weight fragment from registers.  One block per unit: N / 16 blocks of 4 waves
//            (SWIGLU: 16 rows of W1 and the matching 16 of W3, both accumulated for the same (token, j)).
//   weights  HBM -> VGPR with 16-byte non-temporal loads, no LDS: the load IS the operand layout.  Lane l holds row l % 16, k-slot
//            l / 16.  The k label of a slot is free as long as both operands agree on it, so a lane owns 32 CONTIGUOUS bytes of its
//            row per 64-wide K chunk (slot s = elements 16 s .. 16 s + 15: the first 8 go to the chunk's first MFMA, the other 8 to
//            the second) and the two loads of a chunk cover whole 128-byte lines of 16 rows.  Every weight byte is read once chip-wide.
//   tokens   the B fragments come from L2 in the same (row l % 16, 32 bytes at slot l / 16) form, loaded beside the weights they
//            multiply.  Every block reads all of x once: M / 16 times the weight bytes of a unit.
//   K split  the waves of a block take interleaved batches of CH chunks (wave w: batches w, w + 4, ..), so a block streams its 16
//            rows as 4 * CH * 128-byte runs.  A wave keeps a ring of NB batches (weights + tokens) in registers: every load is
//            unconditional with a clamped address (past the end of K: the last chunk again, never multiplied), the loop body is
//            consume batch i / refill the same registers with batch i + NB, and hipcc's counted vmcnt leaves the other NB - 1
//            batches in flight (the scheme of gemv_core.cuh).  No barrier and no LDS inside the loop.
//   reduce   waves 1 .. 3 leave their partial accumulators in LDS, wave 0 adds them as ((w0 + w1) + w2) + w3 - a fixed order, no
//            atomics, no scratch - and runs the epilogue.
//   epilogue the accumulator layout gives a lane 4 consecutive output columns of ONE token (columns 4 (l / 16) .. + 3 of the unit,
//            token l % 16 of the group): the (re, im) pairs of RoPE sit in one lane and the store is 8 bytes (16 for fp32 logits).
//            Rounding points, RoPE arithmetic and the fast SiLU are those of gemm.hip.
//   edges    rows >= N of the last unit and tokens >= M of the last group are clamped on load and masked on store.
#include <cstdlib>

#include "common.cuh"
#include "kernels.h"

namespace {

constexpr int SK_BK = 64;       // K chunk: two MFMAs of 32
constexpr int SK_MAX_G = 4;     // token groups of 16 a launch takes: 64 rows

// one ring entry: CH chunks of NW weight matrices and G token groups, two 16-byte pieces per chunk
template <int NW, int G, int CH>
struct SkBatch {
  u32x4 w[NW][CH][2];
  u32x4 x[G][CH][2];
};

template <int EPI, int G, int CH, int NB>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmArgs g) {
  constexpr int NW = (EPI == GEMM_SWIGLU) ? 2 : 1;
  __shared__ f32x4 red[3][NW * G][64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, ls = lane >> 4;
  const int unit = blockIdx.x;

  // ---- row pointers at this lane's k-slot.  Rows past the edge repeat the last valid one (dropped in the epilogue).
  const bf16_t* wrow[NW];
  {
    const int n = min(unit * 16 + lr, g.N - 1);
    if (EPI == GEMM_SWIGLU) {
      wrow[0] = g.w0 + (size_t)n * g.K + ls * 16;
      wrow[NW - 1] = g.w1 + (size_t)n * g.K + ls * 16;
    } else {
      wrow[0] = seg_row(g, n) + ls * 16;
    }
  }
  const bf16_t* xrow[G];
#pragma unroll
  for (int gg = 0; gg < G; ++gg) xrow[gg] = g.a + (size_t)min(gg * 16 + lr, g.M - 1) * g.lda + ls * 16;

  // the token positions of the RoPE epilogue are the first loads of wave 0: they are old when the epilogue wants them
  const bool rope = EPI == GEMM_STORE && g.rope_cs != nullptr;
  int tpos[G];
#pragma unroll
  for (int gg = 0; gg < G; ++gg) tpos[gg] = (rope && wid == 0) ? g.tok_pos[min(gg * 16 + lr, g.M - 1)] : 0;

  const int nk = g.K / SK_BK;                               // chunks
  const int nbat = (nk + CH - 1) / CH;                      // batches of the block
  const int mine = wid < nbat ? (nbat - wid + 3) >> 2 : 0;  // batches of this wave: wid, wid + 4, ..

  SkBatch<NW, G, CH> ring[NB];
  auto issue = [&](SkBatch<NW, G, CH>& b, int i) {
    const int c0 = (wid + 4 * i) * CH;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int koff = min(c0 + u, nk - 1) * SK_BK;
#pragma unroll
      for (int m = 0; m < NW; ++m) {
        b.w[m][u][0] = ld16_nt(wrow[m] + koff);
        b.w[m][u][1] = ld16_nt(wrow[m] + koff + 8);
      }
#pragma unroll
      for (int gg = 0; gg < G; ++gg) {
        b.x[gg][u][0] = ld16(xrow[gg] + koff);
        b.x[gg][u][1] = ld16(xrow[gg] + koff + 8);
      }
    }
  };

  f32x4 acc[NW][G];
#pragma unroll
  for (int m = 0; m < NW; ++m)
#pragma unroll
    for (int gg = 0; gg < G; ++gg) acc[m][gg] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto consume = [&](const SkBatch<NW, G, CH>& b, int i) {
    const int c0 = (wid + 4 * i) * CH;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      if (c0 + u < nk) {  // (wave-uniform; a chunk past the end of K holds the last chunk again)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int m = 0; m < NW; ++m)
#pragma unroll
            for (int gg = 0; gg < G; ++gg)
              acc[m][gg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b.w[m][u][j]),
                                                                   __builtin_bit_cast(bf16x8, b.x[gg][u][j]), acc[m][gg], 0, 0, 0);
      }
    }
  };

#pragma unroll
  for (int sl = 0; sl < NB; ++sl) issue(ring[sl], sl);
  // ALWAYS all NB steps per trip (gemv_core.cuh: a skip edge inside the trip makes hipcc drain the ring); a step past the wave's
  // last batch multiplies nothing and loads the last chunk once more
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
    for (int m = 0; m < NW; ++m)
#pragma unroll
      for (int gg = 0; gg < G; ++gg) red[wid - 1][m * G + gg][lane] = acc[m][gg];
  }
  __syncthreads();
  if (wid > 0) return;
#pragma unroll
  for (int m = 0; m < NW; ++m)
#pragma unroll
    for (int gg = 0; gg < G; ++gg)
#pragma unroll
      for (int w = 0; w < 3; ++w) acc[m][gg] += red[w][m * G + gg][lane];

  // ---- epilogue.  acc[.][gg][r] is token gg * 16 + lr, output column unit * 16 + 4 ls + r
  const int n0 = unit * 16 + ls * 4;
  if (n0 >= g.N) return;
  const bool full = n0 + 3 < g.N;
#pragma unroll
  for (int gg = 0; gg < G; ++gg) {
    const int t = gg * 16 + lr;
    if (t >= g.M) continue;
    const size_t o = (size_t)t * g.ldo + n0;
    if (EPI == GEMM_SWIGLU) {
      float h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = swiglu_bf_fast(acc[0][gg][r], acc[NW - 1][gg][r]);
      bf16_t* op = reinterpret_cast<bf16_t*>(g.out) + o;
      if (full && (reinterpret_cast<uintptr_t>(op) & 7) == 0) {
        *reinterpret_cast<u32x2*>(op) = u32x2{pack_bf2(h[0], h[1]), pack_bf2(h[2], h[3])};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < g.N) op[r] = f_to_bf(h[r]);
      }
      continue;
    }
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = bf_round(acc[0][gg][r]);
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
    if (EPI == GEMM_LOGITS) {
      float* op = reinterpret_cast<float*>(g.out) + o;
      if (full && (reinterpret_cast<uintptr_t>(op) & 15) == 0) {
        *reinterpret_cast<f32x4*>(op) = f32x4{y[0], y[1], y[2], y[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < g.N) op[r] = y[r];
      }
      continue;
    }
    if (EPI == GEMM_RESIDUAL) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < g.N) y[r] = bf_to_f(g.residual[o + r]) + y[r];
    }
    bf16_t* op = reinterpret_cast<bf16_t*>(g.out) + o;
    if (full && (reinterpret_cast<uintptr_t>(op) & 7) == 0) {
      *reinterpret_cast<u32x2*>(op) = u32x2{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3])};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < g.N) op[r] = f_to_bf(y[r]);
    }
  }
}

// Ring shape per group count: a batch is CH chunks (CH * 2 KiB of weights per wave), NB batches in flight.  Sized so that a wave
// holds 8 .. 16 KiB of weights in flight at one group and the ring stays under 200 VGPRs at four (profiles/EXPERIMENTS.md).
template <int EPI, int G>
hipError_t launch_g(const GemmArgs& g, hipStream_t s) {
  constexpr int CH = G == 1 ? 4 : 2, NB = G == 2 ? 3 : 2;
  hipLaunchKernelGGL((gemm_skinny_kernel<EPI, G, CH, NB>), dim3((unsigned)((g.N + 15) / 16)), dim3(256), 0, s, g);
  return hipGetLastError();
}
template <int EPI>
hipError_t launch_epi(const GemmArgs& g, hipStream_t s) {
  switch ((g.M + 15) / 16) {
    case 1: return launch_g<EPI, 1>(g, s);
    case 2: return launch_g<EPI, 2>(g, s);
    case 3: return launch_g<EPI, 3>(g, s);
    default: return launch_g<EPI, 4>(g, s);
  }
}

// rows [m0, m0 + rows) of the same problem
GemmArgs row_slice(const GemmArgs& g, int m0, int rows) {
  GemmArgs r = g;
  r.M = rows;
  r.a = g.a + (size_t)m0 * g.lda;
  r.out = reinterpret_cast<char*>(g.out) + (size_t)m0 * g.ldo * (g.epi == GEMM_LOGITS ? 4 : 2);
  if (g.residual) r.residual = g.residual + (size_t)m0 * g.ldo;
  if (g.tok_pos) r.tok_pos = g.tok_pos + m0;
  return r;
}

// MI_GEMM_SKINNY / mi_debug_set_gemm_skinny: 0 off, 1 on with the shipped bounds, above 1: every epilogue up to that many rows
// (tests of the kernel itself, probes)
int skinny_mode = -1;

int mode_now() {
  if (skinny_mode < 0) {
    const char* e = getenv("MI_GEMM_SKINNY");
    skinny_mode = e ? atoi(e) : 1;
    if (skinny_mode < 0) skinny_mode = 1;
  }
  return skinny_mode;
}

}  // namespace

int gemm_skinny_set_mode(int mode) {
  const int prev = mode_now();
  if (mode >= 0) skinny_mode = mode;
  return prev;
}

// The largest M launch_gemm gives to this kernel (0: none).  The LM head stops at 48 rows: at 64 every block reads 4 x its weight
// bytes of activations from L2 and the head's 2048 blocks measured 12 % slower than the 128-tile kernel (profiles/EXPERIMENTS.md);
// the four linears of a layer are faster up to 64.
int gemm_skinny_max_rows(int epi) {
  const int m = mode_now();
  return m == 1 ? (epi == GEMM_LOGITS ? GEMM_SKINNY_MAX_M_LOGITS : GEMM_SKINNY_MAX_M) : m;
}

bool gemm_skinny_applicable(const GemmArgs& g) {
  return g.tile_tab == nullptr && g.a_gather == nullptr && g.M > GEMV_MAX_T && g.M <= gemm_skinny_max_rows(g.epi) && g.N > 0 && g.K > 0 &&
         g.K % SK_BK == 0 && (g.epi == GEMM_STORE || g.epi == GEMM_RESIDUAL || g.epi == GEMM_SWIGLU || g.epi == GEMM_LOGITS);
}

// Any M >= 1 (the route keeps it to 9 .. 64): more than 64 rows run as launches of 64, each streaming the weights again.
hipError_t launch_gemm_skinny(const GemmArgs& g, hipStream_t s) {
  if (g.tile_tab || g.a_gather || g.M <= 0 || g.N <= 0 || g.K <= 0 || g.K % SK_BK != 0) return hipErrorInvalidValue;
  for (int m0 = 0; m0 < g.M; m0 += 16 * SK_MAX_G) {
    const GemmArgs p = row_slice(g, m0, g.M - m0 < 16 * SK_MAX_G ? g.M - m0 : 16 * SK_MAX_G);
    hipError_t e;
    switch (g.epi) {
      case GEMM_STORE: e = launch_epi<GEMM_STORE>(p, s); break;
      case GEMM_RESIDUAL: e = launch_epi<GEMM_RESIDUAL>(p, s); break;
      case GEMM_SWIGLU: e = launch_epi<GEMM_SWIGLU>(p, s); break;
      case GEMM_LOGITS: e = launch_epi<GEMM_LOGITS>(p, s); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
