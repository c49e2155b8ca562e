// W8A8 MFMA GEMM for prefills of FP8 models: out[M,N] = epilogue((A_q . W_q^T)[m, n] * s_x[m] * s_w[n]), A_q [M, K] e4m3 bytes with one
// fp32 scale per row (act_quant_e4m3, elementwise.hip), W_q [N, K] e4m3 bytes with one fp32 scale per row (the checkpoint's).
//
// The structure is gemm256.hip's, on the same bytes: 8 waves = 2 (M) x 4 (N), a 256 x 256 block tile, half tiles of 128 rows x 128 B
// staged by `global_load_lds` (16 bytes per lane, the 16-byte slot XOR-swizzled by row & 7 on the DMA's SOURCE address), two stages,
// four phases per K tile with the single counted `vmcnt(6)` per tile, the wr = 1 waves one barrier behind the wr = 0 waves.  What
// changes is the element: at one byte each a half tile's 128-byte row is K = 128, i.e. ONE `v_mfma_scale_f32_16x16x128_f8f6f4` per
// (row fragment, column fragment) where the bf16 kernel issues two 16x16x32 - the same LDS bytes per MFMA clock carry twice the flops.
// Both block-scale operands are 127 (2^0): the scales that matter are per ROW of either operand and enter in the epilogue.
//
// Fragments: lane l reads the 32 bytes k = 32 * (l >> 4) .. + 32 of row / column l & 15, for A and for B alike.  The contraction
// pairs A's and B's bytes register by register, so any k map that is the same for both operands (the hardware's is) gives the
// sum over all 128 k; tests/test_gpu_w8a8.py holds the exact structured cases that would show a wrong one.
// C/D: the 16x16 fp32 layout of the bf16 form.  MFMAs are issued W-fragment x A-fragment (transposed tiles) so that a lane holds
// four consecutive output columns, as gemm256.hip does for its bf16 epilogues.
//
// Epilogues: GEMM_STORE (with the RoPE epilogue of q|k|v and up to three weight segments), GEMM_RESIDUAL, GEMM_SWIGLU; the rounding
// points are the bf16 kernel's, with acc * (s_x[m] * s_w[n]) in fp32 where the bf16 kernel reads acc (gemv_core.cuh F::SCALED).
// No LM head, no token-grouped form, no half-height tail tile.
#include "common.cuh"
#include "kernels.h"

using E = Elem16<0>;  // outputs, residual and the RoPE / SwiGLU chains are bf16

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;                      // bytes = e4m3 elements of K per tile
constexpr int HALF_BYTES = 128 * BK;         // 16 KiB: 128 rows x 128 B
constexpr int STAGE_BYTES = 4 * HALF_BYTES;  // A0 A1 B0 B1
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 128 KiB

__device__ __forceinline__ void dma16(const uint8_t* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void lds_reads_done_then_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();
}
// weight row r (bytes) of up to three matrices side by side, and its scale
__device__ __forceinline__ const uint8_t* seg_row8(const GemmArgs& g, int r) {
  const uint8_t *w0 = reinterpret_cast<const uint8_t*>(g.w0), *w1 = reinterpret_cast<const uint8_t*>(g.w1),
                *w2 = reinterpret_cast<const uint8_t*>(g.w2);
  if (r < g.n0) return w0 + (size_t)r * g.K;
  if (r < g.n1) return w1 + (size_t)(r - g.n0) * g.K;
  return w2 + (size_t)(r - g.n1) * g.K;
}
__device__ __forceinline__ float seg_scale(const GemmW8A8Args& a, int r) {
  if (r < a.g.n0) return a.sw[0][r];
  if (r < a.g.n1) return a.sw[1][r - a.g.n0];
  return a.sw[2][r - a.g.n1];
}
__device__ __forceinline__ i32x8 frag32(const char* row, int s0, int s1) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(row + s0), hi = *reinterpret_cast<const u32x4*>(row + s1);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// e4m3 x e4m3 (format codes 0, 0), both block scales 2^(127 - 127)
__device__ __forceinline__ f32x4 mfma128(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_w8a8_kernel(GemmW8A8Args args) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& g = args.g;
  constexpr int NOUT = (EPI == GEMM_SWIGLU) ? 128 : 256;  // output columns per block
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  // ---- block -> tile: gemm256.hip's 4 (m) x 8 (n) supertiles, one per XCD at a time
  const int m_tiles = (g.M + 255) >> 8, n_tiles = (g.N + NOUT - 1) / NOUT;
  const int MS = (m_tiles + 3) >> 2, NS = (n_tiles + 7) >> 3;
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int st = (q >> 5) * 8 + xcd, wi = q & 31;
  if (st >= MS * NS) return;
  const int m_tile = (st % MS) * 4 + (wi & 3), n_tile = (st / MS) * 8 + (wi >> 2);
  if (m_tile >= m_tiles || n_tile >= n_tiles) return;
  const int row0 = m_tile * 256, rows_valid = min(256, g.M - row0);

  // ---- DMA sources.  One instruction fills 8 consecutive 128-B rows of a half tile; wave w, piece j covers rows (2w + j) * 8 .. + 8;
  // lane l lands at (row + (l >> 3), slot l & 7) and fetches global slot (l & 7) ^ (row & 7).  Rows at or past M / N are clamped to
  // the last valid one: never read out of bounds, never stored.
  const int sslot = (lane & 7) ^ ((lane >> 3) & 7);
  const uint8_t* const a8 = reinterpret_cast<const uint8_t*>(g.a);
  const uint8_t* src[4][2];  // halves of a stage: A0 A1 B0 B1
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = (wid * 2 + j) * 8 + (lane >> 3);
      const int m = row0 + min(h * 128 + r, rows_valid - 1);
      src[h][j] = a8 + (size_t)m * g.lda + sslot * 16;
      if (EPI == GEMM_SWIGLU) {
        const int n = min(n_tile * 128 + r, g.N - 1);
        src[2 + h][j] = reinterpret_cast<const uint8_t*>(h == 0 ? g.w0 : g.w1) + (size_t)n * g.K + sslot * 16;
      } else {
        const int n = min(n_tile * 256 + h * 128 + r, g.N - 1);
        src[2 + h][j] = seg_row8(g, n) + sslot * 16;
      }
    }
  char* const my_piece = smem + wid * 2048;  // this wave's two 1-KiB pieces inside any half tile
#define STAGE_HALF(HALF, KT, STAGE)                                    \
  do {                                                                 \
    char* dst_ = my_piece + (STAGE) * STAGE_BYTES + (HALF) * HALF_BYTES; \
    dma16(src[HALF][0] + (size_t)(KT) * BK, dst_);                     \
    dma16(src[HALF][1] + (size_t)(KT) * BK, dst_ + 1024);              \
  } while (0)

  // ---- fragment addressing: lane holds row lane & 15, bytes 32 * (lane >> 4) .. + 32 = the 16-byte slots 2 fq and 2 fq + 1
  const int fq = lane >> 4;
  const int sw0 = ((2 * fq) ^ (lane & 7)) << 4, sw1 = ((2 * fq + 1) ^ (lane & 7)) << 4;
  const int a_off = (wr * 64 + (lane & 15)) * 128;
  const int b_off = 2 * HALF_BYTES + (wc * 32 + (lane & 15)) * 128;

  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  i32x8 af[4];          // [row fragment] of the A half in use
  i32x8 b0x[2], b1[2];  // [column fragment] of B half 0 / 1
#define READ_A(HA, SB)                                                                    \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) af[i] = frag32((SB) + (HA) * HALF_BYTES + a_off + i * 2048, sw0, sw1);
#define READ_B(DST, HB, SB)                                                               \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) DST[j] = frag32((SB) + (HB) * HALF_BYTES + b_off + j * 2048, sw0, sw1);
#define SEGMENT_END()                          \
  do {                                         \
    lds_reads_done_then_barrier();             \
    __builtin_amdgcn_sched_barrier(0);         \
  } while (0)
#define MFMA_END()                             \
  do {                                         \
    __builtin_amdgcn_sched_barrier(0);         \
    raw_barrier();                             \
    __builtin_amdgcn_sched_barrier(0);         \
  } while (0)
#define MFMA_QUAD(HA, HB, BF)                                                             \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                           \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                           \
    acc[HA][HB][i][j] = mfma128(BF[j], af[i], acc[HA][HB][i][j]);

  const int nk = g.K / BK;
  // ---- prologue: all of tile 0, then A0 B0 B1 of tile 1 (its A1 is staged by phase 1 of tile 0)
  STAGE_HALF(0, 0, 0);
  STAGE_HALF(2, 0, 0);
  STAGE_HALF(3, 0, 0);
  STAGE_HALF(1, 0, 0);
  if (nk > 1) {
    STAGE_HALF(0, 1, 1);
    STAGE_HALF(2, 1, 1);
    STAGE_HALF(3, 1, 1);
    wait_vm<6>();
  } else {
    wait_vm<0>();
  }
  raw_barrier();
  // Every phase is two segments, [fragment reads + one half tile's DMA] | barrier | [8 MFMAs] | barrier, and the wr = 1 waves run
  // one barrier behind the wr = 0 waves: the hazard argument is gemm256.hip's, word for word (a half is re-staged in the read
  // segment after the one in which it was last read; tile t + 1 is waited for in phase 4's first segment and read two barriers later).
  if (wr == 1) raw_barrier();
  for (int t = 0; t < nk; ++t) {
    const int s = t & 1;
    const char* sb = smem + s * STAGE_BYTES;
    const bool more1 = t + 1 < nk, more2 = t + 2 < nk;
    // phase 1: quadrant (0, 0)
    READ_B(b0x, 0, sb)
    READ_A(0, sb)
    if (more1) STAGE_HALF(1, t + 1, s ^ 1);  // A1 of the other stage: last read in phase 3 of tile t - 1
    SEGMENT_END();
    MFMA_QUAD(0, 0, b0x)
    MFMA_END();
    // phase 2: quadrant (0, 1)
    READ_B(b1, 1, sb)
    if (more2) STAGE_HALF(0, t + 2, s);  // A0: read in phase 1
    SEGMENT_END();
    MFMA_QUAD(0, 1, b1)
    MFMA_END();
    // phase 3: quadrant (1, 1)
    READ_A(1, sb)
    if (more2) STAGE_HALF(2, t + 2, s);  // B0: read in phase 1
    SEGMENT_END();
    MFMA_QUAD(1, 1, b1)
    MFMA_END();
    // phase 4: quadrant (1, 0); retire tile t + 1 (everything issued before the last three halves)
    if (more2) {
      STAGE_HALF(3, t + 2, s);  // B1: read in phase 2
      wait_vm<6>();
    } else {
      wait_vm<0>();
    }
    SEGMENT_END();
    MFMA_QUAD(1, 0, b0x)
    MFMA_END();
  }
  if (wr == 0) raw_barrier();
#undef STAGE_HALF
#undef READ_A
#undef READ_B
#undef MFMA_QUAD
#undef SEGMENT_END
#undef MFMA_END

  // ---- epilogue.  acc[ha][hb][i][j][r] is tile row ha*128 + wr*64 + i*16 + (lane & 15), tile column hb*128 + wc*32 + j*16 +
  // (lane >> 4)*4 + r (SwiGLU: hb = 0 is W1's product and hb = 1 W3's, of column wc*32 + j*16 + (lane >> 4)*4 + r).
  const int cq = (lane >> 4) * 4;
  const bool rope = EPI == GEMM_STORE && g.rope_cs != nullptr;
  const bool wide_ok = (g.ldo & 3) == 0 && (reinterpret_cast<size_t>(g.out) & 15) == 0 &&
                       (EPI != GEMM_RESIDUAL || (reinterpret_cast<size_t>(g.residual) & 7) == 0);
#pragma unroll
  for (int ha = 0; ha < 2; ++ha)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rl = ha * 128 + wr * 64 + i * 16 + (lane & 15);
      if (rl >= rows_valid) continue;
      const int row = row0 + rl;
      const size_t ob = (size_t)row * g.ldo;
      const float sx = args.sx[row];
      const int tp = rope ? g.tok_pos[row] : 0;
      if (EPI == GEMM_SWIGLU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = n_tile * 128 + wc * 32 + j * 16 + cq;
          if (n >= g.N) continue;
          float y[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nn = min(n + r, g.N - 1);
            y[r] = E::swiglu_fast(acc[ha][0][i][j][r] * (sx * args.sw[0][nn]), acc[ha][1][i][j][r] * (sx * args.sw[1][nn]));
          }
          bf16_t* o = reinterpret_cast<bf16_t*>(g.out) + ob + n;
          if (n + 3 < g.N && wide_ok) {
            *reinterpret_cast<uint2*>(o) = make_uint2(E::pack2(y[0], y[1]), E::pack2(y[2], y[3]));
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (n + r < g.N) o[r] = E::from_f(y[r]);
          }
        }
      } else {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int n = n_tile * 256 + hb * 128 + wc * 32 + j * 16 + cq;
            if (n >= g.N) continue;
            const bool full = (n + 3 < g.N) && wide_ok;
            float y[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = E::round(acc[ha][hb][i][j][r] * (sx * seg_scale(args, min(n + r, g.N - 1))));
            if (EPI == GEMM_STORE && rope && n < g.rope_cols) {
              // rotary embedding on the bf16-rounded projection, as gemm256.hip: this lane's four columns are two (re, im) pairs
              const int i0 = ((n + g.rope_col0) % g.rope_dh) >> 1;
              const f32x4 cs = *reinterpret_cast<const f32x4*>(g.rope_cs + ((size_t)tp * (g.rope_dh >> 1) + i0) * 2);
              float re, im;
              rope_pair(y[0], y[1], cs[0], cs[1], re, im);
              y[0] = E::round(re); y[1] = E::round(im);
              rope_pair(y[2], y[3], cs[2], cs[3], re, im);
              y[2] = E::round(re); y[3] = E::round(im);
            }
            bf16_t* o = reinterpret_cast<bf16_t*>(g.out) + ob + n;
            if (full) {
              if (EPI == GEMM_RESIDUAL) {
                const uint2 rs = *reinterpret_cast<const uint2*>(g.residual + ob + n);
                y[0] += E::lo(rs.x); y[1] += E::hi(rs.x); y[2] += E::lo(rs.y); y[3] += E::hi(rs.y);
              }
              *reinterpret_cast<uint2*>(o) = make_uint2(E::pack2(y[0], y[1]), E::pack2(y[2], y[3]));
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n + r < g.N) o[r] = E::from_f(EPI == GEMM_RESIDUAL ? E::to_f(g.residual[ob + n + r]) + y[r] : y[r]);
            }
          }
      }
    }
}

template <int EPI>
hipError_t launch_one(const GemmW8A8Args& a, dim3 grid, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS needs the opt-in once per kernel
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm256_w8a8_kernel<EPI>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm256_w8a8_kernel<EPI>), grid, dim3(512), LDS_BYTES, s, a);
  return hipGetLastError();
}

}  // namespace

// (K <= 16384: the activation quantiser in front of this GEMM holds a row in registers, elementwise.hip)
bool gemm256_w8a8_applicable(int M, int K) { return M >= 256 && K >= BK && K % BK == 0 && K <= 16384; }

hipError_t launch_gemm256_w8a8(const GemmW8A8Args& a, hipStream_t s) {
  const GemmArgs& g = a.g;
  if (!gemm256_w8a8_applicable(g.M, g.K) || g.lda < g.K || (g.lda & 15) || (reinterpret_cast<size_t>(g.a) & 15) || g.tile_tab ||
      g.a_gather || !a.sx || !g.w0 || !a.sw[0] || g.N <= 0 || g.n0 <= 0)
    return hipErrorInvalidValue;
  // every DMA fetches 16 aligned bytes: the weight rows are K = 128 k bytes apart, so their bases decide
  if ((reinterpret_cast<size_t>(g.w0) | reinterpret_cast<size_t>(g.w1) | reinterpret_cast<size_t>(g.w2)) & 15) return hipErrorInvalidValue;
  if (g.epi == GEMM_SWIGLU ? (!g.w1 || !a.sw[1]) : ((g.n0 < g.N && (!g.w1 || !a.sw[1])) || (g.n1 < g.N && (!g.w2 || !a.sw[2]))))
    return hipErrorInvalidValue;
  const int nout = (g.epi == GEMM_SWIGLU) ? 128 : 256;
  const int m_tiles = (g.M + 255) >> 8, n_tiles = (g.N + nout - 1) / nout;
  const int supertiles = ((m_tiles + 3) >> 2) * ((n_tiles + 7) >> 3);
  const dim3 grid((unsigned)(((supertiles + 7) / 8) * 8 * 32));
  switch (g.epi) {
    case GEMM_STORE: return launch_one<GEMM_STORE>(a, grid, s);
    case GEMM_RESIDUAL: return launch_one<GEMM_RESIDUAL>(a, grid, s);
    case GEMM_SWIGLU: return launch_one<GEMM_SWIGLU>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}
