// W8A8 MFMA GEMM for prefills of FP8 models: out[M,N] = epilogue((A_q . W_q^T)[m, n] * s_x[m] * s_w[n]), A_q [M, K] e4m3 bytes with one
// fp32 scale per row (act_quant_e4m3, elementwise.hip), W_q [N, K] e4m3 bytes with one fp32 scale per row (the checkpoint's).
//
// Tile map, K loop, hazard argument, epilogue and launcher are gemm256_core.cuh's, on the bf16 kernel's LDS image: half tiles of
// 128 rows x 128 B (the 16-byte slot XOR-swizzled by row & 7 on the DMA's SOURCE address), two stages of A0 A1 B0 B1, two DMAs per
// wave and half.  What is this file's own is the element: at one byte each a half tile's 128-byte row is K = 128, i.e. ONE
// `v_mfma_scale_f32_16x16x128_f8f6f4` per (row fragment, column fragment) where the bf16 kernel issues two 16x16x32 - the same
// LDS bytes per MFMA clock carry twice the flops.  Both block-scale operands are 127 (2^0): the scales that matter are per ROW of
// either operand and enter in the epilogue (gemm256_core ScaleRowCol: acc * (s_x[m] * s_w[n]) in fp32 where the bf16 kernel reads
// acc, as gemv_core.cuh F::SCALED).
//
// Fragments: lane l reads the 32 bytes k = 32 * (l >> 4) .. + 32 of row / column l & 15, for A and for B alike.  The contraction
// pairs A's and B's bytes register by register, so any k map that is the same for both operands (the hardware's is) gives the
// sum over all 128 k; tests/test_gpu_w8a8.py holds the exact structured cases that would show a wrong one.
// C/D: the 16x16 fp32 layout of the bf16 form.  MFMAs are issued W-fragment x A-fragment (transposed tiles) so that a lane holds
// four consecutive output columns, as the shared epilogue expects.
//
// Epilogues: GEMM_STORE (with the RoPE epilogue of q|k|v and up to three weight segments), GEMM_RESIDUAL, GEMM_SWIGLU.
// No LM head, no token-grouped form, no half-height tail tile.
#include "gemm256_core.cuh"

using E = Elem16<0>;  // outputs, residual and the RoPE / SwiGLU chains are bf16

namespace {
using namespace gemm256_core;

constexpr int BK = 128;                      // bytes = e4m3 elements of K per tile
constexpr int HALF_BYTES = 128 * BK;         // 16 KiB: 128 rows x 128 B
constexpr int STAGE_BYTES = 4 * HALF_BYTES;  // A0 A1 B0 B1
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 128 KiB

// weight row r (bytes) of up to three matrices side by side
__device__ __forceinline__ const char* seg_row8(const GemmArgs& g, int r) {
  const char *w0 = reinterpret_cast<const char*>(g.w0), *w1 = reinterpret_cast<const char*>(g.w1), *w2 = reinterpret_cast<const char*>(g.w2);
  if (r < g.n0) return w0 + (size_t)r * g.K;
  if (r < g.n1) return w1 + (size_t)(r - g.n0) * g.K;
  return w2 + (size_t)(r - g.n1) * g.K;
}

// The operands of gemm256_core::k_loop: e4m3 x e4m3 (format codes 0, 0), both block scales 2^(127 - 127)
struct Ops {
  static constexpr int dmas(int) { return 2; }
  const char* src[4][2];  // [half][piece]
  char* my_piece;         // this wave's two 1-KiB pieces inside any half tile of stage 0
  const char* smem;
  int a_off, b_off, sw0, sw1;  // fragment addressing
  f32x4 acc[2][2][4][2];
  i32x8 af[4];     // [row fragment] of the A half in use
  i32x8 bf[2][2];  // [B half][column fragment]

  __device__ __forceinline__ void stage(int half, int kt, int st) {
    char* dst = my_piece + st * STAGE_BYTES + half * HALF_BYTES;
    dma16(src[half][0] + (size_t)kt * BK, dst);
    dma16(src[half][1] + (size_t)kt * BK, dst + 1024);
  }
  __device__ __forceinline__ void read_a(int ha, int st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = frag32(smem + st * STAGE_BYTES + ha * HALF_BYTES + a_off + i * 2048, sw0, sw1);
  }
  __device__ __forceinline__ void read_b(int hb, int st) {
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[hb][j] = frag32(smem + st * STAGE_BYTES + hb * HALF_BYTES + b_off + j * 2048, sw0, sw1);
  }
  __device__ __forceinline__ void mfma_quad(int ha, int hb) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[ha][hb][i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[hb][j], af[i], acc[ha][hb][i][j], 0, 0, 0, 127, 0, 127);
  }
};

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_w8a8_kernel(GemmW8A8Args args) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& g = args.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  int m_tile, n_tile;
  if (!tile_of_block((g.M + 255) >> 8, col_tiles(g.N, EPI), m_tile, n_tile)) return;
  const int row0 = m_tile * 256, rows_valid = min(256, g.M - row0);

  Ops op;
  // ---- DMA sources (gemm256_core: both operands are 16-KiB halves).  Rows at or past M / N are clamped to the last valid one.
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      op.src[h][j] = a_half_src<uint8_t, false>(g, row0, rows_valid, h, wid, j, lane);
      const int r = piece_row(wid, j, lane);
      if (EPI == GEMM_SWIGLU) {
        const int n = min(n_tile * 128 + r, g.N - 1);
        op.src[2 + h][j] = reinterpret_cast<const char*>(h == 0 ? g.w0 : g.w1) + (size_t)n * g.K + src_slot_bytes(lane);
      } else {
        const int n = min(n_tile * 256 + h * 128 + r, g.N - 1);
        op.src[2 + h][j] = seg_row8(g, n) + src_slot_bytes(lane);
      }
    }
  op.my_piece = smem + wid * 2048;
  op.smem = smem;
  // ---- fragment addressing: lane holds row lane & 15, bytes 32 * (lane >> 4) .. + 32 = the 16-byte slots 2 fq and 2 fq + 1
  const int fq = lane >> 4;
  op.sw0 = ((2 * fq) ^ (lane & 7)) << 4;
  op.sw1 = ((2 * fq + 1) ^ (lane & 7)) << 4;
  op.a_off = (wr * 64 + (lane & 15)) * 128;
  op.b_off = 2 * HALF_BYTES + (wc * 32 + (lane & 15)) * 128;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) op.acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  k_loop<true>(op, g.K / BK, wr);
  epilogue16<E, EPI, 2>(g, op.acc, ScaleRowCol{args}, row0, rows_valid, n_tile, wr, wc, lane);
}

}  // namespace

// (K <= 16384: the activation quantiser in front of this GEMM holds a row in registers, elementwise.hip)
bool gemm256_w8a8_applicable(int M, int K) { return M >= 256 && K >= BK && K % BK == 0 && K <= 16384; }

hipError_t launch_gemm256_w8a8(const GemmW8A8Args& a, hipStream_t s) {
  const GemmArgs& g = a.g;
  if (!a8_args_ok(a)) return hipErrorInvalidValue;
  const dim3 grid = tile_grid((g.M + 255) >> 8, col_tiles(g.N, g.epi));
  switch (g.epi) {
    case GEMM_STORE: return launch_one<&gemm256_w8a8_kernel<GEMM_STORE>, LDS_BYTES>(a, grid, s);
    case GEMM_RESIDUAL: return launch_one<&gemm256_w8a8_kernel<GEMM_RESIDUAL>, LDS_BYTES>(a, grid, s);
    case GEMM_SWIGLU: return launch_one<&gemm256_w8a8_kernel<GEMM_SWIGLU>, LDS_BYTES>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}
