// Weight-streaming GEMV launches for M <= 8 tokens whose weight rows are OCP e4m3 bytes (weight-only FP8), and the
// dequantisation pass of the prefill route.
//
// The kernels are gemv_core::gemv_body on the WE4m3 format (gemv_core.cuh: design notes, conversion, where the row scales enter);
// the activation staging is the bf16 kernels', so the normalised rows in LDS are bit-identical to theirs.
//
// A row is half the bytes of a bf16 row, so the fixed cost of a unit (wave reductions, epilogue, loop bookkeeping) weighs twice
// as much.  Units are therefore RP row pairs: RP = 2 (four rows) where the matrix has enough row pairs that every wave of the grid
// still gets at least two units (W1|W3), else RP = 1 (W8::row_pairs; MI_GEMV_W8_RP: its A/B switch).
#include <cstdlib>

#include "common.cuh"
#include "gemv_core.cuh"

namespace {

using namespace gemv_core;

// TT: token rows staged in LDS; MODE: GEMV_STORE / GEMV_RESIDUAL / GEMV_SWIGLU / GEMV_QKV_ROPE, and GEMV_LOGITS for a quantised LM
// head (logit = float(bf16(acc * scale[r])): the one rounding of the bf16 head); RP: row pairs per unit;
// DMA: the activation rows go to LDS by LDS-DMA
template <int TT, int MODE, int RP, bool DMA>
__global__ __launch_bounds__(256, (TT == 1 ? 4 : (TT <= 3 ? 3 : 2))) void gemv_w8_kernel(GemvW8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<WE4m3, TT, MODE, 2 * RP, DMA>(a.g, a.scale, smem, blockIdx.x, gridDim.x, 0);
}

// ---- rows of e4m3 + row scales -> bf16 rows: out[r, k] = bf16(scale[r] * e4m3(W[r, k])).  One 16-byte load and two 16-byte
// stores per lane; up to three matrices side by side (q | k | v, W1 | W3) in one launch.
__global__ __launch_bounds__(256) void dequant_w8_kernel(DequantW8Args a) {
  const int ppr = a.K >> 4;  // pieces per row
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.N * ppr) return;
  const int r = (int)(idx / ppr), pc = (int)(idx - (size_t)r * ppr);
  const uint8_t* src = GEMV_SEG_PICK(r, a.n0, a.n1, a.w[0] + (size_t)r * a.K, a.w[1] + (size_t)(r - a.n0) * a.K, a.w[2] + (size_t)(r - a.n1) * a.K);
  const float sc = GEMV_SEG_PICK(r, a.n0, a.n1, a.scale[0][r], a.scale[1][r - a.n0], a.scale[2][r - a.n1]);
  const u32x4 w = ld16_nt(src + pc * 16);
  u32x4 o[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x2_t lo, hi;
    cvt4_e4m3_f32(w[i], lo, hi);
    o[i >> 1][2 * (i & 1)] = pack_bf2(lo[0] * sc, lo[1] * sc);
    o[i >> 1][2 * (i & 1) + 1] = pack_bf2(hi[0] * sc, hi[1] * sc);
  }
  bf16_t* dst = a.out + (size_t)r * a.K + pc * 16;
  st16(dst, o[0]);
  st16(dst + 8, o[1]);
}

}  // namespace

hipError_t launch_dequant_w8(const DequantW8Args& a, hipStream_t s) {
  const size_t pieces = (size_t)a.N * (a.K >> 4);
  if (pieces == 0) return hipSuccess;
  hipLaunchKernelGGL(dequant_w8_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

namespace {
struct W8 {  // what launch_gemv_scaled (gemv_core.cuh) asks of a weight format
  template <int TT, int MODE, int RP, bool DMA>
  static constexpr auto kernel = gemv_w8_kernel<TT, MODE, RP, DMA>;
  static constexpr const char* kRpEnv = "MI_GEMV_W8_RP";
  // four-row units only where every wave of a full grid (2 blocks of 4 waves per CU) still gets two of them
  static int row_pairs(int npairs, int cus) { return npairs >= 2 * 2 * 8 * cus ? 2 : 1; }
};
}  // namespace
hipError_t launch_gemv_w8(const GemvW8Args& a, hipStream_t s) { return launch_gemv_scaled<W8>(a, s); }
