// Weight-streaming GEMV launches for M <= 8 tokens whose weight rows are OCP MXFP4 (e2m1 codes in blocks of 32 along K, one e8m0
// scale byte per block: weight-only, 4.25 bits per weight), and the dequantisation pass of the prefill route.
//
// The kernels are gemv_core::gemv_body on the WMxfp4 format (gemv_core.cuh: design notes, conversion, the scale-byte loads of a
// batch and the counted wait that includes them); the activation staging is the bf16 kernels', so the normalised rows in LDS are
// bit-identical to theirs.  Every weight 2^(b - 127) * e2m1(code) is exact in bf16: a kernel here computes what the bf16 kernel
// computes on the dequantised weights, up to fp32 summation order.
//
// A row is a quarter of the bytes of a bf16 row, so the fixed cost of a unit (wave reductions, epilogue, loop bookkeeping) weighs
// four times as much.  Units are RP row pairs at one token (gemv_w4_row_pairs: the rule; MI_GEMV_W4_RP: its A/B switch), one pair
// above.
#include <cstdlib>

#include "common.cuh"
#include "gemv_core.cuh"

namespace {

using namespace gemv_core;

// TT: token rows staged in LDS; MODE: GEMV_STORE / GEMV_RESIDUAL / GEMV_SWIGLU / GEMV_QKV_ROPE, and GEMV_LOGITS for a quantised LM
// head (logit = float(bf16(acc)): the one rounding of the bf16 head); RP: row pairs per unit;
// DMA: the activation rows go to LDS by LDS-DMA.  Two batches are 64 piece + 16 scale registers, and a unit's converted pairs come
// on top: at the bf16 kernels' 4 blocks per CU (128 VGPRs) every one-token kernel spilled.  The grid is 2 blocks per CU
// (max_blocks), so 3 (168 VGPRs) costs no occupancy that is used.
template <int TT, int MODE, int RP, bool DMA>
__global__ __launch_bounds__(256, (TT <= 3 ? 3 : 2)) void gemv_w4_kernel(GemvW4Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<WMxfp4, TT, MODE, 2 * RP, DMA>(a.g, a.scale, smem, blockIdx.x, gridDim.x, 0);
}

// ---- rows of MXFP4 -> bf16 rows: out[r, k] = 2^(scale[r, k / 32] - 127) * e2m1(code[r, k]), exact.  One 16-byte load, one scale
// byte and four 16-byte stores per lane; up to three matrices side by side (q | k | v, W1 | W3) in one launch.
__global__ __launch_bounds__(256) void dequant_w4_kernel(DequantW4Args a) {
  const int ppr = a.K >> 5;  // pieces (= scale blocks) per row
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.N * ppr) return;
  const int r = (int)(idx / ppr), pc = (int)(idx - (size_t)r * ppr);
  const int rs = GEMV_SEG_PICK(r, a.n0, a.n1, r, r - a.n0, r - a.n1);  // the row inside its own matrix
  const uint8_t* wm = GEMV_SEG_PICK(r, a.n0, a.n1, a.w[0], a.w[1], a.w[2]);
  const uint8_t* sm = GEMV_SEG_PICK(r, a.n0, a.n1, a.scale[0], a.scale[1], a.scale[2]);
  const u32x4 w = ld16_nt(wm + ((size_t)rs * ppr + pc) * 16);
  const float sc = __uint_as_float((uint32_t)sm[(size_t)rs * ppr + pc] << 23);
  bf16_t* dst = a.out + (size_t)r * a.K + pc * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32x4 o;
    o[0] = cvt2_e2m1<0>(w[i], sc);
    o[1] = cvt2_e2m1<1>(w[i], sc);
    o[2] = cvt2_e2m1<2>(w[i], sc);
    o[3] = cvt2_e2m1<3>(w[i], sc);
    st16(dst + 8 * i, o);
  }
}

}  // namespace

hipError_t launch_dequant_w4(const DequantW4Args& a, hipStream_t s) {
  const size_t pieces = (size_t)a.N * (a.K >> 5);
  if (pieces == 0) return hipSuccess;
  hipLaunchKernelGGL(dequant_w4_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// row pairs per unit at one token: four-row units from 8 row pairs per CU on - every linear of the 7B dims, where forcing them
// everywhere measured 1753 us per step against 1801 (two-row units), 1777 (four rows for W1|W3 only, the e4m3 kernels' rule) and
// 1966 (eight-row units, which are not built); below that, where nothing was measured, a wave keeps the two-row unit (profiles/EXPERIMENTS.md)
int gemv_w4_row_pairs(int npairs, int cus) { return npairs >= 8 * cus ? 2 : 1; }

namespace {
struct W4 {  // what launch_gemv_scaled (gemv_core.cuh) asks of a weight format
  template <int TT, int MODE, int RP, bool DMA>
  static constexpr auto kernel = gemv_w4_kernel<TT, MODE, RP, DMA>;
  static constexpr const char* kRpEnv = "MI_GEMV_W4_RP";
  static int row_pairs(int npairs, int cus) { return gemv_w4_row_pairs(npairs, cus); }
};
}  // namespace
hipError_t launch_gemv_w4(const GemvW4Args& a, hipStream_t s) { return launch_gemv_scaled<W4>(a, s); }
