// W4A8 MFMA GEMM for prefills of MXFP4 models: out[M,N] = epilogue((sum_k e4m3(A_q[m, k]) * e2m1(C[n, k]) * 2^(S[n, k/32] - 127)) *
// s_x[m]), A_q [M, K] e4m3 bytes with one fp32 scale per row (act_quant_e4m3, elementwise.hip), C [N, K / 2] MXFP4 code bytes (two
// e2m1 codes per byte, the low nibble at the even k) and S [N, K / 32] e8m0 block scale bytes, both as the checkpoint stores them.
//
// Tile map, K loop, hazard argument, epilogue and launcher are gemm256_core.cuh's: 8 waves = 2 (M) x 4 (N), a 256 x 256 block
// tile (256 x 128 for SwiGLU, whose B halves are W1 and W3), a K tile of 128 elements, two stages, four phases per K tile.  This
// file's own are the operands.
// One `v_mfma_scale_f32_16x16x128_f8f6f4` per (row fragment, column fragment) with a FORMAT PER OPERAND: the weights are the
// instruction's first operand as e2m1 (cbsz = 4), the activations its second as e4m3 (blgp = 0).  A lane's FP4 operand is 32 codes
// of one weight row - exactly one MX block - and the instruction's per-lane scale byte of the first operand is an e8m0 - exactly
// the checkpoint's byte - so the hardware applies the block scales inside the contraction: no dequantisation, no epilogue work for
// the weights.  The activations' block scale is 127 (2^0); their per-row scale enters in the epilogue (gemm256_core ScaleRow).
//
// Halves.  A: 128 rows x 128 B = 16 KiB, as in the W8A8 kernel (gemm256_core a_half_src: two DMAs per wave).
// B: 128 rows x 64 B = 8 KiB: a row of a K tile is 4 slots of 16 bytes, one DMA fills 16 rows, wave w fills rows 16 w .. + 16 of
// either B half (one DMA per wave); lane l lands at (row 16 w + (l >> 2), slot l & 3) and fetches global slot (l & 3) ^ ((row >> 2)
// & 3) = (l & 3) ^ ((l >> 4) & 3).  A stage is A0 A1 B0 B1 and the scale strip (below): 50 KiB, the two stages 100 KiB.
// Fragments.  The two formats do NOT number k alike inside the instruction (found on the device with one-hot operands; the
// W8A8 kernel never sees it, both its operands being bytes): of an 8-bit operand lane l holds k = 16 (l >> 4) .. + 16 in its first
// four registers and k = 64 + 16 (l >> 4) .. + 16 in its last four; of an FP4 operand it holds k = 32 (l >> 4) .. + 32, in order,
// the low nibble first.  So A: lane l reads the 16-byte slots l >> 4 and 4 + (l >> 4) of row l & 15.  B: ONE 16-byte read, the
// 32 codes k = 32 (l >> 4) .. + 32 of column l & 15 = global slot l >> 4 of that row, which sits in LDS slot (l >> 4) ^ ((row >> 2)
// & 3); row = 32 wc + 16 j + (l & 15), so the XOR term is (l >> 2) & 3.  The 16 lanes of one l >> 4 then cover the 16 distinct
// 16-byte positions of 256 consecutive bytes (row & 3 picks the 64-byte row, the XOR the slot): no bank conflict in a read of 16
// lanes.  The codes go to the low four ints of the i32x8; the high four are not read by an FP4 operand.
// Block scales.  Lane (column n, fq = l >> 4) needs byte 4 t + fq of scale row n for K tile t, for each of its four column
// fragments (B half x j).  They come through a small DMA strip in LDS: the dword 4 t .. 4 t + 3 of each of the block's 256 weight
// rows (STORE / RESIDUAL: 256 columns; SwiGLU: 128 rows of W1, then 128 of W3), 1 KiB, staged by ONE 4-byte `global_load_lds` per
// wave - wave w fetches rows 64 (w & 3) .. + 64 into copy w >> 2 of the strip, so that the wr = 0 and the wr = 1 waves each read a
// copy of their own.  A lane reads its byte with `ds_read_u8` at (row dword + fq): it lands in bits 7:0 of the VGPR the MFMA
// names, op_sel = 0, no shift.  The strip lives in the stage of its tile (2 KiB behind B1); it needs the scale matrices 4-byte
// aligned (rows are K / 32 = 4 k bytes), which the launcher checks.
// The strip rides on A0 in the shared loop: stage(0, ..) issues A0's two DMAs and then the strip's one, read_a(0, ..) reads the
// four bytes behind A0's fragments - once per tile, in phase 1, and held - so the strip is re-staged in phase 2 with A0, the read
// segment after its last read, and the hazard argument covers it as a part of A0.  dmas() = {3, 2, 1, 1}: the loop's counted wait
// is vmcnt(3 + 1 + 1) = vmcnt(5), A0 A0 S B0 B1 of tile t + 2 in flight.  The prologue's DMAs of tile 0 go out as A0 S B0 B1 A1;
// their order is free, the prologue's wait counts totals (gemm256_core).
//
// Rows at or past M / N are clamped to the last valid one, codes and scales alike: nothing is read out of bounds, nothing is stored
// past a ragged edge.  Epilogues: GEMM_STORE (RoPE epilogue of q|k|v, up to three segments), GEMM_RESIDUAL, GEMM_SWIGLU with the
// bf16 kernel's rounding points and acc * s_x[m] in fp32 where it reads acc.  Scale bytes below 3 give bf16 subnormals in the
// weight-only route's image, which it may flush; here they are exact in fp32.  No LM head, no token-grouped form.
// The measured rates (profiles/EXPERIMENTS.md) are of the code as the compiler orders it (gemm256_core: where the MFMAs end up);
// pinning the MFMAs into their phases is untried.
#include "gemm256_core.cuh"

using E = Elem16<0>;  // outputs, residual and the RoPE / SwiGLU chains are bf16

namespace {
using namespace gemm256_core;

constexpr int BK = 128;                                  // elements of K per tile
constexpr int A_HALF = 128 * BK;                         // 16 KiB: 128 rows x 128 e4m3 bytes
constexpr int B_HALF = 128 * BK / 2;                     // 8 KiB: 128 rows x 64 code bytes
constexpr int S_COPY = 256 * 4;                          // 1 KiB: one dword of scale bytes per weight row of the block
constexpr int STAGE_BYTES = 2 * A_HALF + 2 * B_HALF + 2 * S_COPY;  // A0 A1 B0 B1 S S
constexpr int LDS_BYTES = 2 * STAGE_BYTES;               // 100 KiB
constexpr int B_BASE = 2 * A_HALF;                       // of B0 inside a stage
constexpr int S_BASE = B_BASE + 2 * B_HALF;              // of the scale strip's first copy

// code row r (K / 2 bytes) and scale row r (K / 32 bytes) of up to three matrices side by side
__device__ __forceinline__ const uint8_t* seg_codes(const GemmW4A8Args& a, int r) {
  const GemmArgs& g = a.g;
  const size_t ld = (size_t)(g.K >> 1);
  if (r < g.n0) return reinterpret_cast<const uint8_t*>(g.w0) + (size_t)r * ld;
  if (r < g.n1) return reinterpret_cast<const uint8_t*>(g.w1) + (size_t)(r - g.n0) * ld;
  return reinterpret_cast<const uint8_t*>(g.w2) + (size_t)(r - g.n1) * ld;
}
__device__ __forceinline__ const uint8_t* seg_scales(const GemmW4A8Args& a, int r) {
  const GemmArgs& g = a.g;
  const size_t ld = (size_t)(g.K >> 5);
  if (r < g.n0) return a.sw[0] + (size_t)r * ld;
  if (r < g.n1) return a.sw[1] + (size_t)(r - g.n0) * ld;
  return a.sw[2] + (size_t)(r - g.n1) * ld;
}
__device__ __forceinline__ i32x8 frag_b(const char* p) {
  const u32x4 c = *reinterpret_cast<const u32x4*>(p);
  return i32x8{(int)c[0], (int)c[1], (int)c[2], (int)c[3], 0, 0, 0, 0};
}

// The operands of gemm256_core::k_loop: e2m1 (format code 4) x e4m3 (0); the first operand's block scale is byte 0 of sc[][], the
// second's 2^(127 - 127)
struct Ops {
  static constexpr int dmas(int half) { return half == 0 ? 3 : half == 1 ? 2 : 1; }  // A0 + the scale strip, A1, B0, B1
  const char* srcA[2][2];  // [A half][piece]
  const uint8_t* srcB[2];  // [B half]
  const uint8_t* srcS;     // this lane's row of the scale strip
  char *pieceA, *pieceB, *pieceS;  // this wave's two 1-KiB pieces inside either A half, its piece inside either B half, of the strip
  const char* smem;
  int a_off, b_off, s_off, sw0, sw1;  // fragment addressing
  f32x4 acc[2][2][4][2];
  i32x8 af[4];     // [row fragment] of the A half in use
  i32x8 bf[2][2];  // [B half][column fragment]
  int sc[2][2];    // [B half][column fragment]: the e8m0 byte of this lane's block of the tile in use

  __device__ __forceinline__ void stage(int half, int kt, int st) {
    if (half < 2) {
      char* dst = pieceA + st * STAGE_BYTES + half * A_HALF;
      dma16(srcA[half][0] + (size_t)kt * BK, dst);
      dma16(srcA[half][1] + (size_t)kt * BK, dst + 1024);
      if (half == 0) dma4(srcS + (size_t)kt * 4, pieceS + st * STAGE_BYTES);
    } else {
      dma16(srcB[half - 2] + (size_t)kt * (BK / 2), pieceB + st * STAGE_BYTES + (half - 2) * B_HALF);
    }
  }
  __device__ __forceinline__ void read_a(int ha, int st) {
    const char* sb = smem + st * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = frag32(sb + ha * A_HALF + a_off + i * 2048, sw0, sw1);
    if (ha == 0) {
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int j = 0; j < 2; ++j) sc[hb][j] = *reinterpret_cast<const uint8_t*>(sb + s_off + hb * 512 + j * 64);
    }
  }
  __device__ __forceinline__ void read_b(int hb, int st) {
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[hb][j] = frag_b(smem + st * STAGE_BYTES + hb * B_HALF + b_off + j * 1024);
  }
  __device__ __forceinline__ void mfma_quad(int ha, int hb) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[ha][hb][i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[hb][j], af[i], acc[ha][hb][i][j], 4, 0, 0, sc[hb][j], 0, 127);
  }
};

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_w4a8_kernel(GemmW4A8Args args) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& g = args.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  int m_tile, n_tile;
  if (!tile_of_block((g.M + 255) >> 8, col_tiles(g.N, EPI), m_tile, n_tile)) return;
  const int row0 = m_tile * 256, rows_valid = min(256, g.M - row0);

  Ops op;
  // ---- DMA sources (header).  Rows at or past M / N are clamped to the last valid one.
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) op.srcA[h][j] = a_half_src<uint8_t, false>(g, row0, rows_valid, h, wid, j, lane);
  {
    const int bslot = (lane & 3) ^ ((lane >> 4) & 3);
    const int r = wid * 16 + (lane >> 2);
    const size_t ldw = (size_t)(g.K >> 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (EPI == GEMM_SWIGLU) {
        const int n = min(n_tile * 128 + r, g.N - 1);
        op.srcB[h] = reinterpret_cast<const uint8_t*>(h == 0 ? g.w0 : g.w1) + (size_t)n * ldw + bslot * 16;
      } else {
        const int n = min(n_tile * 256 + h * 128 + r, g.N - 1);
        op.srcB[h] = seg_codes(args, n) + bslot * 16;
      }
    }
  }
  {
    const int b = (wid & 3) * 64 + lane;  // weight row of the block
    if (EPI == GEMM_SWIGLU) {
      const int n = min(n_tile * 128 + (b & 127), g.N - 1);
      op.srcS = args.sw[b >> 7] + (size_t)n * (size_t)(g.K >> 5);
    } else {
      op.srcS = seg_scales(args, min(n_tile * 256 + b, g.N - 1));
    }
  }
  op.pieceA = smem + wid * 2048;
  op.pieceB = smem + B_BASE + wid * 1024;
  op.pieceS = smem + S_BASE + (wid >> 2) * S_COPY + (wid & 3) * 256;
  op.smem = smem;
  // ---- fragment addressing (header)
  const int fq = lane >> 4;
  op.sw0 = (fq ^ (lane & 7)) << 4;  // A: k = 16 fq .. + 16 and 64 + 16 fq .. + 16
  op.sw1 = ((4 + fq) ^ (lane & 7)) << 4;
  op.a_off = (wr * 64 + (lane & 15)) * 128;
  op.b_off = B_BASE + (wc * 32 + (lane & 15)) * 64 + ((fq ^ ((lane >> 2) & 3)) << 4);
  op.s_off = S_BASE + wr * S_COPY + (wc * 32 + (lane & 15)) * 4 + fq;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) op.acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  k_loop<true>(op, g.K / BK, wr);
  epilogue16<E, EPI, 2>(g, op.acc, ScaleRow{args.sx}, row0, rows_valid, n_tile, wr, wc, lane);
}

}  // namespace

// (the W8A8 predicate: the activation quantiser in front of either GEMM is the same, and a K tile is 128 elements in both)
bool gemm256_w4a8_applicable(int M, int K) { return gemm256_w8a8_applicable(M, K); }

hipError_t launch_gemm256_w4a8(const GemmW4A8Args& a, hipStream_t s) {
  const GemmArgs& g = a.g;
  if (!a8_args_ok(a)) return hipErrorInvalidValue;
  // the scale strip's DMA fetches 4 aligned bytes: the scale rows are K / 32 = 4 k bytes apart, so their bases decide
  if ((reinterpret_cast<size_t>(a.sw[0]) | reinterpret_cast<size_t>(a.sw[1]) | reinterpret_cast<size_t>(a.sw[2])) & 3) return hipErrorInvalidValue;
  const dim3 grid = tile_grid((g.M + 255) >> 8, col_tiles(g.N, g.epi));
  switch (g.epi) {
    case GEMM_STORE: return launch_one<&gemm256_w4a8_kernel<GEMM_STORE>, LDS_BYTES>(a, grid, s);
    case GEMM_RESIDUAL: return launch_one<&gemm256_w4a8_kernel<GEMM_RESIDUAL>, LDS_BYTES>(a, grid, s);
    case GEMM_SWIGLU: return launch_one<&gemm256_w4a8_kernel<GEMM_SWIGLU>, LDS_BYTES>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}
