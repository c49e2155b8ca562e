// Token-grouped W8A8 MFMA GEMM for prefills of MoE models with FP8 (e4m3) experts: ONE launch covers every expert, and the
// expert bytes meet e4m3 activation bytes on the block-scaled FP8 MFMA as they are - no bf16 image of any expert exists.
//
//   SWIGLU  hid[r, f] = swiglu((sum_k xq[tok(r), k] w1q[e][f, k]) * (s_x[tok(r)] * s1[e][f]),  the same with w3q, s3)
//   STORE   y[r, d]   = bf16((sum_f hq[r, f] w2q[e][d, f]) * (s_h[r] * s2[e][d]))
//
// r: a compact row, i.e. a (token, slot) pair in the order launch_moe_lists sorts them by expert; e: the expert of r's tile.
//
// What is gemm256_core.cuh's: the block -> tile map, the DMA sources of an A half, the four-phase K loop with its stagger and
// hazard argument, the 16-bit-output epilogue, the launcher, and the e4m3 x e4m3 operand policy that gemm256_w8a8.hip uses too
// (OpsE4m3: 16-KiB half tiles of 128 rows x 128 e4m3 bytes, two stages of A0 A1 B0 B1 (128 KiB), one
// `v_mfma_scale_f32_16x16x128_f8f6f4` per (row fragment, column fragment) and K tile with both block scales at 2^0, issued
// W-fragment x A-fragment).  This file's own:
//   * the tile table.  The grid is sized on the host for max_m_tiles; block tile m_tile reads {expert, first compact row, valid
//     rows <= 256} from tile_tab and leaves at m_tile >= *n_tiles_ptr - the table is built on the device, the host never learns
//     how many tiles the routing made.  The expert's byte and scale pointers are four uniform loads from the two device tables
//     [E][3]; everything behind them is the plain kernel's addressing with per-block bases.
//   * the gathered A operand.  The W1|W3 launch reads activation row tok_of[r] for compact row r: x [T, D] is quantised once per
//     TOKEN (T rows, T scales), not once per (token, slot), and the DMA source address carries the gather - a token's 128-byte
//     K slices are fetched straight into the tile of each expert that it was routed to.  The W2 launch reads compact rows.
//     Rows past a tile's valid count are clamped to its last valid one (in bounds, never stored).
//   * the scale policy (gemm256_core ScaleMoe): the activation scale is read through the same gather as the row, the weight scale
//     from the tile's expert; their product is formed first, then meets the fp32 sum, as in ScaleRowCol.
// Tiles are always 256 rows: a tile of an expert with few rows runs the full K loop on clamped rows (a half-height tile for
// sparse experts is the next step, README).
#include "gemm256_core.cuh"

using E = Elem16<0>;  // hid, y and the SwiGLU chain are bf16

namespace {
using namespace gemm256_core;

using Ops = OpsE4m3;  // the e4m3 x e4m3 operand policy (gemm256_core.cuh)
constexpr int BK = Ops::BK, LDS_BYTES = Ops::LDS_BYTES;

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_moe_w8a8_kernel(GemmMoeW8A8Args args) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& g = args.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  // ---- block -> tile -> {expert, rows}: the grid covers max_m_tiles, the device table says how many of them exist
  int m_tile, n_tile;
  if (!tile_of_block(g.max_m_tiles, col_tiles(g.N, EPI), m_tile, n_tile)) return;
  if (m_tile >= *g.n_tiles_ptr) return;
  const int e = g.tile_tab[m_tile * 4];
  const int row0 = g.tile_tab[m_tile * 4 + 1], rows_valid = g.tile_tab[m_tile * 4 + 2];
  const char* wb[2];
  ScaleMoe sc;
  sc.sx = args.sx;
  sc.sx_gather = EPI == GEMM_SWIGLU ? g.a_gather : nullptr;
  wb[0] = reinterpret_cast<const char*>(g.expert_tab[e * 3 + g.w_sel0]);
  sc.sw[0] = args.scale_tab[e * 3 + g.w_sel0];
  if (EPI == GEMM_SWIGLU) {
    wb[1] = reinterpret_cast<const char*>(g.expert_tab[e * 3 + g.w_sel1]);
    sc.sw[1] = args.scale_tab[e * 3 + g.w_sel1];
  } else {
    wb[1] = wb[0];
    sc.sw[1] = sc.sw[0];
  }

  Ops op;
  // ---- DMA sources.  A: compact row -> (W1|W3 launch) token row; B: rows of the tile's expert.  Rows at or past the tile's
  // valid rows / N are clamped to the last valid one.
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      op.src[h][j] = a_half_src<uint8_t, EPI == GEMM_SWIGLU>(g, row0, rows_valid, h, wid, j, lane);
      const int r = piece_row(wid, j, lane);
      const int n = EPI == GEMM_SWIGLU ? min(n_tile * 128 + r, g.N - 1) : min(n_tile * 256 + h * 128 + r, g.N - 1);
      op.src[2 + h][j] = wb[EPI == GEMM_SWIGLU ? h : 0] + (size_t)n * g.K + src_slot_bytes(lane);
    }
  op.init(smem, wid, wr, wc, lane);

  k_loop<true>(op, g.K / BK, wr);
  epilogue16<E, EPI, 2>(g, op.acc, sc, row0, rows_valid, n_tile, wr, wc, lane);
}

}  // namespace

// (D, F <= 16384: the activation quantiser in front of either launch holds a row in registers, elementwise.hip)
bool gemm256_moe_w8a8_applicable(int T, int D, int F) {
  return T >= 256 && D >= BK && F >= BK && D % BK == 0 && F % BK == 0 && D <= 16384 && F <= 16384;
}

hipError_t launch_gemm256_moe_w8a8(const GemmMoeW8A8Args& a, hipStream_t s) {
  const GemmArgs& g = a.g;
  if (!g.tile_tab || !g.n_tiles_ptr || g.tile_rows != 256 || g.max_m_tiles <= 0 || !g.expert_tab || !a.scale_tab || !a.sx || !g.a ||
      !g.out || g.N <= 0 || g.K < BK || g.K % BK || g.lda < g.K || (g.lda & 15) || (reinterpret_cast<size_t>(g.a) & 15) ||
      g.w_sel0 < 0 || g.w_sel0 > 2 || g.rope_cs)
    return hipErrorInvalidValue;
  const dim3 grid = tile_grid(g.max_m_tiles, col_tiles(g.N, g.epi));
  switch (g.epi) {
    case GEMM_STORE:
      if (g.a_gather) return hipErrorInvalidValue;  // (the W2 launch reads compact rows)
      return launch_one<&gemm256_moe_w8a8_kernel<GEMM_STORE>, LDS_BYTES>(a, grid, s);
    case GEMM_SWIGLU:
      if (g.w_sel1 < 0 || g.w_sel1 > 2) return hipErrorInvalidValue;
      return launch_one<&gemm256_moe_w8a8_kernel<GEMM_SWIGLU>, LDS_BYTES>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}
