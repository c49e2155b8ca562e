// bf16 MFMA GEMM, 256x256x64 block tile, for the large prefill shapes: out[M,N] = epilogue(A[M,K] . W[N,K]^T).
//
// Same contract and epilogues as gemm.hip (transformer_layers.py:66,93,105-106; transformer.py:235); launch_gemm
// picks this kernel when M >= 256 and K % 64 == 0, and for the token-grouped MoE form (moe.py:28-32, one launch for all
// experts) when its tile table was built with 256-row m-tiles.
//
// Epilogues: store / residual add / SiLU*mul / fp32 logits as in gemm.hip, plus GEMM_LOGPROB (the LM head reduced to
// log-softmax pieces without storing logits, generate.py:101-118).
//
// Why a second tile shape: the 128x128 kernel moves 32 KiB of operands through LDS per 128x128x64 MACs and is bound by
// LDS bandwidth (DMA writes ~64-85 B/clk + fragment reads 256 B/clk against 16 clk per MFMA): ~37 % of the MFMA peak.
// 256x256 halves the LDS bytes per flop.  The structure - wave layout, tile map, the four-phase K loop with its hazard
// argument, the 16-bit-output epilogue - is gemm256_core.cuh's, shared with the two FP8-activation kernels.  This file's own:
//   * the operands: 16-bit elements, K tile of 64, two MFMA 16x16x32 (k steps) per (row fragment, column fragment), 16 per
//     quadrant and K tile; lane l holds row l & 15, k = (l >> 4) * 8 .. + 8 of each 32-wide k step;
//   * the LDS image: 2 stages x {A0, A1, B0, B1} x 16 KiB half tiles (128 rows x 128 B, 16-byte slot XOR-swizzled by row & 7 on
//     the DMA's SOURCE address), 2 `global_load_lds_dwordx4` per wave and half: the loop's counted wait is vmcnt(6);
//   * the token-grouped MoE form, the half-height tile with its own loop (MH = 1, below), the LOGITS / LOGPROB epilogues, and
//     the build-time experiment switches.
#include <cstdlib>

#include "gemm256_core.cuh"

// A second compile of this file with -DG256_F16=1 (build_native.py: gemm256_f16.o) is the SAME kernel for fp16 storage - the
// data movement of two 16-bit types is identical; what changes is the element E (common.cuh): the MFMA opcode and the
// conversions / rounding points of the epilogues.  That compile exports launch_gemm256_f16 and nothing else (generic.hip:
// prefills of fp16 models); the default compile's code objects are checked against their ISA hash like the decode engine's.
#ifndef G256_F16
#define G256_F16 0
#endif
using E = Elem16<G256_F16>;

// Build-time experiment switches (all off in the shipped build; the experimental main loops live OUTSIDE the product tree, in scripts/probes/gemm256_experiments.inc):
#ifndef G256_PRIO
#define G256_PRIO 0
#endif
#ifndef G256_BAL
#define G256_BAL 0
#endif
#ifndef G256_DMA_AFTER
#define G256_DMA_AFTER 1   // 1 (shipped): a read segment issues its fragment reads before its half-tile DMA
#endif
#ifndef G256_SPLIT
#define G256_SPLIT 0
#endif
#ifndef G256_PIPE
#define G256_PIPE 0
#endif
#ifndef G256_ABL
#define G256_ABL 0
#endif
#ifndef G256_CLK
#define G256_CLK 0         // 1: block 0 records shader-clock and 100 MHz ticks across its main loop (mi_debug_gemm_clock)
#endif

#if G256_CLK
__device__ unsigned long long g256_clk[2];
extern "C" int mi_debug_gemm_clock(unsigned long long* out2) {
  return (int)hipMemcpyFromSymbol(out2, HIP_SYMBOL(g256_clk), sizeof(g256_clk));
}
#endif

namespace {
using namespace gemm256_core;

constexpr int BK = 64;
constexpr int HALF_BYTES = 128 * BK * 2;     // 16 KiB: 128 rows x 128 B
constexpr int STAGE_BYTES = 4 * HALF_BYTES;  // A0 A1 B0 B1
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 128 KiB
// Half-height form (MH = 1, round 4): a 128 x 256 output tile = ONE A half against both B halves, two phases per K tile,
// three stages of {A0, B0, B1} (144 KiB).  It exists for the LAST, partly filled round of a launch: 384 tiles of
// 256 x 256 (q|k|v of Mistral-7B at 4096 tokens) are 1.5 rounds of 256 CUs; the columns of the half round used to go
// to the 128 x 128 kernel (twice the LDS bytes per flop: 0.72 PF); as 128 x 256 tiles they are exactly one full round
// at 1.5x the LDS bytes per flop of the square tile.  Same MFMA shape, same k order: bit-identical outputs.
constexpr int STAGE_BYTES_H = 3 * HALF_BYTES;
constexpr int LDS_BYTES_H = 3 * STAGE_BYTES_H;  // 144 KiB

// The operands of gemm256_core::k_loop (MH = 2) and of the half-height loop below (MH = 1, whose stage is A0 B0 B1: half
// indices 0, 1, 2).  SWAP: MFMAs issued W-fragment x A-fragment (transposed 16x16 result tiles, see the shared epilogue).
template <int MH, bool SWAP>
struct Ops {
  static constexpr int STG = (MH + 2) * HALF_BYTES;  // bytes per stage: the A halves, B0, B1
  static constexpr int dmas(int) { return 2; }
  const char* src[MH + 2][2];  // [half][piece]
  char* my_piece;              // this wave's two 1-KiB pieces inside any half tile of stage 0
  const char* smem;
  int a_off, b_off, sw0, sw1;  // fragment addressing
  f32x4 acc[MH][2][4][2];
  typename E::x8 af[2][4];     // [k step][row fragment] of the A half in use
  typename E::x8 bf[2][2][2];  // [B half][k step][column fragment]

  static __device__ __forceinline__ typename E::x8 frag(const char* p) { return __builtin_bit_cast(typename E::x8, *reinterpret_cast<const u32x4*>(p)); }
  __device__ __forceinline__ void stage(int half, int kt, int st) {
    char* dst = my_piece + st * STG + half * HALF_BYTES;
    dma16(src[half][0] + (size_t)kt * (BK * 2), dst);
    dma16(src[half][1] + (size_t)kt * (BK * 2), dst + 1024);
  }
  __device__ __forceinline__ void read_a(int ha, int st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[0][i] = frag(smem + st * STG + ha * HALF_BYTES + a_off + i * 2048 + sw0);
      af[1][i] = frag(smem + st * STG + ha * HALF_BYTES + a_off + i * 2048 + sw1);
    }
  }
  __device__ __forceinline__ void read_b(int hb, int st) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf[hb][0][j] = frag(smem + st * STG + hb * HALF_BYTES + b_off + j * 2048 + sw0);
      bf[hb][1][j] = frag(smem + st * STG + hb * HALF_BYTES + b_off + j * 2048 + sw1);
    }
  }
  __device__ __forceinline__ void mfma_quad(int ha, int hb) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[ha][hb][i][j] = SWAP ? E::mfma16(bf[hb][ks][j], af[ks][i], acc[ha][hb][i][j]) : E::mfma16(af[ks][i], bf[hb][ks][j], acc[ha][hb][i][j]);
  }
};

template <int EPI, bool STAGGER, int MH = 2>
__global__ __launch_bounds__(512, 1) void gemm256_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MROWS = MH * 128;  // output rows per block
  static_assert(MH == 2 || (EPI == GEMM_STORE || EPI == GEMM_RESIDUAL), "half-height tiles: store / residual epilogues");
  // bf16 outputs: MFMAs issued as W-fragment x A-fragment (transposed 16x16 result tiles, see the epilogue); fp32
  // logits: A x W, whose 4-byte stores already cover 64-byte row segments and measured faster than 16-byte ones.
  constexpr bool kSwap = EPI != GEMM_LOGITS && EPI != GEMM_LOGPROB;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
#if G256_CLK
  const unsigned long long clk_c0 = __builtin_readcyclecounter(), clk_r0 = __builtin_amdgcn_s_memrealtime();
#endif

  // ---- block -> tile (gemm256_core)
  const bool grouped = g.tile_tab != nullptr;  // token-grouped MoE form: m-tiles come from the device tile table
  const int n_tiles = col_tiles(g.N, EPI);
  int m_tile, n_tile;
  if (!tile_of_block(grouped ? g.max_m_tiles : (g.M + MROWS - 1) / MROWS, n_tiles, m_tile, n_tile)) return;
  int row0, rows_valid;
  const bf16_t *w0 = g.w0, *w1 = g.w1;
  if (grouped) {  // one tile of one expert: {expert, first compact row, valid rows (<= 256)}
    if (m_tile >= *g.n_tiles_ptr) return;
    const int e = g.tile_tab[m_tile * 4];
    row0 = g.tile_tab[m_tile * 4 + 1];
    rows_valid = g.tile_tab[m_tile * 4 + 2];
    w0 = reinterpret_cast<const bf16_t*>(g.expert_tab[e * 3 + g.w_sel0]);
    if (g.w_sel1 >= 0) w1 = reinterpret_cast<const bf16_t*>(g.expert_tab[e * 3 + g.w_sel1]);
  } else {
    row0 = m_tile * MROWS;
    rows_valid = min(MROWS, g.M - row0);
  }

  // ---- DMA sources (gemm256_core: both operands are 16-KiB halves).  Rows at or past the tile's valid rows / N are clamped.
  Ops<MH, kSwap> op;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (h < MH) op.src[h][j] = a_half_src<bf16_t, true>(g, row0, rows_valid, h, wid, j, lane);
      const int r = piece_row(wid, j, lane);
      const bf16_t* w;
      if (EPI == GEMM_SWIGLU) {
        const int n = min(n_tile * 128 + r, g.N - 1);
        w = (h == 0 ? w0 : w1) + (size_t)n * g.K;
      } else {
        const int n = min(n_tile * 256 + h * 128 + r, g.N - 1);
        w = grouped ? w0 + (size_t)n * g.K : seg_row(g, n);
      }
      op.src[MH + h][j] = reinterpret_cast<const char*>(w) + src_slot_bytes(lane);
    }
  op.my_piece = smem + wid * 2048;
  op.smem = smem;
  // ---- fragment addressing (MFMA 16x16x32: lane holds row lane & 15, k = (lane >> 4) * 8 .. + 8 of each 32-wide k step)
  const int fq = lane >> 4;
  op.sw0 = ((fq) ^ (lane & 7)) << 4;
  op.sw1 = ((4 + fq) ^ (lane & 7)) << 4;
  op.a_off = (wr * 64 + (lane & 15)) * 128;
  op.b_off = MH * HALF_BYTES + (wc * 32 + (lane & 15)) * 128;
  f32x4 (&acc)[MH][2][4][2] = op.acc;
#pragma unroll
  for (int a = 0; a < MH; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#if G256_PIPE || G256_BAL || G256_SPLIT || G256_ABL || G256_PRIO || !G256_DMA_AFTER
#include "../../scripts/probes/gemm256_experiments.inc"  // probe builds only (scripts/build_variants.py gemm): never part of the shipped library
#else
  const int nk = g.K / BK;
  if constexpr (MH == 1) {
    // ---- half-height tile: stage = {A0, B0, B1} (half indices 0, 1, 2), three stages, tile t in stage t % 3, two phases per K
    // tile with gemm256_core's segments and stagger.  Tile t + 2 is staged during tile t into the stage tile t - 1 was read from
    // (its last reads - by the group that runs one barrier behind - ended with the barrier before this tile's first read
    // segment), and is waited for one tile later (vmcnt(6): everything but the six pieces issued since), two barriers before its
    // first read.
    op.stage(0, 0, 0);
    op.stage(1, 0, 0);
    op.stage(2, 0, 0);
    if (nk > 1) {
      op.stage(0, 1, 1);
      op.stage(1, 1, 1);
      op.stage(2, 1, 1);
      wait_vm<6>();
    } else {
      wait_vm<0>();
    }
    raw_barrier();
    if (STAGGER && wr == 1) raw_barrier();
    int s = 0, s2 = 2;  // stage of tile t, of tile t + 2
    for (int t = 0; t < nk; ++t) {
      const bool more1 = t + 1 < nk, more2 = t + 2 < nk;
      // phase 1: quadrant (0, 0)
      op.read_b(0, s);
      op.read_a(0, s);
      if (more2) op.stage(0, t + 2, s2);
      segment_end();
      op.mfma_quad(0, 0);
      mfma_end<STAGGER>();
      // phase 2: quadrant (0, 1); retire tile t + 1
      op.read_b(1, s);
      if (more2) {
        op.stage(1, t + 2, s2);
        op.stage(2, t + 2, s2);
        wait_vm<6>();
      } else if (more1) {
        wait_vm<0>();
      }
      segment_end();
      op.mfma_quad(0, 1);
      mfma_end<STAGGER>();
      s = (s == 2) ? 0 : s + 1;
      s2 = (s2 == 2) ? 0 : s2 + 1;
    }
    if (STAGGER && wr == 0) raw_barrier();
  } else {
    k_loop<STAGGER>(op, nk, wr);
  }
#if G256_CLK
  if (blockIdx.x == 0 && tid == 0) {
    g256_clk[0] = __builtin_readcyclecounter() - clk_c0;
    g256_clk[1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
  }
#endif
#endif  // experiments

  if constexpr (EPI == GEMM_LOGPROB) {
    // Log-softmax pieces of this tile, nothing stored (transformer.py:235-242 + generate.py:101-118: the LM head's
    // bf16-rounded logits are only ever reduced to log-probabilities of given tokens).  A row's 256 columns live in the
    // four wc waves: 4 values per lane x 16 lanes per wave.  Per wave: lane-local then DPP row reductions; the four
    // waves meet in LDS (free again: every fragment read was waited for before the loop's last barrier).
    __syncthreads();
    float2* part = reinterpret_cast<float2*>(smem);  // [256 rows][4 waves]
#pragma unroll
    for (int ha = 0; ha < MH; ++ha)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = ha * 128 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
          const int row = min(row0 + rl, g.M - 1);
          float v[2][2], mx = -INFINITY;
#pragma unroll
          for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int n = n_tile * 256 + hb * 128 + wc * 32 + j * 16 + (lane & 15);
              v[hb][j] = (n < g.N) ? E::round(acc[ha][hb][i][j][r]) : -INFINITY;
              mx = fmaxf(mx, v[hb][j]);
              if (n + g.lp_col0 == g.lp_target[row] && row0 + rl < g.M) g.lp_tgt[row] = v[hb][j];
            }
          mx = row16_max(mx);
          float sm = 0.f;
#pragma unroll
          for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int j = 0; j < 2; ++j) sm += (v[hb][j] == -INFINITY) ? 0.f : __expf(v[hb][j] - mx);
          sm = row16_sum(sm);
          if ((lane & 15) == 0) part[rl * 4 + wc] = make_float2(mx, sm);
        }
    __syncthreads();
    if (tid < 256 && row0 + tid < g.M) {
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, part[tid * 4 + w].x);
      float S = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) S += (part[tid * 4 + w].x == -INFINITY) ? 0.f : part[tid * 4 + w].y * __expf(part[tid * 4 + w].x - M);
      g.lp_partial[(size_t)(row0 + tid) * (g.lp_tiles ? g.lp_tiles : n_tiles) + (g.lp_col0 >> 8) + n_tile] = make_float2(M, S);
    }
    return;
  }
  if constexpr (!kSwap) {
    // acc[ha][hb][i][j][r]: tile row ha*128 + wr*64 + i*16 + (lane>>4)*4 + r, tile column hb*128 + wc*32 + j*16 + (lane & 15)
#pragma unroll
    for (int ha = 0; ha < MH; ++ha)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = ha * 128 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
          if (rl >= rows_valid) continue;
          const int row = row0 + rl;
          float* o = reinterpret_cast<float*>(g.out) + (size_t)row * g.ldo;
#pragma unroll
          for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int n = n_tile * 256 + hb * 128 + wc * 32 + j * 16 + (lane & 15);
              if (n < g.N) o[n] = E::round(acc[ha][hb][i][j][r]);
            }
        }
    return;
  }
  if constexpr (kSwap) epilogue16<E, EPI, MH>(g, acc, ScaleNone{}, row0, rows_valid, n_tile, wr, wc, lane);  // STORE / RESIDUAL / SWIGLU
}

template <int EPI, int MH = 2>
hipError_t launch_staggered(const GemmArgs& g, dim3 grid, hipStream_t s) {
  constexpr int lds = MH == 2 ? LDS_BYTES : LDS_BYTES_H;
  static int stagger = -1;  // MI_GEMM_STAGGER=0: both wave groups in lockstep (A/B testing)
  if (stagger < 0) {
    const char* e = getenv("MI_GEMM_STAGGER");
    stagger = e ? atoi(e) : 1;
  }
  return stagger ? launch_one<&gemm256_kernel<EPI, true, MH>, lds>(g, grid, s) : launch_one<&gemm256_kernel<EPI, false, MH>, lds>(g, grid, s);
}

}  // namespace

#if !G256_F16  // (host predicates and the half-height launcher do not depend on the element: the default compile has them)
bool gemm256_applicable(const GemmArgs& g) {
  if (g.K % BK != 0 || g.K < 2 * BK) return false;
  if (g.tile_tab != nullptr) return g.tile_rows == 256;  // token-grouped form: the tile table decides
  return g.a_gather == nullptr && g.M >= 256;
}

// 128 x 256 tiles (MH = 1) for the columns of a launch's partly filled last round: plain (not token-grouped) store /
// residual problems only.
bool gemm256_half_applicable(const GemmArgs& g) {
  return gemm256_applicable(g) && g.tile_tab == nullptr && (g.epi == GEMM_STORE || g.epi == GEMM_RESIDUAL);
}

hipError_t launch_gemm256_half(const GemmArgs& g, hipStream_t s) {
  const dim3 grid = tile_grid((g.M + 127) >> 7, col_tiles(g.N, g.epi));
  switch (g.epi) {
    case GEMM_STORE: return launch_staggered<GEMM_STORE, 1>(g, grid, s);
    case GEMM_RESIDUAL: return launch_staggered<GEMM_RESIDUAL, 1>(g, grid, s);
    default: return hipErrorInvalidValue;
  }
}
#endif

#if G256_F16
hipError_t launch_gemm256_f16(const GemmArgs& g, hipStream_t s) {
#else
hipError_t launch_gemm256(const GemmArgs& g, hipStream_t s) {
#endif
  const dim3 grid = tile_grid(g.tile_tab ? g.max_m_tiles : (g.M + 255) >> 8, col_tiles(g.N, g.epi));
  switch (g.epi) {
    case GEMM_STORE: return launch_staggered<GEMM_STORE>(g, grid, s);
    case GEMM_RESIDUAL: return launch_staggered<GEMM_RESIDUAL>(g, grid, s);
    case GEMM_SWIGLU: return launch_staggered<GEMM_SWIGLU>(g, grid, s);
    case GEMM_LOGITS: return launch_staggered<GEMM_LOGITS>(g, grid, s);
    case GEMM_LOGPROB: return launch_staggered<GEMM_LOGPROB>(g, grid, s);
    default: return hipErrorInvalidValue;
  }
}
