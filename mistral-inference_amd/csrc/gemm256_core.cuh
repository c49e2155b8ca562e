// Core of the 256-tile prefill GEMMs: what gemm256.hip (bf16, and fp16 in its -DG256_F16=1 compile), gemm256_w8a8.hip (e4m3 x
// e4m3) and gemm256_w4a8.hip (MXFP4 x e4m3) have in common, each once - the DMA / wait / barrier primitives, the block -> tile map
// with its host mirror, the A half's DMA sources, the four-phase K loop with its hazard argument, the 16-bit-output epilogue and
// the launcher's pieces.  A kernel supplies its operands as a struct (below, "operand policy") and its output scales as another
// ("scale policy"); its own file says only what is its own: operand formats, LDS image, fragment k-numbering.
//
// Common structure (cdna_hip_programming.md section 5, "256^2 8-phase template", written from its description): 8 waves = 2 (M,
// wr) x 4 (N, wc); a wave owns 64 rows of each 128-row A half and 32 columns of each 128-column B half, i.e. four 64 x 32
// quadrants (ha, hb).  LDS holds two stages of {A0, A1, B0, B1} half tiles, filled by `global_load_lds` and never through
// registers.  Half indices of a stage, everywhere below: 0 = A0, 1 = A1, 2 = B0, 3 = B1.
#pragma once
#include "common.cuh"
#include "kernels.h"

namespace gemm256_core {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------- primitives
__device__ __forceinline__ void dma16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_barrier is not a memory operation for the compiler: the asm statements (memory clobber) on both sides keep every
// LDS read and every DMA on its side of the barrier.
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void lds_reads_done_then_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();
}
// the end of a phase's read segment, and of its MFMA segment (the second barrier exists only with the stagger, below)
__device__ __forceinline__ void segment_end() {
  lds_reads_done_then_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
template <bool STAGGER>
__device__ __forceinline__ void mfma_end() {
  if (STAGGER) {
    __builtin_amdgcn_sched_barrier(0);
    raw_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
}
// a 32-byte operand of the 16x16x128 MFMA from two 16-byte LDS slots of one row
__device__ __forceinline__ i32x8 frag32(const char* row, int s0, int s1) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(row + s0), hi = *reinterpret_cast<const u32x4*>(row + s1);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// ---------------------------------------------------------------------------------------------- block -> tile
// Block b runs on XCD b % 8; a 4 (m) x 8 (n) supertile = the 32 blocks one XCD runs at a time stays on one XCD so that its
// blocks share 4 A panels and 8 W panels in that XCD's L2 (guide T1; speed only).  The grid is whole rounds of 8 supertiles;
// a block past the last tile gets `false`.  Tile counts are the caller's (rows per tile: 256, or 128 in the half-height form).
constexpr int tile_cols(int epi) { return epi == GEMM_SWIGLU ? 128 : 256; }  // output columns per block
constexpr int col_tiles(int N, int epi) { return (N + tile_cols(epi) - 1) / tile_cols(epi); }
static inline dim3 tile_grid(int m_tiles, int n_tiles) {
  const int supertiles = ((m_tiles + 3) >> 2) * ((n_tiles + 7) >> 3);
  return dim3((unsigned)(((supertiles + 7) / 8) * 8 * 32));
}
__device__ __forceinline__ bool tile_of_block(int m_tiles, int n_tiles, int& m_tile, int& n_tile) {
  const int MS = (m_tiles + 3) >> 2, NS = (n_tiles + 7) >> 3;
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int st = (q >> 5) * 8 + xcd, wi = q & 31;
  if (st >= MS * NS) return false;
  m_tile = (st % MS) * 4 + (wi & 3);
  n_tile = (st / MS) * 8 + (wi >> 2);
  return m_tile < m_tiles && n_tile < n_tiles;
}

// ---------------------------------------------------------------------------------------------- DMA sources of a 16-KiB half
// One instruction fills 8 consecutive 128-B rows of a half tile; wave w, piece j covers rows (2w + j) * 8 .. + 8; lane l lands at
// (row + (l >> 3), slot l & 7) and fetches global 16-byte slot (l & 7) ^ (row & 7): the swizzle is applied on the SOURCE address.
__device__ __forceinline__ int piece_row(int wid, int piece, int lane) { return (wid * 2 + piece) * 8 + (lane >> 3); }
__device__ __forceinline__ int src_slot_bytes(int lane) { return ((lane & 7) ^ ((lane >> 3) & 7)) << 4; }
// A half `half`: rows at or past the tile's last valid one are clamped to it (never read out of bounds, never stored).
// T: the element (g.lda counts elements; the row offset stays an element index, so m * lda is one 32 x 32 -> 64 multiply);
// GATHER: rows may go through g.a_gather (token-grouped form).
template <class T, bool GATHER>
__device__ __forceinline__ const char* a_half_src(const GemmArgs& g, int row0, int rows_valid, int half, int wid, int piece, int lane) {
  int m = row0 + min(half * 128 + piece_row(wid, piece, lane), rows_valid - 1);
  if (GATHER && g.a_gather) m = g.a_gather[m];
  return reinterpret_cast<const char*>(reinterpret_cast<const T*>(g.a) + (size_t)m * g.lda) + src_slot_bytes(lane);
}

// ---------------------------------------------------------------------------------------------- the four-phase K loop
// Operand policy `Ops`, every member __forceinline__:
//   stage(half, k_tile, stage)   issue this wave's DMAs of one half tile of K tile k_tile into LDS stage `stage`
//   read_a(ha, stage)            LDS -> registers: this wave's four row fragments of A half ha
//   read_b(hb, stage)            ... its two column fragments of B half hb (kept per hb: quadrant (1, 0) reuses B0's)
//   mfma_quad(ha, hb)            the MFMAs of quadrant (ha, hb) on the fragments read last
//   dmas(half)                   constexpr: DMA instructions per wave that stage(half, ..) issues
// A policy may ride more on a half (the W4A8 kernel stages its scale strip with A0 and reads it with A0): what is said of a half
// below then holds for its rider too.
//
// One K tile = 4 phases, one quadrant each, every phase two segments: [fragment reads + one half tile's DMAs] | barrier |
// [MFMAs] | barrier.  The DMAs are never drained inside the loop: the one counted wait per K tile (phase 4) retires tile t + 1 and
// leaves in flight what was issued after it - A0, B0, B1 of tile t + 2, `dmas(0) + dmas(2) + dmas(3)` instructions (loads
// retire in order; the count is computed from the policy, not written).  The prologue issues all of tile 0 and A0 B0 B1 of tile 1
// and waits with the same count, i.e. for all of tile 0: it counts totals, so the order of the DMAs inside tile 0 is free (A1
// goes last only to match the loop's issue order from tile 1 on).
//
// Stagger: the wr = 1 waves run one barrier behind the wr = 0 waves (each SIMD hosts one wave of either group), so while one wave
// of a SIMD issues its MFMAs the other one does its LDS reads, and the matrix pipe never waits for a read segment.  Inside a read
// segment the fragment reads come FIRST: their latency then runs under the ~120 cycles that the DMA's issue takes (the group's
// four waves queue their 1-KiB pieces on the CU's one vector-memory path right after the barrier): -9 % cycles per K tile,
// profiles/EXPERIMENTS.md.
//
// LDS hazards, by construction.
//   WAR - a half is re-staged in the read segment AFTER the one in which it was last read: A1 of the other stage, last read in
//   phase 3 of tile t - 1, in phase 1 of tile t; A0, read in phase 1, in phase 2; B0, last read in phase 1 (phase 4 reuses the
//   registers), in phase 3; B1, read in phase 2, in phase 4.  Every read segment ends in lgkmcnt(0) + barrier and an MFMA
//   segment's barrier follows, so without the stagger two barriers lie between a wave's last read of a half and anybody's DMA
//   into it.  The stagger takes one of them: the latest readers, the wr = 1 waves, close their reads in front of the very
//   barrier behind which the earliest stagers, the wr = 0 waves, issue the DMAs.
//   RAW - tile t + 1 is waited for (the counted vmcnt, each wave for its own DMAs) in phase 4's read segment of tile t, BEFORE
//   that segment's barrier, and first read in phase 1 of tile t + 1, two barriers later.  Again the stagger takes one: the
//   latest waiters, the wr = 1 waves, wait in front of the very barrier behind which the earliest readers, the wr = 0 waves, read.
// What the phases order, and what they do not.  In the generated code the LDS reads, the DMAs and the barriers follow the four
// phases as written.  The MFMAs need not: they are pure register instructions, the passes that sink such instructions are not
// bound by `sched_barrier`, and in the two FP8-activation kernels the compiler gathers the 32 MFMAs of a K tile at the end of the
// iteration - one in front of phase 4's last barrier, 31 behind it; the overlap of MFMAs with memory then comes from the other
// waves of the block and from the DMAs in flight across iterations.  Nothing above depends on where the MFMAs stand: the hazard
// argument is about LDS reads and DMA writes only, and fragments are in registers before their segment's barrier.
template <bool STAGGER, class Ops>
__device__ __forceinline__ void k_loop(Ops& op, int nk, int wr) {
  constexpr int IN_FLIGHT = Ops::dmas(0) + Ops::dmas(2) + Ops::dmas(3);
  // ---- prologue: all of tile 0, then A0 B0 B1 of tile 1 (its A1 is staged by phase 1 of tile 0)
  op.stage(0, 0, 0);
  op.stage(2, 0, 0);
  op.stage(3, 0, 0);
  op.stage(1, 0, 0);
  if (nk > 1) {
    op.stage(0, 1, 1);
    op.stage(2, 1, 1);
    op.stage(3, 1, 1);
    wait_vm<IN_FLIGHT>();
  } else {
    wait_vm<0>();
  }
  raw_barrier();
  if (STAGGER && wr == 1) raw_barrier();
  for (int t = 0; t < nk; ++t) {
    const int s = t & 1;
    const bool more1 = t + 1 < nk, more2 = t + 2 < nk;
    // phase 1: quadrant (0, 0)
    op.read_b(0, s);
    op.read_a(0, s);
    if (more1) op.stage(1, t + 1, s ^ 1);  // A1 of the other stage: last read in phase 3 of tile t - 1
    segment_end();
    op.mfma_quad(0, 0);
    mfma_end<STAGGER>();
    // phase 2: quadrant (0, 1)
    op.read_b(1, s);
    if (more2) op.stage(0, t + 2, s);  // A0: read in phase 1
    segment_end();
    op.mfma_quad(0, 1);
    mfma_end<STAGGER>();
    // phase 3: quadrant (1, 1)
    op.read_a(1, s);
    if (more2) op.stage(2, t + 2, s);  // B0: read in phase 1
    segment_end();
    op.mfma_quad(1, 1);
    mfma_end<STAGGER>();
    // phase 4: quadrant (1, 0); retire tile t + 1 (everything issued before A0 B0 B1 of tile t + 2)
    if (more2) {
      op.stage(3, t + 2, s);  // B1: read in phase 2
      wait_vm<IN_FLIGHT>();
    } else {
      wait_vm<0>();
    }
    segment_end();
    op.mfma_quad(1, 0);
    mfma_end<STAGGER>();
  }
  if (STAGGER && wr == 0) raw_barrier();
}

// ---------------------------------------------------------------------------------------------- the 16-bit-output epilogue
// Scale policy: row(m) is loaded once per output row (ROW_LOAD: it is a load), apply<EPI>(acc, s_row, n, hb) gives what enters E::round / E::swiglu_fast
// where the 16-bit kernels read acc (n: output column, clamped to N - 1; hb: SWIGLU's matrix, 0 = W1, 1 = W3).
struct ScaleNone {  // bf16 / fp16 operands
  static constexpr bool ROW_LOAD = false;
  __device__ __forceinline__ float row(int) const { return 1.f; }
  template <int EPI>
  __device__ __forceinline__ float apply(float acc, float, int, int) const { return acc; }
};
struct ScaleRow {  // one fp32 per activation row (W4A8: the weights' block scales were applied inside the contraction)
  static constexpr bool ROW_LOAD = true;
  const float* sx;
  __device__ __forceinline__ float row(int m) const { return sx[m]; }
  template <int EPI>
  __device__ __forceinline__ float apply(float acc, float s_row, int, int) const { return acc * s_row; }
};
struct ScaleRowCol {  // ... times one fp32 per weight row (W8A8): the product of the two scales is formed first
  static constexpr bool ROW_LOAD = true;
  const GemmW8A8Args& a;
  __device__ __forceinline__ float row(int m) const { return a.sx[m]; }
  template <int EPI>
  __device__ __forceinline__ float apply(float acc, float s_row, int n, int hb) const {
    const GemmArgs& g = a.g;
    const float s_col = EPI == GEMM_SWIGLU ? a.sw[hb][n] : n < g.n0 ? a.sw[0][n] : n < g.n1 ? a.sw[1][n - g.n0] : a.sw[2][n - g.n1];
    return acc * (s_row * s_col);
  }
};

// EPI: GEMM_STORE (with the RoPE epilogue of q|k|v) / GEMM_RESIDUAL / GEMM_SWIGLU.  The MFMAs were issued as W-fragment x
// A-fragment, i.e. they produced the transposed 16x16 tiles: acc[ha][hb][i][j][r] is tile row ha*128 + wr*64 + i*16 + (lane & 15),
// tile column hb*128 + wc*32 + j*16 + (lane >> 4)*4 + r - four CONSECUTIVE output columns per lane, so results (and the
// residual) move as 8-byte accesses instead of 2-byte ones.  (SWIGLU: hb = 0 is W1's product and hb = 1 W3's, of column wc*32 +
// j*16 + (lane >> 4)*4 + r.)
template <class E, int EPI, int MH, class Scale>
__device__ __forceinline__ void epilogue16(const GemmArgs& g, const f32x4 (&acc)[MH][2][4][2], const Scale& sc, int row0, int rows_valid,
                                           int n_tile, int wr, int wc, int lane) {
  const int cq = (lane >> 4) * 4;
  const bool rope = EPI == GEMM_STORE && g.rope_cs != nullptr;
  const bool wide_ok = (g.ldo & 3) == 0 && (reinterpret_cast<size_t>(g.out) & 15) == 0 &&
                       (EPI != GEMM_RESIDUAL || (reinterpret_cast<size_t>(g.residual) & 7) == 0);
#pragma unroll
  for (int ha = 0; ha < MH; ++ha)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rl = ha * 128 + wr * 64 + i * 16 + (lane & 15);
      if (rl >= rows_valid) continue;
      const int row = row0 + rl;
      const size_t ob = (size_t)row * g.ldo;
      const float s_row = sc.row(row);
      const int tp = rope ? g.tok_pos[row] : 0;
      // The row's loads (where the policy or the RoPE epilogue has one) are waited for HERE, once: left to itself the wait sinks
      // into the first column block's conditional, every later block of the row then waits again, and that vmcnt(0) also waits
      // for the block's stores before it.
      if constexpr (Scale::ROW_LOAD) asm volatile("" ::"v"(s_row));
      if constexpr (EPI == GEMM_STORE) asm volatile("" ::"v"(tp));
      if (EPI == GEMM_SWIGLU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = n_tile * 128 + wc * 32 + j * 16 + cq;
          if (n >= g.N) continue;
          float y[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nn = min(n + r, g.N - 1);
            y[r] = E::swiglu_fast(sc.template apply<EPI>(acc[ha][0][i][j][r], s_row, nn, 0), sc.template apply<EPI>(acc[ha][1][i][j][r], s_row, nn, 1));
          }
          uint16_t* o = reinterpret_cast<uint16_t*>(g.out) + ob + n;
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
            for (int r = 0; r < 4; ++r) y[r] = E::round(sc.template apply<EPI>(acc[ha][hb][i][j][r], s_row, min(n + r, g.N - 1), hb));
            if (EPI == GEMM_STORE && rope && n < g.rope_cols) {
              // rotary embedding on the rounded projection (transformer_layers.py:66-70): this lane's four columns are two
              // (re, im) pairs of one head; their (cos, sin) entries are 16 contiguous bytes of the table
              const int i0 = ((n + g.rope_col0) % g.rope_dh) >> 1;
              const f32x4 cs = *reinterpret_cast<const f32x4*>(g.rope_cs + ((size_t)tp * (g.rope_dh >> 1) + i0) * 2);
              float re, im;
              rope_pair(y[0], y[1], cs[0], cs[1], re, im);
              y[0] = E::round(re); y[1] = E::round(im);
              rope_pair(y[2], y[3], cs[2], cs[3], re, im);
              y[2] = E::round(re); y[3] = E::round(im);
            }
            uint16_t* o = reinterpret_cast<uint16_t*>(g.out) + ob + n;
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

// ---------------------------------------------------------------------------------------------- host side
// > 64 KiB of dynamic LDS needs the opt-in once per kernel; then the launch (512 threads)
template <auto KERNEL, int LDS, class Args>
hipError_t launch_one(const Args& a, dim3 grid, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(512), LDS, s, a);
  return hipGetLastError();
}

// What the two FP8-activation launchers ask of a call: the route's shape predicate, lda, 16-byte aligned activations and weight
// bases (every DMA fetches 16 aligned bytes; the rows are a multiple of 64 bytes apart, so the bases decide), the plain form (no
// tile table, no gather), and a pointer for every segment in use.
template <class scale_t>
static inline bool a8_args_ok(const GemmA8Args<scale_t>& a) {
  const GemmArgs& g = a.g;
  if (!gemm256_w8a8_applicable(g.M, g.K) || g.lda < g.K || (g.lda & 15) || (reinterpret_cast<size_t>(g.a) & 15) || g.tile_tab ||
      g.a_gather || !a.sx || !g.w0 || !a.sw[0] || g.N <= 0 || g.n0 <= 0)
    return false;
  if ((reinterpret_cast<size_t>(g.w0) | reinterpret_cast<size_t>(g.w1) | reinterpret_cast<size_t>(g.w2)) & 15) return false;
  return g.epi == GEMM_SWIGLU ? (g.w1 && a.sw[1]) : !((g.n0 < g.N && (!g.w1 || !a.sw[1])) || (g.n1 < g.N && (!g.w2 || !a.sw[2])));
}

}  // namespace gemm256_core
