// W4A8 MFMA GEMM for prefills of MXFP4 models: out[M,N] = epilogue((sum_k e4m3(A_q[m, k]) * e2m1(C[n, k]) * 2^(S[n, k/32] - 127)) *
// s_x[m]), A_q [M, K] e4m3 bytes with one fp32 scale per row (act_quant_e4m3, elementwise.hip), C [N, K / 2] MXFP4 code bytes (two
// e2m1 codes per byte, the low nibble at the even k) and S [N, K / 32] e8m0 block scale bytes, both as the checkpoint stores them.
//
// The structure is gemm256_w8a8.hip's: 8 waves = 2 (M) x 4 (N), a 256 x 256 block tile (256 x 128 for SwiGLU, whose B halves are W1
// and W3), a K tile of 128 elements, halves staged by `global_load_lds` (16 bytes per lane), two stages, four phases per K tile
// (of the LDS reads and DMAs; where the MFMAs end up is said below), the wr = 1 waves one barrier behind the wr = 0 waves.
// One `v_mfma_scale_f32_16x16x128_f8f6f4` per (row fragment, column fragment) with a FORMAT PER OPERAND: the weights are the instruction's first operand as e2m1 (cbsz = 4), the activations its
// second as e4m3 (blgp = 0).  A lane's FP4 operand is 32 codes of one weight row - exactly one MX block - and the instruction's
// per-lane scale byte of the first operand is an e8m0 - exactly the checkpoint's byte - so the hardware applies the block scales
// inside the contraction: no dequantisation, no epilogue work for the weights.  The activations' block scale is 127 (2^0); their
// per-row scale enters in the epilogue.
//
// Halves.  A: 128 rows x 128 B = 16 KiB, as in the W8A8 kernel (one DMA fills 8 rows; slot ^= row & 7 on the SOURCE address).
// B: 128 rows x 64 B = 8 KiB: a row of a K tile is 4 slots of 16 bytes, one DMA fills 16 rows, wave w fills rows 16 w .. + 16 of
// either B half; lane l lands at (row 16 w + (l >> 2), slot l & 3) and fetches global slot (l & 3) ^ ((row >> 2) & 3) =
// (l & 3) ^ ((l >> 4) & 3).  A stage is 48 KiB (A0 A1 B0 B1), the two stages 96 KiB.
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
// names, op_sel = 0, no shift.  The four bytes are read once per tile, in phase 1, and held.  The strip lives in the stage of its
// tile (2 KiB behind B1: a stage is 50 KiB, the two 100 KiB); it needs the scale matrices 4-byte aligned (rows are K / 32 = 4 k
// bytes), which the launcher checks.
//
// The counted vmcnt, re-derived.  Per wave an A half is 2 DMAs, a B half 1, the scale strip 1; loads retire in order.
//   prologue:  A0 B0 B1 A1 S of tile 0 (7), then A0 S B0 B1 of tile 1 (5)                              -> vmcnt(5): tile 0 complete
//   tile t:    phase 1  A1 of t + 1 (2)         phase 2  A0 of t + 2 (2), S of t + 2 (1)
//              phase 3  B0 of t + 2 (1)         phase 4  B1 of t + 2 (1)                               -> vmcnt(5)
// The five still in flight after phase 4's wait are A0 (2), S, B0, B1 of tile t + 2; everything older - A0 S B0 B1 of tile t + 1
// from the tile before, and this tile's phase 1: A1 of t + 1 - has landed.  Without a tile t + 2 the wait is vmcnt(0).
// LDS hazards are gemm256.hip's argument unchanged, since which half is staged in which phase is unchanged: a half is re-staged
// in the read segment AFTER the one in which it was last read (A1 of the other stage: last read in phase 3 of tile t - 1, staged in
// phase 1 of t; A0: read in phase 1, staged in phase 2; B0: last fragment read in phase 1 - phase 4 reuses registers - staged in
// phase 3; B1: read in phase 2, staged in phase 4; the scale strip: read in phase 1, staged in phase 2 like A0), every read segment
// ends in lgkmcnt(0) + barrier, and the wr = 1 waves, one barrier behind, have passed the barrier that closes their reads of a half
// before any wave's next segment stages it.  Tile t + 1 is waited for in phase 4's first segment of tile t by every wave for its
// own DMAs and read two barriers later.
//
// What the phases order, and what they do not.  In the generated code (this kernel and gemm256_w8a8.hip alike) the LDS reads, the
// DMAs and the barriers follow the four phases as written; the MFMAs do not: they are pure register instructions, the passes that
// sink such instructions are not bound by `sched_barrier`, and the compiler gathers the 32 MFMAs of a K tile at the end of the
// iteration - one in front of phase 4's last barrier, 31 behind it.  An iteration therefore runs as [all fragment reads, all DMA
// issues, the barriers] then [32 MFMAs], and the overlap of MFMAs with memory comes from the other waves of the block and from the
// DMAs in flight across iterations, not from phases inside a wave.  Nothing above depends on where the MFMAs stand: the hazard
// argument is about LDS reads and DMA writes only, and fragments are in registers before their segment's barrier.  The measured
// rates (profiles/EXPERIMENTS.md) are of this code; pinning the MFMAs into their phases is untried.
//
// Rows at or past M / N are clamped to the last valid one, codes and scales alike: nothing is read out of bounds, nothing is stored
// past a ragged edge.  Epilogues: GEMM_STORE (RoPE epilogue of q|k|v, up to three segments), GEMM_RESIDUAL, GEMM_SWIGLU with the
// bf16 kernel's rounding points and acc * s_x[m] in fp32 where it reads acc.  Scale bytes below 3 give bf16 subnormals in the
// weight-only route's image, which it may flush; here they are exact in fp32.  No LM head, no token-grouped form.
#include "common.cuh"
#include "kernels.h"

using E = Elem16<0>;  // outputs, residual and the RoPE / SwiGLU chains are bf16

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;                                  // elements of K per tile
constexpr int A_HALF = 128 * BK;                         // 16 KiB: 128 rows x 128 e4m3 bytes
constexpr int B_HALF = 128 * BK / 2;                     // 8 KiB: 128 rows x 64 code bytes
constexpr int S_COPY = 256 * 4;                          // 1 KiB: one dword of scale bytes per weight row of the block
constexpr int STAGE_BYTES = 2 * A_HALF + 2 * B_HALF + 2 * S_COPY;  // A0 A1 B0 B1 S S
constexpr int LDS_BYTES = 2 * STAGE_BYTES;               // 100 KiB
constexpr int B_BASE = 2 * A_HALF;                       // of B0 inside a stage
constexpr int S_BASE = B_BASE + 2 * B_HALF;              // of the scale strip's first copy

__device__ __forceinline__ void dma16(const uint8_t* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const uint8_t* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
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
__device__ __forceinline__ i32x8 frag_a(const char* row, int s0, int s1) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(row + s0), hi = *reinterpret_cast<const u32x4*>(row + s1);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
__device__ __forceinline__ i32x8 frag_b(const char* p) {
  const u32x4 c = *reinterpret_cast<const u32x4*>(p);
  return i32x8{(int)c[0], (int)c[1], (int)c[2], (int)c[3], 0, 0, 0, 0};
}
// e2m1 (format code 4) x e4m3 (0); the first operand's block scale is byte 0 of `scale`, the second's 2^(127 - 127)
__device__ __forceinline__ f32x4 mfma128(i32x8 w, i32x8 x, f32x4 c, int scale) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 0, 0, scale, 0, 127);
}

template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_w4a8_kernel(GemmW4A8Args args) {
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

  // ---- DMA sources (header).  Rows at or past M / N are clamped to the last valid one.
  const uint8_t* const a8 = reinterpret_cast<const uint8_t*>(g.a);
  const uint8_t* srcA[2][2];  // [A half][piece]
  const uint8_t* srcB[2];     // [B half]
  {
    const int sslot = (lane & 7) ^ ((lane >> 3) & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = (wid * 2 + j) * 8 + (lane >> 3);
        const int m = row0 + min(h * 128 + r, rows_valid - 1);
        srcA[h][j] = a8 + (size_t)m * g.lda + sslot * 16;
      }
    const int bslot = (lane & 3) ^ ((lane >> 4) & 3);
    const int r = wid * 16 + (lane >> 2);
    const size_t ldw = (size_t)(g.K >> 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (EPI == GEMM_SWIGLU) {
        const int n = min(n_tile * 128 + r, g.N - 1);
        srcB[h] = reinterpret_cast<const uint8_t*>(h == 0 ? g.w0 : g.w1) + (size_t)n * ldw + bslot * 16;
      } else {
        const int n = min(n_tile * 256 + h * 128 + r, g.N - 1);
        srcB[h] = seg_codes(args, n) + bslot * 16;
      }
    }
  }
  char* const pieceA = smem + wid * 2048;           // this wave's two 1-KiB pieces inside either A half
  char* const pieceB = smem + B_BASE + wid * 1024;  // its 1-KiB piece inside either B half
#define STAGE_A(H, KT, STAGE)                                      \
  do {                                                             \
    char* dst_ = pieceA + (STAGE) * STAGE_BYTES + (H) * A_HALF;    \
    dma16(srcA[H][0] + (size_t)(KT) * BK, dst_);                   \
    dma16(srcA[H][1] + (size_t)(KT) * BK, dst_ + 1024);            \
  } while (0)
#define STAGE_B(H, KT, STAGE) dma16(srcB[H] + (size_t)(KT) * (BK / 2), pieceB + (STAGE) * STAGE_BYTES + (H) * B_HALF)

  // ---- fragment addressing
  const int fq = lane >> 4;
  const int sw0 = (fq ^ (lane & 7)) << 4, sw1 = ((4 + fq) ^ (lane & 7)) << 4;  // A: k = 16 fq .. + 16 and 64 + 16 fq .. + 16
  const int a_off = (wr * 64 + (lane & 15)) * 128;
  const int b_off = B_BASE + (wc * 32 + (lane & 15)) * 64 + ((fq ^ ((lane >> 2) & 3)) << 4);

  // ---- block scales (header): this lane's row of the strip as a DMA source, and its four bytes of the strip as a reader
  const uint8_t* srcS;
  {
    const int b = (wid & 3) * 64 + lane;  // weight row of the block
    if (EPI == GEMM_SWIGLU) {
      const int n = min(n_tile * 128 + (b & 127), g.N - 1);
      srcS = args.sw[b >> 7] + (size_t)n * (size_t)(g.K >> 5);
    } else {
      srcS = seg_scales(args, min(n_tile * 256 + b, g.N - 1));
    }
  }
  char* const pieceS = smem + S_BASE + (wid >> 2) * S_COPY + (wid & 3) * 256;
#define STAGE_S(KT, STAGE) dma4(srcS + (size_t)(KT) * 4, pieceS + (STAGE) * STAGE_BYTES)
  const int s_off = S_BASE + wr * S_COPY + (wc * 32 + (lane & 15)) * 4 + fq;
  int sc[2][2];  // [B half][column fragment]: the e8m0 byte of this lane's block of the tile in use
#define READ_S(SB)                                                                        \
  _Pragma("unroll") for (int hb = 0; hb < 2; ++hb)                                        \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                           \
    sc[hb][j] = *reinterpret_cast<const uint8_t*>((SB) + s_off + hb * 512 + j * 64);

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
  _Pragma("unroll") for (int i = 0; i < 4; ++i) af[i] = frag_a((SB) + (HA) * A_HALF + a_off + i * 2048, sw0, sw1);
#define READ_B(DST, HB, SB)                                                               \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) DST[j] = frag_b((SB) + (HB) * B_HALF + b_off + j * 1024);
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
    acc[HA][HB][i][j] = mfma128(BF[j], af[i], acc[HA][HB][i][j], sc[HB][j]);

  const int nk = g.K / BK;
  // ---- prologue: all of tile 0, then A0 S B0 B1 of tile 1 (its A1 is staged by phase 1 of tile 0)
  STAGE_A(0, 0, 0);
  STAGE_B(0, 0, 0);
  STAGE_B(1, 0, 0);
  STAGE_A(1, 0, 0);
  STAGE_S(0, 0);
  if (nk > 1) {
    STAGE_A(0, 1, 1);
    STAGE_S(1, 1);
    STAGE_B(0, 1, 1);
    STAGE_B(1, 1, 1);
    wait_vm<5>();
  } else {
    wait_vm<0>();
  }
  raw_barrier();
  if (wr == 1) raw_barrier();
  for (int t = 0; t < nk; ++t) {
    const int s = t & 1;
    const char* sb = smem + s * STAGE_BYTES;
    const bool more1 = t + 1 < nk, more2 = t + 2 < nk;
    // phase 1: quadrant (0, 0)
    READ_B(b0x, 0, sb)
    READ_A(0, sb)
    READ_S(sb)
    if (more1) STAGE_A(1, t + 1, s ^ 1);  // A1 of the other stage: last read in phase 3 of tile t - 1
    SEGMENT_END();
    MFMA_QUAD(0, 0, b0x)
    MFMA_END();
    // phase 2: quadrant (0, 1)
    READ_B(b1, 1, sb)
    if (more2) {
      STAGE_A(0, t + 2, s);  // A0: read in phase 1
      STAGE_S(t + 2, s);     // the scale strip: read in phase 1
    }
    SEGMENT_END();
    MFMA_QUAD(0, 1, b1)
    MFMA_END();
    // phase 3: quadrant (1, 1)
    READ_A(1, sb)
    if (more2) STAGE_B(0, t + 2, s);  // B0: read in phase 1
    SEGMENT_END();
    MFMA_QUAD(1, 1, b1)
    MFMA_END();
    // phase 4: quadrant (1, 0); retire tile t + 1 (everything issued before the last five: A0 A0 S B0 B1 of tile t + 2)
    if (more2) {
      STAGE_B(1, t + 2, s);  // B1: read in phase 2
      wait_vm<5>();
    } else {
      wait_vm<0>();
    }
    SEGMENT_END();
    MFMA_QUAD(1, 0, b0x)
    MFMA_END();
  }
  if (wr == 0) raw_barrier();
#undef STAGE_A
#undef STAGE_B
#undef STAGE_S
#undef READ_S
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
          for (int r = 0; r < 4; ++r) y[r] = E::swiglu_fast(acc[ha][0][i][j][r] * sx, acc[ha][1][i][j][r] * sx);
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
            for (int r = 0; r < 4; ++r) y[r] = E::round(acc[ha][hb][i][j][r] * sx);
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
hipError_t launch_one(const GemmW4A8Args& a, dim3 grid, hipStream_t s) {
  static bool attr_set = false;  // > 64 KiB of dynamic LDS needs the opt-in once per kernel
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm256_w4a8_kernel<EPI>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm256_w4a8_kernel<EPI>), grid, dim3(512), LDS_BYTES, s, a);
  return hipGetLastError();
}

}  // namespace

// (the W8A8 predicate: the activation quantiser in front of either GEMM is the same, and a K tile is 128 elements in both)
bool gemm256_w4a8_applicable(int M, int K) { return gemm256_w8a8_applicable(M, K); }

hipError_t launch_gemm256_w4a8(const GemmW4A8Args& a, hipStream_t s) {
  const GemmArgs& g = a.g;
  if (!gemm256_w4a8_applicable(g.M, g.K) || g.lda < g.K || (g.lda & 15) || (reinterpret_cast<size_t>(g.a) & 15) || g.tile_tab ||
      g.a_gather || !a.sx || !g.w0 || !a.sw[0] || g.N <= 0 || g.n0 <= 0)
    return hipErrorInvalidValue;
  // every DMA fetches 16 aligned bytes: the code rows are K / 2 = 64 k bytes apart, so their bases decide
  if ((reinterpret_cast<size_t>(g.w0) | reinterpret_cast<size_t>(g.w1) | reinterpret_cast<size_t>(g.w2)) & 15) return hipErrorInvalidValue;
  // the scale strip's DMA fetches 4 aligned bytes: the scale rows are K / 32 = 4 k bytes apart, so their bases decide
  if ((reinterpret_cast<size_t>(a.sw[0]) | reinterpret_cast<size_t>(a.sw[1]) | reinterpret_cast<size_t>(a.sw[2])) & 3) return hipErrorInvalidValue;
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
