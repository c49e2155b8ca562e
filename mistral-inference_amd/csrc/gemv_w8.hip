// Weight-streaming GEMV kernels for M <= 8 tokens whose weight rows are OCP e4m3 bytes (weight-only FP8), and the
// dequantisation pass of the prefill route.
//
// The real-valued weight is scale[r] * e4m3(W[r, k]) (fp32 row scales).  Per output row: acc = sum_k e4m3(W[r, k]) * x[k] in fp32,
// y = acc * scale[r] in fp32, and y enters the epilogues of gemv_core.cuh exactly where acc enters them there: bf16(y), then RoPE
// and the ring write, the residual, or SwiGLU.
//
// Same structure as gemv.hip: activation loads first (gemv_core::x_issue / x_finish as they are, so the normalised rows in LDS are
// bit-identical to the bf16 kernels'), two batches of 8 unconditional 16-byte non-temporal loads in flight across unit boundaries,
// no `cond ? load : 0`, both steps per trip, epilogue operands (row scales included) fetched when a unit starts.  A 16-byte piece
// is 16 weights, so one wave instruction covers 1024 k and K % 16 == 0.
//
// Conversion: v_cvt_pk_f32_fp8 turns two bytes into two fp32; every finite e4m3 value is exact in bf16, so the high halves of the
// two results, packed by v_perm_b32, are an exact bf16 pair for v_dot2c_f32_bf16.  Per dword of weights: 2 converts + 2 perms
// (shared by all tokens) + 2 dot2 per token, against 4 unpacks + 4 FMAs per token for the plain-fp32 form.
//
// A row is half the bytes of a bf16 row, so the fixed cost of a unit (wave reductions, epilogue, loop bookkeeping) weighs twice
// as much.  Units are therefore RP row pairs: RP = 2 (four rows) where the matrix has enough row pairs that every wave of the grid
// still gets at least two units (W1|W3), else RP = 1 (launch_gemv_w8).
#include <cstdlib>

#include "common.cuh"
#include "gemv_core.cuh"

namespace {

using gemv_core::BATCH;
using gemv_core::XRegs;

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// four e4m3 bytes (k .. k + 3) -> the bf16 pairs (k, k + 1) and (k + 2, k + 3)
__device__ __forceinline__ void cvt4_e4m3(uint32_t w, uint32_t& p01, uint32_t& p23) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  // bytes 2, 3 of the first operand's partner (S1) below bytes 2, 3 of S0: (S1 >> 16) | (S0 & 0xffff0000)
  p01 = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
  p23 = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
}

template <int NR>
struct Rows8 {
  const uint8_t* p[NR];
};

// One batch = chunks [c0, c0 + BATCH / NR) of each of the unit's NR rows: always exactly BATCH unconditional loads; chunk offsets
// past K are clamped to the row's last 16 bytes (fma_batch8 skips them).
template <int NR>
__device__ __forceinline__ void load_batch8(const Rows8<NR>& r, int c0, int K, int lane, u32x4 (&buf)[BATCH]) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = min(((c0 + u) * 64 + lane) * 16, K - 16);
#pragma unroll
    for (int i = 0; i < NR; ++i) buf[i * U + u] = ld16_nt(r.p[i] + e);
  }
}

template <int TT, int NR>
__device__ __forceinline__ void fma_batch8(const u32x4 (&buf)[BATCH], int c0, const bf16_t* xs, int K, int lane, float (&acc)[NR][TT]) {
  constexpr int U = BATCH / NR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = ((c0 + u) * 64 + lane) * 16;
    if (e < K) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // halves of the piece: 8 weights = 2 dwords against one 16-byte piece of x
        uint32_t p[NR][4];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          cvt4_e4m3(buf[i * U + u][2 * h], p[i][0], p[i][1]);
          cvt4_e4m3(buf[i * U + u][2 * h + 1], p[i][2], p[i][3]);
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)t * K + e + 8 * h);
#pragma unroll
          for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][t] = dot2_bf16(p[i][c], xv[c], acc[i][t]);
        }
      }
    }
  }
}

__device__ __forceinline__ const uint8_t* seg_row8(const GemvArgs& a, int r) {
  if (r < a.n0) return reinterpret_cast<const uint8_t*>(a.w0) + (size_t)r * a.K;
  if (r < a.n1) return reinterpret_cast<const uint8_t*>(a.w1) + (size_t)(r - a.n0) * a.K;
  return reinterpret_cast<const uint8_t*>(a.w2) + (size_t)(r - a.n1) * a.K;
}
__device__ __forceinline__ float seg_scale(const GemvW8Args& wa, int r) {
  const GemvArgs& a = wa.g;
  if (r < a.n0) return wa.scale[0][r];
  if (r < a.n1) return wa.scale[1][r - a.n0];
  return wa.scale[2][r - a.n1];
}

// Row pair q: SWIGLU = (W1 row q, W3 row q), else output rows (2 q, 2 q + 1); an odd N's missing last row aliases its partner
// (the epilogue drops it).
template <int MODE>
__device__ __forceinline__ void pair_rows(const GemvArgs& a, int q, const uint8_t*& ra, const uint8_t*& rb) {
  if (MODE == GEMV_SWIGLU) {
    ra = reinterpret_cast<const uint8_t*>(a.w0) + (size_t)q * a.K;
    rb = reinterpret_cast<const uint8_t*>(a.w1) + (size_t)q * a.K;
  } else {
    ra = seg_row8(a, 2 * q);
    rb = (2 * q + 1 < a.N) ? seg_row8(a, 2 * q + 1) : ra;
  }
}

// TT: token rows staged in LDS; MODE: GEMV_STORE / GEMV_RESIDUAL / GEMV_SWIGLU / GEMV_QKV_ROPE; RP: row pairs per unit;
// DMA: the activation rows go to LDS by LDS-DMA (gemv_core.cuh)
template <int TT, int MODE, int RP, bool DMA>
__device__ __forceinline__ void gemv_w8_body(const GemvW8Args& wa, char* smem, int block_id, int n_blocks) {
  const GemvArgs& a = wa.g;
  constexpr int NR = 2 * RP, U = BATCH / NR;
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + (size_t)TT * a.K * 2);
  bf16_t* ws = reinterpret_cast<bf16_t*>(smem + (size_t)TT * a.K * 2 + 16 * TT);  // (launch_gemv_w8 reserves it for TT > 1)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwaves = n_blocks * 4;
  constexpr bool kPairOut = MODE != GEMV_SWIGLU;
  const int npairs = kPairOut ? (a.N + 1) >> 1 : a.N;
  const int units = (npairs + RP - 1) / RP;
  const int nch = (a.K + 1023) >> 10;
  const int nb = (nch + U - 1) / U;  // batches per unit
  const int T = a.T;

  // 1. activation (and norm weight) loads first, 2. two weight batches, 3. finish the prologue under them (gemv_core.cuh)
  constexpr bool kNormMode = MODE == GEMV_QKV_ROPE || MODE == GEMV_SWIGLU;
  constexpr int NX = kNormMode ? 4 : 8, NW = kNormMode ? 4 : 0;
  XRegs<NX, NW> xr;
  const int tl = lane < T ? lane : 0;
  int ep_pos = 0, ep_seq = 0;
  if (MODE == GEMV_QKV_ROPE) {  // the oldest loads of the wave: waited for with the weights in flight
    ep_pos = a.tok_pos[tl];
    ep_seq = a.tok_seq ? a.tok_seq[tl] : tl;
  }
  const bool in_regs = gemv_core::x_issue<TT, NX, NW, DMA, 256>(xr, a.x, a.ldx, T, a.K, a.norm_w, xs, ws);

  // load cursor over the flattened (unit, batch) sequence of this wave: always two batches ahead of the math
  int u = block_id * 4 + wid;
  int ul = u, jl = 0;
  auto unit_rows = [&](int uu) {
    Rows8<NR> r;
#pragma unroll
    for (int p = 0; p < RP; ++p) pair_rows<MODE>(a, min(uu * RP + p, npairs - 1), r.p[2 * p], r.p[2 * p + 1]);
    return r;
  };
  Rows8<NR> rpl = unit_rows(min(ul, units - 1));
  u32x4 bufA[BATCH], bufB[BATCH];
  // past the wave's last unit: BATCH loads of one L2-resident line, selected not branched around (gemv_core.cuh)
  const uint8_t* dummy = reinterpret_cast<const uint8_t*>(a.x);
  auto issue = [&](u32x4 (&buf)[BATCH]) {
    const bool live = ul < units;
    Rows8<NR> r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.p[i] = live ? rpl.p[i] : dummy;
    load_batch8<NR>(r, live ? jl * U : 0, live ? a.K : 16, live ? lane : 0, buf);
    if (live && ++jl == nb) {
      jl = 0;
      ul += nwaves;
      if (ul < units) rpl = unit_rows(ul);
    }
  };
  issue(bufA);
  issue(bufB);
  gemv_core::x_finish<TT, NX, NW, DMA, 256>(in_regs, xr, xs, red, ws, a.x, a.ldx, T, a.K, a.norm_w, a.eps);

  float acc[NR][TT];
#pragma unroll
  for (int i = 0; i < NR; ++i)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;
  int jc = 0;

  // epilogue operands fetched when the unit starts: the rows' scales, the pair's RoPE entry / residual pair
  float ep_s[NR];
  float2 ep_cs[RP];
  uint32_t ep_res[RP];
#pragma unroll
  for (int p = 0; p < RP; ++p) {
    ep_s[2 * p] = ep_s[2 * p + 1] = 1.f;
    ep_cs[p] = make_float2(1.f, 0.f);
    ep_res[p] = 0;
  }
  auto prefetch_epilogue = [&](int uu) {
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const int q = min(uu * RP + p, npairs - 1);
      if (MODE == GEMV_SWIGLU) {
        ep_s[2 * p] = wa.scale[0][q];
        ep_s[2 * p + 1] = wa.scale[1][q];
      } else {
        const int r0 = 2 * q;
        const bool two = r0 + 1 < a.N;
        ep_s[2 * p] = seg_scale(wa, r0);
        ep_s[2 * p + 1] = seg_scale(wa, two ? r0 + 1 : r0);
        if (MODE == GEMV_QKV_ROPE && r0 < a.n1) {
          const int i = (r0 % a.head_dim) >> 1;
          ep_cs[p] = *reinterpret_cast<const float2*>(a.rope_cs + ((size_t)ep_pos * (a.head_dim >> 1) + i) * 2);
        }
        if (MODE == GEMV_RESIDUAL) {
          const bf16_t* rs = a.residual + (size_t)tl * a.ldo + r0;
          if (two) ep_res[p] = *reinterpret_cast<const uint32_t*>(rs);
          else ep_res[p] = rs[0];
        }
      }
    }
  };
  if (u < units) prefetch_epilogue(u);

  auto finish_unit = [&]() {
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[i][t] = wave_sum(acc[i][t]);
    // ---- epilogue: lane t finishes token t
    float v[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] = 0.f;
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (lane == t) {
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = acc[i][t];
      }
    if (lane < T) {
      const int t = lane;
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        const int q = u * RP + p;
        if (q < npairs) {
          const float s0 = v[2 * p] * ep_s[2 * p], s1 = v[2 * p + 1] * ep_s[2 * p + 1];  // y = acc * scale, fp32
          if (MODE == GEMV_SWIGLU) {
            bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + (size_t)t * a.ldo + q;
            *o = f_to_bf(swiglu_bf(s0, s1));
          } else {
            const int r0 = 2 * q;
            const bool two = r0 + 1 < a.N;
            float y0 = bf_round(s0), y1 = bf_round(s1);
            bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + (size_t)t * a.ldo + r0;
            if (MODE == GEMV_RESIDUAL) {
              y0 = bf_lo(ep_res[p]) + y0;
              if (two) y1 = bf_hi(ep_res[p]) + y1;
            }
            if (MODE == GEMV_QKV_ROPE) {
              if (r0 < a.n1) {  // q or k rows: rotate the adjacent pair (rope.py:13-23)
                float re, im;
                rope_pair(y0, y1, ep_cs[p].x, ep_cs[p].y, re, im);
                y0 = re;
                y1 = im;
              }
              if (a.write_kv && r0 >= a.n0) {  // cache.py:83-92: ring slot pos % W of this sequence's row
                const int kv_dim = a.n1 - a.n0;
                const size_t off = kv_offset(a.kv_layout, a.W, kv_dim, a.head_dim, (size_t)ep_seq, ep_pos % a.W,
                                             (r0 < a.n1) ? r0 - a.n0 : r0 - a.n1);
                bf16_t* ring = ((r0 < a.n1) ? reinterpret_cast<bf16_t*>(a.cache_k) : reinterpret_cast<bf16_t*>(a.cache_v)) + off;
                *reinterpret_cast<uint32_t*>(ring) = pack_bf2(y0, y1);
              }
            }
            if (two) {
              *reinterpret_cast<uint32_t*>(o) = pack_bf2(y0, y1);
            } else {
              o[0] = f_to_bf(y0);
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;
  };

  // one step = consume the oldest batch, refill the same registers with the batch two ahead; ALWAYS both steps per trip
  // (gemv_core.cuh: a step past the wave's last unit multiplies dummy lines and stores nothing)
  auto step = [&](u32x4 (&buf)[BATCH]) {
    fma_batch8<TT, NR>(buf, jc * U, xs, a.K, lane, acc);
    issue(buf);
    if (++jc == nb) {
      jc = 0;
      if (u < units) finish_unit();
      u += nwaves;
      if (u < units) prefetch_epilogue(u);
    }
  };
  if (u < units) {
    do {
      step(bufA);
      step(bufB);
    } while (u < units);
  }
}

template <int TT, int MODE, int RP, bool DMA>
__global__ __launch_bounds__(256, (TT == 1 ? 4 : (TT <= 3 ? 3 : 2))) void gemv_w8_kernel(GemvW8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_w8_body<TT, MODE, RP, DMA>(a, smem, blockIdx.x, gridDim.x);
}

template <int TT, int MODE, int RP, bool DMA>
hipError_t launch_tt(const GemvW8Args& a, dim3 grid, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024) {  // more than the default dynamic-LDS limit: an opt-in per function AND per device
    static bool attr_set[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_w8_kernel<TT, MODE, RP, DMA>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMV_LDS_BUDGET + 1024);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL((gemv_w8_kernel<TT, MODE, RP, DMA>), grid, dim3(256), lds, s, a);
  return hipGetLastError();
}
// rows that fit the prologue's register set are staged through registers; 2..8 rows that do not, by LDS-DMA (as gemv.hip)
template <int TT, int MODE>
hipError_t launch_stage(const GemvW8Args& a, int rp, dim3 grid, size_t lds, hipStream_t s) {
  if constexpr (TT > 1) {
    constexpr bool norm_mode = MODE == GEMV_QKV_ROPE || MODE == GEMV_SWIGLU;  // (gemv_w8_body's kNormMode)
    if ((size_t)TT * (a.g.K >> 3) > (norm_mode ? 4u : 8u) * 256u) return launch_tt<TT, MODE, 1, true>(a, grid, lds, s);
    return launch_tt<TT, MODE, 1, false>(a, grid, lds, s);
  } else {
    return rp == 2 ? launch_tt<1, MODE, 2, false>(a, grid, lds, s) : launch_tt<1, MODE, 1, false>(a, grid, lds, s);
  }
}
template <int MODE>
hipError_t launch_mode(const GemvW8Args& a, int TT, int rp, dim3 grid, size_t lds, hipStream_t s) {
  switch (TT) {
    case 1: return launch_stage<1, MODE>(a, rp, grid, lds, s);
    case 2: return launch_stage<2, MODE>(a, rp, grid, lds, s);
    case 3: return launch_stage<3, MODE>(a, rp, grid, lds, s);
    case 4: return launch_stage<4, MODE>(a, rp, grid, lds, s);
    case 6: return launch_stage<6, MODE>(a, rp, grid, lds, s);
    default: return launch_stage<8, MODE>(a, rp, grid, lds, s);
  }
}

// ---- rows of e4m3 + row scales -> bf16 rows: out[r, k] = bf16(scale[r] * e4m3(W[r, k])).  One 16-byte load and two 16-byte
// stores per lane; up to three matrices side by side (q | k | v, W1 | W3) in one launch.
__global__ __launch_bounds__(256) void dequant_w8_kernel(DequantW8Args a) {
  const int ppr = a.K >> 4;  // pieces per row
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.N * ppr) return;
  const int r = (int)(idx / ppr), pc = (int)(idx - (size_t)r * ppr);
  const uint8_t* src;
  float sc;
  if (r < a.n0) {
    src = a.w[0] + (size_t)r * a.K;
    sc = a.scale[0][r];
  } else if (r < a.n1) {
    src = a.w[1] + (size_t)(r - a.n0) * a.K;
    sc = a.scale[1][r - a.n0];
  } else {
    src = a.w[2] + (size_t)(r - a.n1) * a.K;
    sc = a.scale[2][r - a.n1];
  }
  const u32x4 w = ld16_nt(src + pc * 16);
  u32x4 o[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
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

// One launch; a.g.T must be <= gemv_max_tokens(K) (the activation rows are bf16 as in gemv.hip: the same LDS budget).
hipError_t launch_gemv_w8(const GemvW8Args& a, hipStream_t s) {
  const GemvArgs& g = a.g;
  static int max_blocks = 0, rp_env = -1;
  const int cus = device_cus();
  if (max_blocks == 0) {
    const char* e = getenv("MI_GEMV_MAX_BLOCKS");
    max_blocks = e ? atoi(e) : 2 * cus;  // as gemv.hip
    if (max_blocks <= 0) max_blocks = 2 * cus;
  }
  if (rp_env < 0) {
    const char* e = getenv("MI_GEMV_W8_RP");  // 1 / 2: row pairs per unit at one token (A/B); 0: the rule below
    rp_env = e ? atoi(e) : 0;
  }
  const int npairs = g.mode == GEMV_SWIGLU ? g.N : (g.N + 1) / 2;
  // four-row units only where every wave of a full grid (2 blocks of 4 waves per CU) still gets two of them
  int rp = (g.T == 1 && npairs >= 2 * 2 * 8 * cus) ? 2 : 1;
  if (g.T == 1 && (rp_env == 1 || rp_env == 2)) rp = rp_env;
  const int units = (npairs + rp - 1) / rp;
  // persistent-style grid as launch_gemv: the smallest k units per wave whose block count is a multiple of the CUs and divides
  // the units exactly; otherwise the smallest k that fits max_blocks
  int blocks = 0;
  for (int k = 1; k <= 64 && !blocks; ++k) {
    const int b = (units + 4 * k - 1) / (4 * k);
    if (b <= 4 * cus && b % cus == 0 && b * 4 * k == units && (b <= max_blocks || k == 1)) blocks = b;
  }
  if (!blocks) {
    const int k = (units + 4 * max_blocks - 1) / (4 * max_blocks);
    blocks = (units + 4 * k - 1) / (4 * k);
  }
  if (blocks < 1) blocks = 1;
  int TT = g.T;
  if (TT == 5) TT = 6;
  if (TT == 7) TT = 8;
  const size_t lds = (size_t)TT * g.K * 2 + 4 * TT * sizeof(float) + ((TT > 1 && g.norm_w) ? (size_t)g.K * 2 : 0);
  if (lds > 80 * 1024 && blocks > cus) {  // one such block fits a CU
    const int k = (units + 4 * cus - 1) / (4 * cus);
    blocks = (units + 4 * k - 1) / (4 * k);
  }
  const dim3 grid(blocks);
  switch (g.mode) {
    case GEMV_STORE: return launch_mode<GEMV_STORE>(a, TT, rp, grid, lds, s);
    case GEMV_RESIDUAL: return launch_mode<GEMV_RESIDUAL>(a, TT, rp, grid, lds, s);
    case GEMV_SWIGLU: return launch_mode<GEMV_SWIGLU>(a, TT, rp, grid, lds, s);
    case GEMV_QKV_ROPE: return launch_mode<GEMV_QKV_ROPE>(a, TT, rp, grid, lds, s);
    default: return hipErrorInvalidValue;
  }
}
