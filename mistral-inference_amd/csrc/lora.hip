// Un-merged LoRA adapters beside a frozen weight (reference lora.py:22-74, LoRALinear.forward :71-74) on a bf16 model:
//
//   t = bf16(A x)                   lora_down   A [r, K], r a multiple of 8 up to 64
//   d = bf16(bf16(B t) * s)         lora_up     B [N, r]
//   y = bf16(bf16(W x) + d)         lora_up     bf16(W x): written before by the tuned GEMV / GEMM in its plain store form
//   out = epilogue(y)               lora_up     y stands where bf16(acc) stands in the plain linears: store, residual + y,
//                                               silu(y1) * y3
//
// Up to three adapters share an input (q|k|v, w1|w3): their A matrices are treated as one stacked [nseg * r, K] matrix and
// every segment of the output uses its own B and its own r-wide slice of t.
//
// Every kernel exists once, with the adapter bank (ABI v9, kernels.h: LoraBank) as the compile-time flag SLOTS.  The flag only
// chooses WHICH rows of A / B a row of the batch runs against (and skips the rows on slot -1); the loops, and with them the
// order of the fp32 operations of one (row, column), are the same source in both modes.
#include "common.cuh"
#include "kernels.h"

namespace {

__device__ __forceinline__ float dot8(u32x4 a, u32x4 b, float acc) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc = dot2_bf16(a[c], b[c], acc);
  return acc;
}

// Entry `seg` of a per-segment kernel argument (a.A, a.B, a.b_stride).  A macro: the select written out in place is what hipcc
// turns into scalar selects on the three kernel-argument loads.  Indexing the array with a runtime value would move it to
// scratch, picking through a reference to it branches around the loads, and a function taking the three values by value
// changes the branch structure of lora_up's bank mode.
#define SEG_PICK(v, seg) ((seg) == 0 ? (v)[0] : ((seg) == 1 ? (v)[1] : (v)[2]))

// One adapter per sequence: the slot of row m.  The address is wave-uniform wherever it is used as a scalar (a token, a row of
// lora_up's walk).  -1: no adapter; anything else is clamped into the bank (the host has refused values outside it).
__device__ __forceinline__ int slot_of_row(const int32_t* tok_seq, const int32_t* seq_slot, int m, int slots) {
  const int b = tok_seq ? tok_seq[m] : m;
  const int sl = seq_slot[b];
  return sl < 0 ? -1 : min(sl, slots - 1);
}
// ... as a wave-uniform scalar.  Without a bank every row is on slot 0: the pointers as given.
template <bool SLOTS>
__device__ __forceinline__ int uniform_slot(LoraBank bank, int m) {
  if constexpr (SLOTS) return __builtin_amdgcn_readfirstlane(slot_of_row(bank.tok_seq, bank.seq_slot, m, bank.slots));
  else return 0;
}

// ---- lora_down, T <= 8 (decode): weight streaming in the GEMV's style.  One wave per row of the stacked A; 16-byte
// non-temporal loads of the row, four per lane in flight; the activation rows come from L2.  Every load is unconditional
// (clamped piece index, contribution selected afterwards): cdna_hip_programming.md ".s-level traps" (c).
// Without a bank the wave takes TT tokens at once.  With one (TT == 1) it takes the token blockIdx.y against the row of that
// token's slot; a slot's rows are read by every token on it: the repeats are L2 hits.
template <int TT, bool SLOTS>
__global__ __launch_bounds__(256) void lora_down_rows_kernel(LoraDownArgs a) {
  static_assert(!SLOTS || TT == 1, "a bank takes one token per wave");
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int R = a.nseg * a.r;
  if (row >= R) return;
  const int seg = row / a.r;
  const bf16_t* A = SEG_PICK(a.A, seg);
  if (A == nullptr) return;  // (wave-uniform) no adapter on this segment
  const int tok = SLOTS ? (int)blockIdx.y : 0;  // the first token of this wave
  const int nt = SLOTS ? 1 : a.T;               // ... and how many there are from it on
  const int slot = uniform_slot<SLOTS>(a.bank, tok);
  if (slot < 0) return;  // (wave-uniform) no adapter on this token
  const bf16_t* arow = A + (size_t)slot * (size_t)a.a_stride + (size_t)(row - seg * a.r) * a.K;
  const int np = a.K >> 3;
  constexpr int U = 4;
  float acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = 0.f;
  for (int p0 = lane; p0 < np + lane; p0 += 64 * U) {  // (p0 - lane < np: the trip count is wave-uniform)
    u32x4 w[U];
    int pc[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      pc[j] = min(p0 + 64 * j, np - 1);
      w[j] = ld16_nt(arow + (size_t)pc[j] * 8);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const bool live = p0 + 64 * j < np;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const u32x4 xv = ld16(a.x + (size_t)(tok + min(t, nt - 1)) * a.ldx + (size_t)pc[j] * 8);
        const float s = dot8(w[j], xv, 0.f);
        acc[t] += live ? s : 0.f;
      }
    }
  }
  float mine = 0.f;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float s = wave_sum(acc[t]);
    mine = (lane == t) ? s : mine;
  }
  if (lane < nt && lane < TT) a.t[(size_t)(tok + lane) * R + row] = f_to_bf(mine);
}

// ---- lora_down, T > 8 (prefill): tiled over T.  One wave forms 16 rows of x by 64 rows of the stacked A with
// v_mfma_f32_16x16x32_bf16; both operands are K-contiguous, so a lane's eight k values of a fragment are ONE 16-byte load
// straight from global memory (x is read once, A - at most 192 rows - stays in L2): no LDS.
// With a bank the tile runs once per distinct slot among the wave's 16 rows: the slot of the first row still pending is taken
// wave-uniformly, the K loop runs against that slot's A rows, the rows on that slot are stored and leave the pending set.  Rows
// of an MFMA do not interact: a row's value is that of a batch that is all on its slot.  Without a bank: one pass, every row.
template <bool SLOTS>
__global__ __launch_bounds__(256) void lora_down_mfma_kernel(LoraDownArgs a) {
  const int lane = threadIdx.x & 63, wid = (int)threadIdx.x >> 6;
  const int m0 = (blockIdx.x * 4 + wid) * 16;
  if (m0 >= a.T) return;
  const int R = a.nseg * a.r;
  const int c0 = blockIdx.y * 64;
  const int fr = lane & 15, fq = lane >> 4;
  const bf16_t* xrow = a.x + (size_t)min(m0 + fr, a.T - 1) * a.ldx;
  int rs = 0;           // slot of row m0 + (lane & 15), whose x this lane loads
  int os[4] = {};       // slots of rows m0 + fq * 4 + j: this lane's outputs
  if constexpr (SLOTS) {
    rs = m0 + fr < a.T ? slot_of_row(a.bank.tok_seq, a.bank.seq_slot, m0 + fr, a.bank.slots) : -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) os[j] = slot_of_row(a.bank.tok_seq, a.bank.seq_slot, min(m0 + fq * 4 + j, a.T - 1), a.bank.slots);
  }
  const bf16_t* brow[4];
  bool has[4], banked[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int n = min(c0 + ct * 16 + fr, R - 1);
    const int seg = n / a.r;
    const bf16_t* A = SEG_PICK(a.A, seg);
    banked[ct] = SLOTS && A != nullptr;
    has[ct] = A != nullptr && c0 + ct * 16 + fr < R;
    brow[ct] = A ? A + (size_t)(n - seg * a.r) * a.K : a.x;  // (a segment without adapter: any readable line, never stored)
  }
  const u32x4 z = {0u, 0u, 0u, 0u};
  unsigned long long pending = SLOTS ? __ballot(rs >= 0) : 1ull;
  while (pending != 0ull) {  // (wave-uniform; every pass retires at least the row it took its slot from)
    const int cur = SLOTS ? __builtin_amdgcn_readlane(rs, __builtin_ctzll(pending)) : 0;
    const size_t so = (size_t)cur * (size_t)a.a_stride;
    f32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.K; k0 += 32) {
      const int k = k0 + fq * 8;
      const bool live = k < a.K;  // K is a multiple of 8, not necessarily of 32
      const int kc = live ? k : 0;
      u32x4 xa = ld16(xrow + kc);
      u32x4 b[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) b[ct] = ld16(brow[ct] + (banked[ct] ? so : (size_t)0) + kc);
      xa = live ? xa : z;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const u32x4 bv = live ? b[ct] : z;
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xa), __builtin_bit_cast(bf16x8, bv), acc[ct], 0, 0, 0);
      }
    }
    // acc[ct][j]: row m0 + fq * 4 + j, column c0 + ct * 16 + fr
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (!has[ct]) continue;
      const int n = c0 + ct * 16 + fr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + fq * 4 + j;
        if (m < a.T && (!SLOTS || os[j] == cur)) a.t[(size_t)m * R + n] = f_to_bf(acc[ct][j]);
      }
    }
    pending = SLOTS ? pending & ~__ballot(rs == cur) : 0ull;
  }
}

// ---- lora_up: one thread per output column, LORA_UP_ROWS rows per block.  The thread keeps its row(s) of B in registers
// (up to 8 pieces of 8; loaded unconditionally with a clamped piece index) and walks the rows of t, which every thread of a
// segment reads at the same address.  Without a bank the B rows are loaded once, before the walk.  With one they are reloaded
// when the slot of the row the walk comes to differs from the previous row's (the slot of a row is the same for the whole
// block); slot -1: d = 0, y = bf16(base + 0), and t is not read.
constexpr int LORA_UP_ROWS = 8;

struct BRow {
  u32x4 p[8];
};
__device__ __forceinline__ BRow load_brow(const bf16_t* row, int rp) {
  BRow b;
#pragma unroll
  for (int i = 0; i < 8; ++i) b.p[i] = ld16(row + (size_t)min(i, rp - 1) * 8);
  return b;
}
// bf16(bf16(B t) * s)   (lora.py:72-73: lora_B(...) is a bf16 tensor, times the python scalar in fp32, rounded again)
__device__ __forceinline__ float lora_delta(const BRow& b, const bf16_t* trow, int rp, float s) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float next = dot8(b.p[i], ld16(trow + min(i, rp - 1) * 8), acc);
    acc = i < rp ? next : acc;
  }
  return bf_round(bf_round(acc) * s);
}
template <bool F32>
__device__ __forceinline__ float base_at(const void* base, size_t i) {
  if constexpr (F32) return reinterpret_cast<const float*>(base)[i];
  else return bf_to_f(reinterpret_cast<const bf16_t*>(base)[i]);
}

template <int EPI, bool F32, bool FAST, bool SLOTS>
__global__ __launch_bounds__(256) void lora_up_kernel(LoraUpArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const int m0 = blockIdx.y * LORA_UP_ROWS;
  const int m1 = min(m0 + LORA_UP_ROWS, a.T);
  const int rp = a.r >> 3;
  const int ldt = a.nseg * a.r;
  const bf16_t* dummy = a.t;  // a readable line for the segments without adapter
  int loaded = -1;  // (SLOTS) the slot the B registers hold
  if constexpr (EPI == MI_EPI_SWIGLU) {
    const bool h1 = a.B[0] != nullptr, h3 = a.B[1] != nullptr;
    BRow b1 = {}, b3 = {};
    if constexpr (!SLOTS) {
      b1 = load_brow(h1 ? a.B[0] + (size_t)n * a.r : dummy, rp);
      b3 = load_brow(h3 ? a.B[1] + (size_t)n * a.r : dummy, rp);
    }
    for (int m = m0; m < m1; ++m) {
      const int slot = uniform_slot<SLOTS>(a.bank, m);
      if constexpr (SLOTS) {
        if (slot >= 0 && slot != loaded) {
          b1 = load_brow(h1 ? a.B[0] + (size_t)slot * (size_t)a.b_stride[0] + (size_t)n * a.r : dummy, rp);
          b3 = load_brow(h3 ? a.B[1] + (size_t)slot * (size_t)a.b_stride[1] + (size_t)n * a.r : dummy, rp);
          loaded = slot;
        }
      }
      float d1 = 0.f, d3 = 0.f;
      if (slot >= 0) {
        const bf16_t* trow = a.t + (size_t)m * ldt;
        d1 = h1 ? lora_delta(b1, trow, rp, a.scaling) : 0.f;
        d3 = h3 ? lora_delta(b3, trow + a.r, rp, a.scaling) : 0.f;
      }
      const float y1 = bf_round(base_at<F32>(a.base, (size_t)m * a.ldb + n) + d1);
      const float y3 = bf_round(base_at<F32>(a.base, (size_t)m * a.ldb + a.N + n) + d3);
      a.out[(size_t)m * a.ldo + n] = f_to_bf(FAST ? swiglu_bf_fast(y1, y3) : swiglu_bf(y1, y3));
    }
  } else {
    const int seg = n < a.n0 ? 0 : (n < a.n1 ? 1 : 2);
    const int start = seg == 0 ? 0 : (seg == 1 ? a.n0 : a.n1);
    const bf16_t* B = SEG_PICK(a.B, seg);
    const size_t stride = (size_t)SEG_PICK(a.b_stride, seg);
    const bool has = B != nullptr;
    BRow b = {};
    if constexpr (!SLOTS) b = load_brow(has ? B + (size_t)(n - start) * a.r : dummy, rp);
    for (int m = m0; m < m1; ++m) {
      const int slot = uniform_slot<SLOTS>(a.bank, m);
      if constexpr (SLOTS) {
        if (slot >= 0 && slot != loaded) {
          b = load_brow(has ? B + (size_t)slot * stride + (size_t)(n - start) * a.r : dummy, rp);
          loaded = slot;
        }
      }
      float d = 0.f;
      if (slot >= 0 && has) d = lora_delta(b, a.t + (size_t)m * ldt + seg * a.r, rp, a.scaling);
      const float y = bf_round(base_at<F32>(a.base, (size_t)m * a.ldb + n) + d);
      if constexpr (EPI == MI_EPI_RESIDUAL)
        a.out[(size_t)m * a.ldo + n] = f_to_bf(bf_to_f(a.residual[(size_t)m * a.ldo + n]) + y);
      else
        a.out[(size_t)m * a.ldo + n] = f_to_bf(y);
    }
  }
}

template <int EPI, bool SLOTS>
hipError_t launch_up_epi(const LoraUpArgs& a, dim3 grid, hipStream_t s) {
  if (a.base_f32) {
    if (a.fast_silu) hipLaunchKernelGGL((lora_up_kernel<EPI, true, true, SLOTS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_up_kernel<EPI, true, false, SLOTS>), grid, dim3(256), 0, s, a);
  } else {
    if (a.fast_silu) hipLaunchKernelGGL((lora_up_kernel<EPI, false, true, SLOTS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_up_kernel<EPI, false, false, SLOTS>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}
template <bool SLOTS>
hipError_t launch_up(const LoraUpArgs& a, dim3 grid, hipStream_t s) {
  switch (a.epi) {
    case MI_EPI_STORE: return launch_up_epi<MI_EPI_STORE, SLOTS>(a, grid, s);
    case MI_EPI_RESIDUAL: return launch_up_epi<MI_EPI_RESIDUAL, SLOTS>(a, grid, s);
    case MI_EPI_SWIGLU: return launch_up_epi<MI_EPI_SWIGLU, SLOTS>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_lora_down(const LoraDownArgs& a, hipStream_t s) {
  if (a.T <= 0 || a.K <= 0 || a.K % 8 || a.ldx % 8 || a.nseg < 1 || a.nseg > 3 || !lora_rank_ok(a.r)) return hipErrorInvalidValue;
  const bool slots = a.bank.seq_slot != nullptr;  // adapter bank: one slot per sequence
  if (slots && (a.bank.slots < 1 || a.a_stride < (int64_t)a.r * a.K)) return hipErrorInvalidValue;
  const int R = a.nseg * a.r;
  const dim3 tiles((unsigned)((a.T + 63) / 64), (unsigned)((R + 63) / 64)), rows((unsigned)((R + 3) / 4));
  if (a.T > GEMV_MAX_T) {
    if (slots) hipLaunchKernelGGL((lora_down_mfma_kernel<true>), tiles, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_down_mfma_kernel<false>), tiles, dim3(256), 0, s, a);
  } else if (slots) {
    hipLaunchKernelGGL((lora_down_rows_kernel<1, true>), dim3(rows.x, (unsigned)a.T), dim3(256), 0, s, a);
  } else {
    switch (a.T) {
      case 1: hipLaunchKernelGGL((lora_down_rows_kernel<1, false>), rows, dim3(256), 0, s, a); break;
      case 2: hipLaunchKernelGGL((lora_down_rows_kernel<2, false>), rows, dim3(256), 0, s, a); break;
      case 3:
      case 4: hipLaunchKernelGGL((lora_down_rows_kernel<4, false>), rows, dim3(256), 0, s, a); break;
      default: hipLaunchKernelGGL((lora_down_rows_kernel<8, false>), rows, dim3(256), 0, s, a); break;
    }
  }
  return hipGetLastError();
}

hipError_t launch_lora_up(const LoraUpArgs& a, hipStream_t s) {
  if (a.T <= 0 || a.N <= 0 || a.nseg < 1 || a.nseg > 3 || !lora_rank_ok(a.r)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.N + 255) / 256), (unsigned)((a.T + LORA_UP_ROWS - 1) / LORA_UP_ROWS));
  if (a.bank.seq_slot == nullptr) return launch_up<false>(a, grid, s);
  if (a.bank.slots < 1) return hipErrorInvalidValue;
  return launch_up<true>(a, grid, s);
}
