// The Mamba2 sequence mixer (include/mistral_hip.h "Mamba2"): the fp32 residual add + RMSNorm, the causal
// depthwise convolution + selective state-space scan, and the gated group RMSNorm.  The two projections of a layer are
// mi_linear shapes (api.hip).  Fixed by the reference's Mamba2 defaults: d_state N = 128, headdim P = 64, d_conv = 4.
//
// mamba_scan_chunk_kernel (L >= 2): one block of four waves per (sequence, head) walks the sequence in chunks of Q = 64 tokens in
// the chunked ("SSD") form - three bf16 MFMA products per chunk - with the state S [P, N] in fp32 MFMA accumulators from chunk to
// chunk.  mamba_step_kernel (L = 1): one block per (sequence, head) on the fp32 VALU, bound by the state's bytes.
// Neither writes the conv state: the B | C columns of a group are read by every head of the group, and the blocks of one grid are
// not ordered, so the three carried rows are moved by mamba_conv_state_kernel, a launch of its own behind the scan.
#include "common.cuh"
#include "kernels.h"

namespace {

typedef ElemBf16 E;

constexpr int MB_N = 128;                   // d_state
constexpr int MB_P = 64;                    // headdim
constexpr int MB_Q = 64;                    // tokens per chunk
constexpr int MB_CH = MB_P + 2 * MB_N;      // channels a head convolves: its x | its group's B | its group's C
constexpr int MB_XS = MB_Q + 8;             // LDS row strides in elements (+16 bytes: rows start on different banks)
constexpr int MB_NS = MB_N + 8;

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float silu_exact(float a) { return a / (1.0f + expf(-a)); }

// column of channel c (0 .. MB_CH) of head h inside the xBC block: x | B | C
__device__ __forceinline__ int head_channel(int c, int h, int g, int I, int G) {
  return c < MB_P ? h * MB_P + c : c < MB_P + MB_N ? I + g * MB_N + (c - MB_P) : I + (G + g) * MB_N + (c - MB_P - MB_N);
}

// raw xBC row of token tg of sequence b (tg < 0: the carried rows of the conv state, [B, 3, Cc])
__device__ __forceinline__ const bf16_t* xbc_row(const bf16_t* zx, int ld, const bf16_t* conv_state, int b, int L, int tg, int I, int Cc) {
  return tg >= 0 ? zx + ((size_t)b * L + tg) * ld + I : conv_state + ((size_t)b * 3 + (3 + tg)) * Cc;
}

struct ScanArgs {
  bf16_t* y;               // [B * L, I]
  const bf16_t* zx;        // [B * L, ld]: z | xBC | dt
  int ld;
  const bf16_t *conv_w, *conv_b;   // [Cc, 4], [Cc]
  const float *dt_bias, *A_log, *Dskip;  // [H]
  const bf16_t* conv_state;        // [B, 3, Cc]
  float* ssm_state;                // [B, H, P, N]
  int L, H, G;
};

// 8 channels (one 16-byte piece at channel c0 of the xBC block) of token tg: bias + four taps in fp32, SiLU; the caller rounds
__device__ __forceinline__ void conv8(const ScanArgs& a, int b, int tg, int c0, int I, int Cc, const float* w4, const float* bias, float out[8]) {
  u32x4 rows[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) rows[j] = ld16(xbc_row(a.zx, a.ld, a.conv_state, b, a.L, tg - 3 + j, I, Cc) + c0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float acc = bias[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(w4[i * 4 + j], (i & 1) ? bf_hi(rows[j][i >> 1]) : bf_lo(rows[j][i >> 1]), acc);
    out[i] = silu_exact(acc);
  }
}

// one operand fragment of the 32x32x16 MFMA: row `row` of a [rows][stride] array, elements k .. k + 7
__device__ __forceinline__ E::x8 frag(const bf16_t* base, int stride, int row, int k) {
  return __builtin_bit_cast(E::x8, *reinterpret_cast<const u32x4*>(base + row * stride + k));
}
// row of accumulator element r of a 32x32 tile in this lane (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

constexpr int SCAN_LDS_BF16 = MB_P * MB_XS + 2 * MB_Q * MB_NS + MB_N * MB_XS + MB_Q * MB_XS;  // xT | Bs (Sb) | Cs | BT | Gs
constexpr int SCAN_LDS_F32 = 2 * MB_Q + MB_CH * 5;                                           // dt | Lambda | taps | bias
constexpr int SCAN_LDS_BYTES = SCAN_LDS_BF16 * 2 + SCAN_LDS_F32 * 4;

// Steps 3 and 4 of the rule for L >= 2 tokens.  grid (H, B), 256 threads.  Wave w owns the 32 x 32 tile (w >> 1, w & 1) of the
// chunk's [Q, Q] and [Q, P] products and the two tiles (w >> 1, 2 (w & 1) + {0, 1}) of the state [P, N].
__global__ __launch_bounds__(256) void mamba_scan_chunk_kernel(ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xT = reinterpret_cast<bf16_t*>(smem);   // [P][XS]: x' transposed (tokens contiguous)
  bf16_t* Bs = xT + MB_P * MB_XS;                 // [Q][NS]: B'; after the chunk's C.B^T product the same bytes hold Sb
  bf16_t* Sb = Bs;                                // [P][NS]: bf16(S_prev)
  bf16_t* Cs = Bs + MB_Q * MB_NS;                 // [Q][NS]: C'
  bf16_t* BT = Cs + MB_Q * MB_NS;                 // [N][XS]: bf16(exp(Lambda_Q - Lambda_s) dt_s B'_s), transposed
  bf16_t* Gs = BT + MB_N * MB_XS;                 // [Q][XS]: bf16((C.B^T) o M)
  float* dtv = reinterpret_cast<float*>(Gs + MB_Q * MB_XS);  // [Q]
  float* lam = dtv + MB_Q;                        // [Q]: inclusive running sum of a inside the chunk
  float* taps = lam + MB_Q;                       // [CH][4]
  float* bias = taps + MB_CH * 4;                 // [CH]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hf = lane >> 5, ql = lane & 31;
  const int h = blockIdx.x, b = blockIdx.y, H = a.H, G = a.G, I = H * MB_P, Cc = I + 2 * G * MB_N, g = h / (H / G), L = a.L;
  const int tb = w >> 1, pb = w & 1;

  for (int c = tid; c < MB_CH; c += 256) {
    const int col = head_channel(c, h, g, I, G);
#pragma unroll
    for (int j = 0; j < 4; ++j) taps[c * 4 + j] = bf_to_f(a.conv_w[(size_t)col * 4 + j]);
    bias[c] = bf_to_f(a.conv_b[col]);
  }
  const float dt_bias = a.dt_bias[h], negA = -expf(a.A_log[h]), Dh = a.Dskip[h];

  float* Sg = a.ssm_state + ((size_t)b * H + h) * MB_P * MB_N;
  f32x16 S[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) S[i][r] = Sg[(tb * 32 + acc_row(r, hf)) * MB_N + (pb * 2 + i) * 32 + ql];

  for (int c0 = 0; c0 < L; c0 += MB_Q) {
    const int q = min(MB_Q, L - c0);  // valid tokens of the chunk; the others run with dt = 0 and zero rows: they change nothing
    if (w == 0) {
      float dt = 0.f;
      if (lane < q) dt = softplus_f(bf_to_f(a.zx[((size_t)b * L + c0 + lane) * a.ld + I + Cc + h]) + dt_bias);
      float s = dt * negA;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(s, o, 64);
        s += lane >= o ? up : 0.f;
      }
      dtv[lane] = dt;
      lam[lane] = s;
    }
    __syncthreads();
    const float lamQ = lam[MB_Q - 1];
    // ---- convolution + SiLU of the chunk's x | B | C columns into LDS: (token, 16-byte piece) items, pieces of a token adjacent
    for (int it = tid; it < MB_Q * (MB_CH / 8); it += 256) {
      const int s = it / (MB_CH / 8), c = (it % (MB_CH / 8)) * 8;
      float v[8];
      if (s < q) {
        conv8(a, b, c0 + s, head_channel(c, h, g, I, G), I, Cc, taps + c * 4, bias + c, v);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
      }
      if (c < MB_P) {
#pragma unroll
        for (int i = 0; i < 8; ++i) xT[(c + i) * MB_XS + s] = E::from_f(v[i]);
      } else if (c < MB_P + MB_N) {
        const int n = c - MB_P;
        const float f = __expf(lamQ - lam[s]) * dtv[s];
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = E::pack2(v[2 * i], v[2 * i + 1]);
        st16(Bs + s * MB_NS + n, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) BT[(n + i) * MB_XS + s] = E::from_f(f * E::round(v[i]));
      } else {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = E::pack2(v[2 * i], v[2 * i + 1]);
        st16(Cs + s * MB_NS + (c - MB_P - MB_N), o);
      }
    }
    __syncthreads();
    // ---- Gs = bf16((C . B^T) o M), M[t, s] = exp(Lambda_t - Lambda_s) dt_s for s <= t; tile (tb, pb) = (token block, source block)
    {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      if (pb <= tb) {
#pragma unroll
        for (int k = 0; k < MB_N; k += 16)
          acc = E::mfma32(frag(Cs, MB_NS, tb * 32 + ql, k + 8 * hf), frag(Bs, MB_NS, pb * 32 + ql, k + 8 * hf), acc);
      }
      const int s = pb * 32 + ql;
      const float lam_s = lam[s], dt_s = dtv[s];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tb * 32 + acc_row(r, hf);
        const float m = s <= t ? __expf(lam[t] - lam_s) * dt_s : 0.f;
        Gs[t * MB_XS + s] = E::from_f(s <= t ? acc[r] * m : 0.f);
      }
    }
    __syncthreads();  // (Bs is dead from here on: its bytes take Sb)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) Sb[(tb * 32 + acc_row(r, hf)) * MB_NS + (pb * 2 + i) * 32 + ql] = E::from_f(S[i][r]);
    // ---- Y1 = Gs . x'   tile (tb, pb) = (token block, channel block), contraction over the chunk's tokens
    f32x16 y1;
#pragma unroll
    for (int r = 0; r < 16; ++r) y1[r] = 0.f;
#pragma unroll
    for (int k = 0; k < MB_Q; k += 16)
      y1 = E::mfma32(frag(Gs, MB_XS, tb * 32 + ql, k + 8 * hf), frag(xT, MB_XS, pb * 32 + ql, k + 8 * hf), y1);
    __syncthreads();
    // ---- Y2 = C' . bf16(S_prev)^T, scaled by exp(Lambda_t) behind the product; + D x'; store
    {
      f32x16 y2;
#pragma unroll
      for (int r = 0; r < 16; ++r) y2[r] = 0.f;
#pragma unroll
      for (int k = 0; k < MB_N; k += 16)
        y2 = E::mfma32(frag(Cs, MB_NS, tb * 32 + ql, k + 8 * hf), frag(Sb, MB_NS, pb * 32 + ql, k + 8 * hf), y2);
      const int p = pb * 32 + ql;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tb * 32 + acc_row(r, hf);
        if (t < q) {
          const float yv = y1[r] + __expf(lam[t]) * y2[r] + Dh * E::to_f(xT[p * MB_XS + t]);
          a.y[((size_t)b * L + c0 + t) * I + h * MB_P + p] = E::from_f(yv);
        }
      }
    }
    // ---- S = exp(Lambda_Q) S_prev + x'^T . BT^T   tiles (tb, 2 pb + i) = (channel block, state block)
    {
      const float decay = __expf(lamQ);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) S[i][r] *= decay;
#pragma unroll
        for (int k = 0; k < MB_Q; k += 16)
          S[i] = E::mfma32(frag(xT, MB_XS, tb * 32 + ql, k + 8 * hf), frag(BT, MB_XS, (pb * 2 + i) * 32 + ql, k + 8 * hf), S[i]);
      }
    }
    __syncthreads();  // the next chunk overwrites every LDS array
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) Sg[(tb * 32 + acc_row(r, hf)) * MB_N + (pb * 2 + i) * 32 + ql] = S[i][r];
}

// Steps 3 and 4 of the rule for ONE token per sequence (decode).  grid (H, B), 256 threads.  The state is read and written once,
// 16 bytes per lane and 1 KiB per wave instruction; the 32 lanes that share a row p reduce its C contraction by shuffles.
__global__ __launch_bounds__(256) void mamba_step_kernel(ScanArgs a) {
  __shared__ float xbc[MB_CH];  // x' | B' | C' as the bf16 values they round to
  const int tid = threadIdx.x;
  const int h = blockIdx.x, b = blockIdx.y, H = a.H, G = a.G, I = H * MB_P, Cc = I + 2 * G * MB_N, g = h / (H / G);
  for (int c = tid; c < MB_CH; c += 256) {
    const int col = head_channel(c, h, g, I, G);
    float acc = bf_to_f(a.conv_b[col]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc = fmaf(bf_to_f(a.conv_w[(size_t)col * 4 + j]), bf_to_f(xbc_row(a.zx, a.ld, a.conv_state, b, 1, j - 3, I, Cc)[col]), acc);
    xbc[c] = E::round(silu_exact(acc));
  }
  const float dt = softplus_f(bf_to_f(a.zx[(size_t)b * a.ld + I + Cc + h]) + a.dt_bias[h]);
  const float decay = __expf(dt * -expf(a.A_log[h])), Dh = a.Dskip[h];
  __syncthreads();
  float* Sg = a.ssm_state + ((size_t)b * H + h) * MB_P * MB_N;
  const int n = (tid & 31) * 4;
  f32x4 Bv, Cv;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Bv[i] = xbc[MB_P + n + i];
    Cv[i] = xbc[MB_P + MB_N + n + i];
  }
  f32x4 s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = *reinterpret_cast<const f32x4*>(Sg + (i * 8 + (tid >> 5)) * MB_N + n);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = i * 8 + (tid >> 5);
    const float dx = dt * xbc[p];
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[i][e] = fmaf(decay, s[i][e], dx * Bv[e]);
      part = fmaf(s[i][e], Cv[e], part);
    }
    *reinterpret_cast<f32x4*>(Sg + p * MB_N + n) = s[i];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((tid & 31) == 0) a.y[(size_t)b * I + h * MB_P + p] = E::from_f(part + Dh * xbc[p]);
  }
}

// The conv state behind a scan over L tokens: the last 3 rows of [old row 0, 1, 2, new row 0 .. L - 1].  One lane per 16-byte
// piece of a sequence's rows; the three rows are in registers before the first store, so the update is in place.
__global__ __launch_bounds__(256) void mamba_conv_state_kernel(bf16_t* conv_state, const bf16_t* zx, int ld, int L, int I, int Cc) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8, b = blockIdx.y;
  if (c >= Cc) return;
  u32x4 v[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = ld16(xbc_row(zx, ld, conv_state, b, L, L - 3 + j, I, Cc) + c);
#pragma unroll
  for (int j = 0; j < 3; ++j) st16(conv_state + ((size_t)b * 3 + j) * Cc + c, v[j]);
}

// Step 1 of the rule: r += float(h) (FIRST: r = float(h), r is not read; no h: r as it is), u = bf16(r rsqrt(mean(r^2) + eps) w).
// One wave per row, the fp32 row in registers between the two passes (rmsnorm_kernel's form).
template <int NP, bool FIRST>  // 8-element pieces per lane: D <= 64 * 8 * NP
__global__ __launch_bounds__(256) void mamba_add_norm_kernel(bf16_t* out, float* res, const bf16_t* hx, const bf16_t* w, int T, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= T) return;
  const int np = D >> 3;
  float* rr = res + (size_t)t * D;
  float v[NP][8];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = min(lane + j * 64, np - 1);
    const bool live = lane + j * 64 < np;
    if (!FIRST) {
      const f32x4 r0 = *reinterpret_cast<const f32x4*>(rr + p * 8), r1 = *reinterpret_cast<const f32x4*>(rr + p * 8 + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[j][i] = r0[i];
        v[j][4 + i] = r1[i];
      }
    }
    if (hx) {
      const u32x4 hv = ld16(hx + (size_t)t * D + p * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[j][2 * i] = (FIRST ? 0.f : v[j][2 * i]) + bf_lo(hv[i]);
        v[j][2 * i + 1] = (FIRST ? 0.f : v[j][2 * i + 1]) + bf_hi(hv[i]);
      }
      if (live) {
        *reinterpret_cast<f32x4*>(rr + p * 8) = f32x4{v[j][0], v[j][1], v[j][2], v[j][3]};
        *reinterpret_cast<f32x4*>(rr + p * 8 + 4) = f32x4{v[j][4], v[j][5], v[j][6], v[j][7]};
      }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(v[j][i], v[j][i], s);
    ss += live ? s : 0.f;
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / sqrtf(ss / (float)D + eps);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + j * 64;
    if (p < np) {
      const u32x4 wv = ld16(w + p * 8);
      u32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = pack_bf2(v[j][2 * i] * inv * bf_lo(wv[i]), v[j][2 * i + 1] * inv * bf_hi(wv[i]));
      st16(out + (size_t)t * D + p * 8, o);
    }
  }
}

// Step 5 of the rule: v = y silu(z), o = bf16(v rsqrt(mean_group(v^2) + eps) w) per group of I / G channels.  One wave per
// (row, group); out may be y.
template <int NP>  // 8-element pieces per lane: I / G <= 64 * 8 * NP
__global__ __launch_bounds__(256) void mamba_gated_norm_kernel(bf16_t* out, const bf16_t* y, const bf16_t* z, int ldz, const bf16_t* w, int T,
                                                               int I, int G, float eps) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= T * G) return;
  const int t = item / G, gs = I / G, c0 = (item % G) * gs, np = gs >> 3;
  float v[NP][8];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = min(lane + j * 64, np - 1);
    const u32x4 yv = ld16(y + (size_t)t * I + c0 + p * 8), zv = ld16(z + (size_t)t * ldz + c0 + p * 8);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[j][2 * i] = bf_lo(yv[i]) * silu_exact(bf_lo(zv[i]));
      v[j][2 * i + 1] = bf_hi(yv[i]) * silu_exact(bf_hi(zv[i]));
      s = fmaf(v[j][2 * i], v[j][2 * i], s);
      s = fmaf(v[j][2 * i + 1], v[j][2 * i + 1], s);
    }
    ss += lane + j * 64 < np ? s : 0.f;
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / sqrtf(ss / (float)gs + eps);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + j * 64;
    if (p < np) {
      const u32x4 wv = ld16(w + c0 + p * 8);
      u32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = pack_bf2(v[j][2 * i] * inv * bf_lo(wv[i]), v[j][2 * i + 1] * inv * bf_hi(wv[i]));
      st16(out + (size_t)t * I + c0 + p * 8, o);
    }
  }
}

}  // namespace

bool mamba_row_ok(int n) { return n > 0 && n % 8 == 0 && n <= MAMBA_MAX_ROW; }

hipError_t launch_mamba_add_norm(void* out, float* residual, const void* h, const void* w, int T, int D, float eps, bool first, hipStream_t s) {
  if (!mamba_row_ok(D) || (first && !h)) return hipErrorInvalidValue;
  const dim3 grid((T + 3) / 4), block(256);
  bf16_t* o = (bf16_t*)out;
  const bf16_t *hx = (const bf16_t*)h, *ww = (const bf16_t*)w;
  if (D <= 4096) {
    if (first) hipLaunchKernelGGL((mamba_add_norm_kernel<8, true>), grid, block, 0, s, o, residual, hx, ww, T, D, eps);
    else hipLaunchKernelGGL((mamba_add_norm_kernel<8, false>), grid, block, 0, s, o, residual, hx, ww, T, D, eps);
  } else {
    if (first) hipLaunchKernelGGL((mamba_add_norm_kernel<16, true>), grid, block, 0, s, o, residual, hx, ww, T, D, eps);
    else hipLaunchKernelGGL((mamba_add_norm_kernel<16, false>), grid, block, 0, s, o, residual, hx, ww, T, D, eps);
  }
  return hipGetLastError();
}

hipError_t launch_mamba_gated_norm(void* out, const void* y, const void* z, int ldz, const void* w, int T, int I, int G, float eps, hipStream_t s) {
  if (G <= 0 || I % G || !mamba_row_ok(I / G) || ldz % 8) return hipErrorInvalidValue;
  const dim3 grid(((size_t)T * G + 3) / 4), block(256);
  if (I / G <= 4096)
    hipLaunchKernelGGL((mamba_gated_norm_kernel<8>), grid, block, 0, s, (bf16_t*)out, (const bf16_t*)y, (const bf16_t*)z, ldz, (const bf16_t*)w, T, I, G, eps);
  else
    hipLaunchKernelGGL((mamba_gated_norm_kernel<16>), grid, block, 0, s, (bf16_t*)out, (const bf16_t*)y, (const bf16_t*)z, ldz, (const bf16_t*)w, T, I, G, eps);
  return hipGetLastError();
}

hipError_t launch_mamba_scan(const MambaScanArgs& m, hipStream_t s) {
  if (m.B <= 0 || m.L <= 0 || m.H <= 0 || m.G <= 0 || m.H % m.G || m.ld % 8 || m.B > 65535) return hipErrorInvalidValue;
  const int I = m.H * MB_P, Cc = I + 2 * m.G * MB_N;
  if (m.ld < I + Cc + m.H) return hipErrorInvalidValue;
  ScanArgs a = {(bf16_t*)m.y, (const bf16_t*)m.zxbcdt, m.ld, (const bf16_t*)m.conv_w, (const bf16_t*)m.conv_b, m.dt_bias, m.A_log, m.Dskip,
                (const bf16_t*)m.conv_state, m.ssm_state, m.L, m.H, m.G};
  const dim3 grid(m.H, m.B), block(256);
  if (m.L == 1) {
    hipLaunchKernelGGL(mamba_step_kernel, grid, block, 0, s, a);
  } else {
    static bool attr_set[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mamba_scan_chunk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         SCAN_LDS_BYTES);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(mamba_scan_chunk_kernel, grid, block, SCAN_LDS_BYTES, s, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mamba_conv_state_kernel, dim3((Cc / 8 + 255) / 256, m.B), block, 0, s, (bf16_t*)m.conv_state, (const bf16_t*)m.zxbcdt, m.ld,
                     m.L, I, Cc);
  return hipGetLastError();
}
