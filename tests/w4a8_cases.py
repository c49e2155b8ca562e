"""The MXFP4 x FP8 prefill GEMM (`_hip.linear_w4a8`, `_hip.qkv_rope_w4a8`: csrc/gemm256_w4a8.hip behind the per-token activation
quantiser) on inputs for which the route is LOSSLESS and every fp32 sum exact in any order, so that the device must be bit-equal to
one fp64 reference with an explicit rounding at every rounding point (helpers for test_w4a8_host.py and test_gpu_w4a8.py; no test
functions here).  Built from linear_cases.py (`_x`, `_signs`, `guard`, the rope table CS, `_rope64`), w8a8_cases.py (shapes, segments,
positions) and mxfp4_cases.py (`dequant_f64`, the independent statement of the format).

Weights are given as the checkpoint gives them: code bytes [n, K / 2] and e8m0 scale bytes [n, K / 32].
  codes    uniform random bytes
  scales   127 + base(row) + U{-3..3} per block; base walks through BASES = (-8, 3, -2, 8, 0) with the row number counted across the
           segments (+ 2 per segment), so that neighbouring blocks, rows, K tiles and segments all carry different scales.  q|k|v cases
           step base once per (re, im) PAIR of rows: RoPE adds the two outputs of a pair in fp32, and 16 binades between them would
           not leave that sum exact (the rows of a pair still differ in every block's U).
  x        w8a8_cases' devices, exact in e4m3 under the row's power-of-two scale: "plain" has one +-1 per 8-element piece (piece 0:
           +-2 at few pieces) and doubles the odd rows; "round" has x[:, 0] = 8, x[:, 1] = 1 in piece 0.  Neighbouring rows are on
           different activation scales in the plain family (and in SwiGLU's, which halves the odd rows).
  SwiGLU   keeps the a = 128 +- noise device, restated for block-scaled weights: x[:, 0] = 256 alone in piece 0 (256 and 1 are both
           e4m3 values under the row scale 1), W1's rows have base in (-7, -6, -5) and block 0 of W1 carries scale byte 124 / 125 by
           row with the code at k = 0 set to 4.0 / 2.0, i.e. W1[n, 0] = 0.5: a = 128 +- noise (64 on the halved rows), where
           bf16(silu(a)) == a.  W3 is as every other matrix.
  res      r * 2^(e(n) - 8), r an integer in [-7, 7], e(n) the binade of the median |y| of column n: a few bf16 half-ulps of y, the
           regime in which bf16(res + bf16(y)) != bf16(res + y) shows (linear_cases' res in [-7, 7] on 256 < |y| < 1024).
  q|k|v    RoPE with linear_cases' dyadic (cos, sin) table and w8a8_cases' positions.

conditions() asserts for every case: x round-trips through quantize_rows / dequantize bit for bit; per output, sum_k |w x| is below
2^24 units of the smallest product of that output (0.5 * the row's smallest block scale * the token's smallest |x|), so the fp32 sum
is exact in any order; 24 <= a <= 256 and fewer than 15 % zeros in b (SwiGLU); in the round family, as in linear_cases', at least a
quarter of the sums are not bf16 values and (RESIDUAL) bf16(res + bf16(y)) != bf16(res + y) in at least 5 % (the plain family's sums
are not bf16 values either, in a fifth of the outputs at K = 128 and more above: random codes leave no exact family); RESIDUAL: res +
bf16(y) exact in fp32; q|k|v: both RoPE sums exact in fp32 (below 2^24 units of the pair's smaller unit / 4).  linear_cases'
share of exact TIES among 256 < |y| < 1024 has no counterpart: these sums are not integers.  The figure measured instead is the share of
sums with exactly nine significant bits (a tie of the first rounding); it is reported, not bounded.

emulate(case, mutant): the route on the CPU - quantize_rows of x, the codes taken apart low nibble first, K slices of 128 in blocks of
32 with the block's scale, acc * s_x in fp32, the epilogue, stores inside the valid rows and columns of the guarded buffer - bit-equal
to the reference without a mutant; each single-fault mutant of MUTANTS must change at least one case of every epilogue group it
applies to (test_w4a8_host.py)."""
import functools

import torch

import linear_cases as lc
import mxfp4_cases as mc
import w8a8_cases as w8
from linear_cases import BF, QKV, RESIDUAL, STORE, SWIGLU

MS, KS, SEGS, SWIGLU_NS, QKV_HEADS = w8.MS, w8.KS, w8.SEGS, w8.SWIGLU_NS, w8.QKV_HEADS
MIN_M, K_MOD = 256, 128             # the route's applicability (kernels.h gemm256_w4a8_applicable)
BASES = (-8, 3, -2, 8, 0)
W1_BASES = (-7, -6, -5)
E2M1 = torch.tensor(mc.E2M1 + [-v for v in mc.E2M1], dtype=torch.float32)


def _quant():
    from mistral_inference import quant
    return quant


class Case(lc.Case):
    def __init__(self, M, K, segs, epi, fam, heads=None):
        super().__init__(f"m{M}k{K}n{'+'.join(map(str, segs))}-{epi}{'-r' if fam == 'round' else ''}", M, K, segs, epi, "w4a8", fam=fam,
                         qkv=(heads + (None, False)) if heads else None)

    @property
    def key(self):
        return (self.M, self.K, self.segs, self.epi, self.fam, self.qkv)


def all_cases():
    """M in MS, K in KS (1, 2, 3 and 9 K tiles), the segments of w8a8_cases.SEGS, SwiGLU N in SWIGLU_NS, heads (1, 1) and (2, 1)."""
    out = []
    for i, segs in enumerate(SEGS):
        for j, M in enumerate(MS):
            K = KS[(i + j) % len(KS)]
            out.append(Case(M, K, segs, STORE, "plain"))
            out.append(Case(M, K, segs, RESIDUAL, "plain"))
            out.append(Case(M, KS[(i + j + 1) % len(KS)], segs, RESIDUAL, "round"))
    for i, N in enumerate(SWIGLU_NS):
        for j, M in enumerate(MS):
            out.append(Case(M, KS[(i + j) % len(KS)], (N,), SWIGLU, "plain"))
            out.append(Case(M, KS[(i + j + 2) % len(KS)], (N,), SWIGLU, "round"))
    for i, (H, Hkv) in enumerate(QKV_HEADS):
        segs = (H * 128, Hkv * 128, Hkv * 128)
        for j, M in enumerate((256, 300, 513)):
            out.append(Case(M, KS[(i + j) % len(KS)], segs, QKV, "round", heads=(H, Hkv)))
        out.append(Case(257, KS[(i + 3) % len(KS)], segs, QKV, "plain", heads=(H, Hkv)))
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def codes_of(packed):
    """[n, K] code numbers 0 .. 15, the low nibble at the even k."""
    return torch.stack((packed & 15, packed >> 4), dim=2).reshape(packed.shape[0], -1)


def pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).contiguous()


def _matrix(n, K, first, seg, g, pairs, w1=False):
    packed = torch.randint(0, 256, (n, K // 2), generator=g, dtype=torch.uint8)
    row = first + torch.arange(n)
    if w1:
        base = torch.tensor(W1_BASES)[row % len(W1_BASES)]
    else:
        base = torch.tensor(BASES)[((row // 2 if pairs else row) + 2 * seg) % len(BASES)]
    scale = 127 + base[:, None] + torch.randint(-3, 4, (n, K // 32), generator=g)
    if w1:  # W1[n, 0] = 0.5: scale byte 124 with code 4.0 (6), or 125 with code 2.0 (4), by row
        scale[:, 0] = 124 + row % 2
        c = codes_of(packed)
        c[:, 0] = torch.where(row % 2 == 0, 6, 4).to(torch.uint8)
        packed = pack(c)
    return packed, scale.to(torch.uint8).contiguous()


def _dequant32(packed, scale):
    """fp32 [n, K]: exact (an e2m1 value times a power of two)."""
    v = E2M1[codes_of(packed).long()]
    sc = torch.pow(torch.tensor(2.0), scale.float() - 127.0)
    return (v.reshape(v.shape[0], -1, 32) * sc[:, :, None]).reshape(v.shape[0], -1)


@functools.lru_cache(maxsize=8)
def _inputs(key):
    M, K, segs, epi, fam, qkv = key
    case = Case(M, K, segs, epi, fam, heads=qkv[:2] if qkv else None)
    g = torch.Generator().manual_seed(lc._seed(case) + 41)
    x = lc._x(M, K, g, "round" if fam == "round" else epi == SWIGLU, M * sum(segs) < 4096)
    if epi == SWIGLU:
        x[:, 0] = 256.0
        if fam == "round":
            x[:, 1] = 0.0          # (piece 0 holds the carrier alone, as in the plain device: a stays 128 +- noise)
        else:
            x[1::2] *= 0.5
    elif fam == "plain":
        x[1::2] *= 2.0
    rows = [case.N, case.N] if epi == SWIGLU else list(segs)
    mats, first = [], 0
    for i, n in enumerate(rows):
        mats.append(_matrix(n, K, 0 if epi == SWIGLU else first, i, g, epi == QKV, w1=(epi == SWIGLU and i == 0)))
        first += n
    inp = lc.Inputs(x=x.to(BF), codes=[m[0] for m in mats], scales=[m[1] for m in mats], res=None)
    inp.w = [mc.dequant_f64(c, s) for c, s in mats]               # fp64, the reference's operands
    if epi == RESIDUAL:
        y = torch.cat(exact_sums(inp), dim=1)
        e = torch.floor(torch.log2(y.abs().median(dim=0).values.clamp_min(2.0 ** -100)))
        r = torch.randint(-7, 8, (M, case.N), generator=g).double()
        inp.res = (r * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8)[None, :]).to(BF)
    if epi == QKV:
        idx = (7 * torch.arange(lc.ROPE_LEN)[:, None] + 3 * torch.arange(lc.HEAD // 2)[None, :]) % len(lc.CS)
        inp.rope_cs = torch.tensor(lc.CS, dtype=torch.float32)[idx].contiguous()
        inp.tok_pos = w8.positions(M)
    return inp


def inputs(case):
    return _inputs(case.key)


def exact_sums(inp):
    """fp64 [M, rows] per weight matrix: exact (conditions())."""
    x = inp.x.double()
    return [x @ w.T for w in inp.w]


# --------------------------------------------------------------------------------------------------------------- reference
@functools.lru_cache(maxsize=8)
def _reference(key):
    M, K, segs, epi, fam, qkv = key
    inp = _inputs(key)
    rd = lambda v: v.to(BF).double()  # noqa: E731
    sums = exact_sums(inp)
    if epi == SWIGLU:
        a, b = rd(sums[0]), rd(sums[1])
        s = rd(a / (1.0 + torch.exp(-a)))
        assert torch.equal(s, a), key
        return (s * b).to(BF)
    y = rd(torch.cat(sums, dim=1))
    if epi == STORE:
        return y.to(BF)
    if epi == RESIDUAL:
        return (inp.res.double() + y).to(BF)
    H, Hkv = qkv[:2]
    n1 = (H + Hkv) * lc.HEAD
    cs = inp.rope_cs.double()[inp.tok_pos.long()]
    rot = lc._rope64(y[:, :n1].reshape(M, -1, lc.HEAD // 2, 2), cs[:, None])
    return torch.cat((rot.reshape(M, n1), y[:, n1:]), dim=1).to(BF)


def reference(case):
    """[M, N] bf16: fp64 sums, then .to(bfloat16) at every rounding point (linear_cases.reference's chain)."""
    return _reference(case.key)


def expected(case):
    """The reference inside its guard buffer [M + 4, N + 8] of SENT (two rows down, ldo = N + 8)."""
    ref = reference(case)
    buf, view = lc.guard(case.M, ref.shape[1], BF)
    view.copy_(ref)
    return buf


def round_trips(case):
    q, inp = _quant(), inputs(case)
    return torch.equal(q.dequantize(*q.quantize_rows(inp.x)), inp.x)


def _nine_bits(y):
    """sums whose magnitude has exactly nine significant bits: exact ties of the rounding to bf16"""
    m, _ = torch.frexp(y)
    v = m.abs() * 512.0
    return (v == v.floor()) & (v.floor() % 2 == 1)


def conditions(case):
    """Asserts the generator's conditions (module docstring) and returns the measured figures."""
    inp = inputs(case)
    assert round_trips(case), case
    x = inp.x.double()
    xmin = torch.where(x == 0, torch.tensor(float("inf"), dtype=torch.float64), x.abs()).min(dim=1).values      # [M]
    fig, units = {}, []
    for w, s in zip(inp.w, inp.scales):
        wunit = 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double().min(dim=1).values - 127.0)  # [n]
        unit = xmin[:, None] * wunit[None, :]
        fig["bound"] = max(fig.get("bound", 0.0), float(((x.abs() @ w.abs().T) / unit).max()))
        units.append(unit)
    assert fig["bound"] < 2 ** 24, (case, fig)
    assert all(int(s.min()) >= 3 and int(s.max()) < 255 for s in inp.scales), case
    sums = exact_sums(inp)
    if case.epi == SWIGLU:
        a, b = sums
        fig["a"] = (float(a.min()), float(a.max()))
        fig["zeros"] = float((b == 0).double().mean())
        assert 24 <= a.min() and a.max() <= 256 and fig["zeros"] < 0.15, (case, fig)
        y = b
    else:
        y = torch.cat(sums, dim=1)
    fig["inexact"], fig["ties"] = float(lc._inexact(y, BF).double().mean()), float(_nine_bits(y).double().mean())
    if case.fam == "round":
        assert fig["inexact"] >= 0.25, (case, fig)
    if case.epi == RESIDUAL:
        r, yb = inp.res.double(), y.to(BF).double()
        fig["double"] = float(((r + yb).to(BF) != (r + y).to(BF)).double().mean())
        assert case.fam != "round" or fig["double"] >= 0.05, (case, fig)
        assert torch.equal((r + yb).float().double(), r + yb), case                     # the kernel's fp32 sum is exact
    if case.epi == QKV:
        H, Hkv = case.qkv[:2]
        n1 = (H + Hkv) * lc.HEAD
        yb, u = y.to(BF).double()[:, :n1], torch.cat(units, dim=1)[:, :n1]
        span = (1.5 * (yb[:, 0::2].abs() + yb[:, 1::2].abs())) / (torch.minimum(u[:, 0::2], u[:, 1::2]) / 4)
        fig["rope_span"] = float(span.max())
        assert fig["rope_span"] < 2 ** 24, (case, fig)
        pos = inp.tok_pos
        assert int(pos.max()) < lc.ROPE_LEN and len(set(pos.tolist())) > 8 and len({(int(p) % len(lc.CS)) for p in pos[:8]}) == 8
    return fig


# --------------------------------------------------------------------------------------------------------------- emulation
MUTANTS = ["nibbles_exchanged", "scale_next_block", "scale_next_tile", "scale_neighbour_row", "scale_wrong_segment", "scales_all_127",
           "sx_neighbour_row", "kslice_first", "kslice_middle", "kslice_last", "w1_w3_exchanged", "row_past_written", "col_past_written"]


def applies(case, mutant):
    if mutant == "w1_w3_exchanged":
        return case.epi == SWIGLU
    if mutant == "scale_wrong_segment":
        return case.epi != SWIGLU and len(case.segs) > 1
    if mutant == "scale_next_tile":
        return case.K >= 2 * K_MOD
    if mutant == "kslice_middle":
        return case.K >= 3 * K_MOD
    return True


def emulate(case, mutant=None):
    """The guarded buffer the route writes (module docstring)."""
    q, inp = _quant(), inputs(case)
    M, K, N = case.M, case.K, case.N
    xq, sx = q.quantize_rows(inp.x)
    xq = xq.float()
    codes, scales = list(inp.codes), [s.clone() for s in inp.scales]
    if mutant == "w1_w3_exchanged":
        codes, scales = codes[::-1], scales[::-1]
    if mutant == "nibbles_exchanged":
        codes = [(c >> 4) | ((c & 15) << 4) for c in codes]
    if mutant == "scale_wrong_segment":   # segment 1's rows scaled by segment 0's matrix at the same local index
        scales[1] = scales[0][torch.arange(scales[1].shape[0]).clamp_max(scales[0].shape[0] - 1)]
    if mutant == "scale_next_block":
        scales = [torch.roll(s, -1, dims=1) for s in scales]
    if mutant == "scale_next_tile":
        scales = [torch.roll(s, -(K_MOD // 32), dims=1) for s in scales]
    if mutant == "scale_neighbour_row":
        scales = [s[(torch.arange(s.shape[0]) ^ 1).clamp_max(s.shape[0] - 1)] for s in scales]
    if mutant == "scales_all_127":
        scales = [torch.full_like(s, 127) for s in scales]
    if mutant == "sx_neighbour_row":
        sx = sx[(torch.arange(M) ^ 1).clamp_max(M - 1)]
    nk = K // K_MOD
    skip = {"kslice_first": 0, "kslice_middle": nk // 2, "kslice_last": nk - 1}.get(mutant)
    accs = []
    for c, s in zip(codes, scales):
        w = _dequant32(c, s)
        acc = torch.zeros(M, w.shape[0], dtype=torch.float32)
        for t in range(nk):
            if t == skip:
                continue
            for f in range(K_MOD // 32):   # one MFMA: four lane groups, each one MX block under its scale byte
                k0 = t * K_MOD + f * 32
                acc += xq[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
        accs.append(acc * sx[:, None])
    bf = lambda v: v.to(BF).float()  # noqa: E731
    if case.epi == SWIGLU:
        a, b = bf(accs[0]), bf(accs[1])
        out = (bf(a / (1.0 + torch.exp(-a))) * b).to(BF)
    else:
        y = bf(torch.cat(accs, dim=1))
        if case.epi == RESIDUAL:
            out = (inp.res.float() + y).to(BF)
        elif case.epi == QKV:
            H, Hkv = case.qkv[:2]
            n1 = (H + Hkv) * lc.HEAD
            cs = inp.rope_cs[inp.tok_pos.long()]
            p = y[:, :n1].reshape(M, -1, lc.HEAD // 2, 2)
            c, s_ = cs[:, None, :, 0], cs[:, None, :, 1]
            rot = torch.stack((p[..., 0] * c - p[..., 1] * s_, p[..., 0] * s_ + p[..., 1] * c), dim=-1)
            out = torch.cat((rot.reshape(M, n1), y[:, n1:]), dim=1).to(BF)
        else:
            out = y.to(BF)
    buf, view = lc.guard(M, N, BF)
    view.copy_(out)
    if mutant == "row_past_written":      # the clamped A row of a ragged tile stored as row M
        buf[2 + M, :N] = out[M - 1]
    if mutant == "col_past_written":
        buf[2:2 + M, N] = out[:, N - 1]
    return buf
