"""The FP8 prefill GEMM (`_hip.linear_w8a8`, `_hip.qkv_rope_w8a8`: csrc/gemm256_w8a8.hip behind the per-token activation quantiser)
on inputs that e4m3 holds EXACTLY under the power-of-two row scales of `quant.quantize_rows`, so that both quantisations are
lossless, every contraction is an exact integer sum and the result must be bit-equal to one fp64 reference with an explicit
rounding at every rounding point (helpers for test_w8a8_host.py and test_gpu_w8a8.py; no test functions here).

The families are tests/linear_cases.py's, built from its helpers (`_x`, `_signs`, `exact_sums`, `guard`, its rope table CS):

  plain    W dense +-1, x pieces with one +-1 (piece 0: +-2 at few pieces).  STORE / RESIDUAL / q|k|v cases double the odd rows of x
           and the odd rows of W (x in +-{1, 2, 4}, W in +-{1, 2}), so that neighbouring rows of either operand carry DIFFERENT
           scales: a kernel that reads s_x or s_w of the row beside (or of another segment) computes other values.
  round    linear_cases' rounding-point family with the lift c restricted to the multiples of 8 in [56, 104] - 56, 64, .. 104 are
           e4m3 values under the row's scale (c = 56: scale 2^-3, code 448; else 2^-2), the integers between them are not.
           W[n, 1] = n % 2, x[:, 0] = 8, x[:, 1] = 1 as there: 256 < |y| < 1024, sums that are not bf16 values, exact ties.
  arb      every epilogue.  With power-of-two scales bf16(acc) * s == bf16(acc * s), so a kernel that scales AFTER rounding cannot
           be seen by the two families above.  Here the weights are given as codes and scales directly: the round family's codes
           with scale 3 * 2^e in place of 2^e (a checkpoint made elsewhere: positive, finite, not a power of two; SwiGLU: W3's
           scales only, so that a stays 128 +- noise).  Every product acc * (s_x * s_w) is still exact in fp32 (3 * |acc| < 2^24),
           the reference is the same fp64 chain.

SwiGLU keeps linear_cases' device (x[:, 0] = 8 alone in piece 0, W1[:, 0] = 16: a = 128 +- noise, where bf16(silu(a)) == a); its
plain cases HALVE the odd rows of x (x in +-{0.5, 1, 4, 8}: a = 64 +- noise / 2 there, still above 24, a and b multiples of 1/2 that
bf16 holds), so that the SwiGLU instantiation too sees neighbouring activation rows on different scales.
q|k|v: RoPE with linear_cases' dyadic (cos, sin) table, the entry of (position, pair) number (7 pos + 3 pair) % 9, positions
(POSITIONS[t % 8] + 7 * (t // 8)) % 48 - bf16(y0) c - bf16(y1) s is exact in fp32 and rounds once.

conditions() is linear_cases.conditions itself, run on these inputs (its `inputs` swapped for ours while it runs), plus: every
operand of the plain and round families round-trips through quantize_rows / dequantize bit for bit, and sum |w x| < 2^24 / 2^9
(the contraction runs on the codes, i.e. on values scaled by up to 2^5 * 2^4).

emulate(case, mutant): the route on the CPU - quantize_rows of x, the weight codes, K slices of 128 bytes in fragments of 32,
acc * (s_x * s_w) in fp32, the epilogue, stores inside the valid rows and columns of the guarded buffer - bit-equal to the
reference without a mutant; each single-fault mutant of MUTANTS must change at least one case (test_w8a8_host.py)."""
import functools

import torch

import linear_cases as lc
from linear_cases import BF, QKV, RESIDUAL, STORE, SWIGLU

MS = [256, 257, 300, 512, 513]
KS = [128, 256, 384, 1152]
SEGS = [(37,), (64,), (256,), (264,), (12, 13, 12), (128, 64, 64)]
SWIGLU_NS = [64, 128, 136]
QKV_HEADS = [(1, 1), (2, 1)]        # (H, Hkv): 384 and 512 columns, heads of 128
MIN_M, K_MOD = 256, 128             # the route's applicability (kernels.h gemm256_w8a8_applicable)


def _quant():
    from mistral_inference import quant
    return quant


class Case(lc.Case):
    def __init__(self, M, K, segs, epi, fam, heads=None):
        tag = {"plain": "", "round": "-r", "arb": "-arb"}[fam]
        super().__init__(f"m{M}k{K}n{'+'.join(map(str, segs))}-{epi}{tag}", M, K, segs, epi, "w8a8", fam="round" if fam == "arb" else fam,
                         qkv=(heads + (None, False)) if heads else None)
        self.family = fam            # (lc.Case.fam stays one of linear_cases' two: arb is the round family on other scales)

    @property
    def key(self):
        return (self.M, self.K, self.segs, self.epi, self.family, self.qkv)


def all_cases():
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
    for j, (M, segs) in enumerate(((256, (64,)), (300, (12, 13, 12)), (513, (264,)), (257, (37,)))):
        out.append(Case(M, KS[j], segs, STORE, "arb"))
        out.append(Case(M, KS[(j + 1) % len(KS)], segs, RESIDUAL, "arb"))
    for j, (M, N) in enumerate(((256, 64), (300, 136), (513, 128))):
        out.append(Case(M, KS[(j + 2) % len(KS)], (N,), SWIGLU, "arb"))
    out.append(Case(300, 384, (128, 128, 128), QKV, "arb", heads=(1, 1)))
    out.append(Case(513, 128, (256, 128, 128), QKV, "arb", heads=(2, 1)))
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def lift8(w, first=0):
    """linear_cases._lift with c in {56, 64, .., 104}: column 0 = +-c, column 1 = 0 / 1 by row."""
    n = first + torch.arange(w.shape[0])
    w[:, 0] = (56 + 8 * ((17 * n + 5) % 7)).float() * (1 - 2 * ((n // 2) % 2)).float()
    w[:, 1] = (n % 2).float()


def positions(M):
    t = torch.arange(M)
    return ((torch.tensor(lc.POSITIONS)[t % 8] + 7 * (t // 8)) % lc.ROPE_LEN).to(torch.int32)


@functools.lru_cache(maxsize=8)
def _inputs(key):
    M, K, segs, epi, fam, qkv = key
    case = Case(M, K, segs, epi, fam, heads=qkv[:2] if qkv else None)
    g = torch.Generator().manual_seed(lc._seed(case) + (29 if fam == "arb" else 0))
    lifted = fam != "plain"
    x = lc._x(M, K, g, "round" if lifted else epi == SWIGLU, M * sum(segs) < 4096)
    rows = [case.N, case.N] if epi == SWIGLU else list(segs)
    w = [lc._signs((n, K), g) for n in rows]
    if epi == SWIGLU:
        w[0][:, 0] = 16.0
        if lifted:
            lift8(w[1])
    elif lifted:
        for i, wi in enumerate(w):
            lift8(wi, sum(rows[:i]))
    if epi == SWIGLU and not lifted:   # neighbouring activation rows on different scales, a kept inside [24, 256]
        x[1::2] *= 0.5
    elif not lifted:  # neighbouring rows of either operand on different scales
        x[1::2] *= 2.0
        first = 0
        for wi in w:
            wi[(first + torch.arange(wi.shape[0])) % 2 == 1] *= 2.0
            first += wi.shape[0]
    inp = lc.Inputs(x=x.to(BF), w=[wi.to(BF) for wi in w], res=None)
    q = _quant()
    inp.wq, inp.ws = zip(*[q.quantize_rows(wi) for wi in inp.w])      # codes (float8_e4m3fn) and fp32 row scales
    inp.ws = [s.contiguous() for s in inp.ws]
    if fam == "arb":  # the same codes under scales that are not powers of two; the real-valued weights follow
        inp.ws = [(s * (1.0 if epi == SWIGLU and i == 0 else 3.0)).contiguous() for i, s in enumerate(inp.ws)]
        inp.w = [(c.float() * s[:, None]) for c, s in zip(inp.wq, inp.ws)]
        assert all(bool((wi.double() == c.double() * s.double()[:, None]).all()) for wi, c, s in zip(inp.w, inp.wq, inp.ws))
    if epi == RESIDUAL:
        y = lc.exact_sums(inp)[0]
        r = 7 if lifted else min(64, 256 - int(y.abs().max()))
        assert r >= 1, (key, r)
        inp.res = torch.randint(-r, r + 1, (M, case.N), generator=g).to(BF)
    if epi == QKV:
        idx = (7 * torch.arange(lc.ROPE_LEN)[:, None] + 3 * torch.arange(lc.HEAD // 2)[None, :]) % len(lc.CS)
        inp.rope_cs = torch.tensor(lc.CS, dtype=torch.float32)[idx].contiguous()
        inp.tok_pos = positions(M)
    return inp


def inputs(case):
    return _inputs(case.key)


# --------------------------------------------------------------------------------------------------------------- reference
@functools.lru_cache(maxsize=8)
def _reference(key):
    M, K, segs, epi, fam, qkv = key
    inp = _inputs(key)
    rd = lambda v: v.to(BF).double()  # noqa: E731
    sums = lc.exact_sums(inp)
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
    """Every operand equals dequantize(quantize_rows(.)) bit for bit (arb: the activations; its weights ARE codes and scales)."""
    q, inp = _quant(), inputs(case)
    ok = torch.equal(q.dequantize(*q.quantize_rows(inp.x)), inp.x)
    if case.family != "arb":
        ok = ok and all(torch.equal(q.dequantize(*q.quantize_rows(w)), w) for w in inp.w)
    return ok


def conditions(case):
    """linear_cases.conditions on these inputs (q|k|v: its store form - the position rules of its 8-token leaf do not apply to 256
    rows and more; ours are asserted here), and the bound on the contraction of the codes."""
    inp = inputs(case)
    if case.family == "arb":  # 3 x the round family's sums: what must hold is that rounding before and after the scale differ
        y = lc.exact_sums(inp)[1] if case.epi == SWIGLU else torch.cat(lc.exact_sums(inp), dim=1)
        bound = max(float((inp.x.double().abs() @ w.double().abs().T).max()) for w in inp.w)
        fig = dict(bound=bound, maxy=float(y.abs().max()), inexact=float(lc._inexact(y, BF).double().mean()),
                   differs=float(((y / 3).to(BF).double() * 3).to(BF).ne(y.to(BF)).double().mean()))
        assert bound < 2 ** 24 / 2 ** 9 and fig["inexact"] >= 0.25 and fig["differs"] >= 0.05, (case, fig)
        return fig
    proxy = case if case.epi != QKV else lc.Case(case.name, case.M, case.K, case.segs, STORE, "w8a8", fam=case.fam)
    saved = lc.inputs
    lc.inputs = lambda c: inp
    try:
        fig = lc.conditions(proxy)
    finally:
        lc.inputs = saved
    assert fig["bound"] < 2 ** 24 / 2 ** 9, (case, fig)
    if case.epi == QKV:
        pos = inp.tok_pos
        assert int(pos.max()) < lc.ROPE_LEN and len(set(pos.tolist())) > 8 and len({(int(p) % len(lc.CS)) for p in pos[:8]}) == 8
    return fig


# --------------------------------------------------------------------------------------------------------------- emulation
MUTANTS = ["fragment_from_neighbour_k", "kslice_first", "kslice_middle", "kslice_last", "sx_neighbour_row", "sw_neighbour_row",
           "sw_wrong_segment", "w1_w3_exchanged", "scale_after_rounding", "row_past_written", "col_past_written"]


def applies(case, mutant):
    if mutant == "w1_w3_exchanged":
        return case.epi == SWIGLU
    if mutant == "sw_wrong_segment":
        return case.epi != SWIGLU and len(case.segs) > 1
    if mutant == "kslice_middle":
        return case.K >= 3 * K_MOD
    return True


def emulate(case, mutant=None):
    """The guarded buffer the route writes (module docstring)."""
    q, inp = _quant(), inputs(case)
    M, K, N = case.M, case.K, case.N
    xq, sx = q.quantize_rows(inp.x)
    xq = xq.float()
    wq = [c.float() for c in inp.wq]
    sw = [s.clone() for s in inp.ws]
    if mutant == "w1_w3_exchanged":
        wq, sw = wq[::-1], sw[::-1]
    if mutant == "sw_wrong_segment":   # segment 1's rows scaled by segment 0's array at the same local index
        sw[1] = sw[0][torch.arange(sw[1].shape[0]).clamp_max(sw[0].shape[0] - 1)]
    if mutant == "sx_neighbour_row":
        sx = sx[(torch.arange(M) ^ 1).clamp_max(M - 1)]
    if mutant == "fragment_from_neighbour_k":  # rows 16 .. 31 of every m tile: k group 1 of the middle slice read from group 0
        s0 = (K // K_MOD // 2) * K_MOD
        rows = (torch.arange(M) % 256 // 16) == 1
        xq = xq.clone()
        xq[rows, s0 + 32:s0 + 64] = xq[rows, s0:s0 + 32]
    nk = K // K_MOD
    skip = {"kslice_first": 0, "kslice_middle": nk // 2, "kslice_last": nk - 1}.get(mutant)
    accs = []
    for w in wq:
        acc = torch.zeros(M, w.shape[0], dtype=torch.float32)
        for s in range(nk):
            if s == skip:
                continue
            for f in range(K_MOD // 32):   # one MFMA: four lane groups of 32 bytes
                k0 = s * K_MOD + f * 32
                acc += xq[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
        accs.append(acc)
    bf = lambda v: v.to(BF).float()  # noqa: E731
    scaled = []
    for acc, s in zip(accs, sw):
        if mutant == "sw_neighbour_row":
            s = s[(torch.arange(s.shape[0]) ^ 1).clamp_max(s.shape[0] - 1)]
        sc = sx[:, None] * s[None, :]
        scaled.append(bf(acc) * sc if mutant == "scale_after_rounding" else acc * sc)
    if case.epi == SWIGLU:
        a, b = bf(scaled[0]), bf(scaled[1])
        out = (bf(a / (1.0 + torch.exp(-a))) * b).to(BF)
    else:
        y = bf(torch.cat(scaled, dim=1))
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
