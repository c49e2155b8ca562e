"""The generic-storage linears (csrc/generic.hip: g_gemv_kernel at M <= 8, g_gemm_mfma_kernel above, g_gemm_kernel for anything the
16-byte accesses cannot read) in fp32, fp16 and bf16 on inputs whose every contraction is an EXACT integer sum: one fp64 reference
that rounds to T where the kernel header says the kernel rounds, a mirror of linear_t / launch_g_linear's routing, torch emulations
of each kernel's index logic, and single-fault mutants (helpers for test_generic_linear_cases_host.py and
test_gpu_generic_linear_structured.py; no test functions here).  The constructions, the guarded buffers and the bit comparison are
those of linear_cases.py and row_cases.py, imported; the six f16/generic cases of linear_cases.py stay where they are.

A "piece" is what a lane loads at once: 16 bytes, EPP = 8 elements of a 16-bit type, 4 floats.

Plain family (integers that every T holds; fp32 accumulation gives the same bits in any order; v_mfma_f32_32x32x2f32 forms full
fp32 products):
  W        dense, {-1, +1}
  x[t]     ONE nonzero, +-1, per piece (a last partial piece of an unaligned K included), +-2 in piece 0 when the piece count is even
           (the sum is then odd, never 0); K < 8: dense +-1.  Every weight piece of every row moves every token's output by 1 or 2.
  res      integers in [-R, R], R = min(64, 256 - max|y|)
  SwiGLU   piece 0 of x is 8 (and a 1 behind it when the piece count is odd: b is then odd, never 0), W1[:, 0] = 16: a = 128 +- noise
           in [24, 256], where 1 + expf(-a) == 1.0f and so rnd_T(silu(a)) == a in all three types; W3[:, 0] = +-1
Rounding family (fp16, bf16; fp32 has no rounding point): linear_cases' carrier - x[:, 0] = 8 (fp16: 64), x[:, 1] = 1, W[n, 0] = +-c,
c in [56, 104], W[n, 1] = n % 2 - lifts the sums to where T holds every 2nd or 4th integer (bf16: 256 < |y| < 1024, fp16: 2048 <
|y| < 8192); res in [-7, 7].  SwiGLU lifts b; in fp16 a * b must stay below 65504, so there a = 24 for every output (W1 is zero
outside column 0) and W3[n, 0] = +-c with c in [34, 40]: 2048 < |b| < 2729.
Fused RMSNorm: eps = 0, x dense, row m is +-1 (mean square 1) for even m and +-2 (mean square 4) for odd m, norm_w in {+-1, +-2}
(one in eight is +-2).  ss, ss / K, sqrtf and the reciprocal are exact under IEEE sqrtf and division (the build is -O3 without
fast-math), so inv is 1 or 0.5, rnd(rnd(x inv) w) is exact and neighbouring rows have different inv.  Norm with eps > 0 stays with
the tolerance tests of test_gpu_generic.py.
x lives in a buffer of 3.0s with ldx > K (ldx - K = 8, or 3 where the case is about an odd ldx); the mis-aligned case views it 8
bytes into the allocation.  out and res live in sentinel-filled buffers (linear_cases.guard: two rows above and below, eight
columns to the right); where the call goes through the debug leaf the residual's row stride differs from the output's.

Reference: fp64 sums, .to(T) at every rounding point of generic.hip: STORE rnd(acc); RESIDUAL rnd(res + rnd(acc)); LOGITS
float(rnd(acc)); SwiGLU rnd(rnd(silu(rnd a)) * rnd b); prologue rnd(rnd(x inv) norm_w); `active`: a tile (M <= 8: the launch)
without an active row keeps the sentinel, any other is written whole.

Route mirror: route(M, K, N, ldx, aligned, dtype, form) -> gemv/MR=1|2|4|8, mfma, fma, f16/g256 or unsupported.

conditions() asserts: sum|w x| < 2^24; plain: |y| <= 256, fewer than 15 % zeros; rounding family: at least 25 % of the sums are not
values of T, at least 5 % exact ties, at least 5 % of the RESIDUAL outputs show rnd(r + rnd(acc)) != rnd(r + acc); SwiGLU: 24 <= a
<= 256, fewer than 15 % of b are 0.  Measured over all 170 cases, from the reference alone (test_generic_linear_cases_host.py prints
them): plain max|y| = 140, sum|w x| <= 6848, zeros at most 7.4 % of a case's outputs (norm cases; 0 elsewhere: the sums are odd);
SwiGLU a in [24, 173], no b is 0; rounding family bf16 431 <= |y| <= 852, not bf16 values 66.2 .. 74.2 %, ties 25.0 .. 32.5 %, double
rounding visible in 20.8 .. 31.5 %; fp16 2165 <= |y| <= 6670, not fp16 values 50.0 .. 74.5 %, ties 28.2 .. 50.0 %, double rounding
visible in 23.3 .. 32.0 %.  On the MI355X sqrtf and the division are exact on mean squares 1 and 4: every norm case compares bit
for bit, none falls back to a 1-ulp comparison.

fp32 K: linear_t asks K % 8 == 0 of every type, so the fp32 rows of one chunk + ONE piece (K = 516, 1028) go to the FMA kernel -
they are cases of that kernel here - and the GEMV ladder takes K = 520 and 1032, one chunk + two pieces.

Mutants (test_generic_linear_cases_host.py prints "caught / applies" per kernel over all three types).  mutants_of() lists a mutant
where the structure it breaks exists; invisible() names the cases on which it then still cannot show, each reason asserted from
both sides.  Four listed faults change no output of ANY exact case and are proved invisible instead:
  normw_before_rounding   inv is a power of two, so x inv is a value of T and the first rounding is the identity
  swiglu_round@a, @silu   a is an integer <= 256 and silu(a) == a in fp32: both roundings are the identity (@b is caught)
  more_le                 `k0 + BK <= K` only adds a slab that is outside as a whole: it is zeroed
  row_clamp_m             rows past M - 1 are computed but never stored; the clamp keeps their loads in bounds, nothing else
"""
import functools

import torch

import linear_cases as lc
from linear_cases import LOGITS, RESIDUAL, SENT, STORE, SWIGLU
from row_cases import first_diff

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DT_CODE = {"bf16": 0, "f16": 1, "f32": 2}           # include/mistral_hip.h enum mi_dtype
POISON = 3.0                                        # what lies between the rows of x


# ------------------------------------------------------------------------------------------------------------ route mirror
def gemv_mr(M):
    return 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8


def gemv_unr(M):
    return 4 if gemv_mr(M) <= 2 else 2


def route(M, K, N, ldx, aligned, dtype, form, active=False, norm=False, ldr_is_ldo=True):
    """generic.hip launch_g_linear -> g256_f16_args / linear_t.  aligned: x and w start on 16 bytes; form: 'plain' or 'fused'
    (several matrices, a norm prologue or SwiGLU: the M <= 8 kernel only)."""
    if dtype == "f16" and M >= 256 and not active and not norm and ldx % 8 == 0 and aligned and ldr_is_ldo and lc.gemm256_applicable(M, K):
        return "f16/g256"
    al = K % 8 == 0 and ldx % 8 == 0 and aligned
    if M <= 8 and al:
        return f"gemv/MR={gemv_mr(M)}"
    if form == "fused":
        return "unsupported"
    return "mfma" if al else "fma"


# ------------------------------------------------------------------------------------------------------------------- cases
class GCase:
    """One launch_g_linear call.  segs: rows per weight matrix (SwiGLU: one entry, the rows of W1 and of W3).  active: None, 'none'
    (no row), 'one' (row M // 2 only) or a tuple of rows.  xpad: ldx - K.  misalign: x starts 8 bytes into its allocation.  own_ldr:
    through the debug leaf with ldr != ldo."""

    def __init__(self, dtype, M, K, segs, epi, path, fam="plain", norm=False, active=None, xpad=8, misalign=False, own_ldr=False, salt=0):
        self.dtype, self.M, self.K, self.segs, self.epi, self.path, self.fam = dtype, M, K, tuple(segs), epi, path, fam
        self.norm, self.active, self.xpad, self.misalign, self.own_ldr, self.salt = norm, active, xpad, misalign, own_ldr, salt
        self.N = self.segs[0] if epi == SWIGLU else sum(self.segs)
        self.R = DTYPES[dtype]
        self.odt = torch.float32 if epi == LOGITS else self.R
        self.EPP = 4 if dtype == "f32" else 8
        self.ldx = K + xpad
        self.form = "fused" if (len(self.segs) > 1 or norm or epi == SWIGLU) else "plain"
        self.leaf = self.form == "fused" or active is not None or own_ldr
        self.kernel = path.split("/")[0]
        self.name = (f"{dtype}-m{M}k{K}n{'+'.join(map(str, self.segs))}-{epi}" + ("-r" if fam == "round" else "") + ("-norm" if norm else "") +
                     (f"-act{active if isinstance(active, str) else len(active)}" if active is not None else "") +
                     (f"-ldx{self.ldx}" if xpad != 8 else "") + ("-x8b" if misalign else "") + ("-ldr" if own_ldr else ""))
        assert fam == "plain" or (dtype != "f32" and K >= 16 and not norm)
        assert epi != RESIDUAL or self.leaf or not own_ldr

    def __repr__(self):
        return self.name

    @property
    def key(self):
        return (self.dtype, self.M, self.K, self.segs, self.epi, self.fam, self.norm, self.xpad, self.misalign, self.own_ldr, self.salt)

    @property
    def ldr(self):
        return self.N + (24 if self.own_ldr else 8)

    @property
    def tile_rows(self):
        return {"gemv": 8, "mfma": 128, "fma": 64}[self.kernel]

    def active_rows(self):
        if self.active is None:
            return None
        a = torch.zeros(self.M, dtype=torch.int32)
        rows = [] if self.active == "none" else [self.M // 2] if self.active == "one" else list(self.active)
        a[rows] = 7                                  # (any nonzero value)
        return a


GEMV_MS_LOW, GEMV_MS_HIGH = [1, 2], [3, 4, 5, 8]
GEMV_NS = [1, 2, 7, 9, 40]
GEMV_KS = {"f16": [8, 200, 1024, 1032, 2048, 2056, 2560], "bf16": [8, 200, 1024, 1032, 2048, 2056, 2560], "f32": [8, 200, 512, 520, 1024, 1032, 1280]}
EPIS = [STORE, RESIDUAL, LOGITS]


def _gv(M):
    return f"gemv/MR={gemv_mr(M)}"


def gemv_cases(t):
    """M <= 8: both UNR values at every K of the chunk ladder; surplus rows at M = 3 and 5; N = 1, 7, 9 odd; three matrices with odd
    boundaries; SwiGLU; the norm prologue; `active`."""
    ks, out, i = GEMV_KS[t], [], 0
    for iK, K in enumerate(ks):
        for M in (GEMV_MS_LOW[iK % 2], GEMV_MS_HIGH[iK % 4]):
            epi = EPIS[i % 3]
            out.append(GCase(t, M, K, (GEMV_NS[i % 5],), epi, _gv(M), own_ldr=epi == RESIDUAL and i % 2 == 1))
            i += 1
    k1, k2 = ks[3], ks[5]                               # one chunk + one piece at UNR = 2 / at UNR = 4
    out += [GCase(t, 3, 200, (3, 4, 2), STORE, _gv(3)), GCase(t, 1, k1, (5, 2, 33), RESIDUAL, _gv(1), own_ldr=True),
            GCase(t, 8, k2, (7, 2), LOGITS, _gv(8)),
            GCase(t, 1, 8, (1,), SWIGLU, _gv(1)), GCase(t, 2, 200, (5,), SWIGLU, _gv(2)), GCase(t, 5, k1, (40,), SWIGLU, _gv(5)),
            GCase(t, 2, 200, (9,), STORE, _gv(2), norm=True), GCase(t, 5, k1, (7,), STORE, _gv(5), norm=True),
            GCase(t, 3, k2, (3, 4, 2), STORE, _gv(3), norm=True), GCase(t, 2, k2, (40,), LOGITS, _gv(2), norm=True),
            GCase(t, 4, 200, (9,), STORE, _gv(4), active="none"), GCase(t, 4, 200, (9,), STORE, _gv(4), active="one"),
            GCase(t, 5, 200, (7,), RESIDUAL, _gv(5), active="one", own_ldr=True)]
    if t != "f32":
        out += [GCase(t, 5, 200, (40,), RESIDUAL, _gv(5), fam="round", own_ldr=True), GCase(t, 2, k1, (40,), LOGITS, _gv(2), fam="round"),
                GCase(t, 8, k2, (40,), RESIDUAL, _gv(8), fam="round"), GCase(t, 3, 200, (12, 13, 15), RESIDUAL, _gv(3), fam="round", own_ldr=True),
                GCase(t, 4, 200, (40,), SWIGLU, _gv(4), fam="round"), GCase(t, 1, k1, (40,), SWIGLU, _gv(1), fam="round")]
    return out


def mfma_cases(t):
    """M > 8, aligned: every M and N edge of the 128 x 128 tile, K = 8, 24, 40, 72 with outside pieces (8 and 24: a first slab that
    is itself partial), an `active` tile skip."""
    out = [GCase(t, 9, 8, (1,), STORE, "mfma"), GCase(t, 127, 24, (127,), RESIDUAL, "mfma"), GCase(t, 128, 32, (129,), LOGITS, "mfma"),
           GCase(t, 129, 40, (200,), STORE, "mfma"), GCase(t, 300, 72, (127,), RESIDUAL, "mfma", own_ldr=True),
           GCase(t, 300, 200, (200,), LOGITS, "mfma"), GCase(t, 129, 200, (129,), STORE, "mfma"),
           GCase(t, 300, 40, (129,), STORE, "mfma", active=(5, 290)), GCase(t, 300, 72, (1,), RESIDUAL, "mfma", active=(130,), own_ldr=True)]
    if t != "f16":                                       # (fp16 with M >= 256 and K % 64 == 0: the 256-tile kernel, linear_cases' f16/g256)
        out.append(GCase(t, 300, 2560, (40,), STORE, "mfma"))
    if t != "f32":
        out += [GCase(t, 129, 200, (200,), RESIDUAL, "mfma", fam="round"), GCase(t, 9, 72, (127,), LOGITS, "mfma", fam="round"),
                GCase(t, 300, 40, (129,), RESIDUAL, "mfma", fam="round", own_ldr=True)]
    return out


def fma_cases(t):
    """Anything unaligned: K % 8 != 0 (K < 8: dense x), an odd ldx, an x that starts 8 bytes into its allocation; the 64 x 64 tile's
    M and N edges; `active`."""
    out = [GCase(t, 1, 1, (1,), STORE, "fma", xpad=3), GCase(t, 9, 3, (63,), RESIDUAL, "fma", xpad=3), GCase(t, 64, 15, (65,), LOGITS, "fma"),
           GCase(t, 65, 16, (63,), STORE, "fma", xpad=3), GCase(t, 9, 17, (65,), RESIDUAL, "fma", own_ldr=True), GCase(t, 65, 100, (65,), STORE, "fma"),
           GCase(t, 1, 100, (63,), LOGITS, "fma"), GCase(t, 64, 17, (1,), STORE, "fma"),
           GCase(t, 9, 32, (65,), STORE, "fma", misalign=True), GCase(t, 4, 200, (9,), RESIDUAL, "fma", xpad=3),
           GCase(t, 65, 17, (63,), STORE, "fma", active=(3,)), GCase(t, 130, 100, (65,), RESIDUAL, "fma", active=(64, 129), own_ldr=True)]
    if t != "f32":
        out += [GCase(t, 65, 100, (65,), RESIDUAL, "fma", fam="round", own_ldr=True), GCase(t, 9, 100, (63,), LOGITS, "fma", fam="round")]
    else:                                                # fp32 rows of one chunk + ONE piece: K % 8 == 4, which linear_t sends here
        out += [GCase(t, 2, 516, (2,), STORE, "fma"), GCase(t, 5, 1028, (9,), RESIDUAL, "fma")]
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = [c for t in ("f32", "f16", "bf16") for c in gemv_cases(t) + mfma_cases(t) + fma_cases(t)]
    assert len({c.name for c in out}) == len(out), sorted(c.name for c in out)
    return out


def case_route(case):
    """The mirror's label for the call the GPU test makes for this case."""
    return route(case.M, case.K, case.N, case.ldx, not case.misalign, case.dtype, case.form, case.active is not None, case.norm, not case.own_ldr)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _seed(c):
    return (c.M * 1000003 + c.K * 10007 + sum((i + 1) * s for i, s in enumerate(c.segs)) * 101 + EPIS.index(c.epi) * 7 if c.epi != SWIGLU else
            c.M * 1000003 + c.K * 10007 + c.segs[0] * 101 + 29) + (13 if c.fam == "round" else 0) + {"f32": 0, "f16": 3, "bf16": 5}[c.dtype] + \
        (17 if c.norm else 0) + 1009 * c.salt


def _plain_x(M, K, EPP, g):
    if K < 8:
        return lc._signs((M, K), g)
    P = (K + EPP - 1) // EPP
    x = torch.zeros(M, P * EPP)
    width = torch.full((P,), EPP)
    width[-1] = K - (P - 1) * EPP
    pos = (torch.rand(M, P, generator=g) * width).long().clamp(max=EPP - 1)
    x.view(M, P, EPP).scatter_(2, pos[..., None], lc._signs((M, P, 1), g))
    if P % 2 == 0:
        x[:, :EPP] *= 2.0
    return x[:, :K].contiguous()


@functools.lru_cache(maxsize=8)
def _inputs(key):
    dtype, M, K, segs, epi, fam, norm, xpad, misalign, own_ldr, salt = key
    c = GCase(dtype, M, K, segs, epi, "x", fam=fam, norm=norm, xpad=xpad, misalign=misalign, own_ldr=own_ldr, salt=salt)
    g = torch.Generator().manual_seed(_seed(c))
    R, N = c.R, c.N
    rows = [N, N] if epi == SWIGLU else list(segs)
    w = [lc._signs((n, K), g) for n in rows]
    norm_w = None
    if norm:
        x = lc._signs((M, K), g) * (1.0 + (torch.arange(M) % 2).float())[:, None]
        norm_w = lc._signs((K,), g) * (1.0 + (torch.randint(0, 8, (K,), generator=g) == 0).float())
    else:
        x = _plain_x(M, K, c.EPP, g)
    lift = 64.0 if dtype == "f16" else 8.0
    if fam == "round":
        x[:, :c.EPP] = 0.0
        x[:, 0], x[:, 1] = lift, 1.0
    elif epi == SWIGLU:
        x[:, :c.EPP] = 0.0
        x[:, 0] = 8.0
        x[:, 1] = float((K // c.EPP) % 2)                # an odd piece count: one more +-1, so that b is odd, never 0
    if epi == SWIGLU:
        w[0][:, 0] = 16.0
        if fam == "round" and dtype == "f16":            # a = 24 everywhere, 2048 < |b| < 2729: a b < 65504
            w[0][:] = 0.0
            w[0][:, 0] = 0.375
            n = torch.arange(N)
            w[1][:, 0] = (34 + (5 * n + 3) % 7).float() * (1 - 2 * ((n // 2) % 2)).float()
            w[1][:, 1] = (n % 2).float()
        elif fam == "round":
            lc._lift(w[1])
    elif fam == "round":
        for i, wi in enumerate(w):
            lc._lift(wi, sum(rows[:i]))
    inp = lc.Inputs(x=x.to(R), w=[wi.to(R) for wi in w], res=None, norm_w=None if norm_w is None else norm_w.to(R))
    assert torch.equal(inp.x.float(), x) and all(torch.equal(a.float(), b) for a, b in zip(inp.w, w))
    off = (8 // R.itemsize) if misalign else 0
    inp.xbuf = torch.full((off + (M + 1) * c.ldx,), POISON, dtype=R)
    x_view(inp.xbuf, c).copy_(inp.x)
    if epi == RESIDUAL:
        y = torch.cat(exact_sums(c, inp), dim=1)
        r = 7 if fam == "round" else min(64, 256 - int(y.abs().max()))
        assert r >= 1, (key, r)
        inp.res = torch.randint(-r, r + 1, (M, N), generator=g).to(R)
        inp.resbuf = torch.full((M + 4, c.ldr), SENT, dtype=R)
        inp.resbuf[2:2 + M, :N] = inp.res
    return inp


def inputs(case):
    return _inputs(case.key)


def x_view(xbuf, case):
    """x [M, K] with row stride ldx inside its flat buffer (the mis-aligned case: 8 bytes in)."""
    off = (8 // case.R.itemsize) if case.misalign else 0
    return xbuf.as_strided((case.M, case.K), (case.ldx, 1), off)


def res_view(resbuf, case):
    return resbuf[2:2 + case.M, :case.N]


def normalised(case, inp):
    """fp64 [M, K]: what the contraction runs on - x, or rnd(rnd(x inv) norm_w) with inv = 1 / sqrt(mean square) (eps = 0)."""
    x = inp.x.double()
    if not case.norm:
        return x
    inv = 1.0 / torch.sqrt((x * x).sum(dim=1, keepdim=True) / case.K)
    return ((x * inv).to(case.R).double() * inp.norm_w.double()).to(case.R).double()


def exact_sums(case, inp):
    xn = normalised(case, inp)
    return [xn @ w.double().T for w in inp.w]


def written_rows(case):
    """bool [M]: rows of tiles with an active row (every row without a mask)."""
    a = case.active_rows()
    if a is None:
        return torch.ones(case.M, dtype=torch.bool)
    if case.kernel == "gemv":
        return torch.full((case.M,), bool(a.any()))
    tr = case.tile_rows
    return torch.cat([torch.full((min(tr, case.M - m0),), bool(a[m0:m0 + tr].any())) for m0 in range(0, case.M, tr)])


@functools.lru_cache(maxsize=8)
def _reference(key, case):
    inp, R = _inputs(key), case.R
    rd = lambda v: v.to(R).double()          # noqa: E731
    sums = exact_sums(case, inp)
    if case.epi == SWIGLU:
        a, b = rd(sums[0]), rd(sums[1])
        s = rd(a / (1.0 + torch.exp(-a)))
        return (s * b).to(R)
    y = rd(torch.cat(sums, dim=1))
    if case.epi == LOGITS:
        return y.float()
    if case.epi == RESIDUAL:
        return (inp.res.double() + y).to(R)
    return y.to(R)


def reference(case):
    return _reference(case.key, case)


def expected(case):
    """The reference inside its guard buffer; rows of a skipped tile keep the sentinel."""
    buf, view = lc.guard(case.M, case.N, case.odt)
    rows = written_rows(case)
    view[rows] = reference(case)[rows]
    return buf


def mismatch(case, got, want):
    """None when the whole guard buffer is bit-equal to `want`, else a text naming the first differing element of the buffer
    (the view starts at row 2; columns from N on and rows outside [2, 2 + M) are guard elements)."""
    d = first_diff(got.cpu(), want)
    return d and f"{case} [{case.path}] buffer (row - 2, column) {d}"


# -------------------------------------------------------------------------------------------------------------- conditions
def conditions(case):
    """Asserts the constructions' conditions (module docstring) from the reference alone; returns the measured figures."""
    inp, R = inputs(case), case.R
    xn = normalised(case, inp)
    sums = exact_sums(case, inp)
    bound = max(float((xn.abs() @ w.double().abs().T).max()) for w in inp.w)
    assert bound < 2 ** 24, (case, bound)
    fig = dict(bound=bound)
    assert case_route(case) == case.path, (case, case_route(case))
    if case.norm:
        x = inp.x.double()
        ms = (x * x).sum(dim=1) / case.K
        assert torch.equal(ms, 1.0 + 3.0 * (torch.arange(case.M) % 2).double()) and float((x * x).sum(dim=1).max()) < 2 ** 24
        assert case.M < 2 or {1.0, 4.0} == set(ms.tolist())
    if case.epi == SWIGLU:
        a, b = sums
        fig["a"] = (float(a.min()), float(a.max()))
        assert 24 <= a.min() and a.max() <= 256, (case, fig)
        af = a.float()
        assert torch.equal(af / (1.0 + torch.exp(-af)), af) and torch.equal(a.to(R).double(), a)
        fig["bzeros"] = float((b == 0).double().mean())
        assert fig["bzeros"] < 0.15, (case, fig)
        y = b
    else:
        y = torch.cat(sums, dim=1)
    fig["maxy"], fig["miny"] = float(y.abs().max()), float(y.abs().min())
    if case.fam == "plain":
        assert fig["maxy"] <= 256 and not bool(lc._inexact(y, R).any()), (case, fig)
        fig["zeros"] = float((y == 0).double().mean())
        assert fig["zeros"] < 0.15, (case, fig)
        if case.epi == RESIDUAL:
            assert float((inp.res.double() + y).abs().max()) <= 256, case
    else:
        base = 2048 if case.dtype == "f16" else 256
        assert base < fig["miny"] and fig["maxy"] < 4 * base, (case, fig)
        fig["inexact"], fig["ties"] = float(lc._inexact(y, R).double().mean()), float(lc._ties(y, base).double().mean())
        assert fig["inexact"] >= 0.25 and fig["ties"] >= 0.05, (case, fig)
        if case.epi == RESIDUAL:
            r = inp.res.double()
            fig["double"] = float(((r + y.to(R).double()).to(R) != (r + y).to(R)).double().mean())
            assert fig["double"] >= 0.05, (case, fig)
        if case.epi == SWIGLU:
            assert float((sums[0] * y.to(R).double()).abs().max()) < (65504 if case.dtype == "f16" else 2 ** 24), case
    return fig


# ----------------------------------------------------------------------------------------------------------------- mutants
ROUNDING = ["residual_single_rounding", "logits_not_rounded", "residual_ldo_stride"]
GEMV_MUTANTS = ["piece_dropped", "tail_counted", "other_unr_stride", "surplus_row_stored", "col_past_n_stored", "seg_off_by_one@n0",
                "seg_off_by_one@n1", "second_col_first_matrix", "inv_neighbour", "normw_before_rounding", "norm_tail_counted", "up_row_from_w",
                "swiglu_round@a", "swiglu_round@silu", "swiglu_round@b", "active_per_row"] + ROUNDING
MFMA_MUTANTS = ["piece_dropped", "outside_piece_counted", "slab_skipped", "more_le", "row_clamp_m", "rowmap_no_lane_half", "store_past_m",
                "store_past_n", "active_per_row"] + ROUNDING
FMA_MUTANTS = ["piece_dropped", "ktail_counted", "staging_swapped", "store_past_m", "store_past_n", "active_per_row"] + ROUNDING
MUTANTS = {"gemv": GEMV_MUTANTS, "mfma": MFMA_MUTANTS, "fma": FMA_MUTANTS}
NEVER_VISIBLE = {
    "normw_before_rounding": "inv is a power of two: x inv is a value of T, the first rounding is the identity",
    "swiglu_round@a": "a is an integer <= 256, a value of T",
    "swiglu_round@silu": "1 + expf(-a) == 1.0f: silu(a) == a, a value of T",
    "more_le": "the extra slab is outside as a whole and zeroed",
    "row_clamp_m": "rows past M - 1 are computed but never stored",
}


def family(m):
    return m.split("@")[0]


def _chunk(case):
    return 64 * gemv_unr(case.M)


def mutants_of(case):
    """The mutants whose broken structure exists in this case."""
    c, k = case, case.kernel
    if c.active == "none":
        return ["active_per_row"]
    plain, PR, tr = c.fam == "plain", c.K // c.EPP, c.tile_rows
    has = {
        "piece_dropped": plain, "tail_counted": plain and PR % _chunk(c) != 0, "other_unr_stride": plain,
        "surplus_row_stored": gemv_mr(c.M) > c.M, "col_past_n_stored": c.epi != SWIGLU and c.N % 2 == 1,
        "seg_off_by_one@n0": len(c.segs) >= 2, "seg_off_by_one@n1": len(c.segs) >= 3,
        "second_col_first_matrix": any(sum(c.segs[:i]) % 2 for i in range(1, len(c.segs))),
        "inv_neighbour": c.norm, "normw_before_rounding": c.norm, "norm_tail_counted": c.norm and PR % _chunk(c) != 0,
        "up_row_from_w": c.epi == SWIGLU, "swiglu_round@a": c.epi == SWIGLU and not plain, "swiglu_round@silu": c.epi == SWIGLU and not plain,
        "swiglu_round@b": c.epi == SWIGLU and not plain, "active_per_row": c.active is not None,
        "residual_single_rounding": c.epi == RESIDUAL and not plain, "logits_not_rounded": c.epi == LOGITS and not plain,
        "residual_ldo_stride": c.epi == RESIDUAL and c.own_ldr,
        "outside_piece_counted": plain and c.K % 32 != 0, "slab_skipped": plain, "more_le": True, "row_clamp_m": c.M % 128 != 0,
        "rowmap_no_lane_half": True, "store_past_m": c.M % tr != 0, "store_past_n": c.N % tr != 0,
        "ktail_counted": plain and c.K % 16 != 0, "staging_swapped": plain,
    }
    return [m for m in MUTANTS[k] if has[m]]


def _sources(case, mutant=None):
    """[(matrix, local row)] per output column (g_seg_row); a lookup one past a matrix's end wraps to its row 0, as in linear_cases."""
    src, ends = [], []
    for i, n in enumerate(case.segs):
        src += [(i, r) for r in range(n)]
        ends.append(len(src))
    if family(mutant or "") == "seg_off_by_one":
        b = 0 if mutant.endswith("n0") else 1
        src[ends[b]] = (b, 0)
    if mutant == "second_col_first_matrix":
        for e in ends[:-1]:
            if e % 2 == 1:
                src[e] = (src[e - 1][0], 0)
    return src


def invisible(case, mutant):
    """A reason why `mutant`, although its structure exists in `case`, cannot change the compared buffer - or None."""
    c = case
    if mutant in NEVER_VISIBLE:
        return NEVER_VISIBLE[mutant]
    if c.active == "none":
        return "no row is active: nothing is written either way"
    if mutant == "other_unr_stride" and c.kernel == "gemv" and c.K // c.EPP <= 128:
        return "at most 128 pieces: one chunk under either stride"
    if mutant == "inv_neighbour" and c.M < 2:
        return "one row"
    if mutant == "store_past_m" and not bool(written_rows(c)[-1]):
        return "the last row tile has no active row"
    if mutant == "staging_swapped" and c.M == 1 and c.K == 1:
        return "one row of one element: its own transpose"
    if mutant == "norm_tail_counted":                   # the tail's squares move inv by less than the first rounding sees
        x, PR = inputs(c).x.float(), c.K // c.EPP
        extra = _slot_counts(PR, gemv_unr(c.M), _chunk(c), True)[PR - 1] - 1.0
        ss = (x * x).sum(-1)
        inv, off = 1.0 / torch.sqrt(ss / float(c.K)), 1.0 / torch.sqrt((ss + extra * (x[:, -c.EPP:] ** 2).sum(-1)) / float(c.K))
        if torch.equal((x * inv[:, None]).to(c.R), (x * off[:, None]).to(c.R)):
            return "rnd(x inv) absorbs the tail's share of the mean square"
    if mutant == "residual_ldo_stride" and not bool(written_rows(c)[1:].any()):
        return "only row 0 is written: no stride is applied"
    if family(mutant) in ("seg_off_by_one", "second_col_first_matrix"):
        y = torch.cat(exact_sums(c, inputs(c)), dim=1)
        good, bad = _sources(c), _sources(c, mutant)
        first = [sum(c.segs[:s]) for s in range(len(c.segs))]
        if all(torch.equal(y[:, n], y[:, first[b[0]] + b[1]]) for n, (a, b) in enumerate(zip(good, bad)) if a != b):
            return "the substituted row's sums agree for every token"
    return None


# -------------------------------------------------------------------------------------------------------------- emulations
def _epilogue(case, acc, acc_b, res, mutant):
    """fp32 accumulators -> the output dtype: g_store and the SwiGLU tail of g_gemv_kernel."""
    R = case.R
    rd = lambda v: v.to(R).float()           # noqa: E731
    if case.epi == SWIGLU:
        a = acc if mutant == "swiglu_round@a" else rd(acc)
        b = acc_b if mutant == "swiglu_round@b" else rd(acc_b)
        s = a / (1.0 + torch.exp(-a))
        s = s if mutant == "swiglu_round@silu" else rd(s)
        return (s * b).to(R)
    if case.epi == LOGITS:
        return acc if mutant == "logits_not_rounded" else rd(acc)
    y = acc if mutant == "residual_single_rounding" else rd(acc)
    return (res.float() + y).to(R) if case.epi == RESIDUAL else y.to(R)


def _res_at(case, inp, rows, cols, mutant):
    """The residual as g_store reads it: storage element rows * ldr + cols from the view's first element (past the storage: the
    sentinel)."""
    ld = case.N + 8 if mutant == "residual_ldo_stride" else case.ldr
    flat = inp.resbuf.reshape(-1)
    idx = 2 * case.ldr + rows[:, None] * ld + cols[None, :]
    return torch.where(idx < flat.numel(), flat[idx.clamp(max=flat.numel() - 1)], torch.tensor(SENT, dtype=flat.dtype))


def _store(case, inp, buf, rows, cols, acc, acc_b, mutant):
    """Write epilogue(acc [len(rows), len(cols)]) at (rows, cols) of the view; elements past the guard buffer are dropped."""
    big = buf[2:, :]
    rk, ck = rows < big.shape[0], cols < big.shape[1]
    rows, cols, acc = rows[rk], cols[ck], acc[rk][:, ck]
    if not rows.numel() or not cols.numel():
        return
    res = _res_at(case, inp, rows, cols, mutant) if case.epi == RESIDUAL else None
    big[rows[:, None], cols[None, :]] = _epilogue(case, acc, acc_b[rk][:, ck] if acc_b is not None else None, res, mutant)


def _pick_piece(case, xn, wrows, bcol=None):
    """(column, piece) from the middle whose products are nonzero for a stored row (SwiGLU: and whose b is nonzero)."""
    EPP, ncol = case.EPP, wrows.shape[0]
    P = (case.K + EPP - 1) // EPP
    rows = written_rows(case)
    for dn in range(ncol):
        n = (ncol // 2 + dn) % ncol
        for dp in range(P):
            p = (P // 2 + dp) % P
            d = xn[:, p * EPP:(p + 1) * EPP] @ wrows[n, p * EPP:(p + 1) * EPP]
            if bcol is not None:
                d = d * bcol[:, n]
            if bool((d[rows] != 0).any()):
                return n, p
    raise AssertionError((case, "no piece whose loss would show"))


def _slot_counts(PR, unr, stride, count_tail):
    """How often each piece is counted by the chunk loop: lanes start at p0 = lane, walk p0 += stride, take slots p0 + 64 u, u < unr,
    load piece min(slot, PR - 1) and count it when slot < PR."""
    cnt = torch.zeros(PR)
    for lane in range(64):
        for p0 in range(lane, PR, stride):
            for u in range(unr):
                s = p0 + 64 * u
                if s < PR or count_tail:
                    cnt[min(s, PR - 1)] += 1
    return cnt


def gemv_emulation(case, mutant=None):
    inp = inputs(case)
    c, M, K, N, EPP = case, case.M, case.K, case.N, case.EPP
    R, PR, MR, UNR = c.R, K // EPP, gemv_mr(M), gemv_unr(M)
    rd = lambda v: v.to(R).float()           # noqa: E731
    stride = 64 * UNR if mutant != "other_unr_stride" else 64 * (6 - UNR)
    x = inp.x.float()[torch.arange(MR).clamp(max=M - 1)]                       # surplus rows repeat row M - 1
    if c.norm:
        cs = _slot_counts(PR, UNR, 64 * UNR, mutant == "norm_tail_counted")
        ss = ((x * x).view(MR, PR, EPP).sum(-1) * cs).sum(-1)
        inv = 1.0 / torch.sqrt(ss / float(K) + 0.0)
        if mutant == "inv_neighbour" and M >= 2:
            inv = inv[[m + 1 if m + 1 < M else m - 1 for m in range(M)] + [M - 2] * (MR - M)]
        nw = inp.norm_w.float()
        x = rd(x * inv[:, None] * nw) if mutant == "normw_before_rounding" else rd(rd(x * inv[:, None]) * nw)
    cnt = _slot_counts(PR, UNR, stride, mutant == "tail_counted").repeat_interleave(EPP)
    sw = c.epi == SWIGLU
    if sw:
        Wa, Wb = inp.w[0].float(), inp.w[0 if mutant == "up_row_from_w" else 1].float()
        ncols = N
    else:
        src = _sources(c, mutant)
        ncols = 2 * ((N + 1) // 2)                                              # two columns per wave; the odd last one's partner repeats it
        Wa, Wb = lc._gather([w for w in inp.w], [src[min(j, N - 1)] for j in range(ncols)]), None
    if mutant == "piece_dropped":
        n, p = _pick_piece(c, x[:M], Wa[:N], (x[:M] @ Wb.T) if sw else None)
        Wa = Wa.clone()
        Wa[n, p * EPP:(p + 1) * EPP] = 0.0
    acc = (x * cnt) @ Wa.T
    acc_b = (x * cnt) @ Wb.T if sw else None
    buf, _ = lc.guard(M, N, c.odt)
    act = c.active_rows()
    if act is not None and not bool(act.any()):
        return buf
    rows = torch.arange(MR if mutant == "surplus_row_stored" else M)
    if act is not None and mutant == "active_per_row":
        rows = rows[act != 0]
    cols = torch.arange(N + 1 if (mutant == "col_past_n_stored" and not sw) else N)
    _store(c, inp, buf, rows, cols, acc[rows][:, cols], acc_b[rows][:, cols] if sw else None, mutant)
    return buf


def tile_emulation(case, mutant=None):
    """g_gemm_mfma_kernel (128 x 128 tiles, K slabs of 32, 16-byte pieces inside or outside as a whole) and g_gemm_kernel (64 x 64,
    slabs of 16, a per-element K tail): rows and weight rows clamped to the last valid one, stores inside m < M and n < N."""
    inp = inputs(case)
    c, M, K, N, EPP = case, case.M, case.K, case.N, case.EPP
    mf = c.kernel == "mfma"
    BM = BN = 128 if mf else 64
    BK = 32 if mf else 16
    x, W = inp.x.float(), inp.w[0].float()
    if mutant == "piece_dropped":
        n, p = _pick_piece(c, x, W)
        W = W.clone()
        W[n, p * EPP:(p + 1) * EPP] = 0.0
    Kup = (K + BK - 1) // BK * BK
    xflat = torch.cat((inp.xbuf.float()[x_view(inp.xbuf, c).storage_offset():], torch.full((Kup,), POISON)))
    wflat = torch.cat((W.reshape(-1), torch.full((Kup,), POISON)))
    xp, wp = torch.zeros(M + 1, Kup), torch.zeros(N, Kup)
    xp[:M, :K], wp[:, :K] = x, W
    xp[M, :K] = POISON                                                          # what a clamp to M would load
    if mutant == "ktail_counted":                                                # the elements behind each row's end, as they lie in memory
        ks = torch.arange(K, Kup)
        xp[:M, K:] = xflat[torch.arange(M)[:, None] * c.ldx + ks]
        wp[:, K:] = wflat[torch.arange(N)[:, None] * K + ks]
    buf, _ = lc.guard(M, N, c.odt)
    act = c.active_rows()
    tiles = [(mt, nt) for mt in range((M + BM - 1) // BM) for nt in range((N + BN - 1) // BN)]
    live = [t for t in tiles if bool(written_rows(c)[t[0] * BM])]
    hit = live[len(live) // 2]                                                  # the tile of the one-tile mutants: a written one
    nslab = Kup // BK
    for mt, nt in tiles:
        m0, n0 = mt * BM, nt * BN
        rv, cv = min(BM, M - m0), min(BN, N - n0)
        if act is not None and mutant != "active_per_row" and not bool(act[m0:m0 + rv].any()):
            continue
        rows = m0 + torch.arange(BM).clamp(max=rv if mutant == "row_clamp_m" else rv - 1)
        a, wt = xp[rows], wp[n0 + torch.arange(BN).clamp(max=cv - 1)]
        acc = torch.zeros(BM, BN)
        for s in range(nslab + (1 if (mutant == "more_le" and K % BK == 0) else 0)):
            if mutant == "slab_skipped" and (mt, nt) == hit and s == nslab // 2:
                continue
            if s >= nslab:
                continue                                                        # (a slab outside as a whole: zeros)
            asl, wsl = a[:, s * BK:(s + 1) * BK], wt[:, s * BK:(s + 1) * BK]
            if mutant == "staging_swapped":                                     # (row, k) <-> (k, row) inside each 16-row block of the A slab
                asl = asl.reshape(BM // 16, 16, 16).transpose(1, 2).reshape(BM, 16)
            acc = acc + asl @ wsl.T
        if mutant == "outside_piece_counted":
            acc = acc + float((Kup - K) // EPP) * (a[:, :EPP] @ wt[:, :EPP].T)
        srow = torch.arange(rv + (1 if (mutant == "store_past_m" and rv < BM) else 0))
        scol = torch.arange(cv + (1 if (mutant == "store_past_n" and cv < BN) else 0))
        if mutant == "rowmap_no_lane_half":                                      # lanes 32.. store on the rows of lanes 0..31 (and win)
            lo = srow[(srow & 4) == 0]
            acc = acc.clone()
            acc[lo] = acc[lo + 4]
            srow = lo
        if act is not None and mutant == "active_per_row":
            srow = srow[act[m0 + srow.clamp(max=rv - 1)] != 0]
        _store(c, inp, buf, m0 + srow, n0 + scol, acc[srow][:, scol], None, mutant)
    return buf


def emulate(case, mutant=None):
    return gemv_emulation(case, mutant) if case.kernel == "gemv" else tile_emulation(case, mutant)
