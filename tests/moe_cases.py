"""MoE expert leaves (`_hip.moe_experts`) with CHOSEN routing and inputs whose whole rounding chain is exact, one fp64-chain
reference, and torch emulations of both pipelines with single-fault mutants (helpers for test_moe_cases_host.py and
test_gpu_moe_structured.py; no test functions here).

Why: the operator tests take their routing from the router on N(0,1) inputs and compare under 3e-2 max|ref|.  Random routing
gives every expert ~T k / E rows - never an empty expert, a 1-row tile, a count of exactly tile_rows or a second m-tile - and
the bound cannot see one row gathered from the neighbouring token, one tile run with the next expert's weights, or the last
row of a ragged tile dropped: each moves a few rows of hundreds by O(1).

Exact family (every value an integer or a dyadic rational that bf16 holds; every fp32 contraction an exact integer sum, so
the result has the same bits in any summation order - MFMA, v_dot2, torch on the CPU):
  x[t]      integers in [-2, 2], x[:, 0] = 8
  W1_e      {-1, 0, 1} (half of the entries 0), W1_e[:, 0] = 16: a = bf16(W1 x) = 128 +- noise, an integer <= 256
  W3_e      {-1, 0, 1};  W2_e: {-1, 0, 1} thinned to a per-case density (1/16, less at large F)
  h         multiples of 8 in [-1024, 1024]
  sel_w     dyadic, different from token to token: k = 2 pairs such as 0.625 / 0.375 and 0.8125 / 0.1875, k = 4 four distinct
            values summing to 1 (sixteenths or thirty-seconds) in a per-token permutation, k = 1 exactly 1.0
conditions() asserts for every routed (token, expert) pair: 24 <= a <= 256 - there 1 + exp(-a) is exactly 1.0f, so
bf16(silu(a)) == a for swiglu_bf and swiglu_bf_fast alike, even with a 1-ulp rcp - and sum|term| < 2^24 at each of the three
contractions; the combine adds multiples of 1/32 below 2^19, exact in fp32 before each bf16 rounding.  Measured over all GPU
cases: a in [47, 208]; sum|term| <= 348 (W1), 284 (W3), 3.1e5 (W2).

Reference (reference()): fp64 with an explicit .to(bfloat16) at every rounding point of moe.py:24-32 and
transformer_layers.py:105-106, 168: a, b = bf16(W1 x), bf16(W3 x); hid = bf16(bf16(silu a) b); y = bf16(W2 hid); R accumulated in
bf16 from zero over the experts in ascending id of bf16(w y); out = bf16(h + R).

Emulations (CPU torch, fp32 accumulation over 64-wide K slices in reversed order, each slice's partial product formed in fp64
and rounded once to fp32, so that the result does not depend on the BLAS at hand):
  grouped_emulation   moe_lists_kernel (counts, offsets, tile table for tile_rows, tok_of, row_of) -> gather -> per tile the
                      W1|W3 GEMM + SwiGLU, then the W2 GEMM, both honouring rows_valid and max_m_tiles -> moe_combine_kernel
  decode_emulation    GEMV_MOE_W13 per (token, slot) into hid [T k, F], then moe_w2_kernel: experts sorted by id, slot_of remap
Both equal the reference bit for bit on every exact case (test_moe_cases_host.py).

Mutants, measured on the CPU by test_moe_cases_host.py: per path the number of GPU cases whose output changes / the cases
the mutant applies to, and the largest count of differing output rows (tokens) in one case.  A mutant applies where the
structure it breaks exists (a ragged tile followed by another expert's row, an empty expert in front of a row, k >= 2, ...).
The order mutant (combine in slot order) is visible ONLY at k = 4: with two addends bf16(bf16(0 + p) + q) is commutative, so no
k <= 2 case can see it (asserted), and at k = 4 only in tokens whose picks are not written in ascending order.

  mutant                                       128-row tiles   256-row tiles   decode
  last valid row of a ragged tile not written  7/7   1 row     1/1   1         -
  row after a tile's valid rows written        6/6   1         1/1   1         -
  a tile takes expert e+1's weights            6/6   128       3/3   256       -
  an empty expert emits a tile                 2/2   1         1/1   1         -
  W1 and W3 exchanged                          7/7   520       4/4   1024      27/27  8
  tok_of off by one for one row                7/7   1         4/4   1         -
  combine in slot order                        1/7   66        1/4   341       9/18   6     (the k = 4 cases, and only they)
  a token's slot weights exchanged             6/6   1         3/3   1         18/18  1
  slot_of identity                             -               -               18/18  6
  hid left in fp32                             7/7   520       4/4   1024      27/27  8
  K slice skipped, W13 stage: first            7/7   128       4/4   256       27/27  8
                              middle           7/7   128       4/4   256       27/27  8
                              last             7/7   128       4/4   256       27/27  8
  K slice skipped, W2 stage:  first            7/7   128       4/4   256       27/27  8
                              middle           7/7   128       4/4   256       27/27  8
                              last             7/7   128       4/4   256       27/27  8
  128-row table used with 256-row tiles        -               4/4   512       -
The tile mutants break ONE tile (the K-slice and weight mutants the middle tile of the table, the ragged-tile mutants the first
ragged tile), the row mutants one row, the weight exchange one token.  "128-row table used with 256-row tiles": the table is
built for 128-row tiles while the grid is sized for 256-row ones, so the tiles past max_m_tiles = ceil(T k / 256) + E never
run.  The two LDS-edge decode cases (100 MB of weights each) are checked against the reference but carry no mutants;
test_moe_cases_host.py names the cases behind every figure.

Gaussian family (SiLU's sensitive range; N(0,1) x, N(0, 1/K) weights as test_gpu_ops._moe_case, chosen routing, the same
reference): tolerance(S) = c 2^-7 S + 1e-6 per element with S = |h| + sum_k w_k (|W2_e| |hid_e|).  c is measured, not chosen:
the honest emulations above reach at most GAUSS_HONEST = 0.138 of 2^-7 S against the fp64-chain reference (grouped case;
the decode case's 8 tokens come out bit-equal; the host test re-measures both), and GAUSS_C = 0.414 is three times that,
since the GPU differs from the emulation by summation order only.  Both sides share every rounding point, so the whole
error is made of single bf16 roundings that fall the other way.  Measured on the MI355X: 0.237 (grouped), 0 (decode).
"""
import functools

import torch

BF = torch.bfloat16
MOE_MAX_E = 16               # elementwise.hip
GEMV_MAX_T = 8               # T <= 8: mi_moe_experts_decode, above: mi_moe_grouped_gemm
KS = 64                      # K slice of both GEMM kernels (BK)

GAUSS_HONEST = 0.138         # measured on the CPU (module docstring); re-measured by test_moe_cases_host.py
GAUSS_C = 3 * GAUSS_HONEST


def tile_rows_for(T, k, E, D, F):
    """api.hip moe_grouped: 256-row m-tiles once an expert averages two of them and both K are multiples of 64."""
    return 256 if (T * k >= 512 * E and D % 64 == 0 and F % 64 == 0) else 128


def max_m_tiles(T, k, E, tile_rows):
    return (T * k + tile_rows - 1) // tile_rows + E


# --------------------------------------------------------------------------------------------------------------- routing
K2_W = [(0.625, 0.375), (0.8125, 0.1875), (0.375, 0.625), (0.25, 0.75), (0.5625, 0.4375), (0.6875, 0.3125), (0.125, 0.875)]
K4_W = [(0.4375, 0.3125, 0.1875, 0.0625), (0.5, 0.25, 0.15625, 0.09375), (0.375, 0.3125, 0.25, 0.0625), (0.53125, 0.21875, 0.15625, 0.09375)]


def slot_weights(T, k):
    """fp32 [T, k]: dyadic, each row summing to 1, varied from token to token (k = 4: also permuted by token)."""
    if k == 1:
        return torch.ones(T, 1)
    rows = []
    for t in range(T):
        if k == 2:
            rows.append(K2_W[t % len(K2_W)])
        else:
            w = K4_W[t % len(K4_W)]
            r = (t // len(K4_W)) % 4
            rows.append(w[r:] + w[:r])
    return torch.tensor(rows, dtype=torch.float32)


def order_slots(picks, order, t):
    """One token's ascending picks in the prescribed slot order: asc, desc, rot (rotated left by 1 + t % (k - 1)), or mixed
    (t % 3 -> asc, desc, rot)."""
    k = len(picks)
    if order == "mixed":
        order = ("asc", "desc", "rot")[t % 3]
    if order == "asc" or k == 1:
        return list(picks)
    if order == "desc":
        return list(picks[::-1])
    assert order == "rot", order
    r = 1 + t % (k - 1) if k > 2 else 1
    return list(picks[r:] + picks[:r])


def route_from_counts(T, k, counts, order="asc"):
    """sel_idx int32 [T, k]: every token k distinct experts, expert e picked by exactly counts[e] tokens.  The experts are
    laid out as runs (expert e repeated counts[e] times) and position p goes to token p % T: a run no longer than T never
    meets a token twice."""
    assert sum(counts) == T * k and all(0 <= c <= T for c in counts), (T, k, counts)
    seq = [e for e, c in enumerate(counts) for _ in range(c)]
    return torch.tensor([order_slots([seq[t + j * T] for j in range(k)], order, t) for t in range(T)], dtype=torch.int32)


def route_decode(T, k, E, order="mixed"):
    """Decode routing: tokens 0 and 1 pick the same experts (in different slot orders), token 2 none of theirs, the others
    sets drawn at random."""
    g = torch.Generator().manual_seed(700 + 10 * T + k)
    rows = []
    for t in range(T):
        if t <= 1:
            picks = list(range(1, 2 * k, 2)) if 2 * k <= E else list(range(k))
        elif t == 2 and 2 * k <= E:
            picks = list(range(0, 2 * k, 2))
        else:
            picks = sorted(torch.randperm(E, generator=g)[:k].tolist())
        # token 0 descending, token 1 rotated (k = 2, where a rotation IS the descending order: token 1 ascending)
        rows.append(order_slots(picks, order, t + 1 if k > 2 else (1, 0)[t % 2]))
    return torch.tensor(rows, dtype=torch.int32)


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One call of `_hip.moe_experts`.  path: g128 / g256 (grouped, by tile size) or decode.  counts: per-expert targets for
    route_from_counts (None: route_decode).  prefix_of: take the first T tokens of that case's inputs and routing."""

    def __init__(self, name, E, k, T, counts=None, D=256, F=512, order="asc", w2_density=1 / 16, gauss=False, prefix_of=None,
                 mutants=True):
        self.name, self.E, self.k, self.T, self.D, self.F = name, E, k, T, D, F
        self.counts, self.order, self.w2_density, self.gauss, self.prefix_of, self.mutants = counts, order, w2_density, gauss, prefix_of, mutants
        self.path = "decode" if T <= GEMV_MAX_T else ("g256" if tile_rows_for(T, k, E, D, F) == 256 else "g128")
        assert E <= MOE_MAX_E and k in (1, 2, 4) and k <= E

    def __repr__(self):
        return self.name


def _spread(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


G128_CASES = [
    Case("e8k2t300-edges", 8, 2, 300, (0, 1, 127, 128, 129, 215, 0, 0)),
    Case("e4k2t520-wrap", 4, 2, 520, (520, 257, 256, 7)),
    Case("e8k2t516-16tiles", 8, 2, 516, (129,) * 8),
    Case("e16k4t100-order", 16, 4, 100, tuple([100] * 3 + _spread(100, 12) + [0]), order="mixed"),
    Case("e2k1t200-empty0", 2, 1, 200, (0, 200)),
    Case("e2k2t520-k264", 2, 2, 520, (520, 520), D=264, F=520),
]
SWITCH_512 = Case("e2k2t512-switch", 2, 2, 512, (512, 512))
SWITCH_511 = Case("e2k2t511-switch", 2, 2, 511, prefix_of=SWITCH_512)
G256_CASES = [
    Case("e3k2t768-ragged255", 3, 2, 768, (768, 767, 1)),
    Case("e2k1t1024-empty0", 2, 1, 1024, (0, 1024)),
    Case("e4k4t512-order", 4, 4, 512, (512,) * 4, order="mixed"),
    SWITCH_512,
]
DECODE_CASES = [Case(f"decode-k{k}t{T}f{F}", 8, k, T, D=264, F=F, order="mixed")
                for k in (1, 2, 4) for T in (1, 3, 8) for F in (264, 520, 1544)]
LDS_EDGE_CASES = [           # top_k * F * 2 == 65536, the decode combine kernel's whole LDS
    Case("decode-lds-k4f8192", 4, 4, 8, F=8192, order="mixed", w2_density=1 / 256, mutants=False),
    Case("decode-lds-k2f16384", 4, 2, 8, F=16384, order="mixed", w2_density=1 / 512, mutants=False),
]
EXACT_CASES = G128_CASES + [SWITCH_511] + G256_CASES + DECODE_CASES + LDS_EDGE_CASES
GAUSS_CASES = [
    Case("gauss-decode-k4t8", 8, 4, 8, order="mixed", gauss=True),
    Case("gauss-e8k2t300-edges", 8, 2, 300, (0, 1, 127, 128, 129, 215, 0, 0), gauss=True),
]
assert [c.path for c in G128_CASES + [SWITCH_511]] == ["g128"] * 7 and [c.path for c in G256_CASES] == ["g256"] * 4


class Inputs:
    """x [T, D], h [T, D] bf16; experts [(W1 [F, D], W2 [D, F], W3 [F, D])] bf16; sel_idx int32 [T, k]; sel_w fp32 [T, k]."""

    def __init__(self, x, h, experts, sel_idx, sel_w):
        self.x, self.h, self.experts, self.sel_idx, self.sel_w = x, h, experts, sel_idx, sel_w


def _tern(shape, g, density):
    """{-1, 0, 1}: nonzero with probability `density`, sign fair."""
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1
    keep = torch.rand(shape, generator=g) < density
    return (sign * keep).to(BF)


@functools.lru_cache(maxsize=None)
def _experts(E, D, F, density, gauss):
    out = []
    for e in range(E):
        g = torch.Generator().manual_seed(9000 + 131 * e + D + 7 * F)
        if gauss:
            out.append(((torch.randn(F, D, generator=g) * D ** -0.5).to(BF), (torch.randn(D, F, generator=g) * F ** -0.5).to(BF),
                        (torch.randn(F, D, generator=g) * D ** -0.5).to(BF)))
            continue
        w1 = _tern((F, D), g, 0.5)
        w1[:, 0] = 16.0
        out.append((w1, _tern((D, F), g, density), _tern((F, D), g, 2 / 3)))
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    if case.prefix_of is not None:
        p, T = inputs(case.prefix_of), case.T
        return Inputs(p.x[:T].clone(), p.h[:T].clone(), p.experts, p.sel_idx[:T].clone(), p.sel_w[:T].clone())
    E, k, T, D, F = case.E, case.k, case.T, case.D, case.F
    g = torch.Generator().manual_seed(5000 + 17 * T + 3 * k + E)
    if case.gauss:
        x = torch.randn(T, D, generator=g).to(BF)
        h = (2.0 * torch.randn(T, D, generator=g)).to(BF)
    else:
        x = torch.randint(-2, 3, (T, D), generator=g).to(BF)
        x[:, 0] = 8.0
        h = (8 * torch.randint(-128, 129, (T, D), generator=g)).to(BF)
    sel_idx = route_decode(T, k, E, case.order) if case.counts is None else route_from_counts(T, k, case.counts, case.order)
    return Inputs(x, h, _experts(E, D, F, case.w2_density, case.gauss), sel_idx, slot_weights(T, k))


# -------------------------------------------------------------------------------------------------------- fp64 reference
def _bf(v):
    return v.to(BF).double()


@functools.lru_cache(maxsize=None)
def reference(case):
    """(out bf16 [T, D], S fp64 [T, D]): the rounding chain of the module docstring; S = |h| + sum_k w_k (|W2_e| |hid_e|).
    Exact family: also asserts bf16(silu(a)) == a."""
    inp = inputs(case)
    T, D = inp.x.shape
    R = torch.zeros(T, D, dtype=torch.float64)
    S = inp.h.double().abs()
    for e, (w1, w2, w3) in enumerate(inp.experts):          # ascending id: the order in which moe.py:29-31 rounds
        tok, slot = torch.where(inp.sel_idx == e)
        if tok.numel() == 0:
            continue
        xe = inp.x[tok].double()
        a, b = _bf(xe @ w1.double().T), _bf(xe @ w3.double().T)
        s = _bf(a / (1.0 + torch.exp(-a)))
        if not case.gauss:
            assert torch.equal(s, a), case
        hid = _bf(s * b)
        y = _bf(hid @ w2.double().T)
        w = inp.sel_w[tok, slot].double()[:, None]
        R[tok] = _bf(R[tok] + _bf(w * y))
        S[tok] += w * (hid.abs() @ w2.double().abs().T)
    return (inp.h.double() + R).to(BF), S


def conditions(case):
    """The generator's two conditions for every routed pair; returns (a min, a max, [sum|term| max per contraction])."""
    inp = inputs(case)
    lo, hi, bound = 1e30, -1e30, [0.0, 0.0, 0.0]
    for e, (w1, w2, w3) in enumerate(inp.experts):
        tok = torch.where(inp.sel_idx == e)[0]
        if tok.numel() == 0:
            continue
        xe = inp.x[tok].double()
        a, b = _bf(xe @ w1.double().T), _bf(xe @ w3.double().T)
        hid = _bf(a * b)
        y = _bf(hid @ w2.double().T)
        lo, hi = min(lo, float(a.min())), max(hi, float(a.max()))
        for i, v in enumerate((xe.abs() @ w1.double().abs().T, xe.abs() @ w3.double().abs().T, hid.abs() @ w2.double().abs().T)):
            bound[i] = max(bound[i], float(v.max()))
        assert float(y.abs().max()) < 2 ** 19, case        # combine: multiples of 1/32 below 2^19 add exactly in fp32
    assert 24 <= lo and hi <= 256, (case, lo, hi)
    assert max(bound) < 2 ** 24, (case, bound)
    return lo, hi, bound


def tolerance(S):
    return GAUSS_C * 2.0 ** -7 * S + 1e-6


def gauss_ratio(got, ref, S):
    """max over elements of |got - ref| / (2^-7 S) (the quantity c bounds)."""
    return float(((got.double() - ref.double()).abs() / (2.0 ** -7 * S)).max())


# ------------------------------------------------------------------------------------------------------------ emulations
def _mm(a, w, skip=None):
    """fp32 [m, n] = a [m, K] @ w [n, K]^T: 64-wide K slices visited in reversed order, each slice's partial product formed in
    fp64 and rounded once to fp32, fp32 accumulation across slices.  skip: index of a slice left out (mutant)."""
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    a64, w64 = a.double(), w.double()
    for s in reversed(range((K + KS - 1) // KS)):
        if s == skip:
            continue
        acc = acc + (a64[:, s * KS:(s + 1) * KS] @ w64[:, s * KS:(s + 1) * KS].T).float()
    return acc


def _swiglu(acc1, acc3, keep_fp32=False):
    """common.cuh swiglu_bf / swiglu_bf_fast + the caller's rounding: bf16(bf16(silu(bf16 a)) * bf16 b)."""
    a, b = acc1.to(BF).double(), acc3.to(BF).double()
    s = (a / (1.0 + torch.exp(-a))).float().to(BF).float()
    hid = s * b.float()
    return hid if keep_fp32 else hid.to(BF).float()


def _pick_slice(K, which):
    n = (K + KS - 1) // KS
    return {"first": 0, "middle": n // 2, "last": n - 1}[which]


def moe_lists(sel_idx, E, tile_rows, empty_tile=False):
    """moe_lists_kernel with rows inside an expert in ascending (token, slot) order (the kernel's order there is arbitrary).
    Returns tok_of [M], row_of [T, k], tiles [(expert, first row, valid rows)]."""
    T, k = sel_idx.shape
    flat = sel_idx.reshape(-1).long()
    cnt = torch.bincount(flat, minlength=E).tolist()
    order = torch.sort(flat, stable=True).indices
    tok_of = (order // k).clone()
    row_of = torch.empty(T * k, dtype=torch.long)
    row_of[order] = torch.arange(T * k)
    tiles, o = [], 0
    for e in range(E):
        for r in range(0, cnt[e], tile_rows):
            tiles.append((e, o + r, min(tile_rows, cnt[e] - r)))
        o += cnt[e]
    return tok_of, row_of.view(T, k), tiles


def _combine(y, h, sel_idx, sel_w, row, sort=True):
    """moe_combine_kernel / the tail of moe_w2_kernel: per token the picks sorted by expert id (sort=False: slot order), a
    bf16 running sum from zero of bf16(w y), then bf16(h + R).  y: fp32 rows (bf16 values); row [T, k]: y row of (t, slot)."""
    T, k = sel_idx.shape
    pos = torch.argsort(sel_idx.long(), dim=1, stable=True) if sort else torch.arange(k).expand(T, k)
    r = torch.zeros(T, y.shape[1], dtype=torch.float32)
    for j in range(k):
        rows = torch.gather(row, 1, pos[:, j:j + 1])[:, 0]
        w = torch.gather(sel_w, 1, pos[:, j:j + 1])
        r = (r + (w * y[rows]).to(BF).float()).to(BF).float()
    return (h.float() + r).to(BF)


GROUPED_MUTANTS = ["last_row_dropped", "row_past_written", "next_expert_weights", "empty_expert_tile", "w1_w3_exchanged",
                   "tok_of_off_by_one", "combine_slot_order", "slot_weights_exchanged", "hid_fp32",
                   "w13_kskip_first", "w13_kskip_middle", "w13_kskip_last", "w2_kskip_first", "w2_kskip_middle", "w2_kskip_last",
                   "table128_tiles256"]
DECODE_MUTANTS = ["w1_w3_exchanged", "combine_slot_order", "slot_weights_exchanged", "slot_of_identity", "hid_fp32",
                  "w13_kskip_first", "w13_kskip_middle", "w13_kskip_last", "w2_kskip_first", "w2_kskip_middle", "w2_kskip_last"]


def _exchange_weights(sel_w, t):
    w = sel_w.clone()
    w[t, 0], w[t, 1] = sel_w[t, 1], sel_w[t, 0]
    return w


def grouped_emulation(case, mutant=None):
    """mi_moe_grouped_gemm in torch.  Returns out bf16 [T, D], or None where `mutant` has nothing to break in this case.
    Scratch rows that no tile writes read as zero."""
    inp = inputs(case)
    E, k, T, D, F = case.E, case.k, case.T, case.D, case.F
    M = T * k
    tr = tile_rows_for(T, k, E, D, F)
    grid_tiles = max_m_tiles(T, k, E, tr)
    if mutant == "table128_tiles256":
        if tr != 256:
            return None
        tr = 128
    tok_of, row_of, tiles = moe_lists(inp.sel_idx, E, tr)
    if mutant == "table128_tiles256" and len(tiles) <= grid_tiles:
        return None
    assert mutant == "table128_tiles256" or len(tiles) <= grid_tiles
    tiles = [list(t) + [t[0]] for t in tiles[:grid_tiles]]      # (expert, row0, rows valid, expert whose weights are used)
    sel_w, sort = inp.sel_w, True
    last = None                                                 # a faulty tile that runs after all the others
    mid = len(tiles) // 2
    if mutant == "last_row_dropped":
        ragged = [t for t in tiles if t[2] < tr]
        if not ragged:
            return None
        ragged[0][2] -= 1
    elif mutant == "row_past_written":
        cand = [t for t in tiles if t[2] < tr and t[1] + t[2] < M]
        if not cand:
            return None
        tiles.remove(cand[0])
        cand[0][2] += 1
        last = cand[0]
    elif mutant == "next_expert_weights":
        cand = [t for t in tiles if t[0] + 1 < E]
        if not cand:
            return None
        cand[len(cand) // 2][3] += 1
    elif mutant == "empty_expert_tile":
        cnt = torch.bincount(inp.sel_idx.reshape(-1).long(), minlength=E).tolist()
        cand = [(e, sum(cnt[:e])) for e in range(E) if cnt[e] == 0 and sum(cnt[:e]) < M]
        if not cand:
            return None
        last = [cand[0][0], cand[0][1], 1, cand[0][0]]
    elif mutant == "tok_of_off_by_one":
        tok_of = tok_of.clone()
        tok_of[M // 2] += 1 if tok_of[M // 2] + 1 < T else -1
    elif mutant == "combine_slot_order":
        sort = False
    elif mutant == "slot_weights_exchanged":
        if k < 2:
            return None
        sel_w = _exchange_weights(sel_w, T // 2)
    hid = torch.zeros(M, F, dtype=torch.float32)
    y = torch.zeros(M, D, dtype=torch.float32)
    order = tiles + ([last] if last is not None else [])
    for ti, (e, row0, rv, ew) in enumerate(order):
        w1, _, w3 = inp.experts[ew]
        if mutant == "w1_w3_exchanged":
            w1, w3 = w3, w1
        skip = _pick_slice(D, mutant.split("_")[-1]) if (mutant or "").startswith("w13_kskip") and ti == mid else None
        a = inp.x[tok_of[row0:row0 + rv]]
        hid[row0:row0 + rv] = _swiglu(_mm(a, w1, skip), _mm(a, w3, skip), keep_fp32=mutant == "hid_fp32")
    for ti, (e, row0, rv, ew) in enumerate(order):
        skip = _pick_slice(F, mutant.split("_")[-1]) if (mutant or "").startswith("w2_kskip") and ti == mid else None
        y[row0:row0 + rv] = _mm(hid[row0:row0 + rv], inp.experts[ew][1], skip).to(BF).float()
    return _combine(y, inp.h, inp.sel_idx, sel_w, row_of, sort)


def decode_emulation(case, mutant=None):
    """mi_moe_experts_decode in torch: GEMV_MOE_W13 writes hid row t k + slot with the slot's expert; moe_w2_kernel sorts the
    token's experts by id and reads the hidden row slot_of[sorted position].  None where the mutant has nothing to break."""
    inp = inputs(case)
    k, T, D, F = case.k, case.T, case.D, case.F
    if mutant in ("slot_weights_exchanged", "slot_of_identity", "combine_slot_order") and k < 2:
        return None
    skip13 = _pick_slice(D, mutant.split("_")[-1]) if (mutant or "").startswith("w13_kskip") else None
    skip2 = _pick_slice(F, mutant.split("_")[-1]) if (mutant or "").startswith("w2_kskip") else None
    sel_w = _exchange_weights(inp.sel_w, T // 2) if mutant == "slot_weights_exchanged" else inp.sel_w
    hid = []                                                    # GEMV_MOE_W13: row t k + slot, by the slot's expert
    for t in range(T):
        for slot in range(k):
            w1, _, w3 = inp.experts[int(inp.sel_idx[t, slot])]
            if mutant == "w1_w3_exchanged":
                w1, w3 = w3, w1
            xa = inp.x[t:t + 1]
            hid.append(_swiglu(_mm(xa, w1, skip13), _mm(xa, w3, skip13), keep_fp32=mutant == "hid_fp32"))
    out = torch.empty(T, D, dtype=BF)
    for t in range(T):                                          # moe_w2_kernel: one token per blockIdx.y
        pos = list(range(k)) if mutant == "combine_slot_order" else torch.argsort(inp.sel_idx[t].long(), stable=True).tolist()
        r = torch.zeros(1, D, dtype=torch.float32)
        for p, slot in enumerate(pos):
            src = p if mutant == "slot_of_identity" else slot
            yv = _mm(hid[t * k + src], inp.experts[int(inp.sel_idx[t, slot])][1], skip2).to(BF).float()
            r = (r + (float(sel_w[t, slot]) * yv).to(BF).float()).to(BF).float()
        out[t] = (inp.h[t:t + 1].float() + r).to(BF)[0]
    return out


def emulate(case, mutant=None):
    return decode_emulation(case, mutant) if case.path == "decode" else grouped_emulation(case, mutant)


def mutants_of(case):
    return DECODE_MUTANTS if case.path == "decode" else GROUPED_MUTANTS


def describe_rows(case, rows, limit=12):
    """For a mismatch report: per differing token its experts and, on the grouped path, the m-tile of each (token, slot)
    pair in the emulation's row order (inside an expert the kernel's own order is arbitrary, so the tile is nominal)."""
    inp = inputs(case)
    out = []
    if case.path == "decode":
        return [(int(t), inp.sel_idx[t].tolist()) for t in rows[:limit]]
    tr = tile_rows_for(case.T, case.k, case.E, case.D, case.F)
    _, row_of, tiles = moe_lists(inp.sel_idx, case.E, tr)
    for t in rows[:limit]:
        where = []
        for s in range(case.k):
            r = int(row_of[t, s])
            ti = next(i for i, (_, r0, rv) in enumerate(tiles) if r0 <= r < r0 + rv)
            where.append((int(inp.sel_idx[t, s]), ti, r - tiles[ti][1]))
        out.append((int(t), where))
    return out
