"""The dense linears (`_hip.linear`, `_hip.qkv_rope_kvwrite`: gemv.hip / gemv_core.cuh at M <= 8, gemm.hip and gemm256.hip above,
generic.hip and the fp16 compile of gemm256.hip for fp16 storage) on inputs whose every contraction is an EXACT integer sum, one
fp64 reference with an explicit rounding at every rounding point of the model, a mirror of the launchers' routing, torch
emulations of the GEMV unit loop and of the tiled GEMMs, and single-fault mutants (helpers for test_linear_cases_host.py and
test_gpu_linear_structured.py; no test functions here).

Why: the operator tests use N(0,1) activations and N(0,1/K) weights under bounds of 1 - 2 bf16 ulp, because fp32 summation order
is not fixed.  One wrong 16-byte weight piece is about 2 ulp at K = 14336, one wrong product well under 1, and the rounding
chain (the residual added to bf16(Wx), SwiGLU on rounded a and b, logits widened from bf16) is not tested at all.

Plain family (every value an integer that bf16 and fp16 hold; fp32 accumulation gives the same bits in any order):
  W         dense, {-1, +1}
  x[t]      every 8-element piece has exactly ONE nonzero, +-1, at a position drawn per (token, piece).  With an even piece count
            P = K / 8 <= 48 (or fewer than 4096 outputs, where 10 % is not a stable share) the nonzero of piece 0 is +-2: a sum of
            P signs is 0 with probability C(P, P/2) / 2^P (50 % at P = 2, 27 % at P = 8, 16 % at P = 24, 10 % at P = 64), and with
            the 2 the sum is odd, never 0.
  y         a sum of P signs: every weight piece of every row moves every token's output by at least 1
  res       integers in [-R, R], R = min(64, 256 - max|y|), so that |res + y| <= 256
  SwiGLU    moe_cases' device: x[:, 0] = 8 (piece 0 is the carrier alone), W1[:, 0] = 16: a = 128 +- noise, W3[:, 0] = +-1
conditions() asserts |y| <= 256 (every output a bf16 integer: a change of 1 is visible), sum|w x| < 2^24, fewer than 15 % zeros,
24 <= a <= 256 (there 1 + exp(-a) == 1.0f: bf16(silu(a)) == a for swiglu_bf and swiglu_bf_fast), and that outputs a fault would
confuse differ: the output shifted by 1, 2, 64, 128 or 256 rows (columns) differs from itself in at least a quarter of ALL
entries (K >= 16, at least 64 entries compared), and ANY two rows (columns) - all pairs up to 64 rows, 512 drawn pairs above -
in at least a quarter of the entries where a row (column) is >= 32 long and K >= 64.  SwiGLU: fewer than 15 % of b are 0 (a
zero b is a zero output).  (Pair by pair at every size cannot hold: at M = 1 a column is one number, at K = 8 that number is
+-W[n, j] with j the token's one nonzero, so that N = 3 columns cannot all differ and two tokens with the same j give equal or
opposite rows.)

Rounding-point family (RESIDUAL, LOGITS, SWIGLU, q|k|v; K >= 16): x[:, 0] = 8, x[:, 1] = 1 and W[n, 0] = +-c, c walking through
[56, 104] with n, W[n, 1] = n % 2 (both parities of y) lift the sums into 256 < |y| < 1024, where bf16 holds every 2nd (below
512) or 4th integer.  Asserted: at least a quarter of the sums are not bf16 values, at least 5 % are exact ties, res in [-7, 7]
gives bf16(res + bf16(y)) != bf16(res + y) in at least 5 % of the outputs; SwiGLU keeps a = 128 +- noise exact and lifts b the
same way (bf16(b) != b).  fp16 holds every integer below 2048, so the fp16 cases take x[:, 0] = 64: 2048 < |y| < 8192, where
fp16 holds every 2nd (below 4096) or 4th integer, under the same three shares and the same rounding mutants.

q|k|v leaf: the rounding-point family through `mi_qkv_rope_kvwrite` with a rope_cs table of our own: (cos, sin) are dyadics of at
most two bits - (1, 0), (0, 1), (-1, 0), (.5, .5), (.75, -.25), (0, -1), (-.5, .75), (.25, 1), (1.5, .5): not rotations, all
different, the entry of (position, pair) is number (7 pos + 3 pair) % 9 - so that bf16(y0) c - bf16(y1) s is exact in fp32
and rounds once.  Positions 5, 29, 24, 3, 46, 26, 31, 9 (distinct mod 9: no two tokens share a (cos, sin) row), ring W = 24,
tok_seq[t] = T - t (a non-identity map into T + 2 ring rows), every slot the call must not touch keeps the sentinel.  Six
cases run the PLAIN family through the leaf (|y| < 128: (3 y0 + y1) / 4 is exact in bf16, so a dropped piece shows in every
token).  No fused norm here: rsqrt(ms + eps) is not exact, and the fused forms stay with the tolerance tests of test_gpu_ops.py
and test_gpu_fp8.py.

Reference (reference()): fp64 sums, then .to(bfloat16) (fp16 cases: .to(float16)) at every rounding point of
transformer_layers.py:66-70, 93, 105-106, 166-168, rope.py:13-23, cache.py:83-92: y = bf16(W x); residual bf16(res + y); logits
float(y); SwiGLU bf16(bf16(silu(bf16 a)) bf16 b); q, k = bf16(rope(bf16 y)), v = bf16 y, k | v into slot pos % W of row tok_seq.

Measured on the CPU over all cases at 256 CUs, from the reference alone (test_linear_cases_host.py prints them): plain family
max|y| = 185 (K = 28672), sum|w x| <= 3585, zeros at most 10.8 % of a case's outputs, the closest pair of rows or columns differs
in 68 % of its entries; plain SwiGLU a in [45, 200], |b| <= 72, b == 0 in at most 11.8 %; rounding family (bf16) 331 <= |y| <= 942,
sum|w x| <= 2112, sums that are not bf16 values 60.8 .. 78.4 % of a case, exact ties 21.9 .. 38.2 %, bf16(res + bf16(y)) !=
bf16(res + y) in 18.8 .. 35.5 %; rounding-family SwiGLU a in [47, 205], 385 <= |b| <= 878; rounding family (fp16) 3500 <= |y| <= 6745,
sum|w x| <= 7168, not fp16 values 68.3 .. 71.1 %, ties 28.9 .. 31.1 %, double rounding visible in 25.5 .. 26.8 %.

Route mirror: route(M, K, N, epi, cus) follows api.hip linear_group -> gemv_pass_loop / launch_gemv (gemv_max_tokens, round_tt,
stage_by_dma, lds_bytes, blocks_for_lds, even_blocks, spread_blocks, the 5 .. 7-wave search) or launch_gemm (gemm256_applicable,
the tail split, gemm256_half_applicable), and generic.hip launch_g_linear for fp16.  Labels:
  gemv/TT=6[/dma][/2-pass]  gemv/nw=5  g128/dma  g128/regstage  g256  g256+half  g256+g128tail  f16/g256  f16/generic
block_plan() names how the GEMV grid is sized: even-k5, spread-k2, nw-k2-3-per-cu (units per wave, blocks per CU), 1-per-cu
(above 80 KiB of LDS); a case that is about the grid carries that label too (Case.blocks).  The 5 .. 7-wave search takes
k = 1 while the row pairs are at most 16 cus (N = 20 cus: 2 cus blocks of one unit per wave) and k = 2 above (N = 60 cus: 3 cus
blocks whose waves walk two units each, the `u += nwaves` loop with the load cursor running across units).

Emulations (CPU torch; fp32 sums, exact here): gemv_emulation - passes of gemv_max_tokens rows, row pairs, the odd last row's
aliased partner, segment lookup per row, chunks of 64 pieces, batches of 4 chunks with the tail pieces clamped to the row's
last piece and skipped, the epilogue per mode, the ring write; gemm_emulation - the launches of the route (column_slice for
the tail split), m / n tiles, rows clamped to the last valid one, segment rows per tile row, 64-wide K slices accumulated in
reversed order, the epilogue, stores only inside the tile's valid rows and columns.  Both write into the guarded buffer and are
bit-equal to the reference on every case.

Mutants (test_linear_cases_host.py; "seen / applies" counts cases at 256 CUs, then the largest number of differing elements).
A mutant applies where the structure it breaks exists (K % 512 != 0, an odd N, a second segment, a second pass, a ragged
tile, ...).  A mutant that SUBSTITUTES one operand for another - a piece, a row, a token - is placed on the first candidate from
the middle whose substitute multiplies differently; the row substitutions (odd row, segment boundary) have one place only, and
where the two rows' exact sums agree for every token no test can see them: the host test proves exactly that for each such
case (the "=" column), and they occur only at M = 1 or K <= 16.  The W1 / W3 exchange is likewise unseen where bf16(silu(b)) == b for
every b (two cases of one or two outputs with b = 8 or so: silu(a) b == silu(b) a).

  mutant                     gemv              =   qkv              g128              g256 (+ tail)      f16
  piece_dropped_first        333/333 8         -   6/6     24       54/54   1030      26/26   4096       7/7     1030
  piece_dropped_middle       333/333 8         -   6/6     24       54/54   1030      26/26   4096       7/7     1030
  piece_dropped_last         333/333 8         -   6/6     24       54/54   1030      26/26   4096       7/7     1030
  piece_from_neighbour       296/296 7         -   6/6     16       48/48   787       26/26   1532       7/7     627
  tail_counted_again         238/238 8         -   -                -                 -                  -
  x_piece_from_neighbour     275/275 7702      -   4/4     5120     53/53   589       26/26   3045       7/7     324
  odd_row_from_partner       118/118 8         2   -                -                 -                  -
  partner_dropped            120/120 8         -   -                -                 -                  -
  seg_wrong_n0               162/162 8         3   62/62   24       28/28   1030      16/16   4000       8/8     1030
  seg_wrong_n1               122/122 8         5   62/62   16       23/23   1030      16/16   4000       8/8     1030
  w1_w3_exchanged            122/122 319       2   -                24/24   126547    12/12   96354      -
  pass_operands              2/2     74        -   8/8     12280    -                 -                  -
  residual_before_rounding   47/47   144       -   -                13/13   79219     9/9     6556691    8/8     72454
  logits_not_rounded         46/46   373       -   -                12/12   844329    6/6     465193     8/8     465233
  ab_not_rounded             46/46   123       -   -                12/12   53072     6/6     31236      -
  hid_truncated              46/46   251       -   -                12/12   100819    6/6     58994      -
  round_half_away            139/139 146       -   56/56   7922     37/37   175745    21/21   6818778    16/16   95895
  cs_neighbour_pair          -                 -   62/62   126      -                 -                  -
  pos_other_token            -                 -   44/44   3072     -                 -                  -
  k_slot_pos                 -                 -   30/30   10240    -                 -                  -
  k_seq_t                    -                 -   25/25   28672    -                 -                  -
  v_rotated                  -                 -   62/62   14330    -                 -                  -
  ragged_row_dropped         -                 -   -                80/80   128       34/34   256        19/19   256
  ragged_col_dropped         -                 -   -                75/75   128       30/30   256        20/20   256
  row_past_written           -                 -   -                80/80   128       34/34   256        19/19   256
  col_past_written           -                 -   -                75/75   128       30/30   256        20/20   256
  kslice_first               -                 -   -                91/91   16384     47/47   65536      23/23   65536
  kslice_middle              -                 -   -                91/91   16384     47/47   47650      23/23   47718
  kslice_last                -                 -   -                91/91   16384     47/47   47766      23/23   47779
  next_ntile_rows            -                 -   -                60/60   16384     31/31   65536      17/17   65497
  tail_c0_off                -                 -   -                -                 4/4     1048576    -
The piece and activation mutants apply to the plain family only: above 256 a sum moved by 1 can round to the same bf16 value.
"hid left in fp32" has no form in a leaf whose OUTPUT is hid, stored as bf16; its nearest fault is the product truncated to
bf16 instead of rounded (hid_truncated).  The rounding mutants apply to the rounding-point family only.
"""
import functools
import math

import torch

BF, F16 = torch.bfloat16, torch.float16
STORE, RESIDUAL, SWIGLU, LOGITS, QKV = "store", "residual", "swiglu", "logits", "qkv"
EPI_CODE = {STORE: 0, RESIDUAL: 1, SWIGLU: 2, LOGITS: 3}       # _hip.EPI_*
GEMV_MAX_T = 8                      # kernels.h
GEMV_LDS_BUDGET = 144 * 1024        # kernels.h
SENT = -0.3125                      # guard value: no output of either family (integers; RoPE results are multiples of 1/4)
HEAD = 128
RING_W = 24
POSITIONS = [5, 29, 24, 3, 46, 26, 31, 9]
ROPE_LEN = 48
CS = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.5, 0.5), (0.75, -0.25), (0.0, -1.0), (-0.5, 0.75), (0.25, 1.0), (1.5, 0.5)]


# ------------------------------------------------------------------------------------------------------------ route mirror
def gemv_max_tokens(K):
    t = GEMV_LDS_BUDGET // (K * 2)
    if t in (5, 7):                 # 5 and 7 rows run on the 6- and 8-row instantiations, which stage 6 / 8 rows
        t -= 1
    return max(1, min(GEMV_MAX_T, t))


def passes(M, K):
    """api.hip gemv_pass_loop: [(first row, rows)]."""
    cap = gemv_max_tokens(K)
    return [(t0, min(cap, M - t0)) for t0 in range(0, M, cap)]


def round_tt(T):
    return 6 if T == 5 else (8 if T == 7 else T)


def lds_bytes(TT, K, norm=False):
    return TT * K * 2 + 4 * TT * 4 + (K * 2 if TT > 1 and norm else 0)


def norm_mode(epi):
    """gemv_core.cuh norm_mode: the modes whose prologue is the fused-RMSNorm one (4 x 256 pieces in registers), with or without a norm."""
    return epi in (QKV, SWIGLU, LOGITS)


def stage_by_dma(epi, TT, K):
    return TT > 1 and TT * (K >> 3) > (4 if norm_mode(epi) else 8) * 256


def dma_edge(epi, TT):
    """(the last K staged through registers, the first K staged by LDS-DMA) at TT rows."""
    K = 8
    while not stage_by_dma(epi, TT, K + 8):
        K += 8
    return K, K + 8


def max_blocks(cus):
    return 2 * cus


def even_blocks(units, cus):
    for k in range(1, 65):
        b = (units + 4 * k - 1) // (4 * k)
        if b <= 4 * cus and b % cus == 0 and b * 4 * k == units and (b <= max_blocks(cus) or k == 1):
            return b, k
    return 0, 0


def spread_blocks(units, cap):
    k = (units + 4 * cap - 1) // (4 * cap)
    return max(1, (units + 4 * k - 1) // (4 * k)), k


def gemv_plan(T, K, N, epi, cus):
    """One launch_gemv call of T <= gemv_max_tokens(K) rows."""
    units = N if epi == SWIGLU else (N + 1) // 2
    blocks, k = even_blocks(units, cus)
    how, nw = ("even" if blocks else None), 4
    if not blocks and T == 1 and epi in (STORE, RESIDUAL) and K * 2 <= 48 * 1024:
        for w in (5, 6, 7):
            for kk in range(1, 17):
                b = units // (w * kk)
                if nw == 4 and b >= cus and b % cus == 0 and b * w * kk == units and b * w <= 16 * cus:
                    nw, blocks, k, how = w, b, kk, "nw"
    if not blocks:
        (blocks, k), how = spread_blocks(units, max_blocks(cus)), "spread"
    TT = round_tt(T)
    lds = lds_bytes(TT, K)
    one_per_cu = lds > 80 * 1024 and blocks > cus
    if one_per_cu:
        blocks, k = spread_blocks(units, cus)
    return dict(TT=TT, nw=nw, dma=nw == 4 and stage_by_dma(epi, TT, K), blocks=blocks, k=k, how=how, lds=lds, one_per_cu=one_per_cu)


def block_plan(M, K, N, epi, cus):
    """How launch_gemv sizes the grid of the first pass: even-k<units per wave>, spread-k<..>, nw-k<units per wave>-<blocks per CU>-per-cu, or
    1-per-cu (above 80 KiB of LDS)."""
    p = gemv_plan(passes(M, K)[0][1], K, N, epi, cus)
    if p["one_per_cu"]:
        return "1-per-cu"
    return f"nw-k{p['k']}-{p['blocks'] // cus}-per-cu" if p["how"] == "nw" else f"{p['how']}-k{p['k']}"


def gemm256_applicable(M, K):
    return K % 64 == 0 and K >= 128 and M >= 256


def tail_split(M, N, epi, cus, tail):
    """gemm.hip launch_gemm below gemm256_applicable: None (one launch) or (c0, 'half' | 'g128')."""
    nout = 128 if epi == SWIGLU else 256
    m_tiles, n_tiles = (M + 255) // 256, (N + nout - 1) // nout
    tiles = m_tiles * n_tiles
    rem = tiles % cus
    if tail and tiles > cus and rem != 0 and rem < cus * 3 // 4:
        step = cus // math.gcd(cus, m_tiles)
        n_first = (n_tiles // step) * step
        if 0 < n_first < n_tiles:
            half = tail >= 2 and rem * 2 <= cus and epi in (STORE, RESIDUAL)
            return n_first * nout, "half" if half else "g128"
    return None


def route(M, K, N, epi, cus, dtype="bf16", tail=2):
    """The label of the launches behind `_hip.linear` / `_hip.qkv_rope_kvwrite` (N: output columns; SwiGLU: rows of W1)."""
    if dtype == "f16":
        assert M > GEMV_MAX_T
        return "f16/g256" if gemm256_applicable(M, K) else "f16/generic"
    if M <= GEMV_MAX_T:
        ps = passes(M, K)
        p = gemv_plan(ps[0][1], K, N, epi, cus)
        parts = ["gemv", f"nw={p['nw']}" if p["nw"] != 4 else f"TT={p['TT']}"]
        if p["dma"]:
            parts.append("dma")
        if len(ps) > 1:
            parts.append(f"{len(ps)}-pass")
        return "/".join(parts)
    if not gemm256_applicable(M, K):
        return "g128/dma" if K % 64 == 0 else "g128/regstage"
    sp = tail_split(M, N, epi, cus, tail)
    return "g256" if sp is None else ("g256+half" if sp[1] == "half" else "g256+g128tail")


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One call.  segs: rows per weight segment (SwiGLU: one entry, the rows of W1 and of W3).  fam: plain / round.  path: the
    route label the case is meant to hit.  qkv: (H, Hkv, layout 'slot' | 'head' | None (no cache), tok_seq given)."""

    def __init__(self, name, M, K, segs, epi, path, fam="plain", dtype="bf16", tail=2, qkv=None, blocks=None):
        self.name, self.M, self.K, self.segs, self.epi, self.path, self.fam, self.dtype, self.tail, self.qkv, self.blocks = \
            name, M, K, tuple(segs), epi, path, fam, dtype, tail, qkv, blocks
        self.N = self.segs[0] if epi == SWIGLU else sum(self.segs)
        self.R = F16 if dtype == "f16" else BF
        self.odt = torch.float32 if epi == LOGITS else self.R
        assert K % 8 == 0 and (fam == "plain" or K >= 16) and 1 <= len(self.segs) <= 3

    def __repr__(self):
        return self.name

    @property
    def group(self):
        return "qkv" if self.epi == QKV else "f16" if self.dtype == "f16" else "gemv" if self.M <= GEMV_MAX_T else self.path[:4]

    @property
    def key(self):               # the inputs do not depend on the tail mode
        return (self.M, self.K, self.segs, self.epi, self.fam, self.dtype, self.qkv)


def _nm(M, K, segs, epi, fam, extra=""):
    return f"m{M}k{K}n{'+'.join(map(str, segs))}-{epi}{'-r' if fam == 'round' else ''}{extra}"


def _both(M, K, segs, epi, path, min_out=64, **kw):
    """A case in the plain family and, for the epilogues that round twice, also in the rounding-point family (K >= 16, and
    enough outputs that the shares mean something)."""
    N = segs[0] if epi == SWIGLU else sum(segs)
    tag = kw.pop("tag", "")
    out = [Case(_nm(M, K, segs, epi, "plain", tag), M, K, segs, epi, path, **kw)]
    if epi != STORE and K >= 16 and M * N >= min_out:
        out.append(Case(_nm(M, K, segs, epi, "round", tag), M, K, segs, epi, path, fam="round", **kw))
    return out


NSPECS = [(1,), (2,), (3,), (37,), (12, 13, 12), (12, 13, 13), (20, 21, 23), (64,), (30, 34)]
GEMV_KS = [8, 16, 504, 512, 520, 2040, 2048, 2056, 4104]
MODES = [STORE, RESIDUAL, LOGITS, SWIGLU]


def _gemv_label(T, K, epi):
    """Hand-written for the table below (K <= 4104: one pass, few units): rows beyond 2048 pieces (1024 in the norm-style modes)
    go by DMA."""
    dma = T > 1 and round_tt(T) * (K // 8) > (2048 if epi in (STORE, RESIDUAL) else 1024)
    return f"gemv/TT={round_tt(T)}" + ("/dma" if dma else "")


def gemv_cases(cus):
    out = []
    for iT, T in enumerate(range(1, 9)):
        for iK, K in enumerate(GEMV_KS):
            for im, epi in enumerate(MODES):
                segs = NSPECS[(iT + 2 * iK + 3 * im) % len(NSPECS)]
                segs = (sum(segs),) if epi == SWIGLU else segs
                out += _both(T, K, segs, epi, _gemv_label(T, K, epi))
    for T, K, segs, epi in ((1, 14336, (37,), STORE), (4, 14336, (20, 21, 23), RESIDUAL), (2, 28672, (64,), STORE), (1, 28672, (12, 13, 12), RESIDUAL)):
        dma = "/dma" if T > 1 else ""
        out += [Case(_nm(T, K, segs, epi, "plain"), T, K, segs, epi, f"gemv/TT={T}{dma}")]
    for TT in (2, 4, 8):            # stage_by_dma, one K step either side, derived from the function
        for epi, segs in ((STORE, (37,)), (RESIDUAL, (12, 13, 12)), (LOGITS, (38,)), (SWIGLU, (37,))):
            lo, hi = dma_edge(epi, TT)
            out += _both(TT, lo, segs, epi, f"gemv/TT={TT}", tag="-lastreg")
            out += _both(TT, hi, segs, epi, f"gemv/TT={TT}/dma", tag="-firstdma")
    out += _both(8, 10240, (12, 13, 12), RESIDUAL, "gemv/TT=6/dma/2-pass")           # 6 + 2 rows
    out += [Case(_nm(8, 10240, (64,), STORE, "plain"), 8, 10240, (64,), STORE, "gemv/TT=6/dma/2-pass")]
    out += [Case(_nm(6, 10240, (8 * cus + 16,), STORE, "plain"), 6, 10240, (8 * cus + 16,), STORE, "gemv/TT=6/dma", blocks="1-per-cu")]
    for w in (5, 6, 7):             # 5 .. 7-wave blocks: row pairs = cus w
        for epi in (STORE, RESIDUAL):
            out += [Case(_nm(1, 512, (2 * w * cus,), epi, "plain"), 1, 512, (2 * w * cus,), epi, f"gemv/nw={w}", blocks="nw-k1-1-per-cu")]
    for epi in (STORE, RESIDUAL):   # 30 cus pairs: past 16 cus the search takes k = 2 - every wave of the 5-wave blocks walks two units
        out += [Case(_nm(1, 512, (60 * cus,), epi, "plain"), 1, 512, (60 * cus,), epi, "gemv/nw=5", blocks="nw-k2-3-per-cu")]
    out += [Case(_nm(2, 512, (60 * cus,), RESIDUAL, "plain"), 2, 512, (60 * cus,), RESIDUAL, "gemv/TT=2", blocks="spread-k4"),
            Case(_nm(1, 512, (20 * cus,), STORE, "plain"), 1, 512, (20 * cus,), STORE, "gemv/nw=5", blocks="nw-k1-2-per-cu"),
            Case(_nm(2, 512, (10 * cus,), STORE, "plain"), 2, 512, (10 * cus,), STORE, "gemv/TT=2", blocks="spread-k1"),
            Case(_nm(2, 512, (20 * cus,), RESIDUAL, "plain"), 2, 512, (20 * cus,), RESIDUAL, "gemv/TT=2", blocks="spread-k2")]
    ek = next((j for j in range(1, 65) if even_blocks(j * cus, cus)[1] > 1), None)   # even_blocks with k > 1
    if ek is not None:
        k = even_blocks(ek * cus, cus)[1]
        out += [Case(_nm(3, 8, (2 * ek * cus,), STORE, "plain"), 3, 8, (2 * ek * cus,), STORE, "gemv/TT=3", blocks=f"even-k{k}")]
    out += [Case(_nm(3, 8, (2 * (8 * cus + 3) - 1,), STORE, "plain"), 3, 8, (2 * (8 * cus + 3) - 1,), STORE, "gemv/TT=3", blocks="spread-k2")]
    return out


def qkv_cases(cus):
    out = []
    variants = [("slot", True), ("head", False), (None, True)]
    i = 0
    for H, Hkv in ((4, 2), (8, 8)):     # the plain family, where one dropped piece is visible in every token: small sums rotate exactly
        for D, T in ((512, 1), (512, 8), (2560, 3)):
            path = f"gemv/TT={T}" + ("/dma" if T > 1 and T * D // 8 > 1024 else "")
            out.append(Case(f"qkv-h{H}kv{Hkv}d{D}t{T}-slot-seq-plain", T, D, (H * HEAD, Hkv * HEAD, Hkv * HEAD), QKV, path, qkv=(H, Hkv, "slot", True)))
    for H, Hkv in ((4, 2), (8, 8)):
        for D, T in [(D, T) for D in (512, 2560) for T in (1, 3, 8)] + [(10240, 8)]:
            extra = [("head", True), ("slot", False), (None, False)][i % 3]
            for layout, seq in variants + [extra]:
                if D == 10240:
                    path = "gemv/TT=6/dma/2-pass"
                else:
                    path = f"gemv/TT={T}" + ("/dma" if T > 1 and T * D // 8 > 1024 else "")
                name = f"qkv-h{H}kv{Hkv}d{D}t{T}-{layout or 'nocache'}-{'seq' if seq else 'noseq'}"
                out.append(Case(name, T, D, (H * HEAD, Hkv * HEAD, Hkv * HEAD), QKV, path, fam="round", qkv=(H, Hkv, layout, seq)))
            i += 1
    return out


G128_MS = [9, 127, 128, 129, 255, 1030]
G128_KS = [64, 128, 192, 8, 72, 200, 520]
G128_NS = [(8,), (120,), (128,), (136,), (1160,), (40, 50, 46), (128, 8), (300, 500, 360), (128, 128, 64)]


def g128_cases(cus):
    out, i = [], 0
    for M in G128_MS:
        for K in G128_KS:
            if gemm256_applicable(M, K):
                continue
            segs, epi = G128_NS[i % len(G128_NS)], MODES[(i + i // len(G128_NS)) % 3]      # (SwiGLU below)
            out += _both(M, K, segs, epi, "g128/dma" if K % 64 == 0 else "g128/regstage")
            i += 1
    for j, N in enumerate((64, 72, 200)):
        for K, M in ((64, 129), (200, 300), (520, 1030), (192, 127)):
            out += _both(M if j else max(M - 100, 9), K, (N,), SWIGLU, "g128/dma" if K % 64 == 0 else "g128/regstage")
    out += _both(300, 200, (40, 50, 46), RESIDUAL, "g128/regstage")                  # M >= 256 where gemm256 declines
    out += _both(1030, 64, (1160,), LOGITS, "g128/dma")
    return out


G256_MS = [256, 257, 300, 1030]
G256_KS = [128, 192, 448, 4096]
G256_NS = [(8,), (256,), (264,), (200, 240, 200), (640,), (256, 256, 128)]


def g256_cases(cus):
    out, i = [], 0
    for M in G256_MS:
        for K in G256_KS:
            segs, epi = G256_NS[i % len(G256_NS)], MODES[(i + i // len(G256_NS)) % 3]
            out += _both(M, K, segs, epi, "g256")
            i += 1
    for N in (128, 136):
        for K, M in ((128, 256), (192, 257), (448, 1030)):
            out += _both(M, K, (N,), SWIGLU, "g256")
    out += _both(300, 4096, (200, 240, 200), RESIDUAL, "g256")
    return out


def tail_shape(cus):
    """(m_tiles, n_tiles) of 256 x 256 tiles for which launch_gemm splits the columns and the tail takes half-height tiles;
    16 x 24 where that is such a shape (256 CUs), else the smallest one found; None: no such shape at this CU count."""
    cands = [(16, 24)] + [(m, n) for m in (16, 8, 4, 2) for n in range(2, 65)]
    for m, n in cands:
        if route(m * 256, 128, n * 256, STORE, cus, tail=2) == "g256+half" and route(m * 256, 128, n * 256, STORE, cus, tail=1) == "g256+g128tail":
            return m, n
    return None


def tail_cases(cus):
    ts = tail_shape(cus)
    if ts is None:
        return []
    m, n = ts
    N = n * 256
    a = (N // 3 + 52) // 8 * 8          # three segments, both boundaries inside a tile
    segs = (a, a - 104, N - 2 * a + 104)
    out = []
    for M, epi, fam in ((m * 256, STORE, "plain"), (m * 256 - 96, RESIDUAL, "round")):
        for tail, path in ((2, "g256+half"), (1, "g256+g128tail"), (0, "g256")):
            out.append(Case(_nm(M, 128, segs, epi, fam, f"-tail{tail}"), M, 128, segs, epi, path, fam=fam, tail=tail))
    return out


def f16_cases(cus):
    out = []
    for c in g256_cases(cus):
        if c.epi != SWIGLU and c.fam == "plain":
            fam = "round" if c.epi != STORE else "plain"
            out.append(Case("f16-" + _nm(c.M, c.K, c.segs, c.epi, fam), c.M, c.K, c.segs, c.epi, "f16/g256", fam=fam, dtype="f16"))
    for M in (9, 300):
        for segs, epi in (((136,), STORE), ((40, 50, 46), RESIDUAL), ((72,), LOGITS)):
            fam = "round" if epi != STORE else "plain"
            out.append(Case("f16-" + _nm(M, 200, segs, epi, fam), M, 200, segs, epi, "f16/generic", fam=fam, dtype="f16"))
    return out


@functools.lru_cache(maxsize=None)
def all_cases(cus):
    """Every case, built for a device of `cus` compute units (the nw, block-count and tail-split shapes depend on it)."""
    out = gemv_cases(cus) + qkv_cases(cus) + g128_cases(cus) + g256_cases(cus) + tail_cases(cus) + f16_cases(cus)
    assert len({c.name for c in out}) == len(out), sorted(c.name for c in out)
    for c in out:
        c.cus = cus
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """x [M, K]; w: the segments ([n_i, K]; SwiGLU: W1, W3); res [M, N] or None; q|k|v: rope_cs [ROPE_LEN, 64, 2] fp32, tok_pos,
    tok_seq (or None) int32, ring shape."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _seed(case):
    mode = 4 if case.epi == QKV else MODES.index(case.epi)
    return (case.M * 1000003 + case.K * 10007 + sum((i + 1) * s for i, s in enumerate(case.segs)) * 101 + mode * 7 +
            (13 if case.fam == "round" else 0) + (3 if case.dtype == "f16" else 0))


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1).float()


def _x(M, K, g, carrier, few, lift=8.0):
    P = K // 8
    x = torch.zeros(M, P, 8)
    x.scatter_(2, torch.randint(0, 8, (M, P, 1), generator=g), _signs((M, P, 1), g))
    if carrier == "round":
        x[:, 0] = 0.0
        x[:, 0, 0], x[:, 0, 1] = lift, 1.0
    elif carrier:
        x[:, 0] = 0.0
        x[:, 0, 0] = 8.0
    elif P % 2 == 0 and (P <= 48 or few):
        x[:, 0] *= 2.0
    return x.view(M, K)


def _lift(w, first=0):
    """The rounding-point carrier of a weight matrix: column 0 = +-c with c walking through [56, 104] (8 c = 448 .. 832, one in
    six below 512), column 1 = 0 / 1 by row so that both parities of y occur."""
    n = first + torch.arange(w.shape[0])      # (rows are numbered across the segments: no two segments start alike)
    w[:, 0] = (56 + (17 * n + 5) % 49).float() * (1 - 2 * ((n // 2) % 2)).float()
    w[:, 1] = (n % 2).float()


@functools.lru_cache(maxsize=6)
def _inputs(key):
    M, K, segs, epi, fam, dtype, qkv = key
    case = Case("k", M, K, segs, epi, "", fam=fam, dtype=dtype, qkv=qkv)
    g = torch.Generator().manual_seed(_seed(case))
    R = case.R
    x = _x(M, K, g, "round" if fam == "round" else epi == SWIGLU, M * sum(segs) < 4096, 64.0 if dtype == "f16" else 8.0)
    rows = [case.N, case.N] if epi == SWIGLU else list(segs)
    w = [_signs((n, K), g) for n in rows]
    if epi == SWIGLU:
        w[0][:, 0] = 16.0
        if fam == "round":
            _lift(w[1])
    elif fam == "round":
        for i, wi in enumerate(w):
            _lift(wi, sum(rows[:i]))
    inp = Inputs(x=x.to(R), w=[wi.to(R) for wi in w], res=None)
    if epi == RESIDUAL:
        y = exact_sums(inp)[0]
        r = 7 if fam == "round" else min(64, 256 - int(y.abs().max()))
        assert r >= 1, (key, r)
        inp.res = torch.randint(-r, r + 1, (M, case.N), generator=g).to(R)
    if epi == QKV:
        H, Hkv, layout, seq = qkv
        pos = torch.tensor(POSITIONS[:M], dtype=torch.int32)
        idx = (7 * torch.arange(ROPE_LEN)[:, None] + 3 * torch.arange(HEAD // 2)[None, :]) % len(CS)
        inp.rope_cs = torch.tensor(CS, dtype=torch.float32)[idx].contiguous()
        inp.tok_pos = pos
        inp.tok_seq = (M - torch.arange(M)).to(torch.int32) if seq else None
        inp.B = M + 2
    return inp


def inputs(case):
    if case.epi != QKV:
        return _inputs(case.key)
    base = _inputs(case.key[:-1] + (case.qkv[:2] + ("slot", True),))                  # (the ring layout and tok_seq do not change x, W, rope_cs)
    inp = Inputs(**base.__dict__)
    if not case.qkv[3]:
        inp.tok_seq = None
    return inp


def exact_sums(inp):
    """fp64 [M, rows] per weight segment (row chunks, so that the fp64 image of a large matrix is never whole)."""
    x = inp.x.double()
    return [torch.cat([x @ w[i:i + 1024].double().T for i in range(0, w.shape[0], 1024)], dim=1) for w in inp.w]


def guard(M, N, dtype):
    """(buffer [M + 4, N + 8] of SENT, the view [M, N] two rows down: ldo = N + 8)."""
    buf = torch.full((M + 4, N + 8), SENT, dtype=dtype)
    return buf, buf[2:2 + M, :N]


def ring_shape(case):
    H, Hkv, layout, seq = case.qkv
    return (case.M + 2, Hkv, RING_W, HEAD) if layout == "head" else (case.M + 2, RING_W, Hkv, HEAD)


def new_ring(case, W=RING_W):
    """A K or V ring in the reference's shape [B, W, Hkv, 128] (head-major: a permuted view of [B, Hkv, W, 128]) full of SENT."""
    H, Hkv, layout, seq = case.qkv
    if layout == "head":
        return torch.full((case.M + 2, Hkv, W, HEAD), SENT, dtype=BF).permute(0, 2, 1, 3)
    return torch.full((case.M + 2, W, Hkv, HEAD), SENT, dtype=BF)


# ------------------------------------------------------------------------------------------------------------ fp64 reference
def _rope64(y, cs_rows):
    """y [n pairs.., 2] fp64 (bf16 values), cs_rows [.., 2]: rope.py:13-23 as complex multiplication."""
    c, s = cs_rows[..., 0], cs_rows[..., 1]
    return torch.stack((y[..., 0] * c - y[..., 1] * s, y[..., 0] * s + y[..., 1] * c), dim=-1)


@functools.lru_cache(maxsize=4)
def _reference(key):
    M, K, segs, epi, fam, dtype, qkv = key
    case = Case("k", M, K, segs, epi, "", fam=fam, dtype=dtype, qkv=qkv)
    inp, R = _inputs(key), case.R
    rd = lambda v: v.to(R).double()
    sums = exact_sums(inp)
    if epi == SWIGLU:
        a, b = rd(sums[0]), rd(sums[1])
        s = rd(a / (1.0 + torch.exp(-a)))
        assert torch.equal(s, a), key
        return [(s * b).to(R)]
    y = rd(torch.cat(sums, dim=1))
    if epi == STORE:
        return [y.to(R)]
    if epi == LOGITS:
        return [y.float()]
    if epi == RESIDUAL:
        return [(inp.res.double() + y).to(R)]
    H, Hkv, layout, seq = qkv
    n1 = (H + Hkv) * HEAD
    cs = inp.rope_cs.double()[inp.tok_pos.long()]                                     # [T, 64, 2]
    rot = _rope64(y[:, :n1].reshape(M, -1, HEAD // 2, 2), cs[:, None])
    out = torch.cat((rot.reshape(M, n1), y[:, n1:]), dim=1).to(BF)
    res = [out]
    if layout is not None:
        rk, rv = new_ring(case), new_ring(case)
        for t in range(M):
            b = int(inp.tok_seq[t]) if seq else t
            slot = int(inp.tok_pos[t]) % RING_W
            rk[b, slot] = out[t, H * HEAD:n1].view(Hkv, HEAD)
            rv[b, slot] = out[t, n1:].view(Hkv, HEAD)
        res += [rk, rv]
    return res


def reference(case):
    """[out [M, N]] in the output dtype; q|k|v with a cache: [qkv, ring k, ring v] (the rings in the reference's shape)."""
    return _reference(case.key)


def expected(case):
    """The reference inside its guard buffer (+ the rings)."""
    ref = reference(case)
    buf, view = guard(case.M, ref[0].shape[1], case.odt)
    view.copy_(ref[0])
    return [buf] + list(ref[1:])


def _inexact(v, R):
    return v.to(R).double() != v


def _ties(v, base=256):
    """exact ties among integers base <= |v| < 4 base, where the format holds every 2nd integer below 2 base and every 4th from
    there (bf16: base 256, fp16: 2048): odd below 2 base, 2 mod 4 above."""
    a = v.abs()
    return ((a < 2 * base) & (a % 2 == 1)) | ((a >= 2 * base) & (a % 4 == 2))


def _pairs(n, limit=64):
    """index pairs (i < j) of n rows: all of them up to `limit` rows, 512 drawn ones above"""
    if n <= limit:
        i, j = torch.triu_indices(n, n, offset=1)
        return i, j
    g = torch.Generator().manual_seed(n)
    i = torch.randint(0, n, (512,), generator=g)
    j = (i + 1 + torch.randint(0, n - 1, (512,), generator=g)) % n
    return i, j


def _shift_shares(y, dim):
    """[(shift, share of all entries that differ from the entry `shift` rows / columns on, the smallest share over single pairs)]"""
    out = []
    for s in (1, 2, 64, 128, 256):
        if y.shape[dim] > s:
            d = y.narrow(dim, s, y.shape[dim] - s) != y.narrow(dim, 0, y.shape[dim] - s)
            out.append((s, float(d.double().mean()), float(d.double().mean(dim=1 - dim).min())))
    return out


def conditions(case):
    """Asserts the generator's conditions (module docstring) and returns the measured figures."""
    inp, R = inputs(case), case.R
    sums = exact_sums(inp)
    bound = max(float((inp.x.double().abs() @ w.double().abs().T).max()) for w in inp.w)
    assert bound < 2 ** 24, (case, bound)
    fig = dict(bound=bound)
    if case.epi == SWIGLU:
        a, b = sums
        fig["a"] = (float(a.min()), float(a.max()))
        assert 24 <= a.min() and a.max() <= 256, (case, fig)
        y = b
        if case.fam == "plain":
            assert b.abs().max() <= 256, case
            fig["zeros"] = float((b == 0).double().mean())                          # (b == 0: the output is 0 whatever a)
            assert fig["zeros"] < 0.15, (case, fig)
    else:
        y = torch.cat(sums, dim=1)
    fig["maxy"], fig["miny"] = float(y.abs().max()), float(y.abs().min())
    if case.fam == "plain":
        if case.epi != SWIGLU:
            assert fig["maxy"] <= 256, (case, fig)
            fig["zeros"] = float((y == 0).double().mean())
            assert fig["zeros"] < 0.15, (case, fig)
            for dim, other in ((0, 1), (1, 0)):
                for s, share, worst in _shift_shares(y, dim):
                    if case.K >= 16 and (y.shape[dim] - s) * y.shape[other] >= 64:
                        assert share >= 0.25, (case, "shift", s, "dim", dim, share)
                    if y.shape[other] >= 32 and case.K >= 64:
                        assert worst >= 0.25, (case, "pair at shift", s, "dim", dim, worst)
                if y.shape[other] >= 32 and case.K >= 64 and y.shape[dim] >= 2:      # any two rows (columns): all pairs, or 512 drawn ones
                    yt = y if dim == 0 else y.T
                    i, j = _pairs(yt.shape[0])
                    worst = float((yt[i] != yt[j]).double().mean(dim=1).min())
                    fig["pairs"] = min(fig.get("pairs", 1.0), worst)
                    assert worst >= 0.25, (case, "some pair, dim", dim, worst)
        if case.epi == RESIDUAL:
            assert float((inp.res.double() + y).abs().max()) <= 256, case
        assert not bool(_inexact(y, R).any())
    else:
        base = 2048 if case.dtype == "f16" else 256
        assert base < fig["miny"] and fig["maxy"] < 4 * base, (case, fig)
        fig["inexact"], fig["ties"] = float(_inexact(y, R).double().mean()), float(_ties(y, base).double().mean())
        assert fig["inexact"] >= 0.25 and fig["ties"] >= 0.05, (case, fig)
        if case.epi == RESIDUAL:
            r = inp.res.double()
            fig["double"] = float(((r + y.to(R).double()).to(R) != (r + y).to(R)).double().mean())
            assert fig["double"] >= 0.05, (case, fig)
    if case.epi == QKV:
        pos = inp.tok_pos.tolist()
        assert len({p % len(CS) for p in pos}) == len(pos) and (case.qkv[2] is None or max(pos) >= RING_W or case.M == 1)
        if inp.tok_seq is not None:
            seq = inp.tok_seq.tolist()
            assert len(set(seq)) == len(seq) and seq != list(range(case.M)) and max(seq) < inp.B
    return fig


# --------------------------------------------------------------------------------------------------------------- mutants
OPERAND_MUTANTS = ["piece_dropped_first", "piece_dropped_middle", "piece_dropped_last", "piece_from_neighbour", "x_piece_from_neighbour"]
ROW_MUTANTS = ["seg_wrong_n0", "seg_wrong_n1", "w1_w3_exchanged"]
ROUND_MUTANTS = ["residual_before_rounding", "logits_not_rounded", "ab_not_rounded", "hid_truncated", "round_half_away"]
GEMV_MUTANTS = OPERAND_MUTANTS[:4] + ["tail_counted_again"] + OPERAND_MUTANTS[4:] + ["odd_row_from_partner", "partner_dropped"] + ROW_MUTANTS + \
    ["pass_operands"] + ROUND_MUTANTS
QKV_MUTANTS = OPERAND_MUTANTS + ["seg_wrong_n0", "seg_wrong_n1", "pass_operands", "round_half_away", "cs_neighbour_pair", "pos_other_token",
                                 "k_slot_pos", "k_seq_t", "v_rotated"]
TILE_MUTANTS = ["ragged_row_dropped", "ragged_col_dropped", "row_past_written", "col_past_written", "kslice_first", "kslice_middle",
                "kslice_last", "next_ntile_rows", "tail_c0_off"]
GEMM_MUTANTS = OPERAND_MUTANTS + ROW_MUTANTS + ROUND_MUTANTS + TILE_MUTANTS
SUBSTITUTIONS = ("odd_row_from_partner", "seg_wrong_n0", "seg_wrong_n1")          # one place only: may be provably invisible


def mutants_of(case):
    return QKV_MUTANTS if case.epi == QKV else GEMV_MUTANTS if case.M <= GEMV_MAX_T else GEMM_MUTANTS


def _quantum(v, R):
    """fp64: the spacing of format R (bf16: 8 significand bits, fp16: 11) at each |v| (normal range)"""
    e = torch.frexp(v.double().abs().clamp(min=2.0 ** -14))[1]
    return torch.pow(2.0, (e - (8 if R == BF else 11)).double())


def _rha(v, R=BF):
    """fp32 -> R with ties away from zero (as fp32)."""
    q = _quantum(v, R)
    return (torch.sign(v.double()) * torch.floor(v.double().abs() / q + 0.5) * q).float()


def _trunc(v, R=BF):
    q = _quantum(v, R)
    return (torch.sign(v.double()) * torch.floor(v.double().abs() / q) * q).float()


def _rounding_applies(case, mutant):
    need = {"residual_before_rounding": RESIDUAL, "logits_not_rounded": LOGITS, "ab_not_rounded": SWIGLU, "hid_truncated": SWIGLU}
    if case.fam != "round":
        return False
    return mutant == "round_half_away" or case.epi == need[mutant]


def _epilogue(case, acc, acc3, res, mutant):
    """fp32 accumulators -> the output dtype, rounding where the kernels round (common.cuh, gemv_core.cuh finish_unit, gemm.hip)."""
    R = case.R
    rd = (lambda v: _rha(v, R)) if mutant == "round_half_away" else (lambda v: v.to(R).float())
    if case.epi == SWIGLU:
        a, b = (acc, acc3) if mutant == "ab_not_rounded" else (rd(acc), rd(acc3))
        s = rd((a.double() / (1.0 + torch.exp(-a.double()))).float())
        h = s * b
        return (_trunc(h, R) if mutant == "hid_truncated" else rd(h)).to(R)
    if case.epi == LOGITS:
        return acc if mutant == "logits_not_rounded" else rd(acc)
    y = acc if mutant == "residual_before_rounding" else rd(acc)
    if case.epi == RESIDUAL:
        return rd(res.float() + y).to(R)
    return y.to(R)


def _pieces(t):
    return t.float().view(t.shape[0], -1, 8)


def _operands(case, mutant):
    """(x, w list, row map) with an operand mutant applied to ONE row / token, or None where it has nothing to break.  The
    mutated weight row is the middle output row; the pieces: first, middle, last, and for the substitutions the first piece from
    the middle whose substitute multiplies differently (module docstring)."""
    inp = inputs(case)
    x, w = inp.x, list(inp.w)
    P = case.K // 8
    if mutant not in OPERAND_MUTANTS + ["tail_counted_again"]:
        return x, w
    if case.fam != "plain":         # (a sum moved by 1 can round to the same bf16 value above 256: the plain family is the one for pieces)
        return None
    n = (case.N if case.epi == SWIGLU else sum(case.segs)) // 2
    if case.epi == SWIGLU:          # W1's row n is multiplied by b[:, n]: the first row from the middle with a nonzero b
        b = x.float() @ w[1].float().T
        n = next(((n + i) % case.N for i in range(case.N) if bool((b[:, (n + i) % case.N] != 0).any())), None)
        if n is None:
            return None
    si = 0
    while case.epi != SWIGLU and n >= w[si].shape[0]:
        n -= w[si].shape[0]
        si += 1
    order = [(P // 2 + i) % P for i in range(P)]
    if mutant == "x_piece_from_neighbour":
        if case.M < 2:
            return None
        t = case.M // 2
        t2 = t + 1 if t + 1 < case.M else t - 1
        xp = _pieces(x)
        for p in order:
            d = xp[t2, p] - xp[t, p]
            if any(bool((_pieces(wi)[:, p] @ d != 0).any()) for wi in w):
                x = x.clone()
                x[t, 8 * p:8 * p + 8] = inp.x[t2, 8 * p:8 * p + 8]
                return x, w
        return None
    row = w[si][n].clone()
    rp = _pieces(w[si][n:n + 1])[0]
    if mutant.startswith("piece_dropped"):
        p = {"first": 0, "middle": P // 2, "last": P - 1}[mutant.split("_")[-1]]
        row[8 * p:8 * p + 8] = 0
    elif mutant == "tail_counted_again":
        if case.K % 512 == 0:
            return None
        row[-8:] = row[-8:] * 2
    else:
        if P < 2:
            return None
        xp = _pieces(x)
        for p in order:
            p2 = p + 1 if p + 1 < P else p - 1
            if bool((xp[:, p] @ (rp[p2] - rp[p]) != 0).any()):
                row[8 * p:8 * p + 8] = w[si][n, 8 * p2:8 * p2 + 8]
                break
        else:
            return None
    w[si] = w[si].clone()
    w[si][n] = row
    return x, w


def _row_sources(case, w, mutant):
    """[(segment, local row)] per output row of a non-SwiGLU call: the segment lookup of seg_row, with its mutants (a lookup in the
    wrong segment wraps inside that segment), or None."""
    ends, src = [], []
    for i, wi in enumerate(w):
        src += [(i, r) for r in range(wi.shape[0])]
        ends.append(len(src))
    if mutant in ("seg_wrong_n0", "seg_wrong_n1"):
        b = 0 if mutant == "seg_wrong_n0" else 1
        if len(w) < b + 2:
            return None
        src[ends[b]] = (b, 0)       # row n_b looked up in segment b, one past its end: wraps to its row 0
    return src


def _gather(w, src):
    out = torch.empty(len(src), w[0].shape[1], dtype=torch.float32)
    for i, wi in enumerate(w):
        idx = [j for j, (s, _) in enumerate(src) if s == i]
        if idx:
            out[idx] = wi.float()[[src[j][1] for j in idx]]
    return out


# --------------------------------------------------------------------------------------------------------- GEMV emulation
def _slot_maps(K):
    """load_batch / fma_batch: a unit walks nb batches of 4 chunks of 64 pieces; piece slot p loads piece min(p, P - 1) and
    multiplies it only when p < P."""
    P = K // 8
    nch = (K + 511) // 512
    nb = (nch + 3) // 4
    slots = torch.arange(nb * 4 * 64)
    return torch.clamp(slots, max=P - 1), slots < P


def _unit_dot(wrows, xs, K):
    """fp32 [rows, T]: every row's pieces through the slot maps."""
    piece, live = _slot_maps(K)
    cols = (piece[live][:, None] * 8 + torch.arange(8)[None, :]).reshape(-1)
    xcols = (torch.nonzero(live)[:, 0][:, None] * 8 + torch.arange(8)[None, :]).reshape(-1)
    return wrows[:, cols] @ xs.float()[:, xcols].T


def gemv_emulation(case, mutant=None):
    """launch path of M <= 8 in torch: [guard buffer] (+ rings), or None where the mutant has nothing to break."""
    inp = inputs(case)
    if mutant in ROUND_MUTANTS and not _rounding_applies(case, mutant):
        return None
    ops = _operands(case, mutant)
    if ops is None:
        return None
    x, w = ops
    M, K, N, epi = case.M, case.K, case.N, case.epi
    swiglu = epi == SWIGLU
    if mutant == "w1_w3_exchanged":
        if not swiglu:
            return None
        w = [w[1], w[0]]
    if swiglu:
        if mutant in ("seg_wrong_n0", "seg_wrong_n1", "odd_row_from_partner", "partner_dropped"):
            return None
        W1, W3 = w[0].float(), w[1].float()
    else:
        src = _row_sources(case, w, mutant)
        if src is None:
            return None
        if mutant in ("odd_row_from_partner", "partner_dropped") and (N % 2 == 0 or N < 3):
            return None
        if mutant == "odd_row_from_partner":
            src[N - 1] = src[N - 2]
        Wc = _gather(w, src)
    ps = passes(M, K)
    if mutant == "pass_operands" and (len(ps) < 2 or epi not in (RESIDUAL, QKV)):
        return None
    buf, out = guard(M, N, case.odt)
    rings = None
    if epi == QKV:
        H, Hkv, layout, seq = case.qkv
        n0, n1 = H * HEAD, (H + Hkv) * HEAD
        if (mutant == "k_slot_pos" and (layout is None or max(inp.tok_pos.tolist()) < RING_W)) or \
                (mutant == "k_seq_t" and (layout is None or not seq)) or (mutant == "pos_other_token" and M < 2):
            return None
        if layout is not None:
            rings = [new_ring(case, ROPE_LEN), new_ring(case, ROPE_LEN)]             # (room for the slot mutant; the first W slots count)
    for t0, T in ps:
        xs = x[t0:t0 + T]
        e0 = 0 if mutant == "pass_operands" else t0                                 # first row of the pass's epilogue operands
        npairs = N if swiglu else (N + 1) // 2
        if swiglu:                  # unit q: (W1 row q, W3 row q)
            out[t0:t0 + T] = _epilogue(case, _unit_dot(W1, xs, K).T, _unit_dot(W3, xs, K).T, None, mutant)
            continue
        r0 = torch.arange(npairs) * 2
        r1 = torch.where(r0 + 1 < N, r0 + 1, r0)                                    # odd N: the partner aliases, its result is dropped
        acc0, acc1 = _unit_dot(Wc[r0], xs, K), _unit_dot(Wc[r1], xs, K)           # [npairs, T]
        two = r0 + 1 < N
        if mutant == "partner_dropped":
            two = two.clone()
            two[npairs // 2 - (1 if npairs // 2 == npairs - 1 else 0)] = False
        acc = torch.full((T, 2 * npairs), float("nan"))
        acc[:, 0::2], acc[:, 1::2] = acc0.T, acc1.T
        cols = torch.nonzero(torch.stack((torch.ones_like(two), two), dim=1).reshape(-1))[:, 0]   # the results that are stored
        if epi != QKV:
            res = inp.res[e0:e0 + T][:, cols] if epi == RESIDUAL else None
            out[t0:t0 + T, cols] = _epilogue(case, acc[:, cols], None, res, mutant)
            continue
        rd = _rha if mutant == "round_half_away" else (lambda v: v.to(BF).float())
        y = rd(acc[:, :N])
        for t in range(T):
            te = e0 + t
            pos = int(inp.tok_pos[te])
            if mutant == "pos_other_token" and t0 + t == M // 2:
                pos = int(inp.tok_pos[te + 1 if te + 1 < M else te - 1])
            cs = inp.rope_cs[pos]                                                    # [64, 2]
            cs_h = cs[None].expand((N // HEAD), HEAD // 2, 2).clone()
            if mutant == "cs_neighbour_pair" and t0 + t == M // 2:
                cs_h[1] = torch.roll(cs, -1, dims=0)                                 # head 1 of this token: pair i takes pair i + 1's entry
            pr = y[t].view(-1, HEAD // 2, 2)
            c, s = cs_h[..., 0], cs_h[..., 1]
            rot = torch.stack((pr[..., 0] * c - pr[..., 1] * s, pr[..., 0] * s + pr[..., 1] * c), dim=-1).reshape(-1)
            lim = N if mutant == "v_rotated" else n1
            row = torch.cat((rd(rot[:lim]), y[t, lim:])).to(BF)
            out[t0 + t] = row
            if rings is not None:
                b = int(inp.tok_seq[te]) if (seq and mutant != "k_seq_t") else t0 + t
                slot = int(inp.tok_pos[te]) if mutant == "k_slot_pos" else int(inp.tok_pos[te]) % RING_W
                rings[0][b, slot] = row[n0:n1].view(Hkv, HEAD)
                rings[1][b, slot] = row[n1:].view(Hkv, HEAD)
    return [buf] + ([r[:, :RING_W] for r in rings] if rings is not None else [])


# --------------------------------------------------------------------------------------------------------- GEMM emulation
def launches(case, mutant=None):
    """[(c0, c1, BM, BN, BK)]: the launches of the route (gemm.hip launch_gemm; BN: output columns per tile)."""
    sw = case.epi == SWIGLU
    if case.path == "f16/generic":
        return [(0, case.N, 64, 64, 16)]
    if case.path.startswith("g128"):
        return [(0, case.N, 128, 64 if sw else 128, 64)]
    sp = tail_split(case.M, case.N, case.epi, case.cus, case.tail) if case.dtype == "bf16" else None
    bn = 128 if sw else 256
    if sp is None:
        return [(0, case.N, 256, bn, 64)]
    c0, kind = sp
    t0 = c0 + bn if mutant == "tail_c0_off" else c0
    return [(0, c0, 256, bn, 64), (t0, case.N, 128, 256, 64) if kind == "half" else (t0, case.N, 128, 128, 64)]


def column_slice(src, c0, c1):
    """gemm.hip column_slice on the row-source list: the rows of output columns [c0, c1)."""
    return src[c0:c1]


def _tile_acc(a, wt, BK, skip):
    """fp32 [m, n]: BK-wide K slices in reversed order; skip: the index of a slice left out."""
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], wt.shape[0], dtype=torch.float32)
    for s in reversed(range((K + BK - 1) // BK)):
        if s != skip:
            acc = acc + a[:, s * BK:(s + 1) * BK] @ wt[:, s * BK:(s + 1) * BK].T
    return acc


def gemm_emulation(case, mutant=None):
    """launch path of M > 8 in torch: [guard buffer], or None where the mutant has nothing to break."""
    inp = inputs(case)
    if mutant in ROUND_MUTANTS and not _rounding_applies(case, mutant):
        return None
    ops = _operands(case, mutant)
    if ops is None:
        return None
    x, w = ops
    M, K, N, epi = case.M, case.K, case.N, case.epi
    sw = epi == SWIGLU
    if mutant == "w1_w3_exchanged":
        if not sw:
            return None
        w = [w[1], w[0]]
    if sw:
        if mutant in ("seg_wrong_n0", "seg_wrong_n1"):
            return None
        src = [(0, r) for r in range(N)]
    else:
        src = _row_sources(case, w, mutant)
        if src is None:
            return None
    ls = launches(case, mutant)
    if mutant == "tail_c0_off" and (len(ls) < 2 or ls[1][0] >= N):
        return None
    xf = x.float()
    buf, out = guard(M, N, case.odt)
    big = buf[2:, :]                                                                # rows from the view's first, all columns: room to overrun
    tiles = [(li, mt, nt) for li, (c0, c1, BM, BN, BK) in enumerate(ls) for mt in range((M + BM - 1) // BM) for nt in range((c1 - c0 + BN - 1) // BN)]
    hit = tiles[len(tiles) // 2]
    nk = lambda BK: (K + BK - 1) // BK
    if mutant in ("ragged_row_dropped", "row_past_written"):
        c = [t for t in tiles if M % ls[t[0]][2] and t[1] == (M - 1) // ls[t[0]][2]]
        if not c:
            return None
        hit = c[len(c) // 2]
    if mutant in ("ragged_col_dropped", "col_past_written"):
        c = [t for t in tiles if (ls[t[0]][1] - ls[t[0]][0]) % ls[t[0]][3] and t[2] == (ls[t[0]][1] - ls[t[0]][0] - 1) // ls[t[0]][3] and ls[t[0]][1] == N]
        if not c:
            return None
        hit = c[len(c) // 2]
    if mutant == "next_ntile_rows":
        c = [t for t in tiles if (t[0], t[1], t[2] + 1) in tiles]
        if not c:
            return None
        hit = c[len(c) // 2]
    for li, (c0, c1, BM, BN, BK) in enumerate(ls):
        ssrc = column_slice(src, c0, c1)
        Ns = c1 - c0
        Wl = _gather(w[:1] if sw else w, ssrc)
        W3 = _gather(w[1:], ssrc) if sw else None
        for mt in range((M + BM - 1) // BM):
            m0 = mt * BM
            rv = min(BM, M - m0)
            rows = m0 + torch.clamp(torch.arange(BM), max=rv - 1)                   # tile rows past the last valid one repeat it
            a = xf[rows]
            for nt in range((Ns + BN - 1) // BN):
                me = (li, mt, nt) == hit
                wn = nt + 1 if (me and mutant == "next_ntile_rows") else nt
                cols = torch.clamp(wn * BN + torch.arange(BN), max=Ns - 1)          # ... and so do the weight rows
                skip = None
                if me and (mutant or "").startswith("kslice"):
                    skip = {"first": 0, "middle": nk(BK) // 2, "last": nk(BK) - 1}[mutant.split("_")[-1]]
                acc = _tile_acc(a, Wl[cols], BK, skip)
                acc3 = _tile_acc(a, W3[cols], BK, skip) if sw else None
                cv = min(BN, Ns - nt * BN)
                rvs, cvs = rv, cv
                if me:
                    rvs += {"ragged_row_dropped": -1, "row_past_written": 1}.get(mutant, 0)
                    cvs += {"ragged_col_dropped": -1, "col_past_written": 1}.get(mutant, 0)
                oc = c0 + nt * BN
                res = None
                if epi == RESIDUAL:
                    res = torch.zeros(rvs, cvs)
                    res[:min(rvs, rv), :min(cvs, cv)] = inp.res[m0:m0 + min(rvs, rv), oc:oc + min(cvs, cv)].float()
                big[m0:m0 + rvs, oc:oc + cvs] = _epilogue(case, acc[:rvs, :cvs], acc3[:rvs, :cvs] if sw else None, res, mutant)
    return [buf]


def emulate(case, mutant=None):
    return gemv_emulation(case, mutant) if case.M <= GEMV_MAX_T else gemm_emulation(case, mutant)


def differing(got, want):
    """the number of differing elements over the guard buffer and the rings"""
    return sum(int((g.float() != w.float()).sum()) for g, w in zip(got, want))


def describe(case, got, want, limit=8):
    """For a mismatch report: the first differing (row, column) of the view (negative / past the end: a guard element) per tensor."""
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        bad = torch.nonzero(g.float() != w.float())
        if bad.numel():
            where = [tuple(int(v) - (2 if (i == 0 and j == 0) else 0) for j, v in enumerate(b)) for b in bad[:limit]]
            out.append((("out", "ring k", "ring v")[i], int(bad.shape[0]), where, [float(g[tuple(b)]) for b in bad[:limit]], [float(w[tuple(b)]) for b in bad[:limit]]))
    return out
