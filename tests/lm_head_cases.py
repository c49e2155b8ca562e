"""A quantised LM head (`_hip.lm_head_q`: GEMV_LOGITS on e4m3 and MXFP4 rows, gemv_w8.hip / gemv_w4.hip) on inputs whose every
contraction is an EXACT integer sum, after linear_cases.py's rounding-point family: one fp64 reference with the head's one
rounding, a torch emulation of what the kernel computes, and single-fault mutants (helpers for test_lm_head_cases_host.py and
test_gpu_lm_head_quant.py; no test functions here).

Every weight matrix is made in real values first and goes through the project's quantiser, which must give it back bit for bit
(`Head.round_trip`, asserted by whoever builds a head): the test then knows every code and every scale.

  fp8          W in {-1, +1}; W[n, 0] = +-c, c walking the multiples of 8 in [56, 104] with n (e4m3 keeps three mantissa bits:
               another c would not survive); W[n, 1] = n % 2 (both parities of y).  x[:, 0] = 8, x[:, 1] = 1, elsewhere one +-1 per
               8-element piece.  quantize_rows gives row scales 0.125 (c = 56) and 0.25: neighbouring rows differ in scale.
               y = +-8 c + (n % 2) + a sum of K / 8 - 1 signs: 256 < |y| < 1024, where bf16 holds every 2nd or 4th integer.
  mxfp4        the same with W[n, 0] = +-4 / +-6 and x[:, 0] = 128: y = +-512 / +-768 + ...; quantize_blocks gives scale byte 127
               to block 0 and 125 to every other block (+-1 = 4 * 2^-2).
  fp8_hand     the fp8 codes under hand-made row scales 0.75 * 2^(n % 3), not powers of two, bound through load_quantized:
               y = acc * scale is exact in fp32 (|acc| < 2^13, two more bits for the factor 3) but seldom a bf16 value - "the
               scale applied after the rounding" and "the neighbouring row's scale" change the output here where they occur.
  mxfp4_shift  mxfp4 with row n multiplied by 2^(n % 3): the same codes, every scale byte of the row moved by n % 3, so that a
               scale row taken from the next row is visible on MXFP4 too (not asked for by the issue; 256 < |y| < 4096).

All sums are integers below 2^24 in magnitude (sum |w x| is asserted), so fp32 accumulation gives the same bits in any order and
the CPU reference may itself sum in fp32.  Reference: logits = float(bf16(y)), y the exact real-valued product.

Measured on the CPU at N = 520 / 521, K = 288, M = 5 (test_lm_head_cases_host.py prints them): fp8 row scales {0.125, 0.25},
431 <= |y| <= 849, 69 - 70 % of the sums not bf16 values, 29 - 31 % exact ties; mxfp4 scale bytes {125, 127}, 493 <= |y| <= 788,
70 - 71 % not bf16 values, 36 - 37 % ties; fp8_hand 1479 <= |y| <= 11184, 89 - 90 % not bf16 values, 10 % ties; mxfp4_shift scale
bytes {125 .. 129}, 493 <= |y| <= 3152, 70 - 71 % not bf16 values.  Single faults (differing logits of 5 x N): a dropped piece
724 .. 1020 in every case, the next row's scale 740 (fp8), 2595 (fp8_hand, mxfp4_shift) and 0 on plain mxfp4 (all rows share their
scale bytes: why mxfp4_shift exists), logits left in fp32 1796 .. 2340, the scale after the rounding 1646 / 1687 on fp8_hand and 0 on
fp8 (a power of two commutes with the rounding), the odd last row from its partner all 5.
"""
import functools

import torch

BF = torch.bfloat16
FP8, MXFP4, FP8_HAND, MXFP4_SHIFT = "fp8", "mxfp4", "fp8_hand", "mxfp4_shift"
KINDS = (FP8, MXFP4, FP8_HAND, MXFP4_SHIFT)
ISSUE_KINDS = (FP8, MXFP4)         # the two families the issue states, with its conditions; the other two carry weaker ones
PIECE = {FP8: 16, FP8_HAND: 16, MXFP4: 32, MXFP4_SHIFT: 32}     # weights per 16-byte piece
FAULTS = ("piece_dropped", "scale_next_row", "not_rounded", "scale_after_rounding", "odd_row_aliased")


def is_fp8(kind):
    return kind in (FP8, FP8_HAND)


def _quant():
    from mistral_inference import quant
    return quant


def real_weights(kind, N, K):
    """fp32 [N, K]: the real-valued matrix the quantiser is handed (fp8_hand: the fp8 one)."""
    g = torch.Generator().manual_seed(7919 * N + 31 * K + (0 if is_fp8(kind) else 1))
    w = (torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1).float()
    n = torch.arange(N)
    sign = (1 - 2 * ((n // 2) % 2)).float()
    c = (56 + 8 * ((5 * n + 3) % 7)).float() if is_fp8(kind) else (4 + 2 * ((n // 3) % 2)).float()
    w[:, 0] = c * sign
    w[:, 1] = (n % 2).float()
    if kind == MXFP4_SHIFT:
        w *= torch.ldexp(torch.ones(N), n % 3)[:, None]
    return w


def x_rows(kind, M, K):
    """bf16 [M, K]; the first rows of a larger M are the rows of a smaller one."""
    g = torch.Generator().manual_seed(104729 + K)
    P = K // 8
    x = torch.zeros(8, P, 8)
    x.scatter_(2, torch.randint(0, 8, (8, P, 1), generator=g), (torch.randint(0, 2, (8, P, 1), generator=g, dtype=torch.int8) * 2 - 1).float())
    x[:, 0] = 0.0
    x[:, 0, 0], x[:, 0, 1] = (8.0 if is_fp8(kind) else 128.0), 1.0
    assert M <= 8
    return x.view(8, K)[:M].contiguous().to(BF)


class Head:
    """weight: the checkpoint's bytes (uint8: e4m3 codes [N, K] / MXFP4 code pairs [N, K / 2]); scale: fp32 [N] / uint8 [N, K / 32];
    round_trip: the quantiser reproduced the real-valued matrix bit for bit (and, fp8_hand, the hand-made scales are as stated)."""

    def __init__(self, kind, N, K, device="cpu"):
        q = _quant()
        w = real_weights(kind, N, K).to(device)
        self.kind, self.N, self.K = kind, N, K
        if is_fp8(kind):
            codes, scale = q.quantize_rows(w.to(BF))
            self.round_trip = bool(torch.equal(q.dequantize(codes, scale).float(), w))
            if kind == FP8_HAND:
                scale = (0.75 * torch.ldexp(torch.ones(N), torch.arange(N) % 3)).to(device)
            self.weight, self.scale = codes.view(torch.uint8).contiguous(), scale.float().contiguous()
        else:
            self.weight, self.scale = q.quantize_blocks(w.to(BF))
            self.round_trip = bool(torch.equal(q.dequantize_mxfp4(self.weight, self.scale).float(), w))

    def dequantized(self):
        q = _quant()
        return q.dequantize(self.weight, self.scale) if is_fp8(self.kind) else q.dequantize_mxfp4(self.weight, self.scale)

    def parts(self, rows=slice(None)):
        """(codes fp32 [n, K] as values, scales fp64 [n] (FP8) or [n, K] per weight (MXFP4)) of some rows, on the CPU."""
        if is_fp8(self.kind):
            return self.weight[rows].cpu().view(torch.float8_e4m3fn).float(), self.scale[rows].cpu().double()
        wb, sb = self.weight[rows].cpu(), self.scale[rows].cpu()
        one = torch.full_like(sb, 127)
        return _quant().dequantize_mxfp4(wb, one).float(), torch.ldexp(torch.ones(sb.shape, dtype=torch.float64), sb.int() - 127).repeat_interleave(32, dim=1)


@functools.lru_cache(maxsize=8)
def head(kind, N, K):
    return Head(kind, N, K)


def _chunks(N, step=2048):
    return [slice(i, min(N, i + step)) for i in range(0, N, step)]


def exact_products(hd, x):
    """(y, sum |w x|) fp64 [M, N] for bf16 rows x: the real-valued products, exact.  Row chunks; integer sums in fp32 (exact below
    2^24, which the second result lets the caller assert) where the rows are integers, fp64 otherwise (normalised rows)."""
    xf = x.float().cpu()
    integral = bool((xf == xf.round()).all())
    ys, mags = [], []
    for rows in _chunks(hd.N):
        codes, sc = hd.parts(rows)
        if is_fp8(hd.kind):
            a, b = (xf, codes) if integral else (xf.double(), codes.double())
            ys.append((a @ b.T).double() * sc)
            mags.append((a.abs() @ b.abs().T).double() * sc)
        else:
            w = codes.double() * sc                                    # exact: a code times a power of two
            a, b = (xf, w.float()) if integral else (xf.double(), w)
            ys.append((a @ b.T).double())
            mags.append((a.abs() @ b.abs().T).double())
    return torch.cat(ys, dim=1), torch.cat(mags, dim=1)


def reference(hd, x):
    """fp32 [M, N]: float(bf16(y)) - one rounding, then widened, where the bf16 head rounds."""
    return exact_products(hd, x)[0].to(BF).float()


def ulp_bf16(v):
    _, ex = torch.frexp(v.abs().double())
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - 8))


def conditions(hd, x):
    """Asserts the generator's conditions (module docstring) and returns the measured figures."""
    y, mag = exact_products(hd, x)
    fig = dict(bound=float(mag.max()), miny=float(y.abs().min()), maxy=float(y.abs().max()))
    assert hd.round_trip, (hd.kind, "the quantiser does not reproduce the weights")
    assert fig["bound"] < 2 ** 24, fig
    r = y.to(BF).double()
    fig["inexact"] = float((r != y).double().mean())
    fig["ties"] = float(((r - y).abs() * 2 == ulp_bf16(y)).double().mean())
    fig["zeros"] = float((y == 0).double().mean())
    assert fig["inexact"] >= 0.25, (hd.kind, fig)                     # at least a quarter of the sums are not bf16 values
    assert fig["zeros"] < 0.15, (hd.kind, fig)                        # (linear_cases.conditions: the plain family's share)
    if hd.kind in ISSUE_KINDS:
        assert 256 < fig["miny"] and fig["maxy"] < 1024, (hd.kind, fig)
        assert fig["ties"] >= 0.05, (hd.kind, fig)                    # (linear_cases.conditions: the rounding family's share)
    if is_fp8(hd.kind):
        fig["scales"] = sorted(set(hd.scale.cpu().tolist()))
    else:
        fig["scales"] = sorted(set(hd.scale.cpu().reshape(-1).tolist()))
    return fig


def emulate(hd, x, fault=None):
    """fp32 [M, N] as the kernel computes it - acc = sum of code x activation (FP8; MXFP4: of block-scaled code x activation),
    FP8: y = acc * scale[r], logit = float(bf16(y)) - or with ONE fault; None where the fault has no form on this head."""
    codes, sc = hd.parts()
    codes = codes.double()
    N, K, P = hd.N, hd.K, PIECE[hd.kind]
    fp8 = is_fp8(hd.kind)
    if fault == "piece_dropped":                                      # the middle 16-byte piece of every row
        p = (K // P) // 2
        codes[:, p * P:(p + 1) * P] = 0.0
    if fault == "scale_next_row":                                     # row r reads the scale (the scale blocks) of row r + 1
        sc = torch.cat((sc[1:], sc[-1:]))
    if fault == "odd_row_aliased":                                    # the odd last row computed from its pair partner's pointers
        if N % 2 == 0 or N < 3:
            return None
        codes[N - 1] = codes[N - 2]
        sc = sc.clone()
        sc[N - 1] = sc[N - 2]
    xd = x.double().cpu()
    if fp8:
        acc = xd @ codes.T
        if fault == "scale_after_rounding":
            return (acc.to(BF).double() * sc).float()
        y = acc * sc
    else:
        if fault == "scale_after_rounding":
            return None                                               # (block scales sit inside the sum: no such place)
        y = xd @ (codes * sc).T
    return y.float() if fault == "not_rounded" else y.to(BF).float()
