"""The exact family of the MXFP4 tests: inputs whose products are all multiples of 2^-4 and whose sum of magnitudes stays below
2^24 such units, so that the fp32 result is the same in ANY summation order and a kernel is compared with `torch.equal` against an
fp64 chain.  Shared by tests/test_mxfp4_host.py (the reference's teeth) and tests/test_gpu_mxfp4.py."""
import torch

# (K, N): K = 32 is the smallest the kernels take; 2080 = one full chunk of 64 pieces + a one-block tail, N = 33 an odd row;
# N = 8 fewer units than waves; 14336 the largest contraction of the 7B shapes
EXACT_SHAPES = [(32, 8), (2080, 33), (4096, 512), (14336, 64)]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
UNIT = 2.0 ** -4  # 0.5 (smallest nonzero e2m1) * 2^-3 (smallest scale) * 1 (smallest nonzero |x|)


def exact_case(K, N, M, seed=0):
    """codes: uniform random bytes [N, K / 2]; scale bytes 127 + U{-3..3} per (row, block); x: integers in [-2, 2] as bf16 [M, K]"""
    g = torch.Generator().manual_seed(seed * 1000003 + K * 31 + N)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scale = (127 + torch.randint(-3, 4, (N, K // 32), generator=g)).to(torch.uint8)
    x = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16)
    return packed, scale, x


def dequant_f64(packed, scale):
    """fp64 [N, K] of 2^(b - 127) * e2m1(code), the low nibble at the even k - written out here, independent of quant.py"""
    tab = torch.tensor(E2M1 + [-v for v in E2M1], dtype=torch.float64)
    N, half = packed.shape
    codes = torch.stack((packed & 15, packed >> 4), dim=2).reshape(N, half * 2)
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), scale.to(torch.float64) - 127.0)
    return (tab[codes.long()].reshape(N, half * 2 // 32, 32) * sc[:, :, None]).reshape(N, half * 2)


def exact_reference(packed, scale, x):
    """y [M, N] in fp64: exact"""
    return x.double() @ dequant_f64(packed, scale).t()


def exact_sum_of_magnitudes_units(packed, scale, x):
    """max over outputs of sum_k |w x| in units of 2^-4: below 2^24 the fp32 sum is exact in any order"""
    return float((x.double().abs() @ dequant_f64(packed, scale).abs().t()).max() / UNIT)
