"""The MoE expert leaves behind `_hip.moe_experts` - GEMV_MOE_W13 + moe_w2_kernel<1|2|4> at T <= 8, moe_lists_kernel + the
token-grouped GEMMs of gemm.hip / gemm256.hip + moe_combine_kernel above - with CHOSEN routing on inputs whose rounding chain is
exact (moe_cases.py), compared with torch.equal to one fp64-chain reference: empty experts, 1-row and ragged tiles, counts
of exactly tile_rows and one either side, up to five m-tiles per expert, n_tiles one short of max_m_tiles, the 128 / 256-row
switch, k = 1 and 4, picks written in descending and rotated order, K % 64 != 0, and the decode combine kernel's LDS limit.
That the emulated pipelines equal the reference and that every single-row fault changes some case is proved on the CPU in
test_moe_cases_host.py.  Every case runs twice: the scratch and n_tiles carry no state, so the two outputs are bit-equal.

A small Gaussian family covers SiLU's sensitive range under a tolerance three times what an honest emulation reaches."""
import pytest
import torch

import moe_cases as mc

pytestmark = pytest.mark.gpu


def _hip():
    from mistral_inference import _hip
    return _hip


_DEV = {}                    # expert set -> (device weights, [E, 3] pointer table): at most two sets stay on the device


def _dev_experts(case):
    key = (case.E, case.D, case.F, case.w2_density, case.gauss)
    if key not in _DEV:
        if len(_DEV) >= 2:
            _DEV.clear()
        dev = [tuple(w.cuda() for w in ex) for ex in mc.inputs(case).experts]
        tab = torch.tensor([[w1.data_ptr(), w2.data_ptr(), w3.data_ptr()] for w1, w2, w3 in dev], dtype=torch.int64, device="cuda")
        _DEV[key] = (dev, tab)
    return _DEV[key][1]


def _run_twice(case):
    h = _hip()
    inp = mc.inputs(case)
    tab = _dev_experts(case)
    x, res, idx, w = inp.x.cuda(), inp.h.cuda(), inp.sel_idx.cuda(), inp.sel_w.cuda()
    got = h.moe_experts(x, tab, case.E, case.F, idx, w, residual=res).cpu()
    again = h.moe_experts(x, tab, case.E, case.F, idx, w, residual=res).cpu()
    assert torch.equal(got, again), (case, "second run differs in rows", torch.nonzero((got != again).any(dim=1))[:, 0].tolist()[:12])
    return got


def _check_exact(case, got, ref):
    bad = torch.nonzero((got != ref).any(dim=1))[:, 0].tolist()
    assert not bad, (case, len(bad), "rows differ: (token, [(expert, tile, row in tile)])", mc.describe_rows(case, bad),
                     "first", bad[0], "got", got[bad[0]].float()[:8].tolist(), "ref", ref[bad[0]].float()[:8].tolist())


@pytest.mark.parametrize("case", mc.G128_CASES, ids=repr)
def test_moe_grouped_128_row_tiles(case):
    assert case.path == "g128"
    _check_exact(case, _run_twice(case), mc.reference(case)[0])


@pytest.mark.parametrize("case", [c for c in mc.G256_CASES if c is not mc.SWITCH_512], ids=repr)
def test_moe_grouped_256_row_tiles(case):
    assert case.path == "g256"
    _check_exact(case, _run_twice(case), mc.reference(case)[0])


def test_moe_grouped_tile_switch():
    """T k == 512 E is the first size on 256-row tiles: 511 tokens (128-row tiles) and 512 tokens (256-row tiles) of the same
    inputs give the same rows 0..510, equal to the reference."""
    lo, hi = mc.SWITCH_511, mc.SWITCH_512
    assert (lo.path, hi.path) == ("g128", "g256")
    got_lo, got_hi = _run_twice(lo), _run_twice(hi)
    _check_exact(lo, got_lo, mc.reference(lo)[0])
    _check_exact(hi, got_hi, mc.reference(hi)[0])
    assert torch.equal(got_lo, got_hi[:lo.T])


@pytest.mark.parametrize("case", mc.DECODE_CASES + mc.LDS_EDGE_CASES, ids=repr)
def test_moe_decode_leaf(case):
    assert case.path == "decode"
    _check_exact(case, _run_twice(case), mc.reference(case)[0])


def test_moe_decode_past_the_lds_limit_is_a_shape_error():
    """top_k F 2 = 65568 bytes does not fit the combine kernel's LDS: the library's shape error, not a launch."""
    h = _hip()
    E, k, T, D, F = 4, 2, 8, 256, 16392
    assert k * F * 2 > 65536 >= k * (F - 8) * 2
    dev = [tuple(torch.zeros(s, dtype=torch.bfloat16, device="cuda") for s in ((F, D), (D, F), (F, D))) for _ in range(E)]
    tab = torch.tensor([[w.data_ptr() for w in ex] for ex in dev], dtype=torch.int64, device="cuda")
    x = torch.zeros(T, D, dtype=torch.bfloat16, device="cuda")
    idx = mc.route_decode(T, k, E).cuda()
    with pytest.raises(RuntimeError, match="too large for the decode combine kernel") as err:
        h.moe_experts(x, tab, E, F, idx, mc.slot_weights(T, k).cuda(), residual=x)
    assert f"(code {h.MI_ERR_SHAPE})" in str(err.value)


@pytest.mark.parametrize("case", mc.GAUSS_CASES, ids=repr)
def test_moe_gaussian_family(case):
    got = _run_twice(case)
    ref, S = mc.reference(case)
    ratio = (got.double() - ref.double()).abs() / mc.tolerance(S)
    worst = int(ratio.argmax())
    row, col = divmod(worst, ratio.shape[1])
    print(case, "max err / (2^-7 S)", mc.gauss_ratio(got, ref, S), "bound", mc.GAUSS_C)
    assert float(ratio.max()) <= 1.0, (case, "err/tol", float(ratio.max()), "token", row, "col", col, "got", float(got[row, col]),
                                       "ref", float(ref[row, col]), mc.describe_rows(case, [row]))
