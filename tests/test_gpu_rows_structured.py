"""The row kernels of csrc/elementwise.hip on the structured cases of row_cases.py, through the `_hip` leaf wrappers only (no model,
no graph, no engine): greedy_rows_kernel (both loops, every slot of a trip, chosen ties, padded and unaligned rows, -inf logits),
rmsnorm_kernel<NP> at its dispatch edges (exact sums: bit-equal), rope_kernel (every head size, a strided buffer, a table that names
the entry each pair read), moe_router_kernel (exact logits, chosen ties, the fused-norm form), kv_write_kernel on bf16 rings (both
layouts, wrapped rings, an empty sequence, views of a fused buffer) and the two log-probability routes of mi_lm_head_logprobs.

test_row_cases_host.py proves on the CPU what these comparisons catch; the comparison itself (`*_mismatch`) lives in row_cases.py so
that both files apply the same one."""
import pytest
import torch

import row_cases as rc
from test_gpu_kv_layout import dev_ring

pytestmark = pytest.mark.gpu


def _hip():
    from mistral_inference import _hip
    return _hip


def report(bad):
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------------------------------ greedy
@pytest.mark.parametrize("case", rc.greedy_cases(), ids=lambda c: f"v{c.V}-{c.layout}")
def test_greedy_rows(case):
    """One launch, one row per placement: the token is torch.argmax exactly, the log-probability fp64 log_softmax at it within 2e-5,
    finite on the rows that hold -inf."""
    h = _hip()
    labels, buf = rc.greedy_inputs(case)
    dev = buf.cuda()
    tok, lp = h.greedy_sample(dev[:, :case.V])
    want = rc.greedy_expected(case)
    err = (lp.cpu().double() - want[1]).abs()
    print(f"{case}: {len(labels)} rows, worst |logprob error| {float(err[torch.isfinite(err)].max()) if bool(torch.isfinite(err).any()) else float('nan'):.3g}, "
          f"non-finite {int((~torch.isfinite(lp.cpu())).sum())}")
    assert torch.equal(dev.cpu(), buf)
    bad = rc.greedy_mismatch(case, (tok, lp), want)
    assert bad is None, bad


# ----------------------------------------------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("D", rc.RMS_DS)
def test_rmsnorm_exact_rows(D):
    """Bit-equal to the oracle on rows whose sum of squares is exact in any order; the rows after row T of the buffer stay poisoned."""
    h = _hip()
    bad = []
    for case in (c for c in rc.rms_cases() if c.D == D):
        _, _, x, w = rc.rms_inputs(case)
        big = torch.full((case.T + 3, D), rc.RMS_POISON, dtype=rc.BF).cuda()
        got = h.rmsnorm(x.cuda(), w.cuda(), rc.RMS_EPS, out=big[:case.T])
        d = rc.rms_mismatch(case, got, rc.rms_expected(case))
        if d:
            bad.append((case, d))
        if not bool((big[case.T:].cpu() == rc.RMS_POISON).all()):
            bad.append((case, "rows after T were written"))
    report(bad)


# -------------------------------------------------------------------------------------------------------------------------- rope
@pytest.mark.parametrize("Dh,H,Hkv", [(Dh, H, Hkv) for Dh in (64, 80, 128, 256) for H, Hkv in ((4, 2), (3, 1))])
def test_rope_addressing(Dh, H, Hkv):
    """The whole buffer - rotated q | k, untouched v, untouched padding - bit-equal to the oracle on the real table and to the
    read-off (position, pair index) on the selector table."""
    h = _hip()
    bad = []
    for case in (c for c in rc.rope_cases() if (c.Dh, c.H, c.Hkv) == (Dh, H, Hkv)):
        buf, cs, pos = rc.rope_inputs(case)
        dev = buf.cuda()
        h.rope_inplace(dev[:, :(H + 2 * Hkv) * Dh], H, Hkv, Dh, cs.cuda(), pos.cuda())
        d = rc.rope_mismatch(case, dev, rc.rope_expected(case))
        if d:
            bad.append((case, d))
    report(bad)


# ------------------------------------------------------------------------------------------------------------------------ router
@pytest.mark.parametrize("E,k", [(E, k) for E in (2, 8, 16) for k in (1, 2, 4) if k <= E])
def test_moe_router_exact_logits(E, k):
    """Exact indices (ties to the lowest expert id), weights exactly 1 / bf16(1 / k) on k-way ties and within one bf16 ulp of
    bf16(fp64 softmax) otherwise; the fused-norm form also bit-equal to the router run on rmsnorm's output."""
    h = _hip()
    bad = []
    for case in (c for c in rc.router_cases() if (c.E, c.k) == (E, k)):
        x, gate, w, _ = rc.router_inputs(case)
        xd, gd = x.cuda(), gate.cuda()
        if case.form == "norm":
            got = h.moe_router(xd, gd, k, norm_w=w.cuda(), eps=rc.RMS_EPS)
            two = h.moe_router(h.rmsnorm(xd, w.cuda(), rc.RMS_EPS), gd, k)
            if not (torch.equal(got[0], two[0]) and torch.equal(got[1], two[1])):
                bad.append((case, "fused norm differs from rmsnorm + router"))
        else:
            got = h.moe_router(xd, gd, k)
        d = rc.router_mismatch(case, got, rc.router_expected(case))
        if d:
            bad.append((case, d))
    report(bad)


# ---------------------------------------------------------------------------------------------------------------------- kv_write
@pytest.mark.parametrize("case", rc.kv_cases(), ids=lambda c: f"w{c.W}-{'head' if c.head_major else 'slot'}")
def test_kv_write_whole_ring(case):
    """Both rings, every slot, equal to the loop over cache.py's rule - the slots the rule leaves alone still hold the poison."""
    h = _hip()
    fused, tok_seq, tok_pos, q_start, _ = rc.kv_inputs(case)
    ck, cv = rc.kv_rings(case)
    dk, dv = dev_ring(ck, case.head_major), dev_ring(cv, case.head_major)
    assert h.kv_layout_of(dk) == (h.KV_HEAD_MAJOR if case.head_major and case.W > 1 else h.KV_SLOT_MAJOR)
    dev = fused.cuda()
    k, v = rc.kv_views(dev)
    h.kv_write(dk, dv, k, v, tok_seq.cuda(), tok_pos.cuda(), q_start.cuda())
    assert torch.equal(dev.cpu(), fused)
    bad = rc.kv_mismatch(case, (dk, dv), rc.kv_expected(case))
    assert bad is None, bad


# ---------------------------------------------------------------------------------------------------------------------- logprobs
@pytest.mark.parametrize("case", rc.logprob_cases(), ids=lambda c: f"v{c.V}-m{c.M}{c.variant}")
def test_lm_head_logprobs_exact_logits(case):
    """fp64 log_softmax of exact logits at the chosen targets (-1: minus the log-sum-exp), within the suite's 2e-4: three rows through
    logprob_rows_kernel, 256 through the GEMM's per-tile partials and logprob_finalize_kernel."""
    h = _hip()
    x, w, tgt = rc.logprob_inputs(case)
    got = h.lm_head_logprobs(x.cuda(), w.cuda(), tgt.cuda())
    want = rc.logprob_expected(case)
    print(f"{case}: worst error {float((got.cpu().double() - want).abs().max()):.3g}")
    bad = rc.logprob_mismatch(case, got, want)
    assert bad is None, bad
