"""Attention kernels against ONE fp64 reference on structured inputs whose expected output is sharp (attn_cases.py): census
counts every visible key, selector puts the whole weight on keys chosen by their row address, staircase drives the running
maximum up and down across tiles and splits so that the rescale branches run with live accumulators.  What each construction
can see, and the measured size of each mutant against the tolerance, is proved on the CPU in test_attn_cases_host.py.

Prefill: both block shapes (4 and 8 waves) and both ring layouts; decode: every kernel form ((H, Hkv, B) below), both layouts,
sequence lengths on the split and ring edges, and a second launch that must give the same bits."""
import functools

import pytest
import torch

import attn_cases as ac
from test_gpu_kv_layout import dev_ring

pytestmark = pytest.mark.gpu

DH = 128


def _hip():
    from mistral_inference import _hip
    return _hip


def _check(got, ref, S, what):
    ratio = (got.double() - ref).abs() / ac.tolerance(S)
    worst = int(ratio.argmax())
    row, col = divmod(worst, ratio.shape[1])
    assert float(ratio.max()) <= 1.0, (what, "err/tol", float(ratio.max()), "row", row, "head", col // DH, "dim", col % DH,
                                       "got", float(got[row, col]), "ref", float(ref[row, col]))


# ---------------------------------------------------------------------------------------------------------------- prefill
P_H, P_HKV = 4, 2


@functools.lru_cache(maxsize=None)
def _prefill_cons(ci):
    W, seen, new = ac.PREFILL_CASES[ci]
    return {c.name: c for c in ac.constructions(P_H, P_HKV, W, max(p + s for p, s in zip(seen, new)))}


@functools.lru_cache(maxsize=None)
def _prefill_ref(ci, name):
    """Inputs and the fp64 reference of one (case, construction): computed once, shared by block shapes and layouts."""
    W, seen, new = ac.PREFILL_CASES[ci]
    con = _prefill_cons(ci)[name]
    refs = [ac.ref_attention64(q, k, v, qpos, kpos, W, True) for q, k, v, qpos, kpos in ac.prefill_sequences(con, W, seen, new)]
    return ac.prefill_inputs(con, W, seen, new), torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])


def _prefill_params():
    for ci, (W, _, _) in enumerate(ac.PREFILL_CASES):
        names = ["census"] + [f"selector{d}" for d in ac.selector_deltas(W)] + ["staircase"]
        for name in names:
            yield pytest.param(ci, name, id=f"{ac.PREFILL_CASES[ci]}-{name}".replace(" ", ""))


@pytest.mark.parametrize("ci,name", list(_prefill_params()))
def test_attn_prefill_structured(ci, name):
    h = _hip()
    W, seen, new = ac.PREFILL_CASES[ci]
    (qkv, ck, cv, q_start, kv_before), ref, S = _prefill_ref(ci, name)
    dq, dqs, dkb = qkv.cuda(), q_start.cuda(), kv_before.cuda()
    try:
        for hm in (False, True):
            dk, dv = dev_ring(ck, hm), dev_ring(cv, hm)
            for waves in (4, 8):
                h.debug_set_prefill_kernels(attn_waves=waves)
                got = h.attn_prefill(dq, P_H, P_HKV, DH, dk, dv, W, dqs, dkb, len(new), max(new)).cpu()
                _check(got, ref, S, (name, "head-major" if hm else "slot-major", waves))
    finally:
        h.debug_set_prefill_kernels(attn_waves=0)


# ----------------------------------------------------------------------------------------------------------------- decode
DECODE_FORMS = [             # (H, Hkv, B) -> kernel form
    (4, 2, 1), (32, 8, 1),   # attn_decode_kernel<R, false>, UK = 4
    (12, 2, 1), (16, 2, 1),  # R = 6 and R = 8, UK = 2
    (8, 8, 1),               # R = 1
    (4, 2, 3), (32, 8, 3),   # W <= 4096: the all-in form; W = 5000 (160-slot splits): the SMALL form
]


@pytest.mark.parametrize("W", ac.DECODE_RINGS)
@pytest.mark.parametrize("H,Hkv,B", DECODE_FORMS)
def test_attn_decode_structured(H, Hkv, B, W):
    h = _hip()
    lens_all = ac.decode_lens(W)
    assert ac.split_chunk(W, ac.attn_decode_splits(W)) == {300: 112, 4096: 128, 5000: 160}[W]
    launches = [[lens_all[(i * B + b) % len(lens_all)] for b in range(B)] for i in range((len(lens_all) + B - 1) // B)]
    for con in ac.constructions(H, Hkv, W, 2 * W + 4, decode=True):
        for lens in launches:
            q, ck, cv, pos = ac.decode_inputs(con, W, lens)
            refs = [ac.ref_attention64(*ac.decode_sequence(con, W, n), W, True) for n in lens]
            ref, S = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
            dq, dpos = q.cuda(), pos.cuda()
            for hm in (False, True):
                dk, dv = dev_ring(ck, hm), dev_ring(cv, hm)
                got = h.attn_decode(dq, dk, dv, H, dpos).cpu()
                _check(got, ref, S, (con.name, lens, "head-major" if hm else "slot-major"))
                # the arrival counters are left at zero: a second launch gives the same bits
                assert torch.equal(got, h.attn_decode(dq, dk, dv, H, dpos).cpu()), (con.name, lens)
