"""mi_attn_verify against the fp64 reference of attn_cases.py on its structured inputs (census, selector, staircase), unchanged:
m consecutive rows of a sequence whose rows are NOT in the ring.  Every element within attn_cases.tolerance(S), the project's
attention tolerance.  The selector offsets (1 - W) % 128 and -W % 128 probe "oldest visible key present" and "kp = qp - W absent"
for every row of the step on its own: on a wrapped ring these are the slots of the step's own positions, which earlier rows
must read and later rows must not (what test_attn_verify_host.py shows a kernel that wrote the rows first gets wrong).

Shapes: GQA ratios 1, 4 and 6 (passes of four (head, row) pairs: whole, and a ragged last pass); rings of 16 (one block, m = 8
is half the ring), 300 (three blocks, the last one ragged) and 4096 slots (32 blocks); 1, 2, 5 and 8 rows; cached lengths from the
empty ring over the split edges to a ring wrapped twice; both ring layouts; one launch of two sequences with 3 and 5 rows."""
import functools

import pytest
import torch

import attn_cases as ac
import attn_verify_cases as vc
from test_gpu_kv_layout import dev_ring

pytestmark = pytest.mark.gpu

DH = 128


def _hip():
    from mistral_inference import _hip
    return _hip


def _check(got, ref, S, what):
    ratio = (got.double() - ref).abs() / ac.tolerance(S)
    assert not bool(got.float().isnan().any()), what
    worst = int(ratio.argmax())
    row, col = divmod(worst, ratio.shape[1])
    assert float(ratio.max()) <= 1.0, (what, "err/tol", float(ratio.max()), "row", row, "head", col // DH, "dim", col % DH,
                                       "got", float(got[row, col]), "ref", float(ref[row, col]))


@functools.lru_cache(maxsize=None)
def _cons(H, Hkv, W):
    return ac.constructions(H, Hkv, W, vc.n_pos(W))


def _run(con, W, seen, new):
    h = _hip()
    qkv, ck, cv, q_start, kv_before = ac.prefill_inputs(con, W, seen, new)
    refs = [ac.ref_attention64(q, k, v, qpos, kpos, W, True) for q, k, v, qpos, kpos in ac.prefill_sequences(con, W, seen, new)]
    ref, S = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    dq, dqs, dkb = qkv.cuda(), q_start.cuda(), kv_before.cuda()
    for hm in (False, True):
        dk, dv = dev_ring(ck, hm), dev_ring(cv, hm)
        k0, v0 = dk.clone(), dv.clone()
        got = h.attn_verify(dq, con.H, dk, dv, dqs, dkb, len(new)).cpu()
        _check(got, ref, S, (con.name, W, seen, new, "head-major" if hm else "slot-major"))
        assert torch.equal(dk, k0) and torch.equal(dv, v0), "the leaf must not write the rings"


@pytest.mark.parametrize("m", vc.ROWS)
@pytest.mark.parametrize("W", vc.RINGS)
@pytest.mark.parametrize("H,Hkv", vc.HEADS)
def test_attn_verify_structured(H, Hkv, W, m):
    for con in _cons(H, Hkv, W):
        for seen in vc.seen_values(W):
            _run(con, W, [seen], [m])


def test_attn_verify_two_sequences():
    W, seen, new = vc.BATCH2
    for con in _cons(8, 2, W):
        _run(con, W, list(seen), list(new))

