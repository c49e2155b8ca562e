"""CPU proof that the verify-attention cases (attn_verify_cases.py on the inputs of attn_cases.py) have teeth where the feature
can go wrong, in the style of test_attn_cases_host.py: the mutant "the step's rows were written into the ring before the
attention" - a row reads, in the slot of a later row's position, that later row instead of the key W positions before it,
which is what both existing branches of the forward would do - is rejected by at least one construction with
max(err / tolerance) >= 3 at every (W, m, seen) of test_gpu_attn_verify.py where the ring wraps under the step, and changes
nothing elsewhere.  Heads do not interact: one kv head with two query heads.

Also here (no GPU needed): the argument checks of mi_attn_verify with never-dereferenced pointers, and the slot -> position
rule of csrc/attn_verify.hip against attn_cases.ring_positions."""
import functools

import pytest
import torch

import attn_cases as ac
import attn_verify_cases as vc

H, HKV = 2, 1
MIN_RATIO = 3.0


@functools.lru_cache(maxsize=None)
def _cons(W):
    return ac.constructions(H, HKV, W, vc.n_pos(W))


def _mutant_ratio(W, seen, m):
    """Best construction's max(err / tolerance) of the mutant, or None where it changes nothing."""
    best = None
    for con in _cons(W):
        (q, k, v, qpos, kpos), = ac.prefill_sequences(con, W, [seen], [m])
        w = vc.overwritten_first(qpos, kpos, W)
        if w is None:
            return None
        ref, S = ac.ref_attention64(q, k, v, qpos, kpos, W, True)
        got, _ = ac.ref_attention64(q, k, v, qpos, kpos, W, True, weight=w)
        best = max(best or 0.0, ac.err_ratio(got, ref, S))
    return best


@pytest.mark.parametrize("W", vc.RINGS)
def test_rows_written_first_are_caught(W):
    applied = 0
    for m in vc.ROWS:
        for seen in vc.seen_values(W):
            r = _mutant_ratio(W, seen, m)
            wraps = m >= 2 and seen + m - 1 >= W      # some later row's slot holds a key an earlier row sees
            assert (r is not None) == wraps, (W, seen, m, r)
            if r is not None:
                applied += 1
                assert r >= MIN_RATIO, (W, seen, m, r)
    assert applied >= 9, applied     # W - 1, W, W + 7 and 2 W + 3 at m = 2, 5, 8 (and more on the 16-slot ring)


def test_two_sequence_case_has_a_wrapping_and_a_wrapped_ring():
    W, seen, new = vc.BATCH2
    for p, m in zip(seen, new):
        assert _mutant_ratio(W, p, m) >= MIN_RATIO


def test_selector_offsets_probe_the_window_edges_per_row():
    """q of row i selects class (qp + d) % 128: d = -W % 128 is the class of kp = qp - W (must be absent), (1 - W) % 128 that of the
    oldest visible key - a different ring slot for every row of the step."""
    for W in vc.RINGS:
        assert {(-W) % 128, (1 - W) % 128} <= set(ac.selector_deltas(W))
        seen, m = 2 * W + 3, 8
        slots = {(seen + i - W + 1) % W for i in range(m)}
        assert len(slots) == min(m, W)


def _kernel_slot_position(W, p, s):
    """csrc/attn_verify.hip: position held by slot s when positions 0 .. p - 1 were written (negative: never written)."""
    if p <= 0:
        return -1
    last_slot = (p - 1) % W
    base = p - 1 - last_slot
    return base + s if s <= last_slot else base - W + s


@pytest.mark.parametrize("W", [1, 16, 300])
def test_kernel_slot_rule_matches_the_ring(W):
    for p in [0, 1, W - 1, W, W + 1, W + 7, 2 * W, 2 * W + 3]:
        if p < 0:
            continue
        want = ac.ring_positions(W, p - 1) if p > 0 else None
        for s in range(W):
            kp = _kernel_slot_position(W, p, s)
            if p > 0 and s < min(p, W):
                assert kp == int(want[s]) and kp % W == s and p - W <= kp < p, (W, p, s, kp)
            else:
                assert kp < 0, (W, p, s, kp)


def test_attn_verify_argument_checks():
    """Before any launch, by name; the pointers are never dereferenced (as test_fp8_host.py does)."""
    from mistral_inference import _hip
    L = _hip.lib()
    for name in ("mi_attn_verify", "mi_attn_verify_scratch_bytes", "mi_forward_verify", "mi_workspace_bytes_verify"):
        assert hasattr(L, name)

    def call(W=16, T=2, B=1, Hh=4, Hkv=2, Dh=128, lay=0, ld=1024, out=1, q_start=1):
        return L.mi_attn_verify(out, 1, ld, 1, 1, W, T, B, Hh, Hkv, Dh, q_start, 1, 1, lay, None)
    assert call(out=None) == -1 and call(q_start=None) == -1 and call(lay=2) == -1 and call(W=0) == -1
    assert call(lay=0x10) == -4 and b"MI_KV_E4M3" in L.mi_last_error_detail()
    assert call(lay=0x11) == -4
    assert call(T=9) == -4 and b"at most 8" in L.mi_last_error_detail()
    assert call(W=4097) == -4 and b"4096" in L.mi_last_error_detail()
    assert call(T=2, B=3) == -1 and b"m_b >= 1" in L.mi_last_error_detail()
    assert call(Dh=64) == -2 and call(Hh=5) == -2
    assert call(ld=1023) == -1 and b"ld" in L.mi_last_error_detail()
    # scratch: T * H * splits * (Dh + 2) floats, splits = blocks of 128 slots
    for T, Hh, W in [(1, 4, 16), (8, 32, 4096), (5, 12, 300)]:
        assert L.mi_attn_verify_scratch_bytes(T, Hh, 128, W) == (T * Hh * ((W + 127) // 128) * 130 * 4 + 255) // 256 * 256
    assert L.mi_attn_verify_scratch_bytes(0, 4, 128, 16) == 0
