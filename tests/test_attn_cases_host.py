"""CPU proof that the structured attention cases (attn_cases.py) have teeth at the shapes test_gpu_attn_structured.py runs:
an emulation of each kernel's online softmax stays inside the tolerance, every mutant of the operation is rejected by at least
one construction with max(err / tolerance) >= 3, the staircase takes rescales with live accumulators, and the N(0,1) inputs of
the headline prefill test take none (which is why the structured cases exist).

Heads do not interact in attention, so the host analysis runs one kv head with two query heads; of the two long prefill
cases the emulation runs five query blocks (the first three, the middle, the last) and the mutants a subset of the query
rows (both ends and every 37th row), which can only lower a measured ratio."""
import functools

import pytest
import torch

import attn_cases as ac

H, HKV = 2, 1
MIN_RATIO = 3.0


def _q_tiles(s, waves):
    """Query blocks to emulate: all of a short sequence; of a long one the first three, the middle and the last."""
    n = (s + waves * 32 - 1) // (waves * 32)
    return None if s <= 700 else sorted({0, 1, 2, n // 2, n - 1})


def _emulate(q, k, v, qpos, kpos, W, ref, S, waves=4, break_alpha=None):
    out, live = ac.online_softmax_emulation(q, k, v, qpos, kpos, W, waves=waves, break_alpha=break_alpha,
                                            q_tiles=_q_tiles(len(qpos), waves))
    done = ~out.float().isnan().any(dim=1)
    assert bool(done.any())
    return ac.err_ratio(out[done], ref[done], S[done]), live


def _rows(s):
    if s <= 700:
        return torch.arange(s)
    return torch.unique(torch.cat([torch.arange(130), torch.arange(s - 130, s), torch.arange(0, s, 37)]))


@functools.lru_cache(maxsize=None)
def prefill_report(ci):
    """{construction: {"honest": worst emulation ratio, "live": rescales with live state (least over sequences and block
    shapes), mutant: best ratio over sequences or None}}"""
    W, seen, new = ac.PREFILL_CASES[ci]
    rep = {}
    for con in ac.constructions(H, HKV, W, max(p + s for p, s in zip(seen, new))):
        r = {"honest": 0.0, "live": 1 << 30}
        for q, k, v, qpos, kpos in ac.prefill_sequences(con, W, seen, new):
            ref, S = ac.ref_attention64(q, k, v, qpos, kpos, W, True)
            for waves in (4, 8):
                ratio, live = _emulate(q, k, v, qpos, kpos, W, ref, S, waves=waves)
                r["honest"] = max(r["honest"], ratio)
                r["live"] = min(r["live"], live)
            for ba in ("O", "l"):
                ratio, _ = _emulate(q, k, v, qpos, kpos, W, ref, S, break_alpha=ba)
                r["alpha_" + ba] = max(r.get("alpha_" + ba, 0.0), ratio)
            sel = _rows(len(qpos))
            for name in ac.MASK_MUTANTS:
                mut = ac.mutate(name, k, v, qpos[sel], kpos, W, (ac.KT, False))
                if mut is None:
                    r.setdefault(name, None)
                    continue
                got, _ = ac.ref_attention64(q[sel], mut[0], mut[1], qpos[sel], mut[2], W, True, weight=mut[3])
                r[name] = max(r.get(name) or 0.0, ac.err_ratio(got, ref[sel], S[sel]))
        rep[con.name] = r
    return rep


@functools.lru_cache(maxsize=None)
def decode_report(W):
    c = ac.split_chunk(W, ac.attn_decode_splits(W))
    rep = {}
    for con in ac.constructions(H, HKV, W, 2 * W + 4, decode=True):
        r = {"honest": 0.0, "live": 0}
        for n in ac.decode_lens(W):
            q, k, v, qpos, kpos = ac.decode_sequence(con, W, n)
            ref, S = ac.ref_attention64(q, k, v, qpos, kpos, W, True)
            rk, rv = ac.fill_ring(con, W, n - 1)
            out, live = ac.decode_emulation(q[0], rk, rv, n - 1)
            r["honest"] = max(r["honest"], ac.err_ratio(out[None], ref, S))
            r["live"] += live
            for ba in ("O", "l"):
                for where in ("group", "merge"):
                    out, _ = ac.decode_emulation(q[0], rk, rv, n - 1, break_alpha=ba, where=where)
                    key = f"{where}_{ba}"
                    r[key] = max(r.get(key, 0.0), ac.err_ratio(out[None], ref, S))
            extra = (n, rk[n], rv[n]) if n < W else None       # the slot past kv_len holds what position n would bring
            for name in ac.MASK_MUTANTS:
                mut = ac.mutate(name, k, v, qpos, kpos, W, (c, True), extra=extra)
                if mut is None:
                    r.setdefault(name, None)
                    continue
                got, _ = ac.ref_attention64(q, mut[0], mut[1], qpos, mut[2], W, True, weight=mut[3])
                r[name] = max(r.get(name) or 0.0, ac.err_ratio(got, ref, S))
        rep[con.name] = r
    return rep


def best(rep, key):
    """Best construction's ratio for one mutant (None: the mutant changes nothing in this case)."""
    vals = [r[key] for r in rep.values() if r.get(key) is not None]
    return max(vals) if vals else None


PREFILL_KEYS = ac.MASK_MUTANTS + ["alpha_O", "alpha_l"]
DECODE_KEYS = [m for m in ac.MASK_MUTANTS if m != "window_plus_one"] + ["group_O", "group_l", "merge_O", "merge_l"]


@pytest.mark.parametrize("ci", range(len(ac.PREFILL_CASES)), ids=[str(c) for c in ac.PREFILL_CASES])
def test_prefill_cases(ci):
    rep = prefill_report(ci)
    for name, r in rep.items():
        assert r["honest"] <= 1.0, (name, r["honest"])
    assert rep["staircase"]["live"] >= 1
    for key in PREFILL_KEYS:
        b = best(rep, key)
        assert b is None or b >= MIN_RATIO, (key, {n: r.get(key) for n, r in rep.items()})


def test_prefill_every_mutant_applies_somewhere():
    for key in PREFILL_KEYS:
        assert any(best(prefill_report(ci), key) is not None for ci in range(len(ac.PREFILL_CASES))), key


@pytest.mark.parametrize("W", ac.DECODE_RINGS)
def test_decode_cases(W):
    rep = decode_report(W)
    for name, r in rep.items():
        assert r["honest"] <= 1.0, (name, r["honest"])
    assert rep["staircase"]["live"] >= 1
    for key in DECODE_KEYS:
        b = best(rep, key)
        assert b is not None and b >= MIN_RATIO, (key, {n: r.get(key) for n, r in rep.items()})


def test_decode_ring_overwrites_the_key_outside_the_window():
    """kp = qp - W cannot be seen by a decode kernel: its slot holds kp = qp.  The decode form of "one key too many" is the
    slot past kv_len (future_visible)."""
    for W in ac.DECODE_RINGS:
        for n in ac.decode_lens(W):
            assert n - 1 - W not in ac.ring_positions(W, n - 1).tolist()


def test_random_headline_inputs_take_no_live_rescale():
    """test_gpu_ops.test_attn_prefill[(4096, [0], [4096])] (seeds 22 / 23, one kv head of it): after a wave's first tile no
    rescale is ever taken, so a kernel that scaled l but not O would pass it."""
    Hh, Hkv, Dh, T = 4, 2, 128, 4096
    g = torch.Generator().manual_seed(23)
    qkv = torch.randn(T, (Hh + 2 * Hkv) * Dh, generator=g).to(ac.BF)
    nq, nkv = Hh * Dh, Hkv * Dh
    q = qkv[:, :nq].reshape(T, Hh, Dh)[:, :2]
    k = qkv[:, nq:nq + nkv].reshape(T, Hkv, Dh)[:, :1]
    v = qkv[:, nq + nkv:].reshape(T, Hkv, Dh)[:, :1]
    pos = torch.arange(T)
    _, live = ac.online_softmax_emulation(q, k, v, pos, pos, 4096, waves=8)
    assert live == 0


def test_split_geometry_matches_the_source_comments():
    assert [(ac.attn_decode_splits(W), ac.split_chunk(W, ac.attn_decode_splits(W))) for W in ac.DECODE_RINGS] == \
        [(3, 112), (32, 128), (32, 160)]


def teeth_table():
    rows = []
    for key in PREFILL_KEYS:
        vals = [best(prefill_report(ci), key) for ci in range(len(ac.PREFILL_CASES))]
        rows.append(("prefill", key, min(x for x in vals if x is not None)))
    for key in DECODE_KEYS:
        rows.append(("decode", key, min(best(decode_report(W), key) for W in ac.DECODE_RINGS)))
    return rows


if __name__ == "__main__":
    for ci in range(len(ac.PREFILL_CASES)):
        print(ac.PREFILL_CASES[ci], {n: (round(r["honest"], 3), r["live"]) for n, r in prefill_report(ci).items()})
    for W in ac.DECODE_RINGS:
        print(W, {n: (round(r["honest"], 3), r["live"]) for n, r in decode_report(W).items()})
    for row in teeth_table():
        print("%-8s %-18s %.3g" % row)
