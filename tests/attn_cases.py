"""Structured attention inputs with a sharp expected output, one fp64 reference, and torch emulations of the kernels' online
softmax (helpers for test_attn_cases_host.py and test_gpu_attn_structured.py; no test functions here).

Why: with N(0,1) q, K and V every key gets roughly the same weight and every row's running maximum is reached in its first
tile.  One wrong key then moves the output by less than the operator tests' tolerance, and the rescale branches of
csrc/attn_prefill.hip (deferred rescale, threshold 8 in the exp2 domain) and csrc/attn_decode_core.cuh (lagging maximum,
RESCALE_T = 8; split merges) only ever run from the initial state, where alpha = 0 multiplies zeros.

Constructions (every value exact in bf16; ring slot = position % W as in test_gpu_ops._ring_case):
  census      every K row of a kv head is the same random vector, V[kp] = onehot(kp % 128), q random.  All scores of a query are
              equal bit for bit, so out[d] = #(visible kp with kp % 128 == d) / #(visible kp): a key that is missing, extra,
              counted twice or fetched from the wrong V row moves one element by 1/n.  Teeth only while n <= 4096.
  selector(d) K[kp] = 16 onehot(kp % 128), V[kp] = onehot((kp // 128 + 64 (kp % 2) + kv head) % 128), q[qp] = 11.5 onehot((qp + d) % 128):
              scaled score 16.26 on the query's class, exactly 0 elsewhere; the output is 1/c on the dims of the c visible class
              keys and ~1e-7 elsewhere - a full-size signal at any window length that depends on the K row addresses.
              d in {0, 1, (1 - W) % 128, -W % 128} probes "kp = qp present", "kp = qp + 1 absent", "oldest visible key
              present", "kp = qp - W absent".
  staircase   K[kp] = tau(kp) e0 with integer tau, q = 8 e0, V ~ N(0,1): the scaled score tau / sqrt(2) is a step function
              of kp.  Steps of +-3, +-10, +-17 in tau (2.1, 7.1, 12.0 natural units) sit on 64-key tile boundaries, mid-tile and
              on decode split boundaries, total span <= 154 (109 natural units).  Runs of +3 drift past 8 / log2(e) = 5.55 with
              no single step doing so (the deferred path, P > 1); +-10 and +-17 rescale at once; falling runs leave the maximum
              in an early tile or split.

tolerance(S) = 2^-7 S + 1e-6 with S = softmax(..) |v|: P is rounded to bf16 for the P.V MFMA (<= 2^-9 relative, also while
P <= 2^8 under the deferred rescale), the output is rounded once (<= 2^-9 |out| <= 2^-9 S): 2^-8 S, doubled for fp32
accumulation and v_exp_f32.  Decode is fp32 throughout: the same rule is looser than it needs.

Teeth, measured on the CPU by test_attn_cases_host.py (fp64 output of the mutated operation against the honest reference;
the missing factors through the emulations).  Per mutant: the smallest, over the GPU cases where the mutant changes anything,
of the best construction's max(err / tolerance); the bound asserted is 3.  The honest emulations reach at most 0.69 (prefill,
staircase) and 0.45 (decode) of the tolerance.  census alone sees one key in 4096 at 3.9; the larger figures below are selector's.

  mutant                                     prefill    decode
  kp = qp - W visible                        3.0e+04    -         (decode: that slot holds kp = qp)
  oldest visible key dropped                 127        127
  kp = qp dropped                            127        128
  kp = qp + 1 visible                        3.0e+04    1.0e+06   (decode: the slot past kv_len)
  adjacent K rows swapped at tile edges      3.1e+04    4.9e+05   (decode: at split edges)
  adjacent V rows swapped at tile edges      3.1e+04    4.9e+05
  one 64-key tile skipped                    127        3.2e+05
  newest key counted twice                   120        121
  rescale factor missing from O              2.0e+06    896
  rescale factor missing from l              102        110
  merge factor missing from O (decode)       -          6.1e+07
  merge factor missing from l (decode)       -          127
"""
import torch

BF = torch.bfloat16
DH = 128
KT = 64                      # keys per prefill tile (attn_prefill.hip)
LOG2E = 1.4426950408889634
RESCALE_T = 8.0              # both kernels: rescale when the maximum grew by more than 2^8


# ------------------------------------------------------------------------------------------------ decode split geometry
def attn_decode_splits(W: int, slots: int = 128) -> int:
    """attn_decode.hip: attn_decode_splits (default MI_ATTN_SPLIT_SLOTS)."""
    per = slots
    if (W + per - 1) // per > 32:
        per = (((W + 31) // 32) + 15) & ~15
    return max((W + per - 1) // per, 1)


def split_chunk(W: int, n_splits: int) -> int:
    """attn_decode_core.cuh: split_chunk."""
    return ((W + n_splits - 1) // n_splits + 15) & ~15


def decode_lens(W: int):
    """pos + 1 values around the split and ring edges (deduplicated, order kept)."""
    c = split_chunk(W, attn_decode_splits(W))
    out = []
    for n in (1, c - 1, c, c + 1, 2 * c + 1, W - 1, W, W + 7, 2 * W + 3):
        if n >= 1 and n not in out:
            out.append(n)
    return out


# ------------------------------------------------------------------------------------------------------- fp64 reference
def visibility(qpos, kpos, W, causal):
    """[s, n] bool: qp - W < kp <= qp."""
    if not causal:
        return torch.ones(len(qpos), len(kpos), dtype=torch.bool)
    vis = kpos[None, :] <= qpos[:, None]
    if W is not None:
        vis &= kpos[None, :] > qpos[:, None] - W
    return vis


def ref_attention64(q, keys, vals, qpos, kpos, W, causal, weight=None):
    """out = softmax(q k^T / sqrt(Dh) + mask) v and S = softmax(..) |v| in fp64 from the bf16 inputs.

    q [s, H, Dh]; keys / vals [n, Hkv, Dh]; qpos [s], kpos [n] absolute positions.  One kv head (and a slab of queries) at a
    time, so that s = n = 4096 stays small in memory.  `weight` [s, n] replaces the 0/1 mask by a multiplicity (mutants)."""
    s, H, Dh = q.shape
    Hkv = keys.shape[1]
    R = H // Hkv
    w = visibility(qpos, kpos, W, causal).double() if weight is None else weight.double()
    out = torch.empty(s, H, Dh, dtype=torch.float64)
    S = torch.empty(s, H, Dh, dtype=torch.float64)
    for g in range(Hkv):
        kf, vf = keys[:, g].double(), vals[:, g].double()
        va = vf.abs()
        for lo in range(0, s, 1024):
            hi = min(lo + 1024, s)
            qf = q[lo:hi, g * R:(g + 1) * R].double()                      # [t, R, Dh]
            sc = torch.einsum("trd,nd->rtn", qf, kf) * (Dh ** -0.5)
            ww = w[lo:hi][None]
            sc = sc.masked_fill(ww == 0, float("-inf"))
            p = torch.exp(sc - sc.max(dim=-1, keepdim=True).values) * ww
            p = p / p.sum(dim=-1, keepdim=True)
            out[lo:hi, g * R:(g + 1) * R] = torch.einsum("rtn,nd->trd", p, vf)
            S[lo:hi, g * R:(g + 1) * R] = torch.einsum("rtn,nd->trd", p, va)
    return out.reshape(s, H * Dh), S.reshape(s, H * Dh)


def tolerance(S):
    return 2.0 ** -7 * S + 1e-6


def err_ratio(got, ref, S):
    """max over elements of |got - ref| / tolerance(S)."""
    return float(((got.double() - ref).abs() / tolerance(S)).max())


# -------------------------------------------------------------------------------------------------------- constructions
class Construction:
    """keys(kp) / vals(kp) -> [n, Hkv, Dh] bf16, queries(qp) -> [s, H, Dh] bf16, all functions of absolute positions."""

    def __init__(self, name, H, Hkv, keys, vals, queries):
        self.name, self.H, self.Hkv = name, H, Hkv
        self.keys, self.vals, self.queries = keys, vals, queries


def _onehot(idx, scale=1.0):
    o = torch.zeros(len(idx), DH)
    o[torch.arange(len(idx)), idx] = scale
    return o


def census(H, Hkv, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    kvec = torch.randn(Hkv, DH, generator=g).to(BF)

    def keys(kp):
        return kvec[None].expand(len(kp), Hkv, DH).contiguous()

    def vals(kp):
        return _onehot(kp % 128)[:, None].expand(len(kp), Hkv, DH).to(BF).contiguous()

    def queries(qp):
        gq = torch.Generator().manual_seed(2000 + seed + int(qp[0]))
        return torch.randn(len(qp), H, DH, generator=gq).to(BF)

    return Construction("census", H, Hkv, keys, vals, queries)


def selector_deltas(W):
    out = []
    for d in (0, 1, (1 - W) % 128, (-W) % 128):
        if d not in out:
            out.append(d)
    return out


def selector(H, Hkv, delta, name=None):
    """`delta`: an int, or a function of the query positions (decode_edge_delta)."""
    def keys(kp):
        return _onehot(kp % 128, 16.0)[:, None].expand(len(kp), Hkv, DH).to(BF).contiguous()

    def vals(kp):
        return torch.stack([_onehot((kp // 128 + 64 * (kp % 2) + g) % 128) for g in range(Hkv)], dim=1).to(BF)

    def queries(qp):
        d = delta(qp) if callable(delta) else delta
        return _onehot((qp + d) % 128, 11.5)[:, None].expand(len(qp), H, DH).to(BF).contiguous()

    return Construction(name or f"selector{delta}", H, Hkv, keys, vals, queries)


def decode_edge_delta(W):
    """Class offset that puts a class key on the FIRST slot of a split (the middle one of those the query reaches; with one
    split, on slot 64 or on the newest key): rows exchanged across a split edge then change the output."""
    c = split_chunk(W, attn_decode_splits(W))

    def delta(qp):
        out = []
        for p in qp.tolist():
            kv_len = min(p + 1, W)
            n_vis = (kv_len + c - 1) // c
            e = c * (n_vis // 2) if n_vis >= 2 else (KT if kv_len > KT else p % W)
            out.append((int(ring_positions(W, p)[e]) - p) % 128)
        return torch.tensor(out)

    return delta


def staircase_tau(n_pos, edges, seed=0):
    """Integer tau[kp] for kp in [0, n_pos): a walk with steps +-3 (in runs of 3-4), +-10, +-17 kept inside [-77, 77]; step
    positions are drawn from `edges` (tile / mid-tile / split boundaries) first, about 60 of them (more on long ranges)."""
    g = torch.Generator().manual_seed(3000 + seed)
    n_steps = max(1, min(n_pos // 3, max(60, n_pos // 80)))
    pool = sorted({int(e) for e in edges if 0 < e < n_pos})
    if len(pool) > n_steps:
        pick = torch.randperm(len(pool), generator=g)[:n_steps].tolist()
        pos = sorted(pool[i] for i in pick)
    else:
        rest = [p for p in torch.randperm(n_pos - 1, generator=g).add(1).tolist() if p not in set(pool)]
        pos = sorted(pool + rest[:n_steps - len(pool)])
    steps = []      # relative to the drift direction: three moves in four go with it
    while len(steps) < len(pos):
        kind = int(torch.randint(0, 3, (1,), generator=g))
        sign = 1 if int(torch.randint(0, 4, (1,), generator=g)) else -1
        if kind == 0:
            steps += [3 * sign] * int(torch.randint(3, 5, (1,), generator=g))
        else:
            steps.append(sign * (10 if kind == 1 else 17))
    tau = torch.zeros(n_pos, dtype=torch.int64)
    level, prev, drift = -60, 0, 1      # a triangle wave between the bounds: rising stretches, then falling ones
    for p, st in zip(pos, steps):
        tau[prev:p] = level
        st *= drift
        if abs(level + st) > 77:
            st, drift = -st, -drift
        level, prev = level + st, p
    tau[prev:] = level
    return tau


def staircase(H, Hkv, n_pos, edges, seed=0):
    tau = staircase_tau(n_pos, edges, seed)
    g = torch.Generator().manual_seed(4000 + seed)
    vtab = torch.randn(n_pos, Hkv, DH, generator=g).to(BF)

    def keys(kp):
        k = torch.zeros(len(kp), Hkv, DH)
        k[:, :, 0] = tau[kp.clamp(max=n_pos - 1)].float()[:, None]
        return k.to(BF)

    def vals(kp):
        return vtab[kp.clamp(max=n_pos - 1)]

    def queries(qp):
        q = torch.zeros(len(qp), H, DH)
        q[:, :, 0] = 8.0
        return q.to(BF)

    c = Construction("staircase", H, Hkv, keys, vals, queries)
    c.tau = tau
    return c


def tile_edges(n_pos, W=None):
    """Candidate step positions: 64-key tile boundaries, mid-tile, and (W given) decode split boundaries in slot space."""
    e = set(range(KT, n_pos, KT)) | set(range(29, n_pos, KT))
    if W is not None:
        c = split_chunk(W, attn_decode_splits(W))
        e |= {kp for kp in range(1, n_pos) if (kp % W) % c == 0}
    return e


def constructions(H, Hkv, W, n_pos, decode=False):
    """Every construction of one case: census, selector for each delta, staircase.  Decode: kp = qp - W has been overwritten
    in the ring (its slot holds kp = qp), so the fourth offset probes a split edge instead."""
    cons = [census(H, Hkv)]
    if decode:
        cons += [selector(H, Hkv, d) for d in sorted({0, 1, (1 - W) % 128})]
        cons.append(selector(H, Hkv, decode_edge_delta(W), name="selector_edge"))
    else:
        cons += [selector(H, Hkv, d) for d in selector_deltas(W)]
    cons.append(staircase(H, Hkv, n_pos, tile_edges(n_pos, W if decode else None)))
    return cons


# ------------------------------------------------------------------------------------------------------------- cases
PREFILL_CASES = [            # (W, seen, new)
    (64, [0], [200]),                              # W equals the tile size
    (100, [250], [300]),                           # wrapped ring, tiles wrap mid-tile, ring / activation seam
    (1000, [1000, 0, 37], [300, 520, 129]),
    (4096, [4096], [600]),
    (4096, [0], [4096]),
]
DECODE_RINGS = [300, 4096, 5000]


def ring_positions(W, last):
    """Position held by every slot after tokens 0..last were written at slot p % W.  Slots never written hold what position
    `slot` WOULD bring (a future key): a kernel that reads one slot too many sees kp = qp + 1."""
    slot = torch.arange(W)
    p = last - ((last - slot) % W)
    return torch.where(p >= 0, p, slot)


def fill_ring(con, W, last):
    kp = ring_positions(W, last)
    return con.keys(kp), con.vals(kp)


def prefill_sequences(con, W, seen, new):
    """Per sequence: (q [s, H, Dh], keys, vals [n, Hkv, Dh], qpos, kpos) - the keys the window can reach, oldest first."""
    seqs = []
    for p, s in zip(seen, new):
        n_old = min(p, W)
        kpos = torch.arange(p - n_old, p + s)
        qpos = torch.arange(p, p + s)
        seqs.append((con.queries(qpos), con.keys(kpos), con.vals(kpos), qpos, kpos))
    return seqs


def prefill_inputs(con, W, seen, new):
    """Host tensors of one mi_attn_prefill call: qkv [T, (H + 2 Hkv) Dh], rings [B, W, Hkv, Dh], q_start, kv_before."""
    H, Hkv = con.H, con.Hkv
    rows, ck, cv = [], [], []
    for p, s in zip(seen, new):
        qpos = torch.arange(p, p + s)
        rows.append(torch.cat([con.queries(qpos).reshape(s, -1), con.keys(qpos).reshape(s, -1), con.vals(qpos).reshape(s, -1)], dim=1))
        k, v = fill_ring(con, W, p - 1)
        ck.append(k)
        cv.append(v)
    q_start = torch.tensor([0] + list(torch.tensor(new).cumsum(0)), dtype=torch.int32)
    return torch.cat(rows), torch.stack(ck), torch.stack(cv), q_start, torch.tensor(seen, dtype=torch.int32)


def decode_sequence(con, W, n):
    """One decode query at position n - 1 (n tokens seen, the new one included): q [1, H, Dh], keys, vals, qpos, kpos."""
    kpos = torch.arange(max(0, n - W), n)
    qpos = torch.tensor([n - 1])
    return con.queries(qpos), con.keys(kpos), con.vals(kpos), qpos, kpos


def decode_inputs(con, W, lens):
    """Host tensors of one mi_attn_decode call: q [B, H Dh], rings [B, W, Hkv, Dh], pos."""
    q = torch.cat([con.queries(torch.tensor([n - 1])).reshape(1, -1) for n in lens])
    rings = [fill_ring(con, W, n - 1) for n in lens]
    return q, torch.stack([r[0] for r in rings]), torch.stack([r[1] for r in rings]), torch.tensor([n - 1 for n in lens], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------------------ mutants
MASK_MUTANTS = ["window_plus_one", "oldest_dropped", "diag_dropped", "future_visible", "k_rows_swapped", "v_rows_swapped",
                "tile_skipped", "newest_twice"]


def mutate(name, keys, vals, qpos, kpos, W, edge, extra=None):
    """One wrong operation as (keys, vals, kpos, weight [s, n]) or None where it changes nothing.  `edge`: tile size whose
    multiples (of the absolute position; decode: of the ring slot) are the tile edges.  `extra` = (kp, K row, V row): a key
    outside the honest set that the mutant may reach (prefill: none needed, the rows exist; decode: the next slot)."""
    w = visibility(qpos, kpos, W, True).double()
    honest = w.clone()
    k, v, kp = keys, vals, kpos
    if name in ("window_plus_one", "future_visible"):
        tgt = qpos - W if name == "window_plus_one" else qpos + 1
        if extra is not None and bool((tgt == extra[0]).any()) and not bool((kp == extra[0]).any()):
            kp = torch.cat([kp, torch.tensor([extra[0]])])
            k, v = torch.cat([k, extra[1][None]]), torch.cat([v, extra[2][None]])
            w = torch.cat([w, torch.zeros(len(qpos), 1, dtype=w.dtype)], dim=1)
            honest = w.clone()
        w = w + (kp[None, :] == tgt[:, None]).double()
    elif name == "oldest_dropped":
        first = torch.argmax((w > 0).int(), dim=1)
        w[torch.arange(len(qpos)), first] = 0
        w[honest.sum(1) == 1] = honest[honest.sum(1) == 1]      # (a query with one key keeps it: nothing else to attend to)
    elif name == "diag_dropped":
        w = w - (kp[None, :] == qpos[:, None]).double()
        w[honest.sum(1) == 1] = honest[honest.sum(1) == 1]
    elif name == "newest_twice":
        w = w + (kp[None, :] == qpos[:, None]).double()
    elif name in ("k_rows_swapped", "v_rows_swapped"):
        idx = torch.arange(len(kp))
        slot = kp % W if edge[1] else kp
        at = torch.nonzero((slot[1:] % edge[0] == 0) & (kp[1:] == kp[:-1] + 1))[:, 0] + 1     # rows at - 1, at swap
        if len(at) == 0:
            return None
        idx[at], idx[at - 1] = at - 1, at
        if name == "k_rows_swapped":
            k = keys[idx]
        else:
            v = vals[idx]
        if torch.equal(k, keys) and torch.equal(v, vals):
            return None
    elif name == "tile_skipped":
        slot = kp % W if edge[1] else kp
        tiles = torch.unique(slot // KT)
        t = tiles[len(tiles) // 2]
        w = w * (slot // KT != t).double()[None]
        w[w.sum(1) == 0] = honest[w.sum(1) == 0]
    else:
        raise KeyError(name)
    if torch.equal(w, honest) and k is keys and v is vals:
        return None
    return k, v, kp, w


# ----------------------------------------------------------------------------------------------- kernel emulations (CPU)
def online_softmax_emulation(q, keys, vals, qpos, kpos, W, causal=True, waves=4, break_alpha=None, q_tiles=None):
    """The tile loop of attn_prefill_kernel<waves> for one sequence in fp32 torch: 64-key tiles from the block's first needed
    key, wave-uniform deferred rescale (threshold 8 in the exp2 domain) per 32 query rows, P rounded to bf16 for P.V, l summed
    unrounded, bf16 output.  Returns (out [s, H Dh] bf16, rescales taken by a wave in which some row had l > 0 and alpha < 1).
    break_alpha = "O" / "l": the rescale factor is not applied to the accumulator / to l.  q_tiles: only these query blocks
    (the other rows come back as NaN)."""
    s, H, Dh = q.shape
    Hkv = keys.shape[1]
    R = H // Hkv
    QB = waves * 32
    sc = torch.tensor(Dh ** -0.5, dtype=torch.float32) * LOG2E
    p_b, k0, k_last = int(qpos[0]), int(kpos[0]), int(kpos[-1])
    kf = keys.float().repeat_interleave(R, dim=1)      # [n, H, Dh]
    vf = vals.float().repeat_interleave(R, dim=1)
    out = torch.full((s, H, Dh), float("nan"), dtype=BF)
    live = 0
    for qt in (range((s + QB - 1) // QB) if q_tiles is None else q_tiles):
        qi = qt * QB + torch.arange(QB)
        active = (qi - qi % 32) < s                                    # wave_active, per row
        qp = p_b + qi.clamp(max=s - 1)
        blk_lo, blk_hi = p_b + qt * QB, p_b + min(qt * QB + QB - 1, s - 1)
        kp_lo = max(k0, blk_lo - W + 1) if causal else k0
        kp_hi = blk_hi if causal else k_last
        qf = q[qi.clamp(max=s - 1)].float().permute(1, 0, 2)           # [H, QB, Dh]
        m = torch.full((H, QB), -1e30)
        l = torch.zeros(H, QB)
        acc = torch.zeros(H, QB, Dh)
        vis_hi = torch.minimum(qp, torch.tensor(kp_hi)) if causal else torch.full_like(qp, kp_hi)
        vis_lo = qp - W if causal else torch.full_like(qp, -1)
        for it in range((kp_hi - kp_lo + KT) // KT):
            kp = kp_lo + it * KT + torch.arange(KT)
            idx = kp.clamp(max=kp_hi) - k0
            st = torch.einsum("hqd,khd->hqk", qf, kf[idx])
            vis = (kp[None, :] <= vis_hi[:, None]) & (kp[None, :] > vis_lo[:, None]) & active[:, None]
            st = st.masked_fill(~vis[None], float("-inf"))
            m_cand = torch.maximum(m, st.max(dim=-1).values)
            trig = ((m_cand - m) * sc > RESCALE_T).view(H, waves, 32).any(-1, keepdim=True).expand(H, waves, 32).reshape(H, QB)
            alpha = torch.where(trig, torch.exp2((m - m_cand) * sc), torch.ones(()))
            live += int((trig & (l > 0) & (alpha < 1)).view(H, waves, 32).any(-1).sum())
            m = torch.where(trig, m_cand, m)
            p = torch.exp2(st * sc - (m * sc)[..., None])
            l = l * (1.0 if break_alpha == "l" else alpha) + p.sum(-1)
            acc = acc * (1.0 if break_alpha == "O" else alpha[..., None]) + torch.einsum("hqk,khd->hqd", p.to(BF).float(), vf[idx])
        rows = qi[qi < s]
        out[rows] = (acc / l[..., None]).permute(1, 0, 2)[: len(rows)].to(BF)
    return out.reshape(s, H * Dh), live


def decode_emulation(q, ring_k, ring_v, pos, break_alpha=None, where="group"):
    """attn_decode_core.cuh for one sequence in fp32 torch: splits of split_chunk slots, 16 lane groups per split that visit
    slots s_begin + group + 16 j in ascending order with the lagging maximum, then groups -> split -> output merges.
    Returns (out [H Dh] bf16, lane-group rescales taken with l > 0).  break_alpha = "O" / "l" drops the factor from the
    accumulator / from l, in the lane group's rescale (where="group") or in the merges (where="merge")."""
    H, Dh = q.shape[-2], q.shape[-1]
    W, Hkv = ring_k.shape[0], ring_k.shape[1]
    R = H // Hkv
    ns = attn_decode_splits(W)
    c = split_chunk(W, ns)
    kv_len = min(pos + 1, W)
    sc = torch.rsqrt(torch.tensor(float(Dh))) * LOG2E
    qf = (q.reshape(H, Dh).float() * sc).view(Hkv, R, Dh)
    slot = torch.arange(ns * c)
    valid = ((slot < kv_len) & (slot < W)).view(ns, c // 16, 16)
    src = slot.clamp(max=max(kv_len - 1, 0))
    out = torch.empty(Hkv, R, Dh)
    live = 0
    bo = break_alpha == "O" and where == "group"
    bl = break_alpha == "l" and where == "group"
    for g in range(Hkv):
        d = torch.einsum("rd,nd->rn", qf[g], ring_k[src, g].float()).view(R, ns, c // 16, 16)
        v = ring_v[src, g].float().view(ns, c // 16, 16, Dh)
        m = torch.full((R, ns, 16), -1e30)
        l = torch.zeros(R, ns, 16)
        acc = torch.zeros(R, ns, 16, Dh)
        for j in range(c // 16):
            dj, vj = d[:, :, j], valid[None, :, j]
            grow = vj & (dj > m + RESCALE_T)
            mn = torch.where(grow, dj, m)
            alpha = torch.exp2(m - mn)
            live += int((grow & (l > 0)).sum())
            l = l * (1.0 if bl else alpha)
            acc = acc * (1.0 if bo else alpha[..., None])
            m = mn
            p = torch.where(vj, torch.exp2(dj - m), torch.zeros(()))
            l = l + p
            acc = acc + p[..., None] * v[None, :, j]
        M = m.amax(dim=(1, 2), keepdim=True)
        e = torch.exp2(m - M)
        eo = torch.ones_like(e) if (break_alpha == "O" and where == "merge") else e
        el = torch.ones_like(e) if (break_alpha == "l" and where == "merge") else e
        out[g] = (acc * eo[..., None]).sum(dim=(1, 2)) / (l * el).sum(dim=(1, 2))[:, None]
    return out.reshape(H * Dh).to(BF), live
