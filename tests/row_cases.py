"""Structured exact cases for the row kernels of csrc/elementwise.hip: greedy_rows_kernel, rmsnorm_kernel<NP>, rope_kernel,
moe_router_kernel, kv_write_kernel (bf16 rings) and the logprob_rows / logprob_finalize kernels.

Per kernel this module holds (a) constructions whose expected output is sharp - a chosen slot holds the maximum, a sum of squares
is exact in fp32 in any order, a table entry or a ring slot spells its own address -, (b) one high-precision reference (fp64, or
exact integer / copy arithmetic) and (c) a torch emulation of the kernel's INDEX logic with a `mutant` argument: with mutant=None
it equals the reference, with a named single fault it shows what that fault does to the expected output.  `mismatch()` is the
comparison the GPU test applies (test_gpu_rows_structured.py); test_row_cases_host.py uses the same function to prove, on the
CPU, that every mutant is caught on every case it applies to - or is provably invisible there, for a stated and asserted reason.

Every group exposes the same interface through GROUPS[name]: cases(), inputs(case), expected(case), emulate(case, mutant),
mutants_of(case), invisible(case, mutant) -> reason or None, mismatch(case, got, want) -> text or None, conditions(case)."""
import collections
import functools
import types

import torch

import mistral_oracle as mo

BF = torch.bfloat16
NEG_INF = float("-inf")


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) & 0x7fffffff)


def bf_round(x):
    return x.float().to(BF).float()


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t


def lsb_exponent(t):
    """The smallest e such that some nonzero element of the fp64 tensor has its last set bit at 2^e."""
    m, e = torch.frexp(t[t != 0].double())
    mi = (m.abs() * 2.0 ** 53).long()
    low = mi & -mi
    return int((e.long() - 53 + torch.log2(low.double()).long()).min())


def first_diff(got, want):
    """None when bit-equal, else a short text naming the first differing element."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    ne = bits(got) != bits(want)
    if got.dtype.is_floating_point:
        ne = ne & ~(torch.isnan(got.float()) & torch.isnan(want.float()) & (bits(got) == bits(want)))
    if not bool(ne.any()):
        return None
    i = tuple(int(v) for v in ne.nonzero()[0])
    return f"{int(ne.sum())} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


# ======================================================================================================================= greedy
# greedy_rows_kernel: block b reduces row b.  Vector form ((V & 3) == 0 and the row 16-byte aligned): thread t walks the float4s
# q = t + 4096 r (trip r) and q + 1024 k, k < 4 - slot e = 4 k + c of the trip is element (q + 1024 k) * 4 + c.  Scalar form:
# thread t walks elements t + 1024 r.  Then a 64-lane butterfly and a serial merge of the 16 waves, both on (max, lowest index).
GREEDY_VEC_V = (4, 16, 4092, 4096, 4100, 16384, 16388, 32768, 131072)
GREEDY_SCALAR_V = (1, 5, 1023, 1025, 32773)
LP_TOL = 2e-5            # what test_gpu_greedy.py and test_gpu_sampling.py hold this quantity to
PAD_LOGIT = 1000.0       # pad columns [V, ld): above every logit, a read past V wins the argmax
PEAK, TIE = 3.0, 3.0     # placements: the background stays <= -1
I_NONE = 0x7fffffff

GreedyCase = collections.namedtuple("GreedyCase", "V layout")   # layout: dense (ld = V) | pad (ld > V, rows keep their form) |
#                                                                 odd (ld = V + 2: even rows 16-byte aligned, odd rows not)
GREEDY_MUTANTS = ["ge_trip", "ascending_first", "merge_no_index", "tail_mask_absent", "idx_drop_k", "idx_drop_c", "idx_k_by_first",
                  "idx_q_unscaled", "pad_read", "inf_unguarded"]


def vec_index(thread, trip, slot):
    return ((thread + 4096 * trip) + (slot >> 2) * 1024) * 4 + (slot & 3)


def greedy_cases():
    out = [GreedyCase(V, lay) for V in GREEDY_VEC_V for lay in ("dense", "pad", "odd")]
    return out + [GreedyCase(V, lay) for V in GREEDY_SCALAR_V for lay in ("dense", "pad")]


def greedy_ld(case):
    return {"dense": case.V, "pad": case.V + (8 if case.V % 4 == 0 else 3), "odd": case.V + 2}[case.layout]


def greedy_placements(V):
    """(label, single index | (first, second) tie pair | 'all') - every index below V, duplicates dropped."""
    singles, ties = [], []
    if V % 4 == 0:
        singles += [(f"t0/slot{e}", vec_index(0, 0, e)) for e in range(16)]
        singles += [(f"t1023/slot{e}", vec_index(1023, 0, e)) for e in range(16)]
        singles += [(f"t5/trip1/slot{e}", vec_index(5, 1, e)) for e in range(16)] + [(f"t0/trip1/slot{e}", vec_index(0, 1, e)) for e in range(4)]
        ties += [("same float4", vec_index(3, 0, 1), vec_index(3, 0, 3)), ("two float4 of a trip", vec_index(3, 0, 2), vec_index(3, 0, 9)),
                 ("trip 0 / trip 1", vec_index(7, 0, 6), vec_index(7, 1, 6)), ("trip 0 late slot / trip 1 slot 0", vec_index(7, 0, 13), vec_index(7, 1, 0)),
                 ("neighbours, upper thread first", vec_index(6, 0, 1), vec_index(5, 0, 5)), ("neighbours", vec_index(5, 0, 3), vec_index(6, 0, 0)),
                 ("waves, upper wave first", vec_index(900, 0, 0), vec_index(100, 0, 4)), ("waves 0 / 1", vec_index(0, 0, 6), vec_index(64, 0, 2))]
    singles += [("first", 0), ("s1023", 1023), ("s1024", 1024), ("s5/trip1", 5 + 1024), ("s1023/trip1", 2047), ("last", V - 1)]
    ties += [("scalar trips", 7, 7 + 1024), ("scalar neighbours", 7, 8), ("scalar wrap, upper thread first", 5, 1024), ("scalar waves, upper wave first", 900, 100 + 1024),
             ("ends", 0, V - 1), ("middle", V // 2 - 1, V // 2)]
    out, seen = [], set()
    for label, i in singles:
        if 0 <= i < V and i not in seen:
            seen.add(i)
            out.append((label, i))
    for label, a, b in ties:
        a, b = min(a, b), max(a, b)
        if 0 <= a < b < V and (a, b) not in seen:
            seen.add((a, b))
            out.append((label, (a, b)))
    return out + [("all equal", "all")]


def greedy_rows(V):
    """(labels, fp32 [R, V]).  Background -1 - (7919 i mod 1009) / 256: exact in fp32, at most -1, no structure a stride could hide."""
    i = torch.arange(V, dtype=torch.int64)
    bg = (-1.0 - ((i * 7919) % 1009).double() / 256.0).float()
    labels, rows = [], []

    def add(label, row):
        labels.append(label)
        rows.append(row)
    for label, where in greedy_placements(V):
        row = bg.clone()
        if where == "all":
            row[:] = -3.25                         # also the log-probability row with result -log V
        elif isinstance(where, tuple):
            row[list(where)] = TIE
        else:
            row[where] = PEAK
        add(label, row)
    row = bg.clone()
    row[V // 3] = 60.0
    add("lp peaked", row)                          # exp(-61) per other logit: 0 to rounding
    add("lp +-80", torch.where(i % 3 == 0, 80.0, -80.0).float())
    if V >= 2:
        row = bg.clone()
        row[V - 1] = PEAK
        row[min(3, V - 2)] = NEG_INF
        add("-inf low", row)                       # scalar form: the first element of its thread
        trip = [vec_index(2, 0, e) for e in range(16) if vec_index(2, 0, e) < V - 1] or list(range(V - 1))
        row = bg.clone()
        row[V - 1] = PEAK
        row[trip] = NEG_INF
        add("-inf trip", row)                      # vector form: all sixteen slots of thread 2's first trip
        row = bg.clone()
        row[0] = PEAK
        row[(V + 1) // 2:] = NEG_INF
        add("-inf tail", row)                      # as test_gpu_sampling.py v32768_neg_inf: whole threads see nothing finite
    return labels, torch.stack(rows)


@functools.lru_cache(maxsize=2)
def greedy_inputs(case):
    """labels, the [R, ld] buffer (pad columns = PAD_LOGIT) - the logits are its view [:, :V].  In the odd layout every row appears
    twice in a row, so each placement runs through the vector loop (even row) and the scalar loop (odd row) of one launch."""
    labels, x = greedy_rows(case.V)
    if case.layout == "odd":
        labels = [f"{l} ({f})" for l in labels for f in ("aligned", "unaligned")]
        x = x.repeat_interleave(2, dim=0)
    buf = torch.full((x.shape[0], greedy_ld(case)), PAD_LOGIT, dtype=torch.float32)
    buf[:, :case.V] = x
    return labels, buf


def greedy_expected(case):
    _, buf = greedy_inputs(case)
    x = buf[:, :case.V]
    tok = torch.argmax(x, dim=-1)
    lp = torch.log_softmax(x.double(), dim=-1).gather(1, tok[:, None])[:, 0]
    return tok, lp


def greedy_row_is_vector(case, n_rows, V_eff=None):
    V = case.V if V_eff is None else V_eff
    ld = greedy_ld(case)
    return torch.tensor([(V & 3) == 0 and (b * ld * 4) % 16 == 0 for b in range(n_rows)])


def _exp_terms(x, M, mutant):
    """exp(x - M) as the kernel accumulates it; the guarded form subtracts a finite stand-in while M is still -inf."""
    if mutant != "inf_unguarded":
        M = torch.where(M == NEG_INF, torch.zeros_like(M), M)
    return torch.exp(x - M)


def _greedy_threads_vector(x, V, mutant, want_lp):
    R = x.shape[0]
    V4 = V >> 2
    trips = (V4 + 4095) // 4096
    f4 = torch.arange(trips * 4096)
    vals = x.reshape(R, V4, 4)[:, torch.clamp(f4, max=V4 - 1)]                        # the unconditional, clamped load
    if mutant != "tail_mask_absent":
        vals = torch.where((f4 < V4)[None, :, None], vals, torch.full_like(vals, NEG_INF))
    vals = vals.reshape(R, trips, 4, 1024, 4).permute(0, 1, 3, 2, 4).reshape(R, trips, 1024, 16).double()
    t = torch.arange(1024)
    M = torch.full((R, 1024), NEG_INF, dtype=torch.float64)
    S = torch.zeros((R, 1024), dtype=torch.float64)
    I = torch.full((R, 1024), I_NONE, dtype=torch.int64)
    for r in range(trips):
        q = t + 4096 * r
        entered = (q < V4)[None]
        xs = vals[:, r]
        cm = xs.max(dim=-1).values
        upd = ((cm >= M) if mutant == "ge_trip" else (cm > M)) & entered
        hit = (xs == cm[..., None]).to(torch.int8)
        first = 15 - hit.flip(-1).argmax(-1) if mutant == "ascending_first" else hit.argmax(-1)
        k, c = first >> 2, first & 3
        idx = {None: (q + k * 1024) * 4 + c, "idx_drop_k": q * 4 + c, "idx_drop_c": (q + k * 1024) * 4,
               "idx_k_by_first": (q + first * 1024) * 4 + c, "idx_q_unscaled": q + k * 1024 * 4 + c}.get(mutant, (q + k * 1024) * 4 + c)
        if want_lp:
            S = torch.where(upd, S * torch.exp(torch.where(upd, M - cm, torch.zeros_like(M))), S)
        M = torch.where(upd, cm, M)
        I = torch.where(upd, idx, I)
        if want_lp:
            S = torch.where(entered, S + _exp_terms(xs, M[..., None], mutant).sum(-1), S)
    return M, I, S


def _greedy_threads_scalar(x, V, mutant, want_lp):
    R = x.shape[0]
    trips = (V + 1023) // 1024
    vals = torch.full((R, trips * 1024), NEG_INF, dtype=torch.float64)
    vals[:, :V] = x.double()
    vals = vals.reshape(R, trips, 1024)
    t = torch.arange(1024)
    M = torch.full((R, 1024), NEG_INF, dtype=torch.float64)
    S = torch.zeros((R, 1024), dtype=torch.float64)
    I = torch.full((R, 1024), I_NONE, dtype=torch.int64)
    for r in range(trips):
        i = t + 1024 * r
        valid = (i < V)[None]
        xs = vals[:, r]
        gt = ((xs >= M) if mutant == "ge_trip" else (xs > M)) & valid
        if want_lp:
            S = torch.where(gt, S * torch.exp(torch.where(gt, M - xs, torch.zeros_like(M))) + 1.0,
                            torch.where(valid, S + _exp_terms(xs, M, mutant), S))
        M = torch.where(gt, xs, M)
        I = torch.where(gt, i[None].expand_as(I), I)
    return M, I, S


def _greedy_merge(M, I, S, mutant):
    def merge(a, b):
        (M, I, S), (m2, i2, s2) = a, b
        take = (m2 > M) if mutant == "merge_no_index" else (m2 > M) | ((m2 == M) & (i2 < I))
        Mn = torch.where(take, m2, M)
        f1 = torch.where(M == Mn, torch.ones_like(M), torch.exp(M - Mn))
        f2 = torch.where(m2 == Mn, torch.ones_like(M), torch.exp(m2 - Mn))
        return Mn, torch.where(take, i2, I), S * f1 + s2 * f2
    R = M.shape[0]
    st = tuple(v.reshape(R, 16, 64) for v in (M, I, S))
    lane = torch.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        st = merge(st, tuple(v[..., lane ^ o] for v in st))
    acc = tuple(v[:, 0, 0] for v in st)
    for j in range(1, 16):
        acc = merge(acc, tuple(v[:, j, 0] for v in st))
    return acc[1], -torch.log(acc[2])


def greedy_emulate(case, mutant=None, want_lp=True):
    """(token int64 [R], logprob fp64 [R]) by the kernel's own walk: per-thread trips, first-maximum scan, index formula, merges."""
    _, buf = greedy_inputs(case)
    R = buf.shape[0]
    V = greedy_ld(case) if mutant == "pad_read" else case.V
    vec = greedy_row_is_vector(case, R, V)
    M = torch.empty((R, 1024), dtype=torch.float64)
    S = torch.empty((R, 1024), dtype=torch.float64)
    I = torch.empty((R, 1024), dtype=torch.int64)
    for form, fn in ((vec, _greedy_threads_vector), (~vec, _greedy_threads_scalar)):
        if bool(form.any()):
            M[form], I[form], S[form] = fn(buf[form][:, :V], V, mutant, want_lp)
    return _greedy_merge(M, I, S, mutant)


def greedy_mutants_of(case):
    vec = case.V % 4 == 0
    return [m for m in GREEDY_MUTANTS if (vec or m not in ("ascending_first", "tail_mask_absent", "idx_drop_k", "idx_drop_c", "idx_k_by_first",
                                                           "idx_q_unscaled")) and (case.layout != "dense" or m != "pad_read")]


def greedy_thread_starts_on_inf(case):
    """Does some thread see nothing finite in its first trip (vector rows) or first element (scalar rows)?  Only there does the
    accumulation run while the maximum is still -inf."""
    _, buf = greedy_inputs(case)
    V = case.V
    vec = greedy_row_is_vector(case, buf.shape[0])
    hit = bool(torch.isinf(buf[~vec][:, :min(V, 1024)]).any())
    if bool(vec.any()):
        x = torch.full((int(vec.sum()), 16384), NEG_INF)
        x[:, :min(V, 16384)] = buf[vec][:, :min(V, 16384)]
        cm = x.reshape(-1, 4, 1024, 4).permute(0, 2, 1, 3).reshape(-1, 1024, 16).max(-1).values
        hit = hit or bool(torch.isinf(cm[:, :min(V >> 2, 1024)]).any())
    return hit


def greedy_invisible(case, m):
    V, vec, scalar = case.V, case.V % 4 == 0, case.V % 4 != 0 or case.layout == "odd"
    V4 = V >> 2
    if m == "ge_trip" and (not vec or V4 <= 4096) and (not scalar or V <= 1024) and not greedy_thread_starts_on_inf(case):
        return "no thread takes a second trip or starts on -inf: `>=` and `>` differ nowhere"
    if m == "merge_no_index" and (not vec or V4 <= 1024) and (not scalar or V <= 1024):
        return "every thread holds one run of consecutive indices: thread order is index order"
    if m == "tail_mask_absent" and V4 % 4096 == 0:
        return "V / 4 is a multiple of 4096: no trip has a slot past the row"
    if m == "idx_drop_k" and V4 <= 1024:
        return "no thread has a second float4: k = 0 in every trip"
    if m == "idx_q_unscaled" and V4 == 1:
        return "one float4: q = 0"
    if m == "inf_unguarded" and not greedy_thread_starts_on_inf(case):
        return "no thread starts on -inf (V = 1, or one thread holds the whole row): the maximum is finite before anything is added"
    return None


def greedy_mismatch(case, got, want):
    (tok, lp), (wtok, wlp) = got, want
    labels = greedy_inputs(case)[0]
    tok, lp = tok.cpu().long(), lp.cpu().double()
    bad = (tok != wtok).nonzero()
    if len(bad):
        r = int(bad[0])
        return f"row {r} ({labels[r]}): token {int(tok[r])}, want {int(wtok[r])} ({len(bad)} rows)"
    err = (lp - wlp).abs()
    bad = (~torch.isfinite(lp) | ~(err <= LP_TOL)).nonzero()
    if len(bad):
        r = int(bad[0])
        return f"row {r} ({labels[r]}): logprob {float(lp[r])!r}, want {float(wlp[r])!r} ({len(bad)} rows)"
    return None


def greedy_conditions(case):
    labels, buf = greedy_inputs(case)
    x = buf[:, :case.V]
    assert torch.equal(x.double().float(), x) and bool((buf[:, case.V:] == PAD_LOGIT).all()) and float(x.max()) < PAD_LOGIT
    top = x.max(dim=-1, keepdim=True).values
    n_max = (x == top).sum(-1)
    for lab, n in zip(labels, n_max.tolist()):       # ties only where they were placed
        want = case.V if "all equal" in lab else (case.V + 2) // 3 if "+-80" in lab else None
        if want is None:
            want = 2 if any(lab.startswith(t) for t in ("same", "two float4", "trip 0", "neighbours", "waves", "scalar", "ends", "middle")) else 1
        assert n == want, (case, lab, n)
    assert bool(torch.isfinite(greedy_expected(case)[1]).all())
    return {"rows": x.shape[0], "vector rows": int(greedy_row_is_vector(case, x.shape[0]).sum())}


# ====================================================================================================================== rmsnorm
# rmsnorm_kernel<NP>: one wave per row, four rows per block; lane l holds the 16-byte pieces l + 64 j, j < NP, loaded from
# min(l + 64 j, np - 1) and masked by l + 64 j < np; NP = 8 | 12 | 16 | 32 for D <= 4096 | 6144 | 8192 | 16384.
RMS_DS = (8, 504, 512, 520, 4096, 4104, 6144, 6152, 8192, 8200, 16384)
RMS_EPS = 1e-5
RMS_POISON = -77.0
HOT = 96.0               # 8 * 96^2 = 73728 against at most D <= 16384 from the rest of the row

RmsCase = collections.namedtuple("RmsCase", "D T kinds")     # kinds: one label per row


def rms_template(D):
    return 8 if D <= 4096 else 12 if D <= 6144 else 16 if D <= 8192 else 32


def rms_hot_positions(D):
    np_ = D >> 3
    pos = {0, 63, 64, np_ - 1} | {64 * j - 1 for j in range(1, (np_ + 63) // 64 + 1)}
    return sorted(p for p in pos if 0 <= p < np_)


def rms_cases():
    out = []
    for D in RMS_DS:
        out.append(RmsCase(D, 1, ("eps",)))
        out.append(RmsCase(D, 4, ("exact:-4", "exact:3", "zero", "eps")))
        hot = rms_hot_positions(D)
        for i in range(0, len(hot), 3):
            kinds = [f"hot@{p}" for p in hot[i:i + 3]]
            kinds += ["exact:7", "exact:0", "exact:1", "exact:2"][:5 - len(kinds)]
            out.append(RmsCase(D, 5, tuple(kinds)))
    return out


def rms_weight(D):
    c = torch.arange(D)
    return (1.0 + ((3 * (c >> 3) + (c & 7)) % 8).float() / 8.0).to(BF)        # encodes its column; never equal one piece on


def rms_row(D, kind, r):
    g = gen(D, r, len(kind), sum(kind.encode()))
    if kind == "zero":
        return torch.zeros(D), 1.0
    if kind == "eps":
        return torch.randint(-3, 4, (D,), generator=g).float(), 2.0 ** -10      # mean square ~ 4e-6: eps = 1e-5 decides
    if kind.startswith("exact:"):
        return torch.randint(-3, 4, (D,), generator=g).float(), 2.0 ** int(kind[6:])
    p = int(kind[4:])
    row = torch.randint(-1, 2, (D,), generator=g).float()
    row[p * 8:p * 8 + 8] = HOT * (1 - 2 * torch.randint(0, 2, (8,), generator=g).float())
    return row, 2.0 ** ((p + r) % 5 - 2)


@functools.lru_cache(maxsize=None)
def rms_inputs(case):
    """(integer rows fp32 [T, D], per-row scale [T], x bf16 [T, D], w bf16 [D])."""
    rows, scales = zip(*(rms_row(case.D, k, r) for r, k in enumerate(case.kinds)))
    ints, scale = torch.stack(rows), torch.tensor(scales)
    return ints, scale, (ints * scale[:, None]).to(BF), rms_weight(case.D)


def rms_expected(case):
    _, _, x, w = rms_inputs(case)
    return mo.rms_norm(x, w, RMS_EPS)


def rms_expected_fp64(case):
    _, _, x, w = rms_inputs(case)
    xd = x.double()
    inv = 1.0 / torch.sqrt(xd.pow(2).mean(-1, keepdim=True) + float(torch.tensor(RMS_EPS, dtype=torch.float32)))
    return ((xd * inv).to(BF).double() * w.double()).to(BF)


def rms_emulate(case, mutant=None):
    """The kernel's fp32 chain on the exact sum of squares; a mutant changes which pieces enter the sum, the width, eps, whose 1/rms
    a row takes or which weight piece meets which column."""
    ints, scale, x, w = rms_inputs(case)
    D = case.D
    xd = x.double()
    ss = xd.pow(2).sum(-1)
    if mutant and mutant.split("@")[0] in ("drop", "dup"):
        p = int(mutant.split("@")[1])
        piece = xd[:, p * 8:p * 8 + 8].pow(2).sum(-1)
        ss = ss - piece if mutant.startswith("drop") else ss + piece
    width = 512 * (((D >> 3) + 63) // 64) if mutant == "div_padded" else D
    eps = 0.0 if mutant == "eps_dropped" else RMS_EPS
    inv = 1.0 / torch.sqrt(ss.float() / torch.tensor(float(width)) + torch.tensor(eps, dtype=torch.float32))
    if mutant == "neighbour_inv":
        t = torch.arange(case.T)
        inv = inv[torch.where((t ^ 1) < case.T, t ^ 1, t)]
    if mutant == "w_shift":
        w = torch.roll(w, -8)
    return (bf_round(x.float() * inv[:, None]) * w.float()).to(BF)


def rms_mutants_of(case):
    out = ["div_padded", "neighbour_inv", "w_shift"]
    if "eps" in case.kinds or "zero" in case.kinds:
        out.append("eps_dropped")
    for k in case.kinds:
        if k.startswith("hot@"):
            out += [f"drop@{k[4:]}", f"dup@{k[4:]}"]
    return out


def rms_invisible(case, m):
    if m == "div_padded" and case.D % 512 == 0:
        return "D fills its 64-piece groups: the padded width is D"
    if m == "neighbour_inv" and case.T == 1:
        return "one row: no neighbour"
    if m == "w_shift" and case.D == 8:
        return "one piece: the shift wraps onto itself"
    return None


def rms_mismatch(case, got, want):
    d = first_diff(got.cpu(), want)
    return d and f"{d} (row kinds {case.kinds})"


def rms_conditions(case):
    ints, scale, x, w = rms_inputs(case)
    assert torch.equal(x.float(), ints * scale[:, None]) and torch.equal(ints, ints.round())        # bf16 holds every element
    assert float((ints.double() ** 2).sum(-1).max()) < 2 ** 24                                     # any partial sum is an exact fp32 integer
    assert not bool((w[8:] == w[:-8]).any())                                                         # a weight piece never equals the next one
    a, b, c = rms_expected(case), rms_emulate(case), rms_expected_fp64(case)
    assert first_diff(b, a) is None and first_diff(c, a) is None, (case, first_diff(b, a), first_diff(c, a))   # oracle == fp32 chain == fp64 chain
    assert not bool(torch.isnan(a.float()).any())
    if "zero" in case.kinds:
        assert not bool(a[case.kinds.index("zero")].float().any())
    return {"elements": a.numel()}


# ========================================================================================================================= rope
ROPE_LEN = 256
ROPE_POISON = 777.0
RopeCase = collections.namedtuple("RopeCase", "Dh H Hkv pad T table")       # table: real | sel
ROPE_MUTANTS = ["t_for_pos", "col_no_mod", "last_k_unrotated", "first_v_rotated", "ld_ignored"]


def rope_cases():
    return [RopeCase(Dh, H, Hkv, pad, T, tab) for Dh in (64, 80, 128, 256) for H, Hkv in ((4, 2), (3, 1)) for pad in (0, 8)
            for T in (1, 37, 300) for tab in ("real", "sel")]


def rope_positions(T):
    pos = [(t * 37 + 11) % ROPE_LEN for t in range(T)]
    pos[0] = ROPE_LEN - 1
    if T > 2:
        pos[2] = pos[1]
    return torch.tensor(pos, dtype=torch.int32)


@functools.lru_cache(maxsize=8)
def rope_inputs(case):
    """(buffer bf16 [T, ld] with poisoned pad columns, table fp32 [ROPE_LEN, Dh / 2, 2], positions int32 [T])."""
    Dh, H, Hkv, pad, T, tab = case
    width, rot = (H + 2 * Hkv) * Dh, (H + Hkv) * Dh
    buf = torch.full((T, width + pad), ROPE_POISON, dtype=BF)
    buf[:, :width] = torch.randn(T, width, generator=gen(*case[:5])).to(BF)
    if tab == "real":
        cs = mo.rope_angles(Dh, ROPE_LEN, 1e6)
    else:      # entry (pos, i) = (cos, sin) = (pos, i) against pairs (1, 0): the output pair names the entry that was read
        buf[:, :rot] = torch.tensor([1.0, 0.0]).repeat(rot // 2).to(BF)
        cs = torch.stack((torch.arange(ROPE_LEN).float()[:, None].expand(ROPE_LEN, Dh // 2),
                          torch.arange(Dh // 2).float()[None].expand(ROPE_LEN, Dh // 2)), dim=-1).contiguous()
    return buf, cs, rope_positions(T)


def rope_expected(case):
    Dh, H, Hkv, pad, T, tab = case
    buf, cs, pos = rope_inputs(case)
    rot = (H + Hkv) * Dh
    out = buf.clone()
    if tab == "real":
        out[:, :rot] = mo.apply_rope(buf[:, :rot].reshape(T, H + Hkv, Dh), cs[pos.long()]).reshape(T, rot)
    else:
        pair = torch.stack((pos.float()[:, None].expand(T, Dh // 2), torch.arange(Dh // 2).float()[None].expand(T, Dh // 2)), dim=-1)
        out[:, :rot] = pair.reshape(T, 1, Dh).expand(T, H + Hkv, Dh).reshape(T, rot).to(BF)
    return out


def rope_emulate(case, mutant=None):
    """The kernel's addressing on the flat buffer and the flat table: one (t, pair) at a time, in place."""
    Dh, H, Hkv, pad, T, tab = case
    buf, cs, pos = rope_inputs(case)
    width = (H + 2 * Hkv) * Dh
    ld = width if mutant == "ld_ignored" else width + pad
    rot = (H + Hkv) * Dh + {"last_k_unrotated": -Dh, "first_v_rotated": 8}.get(mutant, 0)
    flat = buf.clone().reshape(-1)
    t = torch.arange(T)[:, None]
    col = torch.arange(0, rot, 2)[None]
    i = (col if mutant == "col_no_mod" else col % Dh) >> 1
    p = t if mutant == "t_for_pos" else pos.long()[:, None]
    entry = cs.reshape(-1, 2)[torch.clamp(p * (Dh >> 1) + i, max=cs.numel() // 2 - 1)]      # (a wrong index may leave the table: clamped here)
    addr = t * ld + col
    a, b = flat[addr].float(), flat[addr + 1].float()
    c, s = entry[..., 0], entry[..., 1]
    flat[addr] = (a * c - b * s).to(BF)
    flat[addr + 1] = (a * s + b * c).to(BF)
    return flat.reshape(T, width + pad)


def rope_mutants_of(case):
    return [m for m in ROPE_MUTANTS if m != "ld_ignored" or case.pad]


def rope_invisible(case, m):
    if m == "ld_ignored" and case.T == 1:
        return "one token: row 0 starts at the base for any ld"
    return None


def rope_mismatch(case, got, want):
    return first_diff(got.cpu(), want)


def rope_conditions(case):
    Dh, H, Hkv, pad, T, tab = case
    buf, cs, pos = rope_inputs(case)
    assert int(pos.max()) == ROPE_LEN - 1 and (T == 1 or bool((pos[1:] < pos[:-1]).any())) and (T < 3 or int(pos[1]) == int(pos[2]))
    assert torch.equal(cs.to(BF).float(), cs) or tab == "real"                 # selector codes: integers bf16 holds
    want = rope_expected(case)
    if tab == "sel":        # the read-off equals the rotation formula
        rot = (H + Hkv) * Dh
        assert torch.equal(want[:, :rot], mo.apply_rope(buf[:, :rot].reshape(T, H + Hkv, Dh), cs[pos.long()]).reshape(T, rot))
    return {"pairs": T * (H + Hkv) * Dh // 2}


# ======================================================================================================================= router
# moe_router_kernel: logit_e = bf16(x . gate[e]) (fp32 fma chain, wave e), top-k by repeated first-maximum scans (ties: lowest id),
# softmax over the k picked, bf16.  norm form: x is first normalised as rmsnorm_kernel does.
ROUTER_PATTERNS = ("tie_top", "tie_cut", "all_equal", "round_tie", "distinct")
RouterCase = collections.namedtuple("RouterCase", "E k D T form")          # form: plain | norm
ROUTER_MUTANTS = ["tie_highest", "softmax_all_E", "logit_not_rounded"]


def router_cases():
    return [RouterCase(E, k, D, T, form) for E in (2, 8, 16) for k in (1, 2, 4) if k <= E for D in (8, 504, 512, 520, 4096) for T in (1, 5)
            for form in ("plain", "norm")]


def router_patterns(case):
    if case.T == 1:
        return (ROUTER_PATTERNS[(case.E + case.k + case.D // 8) % 5],)
    return ROUTER_PATTERNS


@functools.lru_cache(maxsize=None)
def router_inputs(case):
    """plain: (x bf16 [T, D], gate bf16 [E, D], None, chosen logits fp64 [T, E]).  Token t owns column cols[t] (x = 1 there, 0 in the
    other tokens' columns) whose gate entries are its chosen logits; the remaining columns come in far-apart pairs (c, c') with
    x[c] = x[c'] and gate[c'] = -gate[c], which cancel exactly in any order - unless a piece is dropped or read twice.  Column
    `inc` adds one unit to the highest expert, making the 257 that bf16 rounds onto the 256 of expert 0 ("round_tie").
    norm: (x = +-2^s, gate small integers / 8, norm weight +-2^(piece mod 3 - 1) with the sign set by the column, None): every
    normalised element is +-r_t w_c with one bf16 number r_t per token, so the logits are still exact fp32 sums."""
    E, k, D, T, form = case
    g = gen(E, k, D, T, len(form))
    if form == "norm":
        w = (2.0 ** ((torch.arange(D) >> 3) % 3 - 1).float() * (1 - 2 * (torch.arange(D) % 3 == 1).float())).to(BF)
        for attempt in range(64):     # drawn again until a router that skips the norm picks other experts for some token
            x = ((1 - 2 * torch.randint(0, 2, (T, D), generator=g).float()) * (2.0 ** torch.tensor([(-2, 0, 3, 1, -5)[t % 5] for t in range(T)]))[:, None]).to(BF)
            gate = (torch.randint(-2, 3, (E, D), generator=g).float() / 8).to(BF)
            with_norm = bf_round((_router_norm(x, w, True).double() @ gate.double().T).float())
            without = bf_round((x.double() @ gate.double().T).float())
            if not torch.equal(router_select(with_norm, k), router_select(without, k)):
                return x, gate, w, None
        raise AssertionError(case)
    cols = [(D - 1) - (t * (D - 1)) // max(T - 1, 1) for t in range(T)]
    inc = next(c for c in range(D) if c not in cols)
    free = torch.tensor([c for c in range(D) if c not in cols and c != inc], dtype=torch.long)
    free = free[torch.randperm(len(free), generator=g)]
    pc = free[:2 * (len(free) // 2)].view(-1, 2)
    x, gate = torch.zeros(T, D), torch.zeros(E, D)
    G = torch.randint(-2, 3, (E, len(pc)), generator=g).float()
    X = torch.randint(-3, 4, (T, len(pc)), generator=g).float()
    gate[:, pc[:, 0]], gate[:, pc[:, 1]] = G, -G
    x[:, pc[:, 0]], x[:, pc[:, 1]] = X, X
    gate[E - 1, inc] = 1.0
    x[:, inc] = 1.0
    perm = torch.randperm(E, generator=g).tolist()
    L = torch.zeros(T, E, dtype=torch.float64)
    sx = []
    for t, pat in enumerate(router_patterns(case)):
        v = torch.zeros(E, dtype=torch.float64)
        for j, e in enumerate(perm):
            v[e] = E + 2 - j
        if pat == "tie_top" or (pat == "tie_cut" and k == E):
            v[perm[1]] = v[perm[0]]
        elif pat == "tie_cut":
            v[perm[k]] = v[perm[k - 1]]
        elif pat == "all_equal":
            v[:] = 5
        elif pat == "round_tie":
            others = [e for e in range(1, E - 1)]
            v[0], v[E - 1] = 256, 257
            for j, e in enumerate(others):
                v[e] = 256 - 8 * (1 + j)
        L[t] = v
        sx.append(-3 if pat == "round_tie" else t % 3)
        gate[:, cols[t]] = (v - torch.tensor([0.0] * (E - 1) + [1.0], dtype=torch.float64)).float()
        x[t, cols[t]] = 1.0
    scale = 2.0 ** torch.tensor(sx, dtype=torch.float64)
    return (x * scale[:, None].float()).to(BF), (gate / 8).to(BF), None, L * scale[:, None] / 8


def _router_norm(x, w, fp64):
    eps32 = torch.tensor(RMS_EPS, dtype=torch.float32)
    if fp64:
        xd = x.double()
        inv = 1.0 / torch.sqrt(xd.pow(2).mean(-1, keepdim=True) + float(eps32))
        return ((xd * inv).to(BF).double() * w.double()).to(BF)
    ss = x.double().pow(2).sum(-1).float()
    inv = 1.0 / torch.sqrt(ss / torch.tensor(float(x.shape[1])) + eps32)
    return (bf_round(x.float() * inv[:, None]) * w.float()).to(BF)


def router_norm_x(case, fp64):
    """The bf16 rows the router's fused norm hands its dot products (== rmsnorm's output), by the fp64 or the fp32 chain."""
    x, _, w, _ = router_inputs(case)
    return _router_norm(x, w, fp64)


def router_select(logits, k, tie_highest=False):
    """Indices [T, k] of k repeated first-maximum scans (or last-maximum ones)."""
    T, E = logits.shape
    lg = logits.clone()
    out = torch.empty((T, k), dtype=torch.int64)
    for j in range(k):
        top = lg.max(dim=-1, keepdim=True).values
        hit = (lg == top).to(torch.int8)
        out[:, j] = E - 1 - hit.flip(-1).argmax(-1) if tie_highest else hit.argmax(-1)
        lg[torch.arange(T), out[:, j]] = NEG_INF
    return out


def router_expected(case):
    """(indices int64 [T, k], weights fp32 [T, k] = bf16(fp64 softmax), exact-weight mask [T]): fp64 logits of the bf16 inputs,
    rounded once to bf16; ties to the lowest expert id."""
    x, gate, w, _ = router_inputs(case)
    xin = router_norm_x(case, fp64=True) if case.form == "norm" else x
    logits = (xin.double() @ gate.double().T).float().to(BF).double()
    idx = router_select(logits, case.k)
    tw = logits.gather(1, idx)
    wt = torch.softmax(tw, dim=-1).float().to(BF).float()
    exact = (tw == tw[:, :1]).all(-1)            # k = 1, or a k-way tie: the weight is exactly bf16(1 / k)
    return idx, wt, exact


def router_emulate(case, mutant=None):
    x, gate, w, _ = router_inputs(case)
    xin = x if (case.form == "plain" or mutant == "norm_skipped") else router_norm_x(case, fp64=False)
    acc = (xin.double() @ gate.double().T).float()                       # exact sums: the fma chain's order does not enter
    logits = acc if mutant == "logit_not_rounded" else bf_round(acc)
    idx = router_select(logits, case.k, tie_highest=mutant == "tie_highest")
    tw = logits.gather(1, idx)
    ex = torch.exp(tw - tw[:, :1])
    den = ex.sum(-1, keepdim=True)
    if mutant == "softmax_all_E":
        den = torch.exp(logits - tw[:, :1]).sum(-1, keepdim=True)
    return idx, bf_round(ex / den)


def router_mutants_of(case):
    return ["norm_skipped"] if case.form == "norm" else list(ROUTER_MUTANTS)


def router_invisible(case, m):
    if m == "softmax_all_E" and case.k == case.E:
        return "k = E: the k picked are all the experts"
    if m == "tie_highest" and router_patterns(case) == ("distinct",):
        return "no two logits are equal"
    if m == "logit_not_rounded" and "round_tie" not in router_patterns(case):
        return "every chosen logit is a bf16 number: the rounding is the identity"
    return None


def router_mismatch(case, got, want):
    (idx, wt), (widx, wwt, exact) = got, want
    idx, wt = idx.cpu().long(), wt.cpu().float()
    d = first_diff(idx, widx)
    if d:
        return "indices: " + d
    if not bool(torch.isfinite(wt).all()):
        return "weights: not finite"
    ulp = 2.0 ** (torch.floor(torch.log2(wwt.clamp(min=2.0 ** -126))) - 7)
    tol = torch.where(exact[:, None], torch.zeros_like(ulp), ulp)
    bad = ((wt - wwt).abs() > tol).nonzero()
    if len(bad):
        t, j = (int(v) for v in bad[0])
        return f"weights: token {t} slot {j}: {float(wt[t, j])!r}, want {float(wwt[t, j])!r} ({'exactly' if bool(exact[t]) else 'within one bf16 ulp'})"
    return None


def router_conditions(case):
    x, gate, w, L = router_inputs(case)
    E, k, D, T, form = case
    xin = router_norm_x(case, True) if form == "norm" else x
    exact = (xin.double() @ gate.double().T)
    assert torch.equal(exact.float().double(), exact)                                # every logit is an fp32 number ...
    prod = xin.double()[:, None, :] * gate.double()[None]
    unit = 2.0 ** lsb_exponent(prod)                                                 # ... and so is every partial sum, in any order:
    assert float(prod.abs().sum(-1).max()) / unit < 2 ** 24                          # integers below 2^24 in units of the products' last bit
    idx, wt, ex = router_expected(case)
    if form == "plain":
        assert torch.equal(exact, L), case                                           # ... the chosen one
        lg = exact.float().to(BF).double()
        for t, pat in enumerate(router_patterns(case)):
            srt = torch.sort(lg[t], descending=True).values
            ties = [j for j in range(E - 1) if srt[j] == srt[j + 1]]
            want = {"tie_top": [0], "tie_cut": [k - 1] if k < E else [0], "all_equal": list(range(E - 1)), "round_tie": [0], "distinct": []}[pat]
            assert ties == want, (case, pat, ties)                                   # ties where they were placed, nowhere else
            if pat == "round_tie":
                assert exact[t, E - 1] > exact[t, 0] and lg[t, E - 1] == lg[t, 0] and idx[t, 0] == 0
            if pat == "all_equal":
                assert idx[t].tolist() == list(range(k)) and bool((wt[t] == float(torch.tensor(1.0 / k).to(BF))).all())
        if k == 1:
            assert bool((wt == 1.0).all()) and bool(ex.all())
    else:
        assert first_diff(router_norm_x(case, True), router_norm_x(case, False)) is None   # the fp64 and the fp32 norm chain agree
        xn = router_norm_x(case, True).double()
        assert all(len(set((xn[t] / w.double()).abs().tolist())) == 1 for t in range(T))      # one magnitude r_t per token
        full = xn @ gate.double().T
        assert torch.equal(full.float().double(), full)
    return {"exact-weight tokens": int(ex.sum())}


# ===================================================================================================================== kv_write
KV_HQ, KV_HKV, KV_DH = 2, 3, 16
KvCase = collections.namedtuple("KvCase", "W head_major")
KV_MUTANTS = ["le_window", "no_mod", "layouts_exchanged", "ld_ignored"]
KV_POISON_K, KV_POISON_V = -7.0, -9.0


def kv_cases():
    return [KvCase(W, hm) for W in (1, 7, 300) for hm in (False, True)]


@functools.lru_cache(maxsize=None)
def kv_inputs(case):
    """Chunks of W - 1, W, 0, W + 1 and 2 W + 1 tokens on sequences that have seen 0, W + 3 (a ring already wrapped), 5, W - 1 and
    2 W + 5 tokens.  k and v are column views of one fused [T, q | k | v] buffer; the eight elements of a piece spell
    (t mod 256, t div 256, head, piece, 1 for k | 2 for v, sequence, 0 .. ) - a row, a head or a piece taken from elsewhere shows."""
    W = case.W
    new = [W - 1, W, 0, W + 1, 2 * W + 1]
    seen = [0, W + 3, 5, W - 1, 2 * W + 5]
    T, kv = sum(new), KV_HKV * KV_DH
    tok_seq = torch.tensor([b for b, n in enumerate(new) for _ in range(n)], dtype=torch.int32)
    tok_pos = torch.tensor([seen[b] + i for b, n in enumerate(new) for i in range(n)], dtype=torch.int32)
    q_start = torch.tensor([0] + list(torch.tensor(new).cumsum(0)), dtype=torch.int32)
    fused = torch.full((T, KV_HQ * KV_DH + 2 * kv), 55.0)
    t = torch.arange(T)[:, None, None].float()
    h = torch.arange(KV_HKV)[None, :, None].float()
    p = torch.arange(KV_DH // 8)[None, None, :].float()
    for which in (1, 2):
        code = torch.stack(torch.broadcast_tensors(t % 256, t // 256, h, p, torch.tensor(float(which)), tok_seq[:, None, None].float(),
                                                   torch.tensor(0.0), t % 7), dim=-1)
        c0 = KV_HQ * KV_DH + (which - 1) * kv
        fused[:, c0:c0 + kv] = code.reshape(T, kv)
    return fused.to(BF), tok_seq, tok_pos, q_start, new


def kv_views(fused):
    q, kv = KV_HQ * KV_DH, KV_HKV * KV_DH
    return fused[:, q:q + kv], fused[:, q + kv:]


def kv_rings(case):
    shape = (5, case.W, KV_HKV, KV_DH)
    return torch.full(shape, KV_POISON_K, dtype=BF), torch.full(shape, KV_POISON_V, dtype=BF)


def kv_expected(case):
    """The rule of cache.py as a loop: token i of a chunk of s enters iff i >= s - W, at slot pos mod W of its sequence."""
    fused, tok_seq, tok_pos, q_start, new = kv_inputs(case)
    k, v = kv_views(fused)
    ck, cv = kv_rings(case)
    for t in range(fused.shape[0]):
        b = int(tok_seq[t])
        if t - int(q_start[b]) >= new[b] - case.W:
            ck[b, int(tok_pos[t]) % case.W] = k[t].view(KV_HKV, KV_DH)
            cv[b, int(tok_pos[t]) % case.W] = v[t].view(KV_HKV, KV_DH)
    return ck, cv


def kv_offsets(layout, W, seq, slot, c):
    kv = KV_HKV * KV_DH
    return ((seq * KV_HKV + c // KV_DH) * W + slot) * KV_DH + c % KV_DH if layout else (seq * W + slot) * kv + c


def kv_emulate(case, mutant=None):
    """kv_write_kernel on flat memory: one (token, piece) per thread, kv_offset() for the layout; returns logical [B, W, Hkv, Dh]."""
    fused, tok_seq, tok_pos, q_start, new = kv_inputs(case)
    W, kv, T = case.W, KV_HKV * KV_DH, fused.shape[0]
    layout = int(case.head_major) ^ (mutant == "layouts_exchanged")
    ld = kv if mutant == "ld_ignored" else fused.shape[1]
    src = fused.reshape(-1)
    t = torch.arange(T)[:, None]
    p = torch.arange(kv // 8)[None]
    b = tok_seq.long()[:, None]
    i, s = t - q_start.long()[b], (q_start.long()[b + 1] - q_start.long()[b])
    keep = (i > s - W) if mutant == "le_window" else (i >= s - W)
    slot = tok_pos.long()[:, None] if mutant == "no_mod" else tok_pos.long()[:, None] % W
    off = kv_offsets(layout, W, b, slot, p * 8)
    keep = (keep & (off + 8 <= 5 * W * kv)).expand(T, kv // 8)           # (a wrong slot may leave the ring: dropped here)
    e = torch.arange(8)
    dst = (off.expand(T, kv // 8)[keep][:, None] + e).reshape(-1)
    out = []
    for which, ring in enumerate(kv_rings(case)):
        base = KV_HQ * KV_DH + which * kv
        rd = (base + t * ld + p * 8).expand(T, kv // 8)[keep][:, None] + e
        phys = ring.permute(0, 2, 1, 3).contiguous() if case.head_major else ring.contiguous()
        flat = phys.reshape(-1)
        flat[dst] = src[rd.reshape(-1)]
        out.append(phys.permute(0, 2, 1, 3) if case.head_major else phys)
    return tuple(out)


def kv_mutants_of(case):
    return list(KV_MUTANTS)


def kv_invisible(case, m):
    if m == "layouts_exchanged" and case.W == 1:
        return "one slot: both layouts put (sequence, head, d) at the same offset"
    return None


def kv_mismatch(case, got, want):
    for name, g, w in zip("kv", got, want):
        d = first_diff(g.cpu(), w)
        if d:
            return f"{name} ring [sequence, slot, head, d]: {d}"
    return None


def kv_conditions(case):
    fused, tok_seq, tok_pos, q_start, new = kv_inputs(case)
    W = case.W
    assert torch.equal(fused.float().round(), fused.float()) and float(fused.max()) <= 256
    assert new[2] == 0 and int(q_start[2]) == int(q_start[3]) and {n - W for n in new if n} == {d for d in (-1, 0, 1, W + 1) if d + W}
    k, v = kv_views(fused)
    assert k.stride(0) == v.stride(0) == fused.shape[1] > KV_HKV * KV_DH
    pieces = torch.cat((k, v), 1).reshape(-1, 8)
    assert len(torch.unique(pieces, dim=0)) == len(pieces)                    # every piece names its place
    if W == 1:
        assert all(kv_offsets(0, 1, b, 0, c) == kv_offsets(1, 1, b, 0, c) for b in range(5) for c in range(0, KV_HKV * KV_DH, 8))
    ck, _ = kv_expected(case)
    return {"slots left poisoned": int((ck[:, :, 0, 0] == KV_POISON_K).sum()), "tokens": fused.shape[0]}


# ===================================================================================================================== logprobs
# mi_lm_head_logprobs: M < 256 -> fp32 logits + logprob_rows_kernel; M >= 256 (K % 64 == 0) -> per-256-column-tile (max, sum exp)
# partials from the GEMM epilogue + logprob_finalize_kernel.  target -1: the row returns -logsumexp.
LOGPROB_TOL = 2e-4
LOGPROB_K = 128
LogprobCase = collections.namedtuple("LogprobCase", "V M variant")
LOGPROB_MUTANTS = ["last_tile_dropped", "ignored_reads_last", "target_row_above"]


def logprob_cases():
    return [LogprobCase(V, M, var) for V in (1000, 4096) for M, var in ((3, "a"), (3, "b"), (256, "a"))]


@functools.lru_cache(maxsize=None)
def logprob_inputs(case):
    """(x bf16 [M, K] one-hot, w bf16 [V, K] integer-coded quarters, targets int32 [M]): logit[m, v] = w[v, j_m], exactly.
    Row 1 of variant a has one dominant logit (60 against |.| <= 4) in the last tile - the ragged one at V = 1000."""
    V, M, var = case
    K = LOGPROB_K
    j = (torch.arange(M) * 5 + 3) % K
    x = torch.zeros(M, K)
    x[torch.arange(M), j] = 1.0
    v = torch.arange(V)[:, None]
    w = (((v * 7 + torch.arange(K)[None] * 13) % 33) - 16).float() / 4
    cyc = [0, V - 3, 255, 256, V - 1, -1]
    if M == 3:
        tgt = cyc[:3] if var == "a" else cyc[3:]
    else:
        tgt = [cyc[m % 6] if m < 12 else (m * 37) % V for m in range(M)]
    if var == "a":
        w[V - 3, int(j[1])] = 60.0
    return x.to(BF), w.to(BF), torch.tensor(tgt, dtype=torch.int32)


def logprob_logits(case):
    x, w, _ = logprob_inputs(case)
    return x.double() @ w.double().T


def logprob_expected(case):
    _, _, tgt = logprob_inputs(case)
    lg = logprob_logits(case)
    lse = torch.logsumexp(lg, dim=-1)
    at = lg.gather(1, tgt.clamp(min=0).long()[:, None])[:, 0]
    return torch.where(tgt >= 0, at, torch.zeros_like(at)) - lse


def logprob_emulate(case, mutant=None):
    """Per-tile (max, sum exp) partials of 256 columns and their merge, as the fused route keeps them; the row route is one tile."""
    _, _, tgt = logprob_inputs(case)
    lg = logprob_logits(case)
    V, M = case.V, case.M
    tile = 256 if M >= 256 else V
    n_tiles = (V + tile - 1) // tile - (1 if mutant == "last_tile_dropped" and V > tile else 0)
    parts = [lg[:, j * tile:min((j + 1) * tile, V)] for j in range(n_tiles)]
    pm = torch.stack([p.max(-1).values for p in parts], -1)
    ps = torch.stack([torch.exp(p - p.max(-1, keepdim=True).values).sum(-1) for p in parts], -1)
    Mx = pm.max(-1).values
    lse = Mx + torch.log((ps * torch.exp(pm - Mx[:, None])).sum(-1))
    rows = (torch.arange(M) + 1) % M if mutant == "target_row_above" else torch.arange(M)
    at = lg[rows, tgt.clamp(min=0).long()]
    if mutant == "ignored_reads_last":
        at = torch.where(tgt >= 0, at, lg[:, V - 1])
    else:
        at = torch.where(tgt >= 0, at, torch.zeros_like(at))
    return at - lse


def logprob_mutants_of(case):
    _, _, tgt = logprob_inputs(case)
    return [m for m in LOGPROB_MUTANTS if (m != "ignored_reads_last" or int(tgt.min()) < 0) and (m != "last_tile_dropped" or case.M >= 256)]


def logprob_invisible(case, m):
    return None


def logprob_mismatch(case, got, want):
    got = got.cpu().double()
    err = (got - want).abs()
    bad = (~torch.isfinite(got) | ~(err <= LOGPROB_TOL)).nonzero()
    if len(bad):
        m = int(bad[0])
        return f"row {m}: {float(got[m])!r}, want {float(want[m])!r} ({len(bad)} rows, worst {float(err.max()):.3g})"
    return None


def logprob_conditions(case):
    x, w, tgt = logprob_inputs(case)
    lg = logprob_logits(case)
    assert torch.equal(lg.float().to(BF).double(), lg)                        # the logits are bf16 numbers: the LM head's rounding is the identity
    V = case.V
    if case.M == 256:
        assert {0, 255, 256, V - 1, -1, V - 3} <= set(tgt.tolist())
    if case.variant == "a":
        assert float(lg[1, V - 3]) == 60.0 and float(lg[1].topk(2).values[1]) <= 4 and (V - 3) // 256 == (V - 1) // 256
    return {"worst |logprob|": float(logprob_expected(case).abs().max())}


# ======================================================================================================================== table
def _group(prefix):
    g = globals()
    return types.SimpleNamespace(**{n: g[f"{prefix}_{n}"] for n in ("cases", "inputs", "expected", "emulate", "mutants_of", "invisible",
                                                                    "mismatch", "conditions")})


GROUPS = collections.OrderedDict((name, _group(name)) for name in ("greedy", "rms", "rope", "router", "kv", "logprob"))
