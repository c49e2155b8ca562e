"""Shared by tests/test_spec_sampling_host.py and tests/test_gpu_spec_sampling.py: the float64 restatement of the sampled
verification rule of include/mistral_hip.h (`mi_verify_sample`), the logits rows and drafts both files test it on, and the
variate grids; no test functions here.

The distribution P of a row is `mistral_oracle.top_p_distribution`'s (descending probability, ties by ascending id - a stable
sort - kept = the prefix whose mass before the token is <= p, renormalised) with the cut taken where the EXACT float64
mass-before exceeds p, as tests/test_gpu_sampling.py::_exact_distribution takes it: the kernel's 40-bit fixed-point masses sit on
the exact side, the oracle's fp32 cumsum up to a token or two away in a wide nucleus (`oracle_kept` is there to compare)."""
import functools
import os
import sys

import torch

import mistral_oracle as mo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from make_golden_sampling_cases import sampling_cases  # noqa: E402

NEAR = 2e-6   # a variate this close to a decision point (or within a quarter of the step) is not counted


class Nucleus:
    """One logits row under (temperature, top_p): `order` (token ids, descending probability, ties by ascending id), `mass`
    (float64, by sorted position: softmax(row / t) inside the kept prefix, 0 behind the cut), `lsm` = log_softmax of the
    UNSCALED row.  top_p is rounded to fp32 first, which is what the library receives."""

    def __init__(self, row: torch.Tensor, t: float, p: float):
        row = row.detach().cpu().float()
        p = float(torch.tensor(p, dtype=torch.float32))
        self.V = row.numel()
        probs = torch.softmax(row.double() / t, dim=-1)
        ps, self.order = torch.sort(probs, descending=True, stable=True)
        before = torch.cumsum(ps, 0) - ps
        self.mass = ps.masked_fill(before > p, 0.0)
        self.pos_of = torch.empty(self.V, dtype=torch.long)
        self.pos_of[self.order] = torch.arange(self.V)
        self.lsm = torch.log_softmax(row.double(), dim=-1)
        self.oracle_kept = int((mo.top_p_distribution(row, t, p)[1] > 0).sum())
        self._cdf = {}

    # ---- distributions over token ids, dense [V]
    def P(self) -> torch.Tensor:
        return torch.zeros(self.V, dtype=torch.float64).scatter_(0, self.order, self.mass / self.mass.sum())

    def prob(self, d: int) -> float:
        """P(d): 0 for a token outside the kept set, also one tied at the cut value that the ascending-id rule leaves out."""
        return float(self.mass[self.pos_of[d]] / self.mass.sum())

    def residual(self, d: int) -> torch.Tensor:
        """P with d removed and renormalised (defined when P(d) < 1)."""
        m = self._without(d)
        return torch.zeros(self.V, dtype=torch.float64).scatter_(0, self.order, m / m.sum())

    def _without(self, d) -> torch.Tensor:
        m = self.mass.clone()
        if d is not None:
            m[self.pos_of[d]] = 0.0
        return m

    # ---- the inverse CDF in the kept order, d's mass taken out of the running sums (d None: the plain draw)
    def draw(self, d, u: float):
        """(token, near): the first sorted position whose cumulative mass exceeds u; near = u within min(NEAR, step / 4) of
        one of the two CDF values that bound that position."""
        if d not in self._cdf:
            m = self._without(d)
            self._cdf[d] = (torch.cumsum(m, 0) / m.sum(), int((m > 0).nonzero()[-1]), m / m.sum())
        cdf, last, m = self._cdf[d]
        pos = min(int(torch.searchsorted(cdf, torch.tensor(u, dtype=torch.float64), right=True)), last)
        tol = min(NEAR, 0.25 * float(m[pos]))
        near = abs(float(cdf[pos]) - u) < tol or (pos > 0 and abs(u - float(cdf[pos - 1])) < tol)
        return int(self.order[pos]), near

    def decide(self, d: int, u_acc: float, u_draw: float):
        """A drafted row: (accepted, token, near).  Accept iff u_acc < P(d); else the draw from P without d."""
        pd = self.prob(d)
        near = 0.0 < pd < 1.0 and abs(u_acc - pd) < min(NEAR, 0.25 * pd)
        if u_acc < pd:
            return True, d, near
        tok, near_draw = self.draw(d, u_draw)
        return False, tok, near or near_draw


def verify_sample_reference(logits, ids, q_start, t, p, u):
    """The rule on T rows in B sequences.  logits: fp32 [T, V], or a list of T `Nucleus` objects (rows that repeat share one);
    ids [T]; q_start [B + 1]; u [T][2] = (u_acc, u_draw).  Returns (tokens [T] long, logprobs [T] float64, n_accept list [B],
    near [T] bool): rows behind a sequence's first rejection hold (-1, 0); near[i] marks a row whose variate sat within the
    tolerance of a decision point - what follows it in its sequence is not to be counted."""
    ids = [int(x) for x in (ids.tolist() if torch.is_tensor(ids) else ids)]
    q_start = [int(x) for x in (q_start.tolist() if torch.is_tensor(q_start) else q_start)]
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1, 2).tolist()
    T = len(ids)
    rows = logits if isinstance(logits, (list, tuple)) else [Nucleus(logits[i], t, p) for i in range(T)]
    tokens = torch.full((T,), -1, dtype=torch.long)
    logprobs = torch.zeros(T, dtype=torch.float64)
    near = torch.zeros(T, dtype=torch.bool)
    n_accept = []
    for b in range(len(q_start) - 1):
        q0, m = q_start[b], q_start[b + 1] - q_start[b]
        a = 0
        for i in range(m):
            r, row = q0 + i, rows[q0 + i]
            if i + 1 < m:
                ok, tok, nr = row.decide(ids[r + 1], u[r][0], u[r][1])
            else:
                ok = False
                tok, nr = row.draw(None, u[r][1])
            tokens[r], logprobs[r], near[r] = tok, row.lsm[tok], nr
            if not ok:
                break
            a += 1
        n_accept.append(a)
    return tokens, logprobs, n_accept, near


def counted_sequences(q_start, near):
    """bool [B]: the sequences none of whose rows sat near a decision point."""
    return torch.tensor([not bool(near[q_start[b]: q_start[b + 1]].any()) for b in range(len(q_start) - 1)])


# ------------------------------------------------------------------------------------------------ the rows of the GPU test
@functools.lru_cache(maxsize=None)
def gpu_rows():
    """name -> (row fp32 [V], temperature, top_p).  The big rows are tests/test_gpu_sampling.py's, regenerated from its seed."""
    g = torch.Generator().manual_seed(99)
    torch.randn(32768, generator=g), torch.randn(32000, generator=g)   # (its two rows before these: the stream stays in step)
    peaked131072 = (torch.randn(131072, generator=g) * 3.0).to(torch.bfloat16).float()
    cold = torch.randn(32773, generator=g) * 2.0
    neg_inf = torch.cat([torch.randn(100, generator=g), torch.full((32668,), -float("inf"))])
    tiny = (torch.randn(512, generator=torch.Generator().manual_seed(512)) * 2.0).to(torch.bfloat16).float()
    tiny[[7, 300]] = float(tiny[40])  # (three tokens share one value: ties inside a 512-wide row, the tiny model's vocabulary)
    return {
        "flat_t0.7_p0.8": sampling_cases()["flat_t0.7_p0.8"],
        "v4099_all_equal": (torch.full((4099,), -1.25), 0.7, 0.8),
        "v32773_fp32_cold": (cold, 0.05, 0.8),
        "v32768_neg_inf": (neg_inf, 0.7, 0.8),
        "v131072_peaked_bf16": (peaked131072, 1.0, 0.8),
        "v512_tiny_vocab": (tiny, 0.7, 0.8),
    }


def drafts_for(nuc: Nucleus, row: torch.Tensor):
    """kind -> draft id, for the kinds the row has: the mode, a mid-nucleus token, the last kept token, the first token outside,
    a kept and an unkept token tied at the cut value, a -inf token."""
    n = int((nuc.mass > 0).sum())
    out = {"mode": int(nuc.order[0]), "last_kept": int(nuc.order[n - 1])}
    if n >= 3:
        out["mid"] = int(nuc.order[n // 2])
    if n < nuc.V:
        out["first_outside"] = int(nuc.order[n])
        cut_value = row[nuc.order[n - 1]]
        tied = (row == cut_value).nonzero()[:, 0]
        kept_ties = [int(i) for i in tied if nuc.pos_of[i] < n]
        left_out = [int(i) for i in tied if nuc.pos_of[i] >= n]
        if left_out:
            out["tied_kept"], out["tied_left_out"] = kept_ties[-1], left_out[0]
    inf = (row == -float("inf")).nonzero()[:, 0]
    if inf.numel():
        out["neg_inf"] = int(inf[0])
    return out


def variate_grid(n: int, seed: int) -> torch.Tensor:
    """fp32 [n, 2] = (u_acc, u_draw) in [0, 1): the corners first, then a seeded uniform grid.  fp32-valued, so the library and the
    float64 rule see the same numbers."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 2, generator=g).float()
    edge = torch.tensor([[0.0, 0.0], [0.999999, 0.999999], [1e-7, 0.5]])
    k = min(n, edge.shape[0])
    u[:k] = edge[:k]
    return u


def n_variates(name: str) -> int:
    """Variate pairs per draft kind: fewer on the 131072-wide row (every row of a launch is a copy of it)."""
    return 48 if gpu_rows()[name][0].numel() > 100000 else 64


def two_row_problem(name: str, n_u: int):
    """The leaf problem of one row: for every draft kind and n_u variate pairs, the two-row sequence [any token, draft] on two
    copies of the row - row 0 decides about the draft, row 1 (reached when it is accepted) takes the plain draw.
    Returns (row, t, p, nuclei list [T], ids [T], q_start [B + 1], u [T, 2], kinds list [B])."""
    row, t, p = gpu_rows()[name]
    nuc = Nucleus(row, t, p)
    drafts = drafts_for(nuc, row)
    ids, kinds, u = [], [], []
    for j, (kind, d) in enumerate(drafts.items()):
        ids += [0, d] * n_u
        kinds += [kind] * n_u
        first, second = variate_grid(n_u, seed=1000 + j), variate_grid(n_u, seed=2000 + j)
        u.append(torch.stack([first, second], 1).reshape(2 * n_u, 2))   # (every kind meets the corners)
    T = len(ids)
    return row, t, p, [nuc] * T, torch.tensor(ids), list(range(0, T + 1, 2)), torch.cat(u), kinds


SPLITS = {"B1": [0, 8], "B2": [0, 3, 8], "B3": [0, 2, 3, 8]}


@functools.lru_cache(maxsize=None)
def eight_row_launches(split: str):
    """Launches of T = 8 rows as the sequences of SPLITS[split]: (rows [2], nuclei [2], t, p, launches) with launches = a list of
    (which [8] - the logits row of every step row -, ids [8], u fp32 [8, 2]).  Two different 512-wide rows alternate; drafts come
    from every kind of either row (each third launch: the mode of its row); about 60 % of the drafted rows with a draft of
    positive mass get a variate inside their accept interval - all of them in the first launch - so the scans run deep."""
    q_start = SPLITS[split]
    row, t, p = gpu_rows()["v512_tiny_vocab"]
    rows = [row, row.roll(37)]
    nucs = [Nucleus(r, t, p) for r in rows]
    pool = [d for n, r in zip(nucs, rows) for d in drafts_for(n, r).values()]
    g = torch.Generator().manual_seed(len(q_start))
    launches = []
    for launch in range(24):
        which = [(i + launch) % 2 for i in range(8)]
        ids = [pool[int(torch.randint(0, len(pool), (1,), generator=g))] for _ in range(8)]
        if launch % 3 == 0:
            ids = [int(nucs[which[i - 1]].order[0]) if i else 0 for i in range(8)]
        u = torch.rand(8, 2, generator=g).float()
        for i in range(7):
            pd = nucs[which[i]].prob(ids[i + 1])
            if i + 1 not in q_start and pd > 0 and (launch == 0 or float(torch.rand(1, generator=g)) < 0.6):
                u[i, 0] = 0.5 * pd
        launches.append((which, ids, u))
    return rows, nucs, t, p, launches


@functools.lru_cache(maxsize=None)
def frequency_problem():
    """(row, t, p, d): the 512-wide row with token d = 11 lifted until P(d) is 0.3 to within 1e-3 (bisection on its logit)."""
    row, t, p = gpu_rows()["v512_tiny_vocab"]
    d, lo, hi = 11, -10.0, 20.0
    for _ in range(40):
        row = row.clone()
        row[d] = 0.5 * (lo + hi)
        lo, hi = (float(row[d]), hi) if Nucleus(row, t, p).prob(d) < 0.3 else (lo, float(row[d]))
    assert abs(Nucleus(row, t, p).prob(d) - 0.3) < 1e-3
    return row, t, p, d
