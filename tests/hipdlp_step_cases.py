"""The Halpern step of solver="hipdlp" on the problems of tests/edge_cases.py, which sit exactly on the structural thresholds
where the SpMV launches change path: the cases, what the planners must make of them, and planted starts whose step is exact
in any summation order.  For tests/test_hipdlp_step_host.py and tests/test_gpu_hipdlp_step.py.  Fixed seeds, nothing read from
disk, no GPU; of the product only solver.stream_plan, the host-only hook of the planners (the work blocks decide which majors
a plan speaks about).

The restatement of the step is hipdlp_check_cases.halpern_step (performHalpernPdhgStep, hipdlp/pdhg.cc:961-1018 of the
reference implementation, elementwise on whole vectors), unchanged.

HiPDLP's formulation turns every `<=` row of an edge case into a `>=` row (rl finite, ru = inf): it negates the row's integer
coefficients, keeps the pattern, adds no slack column and reorders no row (n_eqs == 0).  The tests plant cost, column bounds
and row bounds of their own on that matrix."""
from collections import namedtuple

import numpy as np

import edge_cases as E
import hipdlp_check_cases as H
from highs_amd import solver

INF = H.INF
LONG = 256  # a major of more than 256 entries is long in the slab layout, and in every layout beyond its chunk
TAU = 0.25

# name -> (maker(values), layouts).  The many_long cases: slab layout only, as in test_gpu_edges.SPMV_CASES (the stream
# layout reaches the cap of contribution slots at 4.2 M nonzeros only).
CASES = {
    "limit512": (lambda v: E.majors_at_limit(512, v), ("csr", "slab")),
    "limit2048": (lambda v: E.majors_at_limit(2048, v), ("csr", "slab")),
    "segments": (E.segments, ("csr", "slab")),
    "empty_runs": (E.empty_runs, ("csr", "slab")),
    "empty_runs4600": (lambda v: E.empty_runs(v, long_row=4600), ("csr", "slab")),
    "grid32": (lambda v: E.grid(32, v), ("csr", "slab")),
    "grid33": (lambda v: E.grid(33, v), ("csr", "slab")),
    "grid64": (lambda v: E.grid(64, v), ("csr", "slab")),
    "grid65": (lambda v: E.grid(65, v), ("csr", "slab")),
    "wide10000": (lambda v: E.wide(10000, v), ("csr", "slab")),
    "wide16385": (lambda v: E.wide(16385, v), ("csr", "slab")),
    "long2048": (lambda v: E.many_long(2048, v), ("slab",)),
    "long2049": (lambda v: E.many_long(2049, v), ("slab",)),
}
PARAMS = [(name, layout) for name, (_, layouts) in CASES.items() for layout in layouts]
PERSISTENT_CASES = ("empty_runs", "empty_runs4600", "grid32", "grid33", "grid64", "wide10000", "wide16385")

# What the planners make of each case in the oracle's form (asserted in tests/test_hipdlp_step_host.py; the GPU test asserts
# the same numbers on what the device built):
#   chunk            the stream layout's chunk
#   a, at            stream layout of A and of A': (work blocks, long majors, segment tasks)
#   slab             long majors of A and of A' in the slab layout (limit 256)
#   group            long majors per contribution slot of A in the slab layout
#   rule             pdlp_halpern_small.hpp halpernSmallReason / Grid / Mode on the stream layout: (reason, grid, mode), or the
#                    reason alone where the solver keeps the plain launches (5: a chunk that is not 512, 6: a long major, 7: more
#                    than 64 work blocks)
Expect = namedtuple("Expect", "chunk a at slab group rule")
EXPECT = {
    "limit512": Expect(512, (11, 1, 2), (9, 1, 2), (4, 3), 1, 6),
    "limit2048": Expect(2048, (130, 1, 5), (131, 1, 5), (4, 3), 1, 5),
    "segments": Expect(512, (2, 7, 118), (142, 0, 0), (7, 0), 1, 6),
    "empty_runs": Expect(512, (4, 0, 0), (4, 0, 0), (1, 0), 1, (0, 4, 1)),
    "empty_runs4600": Expect(512, (4, 0, 0), (4, 0, 0), (1, 0), 1, (0, 4, 1)),
    "grid32": Expect(512, (32, 0, 0), (32, 0, 0), (32, 0), 1, (0, 32, 1)),
    "grid33": Expect(512, (33, 0, 0), (33, 0, 0), (33, 0), 1, (0, 33, 0)),
    "grid64": Expect(512, (64, 0, 0), (64, 0, 0), (64, 0), 1, (0, 64, 0)),
    "grid65": Expect(512, (65, 0, 0), (65, 0, 0), (65, 0), 1, 7),
    "wide10000": Expect(512, (4, 0, 0), (8, 0, 0), (4, 0), 1, (0, 8, 1)),
    "wide16385": Expect(512, (4, 0, 0), (11, 0, 0), (4, 0), 1, (0, 11, 1)),
    "long2048": Expect(2048, (293, 0, 0), (266, 0, 0), (2048, 0), 1, 5),
    "long2049": Expect(2048, (293, 0, 0), (266, 0, 0), (2049, 0), 2, 5),
}
# stream layout: (blocks of exactly 2048 majors, blocks without entries) of A and of A', where a case has any
CAPPED = {
    "empty_runs": ((2, 0), (2, 1)),
    "empty_runs4600": ((2, 1), (2, 1)),
    "wide10000": ((0, 0), (4, 4)),
    "wide16385": ((0, 0), (7, 7)),
}

_lps, _forms, _plans = {}, {}, {}


def case_lp(name, values):
    if (name, values) not in _lps:
        _lps[(name, values)] = CASES[name][0](values)
    return _lps[(name, values)]


def formulated(name, values="integer"):
    """hipdlp_check_cases.formulated_lp of a case: the oracle's own formulation (integer: no scaling; real: scaled).  Made once."""
    if (name, values) not in _forms:
        _forms[(name, values)] = H.formulated_lp(case_lp(name, values), values)
    return _forms[(name, values)]


def plan_form(F):
    """The oracle's form as the dict solver.stream_plan takes (both compressed orders; the planner sizes the blocks itself)."""
    csc = F.A.tocsc()
    csc.sort_indices()
    csr = F.A.tocsr()
    csr.sort_indices()
    return dict(n=F.n, m=F.m, nnz=csc.nnz, spmv_blocks_ax=0, spmv_blocks_aty=0, csr_beg=csr.indptr, csr_idx=csr.indices,
                csr_val=csr.data, csc_beg=csc.indptr, csc_idx=csc.indices, csc_val=csc.data)


def plans(name):
    """(stream plan of A, of A', slab-layout long majors of A, of A') of the integer form of a case.  Made once."""
    if name not in _plans:
        P = plan_form(formulated(name))
        _plans[name] = tuple(solver.stream_plan(P, w, lim) for lim in (0, LONG) for w in (0, 1))
    return _plans[name]


def rule_shape(name):
    """The fields of pdlp_halpern_small.hpp HalpernSmallShape that the stream layout of a case decides."""
    a, at = plans(name)[:2]
    return dict(blocks_a=a["n_blocks"], blocks_at=at["n_blocks"], chunk_a=a["chunk"], chunk_at=at["chunk"], use_slab=0,
                long_tasks=a["n_tasks"] + at["n_tasks"], long_contrib=1 if max(a["long_group"], at["long_group"]) > 1 else 0)


# ---- the majors a plan speaks about -------------------------------------------------------------------------------------------
def marked(name):
    """(row mask, column mask): the majors whose clamp class the two plans control.  Every major of more than 256 entries; the
    first and the last major of every work block of the stream layout; every major of a work block without entries."""
    F = formulated(name)
    a, at = plans(name)[:2]
    out = []
    for M, plan in ((F.A.tocsr(), a), (F.A.tocsc(), at)):
        mask = np.diff(M.indptr) > LONG
        for b0, b1, e0, e1 in plan["blocks"]:
            mask[b0] = mask[b1 - 1] = True
            if e0 == e1:
                mask[b0:b1] = True
        out.append(mask)
    return tuple(out)


# ---- planted starts -----------------------------------------------------------------------------------------------------------
PLANS = ("free", "clamped")


def _column_bounds(F, rng):
    """Five kinds by j % 5 (free, lower, upper, boxed, fixed) on the integer grid, then hipdlp_check_cases.plan's -0.0 bounds in
    every seventh group of five."""
    j = np.arange(F.n)
    lo0 = rng.integers(-4, 1, F.n).astype(np.float64)
    up0 = lo0 + rng.integers(1, 5, F.n)
    kind = j % 5
    lo = np.where((kind == 1) | (kind == 3) | (kind == 4), lo0, -INF)
    up = np.where((kind == 2) | (kind == 3), up0, np.where(kind == 4, lo0, INF))
    v = H.plan(F, "integer", rng, lower=lo, upper=up)
    return v["lower"], v["upper"]


def step_data(name, plan_name, rng, sigma=2.0, dyadic_anchors=True):
    """The vectors of one start of the integer form of a case, as hipdlp_check_cases.halpern_step takes them: x, y, x_anchor,
    y_anchor, cost, lower, upper, rhs, row_upper.  From hipdlp_check_cases.step_plan (y integer, x and the cost on the grid of
    1/4, every eleventh bounded column with temp = x - tau (c - A'y) exactly on its bound), with
      cost     rint(4 c) / 4 of the problem's real cost, zeros replaced by 1/4
      rows     kinds by i % 3: rl finite and ru = inf; rl == ru; ranged (rl < ru finite), on the integer grid.  Every eleventh row
               has temp_y = y / sigma - A x_reflected exactly on -rl, every eleventh ranged row on -ru: y enters temp_y through
               both products (A'y moves x_reflected), so the BOUND is moved onto temp_y, not y onto the bound
      marked   (marked(name)) majors: plan "free" puts every one strictly inside its bounds (columns boxed [-2, 3] with
               temp = -3/2; rows ranged with rl < -temp_y < ru); plan "clamped" puts them below, above and exactly on a finite bound
               in turn (the first marked major of either side exactly on it).
    tau = 1/4 throughout; sigma is the dual step the row plan is made for."""
    assert plan_name in PLANS
    F = formulated(name)
    assert np.array_equal(F.A.data, np.rint(F.A.data))
    rows, cols = marked(name)
    cost = np.rint(4.0 * F.cost) / 4.0
    cost[cost == 0.0] = 0.25
    lower, upper = _column_bounds(F, rng)
    nc = int(cols.sum())
    lower[cols], upper[cols] = -2.0, 3.0
    d = H.step_plan(F._replace(cost=cost), lower, upper, rng, dyadic_anchors)
    red = TAU * (cost - F.A.T @ d["y"])
    turn = np.arange(nc) % 3
    target = np.full(nc, -1.5) if plan_name == "free" else np.where(turn == 0, -2.0, np.where(turn == 1, -3.25, 4.5))
    d["x"][cols] = target + red[cols]
    # the column side of the step, restated: what the row side will be given
    temp = d["x"] - TAU * (cost - F.A.T @ d["y"])
    proj = H._std_max(lower, H._std_min(temp, upper))
    temp_y = d["y"] / sigma - F.A @ (2.0 * proj - d["x"])
    i = np.arange(F.m)
    kind = i % 3
    rl = rng.integers(-8, 9, F.m).astype(np.float64)
    width = rng.integers(1, 5, F.m).astype(np.float64)
    on_l = i % 11 == 0
    on_u = (kind == 2) & ((i // 3) % 11 == 5) & ~on_l
    rl = np.where(on_l, -temp_y, np.where(on_u, -temp_y - width, rl))
    ru = np.where(kind == 0, INF, np.where(kind == 1, rl, np.where(on_u, -temp_y, rl + width)))
    base = np.floor(-temp_y[rows])
    turn = np.arange(int(rows.sum())) % 3
    if plan_name == "free":
        rl[rows], ru[rows] = base - 1.0, base + 2.0
    else:  # on -rl; above -rl (clamped to it); below -ru
        rl[rows] = np.where(turn == 0, -temp_y[rows], np.where(turn == 1, base + 2.0, base - 6.0))
        ru[rows] = np.where(turn == 0, rl[rows] + 3.0, np.where(turn == 1, INF, base - 2.0))
    assert np.all(rl <= ru) and np.all(np.isfinite(rl))
    d["rhs"], d["row_upper"] = rl, ru
    return d


def row_temp(A, y_before, x_reflected, sigma):
    """temp_y of the step that turned y_before into what it is now (pdhg.cc:995-1000), from the restatement's own vectors."""
    return y_before / sigma - A @ x_reflected


def classes(temp, lo, up):
    """-1 clamped below its bound, -2 exactly on its lower end, 0 strictly inside, 2 exactly on its upper end, 1 beyond."""
    return np.where(temp < lo, -1, np.where(temp == lo, -2, np.where(temp == up, 2, np.where(temp > up, 1, 0))))


# ---- exactness ----------------------------------------------------------------------------------------------------------------
def grid_of(v):
    """The largest power of two (at most 1) that every element of v is a multiple of."""
    g = 1.0
    while not np.array_equal(v / g, np.rint(v / g)):
        g *= 0.5
        assert g >= 2.0**-40, "not on a dyadic grid of 2^-40 or coarser"
    return g


def exact_units(A, v):
    """(g, u): the grid g of the operand v, and max over the majors of A of sum |a_i v_i| in units of g.  With integer
    coefficients every product and every partial sum of A v, in any order, is a multiple of g of at most u units: exact in
    float64 while u < 2^53."""
    g = grid_of(v)
    assert np.array_equal(A.data, np.rint(A.data))
    u = float((abs(A) @ np.abs(v / g)).max()) if A.nnz else 0.0
    return g, u


def restate(name, d, steps, sigma, h_iter):
    """`steps` major steps of halpern_step from the start d (not changed): -> (vectors after, per step a dict with the four
    operand checks' inputs and the clamp classes): step["aty_operand"], ["ax_operand"], ["col_class"], ["row_class"]."""
    F = formulated(name)
    want = {k: a.copy() for k, a in d.items()}
    trace = []
    for i in range(1, steps + 1):
        y_before = want["y"].copy()
        temp = H.halpern_step(F.A, want, TAU, sigma, h_iter, i, True)
        temp_y = row_temp(F.A, y_before, want["x_reflected"], sigma)
        trace.append(dict(aty_operand=y_before, ax_operand=want["x_reflected"].copy(), temp=temp, temp_y=temp_y,
                          col_class=classes(temp, d["lower"], d["upper"]), row_class=classes(temp_y, -d["row_upper"], -d["rhs"])))
    return want, trace
