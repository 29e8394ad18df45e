"""The kernels on problems that sit exactly on the structural thresholds where they change path (tests/edge_cases.py; the
structural claims themselves are proven on the host planners in tests/test_edge_cases_host.py).

1. A x and A' y against references that depend on no summation order, so that a placement rule mirrored wrongly in the
   oracle's device-order model cannot hide a mistake:
   - integer data (coefficients in [-8, 8], vector in [-1024, 1024], no scaling): every product and partial sum is an exact
     double, the kernel must return the integer result computed in int64 — `==`;
   - real data: bit for bit against the left-to-right oracle on majors up to the limit and against the device-order model
     on all majors, and against the exact sum (edge_cases.exact_major_sums) within the bound that holds for ANY order.
     Derivation: a major of k entries is summed as k rounded products and k - 1 rounded additions in some order; every
     intermediate carries at most k roundings of relative size u = 2^-53, so |computed - exact| <= gamma_k sum|a_i x_i| with
     gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, section 4.2, any ordering).  The reference itself is the exact
     sum rounded once: another u |exact| <= u sum|a_i x_i|.  Together (k + 1) u sum|a_i x_i| up to the factor 1 / (1 - k u),
     which (1 + 1e-6) covers for k < 10^9, as it covers the rounding of sum|a_i x_i| itself.  Nothing is measured.
2. One trial step (x+, y+, the epilogues, the three reductions) with test_gpu_parity._trial_step_check at these shapes.
3. Whole solves, the persistent loop, the one-launch check and the batch lanes at grids of 32 / 33 and 64 / 65 workgroups, with
   more column-step workgroups than blocks, with runs of empty majors and on the small QP whose N fills a block exactly:
   bit for bit against the oracle's device-order mode, and switch against switch.

Oracle alone, device-order mode, kkt_tolerance 1e-7, capped (edge_cases.SOLVES) — iterations / trials / restarts, each with a
rejected trial (trials > iterations) and a restart inside the cap (asserted below and, without a GPU, in
test_edge_cases_host.py):
  grid32 400 / 403 / 11     grid33 760 / 764 / 11     grid64 560 / 561 / 10     grid65 640 / 645 / 11
  wide10000 999 / 1053 / 11 wide16384 520 / 549 / 12  wide16385 600 / 628 / 12
  empty_runs 80 / 82 / 7    arrow512 120 / 127 / 6    arrow513 120 / 125 / 6
  empty_runs4600 120 / 123 / 8 (a block of A without entries)   arrow512n4200 200 / 211 / 8 (blocks of N without entries)
Every comparison is `==` / array_equal, except the derived summation bound of 1 and what _trial_step_check holds."""
import numpy as np
import pytest

import edge_cases as E
import oraclelib as O
import update_cases as UC
from highs_amd import solver
from test_gpu_parity import _spmv, _trial_step_check
from test_gpu_qp_small import _assert_equals_oracle, _assert_same_result

pytestmark = pytest.mark.gpu

# name -> (maker(values), layouts)
SPMV_CASES = {
    "limit512": (lambda v: E.majors_at_limit(512, v), ("csr", "slab")),
    "limit2048": (lambda v: E.majors_at_limit(2048, v), ("csr", "slab")),
    "segments": (E.segments, ("csr", "slab")),
    "long2048": (lambda v: E.many_long(2048, v), ("slab",)),  # (the cap of contribution slots: slab layout only)
    "long2049": (lambda v: E.many_long(2049, v), ("slab",)),
    "empty_runs": (E.empty_runs, ("csr", "slab")),
    "empty_runs4600": (lambda v: E.empty_runs(v, long_row=4600), ("csr", "slab")),  # (a capped block of A without entries)
    "wide10000": (lambda v: E.wide(10000, v), ("csr", "slab")),
    "wide16384": (lambda v: E.wide(16384, v), ("csr", "slab")),
    "wide16385": (lambda v: E.wide(16385, v), ("csr", "slab")),
}
SPMV_PARAMS = [(name, layout) for name, (_, layouts) in SPMV_CASES.items() for layout in layouts]
_made = {}


def _case(name, values):
    """(lp, Prepared) of a case, made once; integer cases are prepared and run without scaling."""
    if (name, values) not in _made:
        lp = SPMV_CASES[name][0](values)
        _made[(name, values)] = (lp, solver.Prepared(lp, **_options(values)))
    return _made[(name, values)]


def _options(values):
    return dict(pdlp_features_off=1) if values == "integer" else {}


def _device_products(lp, P, x, y, values):
    S = solver.DeviceSolver(lp, **_options(values))
    assert (S.n, S.m, S.nnz) == (P.n, P.m, P.nnz)
    S.set("x", x); S.set("y", y)
    S.stage("ax"); S.stage("aty")
    out = S.get("ax", P.m), S.get("aty", P.n)
    S.close()
    return out


def _limit(P, layout):
    return 256 if layout == "slab" else (512 if P.nnz < 2**18 else 2048)


# ---- 1: SpMV against order-free references ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", SPMV_PARAMS)
def test_spmv_integer_data_is_exact(name, layout, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1" if layout == "slab" else "0")
    lp, P = _case(name, "integer")
    assert np.array_equal(P.csr_val, np.rint(P.csr_val)) and np.abs(P.csr_val).max() <= 8 and np.abs(P.csr_val).min() >= 1
    assert np.array_equal(P.csc_val, np.rint(P.csc_val))
    rng = np.random.default_rng(3)
    x, y = rng.integers(-1024, 1025, P.n), rng.integers(-1024, 1025, P.m)
    ax, aty = _device_products(lp, P, x.astype(np.float64), y.astype(np.float64), "integer")
    for got, beg, idx, val, vec in ((ax, P.csr_beg, P.csr_idx, P.csr_val, x), (aty, P.csc_beg, P.csc_idx, P.csc_val, y)):
        want = np.zeros(len(beg) - 1, dtype=np.int64)
        np.add.at(want, np.repeat(np.arange(len(beg) - 1), np.diff(beg)), val.astype(np.int64) * vec[idx])
        assert np.abs(want).max() < 2**53
        assert np.array_equal(got, want.astype(np.float64)), np.nonzero(got != want)[0][:8]


@pytest.mark.parametrize("name,layout", SPMV_PARAMS)
def test_spmv_real_data_against_oracle_orders_and_the_exact_sum(name, layout, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1" if layout == "slab" else "0")
    lp, P = _case(name, "real")
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(P.n), rng.standard_normal(P.m)
    ax, aty = _device_products(lp, P, x, y, "real")
    limit = _limit(P, layout)
    for got, beg, idx, val, vec in ((ax, P.csr_beg, P.csr_idx, P.csr_val, x), (aty, P.csc_beg, P.csc_idx, P.csc_val, y)):
        nm = len(beg) - 1
        short = np.diff(beg) <= limit
        assert np.array_equal(got[short], _spmv(beg, idx, val, vec, nm)[short])  # left to right
        assert np.array_equal(got, _spmv(beg, idx, val, vec, nm, limit))  # long majors: the modelled segment order
        exact, scale, lens = E.exact_major_sums(beg, idx, val, vec)
        bound = (lens + 1) * 2.0**-53 * scale * (1 + 1e-6)
        worst = np.argmax(np.abs(got - exact) - bound)
        print(name, layout, "worst major", worst, "entries", lens[worst], "error", abs(got[worst] - exact[worst]), "bound", bound[worst])
        assert np.all(np.abs(got - exact) <= bound)
        assert np.all(got[lens == 0] == 0.0)


# ---- 2: one trial step ------------------------------------------------------------------------------------------------------
# (long2048 / long2049: the reduction contributions of more long majors than slots — k_long_groups — exist only in a trial)
@pytest.mark.parametrize("name,layout", [(n, l) for n in ("limit512", "segments", "empty_runs", "empty_runs4600", "wide16385") for l in ("csr", "slab")] +
                         [("long2048", "slab"), ("long2049", "slab")])
def test_trial_step_at_the_thresholds(name, layout, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1" if layout == "slab" else "0")
    _trial_step_check(_case(name, "real")[0], None)


# ---- 3: whole solves --------------------------------------------------------------------------------------------------------
_lps, _oracles = {}, {}


def _lp(name):
    if name not in _lps:
        _lps[name] = E.SOLVES[name][0]()
    return _lps[name]


def _kw(name):
    return dict(kkt_tolerance=1e-7, pdlp_iteration_limit=E.SOLVES[name][1])


def _oracle(name):
    """The oracle's solve in the device's reduction order (computed once per case, shared, never changed)."""
    if name not in _oracles:
        _oracles[name] = O.oracle_solve(_lp(name), device_reduction_order=True, device_layout="csr", **_kw(name))
    return _oracles[name]


# name -> workgroups of the persistent loop (test_edge_cases_host.py proves them on the planner)
GRID = {"grid32": 32, "grid33": 33, "grid64": 64, "grid65": 65, "wide10000": 40, "wide16384": 64, "wide16385": 64,
        "empty_runs": 24, "empty_runs4600": 24, "arrow512": 3, "arrow512n4200": 17}
QPS = ("arrow512", "arrow512n4200")


def _loop(ds):
    """(workgroups, mode, one-launch check) of the persistent loop as the solver set it up: mode 0 = all XCDs with the sweep
    barrier, 1 = XCD-local, 2 = all XCDs with the hierarchical barrier."""
    out = ds.stage("small_loop", 3)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("name", sorted(GRID))
def test_whole_solve_on_the_persistent_loop_has_the_oracles_bits(name, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    lp, cpu = _lp(name), _oracle(name)
    print(name, "oracle: iterations", cpu.num_iter, "trials", cpu.num_trials, "restarts", cpu.num_restarts)
    assert cpu.num_trials > cpu.num_iter and cpu.num_restarts >= 1
    ds = solver.DeviceSolver(lp, **_kw(name))
    barriers, checks = ds.stage("trial_barriers", 1)[0], ds.stage("check_launches", 1)[0]
    g = GRID[name]
    # what the set-up derived on the device: the grid, XCD-local up to 32 workgroups, the sweep barrier up to 64, the
    # hierarchical one beyond, the one-launch check up to 64
    assert _loop(ds) == (g, 1 if g <= 32 else 0 if g <= 64 else 2, 1 if g <= 64 else 0)
    gpu = ds.solve()
    launches, fallbacks = ds.stage("persistent_launches", 1)[0], ds.stage("barrier_fallbacks", 1)[0]
    ds.close()
    print(name, "trial_barriers", barriers, "check_launches", checks, "persistent_launches", launches)
    assert launches > 0 and fallbacks == 0
    assert (barriers == 3) if name in QPS else (barriers in (2, 3))
    assert checks == (1 if GRID[name] <= 64 else 10)  # the one-launch check takes at most 64 workgroups
    _assert_equals_oracle(gpu, cpu)


def test_a_qp_whose_n_has_513_entries_in_a_major_keeps_its_launches(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    name = "arrow513"
    lp, cpu = _lp(name), _oracle(name)
    assert cpu.num_trials > cpu.num_iter and cpu.num_restarts >= 1
    ds = solver.DeviceSolver(lp, **_kw(name))
    assert ds.stage("trial_barriers", 1)[0] == 0 and ds.stage("check_launches", 1)[0] == 10 and _loop(ds) == (0, -1, 0)
    gpu = ds.solve()
    assert ds.stage("persistent_launches", 1)[0] == 0
    ds.close()
    _assert_equals_oracle(gpu, cpu)
    batch = solver.DeviceBatch(lp, lanes=2, **_kw(name))
    batch.run([{}])
    I = batch.info()
    batch.close()
    assert I.lanes_concurrent == 1 and I.text.startswith("sequential: ") and "N has a long major" in I.text, I.text


# ---- 3: switch against switch -----------------------------------------------------------------------------------------------
def _state(ds, qp):
    out = {k: ds.get(k, ds.m if k == "y" else ds.n) for k in ("x", "y", "aty") + (("nx",) if qp else ())}
    out["ax"] = ds.get("ax", ds.m)
    out["steps"] = ds.get("steps", 8)
    return out


SWITCHES = [(name, {"PDLP_MI355X_PERSISTENT": "0"}, {}) for name in sorted(GRID)] + [
    ("arrow512", {"PDLP_MI355X_PERSISTENT_QP": "0"}, {}),
    ("arrow512n4200", {"PDLP_MI355X_PERSISTENT_QP": "0"}, {}),
    ("grid32", {"PDLP_MI355X_XCD_LOCAL": "0"}, {"PDLP_MI355X_XCD_LOCAL": "1"}),
    ("grid64", {"PDLP_MI355X_HIER_BARRIER": "0"}, {"PDLP_MI355X_HIER_BARRIER": "1"}),
    ("grid65", {"PDLP_MI355X_HIER_BARRIER": "0"}, {"PDLP_MI355X_HIER_BARRIER": "1"}),
    ("grid64", {"PDLP_MI355X_CHECK_SMALL": "0"}, {"PDLP_MI355X_CHECK_SMALL": "1"}),
]


@pytest.mark.parametrize("name,env_a,env_b", SWITCHES, ids=["%s-%s" % (n, "-".join(sorted(a)).replace("PDLP_MI355X_", "")) for n, a, _ in SWITCHES])
def test_switches_give_the_same_iterates_and_the_same_solve(name, env_a, env_b, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    lp = _lp(name)
    made = []
    for env in (env_a, env_b):  # (switches are read at create)
        for k in ("PDLP_MI355X_PERSISTENT", "PDLP_MI355X_PERSISTENT_QP", "PDLP_MI355X_XCD_LOCAL", "PDLP_MI355X_HIER_BARRIER", "PDLP_MI355X_CHECK_SMALL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        made.append(solver.DeviceSolver(lp, **_kw(name)))
    a, b = made
    qp, g = name in QPS, GRID[name]
    off = "PDLP_MI355X_PERSISTENT" in env_a or "PDLP_MI355X_PERSISTENT_QP" in env_a  # side a keeps its launches per trial
    on_barriers = (3,) if qp else (2, 3)
    if off:
        assert a.stage("trial_barriers", 1)[0] == 0 and b.stage("trial_barriers", 1)[0] in on_barriers
        assert _loop(a) == (0, -1, 0) and _loop(b)[0] == g
    else:
        assert a.stage("trial_barriers", 1)[0] == b.stage("trial_barriers", 1)[0] and a.stage("trial_barriers", 1)[0] in on_barriers
        assert _loop(a)[0] == _loop(b)[0] == g
    if "PDLP_MI355X_XCD_LOCAL" in env_a:
        assert (_loop(a)[1], _loop(b)[1]) == (0, 1)
    if "PDLP_MI355X_HIER_BARRIER" in env_a:
        assert (_loop(a)[1], _loop(b)[1]) == (0, 2)
    if "PDLP_MI355X_CHECK_SMALL" in env_a:
        assert (a.stage("check_launches", 1)[0], b.stage("check_launches", 1)[0]) == (10, 1)
    for iters in (40, 1):  # after 40 and after 41 iterations: both parities of the buffers
        sa, sb = a.iterate(iters), b.iterate(iters)
        assert (sa.iters, sa.trials, sa.restarts) == (sb.iters, sb.trials, sb.restarts)
        va, vb = _state(a, qp), _state(b, qp)
        for k in va:
            assert np.array_equal(va[k], vb[k]), (iters, k)
    a.reset(); b.reset()
    _assert_same_result(a.run(lp.num_col, lp.num_row), b.run(lp.num_col, lp.num_row), name)
    assert b.stage("persistent_launches", 1)[0] > 0 and a.stage("barrier_fallbacks", 1)[0] == 0 and b.stage("barrier_fallbacks", 1)[0] == 0
    assert (a.stage("persistent_launches", 1)[0] == 0) == off
    a.close(); b.close()


# ---- 3: batch lanes at 32 / 33 workgroups -----------------------------------------------------------------------------------
BATCH = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)


@pytest.mark.parametrize("name,concurrent", [("grid32", 8), ("grid33", 1)])
def test_batch_lanes_up_to_32_workgroups(name, concurrent):
    lp = _lp(name)
    variants = [UC.modification(lp, "cost", 3 + i) for i in range(8)]
    held = solver.DeviceSolver(lp, updatable=True, **BATCH)
    solo = []
    for u in variants:  # each variant alone: update + run on one held solver
        held.update(**u)
        solo.append(held.run(lp.num_col, lp.num_row))
    held.close()
    batch = solver.DeviceBatch(lp, lanes=8, **BATCH)
    out = batch.run(variants)
    I = batch.info()
    batch.close()
    print("batch info:", I.text, I.lanes_concurrent)
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, concurrent, 8, 0), I.text
    if concurrent == 1:
        assert "more than one XCD" in I.text, I.text
    for i, (o, ref) in enumerate(zip(out, solo)):
        _assert_same_result(o.result, ref, "variant %d" % i)
