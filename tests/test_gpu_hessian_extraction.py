"""The Hessian's extraction on the device (highs_amd/csrc/pdlp_setup.hip gpuExtractHessian) against the host walk it
restates (pdlp_host.cpp extractHessian / extractHessianKept).  Three solvers of one problem: `dev` — device-side set-up with the
extraction on the device; `walk` — the same set-up with PDLP_MI355X_GPU_HESSIAN=0, the walk's result uploaded; `host` — the
whole set-up on the host.  Every comparison is == on bit patterns.  The kept assembly map of a Hessian-updatable solver is
held against the numpy restatement of tests/hessian_restated.py, which tests/test_hessian_extraction_host.py holds against
the walk.  The problems are those of tests/hessian_extraction_cases.py."""
import numpy as np
import pytest

import hessian_extraction_cases as XC
import hessian_restated as HR
import qp_setup_cases as QC
import update_hessian_cases as HC
from highs_amd import abi, solver

pytestmark = pytest.mark.gpu
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)
MODES = {"plain": {}, "kept": dict(updatable="hessian")}
DATA = ("cost", "rhs", "lower", "upper", "col_scale", "row_scale")
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
PATHS = {"dev": ("1", "1"), "walk": ("1", "0"), "host": ("0", "1")}  # name -> PDLP_MI355X_GPU_SETUP, PDLP_MI355X_GPU_HESSIAN
REASON = {"dev": "on_device", "walk": "switched_off", "host": "host_setup"}
SLAB_CASES = ("crafted", "tridiagonal_129", "triple_pair", "dense_block", "large_tridiagonal")
LAYOUTS = [(name, "0") for name in sorted(XC.CASES)] + [(name, "1") for name in SLAB_CASES]
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = XC.CASES[name]()
    return _cache[name]


def _start(lp, seed=3):
    rng = np.random.default_rng(seed)  # dense: every slot of N takes part in N x_start
    return dict(col_value=rng.uniform(0.5, 1.5, lp.num_col), row_value=rng.standard_normal(lp.num_row),
                row_dual=rng.standard_normal(lp.num_row))


def _create(lp, path, monkeypatch, start=None, **options):
    setup, hessian = PATHS[path]
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", setup)
    monkeypatch.setenv("PDLP_MI355X_GPU_HESSIAN", hessian)
    if start is None:
        ds = solver.DeviceSolver(lp, **dict(OPTIONS, **options))
    else:
        handle = abi.ProblemHandle(lp, start)
        ds = solver.DeviceSolver(problem_struct=handle.struct, **dict(OPTIONS, **options))
        ds._keep = handle
    x = ds.hessian_extraction()
    assert solver.HESSIAN_REASONS[int(x["reason"])] == REASON[path] and x["on_device"] == (1.0 if path == "dev" else 0.0), (path, x)
    assert ds.setup_scalars()["gpu_setup"] == float(setup)
    return ds


def triplet(lp, monkeypatch, start=None, **options):
    return [_create(lp, path, monkeypatch, start=start, **options) for path in ("dev", "walk", "host")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _vectors(ds, n_off, has_diag):
    out = {k: ds.get(k, ds.m if k in ("rhs", "row_scale") else ds.n) for k in DATA}
    if has_diag:
        out["qdiag"] = ds.get("qdiag", ds.n)
    if n_off:
        out["nx"] = ds.get("nx", ds.n)  # N x_start of a dense start: every value of N in whatever layout it got
    return out


def _state(ds, iters=200):
    st = ds.iterate(iters)
    out = {k: ds.get(k, ds.m if k in ("y", "ax") else ds.n) for k in ("x", "y", "ax", "aty")}
    return out, (st.iters, st.trials, st.restarts)


def _assert_same_dict(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def _assert_same_result(a, b):
    for k in SOLUTION:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), k
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))


# ---- 1: which path ran, and what it counted ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_switch_chooses_the_path_and_both_count_the_same(mode, monkeypatch):
    lp = _lp("crafted")
    R = HR.extraction(lp, lp.num_col, kept=mode == "kept")
    for path in PATHS:  # (_create asserts stage "hessian_extraction" [0] and [1])
        ds = _create(lp, path, monkeypatch, **MODES[mode])
        x = ds.hessian_extraction()
        assert (x["taken_slots"], x["n_slots"]) == (R["taken"], R["n_off"]), (path, x)
        sec = ds.stage("setup_seconds", 5)
        assert np.all(sec >= 0.0) and (path == "host" or sec[0] + sec[1] > 0.0)  # extraction and upload, whichever side did them
        assert (x["temp_bytes"] > 0.0) == (path == "dev")
        ds.close()


def test_an_lp_and_a_decreasing_q_start_are_left_to_the_host(monkeypatch):
    lp = XC.decreasing_start_qp()
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "1")
    monkeypatch.setenv("PDLP_MI355X_GPU_HESSIAN", "1")
    for mode in MODES.values():
        ds = solver.DeviceSolver(lp, **dict(OPTIONS, **mode))
        x = ds.hessian_extraction()
        assert x["on_device"] == 0.0 and solver.HESSIAN_REASONS[int(x["reason"])] == "q_start" and x["n_slots"] == 2.0
        host = _create(lp, "host", monkeypatch, **mode)
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "1")
        _assert_same_dict(_vectors(ds, 2, True), _vectors(host, 2, True), "decreasing q_start")
        _assert_same_dict(*[_state(s)[0] for s in (ds, host)], "decreasing q_start, iterates")
        ds.close(); host.close()
    lp = XC.all_zero_qp()
    lp.hessian = None
    ds = solver.DeviceSolver(lp, **OPTIONS)
    assert solver.HESSIAN_REASONS[int(ds.hessian_extraction()["reason"])] == "no_slots"
    ds.close()


# ---- 2: bit equality of everything the set-up leaves, and of the run that follows ------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,slab", LAYOUTS)
def test_device_extraction_equals_the_walk(name, slab, mode, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", slab)
    lp = _lp(name)
    kept = mode == "kept"
    R = HR.extraction(lp, lp.num_col, kept=kept)  # (the map's first num_col destinations and its counts need no slack columns)
    n_off, has_diag = R["n_off"], (XC.caller_slots(lp) > 0 if kept else R["taken"] > 0)
    S = triplet(lp, monkeypatch, start=_start(lp), **MODES[mode])
    dev = S[0]
    x = dev.hessian_extraction()
    assert (x["taken_slots"], x["n_slots"]) == (R["taken"], n_off)
    ref = _vectors(dev, n_off, has_diag)
    if n_off:
        assert np.any(ref["nx"] != 0.0) or not np.any(R["q_val"] != 0.0)
    if not has_diag:  # every value zero, plain solver: an LP, with no such vector
        with pytest.raises(RuntimeError):
            dev.get("qdiag", dev.n)
    scal, upd = dev.setup_scalars(), dev.stage("update_state")
    for other, path in zip(S[1:], ("walk", "host")):
        assert (dev.n, dev.m, dev.nnz, dev.n_eqs) == (other.n, other.m, other.nnz, other.n_eqs)
        _assert_same_dict(ref, _vectors(other, n_off, has_diag), path)
        so = other.setup_scalars()
        for k in scal:
            assert k == "gpu_setup" or np.array_equal(bits([scal[k]]), bits([so[k]])), (path, k, scal[k], so[k])
        assert np.array_equal(upd, other.stage("update_state")), (path, upd, other.stage("update_state"))
    if kept:  # the kept map, array for array: the device's own and the walk's uploaded one
        full = HR.extraction(lp, dev.n, kept=True)
        for s, path in zip(S, ("dev", "walk", "host")):
            got = s.hessian_map()
            for k in ("dst_beg", "src_slot", "off_row", "off_col"):
                assert np.array_equal(got[k], full[k]), (path, k)
        assert upd[7] == 1.0 and upd[6] > 0.0
    states = [_state(s) for s in S]
    for (st, counts), path in zip(states[1:], ("walk", "host")):
        assert counts == states[0][1], path
        _assert_same_dict(states[0][0], st, path + ", iterates")
    for s in S:
        s.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["crafted", "sq100", "dense_block"])
def test_whole_solves_are_the_same(name, mode, monkeypatch):
    lp = _lp(name)
    S = triplet(lp, monkeypatch, **MODES[mode])
    res = [s.run(lp.num_col, lp.num_row) for s in S]
    assert res[0].num_iter > 0
    _assert_same_result(res[0], res[1])
    _assert_same_result(res[0], res[2])
    for s in S:
        s.close()


# ---- 3: an update on the device-built map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("updatable", ["hessian", "matrix+hessian"])
@pytest.mark.parametrize("name", ["crafted", "random_sparse_qp", "triple_pair"])
def test_update_values_on_the_device_built_map_equals_a_host_prepared_solver(name, updatable, monkeypatch):
    lp = _lp(name)
    start = _start(lp)
    u = HC.modification(lp, "regen", seed=len(name) + 5, sparse_seed=QC.SPARSE_SEED if name == "random_sparse_qp" else None)
    dev, host = (_create(lp, path, monkeypatch, updatable=updatable) for path in ("dev", "host"))
    n_off = int(dev.hessian_extraction()["n_slots"])
    for s in (dev, host):
        s.update_values(start=start, **u)
    after = _vectors(dev, n_off, True)
    _assert_same_dict(after, _vectors(host, n_off, True), "after update_values")
    assert np.array_equal(dev.stage("update_state"), host.stage("update_state"))
    # ... and a fresh host-prepared solver of the modified problem
    fresh = _create(HC.apply(lp, u), "host", monkeypatch, start=start, updatable=updatable)
    _assert_same_dict(after, _vectors(fresh, n_off, True), "fresh create")
    res = [s.run(lp.num_col, lp.num_row) for s in (dev, host, fresh)]
    _assert_same_result(res[0], res[1])
    _assert_same_result(res[0], res[2])
    for s in (dev, host, fresh):
        s.close()


# ---- 4: refusals, word for word ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("what", sorted(XC.REFUSALS))
def test_refusals_say_the_same_on_every_path(what, mode, monkeypatch):
    make, words, modes = XC.REFUSALS[what]
    bad = make()
    said = []
    for path in ("dev", "walk", "host"):
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", PATHS[path][0])
        monkeypatch.setenv("PDLP_MI355X_GPU_HESSIAN", PATHS[path][1])
        try:
            ds = solver.DeviceSolver(bad, **dict(OPTIONS, **MODES[mode]))
        except RuntimeError as e:
            said.append(str(e))
        else:
            said.append(None)
            assert ds.hessian_extraction()["on_device"] == (1.0 if path == "dev" else 0.0)
            ds.close()
    assert said[0] == said[1] == said[2], said
    if mode in modes:
        assert said[0] is not None and words in said[0], said
    else:
        assert said[0] is None
    # the refusal left the device usable
    good = _create(_lp("crafted"), "dev", monkeypatch, **MODES[mode])
    assert good.iterate(40).iters > 0
    good.close()
