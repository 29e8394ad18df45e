"""The device-side set-up of QPs whose Hessian has an off-diagonal part N (pdlp_setup.hip k_scale_qoff inside the scaling
passes, N's layouts by DeviceMatrix::buildFromDevice, the Hessian-updatable keep from device arrays) against the host set-up
of the same problem (pdlp_host.cpp formulate / scale / finalize): one solver per path, and every comparison is == on bit
patterns — the device's vectors and scalars right after create, N x_start of a dense hot start (every value of N in whatever
layout it got), the iterates after 200 iterations, whole solves.  The oracle is code that exists without this feature: the
host path.  The problems are those of tests/qp_setup_cases.py."""
import numpy as np
import pytest

import qp_setup_cases as QC
import update_hessian_cases as HC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)
DATA = ("cost", "rhs", "lower", "upper", "col_scale", "row_scale")
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
ALL_CASES = sorted(QC.CASES)
SOLVED_CASES = ["sq0", "sq100", "dense_block", "crafted"]
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = QC.large_tridiagonal_qp() if name == "large_tridiagonal" else QC.CASES[name]()
    return _cache[name]


def _start(lp, seed=3):
    rng = np.random.default_rng(seed)  # dense: every slot of N takes part in N x_start
    return dict(col_value=rng.uniform(0.5, 1.5, lp.num_col), row_value=rng.standard_normal(lp.num_row),
                row_dual=rng.standard_normal(lp.num_row))


def _create(lp, start=None, **options):
    if start is None:
        return solver.DeviceSolver(lp, **dict(OPTIONS, **options))
    handle = abi.ProblemHandle(lp, start)
    ds = solver.DeviceSolver(problem_struct=handle.struct, **dict(OPTIONS, **options))
    ds._keep = handle
    return ds


def twins(lp, monkeypatch, start=None, **opts):
    """(host-prepared solver, device-prepared solver) of one problem; the set-up path really differs."""
    out = []
    for dev in ("0", "1"):
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", dev)
        out.append(_create(lp, start=start, **opts))
    assert out[0].setup_scalars()["gpu_setup"] == 0.0
    assert out[1].setup_scalars()["gpu_setup"] == 1.0
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _vectors(ds, off=True):
    out = {k: ds.get(k, ds.m if k in ("rhs", "row_scale") else ds.n) for k in DATA}
    if ds.lp is None or ds.lp.hessian is not None:  # (an LP holds no such vector)
        out["qdiag"] = ds.get("qdiag", ds.n)
    if off:
        out["nx"] = ds.get("nx", ds.n)
    return out


def _assert_same_vectors(a, b, off=True):
    va, vb = _vectors(a, off), _vectors(b, off)
    for k in va:
        assert va[k].shape == vb[k].shape and np.array_equal(bits(va[k]), bits(vb[k])), k
    if off:  # (N x_start is no trivial zero)
        assert np.any(va["nx"] != 0.0)


def _assert_same_setup(a, b, off=True):
    assert (a.n, a.m, a.nnz, a.n_eqs) == (b.n, b.m, b.nnz, b.n_eqs)
    sa, sb = a.setup_scalars(), b.setup_scalars()
    for k in sa:
        if k != "gpu_setup":
            assert np.array_equal(bits([sa[k]]), bits([sb[k]])), (k, sa[k], sb[k])
    _assert_same_vectors(a, b, off)


def _iterate_state(ds, iters=200):
    st = ds.iterate(iters)
    out = {k: ds.get(k, ds.m if k in ("y", "ax") else ds.n) for k in ("x", "y", "ax", "aty")}
    out["counts"] = (st.iters, st.trials, st.restarts)
    return out


def _assert_same_state(a, b):
    assert a["counts"] == b["counts"]
    for k in ("x", "y", "ax", "aty"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def _assert_same_result(a, b):
    for k in SOLUTION:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), k
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))


# ---- 1: same set-up ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", ["0", "1"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_device_setup_equals_host_setup(name, slab, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", slab)
    lp = _lp(name)
    H, D = twins(lp, monkeypatch, start=_start(lp))
    _assert_same_setup(H, D)
    H.close(); D.close()


# ---- 2: same run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_device_setup_iterates_as_host_setup(name, monkeypatch):
    lp = _lp(name)
    H, D = twins(lp, monkeypatch)
    _assert_same_state(_iterate_state(H), _iterate_state(D))
    H.close(); D.close()


@pytest.mark.parametrize("name", SOLVED_CASES)
def test_device_setup_solves_as_host_setup(name, monkeypatch):
    lp = _lp(name)
    H, D = twins(lp, monkeypatch)
    _assert_same_result(H.run(lp.num_col, lp.num_row), D.run(lp.num_col, lp.num_row))
    H.close(); D.close()


# ---- 3: scaling off, sense = -1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,options", [("sq3", dict(pdlp_features_off=abi.FEATURE_SCALING_OFF)), ("random_sparse_qp", {})],
                         ids=["scaling_off", "maximisation"])
def test_scaling_off_and_maximisation(name, options, monkeypatch):
    lp = _lp(name)
    H, D = twins(lp, monkeypatch, start=_start(lp), **options)
    assert D.setup_scalars()["scaled"] == (0.0 if options else 1.0)
    _assert_same_setup(H, D)
    _assert_same_state(_iterate_state(H), _iterate_state(D))
    H.close(); D.close()
    H, D = twins(lp, monkeypatch, **options)
    _assert_same_result(H.run(lp.num_col, lp.num_row), D.run(lp.num_col, lp.num_row))
    H.close(); D.close()


# ---- 4: updatable solvers from the device path -----------------------------------------------------------------------------------
UPDATABLE = [(name, b) for name in ("random_sparse_qp", "crafted") for b in ("hessian", "matrix+hessian")]


@pytest.mark.parametrize("name,updatable", UPDATABLE)
def test_updatable_solvers_keep_the_same_from_both_paths(name, updatable, monkeypatch):
    lp = _lp(name)
    H, D = twins(lp, monkeypatch, start=_start(lp), updatable=updatable)
    sh, sd = H.stage("update_state"), D.stage("update_state")
    assert np.array_equal(sh, sd), (sh, sd)
    assert sd[7] == 1.0 and sd[6] > 0.0
    _assert_same_setup(H, D)
    H.close(); D.close()


@pytest.mark.parametrize("name,updatable", UPDATABLE)
def test_update_values_on_a_device_prepared_solver_equals_fresh_host_create(name, updatable, monkeypatch):
    lp = _lp(name)
    sparse_seed = QC.SPARSE_SEED if name == "random_sparse_qp" else None
    start = _start(lp)
    kinds = ("regen", "scale7") + (("all",) if updatable == "matrix+hessian" else ())
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "1")
    held = _create(lp, updatable=updatable)
    assert held.setup_scalars()["gpu_setup"] == 1.0
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "0")
    for what in kinds:
        u = HC.modification(lp, what, seed=len(name) + 5, sparse_seed=sparse_seed)
        held.update_values(start=start, **u)
        fresh = _create(HC.apply(lp, u), start=start, updatable=updatable)
        assert fresh.setup_scalars()["gpu_setup"] == 0.0
        _assert_same_vectors(held, fresh)
        _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
        fresh.close()
    held.close()


@pytest.mark.parametrize("name,updatable", UPDATABLE)
def test_updatable_device_prepared_solver_never_updated_equals_default(name, updatable, monkeypatch):
    """With the bit the explicit zeros of `crafted` are kept slots of N: they add 0.0 to a sum and change no bit of it."""
    lp = _lp(name)
    start = _start(lp)
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "1")
    a, b = _create(lp, start=start, updatable=updatable), _create(lp, start=start)
    assert a.setup_scalars()["gpu_setup"] == 1.0 and b.setup_scalars()["gpu_setup"] == 1.0
    _assert_same_setup(a, b)
    _assert_same_result(a.run(lp.num_col, lp.num_row), b.run(lp.num_col, lp.num_row))
    a.close(); b.close()


# ---- 5: the automatic rule -----------------------------------------------------------------------------------------------------
def test_large_off_diagonal_qp_takes_the_device_setup_by_itself(monkeypatch):
    monkeypatch.delenv("PDLP_MI355X_GPU_SETUP", raising=False)
    lp = _lp("large_tridiagonal")
    assert lp.num_nz >= 200_000
    D = _create(lp)
    assert D.setup_scalars()["gpu_setup"] == 1.0
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "0")
    H = _create(lp)
    assert H.setup_scalars()["gpu_setup"] == 0.0
    _assert_same_state(_iterate_state(H), _iterate_state(D))
    H.close(); D.close()


# ---- 6: refusals in the same words on both paths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(QC.REFUSALS))
def test_refusals_say_the_same_on_both_paths(what, monkeypatch):
    bad = QC.refused(what)
    words = []
    for dev in ("0", "1"):
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", dev)
        out = solver.solveLpCupdlp(bad, **OPTIONS)
        assert out.status == solver.kError
        words.append(solver.lib().pdlp_mi355x_last_error().decode())
    assert words[0] == words[1] and QC.REFUSALS[what] in words[1], words
    good = _lp("crafted")
    D = _create(good)
    assert D.setup_scalars()["gpu_setup"] == 1.0 and D.iterate(40).iters > 0
    D.close()


# ---- 7: untouched paths report what they reported ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp2", "25fv47"])
def test_diagonal_qp_and_lp_are_prepared_as_before(name, monkeypatch):
    import os
    lp = QC.golden(name) if name == "qp2" else L.HighsLp.from_npz(os.path.join(QC.GOLD, "instances", name + ".npz"))
    H, D = twins(lp, monkeypatch)
    _assert_same_setup(H, D, off=False)
    H.close(); D.close()
