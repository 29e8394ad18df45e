"""The device-resident entries on the GPU: pdlp_mi355x_create_device / _update_device / _run_device, given the problem, the
updates and the result vectors as arrays in HBM (torch tensors), must give the bits of pdlp_mi355x_create / _update /
_update_matrix / _update_values / _run on the same data in host arrays — every solution vector (array_equal), every count
and scalar (==).  The reference is always the existing host entry on the same problem, computed first and shared.  No
tolerance anywhere."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

torch = pytest.importorskip("torch")
from highs_amd import tensors as T  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "term_iterate", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
FLAGS = ("value_valid", "dual_valid")
INSTANCES = ("afiro", "adlittle", "25fv47", "standmps", "galenet", "qp0", "sq100", "maximise")
_lps, _refs = {}, {}


def _lp(name):
    if name not in _lps:
        if name == "maximise":
            _lps[name] = lpgen.random_lp(1)  # (odd seeds maximise)
            assert _lps[name].sense == -1
        else:
            sub = "qp" if name.startswith(("qp", "sq")) else "instances"
            _lps[name] = L.HighsLp.from_npz(os.path.join(GOLD, sub, name + ".npz"))
    return _lps[name]


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to("cuda")


def _dev_update(u):
    """update_cases / update_matrix_cases keyword arguments with every array a tensor."""
    out = {}
    for k, v in u.items():
        if k == "offset":
            out[k] = v
        elif k == "start":
            out[k] = None if v is None else {s: _dev(a) for s, a in v.items()}
        else:
            out[k] = _dev(v)
    return out


def _host_run(S, lp):
    return S.run(lp.num_col, lp.num_row)


def _ref(name, scaling_off=False):
    """create + run on host arrays: the reference of create_device + run_device."""
    key = (name, scaling_off)
    if key not in _refs:
        lp = _lp(name)
        S = solver.DeviceSolver(lp, pdlp_features_off=abi.FEATURE_SCALING_OFF if scaling_off else 0, **OPTIONS)
        _refs[key] = _host_run(S, lp)
        S.close()
    return _refs[key]


def _same(got, want, what, vectors=SOLUTION):
    """got: tensors.TensorResult (or a host ResultHandle); want: a host ResultHandle."""
    for k in vectors:
        g = getattr(got, k)
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert np.array_equal(g, getattr(want, k)), (what, k)
    for k in COUNTS + SCALARS + FLAGS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


# ---- 1. create_device + run_device = create + run -----------------------------------------------------------------------
@pytest.mark.parametrize("scaling_off", [False, True], ids=["scaled", "scaling_off"])
@pytest.mark.parametrize("name", INSTANCES)
def test_create_device_and_run_device_match_create_and_run(name, scaling_off):
    ref = _ref(name, scaling_off)
    lp = _lp(name)
    tp = T.TensorProblem.from_lp(lp, "cuda")
    S = solver.DeviceSolver.from_tensors(tp, pdlp_features_off=abi.FEATURE_SCALING_OFF if scaling_off else 0, **OPTIONS)
    got = S.run_tensors()
    print(name, "scaling off" if scaling_off else "scaled", "term", got.term_code, "iterate", got.term_iterate, "iterations", got.num_iter)
    _same(got, ref, name)
    assert all(getattr(got, k).is_cuda for k in SOLUTION)
    S.close()


def test_both_average_and_current_iterates_are_returned_among_the_references():
    iterates = {(_ref(n, off).term_code, _ref(n, off).term_iterate) for n in INSTANCES for off in (False, True)}
    print(sorted(iterates))
    assert {it for _, it in iterates} == {0, 1}, iterates
    assert _ref("galenet").term_code in (abi.TERM_INFEASIBLE, abi.TERM_INFEASIBLE_OR_UNBOUNDED)


# ---- 2. post-solve edges ------------------------------------------------------------------------------------------------
def _kinds_lp(m, n0, kinds, seed):
    """m rows whose kinds cycle through `kinds` (0 equality, 1 <=, 2 >=, 3 ranged, 4 free), n0 boxed columns, about four
    entries per row, feasible at a point inside the box."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n0))
    for i in range(m):
        at = rng.choice(n0, 4, replace=False)
        A[i, at] = rng.uniform(0.5, 2.0, 4) * rng.choice([-1.0, 1.0], 4)
    xs = rng.uniform(0.2, 0.8, n0)
    ax = A @ xs
    inf = float("inf")
    rl, ru = np.full(m, -inf), np.full(m, inf)
    for i in range(m):
        k = kinds[i % len(kinds)]
        if k == 0: rl[i] = ru[i] = ax[i]
        elif k == 1: ru[i] = ax[i] + 0.3
        elif k == 2: rl[i] = ax[i] - 0.3
        elif k == 3: rl[i], ru[i] = ax[i] - 0.2, ax[i] + 0.4
    rows, cols = np.nonzero(A.T)
    a_start = np.zeros(n0 + 1, np.int32)
    a_start[1:] = np.cumsum(np.bincount(rows, minlength=n0))
    return L.HighsLp(n0, m, rng.standard_normal(n0), np.zeros(n0), np.ones(n0), rl, ru, a_start, cols.astype(np.int32),
                     A.T[rows, cols], 1, 0.25, "kinds").normalise()


def _device_equals_host(lp, what, **options):
    host = solver.DeviceSolver(lp, **OPTIONS, **options)
    ref = _host_run(host, lp)
    host.close()
    S = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), **OPTIONS, **options)
    _same(S.run_tensors(), ref, what)
    S.close()
    return ref


@pytest.mark.parametrize("m, n0", [(255, 255), (256, 257), (257, 255), (255, 257), (256, 255), (257, 257)])
def test_postsolve_with_all_row_kinds_interleaved_across_a_workgroup_boundary(m, n0):
    # ranged and free rows every second and fifth row: their ranks (about 100) sit beside rows on both sides of i = 256
    lp = _kinds_lp(m, n0, (0, 1, 3, 2, 4), seed=m * 1000 + n0)
    ref = _device_equals_host(lp, (m, n0))
    assert np.any(ref.row_value != 0.0) and np.any(ref.row_dual != 0.0)
    _device_equals_host(lp, (m, n0, "scaling off"), pdlp_features_off=abi.FEATURE_SCALING_OFF)


def test_postsolve_without_a_ranged_or_free_row_and_with_ranged_rows_only():
    _device_equals_host(_kinds_lp(257, 255, (0, 1, 2), seed=7), "no ranged row")
    _device_equals_host(_kinds_lp(257, 255, (3,), seed=8), "ranged rows only")


def test_every_subset_of_null_result_vectors_matches_run():
    lp = _kinds_lp(257, 255, (0, 1, 3, 2, 4), seed=11)
    host = solver.DeviceSolver(lp, **OPTIONS)
    refs = {}
    for r in range(5):
        for absent in itertools.combinations(SOLUTION, r):
            R = abi.ResultHandle(lp.num_col, lp.num_row)
            for k in absent:
                setattr(R.struct, k, None)
            assert solver.lib().pdlp_mi355x_run(host.h, C.byref(R.struct)) == 0
            refs[absent] = R
    host.close()
    S = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), **OPTIONS)
    seen = set()
    for absent, ref in refs.items():
        R = T.TensorResult(lp.num_col, lp.num_row, torch.device("cuda", 0))
        for k in SOLUTION:
            R.tensors[k].fill_(-7.0)
        for k in absent:
            setattr(R.struct, k, None)
        torch.cuda.synchronize()
        assert solver.lib().pdlp_mi355x_run_device(S.h, C.byref(R.struct)) == 0, solver.lib().pdlp_mi355x_last_error()
        present = tuple(k for k in SOLUTION if k not in absent)
        _same(R, ref, absent, vectors=present)
        for k in absent:  # a NULL vector is skipped: nothing is written anywhere near it
            assert bool((R.tensors[k] == -7.0).all()), (absent, k)
        seen.add((R.value_valid, R.dual_valid))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    S.close()


# ---- 3. updates ---------------------------------------------------------------------------------------------------------
def _pair(lp, **options):
    """A host-made and a device-made solver of the same problem (two solvers, so neither side sees the other's update)."""
    host = solver.DeviceSolver(lp, **OPTIONS, **options)
    dev = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), **OPTIONS, **options)
    return host, dev


@pytest.mark.parametrize("what", UC.KINDS)
@pytest.mark.parametrize("name", ["adlittle", "25fv47"])
def test_update_device_and_run_device_match_update_and_run(name, what):
    lp = _lp(name)
    u = UC.modification(lp, what, seed=31)
    host, dev = _pair(lp, updatable=True)
    host.update(**u)
    ref = _host_run(host, lp)
    dev.update_tensors(**_dev_update(u))
    _same(dev.run_tensors(), ref, (name, what))
    host.close(); dev.close()


def test_update_device_with_matrix_values_matches_update_matrix():
    lp = _lp("25fv47")
    a = MC.new_values(lp, 200, ("jitter",))
    u = UC.modification(lp, "all", seed=32)
    host, dev = _pair(lp, updatable="matrix")
    host.update_matrix(a, **u)
    ref = _host_run(host, lp)
    dev.update_tensors(a_value=_dev(a), **_dev_update(u))
    _same(dev.run_tensors(), ref, "a_value + data")
    # a_value alone, on the solvers as the first update left them
    a2 = MC.new_values(lp, 201, ("jitter",))
    host.update_matrix(a2)
    ref = _host_run(host, lp)
    dev.update_tensors(a_value=_dev(a2))
    _same(dev.run_tensors(), ref, "a_value alone")
    host.close(); dev.close()


def test_update_device_with_hessian_values_matches_update_values():
    lp = _lp("sq100")
    q = np.asarray(lp.hessian[2]) * 0.7
    host, dev = _pair(lp, updatable="hessian")
    host.update_values(q_value=q)
    ref = _host_run(host, lp)
    dev.update_tensors(q_value=_dev(q))
    _same(dev.run_tensors(), ref, "q_value")
    host.close(); dev.close()
    # both arrays together, with data
    a = MC.new_values(lp, 202, ("jitter",))
    u = UC.modification(lp, "cost", seed=33)
    host, dev = _pair(lp, updatable="matrix+hessian")
    host.update_values(a_value=a, q_value=q * 1.9, **u)
    ref = _host_run(host, lp)
    dev.update_tensors(a_value=_dev(a), q_value=_dev(q * 1.9), **_dev_update(u))
    _same(dev.run_tensors(), ref, "a_value + q_value + cost")
    # a_value alone on a Hessian-updatable solver goes to update_values as well
    host.update_matrix(lp.a_value)
    ref = _host_run(host, lp)
    dev.update_tensors(a_value=_dev(lp.a_value))
    _same(dev.run_tensors(), ref, "a_value on a Hessian-updatable solver")
    host.close(); dev.close()


def test_a_hot_start_from_device_vectors_equals_the_host_hot_start():
    lp = _lp("adlittle")
    first = _ref("adlittle")
    start = dict(col_value=first.col_value, row_value=first.row_value, row_dual=first.row_dual)
    dstart = {k: _dev(v) for k, v in start.items()}
    # at create
    handle = abi.ProblemHandle(lp, start)
    host = solver.DeviceSolver(problem_struct=handle.struct, updatable=True, **OPTIONS)
    ref = _host_run(host, lp)
    dev = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), start=dstart, updatable=True, **OPTIONS)
    got = dev.run_tensors()
    _same(got, ref, "start at create")
    assert ref.num_iter != first.num_iter  # the start was honoured: another solve
    # with an update
    u = UC.modification(lp, "cost", seed=34)
    host.update(start=start, **u)
    ref = _host_run(host, lp)
    dev.update_tensors(start=dstart, **_dev_update(u))
    _same(dev.run_tensors(), ref, "start with an update")
    # and a cold start afterwards
    host.update(**u)
    ref = _host_run(host, lp)
    dev.update_tensors(**_dev_update(u))
    _same(dev.run_tensors(), ref, "cold again")
    host.close(); dev.close()


def test_host_and_device_entries_mix_on_one_solver():
    lp = _lp("adlittle")
    u = UC.modification(lp, "all", seed=35)
    ref_solver = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    ref_solver.update(**u)
    ref = _host_run(ref_solver, lp)
    ref_solver.close()
    # host create, update_device, host run
    S = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    S.update_tensors(**_dev_update(u))
    _same(_host_run(S, lp), ref, "create, update_device, run")
    S.close()
    # create_device, host update, run_device
    S = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), updatable=True, **OPTIONS)
    S.update(**u)
    _same(S.run_tensors(), ref, "create_device, update, run_device")
    S.close()


def test_three_updates_in_a_row_on_one_solver():
    lp = _lp("25fv47")
    host, dev = _pair(lp, updatable=True)
    out = {k: torch.empty(lp.num_col if k.startswith("col") else lp.num_row, dtype=torch.float64, device="cuda") for k in SOLUTION}
    for step, what in enumerate(("cost", "row_bounds", "all")):
        u = UC.modification(lp, what, seed=40 + step)
        host.update(**u)
        ref = _host_run(host, lp)
        dev.update_tensors(**_dev_update(u))
        _same(dev.run_tensors(out=out), ref, (step, what))
    host.close(); dev.close()


# ---- 4. refusals leave the solver as it was -------------------------------------------------------------------------------
def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_refused_updates_leave_the_solver_as_it_was():
    lp = _lp("adlittle")
    ref = _ref("adlittle")
    kind = UC.row_kind(np.asarray(lp.row_lower), np.asarray(lp.row_upper))
    row = int(np.nonzero(kind == 0)[0][0])  # an equality row becomes a <= row
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    lo[row] = -np.inf
    host, dev = _pair(lp, updatable="matrix")
    host_words = _refused(host.update, row_lower=lo, row_upper=up)
    words = _refused(dev.update_tensors, row_lower=_dev(lo), row_upper=_dev(up), col_cost=_dev(np.asarray(lp.col_cost) * 2.0))
    assert words == host_words.replace("pdlp_mi355x_update failed: ", "pdlp_mi355x_update_device failed: pdlp_mi355x_update_device: ")
    assert "row %d would change its kind from equality to <= (upper bound only)" % row in words
    _same(dev.run_tensors(), ref, "after a kind change")
    words = _refused(dev.update_tensors, a_value=_dev(np.zeros(lp.a_value.size)), col_cost=_dev(np.asarray(lp.col_cost) * 2.0))
    assert words.startswith("pdlp_mi355x_update_device failed: pdlp_mi355x_update_device: ") and "no matrix nonzeros" in words
    assert "no matrix nonzeros" in _refused(host.update_matrix, np.zeros(lp.a_value.size))
    _same(dev.run_tensors(), ref, "after an all-zero matrix")
    host.close(); dev.close()
    # a missing updatable bit
    dev = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), **OPTIONS)
    words = _refused(dev.update_tensors, col_cost=_dev(lp.col_cost))
    assert "pdlp_mi355x_update_device: pdlp_mi355x_update: the solver was not created for updates" in words
    _same(dev.run_tensors(), ref, "after a refused update of a solver that takes none")
    dev.close()
    dev = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), updatable=True, **OPTIONS)
    assert "lacks PDLP_UPDATABLE_MATRIX" in _refused(dev.update_tensors, a_value=_dev(lp.a_value))
    _same(dev.run_tensors(), ref, "after a refused matrix update")
    dev.close()


def test_a_negative_diagonal_is_refused_and_leaves_the_solver_as_it_was():
    lp = _lp("sq100")
    ref = _ref("sq100")
    q = -np.asarray(lp.hessian[2], dtype=np.float64)
    host, dev = _pair(lp, updatable="hessian")
    host_words = _refused(host.update_values, q_value=q)
    words = _refused(dev.update_tensors, q_value=_dev(q), col_cost=_dev(np.asarray(lp.col_cost) * 3.0))
    assert words == host_words.replace("pdlp_mi355x_update_values failed: ", "pdlp_mi355x_update_device failed: pdlp_mi355x_update_device: ")
    assert "the diagonal entry of column" in words
    _same(dev.run_tensors(), ref, "after a negative diagonal")
    host.close(); dev.close()


# ---- 5. the pointer check -------------------------------------------------------------------------------------------------
# Host memory is refused BEFORE anything is launched or copied, so nothing below runs a kernel on a bad pointer.
def test_create_device_refuses_a_host_pointer_in_every_field():
    lp = _lp("sq100")
    tp = T.TensorProblem.from_lp(lp, "cuda")
    zeros = {k: _dev(np.zeros(lp.num_col if k == "col_value" else lp.num_row)) for k in ("col_value", "row_value", "row_dual")}
    opt = abi.default_params(**OPTIONS)
    fields = [("a_start", abi.c_i32p, np.int32), ("a_index", abi.c_i32p, np.int32), ("a_value", abi.c_f64p, np.float64),
              ("col_cost", abi.c_f64p, np.float64), ("col_lower", abi.c_f64p, np.float64), ("col_upper", abi.c_f64p, np.float64),
              ("row_lower", abi.c_f64p, np.float64), ("row_upper", abi.c_f64p, np.float64),
              ("start_col_value", abi.c_f64p, np.float64), ("start_row_value", abi.c_f64p, np.float64),
              ("start_row_dual", abi.c_f64p, np.float64), ("q_start", abi.c_i32p, np.int32), ("q_index", abi.c_i32p, np.int32),
              ("q_value", abi.c_f64p, np.float64)]
    host_array = np.zeros(max(lp.num_col, lp.num_row, lp.a_value.size) + 1)
    for field, ctype, dtype in fields:
        P, keep = tp.struct(zeros)
        setattr(P, field, host_array.view(dtype).ctypes.data_as(ctype))
        h = C.c_void_p()
        assert solver.lib().pdlp_mi355x_create_device(C.byref(P), C.byref(opt), None, C.byref(h)) != 0, field
        assert solver.lib().pdlp_mi355x_last_error().decode() == "pdlp_mi355x_create_device: %s is not device memory on device 0" % field
        assert not h.value
    # tensors on the right device are accepted, and the refusals have left nothing behind in the runtime
    S = solver.DeviceSolver.from_tensors(tp, **OPTIONS)
    _same(S.run_tensors(), _ref("sq100"), "after the refusals")
    S.close()


def test_update_device_and_run_device_refuse_a_host_pointer_in_every_field():
    lp = _lp("sq100")
    ref = _ref("sq100")
    dev = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), updatable="matrix+hessian", **OPTIONS)
    host_array = np.ones(max(lp.num_col, lp.num_row, lp.a_value.size, lp.hessian[2].size) + 1)
    hp = host_array.ctypes.data_as(abi.c_f64p)
    a, q = _dev(lp.a_value), _dev(lp.hessian[2])
    good = dict(col_cost=_dev(lp.col_cost), col_lower=_dev(lp.col_lower), col_upper=_dev(lp.col_upper), row_lower=_dev(lp.row_lower),
                row_upper=_dev(lp.row_upper),
                start=dict(col_value=_dev(np.zeros(lp.num_col)), row_value=_dev(np.zeros(lp.num_row)), row_dual=_dev(np.zeros(lp.num_row))))
    lib = solver.lib()
    for field in ("a_value", "q_value", "col_cost", "col_lower", "col_upper", "row_lower", "row_upper", "start_col_value",
                  "start_row_value", "start_row_dual"):
        U = T.TensorUpdate(lp.num_col, lp.num_row, torch.device("cuda", 0), **good)
        ap, qp = T.pointer(a, abi.c_f64p), T.pointer(q, abi.c_f64p)
        if field == "a_value": ap = hp
        elif field == "q_value": qp = hp
        else: setattr(U.struct, field, hp)
        assert lib.pdlp_mi355x_update_device(dev.h, ap, a.numel(), qp, q.numel(), C.byref(U.struct), None) != 0, field
        assert lib.pdlp_mi355x_last_error().decode() == "pdlp_mi355x_update_device: %s is not device memory on device 0" % field
    for field in SOLUTION:
        R = T.TensorResult(lp.num_col, lp.num_row, torch.device("cuda", 0))
        setattr(R.struct, field, hp)
        assert lib.pdlp_mi355x_run_device(dev.h, C.byref(R.struct)) != 0, field
        assert lib.pdlp_mi355x_last_error().decode() == "pdlp_mi355x_run_device: %s is not device memory on device 0" % field
    assert np.all(host_array == 1.0)
    # the solver is as it was, and takes the same update with tensors
    _same(dev.run_tensors(), ref, "after the refusals")
    dev.update_tensors(a_value=a, q_value=q, **good)
    dev.close()


# ---- 6. stream ordering ---------------------------------------------------------------------------------------------------
def test_update_tensors_reads_behind_the_stream_that_fills_its_tensors():
    lp = _lp("adlittle")
    u = UC.modification(lp, "all", seed=36)
    host, dev = _pair(lp, updatable=True)
    host.update(**u)
    ref = _host_run(host, lp)
    src = _dev_update(u)
    bufs = {k: torch.zeros_like(v) for k, v in src.items() if k != "offset"}
    work = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):  # the fills wait behind some milliseconds of work on this stream
            work = work @ work * 1e-3
        for k, b in bufs.items():
            b.copy_(src[k])
        dev.update_tensors(offset=u["offset"], **bufs)  # (no synchronisation in between)
    _same(dev.run_tensors(), ref, "filled on a side stream")
    torch.cuda.synchronize()
    host.close(); dev.close()


# ---- 7. Python ------------------------------------------------------------------------------------------------------------
def test_run_tensors_writes_into_the_given_tensors_and_returns_them():
    lp = _lp("afiro")
    ref = _ref("afiro")
    S = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda:0"), **OPTIONS)
    out = dict(col_value=torch.full((lp.num_col,), -1.0, dtype=torch.float64, device="cuda"),
               row_dual=torch.full((lp.num_row,), -1.0, dtype=torch.float64, device="cuda"))
    R = S.run_tensors(out=out)
    assert R.col_value is out["col_value"] and R.row_dual is out["row_dual"]
    assert all(getattr(R, k).is_cuda and getattr(R, k).dtype == torch.float64 for k in SOLUTION)
    _same(R, ref, "out=")
    assert np.array_equal(out["col_value"].cpu().numpy(), ref.col_value)
    with pytest.raises(ValueError, match="elements are needed"):
        S.run_tensors(out=dict(col_value=torch.zeros(lp.num_col + 1, dtype=torch.float64, device="cuda")))
    with pytest.raises(ValueError, match="cuda device is needed"):
        S.run_tensors(out=dict(col_value=torch.zeros(lp.num_col, dtype=torch.float64)))
    with pytest.raises(TypeError, match="dtype torch.float64 is needed"):
        S.update_tensors(col_cost=torch.zeros(lp.num_col, dtype=torch.float32, device="cuda"))
    S.close()


def test_the_package_imports_without_torch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.modules['torch'] = None\n"
            "import highs_amd, highs_amd.solver, highs_amd.tensors\n"
            "assert highs_amd.solver.lib().pdlp_mi355x_abi_version() == 6\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
