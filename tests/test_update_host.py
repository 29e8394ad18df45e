"""pdlp_mi355x_update without a GPU, through its host twin pdlp_mi355x_host_prepare_updated: prepare P, keep the scale
factors of every scaling pass, replay the update — the result must be, bit for bit, what pdlp_mi355x_host_prepare gives
on the modified problem P' built in Python.  host_prepare is pinned on the oracle by tests/test_host.py
(test_formulate_scale_bit_exact_vs_oracle), so this ties the replay to the reference.  Also: why the passes are kept
(dividing once by the accumulated scale differs), every refusal that needs no solver handle, and the ABI numbers."""
import ctypes as C
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
from highs_amd import abi, solver
from highs_amd import lp as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CTEST = ["25fv47", "adlittle", "afiro", "avgas", "blending", "chip", "e226", "scrs8", "sctest", "shell", "stair",
         "standata", "standgub"]
MAKERS = {name: (lambda name=name: L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz"))) for name in CTEST}
MAKERS["structured_lp"] = lambda: lpgen.structured_lp()
MAKERS["random_diag_qp"] = lambda: lpgen.random_diag_qp(3)
MAKERS["random_sparse_qp"] = lambda: lpgen.random_sparse_qp(3)
VECTORS = ("cost", "rhs", "lower", "upper", "col_scale", "row_scale")

_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


def _prepare(lp, update=None, **options):
    """(rc, dict of the standard form's vectors and norms): host_prepare, or host_prepare_updated with `update`."""
    lib = solver.lib()
    P = abi.ProblemHandle(lp)
    params = abi.default_params(**options)
    F = abi.PdlpPrepared()
    if update is None:
        rc = lib.pdlp_mi355x_host_prepare(C.byref(P.struct), C.byref(params), C.byref(F))
    else:
        rc = lib.pdlp_mi355x_host_prepare_updated(C.byref(P.struct), C.byref(params), C.byref(update.struct), C.byref(F))
    if rc != 0:
        return rc, lib.pdlp_mi355x_last_error().decode()
    g = lambda p, k: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].copy()
    out = dict(cost=g(F.cost, F.n), rhs=g(F.rhs, F.m), lower=g(F.lower, F.n), upper=g(F.upper, F.n),
               col_scale=g(F.col_scale, F.n), row_scale=g(F.row_scale, F.m), norm_cost=F.norm_cost, norm_rhs=F.norm_rhs,
               row_kind=g(F.row_kind, F.m))
    lib.pdlp_mi355x_free_prepared(C.byref(F))
    return 0, out


def _assert_replay_equals_fresh(lp, u, **options):
    rc, got = _prepare(lp, abi.UpdateHandle(**u), updatable=True, **options)
    assert rc == 0, got
    rc, want = _prepare(UC.apply(lp, u), **options)
    assert rc == 0, want
    for k in VECTORS:
        assert np.array_equal(got[k], want[k]), k
    assert got["norm_cost"] == want["norm_cost"] and got["norm_rhs"] == want["norm_rhs"]


@pytest.mark.parametrize("what", UC.KINDS)
@pytest.mark.parametrize("name", list(MAKERS))
def test_replay_equals_fresh_prepare(name, what):
    lp = _lp(name)
    _assert_replay_equals_fresh(lp, UC.modification(lp, what, seed=len(name) + 7))


def test_replay_equals_fresh_prepare_maximise():
    import copy
    lp = copy.copy(_lp("e226"))
    lp.sense = -1
    _assert_replay_equals_fresh(lp, UC.modification(lp, "all", seed=5))


@pytest.mark.parametrize("name", ["afiro", "25fv47", "random_diag_qp"])
def test_replay_equals_fresh_prepare_without_scaling(name):
    lp = _lp(name)
    _assert_replay_equals_fresh(lp, UC.modification(lp, "all", seed=11), pdlp_features_off=abi.FEATURE_SCALING_OFF)


def test_empty_update_changes_nothing():
    lp = _lp("25fv47")
    _assert_replay_equals_fresh(lp, {})


def test_one_division_by_the_accumulated_scale_is_not_the_same_bits():
    """Why the factors of every pass are kept: cost /= cs, once per pass, rounds eleven times; one division by the
    product of the factors rounds once."""
    differing = 0
    for name in ("25fv47", "e226", "stair"):
        lp = _lp(name)
        u = UC.modification(lp, "cost", seed=3)
        rc, want = _prepare(UC.apply(lp, u))
        assert rc == 0
        n0 = lp.num_col
        once = (u["col_cost"] * float(lp.sense)) / want["col_scale"][:n0]
        differing += int(np.count_nonzero(once != want["cost"][:n0]))
    assert differing > 0


# ---- refusals that need no solver handle -------------------------------------------------------------------------
def _refused(lp, u, **options):
    options.setdefault("updatable", True)
    rc, msg = _prepare(lp, u, **options)
    assert rc != 0
    return msg


def test_refuses_a_solver_not_created_for_updates():
    lp = _lp("afiro")
    msg = _refused(lp, abi.UpdateHandle(col_cost=lp.col_cost), updatable=False)
    assert "updatable" in msg


def test_refuses_hipdlp():
    lp = _lp("afiro")
    msg = _refused(lp, abi.UpdateHandle(col_cost=lp.col_cost), solver="hipdlp")
    assert "HiPDLP" in msg and "algorithm = 1" in msg


def test_refuses_one_row_bound_without_the_other():
    lp = _lp("afiro")
    assert "row_upper is NULL" in _refused(lp, abi.UpdateHandle(row_lower=lp.row_lower))
    assert "row_lower is NULL" in _refused(lp, abi.UpdateHandle(row_upper=lp.row_upper))


@pytest.mark.parametrize("given", [("col_value",), ("row_dual",), ("col_value", "row_value"), ("row_value", "row_dual")])
def test_refuses_a_partial_start(given):
    lp = _lp("afiro")
    full = dict(col_value=np.zeros(lp.num_col), row_value=np.zeros(lp.num_row), row_dual=np.zeros(lp.num_row))
    msg = _refused(lp, abi.UpdateHandle(start={k: full[k] for k in given}))
    assert "partial start" in msg and f"{len(given)} of 3" in msg


def test_refuses_null_update():
    lp = _lp("afiro")
    lib = solver.lib()
    P = abi.ProblemHandle(lp)
    params = abi.default_params(updatable=True)
    F = abi.PdlpPrepared()
    assert lib.pdlp_mi355x_host_prepare_updated(C.byref(P.struct), C.byref(params), None, C.byref(F)) != 0
    assert "null update" in lib.pdlp_mi355x_last_error().decode()
    assert lib.pdlp_mi355x_update(None, C.byref(abi.PdlpUpdate())) != 0
    assert "null solver" in lib.pdlp_mi355x_last_error().decode()


def test_refuses_a_row_kind_change_and_names_the_smallest_row():
    lp = _lp("25fv47")
    kind = UC.row_kind(np.asarray(lp.row_lower), np.asarray(lp.row_upper))
    eq = np.nonzero(kind == 0)[0]
    one_sided = np.nonzero((kind == 1) | (kind == 2))[0]
    assert eq.size >= 2 and one_sided.size >= 1
    lo, up = np.array(lp.row_lower), np.array(lp.row_upper)
    # three offenders; the smallest index must be the one reported
    rows = sorted([int(eq[-1]), int(eq[eq.size // 2]), int(one_sided[-1])])
    for i in rows:
        if kind[i] == 0:
            up[i] = lo[i] + 1.0        # equality -> ranged
        else:
            lo[i] = up[i] = 2.0        # one-sided -> equality
    msg = _refused(lp, abi.UpdateHandle(row_lower=lo, row_upper=up))
    first = rows[0]
    assert f"row {first} " in msg
    assert ("equality" in msg and "ranged or free" in msg) if kind[first] == 0 else "to equality" in msg
    # ... and the refusal comes before anything else is looked at: the same message with every other array given too
    msg2 = _refused(lp, abi.UpdateHandle(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper,
                                         row_lower=lo, row_upper=up))
    assert msg2 == msg


# ---- ABI -------------------------------------------------------------------------------------------------------
def test_abi_numbers():
    lib = solver.lib()
    assert lib.pdlp_mi355x_sizeof(8) == C.sizeof(abi.PdlpUpdate)
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(1) == C.sizeof(abi.PdlpParams) == 104
    assert abi.PdlpParams.updatable.offset == 84 and abi.PdlpParams.updatable.size == 4
    assert lib.pdlp_mi355x_sizeof(9) == -1


def test_default_params_leave_updatable_off():
    p = abi.PdlpParams()
    solver.lib().pdlp_mi355x_default_params(C.byref(p))
    assert p.updatable == 0
    assert abi.default_params().updatable == 0 and abi.default_params(updatable=True).updatable == 1
