"""Variants of one problem that change matrix and Hessian VALUES (pdlp_mi355x_batch_run_values), and their references, for
tests/test_batch_values_host.py and tests/test_gpu_batch_values.py (a helper, not a conftest).

A variant is (tag, dict): the dict is what DeviceBatch.run takes — a_value=, q_value=, DeviceSolver.update's arguments,
iter_limit= —, the tag names it in the shared cache of references.  The reference of a variant is code that exists
without the batches' value variants: ONE held DeviceSolver of its own, created on P with the batch's `updatable`, brought
to the variant by update_values / update_matrix / update with P's arrays filled in where the variant gives none (so that
it would hold the variant whatever it held before), then run."""
import os

import numpy as np

import qp_small_cases as QC
import update_cases as UC
import update_hessian_cases as HC
import update_matrix_cases as MC
from highs_amd import lp as L
from highs_amd import solver

GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "term_iterate", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
_lps, _refs = {}, {}


def lp(name):
    if name not in _lps:
        if name == "portfolio64":
            _lps[name] = QC.portfolio()
        else:
            sub = "qp" if name.startswith(("qp", "sq")) else "instances"
            _lps[name] = L.HighsLp.from_npz(os.path.join(GOLD, sub, name + ".npz"))
    return _lps[name]


def matrix(name, what, seed):
    """(tag, variant) with new matrix values: update_matrix_cases.modification ("all" brings new data along)."""
    return "A:%s%d" % (what, seed), MC.modification(lp(name), what, seed)


def hessian(name, what, seed=0):
    """(tag, variant) with new Hessian values: update_hessian_cases.new_values ("scale<f>" — a risk-aversion sweep —, "regen")."""
    return "Q:%s/%d" % (what, seed), dict(q_value=HC.new_values(lp(name), what, seed))


def both(name, what_a, what_q, seed):
    (ta, va), (tq, vq) = matrix(name, what_a, seed), hessian(name, what_q, seed + 1)
    return ta + "+" + tq, dict(va, **vq)


def data(name, what, seed):
    return "D:%s%d" % (what, seed), UC.modification(lp(name), what, seed)


NOTHING = ("P", {})


def has_values(v):
    return v.get("a_value") is not None or v.get("q_value") is not None


def reference(name, updatable, tagged, env=""):
    """(result, persistent launches of the run) of the variant's solo solve; computed once, shared, never changed.  env
    names the environment switches the caller has set (they are read at create)."""
    tag, v = tagged
    key = (name, updatable, tag, env)
    if key not in _refs:
        P = lp(name)
        v = dict(v)
        limit = v.pop("iter_limit", None)
        options = dict(OPTIONS) if limit is None else dict(OPTIONS, pdlp_iteration_limit=limit)
        parts = updatable.split("+") if isinstance(updatable, str) else []
        a, q = v.pop("a_value", None), v.pop("q_value", None)
        full = dict(col_cost=P.col_cost, col_lower=P.col_lower, col_upper=P.col_upper, row_lower=P.row_lower,
                    row_upper=P.row_upper, offset=P.offset)
        full.update(v)
        held = solver.DeviceSolver(P, updatable=updatable, **options)
        if "matrix" in parts and a is None:
            a = P.a_value
        if "hessian" in parts and q is None and getattr(P, "hessian", None) is not None:
            q = P.hessian[2]
        if "hessian" in parts:
            held.update_values(a_value=a, q_value=q, **full)
        elif "matrix" in parts:
            held.update_matrix(a, **full)
        else:
            held.update(**full)
        before = held.stage("persistent_launches", 1)[0]
        R = held.run(P.num_col, P.num_row)
        _refs[key] = (R, int(held.stage("persistent_launches", 1)[0] - before))
        held.close()
    return _refs[key]


def same_result(got, want):
    """None, or the first field in which two results differ."""
    for k in SOLUTION:
        if not np.array_equal(getattr(got, k), getattr(want, k)):
            return k
    for k in COUNTS + SCALARS:
        if getattr(got, k) != getattr(want, k):
            return "%s: %r != %r" % (k, getattr(got, k), getattr(want, k))
    return None


def really_differs(R, P):
    """A value variant must change the solve: another iteration count or other primal values than P's own."""
    return R.num_iter != P.num_iter or not np.array_equal(R.col_value, P.col_value)
