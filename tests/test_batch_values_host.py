"""pdlp_mi355x_batch_run_values without a GPU: the size of pdlp_variant_t, and the refusals that look at no matrix or
Hessian value — each with the exact words of the update entry its variant maps to behind "variant k: " — through the
library's host twin of the validation (no device call is made), and the batch driver with value variants behind canned
lanes under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_values_cases as BC
from highs_amd import abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refusal(name, updatable, variants, K=None, null_variants=False, null_results=False):
    """-> (return code, message) of validating `variants` (dicts as DeviceBatch.run takes them) for a batch on lp `name`"""
    lp = BC.lp(name)
    P = abi.ProblemHandle(lp)
    params = abi.default_params(**({} if updatable is None else dict(updatable=updatable)))
    handles = [abi.VariantHandle(**v) for v in variants]
    V = (abi.PdlpVariant * max(len(handles), 1))()
    for k, h in enumerate(handles):
        V[k] = h.struct
    R = (abi.PdlpResult * max(len(handles), 1))()
    rc = solver.lib().pdlp_mi355x_host_batch_variants_refusal(
        C.byref(P.struct), C.byref(params), len(handles) if K is None else K, None if null_variants else V, None if null_results else R)
    return rc, solver.lib().pdlp_mi355x_last_error().decode()


def _a(name):
    return np.array(BC.lp(name).a_value, dtype=np.float64)


def _q(name):
    return np.array(BC.lp(name).hessian[2], dtype=np.float64)


def test_symbols_and_the_size_of_a_variant():
    lib = solver.lib()
    assert hasattr(lib, "pdlp_mi355x_batch_run_values")
    assert lib.pdlp_mi355x_variant_size() == C.sizeof(abi.PdlpVariant) == 32 + C.sizeof(abi.PdlpUpdate)
    assert lib.pdlp_mi355x_sizeof(9) == -1  # (pdlp_mi355x_sizeof keeps its indices)


def test_null_arguments_and_no_variants():
    lib = solver.lib()
    assert lib.pdlp_mi355x_batch_run_values(None, 1, None, None) != 0
    assert lib.pdlp_mi355x_last_error().decode() == "pdlp_mi355x_batch_run_values: null batch"
    for K in (0, -2):
        rc, msg = _refusal("afiro", "matrix", [{}], K=K)
        assert rc != 0 and msg == "pdlp_mi355x_batch_run_values: K = %d variants (at least 1)" % K
    for nulls in (dict(null_variants=True), dict(null_results=True)):
        rc, msg = _refusal("afiro", "matrix", [{}], **nulls)
        assert rc != 0 and msg == "pdlp_mi355x_batch_run_values: null argument"


def test_valid_lists_are_not_refused():
    assert _refusal("afiro", None, [{}, dict(col_cost=BC.lp("afiro").col_cost)])[0] == 0
    assert _refusal("afiro", "matrix", [{}, dict(a_value=_a("afiro"))])[0] == 0
    assert _refusal("qp0", "matrix", [dict(a_value=_a("qp0"))])[0] == 0
    assert _refusal("sq100", "matrix+hessian", [dict(a_value=_a("sq100")), dict(q_value=_q("sq100")),
                                                dict(a_value=_a("sq100"), q_value=_q("sq100"))])[0] == 0
    assert _refusal("sq100", "hessian", [dict(q_value=_q("sq100"))])[0] == 0


MATRIX_BIT = "the solver was not created for matrix updates (pdlp_params_t.updatable lacks PDLP_UPDATABLE_MATRIX)"
HESSIAN_BIT = "the solver was not created for Hessian updates (pdlp_params_t.updatable lacks PDLP_UPDATABLE_HESSIAN)"
FIXED = "(the sparsity pattern is fixed: create a new solver)"


def _cases():
    a, q = _a("sq100"), _q("sq100")
    lo, up = np.array(BC.lp("afiro").row_lower, dtype=np.float64), np.array(BC.lp("afiro").row_upper, dtype=np.float64)
    i = int(np.nonzero(lo == up)[0][0])  # an equality row becomes a <= row
    lo[i] = -np.inf
    return {
        # a_value on a batch without the matrix bit: update_matrix's words without the Hessian bit, update_values' with it
        "no matrix bit": ("afiro", None, [{}, dict(a_value=_a("afiro"))], "variant 1: pdlp_mi355x_update_matrix: " + MATRIX_BIT),
        "no matrix bit, hessian": ("sq100", "hessian", [dict(a_value=a)],
                                   "variant 0: pdlp_mi355x_update_values: a_value given, but " + MATRIX_BIT),
        "no hessian bit": ("sq100", None, [{}, {}, dict(q_value=q)], "variant 2: pdlp_mi355x_update_values: " + HESSIAN_BIT),
        "no hessian bit, both": ("qp0", "matrix", [dict(a_value=_a("qp0"), q_value=_q("qp0"))],
                                 "variant 0: pdlp_mi355x_update_values: " + HESSIAN_BIT),
        "wrong num_nz, matrix": ("afiro", "matrix", [dict(a_value=_a("afiro")[:-1])],
                                 "variant 0: pdlp_mi355x_update_matrix: num_nz = %d differs from the %d nonzeros the solver was "
                                 "created with %s" % (len(_a("afiro")) - 1, len(_a("afiro")), FIXED)),
        "wrong num_nz, values": ("sq100", "matrix+hessian", [dict(q_value=q), dict(a_value=a[:-2], q_value=q)],
                                 "variant 1: pdlp_mi355x_update_matrix: num_nz = %d differs from the %d nonzeros the solver was "
                                 "created with %s" % (len(a) - 2, len(a), FIXED)),
        "wrong num_q_nz": ("sq100", "matrix+hessian", [dict(a_value=a, q_value=q[:-1])],
                           "variant 0: pdlp_mi355x_update_values: num_q_nz = %d differs from the %d Hessian slots the solver was "
                           "created with %s" % (len(q) - 1, len(q), FIXED)),
        "no hessian": ("afiro", "matrix+hessian", [dict(q_value=np.ones(3))],
                       "variant 0: pdlp_mi355x_update_values: q_value given to a solver that was created without a Hessian " + FIXED),
        "off-diagonal, matrix bit alone": (
            "sq100", "matrix", [dict(a_value=a)],
            "variant 0: pdlp_mi355x_update_matrix: QPs whose Hessian has off-diagonal entries do not take matrix updates (the "
            "scaled copy of the Hessian follows the column factors; left for a later change)"),
        "kind change": ("afiro", "matrix", [dict(a_value=_a("afiro")), dict(a_value=_a("afiro"), row_lower=lo, row_upper=up)],
                        "variant 1: pdlp_mi355x_update: row %d would change its kind from equality to <= (upper bound only) (the "
                        "kind decides row order, slack columns and signs: create a new solver)" % i),
        "kind change, no values": ("afiro", "matrix", [dict(row_lower=lo, row_upper=up)],
                                   "variant 0: pdlp_mi355x_update: row %d would change its kind from equality to <= (upper bound only) "
                                   "(the kind decides row order, slack columns and signs: create a new solver)" % i),
        "half a pair of row bounds": ("sq100", "matrix+hessian", [dict(q_value=q, row_lower=BC.lp("sq100").row_lower)],
                                      "variant 0: pdlp_mi355x_update: row_lower and row_upper are given together or not at all "
                                      "(row_upper is NULL)"),
    }


@pytest.mark.parametrize("case", sorted(_cases()))
def test_value_free_refusals_by_their_words(case):
    name, updatable, variants, words = _cases()[case]
    rc, msg = _refusal(name, updatable, variants)
    assert rc != 0
    assert msg == words


def test_a_count_without_its_array_is_refused():
    """a_value is NULL but num_nz = 5: what no VariantHandle makes, so the struct is filled by hand"""
    lp = BC.lp("sq100")
    P = abi.ProblemHandle(lp)
    params = abi.default_params(updatable="matrix+hessian")
    keep = abi.VariantHandle(q_value=_q("sq100"))
    V = (abi.PdlpVariant * 2)()
    V[1] = keep.struct
    V[1].num_nz = 5
    R = (abi.PdlpResult * 2)()
    lib = solver.lib()
    assert lib.pdlp_mi355x_host_batch_variants_refusal(C.byref(P.struct), C.byref(params), 2, V, R) != 0
    assert lib.pdlp_mi355x_last_error().decode() == "variant 1: pdlp_mi355x_update_values: a_value is NULL but num_nz = 5"
    V[1] = abi.PdlpVariant()
    V[1].num_q_nz = 7  # neither array, but a count: update_values' refusal, not a silent plain update
    assert lib.pdlp_mi355x_host_batch_variants_refusal(C.byref(P.struct), C.byref(params), 2, V, R) != 0
    assert lib.pdlp_mi355x_last_error().decode() == "variant 1: pdlp_mi355x_update_values: q_value is NULL but num_q_nz = 7"


def test_driver_with_value_variants_behind_canned_lanes_under_sanitizers(tmp_path):
    """Value variants, every restore transition (a lane's "solver" follows whose arrays it holds), a value update that
    throws in the middle of a run and a lane that stops qualifying, in the driver (csrc/pdlp_batch.cpp) with canned
    lanes: a host program of its own, never loaded into Python."""
    env = dict(os.environ, OUT=str(tmp_path / "batch_driver_check"))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "batch_driver_check.sh")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all scenarios passed" in r.stdout
    assert "[AnQnBDQn]" in r.stdout and "value updates" in r.stdout
