"""pdlp_mi355x_update_values without a GPU, through its host twin pdlp_mi355x_host_prepare_qp: prepare P keeping what the
device keeps (the passes, the Hessian's assembly map, the unscaled Hessian), apply new Hessian values — alone, or with new
matrix values and data — as the device does; the result must be, bit for bit and in EVERY field of both structs, what a
plain host_prepare_qp gives on the modified problem P' built in Python with the same `updatable` bits.  Also: the pattern
contract of PDLP_UPDATABLE_HESSIAN, every refusal that needs no solver handle, and the ABI numbers this change must not
move.  No tolerance anywhere."""
import copy
import ctypes as C

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_hessian_cases as HC
from highs_amd import abi, solver

FORM_ARRAYS = ("csr_beg", "csr_idx", "csr_val", "csc_beg", "csc_idx", "csc_val", "cost", "rhs", "lower", "upper", "col_scale",
               "row_scale", "row_kind", "row_new_idx")
FORM_SCALARS = ("n", "m", "n_eqs", "n_orig", "nnz", "norm_cost", "norm_rhs", "mat_norm_inf", "spmv_blocks_ax", "spmv_blocks_aty")
HESS_ARRAYS = ("qdiag", "q_beg", "q_idx", "q_val")
HESS_SCALARS = ("n", "has_diag", "nnz_off")

# name -> (maker, the seed random_sparse_qp was made with or None)
MAKERS = {
    "random_diag_qp": (lambda: lpgen.random_diag_qp(3), None),
    "random_sparse_qp": (lambda: lpgen.random_sparse_qp(3), 3),
    "bench_qp_banded": (lambda: lpgen.bench_qp_at_scale(100, True), None),
    "bench_qp_diagonal": (lambda: lpgen.bench_qp_at_scale(100, False), None),
}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name][0]()
    return _cache[name]


def _flip_sense(lp):
    """The same problem maximised: the Hessian takes the sign with it, so that it stays PSD for the sense."""
    out = copy.copy(lp)
    out.sense = -lp.sense
    out.hessian = (lp.hessian[0], lp.hessian[1], -np.asarray(lp.hessian[2], dtype=np.float64))
    return out


def _assert_same(got, want):
    (gf, gq), (wf, wq) = got, want
    for k in FORM_ARRAYS:
        assert gf[k].shape == wf[k].shape and np.array_equal(gf[k], wf[k]), k
    for k in FORM_SCALARS:
        assert gf[k] == wf[k], (k, gf[k], wf[k])
    for k in HESS_ARRAYS:
        assert gq[k].shape == wq[k].shape and np.array_equal(gq[k], wq[k]), k
    for k in HESS_SCALARS:
        assert gq[k] == wq[k], (k, gq[k], wq[k])


def _handle(u):
    data = {k: v for k, v in u.items() if k not in ("a_value", "q_value")}
    return abi.UpdateHandle(**data) if data else None


def _updatable(u):
    return "matrix+hessian" if u.get("a_value") is not None else "hessian"


def _assert_update_equals_fresh(lp, u, **options):
    options.setdefault("updatable", _updatable(u))
    got = solver.host_prepare_qp(lp, a_value=u.get("a_value"), q_value=u.get("q_value"), update=_handle(u), **options)
    _assert_same(got, solver.host_prepare_qp(HC.apply(lp, u), **options))
    return got


def _message(lp, **kw):
    with pytest.raises(RuntimeError) as e:
        solver.host_prepare_qp(lp, **kw)
    return str(e.value)


def test_the_symbols_exist():
    """This alone fails without the feature."""
    lib = solver.lib()
    for name in ("pdlp_mi355x_update_values", "pdlp_mi355x_host_prepare_qp", "pdlp_mi355x_free_prepared_hessian"):
        assert hasattr(lib, name), name
    assert abi.UPDATABLE_HESSIAN == 4


def test_abi_numbers_stay():
    lib = solver.lib()
    lib.pdlp_mi355x_sizeof.restype = C.c_int64
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(1) == 104 == C.sizeof(abi.PdlpParams)
    assert lib.pdlp_mi355x_sizeof(8) == C.sizeof(abi.PdlpUpdate) == 80
    assert lib.pdlp_mi355x_sizeof(9) == -1


def test_updatable_values():
    assert abi.default_params(updatable="hessian").updatable == 5
    assert abi.default_params(updatable="matrix+hessian").updatable == 7
    assert abi.default_params(updatable=abi.UPDATABLE_HESSIAN).updatable == 5  # HESSIAN implies DATA
    assert abi.default_params(updatable=abi.UPDATABLE_HESSIAN | abi.UPDATABLE_MATRIX).updatable == 7
    assert abi.default_params(updatable="matrix").updatable == 3 and abi.default_params(updatable=True).updatable == 1


@pytest.mark.parametrize("what", HC.KINDS)
@pytest.mark.parametrize("name", list(MAKERS))
def test_hessian_update_equals_fresh_prepare(name, what):
    lp = _lp(name)
    _assert_update_equals_fresh(lp, HC.modification(lp, what, seed=len(name) + 7, sparse_seed=MAKERS[name][1]))


@pytest.mark.parametrize("what", ["regen", "zero_off", "all"])
@pytest.mark.parametrize("name", ["random_sparse_qp", "bench_qp_banded", "random_diag_qp"])
def test_hessian_update_equals_fresh_prepare_other_sense_and_without_scaling(name, what):
    lp = _flip_sense(_lp(name))
    u = HC.modification(lp, what, seed=31, sparse_seed=MAKERS[name][1])
    _assert_update_equals_fresh(lp, u)
    lp = _lp(name)
    u = HC.modification(lp, what, seed=32, sparse_seed=MAKERS[name][1])
    _assert_update_equals_fresh(lp, u, pdlp_features_off=abi.FEATURE_SCALING_OFF)


@pytest.mark.parametrize("name", list(MAKERS))
def test_a_hessian_only_change_leaves_the_form_alone(name):
    """The matrix factors did not move: pdlp_prepared_t is field for field that of P, and the Hessian really changed."""
    lp = _lp(name)
    u = HC.modification(lp, "regen", seed=5, sparse_seed=MAKERS[name][1])
    (form, hess) = _assert_update_equals_fresh(lp, u)
    form0, hess0 = solver.host_prepare_qp(lp, updatable="hessian")
    for k in FORM_ARRAYS:
        assert np.array_equal(form[k], form0[k]), k
    for k in FORM_SCALARS:
        assert form[k] == form0[k], k
    assert not np.array_equal(hess["qdiag"], hess0["qdiag"])
    assert np.array_equal(hess["q_idx"], hess0["q_idx"]) and np.array_equal(hess["q_beg"], hess0["q_beg"])
    if hess0["nnz_off"]:
        assert not np.array_equal(hess["q_val"], hess0["q_val"])


@pytest.mark.parametrize("with_matrix", [False, True])
def test_a_data_update_afterwards_replays_the_right_factors(with_matrix):
    """update_values, then a pdlp_mi355x_update on the same form: the kept factors (Hessian only) or the NEW ones (with
    a_value) take the new costs and bounds."""
    lp = _lp("random_sparse_qp")
    u = HC.modification(lp, "all" if with_matrix else "regen", seed=41, sparse_seed=3)
    lp2 = HC.apply(lp, u)
    then = UC.modification(lp2, "all", seed=42)
    then.pop("start", None)
    bits = _updatable(u)
    got = solver.host_prepare_qp(lp, a_value=u.get("a_value"), q_value=u["q_value"], update=_handle(u),
                                 update_then=abi.UpdateHandle(**then), updatable=bits)
    _assert_same(got, solver.host_prepare_qp(UC.apply(lp2, then), updatable=bits))


def _pattern_lp():
    """4 columns; the Hessian's lower triangle with an explicit zero at (2, 0), the pair (3, 1) twice and the diagonal
    entry (1, 1) twice."""
    lp = copy.copy(lpgen.random_diag_qp(3, m=3, n=4))
    assert lp.num_col == 4
    st = np.array([0, 3, 7, 8, 9], np.int32)
    idx = np.array([0, 1, 2, 1, 3, 1, 3, 2, 3], np.int32)
    val = lp.sense * np.array([2.0, 0.25, 0.0, 1.0, 0.125, 0.5, 0.0625, 1.5, 1.0])
    lp.hessian = (st, idx, val)
    return lp


def test_the_pattern_contract():
    lp = _pattern_lp()
    _, kept = solver.host_prepare_qp(lp, updatable="hessian", pdlp_features_off=abi.FEATURE_SCALING_OFF)
    _, plain = solver.host_prepare_qp(lp, pdlp_features_off=abi.FEATURE_SCALING_OFF)
    # (the form holds Q times the sense; the caller's values carry the sense too, so the products are the numbers below)
    for h in (kept, plain):  # (slack columns behind the four original ones: empty rows, zero diagonal)
        assert np.all(h["q_beg"][4:] == h["nnz_off"]) and not h["qdiag"][4:].any()
        h["q_beg"], h["qdiag"] = h["q_beg"][:5], h["qdiag"][:4]
    # kept: (1,0) (2,0) (3,1) and their mirrors -> 6 slots, the zero among them; the repeated pair is one slot
    assert kept["nnz_off"] == 6 and kept["q_beg"].tolist() == [0, 2, 4, 5, 6]
    assert kept["q_idx"].tolist() == [1, 2, 0, 3, 0, 1]
    assert np.array_equal(kept["q_val"], [0.25, 0.0, 0.25, 0.125 + 0.0625, 0.0, 0.125 + 0.0625])
    assert np.array_equal(kept["qdiag"], [2.0, 1.5, 1.5, 1.0])  # (1, 1): 0.0 + 1.0 + 0.5, in caller order
    # without the bit the zero is dropped and the pair summed, as always
    assert plain["nnz_off"] == 4 and plain["q_beg"].tolist() == [0, 1, 3, 3, 4]
    assert plain["q_idx"].tolist() == [1, 0, 3, 1]
    assert np.array_equal(plain["q_val"], [0.25, 0.25, 0.1875, 0.1875])
    assert np.array_equal(plain["qdiag"], kept["qdiag"])
    # new values on the kept pattern fill the zero's slot; the sums keep create's order
    q = lp.sense * np.array([3.0, 0.5, 0.75, 0.1, 0.3, 0.2, 0.6, 2.0, 1.25])
    _assert_update_equals_fresh(lp, dict(q_value=q))
    _assert_update_equals_fresh(lp, dict(q_value=q), pdlp_features_off=abi.FEATURE_SCALING_OFF)
    _, new = solver.host_prepare_qp(lp, q_value=q, updatable="hessian", pdlp_features_off=abi.FEATURE_SCALING_OFF)
    assert np.array_equal(new["q_val"], [0.5, 0.75, 0.5, 0.3 + 0.6, 0.75, 0.3 + 0.6])
    assert np.array_equal(new["qdiag"][:4], [3.0, (0.0 + 0.1) + 0.2, 2.0, 1.25])


def test_an_all_zero_hessian_keeps_its_structure_under_the_bit_only():
    lp = copy.copy(_lp("random_sparse_qp"))
    lp.hessian = (lp.hessian[0], lp.hessian[1], np.zeros(len(lp.hessian[2])))
    _, kept = solver.host_prepare_qp(lp, updatable="hessian")
    _, plain = solver.host_prepare_qp(lp)
    assert kept["has_diag"] == 1 and kept["nnz_off"] > 0 and not kept["q_val"].any()
    assert plain["has_diag"] == 0 and plain["nnz_off"] == 0


def test_without_explicit_zeros_the_bit_changes_nothing():
    for name in ("random_sparse_qp", "bench_qp_banded"):
        lp = _lp(name)
        assert np.all(np.asarray(lp.hessian[2]) != 0.0)
        _assert_same(solver.host_prepare_qp(lp, updatable="hessian"), solver.host_prepare_qp(lp))


def test_refusals():
    lp = _lp("random_sparse_qp")
    q = np.array(lp.hessian[2], dtype=np.float64)
    a = np.array(lp.a_value, dtype=np.float64)
    msg = _message(lp, q_value=q, updatable="matrix")
    assert "pdlp_mi355x_update_values" in msg and "PDLP_UPDATABLE_HESSIAN" in msg
    msg = _message(lp, q_value=q)
    assert "PDLP_UPDATABLE_HESSIAN" in msg
    msg = _message(lp, a_value=a, q_value=q, updatable="hessian")
    assert "a_value" in msg and "PDLP_UPDATABLE_MATRIX" in msg
    msg = _message(lp, q_value=q, updatable="hessian", solver="hipdlp")
    assert "HiPDLP" in msg and "do not take updates" in msg
    plain_lp = lpgen.random_lp(5)
    msg = _message(plain_lp, q_value=np.ones(3), updatable="hessian")
    assert "created without a Hessian" in msg
    # what update / update_matrix refuse for u and a_value
    n, m = lp.num_col, lp.num_row
    msg = _message(lp, q_value=q, update=abi.UpdateHandle(row_lower=np.zeros(m)), updatable="hessian")
    assert "row_lower and row_upper are given together" in msg
    msg = _message(lp, q_value=q, update=abi.UpdateHandle(start=dict(col_value=np.zeros(n))), updatable="hessian")
    assert "partial start" in msg
    kinds = UC.row_kind(lp.row_lower, lp.row_upper)
    i = int(np.nonzero(kinds != UC.row_kind(np.full(m, -np.inf), lp.row_upper))[0][0])
    lo = np.array(lp.row_lower); lo[i] = -np.inf
    up = np.array(lp.row_upper); up[i] = 1.0 if not np.isfinite(up[i]) else up[i]
    msg = _message(lp, q_value=q, update=abi.UpdateHandle(row_lower=lo, row_upper=up), updatable="hessian")
    assert f"row {i} would change its kind" in msg
    msg = _message(lp, a_value=np.zeros(a.size), q_value=q, updatable="matrix+hessian")
    assert "no matrix nonzeros" in msg


def test_refusal_precedence():
    """Doubly wrong updates: row kind before all-zero matrix before Hessian diagonal (tests/update_hessian_cases.py
    doubly_wrong names the expected words)."""
    lp = _lp("random_sparse_qp")
    for name, (u, words) in HC.doubly_wrong(lp).items():
        msg = _message(lp, a_value=u.get("a_value"), q_value=u.get("q_value"), update=_handle(u), updatable="matrix+hessian")
        assert words in msg, (name, msg)


@pytest.mark.parametrize("with_matrix", [False, True])
def test_a_negative_diagonal_names_the_smallest_column(with_matrix):
    lp = _lp("random_sparse_qp")
    st, idx, val = lp.hessian
    cols = np.repeat(np.arange(len(st) - 1), np.diff(st))
    diag = np.nonzero(np.asarray(idx) == cols)[0]
    assert diag.size >= 3
    q = np.array(val, dtype=np.float64)
    for p in (diag[-1], diag[2]):  # two columns: the smaller one is named
        q[p] = -lp.sense * 0.5
    a = np.array(lp.a_value) if with_matrix else None
    msg = _message(lp, a_value=a, q_value=q, updatable="matrix+hessian")
    assert "not positive semidefinite for this objective sense" in msg
    assert f"column {int(cols[diag[2]])} " in msg
    # the other sense: the same values are fine for the diagonal's sign there
    other = _flip_sense(lp)
    msg = _message(other, q_value=np.array(val, dtype=np.float64), updatable="hessian")
    assert "not positive semidefinite" in msg
