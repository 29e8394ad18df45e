"""The Hessian's extraction without a GPU.  (1) The sort-based restatement the device follows (tests/hessian_restated.py: heads
then tails, two stable sorts, runs) gives what the host walk gives — pdlp_mi355x_host_prepare_qp's q_beg, q_idx, q_val and
qdiag, == on bit patterns, with scaling off so that the values are the assembled ones — on every problem of
tests/hessian_extraction_cases.py, for a plain and a Hessian-updatable solver and for both objective senses.  (2) The rule
that decides where the extraction runs (csrc/pdlp_setup.hpp hessianExtractionReason, through its host-only hook).  (3) The
makers sit on the edges they claim, and every refusal is the walk's."""
import copy

import numpy as np
import pytest

import hessian_extraction_cases as XC
import hessian_restated as HR
from highs_amd import abi, solver

MODES = {"plain": {}, "kept": dict(updatable="hessian")}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = XC.CASES[name]()
    return _cache[name]


def _flipped(lp):
    """The same Q for the other objective sense: the values change sign with it."""
    out = copy.copy(lp)
    out.sense = -lp.sense
    out.hessian = (lp.hessian[0], lp.hessian[1], -np.asarray(lp.hessian[2]))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("flip", [False, True], ids=["sense_as_made", "sense_flipped"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(XC.CASES))
def test_sorting_restates_the_host_walk(name, mode, flip):
    lp = _flipped(_lp(name)) if flip else _lp(name)
    form, hess = solver.host_prepare_qp(lp, pdlp_features_off=abi.FEATURE_SCALING_OFF, **MODES[mode])
    R = HR.extraction(lp, form["n"], kept=mode == "kept")
    has_diag = R["taken"] > 0 if mode == "plain" else XC.caller_slots(lp) > 0
    assert hess["has_diag"] == int(has_diag) and hess["nnz_off"] == R["n_off"]
    if has_diag:
        assert np.array_equal(bits(hess["qdiag"]), bits(R["qdiag"]))
    if R["n_off"]:
        assert np.array_equal(hess["q_beg"], R["q_beg"])
        assert np.array_equal(hess["q_idx"], R["off_col"])
        assert np.array_equal(bits(hess["q_val"]), bits(R["q_val"]))
        # the map is consistent with itself: rows ascending, columns ascending inside a row, no pair twice
        key = R["off_row"] * form["n"] + R["off_col"]
        assert np.all(np.diff(key) > 0)
    assert len(R["dst_beg"]) == form["n"] + R["n_off"] + 1 and R["dst_beg"][-1] == len(R["src_slot"])


def test_the_restatement_is_not_trivially_right():
    """Repeated pairs are summed in slot order, and the order matters to the bits: the triple pair's sum differs from the sum
    of the same three values taken from the right."""
    lp = _lp("triple_pair")
    R = HR.extraction(lp, lp.num_col, kept=False)
    k = int(np.nonzero((R["off_row"] == 5) & (R["off_col"] == 1))[0][0])
    src = R["src_slot"][R["dst_beg"][lp.num_col + k]:R["dst_beg"][lp.num_col + k + 1]]
    assert len(src) == 3 and np.all(np.diff(src) > 0)
    v = np.asarray(lp.hessian[2])[src] * lp.sense
    assert R["q_val"][k] == (v[0] + v[1]) + v[2]
    # its mirror image (1, 5) has the same sources in the same order
    k2 = int(np.nonzero((R["off_row"] == 1) & (R["off_col"] == 5))[0][0])
    assert np.array_equal(R["src_slot"][R["dst_beg"][lp.num_col + k2]:R["dst_beg"][lp.num_col + k2 + 1]], src)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
GOOD = [0, 2, 2, 5]


@pytest.mark.parametrize("kw,q_start,reason", [
    (dict(), GOOD, "on_device"),
    (dict(gpu_setup=False), GOOD, "host_setup"),
    (dict(sharded=True), GOOD, "sharded"),
    (dict(hipdlp=True), GOOD, "hipdlp"),
    (dict(), None, "no_slots"),
    (dict(), [0], "no_slots"),            # q_dim = 0
    (dict(), [0, 0, 0], "no_slots"),      # columns, but no slot
    (dict(), [1, 2, 3], "q_start"),       # does not begin at 0
    (dict(), [0, 2, 1, 3], "q_start"),    # decreases once
    (dict(), [0, 3, 3, 2], "q_start"),    # ... at its end
    (dict(switch_on=False), GOOD, "switched_off"),
    # the order of the tests: the host set-up, sharding and HiPDLP come before anything about the Hessian, the switch last
    (dict(gpu_setup=False, sharded=True, switch_on=False), [0, 2, 1, 3], "host_setup"),
    (dict(sharded=True, hipdlp=True, switch_on=False), None, "sharded"),
    (dict(switch_on=False), [0, 2, 1, 3], "q_start"),
    (dict(switch_on=False), [0, 0], "no_slots"),
])
def test_rule(kw, q_start, reason):
    assert solver.hessian_extraction_rule(q_start, **kw) == reason


def test_rule_on_the_cases():
    for name in XC.CASES:
        assert solver.hessian_extraction_rule(_lp(name).hessian[0]) == "on_device", name
    assert solver.hessian_extraction_rule(XC.decreasing_start_qp().hessian[0]) == "q_start"


# ---- the makers ------------------------------------------------------------------------------------------------------------------
def test_slot_counts_straddle_one_block():
    assert [XC.caller_slots(_lp(k)) for k in ("tridiagonal_128", "slots_256", "tridiagonal_129")] == [XC.BLOCK - 1, XC.BLOCK, XC.BLOCK + 1]
    lp = _lp("large_tridiagonal")
    assert HR.extraction(lp, lp.num_col, kept=False)["n_off"] == 2 * (lp.num_col - 1) >= 79_998  # sort entries: several sort blocks


def test_new_cases_hold_what_they_claim():
    n = XC.NUM_COL
    plain = {k: HR.extraction(_lp(k), n, kept=False) for k in XC.NEW_CASES if k != "slots_256"}
    kept = {k: HR.extraction(_lp(k), n, kept=True) for k in plain}
    st, idx, _ = _lp("triple_pair").hessian
    assert idx[st[1] + 1:st[2]].tolist() == [9, 5, 7, 5, 4, 5, 2]
    assert plain["diagonal_only"]["n_off"] == 0 and plain["diagonal_only"]["taken"] == n
    assert plain["off_diagonal_only"]["taken"] * 2 == plain["off_diagonal_only"]["n_off"] == 8 and not plain["off_diagonal_only"]["qdiag"].any()
    assert plain["all_zero"]["taken"] == 0 and kept["all_zero"]["n_off"] == 14 and kept["all_zero"]["taken"] == XC.caller_slots(_lp("all_zero"))
    val = np.asarray(_lp("negative_zero").hessian[2])
    assert np.sum(np.signbit(val) & (val == 0.0)) == 2
    assert kept["negative_zero"]["n_off"] == plain["negative_zero"]["n_off"] + 2
    st = _lp("empty_border_columns").hessian[0]
    assert st[1] == st[0] and st[-1] == st[-2] and plain["empty_border_columns"]["n_off"] > 0


def test_decreasing_start_is_accepted_by_the_walk():
    lp = XC.decreasing_start_qp()
    for mode in MODES.values():
        _, hess = solver.host_prepare_qp(lp, pdlp_features_off=abi.FEATURE_SCALING_OFF, **mode)
        assert hess["nnz_off"] == 2 and hess["q_idx"].tolist() == [2, 0]
        assert hess["qdiag"][:3].tolist() == [1.0, 0.0, 1.3]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("what", sorted(XC.REFUSALS))
def test_refusals_of_the_walk(what, mode):
    make, words, modes = XC.REFUSALS[what]
    if mode in modes:
        with pytest.raises(RuntimeError) as e:
            solver.host_prepare_qp(make(), **MODES[mode])
        assert words in str(e.value)
    else:
        _, hess = solver.host_prepare_qp(make(), **MODES[mode])
        assert hess["nnz_off"] > 0
