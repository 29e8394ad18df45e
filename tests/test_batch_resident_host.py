"""pdlp_mi355x_batch_run_device without a GPU: the symbol and what it must not move (ABI version, pdlp_mi355x_sizeof), the
refusals that need no device — in refuseBatchArguments' words and, per variant, in the words the host batch gives for the
same list —, the verdict the entry makes of the validation launch's records, on canned records, what run_tensors and
tensors.stacked check in Python, and the batch driver behind canned lanes in device mode under AddressSanitizer + UBSan as
a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_values_cases as BC
from highs_amd import abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pdlp_mi355x_batch_run_device"


def _structs(variants):
    handles = [abi.VariantHandle(**v) for v in variants]
    V = (abi.PdlpVariant * max(len(handles), 1))()
    for k, h in enumerate(handles):
        V[k] = h.struct
    return V, handles


def _refusal(hook, name, updatable, variants, K=None, null_variants=False, null_results=False):
    """-> (return code, message) of `hook` (the host batch's restatement or the device batch's) for a batch on lp `name`"""
    P = abi.ProblemHandle(BC.lp(name))
    params = abi.default_params(**({} if updatable is None else dict(updatable=updatable)))
    V, keep = _structs(variants)
    R = (abi.PdlpResult * max(len(variants), 1))()
    rc = getattr(solver.lib(), hook)(C.byref(P.struct), C.byref(params), len(variants) if K is None else K,
                                     None if null_variants else V, None if null_results else R)
    return rc, solver.lib().pdlp_mi355x_last_error().decode()


HOST, DEVICE = "pdlp_mi355x_host_batch_variants_refusal", "pdlp_mi355x_host_batch_device_variants_refusal"


def _a(name):
    return np.array(BC.lp(name).a_value, dtype=np.float64)


def _q(name):
    return np.array(BC.lp(name).hessian[2], dtype=np.float64)


def test_the_symbol_is_exported_and_moves_nothing():
    lib = solver.lib()
    assert hasattr(lib, ENTRY) and ENTRY in solver.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "pdlp_mi355x.h")).read()
    assert re.search(r"\bint %s\(pdlp_mi355x_batch_t\* B, int32_t K, const pdlp_variant_t\* v_dev, pdlp_result_t\* R_dev,\s*void\* stream\);"
                     % ENTRY, hdr)
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(9) == -1  # (no new struct, no new index)
    assert lib.pdlp_mi355x_variant_size() == C.sizeof(abi.PdlpVariant)


def test_null_arguments_and_no_variants_in_the_entrys_words():
    lib = solver.lib()
    V, R = (abi.PdlpVariant * 1)(), (abi.PdlpResult * 1)()
    # the arguments come before the handle: no batch exists on a machine without a device
    for K in (0, -2):
        assert lib.pdlp_mi355x_batch_run_device(None, K, V, R, None) != 0
        assert lib.pdlp_mi355x_last_error().decode() == ENTRY + ": K = %d variants (at least 1)" % K
        rc, msg = _refusal(DEVICE, "afiro", "matrix", [{}], K=K)
        assert rc != 0 and msg == ENTRY + ": K = %d variants (at least 1)" % K
    for v, r in ((None, R), (V, None)):
        assert lib.pdlp_mi355x_batch_run_device(None, 1, v, r, None) != 0
        assert lib.pdlp_mi355x_last_error().decode() == ENTRY + ": null argument"
    for nulls in (dict(null_variants=True), dict(null_results=True)):
        rc, msg = _refusal(DEVICE, "afiro", "matrix", [{}], **nulls)
        assert rc != 0 and msg == ENTRY + ": null argument"
    assert lib.pdlp_mi355x_batch_run_device(None, 1, V, R, None) != 0
    assert lib.pdlp_mi355x_last_error().decode() == ENTRY + ": null batch"


def _lists():
    a, q = _a("sq100"), _q("sq100")
    fa = _a("afiro")
    return {
        "valid data": ("afiro", None, [{}, dict(col_cost=BC.lp("afiro").col_cost)]),
        "valid values": ("sq100", "matrix+hessian", [dict(a_value=a), dict(q_value=q), dict(a_value=a, q_value=q)]),
        "no matrix bit": ("afiro", None, [{}, dict(a_value=fa)]),
        "no matrix bit, hessian": ("sq100", "hessian", [dict(a_value=a)]),
        "no hessian bit": ("sq100", None, [{}, {}, dict(q_value=q)]),
        "no hessian bit, both": ("qp0", "matrix", [dict(a_value=_a("qp0"), q_value=_q("qp0"))]),
        "wrong num_nz, matrix": ("afiro", "matrix", [dict(a_value=fa[:-1])]),
        "wrong num_nz, values": ("sq100", "matrix+hessian", [dict(q_value=q), dict(a_value=a[:-2], q_value=q)]),
        "wrong num_q_nz": ("sq100", "matrix+hessian", [dict(a_value=a, q_value=q[:-1])]),
        "no hessian": ("afiro", "matrix+hessian", [dict(q_value=np.ones(3))]),
        "off-diagonal, matrix bit alone": ("sq100", "matrix", [dict(a_value=a)]),
        "half a pair of row bounds": ("sq100", "matrix+hessian", [dict(q_value=q, row_lower=BC.lp("sq100").row_lower)]),
        "partial start": ("afiro", None, [{}, dict(start=dict(col_value=np.zeros(BC.lp("afiro").num_col)))]),
        # two offenders: the first one is named
        "first of two": ("afiro", "matrix", [dict(a_value=fa), dict(a_value=fa[:-1]), {}, dict(q_value=np.ones(3))]),
        "first of two, other order": ("afiro", "matrix", [dict(q_value=np.ones(3)), dict(a_value=fa[:-1])]),
    }


@pytest.mark.parametrize("case", sorted(_lists()))
def test_value_free_refusals_are_the_host_batchs(case):
    """Step 1 gives "variant k: " + the words pdlp_mi355x_host_batch_variants_refusal gives for the same list (none of
    these lists changes a row's kind: that is the one refusal the host batch can read off the arrays and step 1 cannot)."""
    name, updatable, variants = _lists()[case]
    want = _refusal(HOST, name, updatable, variants)
    got = _refusal(DEVICE, name, updatable, variants)
    assert (got[0] != 0) == (want[0] != 0)
    if want[0] != 0:
        assert got[1] == want[1] and re.match(r"variant \d+: pdlp_mi355x_update", got[1])
    assert (want[0] != 0) == (not case.startswith("valid"))


def test_the_first_offending_variant_wins():
    fa = _a("afiro")
    rc, msg = _refusal(DEVICE, "afiro", "matrix", [dict(a_value=fa), dict(a_value=fa[:-1]), {}, dict(q_value=np.ones(3))])
    assert rc != 0 and msg.startswith("variant 1: pdlp_mi355x_update_matrix: num_nz = ")
    rc, msg = _refusal(DEVICE, "afiro", "matrix", [dict(q_value=np.ones(3)), dict(a_value=fa[:-1])])
    assert rc != 0 and msg.startswith("variant 0: pdlp_mi355x_update_values: ")


def test_step_one_reads_no_array():
    """A kind change is in the arrays: step 1 lets it pass (the device's launch finds it), the host batch refuses it."""
    lp = BC.lp("afiro")
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    lo[int(np.nonzero(lo == up)[0][0])] = -np.inf
    assert _refusal(HOST, "afiro", None, [dict(row_lower=lo, row_upper=up)])[0] != 0
    assert _refusal(DEVICE, "afiro", None, [dict(row_lower=lo, row_upper=up)])[0] == 0


# ---- the verdict on canned records ---------------------------------------------------------------------------------------
M, N = 6, 5
KIND = np.array([0, 1, 2, 3, 0, 1], dtype=np.int32)  # pdlp_host.hpp: equality, <=, >=, ranged or free
KIND_WORDS = "(the kind decides row order, slack columns and signs: create a new solver)"
ZERO = ("pdlp_mi355x: the LP has no rows, no columns or no matrix nonzeros — HiGHS solves such LPs itself "
        "(solveUnconstrainedLp) before the PDLP path")
NEG = ("pdlp_mi355x_update_values: the Hessian is not positive semidefinite for this objective sense (the diagonal entry of "
       "column %d is negative)")


def _verdict(variants, records):
    V, keep = _structs(variants)
    rec = np.array(records, dtype=np.int32).reshape(-1)
    assert rec.size == 3 * len(variants)
    rc = solver.lib().pdlp_mi355x_host_batch_records_verdict(
        len(variants), V, rec.ctypes.data_as(abi.c_i32p), KIND.ctypes.data_as(abi.c_i32p), M, N)
    return rc, solver.lib().pdlp_mi355x_last_error().decode()


def _rows(**change):
    """Row bounds of the kinds KIND names, with the given rows changed: -> dict(row_lower, row_upper)"""
    inf = np.inf
    lo = np.array([1.0, -inf, 2.0, -inf, 3.0, -inf])
    up = np.array([1.0, 4.0, inf, inf, 3.0, 5.0])
    for i, (l, u) in change.items():
        lo[int(i[1:])], up[int(i[1:])] = l, u
    return dict(row_lower=lo, row_upper=up)


CLEAN = [M, 1, N]


def test_verdict_no_finding():
    everything = dict(a_value=np.ones(4), q_value=np.ones(3), **_rows())
    assert _verdict([everything, {}, everything], [CLEAN, [M, 0, N], CLEAN])[0] == 0
    # the edges: firstBadRow == m, firstNegDiag == n are "none"; anyNonzero == 0 without an a_value is no job, so no refusal
    assert _verdict([dict(q_value=np.ones(3), **_rows())], [[M, 0, N]])[0] == 0
    # a record is looked at only where the variant gave the array
    assert _verdict([{}], [[2, 0, 1]])[0] == 0
    assert _verdict([dict(col_cost=np.ones(N))], [[0, 0, 0]])[0] == 0


def test_verdict_each_finding_in_the_words_of_its_update_entry():
    rc, msg = _verdict([dict(**_rows(r4=(-np.inf, 3.0)))], [[4, 0, N]])
    assert rc != 0 and msg == ("variant 0: pdlp_mi355x_update: row 4 would change its kind from equality to <= (upper bound only) "
                               + KIND_WORDS)
    rc, msg = _verdict([dict(**_rows(r0=(-np.inf, np.inf)))], [[0, 0, N]])
    assert rc != 0 and msg == "variant 0: pdlp_mi355x_update: row 0 would change its kind from equality to ranged or free " + KIND_WORDS
    rc, msg = _verdict([dict(**_rows(r5=(0.0, np.inf)))], [[M - 1, 0, N]])
    assert rc != 0 and msg == ("variant 0: pdlp_mi355x_update: row 5 would change its kind from <= (upper bound only) to >= (lower "
                               "bound only) " + KIND_WORDS)
    rc, msg = _verdict([dict(a_value=np.zeros(4))], [[M, 0, N]])
    assert rc != 0 and msg == "variant 0: " + ZERO
    for col in (0, N - 1):
        rc, msg = _verdict([dict(q_value=-np.ones(3))], [[M, 0, col]])
        assert rc != 0 and msg == "variant 0: " + NEG % col


def test_verdict_order_within_a_variant():
    rows = _rows(r2=(2.0, 2.0))
    everything = dict(a_value=np.zeros(4), q_value=-np.ones(3), **rows)
    rc, msg = _verdict([everything], [[2, 0, 1]])
    assert rc != 0 and msg.startswith("variant 0: pdlp_mi355x_update: row 2 would change its kind from >= (lower bound only) to equality")
    rc, msg = _verdict([dict(a_value=np.zeros(4), q_value=-np.ones(3))], [[M, 0, 1]])
    assert rc != 0 and msg == "variant 0: " + ZERO
    rc, msg = _verdict([dict(a_value=np.ones(4), q_value=-np.ones(3), **_rows())], [[M, 1, 1]])
    assert rc != 0 and msg == "variant 0: " + NEG % 1


def test_verdict_the_lowest_variant_across_variants():
    neg, zero = dict(q_value=-np.ones(3)), dict(a_value=np.zeros(4))
    rc, msg = _verdict([{}, {}, {}, neg, {}, {}, {}, {}, {}, zero], [CLEAN] * 3 + [[M, 0, 3]] + [CLEAN] * 5 + [[M, 0, N]])
    assert rc != 0 and msg == "variant 3: " + NEG % 3
    # a later variant's finding of an earlier kind does not overtake
    rc, msg = _verdict([zero, dict(**_rows(r1=(1.0, 1.0)))], [[M, 0, N], [1, 0, N]])
    assert rc != 0 and msg == "variant 0: " + ZERO


# ---- what Python checks before the library is asked ------------------------------------------------------------------------
def _batch_without_a_device(name="afiro"):
    """A DeviceBatch as far as run_tensors' own checks go: no handle (creating one needs a device)."""
    b = object.__new__(solver.DeviceBatch)
    b.lp, b.params, b.h = BC.lp(name), abi.default_params(), C.c_void_p()
    return b


def test_run_tensors_checks_its_tensors_in_python():
    torch = pytest.importorskip("torch")
    b = _batch_without_a_device()
    n, m = b.lp.num_col, b.lp.num_row
    with pytest.raises(ValueError, match=r"variants\[1\]: col_cost: a tensor on a cuda device is needed, got one on cpu"):
        b.run_tensors([{}, dict(col_cost=torch.zeros(n, dtype=torch.float64))])
    with pytest.raises(TypeError, match=r"variants\[0\]: col_cost: dtype torch.float64 is needed, got torch.float32"):
        b.run_tensors([dict(col_cost=torch.zeros(n, dtype=torch.float32))])
    with pytest.raises(TypeError, match=r"variants\[0\]: a_value: a torch tensor is needed, got ndarray"):
        b.run_tensors([dict(a_value=np.zeros(3))])
    stack = torch.zeros(n, 4, dtype=torch.float64).t()  # [4, n], rows not contiguous
    with pytest.raises(ValueError, match=r"variants\[2\]: col_cost: a contiguous tensor is needed"):
        b.run_tensors([{}, {}, dict(col_cost=stack[2])])
    with pytest.raises(ValueError, match=r"variants\[0\]: col_lower: a one-dimensional tensor is needed, got 2 dimensions"):
        b.run_tensors([dict(col_lower=torch.zeros(1, n, dtype=torch.float64))])  # (a [K, n] tensor is passed row by row)
    with pytest.raises(ValueError, match=r"variants\[0\]: unknown keys \['cost'\]"):
        b.run_tensors([dict(cost=torch.zeros(n, dtype=torch.float64))])


def test_run_tensors_checks_the_shapes_of_out():
    torch = pytest.importorskip("torch")
    b = _batch_without_a_device()
    n, m = b.lp.num_col, b.lp.num_row
    K = 3
    vs = [{}] * K
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"out\['col_value'\]: shape \(3, %d\) is needed, got \(2, %d\)" % (n, n)):
        b.run_tensors(vs, out=dict(col_value=f64(2, n)))
    with pytest.raises(ValueError, match=r"out\['row_dual'\]: shape \(3, %d\) is needed, got \(3, %d\)" % (m, n)):
        b.run_tensors(vs, out=dict(row_dual=f64(K, n)))
    with pytest.raises(ValueError, match=r"out\['col_dual'\]: shape \(3, %d\) is needed" % n):
        b.run_tensors(vs, out=dict(col_dual=f64(K * n)))
    with pytest.raises(TypeError, match=r"out\['col_dual'\]: a torch tensor is needed, got ndarray"):
        b.run_tensors(vs, out=dict(col_dual=np.zeros((K, n))))
    with pytest.raises(ValueError, match="out: unknown vectors"):
        b.run_tensors(vs, out=dict(x=f64(K, n)))
    with pytest.raises(ValueError, match=r"out: one entry per variant is needed \(3\), got 2"):
        b.run_tensors(vs, out=[{}, {}])
    # (per-variant dicts are taken in order, and a vector left out is allocated on the device: the offender comes first here)
    with pytest.raises(TypeError, match=r"variant 0: out\['col_value'\]: dtype torch.float64 is needed"):
        b.run_tensors(vs, out=[dict(col_value=torch.zeros(n, dtype=torch.float32)), {}, {}])
    with pytest.raises(ValueError, match=r"variant 0: out\['row_value'\]: a one-dimensional tensor is needed"):
        b.run_tensors(vs, out=[dict(col_value=None, col_dual=None, row_value=f64(1, m)), {}, {}])
    # shapes right, but host memory: still Python's to refuse
    with pytest.raises(ValueError, match=r"variant 0: out\['col_value'\]: a tensor on a cuda device is needed"):
        b.run_tensors(vs, out=dict(col_value=f64(K, n)))


def test_stacked_turns_stacked_tensors_into_variants():
    torch = pytest.importorskip("torch")
    from highs_amd import tensors as T
    c, a = torch.arange(12, dtype=torch.float64).reshape(3, 4), torch.arange(6, dtype=torch.float64).reshape(3, 2)
    vs = T.stacked(col_cost=c, a_value=a, q_value=None)
    assert len(vs) == 3 and all(set(v) == {"col_cost", "a_value"} for v in vs)
    for k in range(3):
        assert vs[k]["col_cost"].data_ptr() == c[k].data_ptr() and vs[k]["col_cost"].is_contiguous() and vs[k]["col_cost"].dim() == 1
        assert torch.equal(vs[k]["a_value"], a[k])
    with pytest.raises(ValueError, match="a_value: 3 rows are needed as in the other arrays, got 2"):
        T.stacked(col_cost=c, a_value=a[:2])
    with pytest.raises(ValueError, match="col_cost: a two-dimensional tensor"):
        T.stacked(col_cost=c[0])
    with pytest.raises(TypeError, match="col_cost: a torch tensor is needed, got ndarray"):
        T.stacked(col_cost=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="no tensor given"):
        T.stacked()


def test_driver_in_device_mode_behind_canned_lanes_under_sanitizers(tmp_path):
    """The per-call mode in the driver (csrc/pdlp_batch.cpp) with canned lanes: every lane is told the mode, lane 0 alone
    validates, once, all variants; restores come from the copy of P that stands for HBM, after host calls and before them;
    refusals, refills, a throwing update and the failure rule as in host mode.  A host program of its own, never loaded
    into Python."""
    env = dict(os.environ, OUT=str(tmp_path / "batch_driver_check"))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "batch_driver_check.sh")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all scenarios passed" in r.stdout
    device = [line for line in r.stdout.splitlines() if line.startswith("ok: device mode, ")]
    assert len(device) >= 9
    assert any("[AnQnBDQn]: concurrent: 8 lanes" in line for line in device)
    assert any("sequential: 48 work blocks need more than one XCD" in line for line in device)
