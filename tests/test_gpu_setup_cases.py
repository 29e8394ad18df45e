"""The device-side set-up (pdlp_setup.hip, DeviceMatrix::buildFromDevice, k_block_span) against the host build, the oracle's
formulation and the numpy restatements of the layout rules, array for array, on the generated problems of
tests/setup_cases.py.  Every case creates one solver prepared on the host and one prepared on the device and reads what both
hold through the test hook pdlp_mi355x_device_matrix (DeviceSolver.device_matrix): no comparison carries a tolerance, every
assertion is == on integers or on bit patterns.  That each case sits on the edge it claims is checked without a GPU in
tests/test_setup_cases_host.py."""
import numpy as np
import pytest

import oraclelib as O
import setup_cases as SC
import setup_restated as R
from highs_amd import solver

pytestmark = pytest.mark.gpu

HIPDLP_OPTS = [{}, {"pdlp_features_off": 1}, {"pdlp_scaling_mode": 7, "pdlp_ruiz_iterations": 3}]  # as test_gpu_hipdlp.py's set-up test
SCALARS = ("use_slab", "n_major", "n_minor", "nnz", "chunk", "n_blocks", "slab_blocks", "rows_per_block", "minor_bits", "slab_width_log2",
           "n_long", "n_tasks", "task_group", "long_group", "long_slots", "nnz_short", "tile_log2", "n_tiles")
INT_ARRAYS = ("beg", "idx", "block_beg", "tasks", "wave_beg", "wave_ptr", "ent", "long_mask", "long_map", "tile_owner", "span_lo", "span_hi",
              "span_cnt")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def twins(lp, monkeypatch, env, **opts):
    """(host-prepared solver, device-prepared solver) of one problem; the set-up path really differs."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = []
    for dev in ("0", "1"):
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", dev)
        out.append(solver.DeviceSolver(lp, **opts))
    assert out[0].setup_scalars()["gpu_setup"] == 0.0 and out[1].setup_scalars()["gpu_setup"] == 1.0
    return out


def assert_same_scalars(H, D):
    assert (H.n, H.m, H.nnz, H.n_eqs) == (D.n, D.m, D.nnz, D.n_eqs)
    a, b = H.setup_scalars(), D.setup_scalars()
    for k in a:
        if k != "gpu_setup":
            assert same_bits(np.array([a[k]]), np.array([b[k]])), (k, a[k], b[k])
    return b


def assert_same_matrix(a, b):
    """Every scalar and every array of two device_matrix dumps."""
    assert set(a) == set(b) == set(SCALARS) | set(INT_ARRAYS) | {"val", "slab_val"}
    for k in SCALARS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in INT_ARRAYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    for k in ("val", "slab_val"):
        assert same_bits(a[k], b[k]), k


def assert_pads_are_zero(d):
    """The kernels clamp their loads onto the element behind the last entry."""
    assert d["idx"][-1] == 0 and bits(d["val"])[-1] == 0
    if d["use_slab"]:
        assert d["ent"][-1] == 0 and bits(d["slab_val"])[-1] == 0


def assert_stream_operand_is(d, beg, idx, val):
    """A stream-layout dump holds exactly this CSR: every slot, stored zeros included, and the zero pad element."""
    assert d["use_slab"] == 0 and d["n_major"] == len(beg) - 1 and d["nnz"] == len(idx)
    assert np.array_equal(d["beg"], beg) and np.array_equal(d["idx"][:-1], idx) and same_bits(d["val"][:-1], val)
    assert len(d["idx"]) == len(idx) + 1 == len(d["val"])
    assert_pads_are_zero(d)


@pytest.mark.parametrize("features_off", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.FORMULATION))
def test_formulation_on_the_device_is_the_hosts_and_the_oracles(name, features_off, monkeypatch):
    lp = SC.case(name)
    P, F = solver.Prepared(lp, pdlp_features_off=features_off), O.FormulatedView(lp, pdlp_features_off=features_off)
    H, D = twins(lp, monkeypatch, {"PDLP_MI355X_SLAB": "0"}, pdlp_features_off=features_off)
    sc = assert_same_scalars(H, D)
    assert (D.n, D.m, D.nnz, D.n_eqs) == (P.n, P.m, P.nnz, P.n_eqs) == (F.n, F.m, F.nnz, F.n_eqs)
    assert (sc["n_eqs"], sc["n0"], sc["scaled"]) == (P.n_eqs, lp.num_col, 1.0 - features_off)
    assert same_bits([sc["norm_cost"], sc["norm_rhs"], sc["mat_norm_inf"]], [P.norm_cost, P.norm_rhs, P.mat_norm_inf])
    assert same_bits([sc["norm_cost"], sc["norm_rhs"], sc["mat_norm_inf"]], [F.norm_cost, F.norm_rhs, F.mat_norm_inf])
    assert same_bits([sc["sum_cost2"], sc["sum_rhs2"]], [np.cumsum(P.cost * P.cost)[-1], np.cumsum(P.rhs * P.rhs)[-1]])  # left to right
    for k in ("cost", "rhs", "lower", "upper", "col_scale", "row_scale"):
        ref = getattr(P, k)
        assert same_bits(ref, getattr(F, k)), k
        assert same_bits(D.get(k, len(ref)), ref) and same_bits(H.get(k, len(ref)), ref), k
    if lp.hessian is not None:
        form, hess = solver.host_prepare_qp(lp, pdlp_features_off=features_off)
        assert hess["has_diag"] == 1 and hess["nnz_off"] == 0
        assert same_bits(D.get("qdiag", D.n), hess["qdiag"]) and same_bits(H.get("qdiag", H.n), hess["qdiag"])
    # the matrices, entry for entry
    for which, (beg, idx, val) in enumerate([(P.csr_beg, P.csr_idx, P.csr_val), (P.csc_beg, P.csc_idx, P.csc_val)]):
        d, h = D.device_matrix(which), H.device_matrix(which)
        assert_stream_operand_is(d, beg, idx, val)
        assert_same_matrix(h, d)
    assert same_bits(P.csr_val, F.csr_val) and np.array_equal(P.csr_idx, F.csr_idx)
    H.close(); D.close()


@pytest.mark.parametrize("opts", HIPDLP_OPTS, ids=["default", "unscaled", "ruiz3_pc_l2"])
@pytest.mark.parametrize("name", sorted(set(SC.FORMULATION) - {"kinds_qp"}))  # (a quadratic objective: the pdlp path only)
def test_hipdlp_formulation_on_the_device_is_the_hosts(name, opts, monkeypatch):
    lp = SC.case(name)
    P = solver.Prepared(lp, solver="hipdlp", **opts)
    H, D = twins(lp, monkeypatch, {"PDLP_MI355X_SLAB": "0"}, solver="hipdlp", **opts)
    sc = assert_same_scalars(H, D)
    assert (D.n, D.m, D.nnz, D.n_eqs) == (P.n, P.m, P.nnz, P.n_eqs)
    assert same_bits([sc["norm_cost"], sc["norm_rhs"]], [P.norm_cost, P.norm_rhs]) and np.isnan(sc["mat_norm_inf"]) and np.isnan(sc["sum_cost2"])
    for k, ref in (("cost", P.cost), ("lower", P.lower), ("upper", P.upper), ("col_scale", P.col_scale), ("row_lower", P.rhs),
                   ("row_scale", P.row_scale)):
        assert same_bits(D.get(k, len(ref)), ref) and same_bits(H.get(k, len(ref)), ref), k
    assert same_bits(D.get("row_upper", D.m), H.get("row_upper", H.m))
    for which, (beg, idx, val) in enumerate([(P.csr_beg, P.csr_idx, P.csr_val), (P.csc_beg, P.csc_idx, P.csc_val)]):
        d, h = D.device_matrix(which), H.device_matrix(which)
        assert_stream_operand_is(d, beg, idx, val)
        assert_same_matrix(h, d)
    H.close(); D.close()


def test_matrix_norm_sees_the_last_partial_maximum(monkeypatch):
    """max |a_ij| where only the last of the device's 1 024 partial maxima holds it (unscaled, so that the slot decides)."""
    lp = SC.absmax_tail()
    H, D = twins(lp, monkeypatch, dict(SC.LAYOUT_ENV, PDLP_MI355X_SLAB="0"), pdlp_features_off=1)
    sc = assert_same_scalars(H, D)
    assert sc["mat_norm_inf"] == 100.0
    H.close(); D.close()


SLAB_CASES = sorted(SC.LAYOUT) + sorted(SC.FORMULATION)
HIPDLP_SLAB_CASES = ["kinds_257", "kinds_thresholds", "layout_cold", "layout_long_positions", "layout_owners", "layout_m2305"]


@pytest.mark.parametrize("alg,name", [("pdlp", n) for n in SLAB_CASES] + [("hipdlp", n) for n in HIPDLP_SLAB_CASES])
def test_slab_layout_on_the_device_is_the_hosts_and_the_restated_one(alg, name, monkeypatch):
    """Both operands: every scalar and array equal between the two builds — the tile owners, the block spans and the task
    records among them — and, from the device-built solver's dump, equal to the restated partition (with the cold counts and
    the operand's own major cost), block spans, owners, width rule and slab layout at the width the build reports."""
    lp = SC.case(name)
    env = SC.layout_env(name)
    P = solver.Prepared(lp, solver=alg)
    H, D = twins(lp, monkeypatch, env, solver=alg)
    assert_same_scalars(H, D)
    forced = int(env.get("PDLP_MI355X_SLAB_W", 0))
    for which in (0, 1):
        beg, idx, val, n_major, n_minor = (P.csr_beg, P.csr_idx, P.csr_val, P.m, P.n) if which == 0 else (P.csc_beg, P.csc_idx, P.csc_val, P.n, P.m)
        d, h = D.device_matrix(which), H.device_matrix(which)
        assert_same_matrix(h, d)
        assert d["use_slab"] == 1 and (d["n_major"], d["n_minor"], d["nnz"]) == (n_major, n_minor, len(idx))
        assert_pads_are_zero(d)
        nb, mb, wb, _ = R.partition(beg, idx, n_major, n_minor, which)
        assert (d["slab_blocks"], d["minor_bits"], d["n_blocks"]) == (nb, mb, 0) and np.array_equal(d["wave_beg"], wb)
        assert d["rows_per_block"] == np.diff(wb[::16]).max()
        lo, hi, cnt, hist, tl = R.block_spans(beg, idx, wb, n_minor)
        assert np.array_equal(d["span_lo"], lo) and np.array_equal(d["span_hi"], hi) and np.array_equal(d["span_cnt"], cnt)
        assert d["tile_log2"] == tl and np.array_equal(d["tile_owner"], R.tile_owners(hist)[0])
        W = R.slab_width(lo, hi, cnt, forced)
        assert d["slab_width_log2"] == W
        ref = R.slab_layout(beg, idx, val, n_major, n_minor, wb, mb, W)
        assert d["nnz_short"] == ref["nnz_short"] and d["n_long"] == len(ref["long_map"])
        assert np.array_equal(d["long_mask"], ref["long_mask"]) and np.array_equal(d["long_map"], ref["long_map"])
        assert np.array_equal(d["beg"], ref["long_beg"]) and np.array_equal(d["idx"][:-1], ref["long_idx"]) and same_bits(d["val"][:-1], ref["long_val"])
        assert np.array_equal(d["wave_ptr"], ref["wave_ptr"]) and np.array_equal(d["ent"][:-1], ref["ent"]) and same_bits(d["slab_val"][:-1], ref["slab_val"])
        # every segment of every long major is some task's, once
        tk = d["tasks"]
        real = tk[tk[:, 2] >= 0]
        assert d["n_tasks"] % max(d["task_group"], 1) == 0 and (real[:, 1] - real[:, 0]).sum() == ref["long_beg"][-1]
        assert np.array_equal(np.unique(real[:, 5]), ref["long_map"])
    H.close(); D.close()


@pytest.mark.parametrize("alg", ["pdlp", "hipdlp"])
@pytest.mark.parametrize("bad", ["m", "-1"])
def test_a_row_index_out_of_range_is_refused_on_both_paths_with_the_same_words(alg, bad, monkeypatch):
    """validateProblem runs in front of either set-up: the device path never sees the index, and says what the host path says.
    An error return, not a fault; a fresh solver on the good LP works afterwards."""
    lp = SC.case("kinds_5")
    import copy
    broken = copy.copy(lp)
    broken.a_index = lp.a_index.copy()
    broken.a_index[3] = lp.num_row if bad == "m" else -1
    words = []
    for dev in ("0", "1"):
        monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", dev)
        with pytest.raises(RuntimeError) as e:
            solver.DeviceSolver(broken, solver=alg)
        words.append(str(e.value))
    assert words[0] == words[1] == "pdlp_mi355x_create failed: row index out of range"
    S = solver.DeviceSolver(lp, solver=alg)
    assert S.setup_scalars()["gpu_setup"] == 1.0 and S.iterate(40).iters > 0
    S.close()
