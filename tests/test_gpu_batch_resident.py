"""pdlp_mi355x_batch_run_device on the GPU: variants and solutions as tensors in HBM.  Every R[k] must be, bit for bit, what
DeviceBatch.run — code that exists without this feature — gives for the same arrays as numpy: array_equal on the four
vectors, == on every count and scalar.  Full lanes, the restore rule from the batch's copy of P in HBM, the sequential
route, stacked outputs between guard rows, skipped result vectors, a hot start, a side stream, the refusals (all-or-nothing)
and the edges of the validation launch.  No tolerance anywhere."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import batch_values_cases as BC
import update_cases as UC
from highs_amd import abi, solver
from highs_amd import lp as L

torch = pytest.importorskip("torch")
from highs_amd import tensors as T  # noqa: E402

pytestmark = pytest.mark.gpu
OPTIONS = BC.OPTIONS
SOLUTION = BC.SOLUTION
FIELDS = BC.COUNTS + BC.SCALARS + ("value_valid", "dual_valid")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()).to("cuda")


def _dev_variant(v):
    """A variant as DeviceBatch.run takes it -> as run_tensors takes it: every array a tensor."""
    out = {}
    for k, a in v.items():
        if k in ("offset", "iter_limit"):
            out[k] = a
        elif k == "start":
            out[k] = {s: _dev(x) for s, x in a.items()}
        else:
            out[k] = _dev(a)
    return out


def _same(got, want, what, vectors=SOLUTION):
    """got: tensors.TensorResult; want: the host batch's ResultHandle."""
    for k in vectors:
        assert np.array_equal(getattr(got, k).cpu().numpy(), getattr(want, k)), (what, k)
    for k in FIELDS:
        if k in ("value_valid", "dual_valid") and len(vectors) < 4:
            continue
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


def _both(batch, variants, what, device_first=True):
    """run_tensors and run on the same batch with the same arrays; -> (device results, host results, info of the device run)"""
    dv = [_dev_variant(v) for v in variants]
    if device_first:
        got = batch.run_tensors(dv)
        I = batch.info()
        want = batch.run(variants)
    else:
        want = batch.run(variants)
        got = batch.run_tensors(dv)
        I = batch.info()
    assert len(got) == len(want) == len(variants)
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w.result, (what, k))
    return got, want, I


# ---- 1: eight data variants, eight lanes ------------------------------------------------------------------------------------
def test_full_lanes_have_the_bits_of_the_host_batch_and_share_their_launches():
    name = "25fv47"  # 21 work blocks: XCD-local
    lp = BC.lp(name)
    kinds = ["cost", "col_bounds", "row_bounds", "cost", "col_bounds", "row_bounds", "all", "cost"]
    variants = [UC.modification(lp, what, 3 + i) for i, what in enumerate(kinds)]
    batch = solver.DeviceBatch(lp, lanes=8, **OPTIONS)
    got, want, I = _both(batch, variants, name)
    batch.close()
    assert all(getattr(g, k).is_cuda and getattr(g, k).dtype == torch.float64 for g in got for k in SOLUTION)
    print("batch info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches, list(I.xcc_of_lane))
    assert I.text == "concurrent: 8 lanes, 21 workgroups each"
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 8, 8, 0)
    # the bounds DESIGN section 2g derives, against each variant's solo solve on a held solver of its own
    solo = []
    full = dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    for k, u in enumerate(variants):
        held.update(**dict(full, **u))
        before = held.stage("persistent_launches", 1)[0]
        R = held.run(lp.num_col, lp.num_row)
        solo.append(int(held.stage("persistent_launches", 1)[0] - before))
        assert BC.same_result(want[k].result, R) is None  # (the reference itself is the solo solve's)
    held.close()
    print("solo launches:", solo)
    assert I.trial_launches <= max(solo) + 15, (I.trial_launches, solo)
    assert I.check_launches == I.trial_launches + 1


# ---- 2: the restore rule, from the batch's copy of P in HBM ----------------------------------------------------------------
RESTORE = {
    "cost": ("25fv47", None, lambda: BC.data("25fv47", "cost", 11)[1]),
    "a_value": ("25fv47", "matrix", lambda: BC.matrix("25fv47", "jitter", 12)[1]),
    "q_value": ("sq100", "hessian", lambda: BC.hessian("sq100", "scale7")[1]),
}


@pytest.mark.parametrize("kind", sorted(RESTORE))
def test_what_a_variant_leaves_alone_goes_back_to_p(kind):
    name, updatable, make = RESTORE[kind]
    A = make()
    variants = [A, A, {}, {}, A, A]  # whichever lane takes a P has solved an A before
    options = dict(OPTIONS) if updatable is None else dict(OPTIONS, updatable=updatable)
    want = None
    for lanes in (2, 1):
        batch = solver.DeviceBatch(BC.lp(name), lanes=lanes, **options)
        dv = [_dev_variant(v) for v in variants]
        got = batch.run_tensors(dv)  # (first: no host run has touched the lanes)
        if want is None:
            want = batch.run(variants)
            # a broken restore would show: A's result differs from P's
            assert BC.really_differs(want[0].result, want[2].result)
            assert BC.same_result(want[2].result, want[3].result) is None and BC.same_result(want[0].result, want[5].result) is None
        for k in range(len(variants)):
            _same(got[k], want[k].result, (kind, lanes, k))
        again = batch.run_tensors(dv[::-1])  # (and with lanes that differ from P when the call starts)
        for k in range(len(variants)):
            _same(again[k], want[len(variants) - 1 - k].result, (kind, lanes, "reversed", k))
        batch.close()


# ---- 3: the sequential route -------------------------------------------------------------------------------------------------
def test_above_one_xcd_the_variants_run_one_after_the_other():
    name = "80bau3b"
    variants = [BC.matrix(name, "jitter", 71)[1], {}]
    batch = solver.DeviceBatch(BC.lp(name), lanes=8, updatable="matrix", **OPTIONS)
    _, _, I = _both(batch, variants, name)
    batch.close()
    assert I.lanes_concurrent == 1 and I.trial_launches == 0
    m = re.fullmatch(r"sequential: (\d+) work blocks need more than one XCD", I.text)
    assert m and int(m.group(1)) > 32, I.text


# ---- 4: stacked outputs between guard rows; skipped vectors ----------------------------------------------------------------------
def test_stacked_out_writes_rows_one_to_k_and_nothing_else():
    name = "adlittle"
    lp = BC.lp(name)
    K = 5
    costs = np.stack([UC.modification(lp, "cost", 40 + k)["col_cost"] for k in range(K)])
    variants = [dict(col_cost=costs[k]) for k in range(K)]
    batch = solver.DeviceBatch(lp, lanes=3, **OPTIONS)
    want = batch.run(variants)
    sizes = dict(col_value=lp.num_col, col_dual=lp.num_col, row_value=lp.num_row, row_dual=lp.num_row)
    SENTINEL = -12345.678
    bufs = {k: torch.full((K + 2, n), SENTINEL, dtype=torch.float64, device="cuda") for k, n in sizes.items()}
    stack = _dev(costs)  # [K, num_col]: its rows are the variants
    got = batch.run_tensors(T.stacked(col_cost=stack), out={k: b[1:K + 1] for k, b in bufs.items()})
    I = batch.info()
    batch.close()
    assert I.text.startswith("concurrent: 3 lanes") and I.fallback_variants == 0
    for name_, b in bufs.items():
        h = b.cpu().numpy()
        assert np.all(h[0] == SENTINEL) and np.all(h[K + 1] == SENTINEL), name_
        for k in range(K):
            assert np.array_equal(h[1 + k], getattr(want[k].result, name_)), (name_, k)
            assert getattr(got[k], name_).data_ptr() == b[1 + k].data_ptr()
    for k in range(K):
        _same(got[k], want[k].result, ("stacked", k))


def test_every_subset_of_result_vectors_may_be_left_out():
    lp = BC.lp("afiro")
    variants = [UC.modification(lp, "cost", 50), {}]
    batch = solver.DeviceBatch(lp, lanes=2, **OPTIONS)
    want = batch.run(variants)
    dv = [_dev_variant(v) for v in variants]
    for r in range(5):
        for skipped in itertools.combinations(SOLUTION, r):
            got = batch.run_tensors(dv, out=[{k: None for k in skipped}, {}])
            kept = tuple(k for k in SOLUTION if k not in skipped)
            assert all(getattr(got[0], k) is None for k in skipped)
            _same(got[0], want[0].result, ("skipped", skipped), vectors=kept)
            assert got[0].value_valid == int("col_value" in kept and "row_value" in kept)
            assert got[0].dual_valid == int("col_dual" in kept and "row_dual" in kept)
            _same(got[1], want[1].result, ("beside skipped", skipped))
    batch.close()


# ---- 5: a hot start given as device tensors ---------------------------------------------------------------------------------
def test_a_hot_start_inside_a_device_variant():
    name = "adlittle"
    lp = BC.lp(name)
    batch = solver.DeviceBatch(lp, lanes=3, **OPTIONS)
    first = batch.run([{}])[0].result
    start = dict(col_value=first.col_value, row_value=first.row_value, row_dual=first.row_dual)
    u = UC.modification(lp, "cost", 61)
    variants = [u, dict(u, start=start), dict(u, iter_limit=80), {}]
    _, want, I = _both(batch, variants, "hot", device_first=False)
    batch.close()
    assert (I.lanes_concurrent, I.fallback_variants) == (3, 0), I.text
    assert BC.really_differs(want[1].result, want[0].result)  # (the start was taken)
    assert want[2].result.num_iter == 79


# ---- 6: stream ordering -----------------------------------------------------------------------------------------------------
def test_run_tensors_reads_behind_the_stream_that_fills_its_tensors():
    name = "adlittle"
    lp = BC.lp(name)
    K = 4
    variants = [UC.modification(lp, "all", 70 + k) for k in range(K)]
    batch = solver.DeviceBatch(lp, lanes=4, **OPTIONS)
    want = batch.run(variants)
    src = [_dev_variant(v) for v in variants]
    bufs = [{k: torch.zeros_like(t) for k, t in s.items() if k != "offset"} for s in src]
    work = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):  # the fills wait behind some milliseconds of work on this stream
            work = work @ work * 1e-3
        for s, b in zip(src, bufs):
            for k, t in b.items():
                t.copy_(s[k])
        got = batch.run_tensors([dict(b, offset=s["offset"]) for s, b in zip(src, bufs)])  # (no synchronisation in between)
    torch.cuda.synchronize()
    batch.close()
    for k in range(K):
        _same(got[k], want[k].result, ("side stream", k))


# ---- 7: refusals, all-or-nothing ------------------------------------------------------------------------------------------------
def _message(e):
    return str(e.value).split(" failed: ", 1)[1]


def _raw_run(batch, V, Rs, K):
    rc = solver.lib().pdlp_mi355x_batch_run_device(batch.h, K, V, Rs, None)
    return rc, solver.lib().pdlp_mi355x_last_error().decode()


def test_refusals_leave_the_batch_as_it_was():
    name, updatable = "sq100", "matrix+hessian"
    P = BC.lp(name)
    good = [BC.hessian(name, "scale7")[1], BC.matrix(name, "values", 43)[1], {}, BC.both(name, "values", "regen", 44)[1],
            BC.data(name, "cost", 5)[1], {}, BC.data(name, "all", 6)[1], BC.hessian(name, "regen", 3)[1]]
    batch = solver.DeviceBatch(P, lanes=3, updatable=updatable, **OPTIONS)
    dgood = [_dev_variant(v) for v in good]
    before = batch.run_tensors(dgood)
    want = batch.run(good)
    for k in range(len(good)):
        _same(before[k], want[k].result, ("before", k))

    def still_the_same(what):
        after = batch.run_tensors(dgood)
        for k in range(len(good)):
            for f in SOLUTION:
                assert torch.equal(getattr(after[k], f), getattr(before[k], f)), (what, k, f)
            _same(after[k], want[k].result, (what, k))

    # a host pointer (pinned host memory) as col_cost of variant 5 of 8: the struct is filled by hand, Python would refuse it
    pinned = torch.zeros(P.num_col, dtype=torch.float64).pin_memory()
    V, keep = batch._tensor_variants(dgood)
    V[5].u.col_cost = C.cast(C.c_void_p(pinned.data_ptr()), abi.c_f64p)
    results = [T.TensorResult(P.num_col, P.num_row, torch.device("cuda", 0)) for _ in good]
    Rs = (abi.PdlpResult * len(good))(*[r.struct for r in results])
    rc, msg = _raw_run(batch, V, Rs, len(good))
    assert rc != 0 and msg == "variant 5: col_cost is not device memory on device 0", msg
    still_the_same("host pointer in a variant")
    # ... and as a result vector
    V, keep = batch._tensor_variants(dgood)
    host_out = torch.zeros(P.num_row, dtype=torch.float64).pin_memory()
    Rs[2].row_dual = C.cast(C.c_void_p(host_out.data_ptr()), abi.c_f64p)
    rc, msg = _raw_run(batch, V, Rs, len(good))
    assert rc != 0 and msg == "result 2: row_dual is not device memory on device 0", msg
    assert np.all(host_out.numpy() == 0.0)
    still_the_same("host pointer in a result")
    # the value checks: the words are the host batch's for the same arrays
    lo, up = np.array(P.row_lower, dtype=np.float64), np.array(P.row_upper, dtype=np.float64)
    i = P.num_row - 1
    one_sided_or_equality = (lo[i] > -1e20) != (up[i] < 1e20) or lo[i] == up[i]
    (lo[i], up[i]) = (-np.inf, np.inf) if one_sided_or_equality else (1.0, 1.0)  # -> free; a ranged or free row -> equality
    q_neg = np.array(P.hessian[2], dtype=np.float64)
    q_neg[:] = -np.abs(q_neg) - 1.0
    for what, bad in (("kind", dict(good[1], row_lower=lo, row_upper=up)), ("zero", dict(a_value=np.zeros(len(P.a_value)))),
                      ("negative", dict(q_value=q_neg))):
        lst = good[:4] + [bad] + good[5:]
        with pytest.raises(RuntimeError) as host:
            batch.run(lst)
        with pytest.raises(RuntimeError) as dev:
            batch.run_tensors([_dev_variant(v) for v in lst])
        print(what, "->", _message(dev))
        assert _message(dev) == _message(host) and _message(dev).startswith("variant 4: pdlp_mi355x"), (what, _message(dev), _message(host))
        still_the_same(what)
    batch.close()


# ---- 8: the edges of the validation launch -----------------------------------------------------------------------------------
KINDS = (0, 1, 3, 2, 4)  # equality, <=, ranged, >=, free: cycled over the rows


def _kinds_lp(m, n0, seed):
    """m rows whose kinds cycle through KINDS, n0 boxed columns, four entries per row, feasible inside the box."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n0))
    for i in range(m):
        at = rng.choice(n0, 4, replace=False)
        A[i, at] = rng.uniform(0.5, 2.0, 4) * rng.choice([-1.0, 1.0], 4)
    ax = A @ rng.uniform(0.2, 0.8, n0)
    inf = float("inf")
    rl, ru = np.full(m, -inf), np.full(m, inf)
    for i in range(m):
        k = KINDS[i % len(KINDS)]
        if k == 0: rl[i] = ru[i] = ax[i]
        elif k == 1: ru[i] = ax[i] + 0.3
        elif k == 2: rl[i] = ax[i] - 0.3
        elif k == 3: rl[i], ru[i] = ax[i] - 0.2, ax[i] + 0.4
    rows, cols = np.nonzero(A.T)
    a_start = np.zeros(n0 + 1, np.int32)
    a_start[1:] = np.cumsum(np.bincount(rows, minlength=n0))
    return L.HighsLp(n0, m, rng.standard_normal(n0), np.zeros(n0), np.ones(n0), rl, ru, a_start, cols.astype(np.int32),
                     A.T[rows, cols], 1, 0.25, "kinds").normalise()


def _other_kind(lp, rows):
    """Row bounds of lp with the kind of every row in `rows` changed: -> dict(row_lower, row_upper)"""
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    for i in rows:
        if KINDS[i % len(KINDS)] in (3, 4):
            lo[i] = up[i] = 0.5  # ranged or free -> equality
        else:
            lo[i], up[i] = -np.inf, np.inf  # -> free
    return dict(row_lower=lo, row_upper=up)


def _records(batch, dv, n_rec):
    V, keep = batch._tensor_variants(dv)
    out = np.full(3 * n_rec, -7, dtype=np.int32)
    rc = solver.lib().pdlp_mi355x_batch_variant_records(batch.h, len(dv), V, n_rec, out.ctypes.data_as(abi.c_i32p))
    assert rc == 0, solver.lib().pdlp_mi355x_last_error().decode()
    return out.reshape(n_rec, 3)


@pytest.mark.parametrize("m", [255, 256, 257])
def test_validation_launch_at_the_workgroup_edges(m):
    lp = _kinds_lp(m, 48, seed=m)
    batch = solver.DeviceBatch(lp, lanes=1, updatable="matrix", **OPTIONS)

    def refused(variants):
        """-> the device batch's words, which are the host batch's for the same arrays"""
        with pytest.raises(RuntimeError) as host:
            batch.run(variants)
        with pytest.raises(RuntimeError) as dev:
            batch.run_tensors([_dev_variant(v) for v in variants])
        assert _message(dev) == _message(host), (_message(dev), _message(host))
        return _message(dev)

    # the only bad row at 0, at 255, at 256 and at m - 1
    for row in sorted({0, 255, 256, m - 1} & set(range(m))):
        msg = refused([{}, _other_kind(lp, [row])])
        assert msg.startswith("variant 1: pdlp_mi355x_update: row %d would change its kind from " % row), msg
        rec = _records(batch, [_dev_variant(_other_kind(lp, [row]))], 1)
        assert rec[0, 0] == row
    # two bad rows in different workgroups: the smaller one is named
    if m > 256:
        assert refused([_other_kind(lp, [m - 1, 3])]).startswith("variant 0: pdlp_mi355x_update: row 3 would")
        assert refused([_other_kind(lp, [256, 255])]).startswith("variant 0: pdlp_mi355x_update: row 255 would")
    # a finding in variants 3 and 9 of 17 (more variants than the grid holds side by side): variant 3 is named
    a = np.array(lp.a_value, dtype=np.float64)
    lst = [{} for _ in range(17)]
    lst[3], lst[9] = dict(a_value=np.zeros(a.size)), _other_kind(lp, [1])
    assert refused(lst) == "variant 3: " + ("pdlp_mi355x: the LP has no rows, no columns or no matrix nonzeros — HiGHS solves such "
                                            "LPs itself (solveUnconstrainedLp) before the PDLP path")
    lst[16] = _other_kind(lp, [m - 1])
    rec = _records(batch, [_dev_variant(v) for v in lst], 17)
    n_form = rec[0, 2]
    assert n_form >= lp.num_col
    expect = np.tile(np.array([m, 0, n_form], dtype=np.int32), (17, 1))
    expect[9, 0], expect[16, 0] = 1, m - 1
    assert np.array_equal(rec, expect), rec
    # a kind change and an all-zero matrix in the same variant: the kind change is named
    assert refused([dict(a_value=np.zeros(a.size), **_other_kind(lp, [2]))]).startswith("variant 0: pdlp_mi355x_update: row 2 would")
    # a NaN in an a_value that is otherwise zero is not all-zero, as on the host (`!= 0.0`); the last entry alone counts too
    nan, last = np.zeros(a.size), np.zeros(a.size)
    nan[a.size // 2], last[-1] = np.nan, -1e-300
    rec = _records(batch, [_dev_variant(dict(a_value=x)) for x in (nan, last, np.zeros(a.size), a)], 4)
    assert list(rec[:, 1]) == [1, 1, 0, 1] and np.all(rec[:, 0] == m) and np.all(rec[:, 2] == n_form)
    # K = 1: the records beyond the list stay as initialised
    rec = _records(batch, [_dev_variant(dict(a_value=a, **_other_kind(lp, [m - 1])))], 4)
    assert list(rec[0]) == [m - 1, 1, n_form]
    assert np.array_equal(rec[1:], np.tile(np.array([m, 0, n_form], dtype=np.int32), (3, 1))), rec
    # and the batch still solves: the LP as it is, with the bits of the host batch
    _both(batch, [{}], ("kinds", m))
    batch.close()


def test_negative_diagonal_names_the_smallest_column():
    name = "sq100"
    P = BC.lp(name)
    batch = solver.DeviceBatch(P, lanes=1, updatable="hessian", **OPTIONS)
    qs, qi, q0 = (np.asarray(x) for x in P.hessian)
    cols = np.repeat(np.arange(len(qs) - 1), np.diff(qs))
    diag = np.nonzero(qi == cols)[0]  # the slots on the diagonal
    assert diag.size >= 3
    q = np.array(q0, dtype=np.float64)
    q[diag[-1]] = -1.0
    q[diag[1]] = -1.0
    with pytest.raises(RuntimeError) as host:
        batch.run([{}, dict(q_value=q)])
    with pytest.raises(RuntimeError) as dev:
        batch.run_tensors([{}, dict(q_value=_dev(q))])
    assert _message(dev) == _message(host)
    assert ("the diagonal entry of column %d is negative" % cols[diag[1]]) in _message(dev), _message(dev)
    rec = _records(batch, [dict(q_value=_dev(q)), dict(q_value=_dev(q0)), {}], 3)
    assert rec[0, 2] == cols[diag[1]] and rec[1, 2] == rec[2, 2] > cols[diag[-1]]
    batch.close()
