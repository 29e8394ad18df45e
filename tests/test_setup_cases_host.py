"""CPU tests of tests/setup_cases.py: every generated problem sits on the edge of the set-up it claims, checked on the host
form (solver.Prepared), the oracle's formulation (oraclelib.FormulatedView) and the numpy restatements of the layout rules
(tests/setup_restated.py).  These are the conditions that keep tests/test_gpu_setup_cases.py from passing vacuously; they hold
for the references alone.  Every comparison is == on integers or on bit patterns."""
import numpy as np
import pytest

import oraclelib as O
import setup_cases as SC
import setup_restated as R
from highs_amd import solver

KIND = {"eq": 0, "le": 1, "ge": 2, "ranged": 3, "free": 3}  # cuPDLP-C form: ranged and free rows are both kRowBound


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("features_off", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.FORMULATION))
def test_host_formulation_is_the_oracles_bit_for_bit(name, features_off):
    lp = SC.case(name)
    P, F = solver.Prepared(lp, pdlp_features_off=features_off), O.FormulatedView(lp, pdlp_features_off=features_off)
    assert (P.n, P.m, P.n_eqs, P.nnz) == (F.n, F.m, F.n_eqs, F.nnz)
    for k in ("csr_beg", "csr_idx", "csc_beg", "csc_idx"):
        assert np.array_equal(getattr(P, k), getattr(F, k)), k
    assert np.array_equal(P.row_kind, F.row_type) and np.array_equal(P.row_new_idx, F.row_new_idx)
    for k in ("csr_val", "cost", "rhs", "lower", "upper", "col_scale", "row_scale"):
        assert same_bits(getattr(P, k), getattr(F, k)), k
    assert same_bits(np.array([P.norm_cost, P.norm_rhs, P.mat_norm_inf]), np.array([F.norm_cost, F.norm_rhs, F.mat_norm_inf]))


@pytest.mark.parametrize("m", SC.KINDS_SIZES)
def test_kinds_cycle_counts(m):
    lp = SC.case("kinds_%d" % m)
    P = solver.Prepared(lp, pdlp_features_off=1)
    want = np.array([KIND[SC.ROW_KINDS[i % 5]] for i in range(m)])
    assert np.array_equal(P.row_kind, want)
    n_slack = int((want == 3).sum())
    assert P.n_eqs == int(((want == 0) | (want == 3)).sum()) and P.n == lp.num_col + n_slack and P.nnz == lp.num_nz + n_slack
    # the permutation: equality-type rows first, each group in its original order
    eq = (want == 0) | (want == 3)
    assert np.array_equal(P.row_new_idx[eq], np.arange(P.n_eqs)) and np.array_equal(P.row_new_idx[~eq], np.arange(P.n_eqs, m))
    # column 0 holds every row, column 1 none, columns 2..6 one entry; the column kinds cycle
    lens = np.diff(lp.a_start)
    assert lens[0] == m and lens[1] == 0 and np.all(lens[2:7] == 1)
    if m >= 5:  # inside column 0: equality-type rows first, then the inequalities, `<=` rows negated
        col0 = P.csc_idx[P.csc_beg[0]:P.csc_beg[1]]
        assert np.all(np.diff(col0) > 0)  # (the prepared A' is sorted; the reference order shows in the oracle comparison)
        assert set(want.tolist()) == {0, 1, 2, 3}
    fin_l, fin_u = np.isfinite(lp.col_lower), np.isfinite(lp.col_upper)
    got = np.where(~fin_l & ~fin_u, 0, np.where(fin_l & ~fin_u, 1, np.where(~fin_l & fin_u, 2, np.where(lp.col_lower < lp.col_upper, 3, 4))))
    assert np.array_equal(got, np.arange(lp.num_col) % 5)
    assert lp.col_cost[0] == 0.0 and not np.signbit(lp.col_cost[0]) and lp.col_cost[3] == 0.0 and np.signbit(lp.col_cost[3])


@pytest.mark.parametrize("kind", SC.ROW_KINDS)
def test_kinds_all_of_one(kind):
    lp = SC.case("kinds_all_" + kind)
    m = lp.num_row
    assert m == 300  # more than one 256-thread block for the ranking scans
    for alg in ("pdlp", "hipdlp"):
        P = solver.Prepared(lp, solver=alg)
        slack = m if kind in ("ranged", "free") else 0
        assert P.n == lp.num_col + slack and P.n_eqs == (m if kind in ("eq", "ranged", "free") else 0)
        assert np.all(P.row_kind == (4 if (alg, kind) == ("hipdlp", "free") else KIND[kind]))


def test_thresholds_classify_on_each_side_of_1e20_and_of_infinity():
    lp = SC.case("kinds_thresholds")
    pairs = SC.threshold_pairs()
    assert lp.num_row == lp.num_col == len(pairs) > 256 // 4 and lp.sense == -1 and lp.offset != 0.0
    vals = set(SC.THRESHOLD_VALUES)
    assert {1e20, -1e20, SC.BELOW, SC.ABOVE, -SC.BELOW, -SC.ABOVE, 1e30, SC.INF, -SC.INF}.issubset(vals) and SC.BELOW < 1e20 < SC.ABOVE
    assert any(a == 0.0 and np.signbit(a) and not np.signbit(b) and b == 0.0 for a, b in pairs)  # (-0.0, 0.0): an equality row
    P, H = solver.Prepared(lp), solver.Prepared(lp, solver="hipdlp")

    def kind(a, b, inf, free):
        lo, up = a > -inf, b < inf
        return 0 if lo and up and a == b else 2 if lo and not up else 1 if up and not lo else 3 if lo and up else free
    assert np.array_equal(P.row_kind, [kind(a, b, 1e20, 3) for a, b in pairs])
    assert np.array_equal(H.row_kind, [kind(a, b, np.inf, 4) for a, b in pairs])
    i = pairs.index((SC.BELOW, SC.BELOW)); assert P.row_kind[i] == 0          # lo == up inside the threshold: eq
    i = pairs.index((1e20, 1e20)); assert P.row_kind[i] == 2 and H.row_kind[i] == 0   # ... on it: `>=` for cuPDLP-C, eq for HiPDLP
    i = pairs.index((2.5, SC.BELOW)); assert P.row_kind[i] == 3               # ranged, one side one ulp inside
    i = pairs.index((2.5, 1e20)); assert P.row_kind[i] == 2 and H.row_kind[i] == 3
    i = pairs.index((-1e20, 1e20)); assert P.row_kind[i] == 3 and H.row_kind[i] == 3  # free for one form, ranged for the other
    # the column clamps of the cuPDLP-C form: beyond +-1e20 is infinite, +-1e20 itself is not
    j = pairs.index((-1e20, 1e20)); assert P.lower[j] != -np.inf and P.upper[j] != np.inf
    j = pairs.index((-SC.ABOVE, SC.ABOVE)); assert P.lower[j] == -np.inf and P.upper[j] == np.inf and np.isfinite(H.lower[j])
    # the slack column of a ranged row takes the row's bounds through the same clamps
    assert P.n == lp.num_col + int((P.row_kind == 3).sum()) and H.n == lp.num_col + int((H.row_kind >= 3).sum()) and P.n != H.n


def test_zeros_keep_their_slots_and_scale_by_one():
    lp = SC.case("kinds_zeros")
    P = solver.Prepared(lp)
    assert np.all(np.diff(lp.a_start)[:5] == 0) and np.all(lp.a_value[lp.a_start[5]:lp.a_start[6]] == 0.0) and lp.a_start[6] - lp.a_start[5] == 5
    assert P.nnz == lp.num_nz + int((P.row_kind == 3).sum())  # no stored zero dropped
    assert np.all(P.col_scale[:6] == 1.0)  # empty columns and the all-zero one
    rows = P.row_new_idx[[0, 1, 2, 3, 4, 10]]
    assert np.all(P.row_scale[rows[[1, 2]]] == 1.0) and np.all(P.row_scale[rows[5]] == 1.0)  # empty `>=` / `<=` rows, the all-zero row
    r10 = rows[5]
    assert P.csr_beg[r10 + 1] - P.csr_beg[r10] == 4 and np.all(P.csr_val[P.csr_beg[r10]:P.csr_beg[r10 + 1]] == 0.0)
    kinds_of_empty = [SC.ROW_KINDS[i % 5] for i in range(5)]
    assert sorted(kinds_of_empty) == sorted(SC.ROW_KINDS)


def test_qp_and_maximise_cases():
    q = SC.case("kinds_qp").hessian_diagonal()
    assert (q == 0).sum() > 10 and (q > 0).sum() > 10
    lp = SC.case("kinds_maximise")
    assert lp.sense == -1 and lp.offset == -7.5
    P = solver.Prepared(lp, pdlp_features_off=1)
    assert same_bits(P.cost[:lp.num_col], -lp.col_cost) and np.signbit(P.cost[0]) and not np.signbit(P.cost[3])


def test_absmax_tail_case_puts_the_norm_in_the_last_partial():
    lp = SC.absmax_tail()
    P = solver.Prepared(lp, pdlp_features_off=1)
    assert P.nnz == lp.num_nz > 1023 * 256 + (SC.ABSMAX_SLOT - 1023 * 256) and 0 <= SC.ABSMAX_SLOT - 1023 * 256 < 256
    assert P.mat_norm_inf == 100.0 and np.abs(np.delete(lp.a_value, SC.ABSMAX_SLOT)).max() < 100.0
    assert np.array_equal(P.csc_idx, lp.a_index) and bits(P.csc_val)[SC.ABSMAX_SLOT] == bits(np.array([100.0]))[0]  # the slot keeps its place


# ---- layout cases ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prepared():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = solver.Prepared(SC.case(name), pdlp_features_off=1)
        return cache[name]
    return get


def operand(P, which):
    return (P.csr_beg, P.csr_idx, P.csr_val, P.m, P.n) if which == 0 else (P.csc_beg, P.csc_idx, P.csc_val, P.n, P.m)


@pytest.mark.parametrize("name", sorted(SC.LAYOUT))
def test_layout_cases_keep_their_majors_and_the_host_layout_is_the_restated_one(name, prepared):
    lp, P = SC.case(name), prepared(name)
    assert lp.num_nz < 2**20
    if name != "layout_width_few_tiles":  # `<=` rows and boxed columns only: no slack column, no permutation
        assert (P.n, P.m, P.nnz, P.n_eqs) == (lp.num_col, lp.num_row, lp.num_nz, 0) and np.array_equal(P.row_new_idx, np.arange(P.m))
        assert np.array_equal(P.csc_beg, lp.a_start) and np.array_equal(P.csc_idx, lp.a_index)
    for which in (0, 1):
        beg, idx, val, n_major, n_minor = operand(P, which)
        nb, mb, wb, cold = R.partition(beg, idx, n_major, n_minor, which)
        sl = P.slab_layout(which)  # the product's host build at the default width
        assert (nb, mb) == (sl["n_blocks"], sl["minor_bits"]) and np.array_equal(wb, sl["wave_beg"])
        ref = R.slab_layout(beg, idx, val, n_major, n_minor, wb, mb, 17)
        assert np.array_equal(ref["wave_ptr"], sl["wave_ptr"]) and np.array_equal(ref["ent"], sl["ent"]) and same_bits(ref["slab_val"], sl["val"])
        assert np.array_equal(ref["long_map"], sl["long_map"]) and np.array_equal(ref["long_mask"][:len(sl["long_mask"])], sl["long_mask"])  # (Prepared reads n // 32 + 1 words)
        tp = P.task_plan(which)
        lo, hi, cnt, hist, tl = R.block_spans(beg, idx, wb, n_minor)
        own, _ = R.tile_owners(hist)
        assert tl == tp["tile_log2"] and np.array_equal(own, tp["tile_owner"])


@pytest.mark.parametrize("m,blocks", [(31, 1), (32, 1), (33, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 2), (511, 2),
                                      (513, 3), (2303, 9), (2305, 10), (4351, 17), (4353, 18), (65537, 256)])
def test_major_counts_give_the_blocks_they_are_there_for(m, blocks, prepared):
    P = prepared("layout_m%d" % m)
    sl = P.slab_layout(0)
    assert sl["n_blocks"] == blocks == max(1, min(256, -(-m // 256))) and len(sl["long_mask"]) == m // 32 + 1
    qlo, rr = blocks // 8, blocks % 8
    if m in (2303, 2305):
        assert (qlo, rr) in ((1, 1), (1, 2))   # one block per XCD and a rest: both branches of the block -> XCD formula
    if m in (4351, 4353):
        assert (qlo, rr) == (2, {4351: 1, 4353: 2}[m])
    if m == 65537:
        assert P.nnz == 4 * m >= 200000 and sl["rows_per_block"] > 256
    assert [R.xcd_of_block(b, blocks) for b in range(blocks)] == sorted(R.xcd_of_block(b, blocks) for b in range(blocks))
    assert np.bincount([R.xcd_of_block(b, blocks) for b in range(blocks)], minlength=8).max() == qlo + (1 if rr else 0)


def test_long_major_cases(prepared):
    P = prepared("layout_long_positions")
    lens = np.diff(P.csr_beg)
    assert np.array_equal(np.nonzero(lens > 256)[0], [0, 31, 32, 40, 41, 63]) and set(lens[[1, 30, 42]]) == {255} and set(lens[[2, 33, 62]]) == {256}
    sl = P.slab_layout(0)
    assert np.array_equal(sl["long_map"], [0, 31, 32, 40, 41, 63]) and list(sl["long_mask"]) == [0x80000001, 0x80000301, 0]
    assert len(sl["ent"]) == P.nnz - 6 * 257
    N = prepared("layout_no_long")
    assert np.diff(N.csr_beg).max() == 256 and len(N.slab_layout(0)["long_map"]) == 0 and len(N.slab_layout(0)["ent"]) == N.nnz
    A = prepared("layout_all_long")
    assert np.all(np.diff(A.csr_beg) == 257) and len(A.slab_layout(0)["ent"]) == 0 and np.all(np.diff(A.slab_layout(0)["wave_ptr"]) == 0)
    assert np.diff(A.csc_beg).max() <= 256 and len(A.slab_layout(1)["ent"]) == A.nnz
    E = prepared("layout_empty_waves")
    sl = E.slab_layout(0)
    wb, wp = sl["wave_beg"], sl["wave_ptr"]
    assert np.all(np.diff(E.csr_beg)[20:220] == 0)  # a run of far more than 16 empty majors
    assert np.any((np.diff(wb) > 0) & (np.diff(wp) == 0))  # a wave of empty rows only
    assert np.any(np.diff(wb) == 0)                        # a wave with no row at all: wave_beg repeats


@pytest.mark.parametrize("name,n_minor,W,slabs", [("layout_minor_131071", 131071, 17, 1), ("layout_minor_131072", 131072, 17, 1),
                                                  ("layout_minor_131073", 131073, 17, 2), ("layout_minor_w12_4096", 4096, 12, 1),
                                                  ("layout_minor_w12_4097", 4097, 12, 2), ("layout_minor_w12_131071", 131071, 12, 32),
                                                  ("layout_minor_w12_131072", 131072, 12, 32), ("layout_minor_w12_131073", 131073, 12, 33)])
def test_minor_counts_sit_on_the_slab_boundary(name, n_minor, W, slabs, prepared):
    P = prepared(name)
    assert P.n == n_minor and int(SC.layout_env(name).get("PDLP_MI355X_SLAB_W", 17)) == W
    assert len(set((P.csr_idx >> W).tolist())) == slabs == -(-n_minor // (1 << W))  # every slab is gathered from
    assert P.csr_idx.max() == n_minor - 1 and P.csr_idx.min() == 0
    lo, hi, cnt, hist, tl = R.block_spans(P.csr_beg, P.csr_idx, P.slab_layout(0)["wave_beg"], P.n)
    if "w12" not in name:
        assert R.slab_width(lo, hi, cnt) == 17  # the rule's own width, where none is forced


def test_cold_case_counts_and_moves_a_boundary(prepared):
    P = prepared("layout_cold")
    assert (P.m, P.n) == (SC.COLD_M, SC.COLD_N)
    count = np.bincount(P.csr_idx, minlength=P.n)
    assert count[SC.COLD_F64] == 64 and count[SC.COLD_F65] == 65
    cold = R._cold_counts(P.csr_beg, P.csr_idx, P.n, 256)
    assert np.all(cold[:64] == 1) and np.all(cold[100:165] == 0)          # 64 majors touch it: cold; 65: hot
    assert np.all(cold[200:210] == 0) and np.all(cold[300:310] == 1)      # 2^17 - 1 away: near; 2^17: far
    assert list(cold[400:406]) == [0, 0, 1, 1, 3, 0]                      # lengths 1, 1, 2, 2, 256, 257 (long: never cold)
    lens = np.diff(P.csr_beg)
    assert list(lens[400:406]) == [1, 1, 2, 2, 256, 257]
    nb, mb, wb, _ = R.partition(P.csr_beg, P.csr_idx, P.m, P.n, 0)
    nb0, _, wb0, _ = R.partition(P.csr_beg, P.csr_idx, P.m, P.n, 0, cold=False)
    assert nb == nb0 == 12 and not np.array_equal(wb[::16], wb0[::16])    # the cold counts moved a BLOCK boundary
    assert np.array_equal(wb, P.slab_layout(0)["wave_beg"])


def test_owner_case_fills_both_ways_and_the_vote_matters(prepared):
    P = prepared("layout_owners")
    sl = P.slab_layout(0)
    lo, hi, cnt, hist, tl = R.block_spans(P.csr_beg, P.csr_idx, sl["wave_beg"], P.n)
    own, rule = R.tile_owners(hist)
    assert sl["n_blocks"] == 16 and tl == 14 and hist.shape[1] == 10
    assert rule == ["right", "own", "own", "own", "left", "own", "own", "own", "own", "own"]
    assert list(own) == [0, 0, 1, 2, 2, 3, 4, 5, 6, 7] and len(set(own.tolist())) >= 5
    T = P.task_plan(0)
    assert np.array_equal(T["tile_owner"], own) and T["n_long"] == 4
    lb, li = T["long_beg"], T["long_idx"]

    def votes(p0, p1):
        return np.bincount(own[li[[p0 + ((2 * k + 1) * (p1 - p0)) // 16 for k in range(8)]] >> tl], minlength=8)
    assert list(votes(lb[0], lb[0] + 512)[[1, 5]]) == [5, 3] and list(votes(lb[1], lb[1] + 512)[[2, 6]]) == [4, 4]
    tk = T["tasks"]
    real = tk[tk[:, 2] >= 0]
    assert len(real) == 8 and np.all(real[:, 4] == 2)  # two segments per long row


def test_width_rule_verdicts(prepared):
    want = {"layout_width_few_tiles": 14, "layout_width_random": 17, "layout_width_near_true": 14, "layout_width_near_false": 17}
    margins = {}
    for name, W in want.items():
        P = prepared(name)
        lo, hi, cnt, hist, tl = R.block_spans(P.csr_beg, P.csr_idx, P.slab_layout(0)["wave_beg"], P.n)
        margins[name] = R.few_tiles_margin(lo, hi, cnt)
        assert R.slab_width(lo, hi, cnt) == W, name
    assert margins["layout_width_near_true"][0] == 0            # good * 5 == all * 4: on the boundary, the true side
    assert margins["layout_width_near_false"][0] == -4          # one entry beyond it
