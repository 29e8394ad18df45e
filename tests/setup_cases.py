"""Generated problems on the edges of the SET-UP itself (formulate, scale, transpose, slab layout: pdlp_host.cpp on the host,
pdlp_setup.hip / DeviceMatrix::buildFromDevice / k_block_span on the device), for tests/test_setup_cases_host.py and
tests/test_gpu_setup_cases.py: fixed seeds, nothing read from disk.

kinds_*: what formulation decides — every row kind and column kind, bounds on the 1e20 / infinity thresholds, stored zeros,
empty rows and columns, the objective sense, a diagonal Hessian; row counts on each side of one 256-thread block and of the
scans' tiles.  layout_*: what the layout build decides and no sum shows — block and wave boundaries, cold counts, long
majors, slab boundaries, tile owners, the slab width.  These use `<=` rows and boxed columns only, so majors keep their
numbers: major r of the prepared A is row r here, major j of A' is column j."""
import functools

import numpy as np

from highs_amd import lp as L
from edge_cases import _lp_from_rows, _pick

INF = float("inf")
BIG = 1e20
BELOW, ABOVE = float(np.nextafter(1e20, 0.0)), float(np.nextafter(1e20, INF))
ROW_KINDS = ("eq", "ge", "le", "ranged", "free")
COL_KINDS = ("free", "lower", "upper", "boxed", "fixed")


def _lp_from_coo(name, n, m, rows, cols, vals, cost, cl, cu, rl, ru, sense=1, offset=0.0):
    """Column-wise storage with ascending rows inside a column; explicit zeros keep their slots."""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows), "duplicate entry"
    order = np.lexsort((rows, cols))
    a_start = np.zeros(n + 1, dtype=np.int32)
    a_start[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return L.HighsLp(n, m, np.asarray(cost, float), np.asarray(cl, float), np.asarray(cu, float), np.asarray(rl, float),
                     np.asarray(ru, float), a_start, rows[order].astype(np.int32), vals[order], sense, offset, name).normalise()


def _row_bounds(kind, v, w):
    return {"eq": (v, v), "ge": (v, INF), "le": (-INF, v), "ranged": (v, v + abs(w) + 0.5), "free": (-INF, INF)}[kind]


def _col_bounds(kind, v, w):
    return {"free": (-INF, INF), "lower": (v, INF), "upper": (-INF, v), "boxed": (v, v + abs(w) + 0.5), "fixed": (v, v)}[kind]


def kinds(m, row_cycle=ROW_KINDS, seed=1, sense=1, offset=0.0, name=None):
    """m rows whose kinds follow row_cycle, 10 + min(m, 40) columns whose kinds follow COL_KINDS.  Column 0 holds an entry in
    EVERY row (all five kinds: the equality-first order inside a column, `<=` rows negated), column 1 is empty, columns
    2..6 hold one entry, the others 2 to 5.  The costs include 0.0 and -0.0."""
    rng = np.random.default_rng(1000 * seed + m)
    n = 10 + min(m, 40)
    rows, cols = list(range(m)), [0] * m
    for j in range(2, n):
        k = 1 if j <= 6 else min(m, int(rng.integers(2, 6)))
        rr = _pick(rng, np.arange(m), k)
        rows += rr.tolist(); cols += [j] * k
    vals = rng.standard_normal(len(rows))
    rb = [_row_bounds(row_cycle[i % len(row_cycle)], v, w) for i, (v, w) in enumerate(rng.standard_normal((m, 2)))]
    cb = [_col_bounds(COL_KINDS[j % 5], v, w) for j, (v, w) in enumerate(rng.standard_normal((n, 2)))]
    cost = rng.standard_normal(n)
    cost[0], cost[3] = 0.0, -0.0
    return _lp_from_coo(name or "kinds_%d" % m, n, m, rows, cols, vals, cost, [b[0] for b in cb], [b[1] for b in cb],
                        [b[0] for b in rb], [b[1] for b in rb], sense, offset)


THRESHOLD_VALUES = (-INF, -1e30, -ABOVE, -BIG, -BELOW, -1.5, -0.0, 0.0, 2.5, BELOW, BIG, ABOVE, 1e30, INF)


def threshold_pairs():
    """Every (lower, upper) over THRESHOLD_VALUES with lower <= upper, lower < +inf and upper > -inf: +-1e20 exactly, one ulp
    inside and outside, 1e30, +-inf, -0.0 — among them lower == upper (an equality row, also as (-0.0, 0.0); beyond the
    threshold a one-sided or free one) and ranged rows with one side one ulp inside 1e20."""
    return [(a, b) for a in THRESHOLD_VALUES for b in THRESHOLD_VALUES if a <= b and a < INF and b > -INF]


def thresholds(seed=2):
    """One row AND one column per pair of threshold_pairs(); column j holds entries in rows j, 3 j + 1 and 5 j + 2 (mod m).
    Maximised, with an offset, costs with 0.0 and -0.0.  The cuPDLP-C form cuts at 1e20, the HiPDLP form at infinity."""
    rng = np.random.default_rng(seed)
    pairs = threshold_pairs()
    k = len(pairs)
    ent = sorted({(r % k, j) for j in range(k) for r in (j, 3 * j + 1, 5 * j + 2)})
    cost = rng.standard_normal(k)
    cost[0], cost[1] = 0.0, -0.0
    return _lp_from_coo("kinds_thresholds", k, k, [e[0] for e in ent], [e[1] for e in ent], rng.standard_normal(len(ent)), cost,
                        [p[0] for p in pairs], [p[1] for p in pairs], [p[0] for p in pairs], [p[1] for p in pairs], -1, 3.25)


def zeros(seed=3):
    """Rows 0..4: empty, one of every kind.  Columns 0..4: empty, one of every kind.  Column 5: stored entries in rows 5..9
    (one of every kind), all explicit zeros.  Row 10: stored entries in columns 6..9, all explicit zeros.  Rows 5..9 and 11..13
    and columns 6..13 carry ordinary entries.  A zero or empty major scales by 1 and its entries keep their slots."""
    rng = np.random.default_rng(seed)
    m, n = 14, 14
    ent = {(i, 5): 0.0 for i in range(5, 10)}
    ent.update({(10, j): 0.0 for j in range(6, 10)})
    for i in list(range(5, 10)) + [11, 12, 13]:
        for j in _pick(rng, np.arange(6, 14), 4):
            ent[(i, int(j))] = float(rng.standard_normal())
    for j in range(6, 14):  # no ordinary column without an ordinary entry
        ent.setdefault((11 + j % 3, j), float(rng.standard_normal()))
    keys = sorted(ent)
    rb = [_row_bounds(ROW_KINDS[i % 5], v, w) for i, (v, w) in enumerate(rng.standard_normal((m, 2)))]
    cb = [_col_bounds(COL_KINDS[j % 5], v, w) for j, (v, w) in enumerate(rng.standard_normal((n, 2)))]
    return _lp_from_coo("kinds_zeros", n, m, [k[0] for k in keys], [k[1] for k in keys], [ent[k] for k in keys], rng.standard_normal(n),
                        [b[0] for b in cb], [b[1] for b in cb], [b[0] for b in rb], [b[1] for b in rb])


def qp():
    """kinds(257) with a diagonal Hessian of zero and non-zero entries."""
    lp = kinds(257, name="kinds_qp")
    q = np.abs(np.random.default_rng(4).standard_normal(lp.num_col)) + 0.25
    q[::3] = 0.0
    return lp.set_diagonal_hessian(q)


KINDS_SIZES = (1, 5, 255, 256, 257, 1025, 4097)
FORMULATION = {"kinds_%d" % m: functools.partial(kinds, m) for m in KINDS_SIZES}
FORMULATION.update({"kinds_all_" + k: functools.partial(kinds, 300, (k,), 5, name="kinds_all_" + k) for k in ROW_KINDS})
FORMULATION.update(kinds_thresholds=thresholds, kinds_zeros=zeros, kinds_qp=qp,
                   kinds_maximise=functools.partial(kinds, 257, ROW_KINDS, 6, -1, -7.5, "kinds_maximise"))


# ---- layout cases ------------------------------------------------------------------------------------------------------
LONG = 257  # one entry more than the slab layout's limit for a major (pdlp_solver.cpp kSlabLongLimit = 256)


def _random_rows(rng, m, n, k):
    return [_pick(rng, np.arange(n), k) for _ in range(m)]


def majors(m, seed=21):
    """m rows of 4 entries: the mask words (31..65), one / two / three blocks (255..513), 9 and 10 blocks (2303, 2305:
    nBlocks % 8 != 0, one block per XCD and a rest), 17 and 18 (4351, 4353: two per XCD and a rest of one / two), more than 256 blocks' worth of
    256 rows (65 537, over 8 000 columns)."""
    rng = np.random.default_rng(seed + m)
    n = 8000 if m > 60000 else 96
    if m > 60000:  # (thin and cheap to generate: four consecutive columns from a random first one)
        rows = list(rng.integers(0, n - 3, size=m)[:, None] + np.arange(4)[None, :])
    else:
        rows = _random_rows(rng, m, n, 4)
    return _lp_from_rows("layout_m%d" % m, n, rows, rng, "real")


ABSMAX_SLOT, ABSMAX_VALUE = 262000, -100.0


def absmax_tail():
    """majors(65537) with one large coefficient in slot 262 000 of the column-wise values: the device takes max |a_ij| from
    1 024 partial maxima of 256 strided slots each, and only the LAST one sees a slot from 261 888 on."""
    import copy
    lp = copy.copy(majors(65537))
    lp.a_value = lp.a_value.copy()
    lp.a_value[ABSMAX_SLOT] = ABSMAX_VALUE
    lp.model_name = "kinds_absmax_tail"
    return lp


LONG_POSITIONS = {0: LONG, 31: LONG, 32: LONG, 63: LONG, 40: LONG, 41: LONG, 1: 255, 30: 255, 42: 255, 2: 256, 33: 256, 62: 256}


def long_majors(long_len=LONG, seed=22, name="layout_long_positions"):
    """64 rows over 600 columns: rows of 257 entries at 0, 31, 32, the last row and 40 / 41 (adjacent), rows of 255 and 256
    next to them, 3 entries elsewhere.  long_len = 256: the same operand with no long major."""
    rng = np.random.default_rng(seed)
    rows = [_pick(rng, np.arange(600), long_len if LONG_POSITIONS.get(i) == LONG else LONG_POSITIONS.get(i, 3)) for i in range(64)]
    return _lp_from_rows(name, 600, rows, rng, "real")


def all_long(seed=23):
    """40 rows of 257 entries over 300 columns: no short entry at all in A (nnz_short = 0); its columns are short."""
    rng = np.random.default_rng(seed)
    return _lp_from_rows("layout_all_long", 300, _random_rows(rng, 40, 300, LONG), rng, "real")


def empty_waves(seed=24):
    """20 rows of one entry, 200 EMPTY rows, 20 rows of one entry, then one row of 256: waves that hold nothing but empty rows
    (wave_ptr repeats) and, in front of the heavy row, waves that hold no row at all (wave_beg repeats)."""
    rng = np.random.default_rng(seed)
    rows = [_pick(rng, np.arange(400), k) for k in [1] * 20 + [0] * 200 + [1] * 20 + [256]]
    return _lp_from_rows("layout_empty_waves", 400, rows, rng, "real")


def minors(n_minor, seed=25, name=None):
    """300 rows of 20 entries over n_minor columns, the first and the last column and the columns on each side of every
    multiple of 4096 below 2^17 + 1 that exists among them: a slab boundary of A at n_minor = 2^W + 1 and none at 2^W."""
    rng = np.random.default_rng(seed + n_minor)
    edge = sorted({c for c in (0, 4095, 4096, 131071, 131072, n_minor - 1) if c < n_minor})
    rows = []
    for i in range(300):
        own = [edge[i % len(edge)]]
        rows.append(np.unique(np.concatenate([own, _pick(rng, np.arange(n_minor), 19)])))
    return _lp_from_rows(name or "layout_minor_%d" % n_minor, n_minor, rows, rng, "real")


COLD_N, COLD_M = 140000, 3000
COLD_F64, COLD_F65 = 135000, 135001
FAR = 1 << 17


def cold(seed=26):
    """3 000 rows over 140 000 columns; row i holds columns 2 i .. 2 i + 4 and, for
      i in [0, 64):     column 135 000 — touched by exactly 64 rows, 2^17 or more away from the middle entry: COLD;
      i in [100, 165):  column 135 001 — touched by exactly 65 rows: hot, not cold;
      i in [200, 210):  the column exactly 2^17 - 1 beyond the middle entry: near, not cold;
      i in [300, 310):  the column exactly 2^17 beyond it: cold.
    Rows 400 / 401: one entry; 402 / 403: two entries 2^17 apart (the middle entry is the far one: the NEAR one is cold);
    404: 256 entries, 405: 257 (long: never cold), both with far columns."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(COLD_M):
        base = list(range(2 * i, 2 * i + 5))
        mid = 2 * i + 3  # the middle entry of the six
        if i < 64:
            base.append(COLD_F64)
        elif 100 <= i < 165:
            base.append(COLD_F65)
        elif 200 <= i < 210:
            base.append(mid + FAR - 1)
        elif 300 <= i < 310:
            base.append(mid + FAR)
        elif i in (400, 401):
            base = [2 * i]
        elif i in (402, 403):
            base = [2 * i, 2 * i + FAR]
        elif i in (404, 405):
            k = 256 if i == 404 else 257
            base = list(range(2 * i, 2 * i + k - 3)) + [136000 + i, 137000 + i, 138000 + i]
        rows.append(np.array(sorted(base), dtype=np.int64))
    return _lp_from_rows("layout_cold", COLD_N, rows, rng, "real")


OWNER_TILES = (1, 2, 3, 5, 6, 7, 8, 9)  # the tile (2^14 columns) the rows of XCD x gather from; tiles 0 and 4 stay untouched


def owners(seed=27):
    """4 096 rows over 10 tiles of 2^14 columns: 16 blocks, two per XCD; the rows of XCD x hold 8 entries in tile
    OWNER_TILES[x].  Tile 0 (leftmost) and tile 4 (in the middle) are touched by no short row.  The last four rows are long:
    600 entries, 320 in tile 2 then 280 in tile 7 (the first segment's samples vote 5 : 3), 256 in tile 3 then 344 in tile 8
    (4 : 4), and two within tile 9."""
    rng = np.random.default_rng(seed)
    T = 1 << 14
    rows = [_pick(rng, np.arange(OWNER_TILES[i // 512] * T, (OWNER_TILES[i // 512] + 1) * T), 8) for i in range(4092)]
    tile = lambda t, k: _pick(rng, np.arange(t * T, (t + 1) * T), k)
    rows += [np.concatenate([tile(2, 320), tile(7, 280)]), np.concatenate([tile(3, 256), tile(8, 344)]), tile(9, 600), tile(9, 600)]
    return _lp_from_rows("layout_owners", 10 * T, rows, rng, "real")


def width_rule(extra_entries, seed=28):
    """1 280 rows of 8 entries over 6 tiles of 2^14 columns, five blocks of 256 rows.  Blocks 0..3 lie in ONE tile each: 2 048
    entries in 2^14 columns, exactly the density the width rule asks for.  The rows of block 4 alternate between tiles 4 and
    5: too thin.  extra_entries = 0: good * 5 == all * 4, the rule says 2^14 columns per slab; 1: the last row of block 4 holds
    one entry more, good * 5 == all * 4 - 4, it says 2^17."""
    rng = np.random.default_rng(seed)
    T = 1 << 14
    rows = [_pick(rng, np.arange((i // 256) * T, (i // 256 + 1) * T), 8) for i in range(1024)]
    rows += [_pick(rng, np.arange((4 + i % 2) * T, (5 + i % 2) * T), 8 + (extra_entries if i == 255 else 0)) for i in range(256)]
    return _lp_from_rows("layout_width_%s" % ("near_false" if extra_entries else "near_true"), 6 * T, rows, rng, "real")


def width_few_tiles():
    from lpgen import structured_lp
    return structured_lp(seed=2, commodities=12, nodes=1024, arcs=8192, link_rows=24, link_nnz=700, extra_rows=40)


def width_random(seed=29):
    rng = np.random.default_rng(seed)
    return _lp_from_rows("layout_width_random", 40000, _random_rows(rng, 600, 40000, 10), rng, "real")


MAJOR_COUNTS = (31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 2303, 2305, 4351, 4353, 65537)
# name -> (builder, environment on top of PDLP_MI355X_SLAB=1)
LAYOUT = {"layout_m%d" % m: (functools.partial(majors, m), {}) for m in MAJOR_COUNTS}
LAYOUT.update({
    "layout_long_positions": (long_majors, {}),
    "layout_no_long": (functools.partial(long_majors, 256, 22, "layout_no_long"), {}),
    "layout_all_long": (all_long, {}),
    "layout_empty_waves": (empty_waves, {}),
    "layout_cold": (cold, {}),
    "layout_owners": (owners, {}),
    "layout_width_few_tiles": (width_few_tiles, {}),
    "layout_width_random": (width_random, {}),
    "layout_width_near_true": (functools.partial(width_rule, 0), {}),
    "layout_width_near_false": (functools.partial(width_rule, 1), {}),
})
LAYOUT.update({"layout_minor_%d" % k: (functools.partial(minors, k), {}) for k in (FAR - 1, FAR, FAR + 1)})
LAYOUT.update({"layout_minor_w12_%d" % k: (functools.partial(minors, k, 25, "layout_minor_w12_%d" % k), {"PDLP_MI355X_SLAB_W": "12"})
               for k in (4096, 4097, FAR - 1, FAR, FAR + 1)})
# every layout case runs with the slab layout forced and with the block -> XCD map and the pacing named, so that no timing
# chooses anything (tuneXcdMap times operands of 200 000 nonzeros or more otherwise)
LAYOUT_ENV = {"PDLP_MI355X_SLAB": "1", "PDLP_MI355X_XCD_MAP": "1", "PDLP_MI355X_SLAB_PACE": "1"}


@functools.lru_cache(maxsize=None)
def case(name):
    """The LP (or QP) of a case, built once."""
    return FORMULATION[name]() if name in FORMULATION else LAYOUT[name][0]()


def layout_env(name):
    return dict(LAYOUT_ENV, **(LAYOUT[name][1] if name in LAYOUT else {}))
