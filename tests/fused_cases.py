"""Generated LPs whose LAST block of the A' partition owns an exact number T of columns, for the tail of the fused A'y+ launch
(k_spmv_slab<kAtyFused, TWO, CC, ULO>: decision, deferred xSum update, the next trial's primal step), whose structure depends
on the columns per block — tests/test_fused_cases_host.py and tests/test_gpu_fused_tail.py.  Fixed seeds, nothing read from
disk.  Only `<=` rows, so that formulation adds no slack column and column j is major j of A'.

Construction: b groups of k heavy columns of L entries each, then T one-entry columns.  The slab partition cuts
ceil(n / 256) blocks and fills them by work, len + len min(len, 64) / 32 + 10 per column (10 for a long one, whose entries are
summed by segment tasks).  With L the smallest length for which k heavy columns outweigh the T cheap ones and b chosen so that
ceil((k b + T) / 256) = b + 1, every heavy block takes k columns and the last block the T cheap ones.  For a few T that rule
lands one column off, so L (and k) are SEARCHED on a restatement of the partition until the last block has exactly T columns;
the host test asserts the planner's own answer.

  variant                    columns stepped from registers         beyond
  LATE (no task workgroups)  4 + 4 per thread = 8192                tail loop, 2048 per round trip
  TWO (co-task workgroups)   2 per thread = 2048                    tail loop, 3072 per round trip"""
import numpy as np

from highs_amd import lp as L

INF = float("inf")
LONG_LIMIT = 256        # more entries than this: a long major (segment tasks)
THREADS = 1024          # threads of a block of the fused launch
REGS = {"LATE": 8 * THREADS, "TWO": 2 * THREADS}  # columns of a block stepped from registers
LONG_LEN = 600


def major_work(lens):
    """pdlp_host.cpp slabMajorWork without cold entries (none here: every minor index is below 2^17)."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens > LONG_LIMIT, 10, lens + lens * np.minimum(lens, 64) // 32 + 10)


def block_starts(lens):
    """The block level of slabPartition restated: ceil(n / 256) blocks (at most 256, at most 16384 majors each), filled by
    work; a major is taken while the block is closer to its target with it than without, every block keeps one."""
    cost = major_work(lens)
    n = len(cost)
    nb = max(min((n + 255) // 256, 256), (n + 16383) // 16384)
    pre = np.concatenate([[0], np.cumsum(cost)])
    out, r = [0], 0
    for u in range(nb):
        left = nb - u
        rem = int(pre[n] - pre[r])
        target = (rem + left - 1) // left
        rows = n - r
        lo = max(1 if rows > 0 else 0, rows - (left - 1) * 16384)
        hi = min(16384, max(rows - (left - 1), 1))
        cnt = lo
        if lo < hi:
            stop = 2 * (pre[r + lo:r + hi] - pre[r]) + cost[r + lo:r + hi] > 2 * target
            cnt = lo + (int(np.argmax(stop)) if stop.any() else hi - lo)
        r += cnt
        out.append(r)
    return np.array(out)


def _plan(T, long_cols, ks):
    """(k, b, L) for which the last block is exactly the T cheap columns — searched, never a neighbour."""
    for k in ks:
        for b in [b for b in range(1, 256) if (k * b + T + 255) // 256 == b + 1][:2]:
            first = next((l for l in range(1, LONG_LIMIT + 1) if k * int(major_work([l])[0]) > 11 * T), None)
            if first is None:  # (k heavy columns cannot outweigh the cheap ones)
                break
            for length in range(first, min(first + 24, LONG_LIMIT) + 1):
                lens = np.concatenate([np.full(k * b, length), np.ones(T, dtype=np.int64)])
                for j in long_cols:
                    lens[j] = LONG_LEN
                cut = block_starts(lens)
                if cut[-2] == k * b and cut[-1] - cut[-2] == T:
                    return k, b, length
    raise AssertionError("no construction with a last block of exactly %d columns" % T)


# Bound patterns of the LAST block's columns (every other block: 0 <= x <= 1).  Scaling multiplies a bound by its column's
# factor, so that only 0 and +-inf stay uniform: a scaled 0..1 block has uniform LOWER bounds only; the patterns with finite
# non-zero uniform bounds (UNSCALED) run with pdlp_features_off = 1.
#   box            0..1                                          -> bit 0 (scaled: the upper bounds differ), lowerUniform
#   nonneg         0..inf                                        -> bits 3, lowerUniform
#   box37          -0.75..1.5 on EVERY column, unscaled          -> bits 3, lowerUniform with a non-zero scalar
#   upper_uniform  random lowers, no upper bound                 -> bit 1
#   lower_uniform  0..random uppers                              -> bit 0, lowerUniform
#   free           -inf..inf (a uniform infinite bound)          -> bits 3, not lowerUniform
#   fixed          l == u == 0.25, unscaled                      -> bits 3, not lowerUniform
#   signed_zero    lower bounds -0.0 / +0.0 mixed, no upper      -> bit 1: equal numbers, different bit patterns
#   odd_first / odd_last / odd_tail: 0..inf but for ONE column (0.125..0.875) at the block's first column (the one the
#                  block's scalars are taken from), at its last, in a tail-loop round -> bits 0
#   odd_elsewhere  0..inf, the one differing column in the FIRST block -> bits 3 here, not lowerUniform
BOUNDS = ("box", "nonneg", "upper_uniform", "lower_uniform", "free", "fixed", "signed_zero",
          "odd_first", "odd_last", "odd_tail", "odd_elsewhere", "box37")
UNSCALED = ("fixed", "box37")
LAST_BITS = {"box": 1, "nonneg": 3, "box37": 3, "upper_uniform": 2, "lower_uniform": 1, "free": 3, "fixed": 3, "signed_zero": 2,
             "odd_first": 0, "odd_last": 0, "odd_tail": 0, "odd_elsewhere": 3}
LOWER_UNIFORM = ("box", "nonneg", "box37", "lower_uniform")


def _apply_bounds(kind, lo, up, cost, sign, first, T, regs, rng):
    """Bounds by pattern (above).  The cost of a column without a lower (upper) bound gets the sign that keeps the LP bounded
    in that direction."""
    blk = slice(first, first + T)
    odd = None
    if kind == "box":
        pass
    elif kind == "nonneg":
        up[blk] = INF
    elif kind == "box37":
        lo[:], up[:] = -0.75, 1.5
    elif kind == "upper_uniform":
        lo[blk], up[blk] = -rng.uniform(0.0, 1.0, T), INF
    elif kind == "lower_uniform":
        up[blk] = rng.uniform(0.5, 1.5, T)
    elif kind == "free":
        lo[blk], up[blk] = -INF, INF
    elif kind == "fixed":
        lo[blk] = up[blk] = 0.25
    elif kind == "signed_zero":
        lo[blk], up[blk] = np.where(rng.random(T) < 0.5, -0.0, 0.0), INF
        lo[first], lo[first + 1] = 0.0, -0.0
    elif kind in ("odd_first", "odd_last", "odd_tail", "odd_elsewhere"):
        up[blk] = INF
        odd = {"odd_first": first, "odd_last": first + T - 1, "odd_tail": first + regs + 3, "odd_elsewhere": 3}[kind]
        assert kind != "odd_tail" or regs + 3 < T - 1  # a column of the tail loop that is not the block's last
        lo[odd], up[odd] = 0.125, 0.875
    else:
        raise ValueError(kind)
    cost[:] = np.where(np.isinf(lo) & np.isinf(up), -sign * np.abs(cost), np.where(np.isinf(up), np.abs(cost), np.where(np.isinf(lo), -np.abs(cost), cost)))


KS = (128, 129, 132, 140)  # heavy columns per group, tried in this order


def tail_block(T, long_cols=(), bounds="box", qdiag=False, seed=31, variant=None):
    """An LP whose last block of the A' partition owns exactly T columns (module docstring).
    long_cols: columns made long (LONG_LEN = 600 entries); an index >= 0 counts from the first column (a heavy one), an index
    < 0 from the last (a cheap one).  bounds: one of BOUNDS / "box37" on the last block.  qdiag: a diagonal Hessian with about
    a third of its entries zero.  variant: "LATE" / "TWO" — only where "odd_tail" needs to know the register-held columns
    (default: TWO with long columns, else LATE).
    lp.fused: what was built — k, b, L, first column of the last block, T, long columns (absolute)."""
    regs = REGS[variant or ("TWO" if long_cols else "LATE")]
    rng = np.random.default_rng(seed + T)
    # (the long columns' positions need n, which needs b: heavy ones are absolute, cheap ones relative to the end — plan with
    # the relative form, which numpy's indexing takes as it is)
    k, b, length = _plan(T, long_cols, KS)
    n, first = k * b + T, k * b
    longs = sorted(j % n for j in long_cols)
    lens = np.concatenate([np.full(first, length), np.ones(T, dtype=np.int64)])
    lens[longs] = LONG_LEN
    nnz = int(lens.sum())
    m = 64 if nnz < 4096 else 4096 if nnz < 400_000 else 8192 if nnz < 900_000 else 16384 if nnz < 1_900_000 else 32768
    # entries of column j: rows (s_j + i step_j) mod m, step_j odd and m a power of two, so they are distinct and the rows
    # fill evenly
    a_start = np.concatenate([[0], np.cumsum(lens)])
    col = np.repeat(np.arange(n), lens)
    within = np.arange(nnz) - a_start[col]
    start, step = rng.integers(0, m, n), 2 * rng.integers(0, m // 2, n) + 1
    rows = (start[col] + within * step[col]) % m
    order = np.lexsort((rows, col))  # ascending row order inside a column
    rows = rows[order]
    val = rng.standard_normal(nnz)
    row_len = np.bincount(rows, minlength=m)
    assert row_len.max() <= LONG_LIMIT, ("a row of A is long", int(row_len.max()))
    cost = rng.standard_normal(n)
    cost[cost == 0.0] = 1.0
    lo, up = np.zeros(n), np.ones(n)
    sign = np.sign(val[a_start[:-1]])  # (of a cheap column's only entry)
    _apply_bounds(bounds, lo, up, cost, sign, first, T, regs, rng)
    x0 = np.clip(rng.uniform(0.2, 0.8, n), np.where(np.isinf(lo), -1.0, lo), np.where(np.isinf(up), 2.0, up))
    act = np.zeros(m)
    np.add.at(act, rows, val * x0[col])
    lp = L.HighsLp(n, m, cost, lo, up, np.full(m, -INF), act + rng.uniform(0.1, 1.0, m), a_start, rows, val, 1, 0.0,
                   "tail%d%s_%s" % (T, "L" * bool(longs), bounds)).normalise()
    if qdiag:
        lp.set_diagonal_hessian(np.where(rng.random(n) < 1 / 3, 0.0, rng.uniform(0.2, 2.0, n)))
    lp.fused = dict(k=k, b=b, L=length, first=first, T=T, long_cols=longs, rows_longest=int(row_len.max()))
    return lp


def options(bounds):
    """Solver options of a case: the patterns with finite non-zero uniform bounds run without scaling."""
    return dict(pdlp_features_off=1) if bounds in UNSCALED else {}


# ---- what the device derives from the bounds, restated ----------------------------------------------------------------------
def block_uniform_bits(lower, upper, block_beg):
    """Per block of A' (block_beg: first column of every block, then n): bit 0 — every lower bound of the block has the bit
    pattern of the block's first column, bit 1 — the same for the upper bounds; and lowerUniform — every block has bit 0 and
    all of them the same lower bound, bit for bit.  From the prepared (scaled) bounds."""
    lb, ub = np.ascontiguousarray(lower).view(np.uint64), np.ascontiguousarray(upper).view(np.uint64)
    bits = np.zeros(len(block_beg) - 1, dtype=np.int64)
    for i, (c0, c1) in enumerate(zip(block_beg[:-1], block_beg[1:])):
        if c1 > c0:
            bits[i] = int(np.all(lb[c0:c1] == lb[c0])) | (int(np.all(ub[c0:c1] == ub[c0])) << 1)
    nonempty = block_beg[:-1][np.diff(block_beg) > 0]
    all_lower = bool(np.all(bits & 1) and np.all(lb[nonempty] == lb[0]))
    cols = np.diff(block_beg)
    return bits, all_lower, int(cols[(bits & 1) != 0].sum()), int(cols[(bits & 2) != 0].sum())


def tail_step(x, aty, cost, lower, upper, tau, qdiag=None):
    """The next trial's primal step, element by element in the kernel's operation order (no contraction): float64 numpy."""
    t = x + (-tau) * cost
    t = t + tau * aty
    if qdiag is not None:
        t = t / (1.0 + tau * qdiag)
    t = np.where(t < upper, t, upper)
    t = np.where(t > lower, t, lower)
    return t


# ---- the cases --------------------------------------------------------------------------------------------------------------
# T of the LATE variant: threads without a column (the prefetch clamped to the block's last column); 4 and 4 + 1 columns per
# thread (kSlabPre: the first column from xbLate[], qdiag reloaded); 8 and 8 + 1 (the first column of the tail loop).
# T = 10241 (a second tail-loop round) is NOT built: 6.6 M nonzeros, several seconds per solver on the device.
LATE_T = (128, 4096, 4097, 8192, 8193)
# T of the TWO variant (one long column in the first heavy block, one as the last cheap column, which the tail loop steps
# from T = 2049 on): 2 and 2 + 1 columns per thread; 2 + 3 and 2 + 3 + 1 (a second tail-loop round)
TWO_T = (2048, 2049, 5120, 5121)
TWO_LONG = (5, -1)
ITER_CAP = 120
SOLVE = dict(kkt_tolerance=1e-9, pdlp_iteration_limit=ITER_CAP)


# sizeof(DevState) (pdlp_kernels.hpp), part of the launch's LDS request.  Stage "fused_form" reports it in [8] and
# tests/test_gpu_fused_tail.py compares: a grown record moves TWO_MAX, and the failure then names the size.
STATE_BYTES = 192


def two_lds_limit(lds_per_cu=160 * 1024):
    """The largest rowsPerBlock of A' at which two 1024-thread blocks of the fused launch fit a CU's LDS, so that the TWO
    variant runs (fusedLds: even(rowsPerBlock) * 8 + 1024 * 8 + 2 * 16 * 8 + 4 * 4 * 8 + sizeof(DevState) + 16 bytes, twice
    within 160 KiB): 9142.  One column more and fusedCoTaskBlocks returns 0 — the long columns go inline into LATE."""
    fixed = THREADS * 8 + 2 * (THREADS // 64) * 8 + 4 * (256 // 64) * 8 + STATE_BYTES + 16
    return ((lds_per_cu // 2 - fixed) // 8) & ~1


TWO_MAX = two_lds_limit()

# name -> (T, variant, bounds, qdiag, seed).  The variant is what the case is BUILT for; tests/test_gpu_fused_tail.py asserts
# through stage "fused_form" that the device runs it.  Every seed was picked with the oracle alone so that the run capped at
# ITER_CAP iterations holds a rejected trial and a restart (asserted in tests/test_fused_cases_host.py).
CASES = {}
for _T in LATE_T:  # (8192 with seed 31: the oracle's 120 iterations hold no rejected trial)
    CASES["late%d" % _T] = (_T, "LATE", "box", False, 32 if _T == 8192 else 31)
for _T in TWO_T + (TWO_MAX,):
    CASES["two%d" % _T] = (_T, "TWO", "box", False, 31)
CASES["inline%d" % (TWO_MAX + 1)] = (TWO_MAX + 1, "LATE", "box", False, 31)  # (built like a TWO case, runs inline in LATE)
PATTERN_T = {"LATE": 8193, "TWO": 5121}  # the T with a tail loop that carry every bound pattern
for _v, _T in PATTERN_T.items():
    for _b in BOUNDS[1:]:
        # (at 8193 the only column of the tail loop is the block's last one, which is odd_last: odd_tail takes 8200)
        _Tb = 8200 if (_v, _b) == ("LATE", "odd_tail") else _T
        CASES["%s%d_%s" % (_v.lower(), _Tb, _b)] = (_Tb, _v, _b, False, 31)
CASES["late8193_q"] = (8193, "LATE", "box", True, 31)
CASES["two2049_q"] = (2049, "TWO", "box", True, 31)
HAS_LONG = {name for name, c in CASES.items() if c[1] == "TWO" or name.startswith("inline")}

_made = {}


def case(name):
    """(lp, solver options) of a case, made once per process."""
    if name not in _made:
        T, variant, bounds, qdiag, seed = CASES[name]
        _made[name] = (tail_block(T, TWO_LONG if name in HAS_LONG else (), bounds, qdiag, seed=seed, variant=variant), options(bounds))
    return _made[name]
