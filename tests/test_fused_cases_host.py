"""The structural claims of tests/fused_cases.py, proven on the host planner (no GPU), and the oracle's run on every case:

1. the last block of the A' partition owns exactly T columns — Prepared.slab_layout(1), the planner's own answer — and the
   restatement of the partition that the generator searches on gives the same blocks;
2. the long columns are where they were put (one in the first heavy block, one the block's last column);
3. the per-block uniform-bound bits and lowerUniform, restated from Prepared.lower / upper by bit pattern, are what the
   pattern was built to give (tests/test_gpu_fused_tail.py compares the restatement with what the device computed);
4. the oracle alone, in the device's reduction order on the slab layout, kkt_tolerance 1e-9, capped at 120 iterations, holds a
   rejected trial and a restart on every case."""
import numpy as np
import pytest

import fused_cases as F
import oraclelib as O
from highs_amd import solver

NAMES = sorted(F.CASES)


def _prepared(name):
    lp, opt = F.case(name)
    return lp, opt, solver.Prepared(lp, **opt)


@pytest.mark.parametrize("name", NAMES)
def test_blocks_long_columns_and_uniform_bits(name):
    lp, opt, P = _prepared(name)
    T, variant, bounds, qdiag, _ = F.CASES[name]
    info = lp.fused
    assert (P.n, P.m, P.nnz) == (lp.num_col, lp.num_row, lp.num_nz)  # no slack column: column j is major j of A'
    S = P.slab_layout(1)
    cut = S["wave_beg"][::16]
    cols = np.diff(cut)
    print(name, "k", info["k"], "b", info["b"], "L", info["L"], "n", P.n, "m", P.m, "nnz", P.nnz, "longest row", info["rows_longest"],
          "blocks", len(cols), "columns of the last block", cols[-1], "of the others", sorted(set(cols[:-1].tolist())))
    # 1
    assert cols[-1] == T and cut[-2] == info["first"] and S["rows_per_block"] == max(T, cols.max())
    assert np.array_equal(cut, F.block_starts(np.diff(P.csc_beg)))
    assert np.diff(P.csr_beg).max() <= F.LONG_LIMIT  # A has no long row
    # 2
    longs = np.nonzero(np.diff(P.csc_beg) > F.LONG_LIMIT)[0]
    assert np.array_equal(longs, info["long_cols"])
    mask = S["long_mask"]
    assert np.array_equal(np.nonzero([(mask[j >> 5] >> (j & 31)) & 1 for j in range(P.n)])[0], longs)
    if name in F.HAS_LONG:
        assert longs[0] == 5 and longs[0] < cut[1] and longs[1] == P.n - 1
        if T > F.REGS[variant]:
            assert longs[1] - cut[-2] >= F.REGS[variant]  # the tail loop steps it
    else:
        assert len(longs) == 0
    # 3
    bits, all_lower, nlo, nup = F.block_uniform_bits(P.lower, P.upper, cut)
    print(name, "uniform bits of the last block", bits[-1], "of the others", sorted(set(bits[:-1].tolist())), "lowerUniform", int(all_lower))
    unscaled = bounds in F.UNSCALED
    assert bits[-1] == F.LAST_BITS[bounds]
    assert all_lower == (bounds in F.LOWER_UNIFORM)
    # (the other blocks hold 0..1: scaled, their upper bounds differ)
    assert np.all(bits[1:-1] == (3 if unscaled else 1)) and bits[0] == (0 if bounds == "odd_elsewhere" else bits[1])
    if bounds == "free":
        assert np.all(np.isneginf(P.lower[cut[-2]:])) and np.all(np.isposinf(P.upper[cut[-2]:]))
    if bounds == "signed_zero":
        blk = P.lower[cut[-2]:]
        assert np.all(blk == 0.0) and 0 < np.signbit(blk).sum() < T
    if bounds in F.UNSCALED:
        assert np.array_equal(P.lower, lp.col_lower) and np.array_equal(P.upper, lp.col_upper)
    assert (nlo, nup) == (int(cols[(bits & 1) != 0].sum()), int(cols[(bits & 2) != 0].sum()))
    assert (lp.hessian is not None) == qdiag
    if qdiag:
        q = lp.hessian_diagonal()
        assert 0.2 < np.mean(q == 0.0) < 0.45


@pytest.mark.parametrize("name", NAMES)
def test_oracle_run_holds_a_rejected_trial_and_a_restart(name):
    lp, opt = F.case(name)
    cpu = O.oracle_solve(lp, device_reduction_order=True, device_layout="slab", **F.SOLVE, **opt)
    print(name, "oracle: iterations", cpu.num_iter, "trials", cpu.num_trials, "restarts", cpu.num_restarts, "term", cpu.term_code)
    assert cpu.num_trials > cpu.num_iter and cpu.num_restarts >= 1


def test_the_two_variant_ends_at_its_lds_bound():
    # fusedLds at rowsPerBlock = TWO_MAX fills half of the 160 KiB exactly; one more (rounded up to even) does not fit twice
    lds = lambda rows: ((rows + 1) & ~1) * 8 + 1024 * 8 + 2 * 16 * 8 + 4 * 4 * 8 + F.STATE_BYTES + 16
    assert 2 * lds(F.TWO_MAX) <= 160 * 1024 < 2 * lds(F.TWO_MAX + 1)
    assert F.CASES["two%d" % F.TWO_MAX][0] == F.TWO_MAX and F.CASES["inline%d" % (F.TWO_MAX + 1)][0] == F.TWO_MAX + 1
