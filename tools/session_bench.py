#!/usr/bin/env python3
"""session_bench.py — what a re-solve costs before the first iteration through a session (pdlp_mi355x_session_solve, DESIGN.md
section 2f) against the one-shot pdlp_mi355x_solve on the SAME modified problem.

  python tools/session_bench.py [--configs a,b,c] [--reps 5] [--out profiles/session_vs_solve.json]

Per workload (bench configs a: 100k x 100k, b: 1M x 1M synthetic, c: the structured LP) and per path of the ladder
  update         one cost changed                    update_matrix   one matrix value changed
  nothing        the same problem again              create          a row changed its kind
the session holds the problem, takes the modified one and reports pdlp_session_info_t: setup_seconds (everything before
the first iteration), of which upload_seconds (P's arrays from pageable memory into staging), diff_seconds - upload_seconds
(the comparison launch and its record) and apply_seconds (the update from the staged arrays, or the create).  The one-shot
side is pdlp_result_t.setup_seconds of pdlp_mi355x_solve on that problem.  ONE process, one device, `reps` times each
(the problem alternates between the two versions so that every call finds a change), median and all values.  The runs are
cut off after 40 iterations.  Prints one JSON line and writes it to --out.  No threshold is asserted: these are measurements.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import lpgen  # noqa: E402
from highs_amd import abi, solver  # noqa: E402

OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=40)
PATHS = ("update", "update_matrix", "nothing", "create")


def workload(config):
    if config in ("a", "b"):
        m, n, nnz = (100_000, 100_000, 1_000_000) if config == "a" else (1_000_000, 1_000_000, 8_000_000)
        sp = solver.SyntheticProblem(m, n, nnz, 1)
        lp = sp.to_lp()
        sp.close()
        return lp
    if config == "c":
        return lpgen.structured_lp()
    raise SystemExit(f"unknown config {config}")


def variant(lp, path):
    """The other version of lp for this path (the session alternates between lp and it)."""
    out = copy.copy(lp)
    if path == "update":
        c = np.array(lp.col_cost, dtype=np.float64)
        c[c.size // 2] += 1.0
        out.col_cost = c
    elif path == "update_matrix":
        a = np.array(lp.a_value, dtype=np.float64)
        a[a.size // 2] *= 1.5
        out.a_value = a
    elif path == "create":
        lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
        i = int(np.nonzero((lo == up) & np.isfinite(lo))[0][0])
        lo[i] = -np.inf
        out.row_lower = lo
    return out


def measure(config, reps):
    lp = workload(config)
    med = statistics.median
    res = dict(config=config, m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz), reps=reps, paths={})
    S = solver.Session()
    for path in PATHS:
        other = variant(lp, path)
        out, info = S.solve(lp, **OPTIONS)  # what is held when the timed calls begin
        assert out.status != solver.kError, out.info
        rows = dict(setup=[], upload=[], compare=[], apply=[], solve_setup=[])
        taken, held = None, 0
        for r in range(reps):
            target = other if r % 2 == 0 else lp
            out, info = S.solve(target, **OPTIONS)
            assert out.status != solver.kError, out.info
            taken, held = abi.SESSION_PATH_NAME[info.path], int(info.held_bytes)
            rows["setup"].append(info.setup_seconds)
            rows["upload"].append(info.upload_seconds)
            rows["compare"].append(info.diff_seconds - info.upload_seconds)
            rows["apply"].append(info.apply_seconds)
            one = solver.solveLpCupdlp(target, **OPTIONS)
            assert one.status != solver.kError
            rows["solve_setup"].append(one.result.setup_seconds)
        res["paths"][path] = dict(
            path_taken=taken, held_bytes=held,
            session_setup_seconds=med(rows["setup"]), solve_setup_seconds=med(rows["solve_setup"]),
            solve_over_session=med(rows["solve_setup"]) / med(rows["setup"]) if med(rows["setup"]) > 0 else None,
            parts_seconds=dict(upload=med(rows["upload"]), compare=med(rows["compare"]), apply=med(rows["apply"])),
            all_seconds=rows)
    S.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_vs_solve.json"))
    args = ap.parse_args()
    out = dict(what="pdlp_mi355x_session_solve on a held problem vs pdlp_mi355x_solve on the same modified problem: seconds before "
                    "the first iteration, median of reps, one process, one device",
               results=[measure(c, args.reps) for c in args.configs.split(",")])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
