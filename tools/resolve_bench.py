#!/usr/bin/env python3
"""resolve_bench.py — what re-solving a held problem costs before the first iteration: pdlp_mi355x_create on the
modified problem P' (everything again) against pdlp_mi355x_update to P' on a held solver.

  python tools/resolve_bench.py [--configs b,a,c] [--reps 5] [--out profiles/update_vs_create.json]

Both are measured in ONE process on one device (boxes differ by a few per cent), `reps` times each, median:
  create   pdlp_result_t.setup_seconds of a fresh, not updatable solver on P' (the path this feature leaves alone)
  update   pdlp_result_t.setup_seconds of the run after pdlp_mi355x_update (all five arrays given, P -> P' and back in
           turn), with its parts from stage "update_seconds": upload + validation, replay kernels, norms + sums (two
           downloads and the host's left-to-right loops), per-block bounds, graph capture, reset
plus the HBM an updatable solver keeps (stage "update_state").  The runs that report the times are cut off after 40
iterations.  Prints one JSON line and writes it to --out.  No threshold is asserted anywhere: these are measurements.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


import lpgen  # noqa: E402
import update_cases as UC  # noqa: E402
from highs_amd import solver  # noqa: E402

PARTS = ("upload_validate", "kernels", "norms_sums", "block_bounds", "graph_capture", "reset")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=40)


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


def everything(lp):
    return dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)


def measure(config, reps):
    lp = workload(config)
    lp2 = UC.apply(lp, UC.modification(lp, "all", seed=1))
    med = statistics.median
    create = []
    for _ in range(reps):
        ds = solver.DeviceSolver(lp2, **OPTIONS)
        create.append(ds.run(lp.num_col, lp.num_row).setup_seconds)
        ds.close()
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    create_updatable = held.run(lp.num_col, lp.num_row).setup_seconds
    held.update(**everything(lp2))  # (the first update allocates the staging buffer: not timed)
    held.update(**everything(lp))
    update, wall, parts = [], [], {k: [] for k in PARTS}
    for r in range(reps):
        target = lp2 if r % 2 == 0 else lp
        t0 = time.perf_counter()
        held.update(**everything(target))
        wall.append(time.perf_counter() - t0)
        sec = held.stage("update_seconds")
        update.append(held.run(lp.num_col, lp.num_row).setup_seconds)
        for k, v in zip(PARTS, sec):
            parts[k].append(float(v))
    state = held.stage("update_state")
    n, m = held.n, held.m
    held.close()
    return dict(config=config, m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz), formulated_n=n, formulated_m=m, reps=reps,
                create_setup_seconds=med(create), create_setup_seconds_all=create,
                create_updatable_setup_seconds=create_updatable,
                update_setup_seconds=med(update), update_setup_seconds_all=update,
                update_call_wall_seconds=med(wall),
                update_parts_seconds={k: med(v) for k, v in parts.items()},
                create_over_update=med(create) / med(update) if med(update) > 0 else None,
                kept_hbm_bytes=int(state[0]), passes=int(state[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="b,a,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_vs_create.json"))
    args = ap.parse_args()
    out = dict(what="pdlp_mi355x_create on P' vs pdlp_mi355x_update to P' on a held solver: seconds before the first iteration, "
                    "median of reps, one process, one device",
               results=[measure(c, args.reps) for c in args.configs.split(",")])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
