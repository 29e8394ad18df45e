#!/usr/bin/env python3
"""rematrix_bench.py — what re-solving a held problem costs before the first iteration when the VALUES of its matrix
changed: pdlp_mi355x_create on the modified problem P' (everything again) against pdlp_mi355x_update_matrix to P' on a
held solver.  The matrix counterpart of tools/resolve_bench.py, same workloads.

  python tools/rematrix_bench.py [--configs b,a,c] [--reps 5] [--out profiles/update_matrix_vs_create.json]
                                 [--plain-create-seconds b=0.05,a=0.01,c=0.04]

Both are measured in ONE process on one device (boxes differ by a few per cent), `reps` times each, median, all values kept:
  create          pdlp_result_t.setup_seconds of a fresh, not updatable solver on P'
  update_matrix   pdlp_result_t.setup_seconds of the run after pdlp_mi355x_update_matrix (new values and all five data
                  arrays, P -> P' and back in turn), with its parts from stage "update_matrix_seconds": upload +
                  validation, formulate, scaling passes, refills, norms + sums, per-block bounds, graph capture, reset
plus the HBM a matrix-updatable solver keeps (stage "update_state" [0] and [4]) and what the flag costs at create: the
set-up time of a matrix-updatable solver on P against a plain one (same process; --plain-create-seconds records the plain
solver's time measured with a build of the commit before this feature, per config, for the comparison across commits).
The runs that report the times are cut off after 40 iterations.  Prints one JSON line and writes it to --out.  No
threshold is asserted anywhere: these are measurements.
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


import update_matrix_cases as MC  # noqa: E402
from highs_amd import solver  # noqa: E402
from resolve_bench import workload  # noqa: E402

PARTS = ("upload_validate", "formulate", "scaling_passes", "refills", "norms_sums", "block_bounds", "graph_capture", "reset")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=40)


def everything(lp):
    return dict(a_value=lp.a_value, col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper,
                row_lower=lp.row_lower, row_upper=lp.row_upper, offset=lp.offset)


def measure(config, reps, plain_parent):
    lp = workload(config)
    lp2 = MC.apply(lp, MC.modification(lp, "all", seed=1))
    med = statistics.median
    create, create_plain, create_matrix = [], [], []
    for _ in range(reps):
        ds = solver.DeviceSolver(lp2, **OPTIONS)
        create.append(ds.run(lp.num_col, lp.num_row).setup_seconds)
        ds.close()
    for _ in range(reps):
        ds = solver.DeviceSolver(lp, **OPTIONS)
        create_plain.append(ds.run(lp.num_col, lp.num_row).setup_seconds)
        ds.close()
        ds = solver.DeviceSolver(lp, updatable="matrix", **OPTIONS)
        create_matrix.append(ds.run(lp.num_col, lp.num_row).setup_seconds)
        ds.close()
    held = solver.DeviceSolver(lp, updatable="matrix", **OPTIONS)
    held.run(lp.num_col, lp.num_row)
    held.update_matrix(**everything(lp2))  # (the first update allocates the staging buffers: not timed)
    held.update_matrix(**everything(lp))
    update, wall, parts = [], [], {k: [] for k in PARTS}
    for r in range(reps):
        target = lp2 if r % 2 == 0 else lp
        t0 = time.perf_counter()
        held.update_matrix(**everything(target))
        wall.append(time.perf_counter() - t0)
        sec = held.stage("update_matrix_seconds")
        update.append(held.run(lp.num_col, lp.num_row).setup_seconds)
        for k, v in zip(PARTS, sec):
            parts[k].append(float(v))
    state = held.stage("update_state")
    n, m, nnz_f = held.n, held.m, held.nnz
    held.close()
    return dict(config=config, m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz), formulated_n=n, formulated_m=m,
                formulated_nnz=int(nnz_f), reps=reps,
                create_setup_seconds=med(create), create_setup_seconds_all=create,
                update_matrix_setup_seconds=med(update), update_matrix_setup_seconds_all=update,
                update_matrix_call_wall_seconds=med(wall), update_matrix_call_wall_seconds_all=wall,
                update_matrix_parts_seconds={k: med(v) for k, v in parts.items()},
                update_matrix_parts_seconds_all=parts,
                create_over_update_matrix=med(create) / med(update) if med(update) > 0 else None,
                kept_hbm_bytes_data=int(state[0]), kept_hbm_bytes_matrix=int(state[4]),
                kept_matrix_bytes_per_nonzero=float(state[4]) / max(int(nnz_f), 1),
                create_plain_setup_seconds=med(create_plain), create_plain_setup_seconds_all=create_plain,
                create_matrix_updatable_setup_seconds=med(create_matrix), create_matrix_updatable_setup_seconds_all=create_matrix,
                create_plain_setup_seconds_before_this_feature=plain_parent.get(config))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="b,a,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_matrix_vs_create.json"))
    ap.add_argument("--plain-create-seconds", default="",
                    help="config=seconds,...: set-up time of a plain solver measured with a build of the commit before this feature")
    args = ap.parse_args()
    parent = {k: float(v) for k, v in (kv.split("=") for kv in args.plain_create_seconds.split(",") if kv)}
    out = dict(what="pdlp_mi355x_create on P' vs pdlp_mi355x_update_matrix to P' on a held solver: seconds before the first "
                    "iteration, median of reps, one process, one device",
               results=[measure(c, args.reps, parent) for c in args.configs.split(",")])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
