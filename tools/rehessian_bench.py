#!/usr/bin/env python3
"""rehessian_bench.py — what re-solving a held QP costs before the first iteration when the VALUES of its Hessian changed:
pdlp_mi355x_create on the modified problem P' (everything again) against pdlp_mi355x_update_values to P' on a held solver
(DESIGN.md section 2e).  The Hessian counterpart of tools/rematrix_bench.py.

  python tools/rehessian_bench.py [--configs qp,qpn] [--reps 5] [--out profiles/update_hessian_vs_create.json]

Workloads: bench.py's `--config qp` (500k x 500k, 4M nonzeros, diagonal Q) and `--config qpn` (the same with a tridiagonal
PSD Q), built by tests/lpgen.py::bench_qp_at_scale at n = 500 000.  Two cases each:
  hessian   update_values(q_value) alone: a regenerated Hessian on the created pattern
  full      update_values(a_value, q_value, all five data arrays): P -> P' and back in turn
Everything is measured in ONE process on one device, `reps` times each, median, all values kept:
  create          pdlp_result_t.setup_seconds of a fresh, not updatable solver on P'
  update_values   pdlp_result_t.setup_seconds of the run after the update, with the Hessian's parts from stage
                  "update_values_seconds" (upload + validation, assembly, replay, refill of the N operand) and, for the
                  full case, the matrix update's parts from stage "update_matrix_seconds"
plus the HBM a Hessian-updatable solver keeps (stage "update_state" [6]).  The runs that report the times are cut off
after 40 iterations.  Prints one JSON line and writes it to --out.  No threshold is asserted anywhere: these are
measurements.
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
import update_hessian_cases as HC  # noqa: E402
from highs_amd import solver  # noqa: E402

HESSIAN_PARTS = ("upload_validate", "assemble", "replay", "refill")
MATRIX_PARTS = ("upload_validate", "formulate", "scaling_passes", "refills", "norms_sums", "block_bounds", "graph_capture", "reset")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=40)


def workload(config, n):
    if config not in ("qp", "qpn"):
        raise SystemExit(f"unknown config {config}")
    return lpgen.bench_qp_at_scale(n, config == "qpn")


def everything(lp):
    return dict(a_value=lp.a_value, q_value=lp.hessian[2], col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper,
                row_lower=lp.row_lower, row_upper=lp.row_upper, offset=lp.offset)


def create_seconds(lp, reps, **options):
    out = []
    for _ in range(reps):
        ds = solver.DeviceSolver(lp, **dict(OPTIONS, **options))
        out.append(ds.run(lp.num_col, lp.num_row).setup_seconds)
        ds.close()
    return out


def measure(config, reps, n):
    lp = workload(config, n)
    med = statistics.median
    lp_h = HC.apply(lp, HC.modification(lp, "regen", seed=1))   # Hessian only
    lp_f = HC.apply(lp, HC.modification(lp, "all", seed=1))     # Hessian + matrix + data
    out = dict(config=config, m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz), hessian_slots=int(len(lp.hessian[2])), reps=reps)
    create_plain = create_seconds(lp, reps)
    out.update(create_plain_setup_seconds=med(create_plain), create_plain_setup_seconds_all=create_plain)
    for case, bits, target in (("hessian", "hessian", lp_h), ("full", "matrix+hessian", lp_f)):
        create = create_seconds(target, reps)
        create_bits = create_seconds(lp, reps, updatable=bits)
        held = solver.DeviceSolver(lp, updatable=bits, **OPTIONS)
        held.run(lp.num_col, lp.num_row)
        change = (lambda t: dict(q_value=t.hessian[2])) if case == "hessian" else everything
        held.update_values(**change(target))  # (the first update allocates the staging buffers: not timed)
        held.update_values(**change(lp))
        update, wall = [], []
        hparts, mparts = {k: [] for k in HESSIAN_PARTS}, {k: [] for k in MATRIX_PARTS}
        recaptured = 0.0
        for r in range(reps):
            t = target if r % 2 == 0 else lp
            t0 = time.perf_counter()
            held.update_values(**change(t))
            wall.append(time.perf_counter() - t0)
            sec = held.stage("update_values_seconds")
            recaptured += sec[4]
            for k, v in zip(HESSIAN_PARTS, sec):
                hparts[k].append(float(v))
            if case == "full":
                for k, v in zip(MATRIX_PARTS, held.stage("update_matrix_seconds")):
                    mparts[k].append(float(v))
            update.append(held.run(lp.num_col, lp.num_row).setup_seconds)
        state = held.stage("update_state")
        launches = held.stage("trial_launches")[0]
        held.close()
        res = dict(updatable=bits, create_setup_seconds=med(create), create_setup_seconds_all=create,
                   update_values_setup_seconds=med(update), update_values_setup_seconds_all=update,
                   update_values_call_wall_seconds=med(wall), update_values_call_wall_seconds_all=wall,
                   hessian_parts_seconds={k: med(v) for k, v in hparts.items()}, hessian_parts_seconds_all=hparts,
                   create_over_update_values=med(create) / med(update) if med(update) > 0 else None,
                   graph_recaptures=recaptured, trial_launches=launches,
                   kept_hbm_bytes_data=int(state[0]), kept_hbm_bytes_matrix=int(state[4]), kept_hbm_bytes_hessian=int(state[6]),
                   create_updatable_setup_seconds=med(create_bits), create_updatable_setup_seconds_all=create_bits)
        if case == "full":
            res.update(matrix_parts_seconds={k: med(v) for k, v in mparts.items()}, matrix_parts_seconds_all=mparts)
        out[case] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="qp,qpn")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=500_000, help="rows = columns of the workload (bench.py's is 500 000)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_hessian_vs_create.json"))
    args = ap.parse_args()
    out = dict(what="pdlp_mi355x_create on P' vs pdlp_mi355x_update_values to P' on a held solver: seconds before the first "
                    "iteration, median of reps, one process, one device",
               results=[measure(c, args.reps, args.n) for c in args.configs.split(",")])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
