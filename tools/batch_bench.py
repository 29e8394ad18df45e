#!/usr/bin/env python3
"""batch_bench.py — K variants of one small LP through a batch (pdlp_mi355x_batch_run) at 1, 2, 4 and 8
lanes against the same variants solved one after the other by update + run on ONE held solver of a build of the PARENT
commit.

  python tools/batch_bench.py --parent-lib PATH/libpdlp_mi355x.so [--instances 25fv47,afiro] [--ks 8,32] [--reps 5]
                              [--out profiles/batch_vs_sequential.json]

Same box, same session, alternating: every repetition starts one process on the parent's library (sequential side) and
one on this tree's (sequential again, then the batch at each lane count), per instance.  A process creates its solvers,
solves all variants once untimed, then times one pass per configuration: a host clock around calls that end in a device
synchronisation.  Reported per configuration: the median over the repetitions, all values, the spread (max - min) and the
iterations per second (sum of the variants' iteration counts over the wall time).  The variants are update_cases'
modifications (costs, column bounds, row bounds in turn), cut off at 2000 iterations or a KKT error of 1e-4.  Prints one
JSON line and writes it to --out.  No threshold is asserted: these are measurements.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
KINDS = ("cost", "col_bounds", "row_bounds")
LANES = (1, 2, 4, 8)


def variants(lp, K):
    import update_cases as UC
    return [UC.modification(lp, KINDS[k % len(KINDS)], 100 + k) for k in range(K)]


def everything(lp):
    return dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)


def worker(instance, ks, batch):
    """One process: the sequential side and, with `batch`, the batch at every lane count.  -> dict of configuration -> record"""
    from highs_amd import lp as L
    from highs_amd import solver
    lp = L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", instance + ".npz"))
    full = everything(lp)
    out = {}
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)

    def sequential(us):
        iters = 0
        for u in us:
            held.update(**dict(full, **u))
            iters += held.run(lp.num_col, lp.num_row).num_iter
        return iters

    for K in ks:
        us = variants(lp, K)
        sequential(us)  # untimed
        t0 = time.perf_counter()
        iters = sequential(us)
        out["sequential K=%d" % K] = dict(seconds=time.perf_counter() - t0, iterations=iters)
    held.close()
    if batch:
        for lanes in LANES:
            b = solver.DeviceBatch(lp, lanes=lanes, **OPTIONS)
            for K in ks:
                us = variants(lp, K)
                b.run(us)  # untimed
                t0 = time.perf_counter()
                res = b.run(us)
                dt = time.perf_counter() - t0
                I = b.info()
                out["batch lanes=%d K=%d" % (lanes, K)] = dict(
                    seconds=dt, iterations=sum(o.result.num_iter for o in res), reason=I.text, lanes_concurrent=I.lanes_concurrent,
                    trial_launches=I.trial_launches, check_launches=I.check_launches, fallback_variants=I.fallback_variants,
                    xcc_of_lane=list(I.xcc_of_lane))
            b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--instances", default="25fv47,afiro")
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_vs_sequential.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    if a.worker:
        print(json.dumps(worker(a.worker, ks, bool(a.batch))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed for the sequential side")

    def child(instance, lib, batch):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = lib
        else:
            env.pop("PDLP_MI355X_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", instance, "--ks", a.ks, "--batch", str(int(batch))],
                           env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s, %s): %s" % (instance, lib or "this tree", r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    result = dict(options=OPTIONS, reps=a.reps, instances={})
    for instance in a.instances.split(","):
        runs = {}
        for _ in range(a.reps):
            for side, rec in (("parent", child(instance, a.parent_lib, False)), ("this", child(instance, None, True))):
                for cfg, v in rec.items():
                    runs.setdefault(side + " " + cfg, []).append(v)
        table = {}
        for cfg, vs in runs.items():
            secs = [v["seconds"] for v in vs]
            med = statistics.median(secs)
            table[cfg] = dict(median_seconds=med, spread_seconds=max(secs) - min(secs), seconds=secs, iterations=vs[0]["iterations"],
                              iterations_per_second=vs[0]["iterations"] / med)
            for k in ("reason", "lanes_concurrent", "trial_launches", "check_launches", "fallback_variants", "xcc_of_lane"):
                if k in vs[-1]:
                    table[cfg][k] = vs[-1][k]
        for K in ks:
            base = table["parent sequential K=%d" % K]["median_seconds"]
            for lanes in LANES:
                t = table["this batch lanes=%d K=%d" % (lanes, K)]
                t["speedup_over_parent_sequential"] = base / t["median_seconds"]
        result["instances"][instance] = table
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
