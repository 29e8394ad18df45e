#!/usr/bin/env python3
"""batch_values_bench.py — sweeps of VALUE variants through a batch (pdlp_mi355x_batch_run_values) at
1, 2, 4 and 8 lanes against the same variants solved one after the other by update_values / update_matrix + run on ONE
held solver of a build of the PARENT commit (which has both calls, and no value variants in batches).

  python tools/batch_values_bench.py --parent-lib PATH/libpdlp_mi355x.so [--workloads portfolio,25fv47] [--k 64] [--reps 5]
                                     [--out profiles/batch_values_vs_sequential.json]

Workloads:
  portfolio   a risk-aversion sweep: K q_value variants (Q times a factor between 0.1 and 10) of a dense-covariance
              portfolio on --portfolio-n columns (120: N in 28 work blocks, the most that still fit one XCD's 32),
              updatable="hessian"
  25fv47      K a_value variants (every coefficient jittered, update_matrix_cases) of 25fv47, updatable="matrix": every
              update runs all scaling passes
Default tolerance (1e-7), at most 2000 iterations per variant.

Same box, same session, alternating: every repetition starts one process on the parent's library (sequential side) and
one on this tree's (the batch at each lane count), per workload.  A process creates its solvers, solves all variants once
untimed, then times one pass per configuration: a host clock around calls that end in a device synchronisation.  Reported
per configuration: the median over the repetitions, all values, the spread (max - min), the iterations per second (sum of
the variants' iteration counts over the wall time), the share of the wall time spent in the updates (the sum of the
results' setup_seconds, which an update sets to its own duration — in a batch the lanes' updates run one after the other
between rounds), and the batch's launch counts.  A batch that does not run concurrently at 2 or more lanes is an error:
the workload was chosen to.  Prints one JSON line and writes it to --out.  No threshold is asserted: these are measurements.
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

OPTIONS = dict(pdlp_iteration_limit=2000)
LANES = (1, 2, 4, 8)


def workload(name, K, portfolio_n):
    """-> (lp, updatable, variants as DeviceBatch.run takes them)"""
    import numpy as np
    if name == "portfolio":
        import qp_small_cases as QC
        lp = QC.portfolio(n=portfolio_n)
        q0 = np.array(lp.hessian[2], dtype=np.float64)
        return lp, "hessian", [dict(q_value=f * q0) for f in np.geomspace(0.1, 10.0, K)]
    import update_matrix_cases as MC
    from highs_amd import lp as L
    lp = L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", name + ".npz"))
    return lp, "matrix", [dict(a_value=MC.new_values(lp, 200 + k, ("jitter",))) for k in range(K)]


def worker(name, K, portfolio_n, batch):
    """One process: the sequential side, or (batch) the batch at every lane count.  -> dict of configuration -> record"""
    from highs_amd import solver
    lp, updatable, vs = workload(name, K, portfolio_n)
    out = {}
    if not batch:
        held = solver.DeviceSolver(lp, updatable=updatable, **OPTIONS)

        def sequential():
            iters, upd = 0, 0.0
            for v in vs:
                if "q_value" in v:
                    held.update_values(q_value=v["q_value"])
                else:
                    held.update_matrix(v["a_value"])
                R = held.run(lp.num_col, lp.num_row)
                iters += R.num_iter
                upd += R.setup_seconds
            return iters, upd

        sequential()  # untimed
        t0 = time.perf_counter()
        iters, upd = sequential()
        out["sequential"] = dict(seconds=time.perf_counter() - t0, iterations=iters, update_seconds=upd)
        held.close()
        return out
    for lanes in LANES:
        b = solver.DeviceBatch(lp, lanes=lanes, updatable=updatable, **OPTIONS)
        b.run(vs)  # untimed
        t0 = time.perf_counter()
        res = b.run(vs)
        dt = time.perf_counter() - t0
        I = b.info()
        if lanes > 1 and not I.text.startswith("concurrent"):
            raise SystemExit("%s at %d lanes: %s" % (name, lanes, I.text))
        out["batch lanes=%d" % lanes] = dict(
            seconds=dt, iterations=sum(o.result.num_iter for o in res), update_seconds=sum(o.result.setup_seconds for o in res),
            reason=I.text, lanes_concurrent=I.lanes_concurrent, trial_launches=I.trial_launches, check_launches=I.check_launches,
            fallback_variants=I.fallback_variants)
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--workloads", default="portfolio,25fv47")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--portfolio-n", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_values_vs_sequential.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker(a.worker, a.k, a.portfolio_n, bool(a.batch))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed for the sequential side")

    def child(name, lib, batch):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = lib
        else:
            env.pop("PDLP_MI355X_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--k", str(a.k), "--portfolio-n",
                            str(a.portfolio_n), "--batch", str(int(batch))], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s, %s): %s" % (name, lib or "this tree", (r.stdout + r.stderr)[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    result = dict(options=OPTIONS, reps=a.reps, variants=a.k, portfolio_n=a.portfolio_n, workloads={})
    for name in a.workloads.split(","):
        runs = {}
        for _ in range(a.reps):
            for side, rec in (("parent", child(name, a.parent_lib, False)), ("this", child(name, None, True))):
                for cfg, v in rec.items():
                    runs.setdefault(side + " " + cfg, []).append(v)
        table = {}
        for cfg, vs in runs.items():
            secs = [v["seconds"] for v in vs]
            med = statistics.median(secs)
            table[cfg] = dict(median_seconds=med, spread_seconds=max(secs) - min(secs), seconds=secs, iterations=vs[0]["iterations"],
                              iterations_per_second=vs[0]["iterations"] / med,
                              update_share=statistics.median(v["update_seconds"] / v["seconds"] for v in vs))
            for k in ("reason", "lanes_concurrent", "trial_launches", "check_launches", "fallback_variants"):
                if k in vs[-1]:
                    table[cfg][k] = vs[-1][k]
        base = table["parent sequential"]["median_seconds"]
        for lanes in LANES:
            t = table["this batch lanes=%d" % lanes]
            t["speedup_over_parent_sequential"] = base / t["median_seconds"]
        result["workloads"][name] = table
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
