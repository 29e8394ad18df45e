#!/usr/bin/env python3
"""qp_small_bench.py — small QPs with off-diagonal Hessian entries: this tree (trials in the persistent loop, DESIGN.md
section 6c) against a build of the PARENT commit (a chain of launches per trial).

  python tools/qp_small_bench.py --parent-lib PATH/libpdlp_mi355x.so [--instances sq100,sq102,portfolio64,mpc40]
                                 [--iters 2000] [--reps 5] [--out profiles/qp_small_vs_parent.json]

Same box, same session, alternating: every repetition starts one process on the parent's library and one on this tree's,
per instance.  A process measures
  solo    microseconds per iteration of a fixed-work run: create, `--iters` iterations untimed, reset, the same timed (a host
          clock around a call that ends in a device synchronisation; checks and restarts included)
  batch   wall seconds of K = 8 variants (costs, column bounds, row bounds in turn; 2000 iterations or 1e-4): on the parent
          by update + run on ONE held solver, on this tree through an 8-lane batch (and, for reference, sequentially too)
Reported: the median over the repetitions, all values and the spread (max - min).  Prints one JSON line and writes it to
--out.  No threshold is asserted: these are measurements.
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
K = 8


def instance(name):
    import qp_small_cases as QC
    from highs_amd import lp as L
    if name == "portfolio64":
        return QC.portfolio()
    if name == "mpc40":
        return QC.mpc()
    return L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "qp", name + ".npz"))


def worker(name, iters, batch):
    import update_cases as UC
    from highs_amd import solver
    lp = instance(name)
    out = {}
    ds = solver.DeviceSolver(lp, kkt_tolerance=1e-12, pdlp_iteration_limit=10 * iters)
    out["path"] = dict(trial_barriers=float(ds.stage("trial_barriers", 1)[0]), trial_launches=float(ds.stage("trial_launches", 1)[0]),
                       check_launches=float(ds.stage("check_launches", 1)[0]))
    ds.iterate(iters)
    ds.reset()
    t0 = time.perf_counter()
    st = ds.iterate(iters)
    dt = time.perf_counter() - t0
    ds.close()
    out["solo"] = dict(seconds=dt, iterations=int(st.iters), trials=int(st.trials), us_per_iteration=1e6 * dt / max(int(st.iters), 1))
    us = [UC.modification(lp, KINDS[k % len(KINDS)], 100 + k) for k in range(K)]
    full = dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)

    def sequential():
        n = 0
        for u in us:
            held.update(**dict(full, **u))
            n += held.run(lp.num_col, lp.num_row).num_iter
        return n

    sequential()
    t0 = time.perf_counter()
    n = sequential()
    out["sequential"] = dict(seconds=time.perf_counter() - t0, iterations=n)
    held.close()
    if batch:
        b = solver.DeviceBatch(lp, lanes=8, **OPTIONS)
        b.run(us)
        t0 = time.perf_counter()
        res = b.run(us)
        dt = time.perf_counter() - t0
        I = b.info()
        out["batch"] = dict(seconds=dt, iterations=sum(o.result.num_iter for o in res), reason=I.text, lanes_concurrent=I.lanes_concurrent,
                            trial_launches=I.trial_launches, check_launches=I.check_launches, fallback_variants=I.fallback_variants)
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--instances", default="sq100,sq102,portfolio64,mpc40")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_small_vs_parent.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker(a.worker, a.iters, bool(a.batch))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed")

    def child(name, lib):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = lib
        else:
            env.pop("PDLP_MI355X_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--iters", str(a.iters), "--batch", str(int(not lib))],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s, %s): %s" % (name, lib or "this tree", r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    def summary(vs, key):
        xs = [v[key] for v in vs]
        return dict(median=statistics.median(xs), spread=max(xs) - min(xs), values=xs)

    result = dict(options=OPTIONS, iters=a.iters, reps=a.reps, K=K, instances={})
    for name in a.instances.split(","):
        runs = {"parent": [], "this": []}
        for _ in range(a.reps):
            runs["parent"].append(child(name, a.parent_lib))
            runs["this"].append(child(name, None))
        table = {}
        for side, vs in runs.items():
            rec = dict(path=vs[-1]["path"], solo_us_per_iteration=summary([v["solo"] for v in vs], "us_per_iteration"),
                       solo_iterations=vs[-1]["solo"]["iterations"], solo_trials=vs[-1]["solo"]["trials"],
                       sequential_seconds=summary([v["sequential"] for v in vs], "seconds"),
                       sequential_iterations=vs[-1]["sequential"]["iterations"])
            if "batch" in vs[-1]:
                rec["batch_seconds"] = summary([v["batch"] for v in vs], "seconds")
                rec["batch"] = {k: v for k, v in vs[-1]["batch"].items() if k != "seconds"}
            table[side] = rec
        p, t = table["parent"], table["this"]
        table["solo_speedup"] = p["solo_us_per_iteration"]["median"] / t["solo_us_per_iteration"]["median"]
        table["batch_speedup_over_parent_sequential"] = p["sequential_seconds"]["median"] / t["batch_seconds"]["median"]
        result["instances"][name] = table
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
