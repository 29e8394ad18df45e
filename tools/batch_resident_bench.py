#!/usr/bin/env python3
"""batch_resident_bench.py — sweeps whose variants and solutions live in HBM (pdlp_mi355x_batch_run_device, DESIGN.md
section 2j), three ways:

  (a) parent    a build of the PARENT commit (which has the device-resident entries and the batches, but no batch that takes
                tensors): a sequential update_tensors + run_tensors loop on ONE held solver
  (b) host      this tree: DeviceBatch.run at 8 lanes fed by .cpu().numpy() of every tensor, every solution uploaded again
  (c) device    this tree: DeviceBatch.run_tensors at 1, 2, 4 and 8 lanes

  python tools/batch_resident_bench.py --parent-lib PATH/libpdlp_mi355x.so [--workloads 25fv47:8,25fv47:32,portfolio:64]
                                       [--reps 5] [--out profiles/batch_resident_vs_parent.json]

Workloads (name:K):
  25fv47      K data variants (costs, column bounds, row bounds and all of them in turn: update_cases) of 25fv47
  portfolio   the risk-aversion sweep of section 2g: K q_value variants (Q times a factor between 0.1 and 10) of a dense-
              covariance portfolio on 120 columns, updatable="hessian"
Default tolerance (1e-7), at most 2000 iterations per variant, as tools/batch_values_bench.py (the tests use kkt_tolerance=1e-4).

Same box, same session, alternating: every repetition starts one fresh process on the parent's library and one on this
tree's, one at a time, each under a time limit of its own.  A process uploads the variants once, creates its solvers,
solves all variants once untimed, then times one pass per configuration: a host clock around calls that end in a device
synchronisation, with the solutions in HBM at the end on every side.  Reported per configuration: the median over the
repetitions, all values, the spread (max - min), and the share of the wall time spent in the updates (the sum of the
results' setup_seconds, which an update sets to its own duration).  Prints one JSON line and writes it to --out.  No
threshold is asserted: these are measurements; `claims` states whether (c) at 8 lanes beats (a) by more than the two
spreads added, and whether (c) at 8 lanes is slower than (b) beyond them.
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
VECTORS = ("col_value", "col_dual", "row_value", "row_dual")


def workload(name, K):
    """-> (lp, updatable or None, variants as DeviceBatch.run takes them)"""
    import numpy as np
    if name == "portfolio":
        import qp_small_cases as QC
        lp = QC.portfolio(n=120)
        q0 = np.array(lp.hessian[2], dtype=np.float64)
        return lp, "hessian", [dict(q_value=f * q0) for f in np.geomspace(0.1, 10.0, K)]
    import update_cases as UC
    from highs_amd import lp as L
    lp = L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", name + ".npz"))
    kinds = ("cost", "col_bounds", "row_bounds", "all")
    return lp, None, [UC.modification(lp, kinds[k % 4], 300 + k) for k in range(K)]


def worker(name, K, parent):
    """One process: the parent's sequential loop, or this tree's host-fed batch and device batch.  -> configuration -> record"""
    import numpy as np
    import torch

    from highs_amd import solver

    lp, updatable, vs = workload(name, K)
    options = dict(OPTIONS) if updatable is None else dict(OPTIONS, updatable=updatable)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()).to("cuda")
    dvs = [{k: (a if k == "offset" else dev(a)) for k, a in v.items()} for v in vs]  # the sweep as its producer holds it
    sizes = dict(col_value=lp.num_col, col_dual=lp.num_col, row_value=lp.num_row, row_dual=lp.num_row)
    out2d = {k: torch.empty((K, n), dtype=torch.float64, device="cuda") for k, n in sizes.items()}
    torch.cuda.synchronize()
    out = {}

    def timed(fn):
        fn()  # untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters, upd = fn()
        torch.cuda.synchronize()
        return dict(seconds=time.perf_counter() - t0, iterations=iters, update_seconds=upd)

    if parent:
        full = dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                    row_upper=lp.row_upper)
        base = {k: dev(a) for k, a in full.items()}  # a held solver keeps what its last variant set: P's arrays restore it
        held = solver.DeviceSolver(lp, updatable=updatable or True, **OPTIONS)
        held.num_col, held.num_row = lp.num_col, lp.num_row

        def sequential():
            iters, upd = 0, 0.0
            for k, v in enumerate(dvs):
                if "q_value" in v:
                    held.update_tensors(**v)
                else:
                    held.update_tensors(**{**base, "offset": lp.offset, **v})
                R = held.run_tensors(out={f: out2d[f][k] for f in VECTORS})
                iters += R.num_iter
                upd += R.setup_seconds
            return iters, upd

        out["parent sequential tensors"] = timed(sequential)
        held.close()
        return out

    b = solver.DeviceBatch(lp, lanes=8, **options)

    def through_the_host():
        hv = [{k: (a if k == "offset" else a.cpu().numpy()) for k, a in v.items()} for v in dvs]
        res = b.run(hv)
        for k, o in enumerate(res):
            for f in VECTORS:
                out2d[f][k].copy_(torch.from_numpy(getattr(o.result, f)))
        return sum(o.result.num_iter for o in res), sum(o.result.setup_seconds for o in res)

    out["this host batch lanes=8"] = timed(through_the_host)
    b.close()
    for lanes in LANES:
        b = solver.DeviceBatch(lp, lanes=lanes, **options)

        def on_the_device():
            res = b.run_tensors(dvs, out=out2d)
            return sum(r.num_iter for r in res), sum(r.setup_seconds for r in res)

        rec = timed(on_the_device)
        I = b.info()
        if lanes > 1 and not I.text.startswith("concurrent"):
            raise SystemExit("%s at %d lanes: %s" % (name, lanes, I.text))
        rec.update(reason=I.text, lanes_concurrent=I.lanes_concurrent, trial_launches=I.trial_launches,
                   check_launches=I.check_launches, fallback_variants=I.fallback_variants)
        out["this device batch lanes=%d" % lanes] = rec
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--workloads", default="25fv47:8,25fv47:32,portfolio:64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_resident_vs_parent.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--parent", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        name, K = a.worker.split(":")
        print(json.dumps(worker(name, int(K), bool(a.parent))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed for side (a)")

    def child(spec, lib):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = lib
        else:
            env.pop("PDLP_MI355X_LIB", None)
        # a fresh process, alone on the device, under its own limit; a failure ends the whole measurement
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", spec, "--parent", str(int(bool(lib)))],
                           env=env, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s, %s): %s" % (spec, lib or "this tree", (r.stdout + r.stderr)[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    result = dict(options=OPTIONS, reps=a.reps, workloads={})
    for spec in a.workloads.split(","):
        runs = {}
        for _ in range(a.reps):
            for rec in (child(spec, a.parent_lib), child(spec, None)):
                for cfg, v in rec.items():
                    runs.setdefault(cfg, []).append(v)
        table = {}
        for cfg, vs in runs.items():
            secs = [v["seconds"] for v in vs]
            med = statistics.median(secs)
            table[cfg] = dict(median_seconds=med, spread_seconds=max(secs) - min(secs), seconds=secs, iterations=vs[0]["iterations"],
                              update_share=statistics.median(v["update_seconds"] / v["seconds"] for v in vs))
            for k in ("reason", "lanes_concurrent", "trial_launches", "check_launches", "fallback_variants"):
                if k in vs[-1]:
                    table[cfg][k] = vs[-1][k]
        pa, ho, d8 = table["parent sequential tensors"], table["this host batch lanes=8"], table["this device batch lanes=8"]
        for lanes in LANES:
            t = table["this device batch lanes=%d" % lanes]
            t["speedup_over_parent"] = pa["median_seconds"] / t["median_seconds"]
        table["claims"] = dict(
            device8_beats_parent_beyond_spreads=pa["median_seconds"] - d8["median_seconds"] > pa["spread_seconds"] + d8["spread_seconds"],
            device8_slower_than_host8_beyond_spreads=d8["median_seconds"] - ho["median_seconds"] > ho["spread_seconds"] + d8["spread_seconds"],
            same_iterations_on_all_sides=len({t["iterations"] for k, t in table.items() if k != "claims"}) == 1)
        result["workloads"][spec] = table
        print("done:", spec, file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
