#!/usr/bin/env python3
"""resident_bench.py — what a re-solve costs around its loop when the data come from host memory (DeviceSolver.update + run
from numpy arrays, on a build of the PARENT commit's library) and when they are in HBM already (update_tensors +
run_tensors from torch tensors, this tree: pdlp_mi355x_update_device / _run_device).

  python tools/resident_bench.py --parent-lib PATH/libpdlp_mi355x.so [--workloads a,b,25fv47] [--reps 5] [--resolves 10]
                                 [--out profiles/resident_vs_host.json]

Workloads: bench.py's configs a (100k x 100k, 1M nonzeros) and b (1M x 1M, 8M nonzeros) through SyntheticProblem, and
25fv47.  Every update gives all five data arrays (costs, both column bounds, both row bounds: the held problem's times a
factor close to 1, so every row keeps its kind); the iteration limit is 40 on both sides, so the loop is the same work.

Per re-solve three numbers are taken:
  setup_seconds   pdlp_result_t.setup_seconds of the run behind the update: the update's own time, everything before the
                  first iteration
  tail_seconds    the host clock around the run call minus its solve_seconds (the loop): the reset in front of the loop,
                  which is the same on both sides, and everything behind the loop up to the return — the post-solve
  call_seconds    the host clock around the whole Python call pair (update + run / update_tensors + run_tensors); the
                  results are complete when either returns
and, for orientation, solve_seconds (the 40 iterations).

Same box, same session, alternating: every repetition starts one process on the parent's library and one on this tree's,
per workload.  A process creates its solver, re-solves twice untimed, then --resolves times; its figure is the median over
those.  Reported per side: the median over the repetitions, all values and the spread (max - min); and per workload
whether this tree is below the parent by more than the larger of the two spreads.  Prints one JSON line and writes it to
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

SYNTHETIC = {"a": (100_000, 100_000, 1_000_000), "b": (1_000_000, 1_000_000, 8_000_000)}
OPTIONS = dict(pdlp_iteration_limit=40, updatable=True)
FIGURES = ("setup_seconds", "tail_seconds", "call_seconds", "solve_seconds")
DATA = ("col_cost", "col_lower", "col_upper", "row_lower", "row_upper")


def problem(name):
    from highs_amd import lp as L
    from highs_amd import solver
    if name in SYNTHETIC:
        return solver.SyntheticProblem(*SYNTHETIC[name], 1).to_lp()
    return L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", name + ".npz"))


def variants(lp, count):
    """count updates of all five data arrays: the problem's own times 1 + k / 1000 (infinite bounds stay infinite, equal
    bounds stay equal: no row changes its kind)."""
    import numpy as np
    out = []
    for k in range(count):
        f = 1.0 + (k + 1) / 1000.0
        out.append({name: np.asarray(getattr(lp, name), dtype=np.float64) * f for name in DATA})
    return out


def worker(name, resolves, device_side):
    """One process, one side -> dict of figure -> median over the timed re-solves (and what was solved)."""
    import numpy as np
    from highs_amd import solver
    lp = problem(name)
    vs = variants(lp, resolves + 2)
    rec = {k: [] for k in FIGURES}
    if device_side:
        import torch
        from highs_amd import tensors as T
        S = solver.DeviceSolver.from_tensors(T.TensorProblem.from_lp(lp, "cuda"), **OPTIONS)
        tv = [{k: torch.from_numpy(v).to("cuda") for k, v in u.items()} for u in vs]
        out = {k: torch.empty(lp.num_col if k.startswith("col") else lp.num_row, dtype=torch.float64, device="cuda")
               for k in T.TensorResult.VECTORS}
        torch.cuda.synchronize()
    else:
        S = solver.DeviceSolver(lp, **OPTIONS)
    iters = None
    for i, u in enumerate(vs):
        t0 = time.perf_counter()
        if device_side:
            S.update_tensors(**tv[i])
            t1 = time.perf_counter()
            R = S.run_tensors(out=out)
        else:
            S.update(**u)
            t1 = time.perf_counter()
            R = S.run(lp.num_col, lp.num_row)
        t2 = time.perf_counter()
        iters = int(R.num_iter)
        if i >= 2:
            rec["setup_seconds"].append(R.setup_seconds)
            rec["solve_seconds"].append(R.solve_seconds)
            rec["tail_seconds"].append((t2 - t1) - R.solve_seconds)
            rec["call_seconds"].append(t2 - t0)
    parts = [float(x) for x in S.stage("update_seconds", 6)]  # of the last update: stage, kernels, sums, bounds, capture, reset
    S.close()
    res = {k: statistics.median(v) for k, v in rec.items()}
    res.update(iterations=iters, num_col=int(lp.num_col), num_row=int(lp.num_row), nnz=int(np.asarray(lp.a_value).size),
               last_update_parts=dict(zip(("stage", "kernels", "sums", "bounds", "capture", "reset"), parts)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--workloads", default="a,b,25fv47")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolves", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_vs_host.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--device-side", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker(a.worker, a.resolves, bool(a.device_side))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed for the host side")

    def child(name, lib, device_side):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = os.path.abspath(lib)
        else:
            env.pop("PDLP_MI355X_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--resolves", str(a.resolves),
                            "--device-side", str(int(device_side))], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s, %s): %s" % (name, lib or "this tree", (r.stdout + r.stderr)[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    result = dict(options=OPTIONS, reps=a.reps, resolves_per_process=a.resolves,
                  sides=dict(parent="the parent commit's library: DeviceSolver.update + run from numpy arrays",
                             this="this tree: update_tensors + run_tensors from tensors in HBM"), workloads={})
    for name in a.workloads.split(","):
        runs = {"parent": [], "this": []}
        for _ in range(a.reps):
            runs["parent"].append(child(name, a.parent_lib, False))
            runs["this"].append(child(name, None, True))
        table = {}
        for side, rs in runs.items():
            table[side] = {}
            for fig in FIGURES:
                vals = [r[fig] for r in rs]
                table[side][fig] = dict(median=statistics.median(vals), spread=max(vals) - min(vals), values=vals)
            table[side]["last_update_parts"] = rs[-1]["last_update_parts"]
        verdict = {}
        for fig in ("setup_seconds", "tail_seconds", "call_seconds"):
            p, t = table["parent"][fig], table["this"][fig]
            verdict[fig] = dict(parent_minus_this=p["median"] - t["median"],
                                below_parent_by_more_than_the_spread=bool(p["median"] - t["median"] > max(p["spread"], t["spread"])))
        result["workloads"][name] = dict(num_col=runs["this"][0]["num_col"], num_row=runs["this"][0]["num_row"], nnz=runs["this"][0]["nnz"],
                                         iterations=[runs["parent"][0]["iterations"], runs["this"][0]["iterations"]],
                                         sides=table, verdict=verdict)
        print("%-7s %-6s %12s %12s %12s   (medians of %d, ms; +- = spread)" % (name, "", "setup", "tail", "call", a.reps), file=sys.stderr)
        for side in ("parent", "this"):
            print("%-7s %-6s " % ("", side) + " ".join("%7.3f+-%5.3f" % (1e3 * table[side][f]["median"], 1e3 * table[side][f]["spread"])
                                                       for f in ("setup_seconds", "tail_seconds", "call_seconds")), file=sys.stderr)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
