#!/usr/bin/env python3
"""pool_bench.py — 16 different small LPs through a pool (pdlp_mi355x_solve_many) at 1, 2, 4 and 8
lanes against the same LPs solved one after the other by pdlp_mi355x_solve on a build of the PARENT commit.

  python tools/pool_bench.py --parent-lib PATH/libpdlp_mi355x.so [--instances a,b,...] [--iter-limit 20000] [--reps 5]
                             [--out profiles/pool_vs_sequential.json]

Same box, same session, alternating: every repetition starts one process on the parent's library (the sequential loop)
and one on this tree's (the sequential loop again, then the pool at each lane count).  A process first loads the kernels
with a short untimed pass (every LP cut off at 100 iterations), then times one pass per configuration: a host clock around
calls that end in a device synchronisation.  The LPs are solved at the default tolerance (1e-7), cut off at --iter-limit
iterations so that a pass stays under a minute.  Reported per configuration: the median over the repetitions, all values,
the spread (max - min), the iterations per second of the pass, the share of the pass spent in the (serial) creates, and the
iterations per second of the loops alone (the pass without its creates) — for the pool also per lane, against the
sequential loop's.  Prints one JSON line and writes it to --out.  No threshold is asserted: these are measurements.
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

INSTANCES = ("25fv47,adlittle,bgetam,box1,e226,ex72a,forest6,gas11,israel,perold,refinery,scrs8,shell,stair,standmps,standata")
LANES = (1, 2, 4, 8)


def worker(names, iter_limit, pool):
    """One process: the sequential loop and, with `pool`, the pool at every lane count.  -> dict of configuration -> record.
    The clock is around the library's calls alone: problems and results are marshalled before it starts."""
    import ctypes as C
    from highs_amd import abi
    from highs_amd import lp as L
    from highs_amd import solver
    lib = solver.lib()
    lps = [L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", n + ".npz")) for n in names]
    K = len(lps)
    handles = [abi.ProblemHandle(lp) for lp in lps]
    results = [abi.ResultHandle(lp.num_col, lp.num_row) for lp in lps]
    Ps = (C.POINTER(abi.PdlpProblem) * K)(*[C.pointer(h.struct) for h in handles])
    Rs = (abi.PdlpResult * K)(*[r.struct for r in results])
    out = {}

    def sequential(limit):
        params = abi.default_params(pdlp_iteration_limit=limit)
        for k in range(K):
            if lib.pdlp_mi355x_solve(C.byref(handles[k].struct), C.byref(params), C.byref(Rs[k])) != 0:
                raise RuntimeError(lib.pdlp_mi355x_last_error().decode())
        return sum(Rs[k].num_iter for k in range(K)), sum(Rs[k].setup_seconds for k in range(K))

    def many(limit, lanes):
        params = abi.default_params(pdlp_iteration_limit=limit)
        I = abi.PdlpPoolInfo()
        if lib.pdlp_mi355x_solve_many(K, Ps, C.byref(params), lanes, Rs, None, C.byref(I)) != 0:
            raise RuntimeError(lib.pdlp_mi355x_last_error().decode())
        return sum(Rs[k].num_iter for k in range(K)), I

    sequential(100)  # untimed: the kernels are loaded
    t0 = time.perf_counter()
    iters, creates = sequential(iter_limit)
    out["sequential"] = dict(seconds=time.perf_counter() - t0, iterations=iters, create_seconds=creates)
    if pool:
        many(100, 8)  # untimed
        for lanes in LANES:
            t0 = time.perf_counter()
            iters, I = many(iter_limit, lanes)
            dt = time.perf_counter() - t0
            out["pool lanes=%d" % lanes] = dict(
                seconds=dt, iterations=iters, create_seconds=I.create_seconds, reason=I.text,
                lanes_concurrent=I.lanes_concurrent, shared_problems=I.shared_problems, alone_problems=I.alone_problems,
                fallback_problems=I.fallback_problems, trial_launches=I.trial_launches, check_launches=I.check_launches,
                mixed_launches=I.mixed_launches, xcc_of_lane=list(I.xcc_of_lane))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--instances", default=INSTANCES)
    ap.add_argument("--iter-limit", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_vs_sequential.json"))
    ap.add_argument("--worker", type=int, default=-1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = a.instances.split(",")
    if a.worker >= 0:
        print(json.dumps(worker(names, a.iter_limit, bool(a.worker))))
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is needed for the sequential side")

    def child(lib, pool):
        env = dict(os.environ)
        if lib:
            env["PDLP_MI355X_LIB"] = os.path.abspath(lib)
        else:
            env.pop("PDLP_MI355X_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(int(pool)), "--instances", a.instances,
                            "--iter-limit", str(a.iter_limit)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("worker failed (%s): %s" % (lib or "this tree", r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    runs = {}
    for _ in range(a.reps):
        for side, rec in (("parent", child(a.parent_lib, False)), ("this", child(None, True))):
            for cfg, v in rec.items():
                runs.setdefault(side + " " + cfg, []).append(v)
    table = {}
    for cfg, vs in runs.items():
        secs = [v["seconds"] for v in vs]
        med = statistics.median(secs)
        mid = sorted(vs, key=lambda v: v["seconds"])[len(vs) // 2]  # the repetition of the median
        loop = mid["seconds"] - mid["create_seconds"]
        table[cfg] = dict(median_seconds=med, spread_seconds=max(secs) - min(secs), seconds=secs, iterations=vs[0]["iterations"],
                          iterations_per_second=vs[0]["iterations"] / med, create_share=mid["create_seconds"] / mid["seconds"],
                          loop_iterations_per_second=mid["iterations"] / loop)
        for k in ("reason", "lanes_concurrent", "shared_problems", "alone_problems", "fallback_problems", "trial_launches",
                  "check_launches", "mixed_launches", "xcc_of_lane"):
            if k in vs[-1]:
                table[cfg][k] = vs[-1][k]
    base = table["parent sequential"]
    for lanes in LANES:
        t = table["this pool lanes=%d" % lanes]
        t["speedup_over_parent_sequential"] = base["median_seconds"] / t["median_seconds"]
        t["beyond_parent_spread"] = abs(base["median_seconds"] - t["median_seconds"]) > base["spread_seconds"]
        t["per_lane_loop_rate_over_sequential"] = t["loop_iterations_per_second"] / max(t["lanes_concurrent"], 1) / base["loop_iterations_per_second"]
    result = dict(options=dict(kkt_tolerance=1e-7, pdlp_iteration_limit=a.iter_limit), reps=a.reps, instances=names, table=table)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
