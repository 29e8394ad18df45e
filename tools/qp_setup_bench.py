#!/usr/bin/env python3
"""qp_setup_bench.py — what pdlp_mi355x_create costs on a QP whose Hessian has an off-diagonal part, by where the problem is
formulated, scaled and laid out.  The set-up counterpart of tools/rehessian_bench.py.

  python tools/qp_setup_bench.py --parent-lib /path/to/the/parent/commit's/libpdlp_mi355x.so
                                 [--reps 5] [--n 500000] [--out profiles/qp_setup_device_vs_host.json]

Workloads: bench.py's `--config qpn` (500k x 500k, 4M nonzeros, tridiagonal PSD Q: tests/lpgen.py::bench_qp_at_scale) and the
same LP with a denser Hessian, a diagonally dominant band of half-width 8 (17 entries per row of Q).  Three ways each:
  parent        the library of the parent commit (--parent-lib; left out when not given): host set-up
  host          this tree with PDLP_MI355X_GPU_SETUP=0
  device        this tree with no switch set (the automatic rule: 200 000 matrix nonzeros)
Every measurement is a process of its own (the library is chosen when it is loaded); the processes alternate parent / host /
device, `reps` rounds per Hessian in one session.  Reported: pdlp_result_t.setup_seconds of a 40-iteration run, median, all
values, spread (max - min); for this tree also the parts of stage "setup_seconds" — the Hessian's extraction on the host, the
upload of its diagonal and of N, the scaling passes, N's layout build — and the rest.  `device_is_faster`: the device
median is below both other medians by more than the larger of the spreads involved.  Prints one JSON line and writes it to
--out.  Nothing is asserted: these are measurements.

  python tools/qp_setup_bench.py --extraction --parent-lib ... [--out profiles/qp_hessian_extraction.json]

The Hessian's extraction alone: parent / `walk` (this tree with PDLP_MI355X_GPU_HESSIAN=0: the host walk
and the upload of its result, as the parent) / device (this tree's default: pdlp_setup.hip gpuExtractHessian).  Every process
creates twice; the second create carries no module load.  Per way and create: median, all values and spread of
`extraction_and_upload` = slots 0 + 1 of stage "setup_seconds", and of the whole create.  `device_is_below_parent`: the device's
median is below the parent's by more than the larger of the two spreads; `walk_agrees_with_parent`: the two medians differ by
no more than the parent's spread.  Also what stage "hessian_extraction" reports (path, slots, peak of temporary HBM).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARTS = ("host_extraction", "hessian_upload", "scaling_passes", "n_layout_build")
HESSIANS = ("tridiagonal", "band8")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=40)


def band_hessian(n, half_width, seed=1):
    """Lower triangle, column-wise, of a diagonally dominant band: off-diagonals U(-0.5, 0.5) / half_width."""
    import numpy as np
    rng = np.random.default_rng(seed)
    k = np.arange(half_width + 1)
    rows = np.arange(n)[:, None] + k[None, :]
    inside = rows < n
    vals = rng.uniform(-0.5, 0.5, (n, half_width + 1)) / half_width
    vals[:, 0] = 0.0
    vals[~inside] = 0.0
    dom = np.abs(vals).sum(axis=1)                     # the entries below the diagonal in column j ...
    np.add.at(dom, rows[inside], np.abs(vals[inside]))  # ... and their mirror images in row i
    vals[:, 0] = dom + rng.uniform(0.0, 1.0, n)
    st = np.zeros(n + 1, np.int64)
    st[1:] = np.cumsum(inside.sum(axis=1))
    return st.astype(np.int32), rows[inside].astype(np.int32), vals[inside]


def workload(hessian, n):
    import lpgen
    lp = lpgen.bench_qp_at_scale(n, True)
    if hessian == "band8":
        lp.hessian = band_hessian(n, 8)
    elif hessian != "tridiagonal":
        raise SystemExit(f"unknown Hessian {hessian}")
    return lp


def extraction_worker(hessian, n):
    """Two creates in this process (the second without the module load) -> one JSON line."""
    from highs_amd import solver
    lp = workload(hessian, n)
    out = dict(hessian_slots=int(len(lp.hessian[2])), m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz), creates=[])
    for _ in range(2):
        ds = solver.DeviceSolver(lp, **OPTIONS)
        sec = ds.stage("setup_seconds", 5)
        rec = dict(create_seconds=float(sec[4]), extraction_and_upload=float(sec[0] + sec[1]), extraction=float(sec[0]), upload=float(sec[1]),
                   gpu_setup=ds.setup_scalars()["gpu_setup"])
        try:
            rec["hessian_extraction"] = ds.hessian_extraction()
        except RuntimeError:  # (a library from before this stage)
            rec["hessian_extraction"] = None
        out["creates"].append(rec)
        ds.close()
    print(json.dumps(out))


def measure_extraction(hessian, n, reps, parent_lib):
    ways = (("parent",) if parent_lib else ()) + ("walk", "device")
    runs = {w: [] for w in ways}
    one(hessian, n, "device", parent_lib, "--extraction-worker")  # (not kept: warms the driver's caches)
    for _ in range(reps):
        for w in ways:
            runs[w].append(one(hessian, n, w, parent_lib, "--extraction-worker"))
    first = runs["device"][0]
    out = dict(hessian=hessian, m=first["m"], n=first["n"], nnz=first["nnz"], hessian_slots=first["hessian_slots"], reps=reps)
    med = statistics.median
    for w in ways:
        res = dict(hessian_extraction=runs[w][0]["creates"][0]["hessian_extraction"])
        for k, which in enumerate(("first_create", "second_create")):
            res[which] = {}
            for key in ("extraction_and_upload", "extraction", "upload", "create_seconds"):
                v = [r["creates"][k][key] for r in runs[w]]
                res[which][key] = dict(median=med(v), all=v, spread=max(v) - min(v))
        out[w] = res
    if parent_lib:
        for which in ("first_create", "second_create"):
            P, W, D = (out[w][which]["extraction_and_upload"] for w in ("parent", "walk", "device"))
            out["device_is_below_parent_" + which] = P["median"] - D["median"] > max(P["spread"], D["spread"])
            out["walk_agrees_with_parent_" + which] = abs(W["median"] - P["median"]) <= P["spread"]
    return out


def worker(hessian, n):
    """One create in this process, with whatever library and switches its environment names -> one JSON line."""
    from highs_amd import solver
    lp = workload(hessian, n)
    ds = solver.DeviceSolver(lp, **OPTIONS)
    out = dict(setup_seconds=ds.run(lp.num_col, lp.num_row).setup_seconds, gpu_setup=ds.setup_scalars()["gpu_setup"],
               hessian_slots=int(len(lp.hessian[2])), m=int(lp.num_row), n=int(lp.num_col), nnz=int(lp.num_nz))
    try:
        out["parts"] = dict(zip(PARTS, ds.stage("setup_seconds")[:len(PARTS)].tolist()))
    except RuntimeError:  # (a library from before this stage)
        out["parts"] = None
    ds.close()
    print(json.dumps(out))


def one(hessian, n, how, parent_lib, worker_flag="--worker"):
    env = dict(os.environ)
    env.pop("PDLP_MI355X_GPU_SETUP", None)
    env.pop("PDLP_MI355X_GPU_HESSIAN", None)
    env.pop("PDLP_MI355X_LIB", None)
    if how == "parent":
        env["PDLP_MI355X_LIB"] = parent_lib
    elif how == "host":
        env["PDLP_MI355X_GPU_SETUP"] = "0"
    elif how == "walk":
        env["PDLP_MI355X_GPU_HESSIAN"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), worker_flag, hessian, "--n", str(n)], env=env, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"worker {hessian}/{how} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def measure(hessian, n, reps, parent_lib):
    ways = (("parent",) if parent_lib else ()) + ("host", "device")
    runs = {w: [] for w in ways}
    one(hessian, n, "device", parent_lib)  # (not kept: the first process of a session also warms the driver's caches)
    for _ in range(reps):
        for w in ways:
            runs[w].append(one(hessian, n, w, parent_lib))
    first = runs["device"][0]
    out = dict(hessian=hessian, m=first["m"], n=first["n"], nnz=first["nnz"], hessian_slots=first["hessian_slots"], reps=reps)
    med = statistics.median
    for w in ways:
        secs = [r["setup_seconds"] for r in runs[w]]
        res = dict(gpu_setup=runs[w][0]["gpu_setup"], create_seconds=med(secs), create_seconds_all=secs, spread_seconds=max(secs) - min(secs))
        if runs[w][0]["parts"] is not None:
            parts = {k: med([r["parts"][k] for r in runs[w]]) for k in PARTS}
            parts["rest"] = res["create_seconds"] - sum(parts.values())
            res["parts_seconds"] = parts
            res["host_extraction_share"] = parts["host_extraction"] / res["create_seconds"]
        out[w] = res
    others = [w for w in ways if w != "device"]
    out["device_is_faster"] = all(
        out[w]["create_seconds"] - out["device"]["create_seconds"] > max(out[w]["spread_seconds"], out["device"]["spread_seconds"])
        for w in others)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) one create of this Hessian in this process")
    ap.add_argument("--extraction-worker", default=None, help="(internal) two creates of this Hessian in this process")
    ap.add_argument("--extraction", action="store_true", help="measure the Hessian's extraction and upload: parent / walk / device")
    ap.add_argument("--hessians", default=",".join(HESSIANS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=500_000, help="rows = columns of the workload (bench.py's is 500 000)")
    ap.add_argument("--parent-lib", default=None, help="libpdlp_mi355x.so built from the parent commit")
    ap.add_argument("--out", default=None, help="default: profiles/qp_setup_device_vs_host.json, with --extraction "
                                                "profiles/qp_hessian_extraction.json")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.n)
    if args.extraction_worker:
        return extraction_worker(args.extraction_worker, args.n)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    args.out = args.out or os.path.join(ROOT, "profiles", "qp_hessian_extraction.json" if args.extraction else "qp_setup_device_vs_host.json")
    if args.extraction:
        out = dict(what="the Hessian's extraction and the upload that goes with it (slots 0 + 1 of stage setup_seconds) inside "
                        "pdlp_mi355x_create: the parent commit's library, this tree with PDLP_MI355X_GPU_HESSIAN=0, this tree's "
                        "default; a process per measurement with two creates, alternating, median of reps",
                   parent_measured=parent is not None, results=[measure_extraction(h, args.n, args.reps, parent) for h in args.hessians.split(",")])
        line = json.dumps(out)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return
    out = dict(what="pdlp_mi355x_create (setup_seconds) on a QP with an off-diagonal Hessian: the parent commit's library, this "
                    "tree with the host set-up forced, this tree's default; a process per measurement, alternating, median of reps",
               parent_measured=parent is not None, results=[measure(h, args.n, args.reps, parent) for h in args.hessians.split(",")])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
