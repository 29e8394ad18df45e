#!/usr/bin/env python3
"""hipdlp_small_bench.py — HiPDLP (solver="hipdlp") time per iteration on small LPs, with the steps 2..40 of a block as ONE
persistent launch (PDLP_MI355X_PERSISTENT_HIPDLP=1, pdlp_halpern_small.hip) against two launches per step (=0), and
against a build of the PARENT commit.

  python tools/hipdlp_small_bench.py [--parent-lib PATH/libpdlp_mi355x.so] [--instances afiro,adlittle,25fv47,80bau3b]
                                     [--iters 4000] [--reps 5] [--out profiles/hipdlp_small.md]

One process holds, per instance, a solver created with the switch on and one created with it off; after an untimed pass of
400 iterations each, the two are timed alternately, --reps times: reset, then iterate(--iters) — the fixed-work loop, with
its checks and restarts, timed by device events around everything the call queues.  Reported in us per iteration: the
median and the min-max spread.  With --parent-lib a second process does the same on the parent's library (which has one
form only), a third does it once more — the parent against itself shows what a change of process alone does to a
median — and a fourth times this tree's library with the switch off alone, as the parent is timed.  Two checks are printed with the table, neither asserted: the switch-off column agrees with the parent (its first
process) within the parent's own spread (so "off" really is the old path), and the switch-on median beats the parent's
median by more than the parent's spread (the condition for shipping the switch on).  80bau3b is the LP of 33..64 work blocks.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "PDLP_MI355X_PERSISTENT_HIPDLP"


def worker(names, iters, reps, switches):
    """-> {instance: {switch: {"us": [per repeat], "blocks": .., "reason": .., "mode": .., "launches": ..}}}"""
    from highs_amd import lp as L
    from highs_amd import solver
    out = {}
    for name in names:
        lp = L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", name + ".npz"))
        S, rec = {}, {}
        for sw in switches:
            if sw is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = sw
            S[sw] = solver.DeviceSolver(lp=lp, solver="hipdlp")
            blocks = max(S[sw].device_matrix(0)["n_blocks"], S[sw].device_matrix(1)["n_blocks"])
            rec[sw] = dict(us=[], blocks=int(blocks))
            S[sw].iterate(400)
        for _ in range(reps):
            for sw in switches:
                S[sw].reset()
                st = S[sw].iterate(iters)
                rec[sw]["us"].append(1e3 * st.gpu_ms / st.iters)
        for sw in switches:
            try:  # (the parent's library does not know these names)
                rec[sw]["reason"] = int(S[sw].stage("persistent_reason")[0])
                rec[sw]["mode"] = int(S[sw].stage("persistent_mode")[0])
                rec[sw]["launches"] = int(S[sw].stage("persistent_launches")[0])
                rec[sw]["fallbacks"] = int(S[sw].stage("barrier_fallbacks")[0])
            except RuntimeError:
                pass
            S[sw].close()
        out[name] = {("default" if sw is None else sw): r for sw, r in rec.items()}
    return out


def summary(us):
    return dict(median=statistics.median(us), lo=min(us), hi=max(us), spread=max(us) - min(us))


def cell(s):
    return "%.2f (%.2f-%.2f)" % (s["median"], s["lo"], s["hi"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--instances", default="afiro,adlittle,25fv47,80bau3b")
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hipdlp_small.md"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = a.instances.split(",")
    if a.worker:
        print(json.dumps(worker(names, a.iters, a.reps, [None] if a.worker == "parent" else ["0"] if a.worker == "off" else ["1", "0"])))
        return
    mine = worker(names, a.iters, a.reps, ["1", "0"])
    parent = again = alone = None

    def process(kind):
        env = dict(os.environ)
        if kind == "parent":
            env["PDLP_MI355X_LIB"] = os.path.abspath(a.parent_lib)
        env.pop(SWITCH, None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--instances", a.instances, "--iters", str(a.iters),
                            "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit("the process '%s' failed:\n" % kind + p.stderr)
        return json.loads(p.stdout.strip().splitlines()[-1])

    if a.parent_lib:
        parent, again, alone = process("parent"), process("parent"), process("off")
    lines = ["# HiPDLP on small LPs: one persistent launch for the steps 2..40 of a block", "",
             "`tools/hipdlp_small_bench.py`: iterate(%d) of the fixed-work loop, %d repeats, switch on / off alternating in one process;"
             % (a.iters, a.reps),
             "us per iteration, median (min-max), device events.  parent: a build of the parent commit, a process of its own;",
             "parent again: the same build in one more process; off alone: this tree, switch off, a process of its own.", "",
             "| LP | work blocks | mode | parent | parent again | off alone | switch off | switch on | on / parent | off within parent's spread | on beats parent by more than its spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    result = {}
    for n in names:
        on, off = summary(mine[n]["1"]["us"]), summary(mine[n]["0"]["us"])
        par = summary(parent[n]["default"]["us"]) if parent else None
        par2 = summary(again[n]["default"]["us"]) if again else None
        off1 = summary(alone[n]["0"]["us"]) if alone else None
        mode = {1: "XCD-local", 0: "agent scope", -1: "plain"}.get(mine[n]["1"].get("mode"), "?")
        if mine[n]["1"].get("fallbacks"):
            mode += " (fell back)"
        agree = "-" if not par else ("yes" if abs(off["median"] - par["median"]) <= par["spread"] else "no")
        beats = "-" if not par else ("yes" if par["median"] - on["median"] > par["spread"] else "no")
        lines.append("| %s | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            n, mine[n]["1"]["blocks"], mode, cell(par) if par else "-", cell(par2) if par2 else "-", cell(off1) if off1 else "-", cell(off), cell(on),
            "%.2f" % (on["median"] / par["median"]) if par else "-", agree, beats))
        result[n] = dict(on=on, off=off, parent=par, parent_again=par2, off_alone=off1, mode=mode, blocks=mine[n]["1"]["blocks"], launches=mine[n]["1"].get("launches"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
