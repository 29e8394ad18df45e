"""One rank of a multi-process sharded QP solve (launched by test_gpu_qp_sharded.py, one process per rank; on a one-GPU box
every rank uses the same device — the mesh exchange only needs HIP IPC).  Modelled on mesh_worker.py.

usage: qp_mesh_worker.py RANK WORLD IDHEX CASE OUTFILE
  CASE = solve:<qp golden>             -> full solve through create_sharded / run
         iterate:<qp golden|band40k>:<k>  -> k fixed iterations, dumps x, the step sizes and the launch counts
  band40k = bench.py --config qpn's generator at 40 000 columns (tridiagonal PSD Hessian, lpgen.bench_qp_at_scale)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from highs_amd import solver  # noqa: E402
from highs_amd import lp as L  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def qp_problem(name):
    if name == "band40k":
        from lpgen import bench_qp_at_scale
        return bench_qp_at_scale(40000, True)
    return L.HighsLp.from_npz(os.path.join(GOLD, "qp", name + ".npz"))


def main():
    rank, world, idhex, case, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    uid = (C.c_ubyte * 128).from_buffer_copy(bytes.fromhex(idhex))
    kind, name, *rest = case.split(":")
    lp = qp_problem(name)
    if kind == "solve":
        S = solver.DeviceSolver(lp=lp, rank=rank, world=world, unique_id=uid, time_limit=1000.0, kkt_tolerance=1e-8,
                                pdlp_iteration_limit=400000)
        ex, tl, cl = S.stage("exchange")[0], S.stage("trial_launches")[0], S.stage("check_launches")[0]
        R = S.run(lp.num_col, lp.num_row)
        np.savez(out, exchange=ex, trial_launches=tl, check_launches=cl, col_value=R.col_value, col_dual=R.col_dual,
                 row_value=R.row_value, row_dual=R.row_dual, num_iter=R.num_iter, num_trials=R.num_trials,
                 num_restarts=R.num_restarts, term=R.term_code, primal_obj=R.primal_obj, dual_obj=R.dual_obj)
    else:
        k = int(rest[0])
        S = solver.DeviceSolver(lp=lp, rank=rank, world=world, unique_id=uid)
        ex, tl = S.stage("exchange")[0], S.stage("trial_launches")[0]
        st = S.iterate(k)
        np.savez(out, exchange=ex, trial_launches=tl, x=S.get("x", S.n), steps=S.get("steps", 8), iters=st.iters,
                 trials=st.trials, restarts=st.restarts)
    S.close()


if __name__ == "__main__":
    main()
