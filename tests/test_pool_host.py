"""pdlp_mi355x_solve_many without a GPU: the fixed points of the ABI, every refusal that is decided before any device call
(pinned by its words, with R and path left untouched), and the pool driver behind canned lanes under AddressSanitizer +
UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from highs_amd import abi, solver
from highs_amd import lp as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SENTINEL = 12345


def _lp(name="afiro"):
    return L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz"))


def _call(handles, lanes=4, K=None, params=None, null=(), **options):
    """pdlp_mi355x_solve_many on the problem handles (None: a NULL entry) -> (return code, message).  Asserts that R and path
    are as they were.  null: which of "P", "opt", "R" to pass as NULL."""
    lib = solver.lib()
    params = params or abi.default_params(**options)
    n = max(len(handles), 1)
    pP = C.POINTER(abi.PdlpProblem)
    Ps = (pP * n)()
    for k, h in enumerate(handles):
        if h is not None:
            Ps[k] = C.pointer(h.struct)
    Rs = (abi.PdlpResult * n)()
    for k in range(n):
        Rs[k].num_iter = SENTINEL
        Rs[k].term_code = SENTINEL
    path = np.full(n, SENTINEL, dtype=np.int32)
    I = abi.PdlpPoolInfo()
    rc = lib.pdlp_mi355x_solve_many(len(handles) if K is None else K, None if "P" in null else Ps,
                                    None if "opt" in null else C.byref(params), lanes, None if "R" in null else Rs,
                                    path.ctypes.data_as(abi.c_i32p), C.byref(I))
    msg = lib.pdlp_mi355x_last_error().decode()
    assert all(Rs[k].num_iter == SENTINEL and Rs[k].term_code == SENTINEL and not Rs[k].col_value for k in range(n))
    assert (path == SENTINEL).all()
    return rc, msg


def test_symbols_sizes_and_abi_version():
    lib = solver.lib()
    for name in ("pdlp_mi355x_solve_many", "pdlp_mi355x_pool_info_size"):
        assert hasattr(lib, name) and name in solver.EXPORTS, name
    assert lib.pdlp_mi355x_pool_info_size() == C.sizeof(abi.PdlpPoolInfo) == 256
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(9) == -1  # pdlp_mi355x_sizeof keeps its indices
    assert (abi.POOL_NOT_RUN, abi.POOL_SHARED, abi.POOL_ALONE, abi.POOL_FALLBACK) == (0, 1, 2, 3)


@pytest.mark.parametrize("null", ["P", "opt", "R"])
def test_null_arguments_are_refused(null):
    rc, msg = _call([abi.ProblemHandle(_lp())] * 2, null=(null,))
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: null argument"


@pytest.mark.parametrize("K", [0, -3])
def test_fewer_than_one_problem_is_refused(K):
    rc, msg = _call([abi.ProblemHandle(_lp())], K=K)
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: K = %d problems (at least 1)" % K


@pytest.mark.parametrize("lanes", [0, 9, -1])
def test_lane_counts_outside_1_to_8_are_refused(lanes):
    rc, msg = _call([abi.ProblemHandle(_lp())] * 2, lanes=lanes)
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: lanes = %d is outside 1..8 (one lane per XCD)" % lanes


def test_hipdlp_is_refused_by_name():
    rc, msg = _call([abi.ProblemHandle(_lp())] * 2, solver="hipdlp")
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: HiPDLP solvers (algorithm = 1) do not take updates"


def test_more_than_one_device_is_refused_by_name():
    params = abi.default_params()
    params.num_devices = 2
    rc, msg = _call([abi.ProblemHandle(_lp())] * 2, params=params)
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: sharded solvers (more than one device) do not take updates"


def test_forced_sharding_is_refused_by_name(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    rc, msg = _call([abi.ProblemHandle(_lp())] * 2)
    assert rc != 0 and msg == "pdlp_mi355x_solve_many: sharded solvers (sharding forced) do not take updates"


def test_a_bad_row_index_names_its_problem():
    good = [abi.ProblemHandle(_lp("afiro")), abi.ProblemHandle(_lp("adlittle"))]
    lp = _lp("afiro")
    lp.a_index = np.array(lp.a_index, dtype=np.int32)
    lp.a_index[7] = lp.num_row  # one past the last row
    rc, msg = _call(good + [abi.ProblemHandle(lp)] + good)
    assert rc != 0 and msg == "problem 2: row index out of range"


def test_a_null_problem_and_missing_arrays_name_their_problem():
    good = abi.ProblemHandle(_lp())
    rc, msg = _call([good, None, good])
    assert rc != 0 and msg == "problem 1: null problem"
    broken = abi.ProblemHandle(_lp())
    broken.struct.col_cost = None
    rc, msg = _call([good, good, good, broken])
    assert rc != 0 and msg == "problem 3: null column arrays"


def test_more_than_int32_max_nonzeros_name_their_problem():
    good = abi.ProblemHandle(_lp())
    huge = abi.ProblemHandle(_lp())
    huge.struct.num_nz = 2 ** 31  # (refused by the count alone: no array is followed)
    rc, msg = _call([good, huge])
    assert rc != 0 and msg == ("problem 1: pdlp_mi355x: the device path indexes the formulated matrix with 32-bit offsets, at most "
                               "INT32_MAX = 2147483647 nonzeros; this problem has 2147483648 nonzeros")


def test_solve_many_raises_the_refusal():
    with pytest.raises(RuntimeError, match="lanes = 9 is outside 1..8"):
        solver.solve_many([_lp(), _lp()], lanes=9)
    with pytest.raises(ValueError, match="one entry per LP"):
        solver.solve_many([_lp(), _lp()], starts=[None])


def test_driver_behind_canned_lanes_under_sanitizers(tmp_path):
    """Refills, uneven ends, a non-qualifying problem in the middle, the failure rule, a throw mid-run, the number of
    solvers alive and the launch counts of the driver (csrc/pdlp_pool.cpp) with solvers that replay canned verdicts: a host
    program of its own, never loaded into Python."""
    env = dict(os.environ, OUT=str(tmp_path / "pool_driver_check"))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "pool_driver_check.sh")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all scenarios passed" in r.stdout
