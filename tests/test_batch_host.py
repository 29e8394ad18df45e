"""pdlp_mi355x_batch_* without a GPU: the fixed points of the ABI, the refusals of batch_create that are decided before
any device call (pinned by their words), and the batch driver behind canned lanes and the schedule of a device-driven
round under AddressSanitizer + UBSan as stand-alone programs."""
import ctypes as C
import os
import subprocess

import pytest

from highs_amd import abi, solver
from highs_amd import lp as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _afiro():
    return L.HighsLp.from_npz(os.path.join(GOLD, "instances", "afiro.npz"))


def _create(lanes, **options):
    """-> (return code, message, handle)"""
    P = abi.ProblemHandle(_afiro())
    params = abi.default_params(**options)
    h = C.c_void_p()
    rc = solver.lib().pdlp_mi355x_batch_create(C.byref(P.struct), C.byref(params), lanes, C.byref(h))
    return rc, solver.lib().pdlp_mi355x_last_error().decode(), h


def test_symbols_sizes_and_abi_version():
    lib = solver.lib()
    for name in ("pdlp_mi355x_batch_create", "pdlp_mi355x_batch_run", "pdlp_mi355x_batch_info", "pdlp_mi355x_batch_destroy"):
        assert hasattr(lib, name), name
    assert lib.pdlp_mi355x_batch_info_size() == C.sizeof(abi.PdlpBatchInfo) == 232
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(8) == C.sizeof(abi.PdlpUpdate)  # (pdlp_update_t keeps its layout: `reserved` was there)
    assert lib.pdlp_mi355x_sizeof(9) == -1                        # ... and pdlp_mi355x_sizeof its indices


@pytest.mark.parametrize("lanes", [0, 9, -1])
def test_create_refuses_lane_counts_outside_1_to_8(lanes):
    rc, msg, h = _create(lanes)
    assert rc != 0 and not h.value
    assert msg == "pdlp_mi355x_batch_create: lanes = %d is outside 1..8 (one lane per XCD)" % lanes


def test_create_refuses_hipdlp_by_name():
    rc, msg, h = _create(4, solver="hipdlp")
    assert rc != 0 and not h.value
    assert msg == "pdlp_mi355x_batch_create: HiPDLP solvers (algorithm = 1) do not take updates"


def test_create_refuses_more_than_one_device_by_name():
    params = abi.default_params()
    params.num_devices = 2
    P = abi.ProblemHandle(_afiro())
    h = C.c_void_p()
    rc = solver.lib().pdlp_mi355x_batch_create(C.byref(P.struct), C.byref(params), 4, C.byref(h))
    assert rc != 0 and not h.value
    assert solver.lib().pdlp_mi355x_last_error().decode() == \
        "pdlp_mi355x_batch_create: sharded solvers (more than one device) do not take updates"


def test_create_refuses_forced_sharding_by_name(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    rc, msg, h = _create(4)
    assert rc != 0 and not h.value
    assert msg == "pdlp_mi355x_batch_create: sharded solvers (sharding forced) do not take updates"


def test_null_arguments_and_destroy_null():
    lib = solver.lib()
    lib.pdlp_mi355x_batch_destroy(None)  # harmless
    I = abi.PdlpBatchInfo()
    assert lib.pdlp_mi355x_batch_info(None, C.byref(I)) != 0
    assert "null" in lib.pdlp_mi355x_last_error().decode()
    assert lib.pdlp_mi355x_batch_run(None, 1, None, None) != 0
    assert lib.pdlp_mi355x_last_error().decode() == "pdlp_mi355x_batch_run: null batch"
    h = C.c_void_p()
    assert lib.pdlp_mi355x_batch_create(None, None, 4, C.byref(h)) != 0


def test_device_batch_raises_the_refusal():
    with pytest.raises(RuntimeError, match="lanes = 9 is outside 1..8"):
        solver.DeviceBatch(_afiro(), lanes=9)


def test_driver_behind_canned_lanes_under_sanitizers(tmp_path):
    """Refills, uneven ends, the failure rule, all-or-nothing validation and the launch counts of the driver
    (csrc/pdlp_batch.cpp) with lanes that replay canned verdicts: a host program of its own, never loaded into Python."""
    env = dict(os.environ, OUT=str(tmp_path / "batch_driver_check"))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "batch_driver_check.sh")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all scenarios passed" in r.stdout


def test_round_plan_follows_the_reference_schedule_under_sanitizers(tmp_path):
    """The planner, the entry rule and the queue-depth rule of csrc/pdlp_round.hpp, driven round after round by a host
    program of its own that plays the device (tools/round_plan_check.cpp), never loaded into Python."""
    env = dict(os.environ, OUT=str(tmp_path / "round_plan_check"))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "round_plan_check.sh")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all scenarios passed" in r.stdout
