"""CPU tests of the rule that decides whether a HiPDLP solver runs the steps 2..40 of a block as one persistent launch
(highs_amd/csrc/pdlp_halpern_small.hpp halpernSmallReason, reached through the host-only hook
pdlp_mi355x_host_hipdlp_small_rule: the function the solver itself calls, on shapes made by hand)."""
import ctypes as C

import numpy as np
import pytest

from highs_amd import abi, solver

PERSISTENT, SWITCH_OFF, SHARDED, PROFILE, SLAB, NOT_512, LONG_MAJOR, TOO_MANY, NOT_RESIDENT = range(9)
# a shape that qualifies: 21 and 17 blocks of 512 entries, stream layout, no long major, one GPU, switch on, 1024 resident
OK = dict(blocks_a=21, blocks_at=17, chunk_a=512, chunk_at=512, use_slab=0, long_tasks=0, long_contrib=0, sharded=0, profile=0,
          switch_on=1, resident=1024)
ORDER = ("blocks_a", "blocks_at", "chunk_a", "chunk_at", "use_slab", "long_tasks", "long_contrib", "sharded", "profile",
         "switch_on", "resident")


def rule(xcd_local_allowed=1, **change):
    """-> (reason, grid, mode) for OK with the given fields changed."""
    fn = solver.lib().pdlp_mi355x_host_hipdlp_small_rule
    fn.argtypes = [abi.c_i32p, C.c_int32, abi.c_i32p, abi.c_i32p, abi.c_i32p]
    fn.restype = C.c_int
    assert set(change) <= set(ORDER)
    shape = np.array([dict(OK, **change)[k] for k in ORDER], dtype=np.int32)
    reason, grid, mode = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert fn(shape.ctypes.data_as(abi.c_i32p), xcd_local_allowed, C.byref(reason), C.byref(grid), C.byref(mode)) == 0
    return reason.value, grid.value, mode.value


def test_a_small_lp_qualifies_and_the_grid_is_the_larger_block_count():
    assert rule() == (PERSISTENT, 21, 1)
    assert rule(blocks_a=3, blocks_at=9) == (PERSISTENT, 9, 1)
    assert rule(blocks_a=1, blocks_at=1) == (PERSISTENT, 1, 1)  # afiro: the body without cross-workgroup traffic


@pytest.mark.parametrize("change,reason", [
    (dict(switch_on=0), SWITCH_OFF),
    (dict(sharded=1), SHARDED),
    (dict(profile=1), PROFILE),
    (dict(use_slab=1), SLAB),
    (dict(chunk_a=2048), NOT_512),
    (dict(chunk_at=2048), NOT_512),
    (dict(blocks_at=0), NOT_512),
    (dict(long_tasks=4), LONG_MAJOR),
    (dict(long_contrib=1), LONG_MAJOR),
    (dict(blocks_a=313, blocks_at=313), TOO_MANY),
    (dict(resident=20), NOT_RESIDENT),
    (dict(resident=0), NOT_RESIDENT),
])
def test_every_reason_code(change, reason):
    assert rule(**change)[0] == reason


def test_reasons_are_reported_in_the_order_of_the_table():
    """Where several reasons hold, the first of the table is the one reported: a slab solver says 4 whatever its block
    counts, a sharded one 2 whatever its layout."""
    everything = dict(switch_on=0, sharded=1, profile=1, use_slab=1, chunk_a=2048, long_tasks=1, blocks_a=100, resident=0)
    left = dict(everything)
    for key, reason in (("switch_on", SWITCH_OFF), ("sharded", SHARDED), ("profile", PROFILE), ("use_slab", SLAB),
                        ("chunk_a", NOT_512), ("long_tasks", LONG_MAJOR), ("blocks_a", TOO_MANY), ("resident", NOT_RESIDENT)):
        assert rule(**left)[0] == reason, key
        del left[key]
    assert rule(**left)[0] == PERSISTENT


def test_mode_threshold_32_33():
    assert rule(blocks_a=32, blocks_at=5) == (PERSISTENT, 32, 1)
    assert rule(blocks_a=5, blocks_at=32) == (PERSISTENT, 32, 1)
    assert rule(blocks_a=33, blocks_at=5) == (PERSISTENT, 33, 0)
    assert rule(blocks_a=5, blocks_at=33) == (PERSISTENT, 33, 0)
    assert rule(0, blocks_a=32) == (PERSISTENT, 32, 0)  # the XCD-local mode switched off, or given up after a failed placement check


def test_block_threshold_64_65():
    assert rule(blocks_a=64, blocks_at=64) == (PERSISTENT, 64, 0)
    assert rule(blocks_a=64, blocks_at=2) == (PERSISTENT, 64, 0)
    assert rule(blocks_a=65, blocks_at=2)[0] == TOO_MANY
    assert rule(blocks_a=2, blocks_at=65)[0] == TOO_MANY
    # residency counts the working workgroups: exactly as many as the grid is enough
    assert rule(blocks_a=64, resident=64)[0] == PERSISTENT and rule(blocks_a=64, resident=63)[0] == NOT_RESIDENT


def test_one_task_of_a_long_major_keeps_the_plain_launches():
    assert rule(long_tasks=1)[0] == LONG_MAJOR
    assert rule(long_tasks=0)[0] == PERSISTENT
    assert rule(long_tasks=1, blocks_a=1, blocks_at=1)[0] == LONG_MAJOR
