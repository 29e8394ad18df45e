"""The check iteration of solver="hipdlp" (tests/hipdlp_check_cases.py has the definitions): its 14 sums, the decision taken
on them and the copies the decision asks for, in both forms that run it, against references that depend on no summation order.

  form "device"  the gated launches of HalpernSolver::enqueueUnitTail — k_h_fpe_rows / k_h_fpe_cols, k_h_row_stats /
                 k_h_col_stats, k_diff_norm2, five k_final_reduce, then k_h_decide, k_h_restart_copy, k_h_keep_output —
                 stage check_device
  form "host"    the same kernels ungated, one download, halpernDecide on the host's copy of the state, the copies as
                 hipMemcpyAsync (the loop of sharded solves, profile mode and PDLP_MI355X_DEVICE_CHECK=0)   stage check_host
Every test reads the form it ran back from the solver (stage check_forms counts the decisions by who took them).

  a. integer data, no scaling: the statistics slots == the exact integers, the slack vectors == the reference's, in both forms,
     modes 0 (statistics only) and 2 (whole check behind the initial fixed-point error), at every size; the same with
     `scaled` switched on over planted power-of-two scales at 255 x 257 and 65537 x 300; the check of iteration 0 (derived
     slack, stage check_initial) on the same cases.  The products A x, A'y, A'dy the sums are built on == the integer products.
  b. real data, scaling on: |gpu - fsum| <= (len + 1) 2^-53 sum|term| (1 + 1e-6) per quantity, the bound for ANY summation
     order that tests/test_gpu_edges.py derives; the three products are held to the same bound major by major.
  c. every situation of hipdlp_check_cases.SITUATIONS at 255 x 257: record and state == the restated decision on the sums the
     device returned; x / x_anchor / y / y_anchor carry the bits of x_next / y_next where a restart is due and are untouched
     where not (x and y hold a NaN pattern, the anchors their planted values); out_x / out_y carry the iterate exactly when
     the check converged with `terminate`, else their NaN pattern.  The vector part also at 65537 x 300, 524288 x 524289
     (two trips of the copy kernels, split on a block boundary) and 255 x 524100 (split inside the first block).
  d. a halted state: check_device changes no statistics slot, no state word, no vector.
  e. the two forms agree bit for bit wherever both run (asserted inside a, b and c).
  f. the stage is the loop's check: after iterate(40) + iterate(40), in either loop, mode 0 on the vectors the solver holds
     reproduces the loop's own sums and the pFeas, dFeas, pObj, dObj, relGap and fpe of its last record bit for bit.
  g. one and two Halpern steps (stage steps; two also through steps_persistent) == an elementwise restatement of
     pdhg.cc:961-1018, from a start whose products are exact in any order, over every projection class of the columns.

Sizes: hipdlp_check_cases.SIZES — one element; 255 x 257; 256 x 256; 65537 x 300 (257 blocks); 196608 x 196609 (768 / 769
partials: the final reduction's unrolled loop starts at 769); 524288 x 524289 (the last size without and the first with a
second grid-stride trip); 255 x 524100 — and 255 x 257 with all five row kinds."""
import os

import numpy as np
import pytest

import edge_cases as E
import hipdlp_check_cases as H
from highs_amd import lp as L
from highs_amd import solver

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
STAGE = {"device": "check_device", "host": "check_host"}
CASES = [H.case_name(s) for s in H.SIZES] + [H.KINDS]
SIZE_OF = dict([(H.case_name(s), s) for s in H.SIZES] + [(H.KINDS, H.KINDS)])
COMPUTED = {0: (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13), 2: tuple(range(14))}  # the slots a mode writes
_runs = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nan_pattern(k, tag):
    """k quiet NaNs with distinct payloads: a vector nothing may have written to."""
    return (np.uint64(0x7FF8000000000000) + np.uint64(tag << 32) + np.arange(1, k + 1, dtype=np.uint64)).view(np.float64)


def _len(S, name):
    return S.m if name in H.ROW_VECTORS else S.n


def _get(S, name):
    return S.get(name, _len(S, name))


def _create(size, values):
    lp, F = H.case_lp(size, values), H.formulated(size, values)
    S = solver.DeviceSolver(lp=lp, **H.options(values))
    assert (S.n, S.m, S.n_eqs) == (F.n, F.m, F.n_eqs), (H.case_name(size), S.n, S.m, S.n_eqs)
    sc = S.setup_scalars()
    assert sc["scaled"] == (0.0 if values == "integer" else 1.0) and (sc["norm_cost"], sc["norm_rhs"]) == (F.norm_cost, F.norm_rhs)
    return lp, F, S


def _set_state(S, state, scaled):
    S.set("halpern_state", H.state_array(state, scaled))


def _forms_count(S):
    return tuple(int(t) for t in S.stage("check_forms", 2))


def _check(S, form, mode):
    """One check in the form asked for; the form is read back: a whole check (modes 1, 2) is one more decision of that form."""
    before = _forms_count(S)
    out = S.stage(STAGE[form], 16, init=[mode])
    after = _forms_count(S)
    if mode == 0:
        assert after == before
    else:
        halted = H.state_dict(S.get("halpern_state", 28))["halted"] and after == before  # (a halted device loop takes none)
        assert halted or after == ((before[0] + 1, before[1]) if form == "device" else (before[0], before[1] + 1)), (form, before, after)
    return out[:11]


def _plant(S, v):
    for k, a in v.items():
        S.set(k, a)


def _exact_zero_classes(S, F, v, scaled):
    """Real mode: the zero classes of the row residual and of the derived reduced cost, planted from the device's own products
    (deterministic: the same bits in every later launch), so that they are zero exactly and not up to rounding."""
    _set_state(S, dict(H.BASE), scaled)
    S.stage("check_initial", 16)
    aty0 = _get(S, "check_aty")
    z = (np.arange(F.n) // 5 + 1) % 3 == 1
    v["cost"][z] = aty0[z]
    S.set("cost", v["cost"])
    S.stage("check_device", 16, init=[0])
    ax = _get(S, "check_ax")
    z = H.row_class(F) == 1
    v["rhs"][z] = ax[z]
    S.set("rhs", v["rhs"])


def _products(S, F, v, integer):
    """A x_next, A'y_next and A'dy as the check computes them (and A x, A'y of the derived check): read from the device; integer
    mode: asserted equal to the exact integer products."""
    S.stage("check_initial", 16)
    prod = dict(ax0=_get(S, "check_ax"), aty0=_get(S, "check_aty"))
    S.stage("check_device", 16, init=[3])
    prod["dy"], prod["atd"] = _get(S, "delta_y"), _get(S, "check_aty")
    S.stage("check_device", 16, init=[0])
    prod["ax"], prod["aty"] = _get(S, "check_ax"), _get(S, "check_aty")
    assert np.array_equal(prod["dy"], v["y_next"] - v["y_reflected"])
    if integer:
        want = H.exact_products(F, v)
        for k in want:
            assert np.array_equal(prod[k], want[k]), (k, np.nonzero(prod[k] != want[k])[0][:8])
    return prod


def _run(case, values, mode, pow2=False):
    """The case's planted state through check_initial and through mode `mode` of both forms on ONE solver: run once, kept."""
    key = (case, values, mode, pow2)
    if key in _runs:
        return _runs[key]
    size = SIZE_OF[case]
    lp, F, S = _create(size, values)
    integer = values == "integer"
    scaled = pow2 or not integer
    rng = np.random.default_rng(21)
    v = H.plan(F, values, rng)
    if pow2:
        v.update(H.pow2_scales(F, np.random.default_rng(22)))
    _plant(S, v)
    state = dict(H.BASE, fpe0Pending=1, runFpe0=1) if mode == 2 else dict(H.BASE)
    if not integer:
        _exact_zero_classes(S, F, v, scaled)
    _set_state(S, state, scaled)
    assert H.state_dict(S.get("halpern_state", 28))["scaled"] == (1.0 if scaled else 0.0)
    prod = _products(S, F, v, integer)
    held = {k: _get(S, k) for k in H.ITERATE + H.DATA + (("col_scale", "row_scale") if scaled else ())}
    for k in v:
        assert np.array_equal(_bits(held[k]), _bits(v[k])), k
    unit = None if not integer else (2.0**-12 if pow2 else 1.0)
    kept = dict(F=F, prod=prod, ref=H.reference(held, prod, F.n_eqs, scaled, unit),
                ref0=H.reference_initial(held, dict(ax=prod["ax0"], aty=prod["aty0"]), F.n_eqs, scaled, unit), forms={})
    # the check of iteration 0: slots 3..8, the derived slacks, its record
    S.set("check_stats", np.array([-1.0] * 14 + [0.0, 0.0]))
    rec0 = S.stage("check_initial", 16)[:11]
    kept["initial"] = dict(stats=S.get("check_stats", 16), rec=rec0, slack_pos=_get(S, "slack_pos"), slack_neg=_get(S, "slack_neg"))
    for form in FORMS:
        _plant(S, {k: v[k] for k in ("x", "y", "x_anchor", "y_anchor")})  # (a restart of the form before has moved them)
        _set_state(S, state, scaled)
        S.set("check_stats", np.array([-1.0] * 14 + [0.0, 0.0]))
        rec = _check(S, form, mode)
        kept["forms"][form] = dict(stats=S.get("check_stats", 16), rec=rec, state=S.get("halpern_state", 28),
                                   slack_pos=_get(S, "slack_pos"), slack_neg=_get(S, "slack_neg"),
                                   ax=_get(S, "check_ax"), aty=_get(S, "check_aty"))
    S.close()
    kept["state"], kept["offset"] = state, lp.offset
    _runs[key] = kept
    return kept


def _assert_forms_agree(kept, what):
    a, b = kept["forms"]["device"], kept["forms"]["host"]
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, np.nonzero(_bits(a[k]) != _bits(b[k]))[0][:8])


def _assert_decision(kept, form, what):
    """Mode 2: the record and the state behind the check == the restated decision on the sums the device returned."""
    got = kept["forms"][form]
    F = kept["F"]
    after, rec = H.decide(kept["state"], got["stats"], kept["offset"], F.norm_rhs, F.norm_cost)
    want_state = H.state_array(after, got["state"][27] != 0.0)
    assert np.array_equal(got["state"], want_state), (what, form, [(H.STATE_NAMES[k], got["state"][k], want_state[k]) for k in np.nonzero(got["state"] != want_state)[0]])
    assert np.array_equal(got["rec"], H.record_array(rec)), (what, form, got["rec"], H.record_array(rec))


def _assert_exact(kept, mode, what):
    for form in FORMS:
        got, ref = kept["forms"][form], kept["ref"]
        want = np.array([q.exact for q in ref["q"]] + [0.0, 0.0])
        slots = list(COMPUTED[mode]) + [14, 15]
        bad = [k for k in slots if got["stats"][k] != want[k]]
        assert not bad, (what, form, [(H.STAT_NAMES[k], got["stats"][k], want[k]) for k in bad])
        assert all(got["stats"][k] == -1.0 for k in range(14) if k not in COMPUTED[mode])  # (what the mode does not compute is left alone)
        for k in ("slack_pos", "slack_neg"):
            assert np.array_equal(got[k], ref[k]), (what, form, k)
        if mode == 2:
            _assert_decision(kept, form, what)
    ini, ref0 = kept["initial"], kept["ref0"]
    want = np.array([q.exact for q in ref0["q"]])
    assert np.array_equal(ini["stats"][3:9], want), (what, "initial", ini["stats"][3:9], want)
    assert all(ini["stats"][k] == -1.0 for k in (0, 1, 2, 9, 10, 11, 12, 13))
    for k in ("slack_pos", "slack_neg"):
        assert np.array_equal(ini[k], ref0[k]), (what, "initial", k)
    _assert_initial_record(kept, what)
    _assert_forms_agree(kept, what)


def _assert_initial_record(kept, what):
    ini, F = kept["initial"], kept["F"]
    r, conv = H.residuals(ini["stats"], kept["offset"], F.norm_rhs, F.norm_cost, kept["state"]["tol"])
    want = [r[k] for k in H.RECORD_NAMES[1:7]]
    assert list(ini["rec"][1:7]) == want and ini["rec"][10] == (1.0 if conv else 0.0), (what, ini["rec"], want)


def _assert_within_bound(kept, mode, what):
    worst_all = 0.0
    for form in FORMS:
        got, ref = kept["forms"][form], kept["ref"]
        for qs, stats, offset, name in ((ref["q"], got["stats"], 0, form), (kept["ref0"]["q"], kept["initial"]["stats"], 3, "initial")):
            idx = [k for k in range(len(qs)) if offset or k in COMPUTED[mode]]
            err = np.array([abs(stats[k + offset] - qs[k].fsum) for k in idx])
            bound = np.array([H.any_order_bound(qs[k]) for k in idx])
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
            w = int(np.argmax(ratio))
            worst_all = max(worst_all, float(ratio[w]))
            print(what, name, "mode", mode, "worst quantity", H.STAT_NAMES[idx[w] + offset], "length", qs[idx[w]].length, "error", err[w],
                  "bound", bound[w], "ratio", ratio[w])
            assert np.all(err <= bound), (what, name, [(H.STAT_NAMES[idx[k] + offset], err[k], bound[k]) for k in np.nonzero(err > bound)[0]])
        for k in ("slack_pos", "slack_neg"):
            assert np.array_equal(got[k], ref[k]), (what, form, k)
        if mode == 2:
            _assert_decision(kept, form, what)
    for k in ("slack_pos", "slack_neg"):
        assert np.array_equal(kept["initial"][k], kept["ref0"][k]), (what, "initial", k)
    _assert_initial_record(kept, what)
    _assert_forms_agree(kept, what)
    print(what, "mode", mode, "worst error / bound", worst_all)


# ---- a, b, e: every size, both forms, modes 0 and 2 -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", CASES)
def test_integer_data_gives_the_exact_sums(case, mode):
    _assert_exact(_run(case, "integer", mode), mode, case)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", ["255x257", "65537x300", H.KINDS])
def test_integer_data_on_power_of_two_scales(case, mode):
    kept = _run(case, "integer", mode, pow2=True)
    _assert_exact(kept, mode, case + " scaled")
    plain = _run(case, "integer", mode)  # the scales enter: slots 3 and 5 differ from the unscaled run, the others do not
    a, b = kept["forms"]["device"]["stats"], plain["forms"]["device"]["stats"]
    assert a[3] != b[3] and a[5] != b[5] and all(a[k] == b[k] for k in COMPUTED[mode] if k not in (3, 5))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", CASES)
def test_real_data_stays_within_the_any_order_bound(case, mode):
    _assert_within_bound(_run(case, "real", mode), mode, case)


@pytest.mark.parametrize("case", ["255x257", H.KINDS, "65537x300", "524288x524289"])
def test_real_products_stay_within_the_any_order_bound(case):
    """A x_next, A'y_next, A'dy, A x and A'y of the checks, major by major, against the exact sum of the exact products."""
    kept = _run(case, "real", 0)
    F, prod = kept["F"], kept["prod"]
    # the vectors the products were taken of are the planted ones (asserted in _run): plan them again
    v = H.plan(F, "real", np.random.default_rng(21))
    csr, csc = F.A.tocsr(), F.A.tocsc()
    csr.sort_indices(); csc.sort_indices()
    for name, M, vec in (("ax", csr, v["x_next"]), ("aty", csc, v["y_next"]), ("atd", csc, prod["dy"]), ("ax0", csr, v["x"]), ("aty0", csc, v["y"])):
        exact, scale, lens = E.exact_major_sums(M.indptr, M.indices, M.data, vec)
        bound = (lens + 1) * 2.0**-53 * scale * (1 + 1e-6)
        err = np.abs(prod[name] - exact)
        w = int(np.argmax(err - bound))
        print(case, name, "worst major", w, "entries", lens[w], "error", err[w], "bound", bound[w])
        assert np.all(err <= bound), (case, name, np.nonzero(err > bound)[0][:8])
        assert np.all(prod[name][lens == 0] == 0.0)


# ---- c, d, e: the decision and its copies ---------------------------------------------------------------------------------------
def _situation(S, F, lp, base, prod, name, values, form, scaled):
    """Plants the situation on S, runs the whole check in `form`, compares with the restatement; returns what it read."""
    sit = H.SITUATIONS[name]
    v = {k: a.copy() for k, a in base.items()}
    if sit.tweak:
        sit.tweak(v, prod)
    nan_x, nan_y, nan_ox, nan_oy = _nan_pattern(F.n, 1), _nan_pattern(F.m, 2), _nan_pattern(F.n, 3), _nan_pattern(F.m, 4)
    _plant(S, dict(v, x=nan_x, y=nan_y, out_x=nan_ox, out_y=nan_oy))
    # the fixed-point error the thresholds are planted around: from the sums of a first pass (statistics only)
    _set_state(S, dict(H.BASE), scaled)
    S.stage("check_device", 16, init=[0])
    fpe = H.fixed_point_error(H.BASE["omega"], H.BASE["eta"], S.get("check_stats", 16)[0:3])
    state = H.situation_state(name, fpe)
    _set_state(S, state, scaled)
    poison = np.array([np.nan] * 16)
    S.set("check_stats", poison)
    watched = H.ITERATE + ("out_x", "out_y", "slack_pos", "slack_neg", "check_ax", "check_aty")
    before = {k: _get(S, k) for k in watched}
    rec = _check(S, form, sit.mode)
    got = dict(rec=rec, stats=S.get("check_stats", 16), state=S.get("halpern_state", 28), **{k: _get(S, k) for k in watched})
    taken = []
    after, want_rec = H.decide(state, got["stats"], lp.offset, F.norm_rhs, F.norm_cost, taken)
    for b in sit.branches:
        assert b in taken, (name, values, form, taken)
    want_state = H.state_array(after, scaled)
    assert np.array_equal(got["state"], want_state), (name, values, form, taken, [(H.STATE_NAMES[k], got["state"][k], want_state[k]) for k in np.nonzero(got["state"] != want_state)[0]])
    if name == "halted":  # d: nothing at all has changed
        assert np.all(np.isnan(got["stats"])) and not np.any(got["rec"])
        for k in watched:
            assert np.array_equal(_bits(got[k]), _bits(before[k])), (name, k)
        return got
    assert np.array_equal(got["rec"], H.record_array(want_rec)), (name, values, form, taken, got["rec"], H.record_array(want_rec))
    fresh = COMPUTED[2] if sit.mode == 2 and state["fpe0Pending"] else COMPUTED[0]  # every slot the check computes is rewritten, no other
    assert not np.any(np.isnan(got["stats"][list(fresh)])) and np.all(np.isnan(got["stats"][[k for k in range(16) if k not in fresh]]))
    restart, conv = after["doRestart"] == 1, after["converged"] == 1
    for k, src, untouched in (("x", "x_next", nan_x), ("x_anchor", "x_next", v["x_anchor"]), ("y", "y_next", nan_y), ("y_anchor", "y_next", v["y_anchor"])):
        want = v[src] if restart else untouched
        assert np.array_equal(_bits(got[k]), _bits(want)), (name, values, form, k, "restart" if restart else "no restart")
    for k, src, untouched in (("out_x", "x_next", nan_ox), ("out_y", "y_next", nan_oy)):
        want = v[src] if conv else untouched
        assert np.array_equal(_bits(got[k]), _bits(want)), (name, values, form, k, conv)
    for k in ("x_next", "y_next", "x_reflected", "y_reflected", "dual_slack"):
        assert np.array_equal(_bits(got[k]), _bits(v[k])), (name, k)
    return got


def _decision_case(case, values, names):
    size = SIZE_OF[case]
    lp, F, S = _create(size, values)
    integer = values == "integer"
    scaled = not integer
    base = H.plan(F, values, np.random.default_rng(21))
    if integer and size == (255, 257):
        H.square_fpe(F, base, H.BASE["eta"])
    _plant(S, base)
    if not integer:
        _exact_zero_classes(S, F, base, scaled)
    _set_state(S, dict(H.BASE), scaled)
    S.stage("check_device", 16, init=[0])
    prod = dict(ax=_get(S, "check_ax"), aty=_get(S, "check_aty"))
    for name in names:
        if H.SITUATIONS[name].integer_only and not integer:
            continue
        got = {form: _situation(S, F, lp, base, prod, name, values, form, scaled) for form in FORMS if not (form == "host" and name == "halted")}
        if len(got) == 2:  # e
            for k in got["device"]:
                if name == "fpe0_clear" and k == "stats":  # (the device's gate and the host's `if` both skip slots 9..11: poison stays)
                    assert np.all(np.isnan(got["device"][k][9:12])) and np.all(np.isnan(got["host"][k][9:12]))
                assert np.array_equal(_bits(got["device"][k]), _bits(got["host"][k])), (name, values, k)
    S.close()


@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("name", list(H.SITUATIONS))
def test_decision_and_copies_in_every_situation(name, values):
    _decision_case("255x257", values, [name])


@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("case", ["65537x300", "524288x524289", "255x524100"])
def test_copies_at_the_sizes_of_their_second_trip(case, values):
    _decision_case(case, values, H.VECTOR_SITUATIONS)


# ---- f: the stage is the loop's check -----------------------------------------------------------------------------------------
def _netlib(name):
    return L.HighsLp.from_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances", name + ".npz"))


@pytest.mark.parametrize("device_check", ["1", "0"])
@pytest.mark.parametrize("case", ["25fv47 persistent", "25fv47 plain", "65537x300"])
def test_the_stage_is_the_loops_check(case, device_check, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_DEVICE_CHECK", device_check)
    if case.startswith("25fv47"):
        monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
        monkeypatch.setenv("PDLP_MI355X_PERSISTENT_HIPDLP", "1" if case.endswith("persistent") else "0")
        lp = _netlib("25fv47")
    else:
        lp = H.case_lp((65537, 300), "real")
    S = solver.DeviceSolver(lp=lp, solver="hipdlp")
    reason = int(S.stage("persistent_reason")[0])
    assert (reason == 0) == case.endswith("persistent"), reason
    sc = S.setup_scalars()
    assert S.iterate(40).iters == 40
    first = H.state_dict(S.get("halpern_state", 28))  # what the second block and its check read
    assert first["iters"] == 40 and first["nRestarts"] == 1
    assert S.iterate(40).iters == 40
    assert _forms_count(S) == ((2, 0) if device_check == "1" else (0, 2))
    assert (int(S.stage("persistent_launches")[0]) > 0) == (reason == 0) and int(S.stage("barrier_fallbacks")[0]) == 0
    rec = S.get("last_record", 11)
    loop_stats = S.get("check_stats", 16)
    second = H.state_dict(S.get("halpern_state", 28))
    assert rec[0] == 80.0 and second["iters"] == 80 and second["halted"] == 1 and second["run"] == 0
    r, _ = H.residuals(loop_stats, lp.offset, sc["norm_rhs"], sc["norm_cost"], first["tol"])
    want = [r[k] for k in H.RECORD_NAMES[1:7]] + [H.fixed_point_error(first["omega"], first["eta"], loop_stats[0:3])]
    assert list(rec[1:8]) == want, (rec, want)
    held = {k: _get(S, k) for k in ("x_next", "y_next", "x_reflected", "y_reflected", "dual_slack")}
    for form in (("device", "host") if device_check == "1" else ("host", "device")):
        _set_state(S, dict(second, halted=0, run=1, runFpe0=0, doRestart=0), second["scaled"] != 0.0)
        S.set("check_stats", np.array([np.nan] * 16))
        _check(S, form, 0)
        stats = S.get("check_stats", 16)
        slots = [0, 1, 2, 3, 4, 5, 6, 7, 8] + ([] if rec[9] else [12, 13])  # (a restart has moved the anchors of slots 12, 13)
        assert np.array_equal(_bits(stats[slots]), _bits(loop_stats[slots])), (case, form, stats, loop_stats)
        r2, _ = H.residuals(stats, lp.offset, sc["norm_rhs"], sc["norm_cost"], first["tol"])
        assert [r2[k] for k in H.RECORD_NAMES[1:7]] + [H.fixed_point_error(first["omega"], first["eta"], stats[0:3])] == list(rec[1:8])
    for k, a in held.items():
        assert np.array_equal(_bits(_get(S, k)), _bits(a)), k
    S.close()


# ---- g: one Halpern step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,steps,launch", [(H.KINDS, 1, "plain"), (H.KINDS, 2, "plain"), (H.KINDS, 2, "persistent"),
                                               ("65537x300", 1, "plain"), ("65537x300", 2, "plain")])
def test_halpern_steps_equal_the_elementwise_restatement(case, steps, launch, monkeypatch):
    """stage steps (k = 1: one major step; k = 2: two) on the integer-matrix cases, from a start whose products are exact in
    any order (hipdlp_check_cases.step_plan): x, x_next, x_reflected, dual_slack, y, y_next, y_reflected == the elementwise
    restatement of pdhg.cc:961-1018.  k = 1 runs with a real dual step, real anchors and halpern_iteration 7 (w = 8 / 9);
    k = 2 keeps everything on a dyadic grid through the first step (sigma = 2, w = 1 / 2), so that the second step's products
    are exact too — its own blend (w = 2 / 3) is real.  The same two steps through the persistent launch where it exists."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    monkeypatch.setenv("PDLP_MI355X_PERSISTENT_HIPDLP", "1" if launch == "persistent" else "0")
    size = SIZE_OF[case]
    lp, F, S = _create(size, "integer")
    assert (int(S.stage("persistent_reason")[0]) == 0) == (launch == "persistent")
    rng = np.random.default_rng(23)
    bounds = H.plan(F, "integer", np.random.default_rng(21))
    d = H.step_plan(F, bounds["lower"], bounds["upper"], rng, dyadic_anchors=(steps == 2))
    d["rhs"], d["row_upper"] = _get(S, "rhs"), S.get("row_upper", S.m)
    assert np.array_equal(d["rhs"], F.rhs) and np.array_equal(d["cost"], _get(S, "cost"))
    assert np.array_equal(np.isinf(d["row_upper"]), np.arange(F.m) >= F.n_eqs) and np.array_equal(d["row_upper"][:F.n_eqs], d["rhs"][:F.n_eqs])
    tau, sigma, h_iter = 0.25, (0.37 if steps == 1 else 2.0), (7 if steps == 1 else 0)
    for k in ("x", "y", "x_anchor", "y_anchor", "lower", "upper"):
        S.set(k, d[k])
    nan = {k: _nan_pattern(_len(S, k), 5) for k in ("x_next", "y_next", "x_reflected", "y_reflected", "dual_slack")}
    _plant(S, nan)
    _set_state(S, dict(H.BASE, tau=tau, sigma=sigma, hIter=h_iter), False)
    S.stage("steps_persistent" if launch == "persistent" else "steps", 16, init=[steps])
    if launch == "persistent":
        assert int(S.stage("persistent_launches")[0]) == 1 and int(S.stage("barrier_fallbacks")[0]) == 0
        assert int(S.stage("persistent_reason")[0]) == 0
    got = {k: _get(S, k) for k in H.STEP_VECTORS}
    S.close()
    want = {k: a.copy() for k, a in d.items()}
    classes = None
    for i in range(1, steps + 1):
        temp = H.halpern_step(F.A, want, tau, sigma, h_iter, i, True)
        rx = want["x_reflected"]  # the operand of A x stays on its grid: the product is exact in any order
        assert np.array_equal(rx * 2.0**10, np.rint(rx * 2.0**10)) and np.abs(rx).max() < 2.0**20
        if i == 1:
            lo, up = d["lower"], d["upper"]
            classes = {"temp < l": temp < lo, "temp = l": temp == lo, "l < temp < u": (lo < temp) & (temp < up), "temp = u": temp == up,
                       "temp > u": temp > up, "l = -inf": lo == -H.INF, "u = inf": up == H.INF, "l = u": lo == up,
                       "-0.0 bound": ((lo == 0) & np.signbit(lo)) | ((up == 0) & np.signbit(up)),
                       "temp = 0 on a -0.0 bound": (temp == 0) & (((lo == 0) & np.signbit(lo)) | ((up == 0) & np.signbit(up)))}
    for name, mask in classes.items():
        assert mask.any(), name
    for k in H.STEP_VECTORS:
        assert np.array_equal(got[k], want[k]), (case, steps, launch, k, np.nonzero(got[k] != want[k])[0][:8])


# ---- the hooks themselves -------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_they_cannot_do():
    lp, F, S = _create((255, 257), "integer")
    for name in ("slack_pos", "slack_neg", "check_ax", "check_aty", "delta_y"):
        with pytest.raises(RuntimeError, match="can only be read"):
            S.set(name, np.zeros(_len(S, name)))
    with pytest.raises(RuntimeError, match="length mismatch"):
        S.get("halpern_state", 27)
    with pytest.raises(RuntimeError, match="mode 0..3"):
        S.stage("check_device", 16, init=[4])
    state = H.state_array(dict(H.BASE), True)
    S.set("halpern_state", state)
    assert np.array_equal(S.get("halpern_state", 28), state) and S.setup_scalars()["scaled"] == 1.0
    S.reset()  # a reset takes the planted scalars back (the planted `scaled` is the problem's: it stays until set again)
    back = H.state_dict(S.get("halpern_state", 28))
    assert back["iters"] == 0 and back["nChecks"] == 0 and back["run"] == 1 and back["halted"] == 0
    S.close()
