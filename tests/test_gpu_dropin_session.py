"""The resident solver behind the drop-in boundary: integration/capi_resolve_check.c, a plain C client of the reference's
C API, solves a model, changes column costs, a coefficient and a row's kind, and solves again after each — on the
drop-in libhighs (integration/_build, as tests/test_gpu_dropin.py: a missing build FAILS where the reference tree is
present).  With PDLP_MI355X_KEEP_SOLVER=1 the wrapper keeps one solver across the four Highs_run calls; what the client
prints must be the same strings, to the last digit, as without the variable."""
import os
import re
import subprocess

import pytest

from highs_amd import lp as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "integration", "_build")
GOLD = os.path.join(ROOT, "tests", "golden")
needs_build = pytest.mark.usefixtures("dropin_build")  # tests/conftest.py: FAILS where the reference tree is present and the build is not


def _env(**extra):
    e = dict(os.environ)
    e.pop("PDLP_MI355X_KEEP_SOLVER", None)
    e["LD_LIBRARY_PATH"] = BUILD + ":" + os.path.join(ROOT, "highs_amd", "lib") + ":" + e.get("LD_LIBRARY_PATH", "")
    e.update(extra)
    return e


def _run(tmp_path, mps, **env):
    """A fresh child process; a failed one ends the test before anything else runs on the GPU."""
    out = subprocess.run([os.path.join(BUILD, "capi_resolve_check"), mps, "1e-6", "1"], capture_output=True, text=True, timeout=120,
                         env=_env(**env), cwd=str(tmp_path))
    txt = out.stdout + out.stderr
    assert out.returncode == 0, txt[-3000:]
    results = [l for l in txt.splitlines() if l.startswith("capi_resolve_check: run=")]
    paths = re.findall(r"Session: ([a-z\- ]+?):", txt)
    return results, paths, txt


@needs_build
@pytest.mark.parametrize("name", ["adlittle"])
def test_resolves_through_highs_keep_their_bits_and_reuse_the_solver(tmp_path, name):
    assert os.path.exists(os.path.join(BUILD, "capi_resolve_check")), "make -C integration (capi_resolve_check)"
    mps = os.path.join(str(tmp_path), name + ".mps")
    L.write_mps(L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz")), mps)
    plain, plain_paths, plain_txt = _run(tmp_path, mps)
    assert len(plain) == 4, plain_txt[-3000:]
    assert plain_paths == [] and "Session:" not in plain_txt
    assert "model_status=7" in plain[0], plain[0]
    kept, kept_paths, kept_txt = _run(tmp_path, mps, PDLP_MI355X_KEEP_SOLVER="1")
    assert kept_paths == ["create", "update", "update matrix", "create"], kept_txt[-3000:]
    assert "changes kind" in kept_txt
    assert kept == plain, "\n".join(kept + plain)
    assert len(set(plain)) == 4  # the four runs solved four different models
    # 0 is unset
    zero, zero_paths, _ = _run(tmp_path, mps, PDLP_MI355X_KEEP_SOLVER="0")
    assert zero_paths == [] and zero == plain
