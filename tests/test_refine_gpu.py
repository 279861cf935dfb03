"""update_bounds (csrc/refine.hip) on injected states against an exact host reference: every case of tests/refine_cases.py in
every form of the intersection kernel (wave-per-pair with 16 / 32 / 64 lanes, row-grouped on 2- and 4-byte keys, the
dispatcher's own choice) and on every route to the computed-neighbour CSR (built in the call, prepared on the side stream,
the vectorised kernels over the column-ordered copy, the element-wise ones over it).  tests/test_refine_cases.py asserts
without a GPU that the reference is O.update_bounds bit for bit; here the lookahead list is the one the device selected, and
check_case() asserts on it that the case still reaches its edge.

Every candidate bound is one IEEE addition, or one subtraction and a fabs, of two stored doubles, and min / max do not depend
on the order they are taken in: the comparison is np.array_equal, there is no tolerance."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import refine_cases as R
import refine_worker as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixtures():
    made = {}

    def get(nx):
        if nx not in made:
            made[nx] = W.Fixture(nx)
        return made[nx]
    yield get
    for F in made.values():
        F.close()


@pytest.mark.parametrize("form", [f or "default" for f in R.FORMS])
@pytest.mark.parametrize("name", R.CASES)
def test_update_bounds_equals_the_reference(fixtures, name, form, monkeypatch):
    """lb and ub of the listed pairs equal the reference; every other pair and the dad / anchor columns are untouched."""
    F = fixtures(R.SIZES[name])
    t0 = time.time()
    F.case(name)
    t1 = time.time()
    if form == "default":
        monkeypatch.delenv("ANNCHOR_UPDATE_BOUNDS", raising=False)
        print("%s: %d listed pairs, the dispatcher takes %s" % (name, F.case(name)[1].shape[0], F.default_form(name)))
    else:
        monkeypatch.setenv("ANNCHOR_UPDATE_BOUNDS", form)
    bad = F.run(name)
    print("%s/%s: case and reference %.2f s, run %.2f s" % (name, form, t1 - t0, time.time() - t1))
    assert bad == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("name", R.CASES)
def test_update_bounds_on_prepared_lists(fixtures, name, monkeypatch):
    """The CSR's keys written ahead by update_bounds_prepare on the side stream (k_comp_fill<false>), the values by k_comp_vals."""
    F = fixtures(R.SIZES[name])
    monkeypatch.delenv("ANNCHOR_UPDATE_BOUNDS", raising=False)
    side, taken = F.eng.overlap_stats()
    assert side
    assert F.run(name, prepare=True) == (0, 0, 0, 0, 0)
    assert F.eng.overlap_stats() == (True, taken + 1)


SETTINGS = {"column_copy_vectorised": {"ANNCHOR_TRANSPOSE_MIN": "0", "ANNCHOR_ROWC_SHRINK_MIN": "16"},
            "column_copy_elementwise": {"ANNCHOR_TRANSPOSE_MIN": "0", "ANNCHOR_ROWC_SHRINK_MIN": "16", "ANNCHOR_COMP_GENERIC": "1"}}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_update_bounds_on_the_column_ordered_copy(tmp_path, setting):
    """k_comp_count_direct / k_comp_fill_direct (16 flags per load, unaligned heads and tails) and the element-wise kernels
    over the column-ordered copy: every case in a fresh child per setting, `csr_edges` in every form."""
    out = str(tmp_path / (setting + ".json"))
    env = dict(os.environ, **SETTINGS[setting])
    env.pop("ANNCHOR_UPDATE_BOUNDS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refine_worker.py"), out], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as fh:
        res = json.load(fh)
    runs = {k: v for k, v in res.items() if not k.endswith("/seconds")}
    assert len(runs) == len(R.CASES) - 1 + len(R.FORMS)
    assert {k: v for k, v in runs.items() if v != [0, 0, 0, 0, 0]} == {}
