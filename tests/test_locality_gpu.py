"""Candidate generation (csrc/locality.hip) and the pair features (k_features* of csrc/features.hip) on injected anchor tables
chosen to sit on the kernels' edges, every kernel form, against oracle/annchor_oracle.py bit for bit: nearest-anchor masks,
IJs, the CSR index, lb / ub / dad / is_anchor, the not-computed mask, the returned n_pairs and min_row_len and the cached
not-computed count.  tests/locality_cases.py holds the cases, the four environment forms and the reference;
tests/test_locality_cases.py shows without a GPU that cases x forms reach every kernel and that the table notices a wrong
tie rule, keep rule, clamp or count.  The library reads its thresholds once per process: one worker process per form, one
after another, and the forms must also agree with each other (the same state from different kernels).  No tolerances."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import locality_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = {"failed": None, "runs": {}}     # the first form whose worker did not end well stops the rest


@pytest.fixture(scope="module")
def references():
    """Computed once in the test process, shared by the four forms, never written."""
    return ({nm: C.reference(nm) for nm in C.CASES}, {nm: C.query_reference(nm) for nm in C.QUERY_CASES})


def _raw_differences(a, b):
    keys = sorted(k for k in set(a.files) | set(b.files) if k != "seconds_on_cases")
    return [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or a[k].tobytes() != b[k].tobytes()]


@pytest.mark.parametrize("form", list(C.FORMS))
def test_locality_and_features_against_the_oracle(tmp_path, references, form):
    if STATE["failed"] is not None:
        pytest.fail("not started: the worker of form %r did not end well" % STATE["failed"])
    out = str(tmp_path / (form + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in C.FORM_VARIABLES}
    env.update(C.FORMS[form])
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "locality_worker.py"), out], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        STATE["failed"] = form
        raise
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        STATE["failed"] = form
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    print("locality form %-8s worker wall time %.1f s (%.1f s on the cases)" % (form, wall, float(got["seconds_on_cases"][0])))
    refs, qrefs = references
    bad = {}
    for nm, c in C.CASES.items():
        d = C.differences(C.decode(got, nm, c["nx"], c["na"]), refs[nm])
        if d:
            bad[nm] = d
    for nm, c in C.QUERY_CASES.items():
        want = qrefs[nm]
        dec = C.decode(got, nm, c["nx"], c["na"])
        # (an empty list leaves no state behind: the library reports no masks and no row pointers either)
        fields = C.FIELDS if want["n_pairs"] else ("IJs", "I_idx", "features", "ncm", "n_pairs", "min_row_len", "n_unc")
        d = C.differences(dec, want, fields)
        if not want["n_pairs"] and (dec["sid"].size or dec["I_ptr"].size):
            d.append("state of an empty list")
        if d:
            bad[nm] = d
    assert bad == {}, bad
    for other, prev in STATE["runs"].items():
        assert _raw_differences(prev, got) == [], (other, form)
    STATE["runs"][form] = got
