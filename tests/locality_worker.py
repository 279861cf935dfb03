"""Worker of test_locality_gpu.py: every pair-list case and every query case of tests/locality_cases.py in one process, one engine
per case, the downloads of each case written to an .npz under keys prefixed by the case name (the kernel-path thresholds are read
from the environment once per process, hence a process per form):

    python tests/locality_worker.py OUT.npz

No metric is bound (set_opaque): the anchor table is exactly what the case injects.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import locality_cases as C  # noqa: E402


def downloads(eng, nat, name, n_pairs, min_row_len, out):
    """The state the stage leaves behind.  An empty list (query form only) has no features to compute: every field is empty."""
    n_unc = 0
    if n_pairs > 0:
        eng.compute_features()
        n_unc = eng.count_uncomputed()
    for key, field in (("sid", nat.F_SID), ("ijs", nat.F_IJS), ("iptr", nat.F_I_PTR), ("iidx", nat.F_I_IDX),
                       ("feat", nat.F_FEATURES), ("ncm", nat.F_NCM)):
        out["%s__%s" % (name, key)] = eng.download(field)
    out["%s__meta" % name] = np.array([n_pairs, min_row_len, n_unc], dtype=np.int64)


def main(path):
    from annchor_amd import _native as nat
    out = {}
    t0 = time.perf_counter()
    for name, c in C.CASES.items():
        D, A = C.build(name)
        eng = nat.Engine()
        eng.set_opaque(c["nx"])
        eng.set_anchor_distances(D, A)
        n, m = eng.build_locality(c["locality"], c["loc_thresh"], c["loc_min"])
        downloads(eng, nat, name, n, m, out)
        eng.close()
    for name, c in C.QUERY_CASES.items():
        D, A = C.build_query(name)
        eng = nat.Engine()
        eng.set_opaque(c["nx"])
        eng.set_anchor_distances(D, A)
        n, m = eng.build_query_locality(c["nxb"], c["locality"], c["loc_thresh"])
        downloads(eng, nat, name, n, m, out)
        eng.close()
    out["seconds_on_cases"] = np.array([time.perf_counter() - t0])
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
