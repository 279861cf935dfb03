"""The comparisons of test_row_paths_gpu.py -- row thresholds, guarantee_nmin and the final graph of an injected pair-list
state against the oracle's NumPy restatements -- and, run as a script, a worker that does them for all row length classes in
one process and writes the mismatch counts as JSON (the row source and the second cut's minimum are read from the environment
once per process, hence a process per setting):

    python tests/row_paths_worker.py OUT.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import row_paths_cases as C  # noqa: E402
from oracle import annchor_oracle as O  # noqa: E402

N_NEIGHBORS, NMIN, NN = 20, 30, 21
ONE_LIST = [np.array([0.0])]
WORKER_CASES = ("sample_sees_large", "sample_sees_small", "ties_on_cut", "all_equal", "with_marks", "shrink_too_tight")


class Fixture:
    """One engine run up to get_features() on a complete pair list, with its index on the host."""

    def __init__(self, cls):
        from annchor_amd import Annchor, _native
        self.cls, self.nx, self.nat = cls, C.CLASSES[cls], _native
        ann = Annchor(C.points(cls), "euclidean", n_anchors=5, n_neighbors=N_NEIGHBORS, p_work=0.3, niters=1, random_seed=3)
        ann.get_anchors()
        ann.get_locality()
        ann.get_features()
        self.ann, self.eng = ann, ann._engine
        self.n = self.eng.field_size(_native.F_NCM)
        assert ann.n_pairs == self.n == self.nx * (self.nx - 1) // 2
        self.ptr = self.eng.download(_native.F_I_PTR)
        self.idx = self.eng.download(_native.F_I_IDX)
        self.IJs = self.eng.download(_native.F_IJS).reshape(-1, 2)
        ptr, idx, IJs = C.complete_index(self.nx)     # what the CPU tests build their cases on
        assert np.array_equal(self.ptr, ptr) and np.array_equal(self.idx, idx) and np.array_equal(self.IJs, IJs)
        self.len = self.nx - 1
        self.labels = None

    def case(self, case, want, mask="all"):
        return C.build_case(self.ptr, self.idx, self.IJs, self.cls, case, want=want, mask=mask, nmin=NMIN)

    def upload(self, RA, ncm, labels=None):
        self.eng.upload(self.nat.F_RA, RA)
        self.eng.upload(self.nat.F_NCM, ncm)
        labels = np.zeros(self.n, dtype=np.int64) if labels is None else labels
        if self.labels is None or not np.array_equal(self.labels, labels):
            self.eng.set_labels(labels)
            self.labels = labels

    def close(self):
        self.eng.close()


def ne(a, b):
    """Number of elements that differ (shape mismatch: everything)."""
    a, b = np.asarray(a), np.asarray(b)
    return int(max(a.size, b.size)) if a.shape != b.shape else int((a != b).sum())


def thresholds(F, RA, ncm, ks):
    """F_THRESH after select_candidates(k, nmin=0) against O.row_kth, k clamped to the row's last entry as the kernel does."""
    F.upload(RA, ncm)
    bad = 0
    for k in ks:
        F.eng.select_candidates(k, 0, ONE_LIST, 1, 1)
        bad += ne(F.eng.download(F.nat.F_THRESH), O.row_kth(RA, F.ptr, F.idx, min(k, F.len - 1)))
    return bad


def gn_state(F, RA, ncm):
    """The oracle's (thresholds, marked RefineApprox) of a first-iteration selection: thresholds first, as fit() does."""
    thr = O.row_kth(RA, F.ptr, F.idx, N_NEIGHBORS)
    return thr, O.guarantee_nmin(RA.copy(), ncm.astype(bool), F.ptr, F.idx, NMIN)


def guarantee_nmin(F, RA, ncm, want=None, errs=ONE_LIST, labels=None):
    """(RA mismatches, threshold mismatches, probability mismatches) of select_candidates(n_neighbors, nmin)."""
    thr, marked = gn_state(F, RA, ncm) if want is None else want
    F.upload(RA, ncm, labels)
    F.eng.select_candidates(N_NEIGHBORS, NMIN, errs, 7, 5)
    u = ncm.astype(bool)
    lab = np.zeros(F.n, dtype=np.int64) if labels is None else labels
    prob = O.refine_probabilities(marked, u, F.IJs, thr, lab, errs)
    return (ne(F.eng.download(F.nat.F_RA), marked), ne(F.eng.download(F.nat.F_THRESH), thr),
            ne(F.eng.download(F.nat.F_PROB)[u], prob))


def graph(F, RA, ncm, nns):
    F.upload(RA, ncm)
    bad = 0
    for nn in nns:
        gi, gd = F.eng.neighbor_graph(nn)
        oi, od = O.get_nn(RA, ncm.astype(bool), F.IJs, F.ptr, F.idx, nn)
        bad += ne(gi, oi) + ne(gd, od)
    return bad


def main(out):
    res = {}
    for cls in C.CLASSES:
        F = Fixture(cls)
        for case in WORKER_CASES:
            RA, ncm = F.case(case, N_NEIGHBORS + 1, "random70")
            res["%s/%s/thresh" % (cls, case)] = thresholds(F, RA, ncm, (N_NEIGHBORS, F.len + 5))
            RA, ncm = F.case(case, NMIN + 1, "row_counts")
            res["%s/%s/gn" % (cls, case)] = sum(guarantee_nmin(F, RA, ncm))
            RA, ncm = F.case(case, NN - 1, "random70")
            res["%s/%s/graph" % (cls, case)] = graph(F, RA, ncm, (NN,))
        F.close()
    with open(out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main(sys.argv[1])
