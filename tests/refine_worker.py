"""What test_refine_gpu.py runs -- one update_bounds on an injected state of tests/refine_cases.py against the exact host
reference -- and, run as a script, a worker that does it for every case in one process and writes the mismatch counts as JSON
(which kernels build the computed-neighbour CSR is read from the environment once per process, hence a process per setting):

    python tests/refine_worker.py OUT.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refine_cases as R  # noqa: E402

WORKER_FORMS = {"csr_edges": R.FORMS}      # every form on the rows built for the CSR kernels, the dispatcher's choice elsewhere


class Fixture:
    """One engine run up to get_features() on the index of a size class, with the index on the host."""

    def __init__(self, nx):
        from annchor_amd import Annchor, _native
        self.nx, self.nat = nx, _native
        if nx == R.HIGH:
            ann = Annchor(R.high_points()[0], "euclidean", p_work=0.01, n_samples=2000, niters=1, **R.HIGH_CFG)
        else:
            ann = Annchor(np.random.default_rng(nx).standard_normal((nx, 2)), "euclidean", n_anchors=5, n_neighbors=20,
                          p_work=0.3, niters=1, random_seed=3)
        ann.get_anchors()
        ann.get_locality()
        ann.get_features()
        self.ann, self.eng = ann, ann._engine
        self.n = self.eng.field_size(_native.F_NCM)
        self.ix = R.Index(self.eng.download(_native.F_I_PTR), self.eng.download(_native.F_I_IDX),
                          self.eng.download(_native.F_IJS).reshape(-1, 2))
        assert self.ix.n == self.n and (nx == R.HIGH or self.n == nx * (nx - 1) // 2)
        self.cases = {}
        self.eng.set_labels(np.zeros(self.n, dtype=np.int64))

    def case(self, name):
        """(case, lookahead list, reference lb, reference ub): built, selected on the device and checked once."""
        if name not in self.cases:
            case = R.build_case(self.ix, None, None, name)
            nxt = self.select(case)
            # (n_neighbors beyond every row: the threshold is the row's largest entry)
            assert np.array_equal(self.eng.download(self.nat.F_THRESH), np.maximum.reduceat(case.RA[self.ix.idx], self.ix.ptr[:-1]))
            lb, ub = R.check_case(case, self.ix, nxt)
            self.cases[name] = (case, nxt, lb, ub)
        return self.cases[name]

    def select(self, case):
        nat = self.nat
        self.eng.upload(nat.F_RA, case.RA)
        self.eng.upload(nat.F_NCM, case.ncm)
        self.eng.upload(nat.F_FEATURES, case.feats)
        k, n_refine, lookahead = case.sel
        _, nn = self.eng.select_candidates(k, 0, R.ONE_LIST, n_refine, lookahead)
        nxt = self.eng.download(nat.F_NEXT)
        assert nn == nxt.shape[0]
        return nxt

    def run(self, name, prepare=False):
        """Upload, select, update_bounds; the number of feature entries that differ from the reference: (lb, ub of listed
        pairs, lb, ub of the others, dad and anchor columns)."""
        case, nxt, lb, ub = self.case(name)
        again = self.select(case)
        if not np.array_equal(again, nxt):
            return (-1,) * 5
        if prepare:
            self.eng.update_bounds_prepare()
        self.eng.update_bounds()
        got = self.eng.download(self.nat.F_FEATURES).reshape(-1, 4)
        listed = np.zeros(self.n, dtype=bool)
        listed[nxt] = True
        bl, bu = got[:, 0] != lb, got[:, 1] != ub
        return (int(bl[listed].sum()), int(bu[listed].sum()), int(bl[~listed].sum()), int(bu[~listed].sum()),
                int((got[:, 2:] != case.feats[:, 2:]).sum()))

    def default_form(self, name):
        """The form the dispatcher takes by itself (the rule of annchor_update_bounds on the mean computed-list length)."""
        case = self.case(name)[0]
        avg = 2.0 * float((case.ncm == 0).sum()) / self.nx
        return "bits16" if avg >= 256.0 and self.nx <= 131072 else "bits32" if avg >= 256.0 else "pairs16" if avg < 192.0 else "pairs32"

    def close(self):
        self.eng.close()


def set_form(form):
    if form is None:
        os.environ.pop("ANNCHOR_UPDATE_BOUNDS", None)
    else:
        os.environ["ANNCHOR_UPDATE_BOUNDS"] = form


def main(out):
    res = {}
    for nx in (R.SMALL, R.MID, R.HIGH):
        F = Fixture(nx)
        for name in [c for c in R.CASES if R.SIZES[c] == nx]:
            for form in WORKER_FORMS.get(name, (None,)):
                set_form(form)
                t0 = time.time()
                res["%s/%s" % (name, form or "default")] = list(F.run(name))
                res["%s/%s/seconds" % (name, form or "default")] = time.time() - t0
        set_form(None)
        F.close()
    with open(out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main(sys.argv[1])
