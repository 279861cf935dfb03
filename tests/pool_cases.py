"""What the tests of the three metrics on ragged members (DTW, Frechet, Hausdorff) share: the pair lists, the fit configuration,
the cache of host references and the engine bound to a data set."""
import numpy as np

FIT_CFG = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, niters=2)


def all_ordered_pairs(nx):
    i, j = np.meshgrid(np.arange(nx), np.arange(nx), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], axis=1).astype(np.int64)


def sym_matrix(pairs_host, X):
    """pairs_host(X, IJ) on every pair, [nx, nx], computed for i <= j and mirrored: the three measures give the same bits in both
    orders (each test_*_host.py checks both orders against its loop, the small-length tests check both on the device)."""
    nx = len(X)
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = pairs_host(X, np.stack(iu, axis=1))
    T.T[iu] = T[iu]
    return T


def ref_cache():
    """ref(key, build) of one test module: a host reference, computed once and handed out read-only."""
    store = {}

    def ref(key, build):
        if key not in store:
            v = build()
            v.setflags(write=False)
            store[key] = v
        return store[key]

    return ref


def bound(metric, X, **metric_kwargs):
    """An engine with X bound under the bundled metric of that name."""
    from annchor_amd import _native
    from annchor_amd.utils import get_function_from_input

    eng = _native.Engine(0)
    get_function_from_input(metric, metric_kwargs).bind(eng, X)
    return eng


def device_pairs(metric, X, IJ, **metric_kwargs):
    eng = bound(metric, X, **metric_kwargs)
    try:
        return eng.metric_pairs(IJ)
    finally:
        eng.close()
