"""Hausdorff on point sets of 5 .. 512 coordinates per point on the device (csrc/hauswide.hip, k_hauswide) against the host
reference of hausdorff_cases.py, which loops over any dim.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import hausdorff_cases as hc
import pool_cases as pc
import radius_cases as rc
import seqdp_cases as sc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ref = pc.ref_cache()
SHORT = 192   # csrc/hauswide.hip HAUSW_SHORT: the longest set of a data set that still runs the 32 x 32 tile on one wave
# per shape: the tile's side and the lengths of the tile-edge data set (the longest decides the shape)
SHAPES = {"short": (32, [1, 2, 3, 4, 5, 31, 32, 33, SHORT]), "long": (64, sorted({1, 2, 63, 64, 65, 127, 128, 129, 200, SHORT + 1}))}


def check(key, X, dtype):
    """All ordered pairs of X (float32-representable values) on the device in `dtype` against the host; the key leaves dtype out
    on purpose: both dtypes hold the same values and share one reference."""
    IJ = pc.all_ordered_pairs(len(X))
    want = ref(key, lambda: hc.hausdorff_pairs_host(X, IJ))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("hausdorff", [x.astype(dtype) for x in X], IJ, wide=True)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("dim", [5, 16, 17, 64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_edges(shape, dim, dtype):
    """One set of each length around the tile's side, all ordered pairs: both orders put every length on the rows (row minima,
    the exchange between waves) and on the columns (colmin).  dim 5 is one partial chunk of 16 coordinates, 16 exactly one, 17
    one and one coordinate, 64 four."""
    X = sc.one_of_each_length(SHAPES[shape][1], dim, seed=40 + dim, dtype=F32)
    check(("edges", shape, dim), X, dtype)


@pytest.mark.parametrize("lengths, dim, dtype", [([4096, 4095, 1], 5, F64), ([70, 50, 9], 512, F32)])
def test_ceilings(lengths, dim, dtype):
    X = sc.one_of_each_length(lengths, dim, seed=50, dtype=F32)
    check(("ceiling", dim), X, dtype)


@pytest.mark.parametrize("far_last", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_deciding_direction(shape, far_last):
    """y is a random set of at least two tiles and 5 points (and of the shape's data set), x its first points and one far point, in the first strip or at the end of
    the last, partly clamped one.  h(x, y) is the far point's and decides: in the order (x, y) it is a row minimum, in the order
    (y, x) the far point is a column, of the last partly clamped column tile when it is last, and decides through colmin."""
    S = SHAPES[shape][0]
    rng = np.random.default_rng(60)
    y = rng.standard_normal((max(2 * S + 5, SHORT + 1 if shape == "long" else 0), 6))
    far = np.full((1, 6), 40.0)
    x = np.concatenate([y[:-10], far] if far_last else [far, y[:-10]])
    assert hc._directed_loop(x, y) > 100 * hc._directed_loop(y, x) > 0
    IJ = np.array([[0, 1], [1, 0]])
    assert np.array_equal(pc.device_pairs("hausdorff", [x, y], IJ, wide=True), hc.hausdorff_pairs_host([x, y], IJ))


def test_large_magnitudes():
    """Coordinates near 1e6 plus unit noise at dim 13: every square and every partial sum is rounded, and the pairwise order of
    np.sum changes the bits of more than a tenth of the c(i, j) -- so a reordered or fused sum would show."""
    rng = np.random.default_rng(90)
    X = [1e6 + rng.standard_normal((L, 13)) for L in (70, 50, 9)]
    a, b = X[0][:, None, :], X[1][None, :, :]
    assert np.mean(np.sum((a - b) * (a - b), axis=-1) != sc._sq(a, b)) > 0.1
    IJ = pc.all_ordered_pairs(len(X))
    assert np.array_equal(pc.device_pairs("hausdorff", X, IJ, wide=True), hc.hausdorff_pairs_host(X, IJ))


def test_opt_in():
    from annchor_amd import BruteForce, distances

    rng = np.random.default_rng(91)
    X5 = [rng.standard_normal((10, 5)), rng.standard_normal((12, 5))]
    for metric in (distances.Hausdorff(), "hausdorff"):
        with pytest.raises(ValueError, match="hausdorff: set 0 has dim 5; dim 1 .. 4 is supported"):
            BruteForce(X5, metric)
    X3 = sc.one_of_each_length([1, 40, 130, 600], 3, seed=92)
    IJ = pc.all_ordered_pairs(len(X3))
    assert np.array_equal(pc.device_pairs("hausdorff", X3, IJ, wide=True), pc.device_pairs("hausdorff", X3, IJ))
    with pytest.raises(ValueError, match="hausdorff: set 1 has dim 513; dim 1 .. 512 is supported"):
        BruteForce([np.zeros((3, 5)), np.zeros((3, 513))], distances.Hausdorff(wide=True))
    with pytest.raises(ValueError, match="hausdorff: set 1 has 4097 points; at most 4096 are supported"):
        BruteForce([np.zeros((3, 5)), np.zeros((4097, 5))], "hausdorff", func_kwargs={"wide": True})


def test_brute_force_and_radius_graph():
    from annchor_amd import Annchor, BruteForce, distances

    X = sc.clustered_curves(120, 20, 60, 16, seed=93)
    M = ref("fit", lambda: pc.sym_matrix(hc.hausdorff_pairs_host, X))
    bf = BruteForce(X, distances.Hausdorff(wide=True)).fit(10)
    oi, od, _ = O.brute_force(lambda IJ: M[IJ[:, 0], IJ[:, 1]], len(X))
    assert np.array_equal(bf.neighbor_graph[1], od[:, :10])
    assert np.array_equal(bf.neighbor_graph[0], oi[:, :10])
    r = float(np.percentile(M[np.triu_indices(len(X), 1)], 100 * 10 / len(X)))
    g = Annchor(X, "hausdorff", func_kwargs={"wide": True}, n_anchors=8).radius_graph(r)
    assert rc.same_graph((g.indptr, g.indices, g.distances), rc.graph_from_matrix(M, r))
