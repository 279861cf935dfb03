"""
Bundled metrics (reference annchor/distances.py:8-20 and the wasserstein closure of
annchor/utils.py:75-86).

Each bundled metric is a `DeviceMetric`: a callable f(x, y) -- what the reference
hands to plugins as `ann.f` -- whose arithmetic runs in the HIP kernels of
libannchor_hip.so.  Called on two loose objects it evaluates them on the GPU through
a scratch context; inside `Annchor` the data set is uploaded once and whole pair
lists are evaluated per call (`get_exact_ijs`).  There is no CPU implementation.
"""
import os

import numpy as np

from . import _native


def encode_strings(strings):
    """Python strings -> (codes uint8 or uint16, offs int64, lens int32, alphabet size).
    Symbols are mapped to dense codes 0..A-1: one byte per symbol up to 256 distinct symbols, two bytes up to 65 535."""
    strings = list(strings)
    lens = np.fromiter((len(s) for s in strings), dtype=np.int32, count=len(strings))
    joined = "".join(strings)
    try:
        # every code point below 256 (the usual case): one byte per symbol, dense codes through a
        # 256-entry table -- the general path below sorts the whole text to find its alphabet
        # (10 ms for the 0.8 M symbols of the C2 data set, against a 5.5 ms fit)
        raw = np.frombuffer(joined.encode("latin-1"), dtype=np.uint8)
        present = np.bincount(raw, minlength=256) > 0
        symbols = np.flatnonzero(present)
        codes = (np.cumsum(present) - 1).astype(np.uint8)[raw]
    except UnicodeEncodeError:
        raw = np.frombuffer(joined.encode("utf-32-le"), dtype=np.uint32)
        symbols = np.unique(raw)
        if symbols.size > 65535:
            raise ValueError("levenshtein on the GPU supports at most 65 535 distinct symbols, got %d" % symbols.size)
        codes = np.searchsorted(symbols, raw).astype(np.uint8 if symbols.size <= 256 else np.uint16)
    if os.environ.get("ANNCHOR_LEV_WIDE"):   # test hook: the 16-bit path on any alphabet
        codes = codes.astype(np.uint16)
    offs = np.zeros(len(strings), dtype=np.int64)
    if len(strings) > 1:
        np.cumsum(lens[:-1], out=offs[1:])
    if codes.size == 0:
        codes = np.zeros(1, dtype=codes.dtype)
    return codes, offs, lens, max(1, int(symbols.size))


class DeviceMetric:
    """Base class of the GPU-evaluated metrics."""

    name = "device"
    _scratch = None

    def bind(self, engine, X):
        """Upload the data set X into `engine` for pair-list evaluation."""
        raise NotImplementedError

    def _scratch_engine(self):
        if DeviceMetric._scratch is None:
            DeviceMetric._scratch = _native.Engine(0)
        return DeviceMetric._scratch

    def many(self, xs, ys):
        """f(xs[t], ys[t]) for loose objects, evaluated on the GPU."""
        xs, ys = list(xs), list(ys)
        eng = self._scratch_engine()
        self.bind(eng, xs + ys)
        n = len(xs)
        IJ = np.stack([np.arange(n), np.arange(n) + n], axis=1)
        return eng.metric_pairs(IJ)

    def one_to_many(self, x, ys):
        ys = list(ys)
        eng = self._scratch_engine()
        self.bind(eng, [x] + ys)
        IJ = np.stack([np.zeros(len(ys), dtype=np.int64), np.arange(len(ys)) + 1], axis=1)
        return eng.metric_pairs(IJ)

    def __call__(self, x, y):
        return self.many([x], [y])[0]


class _Levenshtein(DeviceMetric):
    """Unit-cost edit distance (distances.py:16-20)."""

    name = "levenshtein"

    def bind(self, engine, X):
        engine.set_strings(*encode_strings(X))

    def __call__(self, x, y):
        return int(self.many([x], [y])[0])


class _Euclidean(DeviceMetric):
    """np.linalg.norm(x - y) in the dtype of X (distances.py:8-13)."""

    name = "euclidean"

    def bind(self, engine, X):
        X = np.asarray(X)
        if X.ndim == 1:
            X = X[:, None]
        if X.dtype != np.float32:
            X = X.astype(np.float64)
        engine.set_points(X)


class _Cosine(DeviceMetric):
    """scipy.spatial.distance.cosine(x, y) = 1 - x.y / (|x| |y|), the dot products in the dtype of
    X, clipped to [0, 2] (utils.py:14,67)."""

    name = "cosine"

    def bind(self, engine, X):
        X = np.asarray(X)
        if X.ndim == 1:
            X = X[:, None]
        if X.dtype != np.float32:
            X = X.astype(np.float64)
        engine.set_points(X, cosine=True)


class Wasserstein(DeviceMetric):
    """kantorovich(x, y, cost=M): exact optimal transport between the normalised
    histograms restricted to their supports (utils.py:75-86).

    wide=False: up to 64 bins, or up to 1024 bins with at most 32 non-zero entries per
    histogram under a metric cost.  wide=True additionally takes, under a metric cost,
    any histograms of up to 256 bins and histograms of up to 1024 bins with at most 128
    non-zero entries each (solves of up to 256 nodes); data the narrow form takes is
    evaluated exactly as without it."""

    name = "wasserstein"

    def __init__(self, cost_matrix, wide=False):
        self.cost_matrix = np.ascontiguousarray(cost_matrix, dtype=np.float64)
        self.wide = bool(wide)

    def bind(self, engine, X):
        engine.set_histograms(np.asarray(X, dtype=np.float64), self.cost_matrix, wide=self.wide)


DTW_MAX_LENGTH = 2048


def pack_series(X):
    """Time series -> (values float32 or float64, offs int64, lens int32).  X is a 2-D float array (rows are series) or a
    sequence of 1-D arrays of any lengths.  float32 stays float32 when every series is float32 (the kernel widens it
    exactly); anything else becomes float64.  Refused here, on the host, before anything is uploaded: an empty series, a
    series longer than DTW_MAX_LENGTH, a series that is not one-dimensional, a value that is not finite."""
    return _pack_points(X, "dtw", "series", 1, lambda dim: DTW_MAX_LENGTH, plural="series", univariate=True)[:3]


DTW_MAX_DIM = 4


def dtw_max_length(dim):
    """The longest series the kernel takes at `dim` coordinates per point: Frechet's limits, 2048 points up to dim 2 (at dim 1
    that is DTW_MAX_LENGTH), 1024 at dim 3 and 4."""
    return 2048 if dim <= 2 else 1024


def pack_dtw_series(X):
    """Series of 1 .. 4 coordinates per point -> (values float32 or float64 [points * dim], offs int64, lens int32, dim): what
    pack_curves takes and returns, refused as "dtw: series <index> ..." with DTW_MAX_DIM and dtw_max_length(dim) as the limits."""
    return _pack_points(X, "dtw", "series", DTW_MAX_DIM, dtw_max_length, plural="series")


class DTW(DeviceMetric):
    """Dynamic time warping between series (no counterpart in the reference), in float64.  A series is 1 .. L points of `dim`
    coordinates, dim in 1 .. 4; a 1-D member is a series of dim 1.

        c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]     (dim 1: (x_i - y_j)^2;
                  every subtraction, product and addition rounded on its own, never an fma)
        D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)),  D(-1, -1) = 0, +inf outside the matrix
        dtw(x, y) = sqrt(D(n-1, m-1))

    window=None: unconstrained.  An integer window >= 0 is a Sakoe-Chiba band that always reaches the corner: cells with
    |i - j| > max(window, |n - m|) are +inf.  The value equals the sequential recurrence bit for bit (csrc/seqdp.hip).

    X is a 2-D array (rows are univariate series), a sequence of 1-D arrays (univariate series of any lengths), a sequence
    of [len, dim] arrays, or a 3-D array [nx, len, dim].

    Limits: dim 1 .. 4; 1 .. 2048 points at dim <= 2, 1 .. 1024 points at dim 3 and 4; finite values; one dim for a data set
    and its queries.  Other step patterns, derivative or weighted DTW and bucketing the series by length are out of scope.
    DTW can violate the triangle inequality: pass is_metric=False to Annchor."""

    name = "dtw"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, window=None):
        if window is not None:
            if int(window) != window or window < 0:
                raise ValueError("dtw: window must be None or an integer >= 0")
            window = int(window)
        self.window = window

    def bind(self, engine, X):
        if not isinstance(X, np.ndarray):
            X = list(X)
        if X.ndim == 2 if isinstance(X, np.ndarray) else all(np.ndim(x) == 1 for x in X):
            engine.set_series(*pack_series(X), window=self.window)   # rows of a 2-D array, or 1-D members: univariate, as ever
        else:
            values, offs, lens, dim = pack_dtw_series(X)
            engine.set_series_nd(values, offs, lens, dim, window=self.window)


EDR_MAX_DIM = LCSS_MAX_DIM = 4


def edr_max_length(dim):
    """The longest series the kernel takes at `dim` coordinates per point: Frechet's limits, 2048 points up to dim 2, 1024 at dim
    3 and 4."""
    return 2048 if dim <= 2 else 1024


def lcss_max_length(dim):
    """EDR's limits."""
    return edr_max_length(dim)


def pack_edr_series(X):
    """Series -> (values float32 or float64 [points * dim], offs int64, lens int32, dim): what pack_erp_series takes and returns,
    refused as "edr: series <index> ..." with edr_max_length(dim) as the length limit."""
    return _pack_points(X, "edr", "series", EDR_MAX_DIM, edr_max_length, plural="series")


def pack_lcss_series(X):
    """The same, refused as "lcss: series <index> ..." with lcss_max_length(dim) as the length limit."""
    return _pack_points(X, "lcss", "series", LCSS_MAX_DIM, lcss_max_length, plural="series")


class EDR(DeviceMetric):
    """Edit distance on real sequences (Chen, Ozsu & Oria 2005) between series (no counterpart in the reference).  A series is
    1 .. L points of `dim` coordinates, dim in 1 .. 4.  All arithmetic is float64; float32 input widens exactly.  `eps` is the
    matching threshold, a finite float64 >= 0 without a default: the right value is a property of the data's scale.

        match(p, q) iff fabs(p[k] - q[k]) <= eps for every k = 0 .. dim-1      (each subtraction rounded on its own; a difference of
                    exactly eps matches; a threshold per coordinate as in the paper, not a Euclidean ball)
        E(-1, -1) = 0     E(i, -1) = i + 1     E(-1, j) = j + 1
        E(i, j) = min( E(i-1, j-1) + (match(x[i], y[j]) ? 0.0 : 1.0),   E(i-1, j) + 1.0,   E(i, j-1) + 1.0 )
        edr(x, y) = E(n-1, m-1)                       normalize=False (the default: an edit count, like "levenshtein")
                  = E(n-1, m-1) / (double)max(n, m)   normalize=True  (one float64 division)

    Every cell is a small integer that float64 holds exactly, so the value equals the sequential recurrence bit for bit
    (csrc/seqdp.hip), and edr(x, y) == edr(y, x) exactly.  A point that is far off costs 1 and not its distance: EDR is robust to
    outliers and noise.  It is no metric: it violates the triangle inequality, and edr(x, y) = 0 does not imply x = y: pass
    is_metric=False to Annchor.  Normalised EDR saturates: between well-separated groups most distances are close to 1.0, and
    the stratified sampler of a fit can then raise "Some sampler bins contain too few samples", as it would in the reference.

    Limits: dim 1 .. 4; 1 .. 2048 points at dim <= 2, 1 .. 1024 points at dim 3 and 4; finite values; finite eps >= 0; one dim
    for a data set and its queries."""

    name = "edr"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, eps, normalize=False):
        self.eps = _real_parameter("edr", "eps", eps, 0.0, False)
        if not isinstance(normalize, (bool, np.bool_)):
            raise ValueError("edr: normalize must be True or False")
        self.normalize = bool(normalize)

    def bind(self, engine, X):
        values, offs, lens, dim = pack_edr_series(X)
        engine.set_edr_series(values, offs, lens, dim, self.eps, self.normalize)


class LCSS(DeviceMetric):
    """Longest-common-subsequence distance (Vlachos, Kollios & Gunopulos 2002) between series (no counterpart in the reference).
    Series, `eps` and match are EDR's.  `delta` is None, or an integer >= 0 that limits how far apart in time two matched points
    may be; it is plain, not widened to |n - m| as DTW's band is.

        L(-1, -1) = L(i, -1) = L(-1, j) = 0
        L(i, j) = L(i-1, j-1) + 1.0          if match(x[i], y[j]) and (delta is None or |i - j| <= delta)
                = max(L(i-1, j), L(i, j-1))  otherwise
        lcss(x, y) = 1.0 - L(n-1, m-1) / (double)min(n, m)      (one division, one subtraction; in [0, 1])

    Every cell is a small integer that float64 holds exactly, so the value equals the sequential recurrence bit for bit
    (csrc/seqdp.hip), and lcss(x, y) == lcss(y, x) exactly.  It is no metric: pass is_metric=False to Annchor.  LCSS saturates:
    between well-separated groups most distances are exactly 1.0, and the stratified sampler of a fit then raises "Some sampler
    bins contain too few samples", as it would in the reference; choose eps by the data's scale.

    Limits: EDR's; delta None or an integer >= 0."""

    name = "lcss"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, eps, delta=None):
        self.eps = _real_parameter("lcss", "eps", eps, 0.0, False)
        if delta is not None:
            if isinstance(delta, (bool, np.bool_)) or not isinstance(delta, (int, np.integer)) or delta < 0:
                raise ValueError("lcss: delta must be None or an integer >= 0")
            delta = int(delta)
        self.delta = delta

    def bind(self, engine, X):
        values, offs, lens, dim = pack_lcss_series(X)
        engine.set_lcss_series(values, offs, lens, dim, self.eps, self.delta)


FRECHET_MAX_DIM = 4


def frechet_max_length(dim):
    """The longest curve the kernel takes at `dim` coordinates per point: 2048 points up to dim 2, 1024 at dim 3 and 4."""
    return 2048 if dim <= 2 else 1024


def _pack_points(X, metric, noun, max_dim, max_length, plural=None, univariate=False):
    """pack_series, pack_curves, pack_point_sets and pack_clouds: members of [len, dim] or [len] -> (values, offs, lens, dim), refusals
    worded "<metric>: <noun> <index> ..."; max_length(dim) is the longest member taken.  univariate: members of [len] only,
    their lengths counted in values."""
    plural = plural or noun + "s"
    if isinstance(X, np.ndarray) and X.ndim in (2, 3):
        rows = list(X)
    else:
        rows = [np.asarray(x) for x in X]
    if not rows:
        raise ValueError("%s: no %s" % (metric, plural))
    for s, x in enumerate(rows):
        if univariate and x.ndim != 1:
            raise ValueError("%s: %s %d has %d dimensions; univariate %s only" % (metric, noun, s, x.ndim, plural))
        if x.ndim not in (1, 2):
            raise ValueError("%s: %s %d has %d dimensions; a %s is [len, dim] or [len]" % (metric, noun, s, x.ndim, noun))
        if x.dtype.kind not in "fiub":
            raise ValueError("%s: %s %d has dtype %s; real numbers only" % (metric, noun, s, x.dtype))
    dims = [1 if x.ndim == 1 else int(x.shape[1]) for x in rows]
    dim = dims[0]
    for s, d in enumerate(dims):
        if d < 1 or d > max_dim:
            raise ValueError("%s: %s %d has dim %d; dim 1 .. %d is supported" % (metric, noun, s, d, max_dim))
        if d != dim:
            raise ValueError("%s: %s %d has dim %d, %s 0 has dim %d; all %s share one dim" % (metric, noun, s, d, noun, dim, plural))
    dtype = np.float32 if all(x.dtype == np.float32 for x in rows) else np.float64
    lens = np.fromiter((x.shape[0] for x in rows), dtype=np.int64, count=len(rows))
    limit = max_length(dim)
    if lens.min() < 1:
        raise ValueError("%s: %s %d is empty" % (metric, noun, int(np.argmin(lens))))
    if lens.max() > limit:
        raise ValueError("%s: %s %d has %d %s; at most %d are supported%s"
                         % (metric, noun, int(np.argmax(lens)), int(lens.max()), "values" if univariate else "points", limit,
                            "" if univariate else " at dim %d" % dim))
    values = np.concatenate([np.asarray(x, dtype=dtype).reshape(-1) for x in rows])
    if not np.all(np.isfinite(values)):
        bad = int(np.searchsorted(np.cumsum(lens) * dim, int(np.flatnonzero(~np.isfinite(values))[0]), side="right"))
        raise ValueError("%s: %s %d holds a value that is not finite" % (metric, noun, bad))
    offs = np.zeros(len(rows), dtype=np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    return values, offs, lens.astype(np.int32), dim


def pack_curves(X):
    """Curves -> (values float32 or float64 [points * dim], offs int64, lens int32, dim); offs and lens count points.

    X is a sequence of curves -- each a 2-D array [len, dim], or a 1-D array (a curve of dim 1) -- or a 3-D array
    [nx, len, dim] (nx curves of equal length), or a 2-D array [nx, len] (nx univariate rows).  float32 stays float32 when
    every curve is float32 (the kernel widens it exactly); anything else becomes float64.  Refused here, on the host, before
    anything is uploaded and with the curve's index in the message: curves of different dim, a dim beyond FRECHET_MAX_DIM,
    an empty curve, a curve longer than frechet_max_length(dim), a dtype that is not real, a value that is not finite."""
    return _pack_points(X, "frechet", "curve", FRECHET_MAX_DIM, frechet_max_length)


class Frechet(DeviceMetric):
    """Discrete Frechet distance between curves (no counterpart in the reference).  A curve is a sequence of 1 .. L points of
    `dim` coordinates, dim in 1 .. 4.  All arithmetic is float64; float32 input widens exactly.

        c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]
                  (every subtraction, product and addition rounded on its own, never an fma;
                   the sum starts from the k = 0 product, not from 0.0 + ...)
        F(i, j) = max(c(i, j), min(F(i-1, j), F(i, j-1), F(i-1, j-1))),   F(-1, -1) = 0, +inf outside the matrix
        frechet(x, y) = sqrt(F(n-1, m-1)), correctly rounded

    max and min are exact and every c(i, j) has fixed operands, so the value equals the sequential recurrence bit for bit
    (csrc/seqdp.hip).  There is no window: a banded Frechet distance loses the triangle inequality.  It is a metric on
    point sequences (a pseudo-metric: two different curves can be at distance 0), so is_metric=True is its intended setting.

    Limits: dim 1 .. 4; 1 .. 2048 points at dim <= 2, 1 .. 1024 points at dim 3 and 4; finite values; one dim for a data
    set and its queries."""

    name = "frechet"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def bind(self, engine, X):
        engine.set_curves(*pack_curves(X))


ERP_MAX_DIM = 4


def erp_max_length(dim):
    """The longest series the kernel takes at `dim` coordinates per point: 2048 values at dim 1, 1024 points at dim 2, 3 and 4."""
    return 2048 if dim == 1 else 1024


def pack_erp_series(X):
    """Series -> (values float32 or float64 [points * dim], offs int64, lens int32, dim); offs and lens count points.

    X is what pack_curves takes: a sequence of series -- each a 2-D array [len, dim], or a 1-D array (a series of dim 1) -- or
    a 3-D array [nx, len, dim] (nx series of equal length), or a 2-D array [nx, len] (nx univariate rows).  float32 stays
    float32 when every series is float32 (the kernel widens it exactly); anything else becomes float64.  Refused here, on the
    host, before anything is uploaded and with the series' index in the message: series of different dim, a dim beyond
    ERP_MAX_DIM, an empty series, a series longer than erp_max_length(dim), a dtype that is not real, a value that is not
    finite."""
    return _pack_points(X, "erp", "series", ERP_MAX_DIM, erp_max_length, plural="series")


class ERP(DeviceMetric):
    """Edit distance with real penalty (Chen & Ng 2004) between series (no counterpart in the reference).  A series is 1 .. L
    points of `dim` coordinates, dim in 1 .. 4.  All arithmetic is float64; float32 input widens exactly.  `gap` is the gap
    value g, a finite float64 scalar with default 0.0.  The gap point is (g, ..., g).

        dist(a, b)  dim 1:   |a[0] - b[0]|
                    dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = a[k] - b[k],  correctly rounded sqrt
                    (every subtraction, product and addition rounded on its own, never an fma; the sum starts from the k = 0 product)
        gx(i) = dist(x[i], gap point)        gy(j) = dist(y[j], gap point)
        E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + gx(i)     E(-1, j) = E(-1, j-1) + gy(j)        (left to right, one addition per step)
        E(i, j) = min( E(i-1, j-1) + dist(x[i], y[j]),   E(i-1, j) + gx(i),   E(i, j-1) + gy(j) )
        erp(x, y) = E(n-1, m-1)                                                                    (no square root at the end)

    Every cell is the min of three sums, and each sum has fixed operands.  min is exact and the additions are commutative, so
    any evaluation order gives the same bits: the value equals the sequential recurrence bit for bit (csrc/seqdp.hip).  dist is
    symmetric bit for bit, so erp(x, y) == erp(y, x) exactly.  There is no window: a banded ERP loses the triangle inequality,
    which is the reason to have it.  ERP tolerates local time shifts as DTW does, takes series of different lengths, and is a
    metric, because a gap is charged against the fixed gap point and not by repeating a neighbour: is_metric=True is its
    intended setting.

    Limits: dim 1 .. 4; 1 .. 2048 values at dim 1, 1 .. 1024 points at dim 2, 3 and 4; finite values, finite gap; one dim for a
    data set and its queries."""

    name = "erp"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, gap=0.0):
        if isinstance(gap, (bool, np.bool_)) or not isinstance(gap, (int, float, np.integer, np.floating)) or not np.isfinite(gap):
            raise ValueError("erp: gap must be a finite real number")
        self.gap = float(gap)

    def bind(self, engine, X):
        values, offs, lens, dim = pack_erp_series(X)
        engine.set_erp_series(values, offs, lens, dim, self.gap)


def _real_parameter(metric, name, value, low, strict):
    """MSM's, TWE's, EDR's and LCSS's parameters: a finite real number above `low` (strict) or not below it."""
    ok = not isinstance(value, (bool, np.bool_)) and isinstance(value, (int, float, np.integer, np.floating)) and np.isfinite(value)
    if not ok or (value <= low if strict else value < low):
        raise ValueError("%s: %s must be a finite real number %s %g" % (metric, name, ">" if strict else ">=", low))
    return float(value)


MSM_MAX_LENGTH = 2048


def pack_msm_series(X):
    """Univariate series -> (values float32 or float64, offs int64, lens int32): what pack_series takes and returns, refused as
    "msm: series <index> ..." -- an empty series, a series longer than MSM_MAX_LENGTH, a series that is not one-dimensional, a
    dtype that is not real, a value that is not finite."""
    return _pack_points(X, "msm", "series", 1, lambda dim: MSM_MAX_LENGTH, plural="series", univariate=True)[:3]


class MSM(DeviceMetric):
    """Move-Split-Merge (Stefan, Athitsos & Das 2013) between univariate series (no counterpart in the reference).  A series is
    1 .. 2048 values.  All arithmetic is float64, every operation rounded on its own; float32 input widens exactly.  `c` is the
    cost of a split or merge, finite and > 0, default 1.0.  Indices are 0-based; x has n >= 1 values, y has m >= 1.

        M(-1, -1) = 0     M(i, -1) = M(-1, j) = +inf     the virtual previous values x[-1] and y[-1] are 0.0
        C(v, a, b) = c                              if a <= v <= b or a >= v >= b
                   = c + min(|v - a|, |v - b|)      otherwise
        M(i, j) = min( M(i-1, j-1) + |x[i] - y[j]|,   M(i-1, j) + C(x[i], x[i-1], y[j]),   M(i, j-1) + C(y[j], x[i], y[j-1]) )
        msm(x, y) = M(n-1, m-1)

    The virtual values only ever meet +inf: this is the textbook form -- M(0, 0) = |x[0] - y[0]|, a first row and column of running
    sums of C -- bit for bit.  Every cell is the min of three sums of fixed operands, so the value equals the sequential
    recurrence bit for bit (csrc/seqdp.hip); C is symmetric in (a, b), so msm(x, y) == msm(y, x) exactly.  A move costs what it
    moves, a split or merge costs c: MSM is a metric and, unlike ERP, invariant under translation: is_metric=True is its intended
    setting.  There is no window: a banded MSM loses the triangle inequality.

    Limits: univariate series of 1 .. 2048 finite values; finite c > 0."""

    name = "msm"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, c=1.0):
        self.c = _real_parameter("msm", "c", c, 0.0, True)

    def bind(self, engine, X):
        engine.set_msm_series(*pack_msm_series(X), c=self.c)


TWE_MAX_DIM = 4


def twe_max_length(dim):
    """The longest series the kernel takes at `dim` coordinates per point: ERP's limits, 2048 values at dim 1 and 1024 points at
    dim 2, 3 and 4 (every shape of the kernel builds without scratch memory there)."""
    return erp_max_length(dim)


def pack_twe_series(X):
    """Series -> (values float32 or float64 [points * dim], offs int64, lens int32, dim): what pack_erp_series takes and returns,
    refused as "twe: series <index> ..." with twe_max_length(dim) as the length limit."""
    return _pack_points(X, "twe", "series", TWE_MAX_DIM, twe_max_length, plural="series")


class TWE(DeviceMetric):
    """Time warp edit distance (Marteau 2009) between series with uniform timestamps (no counterpart in the reference).  A series
    is 1 .. L points of `dim` coordinates, dim in 1 .. 4; point i has time i + 1.  All arithmetic is float64, every operation
    rounded on its own; float32 input widens exactly.  `nu` is the stiffness (default 0.001) and `lam` the penalty of a delete
    (default 1.0), both finite and >= 0.  dist is ERP's dist.  nl = nu + lam and nu2 = 2.0 * nu are formed once.

        T(-1, -1) = 0     T(i, -1) = T(-1, j) = +inf     the virtual previous points x[-1] and y[-1] are the origin
        dx(i) = dist(x[i], x[i-1]) + nl        dy(j) = dist(y[j], y[j-1]) + nl
        T(i, j) = min( T(i-1, j-1) + ((dist(x[i], y[j]) + dist(x[i-1], y[j-1])) + nu2 * (double)|i - j|),
                       T(i-1, j) + dx(i),   T(i, j-1) + dy(j) )
        twe(x, y) = T(n-1, m-1)

    This is Marteau's recurrence in its common implementation: zero-padded series, DP[0, 0] = 0 and +inf on the rest of row 0 and
    column 0.  Every cell is the min of three sums of fixed operands, so the value equals the sequential recurrence bit for bit
    (csrc/seqdp.hip); dist and |i - j| are symmetric, so twe(x, y) == twe(y, x) exactly.  TWE is a metric for every nu >= 0 and
    lam >= 0 (with nu = 0 it ignores the timestamps): is_metric=True is its intended setting.  There is no window: a banded TWE
    loses the triangle inequality.  Explicit timestamps are out of scope.

    Limits: dim 1 .. 4; 1 .. twe_max_length(dim) points (2048 values at dim 1, 1024 points at dim 2, 3 and 4); finite values;
    finite nu >= 0 and lam >= 0; one dim for a data set and its queries."""

    name = "twe"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, nu=0.001, lam=1.0):
        self.nu = _real_parameter("twe", "nu", nu, 0.0, False)
        self.lam = _real_parameter("twe", "lam", lam, 0.0, False)

    def bind(self, engine, X):
        values, offs, lens, dim = pack_twe_series(X)
        engine.set_twe_series(values, offs, lens, dim, self.nu, self.lam)


WED_MAX_ALPHABET = 128
WED_MAX_LENGTH = 2048


def _wed_symbols(alphabet, name="weighted_levenshtein"):
    """The alphabet of a WeightedLevenshtein, an AffineGap or an OSA as a list of one-character strings; its order gives the dense codes."""
    symbols = list(alphabet)
    for a, ch in enumerate(symbols):
        if not isinstance(ch, str) or len(ch) != 1:
            raise ValueError("%s: alphabet entry %d is %r, not a one-character string" % (name, a, ch))
    if not 1 <= len(symbols) <= WED_MAX_ALPHABET:
        raise ValueError("%s: the alphabet has %d symbols; 1 .. %d are supported" % (name, len(symbols), WED_MAX_ALPHABET))
    first = {}
    for a, ch in enumerate(symbols):
        if ch in first:
            raise ValueError("%s: alphabet entries %d and %d are both %r; the symbols are distinct" % (name, first[ch], a, ch))
        first[ch] = a
    return symbols


def pack_coded_strings(X, alphabet, name="weighted_levenshtein", limit=WED_MAX_LENGTH):
    """Python strings -> (codes uint8, offs int64, lens int32) over a GIVEN alphabet (a str or a sequence of one-character strings,
    1 .. 128 distinct symbols): symbol alphabet[a] becomes code a.  A string may be empty.  Refused here, on the host, before anything
    is uploaded, as "weighted_levenshtein: string <index> ...": a member that is not a str, a string of more than WED_MAX_LENGTH
    symbols, a symbol outside the alphabet (the message says which).  name, limit: another metric's name in the messages and its
    longest string (AffineGap's, OSA's)."""
    symbols = _wed_symbols(alphabet, name)
    strings = list(X)
    if not strings:
        raise ValueError("%s: no strings" % name)
    for s, x in enumerate(strings):
        if not isinstance(x, str):
            raise ValueError("%s: string %d is a %s, not a str" % (name, s, type(x).__name__))
    lens = np.fromiter((len(x) for x in strings), dtype=np.int64, count=len(strings))
    if lens.max() > limit:
        s = int(np.argmax(lens > limit))
        raise ValueError("%s: string %d has %d symbols; at most %d are supported" % (name, s, int(lens[s]), limit))
    raw = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    points = np.array([ord(ch) for ch in symbols], dtype=np.uint32)
    order = np.argsort(points)
    at = np.minimum(np.searchsorted(points[order], raw), len(symbols) - 1)
    bad = points[order][at] != raw
    if bad.any():
        k = int(np.argmax(bad))
        s = int(np.searchsorted(np.cumsum(lens), k, side="right"))
        raise ValueError("%s: string %d holds the symbol %r, which is not in the alphabet" % (name, s, chr(int(raw[k]))))
    codes = order[at].astype(np.uint8)
    offs = np.zeros(len(strings), dtype=np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    return codes, offs, lens.astype(np.int32)


def _string_costs(name, word, A, substitution, gap):
    """The checked cost arguments of a string metric `name` over A symbols -> (S float64 [A, A], g float64 [A]); `word` is what the
    per-symbol gap costs are called ("indel", "extend").  S: finite, >= 0, zero diagonal, symmetric bit for bit; g: a scalar or
    [A], finite, >= 0.  A violation raises ValueError("<name>: ..."), naming the offending entry."""
    try:
        S = np.array(substitution, dtype=np.float64)
        g = np.array(gap, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: substitution and %s must be arrays of real numbers" % (name, word)) from None
    if S.shape != (A, A):
        raise ValueError("%s: substitution has shape %s; the alphabet of %d symbols needs (%d, %d)" % (name, S.shape, A, A, A))
    if g.ndim == 0:
        g = np.full(A, float(g))
    if g.shape != (A,):
        raise ValueError("%s: %s has shape %s; a scalar or (%d,) for this alphabet" % (name, word, g.shape, A))
    bad = np.argwhere(~(np.isfinite(S) & (S >= 0.0)))
    if len(bad):
        a, b = map(int, bad[0])
        raise ValueError("%s: substitution[%d][%d] = %r is not a finite cost >= 0" % (name, a, b, float(S[a, b])))
    bad = np.flatnonzero(~(np.isfinite(g) & (g >= 0.0)))
    if len(bad):
        raise ValueError("%s: %s[%d] = %r is not a finite cost >= 0" % (name, word, int(bad[0]), float(g[bad[0]])))
    S, g = S + 0.0, g + 0.0   # (-0.0 -> 0.0)
    bad = np.flatnonzero(np.diag(S) != 0.0)
    if len(bad):
        a = int(bad[0])
        raise ValueError("%s: substitution[%d][%d] = %r; the diagonal is 0" % (name, a, a, float(S[a, a])))
    bad = np.argwhere(S != S.T)
    if len(bad):
        a, b = map(int, bad[0])
        raise ValueError("%s: substitution[%d][%d] = %r but substitution[%d][%d] = %r; the table is symmetric bit for bit"
                         % (name, a, b, float(S[a, b]), b, a, float(S[b, a])))
    return np.ascontiguousarray(S), np.ascontiguousarray(g)


def _string_costs_violation(S, g, sym, word):
    """WeightedLevenshtein.metric_violation's conditions on a substitution table S and per-symbol gap costs g called `word`."""
    A = len(sym)
    bad = np.argwhere((S <= 0.0) & ~np.eye(A, dtype=bool))
    if len(bad):
        a, b = map(int, bad[0])
        return "substitution[%d][%d] = 0 between the distinct symbols %r and %r" % (a, b, sym[a], sym[b])
    bad = np.flatnonzero(g <= 0.0)
    if len(bad):
        return "%s[%d] = 0 for the symbol %r" % (word, int(bad[0]), sym[int(bad[0])])
    bad = np.argwhere(S > g[:, None] + g[None, :])
    if len(bad):
        a, b = map(int, bad[0])
        return "substitution[%d][%d] = %r > %s[%d] + %s[%d] = %r" % (a, b, float(S[a, b]), word, a, word, b, float(g[a] + g[b]))
    bad = np.argwhere(g[:, None] > S + g[None, :])
    if len(bad):
        a, b = map(int, bad[0])
        return "%s[%d] = %r > substitution[%d][%d] + %s[%d] = %r" % (word, a, float(g[a]), a, b, word, b, float(S[a, b] + g[b]))
    for c in range(A):
        bad = np.argwhere(S > S[:, c, None] + S[None, c, :])
        if len(bad):
            a, b = map(int, bad[0])
            return ("substitution[%d][%d] = %r > substitution[%d][%d] + substitution[%d][%d] = %r"
                    % (a, b, float(S[a, b]), a, c, c, b, float(S[a, c] + S[c, b])))
    return None


class WeightedLevenshtein(DeviceMetric):
    """Weighted Levenshtein distance between strings: the edit distance under a substitution table and per-symbol insert / delete
    costs (no counterpart in the reference, which answers every cost model but unit costs with a user-supplied host function).

    An alphabet of A distinct symbols, 1 <= A <= 128.  S is a float64 [A, A] substitution table, g a float64 [A] insert / delete
    cost per symbol.  x_i and y_j are the symbols' codes, their positions in the alphabet.

        E(-1,-1) = 0      E(i,-1) = E(i-1,-1) + g[x_i]      E(-1,j) = E(-1,j-1) + g[y_j]      (left to right, one addition per step)
        E(i,j)   = min( E(i-1,j-1) + S[x_i][y_j],   E(i-1,j) + g[x_i],   E(i,j-1) + g[y_j] )
        wed(x,y) = E(n-1, m-1)                       wed(x, "") = E(n-1,-1)       wed("", "") = 0.0

    All arithmetic is float64.  Every cell is the min of three sums with fixed operands, so any evaluation order gives the same
    bits: the value equals the sequential double loop bit for bit (csrc/wed.hip).  S is required to be symmetric bit for bit; the
    transposed matrix then has the same cells, so wed(x, y) == wed(y, x) exactly.

    alphabet: a str or a sequence of one-character strings, 1 .. 128 distinct symbols; its order gives the dense codes.
    substitution: array-like [A, A]; finite, >= 0, zero diagonal, S == S.T exactly.
    indel: a scalar or array-like [A]; finite, >= 0.
    A violation raises ValueError("weighted_levenshtein: ...") here, naming the offending entry.

    Members are Python str of 0 .. 2048 symbols; empty strings are legal.  Refused on the host, before anything is uploaded, as
    "weighted_levenshtein: string <index> ...": a symbol outside the alphabet, more than 2048 symbols, a member that is not a str.

    Whether the value is a metric depends on the costs: call metric_violation() and pass is_metric=True to Annchor when it
    returns None, is_metric=False otherwise.  Annchor does not consult it.

    Affine gaps -- a run of k symbols against a gap costs open + the sum of their costs -- are AffineGap's, below; swaps of two
    adjacent symbols are OSA's.

    Out of scope: more than 128 symbols, longer strings, asymmetric tables or separate insert and delete costs, local alignment,
    normalised distances, float32 costs, a band."""

    name = "weighted_levenshtein"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, alphabet, substitution, indel=1.0):
        self.symbols = _wed_symbols(alphabet)
        self.substitution, self.indel = _string_costs("weighted_levenshtein", "indel", len(self.symbols), substitution, indel)

    @classmethod
    def unit(cls, alphabet):
        """Off-diagonal substitutions 1, indel 1: the values equal Levenshtein's, as floats."""
        A = len(_wed_symbols(alphabet))
        return cls(alphabet, 1.0 - np.eye(A), 1.0)

    def metric_violation(self):
        """None when the costs make the value a metric, else a short string naming the first violation.  The conditions, over the
        A symbols plus the gap as an (A+1)-th point with d(a, gap) = g[a]: off-diagonal S > 0; g > 0; S[a][b] <= g[a] + g[b];
        g[a] <= S[a][b] + g[b]; S[a][b] <= S[a][c] + S[c][b].  Under these the alignment recurrence is the true edit distance
        (Wagner & Fischer 1974), which is a metric.  Host-only, O(A^3)."""
        return _string_costs_violation(self.substitution, self.indel, self.symbols, "indel")

    def bind(self, engine, X):
        engine.set_coded_strings(*pack_coded_strings(X, self.symbols), self.substitution, self.indel)


AFFINE_MAX_LENGTH = 1024


class AffineGap(DeviceMetric):
    """Alignment distance between strings under affine gap costs: WeightedLevenshtein's substitution table, and a run of k symbols
    against a gap costs open + the sum of their extension costs instead of k independent indels -- what aligners of protein, DNA
    and noisy text score (Gotoh's three-state recurrence; no counterpart in the reference).

    An alphabet of A distinct symbols, 1 <= A <= 128.  S is a float64 [A, A] substitution table, g a float64 [A] extension cost per
    symbol, o the cost of opening a gap.  x_i and y_j are the symbols' codes, their positions in the alphabet.

        H(-1,-1) = 0      P(-1,j) = +inf      Q(i,-1) = +inf      P(-1,-1) = Q(-1,-1) = +inf
        P(i,j) = min( P(i-1,j), H(i-1,j) + o ) + g[x_i]                     (x_i against a gap)
        Q(i,j) = min( Q(i,j-1), H(i,j-1) + o ) + g[y_j]                     (y_j against a gap)
        H(i,j) = min( H(i-1,j-1) + S[x_i][y_j],   P(i,j),   Q(i,j) )
        affine(x,y) = H(n-1, m-1)      affine(x, "") = P(n-1,-1) = ((o + g[x_0]) + g[x_1]) + ...      affine("", "") = 0.0

    All arithmetic is float64.  Every cell is a min of sums with fixed operands, so any evaluation order gives the same bits: the
    value equals the sequential loop bit for bit (csrc/wed.hip, k_affine).  The transposed matrix swaps P and Q and holds the same
    H, so affine(x, y) == affine(y, x) exactly.  With open = 0.0 the value is WeightedLevenshtein(alphabet, substitution, extend)'s
    bit for bit.

    alphabet, substitution: as WeightedLevenshtein takes them.  extend: a scalar or array-like [A]; finite, >= 0.  open: a real
    scalar; finite, >= 0.  A violation raises ValueError("affine_gap: ...") here, naming the offending entry.

    Members are Python str of 0 .. 1024 symbols; empty strings are legal.  Refused on the host, before anything is uploaded, as
    "affine_gap: string <index> ...": a symbol outside the alphabet, more than 1024 symbols, a member that is not a str.

    Whether the value is a metric depends on the costs, as for WeightedLevenshtein: call metric_violation().

    Out of scope: what WeightedLevenshtein leaves out, strings beyond 1024 symbols (the kernel's registers), separate opening
    costs per symbol, other gap functions (logarithmic, piecewise linear)."""

    name = "affine_gap"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, alphabet, substitution, extend=1.0, open=0.0):
        self.symbols = _wed_symbols(alphabet, "affine_gap")
        self.substitution, self.extend = _string_costs("affine_gap", "extend", len(self.symbols), substitution, extend)
        try:
            o = np.array(open, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("affine_gap: open must be a real number") from None
        if o.ndim != 0:
            raise ValueError("affine_gap: open has shape %s; a scalar" % (o.shape,))
        if not (np.isfinite(o) and o >= 0.0):
            raise ValueError("affine_gap: open = %r is not a finite cost >= 0" % float(o))
        self.open = float(o) + 0.0   # (-0.0 -> 0.0)

    def metric_violation(self):
        """None when the costs make the value a metric, else a short string naming the first violation: WeightedLevenshtein's five
        conditions on S and g (`extend` in the place of `indel`).  With open >= 0 they are sufficient: the gap function
        open + sum of g is subadditive, and alignment distance under a subadditive gap function and metric symbol costs is a
        metric (Waterman, Smith & Beyer 1976).  Host-only, O(A^3)."""
        return _string_costs_violation(self.substitution, self.extend, self.symbols, "extend")

    def bind(self, engine, X):
        packed = pack_coded_strings(X, self.symbols, "affine_gap", AFFINE_MAX_LENGTH)   # (the host's refusals come first)
        engine.set_coded_strings_affine(*packed, self.substitution, self.extend, self.open)


OSA_MAX_LENGTH = 1024


class OSA(DeviceMetric):
    """Optimal string alignment: WeightedLevenshtein's edit distance with a fourth edit, the swap of two adjacent symbols at the
    cost `transpose` -- the fourth of Damerau's typo classes, for typed names, OCR output and keyboard input (no counterpart in
    the reference).  This is the RESTRICTED form: no substring is edited twice.  It is NOT the unrestricted Damerau-Levenshtein
    distance, whose cells read arbitrarily far back: osa("ca", "abc") = 3 at unit costs, where Damerau-Levenshtein gives 2.

    An alphabet of A distinct symbols, 1 <= A <= 128.  S is a float64 [A, A] substitution table, g a float64 [A] insert / delete
    cost per symbol, T the cost of a transposition.  x_i and y_j are the symbols' codes, their positions in the alphabet.

        E(-1,-1) = 0      E(i,-1) = E(i-1,-1) + g[x_i]      E(-1,j) = E(-1,j-1) + g[y_j]
        E(i,j)   = min( E(i-1,j-1) + S[x_i][y_j],   E(i-1,j) + g[x_i],   E(i,j-1) + g[y_j],
                        E(i-2,j-2) + T   if i >= 1 and j >= 1 and x_i == y_{j-1} and x_{i-1} == y_j )
        osa(x,y) = E(n-1, m-1)      osa(x, "") = E(n-1,-1)      osa("", "") = 0.0

    Row -1 and column -1 are legal sources of the fourth term: osa("ab", "ba") = T when that is the cheapest.  All arithmetic is
    float64.  Every cell is a min of sums with fixed operands, so any evaluation order gives the same bits: the value equals the
    sequential double loop bit for bit (csrc/wed.hip, k_osa).  The condition of the fourth term is symmetric in the two strings
    and S is symmetric, so osa(x, y) == osa(y, x) exactly.  With transpose = +inf the value is WeightedLevenshtein(alphabet,
    substitution, indel)'s bit for bit.

    alphabet, substitution, indel: as WeightedLevenshtein takes them.  transpose: a real scalar >= 0; +inf is allowed and means
    "no transpositions".  A violation raises ValueError("osa: ...") here, naming the offending entry.

    Members are Python str of 0 .. 1024 symbols; empty strings are legal.  Refused on the host, before anything is uploaded, as
    "osa: string <index> ...": a symbol outside the alphabet, more than 1024 symbols, a member that is not a str.

    OSA is NOT a metric, whatever the costs: at unit costs osa("ca", "abc") = 3 > osa("ca", "ac") + osa("ac", "abc") = 2.  Fit
    it with is_metric=False, as DTW, EDR and LCSS.  metric_violation() says so; Annchor does not consult it.

    Out of scope: what WeightedLevenshtein leaves out, strings beyond 1024 symbols (the kernel's registers), the unrestricted
    Damerau-Levenshtein distance, per-pair transposition costs."""

    name = "osa"
    ragged = True   # members may differ in length: a data set and its queries are concatenated as lists

    def __init__(self, alphabet, substitution, indel=1.0, transpose=1.0):
        self.symbols = _wed_symbols(alphabet, "osa")
        self.substitution, self.indel = _string_costs("osa", "indel", len(self.symbols), substitution, indel)
        try:
            t = np.array(transpose, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("osa: transpose must be a real number") from None
        if t.ndim != 0:
            raise ValueError("osa: transpose has shape %s; a scalar" % (t.shape,))
        if not t >= 0.0:   # (NaN fails too; +inf passes)
            raise ValueError("osa: transpose = %r is not a cost >= 0 (inf: no transpositions)" % float(t))
        self.transpose = float(t) + 0.0   # (-0.0 -> 0.0)

    @classmethod
    def unit(cls, alphabet):
        """Off-diagonal substitutions 1, indel 1, transpose 1: the unit-cost OSA distance, as floats."""
        A = len(_wed_symbols(alphabet, "osa"))
        return cls(alphabet, 1.0 - np.eye(A), 1.0, 1.0)

    def metric_violation(self):
        """None when the costs make the value a metric, else a short string naming the first violation: WeightedLevenshtein's
        finding on S and g if there is one; else None when transpose is +inf (the value then is WeightedLevenshtein's); else
        the counterexample that holds under unit costs and has its like under any finite transpose -- a transposed pair cannot
        be edited again, so the way through the middle string is cheaper.  Host-only, O(A^3)."""
        found = _string_costs_violation(self.substitution, self.indel, self.symbols, "indel")
        if found is not None or np.isinf(self.transpose):
            return found
        return ('a finite transpose breaks the triangle inequality: at unit costs osa("ca", "abc") = 3 > '
                'osa("ca", "ac") + osa("ac", "abc") = 2')

    def bind(self, engine, X):
        packed = pack_coded_strings(X, self.symbols, "osa", OSA_MAX_LENGTH)   # (the host's refusals come first)
        engine.set_coded_strings_osa(*packed, self.substitution, self.indel, self.transpose)


HAUSDORFF_MAX_DIM = 4
HAUSDORFF_MAX_POINTS = 4096


def pack_point_sets(X):
    """Point sets -> (values float32 or float64 [points * dim], offs int64, lens int32, dim); offs and lens count points.

    X is what pack_curves takes: a sequence of sets -- each a 2-D array [len, dim], or a 1-D array (a set of dim 1) -- or a
    3-D array [nx, len, dim] (nx sets of equal size), or a 2-D array [nx, len] (nx univariate rows).  float32 stays float32
    when every set is float32 (the kernel widens it exactly); anything else becomes float64.  Refused here, on the host, before
    anything is uploaded and with the set's index in the message: sets of different dim, a dim beyond HAUSDORFF_MAX_DIM, an
    empty set, a set of more than HAUSDORFF_MAX_POINTS points, a dtype that is not real, a value that is not finite."""
    return _pack_points(X, "hausdorff", "set", HAUSDORFF_MAX_DIM, lambda dim: HAUSDORFF_MAX_POINTS)


class Hausdorff(DeviceMetric):
    """Hausdorff distance between point sets (no counterpart in the reference).  A point set is 1 .. 4096 points of `dim`
    coordinates, with `dim` in 1 .. 4.  All arithmetic is float64.  float32 input widens exactly.

        c(i, j)  = sum over k = 0 .. dim-1, in that order, of t_k * t_k,   t_k = x[i][k] - y[j][k]
                   (every subtraction, product and addition rounded on its own: -ffp-contract=off, never an fma;
                    the sum starts from the k = 0 product, not from 0.0 + ...)
        h(x, y)  = max over i of ( min over j of c(i, j) )          -- directed, x to y
        hausdorff(x, y) = sqrt( max( h(x, y), h(y, x) ) ), correctly rounded

    (x - y)^2 == (y - x)^2 exactly and the order of k is fixed, so c(j, i) computed with the roles swapped has the same bits
    as c(i, j).  min and max are exact and associative, so any evaluation order gives the same bits (csrc/hausdorff.hip), and
    hausdorff(x, y) equals hausdorff(y, x) bit for bit.  A duplicated point changes nothing.  The result is a metric on sets;
    on the stored arrays it is a pseudo-metric, because a permuted or duplicated copy is at distance 0.  is_metric=True is
    the intended setting.

    Limits: dim 1 .. 4; 1 .. 4096 points; finite values; one dim for a data set and its queries."""

    name = "hausdorff"
    ragged = True   # members may differ in size: a data set and its queries are concatenated as lists

    def bind(self, engine, X):
        engine.set_point_sets(*pack_point_sets(X))


EMD_MAX_DIM = 4
EMD_MAX_POINTS = 128


def pack_clouds(X):
    """Point clouds -> (values float32 or float64 [points * dim], offs int64, lens int32, dim); offs and lens count points.

    X is what pack_curves takes: a sequence of clouds -- each a 2-D array [len, dim], or a 1-D array (a cloud of dim 1) -- or a
    3-D array [nx, len, dim] (nx clouds of equal size), or a 2-D array [nx, len] (nx univariate rows).  float32 stays float32
    when every cloud is float32 (the kernel widens it exactly); anything else becomes float64.  Refused here, on the host, before
    anything is uploaded and with the cloud's index in the message: clouds of different dim, a dim beyond EMD_MAX_DIM, an empty
    cloud, a cloud of more than EMD_MAX_POINTS points, a dtype that is not real, a value that is not finite."""
    return _pack_points(X, "emd", "cloud", EMD_MAX_DIM, lambda dim: EMD_MAX_POINTS)


class PointEMD(DeviceMetric):
    """Earth mover's distance (Wasserstein-1) between point clouds with uniform masses (no counterpart in the reference: its
    wasserstein needs one bin space and one cost matrix for the whole data set).  A cloud is 1 .. 128 points of `dim`
    coordinates, with `dim` in 1 .. 4.  All arithmetic is float64.  float32 input widens exactly.

        c(i, j)   dim 1:   |x[i][0] - y[j][0]|
                  dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = x[i][k] - y[j][k]
                  (every operation rounded on its own, never an fma, correctly rounded sqrt: ERP's `dist`, the same bits)
        emd(x, y) = min over F >= 0 of  sum_ij F_ij c(i, j)   with  sum_j F_ij = 1/n,  sum_i F_ij = 1/m

    The optimum is exact: the transportation simplex of the wide Wasserstein kernel (csrc/emd.hip), no Sinkhorn.  Scaled by
    n m / gcd(n, m) the masses are integers, so the flows are exact and the only rounding outside the costs is in the final
    sum(flow x cost) / total.  The value

      1. is a pure function of the two clouds: nothing of the bound data set enters a solve (the pricing tolerance comes from
         the pair's bounding box), so a pair gives the same bits inside a fit, in a query and as loose objects;
      2. is symmetric bit for bit: every pair is solved in one orientation -- the cloud with fewer points is the source side, at
         equal sizes the cloud whose first differing stored coordinate is smaller;
      3. is exactly 0.0 when the two clouds are equal as multisets of points (the same member, a permuted copy, duplicates
         included).

    It is a metric on uniform point measures -- finer than the Hausdorff distance, which sees only the worst point -- and a
    pseudo-metric on the stored arrays (a permuted copy is at distance 0): is_metric=True is its intended setting.  A solve that
    runs into its pivot cap gives NaN.

    Limits: dim 1 .. 4; 1 .. 128 points; finite values; one dim for a data set and its queries.  Out of scope: per-point
    weights, more than 128 points per cloud, more than 4 coordinates, other ground costs (squared, L1), partial or unbalanced
    transport, entropic approximations."""

    name = "emd"
    ragged = True   # members may differ in size: a data set and its queries are concatenated as lists

    def bind(self, engine, X):
        engine.set_clouds(*pack_clouds(X))


JACCARD_MAX_TOKENS = 65536    # distinct tokens in one member
JACCARD_MAX_BITS = 8192       # distinct tokens of a bound list (the universe U) the bits form takes
JACCARD_BITS_DENSITY = 128    # "auto": bits when U <= JACCARD_MAX_BITS and the mean member size is at least U / JACCARD_BITS_DENSITY


def _token_codes(X):
    """What both packers start from: the members of X as dense codes -> (codes int32, offs int64, lens int32, U).  Token members
    (integers) are recoded through the sorted distinct tokens of the whole list, so code order is token order and U their number;
    indicator members (bool rows of one length nbits) give their True positions and U = nbits.  Within a member the codes ascend
    strictly.  The refusals of the Jaccard docstring are made here."""
    if isinstance(X, np.ndarray) and X.ndim == 2 and X.dtype.kind in "biu":
        rows = list(X)
    elif isinstance(X, np.ndarray) and X.ndim > 2:
        raise ValueError("jaccard: set 0 has %d dimensions; a set is a 1-D array of integers or a 1-D bool array" % (X.ndim - 1))
    else:
        rows = []
        for x in X:
            if isinstance(x, (set, frozenset, list, tuple)):
                x = list(x)
                x = np.asarray(x) if x else np.zeros(0, dtype=np.int64)   # (an empty Python container holds no float)
            rows.append(np.asarray(x))
    if not rows:
        raise ValueError("jaccard: no sets")
    for s, x in enumerate(rows):
        if x.dtype.kind not in "biu":
            raise ValueError("jaccard: set %d has dtype %s; integer tokens or a bool indicator row" % (s, x.dtype))
        if x.ndim != 1:
            raise ValueError("jaccard: set %d has %d dimensions; a set is a 1-D array of integers or a 1-D bool array" % (s, x.ndim))
        if (x.dtype.kind == "b") != (rows[0].dtype.kind == "b"):
            raise ValueError("jaccard: set %d is %s and set 0 is %s; bool and integer members do not mix"
                             % (s, x.dtype, rows[0].dtype))
    if rows[0].dtype.kind == "b":
        nbits = len(rows[0])
        for s, x in enumerate(rows):
            if len(x) != nbits:
                raise ValueError("jaccard: set %d has %d bits, set 0 has %d; bool members share one length" % (s, len(x), nbits))
        members = [np.flatnonzero(x) for x in rows]
        U = nbits
    else:
        members = []
        for s, x in enumerate(rows):
            if x.dtype.kind == "u" and x.size and int(x.max()) > np.iinfo(np.int64).max:
                raise ValueError("jaccard: set %d holds a token beyond int64" % s)
            members.append(np.unique(x.astype(np.int64)))
        U = None
    lens = np.fromiter((len(m) for m in members), dtype=np.int64, count=len(members))
    if lens.max() > JACCARD_MAX_TOKENS:
        raise ValueError("jaccard: set %d has %d distinct tokens; at most %d are supported"
                         % (int(np.argmax(lens > JACCARD_MAX_TOKENS)), int(lens[lens > JACCARD_MAX_TOKENS][0]), JACCARD_MAX_TOKENS))
    flat = np.concatenate(members) if lens.sum() else np.zeros(0, dtype=np.int64)
    if U is None:
        universe = np.unique(flat)
        U = int(universe.size)
        flat = np.searchsorted(universe, flat)
    if U >= 2 ** 31:
        raise ValueError("jaccard: %d distinct tokens; fewer than 2^31 are supported" % U)
    offs = np.zeros(len(members), dtype=np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    return flat.astype(np.int32), offs, lens.astype(np.int32), U


def _bit_rows(codes, lens, U):
    nbits = max(int(U), 1)
    W = (-(-nbits // 32) + 3) // 4 * 4
    words = np.zeros((len(lens), W), dtype=np.uint32)   # (set word by word: a dense 0/1 matrix would take 32 times the rows)
    codes = codes.astype(np.int64)
    np.bitwise_or.at(words, (np.repeat(np.arange(len(lens)), lens), codes >> 5), np.uint32(1) << (codes & 31).astype(np.uint32))
    return words, nbits


def pack_token_sets(X):
    """Sets -> (codes int32, offs int64, lens int32, U): the tokens form.  The tokens of the whole list are recoded to dense codes
    0 .. U-1 through their sorted distinct values (for bool members U is their length and a code is a position); within a member
    the codes ascend strictly, duplicates removed.  A member may be empty.  Members and refusals: see Jaccard."""
    return _token_codes(X)


def pack_bitsets(X):
    """Sets -> (words uint32 [nx, W], nbits): the bits form.  nbits is the U of pack_token_sets (1 when every member is empty), W is
    ceil(nbits / 32) rounded up to a multiple of 4, bit p of a member -- its code p -- is bit p % 32 of word p // 32, and the
    padding bits are zero.  Any U is packed here; Jaccard binds this form up to JACCARD_MAX_BITS."""
    codes, _, lens, U = _token_codes(X)
    return _bit_rows(codes, lens, U)


class Jaccard(DeviceMetric):
    """Jaccard (Tanimoto) distance between finite sets of integers (no counterpart in the reference):

        i = |A n B|      u = |A| + |B| - i
        jaccard(A, B) = 0.0 if u == 0 (both empty),   (double)(u - i) / (double)u otherwise

    one IEEE float64 division of two exact integers -- (u - i) / u, not 1 - i / u, which differs in the last bit now and then; it
    is scipy.spatial.distance.jaccard on boolean vectors bit for bit.  jaccard(A, B) == jaccard(B, A) exactly; duplicates and order
    inside a member do not matter; jaccard(empty, empty) = 0 and jaccard(empty, A) = 1.  A true metric with values in [0, 1]:
    is_metric=True is its intended setting.  Disjoint sets are at exactly 1.0; on data whose pairs are mostly disjoint the
    stratified sampler can refuse with "Some sampler bins contain too few samples", as the reference's does on such distances.

    Members.  The dtype decides how a member is read, never its shape.  A token member is a 1-D array, list, tuple, set or
    frozenset of integers (any integer dtype, any int64 value, unsorted, repeats allowed, possibly empty).  An indicator member is
    a 1-D bool array: True at position p means token p is present.  A 2-D integer array [nx, L] is nx token members, a 2-D bool
    array [nx, nbits] nx indicator members.  Refused on the host, before anything is uploaded, as "jaccard: set <index> ...": a
    float or object dtype, a member of more than one dimension, bool and integer members in one data set, bool members of
    different lengths, more than JACCARD_MAX_TOKENS distinct tokens in one member.

    form: the device layout (csrc/jaccard.hip), never the value.  "tokens": ascending dense codes per member, looked up by binary
    search.  "bits": one bit row per member, popcounts of the "and" words; refused when the bound list has more than
    JACCARD_MAX_BITS distinct tokens (for bool members: bits).  "auto": bits when that fits and the mean member size is at least
    U / JACCARD_BITS_DENSITY, tokens otherwise.  A data set and its queries are bound as one list, so both get the same form."""

    name = "jaccard"
    ragged = True   # members may differ in size: a data set and its queries are concatenated as lists

    def __init__(self, form="auto"):
        if form not in ("auto", "bits", "tokens"):
            raise ValueError("jaccard: form must be 'auto', 'bits' or 'tokens', got %r" % (form,))
        self.form = form

    def _choose(self, lens, U):
        if self.form == "bits":
            if U > JACCARD_MAX_BITS:
                raise ValueError("jaccard: form='bits' takes at most %d distinct tokens, this list has %d" % (JACCARD_MAX_BITS, U))
            return "bits"
        if self.form == "auto" and U <= JACCARD_MAX_BITS and float(np.mean(lens)) * JACCARD_BITS_DENSITY >= U:
            return "bits"
        return "tokens"

    def form_for(self, X):
        """The layout bind() gives the list X: "bits" or "tokens"."""
        _, _, lens, U = _token_codes(X)
        return self._choose(lens, U)

    def bind(self, engine, X):
        codes, offs, lens, U = _token_codes(X)
        if self._choose(lens, U) == "bits":
            engine.set_bitsets(*_bit_rows(codes, lens, U))
        else:
            engine.set_token_sets(codes, offs, lens)


levenshtein = _Levenshtein()
jaccard = Jaccard()
emd = PointEMD()
dtw = DTW()
frechet = Frechet()
erp = ERP()
msm = MSM()
twe = TWE()
hausdorff = Hausdorff()
euclidean = _Euclidean()
cosine = _Cosine()
