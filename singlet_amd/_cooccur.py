"""Marshalling of the co-occurrence calls (include/singlet_hip.h, "Co-occurrence by distance"), shared by Context and api: what
cannot be handed to the library is refused here; the library checks the content and names the offender."""
import numpy as np

from ._marshal import nhood_labels

COOCCUR_INFO = ("grid_mode", "W", "H", "bin_path", "lds_bytes", "workgroups", "flushes", "pairs")
MAX_INTERVALS = 64


def cooccur_coords(coords, who):
    """(c1, c2) contiguous float64 vectors from an n x 2 matrix or a pair of vectors."""
    if isinstance(coords, (tuple, list)) and len(coords) == 2 and np.ndim(coords[0]) == 1:
        c1, c2 = (np.asarray(v) for v in coords)
    else:
        xy = np.asarray(coords)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("%s: coords must be an n x 2 matrix or a pair of vectors, not %r" % (who, xy.shape))
        c1, c2 = xy[:, 0], xy[:, 1]
    if c1.ndim != 1 or c1.shape != c2.shape or c1.shape[0] < 1 or c1.dtype.kind not in "fiu" or c2.dtype.kind not in "fiu":
        raise ValueError("%s: coords must hold two numeric vectors of one length (at least one point)" % who)
    if c1.shape[0] >= 2**31:
        raise ValueError("%s: %d points: below 2^31 are taken" % (who, c1.shape[0]))
    return np.ascontiguousarray(c1, dtype=np.float64), np.ascontiguousarray(c2, dtype=np.float64)


def cooccur_thresholds(interval, who):
    """The thresholds r[0 .. T] as a contiguous float64 vector (their content is the library's to check)."""
    r = np.asarray(interval)
    if r.ndim != 1 or r.shape[0] < 1 or r.dtype.kind not in "fiu":
        raise ValueError("%s: interval must be a one-dimensional array of thresholds" % who)
    return np.ascontiguousarray(r, dtype=np.float64)


def cooccur_inputs(coords, labels, interval, n_classes, who):
    """(c1, c2, n, lab, K, r, T) of a library call."""
    c1, c2 = cooccur_coords(coords, who)
    lab, K = nhood_labels(labels, c1.shape[0], n_classes, who)
    r = cooccur_thresholds(interval, who)
    return c1, c2, int(c1.shape[0]), lab, K, r, int(r.shape[0]) - 1


def table_shape(K, T):
    """The buffer of a T x K x K table; outside the legal ranges the library refuses before it writes."""
    return max(min(T, MAX_INTERVALS), 1), max(min(K, 256), 1), max(min(K, 256), 1)


def abt(table, K, T):
    """The library's [t][b][a] buffer as a contiguous K x K x T array indexed [a, b, t]."""
    return np.ascontiguousarray(table[:T, :K, :K].transpose(2, 1, 0))


def tba(table):
    """A K x K x T array indexed [a, b, t] as the library's contiguous [t][b][a] buffer."""
    return np.ascontiguousarray(np.asarray(table).transpose(2, 1, 0))


def default_interval(c1, c2, count, who):
    """The library's own rule for a count of intervals: np.linspace(0, 0.5 * hypot(extent_x, extent_y), count + 1)."""
    if int(count) != count or not 1 <= count <= MAX_INTERVALS:
        raise ValueError("%s: interval = %r intervals: between 1 and %d are taken" % (who, count, MAX_INTERVALS))
    half = 0.5 * float(np.hypot(c1.max() - c1.min(), c2.max() - c2.min()))
    if not (np.isfinite(half) and half > 0):
        raise ValueError("%s: the points have no finite positive extent: give the thresholds" % who)
    return np.linspace(0.0, half, int(count) + 1)
