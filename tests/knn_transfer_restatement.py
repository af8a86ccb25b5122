"""The rules of the label / value transfer (include/singlet_hip.h, "Neighbour index and transfer") restated in numpy, without a
device.  Everything is FP64; every product, quotient and sum is its own rounding; every sum runs over the slots in rank order,
from +0.0.

For one query the slots i = 0 .. K - 1 are valid where idx_i >= 0; the padding (-1 / +Inf) follows the valid slots.
Weights: weighting 0: w_i = 1.  weighting 1 (Dudani 1976): with d_first, d_last the distances of the first and the last valid
slot, w_i = (d_last - d_i) / (d_last - d_first) when d_last is finite and d_last > d_first; otherwise every w_i = 1.
Labels: s_c = sum of w_i over the valid slots whose reference has label c; W = sum over the valid slots whose reference has any
label.  W > 0: scores[c] = s_c / W, pred = the class of the largest score (ties to the lowest class), best = that score;
otherwise all scores +0.0, pred -1, best +0.0.
Values: Wv = sum of w_i over all valid slots; values[f] = (sum over the valid slots of w_i * V[f, idx_i]) / Wv; without a valid
slot NaN.

The loops below run over the slots and are vectorised over the queries: every query's sums still receive their terms one at a
time in rank order, and a slot that does not take part adds nothing."""
import numpy as np

WEIGHTINGS = {"uniform": 0, "distance": 1}


def weights(idx, dist, weighting):
    """(w n_query x K, valid n_query x K) -- w is 1.0 where the slot is not valid (it is never used there)."""
    idx = np.asarray(idx)
    dist = np.asarray(dist, dtype=np.float64)
    nq, K = idx.shape
    valid = idx >= 0
    nv = valid.sum(axis=1)
    assert np.array_equal(valid, np.arange(K)[None, :] < nv[:, None]), "the padding follows the valid slots"
    w = np.ones((nq, K))
    if WEIGHTINGS.get(weighting, weighting) == 1 and nq:
        rows = np.arange(nq)
        d_first = dist[:, 0]
        d_last = dist[rows, np.maximum(nv - 1, 0)]
        with np.errstate(invalid="ignore"):
            by_distance = (nv > 0) & np.isfinite(d_last) & (d_last > d_first)
            num = d_last[:, None] - dist
            den = d_last - d_first
        with np.errstate(invalid="ignore", divide="ignore"):
            q = num / den[:, None]
        w = np.where(by_distance[:, None] & valid, q, 1.0)
    return w, valid


def transfer(idx, dist, labels=None, n_classes=0, V=None, weighting="distance"):
    """idx / dist n_query x K as a search returns them; labels int[n_ref] in [-1, n_classes); V n_values x n_ref.
    -> {"predicted" int32[n_query], "score" [n_query], "scores" n_query x n_classes, "values" n_query x n_values}; None for
    what has no annotation."""
    idx = np.asarray(idx)
    nq, K = idx.shape
    w, valid = weights(idx, dist, weighting)
    out = {"predicted": None, "score": None, "scores": None, "values": None}
    rows = np.arange(nq)
    if labels is not None:
        labels = np.asarray(labels)
        S = np.zeros((nq, int(n_classes)))
        W = np.zeros(nq)
        for t in range(K):
            lab = np.where(valid[:, t], labels[np.maximum(idx[:, t], 0)], -1)
            on = lab >= 0
            S[rows[on], lab[on]] = S[rows[on], lab[on]] + w[on, t]
            W[on] = W[on] + w[on, t]
        voted = W > 0
        scores = np.zeros_like(S)
        scores[voted] = S[voted] / W[voted, None]
        pred = np.full(nq, -1, dtype=np.int32)
        best = np.zeros(nq)
        for j in np.flatnonzero(voted):
            bc = 0
            for c in range(1, int(n_classes)):
                if scores[j, c] > scores[j, bc]:
                    bc = c
            pred[j], best[j] = bc, scores[j, bc]
        out.update(predicted=pred, score=best, scores=scores)
    if V is not None:
        V = np.asarray(V, dtype=np.float64)
        acc = np.zeros((nq, V.shape[0]))
        Wv = np.zeros(nq)
        for t in range(K):
            on = valid[:, t]
            acc[on] = acc[on] + w[on, t][:, None] * V[:, idx[on, t]].T
            Wv[on] = Wv[on] + w[on, t]
        with np.errstate(invalid="ignore", divide="ignore"):
            values = acc / Wv[:, None]
        values[~valid.any(axis=1)] = np.nan
        out["values"] = values
    return out
