"""The pairwise loss (include/kprn.h "pairwise loss") restated in float64, for the tests of the host twin and of the kernel, and the pseudo-labels
that make the oracle's BCE backward carry a given dy.

The oracle's closed-form BCE gradient is (p - t) * inv_batch for ANY real t, so with t'_b = p_b - dy_b / inv_batch (p from the oracle's own forward)
Oracle.forward_backward / Oracle.train_step back-propagate exactly dy through the reducer and the network.  The loss they report is then meaningless
(a logarithm of whatever t' makes); the reference loss is `pairwise`'s.
"""
import numpy as np


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def pairwise(pooled, labels, group_offsets, inv_batch=0.0):
    """-> dict(loss, dy [B], n_terms, theta = y_i - y_j of every term in (group, i, j) order, s = the scale)"""
    y = np.asarray(pooled, np.float64).reshape(-1)
    pos = np.asarray(labels, np.float64).reshape(-1) > 0.5
    go = np.asarray(group_offsets, np.int64)
    dy = np.zeros_like(y)
    thetas, parts = [], []
    for g in range(len(go) - 1):
        lo, hi = int(go[g]), int(go[g + 1])
        ip = lo + np.nonzero(pos[lo:hi])[0]
        im = lo + np.nonzero(~pos[lo:hi])[0]
        if len(ip) == 0 or len(im) == 0:
            continue
        th = y[ip][:, None] - y[im][None, :]
        with np.errstate(over="ignore"):
            sig = 1.0 / (1.0 + np.exp(th))
        dy[ip] -= sig.sum(axis=1)
        dy[im] += sig.sum(axis=0)
        parts.append(float(softplus(-th).sum()))
        thetas.append(th.reshape(-1))
    theta = np.concatenate(thetas) if thetas else np.zeros(0)
    n_terms = int(theta.shape[0])
    s = float(inv_batch) if inv_batch > 0 else (1.0 / n_terms if n_terms else 0.0)
    return dict(loss=s * float(np.sum(parts)), dy=s * dy, n_terms=n_terms, theta=theta, s=s)


def pseudo_labels(probs, dy, inv_batch):
    """t' with (p - t') * inv_batch = dy"""
    return np.asarray(probs, np.float64) - np.asarray(dy, np.float64) / float(inv_batch)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
