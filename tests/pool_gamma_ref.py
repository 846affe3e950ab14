"""The pooling temperature (include/kprn.h "pooling temperature") restated in numpy float64 from path scores: pooled = log sum_q exp(s_q / gamma),
prob, the paths' normalised shares and d pooled / d s_q.  Uses nothing of the code under test.

The independent check of it (tests/test_pool_gamma_host.py, tests/test_gpu_pool_gamma.py): log sum exp(s / gamma) with s = W_out h + b_out is the UNMODIFIED
oracle's LogSumExp layer run on theta' = theta with out.weight and out.bias divided by gamma -- probabilities and loss are equal, every gradient outside the
head is equal, and d L / d theta_head = (1 / gamma) d L' / d theta'_head."""
import numpy as np


def pool(s, gamma):
    """one pair's scores s [cnt] (any float dtype; read as float64) -> dict(pooled, prob, shares [cnt], dS [cnt] = d pooled / d s)"""
    s = np.asarray(s, np.float64)
    t = (s - s.max()) / gamma
    e = np.exp(t)
    pooled = float(np.log(e.sum()) + s.max() / gamma)
    shares = e / e.sum()
    return dict(pooled=pooled, prob=1.0 / (1.0 + np.exp(-pooled)), shares=shares, dS=shares / gamma)


def pool_pairs(scores, offsets, gamma):
    """scores [N] of one class, offsets [B+1] -> pooled [B], prob [B], shares [N], dS [N]"""
    B = len(offsets) - 1
    pooled, prob = np.empty(B), np.empty(B)
    shares, dS = np.empty(len(scores)), np.empty(len(scores))
    for b in range(B):
        r = pool(scores[offsets[b]:offsets[b + 1]], gamma)
        pooled[b], prob[b] = r["pooled"], r["prob"]
        shares[offsets[b]:offsets[b + 1]], dS[offsets[b]:offsets[b + 1]] = r["shares"], r["dS"]
    return pooled, prob, shares, dS


def order(s):
    """the explanation's order over fp32 scores: score descending, index ascending among equals (-0 == +0), a NaN after every number, lower index first"""
    s = np.asarray(s, np.float32).astype(np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), np.where(nan, 0.0, -s), nan))


def scaled_head(theta, layout, gamma):
    """theta' of the identity: a copy of the flat parameters with out.weight and out.bias divided by gamma (layout: name -> (offset, shape))"""
    th = np.array(theta, np.float64, copy=True)
    for name in ("out.weight", "out.bias"):
        o, shp = layout[name]
        th[o:o + int(np.prod(shp))] /= gamma
    return th


def map_head_grads(grad_prime, layout, gamma):
    """d L / d theta from d L' / d theta': the head's entries times 1 / gamma, every other entry as it is"""
    g = np.array(grad_prime, np.float64, copy=True)
    for name in ("out.weight", "out.bias"):
        o, shp = layout[name]
        g[o:o + int(np.prod(shp))] /= gamma
    return g


def share_ratio_bar(gamma):
    """The spread a parity case needs: largest share : smallest share of a pair.  3 at gamma <= 1.  A gamma above 1 flattens the shares by construction --
    over the score span of about 1.7 these models give, gamma = 2 yields exp(1.7 / 2) = 2.3 at the very most ("about 2" is what the oracle shows), so 3 is
    out of reach however the inputs are drawn; there the bar is 1.5, a departure from uniform shares that is 2500 times the gradient bar of 2e-4 (and a
    gamma = 2 that was ignored would show in pooled itself, by several tenths)."""
    return 3.0 if gamma <= 1.0 else 1.5


def spread_conditions(path_scores, offsets, labels, gamma):
    """the two conditions a parity case has to meet on the reference's own numbers before anything is compared: -> (share of the pairs of at least two paths
    whose largest share is at least share_ratio_bar(gamma) x the smallest, largest |pooled| among the label-0 pairs)"""
    pooled, _, shares, _ = pool_pairs(path_scores, offsets, gamma)
    ratios = [shares[offsets[b]:offsets[b + 1]].max() / shares[offsets[b]:offsets[b + 1]].min() for b in range(len(offsets) - 1) if offsets[b + 1] - offsets[b] >= 2]
    neg = np.abs(pooled[np.asarray(labels) < 0.5])
    # (a batch of single-path pairs has no shares to spread: pooled = s / gamma there, which shows gamma by itself)
    return (float(np.mean(np.array(ratios) >= share_ratio_bar(gamma))) if ratios else 1.0), (float(neg.max()) if len(neg) else 0.0)


def labels_within_the_loss_bar(labels, pooled, limit=6.0):
    """labels with every label-0 pair whose |pooled| (the reference's) exceeds the limit turned into a positive: 1 - p of such a pair has lost in fp32 the
    digits the loss bar of 1e-5 needs, so the parity batches do not ask for its -log(1 - p)"""
    out = np.array(labels, np.float32, copy=True)
    out[(out < 0.5) & (np.abs(pooled) > limit)] = 1.0
    return out
