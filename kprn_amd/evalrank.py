"""Ranking evaluation chain after scoring, Python 3 restatement of
release/songPathRnn/eval/combine_result.py, resort.py and eval_score.py.
"""
import heapq
import math


def combine_result(entity_lines, result_lines):
    """combine_result.py:24-27: positional join -> "user \\t item \\t label \\t score"."""
    out = []
    for e, r in zip(entity_lines, result_lines):
        el = e.strip().split("\t")
        rl = r.strip().split("\t")
        out.append(el[1] + "\t" + el[2] + "\t" + rl[-1] + "\t" + rl[-2] + "\n")
    return out


def resort(combined_lines, user_ids):
    """resort.py:22-43: keep users in user_ids; sort by (int(user), -score); score re-printed via str(float)."""
    users = set(u.strip() for u in user_ids)
    items = []
    for line in combined_lines:
        ll = line.strip().split("\t")
        if ll[0] in users:
            items.append((int(ll[0]), ll[1], ll[2], float(ll[3])))
    items.sort(key=lambda x: (x[0], -x[-1]))
    return [str(i[0]) + "\t" + i[1] + "\t" + str(i[2]) + "\t" + str(i[3]) + "\n" for i in items]


def hit_ndcg(scores, k):
    """eval_score.py:20-46: the positive is index 0 among 1 + 100 candidates; heapq.nlargest keeps the first-seen
    element on ties, so the positive wins ties; sum(scores) == 0 -> (0, 0); ndcg = ln2 / ln(rank + 2)."""
    if sum(scores) == 0:
        return 0.0, 0.0
    top = heapq.nlargest(k, range(len(scores)), key=lambda i: scores[i])
    if 0 in top:
        rank = top.index(0)
        return 1.0, math.log(2) / math.log(rank + 2)
    return 0.0, 0.0


def eval_samples(score_of, samples, ks=range(1, 16)):
    """eval_score.py:97-129.  score_of: dict (user,item)->score; samples: iterable of (user, pos_item, [neg items]).
    A sample is skipped if the positive or any negative is unscored (:101-109)."""
    hits = {k: 0.0 for k in ks}
    ndcgs = {k: 0.0 for k in ks}
    n = 0
    for user, pos, negs in samples:
        keys = [(user, pos)] + [(user, x) for x in negs]
        if any(kv not in score_of for kv in keys):
            continue
        sc = [score_of[kv] for kv in keys]
        n += 1
        for k in ks:
            h, d = hit_ndcg(sc, k)
            hits[k] += h
            ndcgs[k] += d
    if n == 0:
        return {k: 0.0 for k in ks}, {k: 0.0 for k in ks}, 0
    return {k: hits[k] / n for k in ks}, {k: ndcgs[k] / n for k in ks}, n


def read_samples(lines):
    """eval_score.py:71-84: `user \\t pos_item \\t neg#neg#...` -> [(user, pos_item, [neg items])]"""
    out = []
    for line in lines:
        ll = line.strip().split("\t")
        if len(ll) < 3:
            continue
        out.append((ll[0], ll[1], [x for x in ll[2].split("#") if x != ""]))
    return out


def group_index(entity_lines, samples, user_ids=None):
    """What combine_result + the (user, item) dict + eval_samples do by string join, as arrays for the engine's ranking stage
    (Engine.rank_groups / _ffi.host_rank_groups): -> (members int64 [M], group_offsets int64 [G+1], n_used).

    The line number of every (user, item) of the positional entity file (a later line replaces an earlier one, as the dict does); one group per
    sample with the positive first (pos = 0); a sample with an unscored positive or negative is left out (eval_score.py:101-109); users outside
    user_ids are unscored (resort.py:22-30)."""
    import numpy as np
    users = None if user_ids is None else set(u.strip() for u in user_ids)
    line_of = {}
    for i, e in enumerate(entity_lines):
        el = e.strip().split("\t")
        if users is not None and el[1] not in users:
            continue
        line_of[(el[1], el[2])] = i
    members, offsets = [], [0]
    for user, pos, negs in samples:
        try:
            g = [line_of[(user, pos)]] + [line_of[(user, x)] for x in negs]
        except KeyError:
            continue
        members.extend(g)
        offsets.append(len(members))
    return np.asarray(members, np.int64), np.asarray(offsets, np.int64), len(offsets) - 1


def metrics_from_hist(hist, hist_len, ks=range(1, 16)):
    """hit@k / ndcg@k from the ranking stage's rank histogram (include/kprn.h "ranking"), in the shape eval_samples returns: (hits, ndcgs, n).
    n = every group that has a positive, zero groups included (they are misses).  An evaluation over scores that were never written (or lie outside
    the mode's range) is an error, not a number."""
    hist = [int(v) for v in hist]
    if len(hist) != hist_len + 4:
        raise ValueError("hist must have hist_len + 4 entries")
    if hist[hist_len + 3] != 0:
        raise ValueError("%d ranked scores were invalid (never written, NaN, or outside [0, 1])" % hist[hist_len + 3])
    ks = list(ks)
    if ks and max(ks) > hist_len:
        raise ValueError("k beyond the histogram's length")
    n = sum(hist[:hist_len + 2])
    if n == 0:
        return {k: 0.0 for k in ks}, {k: 0.0 for k in ks}, 0
    hits = {k: sum(hist[:k]) / n for k in ks}
    ndcgs = {k: sum(hist[r] * (math.log(2) / math.log(r + 2)) for r in range(k)) / n for k in ks}
    return hits, ndcgs, n


def format_metric_lines(hits, ndcgs, ks=range(1, 16)):
    """the two lines eval_score.py:158-159 writes"""
    return ("hit scores\t:" + "\t".join("%.5f" % hits[k] for k in ks) + "\n",
            "ndcg scores\t:" + "\t".join("%.5f" % ndcgs[k] for k in ks) + "\n")
