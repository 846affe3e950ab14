"""Shared by tests/test_rank_targets_host.py, tests/test_gpu_rank_targets.py and tests/test_gpu_evaluate_graph.py: a numpy restatement of include/kprn.h
"ranking targets in groups of any size" that uses nothing of the code under test, and the shape list the host twin, the device kernel and the sanitizer
program are all run on.

The key is the formula of graph._rank_key restated (what "%.5f" prints, times 1e5, in mode 0; the fp32 value in mode 1), with validity as a sort key of its
own -- in mode 1 a valid -inf lies ABOVE an invalid NaN, which one -inf for both would not say.  The order is np.lexsort((index, -key, invalid)); places
are counted by comparison where n * nt is small and read off the sorted order where it is not (the two agree wherever both run: test_rank_targets_host)."""
import numpy as np

PRINTED, RAW = 0, 1
ZERO = -1
COMPARE_MAX = 1_000_000  # n * nt up to which places are counted by comparing every target with every member


def keys(scores, mode):
    """-> (valid bool [n], key float64 [n], 0 where invalid)"""
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore"):
        valid = (s >= 0) & (s <= 1) if mode == PRINTED else ~np.isnan(s)
    safe = np.where(valid, s, np.float32(0)).astype(np.float64)
    return valid, (np.rint(safe * 1e5) if mode == PRINTED else safe + 0.0)


def group_places(s, targets, mode, by_comparison=None):
    """one group's scores [n] and ascending target indices -> (places [nt] int64 with ZERO for zero samples, invalid members)"""
    n, t = len(s), np.asarray(targets, np.int64)
    valid, key = keys(s, mode)
    idx = np.arange(n)
    is_t = np.zeros(n, bool)
    is_t[t] = True
    if by_comparison is None:
        by_comparison = n * len(t) <= COMPARE_MAX
    if by_comparison:
        other = ~is_t
        vo, ko, io = valid[other], key[other], idx[other]
        places = np.zeros(len(t), np.int64)
        for q, i in enumerate(t):       # a non-target lies above target i: valid against invalid, else the larger key, else the smaller index
            above = (vo & ~valid[i]) | ((vo == valid[i]) & ((ko > key[i]) | ((ko == key[i]) & (io < i))))
            places[q] = above.sum()
    else:
        order = np.lexsort((idx, -key, ~valid))
        at = np.empty(n, np.int64)
        at[order] = idx
        targets_before = np.cumsum(is_t[order]) - is_t[order]
        places = at[t] - targets_before[at[t]]
    if mode == PRINTED:
        above_zero = valid & (key >= 1)
        if not above_zero[~is_t].any():
            places = np.where(above_zero[t], places, ZERO)
    return places, int((~valid).sum())


def reference(scores, group_offsets, target_offsets, targets, members=None, mode=PRINTED, hist_len=15):
    """-> (places int32 [NT], hist int64 [hist_len + 4])"""
    scores = np.asarray(scores, np.float32)
    places = np.zeros(int(target_offsets[-1]), np.int32)
    hist = np.zeros(hist_len + 4, np.int64)
    for g in range(len(group_offsets) - 1):
        a, b = int(group_offsets[g]), int(group_offsets[g + 1])
        lines = np.arange(a, b) if members is None else np.asarray(members[a:b], np.int64)
        ta, tb = int(target_offsets[g]), int(target_offsets[g + 1])
        p, inv = group_places(scores[lines], targets[ta:tb], mode)
        places[ta:tb] = p
        hist[hist_len + 3] += inv
        for v in p:
            hist[hist_len + 1 if v < 0 else min(int(v), hist_len)] += 1
    return places, hist


# ---- the shape list ------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 255, 256, 257, 4096, 4097, 8193, 70001)          # 70 001: past 65 536
TARGET_COUNTS = (0, 1, 2, 63, 64, 65, 1024, 1025, 2000, "all")   # 1025 and 2000: the second chunk of 1024 staged targets
TIE_POOL = np.array([0.5, 0.12345, 0.123454999, 0.123455001, 0.1234549, 0.1234551, 0.999995, 0.9999949, 0.0, 0.000004, 0.000006, 0.25, 0.75], np.float32)


def draw_scores(rng, n):
    """ties are the normal case: a third print 1.00000, the rest come from a small pool with values on both sides of a "%.5f" rounding boundary"""
    s = TIE_POOL[rng.randint(len(TIE_POOL), size=n)]
    s[rng.rand(n) < 1 / 3] = np.float32(0.999999)   # prints 1.00000, as 1.0 does
    s[rng.rand(n) < 0.1] = np.float32(1.0)
    return s


def draw_targets(rng, n, nt):
    """nt ascending indices that hold the first index, the last one and a pair of adjacent ones where nt allows"""
    want = [0, n - 1, n // 2, n // 2 + 1][:nt]
    pick = set(int(x) for x in want if 0 <= x < n)
    rest = [i for i in rng.permutation(n)[:nt + 4] if int(i) not in pick] if nt < n else []
    for i in rest:
        if len(pick) >= nt:
            break
        pick.add(int(i))
    return np.array(sorted(pick) if nt < n else range(n), np.int32)


def special_groups(mode):
    """[(scores, targets)]: the groups the rule has a sentence for"""
    f = lambda *v: np.array(v, np.float32)
    nan, inf = np.float32("nan"), np.float32("inf")
    out = [
        (np.zeros(300, np.float32), [0, 7, 299]),                                   # all zero: zero samples in mode 0
        (f(0, 0, 0.5, 0, 0.000004), [2]),                                           # only the target prints above zero
        (f(0, 0.000004, 0.5, 0, 0), [1, 2]),                                        # only ANOTHER target does: zero sample for 1, place 0 for 2
        (f(0.3, nan, 0.3, nan, 0.2, -0.0, 0.0), [1, 2, 5]),                         # NaN member, NaN target, -0.0
        (f(nan, nan, nan), [0, 2]),                                                 # nothing valid
        (f(1.5, -0.25, 0.5, 0.5), [1, 3]),                                          # outside [0, 1]: invalid in mode 0, ordinary in mode 1
    ]
    if mode == RAW:
        out += [(f(inf, -inf, nan, 0.0, -0.0, -inf, inf, 3e38, -3e38), [1, 4, 6]), (f(-inf, nan), [0]), (f(nan, -inf), [0, 1])]
    return out


def cases(mode, seed=7):
    """every size x every target count that fits, the special groups, and one block of scattered members with repeated lines, as ONE call:
    -> dict(scores, members (int64 [M]: every group goes through it), group_offsets, target_offsets, targets)"""
    rng = np.random.RandomState(seed + mode)
    scores, members, goff, toff, targets = [], [], [0], [0], []
    base = 0

    def add(s, t, lines=None):
        nonlocal base
        s = np.asarray(s, np.float32)
        scores.append(s)
        members.append(base + (np.arange(len(s)) if lines is None else lines))
        base += len(s)
        goff.append(goff[-1] + len(members[-1]))
        targets.append(np.asarray(t, np.int32))
        toff.append(toff[-1] + len(t))

    for n in SIZES:
        for nt in TARGET_COUNTS:
            nt = n if nt == "all" else nt
            if nt <= n:
                add(draw_scores(rng, n), draw_targets(rng, n, nt))
    for s, t in special_groups(mode):
        add(s, t)
    for n, nt in ((700, 5), (5000, 70)):                     # scattered: a group of n members over n // 2 lines, every line about twice, reversed runs
        lines = rng.randint(n // 2, size=n)
        lines[::3] = lines[::3][::-1]
        add(draw_scores(rng, n // 2), draw_targets(rng, n, nt), lines)
    return dict(scores=np.concatenate(scores), members=np.concatenate(members).astype(np.int64), group_offsets=np.array(goff, np.int64),
                target_offsets=np.array(toff, np.int64), targets=np.concatenate(targets).astype(np.int32))


def consecutive_cases(mode, seed=11):
    """members = NULL: consecutive board runs, a mixed call of 1, 257, 4097 and 70 001 members with 1, 64, 2000 and 3 targets, starting past line 0"""
    rng = np.random.RandomState(seed + mode)
    sizes, counts = (1, 257, 4097, 70001, 2), (1, 64, 2000, 3, 0)
    goff = np.concatenate([[5], 5 + np.cumsum(sizes)]).astype(np.int64)
    scores = draw_scores(rng, int(goff[-1]) + 3)
    tg = [draw_targets(rng, n, k) for n, k in zip(sizes, counts)]
    return dict(scores=scores, members=None, group_offsets=goff, target_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                targets=np.concatenate(tg).astype(np.int32))
