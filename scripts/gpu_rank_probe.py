#!/usr/bin/env python3
"""What the ranking stage (include/kprn.h "ranking": score board, kprn_rank_groups, kprn_recommend_ragged) buys and costs.  One JSON object from one
process; every comparison is a warm-up and then three alternating repetitions per leg, timed with a device synchronise around each.

1. one user's 101 candidates (177 paths, 7 distinct counts: comparison 2 of gpu_ragged_probe.py), top-10: recommend_ragged against forward_ragged_host
   followed by the same rule on the host (host_rank_groups): us per user;
2. a test set of 1 500 users x 101 candidates and one of about `total_pairs` pairs, in bucket files, every user's candidates scattered over the buckets:
   (a) the text chain -- write_scores to a file, read back, combine_result, (user, item) dict, eval_samples; (b) score_batches + host_rank_groups;
   (c) rank_test_set.  Seconds per evaluation, and the ranking launch alone from the engine's profile;
3. the ranking kernels over the group size: 10 000 groups of 2 .. 4096 members of board_write data, ms per call (arguments up, launch, ranks + top-10 +
   histogram down) and per launch; above 256 members the launch with places by counting against the launch with the LDS sort (option rank_sort_min).

usage: gpu_rank_probe.py [total_pairs]"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kprn_amd import _ffi, evalrank, formats, scoring, synth  # noqa: E402
from kprn_amd.batcher import BatcherFileList  # noqa: E402

total_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
Vt, Ve, Vr, T = 6, 2851220, 9, 6
eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2, seed=1)
res = {"what": "ranking stage: one-call top-K, test-set evaluation by three routes, ranking kernels over group size", "T": T, "D": 64, "H": 64, "L": 2, "Ve": Ve}


def timed(fn):
    eng.sync()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    return time.perf_counter() - t0


def alternate(*legs, reps=3):
    for f in legs:
        f()   # warm-up: allocations, first-launch costs
    ts = [[] for _ in legs]
    for _ in range(reps):
        for t, f in zip(ts, legs):
            t.append(timed(f))
    return ts


def kernel_ms(fn):
    """milliseconds and launches of the ranking kernels inside fn(), from the engine's event profile"""
    eng.set_option("profile_filter", "rank_groups")
    eng.profile(True)
    eng.profile_reset()
    fn()
    got = eng.profile_get().get("rank_groups", (0.0, 0))
    eng.profile(False)
    eng.set_option("profile_filter", "")
    return round(got[0], 4), got[1]


# ---- 1: one user's candidates, the 10 best ---------------------------------------------------------------------------------------------
counts = synth.draw_num_paths(np.random.default_rng(7), 101)
cidx, _, _ = synth.make_ragged(101, T, Ve=Ve, seed=25, counts=counts)
REP = 200
one_group = np.array([0, 101], np.int64)
no_pos = np.array([-1], np.int32)
keep = {}


def engine_call():
    for _ in range(REP):
        keep["dev"] = eng.recommend_ragged(cidx, counts, [101], 10)


def host_route():
    for _ in range(REP):
        probs, _ = eng.forward_ragged_host(cidx, counts, 1)
        keep["host"] = _ffi.host_rank_groups(probs, one_group, pos=no_pos, K=10)


t_dev, t_host = alternate(engine_call, host_route)
assert np.array_equal(keep["dev"][0], keep["host"]["topk_idx"])
res["candidates"] = {"pairs": 101, "paths": int(counts.sum()), "K": 10, "recommend_ragged_us_per_user": [round(1e6 * x / REP, 1) for x in t_dev],
                     "forward_ragged_plus_host_rule_us_per_user": [round(1e6 * x / REP, 1) for x in t_host]}


# ---- 2: a test set, three routes ---------------------------------------------------------------------------------------------------------
def test_set(tag, buckets, cand):
    d = tempfile.mkdtemp(prefix="kprn_rank_")
    names, n_pairs, n_paths = [], 0, 0
    for P in sorted(buckets):
        idx, labels = buckets[P]
        nm = "test_%d.npz" % P
        formats.save_path_file(os.path.join(d, nm), labels, idx, 1)
        names.append(nm)
        n_pairs += idx.shape[0]
        n_paths += idx.shape[0] * P
    with open(os.path.join(d, "test.list"), "w") as f:
        f.write("\n".join(names) + "\n")
    users = n_pairs // cand
    line_of = np.random.default_rng(11).permutation(n_pairs)[:users * cand]   # candidate c of user u is line line_of[u * cand + c]
    who = np.full(n_pairs, -1, np.int64)
    who[line_of] = np.arange(users * cand)
    entity = ["0\t%d\t%d\n" % ((w // cand, w % cand) if w >= 0 else (users, i)) for i, w in enumerate(who)]
    samples = [(str(u), "0", [str(c) for c in range(1, cand)]) for u in range(users)]
    fl = BatcherFileList(d, 512, False, 1000, True, "test.list", check_ids=False)
    out = {}
    res_file = os.path.join(d, "test.res")
    t_index = time.perf_counter()
    members, off, n_used = evalrank.group_index(entity, samples)
    t_index = time.perf_counter() - t_index

    def text_chain():
        fl.reset()
        with open(res_file, "wb") as f:
            scoring.write_scores(eng, fl, f, 1)
        with open(res_file) as f:
            lines = f.readlines()
        score_of = {}
        for line in evalrank.combine_result(entity, lines):
            ll = line.strip().split("\t")
            score_of[(ll[0], ll[1])] = float(ll[3])
        out["a"] = evalrank.eval_samples(score_of, samples)

    def host_rule():
        fl.reset()
        scores = np.concatenate([p for _, p in scoring.score_batches(eng, fl, 1)])
        out["b"] = evalrank.metrics_from_hist(_ffi.host_rank_groups(scores, off, members=members)["hist"], 15)

    def device():
        fl.reset()
        out["c"] = evalrank.metrics_from_hist(scoring.rank_test_set(eng, fl, members, off)[0]["hist"], 15)

    ta, tb, tc = alternate(text_chain, host_rule, device)
    for k in range(1, 16):
        assert out["a"][0][k] == out["b"][0][k] == out["c"][0][k] and abs(out["a"][1][k] - out["c"][1][k]) < 1e-9
    eng.board_reserve(n_pairs)
    fl.reset()
    eng.board_write(0, np.concatenate([p for _, p in scoring.score_batches(eng, fl, 1)]))
    launch = kernel_ms(lambda: eng.rank_groups(off, members=members))
    res[tag] = {"pairs": n_pairs, "paths": n_paths, "users": users, "candidates": cand, "buckets": len(names), "group_index_s_once": round(t_index, 4),
                "text_chain_s": [round(x, 4) for x in ta], "score_batches_plus_host_rule_s": [round(x, 4) for x in tb],
                "rank_test_set_s": [round(x, 4) for x in tc], "rank_launch_ms": launch[0], "hit10": out["c"][0][10], "ndcg10": out["c"][1][10]}
    shutil.rmtree(d, ignore_errors=True)


small = {}
for i, (P, n) in enumerate(((1, 60000), (2, 50000), (3, 30000), (5, 11500))):
    small[P] = synth.make_paths(n, P, T, Ve=Ve, seed=99 + i)
test_set("test_set_1500x101", small, 101)
test_set("test_set_large", synth.make_bucketed(int(total_pairs * 1.75), T, Ve=Ve, seed=77), 101)

# ---- 3: the kernels over the group size ------------------------------------------------------------------------------------------------
# groups above 256 members have two kernel bodies to choose from (rank_groups.hip): places by counting, or an LDS sort; option "rank_sort_min" moves the switch
G = 10000
rng = np.random.default_rng(3)
sizes = {}
for n in (2, 64, 101, 256, 257, 512, 1024, 2048, 4096):
    s = rng.random(G * n).astype(np.float32)
    eng.board_reserve(G * n)
    eng.board_write(0, s)
    off = np.arange(0, G * n + 1, n, dtype=np.int64)
    ref = eng.rank_groups(off, K=10)
    calls = [timed(lambda: eng.rank_groups(off, K=10)) for _ in range(3)]
    host = [timed(lambda: _ffi.host_rank_groups(s, off, K=10)) for _ in range(3)] if n <= 512 else None
    sizes[n] = {"call_ms": [round(1e3 * x, 3) for x in calls], "host_twin_ms": None if host is None else [round(1e3 * x, 3) for x in host]}
    legs = {"shipped": None} if n <= 256 else {"count": "4097", "sort": "257"}
    for _ in range(3):
        for leg, env in legs.items():
            if env is not None:
                eng.set_option("rank_sort_min", env)
            ms, _l = kernel_ms(lambda: eng.rank_groups(off, K=10))
            sizes[n].setdefault("launch_ms_" + leg, []).append(ms)
            if env is not None:
                got = eng.rank_groups(off, K=10)
                assert all(np.array_equal(got[k], ref[k]) for k in ref)
            eng.set_option("rank_sort_min", "512")
res["kernel_over_group_size"] = {"groups": G, "K": 10, "by_members": sizes}
print(json.dumps(res))
