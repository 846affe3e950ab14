"""Times kprn_find_candidates_top against kprn_find_candidates in the same run, and the chain behind each, on the synthetic graph of
scripts/gpu_candidates_bench.py: n_users + n_items nodes, n_ratings `rate` edges and their inverses, skewed item popularity; catalogue = the
items; the same 256 random users; hops 1..3, exclude_adjacent = 1.

  python scripts/gpu_candidates_top_bench.py [--users 80000 --items 20000 --ratings 1000000 --n_users 256 --threads 16 --reps 4 --chain_cap 256
                                              --chain_users 256 --max_paths 28 --out FILE]

Prints one JSON line (and, with --out, rewrites FILE after every stage so that a run cut short leaves what it measured):
  calls_s            the host clock around the synchronous calls, median of --reps calls after one warm-up each, the variants alternating inside one loop:
                     "plain" = kprn_find_candidates (the yardstick), "cap64" / "cap256" / "capmax" = kprn_find_candidates_top (the list is not read back
                     inside the clock)
  kernels_ms         one profiled call of each kind from the engine's profiler: candidates_mark / _count / _fill and candidates_tally / _settle / _select /
                     _fill_top (of the cap 256 call)
  equal_to_twin      the three capped lists, their group counts and their path counts against kprn_host_find_candidates_top; capmax_equals_plain: the
                     list of the largest cap against kprn_find_candidates'
  chain              for --chain_users of the users, the chain of graph.recommend_users up to the ranking, capped at --chain_cap and uncapped: seconds per
                     stage (the stream drained after each: candidates, find_paths_of_candidates, forward_async, board_reserve + board_put, rank_groups),
                     their sum, the pairs and the paths scored."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402

CAP_MAX = 2**31 - 1


def chain(eng, gr, sm, users, cap, max_paths, K=10):
    """graph.recommend_users up to the ranking stage, the stream drained after every stage -> dict of seconds and sizes"""
    t = {}

    def stage(name, fn):
        t0 = time.perf_counter()
        r = fn()
        eng.sync()
        t[name] = time.perf_counter() - t0
        return r

    pairs, gc = stage("candidates", lambda: eng.find_candidates(gr, sm, users, 1, 3, True, cap=cap))   # (with the list read back, as the chain does)
    batch, counts, found = stage("find_paths_of_candidates", lambda: eng.find_paths_of_candidates(gr, len(pairs), 1, 3, max_paths, 4))
    try:
        stage("forward_async", lambda: eng.forward_async(batch, 1))
        stage("board_put", lambda: (eng.board_reserve(batch.B), eng.board_put(0, batch.B)))
        ends = np.concatenate([[0], np.cumsum(gc, dtype=np.int64)])
        goff = [0]
        for g in range(len(users)):
            for lo in range(int(ends[g]), int(ends[g + 1]), _ffi.RANK_MAX_GROUP):
                goff.append(min(lo + _ffi.RANK_MAX_GROUP, int(ends[g + 1])))
        stage("rank_groups", lambda: eng.rank_groups(np.array(goff, np.int64), pos=np.full(len(goff) - 1, -1, np.int32), K=K, mode=_ffi.RANK_PRINTED))
        return dict(seconds={k: round(v, 5) for k, v in t.items()}, total_s=round(sum(t.values()), 5), pairs=int(len(pairs)), pairs_scored=int(batch.B),
                    paths_scored=int(batch.counts.sum()), paths_found=int(found.sum()), sub_groups=len(goff) - 1)
    finally:
        batch.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--n_users", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--chain_cap", type=int, default=256); ap.add_argument("--chain_users", type=int, default=256)
    ap.add_argument("--max_paths", type=int, default=28); ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    pop = 1.0 / (np.arange(a.items) + 10.0) ** 0.8
    u = rng.randint(1, a.users + 1, size=a.ratings).astype(np.int32)
    it = (a.users + 1 + rng.choice(a.items, size=a.ratings, p=pop / pop.sum())).astype(np.int32)
    src, dst = np.concatenate([u, it]), np.concatenate([it, u])
    rel = np.concatenate([np.full(a.ratings, 1, np.int32), np.full(a.ratings, 2, np.int32)])
    Ve, Vr, Vt, end_rel = a.users + a.items + 1, 4, 4, 3
    nt = np.ones((Ve, 1), np.int32)
    nt[a.users:] = 2
    items = np.arange(a.users + 1, a.users + a.items + 1, dtype=np.int32)
    users = rng.randint(1, a.users + 1, size=a.n_users).astype(np.int32)
    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), catalogue=a.items, users=a.n_users, hops=[1, 3], exclude_adjacent=1, threads=a.threads)

    def note():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
    gr = eng.graph(src, dst, rel, nt, end_rel)
    sm = eng.sampler(items)
    gc, total = np.zeros(a.n_users, np.int32), C.c_int64()
    variants = (("plain", 0), ("cap64", 64), ("cap256", 256), ("capmax", CAP_MAX))

    def call(cap):
        if cap == 0:
            eng._ck(eng.L.kprn_find_candidates(eng.h, gr.ptr, sm.ptr, _ffi._fp(users), a.n_users, 1, 3, 1, _ffi._fp(gc), C.byref(total)))
        else:
            eng._ck(eng.L.kprn_find_candidates_top(eng.h, gr.ptr, sm.ptr, _ffi._fp(users), a.n_users, 1, 3, 1, cap, _ffi._fp(gc), C.byref(total)))
        return int(total.value)

    ts, totals = {name: [] for name, _ in variants}, {}
    for rep in range(a.reps + 1):                      # rep 0 warms up; the variants alternate inside the loop
        for name, cap in variants:
            t0 = time.perf_counter()
            totals[name] = call(cap)
            ts[name].append(time.perf_counter() - t0)
    out["calls_s"] = {name: float(np.median(v[1:])) for name, v in ts.items()}
    out["calls_all_s"] = {name: [round(t, 5) for t in v] for name, v in ts.items()}
    out["totals"] = totals
    out["ratio_to_plain"] = {name: round(out["calls_s"][name] / out["calls_s"]["plain"], 3) for name, _ in variants[1:]}
    eng.sync()
    eng.profile(True)
    call(0)
    call(256)
    eng.sync()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("candidates_")}
    eng.profile(False)
    note()
    plain_pairs, plain_gc = eng.find_candidates(gr, sm, users, 1, 3, 1)
    equal = {}
    for name, cap in variants[1:]:
        t0 = time.perf_counter()
        cand, gc_twin, n_twin = _ffi.host_find_candidates_top(src, dst, rel, Ve, items, users, 1, 3, cap, 1, threads=a.threads)
        out.setdefault("twin_s", {})[name] = round(time.perf_counter() - t0, 3)
        pairs, gc_dev = eng.find_candidates(gr, sm, users, 1, 3, 1, cap=cap)
        equal[name] = bool(np.array_equal(gc_dev, gc_twin) and np.array_equal(pairs[:, 1], cand) and np.array_equal(pairs[:, 0], np.repeat(users, gc_twin))
                           and np.array_equal(eng.candidate_path_counts(), n_twin))
        if cap == CAP_MAX:
            out["capmax_equals_plain"] = bool(np.array_equal(pairs, plain_pairs) and np.array_equal(gc_dev, plain_gc))
            out["per_user_max"] = int(gc_dev.max()); out["n_paths_max"] = int(n_twin.max())
    out["equal_to_twin"] = equal
    note()
    if a.chain_users > 0:
        us = users[:a.chain_users]
        out["chain"] = dict(users=len(us), cap=a.chain_cap, max_paths=a.max_paths)
        chain(eng, gr, sm, us[:2], a.chain_cap, a.max_paths)                           # warm-up: two users through every stage
        for name, cap in (("capped", a.chain_cap), ("uncapped", 0)):
            try:
                out["chain"][name] = chain(eng, gr, sm, us, cap, a.max_paths)
            except _ffi.KprnError as ex:                                               # (a refusal or an allocation that did not fit is a result too)
                out["chain"][name] = dict(error=str(ex))
            note()
        c, n = out["chain"]["capped"], out["chain"]["uncapped"]
        if "total_s" in c and "total_s" in n:
            out["chain"]["uncapped_over_capped"] = dict(time=round(n["total_s"] / c["total_s"], 2), pairs=round(n["pairs"] / max(c["pairs"], 1), 2),
                                                        paths=round(n["paths_scored"] / max(c["paths_scored"], 1), 2))
    eng.close()
    note()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
