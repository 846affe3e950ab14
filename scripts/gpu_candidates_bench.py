"""Times kprn_find_candidates against its host twin, and against the route a caller had to take before it -- kprn_find_paths over every (user, catalogue
item) pair -- on the synthetic graph of scripts/gpu_path_find_bench.py: n_users + n_items nodes, n_ratings `rate` edges and their
inverses, skewed item popularity; catalogue = the items; random users; hops 1..3.

  python scripts/gpu_candidates_bench.py [--users 80000 --items 20000 --ratings 1000000 --n_users 256 --threads 16 --reps 5 --catalogue_users 256]

Prints one JSON line: the host clock around kprn_find_candidates (median of --reps calls after one warm-up; the list is not read back inside the clock),
the three kernel families from the engine's profiler, total, the twin on --threads host threads, whether the two agree, and -- for --catalogue_users of
the same users (0 = skip; 256 x 20 000 = 5.1 M workgroups by default, about a second) -- one kprn_find_paths call over users x catalogue with the
number of pairs it finds reachable, and kprn_find_candidates for those users alone.
--meta_paths K (0 = off): every rating is of one of K kinds, each kind a relation and its inverse, and after the unfiltered figures the
graph gets the pattern set "kind 0 all the way" -- rate0; rate0 _rate0 rate0: one K-th of the relations admitted at each position -- and "meta_paths" reports
the same kprn_find_candidates call, its kernels, its total and whether it equals the twin kprn_host_find_candidates_patterns, beside the unfiltered time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--n_users", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--catalogue_users", type=int, default=256); ap.add_argument("--meta_paths", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    pop = 1.0 / (np.arange(a.items) + 10.0) ** 0.8
    u = rng.randint(1, a.users + 1, size=a.ratings).astype(np.int32)
    it = (a.users + 1 + rng.choice(a.items, size=a.ratings, p=pop / pop.sum())).astype(np.int32)
    src, dst = np.concatenate([u, it]), np.concatenate([it, u])
    rel = np.concatenate([np.full(a.ratings, 1, np.int32), np.full(a.ratings, 2, np.int32)])
    Ve, Vr, Vt, end_rel = a.users + a.items + 1, 4, 4, 3
    if a.meta_paths > 0:   # every rating is of one of --meta_paths kinds: relations 2k + 1 (rate) and 2k + 2 (its inverse); a second stream, so the edges stay the same
        kind = np.random.RandomState(11).randint(0, a.meta_paths, size=a.ratings).astype(np.int32)
        rel = np.concatenate([2 * kind + 1, 2 * kind + 2])
        Vr, end_rel = 2 * a.meta_paths + 2, 2 * a.meta_paths + 1
    nt = np.ones((Ve, 1), np.int32)
    nt[a.users:] = 2
    items = np.arange(a.users + 1, a.users + a.items + 1, dtype=np.int32)
    users = rng.randint(1, a.users + 1, size=a.n_users).astype(np.int32)
    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), catalogue=a.items, users=a.n_users, hops=[1, 3], exclude_adjacent=1, threads=a.threads)
    t0 = time.perf_counter()
    cand, gc_twin = _ffi.host_find_candidates(src, dst, rel, Ve, items, users, 1, 3, 1, threads=a.threads)
    out["twin_s"] = time.perf_counter() - t0            # (two calls: the counts, then the ids)
    eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
    gr = eng.graph(src, dst, rel, nt, end_rel)
    sm = eng.sampler(items)
    gc, total = np.zeros(a.n_users, np.int32), C.c_int64()
    ts = []
    for rep in range(a.reps + 1):
        if rep == a.reps:
            eng.profile(True)
        t0 = time.perf_counter()
        eng._ck(eng.L.kprn_find_candidates(eng.h, gr.ptr, sm.ptr, _ffi._fp(users), a.n_users, 1, 3, 1, _ffi._fp(gc), C.byref(total)))
        ts.append(time.perf_counter() - t0)
    eng.sync()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("candidates_")}
    eng.profile(False)
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, 1)
    out.update(find_candidates_s=float(np.median(ts[1:a.reps])), find_candidates_all_s=[round(t, 5) for t in ts], total=int(total.value),
               per_user_max=int(gc.max()), equal_to_twin=bool(np.array_equal(gc, gc_twin) and np.array_equal(pairs[:, 1], cand)
                                                              and np.array_equal(pairs[:, 0], np.repeat(users, gc))))
    if a.catalogue_users > 0:
        # before this call existed: every (user, item) pair through the finder, most of which have no path (counts only matter; the cap is 1)
        us = users[:a.catalogue_users]
        every = np.stack([np.repeat(us, a.items), np.tile(items, len(us))], axis=1).astype(np.int32)
        t0 = time.perf_counter()
        b, c, f = eng.find_paths(gr, every, 1, 3, 1, 4)
        out.update(catalogue_route_users=len(us), catalogue_route_pairs=int(every.shape[0]), catalogue_route_s=time.perf_counter() - t0,
                   catalogue_route_reachable=int((c > 0).sum()))
        if b is not None:
            b.free()
        gc_same = np.zeros(len(us), np.int32)
        t0 = time.perf_counter()
        eng._ck(eng.L.kprn_find_candidates(eng.h, gr.ptr, sm.ptr, _ffi._fp(us), len(us), 1, 3, 0, _ffi._fp(gc_same), C.byref(total)))
        out["find_candidates_same_users_s"] = time.perf_counter() - t0
        out["find_candidates_same_users_total"] = int(total.value)     # (exclude_adjacent = 0, u itself no item: the pairs the route finds reachable)
        out["ratio_route_over_candidates"] = out["catalogue_route_s"] / max(out["find_candidates_same_users_s"], 1e-9)
    if a.meta_paths > 0:
        patterns = [[{1}], [{1}, {2}, {1}]]
        fcand, fgc, _ = _ffi.host_find_candidates_patterns(src, dst, rel, Ve, items, users, 1, 3, 2**31 - 1, 1, patterns, threads=a.threads)
        gr.set_patterns(patterns)
        eng.profile_reset()
        ts = []
        for rep in range(a.reps + 1):
            if rep == a.reps:
                eng.profile(True)
            t0 = time.perf_counter()
            eng._ck(eng.L.kprn_find_candidates(eng.h, gr.ptr, sm.ptr, _ffi._fp(users), a.n_users, 1, 3, 1, _ffi._fp(gc), C.byref(total)))
            ts.append(time.perf_counter() - t0)
        eng.sync()
        kernels = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("candidates_")}
        eng.profile(False)
        pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, 1)
        out["meta_paths"] = dict(kinds=a.meta_paths, find_candidates_s=float(np.median(ts[1:a.reps])), find_candidates_all_s=[round(t, 5) for t in ts],
                                 kernels_ms=kernels, total=int(len(pairs)), equal_to_twin=bool(np.array_equal(gc, fgc) and np.array_equal(pairs[:, 1], fcand)),
                                 unfiltered_find_candidates_s=out["find_candidates_s"], unfiltered_kernels_ms=out["kernels_ms"])
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
