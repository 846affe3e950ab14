"""Times kprn_find_paths against its host twin on one synthetic graph: a user-item graph with skewed item popularity,
n_users + n_items nodes, n_ratings `rate` edges and their inverses, random (user, item) pairs, 3 hops, a cap per pair.

  python scripts/gpu_path_find_bench.py [--users 80000 --items 20000 --ratings 1000000 --pairs 4096 --cap 28 --threads 16 --reps 5]

Prints one JSON line: the graph build, the finder call (counting pass + slot creation with the fill pass, validation, plan and index: what a caller
waits for; median of --reps calls after one warm-up), the two finder kernels from the engine's profiler, and the twin on --threads host threads.
Then, under "cap_modes" (DESIGN.md 3.20), the seeded call kprn_find_paths_sampled at the same hops with option "path_cap" "first" and "spread" in turn in the
same process: per mode the synchronous call, the kernels, and whether the device equals the twin kprn_host_find_paths_cap.
--meta_paths K (0 = off): every rating is of one of K kinds, each kind a relation and its inverse, and after the unfiltered figures the
graph gets the pattern set "kind 0 all the way" -- rate0; rate0 _rate0 rate0: one K-th of the relations admitted at each position -- and "meta_paths" reports
the same call, its kernels, the paths it finds and whether the device equals the twin kprn_host_find_paths_patterns, beside the unfiltered time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402


def alternate(eng, call, reps):
    """option "path_cap" "first" and "spread" in turn in one process, reps + 1 rounds (a warm-up first), then one profiled call each -> per mode: the batch's ids and
    counts of the warm-up, the median and all times of the synchronous call, the finder's kernels from the engine's profiler"""
    res = {m: dict(ts=[]) for m in ("first", "spread")}
    for rep in range(reps + 1):
        for m in res:
            eng.set_option("path_cap", m)
            t0 = time.perf_counter()
            b, c, f = call()
            res[m]["ts"].append(time.perf_counter() - t0)
            if rep == 0:
                res[m]["got"] = (b.read_idx(), c, f)
            b.free()
    for m in res:
        eng.set_option("path_cap", m)
        eng.sync()
        eng.profile_reset()
        eng.profile(True)
        call()[0].free()
        eng.sync()
        eng.profile(False)
        res[m]["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("find_paths")}
    eng.set_option("path_cap", "first")
    return res


def report(r):
    return dict(find_paths_s=float(np.median(r["ts"][1:])), find_paths_all_s=[round(t, 5) for t in r["ts"]], kernels_ms=r["kernels_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--cap", type=int, default=28); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_device", type=int, default=0); ap.add_argument("--meta_paths", type=int, default=0)
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
    pairs = np.stack([rng.randint(1, a.users + 1, size=a.pairs), a.users + 1 + rng.randint(0, a.items, size=a.pairs)], axis=1).astype(np.int32)
    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), pairs=a.pairs, hops=3, cap=a.cap, threads=a.threads)
    t0 = time.perf_counter()
    idx, counts, found = _ffi.host_find_paths(src, dst, rel, nt, Vr, Vt, end_rel, pairs, 1, 3, a.cap, 4, threads=a.threads)
    out["twin_s"] = time.perf_counter() - t0
    out.update(paths_kept=int(counts.sum()), paths_found=int(found.sum()), pairs_with_paths=int((counts > 0).sum()), found_max=int(found.max()))
    if not a.skip_device:
        eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
        t0 = time.perf_counter()
        gr = eng.graph(src, dst, rel, nt, end_rel)
        out["graph_build_s"] = time.perf_counter() - t0
        out["edges_stored"] = gr.n_edges
        ts = []
        for rep in range(a.reps + 1):
            if rep == a.reps:
                eng.profile(True)
            t0 = time.perf_counter()
            b, c, f = eng.find_paths(gr, pairs, 1, 3, a.cap, 4)
            ts.append(time.perf_counter() - t0)
            if rep == 0:
                out["equal_to_twin"] = bool(np.array_equal(c, counts) and np.array_equal(f, found) and np.array_equal(b.read_idx(), idx))
            b.free()
        out["find_paths_s"] = float(np.median(ts[1:a.reps]))
        out["find_paths_all_s"] = [round(t, 5) for t in ts]
        eng.sync()
        out["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("find_paths")}
        eng.profile(False)
        res = alternate(eng, lambda: eng.find_paths(gr, pairs, 1, 3, a.cap, 4, walks=0, seed=1, draw=0), a.reps)
        want = _ffi.host_find_paths_cap(src, dst, rel, nt, Vr, Vt, end_rel, pairs, 1, 3, a.cap, 4, 0, 1, 0, cap="spread", threads=a.threads)
        out["cap_modes"] = {m: report(res[m]) for m in res}
        out["cap_modes"]["first"]["equal_to_twin"] = bool(all(np.array_equal(x, y) for x, y in zip(res["first"]["got"], (idx, counts, found))))
        out["cap_modes"]["spread"]["equal_to_twin"] = bool(all(np.array_equal(x, y) for x, y in zip(res["spread"]["got"], want)))
        out["cap_modes"]["spread"]["rows_that_differ_from_first"] = int((res["spread"]["got"][0] != res["first"]["got"][0]).any(axis=(1, 2)).sum())
        if a.meta_paths > 0:
            patterns = [[{1}], [{1}, {2}, {1}]]
            fidx, fcounts, ffound = _ffi.host_find_paths_patterns(src, dst, rel, nt, Vr, Vt, end_rel, pairs, 1, 3, a.cap, 4, patterns=patterns, threads=a.threads)
            gr.set_patterns(patterns)
            ts = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                b, c, f = eng.find_paths(gr, pairs, 1, 3, a.cap, 4)
                ts.append(time.perf_counter() - t0)
                if rep == 0:
                    equal = bool(np.array_equal(c, fcounts) and np.array_equal(f, ffound) and np.array_equal(b.read_idx(), fidx))
                b.free()
            eng.sync()
            eng.profile_reset()
            eng.profile(True)
            eng.find_paths(gr, pairs, 1, 3, a.cap, 4)[0].free()
            eng.sync()
            eng.profile(False)
            out["meta_paths"] = dict(kinds=a.meta_paths, find_paths_s=float(np.median(ts[1:])), find_paths_all_s=[round(t, 5) for t in ts],
                                     kernels_ms={k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("find_paths")}, equal_to_twin=equal,
                                     paths_kept=int(fcounts.sum()), paths_found=int(ffound.sum()), pairs_with_paths=int((fcounts > 0).sum()),
                                     unfiltered_find_paths_s=out["find_paths_s"], unfiltered_kernels_ms=out["kernels_ms"])
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
