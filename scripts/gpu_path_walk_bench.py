"""Times kprn_find_paths_sampled against its host twin on the synthetic graph of scripts/gpu_path_find_bench.py: hops 1..5, the hops past 3
sampled by --walks walks per pair and hop count, a cap per pair, T = 6 -- and, beside it, the same pairs at max_hops = 3, the figure to read the cost against.

  python scripts/gpu_path_walk_bench.py [--users 80000 --items 20000 --ratings 1000000 --pairs 4096 --cap 28 --walks 64 --threads 16 --reps 5]

Prints one JSON line: per configuration (hops5 / hops3) the synchronous call (median of --reps calls after one warm-up), the finder's kernels from the engine's
profiler and whether the device equals the twin; the twin's time on --threads host threads; the pairs and paths found at 4 and at 5 hops.
Then, under "cap_modes" (DESIGN.md 3.20), the hops5 call with option "path_cap" "first" and "spread" in turn in the same process: per mode the synchronous
call, the kernels, and whether the device equals the twin kprn_host_find_paths_cap.
--meta_paths K (0 = off): every rating is of one of K kinds, each kind a relation and its inverse, and after the unfiltered figures the
graph gets the pattern set "kind 0 all the way" at 1, 3 and 5 hops -- one K-th of the relations admitted at each position -- and "meta_paths" reports the
hops5 call, its kernels, the paths it finds and whether the device equals the twin kprn_host_find_paths_patterns, beside the unfiltered time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402

T = 6


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
    ap.add_argument("--cap", type=int, default=28); ap.add_argument("--walks", type=int, default=64); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--skip_device", type=int, default=0)
    ap.add_argument("--meta_paths", type=int, default=0)
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
    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), pairs=a.pairs, cap=a.cap, walks=a.walks, T=T, threads=a.threads)
    twin = lambda lo, hi, **kw: _ffi.host_find_paths_sampled(src, dst, rel, nt, Vr, Vt, end_rel, pairs, lo, hi, a.cap, T, a.walks, 1, 0, threads=a.threads, **kw)
    want = {}
    for name, hi in (("hops5", 5), ("hops3", 3)):
        t0 = time.perf_counter()
        want[name] = twin(1, hi)
        out[name] = dict(twin_s=time.perf_counter() - t0, paths_kept=int(want[name][1].sum()), paths_found=int(want[name][2].sum()),
                         pairs_with_paths=int((want[name][1] > 0).sum()))
    for h in (4, 5):        # (a user-item graph is bipartite: a user reaches an item over an odd number of hops)
        found = twin(h, h, want_idx=False)[2]
        out["hops5"]["pairs_at_%d" % h], out["hops5"]["paths_at_%d" % h] = int((found > 0).sum()), int(found.sum())
    if not a.skip_device:
        eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
        gr = eng.graph(src, dst, rel, nt, end_rel)
        for name, hi in (("hops5", 5), ("hops3", 3)):
            idx, counts, found = want[name]
            eng.profile(False)
            eng.profile_reset()
            ts = []
            for rep in range(a.reps + 1):
                if rep == a.reps:
                    eng.profile(True)
                t0 = time.perf_counter()
                b, c, f = eng.find_paths(gr, pairs, 1, hi, a.cap, T, walks=a.walks, seed=1, draw=0)
                ts.append(time.perf_counter() - t0)
                if rep == 0:
                    out[name]["equal_to_twin"] = bool(np.array_equal(c, counts) and np.array_equal(f, found) and np.array_equal(b.read_idx(), idx))
                b.free()
            out[name]["find_paths_s"] = float(np.median(ts[1:a.reps]))
            out[name]["find_paths_all_s"] = [round(t, 5) for t in ts]
            eng.sync()
            out[name]["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("find_paths")}
        eng.profile(False)
        res = alternate(eng, lambda: eng.find_paths(gr, pairs, 1, 5, a.cap, T, walks=a.walks, seed=1, draw=0), a.reps)
        spread = _ffi.host_find_paths_cap(src, dst, rel, nt, Vr, Vt, end_rel, pairs, 1, 5, a.cap, T, a.walks, 1, 0, cap="spread", threads=a.threads)
        out["cap_modes"] = {m: report(res[m]) for m in res}
        out["cap_modes"]["first"]["equal_to_twin"] = bool(all(np.array_equal(x, y) for x, y in zip(res["first"]["got"], want["hops5"])))
        out["cap_modes"]["spread"]["equal_to_twin"] = bool(all(np.array_equal(x, y) for x, y in zip(res["spread"]["got"], spread)))
        out["cap_modes"]["spread"]["rows_that_differ_from_first"] = int((res["spread"]["got"][0] != res["first"]["got"][0]).any(axis=(1, 2)).sum())
        if a.meta_paths > 0:
            patterns = [[{1}], [{1}, {2}, {1}], [{1}, {2}, {1}, {2}, {1}]]
            fwant = _ffi.host_find_paths_patterns(src, dst, rel, nt, Vr, Vt, end_rel, pairs, 1, 5, a.cap, T, a.walks, 1, 0, patterns=patterns, threads=a.threads)
            gr.set_patterns(patterns)
            call = lambda: eng.find_paths(gr, pairs, 1, 5, a.cap, T, walks=a.walks, seed=1, draw=0)
            ts = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                b, c, f = call()
                ts.append(time.perf_counter() - t0)
                if rep == 0:
                    equal = bool(all(np.array_equal(x, y) for x, y in zip((b.read_idx(), c, f), fwant)))
                b.free()
            eng.sync()
            eng.profile_reset()
            eng.profile(True)
            call()[0].free()
            eng.sync()
            eng.profile(False)
            out["meta_paths"] = dict(kinds=a.meta_paths, find_paths_s=float(np.median(ts[1:])), find_paths_all_s=[round(t, 5) for t in ts],
                                     kernels_ms={k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("find_paths")}, equal_to_twin=equal,
                                     paths_kept=int(fwant[1].sum()), paths_found=int(fwant[2].sum()), pairs_with_paths=int((fwant[1] > 0).sum()),
                                     unfiltered_find_paths_s=out["hops5"]["find_paths_s"], unfiltered_kernels_ms=out["hops5"]["kernels_ms"])
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
