"""Times kprn_graph_update against the route a caller had to take before it -- kprn_graph_create over the whole edited edge list -- on a seeded random
graph: --nodes-per-edge sets the node count, relations 1..4, every edge drawn uniformly.

  python scripts/gpu_graph_update_bench.py [--edges 2000000,20000000 --deltas 1000,100000,1% --reps 5]

For each graph size and each delta size (a number of changes, or a percentage of E; half additions, half removals of stored edges) the host clock around
kprn_graph_update: the median of --reps calls after one warm-up, every call with a fresh seeded delta on the graph as the previous call left it (the edge
count drifts by less than the delta).  Beside it the median of --reps kprn_graph_create calls (after one warm-up) on the edge list the last update left,
in the same process, and whether that fresh graph's CSR equals the updated one's bit for bit.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="2000000,20000000"); ap.add_argument("--deltas", default="1000,100000,1%")
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--nodes-per-edge", type=float, default=0.1)
    a = ap.parse_args()
    out = dict(reps=a.reps, results=[])
    for E in (int(x) for x in a.edges.split(",")):
        rng = np.random.RandomState(7)
        Ve, Vr, Vt, end_rel = max(int(E * a.nodes_per_edge), 16) + 1, 6, 4, 5
        src, dst = rng.randint(1, Ve, size=E).astype(np.int32), rng.randint(1, Ve, size=E).astype(np.int32)
        rel = rng.randint(1, 5, size=E).astype(np.int32)
        nt = np.ones((Ve, 1), np.int32)
        eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
        gr = eng.graph(src, dst, rel, nt, end_rel)
        for spec in a.deltas.split(","):
            n = int(gr.n_edges * float(spec[:-1]) / 100) if spec.endswith("%") else int(spec)
            ts = []
            for rep in range(a.reps + 1):
                rowptr, col, rl = gr.read_csr()
                at = rng.randint(0, len(col), size=n // 2)                                     # (one listed twice is removed once)
                removes = np.stack([np.searchsorted(rowptr, at, side="right") - 1, col[at], rl[at]], axis=1).astype(np.int32)
                adds = np.stack([rng.randint(1, Ve, n - n // 2), rng.randint(1, Ve, n - n // 2), rng.randint(1, 5, n - n // 2)], axis=1).astype(np.int32)
                t0 = time.perf_counter()
                counts = gr.update(adds, removes)
                ts.append(time.perf_counter() - t0)
            rowptr, col, rl = gr.read_csr()
            s2 = np.repeat(np.arange(Ve, dtype=np.int32), np.diff(rowptr))
            tb, fresh = [], None
            for rep in range(a.reps + 1):
                if fresh is not None:
                    fresh.free()
                t0 = time.perf_counter()
                fresh = eng.graph(s2, col, rl, nt, end_rel)
                tb.append(time.perf_counter() - t0)
            equal = all(np.array_equal(x, y) for x, y in zip(fresh.read_csr(), (rowptr, col, rl)))
            fresh.free()
            up, rb = float(np.median(ts[1:])), float(np.median(tb[1:]))
            out["results"].append(dict(edges=int(len(col)), nodes=Ve - 1, delta=spec, changes=n, last_counts=list(counts), update_s=round(up, 6),
                                       update_all_s=[round(t, 6) for t in ts], rebuild_s=round(rb, 6), rebuild_all_s=[round(t, 6) for t in tb],
                                       rebuild_over_update=round(rb / max(up, 1e-9), 3), equal_to_rebuild=bool(equal)))
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
