#!/usr/bin/env python3
"""What the explanation stage (include/kprn.h "explaining a recommendation": kprn_explain_batch, kprn_recommend_explain_ragged) costs.  One JSON object from
one process; every comparison is a warm-up and then three alternating repetitions per leg, timed with a device synchronise around each.

1. explain_batch over every pair, M = 5, on device-resident batches -- a 65 536-path rectangular batch (P = 4) and a make_bucketed set of ~1 M paths (the set
   of gpu_ragged_probe.py, one rectangular batch per bucket chunk of at most 65 536 paths) -- against (a) forward returning the probabilities only (what the
   stage adds) and (b) today's route: forward returning path_scores [N,46] too, then the host twin over them; and the launch alone from the engine's profile;
2. one user's 101 candidates (177 paths, the batch of gpu_rank_probe.py): recommend_explain_ragged (K = 10, M = 3) against recommend_ragged: us per user.

usage: gpu_explain_probe.py [total_paths]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kprn_amd import _ffi, synth  # noqa: E402

total = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
Vt, Ve, Vr, T = 6, 2851220, 9, 6
M = 5
eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2, seed=1)
res = {"what": "explanation stage: cost over a scoring pass, against the host route, one-user latency", "T": T, "D": 64, "H": 64, "L": 2, "Ve": Ve, "M": M}


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
    eng.set_option("profile_filter", "explain_paths")
    eng.profile(True)
    eng.profile_reset()
    fn()
    got = eng.profile_get().get("explain_paths", (0.0, 0))
    eng.profile(False)
    eng.set_option("profile_filter", "")
    return round(got[0], 4), got[1]


def compare(tag, batches):
    """batches: [(Batch, offsets)]"""
    keep = {}

    def probs_only():
        for b, _ in batches:
            keep["p"] = eng.forward(b, 1)["probs"]

    def device():
        for b, _ in batches:
            keep["d"] = eng.explain_batch(b, M, 1)

    def host_route():
        for b, off in batches:
            f = eng.forward(b, 1, want=("probs", "path_scores"))
            keep["h"] = _ffi.host_explain(f["path_scores"], off, 1, 2, 5, M)

    tp, td, th = alternate(probs_only, device, host_route)
    assert keep["d"]["path_idx"].tobytes() == keep["h"]["path_idx"].tobytes() and keep["d"]["probs"].tobytes() == keep["p"].tobytes()
    launch = kernel_ms(device)
    res[tag] = {"batches": len(batches), "pairs": int(sum(b.B for b, _ in batches)), "paths": int(sum(b.n_paths for b, _ in batches)),
                "forward_probs_only_ms": [round(1e3 * x, 3) for x in tp], "explain_batch_ms": [round(1e3 * x, 3) for x in td],
                "forward_path_scores_plus_host_twin_ms": [round(1e3 * x, 3) for x in th], "explain_launches_ms": launch[0], "explain_launches": launch[1]}


def rect(idx):
    B, P = idx.shape[:2]
    return eng.batch(idx), (np.arange(B + 1, dtype=np.int64) * P).astype(np.int32)


idx, _ = synth.make_paths(16384, 4, T, Ve=Ve, seed=5)
compare("rect_65536", [rect(idx)])
batches = []
for P, (bi, _l) in sorted(synth.make_bucketed(total, T, Ve=Ve, seed=77).items()):
    rows = max(1, 65536 // P)
    for r0 in range(0, bi.shape[0], rows):
        batches.append(rect(bi[r0:r0 + rows]))
compare("bucketed", batches)
del batches

# ---- 2: one user's candidates ------------------------------------------------------------------------------------------------------------
counts = synth.draw_num_paths(np.random.default_rng(7), 101)
cidx, _, _ = synth.make_ragged(101, T, Ve=Ve, seed=25, counts=counts)
REP = 200
keep = {}


def plain():
    for _ in range(REP):
        keep["r"] = eng.recommend_ragged(cidx, counts, [101], 10)


def explained():
    for _ in range(REP):
        keep["e"] = eng.recommend_explain_ragged(cidx, counts, [101], 10, 3)


t_r, t_e = alternate(plain, explained)
assert keep["r"][0].tobytes() == keep["e"]["topk_idx"].tobytes()
res["candidates"] = {"pairs": 101, "paths": int(counts.sum()), "K": 10, "M": 3, "recommend_ragged_us_per_user": [round(1e6 * x / REP, 1) for x in t_r],
                     "recommend_explain_ragged_us_per_user": [round(1e6 * x / REP, 1) for x in t_e]}
print(json.dumps(res))
