"""Times a training step from a graph with hard negatives on the synthetic graph of scripts/gpu_path_find_bench.py, at the benchmark's D = H = 64
shape: --positives positives a step, n = --negatives kept, a pool of P for every P in --pools.

  python scripts/gpu_hard_negatives_bench.py [--users 80000 --items 20000 --ratings 1000000 --positives 128 --negatives 4 --pools 16,64 --cap 28 --steps 20
                                              --rounds 3]

Per P, milliseconds per step (a round = --steps steps after two warm-up steps, the device drained at the end; the median of --rounds rounds, the cases taken in
turn within a round) of
  a  plain_n     the plain step with n negatives:  find_training_paths(n) -> train_step
  b  plain_P     the plain step with P negatives:  find_training_paths(P) -> train_step
  c  pool        the -neg_pool P step:  find_training_paths(P) -> forward_async -> board_put -> select_hardest -> batch_subset -> train_step
  d  two_finds   the composition without the two calls:  find_training_paths(P) -> forward_async -> board_put -> rank_groups top-(n + 1) -> the kept pair list
                 formed on the host -> find_paths on it -> train_step
and select_subset_ms: select_hardest + batch_subset alone on a scored pool batch (host clock around the two synchronous calls, median of --steps).
Prints one JSON line.  Any failing step ends the script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi, graph as kgraph  # noqa: E402

T, LO, HI = 4, 2, 3


def pool_groups(counts, P):
    """the pool batch's non-empty groups as board runs, and each one's positive (0, or -1 where the positive's row kept no path)"""
    goff = kgraph.groups_from_counts(counts, P).astype(np.int64)
    full = np.diff(goff) > 0
    sel_off = np.concatenate([[0], np.cumsum(np.diff(goff)[full])]).astype(np.int64)
    has_pos = np.asarray(counts).reshape(-1, 1 + P)[:, 0] > 0
    return sel_off, np.where(has_pos[full], 0, -1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--positives", type=int, default=128)
    ap.add_argument("--negatives", type=int, default=4); ap.add_argument("--pools", default="16,64"); ap.add_argument("--cap", type=int, default=28)
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
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
    eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
    gr = eng.graph(src, dst, rel, nt, end_rel)
    s = eng.sampler(np.unique(it))
    opt = _ffi.make_opt(method=1, lr=1e-3)
    n, B = a.negatives, a.positives
    positives = np.stack([u, it], axis=1)
    draw = [0]

    def minibatch():
        draw[0] += 1
        return positives[np.random.RandomState(draw[0]).randint(0, len(positives), size=B)], draw[0]

    def plain(n_neg, st):
        pos, d = minibatch()
        batch, _, _, _ = eng.find_training_paths(gr, s, pos, n_neg, 1, d, LO, HI, a.cap, T)
        if batch is None:
            return
        st["pairs"] += batch.B; st["paths"] += batch.n_paths
        eng.train_step(batch, opt, want_loss=False)
        batch.free()

    def pool_step(P, st):
        pos, d = minibatch()
        batch, _, counts, _ = eng.find_training_paths(gr, s, pos, P, 1, d, LO, HI, a.cap, T)
        if batch is None:
            return
        st["pool_pairs"] += batch.B; st["pool_paths"] += batch.n_paths
        sub, _, _ = kgraph._keep_hardest(eng, batch, counts, P, n, 1)
        st["pairs"] += sub.B; st["paths"] += sub.n_paths
        eng.train_step(sub, opt, want_loss=False)
        sub.free()

    def two_finds(P, st):
        pos, d = minibatch()
        batch, prs, counts, _ = eng.find_training_paths(gr, s, pos, P, 1, d, LO, HI, a.cap, T)
        if batch is None:
            return
        st["pool_pairs"] += batch.B; st["pool_paths"] += batch.n_paths
        try:
            eng.forward_async(batch, 1)
            eng.board_put(0, batch.B)
            sel_off, _ = pool_groups(counts, P)
            top = eng.rank_groups(sel_off, pos=np.full(len(sel_off) - 1, -1, np.int32), K=n + 1, mode=_ffi.RANK_RAW)["topk_idx"]
        finally:
            batch.free()
        row_of = np.nonzero(counts > 0)[0]                      # the pair-list row of every pair of the pool batch
        kept = []
        for k in range(len(sel_off) - 1):
            rows = row_of[sel_off[k]:sel_off[k + 1]]
            best = rows[top[k][top[k] >= 0]]
            if rows[0] % (1 + P) == 0:                          # the group's positive has paths: it stays, whatever it scores
                kept.append(rows[0])
            kept.extend(best[best % (1 + P) != 0][:n])
        kept = np.array(sorted(kept))
        labels = (kept % (1 + P) == 0).astype(np.float32)
        again, _, _ = eng.find_paths(gr, prs[kept], LO, HI, a.cap, T, labels=labels, seed=1, draw=d)
        st["pairs"] += again.B; st["paths"] += again.n_paths
        eng.train_step(again, opt, want_loss=False)
        again.free()

    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), positives=B, negatives=n, cap=a.cap, hops=[LO, HI], steps=a.steps, rounds=a.rounds, pools={})
    for P in [int(x) for x in a.pools.split(",")]:
        eng.board_reserve(B * (1 + P))
        cases = dict(plain_n=lambda st: plain(n, st), plain_P=lambda st: plain(P, st), pool=lambda st: pool_step(P, st), two_finds=lambda st: two_finds(P, st))
        ms = {k: [] for k in cases}
        sizes = {}
        for _ in range(a.rounds):
            for name, step in cases.items():
                st = dict(pairs=0, paths=0, pool_pairs=0, pool_paths=0)
                for _ in range(2):
                    step(dict(st))
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(st)
                eng.sync()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
                sizes[name] = {k: round(v / a.steps, 1) for k, v in st.items() if v}
        # select + subset alone, on a scored pool batch
        alone = []
        for _ in range(a.steps):
            pos, d = minibatch()
            batch, _, counts, _ = eng.find_training_paths(gr, s, pos, P, 1, d, LO, HI, a.cap, T)
            eng.forward_async(batch, 1)
            eng.board_put(0, batch.B)
            sel_off, gpos = pool_groups(counts, P)
            eng.sync()
            t0 = time.perf_counter()
            keep, _ = eng.select_hardest(sel_off, n, pos=gpos)
            sub = eng.batch_subset(batch, keep[:batch.B])
            alone.append((time.perf_counter() - t0) * 1e3)
            sub.free(); batch.free()
        med = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
        out["pools"][str(P)] = dict(ms_per_step=med, all_rounds={k: [round(x, 3) for x in v] for k, v in ms.items()}, per_step=sizes,
                                    select_subset_ms=round(float(np.median(alone)), 3), pool_over_two_finds=round(med["pool"] / med["two_finds"], 3),
                                    pool_between=round((med["pool"] - med["plain_n"]) / max(med["plain_P"] - med["plain_n"], 1e-9), 3))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
