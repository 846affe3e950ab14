"""Times what the pooling temperature (option "pool_gamma") could cost: the pooling and loss-stage launches at gamma = 1 against gamma = 0.5,
and bench.py's step on this build against another build's library (the parent commit's, built in the same session).

  python scripts/gpu_pool_gamma_bench.py [--pairs 4096 --reps 200 --warmup 20] [--parent_lib PATH --rounds 3 --steps 24 --bench_warmup 6]

Prints one JSON line.
  launches   one engine (the fused two-layer D = H = 64 model), one rectangular batch of --pairs pairs x 16 paths and one ragged batch of the same pairs with drawn
             counts and a few long pairs (the wave form).  Every repetition runs a scoring pass and a backward at gamma = 1 and at gamma = 0.5, alternating inside
             the one loop, the order flipping every repetition; the profiler's pool_sigmoid and loss_stage entries (device time, ms per launch) are kept per gamma:
             median (p10, p90) of --reps after --warmup.  The same under "loss" = "bpr" on a group table of 1 + 4 (loss_stage_pairwise).
  bench      with --parent_lib: `python bench.py --gpus 1 --steps K --warmup W` (resident feed, the side measurements off) --rounds times with KPRN_LIB = the parent's
             library and --rounds times on this build, alternating; ms_per_step of every run, the parent's own min .. max band, and whether this build's median
             lies inside it.  No rate is set in advance: the parent is the yardstick."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kprn_amd import _ffi, synth  # noqa: E402

GAMMAS = ("1", "0.5")


def launches(a):
    eng = _ffi.Engine(6, 3000, 9, 16, 32, 16, 64, 2, param_init=0.5)
    idx, labels = synth.make_paths(a.pairs, 16, 6, Ve=3000, seed=1)
    counts = synth.draw_num_paths(np.random.default_rng(2), a.pairs)
    counts[:: max(1, a.pairs // 16)] = 70
    ridx, _, rlabels = synth.make_ragged(a.pairs, 6, Ve=3000, seed=3, counts=counts)
    batches = {"rectangular": eng.batch(idx, labels), "ragged": eng.batch_ragged(ridx, counts, rlabels)}
    go = np.arange(0, a.pairs + 1, 5, dtype=np.int32)
    if go[-1] != a.pairs:
        go = np.append(go, a.pairs).astype(np.int32)
    out = {}
    for loss in ("bce", "bpr"):
        eng.set_option("loss", loss)
        for name, b in batches.items():
            if loss == "bpr":
                lab = np.zeros(a.pairs, np.float32)
                lab[go[:-1]] = 1.0
                b = eng.batch(idx, lab) if name == "rectangular" else eng.batch_ragged(ridx, counts, lab)
                b.set_groups(go)
            ts = {g: {} for g in GAMMAS}
            eng.profile(True)
            for k in range(a.warmup + a.reps):
                for g in (GAMMAS if k % 2 == 0 else GAMMAS[::-1]):
                    eng.set_option("pool_gamma", g)
                    eng.profile_reset()
                    eng.forward(b, 1)
                    eng.backward(b, 1, want_loss=False)
                    eng.sync()
                    if k >= a.warmup:
                        for key, v in eng.profile_get().items():
                            if key.startswith(("pool_sigmoid", "loss_stage")):
                                ts[g].setdefault(key, []).append(v[0] / max(1, v[1]))
            eng.profile(False)
            res = {}
            for g in GAMMAS:
                res["gamma_" + g] = {key: [round(float(x), 5) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))] for key, v in ts[g].items()}
            res["ratio_half_over_one"] = {key: round(float(np.median(ts["0.5"][key]) / np.median(ts["1"][key])), 4) for key in ts["1"]}
            out[loss + "_" + name] = res
    eng.set_option("pool_gamma", "1")
    eng.close()
    return dict(pairs=a.pairs, paths=dict(rectangular=a.pairs * 16, ragged=int(counts.sum())), reps=a.reps, warmup=a.warmup, ms_per_launch=out)


def bench_runs(a):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline",
           "--no-other-configs", "--no-batch-sweep", "--no-alt", "--no-extra-regions", "--no-strong-1m", "--no-kernel-events", "--batch-feed", "resident"]
    runs = {"parent": [], "this": []}
    for r in range(a.rounds):
        for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            env.pop("KPRN_LIB", None)
            if who == "parent":
                env["KPRN_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=a.bench_timeout)
            if p.returncode != 0:
                raise SystemExit("bench.py failed (%s): %s" % (who, p.stderr[-2000:]))
            runs[who].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
    lo, hi = min(runs["parent"]), max(runs["parent"])
    med = float(np.median(runs["this"]))
    return dict(steps=a.steps, warmup=a.bench_warmup, rounds=a.rounds, ms_per_step=runs, parent_band=[lo, hi], this_median=med,
                this_median_inside_parent_band=bool(lo <= med <= hi), this_median_over_parent_median=round(med / float(np.median(runs["parent"])), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096); ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent_lib", default=""); ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--bench_warmup", type=int, default=6); ap.add_argument("--bench_timeout", type=int, default=280)
    ap.add_argument("--no_launches", action="store_true")
    a = ap.parse_args()
    out = {}
    if not a.no_launches:
        out["launches"] = launches(a)
    if a.parent_lib:
        out["bench"] = bench_runs(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
