"""What option "deterministic" changes, measured (profiles/deterministic/README.md has the numbers and the commands).

  python scripts/gpu_deterministic_probe.py digests CASE [N]   CASE = tiles16 | tiles64 | bench; N fresh engines (default 20) per mode
      the number of DISTINCT parameter digests after the same steps on the same inputs, option off and on (on must give 1):
      tiles16 / tiles64 are the inputs of tests/test_gpu_deterministic.py (300 paths over 50 entity rows, 12 Adam steps with clip + L2),
      bench is the headline batch shape (16 384 pairs x 4 paths, T = 6, 4 Adam steps; 50 000 entity rows so that 40 engines are quick to make)
  python scripts/gpu_deterministic_probe.py step PATHS         wall time per step and kprn_profile_get's per-family kernel time, option off and on,
      for scripts/gpu_small_batch.py's step (scoring pass queued + training step) at PATHS paths per step

Each call is one bounded piece of GPU work; run it under `timeout`.  The A/B of bench.py against another build's library goes through KPRN_LIB
(kprn_amd/_ffi.py) and bench.py's own --set-option."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kprn_amd import _ffi, synth  # noqa: E402

T = 6


def digests(case, n):
    if case == "bench":
        Ve, steps, options = 50000, 4, ()
        idx, labels = synth.make_paths(16384, 4, T, Ve=Ve, seed=12)
        opt = _ffi.make_opt(method=1, lr=1e-3)
    else:
        Ve, steps, options = 50, 12, ((("small_tiles", "0"),) if case == "tiles64" else ())
        idx, labels = synth.make_paths(150, 2, T, Ve=Ve, seed=5)
        opt = _ffi.make_opt(method=1, lr=2e-3, regularize=1, use_grad_clip=1, grad_clip_norm=0.05, l2=1e-4)
    out = {"case": case, "engines": n, "steps": steps}
    for det in ("0", "1"):
        seen, loss_seen = {}, set()
        for _ in range(n):
            eng = _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2)
            eng.set_option("deterministic", det)
            for k, v in options:
                eng.set_option(k, v)
            rng = np.random.default_rng(4)
            eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
            b = eng.batch(idx, labels)
            losses = [eng.train_step(b, opt) for _ in range(steps)]
            d = hashlib.sha1(eng.get_flat_params().tobytes()).hexdigest()
            seen[d] = seen.get(d, 0) + 1
            loss_seen.add(tuple(losses))
            eng.close()
        out["deterministic=" + det] = {"distinct_parameter_digests": len(seen), "distinct_loss_sequences": len(loss_seen),
                                       "largest_group": max(seen.values())}
    print(json.dumps(out), flush=True)
    assert out["deterministic=1"]["distinct_parameter_digests"] == 1


def step(pps):
    Ve = 2851220
    out = {"paths_per_step": pps}
    for det in ("0", "1"):
        eng = _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2)
        eng.set_option("score_overlap", "1")
        eng.set_option("deterministic", det)
        opt = _ffi.make_opt(method=1, lr=1e-3)
        pool = []
        for i, P in enumerate([1, 2, 3, 4, 5, 8]):
            idx, labels = synth.make_paths(max(1, pps // P), P, T, Ve=Ve, seed=4242 + 13 * i)
            pool.append(eng.batch(idx, labels))

        def one(i):
            b = pool[i % len(pool)]
            eng.forward_async(b, 1)
            eng.train_step(b, opt, 1, want_loss=False)
        for i in range(12):
            one(i)
        eng.sync()
        K = 300
        t0 = time.perf_counter()
        for i in range(K):
            one(i)
        eng.sync()
        wall = time.perf_counter() - t0
        eng.profile_reset(); eng.set_option("profile_filter", ""); eng.profile(True)
        for i in range(60):
            one(i)
        eng.sync(); eng.profile(False)
        fam = {k: round(1e3 * v[0] / 60, 2) for k, v in sorted(eng.profile_get().items(), key=lambda kv: -kv[1][0])}
        out["deterministic=" + det] = {"wall_ms_per_step": round(1e3 * wall / K, 4), "kernel_us_per_step_by_family": fam}
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "digests":
        digests(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    elif len(sys.argv) >= 3 and sys.argv[1] == "step":
        step(int(sys.argv[2]))
    else:
        sys.exit(__doc__)
