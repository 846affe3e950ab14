"""Helper of tests/test_gpu_adam_transitions.py: a SCRIPT of optimiser events run on one engine.

A script is a list of events (ev(...)): training steps with their own kprn_opt, scoring passes, reads and writes of parameters and optimiser state, checkpoints.
The same script runs on engine L (entity_update as the script says, 0 by default: lazy-exact rows), on engine D (entity_update = 1 at every step: the dense sweep
of optim.adam) and on L0 (L without the events that only read).  Option "deterministic" is set first, so that the gradients are a function of the parameters only
and every comparison can be np.array_equal.  Nothing here asserts a tolerance: the bar is bit identity, which follows from the one adam_elem all routes share."""
import os

import numpy as np

from kprn_amd import _ffi, synth

T = 6
VE = 50
PAD = VE - 1                                  # the pad row, 0-based
FUSED = (6, VE, 9, 16, 32, 16, 64, 1)         # D = H = 64: the fused path; rows of 32 floats (G = 8)
READS = ("score", "score_host", "read_rows", "read_state", "read_table", "save", "zero_pad", "check")   # what L0 leaves out


def generic(de):
    """the generic fp32 pipeline (H = 32 is not the fused path's): de = 64 (G = 16), 128 (G = 32), anything else the scalar row kernel"""
    return (6, VE, 9, 16, de, 16, 32, 1)


def ev(kind, *args, expect=None, **kw):
    """expect: {profile family: True (launched) / False (absent)} for this event on engine L"""
    return dict(kind=kind, args=args, expect=expect or {}, **kw)


def step(batch, expect=None, tag=None, **opt):
    return ev("step", batch, expect=expect, tag=tag, opt=opt)


def refused_step(batch, **opt):
    """a training step the library must refuse with KPRN_E_ARG, before it launches or writes anything"""
    return ev("refused_step", batch, opt=opt)


def make_batch(n_pairs, P, seed, lo, width, pads=True):
    """synth.make_paths(..., Ve=50) with its real entity ids folded into ids lo .. lo + width - 1; pad steps keep id Ve (pads=False: full-length paths, no pad)"""
    idx, labels = synth.make_paths(n_pairs, P, T, Ve=VE, seed=seed, real_len=None if pads else T)
    idx = idx.copy()
    e = idx[..., 1]
    real = e < VE
    e[real] = lo + (e[real] - 1) % width
    assert e.min() >= 1 and e.max() <= VE
    return idx, labels


def rows_of(batch):
    return np.unique(batch[0][..., 1]) - 1    # 0-based rows of entity_emb


def four_batches(n_pairs=40, P=2):
    """A, B, C: row sets that overlap only partly (ids 1-20, 11-30, 21-38, each with pad steps); E: ids 39-49, which the others never use, and no pad step"""
    return [make_batch(n_pairs, P, 31, 1, 20), make_batch(n_pairs, P, 32, 11, 20), make_batch(n_pairs, P, 33, 21, 18),
            make_batch(n_pairs, P, 34, 39, 11, pads=False)]


CYCLE = (0, 1, 2, 3, 1, 2, 3)   # A B C E B C E: the rows only A has coast for six steps, the pad row coasts through every E


def cycle(k):
    """the batch of step k (1-based)"""
    return CYCLE[(k - 1) % len(CYCLE)]


# ---- what the idx arrays alone say about a script -------------------------------------------------------------------------------------------------------
def coasting(script, batches, min_gap):
    """[(row, step it was last touched, step it returns)] for every stretch of >= min_gap consecutive steps a row sits out between two touches"""
    steps = [e for e in script if e["kind"] == "step"]
    touched = np.zeros((len(steps) + 1, VE), bool)
    for k, e in enumerate(steps, 1):
        touched[k, rows_of(batches[e["args"][0]])] = True
    out = []
    for r in range(VE):
        ks = np.flatnonzero(touched[:, r])
        out += [(r, int(a), int(b)) for a, b in zip(ks[:-1], ks[1:]) if b - a - 1 >= min_gap]
    return out


def snap_steps(script, batches):
    return sorted({s for _, a, b in coasting(script, batches, 5) for s in (a, b - 1)})


def assert_not_vacuous(script, batches, d_result):
    """at least 8 real rows coast for >= 5 steps and return; the pad row is touched, coasts and returns; in D's trajectory those rows moved while they coasted"""
    gaps = [g for g in coasting(script, batches, 5) if g[0] != PAD]
    assert len({r for r, _, _ in gaps}) >= 8, sorted({r for r, _, _ in gaps})
    assert [g for g in coasting(script, batches, 1) if g[0] == PAD], "the pad row never coasts"
    snaps = d_result["snaps"]
    for r, a, b in gaps:
        assert np.any(snaps[a][r] != snaps[b - 1][r]), (r, a, b)    # momentum moved the row: a replay that did nothing would show


# ---- running one ---------------------------------------------------------------------------------------------------------------------------------------
def theta0(n):
    return (np.random.default_rng(4).random(n) * 0.2 - 0.1).astype(np.float32)


def run(shape, script, batches, mode, det="1", options=(), tmp=None, snaps=()):
    """mode "L" / "D" / "L0".  -> dict(state = [parameters, slot 0, slot 1], losses, reads = [every array a read returned], checks, snaps = {step: entity_emb},
    prof = {event number: families}).  tmp: the folder of the checkpoints (save writes <tmp>/<mode>_<tag>.bin, load reads D's)."""
    eng = _ffi.Engine(*shape)
    eng.set_option("deterministic", det)
    for k, v in options:
        eng.set_option(k, v)
    th0 = theta0(eng.n_params)
    eng.set_flat_params(th0)
    bs = [eng.batch(i, l) for i, l in batches]
    res = dict(losses=[], reads=[], checks=[], snaps={}, prof={}, plans=[b.executed_steps < b.n_paths * T for b in bs])
    n_steps = 0

    def state():
        return [eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1)]
    for n, e in enumerate(script):
        kind, a = e["kind"], e["args"]
        if mode == "L0" and kind in READS:
            continue
        profiled = bool(e["expect"])
        if profiled:
            eng.profile(True)
            eng.profile_reset()
        if kind == "step":
            kw = dict(e["opt"])
            if mode == "D":
                kw["entity_update"] = 1
            res["losses"].append(eng.train_step(bs[a[0]], _ffi.make_opt(**kw)))
            n_steps += 1
            if mode == "D" and n_steps in snaps:
                res["snaps"][n_steps] = eng.get_param("entity_emb")     # (the dense engine has nothing pending: a plain copy)
        elif kind == "refused_step":
            kw = dict(e["opt"], entity_update=1) if mode == "D" else e["opt"]
            for call in (lambda: eng.train_step(bs[a[0]], _ffi.make_opt(**kw)), lambda: eng.train_step_host(*batches[a[0]], _ffi.make_opt(**kw)),
                         lambda: eng.apply_update(_ffi.make_opt(**kw))):
                try:
                    call()
                except _ffi.KprnError as ex:
                    assert ex.code == _ffi.E_ARG and "opt.method changed" in ex.msg and "slot 0" in ex.msg, (ex.code, ex.msg)
                else:
                    raise AssertionError("a change of opt.method was not refused")
        elif kind == "score":
            res["reads"].append(eng.forward(bs[a[0]], 1)["probs"])
        elif kind == "score_host":
            res["reads"] += list(eng.forward_host(batches[a[0]][0], 1))
        elif kind == "read_rows":
            res["reads"].append(eng.get_param_rows("entity_emb", a[0]))
        elif kind == "read_state":
            res["reads"].append(eng.get_flat_opt_state(a[0]))
        elif kind == "read_table":
            res["reads"].append(eng.get_param("entity_emb"))
        elif kind == "save":
            path = os.path.join(tmp, f"{mode}_{a[0]}.bin")
            eng.save(path)
            res["reads"].append(np.fromfile(path, np.uint8))
        elif kind == "zero_pad":
            eng.zero_pad_tokens()
        elif kind == "check":
            res["checks"].append(state())
        elif kind == "write_rows":
            rows = np.asarray(a[0], np.int64)
            vals = (np.random.default_rng(a[1]).random((len(rows), shape[4])) * 0.2 - 0.1).astype(np.float32)
            eng.set_param_rows("entity_emb", rows, vals)
        elif kind == "write_flat":
            eng.set_flat_params(th0 + (np.random.default_rng(a[0]).random(th0.size) * 0.02 - 0.01).astype(np.float32))
        elif kind == "load":
            eng.load(os.path.join(tmp, f"D_{a[0]}.bin"))
        else:
            raise ValueError(kind)
        if profiled:
            fam = eng.profile_get()
            eng.profile(False)
            res["prof"][n] = fam
            if mode == "L":
                for name, want in e["expect"].items():
                    assert (fam.get(name, (0.0, 0))[1] > 0) == want, (n, kind, name, want, sorted(fam))
    res["state"] = state()
    res["losses"] = np.array(res["losses"], np.float32)
    eng.close()
    return res


def assert_same(a, b, reads=True):
    for name, x, y in zip(("parameters", "optimiser slot 0", "optimiser slot 1"), a["state"], b["state"]):
        assert np.array_equal(x, y), (name, int(np.sum(x != y)), float(np.max(np.abs(x.astype(np.float64) - y))))
        assert np.all(np.isfinite(x)) and np.any(x != 0), name
    assert np.array_equal(a["losses"], b["losses"]), np.flatnonzero(a["losses"] != b["losses"])[:5]
    assert np.all(np.isfinite(a["losses"])) and len(a["losses"]) > 0
    if not reads:
        return
    assert len(a["reads"]) == len(b["reads"]) and len(a["checks"]) == len(b["checks"])
    for k, (x, y) in enumerate(zip(a["reads"], b["reads"])):
        assert np.array_equal(x, y), ("read", k, int(np.sum(x != y)))
    for k, (ca, cb) in enumerate(zip(a["checks"], b["checks"])):
        for x, y in zip(ca, cb):
            assert np.array_equal(x, y), ("checkpoint", k, int(np.sum(x != y)))


def run_all(shape, script, batches, det="1", options=(), tmp=None):
    """D (with the table snapshots the non-vacuity statement needs), L, and L0 where the script reads; every comparison of the method"""
    d = run(shape, script, batches, "D", det, options, tmp, snaps=snap_steps(script, batches))
    assert_not_vacuous(script, batches, d)
    lz = run(shape, script, batches, "L", det, options, tmp)
    assert_same(lz, d)
    if any(e["kind"] in READS for e in script):
        l0 = run(shape, script, batches, "L0", det, options, tmp)
        assert_same(lz, l0, reads=False)     # the reads disturbed nothing
    return lz, d


# ---- the run across the growth of the step-size table ---------------------------------------------------------------------------------------------------
def long_script():
    """4 100 steps.  A at steps 1-3, B (disjoint rows, no pad step) at 4 .. 4 097, a scoring pass over A, A at 4 098, B, A.  The table of step sizes starts at
    4 096 entries and grows at step 4 095: A's rows and the pad row replay steps 4 .. 4 097, entries from both sides of the growth, first in the catch-up launch
    of the scoring pass and -- on L0, which has no scoring pass -- in the row update of step 4 098"""
    opt = dict(method=1, lr=2e-3)
    s = [step(0, **opt) for _ in range(3)] + [step(1, **opt) for _ in range(4094)]
    s.append(ev("score", 0, expect={"adam_rows_catchup": True, "adam_flush_all": False}))
    s += [step(0, **opt), step(1, **opt), step(0, **opt)]
    return s


def long_batches():
    """4 pairs x 1 path: a step is latency-bound"""
    return [make_batch(4, 1, 41, 1, 16), make_batch(4, 1, 42, 20, 25, pads=False)]


def long_run(with_l0=True):
    script, batches = long_script(), long_batches()
    assert sum(e["kind"] == "step" for e in script) == 4100 and script[4097]["kind"] == "score"
    assert len(np.intersect1d(rows_of(batches[0]), rows_of(batches[1]))) == 0 and PAD in rows_of(batches[0])
    d = run(FUSED, script, batches, "D", snaps=snap_steps(script, batches))
    assert_not_vacuous(script, batches, d)
    assert all(b - a - 1 == 4094 for _, a, b in coasting(script, batches, 5))
    lz = run(FUSED, script, batches, "L")
    assert_same(lz, d)
    if with_l0:
        assert_same(lz, run(FUSED, script, batches, "L0"), reads=False)
    return lz, d
