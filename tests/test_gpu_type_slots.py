"""-m gpu: SEVERAL TYPE SLOTS per step and unused leading feature columns on every route, against the float64 oracle on the same fp32-rounded parameters.
The cases and the proof that a slot bug cannot hide in them are tests/type_slots_inputs.py (checked on the CPU by tests/test_type_slots_inputs.py); every test
here calls its check() before it runs a case.

  a  every route of tests/test_gpu_gate_extremes.py::ROUTES at (nT, F) = (2, 4) and (3, 6): scores, all class probabilities, loss, every gradient tensor, the
     type_emb / relation_emb gradients row by row, three Adam steps with clipping, the route through the profiler's families.  The families are ROUTES' own,
     changed where a gate on num_types sends the call elsewhere (DESIGN.md "several type slots"): no small-table identity anywhere (embed_scatter runs; no
     gemm_bwd_dw_merged, small_tables_finish, small_tables_fwd), and both bf16 routes on the per-step pipeline, forward AND backward (the persistent BPTT
     launch needs the persistent forward's fragment-order saves: lstm_bf16.hip backward, bptt_persist = act_frag && ...).
     bf16_d64: the scores are compared at their bar but are NO slot check on that route (guard_fwd 0.008 / 0.014 against a bar of 3e-2); the gradient is.
  b  fused, 64-row tiles, a ragged last tile, with and without the identical-prefix plan;  c  16-row tiles with a scoring pass riding in the training step;
  d  ragged batches;  e  option "deterministic";  f  dropout on the summed row;  g  the three ways to feed a batch and the host-pointer calls;
  h  kprn_find_paths on a graph with two type slots per node.

Bars, the project's own: fp32 routes (compute_dtype 0, 2, 3) scores 2e-5 of the largest, probabilities rtol 1e-4, loss 1e-5, every gradient tensor and every
row of the two small tables 2e-4 of the tensor's largest entry, parameters 2e-4 after the steps (the later steps' losses 2e-4, as tests/test_gpu_gate_extremes.py
holds them); bf16 routes (the per-step pipeline's, tests/test_gpu_wide.py) scores 3e-2, probabilities 2e-2 absolute, loss 3e-2, gradients 6e-2.  Every case
prints its measured margins ("MARGINS {...}").

Largest measured margins (MI355X, 55 cases in 8.3 s, the slowest 1.7 s), each as a share of the scale its bar is stated in:
  fp32 routes (45 cases with the ragged, prefix, feed, graph and deterministic ones): scores 9.0e-7 (fused64_noplan_L1-3x6), probabilities 1.5e-7 (ragged), loss
  2.0e-7 (graph_fused), gradient tensors 9.0e-6 (ragged), rows of the two small tables 6.8e-7 (ragged), step losses 1.3e-7 (generic_round1-2x4), parameters after
  the three steps 2.8e-5 (fused64_noplan_L1-2x4): 20 x inside the bars or more, parameters 7 x.
  bf16 routes (4 cases): scores 2.7e-3, probabilities 4.0e-5, loss 3.6e-6 (all bf16_persist_d128_h384-3x6), gradient tensors 8.3e-3 and table rows 4.9e-3
  (bf16_d64-2x4), step losses 2.6e-4, parameters 9.6e-3 (printed only): 7 x inside the bars or more.
  prefix plan against no plan 9.0e-7 (compute_dtype 0) / 1.0e-6 (2) against 1e-5; riding pass: 0 bytes differ, step loss 5.2e-8, parameters 1.3e-7, gradients on the
  stepped parameters 1.2e-6; dropout: loss 6.7e-8, gradients 9.4e-7 (the reference without masks: 0.28 / 0.37 away); host-pointer train step: parameters 1.5e-8
  from the batch path, 3.8e-8 from the oracle; graph cases: step loss 1.7e-7, parameters 2.9e-7; the fused handle's gradient from a fed slot, or from the same
  batch a second time: 41 .. 53 entries differ by 3.7e-11 of the largest."""
import functools
import json

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import make_opt
from tests import dropout_ref as dr
from tests import path_find_ref as pref
from tests import type_slots_inputs as ts

pytestmark = pytest.mark.gpu
STEPS, LR, CLIP = 3, 5e-3, 0.05
AGREE = 1e-5   # two routes to one result: of each tensor's largest entry (tests/test_gpu_parity.py test_embedding_backward_variants_agree)


def engine(c, options=(), **kw):
    dt, de, dr_, H = c.dims
    eng = _ffi.Engine(c.Vt, c.Ve, c.Vr, dt, de, dr_, H, c.L, F=c.F, num_types=c.nT, rnn_type=c.rnn_type, use_relu=c.relu, compute_dtype=c.cdt, **kw)
    for k, v in list(c.options.items()) + list(options):
        eng.set_option(k, v)
    eng.set_flat_params(c.theta.astype(np.float32))
    return eng


def batch_of(eng, c):
    return eng.batch(c.idx, c.labels) if c.counts is None else eng.batch_ragged(c.idx, c.counts, c.labels)


def has(fam, name):
    return any(k.startswith(alt) for alt in name.split("|") for k in fam)


def expected_families(c):
    """ROUTES' families, changed where a gate on num_types says so -> (must run, must not run)"""
    if c.cdt == 1:   # lstm_bf16_persist.hip persist_shape_ok: one type slot only -> the per-step pipeline; no fragment-order saves -> no persistent BPTT, no merged dW
        return (["embed_gather_bf16", "lstm_step_bf16", "lstm_gates_bwd_bf16", "embed_scatter"],
                ["lstm_persist_bf16", "gemm_bwd_dw_merged", "small_tables_finish"])
    fin = list(c.fam_in) + ["embed_scatter"]   # lstm_fused_bwd.hip small_job / generic_pipeline.hip small_tables_route: off
    fout = list(c.fam_out) + ["gemm_bwd_dw_merged", "small_tables_finish", "small_tables_fwd"]
    if c.route is not None and not c.route.startswith("fused"):
        fin.append("embed_gather")
    return fin, fout


def assert_families(fam, fin, fout, m):
    for f in fin:
        assert has(fam, f), (m, f, sorted(fam))
    for f in fout:
        assert not has(fam, f), (m, f, sorted(fam))


def measure(c, eng, b, profile=True):
    """forward, backward, every tensor against the oracle -> (margins, outputs, families)"""
    if profile:
        eng.profile(True)
        eng.profile_reset()
    out = eng.forward(b, 1, want=("probs", "all_probs", "path_scores"))
    loss = eng.backward(b, 1)
    fam = eng.profile_get() if profile else {}
    if profile:
        eng.profile(False)
    g = eng.get_flat_grads().astype(np.float64)
    ps, probs = c.forward()
    ol, og = c.backward()
    bf16 = c.cdt == 1
    m = dict(ts.check(c))
    m.update(score=ts.rel_inf(out["path_scores"], ps),
             probs=float(np.max(np.abs(out["all_probs"] - probs) / (1.0 if bf16 else np.maximum(np.abs(probs), 1e-30)))),
             probs_selected=float(np.max(np.abs(out["probs"] - probs[:, 0]) / (1.0 if bf16 else np.abs(probs[:, 0])))),
             loss=abs(loss - ol) / max(1.0, abs(ol)))
    grads = {nm: ts.rel_inf(g[off:off + int(np.prod(shp))], og[off:off + int(np.prod(shp))]) for nm, (off, shp) in eng.layout().items()}
    m["grad"], m["grad_worst"] = max(grads.values()), max(grads, key=grads.get)
    rows = {}
    for nm in ("type_emb", "relation_emb"):   # row by row: a misplaced row cannot hide in a norm
        ge, go = c.tensor(g, nm), c.tensor(og, nm)
        rows[nm] = (np.max(np.abs(ge - go), axis=1) / np.abs(go).max()).tolist()
    m["rows"] = max(max(v) for v in rows.values())
    m["finite"] = bool(np.all(np.isfinite(out["path_scores"])) and np.all(np.isfinite(out["all_probs"])) and np.isfinite(loss) and np.all(np.isfinite(g)))
    out = dict(out, loss=loss, grads=g, grad_margins=grads, row_margins=rows)
    return m, out, fam


def assert_bars(c, m, out):
    bars = c.bars
    assert m["finite"], m
    assert m["score"] < bars["score"], m
    assert m["probs"] < bars["probs"] and m["probs_selected"] < bars["probs"], m
    assert m["loss"] < bars["loss"], m
    for nm, v in out["grad_margins"].items():
        assert v < bars["grad"], (nm, v, m)
    for nm, v in out["row_margins"].items():
        for r, e in enumerate(v):
            assert e < bars["grad"], (nm, r, e, m)


def adam_steps(c, eng, b, m):
    """three Adam steps with clipping (MyOptimizer.lua:184-218), engine and oracle from the same start"""
    th, st = c.theta.copy(), c.o64.new_state()
    opt, oopt = _ffi.make_opt(method=1, lr=LR, use_grad_clip=1, grad_clip_norm=CLIP), make_opt(method=1, lr=LR, use_grad_clip=1, grad_clip_norm=CLIP)
    losses = []
    for _ in range(STEPS):
        o = c.o64.train_step(th, st, oopt, c.idx, c.labels)[0]
        losses.append((eng.train_step(b, opt), o))
    got = eng.get_flat_params().astype(np.float64)
    m["step_loss"] = [abs(a - o) / max(1.0, abs(o)) for a, o in losses]
    m["params"] = float(np.max(np.abs(got - th)))
    m["moved"] = float(np.max(np.abs(th - c.theta)))
    assert np.all(np.isfinite(got)) and all(np.isfinite(a) for a, _ in losses), m
    assert m["moved"] > 10 * 2e-4, m   # (the steps moved the parameters by far more than the bar they are compared at)
    if c.cdt == 1:
        assert max(m["step_loss"]) < c.bars["loss"], m
    else:
        assert m["step_loss"][0] < c.bars["loss"] and max(m["step_loss"]) < 2e-4, m
        assert m["params"] < c.bars["params"], m


def show(m):
    print("MARGINS " + json.dumps(m))


@pytest.mark.parametrize("name", ts.ROUTE_CASES)
def test_every_route_with_several_type_slots_against_the_f64_oracle(name):
    """bf16_d64: the scores are NO slot check on that route (they hang on the head's bias: a first-slot-only kernel would pass the 3e-2 bar); the type_emb
    gradient, 0.5 of its largest entry away for such a kernel, is."""
    c = ts.case(name)
    eng = engine(c)
    b = batch_of(eng, c)
    m, out, fam = measure(c, eng, b)
    if not m["scores_check_slots"]:
        m["note"] = "scores are no slot check on this route; the type_emb gradient is"
    fin, fout = expected_families(c)
    try:
        adam_steps(c, eng, b, m)
    finally:
        show(m)
        eng.close()
    assert_families(fam, fin, fout, m)
    assert_bars(c, m, out)


@pytest.mark.parametrize("name", ["prefix64_f32", "prefix64_f32x6"])
def test_64_row_tiles_with_a_prefix_and_without_the_plan(name):
    """lstm_fused_prefix.hip's slot loops (layout (3, 6): c0 = 1) on 5 x 64 - 9 paths: with the plan prefix_fwd and prefix_bwd run, with "prefix_plan" 0 they do not;
    both meet the oracle and agree with each other"""
    c = ts.case(name)
    res = {}
    for plan in ("1", "0"):
        eng = engine(c, options=(("small_tiles", "0"), ("prefix_plan", plan)))
        b = batch_of(eng, c)
        m, out, fam = measure(c, eng, b)
        m.update(plan=plan, executed=b.executed_steps)
        show(m)
        eng.close()
        assert has(fam, "lstm_mc_fwd" if c.cdt else "lstm_fused_fwd") and has(fam, "embed_scatter") and not has(fam, "small_tables_finish"), sorted(fam)
        if plan == "1":
            assert "prefix_fwd" in fam and "prefix_bwd" in fam and m["executed"] < c.n_paths * c.idx.shape[2], (m, sorted(fam))
        else:
            assert "prefix_fwd" not in fam and "prefix_bwd" not in fam and m["executed"] == c.n_paths * c.idx.shape[2], (m, sorted(fam))
        assert_bars(c, m, out)
        res[plan] = out
    a, z = res["1"], res["0"]
    agree = {"scores": ts.rel_inf(a["path_scores"], z["path_scores"].astype(np.float64))}
    for nm, (off, shp) in c.o64.layout().items():
        n = int(np.prod(shp))
        agree[nm] = ts.rel_inf(a["grads"][off:off + n], z["grads"][off:off + n])
    print("MARGINS " + json.dumps({"case": name, "plan_vs_noplan": max(agree.values())}))
    for nm, v in agree.items():
        assert v < AGREE, (nm, v)


def test_a_two_slot_scoring_pass_rides_in_a_two_slot_training_step():
    """tests/test_gpu_loss_stage.py test_a_scoring_pass_rides_in_a_training_step with two type slots on both batches: the riding pass's bytes are eng.forward's, and
    the step it rode in has the oracle's loss.  An update clears the gradients, so the step's own gradients cannot be read back: the step is further held only
    through the parameters it leaves (2e-4 after Adam, which normalises the gradient's size: a sign or a dropped entry shows there, a common scale would not), and
    the gradients of the same batch on the stepped parameters by a backward of their own, in which no pass rides"""
    c = ts.case("riding_train")
    ts.check(c)
    theta = c.theta.copy()
    c.o64.zero_pad(theta)   # a training step zeroes the pad rows first: scoring pass and step then see the same parameters
    eng = engine(c, options=(("score_overlap", "1"), ("score_dual", "2"), ("prefix_plan", "0")))
    eng.set_flat_params(theta.astype(np.float32))
    sidx, _ = synth.make_paths(40, 2, 6, F=c.F, Ve=c.Ve, Vr=c.Vr, num_types=c.nT, seed=44)
    sb, tb = eng.batch(sidx), batch_of(eng, c)
    opt, oopt = _ffi.make_opt(method=1, lr=1e-3, entity_update=1), make_opt(method=1, lr=1e-3)
    th, st = theta.copy(), c.o64.new_state()
    eng.train_step(tb, opt)   # (a new engine's first step zeroes the pad rows: a parameter change that places a queued pass ahead of the step)
    c.o64.train_step(th, st, oopt, c.idx, c.labels)
    for step in range(2):
        want = eng.forward(sb, 1)["probs"]
        eng.profile(True)
        eng.profile_reset()
        eng.forward_async(sb, 1)
        loss = eng.train_step(tb, opt)
        got = eng.read_probs(sb.B)
        prof = eng.profile_get()
        eng.profile(False)
        ol = c.o64.train_step(th, st, oopt, c.idx, c.labels)[0]
        m = {"case": "riding", "step": step, "riding_minus_forward": float(np.max(np.abs(got - want))), "loss": abs(loss - ol) / max(1.0, abs(ol)),
             "params": float(np.max(np.abs(eng.get_flat_params() - th)))}
        show(m)
        assert "lstm_fused_fwd_dual" in prof and "loss_stage" in prof and "pool_sigmoid" not in prof and "embed_scatter" in prof, sorted(prof)
        assert got.tobytes() == want.tobytes(), m
        assert m["loss"] < c.bars["loss"] and m["params"] < c.bars["params"], m
    # the gradients of the batch the pass rode on (an update clears them, so they are read from a backward of their own)
    th32 = eng.get_flat_params().astype(np.float64)
    loss = eng.backward(tb, 1)
    g = eng.get_flat_grads().astype(np.float64)
    ol, og = ts.oracle_backward(c.o64, th32, c.idx, c.labels)
    grads = {nm: ts.rel_inf(g[off:off + int(np.prod(shp))], og[off:off + int(np.prod(shp))]) for nm, (off, shp) in eng.layout().items()}
    show({"case": "riding", "after": "steps", "loss": abs(loss - ol) / max(1.0, abs(ol)), "grad": max(grads.values())})
    assert abs(loss - ol) / max(1.0, abs(ol)) < c.bars["loss"]
    for nm, v in grads.items():
        assert v < c.bars["grad"], (nm, v)
    eng.close()


@pytest.mark.parametrize("impl", ["auto", "generic"])
def test_ragged_batch_with_two_type_slots(impl):
    """one pair of 70 paths among 40 pairs (the wave form of the segmented pooling), fused and generic"""
    c = ts.case("ragged")
    assert c.counts.max() == 70 and len(c.counts) == 40
    eng = engine(c, options=(("impl", impl),))
    b = batch_of(eng, c)
    assert b.n_paths == c.n_paths and b.B == 40
    m, out, fam = measure(c, eng, b)
    m["impl"] = impl
    show(m)
    eng.close()
    assert has(fam, "lstm_fused_fwd" if impl == "auto" else "lstm_step_fwd|lstm_gates_fwd") and has(fam, "embed_scatter"), sorted(fam)
    assert not has(fam, "small_tables_finish") and not has(fam, "gemm_bwd_dw_merged"), sorted(fam)
    assert_bars(c, m, out)


def test_deterministic_1_refuses_a_fused_handle_with_two_type_slots():
    """kprn_api.hip det_fused_why: the fused path's general embedding scatter sums with atomics, so "deterministic" = 1 refuses every training call before anything
    is launched or written, and says why"""
    c = ts.case(ts.route_case("fused_small_tiles", 2, 4))
    ts.check(c)
    eng = engine(c)
    b = batch_of(eng, c)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    eng.train_step(b, opt)   # (optimiser state and, an update clears them, gradients that a refused call could disturb)
    eng.backward(b, 1)
    eng.set_option("deterministic", "1")

    def state():
        return [eng.get_flat_params().tobytes(), eng.get_flat_grads().tobytes(), eng.get_flat_opt_state(0).tobytes(), eng.get_flat_opt_state(1).tobytes()]
    before = state()
    assert np.any(np.frombuffer(before[1], np.float32)) and np.any(np.frombuffer(before[3], np.float32))
    for call in (lambda: eng.backward(b, 1), lambda: eng.train_step(b, opt), lambda: eng.train_step_host(c.idx, c.labels, opt)):
        with pytest.raises(_ffi.KprnError) as e:
            call()
        assert e.value.code == _ffi.E_UNSUPPORTED and "deterministic" in e.value.msg and "type slot" in e.value.msg, e.value.msg
        assert state() == before
    assert np.all(np.isfinite(eng.forward(b, 1)["probs"]))   # scoring is never refused
    eng.set_option("deterministic", "0")
    assert np.isfinite(eng.train_step(b, opt))
    assert eng.get_flat_params().tobytes() != before[0]
    eng.close()


@pytest.mark.parametrize("route", ["generic_step_d64", "rnn_relu_step", "wide_persist"])
def test_deterministic_2_with_two_type_slots_three_engines_agree_bit_for_bit(route):
    """the slab form of the one-hot table-gradient product (kernels_basic.hip k_table_grad_mfma<RT, true>) with slots > 1: four steps with clipping and L2 on three
    fresh engines, equal losses, parameters and both Adam slots; the first backward meets the oracle"""
    c = ts.case(ts.route_case(route, 2, 4))
    opt = _ffi.make_opt(method=1, lr=2e-3, regularize=1, use_grad_clip=1, grad_clip_norm=0.05, l2=1e-4)
    runs = []
    for k in range(3):
        eng = engine(c, options=(("deterministic", "2"),))
        b = batch_of(eng, c)
        if k == 0:
            m, out, fam = measure(c, eng, b)
            m["deterministic"] = 2
            show(m)
            assert_families(fam, *expected_families(c), m)
            assert_bars(c, m, out)
        losses = [eng.train_step(b, opt) for _ in range(4)]
        runs.append([np.array(losses, np.float32).tobytes(), eng.get_flat_params().tobytes(), eng.get_flat_opt_state(0).tobytes(), eng.get_flat_opt_state(1).tobytes()])
        assert np.all(np.isfinite(np.frombuffer(runs[-1][1], np.float32)))
        eng.close()
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][1] != c.theta.astype(np.float32).tobytes()


def test_dropout_masks_the_summed_type_row():
    """dropout.hip k_embed_rows_drop with a second slot: the mask falls on the SUM of the slots' rows.  Reference: tests/dropout_ref.py with kprn_host_dropout_keep's
    masks; each step is a backward and an update with lr = 0, so the second step's reference is the same theta with draw 1's masks"""
    p, seed = 0.3, 0x1234567
    c = ts.case(ts.route_case("rnn_relu_step", 2, 4))
    ts.check(c)
    eng = engine(c, options=(("dropout_seed", hex(seed)), ("dropout", repr(p))))
    b = batch_of(eng, c)
    T, N, D = c.idx.shape[2], c.n_paths, sum(c.dims[:3])
    opt = _ffi.make_opt(method=1, lr=0.0, use_grad_clip=0)
    lay = c.o64.layout()
    for draw in range(2):
        eng.profile(True)
        eng.profile_reset()
        loss = eng.backward(b, 1)   # (one training forward = one draw)
        fam = eng.profile_get()
        eng.profile(False)
        g = eng.get_flat_grads().astype(np.float64)
        eng.apply_update(opt)       # (an update clears the gradients: they are read first)
        masks = [_ffi.host_dropout_keep(seed, draw, l, T, N, D if l == 0 else c.dims[3], p) for l in range(c.L)]
        assert 0.6 < masks[0].mean() < 0.8
        rl, rg, _ = dr.forward_backward(lay, c.o64.cfg, c.theta, c.idx, c.labels, masks, dr.scale(p))
        grads = {nm: ts.rel_inf(g[off:off + int(np.prod(shp))], rg[off:off + int(np.prod(shp))]) for nm, (off, shp) in lay.items()}
        plain = ts.rel_inf(c.tensor(c.backward()[1], "type_emb"), c.tensor(rg, "type_emb"))
        m = {"case": "dropout", "draw": draw, "loss": abs(loss - rl) / max(1.0, abs(rl)), "grad": max(grads.values()), "unmasked_reference_at": plain}
        show(m)
        assert "embed_gather_drop" in fam and "embed_gather" not in fam and "embed_scatter" in fam, sorted(fam)
        assert plain > ts.MARGIN * c.bars["grad"], m   # (the masks matter: the reference without them lies far outside the bar)
        assert m["loss"] < c.bars["loss"], m
        for nm, v in grads.items():
            assert v < c.bars["grad"], (nm, v, m)
    assert np.array_equal(eng.get_flat_params(), c.theta.astype(np.float32))
    eng.close()


def _three_ways(c, idx, labels, options=(("small_tiles", "0"),)):
    """(name, engine, batch maker): eng.feed under "feed_build" host and device, and eng.batch"""
    for name, build in (("feed_host", "host"), ("feed_device", "device"), ("batch", None)):
        eng = engine(c, options=tuple(options) + ((("feed_build", build),) if build else ()))
        yield name, eng, (lambda e=eng, f=build: e.feed(idx, labels) if f else e.batch(idx, labels))


@functools.lru_cache(maxsize=None)
def _fed():
    """the case "feed" through the three entry points, once: what each batch holds and what a forward and a backward on it return, as bytes"""
    c = ts.case("feed")
    ts.check(c)
    res = {}
    for name, eng, make in _three_ways(c, c.idx, c.labels):
        b = make()
        out = eng.forward(b, 1, want=("probs", "all_probs", "path_scores"))
        loss = eng.backward(b, 1)
        g = eng.get_flat_grads()
        res[name] = dict(n_uniq=b.n_uniq, executed=b.executed_steps, idx=b.read_idx().tobytes(), probs=out["probs"].tobytes(), all_probs=out["all_probs"].tobytes(),
                         scores=out["path_scores"].tobytes(), loss=np.float32(loss).tobytes(), grads=g.tobytes())
        if name == "batch":
            assert res[name]["idx"] == c.idx.reshape(-1, c.idx.shape[2], c.F).tobytes()
            assert res[name]["executed"] < c.n_paths * c.idx.shape[2]   # (a plan was built: the prefix code ran)
            assert ts.rel_inf(out["path_scores"], c.forward()[0]) < c.bars["score"]
            assert ts.rel_inf(g.astype(np.float64), c.backward()[1]) < c.bars["grad"]
            p2, all2 = eng.forward_host(c.idx, 1)   # kprn_forward on host pointers
            assert np.array_equal(p2, out["probs"]) and np.array_equal(all2, out["all_probs"])
            eng.backward(b, 1)
            res["same_batch_again"] = eng.get_flat_grads().tobytes()
        eng.close()
    return res


def test_three_ways_to_feed_a_two_slot_batch_agree():
    """host_feed.hip's general validation branch and its prefix plan with c0 = F - nT - 2 = 1 (the worker threads, "feed_build" host) against the device build and
    kprn_batch_create: the same index, the same plan, the same bytes out of a forward; kprn_forward on host pointers returns them too"""
    res = _fed()
    for key in ("n_uniq", "executed", "idx", "probs", "all_probs", "scores"):
        assert res["feed_host"][key] == res["batch"][key], ("feed_host", key)
        assert res["feed_device"][key] == res["batch"][key], ("feed_device", key)


def test_three_ways_to_feed_a_two_slot_batch_give_the_same_gradient_bytes():
    """Bytes can only be compared where one batch gives the same bytes twice.  On the fused handle of the test above it does not: with a second slot the type /
    relation gradients leave through embed_scatter, whose sums are atomic (which is why "deterministic" = 1 refuses such a handle) -- measured on an MI355X, the
    SAME batch's second backward differs from its first in 61 entries by up to 7.3e-12 = 3.7e-11 of the largest entry, the host-fed slot in 47 and the
    device-fed slot in 42 entries by the same amount.  So the gradient bytes are compared on a handle whose gradient is bit-reproducible (impl = generic,
    "deterministic" = 2: the slab form of the table-gradient product), where a second backward must return the first one's bytes; on the fused handle the three
    gradients are held to the bar tests/test_gpu_feed.py holds a fed slot to (2e-6 of the largest entry) and the figures are printed"""
    res = _fed()
    diff = {}
    for name in ("feed_host", "feed_device", "same_batch_again"):
        a = np.frombuffer(res[name] if name == "same_batch_again" else res[name]["grads"], np.float32)
        z = np.frombuffer(res["batch"]["grads"], np.float32)
        diff[name] = {"entries": int(np.count_nonzero(a != z)), "max": float(np.max(np.abs(a - z))), "of_largest": float(np.max(np.abs(a - z)) / np.max(np.abs(z)))}
    print("MARGINS " + json.dumps({"case": "feed gradients against eng.batch, fused handle", **diff}))
    for name, d in diff.items():
        assert d["of_largest"] <= 2e-6, (name, d)
    c = ts.case("feed")
    got = {}
    for name, eng, make in _three_ways(c, c.idx, c.labels, options=(("impl", "generic"), ("deterministic", "2"))):
        b = make()
        loss = eng.backward(b, 1)
        got[name] = (np.float32(loss).tobytes(), eng.get_flat_grads().tobytes())
        if name == "batch":
            assert ts.rel_inf(eng.get_flat_grads().astype(np.float64), c.backward()[1]) < c.bars["grad"]
            loss = eng.backward(b, 1)
            assert (np.float32(loss).tobytes(), eng.get_flat_grads().tobytes()) == got[name]   # (this handle's bits are reproducible)
        eng.close()
    assert got["feed_host"] == got["batch"] and got["feed_device"] == got["batch"]


@pytest.mark.parametrize("bad", ["Vt+1", "0"])
def test_a_bad_id_in_the_last_type_slot_only_is_refused_alike(bad):
    c = ts.case("feed")
    idx = c.idx.copy()
    idx[7, 1, 5, c.F - 3] = c.Vt + 1 if bad == "Vt+1" else 0   # the last type slot of a real step; every other column stays valid
    codes = {}
    for name, eng, make in _three_ways(c, idx, c.labels):
        with pytest.raises(_ffi.KprnError) as e:
            eng.forward(make(), 1)   # (a fed slot reports at its first use)
        codes[name] = e.value.code
        good = eng.batch(c.idx, c.labels)
        assert np.all(np.isfinite(eng.forward(good, 1)["probs"]))   # the handle goes on
        eng.close()
    assert codes == {"feed_host": _ffi.E_INDEX, "feed_device": _ffi.E_INDEX, "batch": _ffi.E_INDEX}, codes


def test_host_pointer_train_step_agrees_with_the_batch_path():
    c = ts.case("feed")
    opt = _ffi.make_opt(method=1, lr=1e-3)
    got = []
    for host in (True, False):
        eng = engine(c)
        loss = eng.train_step_host(c.idx, c.labels, opt) if host else eng.train_step(eng.batch(c.idx, c.labels), opt)
        got.append((loss, eng.get_flat_params()))
        eng.close()
    th, st = c.theta.copy(), c.o64.new_state()
    ol = c.o64.train_step(th, st, make_opt(method=1, lr=1e-3), c.idx, c.labels)[0]
    m = {"case": "train_step_host", "loss_vs_batch": abs(got[0][0] - got[1][0]), "params_vs_batch": float(np.max(np.abs(got[0][1] - got[1][1]))),
         "loss": abs(got[0][0] - ol) / max(1.0, abs(ol)), "params": float(np.max(np.abs(got[0][1] - th)))}
    show(m)
    assert m["loss_vs_batch"] < 1e-6 * max(1.0, abs(ol)) and m["params_vs_batch"] < 2e-6, m   # (tests/test_gpu_feed.py: a few fp32 atomics in the embedding backward)
    assert m["loss"] < c.bars["loss"] and m["params"] < c.bars["params"], m


@pytest.mark.parametrize("name", ["graph_fused", "graph_rnn"])
def test_paths_found_on_a_two_slot_graph_train_like_the_oracle(name):
    """kprn_graph_create with node_types [Ve, 2]: kprn_find_paths writes both slots of every node (and the unused leading column of the rnn shape), row for row what
    kprn_host_find_paths writes; one training step on the found batch"""
    c = ts.case(name)
    ts.check(c)
    g, nt, pairs, labels = ts.graph()
    eng = engine(c)
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    lo, hi, cap, T = c.find_args
    batch, counts, _ = eng.find_paths(gr, pairs, lo, hi, cap, T, labels=labels)
    assert np.array_equal(counts[counts > 0], c.counts) and batch.n_paths == c.n_paths and batch.has_labels
    assert np.array_equal(batch.read_idx(), c.idx)
    m, out, fam = measure(c, eng, batch)
    show(m)
    assert has(fam, "embed_scatter") and not has(fam, "small_tables_finish"), sorted(fam)
    assert_bars(c, m, out)
    # one Adam step against okprn_train_step restated in numpy on the oracle's summed per-group gradient (as tests/test_gpu_ragged.py does: zero the pad rows,
    # gradient, Adam, zero the pad rows); the oracle's own train_step takes rectangular batches only
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    th = c.theta.copy()
    eng.set_flat_params(th.astype(np.float32))
    loss = eng.train_step(batch, _ffi.make_opt(method=1, lr=lr, regularize=0))
    c.o64.zero_pad(th)
    ol, og = ts.oracle_backward(c.o64, th, c.idx, c.labels, c.counts)
    want = th - lr * np.sqrt(1.0 - b2) / (1.0 - b1) * ((1.0 - b1) * og / (np.sqrt((1.0 - b2) * og * og) + eps))
    c.o64.zero_pad(want)
    got = eng.get_flat_params().astype(np.float64)
    m2 = {"case": name, "step_loss": abs(loss - ol) / max(1.0, abs(ol)), "params": float(np.max(np.abs(got - want))), "moved": float(np.max(np.abs(want - c.theta)))}
    show(m2)
    eng.close()
    assert m2["step_loss"] < c.bars["loss"] and m2["params"] < c.bars["params"] and m2["moved"] > 4 * c.bars["params"], m2
