"""-m gpu: every route that depends on the NUMBER OF ROWS of the type and relation tables, at the edges of its predicate and with every table row live.

The routes place relation v at one-hot column v and type v at column Vr + v, ids 1-based:
  fused D = H = 64: forward identity (lstm_fused_fwd.hip fwd_body IDENT) and BPTT identity (lstm_fused_bwd.hip bwd_body IDENT, kk::small_tables_finish) while
  Vt + Vr <= 16; one-hot MFMAs inside the bottom BPTT launch ("fused_small_tables") or the passenger job of the entity-gradient launch (bidx::SmallGrad) while
  Vt <= 16 and Vr <= 16; the scatter kernel above; generic fp32: merged dW over [S | x_e] while roundup4(Vr + Vt) <= dt (generic_pipeline.hip small_tables_route);
  bf16: merged dW while Vt + Vr <= 128 (lstm_bf16.hip).
The rest of the suite runs them at Vt = 6, Vr in {9, 100} on synth.make_paths inputs, which never draw type Vt nor relation Vr - 2 (the #UNK rows): the last
one-hot column, a full 16-row accumulator tile and both sides of every cut-off were never live.  Here the inputs come from tests/vocab_inputs.py
paths_every_id (every id 1..Vt / 1..Vr; tests/test_small_table_vocab_inputs.py shows on the CPU that every table row then carries at least 1e-2 of its
tensor's largest gradient entry, 50 x the bar below), T = 6, parameters from Oracle.init_params rounded to fp32.

fp32 routes against the float64 oracle, the suite's own bars (tests/test_gpu_gate_extremes.py): path scores 2e-5 of the largest, all 46 class
probabilities rtol 1e-4, loss 1e-5, every gradient tensor 2e-4 of its largest entry, everything finite.  Two routes over the same sums: 2e-5 of each tensor's
largest (tests/test_gpu_fused_identity.py); "small_tables" = 0 leaves the forward bit-identical.  bf16: the bars of tests/test_gpu_persist.py, imported; merged
dW against the dx route 2e-5 as test_small_table_gradients_from_the_merged_dw_product_match_the_dx_route.  The route of every case is asserted through the
profiler's kernel families: a case that quietly takes another route fails.  Every case prints its measured maxima ("MARGINS {...}") and runs under a time
limit of its own (a hung launch ends the process instead of the session's patience).

Measured maxima (MI355X; no case failed, no kernel or predicate had to change):
  fused, against the oracle (14 cases + the passenger job): path scores 9.8e-7 of the largest, probabilities 1.4e-7, loss 7.2e-8, gradients 7.1e-7 of each
    tensor's largest (type_emb 3.0e-7, relation_emb 2.6e-7);
  fused (7, 9), "small_tables_fwd" on against off: scores 4.7e-7, probabilities 1.6e-7, gradients 3.2e-7; "small_tables" on against off: forward bit-identical,
    gradients 3.2e-7; (16, 16) passenger job against the in-launch one-hot MFMAs: forward bit-identical, gradients 2.7e-7;
  generic, against the oracle (7 cases): scores 3.5e-7, probabilities 1.5e-7, loss 1.0e-7, gradients 2.0e-6 (type_emb 4.9e-7, relation_emb 2.7e-7); merged dW
    against the dx route: forward bit-identical, gradients 1.8e-6;
  bf16, against the oracle: scores 1.40e-3 (rms 3.3e-4), probabilities 7.6e-6 absolute, loss 1.4e-6, gradients 2.09e-3 (rms 4.9e-4, cosine >= 0.999997); merged
    dW against the dx route at 128 rows: 1.3e-6.
That the cases can fail was tried once with a library carrying four off-by-ones (is_t = arow < Vr + Vt - 1 in the forward's Q rows; one workgroup fewer in
k_small_tables_finish_f32; Vt < 16 in small_job; Vt + Vr < 128 in the bf16 predicate): the 16 cases at those edges failed, the 10 others passed."""
import faulthandler
import json
import sys

import numpy as np
import pytest

from kprn_amd import _ffi
from tests import vocab_inputs as vi
from tests.test_gpu_persist import GRAD_COS, GRAD_MAX, GRAD_RMS, GRAD_SIGN, LOSS_REL, PROB_ABS, SCORE_MAX, SCORE_RMS, direction, rel_rms

pytestmark = pytest.mark.gpu
CASE_LIMIT_S = 120   # a case takes a few seconds, the float64 oracle included


@pytest.fixture(autouse=True)
def _time_limit_per_case():
    """a launch that never returns cannot be interrupted from Python: the watchdog thread prints every thread's stack and ends the process"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


def rel_inf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(1e-30, float(np.max(np.abs(b))))


def _vid(v):
    return v if isinstance(v, str) else f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None


def _engine(c, opts, compute_dtype=0):
    dt, de, dr, H = c.dims
    eng = _ffi.Engine(c.Vt, c.Ve, c.Vr, dt, de, dr, H, c.L, rnn_type=c.rnn_type, use_relu=1, param_init=c.init, compute_dtype=compute_dtype)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_flat_params(c.theta.astype(np.float32))
    return eng


def _pass(eng, b):
    """one forward + backward under the profiler -> outputs, loss, gradients, the kernel families that ran"""
    eng.profile_reset()
    eng.profile(True)
    out = eng.forward(b, 1, want=("path_scores", "all_probs"))
    loss = eng.backward(b, 1)
    fam = eng.profile_get()
    eng.profile(False)
    return {"scores": out["path_scores"].copy(), "probs": out["all_probs"].copy(), "loss": loss, "grads": eng.get_flat_grads().astype(np.float64), "fam": fam}


def _run(c, opts, compute_dtype=0):
    eng = _engine(c, opts, compute_dtype)
    r = _pass(eng, eng.batch(c.idx, c.labels))
    r["lay"] = eng.layout()
    eng.close()
    return r


def _tensors(lay, *flats):
    for nm, (off, shp) in lay.items():
        n = int(np.prod(shp))
        yield (nm,) + tuple(f[off:off + n] for f in flats)


def _check_fp32_against_oracle(c, r, tag):
    """the fp32 bars of the module docstring; prints the measured maxima first"""
    ps, probs = c.forward()
    ol, og = c.backward()
    assert r["probs"].shape == probs.shape == (c.idx.shape[0], 46)
    grads = {nm: rel_inf(got, want) for nm, got, want in _tensors(r["lay"], r["grads"], og)}
    m = {"case": tag, "score": rel_inf(r["scores"], ps), "probs": float(np.max(np.abs(r["probs"] - probs) / np.maximum(np.abs(probs), 1e-30))),
         "loss": abs(r["loss"] - ol) / max(1.0, abs(ol)), "grad": max(grads.values()), "type_emb": grads["type_emb"], "relation_emb": grads["relation_emb"]}
    print("MARGINS " + json.dumps(m))
    assert np.all(np.isfinite(r["scores"])) and np.all(np.isfinite(r["probs"])) and np.isfinite(r["loss"]) and np.all(np.isfinite(r["grads"])), m
    assert m["score"] < 2e-5, m
    np.testing.assert_allclose(r["probs"], probs, rtol=1e-4)
    assert m["loss"] < 1e-5, m
    for nm, v in grads.items():
        assert v < 2e-4, (nm, v, m)


def _check_same_sums(r1, r0, tag, forward_bitwise):
    """two routes over the same sums: 2e-5 of each tensor's largest"""
    grads = {nm: rel_inf(a, b) for nm, a, b in _tensors(r1["lay"], r1["grads"], r0["grads"])}
    m = {"case": tag, "score_ab": rel_inf(r1["scores"], r0["scores"]), "probs_ab": rel_inf(r1["probs"], r0["probs"]),
         "loss_ab": abs(r1["loss"] - r0["loss"]) / max(1.0, abs(r0["loss"])), "grad_ab": max(grads.values())}
    print("MARGINS " + json.dumps(m))
    if forward_bitwise:
        assert np.array_equal(r1["scores"], r0["scores"]) and np.array_equal(r1["probs"], r0["probs"]) and r1["loss"] == r0["loss"], m
    assert m["score_ab"] < 2e-5 and m["probs_ab"] < 2e-5 and m["loss_ab"] < 2e-5, m
    for nm, v in grads.items():
        assert v < 2e-5, (nm, v, m)


# ---- (a) fused D = H = 64 ----------------------------------------------------------------------------------------------------------------
def _fused_route(fam, Vt, Vr, tiles, tag):
    assert any(k.startswith("lstm_fused_fwd") for k in fam) and "lstm_fused_bwd" in fam, (tag, sorted(fam))
    if Vt + Vr <= 16:      # both identities; the BPTT one on 64-path tiles only
        assert "small_tables_fwd" in fam, (tag, sorted(fam))
        assert ("small_tables_finish" in fam) == (tiles == "0"), (tag, sorted(fam))
        assert "embed_scatter" not in fam, (tag, sorted(fam))
    elif Vt <= 16 and Vr <= 16:   # the one-hot MFMAs inside the bottom launch / the passenger job
        assert "small_tables_fwd" not in fam and "small_tables_finish" not in fam and "embed_scatter" not in fam, (tag, sorted(fam))
    else:                  # a table above the small-job limit: the scatter kernel
        assert "embed_scatter" in fam, (tag, sorted(fam))
        assert "small_tables_fwd" not in fam and "small_tables_finish" not in fam, (tag, sorted(fam))


@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("vocab", vi.FUSED_VOCABS, ids=_vid)
def test_fused_vocabulary_edges_against_the_f64_oracle(vocab, tiles):
    """Vt + Vr = 16 (column 15 = the last type row; the relation / type split in the middle and at both ends), 17 (identities off), 16 + 16 (both accumulator
    tiles full), 17 rows in either table (scatter kernel) -- on 64-path tiles ("small_tiles" 0) and on 16-row tiles (1)"""
    Vt, Vr = vocab
    c = vi.case("fused64", Vt, Vr)
    tag = ["fused64", Vt, Vr, "tiles" + tiles]
    r = _run(c, {"small_tiles": tiles})
    _fused_route(r["fam"], Vt, Vr, tiles, tag)
    _check_fp32_against_oracle(c, r, tag)


def test_fused_full_accumulator_tiles_through_the_passenger_job():
    """(16, 16) with "fused_small_tables" = 0: on 64-path tiles the table gradients come from the passenger job of the entity-gradient launch (bidx::SmallGrad)"""
    c = vi.case("fused64", 16, 16)
    tag = ["fused64", 16, 16, "tiles0", "passenger"]
    r = _run(c, {"small_tiles": "0", "fused_small_tables": "0"})
    _fused_route(r["fam"], 16, 16, "0", tag)
    _check_fp32_against_oracle(c, r, tag)
    _check_same_sums(r, _run(c, {"small_tiles": "0"}), tag + ["vs in-launch"], forward_bitwise=True)


@pytest.mark.parametrize("tiles", ["0", "1"])
def test_fused_identities_on_against_off_with_sixteen_live_columns(tiles):
    """(7, 9), the same batch: "small_tables_fwd" = 0 (full-row forward) and "small_tables" = 0 (dx route in the BPTT; the forward must not notice)"""
    c = vi.case("fused64", 7, 9)
    on = _run(c, {"small_tiles": tiles})
    _fused_route(on["fam"], 7, 9, tiles, ["on", tiles])
    fwd_off = _run(c, {"small_tiles": tiles, "small_tables_fwd": "0"})
    assert "small_tables_fwd" not in fwd_off["fam"] and ("small_tables_finish" in fwd_off["fam"]) == (tiles == "0"), sorted(fwd_off["fam"])
    _check_same_sums(on, fwd_off, ["fused64", 7, 9, "tiles" + tiles, "small_tables_fwd on/off"], forward_bitwise=False)
    bwd_off = _run(c, {"small_tiles": tiles, "small_tables": "0"})
    assert "small_tables_fwd" in bwd_off["fam"] and "small_tables_finish" not in bwd_off["fam"] and "embed_scatter" not in bwd_off["fam"], sorted(bwd_off["fam"])
    _check_same_sums(on, bwd_off, ["fused64", 7, 9, "tiles" + tiles, "small_tables on/off"], forward_bitwise=True)


# ---- (b) generic fp32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,vocab,on_route", vi.GENERIC_VOCABS, ids=_vid)
def test_generic_merged_dw_at_and_above_ns_equal_dt(shape, vocab, on_route):
    """"impl" = generic: ns = roundup4(Vr + Vt) <= dt takes the merged dW over [S | x_e] (ns = dt: no pad column, the selectors cover the whole type slice; 61 rows:
    three pad columns), one step above takes the dx product and the table-gradient launches"""
    Vt, Vr = vocab
    c = vi.case(shape, Vt, Vr)
    tag = [shape, Vt, Vr]
    r = _run(c, {"impl": "generic"})
    fam = r["fam"]
    assert not any(k.startswith("lstm_fused") for k in fam), sorted(fam)
    if on_route:
        assert "small_tables_finish" in fam and "gemm_bwd_dw_merged" in fam and "embed_scatter" not in fam, (tag, sorted(fam))
    else:
        assert "small_tables_finish" not in fam and "gemm_bwd_dw_merged" not in fam and "embed_scatter" in fam, (tag, sorted(fam))
    _check_fp32_against_oracle(c, r, tag)
    if on_route:
        off = _run(c, {"impl": "generic", "small_tables": "0"})
        assert "embed_scatter" in off["fam"] and "small_tables_finish" not in off["fam"], sorted(off["fam"])
        _check_same_sums(r, off, tag + ["small_tables on/off"], forward_bitwise=True)


# ---- (c) bf16, configs[3] shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,vocab,on_route", vi.BF16_VOCABS, ids=_vid)
def test_bf16_merged_dw_at_128_rows_and_above(shape, vocab, on_route):
    """Vt + Vr = 128 exactly fills the 128 one-hot columns of the merged dW product (lstm_bf16.hip k_onehot_T / k_small_tables_finish); 129 rows take the dx route.
    Against the oracle the bf16 bars of tests/test_gpu_persist.py; at 128 rows also against "bf16_small_tables" = 0 on the same engine and batch (the same dA: fp32
    reordering only, 2e-5 of each tensor's largest -- the bar that can see a single row)."""
    Vt, Vr = vocab
    c = vi.case(shape, Vt, Vr)
    tag = [shape, Vt, Vr]
    eng = _engine(c, {}, compute_dtype=1)
    b = eng.batch(c.idx, c.labels)
    r = _pass(eng, b)
    r["lay"] = eng.layout()
    fam = r["fam"]
    if on_route:
        assert "small_tables_finish" in fam and "gemm_bwd_dw_merged" in fam, (tag, sorted(fam))
        eng.set_option("bf16_small_tables", "0")
        off = _pass(eng, b)
        assert "small_tables_finish" not in off["fam"] and "gemm_bwd_dw_merged" not in off["fam"], sorted(off["fam"])
    else:
        assert "small_tables_finish" not in fam and "gemm_bwd_dw_merged" not in fam, (tag, sorted(fam))
    eng.close()
    ps, probs = c.forward()
    ol, og = c.backward()
    grads = {nm: (rel_inf(got, want), rel_rms(got, want)) + direction(got, want) for nm, got, want in _tensors(r["lay"], r["grads"], og)}
    m = {"case": tag, "score": rel_inf(r["scores"], ps), "score_rms": rel_rms(r["scores"], ps), "probs_abs": float(np.max(np.abs(r["probs"][:, 0] - probs[:, 0]))),
         "loss": abs(r["loss"] - ol) / max(1.0, abs(ol)), "grad": max(v[0] for v in grads.values()), "grad_rms": max(v[1] for v in grads.values()),
         "grad_cos": min(v[2] for v in grads.values()), "type_emb": grads["type_emb"][0], "relation_emb": grads["relation_emb"][0]}
    if on_route:
        ab = {nm: rel_inf(a, d) for nm, a, d in _tensors(r["lay"], r["grads"], off["grads"])}
        m["grad_ab"] = max(ab.values())
    print("MARGINS " + json.dumps(m))
    assert np.all(np.isfinite(r["scores"])) and np.all(np.isfinite(r["probs"])) and np.isfinite(r["loss"]) and np.all(np.isfinite(r["grads"])), m
    assert m["score"] < SCORE_MAX and m["score_rms"] < SCORE_RMS, m
    np.testing.assert_allclose(r["probs"][:, 0], probs[:, 0], atol=PROB_ABS)
    assert m["loss"] < LOSS_REL, m
    for nm, (mx, rms, cos, sign) in grads.items():
        assert mx < GRAD_MAX and rms < GRAD_RMS, (nm, mx, rms, m)
        assert cos > GRAD_COS and sign >= GRAD_SIGN, (nm, cos, sign, m)
    if on_route:
        assert r["loss"] == off["loss"], m
        for nm, v in ab.items():
            assert v < 2e-5, (nm, v, m)
