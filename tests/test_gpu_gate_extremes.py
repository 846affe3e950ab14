"""-m gpu: every recurrent-cell route with SATURATED gates and LARGE inputs, against the float64 oracle on the same fp32-rounded parameters.
The rest of the suite draws its parameters at the init scale, where every gate pre-activation sits within about +-20; a trained model or a loaded
checkpoint (kprn_load, set_param) goes far beyond, which is where the hand-written gate math (kprn_amd/csrc/gate_math.h) parts from libm.
  R1 "gate bands": in every layer and every gate block, every third unit's bias is a ladder over [-130, -92], the next unit's over [+92, +130]
     (rnn-relu: the negative band only); the data-dependent part of each pre-activation spreads a bias over thousands of distinct arguments.
     Asserted from theta: the whole negative band stays below -88.73 (sum |W| max|x| + sum |U| max|h|), where exp_fast once turned into NaN.
  R2 "large inputs": the table rows the batch uses scaled to |x| up to 40 (rnn-relu: identity init, so h grows to hundreds).
In both, out.weight is shrunk until the oracle's pooled scores stay within +-15 (beyond, the final sigmoid saturates and the literal BCE's
fp32 and f64 answers legitimately part).  Each case: scores, all 46 class probabilities, loss, every gradient tensor, 5 Adam steps with
clipping, all finite; the route asserted through the profiler's kernel families.  Bars: the suite's own (fp32 routes: scores 2e-5 of the
largest, probabilities rtol 1e-4, loss 1e-5, gradients 2e-4 of each tensor's largest, parameters 2e-4 after the steps); bf16 routes in R1
the score and gradient bars the suite holds each to (tests/test_gpu_persist.py, tests/test_gpu_wide.py), in R2 finiteness and direction only.  Every case prints its measured margins ("MARGINS {...}")."""
import json

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import Oracle, make_cfg, make_opt
from tests.test_gpu_persist import GRAD_COS, GRAD_MAX, GRAD_RMS, GRAD_SIGN, SCORE_MAX, SCORE_RMS, direction, rel_rms

pytestmark = pytest.mark.gpu
VE, VR, STEPS, LR = 900, 9, 5, 5e-3
NEG_LIMIT = -88.73   # below -128 ln2 = -88.7228: where sigm's exp_fast(-x) overflowed


def rel_inf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(1e-30, np.max(np.abs(b))))


# name: (kind, (dt, de, dr, H), L, pairs, P, T, engine kwargs, options, families that must run, families that must not)
ROUTES = {
    "fused64_plan_L2": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {}, {"small_tiles": "0"}, ["lstm_fused_fwd"], ["lstm_step_fwd", "lstm_gates_fwd"]),
    "fused64_noplan_L1": ("lstm", (16, 32, 16, 64), 1, 100, 3, 6, {}, {"small_tiles": "0", "prefix_plan": "0"}, ["lstm_fused_fwd"], ["lstm_step_fwd", "lstm_gates_fwd"]),
    "fused_small_tiles": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {}, {"small_tiles": "1"}, ["lstm_fused_fwd"], ["lstm_step_fwd", "lstm_gates_fwd"]),
    "fused_f32x6": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {"compute_dtype": 2}, {}, ["lstm_mc_fwd"], ["lstm_step_fwd", "lstm_gates_fwd"]),
    "fused_f32x3": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {"compute_dtype": 3}, {}, ["lstm_mc_fwd"], ["lstm_step_fwd", "lstm_gates_fwd"]),
    "generic_step_d64": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {}, {"impl": "generic"}, ["lstm_step_fwd"], ["lstm_fused_fwd"]),
    "generic_round1": ("lstm", (16, 32, 16, 64), 2, 40, 3, 6, {}, {"impl": "generic"}, ["lstm_gates_fwd"], ["lstm_step_fwd", "lstm_fused_fwd"]),
    "wide_step": ("lstm", (64, 64, 64, 192), 2, 100, 3, 4, {}, {"persist_layers": "0"}, ["lstm_step_fwd"], ["lstm_layer_fwd"]),
    "wide_persist": ("lstm", (64, 64, 64, 192), 2, 100, 3, 4, {}, {"persist_layers": "2"}, ["lstm_layer_fwd", "lstm_layer_bwd"], ["lstm_step_fwd"]),
    "lstm_config_sh": ("lstm", (50, 100, 50, 250), 1, 75, 2, 6, {}, {"persist_layers": "2"}, ["lstm_layer_fwd", "lstm_layer_bwd"], ["lstm_step_fwd"]),
    "rnn_tanh_step": ("rnn", (32, 32, 32, 96), 1, 100, 3, 6, {"use_relu": 0}, {"persist_layers": "0"}, ["rnn_step_fwd"], ["rnn_layer_fwd"]),
    "rnn_tanh_persist": ("rnn", (32, 32, 32, 96), 2, 100, 3, 6, {"use_relu": 0}, {"persist_layers": "2"}, ["rnn_layer_fwd", "rnn_layer_bwd"], ["rnn_step_fwd"]),
    "rnn_relu_step": ("rnn", (32, 32, 32, 96), 1, 100, 3, 6, {"use_relu": 1}, {"persist_layers": "0"}, ["rnn_step_fwd"], ["rnn_layer_fwd"]),
    "rnn_relu_persist": ("rnn", (32, 32, 32, 96), 1, 100, 3, 6, {"use_relu": 1}, {"persist_layers": "2"}, ["rnn_layer_fwd", "rnn_layer_bwd"], ["rnn_step_fwd"]),
    "gru_small_batch_d_ne_h": ("gru", (16, 32, 16, 128), 1, 40, 3, 6, {}, {"persist_layers": "0"}, ["gru_cell_fwd"], ["gru_layer_fwd"]),
    "gru_persist_d_ne_h": ("gru", (16, 32, 16, 128), 1, 100, 3, 6, {}, {"persist_layers": "2"}, ["gru_layer_fwd", "gru_layer_bwd"], ["gru_cell_fwd"]),
    "gru_persist_L2": ("gru", (32, 64, 32, 128), 2, 100, 3, 6, {}, {"persist_layers": "2"}, ["gru_layer_fwd", "gru_layer_bwd"], ["gru_cell_fwd"]),   # (L > 1 needs D = H)
    "bf16_d64": ("lstm", (16, 32, 16, 64), 2, 100, 3, 6, {"compute_dtype": 1}, {}, ["lstm_step_bf16|lstm_persist_bf16"], []),
    "bf16_persist_d128_h384": ("lstm", (128, 128, 128), 1, 129, 2, 4, {"compute_dtype": 1}, {}, ["lstm_persist_bf16"], []),
}


def _blocks(kind, l):
    """gate blocks of layer l: (bias name, number of gate blocks in it, [(input weight, recurrent weight) of block q])"""
    if kind == "lstm":
        return [(f"lstm{l}.i2g.bias", 4, [(f"lstm{l}.i2g.weight", f"lstm{l}.o2g.weight")] * 4)]
    if kind == "gru":
        return [(f"gru{l}.i2g.bias", 2, [(f"gru{l}.i2g.weight", f"gru{l}.o2g.weight")] * 2),
                (f"gru{l}.c_i2h.bias", 1, [(f"gru{l}.c_i2h.weight", f"gru{l}.c_h2h.weight")])]
    return [(f"rnn{l}.i2h.bias", 1, [(f"rnn{l}.i2h.weight", f"rnn{l}.h2h.weight")])]


def _view(theta, lay, nm):
    off, shp = lay[nm]
    return theta[off:off + int(np.prod(shp))].reshape(shp)


def _xmax(theta, lay, idx):
    """largest |x| the batch feeds the bottom layer: the rows of the three tables it uses"""
    m = 0.0
    for k, nm in enumerate(("type_emb", "entity_emb", "relation_emb")):
        rows = np.unique(idx[..., k].ravel()) - 1
        m = max(m, float(np.max(np.abs(_view(theta, lay, nm)[rows]))))
    return m


def _scale_rows(theta, lay, idx, target=40.0):
    """R2: the table rows the batch uses, scaled so that the largest |x| is `target`"""
    s = target / _xmax(theta, lay, idx)
    for k, nm in enumerate(("type_emb", "entity_emb", "relation_emb")):
        rows = np.unique(idx[..., k].ravel()) - 1
        _view(theta, lay, nm)[rows] *= s


def _bands(theta, lay, kind, L, relu, idx, T):
    """R1: bias ladders in every gate block; the weights of the negative-band rows shrunk (if need be) so that the data-dependent part
    cannot lift any of them above NEG_LIMIT.  Returns the largest pre-activation bound over the negative band."""
    worst = -np.inf
    hmax = 1.0   # |h| of a tanh / sigmoid-gated cell
    xmax = _xmax(theta, lay, idx)
    for l in range(1, L + 1):
        xin = xmax if l == 1 else hmax
        for bname, nb, wts in _blocks(kind, l):
            bias = _view(theta, lay, bname)
            H = bias.size // nb
            neg, pos = np.arange(0, H, 3), np.arange(1, H, 3)
            for q in range(nb):
                b = bias[q * H:(q + 1) * H]
                b[neg] = np.linspace(-130.0, -92.0, len(neg))
                if not relu:
                    b[pos] = np.linspace(92.0, 130.0, len(pos))
                W, U = _view(theta, lay, wts[q][0])[q * H:(q + 1) * H], _view(theta, lay, wts[q][1])[q * H:(q + 1) * H]
                extra = np.abs(_view(theta, lay, f"rnn{l}.h2h.bias")) if kind == "rnn" else np.zeros(H)
                if kind == "rnn" and relu:
                    hmax = _relu_hmax(theta, lay, l, xin, T)
                bound = np.abs(W).sum(1) * xin + np.abs(U).sum(1) * hmax + extra
                shrink = np.minimum(1.0, 3.0 / np.maximum(bound[neg], 1e-30))
                W[neg] *= shrink[:, None]
                U[neg] *= shrink[:, None]
                bound = np.abs(W).sum(1) * xin + np.abs(U).sum(1) * hmax + extra
                worst = max(worst, float(np.max(b[neg] + bound[neg])))
    return worst


def _relu_hmax(theta, lay, l, xin, T):
    """an upper bound of h over T steps of a ReLU rnn layer (h >= 0): h_t <= max(0, sum |W| x + b_i2h + b_h2h + sum |U| h_{t-1})"""
    W, U = _view(theta, lay, f"rnn{l}.i2h.weight"), _view(theta, lay, f"rnn{l}.h2h.weight")
    b = _view(theta, lay, f"rnn{l}.i2h.bias") + _view(theta, lay, f"rnn{l}.h2h.bias")
    h = 0.0
    for _ in range(T):
        h = max(0.0, float(np.max(np.abs(W).sum(1) * xin + b + np.abs(U).sum(1) * h)))
    return max(h, 1e-30)


def _case(route, regime, seed=11):
    kind, dims, L, pairs, P, T, kw, opts, fam_in, fam_out = ROUTES[route]
    if len(dims) == 3:
        dims = dims + (384,)
    dt, de, dr, H = dims
    rt = {"lstm": 0, "rnn": 1, "gru": 2}[kind]
    relu = kw.get("use_relu", 1) if kind == "rnn" else 0   # (a ReLU rnn only)
    cdt = kw.get("compute_dtype", 0)
    o64 = Oracle(make_cfg(Vt=6, Ve=VE, Vr=VR, dt=dt, de=de, dr=dr, H=H, L=L, rnn_type=rt, use_relu=relu if kind == "rnn" else 1), np.float64)
    lay = o64.layout()
    idx, labels = synth.make_paths(pairs, P, T, Ve=VE, Vr=VR, seed=seed + pairs)
    init = 0.05
    theta = o64.init_params(seed, init, rnn_init=(regime == "R2" and kind == "rnn" and relu == 1))
    info = {"route": route, "regime": regime}
    if regime == "R1":
        info["neg_band_bound"] = _bands(theta, lay, kind, L, relu, idx, T)
        assert info["neg_band_bound"] < NEG_LIMIT, info
    else:
        _scale_rows(theta, lay, idx)
    if kind == "rnn":
        o64.zero_pad(theta)   # pad embeddings zero -> MaskZero masks the pad steps
    theta = theta.astype(np.float32).astype(np.float64)
    for _ in range(4):   # shrink the head until the pooled scores stay out of the final sigmoid's saturation
        m = float(np.max(np.abs(o64.forward(theta, idx)[1])))
        if m <= 12.0:
            break
        _view(theta, lay, "out.weight")[:] *= 10.0 / m
        theta = theta.astype(np.float32).astype(np.float64)
    info["pooled_max"] = float(np.max(np.abs(o64.forward(theta, idx)[1])))
    assert info["pooled_max"] <= 15.0, info
    eng = _ffi.Engine(6, VE, VR, dt, de, dr, H, L, rnn_type=rt, use_relu=relu if kind == "rnn" else 1, compute_dtype=cdt)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_flat_params(theta.astype(np.float32))
    return eng, o64, theta, idx, labels, info, fam_in, fam_out


def _families(fam, fam_in, fam_out, info):
    for f in fam_in:
        assert any(k.startswith(alt) for alt in f.split("|") for k in fam), (info, f, sorted(fam))
    for f in fam_out:
        assert not any(k.startswith(f) for k in fam), (info, f, sorted(fam))


def _run(route, regime):
    eng, o64, theta, idx, labels, info, fam_in, fam_out = _case(route, regime)
    cdt = ROUTES[route][6].get("compute_dtype", 0)
    bf16 = cdt == 1
    b = eng.batch(idx, labels)
    executed = b.executed_steps
    eng.profile(True)
    out = eng.forward(b, 1, want=("probs", "all_probs", "path_scores"))
    loss = eng.backward(b, 1)
    fam = eng.profile_get()
    g = eng.get_flat_grads().astype(np.float64)
    ps, _, probs = o64.forward(theta, idx)
    ol, og, _ = o64.forward_backward(theta, idx, labels)
    finite = {"scores": bool(np.all(np.isfinite(out["path_scores"]))), "all_probs": bool(np.all(np.isfinite(out["all_probs"]))),
              "loss": bool(np.isfinite(loss)), "grads": bool(np.all(np.isfinite(g)))}
    info.update(score=rel_inf(out["path_scores"], ps), score_rms=rel_rms(out["path_scores"], ps),
                probs=float(np.max(np.abs(out["all_probs"] - probs) / np.maximum(np.abs(probs), 1e-30))),
                probs_abs=float(np.max(np.abs(out["all_probs"] - probs))), loss=abs(loss - ol) / max(1.0, abs(ol)))
    grads = {}
    for nm, (off, shp) in eng.layout().items():
        n = int(np.prod(shp))
        got, want = g[off:off + n], og[off:off + n]
        cos, sign = direction(got, want)
        grads[nm] = (rel_inf(got, want), rel_rms(got, want), cos, sign)
    info["grad"] = max(v[0] for v in grads.values())
    info["grad_cos"] = min(v[2] for v in grads.values())
    # five Adam steps with clipping (MyOptimizer.lua:184-218), engine and oracle from the same start
    th, st = theta.copy(), o64.new_state()
    opt, oopt = _ffi.make_opt(method=1, lr=LR, use_grad_clip=1), make_opt(method=1, lr=LR, use_grad_clip=1)
    step_loss = []
    for _ in range(STEPS):
        o = o64.train_step(th, st, oopt, idx, labels)[0]
        step_loss.append((eng.train_step(b, opt), o))
    got = eng.get_flat_params().astype(np.float64)
    finite["steps"] = bool(all(np.isfinite(a) for a, _ in step_loss)) and bool(np.all(np.isfinite(got)))
    info["step_loss"] = max(abs(a - o) / max(1.0, abs(o)) for a, o in step_loss)
    info["params"] = float(np.max(np.abs(got - th)))
    walk = [direction(got[off:off + int(np.prod(shp))] - theta[off:off + int(np.prod(shp))], th[off:off + int(np.prod(shp))] - theta[off:off + int(np.prod(shp))],
                      floor=0.25) for off, shp in eng.layout().values()]
    info["walk_cos"] = min(c for c, _ in walk)
    info["finite"] = finite
    print("MARGINS " + json.dumps(info))
    eng.close()

    assert all(finite.values()), info
    _families(fam, fam_in, fam_out, info)
    if route == "fused_small_tiles":
        assert executed == idx.shape[0] * idx.shape[1] * idx.shape[2], info   # 16-row tiles: no identical-prefix plan
    if not bf16:
        assert info["score"] < 2e-5, info
        np.testing.assert_allclose(out["all_probs"], probs, rtol=1e-4)
        assert info["loss"] < 1e-5, info
        for nm, v in grads.items():
            assert v[0] < 2e-4, (nm, v, info)
        assert info["step_loss"] < 2e-4, info
        assert info["params"] < 2e-4, info
    elif regime == "R1" and route.startswith("bf16_persist"):   # fp32 biases added: the score and gradient bars of tests/test_gpu_persist.py
        assert info["score"] < SCORE_MAX and info["score_rms"] < SCORE_RMS, info           # (loss, probabilities: printed only)
        for nm, (mx, rms, cos, sign) in grads.items():
            assert mx < GRAD_MAX and rms < GRAD_RMS and cos > GRAD_COS and sign >= GRAD_SIGN, (nm, mx, rms, cos, sign, info)
    elif regime == "R1":   # the per-step bf16 pipeline: the bars tests/test_gpu_wide.py holds it to (scores 3e-2, gradients 6e-2) and its direction
        assert info["score"] < 3e-2, info                                                   # (measured: 2.6e-4, 7.1e-3, cosine 0.99997)
        for nm, (mx, rms, cos, sign) in grads.items():
            assert mx < 6e-2 and cos > 0.9999 and sign >= GRAD_SIGN, (nm, mx, rms, cos, sign, info)
    else:                  # bf16 at large inputs: finite (above) and every gradient pointing the oracle's way (measured cosine >= 0.9995)
        for nm, (mx, rms, cos, sign) in grads.items():
            assert cos > 0.999 and sign >= GRAD_SIGN, (nm, mx, rms, cos, sign, info)


@pytest.mark.parametrize("regime", ["R1", "R2"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_saturated_gates_and_large_inputs_against_the_f64_oracle(route, regime):
    _run(route, regime)


def test_f32x3_operands_at_nine_tenths_of_the_fp16_range():
    """compute_dtype = 3 pre-scales its fp16 pieces by fixed powers of two (kprn_amd/csrc/lstm_fused_fwd_mc.hip McFmt<2>): W_o2g and the top
    layer's W_i2g by 2^8 (x -2 log2e on the g rows: |W| <= 88.7, i / f / o rows 177), the bottom layer's W_i2g by 2^4 (1419 / 2838), the table
    rows by 2^4 (4094).  At 0.9 x those limits every output stays finite; every gate saturates there, so no fp32 bar is promised (the
    distance to the oracle is printed)."""
    eng, o64, theta, idx, labels, info, fam_in, fam_out = _case("fused_f32x3", "R2")
    lay = o64.layout()
    H, L = o64.cfg.H, o64.cfg.L
    rng = np.random.default_rng(5)
    lim = {"o2g": (88.7, 177.4), "top": (88.7, 177.4), "bottom": (1419.0, 2838.0)}
    for l in range(1, L + 1):
        for nm, which in ((f"lstm{l}.o2g.weight", "o2g"), (f"lstm{l}.i2g.weight", "bottom" if l == 1 else "top")):
            W = _view(theta, lay, nm)
            g_lim, ifo_lim = lim[which]
            for q in range(4):
                W[q * H:(q + 1) * H] = rng.uniform(-0.9, 0.9, W[q * H:(q + 1) * H].shape) * (g_lim if q == 1 else ifo_lim)
    _scale_rows(theta, lay, idx, target=0.9 * 4094.0)
    theta = theta.astype(np.float32).astype(np.float64)
    for _ in range(4):
        m = float(np.max(np.abs(o64.forward(theta, idx)[1])))
        if m <= 12.0:
            break
        _view(theta, lay, "out.weight")[:] *= 10.0 / m
        theta = theta.astype(np.float32).astype(np.float64)
    eng.set_flat_params(theta.astype(np.float32))
    b = eng.batch(idx, labels)
    eng.profile(True)
    out = eng.forward(b, 1, want=("probs", "all_probs", "path_scores"))
    loss = eng.backward(b, 1)
    assert any(k.startswith("lstm_mc_fwd") for k in eng.profile_get()), sorted(eng.profile_get())
    g = eng.get_flat_grads()
    opt = _ffi.make_opt(method=1, lr=LR, use_grad_clip=1)
    losses = [eng.train_step(b, opt) for _ in range(STEPS)]
    ps, _, probs = o64.forward(theta, idx)
    print("MARGINS " + json.dumps({"route": "f32x3_range", "score": rel_inf(out["path_scores"], ps),
                                   "probs_abs": float(np.max(np.abs(out["all_probs"] - probs)))}))
    for v in (out["path_scores"], out["all_probs"], g, eng.get_flat_params(), np.array([loss] + losses)):
        assert np.all(np.isfinite(v))
    eng.close()
