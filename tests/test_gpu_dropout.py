"""-m gpu: option "dropout" (nn.Dropout on the rnn cell's step input) against tests/dropout_ref.py -- a float64 autograd restatement of the
graph that takes the masks, and a numpy twin of the documented generator that rebuilds them without asking the engine.

Bars: the project's own for the rnn generic pipeline against float64 (tests/test_gpu_parity.py): loss within 1e-5 max(1, |loss|), every gradient tensor within
2e-4 of its largest entry.  tests/test_dropout_host.py asserts on the CPU that the float64 reference with the right masks lies further than the gradient bar
from the one with no masks (every tensor) and from the one with a single flipped element (some tensor).  Shapes: Vt 6, Ve 300, Vr 9,
dt / de / dr 8 / 24 / 16, H 48, 37 x 3 paths, T 6 unless a case needs another; every route is asserted through the profiler's kernel families.  Every case
prints its measured maxima ("MARGINS {...}").

The persistent forward launch (rnn_layer_fwd) needs the step kernel's 256 paths even with persist_layers = 2, so the route case that asks for it runs at
300 paths; at 111 paths persist_layers = 2 gives the persistent BPTT launch (rnn_layer_bwd) behind the per-step forward, and that case is kept too.

Measured maxima (MI355X, 16 cases in 2.85 s): loss 2.0e-7 of the bar's scale (the identity's return, no dropout), gradients 1.30e-6 of a tensor's largest
entry (rnn1.i2h.weight on the step / persistent routes at 300 paths; width 50: 8.4e-7, width 49: 1.25e-6): 50 and 150 times inside the bars; the mask patterns
equal bit for bit at both depths."""
import faulthandler
import functools
import json
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, model, synth
from tests import dropout_ref as dr

pytestmark = pytest.mark.gpu
SEED = 0x1234567
LOSS_REL, GRAD_RTOL = 1e-5, 2e-4


@pytest.fixture(autouse=True)
def _time_limit_per_case():
    faulthandler.dump_traceback_later(120, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def case(relu, L, dims=(8, 24, 16, 48), pairs=37):
    return dr.Case(relu, L, dims=dims, pairs=pairs)


@functools.lru_cache(maxsize=None)
def reference(relu, L, dims, pairs, seed, draw, p):
    return case(relu, L, dims, pairs).reference(seed, draw, p)


def engine(c, p=None, seed=SEED, opts=(), **kw):
    dt, de, dr_, H = c.dims
    eng = _ffi.Engine(c.Vt, c.Ve, c.Vr, dt, de, dr_, H, c.L, rnn_type=1, use_relu=c.relu, param_init=0.35, **kw)
    eng.set_flat_params(c.theta.astype(np.float32))
    for k, v in opts:
        eng.set_option(k, v)
    if seed is not None:
        eng.set_option("dropout_seed", hex(seed))
    if p is not None:
        eng.set_option("dropout", repr(p))
    return eng


def check(c, loss, grads, ref, tag):
    rl, rg, _ = ref
    worst = {nm: dr.rel_inf(g, w) for nm, g, w in c.tensors(grads, rg)}
    m = {"case": tag, "loss": abs(loss - rl) / max(1.0, abs(rl)), "grad": max(worst.values()), "worst": max(worst, key=worst.get)}
    print("MARGINS " + json.dumps(m))
    assert np.isfinite(loss) and np.all(np.isfinite(grads)), m
    assert m["loss"] < LOSS_REL, m
    for nm, v in worst.items():
        assert v < GRAD_RTOL, (nm, v, m)


def profiled_backward(eng, b):
    eng.profile_reset()
    eng.profile(True)
    loss = eng.backward(b, 1)
    fam = eng.profile_get()
    eng.profile(False)
    return loss, fam


@pytest.mark.parametrize("relu,L", [(1, 1), (0, 1), (1, 2), (0, 2)])
def test_parity_with_the_masked_reference(relu, L):
    c = case(relu, L)
    eng = engine(c, 0.25)
    loss = eng.backward(eng.batch(c.idx, c.labels), 1)
    check(c, loss, eng.get_flat_grads(), reference(relu, L, c.dims, 37, SEED, 0, 0.25), f"parity relu={relu} L={L}")
    eng.close()


@pytest.mark.parametrize("route", ["gemm_cell", "step", "persist_bwd", "persist"])
def test_every_forward_and_backward_route(route):
    pairs = 100 if route in ("step", "persist") else 37   # 300 paths: the step kernel's 256 and more
    c = case(0, 2, pairs=pairs)
    eng = engine(c, 0.25, opts=(("persist_layers", "2" if route.startswith("persist") else "0" if route == "step" else "1"),))
    loss, fam = profiled_backward(eng, eng.batch(c.idx, c.labels))
    print(route, sorted(fam))
    assert "embed_gather_drop" in fam and "embed_gather" not in fam and fam["drop_rows_fwd"][1] == 1 and fam["drop_rows_bwd"][1] == 2, sorted(fam)
    if route == "gemm_cell":
        assert "gemm_i2g_fwd" in fam and "rnn_cell_fwd" in fam and "rnn_cell_bwd" in fam and "rnn_step_fwd" not in fam and "rnn_layer_fwd" not in fam, sorted(fam)
    elif route == "step":
        assert "rnn_step_fwd" in fam and "rnn_layer_fwd" not in fam and "rnn_cell_fwd" not in fam and "rnn_cell_bwd" in fam, sorted(fam)
    elif route == "persist_bwd":
        assert "rnn_layer_bwd" in fam and "rnn_cell_bwd" not in fam, sorted(fam)
    else:
        assert "rnn_layer_fwd" in fam and "rnn_layer_bwd" in fam and "rnn_step_fwd" not in fam and "rnn_cell_bwd" not in fam, sorted(fam)
    check(c, loss, eng.get_flat_grads(), reference(0, 2, c.dims, pairs, SEED, 0, 0.25), "route " + route)
    eng.close()


def test_row_width_not_a_multiple_of_four():
    """D = H = 50: the gather moves half quads (a quad straddles the type / entity cut at 10 and the entity / relation cut at 36), the row kernel and the
    backward scaling run on 8-byte pieces, and the last quad of every row is partial"""
    dims = (10, 26, 14, 50)
    c = case(0, 2, dims=dims)
    eng = engine(c, 0.5)
    loss = eng.backward(eng.batch(c.idx, c.labels), 1)
    check(c, loss, eng.get_flat_grads(), reference(0, 2, dims, 37, SEED, 0, 0.5), "width 50")
    eng.close()


def test_odd_row_width():
    """9 / 25 / 15, H = 49: odd slice widths and an odd row pitch, so the gather, the row kernel and the backward scaling move one element at a time (the
    last branch of both VEC dispatches); D = H = 49 leaves one element in the last quad"""
    dims = (9, 25, 15, 49)
    c = case(0, 2, dims=dims)
    eng = engine(c, 0.5)
    loss = eng.backward(eng.batch(c.idx, c.labels), 1)
    check(c, loss, eng.get_flat_grads(), reference(0, 2, dims, 37, SEED, 0, 0.5), "width 49")
    eng.close()


def test_the_small_table_identity_steps_aside():
    dims = (16, 16, 16, 48)   # roundup4(Vt + Vr) = 16 <= dt: the identity's shape
    c = case(0, 1, dims=dims)
    eng = engine(c)
    b = eng.batch(c.idx, c.labels)
    loss, fam = profiled_backward(eng, b)
    assert "gemm_bwd_dw_merged" in fam and "embed_scatter" not in fam, sorted(fam)
    eng.set_option("dropout", "0.25")
    loss, fam = profiled_backward(eng, b)
    assert "gemm_i2g_bwd_dx" in fam and "embed_scatter" in fam and "gemm_bwd_dw_merged" not in fam and "drop_rows_bwd" in fam, sorted(fam)
    check(c, loss, eng.get_flat_grads(), reference(0, 1, dims, 37, SEED, 0, 0.25), "identity off")
    eng.set_option("dropout", "0")
    loss, fam = profiled_backward(eng, b)
    assert "gemm_bwd_dw_merged" in fam and "embed_scatter" not in fam and not any(k.startswith("drop_") or k == "embed_gather_drop" for k in fam), sorted(fam)
    ol, og, _ = c.oracle.forward_backward(c.theta, c.idx, c.labels)
    check(c, loss, eng.get_flat_grads(), (ol, og, None), "identity back")
    eng.close()


@pytest.mark.parametrize("L", [1, 2])
def test_the_mask_itself_bit_for_bit(L):
    """every entity id is used once, so row id - 1 of the entity table's gradient is one (path, step)'s dx slice: its zero pattern IS the mask.
    (The input seed was picked on the float64 reference alone, so that its smallest kept entry clears the 1e-5 guard below for both depths: 5.1e-4 and
    4.3e-5 of the largest; seeds 5 .. 13 give 1.2e-6 .. 4.3e-5 at two layers.)"""
    Vt, Ve, Vr, B, P, T = 6, 300, 9, 20, 2, 3
    rng = np.random.default_rng(7)
    N = B * P
    idx = np.empty((B, P, T, 3), np.int32)
    idx[..., 0] = rng.integers(1, Vt - 1, size=(B, P, T))          # 1 .. Vt - 2
    idx[..., 1] = (rng.permutation(Ve - 2)[:N * T] + 1).reshape(B, P, T)   # 1 .. Ve - 2, each once
    idx[..., 2] = rng.integers(1, Vr - 2, size=(B, P, T))          # 1 .. Vr - 3
    labels = (rng.random(B) < 0.5).astype(np.float32)
    c = dr.Case(0, L, idx=idx, labels=labels)
    dt, de = c.dims[0], c.dims[1]
    keep = dr.keep_mask(SEED, 0, 0, T, N, sum(c.dims[:3]), 0.5)[:, :, dt:dt + de]   # [T, N, de]
    ids = idx[..., 1].reshape(N, T)

    def rows(flat):
        off, shp = c.lay["entity_emb"]
        g = np.asarray(flat)[off:off + shp[0] * shp[1]].reshape(shp)
        return np.stack([g[ids[:, t] - 1] for t in range(T)])   # [T, N, de]

    ref = rows(c.reference(SEED, 0, 0.5)[1])
    assert np.array_equal(ref != 0, keep)
    assert not keep.all(axis=2).any() and keep.any(axis=2).all()
    assert np.abs(ref[keep]).min() > 1e-5 * np.abs(ref).max()   # (fp32 cannot round a kept entry to zero)
    eng = engine(c, 0.5)
    eng.backward(eng.batch(idx, labels), 1)
    got = rows(eng.get_flat_grads())
    assert np.array_equal(got != 0, keep), int(((got != 0) != keep).sum())
    assert np.array_equal(eng.get_grad("entity_emb").reshape(Ve, de)[ids[:, 0] - 1] != 0, keep[0])
    eng.close()


def test_draw_counts_training_forwards():
    c = dr.Case(0, 2)
    c.oracle.zero_pad(c.theta)   # (a training step zeroes the pad rows before its forward)
    ref = [c.reference(SEED, d, 0.25) for d in range(3)]
    eng = engine(c, 0.25)
    b = eng.batch(c.idx, c.labels)
    l0 = eng.backward(b, 1)
    check(c, l0, eng.get_flat_grads(), ref[0], "draw 0")
    l1 = eng.backward(b, 1)
    check(c, l1, eng.get_flat_grads(), ref[1], "draw 1")
    assert l1 != l0
    eng.set_option("dropout_seed", hex(SEED))
    assert eng.backward(b, 1) == l0   # the same seed from draw 0 again: the first call's loss, bit for bit
    opt = _ffi.make_opt(method=1, lr=0.0, regularize=0)   # (the parameters stay: the next step's reference is the same theta)
    lt = eng.train_step(b, opt)
    lh = eng.train_step_host(c.idx, c.labels, opt)
    m = {"train_step": abs(lt - ref[1][0]), "train_step_host": abs(lh - ref[2][0])}
    print("MARGINS " + json.dumps(m))
    assert m["train_step"] < LOSS_REL * max(1.0, abs(ref[1][0])) and m["train_step_host"] < LOSS_REL * max(1.0, abs(ref[2][0])), m
    eng.close()
    # the default seed is the configuration's seed + rank
    e2 = _ffi.Engine(c.Vt, c.Ve, c.Vr, *c.dims, c.L, rnn_type=1, use_relu=0, seed=4242, rank=1, world=2)
    e2.set_flat_params(c.theta.astype(np.float32))
    e2.set_option("dropout", "0.25")
    ld = e2.backward(e2.batch(c.idx, c.labels), 1, inv_batch=1.0 / c.B)
    rd = c.reference(4243, 0, 0.25)[0]
    assert abs(ld - rd) < LOSS_REL * max(1.0, abs(rd)), (ld, rd)
    e2.close()


def test_scoring_is_untouched():
    c = case(0, 2)
    plain = engine(c, seed=None)
    want = plain.forward(plain.batch(c.idx), 1)["probs"].copy()
    plain.close()
    eng = engine(c, 0.5)
    before = eng.forward(eng.batch(c.idx), 1)["probs"].copy()
    eng.backward(eng.batch(c.idx, c.labels), 1)
    after = eng.forward(eng.batch(c.idx), 1)["probs"].copy()
    eng.close()
    assert np.array_equal(before, want) and np.array_equal(after, want)


FLAGS = ("-entityTypeVocabSize 6 -entityVocabSize 500 -relationVocabSize 9 -entityTypeEmbeddingDim 16 -entityEmbeddingDim 32 -relationEmbeddingDim 16 "
         "-numFeatureTemplates 3 -numEntityTypes 1 -rnnType rnn -rnnHidSize 64 -numLayers 2 -topK 2 -useAdam 1 -learningRate 0.01 -regularize 0 -includeEntity 1")


def test_refusals_and_the_flags_end_to_end():
    for kw in (dict(rnn_type=0), dict(rnn_type=2), dict(rnn_type=1, compute_dtype=1)):
        eng = _ffi.Engine(6, 300, 9, 16, 16, 16, 48, 1, **kw)
        with pytest.raises(_ffi.KprnError) as e:
            eng.set_option("dropout", "0.3")
        assert e.value.code == _ffi.E_UNSUPPORTED, kw
        eng.set_option("dropout", "0")
        eng.close()
    eng = _ffi.Engine(6, 300, 9, 16, 16, 16, 48, 1, rnn_type=1)
    for key, bad in [("dropout", v) for v in ("1", "-0.1", "abc", " 0.3", "0x0.8", "0.3 ", "nan", "")] + \
                    [("dropout_seed", v) for v in ("-1", " -1", " 7", "+7", "0x", "7g", "18446744073709551616", "")]:
        with pytest.raises(_ffi.KprnError) as e:
            eng.set_option(key, bad)
        assert e.value.code == _ffi.E_ARG, (key, bad)
    for key, good in (("dropout", "2.5e-1"), ("dropout", ".25"), ("dropout_seed", "0X1f"), ("dropout_seed", "010"), ("dropout_seed", "18446744073709551615")):
        eng.set_option(key, good)
    eng.close()
    p = model.parse_flags((FLAGS + " -useDropout 1 -dropout 0.3 -dropoutSeed 77").split())
    eng = model.build_engine(p)
    idx, labels = synth.make_paths(16, 3, 6, Vt=6, Ve=500, Vr=9, seed=8)
    c = dr.Case(1, 2, dims=(16, 32, 16, 64), Ve=500, idx=idx, labels=labels)
    c.theta = eng.get_flat_params().astype(np.float64)
    c.oracle.zero_pad(c.theta)
    loss = eng.train_step_host(idx, labels, model.opt_from_flags(p))
    rl = c.reference(77, 0, 0.3)[0]
    l_plain = c.reference(0, 0, 0)[0]
    print("MARGINS " + json.dumps({"loss": abs(loss - rl), "away_from_no_dropout": abs(l_plain - rl)}))
    assert abs(loss - rl) < LOSS_REL * max(1.0, abs(rl))
    eng.close()
    with pytest.raises(_ffi.KprnError) as e:
        model.build_engine(model.parse_flags((FLAGS.replace("-rnnType rnn", "-rnnType lstm") + " -useDropout 1 -dropout 0.3").split()))
    assert e.value.code == _ffi.E_UNSUPPORTED
    eng = model.build_engine(model.parse_flags((FLAGS + " -useDropout 1 -dropout 0").split()))   # an engine without dropout
    _, fam = profiled_backward(eng, eng.batch(idx, labels))
    assert "embed_gather" in fam and "embed_gather_drop" not in fam, sorted(fam)
    eng.close()
