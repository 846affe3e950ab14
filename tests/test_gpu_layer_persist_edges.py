"""-m gpu: the two persistent fp32 layer launches (kprn_amd/csrc/layer_f32_persist.hip k_layer<CELL, NCH, SAVE> / k_bptt<CELL, NCH, UP>) at every edge of
their shape space -- every instantiation the two dispatch blocks can select, H % 4 = 0 / 1 / 2 / 3, a last chunk of one unit, waves without a unit, Din
from 16 to 256, both ring depths and the shape on either side of each LDS boundary, N and T at a tile's and the schedule's edges, several tiles per
workgroup (option "persist_layers_grid") and poisoned slack behind the saves -- against the float64 oracle at the fp32 bars of test_gpu_layer_persist.py
(scores 2e-5 of the largest, every class probability rtol 1e-4, loss 1e-5, every gradient tensor 2e-4 of its largest element) and then against the
per-step launches on the same engine ("persist_layers" = 0: scores 2e-6, gradients 2e-5).  Every case runs impl = generic, "persist_layers" = 2, Ve = 800,
Vt = 6, Vr = 9, theta rounded through fp32, and asserts its route and its launch counts from the profiler's families.

Every case runs a scoring pass (SAVE = false) and a training pass (SAVE = true); with L = 2 the bottom layer's BPTT is UP = true, the top layer's (and
L = 1's) UP = false, and both layers' forwards go through the launch (asserted: L launches per pass).  NCH = ceil(H / 64) (rnn and the gru BPTT: always 1).
Ring depth R of the forward: 3 while KX + KH <= 416, 2 up to 480, refused above (KX, KH: Din, H rounded up to 32); the BPTT ring is always 3 deep.

  instantiation              R   cases (D is Din of layer 0; L = 1 unless said)
  k_layer<0, 1, F|T>         3   lstm H 16, 48, 64 (D 64); D = H = 16 and 64, L = 2; Din 20 and 36 (H 48)
  k_layer<0, 2, F|T>         3   lstm H 65, 67, 70; D = H = 128, L = 2 (also T = 1, grids 1 2 4 5); N 1 63 64 65 (H 70); T 2, 12 (H 67)
  k_layer<0, 3, F|T>         3   lstm H 129; D = H = 160, L = 2
  k_layer<0, 4, F|T>         3   lstm H 193 (also grids 1 2 4 5), 253 (also poisoned), 255
  k_layer<0, 4, F|T>         2   lstm Din 256, H 200 (480); D = H = 224, L = 2 (448, both layers)
  k_layer<1, 1, F|T>         3   rnn H 17, 63, 65, 130, 253, 255 (D 64); D = H = 100, L = 2; N 256 257 319, T 2, 12, grids 1 2 4 5, poisoned N 257 (H 253)
  k_layer<2, 1, F|T>         3   gru H 16; D = H = 16, L = 2; D = H = 64, L = 2, T = 1
  k_layer<2, 2, F|T>         3   gru H 65, 67; N 1 63 64 65, T 2, 12, poisoned (H 67)
  k_layer<2, 3, F|T>         3   gru H 130 (also grids 1 2 4 5); Din 256, H 160 (416: the last R = 3 shape)
  k_layer<2, 4, F|T>         3   gru H 193, 253
  k_layer<2, 4, F|T>         2   gru Din 256, H 200 (480); D = H = 224, L = 2 (448)
  (no forward launch)        -   lstm Din 256, H 250 (512: refused, per-step forward); rnn at N 111 and poisoned N 65 (below the step kernel's 256 rows)
  k_bptt<0, 1, false|true>   3   as k_layer<0, 1>: false every case's top layer, true the bottom layer of the L = 2 cases (D = H = 16, 64)
  k_bptt<0, 2, false|true>   3   as k_layer<0, 2>: true at D = H = 128, L = 2 (T 6, T 1, grids 1 2 4 5: bias sums in registers)
  k_bptt<0, 3, false|true>   3   as k_layer<0, 3>: true at D = H = 160, L = 2 (bias sums in LDS slots)
  k_bptt<0, 4, false|true>   3   as k_layer<0, 4> + lstm Din 256, H 250: true at D = H = 224, L = 2
  k_bptt<1, 1, false|true>   3   every rnn case, N 111 and poisoned N 65 included: true at D = H = 100, L = 2
  k_bptt<2, 1, false|true>   3   every gru case: true at D = H = 16, 224 and 64 (T = 1), L = 2

MaskZero: every rnn batch holds paths with leading pad steps and paths that are pads up to step T - 1 (set by hand, asserted).
The worst figure measured per quantity over all cases, next to its bar, is recorded in CHANGELOG.md under this file's entry."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from tests.test_gpu_layer_persist import _mk, rel_inf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE, PROB_RTOL, LOSS, GRAD = 2e-5, 1e-4, 1e-5, 2e-4   # against the float64 oracle (test_gpu_layer_persist.py's bars)
STEP_SCORE, STEP_GRAD = 2e-6, 2e-5                        # against the per-step launches
STEP_FWD = ("lstm_step_fwd", "rnn_step_fwd", "gemm_i2g_fwd", "gemm_o2g_fwd", "lstm_gates_fwd", "rnn_cell_fwd", "gru_cell_fwd")
STEP_BWD = ("lstm_gates_bwd", "rnn_cell_bwd", "gru_cell_bwd", "gemm_o2g_bwd_dh")
CELL_FWD = {"lstm": "lstm_gates_fwd", "rnn": "rnn_cell_fwd", "gru": "gru_cell_fwd"}
CELL_BWD = {"lstm": "lstm_gates_bwd", "rnn": "rnn_cell_bwd", "gru": "gru_cell_bwd"}
PAD = (5, 800, 8)  # (type, entity, relation) pad ids at Vt = 6, Ve = 800, Vr = 9 (synth.make_paths)

D16, D20, D36, D64, D100, D128, D160, D224, D256 = (4, 8, 4), (4, 12, 4), (8, 20, 8), (16, 32, 16), (24, 52, 24), (32, 64, 32), (40, 80, 40), (56, 112, 56), (64, 128, 64)


def paths(kind, pairs, P, T, seed=None):
    """synth.make_paths; rnn: plus paths that are pads up to step T - 1 and (T > 2) paths with one leading pad, so that MaskZero sees both kinds whatever T is"""
    idx, labels = synth.make_paths(pairs, P, T, Ve=800, seed=pairs + T if seed is None else seed)
    if kind == "rnn":
        flat = idx.reshape(pairs * P, T, 3)
        n = flat.shape[0]
        for r in {0, n // 2, n - 1}:
            flat[r, :T - 1] = PAD
        if T > 2:
            flat[1:n - 1:7, :1] = PAD
        is_pad = flat[:, :, 1] == PAD[1]
        assert not is_pad[:, T - 1].any()
        lead = np.argmin(is_pad, axis=1)
        assert (lead == T - 1).any() and (lead > 0).any() and (T <= 2 or ((lead > 0) & (lead < T - 1)).any()), np.bincount(lead)
    return idx, labels


class Ref:
    """the float64 oracle's answers for one batch, computed once"""

    def __init__(self, o64, theta, idx, labels):
        self.ps, _, self.probs = o64.forward(theta, idx)
        self.loss, self.grads, _ = o64.forward_backward(theta, idx, labels)


def passes(eng, b, kind, L, route):
    """a scoring pass and a training pass under the engine's current options -> (scores and probabilities, loss, gradients); asserts the route: 'persist' (both
    launches, L each per pass), 'step_fwd' / 'cell_fwd' (forward on the step kernel / on product + cell launches, BPTT persistent), 'step' (neither launch)"""
    lf, lb = kind + "_layer_fwd", kind + "_layer_bwd"
    eng.profile_reset()
    eng.profile(True)
    out = eng.forward(b, 1, want=("probs", "all_probs", "path_scores"))
    fam = eng.profile_get()
    if route == "persist":
        assert lf in fam and fam[lf][1] == L and not [f for f in STEP_FWD if f in fam], sorted(fam)
    else:
        assert lf not in fam, sorted(fam)
        if route == "step_fwd":
            assert kind + "_step_fwd" in fam, sorted(fam)
        if route == "cell_fwd":
            assert "gemm_i2g_fwd" in fam and CELL_FWD[kind] in fam and kind + "_step_fwd" not in fam, sorted(fam)
    eng.profile_reset()
    loss = eng.backward(b, 1)
    fam = eng.profile_get()
    eng.profile(False)
    if route == "persist":
        assert lf in fam and fam[lf][1] == L and not [f for f in STEP_FWD if f in fam], sorted(fam)   # (the training forward is the launch too)
    else:
        assert lf not in fam, sorted(fam)
    if route == "step":
        assert lb not in fam and CELL_BWD[kind] in fam, sorted(fam)
    else:
        assert lb in fam and fam[lb][1] == L and not [f for f in STEP_BWD if f in fam], sorted(fam)
    return out, loss, eng.get_flat_grads()


def tensors(eng):
    for nm, (off, shp) in eng.layout().items():
        yield nm, slice(off, off + int(np.prod(shp)))


def against_oracle(tag, eng, got, ref):
    out, loss, g = got
    worst = {nm: rel_inf(g[sl], ref.grads[sl]) for nm, sl in tensors(eng)}
    m = {"case": tag, "score": rel_inf(out["path_scores"], ref.ps), "prob": float(np.max(np.abs(out["all_probs"] - ref.probs) / np.abs(ref.probs))),
         "loss": abs(loss - ref.loss) / max(1, abs(ref.loss)), "grad": max(worst.values()), "worst": max(worst, key=worst.get)}
    print("EDGES " + json.dumps(m))
    assert np.isfinite(out["path_scores"]).all() and np.isfinite(out["all_probs"]).all() and np.isfinite(loss) and np.isfinite(g).all(), m
    assert m["score"] < SCORE, m
    np.testing.assert_allclose(out["all_probs"], ref.probs, rtol=PROB_RTOL)
    np.testing.assert_allclose(out["probs"], ref.probs[:, 0], rtol=PROB_RTOL)
    assert m["loss"] < LOSS, m
    for nm, v in worst.items():
        assert v < GRAD, (nm, v, m)
    return m


def against_other(tag, eng, got, other):
    """two runs of the same arithmetic in another accumulation order (the per-step launches, another grid)"""
    worst = {nm: rel_inf(got[2][sl], other[2][sl].astype(np.float64)) for nm, sl in tensors(eng)}
    m = {"case": tag, "step_score": rel_inf(got[0]["path_scores"], other[0]["path_scores"].astype(np.float64)), "step_grad": max(worst.values()), "worst": max(worst, key=worst.get)}
    print("EDGES " + json.dumps(m))
    assert m["step_score"] < STEP_SCORE, m
    for nm, v in worst.items():
        assert v < STEP_GRAD, (nm, v, m)


def check(tag, kind, dims, H, L, pairs, P, T, route="persist"):
    eng, o64, theta = _mk(kind, dims + (H,), L)
    try:
        idx, labels = paths(kind, pairs, P, T)
        b = eng.batch(idx, labels)
        got = passes(eng, b, kind, L, route)
        against_oracle(tag, eng, got, Ref(o64, theta, idx, labels))
        eng.set_option("persist_layers", "0")
        against_other(tag + " vs steps", eng, got, passes(eng, b, kind, L, "step"))
    finally:
        eng.close()


# ---- hidden-size remainders and chunk counts: H % 4 = 0 .. 3, a last chunk of one unit (65, 129, 193), waves that own no unit (H < 64), K pads of the recurrent half
@pytest.mark.parametrize("H", [16, 48, 64, 65, 67, 70, 129, 193, 253, 255])
def test_lstm_hidden_sizes(H):
    check(f"lstm H={H}", "lstm", D64, H, 1, 100, 3, 6)


@pytest.mark.parametrize("H", [17, 63, 65, 130, 253, 255])
def test_rnn_hidden_sizes(H):
    check(f"rnn H={H}", "rnn", D64, H, 1, 100, 3, 6)


def test_rnn_two_layers_kh_padded():
    """D = H = 100: KX and KH both padded 100 -> 128, the upper layer's mask follows h of the lower one, k_bptt<1, 1, true>"""
    check("rnn D=H=100 L=2", "rnn", D100, 100, 2, 100, 3, 6)


@pytest.mark.parametrize("H", [16, 65, 67, 130, 193, 253])
def test_gru_hidden_sizes(H):
    check(f"gru H={H}", "gru", D64, H, 1, 100, 3, 6)


# ---- a layer above (L = 2 needs D = H: layer 1's Din is H): write_all_h, UP, every NCH of the FastLSTM BPTT with UP
@pytest.mark.parametrize("kind,dims", [("lstm", D16), ("lstm", D64), ("lstm", D128), ("lstm", D160), ("lstm", D224), ("gru", D16), ("gru", D224)])
def test_a_layer_above(kind, dims):
    H = sum(dims)
    check(f"{kind} D=H={H} L=2", kind, dims, H, 2, 100, 3, 6)


# ---- Din: the minimum's neighbours and both KX pads, all 16 prefetch pieces, the shapes on either side of R = 3 | R = 2 | refused
@pytest.mark.parametrize("kind,dims,H,route", [("lstm", D20, 48, "persist"),      # KX pad 12
                                               ("lstm", D36, 48, "persist"),      # KX pad 28
                                               ("lstm", D256, 200, "persist"),    # KX + KH = 480: R = 2, the last shape the forward takes
                                               ("gru", D256, 200, "persist"),
                                               ("gru", D256, 160, "persist"),     # 416: the last R = 3 shape
                                               ("lstm", D256, 250, "step_fwd")])  # 512: the forward is refused (per-step launches), the BPTT is not
def test_din_and_the_lds_boundary(kind, dims, H, route):
    check(f"{kind} Din={sum(dims)} H={H}", kind, dims, H, 1, 100, 3, 6, route)


# ---- N at a tile's edges: every lane clamped to row 0, a tile one row short, exactly full, one row into the second tile
@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("kind,H", [("lstm", 70), ("gru", 67)])
def test_n_at_a_tile_edge(kind, H, N):
    check(f"{kind} H={H} N={N}", kind, D64, H, 1, N, 1, 6)


@pytest.mark.parametrize("N", [256, 257, 319])
def test_rnn_n_at_a_tile_edge(N):
    check(f"rnn H=253 N={N}", "rnn", D64, 253, 1, N, 1, 6)


def test_rnn_below_the_step_kernels_rows():
    """111 paths: no step kernel, so no persistent forward either (generic_pipeline.hip: the rnn's launch goes where the step kernel would) -- product + cell
    launches forward, the persistent BPTT over the saves they wrote"""
    check("rnn H=253 N=111", "rnn", D64, 253, 1, 37, 3, 6, "cell_fwd")


# ---- T at its edges: the ring's shortest schedule with a recurrent half, a long one, and no recurrent half at all under a layer above
@pytest.mark.parametrize("T", [2, 12])
@pytest.mark.parametrize("kind,H", [("lstm", 67), ("rnn", 253), ("gru", 67)])
def test_t_at_its_edges(kind, H, T):
    check(f"{kind} H={H} T={T}", kind, D64, H, 1, 100, 3, T)


@pytest.mark.parametrize("kind,dims", [("lstm", D128), ("gru", D64)])
def test_one_step_with_a_layer_above(kind, dims):
    H = sum(dims)
    check(f"{kind} D=H={H} L=2 T=1", kind, dims, H, 2, 100, 3, 1)


# ---- several tiles per workgroup
@pytest.mark.parametrize("kind,dims,H,L", [("lstm", D128, 128, 2),    # bias sums in registers
                                           ("lstm", D64, 193, 1),     # bias sums in LDS slots
                                           ("rnn", D64, 253, 1),
                                           ("gru", D64, 130, 1)])
def test_several_tiles_per_workgroup(kind, dims, H, L):
    """327 paths = 5 full tiles + 7 rows on 1, 2, 4 and 5 workgroups ("persist_layers_grid"): 6, 3 + 3, 1 + 2 + 1 + 2 and 1 + 1 + 1 + 1 + 2 tiles -- the ring's cursor
    running into the next tile, bias sums carried over a workgroup's tiles, a ragged last tile behind full ones.  Each grid against the oracle; the forward is
    bit-identical across grids (a tile's forward does not depend on the workgroup that runs it); gradients across grids and against the per-step launches at the
    reordering bar (dW products and bias sums add in another order)."""
    eng, o64, theta = _mk(kind, dims + (H,), L)
    try:
        idx, labels = paths(kind, 109, 3, 6)
        ref = Ref(o64, theta, idx, labels)
        b = eng.batch(idx, labels)
        res = {}
        for grid in (1, 2, 4, 5, 0):
            eng.set_option("persist_layers_grid", str(grid))
            res[grid] = passes(eng, b, kind, L, "persist")
            against_oracle(f"{kind} H={H} L={L} grid={grid}", eng, res[grid], ref)
        for grid in (1, 2, 4, 5):
            for k in ("path_scores", "all_probs", "probs"):
                assert np.array_equal(res[grid][0][k].view(np.uint32), res[0][0][k].view(np.uint32)), (grid, k)
            against_other(f"{kind} H={H} L={L} grid={grid} vs grid=0", eng, res[grid], res[0])
        eng.set_option("persist_layers", "0")
        steps = passes(eng, b, kind, L, "step")
        for grid in (1, 2, 4, 5, 0):
            against_other(f"{kind} H={H} L={L} grid={grid} vs steps", eng, res[grid], steps)
    finally:
        eng.close()


def test_grid_option_values():
    eng, _, _ = _mk("lstm", D64 + (70,), 1)
    try:
        for bad in ("-1", "x", "", "2x"):
            with pytest.raises(_ffi.KprnError) as e:
                eng.set_option("persist_layers_grid", bad)
            assert e.value.code == _ffi.E_ARG
        eng.set_option("persist_layers_grid", "3")
        eng.set_option("persist_layers_grid", "0")
    finally:
        eng.close()


# ---- poisoned slack: a quad straddling H is read where it lies; behind the last row of the last plane lie bytes nobody wrote
def poison_child(kind):
    """(runs in the child process) H % 4 != 0, 65 paths, T = 3, forward and backward: check() asserts finiteness, the oracle bars and the route"""
    H = 67 if kind == "gru" else 253
    check(f"poisoned {kind} H={H} N=65", kind, D64, H, 1, 65, 1, 3, "cell_fwd" if kind == "rnn" else "persist")
    if kind == "rnn":   # (65 paths are below the rnn forward launch's 256: once more where it runs)
        check(f"poisoned rnn H={H} N=257", kind, D64, H, 1, 257, 1, 3)


@pytest.mark.parametrize("kind", ["lstm", "rnn", "gru"])
def test_poisoned_slack(kind):
    """KPRN_POISON_ALLOC=1 in a fresh process: every device allocation starts as 0xFF bytes (NaN), so the lanes past H of the straddling quad of the last row of the
    last plane hold NaN -- the selects must keep them out of every score, the loss and every gradient"""
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_layer_persist_edges import poison_child; poison_child(%r)" % (ROOT, kind)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    ms = [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("EDGES ")]
    # check() has asserted every bar in the child already; what only the parent can tell is that the child ran ALL its checks -- one EDGES line for the oracle and
    # one for the per-step launches per check() call (rnn: two calls).  A child that returned early would exit 0 with fewer lines.
    assert len(ms) == (4 if kind == "rnn" else 2), ms
    for m in ms:
        if "score" in m:
            assert m["score"] < SCORE and m["prob"] < PROB_RTOL and m["loss"] < LOSS and m["grad"] < GRAD, m
        else:
            assert m["step_score"] < STEP_SCORE and m["step_grad"] < STEP_GRAD, m
