"""-m gpu: the small-table identity on the fused D = H = 64 BPTT (kprn_amd/csrc/lstm_fused_bwd.hip bwd_body IDENT).

With x = [Wt[type] | We[entity] | Wr[relation]], the bottom layer's launch forms dx for the entity slice only and G = dA^T [S_r | S_t] in place of the
type / relation blocks of dW_i2g; kk::small_tables_finish turns G into those blocks and both table gradients (nn.LookupTable backward,
net/FeatureEmbedding.lua:86,112-121).  Option "small_tables" = 0 keeps the dx route in-process.  What must hold, on one engine shape:
  * the forward is untouched: scores and loss bit-identical;
  * every gradient (W_i2g blocks, Wt, Wr, We rows, the rest) within 2e-5 of the tensor's largest element: the same sums in another order;
  * 64-path tiles with and without the identical-prefix plan and the tile hand-over take the route; 16-row tiles and de != 32 fall back;
  * 20 Adam steps with clipping and L2 agree in the parameters."""
import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu
T = 6


def mk(small_tables, plan=True, handover=2, dims=(16, 32, 16), Ve=30000, small_tiles="0"):
    eng = _ffi.Engine(6, Ve, 9, dims[0], dims[1], dims[2], 64, 2)
    eng.set_option("small_tiles", small_tiles)
    eng.set_option("prefix_plan", "1" if plan else "0")
    eng.set_option("tile_handover", str(handover))
    eng.set_option("small_tables", str(small_tables))
    rng = np.random.default_rng(5)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    return eng


def rel_inf(a, c):
    return float(np.max(np.abs(a - c))) / max(1e-30, float(np.max(np.abs(c))))


# (pairs, P, plan, hand-over, small tiles, dims, route taken)
CASES = [(65536 // 4, 4, True, 2, "0", (16, 32, 16), True),
         (65536 // 4, 4, False, 0, "0", (16, 32, 16), True),
         (4000, 4, True, 1, "0", (16, 32, 16), True),
         (19200, 1, False, 2, "0", (16, 32, 16), True),
         (300, 4, False, 0, "0", (16, 32, 16), True),
         (60, 4, True, 2, "1", (16, 32, 16), False),
         (4000, 4, True, 2, "0", (16, 16, 32), False)]


@pytest.mark.parametrize("pairs,P,plan,handover,small,dims,route", CASES)
def test_identity_route_equals_dx_route(pairs, P, plan, handover, small, dims, route):
    idx, labels = synth.make_paths(pairs, P, T, Ve=30000, seed=pairs % 997 + P)
    res = []
    for st in (1, 0):
        eng = mk(st, plan, handover, dims, small_tiles=small)
        b = eng.batch(idx, labels)
        out = eng.forward(b, 1, want=("path_scores", "probs"))
        eng.profile(True)
        loss = eng.backward(b, 1)
        fam = eng.profile_get()
        assert ("small_tables_finish" in fam) == (route and st == 1), sorted(fam)
        res.append((out["path_scores"].copy(), out["probs"].copy(), loss, eng.get_flat_grads().astype(np.float64), eng.layout()))
        eng.close()
    (s1, p1, l1, g1, lay), (s0, p0, l0, g0, _) = res
    assert np.array_equal(s1, s0) and np.array_equal(p1, p0) and l1 == l0
    seen = 0
    for nm, (off, shp) in lay.items():
        n = int(np.prod(shp))
        a, c = g1[off:off + n], g0[off:off + n]
        assert rel_inf(a, c) < 2e-5, nm
        seen += float(np.max(np.abs(c))) > 0
    assert seen >= 8


def test_identity_route_adam_steps_with_clip_and_l2():
    batches = [synth.make_paths(4000, 4, T, Ve=30000, seed=71 + i) for i in range(2)]
    res = []
    for st in (1, 0):
        eng = mk(st)
        opt = _ffi.make_opt(method=1, lr=1e-3, use_grad_clip=1, grad_clip_norm=0.5, l2=1e-3)
        bs = [eng.batch(i, l) for i, l in batches]
        losses = [eng.train_step(bs[k % 2], opt) for k in range(20)]
        res.append((eng.get_flat_params().astype(np.float64), losses))
        eng.close()
    (w1, l1), (w0, l0) = res
    assert np.max(np.abs(np.asarray(l1) - np.asarray(l0))) < 1e-4 * max(1.0, float(np.max(np.abs(l0))))
    assert rel_inf(w1, w0) < 2e-5
