"""The inputs of tests/test_gpu_type_slots.py, checked on the CPU with the float64 oracle alone (no GPU): for every case of tests/type_slots_inputs.py
  * a kernel that reads only the first type slot gives scores (guard_fwd) and a type_emb gradient (guard_bwd) at least 3 x further from the oracle than the
    bar the case's route holds that quantity to -- except the scores of the route bf16_d64, which its GPU case says are no slot check;
  * at least 20 % of the non-pad steps carry one id in two slots;
  * no case has more than 320 paths.
The guards are printed ("GUARDS {...}"); the conditions are asserted, the numbers are not pinned.  Measured with these seeds, (2, 4) / (3, 6):
guard_fwd D = H = 64 L = 2 0.0080 .. 0.0083 / 0.0128 .. 0.0135, L = 1 0.105 / 0.188, H = 192 0.043 / 0.075, 50-100-50 -> 250 0.21 / 0.32, 128 x 3 -> 384
0.37 / 0.52, rnn 96 0.088 .. 0.32 / 0.16 .. 0.45, gru 128 0.078 .. 0.20 / 0.14 .. 0.35; guard_bwd over the route cases 0.445 (lstm_config_sh-2x4) .. 0.57 /
0.63 .. 0.75; repeat share 0.24 .. 0.27 at nT = 2 and 0.59 .. 0.65 at nT = 3 (Vt = 6: four real type ids).  The further cases: prefix64 0.014 / 0.68 / 0.63,
riding_train 0.0091 / 0.56 / 0.26, ragged 0.0080 / 0.81 / 0.24, feed 0.014 / 0.61 / 0.62, graph_fused 0.0064 / 0.69 / 0.45, graph_rnn 0.047 / 0.58 / 0.45
(guard_fwd / guard_bwd / repeat share)."""
import json

import numpy as np
import pytest

from tests import type_slots_inputs as ts


@pytest.mark.parametrize("name", ts.ALL_CASES)
def test_a_first_slot_only_kernel_cannot_pass(name):
    c = ts.case(name)
    assert c.idx.dtype == np.int32 and c.idx.shape[-1] == c.F and c.F >= c.nT + 2 and c.nT >= 2
    c0 = c.F - c.nT - 2
    assert c.idx[..., c0:c0 + c.nT].min() >= 1 and c.idx[..., c0:c0 + c.nT].max() <= c.Vt
    m = ts.check(c)
    print("GUARDS " + json.dumps(m))
    assert m["scores_check_slots"] == (c.route not in ts.SCORES_ARE_NO_SLOT_CHECK), m


def test_both_layouts_of_every_route_are_cases():
    from tests.test_gpu_gate_extremes import ROUTES
    assert ts.LAYOUTS == [(2, 4), (3, 6)]
    assert set(ts.ROUTE_CASES) == {f"{r}-{nT}x{F}" for r in ROUTES for nT, F in ts.LAYOUTS}
    for r in ROUTES:
        c = ts.case(ts.route_case(r, 3, 6))
        assert c.n_paths == ROUTES[r][3] * ROUTES[r][4] and c.idx.shape[2] == ROUTES[r][5]
        assert np.all(c.idx[..., 0] == c.Vt - 1)   # the unused leading column: the filler synth.make_paths writes, read by nothing


def test_theta_is_fp32_and_the_type_rows_are_scaled():
    c = ts.case(ts.route_case("rnn_tanh_step", 2, 4))
    assert np.array_equal(c.theta, c.theta.astype(np.float32).astype(np.float64))
    raw = c.o64.init_params(ts.PARAM_SEED, 0.05)
    t, r = c.tensor(c.theta, "type_emb"), c.tensor(raw, "type_emb")
    assert np.allclose(t[:-1], ts.TYPE_SCALE * r[:-1], rtol=1e-6) and not t[-1].any()   # (rnn: Oracle.zero_pad zeroes the last row of each table)


@pytest.mark.parametrize("name", ["rnn_relu_step-2x4", "rnn_tanh_persist-3x6"])
def test_the_dropout_reference_sums_the_slots_like_the_oracle(name):
    """tests/dropout_ref.py forward_backward with all-ones masks and scale 1 is the oracle's graph, with several type slots and a leading column too"""
    from tests import dropout_ref as dr
    c = ts.case(name)
    T, N = c.idx.shape[2], c.n_paths
    loss, grad, _ = dr.forward_backward(c.o64.layout(), c.o64.cfg, c.theta, c.idx, c.labels, dr.ones_masks(c.o64.cfg, T, N), 1.0)
    ol, og = c.backward()
    assert abs(loss - ol) < 1e-10   # (the bars of tests/test_dropout_host.py)
    for nm, (off, shp) in c.o64.layout().items():
        n = int(np.prod(shp))
        assert ts.rel_inf(grad[off:off + n], og[off:off + n]) < 1e-10, nm


def test_the_feed_case_fills_its_leading_column_with_arbitrary_values():
    """nothing may read the columns before the type slots: the case the feed tests run holds values there that are no id of any table, different in every step,
    so a validator, a prefix comparison or a gather that starts at column 0 instead of F - nT - 2 refuses the batch, finds no prefix or misses the oracle"""
    c = ts.case("feed")
    lead = c.idx[..., 0]
    assert c.F - c.nT - 2 == 1 and lead.min() < 1 and lead.max() > max(c.Vt, c.Ve, c.Vr) and len(np.unique(lead)) > lead.size // 2
    pads = c.idx[..., c.F - 2] == c.Ve
    assert pads[:, :, :2].all(axis=2).any() and len(np.unique(lead[pads])) > 10   # pad steps, equal from column 1 on, differ in column 0
