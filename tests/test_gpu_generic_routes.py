"""-m gpu: the launch table of the generic fp32 pipeline (kprn_amd/csrc/generic_pipeline.hip).

One profiled call per case; the {family: launches} dict of every family the pipeline's forward and backward open is compared with a literal table.  A family's
count is the number of profile scopes opened (a scope around the T launches of a step tier counts T), so the table pins which tier every layer took, which route
layer 0's input gradients took and how often each product ran.  The table was recorded from the library as it stood BEFORE the pipeline moved into its own file
and the three per-cell layer loops became one walk; it is the statement that the walk launches what the loops launched.

The batch is 130 pairs x 2 paths, T = 3: 260 paths is the smallest batch with a second 256-row tile where the step kernels apply (gemm::step_supported: N >= 256),
T > 1 gives the recurrent products and two layers give has_up.  The cases named "small" run 100 pairs x 2 paths: under 256 paths no step kernel and (persist_layers
= 0) no persistent launch applies, which is the only way to the unfused tier (a layer width that is no multiple of 4 keeps a layer off the persistent launch only;
the step kernels take any width: case lstm-odd-p2, whose forward runs lstm_step_fwd beside the persistent BPTT launch).

The last test holds generic::small_tables_route, as det_check calls it before anything is launched, against the backward's own call: under deterministic = 2 a
training call goes through exactly where the route the backward then takes has a deterministic form."""
import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu
T = 3
VE = 50
S = (6, VE, 9, 20, 60, 20, 100, 2)    # rnn, two layers: D = H = 100
S1 = (6, VE, 9, 20, 40, 20, 100, 1)   # rnn, one layer: D = 80 != H
W = (6, VE, 9, 24, 48, 24, 96, 2)     # FastLSTM / GRU, wide
ODD = (6, VE, 9, 22, 47, 22, 96, 1)   # FastLSTM, D = 91: no multiple of 4
G64 = (6, VE, 9, 16, 32, 16, 64, 2)   # the fused path's shape
R128 = (6, VE, 9, 20, 40, 132, 100, 1)   # rnn, a relation slice of 132 columns: the scatter route has no deterministic form (more than 128), the identity has

# families opened outside the pipeline (loss and pooling stages, one Adam step without clipping): not part of the table
NOT_GENERIC = {"loss_stage", "pool_sigmoid", "adam_step", "adam_dense", "adam_entity_rows"}


def _opts(persist, small=None, dropout=None, extra=()):
    o = [("persist_layers", persist)]
    if small is not None:
        o.append(("small_tables", small))
    if dropout:
        o += [("dropout", dropout), ("dropout_seed", "7")]
    return tuple(o) + tuple(extra)


def _cases():
    c = {}
    for name, shape in (("S", S), ("S1", S1)):
        for persist in ("0", "2"):
            for small in ("0", "1"):
                for drop in (None, "0.3"):
                    c[f"rnn-{name}-p{persist}-s{small}-d{drop or 0}"] = (shape, 1, _opts(persist, small, drop), "train", 130)
    for persist in ("0", "2"):
        for small in ("0", "1"):
            c[f"lstm-W-p{persist}-s{small}"] = (W, 0, _opts(persist, small), "train", 130)
        c[f"gru-W-p{persist}"] = (W, 2, _opts(persist), "train", 130)
    c["lstm-odd-p2"] = (ODD, 0, _opts("2"), "train", 130)
    c["lstm-G64-generic"] = (G64, 0, (("impl", "generic"),), "train", 130)
    for name, shape, rt in (("rnn-S", S, 1), ("lstm-W", W, 0), ("gru-W", W, 2)):
        c[f"{name}-small-p0"] = (shape, rt, _opts("0"), "train", 100)
        for persist in ("0", "2"):
            c[f"{name}-score-p{persist}"] = (shape, rt, _opts(persist), "score", 130)
    return c


CASES = _cases()


def _paths(pairs):
    return synth.make_paths(pairs, 2, T, Ve=VE, seed=5)


def run_case(case, pre_options=()):
    """one profiled call -> the full {family: launches} dict"""
    shape, rnn_type, options, what, pairs = case
    eng = _ffi.Engine(*shape, rnn_type=rnn_type)
    for k, v in tuple(pre_options) + tuple(options):
        eng.set_option(k, v)
    rng = np.random.default_rng(4)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    idx, labels = _paths(pairs)
    b = eng.batch(idx, labels)
    eng.profile(True)
    try:
        if what == "train":
            assert np.isfinite(eng.train_step(b, _ffi.make_opt(method=1, lr=1e-3)))
        else:
            assert np.all(np.isfinite(eng.forward(b, 1)["probs"]))
        fam = eng.profile_get()
    finally:
        eng.close()
    return {k: v[1] for k, v in fam.items()}


def generic(fam):
    return {k: n for k, n in sorted(fam.items()) if k not in NOT_GENERIC}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
# (counts are per call: two layers of T = 3 steps on a step tier give 6, their two T > 1 products 4, a persistent launch per layer 2)
TABLE = {
    "gru-W-p0": {'bias_colsum': 2, 'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_i2g_fwd': 2, 'gemm_o2g_bwd_dh': 8, 'gemm_o2g_bwd_dw': 2, 'gemm_o2g_fwd': 8, 'gru_cell_bwd': 12, 'gru_cell_fwd': 12, 'head_bwd': 1},
    "gru-W-p2": {'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dw': 2, 'gru_layer_bwd': 2, 'gru_layer_fwd': 2, 'head_bwd': 1},
    "gru-W-score-p0": {'embed_gather': 1, 'gemm_head_fwd': 1, 'gemm_i2g_fwd': 2, 'gemm_o2g_fwd': 8, 'gru_cell_fwd': 12},
    "gru-W-score-p2": {'embed_gather': 1, 'gemm_head_fwd': 1, 'gru_layer_fwd': 2},
    "gru-W-small-p0": {'bias_colsum': 2, 'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_i2g_fwd': 2, 'gemm_o2g_bwd_dh': 8, 'gemm_o2g_bwd_dw': 2, 'gemm_o2g_fwd': 8, 'gru_cell_bwd': 12, 'gru_cell_fwd': 12, 'head_bwd': 1},
    "lstm-G64-generic": {'bias_colsum': 2, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'lstm_gates_bwd': 6, 'lstm_step_fwd': 6, 'small_tables_finish': 1},
    "lstm-W-p0-s0": {'bias_colsum': 2, 'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'lstm_gates_bwd': 6, 'lstm_step_fwd': 6},
    "lstm-W-p0-s1": {'bias_colsum': 2, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'lstm_gates_bwd': 6, 'lstm_step_fwd': 6, 'small_tables_finish': 1},
    "lstm-W-p2-s0": {'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'lstm_layer_bwd': 2, 'lstm_layer_fwd': 2},
    "lstm-W-p2-s1": {'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'lstm_layer_bwd': 2, 'lstm_layer_fwd': 2, 'small_tables_finish': 1},
    "lstm-W-score-p0": {'embed_gather': 1, 'gemm_head_fwd': 1, 'lstm_step_fwd': 6},
    "lstm-W-score-p2": {'embed_gather': 1, 'gemm_head_fwd': 1, 'lstm_layer_fwd': 2},
    "lstm-W-small-p0": {'bias_colsum': 2, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_i2g_fwd': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'gemm_o2g_fwd': 4, 'head_bwd': 1, 'lstm_gates_bwd': 6, 'lstm_gates_fwd': 6, 'small_tables_finish': 1},
    "lstm-odd-p2": {'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'lstm_layer_bwd': 1, 'lstm_step_fwd': 3, 'small_tables_finish': 1},
    "rnn-S-p0-s0-d0": {'bias_colsum': 2, 'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_cell_bwd': 6, 'rnn_mask': 1, 'rnn_step_fwd': 6},
    "rnn-S-p0-s0-d0.3": {'bias_colsum': 2, 'drop_rows_bwd': 2, 'drop_rows_fwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_cell_bwd': 6, 'rnn_mask': 1, 'rnn_step_fwd': 6},
    "rnn-S-p0-s1-d0": {'bias_colsum': 2, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_cell_bwd': 6, 'rnn_mask': 1, 'rnn_step_fwd': 6, 'small_tables_finish': 1},
    "rnn-S-p0-s1-d0.3": {'bias_colsum': 2, 'drop_rows_bwd': 2, 'drop_rows_fwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_cell_bwd': 6, 'rnn_mask': 1, 'rnn_step_fwd': 6},
    "rnn-S-p2-s0-d0": {'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_layer_bwd': 2, 'rnn_layer_fwd': 2, 'rnn_mask': 1},
    "rnn-S-p2-s0-d0.3": {'drop_rows_bwd': 2, 'drop_rows_fwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_layer_bwd': 2, 'rnn_layer_fwd': 2, 'rnn_mask': 1},
    "rnn-S-p2-s1-d0": {'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_layer_bwd': 2, 'rnn_layer_fwd': 2, 'rnn_mask': 1, 'small_tables_finish': 1},
    "rnn-S-p2-s1-d0.3": {'drop_rows_bwd': 2, 'drop_rows_fwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 2, 'gemm_i2g_bwd_dx': 2, 'gemm_o2g_bwd_dw': 2, 'head_bwd': 1, 'rnn_layer_bwd': 2, 'rnn_layer_fwd': 2, 'rnn_mask': 1},
    "rnn-S-score-p0": {'embed_gather': 1, 'gemm_head_fwd': 1, 'rnn_mask': 1, 'rnn_step_fwd': 6},
    "rnn-S-score-p2": {'embed_gather': 1, 'gemm_head_fwd': 1, 'rnn_layer_fwd': 2, 'rnn_mask': 1},
    "rnn-S-small-p0": {'bias_colsum': 2, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_i2g_fwd': 2, 'gemm_o2g_bwd_dh': 4, 'gemm_o2g_bwd_dw': 2, 'gemm_o2g_fwd': 4, 'head_bwd': 1, 'rnn_cell_bwd': 6, 'rnn_cell_fwd': 6, 'rnn_mask': 1, 'small_tables_finish': 1},
    "rnn-S1-p0-s0-d0": {'bias_colsum': 1, 'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dh': 2, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_cell_bwd': 3, 'rnn_step_fwd': 3},
    "rnn-S1-p0-s0-d0.3": {'bias_colsum': 1, 'drop_rows_bwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dh': 2, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_cell_bwd': 3, 'rnn_step_fwd': 3},
    "rnn-S1-p0-s1-d0": {'bias_colsum': 1, 'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dh': 2, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_cell_bwd': 3, 'rnn_step_fwd': 3, 'small_tables_finish': 1},
    "rnn-S1-p0-s1-d0.3": {'bias_colsum': 1, 'drop_rows_bwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dh': 2, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_cell_bwd': 3, 'rnn_step_fwd': 3},
    "rnn-S1-p2-s0-d0": {'embed_gather': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_layer_bwd': 1, 'rnn_layer_fwd': 1},
    "rnn-S1-p2-s0-d0.3": {'drop_rows_bwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_layer_bwd': 1, 'rnn_layer_fwd': 1},
    "rnn-S1-p2-s1-d0": {'embed_gather': 1, 'entity_grad': 1, 'gemm_bwd_dw_merged': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dx_e': 1, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_layer_bwd': 1, 'rnn_layer_fwd': 1, 'small_tables_finish': 1},
    "rnn-S1-p2-s1-d0.3": {'drop_rows_bwd': 1, 'embed_gather_drop': 1, 'embed_scatter': 1, 'entity_grad': 1, 'gemm_head_fwd': 1, 'gemm_i2g_bwd_dw': 1, 'gemm_i2g_bwd_dx': 1, 'gemm_o2g_bwd_dw': 1, 'head_bwd': 1, 'rnn_layer_bwd': 1, 'rnn_layer_fwd': 1},
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_table(name):
    got = generic(run_case(CASES[name]))
    print(name, got)
    assert got == TABLE[name], (name, got)


@pytest.mark.parametrize("dropout", [None, "0.3"])
@pytest.mark.parametrize("small", ["0", "1"])
@pytest.mark.parametrize("shape", [S, R128], ids=["S", "R128"])
def test_the_route_det_check_expects_is_the_route_the_backward_takes(shape, small, dropout):
    """deterministic = 2.  S: both routes have a deterministic form, so every call trains, through the identity exactly when small_tables is on and nothing is dropped.
    R128: only the identity has one, so the call trains exactly in that case and is refused otherwise, before anything is launched."""
    ident = small == "1" and dropout is None
    case = (shape, 1, _opts("0", small, dropout), "train", 130)
    if shape is R128 and not ident:
        with pytest.raises(_ffi.KprnError) as e:
            run_case(case, pre_options=(("deterministic", "2"),))
        assert e.value.code == _ffi.E_UNSUPPORTED and "deterministic" in e.value.msg, e.value.msg
        return
    fam = run_case(case, pre_options=(("deterministic", "2"),))
    assert ("gemm_bwd_dw_merged" in fam) == ident and ("embed_scatter" in fam) == (not ident), sorted(fam)
