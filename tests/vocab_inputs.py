"""Inputs that reach EVERY row of the type and relation tables, and the case table of the vocabulary-edge tests (tests/test_small_table_vocab_inputs.py on
the CPU, tests/test_gpu_small_table_vocab.py on the GPU).

synth.make_paths follows the shipped sample: types 1..Vt-2 and the pad id Vt-1, relations 1..Vr-3, the pad id Vr-1 and #END_RELATION Vr -- the #UNK rows
(type Vt, relation Vr-2) are never drawn, so the last one-hot column of a small-table route carries a gradient of exactly zero on both sides of every
comparison built on it.  paths_every_id keeps make_paths' entity column and labels and draws both small columns uniformly over the whole vocabulary.
Forward and backward only: a row that is a pad row to train_step (zeroPadTokens) is a row like any other here."""
import functools

import numpy as np

from kprn_amd import synth
from oracle.oracle import Oracle, make_cfg

T = 6
ROW_SHARE = 1e-2   # every table row's largest gradient entry, as a share of the tensor's largest: 50 x the 2e-4 gradient bar of the fp32 routes


def paths_every_id(pairs, P, T, Vt, Vr, Ve, seed):
    """-> (idx int32 [pairs, P, T, 3], labels f32 [pairs]): synth.make_paths' entities and labels, type ids uniform over 1..Vt, relation ids uniform over 1..Vr"""
    idx, labels = synth.make_paths(pairs, P, T, F=3, Vt=Vt, Ve=Ve, Vr=Vr, num_types=1, seed=seed)
    rng = np.random.default_rng([seed, Vt, Vr])
    idx = idx.copy()
    idx[..., 0] = rng.integers(1, Vt + 1, size=idx.shape[:3], dtype=np.int32)
    idx[..., 2] = rng.integers(1, Vr + 1, size=idx.shape[:3], dtype=np.int32)
    return idx, labels


# name: (kind, (dt, de, dr, H), L, Ve, pairs, P, parameter seed, parameter scale, data seed)
SHAPES = {
    "fused64": ("lstm", (16, 32, 16, 64), 2, 900, 170, 3, 1, 0.1, 33),       # the fused D = H = 64 kernels (tests/test_gpu_parity.py mk)
    "generic64": ("lstm", (16, 32, 16, 64), 2, 900, 170, 3, 17, 0.06, 33),   # "impl" = generic (tests/test_gpu_wide.py test_generic_small_table_gradients_match_the_dx_route)
    "generic192": ("lstm", (64, 64, 64, 192), 2, 900, 170, 3, 17, 0.06, 33),
    "rnn250": ("rnn", (50, 100, 50, 250), 1, 900, 170, 3, 17, 0.06, 33),
    "bf16_384": ("lstm", (128, 128, 128, 384), 1, 700, 700, 3, 4, 0.05, 5),  # configs[3] (tests/test_gpu_persist.py _case)
}

# (Vt, Vr) of the fused D = H = 64 cases: one-hot columns Vr + Vt = 16 with the relation / type split in the middle and at both ends (column 15 = the last type
# row), 17 (both identities off), both 16-row accumulator tiles full, either table one row above the small-job limit
FUSED_VOCABS = [(7, 9), (2, 14), (13, 3), (8, 9), (16, 16), (17, 9), (6, 17)]
# generic fp32, ns = roundup4(Vr + Vt) against dt: (shape, (Vt, Vr), on the route)
GENERIC_VOCABS = [("generic64", (7, 9), True), ("generic64", (8, 9), False),
                  ("generic192", (32, 32), True), ("generic192", (30, 31), True), ("generic192", (32, 33), False),
                  ("rnn250", (24, 24), True), ("rnn250", (25, 24), False)]
# bf16 merged dW: Vt + Vr = 128 exactly, and 129
BF16_VOCABS = [("bf16_384", (28, 100), True), ("bf16_384", (29, 100), False)]

ALL_CASES = [("fused64", v) for v in FUSED_VOCABS] + [(s, v) for s, v, _ in GENERIC_VOCABS] + [(s, v) for s, v, _ in BF16_VOCABS]


class Case:
    """one (shape, vocabulary): the float64 oracle, parameters rounded to fp32, inputs from paths_every_id; the oracle's answers are computed once and shared"""

    def __init__(self, shape, Vt, Vr):
        kind, (dt, de, dr, H), L, Ve, pairs, P, pseed, init, dseed = SHAPES[shape]
        self.shape, self.kind, self.dims, self.L, self.Vt, self.Vr, self.Ve, self.init = shape, kind, (dt, de, dr, H), L, Vt, Vr, Ve, init
        self.rnn_type = 1 if kind == "rnn" else 0
        self.o64 = Oracle(make_cfg(Vt=Vt, Ve=Ve, Vr=Vr, dt=dt, de=de, dr=dr, H=H, L=L, rnn_type=self.rnn_type, use_relu=1), np.float64)
        theta = self.o64.init_params(pseed, init).astype(np.float32).astype(np.float64)   # the oracle sees exactly the fp32 values
        if self.rnn_type:
            self.o64.zero_pad(theta)
        self.theta = theta
        self.idx, self.labels = paths_every_id(pairs, P, T, Vt, Vr, Ve, dseed)
        self._fwd = self._bwd = None

    def forward(self):
        """(path scores [N, 46], all class probabilities [B, 46])"""
        if self._fwd is None:
            ps, _, probs = self.o64.forward(self.theta, self.idx)
            self._fwd = (ps, probs)
        return self._fwd

    def backward(self):
        """(loss, flat gradient)"""
        if self._bwd is None:
            ol, og, _ = self.o64.forward_backward(self.theta, self.idx, self.labels)
            self._bwd = (ol, og)
        return self._bwd

    def table_grads(self):
        _, og = self.backward()
        out = {}
        for nm in ("type_emb", "relation_emb"):
            off, shp = self.o64.layout()[nm]
            out[nm] = og[off:off + int(np.prod(shp))].reshape(shp)
        return out


@functools.lru_cache(maxsize=None)
def case(shape, Vt, Vr):
    return Case(shape, Vt, Vr)
