"""Inputs with SEVERAL TYPE SLOTS and unused leading feature columns, and the proof that a slot bug cannot hide in them: the one case list of
tests/test_type_slots_inputs.py (CPU, the float64 oracle alone) and tests/test_gpu_type_slots.py (GPU).

The model's input is [pairs, paths, steps, F]: the last two columns are entity and relation, the num_types columns before them are type slots whose table
rows are summed (CAddTable, net/FeatureEmbedding.lua:55), any column before those is ignored.  Two layouts: (nT, F) = (2, 4) and (3, 6), the second with one
unused leading column.  Every route of tests/test_gpu_gate_extremes.py::ROUTES runs at both, with its own pairs / P / T; the further cases (64-row tiles with
a prefix, ragged, a graph's paths) are listed in EXTRA.  Parameters: init_params(seed, 0.05), the type_emb rows multiplied by TYPE_SCALE, rnn: pad rows
zeroed, all rounded to fp32.

check(case) asserts three conditions, and the GPU tests call it before they run a case:
  forward guard   o1 = the oracle with numTypes = 1, F = 3 on the same theta (the parameter layout does not depend on F), idx1 = idx[..., [F-nT-2, F-2, F-1]]:
                  what a kernel computes that reads the first slot only.  guard_fwd = rel_inf(scores(o1, idx1), scores(o64, idx)).
  backward guard  the same on the type_emb gradient tensor: guard_bwd.
  repeat share    at least 20 % of the non-pad steps carry one id in two slots: a "set, not add" one-hot or a lost second atomic on one row shows only there.
Each guard must be at least MARGIN = 3 times the bar its quantity is held to on the case's route (BARS: the project's own; with a second slot both bf16 routes
run the per-step pipeline and take its bars from tests/test_gpu_wide.py).  The one exception is the route bf16_d64: at D = H = 64 the scores hang mostly on the
head's bias (guard_fwd about 0.01, rising only linearly with the scale), so on that route the scores are compared at their bar but are NO slot check; the
type_emb gradient is.  check() fails if any other case needs the exception."""
import functools

import numpy as np

from kprn_amd import _ffi, synth
from oracle.oracle import Oracle, make_cfg
from tests import path_find_ref as pref
from tests.test_gpu_gate_extremes import ROUTES

VT, VE, VR = 6, 900, 9
TYPE_SCALE = 4.0
LAYOUTS = [(2, 4), (3, 6)]
MARGIN = 3.0
REPEAT_SHARE = 0.20
# what each quantity is held to: scores and every gradient tensor as a share of the largest entry, probabilities (rtol for fp32, atol for bf16), loss, parameters
BARS = {"fp32": dict(score=2e-5, probs=1e-4, loss=1e-5, grad=2e-4, params=2e-4),
        "bf16": dict(score=3e-2, probs=2e-2, loss=3e-2, grad=6e-2, params=None)}
SCORES_ARE_NO_SLOT_CHECK = {"bf16_d64"}   # (see the module docstring)
PARAM_SEED, DATA_SEED = 11, 11


def rel_inf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(1e-30, np.max(np.abs(b))))


def route_case(route, nT, F):
    return f"{route}-{nT}x{F}"


# name: (kind, (dt, de, dr, H), L, (nT, F), engine kwargs, data) -- data: ("rect", pairs, P, T) | ("ragged", pairs, long pair's paths, T) | ("graph", T, cap)
FUSED, RNN4 = (16, 32, 16, 64), (8, 16, 8, 40)
EXTRA = {
    "prefix64_f32": ("lstm", FUSED, 2, (3, 6), {}, ("rect", 5 * 64 - 9, 1, 6)),                        # 64-row tiles, a ragged last tile, a real prefix
    "prefix64_f32x6": ("lstm", FUSED, 2, (3, 6), {"compute_dtype": 2}, ("rect", 5 * 64 - 9, 1, 6)),
    "riding_train": ("lstm", FUSED, 2, (2, 4), {}, ("rect", 53, 3, 6)),                               # the training batch a scoring pass rides in
    "ragged": ("lstm", FUSED, 2, (2, 4), {}, ("ragged", 40, 70, 6)),
    "feed": ("lstm", FUSED, 2, (3, 6), {}, ("rect", 60, 3, 6)),                                       # (its leading column is overwritten with arbitrary values)
    "graph_fused": ("lstm", FUSED, 2, (2, 4), {}, ("graph", 4, 28)),
    "graph_rnn": ("rnn", RNN4, 1, (2, 5), {"use_relu": 1}, ("graph", 4, 28)),                          # tests/test_gpu_path_find.py SHAPES[4] with a second slot
}
ROUTE_CASES = [route_case(r, nT, F) for r in ROUTES for nT, F in LAYOUTS]
ALL_CASES = ROUTE_CASES + list(EXTRA)


@functools.lru_cache(maxsize=None)
def graph():
    """the typed graph of tests/test_gpu_path_find.py with two type slots per node, its pairs and labels.  pref.node_types leaves slot 0 at the pad id for half
    of the nodes, so a step repeats an id with probability 1 / 6 on average; the share of a batch hangs on the few nodes its paths run through (seeds 23 .. 27:
    0.09 .. 0.28) and seed 31 is one whose found paths meet REPEAT_SHARE (0.45, 85 paths of 9 pairs)"""
    g = pref.make_graph(n_rand=380, n_rand_edges=900, seed=31, hub=True)
    pairs = pref.pairs_of(g, 60, seed=29)
    return g, pref.node_types(g, 2), pairs, (np.arange(len(pairs)) % 2).astype(np.float32)


def groups(counts):
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    for P in np.unique(counts):
        pairs = np.nonzero(counts == P)[0]
        yield int(P), pairs, (off[pairs][:, None] + np.arange(int(P))[None, :]).reshape(-1)


def oracle_forward(o, theta, idx, counts=None):
    """(path scores [N, C], probabilities [B, C]); counts: a ragged batch idx [N, T, F], pair b with counts[b] consecutive paths"""
    if counts is None:
        ps, _, probs = o.forward(theta, idx)
        return ps, probs
    ps, probs = np.empty((idx.shape[0], o.cfg.C)), np.empty((len(counts), o.cfg.C))
    for P, pairs, rows in groups(counts):
        a, _, c = o.forward(theta, idx[rows].reshape((len(pairs), P) + idx.shape[1:]))
        ps[rows], probs[pairs] = a, c
    return ps, probs


def oracle_backward(o, theta, idx, labels, counts=None):
    """(loss, flat gradient) of the whole batch"""
    if counts is None:
        return o.forward_backward(theta, idx, labels)[:2]
    loss, grad = 0.0, np.zeros(o.n)
    for P, pairs, rows in groups(counts):
        l, g, _ = o.forward_backward(theta, idx[rows].reshape((len(pairs), P) + idx.shape[1:]), labels[pairs], inv_batch=1.0 / len(counts))
        loss, grad = loss + l, grad + g
    return loss, grad


class Case:
    """one case: the float64 oracle, theta rounded to fp32, the inputs; the oracle's answers are computed once and shared"""

    def __init__(self, name):
        self.name = name
        if name in EXTRA:
            kind, dims, L, (nT, F), kw, data = EXTRA[name]
            self.route, self.options, self.fam_in, self.fam_out = None, {}, [], []
        else:
            self.route, lay = name.rsplit("-", 1)
            nT, F = (int(v) for v in lay.split("x"))
            kind, dims, L, pairs, P, T, kw, self.options, self.fam_in, self.fam_out = ROUTES[self.route]
            data = ("rect", pairs, P, T)
        if len(dims) == 3:
            dims = dims + (384,)
        self.kind, self.dims, self.L, self.nT, self.F, self.kw = kind, dims, L, nT, F, dict(kw)
        self.rnn_type = {"lstm": 0, "rnn": 1, "gru": 2}[kind]
        self.relu = kw.get("use_relu", 1) if kind == "rnn" else 1
        self.cdt = kw.get("compute_dtype", 0)
        self.bars = BARS["bf16" if self.cdt == 1 else "fp32"]
        self.counts = None
        self.Vt, self.Ve, self.Vr = VT, VE, VR
        if data[0] == "rect":
            self.idx, self.labels = synth.make_paths(data[1], data[2], data[3], F=F, Ve=VE, Vr=VR, num_types=nT, seed=DATA_SEED + data[1])
        elif data[0] == "ragged":
            counts = np.concatenate([synth.draw_num_paths(np.random.default_rng(5), data[1] - 1), [data[2]]]).astype(np.int32)
            self.idx, self.counts, self.labels = synth.make_ragged(len(counts), data[3], F=F, Ve=VE, Vr=VR, num_types=nT, seed=DATA_SEED, counts=counts)
        else:
            g, nt, pairs, labels = graph()
            self.Vt, self.Ve, self.Vr = pref.VT, g["Ve"], pref.VR
            idx, counts, _ = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, pref.VR, pref.VT, pref.END_REL, pairs, 1, 3, data[2], data[1], F=F, threads=4)
            self.idx, self.counts, self.labels = idx, counts[counts > 0], labels[counts > 0]
            self.find_args = (1, 3, data[2], data[1])
        if name == "feed":   # the unused leading column holds anything, ids out of every range included: whatever validates, plans or gathers from column 0 shows
            lead = F - nT - 2
            rng = np.random.default_rng(DATA_SEED)
            junk = rng.integers(1, 1 << 20, size=self.idx.shape[:3] + (lead,), dtype=np.int32)
            self.idx[..., :lead] = np.where(rng.random(junk.shape) < 0.1, rng.integers(-3, 1, size=junk.shape, dtype=np.int32), junk)   # (a tenth: 0 and below)
        dt, de, dr, H = dims
        cfg = dict(Vt=self.Vt, Ve=self.Ve, Vr=self.Vr, dt=dt, de=de, dr=dr, H=H, L=L, rnn_type=self.rnn_type, use_relu=self.relu)
        self.o64 = Oracle(make_cfg(F=F, numTypes=nT, **cfg), np.float64)
        self.o1 = Oracle(make_cfg(F=3, numTypes=1, **cfg), np.float64)
        theta = self.o64.init_params(PARAM_SEED, 0.05)
        off, shp = self.o64.layout()["type_emb"]
        theta[off:off + int(np.prod(shp))] *= TYPE_SCALE
        if kind == "rnn":
            self.o64.zero_pad(theta)
        self.theta = theta.astype(np.float32).astype(np.float64)
        self.n_paths = int(self.idx.shape[0] if self.counts is not None else self.idx.shape[0] * self.idx.shape[1])
        self._fwd = self._bwd = self._guards = None

    def forward(self):
        if self._fwd is None:
            self._fwd = oracle_forward(self.o64, self.theta, self.idx, self.counts)
        return self._fwd

    def backward(self):
        if self._bwd is None:
            self._bwd = oracle_backward(self.o64, self.theta, self.idx, self.labels, self.counts)
        return self._bwd

    def tensor(self, flat, nm):
        off, shp = self.o64.layout()[nm]
        return np.asarray(flat)[off:off + int(np.prod(shp))].reshape(shp)

    def repeat_share(self):
        """share of the non-pad steps whose type slots hold one id twice"""
        c0 = self.F - self.nT - 2
        slots = np.sort(self.idx[..., c0:c0 + self.nT].reshape(-1, self.nT), axis=1)
        real = self.idx[..., self.F - 2].reshape(-1) != self.Ve
        return float(np.mean(np.any(slots[real, 1:] == slots[real, :-1], axis=1)))

    def guards(self):
        if self._guards is None:
            idx1 = np.ascontiguousarray(self.idx[..., [self.F - self.nT - 2, self.F - 2, self.F - 1]])
            g_fwd = rel_inf(oracle_forward(self.o1, self.theta, idx1, self.counts)[0], self.forward()[0])
            g1 = oracle_backward(self.o1, self.theta, idx1, self.labels, self.counts)[1]
            g_bwd = rel_inf(self.tensor(g1, "type_emb"), self.tensor(self.backward()[1], "type_emb"))
            self._guards = dict(case=self.name, guard_fwd=g_fwd, guard_bwd=g_bwd, repeat=self.repeat_share(), paths=self.n_paths)
        return self._guards


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def check(c):
    """the three conditions of the module docstring -> the measured guards.  Returns with "scores_check_slots" False only for SCORES_ARE_NO_SLOT_CHECK"""
    m = dict(c.guards())
    assert c.o1.n == c.o64.n, m
    assert c.n_paths <= 320, m
    assert m["repeat"] >= REPEAT_SHARE, m
    assert m["guard_bwd"] >= MARGIN * c.bars["grad"], m
    m["scores_check_slots"] = bool(m["guard_fwd"] >= MARGIN * c.bars["score"])
    if not m["scores_check_slots"]:
        assert c.route in SCORES_ARE_NO_SLOT_CHECK, m
    return m
