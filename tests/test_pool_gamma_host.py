"""not gpu: the pooling temperature (include/kprn.h "pooling temperature") on the host -- the numpy restatement (tests/pool_gamma_ref.py) against the
unmodified float64 oracle run on the scaled head, kprn_host_explain_gamma against the restatement, its refusals, the twin as a stand-alone program under the
host sanitizers, and the command line's refusal.

Bounds.  Indices and scores: equality.  Shares against float64 on the same fp32 scores: tests/test_explain_host.py derives (a + 8) * 2^-24 absolute for the
plain LogSumExp (a = the longest chain of additions).  Under a temperature the exponent t_q = (s_q - m) * ig carries up to three more roundings (the
subtraction is counted there; ig itself, and the product), each relative to t_q, so expf(t_q) is off by 3 * 2^-24 |t_q| relative.  For a share w_q that is
w_q |t_q| <= 1 / e absolute from its own exponent, and sum_q w_q |t_q| <= ln(cnt) relative through the sum (entropy: -sum w ln w = ln(sum) + sum w |t|
with sum >= 1).  gamma_bound(cnt) = bound(cnt) + 3 (1 + ln cnt) 2^-24; at gamma = 1 the products are exact and bound(cnt) itself is asserted.
pooled: the sum's relative error becomes absolute through the logarithm, plus 2^-22 * max(1, |pooled|, |m| / gamma) for logf, the product m * ig (ig's
rounding and its own) and the last addition."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import Oracle, make_cfg

from . import pool_gamma_ref as ref
from .test_explain_host import bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 28, 29, 64, 65, 449, 4096)
GAMMAS = (1e-3, 0.1, 0.5, 1.0, 2.0, 1e3)
C_ = 3
KEYS = ("path_idx", "path_score", "path_weight", "pooled", "probs")


def gamma_bound(cnt, gamma):
    return bound(cnt) if gamma == 1.0 else bound(cnt) + 3.0 * (1.0 + np.log(cnt)) * 2.0 ** -24


def g32(gamma):
    """the temperature the twin sees: the float argument, read back as float64"""
    return float(np.float32(gamma))


# ---- the restatement against the oracle through the scaled head ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("init,gamma", [(0.5, 0.5), (0.5, 2.0), (0.3, 0.1), (0.5, 0.25)])
def test_restatement_equals_the_oracle_on_the_scaled_head(L, init, gamma):
    """numpy log sum exp(s / gamma) over the oracle's own path scores = the unmodified LogSumExp oracle on theta' (head divided by gamma): pooled,
    probabilities, and d loss / d theta through the 1 / gamma map of the head (float64: 1e-12)"""
    o64 = Oracle(make_cfg(Vt=6, Ve=300, Vr=9, dt=16, de=32, dr=16, H=64, L=L, reducer=2), np.float64)
    theta = o64.init_params(1, init)
    lay = o64.layout()
    theta_p = ref.scaled_head(theta, lay, gamma)
    for P in (28, 70):
        idx, labels = synth.make_paths(9, P, 6, Ve=300, seed=41)
        off = np.arange(10) * P
        ps, _, _ = o64.forward(theta, idx)
        _, pooled_p, probs_p = o64.forward(theta_p, idx)
        for class_id in (1, 3):
            pooled, prob, shares, dS = ref.pool_pairs(ps[:, class_id - 1], off, gamma)
            assert np.max(np.abs(pooled - pooled_p[:, class_id - 1])) < 1e-12
            assert np.max(np.abs(prob - probs_p[:, class_id - 1])) < 1e-12
            for b in range(9):
                assert abs(shares[off[b]:off[b + 1]].sum() - 1.0) < 1e-12 and abs(dS[off[b]:off[b + 1]].sum() - 1.0 / gamma) < 1e-12 / gamma
            # the gradient of the BCE loss with respect to the head's bias, by hand from dS, against the mapped oracle gradient
            _, g_p, _ = o64.forward_backward(theta_p, idx, labels, class_id=class_id)
            g = ref.map_head_grads(g_p, lay, gamma)
            dy = (prob - labels) / 9.0
            ob, _ = lay["out.bias"]
            want = float(np.sum(np.repeat(dy, P) * dS))
            assert abs(g[ob + class_id - 1] - want) < 1e-12 * max(1.0, abs(want))


def test_the_parity_cases_meet_both_conditions_on_the_oracle():
    """(init 0.5, gamma 0.5), (0.5, 2) and (0.3, 0.1) spread the shares and keep every label-0 pair's |pooled| at most 6; (0.5, 0.25) spreads only.
    (At gamma = 2 the share condition is 1.5 : 1, not 3 : 1: pool_gamma_ref.share_ratio_bar says why.)"""
    for L, init, gamma, both in ((2, 0.5, 0.5, True), (2, 0.5, 2.0, True), (2, 0.3, 0.1, True), (2, 0.5, 0.25, False)):
        o64 = Oracle(make_cfg(Vt=6, Ve=300, Vr=9, dt=16, de=32, dr=16, H=64, L=L, reducer=2), np.float64)
        theta = o64.init_params(1, init).astype(np.float32).astype(np.float64)
        idx, labels = synth.make_paths(17, 28, 6, Ve=300, seed=41)
        ps, _, _ = o64.forward(theta, idx)
        spread, worst = ref.spread_conditions(ps[:, 0], np.arange(18) * 28, labels, gamma)
        print("init %.1f gamma %.2f: share of pairs with a ratio >= 3: %.2f, largest label-0 |pooled| %.2f" % (init, gamma, spread, worst))
        assert spread >= 0.5
        if both:
            assert worst <= 6.0


# ---- the twin against the restatement -----------------------------------------------------------------------------------------------------------
def scores_and_offsets(rng, spread=1.0):
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    sc = (rng.normal(0, spread, (int(off[-1]), C_))).astype(np.float32)
    return sc, off


def check_twin(res, sc, off, class_id, gamma, M):
    g = g32(gamma)
    for b in range(len(off) - 1):
        s32 = sc[off[b]:off[b + 1], class_id - 1]
        cnt = len(s32)
        r = ref.pool(s32, g)
        o = ref.order(s32)
        n = min(M, cnt)
        assert np.array_equal(res["path_idx"][b, :n], o[:n]), (b, cnt)
        assert np.all(res["path_idx"][b, n:] == -1) and np.all(res["path_score"][b, n:] == 0) and np.all(res["path_weight"][b, n:] == 0)
        assert res["path_score"][b, :n].tobytes() == s32[o[:n]].tobytes()
        tol = gamma_bound(cnt, gamma)
        got = res["path_weight"][b, :n].astype(np.float64)
        err = float(np.abs(got - r["shares"][o[:n]]).max())
        assert err <= tol, (b, cnt, gamma, err, tol)
        assert np.all(np.isfinite(got)) and np.all(got >= 0) and np.all(got <= 1)
        if cnt <= M:   # every share is there: they sum to 1 within fp32 summation error of the count
            assert abs(got.sum() - 1.0) <= tol + cnt * 2.0 ** -24, (b, cnt, gamma, got.sum())
        ptol = tol + 2.0 ** -22 * max(1.0, abs(r["pooled"]), abs(float(s32.max())) / g)
        assert abs(float(res["pooled"][b]) - r["pooled"]) <= ptol, (b, cnt, gamma, res["pooled"][b], r["pooled"])
        p = 1.0 / (1.0 + np.exp(-np.float64(res["pooled"][b])))
        assert abs(float(res["probs"][b]) - p) <= 2.0 ** -22


@pytest.mark.parametrize("gamma", GAMMAS)
def test_twin_equals_the_restatement(gamma):
    rng = np.random.default_rng(23)
    sc, off = scores_and_offsets(rng)
    for class_id in (1, 3):
        for M in (1, 32):
            check_twin(_ffi.host_explain(sc, off, class_id, 2, 5, M, gamma=gamma), sc, off, class_id, gamma, M)
    # every share of the longest pairs, 32 places at a time is not possible (M <= 32): the sum over all shares is checked where cnt <= 32 above, and for the
    # long pairs through pooled, which is the logarithm of the same sum


def test_gamma_one_is_kprn_host_explain_bit_for_bit():
    rng = np.random.default_rng(24)
    for spread in (1.0, 30.0):
        sc, off = scores_and_offsets(rng, spread)
        for reducer in (2, 0, 1):
            a = _ffi.host_explain(sc, off, 2, reducer, 5, 32, gamma=1.0)
            n = len(off) - 1
            out = {k: np.empty((n, 32) if k.startswith("path") else (n,), np.int32 if k == "path_idx" else np.float32) for k in KEYS}
            rc = _ffi.lib().kprn_host_explain(_ffi._fp(sc), _ffi._fp(off), n, C_, 2, reducer, 5, None, n, 32, *[_ffi._fp(out[k]) for k in KEYS])
            assert rc == 0
            for k in KEYS:
                assert a[k].tobytes() == out[k].tobytes(), (reducer, k)


def test_ties_and_a_nan_score():
    s = np.array([0.5, 2.0, 0.5, 2.0, -0.0, 0.0, 2.0], np.float32)[:, None]
    off = np.array([0, 7], np.int32)
    for gamma in (0.1, 2.0):
        res = _ffi.host_explain(s, off, 1, 2, 5, 7, gamma=gamma)
        assert res["path_idx"][0].tolist() == [1, 3, 6, 0, 2, 4, 5]
        w = res["path_weight"][0]
        assert w[0] == w[1] == w[2] and w[3] == w[4] and w[5] == w[6]          # equal scores take equal shares
        check_twin(res, s, off, 1, gamma, 7)
    s = np.array([1.0, np.nan, 3.0, 2.0], np.float32)[:, None]
    for gamma in (0.5, 1.0):
        res = _ffi.host_explain(s, np.array([0, 4], np.int32), 1, 2, 5, 4, gamma=gamma)
        assert res["path_idx"][0].tolist() == [2, 3, 0, 1]                     # the NaN sorts last
        assert res["path_score"][0, :3].tolist() == [3.0, 2.0, 1.0] and np.isnan(res["path_score"][0, 3])
        assert np.isnan(res["pooled"][0]) and np.all(np.isnan(res["path_weight"][0]))   # expf(NaN) poisons the sum: as at gamma = 1


def test_the_smallest_gamma_with_a_spread_of_one():
    """gamma = 1e-3, scores 0 .. 1: the exponents reach -1000, expf underflows to 0 and nothing is NaN or inf; where the runner-up is 1 / 28 or more
    below the best (t <= -35) the top share is exactly 1"""
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    rng = np.random.default_rng(25)
    col = np.concatenate([rng.permutation(np.linspace(0.0, 1.0, c)) if c > 1 else np.array([0.5]) for c in COUNTS]).astype(np.float32)
    sc = np.stack([col, col], axis=1)
    res = _ffi.host_explain(sc, off, 1, 2, 5, 32, gamma=1e-3)
    for k in KEYS:
        assert np.all(np.isfinite(res[k])), k
    for b, c in enumerate(COUNTS):
        assert res["path_weight"][b, 0] == res["path_weight"][b].max()
        if c <= 29:
            assert res["path_weight"][b, 0] == 1.0 and np.all(res["path_weight"][b, 1:] <= 1e-15), (c, res["path_weight"][b, :3])
        assert res["probs"][b] == 1.0 or c == 1
    check_twin(res, sc, off, 1, 1e-3, 32)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def poisoned_call(gamma, reducer=2, K=5, M=3):
    sc = np.random.default_rng(1).normal(0, 1, (20, C_)).astype(np.float32)
    off = np.array([0, 5, 6, 20], np.int32)
    out = dict(path_idx=np.full((3, M), -7, np.int32), path_score=np.full((3, M), -7, np.float32), path_weight=np.full((3, M), -7, np.float32),
               pooled=np.full(3, -7, np.float32), probs=np.full(3, -7, np.float32))
    try:
        _ffi.host_explain(sc, off, 1, reducer, K, M, out=out, gamma=gamma)
        code = 0
    except _ffi.KprnError as e:
        code = e.code
    return code, all(bool(np.all(v == -7)) for v in out.values())


def test_refusals_write_nothing():
    assert poisoned_call(0.5) == (0, False)
    for gamma in (0.0, -0.5, -1.0, float("nan"), float("inf"), -float("inf"), 9.99e-4, 1000.5, 1e-30, 3e38):
        assert poisoned_call(gamma) == (_ffi.E_ARG, True), gamma
    for gamma in (1e-3, 1e3, 1.0):
        assert poisoned_call(gamma) == (0, False), gamma
    for reducer in (0, 1):
        assert poisoned_call(0.5, reducer=reducer) == (_ffi.E_UNSUPPORTED, True)
        assert poisoned_call(2.0, reducer=reducer) == (_ffi.E_UNSUPPORTED, True)
        assert poisoned_call(1.0, reducer=reducer) == (0, False)
    # the refusals of kprn_host_explain stay
    assert poisoned_call(0.5, reducer=3) == (_ffi.E_ARG, True)
    assert poisoned_call(0.5, M=33) == (_ffi.E_ARG, True)
    assert poisoned_call(float("nan"), reducer=0) == (_ffi.E_ARG, True)


# ---- the twin as a stand-alone program under the host sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_program(tmp_path_factory):
    """explain_paths.hip (the twin's translation unit) and tests/pool_gamma_san_main.cpp, the host side under -fsanitize=address,undefined.  The program
    calls the host twin only: no GPU is opened, nothing is preloaded."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc), "no hipcc"
    exe = str(tmp_path_factory.mktemp("san") / "pool_gamma_san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-w"] + [w for f in san for w in ("-Xarch_host", f)] + \
          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kprn_amd", "csrc"), os.path.join(ROOT, "kprn_amd", "csrc", "explain_paths.hip"),
           os.path.join(ROOT, "tests", "pool_gamma_san_main.cpp"), "-fsanitize=address,undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_san(exe, tmp_path, sc, off, class_id, reducer, K, M, gamma, pairs=None):
    sc, off = np.ascontiguousarray(sc, np.float32), np.ascontiguousarray(off, np.int32)
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
    n = len(off) - 1 if pr is None else len(pr)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([sc.shape[0], sc.shape[1], len(off) - 1, class_id, reducer, K, n, M, 0 if pr is None else 1], np.int32).tobytes())
        f.write(np.float32(gamma).tobytes())
        f.write(sc.tobytes())
        f.write(off.tobytes())
        if pr is not None:
            f.write(pr.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    m = max(M, 1)
    rc = int(np.frombuffer(raw[:4], np.int32)[0])
    parts, at = {}, 4
    for k, cnt, dt in (("path_idx", n * m, np.int32), ("path_score", n * m, np.float32), ("path_weight", n * m, np.float32), ("pooled", n, np.float32),
                       ("probs", n, np.float32)):
        parts[k] = np.frombuffer(raw[at:at + 4 * cnt], dt).reshape((n, m) if k.startswith("path") else (n,))
        at += 4 * cnt
    assert at == len(raw)
    return rc, parts


def test_sanitized_twin_equals_the_library(san_program, tmp_path):
    rng = np.random.default_rng(26)
    sc, off = scores_and_offsets(rng)
    for gamma, reducer, M, pairs in ((0.5, 2, 32, None), (1e-3, 2, 1, None), (1e3, 2, 3, [7, 0, 7, 3]), (1.0, 0, 5, None), (1.0, 1, 32, [6])):
        rc, got = run_san(san_program, tmp_path, sc, off, 2, reducer, 5, M, gamma, pairs)
        want = _ffi.host_explain(sc, off, 2, reducer, 5, M, pairs=pairs, gamma=gamma)
        assert rc == 0
        for k in KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (gamma, reducer, k)


def test_sanitized_twin_refuses_cleanly(san_program, tmp_path):
    rng = np.random.default_rng(27)
    sc, off = scores_and_offsets(rng)
    for gamma, reducer, M, status in ((0.0, 2, 3, _ffi.E_ARG), (float("nan"), 2, 3, _ffi.E_ARG), (2000.0, 2, 3, _ffi.E_ARG), (0.5, 0, 3, _ffi.E_UNSUPPORTED),
                                      (0.5, 1, 3, _ffi.E_UNSUPPORTED), (0.5, 2, 33, _ffi.E_ARG)):
        rc, got = run_san(san_program, tmp_path, sc, off, 1, reducer, 5, M, gamma)
        assert rc == status and all(bool(np.all(v == -77)) for v in got.values()), (gamma, reducer, M, rc)


# ---- command line -----------------------------------------------------------------------------------------------------------------------------------
def test_gamma_beside_another_reducer_is_refused_before_an_engine_exists():
    """-gamma 0.5 -topK 0: the message names both flags; no engine exists yet (this runs without a GPU, where creating one fails differently)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for top, name in (("0", "max pooling"), ("1", "TopK + Mean")):
        r = subprocess.run([sys.executable, "-m", "kprn_amd.train", "-gamma", "0.5", "-topK", top], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode != 0 and "-gamma" in r.stderr and "-topK" in r.stderr and name in r.stderr, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "kprn_amd.train", "-gamma", "0", "-topK", "2"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "-gamma must be in" in r.stderr, r.stderr[-2000:]
    for mod, needs in (("kprn_amd.score", ["-input_dir", "nowhere"]), ("kprn_amd.recommend", ["-interaction_rel", "rate", "-kg", "nowhere.tsv", "-vocab_dir", "nowhere", "-user", "u"])):
        r = subprocess.run([sys.executable, "-m", mod, "-gamma", "0.5", "-top_k", "0"] + needs, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode != 0 and "-gamma" in r.stderr and "-top_k" in r.stderr, (mod, r.stderr[-2000:])
    from kprn_amd import model
    assert model.parse_flags(["-gamma", "0.5", "-topK", "2"]).gamma == 0.5 and model.parse_flags([]).gamma is None
    assert model.parse_flags(["-gamma", "1", "-topK", "0"]).gamma == 1.0
