"""-m gpu: the gate functions of the recurrent cells over EVERY finite float32 (about 4.3e9 arguments per function), against the double-precision
sigmoid 1 / (1 + exp(-x)) and tanh computed on the device (tests/gate_math_sweep.hip, which includes the kernels' own headers):
  * exp_fast family (kprn_amd/csrc/gate_math.h sigm / tanh_fast: gemm_tiled.hip, layer_f32_persist.hip): absolute error <= 1.5e-7;
  * exp2 / rcp family (gate_math.h sigm_e2 / tanh_e2: the bf16 pipelines) and the fused kernels' fast_sigmoid / fast_tanh
    (lstm_fused_common.h): the bound measured by this sweep, written next to each function;
  * for all of them: no inf / NaN result and every result inside [0, 1] / [-1, 1].
The exp_fast family once returned NaN from 128 ln2 = 88.7228 on (v_exp_f32 gives +inf, the residual fma(inf, <= 0, inf) is NaN); its argument clamp
must leave every result the unclamped form computed finite unchanged, so that no parity number of the suite moves."""
import ctypes
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kprn_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "gate_math_sweep.hip")
LIB = os.path.join(ROOT, "tests", "_build", "libgate_math_sweep.so")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("gate_math.h", "lstm_fused_common.h", "kprn_internal.h")]

# name -> (id in gate_math_sweep.hip, largest absolute error allowed)
FUNCS = {"sigm": (0, 1.5e-7), "tanh_fast": (1, 1.5e-7),                 # measured 1.096e-7 / 1.248e-7
         "sigm_e2": (2, 1.2e-7), "tanh_e2": (3, 2.3e-7),            # measured 1.108e-7 / 2.216e-7
         "fast_sigmoid": (4, 1.2e-7), "fast_tanh": (5, 2.3e-7)}     # measured 1.108e-7 / 2.216e-7
UNCLAMPED = {"sigm": 6, "tanh_fast": 7}


def build_sweep():
    if os.path.exists(LIB) and os.path.getmtime(LIB) > max(os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "-x", "hip", "--offload-arch=gfx950", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])
    return LIB


_CACHE = {}


def sweep(fn):
    """{err, worst, nonfinite, outside, changed, old_nonfinite} of one function id over every finite float32"""
    if fn not in _CACHE:
        lib = ctypes.CDLL(build_sweep())
        res = (ctypes.c_double * 2)()
        cnt = (ctypes.c_ulonglong * 4)()
        rc = lib.gate_sweep(ctypes.c_int(fn), res, cnt)
        assert rc == 0, f"gate_sweep({fn}) failed: HIP error {rc}"
        _CACHE[fn] = dict(err=res[0], worst=res[1], nonfinite=cnt[0], outside=cnt[1], changed=cnt[2], old_nonfinite=cnt[3])
    return _CACHE[fn]


@pytest.mark.parametrize("name", list(FUNCS))
def test_every_finite_float32_against_double_precision(name):
    fn, bound = FUNCS[name]
    r = sweep(fn)
    print(f"{name}: max abs err {r['err']:.4g} at x = {r['worst']!r}, non-finite {r['nonfinite']}, outside the range {r['outside']}")
    assert r["nonfinite"] == 0, (name, r)
    assert r["outside"] == 0, (name, r)
    assert r["err"] <= bound, (name, r)


@pytest.mark.parametrize("name", list(UNCLAMPED))
def test_the_argument_clamp_changes_no_result_that_was_finite(name):
    """sigm for x >= -88.72 and tanh_fast everywhere: bit-identical to the unclamped exp_fast wherever that one was finite.  The unclamped
    form itself must show the failure the clamp is there for (sigm: NaN for a third of x in [-130, -88.72]; both: |x| beyond ~1e38)."""
    fn, _ = FUNCS[name]
    r = sweep(fn)
    old = sweep(UNCLAMPED[name])
    print(f"{name}: results changed by the clamp {r['changed']}, non-finite results of the unclamped form {r['old_nonfinite']} "
          f"(its own sweep: {old['nonfinite']} non-finite, max abs err {old['err']:.4g})")
    assert r["changed"] == 0, (name, r)
    assert r["old_nonfinite"] == old["nonfinite"] > 0, (name, r, old)
