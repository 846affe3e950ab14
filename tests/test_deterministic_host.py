"""not gpu: the host side of option "deterministic"  -- the training flag, the CPU emulation of the new summation orders against
float64, and the register bounds of tests/test_hazards.py for the deterministic instantiations of the fused backward."""
import os
import re
import sys

import numpy as np

from kprn_amd import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

FLAGS = "-rnnType lstm -useAdam 1 -topK 2 -numLayers 2 -regularize 0"


def test_training_flag_carries_the_option_and_defaults_to_off():
    assert model.parse_flags(FLAGS.split()).deterministic == 0
    assert model.parse_flags((FLAGS + " -deterministic 1").split()).deterministic == 1
    assert model.parse_flags([]).deterministic == 0


def test_build_engine_sets_the_option(monkeypatch):
    seen = []

    class Fake:
        def __init__(self, *a, **k):
            pass

        def set_option(self, key, value):
            seen.append((key, value))
    monkeypatch.setattr(model._ffi, "Engine", Fake)
    base = FLAGS + " -numFeatureTemplates 3 -numEntityTypes 1 -includeEntity 1"
    model.build_engine(model.parse_flags(base.split()))
    assert seen == []
    model.build_engine(model.parse_flags((base + " -deterministic 1").split()))
    assert seen == [("deterministic", "1")]


def _owner_sum(parts):
    """the entity gradient's owner pass / the slab joins: one running fp32 sum in index order"""
    acc = np.float32(parts[0])
    for p in parts[1:]:
        acc = np.float32(acc + np.float32(p))
    return acc


def _slab_reduce_ny1(slabs):
    """bidx::slab_reduce_block with one range: slab s goes to accumulator s & 3 in ascending order, then (a0 + a1) + (a2 + a3)"""
    acc = [np.float32(0)] * 4
    for s, v in enumerate(slabs):
        acc[s & 3] = np.float32(acc[s & 3] + np.float32(v))
    return np.float32(np.float32(acc[0] + acc[1]) + np.float32(acc[2] + acc[3]))


def test_fixed_order_sums_are_as_close_to_float64_as_any_order_of_the_same_partials():
    """the orders DESIGN.md 3.11 writes down, emulated in fp32 against the float64 sum of the same partials: recursive summation of n terms is within
    (n - 1) u sum |x_i| of the exact sum, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) -- the bound ANY order of these
    additions has, the atomics' included; the four-accumulator slab reduce adds fewer terms per chain and meets it too.  Sizes: two partials, a hub row of the
    test batch (7 segments), the bench batch's pad row (750), five and 256 workgroup slabs"""
    rng = np.random.default_rng(0)
    eps = float(np.finfo(np.float32).eps)
    for n, f in ((2, _owner_sum), (7, _owner_sum), (750, _owner_sum), (5, _slab_reduce_ny1), (256, _slab_reduce_ny1)):
        parts = rng.standard_normal(n).astype(np.float32)
        want = float(np.sum(parts.astype(np.float64)))
        bound = (n - 1) * 0.5 * eps * float(np.sum(np.abs(parts.astype(np.float64))))
        assert abs(float(f(parts)) - want) <= bound, (n, f.__name__)
    # three partials do not commute: what the atomics left open (two orders of the same three addends, different bits)
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    assert np.float32(np.float32(a + b) + c) != np.float32(a + np.float32(b + c))


def test_register_bounds_hold_for_the_deterministic_backward_kernels():
    """the bounds of tests/test_hazards.py::test_register_spills_of_the_persistent_kernels, per instantiation, for the k_lstm_bwd_det twins (the same bodies
    with a plain-store flush): spills as in the default kernels, and none inside a block that holds a step's MFMAs"""
    text = chk.compile_isa(os.path.join(ROOT, "kprn_amd", "csrc", "lstm_fused_bwd.hip"))
    res = {k: v for k, v in chk.kernel_resources(text).items() if re.search(r"k_lstm_bwd_detI", k)}
    assert len(res) == 6, sorted(res)
    for k, v in res.items():
        assert v["vgpr_count"] <= 512
        if "k_lstm_bwd_detILb1ELb1E" in k:
            assert v["vgpr_spill_count"] <= 80, (k, v)
        elif "k_lstm_bwd_detILb1ELb0E" in k:
            assert v["vgpr_spill_count"] <= 64, (k, v)
        else:
            assert v["vgpr_spill_count"] <= 8, (k, v)
    seen = 0
    for km in re.finditer(r"\n(_ZN5fused\d+k_lstm_bwd_detIL\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S):
        if "Li4ELb" not in km.group(1):
            continue
        blocks = re.split(r"\n\.LBB\d+_\d+:", km.group(2))
        hot = [b for b in blocks if len(re.findall(r"\bv_mfma", b)) >= 60]
        assert len(hot) >= 4, (km.group(1), len(hot))
        for b in hot:
            assert not re.findall(r"scratch_store", b), km.group(1)
            assert len(re.findall(r"scratch_load", b)) <= (4 if "detILb1E" in km.group(1) else 1), km.group(1)
        seen += 1
    assert seen >= 4
