"""not gpu: the host side of option "deterministic" = "2"  -- the training flag's third value, what build_engine hands the library, the CPU
emulation of the slab join's order against float64, and the load pattern of the new slab producers."""
import os
import sys

import numpy as np

from kprn_amd import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

CSRC = os.path.join(ROOT, "kprn_amd", "csrc")
FLAGS = "-rnnType rnn -useAdam 1 -topK 2 -numLayers 1 -regularize 0"


def test_training_flag_takes_the_third_value():
    assert model.parse_flags((FLAGS + " -deterministic 2").split()).deterministic == 2
    assert model.parse_flags((FLAGS + " -deterministic 1").split()).deterministic == 1
    assert model.parse_flags(FLAGS.split()).deterministic == 0


def test_build_engine_passes_the_value_through(monkeypatch):
    seen = []

    class Fake:
        def __init__(self, *a, **k):
            pass

        def set_option(self, key, value):
            seen.append((key, value))
    monkeypatch.setattr(model._ffi, "Engine", Fake)
    base = FLAGS + " -numFeatureTemplates 3 -numEntityTypes 1 -includeEntity 1"
    model.build_engine(model.parse_flags((base + " -deterministic 2").split()))
    assert seen == [("deterministic", "2")]
    del seen[:]
    model.build_engine(model.parse_flags((base + " -deterministic 1").split()))
    assert seen == [("deterministic", "1")]
    del seen[:]
    model.build_engine(model.parse_flags(base.split()))
    assert seen == []


def _slab_join(slabs, c):
    """kk::slab_join: per output element one running fp32 sum ((p0 + p1) + p2) + ... over the slabs in slab order, then C += sum"""
    acc = np.zeros(slabs.shape[1:], np.float32)
    for p in slabs:
        acc = (acc + p).astype(np.float32)
    return (c + acc).astype(np.float32)


def test_slab_join_order_is_as_close_to_float64_as_any_order_of_the_same_partials():
    """3 slabs (the test batch's split count), 12 (the 4 200-path batch), 192 (an untiled product of the shipped shape): recursive summation of n terms is within
    (n - 1) u sum |x_i| of the exact sum, u = 2^-24 = eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); with the += on C that is
    n additions over n + 1 terms, inside n eps sum |p|"""
    rng = np.random.default_rng(2)
    eps = float(np.finfo(np.float32).eps)
    for n in (3, 12, 192):
        slabs = rng.standard_normal((n, 7, 5)).astype(np.float32)
        c = rng.standard_normal((7, 5)).astype(np.float32)
        got = _slab_join(slabs, c).astype(np.float64)
        want = c.astype(np.float64) + slabs.astype(np.float64).sum(0)
        bound = n * eps * (np.abs(slabs.astype(np.float64)).sum(0) + np.abs(c.astype(np.float64)))
        assert np.all(np.abs(got - want) <= bound), n
    # three partials do not commute: two splits would prove nothing about the order
    a, b, c_ = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    assert np.float32(np.float32(a + b) + c_) != np.float32(a + np.float32(b + c_))


def test_slab_producers_keep_their_loads_in_flight():
    """the slab kernels are the default bodies with another flush: their operand loads must stay a batch in flight, not a chain of round trips (the bars
    tests/test_hazards.py::test_operand_loads_are_not_a_chain_of_round_trips applies to the default kernels of the same files), and they add no scratch memory"""
    isa = chk.compile_isa(os.path.join(CSRC, "gemm_f32_slab.hip"))   # (the slab instantiations of gemm_f32_kernels.h live in this translation unit)
    res = chk.serialized_loads(isa, r"gemm_kernel\w*Lb0ELb1EEEv")
    assert len(res) == 8, sorted(res)   # two tile sizes x four layouts, fp32, SLAB
    for k, (loads, serial) in res.items():
        assert loads >= 32 and serial <= 4, (k, loads, serial)   # prologue + main loop: 16 operand loads each (no old values: a slab is stored, not added to)
    isa = chk.compile_isa(os.path.join(CSRC, "batch_index.hip"))
    res = chk.serialized_loads(isa, r"k_egrad_det_rowmajor")
    assert len(res) == 1
    for k, (loads, serial) in res.items():
        assert loads >= 64 and serial <= 8, (k, loads, serial)
    isa = chk.compile_isa(os.path.join(CSRC, "gemm_tiled.hip"))
    tiled = {k: v for k, v in chk.kernel_resources(isa).items() if "k_gemm_tiled" in k}
    slab = {k: v for k, v in tiled.items() if "ELi4ELi" in k}   # EPI_SLAB = 4
    assert len(slab) == 6, sorted(tiled)    # three layouts x two tile widths
    for k, v in slab.items():
        twin = k.replace("ELi4ELi", "ELi1ELi")   # the += epilogue's instantiation of the same layouts
        assert v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= tiled[twin]["vgpr_count"] + 8, (k, v, tiled[twin])
