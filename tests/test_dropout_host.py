"""not gpu: the dropout generator's numpy twin against its known answers and against the library's host twin, the statistics of the masks, the yardstick
(tests/dropout_ref.py) against the float64 oracle, and the flags (-useDropout / -dropout / -dropoutSeed)."""
import numpy as np
import pytest

from kprn_amd import _ffi, model
from tests import dropout_ref as dr

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_numpy_philox_reproduces_the_known_answers(ctr, key, want):
    got = tuple(int(w) for w in dr.philox4x32_10(*ctr, *key))
    assert got == want, [hex(g) for g in got]


@pytest.mark.parametrize("seed", [0x1234567, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("p", [0.25, 0.5, 0.999, 2.0 ** -33])
def test_host_twin_equals_the_numpy_twin_bit_for_bit(seed, p):
    for Din in (48, 50):   # 50: a partial last quad
        for layer in (0, 1):
            for draw in (0, 1):
                got = _ffi.host_dropout_keep(seed, draw, layer, 6, 111, Din, p)
                want = dr.keep_mask(seed, draw, layer, 6, 111, Din, p)
                assert got.shape == want.shape == (6, 111, Din) and got.dtype == np.uint8
                assert np.array_equal(got.astype(bool), want), (seed, p, Din, layer, draw)
                if p == 2.0 ** -33:
                    assert dr.threshold(p) == 0 and got.all()   # thr = 0: everything is kept


def test_host_twin_refuses_what_the_generator_cannot_address():
    for bad in (dict(layer=-1), dict(layer=65536), dict(T=0), dict(T=65536), dict(N=0), dict(N=2 ** 32), dict(Din=0), dict(p=1.0), dict(p=-0.1)):
        a = dict(seed=1, draw=0, layer=0, T=1, N=1, Din=4, p=0.5)
        a.update(bad)
        if a["N"] > 4 or a["T"] > 4:   # (the refusal must come before anything is written: a token buffer is enough)
            keep = np.zeros(4, np.uint8)
            rc = _ffi.lib().kprn_host_dropout_keep(_ffi.C.c_uint64(1), _ffi.C.c_uint32(0), a["layer"], a["T"], _ffi.C.c_int64(a["N"]), a["Din"],
                                                   _ffi.C.c_float(a["p"]), _ffi._fp(keep))
            assert rc == _ffi.E_ARG, bad
            continue
        with pytest.raises(_ffi.KprnError) as e:
            _ffi.host_dropout_keep(**a)
        assert e.value.code == _ffi.E_ARG, bad


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_mask_statistics(p):
    """kept fraction within 4 binomial standard deviations of 1 - p; two draws differ in about 2 p (1 - p) of the elements"""
    m0 = dr.keep_mask(0x1234567, 0, 0, 6, 111, 48, p)
    m1 = dr.keep_mask(0x1234567, 1, 0, 6, 111, 48, p)
    n = m0.size
    print("kept", m0.mean(), "differ", (m0 != m1).mean())
    assert abs(m0.mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)
    d = 2 * p * (1 - p)
    assert abs((m0 != m1).mean() - d) < 4 * np.sqrt(d * (1 - d) / n)
    # layers and seeds are streams of their own
    assert (dr.keep_mask(0x1234567, 0, 1, 6, 111, 48, p) != m0).mean() > d / 2
    assert (dr.keep_mask(0x1234568, 0, 0, 6, 111, 48, p) != m0).mean() > d / 2


@pytest.mark.parametrize("relu,L", [(1, 1), (0, 1), (1, 2), (0, 2)])
def test_yardstick_with_all_ones_masks_equals_the_oracle(relu, L):
    c = dr.Case(relu, L)
    loss, grad, probs = c.reference(0, 0, 0)
    ol, og, op = c.oracle.forward_backward(c.theta, c.idx, c.labels)
    worst = {nm: dr.rel_inf(g, w) for nm, g, w in c.tensors(grad, og)}
    print("loss", abs(loss - ol), "grad", max(worst.values()))
    assert abs(loss - ol) < 1e-10
    assert np.max(np.abs(probs - op)) < 1e-12
    for nm, v in worst.items():
        assert v < 1e-12, (nm, v)


def test_yardstick_separates_dropout_from_none_and_one_flipped_element():
    """the GPU bars (loss 1e-5, gradients 2e-4 of a tensor's largest) tell the right masks from no masks and from a single wrong element"""
    c = dr.Case(0, 2)
    l0, g0, _ = c.reference(0, 0, 0)
    masks = c.masks(0x1234567, 0, 0.25)
    s = dr.scale(0.25)
    l1, g1, _ = dr.forward_backward(c.lay, c.cfg, c.theta, c.idx, c.labels, masks, s)
    assert abs(l1 - l0) > 1e-4 and all(dr.rel_inf(a, b) > 2e-4 for _, a, b in c.tensors(g1, g0))
    t, n = c.T - 1, 5   # a live step of a path (the last step is never padding)
    masks[0] = masks[0].copy()
    masks[0][t, n, 10] ^= True
    l2, g2, _ = dr.forward_backward(c.lay, c.cfg, c.theta, c.idx, c.labels, masks, s)
    assert max(dr.rel_inf(a, b) for _, a, b in c.tensors(g2, g1)) > 2e-4


def test_flags():
    base = "-numFeatureTemplates 3 -numEntityTypes 1"
    p = model.parse_flags((base + " -dropoutSeed 0x100000001").split())
    assert p.dropoutSeed == 2 ** 32 + 1 and model.parse_flags(base.split()).dropoutSeed is None
    assert model.dropout_rate(model.parse_flags((base + " -useDropout 0 -dropout 0.3").split())) == 0
    assert model.dropout_rate(model.parse_flags((base + " -useDropout 1 -dropout 0.3").split())) == 0.3
    assert model.dropout_rate(model.parse_flags((base + " -useDropout 1 -dropout 0").split())) == 0
