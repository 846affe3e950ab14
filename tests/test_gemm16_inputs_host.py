"""not gpu: the inputs and references of tests/test_gpu_gemm16_products.py (tests/gemm16_ref.py), for EVERY case of that file: the operands are exact in
bf16, and the exactness argument of the integer class -- every partial sum an integer below 2^24 -- holds for the case as written."""
import numpy as np
import pytest
import torch

from tests import gemm16_ref as R
from tests.test_gpu_gemm16_products import CASES, REFUSALS


def test_the_gpu_file_covers_every_kernel_and_names_each_case_once():
    assert len(CASES) >= 100 and len({c.name for c in CASES}) == len(CASES) and len(REFUSALS) >= 15
    assert {c.kernel for c in CASES} == {"declined", "k_gemm16_small", "k_gemm16_big", "x", "r", "p", "xt"}
    assert {c.kernel for c in CASES if c.cls == "real"} == {"k_gemm16_small", "x", "r", "p", "xt"}


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-20, 20, 200000))).astype(np.float32)
    x[:4] = np.float32([1.00390625, 1.01171875, -1.00390625, 0.0])   # ties: to even
    assert np.array_equal(R.to_bf16(x), torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy())


def test_the_float64_route_to_the_integer_product_is_the_int64_matmul():
    c = next(c for c in CASES if c.name == "k-acc-129x130x200")
    A, B, Cin, bias = R.operands(c)
    ref, _ = R.reference(c, A, B, Cin, bias)
    assert ref.dtype == np.int64 and np.array_equal(ref, A.astype(np.int64) @ B.astype(np.int64).T + Cin.astype(np.int64))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_inputs(c):
    A, B, Cin, bias = R.operands(c)
    assert A.shape == (c.M, c.K) and B.shape == (c.N, c.K) and A.dtype == B.dtype == np.float32
    for X in (A, B):   # the device's conversion changes nothing
        assert np.array_equal(torch.from_numpy(X).to(torch.bfloat16).to(torch.float32).numpy(), X)
    ref, mag = R.reference(c, A, B, Cin, bias)
    if c.cls == "int":
        assert np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B)) and np.array_equal(Cin, np.rint(Cin))
        assert np.max(np.abs(A)) <= 15 and np.max(np.abs(B)) <= 15 and np.max(np.abs(Cin)) <= 1000
        top = float(np.max(mag)) + float(np.max(np.abs(Cin))) + (float(np.max(np.abs(bias))) if bias is not None else 0.0)
        assert top < 2.0 ** 24, top
    else:
        assert not c.bias and not np.any(Cin) and np.all(R.real_bound(c, mag) >= 0)
    if c.k_lo:   # the contract of n_lo / k_lo: those rows of B are zero below k_lo, and the rest is not all zero there
        assert not np.any(B[c.n_lo:, :c.k_lo]) and np.any(B[:c.n_lo, :c.k_lo])
    if not c.accumulate:
        assert not np.any(Cin)
    assert not (c.bias and c.accumulate)
    # the flat arrays: the window holds the operands, everything else NaN (A, B) or the sentinel (C)
    g = R.geometry(c)
    Af, Bf, Cf, inside = R.arrays(c, A, B, Cin)
    assert Af.size == g["a_count"] and Bf.size == g["b_count"] and Cf.size == g["c_count"] == inside.size
    assert np.count_nonzero(~np.isnan(Af)) == A.size and np.count_nonzero(~np.isnan(Bf)) == B.size and np.count_nonzero(inside) == c.M * c.N
    assert np.all(Cf[~inside] == R.SENTINEL) and np.isnan(Af[-1]) and np.isnan(Bf[-1])
    assert np.array_equal(R.c_window(c, Cf), Cin if c.accumulate else np.full((c.M, c.N), R.SENTINEL))
    assert g["lda"] % 8 == 0 and g["ldb"] % 8 == 0 and c.K % 8 == 0 and g["a_off"] % 8 == 0 and g["b_off"] % 8 == 0 and g["c_off"] % 4 == 0 and c.k_lo % 8 == 0
    if c.route == "xt":
        assert c.M == c.T * c.Nv and c.Np % 8 == 0 and c.Nv <= c.Np and g["lda"] >= g["Mp"]
        at = Af[g["a_off"]:g["a_off"] + c.K * g["lda"]].reshape(c.K, g["lda"])
        assert np.all(np.isnan(at[:, g["Mp"]:]))
        cols = at[:, :g["Mp"]].reshape(c.K, c.T, c.Np)
        assert np.all(np.isnan(cols[:, :, c.Nv:])) and np.array_equal(cols[:, :, :c.Nv].reshape(c.K, c.M).T, A)
    else:
        assert np.array_equal(Af[g["a_off"]:g["a_off"] + c.M * g["lda"]].reshape(c.M, g["lda"])[:, :c.K], A)
    assert np.array_equal(Bf[g["b_off"]:g["b_off"] + c.N * g["ldb"]].reshape(c.N, g["ldb"])[:, :c.K], B)
