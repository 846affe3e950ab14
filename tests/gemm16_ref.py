"""Inputs and references for the bf16 products of gemm_bf16.hip (tests/test_gpu_gemm16_products.py; checked on the host by
tests/test_gemm16_inputs_host.py).  Plain numpy.

C[M][N] (fp32) = or += bf16(A)[M][K] bf16(B)[N][K]^T (+ bias) with fp32 accumulation.

Integer class: operand entries are integers in [-15, 15] (exact in bf16), C_in and the bias integers in [-1000, 1000].  Every partial sum of every
accumulation order is then an integer below 2^24, hence exact in fp32: the result is the SAME in every order, K split and atomic landing order, and the
test is array_equal against the integer product -- no tolerance.  (The product is formed by a float64 matmul: all its partial sums are integers below
2^53, so it is the int64 product exactly, at BLAS speed; the host test holds it equal to numpy's int64 matmul.)

Real class: standard normal entries scaled by 2^e, e drawn per row from [-6, 6], rounded to bf16 on the host, so the device's conversion is exact and the
only error left is the fp32 accumulation.  Reference: float64 matmul.  Bound per element: (K + 64) 2^-23 (|A| |B|^T) -- the textbook bound for K - 1
additions plus up to 64 atomic partial sums, with the unit roundoff doubled (2^-23 instead of 2^-24) because nobody here has established that the MFMA
accumulator rounds to nearest rather than truncating; that doubling is a supposition.  C_in of an accumulating real case is zero (the bound has no
term for it).

Operands are windows inside larger flat arrays: origin offset, row pitch, and a tail behind the last row.  Everything of A and B outside the window is
NaN (also the pitch padding inside the rows, the pad columns of a k-major A and what lies beyond its Mp columns); everything of C outside the window
is SENTINEL."""
import zlib
from dataclasses import dataclass

import numpy as np

SENTINEL = np.float32(-7777.25)
TAIL = 40   # elements behind every window's last row


@dataclass(frozen=True)
class Case:
    name: str
    route: str              # "gemm16" (dispatcher) | "x" | "xt" | "k_gemm16"
    M: int                  # rows of C (xt: T * Nv)
    N: int
    K: int
    kernel: str             # what the launcher must report: declined | k_gemm16_small | k_gemm16_big | x | r | p | xt
    nsplit: int             # ... worked out by hand from the planner text (gemm16_plain / gemm16x / gemm16xt of gemm_bf16.hip)
    kchunk: int
    accumulate: bool = False
    split_k: int = 1
    sx_min: int = 1
    n_lo: int = 0
    k_lo: int = 0           # rows n >= n_lo of B are zero for k < k_lo (the generator makes them so)
    pitched: bool = False   # lda = K + 8, ldb = K + 24, ldc = N + 3 and non-zero window origins
    ldc: int = 0            # 0: N (N + 3 when pitched)
    bias: bool = False
    opts: tuple = ()        # (("bf16_gemm_touch", "6"), ...): options set for the case, put back to "0" behind it
    tile_env: str = ""      # KPRN_BF16_TILE
    T: int = 0              # xt: steps, Np padded / Nv valid paths per step, ldat = T Np + ldat_extra
    Np: int = 0
    Nv: int = 0
    ldat_extra: int = 0
    dx_t_ok: bool = False   # xt: what dx_from_transposed_ok must say
    cls: str = "int"        # "int" | "real"


def to_bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def geometry(c):
    """pitches, origins and element counts of the three arrays"""
    g = {}
    if c.route == "xt":
        Mp = c.T * c.Np
        g["Mp"] = Mp
        g["lda"] = Mp + c.ldat_extra
        g["a_off"] = 16 if c.pitched else 0
        g["a_count"] = g["a_off"] + c.K * g["lda"] + TAIL
    else:
        g["lda"] = c.K + (8 if c.pitched else 0)
        g["a_off"] = 16 if c.pitched else 0
        g["a_count"] = g["a_off"] + c.M * g["lda"] + TAIL
    g["ldb"] = c.K + (24 if c.pitched else 0)
    g["b_off"] = 8 if c.pitched else 0
    g["b_count"] = g["b_off"] + c.N * g["ldb"] + TAIL
    g["ldc"] = c.ldc if c.ldc else c.N + (3 if c.pitched else 0)
    g["c_off"] = 4 if c.pitched else 0
    g["c_count"] = g["c_off"] + c.M * g["ldc"] + TAIL
    return g


def _window(flat, off, rows, ld, cols):
    """the [rows][cols] window of a flat array, as a view"""
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(rows, cols), strides=(ld * flat.itemsize, flat.itemsize))


def operands(c):
    """the logical operands: A [M][K], B [N][K], C_in [M][N] (zeros for a storing form), bias [N] or None -- float32, exact in bf16 (A, B)"""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    if c.cls == "int":
        A = rng.integers(-15, 16, size=(c.M, c.K)).astype(np.float32)
        B = rng.integers(-15, 16, size=(c.N, c.K)).astype(np.float32)
        Cin = rng.integers(-1000, 1001, size=(c.M, c.N)).astype(np.float32)
        bias = rng.integers(-1000, 1001, size=c.N).astype(np.float32)
    else:
        A = to_bf16(rng.standard_normal((c.M, c.K)) * np.exp2(rng.integers(-6, 7, size=(c.M, 1))))
        B = to_bf16(rng.standard_normal((c.N, c.K)) * np.exp2(rng.integers(-6, 7, size=(c.N, 1))))
        Cin = np.zeros((c.M, c.N), np.float32)
        bias = rng.standard_normal(c.N).astype(np.float32)
    if c.k_lo > 0:
        B[c.n_lo:, :c.k_lo] = 0.0
    if not c.accumulate:
        Cin[:] = 0.0
    return A, B, Cin, (bias if c.bias else None)


def reference(c, A, B, Cin, bias):
    """-> (ref [M][N], mag [M][N] = |A| |B|^T): int64 for the integer class, float64 for the real class"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = A64 @ B64.T + Cin.astype(np.float64)
    if bias is not None:
        ref = ref + bias.astype(np.float64)[None, :]
    mag = np.abs(A64) @ np.abs(B64).T
    if c.cls == "int":
        assert np.array_equal(ref, np.rint(ref))
        return ref.astype(np.int64), mag
    return ref, mag


def real_bound(c, mag):
    return (c.K + 64) * 2.0 ** -23 * mag


def arrays(c, A, B, Cin):
    """the flat arrays the hook takes: (A_flat, B_flat, C_flat, inside) -- inside: boolean mask of C_flat's window elements"""
    g = geometry(c)
    Af = np.full(g["a_count"], np.nan, np.float32)
    Bf = np.full(g["b_count"], np.nan, np.float32)
    Cf = np.full(g["c_count"], SENTINEL, np.float32)
    if c.route == "xt":   # AT[k][step Np + path]: the Nv valid paths of every step; pad columns and everything beyond Mp stay NaN
        at = _window(Af, g["a_off"], c.K, g["lda"], g["Mp"]).reshape(c.K, c.T, c.Np)
        at[:, :, :c.Nv] = A.T.reshape(c.K, c.T, c.Nv)
    else:
        _window(Af, g["a_off"], c.M, g["lda"], c.K)[:] = A
    _window(Bf, g["b_off"], c.N, g["ldb"], c.K)[:] = B
    if c.accumulate:
        _window(Cf, g["c_off"], c.M, g["ldc"], c.N)[:] = Cin
    inside = np.zeros(g["c_count"], bool)
    _window(inside, g["c_off"], c.M, g["ldc"], c.N)[:] = True
    return Af, Bf, Cf, inside


def c_window(c, Cf):
    g = geometry(c)
    return _window(Cf, g["c_off"], c.M, g["ldc"], c.N)
