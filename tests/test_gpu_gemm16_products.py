"""gpu: the bf16 products of gemm_bf16.hip one launch at a time, through kprn_debug_gemm16_run -- k_gemm16 (both tile geometries; store, bias, += and
atomic split-K), gx::k_gemm16x / r / p (split-K ranges, counted waits, n_lo / k_lo) and gx::k_gemm16xt (pad-column remap), at the smallest shapes that
reach each tile edge, K tail and range count.

Integer class (tests/gemm16_ref.py): operands are small integers, every partial sum is an integer below 2^24, so the result is the same in every
accumulation order, split and atomic landing order: array_equal against the integer product, no tolerance.  Every case checks (1) the M x N window,
(2) every element of the C array outside it, bit for bit against the sentinel (pitch padding, the rows behind M, and A / B surrounded by NaN: anything
read from outside an operand window poisons the window), (3) the kernel, the number of K ranges and their width the launcher reports -- worked out by
hand from the planner text and written into the case: a case that lands on another kernel or chunk count no longer covers its edge, and fails -- and
(4) that a second launch gives identical bits.

Hand-worked plans.  gemm16x, accumulate and split_k > 1: tiles = ceil(M / bm) ceil(N / bn) (x, r: 256 x 128; p: 256 x 256); of the sx in sx_min .. 8 with
8 sx <= max(split_k, 8) the first with the least ceil(tiles sx / 32) / sx; ranges asked = 8 sx; kchunk = ceil(K / asked) rounded up to bk (x, r: 64, p: 32);
nsplit = ceil(K / kchunk).  split_k = 1024: 1 and 3 tiles -> sx 8 -> 64 asked; 6 tiles -> sx 5 (ceil(30 / 32) / 5 = 0.2 beats 2 / 8) -> 40 asked, with
sx_min 8 -> 64.  split_k = 8 -> sx 1 -> 8 asked.  gemm16_plain (k_gemm16), accumulate and split_k > 1: tiles of 128 x 128, asked = min(split_k,
ceil(768 / tiles)), kchunk = ceil(K / asked) rounded up to 64, nsplit = ceil(K / kchunk); K <= 64 always gives one range.
Note K = 12 328 at 64 asked: ceil(12 328 / 64) = 193 rounds up to 256, so the launch has 48 ranges of four chunks and one of 40 (a chunk with a tail
of 40), not 64 ranges of three; at 40 asked it has 38 ranges of five chunks and one of 168 (three chunks, the last 40 wide).  K = 8 192 and 8 200 are
added for the ranges of exactly two and three chunks."""
import numpy as np
import pytest

from tests import gemm16_ref as R
from tests.gemm16_ref import Case


def _up(x, m):
    return (x + m - 1) // m * m


def _cases():
    cs = []
    # ---- x, store and accumulate with split_k = 1: one range of ceil(K / 64) chunks; (2309, 128, 64): 10 M tiles on 16 workgroups, the M-tile index wraps onto a
    # second round of XCDs and six workgroups return early
    for (M, N, K) in ((256, 128, 64), (257, 129, 72), (300, 200, 8), (2309, 128, 64)):
        for acc in (False, True):
            for pit in (False, True):
                cs.append(Case(f"x-{'acc' if acc else 'store'}-{M}x{N}x{K}{'-pitched' if pit else ''}", "x", M, N, K, "x", 1, _up(K, 64), accumulate=acc, pitched=pit))
    # ---- x, split-K (accumulate, split_k = 1024): (nsplit, kchunk) by K and ranges asked
    plan = {(64, 64): (1, 64), (64, 40): (1, 64), (72, 64): (2, 64), (72, 40): (2, 64), (520, 64): (9, 64), (520, 40): (9, 64),
            (8192, 64): (64, 128), (8200, 64): (43, 192), (12328, 64): (49, 256), (12328, 40): (39, 320)}
    for (M, N) in ((256, 128), (300, 384)):
        for K in (64, 72, 520, 12328):
            for sx_min in (1, 8):
                asked = 40 if (M == 300 and sx_min == 1) else 64
                ns, kc = plan[(K, asked)]
                cs.append(Case(f"x-split-{M}x{N}x{K}-sxmin{sx_min}", "x", M, N, K, "x", ns, kc, accumulate=True, split_k=1024, sx_min=sx_min))
        for K in (520, 12328):   # the touches change the counted waits
            for touch in ("1", "6"):
                ns, kc = plan[(K, 40 if M == 300 else 64)]
                cs.append(Case(f"x-split-{M}x{N}x{K}-touch{touch}", "x", M, N, K, "x", ns, kc, accumulate=True, split_k=1024, opts=(("bf16_gemm_touch", touch),)))
    for K in (8192, 8200):       # ranges of exactly two chunks / three chunks with a last range of 136 (tail 8)
        for touch in ("0", "1"):
            ns, kc = plan[(K, 64)]
            cs.append(Case(f"x-split-256x128x{K}-touch{touch}", "x", 256, 128, K, "x", ns, kc, accumulate=True, split_k=1024, opts=(("bf16_gemm_touch", touch),)))
    # ---- n_lo / k_lo: K = 1024 in 8 ranges of 128; k_lo = 64: inside range 0; 136: range 0 returns early for the tiles from n_lo on and range 1 starts at 136
    # (not a multiple of 64); 520: ranges 0 - 3 return early and range 4 starts at 520
    for k_lo in (64, 136, 520):
        cs.append(Case(f"x-klo{k_lo}-256x384x1024", "x", 256, 384, 1024, "x", 8, 128, accumulate=True, split_k=8, n_lo=256, k_lo=k_lo))
        cs.append(Case(f"r-klo{k_lo}-256x384x1024", "x", 256, 384, 1024, "r", 8, 128, accumulate=True, split_k=8, n_lo=256, k_lo=k_lo, opts=(("bf16_gemm_regstage", "1"),)))
        cs.append(Case(f"p-klo{k_lo}-256x512x1024", "x", 256, 512, 1024, "p", 8, 128, accumulate=True, split_k=8, n_lo=256, k_lo=k_lo, opts=(("bf16_gemm_pingpong", "1"),)))
    # n_lo = 200 inside the column tile 128 .. 255: that tile holds non-zero rows of B below k_lo and must not skip
    cs.append(Case("x-klo136-nlo200-256x384x1024", "x", 256, 384, 1024, "x", 8, 128, accumulate=True, split_k=8, n_lo=200, k_lo=136))
    cs.append(Case("r-klo136-nlo200-256x384x1024", "x", 256, 384, 1024, "r", 8, 128, accumulate=True, split_k=8, n_lo=200, k_lo=136, opts=(("bf16_gemm_regstage", "1"),)))
    # ---- r: 8 ranges asked; K = 512 c: 8 ranges of c chunks (ring period 4); + 8: kchunk = ceil((K + 8) / 8) rounded up to 64
    rplan = {512: (8, 64), 1024: (8, 128), 1536: (8, 192), 2048: (8, 256), 2560: (8, 320),
             520: (5, 128), 1032: (6, 192), 1544: (7, 256), 2056: (7, 320), 2568: (7, 384)}
    for K, (ns, kc) in sorted(rplan.items()):
        cs.append(Case(f"r-257x129x{K}", "x", 257, 129, K, "r", ns, kc, accumulate=True, split_k=8, opts=(("bf16_gemm_regstage", "1"),)))
    cs.append(Case("r-declines-K64-257x129x64", "x", 257, 129, 64, "x", 1, 64, accumulate=True, split_k=8, opts=(("bf16_gemm_regstage", "1"),)))
    # ---- p: 8 ranges asked, K tiles of 32; K = 264: kchunk = 33 -> 64, four ranges of 64 and one of 8
    pplan = {256: (8, 32), 512: (8, 64), 768: (8, 96), 1024: (8, 128), 1280: (8, 160), 264: (5, 64)}
    for (M, N) in ((256, 256), (300, 257), (512, 640)):
        for K, (ns, kc) in sorted(pplan.items()):
            cs.append(Case(f"p-{M}x{N}x{K}", "x", M, N, K, "p", ns, kc, accumulate=True, split_k=8, opts=(("bf16_gemm_pingpong", "1"),)))
    cs.append(Case("p-declines-N200-300x200x512", "x", 300, 200, 512, "x", 8, 64, accumulate=True, split_k=8, opts=(("bf16_gemm_pingpong", "1"),)))
    # ---- xt: C[(step, path)][N] from AT[K][T Np]; one range of ceil(K / 64) chunks; (3, 776, 771): Mp = 2328, 10 M tiles
    for (T, Np, Nv, N, K) in ((2, 136, 130, 128, 8), (2, 136, 136, 129, 72), (3, 776, 771, 200, 200), (1, 256, 249, 128, 64)):
        for extra in (0, 16):
            cs.append(Case(f"xt-T{T}-Np{Np}-Nv{Nv}-N{N}-K{K}-ldat+{extra}", "xt", T * Nv, N, K, "xt", 1, _up(K, 64), T=T, Np=Np, Nv=Nv, ldat_extra=extra, dx_t_ok=True,
                           pitched=(extra != 0)))
    cs.append(Case("xt-declines-Mp128", "xt", 120, 128, 64, "declined", 0, 0, T=1, Np=128, Nv=120))
    cs.append(Case("xt-declines-N127", "xt", 249, 127, 64, "declined", 0, 0, T=1, Np=256, Nv=249))
    # ---- k_gemm16 alone: ldc a multiple of 4 (with N % 4 == 0: the 16-byte stores) and not (scalar stores)
    for (M, N, K) in ((1, 1, 8), (129, 130, 200), (130, 132, 72)):
        for bias in (False, True):
            for ldc in (_up(N, 4) + 4, _up(N, 4) + 5):
                cs.append(Case(f"k-store-{M}x{N}x{K}-ldc{ldc}{'-bias' if bias else ''}", "k_gemm16", M, N, K, "k_gemm16_small", 1, _up(K, 64), ldc=ldc, bias=bias))
        cs.append(Case(f"k-acc-{M}x{N}x{K}", "k_gemm16", M, N, K, "k_gemm16_small", 1, _up(K, 64), accumulate=True, ldc=_up(N, 4) + 5))
    # atomic split-K: 4 tiles -> min(1024, 192) asked -> kchunk 64; K = 8 cannot be split (one range, still through the accumulating epilogue)
    cs.append(Case("k-atomic-1x1x8", "k_gemm16", 1, 1, 8, "k_gemm16_small", 1, 64, accumulate=True, split_k=1024))
    cs.append(Case("k-atomic-129x130x200", "k_gemm16", 129, 130, 200, "k_gemm16_small", 4, 64, accumulate=True, split_k=1024, pitched=True))
    cs.append(Case("k-atomic-130x132x72", "k_gemm16", 130, 132, 72, "k_gemm16_small", 2, 64, accumulate=True, split_k=1024))
    cs.append(Case("k-store-1025x128x64", "k_gemm16", 1025, 128, 64, "k_gemm16_small", 1, 64))   # 9 M tiles
    for (M, N, K) in ((257, 260, 72), (256, 256, 8)):   # the 256-wide geometry
        cs.append(Case(f"k-big-store-{M}x{N}x{K}", "k_gemm16", M, N, K, "k_gemm16_big", 1, _up(K, 64), tile_env="b"))
        cs.append(Case(f"k-big-acc-{M}x{N}x{K}", "k_gemm16", M, N, K, "k_gemm16_big", 1, _up(K, 64), tile_env="b", accumulate=True, pitched=True))
    # ---- the dispatcher: x from 256 x 128 on, k_gemm16 below and whenever there is a bias
    cs.append(Case("d-255x128x64", "gemm16", 255, 128, 64, "k_gemm16_small", 1, 64))
    cs.append(Case("d-256x127x64", "gemm16", 256, 127, 64, "k_gemm16_small", 1, 64))
    cs.append(Case("d-256x128x64", "gemm16", 256, 128, 64, "x", 1, 64))
    cs.append(Case("d-256x128x64-bias", "gemm16", 256, 128, 64, "k_gemm16_small", 1, 64, bias=True))
    cs.append(Case("d-300x200x72-bias", "gemm16", 300, 200, 72, "k_gemm16_small", 1, 128, bias=True, pitched=True))
    # ---- real class: per kernel the case with the most chunks per range
    cs.append(Case("real-x-300x384x12328", "x", 300, 384, 12328, "x", 39, 320, accumulate=True, split_k=1024, cls="real"))
    cs.append(Case("real-r-257x129x2568", "x", 257, 129, 2568, "r", 7, 384, accumulate=True, split_k=8, opts=(("bf16_gemm_regstage", "1"),), cls="real"))
    cs.append(Case("real-p-300x257x1280", "x", 300, 257, 1280, "p", 8, 160, accumulate=True, split_k=8, opts=(("bf16_gemm_pingpong", "1"),), cls="real"))
    cs.append(Case("real-xt-T3-Np776-Nv771-N200-K200", "xt", 3 * 771, 200, 200, "xt", 1, 256, T=3, Np=776, Nv=771, dx_t_ok=True, cls="real"))
    cs.append(Case("real-k-129x130x200", "k_gemm16", 129, 130, 200, "k_gemm16_small", 1, 256, cls="real"))
    cs.append(Case("real-k-atomic-129x130x200", "k_gemm16", 129, 130, 200, "k_gemm16_small", 4, 64, accumulate=True, split_k=1024, cls="real"))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _cases()


@pytest.fixture(scope="module")
def eng():
    from kprn_amd import _ffi
    e = _ffi.Engine(6, 100, 9, 4, 8, 4, 16)
    yield e
    e.close()


def _run(eng, c, A, B, C, bias):
    g = R.geometry(c)
    return eng.gemm16_run(c.route, A, B, C, (g["Mp"] if c.route == "xt" else c.M), c.N, c.K, g["lda"], g["ldb"], g["ldc"], g["a_off"], g["b_off"], g["c_off"],
                          accumulate=c.accumulate, split_k=c.split_k, n_lo=c.n_lo, k_lo=c.k_lo, sx_min=c.sx_min, Np=c.Np, Nv=c.Nv, bias=bias)


RATIOS = {}   # real class: case -> largest |error| / bound (printed: run with -s)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_one_launch_against_the_exact_product(eng, c, monkeypatch):
    if c.tile_env:
        monkeypatch.setenv("KPRN_BF16_TILE", c.tile_env)
    else:
        monkeypatch.delenv("KPRN_BF16_TILE", raising=False)
    A, B, Cin, bias = R.operands(c)
    ref, mag = R.reference(c, A, B, Cin, bias)
    Af, Bf, C0, inside = R.arrays(c, A, B, Cin)
    for k, v in c.opts:
        eng.set_option(k, v)
    try:
        C1 = C0.copy()
        ran = _run(eng, c, Af, Bf, C1, bias)
        C2 = C0.copy()
        ran2 = _run(eng, c, Af, Bf, C2, bias)
    finally:
        for k, _ in c.opts:
            eng.set_option(k, "0")
    # (3) what ran
    assert (ran["kernel"], ran["nsplit"], ran["kchunk"]) == (c.kernel, c.nsplit, c.kchunk), ran
    assert ran2 == ran
    if c.route == "xt":
        assert ran["dx_t_ok"] == c.dx_t_ok and (ran["kernel"] == "xt") == ran["dx_t_ok"], ran
    # (2) nothing outside the window was written
    outside = ~inside
    assert np.array_equal(C1.view(np.uint32)[outside], C0.view(np.uint32)[outside]), "C was written outside its window"
    if c.kernel == "declined":
        assert np.array_equal(C1.view(np.uint32), C0.view(np.uint32))
        return
    # (1) the window
    got = R.c_window(c, C1)
    if c.cls == "int":
        assert np.all(np.isfinite(got)), "NaN / Inf in the window: something outside an operand window was read"
        bad = np.argwhere(got.astype(np.int64) != ref)
        assert bad.size == 0 and np.array_equal(got, ref.astype(np.float32)), (len(bad), bad[:8].tolist())
    else:
        err = np.abs(got.astype(np.float64) - ref)
        bound = R.real_bound(c, mag)
        ratio = float(np.max(err / bound))
        RATIOS[c.name] = ratio
        print(f"{c.name}: largest |error| / bound = {ratio:.3e}")
        assert np.all(err <= bound), (ratio, np.argwhere(err > bound)[:8].tolist())
    # (4) a second launch gives identical bits (real class with more than one K range: float atomics land in any order, so only the bound holds again)
    if c.cls == "int" or c.nsplit == 1:
        assert np.array_equal(C1.view(np.uint32), C2.view(np.uint32))
    else:
        assert np.all(np.abs(R.c_window(c, C2).astype(np.float64) - ref) <= R.real_bound(c, mag))


def _refusal_calls():
    """(name, keyword overrides) on a valid k_gemm16 / xt call: each violates one clause of the products' contracts"""
    base = dict(route="k_gemm16", M=130, N=132, K=72, lda=72, ldb=72, ldc=132, a_off=0, b_off=0, c_off=0)
    xt = dict(route="xt", M=272, N=128, K=72, lda=272, ldb=72, ldc=128, a_off=0, b_off=0, c_off=0, Np=136, Nv=130)
    return [
        ("K % 8", base, dict(K=68)),
        ("lda % 8", base, dict(lda=76)),
        ("ldb % 8", base, dict(ldb=76)),
        ("k_lo % 8", dict(base, route="x", M=256, N=128), dict(k_lo=12)),
        ("Np % 8", xt, dict(Np=68, Nv=60)),
        ("lda < K", base, dict(lda=64)),
        ("ldb < K", base, dict(ldb=64)),
        ("ldc < N", base, dict(ldc=128)),
        ("A window past its array", base, dict(a_short=8)),
        ("B window past its array", base, dict(b_short=8)),
        ("C window past its array", base, dict(c_short=1)),
        ("AT window past its array", xt, dict(a_short=8)),
        ("xt C window past its array (T Nv rows)", xt, dict(c_short=1)),
        ("Nv > Np", xt, dict(Nv=137)),
        ("Mp % Np", xt, dict(Np=128, Nv=120)),
        ("ldat < Mp", xt, dict(lda=264)),
        ("bias with accumulate", base, dict(accumulate=True, bias=True)),
        ("bias on x", dict(base, route="x", M=256, N=128), dict(bias=True)),
        ("a_off % 8", base, dict(a_off=4)),
        ("b_off % 8", base, dict(b_off=12)),
        ("c_off % 4", base, dict(c_off=2)),
    ]


REFUSALS = _refusal_calls()


@pytest.mark.gpu
@pytest.mark.parametrize("name,base,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_what_the_contracts_exclude_is_refused_before_anything_runs(eng, name, base, over):
    from kprn_amd import _ffi
    kw = dict(base)
    kw.update(over)
    short = {k: kw.pop(k, 0) for k in ("a_short", "b_short", "c_short")}
    with_bias = kw.pop("bias", False)
    xt = kw["route"] == "xt"
    rows_c = (kw["M"] // max(kw.get("Np", 1), 1)) * kw.get("Nv", 0) if xt else kw["M"]
    na = kw["a_off"] + (kw["K"] * kw["lda"] if xt else kw["M"] * kw["lda"]) - short["a_short"]
    nb = kw["b_off"] + kw["N"] * kw["ldb"] - short["b_short"]
    nc = kw["c_off"] + max(rows_c, 1) * kw["ldc"] - short["c_short"]
    if xt:   # (exact fit: the last row ends at M, not at the pitch)
        na -= kw["lda"] - kw["M"]
    A = np.ones(max(na, 1), np.float32)
    B = np.ones(max(nb, 1), np.float32)
    C = np.full(max(nc, 1), R.SENTINEL, np.float32)
    route = kw.pop("route")
    with pytest.raises(_ffi.KprnError) as ei:
        eng.gemm16_run(route, A, B, C, kw.pop("M"), kw.pop("N"), kw.pop("K"), kw.pop("lda"), kw.pop("ldb"), kw.pop("ldc"),
                       bias=(np.ones(base["N"], np.float32) if with_bias else None), **kw)
    assert ei.value.code == _ffi.E_ARG, (name, ei.value)
    assert np.all(C.view(np.uint32) == np.float32(R.SENTINEL).view(np.uint32)), "a refused call wrote to C on the host"


@pytest.mark.gpu
def test_the_valid_twins_of_the_refused_calls_run(eng):
    """the base calls the refusals are derived from are accepted at an exact fit (no slack behind the window) -- so each refusal above is due to its one change"""
    A = np.ones(130 * 72, np.float32)
    B = np.ones(132 * 72, np.float32)
    C = np.full(130 * 132, R.SENTINEL, np.float32)
    ran = eng.gemm16_run("k_gemm16", A, B, C, 130, 132, 72, 72, 72, 132)
    assert ran["kernel"] == "k_gemm16_small" and np.all(C == 72.0)
    AT = np.ones(72 * 272, np.float32)
    B = np.ones(128 * 72, np.float32)
    C = np.full(260 * 128, R.SENTINEL, np.float32)
    ran = eng.gemm16_run("xt", AT, B, C, 272, 128, 72, 272, 72, 128, Np=136, Nv=130)
    assert ran["kernel"] == "xt" and ran["dx_t_ok"] and np.all(C == 72.0)
