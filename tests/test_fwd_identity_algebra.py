"""not gpu: the algebra and the index arithmetic of the forward's identity route (kprn_amd/csrc/lstm_fused_fwd.hip fwd_body IDENT),
restated in numpy fp32 before a GPU sees them.

x = [Wt[ty] | We[en] | Wr[re]] (net/FeatureEmbedding.lua:112-121) and z = W_i2g x (nn.FastLSTM i2g), so
    z = W_i2g[:, e cols] We[en] + Q_t[ty] + Q_r[re],   Q_t = Wt W_i2g[:, t cols]^T,   Q_r = Wr W_i2g[:, r cols]^T,
i.e. z = [S | x_e] [Q ; W_i2g[:, e cols]^T] with S the one-hot columns (relation v at column v, type v at Vr + v) and Q the stacked tables' products.
  * the two forms agree to 1e-6 of max |z| in fp32 (sequential accumulation, as an accumulation chain of MFMAs does), pad rows of the tables zero;
  * the launch prologue's fragment map reproduces Q: v_mfma_f32_16x16x4_f32 with the table rows as A and the weight pieces as B leaves, in lane
    (arow, ag), register r, Q[one-hot column 4 ag + r][gate row 16 j + arow] -- which is the B fragment the one-hot k-group reads (k-slot ag, register jj
    <-> k = 4 ag + jj)."""
import numpy as np

DT, DE, DR, H, VT, VR, NS = 16, 32, 16, 64, 6, 9, 16


def _params(seed=0):
    rng = np.random.default_rng(seed)
    u = lambda *s: (rng.random(s) * 0.2 - 0.1).astype(np.float32)
    Wt, We, Wr, W = u(VT, DT), u(500, DE), u(VR, DR), u(4 * H, DT + DE + DR)
    Wt[0] = 0; We[0] = 0; Wr[0] = 0   # the pad tokens' rows are zero rows (kprn_zero_pad_tokens)
    return Wt, We, Wr, W


def _seq_matmul(A, B):
    """A [n, k] B [k, m] accumulated k after k in fp32"""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    return acc


def _tables_as_a(Wt, Wr):
    """rows of the stacked [relation ; type ; zero] tables, split into the relation and the type operand"""
    tab_r, tab_t = np.zeros((NS, DR), np.float32), np.zeros((NS, DT), np.float32)
    tab_r[:VR] = Wr
    tab_t[VR:VR + VT] = Wt
    return tab_r, tab_t


def test_identity_form_equals_the_full_row_form():
    Wt, We, Wr, W = _params()
    rng = np.random.default_rng(1)
    n = 20000
    ty, en, re_ = rng.integers(0, VT, n), rng.integers(0, 500, n), rng.integers(0, VR, n)
    x = np.concatenate([Wt[ty], We[en], Wr[re_]], axis=1)
    z64 = x.astype(np.float64) @ W.astype(np.float64).T
    z_direct = _seq_matmul(x, np.ascontiguousarray(W.T))
    tab_r, tab_t = _tables_as_a(Wt, Wr)
    Q = _seq_matmul(np.concatenate([tab_t, tab_r], axis=1), np.concatenate([W[:, :DT].T, W[:, DT + DE:].T], axis=0))   # the prologue's order: type, then relation
    S = np.zeros((n, NS), np.float32)
    S[np.arange(n), re_] = 1
    S[np.arange(n), VR + ty] = 1
    z_ident = _seq_matmul(np.concatenate([S, We[en]], axis=1), np.concatenate([Q, W[:, DT:DT + DE].T], axis=0))
    scale = float(np.max(np.abs(z64)))
    assert float(np.max(np.abs(z_ident - z_direct))) < 1e-6 * scale
    assert float(np.max(np.abs(z_ident - z64))) < 1e-6 * scale
    assert float(np.max(np.abs(z_direct - z64))) < 1e-6 * scale


def _mfma_16x16x4(A_lane, B_lane, D_lane):
    """v_mfma_f32_16x16x4_f32 on per-lane operands: A_lane[lane] = A[i = lane & 15][k = lane >> 4], B_lane[lane] = B[k = lane >> 4][n = lane & 15],
    D_lane[lane][r] = D[i = 4 (lane >> 4) + r][n = lane & 15]"""
    A, B = np.zeros((16, 4), np.float32), np.zeros((4, 16), np.float32)
    for lane in range(64):
        A[lane & 15, lane >> 4] = A_lane[lane]
        B[lane >> 4, lane & 15] = B_lane[lane]
    D = _seq_matmul(A, B)
    for lane in range(64):
        for r in range(4):
            D_lane[lane, r] += D[4 * (lane >> 4) + r, lane & 15]


def test_prologue_fragment_map_reproduces_q():
    Wt, We, Wr, W = _params(3)
    tab_r, tab_t = _tables_as_a(Wt, Wr)
    Q64 = np.concatenate([tab_t, tab_r], axis=1).astype(np.float64) @ np.concatenate([W[:, :DT].T, W[:, DT + DE:].T], axis=0).astype(np.float64)   # [NS][4H]
    rng = np.random.default_rng(4)
    for j in range(4):           # wave: hidden units 16 j ..
        for q in range(4):       # gate
            sc = np.float32(-2.8853900817779268 if q == 1 else -1.4426950408889634)
            frag = np.zeros((64, 4), np.float32)
            for tab, col0 in ((tab_t, 0), (tab_r, DT + DE)):
                for jj in range(4):
                    a_lane = np.array([tab[lane & 15, 4 * (lane >> 4) + jj] for lane in range(64)], np.float32)
                    b_lane = np.array([W[q * H + 16 * j + (lane & 15), col0 + 4 * (lane >> 4) + jj] * sc for lane in range(64)], np.float32)
                    _mfma_16x16x4(a_lane, b_lane, frag)
            # the fragment map
            for lane in range(64):
                arow, ag = lane & 15, lane >> 4
                for r in range(4):
                    want = Q64[4 * ag + r, q * H + 16 * j + arow] * float(sc)
                    assert abs(frag[lane, r] - want) < 1e-6 * max(1.0, float(np.max(np.abs(Q64))) * abs(float(sc))), (j, q, lane, r)
            # ... and its use: the one-hot k-group (4 MFMAs: A[row][k-slot ag] = S[row][4 ag + jj], B = register jj of the fragment) picks Q's rows
            ty, re_ = rng.integers(0, VT, 16), rng.integers(0, VR, 16)
            S = np.zeros((16, NS), np.float32)
            S[np.arange(16), re_] = 1
            S[np.arange(16), VR + ty] = 1
            acc = np.zeros((64, 4), np.float32)
            for jj in range(4):
                a_lane = np.array([S[lane & 15, 4 * (lane >> 4) + jj] for lane in range(64)], np.float32)
                _mfma_16x16x4(a_lane, frag[:, jj].copy(), acc)
            for lane in range(64):
                arow, ag = lane & 15, lane >> 4
                for r in range(4):
                    row = 4 * ag + r
                    want = (Q64[re_[row], q * H + 16 * j + arow] + Q64[VR + ty[row], q * H + 16 * j + arow]) * float(sc)
                    assert abs(acc[lane, r] - want) < 1e-6 * max(1.0, abs(want)), (j, q, lane, r)
