// hipcc-flags: -fno-slp-vectorize     (packed fp32 VALU beside MFMAs is slower than the scalar pair it replaces; kprn_amd/build.py reads this line)
// configs[3] (BASELINE.json: 20 M entities, d = 128 -> D = H = 384, "bf16 MFMA LSTM"): one FastLSTM layer as ONE persistent launch.
//
// Stands for   FeatureEmbedding (3 x nn.LookupTable + JoinTable)        release/songPathRnn/net/FeatureEmbedding.lua:112-121
//           -> nn.Sequencer(nn.FastLSTM(D, H)), all T steps            release/songPathRnn/model/OneModel.lua:236,268-274
// at the bf16 pipeline's precision (lstm_bf16.hip: bf16 operands, fp32 accumulation, fp32 cell state), replacing its gather launch
// and its T step launches.  What the per-step launches paid for (profiles/r02: 0.27 ms for 62 us of MFMA work) was state through
// HBM: x_t and h_{t-1} in, c in / out, h and four gate planes out, every step, every launch at the mercy of its slowest phase.
//
// Shape of the work.  gates[n, 4H] = [x_t | h_{t-1}] [W_i2g | W_o2g]^T is 2.36 MB of bf16 weights against M path rows; the
// weights cannot stay in registers (1.2 MB would be needed per CU), so they are STREAMED from L2 every step and what is chosen
// is how many rows ride on each pass: the operand rows [x_t | h_{t-1}] of a tile must sit in LDS for the whole step
// ((D + H) * 2 bytes a row), which caps a tile at 96 rows (144 KB of the 160 KB).  One workgroup (4 waves, one per SIMD) owns
// a tile for all T steps:
//   * The product is taken TRANSPOSED on v_mfma_f32_32x32x16_bf16: the weight fragment is the A operand, the path rows are the
//     B operand.  The 32 result rows of a wave are [i | g | f | o] of EIGHT hidden units (packed that way by k_pack_w), the 32
//     result columns are 32 paths.  In the C/D layout (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) a lane then
//     holds all four gates of four consecutive hidden units of one path: the cell is lane-local, h leaves as 4 packed bf16.
//   * chunk = 32 hidden units (8 per wave); per chunk a wave runs (D + H) / 16 k-steps of NPT MFMAs (NPT = 3 path tiles of 32)
//     on ONE 1 KiB weight fragment each -- every wave reads different weights, so they go L2 -> registers directly, PF
//     fragments ahead, 1 KiB contiguous per wave instruction (packed in exactly that order), no LDS round trip.
//   * x_t / h_{t-1} live in LDS in FRAGMENT-MAJOR order [path tile][k-step][lane][16 B]: every B fragment is one conflict-free
//     ds_read_b128 of a contiguous 1 KiB, and exactly what one LDS-DMA instruction (global_load_lds_dwordx4) writes.  The
//     embedding gather IS that DMA (per-lane source address = table row + column piece); no [N, T, D] tensor when scoring.
//   * the cell of chunk c - 1 (12 elements per lane: exp2 / rcp gates, c, h) is issued in slices behind the MFMAs of chunk c's
//     input half (bf16 MFMA runs on the matrix cores: VALU beside it is nearly free, scripts/ubench/mfma_bf16_overlap.hip).
//   * h_t cannot overwrite h_{t-1} in LDS before the step's last chunk has read it and there is no room for a second copy,
//     so the cell writes h_t (packed bf16, fragment order) to a private scratch slab that the next step's DMA brings back:
//     a round trip through this XCD's L2, 72 KB a step against 2.36 MB of weights.  c_t (fp32) goes the same way
//     (fragment-order scratch when scoring; the saved [T][N][H] plane when training).
// Training (SAVE) additionally stores h row-major and c and the four gate activations in fragment order (one contiguous KiB per wave store);
// lstm_bf16.hip's k_gates_bwd16_frag re-lays them out through LDS.
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "gate_math.h"
#include "kprn_internal.h"

namespace bf16p {

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace pk {

constexpr int MAXPT = 3;     // path tiles (32 rows each) of a work tile
constexpr int ROWS = 32 * MAXPT;
constexpr int PF_DEFAULT = 8;    // weight fragments in flight per wave (must divide the k-steps of a half)
constexpr int LA_DEFAULT = 1;    // k-steps the LDS operand fragments are read ahead
constexpr int NW_DEFAULT = 8;     // waves per workgroup: 8 = two per SIMD (a wave's VMEM / LDS / VALU issue fills the other's MFMA time)
constexpr int MAXT = 8;      // steps whose ids are staged in LDS
constexpr int MAXSEG = 3;

struct Args {
  const int32_t* idx; int64_t N; int T, F;
  // the step input as column segments: a table (row = id - 1 of column seg_col of the path step) or, seg_col < 0, row t N + n of a
  // [T][N][w] plane (a layer above the first)
  const bf16* seg_base[MAXSEG]; int seg_w[MAXSEG]; int seg_col[MAXSEG]; int seg_off[MAXSEG]; int nseg;
  const bf16* Wp;    // packed weights [H/32][4 waves][(D + H)/16][64 lanes][8]
  const float* Bp;   // packed bias    [H/32][4 waves][2 halves][16]
  bf16* hscr;        // per workgroup: 2 x [MAXPT][H/16][64][8]  h_t in B-fragment order (ping-pong over steps)
  float* cscr;       // per workgroup: [H/32][MAXPT][4][64][4]   c_t in accumulator order (scoring)
  bf16* H16;         // SAVE: h_t row-major [T][N][H] (the backward's dW product reads it)
  bf16* CsF; bf16* ActF0; bf16* ActF1; int64_t NU;   // SAVE: c_t (bf16) and the gate activations in FRAGMENT order (see Cell::store), NU = units of 32 rows
  bf16* HsF;         // SAVE: h_t in the same fragment order (4 hidden units per record); lstm_bf16.hip k_hfrag_T builds the dW product's h^T from it
  float* hT;         // [N][H] fp32 h_T (the head's input)
  int64_t units;     // ceil(N / 32)
};

// compile-time loop: the body sees its index as a constant (register arrays stay registers, stage switches fold)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p; }

// One LDS-DMA piece: 64 lanes x 16 bytes, lane l's bytes land at lds_dst + 16 l (lds_dst wave-uniform).  Inline asm so that hipcc
// does not see an LDS-DMA in flight (it would wait vmcnt(0) at every later use of a register load, i.e. drain the weight
// prefetch ring at every k-step).  Unknown to hipcc's vmcnt bookkeeping, the pieces only make its counted waits stricter.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// workgroup barrier ordering LDS traffic only (no vmcnt drain: the weight ring stays in flight across it)
__device__ __forceinline__ void bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// every wave's global stores and LDS-DMA pieces have landed, then the barrier
__device__ __forceinline__ void bar_vm0() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Global accesses go through buffer instructions: descriptor (SGPRs) + wave-uniform byte offset (SGPR) + 32-bit lane offset (VGPR).
// With ordinary pointers hipcc re-associates (uniform base + constant) + lane offset into per-lane 64-bit pointers, precomputes one VGPR pair
// for every 4 KB of every weight / scratch stream the unrolled bodies touch, and spills ~200 registers that are then reloaded from
// scratch inside the MFMA loops; a buffer access keeps everything uniform in scalar registers and steps it with scalar adds.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ rsrc_t make_rsrc(const void* base) { return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000); }
template <class V> __device__ __forceinline__ V ldb(rsrc_t r, unsigned voff, unsigned soff) {
  static_assert(sizeof(V) == 16, "16-byte pieces");
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
  return __builtin_bit_cast(V, v);
}
// AUX: cache policy bits of the store (0 default; 2 = nt, a streaming store -- the training saves are not read again by this launch)
#ifndef KPRN_SAVE_AUX
#define KPRN_SAVE_AUX 0
#endif
template <class V, int AUX = 0> __device__ __forceinline__ void stb(rsrc_t r, unsigned voff, unsigned soff, V v) {
  if constexpr (sizeof(V) == 16) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)voff, (int)soff, AUX);
  else { static_assert(sizeof(V) == 8, "8- or 16-byte pieces"); __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)voff, (int)soff, AUX); }
}

// ---- the cell of one finished chunk, as a software pipeline that rides behind the next chunk's MFMAs ---------------------------
// A lane owns NPT x 4 elements (path tile, hidden unit) of the chunk.  One element = 25 VALU operations (10 of them exp2 / rcp),
// cut into 8 stages of <= 4 operations in which nothing consumes a transcendental issued in the same stage; the product loop
// calls micro(k) once behind every MFMA (k = 0 .. NSLOT - 1): element e enters the pipeline at slot start(e), two elements are
// in flight at any time.  hipcc's own interleaving left the cell as one VALU-only stretch between bunched MFMAs (measured:
// 1.12 ms against 0.77 ms without the cell), so the order is pinned at the call site with sched_barrier.
template <int NPT, int KH, bool SAVE, int NW, int DBG = 0>
struct Cell {
  static constexpr int H = KH * 16;
  static constexpr int HC = 8 * NW;      // hidden units per chunk (8 per wave)
  static constexpr int NE = NPT * 4;     // elements per lane
  static constexpr int NST = 9;          // stages per element (the last one: the path tile's stores, after its 4th element)
  const Args& a;
  int wave, lane, ln, half;
  int64_t row0; int nvalid;
  rsrc_t hs, cs;             // this workgroup's scratch slabs (h_t fragments, ping-pong; c_t, scoring)
  int te, ce;                // the chunk being finished: step, chunk
  f32x4 cp[MAXPT];           // c_{t-1} of its elements
  struct El { float vi, vg, vf, vo, ig, c, t; } el[2];      // the two elements in flight
  float gi[4], gg[4], gf[4], go[4], cc[4], hh[4];   // finished values of a path tile (its stores are issued before the next tile's first element finishes)

  __device__ __forceinline__ Cell(const Args& a_, int wave_, int lane_, int64_t row0_, int nvalid_, rsrc_t hs_, rsrc_t cs_)
      : a(a_), wave(wave_), lane(lane_), ln(lane_ & 31), half(lane_ >> 5), row0(row0_), nvalid(nvalid_), hs(hs_), cs(cs_), te(0), ce(0) {}

  // byte offsets of this lane's piece inside (uniform) row-major planes of pitch H / 4H elements: row ln, hidden units 4 half ..
  __device__ __forceinline__ unsigned lo_row(int pitch_elems, int elt) const { return (unsigned)((ln * pitch_elems + 4 * half) * elt); }

  // c_{t-1} of chunk (t, c)'s elements: requested one chunk ahead of the cell that needs it (a dependent load at the head of a
  // chunk would stall its first stages for an L2 round trip)
  __device__ __forceinline__ void request(int t, int c, f32x4 (&cpn)[MAXPT]) const {
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      cpn[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t > 0 && !(DBG & 16)) {
        // (scoring and training alike: the recurrence runs on the fp32 c of this workgroup's L2-resident slab, so the two launches compute the same
        //  forward; the training launch's saved plane is a bf16 copy for the backward)
        cpn[pt] = ldb<f32x4>(cs, (unsigned)lane * 16u, (unsigned)((c * MAXPT + pt) * NW + wave) * 1024u);
      }
    }
  }
  // take over a finished chunk (its pre-activations stay in the accumulator set they were formed in and are handed to every stage)
  __device__ __forceinline__ void take(int t, int c, const f32x4 (&cpn)[MAXPT]) {
    te = t; ce = c;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) cp[pt] = cpn[pt];
  }

  __device__ __forceinline__ void store(int pt) {
    if (DBG & 16) {   // (measurement: the cell's arithmetic without its memory traffic)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" :: "v"(hh[j]), "v"(cc[j]));
      return;
    }
    const int r = 32 * pt + ln;
    const bool ok = r < nvalid;
    bf16x4 hb;
    f32x4 cv, hv;
#pragma unroll
    for (int j = 0; j < 4; ++j) { hb[j] = (bf16)hh[j]; cv[j] = cc[j]; hv[j] = hh[j]; }
    // h_t for the next step's recurrent half: B-fragment order, k = hidden unit (HC ce + 8 wave + 4 half + j: k-step (HC / 16) ce + (wave >> 1),
    // k-group wave & 1, element 4 half + j)
    stb<bf16x4>(hs, (unsigned)(ln * 16 + half * 8), (unsigned)((te & 1) * (MAXPT * KH * 1024) + (pt * KH + (HC / 16) * ce + (wave >> 1)) * 1024 + (wave & 1) * 512), hb);
    const int64_t cu = HC * ce + 8 * wave;   // first hidden unit of this wave's piece
    if (SAVE && 32 * pt < nvalid) {   // (wave-uniform: a workgroup left with a lone 32-row unit runs the two-unit body, whose second unit's records belong to another workgroup -- or lie past the planes)
      // c_t and the four gate activations in FRAGMENT order -- record ((((t NU + unit) NCH + chunk) NW + wave) 64 + lane): c 4 floats, gates [i4 g4] and
      // [f4 o4] as two bf16x8 planes -- every store one contiguous KiB per wave (row-major planes cost this kernel five scattered 8 / 16-byte
      // stores per lane and chunk: 1.27 ms against 0.76 ms for the scoring launch); lstm_bf16.hip's k_gates_bwd16_frag reads them back coalesced
      // and does the re-layout to row-major through LDS on its own side.  Rows past N land in the padded tail of their unit.
      const int64_t rec = ((((int64_t)te * a.NU + row0 / 32 + pt) * (H / HC) + ce) * NW + wave) * 64;
      bf16x4 cb;
#pragma unroll
      for (int j = 0; j < 4; ++j) cb[j] = (bf16)cc[j];
      stb<bf16x4, KPRN_SAVE_AUX>(make_rsrc(a.CsF + rec * 4), (unsigned)lane * 8u, 0, cb);   // (bf16: 0.3 GB less to HBM per launch; the backward's tanh(c), c_{t-1} f (1 - f) take it)
      bf16x8 v0, v1;
#pragma unroll
      for (int j = 0; j < 4; ++j) { v0[j] = (bf16)gi[j]; v0[4 + j] = (bf16)gg[j]; v1[j] = (bf16)gf[j]; v1[4 + j] = (bf16)go[j]; }
      stb<bf16x8, KPRN_SAVE_AUX>(make_rsrc(a.ActF0 + rec * 8), (unsigned)lane * 16u, 0, v0);
      stb<bf16x8, KPRN_SAVE_AUX>(make_rsrc(a.ActF1 + rec * 8), (unsigned)lane * 16u, 0, v1);
      // h_t for the backward's dW product: in fragment order too (one contiguous 512 bytes per wave store).  Row-major, the same 8 bytes per lane land in 32
      // different rows per wave instruction: measured 0.12 ms of the training launch's 1.09 (profiles/r04: KPRN_DBG_NO_H16 build) for 0.3 GB.
      stb<bf16x4, KPRN_SAVE_AUX>(make_rsrc(a.HsF + rec * 4), (unsigned)lane * 8u, 0, hb);
      if (a.H16 && ok) stb<bf16x4, KPRN_SAVE_AUX>(make_rsrc(a.H16 + ((int64_t)te * a.N + row0 + 32 * pt) * H + cu), lo_row(H, 2), 0, hb);   // (the per-step backward's row-major plane: KPRN_BF16_BWD_PERSIST=0)
    }
    stb<f32x4>(cs, (unsigned)lane * 16u, (unsigned)((ce * MAXPT + pt) * NW + wave) * 1024u, cv);
    if (te == a.T - 1 && ok) stb<f32x4>(make_rsrc(a.hT + (row0 + 32 * pt) * H + cu), lo_row(H, 4), 0, hv);
  }

  // stage ST of element E = (path tile pt, hidden unit j)
  template <int E, int ST>
  __device__ __forceinline__ void stage(const f32x16 (&pre)[MAXPT]) {
    constexpr float K1 = -1.4426950408889634f, K2 = -2.8853900817779268f;   // sigmoid(x) = rcp(1 + exp2(K1 x)), tanh(x) = 2 rcp(1 + exp2(K2 x)) - 1
    constexpr int pt = E >> 2, j = E & 3;
    El& x = el[E & 1];
    if constexpr (ST == 0) { x.vi = __builtin_amdgcn_exp2f(pre[pt][j] * K1); x.vg = pre[pt][4 + j] * K2; }
    else if constexpr (ST == 1) { x.vg = __builtin_amdgcn_exp2f(x.vg); x.vf = pre[pt][8 + j] * K1; x.vo = pre[pt][12 + j] * K1; }
    else if constexpr (ST == 2) { x.vf = __builtin_amdgcn_exp2f(x.vf); x.vo = __builtin_amdgcn_exp2f(x.vo); x.vi += 1.0f; x.vg += 1.0f; }
    else if constexpr (ST == 3) { x.vi = __builtin_amdgcn_rcpf(x.vi); x.vg = __builtin_amdgcn_rcpf(x.vg); x.vf += 1.0f; x.vo += 1.0f; }
    else if constexpr (ST == 4) { x.vf = __builtin_amdgcn_rcpf(x.vf); x.vo = __builtin_amdgcn_rcpf(x.vo); x.vg = 2.0f * x.vg - 1.0f; x.ig = x.vi * x.vg; }
    else if constexpr (ST == 5) { x.c = x.vf * cp[pt][j] + x.ig; x.t = __builtin_amdgcn_exp2f(x.c * K2); }
    else if constexpr (ST == 6) { x.t = __builtin_amdgcn_rcpf(x.t + 1.0f); }
    else if constexpr (ST == 7) {
      x.t = 2.0f * x.t - 1.0f;
      cc[j] = x.c; hh[j] = x.vo * x.t;
      if (SAVE) { gi[j] = x.vi; gg[j] = x.vg; gf[j] = x.vf; go[j] = x.vo; }
    } else if constexpr (j == 3) {
      store(pt);
    }
  }
  // slot K of NSLOT behind the MFMAs that carry this cell (one or two product halves): every element whose pipeline covers the slot
  // advances one stage
  template <int NSLOT, int K>
  __device__ __forceinline__ void micro(const f32x16 (&pre)[MAXPT]) {
    static_assert(NSLOT >= NE + NST, "too few MFMAs to carry the cell");
    static_for<0, NE>([&](auto ec) __attribute__((always_inline)) {
      constexpr int e = decltype(ec)::value;
      constexpr int st = K - (e * (NSLOT - NST)) / (NE - 1);
      if constexpr (st >= 0 && st < NST) stage<e, st>(pre);
    });
  }
  __device__ __forceinline__ void all(const f32x16 (&pre)[MAXPT]) {
    static_for<0, NE * NST>([&](auto ic) __attribute__((always_inline)) {
      constexpr int n = decltype(ic)::value;
      stage<n / NST, n % NST>(pre);
    });
  }
};

// ---- one half of a chunk's product: NK k-steps over one LDS operand tile -----------------------------------------------------
// ring[s % PF] holds the weight fragment of k-step s; the fragment of step s + PF is requested as soon as step s has been issued
// (from this half's stream, or from the head of the next half's); the LDS operand fragments are read LA k-steps ahead.
// Issue order, pinned (one wave per SIMD: nothing else fills an MFMA's shadow): behind every MFMA one operand read and one slot
// of the finished chunk's cell (CELL), the weight request behind the k-step's last.
// DBG (measurement builds only, KPRN_PERSIST_DBG): 1 no cell, 2 no weight stream, 4 no LDS operand reads, 8 no MFMAs.
// CSLOTS / COFF: the finished chunk's cell is carried by CSLOTS MFMAs of which this half supplies [COFF, COFF + NK NPT) (CSLOTS = 0: none).
// INIT: the chunk starts here, its accumulators are formed from the bias image (srcC of the first MFMAs: no copies), which is then
// reloaded for the next chunk to start (bias_next).
template <int NPT, int NK, int PF, int LA, bool INIT, int CSLOTS, int COFF, int DBG, class CellT>
__device__ __forceinline__ void half_product(f32x16 (&acc)[MAXPT], f32x16& bias, rsrc_t rB, unsigned bias_next /* byte offset of the next chunk's image */,
                                             const f32x16 (&prev)[MAXPT], bf16x8 (&ring)[PF], rsrc_t rW, unsigned cur /* byte offset of this half's weight stream of this wave */,
                                             unsigned nxt /* ... of the next half's */, const char* tile /* LDS operand tile + 16 lane */, CellT& cell) {
  const unsigned l16 = (unsigned)cell.lane * 16u;
  static_assert(NK % PF == 0, "the weight ring must keep its phase across halves");
  static_assert(LA >= 1 && LA < NK, "operand fragments are read LA k-steps ahead of their MFMAs");
  bf16x8 xf[LA + 1][MAXPT];
#pragma unroll
  for (int q = 0; q < LA; ++q)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) xf[q][pt] = *(const bf16x8*)(tile + (pt * NK + q) * 1024);
  static_for<0, NK * NPT>([&](auto ic) __attribute__((always_inline)) {
    constexpr int k = decltype(ic)::value, s = k / NPT, pt = k % NPT;
    const bf16x8 xv = xf[(DBG & 4) ? 0 : (s % (LA + 1))][pt];
    if constexpr ((DBG & 8) != 0) { asm volatile("" :: "v"(ring[s % PF]), "v"(xv)); if (INIT && s == 0) acc[pt] = bias; }
    else if constexpr (INIT && s == 0) acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[s % PF], xv, bias, 0, 0, 0);
    else acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[s % PF], xv, acc[pt], 0, 0, 0);
    // the k-step's operand reads go out together behind its first MFMA: one lgkmcnt wait per k-step instead of one per MFMA
    if constexpr (pt == 0 && s + LA < NK && !(DBG & 4)) {
#pragma unroll
      for (int q = 0; q < NPT; ++q) xf[(s + LA) % (LA + 1)][q] = *(const bf16x8*)(tile + (q * NK + s + LA) * 1024);
    }
    if constexpr (pt == NPT - 1 && !(DBG & 2)) {   // (1 KiB pieces: three of four requests differ from the one before in the immediate offset only)
      constexpr int sn = (s + PF < NK) ? s + PF : s + PF - NK;
      ring[s % PF] = ldb<bf16x8>(rW, l16 + (unsigned)(sn & 3) * 1024u, ((s + PF < NK) ? cur : nxt) + (unsigned)(sn & ~3) * 1024u);
    }
    if constexpr (INIT && k == NPT - 1) {   // the bias image has been consumed: request the next chunk's
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = ldb<f32x4>(rB, (unsigned)cell.half * 64u + 16u * q, bias_next);
        bias[4 * q] = v[0]; bias[4 * q + 1] = v[1]; bias[4 * q + 2] = v[2]; bias[4 * q + 3] = v[3];
      }
    }
    if constexpr (CSLOTS > 0 && !(DBG & 1)) cell.template micro<CSLOTS, COFF + k>(prev);
    __builtin_amdgcn_sched_barrier(0);
  });
}

// ---- a work tile: NPT path tiles, all T steps ---------------------------------------------------------------------------------
template <int NPT, int KX, int KH, bool SAVE, int NW, int PF, int LA, int DBG>
__device__ __forceinline__ void run_tile(const Args& a, char* XB, char* HB, int32_t* IDS, bf16x8 (&ring)[PF], rsrc_t rW, rsrc_t rB, const bf16* hs_ptr, rsrc_t hs, rsrc_t cs,
                                         int64_t row0, int nvalid, int wave, int lane) {
  constexpr int H = KH * 16, HC = 8 * NW, NCH = H / HC, KS = KX + KH, NTHR = 64 * NW;
  static_assert(H % HC == 0, "whole chunks");
  constexpr unsigned WCH = (unsigned)NW * KS * 1024u;   // bytes between a wave's fragments of consecutive chunks
  const unsigned wbase = (unsigned)wave * KS * 1024u;   // this wave's fragments of chunk 0
  const int ln = lane & 31, half = lane >> 5;
  const int T = a.T;
  // ids of the tile: IDS[(t * MAXSEG + seg) * ROWS + r] = table row (0-based) / path (plane segments); rows past the tile repeat its last
  for (int i = threadIdx.x; i < T * a.nseg * ROWS; i += NTHR) {
    const int r = i % ROWS, sg = (i / ROWS) % a.nseg, t = i / (ROWS * a.nseg);
    const int64_t n = row0 + (r < nvalid ? r : nvalid - 1);
    IDS[(t * MAXSEG + sg) * ROWS + r] = (a.seg_col[sg] >= 0) ? a.idx[(n * T + t) * a.F + a.seg_col[sg]] - 1 : (int32_t)n;
  }
  bar();
  // FeatureEmbedding of step t as LDS-DMA: piece f = (path tile, k-step) is one instruction
  const unsigned xb_lds = lds_off(XB), hb_lds = lds_off(HB);
  auto gather_x = [&](int t) {
    const int k0l = 8 * half;
    for (int f = wave; f < NPT * KX; f += NW) {
      const int pt = f / KX, s = f - pt * KX;
      const int k0 = 16 * s + k0l;
      int sg = 0;
      if (a.nseg > 1 && k0 >= a.seg_off[1]) sg = 1;
      if (a.nseg > 2 && k0 >= a.seg_off[2]) sg = 2;
      int64_t row = IDS[(t * MAXSEG + sg) * ROWS + 32 * pt + ln];
      if (a.seg_col[sg] < 0) row += (int64_t)t * a.N;
      const bf16* src = a.seg_base[sg] + row * a.seg_w[sg] + (k0 - a.seg_off[sg]);
      dma16(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(xb_lds + (unsigned)f * 1024u)));
    }
  };
  auto fetch_h = [&](int t_src) {   // h_{t_src} from the scratch slab into the LDS operand tile
    const char* slab = (const char*)(hs_ptr + (int64_t)(t_src & 1) * (MAXPT * KH * 512));
    for (int f = wave; f < NPT * KH; f += NW)
      dma16(slab + (int64_t)f * 1024 + lane * 16, (unsigned)__builtin_amdgcn_readfirstlane((int)(hb_lds + (unsigned)f * 1024u)));
  };
  auto BP = [&](int c) -> unsigned { return (unsigned)((c < NCH ? c : c - NCH) * NW + wave) * 128u; };   // byte offset of chunk c's (mod NCH) bias image: [2 halves][16]
  auto load_bias = [&](int c) -> f32x16 {   // accumulator image of chunk c's bias (the same for every path column)
    f32x16 b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = ldb<f32x4>(rB, (unsigned)half * 64u, BP(c) + 16 * q);
      b[4 * q] = v[0]; b[4 * q + 1] = v[1]; b[4 * q + 2] = v[2]; b[4 * q + 3] = v[3];
    }
    return b;
  };
  gather_x(0);
  bar_vm0();

  // Two accumulator sets: even chunks form in A, odd chunks in B (NCH is even); while a chunk forms in one set, the cell of the chunk
  // before it reads the other.  Per set: the c_{t-1} requested for the chunk forming in it, and the bias image it starts from.
  static_assert(NCH % 2 == 0 && NCH >= 4, "the chunk schedule below alternates two accumulator sets and reorders the first two chunks of a step");
  constexpr int XS = KX * NPT, HS = KH * NPT;   // MFMAs of an input half / a recurrent half
  Cell<NPT, KH, SAVE, NW, DBG> cell(a, wave, lane, row0, nvalid, hs, cs);
  const char* xt = XB + lane * 16;
  const char* ht = HB + lane * 16;
  f32x16 accA[MAXPT], accB[MAXPT], bn;
  f32x4 cpn[MAXPT];
  auto X = [&](int c) -> unsigned { return wbase + (unsigned)c * WCH; };               // weight stream of chunk c's input half (byte offset)
  auto Hh = [&](int c) -> unsigned { return wbase + (unsigned)c * WCH + KX * 1024u; };   // ... of its recurrent half
  auto keep = [&](f32x16 (&acc)[MAXPT]) {   // (measurement builds without the cell: the products stay alive)
    if (DBG & 1) {
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) asm volatile("" :: "v"(acc[pt]));
    }
  };
  const int T1 = T - 1;
  // ---- t = 0: input halves only; the cell of chunk c - 1 rides behind chunk c's
  bn = load_bias(0);
  cell.request(0, 0, cpn);
  half_product<NPT, KX, PF, LA, true, 0, 0, DBG>(accA, bn, rB, BP(1), accB, ring, rW, X(0), X(1), xt, cell);
  for (int c0 = 0; c0 < NCH; c0 += 2) {
    if (c0 > 0) {
      cell.take(0, c0 - 1, cpn); keep(accB);
      cell.request(0, c0, cpn);
      half_product<NPT, KX, PF, LA, true, XS, 0, DBG>(accA, bn, rB, BP(c0 + 1), accB, ring, rW, X(c0), X(c0 + 1), xt, cell);
    }
    cell.take(0, c0, cpn); keep(accA);
    cell.request(0, c0 + 1, cpn);
    half_product<NPT, KX, PF, LA, true, XS, 0, DBG>(accB, bn, rB, BP(c0 + 2), accA, ring, rW, X(c0 + 1), X(c0 + 2 < NCH ? c0 + 2 : 0), xt, cell);
  }
  if (T > 1) { bar(); gather_x(1); bar_vm0(); }   // (t = 0 has no recurrent half to hide this gather behind)
  // ---- t >= 1.  Order of the product halves: X0 X1 H0 H1, then X_c H_c for c >= 2 -- the fetch of h_{t-1} (which has to wait for the last
  // cell of step t - 1, riding behind X0) lands while X1 runs.
  for (int t = 1; t < T; ++t) {
    cell.take(t - 1, NCH - 1, cpn); keep(accB);
    cell.request(t, 0, cpn);
    half_product<NPT, KX, PF, LA, true, XS, 0, DBG>(accA, bn, rB, BP(1), accB, ring, rW, X(0), X(1), xt, cell);
    bar_vm0();        // every wave's cell stores of step t - 1 have landed, and every wave is done with h_{t-2}
    fetch_h(t - 1);
    half_product<NPT, KX, PF, LA, true, 0, 0, DBG>(accB, bn, rB, BP(2), accA, ring, rW, X(1), Hh(0), xt, cell);
    bar_vm0();        // h_{t-1} is in place
    half_product<NPT, KH, PF, LA, false, 0, 0, DBG>(accA, bn, rB, 0u, accB, ring, rW, Hh(0), Hh(1), ht, cell);
    cell.take(t, 0, cpn); keep(accA);
    cell.request(t, 1, cpn);
    half_product<NPT, KH, PF, LA, false, HS, 0, DBG>(accB, bn, rB, 0u, accA, ring, rW, Hh(1), X(2), ht, cell);
    for (int c0 = 2; c0 < NCH; c0 += 2) {
      const bool last = (c0 + 2 == NCH);
      cell.take(t, c0 - 1, cpn); keep(accB);
      cell.request(t, c0, cpn);
      half_product<NPT, KX, PF, LA, true, XS + HS, 0, DBG>(accA, bn, rB, BP(c0 + 1), accB, ring, rW, X(c0), Hh(c0), xt, cell);
      half_product<NPT, KH, PF, LA, false, XS + HS, XS, DBG>(accA, bn, rB, 0u, accB, ring, rW, Hh(c0), X(c0 + 1), ht, cell);
      cell.take(t, c0, cpn); keep(accA);
      cell.request(t, c0 + 1, cpn);
      half_product<NPT, KX, PF, LA, true, XS + HS, 0, DBG>(accB, bn, rB, BP(c0 + 2), accA, ring, rW, X(c0 + 1), Hh(c0 + 1), xt, cell);
      if (last && t < T1) { bar(); gather_x(t + 1); }   // every wave has read x_t for the last time
      half_product<NPT, KH, PF, LA, false, XS + HS, XS, DBG>(accB, bn, rB, 0u, accA, ring, rW, Hh(c0 + 1), X(last ? 0 : c0 + 2), ht, cell);
      if (last && t < T1) bar_vm0();                    // x_{t+1} is in place
    }
  }
  cell.take(T1, NCH - 1, cpn); keep(accB);
  if (!(DBG & 1)) cell.all(accB);
  bar();   // the operand tiles and the id tile are free for the next work tile
}

template <int KX, int KH, bool SAVE, int NW, int PF, int LA, int DBG>
__global__ __launch_bounds__(64 * NW, NW / 4) void k_lstm16_persist(Args a) {
  constexpr int KS = KX + KH;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* XB = smem;
  char* HB = smem + MAXPT * KX * 1024;
  int32_t* IDS = (int32_t*)(HB + MAXPT * KH * 1024);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t G = gridDim.x, b = blockIdx.x;
  const int64_t u_beg = a.units * b / G, u_end = a.units * (b + 1) / G;
  if (u_beg >= u_end) return;
  const bf16* hs_ptr = a.hscr + b * (int64_t)(2 * MAXPT * KH * 512);
  const rsrc_t hs = make_rsrc(hs_ptr), cs = make_rsrc(a.cscr + b * (int64_t)(KH * 16 * ROWS));   // c_t: [H][96 rows] floats per workgroup
  const rsrc_t rW = make_rsrc(a.Wp), rB = make_rsrc(a.Bp);
  bf16x8 ring[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) ring[s] = ldb<bf16x8>(rW, (unsigned)lane * 16u, (unsigned)(wave * KS + s) * 1024u);
  for (int64_t u = u_beg; u < u_end;) {
    const int64_t rem = u_end - u;
    const int take = rem >= 5 ? 3 : (rem == 4 ? 2 : (int)rem);   // 4 left: 2 + 2 rather than 3 + 1
    const int64_t row0 = u * 32;
    const int nvalid = (int)std::min<int64_t>((int64_t)take * 32, a.N - row0);
    if (take == 3) run_tile<3, KX, KH, SAVE, NW, PF, LA, DBG>(a, XB, HB, IDS, ring, rW, rB, hs_ptr, hs, cs, row0, nvalid, wave, lane);
    else run_tile<2, KX, KH, SAVE, NW, PF, LA, DBG>(a, XB, HB, IDS, ring, rW, rB, hs_ptr, hs, cs, row0, nvalid, wave, lane);
    u += take;
  }
}

// ---- weight / bias packing (whenever the dense parameters change) ----------------------------------------------------------
// Wp[((c * NW + w) * KS + s) * 64 + lane][j]: A fragment of k-step s for wave w of chunk c (HC = 8 NW hidden units); lane = (m, kg), row m =
// gate (m >> 3) of hidden unit HC c + 8 w + (m & 7), k = 16 s + 8 kg + j over [x | h].  From the fp32 masters (rounded once, as the shadow is).
__global__ void k_pack_w(const float* __restrict__ Wi, const float* __restrict__ Wo, const float* __restrict__ bi, int D, int H, int NW, bf16* __restrict__ Wp,
                         float* __restrict__ Bp) {
  const int KS = (D + H) / 16, HC = 8 * NW;
  const int64_t total = (int64_t)(H / HC) * NW * KS * 64;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) {
    const int lane = (int)(i & 63);
    const int64_t f = i >> 6;
    const int s = (int)(f % KS);
    const int w = (int)((f / KS) % NW);
    const int c = (int)(f / ((int64_t)KS * NW));
    const int m = lane & 31, kg = lane >> 5;
    const int row = (m >> 3) * H + HC * c + 8 * w + (m & 7);
    const int k0 = 16 * s + 8 * kg;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      o[j] = (bf16)(k < D ? Wi[(int64_t)row * D + k] : Wo[(int64_t)row * H + (k - D)]);
    }
    *(bf16x8*)(Wp + i * 8) = o;
  }
  if (i < (int64_t)(H / HC) * NW * 2 * 16) {   // Bp[((c * NW + w) * 2 + half) * 16 + r]: accumulator register r of a lane in that half
    const int r = (int)(i & 15), half = (int)((i >> 4) & 1), w = (int)((i >> 5) % NW), c = (int)((i >> 5) / NW);
    Bp[i] = bi[(r >> 2) * H + HC * c + 8 * w + 4 * half + (r & 3)];
  }
}

}  // namespace pk

// ---- host side --------------------------------------------------------------------------------------------------------------
struct PersistSaves { const bf16* CsF; const bf16* ActF0; const bf16* ActF1; const bf16* HsF; int64_t NU, step_recs; int NW; };   // (also declared in lstm_bf16.hip, lstm_bf16_bwd_persist.hip)
struct PersistState {
  bf16* Wp = nullptr; float* Bp = nullptr; bf16* hscr = nullptr; float* cscr = nullptr;
  int grid = 0;
  int packed_nw = 0;   // waves per workgroup the packed weights are laid out for
  bf16* CsF = nullptr; bf16* ActF0 = nullptr; bf16* ActF1 = nullptr; bf16* HsF = nullptr; int64_t save_recs = 0;   // training saves, fragment order
};

bool persist_shape_ok(const kprn_handle* h, const kprn_batch* b) {
  const kprn_config& c = h->cfg;
  static const bool off = [] { const char* e = getenv("KPRN_BF16_PERSIST"); return e && e[0] == '0'; }();
  if (off) return false;
  // instantiated shape: D = H = 384 (three 128-wide tables), one layer, one type slot
  return c.L == 1 && c.H == 384 && h->D == 384 && c.num_types == 1 && (c.dt % 8) == 0 && (c.de % 8) == 0 && (c.dr % 8) == 0 && b->T >= 1 && b->T <= pk::MAXT;
}

void persist_release(void*& st) {
  PersistState* p = (PersistState*)st;
  if (!p) return;
  for (void* q : {(void*)p->Wp, (void*)p->Bp, (void*)p->hscr, (void*)p->cscr, (void*)p->CsF, (void*)p->ActF0, (void*)p->ActF1, (void*)p->HsF}) if (q) hipFree(q);
  delete p;
  st = nullptr;
}

template <typename Tp> static Tp* pal(int64_t n) {
  void* p = nullptr;
  hipError_t e = kprn_dev_malloc(&p, (size_t)std::max<int64_t>(n, 1) * sizeof(Tp));
  if (e != hipSuccess) throw KprnError{KPRN_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e)};
  return (Tp*)p;
}

// repack: true when the dense parameters changed since the last call
void persist_forward(kprn_handle* h, const kprn_batch* b, bool save, void*& st, bool repack, const bf16* Wt16, const bf16* We16, const bf16* Wr16, bf16* H16,
                     PersistSaves* sv) {
  constexpr int KX = 24, KH = 24;
  const kprn_config& c = h->cfg;
  const int H = c.H, D = h->D, T = b->T;
  const int64_t N = b->N;
  hipStream_t strm = h->stream;
  PersistState* p = (PersistState*)st;
  if (!p) {
    p = new PersistState();
    st = p;
    int dev = 0, ncu = 256;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    p->grid = ncu;
    p->Wp = pal<bf16>((int64_t)4 * H * (D + H) + 64);
    p->Bp = pal<float>((int64_t)4 * H);
    p->hscr = pal<bf16>((int64_t)ncu * 2 * pk::MAXPT * KH * 512);
    p->cscr = pal<float>((int64_t)ncu * H * pk::ROWS);
    repack = true;
  }
  int nw = pk::NW_DEFAULT;
#ifdef KPRN_PERSIST_VARIANTS
  int dbg = 0, pf = pk::PF_DEFAULT, la = pk::LA_DEFAULT;
  // measurement builds (scripts/gpu_persist_knockouts.py): KPRN_PERSIST_NW = waves per workgroup, _DBG = knock-out mask, _PF = ring depth, _LA
  if (!save) {
    if (const char* e = KPRN_DEV_ENV("KPRN_PERSIST_NW")) nw = atoi(e);
    if (const char* e = KPRN_DEV_ENV("KPRN_PERSIST_DBG")) dbg = atoi(e);
    if (const char* e = KPRN_DEV_ENV("KPRN_PERSIST_PF")) pf = atoi(e);
    if (const char* e = KPRN_DEV_ENV("KPRN_PERSIST_LA")) la = atoi(e);
  }
#endif
  if (repack || p->packed_nw != nw) {
    const int64_t total = (int64_t)4 * H * ((D + H) / 16) * 8;   // 16-byte pieces of the packed weights
    hipLaunchKernelGGL(pk::k_pack_w, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, strm, h->dense + h->layer[0].Wi, h->dense + h->layer[0].Wo,
                       h->dense + h->layer[0].bi, D, H, nw, p->Wp, p->Bp);
    HIP_TRY(hipGetLastError());
    p->packed_nw = nw;
  }
  pk::Args a;
  memset(&a, 0, sizeof(a));
  a.idx = b->idx; a.N = N; a.T = T; a.F = b->F;
  a.nseg = 3;
  a.seg_base[0] = Wt16; a.seg_w[0] = c.dt; a.seg_col[0] = b->F - c.num_types - 2; a.seg_off[0] = 0;
  a.seg_base[1] = We16; a.seg_w[1] = c.de; a.seg_col[1] = b->F - 2; a.seg_off[1] = c.dt;
  a.seg_base[2] = Wr16; a.seg_w[2] = c.dr; a.seg_col[2] = b->F - 1; a.seg_off[2] = c.dt + c.de;
  a.Wp = p->Wp; a.Bp = p->Bp; a.hscr = p->hscr; a.cscr = p->cscr;
  a.H16 = H16; a.NU = (N + 31) / 32;
  if (save) {
    PersistState* q = p;
    const int64_t recs = (int64_t)T * a.NU * 32 * H / 4;   // 4-element records of one plane
    if (recs > q->save_recs) {
      HIP_TRY(hipStreamSynchronize(strm));
      for (void* x : {(void*)q->CsF, (void*)q->ActF0, (void*)q->ActF1, (void*)q->HsF}) if (x) hipFree(x);
      q->CsF = pal<bf16>(recs * 4); q->ActF0 = pal<bf16>(recs * 8); q->ActF1 = pal<bf16>(recs * 8); q->HsF = pal<bf16>(recs * 4);
      q->save_recs = recs;
    }
    a.CsF = q->CsF; a.ActF0 = q->ActF0; a.ActF1 = q->ActF1; a.HsF = q->HsF;
    sv->CsF = q->CsF; sv->ActF0 = q->ActF0; sv->ActF1 = q->ActF1; sv->HsF = q->HsF; sv->NU = a.NU; sv->NW = nw; sv->step_recs = a.NU * 32 * H / 4;
  }
  a.hT = h->ws.Hs + (int64_t)(T - 1) * N * H;   // (L = 1: layer 0's last step)
  a.units = (N + 31) / 32;
  int grid = p->grid;
  if (h->reserve_cus > 0 && !save) grid = std::max(1, grid - h->reserve_cus);
  grid = (int)std::min<int64_t>(grid, std::max<int64_t>(1, a.units / 2));
  if (const char* e = getenv("KPRN_PERSIST_GRID"))   // (tests: few workgroups -> 96-row tiles at small N; many -> lone 32-row units)
    grid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p->grid, a.units), atoi(e)));
  const size_t lds_bytes = (size_t)pk::MAXPT * (KX + KH) * 1024 + (size_t)pk::MAXT * pk::MAXSEG * pk::ROWS * sizeof(int32_t);
  typedef void (*Kern)(pk::Args);
  Kern k = save ? (Kern)pk::k_lstm16_persist<KX, KH, true, pk::NW_DEFAULT, pk::PF_DEFAULT, pk::LA_DEFAULT, 0>
                : (Kern)pk::k_lstm16_persist<KX, KH, false, pk::NW_DEFAULT, pk::PF_DEFAULT, pk::LA_DEFAULT, 0>;
#ifdef KPRN_PERSIST_VARIANTS
  if (!save) {
    bool found = false;
#define KV(W, P, A, Dg) if (nw == W && pf == P && la == A && dbg == Dg) { k = (Kern)pk::k_lstm16_persist<KX, KH, false, W, P, A, Dg>; found = true; }
    KV(8, 8, 1, 0) KV(8, 12, 1, 0) KV(8, 8, 2, 0) KV(8, 12, 2, 0) KV(4, 12, 2, 0) KV(4, 24, 2, 0)
    KV(8, 8, 1, 1) KV(8, 8, 1, 2) KV(8, 8, 1, 4) KV(8, 8, 1, 6) KV(8, 8, 1, 7) KV(8, 8, 1, 9) KV(8, 8, 1, 13) KV(8, 8, 1, 15) KV(8, 8, 1, 16)
#undef KV
    KPRN_REQUIRE(found, KPRN_E_ARG, "this variant of the persistent kernel is not compiled in");
  }
#endif
  HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  ProfScope ps(h, save ? "lstm_persist_bf16_train" : "lstm_persist_bf16_score");
  hipLaunchKernelGGL(k, dim3(grid), dim3(64 * nw), lds_bytes, strm, a);
  HIP_TRY(hipGetLastError());
}

}  // namespace bf16p
