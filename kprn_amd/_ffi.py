"""ctypes binding of libkprn.so (include/kprn.h).  There is NO CPU path: if the HIP library
is missing or no GPU is visible, everything here fails loudly.

The LuaJIT twin of this file is bindings/kprn.lua.
"""
import ctypes as C
import os
import re
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KPRN_LIB") or os.path.join(_HERE, "libkprn.so")   # (KPRN_LIB: a measurement build, scripts/build_variants.py)
HEADER = os.path.join(_HERE, "..", "include", "kprn.h")


class KprnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"kprn error {code}: {msg}")
        self.code = code
        self.msg = msg


E_ARG, E_INDEX, E_DEVICE, E_UNSUPPORTED, E_IO, E_NOMEM = -1, -2, -3, -4, -5, -6


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("Vt", "Ve", "Vr", "dt", "de", "dr", "F", "num_types", "H", "L", "C",
                                          "rnn_type", "use_relu", "rnn_init", "compute_dtype", "reducer", "K", "device_id", "rank", "world")] + \
               [("param_init", C.c_float), ("seed", C.c_uint64), ("stream", C.c_void_p)]


class Opt(C.Structure):
    _fields_ = [("method", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("lr_decay", C.c_float), ("regularize", C.c_int32), ("use_grad_clip", C.c_int32),
                ("grad_clip_norm", C.c_float), ("l2", C.c_float), ("bce_literal", C.c_int32), ("entity_update", C.c_int32)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("launches", C.c_int64)]


class Gemm16Call(C.Structure):   # kprn_gemm16_call
    _fields_ = [(n, C.c_int32) for n in ("route", "accumulate", "split_k", "n_lo", "sx_min", "N")] + \
               [(n, C.c_int64) for n in ("M", "K", "k_lo", "Np", "Nv", "a_count", "a_off", "lda", "b_count", "b_off", "ldb", "c_count", "c_off", "ldc")]


class Gemm16Ran(C.Structure):    # kprn_gemm16_ran
    _fields_ = [("kernel", C.c_int32), ("nsplit", C.c_int32), ("kchunk", C.c_int64), ("dx_t_ok", C.c_int32), ("reserved", C.c_int32)]


GEMM16_ROUTES = {"gemm16": 0, "x": 1, "xt": 2, "k_gemm16": 3}                          # kprn_gemm16_call.route
GEMM16_KERNELS = ("declined", "k_gemm16_small", "k_gemm16_big", "x", "r", "p", "xt")   # KPRN_GEMM16_*


def declared_symbols():
    """every function include/kprn.h declares (used by the CPU test that the library exports them all)."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(kprn_[a-z_0-9]+)\s*\(", txt)))


def dp_unique_id(rccl_path=None):
    """128 bytes from ncclGetUniqueId (rank 0 draws it; the caller broadcasts it to every rank's Engine.dp_init)"""
    L = lib()
    buf = (C.c_char * 128)()
    rc = L.kprn_dp_unique_id(rccl_path.encode() if rccl_path else None, buf)
    if rc != 0:
        raise KprnError(rc, L.kprn_last_error(None).decode())
    return bytes(buf.raw)


def dp_available(rccl_path=None):
    return lib().kprn_dp_available(rccl_path.encode() if rccl_path else None) == 0


def torch_rccl_path():
    """the librccl.so the running torch build ships (the copy torch.distributed's "nccl" backend has loaded), or None"""
    try:
        import torch
        p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        return p if os.path.exists(p) else None
    except Exception:
        return None


RAGGED_MAX_SEG = 4096   # paths per pair of a ragged batch (kprn_host_ragged_plan refuses more)


def host_ragged_plan(counts, N=None):
    """kprn_host_ragged_plan (no handle, no GPU): -> dict(offsets [B+1], wg_first [n_wg+1], n_wg, max_count, wave, max_seg, thread_max, wg_paths,
    wg_pairs); raises KprnError(E_ARG) for a count outside 1..max_seg or counts that do not add up to N"""
    counts = np.ascontiguousarray(counts, np.int32)
    B = int(counts.shape[0])
    N = int(counts.astype(np.int64).sum()) if N is None else int(N)
    off = np.zeros(B + 1, np.int32)
    wg = np.zeros(B + 1, np.int32)
    sm = np.zeros(8, np.int32)
    rc = lib().kprn_host_ragged_plan(_fp(counts), B, C.c_int64(N), _fp(off), _fp(wg), _fp(sm))
    if rc != 0:
        raise KprnError(rc, "kprn_host_ragged_plan: bad counts")
    return dict(offsets=off, wg_first=wg[:int(sm[0]) + 1].copy(), n_wg=int(sm[0]), max_count=int(sm[1]), wave=int(sm[2]), max_seg=int(sm[3]),
                thread_max=int(sm[4]), wg_paths=int(sm[5]), wg_pairs=int(sm[6]))


RANK_PRINTED, RANK_RAW = 0, 1          # kprn_rank_groups modes: the evaluation chain's printed "%.5f" scores | the raw fp32 values
RANK_ZERO_GROUP, RANK_NO_POSITIVE = -1, -2
RANK_MAX_GROUP, RANK_MAX_K = 4096, 64


def _rank_args(group_offsets, members, pos, K, hist_len):
    """the arrays of kprn_rank_groups / kprn_host_rank_groups; K = 0: no top-K (the C call still wants a K in range)"""
    goff = np.ascontiguousarray(group_offsets, np.int64)
    if goff.ndim != 1 or goff.shape[0] < 2:
        raise KprnError(E_ARG, "group_offsets must be [G+1], G >= 1")
    G = int(goff.shape[0]) - 1
    mem = None if members is None else np.ascontiguousarray(members, np.int64)
    if mem is not None and (mem.ndim != 1 or goff[0] < 0 or goff[-1] > mem.shape[0]):
        raise KprnError(E_ARG, "group_offsets must lie inside members")
    p = None if pos is None else np.ascontiguousarray(pos, np.int32)
    if p is not None and p.shape != (G,):
        raise KprnError(E_ARG, "pos must be [G]")
    if K < 0:
        raise KprnError(E_ARG, "K must be in 0..64")
    out = dict(ranks=np.full(G, -3, np.int32), hist=np.zeros(int(max(hist_len, 0)) + 4, np.int64))
    if K > 0:
        out["topk_idx"] = np.full((G, K), -3, np.int32)
        out["topk_score"] = np.zeros((G, K), np.float32)
    return goff, G, mem, p, out


def host_rank_groups(scores, group_offsets, members=None, pos=None, mode=0, K=0, hist_len=15):
    """kprn_host_rank_groups (no handle, no GPU): the ranking rule of include/kprn.h over a host score array ->
    dict(ranks [G], hist [hist_len + 4], and with K > 0 topk_idx / topk_score [G,K])"""
    sc = np.ascontiguousarray(scores, np.float32)
    goff, G, mem, p, out = _rank_args(group_offsets, members, pos, K, hist_len)
    rc = lib().kprn_host_rank_groups(_fp(sc), C.c_int64(int(sc.shape[0])), _fp(mem), _fp(goff), _fp(p), G, int(mode), int(K) if K > 0 else 1,
                                     _fp(out["ranks"]), _fp(out.get("topk_idx")), _fp(out.get("topk_score")), _fp(out["hist"]), int(hist_len))
    if rc != 0:
        raise KprnError(rc, "kprn_host_rank_groups: bad groups / members / pos / K / hist_len / mode")
    return out


SELECT_MAX_KEEP = 256   # kprn_select_hardest's n_keep limit (KPRN_SELECT_MAX_KEEP)


def _select_args(group_offsets, members, pos, keep):
    """the arrays of kprn_select_hardest / kprn_host_select_hardest; what the C call reads through an array's length is checked here, the rest there.
    keep: a uint8 array of at least group_offsets[G] entries to write into (None: a new one of zeros)"""
    goff = np.ascontiguousarray(group_offsets, np.int64)
    if goff.ndim != 1 or goff.shape[0] < 2:
        raise KprnError(E_ARG, "group_offsets must be [G+1], G >= 1")
    G = int(goff.shape[0]) - 1
    mem = None if members is None else np.ascontiguousarray(members, np.int64)
    if mem is not None and (mem.ndim != 1 or goff[0] < 0 or goff[-1] > mem.shape[0]):
        raise KprnError(E_ARG, "group_offsets must lie inside members")
    p = None if pos is None else np.ascontiguousarray(pos, np.int32)
    if p is not None and p.shape != (G,):
        raise KprnError(E_ARG, "pos must be [G]")
    if keep is None:
        keep = np.zeros(max(int(goff[-1]), 0), np.uint8)
    elif keep.dtype != np.uint8 or keep.ndim != 1 or not keep.flags.c_contiguous or keep.shape[0] < goff[-1]:
        raise KprnError(E_ARG, "keep must be a contiguous uint8 array of at least group_offsets[G] entries")
    return goff, G, mem, p, keep


def host_select_hardest(scores, group_offsets, n_keep, members=None, pos=None, keep=None):
    """kprn_host_select_hardest (no handle, no GPU): the rule of include/kprn.h "hard negatives" over a host score array -> (keep uint8 [group_offsets[G]] in
    member order: the group's positive pos[g] (-1 / None: none) and its n_keep highest-scoring other members, n_invalid)"""
    sc = np.ascontiguousarray(scores, np.float32)
    goff, G, mem, p, keep = _select_args(group_offsets, members, pos, keep)
    ninv = C.c_int64(0)
    rc = lib().kprn_host_select_hardest(_fp(sc), C.c_int64(int(sc.shape[0])), _fp(mem), _fp(goff), _fp(p), G, int(n_keep), _fp(keep), C.byref(ninv))
    if rc != 0:
        raise KprnError(rc, "kprn_host_select_hardest: bad groups / members / pos / n_keep")
    return keep, int(ninv.value)


def _rank_targets_args(group_offsets, target_offsets, targets, members, hist_len):
    """the arrays of kprn_rank_targets / kprn_host_rank_targets; what the C call reads through an array's length is checked here, the rest there"""
    goff = np.ascontiguousarray(group_offsets, np.int64)
    toff = np.ascontiguousarray(target_offsets, np.int64)
    if goff.ndim != 1 or goff.shape[0] < 2 or toff.shape != goff.shape:
        raise KprnError(E_ARG, "group_offsets and target_offsets must be [G+1], G >= 1")
    tg = np.ascontiguousarray(targets, np.int32)
    if tg.ndim != 1 or toff[0] != 0 or np.any(np.diff(toff) < 0) or toff[-1] != tg.shape[0] or tg.shape[0] < 1:
        raise KprnError(E_ARG, "target_offsets must run from 0 to len(targets) >= 1 without decreasing")
    mem = None if members is None else np.ascontiguousarray(members, np.int64)
    if mem is not None and (mem.ndim != 1 or goff[0] < 0 or goff[-1] > mem.shape[0]):
        raise KprnError(E_ARG, "group_offsets must lie inside members")
    out = dict(places=np.full(tg.shape[0], -3, np.int32), hist=np.zeros(int(max(hist_len, 0)) + 4, np.int64))
    return goff, toff, tg, mem, int(goff.shape[0]) - 1, out


def host_rank_targets(scores, group_offsets, target_offsets, targets, members=None, mode=0, hist_len=15, out=None):
    """kprn_host_rank_targets (no handle, no GPU): the rule of include/kprn.h "ranking targets in groups of any size" over a host score array ->
    dict(places [NT], hist [hist_len + 4]); out: a dict with those two arrays to write into"""
    sc = np.ascontiguousarray(scores, np.float32)
    goff, toff, tg, mem, G, res = _rank_targets_args(group_offsets, target_offsets, targets, members, hist_len)
    res = res if out is None else out
    rc = lib().kprn_host_rank_targets(_fp(sc), C.c_int64(int(sc.shape[0])), _fp(mem), _fp(goff), _fp(toff), _fp(tg), G, int(mode), _fp(res["places"]),
                                      _fp(res["hist"]), int(hist_len))
    if rc != 0:
        raise KprnError(rc, "kprn_host_rank_targets: bad groups / members / targets / hist_len / mode")
    return res


EXPLAIN_MAX_M = 32   # strongest paths per explained pair (KPRN_EXPLAIN_MAX_M)


def _explain_out(shape, M, out, scalars=True):
    """the result arrays of the explanation calls: path_idx / path_score / path_weight [*shape, M] (+ pooled / probs [*shape]); `out` supplies any of them"""
    M = max(int(M), 1)   # (the range is the library's to refuse)
    spec = [("path_idx", np.int32, tuple(shape) + (M,)), ("path_score", np.float32, tuple(shape) + (M,)), ("path_weight", np.float32, tuple(shape) + (M,))]
    if scalars:
        spec += [("pooled", np.float32, tuple(shape)), ("probs", np.float32, tuple(shape))]
    res = {}
    for name, dt, shp in spec:
        a = (out or {}).get(name)
        if a is None:
            a = np.full(shp, -3 if dt is np.int32 else 0, dt)
        if a.dtype != dt or a.shape != shp or not a.flags.c_contiguous:
            raise KprnError(E_ARG, "%s must be a C-contiguous %s array of shape %s" % (name, np.dtype(dt).name, shp))
        res[name] = a
    return res


def host_explain(path_scores, offsets, class_id, reducer, K_reducer, M, pairs=None, out=None, gamma=1.0):
    """kprn_host_explain_gamma (no handle, no GPU): the explanation rule of include/kprn.h over a host score matrix path_scores [N,C]; pair b owns the rows
    offsets[b] .. offsets[b+1]-1; pairs None = every pair -> dict(path_idx / path_score / path_weight [n,M], pooled / probs [n]).  gamma: the pooling
    temperature (include/kprn.h "pooling temperature"); 1.0 is kprn_host_explain"""
    sc = np.ascontiguousarray(path_scores, np.float32)
    off = np.ascontiguousarray(offsets, np.int32)
    if sc.ndim != 2 or off.ndim != 1 or off.shape[0] < 2 or int(off[-1]) > sc.shape[0]:
        raise KprnError(E_ARG, "path_scores must be [N,C] and offsets [B+1] inside it")
    B = int(off.shape[0]) - 1
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1)
    n = B if pr is None else int(pr.shape[0])
    res = _explain_out((n,), M, out)
    rc = lib().kprn_host_explain_gamma(_fp(sc), _fp(off), B, int(sc.shape[1]), int(class_id), int(reducer), int(K_reducer), _fp(pr), n, int(M),
                                       _fp(res["path_idx"]), _fp(res["path_score"]), _fp(res["path_weight"]), _fp(res["pooled"]), _fp(res["probs"]),
                                       C.c_float(float(gamma)))
    if rc != 0:
        raise KprnError(rc, "kprn_host_explain_gamma: bad offsets / class_id / reducer / pairs / M / gamma")
    return res


def host_dropout_keep(seed, draw, layer, T, N, Din, p):
    """kprn_host_dropout_keep (no handle, no GPU): the keep flags [T, N, Din] (uint8, 1 = kept) of the engine's dropout generator for one layer of one
    training forward (include/kprn.h: Philox4x32-10 addressed by seed, draw, layer, step, path, element)"""
    keep = np.zeros((max(int(T), 0), max(int(N), 0), max(int(Din), 0)), np.uint8)
    rc = lib().kprn_host_dropout_keep(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(draw) & 0xFFFFFFFF), int(layer), int(T), C.c_int64(int(N)), int(Din),
                                      C.c_float(float(p)), _fp(keep) if keep.size else None)
    if rc != 0:
        raise KprnError(rc, "kprn_host_dropout_keep: bad layer / T / N / Din / p")
    return keep


PAIRWISE_MAX_GROUP = 1024   # pairs per group of the pairwise loss (KPRN_PAIRWISE_MAX_GROUP)


def host_pairwise_loss(pooled, labels, group_offsets, inv_batch=0.0):
    """kprn_host_pairwise_loss (no handle, no GPU): the pairwise loss over the groups of consecutive pairs that group_offsets [G+1] cuts (include/kprn.h
    "pairwise loss") -> (loss, dy [B] = d loss / d pooled, n_terms); inv_batch > 0: the scale, else 1 / n_terms.  Raises KprnError(E_ARG) for a bad table"""
    y = np.ascontiguousarray(pooled, np.float32).reshape(-1)
    t = np.ascontiguousarray(labels, np.float32).reshape(-1)
    go = np.ascontiguousarray(group_offsets, np.int32).reshape(-1)
    if t.shape != y.shape:
        raise KprnError(E_ARG, "pooled and labels must both be [B]")
    dy = np.zeros(y.shape, np.float32)
    loss, n = C.c_float(), C.c_int64()
    rc = lib().kprn_host_pairwise_loss(_fp(y), _fp(t), _fp(go), int(go.shape[0]) - 1, int(y.shape[0]), C.c_float(float(inv_batch)), _fp(dy), C.byref(loss), C.byref(n))
    if rc != 0:
        raise KprnError(rc, "kprn_host_pairwise_loss: bad group_offsets (go[0] = 0, go[G] = B, non-decreasing, groups of at most %d pairs)" % PAIRWISE_MAX_GROUP)
    return float(loss.value), dy, int(n.value)


FIND_MAX_HOPS, FIND_MAX_PATHS = 3, 4096   # kprn_find_paths: hops per path, kept paths per pair
FIND_MAX_HOPS_SAMPLED, FIND_MAX_WALKS = 5, 256   # kprn_find_paths_sampled: hops per path, walks per pair and sampled hop count
CAND_TOP_MAX_BM = 1 << 28   # kprn_find_candidates_top: users * catalogue items of one call must stay below this


def _graph_arrays(src, dst, rel, node_types):
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    nt = np.ascontiguousarray(node_types, np.int32)
    if not (src.shape == dst.shape == rel.shape) or nt.ndim != 2:
        raise KprnError(E_ARG, "a graph is src / dst / rel [E] and node_types [Ve, num_types]")
    return src, dst, rel, nt


def _pairs_array(pairs, labels):
    pr = np.ascontiguousarray(pairs, np.int32)
    if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] < 1:
        raise KprnError(E_ARG, "pairs must be [B, 2] = (user, item)")
    lab = None if labels is None else np.ascontiguousarray(labels, np.float32)
    if lab is not None and lab.shape != (pr.shape[0],):
        raise KprnError(E_ARG, "labels must be [B]")
    return pr, lab


def _seed_draw(seed, draw):
    return C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(draw) & 0xFFFFFFFF)


def _host_find(call_lib, what, src, dst, rel, node_types, pairs, T, F, want_idx):
    """the two calls of a host finder: counts, then rows.  call_lib(arrays .., counts, found, idx) -> status"""
    src, dst, rel, nt = _graph_arrays(src, dst, rel, node_types)
    pr, _ = _pairs_array(pairs, None)
    F = int(nt.shape[1]) + 2 if F is None else int(F)
    B = int(pr.shape[0])
    counts, found = np.zeros(B, np.int32), np.zeros(B, np.int64)

    def call(idx):
        rc = call_lib(src, dst, rel, nt, pr, B, F, counts, found, idx)
        if rc != 0:
            raise KprnError(rc, what + ": bad graph ids / pairs / hops / max_paths / T / F / walks")
    call(None)
    if not want_idx:
        return None, counts, found
    idx = np.zeros((int(counts.astype(np.int64).sum()), int(T), F), np.int32)
    if idx.size:
        call(idx)
    return idx, counts, found


def host_find_paths(src, dst, rel, node_types, Vr, Vt, end_relation, pairs, min_hops, max_hops, max_paths, T, F=None, threads=1, want_idx=True):
    """kprn_host_find_paths (no handle, no GPU): the finder's rule of include/kprn.h over the graph's raw arrays; Ve and num_types are node_types' shape ->
    (idx [N,T,F] of the pairs with counts > 0 in input order, or None with want_idx=False; counts [B]; found [B])"""
    def call(src, dst, rel, nt, pr, B, F, counts, found, idx):
        return lib().kprn_host_find_paths(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), _fp(nt), int(nt.shape[0]), int(Vr), int(Vt), int(nt.shape[1]),
                                          int(end_relation), _fp(pr), B, int(min_hops), int(max_hops), int(max_paths), int(T), F, int(threads), _fp(counts),
                                          _fp(found), _fp(idx))
    return _host_find(call, "kprn_host_find_paths", src, dst, rel, node_types, pairs, T, F, want_idx)


def host_find_paths_sampled(src, dst, rel, node_types, Vr, Vt, end_relation, pairs, min_hops, max_hops, max_paths, T, walks, seed, draw, F=None, threads=1,
                            want_idx=True):
    """kprn_host_find_paths_sampled (no handle, no GPU): host_find_paths with max_hops up to 5, the hops past 3 sampled by `walks` walks per pair and hop
    count (include/kprn.h "sampled paths of four and five hops") -> (idx, counts, found)"""
    sd, dr = _seed_draw(seed, draw)

    def call(src, dst, rel, nt, pr, B, F, counts, found, idx):
        return lib().kprn_host_find_paths_sampled(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), _fp(nt), int(nt.shape[0]), int(Vr), int(Vt),
                                                  int(nt.shape[1]), int(end_relation), _fp(pr), B, int(min_hops), int(max_hops), int(max_paths), int(T), F,
                                                  int(walks), sd, dr, int(threads), _fp(counts), _fp(found), _fp(idx))
    return _host_find(call, "kprn_host_find_paths_sampled", src, dst, rel, node_types, pairs, T, F, want_idx)


PATH_CAPS = {"first": 0, "spread": 1}   # option "path_cap" / the cap_mode of kprn_host_find_paths_cap (include/kprn.h "finding a pair's paths", cap mode)


def host_find_paths_cap(src, dst, rel, node_types, Vr, Vt, end_relation, pairs, min_hops, max_hops, max_paths, T, walks, seed, draw, cap="first", F=None,
                        threads=1, want_idx=True):
    """kprn_host_find_paths_cap (no handle, no GPU): host_find_paths_sampled with the cap mode -- "first" (exactly host_find_paths_sampled) or "spread", one
    path drawn in each of max_paths strata of a pair's sequence under (seed, draw) -> (idx, counts, found)"""
    if cap not in PATH_CAPS:
        raise KprnError(E_ARG, "cap must be first or spread")
    sd, dr = _seed_draw(seed, draw)

    def call(src, dst, rel, nt, pr, B, F, counts, found, idx):
        return lib().kprn_host_find_paths_cap(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), _fp(nt), int(nt.shape[0]), int(Vr), int(Vt),
                                              int(nt.shape[1]), int(end_relation), _fp(pr), B, int(min_hops), int(max_hops), int(max_paths), int(T), F,
                                              int(walks), sd, dr, PATH_CAPS[cap], int(threads), _fp(counts), _fp(found), _fp(idx))
    return _host_find(call, "kprn_host_find_paths_cap", src, dst, rel, node_types, pairs, T, F, want_idx)


PATTERN_MAX, PATTERN_MAX_HOPS = 32, 5   # KPRN_PATTERN_MAX; a pattern's positions (include/kprn.h "meta-paths")


def _delta_array(d):
    """a delta's additions or removals: [n, 3] int32 rows of (src, dst, rel); None or empty: no rows"""
    if d is None:
        return np.zeros((0, 3), np.int32)
    d = np.ascontiguousarray(d, np.int32)
    if d.size == 0:
        return np.zeros((0, 3), np.int32)
    if d.ndim != 2 or d.shape[1] != 3:
        raise KprnError(E_ARG, "a delta is [n, 3] = (src, dst, rel)")
    return d


def _delta_args(adds, removes):
    """the six delta arguments of kprn_graph_update / kprn_host_graph_update (the columns as arrays of their own, kept alive by the returned list)"""
    cols = [np.ascontiguousarray(d[:, k]) for d in (_delta_array(adds), _delta_array(removes)) for k in range(3)]
    a, r = cols[:3], cols[3:]
    return cols, ([_fp(c) if len(c) else None for c in a] + [C.c_int64(len(a[0]))] + [_fp(c) if len(c) else None for c in r] + [C.c_int64(len(r[0]))])


def host_graph_update(src, dst, rel, Ve, Vr, adds=None, removes=None):
    """kprn_host_graph_update (no handle, no GPU): the update rule of include/kprn.h "updating a graph in place" over an edge list in any order ->
    (rowptr [Ve + 1], col [E_new], rel [E_new], n_added, n_removed): the CSR kprn_graph_create stores for the updated edge set"""
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    if not (src.shape == dst.shape == rel.shape):
        raise KprnError(E_ARG, "a graph is src / dst / rel [E]")
    keep, args = _delta_args(adds, removes)
    room = int(src.shape[0]) + len(keep[0])
    rowptr, col, rel_out = np.zeros(int(Ve) + 1 if int(Ve) >= 0 else 1, np.int32), np.zeros(room + 1, np.int32), np.zeros(room + 1, np.int32)
    E_out, n_added, n_removed = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rc = lib().kprn_host_graph_update(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), int(Ve), int(Vr), *args, _fp(rowptr), _fp(col), _fp(rel_out),
                                      C.byref(E_out), C.byref(n_added), C.byref(n_removed))
    if rc != 0:
        raise KprnError(rc, "kprn_host_graph_update: bad graph ids / delta ids / sizes")
    n = int(E_out.value)
    return rowptr, col[:n].copy(), rel_out[:n].copy(), int(n_added.value), int(n_removed.value)


def _pattern_arrays(patterns):
    """patterns: a list of patterns, each a list of positions, each an iterable of relation ids or None / empty for any -> the four pattern arguments of
    kprn_graph_set_patterns: (hops [n] int32, set_offsets [S + 1] int64, set_rels int32, n); None or an empty list: (None, None, None, 0)"""
    if not patterns:
        return None, None, None, 0
    hops, offs, rels = [], [0], []
    for pat in patterns:
        pat = list(pat)
        hops.append(len(pat))
        for pos in pat:
            rels += [] if pos is None else [int(r) for r in pos]
            offs.append(len(rels))
    return np.array(hops, np.int32), np.array(offs, np.int64), np.array(rels if rels else [0], np.int32), len(hops)


def host_find_paths_patterns(src, dst, rel, node_types, Vr, Vt, end_relation, pairs, min_hops, max_hops, max_paths, T, walks=0, seed=0, draw=0, cap="first",
                             patterns=None, F=None, threads=1, want_idx=True):
    """kprn_host_find_paths_patterns (no handle, no GPU): host_find_paths_cap over the pairs' filtered sequences -- only the paths whose relation sequence
    matches one of `patterns` (include/kprn.h "meta-paths"; the form of Graph.set_patterns); no patterns: exactly host_find_paths_cap -> (idx, counts, found)"""
    if cap not in PATH_CAPS:
        raise KprnError(E_ARG, "cap must be first or spread")
    sd, dr = _seed_draw(seed, draw)
    ph, po, prl, n = _pattern_arrays(patterns)

    def call(src, dst, rel, nt, pr, B, F, counts, found, idx):
        return lib().kprn_host_find_paths_patterns(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), _fp(nt), int(nt.shape[0]), int(Vr), int(Vt),
                                                   int(nt.shape[1]), int(end_relation), _fp(pr), B, int(min_hops), int(max_hops), int(max_paths), int(T), F,
                                                   int(walks), sd, dr, PATH_CAPS[cap], int(threads), _fp(counts), _fp(found), _fp(idx), _fp(ph), _fp(po),
                                                   _fp(prl), n)
    return _host_find(call, "kprn_host_find_paths_patterns", src, dst, rel, node_types, pairs, T, F, want_idx)


def host_cap_select(found, max_paths, b, seed, draw):
    """kprn_host_cap_select: the ranks "spread" keeps of the pair in row b of a pair list that has `found` paths -> ranks [min(found, max_paths)] int64, ascending"""
    n = max(min(int(found), int(max_paths)), 0)
    ranks = np.zeros(n, np.int64)
    sd, dr = _seed_draw(seed, draw)
    rc = lib().kprn_host_cap_select(C.c_int64(int(found)), int(max_paths), int(b), sd, dr, _fp(ranks))
    if rc != 0:
        raise KprnError(rc, "kprn_host_cap_select: found must be in 0 .. 2^51 - 1, max_paths in 1..4096, b >= 0")
    return ranks


SAMPLE_MAX_NEG, SAMPLE_MAX_ATTEMPTS = 256, 64   # kprn_sample_negatives: negatives per user slot, attempts per negative


def _sampler_arrays(items, weights):
    it = np.ascontiguousarray(items, np.int32).reshape(-1)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w is not None and w.shape != it.shape:
        raise KprnError(E_ARG, "weights must be [M] like items")
    return it, w


def host_sample_negatives(src, dst, rel, Ve, items, weights, users, n_neg, seed, draw, max_attempts=16, threads=1, out=None):
    """kprn_host_sample_negatives (no handle, no GPU): the sampling rule of include/kprn.h over the graph's raw edge arrays -> (neg [B, n_neg], n_found [B]);
    `out` = (neg, n_found) arrays to write into (a refused call leaves them as they are)"""
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    if not (src.shape == dst.shape == rel.shape):
        raise KprnError(E_ARG, "a graph is src / dst / rel [E]")
    it, w = _sampler_arrays(items, weights)
    us = np.ascontiguousarray(users, np.int32).reshape(-1)
    B = int(us.shape[0])
    neg, nf = out if out is not None else (np.zeros((B, max(int(n_neg), 0)), np.int32), np.zeros(B, np.int32))
    sd, dr = _seed_draw(seed, draw)
    rc = lib().kprn_host_sample_negatives(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), int(Ve), _fp(it), _fp(w), C.c_int64(int(it.shape[0])), _fp(us),
                                          B, int(n_neg), int(max_attempts), sd, dr, int(threads), _fp(neg), _fp(nf))
    if rc != 0:
        raise KprnError(rc, "kprn_host_sample_negatives: bad edges / items / weights / users / n_neg / max_attempts")
    return neg, nf


def host_find_candidates(src, dst, rel, Ve, items, users, min_hops, max_hops, exclude_adjacent=True, threads=1):
    """kprn_host_find_candidates (no handle, no GPU): the rule of include/kprn.h "candidates of a user" over the graph's raw edge arrays and the catalogue
    `items` -> (cand [sum(group_counts)] entity ids, users in input order; group_counts [B]).  Two calls: the counts, then the ids"""
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    if not (src.shape == dst.shape == rel.shape):
        raise KprnError(E_ARG, "a graph is src / dst / rel [E]")
    it, _ = _sampler_arrays(items, None)
    us = np.ascontiguousarray(users, np.int32).reshape(-1)
    B = int(us.shape[0])
    gc = np.zeros(B, np.int32)

    def call(counts, cand):
        rc = lib().kprn_host_find_candidates(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), int(Ve), _fp(it), C.c_int64(int(it.shape[0])), _fp(us), B,
                                             int(min_hops), int(max_hops), int(bool(exclude_adjacent)), int(threads), _fp(counts), _fp(cand))
        if rc != 0:
            raise KprnError(rc, "kprn_host_find_candidates: bad edges / items / users / hops")
    call(gc, None)
    cand = np.zeros(int(gc.astype(np.int64).sum()), np.int32)
    if cand.size:
        call(np.zeros(B, np.int32), cand)
    return cand, gc


def host_find_candidates_top(src, dst, rel, Ve, items, users, min_hops, max_hops, cap, exclude_adjacent=True, threads=1):
    """kprn_host_find_candidates_top (no handle, no GPU): include/kprn.h "the N strongest candidates of a user" -> (cand [sum(group_counts)] entity ids,
    users in input order and ids ascending; group_counts [B]; n_paths [sum] int64).  Two calls: the counts, then the ids and path counts"""
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    if not (src.shape == dst.shape == rel.shape):
        raise KprnError(E_ARG, "a graph is src / dst / rel [E]")
    it, _ = _sampler_arrays(items, None)
    us = np.ascontiguousarray(users, np.int32).reshape(-1)
    B = int(us.shape[0])
    gc = np.zeros(B, np.int32)

    def call(counts, cand, n_paths):
        rc = lib().kprn_host_find_candidates_top(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), int(Ve), _fp(it), C.c_int64(int(it.shape[0])), _fp(us),
                                                 B, int(min_hops), int(max_hops), int(bool(exclude_adjacent)), C.c_int32(_as_cap(cap)), int(threads), _fp(counts),
                                                 _fp(cand), _fp(n_paths))
        if rc != 0:
            raise KprnError(rc, "kprn_host_find_candidates_top: bad edges / items / users / hops / cap")
    call(gc, None, None)
    total = int(gc.astype(np.int64).sum())
    cand, n_paths = np.zeros(total, np.int32), np.zeros(total, np.int64)
    if total:
        call(np.zeros(B, np.int32), cand, n_paths)
    return cand, gc, n_paths


EVAL_MAX_NEG = RANK_MAX_GROUP - 1   # kprn_sample_eval_groups: negatives per held pair (a group of kprn_rank_groups with its positive)


def _eval_sample_args(group_counts, target_offsets, target_items, n_neg):
    """the arrays of kprn_sample_eval_groups / kprn_host_sample_eval_groups; what the C call reads through an array's length is checked here, the rest there"""
    gc = np.ascontiguousarray(group_counts, np.int32).reshape(-1)
    toff = np.ascontiguousarray(target_offsets, np.int64).reshape(-1)
    ti = np.ascontiguousarray(target_items, np.int32).reshape(-1)
    B, n_neg = int(gc.shape[0]), int(n_neg)
    if toff.shape[0] != B + 1 or toff[-1] != ti.shape[0]:
        raise KprnError(E_ARG, "group_counts must be [B] and target_offsets [B+1] end at len(target_items)")
    NT = int(ti.shape[0])
    out = dict(group_counts=np.full(B, -3, np.int32), target_rows=np.full(NT, -3, np.int32),
               neg_rows=np.full((NT, min(max(n_neg, 1), EVAL_MAX_NEG)), -3, np.int32), n_drawn=np.full(NT, -3, np.int32))
    return gc, toff, ti, B, n_neg, out


def host_sample_eval_groups(pairs, Ve, group_counts, target_offsets, target_items, n_neg, seed, draw=0):
    """kprn_host_sample_eval_groups (no handle, no GPU): the rule of include/kprn.h "sampled evaluation groups" over a host candidate list `pairs`
    [total, 2] made on a graph of Ve entities -> dict(pairs [new_total, 2] the cut list, group_counts [B], target_rows [NT] (-1: unreachable), neg_rows
    [NT, n_neg] (rows of the cut list, ascending, -1-padded), n_drawn [NT])"""
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    gc, toff, ti, B, n_neg, out = _eval_sample_args(group_counts, target_offsets, target_items, n_neg)
    new_list = np.zeros((max(int(pr.shape[0]), 1), 2), np.int32)
    total = C.c_int64(-3)
    sd, dr = _seed_draw(seed, draw)
    rc = lib().kprn_host_sample_eval_groups(_fp(pr) if pr.size else None, C.c_int64(int(pr.shape[0])), int(Ve), _fp(gc), B, _fp(toff), _fp(ti), n_neg, sd, dr,
                                            _fp(out["group_counts"]), C.byref(total), _fp(out["target_rows"]), _fp(out["neg_rows"]), _fp(out["n_drawn"]),
                                            _fp(new_list))
    if rc != 0:
        raise KprnError(rc, "kprn_host_sample_eval_groups: bad list / group_counts / targets / n_neg")
    out["pairs"] = new_list[:int(total.value)].copy()
    return out


def host_find_candidates_patterns(src, dst, rel, Ve, items, users, min_hops, max_hops, cap=2**31 - 1, exclude_adjacent=True, patterns=None, threads=1):
    """kprn_host_find_candidates_patterns (no handle, no GPU): host_find_candidates_top where only the paths that match one of `patterns` count (include/kprn.h
    "meta-paths"); cap = 2^31 - 1: the plain candidates; no patterns: exactly host_find_candidates_top -> (cand, group_counts, n_paths)"""
    src, dst, rel = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (src, dst, rel))
    if not (src.shape == dst.shape == rel.shape):
        raise KprnError(E_ARG, "a graph is src / dst / rel [E]")
    it, _ = _sampler_arrays(items, None)
    us = np.ascontiguousarray(users, np.int32).reshape(-1)
    B = int(us.shape[0])
    gc = np.zeros(B, np.int32)
    ph, po, prl, n = _pattern_arrays(patterns)

    def call(counts, cand, n_paths):
        rc = lib().kprn_host_find_candidates_patterns(_fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), int(Ve), _fp(it), C.c_int64(int(it.shape[0])),
                                                      _fp(us), B, int(min_hops), int(max_hops), int(bool(exclude_adjacent)), C.c_int32(_as_cap(cap)), int(threads),
                                                      _fp(counts), _fp(cand), _fp(n_paths), _fp(ph), _fp(po), _fp(prl), n)
        if rc != 0:
            raise KprnError(rc, "kprn_host_find_candidates_patterns: bad edges / items / users / hops / cap / patterns")
    call(gc, None, None)
    total = int(gc.astype(np.int64).sum())
    cand, n_paths = np.zeros(total, np.int32), np.zeros(total, np.int64)
    if total:
        call(np.zeros(B, np.int32), cand, n_paths)
    return cand, gc, n_paths


def _as_cap(cap):
    """a cap as the int32 the library takes: anything outside int32 becomes a value it refuses (0) rather than one that wraps"""
    cap = int(cap)
    return cap if -2**31 <= cap <= 2**31 - 1 else 0


def format_score_lines(counter0, probs, labels):
    """bytes of the scoring writer's lines for pairs counter0 .. (kprn_format_score_lines; host-only)"""
    L = lib()
    probs = np.ascontiguousarray(probs, np.float32)
    labels = np.ascontiguousarray(labels, np.float32)
    n = int(probs.shape[0])
    cap = 32 * n + 64
    w = C.c_int64()
    while True:
        buf = C.create_string_buffer(cap)
        rc = L.kprn_format_score_lines(C.c_int64(int(counter0)), _fp(probs), _fp(labels), C.c_int64(n), buf, C.c_int64(cap), C.byref(w))
        if rc == 0:
            return buf.raw[:w.value]
        if w.value >= 0:
            raise KprnError(rc, "kprn_format_score_lines failed")
        cap = -w.value + 64


_lib = None


def lib():
    """Loads libkprn.so.  torch (if importable) is imported first so that both share ONE HIP runtime
    (torch bundles libamdhip64.so.7; the loader de-duplicates by SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m kprn_amd.build` "
                          "(hipcc --offload-arch=gfx950). kprn_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(LIB_PATH)
    L.kprn_last_error.restype = C.c_char_p
    L.kprn_last_error.argtypes = [C.c_void_p]
    L.kprn_version.restype = C.c_char_p
    L.kprn_destroy.restype = None
    L.kprn_destroy.argtypes = [C.c_void_p]
    L.kprn_batch_destroy.restype = None
    L.kprn_batch_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.kprn_graph_destroy.restype = None
    L.kprn_graph_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.kprn_sampler_destroy.restype = None
    L.kprn_sampler_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.kprn_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.kprn_host_free.argtypes = [C.c_void_p, C.c_void_p]
    _lib = L
    return L


_SLOW_FP = os.environ.get("KPRN_FFI_NUMPY_POINTERS") == "1"   # (measurement: ndarray.ctypes for every pointer, as before round 6)


def _fp(a):
    """the array's address as a ctypes pointer.  `ndarray.ctypes` builds a helper object per access (2.8 us a call: two of them were 4 % of a 128-pair
    kprn_train_step); the buffer protocol gives the same address in 0.9 us.  Empty, read-only and non-contiguous arrays take numpy's route."""
    if a is None:
        return None
    if _SLOW_FP:
        return a.ctypes.data_as(C.c_void_p)
    try:
        return C.c_void_p(C.addressof(C.c_char.from_buffer(a)))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data_as(C.c_void_p)


def make_opt(method=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, lr_decay=0.0, regularize=0, use_grad_clip=1,
             grad_clip_norm=5.0, l2=1e-3, bce_literal=0, entity_update=0):
    return Opt(method, lr, beta1, beta2, eps, lr_decay, regularize, use_grad_clip, grad_clip_norm, l2, bce_literal, entity_update)


class Batch:
    """A minibatch resident in HBM (BatcherFileList:populateGPUTensor, BatcherFileList.lua:78-96)."""

    def __init__(self, engine, idx, labels=None, feed=False):
        """feed=False: kprn_batch_create (ready on return).  feed=True: a slot for Batch.refill -- the upload and the index build
        run on the engine's feed stream, under whatever is queued next (kprn_batch_feed_async)."""
        self._attach(engine)
        if feed:
            self.refill(idx, labels)
            return
        idx, lab = self._check(idx, labels)
        engine._ck(engine.L.kprn_batch_create(engine.h, _fp(idx), _fp(lab), self.B, self.P, self.T, self.F, C.byref(self.ptr)))

    def _attach(self, engine):
        self.engine = engine
        self.ptr = C.c_void_p()
        self._src = None
        engine._batches.add(self)   # Engine.close() releases the batches still alive before the handle goes

    def _check(self, idx, labels):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 4:
            raise KprnError(E_ARG, "idx must be [B,P,T,F]")
        self.B, self.P, self.T, self.F = (int(x) for x in idx.shape)
        self.counts = None
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        if lab is not None and lab.shape != (self.B,):
            raise KprnError(E_ARG, "labels must be [B]")
        self.has_labels = lab is not None
        return idx, lab

    @classmethod
    def reserve(cls, engine, max_pairs, max_paths, T, F, with_labels=True):
        """an empty feed slot sized for the largest minibatch it will hold (kprn_batch_slot_reserve)"""
        self = cls.__new__(cls)
        self._attach(engine)
        self.B = self.P = 0
        self.counts = None
        self.T, self.F, self.has_labels = T, F, with_labels
        engine._ck(engine.L.kprn_batch_slot_reserve(engine.h, C.byref(self.ptr), int(max_pairs), C.c_int64(int(max_paths)), int(T), int(F), int(bool(with_labels))))
        return self

    def refill(self, idx, labels=None):
        """streaming feed: new contents for this slot, asynchronously.  idx / labels should live in page-locked memory
        (Engine.host_array) and must stay unchanged until the slot is first used."""
        idx, lab = self._check(idx, labels)
        self._src = (idx, lab)  # keep the host buffers alive until the copy has run
        self.engine._ck(self.engine.L.kprn_batch_feed_async(self.engine.h, C.byref(self.ptr), _fp(idx), _fp(lab), self.B, self.P, self.T, self.F))
        return self

    def _check_ragged(self, idx, counts, labels):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if idx.ndim != 3 or counts.ndim != 1 or counts.shape[0] < 1:
            raise KprnError(E_ARG, "a ragged batch is idx [N,T,F] and counts [B]")
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        if lab is not None and lab.shape != counts.shape:
            raise KprnError(E_ARG, "labels must be [B]")
        return idx, counts, lab

    def _set_ragged(self, idx, counts, lab):
        self.B, self.P = int(counts.shape[0]), 0
        self.N, self.T, self.F = (int(x) for x in idx.shape)
        self.counts = counts
        self.has_labels = lab is not None

    @classmethod
    def ragged(cls, engine, idx, counts, labels=None, feed=False):
        """a ragged batch (kprn_batch_create_ragged): pair b owns counts[b] consecutive paths of idx [N,T,F].  feed=True: through the
        streaming feed, as Batch(..., feed=True)."""
        self = cls.__new__(cls)
        self._attach(engine)
        self.counts = None
        if feed:
            return self.refill_ragged(idx, counts, labels)
        idx, counts, lab = self._check_ragged(idx, counts, labels)
        engine._ck(engine.L.kprn_batch_create_ragged(engine.h, _fp(idx), _fp(counts), _fp(lab), int(counts.shape[0]), C.c_int64(int(idx.shape[0])),
                                                     int(idx.shape[1]), int(idx.shape[2]), C.byref(self.ptr)))
        self._set_ragged(idx, counts, lab)
        return self

    def refill_ragged(self, idx, counts, labels=None):
        """streaming feed of a ragged batch into this slot (kprn_batch_feed_ragged_async); the slot may have held a rectangular batch"""
        idx, counts, lab = self._check_ragged(idx, counts, labels)
        self._src = (idx, lab)
        self.engine._ck(self.engine.L.kprn_batch_feed_ragged_async(self.engine.h, C.byref(self.ptr), _fp(idx), _fp(counts), _fp(lab), int(counts.shape[0]),
                                                                   C.c_int64(int(idx.shape[0])), int(idx.shape[1]), int(idx.shape[2])))
        self._set_ragged(idx, counts, lab)
        return self

    def refill_rows(self, data, labels, rows):
        """shuffled streaming feed (kprn_batch_feed_rows_async): pair i of the minibatch = row rows[i] of the file's arrays
        data [n,P,T,F] int32 / labels [n] float32, gathered by the engine's worker threads -- no host-side copy here."""
        if data.dtype != np.int32 or not data.flags.c_contiguous or data.ndim != 4:
            raise KprnError(E_ARG, "data must be a C-contiguous int32 [n,P,T,F] array")
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        self.B, (_, self.P, self.T, self.F) = int(rows.shape[0]), (int(x) for x in data.shape)
        self.counts = None
        self.has_labels = lab is not None
        self._src = (data, lab, rows)   # alive until the worker threads have read them
        self.engine._ck(self.engine.L.kprn_batch_feed_rows_async(self.engine.h, C.byref(self.ptr), _fp(data), _fp(lab), C.c_int64(int(data.shape[0])), _fp(rows),
                                                                   self.B, self.P, self.T, self.F))
        return self

    @classmethod
    def _adopt(cls, engine, ptr, counts, T, F, has_labels):
        """the ragged batch a library call made (kprn_find_paths)"""
        self = cls.__new__(cls)
        self._attach(engine)
        self.ptr = ptr
        self.B, self.P = int(counts.shape[0]), 0
        self.N, self.T, self.F = int(counts.astype(np.int64).sum()), int(T), int(F)
        self.counts = counts
        self.has_labels = has_labels
        return self

    def set_groups(self, group_offsets):
        """kprn_batch_set_groups: the group table [G+1] over this batch's consecutive pairs that the pairwise loss (option "loss" = "bpr") trains on -> n_terms,
        the (positive, negative) pairs within the groups.  The table goes with the contents: a refill drops it.  Raises KprnError(E_ARG) for a bad table"""
        go = np.ascontiguousarray(group_offsets, np.int32).reshape(-1)
        n = C.c_int64()
        self.engine._ck(self.engine.L.kprn_batch_set_groups(self.engine.h, self.ptr, _fp(go), int(go.shape[0]) - 1, C.byref(n)))
        return int(n.value)

    @property
    def n_paths(self):
        return self.N if getattr(self, "counts", None) is not None else self.B * self.P

    def read_idx(self):
        """kprn_batch_read_idx: the batch's ids [N,T,F] in the caller's path order, back on the host"""
        out = np.empty((self.n_paths, self.T, self.F), np.int32)
        self.engine._ck(self.engine.L.kprn_batch_read_idx(self.engine.h, self.ptr, _fp(out)))
        return out

    @property
    def n_uniq(self):
        """distinct entity rows of the batch (the rows one training step touches)"""
        n = C.c_int32()
        self.engine._ck(self.engine.L.kprn_batch_distinct_rows(self.engine.h, self.ptr, C.byref(n)))
        return int(n.value)

    @property
    def executed_steps(self):
        """(path, step) positions a pass executes: B*P*T less the identical leading steps that are run once per batch"""
        n = C.c_int64()
        self.engine._ck(self.engine.L.kprn_batch_executed_steps(self.engine.h, self.ptr, C.byref(n)))
        return int(n.value)

    @property
    def handover_stats(self):
        """time-split tile hand-over on this batch: (pairs, steps moved, longest workgroup in half steps without, with)"""
        out = (C.c_int64 * 4)()
        self.engine._ck(self.engine.L.kprn_batch_handover_stats(self.engine.h, self.ptr, out))
        return tuple(int(v) for v in out)

    def free(self):
        if self.ptr:
            self.engine.L.kprn_batch_destroy(self.engine.h, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            if self.engine.h:
                self.free()
        except Exception:
            pass


class Graph:
    """A knowledge graph resident in HBM as CSR (kprn_graph_create): the input of Engine.find_paths."""

    def __init__(self, engine, src, dst, rel, node_types, end_relation):
        src, dst, rel, nt = _graph_arrays(src, dst, rel, node_types)
        if nt.shape != (engine.cfg.Ve, engine.cfg.num_types):
            raise KprnError(E_ARG, "node_types must be [Ve, num_types] of the engine")
        self.engine = engine
        self.ptr = C.c_void_p()
        engine._graphs.add(self)
        engine._ck(engine.L.kprn_graph_create(engine.h, _fp(src), _fp(dst), _fp(rel), C.c_int64(int(src.shape[0])), _fp(nt), int(end_relation), C.byref(self.ptr)))

    @property
    def n_edges(self):
        """edges stored: the input's less duplicates and self-loops"""
        n = C.c_int64()
        self.engine._ck(self.engine.L.kprn_graph_num_edges(self.engine.h, self.ptr, C.byref(n)))
        return int(n.value)

    def update(self, adds=None, removes=None):
        """kprn_graph_update (include/kprn.h "updating a graph in place"): adds / removes are [n, 3] int32 rows of (src, dst, rel); the removals apply first;
        a removal's rel 0 names every stored edge src -> dst.  Afterwards the graph stores what a fresh build of the edited edge set stores, bit for bit.
        A refused call leaves the graph untouched -> (n_added, n_removed)"""
        keep, args = _delta_args(adds, removes)
        n_added, n_removed = C.c_int64(), C.c_int64()
        self.engine._ck(self.engine.L.kprn_graph_update(self.engine.h, self.ptr, *args, C.byref(n_added), C.byref(n_removed)))
        return int(n_added.value), int(n_removed.value)

    def read_csr(self):
        """kprn_graph_read: the CSR as stored -> (rowptr [Ve + 1], col [E], rel [E]) int32"""
        E = self.n_edges
        rowptr, col, rel = np.zeros(self.engine.cfg.Ve + 1, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)
        self.engine._ck(self.engine.L.kprn_graph_read(self.engine.h, self.ptr, _fp(rowptr), _fp(col) if E else None, _fp(rel) if E else None))
        return rowptr, col, rel

    def set_node_types(self, entities, rows):
        """kprn_graph_set_node_types: the type rows of `entities` [n] become rows [n, num_types] (a node that first appears in a delta has the row the
        graph was created with)"""
        ent = np.ascontiguousarray(entities, np.int32).reshape(-1)
        rows = np.ascontiguousarray(rows, np.int32)
        if rows.shape != (ent.shape[0], self.engine.cfg.num_types):
            raise KprnError(E_ARG, "rows must be [n, num_types] for entities [n]")
        self.engine._ck(self.engine.L.kprn_graph_set_node_types(self.engine.h, self.ptr, _fp(ent) if len(ent) else None, _fp(rows) if len(ent) else None,
                                                                C.c_int64(len(ent))))

    def set_patterns(self, patterns):
        """kprn_graph_set_patterns (include/kprn.h "meta-paths"): from the next call on, every device call that takes this graph sees only the paths whose
        relation sequence matches a pattern.  patterns: a list of patterns; a pattern: a list of 1..5 positions; a position: an iterable of relation ids, or
        None / empty for any relation.  None or an empty list clears the set.  A refused call leaves the previous set in place"""
        ph, po, prl, n = _pattern_arrays(patterns)
        self.engine._ck(self.engine.L.kprn_graph_set_patterns(self.engine.h, self.ptr, _fp(ph), _fp(po), _fp(prl), n))

    def num_patterns(self):
        n = C.c_int32()
        self.engine._ck(self.engine.L.kprn_graph_num_patterns(self.engine.h, self.ptr, C.byref(n)))
        return int(n.value)

    def free(self):
        if self.ptr:
            self.engine.L.kprn_graph_destroy(self.engine.h, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            if self.engine.h:
                self.free()
        except Exception:
            pass


class Sampler:
    """A weighted candidate list resident in HBM (kprn_sampler_create): the input of Engine.sample_negatives / find_training_paths."""

    def __init__(self, engine, items, weights=None):
        it, w = _sampler_arrays(items, weights)
        self.engine = engine
        self.ptr = C.c_void_p()
        self.M = int(it.shape[0])
        engine._samplers.add(self)
        engine._ck(engine.L.kprn_sampler_create(engine.h, _fp(it), _fp(w), C.c_int64(self.M), C.byref(self.ptr)))

    def free(self):
        if self.ptr:
            self.engine.L.kprn_sampler_destroy(self.engine.h, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            if self.engine.h:
                self.free()
        except Exception:
            pass


STREAM_LEGACY_DEFAULT = C.c_void_p(-1).value   # kprn_config.stream: queue on the legacy default (null) stream (KPRN_STREAM_LEGACY_DEFAULT)


class Engine:
    """Thin object wrapper over one kprn_handle.  stream: None = the engine creates its own; a hipStream_t handle; or
    STREAM_LEGACY_DEFAULT for the null stream (whose handle, 0, would otherwise read as "create your own")."""

    def __init__(self, Vt, Ve, Vr, dt, de, dr, H, L=1, F=3, num_types=1, C_=46, reducer=2, K=5, rnn_type=0, device_id=0,
                 rank=0, world=1, param_init=0.1, seed=12345, stream=None, use_relu=1, rnn_init=0, compute_dtype=0):
        self.L = lib()
        self._batches = weakref.WeakSet()
        self._graphs = weakref.WeakSet()
        self._samplers = weakref.WeakSet()
        self.options = {}   # what set_option has set on this handle (the library has no getter): key -> last accepted value
        self.cfg = Config(Vt, Ve, Vr, dt, de, dr, F, num_types, H, L, C_, rnn_type, use_relu, rnn_init, compute_dtype, reducer, K, device_id, rank, world,
                          param_init, seed, stream)
        self.h = C.c_void_p()
        rc = self.L.kprn_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise KprnError(rc, (self.L.kprn_last_error(None) or b"").decode())
        n = C.c_int64()
        self._ck(self.L.kprn_num_params(self.h, C.byref(n)))
        self.n_params = int(n.value)
        self.D = dt + de + dr
        if os.environ.get("KPRN_SMALL_TILES") is not None:   # (tests: the 64-path tiles + identical-prefix plan at small sizes too)
            self.set_option("small_tiles", os.environ["KPRN_SMALL_TILES"])

    # -- plumbing ------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise KprnError(rc, (self.L.kprn_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            for b in list(self._batches):   # (device blocks, page-locked images and events of batches the caller still holds)
                b.free()
            for g in list(self._graphs) + list(self._samplers):
                g.free()
            for p in getattr(self, "_pinned", []):
                self.L.kprn_host_free(self.h, p)
            self._pinned = []
            self.L.kprn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def layout(self):
        """name -> (flat offset, shape) in nn.Module:getParameters() order."""
        c = self.cfg
        out, off = {}, 0
        items = [("type_emb", (c.Vt, c.dt)), ("entity_emb", (c.Ve, c.de)), ("relation_emb", (c.Vr, c.dr))]
        for i in range(c.L):
            din = self.D if i == 0 else c.H
            if c.rnn_type == 1:  # nn.Recurrence: i2h / h2h nn.Linear (OneModel.lua:231-232)
                items += [(f"rnn{i + 1}.i2h.weight", (c.H, din)), (f"rnn{i + 1}.i2h.bias", (c.H,)),
                          (f"rnn{i + 1}.h2h.weight", (c.H, c.H)), (f"rnn{i + 1}.h2h.bias", (c.H,))]
            elif c.rnn_type == 2:  # nn.GRU: gates (r, z) + candidate maps
                items += [(f"gru{i + 1}.i2g.weight", (2 * c.H, din)), (f"gru{i + 1}.i2g.bias", (2 * c.H,)),
                          (f"gru{i + 1}.o2g.weight", (2 * c.H, c.H)), (f"gru{i + 1}.c_i2h.weight", (c.H, din)),
                          (f"gru{i + 1}.c_i2h.bias", (c.H,)), (f"gru{i + 1}.c_h2h.weight", (c.H, c.H))]
            else:
                items += [(f"lstm{i + 1}.i2g.weight", (4 * c.H, din)), (f"lstm{i + 1}.i2g.bias", (4 * c.H,)),
                          (f"lstm{i + 1}.o2g.weight", (4 * c.H, c.H))]
        items += [("out.weight", (c.C, c.H)), ("out.bias", (c.C,))]
        for nm, shp in items:
            out[nm] = (off, shp)
            off += int(np.prod(shp))
        assert off == self.n_params
        return out

    # -- parameters ----------------------------------------------------------------------
    def _shape(self, name):
        lay = self.layout()
        if name not in lay:  # let the library produce its own error code / message
            self._ck(self.L.kprn_get_param(self.h, str(name).encode(), None, C.c_int64(0)))
            raise KprnError(E_ARG, f"unknown parameter name: {name}")
        return lay[name][1]

    def get_param(self, name):
        shp = self._shape(name)
        a = np.empty(shp, np.float32)
        self._ck(self.L.kprn_get_param(self.h, name.encode(), _fp(a), C.c_int64(a.size)))
        return a

    def set_param(self, name, value):
        a = np.ascontiguousarray(value, np.float32)
        self._ck(self.L.kprn_set_param(self.h, name.encode(), _fp(a), C.c_int64(a.size)))

    def get_param_rows(self, name, rows):
        """rows (0-based) of one parameter tensor: [len(rows), cols]"""
        rows = np.ascontiguousarray(rows, np.int64)
        out = np.empty((len(rows), self._shape(name)[1] if len(self._shape(name)) > 1 else 1), np.float32)
        self._ck(self.L.kprn_get_param_rows(self.h, name.encode(), _fp(rows), C.c_int64(len(rows)), _fp(out)))
        return out

    def set_param_rows(self, name, rows, values):
        rows = np.ascontiguousarray(rows, np.int64)
        values = np.ascontiguousarray(values, np.float32)
        self._ck(self.L.kprn_set_param_rows(self.h, name.encode(), _fp(rows), C.c_int64(len(rows)), _fp(values)))

    def get_grad(self, name):
        shp = self._shape(name)
        a = np.empty(shp, np.float32)
        self._ck(self.L.kprn_get_grad(self.h, name.encode(), _fp(a), C.c_int64(a.size)))
        return a

    def get_flat_params(self):
        a = np.empty(self.n_params, np.float32)
        self._ck(self.L.kprn_get_flat_params(self.h, _fp(a), C.c_int64(a.size)))
        return a

    def set_flat_params(self, theta):
        a = np.ascontiguousarray(theta, np.float32)
        self._ck(self.L.kprn_set_flat_params(self.h, _fp(a), C.c_int64(a.size)))

    def get_flat_grads(self):
        a = np.empty(self.n_params, np.float32)
        self._ck(self.L.kprn_get_flat_grads(self.h, _fp(a), C.c_int64(a.size)))
        return a

    def get_flat_opt_state(self, slot):
        a = np.empty(self.n_params, np.float32)
        self._ck(self.L.kprn_get_flat_opt_state(self.h, int(slot), _fp(a), C.c_int64(a.size)))
        return a

    def zero_pad_tokens(self):
        self._ck(self.L.kprn_zero_pad_tokens(self.h))

    # -- scoring -------------------------------------------------------------------------
    def batch(self, idx, labels=None):
        return Batch(self, idx, labels)

    def feed(self, idx, labels=None, slot=None):
        """streaming feed (BatcherFileList.lua:53-96): fills `slot` (or a new one) on the feed stream and returns at once"""
        if slot is None:
            return Batch(self, idx, labels, feed=True)
        return slot.refill(idx, labels)

    def batch_ragged(self, idx, counts, labels=None):
        """B pairs with their own path counts in one batch: idx [N,T,F], counts [B] (>= 1, sum N).  Accepted wherever a Batch is."""
        return Batch.ragged(self, idx, counts, labels)

    def feed_ragged(self, idx, counts, labels=None, slot=None):
        """the streaming feed for a ragged batch; `slot` may be any Batch (its previous contents may have been rectangular)"""
        if slot is None:
            return Batch.ragged(self, idx, counts, labels, feed=True)
        return slot.refill_ragged(idx, counts, labels)

    def forward_ragged_host(self, idx, counts, class_id=1, want_all=False):
        """kprn_forward_ragged: host buffers in, the selected class's probabilities [B] (and all classes [B,C]) out, one call"""
        idx = np.ascontiguousarray(idx, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        if idx.ndim != 3 or counts.ndim != 1:
            raise KprnError(E_ARG, "a ragged batch is idx [N,T,F] and counts [B]")
        B = int(counts.shape[0])
        probs = np.empty(B, np.float32)
        allp = np.empty((B, self.cfg.C), np.float32) if want_all else None
        self._ck(self.L.kprn_forward_ragged(self.h, _fp(idx), _fp(counts), B, C.c_int64(int(idx.shape[0])), int(idx.shape[1]), int(idx.shape[2]),
                                            int(class_id), _fp(probs), _fp(allp)))
        return probs, allp

    def feed_rows(self, data, labels, rows, slot=None):
        """the feed for a shuffled order: rows of the file's arrays, gathered inside the engine (Batch.refill_rows)"""
        if slot is None:
            slot = Batch.__new__(Batch)
            slot._attach(self)
        return slot.refill_rows(data, labels, rows)

    def host_array(self, shape, dtype=np.int32):
        """numpy array in page-locked host memory (kprn_host_alloc): the staging buffers of the streaming feed"""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._ck(self.L.kprn_host_alloc(self.h, C.c_size_t(max(n, 1)), C.byref(p)))
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return arr

    def forward(self, batch, class_id=1, want=("probs",)):
        """want: any of probs [B], all_probs [B,C], pooled [B,C], path_scores [B*P,C]."""
        if not isinstance(batch, Batch):
            batch = Batch(self, batch)
        c = self.cfg
        bufs = {"probs": np.empty(batch.B, np.float32) if "probs" in want else None,
                "all_probs": np.empty((batch.B, c.C), np.float32) if "all_probs" in want else None,
                "pooled": np.empty((batch.B, c.C), np.float32) if "pooled" in want else None,
                "path_scores": np.empty((batch.n_paths, c.C), np.float32) if "path_scores" in want else None}
        self._ck(self.L.kprn_forward_batch(self.h, batch.ptr, int(class_id), _fp(bufs["probs"]), _fp(bufs["all_probs"]),
                                           _fp(bufs["pooled"]), _fp(bufs["path_scores"])))
        return {k: v for k, v in bufs.items() if v is not None}

    def forward_host(self, idx, class_id=1, want_all=True):
        """the host-pointer entry point kprn_forward (one H2D copy per call).  want_all=False: only the selected class's probabilities come back --
        what test_from_checkpoint.lua:82,109 reads (its model ends in nn.Select(2, 1)); returns (probs, None)."""
        idx = np.ascontiguousarray(idx, np.int32)
        B, P, T, F = idx.shape
        probs = np.empty(B, np.float32)
        allp = np.empty((B, self.cfg.C), np.float32) if want_all else None
        self._ck(self.L.kprn_forward(self.h, _fp(idx), B, P, T, F, int(class_id), _fp(probs), _fp(allp)))
        return probs, allp

    def forward_async(self, batch, class_id=1):
        self._ck(self.L.kprn_forward_batch_async(self.h, batch.ptr, int(class_id)))

    def forward_async_rest(self):
        """second part of a split scoring pass (set_option("score_split", f))"""
        self._ck(self.L.kprn_forward_batch_async_rest(self.h))

    def read_probs(self, B):
        a = np.empty(B, np.float32)
        self._ck(self.L.kprn_read_probs(self.h, _fp(a), int(B)))
        return a

    # -- ranking (include/kprn.h "ranking") ------------------------------------------------
    def board_reserve(self, n):
        """device-resident scores addressed by global line number; every entry starts as NaN"""
        self._ck(self.L.kprn_board_reserve(self.h, C.c_int64(int(n))))

    def board_put(self, offset, B):
        """the most recent scoring pass's probabilities (what read_probs(B) would return) -> board[offset : offset + B], asynchronously"""
        self._ck(self.L.kprn_board_put(self.h, C.c_int64(int(offset)), int(B)))

    def board_write(self, offset, scores):
        a = np.ascontiguousarray(scores, np.float32)
        self._ck(self.L.kprn_board_write(self.h, C.c_int64(int(offset)), _fp(a), C.c_int64(a.size)))

    def board_read(self, offset, n):
        a = np.empty(int(n), np.float32)
        self._ck(self.L.kprn_board_read(self.h, C.c_int64(int(offset)), _fp(a), C.c_int64(a.size)))
        return a

    def rank_groups(self, group_offsets, members=None, pos=None, mode=0, K=0, hist_len=15):
        """kprn_rank_groups over the board: -> dict(ranks [G], hist [hist_len + 4], and with K > 0 topk_idx / topk_score [G,K])"""
        goff, G, mem, p, out = _rank_args(group_offsets, members, pos, K, hist_len)
        self._ck(self.L.kprn_rank_groups(self.h, _fp(mem), _fp(goff), _fp(p), G, int(mode), int(K) if K > 0 else 1, _fp(out["ranks"]),
                                         _fp(out.get("topk_idx")), _fp(out.get("topk_score")), _fp(out["hist"]), int(hist_len)))
        return out

    def rank_targets(self, group_offsets, target_offsets, targets, members=None, mode=0, hist_len=15, out=None):
        """kprn_rank_targets over the board: groups of any size, group g's targets = targets[target_offsets[g] : target_offsets[g + 1]] (indices within
        the group, ascending), each placed among the group's non-targets -> dict(places [NT], hist [hist_len + 4]); out: a dict to write into"""
        goff, toff, tg, mem, G, res = _rank_targets_args(group_offsets, target_offsets, targets, members, hist_len)
        res = res if out is None else out
        self._ck(self.L.kprn_rank_targets(self.h, _fp(mem), _fp(goff), _fp(toff), _fp(tg), G, int(mode), _fp(res["places"]), _fp(res["hist"]), int(hist_len)))
        return res

    # -- hard negatives (include/kprn.h "hard negatives") ---------------------------------------
    def select_hardest(self, group_offsets, n_keep, members=None, pos=None, keep=None):
        """kprn_select_hardest over the board: per group its positive pos[g] (-1 / None: none) and the n_keep other members that score highest (raw fp32 order,
        NaN last, ties to the lower index) -> (keep uint8 [group_offsets[G]] in member order, n_invalid); keep: an array to write into"""
        goff, G, mem, p, keep = _select_args(group_offsets, members, pos, keep)
        ninv = C.c_int64(0)
        self._ck(self.L.kprn_select_hardest(self.h, _fp(mem), _fp(goff), _fp(p), G, int(n_keep), _fp(keep), C.byref(ninv)))
        return keep, int(ninv.value)

    def batch_subset(self, batch, keep):
        """kprn_batch_subset: a ragged Batch of the pairs of `batch` (ragged or rectangular) with keep[b] != 0, in order, their rows taken from the batch where
        they lie in HBM and their labels with them -> the Batch, or None when nothing is kept.  `batch` stays as it was"""
        kp = np.ascontiguousarray(keep).reshape(-1)
        if kp.shape[0] != batch.B:
            raise KprnError(E_ARG, "keep must have one entry per pair of the batch")
        kp = np.ascontiguousarray(kp != 0, np.uint8)
        ptr = C.c_void_p()
        self._ck(self.L.kprn_batch_subset(self.h, batch.ptr, _fp(kp), C.byref(ptr)))
        if not ptr:
            return None
        src_counts = batch.counts if getattr(batch, "counts", None) is not None else np.full(batch.B, batch.P, np.int32)
        return Batch._adopt(self, ptr, np.ascontiguousarray(src_counts[kp != 0], np.int32), batch.T, batch.F, batch.has_labels)

    def recommend_ragged(self, idx, counts, group_counts, K, class_id=1, mode=0, want_probs=False):
        """kprn_recommend_ragged: idx [N,T,F] / counts [B] as forward_ragged_host; group_counts [G] pairs per group (sum B) ->
        (topk_idx [G,K] index within the group, topk_score [G,K], probs [B] or None)"""
        idx = np.ascontiguousarray(idx, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        gc = np.ascontiguousarray(group_counts, np.int32)
        if idx.ndim != 3 or counts.ndim != 1 or gc.ndim != 1 or K < 1:
            raise KprnError(E_ARG, "a ragged batch is idx [N,T,F] and counts [B]; group_counts [G]; K >= 1")
        B, G = int(counts.shape[0]), int(gc.shape[0])
        ti = np.full((G, K), -3, np.int32)
        ts = np.zeros((G, K), np.float32)
        probs = np.empty(B, np.float32) if want_probs else None
        self._ck(self.L.kprn_recommend_ragged(self.h, _fp(idx), _fp(counts), B, C.c_int64(int(idx.shape[0])), int(idx.shape[1]), int(idx.shape[2]),
                                              int(class_id), _fp(gc), G, int(mode), int(K), _fp(ti), _fp(ts), _fp(probs)))
        return ti, ts, probs

    # -- path finder (include/kprn.h "finding a pair's paths") ---------------------------------
    def graph(self, src, dst, rel, node_types, end_relation):
        """kprn_graph_create: directed edges (src, rel, dst) [E] with 1-based ids, node_types [Ve, num_types] (row e - 1 = entity e's type slots)"""
        return Graph(self, src, dst, rel, node_types, end_relation)

    def find_paths(self, graph, pairs, min_hops, max_hops, max_paths, T, labels=None, walks=0, seed=0, draw=0):
        """kprn_find_paths: every path of min_hops .. max_hops (<= 3) hops between the pairs [B,2] = (user, item), the first max_paths per pair in the
        canonical order -> (ragged Batch of the pairs that have paths, or None when none has; counts [B]; found [B]).  walks > 0:
        kprn_find_paths_sampled, max_hops up to 5 with the hops past 3 sampled by `walks` walks per pair and hop count under (seed, draw).  An engine whose
        option "path_cap" is "spread" takes the seeded call at walks == 0 too (kprn_find_paths has no seed and always keeps the first paths)"""
        pr, lab = _pairs_array(pairs, labels)
        B = int(pr.shape[0])
        counts, found = np.zeros(B, np.int32), np.zeros(B, np.int64)
        ptr = C.c_void_p()
        if int(walks) != 0 or self.options.get("path_cap", "first") == "spread":
            sd, dr = _seed_draw(seed, draw)
            self._ck(self.L.kprn_find_paths_sampled(self.h, graph.ptr, _fp(pr), _fp(lab), B, int(min_hops), int(max_hops), int(max_paths), int(T), int(walks), sd, dr,
                                                    _fp(counts), _fp(found), C.byref(ptr)))
        else:
            self._ck(self.L.kprn_find_paths(self.h, graph.ptr, _fp(pr), _fp(lab), B, int(min_hops), int(max_hops), int(max_paths), int(T), _fp(counts), _fp(found),
                                            C.byref(ptr)))
        if not ptr:
            return None, counts, found
        return Batch._adopt(self, ptr, counts[counts > 0].copy(), T, self.cfg.F, lab is not None), counts, found

    # -- negative sampler (include/kprn.h "sampling negatives") -------------------------------
    def sampler(self, items, weights=None):
        """kprn_sampler_create: candidate items [M] (entity ids, strictly ascending) and their weights (None = uniform)"""
        return Sampler(self, items, weights)

    def sample_negatives(self, graph, sampler, users, n_neg, seed, draw, max_attempts=16, out=None):
        """kprn_sample_negatives: n_neg distinct items per user slot, none the user or adjacent to it in `graph` -> (neg [B, n_neg] with 0 = no item found,
        n_found [B]); `out` = (neg, n_found) arrays to write into"""
        us = np.ascontiguousarray(users, np.int32).reshape(-1)
        B = int(us.shape[0])
        neg, nf = out if out is not None else (np.zeros((B, max(int(n_neg), 0)), np.int32), np.zeros(B, np.int32))
        sd, dr = _seed_draw(seed, draw)
        self._ck(self.L.kprn_sample_negatives(self.h, graph.ptr, sampler.ptr, _fp(us), B, int(n_neg), int(max_attempts), sd, dr, _fp(neg), _fp(nf)))
        return neg, nf

    def find_training_paths(self, graph, sampler, positives, n_neg, seed, draw, min_hops, max_hops, max_paths, T, max_attempts=16, walks=0):
        """kprn_find_training_paths: the positives [B,2] = (user, item), each with n_neg negatives sampled on the device, through the finder ->
        (ragged Batch with labels 1 / 0 of the pairs that have paths, or None; pairs [B * (1 + n_neg), 2]; counts; found).  walks > 0:
        kprn_find_training_paths_sampled, max_hops up to 5 (the same seed and draw serve the negatives and the walks)"""
        pos, _ = _pairs_array(positives, None)
        B = int(pos.shape[0])
        n = B * (1 + max(int(n_neg), 0))
        pairs, counts, found = np.zeros((n, 2), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        ptr = C.c_void_p()
        sd, dr = _seed_draw(seed, draw)
        if int(walks) != 0:
            self._ck(self.L.kprn_find_training_paths_sampled(self.h, graph.ptr, sampler.ptr, _fp(pos), B, int(n_neg), int(max_attempts), sd, dr, int(min_hops),
                                                             int(max_hops), int(max_paths), int(T), int(walks), _fp(pairs), _fp(counts), _fp(found), C.byref(ptr)))
        else:
            self._ck(self.L.kprn_find_training_paths(self.h, graph.ptr, sampler.ptr, _fp(pos), B, int(n_neg), int(max_attempts), sd, dr, int(min_hops),
                                                     int(max_hops), int(max_paths), int(T), _fp(pairs), _fp(counts), _fp(found), C.byref(ptr)))
        if not ptr:
            return None, pairs, counts, found
        return Batch._adopt(self, ptr, counts[counts > 0].copy(), T, self.cfg.F, True), pairs, counts, found

    # -- candidates of a user (include/kprn.h "candidates of a user") ---------------------------
    def find_candidates(self, graph, sampler, users, min_hops, max_hops, exclude_adjacent=True, cap=0):
        """kprn_find_candidates + kprn_read_candidates: the members of the sampler's item list that min_hops .. max_hops (<= 3) hops reach from each of
        `users`, less the user and (exclude_adjacent) the items it has an edge to -> (pairs [total, 2] = (user, item), users in input order and items
        ascending; group_counts [B]).  The list stays on the device for find_paths_of_candidates.
        cap > 0: kprn_find_candidates_top, at most `cap` per user, the strongest by path count (include/kprn.h "the N strongest candidates of a user");
        candidate_path_counts() then returns the counts"""
        us = np.ascontiguousarray(users, np.int32).reshape(-1)
        B = int(us.shape[0])
        gc = np.zeros(B, np.int32)
        total = C.c_int64()
        if cap == 0:
            self._ck(self.L.kprn_find_candidates(self.h, graph.ptr, sampler.ptr, _fp(us), B, int(min_hops), int(max_hops), int(bool(exclude_adjacent)), _fp(gc),
                                                 C.byref(total)))
        else:
            self._ck(self.L.kprn_find_candidates_top(self.h, graph.ptr, sampler.ptr, _fp(us), B, int(min_hops), int(max_hops), int(bool(exclude_adjacent)),
                                                     C.c_int32(_as_cap(cap)), _fp(gc), C.byref(total)))
        self._cand_total = int(total.value)
        pairs = np.zeros((int(total.value), 2), np.int32)
        self._ck(self.L.kprn_read_candidates(self.h, _fp(pairs), C.c_int64(int(total.value))))
        return pairs, gc

    def candidate_path_counts(self):
        """kprn_read_candidate_paths: n_paths [total] int64 of the candidate list a find_candidates(cap > 0) left, row for row (KprnError E_ARG after a
        plain find_candidates)"""
        total = getattr(self, "_cand_total", 0)
        n_paths = np.zeros(total, np.int64)
        self._ck(self.L.kprn_read_candidate_paths(self.h, _fp(n_paths), C.c_int64(total)))
        return n_paths

    def sample_eval_groups(self, group_counts, target_offsets, target_items, n_neg, seed, draw=0):
        """kprn_sample_eval_groups + kprn_read_candidates: for every held pair (user slot b, target_items[target_offsets[b] : target_offsets[b + 1]], ascending)
        up to n_neg negatives drawn from the user's rows of the engine's candidate list (group_counts as find_candidates returned them), on the device; the
        list is cut down to the rows some sample needs and replaces the engine's (include/kprn.h "sampled evaluation groups") -> dict(pairs [new_total, 2]
        the cut list, group_counts [B], target_rows [NT] (-1: unreachable), neg_rows [NT, n_neg] (rows of the cut list, ascending, -1-padded), n_drawn [NT])"""
        gc, toff, ti, B, n_neg, out = _eval_sample_args(group_counts, target_offsets, target_items, n_neg)
        total = C.c_int64(-3)
        sd, dr = _seed_draw(seed, draw)
        self._ck(self.L.kprn_sample_eval_groups(self.h, _fp(gc), B, _fp(toff), _fp(ti), n_neg, sd, dr, _fp(out["group_counts"]), C.byref(total),
                                                _fp(out["target_rows"]), _fp(out["neg_rows"]), _fp(out["n_drawn"])))
        self._cand_total = int(total.value)
        out["pairs"] = np.zeros((self._cand_total, 2), np.int32)
        self._ck(self.L.kprn_read_candidates(self.h, _fp(out["pairs"]), C.c_int64(self._cand_total)))
        return out

    def find_paths_of_candidates(self, graph, total, min_hops, max_hops, max_paths, T, walks=0, seed=0, draw=0):
        """kprn_find_paths_of_candidates: find_paths over the engine's candidate list (`total` rows, as find_candidates returned them), which never visits
        the host -> (ragged Batch of the pairs that have paths, or None; counts [total]; found [total])"""
        total = int(total)
        if total != getattr(self, "_cand_total", total):   # (the library writes counts / found [the list's total])
            raise KprnError(E_ARG, "total is not the candidate list's")
        counts, found = np.zeros(total, np.int32), np.zeros(total, np.int64)
        ptr = C.c_void_p()
        sd, dr = _seed_draw(seed, draw)
        self._ck(self.L.kprn_find_paths_of_candidates(self.h, graph.ptr, int(min_hops), int(max_hops), int(max_paths), int(T), int(walks), sd, dr, _fp(counts),
                                                      _fp(found), C.byref(ptr)))
        if not ptr:
            return None, counts, found
        return Batch._adopt(self, ptr, counts[counts > 0].copy(), T, self.cfg.F, False), counts, found

    # -- explanation (include/kprn.h "explaining a recommendation") ---------------------------
    def explain_batch(self, batch, M, class_id=1, pairs=None, out=None):
        """kprn_explain_batch: the scoring pass over `batch`, then the M strongest paths of `pairs` (0-based, repeats allowed; None = every pair) ->
        dict(path_idx / path_score / path_weight [n,M], pooled / probs [n]); `out` may supply any of the arrays"""
        if not isinstance(batch, Batch):
            batch = Batch(self, batch)
        pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1)
        n = batch.B if pr is None else int(pr.shape[0])
        res = _explain_out((n,), M, out)
        self._ck(self.L.kprn_explain_batch(self.h, batch.ptr, int(class_id), _fp(pr), n, int(M), _fp(res["path_idx"]), _fp(res["path_score"]),
                                           _fp(res["path_weight"]), _fp(res["pooled"]), _fp(res["probs"])))
        return res

    def recommend_explain_ragged(self, idx, counts, group_counts, K, M, class_id=1, mode=0, want_probs=False, out=None):
        """kprn_recommend_explain_ragged: recommend_ragged, and each group's K winners explained in the same call ->
        dict(topk_idx / topk_score [G,K], path_idx / path_score / path_weight [G,K,M], probs [B] or None)"""
        idx = np.ascontiguousarray(idx, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        gc = np.ascontiguousarray(group_counts, np.int32)
        if idx.ndim != 3 or counts.ndim != 1 or gc.ndim != 1 or K < 1:
            raise KprnError(E_ARG, "a ragged batch is idx [N,T,F] and counts [B]; group_counts [G]; K >= 1")
        B, G = int(counts.shape[0]), int(gc.shape[0])
        res = _explain_out((G, int(K)), M, out, scalars=False)
        res["topk_idx"] = np.full((G, K), -3, np.int32)
        res["topk_score"] = np.zeros((G, K), np.float32)
        res["probs"] = np.empty(B, np.float32) if want_probs else None
        self._ck(self.L.kprn_recommend_explain_ragged(self.h, _fp(idx), _fp(counts), B, C.c_int64(int(idx.shape[0])), int(idx.shape[1]),
                                                      int(idx.shape[2]), int(class_id), _fp(gc), G, int(mode), int(K), int(M), _fp(res["topk_idx"]),
                                                      _fp(res["topk_score"]), _fp(res["path_idx"]), _fp(res["path_score"]), _fp(res["path_weight"]),
                                                      _fp(res["probs"])))
        return res

    def embed(self, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        T, F = idx.shape[-2], idx.shape[-1]
        N = idx.size // (T * F)
        x = np.empty((N, T, self.D), np.float32)
        self._ck(self.L.kprn_embed(self.h, _fp(idx), C.c_int64(N), T, F, _fp(x)))
        return x

    # -- training ------------------------------------------------------------------------
    def backward(self, batch, class_id=1, bce_literal=False, inv_batch=0.0, want_loss=True):
        loss = C.c_float()
        self._ck(self.L.kprn_backward_batch(self.h, batch.ptr, int(class_id), int(bool(bce_literal)), C.c_float(inv_batch),
                                            C.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def apply_update(self, opt):
        self._ck(self.L.kprn_apply_update(self.h, C.byref(opt)))

    def train_step(self, batch, opt, class_id=1, want_loss=True):
        loss = C.c_float()
        self._ck(self.L.kprn_train_step_batch(self.h, batch.ptr, int(class_id), C.byref(opt), C.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def train_step_host(self, idx, labels, opt, class_id=1):
        idx = np.ascontiguousarray(idx, np.int32)
        labels = np.ascontiguousarray(labels, np.float32)
        B, P, T, F = idx.shape
        loss = C.c_float()
        self._ck(self.L.kprn_train_step(self.h, _fp(idx), B, P, T, F, _fp(labels), int(class_id), C.byref(opt), C.byref(loss)))
        return float(loss.value)

    def read_loss(self):
        loss = C.c_float()
        self._ck(self.L.kprn_read_loss(self.h, C.byref(loss)))
        return float(loss.value)

    def loss_sum(self, reset=True):
        """(sum of the losses, number of steps) accumulated on the device since the last reset (option loss_accumulate = 1)"""
        v, n = C.c_float(), C.c_int32()
        self._ck(self.L.kprn_read_loss_sum(self.h, C.byref(v), C.byref(n), int(bool(reset))))
        return float(v.value), int(n.value)

    def sync(self):
        self._ck(self.L.kprn_sync(self.h))

    # -- data parallel -------------------------------------------------------------------
    def dense_grad_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        self._ck(self.L.kprn_dense_grad_buffer(self.h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def sparse_grad_capacity(self):
        n = C.c_int32()
        self._ck(self.L.kprn_sparse_grad_capacity(self.h, C.byref(n)))
        return int(n.value)

    def sparse_grad_pack(self, capacity):
        """-> (device pointer of the packed buffer, its length in 32-bit words)"""
        buf, n = C.c_void_p(), C.c_int64()
        self._ck(self.L.kprn_sparse_grad_pack(self.h, int(capacity), C.byref(buf), C.byref(n)))
        return int(buf.value), int(n.value)

    def sparse_grad_merge(self, all_ptr, world, capacity):
        self._ck(self.L.kprn_sparse_grad_merge(self.h, C.c_void_p(all_ptr), int(world), int(capacity)))

    # ---- the exchange issued by the engine over RCCL (kprn_dp_*) ----
    def dp_init(self, id128, rank, world, rccl_path=None):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._ck(self.L.kprn_dp_init(self.h, rccl_path.encode() if rccl_path else None, buf, int(rank), int(world)))

    def dp_exchange_begin(self, capacity):
        self._ck(self.L.kprn_dp_exchange_begin(self.h, int(capacity)))

    def dp_exchange_finish(self, opt):
        self._ck(self.L.kprn_dp_exchange_finish(self.h, C.byref(opt)))

    def dp_comm_size(self):
        n = C.c_int32()
        self._ck(self.L.kprn_dp_comm_size(self.h, C.byref(n)))
        return n.value

    def dp_shutdown(self):
        self._ck(self.L.kprn_dp_shutdown(self.h))

    def stream(self):
        p = C.c_void_p()
        self._ck(self.L.kprn_stream(self.h, C.byref(p)))
        return p.value or 0

    # -- checkpoints / measurement ---------------------------------------------------------
    def save(self, path):
        self._ck(self.L.kprn_save(self.h, os.fsencode(path)))

    def load(self, path):
        self._ck(self.L.kprn_load(self.h, os.fsencode(path)))

    def profile(self, on=True):
        self._ck(self.L.kprn_profile_enable(self.h, int(bool(on))))

    def profile_reset(self):
        self._ck(self.L.kprn_profile_reset(self.h))

    def profile_get(self):
        n = C.c_int32()
        arr = (ProfEntry * 128)()
        self._ck(self.L.kprn_profile_get(self.h, arr, 128, C.byref(n)))
        return {arr[i].name.decode(): (arr[i].total_ms, int(arr[i].launches)) for i in range(min(n.value, 128))}

    def set_option(self, key, value):
        self._ck(self.L.kprn_set_option(self.h, key.encode(), value.encode()))
        self.options[key] = value

    def gemm16_run(self, route, A, B, C_, M, N, K, lda, ldb, ldc, a_off=0, b_off=0, c_off=0, accumulate=False, split_k=1, n_lo=0, k_lo=0, sx_min=1,
                   Np=0, Nv=0, bias=None):
        """kprn_debug_gemm16_run: ONE launch of a bf16 product (route: a key of GEMM16_ROUTES) on windows of the flat float32 arrays A, B, C_ under this
        handle's "bf16_gemm_*" options; C_ is overwritten with the whole array as the device left it.  -> {"kernel": a name of GEMM16_KERNELS, "nsplit",
        "kchunk", "dx_t_ok"}.  KprnError(E_ARG) for what the products' contracts exclude, C_ untouched"""
        for name, a in (("A", A), ("B", B), ("C", C_)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 1 and a.flags.c_contiguous and a.size >= 1):
                raise KprnError(E_ARG, "%s must be a flat C-contiguous float32 array" % name)
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            if bias.shape != (N,):
                raise KprnError(E_ARG, "bias must be [N]")
        call = Gemm16Call(GEMM16_ROUTES[route], int(bool(accumulate)), split_k, n_lo, sx_min, N, M, K, k_lo, Np, Nv,
                          A.size, a_off, lda, B.size, b_off, ldb, C_.size, c_off, ldc)
        ran = Gemm16Ran()
        self._ck(self.L.kprn_debug_gemm16_run(self.h, C.byref(call), _fp(A), _fp(B), _fp(bias), _fp(C_), C.byref(ran)))
        return {"kernel": GEMM16_KERNELS[ran.kernel], "nsplit": int(ran.nsplit), "kchunk": int(ran.kchunk), "dx_t_ok": bool(ran.dx_t_ok)}
