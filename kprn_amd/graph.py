"""From a knowledge graph to a recommendation: the arrays of kprn_graph_create built with the formatter's own id rules, and the chain
find paths -> score -> rank -> explain -> read the winning paths back, all on the device (include/kprn.h "finding a pair's paths").

The reference mines paths offline (release/data_prepare/path_find_depth_3.py: random walks over pickled dictionaries); here the finder is exhaustive
and deterministic, and its output is a ragged batch, so nothing downstream changes.

Ids: the vocab files are 0-based and the engine's ids are those + 1 (int2torch.lua:60-63), like everything the formatter prints.  The finder pads a
path on the left with the engine's pad rows (Vt, Ve, Vr: the last row of each table); `from_triples(strict=True)` refuses a vocabulary whose
#PAD_TOKEN is not the last id of its table, because the rows would then differ from the formatter's.
"""
import sys
import time

import numpy as np

from . import _ffi
from .pathformat import PathFormatter


class KnowledgeGraph:
    """src / dst / rel [E] (1-based ids), node_types [Ve, num_types] (row e - 1 = entity e), end_relation, the table sizes Ve / Vr / Vt."""

    def __init__(self, src, dst, rel, node_types, end_relation, Vr, Vt, vocabs=None, patterns=None):
        self.src, self.dst, self.rel = (np.ascontiguousarray(a, np.int32) for a in (src, dst, rel))
        self.node_types = np.ascontiguousarray(node_types, np.int32)
        self.Ve, self.num_types = (int(x) for x in self.node_types.shape)
        self.Vr, self.Vt, self.end_relation = int(Vr), int(Vt), int(end_relation)
        self.vocabs = vocabs
        self.patterns = patterns   # meta-paths (include/kprn.h "meta-paths"): the form of _ffi.Graph.set_patterns; None = every path; set it before .on(eng)
        self._names = None
        self._device = {}   # id(engine) -> _ffi.Graph

    @classmethod
    def from_triples(cls, triples, vocabs, num_types, strict=True):
        """triples: (head name, relation name, tail name), directed -- inverse edges are the caller's, as in the reference's data.  Names the vocabularies do
        not know fall back to #UNK_ENTITY / #UNK_RELATION, a node's type slots are what PathFormatter prints for a step that leaves it (sorted as strings,
        truncated, reversed, left-padded with the type table's #PAD_TOKEN; #UNK_ENTITY_TYPE where the entity has no type entry).  Entities that share an id
        (several unknown names) share the first one's type row."""
        fmt = PathFormatter(vocabs, 0, num_types)
        one = lambda v: int(v) + 1
        Ve = max(int(v) for v in vocabs.entity.values()) + 1
        Vr = max(int(v) for v in vocabs.relation.values()) + 1
        Vt = max(int(v) for v in vocabs.entity_type.values()) + 1
        pads = (one(vocabs.entity_type["#PAD_TOKEN"]), one(vocabs.entity["#PAD_TOKEN"]), one(vocabs.relation["#PAD_TOKEN"]))
        if strict and pads != (Vt, Ve, Vr):
            raise ValueError("the finder pads with the last row of each table (%d, %d, %d); this vocabulary's #PAD_TOKEN ids are %s" % (Vt, Ve, Vr, pads))
        node_types = np.full((Ve, num_types), pads[0], np.int32)
        seen = set()

        def node(name):
            feat = fmt._feature(name, "#END_RELATION").split(",")
            e = int(feat[num_types]) + 1
            if e not in seen:
                seen.add(e)
                node_types[e - 1] = [int(t) + 1 for t in feat[:num_types]]
            return e

        src, dst, rel = [], [], []
        unk_rel = one(vocabs.relation["#UNK_RELATION"])
        for head, r, tail in triples:
            src.append(node(head)); dst.append(node(tail))
            rel.append(one(vocabs.relation[r]) if r in vocabs.relation else unk_rel)
        return cls(src, dst, rel, node_types, one(vocabs.relation["#END_RELATION"]), Vr, Vt, vocabs)

    def entity_id(self, name):
        v = self.vocabs.entity
        return int(v[name] if name in v else v["#UNK_ENTITY"]) + 1

    def entity_name(self, e):
        if self._names is None:
            self._names = {int(i) + 1: n for n, i in self.vocabs.entity.items()}
        return self._names.get(int(e), str(e))

    def on(self, eng):
        """the graph in this engine's HBM (built once per engine)"""
        g = self._device.get(id(eng))
        if g is None or not g.ptr:
            g = self._device[id(eng)] = eng.graph(self.src, self.dst, self.rel, self.node_types, self.end_relation)
            g._patterns = None
        if g._patterns is not self.patterns:   # (the attribute was set or replaced since: the device graph follows)
            g.set_patterns(self.patterns)
            g._patterns = self.patterns
        return g

    def relation_id(self, relation_name):
        if self.vocabs is None or relation_name not in self.vocabs.relation:
            raise ValueError("the relation vocabulary has no %r" % (relation_name,))
        return int(self.vocabs.relation[relation_name]) + 1

    def interactions(self, relation_name):
        """the distinct (user, item) pairs joined by an edge of that relation, [n, 2] int32, sorted by (user, item): the positives to train on"""
        m = self.rel == self.relation_id(relation_name)
        pr = np.stack([self.src[m], self.dst[m]], axis=1).astype(np.int32)
        return np.unique(pr, axis=0) if len(pr) else pr.reshape(0, 2)

    def item_weights(self, items, alpha, relation_name):
        """(in-degree over that relation) ^ alpha for each of `items`, fp32 computed in double: the reference's generate_fq_dict (data_prepare/sample.py)
        without its normalisation, which the sampler's thresholds do.  alpha = 0: all ones (uniform)"""
        deg = np.bincount(self.interactions(relation_name)[:, 1], minlength=self.Ve + 1).astype(np.float64)
        return np.power(deg[np.asarray(items, np.int64)], float(alpha)).astype(np.float32)

    def holdout(self, relation_name, train_fraction=0.8, seed=1):
        """The reference's split (release/data_prepare/split_train_test.py: a global shuffle, the first int(n * fraction) positives to train) as arrays:
        pos = interactions(relation), perm = np.random.RandomState(seed).permutation(len(pos)), the first int(len * train_fraction) of pos[perm] stay in
        train.  A user all of whose pairs were held keeps them all in train instead: a user without an edge cannot be reached (cold start is out of scope).
        -> (train_kg, held [m, 2] sorted by (user, item)).  train_kg is this graph without EVERY stored edge between a held user and its held item, in
        either direction and under any relation -- the held pair is not adjacent in the graph the model trains on and is queried through; node types,
        vocabularies and table sizes are unchanged."""
        pos = self.interactions(relation_name)
        if not 0.0 <= float(train_fraction) <= 1.0:
            raise ValueError("train_fraction must be in 0..1")
        perm = np.random.RandomState(int(seed) & 0xFFFFFFFF).permutation(len(pos))
        is_held = np.zeros(len(pos), bool)
        is_held[perm[int(len(pos) * float(train_fraction)):]] = True
        kept = np.bincount(pos[~is_held, 0], minlength=self.Ve + 1)   # train pairs per user
        is_held &= kept[pos[:, 0]] > 0
        held = pos[is_held]
        code = lambda a, b: a.astype(np.int64) * (self.Ve + 1) + b.astype(np.int64)
        gone = code(held[:, 0], held[:, 1])
        keep = ~(np.isin(code(self.src, self.dst), gone) | np.isin(code(self.dst, self.src), gone))
        train = KnowledgeGraph(self.src[keep], self.dst[keep], self.rel[keep], self.node_types, self.end_relation, self.Vr, self.Vt, self.vocabs,
                               self.patterns)
        return train, held

    def apply(self, adds=None, removes=None, node_types=None):
        """A delta applied to this graph and to every device copy of it (include/kprn.h "updating a graph in place"): adds / removes are [n, 3] int32 rows of
        (src, dst, rel) entity and relation ids; the removals apply first, a removal's rel 0 names every stored edge src -> dst.  node_types (optional):
        (entities [n], rows [n, num_types]) -- the type rows of nodes that first appear in the delta (read_delta returns them).
        The host arrays src / dst / rel become the updated edge set in stored order (the host twin, kprn_host_graph_update: duplicates and self-loops are
        gone), so interactions(), item_weights() and holdout() see the new graph; every device copy made by .on(eng) is edited with one Graph.update.  A
        delta the rule refuses raises before anything changes.  `patterns` is untouched.  -> (n_added, n_removed)"""
        rowptr, col, rel, n_added, n_removed = _ffi.host_graph_update(self.src, self.dst, self.rel, self.Ve, self.Vr, adds, removes)
        if node_types is not None:
            ent = np.ascontiguousarray(node_types[0], np.int32).reshape(-1)
            rows = np.ascontiguousarray(node_types[1], np.int32).reshape(len(ent), self.num_types)
            if len(ent) and (ent.min() < 1 or ent.max() >= self.Ve or rows.min() < 1 or rows.max() > self.Vt or len(np.unique(ent)) != len(ent)):
                raise ValueError("node_types: distinct entities in 1..Ve-1 and type ids in 1..Vt")
        live = [g for g in self._device.values() if g.ptr and g.engine.h]
        for g in live:
            if node_types is not None and len(ent):
                g.set_node_types(ent, rows)
            if g.update(adds, removes) != (n_added, n_removed):
                raise RuntimeError("a device copy of the graph was out of step with the host arrays")
        if node_types is not None and len(ent):
            self.node_types[ent - 1] = rows
        self.src = np.repeat(np.arange(self.Ve, dtype=np.int32), np.diff(rowptr))
        self.dst, self.rel = col, rel
        return n_added, n_removed

    def host_find_paths(self, pairs, min_hops, max_hops, max_paths, T, F=None, threads=1, want_idx=True, walks=0, seed=0, draw=0, cap="first"):
        """walks > 0: the hops past 3 sampled (_ffi.host_find_paths_sampled); cap = "spread": the cap keeps a spread of a pair's paths under (seed, draw)
        (_ffi.host_find_paths_cap); with `patterns` set, only the matching paths (_ffi.host_find_paths_patterns)"""
        if self.patterns:
            return _ffi.host_find_paths_patterns(self.src, self.dst, self.rel, self.node_types, self.Vr, self.Vt, self.end_relation, pairs, min_hops, max_hops,
                                                 max_paths, T, walks, seed, draw, cap=cap, patterns=self.patterns, F=F, threads=threads, want_idx=want_idx)
        if cap != "first":
            return _ffi.host_find_paths_cap(self.src, self.dst, self.rel, self.node_types, self.Vr, self.Vt, self.end_relation, pairs, min_hops, max_hops,
                                            max_paths, T, walks, seed, draw, cap=cap, F=F, threads=threads, want_idx=want_idx)
        if int(walks) != 0:
            return _ffi.host_find_paths_sampled(self.src, self.dst, self.rel, self.node_types, self.Vr, self.Vt, self.end_relation, pairs, min_hops, max_hops,
                                                max_paths, T, walks, seed, draw, F=F, threads=threads, want_idx=want_idx)
        return _ffi.host_find_paths(self.src, self.dst, self.rel, self.node_types, self.Vr, self.Vt, self.end_relation, pairs, min_hops, max_hops, max_paths,
                                    T, F=F, threads=threads, want_idx=want_idx)


def parse_meta_paths(lines, kg):
    """The text form of a pattern set (include/kprn.h "meta-paths") -> the list KnowledgeGraph.patterns takes.  One pattern per line; positions separated by
    whitespace; a position is `*` (any relation) or relation names joined by `|`, as spelt in kg's relation vocabulary; `#` starts a comment, blank lines are
    skipped.  An unknown relation name, a line of more than 5 positions or more than 32 patterns raises ValueError naming the line."""
    patterns = []
    for no, line in enumerate(lines, 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue
        if len(words) > _ffi.PATTERN_MAX_HOPS:
            raise ValueError("meta-paths line %d: %d positions, at most %d" % (no, len(words), _ffi.PATTERN_MAX_HOPS))
        if len(patterns) == _ffi.PATTERN_MAX:
            raise ValueError("meta-paths line %d: more than %d patterns" % (no, _ffi.PATTERN_MAX))
        pat = []
        for w in words:
            if w == "*":
                pat.append(None)
                continue
            try:
                pat.append(sorted({kg.relation_id(name) for name in w.split("|")}))
            except ValueError as e:
                raise ValueError("meta-paths line %d: %s" % (no, e)) from None
        patterns.append(pat)
    return patterns


def format_meta_paths(patterns, kg):
    """parse_meta_paths backwards: the lines of a pattern set"""
    names = {int(i) + 1: n for n, i in kg.vocabs.relation.items()}
    return [" ".join("*" if not pos else "|".join(names[int(r)] for r in pos) for pos in pat) for pat in patterns]


def read_triples(path):
    """a TSV of `head \\t relation \\t tail` names, one directed edge per line"""
    with open(path) as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            if len(parts) >= 3:
                yield parts[0], parts[1], parts[2]


def read_delta(path, kg):
    """A delta file for KnowledgeGraph.apply: one change per line, `+\thead\trelation\ttail` adds an edge and `-\thead\trelation\ttail` removes one;
    relation `*` on a `-` line stands for every relation between the two; blank lines and lines that start with `#` are skipped.  Names are resolved as
    from_triples resolves them (unknown ones fall back to #UNK_ENTITY / #UNK_RELATION); a head or tail of a `+` line that kg has not seen -- its type row
    is still the pad row -- gets the row PathFormatter prints for it.  A malformed line, or `*` on a `+` line, raises ValueError naming the line number.
    -> (adds [n, 3], removes [m, 3], (entities [k], rows [k, num_types])): the arguments of KnowledgeGraph.apply"""
    vocabs = kg.vocabs
    fmt = PathFormatter(vocabs, 0, kg.num_types)
    unk_rel = int(vocabs.relation["#UNK_RELATION"]) + 1
    adds, removes, new = [], [], {}

    def node(name, added):
        feat = fmt._feature(name, "#END_RELATION").split(",")
        e = int(feat[kg.num_types]) + 1
        if added and e not in new and 1 <= e < kg.Ve and (kg.node_types[e - 1] == kg.Vt).all():
            new[e] = [int(t) + 1 for t in feat[:kg.num_types]]
        return e

    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            parts = line.split("\t")
            if len(parts) != 4 or parts[0] not in ("+", "-") or not all(parts[1:]):
                raise ValueError("delta line %d: expected `+|-<TAB>head<TAB>relation<TAB>tail`" % no)
            sign, head, r, tail = parts
            if r == "*":
                if sign == "+":
                    raise ValueError("delta line %d: `*` stands for every relation on a `-` line only" % no)
                rid = 0
            else:
                rid = int(vocabs.relation[r]) + 1 if r in vocabs.relation else unk_rel
            (adds if sign == "+" else removes).append((node(head, sign == "+"), node(tail, sign == "+"), rid))
    ent = np.array(sorted(new), np.int32)
    rows = np.array([new[e] for e in sorted(new)], np.int32).reshape(len(ent), kg.num_types)
    return np.array(adds, np.int32).reshape(-1, 3), np.array(removes, np.int32).reshape(-1, 3), (ent, rows)


class path_cap:
    """`with path_cap(eng, cap):` the engine's option "path_cap" is `cap` ("first" | "spread") inside and what it was afterwards; cap=None changes nothing"""

    def __init__(self, eng, cap):
        self.eng, self.cap = eng, cap

    def __enter__(self):
        self.before = self.eng.options.get("path_cap", "first")
        if self.cap is not None:
            self.eng.set_option("path_cap", self.cap)

    def __exit__(self, *exc):
        if self.cap is not None:
            self.eng.set_option("path_cap", self.before)


def recommend(eng, kg, user, items, K, M, min_hops=1, max_hops=3, max_paths=28, T=None, class_id=1, mode=_ffi.RANK_PRINTED, walks=0, seed=1, draw=0, sampler=None,
              exclude_adjacent=True, max_candidates=0, cap=None):
    """Which of `items` for `user` (entity ids), and why: find every pair's paths on the device, score the batch, put the scores on the board, rank the
    one group, explain the K winners and read their paths' ids back.  kg: a KnowledgeGraph, or an _ffi.Graph already on the engine.  The board is
    resized to the candidates that have paths (kprn_board_reserve keeps nothing).  walks > 0: max_hops may be 4 or 5, the hops past 3 sampled by `walks`
    walks per item and hop count under (seed, draw) (include/kprn.h "sampled paths of four and five hops").
    -> the K best items, best first: dict(item, rank, score, n_paths, found, paths = the M strongest as (ids [T,F], weight, score)); items without any
    path are not candidates, so the list may be shorter than K -- empty when no item is reachable.
    items=None: the candidates are found on the device among the items of `sampler` (an _ffi.Sampler: the catalogue), recommend_users for the one user;
    max_candidates as there (it has no meaning beside a list of items).
    cap = "first" | "spread": the engine's option "path_cap" for this call (None: as the engine stands) -- "spread" keeps one path in each of max_paths strata
    of a pair's sequence under (seed, draw) instead of its first max_paths; the same (seed, draw) gives the same answer every time."""
    if cap is not None:
        with path_cap(eng, cap):
            return recommend(eng, kg, user, items, K, M, min_hops, max_hops, max_paths, T, class_id, mode, walks, seed, draw, sampler, exclude_adjacent,
                             max_candidates)
    if items is None:
        if sampler is None:
            raise ValueError("recommend needs items, or a sampler whose item list is the catalogue")
        return recommend_users(eng, kg, sampler, [user], K, M, min_hops, max_hops, max_paths, T, class_id, mode, walks, seed, draw, exclude_adjacent,
                               max_candidates)[0]
    if max_candidates:
        raise ValueError("max_candidates caps the candidates found on the device: it cannot be combined with items")
    graph = kg.on(eng) if isinstance(kg, KnowledgeGraph) else kg
    items = np.asarray(items, np.int32).reshape(-1)
    pairs = np.stack([np.full(items.shape, int(user), np.int32), items], axis=1)
    T = max_hops + 1 if T is None else int(T)
    batch, counts, found = eng.find_paths(graph, pairs, min_hops, max_hops, max_paths, T, walks=walks, seed=seed, draw=draw)
    if batch is None:
        return []
    try:
        cand = np.nonzero(counts)[0]            # pair b of the batch is items[cand[b]]
        eng.forward_async(batch, class_id)      # the scoring pass; its probabilities stay on the device
        eng.board_reserve(batch.B)
        eng.board_put(0, batch.B)
        kk = min(int(K), _ffi.RANK_MAX_K)
        top = eng.rank_groups(np.array([0, batch.B], np.int64), K=kk, mode=mode)
        win = top["topk_idx"][0]
        win = win[win >= 0]
        ex = eng.explain_batch(batch, M, class_id, pairs=win)
        idx = batch.read_idx()
        off = np.concatenate([[0], np.cumsum(batch.counts, dtype=np.int64)])
        out = []
        for place, b in enumerate(win):
            paths = [(idx[off[b] + q], float(ex["path_weight"][place, r]), float(ex["path_score"][place, r]))
                     for r, q in enumerate(ex["path_idx"][place]) if q >= 0]
            out.append(dict(item=int(items[cand[b]]), rank=place, score=float(top["topk_score"][0, place]), n_paths=int(batch.counts[b]),
                            found=int(found[cand[b]]), paths=paths))
        return out
    finally:
        batch.free()


def _rank_key(scores, mode):
    """the ranking stage's key (include/kprn.h "ranking"): what "%.5f" prints, times 1e5, in mode PRINTED; the fp32 value in mode RAW; an invalid member
    sorts below every valid one"""
    s = np.asarray(scores, np.float32)
    if mode == _ffi.RANK_PRINTED:
        valid = (s >= 0) & (s <= 1)
        return np.where(valid, np.rint(np.where(valid, s, 0).astype(np.float64) * 1e5), -np.inf)
    return np.where(np.isnan(s), -np.inf, s.astype(np.float64))


def _score_candidates(eng, graph, sampler, users, min_hops, max_hops, max_paths, T, class_id, walks, seed, draw, exclude_adjacent, max_candidates, cut=None):
    """The front half of recommend_users and evaluate_from_graph, up to the board put: the users' candidates found on the device (capped at max_candidates by
    path count when that is > 0), the finder reading that list where it lies, the batch scored, its probabilities put on a board of exactly batch.B lines.
    cut(pairs, group_counts) -> (pairs, group_counts): a stage that replaces the engine's candidate list before the finder reads it (sampled evaluation).
    -> None when no user has a candidate with a path, else (batch, pairs, cand, uoff, found): pair b of the batch is row cand[b] of the candidate list
    `pairs` [n, 2] = (user, item), user g's surviving pairs are the batch's pairs uoff[g] .. uoff[g + 1] = those board lines.  The caller frees the batch."""
    T = max_hops + 1 if T is None else int(T)
    pairs, gc = eng.find_candidates(graph, sampler, users, min_hops, min(int(max_hops), _ffi.FIND_MAX_HOPS), exclude_adjacent, cap=max_candidates)
    if len(pairs) == 0:
        return None
    if cut is not None:
        pairs, gc = cut(pairs, gc)
        if len(pairs) == 0:
            return None
    batch, counts, found = eng.find_paths_of_candidates(graph, len(pairs), min_hops, max_hops, max_paths, T, walks=walks, seed=seed, draw=draw)
    if batch is None:
        return None
    try:
        cand = np.nonzero(counts)[0]
        ends = np.cumsum(gc, dtype=np.int64)
        uoff = np.searchsorted(cand, np.concatenate([[0], ends]))
        eng.forward_async(batch, class_id)
        eng.board_reserve(batch.B)
        eng.board_put(0, batch.B)
    except BaseException:
        batch.free()
        raise
    return batch, pairs, cand, uoff, found


def recommend_users(eng, kg, sampler, users, K, M=0, min_hops=1, max_hops=3, max_paths=28, T=None, class_id=1, mode=_ffi.RANK_PRINTED, walks=0, seed=1, draw=0,
                    exclude_adjacent=True, max_candidates=0):
    """What should each of `users` (entity ids) get, and why, without a candidate list: one chain for all of them.  The candidates -- the items of
    `sampler` (an _ffi.Sampler: the catalogue) that min_hops .. min(max_hops, 3) hops reach from the user, less the user and, with exclude_adjacent, the
    items it already has an edge to -- are found on the device (include/kprn.h "candidates of a user"), the finder reads that list where it lies, the
    batch is scored and put on the board, one rank_groups call ranks every user's group, the winners are explained (M > 0) and their paths read back.
    A group of more than 4096 surviving pairs (kprn_rank_groups' limit) is ranked as consecutive sub-groups of at most 4096 in the same call, whose
    top-K rows are merged here by (key descending, index within the user's group ascending): what a single group would have given.
    max_candidates = N > 0: only each user's N strongest candidates by path count enter the chain (include/kprn.h "the N strongest candidates of a user"),
    the users taken in chunks of fewer than 2^28 / M (the catalogue's size) -- a user's result is that of one call; 0: every candidate.
    -> per user, the list of dicts `recommend` returns."""
    graph = kg.on(eng) if isinstance(kg, KnowledgeGraph) else kg
    users = np.asarray(users, np.int32).reshape(-1)
    max_candidates = int(max_candidates)
    if max_candidates < 0:
        raise ValueError("max_candidates must be >= 0")
    chunk = (_ffi.CAND_TOP_MAX_BM - 1) // max(int(sampler.M), 1)   # the most users of one kprn_find_candidates_top call
    if max_candidates > 0 and 0 < chunk < len(users):
        out = []
        for lo in range(0, len(users), chunk):
            out += recommend_users(eng, graph, sampler, users[lo:lo + chunk], K, M, min_hops, max_hops, max_paths, T, class_id, mode, walks, seed, draw,
                                   exclude_adjacent, max_candidates)
        return out
    out = [[] for _ in users]
    scored = _score_candidates(eng, graph, sampler, users, min_hops, max_hops, max_paths, T, class_id, walks, seed, draw, exclude_adjacent, max_candidates)
    if scored is None:
        return out
    batch, pairs, cand, uoff, found = scored
    try:
        kk = min(int(K), _ffi.RANK_MAX_K)
        goff, owner = [0], []                   # the sub-groups of at most RANK_MAX_GROUP members, and the user each belongs to
        for g in range(len(users)):
            for lo in range(int(uoff[g]), int(uoff[g + 1]), _ffi.RANK_MAX_GROUP):
                goff.append(min(lo + _ffi.RANK_MAX_GROUP, int(uoff[g + 1])))
                owner.append(g)
        owner = np.array(owner)
        top = eng.rank_groups(np.array(goff, np.int64), pos=np.full(len(owner), -1, np.int32), K=kk, mode=mode)
        wins, scores = [], []                   # per user with candidates: the winners as pairs of the batch, best first
        for g in range(len(users)):
            rows = np.nonzero(owner == g)[0]
            if len(rows) == 0:
                wins.append(np.zeros(0, np.int64)); scores.append(np.zeros(0, np.float32))
                continue
            ti, ts = top["topk_idx"][rows], top["topk_score"][rows]
            b = (ti.astype(np.int64) + np.array(goff, np.int64)[rows][:, None])[ti >= 0]
            sc = ts[ti >= 0]
            if len(rows) > 1:
                order = np.lexsort((b, -_rank_key(sc, mode)))[:kk]
                b, sc = b[order], sc[order]
            wins.append(b); scores.append(sc)
        win = np.concatenate(wins).astype(np.int32)
        ex = eng.explain_batch(batch, M, class_id, pairs=win) if int(M) > 0 and len(win) else None
        idx = batch.read_idx()
        off = np.concatenate([[0], np.cumsum(batch.counts, dtype=np.int64)])
        at = 0
        for g in range(len(users)):
            for place, (b, sc) in enumerate(zip(wins[g], scores[g])):
                paths = [] if ex is None else [(idx[off[b] + q], float(ex["path_weight"][at, r]), float(ex["path_score"][at, r]))
                                               for r, q in enumerate(ex["path_idx"][at]) if q >= 0]
                out[g].append(dict(item=int(pairs[cand[b], 1]), rank=place, score=float(sc), n_paths=int(batch.counts[b]), found=int(found[cand[b]]),
                                   paths=paths))
                at += 1
        return out
    finally:
        batch.free()


PLACE_UNREACHABLE = -3   # evaluate_from_graph's place of a held pair that never reached the ranking stage


def _rank_sampled(eng, graph, sampler, users, items, ends, n_neg, chain, mode, hist_len, places, hist):
    """One chunk of evaluate_from_graph under eval_negatives = n_neg: user g's held items are items[ends[g - 1] : ends[g]] (ascending), `chain` the arguments
    of _score_candidates behind the users.  The candidates, one sample_eval_groups call (seed = chain[6], draw 0) that cuts the list down to the rows some
    sample needs, the finder on that list, the pass, the board put, one rank_groups call with a members table: every reachable held pair is the group
    [target, its negatives ascending], pos 0.  Writes the ranks into places (a view: one entry per held item) and adds the histogram to hist
    -> the ranked samples with fewer than n_neg negatives"""
    hoff = np.concatenate([[0], ends]).astype(np.int64)
    drawn = {}

    def cut(pairs, gc):
        drawn.update(eng.sample_eval_groups(gc, hoff, items, n_neg, chain[6], 0))
        return drawn["pairs"], drawn["group_counts"]
    scored = _score_candidates(eng, graph, sampler, users, *chain, cut=cut)
    if scored is None:
        return 0
    batch, pairs, cand, _uoff, _found = scored
    try:
        line = np.full(len(pairs), -1, np.int64)            # the board line of every list row; -1: the finder dropped the pair
        line[cand] = np.arange(len(cand))
        trow, nd = drawn["target_rows"], drawn["n_drawn"]
        members, goff, rows, n_short = [], [0], [], 0
        for k in np.nonzero(trow >= 0)[0]:
            if line[trow[k]] < 0:
                continue                                    # a dropped target is unreachable
            neg = line[drawn["neg_rows"][k, :nd[k]]]
            neg = neg[neg >= 0]                             # a negative whose pair the finder dropped leaves its group
            members += [line[trow[k]:trow[k] + 1], neg]
            goff.append(goff[-1] + 1 + len(neg)); rows.append(k)
            n_short += len(neg) < n_neg
        if not rows:
            return 0
        res = eng.rank_groups(np.array(goff, np.int64), members=np.concatenate(members), pos=np.zeros(len(rows), np.int32), mode=mode, hist_len=hist_len)
        places[np.array(rows)] = res["ranks"]
        hist += res["hist"]
        return int(n_short)
    finally:
        batch.free()


def evaluate_from_graph(eng, train_kg, held, sampler, users_per_call=64, min_hops=1, max_hops=3, max_paths=28, T=None, class_id=1, mode=_ffi.RANK_PRINTED, walks=0,
                        seed=1, max_candidates=0, ks=range(1, 16), max_users=0, eval_negatives=0):
    """Held-out evaluation against everything a user reaches (KnowledgeGraph.holdout made train_kg and held): for the held pairs' distinct users,
    users_per_call at a time (max_users > 0: the first that many users only), the chain of recommend_users up to the board put on the TRAIN graph with
    exclude_adjacent -- so a user's train items are no candidates and its held items are -- and then ONE rank_targets call: the groups are the users'
    surviving pairs, the targets the held items among them, each placed among the user's non-held candidates (include/kprn.h "ranking targets in groups
    of any size").  A held pair that is not there -- its item outside the sampler's catalogue, not reached, cut by max_candidates, or left without a
    kept path -- is a miss for every k: it is counted in hist[hist_len] and reported as n_unreachable.
    eval_negatives = N > 0: the reference's protocol instead (data_prepare/sample.py, eval/eval_score.py): every held pair is ranked against at most N
    negatives drawn from its user's candidates that are no held items of that user (include/kprn.h "sampled evaluation groups").  After the candidates
    (cap included) ONE sample_eval_groups call per chunk with the users' held items, `seed` and draw 0 -- every epoch ranks the same samples -- cuts the
    list down to the rows some sample needs; only those are given paths and scored; ONE rank_groups call with a members table then ranks every reachable
    held pair as the group [target, its negatives ascending] with pos 0.  A negative whose pair the finder dropped leaves its group; a dropped target is
    unreachable.  The held pairs must be distinct.
    -> dict(hits, ndcgs, n (evalrank.metrics_from_hist over the summed histogram), n_unreachable, n_zero, places [m] int32 in the order of `held` (the
    evaluated rows: place, _ffi.RANK_ZERO_GROUP or PLACE_UNREACHABLE), held [m, 2], hist); with eval_negatives > 0 also n_short = the ranked samples
    with fewer than N negatives."""
    from . import evalrank
    eval_negatives = int(eval_negatives)
    if eval_negatives < 0 or eval_negatives > _ffi.EVAL_MAX_NEG:
        raise ValueError("eval_negatives must be in 0..%d" % _ffi.EVAL_MAX_NEG)
    graph = train_kg.on(eng) if isinstance(train_kg, KnowledgeGraph) else train_kg
    held = np.ascontiguousarray(held, np.int32).reshape(-1, 2)
    held = held[np.lexsort((held[:, 1], held[:, 0]))]
    users = np.unique(held[:, 0])
    if int(max_users) > 0:
        users = users[:int(max_users)]
        held = held[np.isin(held[:, 0], users)]
    ks = list(ks)
    hist_len = max(ks) if ks else 1
    per = max(int(users_per_call), 1)
    if int(max_candidates) > 0:
        per = max(min(per, (_ffi.CAND_TOP_MAX_BM - 1) // max(int(sampler.M), 1)), 1)
    first = np.searchsorted(held[:, 0], users)             # user u's held rows = held[first[u] : last[u]]
    last = np.searchsorted(held[:, 0], users, side="right")
    places = np.full(len(held), PLACE_UNREACHABLE, np.int32)
    hist = np.zeros(hist_len + 4, np.int64)
    n_short = 0
    for lo in range(0, len(users), per):
        us = users[lo:lo + per]
        if eval_negatives > 0:                              # (the chunk's held rows are consecutive: held[first[lo] : last[lo + len(us) - 1]], user by user)
            n_short += _rank_sampled(eng, graph, sampler, us, held[first[lo]:last[lo + len(us) - 1], 1], last[lo:lo + len(us)] - first[lo], eval_negatives,
                                     (min_hops, max_hops, max_paths, T, class_id, walks, seed, 0, True, int(max_candidates)), mode, hist_len,
                                     places[first[lo]:last[lo + len(us) - 1]], hist)
            continue
        scored = _score_candidates(eng, graph, sampler, us, min_hops, max_hops, max_paths, T, class_id, walks, seed, 0, True, int(max_candidates))
        if scored is None:
            continue
        batch, pairs, cand, uoff, _found = scored
        try:
            items = pairs[cand, 1]                          # the item of every board line
            goff, toff, targets, rows = [int(uoff[0])], [0], [], []
            for g in range(len(us)):
                a, b = int(uoff[g]), int(uoff[g + 1])
                if a == b:
                    continue                                # nothing of this user survived: every held pair of it is unreachable
                mine = held[first[lo + g]:last[lo + g], 1]
                at = np.nonzero(np.isin(items[a:b], mine))[0]                  # ascending within the group
                targets.append(at.astype(np.int32))
                rows.append(first[lo + g] + np.searchsorted(mine, items[a:b][at]))   # the held row of each target
                goff.append(b); toff.append(toff[-1] + len(at))
            if toff[-1] == 0:
                continue
            res = eng.rank_targets(np.array(goff, np.int64), np.array(toff, np.int64), np.concatenate(targets), mode=mode, hist_len=hist_len)
            places[np.concatenate(rows)] = res["places"]
            hist += res["hist"]
        finally:
            batch.free()
    n_unreachable = int((places == PLACE_UNREACHABLE).sum())
    hist[hist_len] += n_unreachable
    hits, ndcgs, n = evalrank.metrics_from_hist(hist, hist_len, ks)
    out = dict(hits=hits, ndcgs=ndcgs, n=n, n_unreachable=n_unreachable, n_zero=int(hist[hist_len + 1]), places=places, held=held, hist=hist)
    if eval_negatives > 0:
        out["n_short"] = int(n_short)
    return out


def groups_from_counts(counts, n_neg):
    """The group table of a minibatch that find_training_paths made: rows g (1 + n_neg) .. of its pair list are group g (one positive, then that user's
    negatives), a row with counts == 0 was dropped from the batch, so group g owns the sum(counts[rows] > 0) consecutive pairs that are left -- none, when
    all of its rows were dropped.  -> group_offsets [G + 1] int32 for Batch.set_groups"""
    per = 1 + max(int(n_neg), 0)
    kept = (np.asarray(counts).reshape(-1) > 0)
    if kept.shape[0] % per != 0:
        raise ValueError("counts holds %d rows, not a multiple of 1 + n_neg = %d" % (kept.shape[0], per))
    sizes = kept.reshape(-1, per).sum(axis=1)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _keep_hardest(eng, pool_batch, counts, pool, n_keep, class_id):
    """One step's selection (train_from_graph, neg_pool): the pool batch that find_training_paths(n_neg=pool) made is scored, its probabilities put on the
    board from line 0, every group's positive and n_keep highest-scoring negatives kept, and the kept pairs' rows taken from the pool batch, which is freed.
    -> (the kept pairs' batch or None, its group table [G + 1] int32 over ALL the step's groups, the pool batch's pair count)"""
    try:
        eng.forward_async(pool_batch, class_id)
        eng.board_put(0, pool_batch.B)
        goff = groups_from_counts(counts, pool).astype(np.int64)
        has_pos = np.asarray(counts).reshape(-1, 1 + pool)[:, 0] > 0
        full = np.diff(goff) > 0                         # (kprn_select_hardest takes no empty group: those are left out of the call)
        sel_off = np.concatenate([[0], np.cumsum(np.diff(goff)[full])]).astype(np.int64)
        keep, _ = eng.select_hardest(sel_off, n_keep, pos=np.where(has_pos[full], 0, -1).astype(np.int32))
        keep = keep[:pool_batch.B]
        sub = eng.batch_subset(pool_batch, keep)
        upto = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        return sub, upto[goff].astype(np.int32), pool_batch.B
    finally:
        pool_batch.free()


def train_from_graph(eng, kg, positives, opt, minibatch, n_neg, num_epochs, seed, sampler=None, max_attempts=16, min_hops=2, max_hops=3, max_paths=28, T=None,
                     class_id=1, epoch_hooks=(), start_iteration=1, gradient_step_counter=100, out=None, stats=None, walks=0, loss="bce", cap=None, neg_pool=0):
    """Training from a knowledge graph alone: every step samples its negatives, finds the paths and trains, all on the device.
    positives [n, 2] = (user, item) entity ids (KnowledgeGraph.interactions); sampler: an _ffi.Sampler (None: the positives' distinct items, uniform).
    Each epoch e shuffles the positives with np.random.RandomState(seed + e) and walks them `minibatch` at a time; a step is
    Engine.find_training_paths (seed, draw = the global step number) -> train_step -> free.  A minibatch in which no pair has a path is skipped and counted.
    loss = "bpr": the pairwise loss over each positive's group (include/kprn.h "pairwise loss") instead of BCE on each pair: the engine's option "loss" is set
    for the run and put back afterwards, every step sets the batch's group table (groups_from_counts), and a minibatch without a term -- no group kept both
    its positive and a negative -- is skipped and counted as well.
    walks > 0: max_hops may be 4 or 5, the hops past 3 sampled by `walks` walks per pair and hop count under the same seed and draw.
    cap = "first" | "spread": the engine's option "path_cap" for the run, put back afterwards (None: as the engine stands).  Under "spread" the draw -- the
    global step -- addresses the cap's draws too, so every epoch trains on another subset of a busy pair's paths.
    neg_pool = P > n_neg (at most 256): hard negatives (include/kprn.h "hard negatives").  A step draws P negatives per positive instead of n_neg, scores that
    pool batch with the current model (forward_async -> board_put, on a board of minibatch * (1 + P) lines reserved once per run: the engine's previous board
    is gone), keeps each group's positive and its n_neg highest-scoring negatives (Engine.select_hardest; pos = -1 where the positive's row kept no path),
    and trains on Engine.batch_subset of the pool batch -- the rows that were scored, not the rows a second find call would draw.  Under bpr the group table
    comes from the kept sizes.  The skip rules are unchanged.  0 or n_neg: today's step, not one call differs.
    Losses are summed on the device (option "loss_accumulate"); the epoch lines and hooks (OptimizerCallback) are MyOptimizer's.
    -> the epochs' average losses; stats (a dict, optional) receives steps / skipped / pairs, and with a pool pool_pairs / kept_pairs (the pairs scored and
    the pairs kept, summed over the steps that made a selection)."""
    out = sys.stdout if out is None else out
    graph = kg.on(eng) if isinstance(kg, KnowledgeGraph) else kg
    pos = np.ascontiguousarray(positives, np.int32).reshape(-1, 2)
    if len(pos) == 0:
        raise ValueError("no positives to train on")
    own = sampler is None
    if own:
        sampler = eng.sampler(np.unique(pos[:, 1]))
    T = max_hops + 1 if T is None else int(T)
    st = dict(steps=0, skipped=0, pairs=0)
    history = []
    for hook in epoch_hooks:
        if hook.epochHookFreq == 1:
            hook.hook(0)
    if loss not in ("bce", "bpr"):
        raise ValueError("loss must be bce or bpr")
    if cap not in (None,) + tuple(_ffi.PATH_CAPS):
        raise ValueError("cap must be first or spread")
    pool = int(neg_pool)
    if pool != 0 and not int(n_neg) <= pool <= _ffi.SELECT_MAX_KEEP:
        raise ValueError("neg_pool must be 0 or in n_neg .. %d" % _ffi.SELECT_MAX_KEEP)
    hard = pool > int(n_neg)
    if hard:
        st.update(pool_pairs=0, kept_pairs=0)
    board_ready = False
    loss_before, cap_before = eng.options.get("loss", "bce"), eng.options.get("path_cap", "first")
    eng.set_option("loss_accumulate", "1")
    eng.loss_sum(reset=True)
    try:
        eng.set_option("loss", loss)
        if cap is not None:
            eng.set_option("path_cap", cap)
        draw = 0
        prev = time.time()
        for i in range(int(start_iteration), int(num_epochs) + 1):
            order = np.random.RandomState((int(seed) + i) & 0xFFFFFFFF).permutation(len(pos))
            total, batches, processed, since = 0.0, 0, 0, 0
            for k in range(0, len(pos), int(minibatch)):
                mb = pos[order[k:k + int(minibatch)]]
                batch, _, counts, _ = eng.find_training_paths(graph, sampler, mb, pool if hard else n_neg, seed, draw, min_hops, max_hops, max_paths, T,
                                                              max_attempts=max_attempts, walks=walks)
                draw += 1
                if batch is None:
                    st["skipped"] += 1
                    continue
                groups = None
                if hard:
                    if not board_ready:
                        eng.board_reserve(int(minibatch) * (1 + pool))
                        board_ready = True
                    batch, groups, n_pool = _keep_hardest(eng, batch, counts, pool, n_neg, class_id)   # (frees the pool batch)
                    if batch is None:
                        st["skipped"] += 1
                        continue
                    st["pool_pairs"] += n_pool
                    st["kept_pairs"] += batch.B
                try:
                    if loss == "bpr" and batch.set_groups(groups_from_counts(counts, n_neg) if groups is None else groups) == 0:
                        st["skipped"] += 1
                        continue
                    eng.train_step(batch, opt, class_id, want_loss=False)
                finally:
                    batch.free()
                batches += 1
                since += 1
                processed += len(mb)
                st["steps"] += 1
                st["pairs"] += batch.B
                if since % int(gradient_step_counter) == 0:
                    total += eng.loss_sum(reset=True)[0]
                    print("Printing after %d gradient steps\navg loss in epoch = %f\n" % (gradient_step_counter, total / since), file=out)
            total += eng.loss_sum(reset=True)[0]
            avg = total / max(batches, 1)
            now = time.time()
            elapsed, prev = now - prev, now
            print("\nIter: %d\navg loss in epoch = %f\ntotal elapsed = %f\ntime per batch = %f" % (i, avg, elapsed, elapsed / max(batches, 1)), file=out)
            print("examples/sec = %f" % (processed / max(elapsed, 1e-9)), file=out)
            history.append(avg)
            for hook in epoch_hooks:
                if i % hook.epochHookFreq == 0:
                    hook.hook(i)
    finally:
        eng.set_option("loss_accumulate", "0")
        eng.set_option("loss", loss_before)
        if cap is not None:
            eng.set_option("path_cap", cap_before)
        if own:
            sampler.free()
    if stats is not None:
        stats.update(st)
    return history
