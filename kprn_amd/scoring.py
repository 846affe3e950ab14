"""Scoring entry point: release/songPathRnn/eval/test_from_checkpoint.lua.

Loads a checkpoint, runs model:forward on every batch of the test list (minibatch 512, no
shuffle, :47-49,57) and writes `counter \\t %.5f score \\t label` with a global 0-based counter
(:110-118).  Line order = list order x in-file row order: the downstream join is positional
(eval/combine_result.py:24-27).
"""
import time

from .batcher import BatcherFileList


def lua_number(x):
    """how Lua 5.1 concatenates a number into a string: "%.14g" (labels print as 1 / 0)."""
    return "%.14g" % float(x)


ENGINE_BATCH_PATHS = 65536   # paths per engine call: the script's minibatch (512 pairs) is a memory knob of the Torch7 graph, not
                             # part of the result -- pairs are scored independently, so the engine takes them in chip-sized groups
FEED_AHEAD = 2


def _next_group(engine, batcher, merge):
    """-> (labels, pairs, feed(slot) -> slot, batch() -> Batch) of the next group, or None"""
    if merge:
        got = batcher.getMergedGroup(ENGINE_BATCH_PATHS)
        if got is None:
            return None
        labs, idx, counts, count, _classId = got
        return labs, count, (lambda slot: engine.feed_ragged(idx, counts, None, slot=slot)), (lambda: engine.batch_ragged(idx, counts))
    got = batcher.getBatch()
    if got is None:
        return None
    labs, inputs, count, _classId = got
    return labs, count, (lambda slot: engine.feed(inputs, None, slot=slot)), (lambda: engine.batch(inputs))


def score_batches(engine, batcher, class_id=1, merge=False):
    """merge=True (an extension, default off): consecutive rows of consecutive bucket files are packed into ragged groups of up to
    ENGINE_BATCH_PATHS paths (BatcherFileList.getMergedGroup), so that a small bucket does not cost an engine call of its own; the pairs
    come back in the same order.

    -> (labels [n], probabilities [n]) per group of pairs, in list x in-file order.  With the HIP engine every group is a
    label-less feed slot (upload + identical-prefix plan built by the host threads under the previous group's kernels), scored
    asynchronously; the probabilities of group i come back while group i + 1 runs, so the caller's formatting overlaps too."""
    streaming = hasattr(engine, "feed") and hasattr(engine, "forward_async")
    saved = [(b, b.batchSize) for b in getattr(batcher, "batchers", [])]
    try:
        if streaming:
            for b, _ in saved:       # chip-sized groups per bucket file (the caller's batch sizes are put back when the generator ends)
                b.batchSize = max(b.batchSize, ENGINE_BATCH_PATHS // max(1, b.numPaths))
        yield from _score_batches(engine, batcher, class_id, streaming, merge)
    finally:
        for b, size in saved:
            b.batchSize = size


def _score_batches(engine, batcher, class_id, streaming, merge=False):
    if not streaming:
        while True:
            got = _next_group(engine, batcher, merge)
            if got is None:
                return
            labs, count, _feed, make = got
            yield labs, engine.forward(make(), class_id)["probs"]  # nn.Select(2,1) is fixed in the script (:82)
    slots = [None] * (FEED_AHEAD + 2)
    k = 0
    fed = []           # (slot, labels, count): fed, not yet scored
    running = None     # (labels, count): scored asynchronously, probabilities not yet read
    done = False
    while True:
        while not done and len(fed) < FEED_AHEAD:
            got = _next_group(engine, batcher, merge)
            if got is None:
                done = True
                break
            labs, count, feed, _make = got
            slots[k] = feed(slots[k])
            fed.append((slots[k], labs, count))
            k = (k + 1) % len(slots)
        out = None
        if running is not None:
            out = (running[0], engine.read_probs(running[1]))
        running = None
        if fed:
            slot, labs, count = fed.pop(0)
            engine.forward_async(slot, class_id)
            running = (labs, count)
        if out is not None:
            yield out
        if running is None and not fed and done:
            return


def rank_test_set(engine, batcher, members, group_offsets, mode=0, K=0, merge=False, class_id=1, pos=None, hist_len=15, on_scores=None):
    """Scores the batcher's test set and ranks groups of its pairs on the device: the streaming loop of score_batches with Engine.board_put in
    place of read_probs -- the probabilities never leave the device and no engine call waits for the host -- and ONE Engine.rank_groups at the end.
    members / group_offsets address pairs by global line number (= the counter of the scoring writer's lines; evalrank.group_index builds them).
    on_scores(counter, labels, count): called per group of pairs once its put is queued (the caller that also wants the lines reads the board).
    -> (dict of Engine.rank_groups, number of pairs scored)"""
    import numpy as np
    group_offsets = np.ascontiguousarray(group_offsets, np.int64)
    members = None if members is None else np.ascontiguousarray(members, np.int64)
    saved = [(b, b.batchSize) for b in getattr(batcher, "batchers", [])]
    total = sum(int(b.labels.shape[0]) for b, _ in saved)
    need = int(members.max()) + 1 if members is not None and members.size else int(group_offsets[-1])
    engine.board_reserve(max(total, need, 1))
    counter = 0
    try:
        for b, _ in saved:
            b.batchSize = max(b.batchSize, ENGINE_BATCH_PATHS // max(1, b.numPaths))
        slots = [None] * (FEED_AHEAD + 2)
        k = 0
        fed = []
        done = False
        while True:
            while not done and len(fed) < FEED_AHEAD:
                got = _next_group(engine, batcher, merge)
                if got is None:
                    done = True
                    break
                labs, count, feed, _make = got
                slots[k] = feed(slots[k])
                fed.append((slots[k], labs, count))
                k = (k + 1) % len(slots)
            if not fed:
                break
            slot, labs, count = fed.pop(0)
            engine.forward_async(slot, class_id)
            engine.board_put(counter, count)
            if on_scores is not None:
                on_scores(counter, labs, count)
            counter += count
    finally:
        for b, size in saved:
            b.batchSize = size
    return engine.rank_groups(group_offsets, members, pos=pos, mode=mode, K=K, hist_len=hist_len), counter


def score_lines(engine, batcher, class_id=1):
    counter = 0
    for labs, preds in score_batches(engine, batcher, class_id):
        for i in range(len(labs)):
            yield "%d\t%.5f\t%s\n" % (counter, preds[i], lua_number(labs[i]))
            counter += 1


def write_scores(engine, batcher, f, class_id=1, merge=False):
    """the script's output loop (:110-118) into the binary file f; lines formatted by the host cores (kprn_format_score_lines)"""
    from . import _ffi
    counter = 0
    for labs, preds in score_batches(engine, batcher, class_id, merge):
        f.write(_ffi.format_score_lines(counter, preds, labs))
        counter += len(labs)
    return counter


def format_path(path, pad_entity):
    """a path [T,F] of 1-based ids -> its non-pad steps in step order, a step as `type ids,entity id,relation id` (the .int files' step feature), steps
    joined with ' '.  A pad step is one whose entity is the entity table's pad row (id = entityVocabSize: the row zeroPadTokens clears, the id
    pathformat.format_entity_pair skips)."""
    return " ".join(",".join(str(int(v)) for v in step) for step in path if int(step[-2]) != pad_entity)


def explain_test_set(engine, batcher, f, M, class_id=1, merge=False, res_file=None):
    """Scores the batcher's test set like write_scores and writes, into the text file f, the M strongest paths behind every scored line
    (Engine.explain_batch: one synchronous call per group of pairs; not a throughput mode).  One line per (scored line, filled place), tab separated:
    the global 0-based line counter of the score writer, the place (0-based), the path's index within its pair, its weight "%.5f", its score "%.6g",
    the path (format_path).  A pair with fewer than M paths has that many lines.  res_file (binary): also gets the score writer's lines, from the
    same pass -- the bytes write_scores writes.  -> pairs scored"""
    import numpy as np
    from . import _ffi
    pad_entity = int(engine.cfg.Ve)
    saved = [(b, b.batchSize) for b in getattr(batcher, "batchers", [])]
    counter = 0
    try:
        for b, _ in saved:       # the groups score_batches forms, so that both runs hand the engine the same batches
            b.batchSize = max(b.batchSize, ENGINE_BATCH_PATHS // max(1, b.numPaths))
        while True:
            if merge:
                got = batcher.getMergedGroup(ENGINE_BATCH_PATHS)
                if got is None:
                    break
                labs, idx, counts, count, _classId = got
                batch = engine.batch_ragged(idx, counts)
                off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
            else:
                got = batcher.getBatch()
                if got is None:
                    break
                labs, inputs, count, _classId = got
                batch = engine.batch(inputs)
                idx = np.asarray(inputs).reshape((-1,) + tuple(inputs.shape[2:]))
                off = np.arange(count + 1, dtype=np.int64) * int(inputs.shape[1])
            res = engine.explain_batch(batch, M, class_id)
            batch.free()
            if res_file is not None:
                res_file.write(_ffi.format_score_lines(counter, res["probs"], labs))
            pi, ps, pw = res["path_idx"], res["path_score"], res["path_weight"]
            lines = []
            for b in range(count):
                for r in range(pi.shape[1]):
                    q = int(pi[b, r])
                    if q < 0:
                        break
                    lines.append("%d\t%d\t%d\t%.5f\t%.6g\t%s\n" % (counter + b, r, q, pw[b, r], ps[b, r], format_path(idx[off[b] + q], pad_entity)))
            f.write("".join(lines))
            counter += count
    finally:
        for b, size in saved:
            b.batchSize = size
    return counter


def test_from_checkpoint(engine, input_dir, test_list, out_file, minibatch=512, log=None, rank=0, world=1, barrier=None, merge_path_counts=False):
    """engine: built with the same -top_k reducer the script would rebuild (:69-79).  merge_path_counts (an extension, default off): score
    the bucket files in ragged groups (score_batches merge=True); same lines, same order.

    Data-parallel scoring (new; the reference is single-device): pairs are independent units, so the FILES of the test list are
    sharded over the ranks in contiguous ranges (dp.shard_pairs), every rank scores its files with no collective and writes
    `<out_file>.part<rank>`; after `barrier()` (torch.distributed.barrier in a real run) rank 0 concatenates the parts in rank
    order = list order and renumbers the global 0-based counter, so that `out_file` is byte-identical to the single-rank file
    (the downstream join with test.list.entity is positional, eval/combine_result.py:24-27)."""
    if world <= 1:
        batcher = BatcherFileList(input_dir, minibatch, False, 1000, True, test_list, check_ids=False)   # (the engine validates every id)
        start = time.time()
        n = 0
        with open(out_file, "wb") as f:
            n = write_scores(engine, batcher, f, 1, merge_path_counts)
        if log:
            print("total cost time:", time.time() - start, file=log)
        return n
    import os
    import tempfile
    from .dp import shard_pairs
    with open(os.path.join(input_dir, test_list)) as f:
        files = [l.strip() for l in f if l.strip()]
    lo, hi = shard_pairs(len(files), rank, world)
    start = time.time()
    n = 0
    part = f"{out_file}.part{rank}"
    with open(part, "wb") as out:
        if hi > lo:
            # a list file of this rank's shard, next to the original (paths in it stay relative to input_dir)
            fd, shard_list = tempfile.mkstemp(prefix=f".{os.path.basename(test_list)}.rank{rank}.", dir=input_dir)
            try:
                with os.fdopen(fd, "w") as sl:
                    sl.write("\n".join(files[lo:hi]) + "\n")
                batcher = BatcherFileList(input_dir, minibatch, False, 1000, True, os.path.basename(shard_list), check_ids=False)
                n = write_scores(engine, batcher, out, 1, merge_path_counts)
            finally:
                os.unlink(shard_list)
    if barrier is not None:
        barrier()
    if rank == 0:
        counter = 0
        with open(out_file, "w") as f:
            for r in range(world):
                with open(f"{out_file}.part{r}") as pf:
                    for line in pf:
                        _, rest = line.split("\t", 1)
                        f.write("%d\t%s" % (counter, rest))
                        counter += 1
        for r in range(world):
            os.unlink(f"{out_file}.part{r}")
        if log:
            print("total cost time:", time.time() - start, file=log)
    return n


def test_and_rank(engine, input_dir, test_list, out_file, samples_file, entity_file, users_file=None, rank_out=None, minibatch=512, log=None,
                  merge_path_counts=False):
    """test_from_checkpoint (single rank) + the evaluation chain's metrics in one pass: every pair is scored once, its probability goes to the
    engine's board, the groups of `samples_file` (eval_score.py's test samples) are ranked on the device, and `out_file` gets the scoring writer's
    lines from the same board -- byte-identical to test_from_checkpoint's.  rank_out: the two lines of eval_score.py:158-159.
    -> (pairs scored, hits, ndcgs, groups ranked)"""
    import numpy as np
    from . import _ffi, evalrank
    with open(entity_file) as f:
        entity_lines = f.readlines()
    with open(samples_file) as f:
        samples = evalrank.read_samples(f)
    users = None
    if users_file:
        with open(users_file) as f:
            users = f.readlines()
    members, group_offsets, n_used = evalrank.group_index(entity_lines, samples, users)
    batcher = BatcherFileList(input_dir, minibatch, False, 1000, True, test_list, check_ids=False)
    start = time.time()
    labels = []
    ks = range(1, 16)
    if n_used == 0:
        res, n = None, 0
        with open(out_file, "wb") as f:
            n = write_scores(engine, batcher, f, 1, merge_path_counts)
        hits, ndcgs = {k: 0.0 for k in ks}, {k: 0.0 for k in ks}
    else:
        res, n = rank_test_set(engine, batcher, members, group_offsets, merge=merge_path_counts, on_scores=lambda c, labs, cnt: labels.append(np.array(labs[:cnt], np.float32)))
        with open(out_file, "wb") as f:
            if n:
                f.write(_ffi.format_score_lines(0, engine.board_read(0, n), np.concatenate(labels)))
        hits, ndcgs, n_used = evalrank.metrics_from_hist(res["hist"], 15, ks)
    if log:
        print("total cost time:", time.time() - start, file=log)
        print("hit score:", ["%.5f" % hits[k] for k in ks], file=log)      # eval_score.py:153-154
        print("ndcg score:", ["%.5f" % ndcgs[k] for k in ks], file=log)
    if rank_out:
        with open(rank_out, "w") as f:
            f.writelines(evalrank.format_metric_lines(hits, ndcgs, ks))
    return n, hits, ndcgs, n_used
