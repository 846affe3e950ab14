"""`python -m kprn_amd.score <flags>` == `th eval/test_from_checkpoint.lua <flags>`
(release/songPathRnn/eval/model_test_one_list.sh:20).  Flags: test_from_checkpoint.lua:23-31 plus the
model-shape flags (the Torch7 checkpoint carried the module graph; the native checkpoint carries weights)."""
import argparse
import sys

from . import model, scoring


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-input_dir", default=""); p.add_argument("-out_file", default=""); p.add_argument("-predicate_name", default="")
    p.add_argument("-meanModel", type=int, default=0); p.add_argument("-model_path", default=""); p.add_argument("-test_list", default="")
    p.add_argument("-gpu_id", type=int, default=-1); p.add_argument("-top_k", type=int, default=2); p.add_argument("-k", type=int, default=5)
    p.add_argument("-mergePathCounts", type=int, default=0)   # 1: bucket files are scored in ragged groups (an extension; same output lines)
    # ranking on the device (an extension): the evaluation chain's hit@k / ndcg@k (eval/combine_result.py, resort.py, eval_score.py) in the same run
    p.add_argument("-rank_samples", default=""); p.add_argument("-rank_entity", default=""); p.add_argument("-rank_users", default="")
    p.add_argument("-rank_out", default="")
    # explaining every scored line by its strongest paths (an extension): -explain_out FILE gets the -explain_paths M strongest paths per line and their
    # weights (scoring.explain_test_set); -out_file is written as without the flags
    p.add_argument("-explain_out", default=""); p.add_argument("-explain_paths", type=int, default=3)
    args, rest = p.parse_known_args(argv)
    assert args.input_dir != "", "input_dir isnt set. Point to the dir where train/dev/test.list files reside"
    params = model.parse_flags(rest, gamma_beside=None)
    model.check_gamma(params.gamma, model.reducer_of_score_flag(args.top_k), "-top_k", p.error)
    import os as _os
    params.reducer, params.K, params.initModel = model.reducer_of_score_flag(args.top_k), args.k, args.model_path
    params.gpuid = int(_os.environ.get("LOCAL_RANK", args.gpu_id)) if "LOCAL_RANK" in _os.environ else args.gpu_id
    print("using model:", args.model_path)
    eng = model.build_engine(params)
    print({0: "Reducer is max pool", 1: "Reducer is topK", 2: "Reducer is log sum"}[params.reducer])
    print("start predicting...")
    # under torch.distributed.run (python -m torch.distributed.run --nproc-per-node N -m kprn_amd.score ...): one rank per GPU, the test
    # list's files sharded over the ranks, test.res assembled by rank 0 in list order
    import os
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    barrier = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")   # (a barrier only: no tensor moves between the ranks)
        barrier = dist.barrier
    if args.explain_out:
        if args.rank_samples:
            sys.exit("-explain_out cannot be combined with -rank_samples: run the ranking and the explanation as two commands")
        if world > 1:
            sys.exit("-explain_out explains what one rank scored: run it on a single rank")
        if not 1 <= args.explain_paths <= 32:
            sys.exit("-explain_paths must be in 1..32")
        from .batcher import BatcherFileList
        fl = BatcherFileList(args.input_dir, 512, False, 1000, True, args.test_list, check_ids=False)
        with open(args.out_file, "wb") as res, open(args.explain_out, "w") as ex:
            scoring.explain_test_set(eng, fl, ex, args.explain_paths, merge=bool(args.mergePathCounts), res_file=res)
        return 0
    if args.rank_samples:
        assert args.rank_entity != "", "-rank_samples needs -rank_entity (the positional test.list.entity file)"
        assert world == 1, "-rank_samples ranks what one rank scored: run it on a single rank"
        scoring.test_and_rank(eng, args.input_dir, args.test_list, args.out_file, args.rank_samples, args.rank_entity, args.rank_users or None,
                              args.rank_out or None, log=sys.stdout, merge_path_counts=bool(args.mergePathCounts))
        return 0
    scoring.test_from_checkpoint(eng, args.input_dir, args.test_list, args.out_file, log=sys.stdout if rank == 0 else None,
                                 rank=rank, world=world, barrier=barrier, merge_path_counts=bool(args.mergePathCounts))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
