"""-m gpu: the host-side mirror (batch feed -> MyOptimizer -> checkpoint -> scoring writer) end to end
on the GPU against an oracle replay, and the committed golden vectors through the C ABI."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, batcher, formats, model, optimizer, scoring, synth
from oracle.oracle import Oracle, make_cfg, make_opt

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    """a golden case's arrays; a case whose arrays exceed one fixture file keeps theta_after3 in <case>_after3.npz (tests/golden/make_golden.py)"""
    z = dict(np.load(os.path.join(GOLD, name)))
    after3 = os.path.join(GOLD, name[:-len(".npz")] + "_after3.npz")
    if os.path.exists(after3):
        z.update(np.load(after3))
    return z


@pytest.mark.parametrize("name", ["c1_small.npz", "c2_small.npz"])
def test_golden_vectors_through_the_c_abi(name):
    z = _golden(name)
    c = [int(x) for x in z["cfg"]]
    eng = _ffi.Engine(c[0], c[1], c[2], c[3], c[4], c[5], c[8], c[9], F=c[6], num_types=c[7], C_=c[10], reducer=c[11], K=c[12])
    eng.set_flat_params(z["theta"])
    b = eng.batch(z["idx"], z["labels"])
    out = eng.forward(b, 1, want=("probs", "pooled", "path_scores"))
    assert np.max(np.abs(out["path_scores"] - z["path_scores"])) / np.max(np.abs(z["path_scores"])) < 2e-5
    np.testing.assert_allclose(out["probs"], z["probs"][:, 0], rtol=1e-4)
    loss = eng.backward(b, 1)
    assert abs(loss - float(z["loss"])) < 1e-5
    g = eng.get_flat_grads()
    assert np.max(np.abs(g - z["grad"])) / np.max(np.abs(z["grad"])) < 2e-4
    opt = _ffi.make_opt(method=1, lr=1e-2)
    losses = [eng.train_step(b, opt) for _ in range(3)]
    np.testing.assert_allclose(losses, z["losses3"], rtol=2e-4)
    assert np.max(np.abs(eng.get_flat_params() - z["theta_after3"])) < 1e-4


def _write_dataset(root, ext):
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    os.makedirs(os.path.join(root, "test"), exist_ok=True)
    tr, te = [], []
    for i, (n, P) in enumerate([(40, 1), (24, 3), (9, 5)]):
        idx, labels = synth.make_paths(n, P, 6, Ve=500, seed=50 + i)
        name = f"train/train.txt.{P}{ext}"
        formats.save_path_file(os.path.join(root, name), labels, idx, 1)
        tr.append(name)
    for i, (n, P) in enumerate([(30, 2), (11, 4)]):
        idx, labels = synth.make_paths(n, P, 6, Ve=500, seed=70 + i)
        name = f"test/test.txt.{P}{ext}"
        formats.save_path_file(os.path.join(root, name), labels, idx, 1)
        te.append(name)
    open(os.path.join(root, "train.list"), "w").write("\n".join(tr) + "\n")
    open(os.path.join(root, "test.list"), "w").write("\n".join(te) + "\n")


FLAGS = ("-entityTypeVocabSize 6 -entityVocabSize 500 -relationVocabSize 9 -entityTypeEmbeddingDim 16 -entityEmbeddingDim 32 "
         "-relationEmbeddingDim 16 -numFeatureTemplates 3 -numEntityTypes 1 -rnnType lstm -rnnHidSize 64 -numLayers 2 -topK 2 "
         "-useAdam 1 -learningRate 0.01 -regularize 0 -includeEntity 1 -minibatch 16 -numEpochs 2 -gradientStepCounter 100000")


@pytest.mark.parametrize("ext", [".torch", ".npz"])
def test_train_loop_checkpoint_and_scoring_match_an_oracle_replay(tmp_path, ext):
    root = str(tmp_path)
    _write_dataset(root, ext)
    params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
    eng = model.build_engine(params)
    ocfg = make_cfg(Vt=6, Ve=500, Vr=9, dt=16, de=32, dr=16, H=64, L=2)
    o64 = Oracle(ocfg, np.float64)
    theta = eng.get_flat_params().astype(np.float64)  # the engine's own uniform(-paramInit, paramInit) init
    assert np.all(np.abs(theta) <= 0.1 + 1e-7) and abs(theta.mean()) < 1e-3
    log = io.StringIO()
    fl = batcher.BatcherFileList(root, params.minibatch, False, 100, True, "train.list")
    opt = optimizer.MyOptimizer(eng, {"numEpochs": 2, "epochHooks": [], "minibatchsize": 16}, model.opt_from_flags(params), out=log)
    hist = opt.train(fl)
    # oracle replay in the same order
    fl2 = batcher.BatcherFileList(root, params.minibatch, False, 100, False, "train.list")
    st = o64.new_state()
    oo = make_opt(method=1, lr=0.01, regularize=0)
    ohist = []
    for _ in range(2):
        tot, nb = 0.0, 0
        while True:
            got = fl2.getBatch()
            if got is None:
                break
            labels, data, n, cid = got
            l, _ = o64.train_step(theta, st, oo, data, labels, cid)
            tot += l
            nb += 1
        ohist.append(tot / nb)
        fl2.reset()
    np.testing.assert_allclose(hist, ohist, rtol=2e-4)
    assert "Total num batches 6" in log.getvalue() and "examples/sec" in log.getvalue() and "Iter: 2" in log.getvalue()
    assert np.max(np.abs(eng.get_flat_params() - theta)) < 2e-4
    # checkpoint -> fresh engine -> test_from_checkpoint writer
    ck = os.path.join(root, "model-latest")
    eng.save(ck)
    params2 = model.parse_flags(FLAGS.split() + ["-initModel", ck])
    eng2 = model.build_engine(params2)
    out_file = os.path.join(root, "test.res")
    n = scoring.test_from_checkpoint(eng2, root, "test.list", out_file)
    lines = open(out_file).read().splitlines()
    assert n == len(lines) == 41
    k = 0
    for name in open(os.path.join(root, "test.list")).read().split():
        labels, data, _ = formats.load_path_file(os.path.join(root, name))
        _, _, probs = o64.forward(theta, data)
        for i in range(len(labels)):
            c, s, lab = lines[k].split("\t")
            assert int(c) == k and lab == ("1" if labels[i] == 1 else "0")
            assert len(s.split(".")[1]) == 5 and abs(float(s) - probs[i, 0]) < 2e-5
            k += 1


def test_cli_train_and_score(tmp_path):
    root = str(tmp_path)
    _write_dataset(root, ".int")
    env = dict(os.environ, PYTHONPATH=ROOT)
    ck = os.path.join(root, "m")
    r = subprocess.run([sys.executable, "-m", "kprn_amd.train"] + FLAGS.split() +
                       ["-dataDir", root, "-model", ck, "-exptDir", os.path.join(root, "expt"), "-saveFrequency", "1", "-gpuid", "0"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Reducer is LogSumExp" in r.stdout and "Using Adam!" in r.stdout and "saving to " + ck + "-latest" in r.stdout
    assert os.path.exists(os.path.join(root, "expt", "config.txt"))
    out_file = os.path.join(root, "test.res")
    r = subprocess.run([sys.executable, "-m", "kprn_amd.score", "-input_dir", root, "-test_list", "test.list", "-model_path", ck + "-latest",
                        "-out_file", out_file, "-top_k", "2", "-gpu_id", "0"] + FLAGS.split(),
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out_file).read().splitlines()
    assert len(lines) == 41 and lines[0].startswith("0\t") and lines[-1].startswith("40\t")


def test_unsupported_reference_options_fail_loudly():
    # rnnType rnn (the shipped config.sh default) and gru are built: same flags, generic pipeline
    eng = model.build_engine(model.parse_flags(FLAGS.replace("-rnnType lstm", "-rnnType rnn").split()))
    assert "rnn1.h2h.bias" in eng.layout()
    eng = model.build_engine(model.parse_flags(FLAGS.replace("-rnnType lstm", "-rnnType gru").split()))
    assert "gru2.c_h2h.weight" in eng.layout()
    # the embedding variants of OneModel.lua:207-219 are built (a left-out table has width 0); dropout is not
    p = model.parse_flags(FLAGS.replace("-includeEntity 1", "-includeEntity 0").replace("-numLayers 2", "-numLayers 1").split())
    eng = model.build_engine(p)
    assert eng.D == 32 and eng.layout()["entity_emb"][1] == (500, 0)
    p = model.parse_flags((FLAGS + " -useDropout 1").split())
    with pytest.raises(_ffi.KprnError) as e:
        model.build_engine(p)
    assert e.value.code == _ffi.E_UNSUPPORTED


def test_hit_and_ndcg_at_k_match_the_oracle_within_1e_3():
    """north_star: hit@10 / ndcg@10 must match the reference's within 1e-3.  The MI / KKBox path sets are not shipped
    (SURVEY.md 6), so the clause is checked on MI-SHAPED synthetic evaluation data: every test user has 1 positive + 100
    uniformly sampled negative items (eval_score.py:17,97-129), each (user, item) pair a bucket of P paths; the engine's
    fp32 scores and the float64 oracle's scores go through the SAME chain the reference runs after scoring --
    "%.5f" score lines (test_from_checkpoint.lua:112), positional join (combine_result.py:24-27), 5-decimal ties resolved
    for the positive (heapq.nlargest) -- and hit@k / ndcg@k (k = 1, 5, 10, 15) are compared."""
    from kprn_amd import evalrank
    from oracle.oracle import Oracle, make_cfg
    users, negs, P, T, Ve = 1500, 100, 2, 6, 20000
    eng = _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2, param_init=0.35, seed=7)
    o64 = Oracle(make_cfg(Vt=6, Ve=Ve, Vr=9, dt=16, de=32, dr=16, H=64, L=2), np.float64)
    theta = eng.get_flat_params().astype(np.float64)
    pairs = users * (negs + 1)
    idx, _ = synth.make_paths(pairs, P, T, Ve=Ve, seed=99)
    labels = np.zeros(pairs, np.float32)
    labels[::negs + 1] = 1.0  # eval_score.py:113-114: the positive is the first candidate of each user
    g_scores = np.concatenate([eng.forward(eng.batch(idx[i:i + 8192]), 1)["probs"] for i in range(0, pairs, 8192)])
    o_scores = np.concatenate([o64.forward(theta, idx[i:i + 8192])[2][:, 0] for i in range(0, pairs, 8192)])

    def chain(scores):
        res = ["%d\t%.5f\t%s\n" % (i, scores[i], "%.14g" % labels[i]) for i in range(pairs)]
        ent = ["%d\t%d\t%d\n" % (labels[i], i // (negs + 1), i % (negs + 1)) for i in range(pairs)]  # label, user, item
        comb = evalrank.combine_result(ent, res)
        score_of = {}
        for line in comb:
            u, it, _, sc = line.strip().split("\t")
            score_of[(u, it)] = float(sc)
        samples = [(str(u), "0", [str(k) for k in range(1, negs + 1)]) for u in range(users)]
        return evalrank.eval_samples(score_of, samples, ks=[1, 5, 10, 15])

    gh, gn, n1 = chain(g_scores)
    oh, on, n2 = chain(o_scores)
    assert n1 == n2 == users
    assert float(np.max(np.abs(g_scores - o_scores) / o_scores)) < 1e-4  # the score bar itself
    for k in (1, 5, 10, 15):
        assert abs(gh[k] - oh[k]) <= 1e-3, (k, gh[k], oh[k])
        assert abs(gn[k] - on[k]) <= 1e-3, (k, gn[k], on[k])
    assert 0.0 < oh[10] < 1.0  # the ranking is not degenerate (scores are spread, not all tied)


def test_shuffled_epochs_match_an_oracle_replay_in_the_same_order(tmp_path):
    """OneModel.lua:326 trains with shuffle on: MyOptimizer streams every minibatch (rows of the untouched file, gathered inside the
    engine, kprn_batch_feed_rows_async) and sums the epoch's error on the device; an f64 oracle fed the same BatcherFileList order
    (same seed, tensors materialised on the host) must see the same per-epoch error and end at the same parameters."""
    root = str(tmp_path)
    _write_dataset(root, ".npz")
    params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
    eng = model.build_engine(params)
    theta = eng.get_flat_params().astype(np.float64)
    log = io.StringIO()
    fl = batcher.BatcherFileList(root, params.minibatch, True, 100, True, "train.list", seed=11)
    opt = optimizer.MyOptimizer(eng, {"numEpochs": 3, "epochHooks": [], "minibatchsize": 16}, model.opt_from_flags(params), gradientStepCounter=4, out=log)
    hist = opt.train(fl)
    o64 = Oracle(make_cfg(Vt=6, Ve=500, Vr=9, dt=16, de=32, dr=16, H=64, L=2), np.float64)
    fl2 = batcher.BatcherFileList(root, params.minibatch, True, 100, False, "train.list", seed=11)
    while fl2.getBatch(rows=True) is not None:   # (MyOptimizer's counting pass consumes one epoch order before the first reset)
        pass
    fl2.reset()
    st = o64.new_state()
    oo = make_opt(method=1, lr=0.01, regularize=0)
    ohist = []
    for _ in range(3):
        tot, nb = 0.0, 0
        while True:
            got = fl2.getBatch()
            if got is None:
                break
            labels, data, n, cid = got
            l, _ = o64.train_step(theta, st, oo, data, labels, cid)
            tot += l
            nb += 1
        ohist.append(tot / nb)
        fl2.reset()
    np.testing.assert_allclose(hist, ohist, rtol=3e-4)
    assert np.max(np.abs(eng.get_flat_params() - theta)) < 3e-4
    assert log.getvalue().count("Printing after 4 gradient steps") == 3 and "Iter: 3" in log.getvalue()


def test_engine_trained_model_round_trips_through_a_torch7_checkpoint(tmp_path):
    """OneModel.lua:392-400 <-> test_from_checkpoint.lua:68: a model trained here, written as torch.save{embeddingLayer, predictor_net},
    read back into a fresh engine, scores identically (bit for bit: the file holds float64 images of the fp32 parameters); a shuffled
    epoch exercises MyOptimizer's streaming feed on the way."""
    root = str(tmp_path)
    _write_dataset(root, ".npz")
    params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
    eng = model.build_engine(params)
    fl = batcher.BatcherFileList(root, params.minibatch, True, 100, True, "train.list", seed=5)   # shuffle: streamed batches
    opt = optimizer.MyOptimizer(eng, {"numEpochs": 2, "epochHooks": [], "minibatchsize": 16}, model.opt_from_flags(params), out=io.StringIO())
    hist = opt.train(fl)
    assert len(hist) == 2 and np.isfinite(hist).all()
    path = os.path.join(root, "model-latest")
    model.save_checkpoint_t7(eng, path)
    eng2 = model.build_engine(model.parse_flags(FLAGS.split() + ["-dataDir", root, "-seed", "777"]))
    assert not np.array_equal(eng2.get_flat_params(), eng.get_flat_params())
    assert model.load_checkpoint(eng2, path) == "t7"
    assert np.array_equal(eng2.get_flat_params(), eng.get_flat_params())
    idx, _ = synth.make_paths(40, 3, 6, Ve=500, seed=9)
    assert np.array_equal(eng2.forward(eng2.batch(idx), 1)["probs"], eng.forward(eng.batch(idx), 1)["probs"])
    native = os.path.join(root, "model-native")
    eng.save(native)
    assert model.load_checkpoint(eng2, native) == "native"


def test_data_parallel_step_at_world_one_equals_the_plain_step(tmp_path):
    """kprn_amd/dp.py on the GPU with a real process group of size 1 (RCCL: every collective is issued -- the call sequence of the
    N-GPU run): DataParallel.train_step == Engine.train_step, and MyOptimizer(dp=...) over shuffled files == MyOptimizer without it.
    The world-size-2 arithmetic (rank-ordered merge, global loss scale, ragged shards) is covered on CPU in tests/test_dp_gloo.py."""
    import socket
    import torch
    import torch.distributed as dist
    from kprn_amd import dp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        shape = (6, 500, 9, 16, 32, 16, 64, 2)
        stream = torch.cuda.current_stream().cuda_stream
        a = _ffi.Engine(*shape, seed=4, stream=stream)
        b = _ffi.Engine(*shape, seed=4)
        a.zero_pad_tokens(); b.zero_pad_tokens()   # (trainBatch zeroes the pad rows first: the scoring passes below come before / after it)
        opt = _ffi.make_opt(method=1, lr=1e-2)
        x = dp.DataParallel(dp.GpuAdapter(a, "cuda:0"))
        assert x.native   # the engine's own exchange: communicator bootstrapped over the process group, in-place all-gather on the engine's stream
        # ... and the same step with the collectives left to torch.distributed (the pack / merge hooks)
        t = _ffi.Engine(*shape, seed=4, stream=stream)
        t.zero_pad_tokens()
        os.environ["KPRN_DP_NATIVE"] = "0"
        try:
            xt = dp.DataParallel(dp.GpuAdapter(t, "cuda:0"))
        finally:
            del os.environ["KPRN_DP_NATIVE"]
        assert not xt.native
        data = [synth.make_paths(200 + 37 * i, 1 + i % 3, 6, Ve=500, seed=60 + i) for i in range(5)]
        for d_ in (x, xt):
            d_.set_capacity(max(len(np.unique(i[..., 1])) for i, _ in data) + 8)
        assert x.capacity % 4 == 0
        for k, (idx, lab) in enumerate(data):
            ba, bb, bt = a.batch(idx, lab), b.batch(idx, lab), t.batch(idx, lab)
            if k % 2:   # the scoring pass queued first (beside the training forward) ...
                a.forward_async(ba, 1)
                x.train_step(ba, opt, 1)
            else:       # ... or between the exchange's two halves
                x.train_step(ba, opt, 1, overlap=lambda: a.forward_async(ba, 1))
            pa = a.read_probs(ba.B)
            xt.train_step(bt, opt, 1, overlap=lambda: t.forward_async(bt, 1))
            pt = t.read_probs(bt.B)
            pb = b.forward(bb, 1)["probs"]
            b.train_step(bb, opt)
            np.testing.assert_allclose(pa, pb, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(pt, pb, rtol=1e-5, atol=1e-7)
            assert abs(a.read_loss() - b.read_loss()) < 1e-6 * max(1.0, abs(b.read_loss()))
        assert np.max(np.abs(a.get_flat_params() - b.get_flat_params())) < 2e-6
        assert np.max(np.abs(t.get_flat_params() - b.get_flat_params())) < 2e-6
        # the collective on a stream of its own (what a world > 1 run with the pass under the all-gather uses; at world 1 it degenerates)
        a.set_option("dp_comm_stream", "1")
        idx, lab = data[0]
        ba, bb = a.batch(idx, lab), b.batch(idx, lab)
        x.train_step(ba, opt, 1, overlap=lambda: a.forward_async(ba, 1))
        b.train_step(bb, opt)
        assert np.max(np.abs(a.get_flat_params() - b.get_flat_params())) < 2e-6
        t.close()
        # the training loop with a DataParallel object: shuffled files, streamed minibatches
        root = str(tmp_path)
        _write_dataset(root, ".npz")
        hists = []
        for use_dp in (True, False):
            params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
            eng = _ffi.Engine(6, 500, 9, 16, 32, 16, 64, 2, seed=9, stream=stream if use_dp else None)
            fl = batcher.BatcherFileList(root, params.minibatch, True, 100, True, "train.list", seed=3)
            xx = dp.DataParallel(dp.GpuAdapter(eng, "cuda:0"), equal_shards=False) if use_dp else None
            mo = optimizer.MyOptimizer(eng, {"numEpochs": 2, "epochHooks": [], "minibatchsize": 16}, model.opt_from_flags(params), dp=xx, out=io.StringIO())
            hists.append((mo.train(fl), eng.get_flat_params()))
            eng.close()
        np.testing.assert_allclose(hists[0][0], hists[1][0], rtol=1e-5)
        assert np.max(np.abs(hists[0][1] - hists[1][1])) < 5e-6
        # kprn_config.stream: NULL = "create a stream" -- the hooks refuse an engine whose stream the caller never saw; the legacy default
        # stream is asked for by name, and the exchange on it (torch's default stream IS the engine's stream then) equals the plain step
        blind = _ffi.Engine(*shape, seed=4)
        with pytest.raises(_ffi.KprnError):
            blind.dense_grad_buffer()
        blind.stream()
        blind.dense_grad_buffer()
        blind.close()
        c, d = _ffi.Engine(*shape, seed=4, stream=_ffi.STREAM_LEGACY_DEFAULT), _ffi.Engine(*shape, seed=4)
        assert c.stream() == 0
        c.zero_pad_tokens(); d.zero_pad_tokens()
        y = dp.DataParallel(dp.GpuAdapter(c, "cuda:0"))
        y.set_capacity(max(len(np.unique(i[..., 1])) for i, _ in data) + 8)
        for idx, lab in data[:3]:
            y.train_step(c.batch(idx, lab), opt, 1)
            d.train_step(d.batch(idx, lab), opt)
        assert np.max(np.abs(c.get_flat_params() - d.get_flat_params())) < 2e-6
        c.close(); d.close()
        a.close(); b.close()
    finally:
        dist.destroy_process_group()
