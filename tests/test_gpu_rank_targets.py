"""gpu: kprn_rank_targets against its host twin kprn_host_rank_targets (itself held to a numpy restatement by tests/test_rank_targets_host.py), integer
for integer: places and histogram, on the same shape list, with the scores written by board_write.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi

from . import rank_targets_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST_LEN = 15


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(6, 50, 9, 16, 32, 16, 64, 2, seed=3)
    yield e
    e.close()


def both(eng, c, mode, hist_len=HIST_LEN):
    """the board holds c's scores -> (device result, twin result)"""
    dev = eng.rank_targets(c["group_offsets"], c["target_offsets"], c["targets"], members=c["members"], mode=mode, hist_len=hist_len)
    host = _ffi.host_rank_targets(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], members=c["members"], mode=mode, hist_len=hist_len)
    return dev, host


def same(dev, host):
    bad = np.nonzero(dev["places"] != host["places"])[0]
    assert len(bad) == 0, (len(bad), bad[:8], dev["places"][bad[:8]], host["places"][bad[:8]])
    assert np.array_equal(dev["hist"], host["hist"]), (dev["hist"], host["hist"])


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_device_equals_twin_on_the_shape_list(eng, mode):
    """every size x every target count (0 .. every member, 1025 and 2000: a second chunk), the special groups, scattered members with repeated lines"""
    c = ref.cases(mode)
    eng.board_reserve(len(c["scores"]))
    eng.board_write(0, c["scores"])
    dev, host = both(eng, c, mode)
    same(dev, host)
    assert (host["places"] >= HIST_LEN).any() and host["hist"][HIST_LEN + 3] > 0
    again, _ = both(eng, c, mode)                      # the same call twice: identical, and hist holds one call only
    same(again, host)
    one = np.nonzero(np.diff(c["target_offsets"]) > 0)[0][-1]     # a sub-range of the groups: offsets into members that do not start at 0
    sub = dict(c, group_offsets=c["group_offsets"][one:one + 2], target_offsets=c["target_offsets"][one:one + 2] - c["target_offsets"][one],
               targets=c["targets"][c["target_offsets"][one]:c["target_offsets"][one + 1]])
    same(*both(eng, sub, mode, hist_len=1))


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_a_mixed_call_over_consecutive_runs(eng, mode):
    """members NULL: 1, 257, 4097 and 70 001 members in one call, 2000 targets in the 4097 (the second chunk), hist_len at its maximum"""
    c = ref.consecutive_cases(mode)
    assert np.diff(c["group_offsets"]).tolist()[:4] == [1, 257, 4097, 70001] and np.diff(c["target_offsets"]).tolist()[2] == 2000
    eng.board_reserve(len(c["scores"]))
    eng.board_write(0, c["scores"])
    for hist_len in (4096, 1):
        dev, host = both(eng, c, mode, hist_len)
        same(dev, host)


def test_unwritten_board_entries_are_invalid(eng):
    eng.board_reserve(1000)                           # every entry NaN
    eng.board_write(10, np.array([0.5, 0.25], np.float32))
    r = eng.rank_targets([0, 1000], [0, 3], [0, 10, 11], mode=ref.PRINTED, hist_len=4)
    assert r["places"].tolist() == [-1, 0, 0] and r["hist"].tolist() == [2, 0, 0, 0, 0, 1, 0, 998]   # (no non-target prints above zero, nor does target 0)
    r = eng.rank_targets([0, 10], [0, 2], [3, 9], mode=ref.PRINTED, hist_len=4)       # nothing valid: zero samples
    assert r["places"].tolist() == [-1, -1] and r["hist"].tolist() == [0, 0, 0, 0, 0, 2, 0, 10]


def test_results_do_not_depend_on_what_hipmalloc_returns():
    """a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), each call twice"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import rank_targets_ref as ref
        eng = _ffi.Engine(6, 50, 9, 16, 32, 16, 64, 2, seed=3)
        ok = []
        for mode in (0, 1):
            for c in (ref.consecutive_cases(mode), ref.cases(mode)):
                eng.board_reserve(len(c["scores"]))
                eng.board_write(0, c["scores"])
                host = _ffi.host_rank_targets(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], members=c["members"], mode=mode)
                for _ in range(2):
                    dev = eng.rank_targets(c["group_offsets"], c["target_offsets"], c["targets"], members=c["members"], mode=mode)
                    ok.append(bool(np.array_equal(dev["places"], host["places"]) and np.array_equal(dev["hist"], host["hist"])))
        eng.close()
        print(json.dumps(ok))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ok = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(ok) == 8 and all(ok), ok


def test_a_refused_call_leaves_the_outputs_and_the_board_untouched(eng):
    scores = np.linspace(0, 1, 10).astype(np.float32)
    eng.board_reserve(10)
    eng.board_write(0, scores)
    from .test_rank_targets_host import REFUSALS
    for what, members, goff, toff, targets, G, mode, hist_len, status in REFUSALS:
        arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        mem, go, to, tg = arr(members, np.int64), arr(goff, np.int64), arr(toff, np.int64), arr(targets, np.int32)
        places, hist = np.full(4, -77, np.int32), np.full(4096 + 4, -77, np.int64)
        rc = eng.L.kprn_rank_targets(eng.h, _ffi._fp(mem), _ffi._fp(go), _ffi._fp(to), _ffi._fp(tg), G, mode, _ffi._fp(places), _ffi._fp(hist), hist_len)
        assert rc == status and (places == -77).all() and (hist == -77).all(), what
        assert np.array_equal(eng.board_read(0, 10), scores), what
    go, to, tg = np.array([0, 5], np.int64), np.array([0, 1], np.int64), np.array([0], np.int32)
    hist = np.full(19, -77, np.int64)
    assert eng.L.kprn_rank_targets(eng.h, None, _ffi._fp(go), _ffi._fp(to), _ffi._fp(tg), 1, 0, None, _ffi._fp(hist), 15) == _ffi.E_ARG and (hist == -77).all()
    with pytest.raises(_ffi.KprnError) as ei:
        eng.rank_targets([0, 11], [0, 1], [0])
    assert ei.value.code == _ffi.E_INDEX
    r = eng.rank_targets([0, 10], [0, 1], [9], mode=ref.RAW)                          # and the next accepted call is not disturbed
    assert r["places"].tolist() == [0] and r["hist"][0] == 1 and r["hist"].sum() == 1


def test_no_board_is_refused():
    e = _ffi.Engine(6, 50, 9, 16, 32, 16, 64, 2, seed=3)
    try:
        with pytest.raises(_ffi.KprnError) as ei:
            e.rank_targets([0, 1], [0, 1], [0])
        assert ei.value.code == _ffi.E_ARG
    finally:
        e.close()
