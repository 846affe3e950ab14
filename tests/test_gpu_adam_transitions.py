"""-m gpu: the lazy-exact Adam step of the entity table across its transitions (include/kprn.h, kprn_opt: "bit-identical to the dense update of optim.adam").

A row that a minibatch does not touch falls behind and is later replayed with gradient 0 from the device's table of step sizes.  The straight road -- one kprn_opt
for the whole run, at most 40 steps, nothing read or written in between -- is held by tests/test_gpu_parity.py and tests/test_gpu_deterministic.py.  Here the same
SCRIPT of events (tests/adam_script.py) runs on engine L (lazy rows), engine D (entity_update = 1 at every step: the dense sweep) and, where the script reads, L0
(L without the reads), with option "deterministic" set first, and everything is compared with np.array_equal: flat parameters, both optimiser slots, every loss,
every array a read returned.  The scripts: more than 4 096 steps (the step-size table grows), a kprn_opt that changes between steps (lr, regularize, entity_update,
beta2 / eps; a change of method is refused), readers and writers while rows lag.  Shapes: the fused D = H = 64 engine with 32-float rows (G = 8 lanes a row), and the generic fp32 pipeline
under "deterministic" = "2" with rows of 64 (G = 16), 128 (G = 32) and 40 floats (the scalar row kernel).

Each script proves from its idx arrays that it is not vacuous (adam_script.assert_not_vacuous): at least 8 real rows coast for 5 or more steps and return, the pad
row is touched and coasts, and in D's own trajectory those rows moved while they coasted.  Where a whole-table flush or a row catch-up is the point of an event its
profile family (adam_flush_all / adam_rows_catchup) is asserted present, where none is due, absent.  One test anchors D to the float64 oracle at the bars of
tests/test_gpu_parity.py's _train_compare."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi
from oracle.oracle import Oracle, make_cfg
from oracle.oracle import make_opt as oracle_opt
from tests import adam_script as S
from tests.adam_script import cycle, ev, step

pytestmark = pytest.mark.gpu

PLAN0 = (("prefix_plan", "0"),)                       # "deterministic" = "2" trains batches that carry the index and no identical-prefix plan
FUSED_CASE = pytest.param(S.FUSED, "1", (), id="fused-de32")
GENERIC_CASES = [pytest.param(S.generic(de), "2", PLAN0, id=f"generic-de{de}") for de in (64, 128, 40)]
# the fused engine on 64-path tiles with the identical-prefix plan: the row update alone or merged with the dense arena's, the catch-up alone or with the prefix table
ROUTES = [pytest.param(S.FUSED, "1", (("small_tiles", "0"), ("prefix_plan", "1"), ("adam_merged", m), ("catchup_prefix", c)), id=f"fused-merged{m}-prefix{c}")
          for m in "01" for c in "01"]

BATCHES = S.four_batches()
A_ONLY = np.setdiff1d(S.rows_of(BATCHES[0]), np.concatenate([S.rows_of(b) for b in BATCHES[1:]]))   # rows that lag whenever A sits out
E_ROWS = S.rows_of(BATCHES[3])
ADAM = dict(method=1, lr=5e-3)
FLUSH, NO_FLUSH = {"adam_flush_all": True}, {"adam_flush_all": False}
CATCH_UP = {"adam_rows_catchup": True, "adam_flush_all": False}


def _find(script, tag):
    return [n for n, e in enumerate(script) if e.get("tag") == tag][0]


def _check_routes(lz, options, step_event, catchup_event=None):
    """which launches an Adam step and a catch-up of a batch with a plan took, by the options"""
    o = dict(options)
    if "adam_merged" not in o:
        return
    assert lz["plans"][0] and lz["plans"][1] and lz["plans"][2], lz["plans"]   # (the batches with pad steps carry a plan on these tiles)
    fam = lz["prof"][step_event]
    assert ("adam_step" in fam) == (o["adam_merged"] == "1") and ("adam_entity_rows" in fam) == (o["adam_merged"] == "0"), sorted(fam)
    if catchup_event is not None:
        fam = lz["prof"][catchup_event]
        assert ("prefix_fwd" in fam) == (o["catchup_prefix"] == "0"), sorted(fam)   # with the option the table rides in the catch-up's launch


def test_the_batches_are_what_the_scripts_assume():
    assert len(A_ONLY) >= 8 and S.PAD not in E_ROWS and all(S.PAD in S.rows_of(b) for b in BATCHES[:3])
    sets = [set(S.rows_of(b)) - {S.PAD} for b in BATCHES]
    assert sets[0] & sets[1] and sets[1] & sets[2] and sets[0] - sets[1] and sets[1] - sets[0] and sets[2] - sets[1]   # partial overlap
    assert not sets[3] & (sets[0] | sets[1] | sets[2])                                                            # E: rows nobody else uses


# ---- 1: across the growth of the step-size table ----------------------------------------------------------------------------------------------------------
def test_rows_coast_across_the_growth_of_the_step_table():
    """4 100 steps of 4 pairs x 1 path (adam_script.long_script): A's rows and the pad row sit out steps 4 .. 4 097 and replay step sizes from both sides of the
    table's growth at step 4 095, in the catch-up of a scoring pass (L) and in a step's row update (L0).  Then once more in a fresh process whose every new
    device allocation is filled with 0xFF bytes (KPRN_POISON_ALLOC=1): an entry the growth did not copy would be NaN.
    Measured on an MI355X: 7.8 s for the whole test -- five engines of 4 100 steps each and the start of the second process."""
    S.long_run()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import adam_script as S\n"
            "import numpy as np, json\n"
            "lz, d = S.long_run(with_l0=False)\n"
            "print(json.dumps({'equal': True, 'finite': bool(all(np.all(np.isfinite(x)) for x in lz['state'] + [lz['losses']]))}))\n"
            ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"equal": True, "finite": True}


# ---- 2: step size and regularisation change every step ------------------------------------------------------------------------------------------------------
def lr_reg_script():
    """30 steps, lr = 1e-2 (1 + k % 5); clip + L2 (the dense sweep, in L too) on steps 7-9 and 20"""
    s = []
    for k in range(1, 31):
        expect = FLUSH if k in (7, 20) else NO_FLUSH if k in (8, 10) else None    # entering the sweep flushes; inside it and on the way out nothing is pending
        s.append(step(cycle(k), expect=expect, method=1, lr=1e-2 * (1 + k % 5), regularize=int(k in (7, 8, 9, 20)), use_grad_clip=1, grad_clip_norm=0.02,
                      l2=1e-3))
    return s


@pytest.mark.parametrize("shape,det,options", [FUSED_CASE] + GENERIC_CASES)
def test_step_size_and_regularisation_change_every_step(shape, det, options):
    lz, _ = S.run_all(shape, lr_reg_script(), BATCHES, det, options)
    fam = lz["prof"][6]                                                      # step 7: the shapes train where this module says they do
    assert ("lstm_fused_bwd" in fam) == (shape == S.FUSED) and "adam_entity_dense" in fam, sorted(fam)


def test_the_dense_engine_follows_the_float64_oracle_through_that_schedule():
    """D itself against something independent: the schedule above, step by step with the same options, at _train_compare's bars (tests/test_gpu_parity.py:
    every loss within 2e-4 relative, the parameters after the 30 steps within 2e-4 absolute)"""
    script = lr_reg_script()
    Vt, Ve, Vr, dt, de, dr, H, L = S.FUSED
    o64 = Oracle(make_cfg(Vt=Vt, Ve=Ve, Vr=Vr, dt=dt, de=de, dr=dr, H=H, L=L), np.float64)
    eng = _ffi.Engine(*S.FUSED)
    eng.set_option("deterministic", "1")
    th32 = S.theta0(eng.n_params)
    eng.set_flat_params(th32)
    th, st = th32.astype(np.float64), o64.new_state()
    gb = [eng.batch(i, l) for i, l in BATCHES]
    for k, e in enumerate(script, 1):
        i, l = BATCHES[e["args"][0]]
        ol, _ = o64.train_step(th, st, oracle_opt(**e["opt"]), i, l)
        gl = eng.train_step(gb[e["args"][0]], _ffi.make_opt(entity_update=1, **e["opt"]))
        print(f"step {k}: loss {gl:.6f} oracle {ol:.6f} rel {abs(gl - ol) / max(1.0, abs(ol)):.2e}")
        assert abs(gl - ol) < 2e-4 * max(1.0, abs(ol)), (k, gl, ol)
    d = float(np.max(np.abs(eng.get_flat_params() - th)))
    print(f"max |theta - oracle| after 30 steps: {d:.3e}")
    assert d < 2e-4, d
    eng.close()


# ---- 3: the update mode switches ------------------------------------------------------------------------------------------------------------------------------
SWITCHES = [0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]


def switch_script(first_dense):
    """24 steps, L's entity_update by SWITCHES (first_dense: shifted by one, so that the very first step is dense and the second the switch to lazy rows).  A read
    that flushes stands directly before one 0 -> 1 switch: that switch finds nothing pending; the other 0 -> 1 switches flush"""
    pattern = ([1] + SWITCHES[:-1]) if first_dense else SWITCHES
    ups = [k for k in range(2, 25) if pattern[k - 1] == 1 and pattern[k - 2] == 0]
    s = []
    for k in range(1, 25):
        if k == ups[1]:
            s.append(ev("read_state", 0, expect=FLUSH))
        expect = FLUSH if k in (ups[0], ups[2]) else NO_FLUSH if k == ups[1] or k == 8 else None
        s.append(step(cycle(k), expect=expect, entity_update=pattern[k - 1], tag="lazy_step" if k == 8 else None, **ADAM))
    assert pattern[7] == 0
    return s


@pytest.mark.parametrize("first_dense", [False, True], ids=["lazy-first", "dense-first"])
@pytest.mark.parametrize("shape,det,options", [FUSED_CASE] + GENERIC_CASES + ROUTES)
def test_update_mode_switches_between_steps(shape, det, options, first_dense):
    script = switch_script(first_dense)
    lz, _ = S.run_all(shape, script, BATCHES, det, options)
    _check_routes(lz, options, _find(script, "lazy_step"))


# ---- 4: readers while rows lag --------------------------------------------------------------------------------------------------------------------------------
def reader_script():
    """20 steps; the steps are 1 A 2 B 3 C 4 E 5 B 6 C 7 E 8 A 9 B 10 C 11 E 12 B 13 C 14 E 15 A 16 B 17 C 18 E 19 B 20 C: the rows only A has lag
    whenever a reader comes, the pad row lags after every E"""
    at = {4: [ev("read_rows", [int(A_ONLY[0]), int(A_ONLY[1]), int(E_ROWS[0]), S.PAD], expect=FLUSH)],           # lagging, lagging, current, pad (lagging)
          6: [ev("score", 0, expect=CATCH_UP, tag="catch_up")],                                                   # a scoring pass: catch-up without a step
          11: [ev("score_host", 0, expect={"adam_entity_rows": False, "adam_step": False}, tag="host")],          # the host-buffer scoring entry point
          13: [ev("read_state", 0, expect=FLUSH), ev("read_state", 1, expect=NO_FLUSH)],
          14: [ev("read_table", expect=FLUSH)],
          17: [ev("save", "reader", expect=FLUSH)],
          18: [ev("zero_pad", expect={"adam_flush_all": False, "adam_rows_catchup": False})]}                     # the pad rows are known to be zero: no work
    s = []
    for k in range(1, 21):
        s.append(step(cycle(k), **ADAM))
        s += at.get(k, [])
    return s


@pytest.mark.parametrize("shape,det,options", [FUSED_CASE] + GENERIC_CASES + ROUTES)
def test_readers_while_rows_lag_see_the_dense_values_and_disturb_nothing(shape, det, options, tmp_path):
    script = reader_script()
    lz, _ = S.run_all(shape, script, BATCHES, det, options, str(tmp_path))
    fam = lz["prof"][_find(script, "host")]     # its rows come up to date by their list or with the whole table: one of the two launches
    assert fam.get("adam_rows_catchup", (0, 0))[1] + fam.get("adam_flush_all", (0, 0))[1] > 0, sorted(fam)
    o = dict(options)
    if "catchup_prefix" in o:
        assert lz["plans"][0], lz["plans"]
        assert ("prefix_fwd" in lz["prof"][_find(script, "catch_up")]) == (o["catchup_prefix"] == "0")   # with the option the table rides in the catch-up's launch


# ---- 5: writers while rows lag ----------------------------------------------------------------------------------------------------------------------------------
def writer_script():
    """36 steps, the writes applied to both engines: rows written after step 6 (a lagging row, a row of step 6's batch, the pad row), the flat vector after step 16
    (just after a checkpoint is saved), that checkpoint -- D's file, ten steps old -- loaded after step 26; ten further steps after each"""
    c_row = int(np.setdiff1d(S.rows_of(BATCHES[2]), [S.PAD])[0])
    at = {6: [ev("write_rows", [int(A_ONLY[0]), c_row, S.PAD], 7)], 16: [ev("save", "writer", expect=FLUSH), ev("write_flat", 8)], 26: [ev("load", "writer")]}
    s = []
    for k in range(1, 37):
        s.append(step(cycle(k), **ADAM))
        s += at.get(k, [])
    return s


@pytest.mark.parametrize("shape,det,options", [FUSED_CASE] + GENERIC_CASES)
def test_writers_while_rows_lag_land_on_the_dense_values(shape, det, options, tmp_path):
    S.run_all(shape, writer_script(), BATCHES, det, options, str(tmp_path))


# ---- 6: the optimiser's constants change ------------------------------------------------------------------------------------------------------------------------
def constants_script(what):
    """rows lag at step 10 (the rows only A has: touched at step 8).  "betas": beta2 0.999 -> 0.99 and eps 1e-8 -> 1e-6 from step 10 on -- steps 9 and before are
    replayed with the constants they ran with: the step that brings new ones flushes first.  "method": an Adagrad step asked for after step 9 is refused -- through
    every entry point, with KPRN_E_ARG and the reason -- and the handle trains on as if nobody had asked.  (Both methods keep their state in optimiser slot 0:
    before this test the dense engine itself answered NaN to Adam -> Adagrad, the square root of a negative first moment, and the lazy one replayed step sizes
    Adagrad's steps never wrote.)"""
    s = []
    for k in range(1, 25):
        late = k >= 10
        if what == "method" and k == 10:
            s.append(S.refused_step(cycle(k), **dict(ADAM, method=0)))
        opt = dict(ADAM, beta2=0.99 if late else 0.999, eps=1e-6 if late else 1e-8) if what == "betas" else ADAM
        s.append(step(cycle(k), expect=(FLUSH if k == 10 else NO_FLUSH if k == 11 else None) if what == "betas" else None, **opt))
    return s


@pytest.mark.parametrize("what", ["betas", "method"])
def test_optimiser_constants_change_while_rows_lag(what):
    S.run_all(S.FUSED, constants_script(what), BATCHES)


def test_adam_after_adagrad_is_refused_and_the_handle_trains_on():
    eng = _ffi.Engine(*S.FUSED)
    eng.set_flat_params(S.theta0(eng.n_params))
    b = eng.batch(*BATCHES[0])
    adagrad = _ffi.make_opt(method=0, lr=5e-3)
    eng.train_step(b, adagrad)
    before = [eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1)]
    with pytest.raises(_ffi.KprnError) as e:
        eng.train_step(b, _ffi.make_opt(**ADAM))
    assert e.value.code == _ffi.E_ARG and "adagrad to adam" in e.value.msg and "slot 0" in e.value.msg, e.value.msg
    for x, y in zip(before, [eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1)]):
        assert np.array_equal(x, y)
    assert np.isfinite(eng.train_step(b, adagrad)) and not np.array_equal(before[0], eng.get_flat_params())
    eng.close()
