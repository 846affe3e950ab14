"""not gpu: the group table the graph trainer derives for the pairwise loss (graph.groups_from_counts) and the -loss flag of python -m kprn_amd.train."""
import numpy as np
import pytest

from kprn_amd import graph, model


def test_groups_of_a_full_minibatch():
    go = graph.groups_from_counts([3, 1, 2, 5, 7, 1, 1, 1, 9, 2], 4)
    assert go.dtype == np.int32 and go.tolist() == [0, 5, 10]


def test_dropped_negatives_shrink_their_group():
    #        group 0: positive + 2 of 4 negatives | group 1: all five | group 2: positive alone
    counts = [2, 0, 4, 0, 1,                        1, 1, 1, 1, 1,      6, 0, 0, 0, 0]
    assert graph.groups_from_counts(counts, 4).tolist() == [0, 3, 8, 9]


def test_a_dropped_positive_leaves_its_negatives_a_group():
    counts = [0, 3, 3, 0, 1,   2, 2, 2, 2, 2]
    go = graph.groups_from_counts(counts, 4)
    assert go.tolist() == [0, 3, 8]   # (group 0 holds negatives only: it contributes no term, which is set_groups' count to find)


def test_an_all_dropped_group_is_empty_wherever_it_lies():
    counts = [0, 0, 0,   1, 0, 2,   0, 0, 0,   4, 4, 4,   0, 0, 0]
    assert graph.groups_from_counts(counts, 2).tolist() == [0, 0, 2, 2, 5, 5]


def test_one_negative_per_positive():
    assert graph.groups_from_counts([1, 1, 1, 0, 0, 1, 0, 0], 1).tolist() == [0, 2, 3, 4, 4]


def test_the_table_matches_the_batchs_pairs():
    rng = np.random.default_rng(1)
    for n_neg in (1, 4, 7):
        counts = rng.integers(0, 3, size=6 * (1 + n_neg))
        go = graph.groups_from_counts(counts, n_neg)
        assert go[0] == 0 and go[-1] == int((counts > 0).sum()) and len(go) == 7 and np.all(np.diff(go) >= 0)


def test_counts_that_are_no_whole_groups_are_refused():
    with pytest.raises(ValueError):
        graph.groups_from_counts([1, 1, 1], 1)


KG = ["-kg", "triples.tsv", "-vocab_dir", "vocab", "-interaction_rel", "rates"]


def test_the_loss_flag():
    assert model.parse_flags([]).loss == "bce"
    assert model.parse_flags(KG).loss == "bce"
    assert model.parse_flags(KG + ["-loss", "bpr"]).loss == "bpr"
    assert model.parse_flags(KG + ["-loss", "bce"]).loss == "bce"
    assert model.parse_flags(["-loss", "bce"]).loss == "bce"


def test_an_unknown_loss_exits(capsys):
    with pytest.raises(SystemExit):
        model.parse_flags(KG + ["-loss", "hinge"])
    assert "-loss" in capsys.readouterr().err


def test_bpr_without_a_graph_exits_with_a_message(capsys):
    with pytest.raises(SystemExit) as e:
        model.parse_flags(["-loss", "bpr"])
    assert e.value.code != 0
    assert "-loss bpr needs -kg" in capsys.readouterr().err
