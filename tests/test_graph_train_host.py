"""not gpu: what training from a knowledge graph needs on the host -- KnowledgeGraph.interactions / item_weights on a ten-triple graph written out here,
and the -kg flags of python -m kprn_amd.train (model.parse_flags)."""
import numpy as np
import pytest

from kprn_amd import model
from kprn_amd.graph import KnowledgeGraph
from kprn_amd.pathformat import Vocabs

from .test_path_find_host import _write_vocab

TRIPLES = [("u0", "rate", "m0"), ("u0", "rate", "m1"), ("u1", "rate", "m1"), ("u2", "rate", "m1"), ("u2", "rate", "m3"), ("u0", "rate", "m1"),   # (one twice)
           ("m1", "_rate", "u0"), ("m1", "act", "a0"), ("a0", "_act", "m1"), ("u3", "act", "m4")]


@pytest.fixture()
def kg(tmp_path):
    _write_vocab(str(tmp_path))
    return KnowledgeGraph.from_triples(TRIPLES, Vocabs(str(tmp_path)), 1)


def test_interactions_are_the_distinct_sorted_pairs_of_one_relation(kg):
    assert len(TRIPLES) == 10
    e = kg.entity_id
    got = kg.interactions("rate")
    assert got.dtype == np.int32 and got.tolist() == [[e("u0"), e("m0")], [e("u0"), e("m1")], [e("u1"), e("m1")], [e("u2"), e("m1")], [e("u2"), e("m3")]]
    assert kg.interactions("_rate").tolist() == [[e("m1"), e("u0")]]
    assert kg.interactions("act").tolist() == sorted([[e("m1"), e("a0")], [e("u3"), e("m4")]])
    assert kg.interactions("_act").shape == (1, 2)
    with pytest.raises(ValueError):
        kg.interactions("made_of")


def test_item_weights_are_in_degree_to_the_alpha(kg):
    items = [kg.entity_id(n) for n in ("m0", "m1", "m2", "m3", "m4")]
    deg = np.array([1, 3, 0, 1, 0], np.float64)                                  # over "rate": the repeated triple counts once, "act" into m4 not at all
    w0 = kg.item_weights(items, 0, "rate")
    assert w0.dtype == np.float32 and w0.tolist() == [1, 1, 1, 1, 1]
    assert np.array_equal(kg.item_weights(items, 1, "rate"), deg.astype(np.float32))
    assert np.array_equal(kg.item_weights(items, 0.75, "rate"), (deg ** 0.75).astype(np.float32))
    assert kg.item_weights(items, 1, "act").tolist() == [0, 0, 0, 0, 1]


def test_kg_flags(capsys):
    base = ["-numFeatureTemplates", "3", "-numEntityTypes", "1"]
    p = model.parse_flags(base)
    assert p.kg == "" and p.vocab_dir == "" and p.interaction_rel == ""
    for extra in (["-kg", "t.tsv"], ["-kg", "t.tsv", "-vocab_dir", "v"], ["-kg", "t.tsv", "-interaction_rel", "rate"]):
        with pytest.raises(SystemExit):
            model.parse_flags(base + extra)
        assert "-kg needs -vocab_dir" in capsys.readouterr().err
    p = model.parse_flags(base + ["-kg", "t.tsv", "-vocab_dir", "v", "-interaction_rel", "rate"])
    assert (p.kg, p.vocab_dir, p.interaction_rel) == ("t.tsv", "v", "rate")
    assert (p.negatives, p.neg_alpha, p.neg_attempts, p.min_hops, p.max_hops, p.max_paths, p.sampleSeed) == (4, 0.0, 16, 2, 3, 28, 1)
    p = model.parse_flags(base + ["-kg", "t.tsv", "-vocab_dir", "v", "-interaction_rel", "rate", "-negatives", "2", "-neg_alpha", "0.5", "-sampleSeed", "9"])
    assert (p.negatives, p.neg_alpha, p.sampleSeed) == (2, 0.5, 9)
