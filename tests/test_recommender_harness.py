"""tests/recommender_harness.py without a GPU: the default world's bytes, and the two monkeypatching helpers on a stub."""
from __future__ import annotations

import json

import pytest

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.model_io import load_model_dir
from tests.recommender_harness import forbid_gpu_work, graph_replays, synthetic_world


def test_synthetic_world_defaults_and_keywords(tmp_path):
    w = synthetic_world(tmp_path / "default")
    assert load_model_dir(w.model_dir).shape.layers == 2
    assert w.corpus_path == tmp_path / "default" / "processed" / "eval_corpus.json"
    want = syn.synthetic_catalog(700)
    assert list(json.loads(w.corpus_path.read_text()).items()) == list(want.items()) == list(w.corpus.items())
    small = synthetic_world(tmp_path / "cls", 20, pooling="cls")
    assert load_model_dir(small.model_dir).pooling == "cls" and load_model_dir(w.model_dir).pooling == "mean"
    assert json.loads(small.corpus_path.read_text()) == syn.synthetic_catalog(20)


class StubPath:
    def run(self, *a, **kw):
        return ("ran", a, kw)


class StubRecommender:
    def __init__(self):
        self._path = StubPath()

    def _fast_path(self):
        return self._path

    def _encode_search(self, *a, **kw):
        return "searched"


def test_graph_replays_records_the_path_and_passes_the_result_through(monkeypatch):
    rec = StubRecommender()
    replays = graph_replays(rec, monkeypatch)
    assert replays == []
    assert rec._fast_path().run(1, k=2) == ("ran", (1,), {"k": 2})
    assert rec._fast_path().run() == ("ran", (), {})
    assert len(replays) == 2 and all(r is rec._fast_path() for r in replays)
    monkeypatch.undo()
    rec._fast_path().run()
    assert len(replays) == 2


def test_forbid_gpu_work_makes_both_entry_points_raise(monkeypatch):
    rec = StubRecommender()
    forbid_gpu_work(rec, monkeypatch)
    with pytest.raises(AssertionError, match="GPU work"):
        rec._encode_search(["q"], 5)
    with pytest.raises(AssertionError, match="GPU work"):
        rec._fast_path().run("q", 5)
    monkeypatch.undo()
    assert rec._encode_search() == "searched" and rec._fast_path().run() == ("ran", (), {})
