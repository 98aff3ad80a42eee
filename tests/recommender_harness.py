"""Shared by the GPU tests that build a whole Recommender on a synthetic model directory and catalog
(test_*_recommender_gpu, test_ivf_gpu, test_request_calls_gpu, the two catalog-edit tests, test_hybrid_gpu and the end-to-end
tests of the encoder features): the GPU fixture, the world a recommender is built on, the five queries, the recorder of
graph replays, the guard against GPU work, and a result row as (product id, score) pairs.  One definition each; importing
this needs no GPU.  Every test module still builds its OWN world in its own temp directory: several edit theirs."""
from __future__ import annotations

import json
from pathlib import Path
from typing import NamedTuple

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir
from tests.search_harness import torch_cuda  # noqa: F401  (re-exported: a recommender test imports one harness)

#: four seeded user contexts and one of a single product name (a one-order, few-token request)
QUERIES = syn.synthetic_user_contexts(4, seed=9) + ["[+1d w0h1] Milk."]


def two_layer_shape():
    """MiniLM's widths over the synthetic vocab, 2 layers instead of 6: 700 products encode in milliseconds."""
    return syn.BertShape(vocab_size=len(syn.synthetic_vocab()), layers=2)


class World(NamedTuple):
    model_dir: Path
    corpus_path: Path
    corpus: dict


def write_corpus(directory, corpus) -> Path:
    """directory/processed/eval_corpus.json (parents made) holding json.dumps(corpus): the key order is the row order."""
    path = Path(directory) / "processed" / "eval_corpus.json"
    path.parent.mkdir(parents=True)
    path.write_text(json.dumps(corpus))
    return path


def synthetic_world(tmp, n_products=700, *, model_seed=3, shape=two_layer_shape(), catalog_seed=42, **model_dir_kwargs):
    """tmp/model, a synthetic model directory (shape=None: write_synthetic_model_dir's own default, MiniLM's 6 layers;
    pooling= and architecture= go through), and tmp/processed/eval_corpus.json, synthetic_catalog(n_products,
    catalog_seed) -> World(model_dir, corpus_path, corpus)."""
    model_dir = write_synthetic_model_dir(Path(tmp) / "model", seed=model_seed, shape=shape, **model_dir_kwargs)
    corpus = syn.synthetic_catalog(n_products, seed=catalog_seed)
    return World(model_dir, write_corpus(tmp, corpus), corpus)


def graph_replays(rec, monkeypatch) -> list:
    """From here to the end of the test, every replay of a captured request graph (SingleRequestPath.run) appends its
    path object to the returned list: len() counts the requests that took the graph path."""
    cls = type(rec._fast_path())
    real_run, replays = cls.run, []

    def run(self, *a, **kw):
        replays.append(self)
        return real_run(self, *a, **kw)

    monkeypatch.setattr(cls, "run", run)
    return replays


def no_gpu(*a, **kw):
    raise AssertionError("GPU work before the argument check")


def forbid_gpu_work(rec, monkeypatch):
    """Both ways a request reaches the GPU raise AssertionError: rec._encode_search and the graph path's run."""
    monkeypatch.setattr(rec, "_encode_search", no_gpu)
    monkeypatch.setattr(type(rec._fast_path()), "run", no_gpu)


def as_results(rec, idx_row, score_row):
    """One result row (catalog rows, scores; row -1 = pad) -> [(product id, float score)] without the pads.  The
    test-side twin of Recommender._to_results, kept apart from it: an expectation is never built with the product's own
    helper."""
    return [(rec.product_ids[int(i)], float(s)) for i, s in zip(idx_row, score_row) if i >= 0]


PER_QUERY = ("aisles", "departments", "boosts", "within", "history")  # recommend_batch takes one entry per query of these


def assert_batch_equals_single_calls(rec, queries, top_k, excl, **options):
    """recommend_batch's row i is recommend(queries[i]) with the i-th entry of excl and of every PER_QUERY option and
    the other options as they are; recommend_batch_timed returns the same rows and two times > 0.  -> the batch."""
    batch = rec.recommend_batch(queries, top_k, excl, **options)
    for i, q in enumerate(queries):
        one = {k: v[i] if k in PER_QUERY else v for k, v in options.items()}
        assert batch[i] == rec.recommend(q, top_k, exclude_product_ids=excl[i], **one), i
    timed, enc_ms, sim_ms = rec.recommend_batch_timed(queries, top_k, excl, **options)
    assert timed == batch and enc_ms > 0 and sim_ms > 0
    return batch
