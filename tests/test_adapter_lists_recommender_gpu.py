"""Recommender.fit_adapter_lists and RerankedRecommender.distill_adapter end to end on the GPU, on synthetic 2-layer
models: impression lists train and install the adapter, and a later recommend equals encode -> the reference's apply ->
search by hand; distilling a synthetic cross-encoder runs, lowers lists_loss on its own training lists and leaves the
index's bits alone; the plan's errors raise before any GPU work."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.recommender import DEFAULT_GAINS, MonitoredRecommender, Recommender
from tests.recommender_harness import QUERIES, forbid_gpu_work, graph_replays, synthetic_world, torch_cuda  # noqa: F401  (fixture)
from tests.adapter_harness import by_hand

pytestmark = pytest.mark.gpu


def impressions_of(rec, n=48, shown=20, seed=3):
    """n contexts, each shown `shown` distinct products: one purchased, two clicked, one with a number, the rest ignored."""
    rng = np.random.default_rng(seed)
    events = ["purchase", "click", "click", 2.5] + ["impression"] * (shown - 4)
    return [(c, {rec.product_ids[int(r)]: e for r, e in zip(rng.choice(len(rec.product_ids), shown, replace=False), events)})
            for c in syn.synthetic_user_contexts(n, seed=5)]


def test_fit_adapter_lists_installs_and_trains_in_place(tmp_path, torch_cuda, monkeypatch):
    world = synthetic_world(tmp_path)
    rec = MonitoredRecommender(world.model_dir, world.corpus_path, use_index=False)
    impressions = impressions_of(rec)
    plain = rec.recommend(QUERIES[0], 10)
    assert rec._adapter is None
    first = rec.fit_adapter_lists(impressions, epochs=2, batch_size=16, lr=1e-2)  # trains a new adapter and installs it
    ad = rec._adapter
    assert ad is not None and len(first) == 6 and ad.steps == 6 and np.isfinite(first).all()
    replays = graph_replays(rec, monkeypatch)
    got = rec.recommend(QUERIES[0], 10)
    assert got == by_hand(rec, ad.state()["delta"], QUERIES[0], 10) and got != plain
    more = rec.fit_adapter_lists(impressions, {**DEFAULT_GAINS, "click": 3}, epochs=3, batch_size=16, lr=1e-2)  # in place
    assert rec._adapter is ad and ad.steps == 6 + 9 and np.isfinite(more).all()
    assert rec.recommend(QUERIES[0], 10) == by_hand(rec, ad.state()["delta"], QUERIES[0], 10)
    assert len(replays) == 2  # the captured request followed the new weights
    # what it trained on scores better than at the start: the held-out number on the training lists, before and after
    texts = [c for c, _ in impressions]
    lists = [[(rec._pid_to_row[p], float(DEFAULT_GAINS.get(e, e))) for p, e in shown.items()] for _, shown in impressions]
    anchors = rec.model.encode_to_device(texts)
    from instacart_next_order_recommendation_amd.adapter import QueryAdapter

    zero = QueryAdapter(ad.dim, rec.device)
    assert ad.lists_loss(rec._index, anchors, lists) < zero.lists_loss(rec._index, anchors, lists, scale=ad.scale)
    zero.close()


def test_plan_errors_raise_before_gpu_work(tmp_path, torch_cuda, monkeypatch):
    world = synthetic_world(tmp_path, 100)
    rec = Recommender(world.model_dir, world.corpus_path, use_index=False)
    good = impressions_of(rec, n=4, shown=5)
    forbid_gpu_work(rec, monkeypatch)
    monkeypatch.setattr(rec.model, "encode_to_device", lambda *a, **kw: pytest.fail("encoded before the plan was checked"))
    pid = rec.product_ids[0]
    for impressions, kw, text in ((good + [("tea", {"no-such-product": "click"})], {}, "unknown product id"),
                                  (good + [("tea", {pid: "returned"})], {}, "unknown event 'returned'"),
                                  (good + [("tea", {pid: -1.0})], {}, "finite number >= 0"),
                                  (good + [("tea", {pid: "impression"})], {}, "impression 4 has no product with a positive gain"),
                                  (good, dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=text):
            rec.fit_adapter_lists(impressions, **kw)
    assert rec._adapter is None


def test_distill_adapter_from_a_synthetic_cross_encoder(tmp_path, torch_cuda):
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_cross_encoder_dir
    from instacart_next_order_recommendation_amd.reranker import CrossEncoderReranker, RerankedRecommender

    world = synthetic_world(tmp_path, 300, model_seed=8)
    ce_shape = syn.BertShape(vocab_size=len(syn.synthetic_vocab()), layers=2, n_normalize=0)
    ce_dir = write_synthetic_cross_encoder_dir(tmp_path / "ce", seed=9, shape=ce_shape)
    rec = Recommender(world.model_dir, world.corpus_path)
    rr = CrossEncoderReranker(ce_dir)
    both = RerankedRecommender(rec, rr, candidates=20)
    contexts = syn.synthetic_user_contexts(32, seed=9)
    for bad, kw, text in (([], {}, "non-empty"), ("milk", {}, "non-empty"), (contexts, dict(candidates=0), "candidates"),
                          (contexts, dict(candidates=2000), "candidates"), (contexts, dict(temperature=0.0), "temperature"),
                          (contexts, dict(negatives=5), "not \\['negatives'\\]"), (contexts, dict(epochs=0), "epochs")):
        with pytest.raises(ValueError, match=text):
            both.distill_adapter(bad, **kw)
    assert rec._adapter is None
    index_bits = rec._index.export().cpu().numpy().tobytes()

    # A synthetic bi-encoder's rows lie close together and a synthetic cross-encoder's logits differ little, so at D = 0
    # the scores are flat (the loss starts at ln 20) and the gradient is small.  AdamW's steps are lr-sized whatever the
    # gradient's size: a small lr keeps 12 of them inside the region where the first-order decrease holds, and a low
    # temperature makes the targets sharp enough to give that decrease a size (the float64 reference on rows of this
    # kind: flat targets at lr 5e-3 RAISE the training loss, lr 2e-4 lowers it at every sharpness tried).
    TEMPERATURE, LR = 0.01, 2e-4
    # the training lists, made here the way distill_adapter makes them, from the first stage BEFORE training
    found = rec.recommend_batch(contexts, 20)
    q_sides = rr.side_ids(contexts)
    lists = []
    for q, hits in zip(q_sides, found):
        logits = rr.logit_ids([q] * len(hits), [both._product_side[p] for p, _ in hits])
        lists.append(list(zip([rec._pid_to_row[p] for p, _ in hits], torch.softmax(logits / TEMPERATURE, dim=0).cpu().tolist())))
    anchors = rec.model.encode_to_device(contexts)
    from instacart_next_order_recommendation_amd.adapter import QueryAdapter

    zero = QueryAdapter(rec._index.dim, rec.device)
    before = zero.lists_loss(rec._index, anchors, lists, scale=30.0)
    zero.close()

    losses = both.distill_adapter(contexts, temperature=TEMPERATURE, epochs=6, batch_size=16, lr=LR)
    ad = rec._adapter
    assert ad is not None and len(losses) == 12 and ad.steps == 12 and np.isfinite(losses).all()
    after = ad.lists_loss(rec._index, anchors, lists)
    print(f"lists_loss on the training lists {before:.4f} -> {after:.4f}")
    assert 0 < after < before
    assert rec._index.export().cpu().numpy().tobytes() == index_bits
    assert both.recommend(contexts[0], 5)  # the two-stage request still answers, now through the adapter
    more = both.distill_adapter(contexts[:16], candidates=10, epochs=1, batch_size=16)  # in place, from the trained first stage
    assert rec._adapter is ad and ad.steps == 13 and len(more) == 1
    rr.close()
