"""Recommender.similar_products / recommend_from_products / recommend(..., like=, unlike=) end to end on the GPU, on the
default world of tests/recommender_harness.py (2-layer model directory, 700 products): a request equals the host
restatement - tests/compose_reference.py over the recommender's own text embedding and exported rows, then
oracle.search - bit for bit; it composes with every other option; without a known id it is today's request on the graph
path; and the command line prints what the methods return."""
from __future__ import annotations

import json

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.baselines import ItemItemCFBaseline
from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender, Recommender
from oracle import oracle
from tests import compose_reference as ref
from tests import recommender_harness as harness
from tests.recommender_harness import QUERIES, as_results, graph_replays, synthetic_world, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PER_QUERY = harness.PER_QUERY + ("like", "unlike")  # recommend_batch takes one entry per query of these


def assert_batch_equals_single_calls(rec, queries, top_k, excl, **options):
    """recommender_harness.assert_batch_equals_single_calls with like / unlike among the per-query options."""
    batch = rec.recommend_batch(queries, top_k, excl, **options)
    for i, q in enumerate(queries):
        one = {k: v[i] if k in PER_QUERY and v is not None else v for k, v in options.items()}
        assert batch[i] == rec.recommend(q, top_k, exclude_product_ids=excl[i], **one), i
    if "probes" not in options:  # (recommend_batch_timed has no probes keyword)
        timed, enc_ms, sim_ms = rec.recommend_batch_timed(queries, top_k, excl, **options)
        assert timed == batch and enc_ms > 0 and sim_ms > 0
    return batch


@pytest.fixture(scope="module")
def rec(tmp_path_factory, torch_cuda):
    w = synthetic_world(tmp_path_factory.mktemp("compose_rec"))
    sets = {"store": list(w.corpus)[::2], "stock": list(w.corpus)[100:600]}
    r = MonitoredRecommender(w.model_dir, w.corpus_path, use_index=False, product_sets=sets)
    assert r._fast is not None and r._index.n_facets == 2 and len(r.product_ids) == 700
    return r


@pytest.fixture(scope="module")
def stored(rec):
    """The rows the index holds, as exported, and the storage kind the oracle's search takes."""
    return rec._index.export().cpu().numpy(), "bf16" if rec._index.storage.startswith("bf16") else "f32"


@pytest.fixture(scope="module")
def feedback(rec):
    """Per query (like, unlike): id lists, mappings, an unknown id, None and [] - the forms a request may take."""
    rng = np.random.default_rng(21)
    ids = rec.product_ids
    pick = lambda n: [ids[int(r)] for r in rng.choice(700, n, replace=False)]  # noqa: E731
    a, b, c, d = pick(12), pick(5), pick(64), pick(3)
    like = [a[:8] + ["no-such-product"], None, {p: float(w) for p, w in zip(c, rng.uniform(0.0, 0.2, 64))}, [], d[:1]]
    unlike = [a[8:], b, None, {d[1]: 0.75, d[2]: 0.0}, None]
    return like, unlike


def terms_of(rec, like, unlike, like_weight=1.0, unlike_weight=0.5):
    """The test's own statement of the weights: an id list is a centroid, a mapping is taken as written."""
    terms = []
    for given, scale, sign in ((like, like_weight, 1.0), (unlike, unlike_weight, -1.0)):
        if given is None:
            continue
        known = [p for p in given if p in rec._pid_to_row]
        for p in known:
            w = sign * given[p] if hasattr(given, "items") else sign * scale / len(known)
            terms.append((rec._pid_to_row[p], np.float32(w)))
    return terms


def expected(rec, stored, query, terms, top_k, exclude=(), query_weight=1.0, admit=None):
    """Reference compose over the recommender's own text embedding (None: no text part) and exported rows, then the
    oracle's search of the catalog with that vector -> [(product id, score)]."""
    p_hat, kind = stored
    base = None if query is None else rec.model.encode([query])
    q = ref.compose_lists(p_hat, base, [terms], None if query is None else [query_weight])
    excl = {rec._pid_to_row[p] for p in exclude if p in rec._pid_to_row}
    if admit is not None:
        excl |= set(np.flatnonzero(~admit).tolist())
    idx, sc = oracle.search(q, rec.product_embeddings, top_k, [sorted(excl)], storage=kind)
    return as_results(rec, idx[0], sc[0])


def test_similar_products_is_the_search_of_the_products_own_row(rec, stored, monkeypatch):
    p_hat, kind = stored
    np.testing.assert_array_equal(p_hat, ref.stored_rows(rec.product_embeddings, rec._index.storage))

    def no_encoder(*a, **kw):
        raise AssertionError("an encoder launch for a query without a text")

    monkeypatch.setattr(rec.model.encoder, "encode_packed_host", no_encoder)
    for row in (0, 347, 699):
        pid = rec.product_ids[row]
        idx, sc = rec._index.search(p_hat[row:row + 1], 10, [[row]])
        got = rec.similar_products(pid, 10)
        assert got == as_results(rec, idx[0].cpu().numpy(), sc[0].cpu().numpy()) == expected(rec, stored, None, [(row, 1.0)], 10, [pid])
        assert len(got) == 10 and pid not in [p for p, _ in got]
        # the product itself comes first.  Its score is 1 up to: the stored row's norm, |p| = 1 +- 8.5 u for fp32 rows (the
        # 64 partial chains of dim / 64 fmaf and the 6 butterfly sums carry (dim / 64 + 7) u on the sum of squares, half of
        # it after the root, + u for the root, + u for the division), + 2^-9 for rows rounded to bfloat16; the query's
        # own normalisation, 7.5 u + u again; and the score's chain of dim fmaf over non-negative products, dim u.
        with_self = rec.similar_products(pid, 10, exclude_self=False)
        u, dim = 2.0 ** -24, p_hat.shape[1]
        norm = (dim // 64 + 7) / 2 + 1
        bound = ((norm + 1) + (norm + 1) + dim) * u * 1.001 + (2.0 ** -9 if kind == "bf16" else 0.0)
        assert with_self[0][0] == pid and abs(with_self[0][1] - 1.0) <= bound, (with_self[0], bound)
        assert with_self[1:] == got[:9]
        assert rec.similar_products(pid, 10, exclude_product_ids={got[0][0]}) == rec.similar_products(pid, 11)[1:]
    # a basket's profile: ids share like_weight, a mapping is taken as written; the products are not removed
    basket = [rec.product_ids[r] for r in (5, 17, 600)]
    want = expected(rec, stored, None, [(5, np.float32(1 / 3)), (17, np.float32(1 / 3)), (600, np.float32(1 / 3))], 20)
    assert rec.recommend_from_products(basket + ["no-such-product"], 20) == want
    assert {p for p, _ in want} & set(basket)
    weighted = {basket[0]: 2.0, basket[2]: 0.25}
    assert rec.recommend_from_products(weighted, 20, set(basket)) == \
        expected(rec, stored, None, [(5, np.float32(2.0)), (600, np.float32(0.25))], 20, basket)
    assert rec.recommend_from_products(["no-such-product"], 20) == [] and rec.recommend_from_products({}, 20) == []
    with pytest.raises(KeyError):
        rec.similar_products("no-such-product")
    # with other options: inside an aisle, diversified
    aisle = rec.aisles[3]
    admit = np.asarray([f". Aisle: {aisle}. " in t for t in rec.product_texts], bool)
    assert rec.similar_products(rec.product_ids[0], 5, aisles=[aisle]) == \
        expected(rec, stored, None, [(0, 1.0)], 5, [rec.product_ids[0]], admit=admit)
    assert len(rec.similar_products(rec.product_ids[0], 5, diversity=0.5)) == 5


def test_like_and_unlike_equal_the_host_restatement(rec, stored, feedback):
    like, unlike = feedback
    moved = 0
    for i, q in enumerate(QUERIES):
        terms = terms_of(rec, like[i], unlike[i])
        got = rec.recommend(q, 20, like=like[i], unlike=unlike[i])
        assert got == expected(rec, stored, q, terms, 20), i
        moved += got != rec.recommend(q, 20)
    assert moved == len(QUERIES)  # every query of the fixture has a known id: none is the plain request
    # the weights: query_weight, like_weight, unlike_weight; exclusions drop liked products, nothing else does
    q, lk, ul = QUERIES[0], like[0], unlike[0]
    got = rec.recommend(q, 20, like=lk, unlike=ul, query_weight=0.5, like_weight=2.0, unlike_weight=1.5)
    assert got == expected(rec, stored, q, terms_of(rec, lk, ul, 2.0, 1.5), 20, query_weight=0.5)
    only_products = rec.recommend(q, 20, like=lk, query_weight=0.0)
    assert [p for p, _ in only_products] == [p for p, _ in rec.recommend_from_products(lk, 20)]
    assert set(lk) & {p for p, _ in only_products}
    assert rec.recommend(q, 20, exclude_product_ids=set(lk), like=lk, query_weight=0.0) == expected(rec, stored, q, terms_of(rec, lk, None), 20, lk, 0.0)
    # the monitored form passes the keywords through and times the request
    got = rec.recommend(q, 20, user_id="u1", like=lk, unlike=ul)
    assert got == expected(rec, stored, q, terms_of(rec, lk, ul), 20) and rec.last_metrics.num_recommendations == 20
    assert rec.last_metrics.query_embedding_time_ms > 0 and rec.last_metrics.similarity_compute_time_ms > 0


def test_it_composes_with_the_other_options(rec, stored, feedback):
    like, unlike = feedback
    n = len(QUERIES)
    excl = [None, {rec.product_ids[3]}, set(like[2]), None, set()]
    assert_batch_equals_single_calls(rec, QUERIES, 20, excl, like=like, unlike=unlike)
    assert_batch_equals_single_calls(rec, QUERIES, 20, excl, like=like, unlike=None, query_weight=0.25, like_weight=3.0)
    aisles = [None, rec.aisles[:40], None, rec.aisles[10:90], rec.aisles[:5]]
    within = ["store", None, ["store", "stock"], None, "stock"]
    boosts = [{rec.product_ids[9]: 0.3, rec.product_ids[400]: 0.01}, None, {rec.product_ids[100]: 0.2}, None, None]
    batch = assert_batch_equals_single_calls(rec, QUERIES, 10, excl, like=like, unlike=unlike, aisles=aisles, within=within,
                                             boosts=boosts, diversity=0.3, max_per_aisle=2)
    plain = rec.recommend_batch(QUERIES, 10, excl, aisles=aisles, within=within, boosts=boosts, diversity=0.3, max_per_aisle=2)
    assert sum(b != p for b, p in zip(batch, plain)) >= 3
    assert_batch_equals_single_calls(rec, QUERIES, 10, excl, like=like, unlike=unlike, max_per_aisle=1, max_per_department=3)
    assert_batch_equals_single_calls(rec, QUERIES, 10, excl, like=like, boosts=boosts, only_boosted=True)
    # against the restatement under a facet: the result of excluding every product outside the aisles
    admit = np.asarray([any(f". Aisle: {a}. " in t for a in aisles[3]) for t in rec.product_texts], bool)
    assert rec.recommend(QUERIES[3], 10, aisles=aisles[3], like=like[3], unlike=unlike[3]) == \
        expected(rec, stored, QUERIES[3], terms_of(rec, like[3], unlike[3]), 10, admit=admit)


def test_it_composes_with_probes_and_history(tmp_path, torch_cuda):
    w = synthetic_world(tmp_path, 300)
    ids = list(w.corpus)
    rng = np.random.default_rng(8)
    baskets = [[ids[int(r)] for r in rng.choice(300, int(rng.integers(2, 9)), replace=False)] for _ in range(400)]
    rec = Recommender(w.model_dir, w.corpus_path, use_index=False, ann_lists=8, cf=ItemItemCFBaseline.from_arrays(baskets, {}, ids))
    stored = (rec._index.export().cpu().numpy(), "bf16" if rec._index.storage.startswith("bf16") else "f32")
    queries = QUERIES[:3]
    like = [ids[10:14], None, {ids[200]: 0.5}]
    unlike = [None, ids[50:52], [ids[7]]]
    excl = [None, {ids[11]}, None]
    batch = assert_batch_equals_single_calls(rec, queries, 10, excl, like=like, unlike=unlike, probes=3, diversity=0.2)
    assert sum(b != p for b, p in zip(batch, rec.recommend_batch(queries, 10, excl, probes=3, diversity=0.2))) >= 2
    # every list probed is the exact search: the restatement again
    for i, q in enumerate(queries):
        assert rec.recommend(q, 10, exclude_product_ids=excl[i], like=like[i], unlike=unlike[i], probes=8) == \
            expected(rec, stored, q, terms_of(rec, like[i], unlike[i]), 10, excl[i] or ())
    history = [baskets[0], baskets[1][:2], None]
    batch = assert_batch_equals_single_calls(rec, queries[:2], 10, excl[:2], like=like[:2], unlike=unlike[:2], history=history[:2],
                                             cf_weight=0.5)
    assert batch != rec.recommend_batch(queries[:2], 10, excl[:2], history=history[:2], cf_weight=0.5)  # the content list moved


def test_without_a_known_id_it_is_the_plain_request_on_the_graph_path(rec, monkeypatch):
    q = QUERIES[0]
    plain = rec.recommend(q, 20)
    replays = graph_replays(rec, monkeypatch)
    for kw in (dict(like=None), dict(like=[]), dict(unlike=[]), dict(like=["no-such-product"], unlike={"-1": 1.0}),
               dict(like={}, query_weight=3.0, like_weight=0.0)):
        assert rec.recommend(q, 20, **kw) == plain, kw
    assert len(replays) == 5
    assert rec.recommend(q, 20, like=[rec.product_ids[0]]) != plain and len(replays) == 5  # with a term: un-captured
    assert rec.recommend_batch([q, q], 20, like=[None, ["no-such-product"]]) == [plain, plain]
    # bad arguments raise before any GPU work
    harness.forbid_gpu_work(rec, monkeypatch)
    for kw, text in ((dict(like="12"), "not a string"), (dict(like={"1": -1.0}), "finite number >= 0"),
                     (dict(like=["1"], unlike=["1"]), "in both like and unlike"), (dict(unlike=["1", "1"]), "named twice")):
        with pytest.raises(ValueError, match=text):
            rec.recommend(q, 20, **kw)
    with pytest.raises(ValueError, match="one entry per query"):
        rec.recommend_batch([q, q], 20, like=["1", "2"][0])
    with pytest.raises(ValueError, match="not a string"):
        rec.similar_products(rec.product_ids[0], 5, exclude_self=False, boosts="12", boost_weight=1.0)


def test_cli_similar_to_and_like(rec, tmp_path, capsys):
    import yaml

    from instacart_next_order_recommendation_amd import cli

    cfg = tmp_path / "inference.yaml"
    cfg.write_text(yaml.safe_dump({"model_dir": str(rec.model_dir), "corpus": str(rec.corpus_path), "use_index": False,
                                   "top_k": 5, "query": QUERIES[0]}))
    a, b, c = rec.product_ids[40], rec.product_ids[41], rec.product_ids[500]

    def rows():
        return [(r["product_id"], r["score"]) for r in map(json.loads, capsys.readouterr().out.splitlines())]

    assert cli.main(["--config", str(cfg), "--json", "--similar-to", a]) == 0
    assert rows() == rec.similar_products(a, 5)
    assert cli.main(["--config", str(cfg), "--json", "--similar-to", a, "--top-k", "7", "--department", rec.departments[0]]) == 0
    assert rows() == rec.similar_products(a, 7, departments=[rec.departments[0]])
    assert cli.main(["--config", str(cfg), "--json", "--like", a, "--like", b, "--unlike", f"{c}=0.75", "--like-weight", "2",
                     "--query-weight", "0.5"]) == 0
    assert rows() == rec.recommend(QUERIES[0], 5, like=[a, b], unlike={c: 0.75}, like_weight=2.0, query_weight=0.5)
    assert cli.main(["--config", str(cfg), "--json", "--unlike", a, "--unlike-weight", "1"]) == 0
    assert rows() == rec.recommend(QUERIES[0], 5, unlike=[a], unlike_weight=1.0)
    for argv, text in ((["--similar-to", a, "--query", "milk"], "cannot be combined with --query"),
                       (["--similar-to", a, "--like", b], "cannot be combined with --like"),
                       (["--similar-to", "no-such-product"], "no such product"), (["--like", f"{a}=x"], "not a weight"),
                       (["--like", a, "--like", f"{b}=1"], "every product its =W or none"), (["--like", a, "--like", a], "twice"),
                       (["--like", a, "--unlike", a], "in both like and unlike"), (["--like", f"{a}=-1"], ">= 0")):
        with pytest.raises(SystemExit, match=text):
            cli.main(["--config", str(cfg)] + argv)
