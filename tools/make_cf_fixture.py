"""Regenerate tests/golden/cf_small/: tiny Instacart-shaped inputs, and what the UPSTREAM project's own
ItemItemCFBaseline.rank_all and compute_ir_metrics return on them.

    python tools/make_cf_fixture.py /path/to/instacart_next_order_recommendation [--out tests/golden/cf_small]

Needs the upstream checkout plus pandas and tqdm (its imports); run on a development machine only.  The tests read
the written files, never the checkout.  The inputs hold every edge the loader and the ranking have: a product twice in
one order, a user without a prior order, an eval query that orders.csv does not know, a prior product outside the
corpus, a corpus product nobody bought.
"""
from __future__ import annotations

import argparse
import csv
import json
import random
import sys
import types
from pathlib import Path


def write_inputs(out: Path, seed: int = 7) -> None:
    rng = random.Random(seed)
    data, processed = out / "data", out / "processed"
    data.mkdir(parents=True, exist_ok=True)
    processed.mkdir(parents=True, exist_ok=True)
    corpus_products = list(range(1, 61))          # 60 corpus products; 58, 59, 60 are bought by nobody
    bought = list(range(1, 58)) + [901, 902, 903, 904]  # 90x: prior products absent from the corpus
    weights = [1.0 / (i + 1) ** 0.7 for i in range(len(bought))]
    orders, prior_rows = [], []
    next_order = 1000
    eval_orders, other_train = [], []
    for user in range(1, 41):
        n_prior = 0 if user == 37 else rng.randint(3, 11)   # user 37 has no prior order
        for num in range(1, n_prior + 1):
            oid = next_order = next_order + 1
            orders.append((oid, user, "prior", num))
            size = rng.randint(1, 9)
            basket = []
            while len(basket) < size:
                p = rng.choices(bought, weights)[0]
                if p not in basket:
                    basket.append(p)
            if rng.random() < 0.15:                          # the same product twice in one order
                basket.insert(rng.randrange(len(basket) + 1), rng.choice(basket))
            for pos, p in enumerate(basket, 1):
                prior_rows.append((oid, p, pos, rng.randint(0, 1)))
        oid = next_order = next_order + 1
        # user 39's train order is numbered BELOW some of their prior orders: only the earlier ones are history
        orders.append((oid, user, "train", 3 if user == 39 else n_prior + 1))
        (eval_orders if user % 4 else other_train).append(oid)  # users 4, 8, ... have no eval order
    rng.shuffle(prior_rows)                                  # the real file is not grouped by user either
    with open(data / "orders.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["order_id", "user_id", "eval_set", "order_number", "order_dow", "order_hour_of_day", "days_since_prior_order"])
        for oid, user, es, num in orders:
            w.writerow([oid, user, es, num, rng.randint(0, 6), rng.randint(0, 23), "" if num == 1 else float(rng.randint(1, 30))])
    with open(data / "order_products__prior.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["order_id", "product_id", "add_to_cart_order", "reordered"])
        w.writerows(prior_rows)
    eval_ids = [str(o) for o in eval_orders] + ["999999"]    # 999999: an eval query that orders.csv does not know
    rng.shuffle(eval_ids)
    queries = {q: f"[+{rng.randint(1, 30)}d w{rng.randint(0, 6)}h{rng.randint(0, 23)}] context of order {q}" for q in eval_ids}
    order = corpus_products[:]
    rng.shuffle(order)                                       # corpus order is file order, not numeric order
    corpus = {str(p): f"Product {p}. Aisle: a{p % 7}. Department: d{p % 3}." for p in order}
    relevant = {q: sorted(str(p) for p in rng.sample(corpus_products, rng.randint(1, 6))) for q in eval_ids}
    relevant[eval_ids[3]] = []                               # a query with nothing relevant: not counted
    (processed / "eval_queries.json").write_text(json.dumps(queries, indent=0))
    (processed / "eval_corpus.json").write_text(json.dumps(corpus, indent=0))
    (processed / "eval_relevant_docs.json").write_text(json.dumps(relevant, indent=0))


def run_upstream(upstream: Path, out: Path) -> None:
    sys.path.insert(0, str(upstream))
    # src/baselines/__init__.py imports the content-based baseline (sentence-transformers); only the CF class and the
    # metrics are needed, so the package is entered without running its __init__
    pkg = types.ModuleType("src.baselines")
    pkg.__path__ = [str(upstream / "src" / "baselines")]
    sys.modules["src.baselines"] = pkg
    from src.baselines.collaborative_filtering import ItemItemCFBaseline, load_eval_data
    from src.baselines.metrics import compute_ir_metrics

    queries, _, relevant = load_eval_data(out / "processed")
    cf = ItemItemCFBaseline(out / "data", out / "processed")
    rankings = cf.rank_all(eval_query_ids=list(queries.keys()))
    recorded = {
        "rankings": rankings,
        "metrics": compute_ir_metrics(rankings, relevant),
        "histories": {q: sorted(h) for q, h in cf.eval_order_to_history.items()},
        "baskets": {str(o): pids for o, pids in cf.order_to_products.items()},
        "corpus_ids": cf.corpus_ids,
    }
    (out / "upstream.json").write_text(json.dumps(recorded, indent=0))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("upstream", type=Path, help="checkout of the upstream project")
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parents[1] / "tests" / "golden" / "cf_small")
    args = ap.parse_args()
    write_inputs(args.out)
    run_upstream(args.upstream.resolve(), args.out)
    print(f"wrote {args.out}: {sum(f.stat().st_size for f in args.out.rglob('*') if f.is_file())} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
