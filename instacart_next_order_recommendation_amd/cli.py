"""Command-line front of the recommender: one query in, the ranked products out.

Takes the YAML file the reference's `python -m src.inference` takes (configs/inference.yaml; keys model_dir, corpus,
use_index, query, eval_query_id, top_k — the drop-in contract, serve_recommendations.py:296-340) so an existing
deployment's config keeps working, but it is a different tool: the query can also come from the command line, the
output is either a table or one JSON object per result, and nothing is fetched from a hub (`corpus_hf_repo*` keys are
ignored; a missing model directory or corpus file is an error).

    python -m instacart_next_order_recommendation_amd --config configs/inference.yaml [--query "..."] [--json]
                                                      [--aisle NAME]... [--department NAME]...
                                                      [--diversity FLOAT] [--candidates INT]
                                                      [--ann-lists N --probes P]
                                                      [--boost PID[=W]]... [--boost-weight W] [--only-boosted]
                                                      [--product-sets FILE --within NAME]...
                                                      [--max-per-aisle N] [--max-per-department N]
                                                      [--cf-data-dir DIR --cf-processed-dir DIR --history PID...
                                                       [--cf-weight W] [--rrf-c C]]
                                                      [--adapter FILE]

`--adapter FILE` (or the optional `adapter_path` key of the config) puts a learned query adapter (adapter.py) behind the
encoder.  `fit-adapter` as the first argument learns one from (context, product) pairs - lines of
{"anchor": text, "positive": product_id} - against the catalog's stored rows and writes it to --out:

    python -m instacart_next_order_recommendation_amd fit-adapter --config configs/inference.yaml --pairs FILE.jsonl
                                                                  --out FILE [--epochs N] [--batch-size B]
                                                                  [--negatives M|all] [--lr LR] [--weight-decay WD]
                                                                  [--scale S] [--seed N]

With `--lists FILE.jsonl [--gain EVENT=G ...]` in place of `--pairs` it learns from impression lists - lines of
{"anchor": text, "products": {product_id: event name or gain, ...}}, what was shown for a context and what happened to
each product - with the listwise loss (Recommender.fit_adapter_lists; impression=0 click=1 add_to_cart=2 purchase=4).

`baselines` as the first argument runs the reference's `python -m src.baselines.run_baselines` instead: the content-based
and the item-item CF baseline over a processed directory, eight IR metrics each (configs/baselines.yaml; keys
processed_dir, data_dir, model_name, content_only, cf_only).

    python -m instacart_next_order_recommendation_amd baselines --config configs/baselines.yaml [--cf-only]
                                                                [--reorder-boost W]
                                                                [--hybrid [--cf-weight W] [--rrf-c C]]
                                                                [--adapter FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import yaml

_DEFAULTS = {"model_dir": "models/two_tower_sbert/final", "corpus": "processed/p5_mp20_ef0.1/eval_corpus.json",
             "use_index": True, "query": None, "eval_query_id": None, "top_k": 10, "adapter_path": None}
_FALLBACK_QUERY = "[+7d w4h14] Organic Milk, Whole Wheat Bread."  # the reference's demo context


def read_settings(path: Path | None) -> dict:
    """YAML -> settings dict with the reference's defaults filled in; unknown keys are dropped."""
    raw = yaml.safe_load(Path(path or "configs/inference.yaml").read_text()) or {}
    cfg = {key: (raw[key] if raw.get(key) is not None else default) for key, default in _DEFAULTS.items()}
    cfg["model_dir"], cfg["corpus"] = Path(str(cfg["model_dir"])), Path(str(cfg["corpus"]))
    cfg["top_k"], cfg["use_index"] = int(cfg["top_k"]), bool(cfg["use_index"])
    cfg["adapter_path"] = Path(str(cfg["adapter_path"])) if cfg["adapter_path"] else None
    return cfg


def adapter_file(cfg: dict, override: Path | None) -> Path | None:
    """The adapter file of a run: --adapter beats the config's adapter_path; None: no adapter.  A file that does not
    exist ends the run."""
    path = override or cfg["adapter_path"]
    if path is not None and not Path(path).exists():
        raise SystemExit(f"adapter file {path} does not exist")
    return path


def read_pairs(path: Path) -> list[tuple[str, str]]:
    """A .jsonl of {"anchor": context text, "positive": product id} -> [(text, id)]; blank lines are skipped.  ValueError
    names the first line that is not such an object."""
    pairs = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        if not line.strip():
            continue
        try:
            row = json.loads(line)
            pairs.append((row["anchor"], str(row["positive"])))
        except (ValueError, KeyError, TypeError):
            raise ValueError(f"{path}:{n}: not a {{\"anchor\": ..., \"positive\": ...}} object")
        if not isinstance(pairs[-1][0], str):
            raise ValueError(f"{path}:{n}: the anchor must be a string")
    return pairs


def read_lists(path: Path) -> tuple[list[tuple[str, dict]], list[str]]:
    """A .jsonl of {"anchor": context text, "products": {product id: event name or gain}} -> ([(text, products)], what
    names each of them in a message: "FILE:line"); blank lines are skipped.  ValueError names the first line that is not
    such an object."""
    lists, where = [], []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        if not line.strip():
            continue
        try:
            row = json.loads(line)
            anchor, products = row["anchor"], row["products"]
        except (ValueError, KeyError, TypeError):
            raise ValueError(f"{path}:{n}: not a {{\"anchor\": ..., \"products\": {{...}}}} object")
        if not isinstance(anchor, str):
            raise ValueError(f"{path}:{n}: the anchor must be a string")
        if not isinstance(products, dict):
            raise ValueError(f"{path}:{n}: products must be an object of product id -> event name or gain")
        lists.append((anchor, {str(pid): v for pid, v in products.items()}))
        where.append(f"{path}:{n}")
    return lists, where


def gain_args(entries, defaults: dict) -> dict:
    """--gain EVENT=G ...: `defaults` with the named events' gains replaced or added.  ValueError: an entry that is not
    EVENT=number."""
    gains = dict(defaults)
    for entry in entries or []:
        event, sep, value = entry.partition("=")
        try:
            gains[event] = float(value)
        except ValueError:
            sep = ""
        if not sep or not event:
            raise ValueError(f"--gain takes EVENT=number, got {entry!r}")
    return gains


def negatives_arg(text: str):
    """--negatives: an integer, or 'all' (QueryAdapter.fit's negatives="all")."""
    return "all" if text == "all" else int(text)


def fit_adapter_main(argv) -> int:
    ap = argparse.ArgumentParser(prog="instacart_next_order_recommendation_amd fit-adapter",
                                 description="Learn a query adapter from (context, product) pairs on the GPU.")
    ap.add_argument("--config", type=Path, default=None, help="YAML settings (default: configs/inference.yaml): model_dir, corpus")
    ap.add_argument("--pairs", type=Path, default=None, metavar="FILE.jsonl",
                    help='lines of {"anchor": context text, "positive": product_id}')
    ap.add_argument("--lists", type=Path, default=None, metavar="FILE.jsonl",
                    help='instead of --pairs: impression lists, lines of {"anchor": context text, "products": {product_id: '
                         'event name or gain}}, trained with the listwise loss')
    ap.add_argument("--gain", action="append", default=None, metavar="EVENT=G",
                    help="with --lists: the gain of an event (default: impression=0 click=1 add_to_cart=2 purchase=4)")
    ap.add_argument("--out", type=Path, required=True, metavar="FILE", help="where the adapter is written (.npz)")
    ap.add_argument("--adapter", type=Path, default=None, metavar="FILE", help="an adapter to train further")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--negatives", type=negatives_arg, default=0, metavar="M|all",
                    help="extra catalog rows drawn per step beside the in-batch negatives; 'all': every step is the exact "
                         "cross-entropy against the whole catalog, nothing is drawn")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--weight-decay", type=float, default=0.01)
    ap.add_argument("--scale", type=float, default=30.0, help="the loss scale (the reference trains with 30)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if (args.pairs is None) == (args.lists is None):
        ap.error("exactly one of --pairs and --lists must be given")
    if args.gain and args.lists is None:
        ap.error("--gain goes with --lists")
    cfg = read_settings(args.config)
    if not cfg["corpus"].exists():
        raise SystemExit(f"corpus file {cfg['corpus']} does not exist (this build never downloads one)")
    source = args.pairs if args.lists is None else args.lists
    if not source.exists():
        raise SystemExit(f"{'pairs' if args.lists is None else 'lists'} file {source} does not exist")
    start = adapter_file(cfg, args.adapter)
    try:
        if args.lists is None:
            pairs = read_pairs(args.pairs)
        else:
            from .recommender import DEFAULT_GAINS

            gains = gain_args(args.gain, DEFAULT_GAINS)
            pairs, where = read_lists(args.lists)
    except ValueError as e:
        raise SystemExit(str(e))

    from .recommender import Recommender

    rec = Recommender(model_dir=cfg["model_dir"], corpus_path=cfg["corpus"], use_index=cfg["use_index"], adapter=start)
    try:
        if args.lists is None:
            losses = rec.fit_adapter(pairs, epochs=args.epochs, batch_size=args.batch_size, negatives=args.negatives,
                                     lr=args.lr, weight_decay=args.weight_decay, scale=args.scale, seed=args.seed)
        else:
            losses = rec.fit_adapter_lists(pairs, gains, epochs=args.epochs, batch_size=args.batch_size, lr=args.lr,
                                           weight_decay=args.weight_decay, scale=args.scale, seed=args.seed, where=where)
    except ValueError as e:
        raise SystemExit(str(e))
    rec._adapter.save(args.out)
    print(f"{len(pairs)} {'pairs' if args.lists is None else 'lists'}, {len(losses)} steps: loss {losses[0]:.4f} -> "
          f"{losses[-1]:.4f}; adapter written to {args.out}")
    return 0


def pick_query(cfg: dict, override: str | None) -> tuple[str, str]:
    """(query text, where it came from): --query beats eval_query_id beats `query` beats the demo context."""
    if override:
        return override, "command line"
    if cfg["eval_query_id"]:
        table = json.loads((cfg["corpus"].parent / "eval_queries.json").read_text())
        try:
            return table[cfg["eval_query_id"]], f"eval_queries.json[{cfg['eval_query_id']}]"
        except KeyError:
            raise SystemExit(f"eval_query_id {cfg['eval_query_id']!r} is not in {cfg['corpus'].parent / 'eval_queries.json'}")
    if cfg["query"]:
        return str(cfg["query"]), "config"
    return _FALLBACK_QUERY, "built-in demo context"


_BASELINE_DEFAULTS = {"processed_dir": "processed/p5_mp20_ef0.1", "data_dir": "data",
                      "model_name": "sentence-transformers/all-MiniLM-L6-v2", "content_only": False, "cf_only": False}


def print_metrics(name: str, metrics: dict) -> None:
    """The reference's eight lines per baseline (run_baselines.py:32-42)."""
    print(f"\n--- {name} ---")
    for label, key in (("Accuracy@1:  ", "accuracy_at_1"), ("Accuracy@3:  ", "accuracy_at_3"), ("Accuracy@5:  ", "accuracy_at_5"),
                       ("Accuracy@10: ", "accuracy_at_10"), ("Recall@10:   ", "recall_at_10"), ("MRR@10:      ", "mrr_at_10"),
                       ("NDCG@10:     ", "ndcg_at_10"), ("MAP@100:     ", "map_at_100")):
        print(f"  {label} {metrics[key]:.4f}")


def baselines_main(argv) -> int:
    ap = argparse.ArgumentParser(prog="instacart_next_order_recommendation_amd baselines",
                                 description="Content-based and item-item CF baselines: eight IR metrics each.")
    ap.add_argument("--config", type=Path, default=None, help="YAML settings (default: configs/baselines.yaml if it exists)")
    ap.add_argument("--processed-dir", type=Path, default=None, help="overrides processed_dir of the config")
    ap.add_argument("--data-dir", type=Path, default=None, help="overrides data_dir of the config (orders.csv, order_products__prior.csv)")
    ap.add_argument("--model-name", type=Path, default=None, help="overrides model_name: a LOCAL SentenceTransformer directory")
    ap.add_argument("--content-only", action="store_true", help="only the content-based baseline")
    ap.add_argument("--cf-only", action="store_true", help="only the collaborative-filtering baseline")
    ap.add_argument("--reorder-boost", type=float, default=None, metavar="W",
                    help="a third block: the content-based ranking with W added to the scores of the products of the "
                         "user's earlier orders (the histories the CF baseline reads)")
    ap.add_argument("--hybrid", action="store_true",
                    help="a further block: the content-based and the CF ranking fused by position on the GPU (reciprocal "
                         "rank fusion); needs both baselines")
    ap.add_argument("--cf-weight", type=float, default=1.0, metavar="W", help="--hybrid: the weight of the CF list (default 1)")
    ap.add_argument("--rrf-c", type=float, default=60.0, metavar="C", help="--hybrid: the constant of 1 / (C + rank) (default 60)")
    ap.add_argument("--adapter", type=Path, default=None, metavar="FILE",
                    help="a further block: the content-based ranking with this query adapter behind the encoder")
    args = ap.parse_args(argv)
    path = args.config or (Path("configs/baselines.yaml") if Path("configs/baselines.yaml").exists() else None)
    raw = (yaml.safe_load(Path(path).read_text()) or {}) if path else {}
    cfg = {key: (raw[key] if raw.get(key) is not None else default) for key, default in _BASELINE_DEFAULTS.items()}
    processed_dir = Path(args.processed_dir or str(cfg["processed_dir"]))
    data_dir = Path(args.data_dir or str(cfg["data_dir"]))
    model_name = Path(args.model_name or str(cfg["model_name"]))
    content_only, cf_only = args.content_only or bool(cfg["content_only"]), args.cf_only or bool(cfg["cf_only"])
    if args.hybrid and (content_only or cf_only):
        raise SystemExit("--hybrid fuses the two baselines: it cannot be combined with --content-only or --cf-only")
    if args.hybrid and not (args.cf_weight >= 0.0 and -1.0 < args.rrf_c < float("inf")):
        raise SystemExit("--cf-weight takes a weight >= 0 and --rrf-c a finite constant > -1")
    if not (processed_dir / "eval_queries.json").exists():
        raise SystemExit(f"{processed_dir} holds no eval_queries.json (this build never downloads one)")
    if args.reorder_boost is not None and (cf_only or not args.reorder_boost >= 0.0):
        raise SystemExit("--reorder-boost takes a weight >= 0 and needs the content-based baseline (not --cf-only)")
    if args.adapter is not None and (cf_only or not args.adapter.exists()):
        raise SystemExit("--adapter takes an existing adapter file and needs the content-based baseline (not --cf-only)")

    from .baselines import ContentBasedBaseline, HybridBaseline, ItemItemCFBaseline
    from .ir_metrics import load_eval_data

    eval_queries, eval_corpus, relevant = load_eval_data(processed_dir)
    print(f"Processed dir: {processed_dir}\nEval queries: {len(eval_queries)}, corpus size: {len(eval_corpus)}")
    if not cf_only:
        if not model_name.is_dir():
            raise SystemExit(f"model_name {model_name} is not a local model directory (nothing is fetched from a hub)")
        cb = ContentBasedBaseline(eval_queries, eval_corpus, model_name=model_name)
        print_metrics("Content-based (untrained SBERT)", cb.evaluate(relevant))
        if args.adapter is not None:
            from .adapter import QueryAdapter

            cb.adapter = QueryAdapter.load(args.adapter, cb.device)
            print_metrics(f"Content-based + query adapter ({args.adapter.name})", cb.evaluate(relevant))
            cb.adapter = None
    if not content_only:
        cf = ItemItemCFBaseline(data_dir, processed_dir)
        print_metrics("Collaborative filtering (item-item)", cf.evaluate(relevant))
    if args.reorder_boost is not None:
        histories = cf.eval_order_to_history if not content_only else ItemItemCFBaseline.load_arrays(data_dir, processed_dir)["histories"]
        print_metrics(f"Content-based + reorder boost ({args.reorder_boost:g})",
                      cb.evaluate(relevant, boosts=histories, boost_weight=args.reorder_boost))
    if args.hybrid:
        hybrid = HybridBaseline(cb, cf, cf_weight=args.cf_weight, rrf_c=args.rrf_c)
        print_metrics(f"Hybrid (rank fusion, cf weight {args.cf_weight:g}, c {args.rrf_c:g})", hybrid.evaluate(relevant))
    return 0


def parse_boosts(entries, flag: str = "--boost"):
    """The --boost PID[=W] arguments (or another flag's of that form) -> (mapping PID -> W or None for an entry without
    a weight); ValueError for a W that is not a number."""
    out = {}
    for e in entries or ():
        pid, eq, w = e.rpartition("=")
        if not eq:
            out[e] = None
            continue
        try:
            out[pid] = float(w)
        except ValueError:
            raise ValueError(f"{flag} {e!r}: {w!r} is not a weight")
    return out


def parse_feedback(entries, flag: str):
    """The --like / --unlike PID[=W] arguments -> None (none given), the list of ids when no entry has a weight (they
    share --like-weight / --unlike-weight), or the mapping PID -> W when every entry has one; ValueError for a W that
    is not a number, an id given twice, and a mix of entries with and without =W."""
    if not entries:
        return None
    pairs = parse_boosts(entries, flag)
    if len(pairs) != len(entries):
        raise ValueError(f"{flag}: a product id is given twice")
    weighted = [w is not None for w in pairs.values()]
    if any(weighted) and not all(weighted):
        raise ValueError(f"{flag}: give every product its =W or none (they then share {flag}-weight)")
    return pairs if all(weighted) else list(pairs)


def build_parser() -> argparse.ArgumentParser:
    """The recommend command's arguments."""
    ap = argparse.ArgumentParser(prog="instacart_next_order_recommendation_amd", description=__doc__.splitlines()[0])
    ap.add_argument("--config", type=Path, default=None, help="YAML settings (default: configs/inference.yaml)")
    ap.add_argument("--query", default=None, help="user context to rank for (overrides the config)")
    ap.add_argument("--top-k", type=int, default=None, help="overrides top_k of the config")
    ap.add_argument("--json", action="store_true", help="one JSON object per result instead of the table")
    ap.add_argument("--aisle", action="append", default=None, metavar="NAME",
                    help="only products of this aisle (repeatable: any of the named aisles)")
    ap.add_argument("--department", action="append", default=None, metavar="NAME",
                    help="only products of this department (repeatable: any of the named departments)")
    ap.add_argument("--diversity", type=float, default=None, metavar="FLOAT",
                    help="0..1: re-select the results for diversity (Maximal Marginal Relevance, lambda = 1 - FLOAT); "
                         "they are then listed in selection order, not by score")
    ap.add_argument("--candidates", type=int, default=None, metavar="INT",
                    help="how many best matches a diversified request chooses from (default min(128, 4 * top_k))")
    ap.add_argument("--ann-lists", type=int, default=None, metavar="N",
                    help="build an IVF index of N lists beside the exact one (k-means on the catalog at start-up)")
    ap.add_argument("--probes", type=int, default=None, metavar="P",
                    help="search only the P best of the --ann-lists lists (approximate; P = N is the exact result)")
    ap.add_argument("--boost", action="append", default=None, metavar="PID[=W]",
                    help="a product the user has bought before: W (>= 0) is added to its score (repeatable; without =W "
                         "it takes --boost-weight)")
    ap.add_argument("--boost-weight", type=float, default=None, metavar="W", help="the weight of every --boost without its own")
    ap.add_argument("--only-boosted", action="store_true", help="rank the --boost products alone (buy it again)")
    ap.add_argument("--product-sets", type=Path, default=None, metavar="FILE",
                    help="JSON file {set name: [product id, ...]}: named product sets (store assortments, in stock, ...)")
    ap.add_argument("--within", action="append", default=None, metavar="NAME",
                    help="only products of this --product-sets set (repeatable, up to 4: products in every named set)")
    ap.add_argument("--max-per-aisle", type=int, default=None, metavar="N",
                    help="at most N results of one aisle (the best N of it, in the ranking's order)")
    ap.add_argument("--max-per-department", type=int, default=None, metavar="N",
                    help="at most N results of one department")
    ap.add_argument("--cf-data-dir", type=Path, default=None, metavar="DIR",
                    help="with --cf-processed-dir: build the item-item CF baseline from DIR's orders.csv and "
                         "order_products__prior.csv, for --history")
    ap.add_argument("--cf-processed-dir", type=Path, default=None, metavar="DIR",
                    help="the processed directory of the CF baseline; its eval_corpus.json must list the corpus' products")
    ap.add_argument("--history", action="append", default=None, metavar="PID",
                    help="a product of the user's earlier orders (repeatable): the results are the content ranking fused "
                         "with the CF ranking of these products; the scores are then fused scores")
    ap.add_argument("--cf-weight", type=float, default=1.0, metavar="W", help="the weight of the CF list in the fusion (default 1)")
    ap.add_argument("--rrf-c", type=float, default=60.0, metavar="C", help="the constant of 1 / (C + rank) in the fusion (default 60)")
    ap.add_argument("--like", action="append", default=None, metavar="PID[=W]",
                    help="a product the user accepted: the query vector moves toward it (repeatable; without =W the "
                         "products share --like-weight)")
    ap.add_argument("--unlike", action="append", default=None, metavar="PID[=W]",
                    help="a product the user dismissed: the query vector moves away from it (repeatable; without =W the "
                         "products share --unlike-weight)")
    ap.add_argument("--query-weight", type=float, default=1.0, metavar="A", help="the weight of the text's vector (default 1)")
    ap.add_argument("--like-weight", type=float, default=1.0, metavar="B", help="the weight of the --like centroid (default 1)")
    ap.add_argument("--unlike-weight", type=float, default=0.5, metavar="C", help="the weight of the --unlike centroid (default 0.5)")
    ap.add_argument("--adapter", type=Path, default=None, metavar="FILE",
                    help="a learned query adapter (fit-adapter) behind the encoder; overrides adapter_path of the config")
    ap.add_argument("--similar-to", default=None, metavar="PID",
                    help="similar items: rank by similarity with this catalog product instead of a text (not with --query, "
                         "--like, --unlike); the product itself is left out")
    return ap


def fusion_args(args) -> bool:
    """The --cf-* / --history arguments checked against each other and the rest: the two directories go together,
    --history needs them, and a fused request takes --top-k and --candidates only.  -> whether a CF baseline is built."""
    if (args.cf_data_dir is None) != (args.cf_processed_dir is None):
        raise SystemExit("--cf-data-dir and --cf-processed-dir go together")
    if args.history and args.cf_data_dir is None:
        raise SystemExit("--history needs --cf-data-dir and --cf-processed-dir")
    if args.history:
        for flag, given in (("--aisle", args.aisle), ("--department", args.department), ("--diversity", args.diversity),
                            ("--probes", args.probes), ("--boost", args.boost), ("--only-boosted", args.only_boosted),
                            ("--within", args.within), ("--max-per-aisle", args.max_per_aisle),
                            ("--max-per-department", args.max_per_department)):
            if given:
                raise SystemExit(f"--history cannot be combined with {flag}: the CF list is the best of the whole catalog "
                                 "and knows none of these constraints")
    return args.cf_data_dir is not None


def ann_args(args) -> tuple[int | None, int | None]:
    """(--ann-lists, --probes) checked against each other: each needs the other, both are >= 1, P <= N."""
    n, p = args.ann_lists, args.probes
    if (n is None) != (p is None):
        raise SystemExit("--ann-lists and --probes go together")
    if n is not None and not 1 <= p <= n:
        raise SystemExit(f"--probes must be in [1, --ann-lists = {n}], got {p}")
    return n, p


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "baselines":
        return baselines_main(argv[1:])
    if argv and argv[0] == "fit-adapter":
        return fit_adapter_main(argv[1:])
    args = build_parser().parse_args(argv)
    ann_lists, probes = ann_args(args)
    with_cf = fusion_args(args)
    if args.within and args.product_sets is None:
        raise SystemExit("--within needs --product-sets")
    if args.product_sets is not None and not args.product_sets.exists():
        raise SystemExit(f"product sets file {args.product_sets} does not exist")
    if args.similar_to is not None:
        for flag, given in (("--query", args.query), ("--like", args.like), ("--unlike", args.unlike)):
            if given:
                raise SystemExit(f"--similar-to cannot be combined with {flag}: the product is the whole query")
    try:
        like, unlike = parse_feedback(args.like, "--like"), parse_feedback(args.unlike, "--unlike")
    except ValueError as e:
        raise SystemExit(str(e))
    cfg = read_settings(args.config)
    if not cfg["corpus"].exists():
        raise SystemExit(f"corpus file {cfg['corpus']} does not exist (this build never downloads one)")
    query, origin = pick_query(cfg, args.query)
    adapter = adapter_file(cfg, args.adapter)
    top_k = args.top_k or cfg["top_k"]
    try:
        boosts = parse_boosts(args.boost)
    except ValueError as e:
        raise SystemExit(str(e))
    if any(w is None for w in boosts.values()):
        if args.boost_weight is None:
            raise SystemExit("--boost without =W needs --boost-weight")
        boosts = {pid: args.boost_weight if w is None else w for pid, w in boosts.items()}

    from .recommender import Recommender, load_product_sets

    try:
        product_sets = load_product_sets(args.product_sets) if args.product_sets is not None else None
    except ValueError as e:  # (a file that is not JSON raises json.JSONDecodeError, a ValueError too)
        raise SystemExit(f"--product-sets {args.product_sets}: {e}")
    cf = None
    if with_cf:
        from .baselines import ItemItemCFBaseline

        cf = ItemItemCFBaseline(args.cf_data_dir, args.cf_processed_dir)
    try:
        rec = Recommender(model_dir=cfg["model_dir"], corpus_path=cfg["corpus"], use_index=cfg["use_index"],
                          ann_lists=ann_lists, product_sets=product_sets, cf=cf, adapter=adapter)
    except ValueError as e:  # the CF baseline's corpus is not the catalog; an adapter file of another width
        raise SystemExit(str(e))
    options = dict(aisles=args.aisle, departments=args.department, diversity=args.diversity, candidates=args.candidates,
                   boosts=boosts or None, only_boosted=args.only_boosted, probes=probes, within=args.within,
                   max_per_aisle=args.max_per_aisle, max_per_department=args.max_per_department, history=args.history,
                   cf_weight=args.cf_weight, rrf_c=args.rrf_c)
    try:
        if args.similar_to is not None:
            query, origin = f"products similar to {args.similar_to}", "--similar-to"
            hits = rec.similar_products(args.similar_to, top_k, **options)
        else:
            hits = rec.recommend(query=query, top_k=top_k, like=like, unlike=unlike, query_weight=args.query_weight,
                                 like_weight=args.like_weight, unlike_weight=args.unlike_weight, **options)
    except KeyError:
        raise SystemExit(f"--similar-to {args.similar_to!r}: the catalog has no such product")
    except ValueError as e:  # an aisle / department / product set the catalog does not have, a bad --diversity / --candidates / --boost / --probes / --max-per-*
        raise SystemExit(str(e))
    if args.json:
        for rank, (pid, score) in enumerate(hits, 1):
            print(json.dumps({"rank": rank, "product_id": pid, "score": score, "product_text": rec.pid_to_text[pid]}))
        return 0
    shown = query if len(query) <= 200 else query[:200] + " ..."
    print(f"context ({origin}): {shown}")
    width = max((len(pid) for pid, _ in hits), default=1)
    for rank, (pid, score) in enumerate(hits, 1):
        print(f"{rank:>3}  {pid:>{width}}  {score:7.4f}  {rec.pid_to_text[pid]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
