"""HTTP surface of the reference's /recommend service, served by the MI355X recommender.

Mirrors src/api/{main,schemas,metrics,auth}.py and src/api/routes/{recommend,corpus}.py of the
reference for the hot path only; feedback storage and rate limiting are out of scope.
"""

DEFAULT_MODEL_DIR = "models/two_tower_sbert/final"  # MODEL_DIR
DEFAULT_CORPUS_PATH = "processed/p5_mp20_ef0.1/eval_corpus.json"  # CORPUS_PATH
