"""CLS pooling without a GPU: the model-directory loader's pooling modes, and the references tests/test_cls_pooling_gpu.py
compares against (tests/cls_pooling.py, tests/token_states.py) - that the fp32 and the float64 reference agree as closely as their hidden
states say they must, and that on the GPU tests' inputs a CLS embedding is far enough from the mean embedding of the
same sequence for the GPU bound to tell the two apart."""
from __future__ import annotations

import json

import numpy as np
import pytest

from tests import cls_pooling as cp
from tests import token_states as ts

MODES = ("f32", "f16x3")


def _pooling_dir(tmp_path, name, **modes):
    """A synthetic model directory whose 1_Pooling/config.json has the given pooling_mode_* flags."""
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir

    d = write_synthetic_model_dir(tmp_path / name, seed=2)
    pc = d / "1_Pooling" / "config.json"
    base = {k: v for k, v in json.loads(pc.read_text()).items() if not k.startswith("pooling_mode_")}
    pc.write_text(json.dumps({**base, **{f"pooling_mode_{k}": v for k, v in modes.items()}}))
    return d


def test_loader_reports_the_pooling_mode(tmp_path):
    from instacart_next_order_recommendation_amd.model_io import load_model_dir, write_synthetic_model_dir

    cls_dir = write_synthetic_model_dir(tmp_path / "cls", seed=2, pooling="cls")
    cfg = json.loads((cls_dir / "1_Pooling" / "config.json").read_text())
    assert cfg["pooling_mode_cls_token"] is True and cfg["pooling_mode_mean_tokens"] is False
    m = load_model_dir(cls_dir)
    assert m.pooling == "cls"
    mean = load_model_dir(write_synthetic_model_dir(tmp_path / "mean", seed=2, pooling="mean"))
    assert mean.pooling == "mean" and load_model_dir(write_synthetic_model_dir(tmp_path / "default", seed=2)).pooling == "mean"
    # the mode changes nothing else about the loaded model
    np.testing.assert_array_equal(m.weights, mean.weights)
    assert m.shape == mean.shape and m.max_seq_length == mean.max_seq_length
    # what BGE's own config looks like: every flag spelled out, one of them true
    bge = _pooling_dir(tmp_path, "bge", cls_token=True, mean_tokens=False, max_tokens=False, mean_sqrt_len_tokens=False,
                       weightedmean_tokens=False, lasttoken=False)
    assert load_model_dir(bge).pooling == "cls"
    with pytest.raises(ValueError):
        write_synthetic_model_dir(tmp_path / "bad", pooling="max")


@pytest.mark.parametrize("modes", [
    dict(cls_token=False, mean_tokens=False, max_tokens=True),                  # max pooling
    dict(cls_token=True, mean_tokens=True, max_tokens=False),                   # cls + mean: output twice as wide
    dict(cls_token=False, mean_tokens=False, max_tokens=False),                 # no mode at all
    dict(cls_token=False, mean_tokens=False, mean_sqrt_len_tokens=True),
    dict(cls_token=False, mean_tokens=False, weightedmean_tokens=True),
    dict(cls_token=False, mean_tokens=False, lasttoken=True),
    dict(cls_token=True, mean_tokens=False, max_tokens=True),
], ids=["max", "cls+mean", "none", "mean_sqrt_len", "weightedmean", "lasttoken", "cls+max"])
def test_loader_refuses_other_pooling(tmp_path, modes):
    from instacart_next_order_recommendation_amd.model_io import load_model_dir

    with pytest.raises(ValueError) as e:
        load_model_dir(_pooling_dir(tmp_path, "m", **modes))
    assert "pooling_mode_" in str(e.value)  # the message carries the config


@pytest.mark.parametrize("batch", list(cp.BATCHES))
@pytest.mark.parametrize("hidden,layers", cp.SHAPES)
@pytest.mark.parametrize("kind", ts.KINDS)
def test_references_agree_and_cls_is_not_mean(kind, hidden, layers, batch):
    """The fp32 and float64 CLS references against each other, and the discrimination condition.

    Agreement.  A CLS embedding is a token row h scaled to unit length.  If the fp32 row is h + d, its normalised form
    differs from h / |h| by at most |d|_2 / |h|_2 to first order (the component of d along h drops out), and
    |d|_2 <= sqrt(H) x (the row's rms error); each fp32 normalisation adds at most 32 roundings of a component <= 1
    (tests/test_token_states_gpu.py counts them the same way).  So with E_rms the oracle's per-token-row rms error
    against float64 - the E_ref of tests/token_states.py's scheme - on this batch,
        max|cls32 - cls64| <= margin x sqrt(H) x E_rms / min|h|_2 + n_normalize x 32 x 2^-24,
    with the f32 margin of token_states.MARGINS (the oracle IS the f32 arithmetic).

    Discrimination.  For every sequence of two or more tokens the float64 CLS embedding and the float64 mean embedding
    are at least 100 x further apart (max abs) than the loosest max-abs bound a GPU result must meet in any mode: a
    library that silently mean-pooled could not pass."""
    r = cp.reference(kind, hidden, layers, batch)
    cu = r["cu"]
    first = cu[:-1].astype(np.int64)
    e_rms, _ = ts.row_errors(r["h32"], r["h64"])
    m_rms, _ = ts.MARGINS[("f32", hidden, kind)]
    h_norm = float(np.linalg.norm(r["h64"][first], axis=1).min())
    for n in cp.N_NORMALIZE:
        got = float(np.abs(r["cls32"][n].astype(np.float64) - r["cls64"][n]).max())
        limit = m_rms * np.sqrt(hidden) * e_rms / h_norm + n * 32 * 2.0 ** -24
        print(f"[{kind} {hidden}x{layers} {batch} n_normalize={n}] max|cls32 - cls64| = {got:.3e} (limit {limit:.3e})")
        assert 0 < got <= limit
        assert np.abs(np.linalg.norm(r["cls64"][n], axis=1) - 1).max() < 1e-12
        loosest = max(ts.MARGINS[(mode, hidden, kind)][1] for mode in MODES) * ts.row_errors(r["cls32"][n], r["cls64"][n])[1]
        many = np.flatnonzero(np.diff(cu) >= 2)
        assert many.size >= 3
        apart = np.abs(r["cls64"][n][many] - r["mean64"][n][many]).max(axis=1)
        print(f"    CLS vs mean, closest sequence: {apart.min():.3e} = {apart.min() / loosest:.0f} x the loosest bound {loosest:.3e}")
        assert apart.min() >= 100 * loosest, (kind, hidden, layers, batch, n, float(apart.min()), loosest)
    # a one-token sequence's CLS and mean embeddings are the same vector
    one = np.flatnonzero(np.diff(cu) == 1)
    for n in cp.N_NORMALIZE:
        assert np.abs(r["cls64"][n][one] - r["mean64"][n][one]).max(initial=0.0) < 1e-15
