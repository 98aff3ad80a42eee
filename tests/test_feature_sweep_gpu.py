"""The seeded parity sweep over combined request features and index edits (tools/fuzz_features.py over
tests/feature_cases.py), one run per request kind with the committed seed and counts: every run draws the same cases,
and a failure names its kind.  The tool takes a case count and a seed for longer soaks, --case I to repeat one case."""
from __future__ import annotations

import subprocess
import sys
from pathlib import Path

import pytest

from tests.feature_cases import COUNTS, KINDS, SEED

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("kind", KINDS)
def test_feature_parity(kind):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz_features.py"), str(COUNTS[kind]), str(SEED), "--kind", kind],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{COUNTS[kind] // len(KINDS)} cases, 0 mismatches" in r.stdout, r.stdout[-3000:]
