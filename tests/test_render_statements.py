"""The render tests' float32 numpy statements, held to what they computed before they were folded onto
tests/chain_ref.py: tests/golden/render_statements.json was recorded by tests/golden/make_render_statements.py with the
modules of the commit BEFORE that change; the same maker, unchanged, recomputes every call with the current modules.  The
file holds one sha256 per group of calls (a family on one shape and one field); the maker's --calls gives the hash of
every call, to find the one that moved.  No GPU, no library call.  A change of the chain or of the tail that is meant to
change bits records the file anew and says so."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recorded():
    spec = importlib.util.spec_from_file_location("make_render_statements", os.path.join(GOLDEN, "make_render_statements.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    calls, nans = maker.record()
    return maker.groups(calls), nans


def test_every_call_gives_the_recorded_bits(recorded):
    want = json.load(open(os.path.join(GOLDEN, "render_statements.json")))
    got, _ = recorded
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:20]
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, (len(differ), differ[:20])


def test_the_nan_field_leaves_nans_in_what_is_hashed(recorded):
    """so that the one-pattern-for-every-NaN step of the hash is exercised"""
    assert recorded[1] >= 1
