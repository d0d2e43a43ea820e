"""The single-launch C entry points against tests/golden/entry_surface_gpu.json: which refusal each gives, in which order of checks,
what an accepted call returns and under which launch names, and nothing else launched.  The file was recorded by
tools/record_entry_surface.py on the library of the commit before these entry points got one host round trip; the case table
(tests/entry_surface_cases.py) is replayed here once and compared entry by entry.  Every comparison is exact."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_surface_cases as cases  # noqa: E402

from dot_ring_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay():
    return cases.run_all(_native.lib(), cases.table())[0]


def test_table_and_file_have_the_same_keys():
    golden = cases.load_golden()
    assert sorted(golden) == sorted(c.key for c in cases.table())


def test_every_entry_point_is_covered():
    golden, table = cases.load_golden(), cases.table()
    for fn in cases.COVERED:
        mine = [golden[c.key] for c in table if c.fn == fn and c.key in golden]
        assert any(r["rc"] == 0 and ("out" in r or "launches" in r) for r in mine), f"{fn}: no accepted entry"
        assert any(r["rc"] != 0 for r in mine), f"{fn}: no refused entry"


def test_no_refusal_launches():
    golden = cases.load_golden()
    assert [k for k, r in golden.items() if r["rc"] != 0 and ("launches" in r or "out" in r) and k not in cases.REFUSED_AFTER_SW_TO_TE] == []
    # the four refusals of the SW boundary's inner call: after the map of the (valid) points to their TE images, and nothing else
    for k in cases.REFUSED_AFTER_SW_TO_TE:
        assert golden[k]["rc"] != 0 and golden[k]["launches"] == {"k_sw_to_te": 1} and "out" not in golden[k], k


def test_replay_equals_the_record(replay):
    golden = cases.load_golden()
    differing = {k: (replay.get(k), want) for k, want in golden.items() if replay.get(k) != want}
    assert not differing, f"{len(differing)} of {len(golden)} entries differ: " + "; ".join(f"{k}: {got} != {want}" for k, (got, want) in list(differing.items())[:8])
