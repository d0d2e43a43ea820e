"""The host side of every point type against tests/golden/point_surface_cpu.json, which tools/record_point_surface.py --cpu wrote at
the commit before curve.py got its common base classes: the tables are recomputed with the tool's own builders and compared entry by
entry.  The file is never regenerated; a difference is a change of behaviour."""
import importlib.util
import os

import pytest

_TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_point_surface.py")
_spec = importlib.util.spec_from_file_location("record_point_surface", _TOOL)
rps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rps)


def compare(want, name, tree):
    """the recorded entries of one variant against its table as it is now"""
    now, got = rps.entries(tree), rps.briefed(name, tree)
    bad = [f"{name}/{k}: recorded {want.get(k, '<absent>')}, now {got.get(k, '<absent>')} = {str(now.get(k))[:300]}"
           for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
    assert not bad, f"{len(bad)} of {len(want)} entries differ:\n" + "\n".join(bad[:20])


@pytest.fixture(scope="module")
def recorded():
    return rps.load("cpu")


def test_record_covers_every_variant(recorded):
    import dot_ring_amd as d

    assert len(rps.NAMES) == 28 and set(rps.NAMES) == {n for n in d.__all__ if hasattr(getattr(d, n), "point_type")}
    assert sorted(recorded) == sorted(rps.UNIQUE + ["cross"])
    for name, target in rps.ALIASES.items():
        assert getattr(d, name) is getattr(d, target)


@pytest.mark.parametrize("name", rps.UNIQUE)
def test_variant(recorded, name):
    compare(recorded[name], name, rps.cpu_variant(name))


def test_cross(recorded):
    compare(recorded["cross"], "cross", rps.cpu_cross())
