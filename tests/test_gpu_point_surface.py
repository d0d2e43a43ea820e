"""What the point types do through the kernels against tests/golden/point_surface_gpu.json, which tools/record_point_surface.py --gpu
wrote at the commit before curve.py got its common base classes: the smallest inputs that take each branch of the Python dispatch
(the kernels themselves have their own tests).  The file is never regenerated; a difference is a change of behaviour."""
import pytest

from test_point_surface_cpu import compare, rps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return rps.load("gpu")


def test_record_covers_every_variant(recorded):
    assert sorted(recorded) == sorted(rps.UNIQUE)


@pytest.mark.parametrize("name", rps.UNIQUE)
def test_variant(recorded, name):
    compare(recorded[name], name, rps.gpu_variant(name))
