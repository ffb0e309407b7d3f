"""The plan of every tracking / multi-hand scenario of tests/helpers/step_plan.py on the GPU: the profile rows in order, the counter deltas
and the bytes of every output equal what the library gave before the step functions were rebuilt from shared helpers
(tests/golden/step_plan.json, section "gpu": recorded twice from that library, the two recordings identical)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import step_plan as SP      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def plan_engine():
    from hand3d_amd import _lib
    assert os.path.exists(_lib.DEFAULT_LIB), "libhp3d.so not built (python -m hand3d_amd.build)"
    e = SP.plan_engine(_lib.DEFAULT_LIB)
    yield e
    e.close()


@pytest.fixture(scope='module')
def expected():
    return SP.expected('gpu')


def test_the_fixture_covers_every_scenario(expected):
    assert sorted(expected) == sorted(SP.SCENARIOS)


@pytest.mark.parametrize("name", list(SP.SCENARIOS))
def test_step_plan_is_the_recorded_one(plan_engine, expected, name):
    got = SP.run(plan_engine, name)
    want = expected[name]
    assert got['rows'] == want['rows']
    assert got['counters'] == want['counters']
    assert got['digests'] == want['digests']
