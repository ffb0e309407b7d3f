"""The plan of every tracking / multi-hand scenario of tests/helpers/step_plan.py on the CPU interpreter: the profile rows in order, the
counter deltas and the bytes of every output equal what the library gave before the step functions were rebuilt from shared helpers
(tests/golden/step_plan.json, section "emu").  The interpreter needs about a minute per slot and step, so only the two cheapest scenarios
run by default; the others are marked slow and run with HP3D_SLOW=1.  tests/test_gpu_step_plan.py runs all of them on the GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import step_plan as SP      # noqa: E402

skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="a minute per slot and step on the CPU interpreter; set HP3D_SLOW=1")


@pytest.fixture(scope='module')
def plan_engine(emu_engine):
    e = SP.plan_engine(emu_engine.lib._name)
    yield e
    e.close()


@pytest.fixture(scope='module')
def expected():
    return SP.expected('emu')


def check(e, expected, name):
    got = SP.run(e, name)
    want = expected[name]
    assert got['rows'] == want['rows']
    assert got['counters'] == want['counters']
    assert got['digests'] == want['digests']


def test_the_fixture_covers_every_scenario(expected):
    assert sorted(expected) == sorted(SP.SCENARIOS) and set(SP.CHEAPEST) <= set(SP.SCENARIOS)


@pytest.mark.parametrize("name", SP.CHEAPEST)
def test_step_plan_is_the_recorded_one(plan_engine, expected, name):
    check(plan_engine, expected, name)


@pytest.mark.slow
@skip_unless_slow
@pytest.mark.parametrize("name", [n for n in SP.SCENARIOS if n not in SP.CHEAPEST])
def test_step_plan_is_the_recorded_one_slow(plan_engine, expected, name):
    check(plan_engine, expected, name)
