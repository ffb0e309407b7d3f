"""Option "track_hands_partial_detect"  through the real library, with the helpers the interpreter tests use
(tests/helpers/track_hands_partial_oracle.py): the index kernel and the positional select against NumPy bit for bit; detect steps of the
multi-hand tracker that run HandSegNet on the frames that lost a hand only -- rows, counters, the boxes of those frames against the
per-op chain on the gathered frames, the extended state machine, the composition of the back half, and slot by slot against the same
two steps on a second context with the option off; chunks; fresh and scheduled steps; hands_compact; the device-pointer and NV12
forms; half-precision trunks; the entry points that ignore the option."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import track_hands_partial_oracle as THP      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engines(gpu_engine, synth_weights):
    from hand3d_amd import _lib
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    off = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    off.load_weight_dict(synth_weights)
    off.finalize_weights(0)
    yield gpu_engine, off
    off.close()
    gpu_engine.track_hands_reset()


def test_option_values(gpu_engine):
    THP.assert_option_values(gpu_engine)


@pytest.mark.parametrize("nb,K", THP.INDEX_SHAPES)
def test_index_bit_exact(gpu_engine, nb, K):
    """(257, 1) and (600, 4): the scan crosses a 256 boundary with a non-zero running count."""
    THP.assert_index_exact(gpu_engine, nb, K)


@pytest.mark.parametrize("nb,K", [(1, 1), (7, 2), (300, 4)])
def test_select_pos_bit_exact(gpu_engine, nb, K):
    THP.assert_select_exact(gpu_engine, nb, K)


@pytest.mark.parametrize("B,K,H,W,lost,absent,kind,f", THP.STEP_CASES)
def test_partial_step(engines, B, K, H, W, lost, absent, kind, f):
    """(8, 2, 320, 320) reaches the filled-launch plan of the back half at 16 slots while HandSegNet runs the small-batch plan at m = 1:
    the case where 'a kept slot outside L is bit-equal to the option off' can break.
    Every output of a kept slot outside L is held to the option-off engine except `claimed`, which the rule itself sets to 0 for a frame
    that was not looked at while the whole-batch step counts the frame's claimed objects there (first case: on 0 0 0 0 0, off 1 0 1 2 0;
    last case: one slot of 13 reads 1 with the option off): `claimed` of those slots is held to the rule."""
    THP.assert_partial_step(engines[0], engines[1], B, K, H, W, lost, absent, kind, f)


def test_partial_step_chunks(engines):
    THP.assert_chunks(engines[0], engines[1])


def test_fresh_and_scheduled_steps_run_whole(engines):
    THP.assert_fresh_and_scheduled_whole(engines[0], engines[1])


def test_hands_compact_composes(engines):
    THP.assert_compact_composes(engines[0])


def test_dev_form_equals_host_form(engines):
    THP.assert_dev_form_equals_host_form(engines[0])


def test_nv12_form_equals_u8_form(engines):
    THP.assert_nv12_equals_u8(engines[0])


def test_half_precision_trunks(synth_weights):
    """(3, 2, 64, 64) on a half-precision context of its own: the boxes of L are the per-op chain's on the same context."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        res = THP.assert_partial_step(e, None, 3, 2, 64, 64, [(1, 0)], [(2, 1)], 'f32', 1, compare_off=False)
        assert not res['o2']['detected'][[0, 2]].any()
    finally:
        e.close()


def test_other_entry_points_ignore_the_option(engines):
    THP.assert_ignored_elsewhere(engines[0], 64, 64)
