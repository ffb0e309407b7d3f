"""Option "track_hands_partial_detect"  on the CPU interpreter: the option's values, the index kernel and the positional
select against their NumPy restatements bit for bit, and that the option leaves the per-op calls and the single-hand tracker's option
alone.  The step checks go through tests/helpers/track_hands_partial_oracle.py; the interpreter needs minutes per slot and step for
PoseNet2D, so they are marked slow and run with HP3D_SLOW=1 like tests/test_track_partial.py's; tests/test_gpu_track_hands_partial.py
runs the same helpers on the GPU at the issue's shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO                     # noqa: E402
import track_hands_oracle as TH               # noqa: E402
import track_hands_partial_oracle as THP      # noqa: E402

skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per slot and step on the CPU interpreter; set HP3D_SLOW=1")


def test_option_values(emu_engine):
    THP.assert_option_values(emu_engine)


@pytest.mark.parametrize("nb,K", THP.INDEX_SHAPES)
def test_index_bit_exact(emu_engine, nb, K):
    THP.assert_index_exact(emu_engine, nb, K)


@pytest.mark.parametrize("nb,K", [(1, 1), (7, 2), (300, 4)])
def test_select_pos_bit_exact(emu_engine, nb, K):
    THP.assert_select_exact(emu_engine, nb, K)


def test_per_op_argument_errors(emu_engine):
    e = emu_engine
    ones = np.ones((3, 2), np.int32)
    with pytest.raises(AssertionError, match="max hands"):
        e.track_hands_partial_index(np.ones((3, 5), np.int32), np.ones((3, 5), np.int32))
    det = {'center': np.zeros((1, 2, 2), np.float32), 'scale': np.ones((1, 2), np.float32), 'valid': ones[:1], 'area': ones[:1], 'claimed': ones[:1]}
    for bad in ([1, -1, -1], [-2, 0, -1]):          # no dense index of m = 1
        with pytest.raises(AssertionError, match="is no dense index"):
            e.track_hands_select_pos(bad, ones, det, np.zeros((3, 2, 2), np.float32), np.ones((3, 2), np.float32), ones)


def test_option_leaves_the_per_ops_and_the_other_option_alone(emu_engine):
    """The cheap part of 'ignored elsewhere': with the option on, the claimed mask stage and hp3d_gather_frames give the same bits, the
    single-hand tracker's option keeps its own value checks, and no counter of this option moves."""
    e = emu_engine
    sm = HO.rect_scoremap(TH.RECTS5, 120, 160)
    keep = TH.as_keep(2, {0: (20.0, 25.0, 10.0)})
    x = np.random.default_rng(3).uniform(-0.5, 0.5, (3, 16, 16, 3)).astype(np.float32)
    n0 = e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')
    res = {}
    for opt in ('0', '1'):
        e.set_option(THP.OPTION, opt)
        try:
            res[opt] = (e.masks_from_scoremap(sm, 2, keep=keep), {'g': e.gather_frames(x, [0, 2])})
            with pytest.raises(AssertionError, match="track_partial_detect wants 0 or 1"):
                e.set_option('track_partial_detect', '2')
        finally:
            e.set_option(THP.OPTION, '0')
    for a, b in zip(res['0'], res['1']):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert (e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')) == n0


@pytest.fixture(scope='module')
def engines(emu_engine, synth_weights):
    from hand3d_amd import _lib
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    off = _lib.Engine(0, path=emu_engine.lib._name)
    off.load_weight_dict(synth_weights)
    off.finalize_weights(0)
    yield emu_engine, off
    off.close()
    emu_engine.track_hands_reset()


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_b2_k2_32x32(engines):
    """(2, 2, 32, 32), slot (1, 0) lost: HandSegNet at batch 1 on frame 1; frame 0's slots are bit-equal to the option-off run."""
    THP.assert_partial_step(engines[0], engines[1], 2, 2, 32, 32, [(1, 0)], [], 'f32', 1)


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_chunks(engines):
    THP.assert_chunks(engines[0], engines[1], 32, 32)


@pytest.mark.slow
@skip_unless_slow
def test_other_entry_points_ignore_the_option(engines):
    THP.assert_ignored_elsewhere(engines[0], 32, 32)
