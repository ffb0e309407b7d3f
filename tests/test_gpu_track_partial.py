"""Option "track_partial_detect"  through the real library, with the helpers the interpreter tests use
(tests/helpers/track_partial_oracle.py): hp3d_gather_frames against the existing per-ops bit for bit; a detect step that runs
HandSegNet on the lost frames only -- rows, counters, the boxes of the lost frames against the same ops on the gathered frames, the
composition of the back half, and image by image against the same two steps on a second context with the option off (bit-equal
outside the lost set); chunks; the device-pointer form; half-precision trunks."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import track_oracle as TO              # noqa: E402
import track_partial_oracle as TP      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


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
    gpu_engine.track_reset()


def test_option_values(gpu_engine):
    try:
        for v in ('0', '1'):
            gpu_engine.set_option('track_partial_detect', v)
        for v in ('2', 'on'):
            with pytest.raises(AssertionError, match="track_partial_detect wants 0 or 1"):
                gpu_engine.set_option('track_partial_detect', v)
    finally:
        gpu_engine.set_option('track_partial_detect', '0')


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("B,H,W", TP.GATHER_SHAPES)
def test_gather_frames_bit_exact(gpu_engine, B, H, W, f, u8):
    for idx in TP.gather_indices(B):
        TP.assert_gather_frames_exact(gpu_engine, B, H, W, f, idx, u8)


def test_gather_frames_hd_u8_f4(gpu_engine):
    """(2, 1080, 1920) uint8 at f = 4: the one-load window rows, on the selected frame's base."""
    TP.assert_gather_frames_exact(gpu_engine, 2, 1080, 1920, 4, [1], True)


def test_gather_frames_errors(gpu_engine):
    TP.assert_gather_frames_errors(gpu_engine)


@pytest.mark.parametrize("B,H,W,lost,u8,f", [(4, 64, 64, [0], False, 1), (4, 64, 64, [3], True, 1), (5, 37, 53, [1, 3], False, 1),
                                             (4, 70, 100, [0, 1, 2], True, 3), (8, 320, 320, [5], False, 1)])
def test_partial_step(engines, B, H, W, lost, u8, f):
    """(8, 320, 320, {5}) reaches the filled-launch plan at nb = 8 while HandSegNet runs the small-batch plan at m = 1: the case where
    'an image that kept its box is bit-equal to the option off' can break."""
    TP.assert_partial_step(engines[0], engines[1], B, H, W, lost, u8, f)


def test_partial_step_chunks(engines):
    """micro_batch = 2, B = 5, lost = {1, 4}: a partial chunk, a chunk enqueued as a tracked one, a whole chunk; one detect step."""
    o2 = TP.assert_partial_step(engines[0], engines[1], 5, 64, 64, [1, 4], False, 1, micro_batch=2)
    assert o2['detected'].tolist() == [0, 1, 0, 0, 1]


def test_fresh_and_scheduled_steps_untouched(engines):
    TP.assert_scheduled_and_fresh_untouched(engines[0], 64, 64)


def test_other_entry_points_ignore_the_option(engines):
    TP.assert_other_entry_points_ignore(engines[0], 64, 64)


STEP_SHAPES = lambda B: {'crop': ((B, 256, 256, 3), F32), 'scale': ((B, 1), F32), 'center': ((B, 2), F32), 'kpmap': ((B, 256, 256, 21), F32),
                         'coord3d': ((B, 21, 3), F32), 'kp_crop': ((B, 21, 2), np.int32), 'kp_hw': ((B, 21, 2), np.float64),
                         'confidence': ((B,), F32), 'lost': ((B,), np.int32), 'detected': ((B,), np.int32)}


def test_dev_form_equals_host_form(engines):
    eng = engines[0]
    B, H, W, lost = 4, 64, 64, [2]
    hs = synth.hand_sides(B)
    _, host, _, dn, fr1, _ = TP.run_two_steps(eng, '1', B, H, W, lost, False, 1)
    assert dn['track_partial_frames_run'] == 1
    shapes = STEP_SHAPES(B)
    bufs = {k: eng.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    d_hs, d_img0, d_img1 = eng.to_device(hs), eng.to_device(TO.frames(21, 0, B, H, W)), eng.to_device(fr1)
    eng.set_option('track_partial_detect', '1')
    try:
        eng.track_seed(*TP.seed_boxes(B, H, W, lost), H, W)
        args = {k: int(v) for k, v in bufs.items()}
        eng.track_step_dev(B, H, W, d_img0, d_hs, **args)
        eng.sync()
        assert np.array_equal(eng.to_host(bufs['lost'], (B,), np.int32), TP.pattern(B, lost))
        n = eng.counter('track_partial_frames_run'), eng.counter('frame_gather_launches')
        eng.track_step_dev(B, H, W, d_img1, d_hs, **args)
        eng.sync()
        assert (eng.counter('track_partial_frames_run'), eng.counter('frame_gather_launches')) == (n[0] + 1, n[1] + 1)
        for k, (s, dt) in shapes.items():
            assert np.array_equal(eng.to_host(bufs[k], s, dt), host[k]), k
    finally:
        eng.set_option('track_partial_detect', '0')
        eng.track_reset()
        for b in list(bufs.values()) + [d_hs, d_img0, d_img1]:
            b.free()


def test_half_precision_trunks(synth_weights):
    """(3, 64, 64, {1}) on a half-precision context: the lost frame's box is infer_full's on the gathered frame on the same context."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        o2 = TP.assert_partial_step(e, None, 3, 64, 64, [1], False, 1, compare_off=False)
        assert o2['detected'].tolist() == [0, 1, 0]
    finally:
        e.close()
