"""Detection on a reduced frame (option "detect_scale") through the real library, with the helpers the interpreter tests
use (tests/helpers/detect_scale_oracle.py): the downscale kernels and the box maps bit for bit; detect steps as the composition of the
engine's own per-op calls (float32 host frames, uint8 HD frames, half-precision trunks); the multi-hand tracker against the restated
state machine with rules 3 and 4 around its detection; the device-pointer form.  Every comparison is bit-exact: the mask stage is held
on the device's own score map."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import detect_scale_oracle as DS     # noqa: E402
import hands_oracle as HO            # noqa: E402
import track_oracle as TO            # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    yield gpu_engine
    gpu_engine.set_option('detect_scale', '1')
    gpu_engine.track_reset()
    gpu_engine.track_hands_reset()


@pytest.mark.parametrize("B,H,W,f", DS.DOWNSCALE_SHAPES + DS.DOWNSCALE_SHAPES_WIDE + [(1, 1080, 1920, 4), (2, 240, 320, 2), (1, 1080, 1920, 8), (1, 270, 482, 2)])
def test_downscale_bit_exact(gpu_engine, B, H, W, f):
    DS.assert_downscale_exact(gpu_engine, B, H, W, f)


@pytest.mark.parametrize("f", [2, 3, 4, 8])
def test_boxes_bit_exact(gpu_engine, f):
    DS.assert_boxes_exact(gpu_engine, f)


def test_claim_rule_at_f2(gpu_engine):
    DS.run_claim_at(gpu_engine, 2)


def test_detect_step_is_the_composition_240x320(eng):
    """B = 2, 240 x 320, f = 2, float32 host frames; then a tracked step, which the option leaves alone."""
    B, H, W = 2, 240, 320
    fr, hs = TO.frames(7, 0, B, H, W), synth.hand_sides(B)
    eng.set_option('detect_scale', '2')
    try:
        eng.track_reset()
        o, rows, dn = DS.run_detect_step(eng, lambda: eng.track_step(fr, hs, want_kpmap=True))
        assert (dn['track_detect_steps'], dn['detect_scale_steps'], dn['crop_u8_launches']) == (1, 1, 0)
        DS.assert_detect_step_is_composition(eng, o, rows, fr, 2)
        TO.assert_step_is_composition(eng, o, fr, hs, o['center'], o['scale'], H, W)          # the back half, in frame coordinates
        # seeded with the boxes the keypoints give, the next step is tracked: the rows and outputs of a tracked step at f = 1
        c, s, _, _ = eng.track_box(o['kp_hw'], H, W)
        fr1 = TO.frames(7, 1, B, H, W)
        eng.track_seed(c, s, H, W)
        t2, rows2, dn2 = DS.run_detect_step(eng, lambda: eng.track_step(fr1, hs, want_kpmap=True))
        assert (dn2['track_tracked_steps'], dn2['detect_scale_steps']) == (1, 0) and not [r for r in rows2 if r.startswith(('downscale', 'box_to'))]
        eng.set_option('detect_scale', '1')
        eng.track_seed(c, s, H, W)
        t1, rows1, _ = DS.run_detect_step(eng, lambda: eng.track_step(fr1, hs, want_kpmap=True))
        assert rows1 == rows2
        for k, v in t1.items():
            assert np.array_equal(v, t2[k]), k
        # a change of the option counts as a change of shape: seeded at f = 1 (nothing lost), the step at f = 2 detects all the same
        eng.track_seed(c, s, H, W)
        eng.set_option('detect_scale', '2')
        o3, rows3, dn3 = DS.run_detect_step(eng, lambda: eng.track_step(fr1, hs))
        assert (dn3['track_detect_steps'], dn3['detect_scale_steps']) == (1, 1)
        DS.assert_detect_step_is_composition(eng, o3, rows3, fr1, 2)
    finally:
        eng.set_option('detect_scale', '1')
        eng.track_reset()


def test_detect_step_u8_720p_f4(synth_weights):
    """B = 1, 720 x 1280, f = 4 through hp3d_track_step_u8 on a context of its own: no preprocess_u8 row, one crop_and_resize_u8 row, and
    an arena that follows the 180 x 320 detection frame (two activation buffers of 720 x 1280 x 64 floats are 472 MB)."""
    from hand3d_amd import _lib
    B, H, W, f = 1, 720, 1280, 4
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights(0)
        e.set_option('detect_scale', str(f))
        u8 = TO.to_u8(TO.frames(5, 0, B, H, W))
        hs = synth.hand_sides(B)
        fr = (u8.astype(F32) / F32(255.0) - F32(0.5)).astype(F32)          # oracle.general.preprocess_u8 at equal sizes
        o, rows, dn = DS.run_detect_step(e, lambda: e.track_step_u8(u8, hs))
        assert (dn['track_detect_steps'], dn['detect_scale_steps'], dn['crop_u8_launches']) == (1, 1, 1)
        assert dn['mask_grow_global_launches'] == 0           # 180 x 320 fits the in-LDS growth; 720 x 1280 does not
        assert e.counter('arena_bytes') < 2 * H * W * 64 * 4 // 8
        DS.assert_detect_step_is_composition(e, o, rows, fr, f, u8=u8)
    finally:
        e.close()


def test_track_hands_at_f2(eng):
    """B = 1, K = 2, 240 x 320, f = 2: a detect step; seeded like tests/test_gpu_track_hands.py's claim path (slot 0 on hand 0 with scale
    10 -- it cannot be lost --, slot 1 far outside the frame) a tracked step that loses slot 1; then a detect step that keeps slot 0,
    whose box mapped by rule 4 claims object 0, and gives slot 1 the first unclaimed object.  Step kinds, valid, detected, claimed,
    area and the boxes are MachineAt's."""
    H, W, K, f = 240, 320, 2, 2
    fr, hs = synth.make_batch(0, 1, H, W), HO.hand_sides(1, K)
    eng.set_option('detect_scale', str(f))
    try:
        eng.track_hands_reset()
        m = DS.MachineAt(f)
        o0, detect, _ = DS.step_hands_and_check(eng, m, fr, hs, K)
        assert detect and o0['valid'][0, 0] == 1 and not o0['claimed'].any()
        c0 = o0['center'][0, 0]
        assert 12.8 <= c0[0] <= H - 12.8 and 12.8 <= c0[1] <= W - 12.8
        center = np.array([[c0, [-5000.0, -7000.0]]], F32)
        scale, valid = np.array([[10.0, 1.0]], F32), np.ones((1, K), np.int32)
        eng.track_hands_seed(center, scale, valid, H, W)
        m.seed(center, scale, valid, H, W)
        o1, detect, _ = DS.step_hands_and_check(eng, m, fr, hs, K)
        assert not detect and o1['lost'][0].tolist() == [0, 1]
        tc, ts, _, _ = eng.track_box(o1['kp_hw'][0, :1], H, W)
        o2, detect, rows = DS.step_hands_and_check(eng, m, fr, hs, K)
        assert detect and o2['detected'][0].tolist() == [0, 1] and o2['claimed'][0, 0] >= 1 and o2['valid'][0].tolist() == [1, 1]
        assert np.array_equal(o2['center'][0, 0], tc[0]) and o2['scale'][0, 0] == ts[0]
        assert rows.index('box_to_detect') < rows.index('mask_grow_multi') < rows.index('box_to_frame') < rows.index('track_hands_select')
    finally:
        eng.set_option('detect_scale', '1')
        eng.track_hands_reset()


STEP_SHAPES = lambda B: {'crop': ((B, 256, 256, 3), F32), 'scale': ((B, 1), F32), 'center': ((B, 2), F32), 'kpmap': ((B, 256, 256, 21), F32),
                         'coord3d': ((B, 21, 3), F32), 'kp_crop': ((B, 21, 2), np.int32), 'kp_hw': ((B, 21, 2), np.float64),
                         'confidence': ((B,), F32), 'lost': ((B,), np.int32), 'detected': ((B,), np.int32)}


def test_dev_form_equals_host_form(eng):
    B, H, W = 2, 240, 320
    fr, hs = TO.frames(70, 0, B, H, W), synth.hand_sides(B)
    shapes = STEP_SHAPES(B)
    bufs = {k: eng.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    d_hs, d_img = eng.to_device(hs), eng.to_device(fr)
    eng.set_option('detect_scale', '2')
    try:
        eng.track_reset()
        host = eng.track_step(fr, hs, want_kpmap=True)
        eng.track_reset()
        n = eng.counter('detect_scale_steps')
        eng.track_step_dev(B, H, W, d_img, d_hs, **{k: int(v) for k, v in bufs.items()})
        eng.sync()
        assert eng.counter('detect_scale_steps') == n + 1
        for k, (s, dt) in shapes.items():
            assert np.array_equal(eng.to_host(bufs[k], s, dt), host[k]), k
    finally:
        eng.set_option('detect_scale', '1')
        eng.track_reset()
        for b in list(bufs.values()) + [d_hs, d_img]:
            b.free()


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    B, H, W = 2, 240, 320
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        e.set_option('detect_scale', '2')
        fr, hs = TO.frames(7, 0, B, H, W), synth.hand_sides(B)
        o, rows, dn = DS.run_detect_step(e, lambda: e.track_step(fr, hs))
        assert dn['detect_scale_steps'] == 1
        DS.assert_detect_step_is_composition(e, o, rows, fr, 2)
    finally:
        e.close()
