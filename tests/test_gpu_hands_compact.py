"""Option "hands_compact"  through the real library, with the helper the interpreter tests use
(tests/helpers/hands_compact_oracle.py): tracked steps with absent slots against the composition at batch m, the absent rule and the
restated state machine; valid slots equal to the single-hand tracker at batch m; a step without an absent slot equal to the option off;
on against off within the project's end-to-end gates; detect steps and hp3d_infer_hands (the flag wait, an engine that finds no hand at
all); the device-pointer, uint8, detect_scale and half-precision forms; and that the option off enqueues what it did."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth
from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO            # noqa: E402
import track_oracle as TO            # noqa: E402
import track_hands_oracle as THO     # noqa: E402
import hands_compact_oracle as HCO   # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
H, W = 240, 320


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    return gpu_engine


@pytest.fixture()
def on(eng):
    eng.set_option('hands_compact', '1')
    yield eng
    eng.set_option('hands_compact', '0')
    eng.set_option('micro_batch', 'auto')
    eng.track_hands_reset()
    eng.track_reset()


def seeds(valid, h=H, w=W):
    """Boxes for a valid pattern [B,K]: scale 10 around points at least 40 px inside the frame, so that every keypoint of a valid slot
    lands within 12.8 px of its seed, inside the frame: no valid slot can be lost on the first step."""
    valid = np.asarray(valid, np.int32)
    B, K = valid.shape
    center = np.zeros((B, K, 2), F32)
    for b in range(B):
        for j in range(K):
            center[b, j] = (40.0 + (h - 80.0) * (j + 1) / (K + 1) + 3 * b, 40.0 + (w - 80.0) * (K - j) / (K + 1) - 5 * b)
    return center, np.full((B, K), 10.0, F32), valid


def seeded(e, valid, h=H, w=W):
    c, s, v = seeds(valid, h, w)
    e.track_hands_seed(c, s, v, h, w)
    m = THO.Machine()
    m.seed(c, s, v, h, w)
    return m, c, s, v


PATTERNS = {(2, 2): [[1, 0], [1, 1]],                                   # an image with one valid slot, an image with all
            (3, 4): [[1, 0, 0, 0], [1, 1, 1, 1], [0, 1, 0, 1]]}         # ... and with micro_batch = 4 one frame per chunk: 1, 4 (uncompacted), 2


@pytest.mark.parametrize("B,K,micro", [(2, 2, None), (3, 4, 4)])
def test_tracked_steps_against_the_composition(on, B, K, micro):
    e = on
    if micro:
        e.set_option('micro_batch', str(micro))
    per_chunk = HCO.chunk_frames(B, K, micro or 32)
    hs = HO.hand_sides(B, K)
    m, _, _, valid = seeded(e, PATTERNS[(B, K)])
    for t in range(3):
        o, detect, ms = HCO.step_and_check(e, m, TO.frames(11, t, B, H, W), hs, K, per_chunk)
        if t == 0:
            assert not detect and np.array_equal(o['valid'], valid) and not o['lost'].any()
            assert 'slot_scatter' in HCO.last_rows
            assert ms == ([3] if micro is None else [1, 4, 2])
            if micro:          # the chunk without an absent slot took the uncompacted crop, the others the indexed one
                assert HCO.last_rows.count('crop_and_resize') == 1 and HCO.last_rows.count('crop_and_resize_idx') == 2


def test_valid_slots_equal_the_single_hand_tracker_at_batch_m(on):
    """test_k1_is_the_single_hand_tracker's argument at K > 1: the m valid slots of a compacted tracked step against hp3d_track_step on
    the frames idx // K seeded with the same boxes."""
    e = on
    B, K = 2, 2
    hs, fr = HO.hand_sides(B, K), TO.frames(21, 0, B, H, W)
    m, c, s, valid = seeded(e, PATTERNS[(B, K)])
    nt = e.counter('track_hands_tracked_steps')
    o = e.track_hands_step(fr, hs, K, want_kpmap=True)
    assert e.counter('track_hands_tracked_steps') == nt + 1
    idx, _ = HCO.idx_pos(valid)
    assert idx.tolist() == [0, 2, 3]
    e.track_seed(c.reshape(-1, 2)[idx], s.reshape(-1)[idx], H, W)
    nt = e.counter('track_tracked_steps')
    a = e.track_step(fr[idx // K], hs.reshape(-1, 2)[idx], want_kpmap=True)
    assert e.counter('track_tracked_steps') == nt + 1
    for k in ('crop', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost'):
        assert np.array_equal(o[k].reshape((B * K,) + o[k].shape[2:])[idx], a[k]), k


def test_no_absent_slot_is_the_option_off(eng):
    B, K = 2, 2
    hs, fr = HO.hand_sides(B, K), TO.frames(31, 0, B, H, W)
    outs, rows = [], []
    try:
        for opt in ('0', '1'):
            eng.set_option('hands_compact', opt)
            seeded(eng, np.ones((B, K), np.int32))
            c0 = HCO.counters(eng)
            eng.set_profiling(1)
            try:
                outs.append(eng.track_hands_step(fr, hs, K, want_kpmap=True))
                rows.append([r[0] for r in eng.profile()])
            finally:
                eng.set_profiling(0)
            assert tuple(np.subtract(HCO.counters(eng), c0)) == ((0, 0, 0) if opt == '0' else (B * K, 0, 0))
    finally:
        eng.set_option('hands_compact', '0')
        eng.track_hands_reset()
    assert rows[0] == rows[1] and not set(rows[1]) & set(HCO.NEW_ROWS)
    for k, v in outs[0].items():
        assert np.array_equal(v, outs[1][k]), k


def test_against_the_option_off(eng):
    """The same seeded state with the option off and on: on valid slots the crop and the box are bit-equal; the heat maps and the 3-D
    keypoints agree within the project's end-to-end gates -- the kernel plan follows the batch size."""
    B, K = 3, 4
    hs, fr = HO.hand_sides(B, K), TO.frames(41, 0, B, H, W)
    outs = []
    try:
        for opt in ('0', '1'):
            eng.set_option('hands_compact', opt)
            _, _, _, valid = seeded(eng, PATTERNS[(B, K)])
            outs.append(eng.track_hands_step(fr, hs, K, want_kpmap=True))
    finally:
        eng.set_option('hands_compact', '0')
        eng.track_hands_reset()
    off, on_ = outs
    v = valid != 0
    for k in ('center', 'scale', 'valid', 'detected', 'area', 'claimed'):
        assert np.array_equal(off[k], on_[k]), k
    assert np.array_equal(off['crop'][v], on_['crop'][v])
    d_map, d_xyz = np.abs(off['kpmap'][v] - on_['kpmap'][v]).max(), np.abs(off['coord3d'][v] - on_['coord3d'][v]).max()
    print('on vs off: kpmap %.3g coord3d %.3g' % (d_map, d_xyz))
    assert d_map < TO.TOL_HEATMAP and d_xyz < TO.TOL_KP3D
    HCO.assert_absent_rule(on_, valid)
    assert off['confidence'][~v].any()          # (the one difference: the option off reports the fall-back crop's score)


def test_detect_steps_and_infer_hands(on):
    """K = 4 on the synthetic frames with `hands_min_area` at the second-largest object's size, so that fewer than four objects per frame
    are hands: hp3d_infer_hands and a fresh detect step, one wait per chunk."""
    e = on
    B, K = 2, 4
    hs, fr = HO.hand_sides(B, K), synth.make_batch(0, B, H, W)
    e.set_option('hands_compact', '0')
    probe = e.infer_hands(fr, hs, K, outputs=())
    min_area = int(np.sort(probe['area'].reshape(-1))[-2])
    e.set_option('hands_min_area', str(min_area))
    try:
        off = e.infer_hands(fr, hs, K, want_mask=True)
        e.set_option('hands_compact', '1')
        assert 0 < off['valid'].sum() < B * K, off['valid'].tolist()
        o, ms = HCO.infer_hands_and_check(e, fr, hs, K, HCO.chunk_frames(B, K), off=off)
        assert ms == [int(off['valid'].sum())] and 'slot_scatter' in HCO.last_rows and 'crop_and_resize_idx' in HCO.last_rows
        # two chunks of one frame each: two waits (counted inside the helper)
        # (HandSegNet's kernel plan follows the chunk: the option-off reference is taken at the same micro_batch)
        e.set_option('micro_batch', '4')
        e.set_option('hands_compact', '0')
        off = e.infer_hands(fr, hs, K, want_mask=True)
        e.set_option('hands_compact', '1')
        assert 0 < off['valid'].sum() < B * K, off['valid'].tolist()
        HCO.infer_hands_and_check(e, fr, hs, K, 1, off=off)
        e.track_hands_reset()
        m = THO.Machine(min_area=min_area)
        o, detect, ms = HCO.step_and_check(e, m, fr, hs, K, 1)
        assert detect and np.array_equal(o['valid'], off['valid']) and np.array_equal(o['area'], off['area'])
    finally:
        e.set_option('hands_min_area', '0')


def test_no_hand_at_all_runs_no_back_half():
    """HandSegNet weights whose foreground logit is far below zero: det is empty, m = 0 -- no PoseNet2D row, every back-half output 0,
    and the tracker detects every step (test_all_background_engine_detects_every_step with the option on)."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth.make_weights(seg_bias=-60.0))
        e.finalize_weights(0)
        B, K = 2, 3
        hs = HO.hand_sides(B, K)
        off = e.infer_hands(TO.frames(9, 0, B, H, W), hs, K, want_mask=True)
        e.set_option('hands_compact', '1')
        o, ms = HCO.infer_hands_and_check(e, TO.frames(9, 0, B, H, W), hs, K, HCO.chunk_frames(B, K), off=off)
        assert ms == [0] and not o['valid'].any() and not [r for r in HCO.last_rows if r.startswith(('PoseNet2D/', 'PosePrior', 'ViewpointNet/'))]
        for k in HCO.BACK_KEYS:
            assert not o[k].any(), k
        m = THO.Machine()
        for t in range(3):
            o, detect, ms = HCO.step_and_check(e, m, TO.frames(9, t, B, H, W), hs, K, HCO.chunk_frames(B, K))
            assert detect and ms == [0] and not o['valid'].any() and not o['lost'].any() and not o['confidence'].any()
            assert not [r for r in HCO.last_rows if r.startswith('PoseNet2D/')]
            assert np.all(o['center'] == 160.0) and np.all(o['scale'] == THO.FALLBACK_SCALE)
        assert e.counter('track_hands_tracked_steps') == 0 and e.counter('track_hands_detect_steps') == 3
    finally:
        e.close()


STEP_SHAPES = lambda B, K: {'crop': ((B, K, 256, 256, 3), F32), 'scale': ((B, K), F32), 'center': ((B, K, 2), F32),
                            'kpmap': ((B, K, 256, 256, 21), F32), 'coord3d': ((B, K, 21, 3), F32), 'kp_crop': ((B, K, 21, 2), np.int32),
                            'kp_hw': ((B, K, 21, 2), np.float64), 'confidence': ((B, K), F32), 'lost': ((B, K), np.int32),
                            'detected': ((B, K), np.int32), 'valid': ((B, K), np.int32), 'area': ((B, K), np.int32),
                            'claimed': ((B, K), np.int32)}


def test_dev_form_equals_host_form(on):
    """The scatter into the caller's device buffers: a seeded tracked step and hp3d_infer_hands_dev, each also with one output left NULL
    (the heat maps), whose buffer must come back untouched."""
    e = on
    B, K = 2, 2
    hs, fr = HO.hand_sides(B, K), synth.make_batch(0, B, H, W)
    shapes = STEP_SHAPES(B, K)
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    d_hs, d_img = e.to_device(hs), e.to_device(fr)
    fill = np.full(shapes['kpmap'][0], -3.0, F32)
    try:
        seeded(e, PATTERNS[(B, K)])
        host = e.track_hands_step(fr, hs, K, want_kpmap=True)
        for skip in ((), ('kpmap',)):
            seeded(e, PATTERNS[(B, K)])
            e._chk(e.lib.hp3d_memcpy(e.h, int(bufs['kpmap']), fill.ctypes.data, fill.nbytes, 0))
            e.track_hands_step_dev(B, H, W, K, d_img, d_hs, **{k: int(v) for k, v in bufs.items() if k not in skip})
            e.sync()
            for k, (s, dt) in shapes.items():
                got = e.to_host(bufs[k], s, dt)
                assert np.array_equal(got, fill if k in skip else host[k]), (k, skip)
        hosth = e.infer_hands(fr, hs, K)
        names = {'crop': 'crop', 'scale': 'scale', 'center': 'center', 'kpmap': 'kpmap', 'coord3d': 'coord3d', 'kp_crop': 'kp_crop',
                 'kp_hw': 'kp_hw', 'valid': 'valid', 'area': 'area'}
        for skip in ((), ('kpmap',)):
            e._chk(e.lib.hp3d_memcpy(e.h, int(bufs['kpmap']), fill.ctypes.data, fill.nbytes, 0))
            e.infer_hands_dev(B, H, W, K, d_img, d_hs, **{k: int(bufs[k]) for k in names if k not in skip})
            e.sync()
            for k in names:
                got = e.to_host(bufs[k], *shapes[k])
                assert np.array_equal(got, fill if k in skip else hosth[k]), (k, skip)
    finally:
        for b in list(bufs.values()) + [d_hs, d_img]:
            b.free()


def test_uint8_frames_720p(on):
    """uint8 at 720 x 1280, K = 2: a detect step (global mask growth; it crops from the frame it normalised for HandSegNet), then a
    seeded tracked step with slot 1 absent (the indexed crop straight from the uint8 frame)."""
    e = on
    h, w, K = 720, 1280, 2
    hs = HO.hand_sides(1, K)
    u8 = TO.to_u8(TO.frames(5, 0, 1, h, w))
    fr = G.preprocess_u8(u8, h, w)
    e.track_hands_reset()
    ng = e.counter('mask_grow_global_launches')
    o, detect, ms = HCO.step_and_check(e, THO.Machine(), fr, hs, K, 1, u8=u8)
    assert detect and e.counter('mask_grow_global_launches') == ng + 1
    m, _, _, _ = seeded(e, [[1, 0]], h, w)
    nu = e.counter('crop_u8_launches')
    o, detect, ms = HCO.step_and_check(e, m, fr, hs, K, 1, u8=u8)
    assert not detect and ms == [1] and 'crop_and_resize_idx_u8' in HCO.last_rows and e.counter('crop_u8_launches') == nu + 1


def test_detect_scale_2_at_720p(eng):
    """detect_scale = 2 at 720 x 1280, K = 4: a fresh detect step with the option on against the option off -- everything in front of the
    crop and the crop of the valid slots bit-equal, behind it the composition at batch m on the step's own boxes and the absent rule."""
    h, w, B, K = 720, 1280, 1, 4
    hs, fr = HO.hand_sides(B, K), TO.frames(5, 0, B, h, w)
    outs = []
    eng.set_option('detect_scale', '2')
    try:
        for opt in ('0', '1'):
            eng.set_option('hands_compact', opt)
            eng.track_hands_reset()
            c0 = HCO.counters(eng)
            outs.append(eng.track_hands_step(fr, hs, K, want_kpmap=True))
            c1 = HCO.counters(eng)
        off, on_ = outs
        v = on_['valid'] != 0
        for k in ('center', 'scale', 'valid', 'detected', 'area', 'claimed'):
            assert np.array_equal(off[k], on_[k]), k
        assert np.array_equal(off['crop'][v], on_['crop'][v])
        assert tuple(np.subtract(c1, c0)) == (int(v.sum()), int((~v).sum()), 1)
        back, ms = HCO.expected_back_half(eng, fr, hs, on_['center'], on_['scale'], on_['valid'], K, 1)
        HCO.assert_back_half(on_, back)
        HCO.assert_absent_rule(on_, on_['valid'])
    finally:
        eng.set_option('hands_compact', '0')
        eng.set_option('detect_scale', '1')
        eng.track_hands_reset()


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        e.set_option('hands_compact', '1')
        B, K = 2, 2
        m, _, _, _ = seeded(e, PATTERNS[(B, K)])
        o, detect, ms = HCO.step_and_check(e, m, TO.frames(3, 0, B, H, W), HO.hand_sides(B, K), K, B)
        assert not detect and ms == [3]
    finally:
        e.close()


def test_option_off_is_the_parent(eng):
    """One track_hands_step and one infer_hands with the option off: the profile rows test_gpu_track_hands.test_profile_rows pins, none
    of the new rows, and the new counters do not move."""
    fr, hs = synth.make_batch(2, 2, H, W), HO.hand_sides(2, 4)
    eng.set_option('hands_compact', '1')
    eng.set_option('hands_compact', '0')
    eng.track_hands_reset()
    c0 = HCO.counters(eng)
    eng.set_profiling(1)
    try:
        eng.track_hands_step(fr, hs, 4)
        rows = [r[0] for r in eng.profile()]
        eng.infer_hands(fr, hs, 4, outputs=('coord3d',))
        hands = [r[0] for r in eng.profile()]
    finally:
        eng.set_profiling(0)
        eng.track_hands_reset()
    extra = ('track_hands_select', 'track_hands_box', 'kp_detect')
    assert [r for r in rows if r not in extra] == [r for r in hands if r not in extra]
    assert rows.count('track_hands_select') == 1 and rows.count('track_hands_box') == 1 and rows.count('mask_grow_multi') == 1
    assert rows.index('mask_grow_multi') < rows.index('track_hands_select') < rows.index('crop_and_resize')
    assert not set(rows + hands) & set(HCO.NEW_ROWS)
    assert HCO.counters(eng) == c0
