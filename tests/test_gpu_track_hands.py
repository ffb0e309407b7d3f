"""The multi-hand tracker through the real library, with the helpers the interpreter tests use
(tests/helpers/track_hands_oracle.py): the claim rule per op in both kernel forms; K = 1 equal to the single-hand tracker; three steps at
K = 2 and 4 at the shipped shapes against hp3d_infer_hands, the restated state machine, the chain of per-op calls and the oracle; the
claim path through the whole executor; the schedule and the resets; the device-pointer, chunked, uint8 and half-precision forms; an
all-background engine."""
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

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    return gpu_engine


def test_claim_rule_per_op(gpu_engine):
    THO.run_claim_cases(gpu_engine)
    THO.run_random_keeps(gpu_engine, trials=8)
    # once at 540 x 960, where only the global form runs: the stronger ellipse is kept and claimed, the other one fills slot 1
    H, W = 540, 960
    y, x = np.mgrid[:H, :W]
    sm = np.zeros((1, H, W, 2), F32)
    sm[..., 1] = -2.0
    for cy, cx, s in ((120, 150, 3.0), (400, 800, 4.0)):
        sm[0, :, :, 1] = np.where(((y - cy) / 45.0) ** 2 + ((x - cx) / 35.0) ** 2 <= 1.0, s, sm[0, :, :, 1])
    n_g = gpu_engine.counter('mask_grow_global_launches')
    got = THO.assert_keep_exact(gpu_engine, sm, 3, THO.as_keep(3, {0: (395.0, 790.0, 4.0)}), both_forms=False)
    assert gpu_engine.counter('mask_grow_global_launches') == n_g + 1
    assert got['claimed'][0].tolist() == [1, 0, 0] and got['valid'][0].tolist() == [0, 1, 0] and got['seed'][0, 1, 0] < 200


def test_per_slot_box_rule(gpu_engine):
    rng = np.random.default_rng(22)
    for (B, K, H, W) in ((8, 4, 320, 320), (1, 2, 1080, 1920)):
        kp = rng.normal([H / 2, W / 2], [H / 2, W / 2], (B, K, 21, 2))
        valid = (rng.random((B, K)) < 0.6).astype(np.int32)
        bc, bs = rng.uniform(0, [H, W], (B, K, 2)).astype(F32), rng.uniform(1, 5, (B, K)).astype(F32)
        THO.assert_box_slots(gpu_engine, kp, valid, bc, bs, H, W, score32=rng.standard_normal((B, K, 32, 32, 21)).astype(F32))


def test_k1_is_the_single_hand_tracker(eng):
    """Three steps at B = 3, 240 x 320, track_redetect = 0: every common output of hp3d_track_hands_step at K = 1 equals
    hp3d_track_step's bit for bit.  (Where det is empty the two differ on purpose -- an image without a valid slot detects on every
    step -- so every detect step's det is asserted non-empty.)"""
    B, H, W = 3, 240, 320
    hs = synth.hand_sides(B)
    eng.track_reset()
    eng.track_hands_reset()
    kinds = []
    for t in range(3):
        fr = TO.frames(7, t, B, H, W)
        nd = eng.counter('track_detect_steps'), eng.counter('track_hands_detect_steps')
        a = eng.track_step(fr, hs, want_kpmap=True)
        b = eng.track_hands_step(fr, hs.reshape(B, 1, 2), 1, want_kpmap=True)
        da, db = eng.counter('track_detect_steps') - nd[0], eng.counter('track_hands_detect_steps') - nd[1]
        assert da == db, t
        kinds.append(da)
        if da:
            assert G.fg_and_detmap(eng.handsegnet(fr))[1].reshape(B, -1).any(axis=1).all()
        for k in ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost', 'detected'):
            assert np.array_equal(b[k].reshape(a[k].shape), a[k]), (t, k)
        assert np.all(b['valid'] == 1)
    assert kinds[0] == 1
    eng.track_reset()
    eng.track_hands_reset()


@pytest.mark.parametrize("K", [2, 4])
def test_three_steps_240x320(eng, synth_weights, K):
    assert THO.run_steps(eng, synth_weights, 3, K, 240, 320, seed=0, oracle_slots=[(0, 0), (2, K - 1)]) >= 1


def test_three_steps_without_reseeding(eng):
    """Whatever the random-weight keypoints do -- losses, claimed detect steps -- every step is the restated machine's."""
    THO.run_steps(eng, None, 3, 2, 240, 320, seed=0, steps=4, reseed=False)


def test_three_steps_b8_320(eng, synth_weights):
    assert THO.run_steps(eng, synth_weights, 8, 4, 320, 320, seed=40, oracle_slots=[(7, 3)]) >= 1
    assert THO.run_steps(eng, None, 8, 2, 320, 320, seed=40) >= 1


@pytest.mark.parametrize("K", [2, 4])
def test_three_steps_u8_720p(eng, synth_weights, K):
    nu, ng = eng.counter('crop_u8_launches'), eng.counter('mask_grow_global_launches')
    assert THO.run_steps(eng, synth_weights, 1, K, 720, 1280, seed=5, u8=True, oracle_slots=[(0, K - 1)], expect_global=True) >= 1
    assert eng.counter('crop_u8_launches') > nu and eng.counter('mask_grow_global_launches') > ng


@pytest.mark.parametrize("K", [2, 4])
def test_claim_path_through_the_executor(eng, K):
    """Slot 0 seeded on hand 0's mask centre with scale 10, slot 1 far outside the frame, the same frame twice.  Slot 0 cannot be lost
    (its keypoints lie within 12.8 px of the seed, which is asserted to be that far from the border) and its next box has half >= 25 px
    around a centre within 12.8 px of object 0's, so the detect step behind the loss of slot 1 must claim object 0 for slot 0, keep slot
    0's tracked box, and give slot 1 the first unclaimed object."""
    H, W = 240, 320
    fr = synth.make_batch(0, 1, H, W)
    hs = HO.hand_sides(1, K)
    full = eng.infer_hands(fr, hs, K)
    assert full['valid'][0, 0] == 1
    c0 = full['center'][0, 0]
    assert 12.8 <= c0[0] <= H - 12.8 and 12.8 <= c0[1] <= W - 12.8
    center = np.tile(np.array([-5000.0, -7000.0], F32), (1, K, 1))
    center[0, 0] = c0
    scale = np.ones((1, K), F32)
    scale[0, 0] = 10.0
    valid = np.zeros((1, K), np.int32)
    valid[0, :2] = 1
    eng.track_hands_seed(center, scale, valid, H, W)
    m = THO.Machine()
    m.seed(center, scale, valid, H, W)
    o1, detect = THO.step_and_check(eng, m, fr, hs, K)
    assert not detect and o1['lost'][0, :2].tolist() == [0, 1]
    tc, ts, _, _ = eng.track_box(o1['kp_hw'][0, :1], H, W)
    assert F32(128.0) / ts[0] >= 25.0
    sm = eng.handsegnet(fr)
    o2, detect = THO.step_and_check(eng, m, fr, hs, K, scoremap=sm)
    assert detect and o2['detected'][0, :2].tolist() == [0, 1] and o2['claimed'][0, 0] >= 1
    assert np.array_equal(o2['center'][0, 0], tc[0]) and o2['scale'][0, 0] == ts[0]
    keep = (np.array([[1] + [0] * (K - 1)], np.int32), np.concatenate([tc[None], np.zeros((1, K - 1, 2), F32)], 1),
            np.concatenate([ts[None], np.ones((1, K - 1), F32)], 1))
    ref = THO.masks_keep_rule(sm, K, *keep)
    assert ref['valid'][0, 1] == 1 and np.array_equal(o2['center'][0, 1], ref['center'][0, 1]) and o2['area'][0, 1] == ref['area'][0, 1]
    assert np.array_equal(o2['valid'][0, 1:], ref['valid'][0, 1:]) and np.array_equal(o2['center'][0, 1:], ref['center'][0, 1:])
    eng.track_hands_reset()


def test_schedule_and_resets(eng):
    H, W, K = 240, 320, 2
    fr = [TO.frames(0, t, 1, H, W) for t in range(3)]
    fr[0] = synth.make_batch(0, 1, H, W)
    hs = HO.hand_sides(1, K)
    # track_redetect = 2: slot 0 seeded at the frame's centre with scale 10 (cannot be lost), slot 1 absent.  The first step is tracked,
    # the second detects on schedule: it fills slot 1 and does not re-box slot 0
    eng.set_option('track_redetect', '2')
    try:
        center, scale, valid = np.array([[[H / 2.0, W / 2.0], [0.0, 0.0]]], F32), np.array([[10.0, 1.0]], F32), np.array([[1, 0]], np.int32)
        eng.track_hands_seed(center, scale, valid, H, W)
        m = THO.Machine(redetect=2)
        m.seed(center, scale, valid, H, W)
        oa, detect = THO.step_and_check(eng, m, fr[1], hs, K, want_kpmap=False)
        assert not detect and oa['valid'][0].tolist() == [1, 0] and oa['lost'][0].tolist() == [0, 0]
        assert oa['center'][0, 1].tolist() == [160.0, 160.0] and oa['scale'][0, 1] == THO.FALLBACK_SCALE
        ob, detect = THO.step_and_check(eng, m, fr[0], hs, K, want_kpmap=False)
        assert detect and ob['detected'][0].tolist() == [0, 1] and ob['valid'][0].tolist() == [1, 1]
        tc, ts, _, _ = eng.track_box(oa['kp_hw'][0, :1], H, W)
        assert np.array_equal(ob['center'][0, 0], tc[0]) and ob['scale'][0, 0] == ts[0]
    finally:
        eng.set_option('track_redetect', '0')
    # reset, a change of B, of K and of the frame size: detect steps that keep nothing
    eng.track_hands_step(fr[0], hs, K)
    for what in ('reset', 'B', 'K', 'size'):
        f, k = fr[0], K
        if what == 'reset':
            eng.track_hands_reset()
        elif what == 'B':
            f = np.concatenate([fr[0], fr[1]], 0)
        elif what == 'K':
            k = 3
        else:
            f = TO.frames(0, 5, 2, H - 16, W)
        B = f.shape[0]
        nd = eng.counter('track_hands_detect_steps')
        o = eng.track_hands_step(f, HO.hand_sides(B, k), k)
        assert eng.counter('track_hands_detect_steps') == nd + 1, what
        full = eng.infer_hands(f, HO.hand_sides(B, k), k, outputs=('scale', 'center'))
        assert np.array_equal(o['center'], full['center']) and np.array_equal(o['detected'], full['valid']) and not o['claimed'].any(), what
    eng.track_hands_reset()
    # the single-hand tracker's state is its own: a multi-hand step between two of its steps changes nothing for it
    eng.track_reset()
    a0 = eng.track_step(fr[0], synth.hand_sides(1))
    eng.track_hands_step(fr[1], hs, K)
    nd, nt = eng.counter('track_detect_steps'), eng.counter('track_tracked_steps')
    a1 = eng.track_step(fr[1], synth.hand_sides(1))
    assert (eng.counter('track_detect_steps') - nd, eng.counter('track_tracked_steps') - nt) == ((1, 0) if a0['lost'][0] else (0, 1))
    eng.track_reset()
    eng.track_hands_reset()


STEP_SHAPES = lambda B, K: {'crop': ((B, K, 256, 256, 3), F32), 'scale': ((B, K), F32), 'center': ((B, K, 2), F32),
                            'kpmap': ((B, K, 256, 256, 21), F32), 'coord3d': ((B, K, 21, 3), F32), 'kp_crop': ((B, K, 21, 2), np.int32),
                            'kp_hw': ((B, K, 21, 2), np.float64), 'confidence': ((B, K), F32), 'lost': ((B, K), np.int32),
                            'detected': ((B, K), np.int32), 'valid': ((B, K), np.int32), 'area': ((B, K), np.int32),
                            'claimed': ((B, K), np.int32)}


def test_dev_form_equals_host_form(eng):
    B, H, W, K = 2, 240, 320, 2
    hs = HO.hand_sides(B, K)
    shapes = STEP_SHAPES(B, K)
    bufs = {k: eng.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    d_hs = eng.to_device(hs)
    try:
        for t in range(2):          # a detect step, then (seeded) a tracked one
            fr = TO.frames(70, t, B, H, W)
            d_img = eng.to_device(fr)
            outs = []
            for dev in (False, True):
                if t == 0:
                    eng.track_hands_reset()
                else:
                    eng.track_hands_seed(seed_c, seed_s, np.ones((B, K), np.int32), H, W)
                nd, nt = eng.counter('track_hands_detect_steps'), eng.counter('track_hands_tracked_steps')
                if dev:
                    eng.track_hands_step_dev(B, H, W, K, d_img, d_hs, **{k: int(v) for k, v in bufs.items()})
                    eng.sync()
                    outs.append({k: eng.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()})
                else:
                    outs.append(eng.track_hands_step(fr, hs, K, want_kpmap=True))
                assert (eng.counter('track_hands_detect_steps') - nd, eng.counter('track_hands_tracked_steps') - nt) == ((1, 0) if t == 0 else (0, 1))
            for k in shapes:
                assert np.array_equal(outs[0][k], outs[1][k]), (t, k)
            seed_c, seed_s = outs[0]['center'], outs[0]['scale']
            d_img.free()
    finally:
        for b in list(bufs.values()) + [d_hs]:
            b.free()
        eng.track_hands_reset()


def test_chunks_equal_call_by_call(eng):
    """A batch above micro_batch / K runs chunk by chunk on one stream and equals the same frames call by call, detect and tracked."""
    B, K, H, W = 5, 2, 240, 320
    fr, hs = synth.make_batch(60, B, H, W), HO.hand_sides(B, K)
    eng.set_option('micro_batch', '4')          # 4 / 2 = two frames per chunk: 2 + 2 + 1
    try:
        eng.track_hands_reset()
        n = eng.counter('mask_grow_multi_launches')
        o = eng.track_hands_step(fr, hs, K, want_kpmap=True)
        assert eng.counter('mask_grow_multi_launches') == n + 3
        for b0, b1 in ((0, 2), (2, 4), (4, 5)):
            eng.track_hands_reset()
            p = eng.track_hands_step(fr[b0:b1], hs[b0:b1], K, want_kpmap=True)
            for k, v in p.items():
                assert np.array_equal(o[k][b0:b1], v), (k, b0)
        c, s, v = o['center'], o['scale'], np.ones((B, K), np.int32)
        eng.track_hands_seed(c, s, v, H, W)
        nt = eng.counter('track_hands_tracked_steps')
        o = eng.track_hands_step(fr, hs, K, want_kpmap=True)
        assert eng.counter('track_hands_tracked_steps') == nt + 1
        for b0, b1 in ((0, 2), (2, 4), (4, 5)):
            eng.track_hands_seed(c[b0:b1], s[b0:b1], v[b0:b1], H, W)
            p = eng.track_hands_step(fr[b0:b1], hs[b0:b1], K, want_kpmap=True)
            for k, v2 in p.items():
                assert np.array_equal(o[k][b0:b1], v2), (k, b0)
    finally:
        eng.set_option('micro_batch', 'auto')
        eng.track_hands_reset()


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        assert THO.run_steps(e, None, 2, 2, 240, 320) >= 1
    finally:
        e.close()


def test_all_background_engine_detects_every_step():
    """HandSegNet weights whose foreground logit is far below zero: det is empty, every slot is absent, no image has anything to
    follow -- every step is a detect step, every output is finite and the machine's."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth.make_weights(seg_bias=-60.0))
        e.finalize_weights(0)
        B, K, H, W = 2, 3, 240, 320
        hs = HO.hand_sides(B, K)
        m = THO.Machine()
        for t in range(3):
            o, detect = THO.step_and_check(e, m, TO.frames(9, t, B, H, W), hs, K)
            assert detect and not o['valid'].any() and not o['detected'].any() and not o['area'].any() and not o['lost'].any()
            assert np.all(o['center'] == 160.0) and np.all(o['scale'] == THO.FALLBACK_SCALE)
        assert e.counter('track_hands_tracked_steps') == 0 and e.counter('track_hands_detect_steps') == 3
    finally:
        e.close()


def test_profile_rows(eng):
    fr, hs = synth.make_batch(2, 2, 240, 320), HO.hand_sides(2, 4)
    eng.track_hands_reset()
    eng.set_profiling(1)
    try:
        o = eng.track_hands_step(fr, hs, 4)
        rows = [r[0] for r in eng.profile()]
        eng.infer_hands(fr, hs, 4, outputs=('coord3d',))
        hands = [r[0] for r in eng.profile()]
    finally:
        eng.set_profiling(0)
        eng.track_hands_reset()
    extra = ('track_hands_select', 'track_hands_box', 'kp_detect')
    assert [r for r in rows if r not in extra] == [r for r in hands if r not in extra]          # the same launches but the tracker's own
    assert rows.count('track_hands_select') == 1 and rows.count('track_hands_box') == 1 and rows.count('mask_grow_multi') == 1
    assert rows.index('mask_grow_multi') < rows.index('track_hands_select') < rows.index('crop_and_resize')
