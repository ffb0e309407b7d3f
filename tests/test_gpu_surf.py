"""A batch of separate surfaces, formats mixed through the real library: the per-op kernels on the interpreter tests'
cases and two large ones, both trackers against their uint8 forms on the stacked RGB frames with every option in turn and a different
mix of formats and layouts each, the device-pointer forms on surfaces placed with hp3d_dev_alloc in separate allocations handed over
in descending order of addresses, and ten device steps that reuse the table staging without a host synchronise.  Every comparison is
bit for bit (tests/helpers/surf_oracle.py); the poison bytes of the surfaces are the over-read check."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import px_oracle as PX                 # noqa: E402
import surf_oracle as SF               # noqa: E402
import track_partial_oracle as TP      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    yield gpu_engine
    gpu_engine.track_reset()
    gpu_engine.track_hands_reset()


# ---- per-op -----------------------------------------------------------------------------------------------------------------------------
def test_surf_to_rgb(gpu_engine):
    SF.assert_to_rgb_cases(gpu_engine)


@pytest.mark.parametrize("H,W", PX.CROP_FRAMES)
def test_crop_bit_exact(gpu_engine, H, W):
    SF.assert_crop_cases(gpu_engine, H, W, big=256 if (H, W) == PX.CROP_FRAMES[1] else None)


@pytest.mark.parametrize("f", SF.DOWNSCALE_FACTORS)
@pytest.mark.parametrize("name,specs,H,W", SF.DOWNSCALE_BATCHES, ids=[c[0] for c in SF.DOWNSCALE_BATCHES])
def test_downscale_bit_exact(gpu_engine, name, specs, H, W, f):
    SF.assert_downscale_case(gpu_engine, specs(W), H, W, f)


def test_downscale_1080p_bgra_beside_nv12(gpu_engine):
    """1 x 1080 x 1920 bgra at pitch 7680 plus 1 x 1080 x 1920 nv12 at pitch 2048 in one batch, f = 4."""
    SF.assert_downscale_case(gpu_engine, [('bgra', dict(pitch=7680)), ('nv12', dict(pitch=2048))], 1080, 1920, 4, idx=(1,))


def test_downscale_270x482_bgr(gpu_engine):
    """270 x 482 bgr, tight, f = 2: a ragged last window row is absent, the pitch (1446) is off the 4-byte grid."""
    SF.assert_downscale_case(gpu_engine, [('bgr', dict())], 270, 482, 2, idx=(0,))


# ---- the trackers, small -------------------------------------------------------------------------------------------------------------
B, H, W = 3, 64, 64

DEFAULTS = {'detect_scale': '1', 'track_partial_detect': '0', 'track_hands_partial_detect': '0', 'micro_batch': 'auto', 'track_redetect': '0',
            'hands_compact': '0'}


def _set(e, options, on):
    for k, v in options.items():
        e.set_option(k, v if on else DEFAULTS[k])


def _three_steps(e, step):
    """A fresh detect step; seeded so that frame 1 alone is lost, a tracked step; the detect step that follows.  [(outputs, rows)]"""
    e.track_reset()
    out = [SF.profile_rows(e, lambda: step(0))]
    c, s = TP.seed_boxes(B, H, W, [1])
    e.track_seed(c, s, H, W)
    out += [SF.profile_rows(e, lambda: step(1)), SF.profile_rows(e, lambda: step(2))]
    e.track_reset()
    return out


_ids = lambda o: '+'.join('%s=%s' % kv for kv in o.items()) if isinstance(o, dict) and o else ('defaults' if isinstance(o, dict) else None)
# the option sets of tests/test_gpu_px.py, each with its own mix of formats and layouts (an int: the record names that surface again)
TRACK_OPTIONS = [
    ({}, [('bgra', dict()), ('nv12', dict(pitch=W + 32)), ('bgr', dict(pitch=W * 3 + 1, lead=1))]),
    ({'detect_scale': '2'}, [('nv12', dict()), ('rgba', dict(pitch=W * 4 + 4, lead=1)), ('nv12', dict(pitch=W + 1))]),
    ({'track_partial_detect': '1'}, [('abgr', dict()), ('rgb', dict(pitch=W * 3 + 64)), ('argb', dict(lead=1))]),
    ({'detect_scale': '2', 'track_partial_detect': '1'}, [('bgr', dict()), ('nv12', dict(pitch=W + 64)), ('bgra', dict(pitch=W * 4 + 16))]),
    ({'micro_batch': '2'}, [('rgba', dict()), 0, ('nv12', dict(pitch=W + 2, lead=1))]),
    ({'track_redetect': '2'}, [('rgb', dict(pitch=W * 3 + 1, lead=1)), ('bgr', dict()), ('argb', dict(pitch=W * 4 + 64))]),
]
HANDS_OPTIONS = [
    ({}, [('nv12', dict()), ('bgr', dict()), ('bgra', dict(pitch=W * 4 + 4, lead=1))]),
    ({'hands_compact': '1'}, [('abgr', dict(lead=1)), ('nv12', dict(pitch=W + 32)), ('rgb', dict())]),
    ({'hands_compact': '1', 'detect_scale': '2'}, [('bgra', dict(pitch=W * 4 + 64)), ('rgba', dict()), ('nv12', dict(pitch=W + 1))]),
    ({'detect_scale': '2', 'micro_batch': '4'}, [('rgb', dict()), ('argb', dict(pitch=W * 4 + 4)), ('bgr', dict(pitch=W * 3 + 1, lead=1))]),
    ({'track_hands_partial_detect': '1'}, [('nv12', dict(pitch=W + 2, lead=1)), 0, ('bgra', dict())]),
    ({'track_redetect': '2'}, [('bgr', dict(pitch=W * 3 + 64)), ('abgr', dict()), ('rgba', dict(lead=1))]),
]


def test_the_option_sets_are_those_of_the_packed_tests_and_half_hold_nv12():
    import test_gpu_px as GP
    for mine, theirs in ((TRACK_OPTIONS, GP.TRACK_OPTIONS), (HANDS_OPTIONS, GP.HANDS_OPTIONS)):
        assert [o for o, _ in mine] == [o for o, _ in theirs]
        mixes = [tuple(str(s) for s in specs) for _, specs in mine]
        assert len(set(mixes)) == len(mixes) and sum(any(not isinstance(s, int) and s[0] == 'nv12' for s in specs) for _, specs in mine) >= 3


def _batches(specs, seed):
    return [SF.synth_batch(seed, t, specs, H, W) for t in range(3)]


@pytest.mark.parametrize("options,specs", TRACK_OPTIONS, ids=_ids)
def test_track_steps_equal_the_uint8_steps(eng, options, specs):
    e = eng
    hs = synth.hand_sides(B)
    bat = _batches(specs, 21)
    rgb = [SF.to_rgb(b) for b in bat]
    names = ('track_detect_steps', 'track_tracked_steps', 'detect_scale_steps', 'track_partial_frames_run', 'track_partial_frames_skipped')
    _set(e, options, True)
    try:
        n0, c0 = e.counter('crop_surf_launches'), [e.counter(k) for k in names]
        sf = _three_steps(e, lambda t: e.track_step_surf(bat[t].surfaces, bat[t].formats, hs, want_kpmap=True))
        n1, c1 = e.counter('crop_surf_launches'), [e.counter(k) for k in names]
        u8 = _three_steps(e, lambda t: e.track_step_u8(rgb[t], hs, want_kpmap=True))
        assert e.counter('crop_surf_launches') == n1
        c2 = [e.counter(k) for k in names]
    finally:
        _set(e, options, False)
    for t in range(3):
        SF.assert_equal_outputs(sf[t][0], u8[t][0], (options, t))
        assert SF.u8_rows(sf[t][1]) == u8[t][1], (options, t)          # the same launches, the surface rows where the uint8 rows stand
    assert [b - a for a, b in zip(c0, c1)] == [b - a for a, b in zip(c1, c2)]          # every counter the uint8 steps move
    (o0, r0), (o1, r1), (o2, r2) = sf
    chunks = 2 if 'micro_batch' in options else 1
    assert np.all(o0['detected'] == 1) and o1['lost'].tolist() == [0, 1, 0] and not o1['detected'].any() and o2['detected'][1] == 1
    SF.assert_tracked_rows(r1, chunks)
    f = int(options.get('detect_scale', 1))
    assert ('downscale_surf' if f > 1 else 'preprocess_surf') in r0
    if f > 1:
        assert not [r for r in r0 + r2 if r.startswith('preprocess')] and r0.count('crop_and_resize_surf') == chunks
    if 'track_partial_detect' in options:
        assert o2['detected'].tolist() == [0, 1, 0] and ('downscale_surf_idx' if f > 1 else 'preprocess_surf_idx') in r2
        assert r2.count('crop_and_resize_surf') == chunks and 'preprocess_surf' not in r2 and 'downscale_surf' not in r2
    # one crop launch per chunk of every step that crops from the surfaces
    assert n1 - n0 == sum(r.count('crop_and_resize_surf') for _, r in sf) > 0 and n1 - n0 >= chunks


@pytest.mark.parametrize("options,specs", HANDS_OPTIONS, ids=_ids)
def test_track_hands_steps_equal_the_uint8_steps(eng, options, specs):
    """K = 2: a fresh detect step; seeded with an absent slot in frame 0 and a slot far outside frame 1, a tracked step that loses that
    slot; the detect step behind it."""
    e, K = eng, 2
    hs = HO.hand_sides(B, K)
    bat = _batches(specs, 5)
    rgb = [SF.to_rgb(b) for b in bat]
    mid = [H / 2.0, W / 2.0]
    sc = TP.seed_scale(H, W)
    center = np.array([[mid, [7.0, 9.0]], [mid, [-5000.0, -7000.0]], [mid, mid]], F32)
    scale = np.array([[sc, 3.0], [sc, 1.0], [sc, sc]], F32)
    valid = np.array([[1, 0], [1, 1], [1, 1]], np.int32)
    names = ('track_hands_detect_steps', 'track_hands_tracked_steps', 'detect_scale_steps', 'track_hands_partial_frames_run',
             'track_hands_partial_frames_skipped', 'hands_compact_waits')

    def three(step):
        e.track_hands_reset()
        out = [SF.profile_rows(e, lambda: step(0))]
        e.track_hands_seed(center, scale, valid, H, W)
        out += [SF.profile_rows(e, lambda: step(1)), SF.profile_rows(e, lambda: step(2))]
        e.track_hands_reset()
        return out

    _set(e, options, True)
    try:
        n0, c0 = e.counter('crop_surf_launches'), [e.counter(k) for k in names]
        sf = three(lambda t: e.track_hands_step_surf(bat[t].surfaces, bat[t].formats, hs, K, want_kpmap=True))
        n1, c1 = e.counter('crop_surf_launches'), [e.counter(k) for k in names]
        u8 = three(lambda t: e.track_hands_step_u8(rgb[t], hs, K, want_kpmap=True))
        c2 = [e.counter(k) for k in names]
    finally:
        _set(e, options, False)
    for t in range(3):
        SF.assert_equal_outputs(sf[t][0], u8[t][0], (options, t))
        assert SF.u8_rows(sf[t][1]) == u8[t][1], (options, t)
    assert [b - a for a, b in zip(c0, c1)] == [b - a for a, b in zip(c1, c2)]
    o1, r1 = sf[1]
    assert o1['valid'][0].tolist() == [1, 0] and o1['lost'][1].tolist() == [0, 1] and not o1['detected'].any()
    chunks = 2 if 'micro_batch' in options else 1
    SF.assert_tracked_rows(r1, chunks, idx='hands_compact' in options)
    assert n1 - n0 == sum(r.count('crop_and_resize_surf') + r.count('crop_and_resize_idx_surf') for _, r in sf) > 0


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        e.set_option('detect_scale', '2')
        hs = synth.hand_sides(B)
        bat = _batches([('abgr', dict(lead=1)), ('nv12', dict(pitch=W + 32)), ('bgr', dict())], 21)
        sf = _three_steps(e, lambda t: e.track_step_surf(bat[t].surfaces, bat[t].formats, hs))
        u8 = _three_steps(e, lambda t: e.track_step_u8(SF.to_rgb(bat[t]), hs))
        for t in range(3):
            SF.assert_equal_outputs(sf[t][0], u8[t][0], t)
            assert SF.u8_rows(sf[t][1]) == u8[t][1], t
    finally:
        e.close()


# ---- the device-pointer forms ---------------------------------------------------------------------------------------------------------
STEP_SHAPES = lambda n: {'crop': ((n, 256, 256, 3), F32), 'scale': ((n, 1), F32), 'center': ((n, 2), F32), 'kpmap': ((n, 256, 256, 21), F32),
                         'coord3d': ((n, 21, 3), F32), 'kp_crop': ((n, 21, 2), np.int32), 'kp_hw': ((n, 21, 2), np.float64),
                         'confidence': ((n,), F32), 'lost': ((n,), np.int32), 'detected': ((n,), np.int32)}
HANDS_EXTRA = lambda n: {'valid': ((n,), np.int32), 'area': ((n,), np.int32), 'claimed': ((n,), np.int32)}
# three surfaces in three separate allocations (the NV12 one: a fourth for its chroma plane): one at a 1-byte offset, one at a padded
# pitch, one NV12
DEV_SPECS = [('bgra', dict(pitch=W * 4 + 4, lead=1)), ('bgr', dict(pitch=W * 3 + 64)), ('nv12', dict(pitch=W + 32))]


def _on_device(e, bat):
    placed = [SF.on_device(e, b) for b in bat]
    for _, recs in placed:
        first = [r[0] for r in recs]
        assert first == sorted(first, reverse=True) and recs[0][0] % 4 == 1          # descending addresses; the 1-byte offset
    return placed


def test_dev_form_equals_host_form(eng):
    """Single-hand, detect_scale = 2 plus partial detect, over the three steps: results and rows equal the host form's."""
    e = eng
    options = {'detect_scale': '2', 'track_partial_detect': '1'}
    hs = synth.hand_sides(B)
    bat = _batches(DEV_SPECS, 21)
    shapes = STEP_SHAPES(B)
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    placed = _on_device(e, bat)
    d_hs = e.to_device(hs)

    def dev_step(t):
        e.track_step_surf_dev(B, H, W, placed[t][1], d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

    _set(e, options, True)
    try:
        host = _three_steps(e, lambda t: e.track_step_surf(bat[t].surfaces, bat[t].formats, hs, want_kpmap=True))
        dev = _three_steps(e, dev_step)
    finally:
        _set(e, options, False)
        for b in list(bufs.values()) + [d_hs] + [x for p in placed for x in p[0]]:
            b.free()
    for t in range(3):
        SF.assert_equal_outputs(dev[t][0], host[t][0], t)
        assert dev[t][1] == host[t][1], t
    assert host[1][0]['lost'].tolist() == [0, 1, 0] and 'downscale_surf_idx' in host[2][1]


def test_hands_dev_form_equals_host_form(eng):
    """Multi-hand with hands_compact over the three steps: results and rows equal the host form's."""
    e, K = eng, 2
    n = B * K
    hs = HO.hand_sides(B, K)
    bat = _batches(DEV_SPECS, 5)
    shapes = dict(STEP_SHAPES(n), **HANDS_EXTRA(n))
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    placed = _on_device(e, bat)
    d_hs = e.to_device(hs)
    mid = [H / 2.0, W / 2.0]
    sc = TP.seed_scale(H, W)
    center = np.array([[mid, [7.0, 9.0]], [mid, [-5000.0, -7000.0]], [mid, mid]], F32)
    scale = np.array([[sc, 3.0], [sc, 1.0], [sc, sc]], F32)
    valid = np.array([[1, 0], [1, 1], [1, 1]], np.int32)

    def dev_step(t):
        e.track_hands_step_surf_dev(B, H, W, K, placed[t][1], d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

    def three(step):
        e.track_hands_reset()
        out = [SF.profile_rows(e, lambda: step(0))]
        e.track_hands_seed(center, scale, valid, H, W)
        out += [SF.profile_rows(e, lambda: step(1)), SF.profile_rows(e, lambda: step(2))]
        e.track_hands_reset()
        return out

    e.set_option('hands_compact', '1')
    try:
        host = three(lambda t: e.track_hands_step_surf(bat[t].surfaces, bat[t].formats, hs, K, want_kpmap=True))
        dev = three(dev_step)
    finally:
        e.set_option('hands_compact', '0')
        for b in list(bufs.values()) + [d_hs] + [x for p in placed for x in p[0]]:
            b.free()
    for t in range(3):
        for k, (s, dt) in shapes.items():
            assert np.array_equal(dev[t][0][k].reshape(host[t][0][k].shape), host[t][0][k], equal_nan=True), (t, k)
        assert dev[t][1] == host[t][1], t
    SF.assert_tracked_rows(host[1][1], idx=True)


def test_table_staging_under_reuse(synth_weights):
    """Ten consecutive device tracked steps that alternate between two sets of surface addresses, with no host synchronise in between
    and each step's outputs in device buffers of its own, read after one final hp3d_sync: equal to the same ten steps with a synchronise
    after each.  A later step's table that overwrote an earlier one's before it was used would crop the wrong surfaces.
    Every step is a tracked one (asserted), whatever random-weight keypoints say: a step's box is centred on keypoint 12, which lies
    inside the previous crop window; with track_margin = 0.01 every derived window is the smallest the box rule allows, 50 pixels, and
    the seed's is 51.2 (scale 5), so keypoint 12 moves by at most 25.6 pixels a step -- 256 in ten, from the centre of a 720 x 1280
    frame: it never leaves the frame, which is the only way to lose a hand here."""
    from hand3d_amd import _lib
    Bn, Hh, Ww, steps = 2, 720, 1280, 10
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        e.set_option('track_margin', '0.01')
        sets = [SF.random_batch(11, [('bgra', dict(pitch=Ww * 4 + 64)), ('nv12', dict(pitch=Ww + 768))], Hh, Ww),
                SF.random_batch(12, [('nv12', dict()), ('bgr', dict(pitch=Ww * 3 + 1, lead=1))], Hh, Ww)]
        placed = [SF.on_device(e, s) for s in sets]
        d_hs = e.to_device(synth.hand_sides(Bn))
        shapes = {k: v for k, v in STEP_SHAPES(Bn).items() if k not in ('crop', 'kpmap')}
        bufs = [{k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()} for _ in range(steps)]
        seed = np.tile(np.array([Hh / 2.0, Ww / 2.0], F32), (Bn, 1)), np.full(Bn, 5.0, F32)

        def run(sync_each):
            e.track_seed(seed[0], seed[1], Hh, Ww)
            n0 = e.counter('track_tracked_steps')
            for t in range(steps):
                e.track_step_surf_dev(Bn, Hh, Ww, placed[t % 2][1], d_hs, **{k: int(v) for k, v in bufs[t].items()})
                if sync_each:
                    e.sync()
            e.sync()
            assert e.counter('track_tracked_steps') == n0 + steps, "a step detected"
            return [{k: e.to_host(bufs[t][k], s, dt) for k, (s, dt) in shapes.items()} for t in range(steps)]

        want = run(True)
        got = run(False)
        for t in range(steps):
            SF.assert_equal_outputs(got[t], want[t], t)
            assert not want[t]['lost'].any() and not want[t]['detected'].any()
        # the two sets hold different pictures: consecutive steps do differ
        assert not np.array_equal(want[0]['coord3d'], want[1]['coord3d'])
    finally:
        e.close()
