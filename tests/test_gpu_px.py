"""Packed 8-bit frames through the real library: the crop / detection frame / normalise kernels on the interpreter
tests' cases and two large ones, both trackers against their uint8 forms on the repacked frames with every option in turn and a
different format each, the device-pointer forms on surfaces placed with hp3d_dev_alloc (one at a 1-byte offset, one at a padded
pitch), and one capture-shaped 1080p BGRA surface.  Every comparison is bit for bit (tests/helpers/px_oracle.py); the poison bytes of
the surfaces are the over-read check."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import px_oracle as PX                 # noqa: E402
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


@pytest.mark.parametrize("fmt", PX.FORMATS)
@pytest.mark.parametrize("H,W", PX.CROP_FRAMES)
def test_crop_bit_exact(gpu_engine, H, W, fmt):
    PX.assert_crop_cases(gpu_engine, H, W, fmt, big=256 if (H, W) == PX.CROP_FRAMES[1] else None)


@pytest.mark.parametrize("B,H,W,f,fmt,kind", PX.DOWNSCALE_CASES + [(1, 1080, 1920, 4, 'bgra', 7680), (1, 270, 482, 2, 'bgr', 'tight')])
def test_downscale_bit_exact(gpu_engine, B, H, W, f, fmt, kind):
    PX.assert_downscale_case(gpu_engine, B, H, W, f, fmt, kind)


# ---- the trackers, small -------------------------------------------------------------------------------------------------------------
B, H, W = 3, 64, 64


def _layout(fmt, i):
    """A different layout with each format: tight, an odd pitch with a misaligned base, a padded aligned pitch with unused rows."""
    pb = PX.pixel_bytes(fmt)
    return [dict(), dict(pitch=W * pb + 1, lead=1, gap_rows=1), dict(pitch=W * pb + 64, tail_rows=2)][i % 3]


def _surfaces(fmt, i, seed=21):
    return [PX.synth_surface(seed, t, B, H, W, fmt, **_layout(fmt, i)) for t in range(3)]


def _three_steps(e, step):
    """A fresh detect step; seeded so that frame 1 alone is lost, a tracked step; the detect step that follows.  [(outputs, rows)]"""
    e.track_reset()
    out = [PX.profile_rows(e, lambda: step(0))]
    c, s = TP.seed_boxes(B, H, W, [1])
    e.track_seed(c, s, H, W)
    out += [PX.profile_rows(e, lambda: step(1)), PX.profile_rows(e, lambda: step(2))]
    e.track_reset()
    return out


DEFAULTS = {'detect_scale': '1', 'track_partial_detect': '0', 'track_hands_partial_detect': '0', 'micro_batch': 'auto', 'track_redetect': '0',
            'hands_compact': '0'}


def _set(e, options, on):
    for k, v in options.items():
        e.set_option(k, v if on else DEFAULTS[k])


_ids = lambda o: '+'.join('%s=%s' % kv for kv in o.items()) if isinstance(o, dict) and o else ('defaults' if isinstance(o, dict) else str(o))
TRACK_OPTIONS = [({}, 'bgra'), ({'detect_scale': '2'}, 'bgr'), ({'track_partial_detect': '1'}, 'rgba'),
                 ({'detect_scale': '2', 'track_partial_detect': '1'}, 'argb'), ({'micro_batch': '2'}, 'abgr'),
                 ({'track_redetect': '2'}, 'rgb')]


@pytest.mark.parametrize("options,fmt", TRACK_OPTIONS, ids=_ids)
def test_track_steps_equal_the_uint8_steps(eng, options, fmt):
    e = eng
    hs = synth.hand_sides(B)
    surf = [s for s, _ in _surfaces(fmt, PX.FORMATS.index(fmt))]
    rgb = [PX.to_rgb(s, fmt) for s in surf]
    names = ('track_detect_steps', 'track_tracked_steps', 'detect_scale_steps', 'track_partial_frames_run', 'track_partial_frames_skipped')
    _set(e, options, True)
    try:
        n0, c0 = e.counter('crop_px_launches'), [e.counter(k) for k in names]
        px = _three_steps(e, lambda t: e.track_step_px(surf[t], fmt, hs, want_kpmap=True))
        n1, c1 = e.counter('crop_px_launches'), [e.counter(k) for k in names]
        u8 = _three_steps(e, lambda t: e.track_step_u8(rgb[t], hs, want_kpmap=True))
        assert e.counter('crop_px_launches') == n1
        c2 = [e.counter(k) for k in names]
    finally:
        _set(e, options, False)
    for t in range(3):
        PX.assert_equal_outputs(px[t][0], u8[t][0], (options, t))
        # the same launches, with the packed rows where the uint8 rows stand
        assert [r.replace('_px', '_u8') for r in px[t][1]] == u8[t][1], (options, t)
    assert [b - a for a, b in zip(c0, c1)] == [b - a for a, b in zip(c1, c2)]          # every counter the uint8 steps move
    (o0, r0), (o1, r1), (o2, r2) = px
    chunks = 2 if 'micro_batch' in options else 1
    assert np.all(o0['detected'] == 1) and o1['lost'].tolist() == [0, 1, 0] and not o1['detected'].any() and o2['detected'][1] == 1
    PX.assert_tracked_rows(r1, chunks)
    f = int(options.get('detect_scale', 1))
    assert ('downscale_px' if f > 1 else 'preprocess_px') in r0
    if f > 1:
        assert not [r for r in r0 + r2 if r.startswith('preprocess')] and r0.count('crop_and_resize_px') == chunks
    if 'track_partial_detect' in options:
        assert o2['detected'].tolist() == [0, 1, 0] and ('downscale_px_idx' if f > 1 else 'preprocess_px_idx') in r2
        assert r2.count('crop_and_resize_px') == chunks and 'preprocess_px' not in r2 and 'downscale_px' not in r2
    # one crop launch per chunk of every step that crops from the surface
    assert n1 - n0 == sum(r.count('crop_and_resize_px') for _, r in px) > 0


HANDS_OPTIONS = [({}, 'bgr'), ({'hands_compact': '1'}, 'abgr'), ({'hands_compact': '1', 'detect_scale': '2'}, 'bgra'),
                 ({'detect_scale': '2', 'micro_batch': '4'}, 'rgba'), ({'track_hands_partial_detect': '1'}, 'argb'),
                 ({'track_redetect': '2'}, 'rgb')]


@pytest.mark.parametrize("options,fmt", HANDS_OPTIONS, ids=_ids)
def test_track_hands_steps_equal_the_uint8_steps(eng, options, fmt):
    """K = 2: a fresh detect step; seeded with an absent slot in frame 0 and a slot far outside frame 1, a tracked step that loses that
    slot; the detect step behind it."""
    e, K = eng, 2
    hs = HO.hand_sides(B, K)
    surf = [s for s, _ in _surfaces(fmt, PX.FORMATS.index(fmt) + 1, seed=5)]
    rgb = [PX.to_rgb(s, fmt) for s in surf]
    mid = [H / 2.0, W / 2.0]
    sc = TP.seed_scale(H, W)
    center = np.array([[mid, [7.0, 9.0]], [mid, [-5000.0, -7000.0]], [mid, mid]], F32)
    scale = np.array([[sc, 3.0], [sc, 1.0], [sc, sc]], F32)
    valid = np.array([[1, 0], [1, 1], [1, 1]], np.int32)
    names = ('track_hands_detect_steps', 'track_hands_tracked_steps', 'detect_scale_steps', 'track_hands_partial_frames_run',
             'track_hands_partial_frames_skipped', 'hands_compact_waits')

    def three(step):
        e.track_hands_reset()
        out = [PX.profile_rows(e, lambda: step(0))]
        e.track_hands_seed(center, scale, valid, H, W)
        out += [PX.profile_rows(e, lambda: step(1)), PX.profile_rows(e, lambda: step(2))]
        e.track_hands_reset()
        return out

    _set(e, options, True)
    try:
        n0, c0 = e.counter('crop_px_launches'), [e.counter(k) for k in names]
        px = three(lambda t: e.track_hands_step_px(surf[t], fmt, hs, K, want_kpmap=True))
        n1, c1 = e.counter('crop_px_launches'), [e.counter(k) for k in names]
        u8 = three(lambda t: e.track_hands_step_u8(rgb[t], hs, K, want_kpmap=True))
        c2 = [e.counter(k) for k in names]
    finally:
        _set(e, options, False)
    for t in range(3):
        PX.assert_equal_outputs(px[t][0], u8[t][0], (options, t))
        assert [r.replace('_px', '_u8') for r in px[t][1]] == u8[t][1], (options, t)
    assert [b - a for a, b in zip(c0, c1)] == [b - a for a, b in zip(c1, c2)]
    o1, r1 = px[1]
    assert o1['valid'][0].tolist() == [1, 0] and o1['lost'][1].tolist() == [0, 1] and not o1['detected'].any()
    chunks = 2 if 'micro_batch' in options else 1
    PX.assert_tracked_rows(r1, chunks, idx='hands_compact' in options)
    assert n1 - n0 == sum(r.count('crop_and_resize_px') + r.count('crop_and_resize_idx_px') for _, r in px) > 0


def test_python_surface(eng):
    """track_hands(..., pixel_format=) and track(..., pixel_format=) on a region of interest of a wider BGRA surface equal the calls on
    the repacked uint8 frames."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    from hand3d_amd.utils.pixels import to_rgb
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = eng
    wide, _ = PX.synth_surface(5, 0, B, H + 20, W + 30, 'bgra')
    roi = wide[:, 10:10 + H, 20:20 + W]
    rgb = to_rgb(roi, 'bgra')
    assert np.array_equal(rgb, PX.to_rgb(roi, 'bgra')) and not roi.flags['C_CONTIGUOUS']
    try:
        for n, call in ((10, lambda image, **kw: net.track_hands(image, HO.hand_sides(B, 2), 2, **kw)),
                        (8, lambda image, **kw: net.track(image, synth.hand_sides(B), **kw))):
            got = []
            for image, kw in ((roi, {'pixel_format': 'bgra'}), (rgb, {})):
                net.track_reset()
                net.track_hands_reset()
                got.append(call(image, **kw))
            assert len(got[0]) == len(got[1]) == n
            for i in range(n):
                assert np.array_equal(got[0][i], got[1][i], equal_nan=True), (n, i)
    finally:
        net.track_reset()
        net.track_hands_reset()


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        e.set_option('detect_scale', '2')
        hs = synth.hand_sides(B)
        surf = [s for s, _ in _surfaces('abgr', 1)]
        px = _three_steps(e, lambda t: e.track_step_px(surf[t], 'abgr', hs))
        u8 = _three_steps(e, lambda t: e.track_step_u8(PX.to_rgb(surf[t], 'abgr'), hs))
        for t in range(3):
            PX.assert_equal_outputs(px[t][0], u8[t][0], t)
    finally:
        e.close()


# ---- the device-pointer forms ---------------------------------------------------------------------------------------------------------
STEP_SHAPES = lambda n: {'crop': ((n, 256, 256, 3), F32), 'scale': ((n, 1), F32), 'center': ((n, 2), F32), 'kpmap': ((n, 256, 256, 21), F32),
                         'coord3d': ((n, 21, 3), F32), 'kp_crop': ((n, 21, 2), np.int32), 'kp_hw': ((n, 21, 2), np.float64),
                         'confidence': ((n,), F32), 'lost': ((n,), np.int32), 'detected': ((n,), np.int32)}
HANDS_EXTRA = lambda n: {'valid': ((n,), np.int32), 'area': ((n,), np.int32), 'claimed': ((n,), np.int32)}


def _surface_on_device(e, view, alloc):
    """The whole allocation behind the view (lead byte, padding and their poison included) -> (buffer, the view's device address)."""
    buf = e.to_device(alloc)
    return buf, int(buf) + (view.ctypes.data - alloc.ctypes.data)


@pytest.mark.parametrize("options,fmt,layout", [({}, 'bgra', dict(pitch=W * 4 + 4, lead=1, gap_rows=1)),
                                                ({'detect_scale': '2', 'track_partial_detect': '1'}, 'bgr', dict(pitch=W * 3 + 64, tail_rows=1)),
                                                ({'detect_scale': '4'}, 'rgb', dict())],
                         ids=['bgra-1-byte-offset', 'bgr-padded-pitch-f2+partial', 'rgb-tight-f4'])
def test_dev_form_equals_host_form(eng, options, fmt, layout):
    e = eng
    hs = synth.hand_sides(B)
    pairs = [PX.synth_surface(21, t, B, H, W, fmt, **layout) for t in range(3)]
    shapes = STEP_SHAPES(B)
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    surf = [_surface_on_device(e, v, a) for v, a in pairs]
    d_hs = e.to_device(hs)
    pitch, fs = PX.layout(pairs[0][0])
    if 'lead' in layout:
        assert surf[0][1] % 4 == 1

    def dev_step(t):
        e.track_step_px_dev(B, H, W, surf[t][1], pitch, fs, fmt, d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

    _set(e, options, True)
    try:
        host = _three_steps(e, lambda t: e.track_step_px(pairs[t][0], fmt, hs, want_kpmap=True))
        dev = _three_steps(e, dev_step)
    finally:
        _set(e, options, False)
        for b in list(bufs.values()) + [d_hs] + [s[0] for s in surf]:
            b.free()
    for t in range(3):
        PX.assert_equal_outputs(dev[t][0], host[t][0], t)
        assert dev[t][1] == host[t][1], t


def test_hands_dev_form_equals_host_form(eng):
    e, K, fmt = eng, 2, 'argb'
    n = B * K
    hs = HO.hand_sides(B, K)
    view, alloc = PX.synth_surface(5, 0, B, H, W, fmt, pitch=W * 4 + 12, lead=1, gap_rows=2)
    shapes = dict(STEP_SHAPES(n), **HANDS_EXTRA(n))
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    buf, addr = _surface_on_device(e, view, alloc)
    d_hs = e.to_device(hs)
    pitch, fs = PX.layout(view)
    e.set_option('hands_compact', '1')
    try:
        e.track_hands_reset()
        host = e.track_hands_step_px(view, fmt, hs, K, want_kpmap=True)
        e.track_hands_reset()
        e.track_hands_step_px_dev(B, H, W, K, addr, pitch, fs, fmt, d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        for k, (s, dt) in shapes.items():
            assert np.array_equal(e.to_host(bufs[k], s, dt).reshape(host[k].shape), host[k], equal_nan=True), k
    finally:
        e.set_option('hands_compact', '0')
        e.track_hands_reset()
        for b in list(bufs.values()) + [d_hs, buf]:
            b.free()


def test_one_capture_shaped_1080p_surface(synth_weights):
    """B = 1, 1080 x 1920 BGRA at pitch 7680, detect_scale = 4: a detect step and a tracked step (seeded at the frame's centre with
    scale 1, a 256-pixel window: every keypoint stays inside the frame) through hp3d_track_step_px_dev equal hp3d_track_step_u8 on the
    repacked frame; the tracked step reads the surface with one launch, the packed crop."""
    from hand3d_amd import _lib
    Hh, Ww, pitch = 1080, 1920, 7680
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights(0)
        e.set_option('detect_scale', '4')
        hs = synth.hand_sides(1)
        pairs = [PX.synth_surface(5, t, 1, Hh, Ww, 'bgra', pitch=pitch) for t in range(2)]
        shapes = STEP_SHAPES(1)
        bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
        surf = [_surface_on_device(e, v, a) for v, a in pairs]
        d_hs = e.to_device(hs)
        seed = np.array([[Hh / 2.0, Ww / 2.0]], F32), np.array([1.0], F32)

        def dev_step(t):
            e.track_step_px_dev(1, Hh, Ww, surf[t][1], pitch, 0, 'bgra', d_hs, **{k: int(v) for k, v in bufs.items()})
            e.sync()
            return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

        def run(step):
            e.track_reset()
            out = [PX.profile_rows(e, lambda: step(0))]
            e.track_seed(seed[0], seed[1], Hh, Ww)
            out.append(PX.profile_rows(e, lambda: step(1)))
            return out

        names = ('track_detect_steps', 'track_tracked_steps', 'crop_px_launches')
        n0 = [e.counter(k) for k in names]
        px = run(dev_step)
        assert [e.counter(k) for k in names] == [n0[0] + 1, n0[1] + 1, n0[2] + 2]
        u8 = run(lambda t: e.track_step_u8(PX.to_rgb(pairs[t][0], 'bgra'), hs, want_kpmap=True))
        for t in range(2):
            PX.assert_equal_outputs(px[t][0], u8[t][0], t)
        r0 = px[0][1]
        assert 'downscale_px' in r0 and r0.count('crop_and_resize_px') == 1 and not [r for r in r0 if r.startswith('preprocess')]
        PX.assert_tracked_rows(px[1][1])
        assert not px[1][0]['lost'].any() and not px[1][0]['detected'].any()
    finally:
        e.close()
