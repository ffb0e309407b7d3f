"""NV12 frames through the real library: the colour rule on all 2^24 (Y, U, V) triples, the crop / detection frame /
normalise kernels on the interpreter tests' cases, both trackers against their uint8 forms on the converted frames with every option
in turn, the device-pointer forms on surfaces placed with hp3d_dev_alloc, and one decoder-shaped 1080p surface.  Every comparison is
bit for bit (tests/helpers/nv12_oracle.py)."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import nv12_oracle as NV               # noqa: E402
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


@pytest.fixture(scope='module')
def all_triples():
    return NV.exhaustive_planes()


@pytest.mark.parametrize("matrix", NV.MATRICES)
def test_nv12_to_rgb_all_triples(gpu_engine, all_triples, matrix):
    y, uv = all_triples
    gpu_engine.set_option('nv12_matrix', matrix)
    try:
        got = gpu_engine.nv12_to_rgb(y, uv)
    finally:
        gpu_engine.set_option('nv12_matrix', 'bt709')
    for b in range(4):          # (frame by frame: the expected value of 4 M pixels at a time)
        assert np.array_equal(got[b:b + 1], NV.to_rgb(y[b:b + 1], uv[b:b + 1], 2048, matrix)), (matrix, b)
    if matrix == NV.MATRICES[0]:          # the planes do hold every triple once: 65536 pairs x 256 luma values
        key = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(uv[:, :, 0::2], 2, 1), 2, 2).astype(np.int64) << 8) | np.repeat(np.repeat(uv[:, :, 1::2], 2, 1), 2, 2)
        assert np.array_equal(np.sort(key.reshape(-1)), np.arange(1 << 24))


@pytest.mark.parametrize("H,W", NV.CROP_FRAMES)
def test_crop_bit_exact(gpu_engine, H, W):
    for i, pitch in enumerate(NV.crop_pitches(W)):
        NV.assert_crop_cases(gpu_engine, H, W, pitch, NV.MATRICES[i % 4], crop=256 if i == 0 else 8)


@pytest.mark.parametrize("B,H,W,f,pitch", NV.DOWNSCALE_CASES + [(1, 1080, 1920, 4, 2048), (1, 270, 482, 2, 482)])
def test_downscale_bit_exact(gpu_engine, B, H, W, f, pitch):
    NV.assert_downscale_case(gpu_engine, B, H, W, f, pitch, NV.MATRICES[(f + pitch) % 4])


# ---- the trackers, small -------------------------------------------------------------------------------------------------------------
B, H, W, PITCH = 3, 32, 32, 40


def _planes(t, seed=21):
    return NV.synth_planes(seed, t, B, H, W, pitch=PITCH, gap_rows=1, tail_rows=2)


def _three_steps(e, step):
    """A fresh detect step; seeded so that frame 1 alone is lost, a tracked step; the detect step that follows.  [(outputs, rows)]"""
    e.track_reset()
    out = [NV.profile_rows(e, lambda: step(0))]
    c, s = TP.seed_boxes(B, H, W, [1])
    e.track_seed(c, s, H, W)
    out += [NV.profile_rows(e, lambda: step(1)), NV.profile_rows(e, lambda: step(2))]
    e.track_reset()
    return out


def _set(e, options, on):
    defaults = {'detect_scale': '1', 'track_partial_detect': '0', 'micro_batch': 'auto', 'track_redetect': '0', 'hands_compact': '0',
                'nv12_matrix': 'bt709'}
    for k, v in options.items():
        e.set_option(k, v if on else defaults[k])


TRACK_OPTIONS = [{}, {'detect_scale': '2'}, {'track_partial_detect': '1'}, {'detect_scale': '2', 'track_partial_detect': '1'},
                 {'micro_batch': '2'}, {'micro_batch': '2', 'track_partial_detect': '1'}, {'track_redetect': '2'}, {'nv12_matrix': 'bt601_full'}]


@pytest.mark.parametrize("options", TRACK_OPTIONS, ids=lambda o: '+'.join('%s=%s' % kv for kv in o.items()) or 'defaults')
def test_track_steps_equal_the_uint8_steps(eng, options):
    e = eng
    hs = synth.hand_sides(B)
    matrix = options.get('nv12_matrix', 'bt709')
    planes = [_planes(t) for t in range(3)]
    rgb = [NV.to_rgb(y, uv, W, matrix) for y, uv in planes]
    _set(e, options, True)
    try:
        n0 = e.counter('crop_nv12_launches')
        nv = _three_steps(e, lambda t: e.track_step_nv12(planes[t][0], planes[t][1], hs, W=W, want_kpmap=True))
        n1 = e.counter('crop_nv12_launches')
        u8 = _three_steps(e, lambda t: e.track_step_u8(rgb[t], hs, want_kpmap=True))
        assert e.counter('crop_nv12_launches') == n1
    finally:
        _set(e, options, False)
    for t in range(3):
        NV.assert_equal_outputs(nv[t][0], u8[t][0], (options, t))
        # the same launches, with the NV12 rows where the uint8 rows stand
        assert [r.replace('_nv12', '_u8') for r in nv[t][1]] == u8[t][1], (options, t)
    (o0, r0), (o1, r1), (o2, r2) = nv
    chunks = 2 if 'micro_batch' in options else 1
    assert np.all(o0['detected'] == 1) and o1['lost'].tolist() == [0, 1, 0] and not o1['detected'].any() and o2['detected'][1] == 1
    NV.assert_tracked_rows(r1, chunks)
    f = int(options.get('detect_scale', 1))
    assert ('downscale_nv12' if f > 1 else 'preprocess_nv12') in r0
    if f > 1:
        assert not [r for r in r0 + r2 if r.startswith('preprocess')] and r0.count('crop_and_resize_nv12') == chunks
    if 'track_partial_detect' in options:
        assert o2['detected'].tolist() == [0, 1, 0] and ('downscale_nv12_idx' if f > 1 else 'preprocess_nv12_idx') in r2
        assert r2.count('crop_and_resize_nv12') == chunks and 'preprocess_nv12' not in r2 and 'downscale_nv12' not in r2
    # one crop launch per chunk of every step that crops from the planes
    assert n1 - n0 == sum(r.count('crop_and_resize_nv12') for _, r in nv) > 0


HANDS_OPTIONS = [{}, {'hands_compact': '1'}, {'hands_compact': '1', 'detect_scale': '2'}, {'detect_scale': '2', 'micro_batch': '4'}]


@pytest.mark.parametrize("options", HANDS_OPTIONS, ids=lambda o: '+'.join('%s=%s' % kv for kv in o.items()) or 'defaults')
def test_track_hands_steps_equal_the_uint8_steps(eng, options):
    """K = 2: a fresh detect step; seeded with an absent slot in frame 0 and a slot far outside frame 1, a tracked step that loses that
    slot; the detect step behind it."""
    e, K = eng, 2
    hs = HO.hand_sides(B, K)
    planes = [_planes(t, seed=5) for t in range(3)]
    rgb = [NV.to_rgb(y, uv, W, 'bt709') for y, uv in planes]
    mid = [H / 2.0, W / 2.0]
    center = np.array([[mid, [7.0, 9.0]], [mid, [-5000.0, -7000.0]], [mid, mid]], F32)
    scale = np.array([[10.0, 3.0], [10.0, 1.0], [10.0, 10.0]], F32)
    valid = np.array([[1, 0], [1, 1], [1, 1]], np.int32)

    def three(step):
        e.track_hands_reset()
        out = [NV.profile_rows(e, lambda: step(0))]
        e.track_hands_seed(center, scale, valid, H, W)
        out += [NV.profile_rows(e, lambda: step(1)), NV.profile_rows(e, lambda: step(2))]
        e.track_hands_reset()
        return out

    _set(e, options, True)
    try:
        n0 = e.counter('crop_nv12_launches')
        nv = three(lambda t: e.track_hands_step_nv12(planes[t][0], planes[t][1], hs, K, W=W, want_kpmap=True))
        n1 = e.counter('crop_nv12_launches')
        u8 = three(lambda t: e.track_hands_step_u8(rgb[t], hs, K, want_kpmap=True))
    finally:
        _set(e, options, False)
    for t in range(3):
        NV.assert_equal_outputs(nv[t][0], u8[t][0], (options, t))
    o1, r1 = nv[1]
    assert o1['valid'][0].tolist() == [1, 0] and o1['lost'][1].tolist() == [0, 1] and not o1['detected'].any()
    chunks = 2 if 'micro_batch' in options else 1
    if 'hands_compact' in options:
        NV.assert_tracked_rows(r1, chunks, idx=True)
    else:
        NV.assert_tracked_rows(r1, chunks)
    assert n1 - n0 == sum(r.count('crop_and_resize_nv12') + r.count('crop_and_resize_idx_nv12') for _, r in nv) > 0


def test_python_surface(eng):
    """track_hands(image=(y, uv)) and track(image=[y, uv]) equal the calls on the converted uint8 frames."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    from hand3d_amd.utils.nv12 import nv12_to_rgb
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = eng
    y, uv = NV.synth_planes(5, 0, B, H, W)
    rgb = nv12_to_rgb(y, uv, matrix='bt601')
    try:
        for n, call in ((10, lambda image: net.track_hands(image, HO.hand_sides(B, 2), 2, nv12_matrix='bt601')),
                        (8, lambda image: net.track(image, synth.hand_sides(B), nv12_matrix='bt601'))):
            got = []
            for image in ((y, uv), [y, uv], rgb):
                net.track_reset()
                net.track_hands_reset()
                got.append(call(image))
            assert len(got[0]) == len(got[1]) == len(got[2]) == n
            for i in range(n):
                assert np.array_equal(got[0][i], got[2][i], equal_nan=True) and np.array_equal(got[1][i], got[2][i], equal_nan=True), (n, i)
    finally:
        eng.set_option('nv12_matrix', 'bt709')
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
        planes = [_planes(t) for t in range(3)]
        nv = _three_steps(e, lambda t: e.track_step_nv12(planes[t][0], planes[t][1], hs, W=W))
        u8 = _three_steps(e, lambda t: e.track_step_u8(NV.to_rgb(planes[t][0], planes[t][1], W, 'bt709'), hs))
        for t in range(3):
            NV.assert_equal_outputs(nv[t][0], u8[t][0], t)
    finally:
        e.close()


# ---- the device-pointer forms ---------------------------------------------------------------------------------------------------------
STEP_SHAPES = lambda n: {'crop': ((n, 256, 256, 3), F32), 'scale': ((n, 1), F32), 'center': ((n, 2), F32), 'kpmap': ((n, 256, 256, 21), F32),
                         'coord3d': ((n, 21, 3), F32), 'kp_crop': ((n, 21, 2), np.int32), 'kp_hw': ((n, 21, 2), np.float64),
                         'confidence': ((n,), F32), 'lost': ((n,), np.int32), 'detected': ((n,), np.int32)}
HANDS_EXTRA = lambda n: {'valid': ((n,), np.int32), 'area': ((n,), np.int32), 'claimed': ((n,), np.int32)}


def _surface_on_device(e, y, uv):
    """The whole allocation behind the two views (padding and its poison included) -> (buffer, y address, uv address)."""
    base = y.base
    assert base is not None and uv.base is base
    buf = e.to_device(base)
    at = lambda v: int(buf) + (v.ctypes.data - base.ctypes.data)
    return buf, at(y), at(uv)


@pytest.mark.parametrize("options", [{}, {'detect_scale': '2', 'track_partial_detect': '1'}], ids=['defaults', 'f2+partial'])
def test_dev_form_equals_host_form(eng, options):
    e = eng
    hs = synth.hand_sides(B)
    planes = [_planes(t) for t in range(3)]
    shapes = STEP_SHAPES(B)
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    surf = [_surface_on_device(e, y, uv) for y, uv in planes]
    d_hs = e.to_device(hs)
    fs = planes[0][0].strides[0]

    def dev_step(t):
        e.track_step_nv12_dev(B, H, W, surf[t][1], surf[t][2], PITCH, fs, d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

    _set(e, options, True)
    try:
        host = _three_steps(e, lambda t: e.track_step_nv12(planes[t][0], planes[t][1], hs, W=W, want_kpmap=True))
        dev = _three_steps(e, dev_step)
    finally:
        _set(e, options, False)
        for b in list(bufs.values()) + [d_hs] + [s[0] for s in surf]:
            b.free()
    for t in range(3):
        NV.assert_equal_outputs(dev[t][0], host[t][0], t)
        assert dev[t][1] == host[t][1], t


def test_hands_dev_form_equals_host_form(eng):
    e, K = eng, 2
    n = B * K
    hs = HO.hand_sides(B, K)
    y, uv = _planes(0, seed=5)
    shapes = dict(STEP_SHAPES(n), **HANDS_EXTRA(n))
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    surf = _surface_on_device(e, y, uv)
    d_hs = e.to_device(hs)
    e.set_option('hands_compact', '1')
    try:
        e.track_hands_reset()
        host = e.track_hands_step_nv12(y, uv, hs, K, W=W, want_kpmap=True)
        e.track_hands_reset()
        e.track_hands_step_nv12_dev(B, H, W, K, surf[1], surf[2], PITCH, y.strides[0], d_hs, **{k: int(v) for k, v in bufs.items()})
        e.sync()
        for k, (s, dt) in shapes.items():
            assert np.array_equal(e.to_host(bufs[k], s, dt).reshape(host[k].shape), host[k], equal_nan=True), k
    finally:
        e.set_option('hands_compact', '0')
        e.track_hands_reset()
        for b in list(bufs.values()) + [d_hs, surf[0]]:
            b.free()


def test_one_decoder_shaped_1080p_surface(synth_weights):
    """B = 1, 1080 x 1920 at pitch 2048 with the chroma plane at row 1088, detect_scale = 4: a detect step and two tracked steps (seeded
    at the frame's centre with scale 1, a 256-pixel window: every keypoint stays inside the frame) through hp3d_track_step_nv12_dev equal
    hp3d_track_step_u8 on the converted frame; the tracked steps read the surface with one launch, the NV12 crop."""
    from hand3d_amd import _lib
    Hh, Ww, pitch = 1080, 1920, 2048
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights(0)
        e.set_option('detect_scale', '4')
        hs = synth.hand_sides(1)
        planes = [NV.synth_planes(5, t, 1, Hh, Ww, pitch=pitch, gap_rows=8) for t in range(3)]
        assert planes[0][1].ctypes.data - planes[0][0].ctypes.data == 1088 * pitch
        shapes = STEP_SHAPES(1)
        bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
        surf = [_surface_on_device(e, y, uv) for y, uv in planes]
        d_hs = e.to_device(hs)
        seed = np.array([[Hh / 2.0, Ww / 2.0]], F32), np.array([1.0], F32)

        def dev_step(t):
            e.track_step_nv12_dev(1, Hh, Ww, surf[t][1], surf[t][2], pitch, 0, d_hs, **{k: int(v) for k, v in bufs.items()})
            e.sync()
            return {k: e.to_host(bufs[k], s, dt) for k, (s, dt) in shapes.items()}

        def run(step):
            e.track_reset()
            out = [NV.profile_rows(e, lambda: step(0))]
            e.track_seed(seed[0], seed[1], Hh, Ww)
            out += [NV.profile_rows(e, lambda: step(1)), NV.profile_rows(e, lambda: step(2))]
            return out

        n0 = (e.counter('track_detect_steps'), e.counter('track_tracked_steps'), e.counter('crop_nv12_launches'))
        nv = run(dev_step)
        assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps'), e.counter('crop_nv12_launches')) == (n0[0] + 1, n0[1] + 2, n0[2] + 3)
        u8 = run(lambda t: e.track_step_u8(NV.to_rgb(planes[t][0], planes[t][1], Ww, 'bt709'), hs, want_kpmap=True))
        for t in range(3):
            NV.assert_equal_outputs(nv[t][0], u8[t][0], t)
        r0 = nv[0][1]
        assert 'downscale_nv12' in r0 and r0.count('crop_and_resize_nv12') == 1 and not [r for r in r0 if r.startswith('preprocess')]
        NV.assert_tracked_rows(nv[1][1])
        NV.assert_tracked_rows(nv[2][1])
        assert not nv[1][0]['lost'].any() and not nv[2][0]['detected'].any()
    finally:
        e.close()
