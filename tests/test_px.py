"""Packed 8-bit frames on the CPU interpreter: the repack, the crop / detection frame / normalise kernels against the
uint8 kernels on the repacked frame, the refusals, the Python surface, and whole tracker steps on a 32 x 32 frame against the uint8
steps on the repacked frames -- everything bit for bit.  The interpreter needs about a minute per image and step, so the whole steps
are kept to the fewest that reach the code; tests/test_gpu_px.py runs every option over three steps on the GPU."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import px_oracle as PX                 # noqa: E402
import track_partial_oracle as TP      # noqa: E402

F32 = np.float32


def test_helper_surfaces():
    """The oracle itself: poison wherever no sample lies, the allocation ends at the last used byte, one picture per seed."""
    for fmt in PX.FORMATS:
        pb = PX.pixel_bytes(fmt)
        s, buf = PX.random_surface(3, 2, 16, 18, fmt, pitch=18 * pb + 5, lead=1, gap_rows=1, tail_rows=1)
        assert buf.ctypes.data % 64 == 0 and s.ctypes.data == buf.ctypes.data + 1 and PX.layout(s) == (18 * pb + 5, (18 * pb + 5) * 18)
        assert s[1, 15, 17].ctypes.data + pb == buf.ctypes.data + buf.size
        used = np.zeros(buf.size, bool)
        for b in range(2):
            for r in range(16):
                o = s[b, r].ctypes.data - buf.ctypes.data
                used[o:o + 18 * pb] = True
        assert np.all(buf[~used] == PX.POISON) and buf[used].reshape(-1, pb)[:, list(PX.TABLE[fmt][1])].max() <= 250
        t, _ = PX.random_surface(3, 2, 16, 18, 'rgb')
        assert np.array_equal(PX.to_rgb(s, fmt), t)
    s, _ = PX.random_surface(1, 1, 16, 16, 'argb')
    assert tuple(PX.to_rgb(s, 'argb')[0, 3, 4]) == tuple(s[0, 3, 4, 1:4]) and tuple(PX.to_rgb(s, 'argb')[0, 3, 4]) == tuple(s[0, 3, 4, 3:0:-1][::-1])
    assert tuple(PX.to_rgb(s.copy(), 'abgr')[0, 3, 4]) == tuple(s[0, 3, 4, 3:0:-1])


def test_product_numpy_forms_agree_with_the_helper():
    from hand3d_amd.utils import pixels as U
    assert {k: (v[1], v[2]) for k, v in U.FORMATS.items()} == PX.TABLE and {k: v[0] for k, v in U.FORMATS.items()} == PX.VALUE
    rgb = np.random.default_rng(0).integers(0, 256, (2, 16, 18, 3), dtype=np.uint8)
    for fmt in PX.FORMATS:
        pb = PX.pixel_bytes(fmt)
        s, _ = PX.random_surface(5, 2, 16, 18, fmt, pitch=18 * pb + 3)
        assert np.array_equal(U.to_rgb(s, fmt), PX.to_rgb(s, fmt))
        for pitch in (None, 18 * pb + 7):
            v = U.from_rgb(rgb, fmt, pitch=pitch, fill=9)
            assert v.shape == (2, 16, 18, pb) and v.strides[1] == (pitch or 18 * pb) and np.array_equal(PX.to_rgb(v, fmt), rgb)
            if pb == 4:
                assert np.all(v[..., 6 - sum(PX.TABLE[fmt][1])] == 9)


@pytest.mark.parametrize("fmt", PX.FORMATS)
def test_px_to_rgb(emu_engine, fmt):
    pb = PX.pixel_bytes(fmt)
    for kw in (dict(), dict(pitch=18 * pb + 1, lead=1, gap_rows=1), dict(pitch=128, tail_rows=1)):
        s, _ = PX.random_surface(7, 2, 16, 18, fmt, **kw)
        assert np.array_equal(emu_engine.px_to_rgb(s, fmt), PX.to_rgb(s, fmt)), (fmt, kw)


@pytest.mark.parametrize("fmt", PX.FORMATS)
@pytest.mark.parametrize("H,W", PX.CROP_FRAMES)
def test_crop_bit_exact(emu_engine, H, W, fmt):
    PX.assert_crop_cases(emu_engine, H, W, fmt)


@pytest.mark.parametrize("B,H,W,f,fmt,kind", PX.DOWNSCALE_CASES)
def test_downscale_bit_exact(emu_engine, B, H, W, f, fmt, kind):
    PX.assert_downscale_case(emu_engine, B, H, W, f, fmt, kind)


def test_downscale_cases_cover_the_formats():
    assert {c[4] for c in PX.DOWNSCALE_CASES} == set(PX.FORMATS)
    wide = {PX.pixel_bytes(c[4]) for c in PX.DOWNSCALE_CASES if c[3] in (2, 4, 8) and c[1] % c[3] == 0 and c[2] % c[3] == 0
            and PX.case_pitch(c[2], c[4], c[5]) % 16 == 0}
    assert wide == {3, 4}


def test_refusals_come_before_any_launch(emu_engine, synth_weights):
    """An unknown format, px NULL, pitch < W pixel_bytes, a short frame stride at B > 1, H or W below 16: HP3D_ERR_ARG with a message that
    names the argument, counters and profile untouched."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        lib, h, p = e.lib, e.h, _lib._ptr
        H, W = 32, 32
        hs1, hs2 = synth.hand_sides(2), HO.hand_sides(2, 2)
        crop, bc, bs = np.zeros((2, H, W, 3), F32), np.tile(np.array([16.0, 16.0], F32), (2, 1)), np.ones(2, F32)
        names = ('track_detect_steps', 'track_tracked_steps', 'track_hands_detect_steps', 'track_hands_tracked_steps', 'crop_px_launches',
                 'crop_nv12_launches', 'crop_u8_launches', 'detect_scale_steps')
        e.set_profiling(1)
        rows0, c0 = e.profile(), [e.counter(k) for k in names]
        nul10, nul13 = [None] * 10, [None] * 13

        def calls(B, H, W, px, pitch, fs, fmt):
            return [lib.hp3d_track_step_px(h, B, H, W, px, pitch, fs, fmt, p(hs1), *nul10),
                    lib.hp3d_track_step_px_dev(h, B, H, W, px, pitch, fs, fmt, p(hs1), *nul10),
                    lib.hp3d_track_hands_step_px(h, B, H, W, px, pitch, fs, fmt, 2, p(hs2), *nul13),
                    lib.hp3d_track_hands_step_px_dev(h, B, H, W, px, pitch, fs, fmt, 2, p(hs2), *nul13),
                    lib.hp3d_px_to_rgb(h, px, B, H, W, pitch, fs, fmt, p(crop)),
                    lib.hp3d_crop_and_resize_px(h, px, B, H, W, pitch, fs, fmt, 1, p(bc), p(bs), None, 0, 8, p(crop)),
                    lib.hp3d_downscale_px(h, px, B, H, W, pitch, fs, fmt, 2, None, 0, p(crop))]

        for fmt in ('bgr', 'bgra'):
            pb, v = PX.pixel_bytes(fmt), PX.VALUE[fmt]
            s, _ = PX.random_surface(3, 2, H, W, fmt, pitch=W * pb + 8)
            pitch, fs = PX.layout(s)
            for args, word in (((2, H, W, p(s), pitch, fs, 6), 'format=6'), ((2, H, W, p(s), pitch, fs, -1), 'format=-1'),
                               ((2, H, W, None, pitch, fs, v), 'px (the surface) is NULL'),
                               ((2, H, W, p(s), W * pb - 1, fs, v), 'pitch=%d' % (W * pb - 1)),
                               ((2, H, W, p(s), pitch, pitch * (H - 1) + W * pb - 1, v), 'frame_stride='),
                               ((2, 15, W, p(s), pitch, fs, v), 'H=15'), ((2, H, 15, p(s), pitch, fs, v), 'W=15')):
                for rc in calls(*args):
                    assert rc == -1, (word, rc)
                    assert word in e.lib.hp3d_last_error(h).decode(), (word, e.lib.hp3d_last_error(h))
            assert [e.counter(k) for k in names] == c0 and e.profile() == rows0
            # the short stride is no error at B = 1, where the stride is not used
            assert lib.hp3d_px_to_rgb(h, p(s), 1, H, W, pitch, 0, v, p(np.zeros((1, H, W, 3), np.uint8))) == 0
    finally:
        e.close()


# ---- whole steps --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


H = W = 32


def test_steps_equal_the_uint8_steps(net_engine):
    """BGRA, aligned: a detect step and a tracked step (on a frame this small random weights lose every hand, so it is seeded at the
    frame's centre with scale 10 as tests/test_track.py does) -- every output and flag of track_step_px equals track_step_u8 on the
    repacked frames; the tracked step's one frame-reading launch is the packed crop."""
    e = net_engine
    hs = synth.hand_sides(1)
    surf = [PX.synth_surface(4, t, 1, H, W, 'bgra')[0] for t in range(2)]
    names = ('crop_px_launches', 'crop_u8_launches', 'track_detect_steps', 'track_tracked_steps')

    def sequence(step):
        c0 = [e.counter(k) for k in names]
        e.track_reset()
        out = [PX.profile_rows(e, lambda: step(0))]
        e.track_seed(np.array([[H / 2.0, W / 2.0]], F32), np.array([10.0], F32), H, W)
        out.append(PX.profile_rows(e, lambda: step(1)))
        e.track_reset()
        return out, [e.counter(k) - c for k, c in zip(names, c0)]

    px, dpx = sequence(lambda t: e.track_step_px(surf[t], 'bgra', hs, want_kpmap=True))
    u8, du8 = sequence(lambda t: e.track_step_u8(PX.to_rgb(surf[t], 'bgra'), hs, want_kpmap=True))
    for t in range(2):
        PX.assert_equal_outputs(px[t][0], u8[t][0], t)
        assert [r.replace('_px', '_u8') for r in px[t][1]] == u8[t][1], t
    (o0, r0), (o1, r1) = px
    assert o0['detected'][0] == 1 and o1['detected'][0] == 0 and o1['crop'].any()
    assert 'preprocess_px' in r0 and 'crop_and_resize' in r0 and not [r for r in r0 if r.startswith('preprocess_u8')]
    PX.assert_tracked_rows(r1)
    # every counter the uint8 step moves, with the packed crop counter where the uint8 one stands
    assert dpx == [1, 0, 1, 1] and du8 == [0, 1, 1, 1]


def test_detect_step_with_detect_scale(net_engine):
    """BGR at an odd pitch, detect_scale = 2: one detect step from the surface (run_detect_reduced's packed branch)."""
    e = net_engine
    hs = synth.hand_sides(1)
    s, _ = PX.synth_surface(4, 0, 1, H, W, 'bgr', pitch=W * 3 + 1)
    e.set_option('detect_scale', '2')
    try:
        n0, c0 = e.counter('detect_scale_steps'), e.counter('crop_px_launches')
        e.track_reset()
        a, rows = PX.profile_rows(e, lambda: e.track_step_px(s, 'bgr', hs, want_kpmap=True))
        e.track_reset()
        b, rows8 = PX.profile_rows(e, lambda: e.track_step_u8(PX.to_rgb(s, 'bgr'), hs, want_kpmap=True))
        PX.assert_equal_outputs(a, b)
        assert a['detected'][0] == 1
        assert rows.count('downscale_px') == 1 and rows.count('crop_and_resize_px') == 1 and not [r for r in rows if r.startswith('preprocess')]
        assert [r.replace('_px', '_u8') for r in rows] == rows8
        assert e.counter('detect_scale_steps') == n0 + 2 and e.counter('crop_px_launches') == c0 + 1
    finally:
        e.set_option('detect_scale', '1')
        e.track_reset()


def test_partial_detect_step(net_engine):
    """RGBA, B = 2, track_partial_detect = 1 at detect_scale = 2, as tests/test_nv12.py arranges it: seeded so that the tracked step loses
    frame 1 only, then the partial detect step, which builds the detection frame of the lost frame alone (downscale_px_idx) and crops both
    frames from the surface.  (The f = 1 form, preprocess_px_idx, is held to preprocess_u8 by test_downscale_bit_exact and runs inside a
    step in tests/test_gpu_px.py.)"""
    e = net_engine
    B = 2
    hs = synth.hand_sides(B)
    surf = [PX.synth_surface(21, t, B, H, W, 'rgba', pitch=W * 4 + 4, tail_rows=1)[0] for t in range(2)]
    e.set_option('track_partial_detect', '1')
    e.set_option('detect_scale', '2')
    try:
        res = []
        for px in (True, False):
            c, s = TP.seed_boxes(B, H, W, [1])
            e.track_seed(c, s, H, W)
            outs = []
            for t in range(2):
                call = (lambda: e.track_step_px(surf[t], 'rgba', hs, want_kpmap=True)) if px else \
                       (lambda: e.track_step_u8(PX.to_rgb(surf[t], 'rgba'), hs, want_kpmap=True))
                outs.append(PX.profile_rows(e, call))
            res.append(outs)
        for t in range(2):
            PX.assert_equal_outputs(res[0][t][0], res[1][t][0], t)
            assert [r.replace('_px', '_u8') for r in res[0][t][1]] == res[1][t][1], t
        assert res[0][0][0]['lost'].tolist() == [0, 1] and res[0][1][0]['detected'].tolist() == [0, 1]
        PX.assert_tracked_rows(res[0][0][1])
        rows = res[0][1][1]
        assert rows.count('downscale_px_idx') == 1 and rows.count('crop_and_resize_px') == 1
        assert not [r for r in rows if r.startswith('preprocess') or r == 'downscale_px' or '_u8' in r]
    finally:
        e.set_option('track_partial_detect', '0')
        e.set_option('detect_scale', '1')
        e.track_reset()


def test_hands_step_compacted(emu_engine, synth_weights):
    """ARGB, track_hands_step_px at K = 2 with hands_compact: slot 1 absent (tests/test_hands_compact.py's seed), one tracked step."""
    from hand3d_amd import _lib
    K = 2
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        e.set_option('hands_compact', '1')
        hs = HO.hand_sides(1, K)
        center = np.array([[[H / 2, W / 2], [7.0, 9.0]]], F32)
        scale, valid = np.array([[10.0, 3.0]], F32), np.array([[1, 0]], np.int32)
        s, _ = PX.synth_surface(2, 0, 1, H, W, 'argb', pitch=W * 4 + 2, lead=1)
        e.track_hands_seed(center, scale, valid, H, W)
        n0 = e.counter('crop_px_launches')
        a, rows = PX.profile_rows(e, lambda: e.track_hands_step_px(s, 'argb', hs, K, want_kpmap=True))
        e.track_hands_seed(center, scale, valid, H, W)
        b = e.track_hands_step_u8(PX.to_rgb(s, 'argb'), hs, K, want_kpmap=True)
        PX.assert_equal_outputs(a, b)
        assert a['valid'][0].tolist() == [1, 0]
        PX.assert_tracked_rows(rows, idx=True)
        assert e.counter('crop_px_launches') == n0 + 1
    finally:
        e.close()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def test_python_surface(net_engine):
    """track(..., pixel_format='bgr') equals track() on frame[..., ::-1]."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = net_engine
    rgb = PX.TO.to_u8(PX.TO.frames(4, 1, 1, H, W))
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    hs = synth.hand_sides(1)
    try:
        net.track_reset()
        a = net.track(bgr, hs, pixel_format='bgr')
        net.track_reset()
        b = net.track(bgr[..., ::-1], hs)
        assert len(a) == len(b) == 8
        for i, (p, q) in enumerate(zip(a, b)):
            assert np.array_equal(p, q, equal_nan=True), i
        assert not np.array_equal(rgb, bgr)
    finally:
        net.track_reset()


class _Recorder:
    """An engine that records what track() / track_hands() hand it."""

    def __init__(self):
        self.calls = []

    def set_option(self, k, v):
        self.calls.append(('set_option', k, v))

    def __getattr__(self, name):
        def step(*a):
            self.calls.append((name,) + a)
            z = np.zeros(1)
            return dict.fromkeys(('coord3d', 'kp_hw', 'kp_crop', 'scale', 'center', 'confidence', 'lost', 'detected', 'valid', 'area'), z)
        return step


def test_python_surface_routing_and_errors():
    """pixel_format=None: exactly today's routing; a format: the packed step; the three ValueErrors."""
    from hand3d_amd import _lib
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = rec = _Recorder()
    hs1, hs2 = synth.hand_sides(1), HO.hand_sides(1, 2)
    rgb = np.zeros((1, 16, 16, 3), np.uint8)
    bgra = np.zeros((1, 16, 16, 4), np.uint8)
    net.track(rgb, hs1)
    net.track_hands(rgb, hs2, 2, pixel_format=None)
    net.track(bgra, hs1, pixel_format='bgra')
    net.track_hands(rgb, hs2, 2, pixel_format='bgr')
    assert [c[0] for c in rec.calls] == ['track_step_u8', 'track_hands_step_u8', 'track_step_px', 'track_hands_step_px']
    assert rec.calls[2][1] is bgra and rec.calls[2][2] == 'bgra' and rec.calls[3][1] is rgb and rec.calls[3][2] == 'bgr' and rec.calls[3][4] == 2
    # the real binding checks the frames before the library is called: a library-less engine is enough
    e = _lib.Engine.__new__(_lib.Engine)
    net.engine = e
    y, uv = np.zeros((1, 16, 16), np.uint8), np.zeros((1, 8, 16), np.uint8)
    for call in (lambda **kw: net.track(kw.pop('image'), hs1, **kw), lambda **kw: net.track_hands(kw.pop('image'), hs2, 2, **kw)):
        with pytest.raises(ValueError, match=r"\[B,H,W,4\]"):
            call(image=rgb, pixel_format='bgra')                       # the last axis does not match the format
        with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
            call(image=bgra, pixel_format='rgb')
        with pytest.raises(ValueError, match="uint8"):
            call(image=rgb.astype(F32), pixel_format='rgb')            # not uint8
        with pytest.raises(ValueError, match="NV12"):
            call(image=(y, uv), pixel_format='bgr')                    # an (y, uv) pair
        with pytest.raises(ValueError, match="NV12"):
            call(image=[y, uv], pixel_format='bgr')
        with pytest.raises(ValueError, match="pixel_format"):
            call(image=rgb, pixel_format='yuyv')


def test_roi_view_goes_in_place():
    """A region of interest of a wider BGRA surface is passed as it lies: the address handed to the library is the view's own, with
    the surface's pitch and stride; a view the layout cannot describe is copied once."""
    from hand3d_amd import _lib

    class Lib:
        def __init__(self):
            self.args = None

        def hp3d_track_step_px(self, *a):
            self.args = a
            return 0

    e = _lib.Engine.__new__(_lib.Engine)
    e.lib, e.h = Lib(), None
    surface = np.random.default_rng(0).integers(0, 256, (2, 64, 96, 4), dtype=np.uint8)
    roi = surface[:, 10:42, 20:68]
    assert not roi.flags['C_CONTIGUOUS']
    e.track_step_px(roi, 'bgra', synth.hand_sides(2))
    h, B, Hh, Ww, px, pitch, fs, fmt = e.lib.args[:8]
    assert (B, Hh, Ww, pitch, fs, fmt) == (2, 32, 48, 96 * 4, 64 * 96 * 4, PX.VALUE['bgra'])
    assert px.value == roi.ctypes.data == surface.ctypes.data + 10 * 96 * 4 + 20 * 4
    # B = 1: the stride is not used, and a single picture of a batch goes in place too
    e.track_step_px(roi[1:], 'bgra', synth.hand_sides(1))
    assert e.lib.args[4].value == roi[1:].ctypes.data and e.lib.args[6] == 0
    # every second column: no pitch describes it -> one contiguous copy
    e.track_step_px(surface[:, :32, ::2], 'bgra', synth.hand_sides(2))
    assert e.lib.args[5] == 48 * 4 and e.lib.args[6] == 32 * 48 * 4
    lo, hi = surface.ctypes.data, surface.ctypes.data + surface.nbytes
    assert not lo <= e.lib.args[4].value < hi
    # flipped rows (a negative row stride) likewise
    e.track_step_px(surface[:, ::-1], 'bgra', synth.hand_sides(2))
    assert not lo <= e.lib.args[4].value < hi and e.lib.args[5] == 96 * 4
