"""A batch of separate surfaces, formats mixed on the CPU interpreter: the RGB stack, the crop / detection frame /
normalise kernels against the uint8 kernels on the stacked RGB frames, every refusal, the Python surface, and one whole tracked step
and one whole detect step at B = 2, 32 x 32, [bgra, nv12] against track_step_u8 on the stack -- everything bit for bit.  The
interpreter needs about a minute per image and whole step, so the whole steps are the fewest that reach the code;
tests/test_gpu_surf.py runs every option over three steps on the GPU."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import px_oracle as PX                 # noqa: E402
import surf_oracle as SF               # noqa: E402

F32 = np.float32


def test_helper_batches():
    """The oracle itself: separate allocations in descending order of addresses, poison wherever no sample lies, each allocation ends at
    its last used byte, a repeated record shares its surface, and the stack is the two existing NumPy forms'."""
    H, W = 16, 18
    b = SF.random_batch(3, SF.mixed3(W) + [1], H, W)
    SF.assert_poisoned(b, H, W)
    assert b.formats == ['bgra', 'bgr', 'nv12', 'bgr'] and b.addresses(3) == b.addresses(1) and b.surfaces[3] is b.surfaces[1]
    first = [b.allocs[i][0].ctypes.data for i in range(3)] + [b.allocs[2][1].ctypes.data]
    assert first == sorted(first, reverse=True) and len(set(first)) == 4
    assert b.addresses(0)[0] % 64 == 0 and b.addresses(1)[0] % 64 == 1 and b.pitch == [W * 4, W * 3 + 1, W + 10, W * 3 + 1]
    rgb = SF.to_rgb(b)
    pictures = np.random.default_rng(3).integers(0, 251, (4, H, W, 3)).astype(np.uint8)
    assert rgb.shape == (4, H, W, 3) and np.array_equal(rgb[:2], pictures[:2]) and np.array_equal(rgb[3], rgb[1])
    y, uv = b.surfaces[2]
    assert np.array_equal(rgb[2], SF.NV.to_rgb(np.ascontiguousarray(y)[None], np.ascontiguousarray(uv)[None], W, 'bt709')[0])
    assert SF.value('nv12') == 16 and SF.value('abgr') == 5


def test_product_numpy_form_agrees_with_the_helper():
    from hand3d_amd.utils import pixels as U
    assert U.SURF_NV12 == SF.NV12_VALUE
    b = SF.random_batch(5, SF.mixed3(18), 16, 18)
    for m in ('bt709', 'bt601_full'):
        assert np.array_equal(U.surfaces_to_rgb(b.surfaces, b.formats, nv12_matrix=m), SF.to_rgb(b, m))


def test_surf_to_rgb(emu_engine):
    SF.assert_to_rgb_cases(emu_engine)


def test_surf_to_rgb_follows_the_matrix_option(emu_engine):
    b = SF.random_batch(9, SF.mixed3(18), 16, 18)
    emu_engine.set_option('nv12_matrix', 'bt601')
    try:
        assert np.array_equal(emu_engine.surf_to_rgb(b.surfaces, b.formats), SF.to_rgb(b, 'bt601'))
    finally:
        emu_engine.set_option('nv12_matrix', 'bt709')


@pytest.mark.parametrize("H,W", PX.CROP_FRAMES)
def test_crop_bit_exact(emu_engine, H, W):
    SF.assert_crop_cases(emu_engine, H, W)


@pytest.mark.parametrize("f", SF.DOWNSCALE_FACTORS)
@pytest.mark.parametrize("name,specs,H,W", SF.DOWNSCALE_BATCHES, ids=[c[0] for c in SF.DOWNSCALE_BATCHES])
def test_downscale_bit_exact(emu_engine, name, specs, H, W, f):
    SF.assert_downscale_case(emu_engine, specs(W), H, W, f)


def test_downscale_batches_hold_a_wide_surface_beside_a_narrow_one():
    """The 'wide-and-not' batch by the rules of include/hp3d.h: surfaces 0, 2 and 4 lie on 16-byte grids (every wide load of f = 2, 4, 8
    is allowed), their neighbours 1, 3 and 5 are off every grid; windows are ragged at f = 4 and 8."""
    name, specs, H, W = SF.DOWNSCALE_BATCHES[2]
    b = SF.random_batch(3 + H + W, specs(W), H, W)
    for i in (0, 2, 4):
        assert all(a % 16 == 0 for a in b.addresses(i)) and b.pitch[i] % 16 == 0
    assert b.addresses(1)[0] % 2 == 1 and b.pitch[3] % 2 == 1 and b.pitch[5] % 2 == 1
    assert H % 4 and H % 8 and W % 8 == 0 and SF.DOWNSCALE_BATCHES[0][3] % 4


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(emu_engine, synth_weights):
    """Every refusal: HP3D_ERR_ARG with a message that names the offending surface index, from every entry point, with counters, the
    profile and the trackers' state untouched -- the step behind a refusal is the kind it would have been."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        lib, h, p = e.lib, e.h, _lib._ptr
        B, H, W = 2, 32, 32
        hs1, hs2 = synth.hand_sides(B), HO.hand_sides(B, 1)
        out = np.zeros((B, H, W, 3), F32)
        bc, bs = np.tile(np.array([16.0, 16.0], F32), (B, 1)), np.ones(B, F32)
        batch = SF.synth_batch(4, 0, [('bgra', dict(pitch=W * 4 + 8)), ('nv12', dict(pitch=W + 6))], H, W)
        good = SF.records(batch, H, W)
        # a tracked state for both trackers: the next step of either is a tracked step
        e.track_seed(np.tile(np.array([H / 2.0, W / 2.0], F32), (B, 1)), np.full(B, 10.0, F32), H, W)
        e.track_hands_seed(np.tile(np.array([H / 2.0, W / 2.0], F32), (B, 1, 1)), np.full((B, 1), 10.0, F32), np.ones((B, 1), np.int32), H, W)
        names = ('track_detect_steps', 'track_tracked_steps', 'track_hands_detect_steps', 'track_hands_tracked_steps', 'crop_surf_launches',
                 'crop_px_launches', 'crop_nv12_launches', 'crop_u8_launches', 'detect_scale_steps')
        e.set_profiling(1)
        rows0, c0 = e.profile(), [e.counter(k) for k in names]
        nul10, nul13 = [None] * 10, [None] * 13

        def calls(B, H, W, recs):
            arr = None if recs is None else _lib.Engine.surface_records(recs)
            sf = None if recs is None else _lib.C.addressof(arr)
            return [lib.hp3d_track_step_surf(h, B, H, W, sf, p(hs1), *nul10),
                    lib.hp3d_track_step_surf_dev(h, B, H, W, sf, p(hs1), *nul10),
                    lib.hp3d_track_hands_step_surf(h, B, H, W, sf, 1, p(hs2), *nul13),
                    lib.hp3d_track_hands_step_surf_dev(h, B, H, W, sf, 1, p(hs2), *nul13),
                    lib.hp3d_surf_to_rgb(h, sf, B, H, W, p(out)),
                    lib.hp3d_crop_and_resize_surf(h, sf, B, H, W, 1, p(bc), p(bs), None, 0, 8, p(out)),
                    lib.hp3d_downscale_surf(h, sf, B, H, W, 2, None, 0, p(out))]

        def change(i, **kw):
            keys = ('data', 'chroma', 'pitch', 'format', 'height', 'width')
            r = dict(zip(keys, good[i]), **kw)
            return [tuple(r[k] for k in keys) if j == i else g for j, g in enumerate(good)]

        cases = [((B, H, W, None), 'surfaces is NULL'),
                 ((B, H, W, change(0, data=0)), 'surfaces[0].data is NULL'),
                 ((B, H, W, change(1, data=0)), 'surfaces[1].data is NULL'),
                 ((B, H, W, change(1, chroma=0)), 'surfaces[1].chroma is NULL'),
                 ((B, H, W, change(0, chroma=good[1][1])), 'surfaces[0].chroma must be NULL'),
                 ((B, H, W, change(0, format=6)), 'surfaces[0].format=6'),
                 ((B, H, W, change(1, format=-1, chroma=0)), 'surfaces[1].format=-1'),
                 ((B, H, W, change(1, format=15)), 'surfaces[1].format=15'),
                 ((B, H, W, change(0, pitch=W * 4 - 1)), 'surfaces[0].pitch=%d' % (W * 4 - 1)),
                 ((B, H, W, change(1, pitch=W - 1)), 'surfaces[1].pitch=%d' % (W - 1)),
                 ((B, H, W, change(0, height=H + 2)), 'surfaces[0] is %dx%d' % (H + 2, W)),
                 ((B, H, W, change(1, width=W - 2)), 'surfaces[1] is %dx%d' % (H, W - 2)),
                 ((0, H, W, good), 'B=0'), ((B, 14, W, [g[:4] + (14, W) for g in good]), 'H=14'),
                 ((B, H, 14, [g[:4] + (H, 14) for g in good]), 'W=14')]
        # an NV12 surface with odd H or W (the packed neighbour is fine with both)
        cases += [((B, 31, W, [g[:4] + (31, W) for g in good]), 'surfaces[1] is NV12'), ((B, H, 31, [g[:4] + (H, 31) for g in good]), 'surfaces[1] is NV12')]
        for args, word in cases:
            for rc in calls(*args):
                assert rc == -1, (word, rc)
                assert word in lib.hp3d_last_error(h).decode(), (word, lib.hp3d_last_error(h))
            if 'is %d' % (H + 2) in word or 'is %dx%d' % (H, W - 2) in word:
                assert 'mixed sizes are not supported yet' in lib.hp3d_last_error(h).decode()
        assert [e.counter(k) for k in names] == c0 and e.profile() == rows0
        # the state was left as it was: the next step is the tracked step it would have been (the multi-hand tracker shares the code
        # in front of the refusal, and its counters did not move either)
        e.set_profiling(0)
        e.track_step_surf(batch.surfaces, batch.formats, hs1)
        got = [e.counter(k) - c for k, c in zip(names, c0)]
        assert got[:5] == [0, 1, 0, 0, 1], got
    finally:
        e.close()


# ---- whole steps --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


H = W = 32
STEP_SPECS = [('bgra', dict()), ('nv12', dict(pitch=W + 6))]


def test_steps_equal_the_uint8_steps(net_engine):
    """B = 2, [bgra, nv12]: one whole detect step and one whole tracked step (on a frame this small random weights lose every hand, so
    it is seeded at the frame's centre with scale 10 as tests/test_track.py does) -- every output and flag of track_step_surf equals
    track_step_u8 on the stack; the tracked step's one frame-reading launch is the surface crop."""
    e = net_engine
    B = 2
    hs = synth.hand_sides(B)
    batches = [SF.synth_batch(4, t, STEP_SPECS, H, W) for t in range(2)]
    names = ('crop_surf_launches', 'crop_u8_launches', 'track_detect_steps', 'track_tracked_steps')

    def sequence(step):
        c0 = [e.counter(k) for k in names]
        e.track_reset()
        out = [SF.profile_rows(e, lambda: step(0))]
        e.track_seed(np.tile(np.array([H / 2.0, W / 2.0], F32), (B, 1)), np.full(B, 10.0, F32), H, W)
        out.append(SF.profile_rows(e, lambda: step(1)))
        e.track_reset()
        return out, [e.counter(k) - c for k, c in zip(names, c0)]

    sf, dsf = sequence(lambda t: e.track_step_surf(batches[t].surfaces, batches[t].formats, hs, want_kpmap=True))
    u8, du8 = sequence(lambda t: e.track_step_u8(SF.to_rgb(batches[t]), hs, want_kpmap=True))
    for t in range(2):
        SF.assert_equal_outputs(sf[t][0], u8[t][0], t)
        assert SF.u8_rows(sf[t][1]) == u8[t][1], t
    (o0, r0), (o1, r1) = sf
    assert np.all(o0['detected'] == 1) and not o1['detected'].any() and o1['crop'][0].any() and o1['crop'][1].any()
    assert 'preprocess_surf' in r0 and 'crop_and_resize' in r0 and not [r for r in r0 if '_u8' in r]
    SF.assert_tracked_rows(r1)
    # every counter the uint8 step moves, with the surface crop counter where the uint8 one stands
    assert dsf == [1, 0, 1, 1] and du8 == [0, 1, 1, 1]


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
class _Calls:
    """A library that records the surface steps it is handed and answers success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            from hand3d_amd import _lib
            n = a[1]
            arr = (_lib.Surface * n).from_address(a[4])
            self.calls.append((name, a[1:4], [(r.data, r.chroma, r.pitch, r.format, r.height, r.width) for r in arr]))
            return 0
        return call


def test_python_list_forms_reach_the_library_in_place():
    """track() / track_hands() with a list of surfaces: one record per surface with the array's own address and pitch (a region of
    interest of a wider surface goes in place), one name for all or one per surface."""
    from hand3d_amd import _lib
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    e = _lib.Engine.__new__(_lib.Engine)
    e.lib, e.h = _Calls(), None
    net.engine = e
    wide = np.zeros((40, 50, 4), np.uint8)
    roi = wide[4:36, 6:38]
    bgr = np.zeros((32, 32, 3), np.uint8)
    y, uv = np.zeros((32, 40), np.uint8)[:, :32], np.zeros((16, 40), np.uint8)[:, :32]
    net.track([roi, bgr, (y, uv)], synth.hand_sides(3), pixel_format=['bgra', 'bgr', 'nv12'])
    net.track_hands([roi, roi], HO.hand_sides(2, 2), 2, pixel_format='bgra')
    (n0, shape0, r0), (n1, shape1, r1) = e.lib.calls
    assert (n0, shape0) == ('hp3d_track_step_surf', (3, 32, 32)) and (n1, shape1) == ('hp3d_track_hands_step_surf', (2, 32, 32))
    assert r0 == [(roi.ctypes.data, None, 200, 3, 32, 32), (bgr.ctypes.data, None, 96, 1, 32, 32), (y.ctypes.data, uv.ctypes.data, 40, 16, 32, 32)]
    assert r1 == [(roi.ctypes.data, None, 200, 3, 32, 32)] * 2
    assert roi.ctypes.data == wide.ctypes.data + 4 * 200 + 24


def test_python_list_form_errors():
    from hand3d_amd import _lib
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = _lib.Engine.__new__(_lib.Engine)          # the frames are checked before the library is called
    hs1, hs2 = synth.hand_sides(2), HO.hand_sides(2, 2)
    bgra, bgr = np.zeros((16, 16, 4), np.uint8), np.zeros((16, 16, 3), np.uint8)
    y, uv = np.zeros((16, 16), np.uint8), np.zeros((8, 16), np.uint8)
    for call in (lambda **kw: net.track(kw.pop('image'), hs1, **kw), lambda **kw: net.track_hands(kw.pop('image'), hs2, 2, **kw)):
        with pytest.raises(ValueError, match="names 3 formats, image holds 2"):
            call(image=[bgra, bgr], pixel_format=['bgra', 'bgr', 'bgr'])          # wrong lengths
        with pytest.raises(ValueError, match="names 1 formats, image holds 2"):
            call(image=[bgra, bgr], pixel_format=['bgra'])
        with pytest.raises(ValueError, match="surface 1: pixel_format='bgr' names a packed frame.*NV12"):
            call(image=[bgra, (y, uv)], pixel_format=['bgra', 'bgr'])             # a pair under a packed name
        with pytest.raises(ValueError, match="NV12"):
            call(image=[(y, uv), (y, uv)], pixel_format='bgra')
        with pytest.raises(ValueError, match="surface 0: pixel_format='nv12' wants a pair"):
            call(image=[bgra, bgr], pixel_format='nv12')
        with pytest.raises(ValueError, match="must then be a list"):
            call(image=np.zeros((2, 16, 16, 3), np.uint8), pixel_format=['bgr', 'bgr'])
        with pytest.raises(ValueError, match=r"surface 1: format 'bgra' wants a uint8 frame \[H,W,4\]"):
            call(image=[bgra, bgr], pixel_format='bgra')                          # the last axis does not match the format
        with pytest.raises(ValueError, match="surface 0: format must be"):
            call(image=[bgra, bgr], pixel_format=['yuyv', 'bgr'])


def test_python_list_forms_equal_the_stacked_uint8_calls(net_engine):
    """The list forms of track() (a list of one BGRA surface) and track_hands() (a list of one NV12 surface) equal the calls on the
    stacked uint8 frames (tracked steps: both trackers are seeded, so no HandSegNet pass runs on the interpreter; a mixed batch through
    the engine is test_steps_equal_the_uint8_steps, a mixed list through the binding test_python_list_forms_reach_the_library_in_place)."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    from hand3d_amd.utils.pixels import surfaces_to_rgb
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = e = net_engine
    batch = SF.synth_batch(4, 1, STEP_SPECS, H, W)
    rgb = surfaces_to_rgb(batch.surfaces, batch.formats)
    assert np.array_equal(rgb, SF.to_rgb(batch))
    c1, s1 = np.array([[H / 2.0, W / 2.0]], F32), np.full(1, 10.0, F32)
    c2, s2, v2 = np.array([[[H / 2.0, W / 2.0]]], F32), np.full((1, 1), 10.0, F32), np.ones((1, 1), np.int32)
    try:
        for n, seed, call, forms in (
                (8, lambda: e.track_seed(c1, s1, H, W), lambda image, **kw: net.track(image, synth.hand_sides(1), **kw),
                 ((batch.surfaces[:1], {'pixel_format': ['bgra']}), (rgb[:1], {}))),
                (10, lambda: e.track_hands_seed(c2, s2, v2, H, W), lambda image, **kw: net.track_hands(image, HO.hand_sides(1, 1), 1, **kw),
                 ((batch.surfaces[1:], {'pixel_format': 'nv12'}), (rgb[1:], {})))):
            got = []
            for image, kw in forms:
                seed()
                got.append(call(image, **kw))
            assert len(got[0]) == len(got[1]) == n
            for i in range(n):
                assert np.array_equal(got[0][i], got[1][i], equal_nan=True), (n, i)
            assert not got[0][7].any()          # detected: both were tracked steps
    finally:
        net.track_reset()
        net.track_hands_reset()
