"""NV12 frames on the CPU interpreter: the colour rule on a lattice of (Y, U, V), the crop / detection frame /
normalise kernels against the uint8 kernels on the converted frame, the refusals, the Python surface, and whole tracker steps at
B = 1 on a 32 x 32 frame against hp3d_track_step_u8 on the converted frames -- everything bit for bit.  The interpreter needs about a
minute per image and step, so the steps with options are kept to the fewest that reach the code: one detect step at detect_scale = 2,
one lost frame and its partial detect step, one compacted multi-hand tracked step; tests/test_gpu_nv12.py runs every option over
three steps on the GPU."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO              # noqa: E402
import nv12_oracle as NV               # noqa: E402
import track_partial_oracle as TP      # noqa: E402

F32 = np.float32


def test_helper_on_hand_worked_triples():
    for matrix, yuv, rgb in NV.TRIPLES:
        assert tuple(NV.convert(*yuv, matrix)) == rgb, (matrix, yuv)
    # bt601 (81, 90, 240): blue is -110 before the shift, which floors to -1 and clamps to 0
    ky, yoff, rows = NV.TABLE['bt601']
    assert ky * (81 - yoff) + rows[2][0] * (90 - 128) + 128 == -110 and -110 // 256 == -1
    v = np.arange(256)
    for matrix in ('bt709_full', 'bt601_full'):
        assert np.array_equal(NV.convert(v, np.full(256, 128), np.full(256, 128), matrix), np.stack([v, v, v], -1))
    # the planes -> frame form: chroma replicated over its 2 x 2 block
    y, uv = NV.random_planes(1, 1, 16, 16, 18)
    rgb = NV.to_rgb(y, uv, 16, 'bt709')
    assert tuple(rgb[0, 5, 7]) == tuple(NV.convert(y[0, 5, 7], uv[0, 2, 6], uv[0, 2, 7], 'bt709'))
    assert tuple(rgb[0, 4, 6]) == tuple(NV.convert(y[0, 4, 6], uv[0, 2, 6], uv[0, 2, 7], 'bt709'))


def test_product_numpy_form_agrees_with_the_helper():
    from hand3d_amd.utils import nv12 as U
    y, uv, W = NV.lattice_planes()
    for matrix in NV.MATRICES:
        assert np.array_equal(U.nv12_to_rgb(y, uv, W, matrix), NV.to_rgb(y, uv, W, matrix)), matrix
    rgb = np.random.default_rng(0).integers(0, 256, (2, 16, 18, 3), dtype=np.uint8)
    yy, cc = U.rgb_to_nv12(rgb, 'bt601', pitch=20)
    assert yy.shape == (2, 16, 20) and cc.shape == (2, 8, 20) and not yy[:, :, 18:].any() and not cc[:, :, 18:].any()
    flat = np.repeat(np.repeat(rgb[:, ::2, ::2], 2, 1), 2, 2)          # constant 2 x 2 blocks: the round trip is within rounding
    for matrix in NV.MATRICES:
        back = U.nv12_to_rgb(*U.rgb_to_nv12(flat, matrix), matrix=matrix)
        assert np.abs(back.astype(int) - flat).max() <= 2, matrix


@pytest.mark.parametrize("matrix", NV.MATRICES)
def test_nv12_to_rgb_lattice(emu_engine, matrix):
    y, uv, W = NV.lattice_planes()
    vals = NV.lattice_values()
    assert {0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255} <= set(vals) and set(range(0, 256, 17)) <= set(vals)
    # the planes do hold every triple of the lattice
    seen = set(zip(y[0, :, :W].reshape(-1).tolist(), np.repeat(np.repeat(uv[0, :, 0:W:2], 2, 0), 2, 1).reshape(-1).tolist(),
                   np.repeat(np.repeat(uv[0, :, 1:W:2], 2, 0), 2, 1).reshape(-1).tolist()))
    assert len({(a, b, c) for a in vals for b in vals for c in vals} - seen) == 0
    emu_engine.set_option('nv12_matrix', matrix)
    try:
        assert np.array_equal(emu_engine.nv12_to_rgb(y, uv, W), NV.to_rgb(y, uv, W, matrix))
    finally:
        emu_engine.set_option('nv12_matrix', 'bt709')


@pytest.mark.parametrize("H,W", NV.CROP_FRAMES)
def test_crop_bit_exact(emu_engine, H, W):
    for i, pitch in enumerate(NV.crop_pitches(W)):
        NV.assert_crop_cases(emu_engine, H, W, pitch, NV.MATRICES[i % 4])


@pytest.mark.parametrize("B,H,W,f,pitch", NV.DOWNSCALE_CASES)
def test_downscale_bit_exact(emu_engine, B, H, W, f, pitch):
    NV.assert_downscale_case(emu_engine, B, H, W, f, pitch, NV.MATRICES[(f + pitch) % 4])


def test_refusals_come_before_any_launch(emu_engine, synth_weights):
    """Odd H or W, pitch < W, a NULL plane, a short frame stride, an unknown matrix: HP3D_ERR_ARG with a message that names the argument,
    counters and profile untouched."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        lib, h, p = e.lib, e.h, _lib._ptr
        H, W, pitch = 32, 32, 40
        y, uv = NV.random_planes(3, 2, H, W, pitch)
        fs = y.strides[0]
        hs1, hs2 = synth.hand_sides(2), HO.hand_sides(2, 2)
        crop, bc, bs = np.zeros((2, 8, 8, 3), F32), np.tile(np.array([16.0, 16.0], F32), (2, 1)), np.ones(2, F32)
        names = ('track_detect_steps', 'track_tracked_steps', 'track_hands_detect_steps', 'track_hands_tracked_steps', 'crop_nv12_launches',
                 'crop_u8_launches', 'detect_scale_steps')
        e.set_profiling(1)
        rows0, c0 = e.profile(), [e.counter(k) for k in names]
        nul10, nul13 = [None] * 10, [None] * 13

        def calls(B, H, W, py, puv, pitch, fs):
            return [lib.hp3d_track_step_nv12(h, B, H, W, py, puv, pitch, fs, p(hs1), *nul10),
                    lib.hp3d_track_step_nv12_dev(h, B, H, W, py, puv, pitch, fs, p(hs1), *nul10),
                    lib.hp3d_track_hands_step_nv12(h, B, H, W, py, puv, pitch, fs, 2, p(hs2), *nul13),
                    lib.hp3d_track_hands_step_nv12_dev(h, B, H, W, py, puv, pitch, fs, 2, p(hs2), *nul13),
                    lib.hp3d_nv12_to_rgb(h, py, puv, B, H, W, pitch, fs, p(crop)),
                    lib.hp3d_crop_and_resize_nv12(h, py, puv, B, H, W, pitch, fs, 1, p(bc), p(bs), None, 0, 8, p(crop)),
                    lib.hp3d_downscale_nv12(h, py, puv, B, H, W, pitch, fs, 2, None, 0, p(crop))]

        for args, word in (((2, 31, W, p(y), p(uv), pitch, fs), 'H=31'), ((2, H, 31, p(y), p(uv), pitch, fs), 'W=31'),
                           ((2, H, W, p(y), p(uv), 30, fs), 'pitch=30'), ((2, H, W, None, p(uv), pitch, fs), 'y (the luma plane) is NULL'),
                           ((2, H, W, p(y), None, pitch, fs), 'uv (the chroma plane) is NULL'), ((2, H, W, p(y), p(uv), pitch, pitch * (H - 1) + W - 1), 'frame_stride=')):
            for rc in calls(*args):
                assert rc == -1, (word, rc)
                assert word in e.lib.hp3d_last_error(h).decode(), (word, e.lib.hp3d_last_error(h))
        with pytest.raises(AssertionError, match="nv12_matrix"):
            e.set_option('nv12_matrix', 'bt2020')
        for ok in NV.MATRICES:
            e.set_option('nv12_matrix', ok)
        e.set_option('nv12_matrix', 'bt709')
        assert [e.counter(k) for k in names] == c0 and e.profile() == rows0
        # the short stride is no error at B = 1, where the stride is not used
        assert lib.hp3d_nv12_to_rgb(h, p(y), p(uv), 1, H, W, pitch, 0, p(np.zeros((1, H, W, 3), np.uint8))) == 0
    finally:
        e.close()


# ---- whole steps --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


FAR = (np.array([[-5000.0, -7000.0]], F32), np.array([1.0], F32))


def _sequence(e, H, W, step, frame):
    """reset -> a detect step; a tracked step (on a frame this small random weights lose every hand, so it is seeded at the frame's
    centre with scale 10 as tests/test_track.py does); a seeded tracked step whose box leaves the frame.  [(outputs, profile rows)]"""
    hs = synth.hand_sides(1)
    e.track_reset()
    out = [NV.profile_rows(e, lambda: step(frame(0), hs))]
    e.track_seed(np.array([[H / 2.0, W / 2.0]], F32), np.array([10.0], F32), H, W)
    out.append(NV.profile_rows(e, lambda: step(frame(1), hs)))
    e.track_seed(FAR[0], FAR[1], H, W)
    out.append(NV.profile_rows(e, lambda: step(frame(2), hs)))
    e.track_reset()
    return out


def _both_sequences(e, H, W, pitch, matrix='bt709'):
    planes = [NV.synth_planes(4, t, 1, H, W, pitch=pitch, gap_rows=1) for t in range(3)]
    e.set_option('nv12_matrix', matrix)
    try:
        nv = _sequence(e, H, W, lambda f, hs: e.track_step_nv12(f[0], f[1], hs, W=W, want_kpmap=True), lambda t: planes[t])
        u8 = _sequence(e, H, W, lambda f, hs: e.track_step_u8(f, hs, want_kpmap=True), lambda t: NV.to_rgb(planes[t][0], planes[t][1], W, matrix))
    finally:
        e.set_option('nv12_matrix', 'bt709')
    for t, ((a, _), (b, _)) in enumerate(zip(nv, u8)):
        NV.assert_equal_outputs(a, b, t)
    return nv, u8


def test_steps_equal_the_uint8_steps(net_engine):
    """B = 1, 32 x 32, pitch 40: detect, tracked, seeded tracked step whose box leaves the frame -- every output and flag of
    track_step_nv12 equals track_step_u8 on the converted frames; the tracked steps' one frame-reading launch is the NV12 crop."""
    e = net_engine
    n0 = e.counter('crop_nv12_launches')
    nv, u8 = _both_sequences(e, 32, 32, 40, 'bt601')
    (o0, r0), (o1, r1), (o2, r2) = nv
    assert o0['detected'][0] == 1 and o1['detected'][0] == 0 and o2['detected'][0] == 0 and o2['lost'][0] == 1 and not o2['crop'].any()
    assert 'preprocess_nv12' in r0 and 'crop_and_resize' in r0 and not [r for r in r0 if r.startswith('preprocess_u8')]
    NV.assert_tracked_rows(r1)
    NV.assert_tracked_rows(r2)
    assert e.counter('crop_nv12_launches') == n0 + 2
    assert 'crop_and_resize_u8' in u8[1][1] and 'preprocess_u8' in u8[0][1]


def test_python_surface(net_engine):
    """track(image=(y, uv)) equals track() on the converted uint8 frame; nv12_matrix= sets the option."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    from hand3d_amd.utils.nv12 import nv12_to_rgb
    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = net_engine
    H = W = 32
    y, uv = NV.synth_planes(4, 1, 1, H, W)
    hs = synth.hand_sides(1)
    try:
        net.track_reset()
        a = net.track((y, uv), hs, nv12_matrix='bt601_full')
        net.track_reset()
        b = net.track(nv12_to_rgb(y, uv, matrix='bt601_full'), hs)
        assert len(a) == len(b) == 8
        for i, (p, q) in enumerate(zip(a, b)):
            assert np.array_equal(p, q, equal_nan=True), i
        assert not np.array_equal(NV.to_rgb(y, uv, W, 'bt601_full'), NV.to_rgb(y, uv, W, 'bt709'))
    finally:
        net_engine.set_option('nv12_matrix', 'bt709')
        net.track_reset()


def test_python_surface_routing():
    """track() and track_hands(): a tuple or a list of the two planes goes to the NV12 step, a packed frame (an array or a nested list)
    where it always went, and a tuple that is no pair of planes is refused by name."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork

    class Recorder:
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

    net = ColorHandPose3DNetwork.__new__(ColorHandPose3DNetwork)
    net.engine = rec = Recorder()
    y, uv = NV.random_planes(0, 1, 16, 16, 20)
    hs1, hs2 = synth.hand_sides(1), HO.hand_sides(1, 2)
    for image in ((y, uv), [y, uv]):
        assert len(net.track(image, hs1)) == 8 and len(net.track_hands(image, hs2, 2, nv12_matrix='bt601')) == 10
    names = [c[0] for c in rec.calls]
    assert names == ['track_step_nv12', 'set_option', 'track_hands_step_nv12'] * 2 and rec.calls[1] == ('set_option', 'nv12_matrix', 'bt601')
    assert rec.calls[0][1] is y and rec.calls[0][2] is uv and rec.calls[2][1] is y and rec.calls[2][2] is uv and rec.calls[2][4] == 2
    del rec.calls[:]
    rgb = NV.to_rgb(y, uv, 16, 'bt709')
    f32 = rgb.astype(F32) / F32(255) - F32(0.5)
    for image in (rgb, f32, f32.tolist(), [rgb[0], rgb[0]]):          # (the last: a list of two uint8 pictures is a batch of two)
        net.track(image, hs1)
        net.track_hands(image, hs2, 2)
    assert [c[0] for c in rec.calls] == ['track_step_u8', 'track_hands_step_u8', 'track_step', 'track_hands_step', 'track_step', 'track_hands_step',
                                         'track_step_u8', 'track_hands_step_u8']
    for bad in ((y,), (y, uv, uv), (y, uv[:, :-1]), (y, uv.astype(F32)), (rgb, rgb)):
        with pytest.raises(ValueError, match="NV12 planes"):
            net.track(bad, hs1)
        with pytest.raises(ValueError, match="NV12 planes"):
            net.track_hands(bad, hs2, 2)


def test_detect_step_with_detect_scale(net_engine):
    """detect_scale = 2: one detect step from the planes (run_detect_reduced's NV12 branch) against the uint8 detect step.  The tracked
    steps behind it are the ones test_steps_equal_the_uint8_steps runs: the option changes nothing in them."""
    e = net_engine
    H, W = 32, 32
    hs = synth.hand_sides(1)
    y, uv = NV.synth_planes(4, 0, 1, H, W, pitch=32)          # pitch 32 at f = 2: the wide path if the upload is aligned
    e.set_option('detect_scale', '2')
    try:
        n0, c0 = e.counter('detect_scale_steps'), e.counter('crop_nv12_launches')
        e.track_reset()
        a, rows = NV.profile_rows(e, lambda: e.track_step_nv12(y, uv, hs, W=W, want_kpmap=True))
        e.track_reset()
        b, rows8 = NV.profile_rows(e, lambda: e.track_step_u8(NV.to_rgb(y, uv, W, 'bt709'), hs, want_kpmap=True))
        NV.assert_equal_outputs(a, b)
        assert a['detected'][0] == 1
        assert rows.count('downscale_nv12') == 1 and rows.count('crop_and_resize_nv12') == 1 and not [r for r in rows if r.startswith('preprocess')]
        assert [r.replace('_nv12', '_u8') for r in rows] == rows8
        assert e.counter('detect_scale_steps') == n0 + 2 and e.counter('crop_nv12_launches') == c0 + 1
    finally:
        e.set_option('detect_scale', '1')
        e.track_reset()


def test_partial_detect_step(net_engine):
    """B = 2, track_partial_detect = 1 at detect_scale = 2: seeded so that the tracked step loses frame 1 only
    (tests/helpers/track_partial_oracle.py), then the partial detect step, which builds the detection frame of the lost frame alone
    (downscale_nv12_idx) and crops both frames from the planes.  (The f = 1 form of the partial step, preprocess_nv12_idx, is held to
    preprocess_u8 by test_downscale_bit_exact and runs inside a step in tests/test_gpu_nv12.py.)"""
    e = net_engine
    B, H, W = 2, 32, 32
    hs = synth.hand_sides(B)
    planes = [NV.synth_planes(21, t, B, H, W, pitch=36, tail_rows=1) for t in range(2)]
    e.set_option('track_partial_detect', '1')
    e.set_option('detect_scale', '2')
    try:
        res = []
        for nv in (True, False):
            c, s = TP.seed_boxes(B, H, W, [1])
            e.track_seed(c, s, H, W)
            outs = []
            for t in range(2):
                y, uv = planes[t]
                call = (lambda: e.track_step_nv12(y, uv, hs, W=W, want_kpmap=True)) if nv else \
                       (lambda: e.track_step_u8(NV.to_rgb(y, uv, W, 'bt709'), hs, want_kpmap=True))
                outs.append(NV.profile_rows(e, call))
            res.append(outs)
        for t in range(2):
            NV.assert_equal_outputs(res[0][t][0], res[1][t][0], t)
        assert res[0][0][0]['lost'].tolist() == [0, 1] and res[0][1][0]['detected'].tolist() == [0, 1]
        NV.assert_tracked_rows(res[0][0][1])
        rows = res[0][1][1]
        assert rows.count('downscale_nv12_idx') == 1 and rows.count('crop_and_resize_nv12') == 1
        assert not [r for r in rows if r.startswith('preprocess') or r == 'downscale_nv12' or '_u8' in r]
    finally:
        e.set_option('track_partial_detect', '0')
        e.set_option('detect_scale', '1')
        e.track_reset()


def test_hands_step_compacted(emu_engine, synth_weights):
    """track_hands_step_nv12 at K = 2 with hands_compact: slot 1 absent (tests/test_hands_compact.py's seed), one tracked step."""
    from hand3d_amd import _lib
    H, W, K = 32, 32, 2
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        e.set_option('hands_compact', '1')
        hs = HO.hand_sides(1, K)
        center = np.array([[[H / 2, W / 2], [7.0, 9.0]]], F32)
        scale, valid = np.array([[10.0, 3.0]], F32), np.array([[1, 0]], np.int32)
        y, uv = NV.synth_planes(2, 0, 1, H, W, pitch=34)
        e.track_hands_seed(center, scale, valid, H, W)
        n0 = e.counter('crop_nv12_launches')
        a, rows = NV.profile_rows(e, lambda: e.track_hands_step_nv12(y, uv, hs, K, W=W, want_kpmap=True))
        e.track_hands_seed(center, scale, valid, H, W)
        b = e.track_hands_step_u8(NV.to_rgb(y, uv, W, 'bt709'), hs, K, want_kpmap=True)
        NV.assert_equal_outputs(a, b)
        assert a['valid'][0].tolist() == [1, 0]
        NV.assert_tracked_rows(rows, idx=True)
        assert e.counter('crop_nv12_launches') == n0 + 1
    finally:
        e.close()
