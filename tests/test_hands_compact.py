"""Option "hands_compact"  on the CPU interpreter, everything bit for bit: the indexed crop against the oracle's crop on
the gathered frames and boxes for every subset of valid slots, the scatter in its 16-byte and its 4-byte form, the option's parsing,
that the option off enqueues none of the new launches, and one compacted tracked step at B = 1, K = 2 with an absent slot against the
composition at batch 1 and the restated state machine (tests/helpers/hands_compact_oracle.py).  The interpreter's time is PoseNet2D per
slot, so longer sequences are marked slow (HP3D_SLOW=1); tests/test_gpu_hands_compact.py runs the same helper on the GPU."""
import itertools
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

F32 = np.float32
skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per step on the CPU interpreter; set HP3D_SLOW=1")


def _boxes(rng, n, H, W):
    center = rng.uniform([-4.0, -4.0], [H + 4.0, W + 4.0], (n, 2)).astype(F32)          # (some windows leave the frame: the 0 fill)
    scale = rng.uniform(0.6, 6.0, n).astype(F32)
    return center, scale


def test_indexed_crop_every_subset_of_slots(emu_engine):
    """B = 2, K = 3 at 48 x 64: every subset of the six slots, the empty one, the full one and the last slot alone included."""
    e = emu_engine
    B, K, H, W, crop = 2, 3, 48, 64, 24
    rng = np.random.default_rng(5)
    frame = synth.make_batch(3, B, H, W)
    u8 = TO.to_u8(frame)
    fu8 = G.preprocess_u8(u8, H, W)
    center, scale = _boxes(rng, B * K, H, W)
    ref = G.crop_image_from_xy(np.repeat(frame, K, axis=0), center, crop, scale)
    ref8 = G.crop_image_from_xy(np.repeat(fu8, K, axis=0), center, crop, scale)
    assert np.array_equal(ref, e.crop_and_resize(np.repeat(frame, K, axis=0), center, scale, crop))
    n_u8 = e.counter('crop_u8_launches')
    subsets = [s for r in range(B * K + 1) for s in itertools.combinations(range(B * K), r)]
    assert len(subsets) == 64 and () in subsets and (B * K - 1,) in subsets and tuple(range(B * K)) in subsets
    for sub in subsets:
        idx = np.array(sub, np.int32)
        got = e.crop_and_resize_idx(frame, center, scale, idx, K, crop)
        assert got.shape == (len(sub), crop, crop, 3) and np.array_equal(got, ref[idx]), sub
        got8 = e.crop_and_resize_idx(u8, center, scale, idx, K, crop)
        assert np.array_equal(got8, ref8[idx]), sub
    assert e.counter('crop_u8_launches') == n_u8 + 63          # (the empty subset launches nothing)
    # an index that is no slot is refused before any launch
    with pytest.raises(AssertionError, match="no slot"):          # (HP3D_ERR_ARG: the binding raises it as the reference's bare asserts)
        e.crop_and_resize_idx(frame, center, scale, np.array([B * K], np.int32), K, crop)


@pytest.mark.parametrize('words', [8192 + 40, 63, 4])
def test_scatter_both_forms(emu_engine, words):
    """A 16-byte aligned destination (16-byte loads and stores where the slot size allows) and one 4 bytes off (the 4-byte form): the
    same result, absent slots exactly 0, the words behind the last slot untouched.  8232 words: more than one segment per slot."""
    e = emu_engine
    rng = np.random.default_rng(words)
    for pos in ([1, -1, 0, -1, 2], [-1, -1, -1], [0, 1, 2], [-1, -1, 0]):
        pos = np.array(pos, np.int32)
        m = int(pos.max()) + 1
        dense = rng.standard_normal((m, words)).astype(F32)
        exp = np.zeros((pos.size, words), F32)
        exp[pos >= 0] = dense[pos[pos >= 0]]
        for skew in (0, 1):
            out, tail = e.slot_scatter(dense, pos, skew_words=skew, sentinel=-7.0)
            assert np.array_equal(out, exp), (pos.tolist(), skew)
            assert np.array_equal(tail, np.full(4, -7.0, F32)), (pos.tolist(), skew)
            assert not out[pos < 0].any()
    # bits, not floats: int32 payloads (keypoint_hw_crop) and NaN patterns survive
    ints = rng.integers(-2 ** 31, 2 ** 31 - 1, (2, words), dtype=np.int64).astype(np.int32)
    out, _ = e.slot_scatter(ints, np.array([1, -1, 0], np.int32), skew_words=3)
    assert out.dtype == np.int32 and np.array_equal(out, np.stack([ints[1], np.zeros(words, np.int32), ints[0]]))


def test_option_parsing(emu_engine):
    e = emu_engine
    for bad in ('2', '-1', 'on', '', '01'):
        assert e.lib.hp3d_set_option(e.h, b'hands_compact', bad.encode()) == -1          # HP3D_ERR_ARG
        assert 'hands_compact' in e.lib.hp3d_last_error(e.h).decode()
    with pytest.raises(AssertionError, match="hands_compact wants 0 or 1"):
        e.set_option('hands_compact', '2')
    e.set_option('hands_compact', '1')
    e.set_option('hands_compact', '0')


def test_python_surface():
    import inspect
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    assert inspect.signature(ColorHandPose3DNetwork.inference_hands).parameters['compact'].default is None
    assert inspect.signature(ColorHandPose3DNetwork.track_hands).parameters['compact'].default is None


class _RecordingEngine(object):
    """What ColorHandPose3DNetwork's multi-hand wrappers touch of an Engine: the option writes are recorded."""

    def __init__(self):
        self.options = []

    def set_option(self, key, value):
        self.options.append((key, value))

    def _outputs(self, B, K):
        z = lambda *s: np.zeros((B, K) + s, F32)
        return {'scoremap': np.zeros((B, 8, 8, 2), F32), 'crop': z(256, 256, 3), 'scale': z(), 'center': z(2), 'kpmap': z(256, 256, 21),
                'coord3d': z(21, 3), 'kp_hw': z(21, 2), 'kp_crop': np.zeros((B, K, 21, 2), np.int32), 'confidence': z(),
                'lost': z(), 'detected': z(), 'valid': z(), 'area': z()}

    def infer_hands(self, image, hand_side, max_hands):
        return self._outputs(len(image), max_hands)

    def track_hands_step(self, image, hand_side, max_hands):
        return self._outputs(len(image), max_hands)


def test_wrappers_write_the_option_only_when_asked_and_only_on_change():
    """compact=None leaves the engine's option alone (an engine-level set_option survives, no captured graph is dropped); True / False
    write it once, not on every frame; both wrappers share what was last written."""
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    eng = _RecordingEngine()
    net = ColorHandPose3DNetwork(engine=eng)
    img, hs = np.zeros((1, 8, 8, 3), F32), HO.hand_sides(1, 2)
    net.track_hands(img, hs, 2)
    net.inference_hands(img, hs, 2)
    assert eng.options == []
    for _ in range(3):
        net.track_hands(img, hs, 2, compact=True)
    net.inference_hands(img, hs, 2, compact=True)
    net.track_hands(img, hs, 2)
    assert eng.options == [('hands_compact', '1')]
    net.inference_hands(img, hs, 2, compact=False)
    net.track_hands(img, hs, 2, compact=False)
    assert eng.options == [('hands_compact', '1'), ('hands_compact', '0')]


@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


def test_option_off_enqueues_nothing_new(net_engine):
    """B = 1, K = 1 at 32 x 32 with the option at its default: one multi-hand tracking step and one hp3d_infer_hands show none of the
    new profile rows and move none of the new counters."""
    e = net_engine
    e.set_option('hands_compact', '1')
    e.set_option('hands_compact', '0')
    frame, hs = synth.make_batch(0, 1, 32, 32), HO.hand_sides(1, 1)
    c0 = HCO.counters(e)
    e.track_hands_reset()
    e.set_profiling(1)
    try:
        e.track_hands_step(frame, hs, 1)
        rows = [r[0] for r in e.profile()]
        e.infer_hands(frame, hs, 1)
        rows += [r[0] for r in e.profile()]
    finally:
        e.set_profiling(0)
        e.track_hands_reset()
    assert 'crop_and_resize' in rows and 'track_hands_box' in rows and not set(rows) & set(HCO.NEW_ROWS)
    assert HCO.counters(e) == c0


def test_compacted_tracked_step_with_an_absent_slot(emu_engine, synth_weights):
    """B = 1, K = 2 at 240 x 320, PoseNet2D + lifting weights only: slot 0 seeded at the frame's centre with scale 10, slot 1 absent.
    One tracked step with the option on: one slot runs, one is skipped, no wait, no HandSegNet; slot 0 equals the composition at batch
    1, slot 1 the absent rule, the next state the restated machine's."""
    from hand3d_amd import _lib
    H, W, K = 240, 320, 2
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        e.set_option('hands_compact', '1')
        hs = HO.hand_sides(1, K)
        center = np.array([[[H / 2, W / 2], [7.0, 9.0]]], F32)
        scale, valid = np.array([[10.0, 3.0]], F32), np.array([[1, 0]], np.int32)
        e.track_hands_seed(center, scale, valid, H, W)
        m = THO.Machine()
        m.seed(center, scale, valid, H, W)
        held_c, held_s = m.center.copy(), m.scale.copy()
        c0 = HCO.counters(e)
        o, detect, ms = HCO.step_and_check(e, m, TO.frames(2, 0, 1, H, W), hs, K, per_chunk=1)
        assert not detect and ms == [1]
        assert tuple(np.subtract(HCO.counters(e), c0)) == (1, 1, 0)
        assert o['valid'][0].tolist() == [1, 0] and not o['lost'].any() and not o['detected'].any()
        assert o['confidence'][0, 1] == 0.0 and o['confidence'][0, 0] != 0.0
        assert np.array_equal(o['center'], held_c) and np.array_equal(o['scale'], held_s)          # slot 1: the held fall-back box
        assert np.array_equal(m.center[0, 1], held_c[0, 1]) and m.scale[0, 1] == held_s[0, 1] and m.lost[0, 1] == 0
    finally:
        e.close()


@pytest.mark.slow
@skip_unless_slow
def test_detect_step_and_infer_hands_with_absent_slots(net_engine):
    """B = 1, K = 2 at 48 x 64, all weights: a fresh detect step and hp3d_infer_hands with the option on against the option off."""
    e = net_engine
    H, W, K = 48, 64, 2
    frame, hs = TO.frames(7, 0, 1, H, W), HO.hand_sides(1, K)
    off = e.infer_hands(frame, hs, K, want_mask=True)
    e.set_option('hands_compact', '1')
    try:
        HCO.infer_hands_and_check(e, frame, hs, K, per_chunk=1, off=off)
        e.track_hands_reset()
        o, detect, _ = HCO.step_and_check(e, THO.Machine(), frame, hs, K, per_chunk=1)
        assert detect
    finally:
        e.set_option('hands_compact', '0')
        e.track_hands_reset()
