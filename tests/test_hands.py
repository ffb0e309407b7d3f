"""Several hands per frame on the CPU interpreter: the mask stage of hp3d_infer_hands (glue.hip:
mask_grow_multi_kernel / mask_grow_multi_global_kernel through hp3d_masks_from_scoremap) bit for bit against the rule written with
oracle.general's functions (tests/helpers/hands_oracle.py), both forms of the kernel against each other, the C surface's errors, and
the whole path on a small frame (marked slow like the other whole-path interpreter tests: minutes per image;
tests/test_gpu_hands.py runs the same helpers on the GPU at the shipped shapes)."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth
from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO      # noqa: E402

F32 = np.float32
skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per image on the CPU interpreter; set HP3D_SLOW=1")


class min_area(object):
    def __init__(self, e, n):
        self.e, self.n = e, n

    def __enter__(self):
        self.e.set_option('hands_min_area', str(self.n))

    def __exit__(self, *a):
        self.e.set_option('hands_min_area', '0')


def check_all(e, sm, K, area=0):
    """Exact against the rule, both kernel forms equal, K = 1's slot equal to the single-hand op."""
    got = HO.assert_masks_exact(e, sm, K, area)
    both = HO.assert_lds_equals_global(e, sm, K)
    for k in HO.MASK_KEYS:
        assert np.array_equal(got[k], both[k]), k
    if area == 0:
        HO.assert_slot0_is_single_hand(e, sm, got)
    return got


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("case", ['one_blob', 'two_blobs_gap10', 'two_blobs_gap11', 'full', 'border'])
def test_mask_cases(emu_engine, case, K):
    sm = synth.blob_scoremap(case)
    got = check_all(emu_engine, sm, K)
    # (two_blobs_gap10: its rectangles are 10 background pixels apart, columns 50..59.  A 21 x 21 dilation reaches column 59 from
    #  column 49 and not column 60, so the oracle -- and hp3d_mask_from_scoremap today: area 900 -- keeps them apart: two hands, not
    #  the one hand and an absent slot the case's name suggests.  What is asserted is what the rule gives.)
    nobj = 2 if case.startswith('two_blobs') else 1
    assert got['valid'][0].tolist() == [1 if j < nobj else 0 for j in range(K)]
    if nobj == 2 and K >= 2:
        # score order: the 1.2-strength rectangle (columns 20..49) first
        assert 20 <= got['seed'][0, 0, 1] < 50 and 60 <= got['seed'][0, 1, 1] < 90
        assert got['area'][0, :2].tolist() == [900, 900 if case == 'two_blobs_gap10' else 29 * 30]
    if case == 'full':
        assert got['area'][0, 0] == 120 * 160
    for j in range(nobj, K):
        assert got['seed'][0, j].tolist() == [-1, -1] and got['area'][0, j] == 0 and not got['mask'][0, j].any()
        assert got['crop_size'][0, j] == 100.0 and got['center'][0, j].tolist() == [160.0, 160.0]


@pytest.mark.parametrize("mode", ["inf", "fltmax"])
def test_empty_map_every_slot_absent(emu_engine, monkeypatch, mode):
    sm = synth.blob_scoremap('empty')
    monkeypatch.setattr(G, 'EMPTY_REDUCE', mode)
    emu_engine.set_option('empty_reduce', mode)
    try:
        for K in (1, 2, 3):
            got = check_all(emu_engine, sm, K)
            assert not got['valid'].any() and not got['area'].any() and not got['mask'].any()
            assert np.all(got['crop_size'] == 100.0)
            assert np.all(got['center'] == (160.0 if mode == 'inf' else 0.0))
            # slot 0 keeps the single-hand seed (the global arg-max), the others have none
            assert np.array_equal(got['seed'][:, 0], emu_engine.mask_from_scoremap(sm)[4])
            assert np.all(got['seed'][:, 1:] == -1)
    finally:
        emu_engine.set_option('empty_reduce', 'inf')


RECTS5 = [(10, 30, 10, 40, 3.0), (10, 40, 70, 90, 5.0), (60, 100, 20, 50, 4.0), (70, 90, 90, 120, 2.0), (100, 118, 130, 158, 6.0)]


@pytest.mark.parametrize("n,K", [(3, 2), (3, 4), (5, 2), (5, 4)])
def test_more_and_fewer_objects_than_slots(emu_engine, n, K):
    rects = RECTS5[:n]
    got = check_all(emu_engine, HO.rect_scoremap(rects), K)
    order = sorted(rects, key=lambda r: -r[4])
    assert got['valid'][0].sum() == min(n, K)
    for j in range(min(n, K)):
        y0, y1, x0, x1, _ = order[j]
        assert got['seed'][0, j].tolist() == [y0, x0] and got['area'][0, j] == (y1 - y0) * (x1 - x0)
        assert got['center'][0, j].tolist() == [0.5 * (y0 + y1 - 1), 0.5 * (x0 + x1 - 1)]


def test_equal_scores_tie_goes_to_the_first_pixel(emu_engine):
    got = check_all(emu_engine, HO.rect_scoremap([(50, 70, 10, 30, 3.0), (20, 40, 100, 130, 3.0), (21, 30, 40, 60, 3.0)]), 3)
    assert got['seed'][0].tolist() == [[20, 100], [21, 40], [50, 10]]


def test_speck_below_min_area_is_dropped(emu_engine):
    sm = HO.rect_scoremap([(10, 12, 10, 12, 6.0), (60, 80, 60, 80, 3.0)])
    with min_area(emu_engine, 10):
        for K in (1, 2):
            got = check_all(emu_engine, sm, K, 10)
            assert got['valid'][0].tolist() == [1, 0][:K] and got['seed'][0, 0].tolist() == [60, 60] and got['area'][0, 0] == 400
    got = check_all(emu_engine, sm, 2)          # off: the speck is hand 0
    assert got['valid'][0].tolist() == [1, 1] and got['area'][0].tolist() == [4, 400]


def test_more_specks_than_tries(emu_engine):
    specks = [(5 + 20 * i, 7 + 20 * i, 5 + 25 * i, 7 + 25 * i, 9.0 - i) for i in range(5)]
    sm = HO.rect_scoremap(specks + [(90, 115, 10, 40, 3.0)])
    with min_area(emu_engine, 10):
        got = check_all(emu_engine, sm, 1, 10)          # 4 tries, all specks: no hand although one is there
        assert got['valid'][0].tolist() == [0] and got['seed'][0].tolist() == [[-1, -1]]
        got = check_all(emu_engine, sm, 2, 10)          # 8 tries: five specks, then the hand
        assert got['valid'][0].tolist() == [1, 0] and got['area'][0].tolist() == [25 * 30, 0]


def test_serpentine_beyond_the_pass_cap(emu_engine):
    """The reference's pass cap cuts the object short; what it leaves in R comes back as later hands, disjoint from hand 0."""
    H, W = 120, 160
    det = HO.serpentine(H, W)
    sm = np.zeros((1, H, W, 2), F32)
    sm[0, :, :, 1] = np.where(det > 0, 2.0, -2.0)
    sm[0, 0, 0, 1] = 3.0
    _, passes = G.grow_objectmap(det.astype(F32), (0, 0), early_exit=True)
    assert passes == max(H, W) // 10                # the cap binds
    got = check_all(emu_engine, sm, 4)
    single = emu_engine.mask_from_scoremap(sm)[0]
    assert np.array_equal(got['mask'][0, 0], single[0]) and 0 < got['area'][0, 0] < det.sum()
    assert got['valid'][0].tolist() == [1, 1, 1, 1]
    rest = det - single[0]
    first = int(np.argmax(rest.reshape(-1) > 0))
    assert got['seed'][0, 1].tolist() == [first // W, first % W]
    assert got['mask'][0].sum(axis=0).max() == 1 and np.all(got['mask'][0].sum(axis=0) <= det)


def test_properties_over_random_rectangles(emu_engine):
    rng = np.random.default_rng(5)
    H, W = 96, 128
    for trial in range(6):
        rects = []
        for _ in range(int(rng.integers(1, 5))):
            y0, x0 = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 12))
            rects.append((y0, y0 + int(rng.integers(3, 12)), x0, x0 + int(rng.integers(3, 12)), float(rng.uniform(1.0, 6.0))))
        sm = HO.rect_scoremap(rects, H, W)
        det = G.fg_and_detmap(sm)[1][0]
        got = check_all(emu_engine, sm, 4)
        m = got['mask'][0]
        assert m.sum(axis=0).max() <= 1, trial                          # pairwise disjoint
        assert np.all(m <= det[None]), trial                            # each inside det
        assert np.array_equal(m.sum(axis=0), det), trial                # at most four objects: their union is det
        assert np.all(np.diff(got['valid'][0]) <= 0)                    # hands first, absent slots behind


def test_global_form_by_auto_on_a_large_frame(emu_engine):
    H, W = 540, 960
    y, x = np.mgrid[:H, :W]
    sm = np.zeros((1, H, W, 2), F32)
    sm[..., 1] = -2.0
    for cy, cx, s in ((120, 150, 3.0), (400, 800, 4.0)):
        sm[0, :, :, 1] = np.where(((y - cy) / 45.0) ** 2 + ((x - cx) / 35.0) ** 2 <= 1.0, s, sm[0, :, :, 1])
    n_m, n_g = emu_engine.counter('mask_grow_multi_launches'), emu_engine.counter('mask_grow_global_launches')
    got = HO.assert_masks_exact(emu_engine, sm, 3)
    assert (emu_engine.counter('mask_grow_multi_launches'), emu_engine.counter('mask_grow_global_launches')) == (n_m + 1, n_g + 1)
    assert got['valid'][0].tolist() == [1, 1, 0] and got['seed'][0, 0, 0] > 300 and got['seed'][0, 1, 0] < 200
    HO.assert_slot0_is_single_hand(emu_engine, sm, got)


def test_errors_are_loud(emu_engine):
    from hand3d_amd import _lib
    lib, h = emu_engine.lib, emu_engine.h
    sm = synth.blob_scoremap('one_blob')
    for K in (0, 5):
        with pytest.raises(AssertionError, match="max hands"):
            emu_engine.masks_from_scoremap(sm, K)
    assert lib.hp3d_masks_from_scoremap(h, _lib._ptr(sm), 1, 120, 160, -1, *[None] * 7) == -1
    img, hs = synth.make_batch(0, 1, 32, 48), HO.hand_sides(1, 2)
    nul = [None] * 11
    for K in (0, 5):
        assert lib.hp3d_infer_hands(h, 1, 32, 48, K, _lib._ptr(img), _lib._ptr(hs), *nul) == -1
        assert "max hands" in lib.hp3d_last_error(h).decode()
        assert lib.hp3d_infer_hands_dev(h, 1, 32, 48, K, _lib._ptr(img), _lib._ptr(hs), *nul) == -1
        assert lib.hp3d_infer_hands_u8(h, 1, 32, 48, _lib._ptr(img), 32, 48, K, _lib._ptr(hs), *nul) == -1
    assert lib.hp3d_infer_hands(h, 1, 32, 48, 2, _lib._ptr(img), None, *nul) == -1
    assert "hand_side is NULL" in lib.hp3d_last_error(h).decode()
    assert lib.hp3d_infer_hands(h, 1, 32, 48, 2, None, _lib._ptr(hs), *nul) == -1
    assert lib.hp3d_infer_hands_u8(h, 1, 32, 48, None, 32, 48, 2, _lib._ptr(hs), *nul) == -1
    assert lib.hp3d_infer_hands(None, 1, 32, 48, 2, None, None, *nul) == -1
    assert lib.hp3d_masks_from_scoremap(h, None, 1, 32, 48, 2, *[None] * 7) == -1
    for bad in ('-1', 'x', '1.5'):
        with pytest.raises(AssertionError, match="hands_min_area"):
            emu_engine.set_option('hands_min_area', bad)
    emu_engine.set_option('mask_grow', 'lds')
    try:
        with pytest.raises(AssertionError, match="map too large"):
            emu_engine.masks_from_scoremap(np.zeros((1, 540, 960, 2), F32), 2)
        with pytest.raises(AssertionError, match="too large for the in-LDS mask growth"):
            emu_engine.infer_hands(np.zeros((1, 540, 960, 3), F32), HO.hand_sides(1, 2), 2)
    finally:
        emu_engine.set_option('mask_grow', 'auto')


def test_python_surface_shapes():
    """ColorHandPose3DNetwork.inference_hands and the binding agree with the header on the limit."""
    from hand3d_amd import _lib
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    assert _lib.MAX_HANDS == 4 and hasattr(ColorHandPose3DNetwork, 'inference_hands')
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hp3d.h')).read()
    assert '#define HP3D_MAX_HANDS 4' in hdr


@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


@pytest.mark.slow
@skip_unless_slow
def test_k1_is_infer_full(net_engine):
    HO.assert_k1_is_infer_full(net_engine, synth.make_batch(3, 1, 32, 48))


@pytest.mark.slow
@skip_unless_slow
def test_two_slots_whole_path(net_engine):
    """B = 1, K = 2 on a small frame: the mask stage exact on the device's own score map, slot 0 the K = 1 call's, the back half the
    chain of per-op calls on the one frame (the crop's box-to-image stride), one multi-hand growth per call."""
    n = net_engine.counter('mask_grow_multi_launches')
    HO.check_whole_path(net_engine, synth.make_batch(3, 1, 32, 48), 2, expect_all_valid=False)
    assert net_engine.counter('mask_grow_multi_launches') == n + 2          # the K = 2 call and the K = 1 call inside the check


def test_lds_kernel_statics_leave_room_for_the_largest_map(tmp_path):
    """hipFuncSetAttribute refuses a dynamic LDS limit that, with the kernel's static LDS, passes 160 KB -- and the refusal stays behind
    as the stream's last error.  The multi-hand LDS kernel asks for 160 KB - 1 KB (the largest map mask_grow_lds_fits admits): its
    statics in the SHIPPED code object must fit the remaining 1 KB."""
    import glob
    import re
    import shutil
    import subprocess
    from hand3d_amd import _lib, build
    build.build(verbose=False)
    lib = str(tmp_path / 'libhp3d.so')
    shutil.copy(_lib.DEFAULT_LIB, lib)
    subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-objdump', '--offloading', lib], capture_output=True, text=True, cwd=str(tmp_path))
    cos = [f for f in glob.glob(str(tmp_path / '*')) if 'gfx950' in os.path.basename(f) and f != lib]
    assert cos
    notes = ''.join(subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--notes', f], capture_output=True, text=True).stdout for f in cos)
    static = dict((name, int(size)) for size, name in re.findall(r'\.group_segment_fixed_size:\s*(\d+)\n(?:.*\n)*?\s*\.name:\s*(\S+)', notes))
    multi = [v for k, v in static.items() if 'mask_grow_multi_kernel' in k]
    assert len(multi) == 1 and 0 < multi[0] <= 1024, static
    src = open(os.path.join(os.path.dirname(_lib.DEFAULT_LIB), 'csrc', 'glue.hip')).read()
    assert re.search(r'mask_grow_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 \* 1024 - 1024\)', src)
