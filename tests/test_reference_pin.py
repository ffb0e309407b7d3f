"""Parity pinned to the reference's OWN code.

TensorFlow 1.3 cannot be installed, but every line the reference itself wrote is Python.  `oracle/refrun.py` imports the
reference's modules UNMODIFIED with `oracle/tfshim` standing in for `tensorflow` (an eager NumPy implementation of the ~70 TF
calls the reference makes, whose kernels are oracle/tf_ops.py); scripts/make_pin_fixtures.py runs them on the inputs this
module builds and records every result in tests/golden/ref_pin.npz.  These tests check, on the same seeded inputs,

  * oracle/nets.py, oracle/general.py, oracle/relative_trafo.py  ==  the reference's nets / glue / trafo code;
  * hand3d_amd.utils.general (product host helpers)              ==  the reference's TF-free NumPy functions,
    run as they are (detect_keypoints, trafo_coords, EvalUtil, calc_auc: utils/general.py:331-357,522-611,654-659);
  * hand3d_amd.data readers + record packers                      ==  the reference's writer
    (create_binary_db.py:44-88, ast-extracted: the module itself is a script) and its BinaryDbReader /
    BinaryDbReaderSTB (data/*.py) reading the same bytes.

Small results are stored as arrays and compared with the tolerances below; large ones (heat-maps, crops, reader images) as a
digest of their shape and values (`digest`), i.e. compared bit for bit.

What this does NOT pin: the arithmetic inside TensorFlow's kernels (restated in oracle/tf_ops.py; a box with
TF 1.x closes that with scripts/make_tf_fixtures.py -> tests/test_tf13_fixtures.py).
"""
import hashlib
import os

import numpy as np
import pytest

from hand3d_amd import synth
from hand3d_amd.utils import general as PG          # the product's host helpers
from oracle import general as G
from oracle import nets as N
from oracle import relative_trafo as RT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_pin.npz')
INLINE_BYTES = 16384              # results up to this size are stored as arrays, larger ones as digest()
DIGEST_SUFFIX = '.digest'

INFERENCE_SEEDS = (0, 3)
POSEPRIOR_VARIANTS = ('direct', 'bottleneck', 'local', 'local_w_xyz_loss', 'proposed')
MASK_CASES = ('one_blob', 'two_blobs_gap10', 'two_blobs_gap11', 'empty', 'full', 'border')
REDUCE_IDS = ('inf', 'fltmax')
RHD_FLAGS = (dict(use_wrist_coord=True), dict(use_wrist_coord=False), dict(use_wrist_coord=False, hand_crop=True),
             dict(use_wrist_coord=True, scale_to_size=True))
STB_RECORDS = 2
STB_KEYS = ('image', 'keypoint_xyz21', 'keypoint_uv21', 'keypoint_vis21', 'cam_mat', 'hand_side', 'keypoint_scale',
            'keypoint_xyz21_normed', 'scoremap')


def digest(a):
    """sha256 over the shape and the VALUES (float -> float64, everything else -> int64): equal digests = np.array_equal."""
    a = np.asarray(a)
    v = np.ascontiguousarray(a.astype(np.float64 if a.dtype.kind == 'f' else np.int64))
    return hashlib.sha256(repr(tuple(a.shape)).encode() + v.tobytes()).hexdigest()


def _np(x):
    return np.asarray(x).view(np.ndarray)


@pytest.fixture(scope='module')
def R():
    return np.load(GOLDEN)


def same(R, name, a):
    """`a` equals the reference's result bit for bit (value and shape)."""
    a = np.asarray(a)
    if name in R.files:
        assert a.shape == R[name].shape and np.array_equal(a, R[name]), name
    else:
        assert digest(a) == str(R[name + DIGEST_SUFFIX]), name


def close(R, name, a, tol):
    """max |a - reference| <= tol; a result too large to store is held to its digest (exact)."""
    a = np.asarray(a)
    if name in R.files:
        assert a.shape == R[name].shape and np.abs(a - R[name]).max() <= tol, name
    else:
        same(R, name, a)


# ----------------------------------------------------------------------------------------------- inputs (shared with the fixture maker)
def inference_inputs(seed):
    img = synth.make_batch(seed, 1, 240, 320)
    hs = np.array([[0.0, 1.0]], np.float32) if seed % 2 else np.array([[1.0, 0.0]], np.float32)
    return img, hs


def batch_inputs():
    return synth.make_batch(10, 2, 240, 320), synth.hand_sides(2)


def subnet_inputs():
    return synth.make_batch(20, 1, 64, 96), synth.make_batch(21, 1, 64, 64)


def poseprior_inputs(variant):
    w = synth.make_weights(bottleneck=(variant == 'bottleneck'))
    w = {k: v for k, v in w.items() if k.startswith(('PosePrior', 'ViewpointNet'))}
    rng = np.random.default_rng(5)
    sm = (rng.standard_normal((2, 256, 256, 21)) * 0.3).astype(np.float32)
    return w, sm, synth.hand_sides(2)


def _blob_scoremap(H, W, blobs, strength=4.0, seed=0):
    rng = np.random.default_rng(seed)
    sm = np.zeros((1, H, W, 2), np.float32)
    sm[..., 0] = 1.0
    for (y0, y1, x0, x1, s) in blobs:
        sm[0, y0:y1, x0:x1, 1] = s * strength
    sm += (rng.standard_normal(sm.shape) * 0.01).astype(np.float32)
    return sm


def mask_input(case, H=120, W=160):
    blobs = {'one_blob': [(30, 70, 40, 90, 1.0)],
             # the 21x21 dilation bridges a gap of 10 background pixels but not 11
             'two_blobs_gap10': [(30, 60, 20, 50, 1.2), (30, 60, 60, 90, 1.0)],
             'two_blobs_gap11': [(30, 60, 20, 50, 1.2), (30, 60, 61, 90, 1.0)],
             'empty': [], 'full': [(0, H, 0, W, 1.0)], 'border': [(0, 12, 150, W, 1.0)]}[case]
    return _blob_scoremap(H, W, blobs)


def crop_inputs():
    rng = np.random.default_rng(7)
    img = rng.uniform(-0.5, 0.5, (4, 60, 80, 3)).astype(np.float32)
    center = np.array([[30, 40], [0, 0], [59.5, 79.5], [10.25, 70.75]], np.float32)
    size = np.array([[40.0], [0.0], [500.0], [17.3]], np.float32)
    return img, center, size


def bone_inputs():
    rng = np.random.default_rng(11)
    xyz = rng.normal(0, 1, (3, 21, 3)).astype(np.float32)
    xyz[:, 0] = 0
    return xyz


def host_helper_inputs():
    rng = np.random.default_rng(3)
    sms = []
    for trial in range(4):
        sm = rng.standard_normal((40, 56, 21)).astype(np.float32)
        if trial == 1:          # ties: first maximum in row-major order wins
            sm[5, 7, :] = sm[20, 3, :] = 9.0
        if trial == 2:
            sm[:] = 0.0
        sms.append(sm[None] if trial == 3 else sm)
    feeds = []
    for i in range(50):
        gt = rng.normal(0, 10, (21, 2))
        pr = gt + rng.normal(0, 4, (21, 2))
        vis = rng.uniform(size=21) > 0.3
        vis[7] = False                  # a keypoint that never receives data
        feeds.append((gt, vis, pr))
    x = np.linspace(0, 1, 9)
    y = rng.uniform(size=9)
    return {'scoremaps': sms, 'center': np.array([[120.5, 160.25]]), 'scale': np.array([[1.7]]), 'feeds': feeds,
            'auc_x': x, 'auc_y': y}


def _rhd_sample(rng, left):
    img = rng.integers(0, 256, (320, 320, 3), dtype=np.uint8)
    mask = np.zeros((320, 320), np.uint8)
    mask[100:180, 90:200] = 5 if left else 20
    mask[10:20, 10:30] = 20 if left else 5
    xyz = rng.normal(0, 0.05, (42, 3)).astype(np.float32)
    uv = rng.uniform(60, 250, (42, 2)).astype(np.float32)
    vis = rng.uniform(size=42) > 0.2
    K = np.array([[283.1, 0, 160.0], [0, 283.1, 160.0], [0, 0, 1]], np.float32)
    return img, mask, xyz, uv, vis, K


def rhd_samples():
    rng = np.random.default_rng(0)
    return [_rhd_sample(rng, left=(i % 2 == 0)) for i in range(3)]


def write_stb_records(path):
    from hand3d_amd.data import binary_format as fmt
    rng = np.random.default_rng(2)
    recs = []
    with open(path, 'wb') as f:
        for _ in range(STB_RECORDS):
            img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
            xyz = rng.normal(0, 80, (21, 3)).astype(np.float32) + np.array([0, 0, 600], np.float32)
            uvv = np.concatenate([rng.uniform(100, 400, (21, 2)), (rng.uniform(size=(21, 1)) > 0.2)], 1).astype(np.float32)
            recs.append((img, xyz, uvv))
            f.write(fmt.pack_stb_record(img, xyz, uvv))
    return recs


# ----------------------------------------------------------------------------------------------- networks
@pytest.fixture(scope='module')
def weights():
    return synth.make_weights()


@pytest.mark.parametrize('seed', list(INFERENCE_SEEDS))
def test_inference_reference_code_equals_oracle(R, weights, seed):
    """ColorHandPose3DNetwork.inference (CHP3D.py:61-99), BASELINE config 1 images."""
    img, hs = inference_inputs(seed)
    exp = N.inference(weights, img, hs, True)
    names = ['hand_scoremap', 'image_crop', 'scale_crop', 'center', 'keypoints_scoremap', 'keypoint_coord3d']
    for n, b in zip(names, exp):
        assert b.dtype == np.float32, n
    for i in (0, 1, 2, 3, 4):           # same kernels, same composition: bit-identical
        same(R, 'inference_s%d_%d' % (seed, i), exp[i])
    close(R, 'inference_s%d_5' % seed, exp[5], 1e-6)


def test_inference_batch_and_inference2d_order(R, weights):
    """B = 2 (left + right hand) and inference2d's different return order (CHP3D.py:101-129)."""
    img, hs = batch_inputs()
    exp = N.inference(weights, img, hs, True)
    for i, b in enumerate(exp):
        close(R, 'batch_%d' % i, b, 1e-6)
    e2 = N.inference2d(weights, img)
    assert [a.shape for a in e2] == [(2, 256, 256, 21), (2, 256, 256, 3), (2, 1), (2, 2)]
    for i, b in enumerate(e2):
        same(R, 'batch2d_%d' % i, b)
    # the reference's inference2d returns the very heat-maps / crops of its inference()
    assert str(R['batch2d_0' + DIGEST_SUFFIX]) == str(R['batch_4' + DIGEST_SUFFIX])
    assert str(R['batch2d_1' + DIGEST_SUFFIX]) == str(R['batch_1' + DIGEST_SUFFIX])


def test_subnet_entry_points(R, weights):
    """inference_detection returns a list of 1, inference_pose2d a list of 3 (CHP3D.py:131-219)."""
    img, crop = subnet_inputs()
    assert int(R['detection_len']) == 1 and int(R['pose2d_len']) == 3
    same(R, 'detection_0', N.handsegnet(weights, img)[1][0])
    for i, b in enumerate(N.posenet2d(weights, crop)):
        same(R, 'pose2d_%d' % i, b)


@pytest.mark.parametrize('variant', list(POSEPRIOR_VARIANTS))
def test_poseprior_network_variants(R, variant):
    """PosePriorNetwork(variant).inference (nets/PosePriorNetwork.py:59-95), incl. bone_rel_trafo_inv."""
    w, sm, hs = poseprior_inputs(variant)
    erel, ec3d, eR = N.poseprior_network(w, variant, sm, hs)
    close(R, 'poseprior_%s_rel' % variant, erel, 2e-6)
    close(R, 'poseprior_%s_coord3d' % variant, ec3d, 1e-6)
    assert bool(R['poseprior_%s_has_R' % variant]) == (eR is not None)
    if eR is not None:
        close(R, 'poseprior_%s_R' % variant, eR, 1e-6)


def test_unknown_variant_and_missing_file(R):
    """The reference's messages for an unknown PosePrior variant and a missing weight file; the product and the oracle raise the same."""
    assert str(R['error_unknown_variant']) == "Unknown variant." and str(R['error_missing_file']) == "File not found."
    with pytest.raises(AssertionError, match=str(R['error_unknown_variant'])):
        N.poseprior_network({}, 'nope', np.zeros((1, 256, 256, 21), np.float32), np.array([[1., 0.]], np.float32))
    from hand3d_amd.nets.ColorHandPose3DNetwork import load_weight_files
    with pytest.raises(AssertionError, match=str(R['error_missing_file'])):
        load_weight_files(None, ['/nonexistent.pickle'])


# ----------------------------------------------------------------------------------------------- mask / crop glue
@pytest.mark.parametrize('case', list(MASK_CASES))
@pytest.mark.parametrize('reduce_id', list(REDUCE_IDS))
def test_mask_glue_reference_code_equals_oracle(R, case, reduce_id, monkeypatch):
    """single_obj_scoremap + calc_center_bb (utils/general.py:233-328) on engineered score maps."""
    sm = mask_input(case)
    monkeypatch.setattr(G, 'EMPTY_REDUCE', reduce_id)
    emask = G.single_obj_scoremap(sm)
    ecenter, ebb, esize = G.calc_center_bb(emask)
    k = 'mask_%s_%s_' % (case, reduce_id)
    same(R, k + 'mask', emask)
    same(R, k + 'center', ecenter)
    same(R, k + 'size', esize)
    if case != 'empty':
        same(R, k + 'bb', ebb)
        assert emask.sum() > 0
    else:
        assert emask.sum() == 0 and float(esize[0, 0]) == 100.0
        assert ecenter[0].tolist() == ([160.0, 160.0] if reduce_id == 'inf' else [0.0, 0.0])
    if case == 'two_blobs_gap11':       # the weaker blob must not be reached
        assert emask[0, 30:60, 61:90, 0].sum() == 0


def test_crop_image_from_xy_and_scale(R):
    """crop_image_from_xy (utils/general.py:163-196) + the scale clip of CHP3D.py:84-85."""
    img, center, size = crop_inputs()
    scale = G.scale_from_crop_size(size)
    same(R, 'crop_scale', scale)
    same(R, 'crop_image', G.crop_image_from_xy(img, center, 256, R['crop_scale']))


def test_bone_rel_trafo_roundtrip(R):
    """utils/relative_trafo.py:243-295 (inverse, PosePriorNetwork `local*`) and :148-240 (forward)."""
    xyz = bone_inputs()
    close(R, 'bone_rel', RT.bone_rel_trafo(xyz), 2e-5)
    close(R, 'bone_back', RT.bone_rel_trafo_inv(R['bone_rel']), 2e-5)
    assert np.abs(R['bone_back'] - xyz).max() <= 1e-3


# ----------------------------------------------------------------------------------------------- host helpers (product)
def test_product_host_helpers_equal_reference_functions(R):
    """The product's detect_keypoints / trafo_coords / EvalUtil / calc_auc against the reference's NumPy functions."""
    h = host_helper_inputs()
    for t, sm in enumerate(h['scoremaps']):
        b = PG.detect_keypoints(sm)
        assert b.dtype == R['helpers_kp_%d' % t].dtype == np.float64
        same(R, 'helpers_kp_%d' % t, b)
        same(R, 'helpers_trafo_%d' % t, PG.trafo_coords(b, h['center'], h['scale'], 256))
    with pytest.raises(AssertionError):
        PG.detect_keypoints(np.zeros((21, 40, 56), np.float32))
    pu = PG.EvalUtil()
    for gt, vis, pr in h['feeds']:
        pu.feed(gt[None], vis[None], pr)
    pm = pu.get_measures(0.0, 30.0, 20)
    assert len(pm) == len([k for k in R.files if k.startswith('helpers_measures_')])
    for i, b in enumerate(pm):
        assert np.allclose(R['helpers_measures_%d' % i], b, rtol=1e-13, atol=0)
    for k in (0, 7):
        for name, got in (('helpers_pck_%d' % k, [pu._get_pck(k, 5.0)]), ('helpers_epe_%d' % k, list(pu._get_epe(k)))):
            assert [x is None for x in got] == R[name + '_none'].tolist(), name
            assert all(x is None or x == r for x, r in zip(got, R[name].tolist())), name
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        assert np.isclose(float(R['helpers_auc']), PG.calc_auc(h['auc_x'], h['auc_y']), rtol=1e-14)


# ----------------------------------------------------------------------------------------------- record writer / readers
@pytest.fixture()
def rhd_db(tmp_path, monkeypatch):
    """Three RHD records (the bytes the reference's writer produced: test_record_bytes_equal_reference_writer) in
    ./data/bin/rhd_evaluation.bin of a scratch cwd."""
    from hand3d_amd.data import binary_format as fmt
    samples = rhd_samples()
    os.makedirs(tmp_path / 'data' / 'bin')
    path = tmp_path / 'data' / 'bin' / 'rhd_evaluation.bin'
    with open(path, 'wb') as f:
        for s in samples:
            f.write(fmt.pack_rhd_record(*s))
    monkeypatch.chdir(tmp_path)
    return samples, str(path)


def test_record_bytes_equal_reference_writer(R, rhd_db):
    from hand3d_amd.data import binary_format as fmt
    samples, path = rhd_db
    raw = open(path, 'rb').read()
    assert len(raw) == 3 * fmt.RHD_RECORD_BYTES
    same(R, 'rhd_bytes', np.frombuffer(b''.join(fmt.pack_rhd_record(*s) for s in samples), np.uint8))


@pytest.mark.parametrize('flags', list(RHD_FLAGS))
def test_rhd_reader_equals_reference_reader(R, rhd_db, emu_engine, flags):
    """Product reader vs the reference's BinaryDbReader (data/BinaryDbReader.py) on bytes the reference wrote; the call
    sites are eval2d.py:44, eval2d_gt_cropped.py:37, eval3d.py:48."""
    from hand3d_amd.data import BinaryDbReader
    samples, path = rhd_db
    same(R, 'rhd_bytes', np.frombuffer(open(path, 'rb').read(), np.uint8))
    fi = RHD_FLAGS.index(flags)
    pr = BinaryDbReader(mode='evaluation', shuffle=False, path_to_db=path, engine=emu_engine, **flags)
    it = pr.get()
    for i in range(len(samples)):
        pd = next(it)
        # everything the inference scripts read; training labels (canonical / local frames) are out of scope
        skip = {'keypoint_xyz21_local', 'keypoint_xyz21_can', 'rot_mat'}
        for k in str(R['rhd_f%d_s%d_keys' % (fi, i)]).split():
            if k in skip:
                continue
            assert k in pd, k
            name = 'rhd_f%d_s%d_%s' % (fi, i, k)
            p = np.asarray(pd[k])
            if name in R.files:
                v = R[name]
                assert p.shape == v.shape, (k, p.shape, v.shape)
                if v.dtype == np.bool_ or np.issubdtype(v.dtype, np.integer):
                    assert np.array_equal(p, v), k
                elif k in ('scoremap',):
                    assert np.abs(p - v).max() <= 2e-7, k        # exp(): libm vs NumPy SIMD
                elif k in ('image_crop',):
                    assert np.abs(p - v).max() <= 1e-6, k
                else:
                    assert np.allclose(p, v, rtol=1e-6, atol=1e-6), k
            else:
                same(R, name, p)


def test_stb_reader_equals_reference_reader(R, tmp_path, monkeypatch):
    """BinaryDbReaderSTB (data/BinaryDbReaderSTB.py; eval_full.py:46): xyz in mm, uv+vis triplets, keypoint re-ordering."""
    from hand3d_amd.data import BinaryDbReaderSTB
    os.makedirs(tmp_path / 'data' / 'stb')
    path = tmp_path / 'data' / 'stb' / 'stb_eval.bin'
    recs = write_stb_records(str(path))
    monkeypatch.chdir(tmp_path)
    for wrist in (True, False):
        it = BinaryDbReaderSTB(mode='evaluation', shuffle=False, use_wrist_coord=wrist, path_to_db=str(path)).get()
        for i in range(len(recs)):
            pd = next(it)
            for k in STB_KEYS:
                name = 'stb_w%d_s%d_%s' % (int(wrist), i, k)
                p = np.asarray(pd[k])
                if name in R.files:
                    v = R[name]
                    assert p.shape == v.shape, (k, p.shape, v.shape)
                    if v.dtype == np.bool_:
                        assert np.array_equal(p, v), k
                    else:
                        assert np.allclose(p, v, rtol=1e-6, atol=2e-7), k
                else:
                    same(R, name, p)
