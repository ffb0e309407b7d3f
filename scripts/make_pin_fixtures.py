"""Writes tests/golden/ref_pin.npz: every result of the REFERENCE'S OWN CODE that tests/test_reference_pin.py compares with, taken
by executing the reference's modules (unmodified, through oracle/refrun.py over oracle/tfshim) on the inputs that test module builds.

Small arrays are stored as they are; larger ones (heat-maps, crops, reader images: megabytes each) as a digest of their shape and
values (the test module's `digest()`), so that the test still asserts bit-for-bit equality.  Error messages are stored as strings.  Needs the reference tree (refrun.REFERENCE); the tests need only the file it writes.

    python scripts/make_pin_fixtures.py                 (from the repo root)
"""
import ast
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from hand3d_amd import synth  # noqa: E402
from oracle import general as G  # noqa: E402
from oracle import refrun  # noqa: E402
import test_reference_pin as T  # noqa: E402    (the inputs: one definition, in the test module)

OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_pin.npz')


class Rec(object):
    def __init__(self):
        self.d = {}

    def put(self, name, a):
        a = np.asarray(a).view(np.ndarray)
        if a.nbytes <= T.INLINE_BYTES:
            self.d[name] = a
        else:
            self.d[name + T.DIGEST_SUFFIX] = np.array(T.digest(a))

    def text(self, name, s):
        self.d[name] = np.array(str(s))


def _raises(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    raise RuntimeError('the reference did not raise')


def reference_write_to_binary():
    """create_binary_db.py is a script (it opens the dataset at import): take the function definition only."""
    path = os.path.join(refrun.REFERENCE, 'create_binary_db.py')
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'write_to_binary']
    assert len(fn) == 1
    ns = {}
    exec(compile(ast.Module(body=[ast.parse('import struct').body[0]] + fn, type_ignores=[]), path, 'exec'), ns)
    return ns['write_to_binary']


def main():
    ref = refrun.load()
    assert ref is not None, "needs the reference tree at %s" % refrun.REFERENCE
    assert not hasattr(ref, 'reader_import_error'), ref.reader_import_error
    tf, R = ref.tf, Rec()
    weights = synth.make_weights()
    ref.reset()
    net = ref.ColorHandPose3DNetwork()
    ref.init(net, weights, split=[('HandSegNet',), ('PoseNet2D', 'PosePrior', 'ViewpointNet')])
    np_ = T._np

    # ---- networks
    for seed in T.INFERENCE_SEEDS:
        img, hs = T.inference_inputs(seed)
        for i, o in enumerate(net.inference(tf.constant(img), tf.constant(hs), tf.constant(True))):
            R.put('inference_s%d_%d' % (seed, i), np_(o))
    img, hs = T.batch_inputs()
    for i, o in enumerate(net.inference(tf.constant(img), tf.constant(hs), tf.constant(True))):
        R.put('batch_%d' % i, np_(o))
    for i, o in enumerate(net.inference2d(tf.constant(img))):
        R.put('batch2d_%d' % i, np_(o))
    img, crop = T.subnet_inputs()
    det = net.inference_detection(tf.constant(img))
    R.put('detection_len', len(det))
    R.put('detection_0', np_(det[0]))
    maps = net.inference_pose2d(tf.constant(crop))
    R.put('pose2d_len', len(maps))
    for i, m in enumerate(maps):
        R.put('pose2d_%d' % i, np_(m))
    for variant in T.POSEPRIOR_VARIANTS:
        w, sm, hs = T.poseprior_inputs(variant)
        ref.reset()
        pp = ref.PosePriorNetwork(variant)
        ref.init(pp, w)
        rel, c3d, Rm = pp.inference(tf.constant(sm), tf.constant(hs), tf.constant(True))
        R.put('poseprior_%s_rel' % variant, np_(rel))
        R.put('poseprior_%s_coord3d' % variant, np_(c3d))
        R.put('poseprior_%s_has_R' % variant, Rm is not None)
        if Rm is not None:
            R.put('poseprior_%s_R' % variant, np_(Rm))
    R.text('error_unknown_variant', _raises(lambda: ref.PosePriorNetwork('nope').inference(
        tf.constant(np.zeros((1, 256, 256, 21), np.float32)), tf.constant(np.array([[1., 0.]], np.float32)), tf.constant(True))))
    R.text('error_missing_file', _raises(lambda: ref.ColorHandPose3DNetwork().init(tf.Session(), weight_files=['/nonexistent.pickle'])))

    # ---- mask / crop glue
    saved = G.EMPTY_REDUCE
    try:
        for case in T.MASK_CASES:
            for rid in T.REDUCE_IDS:
                G.EMPTY_REDUCE = rid          # (the shim's reductions follow the oracle's switch)
                mask = ref.general.single_obj_scoremap(tf.constant(T.mask_input(case)))
                center, bb, size = ref.general.calc_center_bb(mask)
                k = 'mask_%s_%s_' % (case, rid)
                R.put(k + 'mask', np_(mask))
                R.put(k + 'center', np_(center))
                R.put(k + 'bb', np_(bb))
                R.put(k + 'size', np_(size))
    finally:
        G.EMPTY_REDUCE = saved
    img, center, size = T.crop_inputs()
    cs = size * np.float32(1.25)
    with np.errstate(divide='ignore'):
        scale = np_(tf.minimum(tf.maximum(256 / tf.constant(cs), 0.25), 5.0))
    R.put('crop_scale', scale)
    R.put('crop_image', np_(ref.general.crop_image_from_xy(tf.constant(img), tf.constant(center), 256, scale=tf.constant(scale))))
    xyz = T.bone_inputs()
    rel = np_(ref.relative_trafo.bone_rel_trafo(tf.constant(xyz)))
    R.put('bone_rel', rel)
    R.put('bone_back', np_(ref.relative_trafo.bone_rel_trafo_inv(tf.constant(rel))))

    # ---- host helpers (the reference's NumPy functions)
    H = ref.general
    h = T.host_helper_inputs()
    for t, sm in enumerate(h['scoremaps']):
        kp = H.detect_keypoints(sm)
        R.put('helpers_kp_%d' % t, kp)
        R.put('helpers_trafo_%d' % t, H.trafo_coords(kp, h['center'], h['scale'], 256))
    ev = H.EvalUtil()
    for gt, vis, pr in h['feeds']:
        ev.feed(gt[None], vis[None], pr)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        for i, m in enumerate(ev.get_measures(0.0, 30.0, 20)):
            R.put('helpers_measures_%d' % i, m)
        for k in (0, 7):          # (None for a keypoint that never received data: stored as NaN + a flag)
            for name, v in (('helpers_pck_%d' % k, [ev._get_pck(k, 5.0)]), ('helpers_epe_%d' % k, list(ev._get_epe(k)))):
                R.put(name, np.array([np.nan if x is None else x for x in v], np.float64))
                R.put(name + '_none', np.array([x is None for x in v]))
        R.put('helpers_auc', H.calc_auc(h['auc_x'], h['auc_y']))

    # ---- record writer / readers
    samples = T.rhd_samples()
    write = reference_write_to_binary()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, 'data', 'bin'))
        path = os.path.join(d, 'data', 'bin', 'rhd_evaluation.bin')
        with open(path, 'wb') as f:
            for s in samples:
                write(f, *s)
        raw = open(path, 'rb').read()
        R.put('rhd_bytes', np.frombuffer(raw, np.uint8))
        os.chdir(d)
        try:
            for fi, flags in enumerate(T.RHD_FLAGS):
                tf.FixedLengthRecordReader.rewind()
                rr = ref.BinaryDbReader(mode='evaluation', shuffle=False, **flags)
                for i in range(len(samples)):
                    rd = {k: np_(v) for k, v in rr.get().items()}
                    R.text('rhd_f%d_s%d_keys' % (fi, i), ' '.join(sorted(rd)))
                    for k, v in rd.items():
                        R.put('rhd_f%d_s%d_%s' % (fi, i, k), v)
        finally:
            os.chdir(cwd)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, 'data', 'stb'))
        T.write_stb_records(os.path.join(d, 'data', 'stb', 'stb_eval.bin'))
        os.chdir(d)
        try:
            for wrist in (True, False):
                tf.FixedLengthRecordReader.rewind()
                rr = ref.BinaryDbReaderSTB(mode='evaluation', shuffle=False, use_wrist_coord=wrist)
                for i in range(T.STB_RECORDS):
                    rd = {k: np_(v) for k, v in rr.get().items()}
                    for k in T.STB_KEYS:
                        R.put('stb_w%d_s%d_%s' % (int(wrist), i, k), rd[k])
        finally:
            os.chdir(cwd)
    np.savez_compressed(OUT, **R.d)
    print('wrote', OUT, '(%d entries, %d bytes)' % (len(R.d), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
