"""The multi-layer kernels held to the float64 oracle BIT FOR BIT on integer data (oracle/chain_exact.py): the 1x1 head pairs of
HandSegNet / PoseNet2D as one launch each (conv_pw2.hip) and as two, and the lifting stage on every path -- lift_fused.hip's nine
phases, the layer-by-layer form with fc_partial + fc_reduce or fc_tail and with conv_s2_gemm or the direct kernel, on one stream
and on two.

* Every value that meets a leaky-ReLU is >= 0 or a negative multiple of 100 (fl32(0.01f * (-100 m)) == -m), so a whole chain of
  layers stays integer; the preconditions (integer taps, |w| |x| bound below 2^24, the negative branch taken by a quarter of a
  layer's values at least, no constant or unread channel) are asserted on the oracle's taps before a kernel runs.
* conv_impl = direct throughout: the Winograd kernels the default policy picks for 3x3 layers have filter transforms with
  denominators 3 and 6 and cannot be exact on these weights (they have their own exact tests on multiples of 36 / 576).
* Counters prove which path ran.
* R and rel pass through sinf / cosf and cannot be exact.  They are anchored twice: across paths (the path lift_fused = 0,
  fc_tail = 0, tiny_gemm = 0 consists of kernels test_gpu_conv_exact.py pins one by one; every other path must give the same bits),
  and on a data set whose u is an integer vector with |u|_inf <= 8, where one unit in any component moves the rotation matrix by
  more than 0.05: there R matches the oracle within TOL_KP3D and rel within TOL_KP3D max |can|.
Not pinned here: lift_epilogue's own arithmetic beyond that tolerance, bone_rel_inv and the 'local' variant.
"""
import contextlib

import numpy as np
import pytest

from hand3d_amd import synth
from oracle import chain_exact as C
from oracle import conv_exact as X

pytestmark = pytest.mark.gpu

TOL_KP3D = 1e-4                        # the project's gate on 3-D outputs (tests/test_gpu_parity.py)
DEFAULTS = {'conv_impl': 'mfma', 'pw2': '1', 'lift_fused': 'auto', 'fc_tail': '1', 'tiny_gemm': '1', 'lift_overlap': '1', 'kp_up_side': '1'}
NOT_DIRECT = ['conv_first_launches', 'conv_wino_launches', 'conv_wino2_launches', 'conv_wino4_launches', 'conv_wino4s_launches',
              'conv_wino7_launches', 'conv_wino4_tail_launches', 'conv_wino4s_tail_launches', 'conv_wino7_split_launches']
PATH_COUNTERS = ['conv_pw2_launches', 'lift_fused_launches', 'fc_tail_launches', 'conv_s2_gemm_launches', 'lift_overlap_calls', 'conv_mfma_launches']
HEAD_SEED = 1                          # oracle.chain_exact.head_weights(HEAD_SEED): the set the preconditions were established with


@contextlib.contextmanager
def options(e, **kv):
    """Engine options for the duration of the block; the defaults come back whatever happens inside."""
    try:
        for k, v in kv.items():
            e.set_option(k, v)
        yield
    finally:
        for k in kv:
            e.set_option(k, DEFAULTS[k])


@contextlib.contextmanager
def counted(e, out):
    c0 = {c: e.counter(c) for c in NOT_DIRECT + PATH_COUNTERS}
    yield
    out.update({c: e.counter(c) - c0[c] for c in c0})


def restore(e, synth_weights):
    for k, v in DEFAULTS.items():
        e.set_option(k, v)
    e.load_weight_dict(synth_weights)
    e.finalize_weights()


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def mismatch(y, r):
    return X.exact_mismatch(y, np.asarray(r, np.float64))


# ---------------------------------------------------------------------------------------------------------- head pairs
# (B, H, W, calls, image seed): the data set is `calls` batches of B images.  Map pixels per call (a tile of conv_pw2.hip is 64 pixels):
# 4, 63, 64, 65, 129 and a multi-image case above 256; the 4-pixel case takes three calls for every channel to vary.
HEAD_CASES = [(1, 16, 16, 3, 1), (7, 24, 24, 1, 0), (1, 64, 64, 1, 0), (1, 40, 104, 1, 0), (1, 24, 344, 1, 0), (3, 80, 96, 1, 0)]


def head_data(case):
    """(weights, images, {net: (oracle outputs, fraction of negative hidden pre-activations per pair)}), preconditions asserted."""
    B, H, W, calls, seed = case
    w = cached('head_w', lambda: C.head_weights(HEAD_SEED))
    img = C.head_image(seed, B * calls, H, W)
    ref = {}
    for net in ('HandSegNet', 'PoseNet2D'):
        out, taps, bound = C.head_reference(w, img, net)
        ref[net] = (out, C.check_heads(w, taps, bound, net))
    return w, img, ref


def head_run(e, img, B, mode):
    """HandSegNet's small score map and PoseNet2D's three maps of every batch of B images with pw2 = mode; counters asserted."""
    d = {}
    calls = img.shape[0] // B
    with options(e, conv_impl='direct', pw2=mode), counted(e, d):
        outs = [[e.handsegnet(img[i * B:(i + 1) * B], want_small=True)[1]] + list(e.posenet2d(img[i * B:(i + 1) * B])) for i in range(calls)]
    assert d['conv_pw2_launches'] == (4 * calls if mode == 'force' else 0), (mode, d)
    assert all(d[c] == 0 for c in NOT_DIRECT), (mode, d)
    return [np.concatenate([o[j] for o in outs], axis=0) for j in range(4)]


def head_case(e, case, modes=('force', '0')):
    """One launch per pair (pw2 = force) and two (pw2 = 0): all four score maps bit-equal to the float64 oracle."""
    w, img, ref = head_data(case)
    want = ref['HandSegNet'][0] + ref['PoseNet2D'][0]
    for mode in modes:
        got = head_run(e, img, case[0], mode)
        for name, y, r in zip(('HandSegNet small', 'PoseNet2D 1', 'PoseNet2D 2', 'PoseNet2D 3'), got, want):
            assert mismatch(y, r) == 0, "pw2=%s %s %s: %d of %d values differ" % (mode, case, name, mismatch(y, r), r.size)
    print("head pairs %s: negative hidden pre-activations %s" % (case, {k: '%.0f %%' % (100 * v) for n in ref for k, v in ref[n][1].items()}))


@pytest.fixture(scope='module')
def head_engine(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(cached('head_w', lambda: C.head_weights(HEAD_SEED)))
    gpu_engine.finalize_weights()
    yield gpu_engine
    restore(gpu_engine, synth_weights)


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "B%d_%dx%d_x%d" % c[:4])
def test_head_pairs_exact(head_engine, case):
    head_case(head_engine, case)


# ---------------------------------------------------------------------------------------------------------- lifting stage
# path -> options.  'anchor' is made of kernels that have exact tests of their own (conv_mfma.hip, hp3d_fc's fc_partial + fc_reduce).
LIFT_PATHS = {
    'fused': dict(lift_fused='1'),
    'auto': dict(lift_fused='auto'),
    'unfused': dict(lift_fused='0'),
    'tail_only': dict(lift_fused='0', tiny_gemm='0'),
    'gemm_only': dict(lift_fused='0', fc_tail='0'),
    'anchor': dict(lift_fused='0', fc_tail='0', tiny_gemm='0'),
    'serial': dict(lift_fused='0', lift_overlap='0'),
}
FUSED_LIMIT = 4                        # lift_fused = auto takes the one-launch form up to this batch


def lift_data(name, n, bottleneck=False):
    """(weights, sm, hs, (rel, can, R, u)) of a data set with a pool of n samples; the preconditions asserted on the oracle's taps."""
    def make():
        w, sm, hs, neg = C.lift_set(name, n, bottleneck=bottleneck)
        rel, can, R, u, taps, bound = C.lift_reference(w, sm, hs, bottleneck, rot=not bottleneck)
        C.check(taps, bound, [k for k in neg if k in taps],
                C.lift_layers(w, taps, sm, hs, bottleneck, towers=('PosePrior',) if bottleneck else ('PosePrior', 'ViewpointNet'),
                              skip=('fc_vp_ux',) if name == 'small_u' else ()))
        return w, sm, hs, (rel, can, R, u)
    return cached(('lift', name, n, bottleneck), make)


def lift_load(e, w):
    e.load_weight_dict(w)
    e.finalize_weights()


def lift_run(e, path, sm, hs, overlap_counts=True):
    """pose3d on `path` (conv_impl = direct); the counters must show that path and no other."""
    opts = dict(LIFT_PATHS[path], conv_impl='direct')
    B = sm.shape[0]
    fused = opts['lift_fused'] == '1' or (opts['lift_fused'] == 'auto' and B <= FUSED_LIMIT)
    d = {}
    with options(e, **opts), counted(e, d):
        out = e.pose3d(sm, hs)
    want = {'lift_fused_launches': int(fused), 'fc_tail_launches': int(not fused and opts.get('fc_tail', '1') == '1'),
            'conv_s2_gemm_launches': int(not fused and opts.get('tiny_gemm', '1') == '1'), 'conv_pw2_launches': 0}
    if overlap_counts:
        want['lift_overlap_calls'] = int(not fused and opts.get('lift_overlap', '1') == '1')
    assert all(d[c] == v for c, v in want.items()) and all(d[c] == 0 for c in NOT_DIRECT), (path, B, d)
    assert (d['conv_mfma_launches'] == 0) == fused, (path, B, d)
    return out


def lift_case(e, name, n, batches, paths=tuple(LIFT_PATHS), overlap_counts=True):
    """Data set `name` at every batch on every path: can bit-equal to the float64 oracle, R and rel bit-identical to the anchor path's.
    A batch given as (B, paths) runs those paths only."""
    w, sm, hs, (rel, can, R, u) = lift_data(name, n)
    lift_load(e, w)
    for B in batches:
        B, ps = B if isinstance(B, tuple) else (B, paths)
        anchor = lift_run(e, 'anchor', sm[:B], hs[:B], overlap_counts)
        for path in ps + ('anchor',):
            if path == 'fused' and B > FUSED_LIMIT + 1:
                continue                          # (the forced one-launch form: the first batch above the limit only)
            o = anchor if path == 'anchor' else lift_run(e, path, sm[:B], hs[:B], overlap_counts)
            assert mismatch(o[1], can[:B]) == 0, "%s B=%d %s: %d of %d can values differ from float64" % (name, B, path, mismatch(o[1], can[:B]), 63 * B)
            assert np.array_equal(o[2], anchor[2]) and np.array_equal(o[0], anchor[0]), "%s B=%d %s: R / rel differ from the anchor path" % (name, B, path)
    return w, sm, hs, (rel, can, R, u)


@pytest.fixture(scope='module')
def lift_engine(gpu_engine, synth_weights):
    yield gpu_engine
    restore(gpu_engine, synth_weights)


GPU_POOL = 33
GPU_BATCHES = (1, 2, 3, 4, 5, 33)      # 5: the first batch above the fused limit; 33 crosses fc_partial's 32-row block ([x | x2] form) and
#                                        gives conv_s2_gemm 528 rows


@pytest.mark.parametrize("name", ['nonneg', 'negconv', 'negfc0', 'negfc1'])
def test_lift_exact_on_every_path(lift_engine, name):
    lift_case(lift_engine, name, GPU_POOL, GPU_BATCHES)


def small_u_case(e, n, batches, paths, overlap_counts=True):
    w, sm, hs, (rel, can, R, u) = lift_case(e, 'small_u', n, batches, paths, overlap_counts)
    assert np.array_equal(u, np.rint(u)) and np.abs(u).max() <= 8 and len(np.unique(u, axis=0)) > 1
    assert C.rot_sensitivity(u) > 0.05, "precondition: one unit of u moves the float64 rotation matrix by %.3f only" % C.rot_sensitivity(u)
    for path in paths:
        B = min(batches[-1], FUSED_LIMIT + 1) if path == 'fused' else batches[-1]
        o = lift_run(e, path, sm[:B], hs[:B], overlap_counts)
        assert np.abs(o[2] - R[:B]).max() < TOL_KP3D, (path, float(np.abs(o[2] - R[:B]).max()))
        assert np.abs(o[0] - rel[:B]).max() < TOL_KP3D * np.abs(can[:B]).max(), (path, float(np.abs(o[0] - rel[:B]).max()), float(np.abs(can[:B]).max()))


def test_lift_rotation_on_small_integer_u(lift_engine):
    """u is an integer vector with |u|_inf <= 8 and a unit in any component moves R by more than 0.05: R within TOL_KP3D of the
    oracle's get_rot_mat(u_ref) means u itself is exact -- on fc_tail (its reduce, fc_vp1, fc_vp_u) and on lift_fused's last phases."""
    small_u_case(lift_engine, GPU_POOL, (1, 4, 5, 33), tuple(LIFT_PATHS))


def interleave_case(e, n, B, paths, repeats=10):
    """A, B, A on one weight set, then one call `repeats` times: a stale activation, partial sum or barrier counter would show as a
    mismatch with the float64 reference."""
    w, sm, hs, (rel, can, R, u) = lift_data('negfc0', n)
    lift_load(e, w)
    a, b = slice(0, B), slice(n - B, n)
    for path in paths:
        for s in (a, b, a) + (b,) * repeats:
            o = lift_run(e, path, sm[s], hs[s])
            assert mismatch(o[1], can[s]) == 0, (path, s)


def test_lift_interleaved_and_repeated_calls(lift_engine):
    interleave_case(lift_engine, GPU_POOL, 4, ('fused', 'unfused'))
    interleave_case(lift_engine, GPU_POOL, 5, ('fused', 'unfused', 'serial'), repeats=2)


def variants_case(e, n, B):
    """PosePriorNetwork variants 'direct' and 'bottleneck' (lift_fused's bn_w branch, fc_bottleneck): the 256 x 256 input is the 32 x 32
    score map repeated over 8x8 blocks, so avgpool8 is exact."""
    for variant, bn in (('direct', False), ('bottleneck', True)):
        w, sm, hs, (rel, can, R, u) = lift_data('negfc1', n, bottleneck=bn)
        lift_load(e, {k: v for k, v in w.items() if k.startswith('PosePrior/')})
        sm256 = np.kron(sm[:B], np.ones((1, 8, 8, 1), np.float32))
        for fused in ('1', '0'):
            d = {}
            with options(e, conv_impl='direct', lift_fused=fused), counted(e, d):
                got = e.poseprior(variant, sm256, hs[:B])
            assert d['lift_fused_launches'] == int(fused) and all(d[c] == 0 for c in NOT_DIRECT), (variant, fused, d)
            assert got[2] is None and np.array_equal(got[0], got[1])
            assert mismatch(got[0], can[:B]) == 0, "%s lift_fused=%s: %d values differ from float64" % (variant, fused, mismatch(got[0], can[:B]))


def test_poseprior_variants_exact(lift_engine):
    variants_case(lift_engine, GPU_POOL, 3)
    variants_case(lift_engine, GPU_POOL, 5)


def test_kp_up_side_bit_identical(lift_engine, synth_weights):
    """Option "kp_up_side": the heat-map up-sampling behind ViewpointNet on the child stream or behind PosePrior on this one -- every
    output of infer_full the same bits at B = 5 (the unfused, two-stream lifting stage)."""
    restore(lift_engine, synth_weights)
    img, hs = synth.make_batch(7300, 5), synth.hand_sides(5)
    keys = ('scoremap', 'crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw')
    outs = {}
    for side in ('1', '0'):
        with options(lift_engine, kp_up_side=side):
            n0 = lift_engine.counter('lift_overlap_calls')
            outs[side] = lift_engine.infer_full(img, hs, want_mask=True, outputs=keys)
            assert lift_engine.counter('lift_overlap_calls') == n0 + 1
    for k in keys + ('mask',):
        assert np.array_equal(outs['1'][k], outs['0'][k]), k
