"""Integer data on which a CHAIN of layers must equal the float64 oracle bit for bit (oracle; test infrastructure only): the 1x1
head pairs of HandSegNet / PoseNet2D (conv_pw2.hip) and the lifting stage (lift_fused.hip, fc_partial / fc_reduce / fc_tail,
conv_s2_gemm).  tests/test_chain_exact.py and tests/test_gpu_chain_exact.py use it as test_conv_exact.py uses conv_exact.py.

The multiple-of-100 rule.  A negative value v that passes max(v, 0.01f v) stops being an integer, and the sums behind it then depend
on their order -- unless v = -100 m: fl32(0.01f * (-100 m)) == -m exactly for every integer m <= 2^24 / 100 (slope_identity_holds;
0.01f = 0.00999999977648..., the product errs by 2.2e-8 |v| < 1/2 and lands within half a float32 spacing of -m).  So

    every value that meets a leaky-ReLU is >= 0 or a negative multiple of 100,

and the whole chain stays integer: a layer that exercises the negative branch ('neg') has weights 100 {-1, 0, 1} and a bias that is
a multiple of 100; the layer behind it ('pos') gets a bias that keeps its own pre-activations >= 0 on the data set, because the
-m it reads are no multiples of 100 any more.  check() asserts the rule's consequences on the oracle's own taps before any kernel
runs: every tap an integer, every tap of a second pass over |w|, |b|, |x| (a bound on every partial sum of any summation order)
below 2^24, the 'neg' layers with at least a quarter of their values on either side of zero, and in the layers under test every
input channel with two distinct values over the data set and a non-zero outgoing weight (a dropped channel cannot hide).

The builders fit the biases to a POOL of samples (the data set); the tests' batches are slices of the pool.

head_weights   HandSegNet + PoseNet2D: a "selection" trunk (one tap equal to 1 per output channel, bias 0: every activation is a
               shifted copy of an image channel, values 0 .. 3, so the 3x3 / 7x7 layers cannot grow the numbers) and the four head
               pairs: hidden layer 100 {-1, 0, 1} at fan-in 3 .. 8 with biases 100 {-2 .. 2}, linear layer {-1, 0, 1} covering every
               hidden channel (no leaky-ReLU follows it, so it needs no factor 100; with it conv6_2's 256 terms would pass 2^24).
               conv6_1 / conv7_1 select from the 128 encoding channels of the concat only: a score map (a multiple of nothing,
               negative half of the time) must not reach the five leaky-ReLUs behind them.
lift_weights   PosePrior + ViewpointNet fitted layer by layer to a pool of score maps and hand sides.
rodrigues64    the float64 rotation matrix of nets.get_rot_mat, for the sensitivity precondition of the small-u data set.
"""
import numpy as np

from . import conv_exact as X
from . import nets as N

LEAKY = X.LEAKY
TWO24 = 2.0 ** 24

HEAD_PAIRS = [('HandSegNet', 'conv6_1', 'conv6_2'), ('PoseNet2D', 'conv5_1', 'conv5_2'), ('PoseNet2D', 'conv6_6', 'conv6_7'),
              ('PoseNet2D', 'conv7_6', 'conv7_7')]
# (scope, name, k, cin, cout, stride) of the two trunks, in order (nets.handsegnet / nets.posenet2d)
SEG_LAYERS = [('HandSegNet', 'conv%d_%d' % (b, i + 1), 3, ci if i == 0 else c, c, 1)
              for b, (n, ci, c) in enumerate([(2, 3, 64), (2, 64, 128), (4, 128, 256), (4, 256, 512)], 1) for i in range(n)] + \
             [('HandSegNet', 'conv5_1', 3, 512, 512, 1), ('HandSegNet', 'conv5_2', 3, 512, 128, 1), ('HandSegNet', 'conv6_1', 1, 128, 512, 1),
              ('HandSegNet', 'conv6_2', 1, 512, 2, 1)]
POSE_LAYERS = [('PoseNet2D', 'conv%d_%d' % (b, i + 1), 3, ci if i == 0 else c, c, 1)
               for b, (n, ci, c) in enumerate([(2, 3, 64), (2, 64, 128), (4, 128, 256), (2, 256, 512)], 1) for i in range(n)] + \
              [('PoseNet2D', n, 3, ci, co, 1) for n, ci, co in (('conv4_3', 512, 256), ('conv4_4', 256, 256), ('conv4_5', 256, 256),
                                                                ('conv4_6', 256, 256), ('conv4_7', 256, 128))] + \
              [('PoseNet2D', 'conv5_1', 1, 128, 512, 1), ('PoseNet2D', 'conv5_2', 1, 512, 21, 1)] + \
              [('PoseNet2D', 'conv%d_%d' % (p, r), 7 if r < 6 else 1, 149 if r == 1 else 128, 128 if r < 7 else 21, 1) for p in (6, 7) for r in range(1, 8)]
PRIOR_CONVS = [('PosePrior', 'conv_pose_%d_%d' % (i, j), 3, ci if j == 1 else c, c, j) for i, (ci, c) in enumerate([(21, 32), (32, 64), (64, 128)])
               for j in (1, 2)]
VP_CONVS = [('ViewpointNet', 'conv_vp_%d_%d' % (i, j), 3, ci if j == 1 else c, c, j) for i, (ci, c) in enumerate([(21, 64), (64, 128), (128, 256)])
            for j in (1, 2)]


def slope_identity_holds(slope=LEAKY, mmax=int(TWO24) // 100):
    """fl32(slope * fl32(-100 m)) == -m for every integer 0 <= m <= mmax, in float32 as the kernels and tf_ops.leaky_relu form it."""
    m = np.arange(mmax + 1, dtype=np.float64)
    v = (-100.0 * m).astype(np.float32)
    return bool(np.array_equal((np.float32(slope) * v).astype(np.float64), -m))


# --------------------------------------------------------------------------- sparse integer layers
def _cover(rng, n_in, n_slots):
    """n_slots indices into range(n_in), every index at least once where n_slots >= n_in."""
    idx = np.concatenate([rng.permutation(n_in) for _ in range(-(-n_slots // n_in))])[:n_slots]
    return rng.permutation(idx)


def selection_conv(rng, k, cin, cout, lo=0, centre=0.75):
    """One tap equal to 1 per output channel (the centre tap with probability `centre`, else one of the 3x3 taps round it), on an
    input channel >= lo; every such channel is read where cout allows."""
    w = np.zeros((k, k, cin, cout), np.float32)
    ci = lo + _cover(rng, cin - lo, cout)
    for o in range(cout):
        ty, tx = (k // 2, k // 2) if (k == 1 or rng.random() < centre) else k // 2 + rng.integers(-1, 2, 2)
        w[ty, tx, ci[o], o] = 1
    return w


def sparse_conv(rng, k, cin, cout, fan, scale=1):
    """`fan` taps scale {-1, 1} per output channel ((cin, tap) drawn so that every input channel is read where cout * fan >= cin)."""
    w = np.zeros((k, k, cin, cout), np.float32)
    ci = _cover(rng, cin, cout * fan).reshape(cout, fan)
    for o in range(cout):
        for j in range(fan):
            ty, tx = rng.integers(0, k, 2)
            w[ty, tx, ci[o, j], o] = scale * rng.choice([-1, 1])
    return w


def sparse_fc(rng, cin, cout, fan, scale=1):
    """At least `fan` entries scale {-1, 1} per output, as many as it takes for every input to be read."""
    fan = max(fan, -(-cin // cout))
    w = np.zeros((cin, cout), np.float32)
    ci = _cover(rng, cin, cout * fan).reshape(cout, fan)
    for o in range(cout):
        w[ci[o], o] = scale * rng.choice([-1, 1], fan)
    return w


def probe(w, b):
    """Output 0 of a linear layer (w [..., cin, cout], b) behind a 'neg' layer becomes the LAST hidden channel alone, weight 1, bias 0.
    That channel is always negative, so the output is fl32(0.01f * (-100 m)) itself: the one place where a slope that is one ulp off
    shows (anywhere else the 1e-7 m it adds to an integer vanishes in the next float32 sum of larger terms).  Hidden channels that
    only output 0 read get a weight into another output."""
    w2 = w.reshape(-1, w.shape[-2], w.shape[-1])
    w2[:, :, 0] = 0
    w2[0, -1, 0] = 1
    b[0] = 0
    dead = np.flatnonzero(~np.any(w2 != 0, axis=(0, 2)))
    w2[0, dead, 1 + np.arange(dead.size) % (w.shape[-1] - 1)] = 1
    return w, b


# --------------------------------------------------------------------------- head pairs
def head_weights(seed=0):
    """The weight dict of HandSegNet + PoseNet2D described in the module docstring."""
    rng = np.random.default_rng(seed)
    hidden = {(s, a) for s, a, _ in HEAD_PAIRS}
    linear = {(s, b) for s, _, b in HEAD_PAIRS}
    w = {}
    for scope, name, k, cin, cout, _ in SEG_LAYERS + POSE_LAYERS:
        base = '%s/%s/' % (scope, name)
        if (scope, name) in hidden:
            fan = int(rng.integers(3, 9))
            w[base + 'weights'] = sparse_conv(rng, 1, cin, cout, fan, 100)
            w[base + 'biases'] = (100 * rng.integers(-2, 3, cout)).astype(np.float32)
            w[base + 'biases'][cout - cout // 8:] = -(300 * fan + 100)        # always negative on inputs 0 .. 3 (probe())
        elif (scope, name) in linear:
            w[base + 'weights'], w[base + 'biases'] = probe(sparse_conv(rng, 1, cin, cout, max(3, -(-cin // cout))),
                                                            rng.integers(-5, 6, cout).astype(np.float32))
        else:
            # off-centre taps at full and half resolution only: on a 2x2 map a shifted channel is mostly padding
            w[base + 'weights'] = selection_conv(rng, k, cin, cout, lo=21 if cin == 149 else 0, centre=0.5 if name[:5] in ('conv1', 'conv2') else 1.0)
            w[base + 'biases'] = np.zeros(cout, np.float32)
    return w


def head_image(seed, B, H, W):
    """Values 0 .. 3, constant over 8x8 blocks (three 2x2 max-pools of independent pixels would leave hardly anything but 3)."""
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 4, (B, -(-H // 8), -(-W // 8), 3)), np.ones((1, 8, 8, 1)))[:, :H, :W].astype(np.float32)


def head_reference(w, image, net):
    """(oracle outputs, taps, taps of the |w|, |b|, |x| pass) of net = 'HandSegNet' (the small score map) or 'PoseNet2D' (three maps)."""
    taps, bound = {}, {}
    wa = {k: np.abs(v) for k, v in w.items()}
    if net == 'HandSegNet':
        out = [N.handsegnet(w, image, acc=np.float64, taps=taps)[0]]
        N.handsegnet(wa, np.abs(image), acc=np.float64, taps=bound)
    else:
        out = N.posenet2d(w, image, acc=np.float64, taps=taps)
        N.posenet2d(wa, np.abs(image), acc=np.float64, taps=bound)
    return out, taps, bound


def head_layers(net):
    """[(hidden tap, linear tap, input tap)] of the pairs of `net`."""
    inp = {'conv6_1': 'conv5_2', 'conv5_1': 'conv4_7', 'conv6_6': 'conv6_5', 'conv7_6': 'conv7_5'}
    return [('%s/%s' % (s, a), '%s/%s' % (s, b), '%s/%s' % (s, inp[a])) for s, a, b in HEAD_PAIRS if s == net]


# --------------------------------------------------------------------------- preconditions
def _distinct(a, what):
    """Every channel (last axis) of `a` takes at least two values."""
    a = np.asarray(a).reshape(-1, np.shape(a)[-1])
    flat = np.flatnonzero(a.min(axis=0) == a.max(axis=0))
    assert flat.size == 0, "precondition: %s: %d of %d channels are constant over the data set (first %s)" % (what, flat.size, a.shape[1], flat[:5])


def _outgoing(w, what):
    """Every input channel of the weight array (axis -2) has a non-zero weight."""
    dead = np.flatnonzero(~np.any(np.asarray(w).reshape(-1, w.shape[-2], w.shape[-1]) != 0, axis=(0, 2)))
    assert dead.size == 0, "precondition: %s: %d input channels have no outgoing weight (first %s)" % (what, dead.size, dead[:5])


def check(taps, bound, neg=(), under_test=()):
    """The preconditions of an exact chain on the oracle's taps (module docstring).  neg: taps that must have a quarter of their values on
    either side of zero; under_test: (what, input activation, weight array) triples.  Raises AssertionError naming what failed."""
    for k, v in taps.items():
        if k == 'hand_mask':
            continue
        assert np.array_equal(v, np.rint(v)), "precondition: tap %s is not integer (%d values): a negative value that is no multiple " \
            "of 100 met a leaky-ReLU" % (k, int(np.count_nonzero(v != np.rint(v))))
    for k, v in bound.items():
        assert float(np.max(v)) < TWO24, "precondition: |w| |x| bound of %s is %.3g >= 2^24" % (k, float(np.max(v)))
    for k in neg:
        v = taps[k]
        lo, hi = float(np.mean(v < 0)), float(np.mean(v > 0))
        assert lo >= 0.25 and hi >= 0.25, "precondition: %s has %.0f %% negative and %.0f %% positive values" % (k, 100 * lo, 100 * hi)
    for what, x, w in under_test:
        if x is not None:
            _distinct(x, what + ' input')
        _outgoing(w, what)


def check_heads(w, taps, bound, net):
    """check() for the pairs of `net`: the hidden layers are the 'neg' layers; both layers of every pair are under test."""
    neg, ut = [], []
    for hid, lin, inp in head_layers(net):
        neg.append(hid)
        ut += [(hid, taps[inp], w[hid + '/weights']), (lin, taps[hid], w[lin + '/weights'])]
    check(taps, bound, neg, ut)
    return {hid: float(np.mean(taps[hid] < 0)) for hid in neg}


# --------------------------------------------------------------------------- lifting stage
def lift_pool(seed, n, vmax=3, density=0.5):
    """n score maps [n,32,32,21] with integer values 0 .. vmax (a fraction `density` non-zero) and hand sides [n,2], both sides present."""
    rng = np.random.default_rng(seed)
    sm = (rng.integers(1, vmax + 1, (n, 32, 32, 21)) * (rng.random((n, 32, 32, 21)) < density)).astype(np.float32)
    hs = np.zeros((n, 2), np.float32)
    side = rng.integers(0, 2, n)
    if n > 1:
        side[:2] = [0, 1]
    hs[np.arange(n), side] = 1
    return sm, hs


def _fit_bias(pre, mode, rng):
    """The bias of a layer from its bias-free pre-activations on the pool (channels last): 'pos' lifts every channel to >= 0, 'neg' puts
    a multiple of 100 near the channel's median at zero, 'lin' (no activation behind it) is free."""
    p = pre.reshape(-1, pre.shape[-1])
    if mode == 'pos':
        return np.maximum(-p.min(axis=0), 0).astype(np.float32)
    if mode == 'neg':
        b = -100 * np.rint(np.median(p, axis=0) / 100)
        k = p.shape[1] - p.shape[1] // 8                # the last eighth of the channels: always negative (probe())
        b[k:] = -100 * (np.ceil(p.max(axis=0)[k:] / 100) + 1)
        return b.astype(np.float32)
    return rng.integers(-5, 6, p.shape[1]).astype(np.float32)


def _act(v):
    v32 = v.astype(np.float32)              # (a set that breaks the rule is built all the same: check() is what rejects it)
    return np.maximum(v32, LEAKY * v32).astype(np.float64)


def lift_weights(seed, sm, hs, spec=None, bottleneck=False, small_u=False):
    """PosePrior + ViewpointNet weights fitted to the pool (sm, hs).  spec: {layer name: (mode, fan-in)}, modes 'sel' (one tap equal to 1,
    bias 0), 'pos' ({-1, 1} taps, bias lifts the layer to >= 0), 'neg' (100 {-1, 1} taps, bias 100 n near the median; the layer behind
    it must be 'pos'); default ('sel', 1) for a convolution (a layer that does not grow the numbers), ('pos', 3) for an FC layer.  The first FC layer of a tower reads every one of its inputs (fan-in 4 / 16 at least) and
    both hand-side columns in every second output; fc_xyz / fc_vp_u* are linear.  small_u: fc_vp_u* are searched ({-1, 1} x 2 inputs
    + bias) so that u is an integer vector with 0 < |u|_inf <= 8 that differs between samples."""
    rng = np.random.default_rng(seed)
    spec = spec or {}
    w = {}
    sm = np.asarray(sm, np.float64)
    for scope, convs, fcs in (('PosePrior', PRIOR_CONVS, [('fc_rel0', 512), ('fc_rel1', 512)]),
                              ('ViewpointNet', VP_CONVS, [('fc_vp0', 256), ('fc_vp1', 128)])):
        x = sm
        for _, name, k, cin, cout, stride in convs:
            mode, fan = spec.get(name, ('sel', 1))
            if mode == 'sel':
                wt, b = selection_conv(rng, k, cin, cout, centre=0.5), np.zeros(cout, np.float32)
            else:
                wt = sparse_conv(rng, k, cin, cout, fan, 100 if mode == 'neg' else 1)
                b = _fit_bias(X.conv_ref_f64(x, wt, np.zeros(cout), stride, act=False), mode, rng)
            x = X.conv_ref_f64(x, wt, b, stride, act=True)
            w['%s/%s/weights' % (scope, name)], w['%s/%s/biases' % (scope, name)] = wt, b
        x = np.concatenate([x.reshape(x.shape[0], -1), np.asarray(hs, np.float64)], axis=1)
        for i, (name, cout) in enumerate(fcs):
            mode, fan = spec.get(name, ('pos', 3))
            scale = 100 if mode == 'neg' else 1
            wt = sparse_fc(rng, x.shape[1], cout, fan, scale)
            if i == 0:          # the hand side: both columns, unequal, in every second output
                sel = rng.random(cout) < 0.5
                wt[-2:, sel] = scale * np.array([[1], [-1]]) * rng.choice([-1, 1], int(sel.sum()))
            b = _fit_bias(x @ wt.astype(np.float64), mode, rng)
            x = _act(x @ wt.astype(np.float64) + b)
            w['%s/%s/weights' % (scope, name)], w['%s/%s/biases' % (scope, name)] = wt, b
        if scope == 'PosePrior':
            if bottleneck:
                wt = sparse_fc(rng, 512, 30, 3)
                b = _fit_bias(x @ wt, 'lin', rng)
                w['PosePrior/fc_bottleneck/weights'], w['PosePrior/fc_bottleneck/biases'] = wt, b
                w['PosePrior/fc_xyz/weights'], w['PosePrior/fc_xyz/biases'] = sparse_fc(rng, 30, 63, 3), rng.integers(-5, 6, 63).astype(np.float32)
            else:
                wt, b = sparse_fc(rng, 512, 63, 3), rng.integers(-5, 6, 63).astype(np.float32)
                if spec.get('fc_rel1', ('pos',))[0] == 'neg':
                    wt, b = probe(wt, b)
                w['PosePrior/fc_xyz/weights'], w['PosePrior/fc_xyz/biases'] = wt, b
        else:
            for a in ('ux', 'uy', 'uz'):
                wt, b = sparse_fc(rng, 128, 1, 3), rng.integers(-5, 6, 1).astype(np.float32)
                if small_u:
                    for _ in range(4000):
                        i, j = rng.choice(128, 2, replace=False)
                        d = x[:, i] - x[:, j]
                        if d.max() - d.min() <= 14 and d.max() > d.min():
                            break
                    else:
                        raise AssertionError("small-u search failed")
                    wt = np.zeros((128, 1), np.float32)
                    wt[i], wt[j] = 1, -1
                    b = np.array([-np.rint((d.max() + d.min()) / 2)], np.float32)
                w['ViewpointNet/fc_vp_%s/weights' % a], w['ViewpointNet/fc_vp_%s/biases' % a] = wt, b
    return w


def lift_layers(w, taps, sm, hs, bottleneck=False, towers=('PosePrior', 'ViewpointNet'), skip=()):
    """The (what, input activation, weights) triples of every layer of the towers but `skip`, for check(under_test=...)."""
    out = []
    for scope, convs, fcs in (('PosePrior', PRIOR_CONVS, ['fc_rel0', 'fc_rel1', 'fc_xyz']), ('ViewpointNet', VP_CONVS, ['fc_vp0', 'fc_vp1', 'fc_vp_ux'])):
        if scope not in towers:
            continue
        x = np.asarray(sm)
        for _, name, *_r in convs:
            out.append((name, x, w['%s/%s/weights' % (scope, name)]))
            x = taps['%s/%s' % (scope, name)]
        c = x.shape[-1]
        w0 = w['%s/%s/weights' % (scope, fcs[0])]
        # the first FC layer: every map channel varies, every ROW (position x channel, hand side) is read, both hand sides occur
        out += [(fcs[0] + ' maps', x, w0[:-2].reshape(16, c, -1)), (fcs[0] + ' rows', None, w0), (fcs[0] + ' hand side', hs, w0[-2:])]
        x = taps['%s/%s/relu' % (scope, fcs[0])]
        for name in fcs[1:]:
            if scope == 'ViewpointNet' and name == 'fc_vp_ux':
                wt = np.concatenate([w['ViewpointNet/fc_vp_u%s/weights' % a] for a in 'xyz'], axis=1)
            elif name == 'fc_xyz' and bottleneck:
                out.append(('fc_bottleneck', x, w['PosePrior/fc_bottleneck/weights']))
                continue                      # (fc_xyz's 30 inputs are the bottleneck's outputs: linear, covered by the oracle equality)
            else:
                wt = w['%s/%s/weights' % (scope, name)]
            out.append((name, x, wt))
            if name in ('fc_rel1', 'fc_vp1'):
                x = taps['%s/%s/relu' % (scope, name)]
    return [t for t in out if t[0] not in skip]


def lift_reference(w, sm, hs, bottleneck=False, rot=True):
    """(rel, can, R, u [n,3] or None, taps, bound taps) of the float64 oracle on the pool."""
    taps, bound = {}, {}
    wa = {k: np.abs(v) for k, v in w.items()}
    if rot:
        rel, can, R = N.pose3d(w, sm, hs, acc=np.float64, taps=taps)
        N.pose3d(wa, np.abs(sm), hs, acc=np.float64, taps=bound)
        u = np.concatenate([taps['ViewpointNet/fc_vp_u%s' % a] for a in 'xyz'], axis=1).astype(np.float64)
    else:
        can = N.poseprior_can(w, sm, hs, acc=np.float64, taps=taps, bottleneck=bottleneck)
        N.poseprior_can(wa, np.abs(sm), hs, acc=np.float64, taps=bound, bottleneck=bottleneck)
        rel, R, u = can, None, None
    return rel, can, R, u, taps, bound


def rodrigues64(u):
    """The rotation matrix of nets.get_rot_mat in float64: u [n,3] -> [n,3,3]."""
    u = np.asarray(u, np.float64)
    th = np.sqrt((u * u).sum(axis=1) + 1e-8)
    a = u / th[:, None]
    K = np.zeros((u.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    st, ct = np.sin(th)[:, None, None], np.cos(th)[:, None, None]
    return ct * np.eye(3) + st * K + (1 - ct) * a[:, :, None] * a[:, None, :]


def rot_sensitivity(u):
    """min over samples, axes i and signs of max |R(u +- e_i) - R(u)|."""
    r0 = rodrigues64(u)
    return min(float(np.abs(rodrigues64(u + s * np.eye(3)[i]) - r0).max(axis=(1, 2)).min()) for i in range(3) for s in (-1, 1))


# The lifting data sets: name -> (spec of lift_weights, layers that exercise the negative branch, lift_pool's (vmax, density), small_u).
# Fan-ins 3 .. 8 (16 at fc_vp0, whose 4098 inputs each need a weight); convolutions not named are selections, so that the |w| |x|
# bound stays below 2^24 behind a layer with the factor 100.
_P3 = ('pos', 3)
LIFT_SETS = {
    'nonneg': ({'conv_pose_0_1': _P3, 'conv_pose_1_2': ('pos', 4), 'conv_pose_2_2': ('pos', 8), 'conv_vp_0_2': _P3, 'conv_vp_1_1': ('pos', 5),
                'conv_vp_2_2': ('pos', 8)}, (), (3, 0.5), False),
    'negconv': ({'conv_pose_1_2': ('neg', 5), 'conv_pose_2_1': _P3, 'conv_vp_0_1': ('neg', 4), 'conv_vp_0_2': _P3},
                ('PosePrior/conv_pose_1_2', 'ViewpointNet/conv_vp_0_1'), (3, 0.5), False),
    'negfc0': ({'conv_pose_2_1': _P3, 'conv_vp_2_1': _P3, 'fc_rel0': ('neg', 4), 'fc_vp0': ('neg', 16)},
               ('PosePrior/fc_rel0', 'ViewpointNet/fc_vp0'), (3, 0.5), False),
    'negfc1': ({'conv_pose_0_2': _P3, 'conv_vp_1_2': _P3, 'fc_rel1': ('neg', 6), 'fc_vp1': ('neg', 8)},
               ('PosePrior/fc_rel1', 'ViewpointNet/fc_vp1'), (3, 0.5), False),
    'small_u': ({'conv_pose_1_1': _P3, 'fc_vp0': ('pos', 16)}, (), (1, 0.3), True),
}


def lift_set(name, n, seed=0, bottleneck=False):
    """(weights, sm, hs, neg layers) of the data set `name` with a pool of n samples."""
    spec, neg, (vmax, density), small_u = LIFT_SETS[name]
    sm, hs = lift_pool(seed + 1, n, vmax, density)
    return lift_weights(seed + 2, sm, hs, spec, bottleneck, small_u), sm, hs, neg
