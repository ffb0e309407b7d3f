"""Every float32 kernel hp3d_conv2d reaches, held to a float64 reference at the trunks' full size (oracle/conv_exact.py).

* Exact runs: small-integer inputs, filters that are multiples of the denominator of G (x) G, integer biases.  Every value every
  kernel forms is then an integer below 2^24 (the precondition is asserted per case), so the result must equal the float64
  reference BIT FOR BIT, whatever the tiling, channel split, tail pieces or summation order.  The float64 reference runs on the
  CPU in torch, so the bench's B = 32 layers are checked against it, not against another GPU kernel.
* Power-of-two equivariance on random-normal data: conv(2^a x, 2^c w, 2^(a+c) b) = 2^(a+c) conv(x, w, b) exactly.
* Normalised error on what a trunk layer is fed (leaky-ReLU outputs with a mean offset and unequal channel scales, with and without
  70 % zeros): rho = max |y - r| / (u abs_bound) <= RHO_LAMBDA sqrt(n), n the accumulation chain (the gate and why: conv_exact.py).
Each case asserts that its kernel's launch counter moved and that no other conv kernel ran: an option that silently falls back fails.

F(4x4,4x4) (conv_wino7.hip) cannot be exact: its filter transform has denominators 3^4 5^2 and its transforms 2^-8, so one non-zero
tap on one input pixel already needs 31 x 2^24 (oracle/conv_exact.py, tests/test_conv_exact.py).  It is covered by the equivariance
and rho checks only.
"""
import time

import numpy as np
import pytest

from oracle import conv_exact as X
from tests.test_gpu_parity import CONV_CASES, W2_CASES, W4_CASES, W4S_CASES, WINO_CASES

pytestmark = pytest.mark.gpu

DEFAULTS = {'conv_impl': 'mfma', 'wino2': 'auto', 'wino4': 'auto', 'wino4_split': '0', 'wino4_tail': '1', 'wino_splitk': '1',
            'wino7': 'auto', 'wino7_ksplit': 'auto', 'first_walk': 'balanced'}
KERNEL_COUNTERS = ['conv_mfma_launches', 'conv_first_launches', 'conv_wino_launches', 'conv_wino2_launches', 'conv_wino4_launches',
                   'conv_wino4s_launches', 'conv_wino7_launches']
PATH_COUNTERS = ['conv_splitk_reduce_launches', 'conv_wino4_tail_launches', 'conv_wino4s_tail_launches', 'conv_wino7_split_launches']
# form -> (options, the kernel's launch counter (None: conv_impl=naive, which has none), exactness kind)
FORMS = {
    'direct': ({'conv_impl': 'direct'}, 'conv_mfma_launches', 'direct'),
    'naive': ({'conv_impl': 'naive'}, None, 'direct'),
    'first': ({}, 'conv_first_launches', 'direct'),
    'first_rows': ({'first_walk': 'rows'}, 'conv_first_launches', 'direct'),
    'wino': ({'conv_impl': 'winograd'}, 'conv_wino_launches', 'wino2'),
    'wino_nosplit': ({'conv_impl': 'winograd', 'wino_splitk': '0'}, 'conv_wino_launches', 'wino2'),
    'wino2': ({'wino2': '1'}, 'conv_wino2_launches', 'wino2'),
    'wino2_nosplit': ({'wino2': '1', 'wino_splitk': '0'}, 'conv_wino2_launches', 'wino2'),
    'wino4': ({'wino4': '1'}, 'conv_wino4_launches', 'wino4'),
    'wino4_nosplit': ({'wino4': '1', 'wino_splitk': '0'}, 'conv_wino4_launches', 'wino4'),
    'wino4_notail': ({'wino4': '1', 'wino_splitk': '0', 'wino4_tail': '0'}, 'conv_wino4_launches', 'wino4'),
    'wino4s': ({'wino4_split': '1'}, 'conv_wino4s_launches', 'wino4s'),
    'wino4s_notail': ({'wino4_split': '1', 'wino4_tail': '0'}, 'conv_wino4s_launches', 'wino4s'),
    'wino7': ({'wino7': '1', 'wino_splitk': '0'}, 'conv_wino7_launches', 'wino7'),
    'wino7_ks2': ({'wino7': '1', 'wino7_ksplit': '2'}, 'conv_wino7_launches', 'wino7'),
    'wino7_ks5': ({'wino7': '1', 'wino7_ksplit': '5'}, 'conv_wino7_launches', 'wino7'),
}


def run(e, form, x, w, b, stride=1, act=True, pool=False, calls=2):
    """`calls` runs of one layer on `form`; asserts the counters (its kernel ran every time, no other conv kernel ran) and that the
    runs are bit-identical.  Returns (output, {path counter: increase})."""
    opts, counter, _ = FORMS[form]
    c0 = {c: e.counter(c) for c in KERNEL_COUNTERS + PATH_COUNTERS}
    for k, v in opts.items():
        e.set_option(k, v)
    try:
        ys = [e.conv2d(x, w, b, stride, act, pool) for _ in range(calls)]
    finally:
        for k in opts:
            e.set_option(k, DEFAULTS[k])
    d = {c: e.counter(c) - c0[c] for c in KERNEL_COUNTERS + PATH_COUNTERS}
    for c in KERNEL_COUNTERS:
        assert d[c] == (calls if c == counter else 0), (form, d)
    for y in ys[1:]:
        assert np.array_equal(ys[0], y), "%s: two calls differ" % form
    return ys[0], d


def exact_case(e, form, shape, stride=1, pool=False, act=True, seed=0, old_gate=None):
    """An exact run of `form` on shape (B, H, W, Cin, Cout, k): precondition, then bit-equality with the float64 reference."""
    kind = FORMS[form][2]
    rng = np.random.default_rng(seed + sum(shape))
    t0 = time.time()
    x, w, b, bound = X.exact_data(kind, shape, rng, stride=stride)
    assert X.exact_ok(kind, bound, x, w), "precondition: abs_bound %.3g" % bound.max()
    r = X.conv_ref_f64(x, w, b, stride, act, pool)
    t1 = time.time()
    y, d = run(e, form, x, w, b, stride, act, pool)
    assert y.shape == r.shape
    nbad = X.exact_mismatch(y, r)
    assert nbad == 0, "%s %s: %d of %d outputs differ, max %.3g (|r| max %.3g)" % (form, shape, nbad, r.size, np.abs(y - r).max(), np.abs(r).max())
    msg = "exact %-14s %-28s bound/2^24 %.3f  ref %.1f s  path %s" % (
        form, shape, bound.max() * 2.0 ** X.grid_log2(kind) / 2 ** 24, t1 - t0, {c: v for c, v in d.items() if v and c in PATH_COUNTERS})
    if old_gate is not None:          # how far inside the old fixed gates on unit-normal data the kernel sits
        B, H, W, Cin, Cout, k = shape
        x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
        w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
        b = rng.standard_normal(Cout).astype(np.float32)
        y, _ = run(e, form, x, w, b, stride, act, pool, calls=1)
        msg += "  unit-normal max|err| %.2e (old gate %.0e)" % (np.abs(y - X.conv_ref_f64(x, w, b, stride, act, pool)).max(), old_gate)
    print(msg)
    return d


# ---------------------------------------------------------------------------------------------------------- the existing shapes, exact
def _conv_id(c):
    return "B%d_%dx%d_%d-%d_k%ds%dp%d" % c


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_direct_exact(gpu_engine, case):
    """conv_mfma.hip (conv_impl = direct) on the layer geometries: k = 1, 3, 7, stride 2, Cout 2 / 21, Cin 3 ... 512."""
    B, H, W, Cin, Cout, k, stride, pool = case
    exact_case(gpu_engine, 'direct', (B, H, W, Cin, Cout, k), stride, bool(pool), act=Cout not in (2, 21))


@pytest.mark.parametrize("case", [c for c in CONV_CASES if not c[7] and c[0] * c[1] * c[2] * c[4] <= 2e5] +
                         [(1, 17, 23, 3, 21, 7, 1, 0), (2, 9, 9, 149, 2, 7, 2, 0)], ids=_conv_id)
def test_naive_exact(gpu_engine, case):
    """The one-thread-per-output debug kernel (conv_impl = naive; it has no fused pool and no counter: no other conv kernel may run)."""
    B, H, W, Cin, Cout, k, stride, pool = case
    exact_case(gpu_engine, 'naive', (B, H, W, Cin, Cout, k), stride, False)


@pytest.mark.parametrize("case", [(32, 320, 320), (32, 256, 256), (3, 240, 320), (1, 37, 53), (5, 200, 264)], ids=lambda c: "B%d_%dx%d" % c)
@pytest.mark.parametrize("form", ['first', 'first_rows'])
def test_first_layer_exact(gpu_engine, case, form):
    """conv_first.hip (conv1_1, 3 -> 64) in both walks, at the bench's B = 32 crops, C1's frame and ragged sizes."""
    B, H, W = case
    exact_case(gpu_engine, form, (B, H, W, 3, 64, 3))


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "B%d_%dx%d_%d-%d_p%d" % c)
@pytest.mark.parametrize("form", ['wino', 'wino_nosplit'])
def test_wino_f2x2_exact(gpu_engine, case, form):
    """conv_wino.hip (conv_impl = winograd), with and without the whole-launch channel split (then conv_splitk_reduce)."""
    B, H, W, Cin, Cout, pool = case
    d = exact_case(gpu_engine, form, (B, H, W, Cin, Cout, 3), pool=bool(pool))
    if form == 'wino_nosplit':
        assert d['conv_splitk_reduce_launches'] == 0


@pytest.mark.parametrize("case", W2_CASES + [(1, 32, 32, 160, 128, 0, 7), (4, 32, 32, 128, 128, 0, 7), (32, 32, 32, 128, 128, 0, 7)],
                         ids=lambda c: "B%d_%dx%d_%d-%d_p%d" % c[:6] + ("_k%d" % c[6] if len(c) > 6 else ""))
def test_wino2_exact(gpu_engine, case):
    """conv_wino2.hip (wino2 = 1) on the conv_wino.hip shapes, the batch-1 PoseNet2D shapes, B = 32 160x160 and the 7x7 nine-block form."""
    B, H, W, Cin, Cout, pool = case[:6]
    k = case[6] if len(case) > 6 else 3
    exact_case(gpu_engine, 'wino2', (B, H, W, Cin, Cout, k), pool=bool(pool))


@pytest.mark.parametrize("case", W4_CASES, ids=lambda c: "B%d_%dx%d_%d-%d_p%d_k%d" % c)
@pytest.mark.parametrize("form", ['wino4', 'wino4_nosplit'])
def test_wino4_exact(gpu_engine, case, form):
    """conv_wino4.hip (wino4 = 1), k = 3 and the 7x7 nine-block form, with and without the whole-launch channel split."""
    B, H, W, Cin, Cout, pool, k = case
    exact_case(gpu_engine, form, (B, H, W, Cin, Cout, k), pool=bool(pool))


TAIL_CASES = [(10, 64, 64, 256, 256, 0), (32, 40, 40, 512, 512, 0), (32, 80, 80, 256, 256, 1), (5, 126, 158, 128, 128, 0), (3, 40, 40, 512, 128, 0)]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "B%d_%dx%d_%d-%d_p%d" % c)
@pytest.mark.parametrize("form", ['wino4_nosplit', 'wino4_notail'])
def test_wino4_tail_pieces_exact(gpu_engine, case, form):
    """conv_wino4.hip's tail pieces (wino4_tail = 1: an under-filled last round as channel slices + wino4_tail_reduce) and the same
    launch without them, at the bench's B = 32 40x40 / 80x80 layers."""
    B, H, W, Cin, Cout, pool = case
    d = exact_case(gpu_engine, form, (B, H, W, Cin, Cout, 3), pool=bool(pool))
    assert d['conv_wino4_tail_launches'] == (2 if form == 'wino4_nosplit' else 0), d


@pytest.mark.parametrize("case", W4S_CASES, ids=lambda c: "B%d_%dx%d_%d-%d_p%d" % c)
def test_wino4s_exact(gpu_engine, case):
    """conv_wino4s.hip (wino4_split = 1): every transformed operand below 2^16, so its two bfloat16 pieces hold it and the six
    piece products are the exact product."""
    B, H, W, Cin, Cout, pool = case
    exact_case(gpu_engine, 'wino4s', (B, H, W, Cin, Cout, 3), pool=bool(pool))


@pytest.mark.parametrize("case", TAIL_CASES[:3], ids=lambda c: "B%d_%dx%d_%d-%d_p%d" % c)
@pytest.mark.parametrize("form", ['wino4s', 'wino4s_notail'])
def test_wino4s_tail_pieces_exact(gpu_engine, case, form):
    B, H, W, Cin, Cout, pool = case
    d = exact_case(gpu_engine, form, (B, H, W, Cin, Cout, 3), pool=bool(pool))
    assert d['conv_wino4s_tail_launches'] == (2 if form == 'wino4s' else 0), d


def test_fc_exact(gpu_engine):
    """hp3d_fc on integer data: bit-equal to the float64 reference (the lifting towers' shapes, with and without activation)."""
    rng = np.random.default_rng(5)
    for B, Cin, Cout, act in [(1, 2050, 512, True), (32, 4098, 256, True), (5, 512, 63, False), (3, 128, 3, False), (32, 32768, 512, True)]:
        x = rng.integers(-3, 4, (B, Cin)).astype(np.float32)
        w = rng.integers(-3, 4, (Cin, Cout)).astype(np.float32)
        b = rng.integers(-50, 51, Cout).astype(np.float32)
        y = gpu_engine.fc(x, w, b, act)
        assert (np.abs(x).astype(np.float64) @ np.abs(w) + np.abs(b) < 2 ** 24).all()
        r = X.fc_ref_f64(x, w, b, act)
        assert np.array_equal(y.astype(np.float64), r), (B, Cin, Cout, int((y != r).sum()))
        assert np.array_equal(y, gpu_engine.fc(x, w, b, act))


# ---------------------------------------------------------------------------------------------------------- production layers, exact
# (B, H, W, Cin, Cout, k, pool): HandSegNet at 320x320 and C1's 240x320, PoseNet2D at 256x256 (its 32x32 7x7 units), B = 32 (16 where
# a layer's output passes 50 M values: the host side holds it in float64 three times)
PROD = {
    'hs320_conv2_1': (16, 160, 160, 64, 128, 3, 0), 'hs320_conv2_2': (16, 160, 160, 128, 128, 3, 1), 'hs320_conv3_2': (32, 80, 80, 256, 256, 3, 0),
    'hs320_conv3_4': (32, 80, 80, 256, 256, 3, 1), 'hs320_conv4_2': (32, 40, 40, 512, 512, 3, 0), 'hs320_conv1_2': (16, 320, 320, 64, 64, 3, 1),
    'c1_conv3_1': (16, 60, 80, 128, 256, 3, 0), 'c1_conv4_1': (16, 30, 40, 256, 512, 3, 0),
    'pn256_conv2_1': (32, 128, 128, 64, 128, 3, 0), 'pn256_conv3_4': (32, 64, 64, 256, 256, 3, 1), 'pn256_conv4_2': (32, 32, 32, 512, 512, 3, 0),
    'pn256_conv6_1': (32, 32, 32, 149, 128, 7, 0), 'pn256_conv6_2': (32, 32, 32, 128, 128, 7, 0),
}
PROD_FORMS = {
    'direct': ['hs320_conv3_2', 'hs320_conv3_4', 'hs320_conv4_2', 'c1_conv4_1', 'pn256_conv6_1'],
    'wino': ['hs320_conv2_1', 'hs320_conv3_4', 'hs320_conv4_2', 'c1_conv3_1', 'pn256_conv4_2', 'pn256_conv6_2'],
    'wino2': ['hs320_conv1_2', 'hs320_conv2_2', 'c1_conv4_1', 'pn256_conv6_2'],
    'wino4': ['hs320_conv2_1', 'hs320_conv2_2', 'hs320_conv3_2', 'hs320_conv3_4', 'hs320_conv4_2', 'c1_conv3_1', 'c1_conv4_1', 'pn256_conv2_1',
              'pn256_conv3_4', 'pn256_conv4_2', 'pn256_conv6_1', 'pn256_conv6_2'],
    'wino4s': ['hs320_conv2_2', 'hs320_conv3_2', 'hs320_conv3_4', 'hs320_conv4_2', 'c1_conv4_1', 'pn256_conv3_4', 'pn256_conv4_2'],
}
OLD_GATE = {'direct': 5e-5, 'wino': 5e-5, 'wino2': 5e-5, 'wino4': 2e-4, 'wino4s': 2e-4}


@pytest.mark.parametrize("form,layer", [(f, l) for f, ls in PROD_FORMS.items() for l in ls])
def test_production_layers_exact(gpu_engine, form, layer):
    B, H, W, Cin, Cout, k, pool = PROD[layer]
    exact_case(gpu_engine, form, (B, H, W, Cin, Cout, k), pool=bool(pool), old_gate=OLD_GATE[form])


# ---------------------------------------------------------------------------------------------------------- equivariance
EQ_FORMS = {
    'direct': ['hs320_conv3_4', 'hs320_conv4_2', 'pn256_conv6_1'], 'first': [], 'wino': ['hs320_conv3_4', 'pn256_conv6_2'],
    'wino2': ['hs320_conv2_2', 'pn256_conv6_2'], 'wino4': ['hs320_conv3_4', 'hs320_conv4_2', 'pn256_conv6_1'],
    'wino4s': ['hs320_conv3_4', 'hs320_conv4_2'], 'wino7': ['pn256_conv6_1', 'pn256_conv6_2'],
    'wino7_ks2': [(2, 32, 32, 128, 128, 7, 0)], 'wino7_ks5': [(1, 32, 32, 160, 128, 7, 0)], 'naive': [(2, 30, 40, 96, 64, 3, 0)],
    'wino4_notail': [(32, 40, 40, 512, 512, 3, 0)],
}


@pytest.mark.parametrize("form,layer", [(f, l) for f, ls in EQ_FORMS.items() for l in ls] + [('first', (32, 320, 320, 3, 64, 3, 0))],
                         ids=lambda v: v if isinstance(v, str) else "B%d_%dx%d_%d-%d_k%d_p%d" % v)
def test_power_of_two_equivariance(gpu_engine, form, layer):
    """On random-normal data: x 2^a, w 2^c, b 2^(a+c) must give exactly 2^(a+c) times the output, for (a, c) = (+20, -7), (-24, +9)."""
    B, H, W, Cin, Cout, k, pool = PROD[layer] if isinstance(layer, str) else layer
    rng = np.random.default_rng(B + H + Cin + Cout + k)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    y, d = run(gpu_engine, form, x, w, b, 1, True, bool(pool), calls=1)
    if form.startswith('wino7_ks'):
        assert d['conv_wino7_split_launches'] == 1 and d['conv_splitk_reduce_launches'] == 1, d
    for a, c in [(20, -7), (-24, 9)]:
        ys, _ = run(gpu_engine, form, np.ldexp(x, a), np.ldexp(w, c), np.ldexp(b, a + c), 1, True, bool(pool), calls=1)
        assert np.array_equal(ys, np.ldexp(y, a + c)), (form, a, c, int((ys != np.ldexp(y, a + c)).sum()))


# ---------------------------------------------------------------------------------------------------------- normalised error
RHO_FORMS = {'wino': 'wino2', 'wino2': 'wino2', 'wino4': 'wino4', 'wino4s': 'wino4s', 'wino7': 'wino7', 'wino7_ks2': 'wino7'}
RHO_LAYERS = {'wino': ['hs320_conv3_4', 'c1_conv4_1'], 'wino2': ['hs320_conv2_2', 'pn256_conv6_2'],
              'wino4': ['hs320_conv2_1', 'hs320_conv4_2', 'pn256_conv6_1'], 'wino4s': ['hs320_conv3_4', 'pn256_conv4_2'],
              'wino7': ['pn256_conv6_1', 'pn256_conv6_2'], 'wino7_ks2': [(4, 32, 32, 128, 128, 7, 0)]}


@pytest.mark.parametrize("zeros", [0.0, 0.7])
@pytest.mark.parametrize("form,layer", [(f, l) for f, ls in RHO_LAYERS.items() for l in ls],
                         ids=lambda v: v if isinstance(v, str) else "B%d_%dx%d_%d-%d_k%d_p%d" % v)
def test_normalised_error_on_trunk_data(gpu_engine, form, layer, zeros):
    B, H, W, Cin, Cout, k, pool = PROD[layer] if isinstance(layer, str) else layer
    B = min(B, 8)                       # (rho is per output: the batch adds nothing the launch regimes above do not cover)
    rng = np.random.default_rng(B + H + Cin + Cout + k + int(10 * zeros))
    x = X.realistic_input((B, H, W, Cin), rng, zeros)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    y, _ = run(gpu_engine, form, x, w, b, 1, True, bool(pool), calls=1)
    kind = RHO_FORMS[form]
    bound = X.abs_bound(x, w, kind, b)
    r = X.conv_ref_f64(x, w, b, 1, True, bool(pool))
    rho = X.rho(y, r, X.pool_bound(bound) if pool else bound)
    print("rho %-10s %-16s zeros %.1f: %.3f  (n %d, gate %.2f)" % (form, layer, zeros, rho, X.n_chain(kind, Cin, k), X.rho_gate(kind, Cin, k)))
    assert rho <= X.rho_gate(kind, Cin, k)
