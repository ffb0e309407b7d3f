"""The checks of tests/test_gpu_conv_exact.py, checked (CPU): oracle/conv_exact.py's reference, bound and exact data against
tf_ops and a float32 NumPy restatement of every Winograd form; every kernel form on the CPU interpreter of the kernel sources
(tests/emu) at small shapes; and the tests of the tests -- perturbed copies of correct results, made in NumPy, must fail them."""
import numpy as np
import pytest

from oracle import conv_exact as X
from oracle import tf_ops as T
from tests import test_gpu_conv_exact as G

WINO_SHAPES = [('wino2', 3), ('wino4', 3), ('wino4', 7), ('wino2', 7), ('wino7', 7)]


# ---------------------------------------------------------------------------------------------------------- the helper itself
@pytest.mark.parametrize("case", [(2, 9, 11, 5, 7, 3, 1), (1, 8, 8, 4, 3, 3, 2), (1, 9, 7, 4, 3, 3, 2), (2, 10, 6, 3, 5, 7, 1), (1, 6, 5, 8, 2, 1, 1),
                                  (1, 15, 15, 4, 4, 3, 2), (1, 16, 10, 3, 4, 7, 2)])
def test_conv_ref_f64_equals_tf_ops(case):
    """conv_ref_f64 = tf_ops.conv2d_same(acc=float64) + bias, incl. stride 2 with asymmetric SAME pads (even sizes) and symmetric ones."""
    B, H, W, Cin, Cout, k, s = case
    rng = np.random.default_rng(sum(case))
    x, w, b = (rng.standard_normal(sh).astype(np.float32) for sh in ((B, H, W, Cin), (k, k, Cin, Cout), Cout))
    r = X.conv_ref_f64(x, w, b, s, act=False)
    t = T.conv2d_same(x, w, s, acc=np.float64)            # (rounded once to float32 at the end)
    assert r.shape == t.shape and (np.abs(r - b - t) <= 2.0 ** -24 * np.abs(t) + 1e-12).all()
    ra = X.conv_ref_f64(x, w, b, s, act=True, pool=True)
    assert np.array_equal(ra, T.max_pool_2x2(np.maximum(r, np.float64(X.LEAKY) * r)))


@pytest.mark.parametrize("kind,k", WINO_SHAPES)
def test_winograd_restatement_and_abs_bound(kind, k):
    """The restated transforms are Winograd's (float32 restatement = the float64 conv to rounding), and abs_bound bounds every
    partial sum the restatement forms (channel by channel in the transform domain, and the outputs) with every sign pattern."""
    rng = np.random.default_rng(k + len(kind))
    for x in [rng.standard_normal((2, 9, 11, 8)), np.abs(rng.standard_normal((2, 9, 11, 8)))]:
        x = x.astype(np.float32)
        w = rng.standard_normal((k, k, 8, 5)).astype(np.float32)
        b = rng.standard_normal(5).astype(np.float32)
        for ww in (w, np.abs(w)):
            tr = []
            y = X.wino_f32(x, ww, b, kind, act=False, track=tr)
            r = X.conv_ref_f64(x, ww, b, 1, act=False)
            bound = X.abs_bound(x, ww, kind, b)
            assert np.abs(y - r).max() < 1e-3 * np.abs(r).max()
            assert (tr[0] <= bound).all() and (np.abs(y) <= bound).all()
    # the direct bound is the absolute conv, attained by non-negative data
    xa, wa = np.abs(x), np.abs(w)
    assert np.allclose(X.abs_bound(xa, wa, 'direct', np.abs(b)), X.conv_ref_f64(xa, wa, np.abs(b), 1, act=False))


@pytest.mark.parametrize("kind,k", [('direct', 3), ('direct', 7), ('wino2', 3), ('wino2', 7), ('wino4', 3), ('wino4', 7), ('wino4s', 3)])
@pytest.mark.parametrize("shape", [(2, 13, 17, 32, 64), (1, 24, 20, 160, 64)])
def test_exact_data_meets_its_precondition(kind, k, shape):
    """exact_data meets exact_ok, and on it the float32 restatement (three bfloat16 pieces for wino4s) is bit-equal to the reference."""
    rng = np.random.default_rng(sum(shape) + k)
    x, w, b, bound = X.exact_data(kind, shape + (k,), rng)
    assert X.exact_ok(kind, bound, x, w)
    assert np.array_equal(x, np.round(x)) and np.array_equal(w / X.denominator(kind), np.round(w / X.denominator(kind)))
    assert (w != 0).sum() >= shape[4], "the filters are all but empty"
    r = X.conv_ref_f64(x, w, b, 1)
    if kind != 'direct':
        assert X.exact_mismatch(X.wino_f32(x, w, b, 'wino4' if kind == 'wino4s' else kind, pieces=3 if kind == 'wino4s' else None), r) == 0


def test_wino7_cannot_be_exact():
    """F(4x4,4x4): D = 180^2 and a 2^-8 grid -- one tap of one input pixel already exceeds 2^24 (so conv_wino7 is covered by
    equivariance and rho only)."""
    assert X.denominator('wino7') == 32400 and X.grid_log2('wino7') == 8
    x = np.zeros((1, 16, 16, 16), np.float32)
    x[0, 8, 8, 0] = 1
    for tap in [(0, 0), (3, 3), (6, 6), (2, 5)]:
        w = np.zeros((7, 7, 16, 64), np.float32)
        w[tap + (0, 0)] = X.denominator('wino7')
        assert not X.exact_ok('wino7', X.abs_bound(x, w, 'wino7'))


# ---------------------------------------------------------------------------------------------------------- the tests of the tests
def _exact_small(kind='wino4', shape=(1, 12, 16, 32, 64, 3), act=True):
    rng = np.random.default_rng(3)
    x, w, b, _ = X.exact_data(kind, shape, rng)
    return x, w, b, X.conv_ref_f64(x, w, b, 1, act)


def test_exact_check_sees_one_ulp():
    x, w, b, r = _exact_small()
    y = r.astype(np.float32)
    assert X.exact_mismatch(y, r) == 0
    i = np.unravel_index(np.argmax(np.abs(r)), r.shape)
    y[i] = np.nextafter(y[i], np.float32(np.inf))
    assert X.exact_mismatch(y, r) == 1


def test_exact_check_sees_a_halo_tap_dropped_at_a_tile_edge():
    """The tap (1, 2) of the outputs in the last column of each 4-wide tile (the tap that reads the next tile's column) left out."""
    x, w, b, r = _exact_small(act=False)
    wt = np.zeros_like(w)
    wt[1, 2] = w[1, 2]
    contrib = X.conv_ref_f64(x, wt, np.zeros_like(b), 1, act=False)
    edge = (np.arange(r.shape[2]) % 4 == 3)[None, None, :, None]
    bad = (r - contrib * edge).astype(np.float32)
    assert np.count_nonzero(contrib * edge) > 0
    assert X.exact_mismatch(bad, r) > 0


@pytest.mark.parametrize("zeros", [0.0, 0.7])
@pytest.mark.parametrize("cin,k", [(32, 3), (64, 3), (16, 7)])
def test_rho_gate_sees_two_bfloat16_pieces_and_a_filter_plane_off(cin, k, zeros):
    """On trunk-like data the correct float32 restatement (and the three-piece bfloat16 form of conv_wino4s) pass the rho gate; two
    pieces per operand instead of three, or one transform plane's filter off by one part in 2^16, fail it."""
    rng = np.random.default_rng(cin + k + int(10 * zeros))
    x = X.realistic_input((1, 12, 16, cin), rng, zeros)
    w = (rng.standard_normal((k, k, cin, 64)) / np.sqrt(k * k * cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(64)).astype(np.float32)
    r, bound, gate = X.conv_ref_f64(x, w, b), X.abs_bound(x, w, 'wino4', b), X.rho_gate('wino4', cin, k)
    assert X.rho(X.wino_f32(x, w, b, 'wino4'), r, bound) <= gate / 2
    assert X.rho(X.wino_f32(x, w, b, 'wino4', pieces=3), r, bound) <= gate / 2
    assert X.rho(X.wino_f32(x, w, b, 'wino4', pieces=2), r, bound) > gate
    us = np.ones((6, 6))
    us[1, 2] += 2.0 ** -16
    assert X.rho(X.wino_f32(x, w, b, 'wino4', u_scale=us), r, bound) > gate


@pytest.mark.parametrize("kind,k,e", [('wino2', 3, 16), ('wino7', 7, 14)])
def test_rho_gate_sees_a_filter_plane_off_in_the_other_forms(kind, k, e):
    """One plane's filter off by 2^-e.  F(4x4,4x4)'s bound is loose enough (|B^T| rows sum to 15) that 2^-16 lands at 0.5 ... 0.95 of
    the gate at n = 142: the gate resolves 2^-14 there, not 2^-16."""
    rng = np.random.default_rng(k)
    cin = 32
    x = X.realistic_input((1, 12, 16, cin), rng)
    w = (rng.standard_normal((k, k, cin, 64)) / np.sqrt(k * k * cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(64)).astype(np.float32)
    r, bound, gate = X.conv_ref_f64(x, w, b), X.abs_bound(x, w, kind, b), X.rho_gate(kind, cin, k)
    assert X.rho(X.wino_f32(x, w, b, kind), r, bound) <= gate / 2
    al = X.mat(kind, 'BT').shape[0]
    us = np.ones((al, al))
    us[3, 3] += 2.0 ** -e
    assert X.rho(X.wino_f32(x, w, b, kind, u_scale=us), r, bound) > gate


# ---------------------------------------------------------------------------------------------------------- the kernels on the interpreter
EMU_EXACT = [('direct', (2, 9, 11, 40, 21, 3), 1, False), ('direct', (1, 10, 10, 20, 64, 3), 2, False), ('direct', (1, 8, 9, 24, 32, 7), 1, False),
             ('direct', (2, 8, 8, 40, 64, 1), 1, False), ('direct', (1, 12, 12, 32, 64, 3), 1, True), ('naive', (1, 7, 9, 21, 32, 3), 2, False),
             ('first', (2, 13, 17, 3, 64, 3), 1, False), ('first_rows', (2, 13, 17, 3, 64, 3), 1, False),
             ('wino', (2, 10, 12, 64, 128, 3), 1, False), ('wino_nosplit', (2, 10, 12, 64, 128, 3), 1, True), ('wino', (1, 8, 8, 32, 64, 7), 1, False),
             ('wino2', (2, 10, 12, 32, 64, 3), 1, True), ('wino2_nosplit', (1, 9, 11, 32, 128, 3), 1, False), ('wino2', (1, 8, 8, 32, 64, 7), 1, False),
             ('wino4', (2, 10, 14, 32, 64, 3), 1, True), ('wino4_nosplit', (3, 10, 6, 16, 64, 3), 1, False), ('wino4_notail', (2, 9, 11, 32, 64, 3), 1, False),
             ('wino4', (1, 9, 11, 48, 64, 7), 1, False), ('wino4s', (2, 10, 14, 32, 64, 3), 1, True), ('wino4s_notail', (1, 9, 11, 32, 128, 3), 1, False)]


@pytest.mark.parametrize("form,shape,stride,pool", EMU_EXACT, ids=lambda v: v if isinstance(v, str) else str(v))
def test_exact_on_interpreter(emu_engine, form, shape, stride, pool):
    """Part of the GPU file's exact cases on the CPU interpreter of the same kernel sources (3 CUs: persistent grids walk several
    items, channel splits, tail pieces): counters, precondition, bit-equality, two calls bit-identical."""
    G.exact_case(emu_engine, form, shape, stride, pool)


@pytest.mark.parametrize("form,shape", [('wino', (1, 10, 12, 64, 64, 3)), ('wino2', (1, 10, 12, 32, 64, 3)), ('wino4', (1, 10, 14, 32, 64, 3)),
                                        ('wino4s', (1, 10, 14, 32, 64, 3)), ('wino7', (1, 8, 8, 32, 64, 7)), ('wino7_ks2', (1, 8, 8, 32, 64, 7)),
                                        ('direct', (1, 9, 9, 24, 64, 7))], ids=lambda v: v if isinstance(v, str) else str(v))
def test_equivariance_and_rho_on_interpreter(emu_engine, form, shape):
    B, H, W, Cin, Cout, k = shape
    rng = np.random.default_rng(sum(shape))
    x = X.realistic_input((B, H, W, Cin), rng, 0.3)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    y, _ = G.run(emu_engine, form, x, w, b, calls=1)
    for a, c in [(20, -7), (-24, 9)]:
        ys, _ = G.run(emu_engine, form, np.ldexp(x, a), np.ldexp(w, c), np.ldexp(b, a + c), calls=1)
        assert np.array_equal(ys, np.ldexp(y, a + c))
    kind = G.FORMS[form][2]
    rho = X.rho(y, X.conv_ref_f64(x, w, b), X.abs_bound(x, w, kind, b))
    print("interpreter rho %s %.3f (gate %.2f)" % (form, rho, X.rho_gate(kind, Cin, k)))
    assert rho <= X.rho_gate(kind, Cin, k)
