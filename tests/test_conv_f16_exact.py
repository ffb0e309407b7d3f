"""The checks of tests/test_gpu_conv_f16_exact.py, checked (CPU): conv_ref_f16 against oracle/nets.py's f16 layer; the property the
exact runs rest on (every integer pre-activation within +-1024 keeps its own half through the leaky-ReLU); a one- or two-tile subset
of the GPU cases on the CPU interpreter of the kernel sources (tests/emu, 3 CUs: the persistent grids need few items to walk a ragged
third round); and the tests of the tests -- perturbed copies of correct results, made in NumPy, must fail the checks."""
import numpy as np
import pytest

from oracle import conv_exact as X
from oracle import nets as N
from tests import test_gpu_conv_f16_exact as G

EMU_CUS = 3


# ---------------------------------------------------------------------------------------------------------- the helpers themselves
def _ops(w, b, acc):
    return N._Ops({'s/l/weights': w, 's/l/biases': b}, 's', acc=acc, f16=True)


@pytest.mark.parametrize("case", [(2, 9, 11, 40, 24, 3), (1, 10, 6, 19, 5, 7), (2, 6, 5, 70, 8, 1), (1, 8, 12, 3, 64, 3)])
def test_conv_ref_f16_equals_the_oracle_nets_f16_layer(case):
    """On exact data bit for bit (conv_relu + max_pool: halves; conv_lin: the float32 head); on random data the pre-activation to one
    float32 rounding (nets.py rounds its float64 sums to float32 before the bias)."""
    B, H, W, Cin, Cout, k = case
    rng = np.random.default_rng(sum(case))
    x, w, b, bound = X.exact_data_f16(case, rng)
    assert X.exact_ok_f16(bound, X.pre_f16(x, w, b))
    for acc in (np.float32, np.float64):
        ops = _ops(w, b, acc)
        assert np.array_equal(ops.conv_relu(x, 'l', k, 1, Cout), X.conv_ref_f16(x, w, b))
        assert np.array_equal(ops.max_pool(ops.conv_relu(x, 'l', k, 1, Cout), 'p'), X.conv_ref_f16(x, w, b, pool=True))
        assert np.array_equal(ops.conv_lin(x, 'l', k, 1, Cout), X.conv_ref_f16(x, w, b, act=False, out_f32=True))
    x, w, b = G.realistic(case, rng)
    t = _ops(w, b, np.float64).conv_lin(x, 'l', k, 1, Cout)
    r = X.conv_ref_f16(x, w, b, act=False, out_f32=True)
    assert t.shape == r.shape and (np.abs(t - r) <= 2.0 ** -23 * (np.abs(r) + np.abs(b))).all()
    # ... and the stored half: one nearest-even rounding of the float64 value, sub-normals kept
    h = X.conv_ref_f16(x, 2.0 ** -8 * w, 2.0 ** -8 * b)
    u = X.conv_ref_f16(x, 2.0 ** -8 * w, 2.0 ** -8 * b, out_f32=True)
    assert np.array_equal(h, u.astype(np.float16).astype(np.float64)) and ((np.abs(h) < 2.0 ** -14) & (h != 0)).any()


def test_first_block_ref_pads_conv1_1_output_with_zeros():
    """conv1_2's SAME padding pads conv1_1's OUTPUT (b1 = 27 makes a padded IMAGE differ: conv1_1 of zeros is 27, not 0)."""
    rng = np.random.default_rng(1)
    image, w1, b1, w2, b2 = X.first_block_data_f16((1, 6, 8), rng)
    r, y1 = X.first_block_ref_f16(image, w1, b1, w2, b2)
    assert r.shape == (1, 3, 4, 64) and y1.min() >= 0 and y1.max() <= 54
    y1p = np.zeros((1, 8, 10, 64))
    y1p[:, 1:-1, 1:-1] = y1
    inner = X.conv_ref_f16(y1p, w2, b2)[:, 1:-1, 1:-1]
    assert np.array_equal(X._pool2(inner), r)
    big = X.conv_ref_f16(np.pad(image, ((0, 0), (1, 1), (1, 1), (0, 0))), w1, b1, first=True)
    assert not np.array_equal(X._pool2(X.conv_ref_f16(big, w2, b2)[:, 1:-1, 1:-1]), r)


def test_every_exact_pre_activation_keeps_its_own_half():
    """Up to 2048 every integer is a half, and half(0.01f y) is pairwise distinct for y = -1600 .. 0: within exact_ok_f16's +-1024 two
    different sums never store the same half.  (The property is not a triviality: it ends before -2100.)"""
    y = np.arange(0, 2049, dtype=np.float32)
    assert np.array_equal(y.astype(np.float16).astype(np.float32), y)
    assert X.HALF_EXACT_MAX <= 1600 and X.neg_slope_halves_distinct(-1600)
    assert not X.neg_slope_halves_distinct(-2100)
    v = np.concatenate([X.LEAKY * np.arange(-1024, 0, dtype=np.float32), y[:1025]]).astype(np.float16)
    assert len(np.unique(v)) == 2049            # ... and no negative's half collides with a non-negative one


def test_spacing_half_and_half_trunc():
    v = np.array([1.0, 1.5, 2.0, 1000.0, 2.0 ** -14, 2.0 ** -15, 3e-7, 0.0])
    want = [np.float64(np.nextafter(np.float16(a), np.float16(np.inf))) - np.float64(np.float16(a)) for a in (1.0, 1.5, 2.0, 1000.0, 2.0 ** -14)]
    assert np.array_equal(X.spacing_half(v), np.array(want + [2.0 ** -24] * 3))
    t = X.half_trunc([0.1, -0.1, 1.0, 2049.0, -2.0 ** -25, 1e-8])
    assert np.array_equal(t, np.array([np.float16(0.09998), -np.float64(np.float16(0.09998)), 1.0, 2048.0, 0.0, 0.0], np.float64))


# ---------------------------------------------------------------------------------------------------------- the tests of the tests
def _exact_small(shape=(1, 12, 20, 32, 64, 3), act=True):
    rng = np.random.default_rng(3)
    x, w, b, bound = X.exact_data_f16(shape, rng)
    pre = X.pre_f16(x, w, b)
    assert X.exact_ok_f16(bound, pre)
    return x, w, b, pre, X.conv_ref_f16(x, w, b, act=act, pre=pre)


def _realistic_small(shape=(1, 12, 20, 32, 64, 3), w_scale=1.0):
    rng = np.random.default_rng(4)
    x, w, b = G.realistic(shape, rng, w_scale)
    r = X.conv_ref_f16(x, w, b, out_f32=True)
    return x, w, b, r, X.abs_bound(X._h(x), X._h(w), 'direct', b)


def _past_gate(y, r, bound, cin=32, k=3):
    return int((np.abs(y - r) > X.gate_f16(y, r, bound, cin, k)).sum())


def test_checks_see_half_an_ulp_on_one_output():
    """One output moved to the neighbouring half (one half-ulp of float32 at that value is far less: the stored half is the resolution)."""
    x, w, b, pre, r = _exact_small()
    y = r.astype(np.float32)
    assert X.exact_mismatch(y, r) == 0
    for i in (np.unravel_index(np.argmax(r), r.shape), np.unravel_index(np.argmin(r), r.shape)):
        bad = y.copy()
        bad[i] = np.nextafter(np.float16(y[i]), np.float16(np.inf))
        assert X.exact_mismatch(bad, r) == 1
    x, w, b, r, bound = _realistic_small()
    y = X._h(r)
    assert _past_gate(y, r, bound) == 0
    i = np.unravel_index(np.argmax(np.abs(r)), r.shape)
    y[i] = np.nextafter(np.float16(y[i]), np.float16(np.inf if y[i] >= r[i] else -np.inf))      # (away from r: the rounding's own error adds)
    assert _past_gate(y, r, bound) == 1


def test_checks_see_a_halo_tap_dropped_at_a_tile_edge():
    """The tap (1, 2) of the outputs in the last column of each 16-wide tile (the tap that reads the patch's halo column) left out:
    EVERY output whose sum changed stores another half."""
    x, w, b, pre, r = _exact_small()
    wt = np.zeros_like(w)
    wt[1, 2] = w[1, 2]
    contrib = X.pre_f16(x, wt, np.zeros_like(b))
    edge = (np.arange(r.shape[2]) % 16 == 15)[None, None, :, None]
    bad = X.conv_ref_f16(x, w, b, pre=pre - contrib * edge)
    changed = int(np.count_nonzero(contrib * edge))
    assert changed > 100 and X.exact_mismatch(bad, r) == changed
    x, w, b, r, bound = _realistic_small()
    wt = np.zeros_like(w)
    wt[1, 2] = w[1, 2]
    contrib = X.pre_f16(x, wt, np.zeros_like(b))
    bad = X._h(X.conv_ref_f16(x, w, b, out_f32=True, pre=X.pre_f16(x, w, b) - contrib * edge))
    assert _past_gate(bad, r, bound) > 100


def test_checks_see_truncation_instead_of_nearest_even():
    x, w, b, pre, r = _exact_small()
    unrounded = X.conv_ref_f16(x, w, b, out_f32=True, pre=pre)
    bad = X.half_trunc(unrounded)
    assert X.exact_mismatch(bad, r) > 0.2 * r.size          # (the negative outputs: 0.01f y is no half)
    x, w, b, r, bound = _realistic_small()
    assert _past_gate(X._h(r), r, bound) == 0
    assert _past_gate(X.half_trunc(r), r, bound) > 0.2 * r.size
    # ... and flushed sub-normals, on data that reach them
    x, w, b, r, bound = _realistic_small(w_scale=2.0 ** -6)
    y = X._h(r)
    sub = (np.abs(y) < 2.0 ** -14) & (y != 0)
    assert sub.sum() > 100 and _past_gate(y, r, bound) == 0
    assert _past_gate(np.where(sub, 0.0, y), r, bound) > 0.5 * sub.sum()


def test_checks_see_a_filter_tap_off_by_one():
    """The exact run's own: a filter's last bit moves an output by less than the stored half resolves on unit-normal data (the gate is
    there for the rounding mode, the exact run for the sums)."""
    x, w, b, pre, r = _exact_small()
    w2 = w.copy()
    w2[2, 0, 17, 5] += 1
    bad = X.conv_ref_f16(x, w2, b)
    changed = int(np.count_nonzero(X.pre_f16(x, w2, b) != pre))
    assert changed > 50 and X.exact_mismatch(bad, r) == changed


def test_first_bias_term_bounds_the_two_half_rows():
    """conv_first's bias as hi + lo halves: the term bounds what the two rows lose, and is attained within a factor of four."""
    b = np.concatenate([np.random.default_rng(0).standard_normal(4096) * s for s in (1.0, 1e-3, 1e-5, 100.0)]).astype(np.float32)
    hi = b.astype(np.float16).astype(np.float32)
    lo = (b - hi).astype(np.float16).astype(np.float32)
    err = np.abs(b.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    assert (err <= X.first_bias_term(b)).all() and (err > X.first_bias_term(b) / 4).any()


# ---------------------------------------------------------------------------------------------------------- the kernels on the interpreter
K7K1 = {'f16_impl': 'h16_force', 'f16_k7k1': '1'}
K7K1_OFF = {'f16_impl': 'h16_force', 'f16_k7k1': '0'}
MF = {'f16_impl': 'mfma'}
# (name, options, counters, (B, H, W, Cin, Cout, k), keywords)
EMU_CONV = [
    ('nt1', G.FORCE, G.H16, (1, 10, 12, 64, 64, 3), {}),
    ('nt1_pool_two_tiles', G.FORCE, G.H16, (1, 10, 20, 64, 64, 3), dict(pool=True)),
    ('nt1_odd_cin_pad_3_blocks', G.FORCE, G.H16, (1, 17, 9, 100, 192, 3), dict(act=False)),
    ('nt2', G.FORCE, G.H16, (1, 9, 11, 128, 128, 3), {}),
    ('nt2_pool', G.FORCE, G.H16, (1, 10, 12, 128, 128, 3), dict(pool=True, act=False)),
    ('nt4_nine_chunks', G.FORCE, G.H16, (1, 8, 8, 576, 256, 3), {}),
    ('pooled_odd_rows_to_mfma', G.FORCE, G.MFMA, (1, 9, 12, 64, 64, 3), dict(pool=True)),
    ('h16_unfilled_to_mfma', {}, G.MFMA, (1, 10, 12, 64, 64, 3), {}),
    ('walk_nt1', G.FORCE, G.H16, (2 * 3 * EMU_CUS + 1, 6, 5, 64, 64, 3), {}),
    ('walk_nt2', G.FORCE, G.H16, (2 * 2 * EMU_CUS + 1, 5, 6, 64, 128, 3), {}),
    ('k7', K7K1, G.H16, (1, 9, 9, 64, 64, 7), {}),
    ('k7_nt2_cin149', K7K1, G.H16, (1, 7, 17, 149, 128, 7), {}),
    ('k1', K7K1, G.H16, (1, 9, 11, 128, 64, 1), {}),
    ('k7_off', K7K1_OFF, G.MFMA, (1, 9, 9, 64, 64, 7), {}),
    ('k1_off', K7K1_OFF, G.MFMA, (1, 9, 11, 128, 64, 1), {}),
    ('mfma_3x3', MF, G.MFMA, (1, 9, 11, 128, 128, 3), {}),
    ('mfma_pool', MF, G.MFMA, (1, 10, 12, 64, 64, 3), dict(pool=True)),
    ('mfma_head_splitk', MF, G.MFMA_SPLITK, (1, 9, 11, 128, 21, 1), dict(act=False, out_f32=True)),
    ('mfma_head', MF, G.MFMA, (1, 9, 11, 64, 2, 1), dict(act=False, out_f32=True)),
    ('first', {}, G.FIRST, (2, 13, 17, 3, 64, 3), {}),
    ('first_rows', {'first_walk': 'rows'}, G.FIRST, (2, 13, 17, 3, 64, 3), {}),
]


@pytest.mark.parametrize("name,opts,expect,shape,kw", EMU_CONV, ids=[c[0] for c in EMU_CONV])
def test_exact_on_interpreter(emu_engine, name, opts, expect, shape, kw):
    G.exact_conv(emu_engine, opts, expect, shape, **kw)


EMU_BLOCK = [('two_launch', '0', G.TWO_LAUNCH_H16, (2, 12, 10)), ('ring', 'ring', G.H16, (2, 12, 10)), ('resident', 'resident', G.RESIDENT, (2, 12, 10)),
             ('ring_two_tiles', 'ring', G.H16, (1, 18, 10)), ('resident_two_tiles', 'resident', G.RESIDENT, (1, 10, 18)),
             ('odd_rows_two_launch', '1', G.TWO_LAUNCH_MFMA, (1, 9, 12)),
             ('walk_resident', 'resident', G.RESIDENT, (2 * EMU_CUS + 1, 6, 8)), ('walk_ring', 'ring', G.H16, (2 * 2 * EMU_CUS + 1, 8, 6))]


@pytest.mark.parametrize("name,fuse,expect,shape", EMU_BLOCK, ids=[c[0] for c in EMU_BLOCK])
def test_first_block_exact_on_interpreter(emu_engine, name, fuse, expect, shape):
    G.exact_block(emu_engine, {'f16_impl': 'h16_force', 'f16_fuse12': fuse}, expect, shape)


EMU_GATE = [('h16_subnormal', G.FORCE, G.H16, (1, 10, 12, 64, 64, 3), dict(w_scale=2.0 ** -6, subnormal=True)),
            ('h16_k7', K7K1, G.H16, (1, 9, 9, 64, 64, 7), {}),
            ('mfma_pool', MF, G.MFMA, (1, 10, 12, 64, 64, 3), dict(pool=True)),
            ('mfma_head_splitk', MF, G.MFMA_SPLITK, (1, 9, 11, 128, 21, 1), dict(act=False, out_f32=True)),
            ('first', {}, G.FIRST, (2, 13, 17, 3, 64, 3), {})]


@pytest.mark.parametrize("name,opts,expect,shape,kw", EMU_GATE, ids=[c[0] for c in EMU_GATE])
def test_gate_on_interpreter(emu_engine, name, opts, expect, shape, kw):
    G.gated_conv(emu_engine, opts, expect, shape, **kw)


@pytest.mark.parametrize("fuse", ['ring', 'resident'])
def test_first_block_gate_on_interpreter(emu_engine, fuse):
    G.gated_block(emu_engine, fuse, G.RESIDENT if fuse == 'resident' else G.H16, (1, 12, 10))


def test_refusals_and_untouched_state(emu_engine):
    """Shapes no half-precision kernel takes are refused by run_conv's own errors, on a context without finalized weights."""
    rng = np.random.default_rng(0)
    x, w, b, _ = X.exact_data_f16((1, 8, 8, 64, 64, 3), rng)
    with pytest.raises(NotImplementedError):
        emu_engine.conv2d_f16(x, w, b, stride=2)
    w7 = rng.integers(-1, 2, (7, 7, 64, 64)).astype(np.float32)
    with pytest.raises(NotImplementedError):
        emu_engine.conv2d_f16(x, w7, b, pool=True)
