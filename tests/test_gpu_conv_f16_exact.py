"""Every half-precision convolution kernel, layer by layer, held to a float64 reference (oracle/conv_exact.py: conv_ref_f16).

* Exact runs: integer inputs, filters in {-1, 0, 1}, integer biases, such that (a) every partial sum stays below 2^24 and (b) every
  pre-activation is an integer within +-1024 (both asserted per case on the reference, before the kernel runs).  Every value a kernel
  forms is then exact in float32, every y >= 0 is its own half and half(0.01f y) tells any two y < 0 apart, so the result must equal the
  reference BIT FOR BIT whatever the tiling, cout blocking, chunk count, buffering or summation order -- and a sum that is off by one
  shows.  Every case runs twice (bit-identical repeats) and asserts that exactly the intended kernel's launch counter moved.
* Non-integer data (unit-normal input, He-scaled filters), one case per kernel family, under gate_f16: half a half-spacing for the one
  nearest-even rounding of the stored half + the float32 sums' rho gate; one case reaches the half sub-normal range.

The shapes are the smallest at which each mechanism is live (cout blocks per wave NT = 1, 2, 4; ragged tiles; an odd chunk count of
the double-buffered patch; a persistent grid that walks a ragged third round; the split-K heads).  (B, H, W, Cin, Cout).
"""
import time

import numpy as np
import pytest

from oracle import conv_exact as X

pytestmark = pytest.mark.gpu

CUS = 256                         # compute units of the MI355X: the persistent grids are CUS x workgroups per CU
DEFAULTS = {'f16_impl': 'h16', 'f16_k7k1': '1', 'f16_fuse12': '1', 'first_walk': 'balanced'}
COUNTERS = ['conv_h16_launches', 'conv_h16_first_resident_launches', 'conv_mfma_launches', 'conv_first_launches', 'conv_splitk_reduce_launches',
            'conv_wino_launches', 'conv_wino2_launches', 'conv_wino4_launches', 'conv_wino4s_launches', 'conv_wino7_launches', 'conv_pw2_launches']
H16 = {'conv_h16_launches': 1}
MFMA = {'conv_mfma_launches': 1}
MFMA_SPLITK = {'conv_mfma_launches': 1, 'conv_splitk_reduce_launches': 1}
FIRST = {'conv_first_launches': 1}
RESIDENT = {'conv_h16_launches': 1, 'conv_h16_first_resident_launches': 1}
TWO_LAUNCH_H16 = {'conv_first_launches': 1, 'conv_h16_launches': 1}
TWO_LAUNCH_MFMA = {'conv_first_launches': 1, 'conv_mfma_launches': 1}
FORCE = {'f16_impl': 'h16_force'}


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run(e, opts, expect, call, calls=2):
    """`calls` runs of `call` under options `opts`: every counter moved by exactly `expect` per call (nothing else ran) and the runs
    are bit-identical.  Returns (output, seconds per call)."""
    c0 = {c: e.counter(c) for c in COUNTERS}
    for k, v in opts.items():
        e.set_option(k, v)
    try:
        t0 = time.time()
        ys = [call() for _ in range(calls)]
        dt = (time.time() - t0) / calls
    finally:
        for k in opts:
            e.set_option(k, DEFAULTS[k])
    d = {c: e.counter(c) - c0[c] for c in COUNTERS}
    for c in COUNTERS:
        assert d[c] == calls * expect.get(c, 0), (opts, {c: v for c, v in d.items() if v}, expect)
    for y in ys[1:]:
        assert bits_equal(ys[0], y), "two calls differ (%s)" % opts
    return ys[0], dt


def _kernel(expect):
    return '+'.join(c.replace('_launches', '') for c in expect)


def exact_conv(e, opts, expect, shape, pool=False, act=True, out_f32=False, seed=0):
    """An exact run of one layer, shape (B, H, W, Cin, Cout, k): preconditions, then bit-equality with conv_ref_f16."""
    B, H, W, Cin, Cout, k = shape
    rng = np.random.default_rng(seed + sum(shape))
    t0 = time.time()
    x, w, b, bound = X.exact_data_f16(shape, rng)
    pre = X.pre_f16(x, w, b)
    assert X.exact_ok_f16(bound, pre), "precondition: abs_bound %.3g, max |y| %.3g" % (bound.max(), np.abs(pre).max())
    r = X.conv_ref_f16(x, w, b, 1, act, pool, out_f32, first=(Cin == 3 and Cout == 64 and k == 3 and not pool), pre=pre)
    t1 = time.time()
    y, dt = run(e, opts, expect, lambda: e.conv2d_f16(x, w, b, 1, act, pool, out_f32))
    print("f16exact %-22s %-30s pool %d act %d f32 %d  max|y| %4d  neg %.2f  ref %.2f s  kernel %.3f s" % (
        _kernel(expect), shape, pool, act, out_f32, np.abs(pre).max(), (pre < 0).mean(), t1 - t0, dt))
    nbad = X.exact_mismatch(y, r)
    assert nbad == 0, "%s %s: %d of %d outputs differ, max %.3g (|r| max %.3g)" % (opts, shape, nbad, r.size, np.nanmax(np.abs(y - r)), np.abs(r).max())


def exact_block(e, opts, expect, shape, seed=0):
    """An exact run of the first block on an image (B, H, W): conv1_1's output an integer in 0 .. 54, conv1_2 under exact_ok_f16."""
    rng = np.random.default_rng(seed + sum(shape))
    t0 = time.time()
    image, w1, b1, w2, b2 = X.first_block_data_f16(shape, rng, density2=1.0 / 16)
    r, y1 = X.first_block_ref_f16(image, w1, b1, w2, b2)
    assert y1.min() >= 0 and y1.max() <= 54 and np.array_equal(y1, np.round(y1))
    pre2 = X.pre_f16(y1, w2, b2)
    assert X.exact_ok_f16(X.abs_bound(y1, w2, 'direct', b2), pre2), "precondition: max |y2| %.3g" % np.abs(pre2).max()
    t1 = time.time()
    y, dt = run(e, opts, expect, lambda: e.first_block_f16(image, w1, b1, w2, b2))
    print("f16exact %-22s %-30s %-26s max|y| %4d  neg %.2f  ref %.2f s  kernel %.3f s" % (
        _kernel(expect), shape, opts.get('f16_fuse12', ''), np.abs(pre2).max(), (pre2 < 0).mean(), t1 - t0, dt))
    nbad = X.exact_mismatch(y, r)
    assert nbad == 0, "%s %s: %d of %d outputs differ, max %.3g" % (opts, shape, nbad, r.size, np.nanmax(np.abs(y - r)))


def _id(c):
    return "B%d_%dx%d_%d-%d" % tuple(c[:5]) + ''.join("_%s" % v for v in c[5:])


# ---------------------------------------------------------------------------------------------------------- conv_h16.hip, 3x3
# (B, H, W, Cin, Cout, pool, act)
H16_3X3 = [
    (2, 24, 40, 64, 64, 0, 1), (2, 24, 40, 64, 64, 1, 1),             # NT = 1 (three workgroups per CU), ragged tile rows
    (1, 17, 33, 100, 192, 0, 0),                                      # odd extents, Cin padded to 128, three cout blocks, no activation
    (2, 24, 40, 128, 128, 0, 1), (2, 24, 40, 128, 128, 1, 1),         # NT = 2
    (1, 40, 24, 256, 384, 0, 0),                                      # NT = 2 (384 is no multiple of 256), four chunks
    (1, 24, 40, 512, 256, 0, 1), (1, 24, 40, 512, 256, 1, 1),         # NT = 4: the double-buffered patch, eight chunks
    (1, 16, 16, 512, 512, 0, 0),                                      # NT = 4, one tile, two cout blocks
    (1, 20, 20, 576, 256, 0, 1),                                      # NT = 4, nine chunks: an odd count on two buffers
]


@pytest.mark.parametrize("case", H16_3X3, ids=_id)
def test_h16_3x3_exact(gpu_engine, case):
    B, H, W, Cin, Cout, pool, act = case
    exact_conv(gpu_engine, FORCE, H16, (B, H, W, Cin, Cout, 3), bool(pool), bool(act))


def test_h16_pooled_odd_rows_run_on_conv_mfma(gpu_engine):
    """conv_h16's pooled epilogue needs even Ho and Wo: 25 rows go to conv_mfma's pooled F16 form (Ho / 2 = 12 rows out)."""
    exact_conv(gpu_engine, FORCE, MFMA, (1, 25, 40, 64, 64, 3), pool=True)


def test_h16_unfilled_grid_runs_on_conv_mfma(gpu_engine):
    """f16_impl = h16 (the default) takes conv_h16 only where the grid fills the chip: 12 items do not."""
    exact_conv(gpu_engine, {}, MFMA, (2, 24, 40, 64, 64, 3))


# one case per NT whose persistent grid walks a ragged third round: items >= 2 slots + 1, slots = CUS x workgroups per CU.
# Single-tile images (some ragged) and a large B keep the reference small.  (B, H, W, Cin, Cout, workgroups per CU, NT, act)
H16_WALK = [(513, 12, 9, 64, 192, 3, 1, 1), (342, 9, 12, 128, 384, 2, 2, 1), (257, 5, 7, 512, 512, 1, 4, 1)]


@pytest.mark.parametrize("case", H16_WALK, ids=_id)
def test_h16_persistent_walk_exact(gpu_engine, case):
    B, H, W, Cin, Cout, wps, nt, act = case
    assert B * (Cout // (64 * nt)) >= 2 * CUS * wps + 1
    exact_conv(gpu_engine, {}, H16, (B, H, W, Cin, Cout, 3), act=bool(act))         # (f16_impl = h16: the grid fills)


# ---------------------------------------------------------------------------------------------------------- conv_h16.hip, 7x7 and 1x1
# (B, H, W, Cin, Cout, k)
K7K1 = [(1, 24, 40, 64, 64, 7), (2, 17, 33, 149, 128, 7), (2, 24, 40, 512, 128, 1), (1, 17, 33, 128, 64, 1),
        (1, 24, 24, 512, 512, 1)]                                     # (the last: NT 4 is demoted to 2)


@pytest.mark.parametrize("k7k1", ['1', '0'])
@pytest.mark.parametrize("case", K7K1, ids=_id)
def test_h16_k7_k1_exact(gpu_engine, case, k7k1):
    """The single-buffer 7x7 / 1x1 forms (f16_k7k1 = 1); with f16_k7k1 = 0 the same layers go to conv_mfma and stay exact."""
    exact_conv(gpu_engine, {'f16_impl': 'h16_force', 'f16_k7k1': k7k1}, H16 if k7k1 == '1' else MFMA, case)


# ---------------------------------------------------------------------------------------------------------- conv_mfma.hip, F16
# (B, H, W, Cin, Cout, k, pool)
MFMA_CASES = [(2, 24, 40, 128, 128, 3, 0), (2, 24, 40, 64, 64, 3, 1), (2, 17, 33, 149, 128, 7, 0), (1, 17, 33, 128, 64, 1, 0)]


@pytest.mark.parametrize("case", MFMA_CASES, ids=_id)
def test_mfma_f16_exact(gpu_engine, case):
    exact_conv(gpu_engine, {'f16_impl': 'mfma'}, MFMA, case[:6], pool=bool(case[6]))


# The float32 score-map heads (out_f32, no activation).  conv_mfma_plan: Cout pads to 32 (bn = 32), blocks = B ceil(H/8) ceil(W/8)
# < 768, so the Cin / 64 chunks of 64 halves split min(ceil(768 / blocks), chunks, 16) ways: 8 for 512 channels on 40 blocks, 2 for
# 128 channels on 16 blocks, and not at all for the one chunk of 64 channels.  (B, H, W, Cin, Cout, splits)
HEADS = [(2, 30, 40, 512, 2, 8), (1, 32, 32, 128, 21, 2), (2, 24, 24, 64, 21, 1)]


@pytest.mark.parametrize("case", HEADS, ids=_id)
def test_mfma_f16_heads_exact(gpu_engine, case):
    B, H, W, Cin, Cout, ks = case
    exact_conv(gpu_engine, {'f16_impl': 'mfma'}, MFMA_SPLITK if ks > 1 else MFMA, (B, H, W, Cin, Cout, 1), act=False, out_f32=True)


# ---------------------------------------------------------------------------------------------------------- conv_first.hip, F16
@pytest.mark.parametrize("walk", ['balanced', 'rows'])
@pytest.mark.parametrize("case", [(1, 37, 53), (3, 24, 40)], ids=lambda c: "B%d_%dx%d" % c)
def test_first_layer_f16_exact(gpu_engine, case, walk):
    B, H, W = case
    exact_conv(gpu_engine, {'first_walk': walk}, FIRST, (B, H, W, 3, 64, 3))


# ---------------------------------------------------------------------------------------------------------- the fused first block
@pytest.mark.parametrize("fuse", ['0', 'ring', 'resident'])
@pytest.mark.parametrize("case", [(2, 24, 40), (1, 50, 34)], ids=lambda c: "B%d_%dx%d" % c)
def test_first_block_exact(gpu_engine, case, fuse):
    expect = {'0': TWO_LAUNCH_H16, 'ring': H16, 'resident': RESIDENT}[fuse]
    exact_block(gpu_engine, {'f16_impl': 'h16_force', 'f16_fuse12': fuse}, expect, case)


# a persistent grid that walks a ragged third round, per fused form: one workgroup per CU (resident), two (ring)
@pytest.mark.parametrize("fuse,case", [('resident', (513, 12, 10)), ('ring', (1025, 10, 12))], ids=lambda v: v if isinstance(v, str) else "B%d_%dx%d" % v)
def test_first_block_persistent_walk_exact(gpu_engine, fuse, case):
    assert case[0] >= 2 * CUS * (1 if fuse == 'resident' else 2) + 1
    exact_block(gpu_engine, {'f16_fuse12': fuse}, RESIDENT if fuse == 'resident' else H16, case)


@pytest.mark.parametrize("fuse", ['1', 'resident'])
def test_first_block_odd_extent_takes_two_launches(gpu_engine, fuse):
    """25 rows: no fused form (and no pooled conv_h16) takes an odd extent -- conv_first, then conv_mfma's pooled form."""
    exact_block(gpu_engine, {'f16_impl': 'h16_force', 'f16_fuse12': fuse}, TWO_LAUNCH_MFMA, (1, 25, 40))


# ---------------------------------------------------------------------------------------------------------- non-integer data
def realistic(shape, rng, w_scale=1.0):
    B, H, W, Cin, Cout, k = shape
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (w_scale * rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = (w_scale * 0.1 * rng.standard_normal(Cout)).astype(np.float32)
    return x, w, b


def gated_conv(e, opts, expect, shape, pool=False, act=True, out_f32=False, w_scale=1.0, subnormal=False):
    """A run on unit-normal data against the UNROUNDED reference under gate_f16.  Returns the output."""
    B, H, W, Cin, Cout, k = shape
    rng = np.random.default_rng(sum(shape) + 7)
    x, w, b = realistic(shape, rng, w_scale)
    xh, wh = X._h(x), X._h(w)
    r = X.conv_ref_f16(x, w, b, 1, act, pool, out_f32=True)
    bound = X.abs_bound(xh, wh, 'direct', b)
    bound = X.pool_bound(bound) if pool else bound
    first_b = b if expect is FIRST else None
    y, _ = run(e, opts, expect, lambda: e.conv2d_f16(x, w, b, 1, act, pool, out_f32))
    err = np.abs(y.astype(np.float64) - r)
    tol = X.gate_f16(y, r, bound, Cin, k, out_f32, first_b)
    sub = int(np.count_nonzero((np.abs(r) < 2.0 ** -14) & (r != 0)))
    print("f16rho   %-22s %-30s pool %d f32 %d  rho %.3f (gate %.2f)  worst err/tol %.3f  sub-normal outputs %d" % (
        _kernel(expect), shape, pool, out_f32, X.rho_f16(y, r, bound, out_f32, first_b), X.rho_gate('direct', Cin, k), float(np.max(err / tol)), sub))
    if subnormal:
        assert sub > 100, "no outputs in the half sub-normal range: %d" % sub
    assert np.isfinite(y).all() and (err <= tol).all(), "%d outputs past the gate, worst %.3g x" % (int((err > tol).sum()), float(np.max(err / tol)))
    return y


REALISTIC = [
    ('h16_nt1_pool', FORCE, H16, (2, 24, 40, 64, 64, 3), dict(pool=True)),
    ('h16_nt2', FORCE, H16, (1, 40, 24, 256, 384, 3), {}),
    ('h16_nt4', FORCE, H16, (1, 20, 20, 576, 256, 3), {}),
    ('h16_k7', FORCE, H16, (2, 17, 33, 149, 128, 7), {}),
    ('h16_k1', FORCE, H16, (1, 17, 33, 128, 64, 1), dict(act=False)),
    ('h16_subnormal', FORCE, H16, (2, 24, 40, 64, 64, 3), dict(w_scale=2.0 ** -6, subnormal=True)),
    ('mfma_pool', {'f16_impl': 'mfma'}, MFMA, (2, 24, 40, 64, 64, 3), dict(pool=True)),
    ('mfma_k7', {'f16_impl': 'mfma'}, MFMA, (2, 17, 33, 149, 128, 7), {}),
    ('mfma_subnormal', {'f16_impl': 'mfma'}, MFMA, (2, 24, 40, 128, 128, 3), dict(w_scale=2.0 ** -6, subnormal=True)),
    ('mfma_head_splitk', {'f16_impl': 'mfma'}, MFMA_SPLITK, (2, 30, 40, 512, 2, 1), dict(act=False, out_f32=True)),
    ('first', {}, FIRST, (3, 24, 40, 3, 64, 3), {}),
    ('first_subnormal', {}, FIRST, (1, 37, 53, 3, 64, 3), dict(w_scale=2.0 ** -6, subnormal=True)),
]


@pytest.mark.parametrize("name,opts,expect,shape,kw", REALISTIC, ids=[c[0] for c in REALISTIC])
def test_gate_on_unit_normal_data(gpu_engine, name, opts, expect, shape, kw):
    gated_conv(gpu_engine, opts, expect, shape, **kw)


def gated_block(e, fuse, expect, shape):
    """The fused forms on unit-normal data.  Their patch stage restates conv_first_kernel<true> (operand order, rounding points and
    accumulation order: bit-identical halves), so conv1_2's reference is taken on conv1_1's output as conv_first gives it -- itself
    held to its own gate here -- and the fused result is held to conv1_2's gate on that input."""
    B, H, W = shape
    rng = np.random.default_rng(sum(shape) + 11)
    image, w1, b1 = realistic((B, H, W, 3, 64, 3), rng)
    _, w2, b2 = realistic((1, 1, 1, 64, 64, 3), rng)
    y1, _ = run(e, {}, FIRST, lambda: e.conv2d_f16(image, w1, b1), calls=1)
    r1 = X.conv_ref_f16(image, w1, b1, out_f32=True)
    assert (np.abs(y1 - r1) <= X.gate_f16(y1, r1, X.abs_bound(X._h(image), X._h(w1), 'direct', b1), 3, 3, first_b=b1)).all()
    r = X.conv_ref_f16(y1, w2, b2, pool=True, out_f32=True)
    bound = X.pool_bound(X.abs_bound(y1, X._h(w2), 'direct', b2))
    y, _ = run(e, {'f16_impl': 'h16_force', 'f16_fuse12': fuse}, expect, lambda: e.first_block_f16(image, w1, b1, w2, b2))
    err, tol = np.abs(y.astype(np.float64) - r), X.gate_f16(y, r, bound, 64, 3)
    print("f16rho   %-22s %-30s %-8s rho %.3f (gate %.2f)  worst err/tol %.3f" % (_kernel(expect), shape, fuse, X.rho_f16(y, r, bound), X.rho_gate('direct', 64, 3),
                                                                                 float(np.max(err / tol))))
    assert np.isfinite(y).all() and (err <= tol).all(), "%d outputs past the gate, worst %.3g x" % (int((err > tol).sum()), float(np.max(err / tol)))


@pytest.mark.parametrize("fuse", ['ring', 'resident'])
def test_first_block_gate_on_unit_normal_data(gpu_engine, fuse):
    gated_block(gpu_engine, fuse, RESIDENT if fuse == 'resident' else H16, (2, 24, 40))
