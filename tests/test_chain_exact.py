"""The checks of tests/test_gpu_chain_exact.py, checked (CPU): the multiple-of-100 rule and the preconditions of oracle/chain_exact.py
on their own, the tests of the tests (one weight, one bias, one hand-side flag, the slope's float32 neighbour, a data set that breaks
the rule), and the multi-layer kernels themselves on the CPU interpreter of the kernel sources (tests/emu) at the small batches and
the 4- and 6-pixel maps: the same case functions the GPU file runs."""
import os

import numpy as np
import pytest

from oracle import chain_exact as C
from oracle import nets as N
from oracle import tf_ops as T
from tests import test_gpu_chain_exact as G

slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="long CPU-interpreter run; HP3D_SLOW=1 to enable")
CPU_POOL = 6


# ---------------------------------------------------------------------------------------------------------- the rule and the builders
def test_multiple_of_100_rule():
    """fl32(0.01f * (-100 m)) == -m for every m up to 2^24 / 100, under power-of-two scalings too; not so for the slope's float32
    neighbours, nor for multiples of 10 (the rule is about 0.01f, not about round numbers)."""
    assert C.slope_identity_holds()
    m = np.arange(1, int(C.TWO24) // 100 + 1, dtype=np.float64)
    for e in (-20, -3, 7, 30):
        v = np.ldexp((-100.0 * m).astype(np.float32), e)
        assert np.array_equal((C.LEAKY * v).astype(np.float64), np.ldexp(-m, e))
    assert not C.slope_identity_holds(np.nextafter(C.LEAKY, np.float32(1)))
    assert not C.slope_identity_holds(np.nextafter(C.LEAKY, np.float32(0)))
    v = (-10.0 * np.arange(1, 1000)).astype(np.float32)
    assert not np.array_equal(C.LEAKY * v, np.rint(C.LEAKY * v))


@pytest.mark.parametrize("name", list(C.LIFT_SETS))
def test_lift_sets_meet_their_preconditions(name):
    """Every lifting data set at the GPU file's pool size (the reference alone: integer taps, bound, negative fractions, live channels)."""
    w, sm, hs, (rel, can, R, u) = G.lift_data(name, G.GPU_POOL)
    assert len(np.unique(hs, axis=0)) == 2, "both hand sides"
    assert np.array_equal(can, np.rint(can))
    if name == 'small_u':
        assert np.array_equal(u, np.rint(u)) and np.abs(u).max() <= 8 and C.rot_sensitivity(u) > 0.05


@pytest.mark.parametrize("case", G.HEAD_CASES, ids=lambda c: "B%d_%dx%d_x%d" % c[:4])
def test_head_cases_meet_their_preconditions(case):
    w, img, ref = G.head_data(case)
    for net in ref:
        for hid, frac in ref[net][1].items():
            assert 0.25 <= frac <= 0.75, (hid, frac)


def test_rodrigues64_is_get_rot_mat():
    u = np.random.default_rng(0).integers(-8, 9, (40, 3)).astype(np.float64)
    R = N.get_rot_mat(u[:, :1], u[:, 1:2], u[:, 2:])
    assert np.abs(C.rodrigues64(u) - R).max() < 2e-6


# ---------------------------------------------------------------------------------------------------------- the tests of the tests
def _negconv_small():
    return G.lift_data('negconv', CPU_POOL)


def test_reference_sees_one_weight_one_bias_one_hand_side_flag():
    """The float64 reference itself moves when one weight changes by 1, one bias by 100 or one hand-side flag flips (the equality with
    an unchanged kernel output would fail); on the interpreter the same three changes: test_kernel_sees_... below."""
    w, sm, hs, (rel, can, R, u) = _negconv_small()
    for key, idx, step in (('PosePrior/conv_pose_2_2/weights', None, 1), ('PosePrior/fc_rel1/biases', (511,), 100), ('PosePrior/fc_xyz/weights', None, 1)):
        w2 = dict(w)
        a = w[key].copy()
        i = idx if idx is not None else tuple(np.argwhere(a != 0)[-1])
        a[i] += step
        w2[key] = a
        assert G.mismatch(N.poseprior_can(w2, sm, hs, acc=np.float64), can) > 0, key
    hs2 = hs.copy()
    hs2[1] = hs2[1, ::-1]
    assert G.mismatch(N.poseprior_can(w, sm, hs2, acc=np.float64)[1], can[1]) > 0
    assert G.mismatch(N.poseprior_can(w, sm, hs2, acc=np.float64)[0], can[0]) == 0


def test_rule_violation_is_rejected():
    """The layer behind a 'neg' layer turned into a selection: the -m it passes on are no multiples of 100 and meet the next leaky-ReLU.
    check() flags the set (non-integer taps); the same set with the 'pos' layer in place passes."""
    spec, neg, (vmax, density), _ = C.LIFT_SETS['negconv']
    bad = dict(spec)
    bad['conv_pose_2_1'] = ('sel', 1)
    sm, hs = C.lift_pool(1, CPU_POOL, vmax, density)
    for s, ok in ((spec, True), (bad, False)):
        w = C.lift_weights(2, sm, hs, s)
        rel, can, R, u, taps, bound = C.lift_reference(w, sm, hs)
        if ok:
            C.check(taps, bound, neg, C.lift_layers(w, taps, sm, hs))
        else:
            with pytest.raises(AssertionError, match="not integer"):
                C.check(taps, bound, neg, C.lift_layers(w, taps, sm, hs))


def test_preconditions_flag_bound_dead_channel_and_one_sided_layer():
    w, sm, hs, (rel, can, R, u) = _negconv_small()
    rel, can, R, u, taps, bound = C.lift_reference(w, sm, hs)
    C.check(taps, bound, C.LIFT_SETS['negconv'][1], C.lift_layers(w, taps, sm, hs))
    with pytest.raises(AssertionError, match="2\\^24"):
        C.check(taps, dict(bound, x=np.array([C.TWO24])), (), ())
    with pytest.raises(AssertionError, match="negative"):
        C.check(taps, bound, ['PosePrior/conv_pose_0_1'], ())         # a selection layer: nothing below zero
    w2 = dict(w)
    w2['PosePrior/conv_pose_1_1/weights'] = w['PosePrior/conv_pose_1_1/weights'].copy()
    w2['PosePrior/conv_pose_1_1/weights'][:, :, 7, :] = 0
    with pytest.raises(AssertionError, match="no outgoing weight"):
        C.check(taps, bound, (), C.lift_layers(w2, taps, sm, hs))
    t2 = dict(taps)
    t2['PosePrior/conv_pose_0_2'] = taps['PosePrior/conv_pose_0_2'].copy()
    t2['PosePrior/conv_pose_0_2'][..., 3] = 5
    with pytest.raises(AssertionError, match="constant"):
        C.check(t2, bound, (), C.lift_layers(w, t2, sm, hs))


def test_slope_neighbour_changes_the_reference(monkeypatch):
    """0.01f replaced by its float32 neighbour in the oracle's leaky-ReLU: the reference of a set that takes the negative branch moves
    (so a kernel whose slope is one ulp off cannot equal it), the all-non-negative set's does not.  The sets that show it have a probe
    output (chain_exact.probe): behind any further layer the 1e-7 m a wrong slope adds vanishes in a float32 sum of larger terms."""
    leaky = T.leaky_relu
    for name, moves in (('negfc1', True), ('nonneg', False)):
        w, sm, hs, (rel, can, R, u) = G.lift_data(name, CPU_POOL)
        for nb in (np.nextafter(C.LEAKY, np.float32(1)), np.nextafter(C.LEAKY, np.float32(0))):
            monkeypatch.setattr(T, 'leaky_relu', lambda x, slope=0.01, nb=nb: leaky(x, nb))
            assert (G.mismatch(N.poseprior_can(w, sm, hs, acc=np.float64), can) > 0) == moves, (name, nb)
            monkeypatch.setattr(T, 'leaky_relu', leaky)
    w, img, ref = G.head_data(G.HEAD_CASES[0])
    monkeypatch.setattr(T, 'leaky_relu', lambda x, slope=0.01: leaky(x, np.nextafter(C.LEAKY, np.float32(1))))
    assert G.mismatch(N.handsegnet(w, img, acc=np.float64)[0], ref['HandSegNet'][0][0]) > 0
    for a, b in zip(N.posenet2d(w, img, acc=np.float64), ref['PoseNet2D'][0]):
        assert G.mismatch(a, b) > 0


# ---------------------------------------------------------------------------------------------------------- the kernels on the interpreter
@pytest.fixture(scope='module')
def lift_engine(emu_engine, synth_weights):
    yield emu_engine
    G.restore(emu_engine, synth_weights)


@pytest.fixture(scope='module')
def head_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(G.cached('head_w', lambda: C.head_weights(G.HEAD_SEED)))
    emu_engine.finalize_weights()
    yield emu_engine
    G.restore(emu_engine, synth_weights)


# (the interpreter has no second stream: lift_overlap = 1 runs the towers one after the other there and its counter stays put, so the
#  'serial' path is the 'unfused' one; 'auto' is 'fused' up to B = 4)
CPU_PATHS = ('fused', 'unfused', 'tail_only', 'gemm_only', 'anchor')


_FU = ('fused', 'unfused')


@pytest.mark.parametrize("name,batches", [('nonneg', (3, (1, ('auto',)), (5, ('fused',)))), ('negconv', ((2, _FU),)),
                                          ('negfc0', ((2, _FU),)), ('negfc1', ((2, _FU),))], ids=lambda v: v if isinstance(v, str) else '')
def test_lift_exact_on_interpreter(lift_engine, name, batches):
    """Every path at B = 3 (an odd batch: fc_tail takes two images per workgroup) on the non-negative set, the one-launch and the
    default layer-by-layer form on the others, the one-launch form at B = 1 and at the first batch above the fused limit."""
    G.lift_case(lift_engine, name, CPU_POOL, batches, CPU_PATHS, overlap_counts=False)


def test_lift_rotation_on_small_integer_u_on_interpreter(lift_engine):
    G.small_u_case(lift_engine, CPU_POOL, (2,), ('fused', 'unfused'), overlap_counts=False)


def test_lift_interleaved_and_repeated_calls_on_interpreter(lift_engine, monkeypatch):
    monkeypatch.setattr(G, 'lift_run', lambda e, path, sm, hs, oc=True, f=G.lift_run: f(e, path, sm, hs, False))
    G.interleave_case(lift_engine, CPU_POOL, 2, ('fused', 'unfused'), repeats=1)


def test_poseprior_variants_exact_on_interpreter(lift_engine):
    G.variants_case(lift_engine, CPU_POOL, 3)


def test_kernel_sees_one_weight_one_bias_one_hand_side_flag(lift_engine):
    """The equality fails on the interpreter when the ENGINE's weights differ from the reference's by one weight (+1), one bias (+100) or
    when one hand-side flag is flipped (the flag on the one-launch and the layer-by-layer form, the weights on the one-launch form)."""
    w, sm, hs, (rel, can, R, u) = G.lift_data('negfc0', CPU_POOL)
    B = 3
    hs2 = hs[:B].copy()
    hs2[2] = hs2[2, ::-1]
    wk = w['PosePrior/conv_pose_2_2/weights'].copy()
    wk[tuple(np.argwhere(wk != 0)[-1])] += 1
    bk = w['PosePrior/fc_rel0/biases'].copy()
    bk[-1] += 100
    try:
        for change in ({}, {'PosePrior/conv_pose_2_2/weights': wk}, {'PosePrior/fc_rel0/biases': bk}):
            G.lift_load(lift_engine, dict(w, **change))
            for path in ('fused', 'unfused') if not change else ('fused',):
                o = G.lift_run(lift_engine, path, sm[:B], hs[:B], False)
                assert (G.mismatch(o[1], can[:B]) > 0) == bool(change), (path, list(change))
                if not change:
                    o = G.lift_run(lift_engine, path, sm[:B], hs2, False)
                    assert G.mismatch(o[1][2], can[2]) > 0 and G.mismatch(o[1][:2], can[:2]) == 0, path
    finally:
        G.lift_load(lift_engine, w)


@pytest.mark.parametrize("case", [(1, 16, 16, 2, 5), (1, 16, 24, 2, 3)], ids=lambda c: "B%d_%dx%d_x%d" % c[:4])
def test_head_pairs_exact_on_interpreter(head_engine, case):
    """The 4- and 6-pixel maps (a partial tile of conv_pw2.hip's 64 pixels) as one launch per pair.  (A pass through both networks
    takes the interpreter 20 s: the two-launch form, whose kernels test_conv_exact.py pins layer by layer, and the sizes at the tile
    edges are part of the HP3D_SLOW test.)"""
    G.head_case(head_engine, case, ('force',))


@slow
def test_head_pairs_exact_on_interpreter_tile_edges(head_engine):
    for case in [(1, 16, 16, 2, 5), (1, 16, 24, 2, 3)] + G.HEAD_CASES[1:4]:
        G.head_case(head_engine, case)
