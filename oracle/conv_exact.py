"""Exact and error-normalised checks of the float32 convolution kernels (oracle; test infrastructure only).

conv_ref_f64  TF-SAME conv2d + bias (+ leaky-ReLU) (+ 2x2 max-pool) in torch CPU float64 (full-size layers in seconds).
abs_bound     a float64 upper bound, per conv output, on every partial sum a kernel of the given kind forms: the direct sum, or
              the Winograd transform-domain sums sum_c (|G||g||G^T|) .* (|B^T||d||B|) and their output transform.
exact_data    small-integer inputs, weights that are multiples of the common denominator D of G (x) G and integer biases: every
              value every kernel forms is then an integer (a multiple of 2^-8 for F(4x4,4x4)); as long as abs_bound stays
              below 2^24 (scaled by that grid) float32 holds all of them exactly and the result must equal the reference BIT FOR BIT,
              whatever the tiling, channel split or summation order.
rho           max |y - r| / (u abs_bound), u = 2^-24: the error of a non-exact run in units of the rounding of its partial sums.
conv_ref_f16  the same layer in the half-precision trunks' arithmetic: operands rounded to half (nearest even), float64 sums, the
              result rounded to half (unless out_f32); first_block_ref_f16 chains conv1_1 and the pooled conv1_2.
exact_data_f16  integer data on which a half-precision layer must equal conv_ref_f16 bit for bit: partial sums below 2^24 and
              pre-activations within +-1024, where every integer y and every half(0.01f y) is its own half (neg_slope_halves_distinct).
gate_f16      the tolerance of a half-precision run on non-integer data: half a half-spacing + the float32 sums' rho gate.

The transform matrices restate the kernels': F(2x2,3x3) conv_wino.hip / conv_wino2.hip (B^T at the input transform, A^T in the
epilogue, G in wino_pack_weights); F(4x4,3x3) wino4_shared.h (w4_bt_t, w4_at_t) and wino4_pack_weights / wino4s_pack_weights; F(4x4,4x4)
conv_wino7.hip (w7_bt, w7_at, wino7_pack_weights).  A 7x7 filter runs on F(4x4,3x3) / F(2x2,3x3) as nine 3x3 blocks of the filter
zero-extended to 9x9 and on F(4x4,4x4) as four 4x4 blocks of it zero-extended to 8x8; the blocks' transform-domain sums share one
accumulator and one output transform.
"""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                       # unit roundoff of float32
LEAKY = np.float32(0.01)               # HP3D_LEAKY_SLOPE

torch.set_num_threads(min(16, torch.get_num_threads()))

_H = Fraction(1, 2)
WINO = {
    'wino2': dict(m=2, r=3,
                  BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
                  G=[[1, 0, 0], [_H, _H, _H], [_H, -_H, _H], [0, 0, 1]],
                  AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    'wino4': dict(m=4, r=3,
                  BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                      [0, 4, 0, -5, 0, 1]],
                  G=[[Fraction(1, 4), 0, 0], [Fraction(-1, 6)] * 3, [Fraction(-1, 6), Fraction(1, 6), Fraction(-1, 6)],
                     [Fraction(1, 24), Fraction(1, 12), Fraction(1, 6)], [Fraction(1, 24), Fraction(-1, 12), Fraction(1, 6)], [0, 0, 1]],
                  AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
    'wino7': dict(m=4, r=4,
                  BT=[[-2, 4, Fraction(5, 2), -5, -_H, 1, 0], [0, 2, -2, Fraction(-9, 2), _H, 1, 0],
                      [0, -2, 6, Fraction(-7, 2), Fraction(-3, 2), 1, 0], [0, 1, Fraction(-3, 2), -2, Fraction(3, 2), 1, 0],
                      [0, -1, Fraction(5, 2), 0, Fraction(-5, 2), 1, 0], [0, 4, 0, -5, 0, 1, 0], [0, -2, 4, Fraction(5, 2), -5, -_H, 1]],
                  G=[[-_H, 0, 0, 0], [Fraction(-1, 3)] * 4, [Fraction(1, 9), Fraction(-1, 9), Fraction(1, 9), Fraction(-1, 9)],
                     [Fraction(1, 36), Fraction(1, 18), Fraction(1, 9), Fraction(2, 9)],
                     [Fraction(-1, 60), Fraction(1, 30), Fraction(-1, 15), Fraction(2, 15)],
                     [Fraction(32, 45), Fraction(16, 45), Fraction(8, 45), Fraction(4, 45)], [0, 0, 0, 1]],
                  AT=[[1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, _H, 0], [0, 1, 1, 4, 4, Fraction(1, 4), 0],
                      [0, 1, -1, 8, -8, Fraction(1, 8), 1]]),
}
KINDS = ('direct', 'wino2', 'wino4', 'wino4s', 'wino7')


def _spec(kind):
    return WINO['wino4' if kind == 'wino4s' else kind]


def mat(kind, name):
    """A transform matrix of `kind` ('BT', 'G', 'AT') as float64 (all entries are exact binary fractions or rounded once)."""
    return np.array([[float(v) for v in row] for row in _spec(kind)[name]])


def _lcm_den(rows):
    return math.lcm(*[Fraction(v).denominator for row in rows for v in row])


def denominator(kind):
    """D: the least common denominator of G (x) G.  A filter that is a multiple of D has integer transforms G g G^T."""
    return 1 if kind == 'direct' else _lcm_den(_spec(kind)['G']) ** 2


def grid_log2(kind):
    """d: every value of an exact run is a multiple of 2^-d (the power-of-two denominators of B^T on both sides and A^T on both)."""
    if kind == 'direct':
        return 0
    s = _spec(kind)
    return 2 * int(math.log2(_lcm_den(s['BT']))) + 2 * int(math.log2(_lcm_den(s['AT'])))


def blocks(kind, k):
    """The filter blocks a kernel of `kind` runs a k x k filter as: [(row offset, column offset)], block size r."""
    if kind == 'direct':
        return [(0, 0)]
    r = _spec(kind)['r']
    if k == r:
        return [(0, 0)]
    assert (kind, k) in (('wino7', 7), ('wino2', 7), ('wino4', 7), ('wino4s', 7)), (kind, k)
    return [(r * i, r * j) for i in range(-(-k // r)) for j in range(-(-k // r))]


def n_chain(kind, cin, k):
    """Length of the longest accumulation chain behind one output: channels x taps (direct), channels x filter blocks plus the
    depth of the input and output transforms (Winograd)."""
    if kind == 'direct':
        return cin * k * k
    s = _spec(kind)
    return cin * len(blocks(kind, k)) + 2 * (s['m'] + s['r'] - 1)


# --------------------------------------------------------------------------- references
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _pads(n, k, stride):
    o = -(-n // stride)
    p = max((o - 1) * stride + k - n, 0)
    return o, p // 2, p - p // 2


def _conv64(x, w, stride):
    """TF-SAME cross-correlation, NHWC x HWIO -> NHWC, float64 torch tensors (padding as test_oracle_nets_torch.conv_tf_same)."""
    k = w.shape[0]
    _, pt, pb = _pads(x.shape[1], k, stride)
    _, pl, pr = _pads(x.shape[2], k, stride)
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xn, w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)


def _pool2(y):
    B, H, W, C = y.shape
    return y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def conv_ref_f64(x, w, b, stride=1, act=True, pool=False):
    """float64 NHWC reference of hp3d_conv2d.  The activation is the kernels' float32 max(v, 0.01f v) applied to float32(v) wherever
    the float64 pre-activation is a float32 value (an exact run), and max(v, 0.01f v) in float64 elsewhere."""
    with torch.no_grad():
        r = (_conv64(_t(x), _t(w), stride) + _t(b)).numpy()
    if act:
        r32 = r.astype(np.float32)
        if np.array_equal(r32.astype(np.float64), r):
            r = np.maximum(r32, LEAKY * r32).astype(np.float64)
        else:
            r = np.maximum(r, np.float64(LEAKY) * r)
    return _pool2(r) if pool else r


def fc_ref_f64(x, w, b, act):
    r = np.asarray(x, np.float64) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)
    if act:
        r32 = r.astype(np.float32)
        assert np.array_equal(r32.astype(np.float64), r), "fc_ref_f64: exact data only"
        r = np.maximum(r32, LEAKY * r32).astype(np.float64)
    return r


# --------------------------------------------------------------------------- bounds
def _tile_grid(kind, H, W, k):
    """Winograd tile grid of a stride-1 SAME layer: (tiles down, tiles across, top pad, left pad)."""
    m = _spec(kind)['m']
    _, pt, _ = _pads(H, k, 1)
    _, pl, _ = _pads(W, k, 1)
    return -(-H // m), -(-W // m), pt, pl


def _wino_planes(kind, x, w, k, stride, want_vmax=False):
    """Per filter block: |V| bounds [B, C, a, b, ty, tx] and |U| bounds [a, b, C, Cout] (float64 torch), for a stride-1 layer."""
    s = _spec(kind)
    m, r = s['m'], s['r']
    al = m + r - 1
    BT, G = torch.from_numpy(np.abs(mat(kind, 'BT'))), torch.from_numpy(np.abs(mat(kind, 'G')))
    B, H, W, C = x.shape
    ty, tx, pt, pl = _tile_grid(kind, H, W, k)
    nb = -(-k // r)
    # |x| with the SAME pads and room for every window of every block
    xa = F.pad(x.abs().permute(0, 3, 1, 2), (pl, tx * m + al + r * (nb - 1) - W - pl, pt, ty * m + al + r * (nb - 1) - H - pt))
    kern = torch.einsum('ai,bj->abij', BT, BT).reshape(al * al, 1, al, al)
    wk = np.zeros((nb * r, nb * r) + w.shape[2:])
    wk[:k, :k] = np.abs(w.numpy() if isinstance(w, torch.Tensor) else w)
    for (u0, v0) in blocks(kind, k):
        g = torch.from_numpy(wk[u0:u0 + r, v0:v0 + r])                                   # [r, r, C, Cout]
        Ub = torch.einsum('ar,rsco,bs->abco', G, g, G)
        xs = xa[:, :, u0:u0 + (ty - 1) * m + al, v0:v0 + (tx - 1) * m + al].reshape(B * C, 1, (ty - 1) * m + al, (tx - 1) * m + al)
        Vb = F.conv2d(xs, kern, stride=m).reshape(B, C, al, al, ty, tx)
        yield Ub, Vb


def abs_bound(x, w, kind, b=None, stride=1):
    """float64 [B, Ho, Wo, Cout]: a bound on |every partial sum| a kernel of `kind` forms for each conv output (before the pool)."""
    x = _t(x) if not isinstance(x, torch.Tensor) else x
    w = np.asarray(w, np.float64)
    k, Cout = w.shape[0], w.shape[3]
    bb = np.abs(np.asarray(b, np.float64)) if b is not None else np.zeros(Cout)
    with torch.no_grad():
        if kind == 'direct':
            return (_conv64(x.abs(), torch.from_numpy(np.abs(w)), stride) + torch.from_numpy(bb)).numpy()
        assert stride == 1
        s = _spec(kind)
        m = s['m']
        AT = torch.from_numpy(np.abs(mat(kind, 'AT')))
        B, H, W, _ = x.shape
        out = np.empty((B, H, W, Cout))
        for i in range(B):                     # an image at a time: |V| is (alpha/m)^2 x the input
            M = None
            for Ub, Vb in _wino_planes(kind, x[i:i + 1], w, k, stride):
                t = torch.einsum('abco,ncabyx->naboyx', Ub, Vb)
                M = t if M is None else M + t
            Y = torch.einsum('ia,naboyx,jb->nyixjo', AT, M, AT)                            # [1, ty, m, tx, m, Cout]
            ty, tx = Y.shape[1], Y.shape[3]
            out[i] = Y.reshape(ty * m, tx * m, Cout)[:H, :W].numpy()
        return out + bb


def operand_max(x, w, kind):
    """(max |U|, max |V|) over the transformed filters and inputs of a stride-1 Winograd layer (bounds, as in abs_bound)."""
    with torch.no_grad():
        mu = mv = 0.0
        for Ub, Vb in _wino_planes(kind, _t(x), np.asarray(w, np.float64), w.shape[0], 1):
            mu, mv = max(mu, float(Ub.max())), max(mv, float(Vb.max()))
        return mu, mv


def exact_ok(kind, bound, x=None, w=None):
    """The exactness precondition of `kind` on an integer run: every partial sum, on the grid 2^-d, below 2^24; for the split
    bfloat16 kernel (conv_wino4s: six of the nine piece products u_i v_j, i + j <= 2) additionally every transformed operand an
    integer below 2^16, i.e. two bfloat16 pieces: its third pieces are then zero and the three dropped products vanish."""
    ok = float(np.max(bound)) * 2.0 ** grid_log2(kind) < 2.0 ** 24
    if ok and kind == 'wino4s':
        mu, mv = operand_max(x, w, kind)
        ok = mu < 2.0 ** 16 and mv < 2.0 ** 16
    return ok


# --------------------------------------------------------------------------- data
def exact_data(kind, shape, rng, per_out=None, stride=1):
    """Integer x in {-1, 0, 1}, w = D m with m in {-1, 0, 1}, b = D n with n in {-2 .. 2} (float32 arrays) for shape
    (B, H, W, Cin, Cout, k).  m is sparse: about `per_out` non-zero taps per output channel (spread over all channels and taps);
    halved until abs_bound meets the precondition of `kind`.  Returns (x, w, b, bound)."""
    B, H, W, Cin, Cout, k = shape
    D = denominator(kind)
    x = rng.integers(-1, 2, (B, H, W, Cin)).astype(np.float32)
    if per_out is None:
        per_out = {'direct': 4096, 'wino2': 4096, 'wino4': 64, 'wino4s': 64, 'wino7': 1}[kind]
    per_out = min(per_out, k * k * Cin)
    while True:
        p = per_out / (k * k * Cin)
        m = np.where(rng.random((k, k, Cin, Cout)) < p, rng.choice([-1.0, 1.0], (k, k, Cin, Cout)), 0.0)
        w = (D * m).astype(np.float32)
        b = (D * rng.integers(-2, 3, Cout)).astype(np.float32)
        bound = abs_bound(x, w, kind, b, stride)
        if exact_ok(kind, bound, x, w) or per_out <= 1:
            return x, w, b, bound
        per_out //= 2


def realistic_input(shape, rng, zeros=0.0):
    """What a trunk layer is fed: leaky_relu(N(0.5, 1)) per value, x 2^U(-4, 4) per channel, a fraction `zeros` of it zero."""
    B, H, W, C = shape
    v = rng.normal(0.5, 1.0, shape)
    v = np.maximum(v, 0.01 * v) * 2.0 ** rng.uniform(-4, 4, C)
    if zeros:
        v[rng.random(shape) < zeros] = 0.0
    return v.astype(np.float32)


# rho gate: rho <= RHO_LAMBDA sqrt(n).  Fixed before any GPU run from this module's float32 restatement (wino_f32) of every Winograd
# form on realistic_input data: correct arithmetic measures rho <= 0.75 at n >= 44 (RHO_LAMBDA sqrt(44) = 1.66, a 2x margin that
# grows with sqrt(n)); bfloat16 x2 operands or one filter plane off by 2^-16 measure rho >= 2.4 at n <= 156 (tests/test_conv_exact.py).
RHO_LAMBDA = 0.25


def rho_gate(kind, cin, k):
    return RHO_LAMBDA * math.sqrt(n_chain(kind, cin, k))


def exact_mismatch(y, r):
    """Outputs of y (float32) that are not bit-equal to the float64 reference r."""
    return int(np.count_nonzero(np.asarray(y, np.float32).astype(np.float64) != r)) + (0 if np.shape(y) == np.shape(r) else -1)


def pool_bound(bound):
    """The bound behind a pooled output: the largest of its 2x2 window's."""
    return _pool2(bound)


def rho(y, r, bound):
    """max |y - r| / (u bound): the error in units of the float32 rounding of the largest partial sum behind each output."""
    return float(np.max(np.abs(np.asarray(y, np.float64) - r) / (U32 * np.maximum(bound, 1e-300))))


# --------------------------------------------------------------------------- a float32 restatement (the checks' own tests)
def _bf16_pieces(v, n):
    """v (float32) as the sum of n round-to-nearest bfloat16 pieces (w4s_split3 with n = 3)."""
    out, rest = [], v.astype(np.float32)
    for _ in range(n):
        p = _bf16_rne(rest)
        out.append(p)
        rest = (rest - p).astype(np.float32)
    return out


def _bf16_rne(v):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def wino_f32(x, w, b, kind, act=True, pieces=None, u_scale=None, track=None):
    """NumPy float32 restatement of a stride-1 Winograd layer of `kind`: U = G g G^T in float64 rounded once, V = B^T d B and
    Y = A^T M A in float32, M accumulated channel by channel (block by block) in float32.  pieces = n: products over n bfloat16
    pieces per operand with the products i + j < n (conv_wino4s: n = 3); u_scale: [a, b] factors applied to U (a filter
    constant off).  track: a list that receives max |partial sum| per output [H, W, Cout] (V, M after each channel, Y)."""
    s = _spec(kind)
    m, r = s['m'], s['r']
    al = m + r - 1
    BT, G, AT = mat(kind, 'BT').astype(np.float32), mat(kind, 'G'), mat(kind, 'AT').astype(np.float32)
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float64)
    B, H, W, C = x.shape
    k, Cout = w.shape[0], w.shape[3]
    ty, tx, pt, pl = _tile_grid(kind, H, W, k)
    nb = -(-k // r)
    xp = np.zeros((B, ty * m + al + r * (nb - 1), tx * m + al + r * (nb - 1), C), np.float32)
    xp[:, pt:pt + H, pl:pl + W] = x
    wk = np.zeros((nb * r, nb * r, C, Cout))
    wk[:k, :k] = w
    M = np.zeros((al, al, B, ty, tx, Cout), np.float32)
    big = np.zeros((B, ty, tx, Cout))
    for (u0, v0) in blocks(kind, k):
        Ub = np.einsum('ar,rsco,bs->abco', G, wk[u0:u0 + r, v0:v0 + r], G)
        if u_scale is not None:
            Ub = Ub * u_scale[:, :, None, None]
        Ub = Ub.astype(np.float32)
        # windows [B, ty, tx, al, al, C]
        idx_y = u0 + m * np.arange(ty)[:, None] + np.arange(al)[None, :]
        idx_x = v0 + m * np.arange(tx)[:, None] + np.arange(al)[None, :]
        d = xp[:, idx_y][:, :, :, idx_x]                                  # [B, ty, al, tx, al, C]
        d = d.transpose(0, 1, 3, 2, 4, 5)
        V = np.einsum('ai,nyxijc->anyxjc', BT, d).astype(np.float32)     # rows (float32 sums of <= 7 terms, as the kernels)
        V = np.einsum('bj,anyxjc->abnyxc', BT, V).astype(np.float32)
        for c in range(C):
            Uc, Vc = Ub[:, :, c, :], V[:, :, :, :, :, c]
            if pieces:
                up, vp = _bf16_pieces(Uc, pieces), _bf16_pieces(Vc, pieces)
                for i in range(pieces):
                    for j in range(pieces - i):
                        M = (M + vp[j][..., None] * up[i][:, :, None, None, None, :]).astype(np.float32)
            else:
                M = (M + Vc[..., None] * Uc[:, :, None, None, None, :]).astype(np.float32)
            if track is not None:
                big = np.maximum(big, np.abs(M).max(axis=(0, 1)))
    Y = np.einsum('ia,abnyxo->ibnyxo', AT, M).astype(np.float32)
    Y = np.einsum('jb,ibnyxo->nyixjo', AT, Y).astype(np.float32)
    Y = Y.reshape(B, ty * m, tx * m, Cout)[:, :H, :W]
    if track is not None:
        track.append(np.repeat(np.repeat(big, m, 1), m, 2)[:, :H, :W])
    y = (Y + np.asarray(b, np.float32)).astype(np.float32)
    return np.maximum(y, LEAKY * y) if act else y


# --------------------------------------------------------------------------- half precision (conv_h16.hip, the F16 forms of conv_mfma.hip / conv_first.hip)
U16 = 2.0 ** -11                       # unit roundoff of half
HALF_EXACT_MAX = 1024                  # |pre-activation| of an exact half-precision run (every integer up to 2048 is a half)


def _h(a):
    """Round to half, to nearest even (what cvt_channels_f16_kernel, pack_conv16 and the epilogues' (hp3d_f16) casts do), as float64."""
    return np.asarray(a).astype(np.float16).astype(np.float64)


def pre_f16(x, w, b, stride=1):
    """float64 pre-activation of a half-precision layer: half(x) * half(w) summed in float64, + the float32 bias."""
    with torch.no_grad():
        return (_conv64(_t(_h(x)), _t(_h(w)), stride) + _t(b)).numpy()


def conv_ref_f16(x, w, b, stride=1, act=True, pool=False, out_f32=False, first=False, pre=None):
    """float64-valued NHWC reference of hp3d_conv2d_f16: pre_f16, the activation as conv_ref_f64 applies it (the kernels' float32
    max(v, 0.01f v) on float32(v) wherever the pre-activation is a float32 value -- an exact run --, in float64 elsewhere), ONE rounding
    to half (nearest even, sub-normals kept) unless out_f32, then the 2x2 max-pool (rounding is monotone: the kernels that pool
    before they round give the same).  first: the layer is conv1_1 (raw float32 image, 3 -> 64, k = 3) -- the same arithmetic here; the
    kernel's own extra rounding of that layer (its bias rides through the half MFMA) is gate_f16's term, not the reference's.
    pre: pre_f16(x, w, b, stride) if the caller has it."""
    if first:
        assert w.shape == (3, 3, 3, 64) and stride == 1 and not out_f32
    r = pre_f16(x, w, b, stride) if pre is None else pre
    if act:
        r32 = r.astype(np.float32)
        if np.array_equal(r32.astype(np.float64), r):
            r = np.maximum(r32, LEAKY * r32).astype(np.float64)
        else:
            r = np.maximum(r, np.float64(LEAKY) * r)
    if not out_f32:
        r = _h(r)
    return _pool2(r) if pool else r


def first_block_ref_f16(image, w1, b1, w2, b2):
    """conv1_1 + conv1_2 + 2x2 max-pool of a half-precision trunk: conv1_1's half output is conv1_2's input, and conv1_2's SAME
    padding pads that OUTPUT with zeros.  Returns (reference [B, H/2, W/2, 64], conv1_1's output)."""
    y1 = conv_ref_f16(image, w1, b1, first=True)
    return conv_ref_f16(y1, w2, b2, pool=True), y1


def neg_slope_halves_distinct(lo=-1600):
    """half(0.01f y), y = lo .. 0 as the kernels form it (float32 product, then nearest-even half): True if pairwise distinct."""
    y = np.arange(lo, 1, dtype=np.float32)
    h = (LEAKY * y).astype(np.float16)
    return len(np.unique(h.view(np.uint16))) == len(y)


def exact_data_f16(shape, rng, density=1.0, xmax=2, bmax=8):
    """Integer x in {-xmax .. xmax}, w in {-1, 0, 1} with a fraction `density` non-zero, integer b in {-bmax .. bmax} (float32
    arrays) for shape (B, H, W, Cin, Cout, k).  Returns (x, w, b, bound), bound = abs_bound('direct').  The caller asserts
    exact_ok_f16 on it: data are not thinned here to meet it."""
    B, H, W, Cin, Cout, k = shape
    x = rng.integers(-xmax, xmax + 1, (B, H, W, Cin)).astype(np.float32)
    w = np.where(rng.random((k, k, Cin, Cout)) < density, rng.choice([-1.0, 1.0], (k, k, Cin, Cout)), 0.0).astype(np.float32)
    b = rng.integers(-bmax, bmax + 1, Cout).astype(np.float32)
    return x, w, b, abs_bound(x, w, 'direct', b)


def first_block_data_f16(shape, rng, density2=0.125):
    """(B, H, W): image in {0, 1}, w1 dense in {-1, 0, 1}, b1 = 27 (conv1_1's output is then an integer in 0 .. 54 and its
    leaky-ReLU the identity), w2 in {-1, 0, 1} at `density2`, integer b2 in {-8 .. 8}."""
    B, H, W = shape
    image = rng.integers(0, 2, (B, H, W, 3)).astype(np.float32)
    w1 = rng.choice([-1.0, 0.0, 1.0], (3, 3, 3, 64)).astype(np.float32)
    b1 = np.full(64, 27, np.float32)
    w2 = np.where(rng.random((3, 3, 64, 64)) < density2, rng.choice([-1.0, 1.0], (3, 3, 64, 64)), 0.0).astype(np.float32)
    b2 = rng.integers(-8, 9, 64).astype(np.float32)
    return image, w1, b1, w2, b2


def exact_ok_f16(bound, pre):
    """The preconditions of an exact half-precision run: (a) every partial sum below 2^24 (float32 holds it), (b) every
    pre-activation an integer within +-HALF_EXACT_MAX -- y >= 0 is then its own half and half(0.01f y) tells any two y < 0 apart
    (neg_slope_halves_distinct), so a sum that is off by one changes the stored half."""
    return bool(float(np.max(bound)) < 2.0 ** 24 and float(np.max(np.abs(pre))) <= HALF_EXACT_MAX and np.array_equal(pre, np.round(pre)))


def spacing_half(v):
    """Distance between neighbouring halves at |v| (2^-24 in the sub-normal range)."""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def first_bias_term(b):
    """conv_first_kernel<true> / the fused forms' patch stage carry conv1_1's float32 bias through the half MFMA as two rows, hi =
    half(b) and half(b - hi) (operand 1.0 each).  b - hi is exact in float32 and at most 2^-11 |b|; its own rounding to half errs by
    at most 2^-11 of that, or by half a sub-normal spacing where it falls below 2^-14: 2^-22 |b| + 2^-25 per output channel."""
    return 2.0 ** -22 * np.abs(np.asarray(b, np.float64)) + 2.0 ** -25


def gate_f16(y, r, bound, cin, k, out_f32=False, first_b=None):
    """Per-output tolerance of a half-precision run y against r = conv_ref_f16(..., out_f32=True) (the UNROUNDED reference; pooled
    like y, `bound` through pool_bound):  1/2 spacing_half(max(|y|, |r|))   the one nearest-even rounding of the stored half
                                          + rho_gate('direct') u32 bound     the float32 sums of exact half products
                                          (+ first_bias_term(first_b))       conv1_1 on conv_first.hip.
    A truncating epilogue errs by up to a whole spacing, flushed sub-normals by up to 2^-14 against a spacing of 2^-24."""
    tol = rho_gate('direct', cin, k) * U32 * np.asarray(bound, np.float64)
    if not out_f32:
        tol = tol + 0.5 * spacing_half(np.maximum(np.abs(np.asarray(y, np.float64)), np.abs(r)))
    if first_b is not None:
        tol = tol + first_bias_term(first_b)
    return tol


def rho_f16(y, r, bound, out_f32=False, first_b=None):
    """The measured rho of a half-precision run: what is left of |y - r| after the half rounding's (and conv1_1's bias rows') share,
    in units of u32 bound."""
    err = np.abs(np.asarray(y, np.float64) - r)
    if not out_f32:
        err = err - 0.5 * spacing_half(np.maximum(np.abs(np.asarray(y, np.float64)), np.abs(r)))
    if first_b is not None:
        err = err - first_bias_term(first_b)
    return float(np.max(np.maximum(err, 0.0) / (U32 * np.maximum(bound, 1e-300))))


def half_trunc(v):
    """v rounded to half TOWARDS ZERO (the wrong rounding mode the checks must see), as float64."""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)
