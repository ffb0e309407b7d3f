"""conv_wino4.hip's window addresses on the CPU interpreter of the kernel sources (tests/emu, which range-checks a buffer access on its
vector offset like the hardware): where the image width is a multiple of 4 a 3x3 launch keeps its row offsets once per column class
(column 0 | columns 1..4 | column 5; a class whose column lies outside the image carries the out-of-range constant) and the rest of
the column rides in the load's scalar offset; any other width keeps the row + column terms added per step.  Every case runs through
hp3d_conv2d with conv_wino4 forced, on integer data whose every partial sum float32 holds exactly: the result must equal
oracle/conv_exact.py's float64 reference bit for bit, two calls must agree, the launch counter must show conv_wino4 (and no other
conv kernel), and no load may have left its buffer through the scalar offset."""
import pytest

from tests import test_gpu_conv_exact as G

# (form, (B, H, W, Cin, Cout), pool, the path counter that must move or None)
CASES = [
    ('wino4', (1, 4, 4, 16, 64), 0, None),                  # one tile: column 0 and column 5 outside at once
    ('wino4', (1, 8, 8, 16, 64), 0, None),                  # a left and a right tile column, no interior
    ('wino4', (2, 12, 16, 32, 64), 1, None),                # interior tile columns, pooled, two steps, a tile block across two images
    ('wino4', (1, 6, 10, 16, 64), 0, None),                 # ragged widths: the row + column form
    ('wino4', (1, 7, 9, 16, 64), 0, None),
    ('wino4', (1, 6, 8, 16, 64), 0, None),                  # ragged height under a width that is a multiple of 4
    ('wino4', (3, 8, 8, 16, 128), 0, None),                 # tiles beyond the batch in the last item, two cout blocks
    ('wino4_nosplit', (1, 16, 32, 128, 256), 0, 'conv_wino4_tail_launches'),      # 4 items on 3 CUs: the last one as tail pieces
    ('wino4_nosplit', (1, 16, 32, 64, 128), 1, 'conv_wino4_tail_launches'),       # ... pooled, less than one round
    ('wino4', (1, 8, 8, 64, 64), 0, 'conv_splitk_reduce_launches'),               # one item of four steps: split over the channels
]


@pytest.mark.parametrize("form,shape,pool,path", CASES, ids=lambda v: v if isinstance(v, str) else str(v))
def test_window_addresses_on_interpreter(emu_engine, form, shape, pool, path):
    o0 = emu_engine.counter('emu_soff_overreads')
    d = G.exact_case(emu_engine, form, shape + (3,), 1, bool(pool))
    assert emu_engine.counter('emu_soff_overreads') == o0, "a load left its buffer through the scalar offset"
    if path is not None:
        assert d[path] == 2, d            # (both calls)
    else:
        assert not any(d[c] for c in G.PATH_COUNTERS), d
