"""conv_wino4.hip's window addresses on the device: the shapes of tests/test_emu_wino4_addr.py (one tile, border tile columns only,
interior columns, ragged widths and heights, tiles beyond the batch, tail pieces, the channel split) and two trunk-like layers whose
column term (a pixel's channels x 4 bytes x 0..3) is 256 B ... 768 B and 1 KB ... 3 KB.  Integer data, bit-equal to the float64
reference of oracle/conv_exact.py; two calls bit-identical; the launch counters show conv_wino4 and its path."""
import pytest

from tests import test_gpu_conv_exact as G

pytestmark = pytest.mark.gpu

CASES = [
    ('wino4', (1, 4, 4, 16, 64), 0, None),
    ('wino4', (1, 8, 8, 16, 64), 0, None),
    ('wino4', (2, 12, 16, 32, 64), 1, None),
    ('wino4', (1, 6, 10, 16, 64), 0, None),
    ('wino4', (1, 7, 9, 16, 64), 0, None),
    ('wino4', (1, 6, 8, 16, 64), 0, None),
    ('wino4', (3, 8, 8, 16, 128), 0, None),
    ('wino4_nosplit', (1, 16, 32, 128, 256), 0, 'conv_wino4_tail_launches'),      # 4 items of 8 steps: all of them tail pieces
    ('wino4_nosplit', (1, 16, 32, 64, 128), 1, 'conv_wino4_tail_launches'),
    ('wino4', (1, 8, 8, 64, 64), 0, 'conv_splitk_reduce_launches'),
    ('wino4_nosplit', (2, 40, 40, 64, 64), 1, None),
    ('wino4_nosplit', (2, 32, 32, 256, 256), 0, None),
    ('wino4', (2, 32, 32, 256, 256), 0, 'conv_splitk_reduce_launches'),
]


@pytest.mark.parametrize("form,shape,pool,path", CASES, ids=lambda v: v if isinstance(v, str) else str(v))
def test_window_addresses_on_device(gpu_engine, form, shape, pool, path):
    d = G.exact_case(gpu_engine, form, shape + (3,), 1, bool(pool))
    if path is not None:
        assert d[path] == 2, d            # (both calls)
    elif form == 'wino4':
        assert not any(d[c] for c in G.PATH_COUNTERS), d
