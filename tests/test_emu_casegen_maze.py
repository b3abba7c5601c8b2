"""CPU: gnnpp_casegen_maze (csrc/casegen_maze_kernels.hip), compiled unmodified for the host emulation, on the shared case
table of tests/casegen_maze_cases.py: maps and word counts equal the reference-made fixture exactly, on poisoned outputs with
a guard row behind them; the repository's own restatement equals the same fixture (so it may stand in where the fixture has
no entry); seeds as an array and seed0 + c give the same bytes; two calls give the same bytes; the documented error codes
with nothing written.  Two one-off mutants of the restatement show that named cases can tell a wrong walk.
tests/test_gpu_casegen_maze_cases.py runs the same table on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_maze_cases as mz  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED  # noqa: E402

needs_clang = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                 reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def call(lib, C, H, W, walls, steps, seed0=0, seeds=None, expect=0, dims=None, null_grid=False, want_words=True,
         offset=0):
    """One call on host arrays: the maps poisoned, one guard map behind them, `offset` bytes in front (the map's first byte
    then sits off a 16-byte boundary).  dims: (C, H, W, walls, steps) the call is TOLD."""
    buf = np.full(offset + (C + 1) * H * W, mz.POISON, np.uint8)
    words = np.full(C + 1, -7, np.int32)
    s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    tC, tH, tW, tw, ts = dims or (C, H, W, walls, steps)
    rc = lib.gnnpp_casegen_maze(None if s is None else s.ctypes.data, int(seed0) & 0xffffffff, tC, tH, tW, tw, ts,
                                None if null_grid else buf.ctypes.data + offset,
                                words.ctypes.data if want_words else None, None)
    assert rc == expect, rc
    maps = buf[offset:].reshape(C + 1, H, W)
    assert (buf[:offset] == mz.POISON).all() and (maps[C] == mz.POISON).all() and words[C] == -7   # nothing outside
    return maps[:C], words[:C]


def run_case(lib, name, **kw):
    case = mz.TABLE[name]
    walls, steps = mz.counts_of(case['H'], case['W'], case['density'], case['complexity'])
    if 'seeds' in case:
        kw = dict(kw, seeds=case['seeds'])
    else:
        kw = dict(kw, seed0=case['seed0'])
    return call(lib, case['C'], case['H'], case['W'], walls, steps, **kw)


@pytest.mark.parametrize('name', mz.NAMES)
def test_the_restatement_equals_the_fixture(name):
    maps, words = mz.restate(mz.TABLE[name])
    mz.assert_equal_to_golden(name, maps, words)


@needs_clang
@pytest.mark.parametrize('name', mz.NAMES)
def test_named_cases_equal_the_fixture(lib, name):
    maps, words = run_case(lib, name)
    assert set(np.unique(maps).tolist()) <= {0, 1}           # every byte was written
    mz.assert_equal_to_golden(name, maps, words)


def test_the_table_holds_what_it_is_for():
    """The facts the cases were chosen for, read off the fixture."""
    g = {n: mz.golden(n) for n in mz.NAMES}
    assert (g['side_3x3'][1] == 0).all() and g['side_3x3'][0].any()          # walls, and not one word
    assert (g['no_walls_20x20'][1] == 0).all() and not g['no_walls_20x20'][0].any()
    dots = g['no_steps_20x20'][0]
    assert dots.any() and not dots[:, 1::2, :].any() and not dots[:, :, 1::2].any()      # lattice cells only
    assert ((g['second_refill_21x13'][1] > 624) & (g['second_refill_21x13'][1] < 2 * 624)).all()
    assert (g['many_refills_64x48'][1] > 4 * 624).all() and g['limit_256x256'][1][0] > 80 * 624
    assert g['seed_wraps_to_zero'][2].tolist() == [2 ** 32 - 1, 0]
    assert {0, 1337, 2 ** 32 - 1} <= set(g['explicit_seeds'][2].tolist())
    assert any(mz.TABLE[n]['C'] % 4 for n in mz.NAMES) and any(mz.TABLE[n]['C'] > 4 for n in mz.NAMES)
    assert mz.counts_of(20, 20, 0.1, 0.01) == (10, 2)


@needs_clang
def test_seed_array_and_seed0_agree_and_bytes_repeat(lib):
    case = mz.TABLE['reference_20x20']
    a = run_case(lib, 'reference_20x20')
    b = call(lib, 6, 20, 20, 10, 2, seeds=mz.seeds_of(case))
    c = run_case(lib, 'reference_20x20')
    for x, y in ((a, b), (a, c)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    # a map depends on its seed alone: case 1 of the wrapped pair is seed 0, and so is case 1 of the explicit seeds
    wrap = mz.restate(dict(mz.TABLE['seed_wraps_to_zero'], seed0=0, C=1))
    assert np.array_equal(mz.golden('seed_wraps_to_zero')[0][1], wrap[0][0])


@needs_clang
def test_words_may_be_null_and_the_map_may_start_off_a_boundary(lib):
    for offset in (0, 1, 7, 15):
        maps, words = run_case(lib, 'odd_5x7', offset=offset, want_words=False)
        mz.assert_equal_to_golden('odd_5x7', maps, mz.golden('odd_5x7')[1])
        assert (words == -7).all()
        maps, words = run_case(lib, 'wide_5x70', offset=offset)
        mz.assert_equal_to_golden('wide_5x70', maps, words)


@needs_clang
def test_a_shape_outside_the_fixture_equals_the_restatement(lib):
    case = dict(C=7, H=9, W=130, density=0.4, complexity=0.03, seed0=2 ** 32 - 3)
    walls, steps = mz.counts_of(9, 130, 0.4, 0.03)
    maps, words = call(lib, 7, 9, 130, walls, steps, seed0=case['seed0'])
    want_maps, want_words = mz.restate(case)
    assert np.array_equal(maps, want_maps) and np.array_equal(words, want_words) and (words > 624).all()


@needs_clang
def test_argument_errors_leave_the_outputs_untouched(lib):
    maps, words = call(lib, 1, 4, 4, 1, 1)
    assert words.tolist() == [mz.maze_map(4, 4, 1, 1, 0)[1]]
    for kw, code in ((dict(null_grid=True), ERR_ARG), (dict(dims=(0, 4, 4, 1, 1)), ERR_ARG),
                     (dict(dims=(1, 2, 4, 1, 1)), ERR_ARG), (dict(dims=(1, 4, 2, 1, 1)), ERR_ARG),
                     (dict(dims=(1, 4, 4, -1, 1)), ERR_ARG), (dict(dims=(1, 4, 4, 1, -1)), ERR_ARG),
                     (dict(dims=(1, 4, 4, 2 ** 16, 2 ** 15)), ERR_ARG),
                     (dict(dims=(1, 257, 4, 1, 1)), ERR_UNSUPPORTED), (dict(dims=(1, 4, 257, 1, 1)), ERR_UNSUPPORTED),
                     # the sizes are refused before the map size is looked at
                     (dict(dims=(0, 257, 4, 1, 1)), ERR_ARG), (dict(dims=(1, 257, 2, 1, 1)), ERR_ARG),
                     (dict(dims=(1, 257, 4, -1, 1)), ERR_ARG), (dict(dims=(1, 257, 257, 1, 1), null_grid=True), ERR_ARG)):
        maps, words = call(lib, 1, 4, 4, 1, 1, expect=code, **kw)
        assert (maps == mz.POISON).all() and (words == -7).all(), kw             # nothing enqueued


# ---- the two mutants: a wrong walk, made in the harness; named cases must tell ------------------------------------------
def _differs(name, mutant):
    maps, words = mz.restate(mz.TABLE[name], mutant)
    want_maps, want_words, _ = mz.golden(name)
    return bool((maps != want_maps).any() or (words != want_words).any())


def test_mutant_randint_with_inclusive_high():
    """One-off mutant: the neighbour pick may take the LAST entry of the list (randint with an inclusive high end).  A
    list of two then draws a word, so even the 3 x 3 map -- no word at all in the reference -- tells; so do the reference's
    own setting and the steps of the odd shapes.  Maps without a step cannot tell, and do not."""
    for name in ('side_3x3', 'side_4x4', 'odd_5x7', 'reference_20x20', 'second_refill_21x13'):
        assert _differs(name, 'inclusive_high'), name
    assert not _differs('no_steps_20x20', 'inclusive_high') and not _differs('no_walls_20x20', 'inclusive_high')


def test_mutant_row_drawn_before_the_column():
    """One-off mutant: y drawn before x.  The odd, non-square shapes and the reference's own setting tell; a map whose
    column needs no word and whose row does (W // 2 == 1 on 3 x 3: neither) cannot."""
    for name in ('odd_5x7', 'odd_21x13', 'reference_20x20', 'no_steps_20x20', 'wide_5x70', 'tall_70x5'):
        assert _differs(name, 'y_before_x'), name
    assert not _differs('side_3x3', 'y_before_x')
