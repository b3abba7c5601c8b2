"""MI355X: gnnpp_casegen_maze on the shared case table of tests/casegen_maze_cases.py, through casegen.enqueue_maze_maps on
poisoned device buffers with a guard map behind them: maps and word counts equal the reference-made fixture exactly.
tests/test_emu_casegen_maze.py runs the same table under the host emulation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_maze_cases as mz  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def casegen():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, casegen as m
    _native.lib()
    return m


def run(casegen, case, offset=0):
    """-> (maps, words) on the host.  offset: bytes in front of the first map (it then sits off a 16-byte boundary)."""
    C, H, W = case['C'], case['H'], case['W']
    buf = torch.full((offset + (C + 1) * H * W,), mz.POISON, dtype=torch.uint8, device=DEV)
    words = torch.full((C + 1,), -7, dtype=torch.int32, device=DEV)
    out = buf[offset:offset + C * H * W].view(C, H, W)
    seeds = None
    if 'seeds' in case:
        seeds = torch.from_numpy(mz.seeds_of(case).view(np.int32)).to(DEV)
    casegen.enqueue_maze_maps(out, case['density'], case['complexity'], seed=case.get('seed0', 0), seeds=seeds,
                              words=words[:C])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == mz.POISON).all() and (host[offset + C * H * W:] == mz.POISON).all()   # nothing outside
    assert int(words[C]) == -7
    return host[offset:offset + C * H * W].reshape(C, H, W), words[:C].cpu().numpy()


@pytest.mark.parametrize('name', mz.NAMES)
def test_named_cases_equal_the_fixture(casegen, name):
    maps, words = run(casegen, mz.TABLE[name])
    assert set(np.unique(maps).tolist()) <= {0, 1}           # every byte was written
    mz.assert_equal_to_golden(name, maps, words)


@pytest.mark.parametrize('offset', [1, 7, 15])
def test_maps_off_a_16_byte_boundary(casegen, offset):
    for name in ('odd_5x7', 'wide_5x70'):
        maps, words = run(casegen, mz.TABLE[name], offset=offset)
        mz.assert_equal_to_golden(name, maps, words)


def test_seed_array_and_seed0_agree(casegen):
    case = mz.TABLE['reference_20x20']
    a = run(casegen, case)
    b = run(casegen, dict({k: v for k, v in case.items() if k != 'seed0'}, seeds=mz.seeds_of(case).tolist()))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_shape_outside_the_fixture_equals_the_restatement(casegen):
    """37 maps (ten workgroups, one wave in the last) of 9 x 130 from seeds around the wrap."""
    case = dict(C=37, H=9, W=130, density=0.4, complexity=0.03, seed0=2 ** 32 - 3)
    maps, words = run(casegen, case)
    want_maps, want_words = mz.restate(case)
    assert np.array_equal(maps, want_maps) and np.array_equal(words, want_words) and (words > 624).all()
