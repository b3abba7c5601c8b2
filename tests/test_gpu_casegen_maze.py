"""MI355X: the maze maps through the public interface.  casegen.maze_maps gives the same bytes twice and the restatement's
maps; generate(maps='maze') gives cases whose grid is the raw maze plus the closure only, whose agents share one region,
and whose yaml parses; generate() without the new keywords is byte for byte gnnpp_casegen called directly; one maze launch
replayed from a HIP graph equals the eager call; the refusals, each matched by its word."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_cases as cc  # noqa: E402
import casegen_maze_cases as mz  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def casegen():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, casegen as m
    _native.lib()
    return m


def test_maze_maps_twice_the_same_bytes_and_the_reference_setting(casegen):
    a = casegen.maze_maps(6, 20, 20, DEV, seed=1337)
    b = casegen.maze_maps(6, 20, 20, DEV, seed=1337)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (6, 20, 20) and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), mz.golden('reference_20x20')[0])        # the defaults are 0.1 / 0.01
    case = mz.TABLE['explicit_seeds']
    for seeds in (case['seeds'], np.asarray(case['seeds'], dtype=np.int64), torch.tensor(case['seeds'], dtype=torch.int64)):
        got = casegen.maze_maps(5, 10, 12, DEV, density=case['density'], complexity=case['complexity'], seeds=seeds)
        assert np.array_equal(got.cpu().numpy(), mz.golden('explicit_seeds')[0])
    other = casegen.maze_maps(6, 20, 20, DEV, seed=1338)
    assert torch.equal(other[:5], a[1:])                     # a map depends on its seed alone


def test_generate_on_maze_maps(casegen):
    """16 cases of 10 agents on the reference's 20 x 20 setting at a density that cuts regions off."""
    import yaml
    from gnn_pathplanning_amd import mapf
    C, N, H, W, density, complexity, seed = 16, 10, 20, 20, 0.4, 0.05, 1337
    got = casegen.generate(C, N, H, W, DEV, density=density, seed=seed, maps='maze', complexity=complexity)
    raw = casegen.maze_maps(C, H, W, DEV, density=density, complexity=complexity, seed=seed)
    want_raw, _ = mz.restate(dict(C=C, H=H, W=W, density=density, complexity=complexity, seed0=seed))
    assert np.array_equal(raw.cpu().numpy(), want_raw) and torch.equal(got.raw, raw)
    assert bool(got.ok.all())
    grid = got.grid.cpu().numpy()
    assert (grid[want_raw == 1] == 1).all()                  # no wall of the raw maze was removed
    # ... and what was added is the closure: the yardstick's closure of the raw maze, cell for cell
    want = cc.generate(C, N, H, W, 0, seed, grids=want_raw)
    for k in cc.OUTPUTS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    assert (grid != want_raw).any()                          # (the setting does cut cells off: the closure had work)
    d = mapf.distances(got.grid, got.start, got.goal, DEV)
    assert int(d.dist.min()) >= 1                            # starts and goals in one region
    doc = yaml.safe_load(got.yaml(3))
    assert doc['map']['dimensions'] == [H, W] and len(doc['map']['obstacles']) == int(got.grid[3].sum())
    assert [a['start'] for a in doc['agents']] == got.start[3].tolist()
    assert [a['goal'] for a in doc['agents']] == got.goal[3].tolist()


def test_generate_without_the_new_keywords_is_gnnpp_casegen(casegen):
    from gnn_pathplanning_amd import _native
    C, N, H, W, seed = 8, 10, 20, 20, 13
    got = casegen.generate(C, N, H, W, DEV, density=0.1, seed=seed)
    assert not hasattr(got, 'raw')
    direct = casegen.empty_cases(C, N, H, W, DEV)
    direct.grid.fill_(0x5a)
    for k in cc.OUTPUTS[1:]:
        getattr(direct, k).fill_(-7)
    rc = _native.lib().gnnpp_casegen(None, 0, casegen.threshold_of(0.1), seed, C, N, H, W, direct.grid.data_ptr(),
                                     direct.start.data_ptr(), direct.goal.data_ptr(), direct.cells.data_ptr(),
                                     direct.status.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    for k in cc.OUTPUTS:
        assert torch.equal(getattr(got, k), getattr(direct, k)), k
    want = cc.wants_of('random_20x20')                       # the parent's bytes: seed 13, the first 8 cases
    for k in cc.OUTPUTS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k][:C]), k


def test_one_maze_launch_replayed_from_a_graph(casegen):
    case = mz.TABLE['second_refill_21x13']
    C, H, W = case['C'], case['H'], case['W']

    def fresh():
        return (torch.full((C, H, W), mz.POISON, dtype=torch.uint8, device=DEV),
                torch.full((C,), -7, dtype=torch.int32, device=DEV))

    eager, graphed = fresh(), fresh()
    casegen.enqueue_maze_maps(eager[0], case['density'], case['complexity'], seed=case['seed0'], words=eager[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        casegen.enqueue_maze_maps(graphed[0], case['density'], case['complexity'], seed=case['seed0'], words=graphed[1])
    torch.cuda.synchronize()
    assert (graphed[0] == mz.POISON).all() and (graphed[1] == -7).all()             # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager[0], graphed[0]) and torch.equal(eager[1], graphed[1])
    mz.assert_equal_to_golden('second_refill_21x13', graphed[0].cpu().numpy(), graphed[1].cpu().numpy())


def test_refusals(casegen):
    from gnn_pathplanning_amd import _native
    L = _native.lib()
    st = _native.stream_ptr(torch.device(DEV))
    out = torch.full((2, 8, 8), mz.POISON, dtype=torch.uint8, device=DEV)

    def call(C=2, H=8, W=8, walls=1, steps=1, grid=True):
        return L.gnnpp_casegen_maze(None, 0, C, H, W, walls, steps, out.data_ptr() if grid else None, None, st)
    assert call(H=2) == call(W=2) == call(C=0) == call(grid=False) == call(walls=-1) == _native.ERR_ARG
    assert call(H=257) == call(W=257) == _native.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == mz.POISON).all()                          # nothing enqueued
    for H, W in ((2, 8), (8, 2)):
        with pytest.raises(_native.GnnppError, match='below 3'):
            casegen.maze_maps(2, H, W, DEV)
        with pytest.raises(_native.GnnppError, match='below 3'):
            casegen.generate(2, 4, H, W, DEV, maps='maze')
        with pytest.raises(_native.GnnppError, match='below 3'):
            casegen.enqueue_maze_maps(torch.empty((2, H, W), dtype=torch.uint8, device=DEV), 0.1, 0.01)
    for H, W in ((257, 8), (8, 257)):
        with pytest.raises(_native.GnnppError, match='%d x %d' % (H, W)):
            casegen.maze_maps(2, H, W, DEV)
        with pytest.raises(_native.GnnppError, match='%d x %d' % (H, W)):
            casegen.generate(2, 4, H, W, DEV, maps='maze')
    with pytest.raises(_native.GnnppError, match='grids'):
        casegen.generate(2, 4, 8, 8, DEV, maps='maze', grids=torch.zeros((8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        casegen.maze_maps(2, 8, 8, 'cpu')
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        casegen.generate(2, 4, 8, 8, 'cpu', maps='maze')
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        casegen.enqueue_maze_maps(torch.empty((2, 8, 8), dtype=torch.uint8), 0.1, 0.01)
    with pytest.raises(_native.GnnppError, match='seeds'):
        casegen.maze_maps(2, 8, 8, DEV, seeds=[1, 2, 3])
    with pytest.raises(_native.GnnppError, match='seeds'):
        casegen.maze_maps(2, 8, 8, DEV, seeds=[-1, 2])
