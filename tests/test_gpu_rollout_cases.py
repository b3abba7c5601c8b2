"""MI355X: the hand-built move-step cases of tests/rollout_cases.py (the ones tests/test_emu_rollout.py and
tests/test_emu_rollout_team.py run under the host emulation, which executes the work-items of a workgroup one at a time)
through BatchedRollout.move on the device: real waves, barriers, LDS atomics and ballots.  Positions, flags, reached,
start and end steps and tie-break counts of every episode after every step equal the sequential oracle's, bit for bit,
frozen episodes included; the floors on the number of tie-breaks keep the cases from quietly becoming easy."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def run_move_case(dev, case, tie='lowest', seed=0):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    trace = rc.oracle_trace(case, tie, seed)
    env = BatchedRollout(case['grids'], case['starts'], case['goals'], case['maxstep'], dev, tie_mode=tie, seed=seed)
    for t, acts in enumerate(case['actions']):
        flags = env.move(actions=torch.from_numpy(acts).to(dev)).cpu().numpy()
        where = (case['name'], tie, t)
        assert np.array_equal(flags, trace['flags'][t]), where
        assert np.array_equal(env.pos.cpu().numpy(), trace['pos'][t]), where
        assert np.array_equal(env.reached.cpu().numpy(), trace['reached'][t]), where
        assert np.array_equal(env.choice_count.cpu().numpy(), trace['calls'][t]), where
        assert np.array_equal(env.start_step.cpu().numpy(), trace['start_step'][t]), where
        assert np.array_equal(env.end_step.cpu().numpy(), trace['end_step'][t]), where
        if case['loop']:
            assert np.array_equal(env.done.cpu().numpy() != 0, trace['done'][t]), where
    if tie == 'mt19937':
        env.check_rng()
    if case['loop']:
        assert trace['done'][-1].all()
        assert np.array_equal(env.stats.cpu().numpy(), trace['stats'])
    return trace


@pytest.mark.parametrize('k', range(len(rc.DENSE_SHAPES)), ids=['%dx%d_on_%d' % s for s in rc.DENSE_SHAPES])
def test_move_dense_conflicts_vs_oracle(dev, k):
    """(B, N, W) = (24, 9, 4), (12, 14, 5), (6, 70, 10), (3, 14, 182); the last has no LDS cell-count map."""
    case = rc.dense_conflict_cases()[k]
    assert case['actions'].shape[1:] + case['grids'].shape[2:] == rc.DENSE_SHAPES[k]
    trace = run_move_case(dev, case)
    assert trace['calls'].sum() > 20 * len(case['starts']) // 6


def test_team_dense_conflicts_vs_oracle(dev):
    """129 agents on 16 x 16: the oracle alone counts 541 tie-breaks in the six steps (floor: 500)."""
    trace = run_move_case(dev, rc.team_dense_conflict_case())
    assert trace['calls'].sum() > rc.TEAM_DENSE_FLOOR


@pytest.mark.parametrize('tie', ['lowest', 'mt19937'])
def test_team_dense_corridors_vs_oracle(dev, tie):
    """200 agents head to tail in corridors; 'mt19937': episode b against random.Random(11 + b).choice."""
    trace = run_move_case(dev, rc.team_corridor_case(), tie, seed=11)
    assert trace['all_stop'] > 0 and trace['most_passes'] >= 4, (trace['all_stop'], trace['most_passes'])


@pytest.mark.parametrize('team', [False, True])
def test_mixed_maxstep_freezes_finished_episodes(dev, team):
    case = rc.team_mixed_maxstep_case() if team else rc.mixed_maxstep_case()
    trace = run_move_case(dev, case)
    assert trace['stats'][0].tolist() == [1, case['starts'].shape[1]]
