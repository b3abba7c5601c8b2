"""CPU: the host side of gnn_pathplanning_amd/expert.py against the golden file made by the real reference
(tests/golden/expert_schedules.npz): the failure-case YAML byte for byte, the schedule read back from a solver's
answer, the training .mat file, the sample pool's indexing."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
from gnn_pathplanning_amd import _native, expert, formats  # noqa: E402

GOLD = ec.load_golden()


def golden_samples(cases):
    """ScheduleSamples holding the REFERENCE's tensors (CPU) of the given golden cases (one team size)."""
    gs = [GOLD[c][1] for c in cases]
    bounds = np.cumsum([0] + [len(g['schedule']) for g in gs]).tolist()
    gso = torch.from_numpy(np.concatenate([g['GSO'] for g in gs]))
    return expert.ScheduleSamples(input=torch.from_numpy(np.concatenate([g['input'] for g in gs])).float(),
                                  GSO=gso.float(), GSO64=gso,
                                  target=torch.from_numpy(np.concatenate([g['target'] for g in gs])).float(),
                                  bounds=bounds)


@pytest.mark.parametrize('ci', range(len(GOLD)))
def test_failure_case_yaml_bytes(ci):
    m, g = GOLD[ci]
    text = expert.failure_case_yaml(g['grid'], g['schedule'][0], g['goal'])
    assert text.encode() == bytes(g['failure_yaml'])


def test_write_failure_cases_only_failed_episodes(tmp_path):
    """Three episodes on one map (the 24-agent 20 x 20 case); the second one succeeded: no file for it."""
    m, g = GOLD[4]
    pos = torch.from_numpy(np.stack([g['schedule'][0], g['goal'], g['schedule'][0]]))
    ro = types.SimpleNamespace(B=3, grid=torch.from_numpy(g['grid']), grid_batched=0,
                               goal=torch.from_numpy(np.stack([g['goal']] * 3)))
    res = {'positions': pos, 'success': torch.tensor([False, True, False])}
    written = expert.write_failure_cases(str(tmp_path), ro, ids=[4, 17, 123], results=res)
    assert [b for b, _ in written] == [0, 2]
    assert sorted(os.listdir(tmp_path)) == ['failureCases_ID00004.yaml', 'failureCases_ID00123.yaml']
    for _, path in written:
        assert open(path, 'rb').read() == bytes(g['failure_yaml'])
    with pytest.raises(_native.GnnppError):
        expert.write_failure_cases(str(tmp_path), ro, ids=[1], results=res)
    # one map per episode
    ro.grid, ro.grid_batched = torch.from_numpy(np.stack([g['grid']] * 3)), 1
    (_, path), _ = expert.write_failure_cases(str(tmp_path / 'b'), ro, results=res)
    assert path.endswith('failureCases_ID00000.yaml') and open(path, 'rb').read() == bytes(g['failure_yaml'])


@pytest.mark.parametrize('ci', range(len(GOLD)))
def test_read_solution_equals_reference_schedule(ci, tmp_path):
    m, g = GOLD[ci]
    grid, goal, schedule = expert.read_solution(bytes(g['failure_yaml']).decode(), bytes(g['solution_yaml']).decode())
    assert np.array_equal(grid, g['grid']) and np.array_equal(goal, g['goal'])
    assert schedule.shape == (m['T'], m['N'], 2) and np.array_equal(schedule, g['schedule'])
    a, b = tmp_path / 'in.yaml', tmp_path / 'out.yaml'
    a.write_bytes(bytes(g['failure_yaml']))
    b.write_bytes(bytes(g['solution_yaml']))
    from_files = expert.read_solution(str(a), str(b))
    assert all(np.array_equal(x, y) for x, y in zip(from_files, (grid, goal, schedule)))
    if ci == 0:                                                     # agents arrive at different times: they wait
        assert len(set(m['path_lengths'])) > 2


def test_mat_round_trip(tmp_path):
    m, g = GOLD[6]
    s = golden_samples([0, 6])
    path = str(tmp_path / ('train_ID00006_MP%d.mat' % m['T']))
    expert.save_samples_mat(path, g['grid'], g['goal'], g['schedule'], s, c=1)
    import scipy.io as sio
    d = sio.loadmat(path)
    assert set(k for k in d if not k.startswith('__')) == {'map', 'goal', 'inputState', 'inputTensor', 'target', 'GSO',
                                                          'makespan'}
    assert int(d['makespan'].reshape(-1)[0]) == m['T'] and d['GSO'].dtype == np.float64 and np.array_equal(d['GSO'], g['GSO'])
    assert np.array_equal(d['inputState'], g['schedule']) and np.array_equal(d['map'], g['grid'])
    for t in (0, m['T'] // 2, m['T'] - 1):
        inp, tgt, gso, grid = formats.load_training_step(path, t)
        assert torch.equal(inp, torch.from_numpy(g['input'][t]).float())
        assert torch.equal(tgt, torch.from_numpy(g['target'][t]).long())
        assert torch.equal(gso, torch.from_numpy(g['GSO'][t]).float())
        assert torch.equal(grid, torch.from_numpy(g['grid']).float())


def test_sample_pool_indexing():
    pool = expert.SamplePool()
    with pytest.raises(_native.GnnppError):
        pool.draw(4)
    s0, s6 = golden_samples([0]), golden_samples([6])
    pool.append(s0)
    pool.append(s6)
    n0, n = len(s0), len(s0) + len(s6)
    assert len(pool) == n
    s0.input.zero_()                                               # the pool owns its storage
    gen = torch.Generator().manual_seed(5)
    inp, tgt, gso = pool.draw(16, gen)
    assert inp.shape == (16, 10, 3, 11, 11) and tgt.shape == (16, 10, 5) and gso.shape == (16, 10, 10)
    assert inp.dtype == tgt.dtype == gso.dtype == torch.float32 and inp.is_contiguous()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:16]
    assert len(set(idx.tolist())) == 16
    both = golden_samples([0, 6])
    assert torch.equal(inp, both.input[idx]) and torch.equal(tgt, both.target[idx]) and torch.equal(gso, both.GSO[idx])
    inp, _, _ = pool.gather([0, n0, n - 1])
    assert torch.equal(inp, torch.stack([both.input[0], s6.input[0], s6.input[-1]]))
    assert pool.draw(3 * n, gen)[0].shape[0] == 3 * n              # a batch larger than the pool: with replacement
    with pytest.raises(_native.GnnppError):
        pool.append(golden_samples([2]))                           # another team size


def test_no_cpu_fallback():
    m, g = GOLD[7]
    with pytest.raises(_native.GnnppError):
        expert.samples_from_schedules(g['grid'], g['goal'][None], [g['schedule']], 'cpu')
