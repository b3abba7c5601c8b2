"""CPU: metrics.Summary over records the emulated kernel wrote.  The fixture tests/golden/metrics_summary.npz
(tools/gen_metrics_golden.py: 40 cases fed through the reference's own MonitoringMultiAgentPerformance) is met under the
reference's names, tags included; Summary.merge of three uneven shards equals the unsplit summary; per_group and host of a
grouped record agree with the restatement."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rollout_summary_cases as rc                                                  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics_summary.npz')
RATES = ('rateReachGoal', 'avg_rate_deltaMP', 'std_rate_deltaMP', 'avg_rate_deltaFT', 'std_rate_deltaFT',
         'rateFailedReachGoalSH', 'ratefindOptimalSolution', 'rateCollsionFreeSol', 'rateCollisionPredictedinLoop')


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.load()


def golden_entry():
    z = np.load(GOLDEN)
    x = {'C': int(z['reached'].shape[0]), 'N': int(z['reached'].shape[1]), 'G': 1, 'reached': z['reached'], 'stats': z['stats'],
         'targets': z['targets'], 'target_stride': 2, 'valid': None, 'group': None, 'shielded': z['shielded'],
         'audit_ok': z['audit_ok']}
    return z, x


class Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, value, step))


def assert_meets_reference(summary, z):
    """host() under the reference's names against the fixture's recorded numbers; the tags of write_scalars."""
    res = summary.host()
    for k in RATES:
        assert rc.rel_diff([res[k]], [float(z[k])]) <= rc.TOL, (k, res[k], float(z[k]))
    assert res['list_numAgentReachGoal'] == z['hist_numAgentReachGoal'].tolist()
    assert res['list_numAgentReachGoal'] == np.bincount(z['list_numAgentReachGoal'], minlength=5).tolist()
    assert res['n'] == len(z['list_numAgentReachGoal']) and res['n_degenerate'] == 0 and res['n_bad_group'] == 0
    w = Writer()
    assert summary.write_scalars(w, 'valid', int(z['scalar_epoch'][0])) is w
    assert [c[0] for c in w.calls] == z['scalar_tags'].tolist() and len(w.calls) == 5
    assert [c[2] for c in w.calls] == z['scalar_epoch'].tolist()
    assert rc.rel_diff([c[1] for c in w.calls], z['scalar_values']) <= rc.TOL


def test_fixture_is_what_the_reference_reported():
    """The fixture holds the reference's numbers, not ours: numpy on its recorded per-case rates gives them back."""
    z, x = golden_entry()
    assert x['C'] == 40 and x['N'] == 4 and (z['targets'] > 0).all()
    assert float(z['avg_rate_deltaMP']) == np.mean(z['list_rate_deltaMP'])
    assert float(z['std_rate_deltaFT']) == np.std(z['list_rate_deltaFT'], ddof=1)
    assert 0 < float(z['rateReachGoal']) < 1 and 0 < float(z['rateFailedReachGoalSH']) and float(z['ratefindOptimalSolution']) > 0


def test_emulated_kernel_meets_the_fixture(emu):
    from gnn_pathplanning_amd.metrics import Summary
    z, x = golden_entry()
    got = rc.run_host(emu, x)
    rc.check(got, rc.restate(x), 'fixture')
    assert_meets_reference(Summary(*got), z)


@pytest.mark.parametrize('with_valid', [True, False])
def test_merge_of_three_uneven_parts_equals_the_unsplit_summary(emu, with_valid):
    from gnn_pathplanning_amd.metrics import Summary
    x = rc.inputs(600, 3, 3, with_valid, 'one')
    whole = rc.run_host(emu, x)
    parts = [Summary(*rc.run_host(emu, rc.shard(x, lo, hi))) for lo, hi in ((0, 97), (97, 98), (98, 600))]
    merged = Summary.merge(parts)
    d = rc.check(merged._read(), whole, 'merge')
    print('merge against the unsplit record: largest relative difference %.3g' % d)
    # ... and the merged record reads like any other
    a, b = merged.per_group(2), Summary(*whole).per_group(2)
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], float):
            assert rc.rel_diff([a[k]], [b[k]]) <= rc.TOL, k
        else:
            assert a[k] == b[k], k
    assert merged.per_group(1)['n'] == 0 and math.isnan(merged.per_group(1)['rateReachGoal'])
    # a part without the optional tables drops their counts from the whole, and says so with NaN
    bare = dict(rc.shard(x, 0, 97), shielded=None, audit_ok=None)
    mixed = Summary.merge([Summary(*rc.run_host(emu, bare))] + parts[1:])
    if with_valid:
        assert math.isnan(mixed.per_group(0)['rateFailedReachGoalSH']) and not math.isnan(merged.per_group(0)['rateFailedReachGoalSH'])
    assert mixed.per_group(0)['n'] == merged.per_group(0)['n']


def test_host_of_a_grouped_record_is_the_whole_evaluation(emu):
    """host() of a record of three groups = the one-group record of the same cases without the one whose id is out of range."""
    from gnn_pathplanning_amd.metrics import Summary
    x = rc.inputs(257, 3, 3, True, 'one')
    grouped = Summary(*rc.run_host(emu, x))
    keep = np.ones(x['C'], bool)
    keep[x['C'] // 2] = False
    one = dict(x, G=1, group=None, valid=(x['valid'] * keep).astype(np.int32))
    want = Summary(*rc.run_host(emu, one)).host()
    got = grouped.host()
    assert got['n_bad_group'] == int(x['valid'][x['C'] // 2] != 0) and want['n_bad_group'] == 0
    for k in want:
        if k == 'n_bad_group':
            continue
        if isinstance(want[k], float):
            assert rc.rel_diff([got[k]], [want[k]]) <= rc.TOL, k
        else:
            assert got[k] == want[k], k
    with pytest.raises(Exception, match='group 3 of 3'):
        grouped.per_group(3)
