"""CPU: the training-sequence scenarios (tests/train_sequence_cases.py) before they reach a device -- their shapes, and
the sensitivity condition on their inputs: along the float64 trajectory of every scenario, the statement of each
training or eval operation at the parameters BEFORE the last update (what a one-step-stale weight copy computes) sits at
least STALE_FACTOR x the allowance of f64_yardstick away from the statement at the current parameters, for the logits and
for every gradient that is not identically zero.  The factor is a condition on seeds and learning rates, not a
measurement of any kernel."""
import pytest

import train_sequence_cases as tsc


def test_scenarios_keep_the_issue_shapes():
    assert (tsc.N, tsc.K, tsc.B_FULL, tsc.B_PART) == (4, 3, 8, 3)
    for name, c in tsc.SCENARIOS.items():
        ops = c['ops']
        trains = sum(1 for op, a in ops if op in tsc.TRAINING_OPS) + sum(a for op, a in ops if op == 'capture')
        assert sum(1 for op, _ in ops if op in tsc.TRAINING_OPS) <= 6, name
        assert trains <= 9, name
        mode, captured = True, False
        for op, a in ops:                                    # replays follow a capture; eval calls run in eval mode
            captured |= op == 'capture'
            mode = {'train': True, 'eval': False}.get(op, mode)
            assert op != 'replay' or (captured and mode and a != 'p'), name
            assert op not in ('eval_forward', 'rollout_step') or not mode, name
            assert op not in ('eager', 'forward', 'capture') or mode, name


@pytest.mark.parametrize('name', list(tsc.SCENARIOS))
def test_a_stale_copy_is_far_outside_the_yardstick(name):
    c = tsc.SCENARIOS[name]
    points = tsc.f64_trajectory(name)
    assert points, name
    worst = {}
    for i, kind, cur, prev, batch in points:
        r = tsc.stale_ratios(kind, cur, prev, batch, tsc.frozen_name if c['frozen'] else None)
        k = min(r, key=r.get)
        worst[(i, kind)] = (k, r[k])
    print(name, {k: '%s %.0fx' % v for k, v in worst.items()})
    assert all(v[1] >= tsc.STALE_FACTOR for v in worst.values()), worst
