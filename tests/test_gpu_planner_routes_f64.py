"""GPU (-m gpu): eval-mode DecentralPlannerNet with several graph-filter layers on a GSO with more nodes than the team,
on every route of the planner (tests/planner_route_cases.py), against the float64 statement of the same network
(pc.policy_statement: every layer zero-pads its input to the GSO's nodes and cuts its output back to the team, as the
reference's GraphFilterBatch.forward does, graphML.py:2464-2476) with the fp32 CPU statement as the yardstick
(tests/f64_yardstick.py, factors unchanged).  tests/test_planner_routes.py shows on the CPU that a planner that pads
only once misses every such case by more than 1000 x what the yardstick allows.

Per case and precision ('fp32', 'fp32_mfma', 'split_f16' with range_policy='flag'; graphs beyond graphML.MAX_NODES also
under largeGraphFilter 'dense' and 'lists'): logits through forward_logits, actions through decode_actions.  Observed
of the path: the one-call routes (gnnpp_policy_fwd beyond the fused kernel's teams, gnnpp_policy_team_fwd) fill the
planner's feature workspace and every other route leaves it alone; the per-layer routes on the LDS-resident kernels
get shapes gnnpp_lsigf_fits accepts; under split_f16, 'lists' is the dense form, byte for byte.
"""
import numpy as np
import pytest
import torch

import planner_route_cases as prc
import policy_f64_cases as pc
from gnn_pathplanning_amd._native import TUNE_FUSED_POLICY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def _runs():
    out = []
    for c in prc.CASES:
        for lgf in (('dense', 'lists') if c['Ns'] > prc.MAX_NODES else (None,)):
            for prec in prc.PRECISIONS:
                out.append(pytest.param(c, prec, lgf, id='%s-%s%s' % (prc.case_id(c), prec, '-' + lgf if lgf else '')))
    return out


def run_planner(dev, case, prec, lgf):
    """(logits [N,B,5], actions [B,N], feature workspace [B*N,128] after the call) of the planner on the case.  The
    workspace is the one the one-call routes hand to their C call; it is filled with NaN before the forward."""
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    sd, obs, S = prc.build_case(case)
    net = DecentralPlannerNet(prc.planner_config(case, dev, prec, lgf)).to(dev).eval()
    net.load_state_dict(sd)
    prc.add_gso(net, S, dev)
    with _native.device_guard(dev):
        ws = net._feat_workspace(case['B'] * case['N'], _native.stream_ptr(dev), dev)
    ws.fill_(float('nan'))
    with torch.no_grad():
        logits = net.forward_logits(obs.to(dev))
        acts = net.decode_actions(logits)
    torch.cuda.synchronize()
    assert not net.range_exceeded()
    assert net._ws is ws
    return logits.cpu().numpy(), acts.cpu().numpy(), ws.cpu().numpy()


@pytest.mark.parametrize('case,prec,lgf', _runs())
def test_planner_routes_f64(dev, case, prec, lgf):
    from gnn_pathplanning_amd import _native
    lib = _native.lib()
    B, N, Ns, E = case['B'], case['N'], case['Ns'], case['E']
    L = len(case['taps'])
    rt = prc.route(False, N, Ns, L, E, case['widths'], prec, lgf or 'dense')
    name = '%s/%s/%s' % (prc.case_id(case), prec, rt)
    if rt.startswith('small_general'):          # every layer is served by the LDS-resident kernels, not refused
        F = (prc.FEATURES,) + case['widths']
        for l, K in enumerate(case['taps']):
            assert lib.gnnpp_lsigf_fits(Ns, F[l], F[l + 1], K, E) == 1, (name, l)
    logits, acts, ws = run_planner(dev, case, prec, lgf)
    assert logits.shape == (N, B, 5)
    l64, l32 = prc.statements(case)
    ok, rep = pc.gap(logits, l64, l32)
    print('%s: max %.3g (fp32 statement %.3g), rms %.3g (%.3g), allowed %.3g, scale %.3g'
          % (name, rep['max'], rep['max32'], rep['rms'], rep['rms32'], pc.allowed_error(rep), rep['scale']))
    # the observable half of the path: who writes the planner's feature workspace
    fused = pc.fused_policy_applies(B, N, case['taps'][0], E, _native.precision_code(prec),
                                    lib.gnnpp_get_tuning(TUNE_FUSED_POLICY))
    if rt == 'lists_one_call' or (rt == 'policy_fwd' and not fused):
        assert np.isfinite(ws).all(), name
    else:
        assert np.isnan(ws).all(), name
    rep = pc.check(name + '/logits', logits, l64, l32)
    pc.check_actions(name, acts, l64, rep)


@pytest.mark.parametrize('case', [c for c in prc.CASES if c['Ns'] > prc.MAX_NODES], ids=prc.case_id)
def test_split_f16_lists_is_the_dense_form(dev, case):
    """precision='split_f16' keeps the dense form under largeGraphFilter='lists' (documented): the same bytes."""
    dense, acts_d, _ = run_planner(dev, case, 'split_f16', 'dense')
    lists, acts_l, _ = run_planner(dev, case, 'split_f16', 'lists')
    assert dense.tobytes() == lists.tobytes()
    assert np.array_equal(acts_d, acts_l)
