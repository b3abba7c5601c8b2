"""CPU: the matrix of tests/train_freeze_cases.py reaches every needs_input_grad signature of the training step's autograd
Functions, its float64 statement of a frozen step is right, and every `direct` case would see a ReLU mask lost between two
neighbouring Functions -- so that tests/test_gpu_training_frozen_f64.py cannot pass on a step whose contracts hold only
when everything is trainable."""
import itertools

import pytest
import torch

import train_freeze_cases as fc

# the float64 difference a lost mask makes must exceed the yardstick's allowance by this factor: a condition on the
# inputs, not a tolerance (a case that falls short gets another seed, not another factor)
SENSITIVITY = 1000.0
ISSUE_ELSEWHERE = ('transfer', 'filter_frozen', 'head_frozen', 'biases_frozen')
SMALL_CASES = [c for c in fc.MATRIX if c[1] in fc.SMALL]
DIRECT_CASES = [c for c in fc.MATRIX if c[1] in fc.DIRECT]


def test_restated_limit_is_the_packages():
    import gnn_pathplanning_amd.graphML as gml
    assert fc.MAX_NODES == gml.MAX_NODES


def test_routes_and_required_pairs():
    """The five routes (the neighbour-list one in fp32 and fp32_mfma), E = 2 on one small and one list row, every pattern
    on the first `direct` route, the four named patterns on every other, first_filter_frozen on both L = 2 routes."""
    assert [fc.route_name(r) for r in fc.ROUTES] == ['direct', 'direct', 'padded', 'dense', 'lists', 'lists']
    R = fc.ROUTES
    assert (R['direct']['B'], R['direct']['N'], R['direct']['K'], R['direct']['L']) == (8, 4, 3, 1)
    assert R['direct_L2']['L'] == 2 and len(set(R['direct_L2']['widths'])) == 2
    assert R['padded_L2']['L'] == 2 and R['padded_L2']['Ns'] == R['padded_L2']['N'] + 3
    for r in ('dense', 'lists', 'lists_mfma_E2'):
        assert (R[r]['B'], R[r]['N']) == (2, 113)
    assert {R[r].get('precision') for r in ('lists', 'lists_mfma_E2')} == {'fp32', 'fp32_mfma'}
    assert any(R[r]['E'] == 2 for r in fc.SMALL) and R['lists_mfma_E2']['E'] == 2
    m = set(fc.MATRIX)
    assert len(m) == len(fc.MATRIX)
    for p in fc.ISSUE_PATTERNS:
        assert (p, 'direct') in m or p == 'first_filter_frozen'
    for r in R:
        if r != 'direct':
            assert all((p, r) in m for p in ISSUE_ELSEWHERE)
            assert (('first_filter_frozen', r) in m) == (R[r]['L'] == 2)
    assert sum(R[r]['L'] == 2 for r in R) == 2


def test_transfer_is_what_the_package_freezes():
    """Everything but the graph filter and the action head, and a proper subset."""
    frozen = fc._transfer()
    for r in fc.ROUTES:
        for k in fc.param_names(r):
            assert (k in frozen) == (not k.startswith(('GFL.', 'actionsMLP.'))), k


def test_param_names_are_the_planners():
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    for r, c in fc.ROUTES.items():
        net = DecentralPlannerNet(fc.Cfg(c['N'], c['K'], 'cpu', c['L'], c['E'], c['widths']))
        assert [k for k, _ in net.named_parameters()] == fc.param_names(r)


def test_every_pattern_freezes_something_and_leaves_something():
    for case in fc.MATRIX:
        t = fc.trainable(case)
        assert 0 < len(t) < len(fc.param_names(case[1])), case


def test_needs_input_grad_signatures_are_complete():
    """_LinearFunction (compress, head) and the filter Function of EVERY route: all 7 signatures of (x, W, b) / (h, x, b)
    in which some input needs a gradient.  _EncoderTrainFunction has 20 parameter inputs and no branch on any of them (its
    backward writes all 20 gradients): it is reached with every input trainable, with a proper subset (the BatchNorm
    affine parameters frozen), and not at all (every input frozen: the node does not exist)."""
    want = {s for s in itertools.product((False, True), repeat=3) if any(s)}
    got = {'compress': set(), 'head': set()}
    enc = set()
    for case in fc.MATRIX:
        sig = fc.signatures(case)
        got['compress'].add(sig['compress'])
        got['head'].add(sig['head'])
        enc.add(sig['encoder'])
        r = case[1]
        for l in range(fc.ROUTES[r]['L']):
            # (per filter Function: the LDS-resident form with the folds of `direct`, the same without them on a padded
            # signal, the dense form, the neighbour-list form)
            got.setdefault(fc.route_name(r), set()).add(sig['GFL.%d' % (2 * l)])
    assert got['compress'] >= want and got['head'] >= want
    for fn in ('direct', 'padded', 'dense', 'lists'):
        assert got[fn] >= want, (fn, want - got[fn])
    assert (True,) * 20 in enc and (False,) * 20 in enc and (True, True, False, False) * 5 in enc


def test_signatures_are_autograds():
    """The restated signatures against autograd itself on the float64 statement: a parameter gets a gradient exactly when
    the pattern leaves it trainable."""
    for case in SMALL_CASES:
        w = fc.frozen_statement(case)
        assert list(w['grads']) == fc.trainable(case), case
        assert all(g is not None for g in w['grads'].values())


@pytest.mark.parametrize('case', SMALL_CASES + [('transfer', 'dense')], ids=fc.case_id)
def test_frozen_statement_is_the_unfrozen_one(case):
    """float64: freezing changes no value -- the trainable gradients, loss, logits, features, running statistics and
    num_batches_tracked are those of the statement with nothing frozen, bit for bit."""
    w64, _ = fc.statements(case[1])
    w = fc.frozen_statement(case)
    assert list(w['grads']) == fc.trainable(case)
    for k, g in w['grads'].items():
        assert torch.equal(g, w64['grads'][k]), k
    for k in ('loss', 'logits', 'feat'):
        assert torch.equal(w[k], w64[k]), k
    assert w['running'].keys() == w64['running'].keys() and w['nbt'] == w64['nbt']
    for k, v in w['running'].items():
        assert torch.equal(v, w64['running'][k]), k
    sd = fc.build(case[1])[0]
    N = fc.ROUTES[case[1]]['N']
    for k, n in w['nbt'].items():                        # a frozen encoder's BatchNorm still counts its N calls
        assert n == int(sd[k]) + N
    assert any(not torch.equal(v, sd[k].double()) for k, v in w['running'].items())


@pytest.mark.parametrize('r', fc.SMALL)
def test_mask_regime(r):
    """Between 10 % and 90 % of the pre-activations at the compress output and at each filter output are non-positive: a
    mask that is all ones or all zeros hides a lost or doubled fold."""
    shares = fc.non_positive_shares(r)
    assert list(shares) == fc.mask_names(r)
    print(r, shares)
    for k, s in shares.items():
        assert 0.10 <= s <= 0.90, (r, k, s)


@pytest.mark.parametrize('case', DIRECT_CASES, ids=fc.case_id)
def test_a_lost_relu_mask_is_far_outside_the_yardstick(case):
    """The float64 statement with the compress ReLU's backward mask dropped, and with the last filter's dropped: some
    trainable tensor below the mask differs from the true gradient by more than SENSITIVITY x the yardstick's allowance,
    in RMS and in the largest entry.  Where the pattern leaves nothing trainable below a mask, that ReLU's backward is not
    part of the step: the statement is then unchanged, bit for bit."""
    r = case[1]
    w64, _ = fc.statements(r)
    for which in ('compress', fc.mask_names(r)[-1]):
        excess = fc.lost_mask_excess(case, which)
        print(fc.case_id(case), which, {k: '%.3g' % v for k, v in excess.items()})
        below = [k for k in fc.below_mask(r, which) if k in fc.trainable(case)]
        assert sorted(excess) == sorted(below)
        if below:
            assert max(excess.values()) > SENSITIVITY, (which, excess)
        else:
            wrong = fc.frozen_statement(case, relu=fc.relu_without_backward_mask(which))['grads']
            assert all(torch.equal(g, w64['grads'][k]) for k, g in wrong.items())
