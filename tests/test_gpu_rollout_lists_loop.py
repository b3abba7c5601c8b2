"""GPU (-m gpu): the closed loop on neighbour lists.  The same instances and the same planner (largeGraphFilter='lists',
eval mode) run four steps through BatchedRollout.step(model), once with graph='dense' and once with graph='lists': the
logits of every step are bit-identical and the episodes' state is equal after every step.  The 'lists' rollout has no
S tensor.  What graph='lists' cannot serve is refused with a GnnppError."""
import numpy as np
import pytest
import torch

from oracle import policy_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _planner(dev, N, K=3, route='lists', **cfg):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = N, K, dev, route
    for k, v in cfg.items():
        setattr(Cfg, k, v)
    return DecentralPlannerNet(Cfg()).to(dev).eval()


def _instances(seed, B, N, W):
    from rollout_team_cases import make_instances
    return make_instances(np.random.default_rng(seed), B, N, W, W, 0.05)


class _Tap:
    """The planner, recording the logits of every forward (dense or lists)."""

    def __init__(self, net):
        self.net, self.logits = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def forward_logits(self, obs):
        self.logits.append(self.net.forward_logits(obs).clone())
        return self.logits[-1]

    def forward_logits_lists(self, obs, lists):
        self.logits.append(self.net.forward_logits_lists(obs, lists).clone())
        return self.logits[-1]


STATE = ('pos', 'flags', 'reached', 'radius', 'rng_cursor', 'connected', 'start_step', 'end_step', 'done', 'obs')


@pytest.mark.parametrize('tie', ['lowest', 'mt19937'])
@pytest.mark.parametrize('shape', [(2, 160, 40), (2, 1024, 64)], ids=str)
def test_lists_rollout_equals_dense_rollout(dev, shape, tie):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    B, N, W = shape
    grids, starts, goals = _instances(N + 1, B, N, W)
    net = _planner(dev, N)
    sd = orc.init_state_dict(3, seed=23)
    # a head whose arg-max differs from agent to agent, so that the teams move and collide
    sd['actionsMLP.0.weight'] = torch.randn(5, 128, generator=torch.Generator().manual_seed(5))
    sd['actionsMLP.0.bias'] = torch.zeros(5)
    net.load_state_dict(sd)
    envs = [BatchedRollout(grids, starts, goals, 20, dev, tie_mode=tie, seed=77, graph=g) for g in ('dense', 'lists')]
    taps = [_Tap(net), _Tap(net)]
    assert envs[0].S is not None and envs[0].lists is None
    assert envs[1].S is None and envs[1].lists.dtype is torch.uint8
    with torch.no_grad():
        for t in range(4):
            for env, tap in zip(envs, taps):
                env.step(tap)
            torch.cuda.synchronize(dev)
            assert len(taps[0].logits) == len(taps[1].logits) == t + 1
            assert taps[0].logits[t].cpu().numpy().tobytes() == taps[1].logits[t].cpu().numpy().tobytes(), t
            for name in STATE:
                a, b = getattr(envs[0], name), getattr(envs[1], name)
                if a is None:
                    assert b is None and tie == 'lowest' and name == 'rng_cursor'
                    continue
                assert torch.equal(a, b), (t, name)
    assert envs[0].t == envs[1].t == 4 and envs[1].S is None
    moved = int((envs[0].pos.cpu() != torch.as_tensor(starts)).any(-1).sum())
    print('agents off their start cell after 4 steps: %d of %d' % (moved, B * N))
    assert moved > B * N // 10
    if tie == 'mt19937' and N == 1024:
        assert int(envs[0].rng_cursor.sum()) > 0                # (tie-breaks were drawn)
    # the graph of the positions after the last step, both ways
    from gnn_pathplanning_amd import graphML as gml
    S = envs[0].gso(step=1)
    blk = envs[1].gso(step=1)
    assert torch.equal(gml.team_lists_to_dense(blk, B, N), S)
    assert torch.equal(blk, envs[1].lists)


def test_lists_rollout_multilayer_planner(dev):
    """L = 2, E = 1 planner (the generic shape: encoder, lsigf_team(lists=...), head call) in the closed loop."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    B, N, W = 2, 130, 36
    grids, starts, goals = _instances(9, B, N, W)
    torch.manual_seed(3)
    net = _planner(dev, N, [2, 3], dimNodeSignals=[64, 48])
    envs = [BatchedRollout(grids, starts, goals, 20, dev, graph=g) for g in ('dense', 'lists')]
    taps = [_Tap(net), _Tap(net)]
    with torch.no_grad():
        for t in range(2):
            for env, tap in zip(envs[::-1], taps[::-1]):       # (the lists route is the fresh planner's first forward)
                env.step(tap)
            assert torch.equal(taps[0].logits[t], taps[1].logits[t]) and torch.equal(envs[0].pos, envs[1].pos)


def test_lists_rollout_refusals(dev):
    from gnn_pathplanning_amd import _native, graphML as gml
    from gnn_pathplanning_amd.rollout import BatchedRollout, GroupedRollout
    B, N, W = 2, 130, 36
    grids, starts, goals = _instances(10, B, N, W)
    env = BatchedRollout(grids, starts, goals, 20, dev, graph='lists')
    pos0 = env.pos.clone()
    with torch.no_grad():
        for bad, word in ((_planner(dev, N, route='dense'), 'largeGraphFilter'), (_planner(dev, N + 1), 'teams of'),
                          (_planner(dev, N, precision='split_f16'), 'split_f16'), (_planner(dev, N).train(), 'eval')):
            with pytest.raises(_native.GnnppError, match=word):
                env.step(bad)

        class NoLists:
            training = False
        with pytest.raises(_native.GnnppError, match='forward_logits_lists'):
            env.step(NoLists())
        assert env.t == 0 and torch.equal(env.pos, pos0)
        # the one-launch small-team step reads the dense GSO
        g2, s2, t2 = _instances(11, 2, 10, 20)
        small = BatchedRollout(g2, s2, t2, 20, dev, graph='lists')
        with pytest.raises(_native.GnnppError, match='one-launch'):
            small.step(_planner(dev, 10))
        # a GSO larger than the team: lists are built for the team
        net = _planner(dev, N)
        with pytest.raises(_native.GnnppError, match='built for the team'):
            net.forward_logits_lists(env.observe(), gml.team_lists_from_dense(torch.zeros(B, 1, N + 4, N + 4, device=dev)))
    with pytest.raises(_native.GnnppError):
        BatchedRollout(grids, starts, goals, 20, dev, graph='sparse')
    # GroupedRollout passes the keyword through
    grp = GroupedRollout(grids, starts, goals, 20, dev, groups=2, graph='lists')
    assert all(e.graph == 'lists' and e.S is None for e in grp.envs)
    with torch.no_grad():
        grp.steps(_planner(dev, N), 2)
    assert grp.results()['steps'] == 2
