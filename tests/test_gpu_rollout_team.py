"""GPU (-m gpu): rollouts of teams of 129..1024 agents (the large-team simulator kernels) through BatchedRollout,
against the reference simulator's traces and the CPU oracles.  Integer / boolean / fp64 stages are bit-exact."""
import random

import numpy as np
import pytest
import torch

from oracle import policy_oracle as orc
from oracle import rollout_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


class GreedyModel:
    """Stand-in policy for the rollout driver: every agent steps toward the goal cell of its observation (row
    first), the same logits whatever the batch.  Not trained, not in eval mode: BatchedRollout calls addGSO and
    forward_logits."""
    training = True

    def addGSO(self, S):
        self.S = S

    def forward_logits(self, obs):
        g = obs[:, :, 1].flatten(2).argmax(-1)                      # [B,N] goal cell in the 11 x 11 channel
        dx, dy = g // 11 - 5, g % 11 - 5
        act = torch.where(dx < 0, 0, torch.where(dx > 0, 2, torch.where(dy < 0, 1, torch.where(dy > 0, 3, 4))))
        return torch.nn.functional.one_hot(act, 5).float().transpose(0, 1).contiguous()   # [N,B,5]


def test_team_replays_reference_traces(dev):
    """The reference simulator's traces of 160 / 256 agents on 64 x 64 and 100 x 100 maps, tie-breaks replayed."""
    from rollout_team_cases import load_team_traces
    from test_gpu_rollout import _replay_traces
    z, meta = load_team_traces()
    assert [m['N'] for m in meta] == [160, 256, 160, 256]
    _replay_traces(dev, z, meta)


@pytest.mark.parametrize('tie', ['lowest', 'mt19937'])
@pytest.mark.parametrize('N', [129, 256, 512, 1024])
def test_team_random_actions_vs_oracle(dev, N, tie):
    """Random joint actions on crowded maps: observations, GSO (radius growth at step 0), move flags, positions,
    reached and tie-break counts bit-exact against the oracle."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import Recorder, make_instances
    B, W = 2, int((10 * N) ** 0.5)
    rng = np.random.default_rng(N + len(tie))
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    env = BatchedRollout(grids, starts, goals, 40, dev, tie_mode=tie, seed=11)
    eps = [ro.EpisodeState(grids[b], goals[b], starts[b], 40) for b in range(B)]
    gens = [random.Random(11 + b) for b in range(B)]
    radius = [6.0] * B
    collisions = 0
    for t in range(4):
        obs = env.observe().cpu().numpy()
        S = env.gso(t).cpu().numpy()
        for b in range(B):
            assert (obs[b] == ro.build_observations(grids[b], goals[b], eps[b].cur)).all(), (t, b)
            Sw, radius[b], conn = ro.communication_gso(eps[b].cur, radius[b], t == 0)
            assert (S[b] == Sw.astype(np.float32)).all(), (t, b)
            assert env.radius[b].item() == radius[b] and env.connected[b].item() == int(conn), (t, b)
        acts = rng.integers(0, 5, size=(B, N))
        flags = env.move(actions=torch.from_numpy(acts).to(dev)).cpu().numpy()
        pos, cc = env.pos.cpu().numpy(), env.choice_count.cpu().numpy()
        for b in range(B):
            rec = Recorder(eps[b], (lambda c: c[0]) if tie == 'lowest' else gens[b].choice)
            f = ro.move_step(eps[b], acts[b], t + 1, rec)
            assert [int(v) for v in f] == list(flags[b]), (t, b)
            assert (pos[b] == eps[b].cur).all(), (t, b)
            assert cc[b] == rec.calls, (t, b)
            assert (env.reached[b].cpu().numpy() == np.array(eps[b].reached, np.int32)).all()
            collisions += rec.calls
    env.check_rng()
    assert collisions > 10


def test_team_fused_calls_equal_separate_calls(dev):
    """move_and_observe (gnnpp_rollout_step) and move + gso_observe give what move + observe + gso give."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import make_instances
    B, N, W = 3, 300, 56
    rng = np.random.default_rng(3)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    envs = [BatchedRollout(grids, starts, goals, [6, 9, 12], dev, tie_mode='mt19937', seed=4) for _ in range(3)]
    for env in envs:
        env.observe()
        env.gso(0)
    for t in range(8):
        acts = torch.from_numpy(rng.integers(0, 5, size=(B, N))).to(dev)
        envs[0].move(actions=acts)
        envs[0].observe()
        envs[0].gso()
        envs[1].move_and_observe(actions=acts)
        envs[2].move(actions=acts)
        envs[2].gso_observe()
        for env in envs[1:]:
            for name in ('obs', 'S', 'radius', 'connected', 'pos', 'flags', 'reached', 'start_step', 'end_step',
                         'stats', 'done', 'choice_count', 'rng_cursor'):
                assert torch.equal(getattr(env, name), getattr(envs[0], name)), (t, name)


def test_team_grouped_rollout_equals_one_batch(dev):
    """GroupedRollout (episodes split over two streams) returns exactly the single batch's results; run() ends with
    every episode's loop done."""
    from gnn_pathplanning_amd.rollout import BatchedRollout, GroupedRollout
    from rollout_team_cases import make_instances
    B, N, W = 4, 200, 50
    rng = np.random.default_rng(9)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    limits = [10, 14, 18, 22]
    one = BatchedRollout(grids, starts, goals, limits, dev, tie_mode='mt19937', seed=5).run(GreedyModel())
    two = GroupedRollout(grids, starts, goals, limits, dev, groups=2, tie_mode='mt19937', seed=5).run(GreedyModel())
    assert one['done'].all() and two['done'].all()
    for k in one:
        if k == 'steps':
            assert one[k] == two[k]
        else:
            assert torch.equal(one[k], two[k]), k
    moved = (one['positions'].numpy() != starts).any(-1).mean()
    assert one['reached'].any() and moved > 0.5, moved           # the greedy policy moves most agents


def test_team_closed_loop_rollout_with_policy(dev):
    """DecentralPlannerNet (K = 3) driving 200-agent teams on 50 x 50 maps: observe -> gso -> forward -> move on the
    GPU; logits against the policy oracle, positions against the rollout oracle fed with the GPU's actions."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import make_instances
    B, N, W = 4, 200, 50
    rng = np.random.default_rng(15)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    sd = orc.init_state_dict(3, seed=23)
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(sd)
    env = BatchedRollout(grids, starts, goals, 8, dev, tie_mode='lowest')
    eps = [ro.EpisodeState(grids[b], goals[b], starts[b], 8) for b in range(B)]
    for t in range(6):
        obs = env.observe()
        S = env.gso()
        net.addGSO(S)
        logits = net.forward_logits(obs)                                  # [N,B,5]
        with torch.no_grad():
            want = torch.stack(orc.policy_forward(sd, S.cpu(), obs.cpu()), 0)
        assert (logits.cpu() - want).abs().max().item() <= 1e-4
        acts = net.decode_actions(logits).cpu().numpy()                   # [B,N]
        margin = torch.topk(want, 2, dim=-1).values
        clear = ((margin[..., 0] - margin[..., 1]) > 1e-5).numpy().T
        assert (acts[clear] == want.argmax(-1).numpy().T[clear]).all()
        env.move(logits=logits)
        pos = env.pos.cpu().numpy()
        for b in range(B):
            ro.loop_step(eps[b], acts[b], t + 1, lambda c: c[0])
            assert (pos[b] == eps[b].cur).all(), (t, b)
    out = BatchedRollout(grids, starts, goals, 12, dev).run(net, check_every=4)
    assert out['done'].all() and out['steps'] <= 12


def test_team_limits(dev):
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.rollout import BatchedRollout
    z = np.zeros((1, 1025, 2))
    with pytest.raises(_native.GnnppError, match='at most 1024'):
        BatchedRollout(np.zeros((64, 64)), z, z, 4, dev)
    s = np.stack([np.zeros(200), np.arange(200)], -1)[None]
    with pytest.raises(_native.GnnppError, match='65536 cells'):
        BatchedRollout(np.zeros((257, 256)), s, s, 4, dev)
