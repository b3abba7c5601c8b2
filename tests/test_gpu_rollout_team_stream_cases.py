"""GPU (-m gpu): the shared case tables of streamed rollouts of large teams (tests/rollout_team_stream_cases.py) through
rollout.TeamRolloutStream.move on the device, on the dense graph and on the neighbour lists, with the assertions of the
emulated run: every per-case table equals the plain per-case rollout of the same scripts exactly (BatchedRollout with B = C,
tie mode 'lowest'), the hand-derived values, the prefix seating order, a freshly seated slot's graph / obs / radius equal to
observe() + gso(0) of that case alone bit for bit, and untouched slots keeping their bytes across a reseat."""
import numpy as np
import pytest
import torch

import rollout_team_stream_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


_plain = {}


def plain_rollout(tab, dev):
    """Once per table, shared by the two graph forms: the plain rollout's read-backs and {graph: step-0 state}."""
    if tab['name'] in _plain:
        return _plain[tab['name']]
    from gnn_pathplanning_amd.rollout import BatchedRollout
    C, N = tab['starts'].shape[:2]
    fresh = {}
    for graph in tc.GRAPHS:
        env = BatchedRollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, commR=tab['commR'], graph=graph)
        if graph == 'lists':
            env.lists.zero_()
        env.observe()
        env.gso(0)
        assert bool((env.connected == 1).all())
        S = env.S.cpu().numpy() if graph == 'dense' else tc.lists_slots(env.lists.cpu().numpy(), C, N)
        fresh[graph] = {'obs': env.obs.cpu().numpy(), 'S': S, 'radius': env.radius.cpu().numpy()}
    assert fresh['dense']['radius'].tobytes() == fresh['lists']['radius'].tobytes()
    done_before = []
    for t in range(int(tab['maxstep'].max())):               # (the moves do not read the graph: one run serves both forms)
        done_before.append(env.done.clone())
        env.move(actions=torch.from_numpy(tc.plain_actions(tab, t)).to(dev))
    res = env.results()
    assert res['done'].all()
    frozen = (torch.stack(done_before).cpu().numpy() != 0) | \
        (np.arange(1, len(done_before) + 1)[:, None] > tab['maxstep'][None, :])
    _plain[tab['name']] = ({'reached': res['reached'].numpy().astype(np.int32), 'start_step': res['start_step'].numpy(),
                            'end_step': res['end_step'].numpy(), 'pos': res['positions'].numpy(),
                            'stats': np.stack([res['makespan'].numpy(), res['flowtime'].numpy()], 1),
                            'radius': fresh['dense']['radius'], 'frozen': frozen}, fresh)
    return _plain[tab['name']]


class GpuTeamEngine:
    """The engine of the shared driver over a TeamRolloutStream."""

    def __init__(self, tab, dev, graph):
        from gnn_pathplanning_amd.rollout import TeamRolloutStream
        self.st = TeamRolloutStream(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, slots=tab['slots'],
                                    commR=tab['commR'], reseat_every=tab['reseat_every'], graph=graph)
        self.B, self.C, self.N = self.st.slots, self.st.C, self.st.N
        self.dev, self.graph = dev, graph
        assert (self.st.env.S is None) == (graph == 'lists')

    def reseat(self, now):
        assert self.st.t == now
        self.st.reseat()

    def move(self, actions, step):
        assert self.st.t + 1 == step
        self.st.move(actions=torch.from_numpy(actions).to(self.dev))

    def read(self, name):
        st, e = self.st, self.st.env
        if name == 'S' and self.graph == 'lists':
            return tc.lists_slots(e.lists.cpu().numpy(), self.B, self.N)
        t = {'case': st.case, 't0': st.t0, 'assign': st.assign, 'cursor': st.cursor}.get(name)
        return (getattr(e, name) if t is None else t).cpu().numpy()

    def tables(self):
        res = self.st.results()
        out = {k: res[k].numpy() for k in ('start_step', 'end_step', 'radius', 'makespan', 'flowtime', 'lived', 'slot', 't0')}
        out['reached'] = res['reached'].numpy().astype(np.int32)
        out['pos'] = res['positions'].numpy()
        out['occupancy'] = res['occupancy']
        return out


@pytest.mark.parametrize('graph', tc.GRAPHS)
@pytest.mark.parametrize('name', tc.TABLE_NAMES)
def test_gpu_team_stream_table(dev, name, graph):
    tab = tc.table(name)
    plain, fresh = plain_rollout(tab, dev)
    want = tc.plain_expectation(plain)
    eng = GpuTeamEngine(tab, dev, graph)
    got, seats = tc.run_stream(eng, tab, fresh[graph])
    tc.assert_tables(tab, got, want)
    tc.assert_seats(tab, seats, got)
    # occupancy = live slot-steps / all slot-steps
    assert got['occupancy'] == pytest.approx(float(want['lived'].sum()) / (eng.B * eng.st.t))
    assert (eng.st.pos.cpu().numpy() == want['pos']).all() and eng.st.B == eng.C
