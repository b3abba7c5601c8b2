"""GPU (-m gpu): the shared case table of streamed rollouts (tests/rollout_stream_cases.py) through rollout.RolloutStream on
the device, with the assertions of the emulated run: every per-case table equals the plain per-case rollout of the same
script exactly (BatchedRollout with B = C, tie mode 'lowest'), the hand-derived values, the prefix seating order, a freshly
seated slot's S / obs / radius equal to observe() + gso() at step 0 of that case alone bit for bit, and untouched slots
keeping their bytes across a reseat."""
import numpy as np
import pytest
import torch

import rollout_stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def plain_rollout(tab, dev):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    env = BatchedRollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, commR=sc.COMM_R)
    env.observe()
    env.gso(0)
    fresh = {'obs': env.obs.cpu().numpy(), 'S': env.S.cpu().numpy(), 'radius': env.radius.cpu().numpy()}
    done_before = []
    for t in range(int(tab['maxstep'].max())):
        done_before.append(env.done.clone())
        env.move(actions=torch.from_numpy(sc.plain_actions(tab, t)).to(dev))
    res = env.results()
    assert res['done'].all()
    frozen = (torch.stack(done_before).cpu().numpy() != 0) | \
        (np.arange(1, len(done_before) + 1)[:, None] > tab['maxstep'][None, :])
    return {'reached': res['reached'].numpy().astype(np.int32), 'start_step': res['start_step'].numpy(),
            'end_step': res['end_step'].numpy(), 'pos': res['positions'].numpy(),
            'stats': np.stack([res['makespan'].numpy(), res['flowtime'].numpy()], 1), 'radius': fresh['radius'],
            'frozen': frozen}, fresh


class GpuEngine:
    """The engine of sc.run_stream over a RolloutStream."""

    def __init__(self, tab, dev):
        from gnn_pathplanning_amd.rollout import RolloutStream
        self.st = RolloutStream(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, slots=tab['slots'],
                                commR=sc.COMM_R, reseat_every=tab['reseat_every'])
        self.B, self.C, self.N = self.st.slots, self.st.C, self.st.N
        self.dev = dev

    def reseat(self, now):
        assert self.st.t == now
        self.st.reseat()

    def move(self, actions, step):
        assert self.st.t + 1 == step
        self.st.move(actions=torch.from_numpy(actions).to(self.dev))

    def read(self, name):
        st, e = self.st, self.st.env
        t = {'case': st.case, 't0': st.t0, 'assign': st.assign, 'cursor': st.cursor}.get(name)
        return (getattr(e, name) if t is None else t).cpu().numpy()

    def tables(self):
        res = self.st.results()
        out = {k: res[k].numpy() for k in ('start_step', 'end_step', 'radius', 'makespan', 'flowtime', 'lived', 'slot', 't0')}
        out['reached'] = res['reached'].numpy().astype(np.int32)
        out['pos'] = res['positions'].numpy()
        out['occupancy'] = res['occupancy']
        return out


@pytest.mark.parametrize('name', sc.TABLE_NAMES)
def test_gpu_stream_table(dev, name):
    tab = sc.table(name)
    plain, fresh = plain_rollout(tab, dev)
    want = sc.plain_expectation(plain)
    eng = GpuEngine(tab, dev)
    got, seats = sc.run_stream(eng, tab, fresh)
    sc.assert_tables(tab, got, want)
    sc.assert_seats(tab, seats, got)
    # occupancy = live slot-steps / all slot-steps
    assert got['occupancy'] == pytest.approx(float(want['lived'].sum()) / (eng.B * eng.st.t))
    assert (eng.st.pos.cpu().numpy() == want['pos']).all() and eng.st.B == eng.C
