"""CPU: the large-team rollout kernels (teams of 129..1024 agents, csrc/rollout_team_kernels.hip), compiled
unmodified for the host emulation, against the reference simulator's traces and the CPU oracle, bit-exactly."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


class Episodes:
    """B episodes' state in host arrays and the gnnpp_rollout struct pointing at them (emulated device memory)."""

    def __init__(self, grids, starts, goals, maxstep, commR=6.0, tie_mode=0):
        from gnn_pathplanning_amd._native import RolloutStruct
        B, N = starts.shape[:2]
        self.B, self.N = B, N
        self.grids = np.ascontiguousarray(grids.astype(np.uint8))
        self.goals = np.ascontiguousarray(goals.astype(np.int32))
        self.pos = np.ascontiguousarray(starts.astype(np.int32).copy())
        H, W = grids.shape[-2:]
        self.obs = np.zeros((B, N, 3, 11, 11), np.float32)
        self.radius = np.full(B, commR, np.float64)
        self.S = np.zeros((B, N, N), np.float32)
        self.conn = np.zeros(B, np.int32)
        self.reached = np.zeros((B, N), np.int32)
        self.start = np.full((B, N), -1, np.int32)
        self.end = np.full((B, N), -1, np.int32)
        self.maxstep = np.ascontiguousarray(np.broadcast_to(np.asarray(maxstep, np.int32), (B,)).copy())
        self.flags = np.zeros((B, 3), np.int32)
        self.stats = np.zeros((B, 2), np.int32)
        self.done = np.zeros(B, np.int32)
        self.ccount = np.zeros(B, np.int32)
        r = RolloutStruct()
        r.grid, r.grid_batched, r.goal, r.pos = self.grids.ctypes.data, int(grids.ndim == 3), self.goals.ctypes.data, \
            self.pos.ctypes.data
        r.B, r.N, r.H, r.W = B, N, H, W
        r.obs, r.radius, r.S, r.connected = self.obs.ctypes.data, self.radius.ctypes.data, self.S.ctypes.data, \
            self.conn.ctypes.data
        r.reached, r.start_step, r.end_step = self.reached.ctypes.data, self.start.ctypes.data, self.end.ctypes.data
        r.maxstep, r.flags, r.stats = self.maxstep.ctypes.data, self.flags.ctypes.data, self.stats.ctypes.data
        r.done = self.done.ctypes.data
        r.tie_mode, r.choice_count = tie_mode, self.ccount.ctypes.data
        self.r = r

    def move(self, lib, acts, step):
        a = np.ascontiguousarray(acts.astype(np.int32))
        self.r.logits, self.r.actions, self.r.currentstep = None, a.ctypes.data, step
        assert lib.gnnpp_rollout_move(ctypes.byref(self.r), None) == 0


def check_state_vs_oracle(lib, env, eps, ro, grow):
    """observe + gso of the current positions against the oracle."""
    env.r.grow = int(grow)
    radius_in = env.radius.copy()
    assert lib.gnnpp_rollout_observe(ctypes.byref(env.r), None) == 0
    assert lib.gnnpp_rollout_gso(ctypes.byref(env.r), None) == 0
    for b, ep in enumerate(eps):
        assert (env.obs[b] == ro.build_observations(ep.grid, ep.goal, ep.cur)).all(), b
        S, rad, conn = ro.communication_gso(ep.cur, radius_in[b], grow)
        assert env.radius[b] == rad and env.conn[b] == int(conn), b
        assert (env.S[b] == S.astype(np.float32)).all(), b


def test_emu_team_replays_reference_traces():
    """The reference simulator's traces of 160 and 256 agents, tie-breaks replayed: observations, GSO, radius,
    flags, positions, reached and the final statistics on every step, through the separate calls, the step call
    and the gso_observe call."""
    import emu_lib
    from gnn_pathplanning_amd._native import RolloutStruct
    from rollout_team_cases import load_team_traces
    from test_emu_rollout import replay_case
    lib = emu_lib.load()
    z, meta = load_team_traces()
    assert len(meta) == 4 and all(m['N'] > 128 for m in meta)
    assert sum(m['collisions'] for m in meta) > 100
    for ci, m in enumerate(meta):
        replay_case(lib, RolloutStruct, z, ci, m, fused=(False, True, 'pair', False)[ci])


@pytest.mark.parametrize('N', [129, 200, 300])
def test_emu_team_random_actions_vs_oracle(N):
    """Random joint actions on crowded maps: move (lowest-index tie-break), then observations and GSO of the new
    positions, all bit-exact against the oracle; radius growth at step 0."""
    import emu_lib
    from oracle import rollout_oracle as ro
    from rollout_team_cases import Recorder, make_instances
    lib = emu_lib.load()
    rng = np.random.default_rng(N)
    B, W = 2, 40
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05, box=(20, 20))
    env = Episodes(grids, starts, goals, 50)
    eps = [ro.EpisodeState(grids[b], goals[b], starts[b], 50) for b in range(B)]
    check_state_vs_oracle(lib, env, eps, ro, True)
    collisions = 0
    for t in range(3):
        acts = rng.integers(0, 5, size=(B, N))
        env.move(lib, acts, t + 1)
        for b in range(B):
            rec = Recorder(eps[b], lambda c: c[0])
            f = ro.move_step(eps[b], acts[b], t + 1, rec)
            assert [int(v) for v in f] == list(env.flags[b]), (t, b)
            assert (env.pos[b] == eps[b].cur).all(), (t, b)
            assert env.ccount[b] == rec.calls, (t, b)
            assert list(env.reached[b]) == [int(v) for v in eps[b].reached]
            collisions += rec.calls
        check_state_vs_oracle(lib, env, eps, ro, False)
    assert collisions > 10


def test_emu_team_dense_corridors_vs_oracle():
    """Agents packed head to tail in corridors, mostly pushing forward: the fall-backs chain through many repeat
    passes of the collision check and the all-stop branch fires; positions, flags and tie-break counts match."""
    import emu_lib
    import rollout_cases as rc
    from test_emu_rollout import run_move_case
    trace, _ = run_move_case(emu_lib.load(), rc.team_corridor_case())
    assert trace['all_stop'] > 0 and trace['most_passes'] >= 4, (trace['all_stop'], trace['most_passes'])


def test_emu_team_dense_conflicts_vs_oracle():
    """129 agents on 16 x 16, random joint actions: the dense-conflict case of the one-wave kernels at the smallest team
    the large-team kernels take."""
    import emu_lib
    import rollout_cases as rc
    from test_emu_rollout import run_move_case
    trace, _ = run_move_case(emu_lib.load(), rc.team_dense_conflict_case())
    assert trace['calls'].sum() > rc.TEAM_DENSE_FLOOR


def test_emu_team_mt19937_is_random_choice():
    """tie_mode mt19937 at N = 200: episode b moves as the oracle does with random.Random(seed_b).choice."""
    import emu_lib
    from oracle import rollout_oracle as ro
    from rollout_team_cases import make_instances
    lib = emu_lib.load()
    rng = np.random.default_rng(17)
    B, N, W, NW = 2, 200, 30, 4096
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.03, box=(16, 16))
    env = Episodes(grids, starts, goals, 99, tie_mode=3)
    words = np.array([[g.getrandbits(32) for _ in range(NW)] for g in (random.Random(500 + b) for b in range(B))],
                     dtype=np.uint32)
    cursor = np.zeros(B, np.int32)
    env.r.rng_words, env.r.rng_cursor, env.r.rng_max = words.ctypes.data, cursor.ctypes.data, NW
    eps = [ro.EpisodeState(grids[b], goals[b], starts[b], 99) for b in range(B)]
    gens = [random.Random(500 + b) for b in range(B)]
    draws = 0
    for t in range(4):
        acts = rng.integers(0, 5, size=(B, N))
        env.move(lib, acts, t + 1)
        for b in range(B):
            f = ro.move_step(eps[b], acts[b], t + 1, gens[b].choice)
            assert [int(v) for v in f] == list(env.flags[b]), (t, b)
            assert (env.pos[b] == eps[b].cur).all(), (t, b)
        draws += int(env.ccount.sum())
    assert draws > 20 and cursor.sum() >= draws


def test_emu_team_mixed_maxstep_freezes_finished_episodes():
    """Per-episode limits at N = 160: an episode past its own maxstep, or whose loop broke after allReachGoal,
    is frozen; statistics as the oracle's case loop reports them."""
    import emu_lib
    import rollout_cases as rc
    from test_emu_rollout import run_move_case
    _, stats = run_move_case(emu_lib.load(), rc.team_mixed_maxstep_case())
    assert list(stats[0]) == [1, 160]


def test_emu_team_argument_checks():
    """N = 1025 is GNNPP_ERR_ARG; a map beyond GNNPP_ROLLOUT_TEAM_MAX_CELLS is GNNPP_ERR_UNSUPPORTED for every call
    that needs it (nothing runs); a NULL-pointer struct stays GNNPP_ERR_ARG; the policy step keeps its limit."""
    import emu_lib
    from gnn_pathplanning_amd._native import RolloutStruct
    lib = emu_lib.load()
    r = RolloutStruct()
    r.B, r.N = 1, 200
    for fn in (lib.gnnpp_rollout_observe, lib.gnnpp_rollout_gso, lib.gnnpp_rollout_move, lib.gnnpp_rollout_step,
               lib.gnnpp_rollout_gso_observe):
        assert fn(ctypes.byref(r), None) == -1
    rng = np.random.default_rng(0)
    grids, starts, goals = make_instances_small(rng, 1025, 40)
    env = Episodes(grids, starts, goals, 10)
    for fn in (lib.gnnpp_rollout_observe, lib.gnnpp_rollout_gso, lib.gnnpp_rollout_move, lib.gnnpp_rollout_step,
               lib.gnnpp_rollout_gso_observe):
        assert fn(ctypes.byref(env.r), None) == -1
    # 257 x 256 = 65 792 cells > 65 536
    grids, starts, goals = make_instances_small(rng, 200, 257, 256)
    env = Episodes(grids, starts, goals, 10)
    env.r.actions = np.zeros((1, 200), np.int32).ctypes.data
    env.r.currentstep = 1
    pos0 = env.pos.copy()
    for fn in (lib.gnnpp_rollout_observe, lib.gnnpp_rollout_move, lib.gnnpp_rollout_step,
               lib.gnnpp_rollout_gso_observe):
        assert fn(ctypes.byref(env.r), None) == -2
    assert (env.pos == pos0).all() and (env.obs == 0).all() and (env.S == 0).all()
    assert lib.gnnpp_rollout_gso(ctypes.byref(env.r), None) == 0     # (the graph does not need the map)
    # gnnpp_rollout_policy_step(s) stay at GNNPP_ROLLOUT_MAX_AGENTS
    z = np.zeros(16, np.float32)
    env.r.logits = z.ctypes.data
    assert lib.gnnpp_rollout_policy_step(ctypes.byref(env.r), z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                         z.ctypes.data, z.ctypes.data, 3, 0, None) == -1


def make_instances_small(rng, N, H, W=None):
    from rollout_team_cases import make_instances
    return make_instances(rng, 1, N, H, W or H, 0.0)
