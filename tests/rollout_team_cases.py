"""TEST INFRASTRUCTURE ONLY: instances and oracle drivers for the large-team rollout tests
(tests/test_emu_rollout_team.py on the host emulator, tests/test_gpu_rollout_team.py on the device)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_team_traces():
    """tests/golden/rollout_traces_team.npz: the reference simulator's traces of teams of 160 and 256 agents
    (tools/gen_rollout_traces_team.py)."""
    z = np.load(os.path.join(GOLDEN, 'rollout_traces_team.npz'))
    return z, json.loads(bytes(z['meta']).decode())


def make_instances(rng, B, N, H, W, density=0.05, box=None):
    """B random maps [B,H,W] uint8 with N distinct free start and goal cells each.  box = (h, w): the starts are
    packed into the top-left h x w corner (crowded, many conflicts)."""
    grids = (rng.random((B, H, W)) < density).astype(np.uint8)
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        if box is not None:
            grids[b, :box[0], :box[1]] = 0
        free = np.argwhere(grids[b] == 0)
        sfree = free if box is None else free[(free[:, 0] < box[0]) & (free[:, 1] < box[1])]
        starts[b] = sfree[rng.choice(len(sfree), N, replace=False)]
        goals[b] = free[rng.choice(len(free), N, replace=False)]
    return grids, starts, goals


def corridor_instance(B, N, H, W):
    """Crowded corridors: rows of agents packed head to tail in free lanes separated by obstacle walls, every agent
    headed for the far end of its own lane -- long fall-back chains through the repeat passes."""
    grids = np.ones((B, H, W), np.uint8)
    grids[:, 0::2, :] = 0                               # lanes on even rows
    grids[:, :, 0] = 0                                  # one cross corridor joining them
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    lanes = [(r, c) for r in range(0, H, 2) for c in range(1, W)]
    for b in range(B):
        rng = np.random.default_rng(b)
        pick = rng.choice(len(lanes), 2 * N, replace=False)
        cells = np.array(lanes)[pick]
        starts[b], goals[b] = cells[:N], cells[N:]
    return grids, starts, goals


class Recorder:
    """Tie-break callback for oracle.rollout_oracle.move_step: picks with `pick(collided)`, counts the calls and
    the all-stop branches (a collided agent that already stands still)."""

    def __init__(self, ep, pick):
        self.ep, self.pick, self.calls, self.all_stop = ep, pick, 0, 0

    def __call__(self, collided):
        self.calls += 1
        if any(self.ep.last_action[j] == 4 for j in collided):
            self.all_stop += 1
        return self.pick(collided)
