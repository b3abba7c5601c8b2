"""MAPF cases solved on the device by prioritized planning: the expert of the online-expert loop.

    BatchedRollout -> expert.solve_failures (this module) -> expert.samples_from_solutions -> SamplePool -> train_step

The reference's expert solvers are prebuilt binaries without source (offlineExpert/CasesSolver.py:517-539,
--chosen_solver ecbs | cbs | mapf_prioritized_sipp).  This is the prioritized option, restated exactly (include/gnnpp.h,
gnnpp_mapf): agents are planned one after another in a planning order, each against the finished plans of the agents
before it (vertex, swap and parking conflicts), by a bit-parallel search over time; one call plans C cases with R
orders each (csrc/mapf_kernels.hip).  Restart 0 is the index order, further restarts seeded random permutations; a
case keeps its best restart (solved, then smallest flowtime, smallest makespan, lowest index).  There is no CPU
fallback.  Positions are (row, col) integers: the reference's (x, y).
"""
import ctypes

import numpy as np
import torch

from . import _native

MAX_AGENTS = 128                      # GNNPP_ROLLOUT_MAX_AGENTS
MAX_SIDE = 64                         # GNNPP_MAPF_MAX_SIDE
MAX_STEPS = 1024                      # GNNPP_MAPF_MAX_STEPS
NO_PATH, BAD_CASE = 1, 2              # GNNPP_MAPF_* status bits


class Solutions:
    """Device tensors of one solve call: schedules [C,T+1,N,2] int32 (agents wait on their goal after arriving; -1 for
    agents left unplanned), arrival [C,N], makespan / flowtime / status / failing / restart [C] int32 (-1 where they do
    not apply), and the workspace."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return int(self.status.shape[0])

    def solved(self):
        """bool [C] on the host."""
        return (self.status == 0).cpu().numpy()

    def _solved_case(self, c):
        st = int(self.status[c])
        if st != 0:
            raise _native.GnnppError('case %d is not solved (status %d: %s)' % (
                c, st, 'bad case' if st & BAD_CASE else 'no path for agent %d' % int(self.failing[c])))

    def schedule(self, c):
        """[makespan+1, N, 2] int64 of a solved case: what expert.read_solution returns for it."""
        self._solved_case(c)
        return self.schedules[c, :int(self.makespan[c]) + 1].cpu().numpy().astype(np.int64)

    def paths(self, c):
        """Per agent its plan up to its arrival: [a_i+1, 2] int64 arrays (ECBS's schedule entries)."""
        self._solved_case(c)
        sched = self.schedules[c].cpu().numpy().astype(np.int64)
        return [sched[:int(a) + 1, n] for n, a in enumerate(self.arrival[c].cpu().tolist())]

    def solution_yaml(self, c):
        """The solver's output file in ECBS's format (statistics.cost / makespan, schedule.agentK = [{x, y, t}]):
        expert.read_solution reads it back to schedule(c)."""
        paths = self.paths(c)
        lines = ['statistics:', '  cost: %d' % sum(len(p) - 1 for p in paths),
                 '  makespan: %d' % (max(len(p) for p in paths) - 1), 'schedule:']
        for n, p in enumerate(paths):
            lines.append('  agent%d:' % n)
            for t, (x, y) in enumerate(p):
                lines += ['    - x: %d' % x, '      y: %d' % y, '      t: %d' % t]
        return '\n'.join(lines) + '\n'


def workspace_bytes(C, R, H, T):
    n = _native.lib().gnnpp_mapf_workspace_bytes(int(C), int(R), int(H), int(T))
    if n == 0:
        raise _native.GnnppError('no MAPF workspace for C=%d R=%d H=%d T_max=%d' % (C, R, H, T))
    return n


def empty_solutions(C, N, H, T, device, restarts=1):
    """Output tensors and workspace of a call on C cases of N agents, maps of H rows, horizon T, `restarts` orders."""
    dev = torch.device(device)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)
    return Solutions(schedules=i32(C, T + 1, N, 2), arrival=i32(C, N), makespan=i32(C), flowtime=i32(C),
                     status=i32(C), failing=i32(C), restart=i32(C),
                     workspace=torch.empty(workspace_bytes(C, restarts, H, T), dtype=torch.uint8, device=dev))


def enqueue_solve(grid, start, goal, order, out):
    """The native call alone, on torch's current stream of the tensors' device: no allocation, no host
    synchronisation, capturable in a HIP graph.  grid uint8 [C,H,W] | [H,W]; start, goal int32 [C,N,2]; order int32
    [C,R,N] or None (the index order); out: from empty_solutions (horizon T = out.schedules.shape[1] - 1).  All
    contiguous device tensors."""
    dev = _native.require_gpu(grid, start, goal, order, out.schedules, out.arrival, out.status, out.workspace)
    m = _native.MapfStruct()
    m.grid, m.grid_batched = grid.data_ptr(), int(grid.dim() == 3)
    m.start, m.goal = start.data_ptr(), goal.data_ptr()
    m.order = order.data_ptr() if order is not None else None
    m.C, m.N = int(start.shape[0]), int(start.shape[1])
    m.H, m.W = int(grid.shape[-2]), int(grid.shape[-1])
    m.R = int(order.shape[1]) if order is not None else 1
    m.T_max = int(out.schedules.shape[1]) - 1
    m.schedule, m.arrival, m.makespan = out.schedules.data_ptr(), out.arrival.data_ptr(), out.makespan.data_ptr()
    m.flowtime, m.status, m.failing = out.flowtime.data_ptr(), out.status.data_ptr(), out.failing.data_ptr()
    m.restart = out.restart.data_ptr()
    m.workspace, m.workspace_bytes = out.workspace.data_ptr(), out.workspace.numel()
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_mapf_solve(ctypes.byref(m), _native.stream_ptr(dev)), 'gnnpp_mapf_solve')


def _int32(x):
    return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(torch.int32)


def solve(grids, starts, goals, device, max_steps=None, restarts=1, priorities=None, seed=0):
    """Plan C cases: grids [C,H,W] or [H,W] (1 = obstacle), starts / goals [C,N,2] (row, col), host or device.
    max_steps: the horizon T_max (default 4 (H + W)).  priorities: planning orders [C,R,N] or [R,N] (shared by the
    cases), permutations of the agents; by default restart 0 is the index order and restarts 1 .. restarts-1 are
    random permutations drawn from numpy's default_rng(seed).  Returns Solutions; unsolved and invalid cases are
    reported in .status (NO_PATH, BAD_CASE), never raised."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('mapf.solve needs a HIP device (no CPU fallback)')
    g = grids if torch.is_tensor(grids) else torch.as_tensor(np.asarray(grids))
    start, goal = _int32(starts), _int32(goals)
    if start.dim() != 3 or start.shape[2] != 2 or tuple(goal.shape) != tuple(start.shape) or start.shape[0] < 1:
        raise _native.GnnppError('starts and goals must both be [C,N,2] with C >= 1 (got %s and %s)'
                                 % (tuple(start.shape), tuple(goal.shape)))
    C, N = int(start.shape[0]), int(start.shape[1])
    if not 1 <= N <= MAX_AGENTS:
        raise _native.GnnppError('teams of 1 to %d agents (got %d)' % (MAX_AGENTS, N))
    if g.dim() not in (2, 3) or (g.dim() == 3 and g.shape[0] != C):
        raise _native.GnnppError('grids must be [H,W] or [C,H,W] with one map per case')
    H, W = int(g.shape[-2]), int(g.shape[-1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise _native.GnnppError('maps of at most %d x %d cells (got %d x %d)' % (MAX_SIDE, MAX_SIDE, H, W))
    T = 4 * (H + W) if max_steps is None else int(max_steps)
    if not 0 <= T <= MAX_STEPS:
        raise _native.GnnppError('max_steps must be in 0 .. %d (got %d)' % (MAX_STEPS, T))
    order = None
    if priorities is not None:
        order = _int32(priorities)
        if order.dim() == 2:
            order = order.unsqueeze(0).expand(C, -1, -1)
        if order.dim() != 3 or order.shape[0] != C or order.shape[2] != N or order.shape[1] < 1:
            raise _native.GnnppError('priorities must be [C,R,N] or [R,N] (C = %d, N = %d), got %s'
                                     % (C, N, tuple(order.shape)))
    elif int(restarts) > 1:
        rng = np.random.default_rng(seed)
        perm = np.argsort(rng.random((C, int(restarts) - 1, N)), axis=-1)
        order = torch.from_numpy(np.concatenate([np.broadcast_to(np.arange(N), (C, 1, N)), perm], 1))
        order = order.to(torch.int32)
    elif int(restarts) < 1:
        raise _native.GnnppError('restarts must be >= 1 (got %d)' % restarts)
    R = 1 if order is None else int(order.shape[1])
    _native.lib()
    grid = g.to(torch.uint8).contiguous().to(dev)
    start, goal = start.contiguous().to(dev), goal.contiguous().to(dev)
    order = order.contiguous().to(dev) if order is not None else None
    out = empty_solutions(C, N, H, T, dev, R)
    out._keep = (grid, start, goal, order)              # inputs of the enqueued launches
    enqueue_solve(grid, start, goal, order, out)
    return out
