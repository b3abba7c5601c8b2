"""MAPF cases solved on the device by prioritized planning: the expert of the online-expert loop.

    BatchedRollout -> expert.solve_failures (this module) -> expert.samples_from_solutions -> SamplePool -> train_step

The reference's expert solvers are prebuilt binaries without source (offlineExpert/CasesSolver.py:517-539,
--chosen_solver ecbs | cbs | mapf_prioritized_sipp).  This is the prioritized option, restated exactly (include/gnnpp.h,
gnnpp_mapf): agents are planned one after another in a planning order, each against the finished plans of the agents
before it (vertex, swap and parking conflicts), by a bit-parallel search over time; one call plans C cases with R
orders each (csrc/mapf_kernels.hip: one wave per case, teams of up to 128 agents on maps of up to 64 x 64 -- solve;
csrc/mapf_team_kernels.hip: one workgroup per case, up to 1024 agents on maps of up to 256 x 256 -- solve_team; the
same contract and, where both apply, the same outputs).  Restart 0 is the index order, further restarts seeded random permutations; a
case keeps its best restart (solved, then smallest flowtime, smallest makespan, lowest index).  There is no CPU
fallback.  Positions are (row, col) integers: the reference's (x, y).

Orders that look at the case (include/gnnpp_mapf_distance.h, csrc/mapf_distance_kernels.hip): distances() is every
agent's true shortest-path distance from start to goal on its map, with the lower bounds on makespan and flowtime that
follow; heuristic_orders() ranks planning orders from them on the device (longest first, shortest first, hashed);
priorities='longest_first' | 'shortest_first' | 'mixed' of solve / solve_team enqueue both ahead of the solve on the
same stream; maxstep_from_distances() turns the makespan bound into a rollout's step limit.

The checker of all of it (include/gnnpp_mapf_audit.h, csrc/mapf_audit_kernels.hip): audit() says of any schedule in the
solvers' layout -- their own, or another solver's read from a file -- whether it is a legal, collision-free plan that
ends on the goals, with the agents' arrivals, the costs, the offences counted per class and the first one named;
Solutions.audit() audits a call's own answer, quality() sets the costs against the distances' lower bounds.
"""
import ctypes

import numpy as np
import torch

from . import _native

MAX_AGENTS, MAX_SIDE, MAX_STEPS = _native.ROLLOUT_MAX_AGENTS, _native.MAPF_MAX_SIDE, _native.MAPF_MAX_STEPS
MAX_TEAM, MAX_TEAM_SIDE, MAX_TEAM_STEPS = (_native.ROLLOUT_MAX_TEAM, _native.MAPF_TEAM_MAX_SIDE,      # (solve_team)
                                           _native.MAPF_TEAM_MAX_STEPS)
NO_PATH, BAD_CASE = _native.MAPF_NO_PATH, _native.MAPF_BAD_CASE
UNREACHABLE, INVALID = _native.MAPF_DIST_UNREACHABLE, _native.MAPF_DIST_INVALID         # (negative entries of dist)
AUDIT_CHUNK = _native.MAPF_AUDIT_CHUNK
AUDIT_STATE, AUDIT_VERTEX, AUDIT_MOVE, AUDIT_SWAP = (_native.MAPF_AUDIT_STATE, _native.MAPF_AUDIT_VERTEX,
                                                     _native.MAPF_AUDIT_MOVE, _native.MAPF_AUDIT_SWAP)
AUDIT_BAD_START, AUDIT_NOT_AT_GOAL, AUDIT_SKIPPED = (_native.MAPF_AUDIT_BAD_START, _native.MAPF_AUDIT_NOT_AT_GOAL,
                                                     _native.MAPF_AUDIT_SKIPPED)
AUDIT_CLASSES = ('a state off the map or on an obstacle', 'a vertex conflict', 'a move that is not one of the five actions',
                 'a swap conflict')                      # by GNNPP_MAPF_AUDIT_CLASS_*
ORDER_RULES = {'index': _native.MAPF_ORDER_INDEX, 'longest_first': _native.MAPF_ORDER_LONGEST_FIRST,
               'shortest_first': _native.MAPF_ORDER_SHORTEST_FIRST, 'hashed': _native.MAPF_ORDER_HASHED}


class Solutions:
    """Device tensors of one solve call: schedules [C,T+1,N,2] int32 (agents wait on their goal after arriving; -1 for
    agents left unplanned), arrival [C,N], makespan / flowtime / status / failing / restart [C] int32 (-1 where they do
    not apply), and the workspace.  Of a call with priorities given as a string also distance [C,N], lower_makespan and
    lower_flowtime [C] (see distances()) and priorities [C,R,N], the orders that were planned."""

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

    def audit(self):
        """The call's own schedules audited against the inputs it was given (kept in _keep), rows 0 .. makespan of every
        solved case; an unsolved case (makespan -1) is reported as AUDIT_SKIPPED.  Enqueued behind the solve on the same
        stream.  Returns Audit."""
        grid, start, goal = self._keep[:3]
        C, T1, N = (int(v) for v in self.schedules.shape[:3])
        out = empty_audit(C, N, T1 - 1, self.schedules.device)
        out._keep = (self,)
        enqueue_audit(grid, start, goal, self.schedules, self.makespan, out)
        return out


class Audit:
    """Device tensors of one audit call, all int32: status [C] (0: a legal, collision-free plan that ends on the goals;
    else the OR of AUDIT_STATE, AUDIT_VERTEX, AUDIT_MOVE, AUDIT_SWAP, AUDIT_BAD_START, AUDIT_NOT_AT_GOAL, AUDIT_SKIPPED),
    arrival [C,N], makespan / flowtime [C] (-1 when an agent does not end on its goal), counts [C,4] (flagged (step,
    agent) pairs per class: state, vertex, move, swap), first [C,4] = (t, class, agent, other) of the first offence (-1
    when there is none), and the workspace."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return int(self.status.shape[0])

    def ok(self):
        """bool [C] on the host: the case's schedule is a legal, collision-free plan that ends on the goals."""
        return (self.status == 0).cpu().numpy()

    def describe(self, c):
        """One line on case c: what was found first, where, and between whom."""
        st = int(self.status[c])
        if st == 0:
            return 'case %d: a legal, collision-free plan (makespan %d, flowtime %d)' % (
                c, int(self.makespan[c]), int(self.flowtime[c]))
        if st & AUDIT_SKIPPED:
            return 'case %d: skipped (no schedule to audit)' % c
        parts = []
        t, cls, agent, other = (int(v) for v in self.first[c].cpu().tolist())
        if cls >= 0:
            parts.append('%s at t = %d: agent %d%s (%s flagged)' % (
                AUDIT_CLASSES[cls], t, agent, ' and agent %d' % other if other >= 0 else '',
                ', '.join('%d x %s' % (n, w) for n, w in zip(self.counts[c].cpu().tolist(),
                                                            ('state', 'vertex', 'move', 'swap')) if n)))
        if st & AUDIT_BAD_START:
            parts.append('an agent does not begin on its start')
        if st & AUDIT_NOT_AT_GOAL:
            away = (self.arrival[c] < 0).nonzero().flatten().tolist()
            parts.append('agent %d does not end on its goal (%d agent(s))' % (away[0], len(away)))
        return 'case %d: %s (status %d)' % (c, '; '.join(parts), st)


def workspace_bytes(C, R, H, T):
    n = _native.lib().gnnpp_mapf_workspace_bytes(int(C), int(R), int(H), int(T))
    if n == 0:
        raise _native.GnnppError('no MAPF workspace for C=%d R=%d H=%d T_max=%d' % (C, R, H, T))
    return n


_workspace_bytes = workspace_bytes      # (empty_solutions has a parameter of that name)


def team_workspace_bytes(C, R, H, W, T):
    """Workspace of a solve_team call with a slot for each of its min(C R, 256) workgroups.  enqueue_solve_team takes
    any workspace that holds the summary and at least one slot (team_workspace_min_bytes) and plans as many items at a
    time as slots fit."""
    n = _native.lib().gnnpp_mapf_team_workspace_bytes(int(C), int(R), int(H), int(W), int(T))
    if n == 0:
        raise _native.GnnppError('no MAPF team workspace for C=%d R=%d H=%d W=%d T_max=%d' % (C, R, H, W, T))
    return n


def team_slot_bytes(H, W, T):
    """One workspace slot: six planes of H ceil(W / 64) 64-bit words per time step 0 .. T."""
    return (int(T) + 1) * 6 * int(H) * ((int(W) + 63) // 64) * 8


def team_workspace_min_bytes(C, R, H, W, T):
    """The summary and one slot: the smallest workspace enqueue_solve_team accepts."""
    return team_workspace_bytes(C, R, H, W, T) - (min(int(C) * int(R), 256) - 1) * team_slot_bytes(H, W, T)


def empty_solutions(C, N, H, T, device, restarts=1, W=None, team=False, workspace_bytes=None):
    """Output tensors and workspace of a call on C cases of N agents, maps of H rows, horizon T, `restarts` orders.
    team=True: for enqueue_solve_team (W, the maps' columns, is needed then); workspace_bytes: its workspace, at least
    team_workspace_min_bytes (default: team_workspace_bytes, a slot per workgroup)."""
    dev = torch.device(device)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)
    if team:
        if W is None:
            raise _native.GnnppError('empty_solutions(team=True) needs W, the number of map columns')
        nbytes = team_workspace_bytes(C, restarts, H, W, T)
        if workspace_bytes is not None:
            least = team_workspace_min_bytes(C, restarts, H, W, T)
            if int(workspace_bytes) < least:
                raise _native.GnnppError('workspace_bytes = %d holds no slot: at least %d bytes' % (workspace_bytes, least))
            nbytes = min(nbytes, int(workspace_bytes))
    else:
        if workspace_bytes is not None:
            raise _native.GnnppError('workspace_bytes applies to team=True only')
        nbytes = _workspace_bytes(C, restarts, H, T)
    return Solutions(schedules=i32(C, T + 1, N, 2), arrival=i32(C, N), makespan=i32(C), flowtime=i32(C),
                     status=i32(C), failing=i32(C), restart=i32(C),
                     workspace=torch.empty(nbytes, dtype=torch.uint8, device=dev))


def enqueue_solve(grid, start, goal, order, out, _team=False):
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
    name = 'gnnpp_mapf_team_solve' if _team else 'gnnpp_mapf_solve'
    with _native.device_guard(dev):
        _native.check(getattr(_native.lib(), name)(ctypes.byref(m), _native.stream_ptr(dev)), name)


def enqueue_solve_team(grid, start, goal, order, out):
    """enqueue_solve for teams of up to MAX_TEAM agents on maps of up to MAX_TEAM_SIDE rows and columns
    (gnnpp_mapf_team_solve); out: from empty_solutions(..., W=W, team=True)."""
    enqueue_solve(grid, start, goal, order, out, _team=True)


def audit_workspace_bytes(C, N, T):
    n = _native.lib().gnnpp_mapf_audit_workspace_bytes(int(C), int(N), int(T))
    if n == 0:
        raise _native.GnnppError('no audit workspace for C=%d N=%d T_max=%d' % (C, N, T))
    return n


def empty_audit(C, N, T, device):
    """Output tensors and workspace of enqueue_audit on C cases of N agents with schedules of T + 1 rows."""
    dev = torch.device(device)
    nbytes = audit_workspace_bytes(C, N, T)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)
    return Audit(status=i32(C), arrival=i32(C, N), makespan=i32(C), flowtime=i32(C), counts=i32(C, 4), first=i32(C, 4),
                 workspace=torch.empty(nbytes, dtype=torch.uint8, device=dev))


def enqueue_audit(grid, start, goal, schedule, steps, out):
    """gnnpp_mapf_audit alone, on torch's current stream of the tensors' device: two launches, no allocation, no host
    synchronisation, capturable in a HIP graph.  grid uint8 [C,H,W] | [H,W]; start int32 [C,N,2] or None (no start
    check); goal int32 [C,N,2]; schedule int32 [C,T+1,N,2]; steps int32 [C] or None (the last row of each case that
    counts; negative: the case is skipped); out: from empty_audit.  All contiguous device tensors."""
    dev = _native.require_gpu(grid, start, goal, schedule, steps, out.status, out.arrival, out.makespan, out.flowtime,
                              out.counts, out.first, out.workspace)
    C, T1, N = (int(v) for v in schedule.shape[:3])
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_mapf_audit(
            grid.data_ptr(), int(grid.dim() == 3), start.data_ptr() if start is not None else None, goal.data_ptr(),
            schedule.data_ptr(), steps.data_ptr() if steps is not None else None, C, N, int(grid.shape[-2]),
            int(grid.shape[-1]), T1 - 1, out.status.data_ptr(), out.arrival.data_ptr(), out.makespan.data_ptr(),
            out.flowtime.data_ptr(), out.counts.data_ptr(), out.first.data_ptr(), out.workspace.data_ptr(),
            out.workspace.numel(), _native.stream_ptr(dev)), 'gnnpp_mapf_audit')


def audit(grids, starts, goals, schedules, device, steps=None):
    """Audit C schedules: grids [C,H,W] or [H,W] (1 = obstacle), starts [C,N,2] or None (no start check), goals [C,N,2]
    (row, col), host or device, with solve_team's checks and limits.  schedules: a [C,T+1,N,2] tensor or array (steps:
    None, or [C] integers -- the last row of each case that counts, negative to skip the case), or a list of C arrays
    [T_c,N,2] (what expert.read_solution and Solutions.schedule return), padded to the longest with steps = T_c - 1.
    Returns Audit; offences are reported in .status / .counts / .first, never raised."""
    if isinstance(schedules, (list, tuple)):
        if steps is not None:
            raise _native.GnnppError('mapf.audit: steps come from the lengths of a list of schedules; pass steps=None')
        rows = [_int32(s) for s in schedules]
        for c, s in enumerate(rows):
            if s.dim() != 3 or s.shape[0] < 1 or s.shape[2] != 2 or s.shape[1] != rows[0].shape[1]:
                raise _native.GnnppError('schedule %d must be [T,N,2] with T >= 1 and the N of schedule 0 (got %s)'
                                         % (c, tuple(s.shape)))
        if not rows:
            raise _native.GnnppError('mapf.audit: an empty list of schedules')
        steps = torch.tensor([int(s.shape[0]) - 1 for s in rows], dtype=torch.int32)
        sched = torch.zeros((len(rows), int(steps.max()) + 1) + tuple(rows[0].shape[1:]), dtype=torch.int32,
                            device=rows[0].device)
        for c, s in enumerate(rows):
            sched[c, :s.shape[0]] = s.to(sched.device)
    else:
        sched = _int32(schedules)
    goal = _int32(goals)
    if sched.dim() != 4 or sched.shape[3] != 2 or sched.shape[1] < 1 or goal.dim() != 3 or \
            tuple(sched.shape[0:1] + sched.shape[2:]) != tuple(goal.shape):
        raise _native.GnnppError('schedules must be [C,T+1,N,2] with goals [C,N,2] (got %s and %s)'
                                 % (tuple(sched.shape), tuple(goal.shape)))
    dev, g, start, goal, C, N, H, W = _inputs('mapf.audit', MAX_TEAM, MAX_TEAM_SIDE, grids, goal if starts is None else starts,
                                              goal, device)
    T = int(sched.shape[1]) - 1
    if T > MAX_TEAM_STEPS:
        raise _native.GnnppError('schedules of at most %d steps (got %d)' % (MAX_TEAM_STEPS, T))
    if steps is not None:
        steps = _int32(steps)
        if tuple(steps.shape) != (C,):
            raise _native.GnnppError('steps must be [C] = [%d] (got %s)' % (C, tuple(steps.shape)))
        steps = steps.contiguous().to(dev)
    grid, start, goal = _on_device(dev, g, start, goal)
    if starts is None:
        start = None
    sched = sched.contiguous().to(dev)
    out = empty_audit(C, N, T, dev)
    out._keep = (grid, start, goal, sched, steps)        # inputs of the enqueued launches
    enqueue_audit(grid, start, goal, sched, steps, out)
    return out


def quality(audit_or_solutions, distances):
    """(flowtime / lower_flowtime, makespan / lower_makespan): float64 [C] each, on the device, of an Audit or a Solutions
    against a Distances (or anything with .lower_flowtime / .lower_makespan, such as the Solutions of a solve with
    priorities given as a string); NaN where either side is negative (unsolved, skipped, no path).  A lower bound of 0
    (every agent starts on its goal) gives 1 for a cost of 0 and inf otherwise.  No host synchronisation."""
    def ratio(cost, bound):
        c, b = cost.to(torch.float64), bound.to(torch.float64)
        r = torch.where((c == 0) & (b == 0), torch.ones_like(c), c / b)
        return torch.where((c < 0) | (b < 0), torch.full_like(c, float('nan')), r)
    return (ratio(audit_or_solutions.flowtime, distances.lower_flowtime),
            ratio(audit_or_solutions.makespan, distances.lower_makespan))


def _int32(x):
    return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(torch.int32)


class Distances:
    """Device tensors of one distances() call: dist [C,N] int32 (UNREACHABLE = -1: no path; INVALID = -2: start or goal
    off the map or on an obstacle), lower_makespan / lower_flowtime [C] int32 (max / sum of the case's distances, -1 when
    one of them is negative).  Unpacks as (dist, lower_makespan, lower_flowtime)."""

    def __init__(self, dist, lower_makespan, lower_flowtime):
        self.dist, self.lower_makespan, self.lower_flowtime = dist, lower_makespan, lower_flowtime

    def __iter__(self):
        return iter((self.dist, self.lower_makespan, self.lower_flowtime))


def enqueue_distances(grid, start, goal, out):
    """gnnpp_mapf_distances alone, on torch's current stream: two launches, no allocation, no host synchronisation,
    capturable.  grid uint8 [C,H,W] | [H,W]; start, goal int32 [C,N,2]; out: a Distances of int32 tensors ([C,N], [C],
    [C]).  All contiguous device tensors."""
    dev = _native.require_gpu(grid, start, goal, out.dist, out.lower_makespan, out.lower_flowtime)
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_mapf_distances(
            grid.data_ptr(), int(grid.dim() == 3), start.data_ptr(), goal.data_ptr(), int(start.shape[0]),
            int(start.shape[1]), int(grid.shape[-2]), int(grid.shape[-1]), out.dist.data_ptr(),
            out.lower_makespan.data_ptr(), out.lower_flowtime.data_ptr(), _native.stream_ptr(dev)), 'gnnpp_mapf_distances')


def enqueue_orders(dist, rules, seed, order):
    """gnnpp_mapf_orders alone, on torch's current stream: order [C,R,N] int32 := the agents of every case ranked by
    each of the R rules (codes of ORDER_RULES) from the keys dist [C,N] int32.  One launch per 32 rules, capturable."""
    dev = _native.require_gpu(dist, order)
    C, R, N = (int(v) for v in order.shape)
    codes = (ctypes.c_int * R)(*[int(r) for r in rules])
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_mapf_orders(dist.data_ptr(), C, N, R, codes, int(seed) & 0xffffffff,
                                                      order.data_ptr(), _native.stream_ptr(dev)), 'gnnpp_mapf_orders')


def _rule_codes(rules):
    if isinstance(rules, str):
        rules = [rules]
    rules = list(rules)
    unknown = [r for r in rules if r not in ORDER_RULES]
    if unknown or not rules:
        raise _native.GnnppError('rules: a non-empty sequence of %s (got %r)' % (sorted(ORDER_RULES), unknown or rules))
    return [ORDER_RULES[r] for r in rules]


def distances(grids, starts, goals, device):
    """Every agent's true distance to its goal: grids [C,H,W] or [H,W] (1 = obstacle), starts / goals [C,N,2] (row,
    col), host or device, with solve_team's checks and limits.  Returns Distances (dist, lower_makespan, lower_flowtime
    on the device); agents without a path or with an invalid start / goal are reported in dist, never raised."""
    dev, g, start, goal, C, N, H, W = _inputs('mapf.distances', MAX_TEAM, MAX_TEAM_SIDE, grids, starts, goals, device)
    return _distances(*_on_device(dev, g, start, goal))


def _distances(grid, start, goal):
    C, N = int(start.shape[0]), int(start.shape[1])
    out = Distances(*(torch.empty(shape, dtype=torch.int32, device=start.device) for shape in ((C, N), (C,), (C,))))
    enqueue_distances(grid, start, goal, out)
    return out


def heuristic_orders(dist, rules, seed=0):
    """Planning orders [C,R,N] int32 on the device, one per rule of `rules` ('index' | 'longest_first' |
    'shortest_first' | 'hashed'), ranked from dist [C,N] (distances().dist, or any integer keys; a device tensor).
    longest_first / shortest_first: by distance descending / ascending, agents with a negative distance first; hashed:
    by a counter hash of (seed, case, restart, agent); every tie goes to the lower agent index."""
    codes = _rule_codes(rules)
    if not torch.is_tensor(dist) or dist.dim() != 2 or not 1 <= dist.shape[1] <= MAX_TEAM or dist.shape[0] < 1:
        raise _native.GnnppError('dist must be a [C,N] device tensor with 1 <= N <= %d' % MAX_TEAM)
    _native.require_gpu(dist)
    dist = dist.to(torch.int32).contiguous()
    order = torch.empty((dist.shape[0], len(codes), dist.shape[1]), dtype=torch.int32, device=dist.device)
    enqueue_orders(dist, codes, seed, order)
    return order


def maxstep_from_distances(lower_makespan, rate):
    """int32 [C]: ceil(rate * lower_makespan) (the product in float64), at least 1 -- a per-episode step limit for
    BatchedRollout(maxstep=...) where no expert makespan exists yet (the reference: rate_maxstep * the expert's makespan).
    Raises GnnppError when a case has an agent without a path or with an invalid start / goal (lower_makespan < 0)."""
    lm = lower_makespan if torch.is_tensor(lower_makespan) else torch.as_tensor(np.asarray(lower_makespan))
    if not float(rate) > 0:
        raise _native.GnnppError('rate must be positive (got %r)' % (rate,))
    bad = (lm < 0).nonzero().flatten().tolist()
    if bad:
        raise _native.GnnppError('no step limit for cases %s: an agent cannot reach its goal' % bad[:8])
    return torch.ceil(lm.to(torch.float64) * float(rate)).clamp_(min=1).to(torch.int32)


def solve(grids, starts, goals, device, max_steps=None, restarts=1, priorities=None, seed=0):
    """Plan C cases: grids [C,H,W] or [H,W] (1 = obstacle), starts / goals [C,N,2] (row, col), host or device.
    max_steps: the horizon T_max (default 4 (H + W)).  priorities: planning orders [C,R,N] or [R,N] (shared by the
    cases), permutations of the agents; by default restart 0 is the index order and restarts 1 .. restarts-1 are
    random permutations drawn from numpy's default_rng(seed).  priorities as a string: the orders are ranked on the
    device from the agents' true goal distances, enqueued ahead of the solve on the same stream (distances(),
    heuristic_orders()) -- 'longest_first' / 'shortest_first': that one order; 'mixed': max(restarts, 3) orders, the
    index order, longest first, shortest first, the rest hashed with `seed`; the Solutions then carry .distance,
    .lower_makespan, .lower_flowtime and .priorities.  Returns Solutions; unsolved and invalid cases are reported in
    .status (NO_PATH, BAD_CASE), never raised."""
    return _solve('mapf.solve', False, MAX_AGENTS, MAX_SIDE, MAX_STEPS, grids, starts, goals, device, max_steps,
                  restarts, priorities, seed, None)


def solve_team(grids, starts, goals, device, max_steps=None, restarts=1, priorities=None, seed=0, workspace_bytes=None):
    """solve() for teams of up to MAX_TEAM agents on maps of up to MAX_TEAM_SIDE x MAX_TEAM_SIDE cells and horizons of
    up to MAX_TEAM_STEPS (csrc/mapf_team_kernels.hip): the same arguments, default orders, Solutions and, for a case
    both accept, the same outputs.  workspace_bytes: a cap on the workspace (default: a slot for each of the call's
    min(C R, 256) workgroups -- 12.6 MB per slot at 128 x 128 and T_max = 1024, 100.7 MB at 256 x 256 and 2048); with
    less, fewer items are planned at a time, with the same results; less than one slot raises GnnppError."""
    return _solve('mapf.solve_team', True, MAX_TEAM, MAX_TEAM_SIDE, MAX_TEAM_STEPS, grids, starts, goals, device,
                  max_steps, restarts, priorities, seed, workspace_bytes)


def default_orders(C, N, restarts, seed):
    """[C,restarts,N] int64: restart 0 the index order, the others permutations from numpy's default_rng(seed)."""
    rng = np.random.default_rng(seed)
    perm = np.argsort(rng.random((C, int(restarts) - 1, N)), axis=-1)
    return np.concatenate([np.broadcast_to(np.arange(N), (C, 1, N)), perm], 1)


def _inputs(what, max_agents, max_side, grids, starts, goals, device):
    """The checks of a call's inputs, on the host: (dev, grids, starts, goals as tensors, C, N, H, W)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('%s needs a HIP device (no CPU fallback)' % what)
    g = grids if torch.is_tensor(grids) else torch.as_tensor(np.asarray(grids))
    start, goal = _int32(starts), _int32(goals)
    if start.dim() != 3 or start.shape[2] != 2 or tuple(goal.shape) != tuple(start.shape) or start.shape[0] < 1:
        raise _native.GnnppError('starts and goals must both be [C,N,2] with C >= 1 (got %s and %s)'
                                 % (tuple(start.shape), tuple(goal.shape)))
    C, N = int(start.shape[0]), int(start.shape[1])
    if not 1 <= N <= max_agents:
        raise _native.GnnppError('teams of 1 to %d agents (got %d)' % (max_agents, N))
    if g.dim() not in (2, 3) or (g.dim() == 3 and g.shape[0] != C):
        raise _native.GnnppError('grids must be [H,W] or [C,H,W] with one map per case')
    H, W = int(g.shape[-2]), int(g.shape[-1])
    if not (1 <= H <= max_side and 1 <= W <= max_side):
        raise _native.GnnppError('maps of at most %d x %d cells (got %d x %d)' % (max_side, max_side, H, W))
    return dev, g, start, goal, C, N, H, W


def _on_device(dev, g, start, goal):
    """The checked inputs as contiguous device tensors (grid uint8, start, goal int32)."""
    _native.lib()
    return g.to(torch.uint8).contiguous().to(dev), start.contiguous().to(dev), goal.contiguous().to(dev)


def _solve(what, team, max_agents, max_side, max_steps_limit, grids, starts, goals, device, max_steps, restarts,
           priorities, seed, workspace_bytes):
    dev, g, start, goal, C, N, H, W = _inputs(what, max_agents, max_side, grids, starts, goals, device)
    T = 4 * (H + W) if max_steps is None else int(max_steps)
    if not 0 <= T <= max_steps_limit:
        raise _native.GnnppError('max_steps must be in 0 .. %d (got %d)' % (max_steps_limit, T))
    order, dist, rules = None, None, None
    if isinstance(priorities, str):
        if int(restarts) < 1:
            raise _native.GnnppError('restarts must be >= 1 (got %d)' % restarts)
        if priorities == 'mixed':
            rules = (['index', 'longest_first', 'shortest_first'] + ['hashed'] * (int(restarts) - 3))
        elif priorities in ('longest_first', 'shortest_first'):
            rules = [priorities]
        else:
            raise _native.GnnppError("priorities as a string: 'longest_first', 'shortest_first' or 'mixed' (got %r)"
                                     % priorities)
    elif priorities is not None:
        order = _int32(priorities)
        if order.dim() == 2:
            order = order.unsqueeze(0).expand(C, -1, -1)
        if order.dim() != 3 or order.shape[0] != C or order.shape[2] != N or order.shape[1] < 1:
            raise _native.GnnppError('priorities must be [C,R,N] or [R,N] (C = %d, N = %d), got %s'
                                     % (C, N, tuple(order.shape)))
    elif int(restarts) > 1:
        order = torch.from_numpy(default_orders(C, N, restarts, seed)).to(torch.int32)
    elif int(restarts) < 1:
        raise _native.GnnppError('restarts must be >= 1 (got %d)' % restarts)
    grid, start, goal = _on_device(dev, g, start, goal)
    if rules is not None:                               # enqueued ahead of the solve, on the same stream
        dist = _distances(grid, start, goal)
        order = heuristic_orders(dist.dist, rules, seed)
    R = 1 if order is None else int(order.shape[1])
    order = order.contiguous().to(dev) if order is not None else None
    if team:
        out = empty_solutions(C, N, H, T, dev, R, W=W, team=True, workspace_bytes=workspace_bytes)
    else:
        out = empty_solutions(C, N, H, T, dev, R)
    out._keep = (grid, start, goal, order)              # inputs of the enqueued launches
    if dist is not None:
        out.distance, out.lower_makespan, out.lower_flowtime = dist.dist, dist.lower_makespan, dist.lower_flowtime
        out.priorities = order
    enqueue_solve(grid, start, goal, order, out, _team=team)
    return out
