"""Training samples from expert schedules, on the device: the data side of the reference's "online expert" loop.

    rollout (BatchedRollout) -> write_failure_cases -> any MAPF solver -> read_solution -> samples_from_schedules
        -> SamplePool.draw -> training.train_step

What the reference does with utils/multirobotsim_dcenlocal_onlineExpert.py::save_failure_cases (:705-730), the ECBS
binary, and the four-process transformer onlineExpert/DataTransformer_local_onlineExpert.py (the offline
offlineExpert/DataGen_Transformer.py:295-371, 466-515 computes the same tensors).  The solver stays outside; everything
around it is here.  The tensors come from ONE gnnpp_schedule_samples call for all cases (csrc/expert_kernels.hip),
bit-exact with the reference; there is no CPU fallback.  Teams of up to MAX_TEAM = 1024 agents go through
samples_from_schedules_team: ONE gnnpp_schedule_team_samples call (csrc/expert_team_kernels.hip), the same tensors.
The prioritized expert itself runs on the device too (mapf.py): solve_failures plans the failed episodes of a rollout
and samples_from_solutions turns the solved ones into samples (team=True: teams of any size up to MAX_TEAM).
Large teams can keep their graphs as neighbour lists from the schedule to the training step, with no [N,N] matrix in
between: samples_from_schedules_team(graph='lists') -> SampleListPool.draw -> training.train_step_lists.
The pools above keep every step's tensors.  SchedulePool keeps the schedules and builds each batch when it is drawn
(gnnpp_schedule_draw, csrc/schedule_draw_kernels.hip), the same bytes from a hundredth of the memory:

    ... -> mapf.solve -> SchedulePool.append_solutions -> SchedulePool.draw -> train_step

The schedule's communication radius is NOT the rollout's: it starts at commR (5 in both transformers), grows by
* 1.1 until every step of the case is connected, and the final radius builds every step's graph.
Positions are (row, col) integers: the reference's (x, y).
"""
import ctypes
import os

import numpy as np
import torch

from . import _native, formats

MAX_AGENTS, MAX_TEAM = _native.ROLLOUT_MAX_AGENTS, _native.ROLLOUT_MAX_TEAM
BAD_MOVE, BAD_STATE, NO_RADIUS = _native.SCHEDULE_BAD_MOVE, _native.SCHEDULE_BAD_STATE, _native.SCHEDULE_NO_RADIUS


class ScheduleSamples:
    """Device tensors of one samples_from_schedules call: input [T,N,3,11,11] f32, GSO [T,N,N] f32, GSO64 (f64 or
    None), target [T,N,5] f32, case_start [C+1] i32, radius [C] f64, growth [C] i32, step_growth [T] i32 (the growths
    each step needs on its own).
    With graph='lists' (samples_from_schedules_team) GSO and GSO64 are None and the graphs are a capped lists set
    (include/gnnpp.h): cnt [T,N] i32, idx [T,N,cap] (uint16 row indices held in an int16 tensor: torch concatenates
    those), val [T,N,cap] f32, cap, and step_deg [T] i32, the largest degree of each step."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getitem__(self, key):
        return self.__dict__[key]

    def __len__(self):
        return int(self.input.shape[0])

    def case(self, c):
        """(input, GSO, target) views of case c."""
        a, b = self.bounds[c], self.bounds[c + 1]
        if self.GSO is None:                            # graph='lists': (cnt, idx, val) in the place of the GSO
            return self.input[a:b], (self.cnt[a:b], self.idx[a:b], self.val[a:b]), self.target[a:b]
        return self.input[a:b], self.GSO[a:b], self.target[a:b]


def enqueue_schedule_samples(grid, goal, pos, case_start, out, commR=5.0):
    """The native call alone, on torch's current stream of the tensors' device: no allocation, no host
    synchronisation, capturable in a HIP graph.  grid uint8 [C,H,W] | [H,W], goal [C,N,2] / pos [T,N,2] / case_start
    [C+1] int32, all contiguous device tensors; out: a ScheduleSamples whose tensors match.  out.step_growth receives
    the raw per-step word (growths | status bits << 16) and out.status the per-case bits: the caller checks them."""
    dev = _native.require_gpu(grid, goal, pos, case_start, out.input, out.GSO, out.target)
    s = _schedule_struct(grid, goal, pos, case_start, out, commR)
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_schedule_samples(ctypes.byref(s), _native.stream_ptr(dev)),
                      'gnnpp_schedule_samples')


def _schedule_struct(grid, goal, pos, case_start, out, commR):
    s = _native.ScheduleStruct()
    s.grid, s.grid_batched, s.goal, s.pos = grid.data_ptr(), int(grid.dim() == 3), goal.data_ptr(), pos.data_ptr()
    s.case_start, s.C, s.N = case_start.data_ptr(), int(goal.shape[0]), int(goal.shape[1])
    s.H, s.W, s.T_total = int(grid.shape[-2]), int(grid.shape[-1]), int(pos.shape[0])
    s.radius0 = float(commR)
    ptr = lambda t: t.data_ptr() if t is not None else None                     # noqa: E731
    s.obs, s.S, s.target = ptr(out.input), ptr(out.GSO), out.target.data_ptr()
    s.S64 = ptr(out.GSO64)
    s.radius, s.growth, s.status = out.radius.data_ptr(), out.growth.data_ptr(), out.status.data_ptr()
    s.step_info = out.step_growth.data_ptr()
    return s


def enqueue_schedule_team_samples(grid, goal, pos, case_start, out, commR=5.0):
    """enqueue_schedule_samples for teams of 2 to MAX_TEAM agents: gnnpp_schedule_team_samples alone, same arguments,
    same outputs; out.workspace: a contiguous device tensor of at least gnnpp_schedule_team_workspace_bytes(N, T)
    bytes (any contents)."""
    dev = _native.require_gpu(grid, goal, pos, case_start, out.input, out.GSO, out.target, out.workspace)
    s = _schedule_struct(grid, goal, pos, case_start, out, commR)
    ws = out.workspace
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_schedule_team_samples(ctypes.byref(s), ws.data_ptr(),
                                                                ws.numel() * ws.element_size(), _native.stream_ptr(dev)),
                      'gnnpp_schedule_team_samples')


def enqueue_schedule_team_plan(grid, goal, pos, case_start, out, commR=5.0):
    """gnnpp_schedule_team_plan alone (arguments as enqueue_schedule_team_samples): target, radius, growth, status,
    step_growth and the workspace as that call writes them, and out.step_deg [T] int32, the largest degree of each step.
    out.input / out.GSO / out.GSO64 may be None.  No allocation, no host synchronisation, capturable."""
    dev = _native.require_gpu(grid, goal, pos, case_start, out.target, out.workspace, out.step_deg)
    s = _schedule_struct(grid, goal, pos, case_start, out, commR)
    ws = out.workspace
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_schedule_team_plan(ctypes.byref(s), ws.data_ptr(), ws.numel() * ws.element_size(),
                                                             out.step_deg.data_ptr(), _native.stream_ptr(dev)),
                      'gnnpp_schedule_team_plan')


def enqueue_schedule_team_fill_lists(grid, goal, pos, case_start, out, commR=5.0):
    """gnnpp_schedule_team_fill_lists alone, after enqueue_schedule_team_plan on the same `out`: out.input and the capped
    lists out.cnt [T,N] int32, out.idx [T,N,cap] int16 (read as uint16), out.val [T,N,cap] float32 with out.cap.  No dense
    GSO is written.  No allocation, no host synchronisation, capturable."""
    dev = _native.require_gpu(grid, goal, pos, case_start, out.input, out.workspace, out.cnt, out.idx, out.val)
    s = _schedule_struct(grid, goal, pos, case_start, out, commR)
    ws = out.workspace
    T, N, cap = int(pos.shape[0]), int(pos.shape[1]), int(out.cap)
    if (tuple(out.cnt.shape) != (T, N) or out.cnt.dtype is not torch.int32 or tuple(out.idx.shape) != (T, N, cap)
            or out.idx.dtype is not torch.int16 or tuple(out.val.shape) != (T, N, cap) or out.val.dtype is not torch.float32
            or not (out.cnt.is_contiguous() and out.idx.is_contiguous() and out.val.is_contiguous())):
        raise _native.GnnppError('capped lists of %d steps of %d agents at cap %d: contiguous cnt [T,N] int32, idx [T,N,cap] '
                                 'int16 and val [T,N,cap] float32' % (T, N, cap))
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_schedule_team_fill_lists(
            ctypes.byref(s), ws.data_ptr(), ws.numel() * ws.element_size(), out.cnt.data_ptr(), out.idx.data_ptr(),
            out.val.data_ptr(), cap, _native.stream_ptr(dev)), 'gnnpp_schedule_team_fill_lists')


def team_lists_output_bytes(T_total, N, cap):
    """Bytes of the input, target and capped-lists tensors of T_total steps of N agents: 1.7 MB per step at N = 1024 and
    cap = 24, of which the graph is 0.15 MB."""
    return T_total * N * (1452 + 20 + 4 + 6 * cap)


def team_output_bytes(T_total, N, keep_fp64_gso=False):
    """Bytes of the input, GSO and target tensors (+ the fp64 GSO) of T_total steps of N agents: 5.7 MB per step at
    N = 1024."""
    return T_total * N * (1452 + 4 * N + 20) + (8 * N * N * T_total if keep_fp64_gso else 0)


def samples_from_schedules(grids, goals, schedules, device, commR=5.0, keep_fp64_gso=False, audit=False):
    """grids [C,H,W] or [H,W] (1 = obstacle); goals [C,N,2]; schedules: list of C arrays [T_c,N,2] (states of a solved
    case, agents that arrived waiting on their goal) -> ScheduleSamples.  A schedule with a move that is not one of
    the five actions, or a state off the map / on an obstacle, raises GnnppError naming the case (the reference dies
    with ValueError there); this reads the per-case status back, the only host synchronisation.
    audit=True: the schedules first go through mapf.audit (without a start check), which also looks at two agents at once:
    a vertex or swap conflict, or an agent that does not end on its goal, raises GnnppError naming the case, the class,
    t and the agents before any sample is built (one more read of a status).  The default changes nothing."""
    return _samples_from_schedules(grids, goals, schedules, device, commR, keep_fp64_gso, False, audit=audit)


def samples_from_schedules_team(grids, goals, schedules, device, commR=5.0, keep_fp64_gso=False, graph='dense',
                                audit=False):
    """samples_from_schedules for teams of 2 to MAX_TEAM = 1024 agents on maps of up to 65 536 cells: same arguments,
    same ScheduleSamples (the same bytes for every team both take), same errors naming the bad case.  The outputs are
    team_output_bytes(T, N, keep_fp64_gso) bytes; a call that would not fit the device's free memory raises GnnppError
    with that figure before anything is allocated.
    graph='lists': the graphs are delivered as a capped lists set (ScheduleSamples.cnt / idx / val / cap / step_deg; GSO
    is None) and no [N,N] matrix is written: gnnpp_schedule_team_plan, the host read of the cases' status and the steps'
    largest degrees, cap = that maximum rounded up to 4, then gnnpp_schedule_team_fill_lists.  The outputs are
    team_lists_output_bytes(T, N, cap) bytes, checked against the free memory once cap is known.  SampleListPool takes
    the result.  keep_fp64_gso is refused.  audit=True: as for samples_from_schedules."""
    if graph not in ('dense', 'lists'):
        raise _native.GnnppError("unknown graph %r (one of ['dense', 'lists'])" % (graph,))
    if graph == 'lists' and keep_fp64_gso:
        raise _native.GnnppError("samples_from_schedules_team: graph='lists' keeps no dense GSO, keep_fp64_gso=True needs "
                                 "graph='dense'")
    return _samples_from_schedules(grids, goals, schedules, device, commR, keep_fp64_gso, True, graph == 'lists', audit=audit)


def _raise_if_flagged(bad, C):
    if bool((bad != 0).any()):
        c = int((bad != 0).nonzero()[0])
        what = [w for bit, w in ((BAD_MOVE, 'a move that is not one of the five actions'),
                                 (BAD_STATE, 'a state off the map or on an obstacle'),
                                 (NO_RADIUS, 'no radius connects the team')) if int(bad[c]) & bit]
        raise _native.GnnppError('schedule of case %d (of %d) cannot be transformed: %s (status %d; %d case(s) flagged)'
                                 % (c, C, ' and '.join(what), int(bad[c]), int((bad != 0).sum())))


def _raise_if_audit_flagged(found, C):
    status = found.status.cpu()
    if bool((status != 0).any()):
        c = int((status != 0).nonzero()[0])
        raise _native.GnnppError('schedule of case %d (of %d) fails its audit: %s; %d case(s) flagged'
                                 % (c, C, found.describe(c).split(': ', 1)[1], int((status != 0).sum())))


def _samples_from_schedules(grids, goals, schedules, device, commR, keep_fp64_gso, team, lists=False, audit=False):
    name = 'samples_from_schedules_team' if team else 'samples_from_schedules'
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('%s needs a HIP device (no CPU fallback)' % name)
    L = _native.lib()
    g = torch.as_tensor(np.asarray(grids) if not torch.is_tensor(grids) else grids)
    goal = torch.as_tensor(np.asarray(goals) if not torch.is_tensor(goals) else goals).to(torch.int32)
    C = len(schedules)
    if C == 0 or goal.dim() != 3 or goal.shape[0] != C or goal.shape[2] != 2:
        raise _native.GnnppError('goals must be [C,N,2] with one entry per schedule (C = %d)' % C)
    N = int(goal.shape[1])
    if g.dim() not in (2, 3) or (g.dim() == 3 and g.shape[0] != C):
        raise _native.GnnppError('grids must be [H,W] or [C,H,W]')
    most = MAX_TEAM if team else MAX_AGENTS
    if not 2 <= N <= most:
        raise _native.GnnppError('teams of 2 to %d agents (got %d)' % (most, N))
    sched = [torch.as_tensor(np.asarray(s) if not torch.is_tensor(s) else s).to(torch.int32) for s in schedules]
    for c, s in enumerate(sched):
        if s.dim() != 3 or s.shape[0] < 1 or tuple(s.shape[1:]) != (N, 2):
            raise _native.GnnppError('schedule %d must be [T,%d,2] with T >= 1 (got %s)' % (c, N, tuple(s.shape)))
    if audit:
        from . import mapf
        _raise_if_audit_flagged(mapf.audit(g, None, goal, sched, dev), C)
    bounds = [0]
    for s in sched:
        bounds.append(bounds[-1] + int(s.shape[0]))
    T = bounds[-1]
    workspace = None

    def must_fit(need):
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise _native.GnnppError('%s: the tensors of %d steps of %d agents take %d bytes (%.1f GB), the device has '
                                     '%d bytes free: pass fewer cases per call' % (name, T, N, need, need / 1e9, free))
    if team:
        # (lists: the graph's bytes are known once the plan has run; every column holds at least one group of four)
        must_fit(team_lists_output_bytes(T, N, 4) if lists else team_output_bytes(T, N, keep_fp64_gso))
        workspace = torch.empty(L.gnnpp_schedule_team_workspace_bytes(N, T), dtype=torch.uint8, device=dev)
    grid = g.to(torch.uint8).contiguous().to(dev)
    goal = goal.contiguous().to(dev)
    pos = torch.cat(sched, 0).contiguous().to(dev)
    case_start = torch.tensor(bounds, dtype=torch.int32).to(dev)
    if lists:
        flags = torch.empty(C + T, dtype=torch.int32, device=dev)        # status | step_deg: one read for both
        out = ScheduleSamples(
            input=None, GSO=None, GSO64=None, target=torch.empty(T, N, 5, dtype=torch.float32, device=dev),
            case_start=case_start, bounds=bounds, radius=torch.empty(C, dtype=torch.float64, device=dev),
            growth=torch.empty(C, dtype=torch.int32, device=dev), status=flags[:C], step_deg=flags[C:],
            step_growth=torch.empty(T, dtype=torch.int32, device=dev), workspace=workspace)
        out._keep = (grid, goal, pos)
        enqueue_schedule_team_plan(grid, goal, pos, case_start, out, commR)
        host = flags.cpu()
        _raise_if_flagged(host[:C], C)
        out.cap = max(4, (int(host[C:].max()) + 3) & ~3)
        must_fit(team_lists_output_bytes(T, N, out.cap) - T * N * 20)
        out.input = torch.empty(T, N, 3, 11, 11, dtype=torch.float32, device=dev)
        out.cnt = torch.empty(T, N, dtype=torch.int32, device=dev)
        out.idx = torch.empty(T, N, out.cap, dtype=torch.int16, device=dev)
        out.val = torch.empty(T, N, out.cap, dtype=torch.float32, device=dev)
        enqueue_schedule_team_fill_lists(grid, goal, pos, case_start, out, commR)
        out.step_growth &= 0xffff
        return out
    out = ScheduleSamples(
        input=torch.empty(T, N, 3, 11, 11, dtype=torch.float32, device=dev),
        GSO=torch.empty(T, N, N, dtype=torch.float32, device=dev),
        GSO64=torch.empty(T, N, N, dtype=torch.float64, device=dev) if keep_fp64_gso else None,
        target=torch.empty(T, N, 5, dtype=torch.float32, device=dev),
        case_start=case_start, bounds=bounds,
        radius=torch.empty(C, dtype=torch.float64, device=dev),
        growth=torch.empty(C, dtype=torch.int32, device=dev),
        status=torch.empty(C, dtype=torch.int32, device=dev),
        step_growth=torch.empty(T, dtype=torch.int32, device=dev))
    out._keep = (grid, goal, pos)                       # inputs of the enqueued launches
    if team:
        out.workspace = workspace
        enqueue_schedule_team_samples(grid, goal, pos, case_start, out, commR)
    else:
        enqueue_schedule_samples(grid, goal, pos, case_start, out, commR)
    out.step_growth &= 0xffff                           # (the status bits of a step live above; reported per case)
    _raise_if_flagged(out.status.cpu(), C)
    return out


# ---- the solver on the device (mapf.py) ---------------------------------------------------------------
def solve_failures(rollout, results=None, **kw):
    """Plan every episode of a BatchedRollout whose `success` is false, straight from its device state: the agents'
    final positions as starts, their goals, the episode's map (what write_failure_cases would put in the files).
    kw: mapf.solve's max_steps, restarts, priorities, seed -- priorities='longest_first' | 'shortest_first' | 'mixed'
    ranks the planning orders on the device from the agents' true goal distances (no host round trip; the Solutions then
    also carry .distance, .lower_makespan and .lower_flowtime).  Teams of more than mapf.MAX_AGENTS agents and maps with a
    side beyond mapf.MAX_SIDE go to mapf.solve_team (which also takes workspace_bytes), everything else to mapf.solve.
    Returns mapf.Solutions of those F episodes with `.episodes` (their indices in the rollout, numpy int64 [F]), or
    None when every episode succeeded.  samples_from_solutions turns them into training samples (team=True for teams
    of more than MAX_AGENTS agents)."""
    from . import mapf
    res = rollout.results() if results is None else results
    episodes = np.nonzero(~np.asarray(res['success'], dtype=bool))[0]
    if len(episodes) == 0:
        return None
    idx = torch.as_tensor(episodes, device=rollout.device)
    grid = rollout.grid.index_select(0, idx) if rollout.grid_batched else rollout.grid
    team = rollout.N > mapf.MAX_AGENTS or max(int(rollout.grid.shape[-2]), int(rollout.grid.shape[-1])) > mapf.MAX_SIDE
    sol = (mapf.solve_team if team else mapf.solve)(grid, rollout.pos.index_select(0, idx),
                                                    rollout.goal.index_select(0, idx), rollout.device, **kw)
    sol.episodes = episodes
    return sol


def samples_from_solutions(solutions, grids, goals, commR=5.0, team=False, graph='dense', audit=False):
    """(ScheduleSamples of the solved cases of a mapf.Solutions, their case ids numpy int64 [S]) through
    samples_from_schedules / enqueue_schedule_samples, or with team=True through samples_from_schedules_team (teams of
    up to MAX_TEAM agents, what mapf.solve_team plans; graph='lists' is passed on to it and needs team=True).
    grids [C,H,W] or [H,W] and goals [C,N,2]: the cases' maps and goals as solve() was given them (host or device).
    Unsolved cases are left out (their ids are missing from the list); (None, empty ids) when no case was solved.
    audit=True: the solved schedules are audited first, as for samples_from_schedules."""
    if not team and int(solutions.arrival.shape[1]) > MAX_AGENTS:
        raise _native.GnnppError('samples_from_solutions: samples are built for teams of at most %d agents; these '
                                 'solutions have %d (pass team=True: samples_from_schedules_team takes teams of up to '
                                 '%d agents)' % (MAX_AGENTS, solutions.arrival.shape[1], MAX_TEAM))
    if graph != 'dense' and not team:
        raise _native.GnnppError("samples_from_solutions: graph=%r needs team=True (samples_from_schedules_team builds the "
                                 "lists)" % (graph,))
    status = solutions.status.cpu().numpy()
    ids = np.nonzero(status == 0)[0]
    if len(ids) == 0:
        return None, ids
    dev = solutions.status.device
    makespan = solutions.makespan.cpu().numpy()
    idx = torch.as_tensor(ids, device=dev)
    g = grids if torch.is_tensor(grids) else torch.as_tensor(np.asarray(grids))
    g = g.to(dev).index_select(0, idx) if g.dim() == 3 else g
    gl = (goals if torch.is_tensor(goals) else torch.as_tensor(np.asarray(goals))).to(dev).index_select(0, idx)
    sched = [solutions.schedules[c, :int(makespan[c]) + 1] for c in ids]
    extra = {'audit': True} if audit else {}             # (the default call is the call it always was)
    if graph != 'dense':
        return samples_from_schedules_team(g, gl, sched, dev, commR=commR, graph=graph, **extra), ids
    return (samples_from_schedules_team if team else samples_from_schedules)(g, gl, sched, dev, commR=commR, **extra), ids


# ---- the files around the solver ---------------------------------------------------------------------
def failure_case_yaml(grid, positions, goals):
    """Text of save_failure_cases (multirobotsim_dcenlocal_onlineExpert.py:705-730) for one episode: map dimensions,
    obstacles in row-major order, per agent `start` = where it stood when the episode ended, and its goal."""
    grid = np.asarray(grid)
    out = ['map:\n', '    dimensions: {}\n'.format([int(grid.shape[0]), int(grid.shape[1])]), '    obstacles:\n']
    for x, y in np.argwhere(grid != 0):
        out.append('    - {}\n'.format([int(x), int(y)]))
    out.append('agents:\n')
    for n, (p, gl) in enumerate(zip(np.asarray(positions), np.asarray(goals))):
        out.append('  - name: agent{}\n    start: {}\n    goal: {}\n'.format(n, [int(p[0]), int(p[1])],
                                                                           [int(gl[0]), int(gl[1])]))
    return ''.join(out)


def write_failure_cases(directory, rollout, ids=None, results=None):
    """failureCases_ID{:05d}.yaml in `directory` for every episode of a BatchedRollout whose `success` is false.
    ids: the dataset ID of each episode (default: its index); results: rollout.results() if already at hand.
    Returns the list of (episode index, path) written."""
    res = rollout.results() if results is None else results
    grid, goal = rollout.grid.cpu().numpy(), rollout.goal.cpu().numpy()
    pos = np.asarray(res['positions'])
    ids = list(range(rollout.B)) if ids is None else [int(i) for i in ids]
    if len(ids) != rollout.B:
        raise _native.GnnppError('ids: one per episode (%d), got %d' % (rollout.B, len(ids)))
    os.makedirs(directory, exist_ok=True)
    written = []
    for b in range(rollout.B):
        if bool(res['success'][b]):
            continue
        path = os.path.join(directory, 'failureCases_ID{:05d}.yaml'.format(ids[b]))
        with open(path, 'w') as f:
            f.write(failure_case_yaml(grid[b] if rollout.grid_batched else grid, pos[b], goal[b]))
        written.append((b, path))
    return written


def write_prediction_cases(directory, rollout, ids=None, results=None):
    """The predicted schedule of every episode of a RECORDED rollout (BatchedRollout / GroupedRollout with record=..., or a
    RolloutStream with trace=...: its cases are the episodes, its per-case results() the statistics) next
    to the input file of its ORIGINAL starts, as save_success_cases writes them for the reference's movies
    (multirobotsim_dcenlocal_onlineExpert.py:732-799): `directory`/input/{mode}Cases_ID{:05d}.yaml and
    `directory`/predict_{mode}/{mode}Cases_ID{:05d}.yaml with mode = success | failure.  ids: the dataset ID of each
    episode (default: its index); results: rollout.results() if already at hand.  Returns the list of (episode index,
    input path, prediction path); read_solution(input path, prediction path) reads a pair back."""
    trace = getattr(rollout, 'trace', None)
    if trace is None:
        raise _native.GnnppError('write_prediction_cases needs a recorded rollout (record=True; RolloutStream: trace=True)')
    res = rollout.results() if results is None else results
    grid, goal = trace.grid.cpu().numpy(), trace.goal.cpu().numpy()
    starts = trace.path[:, 0].cpu().numpy()
    ids = list(range(trace.B)) if ids is None else [int(i) for i in ids]
    if len(ids) != trace.B:
        raise _native.GnnppError('ids: one per episode (%d), got %d' % (trace.B, len(ids)))
    written = []
    for b in range(trace.B):
        mode = 'success' if bool(res['success'][b]) else 'failure'
        name = '{}Cases_ID{:05d}.yaml'.format(mode, ids[b])
        paths = [os.path.join(directory, sub, name) for sub in ('input', 'predict_' + mode)]
        texts = (failure_case_yaml(grid[b] if trace.grid_batched else grid, starts[b], goal[b]),
                 trace.prediction_yaml(b, results=res))
        for path, text in zip(paths, texts):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text)
        written.append((b, paths[0], paths[1]))
    return written


def _yaml_of(src):
    import yaml
    if isinstance(src, (bytes, str)) and not os.path.exists(src):
        return yaml.safe_load(src)
    with open(src, 'r') as f:
        return yaml.safe_load(f)


def read_solution(input_yaml, solution_yaml):
    """(grid [H,W] uint8, goal [N,2] int64, schedule [makespan+1,N,2] int64) of a failure-case file and the solver's
    answer to it (paths or YAML text), following load_ExpertSolution / obtainSchedule: an agent whose plan is shorter
    than the team's makespan waits on its goal."""
    cfg, sol = _yaml_of(input_yaml), _yaml_of(solution_yaml)
    H, W = cfg['map']['dimensions']
    grid = np.zeros((H, W), dtype=np.uint8)
    for x, y in cfg['map']['obstacles'] or []:
        grid[x][y] = 1
    agents = cfg['agents']
    goal = np.array([a['goal'] for a in agents], dtype=np.int64)
    T = int(sol['statistics']['makespan']) + 1
    schedule = np.zeros((T, len(agents), 2), dtype=np.int64)
    for n in range(len(agents)):
        plan = sol['schedule']['agent{}'.format(n)]
        for t in range(T):
            schedule[t, n] = [plan[t]['x'], plan[t]['y']] if t < len(plan) else goal[n]
    return grid, goal, schedule


def save_samples_mat(path, grid, goal, schedule, samples, c=0):
    """Case c of `samples` as the reference's training file (keys map, goal, inputState, inputTensor, target, GSO,
    makespan; the transformer's makespan is the number of steps): formats.load_training_step and the reference's
    dataloader read it.  GSO is the fp64 one when the samples kept it."""
    a, b = samples.bounds[c], samples.bounds[c + 1]
    gso = (samples.GSO64 if samples.GSO64 is not None else samples.GSO)[a:b]
    formats.save_case_mat(path, np.asarray(grid, dtype=np.float64), np.asarray(goal, dtype=np.float64),
                          np.asarray(schedule, dtype=np.float64), samples.target[a:b].cpu().numpy().astype(np.float64),
                          b - a, input_tensor=samples.input[a:b].cpu().numpy(), gso=gso.cpu().numpy())


class SamplePool:
    """Device-resident training samples of ONE team size: append ScheduleSamples, draw batches by index gather."""

    def __init__(self):
        self.input = self.target = self.GSO = None

    def __len__(self):
        return 0 if self.input is None else int(self.input.shape[0])

    def append(self, samples):
        new = (samples.input, samples.target, samples.GSO)
        if self.input is None:
            self.input, self.target, self.GSO = (t.clone() for t in new)
            return
        if new[0].shape[1] != self.input.shape[1] or new[0].device != self.input.device:
            raise _native.GnnppError('a SamplePool holds one team size on one device (%d agents on %s)'
                                     % (self.input.shape[1], self.input.device))
        self.input, self.target, self.GSO = (torch.cat((old, t), 0) for old, t in
                                             zip((self.input, self.target, self.GSO), new))

    def draw(self, batch_size, generator=None):
        """(batch_input [B,N,3,11,11], batch_target [B,N,5], batch_GSO [B,N,N]) of batch_size samples drawn uniformly
        without replacement (with, when the pool is smaller): what train_step / GraphedTrainStep.__call__ take.
        generator: a torch.Generator of the pool's device, or of the CPU."""
        n = len(self)
        if n == 0:
            raise _native.GnnppError('the pool is empty')
        gdev = generator.device if generator is not None else self.input.device
        if batch_size <= n:
            idx = torch.randperm(n, generator=generator, device=gdev)[:batch_size]
        else:
            idx = torch.randint(n, (batch_size,), generator=generator, device=gdev)
        return self.gather(idx)

    def gather(self, idx):
        idx = torch.as_tensor(idx, dtype=torch.long).to(self.input.device)
        return self.input.index_select(0, idx), self.target.index_select(0, idx), self.GSO.index_select(0, idx)


class SampleListPool:
    """SamplePool for samples_from_schedules_team(graph='lists'): device-resident samples of ONE team size whose graphs
    stay a capped lists set (cnt [S,N], idx [S,N,cap], val [S,N,cap]); a draw expands the chosen graphs into the standard
    lists block the team filter takes (gnnpp_team_lists_gather), so no [N,N] matrix exists between the schedule and
    training.train_step_lists.  The pool's cap is the largest appended so far."""

    def __init__(self):
        self.input = self.target = self.cnt = self.idx = self.val = None
        self.cap = 0

    def __len__(self):
        return 0 if self.input is None else int(self.input.shape[0])

    @staticmethod
    def _widen(idx, val, cap):
        """idx / val with `cap` entries per column, zeros behind the old ones (a copy: off the hot path)."""
        if idx.shape[2] == cap:
            return idx, val
        wide = [torch.zeros(t.shape[0], t.shape[1], cap, dtype=t.dtype, device=t.device) for t in (idx, val)]
        for w, t in zip(wide, (idx, val)):
            w[:, :, :t.shape[2]] = t
        return wide

    def append(self, samples):
        if getattr(samples, 'cnt', None) is None:
            raise _native.GnnppError("a SampleListPool takes the samples of samples_from_schedules_team(graph='lists')")
        if int(samples.cnt.max()) > int(samples.cap):   # (a host read: appending is off the hot path)
            raise _native.GnnppError('capped lists with a column of %d entries at cap %d are invalid (include/gnnpp.h): '
                                     'they were filled below their need' % (int(samples.cnt.max()), int(samples.cap)))
        if self.input is None:
            self.input, self.target, self.cnt, self.idx, self.val = (
                t.clone() for t in (samples.input, samples.target, samples.cnt, samples.idx, samples.val))
            self.cap = int(samples.cap)
            return
        if samples.input.shape[1] != self.input.shape[1] or samples.input.device != self.input.device:
            raise _native.GnnppError('a SampleListPool holds one team size on one device (%d agents on %s)'
                                     % (self.input.shape[1], self.input.device))
        cap = max(self.cap, int(samples.cap))
        old, new = self._widen(self.idx, self.val, cap), self._widen(samples.idx, samples.val, cap)
        self.idx, self.val = torch.cat((old[0], new[0]), 0), torch.cat((old[1], new[1]), 0)
        self.input, self.target, self.cnt = (torch.cat((o, t), 0) for o, t in
                                             zip((self.input, self.target, self.cnt),
                                                 (samples.input, samples.target, samples.cnt)))
        self.cap = cap

    def draw(self, batch_size, generator=None):
        """(batch_input [B,N,3,11,11], batch_target [B,N,5], lists) of batch_size samples drawn as SamplePool.draw draws
        them; lists: a lists block of B graphs of N nodes (graphML.team_lists_bytes(B, N) bytes): what
        train_step_lists / DecentralPlannerNet.forward_train_lists(..., symmetric=True) take."""
        n = len(self)
        if n == 0:
            raise _native.GnnppError('the pool is empty')
        gdev = generator.device if generator is not None else self.input.device
        if batch_size <= n:
            idx = torch.randperm(n, generator=generator, device=gdev)[:batch_size]
        else:
            idx = torch.randint(n, (batch_size,), generator=generator, device=gdev)
        return self.gather(idx)

    def gather(self, idx):
        dev = self.input.device
        idx = torch.as_tensor(idx, dtype=torch.long).to(dev)
        B, N = int(idx.numel()), int(self.input.shape[1])
        L = _native.lib()
        lists = torch.empty(L.gnnpp_team_lists_bytes(B, N), dtype=torch.uint8, device=dev)
        index = idx.to(torch.int32)
        with _native.device_guard(dev):
            _native.check(L.gnnpp_team_lists_gather(self.cnt.data_ptr(), self.idx.data_ptr(), self.val.data_ptr(),
                                                    len(self), self.cap, index.data_ptr(), B, lists.data_ptr(),
                                                    lists.numel(), N, _native.stream_ptr(dev)),
                          'gnnpp_team_lists_gather')
        return self.input.index_select(0, idx), self.target.index_select(0, idx), lists


class SchedulePool:
    """The sample pool that stores SCHEDULES: device-resident expert schedules of ONE team size on ONE map size, and every
    batch is built when it is drawn (gnnpp_schedule_draw, include/gnnpp_schedule_draw.h: three launches, only the picked
    steps).  Per step it keeps the positions (8 bytes per agent) and the step's largest degree; per case the first step,
    the goals, the radius its graphs are built with, the plan's status and the map -- once for the whole pool when it is
    constructed with grid= [H,W].  Nothing observation-shaped, [steps,N,N] or lists-shaped exists between the schedule
    and the batch: 10 agents on a 20 x 20 map are 84 bytes per step here against 15 KB in a SamplePool.
    The batches are byte for byte those of SamplePool / SampleListPool fed with samples_from_schedules_team of the same
    cases, and the index rule of draw() is theirs, so the same generator state picks the same steps: a drop-in in front of
    training.train_step, GraphedTrainStep.__call__ and training.train_step_lists(..., symmetric=True).
    Arrays grow by capacity doubling: an append copies the new cases' compact arrays, and the old ones only when a
    capacity is exceeded.  A HIP graph captured over enqueue_draw holds the arrays' addresses and the step count of its
    capture: re-capture after an append (reserve() ahead keeps the addresses)."""

    def __init__(self, device='cuda', grid=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _native.GnnppError('SchedulePool needs a HIP device (no CPU fallback)')
        self.steps = self.cases = 0
        self.N = self.H = self.W = None
        self.max_degree = 0
        self.pos = self.step_deg = self.case_start = self.goal = self.radius = self.status = self.grids = None
        self.grid = None
        if grid is not None:
            g = torch.as_tensor(np.asarray(grid) if not torch.is_tensor(grid) else grid)
            if g.dim() != 2:
                raise _native.GnnppError('SchedulePool(grid=...): one shared map [H,W]')
            self.grid = g.to(torch.uint8).contiguous().to(self.device)
            self.H, self.W = int(g.shape[0]), int(g.shape[1])

    def __len__(self):
        return self.steps

    def _tensors(self):
        return [t for t in (self.pos, self.step_deg, self.case_start, self.goal, self.radius, self.status, self.grids,
                            self.grid) if t is not None]

    @property
    def nbytes(self):
        """Bytes allocated (capacities, not fill levels)."""
        return sum(t.numel() * t.element_size() for t in self._tensors())

    def reserve(self, steps, cases):
        """Capacity for `steps` steps and `cases` cases in all (a pool that knows its team and map size: after the first
        append); never shrinks."""
        if self.N is None:
            raise _native.GnnppError('reserve() after the first append: the pool takes its team size from it')
        self._reserve(int(steps), int(cases))

    def _reserve(self, steps, cases):
        dev, N = self.device, self.N

        def grown(old, used, need, shape, dtype):
            have = 0 if old is None else int(old.shape[0])
            if need <= have:
                return old
            new = torch.empty((max(2 * have, need),) + shape, dtype=dtype, device=dev)
            if used:
                new[:used].copy_(old[:used])
            return new
        self.pos = grown(self.pos, self.steps, steps, (N, 2), torch.int32)
        self.step_deg = grown(self.step_deg, self.steps, steps, (), torch.int32)
        self.goal = grown(self.goal, self.cases, cases, (N, 2), torch.int32)
        self.radius = grown(self.radius, self.cases, cases, (), torch.float64)
        self.status = grown(self.status, self.cases, cases, (), torch.int32)
        if self.grid is None:
            self.grids = grown(self.grids, self.cases, cases, (self.H, self.W), torch.uint8)
        fresh = self.case_start is None
        self.case_start = grown(self.case_start, 0 if fresh else self.cases + 1, cases + 1, (), torch.int32)
        if fresh:
            self.case_start[0] = 0

    def append(self, grids, goals, schedules, commR=5.0, audit=False):
        """The arguments of samples_from_schedules_team (grids may be None in a pool constructed with grid=).  Runs
        gnnpp_schedule_team_plan on the NEW cases only and keeps its radius, status and step_deg; the plan's targets and
        workspace are transient.  A flagged case raises what the sample builders raise, naming the case, and leaves the
        pool as it was.  audit=True: the schedules go through mapf.audit first.  One host read (the plan's flags)."""
        dev = self.device
        L = _native.lib()
        goal = torch.as_tensor(np.asarray(goals) if not torch.is_tensor(goals) else goals).to(torch.int32)
        C = len(schedules)
        if C == 0 or goal.dim() != 3 or goal.shape[0] != C or goal.shape[2] != 2:
            raise _native.GnnppError('goals must be [C,N,2] with one entry per schedule (C = %d)' % C)
        N = int(goal.shape[1])
        if not 2 <= N <= MAX_TEAM:
            raise _native.GnnppError('teams of 2 to %d agents (got %d)' % (MAX_TEAM, N))
        if grids is None:
            if self.grid is None:
                raise _native.GnnppError('grids=None needs a pool constructed with grid=')
            g = self.grid
        else:
            g = torch.as_tensor(np.asarray(grids) if not torch.is_tensor(grids) else grids)
            if g.dim() not in (2, 3) or (g.dim() == 3 and g.shape[0] != C):
                raise _native.GnnppError('grids must be [H,W] or [C,H,W]')
            g = g.to(torch.uint8).contiguous().to(dev)
            if self.grid is not None and (g.dim() != 2 or g.shape != self.grid.shape or not torch.equal(g, self.grid)):
                raise _native.GnnppError('this SchedulePool holds ONE shared map (grid=): append its cases with that map, '
                                         'or with grids=None')
        H, W = int(g.shape[-2]), int(g.shape[-1])
        if self.N is not None and N != self.N or self.H is not None and (H, W) != (self.H, self.W):
            raise _native.GnnppError('a SchedulePool holds one team size and one map size (%s agents on %s x %s)'
                                     % (self.N, self.H, self.W))
        sched = [torch.as_tensor(np.asarray(s) if not torch.is_tensor(s) else s).to(torch.int32) for s in schedules]
        for c, s in enumerate(sched):
            if s.dim() != 3 or s.shape[0] < 1 or tuple(s.shape[1:]) != (N, 2):
                raise _native.GnnppError('schedule %d must be [T,%d,2] with T >= 1 (got %s)' % (c, N, tuple(s.shape)))
        if audit:
            from . import mapf
            _raise_if_audit_flagged(mapf.audit(g, None, goal, sched, dev), C)
        bounds = [0]
        for s in sched:
            bounds.append(bounds[-1] + int(s.shape[0]))
        T = bounds[-1]
        goal = goal.contiguous().to(dev)
        pos = torch.cat(sched, 0).contiguous().to(dev)
        case_start = torch.tensor(bounds, dtype=torch.int32).to(dev)
        flags = torch.empty(C + T, dtype=torch.int32, device=dev)        # status | step_deg: one read for both
        plan = ScheduleSamples(
            input=None, GSO=None, GSO64=None, target=torch.empty(T, N, 5, dtype=torch.float32, device=dev),
            radius=torch.empty(C, dtype=torch.float64, device=dev), growth=torch.empty(C, dtype=torch.int32, device=dev),
            status=flags[:C], step_deg=flags[C:], step_growth=torch.empty(T, dtype=torch.int32, device=dev),
            workspace=torch.empty(L.gnnpp_schedule_team_workspace_bytes(N, T), dtype=torch.uint8, device=dev))
        enqueue_schedule_team_plan(g, goal, pos, case_start, plan, commR)
        host = flags.cpu()
        _raise_if_flagged(host[:C], C)                  # (the pool is untouched up to here)
        if self.N is None:
            self.N, self.H, self.W = N, H, W
        T0, C0 = self.steps, self.cases
        self._reserve(T0 + T, C0 + C)
        self.pos[T0:T0 + T].copy_(pos)
        self.step_deg[T0:T0 + T].copy_(plan.step_deg)
        self.goal[C0:C0 + C].copy_(goal)
        self.radius[C0:C0 + C].copy_(plan.radius)
        self.status[C0:C0 + C].copy_(plan.status)
        self.case_start[C0 + 1:C0 + C + 1].copy_(case_start[1:] + T0)
        if self.grid is None:
            self.grids[C0:C0 + C].copy_(g if g.dim() == 3 else g.unsqueeze(0).expand(C, H, W))
        self.steps, self.cases = T0 + T, C0 + C
        self.max_degree = max(self.max_degree, int(host[C:].max()))

    def append_solutions(self, solutions, grids, goals, commR=5.0, audit=False):
        """The solved cases of a mapf.Solutions, selected as samples_from_solutions selects them (status 0, the schedule up
        to the case's makespan); grids [C,H,W] or [H,W] and goals [C,N,2] as solve() was given them.  Returns their case
        ids (numpy int64 [S]); with none solved the pool is unchanged."""
        status = solutions.status.cpu().numpy()
        ids = np.nonzero(status == 0)[0]
        if len(ids) == 0:
            return ids
        dev = solutions.status.device
        makespan = solutions.makespan.cpu().numpy()
        idx = torch.as_tensor(ids, device=dev)
        g = grids
        if g is not None:
            g = g if torch.is_tensor(g) else torch.as_tensor(np.asarray(g))
            g = g.to(dev).index_select(0, idx) if g.dim() == 3 else g
        gl = (goals if torch.is_tensor(goals) else torch.as_tensor(np.asarray(goals))).to(dev).index_select(0, idx)
        self.append(g, gl, [solutions.schedules[c, :int(makespan[c]) + 1] for c in ids], commR=commR, audit=audit)
        return ids

    def draw_buffers(self, batch_size, graph='dense'):
        """Caller-owned tensors for enqueue_draw: a ScheduleSamples with input [B,N,3,11,11], target [B,N,5], workspace,
        and GSO [B,N,N] (graph='dense') or lists, a standard block of B graphs (graph='lists')."""
        if graph not in ('dense', 'lists'):
            raise _native.GnnppError("unknown graph %r (one of ['dense', 'lists'])" % (graph,))
        if self.N is None:
            raise _native.GnnppError('the pool is empty')
        L, dev, B, N = _native.lib(), self.device, int(batch_size), self.N
        out = ScheduleSamples(input=torch.empty(B, N, 3, 11, 11, dtype=torch.float32, device=dev),
                              target=torch.empty(B, N, 5, dtype=torch.float32, device=dev), GSO=None, lists=None,
                              workspace=torch.empty(L.gnnpp_schedule_draw_workspace_bytes(N, B), dtype=torch.uint8,
                                                    device=dev))
        if graph == 'dense':
            out.GSO = torch.empty(B, N, N, dtype=torch.float32, device=dev)
        else:
            out.lists = torch.empty(L.gnnpp_team_lists_bytes(B, N), dtype=torch.uint8, device=dev)
        return out

    def enqueue_draw(self, index, out, graph='dense'):
        """gnnpp_schedule_draw alone, on torch's current stream: index [B] int32 on the pool's device, out as
        draw_buffers(B, graph) makes it (contiguous; out.GSO for 'dense', out.lists for 'lists').  No allocation, no host
        read, capturable in a HIP graph; the contents of `index` may change between replays."""
        if graph not in ('dense', 'lists'):
            raise _native.GnnppError("unknown graph %r (one of ['dense', 'lists'])" % (graph,))
        if self.steps == 0:
            raise _native.GnnppError('the pool is empty')
        B, N = int(index.numel()), self.N
        graph_out = out.GSO if graph == 'dense' else out.lists
        dev = _native.require_gpu(index, out.input, out.target, graph_out, out.workspace)
        if (index.dtype is not torch.int32 or not index.is_contiguous() or tuple(out.input.shape) != (B, N, 3, 11, 11)
                or tuple(out.target.shape) != (B, N, 5) or out.input.dtype is not torch.float32
                or out.target.dtype is not torch.float32 or not (out.input.is_contiguous() and out.target.is_contiguous())
                or not graph_out.is_contiguous()
                or (graph == 'dense' and (tuple(graph_out.shape) != (B, N, N) or graph_out.dtype is not torch.float32))):
            raise _native.GnnppError('a draw of %d steps of %d agents: index [B] int32, contiguous input [B,N,3,11,11], '
                                     'target [B,N,5] and GSO [B,N,N] float32 (or a lists block)' % (B, N))
        s = _native.ScheduleStruct()
        grid = self.grid if self.grid is not None else self.grids
        s.grid, s.grid_batched, s.goal, s.pos = grid.data_ptr(), int(self.grid is None), self.goal.data_ptr(), self.pos.data_ptr()
        s.case_start, s.C, s.N, s.H, s.W, s.T_total = self.case_start.data_ptr(), self.cases, N, self.H, self.W, self.steps
        s.radius, s.status = self.radius.data_ptr(), self.status.data_ptr()
        ws = out.workspace
        dense = graph == 'dense'
        with _native.device_guard(dev):
            _native.check(_native.lib().gnnpp_schedule_draw(
                ctypes.byref(s), index.data_ptr(), B, out.input.data_ptr(), out.target.data_ptr(),
                graph_out.data_ptr() if dense else None, None if dense else graph_out.data_ptr(),
                0 if dense else graph_out.numel() * graph_out.element_size(), ws.data_ptr(), ws.numel() * ws.element_size(),
                _native.stream_ptr(dev)), 'gnnpp_schedule_draw')

    def draw(self, batch_size, generator=None, graph='dense'):
        """(batch_input [B,N,3,11,11], batch_target [B,N,5], batch_GSO [B,N,N]) -- graph='lists': (batch_input,
        batch_target, lists block of B graphs) -- of batch_size steps drawn as SamplePool.draw draws them: uniformly
        without replacement, with replacement when the pool is smaller.  generator: a torch.Generator of the pool's device,
        or of the CPU."""
        n = len(self)
        if n == 0:
            raise _native.GnnppError('the pool is empty')
        gdev = generator.device if generator is not None else self.device
        if batch_size <= n:
            idx = torch.randperm(n, generator=generator, device=gdev)[:batch_size]
        else:
            idx = torch.randint(n, (batch_size,), generator=generator, device=gdev)
        return self.gather(idx, graph)

    def gather(self, idx, graph='dense'):
        index = torch.as_tensor(idx, dtype=torch.long).to(self.device).to(torch.int32).contiguous()
        out = self.draw_buffers(int(index.numel()), graph)
        self.enqueue_draw(index, out, graph)
        return out.input, out.target, out.GSO if graph == 'dense' else out.lists
