"""Batched on-device rollouts: B independent MAPF episodes stepped together on one MI355X.

Mirrors what the reference does per test case on the host (agents/decentralplannerlocal.py:534-592
driving utils/multirobotsim_dcenlocal.py), with the episode state resident in HBM:

    sim.getCurrentState()  -> BatchedRollout.observe()   AgentState.toInputTensor (statetransformer.py:82-130)
    sim.getGSO(step)       -> BatchedRollout.gso(step)   computeAdjacencyMatrix (multirobotsim_dcenlocal.py:320-394)
    model.addGSO / model() -> DecentralPlannerNet.forward_logits
    sim.move(actionVec, t) -> BatchedRollout.move(...)   move + interRobotCollision (:462-723)

A step is ONE kernel launch for teams of up to 16 agents (policy forward, move, next GSO and
observations in the same workgroup per episode), otherwise encoder, filter + head and the simulator
kernels, and never a host synchronisation; `run()` only reads back a "finished"
flag every few steps.  The reference's random.choice tie-break among colliding agents (:489) is
replaced by a deterministic rule (`tie_mode`): 'lowest' index, 'hashed' counter-based RNG, 'replay' of
recorded choices (parity tests), or 'mt19937' = CPython's random.choice itself on a per-episode
Mersenne-Twister stream (episode b behaves as the reference does after random.seed(seed[b])).
Positions are (row, col) integers.

`record=True` keeps what the reference keeps as path_predict / action_predict: a RolloutTrace on the device, one small
launch behind every move on every route, still without a host synchronisation.
"""
import ctypes

import numpy as np
import torch

from . import _native

_TIE = {'lowest': _native.TIE_LOWEST, 'hashed': _native.TIE_HASHED, 'replay': _native.TIE_REPLAY,
        'mt19937': _native.TIE_MT19937}
MAX_AGENTS = _native.ROLLOUT_MAX_AGENTS             # the one-wave simulator kernels
MAX_TEAM = _native.ROLLOUT_MAX_TEAM
MAX_TEAM_CELLS = _native.ROLLOUT_TEAM_MAX_CELLS     # map limit of the large-team kernels
GRAPHS = ('dense', 'lists')  # how a BatchedRollout hands the communication graph to the policy


def _p(t):
    return t.data_ptr() if t is not None else None


class RolloutTrace:
    """What a recorded rollout did, as device tensors (include/gnnpp_rollout_trace.h):

        path      int32 [B,T_cap+1,N,2]  the positions after every step, row 0 = the starts: the solvers' schedule layout
        action    int8  [B,T_cap,N]      the action each agent asked for at step t + 1 (the argmax of its logits, first
                                         maximum), -1 where nothing was recorded
        moves     int32 [B,N]            steps at which the agent's position changed
        shielded  int32 [B,N]            steps at which the agent asked to move and stood still instead: the map's edge, an
                                         obstacle or the collision shield stopped it
        steps     int32 [B]              the last step at which the episode was not frozen

    An episode whose loop has ended is frozen by the move kernels; its rows after steps[b] repeat row steps[b], as a
    solver's schedule repeats a goal, its `action` stays -1 there and its counters stand still.  `seen_done` [B] is the
    recorder's own word behind that rule.  The tensors are filled by launches on the rollout's stream: synchronise (or call
    rollout.results()) before reading them on the host; schedule() and prediction_yaml() do."""

    def __init__(self, owner, grid, grid_batched, goal, T_cap, tensors=None):
        self._owner = owner                                   # the rollout: results() for the files' statistics
        self.grid, self.grid_batched, self.goal = grid, int(grid_batched), goal
        self.B, self.N = int(goal.shape[0]), int(goal.shape[1])
        self.T_cap, self.device = int(T_cap), goal.device
        if tensors is None:
            B, N, T, dev = self.B, self.N, self.T_cap, self.device
            tensors = (torch.zeros(B, T + 1, N, 2, dtype=torch.int32, device=dev),   # (rows no record reached: 0)
                       torch.empty(B, T, N, dtype=torch.int8, device=dev),
                       torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev),
                       torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        self.path, self.action, self.moves, self.shielded, self.steps, self.seen_done = tensors
        s = _native.RolloutTraceStruct()
        s.path, s.action, s.moves, s.shielded = _p(self.path), _p(self.action), _p(self.moves), _p(self.shielded)
        s.steps, s.seen_done, s.T_cap = _p(self.steps), _p(self.seen_done), self.T_cap
        self._s = s

    def _sync(self):
        if hasattr(self._owner, 'join'):
            self._owner.join()
        torch.cuda.synchronize(self.device)

    def schedule(self, b):
        """[steps[b]+1, N, 2] int64 of episode b: what Solutions.schedule and expert.read_solution return."""
        self._sync()
        return self.path[b, :int(self.steps[b]) + 1].cpu().numpy().astype(np.int64)

    def audit(self):
        """mapf.enqueue_audit on `path` as it lies in memory, rows 0 .. steps[b] of every episode, against the rollout's
        maps and goals and with row 0 as the starts, enqueued on the current stream behind the recorded steps.  Returns
        mapf.Audit.  The move rule forbids a jump, a state off the map or on an obstacle and a false start; vertex and
        swap conflicts are what the collision shield left, as the reference reports them in its own flag."""
        from . import mapf
        H, W = int(self.grid.shape[-2]), int(self.grid.shape[-1])
        if H > mapf.MAX_TEAM_SIDE or W > mapf.MAX_TEAM_SIDE:
            raise _native.GnnppError('maps of at most %d x %d cells (got %d x %d)'
                                     % (mapf.MAX_TEAM_SIDE, mapf.MAX_TEAM_SIDE, H, W))
        if self.T_cap > mapf.MAX_TEAM_STEPS:
            raise _native.GnnppError('schedules of at most %d steps (got %d)' % (mapf.MAX_TEAM_STEPS, self.T_cap))
        if hasattr(self._owner, 'join'):
            self._owner.join()
        out = mapf.empty_audit(self.B, self.N, self.T_cap, self.device)
        start = self.path[:, 0].contiguous()
        out._keep = (self, start)
        mapf.enqueue_audit(self.grid, start, self.goal, self.path, self.steps, out)
        return out

    def prediction_yaml(self, b, results=None):
        """Text of the predicted schedule of episode b as save_success_cases writes it
        (multirobotsim_dcenlocal_onlineExpert.py:777-799): statistics (cost = the rollout's flowtime, its makespan,
        succeed) and, per agent, x / y / t of rows 0 .. steps[b].  results: rollout.results() if already at hand."""
        res = self._owner.results() if results is None else results
        sched = self.schedule(b)
        out = ['statistics:\n', '    cost: {}\n'.format(int(res['flowtime'][b])),
               '    makespan: {}\n'.format(int(res['makespan'][b])),
               '    succeed: {}\n'.format(int(bool(res['success'][b]))), 'schedule:\n']
        for n in range(self.N):
            out.append('    agent{}:\n'.format(n))
            for t in range(sched.shape[0]):
                out.append('       - x: {}\n         y: {}\n         t: {}\n'.format(int(sched[t, n, 0]),
                                                                                  int(sched[t, n, 1]), t))
        return ''.join(out)


class StreamTrace(RolloutTrace):
    """What a traced stream did, per CASE of its queue (include/gnnpp_rollout_stream_trace.h): the RolloutTrace interface
    with B = C, rows RELATIVE to each case's seat.

        path      int32 [C,T_cap+1,N,2]  row 0 = the case's starts, row k = the positions after its step k
        action    int8  [C,T_cap,N]      the action each agent asked for at the case's step k + 1, -1 = nothing recorded
        moves     int32 [C,N]            steps at which the agent's position changed
        shielded  int32 [C,N]            steps at which the agent asked to move and stood still instead
        steps     int32 [C]              the case's last step that was not frozen; -1 = no move of the case recorded yet

    Unlike a RolloutTrace, a frozen case writes nothing: the rows beyond steps[c] stay 0 and `action` stays -1 there.
    `seen_done` [slots] is the recorder's own word per SLOT.  `grid`, `grid_batched` and `goal` are the case queue's.
    schedule(c), prediction_yaml(c, results=None) and audit() are keyed by case."""

    def __init__(self, owner, T_cap):
        self._owner = owner                                   # the stream: results() per case for the files' statistics
        self.grid, self.grid_batched, self.goal = owner.grid, owner.grid_batched, owner.goal
        self.B, self.N = owner.C, owner.N
        self.T_cap, self.device = int(T_cap), owner.device
        C, N, T, dev = self.B, self.N, self.T_cap, self.device
        self.path = torch.empty(C, T + 1, N, 2, dtype=torch.int32, device=dev)   # (all of it is set by begin)
        self.action = torch.empty(C, T, N, dtype=torch.int8, device=dev)
        self.moves = torch.empty(C, N, dtype=torch.int32, device=dev)
        self.shielded = torch.empty(C, N, dtype=torch.int32, device=dev)
        self.steps = torch.empty(C, dtype=torch.int32, device=dev)
        self.seen_done = torch.empty(owner.slots, dtype=torch.int32, device=dev)
        s = _native.RolloutStreamTraceStruct()
        s.path, s.action, s.moves, s.shielded = _p(self.path), _p(self.action), _p(self.moves), _p(self.shielded)
        s.steps, s.seen_done, s.T_cap = _p(self.steps), _p(self.seen_done), self.T_cap
        self._s = s

    def audit(self):
        """RolloutTrace.audit per case: rows 0 .. steps[c] of `path` against the case queue's maps and goals, row 0 as the
        starts, with the same map and step limits.  Refused while a case has no recorded move yet (steps[c] < 0: the audit
        would skip it silently) -- run the stream to its end first."""
        self._sync()
        missing = (self.steps < 0).nonzero().flatten()
        if missing.numel():
            raise _native.GnnppError('StreamTrace.audit: %d case(s) have no recorded move yet (steps[c] < 0; first: case %d): '
                                     'run the stream until its queue has drained' % (missing.numel(), int(missing[0])))
        return RolloutTrace.audit(self)


class BatchedRollout:
    def __init__(self, grid, starts, goals, maxstep, device, commR=6.0, tie_mode='lowest', seed=0,
                 rng_words=None, graph='dense', record=False):
        """grid [B,H,W] or [H,W] (1 = obstacle); starts, goals [B,N,2]; maxstep int or [B].  Teams of up to
        MAX_TEAM agents; beyond MAX_AGENTS the simulator runs the large-team kernels, which need H * W <=
        MAX_TEAM_CELLS.  rng_words (tie_mode 'mt19937'): words of each episode's random stream, by default 2048,
        and 64 per agent for teams of more than MAX_AGENTS agents.
        graph: 'dense' (default) -- the communication graph is the GSO S [B,N,N] -- or 'lists': it is the team filter's
        neighbour lists (gnnpp_rollout_lists; `self.lists`, a uint8 block of B graphs, see graphML.team_lists_views), no
        S is ever allocated, and step(model) needs a planner that takes lists (DecentralPlannerNet with
        largeGraphFilter='lists', its forward_logits_lists).  Same episodes, step for step.
        record: True keeps a RolloutTrace (`self.trace`) of max(maxstep) steps, an integer one of that many steps; every
        move of every route is recorded by a launch behind it, a step beyond the trace's last row raises before anything
        is enqueued, and nothing else about the rollout changes."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _native.GnnppError('BatchedRollout needs a HIP device (no CPU fallback)')
        if graph not in GRAPHS:
            raise _native.GnnppError('unknown graph %r (one of %s)' % (graph, list(GRAPHS)))
        self.graph = graph
        _native.lib()
        self.device = dev
        g = torch.as_tensor(grid)
        self.grid_batched = int(g.dim() == 3)
        self.grid = g.to(torch.uint8).contiguous().to(dev)
        self.H, self.W = int(g.shape[-2]), int(g.shape[-1])
        self.pos = torch.as_tensor(starts).to(torch.int32).contiguous().to(dev)
        self.goal = torch.as_tensor(goals).to(torch.int32).contiguous().to(dev)
        self.B, self.N = int(self.pos.shape[0]), int(self.pos.shape[1])
        assert self.goal.shape == self.pos.shape and self.pos.shape[2] == 2
        assert not self.grid_batched or self.grid.shape[0] == self.B
        if self.N > MAX_TEAM:
            raise _native.GnnppError('at most %d agents per episode' % MAX_TEAM)
        if self.N > MAX_AGENTS and self.H * self.W > MAX_TEAM_CELLS:
            raise _native.GnnppError('teams of more than %d agents need a map of at most %d cells (got %d x %d)'
                                     % (MAX_AGENTS, MAX_TEAM_CELLS, self.H, self.W))
        if rng_words is None:
            rng_words = 2048 if self.N <= MAX_AGENTS else 64 * self.N
        ms = torch.as_tensor(maxstep, dtype=torch.int32)
        self.maxstep = (ms if ms.dim() else ms.repeat(self.B)).contiguous().to(dev)
        B, N = self.B, self.N
        self.obs = torch.empty(B, N, 3, 11, 11, dtype=torch.float32, device=dev)
        self.radius = torch.full((B,), float(commR), dtype=torch.float64, device=dev)
        # 'lists': no dense GSO, the lists block instead (sized for the dense worst case, touched only where the
        # graph has neighbours)
        self.S = torch.empty(B, N, N, dtype=torch.float32, device=dev) if graph == 'dense' else None
        self.lists = None
        if graph == 'lists':
            self.lists = torch.empty(_native.lib().gnnpp_team_lists_bytes(B, N), dtype=torch.uint8, device=dev)
        self.connected = torch.zeros(B, dtype=torch.int32, device=dev)
        self.reached = torch.zeros(B, N, dtype=torch.int32, device=dev)
        self.start_step = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        self.end_step = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(B, 3, dtype=torch.int32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)   # the case's loop has ended: frozen
        self.stats = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self.choice_count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.tie_mode = _TIE[tie_mode]
        self.rng_words = self.rng_cursor = None
        if self.tie_mode == 3:
            # raw genrand_uint32() outputs of random.Random(seed_b): the kernel applies random.choice's
            # own rejection sampling to them (csrc/rollout_kernels.hip::choose_mover)
            import random
            seeds = list(seed) if hasattr(seed, '__len__') else [int(seed) + b for b in range(self.B)]
            assert len(seeds) == self.B
            import numpy as np
            rows = np.array([[g.getrandbits(32) for _ in range(int(rng_words))]
                             for g in (random.Random(int(sd)) for sd in seeds)], dtype=np.uint32)
            self.rng_words = torch.from_numpy(rows.view(np.int32)).to(dev)
            self.rng_cursor = torch.zeros(self.B, dtype=torch.int32, device=dev)
            seed = 0
        self.seed = int(seed) & 0xffffffff
        self.t = 0                                            # steps taken so far
        self._state_step = -1                                 # step whose positions obs / S describe
        self._seated = False                                  # RolloutStream: every slot's step-0 state comes from its seat
        self._stream_trace = None                             # RolloutStream(trace=...): the stream whose recorder follows a move
        # teams up to this size run move -> graph -> observations as ONE launch (gnnpp_rollout_step, one workgroup
        # per episode); larger ones as move, then graph || observations in a second launch (gnnpp_rollout_gso_observe:
        # more workgroups than episodes).  Measured per simulator step: N = 10 16.1 (one launch) vs 17.3 us,
        # N = 50 33.2 vs 28.5, N = 100 52.4 vs 42.4
        self.fused_sim_max_agents = 32
        self._logits = None                                   # [N,B,5] of the one-launch step
        r = _native.RolloutStruct()
        r.grid, r.grid_batched, r.goal, r.pos = _p(self.grid), self.grid_batched, _p(self.goal), _p(self.pos)
        r.B, r.N, r.H, r.W = B, N, self.H, self.W
        r.obs, r.radius, r.S, r.connected = _p(self.obs), _p(self.radius), _p(self.S), _p(self.connected)
        r.reached, r.start_step, r.end_step = _p(self.reached), _p(self.start_step), _p(self.end_step)
        r.maxstep, r.flags, r.stats = _p(self.maxstep), _p(self.flags), _p(self.stats)
        r.done = _p(self.done)
        r.tie_mode, r.seed, r.choice_count = self.tie_mode, self.seed, _p(self.choice_count)
        if self.tie_mode == 3:
            r.rng_words, r.rng_cursor, r.rng_max = _p(self.rng_words), _p(self.rng_cursor), int(rng_words)
        self._r = r
        self.trace = None
        if record is not False and record is not None:
            T_cap = int(self.maxstep.max().item()) if record is True else int(record)
            if T_cap < 1:
                raise _native.GnnppError('record: a trace of at least one step (got %d)' % T_cap)
            self.trace = RolloutTrace(self, self.grid, self.grid_batched, self.goal, T_cap)
            self._trace_call(_native.lib().gnnpp_rollout_trace_begin, 'gnnpp_rollout_trace_begin')

    # -- the three simulator calls -------------------------------------------------------------
    def _call(self, fn, what):
        with _native.device_guard(self.device):
            _native.check(fn(ctypes.byref(self._r), _native.stream_ptr(self.device)), what)

    def _trace_call(self, fn, what):
        with _native.device_guard(self.device):
            _native.check(fn(ctypes.byref(self._r), ctypes.byref(self.trace._s), _native.stream_ptr(self.device)), what)

    def _record(self):
        """The trace's row of the move just enqueued (its logits / actions are still in the struct)."""
        if self.trace is not None:
            self._trace_call(_native.lib().gnnpp_rollout_trace_record, 'gnnpp_rollout_trace_record')
        elif self._stream_trace is not None:                 # the slots of a traced stream: its per-case recorder
            self._stream_trace._record()

    def _check_room(self, n=1, currentstep=None):
        """record: the next n steps must fit the trace, and be the rollout's own next steps -- before anything is enqueued."""
        if self.trace is None:
            return
        if currentstep is not None and int(currentstep) != self.t + 1:
            raise _native.GnnppError('a recorded rollout takes its steps in order: the next one is %d (got currentstep=%d)'
                                     % (self.t + 1, int(currentstep)))
        if self.t + n > self.trace.T_cap:
            raise _native.GnnppError('step %d is beyond the trace (record: T_cap = %d steps)'
                                     % (self.t + n, self.trace.T_cap))

    def observe(self):
        """[B,N,3,11,11] float32 observations of the current positions (buffer reused each step)."""
        self._call(_native.lib().gnnpp_rollout_observe, 'gnnpp_rollout_observe')
        return self.obs

    def _lists_call(self):
        with _native.device_guard(self.device):
            _native.check(_native.lib().gnnpp_rollout_lists(ctypes.byref(self._r), _p(self.lists), self.lists.numel(),
                                                            _native.stream_ptr(self.device)), 'gnnpp_rollout_lists')

    def gso(self, step=None):
        """[B,N,N] float32 GSO of the current positions (graph='lists': the lists block of the same graph).  step 0
        grows the radius until connected."""
        step = self.t if step is None else step
        self._r.grow = int(step == 0)
        if self.graph == 'lists':
            self._lists_call()
            return self.lists
        self._call(_native.lib().gnnpp_rollout_gso, 'gnnpp_rollout_gso')
        return self.S

    def gso_observe(self):
        """gso() (no radius growth: not for step 0) and observe() of the current positions as ONE launch
        (gnnpp_rollout_gso_observe): the two are independent given the positions.  graph='lists': the lists launch,
        then the observations (separate launches, as large teams already use); returns (obs, lists)."""
        self._r.grow = 0
        if self.graph == 'lists':
            self._lists_call()
            self._call(_native.lib().gnnpp_rollout_observe, 'gnnpp_rollout_observe')
            self._state_step = self.t
            return self.obs, self.lists
        self._call(_native.lib().gnnpp_rollout_gso_observe, 'gnnpp_rollout_gso_observe')
        self._state_step = self.t
        return self.obs, self.S

    def move(self, logits=None, actions=None, choices=None, currentstep=None):
        """Apply one joint action.  logits [N,B,5] (DecentralPlannerNet.forward_logits) or action
        ids [B,N] int32; `choices` [B,C] int16 only for tie_mode='replay'.  Returns flags [B,3]
        (allReachGoal at entry, moveCollision, predictCollision) -- a device tensor."""
        self._prepare_move(logits, actions, choices, currentstep)
        self._call(_native.lib().gnnpp_rollout_move, 'gnnpp_rollout_move')
        self._record()
        return self.flags

    def _prepare_move(self, logits, actions, choices, currentstep):
        self._check_room(1, currentstep)
        r = self._r
        keep = []
        if logits is not None:
            lg = logits.detach().contiguous().float()
            assert lg.shape == (self.N, self.B, 5)
            keep.append(lg)
            r.logits, r.actions = _p(lg), None
        else:
            ac = actions.to(torch.int32).contiguous()
            assert ac.shape == (self.B, self.N)
            keep.append(ac)
            r.logits, r.actions = None, _p(ac)
        if self.tie_mode == 2:
            ch = choices.to(torch.int16).contiguous().to(self.device)
            keep.append(ch)
            r.choices, r.max_choices = _p(ch), int(ch.shape[1])
        self.t += 1
        r.currentstep = self.t if currentstep is None else int(currentstep)
        self._keep = keep                                   # alive until the launch has been enqueued

    # -- whole episodes ------------------------------------------------------------------------------
    def move_and_observe(self, logits=None, actions=None, choices=None, currentstep=None):
        """move(), then the next step's gso() and observe(), as ONE kernel launch
        (gnnpp_rollout_step).  Same results as the three calls in sequence."""
        self._prepare_move(logits, actions, choices, currentstep)
        self._r.grow = 0
        if self.graph == 'lists':                          # move -> lists -> observations: three launches
            self._call(_native.lib().gnnpp_rollout_move, 'gnnpp_rollout_move')
            self._lists_call()
            self._call(_native.lib().gnnpp_rollout_observe, 'gnnpp_rollout_observe')
        else:
            self._call(_native.lib().gnnpp_rollout_step, 'gnnpp_rollout_step')
        self._record()                                     # (pos, and the logits / actions of this move, are in memory)
        self._state_step = self.t                          # obs / S describe the positions after step t
        return self.flags

    def _policy_step(self, model, nsteps=1):
        """gnnpp_rollout_policy_step(s): policy forward + move + next gso/observe in ONE kernel per step, when
        the model and the team qualify (eval mode, N = model.numAgents <= 16, K = 2..4, not 'replay'); nsteps
        launches are enqueued by one C call."""
        if (self.graph != 'dense' or self.N > 16 or self.tie_mode == 2 or getattr(model, 'training', True)
                or getattr(model, 'numAgents', -1) != self.N or not hasattr(model, 'policy_pointers')):
            return False
        ptrs = model.policy_pointers()
        if ptrs is None or not 2 <= ptrs[5] <= 4:            # (the fused kernel exists for K = 2, 3, 4 taps)
            return False
        enc, taps, gb, aw, ab, K = ptrs
        if self._logits is None:
            self._logits = torch.empty(self.N, self.B, 5, dtype=torch.float32, device=self.device)
        r = self._r
        r.logits, r.actions, r.grow = _p(self._logits), None, 0
        prec = model._prec() if hasattr(model, '_prec') else _native.PREC_FP32
        # range guard: only the opt-in split-f16 arithmetic has an input domain
        r.range_flag = _p(model._flag(self.device)) if prec == _native.PREC_SPLIT_F16 else None
        r.currentstep = self.t + 1
        self._check_room(nsteps)
        with _native.device_guard(self.device):
            if self.trace is not None:              # the same launches, a record launch behind each
                what = 'gnnpp_rollout_policy_steps_traced'
                rc = _native.lib().gnnpp_rollout_policy_steps_traced(ctypes.byref(r), enc, taps, gb, aw, ab, K, nsteps, prec,
                                                                     ctypes.byref(self.trace._s),
                                                                     _native.stream_ptr(self.device))
            elif self._stream_trace is not None:    # the slots of a traced stream: a per-case record behind each launch
                what = 'gnnpp_rollout_stream_policy_steps_traced'
                st = self._stream_trace
                rc = _native.lib().gnnpp_rollout_stream_policy_steps_traced(ctypes.byref(r), enc, taps, gb, aw, ab, K, nsteps,
                                                                            prec, ctypes.byref(st._s), ctypes.byref(st.trace._s),
                                                                            _native.stream_ptr(self.device))
            else:
                what = 'gnnpp_rollout_policy_steps'
                rc = _native.lib().gnnpp_rollout_policy_steps(ctypes.byref(r), enc, taps, gb, aw, ab, K, nsteps, prec,
                                                              _native.stream_ptr(self.device))
        if rc == _native.ERR_UNSUPPORTED:           # shape not supported by the fused kernel
            return False
        _native.check(rc, what)
        self.t += nsteps
        self._state_step = self.t
        return True

    def step(self, model):
        """One rollout step of all episodes: observe -> gso -> policy forward -> move.  From the
        second step on the observation and the GSO were already produced by the previous step's
        fused move kernel."""
        if self.graph == 'lists':
            self._check_lists_model(model)
        self._check_room()
        if self.t == 0 and not self._seated:                 # step 0 may grow the radius
            self.observe()
            self.gso()
        elif self._state_step != self.t:                     # stale state: graph and observations side by side
            self.gso_observe()
        if self.graph == 'lists':
            logits = model.forward_logits_lists(self.obs, self.lists)
            return self.move_and_observe(logits=logits) if self.N <= self.fused_sim_max_agents else self.move(logits=logits)
        if self._policy_step(model):                         # small teams: the whole step is one launch
            return self.flags
        model.addGSO(self.S)
        logits = model.forward_logits(self.obs)
        # one launch for move -> graph -> observations (see fused_sim_max_agents); beyond it: move now, the
        # graph and the observations side by side at the start of the next step
        return self.move_and_observe(logits=logits) if self.N <= self.fused_sim_max_agents else self.move(logits=logits)

    def _check_lists_model(self, model):
        """graph='lists': the planner must take lists, for this team -- refused with the reason, before anything runs."""
        if not hasattr(model, 'forward_logits_lists'):
            raise _native.GnnppError("BatchedRollout(graph='lists') needs a planner with forward_logits_lists "
                                     "(DecentralPlannerNet with largeGraphFilter='lists'); %s has none"
                                     % type(model).__name__)
        why = model.lists_refusal(self.N)
        if why is None and self.N <= 16 and model.policy_pointers() is not None and 2 <= model.policy_pointers()[5] <= 4:
            why = ('this planner and team run the one-launch step (N <= 16, K = 2..4), which reads the dense GSO: use '
                   "graph='dense'")
        if why:
            raise _native.GnnppError("BatchedRollout(graph='lists'): " + why)

    def steps(self, model, n):
        """n rollout steps.  Small teams (the one-launch step): the launches of all n steps are enqueued by ONE
        C call (gnnpp_rollout_policy_steps) -- no interpreter between two steps."""
        self._check_room(n)
        done = 0
        if n > 1 and (self._state_step != self.t or self.t == 0):
            self.step(model)                                 # (the first step may grow the radius)
            done = 1
        if n - done > 1 and self._policy_step(model, n - done):
            return self.flags
        for _ in range(n - done):
            self.step(model)
        return self.flags

    def run(self, model, max_steps=None, check_every=8):
        """Step until every episode's loop has ended: the call after its last agent arrived (that call
        writes its statistics, like the reference loop agents/decentralplannerlocal.py:560-605), or
        the call at its OWN maxstep.  An ended episode is frozen by the move kernel (`done`), so mixed
        per-episode limits (maxstep = rate * makespan[b]) report exactly what the reference reports
        case by case."""
        limit = int(self.maxstep.max().item()) if max_steps is None else int(max_steps)
        steps = 0
        while steps < limit:
            burst = min(check_every - steps % check_every, limit - steps)
            self.steps(model, burst)
            steps += burst
            if steps % check_every == 0:
                if hasattr(model, 'check_range'):
                    model.check_range()                      # an activation left the f16 range: error
                if bool((self.done != 0).all().item()):
                    break
        if hasattr(model, 'check_range'):
            model.check_range()
        return self.results()

    def check_rng(self):
        """tie_mode 'mt19937': every episode gets `rng_words` words of its Mersenne-Twister stream; the kernel
        substitutes 0 for words past the end (and keeps counting them in rng_cursor).  An episode that consumed
        more than it was given no longer follows the reference's random.choice stream: that is an error, not a
        silent deviation."""
        if self.rng_cursor is not None:
            over = (self.rng_cursor > int(self.rng_words.shape[1])).nonzero().flatten()
            if over.numel():
                raise _native.GnnppError(
                    'tie_mode mt19937: episode(s) %s consumed more than the %d random words they were given; '
                    'construct the rollout with a larger rng_words' % (over[:8].tolist(), int(self.rng_words.shape[1])))

    def results(self):
        torch.cuda.synchronize(self.device)
        self.check_rng()
        reached = self.reached.bool()
        return {'steps': self.t, 'reached': reached.cpu(), 'success': reached.all(dim=1).cpu(),
                'makespan': self.stats[:, 0].cpu(), 'flowtime': self.stats[:, 1].cpu(),
                'end_step': self.end_step.cpu(), 'start_step': self.start_step.cpu(),
                'positions': self.pos.cpu(), 'radius': self.radius.cpu(), 'done': self.done.bool().cpu()}


class RolloutStream:
    """C cases through `slots` resident episode slots: when a slot's episode ends, its result goes to a per-CASE table and
    the next case of the queue is seated in that slot -- on the device, between two steps, with no host synchronisation
    (include/gnnpp_rollout_stream.h).  BatchedRollout.run() steps a fixed batch until its slowest episode
    ends and every frozen episode still costs its share of each launch; here a finished slot goes back to work.

    grids [C,H,W] or [H,W]; starts, goals [C,N,2]; maxstep int or [C]: each case's own limit.  The stream owns a
    BatchedRollout of min(slots, C) slots (`env`) and drives it on the rollout's own routes: the one-launch step for
    N <= 16, move_and_observe up to 32 agents, move + gso_observe beyond.  The slots share one global step count; a case
    seated at step count t0 runs its step k as global step t0 + k, and its records are stored relative to t0, so every
    per-case value is what a plain rollout of that case alone reports.  reseat_every: steps between two reseats (1: a slot
    is refilled at the first step after its episode ended).

    Scope: teams of 1 .. MAX_AGENTS agents, the dense graph, tie_mode 'lowest' or 'hashed'.  'hashed' hashes (seed, slot,
    global step), so a case draws a different -- equally arbitrary -- stream than in a plain rollout.  'replay', 'mt19937',
    record=..., graph='lists' and N > MAX_AGENTS are refused by name before anything is enqueued (larger teams, on the dense
    graph or on lists: TeamRolloutStream).

    trace: True keeps a StreamTrace (`self.trace`) of max(maxstep) steps per case, an integer one of that many steps (refused
    when below max(maxstep): rows would be lost silently).  It is what BatchedRollout(record=...) keeps, per CASE and with
    rows relative to the case's seat: one small launch behind every move on every route (the one-launch burst included,
    still enqueued by one C call), nothing else about the stream changes and results() is the same.  record= stays refused:
    its trace is laid out per slot of a fixed batch and repeats a frozen episode's last row, this one writes nothing for a
    frozen slot.

    For expert.solve_failures / write_failure_cases the stream looks like a finished rollout of B = C episodes: `.grid`,
    `.grid_batched`, `.pos` (final positions [C,N,2]), `.goal`, `.B`, `.N`, `.device`, results()."""

    def __init__(self, grids, starts, goals, maxstep, device, slots=512, commR=6.0, tie_mode='lowest', seed=0,
                 reseat_every=1, record=False, graph='dense', trace=False):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _native.GnnppError('RolloutStream needs a HIP device (no CPU fallback)')
        if tie_mode not in _TIE:
            raise _native.GnnppError('unknown tie_mode %r (one of %s)' % (tie_mode, sorted(_TIE)))
        if tie_mode in ('replay', 'mt19937'):
            raise _native.GnnppError("RolloutStream: tie_mode %r keeps per-episode state that a seat would have to rewind; "
                                     "use 'lowest' or 'hashed'" % tie_mode)
        if record is not False and record is not None:
            raise _native.GnnppError('RolloutStream: record=... is not supported (a trace is laid out per episode of a '
                                     'fixed batch); use trace=... for the per-case trace of a stream, or '
                                     'BatchedRollout(record=...)')
        if graph != 'dense':
            raise _native.GnnppError("RolloutStream: graph=%r is not supported (a seat builds the dense GSO); use "
                                     "graph='dense', or TeamRolloutStream for teams of more than %d agents"
                                     % (graph, MAX_AGENTS))
        starts_t, goals_t = torch.as_tensor(starts), torch.as_tensor(goals)
        C, N = int(starts_t.shape[0]), int(starts_t.shape[1])
        if N > MAX_AGENTS:
            raise _native.GnnppError('RolloutStream: N > %d (got N = %d) is not supported: the seat runs the one-wave '
                                     'graph build; use TeamRolloutStream' % (MAX_AGENTS, N))
        if C < 1 or int(slots) < 1 or int(reseat_every) < 1:
            raise _native.GnnppError('RolloutStream: at least one case, one slot and reseat_every >= 1')
        self._open_queue(grids, starts_t, goals_t, maxstep, dev, slots, commR, reseat_every)
        T_cap = None
        if trace is not False and trace is not None:
            longest = int(self.case_maxstep.max().item())
            T_cap = longest if trace is True else int(trace)
            if T_cap < max(longest, 1):
                raise _native.GnnppError('RolloutStream: trace=%d is below the longest case limit, max(maxstep) = %d: a '
                                         'shorter trace would silently lose rows' % (T_cap, longest))
        self._open_slots(tie_mode, seed, 'dense', _native.lib().gnnpp_rollout_stream_begin, 'gnnpp_rollout_stream_begin')
        self.trace = None
        if T_cap is not None:
            self.trace = StreamTrace(self, T_cap)
            self._trace_call(_native.lib().gnnpp_rollout_stream_trace_begin, 'gnnpp_rollout_stream_trace_begin')
            self.env._stream_trace = self                     # every move of the slots is followed by _record()

    def _open_queue(self, grids, starts_t, goals_t, maxstep, dev, slots, commR, reseat_every):
        """The case queue on the device (nothing is enqueued but its copies)."""
        C, N = int(starts_t.shape[0]), int(starts_t.shape[1])
        assert goals_t.shape == starts_t.shape and starts_t.shape[2] == 2
        _native.lib()
        self.device, self.C, self.N = dev, C, N
        self.B = C                                            # a finished rollout of C episodes, to its readers
        self.slots = min(int(slots), C)
        self.reseat_every = int(reseat_every)
        self.commR = float(commR)
        g = torch.as_tensor(grids)
        self.grid_batched = int(g.dim() == 3)
        assert not self.grid_batched or g.shape[0] == C
        self.grid = g.to(torch.uint8).contiguous().to(dev)
        self.start = starts_t.to(torch.int32).contiguous().to(dev)
        self.goal = goals_t.to(torch.int32).contiguous().to(dev)
        ms = torch.as_tensor(maxstep, dtype=torch.int32)
        self.case_maxstep = (ms if ms.dim() else ms.repeat(C)).contiguous().to(dev)
        assert self.case_maxstep.shape == (C,)
        self._limit = int(self.case_maxstep.sum().item())     # (host bound of run(): no stream is longer than that)

    def _open_slots(self, tie_mode, seed, graph, begin, what):
        """The slots' BatchedRollout, the per-case tables, the struct, and `begin` (gnnpp_rollout_[team_]stream_begin)."""
        dev, C, N, B = self.device, self.C, self.N, self.slots
        # the slots start as copies of the first cases (valid cells everywhere), all marked empty by begin()
        self.env = BatchedRollout(self.grid[:B].clone() if self.grid_batched else self.grid, self.start[:B].clone(),
                                  self.goal[:B].clone(), self.case_maxstep[:B].clone(), dev, commR=self.commR,
                                  tie_mode=tie_mode, seed=seed, graph=graph)
        self.env._seated = True
        i32 = dict(dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, **i32)
        self.case = torch.empty(B, **i32)                     # the case each slot holds (-1: empty) ...
        self.t0 = torch.empty(B, **i32)                       # ... and the step count at which it was seated
        self.assign = torch.empty(B, **i32)
        self.reached = torch.empty(C, N, **i32)
        self.start_step = torch.empty(C, N, **i32)
        self.end_step = torch.empty(C, N, **i32)
        self.pos = torch.empty(C, N, 2, **i32)
        self.radius = torch.empty(C, dtype=torch.float64, device=dev)
        self.stats = torch.empty(C, 2, **i32)
        self.lived = torch.empty(C, **i32)
        self.case_slot = torch.empty(C, **i32)
        self.case_t0 = torch.empty(C, **i32)
        e = self.env
        s = _native.RolloutStreamStruct()
        s.case_grid, s.case_grid_batched = _p(self.grid), self.grid_batched
        s.case_start, s.case_goal, s.case_maxstep, s.C, s.commR = _p(self.start), _p(self.goal), _p(self.case_maxstep), C, \
            self.commR
        s.cursor, s.slot_case, s.slot_t0, s.assign = _p(self.cursor), _p(self.case), _p(self.t0), _p(self.assign)
        s.slot_grid = _p(e.grid) if self.grid_batched else None
        s.goal, s.maxstep = _p(e.goal), _p(e.maxstep)
        s.reached, s.start_step, s.end_step, s.pos = _p(self.reached), _p(self.start_step), _p(self.end_step), _p(self.pos)
        s.radius, s.stats, s.lived, s.slot, s.t0 = _p(self.radius), _p(self.stats), _p(self.lived), _p(self.case_slot), \
            _p(self.case_t0)
        self._s = s
        with _native.device_guard(dev):
            _native.check(begin(ctypes.byref(e._r), ctypes.byref(s), _native.stream_ptr(dev)), what)
        self._reseated_at = -1                                # step count of the last reseat

    def _trace_call(self, fn, what):
        with _native.device_guard(self.device):
            _native.check(fn(ctypes.byref(self.env._r), ctypes.byref(self._s), ctypes.byref(self.trace._s),
                             _native.stream_ptr(self.device)), what)

    def _record(self):
        """trace=...: the per-case rows of the move just enqueued (its logits / actions are still in the slots' struct)."""
        self._trace_call(_native.lib().gnnpp_rollout_stream_trace_record, 'gnnpp_rollout_stream_trace_record')

    @property
    def t(self):
        return self.env.t                                     # the global step count

    def reseat(self):
        """Harvest every finished slot into the per-case tables and seat the next cases of the queue, at the current step
        count: two launches on the current stream, nothing read on the host.  Seated slots get their step-0 state
        (radius growth, S, observations) from the seat itself."""
        e = self.env
        with _native.device_guard(self.device):
            _native.check(_native.lib().gnnpp_rollout_stream_reseat(ctypes.byref(e._r), ctypes.byref(self._s), e.t,
                                                                    _native.stream_ptr(self.device)),
                          'gnnpp_rollout_stream_reseat')
        self._reseated_at = e.t
        if e.t == 0:
            e._state_step = 0         # every slot was just seated: S and the observations describe step 0

    def _due(self):
        return self._reseated_at != self.env.t and self.env.t % self.reseat_every == 0

    def move(self, actions=None, logits=None):
        """One scripted step of every slot: a reseat when one is due, then the rollout's move.  actions [slots,N] / logits
        [N,slots,5] are per SLOT: gather them from `case` and `t0` (device tensors) after reseat()."""
        if self._due():
            self.reseat()
        return self.env.move(logits=logits, actions=actions)

    def steps(self, model, n):
        """n policy steps of every slot, a reseat every `reseat_every` of them."""
        left = int(n)
        while left > 0:
            if self._due():
                self.reseat()
            burst = min(left, self.reseat_every - self.env.t % self.reseat_every)
            self.env.steps(model, burst)
            left -= burst
        return self.env.flags

    def finished(self):
        """Every case has been seated and every slot's episode has ended (ONE host read of the cursor and the done count)."""
        state = torch.stack([self.cursor[0], (self.env.done != 0).sum().to(torch.int32)]).tolist()
        return state[0] >= self.C and state[1] == self.slots

    def run(self, model, check_every=8):
        """Step until every case is harvested; the host reads the cursor and the done count once per check_every steps."""
        bound = self._limit + (self.C + 1) * self.reseat_every + check_every
        while True:
            self.steps(model, check_every - self.env.t % check_every)
            if hasattr(model, 'check_range'):
                model.check_range()
            if self.finished():
                break
            if self.env.t > bound:
                raise _native.GnnppError('%s.run: %d steps and the queue has not drained'
                                         % (type(self).__name__, self.env.t))
        return self.results()

    def results(self):
        """Per CASE, the keys BatchedRollout.results() gives per episode (step records relative to the case's seat), plus
        `slot`, `t0`, `lived` and `occupancy` = live slot-steps / all slot-steps so far.  Finished slots that were not
        harvested yet are harvested first; a case that has not ended reads -1 (done: False)."""
        self.reseat()
        torch.cuda.synchronize(self.device)
        lived = self.lived.cpu()
        done = lived >= 0
        reached = self.reached.cpu() > 0
        total = self.slots * self.env.t
        return {'steps': self.env.t, 'reached': reached, 'success': reached.all(dim=1) & done,
                'makespan': self.stats[:, 0].cpu(), 'flowtime': self.stats[:, 1].cpu(), 'end_step': self.end_step.cpu(),
                'start_step': self.start_step.cpu(), 'positions': self.pos.cpu(), 'radius': self.radius.cpu(), 'done': done,
                'slot': self.case_slot.cpu(), 't0': self.case_t0.cpu(), 'lived': lived,
                'occupancy': float(lived[done].sum()) / total if total else 0.0}


class TeamRolloutStream(RolloutStream):
    """RolloutStream for teams of MAX_AGENTS + 1 .. MAX_TEAM agents (include/gnnpp_rollout_team_stream.h):
    the same queue, slots, prefix rule of seating, per-case tables and results(), with the seat built by the large-team
    kernels.  The stream owns a BatchedRollout(..., graph=graph) of min(slots, C) slots (`env`) and drives it on the
    rollout's own large-team route:

        graph='dense'   gso_observe, the planner's forward on S, move
        graph='lists'   the lists launch and the observations, forward_logits_lists on the lists block, move: no dense S is
                        ever allocated, and the planner is checked (BatchedRollout._check_lists_model) before anything is
                        enqueued

    A reseat is three launches (assign, harvest + seat with the step-0 radius search, the seated slots' observations); the
    step after it builds every slot's graph again, a seated slot's at the radius its seat grew: the same bits.

    Scope: tie_mode 'lowest' or 'hashed' (hashing (seed, slot, global step)), maps of at most MAX_TEAM_CELLS cells.
    N <= MAX_AGENTS (use RolloutStream), N > MAX_TEAM, a larger map, 'replay', 'mt19937', record=... and trace=... (the
    per-case trace of a large-team stream does not exist yet: gnnpp_rollout_stream_trace_* refuse N > MAX_AGENTS) are
    refused by name before anything is enqueued."""

    def __init__(self, grids, starts, goals, maxstep, device, slots=16, commR=6.0, tie_mode='lowest', seed=0,
                 reseat_every=1, graph='dense', record=False, trace=False):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _native.GnnppError('TeamRolloutStream needs a HIP device (no CPU fallback)')
        if tie_mode not in _TIE:
            raise _native.GnnppError('unknown tie_mode %r (one of %s)' % (tie_mode, sorted(_TIE)))
        if tie_mode in ('replay', 'mt19937'):
            raise _native.GnnppError("TeamRolloutStream: tie_mode %r keeps per-episode state that a seat would have to "
                                     "rewind; use 'lowest' or 'hashed'" % tie_mode)
        if record is not False and record is not None:
            raise _native.GnnppError('TeamRolloutStream: record=... is not supported (a trace is laid out per episode of a '
                                     'fixed batch); use BatchedRollout(record=...)')
        if trace is not False and trace is not None:
            raise _native.GnnppError('TeamRolloutStream: trace=... is not supported yet: the per-case trace of a stream '
                                     'covers teams of at most %d agents (RolloutStream(trace=...))' % MAX_AGENTS)
        if graph not in GRAPHS:
            raise _native.GnnppError('unknown graph %r (one of %s)' % (graph, list(GRAPHS)))
        starts_t, goals_t, g = torch.as_tensor(starts), torch.as_tensor(goals), torch.as_tensor(grids)
        C, N = int(starts_t.shape[0]), int(starts_t.shape[1])
        if N <= MAX_AGENTS:
            raise _native.GnnppError('TeamRolloutStream: N <= %d (got N = %d) is not supported: use RolloutStream, whose '
                                     'seat runs the one-wave kernels' % (MAX_AGENTS, N))
        if N > MAX_TEAM:
            raise _native.GnnppError('TeamRolloutStream: N > %d (got N = %d) is not supported: at most %d agents per '
                                     'episode' % (MAX_TEAM, N, MAX_TEAM))
        if int(g.shape[-2]) * int(g.shape[-1]) > MAX_TEAM_CELLS:
            raise _native.GnnppError('TeamRolloutStream: a map of at most %d cells (got %d x %d)'
                                     % (MAX_TEAM_CELLS, int(g.shape[-2]), int(g.shape[-1])))
        if C < 1 or int(slots) < 1 or int(reseat_every) < 1:
            raise _native.GnnppError('TeamRolloutStream: at least one case, one slot and reseat_every >= 1')
        self.graph = graph
        self._open_queue(g, starts_t, goals_t, maxstep, dev, slots, commR, reseat_every)
        self._open_slots(tie_mode, seed, graph, _native.lib().gnnpp_rollout_team_stream_begin,
                         'gnnpp_rollout_team_stream_begin')
        self.trace = None

    def reseat(self):
        """RolloutStream.reseat with the large-team seat: three launches on the current stream, nothing read on the host.
        Seated slots get their step-0 state (radius growth, S or their columns of the lists block, observations) from the
        seat itself."""
        e = self.env
        lists, nbytes = (_p(e.lists), e.lists.numel()) if self.graph == 'lists' else (None, 0)
        with _native.device_guard(self.device):
            _native.check(_native.lib().gnnpp_rollout_team_stream_reseat(ctypes.byref(e._r), ctypes.byref(self._s), e.t, lists,
                                                                         nbytes, _native.stream_ptr(self.device)),
                          'gnnpp_rollout_team_stream_reseat')
        self._reseated_at = e.t
        if e.t == 0:
            e._state_step = 0         # every slot was just seated: the graph and the observations describe step 0

    def steps(self, model, n):
        """n policy steps of every slot, a reseat every `reseat_every` of them."""
        if self.graph == 'lists':
            self.env._check_lists_model(model)               # (before the reseat: nothing is enqueued for a planner refused)
        return RolloutStream.steps(self, model, n)


class GroupedRollout:
    """The same batch of episodes as `groups` BatchedRollouts over contiguous slices, each on its OWN HIP stream.
    Episodes are independent, so nothing orders one group's step t + 1 after another group's step t: the launch
    gap and the tail of one group's kernel (workgroups finish at different times, the observation stores drain)
    overlap with the other group's kernel.  Measured at C2 (512 episodes of 10 agents, one-launch steps): 44-49 us
    per step of all 512 episodes with two groups against 52-55 us on one stream.

    Same interface as BatchedRollout for what a rollout driver needs: steps(), run(), results(), and with record=... the
    groups' traces as one (`trace`).  tie_mode
    'lowest' and 'mt19937' give exactly the single-batch results (episode b keeps its generator seed + b);
    'hashed' hashes the episode's index inside its group, i.e. draws a different -- equally arbitrary -- stream."""

    def __init__(self, grid, starts, goals, maxstep, device, groups=2, seed=0, record=False, **kw):
        starts, goals = torch.as_tensor(starts), torch.as_tensor(goals)
        g = torch.as_tensor(grid)
        B = int(starts.shape[0])
        ms = torch.as_tensor(maxstep)
        if record is True:                                   # one T_cap for every group: the slices form one trace
            record = int(ms.max())
        groups = max(1, min(int(groups), B))
        bounds = [round(i * B / groups) for i in range(groups + 1)]
        self.envs, self.streams, self.slices = [], [], []
        dev = torch.device(device)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            sd = seed[lo:hi] if hasattr(seed, '__len__') else int(seed) + lo
            self.envs.append(BatchedRollout(g[lo:hi] if g.dim() == 3 else g, starts[lo:hi], goals[lo:hi],
                                            ms[lo:hi] if ms.dim() else ms, dev, seed=sd, record=record, **kw))
            self.streams.append(torch.cuda.Stream(device=dev))
            self.slices.append((lo, hi))
        self.device, self.B, self.N = dev, B, self.envs[0].N

    def _each(self, fn, wait_caller=True, model=None):
        cur = torch.cuda.current_stream(self.device)
        if model is not None and hasattr(model, 'materialize_packs'):
            # The model's lazily built device caches (packed encoder, packed taps, head pointers) are rebuilt on
            # whichever stream touches them first after a weight change.  Build them HERE, on the caller's stream,
            # which every group stream then waits for -- otherwise the second group could launch on a pack the
            # first group's stream is still writing (a cross-stream read-before-write race).
            if model.materialize_packs():
                wait_caller = True                           # (the groups must see the packs just enqueued)
        for env, st in zip(self.envs, self.streams):
            if wait_caller:
                st.wait_stream(cur)                          # whatever the caller's stream prepared (the episodes'
            with torch.cuda.stream(st):                      # state, new weights) is visible to the group
                fn(env)

    @property
    def t(self):
        return self.envs[0].t                                # (all groups step together)

    @property
    def trace(self):
        """record: the groups' traces as ONE RolloutTrace, their slices concatenated in episode order (a copy, made behind
        a join()); None for an unrecorded rollout."""
        parts = [e.trace for e in self.envs]
        if parts[0] is None:
            return None
        self.join()
        e0 = self.envs[0]
        cat = lambda name: torch.cat([getattr(p, name) for p in parts], 0)                       # noqa: E731
        grid = torch.cat([e.grid for e in self.envs], 0) if e0.grid_batched else e0.grid
        return RolloutTrace(self, grid, e0.grid_batched, torch.cat([e.goal for e in self.envs], 0), parts[0].T_cap,
                            tuple(cat(k) for k in ('path', 'action', 'moves', 'shielded', 'steps', 'seen_done')))

    def join(self):
        """Make the caller's stream wait for every group's work."""
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            cur.wait_stream(st)

    def steps(self, model, n, wait_caller=True):
        """n steps of every group.  wait_caller=False: the groups do not wait for the caller's stream first --
        for back-to-back bursts with nothing in between (after a join() a wait would be a barrier across the
        groups: the faster group would idle until the slower one has finished the previous burst)."""
        self._each(lambda env: env.steps(model, n), wait_caller, model)

    def run(self, model, max_steps=None, check_every=8):
        limit = max(int(e.maxstep.max().item()) for e in self.envs) if max_steps is None else int(max_steps)
        steps = 0
        while steps < limit:
            burst = min(check_every - steps % check_every, limit - steps)
            self.steps(model, burst, wait_caller=steps == 0)
            steps += burst
            if steps % check_every == 0:
                self.join()
                if hasattr(model, 'check_range'):
                    model.check_range()
                if all(bool((e.done != 0).all().item()) for e in self.envs):
                    break
        self.join()
        if hasattr(model, 'check_range'):
            model.check_range()
        return self.results()

    def results(self):
        self.join()
        parts = [e.results() for e in self.envs]
        out = {'steps': max(p['steps'] for p in parts)}
        for k in parts[0]:
            if k != 'steps':
                out[k] = torch.cat([p[k] for p in parts], 0)
        return out


class GraphedPolicyStep:
    """`model.addGSO(S); model(obs)` of a fixed batch shape as ONE HIP-graph replay.

    For small batches -- one test case per step as in the reference's rollout loop
    (agents/decentralplannerlocal.py:560-599), or the 16-graph shard a rank holds when a 128-graph batch of
    100-agent teams is split over 8 GPUs -- the policy step is a chain of one to three kernels that fill a
    fraction of the chip, and the launch boundaries between them are a tenth of the step.  The libgnnpp
    kernels are enqueued on torch's capture stream through the C ABI like any other launch, so the whole
    step (GSO hand-over, encoder, filter + head) becomes one graph; inputs are copied into static buffers
    before a replay, the returned logits are the graph's own output tensors (valid until the next call).

        step = GraphedPolicyStep(model, obs, S)        # eval mode; captures on the current device
        logits = step(obs_t, S_t)                      # list of N tensors [B, 5], as model(obs) returns

    The weights are FROZEN at capture: the graph holds the device addresses of the model's packed weight copies
    (encoder pack, filter taps, head constants).  The step keeps those buffers alive and, before every replay,
    compares the caches' keys (parameter version counters / identities: host-only, a few us) with the captured ones;
    after load_state_dict / an optimizer step / .to() it RE-CAPTURES (`recaptures` counts them) instead of replaying
    freed or stale buffers.  precision='split_f16' with range_policy='strict' is refused: its range check reads a
    device flag on the host, which cannot happen inside a capture (use range_policy='flag' + check_range()).

    Bit-identical to the eager call (tests/test_gpu_parity.py::test_graphed_policy_step_equals_eager)."""

    def __init__(self, model, obs, S, warmup=3):
        if model.training:
            raise ValueError('GraphedPolicyStep captures the eval-mode forward (BatchNorm folded into the packed weights)')
        if getattr(model, 'precision', 'fp32') == 'split_f16' and getattr(model, 'range_policy', None) == 'strict':
            raise ValueError("GraphedPolicyStep cannot capture precision='split_f16' with range_policy='strict' (the "
                             "range check synchronises with the host); use range_policy='flag' and check_range()")
        self.model = model
        self.obs = obs.clone()
        self.S = S.clone()
        self.warmup = warmup
        self.recaptures = -1
        self._retired = []                                 # graphs (and their output pools) replaced by a re-capture
        self._capture()

    def _capture(self):
        model = self.model
        if self.recaptures >= 0:
            # a re-capture used to release the old graph's private pool while logits returned by earlier
            # calls still viewed it, and ran warm-up + capture inside a latency-critical step without a word.  The
            # replaced graph (and with it the memory its outputs live in) is kept -- the last few of them -- and the
            # caller is told.
            import warnings
            self._retired = (self._retired + [(self.graph, self.out)])[-4:]
            warnings.warn('GraphedPolicyStep: the model\'s weights changed since the capture -- re-capturing (warm-up + '
                          'capture inside this call; outputs of earlier calls keep their old values)', RuntimeWarning,
                          stacklevel=3)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(self.warmup):                   # packs, workspaces, allocator
                model.addGSO(self.S)
                model(self.obs)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            model.addGSO(self.S)
            self.out = model(self.obs)
        # what the graph's kernels read through raw pointers: keep it alive, remember what it was built from
        self._keys, self._held = model.pack_state()
        self.recaptures += 1

    def __call__(self, obs, S):
        if obs.shape != self.obs.shape or S.shape != self.S.shape:
            raise ValueError('GraphedPolicyStep was captured for observations %s and GSOs %s'
                             % (tuple(self.obs.shape), tuple(self.S.shape)))
        if self.model.training:
            raise ValueError('GraphedPolicyStep replays the eval-mode forward: call model.eval() first')
        if self.model.pack_state()[0] != self._keys:       # weights changed since the capture
            self._capture()
        self.obs.copy_(obs)
        self.S.copy_(S)
        self.graph.replay()
        return self.out
