"""TEST INFRASTRUCTURE ONLY: the one-wave simulator (csrc/rollout_kernels.hip: teams of at most 128 agents) at its map and
team-size edges.  Each case is built once here, with the facts the sequential oracle's answer must show, and runs through
ONE runner that takes a backend: the host emulation (tests/test_emu_rollout_sim.py) and the device
(tests/test_gpu_rollout_sim_cases.py).  A plain helper module, not a conftest.  The runner serves both simulators:
tests/rollout_team_sim_cases.py brings the cases of the large-team kernels (N > 128) to it.

A case is dict(name, grids [B,H,W] or [H,W] (shared), starts / goals [B,N,2], maxstep [B], actions [T,B,N] (T <= 4),
radius, grow, grid_skew (bytes the map pointer is moved off its 64-byte alignment), check(case, trace)).

What run_case does (tie rule 'lowest'; every comparison is an equality of bytes):
  (a) separate launches: observe, gso (grow as the case says), then per step move, observe, gso.  obs against
      ro.build_observations; S (float32 of the oracle's fp64), radius and connected against ro.communication_gso;
      positions, flags, reached, start / end steps, done, tie-break counts and statistics against ro.loop_step;
  (b) a twin state: gnnpp_rollout_gso_observe, then per step gnnpp_rollout_step (and gso_observe again on the new
      positions): every buffer has the bytes of (a);
  (c) run_policy_case (device only, N <= 16): gnnpp_rollout_policy_step against gnnpp_policy_fwd + (a)'s launches.
Every output of a call is poisoned before it (floats NaN, integers -7; the statistics too, so a call that does not end
an episode must leave them poisoned), every buffer sits between sentinel margins that must keep their bits, every call
is made twice from the same state and must give the same bytes, and inputs (map, goals, limits, actions) never change."""
import ctypes
import functools

import numpy as np

import rollout_lists_cases as lc
from gnn_pathplanning_amd._native import ERR_UNSUPPORTED, RolloutStruct
from oracle import rollout_oracle as ro
from rollout_team_cases import Recorder

SENTINEL, MARGIN, POISON = 0xA5, 64, -7


# ---- buffers between sentinel margins --------------------------------------------------------------------------------
def _store(buf, off, data):
    """bytes `data` (uint8 array) into a backend buffer at byte offset `off` (host array or device tensor)."""
    flat = buf._keep
    if isinstance(flat, np.ndarray):
        flat[off:off + data.size] = data
    else:
        import torch
        flat[off:off + data.size] = torch.from_numpy(np.array(data)).to(flat.device)


class Guarded:
    """An array on the backend, 64-byte aligned (+ skew bytes), with MARGIN sentinel bytes on either side."""

    def __init__(self, bk, a, skew=0):
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.nbytes = a.dtype, a.shape, a.nbytes
        self.buf = bk.put(np.full(a.nbytes + 2 * MARGIN + 64 + skew, SENTINEL, np.uint8))
        self.off = MARGIN + (-(self.buf.ptr.value + MARGIN)) % 64 + skew
        self.ptr = self.buf.ptr.value + self.off
        self.write(a)

    def write(self, a):
        _store(self.buf, self.off, np.frombuffer(np.ascontiguousarray(a, self.dtype).tobytes(), np.uint8))

    def fill(self, value):
        self.write(np.full(self.shape, value, self.dtype))

    def payload(self, raw):
        """The array inside a copy of the whole buffer; the margins must still be sentinels."""
        edge = np.concatenate([raw[:self.off], raw[self.off + self.nbytes:]])
        assert (edge == SENTINEL).all(), 'a sentinel margin was written'
        return raw[self.off:self.off + self.nbytes].copy().view(self.dtype).reshape(self.shape)


OUTPUTS = {'observe': ('obs',), 'gso': ('S', 'connected'), 'gso_observe': ('obs', 'S', 'connected'),
           'move': ('flags', 'choice_count', 'stats'), 'step': ('obs', 'S', 'connected', 'flags', 'choice_count', 'stats')}
INPUTS = ('grid', 'goal', 'maxstep', 'actions')


class SimState:
    """The buffers of B episodes on a backend and the gnnpp_rollout struct that points at them."""

    def __init__(self, bk, case, logits=False):
        self.bk, self.case = bk, case
        B, N = case['starts'].shape[:2]
        grids = case['grids']
        i32 = lambda shape, v: np.full(shape, v, np.int32)                         # noqa: E731
        g = self.g = {
            'grid': Guarded(bk, grids, case.get('grid_skew', 0)), 'goal': Guarded(bk, case['goals']),
            'pos': Guarded(bk, case['starts']), 'obs': Guarded(bk, np.full((B, N, 3, 11, 11), np.nan, np.float32)),
            'radius': Guarded(bk, np.broadcast_to(np.asarray(case['radius'], np.float64), (B,))),
            'S': Guarded(bk, np.full((B, N, N), np.nan, np.float32)), 'connected': Guarded(bk, i32(B, POISON)),
            'reached': Guarded(bk, i32((B, N), 0)), 'start_step': Guarded(bk, i32((B, N), -1)),
            'end_step': Guarded(bk, i32((B, N), -1)), 'maxstep': Guarded(bk, case['maxstep']),
            'done': Guarded(bk, i32(B, 0)), 'flags': Guarded(bk, i32((B, 3), POISON)),
            'stats': Guarded(bk, i32((B, 2), POISON)), 'choice_count': Guarded(bk, i32(B, POISON)),
            'actions': Guarded(bk, i32((B, N), 4))}
        if logits:
            g['logits'] = Guarded(bk, np.full((N, B, 5), np.nan, np.float32))
        r = self.r = RolloutStruct()
        r.grid, r.grid_batched, r.goal, r.pos = g['grid'].ptr, int(grids.ndim == 3), g['goal'].ptr, g['pos'].ptr
        r.B, r.N, r.H, r.W = B, N, grids.shape[-2], grids.shape[-1]
        r.obs, r.radius, r.S, r.connected = g['obs'].ptr, g['radius'].ptr, g['S'].ptr, g['connected'].ptr
        r.reached, r.start_step, r.end_step = g['reached'].ptr, g['start_step'].ptr, g['end_step'].ptr
        r.maxstep, r.done, r.flags, r.stats = g['maxstep'].ptr, g['done'].ptr, g['flags'].ptr, g['stats'].ptr
        r.tie_mode, r.choice_count = 0, g['choice_count'].ptr
        r.logits, r.actions = (g['logits'].ptr, None) if logits else (None, g['actions'].ptr)

    def poison(self, names):
        for name in names:
            self.g[name].fill(np.nan if self.g[name].dtype.kind == 'f' else POISON)

    def read(self):
        """name -> array of every buffer (margins checked)."""
        self.bk.sync()
        return {k: b.payload(b.buf.get()) for k, b in self.g.items()}

    def call(self, what, fn=None, want_rc=0, poison=None):
        """Poison the call's outputs and make it, twice from the same state: the same return code and bytes; inputs
        unchanged.  fn(r, stream) defaults to the library's gnnpp_rollout_<what>.  Returns what read() returns."""
        fn = fn or getattr(self.bk.lib, 'gnnpp_rollout_' + what)
        where = (self.case['name'], what, self.r.currentstep)
        self.bk.sync()
        before = {k: b.buf.get() for k, b in self.g.items()}
        outs = []
        for rep in range(2):
            if rep:
                for k, b in self.g.items():
                    _store(b.buf, 0, before[k])
            self.poison(OUTPUTS[what] if poison is None else poison)
            rc = fn(ctypes.byref(self.r), self.bk.stream)
            assert rc == want_rc, where + (rc,)
            outs.append(self.read())
        for k in outs[0]:
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), where + (k, 'second call differs')
        for k in INPUTS:
            assert outs[0][k].tobytes() == self.g[k].payload(before[k]).tobytes(), where + (k, 'input changed')
        return outs[0]


def same_bytes(where, got, want, names=None):
    for k in names or want:
        assert got[k].tobytes() == want[k].tobytes(), where + (k,)


# ---- the oracle's answer, computed once per case ----------------------------------------------------------------------
_TRACES = {}


def oracle_trace(case):
    """obs / S (float32) / radius / connected for the positions before step 0 and after every step ([T+1, B, ...]), and
    per step pos, flags, reached, start_step, end_step, done, calls (tie-breaks) and stats ([POISON, POISON] except in the
    call that ends the episode's loop), from oracle.rollout_oracle alone."""
    if case['name'] in _TRACES:
        return _TRACES[case['name']]
    T, B, N = case['actions'].shape
    grids = case['grids']
    grid = lambda b: grids[b] if grids.ndim == 3 else grids                    # noqa: E731
    eps = [ro.EpisodeState(grid(b), case['goals'][b], case['starts'][b], case['maxstep'][b]) for b in range(B)]
    radius = np.broadcast_to(np.asarray(case['radius'], np.float64), (B,)).copy()
    tr = {'obs': np.zeros((T + 1, B, N, 3, 11, 11), np.float32), 'S': np.zeros((T + 1, B, N, N), np.float32),
          'radius': np.zeros((T + 1, B), np.float64), 'connected': np.zeros((T + 1, B), np.int32),
          'pos': np.zeros((T + 1, B, N, 2), np.int32), 'flags': np.zeros((T, B, 3), np.int32),
          'reached': np.zeros((T, B, N), np.int32), 'start_step': np.zeros((T, B, N), np.int32),
          'end_step': np.zeros((T, B, N), np.int32), 'done': np.zeros((T, B), np.int32),
          'choice_count': np.zeros((T, B), np.int32), 'stats': np.full((T, B, 2), POISON, np.int32)}
    none = lambda values: [-1 if v is None else int(v) for v in values]        # noqa: E731
    for t in range(T + 1):
        for b, ep in enumerate(eps):
            tr['pos'][t, b] = ep.cur
            tr['obs'][t, b] = ro.build_observations(grid(b), ep.goal, ep.cur)
            S, radius[b], conn = ro.communication_gso(ep.cur, radius[b], bool(case['grow']) and t == 0)
            tr['S'][t, b], tr['radius'][t, b], tr['connected'][t, b] = S.astype(np.float32), radius[b], int(conn)
        if t == T:
            break
        for b, ep in enumerate(eps):
            rec, was_done = Recorder(ep, lambda c: c[0]), ep.done
            tr['flags'][t, b] = [int(v) for v in ro.loop_step(ep, case['actions'][t, b], t + 1, rec)]
            tr['reached'][t, b] = [int(v) for v in ep.reached]
            tr['start_step'][t, b], tr['end_step'][t, b] = none(ep.start_step), none(ep.end_step)
            tr['done'][t, b], tr['choice_count'][t, b] = int(ep.done), rec.calls
            if ep.done and not was_done:
                tr['stats'][t, b] = [ep.makespan, ep.flowtime]
    if case.get('check'):
        case['check'](case, tr)
    _TRACES[case['name']] = tr
    return tr


MOVED = ('flags', 'reached', 'start_step', 'end_step', 'done', 'choice_count', 'stats')
GRAPH = ('S', 'radius', 'connected')


def _expect(where, got, tr, t, names):
    for k in names:
        assert got[k].tobytes() == np.ascontiguousarray(tr[k][t]).tobytes(), where + (k,)


def run_case(bk, case):
    """(a) and (b) of the module's docstring.  Returns the oracle's trace."""
    tr = oracle_trace(case)
    T = case['actions'].shape[0]
    a, twin = SimState(bk, case), SimState(bk, case)
    name = case['name']
    a.r.grow = int(case['grow'])
    got = a.call('observe')
    _expect((name, 'observe', 0), got, tr, 0, ('obs',))
    got = a.call('gso')
    _expect((name, 'gso', 0), got, tr, 0, GRAPH + ('obs',))
    # the twin starts from the radius step 0 found (gso_observe never grows it)
    twin.g['radius'].write(tr['radius'][0])
    twin.r.grow = 0
    same_bytes((name, 'gso_observe', 0), twin.call('gso_observe'), got, ('obs',) + GRAPH + ('pos',))
    for t in range(T):
        for st in (a, twin):
            st.g['actions'].write(case['actions'][t])
            st.r.currentstep, st.r.grow = t + 1, 0
        got = a.call('move')
        _expect((name, 'move', t), got, tr, t, MOVED)
        _expect((name, 'move', t), got, tr, t + 1, ('pos',))
        got = a.call('observe')
        _expect((name, 'observe', t + 1), got, tr, t + 1, ('obs',))
        got = a.call('gso')
        _expect((name, 'gso', t + 1), got, tr, t + 1, GRAPH + ('obs', 'pos'))
        _expect((name, 'gso', t + 1), got, tr, t, MOVED)
        same_bytes((name, 'step', t), twin.call('step'), got)
        same_bytes((name, 'gso_observe', t + 1), twin.call('gso_observe'), got)
    return tr


def run_unsupported(bk, case):
    """A map past the one-wave limit: observe, gso_observe and step answer GNNPP_ERR_UNSUPPORTED and write nothing."""
    st = SimState(bk, case)
    st.r.currentstep, st.r.grow = 1, 0
    everything = OUTPUTS['step'] + ('pos', 'reached', 'start_step', 'end_step', 'done')
    for what in ('observe', 'gso_observe', 'step'):
        got = st.call(what, want_rc=ERR_UNSUPPORTED, poison=everything)
        for k in everything:
            assert (np.isnan(got[k]) if got[k].dtype.kind == 'f' else got[k] == POISON).all(), (case['name'], what, k)


def run_policy_case(bk, case, net, precision):
    """(c): gnnpp_rollout_policy_step on a twin against net.forward_logits (gnnpp_policy_fwd) + move, observe, gso on the
    same logits: logits and every buffer identical after every step.  net: a DecentralPlannerNet in eval mode on bk.dev
    with numAgents = N and the precision under test.  want: GNNPP_OK on every step."""
    import torch
    tr = oracle_trace(case)
    T, B, N = case['actions'].shape
    a, twin = SimState(bk, case, logits=True), SimState(bk, case, logits=True)
    enc, taps, gb, aw, ab, K = net.policy_pointers()
    prec = net._prec()
    twin.r.range_flag = net._flag(bk.dev).data_ptr() if precision == 'split_f16' else None

    def policy_step(r, stream):
        return bk.lib.gnnpp_rollout_policy_step(r, enc, taps, gb, aw, ab, K, prec, stream)

    for st in (a, twin):
        st.r.grow = int(case['grow'])
        st.call('observe')
        got = st.call('gso')
        _expect((case['name'], 'gso', 0), got, tr, 0, GRAPH + ('obs',))
    for t in range(T):
        with torch.no_grad():
            net.addGSO(torch.from_numpy(got['S']).to(bk.dev))
            lg = net.forward_logits(torch.from_numpy(got['obs']).to(bk.dev)).cpu().numpy()
        assert lg.shape == (N, B, 5) and np.isfinite(lg).all()
        a.g['logits'].write(lg)
        for st in (a, twin):
            st.r.currentstep, st.r.grow = t + 1, 0
        a.call('move')
        a.call('observe')
        got = a.call('gso')
        where = (case['name'], precision, 'policy_step', t)
        # (obs and S are the policy's inputs and the simulator's outputs: they are not poisoned here)
        same_bytes(where, twin.call('step', fn=policy_step, poison=OUTPUTS['move'] + ('connected', 'logits')), got)


# ---- instances ---------------------------------------------------------------------------------------------------------
def _case(name, grids, starts, goals, actions, maxstep=None, radius=2.0, grow=1, grid_skew=0, check=None):
    B = len(starts)
    maxstep = [50, 3, 2][:B] if maxstep is None else maxstep
    return {'name': name, 'grids': np.ascontiguousarray(grids, np.uint8), 'starts': np.ascontiguousarray(starts, np.int32),
            'goals': np.ascontiguousarray(goals, np.int32), 'actions': np.ascontiguousarray(actions, np.int32),
            'maxstep': np.broadcast_to(np.asarray(maxstep, np.int32), (B,)).copy(), 'radius': radius, 'grow': grow,
            'grid_skew': grid_skew, 'check': check}


def _random(seed, B, N, H, W, density, T=4, shared=False, box=None):
    """Random maps (one shared map: shared=True), N distinct free starts and goals per episode (starts inside the
    top-left box = (h, w) when given, so that agents collide), T steps of random joint actions."""
    rng = np.random.default_rng(seed)
    while True:
        grids = (rng.random((1 if shared else B, H, W)) < density).astype(np.uint8)
        if box:
            grids[:, :box[0], :box[1]] = 0
        room = [(g[:box[0], :box[1]] if box else g) == 0 for g in grids]
        if min(int(r.sum()) for r in room) >= N:
            break
    starts, goals = np.zeros((B, N, 2), np.int32), np.zeros((B, N, 2), np.int32)
    for b in range(B):
        g = grids[0 if shared else b]
        free = np.argwhere(g == 0)
        sfree = free if not box else free[(free[:, 0] < box[0]) & (free[:, 1] < box[1])]
        starts[b] = sfree[rng.choice(len(sfree), N, replace=False)]
        goals[b] = free[rng.choice(len(free), N, replace=False)]
    actions = rng.integers(0, 5, size=(T, B, N))
    return (grids[0] if shared else grids), starts, goals, actions


def _grid_of(case, b):
    return case['grids'][b] if case['grids'].ndim == 3 else case['grids']


def _check_non_square(case, tr):
    """Some view crosses each of the four map edges; some agent stands at a row index >= W (tall maps) or a column index
    >= H (wide maps), where a swapped H / W goes wrong; some agent sees another agent and an obstacle of the map."""
    H, W = case['grids'].shape[-2:]
    x, y = tr['pos'][..., 0], tr['pos'][..., 1]
    assert (x - 4 < 0).any() and (x + 4 >= H).any() and (y - 4 < 0).any() and (y + 4 >= W).any(), case['name']
    assert (x >= W).any() if H > W else (y >= H).any(), case['name']
    both = False
    for t, b, n in np.argwhere(tr['obs'][:, :, :, 2].sum((-1, -2)) > 1):
        cx, cy = tr['pos'][t, b, n]
        both |= bool(_grid_of(case, b)[max(cx - 4, 0):cx + 5, max(cy - 4, 0):cy + 5].any())
    assert both, case['name']


NON_SQUARE_SHAPES = ((7, 13, 6), (13, 7, 6), (20, 9, 16), (9, 20, 16), (5, 40, 33))


@functools.lru_cache(None)
def non_square_cases():
    cases = []
    for k, (H, W, N) in enumerate(NON_SQUARE_SHAPES):
        for shared in (False, True):
            inst = _random(100 + k, 2, N, H, W, 0.12, shared=shared)
            cases.append(_case('non_square/%dx%d/N%d/%s' % (H, W, N, 'shared' if shared else 'batched'), *inst,
                               check=_check_non_square))
    return cases


FOV_SHAPES = ((1, 9, 3), (9, 1, 3), (3, 3, 4), (2, 9, 5), (11, 11, 7))


@functools.lru_cache(None)
def fov_cases():
    """Maps that lie inside the 11 x 11 frame of every agent on them."""
    return [_case('inside_fov/%dx%d/N%d' % (H, W, N), *_random(200 + k, 2, N, H, W, 0.1))
            for k, (H, W, N) in enumerate(FOV_SHAPES)]


# observe_stage fetches the map 16 cells per load (H*W % 16 == 0 and the episode's map 16-byte aligned), 4 cells per load
# (% 4, 4-byte aligned) or byte by byte.  Restated here from the map's size and the pointers the call is given.
def load_paths(case, grid_ptr):
    HW = case['grids'].shape[-2] * case['grids'].shape[-1]
    out = []
    for b in range(len(case['starts'])):
        p = grid_ptr + (b * HW if case['grids'].ndim == 3 else 0)
        out.append(16 if HW % 16 == 0 and p % 16 == 0 else 4 if HW % 4 == 0 and p % 4 == 0 else 1)
    return out


MAP_LOAD_SHAPES = ((8, 8), (4, 12), (6, 6), (10, 10), (7, 9), (5, 5))
MAP_LOAD_SKEWS = (1, 4, 16)


@functools.lru_cache(None)
def map_load_cases():
    """Three batched maps of N = 5 per shape (the buffer is 64-byte aligned, so episode b starts at b * H * W), and one
    shared 8 x 8 map handed in 1, 4 and 16 bytes past that alignment."""
    cases = [_case('map_load/%dx%d/batched' % (H, W), *_random(300 + k, 3, 5, H, W, 0.15))
             for k, (H, W) in enumerate(MAP_LOAD_SHAPES)]
    cases += [_case('map_load/8x8/shared/base+%d' % skew, *_random(310 + skew, 3, 5, 8, 8, 0.15, shared=True),
                    grid_skew=skew) for skew in MAP_LOAD_SKEWS]
    assert sorted({p for c in cases for p in load_paths(c, 64 + c['grid_skew'])}) == [1, 4, 16]
    assert [load_paths(c, 64 + c['grid_skew']) for c in cases] == \
        [[16] * 3, [16] * 3, [4] * 3, [4] * 3, [1] * 3, [1] * 3, [1] * 3, [4] * 3, [16] * 3]
    return cases


def _check_tie_breaks(case, tr):
    assert (tr['choice_count'].sum(0) >= 1).all(), (case['name'], tr['choice_count'].sum(0))


TEAM_SIZES = (1, 2, 16, 17, 32, 33, 63, 64, 65, 127, 128)


@functools.lru_cache(None)
def team_size_cases():
    """The kernels' own seams: 16 observation agents per workgroup, 256 / 1024 threads of the step kernel at N = 32 / 33,
    the second agent per lane from N = 65, the last one-wave sizes.  24 x 24 maps (12 x 12 up to N = 17), 4 % obstacles,
    the starts packed into a corner at about two cells per agent; from N = 16 on every episode breaks a tie."""
    cases = []
    for N in TEAM_SIZES:
        W = 12 if N <= 17 else 24
        side = min(W, int(np.ceil(np.sqrt(2 * N))))
        cases.append(_case('team/N%d/on_%d' % (N, W), *_random(400 + N, 2, N, W, W, 0.04, box=(side, side)),
                           maxstep=[50, 3], check=_check_tie_breaks if N >= 16 else None))
    return cases


TEAM_DENSE_FLOOR = 700


@functools.lru_cache(None)
def team_dense_case():
    """128 agents on 12 x 12 without obstacles (144 cells: the one-wave counterpart of rollout_cases' 129 on 16 x 16),
    two episodes, four steps of random joint actions.  The oracle alone, on the CPU, counts 749 tie-breaks on this
    instance (417 and 332 per episode): the floor is 700."""
    def check(case, tr):
        assert tr['choice_count'].sum() > TEAM_DENSE_FLOOR, int(tr['choice_count'].sum())
    return _case('team/N128/dense_on_12', *_random(528, 2, 128, 12, 12, 0.0), maxstep=[50, 50], check=check)


def _graph_case(name, pos, radius, H, W, check):
    """A hand-built graph state on an empty map: every action is 4 (stop), so every step rebuilds the same graph."""
    pos = np.asarray(pos, np.int32)
    B, N = pos.shape[:2]
    assert pos.min() >= 0 and pos[..., 0].max() < H and pos[..., 1].max() < W
    return _case('graph/' + name, np.zeros((H, W), np.uint8), pos, pos[:, ::-1], np.full((2, B, N), 4), maxstep=[50] * B,
                 radius=radius, grow=0, check=check)


def _radius5_state():
    """Pairs exactly 5 apart -- (3, 4), (5, 0), (0, 5) -- which the oracle's strict `<` leaves unconnected at radius 5.0,
    next to pairs at 4 and sqrt(18) that it connects."""
    base = [(0, 0), (20, 0), (0, 20), (20, 20), (10, 10)]
    offs = [(3, 4), (5, 0), (0, 5), (4, 0), (3, 3)]
    return np.array([[p for (x, y), (dx, dy) in zip(base, offs) for p in ((x, y), (x + dx, y + dy))]])


def _check_graph(connected=None, isolated=None, degree=None, exact5=False):
    def check(case, tr):
        S, pos = tr['S'], tr['pos']
        assert (S == S[0]).all() and (pos == pos[0]).all()                     # nobody moves
        if connected is not None:
            assert (tr['connected'] == connected).all(), case['name']
        if isolated is not None:
            assert not S[0, 0, isolated].any() and not S[0, 0, :, isolated].any(), case['name']
            assert (np.delete(S[0, 0], isolated, 0) != 0).any(1).all(), case['name']
        if degree is not None:
            assert ((S[0] != 0).sum(-1) == degree).all(), case['name']
        if exact5:
            d2 = ((pos[0, 0][:, None] - pos[0, 0][None]) ** 2).sum(-1)
            i, j = np.nonzero(np.triu(d2 == 25))
            offsets = {tuple(abs(pos[0, 0, a] - pos[0, 0, b])) for a, b in zip(i, j)}
            assert len(i) >= 3 and offsets >= {(3, 4), (5, 0), (0, 5)} and not S[0, 0, i, j].any(), case['name']
            assert (S[0, 0] != 0).sum() >= 4, case['name']
    return check


@functools.lru_cache(None)
def graph_cases():
    """The hand-built positions of rollout_lists_cases.py with N <= 128, and four more, through the fused launches."""
    box = np.stack(np.unravel_index(np.random.default_rng(7).permutation(132)[:128], (12, 11)), 1)[None]
    return [
        _graph_case('outlier', lc._outlier(), 4.0, 64, 64, _check_graph(connected=0, isolated=17)),
        _graph_case('two_components', lc._two_components(), 6.0, 48, 48, _check_graph(connected=0)),
        _graph_case('chain70', lc._chain(70, 3), 3.5, 1, 208, _check_graph(connected=1)),
        _graph_case('chain128', lc._chain(128, 3), 3.5, 1, 382, _check_graph(connected=1)),
        _graph_case('packed_box128/degree127', box, 20.0, 12, 11, _check_graph(connected=1, degree=127)),
        _graph_case('radius5/strict_less', _radius5_state(), 5.0, 32, 32, _check_graph(connected=0, exact5=True)),
    ]


def all_cases():
    return non_square_cases() + fov_cases() + map_load_cases() + team_size_cases() + [team_dense_case()] + graph_cases()


# ---- device only: the launchers' LDS branches ---------------------------------------------------------------------------
# Derived from the launchers of csrc/rollout_kernels.hip, with occ = H*W rounded up to 16 and the cell map = occ for
# H*W <= 32 768 cells (kCellMapMaxCells), 0 beyond:
#   observe / gso_observe request 1 024 + occ bytes, + 23 232 (16 agents x 363 floats: the output stage) while the sum is
#     <= 65 536:  staged for occ <= 41 280;  more than 64 KB from occ = 64 528 on, i.e. H*W >= 64 513;
#   step requests 7 200 + occ + cell map, + N x 1 452 while the sum is <= 65 536:  at N = 16 staged for occ <= 17 552;
#     more than 64 KB for 2 occ > 58 336, i.e. 29 169 <= H*W <= 32 768, and again for occ > 58 336, i.e. H*W >= 58 337;
#   the largest accepted map has occ = 65 536 (256 x 256); one cell more is GNNPP_ERR_UNSUPPORTED.
# (H, W, N, what the pair straddles): the largest map on one side, the smallest on the other.
LDS_SHAPES = (
    (172, 240, 16, 'observe staged: 41 280 cells, the last'), (139, 297, 16, 'observe direct: 41 283 cells'),
    (16, 1097, 16, 'step staged at N = 16: 17 552 cells, the last'), (131, 134, 16, 'step direct at N = 16: 17 554 cells'),
    (181, 181, 16, 'cell map: 32 761 cells'), (128, 256, 16, 'cell map: 32 768 cells, the last'),
    (99, 331, 16, 'all-pairs scan: 32 769 cells, the first'), (182, 182, 16, 'all-pairs scan: 33 124 cells'),
    (16, 1823, 16, 'step with cell map, the last request of 64 KB: 29 168 cells'),
    (63, 463, 16, 'step with cell map, the first request above 64 KB: 29 169 cells'),
    (171, 171, 100, 'step with cell map above 64 KB: 29 241 cells, 100 agents'),
    (32, 1823, 16, 'step without cell map, the last request of 64 KB: 58 336 cells'),
    (126, 463, 16, 'step without cell map, the first request above 64 KB: 58 338 cells'),
    (242, 242, 16, 'step without cell map above 64 KB: 58 564 cells'),
    (252, 256, 16, 'observe, the last request of 64 KB: 64 512 cells'),
    (254, 254, 16, 'observe, the first request above 64 KB: 64 516 cells'),
    (256, 256, 128, 'the largest accepted map, 128 agents'), (256, 256, 10, 'the largest accepted map, 10 agents'),
)
UNSUPPORTED_SHAPES = ((257, 256, 16),)


def requests(H, W, N):
    """(observe bytes, observe staged, step bytes, step staged, cell map bytes) of the launchers, restated."""
    occ = (H * W + 15) & ~15
    obs = 1024 + occ
    obs_staged = obs + 23232 <= 65536
    cmap = occ if H * W <= 32768 else 0
    step = 7200 + occ + cmap
    step_staged = step + N * 1452 <= 65536
    return obs + 23232 * obs_staged, obs_staged, step + N * 1452 * step_staged, step_staged, cmap


@functools.lru_cache(None)
def lds_cases():
    """B = 2, two steps; agents and goals drawn over the whole map, so that goal offsets and row indices use its range."""
    cases = [_case('lds/%dx%d/N%d' % (H, W, N), *_random(600 + k, 2, N, H, W, 0.03, T=2), maxstep=[50, 2])
             for k, (H, W, N) in enumerate(s[:3] for s in LDS_SHAPES)]
    facts = {s[:2]: requests(*s[:3]) for s in LDS_SHAPES}
    # each threshold has a map on either side
    assert facts[(172, 240)][1] and not facts[(139, 297)][1] and facts[(16, 1097)][3] and not facts[(131, 134)][3]
    assert facts[(181, 181)][4] and facts[(128, 256)][4] and not facts[(99, 331)][4] and not facts[(182, 182)][4]
    assert facts[(16, 1823)][2] == 65536 and facts[(63, 463)][2] == 65568 and facts[(171, 171)][2] > 65536
    assert facts[(32, 1823)][2] == 65536 and facts[(126, 463)][2] == 65552 and facts[(242, 242)][2] > 65536
    assert facts[(252, 256)][0] == 65536 and facts[(254, 254)][0] == 65552
    assert facts[(256, 256)][0] == 66560 and facts[(256, 256)][2] == 72736
    assert max(f[0] for f in facts.values()) == 66560 and max(f[2] for f in facts.values()) == 72736
    return cases


@functools.lru_cache(None)
def unsupported_cases():
    return [_case('lds/%dx%d/unsupported' % (H, W), *_random(700 + k, 2, N, H, W, 0.03, T=1))
            for k, (H, W, N) in enumerate(UNSUPPORTED_SHAPES)]


# gnnpp_rollout_policy_step under GNNPP_PREC_FP32 documents 10 208 cells of spare LDS for the map
POLICY_MAP_FITS, POLICY_MAP_TOO_LARGE = (88, 116), (83, 123)


@functools.lru_cache(None)
def policy_map_cases():
    assert 88 * 116 == 10208 and 83 * 123 == 10209
    return [_case('policy_map/%dx%d/N10' % hw, *_random(800 + k, 2, 10, hw[0], hw[1], 0.05, T=3), maxstep=[50, 2])
            for k, hw in enumerate((POLICY_MAP_FITS, POLICY_MAP_TOO_LARGE))]
