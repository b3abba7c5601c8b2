"""CPU: include/gnnpp_rollout_team_stream.h, the companion header of streamed rollouts of large teams, against its Python
statement (_native.ROLLOUT_TEAM_STREAM_SIGNATURES), with the parser and the comparison that hold _native.SIGNATURES to
include/gnnpp.h (tests/test_host_logic.py): exactly two prototypes and no struct of its own; the built library exports the
calls, keeps its version and answers every argument check before any HIP call; and the host side of
rollout.TeamRolloutStream."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header

NAMES = ['gnnpp_rollout_team_stream_begin', 'gnnpp_rollout_team_stream_reseat']


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    text = open(os.path.join(ROOT, 'include', 'gnnpp_rollout_team_stream.h')).read()
    header = _parse_header(text)
    protos, structs, defines = header
    assert list(protos) == list(_native.ROLLOUT_TEAM_STREAM_SIGNATURES) == NAMES
    assert structs == {} and defines == {}                    # struct gnnpp_rollout_stream is reused, by inclusion
    assert '#include "gnnpp_rollout_stream.h"' in text
    assert _abi_mismatches(header, _native.ROLLOUT_TEAM_STREAM_SIGNATURES, {}, {}) == []
    others = (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) | set(_native.CASEGEN_SIGNATURES) |
              set(_native.MAPF_AUDIT_SIGNATURES) | set(_native.ROLLOUT_TRACE_SIGNATURES) |
              set(_native.SCHEDULE_DRAW_SIGNATURES) | set(_native.ROLLOUT_STREAM_SIGNATURES) |
              set(_native.CASEGEN_MAZE_SIGNATURES) | set(_native.ROLLOUT_STREAM_TRACE_SIGNATURES) |
              set(_native.MEASURE_SIGNATURES))
    assert not set(_native.ROLLOUT_TEAM_STREAM_SIGNATURES) & others
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.ROLLOUT_TEAM_STREAM_SIGNATURES[NAMES[1]]
    wrong = dict(_native.ROLLOUT_TEAM_STREAM_SIGNATURES)
    wrong[NAMES[1]] = (restype, argtypes[:4] + [ctypes.c_int] + argtypes[5:])             # lists_bytes as an int
    found = _abi_mismatches(header, wrong, {}, {})
    assert len(found) == 1 and found[0].startswith(NAMES[1] + ':'), found


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    fake, other = 64, 128                                     # (never dereferenced: every call here is refused)
    R_PTRS = ('grid', 'goal', 'pos', 'obs', 'radius', 'S', 'reached', 'start_step', 'end_step', 'maxstep', 'flags', 'stats',
              'done')
    S_PTRS = [f[0] for f in _native.RolloutStreamStruct._fields_ if f[0] not in ('case_grid_batched', 'C', 'commR')]
    N = 129
    need = lib.gnnpp_team_lists_bytes(3, N)
    assert need > 0

    def structs(batched=1, **kw):
        r, s = _native.RolloutStruct(), _native.RolloutStreamStruct()
        for k in R_PTRS:
            setattr(r, k, fake)
        for k in S_PTRS:
            setattr(s, k, fake)
        r.B, r.N, r.H, r.W, r.grid_batched, r.tie_mode = 3, N, 20, 20, batched, 0
        s.C, s.commR, s.case_grid_batched = 8, 6.0, batched
        for k, v in kw.items():
            name = k[2:] if k[:2] in ('r_', 's_') else k
            setattr(r if k.startswith('r_') or (not k.startswith('s_') and hasattr(r, name)) else s, name, v)
        return r, s

    def reseat(now=0, lists=None, lists_bytes=0, **kw):
        r, s = structs(**kw)
        return lib.gnnpp_rollout_team_stream_reseat(ctypes.byref(r), ctypes.byref(s), now, lists, lists_bytes, None)

    def reseat_lists(**kw):
        return reseat(lists=fake, lists_bytes=need, **kw)

    def begin(**kw):
        r, s = structs(**kw)
        return lib.gnnpp_rollout_team_stream_begin(ctypes.byref(r), ctypes.byref(s), None)

    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    r, s = structs()
    for call in (lib.gnnpp_rollout_team_stream_begin,
                 lambda a, b, c: lib.gnnpp_rollout_team_stream_reseat(a, b, 0, None, 0, c),
                 lambda a, b, c: lib.gnnpp_rollout_team_stream_reseat(a, b, 0, fake, need, c)):
        assert call(None, ctypes.byref(s), None) == call(ctypes.byref(r), None, None) == call(None, None, None) == E
    for call in (begin, reseat, reseat_lists):
        assert call(B=0) == call(N=0) == call(H=0) == call(W=-1) == call(C=0) == E
        assert call(r_pos=None) == call(done=None) == E
        for k in S_PTRS:
            if k != 'slot_grid':
                assert call(**{'s_' + k: None}) == E, k
        assert call(r_grid_batched=0) == call(s_case_grid_batched=0) == E             # the two disagree
        assert call(tie_mode=-1) == call(tie_mode=4) == E
        assert call(N=128) == call(N=10) == call(N=1025) == U                         # the team outside the limits ...
        assert call(H=257, W=256) == U                                                # ... and the map
        assert call(tie_mode=_native.TIE_REPLAY) == call(tie_mode=_native.TIE_MT19937) == U     # the refused modes
        assert call(N=128, r_pos=None) == call(N=1025, done=None) == E                # pointers first
    for k in R_PTRS:
        assert reseat(**{'r_' + k: None}) == E, k
        if k != 'S':
            assert reseat_lists(**{'r_' + k: None}) == E, k
    assert reseat_lists(r_S=None, N=128) == U                 # the lists form takes no S: it gets as far as the scope
    for call in (reseat, reseat_lists):
        assert call(s_slot_grid=None) == call(s_slot_grid=other) == E                 # per-case maps: the slots' map is r->grid
        assert call(batched=0, s_case_grid=other) == E                                # one shared map: it is r->grid
        assert call(s_goal=other) == call(s_maxstep=other) == E
        assert call(commR=0.0) == call(commR=-1.0) == call(commR=float('nan')) == call(commR=float('inf')) == E
        assert call(now=-1) == call(now=2**30 + 1) == E
    # the lists block: too small or misaligned is an argument error, before the scope is looked at
    assert reseat(lists=fake, lists_bytes=need - 1) == reseat(lists=fake, lists_bytes=0) == E
    assert reseat(lists=fake + 8, lists_bytes=need) == E
    assert reseat(lists=fake, lists_bytes=lib.gnnpp_team_lists_bytes(3, 128) - 1, N=128) == E
    assert reseat(lists=fake, lists_bytes=need, tie_mode=_native.TIE_REPLAY) == U


def test_host_side_of_the_team_stream():
    import inspect
    import numpy as np
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.rollout import RolloutStream, TeamRolloutStream
    p = inspect.signature(TeamRolloutStream.__init__).parameters
    assert list(p)[:12] == ['self', 'grids', 'starts', 'goals', 'maxstep', 'device', 'slots', 'commR', 'tie_mode', 'seed',
                            'reseat_every', 'graph']
    assert [p[k].default for k in ('slots', 'commR', 'tie_mode', 'seed', 'reseat_every', 'graph')] == \
        [16, 6.0, 'lowest', 0, 1, 'dense']
    for name in ('reseat', 'move', 'steps', 'run', 'finished', 'results', 't'):
        assert hasattr(TeamRolloutStream, name), name
    q = inspect.signature(RolloutStream.__init__).parameters                          # the small-team stream is what it was
    assert [q[k].default for k in ('slots', 'commR', 'tie_mode', 'seed', 'reseat_every', 'record', 'graph', 'trace')] == \
        [512, 6.0, 'lowest', 0, 1, False, 'dense', False]
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        TeamRolloutStream(np.zeros((4, 4), np.uint8), np.zeros((1, 2, 2), np.int64), np.ones((1, 2, 2), np.int64), 5, 'cpu')
