"""CPU: include/gnnpp_rollout_stream.h, the companion header of streamed rollouts, against its Python statement
(_native.ROLLOUT_STREAM_SIGNATURES and RolloutStreamStruct), with the parser and the comparison that hold _native.SIGNATURES
to include/gnnpp.h (tests/test_host_logic.py); the built library exports the calls, keeps its version and answers every
argument check before any HIP call; and the host side of rollout.RolloutStream."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header

FIELDS = ['case_grid', 'case_grid_batched', 'case_start', 'case_goal', 'case_maxstep', 'C', 'commR', 'cursor', 'slot_case',
          'slot_t0', 'assign', 'slot_grid', 'goal', 'maxstep', 'reached', 'start_step', 'end_step', 'pos', 'radius', 'stats',
          'lived', 'slot', 't0']


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_rollout_stream.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.ROLLOUT_STREAM_SIGNATURES) == ['gnnpp_rollout_stream_begin',
                                                                       'gnnpp_rollout_stream_reseat']
    assert list(structs) == ['gnnpp_rollout_stream'] and defines == {}
    assert [f[0] for f in structs['gnnpp_rollout_stream']] == FIELDS
    fields = {'gnnpp_rollout_stream': _native.RolloutStreamStruct._fields_}
    assert _abi_mismatches(header, _native.ROLLOUT_STREAM_SIGNATURES, fields, {}) == []
    others = (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) | set(_native.CASEGEN_SIGNATURES) |
              set(_native.MAPF_AUDIT_SIGNATURES) | set(_native.ROLLOUT_TRACE_SIGNATURES) | set(_native.SCHEDULE_DRAW_SIGNATURES))
    assert not set(_native.ROLLOUT_STREAM_SIGNATURES) & others
    # the comparison must see a changed kind and a changed field order, or it would prove nothing
    restype, argtypes = _native.ROLLOUT_STREAM_SIGNATURES['gnnpp_rollout_stream_reseat']
    wrong = dict(_native.ROLLOUT_STREAM_SIGNATURES,
                 gnnpp_rollout_stream_reseat=(restype, argtypes[:2] + [ctypes.c_size_t] + argtypes[3:]))
    found = _abi_mismatches(header, wrong, fields, {})
    assert len(found) == 1 and found[0].startswith('gnnpp_rollout_stream_reseat:'), found
    f = list(_native.RolloutStreamStruct._fields_)
    f[8], f[9] = f[9], f[8]
    found = _abi_mismatches(header, _native.ROLLOUT_STREAM_SIGNATURES, {'gnnpp_rollout_stream': f}, {})
    assert len(found) == 1 and found[0].startswith('struct gnnpp_rollout_stream:'), found
    # gnnpp.h is what it was: 59 prototypes, and the rollout's struct has no new field
    main = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp.h')).read())
    assert len(main[0]) == 59 and len(main[1]['gnnpp_rollout']) == len(_native.RolloutStruct._fields_)
    assert list(main[0]) == list(_native.SIGNATURES)


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
    S_PTRS = [f for f in FIELDS if f not in ('case_grid_batched', 'C', 'commR')]

    def structs(batched=1, **kw):
        r, s = _native.RolloutStruct(), _native.RolloutStreamStruct()
        for k in R_PTRS:
            setattr(r, k, fake)
        for k in S_PTRS:
            setattr(s, k, fake)
        r.B, r.N, r.H, r.W, r.grid_batched, r.tie_mode = 3, 10, 20, 20, batched, 0
        s.C, s.commR, s.case_grid_batched = 8, 6.0, batched
        for k, v in kw.items():
            name = k[2:] if k[:2] in ('r_', 's_') else k
            setattr(r if k.startswith('r_') or (not k.startswith('s_') and hasattr(r, name)) else s, name, v)
        return r, s

    def reseat(now=0, **kw):
        r, s = structs(**kw)
        return lib.gnnpp_rollout_stream_reseat(ctypes.byref(r), ctypes.byref(s), now, None)

    def begin(**kw):
        r, s = structs(**kw)
        return lib.gnnpp_rollout_stream_begin(ctypes.byref(r), ctypes.byref(s), None)

    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    r, s = structs()
    for call in (lib.gnnpp_rollout_stream_begin, lambda a, b, c: lib.gnnpp_rollout_stream_reseat(a, b, 0, c)):
        assert call(None, ctypes.byref(s), None) == call(ctypes.byref(r), None, None) == call(None, None, None) == E
    for call in (begin, reseat):
        assert call(B=0) == call(N=0) == call(H=0) == call(W=-1) == call(C=0) == E
        assert call(r_pos=None) == call(done=None) == E
        for k in S_PTRS:
            if k != 'slot_grid':
                assert call(**{'s_' + k: None}) == E, k
        assert call(r_grid_batched=0) == call(s_case_grid_batched=0) == E             # the two disagree
        assert call(tie_mode=-1) == call(tie_mode=4) == E
        assert call(N=129) == call(H=257, W=256) == U                                 # the team and the map outside the limits
        assert call(tie_mode=_native.TIE_REPLAY) == call(tie_mode=_native.TIE_MT19937) == U     # the refused modes
        assert call(N=129, r_pos=None) == E                                           # pointers first
    for k in R_PTRS:
        assert reseat(**{'r_' + k: None}) == E, k
    assert reseat(s_slot_grid=None) == reseat(s_slot_grid=other) == E                 # per-case maps: the slots' map is r->grid
    assert reseat(batched=0, s_case_grid=other) == E                                  # one shared map: it is r->grid
    assert reseat(s_goal=other) == reseat(s_maxstep=other) == E
    assert reseat(commR=0.0) == reseat(commR=-1.0) == reseat(commR=float('nan')) == reseat(commR=float('inf')) == E
    assert reseat(now=-1) == reseat(now=2**30 + 1) == E


def test_host_side_of_the_stream():
    import inspect
    import numpy as np
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.rollout import BatchedRollout, RolloutStream
    p = inspect.signature(RolloutStream.__init__).parameters
    assert [p[k].default for k in ('slots', 'commR', 'tie_mode', 'seed', 'reseat_every')] == [512, 6.0, 'lowest', 0, 1]
    assert {'steps', 'run', 'move', 'reseat', 'results'} <= set(vars(RolloutStream))
    assert 'slots' not in inspect.signature(BatchedRollout.__init__).parameters       # the plain rollout is what it was
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        RolloutStream(np.zeros((4, 4), np.uint8), np.zeros((1, 2, 2), np.int64), np.ones((1, 2, 2), np.int64), 5, 'cpu')
