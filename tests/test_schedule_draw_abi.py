"""CPU: include/gnnpp_schedule_draw.h, the companion header of the draw from stored schedules, against its Python statement
(_native.SCHEDULE_DRAW_SIGNATURES), with the parser and the comparison that hold _native.SIGNATURES to include/gnnpp.h
(tests/test_host_logic.py); the built library exports the calls, keeps its version and checks the arguments before any
HIP call; and the host side of expert.SchedulePool."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_schedule_draw.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.SCHEDULE_DRAW_SIGNATURES) == ['gnnpp_schedule_draw_workspace_bytes',
                                                                      'gnnpp_schedule_draw']
    assert structs == {} and defines == {}
    assert _abi_mismatches(header, _native.SCHEDULE_DRAW_SIGNATURES, {}, {}) == []
    assert not set(_native.SCHEDULE_DRAW_SIGNATURES) & (
        set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) | set(_native.CASEGEN_SIGNATURES) |
        set(_native.MAPF_AUDIT_SIGNATURES) | set(_native.ROLLOUT_TRACE_SIGNATURES))
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.SCHEDULE_DRAW_SIGNATURES['gnnpp_schedule_draw']
    wrong = dict(_native.SCHEDULE_DRAW_SIGNATURES, gnnpp_schedule_draw=(restype, argtypes[:7] + [ctypes.c_int] + argtypes[8:]))
    found = _abi_mismatches(header, wrong, {}, {})
    assert len(found) == 1 and found[0].startswith('gnnpp_schedule_draw:'), found
    # gnnpp.h is what it was: the struct the draw reads has no new field
    main = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp.h')).read())
    assert len(main[0]) == 59 and len(main[1]['gnnpp_schedules']) == len(_native.ScheduleStruct._fields_)


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    assert lib.gnnpp_schedule_draw_workspace_bytes(10, 64) == 5120
    assert lib.gnnpp_schedule_draw_workspace_bytes(0, 1) == lib.gnnpp_schedule_draw_workspace_bytes(1025, 1) == 0
    assert lib.gnnpp_schedule_draw_workspace_bytes(10, 0) == 0
    fake = ctypes.c_void_p(1 << 20).value                     # (never dereferenced: every call here is refused)

    def draw(B=4, S=fake, lists=None, lists_bytes=0, ws_bytes=1 << 20, index=fake, **fields):
        s = _native.ScheduleStruct()
        s.grid = s.goal = s.pos = s.case_start = s.radius = s.status = fake
        s.C, s.N, s.H, s.W, s.T_total = 2, 10, 20, 20, 30
        for k, v in fields.items():
            setattr(s, k, v)
        return lib.gnnpp_schedule_draw(ctypes.byref(s), index, B, fake, fake, S, lists, lists_bytes, fake, ws_bytes, None)

    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    assert draw(B=0) == draw(S=None) == draw(lists=fake, lists_bytes=1 << 20) == draw(index=None) == E
    assert draw(N=1025) == draw(N=0) == draw(C=0) == draw(C=31) == draw(T_total=0) == draw(H=0) == E
    assert draw(radius=None) == draw(status=None) == draw(pos=None) == draw(ws_bytes=319) == draw(S=fake + 2) == E
    assert draw(S=None, lists=fake, lists_bytes=lib.gnnpp_team_lists_bytes(4, 10) - 1) == E
    assert draw(S=None, lists=fake + 8, lists_bytes=1 << 20) == E
    assert draw(N=1) == draw(H=256, W=257) == U
    assert lib.gnnpp_schedule_draw(None, fake, 4, fake, fake, fake, None, 0, fake, 1 << 20, None) == E


def test_host_side_of_the_pool():
    import inspect
    from gnn_pathplanning_amd import _native, expert
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        expert.SchedulePool('cpu')
    sig = inspect.signature
    assert list(sig(expert.SchedulePool.append).parameters) == ['self', 'grids', 'goals', 'schedules', 'commR', 'audit']
    assert list(sig(expert.SchedulePool.append_solutions).parameters) == ['self', 'solutions', 'grids', 'goals', 'commR',
                                                                         'audit']
    assert list(sig(expert.SchedulePool.draw).parameters) == ['self', 'batch_size', 'generator', 'graph']
    assert sig(expert.SchedulePool.draw).parameters['graph'].default == 'dense'
    assert list(sig(expert.SchedulePool.enqueue_draw).parameters) == ['self', 'index', 'out', 'graph']
    # the materialised pools are what they were
    assert list(sig(expert.SamplePool.draw).parameters) == ['self', 'batch_size', 'generator']
    assert list(sig(expert.SampleListPool.gather).parameters) == ['self', 'idx']
