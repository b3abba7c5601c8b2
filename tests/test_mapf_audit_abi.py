"""CPU: include/gnnpp_mapf_audit.h, the companion header of the schedule audit, against its Python statement
(_native.MAPF_AUDIT_SIGNATURES and the MAPF_AUDIT_* constants), with the parser and the comparison that hold
_native.SIGNATURES to include/gnnpp.h (tests/test_host_logic.py); the built library exports both calls, keeps its version
and checks the arguments before any HIP call; and the host side of gnn_pathplanning_amd.mapf.audit."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native, mapf
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_mapf_audit.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.MAPF_AUDIT_SIGNATURES) == ['gnnpp_mapf_audit_workspace_bytes', 'gnnpp_mapf_audit']
    assert structs == {}
    assert sorted(defines) == sorted('MAPF_AUDIT_' + k for k in (
        'CHUNK', 'CLASS_STATE', 'CLASS_VERTEX', 'CLASS_MOVE', 'CLASS_SWAP', 'STATE', 'VERTEX', 'MOVE', 'SWAP', 'BAD_START',
        'NOT_AT_GOAL', 'SKIPPED'))
    constants = {k: v for k, v in vars(_native).items() if isinstance(v, int)}
    assert _abi_mismatches(header, _native.MAPF_AUDIT_SIGNATURES, {}, constants) == []
    assert not set(_native.MAPF_AUDIT_SIGNATURES) & (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) |
                                                     set(_native.CASEGEN_SIGNATURES))
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.MAPF_AUDIT_SIGNATURES['gnnpp_mapf_audit']
    assert argtypes[18] is ctypes.c_size_t
    wrong = dict(_native.MAPF_AUDIT_SIGNATURES, gnnpp_mapf_audit=(restype, argtypes[:18] + [ctypes.c_int] + argtypes[19:]))
    found = _abi_mismatches(header, wrong, {}, constants)
    assert len(found) == 1 and found[0].startswith('gnnpp_mapf_audit:'), found
    # the class bit of the status is 1 << the class index of counts / first; the tests' table uses the same numbers
    for cls in ('STATE', 'VERTEX', 'MOVE', 'SWAP'):
        assert defines['MAPF_AUDIT_' + cls] == 1 << defines['MAPF_AUDIT_CLASS_' + cls]
    import mapf_audit_cases as ac
    assert ac.CHUNK == defines['MAPF_AUDIT_CHUNK'] == mapf.AUDIT_CHUNK
    assert (ac.STATE, ac.VERTEX, ac.MOVE, ac.SWAP, ac.BAD_START, ac.NOT_AT_GOAL, ac.SKIPPED) == tuple(
        defines['MAPF_AUDIT_' + k] for k in ('STATE', 'VERTEX', 'MOVE', 'SWAP', 'BAD_START', 'NOT_AT_GOAL', 'SKIPPED'))
    assert (mapf.AUDIT_BAD_START, mapf.AUDIT_NOT_AT_GOAL, mapf.AUDIT_SKIPPED) == (ac.BAD_START, ac.NOT_AT_GOAL, ac.SKIPPED)
    assert len(mapf.AUDIT_CLASSES) == 4


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    ws = lib.gnnpp_mapf_audit_workspace_bytes(2, 10, 64)
    assert ws == 2 * 3 * (8 + 10) * 4 and lib.gnnpp_mapf_audit_workspace_bytes(2, 1025, 64) == 0

    def call(C=2, N=10, H=8, W=8, T=64, nbytes=ws, fill=1):
        p = [ctypes.c_void_p(fill) if fill else None] * 13      # (never dereferenced: every call here is refused)
        return lib.gnnpp_mapf_audit(p[0], 0, p[1], p[2], p[3], p[4], C, N, H, W, T, *p[5:12], nbytes, None)
    assert call(fill=0) == _native.ERR_ARG                    # NULL pointers
    assert call(N=0) == call(N=1025) == call(C=0) == call(H=0) == call(W=0) == _native.ERR_ARG
    assert call(H=257) == call(W=257) == _native.ERR_UNSUPPORTED
    assert call(T=-1) == call(T=2049) == _native.ERR_ARG
    assert call(nbytes=ws - 1) == _native.ERR_ARG
    # the order: sizes, then the sides, then the horizon, then pointers and workspace
    assert call(N=1025, H=257) == _native.ERR_ARG and call(H=257, T=2049) == _native.ERR_UNSUPPORTED
    assert call(H=257, fill=0) == _native.ERR_UNSUPPORTED and call(T=2049, fill=0) == _native.ERR_ARG


def test_host_side_argument_errors():
    from gnn_pathplanning_amd import _native, mapf
    grid = np.zeros((8, 8), np.uint8)
    goal = np.zeros((2, 3, 2), np.int64)
    sched = np.zeros((2, 5, 3, 2), np.int64)
    for kw, text in ((dict(device='cpu'), 'no CPU fallback'),
                     (dict(schedules=sched[:, :, :2]), r'schedules must be \[C,T\+1,N,2\]'),
                     (dict(schedules=sched[0]), 'schedules must be'),
                     (dict(schedules=[sched[0], sched[1, :, :2]]), 'schedule 1 must be'),
                     (dict(schedules=[]), 'empty list'),
                     (dict(schedules=[sched[0], sched[1]], steps=[4, 4]), 'steps come from the lengths'),
                     (dict(steps=[1, 2, 3]), r'steps must be \[C\] = \[2\]'),
                     (dict(starts=np.zeros((2, 4, 2), np.int64)), 'starts and goals must both be'),
                     (dict(grids=np.zeros((3, 8, 8), np.uint8)), 'grids must be'),
                     (dict(grids=np.zeros((257, 8), np.uint8)), '257 x 8'),
                     (dict(schedules=np.zeros((2, 2050, 3, 2), np.int32)), 'at most 2048 steps'),
                     (dict(schedules=np.zeros((1, 2, 1025, 2), np.int32), goals=np.zeros((1, 1025, 2), np.int32)),
                      'teams of 1 to 1024')):
        args = dict(grids=grid, starts=None, goals=goal, schedules=sched, device='cuda:0', steps=None)
        args.update(kw)
        with pytest.raises(_native.GnnppError, match=text):
            mapf.audit(**args)
