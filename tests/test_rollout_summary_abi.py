"""CPU: include/gnnpp_rollout_summary.h, the companion header of a rollout's summary, against its Python statement
(_native.ROLLOUT_SUMMARY_SIGNATURES, RolloutSummaryIn and the SUMMARY_* constants), with the parser and the comparison that
hold _native.SIGNATURES to include/gnnpp.h (tests/test_host_logic.py); the built library exports the calls, keeps its version
and answers every argument check before any HIP call; and the host side of metrics.summarise."""
import ctypes
import os
import types

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header

NAMES = ['gnnpp_rollout_summary_out_bytes', 'gnnpp_rollout_summary']
FIELDS = ['reached', 'stats', 'target_makespan', 'target_flowtime', 'valid', 'group', 'shielded', 'audit_ok', 'C', 'N', 'G',
          'target_stride']


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    text = open(os.path.join(ROOT, 'include', 'gnnpp_rollout_summary.h')).read()
    header = _parse_header(text)
    protos, structs, defines = header
    assert list(protos) == list(_native.ROLLOUT_SUMMARY_SIGNATURES) == NAMES
    assert list(structs) == ['gnnpp_rollout_summary_in'] and [f[0] for f in structs['gnnpp_rollout_summary_in']] == FIELDS
    assert len(defines) == 26 and all(k.startswith('SUMMARY_') for k in defines)
    fields = {'gnnpp_rollout_summary_in': _native.RolloutSummaryIn._fields_}
    constants = {k: v for k, v in vars(_native).items() if isinstance(v, int)}
    assert _abi_mismatches(header, _native.ROLLOUT_SUMMARY_SIGNATURES, fields, constants) == []
    # the words of the two records are numbered 0 .. 14 and 0 .. 7 without a gap
    ints = sorted(v for k, v in defines.items() if k not in ('SUMMARY_MAX_GROUPS', 'SUMMARY_I64', 'SUMMARY_F64'))
    assert ints == sorted(list(range(15)) + list(range(8)))
    others = (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) | set(_native.CASEGEN_SIGNATURES) |
              set(_native.MAPF_AUDIT_SIGNATURES) | set(_native.ROLLOUT_TRACE_SIGNATURES) |
              set(_native.SCHEDULE_DRAW_SIGNATURES) | set(_native.ROLLOUT_STREAM_SIGNATURES) |
              set(_native.CASEGEN_MAZE_SIGNATURES) | set(_native.ROLLOUT_STREAM_TRACE_SIGNATURES) |
              set(_native.ROLLOUT_TEAM_STREAM_SIGNATURES) | set(_native.TRAIN_B3_SIGNATURES) |
              set(_native.MEASURE_SIGNATURES))
    assert not set(_native.ROLLOUT_SUMMARY_SIGNATURES) & others
    # the comparison must see a changed kind, a changed field order and a changed constant, or it would prove nothing
    wrong = dict(_native.ROLLOUT_SUMMARY_SIGNATURES)
    wrong[NAMES[0]] = (ctypes.c_int, [ctypes.c_int, ctypes.c_int])                       # the size as an int
    found = _abi_mismatches(header, wrong, fields, constants)
    assert len(found) == 1 and found[0].startswith(NAMES[0] + ':'), found
    f = list(_native.RolloutSummaryIn._fields_)
    f[4], f[5] = f[5], f[4]                                                               # valid <-> group
    found = _abi_mismatches(header, _native.ROLLOUT_SUMMARY_SIGNATURES, {'gnnpp_rollout_summary_in': f}, constants)
    assert len(found) == 1 and found[0].startswith('struct gnnpp_rollout_summary_in:'), found
    assert _abi_mismatches(header, _native.ROLLOUT_SUMMARY_SIGNATURES, fields, dict(constants, SUMMARY_M2_DFT=6)) == \
        ['GNNPP_SUMMARY_M2_DFT: header 7, _native 6']
    # gnnpp.h is what it was
    main = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp.h')).read())
    assert len(main[0]) == 59 and list(main[0]) == list(_native.SIGNATURES)


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    size = lib.gnnpp_rollout_summary_out_bytes
    assert size(10, 1) == 16 * 8 + 8 * 8 + 11 * 4 and size(1, 64) == 64 * (192 + 8) and size(1024, 3) == 3 * (192 + 4100)
    assert size(0, 1) == size(-1, 1) == size(10, 0) == size(10, 65) == 0
    fake = 64                                                 # (never dereferenced: every call here is refused)
    PTRS = FIELDS[:8]

    def call(out=fake, **kw):
        s = _native.RolloutSummaryIn()
        for k in PTRS:
            setattr(s, k, fake)
        s.C, s.N, s.G, s.target_stride = 8, 10, 3, 1
        for k, v in kw.items():
            setattr(s, k, v)
        return lib.gnnpp_rollout_summary(ctypes.byref(s), out, None)

    E = _native.ERR_ARG
    assert lib.gnnpp_rollout_summary(None, fake, None) == E and call(out=None) == E
    for k in ('reached', 'stats', 'target_makespan', 'target_flowtime'):
        assert call(**{k: None}) == E, k
    assert call(C=0) == call(C=-1) == call(N=0) == call(N=-3) == call(G=0) == call(G=65) == call(G=-1) == E
    assert call(target_stride=0) == call(target_stride=-2) == E
    assert call(group=None) == call(group=None, G=2) == E     # no group ids: one group only
    assert call(C=2 ** 28, N=8) == call(C=2 ** 31 - 1, N=2) == call(C=46341, N=46341) == E       # C * N > 2^31 - 1
    assert call(out=fake + 4) == call(out=fake + 1) == E     # the record holds 64-bit words
    # every optional table missing is no error of its own: the refusals above came from what they name
    assert call(valid=None, shielded=None, audit_ok=None, C=0) == E


def test_host_side_of_summarise():
    """Refusals by name, before anything is enqueued: they are decided on shapes and devices, so stand-ins on the CPU reach
    every one of them."""
    import inspect
    import torch
    from gnn_pathplanning_amd import _native, metrics
    from gnn_pathplanning_amd.mapf import Distances, Solutions
    p = inspect.signature(metrics.summarise).parameters
    assert list(p) == ['run', 'targets', 'group', 'groups', 'audit']
    assert [p[k].default for k in ('group', 'groups', 'audit')] == [None, 1, None]
    for name in ('host', 'per_group', 'write_scalars', 'merge'):
        assert hasattr(metrics.Summary, name), name
    C, N = 4, 3
    i32 = torch.int32
    run = types.SimpleNamespace(reached=torch.zeros(C, N, dtype=i32), stats=torch.zeros(C, 2, dtype=i32))
    good = torch.ones(C, 2, dtype=i32)
    with pytest.raises(_native.GnnppError, match=r'no CPU fallback'):                   # a non-HIP device
        metrics.summarise(run, good)
    for bad in (torch.ones(C, 3, dtype=i32), torch.ones(C + 1, 2, dtype=i32), torch.ones(C, dtype=i32)):
        with pytest.raises(_native.GnnppError, match=r'targets must be an int32 \[C,2\] = \[4,2\]'):
            metrics.summarise(run, bad)
    with pytest.raises(_native.GnnppError, match='must hold integers'):
        metrics.summarise(run, torch.ones(C, 2))
    with pytest.raises(_native.GnnppError, match='Solutions or a mapf.Distances'):
        metrics.summarise(run, [[1, 2]] * C)
    z = lambda *s: torch.zeros(*s, dtype=i32)                                           # noqa: E731
    sol = Solutions(status=z(C + 1), makespan=z(C + 1), flowtime=z(C + 1), arrival=z(C + 1, N))
    with pytest.raises(_native.GnnppError, match=r'the Solutions are of C = 5 cases of N = 3 agents, the run of C = 4, N = 3'):
        metrics.summarise(run, sol)
    with pytest.raises(_native.GnnppError, match=r'the Distances are of C = 4 cases of N = 2 agents'):
        metrics.summarise(run, Distances(z(C, 2), z(C), z(C)))
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):                    # well-formed, on the CPU
        metrics.summarise(run, Distances(z(C, N), z(C), z(C)))
    with pytest.raises(_native.GnnppError, match='groups = 2 needs `group`'):
        metrics.summarise(run, good, groups=2)
    with pytest.raises(_native.GnnppError, match='1 <= groups <= 64'):
        metrics.summarise(run, good, group=z(C), groups=65)
    with pytest.raises(_native.GnnppError, match=r'group must be an int32 \[C\]'):
        metrics.summarise(run, good, group=z(C + 1), groups=2)
    with pytest.raises(_native.GnnppError, match=r'audit must be an int32 \[C\]'):
        metrics.summarise(run, good, audit=z(C, 2))
