"""CPU: include/gnnpp_rollout_stream_trace.h, the companion header of a streamed rollout's trace, against its Python
statement (_native.ROLLOUT_STREAM_TRACE_SIGNATURES and RolloutStreamTraceStruct), with the parser and the comparison that
hold _native.SIGNATURES to include/gnnpp.h (tests/test_host_logic.py); the built library exports the three calls, keeps its
version and answers every argument error before any HIP call (every pointer is poison: a launch would fault); the three
older headers are what they were; and the host side of RolloutStream(trace=...)."""
import ctypes
import hashlib
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header

FIELDS = ['path', 'action', 'moves', 'shielded', 'steps', 'seen_done', 'T_cap']
CALLS = ['gnnpp_rollout_stream_trace_begin', 'gnnpp_rollout_stream_trace_record',
         'gnnpp_rollout_stream_policy_steps_traced']
# the three headers byte for byte (sha256 of the files as the parent commit holds them)
HEADER_SHA256 = {
    'gnnpp.h': '5621be1f6c943b4d8b387729f721e9e444b1cea28e5fa01e6de9f2bd10303c3c',
    'gnnpp_rollout_trace.h': '7ffead93292e3136db01f5a3f7e7fa23a458c3f642335464c4004d2ccc50359b',
    'gnnpp_rollout_stream.h': 'a9e55ae1c4ef2d2e1704fcb1833c5f990f50064e5dd333f8324ac3fcb839afcc',
}


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(_header('gnnpp_rollout_stream_trace.h'))
    protos, structs, defines = header
    assert list(protos) == list(_native.ROLLOUT_STREAM_TRACE_SIGNATURES) == CALLS
    assert list(structs) == ['gnnpp_rollout_stream_trace'] and defines == {}
    assert [f[0] for f in structs['gnnpp_rollout_stream_trace']] == FIELDS
    fields = {'gnnpp_rollout_stream_trace': _native.RolloutStreamTraceStruct._fields_}
    assert _abi_mismatches(header, _native.ROLLOUT_STREAM_TRACE_SIGNATURES, fields, {}) == []
    others = (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES) | set(_native.CASEGEN_SIGNATURES) |
              set(_native.MAPF_AUDIT_SIGNATURES) | set(_native.ROLLOUT_TRACE_SIGNATURES) |
              set(_native.SCHEDULE_DRAW_SIGNATURES) | set(_native.ROLLOUT_STREAM_SIGNATURES) |
              set(_native.CASEGEN_MAZE_SIGNATURES))
    assert not set(_native.ROLLOUT_STREAM_TRACE_SIGNATURES) & others
    # the comparison must see a changed kind and a changed field order, or it would prove nothing
    restype, argtypes = _native.ROLLOUT_STREAM_TRACE_SIGNATURES['gnnpp_rollout_stream_policy_steps_traced']
    assert argtypes[6] is ctypes.c_int
    wrong = dict(_native.ROLLOUT_STREAM_TRACE_SIGNATURES,
                 gnnpp_rollout_stream_policy_steps_traced=(restype, argtypes[:6] + [ctypes.c_size_t] + argtypes[7:]))
    found = _abi_mismatches(header, wrong, fields, {})
    assert len(found) == 1 and found[0].startswith('gnnpp_rollout_stream_policy_steps_traced:'), found
    f = list(_native.RolloutStreamTraceStruct._fields_)
    f[4], f[5] = f[5], f[4]
    found = _abi_mismatches(header, _native.ROLLOUT_STREAM_TRACE_SIGNATURES, {'gnnpp_rollout_stream_trace': f}, {})
    assert len(found) == 1 and found[0].startswith('struct gnnpp_rollout_stream_trace:'), found


def test_the_older_headers_are_what_they_were():
    """gnnpp.h: 59 prototypes in the table's order, the rollout's struct without a new field; the fixed-batch trace's and
    the stream's companion headers: their prototypes, structs and field lists as their own tables state them."""
    from gnn_pathplanning_amd import _native
    main = _parse_header(_header('gnnpp.h'))
    assert len(main[0]) == 59 and list(main[0]) == list(_native.SIGNATURES)
    assert len(main[1]['gnnpp_rollout']) == len(_native.RolloutStruct._fields_)
    trace = _parse_header(_header('gnnpp_rollout_trace.h'))
    assert list(trace[0]) == list(_native.ROLLOUT_TRACE_SIGNATURES) and len(trace[0]) == 3
    assert _abi_mismatches(trace, _native.ROLLOUT_TRACE_SIGNATURES,
                           {'gnnpp_rollout_trace': _native.RolloutTraceStruct._fields_}, {}) == []
    stream = _parse_header(_header('gnnpp_rollout_stream.h'))
    assert list(stream[0]) == list(_native.ROLLOUT_STREAM_SIGNATURES) and len(stream[0]) == 2
    assert _abi_mismatches(stream, _native.ROLLOUT_STREAM_SIGNATURES,
                           {'gnnpp_rollout_stream': _native.RolloutStreamStruct._fields_}, {}) == []
    assert len(stream[1]['gnnpp_rollout_stream']) == 23 and len(trace[1]['gnnpp_rollout_trace']) == 7
    sums = {name: hashlib.sha256(_header(name).encode()).hexdigest() for name in HEADER_SHA256}
    assert sums == HEADER_SHA256


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    for name in CALLS:
        assert getattr(lib, name) is not None
    fake = 64                                                 # (never dereferenced: every call here is refused)
    R_PTRS = ('pos', 'done', 'maxstep')
    S_PTRS = ('slot_case', 'slot_t0', 'case_start')
    T_PTRS = ('path', 'steps', 'seen_done')

    def structs(**kw):
        r, s, tr = _native.RolloutStruct(), _native.RolloutStreamStruct(), _native.RolloutStreamTraceStruct()
        for f, _ in _native.RolloutStruct._fields_:           # every pointer of every struct is poison
            if f in ('grid', 'goal', 'pos', 'obs', 'radius', 'S', 'connected', 'logits', 'reached', 'start_step', 'end_step',
                     'maxstep', 'done', 'flags', 'stats', 'choice_count'):
                setattr(r, f, fake)
        for f, t in _native.RolloutStreamStruct._fields_:
            if t is ctypes.c_void_p:
                setattr(s, f, fake)
        for f in FIELDS[:-1]:
            setattr(tr, f, fake)
        r.B, r.N, r.H, r.W, r.grid_batched, r.tie_mode, r.currentstep = 3, 10, 20, 20, 1, 0, 5
        s.C, s.commR, s.case_grid_batched = 8, 6.0, 1
        tr.T_cap = 12
        for k, v in kw.items():
            obj = {'r_': r, 's_': s, 't_': tr}[k[:2]]
            setattr(obj, k[2:], v)
        return r, s, tr

    def begin(**kw):
        r, s, tr = structs(**kw)
        return lib.gnnpp_rollout_stream_trace_begin(ctypes.byref(r), ctypes.byref(s), ctypes.byref(tr), None)

    def record(**kw):
        r, s, tr = structs(**kw)
        return lib.gnnpp_rollout_stream_trace_record(ctypes.byref(r), ctypes.byref(s), ctypes.byref(tr), None)

    def burst(nsteps=2, **kw):
        r, s, tr = structs(**kw)
        return lib.gnnpp_rollout_stream_policy_steps_traced(ctypes.byref(r), fake, fake, fake, fake, fake, 3, nsteps, 0,
                                                            ctypes.byref(s), ctypes.byref(tr), None)

    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    r, s, tr = structs()
    R, S, T = ctypes.byref(r), ctypes.byref(s), ctypes.byref(tr)
    for fn in (lib.gnnpp_rollout_stream_trace_begin, lib.gnnpp_rollout_stream_trace_record):
        assert fn(None, S, T, None) == fn(R, None, T, None) == fn(R, S, None, None) == fn(None, None, None, None) == E
    f = lib.gnnpp_rollout_stream_policy_steps_traced
    assert f(None, fake, fake, fake, fake, fake, 3, 2, 0, S, T, None) == E
    assert f(R, fake, fake, fake, fake, fake, 3, 2, 0, None, T, None) == E
    assert f(R, fake, fake, fake, fake, fake, 3, 2, 0, S, None, None) == E
    for call in (begin, record, burst):
        for k in R_PTRS:
            assert call(**{'r_' + k: None}) == E, k
        for k in S_PTRS:
            assert call(**{'s_' + k: None}) == E, k
        for k in T_PTRS:
            assert call(**{'t_' + k: None}) == E, k
        assert call(r_B=0) == call(r_B=-1) == call(r_N=0) == call(s_C=0) == call(s_C=-2) == E
        assert call(r_B=2**30, r_N=4) == call(s_C=2**30, r_N=4) == E              # B * N, C * N beyond 2^31 - 1
        assert call(t_T_cap=0) == call(t_T_cap=-1) == E
        assert call(r_N=129) == U                                                   # where the reseat answers it
        assert call(r_tie_mode=_native.TIE_REPLAY) == call(r_tie_mode=_native.TIE_MT19937) == U
        assert call(r_N=129, r_pos=None) == call(r_tie_mode=_native.TIE_REPLAY, t_path=None) == E     # pointers first
        assert call(r_N=129, t_T_cap=0) == E                                        # ... and sizes
    for call in (record, burst):
        assert call(r_currentstep=0) == call(r_currentstep=-3) == E
        assert call(r_logits=None) == E                       # neither logits nor actions while action / shielded is wanted
        assert call(r_logits=None, t_shielded=None) == E and call(r_logits=None, t_action=None) == E
    assert burst(nsteps=0) == burst(nsteps=-1) == E
    assert burst(nsteps=0, r_N=129) == E
    # the traced burst checks the trace first, then answers what gnnpp_rollout_policy_steps answers: a team the one-launch
    # step does not take is refused by THAT call, still before anything is launched
    r, s, tr = structs(r_N=40)
    plain = lib.gnnpp_rollout_policy_steps(ctypes.byref(r), fake, fake, fake, fake, fake, 3, 2, 0, None)
    assert plain != 0 and burst(r_N=40) == plain


def test_host_side_of_the_traced_stream():
    import inspect
    import numpy as np
    from gnn_pathplanning_amd import _native, rollout
    p = inspect.signature(rollout.RolloutStream.__init__).parameters
    assert p['trace'].default is False and p['record'].default is False
    assert issubclass(rollout.StreamTrace, rollout.RolloutTrace)
    assert {'audit', 'schedule', 'prediction_yaml'} <= {k for c in rollout.StreamTrace.__mro__ for k in vars(c)}
    assert 'trace' not in inspect.signature(rollout.BatchedRollout.__init__).parameters    # the plain rollout is what it was
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        rollout.RolloutStream(np.zeros((4, 4), np.uint8), np.zeros((1, 2, 2), np.int64), np.ones((1, 2, 2), np.int64), 5,
                              'cpu', trace=True)
