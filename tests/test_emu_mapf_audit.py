"""CPU: gnnpp_mapf_audit (csrc/mapf_audit_kernels.hip), compiled unmodified for the host emulation, against the sequential
restatement of tests/mapf_audit_cases.py: exact equality of every output element on every named case, on poisoned outputs
and a poisoned workspace, every call made twice with the same bytes; the documented error codes in the documented order
with nothing written.  Under the emulation the highest thread wins every race for an LDS word, on the device anybody
may: the crowd cases put the crowd where that winner is NOT the agent the outputs name.
tests/test_gpu_mapf_audit.py runs the same table on the device.  No case of the table is left out here
(mapf_audit_cases.EMU_LEFT_OUT is empty: the slowest, 1024 agents, takes about a second)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_audit_cases as ac  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def _ptr(a):
    return None if a is None else a.ctypes.data


def raw_call(lib, case, out, expect=0, dims=None, null=None, ws_short=0):
    """One call on host arrays.  dims: (C, N, H, W, T_max) the call is TOLD; null: the name of a pointer passed as NULL;
    ws_short: bytes the workspace is said to be short of."""
    C, T1, N, _ = case['schedule'].shape
    H, W = case['grid'].shape[-2:]
    tC, tN, tH, tW, tT = dims or (C, N, H, W, T1 - 1)
    need = lib.gnnpp_mapf_audit_workspace_bytes(C, N, T1 - 1)
    assert need > 0
    ws = np.full(need, 0x5a, np.uint8)
    ins = {'grid': case['grid'], 'start': case['start'], 'goal': case['goal'], 'schedule': case['schedule'],
           'steps': case['steps']}
    p = {k: None if k == null else _ptr(v) for k, v in list(ins.items()) + list(out.items()) + [('workspace', ws)]}
    rc = lib.gnnpp_mapf_audit(p['grid'], int(case['grid'].ndim == 3), p['start'], p['goal'], p['schedule'], p['steps'],
                              tC, tN, tH, tW, tT, *[p[k] for k in ac.OUTPUTS], p['workspace'], need - ws_short, None)
    assert rc == expect, rc
    return out


def call_of(lib):
    return lambda case, out: raw_call(lib, case, out)


def test_the_table_leaves_out_at_most_a_tenth():
    assert set(ac.EMU_LEFT_OUT) <= set(ac.CASES) and len(ac.EMU_LEFT_OUT) * 10 <= len(ac.CASES)
    assert sorted(set(ac.EMU_CASES) | set(ac.EMU_LEFT_OUT)) == sorted(ac.CASES)


@pytest.mark.parametrize('name', ac.EMU_CASES)
def test_named_cases_equal_the_restatement(lib, name):
    ac.run(call_of(lib), name)


def test_workspace_bytes():
    from gnn_pathplanning_amd import _native
    import emu_lib
    L = emu_lib.load()
    assert L.gnnpp_mapf_audit_workspace_bytes(1, 1, 0) > 0
    one, two = L.gnnpp_mapf_audit_workspace_bytes(3, 10, ac.CHUNK - 1), L.gnnpp_mapf_audit_workspace_bytes(3, 10, ac.CHUNK)
    assert two == 2 * one                                    # a chunk more per case
    for bad in ((0, 1, 0), (1, 0, 0), (1, _native.ROLLOUT_MAX_TEAM + 1, 0), (1, 1, -1),
                (1, 1, _native.MAPF_TEAM_MAX_STEPS + 1), (2 ** 31 - 1, 1, 64)):
        assert L.gnnpp_mapf_audit_workspace_bytes(*bad) == 0, bad


def test_argument_errors_in_their_order_leave_the_outputs_untouched(lib):
    case, _ = ac.wants_of('vertex_t4')
    C, T1, N, _ = case['schedule'].shape
    H, W = case['grid'].shape
    T = T1 - 1
    refused = [(dict(dims=(0, N, H, W, T)), ERR_ARG), (dict(dims=(C, 0, H, W, T)), ERR_ARG),
               (dict(dims=(C, 1025, H, W, T)), ERR_ARG), (dict(dims=(C, N, 0, W, T)), ERR_ARG),
               (dict(dims=(C, N, H, 0, T)), ERR_ARG), (dict(dims=(C, N, 257, W, T)), ERR_UNSUPPORTED),
               (dict(dims=(C, N, H, 257, T)), ERR_UNSUPPORTED), (dict(dims=(C, N, H, W, -1)), ERR_ARG),
               (dict(dims=(C, N, H, W, 2049)), ERR_ARG), (dict(ws_short=1), ERR_ARG),
               # the order: N before the sides, the sides before the horizon, the horizon before the pointers
               (dict(dims=(C, 1025, 257, W, T)), ERR_ARG), (dict(dims=(C, N, 257, W, 2049)), ERR_UNSUPPORTED),
               (dict(dims=(C, N, 257, W, T), null='goal'), ERR_UNSUPPORTED)]
    refused += [(dict(null=k), ERR_ARG) for k in ('grid', 'goal', 'schedule', 'workspace') + ac.OUTPUTS]
    for kw, code in refused:
        out = raw_call(lib, case, ac.poisoned(C, N), expect=code, **kw)
        for k in ac.OUTPUTS:
            assert (out[k] == ac.POISON).all(), (kw, k)      # nothing enqueued
    for null in ('start', 'steps'):                          # the two pointers that may be NULL
        out = raw_call(lib, case, ac.poisoned(C, N), null=null)
        assert out['counts'][0].tolist() == [0, 2, 0, 0]
