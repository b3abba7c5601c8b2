"""CPU: include/gnnpp_mapf_distance.h, the companion header of the MAPF solver's goal distances and planning orders,
against its Python statement (_native.MAPF_DISTANCE_SIGNATURES and the MAPF_DIST_* / MAPF_ORDER_* constants), with the
parser and the comparison that hold _native.SIGNATURES to include/gnnpp.h (tests/test_host_logic.py); and the built
library exports both calls and checks their arguments before any HIP call."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_mapf_distance.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.MAPF_DISTANCE_SIGNATURES) == ['gnnpp_mapf_distances', 'gnnpp_mapf_orders']
    assert structs == {} and len(defines) == 6
    constants = {k: v for k, v in vars(_native).items() if isinstance(v, int)}
    assert _abi_mismatches(header, _native.MAPF_DISTANCE_SIGNATURES, {}, constants) == []
    assert not set(_native.MAPF_DISTANCE_SIGNATURES) & set(_native.EXPORTS)
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.MAPF_DISTANCE_SIGNATURES['gnnpp_mapf_orders']
    wrong = dict(_native.MAPF_DISTANCE_SIGNATURES, gnnpp_mapf_orders=(restype, argtypes[:1] + [ctypes.c_size_t] + argtypes[2:]))
    found = _abi_mismatches(header, wrong, {}, constants)
    assert len(found) == 1 and found[0].startswith('gnnpp_mapf_orders:'), found
    # the rule names of mapf.py are the header's
    from gnn_pathplanning_amd import mapf
    assert mapf.ORDER_RULES == {'index': defines['MAPF_ORDER_INDEX'], 'longest_first': defines['MAPF_ORDER_LONGEST_FIRST'],
                                'shortest_first': defines['MAPF_ORDER_SHORTEST_FIRST'], 'hashed': defines['MAPF_ORDER_HASHED']}
    assert (mapf.UNREACHABLE, mapf.INVALID) == (defines['MAPF_DIST_UNREACHABLE'], defines['MAPF_DIST_INVALID'])


def test_library_exports_both_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    assert lib.gnnpp_mapf_distances(None, 0, None, None, 1, 1, 4, 4, None, None, None, None) == _native.ERR_ARG
    assert lib.gnnpp_mapf_orders(None, 1, 4, 1, None, 0, None, None) == _native.ERR_ARG
