"""CPU: include/gnnpp_casegen.h, the companion header of the case generator, against its Python statement
(_native.CASEGEN_SIGNATURES and the CASEGEN_* constants), with the parser and the comparison that hold
_native.SIGNATURES to include/gnnpp.h (tests/test_host_logic.py); the built library exports the call, keeps its version
and checks the arguments before any HIP call; and the host side of gnn_pathplanning_amd.casegen."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_host_logic import _abi_mismatches, _parse_header


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_casegen.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.CASEGEN_SIGNATURES) == ['gnnpp_casegen']
    assert structs == {} and sorted(defines) == ['CASEGEN_OK', 'CASEGEN_TOO_SMALL']
    constants = {k: v for k, v in vars(_native).items() if isinstance(v, int)}
    assert _abi_mismatches(header, _native.CASEGEN_SIGNATURES, {}, constants) == []
    assert not set(_native.CASEGEN_SIGNATURES) & (set(_native.EXPORTS) | set(_native.MAPF_DISTANCE_SIGNATURES))
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.CASEGEN_SIGNATURES['gnnpp_casegen']
    wrong = {'gnnpp_casegen': (restype, argtypes[:2] + [ctypes.c_size_t] + argtypes[3:])}
    found = _abi_mismatches(header, wrong, {}, constants)
    assert len(found) == 1 and found[0].startswith('gnnpp_casegen:'), found
    from gnn_pathplanning_amd import casegen
    assert (casegen.OK, casegen.TOO_SMALL) == (defines['CASEGEN_OK'], defines['CASEGEN_TOO_SMALL'])


def test_library_exports_the_call_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    assert lib.gnnpp_casegen(None, 0, 0, 0, 1, 1, 4, 4, None, None, None, None, None, None) == _native.ERR_ARG


def test_threshold_and_host_side_argument_errors():
    from gnn_pathplanning_amd import _native, casegen
    assert casegen.threshold_of(0) == 0 and casegen.threshold_of(0.0) == 0
    assert casegen.threshold_of(1) == 2 ** 32 - 1 and casegen.threshold_of(0.5) == 2 ** 31
    assert casegen.threshold_of(0.1) == int(0.1 * 2 ** 32)
    for shape, text in (((1, 1025, 8, 8), 'N = 1025'), ((0, 4, 8, 8), 'C = 0'), ((1, 0, 8, 8), 'N = 0'),
                        ((2, 4, 257, 8), '257 x 8'), ((2, 4, 8, 0), '8 x 0')):
        with pytest.raises(_native.GnnppError, match=text):
            casegen.generate(*shape, 'cuda:0')
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        casegen.generate(2, 4, 8, 8, 'cpu')
