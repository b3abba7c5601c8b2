"""CPU: the opt-in bf16x3 training precision off the device -- include/gnnpp_train_b3.h against its Python statement
(_native.TRAIN_B3_SIGNATURES); the layout of gnnpp_train_pack_b3 (csrc/train_encoder_b3.hip, compiled unmodified for the
host emulation) against a numpy restatement: the three planes of every fragment element sum to the fp32 weight EXACTLY and
padding elements are zero in every plane; the refusals of the new calls, which come before any HIP call; and the config
field `trainPrecision`: unknown values refused by name at construction, the default on the parent's path."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

import train_b3_cases as b3  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_host_logic import _abi_mismatches, _parse_header  # noqa: E402

needs_clang = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                 reason='host clang++ from ROCm not present')


def test_companion_header_matches_its_table():
    from gnn_pathplanning_amd import _native
    header = _parse_header(open(os.path.join(ROOT, 'include', 'gnnpp_train_b3.h')).read())
    protos, structs, defines = header
    assert list(protos) == list(_native.TRAIN_B3_SIGNATURES) == [
        'gnnpp_train_pack_b3_bytes', 'gnnpp_train_pack_b3', 'gnnpp_encoder_train_fwd_prec', 'gnnpp_encoder_train_bwd_prec']
    assert structs == {} and defines == {}
    assert _abi_mismatches(header, _native.TRAIN_B3_SIGNATURES, {}, {}) == []
    assert not set(_native.TRAIN_B3_SIGNATURES) & set(_native.EXPORTS)
    # the _prec calls are the existing pair's argument lists + (int precision, const void* pack_b3)
    for old in ('gnnpp_encoder_train_fwd', 'gnnpp_encoder_train_bwd'):
        assert _native.TRAIN_B3_SIGNATURES[old + '_prec'][1] == _native.SIGNATURES[old][1] + [ctypes.c_int, ctypes.c_void_p]
    # the comparison must see a changed kind, or it would prove nothing
    restype, argtypes = _native.TRAIN_B3_SIGNATURES['gnnpp_train_pack_b3']
    wrong = dict(_native.TRAIN_B3_SIGNATURES, gnnpp_train_pack_b3=(restype, [ctypes.c_int] + argtypes[1:]))
    found = _abi_mismatches(header, wrong, {}, {})
    assert len(found) == 1 and found[0].startswith('gnnpp_train_pack_b3:'), found
    # gnnpp.h is what it was
    assert len(_parse_header(open(os.path.join(ROOT, 'include', 'gnnpp.h')).read())[0]) == 59


def _weights(seed):
    """Convolution weights over fp32's exponent range: normal values, whole layers scaled by 2^-40 and 2^30, and single
    entries at the edges (the largest finite value, the smallest normal one, zero, values of one, two and three planes).
    fp32 subnormals are left out: below 2^-133, the smallest bf16 subnormal, no plane can carry them."""
    rng = np.random.default_rng(seed)
    ws = [rng.standard_normal((co, ci, 3, 3)).astype(np.float32) for ci, co, _ in b3.LAYERS]
    ws[0] *= np.float32(2.0 ** -40)
    ws[2] *= np.float32(2.0 ** 30)
    edges = np.array([3.4028235e38, -3.4028235e38, 1.1754944e-38, -1.1754944e-38, 0.0, 1.0, 1.00390625, 1.0000001, -1 / 3],
                     np.float32)
    ws[1].reshape(-1)[:edges.size] = edges
    ws[4].reshape(-1)[-edges.size:] = edges
    return ws


@needs_clang
def test_pack_layout_against_numpy():
    import emu_lib as el
    from gnn_pathplanning_amd._native import EncoderParams
    lib = el.load()
    ws = _weights(3)
    P = EncoderParams()
    for i in range(5):
        P.conv_w[i] = ws[i].ctypes.data
    offsets, total = b3.pack_offsets()
    assert lib.gnnpp_train_pack_b3_bytes() == total and total % 16 == 0
    assert offsets[(0, True)][1] == 0 and offsets[(0, False)][1] == 2 * 3072          # 27 of 32 slots in ONE k-step
    GUARD = 64
    buf = np.full(total + 2 * GUARD, 0xA5, np.uint8)
    base = buf.ctypes.data + GUARD
    assert base % 16 == 0
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P), ctypes.c_void_p(base), None) == 0
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + total:] == 0xA5).all()
    pack = buf[GUARD:GUARD + total]
    for l in range(5):
        for ig in (False, True):
            if l == 0 and ig:
                continue
            want, pad = b3.fragment_weights(ws[l], l, ig)
            planes, u16 = b3.planes_of(pack, l, ig)
            # h + m + l is the weight, exactly (the sum of three bf16 values of one fp32 is exact in float64)
            got = planes.sum(1)
            assert np.array_equal(got, want.astype(np.float64)), (l, ig, np.abs(got - want).max())
            assert not u16.transpose(0, 2, 3, 1)[pad].any(), (l, ig)               # padding: +0 in every plane
            g = b3.geom(l, ig)
            assert pad.sum() == ((g['M'] // 16) * 16 * 5 if l == 0 else 0), (l, ig)
            # planes in decreasing size: a residual is at most half a bf16 ulp of the plane above, 2^-8 of it -- a whole
            # ulp, 2^-7, where the first plane was clamped at the largest bf16
            h, m, lo = planes[:, 0], planes[:, 1], planes[:, 2]
            assert (np.abs(m) <= np.abs(h) * 2.0 ** -7).all() and (np.abs(lo) <= np.abs(m) * 2.0 ** -8).all()
    # a second call writes the same bytes
    buf2 = np.full(total + 2 * GUARD, 0x5A, np.uint8)
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P), ctypes.c_void_p(buf2.ctypes.data + GUARD), None) == 0
    assert np.array_equal(buf2[GUARD:GUARD + total], pack)


def _refusals(lib):
    """Every refusal of include/gnnpp_train_b3.h with pointers that are never dereferenced."""
    from gnn_pathplanning_amd import _native
    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    fake = ctypes.c_void_p(1 << 20).value
    P, G = _native.EncoderParams(), _native.EncoderGrads()
    for i in range(5):
        P.conv_w[i] = P.conv_b[i] = P.bn_w[i] = P.bn_b[i] = P.bn_mean[i] = P.bn_var[i] = fake
        G.conv_w[i] = G.conv_b[i] = G.bn_w[i] = G.bn_b[i] = fake
    cf = ctypes.c_float(0.1)

    def fwd(prec, pb, p=P, obs=fake, ws=fake, feat=fake, B=2, N=3, upd=0, tp=None):
        return lib.gnnpp_encoder_train_fwd_prec(ctypes.byref(p) if p else None, obs, ws, feat, B, N, cf, upd, None, 1, tp,
                                                None, prec, pb)

    def bwd(prec, pb, p=P, obs=fake, ws=fake, d=fake, g=G, B=2, N=3, tp=None):
        return lib.gnnpp_encoder_train_bwd_prec(ctypes.byref(p) if p else None, obs, ws, d, ctypes.byref(g) if g else None,
                                                B, N, 1, tp, None, prec, pb)
    for call in (fwd, bwd):
        for prec in (_native.PREC_SPLIT_F16, 3, -1, 100):
            assert call(prec, fake) == call(prec, None) == U, (call.__name__, prec)
        assert call(_native.PREC_FP32, None) == call(_native.PREC_FP32, fake + 8) == call(_native.PREC_FP32, fake + 4) == E
        for prec, pb in ((_native.PREC_FP32, fake), (_native.PREC_FP32_MFMA, None), (_native.PREC_FP32_MFMA, fake + 4)):
            assert call(prec, pb, p=None) == call(prec, pb, obs=None) == call(prec, pb, ws=None) == E
            assert call(prec, pb, B=0) == call(prec, pb, N=0) == call(prec, pb, tp=fake + 4) == E
    P2 = _native.EncoderParams()
    ctypes.memmove(ctypes.byref(P2), ctypes.byref(P), ctypes.sizeof(P))
    P2.bn_w[3] = None
    G2 = _native.EncoderGrads()
    ctypes.memmove(ctypes.byref(G2), ctypes.byref(G), ctypes.sizeof(G))
    G2.conv_b[1] = None
    for prec, pb in ((_native.PREC_FP32, fake), (_native.PREC_FP32_MFMA, None)):
        assert fwd(prec, pb, p=P2) == fwd(prec, pb, feat=None) == fwd(prec, pb, ws=fake + 4) == E
        assert bwd(prec, pb, p=P2) == bwd(prec, pb, d=None) == bwd(prec, pb, g=None) == bwd(prec, pb, g=G2) == E
    P3 = _native.EncoderParams()
    ctypes.memmove(ctypes.byref(P3), ctypes.byref(P), ctypes.sizeof(P))
    P3.bn_mean[2] = None
    assert fwd(_native.PREC_FP32, fake, p=P3, upd=1) == E
    # the pack call
    P4 = _native.EncoderParams()
    P4.conv_w[0] = P4.conv_w[1] = P4.conv_w[2] = P4.conv_w[3] = fake
    assert lib.gnnpp_train_pack_b3(None, fake, None) == lib.gnnpp_train_pack_b3(ctypes.byref(P), None, None) == E
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P), fake + 8, None) == lib.gnnpp_train_pack_b3(ctypes.byref(P4), fake, None) == E


def test_library_exports_the_calls_and_checks_arguments_first():
    from gnn_pathplanning_amd import _native
    if not os.path.exists('/opt/rocm/bin/hipcc') and not os.path.exists(_native.LIB_PATH):
        pytest.skip('hipcc not available and libgnnpp.so not prebuilt')
    _native.build()
    lib = _native.lib()
    assert lib.gnnpp_version() == 330                         # added without a version change
    assert lib.gnnpp_train_pack_b3_bytes() == b3.pack_offsets()[1]
    assert lib.gnnpp_encoder_train_workspace_floats(10, 64) > 0
    _refusals(lib)


@needs_clang
def test_emulated_library_refuses_the_same():
    import emu_lib as el
    _refusals(el.load())


class _Cfg:
    def __init__(self, **kw):
        self.num_agents, self.nGraphFilterTaps, self.device = 3, 3, 'cpu'
        for k, v in kw.items():
            setattr(self, k, v)


def test_train_precision_field_is_checked_at_construction():
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    assert DecentralPlannerNet(_Cfg()).trainPrecision == 'fp32'
    assert DecentralPlannerNet(_Cfg(trainPrecision=None)).trainPrecision == 'fp32'
    assert DecentralPlannerNet(_Cfg(trainPrecision='fp32')).trainPrecision == 'fp32'
    assert DecentralPlannerNet(_Cfg(trainPrecision='bf16x3')).trainPrecision == 'bf16x3'
    assert _native.TRAIN_PRECISIONS == {'fp32': _native.PREC_FP32_MFMA, 'bf16x3': _native.PREC_FP32}
    for bad in ('bf16', 'fp32_mfma', 'split_f16', 'BF16X3', '', 0, 1):
        with pytest.raises(_native.GnnppError) as err:
            DecentralPlannerNet(_Cfg(trainPrecision=bad))
        assert repr(bad) in str(err.value) and 'trainPrecision' in str(err.value) and "'bf16x3'" in str(err.value)


@pytest.mark.parametrize('field,want_pack', [(None, False), ('fp32', False), ('bf16x3', True)])
def test_train_precision_chooses_the_door(monkeypatch, field, want_pack):
    """The default (and 'fp32') hands the autograd function no b3 pack -- the parent's calls, and gnnpp_train_pack_b3 is never
    asked for; 'bf16x3' hands it the pack of the current weights.  (Host logic: the device calls are stubbed.)"""
    from gnn_pathplanning_amd import _native, decentralplanner as dp
    net = dp.DecentralPlannerNet(_Cfg(**({'trainPrecision': field} if field else {}))).train()
    seen, asked = {}, []
    monkeypatch.setattr(_native, 'require_gpu', lambda *a: None)
    monkeypatch.setattr(net, '_train_packs', lambda tensors: None)
    monkeypatch.setattr(net, '_train_pack_b3', lambda tensors: asked.append(len(tensors)) or 'PACK')
    monkeypatch.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('args', a) and 'FEAT')
    assert net._train_encoder(torch.zeros(2, 3, 3, 11, 11)) == 'FEAT'
    args = seen['args']
    assert len(args) == 7 + 20 and args[5] is None
    assert args[6] == ('PACK' if want_pack else None) and asked == ([20] if want_pack else [])
    net.eval()                                               # eval mode never reads the field
    assert not asked[1:]
