"""GPU (-m gpu): the entry points of include/gnnpp_train_b3.h on the MI355X, in the manner of
tests/train_encoder_abi_cases.py (runner: tests/train_b3_cases.py).

  poisons    gnnpp_train_pack_b3 + gnnpp_encoder_train_fwd_prec / _bwd_prec under GNNPP_PREC_FP32 on a workspace between
             guards, with workspace, guards, the fp32 pack and the b3 pack filled with 0.0, a NaN of a known payload and
             3e38 before the calls: guards intact, no NaN in any output, the three runs bit for bit the same -- no element of
             the workspace or of a pack is read before it is written -- and the NaN run against float64 with the unchanged
             yardstick; at (N, B) = (1, 1), (2, 3), (3, 7) and (2, 33): every image chunk partial, ragged chunks of the 2-, 4-
             and 32-image geometries, both feature layouts, train_pack NULL and the caller's, update_running 0 and 1;
  refusals   every refusal of the header returns its code with real device buffers, and leaves the outputs, the workspace
             and the running statistics as they were (nothing is enqueued)."""
import ctypes

import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import train_b3_cases as b3
import train_encoder_abi_cases as ab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


@pytest.mark.parametrize('N,B,fsm,upd,ext', [(1, 1, 1, 1, 1), (2, 3, 0, 1, 0), (3, 7, 1, 0, 1), (2, 33, 0, 1, 1)])
def test_b3_entry_points_on_poisoned_buffers(bk, N, B, fsm, upd, ext):
    b3.run_poisoned(bk, N, B, seed=5000 + 100 * N + B, fsm=fsm, upd=upd, ext=ext)


def test_refusals_leave_everything_unchanged(bk):
    from gnn_pathplanning_amd import _native
    lib = bk.lib
    E, U = _native.ERR_ARG, _native.ERR_UNSUPPORTED
    N, B = 2, 3
    sd, obs, cot = ab.inputs(N, B, 5203, False)
    P, keep = b3.params(bk, sd)
    G = _native.EncoderGrads()
    mark = np.float32(-1234.5)
    grads = {k: bk.put(np.full(tuple(sd[k].shape), mark, np.float32)) for k in ab.PARAM_KEYS}
    for field, fmt, idx in ab.FIELDS:
        for i in range(5):
            getattr(G, field)[i] = grads[fmt % idx[i]].ptr.value
    total = lib.gnnpp_encoder_train_workspace_floats(N, B)
    ws = bk.put(np.full(total, mark, np.float32))
    feat = bk.put(np.full((N * B, 128), mark, np.float32))
    pb = bk.put(np.full(lib.gnnpp_train_pack_b3_bytes() // 4, mark, np.float32))
    obs_d, cot_d = bk.put(obs.numpy()), bk.put(cot.numpy())
    nbt = [bk.put(np.full(1, ab.NBT0, np.int64)) for _ in range(5)]
    counters = (ctypes.c_void_p * 5)(*[c.ptr.value for c in nbt])
    cf = ctypes.c_float(ab.MOMENTUM)
    off = lambda buf, n: ctypes.c_void_p(buf.ptr.value + n)                         # noqa: E731

    def fwd(prec, pack, p=P, o=obs_d.ptr, w=ws.ptr, f=feat.ptr, b=B, n=N, tp=None):
        return lib.gnnpp_encoder_train_fwd_prec(ctypes.byref(p) if p else None, o, w, f, b, n, cf, 1, counters, 0, tp,
                                                bk.stream, prec, pack)

    def bwd(prec, pack, p=P, o=obs_d.ptr, w=ws.ptr, d=cot_d.ptr, g=G, b=B, n=N, tp=None):
        return lib.gnnpp_encoder_train_bwd_prec(ctypes.byref(p) if p else None, o, w, d, ctypes.byref(g) if g else None,
                                                b, n, 0, tp, bk.stream, prec, pack)
    P2 = _native.EncoderParams()
    ctypes.memmove(ctypes.byref(P2), ctypes.byref(P), ctypes.sizeof(P))
    P2.conv_w[2] = None
    G2 = _native.EncoderGrads()
    ctypes.memmove(ctypes.byref(G2), ctypes.byref(G), ctypes.sizeof(G))
    G2.bn_w[4] = None
    F32, MF = _native.PREC_FP32, _native.PREC_FP32_MFMA
    for call in (fwd, bwd):
        for prec in (_native.PREC_SPLIT_F16, 3, -1):
            assert call(prec, pb.ptr) == call(prec, None) == U, (call.__name__, prec)
        assert call(F32, None) == call(F32, off(pb, 4)) == call(F32, off(pb, 8)) == E, call.__name__
        for prec, pack in ((F32, pb.ptr), (MF, None)):
            assert call(prec, pack, p=None) == call(prec, pack, p=P2) == call(prec, pack, o=None) == E
            assert call(prec, pack, w=None) == call(prec, pack, b=0) == call(prec, pack, n=-1) == E
            assert call(prec, pack, tp=off(pb, 4)) == E
    for prec, pack in ((F32, pb.ptr), (MF, None)):
        assert fwd(prec, pack, f=None) == fwd(prec, pack, w=off(ws, 4)) == E
        assert bwd(prec, pack, d=None) == bwd(prec, pack, g=None) == bwd(prec, pack, g=G2) == E
    assert lib.gnnpp_train_pack_b3(None, pb.ptr, bk.stream) == lib.gnnpp_train_pack_b3(ctypes.byref(P), None, bk.stream) == E
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P), off(pb, 8), bk.stream) == E
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P2), pb.ptr, bk.stream) == E
    bk.sync()
    # nothing was enqueued: every buffer a call could have written holds what it held
    for buf in [ws, feat, pb] + list(grads.values()):
        assert (buf.get() == mark).all()
    for k in ab.RUNNING_KEYS + ab.PARAM_KEYS:
        assert np.array_equal(keep[k].get(), sd[k].numpy()), k
    assert all(int(c.get()[0]) == ab.NBT0 for c in nbt)
    # and the accepted calls on the very same buffers do run
    assert lib.gnnpp_train_pack_b3(ctypes.byref(P), pb.ptr, bk.stream) == 0
    assert fwd(F32, pb.ptr) == 0 and bwd(F32, pb.ptr) == 0
    bk.sync()
    assert not (feat.get() == mark).any() and np.isfinite(feat.get()).all()
    assert all(int(c.get()[0]) == ab.NBT0 + N for c in nbt)
