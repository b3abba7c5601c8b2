"""The train-mode encoder's opt-in bf16x3 precision through its C entry points (include/gnnpp_train_b3.h: gnnpp_train_pack_b3,
gnnpp_encoder_train_fwd_prec / _bwd_prec; csrc/train_encoder_b3.hip): the runner and the numpy restatement of the pack,
shared by tests/test_gpu_train_b3_abi.py, tests/test_gpu_training_b3_f64.py (MI355X), tests/test_emu_training_b3.py and
tests/test_train_b3_pack.py (host emulation).  A plain helper module, not a conftest.

call_once is tests/train_encoder_abi_cases._call_once with the door chosen by `mode`:
  'old'     gnnpp_encoder_train_fwd / _bwd                       (the parent's calls)
  'fp32'    the _prec calls with GNNPP_PREC_FP32_MFMA, pack_b3 = NULL   (must be the parent's bytes)
  'bf16x3'  the _prec calls with GNNPP_PREC_FP32 and a pack_b3 that was filled with the poison before gnnpp_train_pack_b3
The workspace sits between two guards; workspace, guards and the pack buffers start as the poison value.
"""
import ctypes

import numpy as np

import train_encoder_abi_cases as ab
from gnn_pathplanning_amd._native import PREC_FP32, PREC_FP32_MFMA, EncoderGrads, EncoderParams

# (Cin, Cout, H) per layer and the geometry of conv_geom (csrc/train_encoder.hip), restated
LAYERS = ((3, 32, 11), (32, 32, 5), (32, 64, 5), (64, 64, 2), (64, 128, 2))


def geom(l, input_grad):
    """rows M, contraction length Ck, stages, k-steps of 32 per stage, channels per stage, rows per channel."""
    cin, cout, H = LAYERS[l]
    dense = H == 2
    rpc = 4 if dense else 1
    cc = 256 if dense else 32 if H == 5 else 4
    rows, ck = (cin, cout) if input_grad else (cout, cin)
    M, Ck = rows * rpc, ck * rpc
    sps = 1 if H == 11 else (1 if dense else 9) * cc // 32
    return dict(M=M, Ck=Ck, nchunk=-(-Ck // cc), SPS=sps, CC=cc, RPC=rpc, H=H)


def pack_offsets():
    """{(layer, input_grad): (byte offset, bytes)} of the b3 pack and its total size: per (row tile, stage, k-step) three
    planes of 64 lanes x 8 bf16; layer 0 has no input-gradient pack."""
    out, o = {}, 0
    for l in range(5):
        for ig in (False, True):
            g = geom(l, ig)
            n = 0 if (l == 0 and ig) else (g['M'] // 16) * g['nchunk'] * g['SPS'] * 3072
            out[(l, ig)] = (o, n)
            o += n
    return out, o


def fragment_weights(w, l, input_grad):
    """The fp32 value every element of the (l, input_grad) pack stands for, [block][lane 64][e 8], block = (row tile *
    stages + stage) * k-steps + k-step: A[m = 16 tile + lane % 16][k = 8 (lane // 16) + e]; and the mask of padding slots."""
    g = geom(l, input_grad)
    cin = LAYERS[l][0]
    nblk = (g['M'] // 16) * g['nchunk'] * g['SPS']
    val, pad = np.zeros((nblk, 64, 8), np.float32), np.ones((nblk, 64, 8), bool)
    for blk in range(nblk):
        s, ch, mt = blk % g['SPS'], (blk // g['SPS']) % g['nchunk'], blk // (g['SPS'] * g['nchunk'])
        for lane in range(64):
            m = mt * 16 + lane % 16
            for e in range(8):
                kk = 8 * (lane // 16) + e
                if g['H'] == 11:
                    tap, c = kk // 3, (kk % 3 if kk < 27 else g['Ck'])
                elif g['RPC'] == 1:
                    tap, c = s, ch * g['CC'] + kk
                else:
                    tap, c = 0, ch * g['CC'] + s * 32 + kk
                if c >= g['Ck']:
                    continue
                if g['RPC'] == 1:
                    co, ci, t = (c, m, 8 - tap) if input_grad else (m, c, tap)
                else:
                    row_ch, row_p, k_ch, k_p = m >> 2, m & 3, c >> 2, c & 3
                    co, ci = (k_ch, row_ch) if input_grad else (row_ch, k_ch)
                    po, pi = (k_p, row_p) if input_grad else (row_p, k_p)
                    t = ((pi >> 1) - (po >> 1) + 1) * 3 + ((pi & 1) - (po & 1) + 1)
                val[blk, lane, e] = w.reshape(-1)[(co * cin + ci) * 9 + t]
                pad[blk, lane, e] = False
    return val, pad


def planes_of(pack_bytes, l, input_grad):
    """The three bf16 planes of a pack region as float64 arrays [block][plane 3][lane 64][e 8]."""
    off, n = pack_offsets()[0][(l, input_grad)]
    u16 = np.frombuffer(pack_bytes[off:off + n].tobytes(), np.uint16).reshape(-1, 3, 64, 8)
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64), u16


def params(bk, sd):
    """(EncoderParams, the device copies by name) of a state dict."""
    keep, P = {}, EncoderParams()
    for k in ab.PARAM_KEYS + ab.RUNNING_KEYS:
        keep[k] = bk.put(sd[k].numpy().astype(np.float32))
    for field, fmt, idx in ab.FIELDS + (('bn_mean', 'ConvLayers.%d.running_mean', ab.BN),
                                        ('bn_var', 'ConvLayers.%d.running_var', ab.BN)):
        for i in range(5):
            getattr(P, field)[i] = keep[fmt % idx[i]].ptr.value
    P.bn_eps = ab.EPS
    return P, keep


def call_once(bk, N, B, sd, obs_np, cot_np, poison, mode, fsm=1, upd=1, ext=1):
    """One forward + backward on a workspace (and guards, and packs) filled with `poison`: every output as host arrays, the
    two guards' bits, the workspace's floats after the call."""
    lib = bk.lib
    P, keep = params(bk, sd)
    G = EncoderGrads()
    grads = {k: bk.empty(tuple(sd[k].shape)) for k in ab.PARAM_KEYS}
    for field, fmt, idx in ab.FIELDS:
        for i in range(5):
            getattr(G, field)[i] = grads[fmt % idx[i]].ptr.value
    nbt = [bk.put(np.full(1, ab.NBT0, np.int64)) for _ in range(5)]
    counters = (ctypes.c_void_p * 5)(*[c.ptr.value for c in nbt])
    total = lib.gnnpp_encoder_train_workspace_floats(N, B)
    assert total > 0 and total % 4 == 0
    buf = bk.put(np.full(ab.GUARD + total + ab.GUARD, poison, np.float32))
    ws = ctypes.c_void_p(buf.ptr.value + 4 * ab.GUARD)
    tp = None
    if ext:
        tp = bk.put(np.full(lib.gnnpp_train_pack_floats(), poison, np.float32))
        assert lib.gnnpp_train_pack(ctypes.byref(P), tp.ptr, None, None, None, 0, 0, 0, 0, bk.stream) == 0
    pb = None
    if mode == 'bf16x3':
        nbytes = lib.gnnpp_train_pack_b3_bytes()
        assert nbytes == pack_offsets()[1] and nbytes % 16 == 0
        pb = bk.put(np.full(nbytes // 4, poison, np.float32))
        assert pb.ptr.value % 16 == 0
        assert lib.gnnpp_train_pack_b3(ctypes.byref(P), pb.ptr, bk.stream) == 0
    obs_d, cot_d, feat = bk.put(obs_np), bk.put(cot_np), bk.empty((N * B, 128))
    fwd = (ctypes.byref(P), obs_d.ptr, ws, feat.ptr, B, N, ctypes.c_float(ab.MOMENTUM), upd, counters, fsm,
           tp.ptr if tp else None, bk.stream)
    bwd = (ctypes.byref(P), obs_d.ptr, ws, cot_d.ptr, ctypes.byref(G), B, N, fsm, tp.ptr if tp else None, bk.stream)
    if mode == 'old':
        rc = lib.gnnpp_encoder_train_fwd(*fwd)
        assert rc == 0, rc
        bk.sync()
        rc = lib.gnnpp_encoder_train_bwd(*bwd)
    else:
        extra = (PREC_FP32, pb.ptr) if mode == 'bf16x3' else (PREC_FP32_MFMA, None)
        rc = lib.gnnpp_encoder_train_fwd_prec(*fwd, *extra)
        assert rc == 0, rc
        bk.sync()
        rc = lib.gnnpp_encoder_train_bwd_prec(*bwd, *extra)
    assert rc == 0, rc
    bk.sync()
    f = feat.get()
    f = f.reshape(B, N, 128).transpose(1, 0, 2) if fsm else f.reshape(N, B, 128)
    out = dict(feat=np.ascontiguousarray(f), grads={k: grads[k].get() for k in ab.PARAM_KEYS},
               running={k: keep[k].get() for k in ab.RUNNING_KEYS},
               nbt={'ConvLayers.%d.num_batches_tracked' % ab.BN[i]: int(nbt[i].get()[0]) for i in range(5)})
    bits = buf.get().view(np.uint32)
    return out, bits[:ab.GUARD].copy(), bits[ab.GUARD + total:].copy(), bits[ab.GUARD:ab.GUARD + total].copy()


def run_poisoned(bk, N, B, seed, fsm=1, upd=1, ext=1):
    """The bf16x3 calls three times -- workspace, guards and both packs filled with 0.0, a NaN of a known payload, 3e38:
    guards intact, no NaN in any output, the three runs bit for bit the same (no element is read before it is written),
    and the NaN run against the float64 statement with train_encoder_abi_cases' yardstick.  -> the yardstick's ratios."""
    sd, obs, cot = ab.inputs(N, B, seed, N * B >= 100)
    obs_np = obs.numpy()
    cot_np = np.ascontiguousarray(cot.permute(1, 0, 2).numpy() if fsm else cot.numpy())
    runs = {}
    for name, poison in ab.POISONS:
        want_bits = np.array([poison], np.float32).view(np.uint32)[0]
        out, lo, hi, _ = call_once(bk, N, B, sd, obs_np, cot_np, poison, 'bf16x3', fsm, upd, ext)
        assert (lo == want_bits).all() and (hi == want_bits).all(), (name, 'wrote outside the workspace')
        for k, a in [('feat', out['feat'])] + list(out['grads'].items()) + list(out['running'].items()):
            assert not np.isnan(a).any(), (name, k)
        runs[name] = out
    for name in ('nan', '3e38'):
        assert ab._flat(runs['zero']) == ab._flat(runs[name]), name
    w64, w32 = ab.statements(N, B, seed, N * B >= 100)
    bad, ratios = ab.check_against_f64(runs['nan'], w64, w32, N, B, upd)
    print('train b3 ABI N%d B%d: %s' % (N, B, ' '.join('%s rms x%.2f max x%.2f' % (k, v[0], v[1])
                                                        for k, v in sorted(ratios.items()))))
    assert not bad, '\n'.join(str(b) for b in bad)
    return ratios
