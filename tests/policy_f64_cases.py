"""The inference encoder and the policy forward against a float64 statement: the statements, the case matrix's
building blocks and the runner, shared by tests/test_gpu_policy_f64.py (libgnnpp.so on the MI355X) and
tests/test_emu_policy_f64.py (the same HIP sources on the host emulation of tests/emu/, a reduced matrix).  A plain
helper module, not a conftest.

A case is one call of the C ABI (gnnpp_encoder_fwd, or gnnpp_policy_fwd + gnnpp_decode_actions) under each precision
(GNNPP_PREC_FP32 = bf16x3, _FP32_MFMA, _SPLIT_F16), held to the float64 statement of the same network with the fp32
statement (torch, CPU) as the yardstick (f64_yardstick.gap).  Every case names the kernel instance it reaches: the
dispatch of gnnpp_api.hip / encoder_kernel_b3.hip is restated here (`encoder_kernel`, `policy_kernels`) from the knob
values the library reports, and the runner asserts what it can observe of the path: the fused one-launch kernel never
writes the feature workspace (the unfused path fills it), and the filter schedule of the unfused path is
gnnpp_filter_head_mode's answer.

Networks (`make_net`) start from the reference's initialisation and are then CALIBRATED in float64: layer by layer,
the BatchNorm gamma / beta (compressMLP: weight / bias) of the layer are divided by its largest activation on the
case's observations, so that every layer's largest activation is 1.  Activation scale s is then reached exactly by
scaling the observations, every conv / FC / filter / head bias, the running means and the BatchNorm betas by s (ReLU
networks are positively homogeneous; the running variances stay, so eps never swamps the normalised values).  Edges
applied before the calibration: BatchNorm (gamma < 0 and gamma = 0 channels, running means 1e3 above the spread,
running variances below / far above eps, large conv biases), weights over several decades, and one WEAK output
channel per layer at 1e-4 of the layer's largest weight whose running statistics and gamma are rescaled so that its
BatchNorm output is unchanged (small weights, large gamma / sigma).
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as tF

from f64_yardstick import MAX_K, ULP, ULPS, gap
from filter_f64_cases import Knobs
from gnn_pathplanning_amd import _native
from gnn_pathplanning_amd._native import TUNE_ENCODER_CP_TILE, TUNE_FUSED_POLICY, TUNE_POLICY_CP
from oracle import policy_oracle as orc

PRECS = (0, 1, 2)
PREC_NAMES = {0: 'fp32', 1: 'fp32mfma', 2: 'splitf16'}
EPS = orc.BN_EPS
CONV, BN = orc.CONV_KEYS, orc.BN_KEYS
CP_MAX = 12                                                       # kCpMaxAgents
# one residual pixel: 1 + 2^-8 (its m plane is 2^-8) and 1 + 2^-16 (a residual the size of the old 1e-5 bounds).  The
# round-to-nearest split of gnnpp_common.h b3_split2 puts any non-zero residual into the m plane first (no fp32 value
# has an l plane without an m plane), so both raise the tile's plane flag; dropping them costs 2^-8 / 2^-16 of the pixel
RESID = {'m': 1.0 + 2.0 ** -8, 'l': 1.0 + 2.0 ** -16}


# ---- the statements ------------------------------------------------------------------------------------------------
def encoder_layer(sd, t, li, dt):
    """Layer li of the eval-mode encoder in dtype dt: conv3x3 (pad 1) -> BatchNorm -> ReLU [-> max-pool 2]; li = 5:
    flatten -> compressMLP -> ReLU."""
    if li == 5:
        return tF.relu(tF.linear(t.reshape(t.shape[0], 128), sd['compressMLP.0.weight'].to(dt),
                                 sd['compressMLP.0.bias'].to(dt)))
    bn = 'ConvLayers.%d.' % BN[li]
    t = tF.conv2d(t, sd['ConvLayers.%d.weight' % CONV[li]].to(dt), sd['ConvLayers.%d.bias' % CONV[li]].to(dt),
                  padding=1)
    t = tF.relu(tF.batch_norm(t, sd[bn + 'running_mean'].to(dt), sd[bn + 'running_var'].to(dt),
                              sd[bn + 'weight'].to(dt), sd[bn + 'bias'].to(dt), training=False, eps=EPS))
    return tF.max_pool2d(t, 2) if orc.POOL_AFTER[li] else t


def encoder_statement(sd, obs, dt, acts=None):
    """Eval-mode ConvLayers + compressMLP + ReLU per agent in dtype dt (decentralplanner.py:284-290): obs [M,3,11,11]
    -> [M,128].  acts: a list that receives each layer's largest activation (5 conv layers, then the FC)."""
    t = obs.to(dt)
    for li in range(6):
        t = encoder_layer(sd, t, li, dt)
        if acts is not None:
            acts.append(float(t.abs().max()))
    return t


def filter_stack(h, S4, p, N, relu=None):
    """The L graph-filter layers with their ReLUs (decentralplanner.py:293-301): h [B,F,N] -> [B,F',N].  S4
    [B,E,Ns,Ns] in h's dtype (a GSO with more nodes than agents zero-pads the signal); p holds GFL.{2l}.weight
    [F',E,K,F] and .bias [F',1].  Also the training step's statement (tests/test_gpu_training_f64.py).
    relu(name, pre-activation), name = 'GFL.<2l>': the activation, for the tests that look at a layer's pre-activation
    or state a defect of its backward pass (tests/train_freeze_cases.py); None = ReLU."""
    B, Ns = h.shape[0], S4.shape[-1]
    l = 0
    while 'GFL.%d.weight' % (2 * l) in p:
        w, b = p['GFL.%d.weight' % (2 * l)], p.get('GFL.%d.bias' % (2 * l))
        z0 = torch.cat([h, h.new_zeros(B, h.shape[1], Ns - N)], 2) if Ns > N else h
        y = 0
        for e in range(w.shape[1]):
            z = z0
            for k in range(w.shape[2]):
                if k:
                    z = z @ S4[:, e]
                y = y + torch.einsum('fg,bgn->bfn', w[:, e, k], z)
        if b is not None:
            y = y + b
        h = tF.relu(y[:, :, :N]) if relu is None else relu('GFL.%d' % (2 * l), y[:, :, :N])
        l += 1
    return h


def policy_statement(sd, S, obs, dt):
    """(features [B*N,128], logits [N,B,5]) of the eval-mode policy in dtype dt.  obs [B,N,3,11,11]; S [B,E,Ns,Ns]
    as the kernel receives it, rounded to fp32 first (the kernels load an fp64 GSO as S.float(), graphML.py:2350)."""
    B, N = obs.shape[:2]
    feat = encoder_statement(sd, obs.reshape(B * N, 3, 11, 11), dt)
    p = {k: v.to(dt) for k, v in sd.items() if k.startswith('GFL.')}
    h = filter_stack(feat.reshape(B, N, 128).permute(0, 2, 1), S.float().to(dt), p, N)
    logits = torch.einsum('af,bfn->nba', sd['actionsMLP.0.weight'].to(dt), h) + sd['actionsMLP.0.bias'].to(dt)
    return feat, logits


# ---- inputs --------------------------------------------------------------------------------------------------------
def make_obs(seed, M, kind='binary'):
    """[M,3,11,11] fp32: 'binary' (10 % ones), 'bf16' (0.5, 3, -2: one bf16 plane), 'real' (signed, N(0,1))."""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(M, 3, 11, 11, generator=g) < (0.1 if kind == 'binary' else 0.3)).float()
    if kind == 'binary':
        return mask
    if kind == 'bf16':
        vals = torch.tensor([0.5, 3.0, -2.0])[torch.randint(0, 3, (M, 3, 11, 11), generator=g)]
        return mask * vals
    return torch.randn(M, 3, 11, 11, generator=g)


def with_residual(obs, agent, kind, last_pixel=False):
    """obs with ONE pixel of `agent` set to RESID[kind]: channel 0 at the centre, or the last pixel (channel 2,
    position 120).  Every other pixel of a binary tile stays one bf16 plane."""
    o = obs.clone()
    if last_pixel:
        o[agent, 2, 10, 10] = RESID[kind]
    else:
        o[agent, 0, 5, 5] = RESID[kind]
    return o


def make_gso(seed, B, E, N, Ns=None, f64=False):
    """[B,E,Ns,Ns] symmetric, degree-normalised, no self loops, geometric-graph-like density."""
    Ns = N if Ns is None else Ns
    g = np.random.default_rng(seed)
    A = (g.random((B, E, Ns, Ns)) < min(1.0, 4.0 / max(Ns, 1))).astype(np.float64)
    A = np.triu(A, 1)
    A = A + np.swapaxes(A, -1, -2)
    d = A.sum(-1)
    d[d == 0] = 1
    S = A / np.sqrt(d[..., :, None] * d[..., None, :])
    S = torch.from_numpy(S)
    return S if f64 else S.float()


SPREAD = (1e3, 1e-3, 1e2, 1e-2, 10.0, 0.1)                        # conv 0..4, FC: weights over six decades


def make_net(seed, obs, K=3, E=1, scale=1.0, bn_edge=None, spread=False, weak=False):
    """fp32 state_dict (torch CPU, one filter layer of K taps and E edge features) calibrated on obs [M,3,11,11] so that
    every layer's largest activation is `scale`.  bn_edge: 'gamma' | 'mean' | 'var' | 'bias'."""
    sd = orc.init_state_dict(K, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    if E != 1:
        sd['GFL.0.weight'] = (torch.rand(128, E, K, 128, generator=g) * 2 - 1) / math.sqrt(128 * K * E)
    sd['actionsMLP.0.bias'] = torch.randn(5, generator=g) * 0.1
    for li in range(5):
        w, cb = 'ConvLayers.%d.weight' % CONV[li], 'ConvLayers.%d.bias' % CONV[li]
        bn = 'ConvLayers.%d.' % BN[li]
        C = sd[cb].shape[0]
        v = sd[bn + 'running_var']
        if spread:
            sd[w] = sd[w] * SPREAD[li]
            sd[cb] = sd[cb] * SPREAD[li]
            sd[bn + 'running_mean'] = sd[bn + 'running_mean'] * SPREAD[li]
            sd[bn + 'running_var'] = v = v * SPREAD[li] ** 2
        if bn_edge == 'gamma':                                    # gamma < 0 on every 3rd channel, = 0 on every 7th
            neg = torch.arange(C) % 3 == 1
            sd[bn + 'weight'] = torch.where(neg, -sd[bn + 'weight'].abs(), sd[bn + 'weight'])
            sd[bn + 'bias'] = torch.where(neg, 0.5 * torch.ones(C), sd[bn + 'bias'])
            sd[bn + 'weight'][torch.arange(C) % 7 == 3] = 0.0
            sd[bn + 'bias'][torch.arange(C) % 7 == 3] = 0.25
        elif bn_edge == 'mean':                                   # mean 1e3 spreads off, beta re-centres the output
            sd[bn + 'running_mean'] = sd[bn + 'running_mean'] + 1e3 * v.sqrt()
            sd[bn + 'bias'] = sd[bn + 'bias'] + 1e3 * sd[bn + 'weight'] * v.sqrt() / (v + EPS).sqrt()
        elif bn_edge == 'var':                                    # var far below eps / far above 1, alternately
            sd[bn + 'running_var'] = torch.where(torch.arange(C) % 2 == 0, v * 1e-7, v * 1e6)
        elif bn_edge == 'bias':                                   # conv bias 1e3 spreads, running mean to match
            sd[cb] = sd[cb] + 1e3 * v.sqrt()
            sd[bn + 'running_mean'] = sd[bn + 'running_mean'] + 1e3 * v.sqrt()
        if weak:                                                  # channel li + 1 at 1e-4 of the largest weight
            c = li + 1
            f = 1e-4 * float(sd[w].abs().max()) / float(sd[w][c].abs().max())
            v0 = float(sd[bn + 'running_var'][c])
            sd[w][c] *= f
            sd[cb][c] *= f
            sd[bn + 'running_mean'][c] *= f
            sd[bn + 'running_var'][c] = v0 * f * f
            sd[bn + 'weight'][c] *= math.sqrt(v0 * f * f + EPS) / (f * math.sqrt(v0 + EPS))
    if spread:
        sd['compressMLP.0.weight'] = sd['compressMLP.0.weight'] * SPREAD[5]
    if weak:
        r = 6
        sd['compressMLP.0.weight'][r] *= 1e-4 * float(sd['compressMLP.0.weight'].abs().max()) / float(
            sd['compressMLP.0.weight'][r].abs().max())
        sd['compressMLP.0.bias'][r] *= 1e-4
    sd = {k: v.float().contiguous() if v.dtype.is_floating_point else v for k, v in sd.items()}
    # calibration (float64): layer by layer, divide gamma / beta (FC: weight / bias) by the layer's largest activation
    t = obs.double()
    with torch.no_grad():
        for li in range(6):
            c = float(encoder_layer(sd, t, li, torch.float64).abs().max())
            assert c > 0, ('dead layer', li)
            keys = ('ConvLayers.%d.weight' % BN[li], 'ConvLayers.%d.bias' % BN[li]) if li < 5 else \
                ('compressMLP.0.weight', 'compressMLP.0.bias')
            for k in keys:
                sd[k] = (sd[k].double() / c).float()
            t = encoder_layer(sd, t, li, torch.float64)
    return rescale(sd, scale)


def rescale(sd, scale):
    """The network whose every activation is `scale` x sd's on observations scaled by `scale`: every conv / FC /
    filter / head bias, running mean and BatchNorm beta times `scale` (the running variances stay)."""
    if scale == 1.0:
        return sd
    sd = dict(sd)
    for li in range(5):
        bn = 'ConvLayers.%d.' % BN[li]
        for k in ('ConvLayers.%d.bias' % CONV[li], bn + 'running_mean', bn + 'bias'):
            sd[k] = (sd[k].double() * scale).float()
    for k in [k for k in sd if k.endswith('.bias') and not k.startswith('ConvLayers')]:
        sd[k] = (sd[k].double() * scale).float()
    return sd


def check_scales(sd, obs, scale):
    """Assert in float64 that every layer's largest activation lands within 4x of `scale`; returns them."""
    acts = []
    encoder_statement(sd, obs.double(), torch.float64, acts)
    assert all(scale / 4 <= a <= scale * 4 for a in acts), (scale, acts)
    return acts


# ---- the dispatch, restated ----------------------------------------------------------------------------------------
def encoder_cp_tile(M, cp_knob, policy_cp):
    """encoder_kernel_b3.hip encoder_cp_tile: agents per column-packed tile, 0 = 16-agent tiles."""
    if 1 <= cp_knob <= CP_MAX:
        return cp_knob
    if cp_knob != 0 or policy_cp == 0:
        return 0
    t = (M + 255) // 256
    return t if t <= 8 else 0


def encoder_kernel(M, prec, cp_knob, policy_cp):
    """The instance gnnpp_encoder_fwd launches (encoder_pack.hip encoder_launch)."""
    if prec == 1:
        return 'encoder_kernel_f32'
    if prec == 2:
        return 'encoder_kernel_h2<false,3>'
    t = encoder_cp_tile(M, cp_knob, policy_cp)
    return 'encoder_kernel_b3<false,3,true>[tile%d]' % t if t else 'encoder_kernel_b3<false,3>'


def fused_policy_applies(B, N, K, E, prec, fused_knob):
    """gnnpp_api.hip fused_policy_applies (+ gnnpp_policy_fwd's E == 1)."""
    pays = B <= 512 or N >= 13 or fused_knob == 2
    return E == 1 and bool(fused_knob) and pays and prec != 1 and N <= 16 and 2 <= K <= 4


def policy_kernels(B, N, K, E, prec, knobs):
    """The instance(s) gnnpp_policy_fwd launches under `knobs` (the library's values of the three TUNE_* keys)."""
    if fused_policy_applies(B, N, K, E, prec, knobs[TUNE_FUSED_POLICY]):
        if prec == 0:
            return 'encoder_kernel_b3<true,%d,%s>' % (K, 'true' if N <= CP_MAX and knobs[TUNE_POLICY_CP] else 'false')
        return 'encoder_kernel_h2<true,%d>' % K
    return encoder_kernel(B * N, prec, knobs[TUNE_ENCODER_CP_TILE], knobs[TUNE_POLICY_CP]) + '+filter'


# ---- the runner ----------------------------------------------------------------------------------------------------
def _put_params(bk, sd):
    """(struct gnnpp_encoder_params on bk, the buffers it points to)."""
    p = _native.EncoderParams()
    keep = []
    for i in range(5):
        bn = 'ConvLayers.%d.' % BN[i]
        for field, key in (('conv_w', 'ConvLayers.%d.weight' % CONV[i]), ('conv_b', 'ConvLayers.%d.bias' % CONV[i]),
                           ('bn_w', bn + 'weight'), ('bn_b', bn + 'bias'), ('bn_mean', bn + 'running_mean'),
                           ('bn_var', bn + 'running_var')):
            b = bk.put(sd[key].numpy())
            keep.append(b)
            getattr(p, field)[i] = b.ptr.value
    for field, key in (('fc_w', 'compressMLP.0.weight'), ('fc_b', 'compressMLP.0.bias')):
        b = bk.put(sd[key].numpy())
        keep.append(b)
        setattr(p, field, b.ptr.value)
    p.bn_eps = EPS
    return p, keep


def pack_encoder(bk, sd):
    p, keep = _put_params(bk, sd)
    packed = bk.put(np.zeros(bk.lib.gnnpp_encoder_packed_floats(), np.float32))
    assert bk.lib.gnnpp_encoder_pack(ctypes.byref(p), packed.ptr, bk.stream) == 0
    bk.sync()
    packed._keep = (packed._keep, keep)
    return packed


def pack_filter(bk, h):
    F, E, K, G = h.shape
    hb = bk.put(np.ascontiguousarray(h, np.float32))
    packed = bk.put(np.zeros(bk.lib.gnnpp_filter_packed_floats(G, F, K, E), np.float32))
    assert bk.lib.gnnpp_filter_pack(hb.ptr, packed.ptr, G, F, K, E, bk.stream) == 0
    bk.sync()
    packed._keep = (packed._keep, hb)
    return packed


def knob_values(lib):
    return {k: lib.gnnpp_get_tuning(k) for k in (TUNE_FUSED_POLICY, TUNE_POLICY_CP, TUNE_ENCODER_CP_TILE)}


def allowed_error(rep):
    """The largest error gap() allows for a tensor with report `rep`."""
    return MAX_K * rep['max32'] + ULPS * ULP * rep['scale']


def check(name, got, want64, ref32):
    ok, rep = gap(got, want64, ref32)
    assert ok, '%s: %s' % (name, {k: '%.3g' % v for k, v in rep.items()})
    return rep


def run_encoder(bk, sd, obs, prec, knobs=None, expect=None, name=''):
    """gnnpp_encoder_fwd of obs [M,3,11,11]; returns (features [M,128] fp32 numpy, kernel name, range flag).
    expect: {prec: substring of the kernel name} asserted against the restated dispatch."""
    M = obs.shape[0]
    packed = pack_encoder(bk, sd)
    ob = bk.put(np.ascontiguousarray(obs.numpy(), np.float32))
    feat = bk.empty((M, 128))
    flag = bk.put(np.zeros(1, np.int32))
    with Knobs(bk.lib, knobs or {}):
        kv = knob_values(bk.lib)
        kern = encoder_kernel(M, prec, kv[TUNE_ENCODER_CP_TILE], kv[TUNE_POLICY_CP])
        if expect is not None and prec in expect:
            assert expect[prec] in kern, (name, prec, kern, expect[prec])
        assert bk.lib.gnnpp_encoder_fwd(ob.ptr, packed.ptr, feat.ptr, M, prec, flag.ptr, bk.stream) == 0
        bk.sync()
    return feat.get(), kern, int(flag.get()[0])


def run_policy(bk, sd, obs, S, K, prec, knobs=None, expect=None, name=''):
    """gnnpp_policy_fwd (+ gnnpp_decode_actions) of obs [B,N,3,11,11] on S [B,E,N,N] (fp32 or fp64); returns
    (logits [N,B,5], actions [B,N], features [B*N,128] or None when the fused kernel ran, kernel name, range flag)."""
    B, N = obs.shape[:2]
    E = S.shape[1]
    enc = pack_encoder(bk, sd)
    filt = pack_filter(bk, sd['GFL.0.weight'].numpy())
    ob = bk.put(np.ascontiguousarray(obs.numpy(), np.float32))
    s64 = int(S.dtype == torch.float64)
    Sb = bk.put(np.ascontiguousarray(S.numpy()))
    gb, aw, ab = (bk.put(np.ascontiguousarray(sd[k].numpy().reshape(-1), np.float32))
                  for k in ('GFL.0.bias', 'actionsMLP.0.weight', 'actionsMLP.0.bias'))
    ws = bk.empty((B * N, 128))
    logits = bk.empty((N, B, 5))
    acts = bk.put(np.full((B, N), -1, np.int32))
    flag = bk.put(np.zeros(1, np.int32))
    with Knobs(bk.lib, knobs or {}):
        kv = knob_values(bk.lib)
        kern = policy_kernels(B, N, K, E, prec, kv)
        if expect is not None and prec in expect:
            assert expect[prec] in kern, (name, prec, kern, expect[prec])
        fused = not kern.endswith('+filter')
        if not fused:
            mode = bk.lib.gnnpp_filter_head_mode(B, N, K, prec)
            kern += '[mode%d]' % mode
        rc = bk.lib.gnnpp_policy_fwd(ob.ptr, Sb.ptr, enc.ptr, filt.ptr, gb.ptr, aw.ptr, ab.ptr, ws.ptr, logits.ptr,
                                     B, N, K, E, s64, prec, flag.ptr, bk.stream)
        assert rc == 0, (name, rc)
        assert bk.lib.gnnpp_decode_actions(logits.ptr, acts.ptr, B, N, bk.stream) == 0
        bk.sync()
    feat = ws.get()
    # the observable half of the path: the fused kernel never writes the feature workspace, the encoder launch of
    # the unfused path writes all of it
    if fused:
        assert np.isnan(feat).all(), (name, prec, kern)
    else:
        assert np.isfinite(feat).all(), (name, prec, kern)
    return logits.get(), acts.get(), None if fused else feat, kern, int(flag.get()[0])


def check_actions(name, acts, want64, rep):
    """Decoded actions [B,N] equal the float64 arg-max on every row whose float64 top-2 margin exceeds twice the
    logit error the case allows.  Returns the number of rows checked."""
    w = np.asarray(want64, np.float64)                            # [N,B,5]
    top = np.sort(w, -1)
    sure = (top[..., -1] - top[..., -2]) > 2 * allowed_error(rep)
    want = w.argmax(-1).T                                         # [B,N]
    bad = sure.T & (acts != want)
    assert not bad.any(), '%s: %d decoded actions differ from the float64 arg-max' % (name, int(bad.sum()))
    return int(sure.sum())
