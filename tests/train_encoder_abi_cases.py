"""The train-mode encoder through its C entry points (gnnpp_encoder_train_workspace_floats / _train_fwd / _train_bwd,
gnnpp_train_pack; csrc/train_encoder.hip) on POISONED workspaces: case matrix, float64 statement and runner, shared by
tests/test_emu_train_encoder_abi.py (host emulation, a reduced matrix) and tests/test_gpu_train_encoder_abi.py (MI355X).
A plain helper module, not a conftest.

What a case holds the kernels to (run_case):

  guards    the workspace is the middle of ONE buffer of GUARD + total + GUARD floats (total = the library's answer for
            (N, B) under the case's knobs); buffer and guards are filled with a poison value, and after forward + backward
            both guards hold the poison bit for bit: no kernel writes outside what the size query promised;
  poisons   the case runs three times, with the workspace filled with 0.0, with a NaN of a known payload and with 3e38
            (finite: 0 * x stays 0 while x + y overflows).  The kernels' reduction orders are fixed, so the three runs
            must agree BIT FOR BIT in feat, all 20 gradients, the running statistics and the counters, and no output may
            hold a NaN: a kernel that reads workspace nobody wrote (a ragged image tile, the shared `part` buffer, the
            dxa / dxb ping-pong, a weight-gradient slab) multiplies it by a zero weight or drops it into a padded MFMA
            column -- right with zero or recycled memory, wrong with NaN.  The forward poisons the WHOLE workspace, so
            whatever it did not write is still poison when the backward runs: no knowledge of the layout is used;
  accuracy  the NaN run against the float64 statement below, with the statement in fp32 on the CPU as the yardstick
            (f64_yardstick.gap, RMS_K / MAX_K / ULPS unchanged).  A conv bias in front of train-mode BatchNorm has an
            exactly-zero gradient: the ulps are taken of the roundoff a sum of B x P terms of the layer's weight-gradient
            size makes, as in tests/test_gpu_training_f64.py.

A case is (N, B, feat_sample_major, ext_pack, update_running, wgs, running_fused):
  feat_sample_major   0: feat / dfeat are [N][B][128] (the C default, which the Python door never passes), 1: [B][N][128]
  ext_pack            0: train_pack = NULL (packs built in the workspace), 1: the caller's gnnpp_train_pack buffer
  update_running      1: running statistics and the five counters advance (N sequential updates, += N); 0: they are handed
                      over all the same and must keep their bits (the 0.0-poison run passes NULL counters)
  wgs, running_fused  GNNPP_TUNE_TRAIN_WGRAD_WGS (17), GNNPP_TUNE_TRAIN_RUNNING_FUSED (19); restored in a `finally`

Shapes (N, B): (1, 1) every split count clamps to N*B; (1, 2) the smallest ragged case; (2, 3), (3, 7) ragged image tiles
and N != B (a swapped feature layout cannot pass); (10, 13) N*B = 130: under the default 128 workgroups the 32-channel
layers get 64 splits -> 3 images per split -> 44 splits used, the last holding ONE image (ips * nsplit = 132 > 130);
(7, 1) one image per agent: BatchNorm over 121, 25 and 4 positions.  The 24 (shape, wgs) pairs, wgs in {0, 16, 100
(no multiple of any channel-tile count), 2048 (clamps)}, carry the four two-valued settings so that EVERY PAIR OF VALUES OF
ANY TWO of the six factors (shape, wgs, running_fused, feat_sample_major, ext_pack, update_running) occurs in some case
(_pairwise_cover asserts it at import); the full product (384) is not taken.  (10, 13) runs with the BatchNorm shifts + 3
(ReLU inputs away from zero, as make_case of test_gpu_training_f64.py does for its larger batches: a ReLU input within
roundoff of zero lets a correct fp32 kernel route one gradient entry differently from float64, and the chance of one
such value grows with the number of activations -- 9e5 here); the other shapes run in the plain regime.

GUARD_ONLY: (10, 129), 1 290 images -- the first batch on the 256-workgroup side of the 1 280-image switch -- under wgs = 0
and 2048: guards and the three poisons only, no float64 statement.
"""
import ctypes
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as tF

from f64_yardstick import MAX_K, ULP, ULPS, gap
from filter_f64_cases import Knobs
from gnn_pathplanning_amd._native import (TUNE_TRAIN_RUNNING_FUSED, TUNE_TRAIN_WGRAD_WGS, EncoderGrads, EncoderParams)
from oracle import policy_oracle as orc

CONV = (0, 4, 7, 11, 14)
BN = (1, 5, 8, 12, 15)
CHANNELS = ((3, 32), (32, 32), (32, 64), (64, 64), (64, 128))
POS = (121, 25, 25, 4, 4)                     # positions per image at each convolution's output
EPS, MOMENTUM = 1e-5, 0.1
GUARD = 4096                                  # floats on either side of the workspace (a multiple of 4: 16-byte alignment)
NAN_BITS = 0x7FC5A5A5                         # a quiet NaN with a payload no arithmetic produces
POISONS = (('zero', np.float32(0.0)), ('nan', np.array([NAN_BITS], np.uint32).view(np.float32)[0]),
           ('3e38', np.float32(3e38)))
NBT0 = 7                                      # num_batches_tracked before the call

PARAM_KEYS = [k for i in range(5) for k in ('ConvLayers.%d.weight' % CONV[i], 'ConvLayers.%d.bias' % CONV[i],
                                            'ConvLayers.%d.weight' % BN[i], 'ConvLayers.%d.bias' % BN[i])]
RUNNING_KEYS = [k for i in range(5) for k in ('ConvLayers.%d.running_mean' % BN[i], 'ConvLayers.%d.running_var' % BN[i])]
FIELDS = (('conv_w', 'ConvLayers.%d.weight', CONV), ('conv_b', 'ConvLayers.%d.bias', CONV),
          ('bn_w', 'ConvLayers.%d.weight', BN), ('bn_b', 'ConvLayers.%d.bias', BN))

SHAPES = ((1, 1), (1, 2), (2, 3), (3, 7), (10, 13), (7, 1))
WGS = (0, 16, 100, 2048)
FACTORS = ('shape', 'wgs', 'fused', 'fsm', 'ext', 'upd')


def _case(N, B, fsm, ext, upd, wgs, fused, statement=True):
    return dict(name='N%d-B%d-fsm%d-ext%d-upd%d-wgs%d-fused%d' % (N, B, fsm, ext, upd, wgs, fused), N=N, B=B, shape=(N, B),
                fsm=fsm, ext=ext, upd=upd, wgs=wgs, fused=fused, statement=statement, margin=N * B >= 100,
                seed=1000 * N + B)


def _matrix():
    out = []
    for i, (N, B) in enumerate(SHAPES):
        for j, wgs in enumerate(WGS):
            i0, i1, i2, j0, j1 = i & 1, (i >> 1) & 1, (i >> 2) & 1, j & 1, (j >> 1) & 1
            out.append(_case(N, B, fsm=j1 ^ i1, ext=j0 ^ j1 ^ i2, upd=j0 ^ i1 ^ i2, wgs=wgs, fused=j0 ^ i0))
    return out


def _pairwise_cover(cases):
    """Every pair of values of any two of the six factors occurs in some case."""
    values = {f: sorted({c[f] for c in cases}) for f in FACTORS}
    assert values['shape'] == sorted(SHAPES) and values['wgs'] == sorted(WGS)
    assert all(values[f] == [0, 1] for f in FACTORS[2:])
    for f, g in itertools.combinations(FACTORS, 2):
        seen = {(c[f], c[g]) for c in cases}
        missing = [(a, b) for a in values[f] for b in values[g] if (a, b) not in seen]
        assert not missing, (f, g, missing)


CASES = _matrix()
_pairwise_cover(CASES)
assert all(c['N'] * c['B'] <= 150 for c in CASES)
GUARD_ONLY = [_case(10, 129, fsm=0, ext=0, upd=1, wgs=0, fused=1, statement=False),
              _case(10, 129, fsm=1, ext=1, upd=1, wgs=2048, fused=0, statement=False)]
# the host emulation's share: the smallest, a ragged and the ragged-last-split shape under 0 and 16 workgroups, and the
# other two small shapes under the knob value that is no multiple of a tile count
EMU_CASES = [c for c in CASES if (c['shape'] in ((1, 1), (3, 7), (10, 13)) and c['wgs'] in (0, 16))
             or (c['shape'] in ((1, 2), (2, 3)) and c['wgs'] == 100)]
assert {(c['shape'], c['wgs']) for c in EMU_CASES} >= {(s, w) for s in ((1, 1), (3, 7), (10, 13)) for w in (0, 16)}
for _f in FACTORS[2:]:
    assert {c[_f] for c in EMU_CASES} == {0, 1}, _f


def case_id(c):
    return c['name']


def split_plan(N, B, wgs, cout):
    """(images per split, image splits) of a layer's weight gradient, as train_ws_layout has them."""
    NB = N * B
    w = wgs if wgs > 0 else 128 if NB <= 1280 else 256
    ns = min(-(-w // (cout // 16)), NB)
    ips = -(-NB // ns)
    return ips, -(-NB // ips)


assert split_plan(10, 13, 0, 32) == (3, 44) and 3 * 44 > 130          # the ragged last split the shape is there for
assert split_plan(10, 129, 0, 32)[1] > split_plan(10, 128, 0, 32)[1]  # the 256-workgroup side of the switch
assert all(split_plan(N, B, 2048, 128) == (1, N * B) for N, B in SHAPES)


# ---- inputs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N, B, seed, margin, near_ties=True):
    """Parameters (the oracle's init + non-trivial BatchNorm scale, shift and running state), binary observations without
    max-pool near-ties (test_gpu_training_f64.without_pool_near_ties) and the cotangent on feat, [N,B,128]."""
    sd = orc.init_state_dict(3, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for li in range(5):
        bn = 'ConvLayers.%d.' % BN[li]
        C = sd[bn + 'weight'].shape[0]
        sd[bn + 'weight'] = 1.0 + 0.1 * torch.randn(C, generator=g)
        sd[bn + 'bias'] = 0.1 * torch.randn(C, generator=g) + (3.0 if margin else 0.0)
        sd[bn + 'num_batches_tracked'] = torch.tensor(NBT0, dtype=torch.int64)
    draw = lambda *shape: (torch.rand(*shape, generator=g) < 0.25).float()          # noqa: E731
    obs = draw(B, N, 3, 11, 11)
    if near_ties:
        from test_gpu_training_f64 import without_pool_near_ties
        obs = without_pool_near_ties(sd, obs, draw)
    cot = torch.randn(N, B, 128, generator=g)
    return sd, obs, cot


# ---- the float64 statement --------------------------------------------------------------------------------------------
def statement(sd, obs, cot, dtype, keep=False):
    """test_gpu_training_f64.statement cut at the features, in `dtype` on the CPU: per-agent train-mode encoder calls
    (BatchNorm over that call's batch, N sequential running-statistics updates, num_batches_tracked += 1 per call), the
    cotangent cot [N,B,128] on feat, every gradient by autograd.  -> feat [N,B,128], grads, running, nbt.
    keep: also the per-call inputs and outputs of every convolution (with the gradients the backward left on them)."""
    p = {k: sd[k].to(dtype).clone().requires_grad_(True) for k in PARAM_KEYS}
    run = {k: sd[k].to(dtype).clone() for k in RUNNING_KEYS}
    nbt = {k: int(v) for k, v in sd.items() if 'num_batches' in k}
    B, N = obs.shape[0], obs.shape[1]
    x = obs.to(dtype)
    enc, xs, ys = [], [[] for _ in range(5)], [[] for _ in range(5)]
    for n in range(N):
        t = x[:, n]
        for li in range(5):
            xs[li].append(t)
            t = tF.conv2d(t, p['ConvLayers.%d.weight' % CONV[li]], p['ConvLayers.%d.bias' % CONV[li]], padding=1)
            if keep:
                t.retain_grad()
            ys[li].append(t)
            bn = 'ConvLayers.%d.' % BN[li]
            t = tF.batch_norm(t, run[bn + 'running_mean'], run[bn + 'running_var'], p[bn + 'weight'], p[bn + 'bias'],
                              training=True, momentum=MOMENTUM, eps=EPS)
            nbt[bn + 'num_batches_tracked'] += 1
            t = tF.relu(t)
            if orc.POOL_AFTER[li]:
                t = tF.max_pool2d(t, 2)
        enc.append(t.reshape(B, 128))
    feat = torch.stack(enc, 0)                                            # [N,B,128]
    (feat * cot.to(dtype)).sum().backward()
    res = dict(feat=feat.detach(), grads={k: v.grad for k, v in p.items()}, running=run, nbt=nbt)
    if keep:
        res['x'] = [[t.detach() for t in row] for row in xs]
        res['y'] = [[t.detach() for t in row] for row in ys]
        res['dy'] = [[t.grad for t in row] for row in ys]
    return res


@functools.lru_cache(maxsize=None)
def statements(N, B, seed, margin):
    """(float64, fp32) statements of a shape's inputs: computed once, shared by every case of the shape."""
    sd, obs, cot = inputs(N, B, seed, margin)
    return statement(sd, obs, cot, torch.float64), statement(sd, obs, cot, torch.float32)


def grad_scale(k, g64, B):
    """The scale of the yardstick's floor for the gradient of parameter k (None: the gradient's own largest entry)."""
    li = CONV.index(int(k.split('.')[1])) if int(k.split('.')[1]) in CONV else None
    if li is not None and k.endswith('.bias'):
        return g64['ConvLayers.%d.weight' % CONV[li]].abs().max().item() * np.sqrt(B * POS[li])
    return None


def tensor_class(k):
    if k == 'feat':
        return 'feat'
    if 'running' in k:
        return k.split('.')[-1]
    conv = int(k.split('.')[1]) in CONV
    return ('conv_' if conv else 'bn_') + ('w' if k.endswith('weight') else 'b') + '_grad'


def allowed_error(w64, w32, scale=None):
    """The largest error the yardstick lets pass in a tensor: MAX_K x the fp32 statement's largest error + the floor."""
    _, rep = gap(w32, w64, w32, scale)
    return MAX_K * rep['max32'] + ULPS * ULP * rep['scale']


def check_against_f64(got, w64, w32, N, B, update_running):
    """-> (failures, {tensor class: (largest RMS ratio, largest max ratio) to the fp32 yardstick})."""
    bad, ratios = [], {}

    def cmp(name, a, b64, b32, scale=None):
        ok, rep = gap(a, b64, b32, scale)
        if not ok:
            bad.append((name, rep))
        r = ratios.setdefault(tensor_class(name), [0.0, 0.0])
        if rep['rms32'] > 0 and rep['max32'] > 0:
            r[0], r[1] = max(r[0], rep['rms'] / rep['rms32']), max(r[1], rep['max'] / rep['max32'])
    cmp('feat', got['feat'], w64['feat'], w32['feat'])
    for k in PARAM_KEYS:
        cmp(k, got['grads'][k], w64['grads'][k], w32['grads'][k], grad_scale(k, w64['grads'], B))
    if update_running:
        for k in RUNNING_KEYS:
            cmp(k, got['running'][k], w64['running'][k], w32['running'][k])
        for k, c in got['nbt'].items():
            if c != w64['nbt'][k]:
                bad.append((k, c, w64['nbt'][k]))
    return bad, {k: tuple(v) for k, v in ratios.items()}


# ---- the runner -------------------------------------------------------------------------------------------------------
def _call_once(bk, case, sd, obs_np, cot_np, poison, null_counters):
    """One forward + backward of the case on a workspace (and guards) filled with `poison`: every output as host arrays,
    and the two guards' bits."""
    lib, N, B = bk.lib, case['N'], case['B']
    keep = {}
    P, G = EncoderParams(), EncoderGrads()
    for k in PARAM_KEYS + RUNNING_KEYS:                                   # (fresh running-statistic buffers per run)
        keep[k] = bk.put(sd[k].numpy().astype(np.float32))
    for field, fmt, idx in FIELDS + (('bn_mean', 'ConvLayers.%d.running_mean', BN), ('bn_var', 'ConvLayers.%d.running_var', BN)):
        for i in range(5):
            getattr(P, field)[i] = keep[fmt % idx[i]].ptr.value
    P.bn_eps = EPS
    grads = {k: bk.empty(tuple(sd[k].shape)) for k in PARAM_KEYS}
    for field, fmt, idx in FIELDS:
        for i in range(5):
            getattr(G, field)[i] = grads[fmt % idx[i]].ptr.value
    nbt = [bk.put(np.full(1, NBT0, np.int64)) for _ in range(5)]
    counters = None if null_counters else (ctypes.c_void_p * 5)(*[c.ptr.value for c in nbt])
    total = lib.gnnpp_encoder_train_workspace_floats(N, B)
    assert total > 0 and total % 4 == 0
    buf = bk.put(np.full(GUARD + total + GUARD, poison, np.float32))
    assert buf.ptr.value % 16 == 0
    ws = ctypes.c_void_p(buf.ptr.value + 4 * GUARD)
    tp = None
    if case['ext']:
        tp = bk.empty((lib.gnnpp_train_pack_floats(),))
        assert tp.ptr.value % 16 == 0
        assert lib.gnnpp_train_pack(ctypes.byref(P), tp.ptr, None, None, None, 0, 0, 0, 0, bk.stream) == 0
    obs_d, cot_d, feat = bk.put(obs_np), bk.put(cot_np), bk.empty((N * B, 128))
    rc = lib.gnnpp_encoder_train_fwd(ctypes.byref(P), obs_d.ptr, ws, feat.ptr, B, N, ctypes.c_float(MOMENTUM), case['upd'],
                                     counters, case['fsm'], tp.ptr if tp else None, bk.stream)
    assert rc == 0, rc
    bk.sync()
    rc = lib.gnnpp_encoder_train_bwd(ctypes.byref(P), obs_d.ptr, ws, cot_d.ptr, ctypes.byref(G), B, N, case['fsm'],
                                     tp.ptr if tp else None, bk.stream)
    assert rc == 0, rc
    bk.sync()
    f = feat.get()
    f = f.reshape(B, N, 128).transpose(1, 0, 2) if case['fsm'] else f.reshape(N, B, 128)
    out = dict(feat=np.ascontiguousarray(f), grads={k: grads[k].get() for k in PARAM_KEYS},
               running={k: keep[k].get() for k in RUNNING_KEYS},
               nbt={'ConvLayers.%d.num_batches_tracked' % BN[i]: int(nbt[i].get()[0]) for i in range(5)})
    bits = buf.get().view(np.uint32)
    return out, bits[:GUARD].copy(), bits[GUARD + total:].copy(), total


def _flat(out):
    """Every checked output of a run as bytes, in a fixed order."""
    parts = [out['feat']] + [out['grads'][k] for k in PARAM_KEYS] + [out['running'][k] for k in RUNNING_KEYS]
    return b''.join(np.ascontiguousarray(a, np.float32).tobytes() for a in parts) + repr(sorted(out['nbt'].items())).encode()


def run_case(bk, case):
    """The three poisoned runs of a case under its knobs: guards, bitwise agreement, no NaN, and (cases with a statement)
    the NaN run against float64.  -> the ratios of check_against_f64 ({} without a statement)."""
    N, B = case['N'], case['B']
    sd, obs, cot = inputs(N, B, case['seed'], case['margin'], near_ties=case['statement'])
    obs_np = obs.numpy()
    cot_np = np.ascontiguousarray(cot.permute(1, 0, 2).numpy() if case['fsm'] else cot.numpy())
    runs = {}
    with Knobs(bk.lib, {TUNE_TRAIN_WGRAD_WGS: case['wgs'], TUNE_TRAIN_RUNNING_FUSED: case['fused']}):   # restored in its finally
        for name, poison in POISONS:
            want_bits = np.array([poison], np.float32).view(np.uint32)[0]
            out, lo, hi, total = _call_once(bk, case, sd, obs_np, cot_np, poison,
                                            null_counters=not case['upd'] and name == 'zero')
            assert (lo == want_bits).all(), '%s, poison %s: wrote in front of the workspace' % (case['name'], name)
            assert (hi == want_bits).all(), '%s, poison %s: wrote behind the %d floats of the workspace' % (
                case['name'], name, total)
            runs[name] = out
    for name, out in runs.items():
        for k, a in [('feat', out['feat'])] + list(out['grads'].items()) + list(out['running'].items()):
            assert not np.isnan(a).any(), '%s, poison %s: NaN in %s' % (case['name'], name, k)
        if not case['upd']:                                               # handed over, not to be touched
            for k in RUNNING_KEYS:
                assert np.array_equal(out['running'][k], sd[k].numpy()), (case['name'], name, k)
            assert set(out['nbt'].values()) == {NBT0}, (case['name'], name, out['nbt'])
    for name in ('nan', '3e38'):
        for k, a, b in ([('feat', runs['zero']['feat'], runs[name]['feat'])] +
                        [(k, runs['zero']['grads'][k], runs[name]['grads'][k]) for k in PARAM_KEYS] +
                        [(k, runs['zero']['running'][k], runs[name]['running'][k]) for k in RUNNING_KEYS]):
            assert a.tobytes() == b.tobytes(), '%s: %s differs between the 0.0 and the %s workspace (%d entries)' % (
                case['name'], k, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
        assert _flat(runs['zero']) == _flat(runs[name]), (case['name'], name)
    if not case['statement']:
        return {}
    w64, w32 = statements(N, B, case['seed'], case['margin'])
    bad, ratios = check_against_f64(runs['nan'], w64, w32, N, B, case['upd'])
    print('train-encoder ABI %s: %s' % (case['name'], ' '.join(
        '%s rms x%.2f max x%.2f' % (k, v[0], v[1]) for k, v in sorted(ratios.items()))))
    assert not bad, '%s\n%s' % (case['name'], '\n'.join(str(b) for b in bad))
    return ratios
