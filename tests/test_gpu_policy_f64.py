"""GPU (-m gpu): the inference encoder and the policy forward (the hot path bench.py measures) against a float64
statement of the same network, with the fp32 CPU statement as the yardstick (tests/f64_yardstick.py; statements,
networks, the restated dispatch and the runner in tests/policy_f64_cases.py).  Every case runs under each precision
(GNNPP_PREC_FP32 = bf16x3, _FP32_MFMA, _SPLIT_F16) and its id names the kernel instance it reaches under each
(`expect`; the runner asserts it against the restated dispatch and the observable half of the path).

Checked per call: the features [M,128] of gnnpp_encoder_fwd; the logits [N,B,5] of gnnpp_policy_fwd (and, on the
unfused path, the features it leaves in its workspace); the actions gnnpp_decode_actions makes of them, which must be
the float64 arg-max on every row whose float64 top-2 margin exceeds twice the logit error the case allows.

Covered: encoder launch shapes M = 1 .. 4099 around the tile edges, the column-packed ("CP") b3 tiles auto / 1 / 7 /
12, the 16-agent b3 tiles (M > 2048 or GNNPP_TUNE_ENCODER_CP_TILE = 16 or GNNPP_TUNE_POLICY_CP = 0); the fused b3
kernel <K, CP> for N = 1 .. 16, K = 2..4, B = 1 .. 512, and with B > 512 (GNNPP_TUNE_FUSED_POLICY = 2); the unfused
path (B = 600, N = 17 / 50 / 100, K = 1 / 5, GNNPP_TUNE_FUSED_POLICY = 0); fp32 and fp64 GSOs; planners with two
filter layers, E = 2 edge features and a GSO larger than the team through the module API.  Observations: binary,
one-plane bf16 values, real and signed, and binary tiles with ONE residual pixel (1 + 2^-8: the m plane; 1 + 2^-16:
the l plane only) in the first agent, the last agent of a full tile, the last agent of a ragged tile and at the last
pixel -- the tiles whose L0 plane skipping (encoder_kernel_b3.hip) must keep that pixel's low planes.  Activation
scales 1e-6 .. 1e3 on every layer, BatchNorm edges, weights over six decades, and a weak output channel per layer.

Split-f16 is held to the yardstick at activation scales >= 1.  Below, its encoder has a documented ABSOLUTE error
floor (include/gnnpp.h): the activations are split into f16 hi + lo halves unscaled, so the lo half of an activation
far below 1 is an f16 subnormal (spacing 2^-24) and every product carries an error of up to ~2^-25 |w| whatever the
activation.  The error therefore stops shrinking with the activations; test_split_f16_encoder_error_floor pins that
it grows no further: on the same network the largest absolute feature error at activation scales 1e-3 and 1e-6
stays within 4x of its value at scale 1.
"""
import functools

import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import policy_f64_cases as pc
from gnn_pathplanning_amd._native import TUNE_ENCODER_CP_TILE, TUNE_FUSED_POLICY, TUNE_POLICY_CP

pytestmark = pytest.mark.gpu

B3, B3CP, F32, H2 = 'encoder_kernel_b3<false,3>', 'encoder_kernel_b3<false,3,true>', 'encoder_kernel_f32', \
    'encoder_kernel_h2<false,3>'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


# ---- networks and statements, computed once per case -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(seed, M, kind, variant):
    obs1 = pc.make_obs(seed, M, kind)
    return pc.make_net(seed, obs1, **dict(variant)), obs1


@functools.lru_cache(maxsize=None)
def _base(seed, M, kind, scale, variant):
    """(sd, obs, features f64, features f32) of a calibrated network on obs of `kind` at activation scale `scale`."""
    sd1, obs1 = _net(seed, M, kind, variant)
    sd = pc.rescale(sd1, scale)
    obs = (obs1.double() * scale).float()
    pc.check_scales(sd, obs, scale)
    with torch.no_grad():
        return sd, obs, pc.encoder_statement(sd, obs.double(), torch.float64).numpy(), \
            pc.encoder_statement(sd, obs, torch.float32).numpy()


def _enc_inputs(c, scale):
    sd, obs, w64, w32 = _base(c.get('seed', 1), c['M'], c.get('obs', 'binary'), scale,
                              tuple(sorted(c.get('net', {}).items())))
    if 'resid' in c:                                             # one agent differs: patch its row of the statements
        a, kind, last = c['resid']
        obs = pc.with_residual(obs, a, kind, last)
        w64, w32 = w64.copy(), w32.copy()
        with torch.no_grad():
            w64[a] = pc.encoder_statement(sd, obs[a:a + 1].double(), torch.float64).numpy()[0]
            w32[a] = pc.encoder_statement(sd, obs[a:a + 1], torch.float32).numpy()[0]
    return sd, obs, w64, w32


def _id(c):
    return c['name']


# ---- encoder cases -----------------------------------------------------------------------------------------------
def _enc_cases():
    C = []
    for M in (1, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 4099):
        t = (M + 255) // 256
        kern = B3 if t > 8 else '%s[tile%d]' % (B3CP, t)
        C.append(dict(name='%s/M%d' % (kern, M), M=M, seed=M, obs='real' if M % 2 else 'binary',
                      expect={0: kern, 1: F32, 2: H2}))
    for knob in (1, 7, 12, 16):
        kern = B3 if knob == 16 else '%s[tile%d]' % (B3CP, knob)
        for M in (17, 257):
            C.append(dict(name='%s/M%d/cp_knob%d' % (kern, M, knob), M=M, seed=M, obs='real',
                          knobs={TUNE_ENCODER_CP_TILE: knob}, expect={0: kern, 1: F32, 2: H2}))
    C.append(dict(name='%s/M257/policy_cp0' % B3, M=257, seed=257, obs='real', knobs={TUNE_POLICY_CP: 0},
                  expect={0: B3, 1: F32, 2: H2}))
    C.append(dict(name='%s[tile1]/M40/bf16obs' % B3CP, M=40, seed=40, obs='bf16', expect={0: B3CP + '[tile1]'}))
    C.append(dict(name='%s/M40/bf16obs' % B3, M=40, seed=40, obs='bf16', knobs={TUNE_ENCODER_CP_TILE: 16}, expect={0: B3}))
    # one residual pixel in an otherwise binary tile: 16-agent tiles (M = 4099: 256 full tiles + a ragged one of 3)
    # and CP tiles (M = 2047: tiles of 8, a ragged last one of 7).  The plane flag is a ballot per wave of the staging
    # loop (four waves, 1024 consecutive pixels of the tile per round): agent 0's centre pixel is staged by wave 0,
    # agent 2's by wave 3
    for M, tile, kern in ((4099, 16, B3), (2047, 8, '%s[tile8]' % B3CP)):
        for kind in ('m', 'l'):
            for where, a, last in (('first', 0, False), ('agent2_wave3', 2, False),
                                   ('full_tile_last', 2 * tile - 1, False), ('ragged_tile_last', M - 1, False),
                                   ('last_pixel', tile - 1, True)):
                C.append(dict(name='%s/M%d/resid_%s/%s' % (kern, M, kind, where), M=M, seed=M, obs='binary',
                              resid=(a, kind, last), expect={0: kern}))
    return C


ENC = _enc_cases()


@pytest.mark.parametrize('prec', pc.PRECS, ids=pc.PREC_NAMES.get)
@pytest.mark.parametrize('case', ENC, ids=_id)
def test_encoder_f64(bk, case, prec):
    sd, obs, w64, w32 = _enc_inputs(case, 1.0)
    got, kern, flag = pc.run_encoder(bk, sd, obs, prec, case.get('knobs'), case['expect'], name=case['name'])
    assert flag == 0, (case['name'], kern)
    pc.check('%s/%s' % (kern, pc.PREC_NAMES[prec]), got, w64, w32)


# activation scales and network edges: 16-agent tiles (M = 4099) and CP tiles (M = 300: tiles of 2)
NETS = [('plain', {}), ('spread', dict(spread=True)), ('weak_channel', dict(weak=True)),
        ('bn_gamma_neg_zero', dict(bn_edge='gamma')), ('bn_mean_offset', dict(bn_edge='mean')),
        ('bn_var_edges', dict(bn_edge='var')), ('conv_bias_large', dict(bn_edge='bias'))]
SCALED = [dict(name='%s/M4099/%s' % (B3, n), M=4099, seed=11, obs='real', net=v) for n, v in NETS] + \
         [dict(name='%s[tile2]/M300/%s' % (B3CP, n), M=300, seed=12, obs='binary', net=v) for n, v in NETS[:3]]


@pytest.mark.parametrize('scale', (1e-6, 1e-3, 1.0, 1e3))
@pytest.mark.parametrize('prec', pc.PRECS, ids=pc.PREC_NAMES.get)
@pytest.mark.parametrize('case', SCALED, ids=_id)
def test_encoder_scales_f64(bk, case, prec, scale):
    sd, obs, w64, w32 = _enc_inputs(case, scale)
    got, kern, flag = pc.run_encoder(bk, sd, obs, prec, case.get('knobs'), name=case['name'])
    assert flag == 0, (case['name'], kern, scale)                 # split-f16: below the range guard
    if prec == 2 and scale < 1:
        return                                                    # the documented floor: see the next test
    pc.check('%s/%s/scale=%g' % (kern, pc.PREC_NAMES[prec], scale), got, w64, w32)


@pytest.mark.parametrize('case', [c for c in SCALED if c['net'] in ({}, dict(weak=True))], ids=_id)
def test_split_f16_encoder_error_floor(bk, case):
    """encoder_kernel_h2: the largest absolute feature error at activation scales 1e-3 and 1e-6 stays within 4x of its
    value at scale 1 (the activations' lo halves are f16 subnormals there: an absolute floor of ~2^-25 |w| per product
    that no longer shrinks with the activations, and must not grow either)."""
    err = {}
    for scale in (1.0, 1e-3, 1e-6):
        sd, obs, w64, _ = _enc_inputs(case, scale)
        got, _, flag = pc.run_encoder(bk, sd, obs, 2, case.get('knobs'), name=case['name'])
        assert flag == 0
        err[scale] = float(np.abs(got - w64).max())
    assert err[1e-3] <= 4 * err[1.0] and err[1e-6] <= 4 * err[1.0], err


# ---- policy cases ------------------------------------------------------------------------------------------------
def _fused_name(N, K, prec2=False):
    return 'encoder_kernel_h2<true,%d>' % K if prec2 else \
        'encoder_kernel_b3<true,%d,%s>' % (K, 'true' if N <= pc.CP_MAX else 'false')


def _policy_cases():
    C = []
    unfused = lambda B, N: pc.encoder_kernel(B * N, 0, 0, 1) + '+filter'   # noqa: E731
    for N in (1, 2, 11, 12, 13, 16):
        for K in (2, 3, 4):
            for B in (1, 33, 512):
                C.append(dict(name='%s/B%dN%dK%d' % (_fused_name(N, K), B, N, K), B=B, N=N, K=K,
                              seed=1000 + 100 * N + 10 * K + B % 7, obs='real' if (N + K) % 2 else 'binary',
                              f64=(B + K) % 2 == 0,
                              expect={0: _fused_name(N, K), 1: F32, 2: _fused_name(N, K, True)}))
    C.append(dict(name='%s/B600N10K3/fused2' % _fused_name(10, 3), B=600, N=10, K=3, seed=2001, obs='real',
                  knobs={TUNE_FUSED_POLICY: 2}, expect={0: _fused_name(10, 3), 1: F32, 2: _fused_name(10, 3, True)}))
    C.append(dict(name='encoder_kernel_b3<true,3,false>/B16N10K3/policy_cp0', B=16, N=10, K=3, seed=2002,
                  obs='real', knobs={TUNE_POLICY_CP: 0}, expect={0: 'encoder_kernel_b3<true,3,false>'}))
    C.append(dict(name='%s/B600N10K3' % unfused(600, 10), B=600, N=10, K=3, seed=2003, obs='binary',
                  expect={0: unfused(600, 10), 1: F32, 2: H2}))
    for N, B, K in ((17, 5, 3), (50, 3, 2), (100, 2, 4)):
        C.append(dict(name='%s/B%dN%dK%d' % (unfused(B, N), B, N, K), B=B, N=N, K=K, seed=2010 + N, obs='real',
                      f64=N == 50, expect={0: unfused(B, N), 1: F32, 2: H2}))
    for K in (1, 5):
        C.append(dict(name='%s/B9N10K%d' % (unfused(9, 10), K), B=9, N=10, K=K, seed=2020 + K, obs='real',
                      f64=K == 5, expect={0: unfused(9, 10), 1: F32, 2: H2}))
    C.append(dict(name='%s/B9N10K3/fused0' % unfused(9, 10), B=9, N=10, K=3, seed=2030, obs='real',
                  knobs={TUNE_FUSED_POLICY: 0}, expect={0: unfused(9, 10), 1: F32, 2: H2}))
    # a residual pixel through the fused kernels' L0 (last agent of the team, last pixel)
    for N in (10, 16):
        for kind in ('m', 'l'):
            C.append(dict(name='%s/B33N%dK3/resid_%s' % (_fused_name(N, 3), N, kind), B=33, N=N, K=3,
                          seed=2040 + N, obs='binary', resid=(33 * N - 1, kind, True),
                          expect={0: _fused_name(N, 3)}))
    return C


POLICY = _policy_cases()


@functools.lru_cache(maxsize=None)
def _policy_inputs(name):
    c = next(c for c in POLICY + POLICY_SCALED if c['name'] == name)
    B, N, K, scale = c['B'], c['N'], c['K'], c.get('scale', 1.0)
    obs1 = pc.make_obs(c['seed'], B * N, c['obs'])
    if 'resid' in c:
        obs1 = pc.with_residual(obs1, *c['resid'])
    sd = pc.make_net(c['seed'], obs1, K=K, scale=scale, **c.get('net', {}))
    obs = (obs1.double() * scale).float()
    pc.check_scales(sd, obs, scale)
    S = pc.make_gso(c['seed'], B, 1, N, f64=c.get('f64', False))
    with torch.no_grad():
        f64, l64 = (t.numpy() for t in pc.policy_statement(sd, S, obs.reshape(B, N, 3, 11, 11), torch.float64))
        f32, l32 = (t.numpy() for t in pc.policy_statement(sd, S, obs.reshape(B, N, 3, 11, 11), torch.float32))
    return sd, obs.reshape(B, N, 3, 11, 11), S, f64, l64, f32, l32


def _run_policy_case(bk, c, prec):
    sd, obs, S, f64, l64, f32, l32 = _policy_inputs(c['name'])
    logits, acts, feat, kern, flag = pc.run_policy(bk, sd, obs, S, c['K'], prec, c.get('knobs'), c.get('expect'),
                                                   name=c['name'])
    assert flag == 0, (c['name'], kern)
    tag = '%s/%s/%s' % (c['name'], kern, pc.PREC_NAMES[prec])
    if prec == 2 and c.get('scale', 1.0) < 1:
        return
    rep = pc.check(tag + '/logits', logits, l64, l32)
    if feat is not None:
        pc.check(tag + '/features', feat, f64, f32)
    pc.check_actions(tag, acts, l64, rep)


@pytest.mark.parametrize('prec', pc.PRECS, ids=pc.PREC_NAMES.get)
@pytest.mark.parametrize('case', POLICY, ids=_id)
def test_policy_f64(bk, case, prec):
    _run_policy_case(bk, case, prec)


POLICY_SCALED = [dict(name='%s/B33N10K3/%s/scale=%g' % (_fused_name(10, 3), n, s), B=33, N=10, K=3, seed=3000,
                      obs='real', net=v, scale=s)
                 for n, v in (('plain', {}), ('weak_channel', dict(weak=True)),
                              ('bn_mean_offset', dict(bn_edge='mean')))
                 for s in (1e-6, 1e-3, 1.0, 1e3)] + \
                [dict(name='%s/B3N50K3/%s/scale=%g' % (pc.encoder_kernel(150, 0, 0, 1) + '+filter', n, s), B=3, N=50,
                      K=3, seed=3001, obs='real', net=v, scale=s)
                 for n, v in (('plain', {}), ('spread', dict(spread=True))) for s in (1e-6, 1e-3, 1.0, 1e3)]


@pytest.mark.parametrize('prec', pc.PRECS, ids=pc.PREC_NAMES.get)
@pytest.mark.parametrize('case', POLICY_SCALED, ids=_id)
def test_policy_scales_f64(bk, case, prec):
    _run_policy_case(bk, case, prec)


# ---- the module API: several filter layers, E = 2, a GSO larger than the team --------------------------------------
@pytest.mark.parametrize('prec', ('fp32', 'fp32_mfma', 'split_f16'))
@pytest.mark.parametrize('ci', range(4), ids=lambda i: 'multilayer%d' % i)
def test_module_api_planners_f64(dev, policy_golden, multilayer_golden, ci, prec):
    """DecentralPlannerNet with the planners of tests/golden/policy_multilayer.npz (L = 2 and / or E = 2; teams of 5,
    10 and 50): the encoder kernel, gnnpp_lsigf_fwd per inner layer and gnnpp_filter_head_fwd; the single-layer E = 2
    planner through gnnpp_policy_fwd (E = 2 never takes the fused kernel)."""
    from conftest import multilayer_state_dict
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    zp, _ = policy_golden
    zm, meta = multilayer_golden
    m = meta[ci]

    class C:
        num_agents, nGraphFilterTaps, device = m['N'], list(m['taps']), dev
        dimNodeSignals, numEdgeFeatures, precision, range_policy = list(m['dims']), m['E'], prec, 'flag'
    net = DecentralPlannerNet(C()).to(dev).eval()
    sd = multilayer_state_dict(zp, zm, ci)
    net.load_state_dict(sd)
    obs = torch.from_numpy(zm['m%d_obs' % ci]).float()
    S = torch.from_numpy(zm['m%d_S' % ci])
    S4 = S if S.dim() == 4 else S.unsqueeze(1)
    net.addGSO((S4.squeeze(1) if m['E'] == 1 else S4).to(dev))
    with torch.no_grad():
        logits = net.forward_logits(obs.to(dev))
        acts = net.decode_actions(logits).cpu().numpy()
    assert not net.range_exceeded()
    _, l64 = pc.policy_statement(sd, S4, obs, torch.float64)
    _, l32 = pc.policy_statement(sd, S4, obs, torch.float32)
    rep = pc.check('multilayer%d/%s/logits' % (ci, prec), logits.cpu().numpy(), l64.numpy(), l32.numpy())
    pc.check_actions('multilayer%d/%s' % (ci, prec), acts, l64.numpy(), rep)


@pytest.mark.parametrize('prec', ('fp32', 'fp32_mfma', 'split_f16'))
@pytest.mark.parametrize('f64', (0, 1))
def test_module_api_gso_larger_than_team_f64(dev, f64, prec):
    """A GSO of 9 nodes for a team of 6: the encoder kernel, then gnnpp_filter_head_fwd on the zero-padded signal."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    B, N, Ns, K = 5, 6, 9, 3
    obs1 = pc.make_obs(4000 + f64, B * N, 'real')
    sd = pc.make_net(4000 + f64, obs1, K=K)
    obs = obs1.reshape(B, N, 3, 11, 11)
    S = pc.make_gso(4000 + f64, B, 1, N, Ns=Ns, f64=bool(f64))

    class C:
        num_agents, nGraphFilterTaps, device, precision, range_policy = N, K, dev, prec, 'flag'
    net = DecentralPlannerNet(C()).to(dev).eval()
    net.load_state_dict(sd)
    net.addGSO(S.squeeze(1).to(dev))
    with torch.no_grad():
        logits = net.forward_logits(obs.to(dev))
        acts = net.decode_actions(logits).cpu().numpy()
    assert not net.range_exceeded()
    _, l64 = pc.policy_statement(sd, S, obs, torch.float64)
    _, l32 = pc.policy_statement(sd, S, obs, torch.float32)
    rep = pc.check('gso9_team6/%s' % prec, logits.cpu().numpy(), l64.numpy(), l32.numpy())
    pc.check_actions('gso9_team6/%s' % prec, acts, l64.numpy(), rep)
