"""CPU: run the UNMODIFIED HIP kernel sources through the lane-accurate host emulation in
tests/emu/ (one fiber per work-item, emulated 16x16x4 fp32 MFMA / ballot / readlane, real LDS)
and compare with the golden vectors from the reference.  This checks fragment layouts, LDS
indexing, tap skipping, BN folding, pooling and both output layouts without a GPU.  The `-m gpu`
tests repeat the same comparisons on the real hardware through the real libgnnpp.so."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

from gnn_pathplanning_amd import _native  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')

TOL = 1e-4      # the north_star's fp32 logit tolerance; observed ~1e-6


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib, emu_lib.load()


def test_emu_lsigf_golden(emu, lsigf_golden):
    el, lib = emu
    z, meta = lsigf_golden
    ran = 0
    for i, m in enumerate(meta):
        h, S, x = z['c%d_h' % i], z['c%d_S' % i], z['c%d_x' % i]
        if m['G'] > 32 and S.shape[-1] > 10:
            continue                      # keep the emulated run short; GPU tests cover all
        b = z['c%d_b' % i] if m['has_bias'] else None
        batched = m['kind'] in ('BatchLSIGF', 'GraphFilterBatch')
        y = el.lsigf(lib, h, S, x, b, batched, Nin=m.get('Nin'))
        want = z['c%d_y' % i]
        assert y.shape == want.shape
        err = np.abs(y - want).max()
        assert err <= TOL * max(1.0, np.abs(want).max()), (i, m, err)
        ran += 1
    assert ran >= 30


def test_emu_lsigf_node_major_relu(emu, lsigf_golden):
    el, lib = emu
    z, meta = lsigf_golden
    i = next(i for i, m in enumerate(meta) if m['kind'] == 'BatchLSIGF' and m['K'] == 3
             and z['c%d_S' % i].shape[-1] == 10)
    h, S, x, want = z['c%d_h' % i], z['c%d_S' % i], z['c%d_x' % i], z['c%d_y' % i]
    b = z['c%d_b' % i] if meta[i]['has_bias'] else None
    y = el.lsigf(lib, h, S, np.ascontiguousarray(x.transpose(0, 2, 1)), b, True, relu=1,
                 x_node_major=1, y_node_major=1)
    assert np.abs(y.transpose(0, 2, 1) - np.maximum(want, 0)).max() <= TOL


PRECS = [0, 1, 2]       # GNNPP_PREC_FP32 (bf16x3, default) | GNNPP_PREC_FP32_MFMA (exact) | GNNPP_PREC_SPLIT_F16


@pytest.mark.parametrize('prec', PRECS)
def test_emu_policy_golden(emu, policy_golden, prec):
    el, lib = emu
    z, meta = policy_golden
    sd = {k[3:]: z[k] for k in z.files if k.startswith('sd/')}
    enc = el.pack_encoder(lib, sd)
    for i, m in enumerate(meta):
        if m['N'] > 10:
            continue
        B, N, K = m['B'], m['N'], m['K']
        obs = el.f32(z['p%d_obs' % i])
        feat = np.full((B * N, 128), np.nan, dtype=np.float32)
        assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat), B * N, prec, None, None) == 0
        want_feat = z['p%d_feat' % i].transpose(0, 2, 1).reshape(B * N, 128)
        assert np.abs(feat - want_feat).max() <= TOL, (i, m)
        # whole policy step through the single C entry point
        gw = z['sd/GFL.0.weight'] if K == 3 else z['gfl_w_K%d' % K]
        filt = el.pack_filter(lib, gw)
        S = np.ascontiguousarray(z['p%d_S' % i])
        is64 = int(S.dtype == np.float64)
        logits = np.full((N, B, 5), np.nan, dtype=np.float32)
        ws = np.zeros((B * N, 128), dtype=np.float32)
        gb = el.f32(sd['GFL.0.bias'].reshape(-1))
        aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
        rc = lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb),
                                  el.ptr(aw), el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, K, 1,
                                  is64, prec, None, None)
        assert rc == 0
        want = z['p%d_logits' % i]                         # [B,N,5]
        got = logits.transpose(1, 0, 2)
        assert np.abs(got - want).max() <= TOL, (i, m, np.abs(got - want).max())
        assert (got.argmax(-1) == want.argmax(-1)).all()
        acts = np.full((B, N), -1, dtype=np.int32)
        assert lib.gnnpp_decode_actions(el.ptr(logits), el.ptr(acts), B, N, None) == 0
        assert (acts == want.argmax(-1)).all()


def _non_finite_case(B=4, N=10, K=3):
    """Graph 1 carries one NaN pixel, graph 2 one +Inf pixel; graphs 0 and 3 are clean."""
    import torch
    from oracle import policy_oracle as orc
    sd_t = orc.init_state_dict(K, seed=3)
    obs_t = orc.synth_obs(B, N, seed=4)
    obs_t[1, 3, 0, 5, 5] = float('nan')
    obs_t[2, 0, 1, 2, 7] = float('inf')
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=4)).float()
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S, obs_t), 1).numpy()     # [B,N,5]
    return sd_t, obs_t, S, want


@pytest.mark.parametrize('prec', PRECS)
def test_emu_non_finite_observations_are_flushed(emu, prec):
    """VERDICT r04 item 7, the documented deviation ("Numerics"): torch.relu propagates NaN / Inf
    (graphs/models/decentralplanner.py:166) and the dense x @ S of BatchLSIGF (utils/graphUtils/graphML.py:2350) then
    makes EVERY agent of that graph NaN (0 * NaN); the kernels' ReLU (v_med3 / fmaxf) flushes a non-finite activation to
    a finite value, so the graph's logits stay finite.  Pinned here: the oracle has NaN rows exactly in the two
    poisoned graphs, the kernels (both dispatch paths) return finite logits there and the CLEAN graphs are untouched
    (no leak across graphs, parity within the tolerance)."""
    el, lib = emu
    sd_t, obs_t, S, want = _non_finite_case()
    sd = {k: v.numpy() for k, v in sd_t.items()}
    B, N, K = 4, 10, 3
    assert np.isnan(want[1]).all() and np.isnan(want[2]).all() and np.isfinite(want[[0, 3]]).all()
    enc, filt = el.pack_encoder(lib, sd), el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    try:
        for fused in (1, 0):
            lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, fused)
            obs, Sn = el.f32(obs_t.numpy()), el.f32(S.numpy())
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * N, 128), dtype=np.float32)
            rc = lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(Sn), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                      el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, K, 1, 0, prec, None, None)
            assert rc == 0
            got = logits.transpose(1, 0, 2)
            assert np.abs(got[[0, 3]] - want[[0, 3]]).max() <= TOL
            assert np.isfinite(got).all(), (prec, fused)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, 1)


def test_emu_encoder_negative_and_zero_batchnorm_scales(emu):
    """bf16x3 L0 pools its raw accumulators (sign of the folded BatchNorm scale in the packed weights, |scale| in the
    table): gamma < 0 and gamma = 0 channels, binary and real-valued observations, default and exact-fp32 precision."""
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    sd_t = orc.init_state_dict(3, seed=5)
    g = torch.Generator().manual_seed(1)
    sgn = (torch.rand(32, generator=g) < 0.5).float() * 2 - 1
    sd_t['ConvLayers.1.weight'] = sd_t['ConvLayers.1.weight'].abs() * sgn
    sd_t['ConvLayers.1.weight'][3] = 0.0
    enc = el.pack_encoder(lib, {k: v.numpy() for k, v in sd_t.items()})
    for M, binary in ((16, True), (10, False)):
        obs_t = orc.synth_obs(1, M, seed=2)
        if not binary:
            obs_t = obs_t * torch.randn(obs_t.shape, generator=g)
        obs = el.f32(obs_t.numpy().reshape(M, 3, 11, 11))
        want = orc.policy_features(sd_t, obs_t).permute(0, 2, 1).reshape(M, 128).numpy()
        for prec in (0, 1):
            feat = np.zeros((M, 128), np.float32)
            assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat), M, prec, None, None) == 0
            assert np.abs(feat - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (M, binary, prec)


@pytest.mark.parametrize('prec', [0, 2])
def test_emu_fused_policy_kernel_equals_two_kernels(emu, policy_golden, prec):
    """GNNPP_TUNE_FUSED_POLICY: one workgroup per graph (encoder + dense-MFMA shifts + tap contraction + head).
    Split-f16: the very same logits as the encoder kernel followed by the filter kernel (same arithmetic in the same
    order; the dense shift adds exact zeros).  bf16x3 (the default): the two-kernel path contracts the taps on the
    exact fp32 MFMA, the fused one on bf16x3 planes -- both fp32-equivalent, equal to a few ulps."""
    el, lib = emu
    z, meta = policy_golden
    sd = {k[3:]: z[k] for k in z.files if k.startswith('sd/')}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, z['sd/GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    ran = 0
    try:
        for i, m in enumerate(meta):
            if m['K'] != 3 or m['N'] > 16:
                continue
            B, N = m['B'], m['N']
            obs = el.f32(z['p%d_obs' % i])
            S = np.ascontiguousarray(z['p%d_S' % i])
            outs = []
            for mode in (1, 0):
                assert lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, mode) == 0
                logits = np.full((N, B, 5), np.nan, dtype=np.float32)
                ws = np.zeros((B * N, 128), dtype=np.float32)
                assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb),
                                            el.ptr(aw), el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, 3, 1,
                                            int(S.dtype == np.float64), prec, None, None) == 0
                outs.append(logits)
            if prec == 2:
                assert np.array_equal(outs[0], outs[1]), (i, m, np.abs(outs[0] - outs[1]).max())
            else:
                assert np.abs(outs[0] - outs[1]).max() <= 2e-6 * max(1.0, np.abs(outs[1]).max()), (i, m)
            assert np.abs(outs[0].transpose(1, 0, 2) - z['p%d_logits' % i]).max() <= TOL
            ran += 1
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, 1)
    assert ran >= 2


@pytest.mark.parametrize('prec', [0, 2])
@pytest.mark.parametrize('K', [2, 4])
def test_emu_fused_policy_kernel_other_tap_counts(emu, K, prec):
    """The fused policy kernel is instantiated for K = 2, 3, 4 filter taps (16 more weight-ring items and one
    more z buffer per tap): same logits as the two-kernel path, and as the oracle."""
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    B, N = 2, 5
    sd_t = orc.init_state_dict(K, seed=50 + K)
    sd = {k: v.numpy() for k, v in sd_t.items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    obs_t = orc.synth_obs(B, N, seed=K)
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, N, 12, seed=K)).float()
    obs, S = el.f32(obs_t.numpy()), el.f32(S_t.numpy())
    outs = []
    try:
        for mode in (1, 0):
            assert lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, mode) == 0
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * N, 128), dtype=np.float32)
            assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                        el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, K, 1, 0, prec, None, None) == 0
            outs.append(logits)
            if mode == 1:
                assert not ws.any()                          # one kernel: the feature workspace is not written
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FUSED_POLICY, 1)
    if prec == 2:
        assert np.array_equal(outs[0], outs[1]), np.abs(outs[0] - outs[1]).max()
    else:
        assert np.abs(outs[0] - outs[1]).max() <= 2e-6 * max(1.0, np.abs(outs[1]).max())
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S_t, obs_t), 0).numpy()
    assert np.abs(outs[0] - want).max() <= TOL


def test_emu_filter_forced_gpw(emu, lsigf_golden):
    """The graphs-per-workgroup choice only changes the schedule, never the result."""
    el, lib = emu
    z, meta = lsigf_golden
    i = next(i for i, m in enumerate(meta) if m['kind'] == 'BatchLSIGF' and m['K'] == 3
             and m['G'] == 128 and z['c%d_S' % i].shape[-1] == 10)
    h, S, x, want = z['c%d_h' % i], z['c%d_S' % i], z['c%d_x' % i], z['c%d_y' % i]
    b = z['c%d_b' % i] if meta[i]['has_bias'] else None
    try:
        for gpw, waves in ((1, 8), (2, 16), (2, 8), (1, 16)):
            assert (lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, gpw) == 0
                    and lib.gnnpp_set_tuning(_native.TUNE_FILTER_WAVES, waves) == 0)
            y = el.lsigf(lib, h, S, x, b, True)
            assert np.abs(y - want).max() <= TOL, (gpw, waves)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_WAVES, 0)
    # the arithmetic is a per-call argument since ABI 300: the former precision knobs (0: encoder schedule, 5: filter
    # f16), the retired key 8 and the measurement-only knobs (csrc/gnnpp_measure.h) are not part of the ABI
    for retired_key, value in ((8, 0), (0, 7), (5, 1), (_native.TUNE_FILTER_ABLATE, 1), (_native.TUNE_ENCODER_STOP, 1)):
        assert lib.gnnpp_set_tuning(retired_key, value) == -1
        assert lib.gnnpp_get_tuning(retired_key) == -1
    assert lib.gnnpp_version() == 330


def test_emu_lsigf_transposed_and_tap_dump(emu, lsigf_golden):
    """gnnpp_lsigf_fwd_save: (i) s_transposed == running on S^T, (ii) zs holds z_{e,k} = x S_e^k."""
    el, lib = emu
    g = np.random.default_rng(3)
    B, G, F_out, K, E, N = 3, 20, 12, 3, 2, 7
    h = g.standard_normal((F_out, E, K, G)).astype(np.float32) / 8
    x = g.standard_normal((B, G, N)).astype(np.float32)
    S = (g.random((B, E, N, N)) < 0.4) * g.random((B, E, N, N))
    S = S.astype(np.float32)
    packed = el.pack_filter(lib, h)

    def run(Smat, transposed, want_zs):
        y = np.full((B, F_out, N), np.nan, np.float32)
        zs = np.full((E * K, B * N, G), np.nan, np.float32) if want_zs else None
        Sc = np.ascontiguousarray(Smat)
        rc = lib.gnnpp_lsigf_fwd_save(el.ptr(x), el.ptr(Sc), el.ptr(packed), None, el.ptr(y),
                                      el.ptr(zs) if want_zs else None, B, N, N, G, F_out, K, E, 0, 1,
                                      transposed, 0, 0, 0, 0, 0, None, None)
        assert rc == 0
        return y, zs
    y_t, _ = run(S, 1, False)
    y_ref, zs = run(np.ascontiguousarray(S.transpose(0, 1, 3, 2)), 0, True)
    assert np.abs(y_t - y_ref).max() <= 1e-6
    from oracle import policy_oracle as orc
    want = orc.lsigf_f64(h, S.transpose(0, 1, 3, 2), x)
    assert np.abs(y_ref - want).max() <= 1e-4
    # tap signals of the run on S^T
    St = S.transpose(0, 1, 3, 2).astype(np.float64)
    for e in range(E):
        z = x.astype(np.float64)
        for k in range(K):
            if k > 0:
                z = np.einsum('bgm,bmn->bgn', z, St[:, e])
            got = zs[e * K + k].reshape(B, N, G).transpose(0, 2, 1)
            assert np.abs(got - z).max() <= 1e-4, (e, k)


def test_emu_multilayer_and_edge_features(emu, policy_golden, multilayer_golden):
    """Planners with L = 2 graph-filter layers and / or E = 2 edge features against the re-wired
    reference (tests/golden/policy_multilayer.npz): encoder kernel, gnnpp_lsigf_fwd per inner layer
    (node-major, bias + ReLU fused), gnnpp_filter_head_fwd for the last layer + action head; the
    single-layer E = 2 case also through gnnpp_policy_fwd."""
    el, lib = emu
    zp, _ = policy_golden
    zm, meta = multilayer_golden
    sd = {k[3:]: zp[k] for k in zp.files if k.startswith('sd/')}
    enc = el.pack_encoder(lib, sd)
    ran = 0
    for ci, m in enumerate(meta):
        N, B, E = m['N'], m['B'], m['E']
        if N > 10:
            continue                                  # GPU tests cover the 50-agent case
        obs = el.f32(zm['m%d_obs' % ci])
        S = np.ascontiguousarray(zm['m%d_S' % ci])
        is64 = int(S.dtype == np.float64)
        x = np.full((B * N, 128), np.nan, dtype=np.float32)
        assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(x), B * N, 0, None, None) == 0
        dims = [128] + m['dims']
        aw = el.f32(zm['m%d_actionsMLP.0.weight' % ci]); ab = el.f32(zm['m%d_actionsMLP.0.bias' % ci])
        want = zm['m%d_logits' % ci]
        for l in range(len(m['dims'])):
            h = el.f32(zm['m%d_GFL.%d.weight' % (ci, 2 * l)])
            b = el.f32(zm['m%d_GFL.%d.bias' % (ci, 2 * l)].reshape(-1))
            packed = el.pack_filter(lib, h)
            if l + 1 < len(m['dims']):
                y = np.full((B * N, dims[l + 1]), np.nan, dtype=np.float32)
                rc = lib.gnnpp_lsigf_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(b), el.ptr(y), B, N, N,
                                         dims[l], dims[l + 1], m['taps'][l], E, is64, 1, 1, 1, 1, 0, 0, None, None)
                assert rc == 0
                x = y
            else:
                logits = np.full((N, B, 5), np.nan, dtype=np.float32)
                rc = lib.gnnpp_filter_head_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(b), el.ptr(aw),
                                               el.ptr(ab), el.ptr(logits), B, N, dims[l], dims[l + 1],
                                               m['taps'][l], E, is64, 0, None, None)
                assert rc == 0
        got = logits.transpose(1, 0, 2)
        assert np.abs(got - want).max() <= TOL, (ci, m, np.abs(got - want).max())
        assert (got.argmax(-1) == want.argmax(-1)).all()
        if len(m['dims']) == 1 and m['dims'][0] == 128:
            lg2 = np.full((N, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * N, 128), dtype=np.float32)
            rc = lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(packed), el.ptr(b), el.ptr(aw),
                                      el.ptr(ab), el.ptr(ws), el.ptr(lg2), B, N, m['taps'][0], E, is64, 0, None, None)
            assert rc == 0 and np.array_equal(lg2, logits)
        ran += 1
    assert ran >= 3


def test_emu_range_guard(emu):
    """Activations beyond the f16 range of GNNPP_PREC_SPLIT_F16 raise the caller's flag (and only then); the
    other precisions have no such limit and leave the flag alone."""
    el, lib = emu
    g = np.random.default_rng(5)
    B, N, G, F_out, K = 2, 6, 128, 128, 2
    h = (g.standard_normal((F_out, 1, K, G)) / 16).astype(np.float32)
    S = (g.random((B, 1, N, N)) < 0.4).astype(np.float32) * 0.5
    for scale, prec, want_flag in ((1.0, 2, 0), (3.0e4, 2, 0), (4.0e5, 2, 1), (4.0e5, 0, 0), (4.0e5, 1, 0)):
        x = (np.abs(g.standard_normal((B, G, N))) * 0.25 * scale).astype(np.float32)
        x[0, 3, 2] = 0.3 * scale                              # the largest entries stay below / above 65504
        flag = np.zeros(1, np.int32)
        y = el.lsigf(lib, h, S, x, None, True, flag=flag, precision=prec)
        assert int(flag[0]) == want_flag, (scale, prec, flag, np.abs(x).max())
        if not want_flag:
            ref = el_ref(h, S, x)
            assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max()
    # encoder: huge observations overflow the hi halves of L0's input
    from conftest import GOLDEN
    zp = np.load(os.path.join(GOLDEN, 'policy_model.npz'))
    sd = {k[3:]: zp[k] for k in zp.files if k.startswith('sd/')}
    enc = el.pack_encoder(lib, sd)
    obs = (g.random((4, 3, 11, 11)) < 0.1).astype(np.float32)
    feat = np.zeros((4, 128), np.float32)
    flag = np.zeros(1, np.int32)
    assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat), 4, 2, el.ptr(flag), None) == 0
    assert flag[0] == 0 and np.isfinite(feat).all()
    obs[1, 0, 5, 5] = 1.0e5
    feat0 = np.zeros((4, 128), np.float32)
    assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat0), 4, 0, el.ptr(flag), None) == 0
    assert flag[0] == 0 and np.isfinite(feat0).all()          # the default arithmetic has no input domain
    feat1 = np.zeros((4, 128), np.float32)
    assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat1), 4, 1, el.ptr(flag), None) == 0
    assert flag[0] == 0 and np.abs(feat0 - feat1).max() <= 1e-5 * max(1.0, np.abs(feat1).max())
    assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat), 4, 2, el.ptr(flag), None) == 0
    assert flag[0] == 1


def el_ref(h, S, x):
    from oracle import policy_oracle as orc
    return orc.lsigf_f64(h, S, x).astype(np.float32)


def test_emu_filter_two_workgroups_per_graph(emu, lsigf_golden):
    """GNNPP_TUNE_FILTER_SPLIT = n: n workgroups share a graph's row tiles (all run the early shifts
    on all rows, each the last shift / contraction / epilogue on its own tiles).  Same results as one
    workgroup per graph, bit for bit, in both layouts, with Nin < N, E = 2 and the tap dump; two parts, and
    one part per row tile (v320)."""
    el, lib = emu
    z, meta = lsigf_golden
    picked = 0
    try:
        for i, m in enumerate(meta):
            N = z['c%d_S' % i].shape[-1]
            if N < 17 or (m['G'] > 32 and N > 50) or m['kind'] == 'LSIGF':
                continue
            h, S, x = z['c%d_h' % i], z['c%d_S' % i], z['c%d_x' % i]
            b = z['c%d_b' % i] if m['has_bias'] else None
            batched = m['kind'] in ('BatchLSIGF', 'GraphFilterBatch')
            outs = []
            for split in (1, 2, 7):
                assert (lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, split) == 0
                        and lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 1) == 0)
                outs.append(el.lsigf(lib, h, S, x, b, batched, Nin=m.get('Nin')))
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (i, m)
            assert np.abs(outs[1] - z['c%d_y' % i]).max() <= TOL * max(1.0, np.abs(z['c%d_y' % i]).max())
            picked += 1
        # node-major + ReLU + tap dump (training entry point) on a 37-node graph, odd sizes
        g = np.random.default_rng(11)
        B, G, F_out, K, E, N = 3, 24, 20, 3, 2, 37
        h = g.standard_normal((F_out, E, K, G)).astype(np.float32) / 6
        x = g.standard_normal((B, N, G)).astype(np.float32)
        S = (g.random((B, E, N, N)) < 0.15).astype(np.float32) * g.random((B, E, N, N)).astype(np.float32)
        packed = el.pack_filter(lib, h)
        res = []
        for split in (1, 3):
            assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, split) == 0
            y = np.full((B, N, F_out), np.nan, np.float32)
            zs = np.full((E * K, B * N, G), np.nan, np.float32)
            rc = lib.gnnpp_lsigf_fwd_save(el.ptr(x), el.ptr(S), el.ptr(packed), None, el.ptr(y), el.ptr(zs),
                                          B, N, N, G, F_out, K, E, 0, 1, 0, 1, 1, 1, 0, 0, None, None)
            assert rc == 0
            res.append((y, zs))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        from oracle import policy_oracle as orc
        ref = np.maximum(orc.lsigf_f64(h, S, x.transpose(0, 2, 1)), 0).transpose(0, 2, 1)
        assert np.abs(res[1][0] - ref).max() <= TOL * max(1.0, np.abs(ref).max())
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 0)
    assert picked >= 4


@pytest.mark.parametrize('N,K,f64,split,B', [(20, 3, 0, 1, 2), (37, 2, 1, 1, 2), (50, 3, 0, 2, 1), (33, 4, 1, 2, 2),
                                             (18, 1, 0, 1, 1), (21, 3, 0, 1, 3), (92, 2, 0, 1, 1), (100, 3, 1, 1, 1)])
@pytest.mark.parametrize('prec', PRECS)
def test_emu_policy_filter_kernel(emu, N, K, f64, split, B, prec):
    """policy_filter_kernel (filter + ReLU + action head of the policy step for 17..100 agents, one graph per
    workgroup): the general filter kernel's logits to rounding (the head sums eight 16-feature partial products
    instead of one 128-long chain), an fp64 restatement's within TOL; fp32 / fp64 and 16-byte / unaligned GSO slabs,
    one and two workgroups per graph, K = 1..4; 92 / 100 nodes: three / four row tiles per wave, the partial logits
    in the dead S slab (the LDS is full)."""
    el, lib = emu
    g = np.random.default_rng(100 * N + K)
    h = (g.standard_normal((128, 1, K, 128)) / np.sqrt(128 * K)).astype(np.float32)
    x = np.maximum(g.standard_normal((B, N, 128)), 0).astype(np.float32)
    S = ((g.random((B, N, N)) < 0.2) * g.random((B, N, N))).astype(np.float64 if f64 else np.float32)
    S[0, :, N // 2] = g.random(N)                            # a hub: node N/2 gathers from everybody (whole-wave path)
    S[-1, :, 0] = (g.random(N) < 0.5) * g.random(N)          # and a half-hub at the start of the row range
    for b in range(B):
        np.fill_diagonal(S[b], 0)
    bias = (g.standard_normal(128) / 4).astype(np.float32)
    aw = (g.standard_normal((5, 128)) / 8).astype(np.float32)
    ab = g.standard_normal(5).astype(np.float32)
    packed = el.pack_filter(lib, h)
    outs = []
    lib.gnnpp_set_tuning(_native.TUNE_FILTER_WAVES, 0)
    try:
        assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, split) == 0 and lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 1) == 0
        for mode in (1, 0):
            assert (lib.gnnpp_set_tuning(_native.TUNE_POLICY_FILTER, mode) == 0
                    and lib.gnnpp_get_tuning(_native.TUNE_POLICY_FILTER) == mode)
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            flag = np.zeros(1, np.int32)
            assert lib.gnnpp_filter_head_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(bias), el.ptr(aw),
                                             el.ptr(ab), el.ptr(logits), B, N, 128, 128, K, 1, f64, prec,
                                             el.ptr(flag), None) == 0
            assert flag[0] == 0
            outs.append(logits)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_POLICY_FILTER, 1)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 0)
    # fp64 restatement: z_k[b, n, :] = sum_m S[b, m, n] z_{k-1}[b, m, :]
    z = x.astype(np.float64)
    y = np.zeros((B, N, 128))
    for k in range(K):
        y += z @ h[:, 0, k, :].astype(np.float64).T
        z = np.einsum('bmn,bmg->bng', S.astype(np.float32).astype(np.float64), z)
    want = (np.maximum(y + bias, 0) @ aw.astype(np.float64).T + ab).transpose(1, 0, 2)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(outs[0] - want).max() <= TOL * scale
    assert np.abs(outs[0] - outs[1]).max() <= 4e-6 * scale


@pytest.mark.parametrize('N,K,B,f64,head', [(10, 3, 9, 0, 0), (16, 2, 4, 1, 0), (7, 4, 13, 0, 1), (1, 3, 50, 0, 0),
                                            (12, 1, 5, 0, 1), (10, 3, 3, 1, 1)])
def test_emu_small_graph_throughput_kernel(emu, N, K, B, f64, head):
    """lsigf_small_b3_kernel (GNNPP_TUNE_FILTER_SMALL = 2 forces it however few graphs): many small graphs per
    workgroup, dense in-place shifts, bf16x3 planes written by their producer.  Same results as the general filter
    kernel (exact-fp32 MFMA contraction) to a few ulps and as the float64 statement within TOL; ragged last workgroup,
    a workgroup whose rows do not fill its last row tile, fp64 GSOs, K = 1, the fused action head."""
    el, lib = emu
    g = np.random.default_rng(1000 * N + 10 * K + B)
    h = (g.standard_normal((128, 1, K, 128)) / np.sqrt(128 * K)).astype(np.float32)
    x = np.maximum(g.standard_normal((B, N, 128)), 0).astype(np.float32)
    S = ((g.random((B, N, N)) < 0.4) * g.random((B, N, N))).astype(np.float64 if f64 else np.float32)
    bias = (g.standard_normal(128) / 4).astype(np.float32)
    aw = (g.standard_normal((5, 128)) / 8).astype(np.float32)
    ab = g.standard_normal(5).astype(np.float32)
    packed = el.pack_filter(lib, h)
    outs = []
    try:
        # (mode 3: the producer / consumer pipeline kernel -- persistent 8-wave workgroups, 64-row groups; no head form)
        # (pipeline grid 2 / 1: a persistent workgroup takes several groups -- staging of the next group beside the taps)
        for mode, rows, pgrid in ((2, 32, 0), (2, 48, 0), (0, 0, 0)) + (() if head else ((3, 0, 0), (3, 0, 2), (3, 0, 1))):
            assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_PIPE_GRID, pgrid) == 0
            assert (lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL, mode) == 0
                    and lib.gnnpp_get_tuning(_native.TUNE_FILTER_SMALL) == mode)
            assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL_ROWS, rows) == 0
            if head:
                out = np.full((N, B, 5), np.nan, dtype=np.float32)
                assert lib.gnnpp_filter_head_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(bias), el.ptr(aw),
                                                 el.ptr(ab), el.ptr(out), B, N, 128, 128, K, 1, f64, 0, None, None) == 0
            else:
                out = np.full((B, N, 128), np.nan, dtype=np.float32)
                assert lib.gnnpp_lsigf_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(bias), el.ptr(out), B, N, N,
                                           128, 128, K, 1, f64, 1, 1, 1, 1, 0, 0, None, None) == 0
            outs.append(out)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL, 1)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL_ROWS, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_PIPE_GRID, 0)
    z = x.astype(np.float64)
    y = np.zeros((B, N, 128))
    for k in range(K):
        y += z @ h[:, 0, k, :].astype(np.float64).T
        z = np.einsum('bmn,bmg->bng', S.astype(np.float32).astype(np.float64), z)
    y = np.maximum(y + bias, 0)
    want = (y @ aw.astype(np.float64).T + ab).transpose(1, 0, 2) if head else y
    scale = max(1.0, np.abs(want).max())
    assert np.abs(outs[0] - want).max() <= TOL * scale
    assert np.array_equal(outs[0], outs[1])                 # 32- and 48-row workgroups: the same arithmetic per row
    if not head:
        assert all(np.array_equal(outs[0], o) for o in outs[3:])   # ... and the pipeline kernel's, however the groups are dealt
    assert np.abs(outs[0] - outs[2]).max() <= 4e-6 * scale
    assert (lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL, 4) == -1
            and lib.gnnpp_set_tuning(_native.TUNE_FILTER_SMALL_ROWS, 40) == -1)


@pytest.mark.parametrize('N,K,B,real_obs', [(10, 3, 2, False), (12, 3, 1, False), (1, 2, 2, False), (5, 4, 1, False),
                                            (9, 3, 1, True), (11, 2, 1, False), (7, 3, 1, False), (3, 3, 1, True)])
def test_emu_column_packed_policy_kernel_is_bit_identical(emu, N, K, B, real_obs):
    """GNNPP_TUNE_POLICY_CP: the one-launch policy kernel of teams of <= 12 agents with (agent, position) pairs on the
    MFMA columns of its 5x5 layers computes the SAME logits, bit for bit, as the agents-on-columns schedule (every
    output sums the same products in the same order; a tap outside the image adds exact zeros) -- every team size class
    (tiles that end inside a row, waves without a tile, a last tile with missing columns), K = 2, 3, 4, binary and
    real-valued (three-plane) observations -- and matches the oracle."""
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    sd_t = orc.init_state_dict(K, seed=70 + N)
    sd = {k: v.numpy() for k, v in sd_t.items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    obs_t = orc.synth_obs(B, N, seed=N + K)
    if real_obs:
        obs_t = obs_t * torch.randn(obs_t.shape, generator=torch.Generator().manual_seed(N))
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, N, 12, seed=K)).float()
    obs, S = el.f32(obs_t.numpy()), el.f32(S_t.numpy())
    outs = []
    try:
        for cp in (1, 0):
            assert lib.gnnpp_set_tuning(_native.TUNE_POLICY_CP, cp) == 0 and lib.gnnpp_get_tuning(_native.TUNE_POLICY_CP) == cp
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * N, 128), dtype=np.float32)
            assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                        el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, K, 1, 0, 0, None, None) == 0
            assert not ws.any()                              # the one-launch kernel ran (both times)
            outs.append(logits)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_POLICY_CP, 1)
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1]), np.abs(outs[0] - outs[1]).max()
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S_t, obs_t), 0).numpy()
    assert np.abs(outs[0] - want).max() <= TOL
    assert lib.gnnpp_set_tuning(_native.TUNE_POLICY_CP, 2) == -1


@pytest.mark.parametrize('M,tile', [(23, 7), (16, 12), (5, 1), (30, 4), (37, 0), (25, 10)])
def test_emu_column_packed_encoder_tiles_are_bit_identical(emu, M, tile):
    """GNNPP_TUNE_ENCODER_CP_TILE: the unfused encoder in its latency form (column-packed tiles of <= 12 agents; 0 = the
    heuristic ceil(M / 256) -> one agent per tile here) writes the SAME features, bit for bit, as 16-agent tiles: ragged
    last tiles, tiles whose first agent is not 16-byte aligned, binary and real-valued observations."""
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    sd_t = orc.init_state_dict(3, seed=90 + M)
    enc = el.pack_encoder(lib, {k: v.numpy() for k, v in sd_t.items()})
    obs_t = orc.synth_obs(1, M, seed=M)
    if M % 2:
        obs_t = obs_t * torch.randn(obs_t.shape, generator=torch.Generator().manual_seed(M))
    obs = el.f32(obs_t.numpy().reshape(M, 3, 11, 11))
    feats = []
    try:
        for knob in (tile, 16):
            assert (lib.gnnpp_set_tuning(_native.TUNE_ENCODER_CP_TILE, knob) == 0
                    and lib.gnnpp_get_tuning(_native.TUNE_ENCODER_CP_TILE) == knob)
            feat = np.full((M, 128), np.nan, np.float32)
            assert lib.gnnpp_encoder_fwd(el.ptr(obs), el.ptr(enc), el.ptr(feat), M, 0, None, None) == 0
            feats.append(feat)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_ENCODER_CP_TILE, 0)
    assert np.isfinite(feats[0]).all() and np.array_equal(feats[0], feats[1]), np.abs(feats[0] - feats[1]).max()
    want = orc.policy_features(sd_t, obs_t).permute(0, 2, 1).reshape(M, 128).numpy()
    assert np.abs(feats[0] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert lib.gnnpp_set_tuning(_native.TUNE_ENCODER_CP_TILE, 13) == -1


@pytest.mark.parametrize('N,K,f64,B', [(100, 3, 0, 2), (100, 2, 1, 1), (100, 4, 0, 1), (72, 3, 0, 2), (50, 4, 1, 1), (33, 3, 0, 9)])
def test_emu_policy_filter_kernel_n_way_split(emu, N, K, f64, B):
    """up to ceil(N / 16) workgroups per graph in policy_filter_kernel (GNNPP_TUNE_FILTER_SPLIT = n;
    lsigf_plan picks n itself when few graphs would leave CUs idle).  Every part stages the graph and runs the early
    shifts on all rows, the last shift / contraction / head on its own row tiles -- a row's arithmetic does not
    depend on the partition: with the exact-fp32 contraction the logits of every split are the one-workgroup logits
    bit for bit; with the default precision a finer split can move a team from the fp32 MFMA to bf16x3 planes (they
    fit the LDS once a workgroup owns fewer rows: 72 agents from three parts on), so those agree to rounding.  B = 9:
    two groups of 8 graphs, the second one padded.  Hub and isolated nodes, fp64 slabs."""
    el, lib = emu
    g = np.random.default_rng(77 * N + K)
    h = (g.standard_normal((128, 1, K, 128)) / np.sqrt(128 * K)).astype(np.float32)
    x = np.maximum(g.standard_normal((B, N, 128)), 0).astype(np.float32)
    S = ((g.random((B, N, N)) < 0.08) * g.random((B, N, N))).astype(np.float64 if f64 else np.float32)
    S[0, :, N // 2] = g.random(N)                            # a hub: node N/2 gathers from everybody
    S[:, :, 3] = 0                                           # an isolated node (nobody to gather from)
    S[:, :, N - 1] = 0                                       # ... and the last one
    for b in range(B):
        np.fill_diagonal(S[b], 0)
    bias = (g.standard_normal(128) / 4).astype(np.float32)
    aw = (g.standard_normal((5, 128)) / 8).astype(np.float32)
    ab = g.standard_normal(5).astype(np.float32)
    packed = el.pack_filter(lib, h)
    rt = (N + 15) // 16
    splits = sorted({1, 2, 3, rt, 7})                        # (values above the row tiles are clamped to them)
    outs, modes = {}, {}
    lib.gnnpp_set_tuning(_native.TUNE_FILTER_WAVES, 0)
    try:
        assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 1) == 0
        for prec in (1, 0):
            for split in splits:
                assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, split) == 0
                logits = np.full((N, B, 5), np.nan, dtype=np.float32)
                assert lib.gnnpp_filter_head_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(bias), el.ptr(aw),
                                                 el.ptr(ab), el.ptr(logits), B, N, 128, 128, K, 1, f64, prec, None,
                                                 None) == 0
                outs[prec, split] = logits
                modes[prec, split] = lib.gnnpp_filter_head_mode(B, N, K, prec)
        assert lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, 8) == -1
        # r06: the default arithmetic of a SPLIT team of 65 .. 100 agents keeps its bf16x3 planes in the dead z buffer
        # (mode 3) instead of falling back to the exact fp32 MFMA (mode 1: what one workgroup per graph still runs);
        # GNNPP_TUNE_FILTER_PLANE_ALIAS = 0 restores the fallback, whose logits are those of precision 1 bit for bit
        if N == 100:
            assert modes[0, 1] == 1 and modes[0, 2] == 3 and modes[0, 3] == 3 and modes[0, 7] == 3, modes
            assert (lib.gnnpp_set_tuning(_native.TUNE_FILTER_PLANE_ALIAS, 0) == 0
                    and lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, 2) == 0)
            assert lib.gnnpp_filter_head_mode(B, N, K, 0) == 1
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            assert lib.gnnpp_filter_head_fwd(el.ptr(x), el.ptr(S), el.ptr(packed), el.ptr(bias), el.ptr(aw),
                                             el.ptr(ab), el.ptr(logits), B, N, 128, 128, K, 1, f64, 0, None, None) == 0
            assert np.array_equal(logits, outs[1, 2])
        if N == 72:
            assert modes[0, 1] == 1 and modes[0, 2] == 3 and modes[0, 3] == 2, modes
        assert all(modes[1, sp] == 1 for sp in splits)
    finally:
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_SPLIT, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_GPW, 0)
        lib.gnnpp_set_tuning(_native.TUNE_FILTER_PLANE_ALIAS, 1)
    z = x.astype(np.float64)
    y = np.zeros((B, N, 128))
    for k in range(K):
        y += z @ h[:, 0, k, :].astype(np.float64).T
        z = np.einsum('bmn,bmg->bng', S.astype(np.float32).astype(np.float64), z)
    want = (np.maximum(y + bias, 0) @ aw.astype(np.float64).T + ab).transpose(1, 0, 2)
    scale = max(1.0, np.abs(want).max())
    for split in splits:
        assert np.array_equal(outs[1, split], outs[1, 1]), split            # exact fp32: the same bits
        assert np.isfinite(outs[0, split]).all()
        assert np.abs(outs[0, split] - want).max() <= TOL * scale, split
        assert np.abs(outs[0, split] - outs[0, 1]).max() <= 4e-6 * scale, split
