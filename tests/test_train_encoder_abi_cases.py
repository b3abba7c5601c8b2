"""CPU: the cases of tests/train_encoder_abi_cases.py can tell a wrong train-mode encoder from a right one before any GPU
sees them, so that tests/test_gpu_train_encoder_abi.py cannot pass on an implementation with one of the listed mistakes.

(a) the module's statement is test_gpu_training_f64.statement cut at the features: same features, running statistics and
    counters to the bit, and -- fed the cotangent that statement's own backward leaves on the features -- the same 20
    encoder gradients within 64 x 2^-53 of each tensor's scale (float64 roundoff; the operations are the same);
(b) for every case, each wrong variant that applies to it differs from the float64 statement by far more than the yardstick
    allows (MAX_K x the fp32 statement's largest error + the floor): a condition on the inputs, not a tolerance.  A case
    fails on its worst tensor, so the variant's miss in a case is its largest miss-to-allowance ratio over the tensors named
    for it, and that is >= SENSITIVITY; every single one of those tensors misses too, by >= EACH_TENSOR.  Variants:
    features returned in the other layout ([B][N] read as [N][B]; shapes with N, B > 1; feat), the biased instead of the
    unbiased variance in the running statistics (every case that updates them; the five running variances), the last
    image split of the case's own split plan dropped from a weight gradient (every layer with more than one split; the
    conv weight gradients), num_batches_tracked += 1 instead of += N (N > 1: an integer, any difference is a miss).
    Smallest miss-to-allowance ratios over the matrix (printed by the test): per case, other layout 2.4e4 (10 x 13),
    biased variance 6.7e3 (3 x 7), dropped split 1.3e4 (7 x 1, default workgroups); per tensor, biased variance 7.7 (the
    first layer's running variance at 3 x 7: that layer's batch variance is ~1e-2 of the running variance the floor is
    taken of, times 1 / (7 * 121 - 1)), dropped split 5.5e3, other layout as per case;
(c) the case list holds what the device test is meant to cover."""
import numpy as np
import pytest
import torch
import torch.nn.functional as tF

import train_encoder_abi_cases as ab

SENSITIVITY = 100.0                        # the case's worst tensor of a variant, over the allowance
EACH_TENSOR = 4.0                          # every tensor named for the variant
F64_BOUND = 64 * 2.0 ** -53


def _np(t):
    return t.detach().numpy()


def test_statement_is_the_training_statement_cut_at_the_features(monkeypatch):
    import test_gpu_training_f64 as t64
    B, N = 5, 3
    sd, obs, S, tgt = t64.make_case(B, N, seed=11)
    seen = []
    orig = tF.linear

    def linear(x, w, b=None):
        if w is not None and w.shape == (128, 128) and x.requires_grad and x.shape == (B, 128):
            x.retain_grad()                                   # the features of one agent call, as compressMLP gets them
            seen.append(x)
        return orig(x, w, b)
    monkeypatch.setattr(tF, 'linear', linear)
    full = t64.statement(sd, S, obs, tgt, N, torch.float64)
    monkeypatch.undo()
    assert len(seen) == N
    cot = torch.stack([x.grad for x in seen], 0)              # [N,B,128]
    assert cot.abs().max().item() > 0
    mine = ab.statement(sd, obs, cot, torch.float64)
    assert torch.equal(mine['feat'].permute(1, 0, 2), full['feat'])
    for k in ab.RUNNING_KEYS:
        assert torch.equal(mine['running'][k], full['running'][k]), k
    assert mine['nbt'] == full['nbt'] and set(mine['nbt'].values()) == {N}
    for k in ab.PARAM_KEYS:
        a, b = _np(mine['grads'][k]), _np(full['grads'][k])
        assert np.abs(a - b).max() <= F64_BOUND * max(np.abs(b).max(), np.abs(_np(full['grads'][k.rsplit('.', 1)[0] + '.weight'])).max()), k


def _wrong_variants(case):
    """[(variant, tensor, wrong value, float64 value, fp32 value, scale)] of the variants that apply to the case."""
    N, B = case['N'], case['B']
    sd, obs, cot = ab.inputs(N, B, case['seed'], case['margin'])
    w64, w32 = ab.statements(N, B, case['seed'], case['margin'])
    out = []
    if N > 1 and B > 1:
        f = _np(w64['feat'])
        out.append(('layout', 'feat', np.ascontiguousarray(f.transpose(1, 0, 2)).reshape(N, B, 128), f, _np(w32['feat']),
                    None))
    full = ab.statement(sd, obs, cot, torch.float64, keep=True)
    if case['upd']:
        for li in range(5):
            k = 'ConvLayers.%d.running_var' % ab.BN[li]
            r = sd[k].double()
            for n in range(N):
                r = (1 - ab.MOMENTUM) * r + ab.MOMENTUM * full['y'][li][n].var((0, 2, 3), unbiased=False)
            out.append(('biased', k, _np(r), _np(w64['running'][k]), _np(w32['running'][k]), None))
    for li in range(5):
        cin, cout = ab.CHANNELS[li]
        ips, nsplit = ab.split_plan(N, B, case['wgs'], cout)
        if nsplit < 2:
            continue
        k = 'ConvLayers.%d.weight' % ab.CONV[li]
        lost = torch.zeros_like(w64['grads'][k])
        for img in range((nsplit - 1) * ips, N * B):           # the images of the last split, in [N][B] order
            n, b = divmod(img, B)
            lost += torch.nn.grad.conv2d_weight(full['x'][li][n][b:b + 1], lost.shape, full['dy'][li][n][b:b + 1],
                                                padding=1)
        out.append(('split', k, _np(w64['grads'][k] - lost), _np(w64['grads'][k]), _np(w32['grads'][k]), None))
    return out


@pytest.mark.parametrize('case', ab.CASES, ids=ab.case_id)
def test_wrong_variants_are_far_outside_the_yardstick(case):
    rows = _wrong_variants(case)
    assert {r[0] for r in rows} >= ({'split'} if case['N'] * case['B'] > 1 else set()) | \
        ({'biased'} if case['upd'] else set()) | ({'layout'} if min(case['N'], case['B']) > 1 else set())
    miss = {}
    for variant, k, wrong, f64, f32, scale in rows:
        delta, allowed = float(np.abs(wrong - f64).max()), ab.allowed_error(f64, f32, scale)
        print('%s: %s in %s: %.3g, allowed %.3g (x %.2g)' % (case['name'], variant, k, delta, allowed, delta / allowed))
        assert delta >= EACH_TENSOR * allowed, (variant, k, delta, allowed)    # every tensor of the variant fails the check
        miss[variant] = max(miss.get(variant, 0.0), delta / allowed)
    for variant, ratio in miss.items():                        # ... and the case (its worst tensor) by a wide margin
        print('%s: %s misses by x %.2g' % (case['name'], variant, ratio))
        assert ratio >= SENSITIVITY, (variant, ratio)
    if case['N'] > 1:                                           # += 1 instead of += N
        w64, _ = ab.statements(case['N'], case['B'], case['seed'], case['margin'])
        assert set(w64['nbt'].values()) == {ab.NBT0 + case['N']} and ab.NBT0 + 1 not in w64['nbt'].values()


def test_dropped_split_is_what_the_sum_of_all_splits_says():
    """The per-image weight gradients the `split` variant is built from add up to the statement's gradient."""
    case = next(c for c in ab.CASES if c['shape'] == (3, 7) and c['wgs'] == 0)
    sd, obs, cot = ab.inputs(3, 7, case['seed'], case['margin'])
    full = ab.statement(sd, obs, cot, torch.float64, keep=True)
    for li in range(5):
        k = 'ConvLayers.%d.weight' % ab.CONV[li]
        tot = sum(torch.nn.grad.conv2d_weight(full['x'][li][n], full['grads'][k].shape, full['dy'][li][n], padding=1)
                  for n in range(3))
        assert (tot - full['grads'][k]).abs().max().item() <= F64_BOUND * full['grads'][k].abs().max().item(), k


def test_case_list_holds_the_required_rows():
    def has(cases, **kw):
        return any(all(c.get(k) == v for k, v in kw.items()) for c in cases)
    names = [c['name'] for c in ab.CASES + ab.GUARD_ONLY]
    assert len(set(names)) == len(names)
    for shape in ((1, 1), (1, 2), (2, 3), (3, 7), (10, 13), (7, 1)):
        for wgs in (0, 16, 100, 2048):
            assert has(ab.CASES, shape=shape, wgs=wgs, statement=True)
    ab._pairwise_cover(ab.CASES)
    assert all(c['N'] * c['B'] <= 150 for c in ab.CASES)
    assert has(ab.GUARD_ONLY, shape=(10, 129), wgs=0, statement=False)
    assert has(ab.GUARD_ONLY, shape=(10, 129), wgs=2048, statement=False) and len(ab.GUARD_ONLY) == 2
    for shape in ((1, 1), (3, 7), (10, 13)):
        for wgs in (0, 16):
            assert has(ab.EMU_CASES, shape=shape, wgs=wgs)
    assert all(c in ab.CASES for c in ab.EMU_CASES)
    assert ab.GUARD % 4 == 0 and ab.GUARD == 4096
    # the three poisons: 0.0, a NaN, and a finite value whose double overflows
    z, nan, big = (p for _, p in ab.POISONS)
    assert z == 0 and np.isnan(nan) and np.isfinite(big) and big * 0 == 0
    with np.errstate(over='ignore'):
        assert np.isinf(np.float32(big) + np.float32(big))


def test_split_plan_is_the_library_s_workspace():
    """split_plan restated from train_ws_layout: the workspace grows, from one knob value to another, by exactly the floats
    the restated partial slabs grow by (everything else in the layout does not depend on the knob)."""
    from gnn_pathplanning_amd import _native
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    if not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('host clang++ from ROCm not present')
    import emu_lib
    lib = emu_lib.load()

    def slabs(N, B, wgs):
        tot = 0
        for cin, cout in ab.CHANNELS:
            jt = -(-(cin * 9 + 1) // 16)
            tot += ab.split_plan(N, B, wgs, cout)[1] * (2 if jt <= 2 else 1) * cout * jt * 16
        return tot
    old = lib.gnnpp_get_tuning(_native.TUNE_TRAIN_WGRAD_WGS)
    try:
        for N, B in ab.SHAPES + ((10, 129), (10, 128)):
            sizes = {}
            for wgs in ab.WGS:
                assert lib.gnnpp_set_tuning(_native.TUNE_TRAIN_WGRAD_WGS, wgs) == 0
                sizes[wgs] = lib.gnnpp_encoder_train_workspace_floats(N, B)
            for wgs in ab.WGS[1:]:
                assert sizes[wgs] - sizes[0] == slabs(N, B, wgs) - slabs(N, B, 0), (N, B, wgs)
    finally:
        assert lib.gnnpp_set_tuning(_native.TUNE_TRAIN_WGRAD_WGS, old) == 0
