"""Build and bind libgnnpp.so (hipcc, gfx950) -- the only compute path of this package.

The library is built IN-TREE next to this file so that it travels with the source snapshot to the
GPU box.  Binding is plain ctypes over the C ABI of include/gnnpp.h: raw device pointers, sizes and
a hipStream_t; PyTorch only supplies device memory and the stream.
"""
import ctypes
import os
import shutil
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.path.join(_HERE, 'libgnnpp.so')
MEASURE_LIB_PATH = os.path.join(_HERE, 'libgnnpp_measure.so')
# The column-packed layers issue their MFMAs through inline asm on the weight ring's registers, with hand-placed wait
# states the compiler's hazard recogniser cannot see into (csrc/encoder_kernel_b3.hip ring_mfma16b / ring_mfma_fence).
# The static ISA check and the GPU bit-identity tests were run with THIS hipcc; a library built by another one still
# has to pass the ISA check, but its packed layers are switched off at load time until somebody has re-run
# `pytest -m gpu -k column_packed` on it: GNNPP_TUNE_POLICY_CP = 0 and GNNPP_TUNE_ENCODER_CP_TILE = 16 are
# the compiler-scheduled forms of the same layers (same logits to the bit, ~7 % slower at the 10-agent config).
VALIDATED_HIPCC = 'HIP version: 7.2.26015-fc0010cf6a'
TOOLCHAIN_STAMP = LIB_PATH + '.toolchain'           # (next to the library: travels with it, git-ignored like it)
# written by build() when only the OPT-IN split-f16 kernels fail the ISA check: that precision is refused, the build stands
H2_UNSAFE_MARK = LIB_PATH + '.split_f16_disabled'
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp.h')
MAPF_DISTANCE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_mapf_distance.h')
CASEGEN_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_casegen.h')
CASEGEN_MAZE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_casegen_maze.h')
MAPF_AUDIT_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_mapf_audit.h')
ROLLOUT_TRACE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_rollout_trace.h')
SCHEDULE_DRAW_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_schedule_draw.h')
ROLLOUT_STREAM_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_rollout_stream.h')
ROLLOUT_STREAM_TRACE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_rollout_stream_trace.h')
ROLLOUT_TEAM_STREAM_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_rollout_team_stream.h')
TRAIN_B3_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_train_b3.h')
ROLLOUT_SUMMARY_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'gnnpp_rollout_summary.h')
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC',
               '-Wno-unused-result']


class GnnppError(RuntimeError):
    pass


# ---- the C ABI of include/gnnpp.h, stated once for Python --------------------------------------------------------
# Every `#define GNNPP_<NAME> <integer>` of the header under its name without the prefix, every struct as a
# ctypes.Structure and every prototype as an entry of SIGNATURES.  This is the ONLY Python statement of the contract (the
# package, the tools' measure library and the tests' host build of the same sources all bind through bind() below), and
# tests/test_host_logic.py::test_python_abi_matches_header holds all three to the header.
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_RANGE = 0, -1, -2, -3, -4
# GNNPP_PREC_*: the arithmetic of a call's matrix-pipe contractions, passed PER CALL
PREC_FP32, PREC_FP32_MFMA, PREC_SPLIT_F16 = 0, 1, 2
OBS_C, OBS_HW, FEAT, ACTIONS = 3, 11, 128, 5
MAX_NODES, MAX_ROWS = 100, 112
# GNNPP_TUNE_*: keys of gnnpp_set_tuning / gnnpp_get_tuning
TUNE_FILTER_GPW, TUNE_FILTER_WAVES, TUNE_FUSED_POLICY, TUNE_FILTER_SPLIT, TUNE_POLICY_FILTER = 1, 2, 6, 7, 9
TUNE_FILTER_SMALL, TUNE_FILTER_SMALL_ROWS, TUNE_FILTER_PIPE_GRID = 10, 11, 12
TUNE_POLICY_CP, TUNE_ENCODER_CP_TILE, TUNE_FILTER_PLANE_ALIAS = 13, 14, 16        # (15 and 18: removed, not reused)
TUNE_TRAIN_WGRAD_WGS, TUNE_TRAIN_RUNNING_FUSED, TUNE_ENCODER_ONE_PLANE = 17, 19, 20
ROLLOUT_MAX_AGENTS, ROLLOUT_MAX_TEAM, ROLLOUT_TEAM_MAX_CELLS = 128, 1024, 65536
TIE_LOWEST, TIE_HASHED, TIE_REPLAY, TIE_MT19937 = 0, 1, 2, 3
SCHEDULE_BAD_MOVE, SCHEDULE_BAD_STATE, SCHEDULE_NO_RADIUS = 1, 2, 4
MAPF_NO_PATH, MAPF_BAD_CASE = 1, 2
MAPF_MAX_SIDE, MAPF_MAX_STEPS, MAPF_TEAM_MAX_SIDE, MAPF_TEAM_MAX_STEPS = 64, 1024, 256, 2048
# include/gnnpp_mapf_distance.h (GNNPP_MAPF_DIST_*, GNNPP_MAPF_ORDER_*)
MAPF_DIST_UNREACHABLE, MAPF_DIST_INVALID = -1, -2
MAPF_ORDER_INDEX, MAPF_ORDER_LONGEST_FIRST, MAPF_ORDER_SHORTEST_FIRST, MAPF_ORDER_HASHED = 0, 1, 2, 3
# include/gnnpp_casegen.h (GNNPP_CASEGEN_*)
CASEGEN_OK, CASEGEN_TOO_SMALL = 0, 1
# include/gnnpp_mapf_audit.h (GNNPP_MAPF_AUDIT_*): the seam constant, the class indices, the status bits
MAPF_AUDIT_CHUNK = 32
MAPF_AUDIT_CLASS_STATE, MAPF_AUDIT_CLASS_VERTEX, MAPF_AUDIT_CLASS_MOVE, MAPF_AUDIT_CLASS_SWAP = 0, 1, 2, 3
MAPF_AUDIT_STATE, MAPF_AUDIT_VERTEX, MAPF_AUDIT_MOVE, MAPF_AUDIT_SWAP = 1, 2, 4, 8
MAPF_AUDIT_BAD_START, MAPF_AUDIT_NOT_AT_GOAL, MAPF_AUDIT_SKIPPED = 16, 32, 64
# csrc/gnnpp_measure.h: keys that exist in the -DGNNPP_MEASURE build only (libgnnpp.so answers GNNPP_ERR_ARG)
TUNE_FILTER_ABLATE, TUNE_ENCODER_STOP = 3, 4
# csrc/encoder_kernel_b3.hip: 1 (default) = a team of 10 agents runs the packed policy kernel's compile-time-N form, 0 = the
# run-time-N form like every other team size (same logits to the bit); a key of the tests and the A/B tools, in every build
TUNE_POLICY_CP_TEAM = 21
# csrc/encoder_kernel_b3.hip: inside that form, 1 (default) = a one-plane tile runs the first conv layer with (window, agent)
# pairs on the MFMA columns, 0 = with agents on the columns as every other form (same logits to the bit); key 21 = 0
# selects the whole run-time form whatever this key says
TUNE_POLICY_CP_TEAM_L0 = 22
# include/gnnpp_rollout_summary.h (GNNPP_SUMMARY_*): the limits, then the words of out_i64 and of out_f64
SUMMARY_MAX_GROUPS, SUMMARY_I64, SUMMARY_F64 = 64, 16, 8
(SUMMARY_N, SUMMARY_N_REACH_ALL, SUMMARY_N_OPTIMAL, SUMMARY_AGENTS_REACHED, SUMMARY_N_DEGENERATE, SUMMARY_N_BAD_GROUP,
 SUMMARY_SUM_MP_PRED, SUMMARY_SUM_MP_TARGET, SUMMARY_SUM_FT_PRED, SUMMARY_SUM_FT_TARGET, SUMMARY_MIN_REACHED,
 SUMMARY_MAX_REACHED, SUMMARY_N_FAIL_SHIELDED, SUMMARY_N_COLLISION_FREE, SUMMARY_N_SHIELDED) = range(15)
(SUMMARY_RATE_REACH, SUMMARY_AVG_DMP, SUMMARY_STD_DMP, SUMMARY_AVG_DFT, SUMMARY_STD_DFT, SUMMARY_MEAN_REACHED,
 SUMMARY_M2_DMP, SUMMARY_M2_DFT) = range(8)
PRECISIONS = {'fp32': PREC_FP32, 'fp32_mfma': PREC_FP32_MFMA, 'split_f16': PREC_SPLIT_F16}


def precision_code(p):
    """'fp32' (default: bf16x3 operand split, fp32-equivalent, no input domain) | 'fp32_mfma' (exact fp32 MFMA) |
    'split_f16' (fast 22-bit split, |x| < 65504, guarded) or the integer code -> GNNPP_PREC_*."""
    if isinstance(p, str):
        if p not in PRECISIONS:
            raise GnnppError('unknown precision %r (one of %s)' % (p, sorted(PRECISIONS)))
        p = PRECISIONS[p]
    else:
        p = int(p)
        if p not in (PREC_FP32, PREC_FP32_MFMA, PREC_SPLIT_F16):
            raise GnnppError('unknown precision code %d' % p)
    if p == PREC_SPLIT_F16 and os.path.exists(H2_UNSAFE_MARK):
        raise GnnppError("precision 'split_f16' is disabled in this build: the ISA hipcc generated for the opt-in "
                         "split-f16 encoder failed the weight-ring check (%s); the default 'fp32' and 'fp32_mfma' "
                         "are unaffected" % open(H2_UNSAFE_MARK).read().strip()[:200])
    return p


def _sources():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [HEADER, MAPF_DISTANCE_HEADER, CASEGEN_HEADER,
                                                                          MAPF_AUDIT_HEADER, ROLLOUT_TRACE_HEADER,
                                                                          SCHEDULE_DRAW_HEADER, ROLLOUT_STREAM_HEADER,
                                                                          CASEGEN_MAZE_HEADER, ROLLOUT_STREAM_TRACE_HEADER,
                                                                          ROLLOUT_TEAM_STREAM_HEADER, TRAIN_B3_HEADER,
                                                                          ROLLOUT_SUMMARY_HEADER]


def build(force=False, verbose=False, measure=False):
    """hipcc --offload-arch=gfx950 csrc/gnnpp_api.hip -> libgnnpp.so (cross-compiles without a GPU).

    The device ISA of the very same compilation (-save-temps) then goes through
    tools/check_ring_isa.py: the split-f16 encoder keeps a weight ring in registers the compiler
    must never touch, which only a look at the generated code can guarantee -- a toolchain that
    breaks the scheme fails the BUILD, not a test.  measure=True builds libgnnpp_measure.so with
    -DGNNPP_MEASURE (phase-ablation knobs for tools/ab_bench.py; never loaded by the package)."""
    out = MEASURE_LIB_PATH if measure else LIB_PATH
    if (not force and os.path.exists(out)
            and os.path.getmtime(out) >= max(os.path.getmtime(s) for s in _sources())):
        return out
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        raise GnnppError('hipcc not found: libgnnpp.so cannot be built on this machine')
    tmp = os.path.join(_HERE, 'build', 'measure' if measure else 'product')
    os.makedirs(tmp, exist_ok=True)
    tmp_lib = os.path.join(tmp, 'libgnnpp.so')
    cmd = [hipcc] + HIPCC_FLAGS + (['-DGNNPP_MEASURE'] if measure else []) + \
          ['-save-temps', os.path.join(CSRC, 'gnnpp_api.hip'), '-o', tmp_lib]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd, cwd=tmp)
    isa = os.path.join(tmp, 'gnnpp_api-hip-amdgcn-amd-amdhsa-gfx950.s')
    h2_errors = check_ring_isa(isa, verbose=verbose)
    if not measure:
        if h2_errors:                                        # opt-in precision only: refuse IT, keep the build
            with open(H2_UNSAFE_MARK, 'w') as f:
                f.write('; '.join(h2_errors))
        elif os.path.exists(H2_UNSAFE_MARK):
            os.remove(H2_UNSAFE_MARK)
    if not measure:
        try:
            ver = subprocess.check_output([hipcc, '--version'], stderr=subprocess.STDOUT).decode().splitlines()[0].strip()
        except (OSError, subprocess.CalledProcessError, IndexError):
            ver = 'unknown'
        with open(TOOLCHAIN_STAMP, 'w') as f:
            f.write(ver + '\n')
    for f in os.listdir(tmp):                                # keep the ISA, drop the bulky temporaries
        if f != os.path.basename(isa) and f != 'libgnnpp.so':
            os.remove(os.path.join(tmp, f))
    os.replace(tmp_lib, out)
    return out


# (mangled-name substring, stream items, scratch bytes allowed): the encoder and the fused policy kernels for
# K = 2, 3, 4 filter taps.  MUST PASS -- the bf16x3 (fp32-equivalent, DEFAULT) schedule: three planes per fragment, 24
# filter items per tap ...
RING_KERNELS = (('encoder_kernel_b3ILb0ELi3ELb0E', 294, 0), ('encoder_kernel_b3ILb1ELi2ELb0E', 342, 32),
                ('encoder_kernel_b3ILb1ELi3ELb0E', 366, 32), ('encoder_kernel_b3ILb1ELi4ELb0E', 390, 32),
                # ... and its column-packed form for teams of <= 12 agents (third template argument; fourth = 0: run-time N)
                ('encoder_kernel_b3ILb1ELi2ELb1ELi0E', 342, 32), ('encoder_kernel_b3ILb1ELi3ELb1ELi0E', 366, 32),
                ('encoder_kernel_b3ILb1ELi4ELb1ELi0E', 390, 32), ('encoder_kernel_b3ILb0ELi3ELb1ELi0E', 294, 0))
# ... and the packed policy kernel with the team size as a constant (fourth template argument = 10): its first packed layer
# drops the units that hold nothing but zeros, the ring sees the same items in the same order.  MUST PASS as well.
RING_KERNELS_TEAM = (('encoder_kernel_b3ILb1ELi2ELb1ELi10E', 342, 32), ('encoder_kernel_b3ILb1ELi3ELb1ELi10E', 366, 32),
                     ('encoder_kernel_b3ILb1ELi4ELb1ELi10E', 390, 32))
# OPT-IN precision 'split_f16' (16 more fragments per tap): a violation here disables THAT precision
# (H2_UNSAFE_MARK, precision_code) instead of failing the build of the default path
RING_KERNELS_OPTIONAL = (('encoder_kernel_h2ILb0ELi3E', 196, 0), ('encoder_kernel_h2ILb1ELi2E', 228, 32),
                         ('encoder_kernel_h2ILb1ELi3E', 244, 32), ('encoder_kernel_h2ILb1ELi4E', 260, 32))


def check_ring_isa(isa_path, verbose=False):
    """tools/check_ring_isa.py on every instantiation of the ring-managed encoder kernels: ring registers private to
    the asm, load -> wait -> take discipline on every path, every stream item loaded and taken exactly once, 256
    VGPRs, occupancy 2, no (encoder) / tiny (policy) scratch.  A violation in a kernel of the default bf16x3 schedule
    raises (the build fails); violations in the opt-in split-f16 kernels are RETURNED as a list of messages."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'gnnpp_check_ring_isa', os.path.join(os.path.dirname(_HERE), 'tools', 'check_ring_isa.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    optional_errors = []
    for kern, items, scratch in RING_KERNELS + RING_KERNELS_TEAM + RING_KERNELS_OPTIONAL:
        errors, stats, meta = mod.check(isa_path, kern, scratch)
        ok = (not errors and stats['loads'] == items and stats['takes'] == items
              and meta.get('NumVgprs') == 256 and meta.get('Occupancy') == 2)
        if verbose or not ok:
            print('ring ISA check %s: %s %s, %d violation(s)' % (kern, stats, meta, len(errors)))
        if ok:
            continue
        if (kern, items, scratch) in RING_KERNELS_OPTIONAL:
            optional_errors.append('%s: %s %s %s' % (kern, stats, meta, errors[:2]))
            continue
        raise GnnppError('generated ISA of %s violates the weight-ring discipline (%s): this '
                         'toolchain cannot build the bf16x3 encoder safely' % (kern, errors[:3]))
    return optional_errors


class EncoderParams(ctypes.Structure):
    """struct gnnpp_encoder_params (include/gnnpp.h)."""
    _fields_ = [('conv_w', ctypes.c_void_p * 5), ('conv_b', ctypes.c_void_p * 5),
                ('bn_w', ctypes.c_void_p * 5), ('bn_b', ctypes.c_void_p * 5),
                ('bn_mean', ctypes.c_void_p * 5), ('bn_var', ctypes.c_void_p * 5),
                ('fc_w', ctypes.c_void_p), ('fc_b', ctypes.c_void_p), ('bn_eps', ctypes.c_float)]


class EncoderGrads(ctypes.Structure):
    """struct gnnpp_encoder_grads (include/gnnpp.h)."""
    _fields_ = [('conv_w', ctypes.c_void_p * 5), ('conv_b', ctypes.c_void_p * 5),
                ('bn_w', ctypes.c_void_p * 5), ('bn_b', ctypes.c_void_p * 5)]


class GemmDesc(ctypes.Structure):
    """struct gnnpp_gemm_desc (include/gnnpp.h)."""
    _fields_ = [('A', ctypes.c_void_p), ('a_sb', ctypes.c_longlong), ('a_sm', ctypes.c_longlong),
                ('a_sk', ctypes.c_longlong), ('B', ctypes.c_void_p), ('b_sb', ctypes.c_longlong),
                ('b_sk', ctypes.c_longlong), ('C', ctypes.c_void_p), ('c_sb', ctypes.c_longlong),
                ('c_sm', ctypes.c_longlong), ('batch', ctypes.c_int), ('M', ctypes.c_int), ('N', ctypes.c_int),
                ('K', ctypes.c_int), ('mask', ctypes.c_void_p)]


class AdamTensors(ctypes.Structure):
    """struct gnnpp_adam_tensors (include/gnnpp.h)."""
    _fields_ = [('p', ctypes.c_void_p * 32), ('g', ctypes.c_void_p * 32), ('m', ctypes.c_void_p * 32),
                ('v', ctypes.c_void_p * 32), ('numel', ctypes.c_longlong * 32), ('count', ctypes.c_int)]


class RolloutStruct(ctypes.Structure):
    """struct gnnpp_rollout (include/gnnpp.h)."""
    _fields_ = [('grid', ctypes.c_void_p), ('grid_batched', ctypes.c_int), ('goal', ctypes.c_void_p),
                ('pos', ctypes.c_void_p), ('B', ctypes.c_int), ('N', ctypes.c_int),
                ('H', ctypes.c_int), ('W', ctypes.c_int), ('obs', ctypes.c_void_p),
                ('radius', ctypes.c_void_p), ('S', ctypes.c_void_p), ('connected', ctypes.c_void_p),
                ('grow', ctypes.c_int), ('logits', ctypes.c_void_p), ('actions', ctypes.c_void_p),
                ('reached', ctypes.c_void_p), ('start_step', ctypes.c_void_p),
                ('end_step', ctypes.c_void_p), ('maxstep', ctypes.c_void_p),
                ('done', ctypes.c_void_p), ('flags', ctypes.c_void_p), ('stats', ctypes.c_void_p), ('currentstep', ctypes.c_int),
                ('tie_mode', ctypes.c_int), ('seed', ctypes.c_uint), ('choices', ctypes.c_void_p),
                ('choice_count', ctypes.c_void_p), ('max_choices', ctypes.c_int),
                ('range_flag', ctypes.c_void_p), ('rng_words', ctypes.c_void_p),
                ('rng_cursor', ctypes.c_void_p), ('rng_max', ctypes.c_int)]


class ScheduleStruct(ctypes.Structure):
    """struct gnnpp_schedules (include/gnnpp.h)."""
    _fields_ = [('grid', ctypes.c_void_p), ('grid_batched', ctypes.c_int), ('goal', ctypes.c_void_p),
                ('pos', ctypes.c_void_p), ('case_start', ctypes.c_void_p), ('C', ctypes.c_int), ('N', ctypes.c_int),
                ('H', ctypes.c_int), ('W', ctypes.c_int), ('T_total', ctypes.c_int), ('radius0', ctypes.c_double),
                ('obs', ctypes.c_void_p), ('S', ctypes.c_void_p), ('S64', ctypes.c_void_p),
                ('target', ctypes.c_void_p), ('radius', ctypes.c_void_p), ('growth', ctypes.c_void_p),
                ('status', ctypes.c_void_p), ('step_info', ctypes.c_void_p)]


class MapfStruct(ctypes.Structure):
    """struct gnnpp_mapf (include/gnnpp.h)."""
    _fields_ = [('grid', ctypes.c_void_p), ('grid_batched', ctypes.c_int), ('start', ctypes.c_void_p),
                ('goal', ctypes.c_void_p), ('order', ctypes.c_void_p), ('C', ctypes.c_int), ('N', ctypes.c_int),
                ('H', ctypes.c_int), ('W', ctypes.c_int), ('R', ctypes.c_int), ('T_max', ctypes.c_int),
                ('schedule', ctypes.c_void_p), ('arrival', ctypes.c_void_p), ('makespan', ctypes.c_void_p),
                ('flowtime', ctypes.c_void_p), ('status', ctypes.c_void_p), ('failing', ctypes.c_void_p),
                ('restart', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class RolloutTraceStruct(ctypes.Structure):
    """struct gnnpp_rollout_trace (include/gnnpp_rollout_trace.h)."""
    _fields_ = [('path', ctypes.c_void_p), ('action', ctypes.c_void_p), ('moves', ctypes.c_void_p),
                ('shielded', ctypes.c_void_p), ('steps', ctypes.c_void_p), ('seen_done', ctypes.c_void_p),
                ('T_cap', ctypes.c_int)]


class RolloutStreamStruct(ctypes.Structure):
    """struct gnnpp_rollout_stream (include/gnnpp_rollout_stream.h)."""
    _fields_ = [('case_grid', ctypes.c_void_p), ('case_grid_batched', ctypes.c_int), ('case_start', ctypes.c_void_p),
                ('case_goal', ctypes.c_void_p), ('case_maxstep', ctypes.c_void_p), ('C', ctypes.c_int),
                ('commR', ctypes.c_double), ('cursor', ctypes.c_void_p), ('slot_case', ctypes.c_void_p),
                ('slot_t0', ctypes.c_void_p), ('assign', ctypes.c_void_p), ('slot_grid', ctypes.c_void_p),
                ('goal', ctypes.c_void_p), ('maxstep', ctypes.c_void_p), ('reached', ctypes.c_void_p),
                ('start_step', ctypes.c_void_p), ('end_step', ctypes.c_void_p), ('pos', ctypes.c_void_p),
                ('radius', ctypes.c_void_p), ('stats', ctypes.c_void_p), ('lived', ctypes.c_void_p),
                ('slot', ctypes.c_void_p), ('t0', ctypes.c_void_p)]


class RolloutStreamTraceStruct(ctypes.Structure):
    """struct gnnpp_rollout_stream_trace (include/gnnpp_rollout_stream_trace.h)."""
    _fields_ = [('path', ctypes.c_void_p), ('action', ctypes.c_void_p), ('moves', ctypes.c_void_p),
                ('shielded', ctypes.c_void_p), ('steps', ctypes.c_void_p), ('seen_done', ctypes.c_void_p),
                ('T_cap', ctypes.c_int)]


class RolloutSummaryIn(ctypes.Structure):
    """struct gnnpp_rollout_summary_in (include/gnnpp_rollout_summary.h)."""
    _fields_ = [('reached', ctypes.c_void_p), ('stats', ctypes.c_void_p), ('target_makespan', ctypes.c_void_p),
                ('target_flowtime', ctypes.c_void_p), ('valid', ctypes.c_void_p), ('group', ctypes.c_void_p),
                ('shielded', ctypes.c_void_p), ('audit_ok', ctypes.c_void_p), ('C', ctypes.c_int), ('N', ctypes.c_int),
                ('G', ctypes.c_int), ('target_stride', ctypes.c_int)]


_vp, _ci, _cs, _ll, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_float
_enc, _rollout = ctypes.POINTER(EncoderParams), ctypes.POINTER(RolloutStruct)
_sched, _mapf, _gemm = ctypes.POINTER(ScheduleStruct), ctypes.POINTER(MapfStruct), ctypes.POINTER(GemmDesc)

# name -> (restype, argtypes) of every exported call, in the header's order
SIGNATURES = {
    'gnnpp_version': (_ci, []),
    'gnnpp_error_string': (ctypes.c_char_p, [_ci]),
    'gnnpp_set_tuning': (_ci, [_ci, _ci]),
    'gnnpp_get_tuning': (_ci, [_ci]),
    'gnnpp_filter_packed_floats': (_cs, [_ci] * 4),
    'gnnpp_filter_pack': (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    'gnnpp_lsigf_fwd': (_ci, [_vp] * 5 + [_ci] * 14 + [_vp, _vp]),
    'gnnpp_lsigf_fwd_save': (_ci, [_vp] * 6 + [_ci] * 15 + [_vp, _vp]),
    'gnnpp_lsigf_fits': (_ci, [_ci] * 5),
    'gnnpp_encoder_packed_floats': (_cs, []),
    'gnnpp_encoder_pack': (_ci, [_enc, _vp, _vp]),
    'gnnpp_encoder_fwd': (_ci, [_vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    'gnnpp_encoder_train_workspace_floats': (_cs, [_ci, _ci]),
    'gnnpp_encoder_train_fwd': (_ci, [_enc, _vp, _vp, _vp, _ci, _ci, _cf, _ci, ctypes.POINTER(_vp), _ci, _vp, _vp]),
    'gnnpp_encoder_train_bwd': (_ci, [_enc, _vp, _vp, _vp, ctypes.POINTER(EncoderGrads), _ci, _ci, _ci, _vp, _vp]),
    'gnnpp_train_pack_floats': (_cs, []),
    'gnnpp_train_pack': (_ci, [_enc, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    'gnnpp_lsigf_input_grad': (_ci, [_vp] * 5 + [_ci] * 9 + [_vp]),
    'gnnpp_linear_fwd': (_ci, [_vp] * 4 + [_ci] * 4 + [_vp]),
    'gnnpp_gemm_workspace_floats': (_cs, [_ci] * 4),
    'gnnpp_gemm_kmajor': (_ci, [_vp, _ll, _ll, _ll, _vp, _ll, _ll, _vp, _ll, _ll, _ci, _ci, _ci, _ci, _vp, _vp]),
    'gnnpp_gemm_multi_workspace_floats': (_cs, [_gemm, _ci]),
    'gnnpp_gemm_kmajor_multi': (_ci, [_gemm, _ci, _vp, _vp]),
    'gnnpp_policy_loss': (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    'gnnpp_adam_step': (_ci, [ctypes.POINTER(AdamTensors), _vp, _cf, _cf, _cf, _cf, _cf, _ci, _vp]),
    'gnnpp_policy_fwd': (_ci, [_vp] * 9 + [_ci] * 6 + [_vp, _vp]),
    'gnnpp_filter_head_fwd': (_ci, [_vp] * 7 + [_ci] * 8 + [_vp, _vp]),
    'gnnpp_filter_head_mode': (_ci, [_ci] * 4),
    'gnnpp_decode_actions': (_ci, [_vp, _vp, _ci, _ci, _vp]),
    'gnnpp_lsigf_team_workspace_bytes': (_cs, [_ci] * 6),
    'gnnpp_lsigf_team_fwd': (_ci, [_vp] * 6 + [_cs] + [_ci] * 11 + [_vp]),
    'gnnpp_filter_head_team_fwd': (_ci, [_vp] * 8 + [_cs] + [_ci] * 8 + [_vp]),
    'gnnpp_policy_team_fwd': (_ci, [_vp] * 9 + [_ci] * 6 + [_vp, _vp, _vp, _cs]),
    'gnnpp_team_lists_bytes': (_cs, [_ci, _ci]),
    'gnnpp_team_lists_from_dense': (_ci, [_vp, _vp, _cs, _ci, _ci, _ci, _vp]),
    'gnnpp_lsigf_team_lists_fwd': (_ci, [_vp] * 6 + [_cs] + [_ci] * 10 + [_vp]),
    'gnnpp_filter_head_team_lists_fwd': (_ci, [_vp] * 8 + [_cs] + [_ci] * 7 + [_vp]),
    'gnnpp_policy_team_lists_fwd': (_ci, [_vp] * 9 + [_ci] * 5 + [_vp, _vp, _vp, _cs]),
    'gnnpp_team_lists_transpose': (_ci, [_vp, _vp, _cs, _ci, _ci, _vp]),
    'gnnpp_lsigf_team_lists_fwd_save': (_ci, [_vp] * 7 + [_cs] + [_ci] * 10 + [_vp]),
    'gnnpp_lsigf_team_lists_input_grad': (_ci, [_vp] * 5 + [_cs] + [_ci] * 7 + [_vp]),
    'gnnpp_rollout_observe': (_ci, [_rollout, _vp]),
    'gnnpp_rollout_gso': (_ci, [_rollout, _vp]),
    'gnnpp_rollout_move': (_ci, [_rollout, _vp]),
    'gnnpp_rollout_gso_observe': (_ci, [_rollout, _vp]),
    'gnnpp_rollout_lists': (_ci, [_rollout, _vp, _cs, _vp]),
    'gnnpp_rollout_step': (_ci, [_rollout, _vp]),
    'gnnpp_rollout_policy_step': (_ci, [_rollout] + [_vp] * 5 + [_ci, _ci, _vp]),
    'gnnpp_rollout_policy_steps': (_ci, [_rollout] + [_vp] * 5 + [_ci, _ci, _ci, _vp]),
    'gnnpp_schedule_samples': (_ci, [_sched, _vp]),
    'gnnpp_schedule_team_workspace_bytes': (_cs, [_ci, _ci]),
    'gnnpp_schedule_team_samples': (_ci, [_sched, _vp, _cs, _vp]),
    'gnnpp_schedule_team_plan': (_ci, [_sched, _vp, _cs, _vp, _vp]),
    'gnnpp_schedule_team_fill_lists': (_ci, [_sched, _vp, _cs, _vp, _vp, _vp, _ci, _vp]),
    'gnnpp_team_lists_gather': (_ci, [_vp, _vp, _vp, _ci, _ci, _vp, _ci, _vp, _cs, _ci, _vp]),
    'gnnpp_mapf_workspace_bytes': (_cs, [_ci] * 4),
    'gnnpp_mapf_solve': (_ci, [_mapf, _vp]),
    'gnnpp_mapf_team_workspace_bytes': (_cs, [_ci] * 5),
    'gnnpp_mapf_team_solve': (_ci, [_mapf, _vp]),
}
EXPORTS = tuple(SIGNATURES)
# include/gnnpp_mapf_distance.h, the companion header of the MAPF solver's goal distances and planning orders: exported by
# every build like the calls above, stated in a table of its own because the header is (tests/test_mapf_distance_abi.py
# holds the two to each other the way test_python_abi_matches_header holds SIGNATURES to gnnpp.h)
MAPF_DISTANCE_SIGNATURES = {
    'gnnpp_mapf_distances': (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    'gnnpp_mapf_orders': (_ci, [_vp, _ci, _ci, _ci, _vp, ctypes.c_uint, _vp, _vp]),
}
# include/gnnpp_casegen.h, the companion header of the case generator: a table of its own for the same reason
# (tests/test_casegen_abi.py)
CASEGEN_SIGNATURES = {
    'gnnpp_casegen': (_ci, [_vp, _ci, ctypes.c_uint, ctypes.c_uint, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# include/gnnpp_mapf_audit.h, the companion header of the schedule audit: a table of its own for the same reason
# (tests/test_mapf_audit_abi.py)
MAPF_AUDIT_SIGNATURES = {
    'gnnpp_mapf_audit_workspace_bytes': (_cs, [_ci] * 3),
    'gnnpp_mapf_audit': (_ci, [_vp, _ci] + [_vp] * 4 + [_ci] * 5 + [_vp] * 7 + [_cs, _vp]),
}
# include/gnnpp_rollout_trace.h, the companion header of the rollout's trace: a table of its own for the same reason
# (tests/test_rollout_trace_abi.py)
_trace = ctypes.POINTER(RolloutTraceStruct)
ROLLOUT_TRACE_SIGNATURES = {
    'gnnpp_rollout_trace_begin': (_ci, [_rollout, _trace, _vp]),
    'gnnpp_rollout_trace_record': (_ci, [_rollout, _trace, _vp]),
    'gnnpp_rollout_policy_steps_traced': (_ci, [_rollout] + [_vp] * 5 + [_ci, _ci, _ci, _trace, _vp]),
}
# include/gnnpp_schedule_draw.h, the companion header of the draw from stored schedules: a table of its own for the same
# reason (tests/test_schedule_draw_abi.py)
SCHEDULE_DRAW_SIGNATURES = {
    'gnnpp_schedule_draw_workspace_bytes': (_cs, [_ci, _ci]),
    'gnnpp_schedule_draw': (_ci, [_sched, _vp, _ci, _vp, _vp, _vp, _vp, _cs, _vp, _cs, _vp]),
}
# include/gnnpp_rollout_stream.h, the companion header of streamed rollouts: a table of its own for the same reason
# (tests/test_rollout_stream_abi.py)
_rstream = ctypes.POINTER(RolloutStreamStruct)
ROLLOUT_STREAM_SIGNATURES = {
    'gnnpp_rollout_stream_begin': (_ci, [_rollout, _rstream, _vp]),
    'gnnpp_rollout_stream_reseat': (_ci, [_rollout, _rstream, _ci, _vp]),
}
# include/gnnpp_casegen_maze.h, the companion header of the maze maps: a table of its own for the same reason
# (tests/test_casegen_maze_abi.py)
CASEGEN_MAZE_SIGNATURES = {
    'gnnpp_casegen_maze': (_ci, [_vp, ctypes.c_uint, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
}
# include/gnnpp_rollout_stream_trace.h, the companion header of a streamed rollout's trace: a table of its own for the same
# reason (tests/test_rollout_stream_trace_abi.py)
_rstrace = ctypes.POINTER(RolloutStreamTraceStruct)
ROLLOUT_STREAM_TRACE_SIGNATURES = {
    'gnnpp_rollout_stream_trace_begin': (_ci, [_rollout, _rstream, _rstrace, _vp]),
    'gnnpp_rollout_stream_trace_record': (_ci, [_rollout, _rstream, _rstrace, _vp]),
    'gnnpp_rollout_stream_policy_steps_traced': (_ci, [_rollout] + [_vp] * 5 + [_ci, _ci, _ci, _rstream, _rstrace, _vp]),
}
# include/gnnpp_rollout_team_stream.h, the companion header of streamed rollouts of large teams: a table of its own for the
# same reason (tests/test_rollout_team_stream_abi.py); it adds no struct
ROLLOUT_TEAM_STREAM_SIGNATURES = {
    'gnnpp_rollout_team_stream_begin': (_ci, [_rollout, _rstream, _vp]),
    'gnnpp_rollout_team_stream_reseat': (_ci, [_rollout, _rstream, _ci, _vp, _cs, _vp]),
}
# include/gnnpp_train_b3.h, the companion header of the opt-in bf16x3 training precision: a table of its own for the same
# reason (tests/test_train_b3_pack.py); it adds no struct.  The _prec calls take the argument lists of
# gnnpp_encoder_train_fwd / _bwd + (int precision, const void* pack_b3)
TRAIN_B3_SIGNATURES = {
    'gnnpp_train_pack_b3_bytes': (_cs, []),
    'gnnpp_train_pack_b3': (_ci, [_enc, _vp, _vp]),
    'gnnpp_encoder_train_fwd_prec': (_ci, SIGNATURES['gnnpp_encoder_train_fwd'][1] + [_ci, _vp]),
    'gnnpp_encoder_train_bwd_prec': (_ci, SIGNATURES['gnnpp_encoder_train_bwd'][1] + [_ci, _vp]),
}
# include/gnnpp_rollout_summary.h, the companion header of a rollout's summary: a table of its own for the same reason
# (tests/test_rollout_summary_abi.py)
ROLLOUT_SUMMARY_SIGNATURES = {
    'gnnpp_rollout_summary_out_bytes': (_cs, [_ci, _ci]),
    'gnnpp_rollout_summary': (_ci, [ctypes.POINTER(RolloutSummaryIn), _vp, _vp]),
}
# config field `trainPrecision` of DecentralPlannerNet -> the `precision` of the _prec calls (exact fp32 is the default)
TRAIN_PRECISIONS = {'fp32': PREC_FP32_MFMA, 'bf16x3': PREC_FP32}
# csrc/gnnpp_api.hip, -DGNNPP_MEASURE builds only (int gnnpp_measure_read_stamps(unsigned long long* host, int n))
MEASURE_SIGNATURES = {'gnnpp_measure_read_stamps': (_ci, [_vp, _ci])}


def bind(library):
    """Give every exported call of an opened build of csrc/gnnpp_api.hip (the product, the measure build, the tests' host
    build) its prototype from SIGNATURES, MAPF_DISTANCE_SIGNATURES, CASEGEN_SIGNATURES, MAPF_AUDIT_SIGNATURES,
    ROLLOUT_TRACE_SIGNATURES, SCHEDULE_DRAW_SIGNATURES, ROLLOUT_STREAM_SIGNATURES, CASEGEN_MAZE_SIGNATURES,
    ROLLOUT_STREAM_TRACE_SIGNATURES, ROLLOUT_TEAM_STREAM_SIGNATURES, TRAIN_B3_SIGNATURES and ROLLOUT_SUMMARY_SIGNATURES;
    returns the library."""
    optional = [item for item in MEASURE_SIGNATURES.items() if hasattr(library, item[0])]
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(MAPF_DISTANCE_SIGNATURES.items()) + \
            list(CASEGEN_SIGNATURES.items()) + list(MAPF_AUDIT_SIGNATURES.items()) + \
            list(ROLLOUT_TRACE_SIGNATURES.items()) + list(SCHEDULE_DRAW_SIGNATURES.items()) + \
            list(ROLLOUT_STREAM_SIGNATURES.items()) + list(CASEGEN_MAZE_SIGNATURES.items()) + \
            list(ROLLOUT_STREAM_TRACE_SIGNATURES.items()) + list(ROLLOUT_TEAM_STREAM_SIGNATURES.items()) + \
            list(TRAIN_B3_SIGNATURES.items()) + list(ROLLOUT_SUMMARY_SIGNATURES.items()) + optional:
        f = getattr(library, name)                           # (a missing export raises here, at load time)
        f.restype, f.argtypes = restype, argtypes
    return library


_lib = None
_measure_lib = None


def lib():
    """The loaded library; raises loudly when it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GnnppError(
            'libgnnpp.so is missing (%s). Build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` (hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
    _lib = bind(ctypes.CDLL(LIB_PATH))
    _apply_toolchain_policy(_lib)
    return _lib


def built_with():
    """First line of `hipcc --version` of the compiler that built libgnnpp.so (libgnnpp.so.toolchain), or None when the
    library came without its stamp (then it is treated as the validated build: the stamp travels with the library)."""
    try:
        return open(TOOLCHAIN_STAMP).read().strip() or None
    except OSError:
        return None


def _apply_toolchain_policy(L):
    ver = built_with()
    if ver is None or ver == VALIDATED_HIPCC or os.environ.get('GNNPP_TRUST_TOOLCHAIN') == '1':
        return
    import warnings
    warnings.warn('libgnnpp.so was built by %r, the asm-scheduled column-packed layers were validated with %r: using the '
                  'compiler-scheduled forms (GNNPP_TUNE_POLICY_CP = 0, GNNPP_TUNE_ENCODER_CP_TILE = 16; same results). Run '
                  '`pytest -m gpu -k column_packed` and set GNNPP_TRUST_TOOLCHAIN=1 (or update _native.VALIDATED_HIPCC) '
                  'to re-enable them.' % (ver, VALIDATED_HIPCC))
    L.gnnpp_set_tuning(TUNE_POLICY_CP, 0)
    L.gnnpp_set_tuning(TUNE_ENCODER_CP_TILE, 16)


def measure_lib():
    """libgnnpp_measure.so (-DGNNPP_MEASURE: phase-ablation / early-exit knobs of csrc/gnnpp_measure.h).
    Profiling tools only -- results under those knobs are wrong by construction; the package's
    modules never load it."""
    global _measure_lib
    if _measure_lib is None:
        _measure_lib = bind(ctypes.CDLL(build(measure=True)))
    return _measure_lib


def check(rc, what):
    if rc != 0:
        raise GnnppError('%s failed: %s (code %d)' % (what, lib().gnnpp_error_string(rc).decode(), rc))


def gemm_kmajor(A, a_strides, Bm, b_strides, C, c_strides, batch, M, N, K):
    """C_b(m,n) = sum_k A_b(m,k) B_b(k,n) on gnnpp_gemm_kmajor (split-K fp32 MFMA, deterministic).
    a_strides = (batch, m, k), b_strides = (batch, k) [n contiguous], c_strides = (batch, m) [n contiguous],
    in floats; A, Bm, C are fp32 device tensors that own the addressed storage."""
    import torch
    dev = require_gpu(A, Bm, C)
    L = lib()
    nws = L.gnnpp_gemm_workspace_floats(batch, M, N, K)
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)
    with device_guard(dev):
        check(L.gnnpp_gemm_kmajor(A.data_ptr(), a_strides[0], a_strides[1], a_strides[2], Bm.data_ptr(),
                                  b_strides[0], b_strides[1], C.data_ptr(), c_strides[0], c_strides[1],
                                  batch, M, N, K, ws.data_ptr(), stream_ptr(dev)), 'gnnpp_gemm_kmajor')
    return C


def gemm_kmajor_multi(specs):
    """Several gemm_kmajor products in one launch (gnnpp_gemm_kmajor_multi).  specs: list of tuples
    (A, a_strides, Bm, b_strides, C, c_strides, batch, M, N, K[, mask]) as for gemm_kmajor (at most 8); mask: a
    tensor laid out like C -- C is stored as 0 where mask <= 0 (a ReLU backward folded into the product)."""
    import torch
    dev = require_gpu(*[t for s in specs for t in (s[0], s[2], s[4])])
    L = lib()
    arr = (GemmDesc * len(specs))()
    for d, sp in zip(arr, specs):
        A, a_st, Bm, b_st, C, c_st, batch, M, N, K = sp[:10]
        d.A, d.a_sb, d.a_sm, d.a_sk = A.data_ptr(), a_st[0], a_st[1], a_st[2]
        d.B, d.b_sb, d.b_sk = Bm.data_ptr(), b_st[0], b_st[1]
        d.C, d.c_sb, d.c_sm = C.data_ptr(), c_st[0], c_st[1]
        d.batch, d.M, d.N, d.K = batch, M, N, K
        d.mask = sp[10].data_ptr() if len(sp) > 10 and sp[10] is not None else None
    ws = torch.empty(max(L.gnnpp_gemm_multi_workspace_floats(arr, len(specs)), 1), dtype=torch.float32, device=dev)
    with device_guard(dev):
        check(L.gnnpp_gemm_kmajor_multi(arr, len(specs), ws.data_ptr(), stream_ptr(dev)), 'gnnpp_gemm_kmajor_multi')


# ---- parameter-gradient products that can wait for the end of the backward pass ---------------------------------------
# The backward pass of the planner's training step is a CHAIN of launches (each needs the gradient the one before
# produced), and at the reference's batch every launch is mostly latency.  The products that only yield PARAMETER
# gradients (dW, db of the two Linear layers, the filter's tap / bias gradient) are not on that chain: nothing needs them
# before the optimizer.  They are queued here and launched together with the next product that IS needed -- the compress
# layer's backward launch flushes the queue into its own gemm_kmajor_multi call -- so three multiply + three reduce launches
# become one of each.  A queued product's OUTPUT tensor has already been handed to autograd (which only stores it: the
# callers queue a product only while the parameter has no `.grad` yet, so nothing reads it early), and the autograd engine
# runs flush_deferred_gemms as a final callback of the pass, which covers passes that never reach the flushing node.
_deferred_gemms = []
_defer_depth = 0


class allow_deferred_gemms:
    """Deferral is OPT-IN per backward pass: training.train_step (and with it GraphedTrainStep) runs its backward inside
    this context.  A plain `loss.backward()` of a caller of the reference API computes every gradient inside the node
    that returns it, as autograd's contract says.  Inside the context hooks are honoured too: a tensor hook or a
    post-accumulate-grad hook on a parameter READS the gradient the moment the node has returned it (and a tensor hook
    may replace it), so a node whose parameters carry one -- or have a `.grad` already, or run under anomaly detection --
    computes its products at once (may_defer, decided per node); only the other nodes' products wait."""

    def __enter__(self):
        global _defer_depth
        _defer_depth += 1

    def __exit__(self, *exc):
        global _defer_depth
        _defer_depth -= 1
        if _deferred_gemms:                               # (a pass that raised half-way: nothing may stay queued)
            if exc[0] is None:
                flush_deferred_gemms()
            else:
                del _deferred_gemms[:]
        return False


def deferral_allowed():
    return _defer_depth > 0


def may_defer(*params):
    """May the products that yield the gradients of `params` (None entries are skipped) wait in the queue?  Only inside
    allow_deferred_gemms, and only when nothing can read or replace the gradient before the flush: every parameter is a
    leaf without a `.grad` (autograd then only stores the tensor it is handed) and without tensor hooks or
    post-accumulate-grad hooks (both run the moment the node returns, on a buffer the queue has not filled yet, and a
    hook's returned gradient would be overwritten at flush time); anomaly detection reads every gradient for NaNs as
    well.  Decided per backward node: a hook on one layer costs that layer's deferral only."""
    import torch
    if _defer_depth <= 0 or torch.is_anomaly_enabled():
        return False
    for p in params:
        if p is None:
            continue
        if (not p.is_leaf or p.grad is not None or p._backward_hooks
                or getattr(p, '_post_accumulate_grad_hooks', None)):
            return False
    return True


def defer_gemms(specs, params):
    """Queue gemm_kmajor specs (tuples as for gemm_kmajor_multi; they keep their INPUT tensors alive) until
    flush_deferred_gemms / the end of the running backward pass.  params[i] = the parameter whose gradient spec i
    computes.  The OUTPUT tensor of a spec is held WEAKLY: autograd adopts a gradient as `.grad` without a copy only
    when nobody else references it (AccumulateGrad's use-count test), so a strong reference from this queue would make
    it clone the still-uncomputed buffer.  At flush time the product is written to the tensor that then IS the gradient:
    the one handed to autograd if it is still alive (adopted as `.grad`, or captured by torch.autograd.grad), else the
    parameter's `.grad` (autograd cloned after all)."""
    import weakref
    if not specs:
        return
    if not _deferred_gemms:
        from torch.autograd import Variable
        Variable._execution_engine.queue_callback(flush_deferred_gemms)     # safety net: end of THIS backward pass
    for sp, prm in zip(specs, params):
        _deferred_gemms.append((sp[:4], weakref.ref(sp[4]), tuple(sp[4].shape), sp[5:], prm))


def flush_deferred_gemms(extra=()):
    """Launch every queued product (+ `extra`, the caller's own) in as few gemm_kmajor_multi calls as 8 products each allow."""
    specs = []
    for head, ref, shape, tail, prm in _deferred_gemms:
        out = ref()
        if out is None:
            out = prm.grad                                # (autograd cloned the gradient: the clone is the gradient now)
        if out is None or tuple(out.shape) != shape or not out.is_contiguous():
            continue                                      # nobody holds the result any more
        specs.append(head + (out,) + tail)
    del _deferred_gemms[:]
    specs += list(extra)
    for i in range(0, len(specs), 8):
        gemm_kmajor_multi(specs[i:i + 8])


def require_gpu(*tensors):
    """Every tensor must live on one HIP device; returns that device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise GnnppError('gnn_pathplanning_amd runs on MI355X only: got a %s tensor; move the '
                             'module and its inputs to a HIP device (there is no CPU fallback)'
                             % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise GnnppError('tensors on different devices: %s vs %s' % (dev, t.device))
    return dev


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device):
    """hipStream_t of torch's current stream on `device` (the raw-handle query when this torch has it: building a
    torch.cuda.Stream object per launch costs ~4 us of host time)."""
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class device_guard:
    """Make `device` current for raw HIP launches (no-op in the one-process-per-GPU layout)."""

    def __init__(self, device):
        self.dev = device
        self.ctx = None

    def __enter__(self):
        if torch.cuda.current_device() != self.dev.index:
            self.ctx = torch.cuda.device(self.dev)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# ---- gradient sinks: where the backward kernels write d loss / d parameter --------------------------------------
# training.FlatBucketDP registers every parameter's slice of its ONE flat gradient bucket here; the autograd Functions
# of this package (encoder, Linear, graph filter) ask grad_out() for the tensor a parameter's gradient is written to,
# so the gradients of a step are BORN inside the bucket and the data-parallel exchange is one all-reduce + one scale
# (the exchange used to pack / unpack with 2 x 26 copy launches around the one collective).
_grad_sinks = {}            # parameter data_ptr -> [weakref to the parameter, bucket, offset in elements, weakref to
                            # the view handed out last]


def register_grad_sink(param, bucket, offset):
    import weakref
    _grad_sinks[param.data_ptr()] = [weakref.ref(param), bucket, int(offset), None]


def unregister_grad_sinks(bucket):
    for k in [k for k, e in _grad_sinks.items() if e[1] is bucket]:
        del _grad_sinks[k]


_sinks_bypassed = 0


class no_grad_sinks:
    """Inside this context grad_out() always returns fresh memory.  ops.lsigf_backward runs in it: a registered custom
    op declared with mutates_args=() must return tensors nobody else can write to, never a view of a live gradient
    bucket."""

    def __enter__(self):
        global _sinks_bypassed
        _sinks_bypassed += 1

    def __exit__(self, *exc):
        global _sinks_bypassed
        _sinks_bypassed -= 1
        return False


def grad_out(param_ptr, shape, device):
    """The tensor a backward kernel writes the gradient of the parameter stored at `param_ptr` into: a FRESH view of
    the registered bucket slice when the parameter has no gradient yet (autograd then adopts that view as `.grad` --
    a new tensor object nobody else references -- without a copy), else a new tensor (an existing `.grad` -- kept by
    zero_grad(set_to_none=False), or a second backward of an accumulation step -- is added to in place by autograd:
    handing out its own memory would double it).  The slice is handed out ONCE at a time: while the
    view of an earlier request is still alive and not yet adopted -- a parameter consumed by two backward nodes of one
    pass (shared weights, a module called twice before one backward), or two torch.autograd.grad() calls -- a second
    request gets fresh memory, so the second kernel cannot overwrite the first one's result before autograd adds
    them."""
    import weakref
    e = _grad_sinks.get(param_ptr) if not _sinks_bypassed else None
    if e is not None:
        p = e[0]()
        if p is None or p.data_ptr() != param_ptr:
            del _grad_sinks[param_ptr]                       # the parameter died / moved: a stale entry
        elif (p.grad is None and (e[3] is None or e[3]() is None) and tuple(p.shape) == tuple(shape)
              and p.dtype is torch.float32 and e[1].device == device):
            n = p.numel()
            v = e[1][e[2]:e[2] + n].view(shape)
            e[3] = weakref.ref(v)
            return v
    return torch.empty(shape, dtype=torch.float32, device=device)


_pack_generation = 0


def invalidate_packs():
    """Force every PackCache to rebuild on its next use.  Needed after parameter updates that
    torch's version counters do not see: a HIP-graph replay of an optimizer step
    (training.GraphedTrainStep calls this), or in-place edits through `.data`."""
    global _pack_generation
    _pack_generation += 1


class PackCache:
    """Packed (MFMA-fragment-ordered) copy of some parameters, rebuilt when any of them changes
    (load_state_dict / optimizer step / .to()): keyed on (_version, id) of each tensor plus the
    process-wide generation counter of invalidate_packs()."""

    def __init__(self):
        self.key = None
        self.buf = None

    @staticmethod
    def key_of(tensors):
        """The key a pack of `tensors` built NOW would carry (no rebuild)."""
        # _version changes on every in-place update; id() changes when .to()/.cuda() replaces the
        # tensor objects' storage holders.  (data_ptr() per tensor is 3x slower than this.)
        return tuple([t._version for t in tensors] + [id(t) for t in tensors] +
                     [tensors[0].data_ptr(), tensors[-1].data_ptr(), _pack_generation])

    def get(self, tensors, pack_fn):
        key = self.key_of(tensors)
        if key != self.key:
            self.buf = pack_fn()
            self.key = key
        return self.buf
