"""MAPF cases generated on the device: the step ahead of the expert and of the rollout.

    casegen.generate (this module) -> mapf.distances / mapf.solve / mapf.solve_team -> expert.samples_from_solutions
                                    -> BatchedRollout

The reference draws its cases on the host (offlineExpert/CasesGenerator.py): a random map, a flood fill that leaves one
connected free region (img_fill), start and goal pairs from the free space without duplicates.  gnnpp_casegen
(include/gnnpp_casegen.h, csrc/casegen_kernels.hip) states that generator as a contract on counter hashes -- a case
depends on (seed, case index) alone -- and runs one workgroup per case: the hashed map (or the caller's own), its largest
4-connected free component, N distinct starts and N distinct goals of that component, no agent on its own goal.  Every
agent of a generated case has a path.  The reference's maze-style generator (mapGen: sequential random walks) is not
restated.  There is no CPU fallback.  Positions are (row, col) integers.
"""
import numpy as np
import torch

from . import _native

MAX_TEAM, MAX_SIDE = _native.ROLLOUT_MAX_TEAM, _native.MAPF_TEAM_MAX_SIDE
OK, TOO_SMALL = _native.CASEGEN_OK, _native.CASEGEN_TOO_SMALL


def threshold_of(density):
    """The obstacle threshold of a density in 0 .. 1: a cell is an obstacle iff its 32-bit hash is below it."""
    return min(int(density * 2 ** 32), 2 ** 32 - 1)


class Cases:
    """Device tensors of one generate call: grid [C,H,W] uint8 (1 = obstacle; the closed map), start, goal [C,N,2] int32
    (row, col), cells [C] int32 (the size of the free region), status [C] int32 (OK, or TOO_SMALL: the region holds
    fewer than max(N, 2) cells, and the case's starts and goals are -1).  grid, start and goal go as they are to
    mapf.distances, mapf.solve, mapf.solve_team and BatchedRollout."""

    def __init__(self, grid, start, goal, cells, status):
        self.grid, self.start, self.goal, self.cells, self.status = grid, start, goal, cells, status

    def __len__(self):
        return int(self.status.shape[0])

    @property
    def ok(self):
        """bool [C] on the device."""
        return self.status == OK

    def yaml(self, c):
        """Case c as the reference's solver input (map dimensions, obstacles, agents with start and goal): the text of
        expert.failure_case_yaml."""
        from . import expert
        if int(self.status[c]) != OK:
            raise _native.GnnppError('case %d is too small: its free region holds %d cells for %d agents'
                                     % (c, int(self.cells[c]), int(self.start.shape[1])))
        return expert.failure_case_yaml(self.grid[c].cpu().numpy(), self.start[c].cpu().numpy(),
                                        self.goal[c].cpu().numpy())


def _check_shape(C, N, H, W):
    C, N, H, W = int(C), int(N), int(H), int(W)
    if C < 1 or not 1 <= N <= MAX_TEAM or C * N > 2 ** 31 - 1:
        raise _native.GnnppError('C >= 1 cases of 1 to %d agents, C * N < 2^31 (got C = %d, N = %d, maps of %d x %d)'
                                 % (MAX_TEAM, C, N, H, W))
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise _native.GnnppError('maps of 1 x 1 to %d x %d cells (got %d x %d, C = %d, N = %d)'
                                 % (MAX_SIDE, MAX_SIDE, H, W, C, N))
    return C, N, H, W


def empty_cases(C, N, H, W, device):
    """The output tensors of enqueue_generate for C cases of N agents on H x W maps."""
    C, N, H, W = _check_shape(C, N, H, W)
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('casegen needs a HIP device (no CPU fallback)')
    return Cases(torch.empty((C, H, W), dtype=torch.uint8, device=dev),
                 torch.empty((C, N, 2), dtype=torch.int32, device=dev), torch.empty((C, N, 2), dtype=torch.int32, device=dev),
                 torch.empty((C,), dtype=torch.int32, device=dev), torch.empty((C,), dtype=torch.int32, device=dev))


def enqueue_generate(out, density=0.1, seed=0, grids=None):
    """gnnpp_casegen alone, on torch's current stream of the tensors' device: one launch, no allocation, no host
    synchronisation, capturable in a HIP graph.  out: from empty_cases; grids: None (hashed maps of `density`) or the
    caller's own raw maps, a contiguous uint8 device tensor [C,H,W] or [H,W] (nonzero = obstacle; `density` is unused)."""
    dev = _native.require_gpu(out.grid, out.start, out.goal, out.cells, out.status, grids)
    C, H, W = (int(v) for v in out.grid.shape)
    N = int(out.start.shape[1])
    if grids is not None and (grids.dtype != torch.uint8 or not grids.is_contiguous() or tuple(grids.shape[-2:]) != (H, W)
                              or grids.dim() not in (2, 3) or (grids.dim() == 3 and grids.shape[0] != C)):
        raise _native.GnnppError('grids must be a contiguous uint8 tensor [%d,%d] or [%d,%d,%d] (got %s %s)'
                                 % (H, W, C, H, W, grids.dtype, tuple(grids.shape)))
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_casegen(
            grids.data_ptr() if grids is not None else None, int(grids is not None and grids.dim() == 3),
            threshold_of(density), int(seed) & 0xffffffff, C, N, H, W, out.grid.data_ptr(), out.start.data_ptr(),
            out.goal.data_ptr(), out.cells.data_ptr(), out.status.data_ptr(), _native.stream_ptr(dev)), 'gnnpp_casegen')


def generate(C, N, H, W, device, density=0.1, seed=0, grids=None):
    """C cases of N agents on H x W maps: hashed maps with obstacle density `density`, or, with grids ([C,H,W] or
    [H,W], host or device, nonzero = obstacle), cases drawn on the caller's own maps.  Every map is closed to its largest
    4-connected free component; a case whose component holds fewer than max(N, 2) cells is reported in .status
    (TOO_SMALL), never raised.  The same (seed, arguments) give the same bytes.  Returns Cases."""
    out = empty_cases(C, N, H, W, device)
    if not 0.0 <= float(density) <= 1.0:
        raise _native.GnnppError('density must be in 0 .. 1 (got %r)' % (density,))
    if grids is not None:
        g = grids if torch.is_tensor(grids) else torch.as_tensor(np.asarray(grids))
        if g.dim() not in (2, 3) or tuple(g.shape[-2:]) != (int(H), int(W)) or (g.dim() == 3 and g.shape[0] != int(C)):
            raise _native.GnnppError('grids must be [H,W] or [C,H,W] = [%d,%d,%d] (got %s)' % (C, H, W, tuple(g.shape)))
        grids = (g != 0).to(torch.uint8).contiguous().to(out.grid.device)
    _native.lib()
    enqueue_generate(out, density, seed, grids)
    out._keep = grids                                    # input of the enqueued launch
    return out
