"""Dense Farneback optical flow on the device (HIP kernels of csrc/flow.hip): what the reference's MESSDdt gets from
`cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 10, 2, 7, 1.5, cv2.OPTFLOW_FARNEBACK_GAUSSIAN)` (maggie/utils/metric.py:453-455),
for P plane pairs of one size in one set of launches. Only these parameters are built; the C side rejects any other.

The algorithm is Farneback 2003 as OpenCV structures it, restated from the published method (tests/flow_restatement.py); it is NOT compared
with cv2.calcOpticalFlowFarneback, which is not part of this build. DESIGN.md section 23 lists what is taken on trust."""
import torch

from .. import hip
from ..hip import c_int, c_long
from . import _inputs

PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, FLAGS = 0.5, 5, 10, 2, 7, 1.5, 256        # FLAGS: cv2.OPTFLOW_FARNEBACK_GAUSSIAN
MIN_SIZE = 32
MAX_SIDE = 32767                                 # MG_FLOW_MAX_SIDE
MAX_PAIRS = 32767                                # both frames of every pair ride in one grid dimension


def levels_of(h, w):
    """Pyramid levels below full size: halve up to LEVELS times while both sides stay >= MIN_SIZE (so there are levels_of + 1 scales)."""
    scale, k = 1.0, 0
    while k < LEVELS:
        scale *= PYR_SCALE
        if w * scale < MIN_SIZE or h * scale < MIN_SIZE:
            break
        k += 1
    return k


def level_size(h, w, k):
    """(rows, columns) of level k: the scaled size rounded half to even."""
    scale = PYR_SCALE ** k
    return int(round(h * scale)), int(round(w * scale))


def check_shape(P, H, W):
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise hip.MaggieHipError('the flow needs planes of 1 .. %d pixels a side (got %d x %d)' % (MAX_SIDE, H, W))
    if P > MAX_PAIRS:
        raise hip.MaggieHipError('the flow takes at most %d plane pairs a call (got %d)' % (MAX_PAIRS, P))


def scratch_bytes(P, H, W):
    """Bytes of device scratch one call of mg_flow_farneback needs for P pairs of H x W (26 fp32 values per pixel pair)."""
    check_shape(P, H, W)
    n = hip.ctypes.c_long(0)
    hip.check(hip.lib().mg_flow_scratch_bytes(c_long(P), c_int(H), c_int(W), hip.ctypes.byref(n)), 'mg_flow_scratch_bytes')
    return int(n.value)


def scratch(P, H, W, device):
    return torch.empty(max(scratch_bytes(P, H, W), 1), dtype=torch.uint8, device=device)


def farneback(prev_u8, next_u8, device=None, pyr_scale=PYR_SCALE, levels=LEVELS, winsize=WINSIZE, iterations=ITERATIONS, poly_n=POLY_N,
              poly_sigma=POLY_SIGMA, flags=FLAGS):
    """uint8 (..., H, W) planes (tensors or arrays, host or device) -> fp32 device tensor (P, H, W, 2), P the product of the leading dimensions:
    [..., 0] is the displacement along columns (x), [..., 1] along rows (y), with next(p + flow) ~ prev(p)."""
    prev, lead, P, H, W = _inputs.images(prev_u8, 1, 'farneback')
    nxt, lead2, P2, H2, W2 = _inputs.images(next_u8, 1, 'farneback')
    if (lead, H, W) != (lead2, H2, W2):
        raise ValueError('farneback: the two stacks differ in shape (%s and %s)' % (tuple(prev.shape), tuple(nxt.shape)))
    check_shape(P, H, W)
    prev = _inputs.to_device(prev, device)
    nxt = _inputs.to_device(nxt, prev.device)
    out = torch.empty((P, H, W, 2), dtype=torch.float32, device=prev.device)
    if P == 0:
        return out
    ws = scratch(P, H, W, prev.device)
    hip.call('mg_flow_farneback', hip.ptr(prev), hip.ptr(nxt), c_long(P), c_int(H), c_int(W), hip.ctypes.c_double(pyr_scale), c_int(levels),
             c_int(winsize), c_int(iterations), c_int(poly_n), hip.ctypes.c_double(poly_sigma), c_int(flags), hip.ptr(ws), hip.ptr(out),
             hip.stream())
    return out


def messddt_scratch(F, N, H, W, device):
    """Device scratch of one mg_metric_messddt call on (F, N, H, W) planes (a byte tensor; the C side carves it)."""
    check_shape(max(F - 1, 0) * N, H, W)
    n = hip.ctypes.c_long(0)
    hip.check(hip.lib().mg_messddt_scratch_bytes(c_int(F), c_int(N), c_int(H), c_int(W), hip.ctypes.byref(n)), 'mg_messddt_scratch_bytes')
    return torch.empty(max(int(n.value), 1), dtype=torch.uint8, device=device)
