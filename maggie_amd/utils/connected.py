"""Connected components on the device (HIP kernels of csrc/ccl.hip): `label` with skimage.measure.label's semantics, and the scratch
sizing shared by the largest-component users (metric.Conn, postprocessing.postprocess).

Every plane of a (..., H, W) tensor is labelled independently in one set of launches; nothing is read back to the host."""
import torch

from .. import hip
from ..hip import c_int

OP_LABEL, OP_CONN, OP_LARGEST = 0, 1, 2          # MG_CC_OP_* (include/maggie_hip.h)


def check_plane(H, W):
    if H * W >= (1 << 31) - 1:
        raise hip.MaggieHipError('connected components need H * W < 2^31 (got %d x %d)' % (H, W))


def scratch(op, P, H, W, device):
    """Device scratch for one call of mg_cc_label (OP_LABEL), mg_metric_conn (OP_CONN) or mg_postprocess_largest_cc (OP_LARGEST) on P
    planes of H x W (a byte tensor; the C side carves it)."""
    check_plane(H, W)
    n = hip.ctypes.c_long(0)
    hip.check(hip.lib().mg_cc_scratch_bytes(c_int(op), c_int(P), c_int(H), c_int(W), hip.ctypes.byref(n)), 'mg_cc_scratch_bytes')
    return torch.empty(max(int(n.value), 1), dtype=torch.uint8, device=device)


def label(mask, connectivity=2, return_num=False):
    """skimage.measure.label(mask, connectivity=connectivity, return_num=return_num) for every (H, W) plane of a (..., H, W) bool / uint8
    device tensor (non-zero = foreground). Returns int32 labels of the same shape: 1..num per plane in the raster order of each component's
    first pixel, background 0. connectivity 1: 4-neighbours, 2 (skimage's default in 2-D): 8-neighbours. With return_num, also an int32
    device tensor of shape (...) with the per-plane counts."""
    hip.need_cuda(mask)
    if connectivity not in (1, 2):
        raise hip.MaggieHipError('connectivity must be 1 or 2 for 2-D planes (got %r)' % (connectivity,))
    if mask.dim() < 2:
        raise hip.MaggieHipError('label needs (..., H, W) planes (got shape %s)' % (tuple(mask.shape),))
    shape = tuple(mask.shape)
    H, W = shape[-2:]
    check_plane(H, W)
    if mask.dtype == torch.bool:
        m = mask.contiguous().view(torch.uint8)
    elif mask.dtype == torch.uint8:
        m = mask.contiguous()
    else:
        m = (mask != 0).contiguous().view(torch.uint8)
    m = m.reshape(-1, H, W)
    P = m.shape[0]
    labels = torch.empty((P, H, W), dtype=torch.int32, device=mask.device)
    num = torch.empty(P, dtype=torch.int32, device=mask.device)
    if P > 0:
        ws = scratch(OP_LABEL, P, H, W, mask.device)
        hip.call('mg_cc_label', hip.ptr(m), c_int(P), c_int(H), c_int(W), c_int(connectivity), hip.ptr(labels), hip.ptr(num), hip.ptr(ws),
                 hip.stream())
    labels = labels.reshape(shape)
    if return_num:
        return labels, num.reshape(shape[:-2])
    return labels
