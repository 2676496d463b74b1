"""The contract the device stages of the input side share (groundtruth, maskgen, geometry, crop, affine, photometric, preprocess): what a
stage checks about its uint8 input, where its work runs, and how a table of draws reaches the device. DESIGN.md section 20 states it.

  * pixels arrive as uint8, a torch tensor or a NumPy array, on the host or on the device (`check_u8`, `images`);
  * `device=None` means the device of a CUDA input, else the current device; 'cuda' without an index is the current device
    (`resolve_device`, `to_device`);
  * a table of draws is a NumPy array (uploaded by the call) or a device tensor (taken as it is: nothing is uploaded and nothing
    synchronises, so the call can be captured in a graph) (`int_table`, `lut_table`, `upload`);
  * argument errors are raised before anything touches the device, and without a GPU the error is `hip.MaggieHipError`, never torch's."""
import numpy as np
import torch

from .. import hip

IMAGENET_MEAN = (0.485, 0.456, 0.406)        # maggie/dataloader/him.py: T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
IMAGENET_STD = (0.229, 0.224, 0.225)


def check_u8(x, what='planes'):
    """A uint8 tensor or array -> the tensor (an array becomes a contiguous host tensor); `what` is the word the caller's message uses."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise TypeError('expected uint8 %s, got %s' % (what, x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise TypeError('expected a uint8 tensor or array, got %s' % type(x).__name__)
    if x.dtype != torch.uint8:
        raise TypeError('expected uint8 %s, got %s' % (what, x.dtype))
    return x


def integer(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError('%s must be an int (got %r)' % (what, v))
    return int(v)


def need_gpu(x):
    if not x.is_cuda and not torch.cuda.is_available():
        raise hip.MaggieHipError('MaGGIe HIP kernels need a GPU (got a CPU tensor and no device); there is no CPU fallback')


def resolve_device(device=None, like=None):
    """The device a stage runs on: `device`, or for None the device of `like` when that is a CUDA tensor, else the current device. A 'cuda'
    without an index is the current device."""
    if device is None and torch.is_tensor(like) and like.is_cuda:
        return like.device
    if not torch.cuda.is_available():
        raise hip.MaggieHipError('MaGGIe HIP kernels need a GPU; there is no CPU fallback')
    device = torch.device('cuda') if device is None else torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def to_device(x, device=None):
    """The tensor `x` contiguous on `resolve_device(device, x)`; no copy when it is there already."""
    need_gpu(x)
    x = x.to(resolve_device(device, x), non_blocking=True).contiguous()
    hip.need_cuda(x)
    return x


def upload(a, device):
    """A field of a Draws record on `device`: None stays None, a tensor stays a tensor, an array becomes a contiguous tensor."""
    if a is None:
        return None
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device, non_blocking=True)


def images(x_u8, channels, what):
    """uint8 (..., H, W) planes (channels 1) or (..., H, W, 3) frames (channels 3) -> the tensor, its leading shape, N, H, W."""
    x = check_u8(x_u8)
    need = 2 if channels == 1 else 3
    if x.dim() < need:
        raise ValueError('%s: expected %s (got shape %s)' % (what, '(..., H, W)' if channels == 1 else '(..., H, W, 3)', tuple(x.shape)))
    if channels == 3 and x.shape[-1] != 3:
        raise ValueError('%s: frames must have 3 channels (got shape %s)' % (what, tuple(x.shape)))
    lead = tuple(x.shape[:-need])
    H, W = (int(v) for v in x.shape[-need:][:2])
    if H < 1 or W < 1:
        raise ValueError('%s: the source must have at least one pixel (got %d x %d)' % (what, H, W))
    return x, lead, int(np.prod(lead)) if lead else 1, H, W


def int_table(t, device, n, what):
    """A draw table as a contiguous device int32 tensor of n entries (uploaded when it is an array)."""
    if torch.is_tensor(t):
        if t.dtype != torch.int32 or t.numel() != n:
            raise ValueError('%s must be int32 with %d entries (got %s %s)' % (what, n, t.dtype, tuple(t.shape)))
        hip.need_cuda(t)
        return t.contiguous()
    a = np.asarray(t)
    if a.size != n or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s must hold %d ints (got %s %s)' % (what, n, a.dtype, a.shape))
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device, non_blocking=True)


def lut_table(lut, device=None):
    """A (3, 256) uint8 tone curve (tensor, array or None), checked; with a `device` also uploaded and contiguous. The check comes first,
    so a caller validates with `lut_table(lut)` before anything touches the device."""
    if lut is None:
        return None
    a = lut if torch.is_tensor(lut) else np.asarray(lut)
    if a.dtype != (torch.uint8 if torch.is_tensor(a) else np.uint8) or tuple(a.shape) != (3, 256):
        raise ValueError('lut must be uint8 of shape (3, 256) (got %s %s)' % (a.dtype, tuple(a.shape)))
    return lut if device is None else upload(a, device).contiguous()


def float3(v):
    """Three floats (a mean or a std) as the C array a launch takes by value."""
    return (hip.ctypes.c_float * 3)(*v)
