"""Ground-truth maps of the datasets on the device (HIP kernel of csrc/morph.hip) -- the one batch entry the reference's loaders make with
OpenCV inside `Dataset.__getitem__` (maggie/dataloader/utils.py:5-35, him.py:185-196, vim.py:171-211):

  * `transition_gt`   image training: [dilate^n(alpha) > erode^n(alpha)] per instance, scattered into the `max_inst` slots;
  * `trimap`          evaluation: 2 where alpha > 0.5, then 1 in the transition band of a 25-wide ellipse;
  * `diff_transition` video training: the dilated union of the frame-to-frame alpha changes, frame 0 all ones, one plane for every slot;
  * `dilate` / `erode` the grey-scale filters themselves (cv2.dilate / cv2.erode with the MORPH_ELLIPSE element, default anchor and border).

Everything is decided in the uint8 domain (`v / 255` is strictly increasing, so `dilate - erode > 0` and `alpha > 0.5` are `dilate > erode`
and `v >= 128`): the results are bit-exact, no tolerance anywhere. The random draws (`k_size`, `iterations`, `slot_ids`) stay with the caller.

Supported: 1 <= k_size <= 31, iterations >= 1 and iterations * (k_size - 1) <= MAX_HALO = 48 per frame (k <= 4 with up to 16 passes, k = 5 with
up to 12, any k <= 31 with one pass): the halo of a tile that runs all passes out of LDS. Anything else raises before a launch."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import check_u8, resolve_device, to_device

MAX_K = 31                      # the ellipse span table of csrc/se_table.h
MAX_HALO = 48                   # MG_MORPH_MAX_HALO (include/maggie_hip.h)
MODE_TRANSITION, MODE_TRIMAP = 0, 1          # MG_GT_*
_PREPARED = set()               # device indices whose span table is uploaded


def _per_frame(v, frames, what):
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return [int(v)] * frames
    if isinstance(v, (bool, float, str)) or v is None:
        raise TypeError('%s must be an int or one int per frame (got %r)' % (what, v))
    vs = list(v.tolist() if hasattr(v, 'tolist') else v)
    if len(vs) != frames:
        raise ValueError('%s: one int per frame needs %d entries (got %d)' % (what, frames, len(vs)))
    for e in vs:
        if not isinstance(e, (int, np.integer)) or isinstance(e, bool):
            raise TypeError('%s must hold ints (got %r)' % (what, e))
    return [int(e) for e in vs]


def kn_table(k_size, iterations, frames):
    """The per-frame (k, n) table as a (frames, 2) int32 array and the halo bound it needs; raises on anything the kernel does not support."""
    ks = _per_frame(k_size, frames, 'k_size')
    ns = _per_frame(iterations, frames, 'iterations')
    halo = 0
    for k, n in zip(ks, ns):
        if k < 1 or k > MAX_K:
            raise ValueError('k_size must be in 1..%d (got %d)' % (MAX_K, k))
        if n < 1:
            raise ValueError('iterations must be >= 1 (got %d)' % n)
        if n * (k - 1) > MAX_HALO:
            raise ValueError('iterations * (k_size - 1) must be <= %d (got %d passes of k_size %d)' % (MAX_HALO, n, k))
        halo = max(halo, n * (k - 1))
    return np.asarray(list(zip(ks, ns)), np.int32).reshape(frames, 2), halo


class Draws:
    """A (k, n) table that already lives on the device: `kn` int32 (frames, 2) and the halo bound `halo` it was sized for. Pass it as `k_size`
    (then `iterations` is not read). Nothing is uploaded in a call that gets one, so the call can be captured in a graph; new draws are
    written into `kn` between replays, and must stay within `halo` (the kernel clamps a frame that does not)."""

    def __init__(self, kn, halo):
        self.kn, self.halo = kn, int(halo)


def _prepare(device):
    if device.index not in _PREPARED:
        with torch.cuda.device(device):
            hip.check(hip.lib().mg_morph_prepare(), 'mg_morph_prepare')
        _PREPARED.add(device.index)


def draws(k_size, iterations, frames, halo=None, device=None):
    """Check and upload the per-frame draws once; `halo`: a larger bound to leave room for later draws (default: what these need)."""
    kn, need = kn_table(k_size, iterations, frames)
    halo = need if halo is None else int(halo)
    if halo < need or halo > MAX_HALO:
        raise ValueError('halo must be in %d..%d (got %d)' % (need, MAX_HALO, halo))
    device = resolve_device(device)
    _prepare(device)
    return Draws(torch.from_numpy(kn).to(device), halo)


def _check_draws(k_size, iterations, frames):
    """Argument errors, before anything touches the device."""
    if isinstance(k_size, Draws):
        if tuple(k_size.kn.shape) != (frames, 2) or k_size.kn.dtype != torch.int32:
            raise ValueError('Draws.kn must be int32 of shape (%d, 2) (got %s %s)' % (frames, k_size.kn.dtype, tuple(k_size.kn.shape)))
        if not 0 <= k_size.halo <= MAX_HALO:
            raise ValueError('Draws.halo must be in 0..%d' % MAX_HALO)
    else:
        kn_table(k_size, iterations, frames)


def _device_inputs(x, k_size, iterations, frames, device):
    """The planes and the (k, n) table on the device; without a GPU, the error of `to_device`."""
    x = to_device(x, device)
    if isinstance(k_size, Draws):
        hip.need_cuda(k_size.kn)
        return x, k_size.kn.contiguous(), k_size.halo
    _prepare(x.device)
    kn, halo = kn_table(k_size, iterations, frames)
    return x, torch.from_numpy(kn).to(x.device, non_blocking=True), halo


def _morph(planes_u8, k, iterations, want_dil, want_ero, device):
    x = check_u8(planes_u8)
    if x.dim() < 2:
        raise ValueError('expected (..., H, W) planes (got shape %s)' % (tuple(x.shape),))
    shape = tuple(x.shape)
    H, W = shape[-2:]
    frames = shape[0] if x.dim() >= 3 else 1
    per_frame = int(np.prod(shape[1:-2])) if x.dim() > 3 else 1
    _check_draws(k, iterations, frames)
    x, kn, halo = _device_inputs(x, k, iterations, frames, device)
    dil = torch.empty(shape, dtype=torch.uint8, device=x.device) if want_dil else None
    ero = torch.empty(shape, dtype=torch.uint8, device=x.device) if want_ero else None
    if x.numel() > 0:
        hip.call('mg_morph_u8', hip.ptr(x), hip.ptr(dil), hip.ptr(ero), hip.ptr(kn), c_int(halo), c_long(frames * per_frame), c_int(per_frame),
                 c_int(H), c_int(W), hip.stream())
    return dil, ero


def dilate(planes_u8, k, iterations=1, device=None):
    """cv2.dilate(plane, getStructuringElement(MORPH_ELLIPSE, (k, k)), iterations=iterations) of every (H, W) plane of a (H, W), (F, H, W) or
    (F, ..., H, W) uint8 tensor; `k` / `iterations`: an int, or one int per frame (the leading dimension)."""
    return _morph(planes_u8, k, iterations, True, False, device)[0]


def erode(planes_u8, k, iterations=1, device=None):
    """cv2.erode, as `dilate`."""
    return _morph(planes_u8, k, iterations, False, True, device)[1]


def dilate_erode(planes_u8, k, iterations=1, device=None):
    """Both filters from one read of the planes."""
    return _morph(planes_u8, k, iterations, True, True, device)


def _slot_table(n_i, n_slots, slot_ids, frames):
    if slot_ids is None:
        if n_slots is not None and int(n_slots) != n_i:
            raise ValueError('n_slots != n_i needs slot_ids')
        return n_i, None
    n_slots = n_i if n_slots is None else int(n_slots)
    ids = [int(i) for i in slot_ids]
    if len(ids) != n_i or len(set(ids)) != n_i or (n_i and (min(ids) < 0 or max(ids) >= n_slots)):
        raise ValueError('slot_ids must name %d distinct slots below %d' % (n_i, n_slots))
    src = np.full((n_slots,), -1, np.int32)
    src[ids] = np.arange(n_i, dtype=np.int32)
    return n_slots, np.tile(src, frames)


def _frames4(alphas_u8):
    x = check_u8(alphas_u8)
    if x.dim() != 4:
        raise ValueError('expected (T, n_i, H, W) planes (got shape %s)' % (tuple(x.shape),))
    return x


def transition_gt(alphas_u8, k_size=25, iterations=1, thresh=0, n_slots=None, slot_ids=None, device=None, _mode=MODE_TRANSITION):
    """(T, n_i, H, W) uint8 alphas -> (T, n_slots, H, W) fp32 in {0, 1}: gen_transition_gt (maggie/dataloader/utils.py:15-35) as the datasets call
    it -- `(dilate - erode) > 0` of every instance plane, values below `thresh` read as 0 (5 in training: transforms.py:744), plane j written to
    slot slot_ids[j] (`chosen_ids`, him.py:161-165), other slots exactly 0. The defaults are the evaluation call (k = 25, one pass)."""
    x = _frames4(alphas_u8)
    T, n_i, H, W = x.shape
    n_slots, table = _slot_table(n_i, n_slots, slot_ids, T)
    _check_draws(k_size, iterations, T)
    x, kn, halo = _device_inputs(x, k_size, iterations, T, device)
    out = torch.empty((T, n_slots, H, W), dtype=torch.float32, device=x.device)
    if n_i == 0:
        return out.zero_()
    if out.numel() > 0:
        tab = None if table is None else torch.from_numpy(table).to(x.device, non_blocking=True)
        hip.call('mg_transition_gt', hip.ptr(x), hip.ptr(out), hip.ptr(tab), hip.ptr(kn), c_int(halo), c_int(T), c_int(n_i), c_int(n_slots),
                 c_int(H), c_int(W), c_int(int(thresh)), c_int(_mode), hip.stream())
    return out


def trimap(alphas_u8, device=None):
    """(T, n_i, H, W) uint8 `ori_alphas` -> (T, n_i, H, W) fp32 in {0, 1, 2} (him.py:190-196, vim.py:198-203): 2 where alpha > 0.5 (v >= 128),
    then 1 where the 25-wide ellipse's dilation and erosion differ."""
    return transition_gt(alphas_u8, 25, 1, 0, None, None, device, _mode=MODE_TRIMAP)


def diff_transition(alphas_u8, k_size, iterations, thresh=5, n_slots=None, diff_thresh=5, device=None):
    """(T, n_i, H, W) uint8 alphas of a clip -> (T, n_slots, H, W) fp32 in {0, 1} (vim.py:171-183,211): frame 0 all ones; frame t >= 1 the
    n-pass dilation of the union over instances of |a_t - a_{t-1}| > diff_thresh (values below `thresh` read as 0 first), the same plane in
    every slot -- the padded ones included (n_slots: `max_inst`; default n_i). A per-frame `k_size` / `iterations` has T entries; entry 0 is
    not used."""
    x = _frames4(alphas_u8)
    T, n_i, H, W = x.shape
    n_slots = n_i if n_slots is None else int(n_slots)
    if n_slots < n_i:
        raise ValueError('n_slots (%d) must be >= the number of instances (%d)' % (n_slots, n_i))
    _check_draws(k_size, iterations, T)
    x, kn, halo = _device_inputs(x, k_size, iterations, T, device)
    out = torch.empty((T, n_slots, H, W), dtype=torch.float32, device=x.device)
    if n_i == 0:
        out.zero_()
        out[:1] = 1
        return out
    if out.numel() > 0:
        hip.call('mg_diff_transition', hip.ptr(x), hip.ptr(out), hip.ptr(kn), c_int(halo), c_int(T), c_int(n_i), c_int(n_slots), c_int(H), c_int(W),
                 c_int(int(thresh)), c_int(int(diff_thresh)), hip.stream())
    return out
