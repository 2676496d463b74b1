"""Guidance masks of the training items on the device (HIP kernels of csrc/maskgen.hip) -- the chain the reference's loaders run with OpenCV
inside `Dataset.__getitem__` on every instance plane (maggie/dataloader/transforms.py:388-565, wired in him.py:50-59 and vim.py:58-69):

  GenMaskFromAlpha -> RandomBinarizedMask -> DownUpMask -> CutMask -> MaskDropout (video only)

  * `binarize_morph`  a per-plane threshold and a rectangular dilation and / or erosion (cv2.dilate / cv2.erode with np.ones((k, k)));
  * `down_up`         cv2.resize(INTER_LINEAR) by 1/8 and back, then `> 127`;
  * `cut`             rectangle copies inside a plane (CutMask.internal) or swaps between two planes (CutMask.external);
  * `stats` / `drop`  count and bounding box of the non-zero pixels, and MaskDropout's zeroed rectangle;
  * `synthesize`      the whole chain from one `MaskDraws`; `from_alpha` the evaluation form (GenMaskFromAlpha + DownUpMask(p=1)).

The draws stay on the host and are pure NumPy (`draw_chain`, `draw_dropout`: importable and testable without a GPU); they consume a
`np.random.RandomState` and Python's `random` module in exactly the reference's order. Everything on the device is integer work on uint8
planes: the results are bit-exact, no tolerance anywhere. A `MaskDraws` moved to the device (`.to(device)`) makes `synthesize` upload nothing
and never synchronise, so the call can be captured in a graph and new draws written into the tables between replays -- except the drop-out
branch, whose draws depend on the data (bounding box and pixel count of every plane): `synthesize` then reads the (P, 5) statistics back
once. That read-back is the only host synchronisation of the chain.

Supported: 1 <= k <= 31 (the reference draws k <= 29), 0 < ratio <= 1. Anything else raises before a launch. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import check_u8, resolve_device, to_device, upload

MAX_K = 31                       # MG_MASK_MAX_K (include/maggie_hip.h)
MAX_PATCH = 66                   # MG_MASK_MAX_PATCH: side of the small-image patch one 64-pixel tile may read
TILE = 64
ORDERS = ('dilate_erode', 'erode_dilate', 'dilate', 'erode')      # MG_MASK_DILATE_ERODE .. MG_MASK_ERODE, the order of transforms.py:412
ORDER_NONE = 4                   # MG_MASK_NONE: threshold only
COEF_ONE = 2048                  # OpenCV's INTER_RESIZE_COEF_SCALE
_TABLES = {}                     # (H, W, ratio) -> host tables
_DEVICE_TABLES = {}              # (H, W, ratio, device index) -> the uploaded table
_ALPHA_TABLES = {}               # (planes, device index) -> from_alpha's (P, 4) morph table and its flags, uploaded once


# ---- OpenCV's 8-bit bilinear resize: the host side ------------------------------------------------------------------------------------------
def resize_axis(src, dst, scale):
    """Taps and fixed-point coefficients of one axis of cv2.resize(INTER_LINEAR) on 8-bit data: destination index d reads source indices
    ofs[d] and ofs[d] + 1 (clamped to src - 1) with weights c0[d], c1[d] (int16, scaled by 2048). `scale` is the double OpenCV derives."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * np.float64(scale) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low = s < 0
    s[low], f[low] = 0, 0
    high = s >= src - 1
    s[high], f[high] = src - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(COEF_ONE)).astype(np.int16)
    c1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int16)
    return s, c0, c1


def resize_tables(H, W, ratio=0.125):
    """The tables of `down_up` for (H, W) planes, cached: cv2.resize(m, (0, 0), fx=ratio, fy=ratio) then cv2.resize(., (W, H)). Returns a dict
    with the small size `dh`, `dw`, the four axes `down_x`, `down_y`, `up_x`, `up_y` (each (ofs, c0, c1)) and `tab`, the int32 buffer the
    kernel reads. Raises ValueError when a rounded size is 0 or the ratio is not in (0, 1]."""
    H, W, ratio = int(H), int(W), float(ratio)
    key = (H, W, ratio)
    if key in _TABLES:
        return _TABLES[key]
    if H < 1 or W < 1:
        raise ValueError('planes must have at least one pixel (got %d x %d)' % (H, W))
    if not 0.0 < ratio <= 1.0:
        raise ValueError('ratio must be in (0, 1] (got %r)' % ratio)
    dw, dh = int(np.rint(W * ratio)), int(np.rint(H * ratio))           # saturate_cast<int>: round half to even
    if dw < 1 or dh < 1:
        raise ValueError('a %d x %d plane scaled by %r has a destination size of 0 (%d x %d)' % (H, W, ratio, dh, dw))
    t = {'dh': dh, 'dw': dw,
         'down_x': resize_axis(W, dw, 1.0 / ratio), 'down_y': resize_axis(H, dh, 1.0 / ratio),
         'up_x': resize_axis(dw, W, 1.0 / (W / dw)), 'up_y': resize_axis(dh, H, 1.0 / (H / dh))}
    for name, n_small in (('up_x', dw), ('up_y', dh)):                    # what the kernel's LDS patch holds
        ofs = t[name][0]
        for t0 in range(0, len(ofs), TILE):
            t1 = min(t0 + TILE, len(ofs))
            if min(ofs[t1 - 1] + 1, n_small - 1) - ofs[t0] + 1 > MAX_PATCH:
                raise ValueError('ratio %r: a %d-pixel tile reads more than %d pixels of the small image' % (ratio, TILE, MAX_PATCH))
    t['tab'] = np.concatenate([np.stack([a.astype(np.int32) for a in t[name]], 1).reshape(-1) for name in ('down_x', 'down_y', 'up_x', 'up_y')])
    _TABLES[key] = t
    return t


def _device_table(H, W, ratio, device):
    key = (int(H), int(W), float(ratio), device.index)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(resize_tables(H, W, ratio)['tab']).to(device)
    return _DEVICE_TABLES[key]


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------------
def _order_code(o):
    if isinstance(o, str):
        if o not in ORDERS:
            raise ValueError('order must be one of %s (got %r)' % (ORDERS, o))
        return ORDERS.index(o)
    if isinstance(o, (int, np.integer)) and not isinstance(o, bool) and 0 <= int(o) <= ORDER_NONE:
        return int(o)
    raise ValueError('order must be one of %s or its index (got %r)' % (ORDERS, o))


def _per_plane(v, P, what):
    if isinstance(v, (str, bool, int, float, np.bool_, np.integer, np.floating)):
        return [v] * P
    vs = list(v.tolist() if hasattr(v, 'tolist') else v)
    if len(vs) != P:
        raise ValueError('%s: one value per plane needs %d entries (got %d)' % (what, P, len(vs)))
    return vs


def morph_table(thresh, k_dilate, k_erode, order, n_planes):
    """The (P, 4) int32 table (floor(thresh), k_dilate, k_erode, order code) of `binarize_morph`; raises on anything the kernel does not support."""
    rows = []
    for t, kd, ke, o in zip(_per_plane(thresh, n_planes, 'thresh'), _per_plane(k_dilate, n_planes, 'k_dilate'),
                            _per_plane(k_erode, n_planes, 'k_erode'), _per_plane(order, n_planes, 'order')):
        for k in (kd, ke):
            if not isinstance(k, (int, np.integer)) or isinstance(k, bool):
                raise TypeError('kernel sizes must be ints (got %r)' % (k,))
            if k < 1 or k > MAX_K:
                raise ValueError('kernel sizes must be in 1..%d (got %d)' % (MAX_K, k))
        rows.append((int(np.floor(float(t))), int(kd), int(ke), _order_code(o)))
    return np.asarray(rows, np.int32).reshape(n_planes, 4)


class MaskDraws:
    """The draws of one item's mask chain for `n_planes` planes of (H, W):
      thresh (P,) float64   the binarisation thresholds as drawn (the record; the kernel reads morph[:, 0])
      morph  (P, 4) int32   (threshold the kernel compares with, k_dilate, k_erode, order code)
      downup (P,)   int32   1 where DownUpMask applies
      cut    (P, 8) int32   (src_plane, dst_row, dst_col, src_row, src_col, h, w, 0); src_plane -1: untouched
      dropout               whether MaskDropout follows (its draws depend on the data: `draw_dropout`)
    NumPy arrays as drawn; `.to(device)` gives the same record with device tensors and the resize tables uploaded. A chain call that gets
    that uploads nothing and does not synchronise (drop-out aside): capture it in a graph and write new draws into `morph`, `downup`,
    `cut` between replays (k within 1..31: the kernel clamps)."""

    def __init__(self, H, W, thresh, morph, downup, cut, dropout=False, ratio=0.125, tab=None):
        self.H, self.W, self.thresh, self.morph, self.downup, self.cut = int(H), int(W), thresh, morph, downup, cut
        self.dropout, self.ratio, self.tab = bool(dropout), float(ratio), tab

    @property
    def n_planes(self):
        return int(self.morph.shape[0])

    @property
    def on_device(self):
        return torch.is_tensor(self.morph)

    def to(self, device=None):
        device = resolve_device(device)
        return MaskDraws(self.H, self.W, self.thresh, upload(self.morph, device), upload(self.downup, device), upload(self.cut, device),
                         self.dropout, self.ratio, _device_table(self.H, self.W, self.ratio, device))


def draw_chain(random, pyrandom, n_planes, H, W, binarize_max_k=30, downscale_mask_p=0.5, dropout=False, from_alpha=False, ratio=0.125):
    """The draws of RandomBinarizedMask -> DownUpMask -> CutMask for `n_planes` planes of (H, W), consuming `random` (a np.random.RandomState)
    and `pyrandom` (Python's `random` module or a random.Random) exactly as the reference does: per plane uniform, randint, randint, choice
    (transforms.py:398-412); one rand() per plane (:487); CutMask's random() and then either rand() + four or six randint per plane (:506-512)
    or rand(), `pyrandom.sample` of the plane pair and four randint (:517-521). The reference's own errors surface for sizes where
    randint(h // 8, h // 4) has an empty range. `dropout`: MaskDropout follows (video; `draw_dropout` makes its draws once the statistics
    are known). `from_alpha`: the planes given to the chain are alphas and GenMaskFromAlpha is folded in (vim.py:58-66) -- the drawn
    threshold (0.1 .. 0.95 of 255) then acts on a 0 / 255 mask, which is `alpha > 127` whatever the draw: the table holds 127."""
    P = int(n_planes)
    thresh = np.zeros((P,), np.float64)
    kd, ke, orders = [], [], []
    for p in range(P):
        thresh[p] = random.uniform(0.1, 0.95) * 255
        kd.append(random.randint(1, binarize_max_k))
        ke.append(random.randint(1, binarize_max_k))
        orders.append(str(random.choice(list(ORDERS))))
    downup = np.asarray([1 if random.rand() < downscale_mask_p else 0 for _ in range(P)], np.int32).reshape(P)
    cut = np.zeros((P, 8), np.int32)
    cut[:, 0] = -1
    if random.random() < 0.5:
        for p in range(P):                                                # CutMask.internal
            if random.rand() < 0.5:
                ph, pw = random.randint(H // 8, H // 4), random.randint(W // 8, W // 4)
                x = random.randint(0, H - ph)
                y = random.randint(0, W - pw)
                x1 = random.randint(0, H - ph)
                y1 = random.randint(0, W - pw)
                cut[p] = (p, x, y, x1, y1, ph, pw, 0)
    elif random.rand() < 0.5 and P > 1:                                   # CutMask.external
        i, j = pyrandom.sample(list(range(0, P)), k=2)
        ph, pw = random.randint(H // 8, H // 4), random.randint(W // 8, W // 4)
        x = random.randint(0, H - ph)
        y = random.randint(0, W - pw)
        cut[i] = (j, x, y, x, y, ph, pw, 0)
        cut[j] = (i, x, y, x, y, ph, pw, 0)
    morph = morph_table(127.0 if from_alpha else thresh, [int(k) for k in kd], [int(k) for k in ke], orders, P)
    return MaskDraws(H, W, thresh, morph, downup, cut, dropout, ratio)


def draw_dropout(random, stats):
    """MaskDropout's draws (transforms.py:544-559) from the (P, 5) statistics (count, xmin, xmax, ymin, ymax) of the planes: an (n, 4) int32
    array of (plane, idx, ph, pw) in the order the reference visits the planes; where it `continue`s (an empty plane, or a bounding box
    under 16 pixels on a side) the entry is (-(plane + 1), 0, 0, 0), which the kernel skips. (0, 4) when the branch is not taken."""
    st = np.asarray(stats).reshape(-1, 5)
    P = st.shape[0]
    if random.rand() < 0.5 or P // 2 < 3:
        return np.zeros((0, 4), np.int32)
    n = random.randint(1, P // 2)
    selected = random.choice(P, n, replace=False)
    out = np.zeros((n, 4), np.int32)
    out[:, 0] = -(np.asarray(selected, np.int32) + 1)
    for e, i in enumerate(selected):
        count, xmin, xmax, ymin, ymax = (int(v) for v in st[i])
        if count == 0:
            continue
        eh, ew = ymax - ymin + 1, xmax - xmin + 1
        if eh // 8 < 2 or ew // 8 < 2:
            continue
        ph, pw = random.randint(eh // 16, eh // 8), random.randint(ew // 16, ew // 8)
        idx = int(random.choice(count, 1)[0])
        out[e] = (int(i), idx, ph, pw)
    return out


# ---- the device stages ------------------------------------------------------------------------------------------------------------------------
def _planes(planes_u8):
    """uint8 (..., H, W) -> the tensor, its shape, and (P, H, W). Not `_inputs.images`: an empty plane is legal here (the stages return it)
    and the whole shape is handed back."""
    x = check_u8(planes_u8)
    if x.dim() < 2:
        raise ValueError('expected (..., H, W) planes (got shape %s)' % (tuple(x.shape),))
    shape = tuple(x.shape)
    H, W = shape[-2:]
    P = int(np.prod(shape[:-2])) if x.dim() > 2 else 1
    if H * W >= 2 ** 31:
        raise ValueError('a plane must have fewer than 2^31 pixels')
    return x, shape, P, H, W


def _table(t, rows, cols, what):
    """A draw table as a device int32 tensor of the given shape (uploaded when it is an array)."""
    if torch.is_tensor(t):
        if t.dtype != torch.int32 or tuple(t.shape) != (rows,) + cols:
            raise ValueError('%s must be int32 of shape %s (got %s %s)' % (what, (rows,) + cols, t.dtype, tuple(t.shape)))
        return t
    a = np.asarray(t)
    if a.shape != (rows,) + cols or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s must hold ints of shape %s (got %s %s)' % (what, (rows,) + cols, a.dtype, a.shape))
    return a.astype(np.int32)


def _up(t, device):
    if torch.is_tensor(t):
        hip.need_cuda(t)
        return t.contiguous()
    return torch.from_numpy(np.ascontiguousarray(t)).to(device, non_blocking=True)


def _launch_morph(x, table, P, H, W):
    out = torch.empty_like(x)
    if x.numel() > 0:
        hip.call('mg_mask_morph', hip.ptr(x), hip.ptr(out), hip.ptr(table), c_long(P), c_int(H), c_int(W), hip.stream())
    return out


def _launch_downup(x, apply, tab, dh, dw, P, H, W):
    out = torch.empty_like(x)
    if x.numel() > 0:
        hip.call('mg_mask_downup', hip.ptr(x), hip.ptr(out), hip.ptr(apply), hip.ptr(tab), c_int(dh), c_int(dw), c_long(P), c_int(H), c_int(W),
                 hip.stream())
    return out


def _launch_cut(x, rects, P, H, W):
    out = torch.empty_like(x)
    if x.numel() > 0:
        hip.call('mg_mask_cut', hip.ptr(x), hip.ptr(out), hip.ptr(rects), c_long(P), c_int(H), c_int(W), hip.stream())
    return out


def binarize_morph(planes_u8, thresh, k_dilate=1, k_erode=1, order='dilate_erode', device=None):
    """RandomBinarizeAlpha._gen_single_mask (transforms.py:393-424) of every plane: 255 * morph(v > floor(thresh)), where morph is cv2.dilate
    with np.ones((k_dilate, k_dilate)) and / or cv2.erode with np.ones((k_erode, k_erode)) in the given order. Each of `thresh`, `k_dilate`,
    `k_erode`, `order` is one value or one per plane; or pass a (P, 4) int32 device tensor (`MaskDraws.morph`) as `thresh`."""
    x, shape, P, H, W = _planes(planes_u8)
    table = _table(thresh, P, (4,), 'the morph table') if torch.is_tensor(thresh) else morph_table(thresh, k_dilate, k_erode, order, P)
    x = to_device(x, device)
    return _launch_morph(x, _up(table, x.device), P, H, W).reshape(shape)


def down_up(planes_u8, apply=True, ratio=0.125, device=None):
    """DownUpMask.downup (transforms.py:486-492) where `apply` (one flag, one per plane, or an int32 device tensor) is set: cv2.resize by `ratio`
    with INTER_LINEAR, back to (W, H), `> 127 -> 255`. Other planes are returned as they are. Any uint8 input."""
    x, shape, P, H, W = _planes(planes_u8)
    if not torch.is_tensor(apply):
        apply = np.asarray([1 if a else 0 for a in _per_plane(apply, P, 'apply')], np.int32).reshape(P)
    apply = _table(apply, P, (), 'apply')
    if x.numel() == 0:
        return x.clone()
    t = resize_tables(H, W, ratio)
    x = to_device(x, device)
    return _launch_downup(x, _up(apply, x.device), _device_table(H, W, ratio, x.device), t['dh'], t['dw'], P, H, W).reshape(shape)


def cut(planes_u8, rects, device=None):
    """CutMask (transforms.py:499-534) from a (P, 8) table (`MaskDraws.cut`): plane p gets the h x w rectangle at (src_row, src_col) of plane
    src_plane written at (dst_row, dst_col); the source is the input, so overlapping rectangles and swaps read the old values."""
    x, shape, P, H, W = _planes(planes_u8)
    rects = _table(rects, P, (8,), 'the cut table')
    x = to_device(x, device)
    return _launch_cut(x, _up(rects, x.device), P, H, W).reshape(shape)


def stats(planes_u8, device=None):
    """(P, 5) int32 on the device: (count, xmin, xmax, ymin, ymax) of the non-zero pixels of every plane; an empty plane gives
    (0, W, -1, H, -1)."""
    x, shape, P, H, W = _planes(planes_u8)
    x = to_device(x, device)
    out = torch.empty((P, 5), dtype=torch.int32, device=x.device)
    if P > 0:
        hip.call('mg_mask_stats', hip.ptr(x), hip.ptr(out), c_long(P), c_int(H), c_int(W), hip.stream())
    return out


def drop(planes_u8, selection, plane_stats, inplace=False, device=None):
    """MaskDropout's rectangles (transforms.py:557-563): entry (plane, idx, ph, pw) of `selection` (n, 4) zeroes the ph x pw rectangle anchored
    at the idx-th non-zero pixel of the plane (raster order), moved up / left to stay inside the bounding box of `plane_stats` (`stats`).
    The live entries must name distinct planes: one workgroup per entry reads and zeroes its plane, so two entries on one plane would race.
    That is checked here for a NumPy `selection` only (`draw_dropout` never repeats a plane); a device-resident table is the caller's to keep
    distinct, as there is no looking at it without a synchronisation."""
    x, shape, P, H, W = _planes(planes_u8)
    n = int(selection.shape[0])
    selection = _table(selection, n, (4,), 'the drop-out table')
    plane_stats = _table(plane_stats, P, (5,), 'the statistics')
    if not torch.is_tensor(selection):
        live = selection[selection[:, 0] >= 0, 0]
        if len(set(live.tolist())) != len(live) or (len(live) and live.max() >= P):
            raise ValueError('the drop-out entries must name distinct planes below %d' % P)
    x = to_device(x, device)
    if not inplace or not x.is_contiguous():
        x = x.clone()
    if n > 0 and x.numel() > 0:
        sel, st = _up(selection, x.device), _up(plane_stats, x.device)        # both held until the launch: a freed upload's block is handed out again
        hip.call('mg_mask_drop', hip.ptr(x), hip.ptr(sel), hip.ptr(st), c_int(n), c_long(P), c_int(H), c_int(W), hip.stream())
    return x.reshape(shape)


def synthesize(planes_u8, draws, dropout_random=None, device=None):
    """The training chain on every plane of a (..., H, W) uint8 tensor: binarise + morphology, down / up, cut, and -- when `draws.dropout` --
    the drop-out, whose second-phase draws are made here from `dropout_random` (the loader's RandomState) after ONE read-back of the planes'
    statistics. Image training passes the alphas (him.py:103); video training passes the alphas with draws made with `from_alpha=True`."""
    if not isinstance(draws, MaskDraws):
        raise TypeError('draws must be a MaskDraws (got %s)' % type(draws).__name__)
    x, shape, P, H, W = _planes(planes_u8)
    if (P, H, W) != (draws.n_planes, draws.H, draws.W):
        raise ValueError('the draws were made for %d planes of %d x %d (got %d of %d x %d)' % (draws.n_planes, draws.H, draws.W, P, H, W))
    if draws.dropout and dropout_random is None:
        raise ValueError('draws.dropout is set: the drop-out draws need dropout_random')
    morph = _table(draws.morph, P, (4,), 'MaskDraws.morph')
    apply = _table(draws.downup, P, (), 'MaskDraws.downup')
    rects = _table(draws.cut, P, (8,), 'MaskDraws.cut')
    if not draws.on_device:
        morph_table(0, morph[:, 1].tolist(), morph[:, 2].tolist(), morph[:, 3].tolist(), P)         # the range checks
    if x.numel() == 0:
        return x.clone()
    t = resize_tables(H, W, draws.ratio)
    x = to_device(x, device)
    tab = draws.tab if draws.tab is not None else _device_table(H, W, draws.ratio, x.device)
    y = _launch_morph(x, _up(morph, x.device), P, H, W)
    y = _launch_downup(y, _up(apply, x.device), tab, t['dh'], t['dw'], P, H, W)
    y = _launch_cut(y, _up(rects, x.device), P, H, W)
    if draws.dropout:
        st = torch.empty((P, 5), dtype=torch.int32, device=x.device)
        hip.call('mg_mask_stats', hip.ptr(y), hip.ptr(st), c_long(P), c_int(H), c_int(W), hip.stream())
        sel = draw_dropout(dropout_random, st.cpu().numpy())                                      # the chain's one host synchronisation
        if sel.shape[0] > 0 and (sel[:, 0] >= 0).any():
            dsel = _up(sel, x.device)
            hip.call('mg_mask_drop', hip.ptr(y), hip.ptr(dsel), hip.ptr(st), c_int(sel.shape[0]), c_long(P), c_int(H), c_int(W), hip.stream())
    return y.reshape(shape)


def from_alpha(alphas_u8, down_up=True, ratio=0.125, device=None):
    """The evaluation mask when no mask directory is given (him.py:58-59, vim.py:58-69): GenMaskFromAlpha, `(alpha > 127) * 255`, then
    DownUpMask(p=1) unless `down_up` is False. It takes no generator, and the reference's DownUpMask still draws one rand() per plane from
    the loader's RandomState there, whatever p is: a seeded evaluation loader that draws from that state afterwards and has to follow the
    reference's stream calls `random.rand()` once per plane itself."""
    x, shape, P, H, W = _planes(alphas_u8)
    if x.numel() == 0:
        return x.clone()
    t = resize_tables(H, W, ratio) if down_up else None
    x = to_device(x, device)
    key = (P, x.device.index)
    if key not in _ALPHA_TABLES:
        _ALPHA_TABLES[key] = (torch.tensor([127, 1, 1, ORDER_NONE], dtype=torch.int32).repeat(P, 1).to(x.device),
                              torch.ones((P,), dtype=torch.int32, device=x.device))
    table, apply = _ALPHA_TABLES[key]
    y = _launch_morph(x, table, P, H, W)
    if down_up:
        y = _launch_downup(y, apply, _device_table(H, W, ratio, x.device), t['dh'], t['dw'], P, H, W)
    return y.reshape(shape)
