"""NumPy / torch restatement of the reference's transition and trimap ground truth (maggie/dataloader/utils.py:5-35, him.py:152-200,
vim.py:160-211), for the tests only -- the product never imports it.

OpenCV is not installed where this project is developed, so `dilate` / `erode` restate its DOCUMENTED behaviour (an unpinned third-party
restatement, like the ellipse of tests/test_region_oracle.py): element E = oracle.region.ellipse_kernel(k), anchor a = k // 2,
dst[y, x] = max (min) over E[i, j] != 0 of src[y + i - a, x + j - a], pixels outside the image take no part, `iterations` = the filter
applied that many times. tests/test_groundtruth_cpu.py checks them against scipy.ndimage's footprint filters and hand-written cases.

`gen_transition_gt` / `gen_diff_mask` and the item glue (`him_train_item`, `eval_item`, `vim_train_item`) restate the reference's torch
code statement by statement; tests/golden/groundtruth_pinned.npz pins them against the reference's own functions run over these filters.
The seeded inputs of that fixture are regenerated here (`soft_planes`, `noise_planes`, `clip_planes`): it stores outputs only."""
import numpy as np
import torch

from oracle.region import ellipse_kernel


# ---- the filters, from the definition --------------------------------------------------------------------------------------------------
def _absent(dtype, is_max):
    """The value of a pixel that takes no part: below (above) everything the dtype holds."""
    if np.issubdtype(dtype, np.floating):
        return -np.inf if is_max else np.inf
    info = np.iinfo(dtype)
    return info.min if is_max else info.max


def _morph_once(src, elem, is_max):
    k = elem.shape[0]
    a = k // 2
    H, W = src.shape
    pad = np.full((H + k - 1, W + k - 1), _absent(src.dtype, is_max), src.dtype)
    pad[a:a + H, a:a + W] = src
    out = None
    for i, j in zip(*np.nonzero(elem)):
        view = pad[i:i + H, j:j + W]                      # src[y + i - a, x + j - a]
        out = view.copy() if out is None else (np.maximum(out, view) if is_max else np.minimum(out, view))
    return out


def _morph(src, k, iterations, is_max):
    src = np.asarray(src)
    squeeze = src.ndim == 3 and src.shape[2] == 1          # cv2 returns (H, W) for an (H, W, 1) input
    if squeeze:
        src = src[:, :, 0]
    assert src.ndim == 2 and iterations >= 1
    elem = k if isinstance(k, np.ndarray) else ellipse_kernel(int(k))
    out = np.ascontiguousarray(src)
    for _ in range(int(iterations)):
        out = _morph_once(out, elem, is_max)
    return out


def dilate(src, k, iterations=1):
    """cv2.dilate(src, ellipse(k) or a given element, iterations=iterations) of one plane."""
    return _morph(src, k, iterations, True)


def erode(src, k, iterations=1):
    """cv2.erode, as `dilate`."""
    return _morph(src, k, iterations, False)


def scipy_morph(src, k, iterations, is_max):
    """The independent formulation: scipy.ndimage's footprint filters, constant border 0 / 255, applied `iterations` times (uint8 planes).
    The footprint is centred at k // 2 like OpenCV's anchor; scipy's `origin` is 0 for that centre."""
    from scipy import ndimage
    elem = ellipse_kernel(int(k)).astype(bool)
    out = np.asarray(src)
    for _ in range(int(iterations)):
        out = (ndimage.maximum_filter(out, footprint=elem, mode='constant', cval=0) if is_max
               else ndimage.minimum_filter(out, footprint=elem, mode='constant', cval=255))
    return out


# ---- maggie/dataloader/utils.py, restated ------------------------------------------------------------------------------------------------
def gen_transition_gt(alphas, masks=None, k_size=25, iterations=1):
    """utils.py:15-35. alphas: (n, 1, H, W) tensor; returns (n, 1, H, W) float64. The `masks` branch is kept literally."""
    planes = []
    for x in alphas:
        plane = x[0, :, :, None].numpy()
        band = (dilate(plane, k_size, iterations) - erode(plane, k_size, iterations)) > 0
        planes.append(torch.from_numpy(band.astype(float)))
    out = torch.stack(planes).unsqueeze(1)
    if masks is not None:
        if masks.shape[-1] != alphas.shape[-1]:
            masks = torch.repeat_interleave(masks, 8, dim=-1)
            masks = torch.repeat_interleave(masks, 8, dim=-2)
        diff = (alphas > 127) != (masks == 255)
        out[diff > 0] = 1.0
    return out


def gen_diff_mask(alphas, k_size=25, iterations=1):
    """utils.py:5-13. alphas: (n, 1, H, W) uint8 tensor; returns (n, 1, H, W) of the same dtype."""
    planes = [torch.from_numpy(dilate(x[0, :, :, None].numpy(), k_size, iterations)) for x in alphas]
    return torch.stack(planes).unsqueeze(1)


# ---- the datasets' glue, restated ----------------------------------------------------------------------------------------------------------
def threshold(alphas_u8, thresh=5):
    """transforms.py:744: alphas[alphas < 5] = 0 (applied to `alphas`, not to `ori_alphas`)."""
    a = np.array(alphas_u8, copy=True)
    a[a < thresh] = 0
    return a


def him_train_item(alpha_u8, mask_u8, chosen_ids, max_inst, k_size, iterations, with_masks=True, downscale_mask=True):
    """him.py:157-189. alpha_u8 (1, n_i, H, W) after `threshold`, mask_u8 the same shape -> transition (1, max_inst, H, W) float32.
    `with_masks=False` drops the (dead) masks argument: the device path's behaviour."""
    alpha = torch.from_numpy(np.asarray(alpha_u8)) * 1.0 / 255
    mask = torch.from_numpy(np.asarray(mask_u8)) * 1.0 / 255
    if max_inst - alpha.shape[1] > 0:
        new_alpha = torch.zeros(1, max_inst, *alpha.shape[2:])
        new_mask = torch.zeros(1, max_inst, *mask.shape[2:])
        new_alpha[:, chosen_ids] = alpha
        new_mask[:, chosen_ids] = mask
        alpha, mask = new_alpha, new_mask
    if downscale_mask:                                     # him.py:172-173; gen_transition_gt then repeats the mask 8 x 8 (H, W multiples of 8)
        mask = torch.nn.functional.interpolate(mask, size=(alpha.shape[2] // 8, alpha.shape[3] // 8), mode='nearest')
    trans = gen_transition_gt(alpha[0, :, None], mask[0, :, None] if with_masks else None, k_size=k_size, iterations=iterations)
    return trans.float()[None, :, 0]


def eval_item(ori_alphas_u8):
    """him.py:190-196 / vim.py:198-203. ori_alphas_u8 (T, n_i, H, W) -> trimap (T, n_i, H, W) float32 in {0, 1, 2}."""
    alphas = torch.from_numpy(np.asarray(ori_alphas_u8)) * 1.0 / 255
    trans = gen_transition_gt(alphas.flatten(0, 1)[:, None])
    trans = trans.reshape_as(alphas)
    trimap = torch.zeros_like(alphas)
    trimap[alphas > 0.5] = 2.0
    trimap[trans > 0] = 1.0
    return trimap


def vim_train_item(alphas_u8, chosen_ids, max_inst, k_size, iterations):
    """vim.py:160-183,211. alphas_u8 (T, n_i, H, W) after `threshold` -> transition (T, max_inst, H, W) float32."""
    alphas = torch.from_numpy(np.asarray(alphas_u8))
    if max_inst - alphas.shape[1] > 0:
        new_alpha = torch.zeros(alphas.shape[0], max_inst, *alphas.shape[2:], dtype=alphas.dtype)
        new_alpha[:, chosen_ids] = alphas
        alphas = new_alpha
    diff = (np.abs(alphas[1:].float() - alphas[:-1].float()) > 5).type(torch.uint8) * 255
    t = gen_diff_mask(diff.flatten(0, 1)[:, None], k_size, iterations)
    t = t.reshape_as(diff)
    t = torch.cat([torch.ones_like(t[:1]), t], dim=0)
    t = t.sum(1, keepdim=True).expand_as(t)
    t = (t > 0).type(torch.uint8)
    return t.float()


# ---- the same results in the uint8 domain (what the device computes) -----------------------------------------------------------------------
def transition_u8(plane_u8, k_size, iterations):
    return dilate(plane_u8, k_size, iterations) > erode(plane_u8, k_size, iterations)


def transition_planes(alphas_u8, k_size, iterations, n_slots=None, slot_ids=None):
    """(T, n_i, H, W) uint8 -> (T, n_slots, H, W) float32, plane j in slot slot_ids[j]."""
    a = np.asarray(alphas_u8)
    T, n_i, H, W = a.shape
    n_slots = n_i if n_slots is None else n_slots
    ids = list(range(n_i)) if slot_ids is None else list(slot_ids)
    out = np.zeros((T, n_slots, H, W), np.float32)
    for t in range(T):
        for j in range(n_i):
            out[t, ids[j]] = transition_u8(a[t, j], k_size, iterations)
    return out


def trimap_planes(alphas_u8):
    a = np.asarray(alphas_u8)
    out = np.where(a >= 128, np.float32(2), np.float32(0)).astype(np.float32)
    for idx in np.ndindex(a.shape[:-2]):
        out[idx][transition_u8(a[idx], 25, 1)] = 1
    return out


def diff_planes(alphas_u8, k_size, iterations, n_slots=None, diff_thresh=5):
    a = np.asarray(alphas_u8).astype(np.int16)
    T, n_i, H, W = a.shape
    n_slots = n_i if n_slots is None else n_slots
    out = np.ones((T, n_slots, H, W), np.float32)
    for t in range(1, T):
        union = ((np.abs(a[t] - a[t - 1]) > diff_thresh).any(0) * 255).astype(np.uint8)
        out[t] = (dilate(union, k_size, iterations) > 0)[None]
    return out


# ---- seeded inputs (regenerated, never stored) ----------------------------------------------------------------------------------------------
def soft_ellipse(rng, H, W, cy=None, cx=None):
    """One soft-edged ellipse: semi-axes H/10..H/4 x W/12..W/5 anywhere in the plane, Gaussian blur sigma 0.8..3, values 0..255."""
    from scipy import ndimage
    ry, rx = rng.uniform(H / 10, H / 4), rng.uniform(W / 12, W / 5)
    cy = rng.uniform(0.15 * H, 0.85 * H) if cy is None else cy
    cx = rng.uniform(0.15 * W, 0.85 * W) if cx is None else cx
    yy, xx = np.mgrid[0:H, 0:W]
    hard = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.float64) * 255
    return np.clip(np.rint(ndimage.gaussian_filter(hard, rng.uniform(0.8, 3.0))), 0, 255).astype(np.uint8)


def soft_planes(seed, n, H, W):
    """(n, H, W) uint8 soft ellipses; small planes (where an ellipse of H/10 has no interior) still get their values from the same rule."""
    rng = np.random.default_rng(seed)
    return np.stack([soft_ellipse(rng, H, W) for _ in range(n)])


def noise_planes(seed, n, H, W):
    """(n, H, W) uniform uint8 noise with 0 and 255 planted on the border (both corners of the first row, both of the last)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    a[:, 0, 0] = 255
    a[:, -1, -1] = 0
    a[:, 0, -1] = 0 if W > 1 else a[:, 0, -1]
    a[:, -1, 0] = 255 if H > 1 else a[:, -1, 0]
    return a


def clip_planes(seed, T, n, H, W):
    """(T, n, H, W) uint8: every instance a soft ellipse that drifts a few pixels per frame (so the frame differences are thin bands)."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    out = np.zeros((T, n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for j in range(n):
        ry, rx = rng.uniform(H / 10, H / 4), rng.uniform(W / 12, W / 5)
        cy, cx = rng.uniform(0.3 * H, 0.7 * H), rng.uniform(0.3 * W, 0.7 * W)
        vy, vx = rng.uniform(-3, 3), rng.uniform(-3, 3)
        sigma = rng.uniform(0.8, 3.0)
        for t in range(T):
            hard = (((yy - cy - vy * t) / ry) ** 2 + ((xx - cx - vx * t) / rx) ** 2 <= 1).astype(np.float64) * 255
            out[t, j] = np.clip(np.rint(ndimage.gaussian_filter(hard, sigma)), 0, 255).astype(np.uint8)
    return out


# the cases of tests/golden/groundtruth_pinned.npz: name -> how the reference's functions are called on which seeded input
GOLDEN = {
    # him.py:185-189 (training): alpha and mask already / 255, the mask downscaled by 8 (H, W multiples of 8), padded to max_inst slots
    'train': dict(seed=101, n=3, H=256, W=328, max_inst=5, chosen_ids=[3, 0, 4], k_size=4, iterations=7),
    # him.py:190-196 (evaluation): ori_alphas / 255, the defaults (k = 25, one pass)
    'eval': dict(seed=202, n=3, H=253, W=331),
    # vim.py:171-183 (training): uint8 frame differences
    'diff': dict(seed=303, T=4, n=2, H=253, W=331, max_inst=3, chosen_ids=[2, 0], k_size=3, iterations=4),
}


def golden_inputs(name):
    c = GOLDEN[name]
    if name == 'train':
        alpha = threshold(soft_planes(c['seed'], c['n'], c['H'], c['W']))[None]
        mask = ((alpha > 127) * 255).astype(np.uint8)
        return alpha, mask
    if name == 'eval':
        return soft_planes(c['seed'], c['n'], c['H'], c['W'])[None]
    return threshold(clip_planes(c['seed'], c['T'], c['n'], c['H'], c['W']))
