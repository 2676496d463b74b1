"""Matte output on the device (HIP kernels of csrc/matteout.hip) -- what the reference's predictor does behind the forward
(demo/maggie_predictor.py, demo/app.py): the green-screen composite of every instance, the mask visualisation, the split of a label map into
instance planes, and the files. The fp32 planes never cross to the host and need not exist at full size at all.

  * `composite`        `(image * a + (1 - a) * background).astype(np.uint8)` per instance (maggie_predictor.py:68-76,151-157), with
                       the reverse transform and the snapping in front of it (:62-65,124-128) fused into its launch (`fused=True`) or, by default
                       and faster as measured, as `reverse_transform_tensor` in front of it.
  * `overlay`          `Image.blend(image, palette(mask > 0), alpha)` (app.py:59-65).
  * `label_planes`     `np.unique` of a label map and `(map == id) * 255` per id (maggie_predictor.py:35-40).
  * `predict_image`    maggie_predictor.py:52-78 with any callable model: `predict_item` -> model -> composites (and, asked for, cut-outs).
  * `save_composites`, `save_overlay`   the .jpg files (maggie_predictor.py:158-162, app.py:67-71) through one `jpegenc.encode_clip`.
  * `VideoMatteWriter` the body of the video predictor's loop (maggie_predictor.py:121-167).

The contract: the bytes are NumPy's and Pillow's, exactly, for alphas in [0, 1] (tests/matteout_restatement.py states them
and tests/test_matteout_cpu.py holds the overlay against Pillow itself). The kernels are compiled without floating-point contraction, because a
fused multiply-add changes bytes. Outside [0, 1] NumPy's own cast is undefined; here the sum is clamped to [0, 255] first.

The input contract is that of utils/_inputs.py: uint8 pixels as a tensor or an array, on the host or on the device; `device=None` rules; TypeError /
ValueError before anything touches the device; `hip.MaggieHipError` without a GPU. `composite` and `overlay` read nothing back and can be captured
in a graph; `label_planes` reads back 36 bytes (the presence words). There is no CPU fallback."""
import os

import numpy as np
import torch

from .. import hip
from ..hip import c_float, c_int, c_long
from . import postprocessing
from ._inputs import check_u8, images, need_gpu, resolve_device, to_device

GREEN = (0, 255, 0)                     # maggie_predictor.py:69-70
MAGENTA = (255, 0, 255)                 # app.py:62: putpalette([0, 0, 0, 255, 0, 255])
PRESENCE_WORDS = 9                      # MG_MATTE_PRESENCE_WORDS (include/maggie_hip.h)


def _colour(c, what):
    if not isinstance(c, (tuple, list)) or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in c):
        raise TypeError('%s must be three ints of 0..255 (got %r)' % (what, c))
    if len(c) != 3 or not all(0 <= int(v) <= 255 for v in c):
        raise ValueError('%s must be three ints of 0..255 (got %r)' % (what, c))
    return [int(v) for v in c]


def _frames(frames_u8, what='frames'):
    """(H, W, 3) or (T, H, W, 3) uint8 -> (tensor, single, T, H, W)."""
    f, lead, T, H, W = images(frames_u8, 3, what)
    if len(lead) > 1:
        raise ValueError('%s must be (H, W, 3) or (T, H, W, 3) (got shape %s)' % (what, tuple(f.shape)))
    return f, len(lead) == 0, T, H, W


def _name(tr):
    return tr['name'][0] if isinstance(tr['name'], (list, tuple)) else tr['name']


def _plan(transform_info, h, w):
    """The loader's list, read as `reverse_transform_tensor` reads it -> (crop_h, crop_w, out_h, out_w) when ONE launch can undo it (any
    paddings, then at most one resize as the last step), else None."""
    ops = []
    for tr in transform_info[::-1]:
        if _name(tr) == 'padding':
            ops.append(('pad',) + tuple(postprocessing._scalar(v) for v in tr['pad_size']))
        elif _name(tr) == 'resize':
            ops.append(('resize',) + tuple(postprocessing._scalar(v) for v in tr['ori_size']))
    crop_h, crop_w = h, w
    for i, (name, a, b) in enumerate(ops):
        if name == 'pad':
            crop_h, crop_w = crop_h - a, crop_w - b
        elif i != len(ops) - 1:
            return None
        else:
            return crop_h, crop_w, a, b
    return crop_h, crop_w, crop_h, crop_w


def _background(background, T, H, W):
    """Three bytes, or a uint8 image (H, W, 3) / (1, H, W, 3) / (T, H, W, 3) -> (colour or None, image or None)."""
    if torch.is_tensor(background) or isinstance(background, np.ndarray):
        b, single, n, bh, bw = _frames(background, 'background')
        if (bh, bw) != (H, W) or n not in (1, T):
            raise ValueError('a background image must be (H, W, 3), (1, H, W, 3) or (T, H, W, 3) like the frames (got shape %s for %d frames of %d x %d)'
                             % (tuple(b.shape), T, H, W))
        return None, b.reshape(n, H, W, 3)
    return _colour(background, 'background'), None


def composite(frames_u8, alpha, background=GREEN, *, transform_info=None, snap=False, return_alpha=False, fused=None, device=None):
    """`(image * a[..., None] + (1 - a[..., None]) * background).astype(np.uint8)` for every instance of every frame.

    frames_u8: (H, W, 3) or (T, H, W, 3) uint8 (tensor or array, host or device). alpha: a DEVICE fp32 tensor (..., P, h, w) with T * P planes.
    With `transform_info` (the loader's list, as `postprocessing.reverse_transform_tensor` takes it) the alpha is at the network's size and
    the padding crop, the bilinear resize and -- with `snap` -- the snapping (<= 1/255 -> 0, >= 254/255 -> 1) happen in the same launch; without
    it the planes must have the frame's size. background: three bytes, or a uint8 image (H, W, 3) / (1, H, W, 3) shared by the frames, or
    (T, H, W, 3). Returns uint8 (T, P, H, W, 3); with `return_alpha` also the fp32 (T, P, H, W) alpha the bytes were made from. A list with more
    than one resize goes through `reverse_transform_tensor` first. `fused`: None takes the form that measured faster: one
    launch when nothing is resized (a crop, the snapping and the composite), else `reverse_transform_tensor(snap=snap)` and the composite at
    full size, two launches; True forces the single launch, whose alpha is rounded operation by operation and so differs from
    `reverse_transform_tensor`'s in the last bit here and there. No read-back either way: capturable in a graph."""
    f, _, T, H, W = _frames(frames_u8)
    if not torch.is_tensor(alpha):
        raise TypeError('alpha must be a device tensor (got %s)' % type(alpha).__name__)
    if alpha.dtype != torch.float32:
        raise TypeError('alpha must be float32 (got %s)' % alpha.dtype)
    if alpha.dim() < 3:
        raise ValueError('alpha must be (..., P, h, w) (got shape %s)' % (tuple(alpha.shape),))
    P, h, w = (int(v) for v in alpha.shape[-3:])
    if h < 1 or w < 1 or alpha.numel() != T * P * h * w:
        raise ValueError('alpha of shape %s does not hold P planes for each of %d frames' % (tuple(alpha.shape), T))
    colour, image = _background(background, T, H, W)
    plan = (h, w, h, w) if transform_info is None else _plan(transform_info, h, w)
    if plan is not None:
        if min(plan) < 1:
            raise ValueError('the paddings of transform_info leave nothing of a %d x %d plane' % (h, w))
        if plan[2:] != (H, W):
            raise ValueError('the alpha comes out at %d x %d, the frames are %d x %d' % (plan[2], plan[3], H, W))
    need_gpu(alpha)
    hip.need_cuda(alpha)
    f = to_device(f, alpha.device if device is None else device)
    if f.device != alpha.device:
        raise ValueError('frames on %s, alpha on %s' % (f.device, alpha.device))
    if plan is None or (plan[:2] != plan[2:] and not fused):        # several resizes, or the two-launch form: the reverse transform, then the identity form
        alpha = postprocessing.reverse_transform_tensor(alpha, transform_info, snap=bool(snap))
        h, w = (int(v) for v in alpha.shape[-2:])
        if (h, w) != (H, W):
            raise ValueError('the alpha comes out at %d x %d, the frames are %d x %d' % (h, w, H, W))
        plan = (H, W, H, W)
    a = alpha.reshape(T * P, h, w).contiguous()
    if image is not None:
        image = to_device(image, f.device)
    with torch.cuda.device(f.device):
        out = torch.empty((T, P, H, W, 3), dtype=torch.uint8, device=f.device)
        aout = torch.empty((T, P, H, W), dtype=torch.float32, device=f.device) if return_alpha else None
        if T * P:
            r, g, b = colour if colour is not None else (0, 0, 0)
            hip.call('mg_matte_composite', hip.ptr(a), c_long(T), c_int(P), c_int(h), c_int(w), c_int(plan[0]), c_int(plan[1]), c_int(H), c_int(W),
                     c_int(int(bool(snap))), hip.ptr(f), hip.ptr(image), c_long(0 if image is None else image.shape[0]), c_int(r), c_int(g),
                     c_int(b), hip.ptr(out), hip.ptr(aout), hip.stream())
    return (out, aout) if return_alpha else out


def overlay(frames_u8, masks_u8, colour=MAGENTA, alpha=0.5, *, device=None):
    """`Image.blend(image, mask_rgb, alpha)` with mask_rgb = `colour` where mask > 0 and black elsewhere (app.py:59-65). frames_u8 (H, W, 3) or
    (T, H, W, 3), masks_u8 (H, W) or (T, H, W), both uint8 -> uint8 of the frames' shape. alpha in [0, 1]. One launch, no read-back."""
    f, single, T, H, W = _frames(frames_u8)
    m = check_u8(masks_u8, 'masks')
    if tuple(m.shape) != tuple(f.shape[:-1]):
        raise ValueError('masks must be %s like the frames (got shape %s)' % (tuple(f.shape[:-1]), tuple(m.shape)))
    rgb = _colour(colour, 'colour')
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
        raise TypeError('alpha must be a number in [0, 1] (got %r)' % (alpha,))
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError('alpha must lie in [0, 1] (got %r)' % (alpha,))
    f = to_device(f, device)
    m = to_device(m, f.device)
    with torch.cuda.device(f.device):
        out = torch.empty_like(f)
        hip.call('mg_matte_overlay', hip.ptr(f), hip.ptr(m), c_long(T), c_int(H), c_int(W), c_int(rgb[0]), c_int(rgb[1]), c_int(rgb[2]),
                 c_float(float(alpha)), hip.ptr(out), hip.stream())
    return out


def _label_map(label_map):
    if isinstance(label_map, np.ndarray):
        if label_map.dtype not in (np.uint8, np.int32):
            raise TypeError('a label map is uint8 or int32 (got %s)' % label_map.dtype)
        label_map = torch.from_numpy(np.ascontiguousarray(label_map))
    if not torch.is_tensor(label_map):
        raise TypeError('expected a label map as a tensor or an array, got %s' % type(label_map).__name__)
    if label_map.dtype not in (torch.uint8, torch.int32):
        raise TypeError('a label map is uint8 or int32 (got %s)' % label_map.dtype)
    if label_map.dim() != 2 or label_map.numel() < 1:
        raise ValueError('a label map is (H, W) with at least one pixel (got shape %s)' % (tuple(label_map.shape),))
    return label_map


def label_planes(label_map, *, device=None):
    """A label map (H, W), uint8 or int32 with ids 0..255 -> (ids, planes): the ids other than 0 in ascending order (a list of ints) and uint8
    (len(ids), H, W) with 255 where the map equals the id (maggie_predictor.py:35-40). A map without instances gives ([], an empty (0, H, W)).
    ValueError for an id outside 0..255. Two launches and one read-back of 36 bytes (which ids there are decides the allocation)."""
    m = to_device(_label_map(label_map), device)
    H, W = (int(v) for v in m.shape)
    eb = c_int(m.element_size())
    with torch.cuda.device(m.device):
        presence = torch.empty((PRESENCE_WORDS,), dtype=torch.int32, device=m.device)
        hip.call('mg_matte_label_ids', hip.ptr(m), eb, c_long(H * W), hip.ptr(presence), hip.stream())
        words = presence.cpu().numpy().view(np.uint32)                       # the read-back
        if words[8]:
            raise ValueError('a label map holds ids 0..255; this one has labels outside that range')
        ids = [i for i in range(1, 256) if words[i >> 5] >> (i & 31) & 1]
        planes = torch.empty((len(ids), H, W), dtype=torch.uint8, device=m.device)
        if ids:
            host = (hip.ctypes.c_uint8 * len(ids))(*ids)
            hip.call('mg_matte_label_planes', hip.ptr(m), eb, c_long(H * W), host, c_int(len(ids)), hip.ptr(planes), hip.stream())
    return ids, planes


def predict_image(model, frame_u8, instances, *, preprocessor=None, background=GREEN, postprocess=False, cutouts=False, refine=False):
    """maggie_predictor.py:52-78 on the device: `frame_u8` (H, W, 3) uint8 and `instances`, a label map (H, W) or uint8 planes (n, H, W) of
    0 / 255 -> {'alpha': (n, H, W) fp32, 'composites': (n, H, W, 3) uint8}. `model` is any callable with the model's contract
    (batch -> {'refined_masks': (1, 1, n, Hp, Wp)}); it runs under `no_grad`. `preprocessor`: a `preprocess.DevicePreprocessor` (default: a
    new one). The alpha is reverse-transformed, snapped and composited by `composite(transform_info=..., snap=True)`; with `postprocess` it is
    reverse-transformed and snapped, filtered by `postprocessing.postprocess` (the largest component, as the video predictor does at :130) and composited at full size.
    With `cutouts` the result also has 'cutouts': (n, H, W, 4) uint8, `cutout.cutout` of the frame and the returned alpha (straight RGBA with
    an estimated foreground colour instead of the frame's own: utils/cutout.py). With `refine` (True, or a dict with `radius` and / or `eps`) the
    alpha is `refine.refine(frame, prediction, transform_info=..., snap=True, as_float=True)`, the guided filter against the full-size frame
    (utils/refine.py), in place of the bilinear reverse transform: byte / 255, so the composites and the cut-outs are made from the refined
    bytes; with `postprocess` the largest-component filter runs on it."""
    from .preprocess import DevicePreprocessor
    from . import refine as _refine                          # (that module imports this one)
    ropts = _refine.options(refine)
    frame = check_u8(frame_u8, 'frame')
    if frame.dim() != 3 or frame.shape[-1] != 3:
        raise ValueError('frame must be (H, W, 3) (got shape %s)' % (tuple(frame.shape),))
    H, W = (int(v) for v in frame.shape[:2])
    if not (torch.is_tensor(instances) or isinstance(instances, np.ndarray)):
        raise TypeError('instances must be a label map (H, W) or uint8 planes (n, H, W), got %s' % type(instances).__name__)
    if instances.ndim == 2:
        if tuple(instances.shape) != (H, W):
            raise ValueError('the label map must be (%d, %d) like the frame (got shape %s)' % (H, W, tuple(instances.shape)))
        planes = label_planes(instances, device=None if preprocessor is None else preprocessor.device)[1]
    else:
        planes = check_u8(instances, 'instances')
        if planes.dim() != 3 or tuple(planes.shape[1:]) != (H, W):
            raise ValueError('instance planes must be (n, %d, %d) like the frame (got shape %s)' % (H, W, tuple(planes.shape)))
    pre = DevicePreprocessor() if preprocessor is None else preprocessor
    dev = resolve_device(pre.device, planes if planes.is_cuda else frame)
    n = int(planes.shape[0])
    if n == 0:
        empty = {'alpha': torch.empty((0, H, W), dtype=torch.float32, device=dev), 'composites': torch.empty((0, H, W, 3), dtype=torch.uint8, device=dev)}
        if cutouts:
            empty['cutouts'] = torch.empty((0, H, W, 4), dtype=torch.uint8, device=dev)
        return empty
    frame = to_device(frame, dev)
    batch, info = pre.predict_item(frame, planes)
    with torch.no_grad():
        pred = model(batch)['refined_masks']
    if ropts is not None:
        alpha = _refine.refine(frame, pred.float(), transform_info=info, snap=True, as_float=True, **ropts).reshape(n, H, W)
        if postprocess:
            alpha = postprocessing.postprocess(alpha)
        out = {'alpha': alpha, 'composites': composite(frame, alpha, background)[0]}
    elif postprocess:
        alpha = postprocessing.postprocess(postprocessing.reverse_transform_tensor(pred, info, snap=True)).reshape(n, H, W)
        out = {'alpha': alpha, 'composites': composite(frame, alpha, background)[0]}
    else:
        comp, alpha = composite(frame, pred.float(), background, transform_info=info, snap=True, return_alpha=True)
        out = {'alpha': alpha[0], 'composites': comp[0]}
    if cutouts:
        from . import cutout as _cutout                        # (that module imports this one)
        out['cutouts'] = _cutout.cutout(frame, out['alpha'])[0]
    return out


def _write_all(paths, files):
    from .jpegenc import _write
    for p, data in zip(paths, files):
        _write(p, data)
    return list(paths)


def save_composites(composites, out_dir, stem, quality=75):
    """The files of maggie_predictor.py:158-162: composites (P, H, W, 3) uint8 -> `out_dir/NN_<stem>.jpg` for NN = 00, 01, ... with the bytes
    `Image.fromarray(c).save(path)` writes (Pillow's default quality 75), from one `jpegenc.encode_clip`. Returns the paths."""
    from . import jpegenc
    c = check_u8(composites, 'composites')
    if c.dim() != 4 or c.shape[-1] != 3:
        raise ValueError('composites must be (P, H, W, 3) (got shape %s)' % (tuple(c.shape),))
    if c.shape[0] == 0:
        return []
    files = jpegenc.encode_clip(c, quality)
    return _write_all([os.path.join(out_dir, '%02d_%s.jpg' % (i, stem)) for i in range(len(files))], files)


def save_overlay(overlays, out_dir, names, quality=75):
    """The files of app.py:67-71: overlays (H, W, 3) or (T, H, W, 3) uint8 and one name or T names `<prefix>_<suffix>` ->
    `out_dir/<name>.jpg`, Pillow's bytes at its default quality, from one `jpegenc.encode_clip`. Returns the paths."""
    from . import jpegenc
    o, single, T, _, _ = _frames(overlays, 'overlays')
    names = [names] if isinstance(names, str) else list(names)
    if len(names) != T or not all(isinstance(n, str) for n in names):
        raise ValueError('%d overlays need %d names (got %r)' % (T, T, names))
    files = jpegenc.encode_clip(o.reshape(T, *o.shape[-3:]), quality)
    return _write_all([os.path.join(out_dir, n + '.jpg') for n in names], files)


def _stem(name):
    name = name[0] if isinstance(name, (list, tuple)) else name
    if not isinstance(name, str):
        raise TypeError('a frame name is a string or the loader\'s one-element list (got %r)' % (name,))
    return os.path.basename(name).replace('.jpg', '')


class VideoMatteWriter:
    """The body of the video predictor's loop behind the forward (maggie_predictor.py:121-167), one `push` per clip of three frames: reverse
    transform and snapping, the largest-component filter, the bookkeeping of `all_preds` (a clip's frame t+1 is predicted again as frame t of
    the next clip: the old one is dropped), the composites of the oldest stored frame -- of all stored frames on the last clip -- and their
    files `out_dir/NN_<frame name>.jpg`."""

    def __init__(self, out_dir, background=GREEN, quality=75):
        self.out_dir, self.quality = out_dir, quality
        self.background = _colour(background, 'background')
        self.preds, self.frames, self.names = [], [], []

    def push(self, alpha_clip, transform_info, frames_u8, names, is_first, is_last):
        """alpha_clip (1, 3, n, h, w) fp32 on the device (`output['refined_masks']`), the clip's `transform_info`, its frames (3, H, W, 3) uint8
        and their three names (paths; the loader's one-element lists are accepted) -> the paths written."""
        f, single, T, H, W = _frames(frames_u8)
        if not torch.is_tensor(alpha_clip) or alpha_clip.dim() != 5 or alpha_clip.shape[0] != 1 or alpha_clip.shape[1] != T or single:
            raise ValueError('alpha_clip must be (1, T, n, h, w) for frames (T, H, W, 3)')
        stems = [_stem(n) for n in names]
        if len(stems) != T or T < 2:
            raise ValueError('a clip has one name per frame and at least two frames (got %d names for %d frames)' % (len(stems), T))
        need_gpu(alpha_clip)
        alpha = postprocessing.reverse_transform_tensor(alpha_clip, transform_info, snap=True)              # :124-128
        if tuple(alpha.shape[-2:]) != (H, W):
            raise ValueError('the alpha comes out at %s, the frames are %d x %d' % (tuple(alpha.shape[-2:]), H, W))
        alpha = postprocessing.postprocess(alpha)[0]                                                          # :130
        f = to_device(f, alpha.device)
        if is_first:                                                                                          # :134-141
            self.preds, self.frames, self.names = list(alpha), list(f), stems
        else:
            self.names += stems[2:]
            self.frames += list(f[2:])
            self.preds = self.preds[:-1] + list(alpha[1:])
        end = len(self.preds) if is_last else 1                                                               # :150
        k = min(end, len(self.names))
        paths = []
        if k and alpha.shape[1]:
            comps = composite(torch.stack(self.frames[:k]), torch.stack(self.preds[:k]), self.background)
            n = comps.shape[1]
            from . import jpegenc
            files = jpegenc.encode_clip(comps.reshape(k * n, H, W, 3), self.quality)
            paths = _write_all([os.path.join(self.out_dir, '%02d_%s.jpg' % (i, self.names[t])) for t in range(k) for i in range(n)], files)
        if len(self.preds) > 3:                                                                               # :165-167
            self.preds, self.frames, self.names = self.preds[-3:], self.frames[-3:], self.names[-3:]
        return paths
