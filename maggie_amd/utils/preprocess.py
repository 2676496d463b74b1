"""Input side of the hot path on the device -- the tensor work the reference's DataLoader does on the CPU after
decoding an item, fed from uint8 buffers instead:

  * `ToTensor` + `Normalize` (maggie/dataloader/transforms.py:720-778): frames (T, H, W, 3) uint8 -> (T, 3, H, W) fp32,
    `/ 255`, `(x - mean) / std`; alphas below 5 are zeroed (`alphas[alphas < 5] = 0`, :744);
  * item assembly of `HIMDataset.__getitem__` (maggie/dataloader/him.py:157-173): `alpha / 255`, `mask / 255`, scatter of the
    real instances into `max_inst` slots (`chosen_ids`), nearest downscale of the masks to (H // 8, W // 8).

The caller keeps the host logic (file decoding, augmentation, which instance goes to which slot); what reaches the GPU is uint8 --
4x fewer PCIe bytes than the fp32 `image/alpha/mask` tensors of the reference, and no fp32 `fg`/`bg` tensors at all (the model
never reads them). Two HIP kernels (mg_preprocess_image, mg_preprocess_planes), bit-exact against the reference's arithmetic."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import affine, crop, geometry, groundtruth, maskgen, photometric
from . import motion as motion_blur                   # `motion` is the argument's name in the training item
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, check_u8, float3, resolve_device          # the two constants are this module's public names too


def _u8(x, device):
    """The uint8 check, then the upload to `resolve_device(device)`: a dtype error comes before the no-GPU one."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))                 # first: the message has always named the torch dtype
    return check_u8(x, 'pixels').to(resolve_device(device), non_blocking=True).contiguous()


def normalize_frames(frames_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """(..., H, W, 3) uint8 -> (..., 3, H, W) fp32 normalised (ToTensor + Normalize.norm)."""
    x = _u8(frames_u8, device)
    hip.need_cuda(x)
    device = x.device
    *lead, H, W, C = x.shape
    if C != 3:
        raise ValueError('frames must be (..., H, W, 3)')
    n = int(np.prod(lead)) if lead else 1
    out = torch.empty(tuple(lead) + (3, H, W), dtype=torch.float32, device=device)
    m, s = float3(mean), float3(std)
    for f0 in range(0, n, 65535):
        f1 = min(n, f0 + 65535)
        hip.call('mg_preprocess_image', hip.ctypes.c_void_p(x.data_ptr() + f0 * H * W * 3), hip.ctypes.c_void_p(out.data_ptr() + f0 * H * W * 12),
                 m, s, c_long(f1 - f0), c_long(H * W), hip.stream())
    return out


def scale_planes(planes_u8, n_slots=None, slot_ids=None, out_size=None, thresh=0, device=None):
    """(F, n_i, H, W) uint8 -> (F, n_slots, Ho, Wo) fp32 = v / 255 (0 below `thresh`), plane j of every frame written to slot
    slot_ids[j] (default: identity, n_slots = n_i), other slots zero; (Ho, Wo) != (H, W): F.interpolate(mode='nearest')."""
    x = _u8(planes_u8, device)
    hip.need_cuda(x)
    device = x.device
    F_, n_i, H, W = x.shape
    n_slots = n_i if n_slots is None else int(n_slots)
    Ho, Wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    table = None
    if slot_ids is not None:
        ids = [int(i) for i in slot_ids]
        if len(ids) != n_i or len(set(ids)) != n_i or min(ids) < 0 or max(ids) >= n_slots:
            raise ValueError('slot_ids must name %d distinct slots below %d' % (n_i, n_slots))
        src = np.full((n_slots,), -1, np.int32)
        src[ids] = np.arange(n_i, dtype=np.int32)
        table = torch.from_numpy(np.tile(src, F_)).to(device, non_blocking=True)
    elif n_slots != n_i:
        raise ValueError('n_slots != n_i needs slot_ids')
    out = torch.empty((F_, n_slots, Ho, Wo), dtype=torch.float32, device=device)
    per = max(1, 65535 // n_slots)
    for f0 in range(0, F_, per):
        f1 = min(F_, f0 + per)
        hip.call('mg_preprocess_planes', hip.ctypes.c_void_p(x.data_ptr() + f0 * n_i * H * W), hip.ctypes.c_void_p(out.data_ptr() + f0 * n_slots * Ho * Wo * 4),
                 hip.ptr(None if table is None else table[f0 * n_slots:]), c_int(f1 - f0), c_int(n_i), c_int(n_slots), c_int(H), c_int(W),
                 c_int(Ho), c_int(Wo), c_int(int(thresh)), hip.stream())
    return out


class DevicePreprocessor:
    """frames / alphas / masks of ONE item as uint8 -> the `image`, `alpha`, `mask` entries of the reference's item dict
    (him.py:175-181), on the device. `slot_ids`: the `chosen_ids` of him.py:161 (training pads the instances to `max_inst` slots);
    None keeps the instances where they are (evaluation)."""

    def __init__(self, max_inst=10, downscale_mask=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
        self.max_inst, self.downscale_mask, self.mean, self.std, self.device = max_inst, downscale_mask, mean, std, device

    def __call__(self, frames_u8, alphas_u8=None, masks_u8=None, slot_ids=None, *, transition=None, trimap=False, mask_draws=None):
        """`transition=(k_size, iterations)` adds the training entry 'transition' from the alphas (utils/groundtruth.py): one frame -> the
        per-instance band of him.py:185-189 in the same slots as 'alpha'; a clip (T > 1) -> the frame-difference rule of vim.py:171-183.
        `trimap=True` adds the evaluation entry 'trimap' (him.py:190-196) from the alphas as given (`ori_alphas`: no `< 5` rule).
        `mask_draws` (a maskgen.MaskDraws for the T * n_i planes, or (MaskDraws, RandomState) when its drop-out is on) sends `masks_u8`
        through the loaders' mask chain first (utils/maskgen.py `synthesize`); image training passes the alphas as `masks_u8` (him.py:103)."""
        return self._assemble(normalize_frames(frames_u8, self.mean, self.std, self.device), alphas_u8, masks_u8, slot_ids, transition, trimap,
                              mask_draws)

    def _assemble(self, image, alphas_u8, masks_u8, slot_ids, transition, trimap, mask_draws):
        """The entries of `__call__` around an `image` that is already the normalised (T, 3, H, W) tensor."""
        out = {'image': image}
        T, _, H, W = out['image'].shape
        n_slots = self.max_inst if slot_ids is not None else None
        if alphas_u8 is not None:
            a = alphas_u8.reshape(T, -1, H, W)
            out['alpha'] = scale_planes(a, n_slots, slot_ids, None, 5, self.device)                      # transforms.py:744
        if masks_u8 is not None:
            m = masks_u8.reshape(T, -1, H, W)
            if mask_draws is not None:
                draws, dropout_random = mask_draws if isinstance(mask_draws, tuple) else (mask_draws, None)
                m = maskgen.synthesize(m, draws, dropout_random, device=self.device)
            size = (H // 8, W // 8) if self.downscale_mask else None                                   # him.py:172-173
            out['mask'] = scale_planes(m, n_slots, slot_ids, size, 0, self.device)
        if transition is not None or trimap:
            if alphas_u8 is None:
                raise ValueError('transition / trimap are made from the alphas: alphas_u8 is missing')
            a = alphas_u8.reshape(T, -1, H, W)
            if transition is not None:
                k_size, iterations = transition
                if T == 1:
                    out['transition'] = groundtruth.transition_gt(a, k_size, iterations, 5, n_slots, slot_ids, self.device)
                else:
                    out['transition'] = groundtruth.diff_transition(a, k_size, iterations, 5, n_slots, device=self.device)
            if trimap:
                out['trimap'] = groundtruth.trimap(a, self.device)
        return out

    def train_item(self, frames_u8, alphas_u8, masks_u8, crop_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None):
        """The training item of him.py:36-65 / vim.py:43-74 from the stacked uint8 arrays after PaddingMultiplyBy (`geometry.resize_short_pad`):
        RandomCropByAlpha + RandomHorizontalFlip from `crop_draws` (a crop.CropDraws: `crop.draw_on_device`), then what `__call__` does on the
        crops -- the mask chain of `mask_draws` (made for the cropped size), `/ 255` into the slots, `transition`. 'image' comes from the crop's
        own Normalize epilogue: the uint8 crop of the frames is never stored. `lut`: a (3, 256) uint8 tone curve for the frames (utils/crop.py).
        Image training passes the alphas as `masks_u8` too (him.py:103); the same object is cropped once."""
        return self._train_item(frames_u8, alphas_u8, masks_u8, crop_draws, None, None, slot_ids, transition, mask_draws, lut, False)

    def train_item_affine(self, frames_u8, alphas_u8, masks_u8, crop_draws, affine_draws, slot_ids=None, *, transition=None, mask_draws=None,
                          lut=None, warp_masks=False):
        """`train_item` with the loaders' RandomAffine (him.py:49, vim.py:55; utils/affine.py) between the crop and the mask chain.
        `affine_draws`: an affine.AffineDraws made for the cropped size (`affine.draw`), or None. None, or draws that did not fire (90 % of
        the items), give `train_item` itself, bit for bit. Fired draws take the raw uint8 crop (with `lut`), the warp of frames and alphas, the
        channel shift and Normalize; 'alpha' and `transition` come from the warped alphas. The reference does not warp the masks: with
        `warp_masks=False` (the image loader, him.py:49-57) the mask chain reads the UNWARPED cropped masks, also when `masks_u8 is alphas_u8`;
        `warp_masks=True` (the video loader, which regenerates the masks from the alphas afterwards, vim.py:55-59) hands it the warped alphas."""
        return self._train_item(frames_u8, alphas_u8, masks_u8, crop_draws, None, affine_draws, slot_ids, transition, mask_draws, lut, warp_masks)

    def train_item_photo(self, frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws=None, slot_ids=None, *, transition=None,
                         mask_draws=None, lut=None, warp_masks=False):
        """`train_item` / `train_item_affine` with the photometric steps that follow the flip in the reference's stream (GammaContrast,
        AdditiveGaussionNoise, JpegCompression: him.py:46-48, vim.py:51-54; utils/photometric.py) between the crop and RandomAffine.
        `photo`: a photometric.PhotoDraws made for the cropped size, or None; `affine_draws`: as in `train_item_affine`, or None.
        None, or draws with neither noise nor quality, give `train_item_affine` itself, bit for bit and as a call of it; a `photo.lut` then
        joins the crop's table, after `lut`, and the crop's own Normalize epilogue stays in use. Otherwise the raw uint8 crop (with `lut`)
        feeds `photometric.apply` (`photo.lut`, the noise, the JPEG round trip): with its Normalize epilogue when no affine fires, raw when
        one does, because the warp reads uint8. Alphas and masks are untouched, as in the reference (the alpha line of JpegCompression is
        commented out). The three methods keep their signatures and share one wiring, `_train_item`."""
        self._check_draws(photo, affine_draws)
        if photo is None or not photo.fired:
            if photo is not None and photo.lut is not None:
                lut = photo.lut if lut is None else photometric.compose_luts(lut, photo.lut, resolve_device(self.device, frames_u8))
            return self.train_item_affine(frames_u8, alphas_u8, masks_u8, crop_draws, affine_draws, slot_ids, transition=transition,
                                          mask_draws=mask_draws, lut=lut, warp_masks=warp_masks)
        return self._train_item(frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws, slot_ids, transition, mask_draws, lut, warp_masks)

    def train_item_motion(self, frames_u8, alphas_u8, masks_u8, crop_draws, motion, photo=None, affine_draws=None, slot_ids=None, *,
                          transition=None, mask_draws=None, lut=None, warp_masks=False):
        """The video training item (vim.py:49-55): `train_item_photo` with MotionBlur (transforms.py:965-1034; utils/motion.py) between
        GammaContrast and AdditiveGaussionNoise. `motion`: a motion_blur.MotionDraws (`motion.draw`), or None. None, or draws that did not
        fire, give `train_item_photo` itself, bit for bit and as a call of it. Fired draws take the raw uint8 crop, on whose table every tone
        curve rides (`lut`, then `photo.lut`: Gamma comes before the blur), and blur the frames and the alphas with the one kernel; noise / JPEG
        and the affine follow as before, and Normalize belongs to the last stage that touches the frames -- the blur's epilogue when neither
        follows. 'alpha', `transition` and the affine read the blurred alphas. The masks: with `masks_u8 is alphas_u8` or `warp_masks=True`
        (the video loader regenerates them from the final alphas, vim.py:58-59) the mask chain reads the blurred (and, with `warp_masks`, warped)
        alphas; separate masks are not blurred, as in the reference."""
        self._check_draws(photo, affine_draws)
        if motion is not None and not isinstance(motion, motion_blur.MotionDraws):
            raise TypeError('motion must be a motion.MotionDraws or None (got %s)' % type(motion).__name__)
        if motion is None or not motion.fired:
            return self.train_item_photo(frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws, slot_ids, transition=transition,
                                         mask_draws=mask_draws, lut=lut, warp_masks=warp_masks)
        if photo is not None:                                                                         # the tone curve precedes the blur
            if photo.lut is not None:
                lut = photo.lut if lut is None else photometric.compose_luts(lut, photo.lut, resolve_device(self.device, frames_u8))
            photo = photometric.PhotoDraws(None, photo.noise, photo.quality, photo.qtable) if photo.fired else None
        return self._train_item(frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws, slot_ids, transition, mask_draws, lut, warp_masks,
                                motion)

    @staticmethod
    def _check_draws(photo, affine_draws):
        if photo is not None and not isinstance(photo, photometric.PhotoDraws):
            raise TypeError('photo must be a photometric.PhotoDraws or None (got %s)' % type(photo).__name__)
        if affine_draws is not None and not isinstance(affine_draws, affine.AffineDraws):
            raise TypeError('affine_draws must be an affine.AffineDraws or None (got %s)' % type(affine_draws).__name__)

    def _train_item(self, frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws, slot_ids, transition, mask_draws, lut, warp_masks,
                    motion=None):
        """The one wiring of the training item, in the order of the reference's stream: crop -> (MotionBlur) -> (noise / JPEG) ->
        (RandomAffine) -> assemble. `photo`: fired PhotoDraws or None (a lone tone curve has joined `lut` by now); `motion`: fired MotionDraws
        or None (then `photo` carries no tone curve). Every routing decision is made here, once; DESIGN.md section 20 has the table of which
        launch writes 'image'."""
        self._check_draws(photo, affine_draws)
        if len(frames_u8.shape) != 4:
            raise ValueError('frames must be (T, H, W, 3) (got shape %s)' % (tuple(frames_u8.shape),))
        warped = affine_draws is not None and affine_draws.fired
        blurred = motion is not None
        # the mask chain reads the final alphas (the video loader's wiring: blurred and / or warped), or the cropped (and blurred) alphas when the
        # masks ARE the alphas, or the cropped masks; only the last makes the crop touch `masks_u8`
        shared, from_alpha = masks_u8 is alphas_u8, (warped or blurred) and warp_masks and masks_u8 is not None
        # Normalize belongs to the last stage that touches the frames: the crop's epilogue, the blur's, the photometric one, or affine.shift_normalize
        f, a, m = crop.apply(frames_u8, alphas_u8, None if (shared or from_alpha) else masks_u8, crop_draws,
                             normalize=photo is None and not warped and not blurred, lut=lut, mean=self.mean, std=self.std, device=self.device)
        if blurred:                                                                                   # reads raw uint8; one kernel for frames and alphas
            f, a = motion_blur.apply(f, a, motion, normalize=photo is None and not warped, mean=self.mean, std=self.std, device=self.device)
        if shared:
            m = a
        if photo is not None:
            f = photometric.apply(f, photo, normalize=not warped, mean=self.mean, std=self.std, device=self.device)
        if warped:                                                                                    # reads raw uint8
            f, a = affine.apply(f, a, affine_draws, self.mean, self.std, device=self.device)
        if from_alpha:
            m = a
        return self._assemble(f, a, m, slot_ids, transition, False, mask_draws)

    def eval_item(self, frames_u8, ori_alphas_u8, masks_u8=None, *, short_size=768, divisor=64, trimap=True):
        """The evaluation item of him.py:151-202 / vim.py:150-209 from decoded files: (T, h, w, 3) uint8 frames (a clip of T equal-sized
        frames in one call; (h, w, 3) is T = 1), (T, n_i, h, w) `ori_alphas`, optionally (T, n_i, h, w) guidance masks of a mask directory.
          'image'  (T, 3, Hp, Wp): ResizeShort + PaddingMultiplyBy + Normalize in one launch (utils/geometry.py), no uint8 intermediate;
          'mask'   from `masks_u8` by nearest resize, padding, the nearest 1/8 of him.py:175-176 when `downscale_mask` is set, `/ 255`, as one
                   index map; without `masks_u8`, from the resized and padded alphas through `maskgen.from_alpha` (him.py:58-59);
          'alpha'  `ori_alphas / 255` at the original size, no `< 5` rule (him.py:152);
          'trimap' from the original alphas (utils/groundtruth.py);
          'transform_info' the list `postprocessing.reverse_transform_tensor` reads."""
        frames = check_u8(frames_u8)
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError('frames must be (T, h, w, 3) or (h, w, 3) (got shape %s)' % (tuple(frames.shape),))
        T, h, w = (int(v) for v in frames.shape[:3])
        p = geometry.plan(h, w, short_size, divisor)
        a = self._item_planes(ori_alphas_u8, T, h, w, 'ori_alphas')
        m = None if masks_u8 is None else self._item_planes(masks_u8, T, h, w, 'masks')
        if m is not None and m.shape[1] != a.shape[1]:
            raise ValueError('masks: expected %d planes per frame like the alphas (got %d)' % (a.shape[1], m.shape[1]))
        image, _ = geometry.resize_pad_normalize(frames, p, mean=self.mean, std=self.std, device=self.device)
        out = {'image': image}
        if m is not None:
            out['mask'] = geometry.resize_pad_planes(m, p, interpolation='nearest', down8=self.downscale_mask, device=self.device)
        else:
            g = maskgen.from_alpha(geometry.resize_pad_planes_u8(a, p, device=self.device), device=self.device)
            size = (p.out_h // 8, p.out_w // 8) if self.downscale_mask else None
            out['mask'] = scale_planes(g, None, None, size, 0, self.device)
        out['alpha'] = scale_planes(a, None, None, None, 0, self.device)
        if trimap:
            out['trimap'] = groundtruth.trimap(a, self.device)
        out['transform_info'] = p.transform_info
        return out

    def predict_item(self, frame_u8, instance_masks_u8, *, short_size=576, divisor=64):
        """demo/maggie_predictor.py:34-50: one (h, w, 3) uint8 frame and its (n, h, w) uint8 instance masks (0 / 255) ->
        ({'image': (1, 1, 3, Hp, Wp), 'mask': (1, 1, n, Hp, Wp)}, transform_info); the masks keep the network's full size there."""
        frame = check_u8(frame_u8)
        if frame.dim() != 3 or frame.shape[-1] != 3:
            raise ValueError('frame must be (h, w, 3) (got shape %s)' % (tuple(frame.shape),))
        h, w = (int(v) for v in frame.shape[:2])
        p = geometry.plan(h, w, short_size, divisor)
        m = self._item_planes(instance_masks_u8, 1, h, w, 'instance_masks')
        image, _ = geometry.resize_pad_normalize(frame[None], p, mean=self.mean, std=self.std, device=self.device)
        mask = geometry.resize_pad_planes(m, p, interpolation='nearest', device=self.device)
        return {'image': image[None], 'mask': mask[None]}, p.transform_info

    @staticmethod
    def _item_planes(x_u8, T, h, w, what):
        """uint8 (T, n, h, w) or (T * n, h, w) planes of an item, n >= 1 -> (T, n, h, w)."""
        x = check_u8(x_u8)
        if x.dim() not in (3, 4) or tuple(x.shape[-2:]) != (h, w):
            raise ValueError('%s: expected (T, n, %d, %d) or (T * n, %d, %d) planes like the frames (got shape %s)' % (what, h, w, h, w, tuple(x.shape)))
        count = int(np.prod(x.shape[:-2]))
        if count < 1 or count % T or (x.dim() == 4 and x.shape[0] != T):
            raise ValueError('%s: %d planes do not make %d frames of at least one instance' % (what, count, T))
        return x.reshape(T, count // T, h, w)
