"""The photometric augmentations of the loaders on the device (HIP kernels of csrc/photometric.hip) -- the three steps the reference runs
between the flip and RandomAffine of a training item (maggie/dataloader/transforms.py:812-924; him.py:46-48, vim.py:51-54):

  ... -> RandomHorizontalFlip -> GammaContrast -> AdditiveGaussionNoise -> JpegCompression -> RandomAffine -> [mask chain] -> ...

  * `quality_from_compression`  imgaug's mapping of its `compression` draw to the JPEG quality it saves with;
  * `quant_tables`              libjpeg's scaling of the Annex K tables for a quality;
  * `PhotoDraws`                one item's draws: the tone curve, the noise sample, the quality (one each for the whole clip, as imgaug's
                                deterministic augmenter applies them);
  * `add_noise`                 clip(int(v) + noise, 0, 255);
  * `jpeg_roundtrip`            tone curve -> noise -> `PIL.Image.save(quality=q)` -> `PIL.Image.open`, raw uint8 or straight to the
                                normalised fp32 tensor;
  * `apply`                     whichever of the three steps the draws hold.

The JPEG step is the lossy part of libjpeg-turbo at Pillow's defaults (baseline, 4:2:0, JDCT_ISLOW, no smoothing, fancy upsampling): colour
conversion, edge replication, 2 x 2 downsampling, the integer forward DCT, quantisation, dequantisation, the integer inverse DCT, triangle
upsampling and the conversion back. The entropy coding is lossless and has no part in the round trip; utils/jpegenc.py
adds it where the file itself is wanted. Everything is int32 work or the IEEE divisions of
Normalize: bit-exact against Pillow itself (tests/test_photometric_cpu.py holds the restatement the device is compared with against Pillow),
no tolerance anywhere. A `PhotoDraws` moved to the device (`.to(device)`) makes `apply` upload nothing and never synchronise, so it can be
captured in a graph and new values written into `lut`, `noise` and `qtable` between replays.

What stays with the caller: the draws themselves (imgaug's generators for the gamma, the noise sample and the compression; no equality with
them is claimed). MotionBlur of the video loader (vim.py:52), which runs between the tone curve and the noise, has its own module:
utils/motion.py (`DevicePreprocessor.train_item_motion` puts the curve on the crop's table so that it precedes the blur). The alphas and masks are not
touched (the reference's alpha line in JpegCompression is commented out). Wrong dtype, rank or size raise before a launch. There is no CPU
fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, images, integer, lut_table, resolve_device, to_device, upload

RAW, NORM = 0, 1                           # MG_PHOTO_RAW / MG_PHOTO_NORM (include/maggie_hip.h)
TILE_ROWS, TILE_COLS, THREADS, MAX_SIDE = 32, 64, 384, 32767      # MG_JPEG_TILE_ROWS / _TILE_COLS / _THREADS / _MAX_SIDE
ROW_PITCH, BLOCK_PITCH = 9, 72             # the LDS layout of an 8 x 8 int32 block in mg_jpeg_ycc, in dwords

# ISO/IEC 10918-1 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def quality_from_compression(c):
    """The JPEG quality imgaug's `compress_jpeg` saves with for a `compression` of c in 0..100: int(clip(round(1 + 99 * (1 - c / 100)), 1, 100)).
    Restated from imgaug's published source; imgaug is not installed where this was written, so the mapping was not run against it, and no
    equality with imgaug's generator (which draws c) is claimed."""
    return int(np.clip(np.round(1 + 99 * (1 - float(c) / 100)), 1, 100))


def _quality(quality):
    q = integer(quality, 'quality')
    if not 1 <= q <= 100:
        raise ValueError('quality must be in 1..100 (got %d)' % q)
    return q


def quant_tables(quality):
    """(2, 64) int32, natural order: the luma and chroma quantisation tables libjpeg derives from `quality` (jpeg_set_quality with
    force_baseline): s = 5000 // q below 50, else 200 - 2 q; t = clip((std * s + 50) // 100, 1, 255)."""
    q = _quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((np.asarray(t, np.int64) * s + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]).astype(np.int32)


def _is(a, torch_dtype, numpy_dtype):
    return a.dtype == torch_dtype if torch.is_tensor(a) else a.dtype == numpy_dtype


def _check_noise(noise):
    if noise is not None:
        a = noise if torch.is_tensor(noise) else np.asarray(noise)
        if not _is(a, torch.int16, np.int16) or len(a.shape) != 3 or a.shape[-1] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError('noise must be int16 of shape (h, w, 1) or (h, w, 3) (got %s %s)' % (a.dtype, tuple(a.shape)))
    return noise


class PhotoDraws:
    """The photometric draws of one item, each None when its step did not fire:
      lut      (3, 256) uint8: the tone curve (GammaContrast as a table);
      noise    int16 (h, w, 1) or (h, w, 3) for the cropped size: the noise sample, the same for every frame of the clip;
      quality  1..100: the JPEG quality of the clip;  qtable  (2, 64) int32: `quant_tables(quality)`, what the kernel reads.
    NumPy arrays as drawn; `.to(device)` gives the same record with device tensors. `apply` with that uploads nothing and does not synchronise:
    capture it in a graph and write new values into `lut`, `noise` and `qtable` between replays (the kernel clamps table entries to 1..255)."""

    def __init__(self, lut=None, noise=None, quality=None, qtable=None):
        self.lut, self.noise = lut_table(lut), _check_noise(noise)
        self.quality = None if quality is None else _quality(quality)
        if qtable is None and self.quality is not None:
            qtable = quant_tables(self.quality)
        if qtable is not None and not _check_quality(qtable):
            raise ValueError('qtable must be an int32 (2, 64) table (got %r)' % (qtable,))
        self.qtable = qtable

    @property
    def fired(self):
        """Whether a step that needs the raw uint8 frames runs (noise or JPEG); the tone curve alone rides on the crop's own `lut`."""
        return self.noise is not None or self.quality is not None

    @property
    def on_device(self):
        return all(torch.is_tensor(a) for a in (self.lut, self.noise, self.qtable) if a is not None)

    def to(self, device=None):
        device = resolve_device(device)
        return PhotoDraws(upload(self.lut, device), upload(self.noise, device), self.quality, upload(self.qtable, device))


def compose_luts(first, second, device):
    """The (3, 256) uint8 table of `first` followed by `second` (either may be None), on `device`; no synchronisation."""
    a, b = lut_table(first, device), lut_table(second, device)
    if a is None or b is None:
        return b if a is None else a
    return torch.gather(b, 1, a.long())


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _frames(frames_u8, noise):
    f, lead, n, h, w = images(frames_u8, 3, 'frames')
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError('the frames must be at most %d pixels a side (got %d x %d)' % (MAX_SIDE, h, w))
    _check_noise(noise)
    if noise is not None and tuple(noise.shape[:2]) != (h, w):
        raise ValueError('the noise was drawn for %d x %d frames (got frames of %d x %d)' % (noise.shape[0], noise.shape[1], h, w))
    return f, lead, n, h, w


def _noise(noise, device):
    if noise is None:
        return None, 1
    noise = upload(noise, device).contiguous()
    return noise, int(noise.shape[-1])


def _check_quality(quality):
    """True for a quantisation table (checked), False for a quality (checked)."""
    if torch.is_tensor(quality) or isinstance(quality, np.ndarray):
        if tuple(quality.shape) != (2, 64) or not _is(quality, torch.int32, np.int32):
            raise ValueError('a quantisation table must be int32 of shape (2, 64) (got %s %s)' % (quality.dtype, tuple(quality.shape)))
        return True
    _quality(quality)
    return False


def _qtable(quality, device):
    """`quality` as the device (2, 64) int32 table: an int 1..100, or a table (array or tensor) that is taken as it is."""
    if _check_quality(quality):
        return upload(quality, device).contiguous()
    return torch.from_numpy(quant_tables(quality)).to(device, non_blocking=True)


def plane_bytes(frames, h, w):
    """The bytes of the decoded component planes between mg_jpeg_ycc and mg_jpeg_rgb."""
    return frames * ((h + 15) // 16 * 16) * ((w + 15) // 16 * 16) * 3 // 2


def _out(n, h, w, epilogue, device):
    return torch.empty((n, 3, h, w) if epilogue == NORM else (n, h, w, 3), dtype=torch.float32 if epilogue == NORM else torch.uint8, device=device)


def _point(f, n, h, w, lut, noise, nc, epilogue, mean, std):
    out = _out(n, h, w, epilogue, f.device)
    if n > 0:
        hip.call('mg_photo_noise', hip.ptr(f), hip.ptr(out), hip.ptr(lut), hip.ptr(noise), c_int(nc), c_long(n), c_int(h), c_int(w),
                 c_int(epilogue), float3(mean), float3(std), hip.stream())
    return out


def _jpeg(f, n, h, w, qtable, lut, noise, nc, epilogue, mean, std):
    out = _out(n, h, w, epilogue, f.device)
    if n > 0:
        planes = torch.empty((plane_bytes(n, h, w),), dtype=torch.uint8, device=f.device)
        hip.call('mg_jpeg_ycc', hip.ptr(f), hip.ptr(planes), hip.ptr(lut), hip.ptr(noise), c_int(nc), hip.ptr(qtable), c_long(n), c_int(h),
                 c_int(w), hip.stream())
        hip.call('mg_jpeg_rgb', hip.ptr(planes), hip.ptr(out), c_long(n), c_int(h), c_int(w), c_int(epilogue), float3(mean), float3(std),
                 hip.stream())
    return out


def _shape(out, lead, h, w, normalize):
    return out.reshape(lead + ((3, h, w) if normalize else (h, w, 3)))


def add_noise(frames_u8, noise, device=None):
    """clip(int(v) + noise, 0, 255) of (..., h, w, 3) uint8 frames; `noise` int16 (h, w, 1) or (h, w, 3), the same for every frame.
    Returns uint8 on the device."""
    if noise is None:
        raise ValueError('noise must be int16 of shape (h, w, 1) or (h, w, 3) (got None)')
    f, lead, n, h, w = _frames(frames_u8, noise)
    f = to_device(f, device)
    nz, nc = _noise(noise, f.device)
    return _shape(_point(f, n, h, w, None, nz, nc, RAW, IMAGENET_MEAN, IMAGENET_STD), lead, h, w, False)


def jpeg_roundtrip(frames_u8, quality, *, lut=None, noise=None, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`lut` -> `noise` -> the JPEG round trip at `quality` (1..100, or a (2, 64) int32 quantisation table) of (..., h, w, 3) uint8 frames.
    Returns uint8 (..., h, w, 3) on the device, or with `normalize` fp32 (..., 3, h, w): ToTensor + Normalize of the uint8 result, the bits
    of `normalize_frames` on it, with no uint8 intermediate. Two launches; the decoded component planes between them stay on the device."""
    _check_quality(quality)
    lut_table(lut)
    f, lead, n, h, w = _frames(frames_u8, noise)
    f = to_device(f, device)
    nz, nc = _noise(noise, f.device)
    out = _jpeg(f, n, h, w, _qtable(quality, f.device), lut_table(lut, f.device), nz, nc, NORM if normalize else RAW, mean, std)
    return _shape(out, lead, h, w, normalize)


def apply(frames_u8, draws, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """The steps `draws` (a PhotoDraws) holds on (..., h, w, 3) uint8 frames, in the reference's order: tone curve, noise, JPEG. Returns
    uint8 (..., h, w, 3) on the device, or with `normalize` the normalised fp32 (..., 3, h, w). With a quality: the two launches of
    `jpeg_roundtrip` (curve and noise ride on its load); otherwise one launch of the curve and / or the saturating add; draws with nothing
    set give the frames themselves, or the bits of `normalize_frames` of them (at any size: the pointwise launch with nothing to apply)."""
    if not isinstance(draws, PhotoDraws):
        raise TypeError('draws must be a PhotoDraws (got %s)' % type(draws).__name__)
    f, lead, n, h, w = _frames(frames_u8, draws.noise)
    f = to_device(f, device)
    dev = f.device
    epilogue = NORM if normalize else RAW
    if draws.quality is None and draws.noise is None and draws.lut is None and not normalize:
        return f
    lut = lut_table(draws.lut, dev)
    nz, nc = _noise(draws.noise, dev)
    if draws.quality is not None:
        out = _jpeg(f.reshape(n, h, w, 3), n, h, w, _qtable(draws.qtable, dev), lut, nz, nc, epilogue, mean, std)
    else:
        out = _point(f.reshape(n, h, w, 3), n, h, w, lut, nz, nc, epilogue, mean, std)
    return _shape(out, lead, h, w, normalize)
