"""PNG files written from device planes (HIP kernels of csrc/pngenc.hip) -- the result writer of the evaluation, the reference's
`save_visualization` (maggie/engine/test.py:20-68): `(alphas * 255).astype('uint8')`, `> 0.5`, and one `cv2.imwrite` per instance. The planes
stay on the device; what comes back to the host is the compressed stream, tens of KB for a matte instead of its 8 MB of fp32.

  * `encode_planes`       P planes of one size (P, h, w) -> P complete PNG files (bytes) from ONE pair of launches.
  * `encode`              one plane (h, w) -> bytes.
  * `encode_stats`        the same, returning the block records, the stream sizes, the blob and the guard slices: for the tests and
                          tools/pngenc_bench.py.
  * `encode_images`       N colour images of one size (N, h, w, C), C = 3 (RGB, colour type 2) or 4 (RGBA, colour type 6) -> N complete
                          PNG files, the writer of `cutout.save_cutouts`; `encode_image` one image, `encode_images_stats` the `Encoded` record.
                          Only the filtered stream differs (Sub with the filter distance C); tokens, Huffman codes, emit and Adler-32 are
                          the grey path's.
  * `save_visualization`  the reference's signature, directory and file-name rule; `functools.partial(save_visualization, save_dir=...)` is
                          the `callback` of `eval_image` / `eval_video`.

Input forms (`mode`): 'u8' uint8 samples as they are; 'unit' float32 with byte = (uint8)(x * 255.0f), which is the reference's
`(alphas * 255).astype('uint8')` in float32 for x in [0, 1]; 'threshold' float32 with byte = 255 if x > 0.5 else 0, the `inc_bin_maps` form.
For 'unit' NaN and x < 0 give 0 and x > 1 gives 255: NumPy leaves the cast of such values to uint8 undefined (it wraps on one platform and
saturates on another), so there is nothing to match there. The conversion happens on the kernels' loads; no uint8 copy of a plane is stored.

The files are 8-bit greyscale, non-interlaced, one IDAT, Sub filter on every row, deflate blocks of `BLOCK_BYTES` filtered bytes whose tokens
are runs (distance 1), each block fixed or dynamic Huffman by exact bit count. PNG is lossless: the contract is not
byte equality with another writer but that every reader returns exactly the bytes the reference would have written; tests/pngenc_restatement.py
is the byte-for-byte oracle of this encoder itself. `pngdec.decode_planes(encode_planes(x))` returns x on the device.

Two launches (`mg_pngenc_size`, `mg_pngenc_emit`) with the sizes read back in between, then exactly the streams' bytes: two read-backs per
call, so none of this is graph-capturable. The host adds the signature, IHDR, the IDAT length and `zlib.crc32`, and IEND. Wrong types and
shapes raise before any launch. There is no CPU fallback."""
import os
import struct
import zlib

import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import need_gpu, resolve_device

THREADS, BLOCK_BYTES, REC_WORDS = 256, 16384, 88              # MG_PNGENC_THREADS / _BLOCK_BYTES / _REC_WORDS
MAX_SIDE, MAX_WIDTH, MAX_RAW, MAX_PLANES = 32767, 16384, (1 << 30) - 16, 65536      # MG_PNGENC_MAX_SIDE / _MAX_WIDTH / _MAX_RAW / _MAX_PLANES
MODES = {'u8': 0, 'unit': 1, 'threshold': 2}                  # MG_PNGENC_MODE_*
SIGNATURE = b'\x89PNG\r\n\x1a\n'
IEND = struct.pack('>I', 0) + b'IEND' + struct.pack('>I', zlib.crc32(b'IEND'))


COLOUR_TYPE = {1: 0, 3: 2, 4: 6}                              # channels -> the IHDR colour type


def frame(h, w, stream, channels=1):
    """The PNG file around one zlib stream: signature, IHDR (8-bit, greyscale or for 3 / 4 channels RGB / RGBA, non-interlaced), one IDAT,
    IEND. Host only."""
    ihdr = b'IHDR' + struct.pack('>IIBBBBB', w, h, 8, COLOUR_TYPE[channels], 0, 0, 0)
    idat = b'IDAT' + bytes(stream)
    return b''.join((SIGNATURE, struct.pack('>I', 13), ihdr, struct.pack('>I', zlib.crc32(ihdr)),
                     struct.pack('>I', len(idat) - 4), idat, struct.pack('>I', zlib.crc32(idat)), IEND))


def blocks_of(h, w):
    return -(-(h * (w + 1)) // BLOCK_BYTES)


def _check(planes, mode):
    """Type and shape checks, before anything touches the device -> the tensor (an array becomes a host tensor)."""
    if mode not in MODES:
        raise ValueError("mode must be 'u8', 'unit' or 'threshold' (got %r)" % (mode,))
    if isinstance(planes, np.ndarray):
        planes = torch.from_numpy(np.ascontiguousarray(planes))
    if not torch.is_tensor(planes):
        raise TypeError('planes must be a tensor or an array (got %s)' % type(planes).__name__)
    want = torch.uint8 if mode == 'u8' else torch.float32
    if planes.dtype != want:
        raise TypeError("mode %r takes %s planes (got %s)" % (mode, want, planes.dtype))
    if planes.dim() != 3:
        raise ValueError('planes must be (P, h, w) (got %s)' % (tuple(planes.shape),))
    P, h, w = planes.shape
    if not 1 <= P <= MAX_PLANES:
        raise ValueError('1..%d planes a call (got %d)' % (MAX_PLANES, P))
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_WIDTH or h * (w + 1) > MAX_RAW:
        raise ValueError('heights of 1..%d and widths of 1..%d are written (got %d x %d)' % (MAX_SIDE, MAX_WIDTH, h, w))
    if P * blocks_of(h, w) > 0x7fffffff:
        raise ValueError('%d planes of %d x %d are more deflate blocks than one launch takes' % (P, h, w))
    return planes


class Encoded:
    """What `run` leaves: `files` (P bytes objects), on the host `sizes` int64 (P,), `streams` (the zlib streams), `readbacks`; with
    stats=True also `recs` int32 (P, blocks, REC_WORDS) and `blob` (the device blob, uint8); with a guard `guards`, six slices of 0xA5
    around the record table, the size table and the blob, and `slack`, the zeroed bytes behind the last stream."""


def _guarded(nbytes, guard, dev, fill=None):
    """`nbytes` of device memory (16-byte aligned) between two guards of 0xA5 -> (the slice, [front guard, back guard])."""
    if not guard:
        return (torch.empty if fill is None else torch.zeros)((nbytes,), dtype=torch.uint8, device=dev), []
    buf = torch.full((2 * guard + nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    mid = buf[guard:guard + nbytes]
    if fill is not None:
        mid.zero_()
    return mid, [buf[:guard], buf[guard + nbytes:]]


def run(x, mode, *, guard=0, stats=False):
    """The launches themselves: `x` a contiguous device tensor (P, h, w) of the mode's type, or uint8 (N, h, w, C) with C = 3 or 4 (the colour
    entries). `guard`: bytes of 0xA5 kept on both sides of the record table, the size table and the blob. Returns an `Encoded`."""
    hip.need_cuda(x)
    channels = int(x.shape[3]) if x.dim() == 4 else 1
    P, h, w = (int(v) for v in x.shape[:3])
    nb = blocks_of(h, channels * w)
    if channels == 1:
        size_entry, emit_entry, form = 'mg_pngenc_size', 'mg_pngenc_emit', c_int(MODES[mode])
    else:
        size_entry, emit_entry, form = 'mg_pngenc_size_rgb', 'mg_pngenc_emit_rgb', c_int(channels)
    dev = x.device
    guard = -(-guard // 16) * 16
    with torch.cuda.device(dev):
        rec_b, g1 = _guarded(-(-(P * nb * REC_WORDS * 4) // 16) * 16, guard, dev)
        size_b, g2 = _guarded(-(-(P * 8) // 16) * 16, guard, dev)
        recs, sizes = rec_b.view(torch.int32), size_b.view(torch.int64)
        st = hip.stream
        hip.call(size_entry, hip.ptr(x), form, c_long(P), c_int(h), c_int(w), hip.ptr(recs), hip.ptr(sizes), st())
        host_sizes = sizes[:P].cpu().numpy()                                   # read-back 1
        total = int(host_sizes.sum())
        padded = max(-(-total // 4) * 4, 8)
        blob, g3 = _guarded(padded, guard, dev, fill=0)
        hip.call(emit_entry, hip.ptr(x), form, c_long(P), c_int(h), c_int(w), hip.ptr(recs), hip.ptr(sizes), hip.ptr(blob),
                 c_long(padded), st())
        data = blob[:total].cpu().numpy().tobytes()                            # read-back 2: exactly the bytes
    r = Encoded()
    ends = np.cumsum(host_sizes)
    r.sizes, r.readbacks = host_sizes, 2
    r.streams = [data[int(e - s):int(e)] for s, e in zip(host_sizes, ends)]
    r.files = [frame(h, w, s, channels) for s in r.streams]
    if stats:
        r.recs = recs[:P * nb * REC_WORDS].cpu().numpy().reshape(P, nb, REC_WORDS)
        r.blob, r.slack, r.guards = blob[:total], blob[total:], g1 + g2 + g3
    return r


def _encode(planes, mode, device, guard=0, stats=False):
    x = _check(planes, mode)
    need_gpu(x)
    x = x.to(resolve_device(device, x), non_blocking=True).contiguous()
    return run(x, mode, guard=guard, stats=stats)


def encode_planes(planes, *, mode='u8', device=None):
    """P planes of one size, (P, h, w) device tensor (an array or a host tensor is uploaded) -> a list of P bytes objects, each a complete PNG
    file whose pixels are the plane's bytes under `mode` (module docstring). One `mg_pngenc_size` and one `mg_pngenc_emit` for the whole
    call, two read-backs. TypeError for a dtype that is not the mode's, ValueError for a wrong shape or a size outside 1..32767 x 1..16384,
    both before any launch. Not graph-capturable."""
    return _encode(planes, mode, device).files


def encode(plane, *, mode='u8', device=None):
    """One plane (h, w) -> the bytes of its PNG file."""
    if not (torch.is_tensor(plane) or isinstance(plane, np.ndarray)) or plane.ndim != 2:
        raise ValueError('plane must be a tensor or an array of shape (h, w)')
    return _encode(plane[None], mode, device).files[0]


def encode_stats(planes, *, mode='u8', device=None, guard=0):
    """`encode_planes` returning the whole `Encoded` record (block records, sizes, blob, guard slices): for the tests and
    tools/pngenc_bench.py. One more read-back (the records) than `encode_planes`."""
    return _encode(planes, mode, device, guard=guard, stats=True)


def _check_images(images):
    """Type and shape checks of the colour form, before anything touches the device -> the tensor (an array becomes a host tensor)."""
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images))
    if not torch.is_tensor(images):
        raise TypeError('images must be a tensor or an array (got %s)' % type(images).__name__)
    if images.dtype != torch.uint8:
        raise TypeError('colour images are uint8 (got %s)' % images.dtype)
    if images.dim() != 4 or images.shape[3] not in (3, 4):
        raise ValueError('images must be (N, h, w, 3) or (N, h, w, 4) (got %s)' % (tuple(images.shape),))
    N, h, w, C = (int(v) for v in images.shape)
    if not 1 <= N <= MAX_PLANES:
        raise ValueError('1..%d images a call (got %d)' % (MAX_PLANES, N))
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_WIDTH // C or h * (C * w + 1) > MAX_RAW:
        raise ValueError('heights of 1..%d and, with %d channels, widths of 1..%d are written (got %d x %d)' % (MAX_SIDE, C, MAX_WIDTH // C, h, w))
    if N * blocks_of(h, C * w) > 0x7fffffff:
        raise ValueError('%d images of %d x %d are more deflate blocks than one launch takes' % (N, h, w))
    return images


def _encode_images(images, device, guard=0, stats=False):
    x = _check_images(images)
    need_gpu(x)
    x = x.to(resolve_device(device, x), non_blocking=True).contiguous()
    return run(x, 'u8', guard=guard, stats=stats)


def encode_images(images_u8, *, device=None):
    """N colour images of one size, uint8 (N, h, w, C) with C = 3 (RGB) or 4 (straight RGBA), a device tensor (an array or a host tensor is
    uploaded) -> a list of N bytes objects, each a complete PNG file of colour type 2 / 6: 8-bit, non-interlaced, one IDAT, Sub filter on every
    row with the filter distance C, the grey path's deflate. A row of the filtered stream is 1 + C * w bytes, and `MAX_WIDTH` (16384) bounds
    the BYTES of a row in the grey path (a grey row is w bytes; `pngdec` reads back rows of at most MAX_ROWBYTES = 16384 bytes), so a colour
    row is held to the same C * w <= 16384: w <= 5461 for RGB and w <= 4096 for RGBA, h <= 32767, h * (C * w + 1) <= MAX_RAW
    (`pngcolor.decode_frames` reads all of these back). TypeError for another dtype,
    ValueError for a wrong shape or a size beyond these, both before any launch. One `mg_pngenc_size_rgb` and one `mg_pngenc_emit_rgb`, two
    read-backs. Not graph-capturable."""
    return _encode_images(images_u8, device).files


def encode_image(image_u8, *, device=None):
    """One image (h, w, 3) or (h, w, 4) -> the bytes of its PNG file."""
    if not (torch.is_tensor(image_u8) or isinstance(image_u8, np.ndarray)) or image_u8.ndim != 3:
        raise ValueError('image must be a tensor or an array of shape (h, w, 3) or (h, w, 4)')
    return _encode_images(image_u8[None], device).files[0]


def encode_images_stats(images_u8, *, device=None, guard=0):
    """`encode_images` returning the whole `Encoded` record (block records, sizes, blob, guard slices): for the tests and
    tools/cutout_bench.py. One more read-back (the records) than `encode_images`."""
    return _encode_images(images_u8, device, guard=guard, stats=True)


def _png_name(name):
    """The diff_pred / inc_pred branches name their file after the frame. cv2.imwrite picks the format by the extension; this writer only has
    PNG, so a frame that is not `.png` keeps its stem and takes that extension."""
    return name if name.lower().endswith('.png') else os.path.splitext(name)[0] + '.png'


def plan_paths(image_names, alpha_names, n_inst, has_diff, has_inc):
    """The reference's directory and file-name rule, host only -> [(kind, (frame, instance), path relative to save_dir)] with kind 'alpha',
    'diff' or 'inc', in the reference's order of writing."""
    out = []
    for idx in range(len(image_names)):
        video_name, image_name = image_names[idx][0].split('/')[-2:]
        for inst in range(n_inst):
            target = os.path.join(video_name, image_name[:-4])
            if alpha_names is not None:
                target = os.path.join(target, alpha_names[inst][0])
            elif n_inst > 1:
                target = os.path.join(target, '{:2d}.png'.format(inst).replace(' ', '0'))
            else:
                target = target + '.png'
            out.append(('alpha', (idx, inst), target))
        if has_diff:
            out.append(('diff', (idx, 0), os.path.join('diff_pred', video_name, _png_name(image_name))))
        if has_inc:
            out.append(('inc', (idx, 0), os.path.join('inc_pred', video_name, _png_name(image_name))))
    return out


def _planes_on(x, dev):
    """alphas / a prediction as a device tensor, uint8 or float32. Another float type (fp16, bf16, float64) is widened or narrowed to float32
    first, so its bytes are (uint8)(float32(x) * 255.0f), where the reference's NumPy would multiply in the array's own type."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype != torch.uint8 and x.dtype != torch.float32:
        x = x.float()
    return x.to(dev, non_blocking=True)


@torch.no_grad()
def save_visualization(image_names, alpha_names, alphas, transform_info, output, save_dir):
    """The reference's result writer on device planes. `alphas` (1, T, n_i, H, W), float32 in [0, 1] (other float types are converted
    to float32 first) or uint8 bytes, a device tensor or an array (uploaded); `output['diff_pred']` (1, T, 1, h, w) and `output['inc_bin_maps'][0]` (1, T, 1, h, w) go through
    `reverse_transform_tensor` first, as in the reference. Writes save_dir/<video>/<frame>/<alpha name> (or /NN.png, or <frame>.png for a
    single instance), save_dir/diff_pred/<video>/<frame name> and save_dir/inc_pred/<video>/<frame name>, the last two only where the file
    does not exist yet. All planes of one size and mode go through ONE `encode_planes`; no fp32 plane is copied to the host."""
    from .postprocessing import reverse_transform_tensor
    like = next((t for t in (alphas, output.get('diff_pred')) if torch.is_tensor(t) and t.is_cuda), None)
    dev = resolve_device(None, like)
    a = _planes_on(alphas, dev)
    if a.dim() != 5:
        raise ValueError('alphas must be (1, T, n_i, H, W) (got %s)' % (tuple(a.shape),))
    diff = inc = None
    if 'diff_pred' in output:
        diff = reverse_transform_tensor(_planes_on(output['diff_pred'], dev).float(), transform_info)
    if 'inc_bin_maps' in output:
        inc = reverse_transform_tensor(_planes_on(output['inc_bin_maps'][0], dev).float(), transform_info)
    source = {'alpha': (a, 'u8' if a.dtype == torch.uint8 else 'unit'), 'diff': (diff, 'unit'), 'inc': (inc, 'threshold')}
    groups, seen = {}, set()
    for kind, (idx, inst), rel in plan_paths(image_names, alpha_names, a.shape[2], diff is not None, inc is not None):
        path = os.path.join(save_dir, rel)
        if kind != 'alpha' and (path in seen or os.path.isfile(path)):
            continue
        seen.add(path)
        t, mode = source[kind]
        plane = t[0, idx, inst]
        groups.setdefault((tuple(plane.shape), mode), []).append((plane, path))
    for (_, mode), items in groups.items():
        files = encode_planes(torch.stack([p for p, _ in items]), mode=mode)
        for (_, path), data in zip(items, files):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'wb') as f:
                f.write(data)
