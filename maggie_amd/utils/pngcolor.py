"""Every legal PNG file decoded on the device (HIP kernels of csrc/pngcolor.hip): the frame half of the reference's `T.Load` for `.png` files
(maggie/dataloader/transforms.py:47-50, `Image.open(path).convert("RGB")`), and the alpha / mask half for the files `pngdec.parse` refuses:
16-bit samples and Adam7 interlace. All 15 (colour type, bit depth) pairs, interlaced or not, byte for byte equal to Pillow 12 (DESIGN.md
section 34):

    grey 1 / 2 / 4 / 8        sample x 255 / 85 / 17 / 1, replicated             L: the same value
    grey 16                   min(v, 255), replicated -- Pillow's I;16 conversion SATURATES, it does not take the high byte; this is what the
                              reference's loader gets, so it is what the device returns
    RGB 8 / 16                the bytes / the high bytes                          L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16
    palette 1 / 2 / 4 / 8     the PLTE entry                                      L: the luma of the entry
    grey + alpha 8 / 16       the grey byte / high byte, replicated; RGBA 8 / 16: the RGB bytes / high bytes. Alpha is dropped, not applied.

tRNS and the ancillary chunks (gAMA, sRGB, iCCP, ...) change nothing. A palette index past the last PLTE entry is an error here (status bit INDEX,
ValueError); Pillow returns black.

  * `parse`           the chunk walk of `pngdec` under this module's rules -> a `pngdec.PngPlan` with `interlace`, `passes` (the per-pass table)
                      and `raw_size` (the sum over the passes). `Unsupported` for an unknown critical chunk, sides above 32767, a row above
                      MAX_ROWBYTES, raw bytes above `pngdec.MAX_RAW`, a stream above `pngdec.MAX_BYTES`; ValueError for a broken file.
  * `decode_frames` / `decode_frame`   T files of one size (type, depth, interlace per file) -> uint8 (T, h, w, 3), or with `normalize` fp32
                      (T, 3, h, w) with the bits of `normalize_frames`.
  * `decode_planes` / `decode`         the L planes, the contract of `pngdec.decode_planes`.
  * `decode_stats`    the whole record (defiltered bytes, status words, counters, read-backs): for the tests and tools/pngcolor_bench.py.
  * `load_planes`     what a loader calls for alphas and masks: `pngdec.parse` first, then `parse`.
  * `load_frames`     the frame half of `T.Load` for any file: FF D8 files through `jpegsamp.load_clip`, PNG files through `decode_frames`.

Three launches: `mg_pngcolor_inflate` (one wave per file, the algorithm of `mg_pngdec_inflate`), `mg_pngcolor_unfilter` (one wave per pass of
a file, in place) and `mg_pngcolor_convert` (16 pixels a lane). ONE read-back per set of launches; a status bit becomes a ValueError. Not
graph-capturable. Wrong types raise before any launch. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import jpegsamp, pngdec
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, resolve_device
from .jpegdec import Unsupported
from .pngdec import CHANNELS, INFO_WORDS, MAX_BYTES, MAX_RAW, MAX_SIDE, SIGNATURE, STATUS, THREADS

REC_WORDS, REC_PASSES, REC_LTABLE, REC_PALETTE = 292, 8, 36, 100       # MG_PNGCOLOR_REC_WORDS / _REC_PASSES / _REC_LTABLE / _REC_PALETTE
MAX_ROWBYTES, GROUP = 32768, 16                                        # MG_PNGCOLOR_MAX_ROWBYTES / _GROUP
OUT_RGB, OUT_L, OUT_NORM = 0, 1, 2                                     # MG_PNGCOLOR_OUT_*
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))     # (x0, y0, dx, dy) of the passes


def passes(w, h, color_type, depth, interlace):
    """The per-pass table of a file: [(pw, ph, rb, offset)] -- 7 entries for Adam7, else 1 -- with pw = ceil((w - x0) / dx),
    ph = ceil((h - y0) / dy), rb = ceil(pw x channels x depth / 8) and offset = the sum of ph x (1 + rb) over the non-empty passes in front.
    Returns (table, that sum over all passes)."""
    table, off = [], 0
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        pw, ph = max(0, -(-(w - x0) // dx)), max(0, -(-(h - y0) // dy))
        rb = (pw * CHANNELS[color_type] * depth + 7) // 8
        table.append((pw, ph, rb, off))
        if pw and ph:
            off += ph * (1 + rb)
    return table, off


def _accepts(w, h, depth, ct, lace):
    if w > MAX_SIDE or h > MAX_SIDE:
        raise Unsupported('%d x %d: sides up to %d are decoded' % (w, h, MAX_SIDE))
    rb = pngdec.rowbytes(ct, depth, w)
    if rb > MAX_ROWBYTES:
        raise Unsupported('%d bytes a row: rows up to %d bytes are decoded' % (rb, MAX_ROWBYTES))
    size = passes(w, h, ct, depth, lace)[1]
    if size > MAX_RAW - 16:
        raise Unsupported('%d inflated bytes: up to %d are decoded' % (size, MAX_RAW - 16))
    return size


def parse(data):
    """The chunk walk of one file's bytes -> `pngdec.PngPlan`, with `interlace`, `passes` and `raw_size` the sum over them. Host only. Accepts
    every legal (colour type, depth, interlace); `Unsupported` for an unknown critical chunk and the limits of the module docstring, ValueError
    for a broken file, as `pngdec.parse`."""
    plan = pngdec.walk(data, _accepts)
    plan.passes = passes(plan.width, plan.height, plan.color_type, plan.depth, plan.interlace)[0]
    return plan


def record(plan, offset):
    """A file's int32 record (MG_PNGCOLOR_REC_WORDS words, include/maggie_hip.h) with its zlib stream at `offset` of the buffer."""
    rec = np.zeros(REC_WORDS, np.int32)
    rec[0:7] = offset, len(plan.stream), plan.color_type, plan.depth, plan.entries, plan.interlace, plan.raw_size
    for k, row in enumerate(plan.passes):
        rec[REC_PASSES + 4 * k:REC_PASSES + 4 * k + 4] = row
    rec[REC_LTABLE:REC_LTABLE + 64] = plan.ltable.view(np.int32)
    if plan.palette is not None:
        pal = np.zeros(768, np.uint8)
        pal[:3 * len(plan.palette)] = plan.palette.reshape(-1)
        rec[REC_PALETTE:REC_PALETTE + 192] = pal.view(np.int32)
    return rec


class Decoded:
    """What `run` leaves: on the device `out` (uint8 (T, h, w, 3), uint8 (T, h, w) or float32 (T, 3, h, w)) and `raw` uint8 (T, raw_stride),
    the DEFILTERED scanlines of file t (each behind its filter type byte, pass after pass) in raw[t, :raw_sizes[t]]; on the host `info` int32
    (T, INFO_WORDS), `status`, `rounds`, `blocks`, `tokens` (arrays over the files), `launches` and `readbacks`."""


def run(blob, recs, h, w, mode, *, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, guard=0):
    """The launches themselves: `blob` uint8 device tensor holding the T zlib streams, `recs` int32 (T, REC_WORDS) host records whose offsets
    point into it, `mode` OUT_RGB, OUT_L or OUT_NORM. `out`: a preallocated contiguous destination of the mode's dtype and size (it may start
    at any byte). `guard`: bytes of 0xA5 kept on both sides of `raw` and of an allocated `out` (for the tests: `Decoded.guards`)."""
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, REC_WORDS)
    T = recs.shape[0]
    dev = blob.device
    hip.need_cuda(blob)
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError('blob must be a contiguous 1-D uint8 tensor')
    if mode not in (OUT_RGB, OUT_L, OUT_NORM):
        raise ValueError('mode must be OUT_RGB, OUT_L or OUT_NORM')
    if T < 1 or (recs[:, 0] < 0).any() or (recs[:, 1] < 0).any() or int((recs[:, 0].astype(np.int64) + recs[:, 1]).max()) > blob.numel():
        raise ValueError('a zlib stream lies outside the buffer')
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_SIDE:
        raise ValueError('sides of 1..%d are decoded (got %d x %d)' % (MAX_SIDE, h, w))
    sizes = [int(v) for v in recs[:, 6]]
    if min(sizes) < 1 or max(sizes) > MAX_RAW - 16:
        raise ValueError('a record with an inflated size outside 1..%d' % (MAX_RAW - 16))
    mean3, std3 = float3(mean), float3(std)
    stride = -(-max(sizes) // 16) * 16
    guard = -(-guard // 16) * 16
    tabs = torch.from_numpy(recs).to(dev, non_blocking=True)
    rawbuf = torch.full((2 * guard + T * stride,), 0xA5, dtype=torch.uint8, device=dev) if guard else \
        torch.empty((T * stride,), dtype=torch.uint8, device=dev)
    raw = rawbuf[guard:guard + T * stride]
    info = torch.zeros((T, INFO_WORDS), dtype=torch.int32, device=dev)
    n = T * h * w * (1 if mode == OUT_L else 3)
    dtype = torch.float32 if mode == OUT_NORM else torch.uint8
    shape = (T, h, w) if mode == OUT_L else ((T, h, w, 3) if mode == OUT_RGB else (T, 3, h, w))
    outbuf = None
    if out is None:
        if guard and mode != OUT_NORM:
            outbuf = torch.full((2 * guard + n,), 0xA5, dtype=dtype, device=dev)
            out = outbuf[guard:guard + n]
        else:
            out = torch.empty((n,), dtype=dtype, device=dev)
    elif not torch.is_tensor(out) or out.numel() != n or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous %s tensor of %d elements on %s' % (str(dtype).split('.')[-1], n, dev))
    st = hip.stream
    size = (c_long(T), c_int(h), c_int(w))
    hip.call('mg_pngcolor_inflate', hip.ptr(blob), c_long(blob.numel()), hip.ptr(tabs), hip.ptr(raw), c_long(stride), hip.ptr(info), *size, st())
    hip.call('mg_pngcolor_unfilter', hip.ptr(raw), c_long(stride), hip.ptr(tabs), hip.ptr(info), *size, st())
    hip.call('mg_pngcolor_convert', hip.ptr(raw), c_long(stride), hip.ptr(tabs), hip.ptr(out), hip.ptr(info), *size, c_int(mode), mean3, std3, st())
    host = info.cpu().numpy()
    r = Decoded()
    r.out, r.raw, r.raw_sizes, r.raw_stride, r.info = out.reshape(shape), raw.reshape(T, stride), sizes, stride, host
    r.status, r.rounds, r.blocks, r.tokens = host[:, 0].copy(), host[:, 1].copy(), host[:, 2].copy(), host[:, 3].copy()
    r.launches, r.readbacks = 3, 1
    r.guards = [] if not guard else [rawbuf[:guard], rawbuf[guard + T * stride:]] + \
        ([] if outbuf is None else [outbuf[:guard], outbuf[guard + n:]])
    for k in range(T):
        if host[k, 0]:
            raise ValueError('file %d: a corrupt PNG data stream: %s' % (k, '; '.join(v for b, v in STATUS.items() if host[k, 0] & b)))
    return r


def _datas(datas):
    if isinstance(datas, (bytes, bytearray, memoryview)) or not hasattr(datas, '__len__'):
        raise TypeError('datas must be a sequence of the bytes of PNG files (got %s)' % type(datas).__name__)
    if len(datas) < 1:
        raise ValueError('datas must hold at least one file')


def _one(data):
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a PNG file (got %s)' % type(data).__name__)
    return [data]


def run_plans(plans, mode, mean, std, device, out):
    """One set of launches for parsed files of one size."""
    if any(p.size != plans[0].size for p in plans):
        raise ValueError('the files of one call must share one size (got %s)' % sorted({p.size for p in plans}))
    offsets = np.concatenate([[0], np.cumsum([-(-len(p.stream) // 4) * 4 for p in plans])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of zlib streams in one call' % offsets[-1])
    recs = np.stack([record(p, int(o)) for p, o in zip(plans, offsets[:-1])])
    device = resolve_device(device, out if torch.is_tensor(out) else None)
    buf = bytearray(int(offsets[-1]))
    for p, o in zip(plans, offsets[:-1]):
        buf[int(o):int(o) + len(p.stream)] = p.stream
    blob = torch.frombuffer(buf, dtype=torch.uint8).to(device, non_blocking=True)
    h, w = plans[0].size
    return run(blob, recs, h, w, mode, mean=mean, std=std, out=out)


def _files(datas, mode, mean, std, device, out):
    _datas(datas)
    float3(mean), float3(std)
    return run_plans([parse(d) for d in datas], mode, mean, std, device, out)


def decode_frames(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """T PNG files (a sequence of bytes objects) of one size -> uint8 (T, h, w, 3) on the device, each frame `convert("RGB")` of its file, from
    one set of launches with one read-back; colour type, depth and interlace may differ per file. With `normalize` fp32 (T, 3, h, w): ToTensor
    + Normalize, the bits of `normalize_frames`. `out`: a contiguous destination of that dtype and size. Files of differing size raise
    ValueError, unsupported ones `Unsupported`, a corrupt stream ValueError. Not graph-capturable."""
    return _files(datas, OUT_NORM if normalize else OUT_RGB, mean, std, device, out).out


def decode_frame(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """The bytes of one PNG file -> uint8 (h, w, 3) on the device: `np.asarray(Image.open(BytesIO(data)).convert("RGB"))`; with `normalize`
    fp32 (3, h, w). Not graph-capturable; one read-back."""
    return _files(_one(data), OUT_NORM if normalize else OUT_RGB, mean, std, device, out).out[0]


def decode_planes(datas, *, device=None, out=None):
    """P PNG files of one size -> uint8 (P, h, w) on the device, each plane `convert("L")` of its file: the contract of
    `pngdec.decode_planes` for everything `parse` accepts. Not graph-capturable."""
    return _files(datas, OUT_L, IMAGENET_MEAN, IMAGENET_STD, device, out).out


def decode(data, *, device=None):
    """The bytes of one PNG file -> uint8 (h, w) on the device: `np.asarray(Image.open(BytesIO(data)).convert("L"))`."""
    return _files(_one(data), OUT_L, IMAGENET_MEAN, IMAGENET_STD, device, None).out[0]


def decode_stats(datas, *, planes=False, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """`decode_frames` (or with `planes` `decode_planes`) returning the whole `Decoded` record. Not graph-capturable."""
    return _files(datas, OUT_L if planes else (OUT_NORM if normalize else OUT_RGB), mean, std, device, out)


def load_planes(datas, *, device=None):
    """`decode_planes` for whatever a loader finds: each file goes to `pngdec.parse` first, then to `parse`; if neither takes it, the
    `Unsupported` of `pngdec.parse` propagates. The files share one size; the files of each module are decoded in one set of launches into a
    slice of one tensor, and the result is in the order of `datas`. One read-back per group."""
    _datas(datas)
    found = []
    for d in datas:
        try:
            found.append((0, pngdec.parse(d)))
        except Unsupported as refusal:
            try:
                found.append((1, parse(d)))
            except Unsupported:
                raise refusal from None
    sizes = sorted({p.size for _, p in found})
    if len(sizes) > 1:
        raise ValueError('the files of one call must share one size (got %s)' % sizes)
    device = resolve_device(device)
    (h, w), P = sizes[0], len(datas)
    order = [k for which in (0, 1) for k in range(P) if found[k][0] == which]
    first = sum(1 for which, _ in found if which == 0)
    out = torch.empty((P, h, w), dtype=torch.uint8, device=device)
    if first:
        pngdec.decode_planes([datas[k] for k in order[:first]], device=device, out=out[:first])
    if first < P:
        run_plans([found[k][1] for k in order[first:]], OUT_L, IMAGENET_MEAN, IMAGENET_STD, device, out[first:])
    if order == list(range(P)):
        return out
    back = np.empty(P, np.int64)
    back[order] = np.arange(P)
    return out[torch.from_numpy(back).to(device)]


def load_frames(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """The frame half of `T.Load` for any file: the signature decides. FF D8 files go through `jpegsamp.load_clip`, PNG files through
    `decode_frames`; a mixed clip of one size is decoded per kind into slices of one tensor, and the result -- uint8 (T, h, w, 3), or with
    `normalize` fp32 (T, 3, h, w) -- is in the order of `datas`. Anything else raises ValueError. Not graph-capturable."""
    _datas(datas)
    float3(mean), float3(std)
    kinds = []
    for k, d in enumerate(datas):
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError('datas must hold the bytes of files (got %s)' % type(d).__name__)
        head = bytes(d[:8])
        if head[:2] != b'\xff\xd8' and head != SIGNATURE:
            raise ValueError('file %d is neither a JPEG nor a PNG file (bad signature)' % k)
        kinds.append(head == SIGNATURE)
    png = [k for k, v in enumerate(kinds) if v]
    jpg = [k for k, v in enumerate(kinds) if not v]
    plans = [parse(datas[k]) for k in png]
    if not jpg:
        return run_plans(plans, OUT_NORM if normalize else OUT_RGB, mean, std, device, None).out
    frames = jpegsamp.load_clip([datas[k] for k in jpg], normalize=normalize, mean=mean, std=std, device=device)
    if not png:
        return frames
    h, w = plans[0].size
    if tuple(frames.shape[-2:] if normalize else frames.shape[1:3]) != (h, w):
        raise ValueError('the files of a clip must share one size')
    T = len(datas)
    out = torch.empty((T,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
    run_plans(plans, OUT_NORM if normalize else OUT_RGB, mean, std, frames.device, out[:len(png)])
    out[len(png):] = frames
    order = png + jpg
    if order == list(range(T)):
        return out
    back = np.empty(T, np.int64)
    back[order] = np.arange(T)
    return out[torch.from_numpy(back).to(out.device)]
