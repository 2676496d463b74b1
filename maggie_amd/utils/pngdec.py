"""PNG files decoded on the device (HIP kernels of csrc/pngdec.hip) -- the alpha / mask half of the reference's `T.Load`
(maggie/dataloader/transforms.py:47-50): `Image.open(path).convert("L")` of a `.png`. The loader reads the file's bytes; the pixels never exist
on the host. `geometry.resize_short_pad(jpegdec.decode_clip(...), pngdec.decode_planes(...))` takes file bytes in and returns the item.

  * `parse`          the chunk walk, host only: signature, the CRC of every critical chunk (`zlib.crc32`), IHDR, PLTE, the IDAT payloads
                     concatenated into one zlib stream, and that stream's two header bytes. Raises `Unsupported` (the class of
                     `jpegdec.Unsupported`, a ValueError) for what the device does not decode -- Adam7, 16-bit samples, sides above
                     `mg_pngdec_limits` -- so that a loader's single `except` falls back to PIL, and a plain ValueError for a broken file.
  * `walk`           `parse` under a caller's acceptance rules: what `pngcolor.parse` runs with its own (16-bit samples, Adam7, wider rows).
  * `decode`         one file -> uint8 (h, w) on the device.
  * `decode_planes`  P files of one size (colour type and depth may differ per file) -> (P, h, w) from ONE set of launches.
  * `decode_stats`   the same, returning the inflated bytes, the status words and the counters: for the tests and tools/pngdec_bench.py.

Supported, all non-interlaced: grey and palette at 1, 2, 4 and 8 bits, RGB, RGBA and grey + alpha at 8. Grey samples scale by 255 / 85 / 17 / 1,
palette entries and RGB(A) go through L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, alpha and tRNS do not change `convert("L")`.

Two launches: `mg_pngdec_inflate` runs RFC 1951 with one wave per file and checks the Adler-32 of what it wrote;
`mg_pngdec_unfilter` undoes the scanline filters on a diagonal wavefront and converts to L. Decoding is data-dependent and the host reads the
status words back, so none of this is graph-capturable; ONE read-back per call. A status bit becomes a ValueError (this is stricter than
Pillow, which pads a short stream with zeros). Wrong types raise before any launch. There is no CPU fallback."""
import struct
import zlib

import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import resolve_device
from .jpegdec import Unsupported

THREADS, REC_WORDS, INFO_WORDS, ROUND_TOKENS, FLUSH_BYTES = 64, 72, 8, 64, 4096    # MG_PNGDEC_THREADS / _REC_WORDS / _INFO_WORDS / _ROUND_TOKENS / _FLUSH_BYTES
MAX_SIDE, MAX_ROWBYTES, MAX_BYTES, MAX_RAW = 32767, 16384, 1 << 28, 1 << 30          # MG_PNGDEC_MAX_SIDE / _MAX_ROWBYTES / _MAX_BYTES / _MAX_RAW
STORED_CHUNK = 2048                                          # bytes of a stored block per round (csrc/pngdec.hip)
STATUS = {1: 'a read past the end of the zlib stream', 2: 'more or fewer bytes than height x (1 + rowbytes)',
          4: 'a distance beyond the bytes produced', 8: 'the reserved block type', 16: 'a stored block whose LEN is not ~NLEN',
          32: 'a code set that zlib refuses', 64: 'an unassigned code or a reserved symbol', 128: 'an Adler-32 mismatch',
          256: 'a filter type above 4', 512: 'a palette index past the last PLTE entry', 1024: 'a record outside the buffers'}
SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


class PngPlan:
    """What `parse` found: `width`, `height`, `depth`, `color_type`, `palette` (uint8 (n, 3) or None), `stream` (the zlib stream: the IDAT
    payloads concatenated), `idat_chunks`, `rowbytes`, `raw_size` (height x (1 + rowbytes)), `ltable` (uint8 (256,): the L of each sample value
    or palette index) and `entries` (palette entries; 256 for grey)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def size(self):
        return self.height, self.width


def rowbytes(color_type, depth, w):
    return (w * CHANNELS[color_type] * depth + 7) // 8


def luma(rgb):
    """Pillow's L of RGB (ImagingConvert's L24 >> 16): uint8 (..., 3) -> uint8 (...)."""
    c = np.asarray(rgb).astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def _accepts(w, h, depth, ct, lace):
    """What this module decodes of the legal files: raises `Unsupported` by name, else returns the inflated size."""
    if lace:
        raise Unsupported('Adam7 interlace')
    if depth == 16:
        raise Unsupported('16-bit samples')
    if w > MAX_SIDE or h > MAX_SIDE or rowbytes(ct, depth, w) > MAX_ROWBYTES or h * (1 + rowbytes(ct, depth, w)) > MAX_RAW - 16:
        raise Unsupported('%d x %d at %d bytes a row: sides up to %d and rows up to %d bytes are decoded'
                          % (w, h, rowbytes(ct, depth, w), MAX_SIDE, MAX_ROWBYTES))
    return h * (1 + rowbytes(ct, depth, w))


def parse(data):
    """The chunk walk of one file's bytes -> PngPlan. Host only. `Unsupported` for Adam7, 16-bit samples and sides above the limits;
    ValueError for a bad signature, a bad CRC of a critical chunk, a truncated file, a missing IHDR, IDAT or PLTE, a bad zlib header."""
    return walk(data, _accepts)


def walk(data, accepts):
    """`parse` under a module's own rules (this one's and `pngcolor`'s): `accepts(w, h, depth, ct, interlace)` raises `Unsupported` for a legal
    file the module does not decode and returns the inflated size. The plan carries `interlace` too."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a PNG file (got %s)' % type(data).__name__)
    d = bytes(data)
    n = len(d)
    if d[:8] != SIGNATURE:
        raise ValueError('not a PNG file (bad signature)')
    p = 8
    ihdr = palette = None
    idat = []
    ended = False
    while p < n:
        if p + 12 > n:
            raise ValueError('the file ends inside a chunk header')
        size, kind = struct.unpack('>I4s', d[p:p + 8])
        if p + 12 + size > n:
            raise ValueError('the file ends inside its %s chunk' % kind.decode('latin-1'))
        body = d[p + 8:p + 8 + size]
        if not kind[0] & 0x20:                                 # a critical chunk
            if zlib.crc32(d[p + 4:p + 8 + size]) != struct.unpack('>I', d[p + 8 + size:p + 12 + size])[0]:
                raise ValueError('a bad CRC in the %s chunk' % kind.decode('latin-1'))
            if ihdr is None and kind != b'IHDR':
                raise ValueError('the first chunk is not IHDR')
            if kind == b'IHDR':
                if ihdr is not None or size != 13:
                    raise ValueError('a malformed IHDR chunk')
                ihdr = struct.unpack('>IIBBBBB', body)
            elif kind == b'PLTE':
                if size % 3 or not 3 <= size <= 768 or idat:
                    raise ValueError('a malformed PLTE chunk')
                palette = np.frombuffer(body, np.uint8).reshape(-1, 3).copy()
            elif kind == b'IDAT':
                idat.append(body)
            elif kind == b'IEND':
                ended = True
                break
            else:
                raise Unsupported('a critical chunk this decoder does not know (%s)' % kind.decode('latin-1'))
        p += 12 + size
    if ihdr is None:
        raise ValueError('no IHDR chunk')
    w, h, depth, ct, comp, filt, lace = ihdr
    if ct not in DEPTHS or depth not in DEPTHS[ct] or comp != 0 or filt != 0 or lace > 1 or w < 1 or h < 1:
        raise ValueError('a malformed IHDR chunk (%d x %d, colour type %d, depth %d, methods %d %d %d)' % (w, h, ct, depth, comp, filt, lace))
    raw_size = accepts(w, h, depth, ct, lace)
    if not idat:
        raise ValueError('no IDAT chunk')
    if not ended:
        raise ValueError('the file ends without IEND')
    if ct == 3 and palette is None:
        raise ValueError('a palette file without PLTE')
    stream = b''.join(idat)
    if len(stream) < 6:
        raise ValueError('a zlib stream of %d bytes' % len(stream))
    if len(stream) > MAX_BYTES:
        raise Unsupported('a zlib stream of %d bytes' % len(stream))
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf * 256 + flg) % 31:
        raise ValueError('a bad zlib header (CMF 0x%02x, FLG 0x%02x)' % (cmf, flg))
    ltable = np.zeros(256, np.uint8)
    if ct == 3:
        entries = len(palette)
        ltable[:entries] = luma(palette)
    else:
        entries = 256
        if ct == 0 and depth <= 8:
            ltable[:1 << depth] = np.arange(1 << depth) * (255 // ((1 << depth) - 1))
        else:
            ltable[:] = np.arange(256)
    rb = rowbytes(ct, depth, w)
    return PngPlan(width=w, height=h, depth=depth, color_type=ct, palette=palette if ct == 3 else None, stream=stream, idat_chunks=len(idat),
                   rowbytes=rb, raw_size=raw_size, ltable=ltable, entries=entries, interlace=lace)


def record(plan, offset):
    """A file's int32 record (MG_PNGDEC_REC_WORDS words, include/maggie_hip.h) with its zlib stream at `offset` of the buffer."""
    rec = np.zeros(REC_WORDS, np.int32)
    rec[0], rec[1], rec[2], rec[3], rec[4] = offset, len(plan.stream), plan.color_type, plan.depth, plan.entries
    rec[8:72] = plan.ltable.view(np.int32)
    return rec


class Decoded:
    """What `run` leaves: on the device `out` uint8 (P, h, w) and `raw` uint8 (P, raw_stride), the inflated bytes of file p in
    raw[p, :raw_sizes[p]]; on the host `info` int32 (P, INFO_WORDS), `status`, `rounds`, `blocks`, `tokens` (arrays over the files) and
    `readbacks`."""


def run(blob, recs, h, w, *, out=None, guard=0):
    """The launches themselves: `blob` uint8 device tensor holding the P zlib streams, `recs` int32 (P, REC_WORDS) host records whose offsets
    point into it. `out`: a preallocated contiguous uint8 destination of P x h x w elements (else allocated). `guard`: bytes of 0xA5 kept on
    both sides of `raw` and of an allocated `out` (for the tests: `Decoded.guards` holds the four slices). Returns a `Decoded`."""
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, REC_WORDS)
    P = recs.shape[0]
    dev = blob.device
    hip.need_cuda(blob)
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError('blob must be a contiguous 1-D uint8 tensor')
    if P < 1 or (recs[:, 0] < 0).any() or (recs[:, 1] < 0).any() or int((recs[:, 0].astype(np.int64) + recs[:, 1]).max()) > blob.numel():
        raise ValueError('a zlib stream lies outside the buffer')
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_SIDE:
        raise ValueError('sides of 1..%d are decoded (got %d x %d)' % (MAX_SIDE, h, w))
    if any(int(c) not in CHANNELS or int(b) not in (1, 2, 4, 8) for c, b in recs[:, 2:4]):
        raise ValueError('a record with an unknown colour type or depth')
    sizes = [h * (1 + rowbytes(int(c), int(b), w)) for c, b in recs[:, 2:4]]
    stride = -(-max(sizes) // 16) * 16
    guard = -(-guard // 16) * 16
    tabs = torch.from_numpy(recs).to(dev, non_blocking=True)
    rawbuf = torch.full((2 * guard + P * stride,), 0xA5, dtype=torch.uint8, device=dev) if guard else \
        torch.empty((P * stride,), dtype=torch.uint8, device=dev)
    raw = rawbuf[guard:guard + P * stride]
    info = torch.zeros((P, INFO_WORDS), dtype=torch.int32, device=dev)
    outbuf = None
    if out is None:
        outbuf = torch.full((2 * guard + P * h * w,), 0xA5, dtype=torch.uint8, device=dev) if guard else \
            torch.empty((P * h * w,), dtype=torch.uint8, device=dev)
        out = outbuf[guard:guard + P * h * w]
    elif not torch.is_tensor(out) or out.numel() != P * h * w or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous uint8 tensor of %d elements on %s' % (P * h * w, dev))
    st = hip.stream
    hip.call('mg_pngdec_inflate', hip.ptr(blob), c_long(blob.numel()), hip.ptr(tabs), hip.ptr(raw), c_long(stride), hip.ptr(info), c_long(P),
             c_int(h), c_int(w), st())
    hip.call('mg_pngdec_unfilter', hip.ptr(raw), c_long(stride), hip.ptr(tabs), hip.ptr(out), hip.ptr(info), c_long(P), c_int(h), c_int(w), st())
    host = info.cpu().numpy()
    r = Decoded()
    r.out, r.raw, r.raw_sizes, r.raw_stride, r.info = out.reshape(P, h, w), raw.reshape(P, stride), sizes, stride, host
    r.status, r.rounds, r.blocks, r.tokens, r.readbacks = host[:, 0].copy(), host[:, 1].copy(), host[:, 2].copy(), host[:, 3].copy(), 1
    r.guards = [] if not guard else [rawbuf[:guard], rawbuf[guard + P * stride:]] + \
        ([] if outbuf is None else [outbuf[:guard], outbuf[guard + P * h * w:]])
    for k in range(P):
        if host[k, 0]:
            raise ValueError('file %d: a corrupt PNG data stream: %s' % (k, '; '.join(v for b, v in STATUS.items() if host[k, 0] & b)))
    return r


def _planes(datas, device, out):
    if isinstance(datas, (bytes, bytearray, memoryview)) or not hasattr(datas, '__len__'):
        raise TypeError('datas must be a sequence of the bytes of PNG files (got %s)' % type(datas).__name__)
    if len(datas) < 1:
        raise ValueError('datas must hold at least one file')
    plans = [parse(d) for d in datas]
    if any(p.size != plans[0].size for p in plans):
        raise ValueError('the files of one call must share one size (got %s)' % sorted({p.size for p in plans}))
    offsets = np.concatenate([[0], np.cumsum([len(p.stream) for p in plans])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of zlib streams in one call' % offsets[-1])
    recs = np.stack([record(p, int(o)) for p, o in zip(plans, offsets[:-1])])
    device = resolve_device(device, out if torch.is_tensor(out) else None)
    blob = torch.frombuffer(bytearray(b''.join(p.stream for p in plans)), dtype=torch.uint8).to(device, non_blocking=True)
    h, w = plans[0].size
    return run(blob, recs, h, w, out=out)


def decode_planes(datas, *, device=None, out=None):
    """P PNG files (a sequence of bytes objects) of one size -> uint8 (P, h, w) on the device, each plane `convert("L")` of its file, from one
    set of launches with one read-back; colour type and depth may differ per file. A caller reshapes to (T, n_i, h, w) for
    `DevicePreprocessor`. Files of differing size raise ValueError, unsupported ones `Unsupported`, a corrupt stream ValueError. `out`: a
    contiguous uint8 device tensor of P x h x w elements to write into. Not graph-capturable (the module docstring says why)."""
    return _planes(datas, device, out).out


def decode(data, *, device=None):
    """The bytes of one PNG file -> uint8 (h, w) on the device: `np.asarray(Image.open(BytesIO(data)).convert("L"))`. Not graph-capturable:
    decoding is data-dependent and the host reads the status words back, once."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a PNG file (got %s)' % type(data).__name__)
    return _planes([data], device, None).out[0]


def decode_stats(datas, *, device=None, out=None):
    """`decode_planes` returning the whole `Decoded` record (inflated bytes, status words, rounds, blocks, tokens): for the tests and
    tools/pngdec_bench.py. Not graph-capturable."""
    return _planes(datas, device, out)
