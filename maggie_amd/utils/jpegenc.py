"""Baseline JPEG files written from device frames (HIP kernels of csrc/jpegenc.hip) -- the last step of the reference's synthesis tools,
`PIL.Image.save('....jpg')` (tools/synthesize_image_him.py:93-94,109: the composite, the background and one foreground canvas per instance;
tools/synthesize_video_him.py:189: every composited frame). The frames stay on the device; what comes back to the host is the entropy-coded
segment, a tenth of the pixels or less.

  * `header`        the 623 bytes in front of the scan (SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS): host only.
  * `encode`        one frame (h, w, 3) uint8 -> the bytes of its file.
  * `encode_clip`   T frames of one size (T, h, w, 3) -> T files from ONE set of launches; every frame has its own stream.
  * `encode_stats`  the same, returning coefficients, per-block bits, bit offsets, the unstuffed streams, sizes and guard slices: for the tests
                    and tools/jpegenc_bench.py.
  * `save_sample`   the file tree of synthesize_image_him.py:93-109 from the dict `compose.synthesize_image` returns.
  * `save_frame`    one frame to one path: synthesize_video_him.py:189.

The contract: `encode(x, q)` is `buf = io.BytesIO(); PIL.Image.fromarray(x).save(buf, 'JPEG', quality=q); buf.getvalue()` byte for byte, the whole
file, for every (h, w, 3) uint8 frame with sides of 1..32767 and every quality 1..100 (Pillow 12.2.0 on libjpeg-turbo 3.1.4.1; DESIGN.md section
28; tests/jpegenc_restatement.py is the sequential statement, held against Pillow by tests/test_jpegenc_cpu.py). That is Pillow's `.save(path)`:
quality 75 by default, 4:2:0, the Annex K tables, `optimize=False`, no restart markers -- the only mode the reference uses and the only one
built. NOT built: greyscale, 4:4:4, optimised tables, progressive files, `dpi=` / `exif=` / `icc_profile=`. `quality` may also be a (2, 64) int32
quantisation table in natural order, as `photometric.jpeg_roundtrip` takes; `lut` and `noise` are its operands too, so that the tone curve, the
noise and the file are one chain: `jpegdec.decode(encode(x, q, lut=l, noise=n))` has the bits of `photometric.jpeg_roundtrip(x, q, lut=l, noise=n)`.

Four entry points (`mg_jpegenc_coef`, `_bits`, `_pack`, `_stuff`; nine kernels) and TWO read-backs per call: the sizes (16 bytes a frame), then
exactly the bytes of the scans. The sizes decide an allocation, so none of this is graph-capturable. Wrong dtype, rank, size, quality or table
raise before any launch. There is no CPU fallback."""
import os

import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import lut_table, to_device
from .photometric import MAX_SIDE, _check_quality, _frames, _noise, _qtable, quant_tables

THREADS, PACK_BLOCKS, CHUNK_BYTES, MAX_BLOCK_BITS, MAX_FRAMES = 256, 64, 4096, 1658, 4096        # MG_JPEGENC_* (include/maggie_hip.h)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
EOI = b'\xff\xd9'

# ISO/IEC 10918-1 Annex K.3 - K.6 as the DHT segments hold them: the number of codes of each length 1..16, then the symbols in code order
_AC_TAIL = [r << 4 | n for r in range(16) for n in range(1, 11)]
DHT_DC_LUMA = bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12))
DHT_DC_CHROMA = bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12))
DHT_AC_LUMA = bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]) + bytes([
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
DHT_AC_CHROMA = bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]) + bytes([
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
assert len(DHT_AC_LUMA) == len(DHT_AC_CHROMA) == 16 + 162 and sorted(DHT_AC_LUMA[16:]) == sorted(DHT_AC_CHROMA[16:]) == sorted(_AC_TAIL + [0, 0xF0])


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)


def header(h, w, qtable):
    """The bytes in front of the scan of an h x w RGB file with the (2, 64) quantisation table `qtable` (natural order, entries 1..255): SOI,
    APP0 `JFIF\\0` 1.01 with no units and 1 : 1, DQT 0, DQT 1 (8-bit entries in zig-zag order), SOF0 (1:0x22:0, 2:0x11:1, 3:0x11:1), DHT DC0,
    AC0, DC1, AC1, SOS. 623 bytes. Host only."""
    t = np.asarray(qtable).reshape(2, 64)
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_SIDE or t.min() < 1 or t.max() > 255:
        raise ValueError('sides of 1..%d and table entries of 1..255 are written' % MAX_SIDE)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    out += [_segment(0xDB, bytes([k]) + bytes(int(v) for v in t[k][ZIGZAG])) for k in range(2)]
    out.append(_segment(0xC0, bytes([8]) + int(h).to_bytes(2, 'big') + int(w).to_bytes(2, 'big') + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    out += [_segment(0xC4, bytes([ident]) + tab) for ident, tab in ((0x00, DHT_DC_LUMA), (0x10, DHT_AC_LUMA), (0x01, DHT_DC_CHROMA), (0x11, DHT_AC_CHROMA))]
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])))
    return b''.join(out)


def blocks_of(h, w):
    """Coefficient blocks of one frame: six per 16 x 16 MCU."""
    return ((h + 15) // 16) * ((w + 15) // 16) * 6


def raw_stride(h, w):
    """The bytes of a frame's slice of the unstuffed buffer: every block at its worst case of MAX_BLOCK_BITS bits, rounded up to 16."""
    return -(-((blocks_of(h, w) * MAX_BLOCK_BITS + 7) // 8 + 4) // 16) * 16


def _table_host(quality):
    """The (2, 64) table the header states: a quality's, or the table itself (read back when it lives on the device), clamped as the kernel does."""
    if _check_quality(quality):
        t = quality.cpu().numpy() if torch.is_tensor(quality) else np.asarray(quality)
        return np.clip(t, 1, 255).astype(np.int32)
    return quant_tables(quality)


class Encoded:
    """What `run` leaves: `files` (T bytes objects), on the host `sizes` int64 (4, T) (the scan's bytes in the file, its unstuffed bytes, its
    bits, its offset), `readbacks`; with stats=True also the device tensors `coef` int16 (T, blocks, 64), `bits` int32 (T, blocks), `offs` int64
    (T, blocks), `raw` uint8 (T, raw_stride) and the list `unstuffed` (T bytes objects); with a guard `guards`, slices of 0xA5 on both sides of
    every device buffer, and `slack`, the zeroed bytes behind the last stream."""


def _guarded(nbytes, guard, dev, zero=False):
    """`nbytes` of device memory (16-byte aligned) between two guards of 0xA5 -> (the slice, [front guard, back guard])."""
    nbytes = -(-nbytes // 16) * 16
    if not guard:
        return (torch.zeros if zero else torch.empty)((nbytes,), dtype=torch.uint8, device=dev), []
    buf = torch.full((2 * guard + nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    mid = buf[guard:guard + nbytes]
    if zero:
        mid.zero_()
    return mid, [buf[:guard], buf[guard + nbytes:]]


def run(x, qtable, table_host, lut=None, noise=None, nc=1, *, guard=0, stats=False):
    """The launches themselves: `x` a contiguous device tensor (T, h, w, 3) uint8, `qtable` the device (2, 64) int32 table and `table_host` the
    same on the host, `lut` / `noise` device operands or None. `guard`: bytes of 0xA5 kept on both sides of every buffer. Returns an `Encoded`."""
    hip.need_cuda(x)
    T, h, w, _ = x.shape
    nb, stride = blocks_of(h, w), raw_stride(h, w)
    chunks = -(-stride // CHUNK_BYTES)
    dev = x.device
    guard = -(-guard // 16) * 16
    with torch.cuda.device(dev):
        coef_b, g1 = _guarded(T * nb * 128, guard, dev)
        bits_b, g2 = _guarded(T * nb * 4, guard, dev)
        offs_b, g3 = _guarded(T * nb * 8, guard, dev)
        size_b, g4 = _guarded(4 * T * 8, guard, dev)
        raw, g5 = _guarded(T * stride, guard, dev, zero=True)
        ff_b, g6 = _guarded(T * chunks * 4, guard, dev)
        ch_b, g7 = _guarded(T * chunks * 8, guard, dev)
        coef, bits = coef_b.view(torch.int16)[:T * nb * 64], bits_b.view(torch.int32)[:T * nb]
        offs, sizes = offs_b.view(torch.int64)[:T * nb], size_b.view(torch.int64)[:4 * T]
        st = hip.stream
        geo = (c_long(T), c_int(h), c_int(w))
        hip.call('mg_jpegenc_coef', hip.ptr(x), hip.ptr(lut), hip.ptr(noise), c_int(nc), hip.ptr(qtable), hip.ptr(coef), c_long(coef.numel()),
                 *geo, st())
        hip.call('mg_jpegenc_bits', hip.ptr(coef), c_long(coef.numel()), hip.ptr(bits), hip.ptr(offs), hip.ptr(sizes), *geo, st())
        hip.call('mg_jpegenc_pack', hip.ptr(coef), c_long(coef.numel()), hip.ptr(bits), hip.ptr(offs), hip.ptr(sizes), hip.ptr(raw),
                 c_long(stride), hip.ptr(ff_b), hip.ptr(ch_b), *geo, st())
        host = sizes.cpu().numpy().reshape(4, T)                                # read-back 1: the sizes
        total = int(host[0].sum())
        if int(host[1].max()) + 4 > stride or int(host[1].min()) < 1:
            raise hip.MaggieHipError('mg_jpegenc_pack left a stream of %d bytes in a slice of %d' % (int(host[1].max()), stride))
        out, g8 = _guarded(total, guard, dev, zero=True)
        grid_chunks = min(chunks, -(-int(host[1].max()) // CHUNK_BYTES))
        hip.call('mg_jpegenc_stuff', hip.ptr(raw), c_long(stride), hip.ptr(ch_b), hip.ptr(sizes), hip.ptr(out), c_long(total), *geo,
                 c_long(grid_chunks), st())
        data = out[:total].cpu().numpy().tobytes()                             # read-back 2: exactly the bytes
    r = Encoded()
    head = header(h, w, table_host)
    r.sizes, r.readbacks = host, 2
    r.files = [head + data[int(o):int(o + s)] for o, s in zip(host[3], host[0])]
    if stats:
        r.coef, r.bits, r.offs = coef.view(T, nb, 64), bits.view(T, nb), offs.view(T, nb)
        r.raw = raw[:T * stride].view(T, stride)
        r.unstuffed = [r.raw[t, :int(host[1][t])].cpu().numpy().tobytes() for t in range(T)]
        r.slack, r.guards = out[total:], g1 + g2 + g3 + g4 + g5 + g6 + g7 + g8
    return r


def _encode(frames_u8, quality, lut, noise, device, guard=0, stats=False):
    _check_quality(quality)
    lut_table(lut)
    f, lead, n, h, w = _frames(frames_u8, noise)
    if len(lead) != 1:
        raise ValueError('frames must be (T, h, w, 3) (got %s)' % (tuple(f.shape),))
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError('1..%d frames a call (got %d)' % (MAX_FRAMES, n))
    f = to_device(f, device)
    nz, nc = _noise(noise, f.device)
    table = _table_host(quality)
    return run(f, _qtable(quality, f.device), table, lut_table(lut, f.device), nz, nc, guard=guard, stats=stats)


def encode_clip(frames_u8, quality=75, *, lut=None, noise=None, device=None):
    """T frames of one size, (T, h, w, 3) uint8 (a device tensor; an array or a host tensor is uploaded) -> a list of T bytes objects, each the
    complete file `PIL.Image.fromarray(frame).save(buf, 'JPEG', quality=quality)` writes, from one set of launches and two read-backs. `quality`
    is 1..100 for the whole clip, or a (2, 64) int32 table (natural order); `lut` (3, 256) uint8 and `noise` int16 (h, w, 1 or 3) are applied
    to the pixels first, as in `photometric.jpeg_roundtrip`. TypeError / ValueError for a wrong dtype, rank, size, quality or table, before any
    launch. Not graph-capturable."""
    return _encode(frames_u8, quality, lut, noise, device).files


def _one(frame_u8):
    if not (torch.is_tensor(frame_u8) or isinstance(frame_u8, np.ndarray)) or frame_u8.ndim != 3:
        raise ValueError('frame must be a tensor or an array of shape (h, w, 3)')
    return frame_u8[None]


def encode(frame_u8, quality=75, *, lut=None, noise=None, device=None):
    """One frame (h, w, 3) uint8 -> the bytes of its JPEG file (see `encode_clip`)."""
    return _encode(_one(frame_u8), quality, lut, noise, device).files[0]


def encode_stats(frames_u8, quality=75, *, lut=None, noise=None, device=None, guard=0):
    """`encode_clip` returning the whole `Encoded` record: for the tests and tools/jpegenc_bench.py. Reading its device fields costs further
    read-backs; `readbacks` counts those of the encoding itself."""
    return _encode(frames_u8, quality, lut, noise, device, guard=guard, stats=True)


def _write(path, data):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)


def save_frame(frame_u8, path):
    """`Image.fromarray(frame).save(path)` for a `.jpg` path (synthesize_video_him.py:189): one frame (h, w, 3) uint8 on the device, at Pillow's
    default quality 75."""
    _write(path, encode(frame_u8, 75))


def save_sample(sample, sample_id, image_dir, bg_dir, alpha_dir, fg_dir):
    """The files of synthesize_image_him.py:93-109 from the dict `compose.synthesize_image(..., jpeg=False)` returns: {image_dir}/{id}.jpg,
    {bg_dir}/{id}.jpg, {alpha_dir}/{id}/{k}.png and {fg_dir}/{id}/{k}.jpg for the kept instances k = 0, 1, ... The .jpg files are Pillow's bytes
    at its default quality 75; the .png files come from `pngenc` and are reader-equal. `image`, `bg` and all `fgs` go
    through ONE `encode_clip`, since they share the background's size; the alphas through one `pngenc.encode_planes`. Returns the paths written."""
    from . import pngenc
    if sample is None:
        return []
    image, bg, fgs, alphas = sample['image'], sample['bg'], sample['fgs'], sample['alphas']
    n = int(fgs.shape[0])
    if tuple(image.shape) != tuple(bg.shape) or tuple(fgs.shape[1:]) != tuple(image.shape) or int(alphas.shape[0]) != n:
        raise ValueError('image, bg and fgs must share one size, with one alpha per foreground (got %s, %s, %s, %s)' %
                         (tuple(image.shape), tuple(bg.shape), tuple(fgs.shape), tuple(alphas.shape)))
    jpgs = encode_clip(torch.cat([image[None], bg[None], fgs]), 75)
    pngs = pngenc.encode_planes(alphas)
    sid = str(sample_id)
    paths = [os.path.join(image_dir, sid + '.jpg'), os.path.join(bg_dir, sid + '.jpg')]
    _write(paths[0], jpgs[0])
    _write(paths[1], jpgs[1])
    for k in range(n):
        pa, pf = os.path.join(alpha_dir, sid, '%d.png' % k), os.path.join(fg_dir, sid, '%d.jpg' % k)
        _write(pa, pngs[k])
        _write(pf, jpgs[2 + k])
        paths += [pa, pf]
    return paths
