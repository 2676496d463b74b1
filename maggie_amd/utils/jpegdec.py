"""Baseline JPEG files decoded on the device (HIP kernels of csrc/jpegdec.hip) -- the step in front of every input stage, the reference's
`T.Load` (maggie/dataloader/transforms.py:38-66): `Image.open(path).convert("RGB")` of a `.jpg`. The loader reads the file's bytes; the
pixels never exist on the host.

  * `parse`        the marker walk, host only: size, sampling layout, quantisation and Huffman tables, restart interval, where the
                   entropy-coded segment lies. Raises `Unsupported` (a ValueError) for everything outside the supported set, before any launch,
                   so that a loader can fall back to PIL: `SOF0`, 8 bits, one interleaved scan, YCbCr 4:2:0 or 4:4:4 or one greyscale component.
  * `decode`       one file -> uint8 (h, w, 3) on the device, or with `normalize` fp32 (3, h, w) with the bits of `normalize_frames`.
  * `decode_clip`  T files of one geometry and layout (a video clip) -> (T, h, w, 3) or (T, 3, h, w) from ONE set of launches; tables and
                   stream offsets are per frame.

The Huffman decoding is the self-synchronising parallel form of Weissenberger and Schmidt: the segment is
cut into subsequences of `sub_bytes` raw bytes, one lane each; launch 0 decodes every subsequence from its own first bit and settles each
workgroup, every further launch carries exit states across workgroups, until a launch moves none. The number of rounds is at most the number
of subsequences, and the launches at most the workgroups plus one; both bounds are computed here and a stream that exceeds them raises.
Everything behind the coefficients is section 19's arithmetic (4:2:0 finishes through the existing `mg_jpeg_rgb`): equal to Pillow byte for byte.

Decoding is data-dependent, so it is NOT graph-capturable: the host has to see whether the synchronisation settled. Read-backs per call:
ONE in the usual case -- the output pass is launched behind the second synchronisation launch without waiting, and the `info` words (status,
per-launch "moved" flags, rounds) come back once at the end. Only when that second launch still moved a workgroup's exit state (a stream
that does not self-synchronise within a workgroup, such as a periodic one) is there one more read-back per further launch, and the output
pass runs again. A status bit becomes a ValueError; libjpeg's warn-and-continue on corrupt files is not reproduced. Wrong types raise before
any launch. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, integer, resolve_device
from ._jpegfile import Unsupported, ZIGZAG, walk                  # noqa: F401  (ZIGZAG: for the callers of this module)
from .photometric import MAX_SIDE, NORM, RAW

L420, L444, GREY, L422, L440, L411 = 0, 1, 2, 3, 4, 5          # MG_JPEGDEC_420 / _444 / _GREY / _422 / _440 / _411 (include/maggie_hip.h)
LUMA = {L422: (2, 1), L440: (1, 2), L411: (4, 1)}           # the luma sampling (hs, vs) of the layouts whose planes are pitched
_HV = {L420: (2, 2), L444: (1, 1), GREY: (1, 1), **LUMA}
THREADS, TAB_WORDS, MIN_SUB, MAX_SUB, DEFAULT_SUB = 128, 1120, 8, 4096, 8        # MG_JPEGDEC_THREADS / _TAB_WORDS / _MIN_SUB / _MAX_SUB / _DEFAULT_SUB
MAX_BYTES = 1 << 28                                         # MG_JPEGDEC_MAX_BYTES
STATUS = {1: 'a zig-zag index past 63', 2: 'an unassigned Huffman code', 4: 'the entropy-coded segment ends before the last block',
          8: 'the number of blocks is not MCUs x blocks per MCU', 16: 'a restart marker out of place'}


def geometry(h, w, layout):
    """The geometry of a frame in any of the six layouts, csrc/jpeg_common.h's: (blocks of a frame, plane bytes of a frame, luma rows, luma
    pitch, chroma rows, chroma pitch). An MCU is 8 hs x 8 vs pixels: hs * vs luma blocks, then Cb, then Cr. The planes of 4:2:0, 4:4:4 and
    grey are as wide as their blocks; those of the `LUMA` layouts are pitched to the widest load of a lane of mg_jpeg_rgb_hv: the luma pitch
    is a multiple of 16 bytes and the 4:4:0 chroma pitch too."""
    hs, vs = _HV[layout]
    mx, my, chroma = -(-w // (8 * hs)), -(-h // (8 * vs)), 0 if layout == GREY else 2
    yp, cp = mx * 8 * hs, mx * 8
    if layout in LUMA:
        yp, cp = -(-yp // 16) * 16, -(-cp // 16) * 16 if vs == 2 else cp
    return mx * my * (hs * vs + chroma), my * 8 * (vs * yp + chroma * cp), my * 8 * vs, yp, my * 8, cp


class JpegPlan:
    """What `parse` found: `width`, `height`, `layout` (one of the six), `sampling` ((h, v) per component), `quantization` ({id: int32 (64,)
    natural order}), `qtables` (int32 (3, 64): the table of each output component), `dc` / `ac` ({id: (counts uint8 (16,), values uint8 (n,))}),
    `selectors` ((dc id, ac id) per component), `restart_interval` (MCUs, 0 = none), `offset` / `length` of the entropy-coded segment."""
    kind = 'baseline'

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def geometry(self):
        return self.height, self.width, self.layout

    @property
    def mcus(self):
        hs, vs = _HV[self.layout]
        return -(-self.width // (8 * hs)) * -(-self.height // (8 * vs))


def _layout(sampling):
    """The layout of a frame's ((h, v) per component), or `Unsupported`: what this module and `jpegprog` decode."""
    if len(sampling) == 1:
        return GREY
    if sampling == ((2, 2), (1, 1), (1, 1)):
        return L420
    if sampling == ((1, 1), (1, 1), (1, 1)):
        return L444
    raise Unsupported('sampling %s (only 4:2:0 and 4:4:4 are decoded)' % (sampling,))


def parse(data):
    """The marker walk of one file's bytes -> JpegPlan. Host only; raises `Unsupported` by name for what the device does not decode."""
    return _parse(data, _layout)


def check_frame(frame):
    """The frame headers both decoders take; `frame` gains `sampling`."""
    comps, w, h = frame['comps'], frame['width'], frame['height']
    if len(comps) not in (1, 3):
        raise Unsupported('%d components (only YCbCr and greyscale are decoded)' % len(comps))
    if h == 0:
        raise Unsupported('DNL (the height is defined after the scan)')
    if w < 1 or w > MAX_SIDE or h > MAX_SIDE:
        raise Unsupported('%d x %d: sides of 1..%d are decoded' % (w, h, MAX_SIDE))
    if frame['sof'] == 0xC2 and len({c[0] for c in comps}) != len(comps):
        raise Unsupported('two components with one identifier')
    frame['sampling'] = tuple((c[1], c[2]) for c in comps)


def output_tables(f):
    """int32 (3, 64): the quantisation table of each output component, or `Unsupported` where a component names one the file did not define."""
    comps = f.frame['comps']
    for c in comps:
        if c[3] not in f.quant:
            raise Unsupported('quantisation table %d is not defined' % c[3])
    return np.stack([f.quant[comps[min(k, len(comps) - 1)][3]] for k in range(3)]).astype(np.int32)


def rules(layout_of):
    """(on_frame, on_scan, plan): the acceptance rules of a baseline file for `walk`, and the JpegPlan of what `walk` returns. `layout_of(sampling)`
    returns the layout or raises `Unsupported` (`jpegsamp.parse` walks the same markers for its three samplings)."""
    def on_frame(f):
        pass

    def on_scan(f, scan):                                      # the frame is judged here, where the single scan is known
        check_frame(f.frame)
        if [c[0] for c in f.frame['comps']] != [s[0] for s in scan.selectors]:
            raise Unsupported('several scans, or a scan that does not hold every component in frame order')
        f.frame['layout'] = layout_of(f.frame['sampling'])
        f.qtables = output_tables(f)
        for _, td, ta in scan.selectors:
            if td > 1 or ta > 1 or td not in f.dc or ta not in f.ac:
                raise Unsupported('a scan that selects a Huffman table that is not defined (DC %d, AC %d)' % (td, ta))

    def plan(f):
        scan = f.scans[0]
        if f.next == 0xDC:
            raise Unsupported('DNL (the height is defined after the scan)')
        if f.next != 0xD9:
            raise Unsupported('several scans (marker 0xFF%02X behind the first)' % f.next)
        if scan.length > MAX_BYTES - MAX_SUB:
            raise Unsupported('an entropy-coded segment of %d bytes' % scan.length)
        return JpegPlan(width=f.frame['width'], height=f.frame['height'], layout=f.frame['layout'], sampling=f.frame['sampling'], quantization=f.quant,
                        qtables=f.qtables, dc=f.dc, ac=f.ac, selectors=tuple((s[1], s[2]) for s in scan.selectors),
                        restart_interval=f.restart_interval, offset=scan.offset, length=scan.length)
    return on_frame, on_scan, plan


def _parse(data, layout_of):
    on_frame, on_scan, plan = rules(layout_of)
    return plan(walk(data, False, on_frame, on_scan))


_WORDS = {}                                                 # huffman_words by table: a loader's files share a handful of tables


def huffman_words(counts, values):
    """`_huffman_words`, remembered per table (the Annex K tables recur in every file an encoder writes without optimising)."""
    key = (bytes(counts), bytes(values))
    if key not in _WORDS:
        if len(_WORDS) >= 256:
            _WORDS.clear()
        _WORDS[key] = _huffman_words(counts, values)
    return _WORDS[key]


def _huffman_words(counts, values):
    """One table as the 228 int32 words the kernels read: look uint16[256] (len << 8 | symbol for codes of at most 8 bits), maxcode[18]
    (-1 = no code of that length), valoff[18] (index of the length's first value minus its first code), vals uint8[256]."""
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    vals = np.zeros(256, np.uint8)
    vals[:len(values)] = values
    code = k = 0
    for l in range(1, 17):
        c = int(counts[l - 1])
        if c:
            valoff[l] = k - code
            if l <= 8:
                for i in range(c):
                    look[(code + i) << (8 - l):(code + i + 1) << (8 - l)] = (l << 8) | int(values[k + i])
            code += c
            k += c
            maxcode[l] = code - 1
        code <<= 1
    return np.concatenate([look.view(np.int32), maxcode, valoff, vals.view(np.int32)])


def record(plan, offset):
    """A frame's int32 record (MG_JPEGDEC_TAB_WORDS words, include/maggie_hip.h) with its segment at `offset + plan.offset` of the buffer."""
    rec = np.zeros(TAB_WORDS, np.int32)
    empty = (np.zeros(16, np.uint8), np.zeros(0, np.uint8))
    for k, t in enumerate((plan.dc.get(0, empty), plan.dc.get(1, empty), plan.ac.get(0, empty), plan.ac.get(1, empty))):
        rec[228 * k:228 * (k + 1)] = huffman_words(*t)
    sel = plan.selectors
    hs, vs = plan.sampling[0]                                  # an MCU: the hs * vs luma blocks, then Cb, then Cr
    slots = [sel[0]] * (hs * vs) + [sel[1], sel[2]] if len(sel) == 3 else list(sel)
    for s, (td, ta) in enumerate(slots):
        rec[912 + s] = td | (ta << 4)
    rec[918], rec[919], rec[920] = offset + plan.offset, plan.length, plan.restart_interval
    rec[928:1120] = plan.qtables.reshape(-1)
    return rec


def _sub_bytes(sub_bytes):
    s = DEFAULT_SUB if sub_bytes is None else integer(sub_bytes, 'sub_bytes')
    if not MIN_SUB <= s <= MAX_SUB:
        raise ValueError('sub_bytes must be in %d..%d (got %d)' % (MIN_SUB, MAX_SUB, s))
    return s


class Decoded:
    """What `run` leaves on the device: `out`, the coefficient blocks `coef` (T, blocks, 64) int16 in scan order, the component `planes`, and
    on the host `rounds` (rounds inside workgroups, summed over the launches), `launches`, `subsequences` (the bound of the rounds) and
    `readbacks`."""


def finishing(r, tabs, T, h, w, layout, normalize, mean, std, out):
    """What `run` here and `jpegprog.run` share behind the coefficients. Before any launch: `out` allocated or validated, `r.coef` (zeroed)
    and `r.planes` allocated by `geometry`, `r.out` shaped. Returns the function that launches mg_jpegdec_idct and the colour entry of the layout."""
    dev = tabs.device
    nblocks, per_frame = geometry(h, w, layout)[:2]
    coef = torch.zeros((T, nblocks, 64), dtype=torch.int16, device=dev)
    planes = torch.empty((T * per_frame,), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((T, 3, h, w) if normalize else (T, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=dev)
    elif out.numel() != T * h * w * 3 or out.dtype != (torch.float32 if normalize else torch.uint8) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous %s tensor of %d elements on %s' % ('float32' if normalize else 'uint8', T * h * w * 3, dev))
    r.out, r.coef, r.planes = out.reshape((T, 3, h, w) if normalize else (T, h, w, 3)), coef, planes
    size, epilogue = (c_long(T), c_int(h), c_int(w)), (c_int(NORM if normalize else RAW), float3(mean), float3(std))

    def finish():
        st = hip.stream()
        hip.call('mg_jpegdec_idct', hip.ptr(coef), c_long(coef.numel()), hip.ptr(tabs), hip.ptr(planes), c_long(planes.numel()), *size, c_int(layout), st)
        if layout == L420:
            hip.call('mg_jpeg_rgb', hip.ptr(planes), hip.ptr(out), *size, *epilogue, st)
        elif layout in LUMA:
            hip.call('mg_jpeg_rgb_hv', hip.ptr(planes), c_long(planes.numel()), hip.ptr(out), *size, *map(c_int, LUMA[layout]), *epilogue, st)
        else:
            hip.call('mg_jpegdec_rgb', hip.ptr(planes), c_long(planes.numel()), hip.ptr(out), *size, c_int(layout), *epilogue, st)
    return finish


def run(blob, recs, h, w, layout, *, sub_bytes=None, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """The launches themselves: `blob` uint8 device tensor holding the T segments, `recs` int32 (T, TAB_WORDS) host records whose offsets point
    into it. `out`: a preallocated contiguous destination of the right size and dtype (else allocated). Returns a `Decoded`."""
    S = _sub_bytes(sub_bytes)
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, TAB_WORDS)
    T = recs.shape[0]
    dev = blob.device
    hip.need_cuda(blob)
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError('blob must be a contiguous 1-D uint8 tensor')
    if T < 1 or (recs[:, 918] < 0).any() or (recs[:, 919] < 0).any() or int((recs[:, 918].astype(np.int64) + recs[:, 919]).max()) > blob.numel():
        raise ValueError('a segment lies outside the buffer')
    nsub = max(1, -(-int(recs[:, 919].max()) // S))
    wgs = -(-nsub // THREADS)
    max_launches = wgs + 1
    tabs = torch.from_numpy(recs).to(dev, non_blocking=True)
    exits = torch.empty((T, nsub), dtype=torch.int64, device=dev)
    counts = torch.empty((T, nsub), dtype=torch.int32, device=dev)
    first = torch.empty((T, nsub), dtype=torch.int32, device=dev)
    entries = torch.empty((T, wgs), dtype=torch.int64, device=dev)
    bounds = torch.zeros((2, T, wgs), dtype=torch.int64, device=dev)
    info = torch.zeros((4 + 2 * (max_launches + 1),), dtype=torch.int32, device=dev)
    r = Decoded()
    finish = finishing(r, tabs, T, h, w, layout, normalize, mean, std, out)
    coef = r.coef
    st = hip.stream

    def sync(k):
        hip.call('mg_jpegdec_sync', hip.ptr(blob), c_long(blob.numel()), hip.ptr(tabs), hip.ptr(exits), hip.ptr(counts), hip.ptr(entries),
                 hip.ptr(bounds), hip.ptr(info), c_int(info.numel()), c_long(T), c_int(nsub), c_int(S), c_int(layout), c_int(k), st())

    def output():
        hip.call('mg_jpegdec_coef', hip.ptr(blob), c_long(blob.numel()), hip.ptr(tabs), hip.ptr(exits), hip.ptr(counts), hip.ptr(first),
                 hip.ptr(coef), c_long(coef.numel()), hip.ptr(info), c_long(T), c_int(nsub), c_int(S), c_int(h), c_int(w), c_int(layout), st())
        hip.call('mg_jpegdec_dcsum', hip.ptr(coef), c_long(coef.numel()), hip.ptr(tabs), c_long(T), c_int(h), c_int(w), c_int(layout), st())
        finish()

    sync(0)
    k = 0
    if wgs > 1:
        k = 1
        sync(1)
    output()
    host = info.cpu().numpy()
    readbacks = 1
    again = False
    while k >= 1 and host[2 + 2 * k] != 0:
        if k >= max_launches:
            raise ValueError('the stream did not synchronise within %d launches' % (max_launches + 1))
        k += 1
        sync(k)
        host = info.cpu().numpy()
        readbacks += 1
        again = True
    if again:
        coef.zero_()
        info[0:1].zero_()
        output()
        host = info.cpu().numpy()
        readbacks += 1
    if host[0]:
        raise ValueError('a corrupt entropy-coded segment: ' + '; '.join(v for b, v in STATUS.items() if host[0] & b))
    r.rounds, r.launches, r.subsequences, r.readbacks = int(host[3::2].sum()), k + 1, nsub, readbacks
    return r


def datas_of(datas):
    """`datas` checked: a non-empty sequence of the bytes of files."""
    if isinstance(datas, (bytes, bytearray, memoryview)) or not hasattr(datas, '__len__'):
        raise TypeError('datas must be a sequence of the bytes of JPEG files (got %s)' % type(datas).__name__)
    if len(datas) < 1:
        raise ValueError('datas must hold at least one file')
    for d in datas:
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(d).__name__)


def one_geometry(plans):
    if any(p.geometry != plans[0].geometry for p in plans):
        raise ValueError('the files of a clip must share one size and one sampling layout (got %s)' % sorted({p.geometry for p in plans}))


def offsets_of(datas):
    """The offset of each file in the buffer that holds a clip's files one behind the other."""
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of files in one clip' % offsets[-1])
    return offsets[:-1]


def blob_of(datas, device):
    """That buffer: a uint8 tensor on `device`."""
    return torch.frombuffer(bytearray(b''.join(bytes(d) for d in datas)), dtype=torch.uint8).to(resolve_device(device), non_blocking=True)


def run_files(datas, plans, device, **kw):
    """Baseline files of one geometry and their plans -> records and blob -> `run` (`kw`: its keywords)."""
    recs = np.stack([record(p, int(o)) for p, o in zip(plans, offsets_of(datas))])
    h, w, layout = plans[0].geometry
    return run(blob_of(datas, device), recs, h, w, layout, **kw)


def _clip(datas, normalize, mean, std, device, sub_bytes):
    if isinstance(datas, (bytes, bytearray, memoryview)) or not hasattr(datas, '__len__'):
        raise TypeError('datas must be a sequence of the bytes of JPEG files (got %s)' % type(datas).__name__)
    if len(datas) < 1:
        raise ValueError('datas must hold at least one file')
    _sub_bytes(sub_bytes)
    float3(mean), float3(std)
    plans = [parse(d) for d in datas]
    one_geometry(plans)
    return run_files(datas, plans, device, sub_bytes=sub_bytes, normalize=normalize, mean=mean, std=std)


def decode_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, sub_bytes=None):
    """T JPEG files (a sequence of bytes objects) of one size and one sampling layout -> uint8 (T, h, w, 3) on the device, or with `normalize`
    fp32 (T, 3, h, w), from one set of launches. Files of differing geometry raise ValueError, unsupported ones `Unsupported`, corrupt entropy
    coding ValueError. Not graph-capturable (the module docstring says why); one read-back in the usual case."""
    return _clip(datas, normalize, mean, std, device, sub_bytes).out


def decode(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, sub_bytes=None):
    """The bytes of one JPEG file -> uint8 (h, w, 3) on the device: `np.asarray(Image.open(BytesIO(data)).convert("RGB"))`. With `normalize`
    fp32 (3, h, w): ToTensor + Normalize of that, the bits of `normalize_frames`. `sub_bytes`: the subsequence length (None = the measured
    default). Not graph-capturable: decoding is data-dependent and the host reads the `info` words back: one read-back in the usual case."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return _clip([data], normalize, mean, std, device, sub_bytes).out[0]


def decode_stats(datas, *, device=None, sub_bytes=None):
    """`decode_clip` returning the whole `Decoded` record (coefficients, planes, rounds, launches, read-backs): for tests and tools/jpegdec_bench.py."""
    return _clip(datas, False, IMAGENET_MEAN, IMAGENET_STD, device, sub_bytes)
