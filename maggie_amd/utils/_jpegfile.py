"""The marker walk of a JPEG file, host only: what the file holds, with no word on what the device decodes beyond what both decoders refuse
alike. `jpegdec.parse`, `jpegprog.parse` and `jpegsamp.parse` are this walk plus the acceptance rules of each, handed in as `on_frame` and
`on_scan` so that they speak at the marker at which they always spoke: of two defects of one file the same one is named."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_SOF = {0xC1: 'extended sequential', 0xC2: 'progressive', 0xC3: 'lossless', 0xC9: 'arithmetic-coded sequential',
        0xCA: 'arithmetic-coded progressive'}


class Unsupported(ValueError):
    """A JPEG file outside the set the device decodes (or not a JPEG file): fall back to PIL. `before_frame`: raised by `walk` in front of the frame
    header it accepts."""
    before_frame = False


class Scan:
    """One scan: `selectors` ((component id, DC table id, AC table id) per component), `Ss`, `Se`, `Ah`, `Al`, `restart_interval`, `offset` /
    `length` of its entropy-coded segment; `jpegprog` adds `components` (indices into the frame's components, frame order), `dc` / `ac` (per
    component the table (counts, values) its selector named at this SOS, None where the scan needs none) and `first`."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def script(self):
        return self.components, self.Ss, self.Se, self.Ah, self.Al


class JpegFile:
    """What `walk` found: `frame` (dict: `sof`, `height`, `width`, `comps` [(id, h, v, quantisation table id)]), the tables in force where the
    walk ended -- `quant` {id: int32 (64,) natural order}, `dc` / `ac` {id: (counts uint8 (16,), values uint8 (n,))} --, `restart_interval`,
    `scans` (the `Scan`s in file order), `next`, the marker byte behind the last segment, and `nbytes` of the file."""

    def __init__(self):
        self.frame, self.quant, self.dc, self.ac, self.restart_interval, self.scans, self.next, self.nbytes = None, {}, {}, {}, 0, [], 0, 0
        self.at_frame = False                                  # the walk has reached the frame header it accepts


def walk(data, progressive, on_frame, on_scan):
    """The markers of one file -> JpegFile. `progressive`: SOF2 and every scan up to EOI, else SOF0 and the first scan only (what lies behind
    it is the caller's to judge, by `next`); None: whichever of the two frame headers comes, the progressive rules in front of it (an
    `Unsupported` there, `before_frame`, says no more than that the baseline walk has to name what the file is). `on_frame(file)` runs at the
    frame header and `on_scan(file, scan)` at each SOS, in front of the search for the end of its segment: the caller's acceptance rules.
    Raises `Unsupported`."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    f = JpegFile()
    try:
        _walk(f, bytes(data), progressive, on_frame, on_scan)
    except Unsupported as e:
        e.before_frame = not f.at_frame
        raise
    return f


def _walk(f, d, progressive, on_frame, on_scan):
    n = f.nbytes = len(d)
    either, ids_past_baseline = progressive is None, False
    progressive = progressive or either
    sof = 0xC2 if progressive else 0xC0
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Unsupported('not a JPEG file (no SOI marker)')
    p = 2
    while True:
        if progressive and p + 2 > n:
            raise Unsupported('the file ends without an EOI marker')
        if not progressive and p + 4 > n:
            raise Unsupported('the file ends inside its headers')
        if d[p] != 0xFF:
            raise Unsupported('expected a marker at byte %d' % p)
        m = d[p + 1]
        if m == 0xFF:                                          # fill byte
            p += 1
            continue
        if m == 0xD9:
            if progressive and not (either and f.frame is None):
                break
            raise Unsupported('EOI before any scan')
        if p + 4 > n:
            raise Unsupported('the file ends inside its headers')
        size = (d[p + 2] << 8) | d[p + 3]
        seg = d[p + 4:p + 2 + size]
        if size < 2 or p + 2 + size > n:
            raise Unsupported('a marker segment runs past the end of the file')
        if either and m == 0xC0 and f.frame is None:           # a baseline file after all, if the baseline rules took what came so far
            if ids_past_baseline:
                raise Unsupported('a DHT segment with an id that only progressive files may use')
            progressive, sof = False, 0xC0
        if m == sof:
            f.at_frame = True
            if f.frame is not None:
                raise Unsupported('more than one frame header')
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise Unsupported('a malformed SOF%d segment' % (m - 0xC0))
            if seg[0] != 8:
                raise Unsupported('%d-bit samples (only 8-bit %s is decoded)' % (seg[0], 'progressive' if progressive else 'baseline'))
            f.frame = dict(sof=m, height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4],
                           comps=[(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])])
            on_frame(f)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if progressive and m < 0xC2:
                raise Unsupported('SOF%d (sequential): use jpegdec for baseline files' % (m - 0xC0))
            raise Unsupported('SOF%d (%s): only %s is decoded' % (m - 0xC0, _SOF.get(m, 'differential or arithmetic'),
                                                                  'SOF2 with Huffman coding' if progressive else 'SOF0 baseline'))
        elif m == 0xCC:
            raise Unsupported('arithmetic coding conditioning (DAC)')
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Unsupported('a malformed DHT segment')
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = seg[q + 1:q + 17]
                total = sum(counts)
                if tc > 1 or th > (3 if progressive else 1) or total > 256 or q + 17 + total > len(seg):
                    raise Unsupported('a malformed DHT segment (class %d, id %d)' % (tc, th))
                ids_past_baseline |= th > 1
                code = 0
                for l in range(16):
                    code += counts[l]
                    if code > (2 << l):
                        raise Unsupported('a DHT table whose code lengths overflow')
                    code <<= 1
                (f.ac if tc else f.dc)[th] = (np.frombuffer(counts, np.uint8).copy(), np.frombuffer(seg[q + 17:q + 17 + total], np.uint8).copy())
                q += 17 + total
        elif m == 0xDB:
            if f.scans:
                raise Unsupported('a DQT segment behind the first scan')
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise Unsupported('a 16-bit quantisation table')
                if (seg[q] & 15) > 3 or q + 65 > len(seg):
                    raise Unsupported('a malformed DQT segment')
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                f.quant[seg[q] & 15] = t
                q += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise Unsupported('a malformed DRI segment')
            f.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise Unsupported('DNL (the height is defined after the scan)')
        elif m == 0xEE and seg[:5] == b'Adobe' and len(seg) >= 12:
            if seg[11] != 1:
                raise Unsupported('an Adobe APP14 marker with transform %d (only YCbCr is decoded)' % seg[11])
        elif m == 0xDA:
            if f.frame is None:
                raise Unsupported('SOS before SOF%d' % (sof - 0xC0))
            ns = seg[0] if seg else 0
            if (progressive and ns < 1) or len(seg) != 4 + 2 * ns:
                raise Unsupported('a malformed SOS segment')
            scan = Scan(selectors=[(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)], Ss=seg[1 + 2 * ns],
                        Se=seg[2 + 2 * ns], Ah=seg[3 + 2 * ns] >> 4, Al=seg[3 + 2 * ns] & 15, restart_interval=f.restart_interval)
            on_scan(f, scan)
            scan.offset = p = p + 2 + size
            while True:                                        # up to the first marker that is neither a stuffed 0xFF00 nor RSTn
                p = d.find(b'\xff', p)
                if p < 0 or p + 1 >= n:
                    raise Unsupported('no EOI marker behind the scan')
                if d[p + 1] == 0 or 0xD0 <= d[p + 1] <= 0xD7:
                    p += 2
                    continue
                if d[p + 1] == 0xFF:
                    p += 1
                    continue
                break
            scan.length = p - scan.offset
            f.scans.append(scan)
            f.next = d[p + 1]
            if progressive:
                continue
            break
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise Unsupported('marker 0xFF%02X is not decoded' % m)
        p += 2 + size
