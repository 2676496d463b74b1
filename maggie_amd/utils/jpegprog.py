"""Progressive JPEG files decoded on the device (HIP kernel of csrc/jpegprog.hip) -- the other half of the reference's `T.Load`
(maggie/dataloader/transforms.py:38-66): photographs collected from the web are very often `SOF2`, which `jpegdec.parse` refuses.

  * `parse`        the marker walk, host only: size, sampling layout, quantisation tables, and per scan its components, `Ss`, `Se`, `Ah`, `Al`, the
                   Huffman tables and restart interval in force at its `SOS` (contents, not ids) and where its entropy-coded segment lies. Checks
                   that the progression is legal and COMPLETE; raises `jpegdec.Unsupported` by name for everything else, before any launch.
  * `decode` / `decode_clip` / `decode_stats`   the contracts, dtypes and shapes of their `jpegdec` namesakes.
  * `load` / `load_clip`   the one entry a loader calls: a file `jpegdec.parse` accepts goes the baseline way, one `parse` here accepts the
                   progressive way; a mixed clip decodes each group once into slices of one tensor.

A progressive file holds the coefficients of its baseline twin, coded in several scans. The scans of a file fall into CHAINS that do not depend
on each other: all DC scans, and per component its AC scans, each in file order. One wave decodes one chain, every chain
of every file of a clip in ONE launch; then `mg_jpegdec_idct` and the colour kernels of `jpegdec`, unchanged. The DC terms arrive final, so there
is no `mg_jpegdec_dcsum`. One read-back per call: the status words, at the end; a status bit becomes a ValueError. Wrong types raise before any
launch. There is no CPU fallback.

Not decoded (Unsupported): sequential files (use `jpegdec`), arithmetic coding, samplings other than 4:2:0 / 4:4:4 / grey, 12-bit samples,
16-bit tables, DNL, a DQT between scans, and scan scripts that leave a coefficient short of its last bit (libjpeg smooths those across blocks)."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import jpegdec
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, resolve_device
from .jpegdec import BLOCKS_PER_MCU, GREY, L420, L444, MAX_BYTES, Unsupported, ZIGZAG, huffman_words, planes_size
from .photometric import MAX_SIDE, NORM, RAW

THREADS, SCAN_WORDS, CHAIN_WORDS = 64, 480, 4               # MG_JPEGPROG_THREADS / _SCAN_WORDS / _CHAIN_WORDS (include/maggie_hip.h)
STATUS = dict(jpegdec.STATUS)
STATUS.update({32:'a refinement symbol that is not a 1-bit value, or a value past the end of its band',
               64: "bytes left in a scan's segment behind its last block", 128: 'a scan record outside the buffers'})
_EMPTY = (np.zeros(16, np.uint8), np.zeros(0, np.uint8))


class Scan:
    """One scan: `components` (indices into the frame's components, frame order), `Ss`, `Se`, `Ah`, `Al`, `dc` / `ac` (per component the table
    (counts, values) its selector named at this SOS, None where the scan needs none), `restart_interval`, `offset` / `length` of its segment."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def script(self):
        return self.components, self.Ss, self.Se, self.Ah, self.Al


class ProgPlan:
    """What `parse` found: `width`, `height`, `layout`, `sampling`, `quantization`, `qtables` (int32 (3, 64)) as in `jpegdec.JpegPlan`; `scans`
    (the `Scan`s in file order); `chains`: [('dc', None, [scan numbers])] + [('ac', component, [scan numbers])] per component."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def geometry(self):
        return self.height, self.width, self.layout

    @property
    def script(self):
        return [s.script for s in self.scans]


def parse(data):
    """The marker walk of one SOF2 file's bytes -> ProgPlan. Host only; raises `Unsupported` by name for what the device does not decode."""
    return _parse(data, jpegdec._layout)


def _parse(data, layout_of):
    """`parse` with the accepted samplings given, as `jpegdec._parse`."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Unsupported('not a JPEG file (no SOI marker)')
    quant, dc, ac = {}, {}, {}
    frame, scans, ri, p = None, [], 0, 2
    while True:
        if p + 2 > n:
            raise Unsupported('the file ends without an EOI marker')
        if d[p] != 0xFF:
            raise Unsupported('expected a marker at byte %d' % p)
        m = d[p + 1]
        if m == 0xFF:                                          # fill byte
            p += 1
            continue
        if m == 0xD9:
            break
        if p + 4 > n:
            raise Unsupported('the file ends inside its headers')
        size = (d[p + 2] << 8) | d[p + 3]
        seg = d[p + 4:p + 2 + size]
        if size < 2 or p + 2 + size > n:
            raise Unsupported('a marker segment runs past the end of the file')
        if m == 0xC2:
            if frame is not None:
                raise Unsupported('more than one frame header')
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise Unsupported('a malformed SOF2 segment')
            if seg[0] != 8:
                raise Unsupported('%d-bit samples (only 8-bit progressive is decoded)' % seg[0])
            frame = dict(height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4],
                         comps=[(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])])
            _check_frame(frame, layout_of)
        elif m in (0xC0, 0xC1):
            raise Unsupported('SOF%d (sequential): use jpegdec for baseline files' % (m - 0xC0))
        elif 0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            names = {0xC3: 'lossless', 0xC9: 'arithmetic-coded sequential', 0xCA: 'arithmetic-coded progressive'}
            raise Unsupported('SOF%d (%s): only SOF2 with Huffman coding is decoded' % (m - 0xC0, names.get(m, 'differential or arithmetic')))
        elif m == 0xCC:
            raise Unsupported('arithmetic coding conditioning (DAC)')
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Unsupported('a malformed DHT segment')
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = np.frombuffer(seg[q + 1:q + 17], np.uint8)
                total = int(counts.sum())
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    raise Unsupported('a malformed DHT segment (class %d, id %d)' % (tc, th))
                code = 0
                for l in range(16):
                    code += int(counts[l])
                    if code > (2 << l):
                        raise Unsupported('a DHT table whose code lengths overflow')
                    code <<= 1
                (ac if tc else dc)[th] = (counts.copy(), np.frombuffer(seg[q + 17:q + 17 + total], np.uint8).copy())
                q += 17 + total
        elif m == 0xDB:
            if scans:
                raise Unsupported('a DQT segment behind the first scan')
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise Unsupported('a 16-bit quantisation table')
                if (seg[q] & 15) > 3 or q + 65 > len(seg):
                    raise Unsupported('a malformed DQT segment')
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                quant[seg[q] & 15] = t
                q += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise Unsupported('a malformed DRI segment')
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise Unsupported('DNL (the height is defined after the scan)')
        elif m == 0xEE and seg[:5] == b'Adobe' and len(seg) >= 12:
            if seg[11] != 1:
                raise Unsupported('an Adobe APP14 marker with transform %d (only YCbCr is decoded)' % seg[11])
        elif m == 0xDA:
            if frame is None:
                raise Unsupported('SOS before SOF2')
            ns = seg[0] if seg else 0
            if ns < 1 or len(seg) != 4 + 2 * ns:
                raise Unsupported('a malformed SOS segment')
            ids = [c[0] for c in frame['comps']]
            sel = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            if any(s[0] not in ids for s in sel):
                raise Unsupported('a scan of a component the frame does not have')
            comps = tuple(ids.index(s[0]) for s in sel)
            if any(b <= a for a, b in zip(comps, comps[1:])):
                raise Unsupported('a scan whose components are not in frame order')
            Ss, Se, Ah, Al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            first, need_dc, need_ac = Ah == 0, Ss == 0 and Ah == 0, Ss > 0
            for _, td, ta in sel:
                if (need_dc and td not in dc) or (need_ac and ta not in ac):
                    raise Unsupported('a scan that selects a Huffman table that is not defined (DC %d, AC %d)' % (td, ta))
            start = p + 2 + size
            p = start
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
            scans.append(Scan(components=comps, Ss=Ss, Se=Se, Ah=Ah, Al=Al, dc=[dc[td] if need_dc else None for _, td, _ in sel],
                              ac=[ac[ta] if need_ac else None for _, _, ta in sel], restart_interval=ri, offset=start, length=p - start,
                              first=first))
            continue
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise Unsupported('marker 0xFF%02X is not decoded' % m)
        p += 2 + size
    if frame is None or not scans:
        raise Unsupported('EOI before any scan')
    comps = frame['comps']
    for c in comps:
        if c[3] not in quant:
            raise Unsupported('quantisation table %d is not defined' % c[3])
    _check_progression(scans, len(comps))
    if n > MAX_BYTES:
        raise Unsupported('a file of %d bytes' % n)
    chains = [('dc', None, [k for k, s in enumerate(scans) if s.Ss == 0])]
    chains += [('ac', c, [k for k, s in enumerate(scans) if s.Ss > 0 and s.components == (c,)]) for c in range(len(comps))]
    qt = np.stack([quant[comps[min(k, len(comps) - 1)][3]] for k in range(3)]).astype(np.int32)
    return ProgPlan(width=frame['width'], height=frame['height'], layout=frame['layout'], sampling=frame['sampling'], quantization=quant, qtables=qt,
                    scans=scans, chains=chains)


def _check_frame(frame, layout_of):
    comps, w, h = frame['comps'], frame['width'], frame['height']
    if len(comps) not in (1, 3):
        raise Unsupported('%d components (only YCbCr and greyscale are decoded)' % len(comps))
    if h == 0:
        raise Unsupported('DNL (the height is defined after the scan)')
    if w < 1 or w > MAX_SIDE or h > MAX_SIDE:
        raise Unsupported('%d x %d: sides of 1..%d are decoded' % (w, h, MAX_SIDE))
    if len({c[0] for c in comps}) != len(comps):
        raise Unsupported('two components with one identifier')
    sampling = tuple((c[1], c[2]) for c in comps)
    frame.update(sampling=sampling, layout=layout_of(sampling))


def _check_progression(scans, ncomp):
    """T.81 G.1.1.1: a legal script, and a complete one -- by EOI every coefficient of every component has reached Al == 0."""
    al = [[None] * 64 for _ in range(ncomp)]
    for k, s in enumerate(scans):
        where = 'scan %d (Ss %d, Se %d, Ah %d, Al %d)' % (k, s.Ss, s.Se, s.Ah, s.Al)
        if s.Se > 63 or s.Ss > s.Se or (s.Ss == 0 and s.Se != 0) or s.Al > 13 or s.Ah > 13:
            raise Unsupported('an illegal progression: %s has an impossible band' % where)
        if s.Ss > 0 and len(s.components) != 1:
            raise Unsupported('an illegal progression: %s is an AC scan of %d components' % (where, len(s.components)))
        for c in s.components:
            if s.Ss > 0 and al[c][0] is None:
                raise Unsupported('an illegal progression: %s comes before the first DC scan of its component' % where)
            for z in range(s.Ss, s.Se + 1):
                if al[c][z] is None:
                    if s.Ah != 0:
                        raise Unsupported('an illegal progression: %s refines a coefficient that has no first scan' % where)
                elif s.Ah != al[c][z] or s.Al != s.Ah - 1:
                    raise Unsupported('an illegal progression: %s does not continue at the bit the scan before left (Al %d)' % (where, al[c][z]))
                al[c][z] = s.Al
    for c in range(ncomp):
        short = [z for z in range(64) if al[c][z] != 0]
        if short:
            raise Unsupported('an incomplete progression: coefficient %d of component %d never reaches its last bit (libjpeg smooths such files '
                              'across blocks)' % (short[0], c))


def records(plan, offset, frame, first):
    """A file's scan records int32 (scans, SCAN_WORDS) in chain order and its chain records int32 (chains, CHAIN_WORDS), with the file at `offset`
    of the buffer, for frame `frame`, its first scan record being number `first` of the launch's."""
    recs, chains = [], []
    ny = plan.sampling[0][0] * plan.sampling[0][1]             # an MCU: the luma blocks, then Cb, then Cr
    slots_of = (list(range(ny)), [ny], [ny + 1]) if len(plan.sampling) == 3 else ([0],)
    for _, _, numbers in plan.chains:
        if not numbers:
            continue
        chains.append([frame, first + len(recs), len(numbers), 0])
        for k in numbers:
            s = plan.scans[k]
            rec = np.zeros(SCAN_WORDS, np.int32)
            tables = []
            if s.Ss > 0:
                tables = [s.ac[0]]
            elif s.Ah == 0:
                tables = list(dict.fromkeys((bytes(t[0]), bytes(t[1])) for t in s.dc))
                if len(tables) > 2:
                    raise Unsupported('a DC scan with more than two Huffman tables')
                which = [tables.index((bytes(t[0]), bytes(t[1]))) for t in s.dc]
                tables = [(np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)) for a, b in tables]
            for j, t in enumerate(tables):
                rec[228 * j:228 * (j + 1)] = huffman_words(*t)
            rec[456:463] = offset + s.offset, s.length, s.restart_interval, s.Ss, s.Se, s.Ah, s.Al
            if len(s.components) > 1:
                words = [sl | (c << 4) | ((which[j] if s.Ah == 0 else 0) << 8) for j, c in enumerate(s.components) for sl in slots_of[c]]
                rec[463] = len(words)
                rec[466:466 + len(words)] = words
            else:
                rec[464] = s.components[0]
            recs.append(rec)
    return np.stack(recs), np.asarray(chains, np.int32).reshape(-1, CHAIN_WORDS)


class Decoded:
    """What `run` leaves on the device: `out`, the coefficient blocks `coef` (T, blocks, 64) int16, the component `planes`; on the host `chains`
    (waves of the chain launch), `launches` (kernel launches of the call) and `readbacks`."""


def run(blob, scans, chains, qtables, h, w, layout, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, hv=None):
    """The launches themselves: `blob` uint8 device tensor holding the T files, `scans` int32 (S, SCAN_WORDS) and `chains` int32 (C, CHAIN_WORDS)
    host records whose offsets point into it (`records`), `qtables` int32 (T, 3, 64). `out`: a preallocated contiguous destination of the right
    size and dtype (else allocated). `hv`: the luma sampling (hs, vs) of `jpegsamp`'s layouts, which run the `_hv` entries (`layout` is then not
    passed on). Returns a `Decoded`."""
    scans = np.ascontiguousarray(scans, np.int32).reshape(-1, SCAN_WORDS)
    chains = np.ascontiguousarray(chains, np.int32).reshape(-1, CHAIN_WORDS)
    qtables = np.ascontiguousarray(qtables, np.int32).reshape(-1, 192)
    T = qtables.shape[0]
    dev = blob.device
    hip.need_cuda(blob)
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError('blob must be a contiguous 1-D uint8 tensor')
    if (hv is None and layout not in BLOCKS_PER_MCU) or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError('h, w must be in 1..%d and layout one of L420, L444, GREY' % MAX_SIDE)
    if T < 1 or len(scans) < 1 or len(chains) < 1 or blob.numel() > MAX_BYTES:
        raise ValueError('at least one file, one scan and one chain, and at most %d bytes' % MAX_BYTES)
    if (scans[:, 456] < 0).any() or (scans[:, 457] < 0).any() or int((scans[:, 456].astype(np.int64) + scans[:, 457]).max()) > blob.numel():
        raise ValueError('a segment lies outside the buffer')
    if (chains[:, 0] < 0).any() or (chains[:, 0] >= T).any() or (chains[:, 1:3] < 0).any() or \
            int((chains[:, 1].astype(np.int64) + chains[:, 2]).max()) > len(scans):
        raise ValueError('a chain lies outside the scan records or the frames')
    epilogue = NORM if normalize else RAW
    tabs_host = np.zeros((T, jpegdec.TAB_WORDS), np.int32)
    tabs_host[:, 928:1120] = qtables
    tabs = torch.from_numpy(tabs_host).to(dev, non_blocking=True)
    d_scans = torch.from_numpy(scans).to(dev, non_blocking=True)
    d_chains = torch.from_numpy(chains).to(dev, non_blocking=True)
    info = torch.zeros((T,), dtype=torch.int32, device=dev)
    if hv is None:
        side = 16 if layout == L420 else 8
        nblocks = ((w + side - 1) // side) * ((h + side - 1) // side) * BLOCKS_PER_MCU[layout]
        nplanes = planes_size(T, h, w, layout)
    else:
        nblocks, per_frame = jpegdec.hv_geometry(h, w, *hv)[:2]
        nplanes = T * per_frame
    coef = torch.zeros((T, nblocks, 64), dtype=torch.int16, device=dev)
    planes = torch.empty((nplanes,), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((T, 3, h, w) if normalize else (T, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=dev)
    elif out.numel() != T * h * w * 3 or out.dtype != (torch.float32 if normalize else torch.uint8) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous %s tensor of %d elements on %s' % ('float32' if normalize else 'uint8', T * h * w * 3, dev))
    st = hip.stream
    launch_chains(blob, d_scans, d_chains, coef, info, T, h, w, layout, hv)
    if hv is not None:
        hip.call('mg_jpegdec_idct_hv', hip.ptr(coef), c_long(coef.numel()), hip.ptr(tabs), hip.ptr(planes), c_long(planes.numel()), c_long(T),
                 c_int(h), c_int(w), c_int(hv[0]), c_int(hv[1]), st())
        hip.call('mg_jpeg_rgb_hv', hip.ptr(planes), c_long(planes.numel()), hip.ptr(out), c_long(T), c_int(h), c_int(w), c_int(hv[0]), c_int(hv[1]),
                 c_int(epilogue), float3(mean), float3(std), st())
    else:
        hip.call('mg_jpegdec_idct', hip.ptr(coef), c_long(coef.numel()), hip.ptr(tabs), hip.ptr(planes), c_long(planes.numel()), c_long(T),
                 c_int(h), c_int(w), c_int(layout), st())
        if layout == L420:
            hip.call('mg_jpeg_rgb', hip.ptr(planes), hip.ptr(out), c_long(T), c_int(h), c_int(w), c_int(epilogue), float3(mean), float3(std), st())
        else:
            hip.call('mg_jpegdec_rgb', hip.ptr(planes), c_long(planes.numel()), hip.ptr(out), c_long(T), c_int(h), c_int(w), c_int(layout),
                     c_int(epilogue), float3(mean), float3(std), st())
    host = info.cpu().numpy()
    for t in np.flatnonzero(host):
        raise ValueError('a corrupt entropy-coded segment (file %d): %s' % (t, '; '.join(v for b, v in STATUS.items() if host[t] & b)))
    r = Decoded()
    r.out, r.coef, r.planes = out.reshape((T, 3, h, w) if normalize else (T, h, w, 3)), coef, planes
    r.chains, r.launches, r.readbacks = len(chains), 3, 1
    return r


def launch_chains(blob, d_scans, d_chains, coef, info, T, h, w, layout, hv=None):
    """The chain launch alone (tools/jpegprog_bench.py times subsets of the chains with it): device tensors throughout."""
    geo = (c_int(layout),) if hv is None else (c_int(hv[0]), c_int(hv[1]))
    hip.call('mg_jpegprog_chains' if hv is None else 'mg_jpegprog_chains_hv', hip.ptr(blob), c_long(blob.numel()), hip.ptr(d_scans),
             c_long(d_scans.shape[0]), hip.ptr(d_chains), c_long(d_chains.shape[0]), hip.ptr(coef), c_long(coef.numel()), hip.ptr(info), c_long(T),
             c_int(h), c_int(w), *geo, hip.stream())


def _datas(datas):
    if isinstance(datas, (bytes, bytearray, memoryview)) or not hasattr(datas, '__len__'):
        raise TypeError('datas must be a sequence of the bytes of JPEG files (got %s)' % type(datas).__name__)
    if len(datas) < 1:
        raise ValueError('datas must hold at least one file')
    for d in datas:
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(d).__name__)


def _one_geometry(plans):
    if any(p.geometry != plans[0].geometry for p in plans):
        raise ValueError('the files of a clip must share one size and one sampling layout (got %s)' % sorted({p.geometry for p in plans}))


def pack(plans, datas):
    """The host side of a clip: (file bytes joined, scan records, chain records with the longest chains first, quantisation tables)."""
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of files in one clip' % offsets[-1])
    scans, chains, first = [], [], 0
    for t, (p, o) in enumerate(zip(plans, offsets[:-1])):
        s, c = records(p, int(o), t, first)
        scans.append(s)
        chains.append(c)
        first += len(s)
    scans, chains = np.concatenate(scans), np.concatenate(chains)
    size = np.array([scans[a:a + n, 457].sum() for _, a, n, _ in chains])
    chains = chains[np.argsort(-size, kind='stable')]         # the waves that run longest start first
    return b''.join(bytes(d) for d in datas), scans, chains, np.stack([p.qtables for p in plans])


def _clip(datas, normalize, mean, std, device, out=None, plans=None):
    _datas(datas)
    float3(mean), float3(std)
    plans = [parse(d) for d in datas] if plans is None else plans
    _one_geometry(plans)
    joined, scans, chains, qt = pack(plans, datas)
    device = resolve_device(device)
    blob = torch.frombuffer(bytearray(joined), dtype=torch.uint8).to(device, non_blocking=True)
    h, w, layout = plans[0].geometry
    return run(blob, scans, chains, qt, h, w, layout, normalize=normalize, mean=mean, std=std, out=out)


def decode_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """T progressive JPEG files (a sequence of bytes objects) of one size and one sampling layout -> uint8 (T, h, w, 3) on the device, or with
    `normalize` fp32 (T, 3, h, w), from one set of launches; scan scripts and tables are per file. Files of differing geometry raise ValueError,
    unsupported ones `Unsupported`, corrupt entropy coding ValueError. Not graph-capturable (the status words are read back); one read-back."""
    return _clip(datas, normalize, mean, std, device).out


def decode(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """The bytes of one progressive JPEG file -> uint8 (h, w, 3) on the device: `np.asarray(Image.open(BytesIO(data)).convert("RGB"))`. With
    `normalize` fp32 (3, h, w): ToTensor + Normalize of that, the bits of `normalize_frames`. Not graph-capturable: the status words are read
    back at the end, one read-back per call."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return _clip([data], normalize, mean, std, device).out[0]


def decode_stats(datas, *, device=None):
    """`decode_clip` returning the whole `Decoded` record (coefficients, planes, chains, launches, read-backs): for tests and tools/jpegprog_bench.py."""
    return _clip(datas, False, IMAGENET_MEAN, IMAGENET_STD, device)


def _baseline(datas, plans, normalize, mean, std, device, out):
    """`jpegdec`'s clip into `out` (jpegdec.run's own `out=`)."""
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of files in one clip' % offsets[-1])
    recs = np.stack([jpegdec.record(p, int(o)) for p, o in zip(plans, offsets[:-1])])
    blob = torch.frombuffer(bytearray(b''.join(bytes(d) for d in datas)), dtype=torch.uint8).to(device, non_blocking=True)
    h, w, layout = plans[0].geometry
    return jpegdec.run(blob, recs, h, w, layout, normalize=normalize, mean=mean, std=std, out=out)


def load_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode_clip` for whatever a loader finds: each file goes the way of the parser that accepts it (`jpegdec.parse` first, then `parse`; if
    neither does, the `Unsupported` of `jpegdec.parse` propagates). The baseline files are decoded in one set of launches and the progressive
    files in another, into slices of one tensor; the result is in the order of `datas`."""
    _datas(datas)
    float3(mean), float3(std)
    kinds, plans = [], []
    for d in datas:
        try:
            plans.append(jpegdec.parse(d))
            kinds.append(0)
        except Unsupported as e:
            try:
                plans.append(parse(d))
            except Unsupported:
                raise e from None
            kinds.append(1)
    _one_geometry(plans)
    device = resolve_device(device)
    h, w, _ = plans[0].geometry
    T = len(datas)
    order = [k for k in range(T) if kinds[k] == 0] + [k for k in range(T) if kinds[k] == 1]
    nb = kinds.count(0)
    out = torch.empty((T, 3, h, w) if normalize else (T, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=device)
    if nb:
        _baseline([datas[k] for k in order[:nb]], [plans[k] for k in order[:nb]], normalize, mean, std, device, out[:nb])
    if nb < T:
        _clip([datas[k] for k in order[nb:]], normalize, mean, std, device, out=out[nb:], plans=[plans[k] for k in order[nb:]])
    if order == list(range(T)):
        return out
    back = np.empty(T, np.int64)
    back[order] = np.arange(T)
    return out[torch.from_numpy(back).to(device)]


def load(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode` for whatever a loader finds: a baseline file through `jpegdec`, a progressive one through this module."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return load_clip([data], normalize=normalize, mean=mean, std=std, device=device)[0]
