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
from ._jpegfile import Scan, walk                           # noqa: F401  (Scan: for the callers of this module)
from .jpegdec import MAX_BYTES, Unsupported, huffman_words
from .photometric import MAX_SIDE

THREADS, SCAN_WORDS, CHAIN_WORDS = 64, 480, 4               # MG_JPEGPROG_THREADS / _SCAN_WORDS / _CHAIN_WORDS (include/maggie_hip.h)
STATUS = dict(jpegdec.STATUS)
STATUS.update({32:'a refinement symbol that is not a 1-bit value, or a value past the end of its band',
               64: "bytes left in a scan's segment behind its last block", 128: 'a scan record outside the buffers'})
_EMPTY = (np.zeros(16, np.uint8), np.zeros(0, np.uint8))


class ProgPlan:
    """What `parse` found: `width`, `height`, `layout`, `sampling`, `quantization`, `qtables` (int32 (3, 64)) as in `jpegdec.JpegPlan`; `scans`
    (the `Scan`s in file order); `chains`: [('dc', None, [scan numbers])] + [('ac', component, [scan numbers])] per component."""
    kind = 'progressive'

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


def rules(layout_of):
    """(on_frame, on_scan, plan) of a progressive file, as `jpegdec.rules`."""
    def on_frame(f):
        jpegdec.check_frame(f.frame)
        f.frame['layout'] = layout_of(f.frame['sampling'])

    def on_scan(f, scan):                                      # the tables are taken by content: a later DHT may redefine an id
        ids = [c[0] for c in f.frame['comps']]
        if any(s[0] not in ids for s in scan.selectors):
            raise Unsupported('a scan of a component the frame does not have')
        comps = tuple(ids.index(s[0]) for s in scan.selectors)
        if any(b <= a for a, b in zip(comps, comps[1:])):
            raise Unsupported('a scan whose components are not in frame order')
        need_dc, need_ac = scan.Ss == 0 and scan.Ah == 0, scan.Ss > 0
        for _, td, ta in scan.selectors:
            if (need_dc and td not in f.dc) or (need_ac and ta not in f.ac):
                raise Unsupported('a scan that selects a Huffman table that is not defined (DC %d, AC %d)' % (td, ta))
        scan.components, scan.first = comps, scan.Ah == 0
        scan.dc = [f.dc[td] if need_dc else None for _, td, _ in scan.selectors]
        scan.ac = [f.ac[ta] if need_ac else None for _, _, ta in scan.selectors]

    def plan(f):
        if f.frame is None or not f.scans:
            raise Unsupported('EOI before any scan')
        ncomp = len(f.frame['comps'])
        qt = jpegdec.output_tables(f)
        _check_progression(f.scans, ncomp)
        if f.nbytes > MAX_BYTES:
            raise Unsupported('a file of %d bytes' % f.nbytes)
        chains = [('dc', None, [k for k, s in enumerate(f.scans) if s.Ss == 0])]
        chains += [('ac', c, [k for k, s in enumerate(f.scans) if s.Ss > 0 and s.components == (c,)]) for c in range(ncomp)]
        return ProgPlan(width=f.frame['width'], height=f.frame['height'], layout=f.frame['layout'], sampling=f.frame['sampling'], quantization=f.quant,
                        qtables=qt, scans=f.scans, chains=chains)
    return on_frame, on_scan, plan


def _parse(data, layout_of):
    on_frame, on_scan, plan = rules(layout_of)
    return plan(walk(data, True, on_frame, on_scan))


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


def run(blob, scans, chains, qtables, h, w, layout, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """The launches themselves: `blob` uint8 device tensor holding the T files, `scans` int32 (S, SCAN_WORDS) and `chains` int32 (C, CHAIN_WORDS)
    host records whose offsets point into it (`records`), `qtables` int32 (T, 3, 64). `out`: a preallocated contiguous destination of the right
    size and dtype (else allocated). Returns a `Decoded`."""
    scans = np.ascontiguousarray(scans, np.int32).reshape(-1, SCAN_WORDS)
    chains = np.ascontiguousarray(chains, np.int32).reshape(-1, CHAIN_WORDS)
    qtables = np.ascontiguousarray(qtables, np.int32).reshape(-1, 192)
    T = qtables.shape[0]
    dev = blob.device
    hip.need_cuda(blob)
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError('blob must be a contiguous 1-D uint8 tensor')
    if layout not in jpegdec._HV or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError('h, w must be in 1..%d and layout one of the six of jpegdec' % MAX_SIDE)
    if T < 1 or len(scans) < 1 or len(chains) < 1 or blob.numel() > MAX_BYTES:
        raise ValueError('at least one file, one scan and one chain, and at most %d bytes' % MAX_BYTES)
    if (scans[:, 456] < 0).any() or (scans[:, 457] < 0).any() or int((scans[:, 456].astype(np.int64) + scans[:, 457]).max()) > blob.numel():
        raise ValueError('a segment lies outside the buffer')
    if (chains[:, 0] < 0).any() or (chains[:, 0] >= T).any() or (chains[:, 1:3] < 0).any() or \
            int((chains[:, 1].astype(np.int64) + chains[:, 2]).max()) > len(scans):
        raise ValueError('a chain lies outside the scan records or the frames')
    tabs_host = np.zeros((T, jpegdec.TAB_WORDS), np.int32)
    tabs_host[:, 928:1120] = qtables
    tabs = torch.from_numpy(tabs_host).to(dev, non_blocking=True)
    d_scans = torch.from_numpy(scans).to(dev, non_blocking=True)
    d_chains = torch.from_numpy(chains).to(dev, non_blocking=True)
    info = torch.zeros((T,), dtype=torch.int32, device=dev)
    r = Decoded()
    finish = jpegdec.finishing(r, tabs, T, h, w, layout, normalize, mean, std, out)
    launch_chains(blob, d_scans, d_chains, r.coef, info, T, h, w, layout)
    finish()
    host = info.cpu().numpy()
    for t in np.flatnonzero(host):
        raise ValueError('a corrupt entropy-coded segment (file %d): %s' % (t, '; '.join(v for b, v in STATUS.items() if host[t] & b)))
    r.chains, r.launches, r.readbacks = len(chains), 3, 1
    return r


def launch_chains(blob, d_scans, d_chains, coef, info, T, h, w, layout):
    """The chain launch alone (tools/jpegprog_bench.py times subsets of the chains with it): device tensors throughout."""
    hip.call('mg_jpegprog_chains', hip.ptr(blob), c_long(blob.numel()), hip.ptr(d_scans), c_long(d_scans.shape[0]), hip.ptr(d_chains),
             c_long(d_chains.shape[0]), hip.ptr(coef), c_long(coef.numel()), hip.ptr(info), c_long(T), c_int(h), c_int(w), c_int(layout), hip.stream())


def pack(plans, datas):
    """The host side of a clip: (file bytes joined, scan records, chain records with the longest chains first, quantisation tables)."""
    scans, chains, first = [], [], 0
    for t, (p, o) in enumerate(zip(plans, jpegdec.offsets_of(datas))):
        s, c = records(p, int(o), t, first)
        scans.append(s)
        chains.append(c)
        first += len(s)
    scans, chains = np.concatenate(scans), np.concatenate(chains)
    size = np.array([scans[a:a + n, 457].sum() for _, a, n, _ in chains])
    chains = chains[np.argsort(-size, kind='stable')]         # the waves that run longest start first
    return b''.join(bytes(d) for d in datas), scans, chains, np.stack([p.qtables for p in plans])


def run_files(datas, plans, device, **kw):
    """Progressive files of one geometry and their plans -> records and blob -> `run` (`kw`: its keywords)."""
    joined, scans, chains, qt = pack(plans, datas)
    h, w, layout = plans[0].geometry
    return run(jpegdec.blob_of([joined], device), scans, chains, qt, h, w, layout, **kw)


def _clip(datas, normalize, mean, std, device, out=None, plans=None):
    jpegdec.datas_of(datas)
    float3(mean), float3(std)
    plans = [parse(d) for d in datas] if plans is None else plans
    jpegdec.one_geometry(plans)
    return run_files(datas, plans, device, normalize=normalize, mean=mean, std=std, out=out)


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
    return jpegdec.run_files(datas, plans, device, normalize=normalize, mean=mean, std=std, out=out)


def load_routes(datas, routes, one_layout, normalize, mean, std, device):
    """`load_clip` here and in `jpegsamp`. `routes`: [(parse, run)] -- a file goes to the first whose `parse` accepts it (if none does, the
    `Unsupported` of the first propagates), and `run(files, plans, normalize, mean, std, device, out)` decodes a group of files of one route,
    kind and layout into its slice of the result. `one_layout`: the files share size AND layout and the groups run in the order of the routes;
    else they share the size and the groups run in the order in which their first files come. `device`: a function, called once parsing is done."""
    jpegdec.datas_of(datas)
    float3(mean), float3(std)

    def first_route(d):
        for which, (accepts, _) in enumerate(routes):
            try:
                return which, accepts(d)
            except Unsupported as e:
                refusal = e if which == 0 else refusal
        raise refusal from None
    found = [first_route(d) for d in datas]
    sizes = sorted({p.geometry[:2] for _, p in found})
    if one_layout:
        jpegdec.one_geometry([p for _, p in found])
    elif len(sizes) > 1:
        raise ValueError('the files of a clip must share one size (got %s)' % sizes)
    device = device()
    (h, w), T = sizes[0], len(datas)
    groups = {}
    for k, (which, p) in enumerate(found):
        groups.setdefault((which, p.kind, p.layout), []).append(k)
    keys = sorted(groups, key=(lambda g: g[0]) if one_layout else (lambda g: groups[g][0]))
    order = [k for key in keys for k in groups[key]]
    out = torch.empty((T, 3, h, w) if normalize else (T, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=device)
    at = 0
    for key in keys:
        ks = groups[key]
        routes[key[0]][1]([datas[k] for k in ks], [found[k][1] for k in ks], normalize, mean, std, device, out[at:at + len(ks)])
        at += len(ks)
    if order == list(range(T)):
        return out
    back = np.empty(T, np.int64)
    back[order] = np.arange(T)
    return out[torch.from_numpy(back).to(device)]


def load_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode_clip` for whatever a loader finds: each file goes the way of the parser that accepts it (`jpegdec.parse` first, then `parse`; if
    neither does, the `Unsupported` of `jpegdec.parse` propagates). The baseline files are decoded in one set of launches and the progressive
    files in another, into slices of one tensor; the result is in the order of `datas`."""
    routes = [(jpegdec.parse, lambda *a: _baseline(*a)),
              (parse, lambda files, plans, n, m, s, dev, out: _clip(files, n, m, s, dev, out=out, plans=plans))]
    return load_routes(datas, routes, True, normalize, mean, std, lambda: resolve_device(device))


def load(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode` for whatever a loader finds: a baseline file through `jpegdec`, a progressive one through this module."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return load_clip([data], normalize=normalize, mean=mean, std=std, device=device)[0]
