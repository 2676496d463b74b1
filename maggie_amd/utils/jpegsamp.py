"""JPEG files of the other chroma samplings decoded on the device -- 4:2:2 (cameras), 4:4:0 (the same pictures rotated losslessly) and 4:1:1
(older video grabs), baseline and progressive: the files of the reference's `T.Load` (maggie/dataloader/transforms.py:38-66) that
`jpegdec.parse` and `jpegprog.parse` refuse for their sampling.

  * `parse`        the marker walk of `jpegdec` (SOF0) or `jpegprog` (SOF2), accepting luma sampling (2, 1), (1, 2) or (4, 1) over (1, 1) Cb and
                   Cr: a plan with `kind` ('baseline' / 'progressive'), `geometry` == (h, w, L422 / L440 / L411) and everything `JpegPlan` /
                   `ProgPlan` carry. Raises `jpegdec.Unsupported` by name for everything else, 4:2:0 / 4:4:4 / grey included (use jpegdec / jpegprog).
  * `decode` / `decode_clip` / `decode_stats`   the contracts, dtypes and shapes of their namesakes; a clip holds baseline OR progressive files.
  * `load` / `load_clip`   the one entry a loader calls for any JPEG file: `jpegdec.parse`, then `jpegprog.parse`, then `parse`; a mixed clip (one
                   size) runs one set of launches per (kind, layout) group into slices of one tensor.

The entropy kernels are those of `jpegdec` and `jpegprog`: they know blocks per MCU and the slot words, nothing else. What is new is the
geometry (an MCU of 8 hs x 8 vs pixels, hs * vs luma blocks then Cb then Cr: the `_hv` entries of include/maggie_hip.h) and `mg_jpeg_rgb_hv`,
which upsamples the chroma in registers in front of the colour conversion. Equal to Pillow byte for byte. One read-back per call in the usual
case (see `jpegdec`); not graph-capturable; wrong types raise before any launch; there is no CPU fallback."""
import numpy as np
import torch

from . import jpegdec, jpegprog
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, resolve_device
from .jpegdec import MAX_BYTES, Unsupported

L422, L440, L411 = 3, 4, 5                                  # distinct from jpegdec.L420 / L444 / GREY; never passed to a C entry
LUMA = {L422: (2, 1), L440: (1, 2), L411: (4, 1)}           # the (hs, vs) the `_hv` entries take
BLOCKS_PER_MCU = {L422: 4, L440: 4, L411: 6}
_ELSEWHERE = (((2, 2), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1)))


class SampPlan(jpegdec.JpegPlan):
    """`jpegdec.JpegPlan` of a baseline file with `layout` L422, L440 or L411."""
    kind = 'baseline'

    @property
    def mcus(self):
        hs, vs = LUMA[self.layout]
        return -(-self.width // (8 * hs)) * -(-self.height // (8 * vs))


class SampProgPlan(jpegprog.ProgPlan):
    """`jpegprog.ProgPlan` of a progressive file with `layout` L422, L440 or L411."""
    kind = 'progressive'


def _layout(sampling):
    if len(sampling) == 1 or sampling in _ELSEWHERE:
        raise Unsupported('sampling %s: use jpegdec / jpegprog for 4:2:0, 4:4:4 and greyscale files' % (sampling,))
    for layout, luma in LUMA.items():
        if sampling == (luma, (1, 1), (1, 1)):
            return layout
    raise Unsupported('sampling %s (only 4:2:2, 4:4:0 and 4:1:1 -- luma (2, 1), (1, 2), (4, 1) over (1, 1) chroma -- are decoded)' % (sampling,))


def _progressive(d):
    """Whether the frame header of a file is SOF2 (anything irregular: False, and the baseline walk names it)."""
    p, n = 2, len(d)
    while p + 4 <= n and d[p] == 0xFF:
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xDA or (0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            return m == 0xC2
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
    return False


def parse(data):
    """The marker walk of one file's bytes -> SampPlan (SOF0) or SampProgPlan (SOF2). Host only; raises `Unsupported` by name for what this
    module does not decode: every other sampling, and everything `jpegdec.parse` / `jpegprog.parse` refuse."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    d = bytes(data)
    if _progressive(d):
        return SampProgPlan(**jpegprog._parse(d, _layout).__dict__)
    return SampPlan(**jpegdec._parse(d, _layout).__dict__)


def planes_layout(h, w, layout):
    """(luma rows, luma pitch, chroma rows, chroma pitch) of a frame's planes (`Decoded.planes`: Y of all frames, then Cb, then Cr)."""
    return jpegdec.hv_geometry(h, w, *LUMA[layout])[2:]


def _run(datas, plans, normalize, mean, std, device, sub_bytes, out):
    """One set of launches for files of one kind and one geometry."""
    h, w, layout = plans[0].geometry
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
    if offsets[-1] > MAX_BYTES:
        raise Unsupported('%d bytes of files in one clip' % offsets[-1])
    if plans[0].kind == 'baseline':
        recs = np.stack([jpegdec.record(p, int(o)) for p, o in zip(plans, offsets[:-1])])
        blob = torch.frombuffer(bytearray(b''.join(bytes(d) for d in datas)), dtype=torch.uint8).to(device, non_blocking=True)
        return jpegdec.run(blob, recs, h, w, layout, sub_bytes=sub_bytes, normalize=normalize, mean=mean, std=std, out=out, hv=LUMA[layout])
    joined, scans, chains, qt = jpegprog.pack(plans, datas)
    blob = torch.frombuffer(bytearray(joined), dtype=torch.uint8).to(device, non_blocking=True)
    return jpegprog.run(blob, scans, chains, qt, h, w, layout, normalize=normalize, mean=mean, std=std, out=out, hv=LUMA[layout])


def _clip(datas, normalize, mean, std, device, sub_bytes, out=None):
    jpegprog._datas(datas)
    jpegdec._sub_bytes(sub_bytes)
    float3(mean), float3(std)
    plans = [parse(d) for d in datas]
    if any(p.geometry != plans[0].geometry for p in plans):
        raise ValueError('the files of a clip must share one size and one sampling layout (got %s)' % sorted({p.geometry for p in plans}))
    if any(p.kind != plans[0].kind for p in plans):
        raise ValueError('the files of a clip must be all baseline or all progressive (load_clip takes mixed lists)')
    return _run(datas, plans, normalize, mean, std, resolve_device(device), sub_bytes, out)


def decode_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """T baseline or T progressive files (a sequence of bytes objects) of one size and one of the three layouts -> uint8 (T, h, w, 3) on the
    device, or with `normalize` fp32 (T, 3, h, w), from one set of launches; tables, restart intervals and scan scripts are per file. `out`: a
    preallocated contiguous destination. Files of differing geometry raise ValueError, unsupported ones `Unsupported`, corrupt entropy coding
    ValueError. Not graph-capturable."""
    return _clip(datas, normalize, mean, std, device, None, out).out


def decode(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """The bytes of one file -> uint8 (h, w, 3) on the device: `np.asarray(Image.open(BytesIO(data)).convert("RGB"))`. With `normalize` fp32
    (3, h, w): ToTensor + Normalize of that, the bits of `normalize_frames`. Not graph-capturable; one read-back in the usual case."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return _clip([data], normalize, mean, std, device, None, out).out[0]


def decode_stats(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None, sub_bytes=None):
    """`decode_clip` returning the whole `Decoded` record of `jpegdec` or `jpegprog` (coefficients, planes -- see `planes_layout` -- and the
    counts of launches and read-backs). `sub_bytes`: the subsequence length of baseline files. For tests and tools/jpegsamp_bench.py."""
    return _clip(datas, normalize, mean, std, device, sub_bytes, out)


def _first_parser(d):
    try:
        return 0, jpegdec.parse(d)
    except Unsupported as e:
        for k, f in ((1, jpegprog.parse), (2, parse)):
            try:
                return k, f(d)
            except Unsupported:
                pass
        raise e from None


def load_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode_clip` for whatever a loader finds: each file goes to the first parser that accepts it (`jpegdec.parse`, `jpegprog.parse`, `parse`;
    if none does, the `Unsupported` of `jpegdec.parse` propagates). The files share one size; each group of one kind (baseline / progressive) and
    one layout is decoded in one set of launches into a slice of one tensor, and the result is in the order of `datas`. Not graph-capturable; one
    read-back per group in the usual case."""
    jpegprog._datas(datas)
    float3(mean), float3(std)
    found = [_first_parser(d) for d in datas]
    sizes = sorted({p.geometry[:2] for _, p in found})
    if len(sizes) > 1:
        raise ValueError('the files of a clip must share one size (got %s)' % sizes)
    device = resolve_device(device)
    (h, w), T = sizes[0], len(datas)
    groups = {}
    for k, (which, p) in enumerate(found):
        groups.setdefault((which, getattr(p, 'kind', None), p.layout), []).append(k)
    order = [k for key in sorted(groups, key=lambda g: groups[g][0]) for k in groups[key]]
    out = torch.empty((T, 3, h, w) if normalize else (T, h, w, 3), dtype=torch.float32 if normalize else torch.uint8, device=device)
    at = 0
    for key in sorted(groups, key=lambda g: groups[g][0]):
        ks = groups[key]
        files, plans, dst = [datas[k] for k in ks], [found[k][1] for k in ks], out[at:at + len(ks)]
        if key[0] == 0:
            jpegprog._baseline(files, plans, normalize, mean, std, device, dst)
        elif key[0] == 1:
            jpegprog._clip(files, normalize, mean, std, device, out=dst, plans=plans)
        else:
            _run(files, plans, normalize, mean, std, device, None, dst)
        at += len(ks)
    if order == list(range(T)):
        return out
    back = np.empty(T, np.int64)
    back[order] = np.arange(T)
    return out[torch.from_numpy(back).to(device)]


def load(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode` for whatever a loader finds: any baseline or progressive file of the six layouts."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return load_clip([data], normalize=normalize, mean=mean, std=std, device=device)[0]
