"""JPEG files of the other chroma samplings decoded on the device -- 4:2:2 (cameras), 4:4:0 (the same pictures rotated losslessly) and 4:1:1
(older video grabs), baseline and progressive: the files of the reference's `T.Load` (maggie/dataloader/transforms.py:38-66) that
`jpegdec.parse` and `jpegprog.parse` refuse for their sampling.

  * `parse`        the marker walk of `jpegdec` (SOF0) or `jpegprog` (SOF2), accepting luma sampling (2, 1), (1, 2) or (4, 1) over (1, 1) Cb and
                   Cr: a `JpegPlan` or `ProgPlan` with `kind` ('baseline' / 'progressive') and `geometry` == (h, w, L422 / L440 / L411). Raises
                   `jpegdec.Unsupported` by name for everything else, 4:2:0 / 4:4:4 / grey included (use jpegdec / jpegprog).
  * `decode` / `decode_clip` / `decode_stats`   the contracts, dtypes and shapes of their namesakes; a clip holds baseline OR progressive files.
  * `load` / `load_clip`   the one entry a loader calls for any JPEG file: `jpegdec.parse`, then `jpegprog.parse`, then `parse`; a mixed clip (one
                   size) runs one set of launches per (kind, layout) group into slices of one tensor.

The entropy kernels are those of `jpegdec` and `jpegprog`: they know blocks per MCU and the slot words, nothing else. What is new is the
geometry (an MCU of 8 hs x 8 vs pixels, hs * vs luma blocks then Cb then Cr: layouts 3 to 5 of include/maggie_hip.h) and `mg_jpeg_rgb_hv`,
which upsamples the chroma in registers in front of the colour conversion. Equal to Pillow byte for byte. One read-back per call in the usual
case (see `jpegdec`); not graph-capturable; wrong types raise before any launch; there is no CPU fallback."""
from . import jpegdec, jpegprog
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, resolve_device
from ._jpegfile import walk
from .jpegdec import L411, L422, L440, LUMA, Unsupported           # noqa: F401  (the layouts: for the callers of this module)

_ELSEWHERE = (((2, 2), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1)))


def _layout(sampling):
    if len(sampling) == 1 or sampling in _ELSEWHERE:
        raise Unsupported('sampling %s: use jpegdec / jpegprog for 4:2:0, 4:4:4 and greyscale files' % (sampling,))
    for layout, luma in LUMA.items():
        if sampling == (luma, (1, 1), (1, 1)):
            return layout
    raise Unsupported('sampling %s (only 4:2:2, 4:4:0 and 4:1:1 -- luma (2, 1), (1, 2), (4, 1) over (1, 1) chroma -- are decoded)' % (sampling,))


def parse(data):
    """The marker walk of one file's bytes -> `jpegdec.JpegPlan` (SOF0) or `jpegprog.ProgPlan` (SOF2) with `layout` L422, L440 or L411. Host
    only; raises `Unsupported` by name for what this module does not decode: every other sampling, and everything `jpegdec.parse` /
    `jpegprog.parse` refuse."""
    kinds = {0xC0: jpegdec.rules(_layout), 0xC2: jpegprog.rules(_layout)}
    try:
        f = walk(data, None, lambda f: kinds[f.frame['sof']][0](f), lambda f, scan: kinds[f.frame['sof']][1](f, scan))
    except Unsupported as e:
        if not e.before_frame:
            raise
        return jpegdec._parse(data, _layout)                   # neither frame header, or a defect in front of it: the baseline walk names it
    return kinds[f.frame['sof']][2](f)


def planes_layout(h, w, layout):
    """(luma rows, luma pitch, chroma rows, chroma pitch) of a frame's planes (`Decoded.planes`: Y of all frames, then Cb, then Cr)."""
    return jpegdec.geometry(h, w, layout)[2:]


def _run(datas, plans, normalize, mean, std, device, sub_bytes, out):
    """One set of launches for files of one kind and one geometry."""
    if plans[0].kind == 'baseline':
        return jpegdec.run_files(datas, plans, device, sub_bytes=sub_bytes, normalize=normalize, mean=mean, std=std, out=out)
    return jpegprog.run_files(datas, plans, device, normalize=normalize, mean=mean, std=std, out=out)


def _clip(datas, normalize, mean, std, device, sub_bytes, out=None):
    jpegdec.datas_of(datas)
    jpegdec._sub_bytes(sub_bytes)
    float3(mean), float3(std)
    plans = [parse(d) for d in datas]
    jpegdec.one_geometry(plans)
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


def load_clip(datas, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode_clip` for whatever a loader finds: each file goes to the first parser that accepts it (`jpegdec.parse`, `jpegprog.parse`, `parse`;
    if none does, the `Unsupported` of `jpegdec.parse` propagates). The files share one size; each group of one kind (baseline / progressive) and
    one layout is decoded in one set of launches into a slice of one tensor, and the result is in the order of `datas`. Not graph-capturable; one
    read-back per group in the usual case."""
    routes = [(jpegdec.parse, lambda *a: jpegprog._baseline(*a)),
              (jpegprog.parse, lambda files, plans, n, m, s, dev, out: jpegprog._clip(files, n, m, s, dev, out=out, plans=plans)),
              (parse, lambda files, plans, n, m, s, dev, out: _run(files, plans, n, m, s, dev, None, out))]
    return jpegprog.load_routes(datas, routes, False, normalize, mean, std, lambda: resolve_device(device))


def load(data, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """`decode` for whatever a loader finds: any baseline or progressive file of the six layouts."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('data must be the bytes of a JPEG file (got %s)' % type(data).__name__)
    return load_clip([data], normalize=normalize, mean=mean, std=std, device=device)[0]
