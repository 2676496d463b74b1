"""NumPy + scipy.ndimage restatement of the reference's Conn metric (maggie/utils/metric.py:224-300) and largest-component post-process
(maggie/utils/postprocessing.py:66-86), for the tests only -- the product never imports it.

Threshold semantics are those of the reference's own pin (numpy < 2): `gt >= thresh_steps[i]` compares the float32 plane with the float64
scalar IN FLOAT32 (value-based casting), i.e. against np.float32(np.arange(0, 1.1, 0.1)[i]). numpy 2 compares in float64 instead;
`float64_thresholds=True` restates that variant (the two differ only for pixels holding exactly np.float32(0.7000000000000001) or
np.float32(0.9), which round below their float64 thresholds). Per-pixel terms are float32 like the reference; sums are fp64.

The seeded inputs of tests/golden/conn_pinned.npz are regenerated here (`conn_inputs`, `postprocess_inputs`): the fixture stores seeds
and outputs only."""
import numpy as np

THRESH64 = np.arange(0, 1.1, 0.1)
THRESH32 = THRESH64.astype(np.float32)
# the two float32 values on which numpy 1 and numpy 2 threshold differently (float32(t) < t)
SPLIT_VALUES = (np.float32(THRESH64[7]), np.float32(THRESH64[9]))


def _ndimage():
    from scipy import ndimage
    return ndimage


def label(mask, connectivity=2):
    """skimage.measure.label(mask, connectivity, return_num=True) of one 2-D plane, through scipy.ndimage.label (same raster numbering)."""
    nd = _ndimage()
    st = nd.generate_binary_structure(2, 1) if connectivity == 1 else np.ones((3, 3), bool)
    lab, n = nd.label(np.asarray(mask) != 0, structure=st)
    return lab.astype(np.int32), int(n)


def largest(mask, connectivity):
    """[pixel in the largest component]; a tie goes to the lowest label (np.argmax: the first maximum); all False without foreground."""
    lab, n = label(mask, connectivity)
    if n == 0:
        return np.zeros(lab.shape, bool)
    return lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1


def conn_diff(pred, gt, trimap=None, float64_thresholds=False):
    """Per-plane conn_diff (metric.py:240-298, before * 0.001) of (..., H, W) float32 arrays; fp64 array of shape (P,)."""
    pred = np.asarray(pred, np.float32)
    gt = np.asarray(gt, np.float32)
    H, W = pred.shape[-2:]
    pred, gt = pred.reshape(-1, H, W), gt.reshape(-1, H, W)
    mask = np.ones_like(gt) if trimap is None else (np.asarray(trimap).reshape(-1, H, W) > 0).astype(np.float32)
    out = np.zeros(pred.shape[0], np.float64)
    for b in range(pred.shape[0]):
        rd = -np.ones((H, W), np.float32)
        for i in range(1, len(THRESH64)):
            t = THRESH64[i] if float64_thresholds else THRESH32[i]
            omega = largest((gt[b] >= t) & (pred[b] >= t), 1)
            rd[(rd == -1) & ~omega] = THRESH32[i - 1]
        rd[rd == -1] = 1
        gd, pd = gt[b] - rd, pred[b] - rd
        gphi = np.float32(1) - gd * (gd >= np.float32(0.15))
        pphi = np.float32(1) - pd * (pd >= np.float32(0.15))
        out[b] = (np.abs(gphi - pphi) * mask[b]).astype(np.float64).sum()
    return out


def conn_update(pred, gt, trimap=None):
    """(update() return, score, count) of one Conn.update on a fresh metric."""
    d = conn_diff(pred, gt, trimap)
    score, count = float(d.sum()) * 0.001, d.shape[0]
    return score / count, score, count


def postprocess(alpha, thresh=0.05):
    """alpha * [largest 8-connected component of alpha > thresh] per (H, W) plane; planes without foreground unchanged. float32."""
    a = np.asarray(alpha, np.float32)
    H, W = a.shape[-2:]
    planes = a.reshape(-1, H, W)
    out = np.empty_like(planes)
    for p in range(planes.shape[0]):
        fg = planes[p] > np.float32(thresh)
        lab, n = label(fg, 2)
        out[p] = planes[p] if n == 0 else planes[p] * (lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1)
    return out.reshape(a.shape)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def smooth_field(rs, shape, cell=16):
    """Smooth [0, 1] fields: a coarse uniform grid, bilinearly upsampled with plain float64 arithmetic (bit-identical everywhere), plus a little
    noise. The threshold intersections then have large twisted components, so the largest-component choice matters."""
    shape = tuple(shape)
    H, W = shape[-2:]
    gh, gw = H // cell + 2, W // cell + 2
    g = rs.rand(*(shape[:-2] + (gh, gw)))
    y = np.arange(H, dtype=np.float64) / cell
    x = np.arange(W, dtype=np.float64) / cell
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    a = g[..., y0[:, None], x0[None, :]]
    b = g[..., y0[:, None], x0[None, :] + 1]
    c = g[..., y0[:, None] + 1, x0[None, :]]
    d = g[..., y0[:, None] + 1, x0[None, :] + 1]
    f = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
    f = f * 1.3 - 0.15 + rs.normal(0, 0.02, size=shape)
    return np.clip(f, 0, 1).astype(np.float32)


def avoid_split_values(*arrays):
    """Moves any pixel holding one of SPLIT_VALUES one ulp up, so that numpy 1 and numpy 2 threshold the planes alike."""
    for a in arrays:
        for v in SPLIT_VALUES:
            a[a == v] = np.nextafter(v, np.float32(2))
    return arrays


# key: (shape, seed, kind, with_trimap)
CONN_CASES = {'random_tri': ((2, 3, 48, 40), 41, 'random', True), 'random_notri': ((1, 2, 33, 57), 42, 'random', False),
              'smooth_tri': ((3, 96, 128), 43, 'smooth', True), 'smooth_notri': ((2, 80, 100), 44, 'smooth', False),
              'clip': ((3, 2, 64, 72), 45, 'smooth', True)}


def conn_inputs(key, shape=None, seed=None):
    """(pred, gt, trimap or None) of a CONN_CASES entry (or of its kind at another shape / seed)."""
    shape0, seed0, kind, with_tri = CONN_CASES[key]
    shape, seed = shape or shape0, seed0 if seed is None else seed
    rs = np.random.RandomState(seed)
    if kind == 'random':
        pred = rs.rand(*shape).astype(np.float32)
        gt = np.clip(pred + rs.normal(0, 0.1, size=shape), 0, 1).astype(np.float32)
    else:
        pred = smooth_field(rs, shape)
        gt = np.clip(pred + smooth_field(rs, shape, cell=32) * 0.2 - 0.1, 0, 1).astype(np.float32)
    tri = rs.randint(0, 3, size=shape).astype(np.float32) if with_tri else None
    avoid_split_values(pred, gt)
    return pred, gt, tri


POSTPROCESS_SHAPE, POSTPROCESS_SEED = (2, 3, 70, 90), 46


def postprocess_inputs(shape=POSTPROCESS_SHAPE, seed=POSTPROCESS_SEED):
    """(B, N, H, W) alpha planes in [-0.05, 1.05]: smooth fields (negative values outside the kept component give -0.0), plane [0, 0] all
    <= 0.05 (returned unchanged, -0.0 included), plane [0, 1] holding two equal-size largest components (the raster-first one wins)."""
    rs = np.random.RandomState(seed)
    a = smooth_field(rs, shape, cell=12) * 1.1 - 0.05
    a = a.astype(np.float32)
    H, W = shape[-2:]
    bg = rs.uniform(-0.05, 0.05, size=(H, W)).astype(np.float32)
    bg[::7, ::5] = -0.0
    a[0, 0] = bg
    two = rs.uniform(-0.05, 0.04, size=(H, W)).astype(np.float32)
    two[10:15, 60:75] = rs.uniform(0.1, 1.0, size=(5, 15))           # 75 px, first pixel at row 10: the winner
    two[40:55, 50:55] = rs.uniform(0.1, 1.0, size=(15, 5))           # 75 px, first pixel at row 40
    two[2:4, 2:4] = 0.5                                              # a small third component
    a[0, 1] = two
    return a
