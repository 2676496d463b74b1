"""A NumPy statement of the device matte refinement (maggie_amd/csrc/refine.hip): the byte-for-byte oracle of the kernels
and of `maggie_amd.utils.refine`. The fast guided filter (He & Sun) stated on bytes: window sums as int64 from a cumulative sum over the reflected,
padded plane (exact, so the order of adding cannot matter), then the fit, the fixed-point rounding, the second window, the bilinear step to full
size and the byte in float64, one NumPy operation per stated operation, in the stated order."""
import numpy as np

from cutout_restatement import alpha_byte, reflect, window_sums    # noqa: F401  (the window of section 35)

RADIUS, EPS = 5, 1e-4
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def solve3(s, k):
    """The cofactor solve of step 3: s = {(c, d): s_cd for c <= d} (eps already added), k = (k_0, k_1, k_2) -> (a_0, a_1, a_2)."""
    s00, s01, s02, s11, s12, s22 = (s[q] for q in PAIRS)
    c00 = s11 * s22 - s12 * s12
    c01 = s02 * s12 - s01 * s22
    c02 = s01 * s12 - s02 * s11
    c11 = s00 * s22 - s02 * s02
    c12 = s01 * s02 - s00 * s12
    c22 = s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    a0 = ((c00 * k[0] + c01 * k[1]) + c02 * k[2]) / det
    a1 = ((c01 * k[0] + c11 * k[1]) + c12 * k[2]) / det
    a2 = ((c02 * k[0] + c12 * k[1]) + c22 * k[2]) / det
    return a0, a1, a2


def coefficients(G, p, r=RADIUS, eps=EPS):
    """Steps 1-3: G uint8 (h, w, 3), p uint8 (h, w) -> (A int64 (3, h, w), B int64 (h, w), the largest unclipped |a|)."""
    n = float(r * r)
    g = [G[..., c].astype(np.int64) for c in range(3)]
    p64 = p.astype(np.int64)
    SI = [window_sums(g[c], r) for c in range(3)]
    SII = {q: window_sums(g[q[0]] * g[q[1]], r) for q in PAIRS}
    Sp = window_sums(p64, r)
    SIp = [window_sums(g[c] * p64, r) for c in range(3)]
    assert max(int(v.max()) for v in SI + list(SII.values()) + [Sp] + SIp) < 2 ** 32
    m = [SI[c].astype(np.float64) / (255.0 * n) for c in range(3)]
    mp = Sp.astype(np.float64) / (255.0 * n)
    s = {}
    for c, d in PAIRS:
        t = m[c] * m[d]
        s[(c, d)] = SII[(c, d)].astype(np.float64) / (65025.0 * n) - t
    for c in range(3):
        s[(c, c)] = s[(c, c)] + eps
    k = []
    for c in range(3):
        t = m[c] * mp
        k.append(SIp[c].astype(np.float64) / (65025.0 * n) - t)
    a = solve3(s, k)
    b = mp - ((a[0] * m[0] + a[1] * m[1]) + a[2] * m[2])
    A = np.stack([np.floor(np.clip(v, -256.0, 256.0) * 65536.0 + 0.5).astype(np.int64) for v in a])
    B = np.floor(np.clip(b, -1024.0, 1024.0) * 65536.0 + 0.5).astype(np.int64)
    return A, B, float(max(np.abs(v).max() for v in a))


def means(A, B, r=RADIUS):
    """Step 4: -> float64 (4, h, w) = (abar_0, abar_1, abar_2, bbar)."""
    n = float(r * r)
    out = []
    for v in list(A) + [B]:
        S = window_sums(v, r)
        assert np.abs(S).max() < 2 ** 39
        out.append(S.astype(np.float64) / (n * 65536.0))
    return np.stack(out)


def axis(src, dst):
    """Step 5 along one axis: dst outputs over src inputs -> (i0, i1, f)."""
    ratio = np.float64(src) / np.float64(dst)
    s = (np.arange(dst, dtype=np.float64) + 0.5) * ratio - 0.5
    s = np.clip(s, 0.0, float(src - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, s - i0


def up(v, ya, xa):
    y0, y1, fy = ya
    x0, x1, fx = xa
    fy = fy[:, None]
    top = v[y0][:, x0] * (1.0 - fx) + v[y0][:, x1] * fx
    bot = v[y1][:, x0] * (1.0 - fx) + v[y1][:, x1] * fx
    return top * (1.0 - fy) + bot * fy


def snapped(b):
    b = b.copy()
    b[b <= 1] = 0
    b[b >= 254] = 255
    return b


def apply(I, mean4, snap=False):
    """Step 5: I uint8 (H, W, 3), the four means (4, h, w) -> uint8 (H, W)."""
    H, W = I.shape[:2]
    h, w = mean4.shape[1:]
    ya, xa = axis(h, H), axis(w, W)
    i = [I[..., c].astype(np.float64) / 255.0 for c in range(3)]
    u = [up(mean4[q], ya, xa) for q in range(4)]
    q = ((u[3] + u[0] * i[0]) + u[1] * i[1]) + u[2] * i[2]
    out = np.floor(np.clip(q, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return snapped(out) if snap else out


def refine(I, G, p, r=RADIUS, eps=EPS, snap=False, with_max=False):
    """I uint8 (H, W, 3), G uint8 (h, w, 3), p (h, w) uint8 or float32 -> the refined alpha bytes (H, W) [, the largest unclipped |a|]."""
    A, B, amax = coefficients(G, alpha_byte(p), r, eps)
    out = apply(I, means(A, B, r), snap)
    return (out, amax) if with_max else out


def refine_all(frames, guides, alpha, r=RADIUS, eps=EPS, snap=False):
    """frames (T, H, W, 3), guides (T, h, w, 3), alpha (T, P, h, w) -> (T, P, H, W)."""
    H, W = frames.shape[1:3]
    return np.stack([np.stack([refine(frames[t], guides[t], alpha[t, p], r, eps, snap) for p in range(alpha.shape[1])]).reshape(-1, H, W)
                     for t in range(frames.shape[0])])


def bilinear_up(v, H, W):
    """`up` of a single plane (h, w) float64 to (H, W): the plain resize the refinement is measured against."""
    return up(v, axis(v.shape[0], H), axis(v.shape[1], W))


def scene(H=480, W=640, k=4):
    """The scene of the property check: a disc with hair-like strands over a gradient -> (I (H, W, 3), G, p at 1/k size, the true alpha byte)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.hypot(yy - 240.0, xx - 320.0)
    ang = np.arctan2(yy - 240.0, xx - 320.0)
    al = np.clip((150.0 + 25.0 * np.sin(37.0 * ang) - d) / 6.0 + 0.5, 0.0, 1.0)
    F = np.stack([200.0 + 30.0 * np.sin(xx / 7.0), 120.0 + 40.0 * np.cos(yy / 9.0), 60.0 + 20.0 * np.sin((xx + yy) / 5.0)], -1)
    B = np.stack([30.0 + 0.1 * xx, 60.0 + 0.2 * yy, 160.0 - 0.1 * xx], -1)
    noise = np.random.default_rng(0).normal(0, 2, (H, W, 3))
    I = np.clip(al[..., None] * F + (1.0 - al[..., None]) * B + noise, 0, 255).astype(np.uint8)
    G = np.round(I.astype(np.float64).reshape(H // k, k, W // k, k, 3).mean((1, 3))).astype(np.uint8)
    p = np.round((255.0 * al).reshape(H // k, k, W // k, k).mean((1, 3))).astype(np.uint8)
    return I, G, p, np.round(255.0 * al).astype(np.uint8)
