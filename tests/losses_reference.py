"""float64 reference, case construction and comparison for the matting-loss kernels of csrc/losses.hip (tests/test_gpu_losses.py on the
device, tests/test_losses_reference_cpu.py on the host). Plain torch on the CPU.

The losses are restated from the reference's statements (maggie/network/arch/maggie.py:237-262 regression_loss, maggie/network/loss.py:67-118
GradientLoss, :120-191 LapLoss with its 3-fold channel sum and its [::2, ::2] weight pyramid; `pred * valid` per plane as in
arch/maggie.py:112-118) on (P, H, W) planes, in whatever dtype they are given. Every gradient comes from autograd in float64: the
adjoints U^T and D^T owe nothing to csrc/loss_stencils.h.

Comparison, element-wise, with rows_reference.check():   |got - ref| <= U32 * k * S,   U32 = 2^-23,
S = the float64 sum of the absolute values of the terms that form the element (for a gradient: the reference backward run on absolute
values and absolute coefficients), k = fp32 operations on the longest path to the element (K_* below, each next to its count).

Sign decisions. G_l = w_l sign(L_l) and s = sign(mag_p - mag_t) may differ between fp32 and fp64 where the quantity is within rounding of zero.
The reference returns the magnitude of every such quantity and its band tau = U32 * k * S (the forward error bound of that quantity).
A cell is a TIE when every term that forms the quantity is zero (S == 0 for L; identical 3 x 3 windows for the Sobel pair): both precisions
give exactly 0 there. A cell is UNDECIDED when it is no tie and its magnitude is below tau. The sign of p * pv - t is exact in fp32 (the
rounded difference of two floats has the sign of the exact one): the L1 term has no band.
"""
import numpy as np
import torch
import torch.nn.functional as F

from rows_reference import MEASURED, U32, bits_of, check, close, error_ratio      # noqa: F401  (re-exported)

F64 = torch.float64
GOUT = (1.3, 0.7, 2.1)          # upstream gradients of (rec, lap, grad); rounded to fp32 before either side uses them

# ------------------------------------------------------------------------------------------------------------------
# k: fp32 operations on the longest path (an exact operation -- a product with 0, 1, 2, 4 or a power of two -- counts 0)
# ------------------------------------------------------------------------------------------------------------------
K_D = 1                  # d = p * pv - t: pv is 0 / 1, one subtraction, whose error is relative to |d| (S of d is |d|)
K_DOWN = 10              # row: product with g_j, 4 additions; column: product with g_i, 4 additions
K_UP = 6                 # at most 3 stuffed taps per axis: product, 2 additions, twice
K_LAPCELL = K_UP + 1     # L = x - 4 up (4 up is exact)
K_UPT = 18               # 5 rows + 2 pre-image rows: product, 7 additions, twice; times 4 c; the subtraction from `add`
K_DOWNT = 12             # at most 5 taps per axis (3 + pre-images): product, 4 additions, twice; c q; the addition
K_COEF = 3               # c_l = 3 g / (sum w_l + 1e-6): product, addition, division (c_rec, c_grad: 2)
K_MAG = 4                # mag = sqrt(gx^2 + gy^2 + eps) over S_MAG = (|gx| S_gx + |gy| S_gy) / mag + mag: gx 3 operations, the radicand 3 relative
                         # operations halved by the root, the root 2 -- 3 on the first term, 3.5 on the second, rounded up
K_MAGDIFF = K_MAG + 1    # mag_p - mag_t
K_A = 6                  # A = s gx / mag over S_A = S_gx / mag + |gx| S_MAG / mag^2: gx 3 + product and division 2 = 5 on the first, K_MAG on the second
K_ADJ = 32               # the Sobel adjoint at a corner: 4 neighbours x 4 clamped taps x 2 additions (18 away from the border)
K_POINT_BWD = K_A + K_ADJ + 1 + 2         # + times c_grad (w and 1/8 are exact) + the two additions of the three terms
# the Laplacian path to dpred: c_2 G_2 (K_COEF + 1) -> U^T -> D^T at level 2 -> `add` of level 1 (1) -> D^T -> `add` of level 0 (1) -> D^T -> 2 additions
K_DPRED = K_COEF + 1 + K_UPT + 3 * K_DOWNT + 2 + 2          # 62; the Sobel path is K_POINT_BWD + 2 = 43, the L1 path 5


def k_level(lvl):
    """k of L at pyramid level lvl of the end-to-end pipeline: its input went through K_D and lvl blur-decimations."""
    return K_D + (lvl + 1) * K_DOWN + K_LAPCELL              # 18, 28, 38


def sum_depth(cells, planes):
    """Additions on the longest path of a sum over `planes` planes of `cells` cells through the reducing launches of losses.hip:
    blocks = min(ceil(cells / 256), 256) workgroups per plane; a thread adds at most 4 cells per trip of ceil(cells / (256 blocks)) trips;
    6 butterfly steps in the wave; 4 waves; then either the ordered slots (16 chunks of ceil(n / 16) slots, each 4 interleaved running sums
    + 2, 16 chunk additions, 1 into the accumulator) or the atomics (ceil(n / 32) per replica, min(n, 32) replicas), n = blocks * planes.
    The tail is sequential, so the depth follows the launch geometry and not ceil(log2 n) alone."""
    blocks = min(-(-cells // 256), 256)
    per_thread = 4 * -(-cells // (256 * blocks))
    n = blocks * planes
    slots = -(-(-(-n // 16)) // 4) + 2 + 16 + 1
    atomics = -(-n // 32) + min(n, 32)
    return per_thread + 6 + 4 + max(slots, atomics)


# ------------------------------------------------------------------------------------------------------------------
# the single operators, on (P, h, w) planes
# ------------------------------------------------------------------------------------------------------------------
def _gauss(dtype):
    g = torch.tensor([1., 4., 6., 4., 1.], dtype=dtype)
    return (g[:, None] * g[None, :]) / 256.


def conv_gauss(x, scale=1.0):
    """gauss5 with reflect padding (loss.py:143-146)."""
    k = (_gauss(x.dtype) * scale)[None, None]
    return F.conv2d(F.pad(x[:, None], (2, 2, 2, 2), mode='reflect'), k)[:, 0]


def D(x):
    """blur, then decimate (loss.py:131-132, 152-153)."""
    return conv_gauss(x)[:, ::2, ::2]


def U(x):
    """zero-stuff, then 4 x gauss5 (loss.py:134-141)."""
    P, h, w = x.shape
    up = x.new_zeros((P, 2 * h, 2 * w))
    up[:, ::2, ::2] = x
    return conv_gauss(up, 4.0)


def adjoint(op, q, in_shape):
    """op^T q = d <op(x), q> / dx."""
    x = torch.zeros(in_shape, dtype=q.dtype, requires_grad=True)
    return torch.autograd.grad((op(x) * q).sum(), x)[0]


def UT(q):
    P, h, w = q.shape
    return adjoint(U, q, (P, h // 2, w // 2))


def DT(r):
    P, hd, wd = r.shape
    return adjoint(D, r, (P, 2 * hd, 2 * wd))


KX = ((-1., 0., 1.), (-2., 0., 2.), (-1., 0., 1.))


def sobel_xy(v, kx=None, absolute=False):
    """(gx, gy) of the replicate-padded Sobel pair, kernel / 8 (loss.py:90-118)."""
    kx = torch.tensor(KX, dtype=v.dtype) if kx is None else kx
    ky = kx.t().contiguous()
    if absolute:
        kx, ky = kx.abs(), ky.abs()
    vp = F.pad(v[:, None], (1, 1, 1, 1), mode='replicate')
    return F.conv2d(vp, kx[None, None] / 8)[:, 0], F.conv2d(vp, ky[None, None] / 8)[:, 0]


def sobel_adjoint(A, B, kx=None, absolute=False):
    """d (<gx(v), A> + <gy(v), B>) / dv."""
    v = torch.zeros_like(A, requires_grad=True)
    gx, gy = sobel_xy(v, kx, absolute)
    return torch.autograd.grad((gx * A).sum() + (gy * B).sum(), v)[0]


# ------------------------------------------------------------------------------------------------------------------
# the three losses, restated (any float dtype)
# ------------------------------------------------------------------------------------------------------------------
def regression_loss(p, t, w):
    return (p * w - t * w).abs().sum() / (w.sum() + 1e-8)


def laplacian_pyramid(x, levels=3):
    pyr = []
    for _ in range(levels):
        down = D(x)
        pyr.append(x - U(down))
        x = down
    return pyr


def lap_loss(p, t, w, levels=3):
    pp, pt = laplacian_pyramid(p, levels), laplacian_pyramid(t, levels)
    total = 0
    for i in range(levels):
        total = total + ((pp[i] - pt[i]).abs() * w).sum() / (w.sum() + 1e-6)
        w = w[:, ::2, ::2]
    return 3 * total                         # LapLoss(channels=3) on a 1-channel plane: three identical channels against one weight


def sobel_mag(v, eps=1e-6):
    gx, gy = sobel_xy(v)
    return torch.sqrt(gx * gx + gy * gy + eps)


def grad_loss(p, t, w, eps=1e-6):
    return (sobel_mag(p * w, eps) - sobel_mag(t * w, eps)).abs().sum() / (w.sum() + eps)


def restated(pred, target, weight, pvalid=None, dtype=F64):
    """-> (rec, lap, grad) as one tensor with an autograd graph, and the leaf `pred` it hangs on."""
    p = pred.to(dtype).clone().requires_grad_(True)
    t, w = target.to(dtype), weight.to(dtype)
    pe = p if pvalid is None else p * pvalid.to(dtype)[:, None, None]
    return torch.stack([regression_loss(pe, t, w), lap_loss(pe, t, w), grad_loss(pe, t, w)]), p


# ------------------------------------------------------------------------------------------------------------------
# the float64 reference of one scale with everything the comparison needs
# ------------------------------------------------------------------------------------------------------------------
def lap_grad(G, c, absolute=False):
    """d/dx_0 of sum_l c_l <L_l(x), G_l> through autograd of D and U; absolute: every operator and coefficient by absolute value (I + U D)."""
    x = torch.zeros_like(G[0], requires_grad=True)
    cur, total = x, 0
    for l in range(len(G)):
        down = D(cur)
        L = cur + U(down) if absolute else cur - U(down)
        total = total + (abs(c[l]) if absolute else c[l]) * (L * (G[l].abs() if absolute else G[l])).sum()
        cur = down
    return torch.autograd.grad(total, x)[0]


def sobel_terms(v):
    """gx, gy, mag and their S for v = a * w."""
    gx, gy = sobel_xy(v)
    sx, sy = sobel_xy(v.abs(), absolute=True)
    mag = torch.sqrt(gx * gx + gy * gy + 1e-6)
    return gx, gy, mag, sx, sy, (gx.abs() * sx + gy.abs() * sy) / mag + mag


def window_max(x):
    return F.max_pool2d(F.pad(x[:, None], (1, 1, 1, 1), mode='replicate'), 3, stride=1)[:, 0]


def reference(pred, target, weight, pvalid=None, gout=GOUT):
    """One scale in float64. pred / target / weight: (P, H, W) fp32 tensors as the kernels get them, pvalid: (P,) 0 / 1 or None.
    -> dict: values (3,), S_values, k_values (for the given plane count), grad, S_grad, the gradient's three terms, the pyramid (L, S_L, wl, G,
    tie, undecided per level), the Sobel pair (diff, tau, tie, undecided) and the coefficients."""
    p, t, w = pred.double(), target.double(), weight.double()
    P, H, W = p.shape
    pv = torch.ones(P, dtype=F64) if pvalid is None else pvalid.double()
    pv3 = pv[:, None, None]
    g = torch.tensor(gout, dtype=torch.float32).double()
    vals, leaf = restated(pred, target, weight, None if pvalid is None else pvalid, F64)
    grad = torch.autograd.grad((vals * g).sum(), leaf)[0]
    pe = p * pv3
    out = {'values': vals.detach(), 'grad': grad, 'pv': pv}

    # L1
    d = pe - t
    s_d = d.abs()                   # the rounding error of a difference of two floats is relative to the difference itself
    sw = w.sum()
    c_rec, c_grad = g[0] / (sw + 1e-8), g[2] / (sw + 1e-6)
    g_l1 = c_rec * w * torch.sign(d) * pv3
    s_l1 = c_rec.abs() * w * (d != 0) * pv3

    # pyramid of d
    levels, x, s_x, wl, c = [], d, s_d, w, []
    for l in range(3):
        down, s_down = D(x), D(s_x)
        L, s_L = x - U(down), s_x + U(s_down)
        tau = U32 * k_level(l) * s_L
        tie = s_L == 0
        levels.append({'L': L, 'S': s_L, 'wl': wl, 'tau': tau, 'tie': tie, 'undecided': (~tie) & (L.abs() < tau) & (wl > 0),
                       'G': wl * torch.sign(L), 'x': x, 'down': down})
        c.append(3 * g[1] / (wl.sum() + 1e-6))
        x, s_x, wl = down, s_down, wl[:, ::2, ::2]
    G = [lv['G'] for lv in levels]
    g_lap = lap_grad(G, c) * pv3
    s_lap = lap_grad(G, c, absolute=True) * pv3

    # Sobel pair
    gxp, gyp, mp, sxp, syp, s_mp = sobel_terms(pe * w)
    _, _, mt, _, _, s_mt = sobel_terms(t * w)
    diff = mp - mt
    s_diff = s_mp + s_mt
    tau_s = U32 * K_MAGDIFF * s_diff
    tie_s = window_max((pe * w - t * w).abs()) == 0
    und_s = (~tie_s) & (diff.abs() < tau_s)
    s = torch.where(tie_s, torch.zeros_like(diff), torch.sign(diff))
    A, B = s * gxp / mp, s * gyp / mp
    s_A = s.abs() * (sxp / mp + gxp.abs() * s_mp / mp ** 2)
    s_B = s.abs() * (syp / mp + gyp.abs() * s_mp / mp ** 2)
    g_sob = c_grad * w * sobel_adjoint(A, B) * pv3
    s_sob = c_grad.abs() * w * sobel_adjoint(s_A, s_B, absolute=True) * pv3

    out.update(g_l1=g_l1, g_lap=g_lap, g_sob=g_sob, S_grad=s_l1 + s_lap + s_sob, levels=levels, coef=(c_rec, c_grad, c[0], c[1], c[2]),
               sobel={'diff': diff, 'S': s_diff, 'tau': tau_s, 'tie': tie_s, 'undecided': und_s, 'A': A, 'B': B}, d=d, S_d=s_d)

    # S and k of the three values
    live = int((w.reshape(P, -1).sum(1) > 0).sum())           # planes without weight add nothing to any sum
    depth = [sum_depth((H >> l) * (W >> l), max(live, 1)) for l in range(3)]
    s_rec = (w * s_d).sum() / (sw + 1e-8)
    s_lapv = 3 * sum((lv['wl'] * lv['S']).sum() / (lv['wl'].sum() + 1e-6) for lv in levels)
    live_w = (w.reshape(P, -1).sum(1) > 0).double()[:, None, None]
    s_gradv = (s_diff * live_w).sum() / (sw + 1e-6)
    out['S_values'] = torch.stack([s_rec, s_lapv, s_gradv])
    out['k_values'] = (K_D + 1 + depth[0] + 2,                                 # w |d|; the sum; + 1e-8, the division
                       max(k_level(l) + 1 + depth[l] for l in range(3)) + 5,   # |L| w; the sum; + 1e-6, the division, 2 additions, times 3
                       K_MAGDIFF + depth[0] + 2)
    return out


def sobel_keep(ref, weight):
    """Mask of the gradient elements that stay in the comparison of the large case: everything but the 3 x 3 neighbourhood of an undecided
    Sobel cell; and the fraction of the weighted cells that is left out."""
    drop = window_max(ref['sobel']['undecided'].double()) > 0
    weighted = weight.double() > 0
    frac = float((drop & weighted).sum()) / max(1, int(weighted.sum()))
    return ~drop, frac


# ------------------------------------------------------------------------------------------------------------------
# references of the single kernels: (value, S, k)
# ------------------------------------------------------------------------------------------------------------------
def ref_down(x):
    x = x.double()
    return D(x), D(x.abs()), K_DOWN


def ref_upT(q, coef, add=None):
    """r = add - coef * U^T q (U carries the factor 4)."""
    q, c = q.double(), float(coef)
    v, s = -c * UT(q), abs(c) * UT(q.abs())
    if add is not None:
        v, s = v + add.double(), s + add.double().abs()
    return v, s, K_UPT


def ref_downT(r, q, coef):
    """dd = coef * q + D^T r."""
    r, q, c = r.double(), q.double(), float(coef)
    return c * q + DT(r), (c * q).abs() + DT(r.abs()), K_DOWNT


def ref_lap_fwd(x, down, w0, lvl):
    """-> L, S_L, tau, wl, tie, undecided, (sum |L| wl, S, k without the sum's depth), sum wl."""
    x, down = x.double(), down.double()
    wl = w0.double()[:, ::1 << lvl, ::1 << lvl]
    L, s_L = x - U(down), x.abs() + U(down.abs())
    tau = U32 * K_LAPCELL * s_L
    tie = s_L == 0
    return {'L': L, 'S': s_L, 'tau': tau, 'wl': wl, 'tie': tie, 'undecided': (~tie) & (L.abs() < tau) & (wl > 0),
            'sum': (L.abs() * wl).sum(), 'S_sum': (s_L * wl).sum(), 'k_sum': K_LAPCELL + 1, 'sum_w': wl.sum()}


def ref_point_bwd(p, t, w, c_rec, c_grad, dd):
    """dp = c_rec w sign(p - t) + dd + c_grad w SobelAdjoint(A, B) by autograd -> value, S, k, and the Sobel decisions."""
    p, t, w = p.double(), t.double(), w.double()
    leaf = p.clone().requires_grad_(True)
    f = float(c_rec) * (w * (leaf - t).abs()).sum() + float(c_grad) * (sobel_mag(leaf * w) - sobel_mag(t * w)).abs().sum()
    if dd is not None:
        f = f + (dd.double() * leaf).sum()
    val = torch.autograd.grad(f, leaf)[0]
    gxp, gyp, mp, sxp, syp, s_mp = sobel_terms(p * w)
    _, _, mt, _, _, s_mt = sobel_terms(t * w)
    diff, s_diff = mp - mt, s_mp + s_mt
    tie = window_max((p * w - t * w).abs()) == 0
    und = (~tie) & (diff.abs() < U32 * K_MAGDIFF * s_diff)
    s = torch.where(tie, torch.zeros_like(diff), torch.sign(diff)).abs()
    s_A, s_B = s * (sxp / mp + gxp.abs() * s_mp / mp ** 2), s * (syp / mp + gyp.abs() * s_mp / mp ** 2)
    S = abs(float(c_rec)) * w * (p != t) + abs(float(c_grad)) * w * sobel_adjoint(s_A, s_B, absolute=True)
    if dd is not None:
        S = S + dd.double().abs()
    return val, S, K_POINT_BWD, {'undecided': und, 'tie': tie}


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
TIE = 12                 # side of the pred == target block (top left corner of plane 0, non-zero weight)
ZERO_H, ZERO_W = 4, 12   # the zero-weight block (bottom right corner of plane 0)
SMALL = [(16, 16, 1, 3), (16, 24, 1, 3), (24, 16, 1, 3), (32, 32, 2, 2), (24, 40, 1, 4), (40, 40, 1, 3)]
LARGE = (264, 256, 1, 2)            # 67 584 cells per plane: one full trip of the 256-workgroup reducing grid and a partial second one
# seeds chosen on the host (test_losses_reference_cpu.py proves the condition of each): the first seed from 0 up whose three scales, with and
# without pvalid, have no undecided cell (small cases) / leave out at most 1 % of the weighted cells (large case). The seeds passed over hold
# Sobel near-ties (8-bit windows whose (gx, gy) pairs differ but whose magnitudes coincide): one or two cells at 24 x 40 and 40 x 40.
SEEDS = {(16, 16): 0, (16, 24): 0, (24, 16): 0, (32, 32): 0, (24, 40): 4, (40, 40): 20, (264, 256): 0}
MAX_LEFT_OUT = 0.01


def case_id(c):
    return '%dx%d' % (c[0], c[1])


def make_case(H, W, N, slots, seed=None, scales=3):
    """-> dict: preds [S] / target / weights [S] as (N, slots, H, W) fp32 tensors, pvalid (P,) int32, P.
    8-bit planes (k / 255); weights in {0, 1, 2}; plane 0 carries the tie block (pred == target bit for bit in every scale, weight 1 or 2)
    and the zero-weight block; plane 1 has no weight in scale 0 (and in a single-scale run), plane P - 1 none in scale 1; pvalid masks plane P - 1."""
    seed = SEEDS[(H, W)] if seed is None else seed
    rs = np.random.RandomState(1000 * H + W + 7919 * seed)
    P = N * slots
    q = lambda: torch.from_numpy((rs.randint(0, 256, size=(P, H, W)) / 255.0).astype(np.float32))      # noqa: E731
    target = q()
    preds, weights = [], []
    for s in range(scales):
        p = q()
        w = torch.from_numpy(rs.randint(0, 3, size=(P, H, W)).astype(np.float32))
        p[0, :TIE, :TIE] = target[0, :TIE, :TIE]
        w[0, :TIE, :TIE] = torch.from_numpy(rs.randint(1, 3, size=(TIE, TIE)).astype(np.float32))
        w[0, H - ZERO_H:, W - ZERO_W:] = 0
        if s == 0:
            w[1] = 0
        if s == 1:
            w[P - 1] = 0
        preds.append(p.reshape(N, slots, H, W))
        weights.append(w.reshape(N, slots, H, W))
    pvalid = torch.ones(P, dtype=torch.int32)
    pvalid[P - 1] = 0
    return {'preds': preds, 'target': target.reshape(N, slots, H, W), 'weights': weights, 'pvalid': pvalid, 'P': P, 'H': H, 'W': W}


def planes(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1])


def case_references(case, with_valid):
    """The float64 reference of every scale of a case."""
    pv = case['pvalid'] if with_valid else None
    return [reference(planes(p), planes(case['target']), planes(w), pv) for p, w in zip(case['preds'], case['weights'])]


def seed_condition(case, small):
    """What a seed must meet, on the reference alone -> (ok, detail)."""
    worst = 0.0
    for with_valid in (False, True):
        for ref, w in zip(case_references(case, with_valid), case['weights']):
            if small:
                n = sum(int(lv['undecided'].sum()) for lv in ref['levels']) + int(ref['sobel']['undecided'].sum())
                if n:
                    return False, '%d undecided cells' % n
            else:
                worst = max(worst, sobel_keep(ref, planes(w))[1])
    return worst <= MAX_LEFT_OUT, 'left out %.4f' % worst


def random_planes(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).float()
