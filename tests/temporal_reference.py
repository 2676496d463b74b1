"""float64 references, sensitivities, case construction and operation counts for the video-side kernels of maggie_amd/csrc/temporal.hip and
temporal2.hip (tests/test_gpu_temporal.py on the device, tests/test_temporal_reference_cpu.py on the host). Plain torch / numpy on the CPU.

Every reference takes the operands as the kernel receives them (already rounded to the storage type for the ConvGRU kernels, fp32 for the rest),
works in `dt` (float64; the host proof also runs them in float32 with the sigmoid written the way the device forms it) and returns
{name: (value, S)}; S is None for an output that is compared with equality. The comparison is rows_reference.check:

    |got - ref| <= u_out |ref| + floor + U32 k S            element-wise

Rules for S (written before any device run):
  * S is the sum of the absolute values of the terms under every sum, carried through the chain;
  * every sigm(v) = 1 / (1 + __expf(-v)) multiplies the S of what it feeds by (1 + |v|): __expf forms exp2(v * log2 e) and the rounding of that
    product is a relative error |v| u32 / 2 of the result (rows_reference.sigmoid_mul);
  * a difference 1 - s or 1 - tc * tc enters S as 1 + s and 1 + tc * tc;
  * the recursions of the bidirectional fusion carry S frame by frame: the error a frame inherits is damped by the coefficient it is multiplied
    with (s or 1 - s), and every product and sum of the frame itself enters S with the rules above. The sum over the frames is therefore IN S and
    K_BIFUSE counts the operations of ONE frame step, not of the whole chain;
  * fp32 flush: a float64 sigmoid factor below 2^-126 may arrive as 0 (denormal flush of the reciprocal, or __expf overflowing to inf for
    v <= -89 so that 1 / (1 + inf) = 0). The lost quantity is factor * cofactor < 2^-126 |cofactor|, so elements whose factor is below 2^-126 get
    2^-126 |cofactor| / U32 added to S (_fl): an absolute term of k * 2^-126 |cofactor|, a property of the fp32 format, thirty orders of
    magnitude below any element that is not flushed. No other element gets a floor.

`fault=` plants a defect (the host proof shows that the comparison rejects each of them, the element-wise ones by 16 x k); None: the operation."""
import numpy as np
import torch
import torch.nn.functional as F

from rows_reference import U32, U_OUT, FLOOR, sum_k, K_SIGMUL, K_SIGMUL_BWD     # noqa: F401  (re-exported for the two test files)

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
LOG2E = 1.4426950408889634
TINY = 2.0 ** -126
GRID = 4096 * 256                # work items of one pass of a capped 4096-block grid
MAXT = 16


def sig(v, dt=F64):
    """float64: the sigmoid itself; float32: the device's form 1 / (1 + exp2(-v * log2 e))."""
    if dt == F64:
        return torch.sigmoid(v)
    return 1 / (1 + torch.exp2(-v * LOG2E))


def _fl(factor, cof):
    """The fp32 flush term of S (module docstring): 2^-126 |cof| / U32 where |factor| < 2^-126."""
    z = cof.abs() * (TINY / U32)
    return torch.where(factor.abs() < TINY, z, torch.zeros((), dtype=z.dtype))


# ------------------------------------------------------------------------------------------------------------------
# ConvGRU gate math (conv_gru.py:22-27)
# ------------------------------------------------------------------------------------------------------------------
PLANTED = [0.0, 2.0 ** -10, -2.0 ** -10, 8.0, -8.0, 16.0, -16.0, 88.0, -88.0, 100.0, -100.0, 20000.0, -20000.0]
GRU_GEOMS = [(1, 8, BF16), (1, 8, F16), (1, 4, F32)] + [(M, C, dt) for (M, C) in ((7, 24), (60, 16), (257, 16)) for dt in (BF16, F16, F32)] + \
            [(8200, 512, F32), (16400, 512, BF16)]          # the last two: 1 049 600 chunks each, one wrap of the 4096 x 256 grid


def gru_case(M, C, dtype, seed=0):
    """Operands of the four kernels, rounded to `dtype`: normal draws with standard deviation 2; the first and the last row of rz and cpre carry
    the planted pre-activations (20000 is 19968 in bf16; all of them lie inside fp16's range)."""
    g = torch.Generator().manual_seed(1000 + seed)
    t = {n: torch.randn((M, w), generator=g, dtype=F32) * 2 for n, w in (('rz', 2 * C), ('x', C), ('h', C), ('cpre', C), ('dxrh', 2 * C), ('dhn', C))}
    pl = torch.tensor(PLANTED, dtype=F32)
    for name in ('rz', 'cpre'):
        w = t[name].shape[1]
        t[name][0] = pl[torch.arange(w) % len(pl)]
        t[name][M - 1] = pl[(torch.arange(w) + 7) % len(pl)] if M > 1 else t[name][0]
    return {n: v.to(dtype) for n, v in t.items()}


def gru(rz, x, h, cpre, dxrh, dhn, dt=F64, fault=None, ce=4, row0=0):
    """xrh = [x | sigmoid(r) h], hn = (1 - z) h + z tanh(c) and the six gradients dx, dr (= drz[:, :C]), dh1, dz (= drz[:, C:]), dc, dh2.
    ce: elements per work item (8 in 16-bit, 4 in fp32), row0: the row the operands start at in their case; both for the 'past_grid' fault only."""
    rz, x, h, cpre, dxrh, dhn = (t.to(dt) for t in (rz, x, h, cpre, dxrh, dhn))
    C = x.shape[1]
    rv, zv = rz[:, :C], rz[:, C:]
    if fault == 'swap_rz':
        rv, zv = zv, rv
    r, z, tc = sig(rv, dt), sig(zv, dt), torch.tanh(cpre)
    cr, cz = 1 + rv.abs(), 1 + zv.abs()
    g2, atc = dxrh[:, C:], tc.abs()
    out = {}
    rh = r * h
    out['xrh'] = (torch.cat([x, rh], 1), torch.cat([x.abs(), rh.abs() * cr + _fl(r, h)], 1))
    hn = (z if fault == 'z_for_1mz' else 1 - z) * h + z * tc
    out['hn'] = (hn, ((1 + z) * h.abs() + z * atc) * cz + _fl(z, tc))
    out['dx'] = (dxrh[:, :C].clone(), dxrh[:, :C].abs())
    out['dr'] = (g2 * h * r * (1 - r), (g2 * h).abs() * r * (1 + r) * cr + _fl(r * (1 - r), g2 * h))
    out['dh1'] = (g2 * r, g2.abs() * r * cr + _fl(r, g2))
    out['dz'] = (dhn * (tc - h) * z * (1 - z), dhn.abs() * (atc + h.abs()) * z * (1 + z) * cz + _fl(z * (1 - z), dhn * (atc + h.abs())))
    omt = (1 - tc) if fault == 'one_minus_tc' else 1 - tc * tc
    out['dc'] = (dhn * z * omt, dhn.abs() * z * (1 + tc * tc) * cz + _fl(z, dhn * (1 + tc * tc)))
    out['dh2'] = (dhn * (1 - z), dhn.abs() * (1 + z) * cz)
    if fault == 'drop_last_row':
        for v, _ in out.values():
            v[-1] = 0
    if fault == 'past_grid':                    # everything past work item 4096 x 256 left unwritten
        cpr = C // ce
        item = (row0 + torch.arange(x.shape[0]))[:, None] * cpr + (torch.arange(C) // ce)[None, :]
        for name, (v, _) in out.items():
            v[(item.repeat(1, 2) if v.shape[1] == 2 * C else item) >= GRID] = 0
    return out


K_GRU = {
    'xrh': K_SIGMUL,             # sigm 7 (__expf 4, 1 + e, reciprocal 2), times h; the x half is a copy (compared with equality as well)
    'hn': 15,                    # sigm 7, 1 - z, times h, tanhf 4, z * tc, the sum
    'dx': 0,                     # a copy
    'dr': K_SIGMUL_BWD,          # sigm 7, 1 - r, three products, one spare for the product order (rows_reference)
    'dh1': K_SIGMUL,             # sigm 7, times g
    'dz': 16,                    # sigm 7, 1 - z, tanhf 4, tc - h, three products
    'dc': 15,                    # sigm 7, tanhf 4, tc * tc, 1 - ., two products
    'dh2': 9,                    # sigm 7, 1 - z, times g
}


# ------------------------------------------------------------------------------------------------------------------
# eval-time alpha aggregation (maggie_temp.py:34-77, n_frames >= 3, "t+1" = the last frame): compared with equality
# ------------------------------------------------------------------------------------------------------------------
FUSE_FRAMES = [3, 4, 5, 16]
FUSE_PLANES = [1, 255, 256, 257, GRID + 513]


def fuse_case(n_frames, n, seed=0, with_prev=True):
    """alphas (n_frames, n) uniform, prev (n,), difference maps (n_frames, n) uniform with the values exactly 0.5 and the next float above it planted
    in frames 1 and 2. On a third of the pixels the last frame equals prev (or frame 0), so that the propagated values can agree where neither
    difference map fires. A one-pixel plane carries df[1] = 0.5 and db[1] = nextafter(0.5)."""
    g = torch.Generator().manual_seed(2000 + seed)
    a = torch.rand((n_frames, n), generator=g)
    prev = torch.rand(n, generator=g) if with_prev else None
    same = torch.rand(n, generator=g) < 1 / 3
    a[n_frames - 1] = torch.where(same, a[0] if prev is None else prev, a[n_frames - 1])
    df, db = torch.rand((n_frames, n), generator=g), torch.rand((n_frames, n), generator=g)
    half, above = 0.5, float(np.nextafter(np.float32(0.5), np.float32(1)))
    for t in (df, db):
        for fr in (1, 2):
            t[fr, 0::7] = half
            t[fr, 3::7] = above
    if n == 1:
        db[1, 0] = above
    return a, prev, df, db


def fuse(alphas, prev, df, db, fault=None):
    """With the difference maps thresholded to 0 / 1 every product and sum below is exact. -> {'alphas': all frames, 'disagree': bool mask}"""
    a = alphas.double()
    last = 2 if fault == 'last_is_2' else a.shape[0] - 1
    on = (lambda t: (t >= 0.5).double()) if fault == 'ge' else (lambda t: (t > 0.5).double())
    f1, f2, b1 = on(df[1]), on(df[2]), on(db[1])
    pv = a[0] if prev is None else prev.double()
    fwd = pv * (1 - f1) + a[1] * f1                     # t-1 -> t
    bwd = a[last] * (1 - b1) + a[1] * b1                # t+1 -> t
    dis = (fwd - bwd).abs() > 0
    fwd = torch.where(dis, a[1], fwd)                   # the two disagree: keep the model's own prediction
    out = a.clone()
    out[1] = fwd
    out[2] = fwd * (1 - f2) + a[last] * f2              # t -> t+1
    return {'alphas': (out, None), 'disagree': (dis, None)}


# ------------------------------------------------------------------------------------------------------------------
# bidirectional fusion (resnet_inst_matt_spconv_temp.py:53-78), forward and backward
# ------------------------------------------------------------------------------------------------------------------
BIFUSE_T = [2, 3, 5, 16]
BIFUSE_SHAPES = [(1, 1, 1, 1), (2, 3, 8, 24), (3, 2, 5, 51), (2, 1, 1, 257)]
BIFUSE_WRAP = (1, 1, 1025, 1024)          # at T = 2 only: 1 049 600 pixels, one wrap of the grid
K_BIFUSE = 11                             # one frame step: sigm 7, 1 - s, two products, one sum (the 0.5 of the average is exact)
K_BIFUSE_SIG = K_SIGMUL                   # the sigmoid stacks: sigm 7 (times one)


def k_bifuse_dd(NI):
    """ddiffs: a sum over NI instances of products formed by frame steps, then times s (1 - s): 1 - s and two products."""
    return sum_k(NI) + K_BIFUSE + 3


def bifuse_case(B, T, NI, H, W, seed=0):
    """preds uniform, logits normal with standard deviation 3 and 0, +-30, +-100 planted, a normal weight on the fused output."""
    g = torch.Generator().manual_seed(3000 + seed)
    preds = torch.rand((B, T, NI, H, W), generator=g)
    diffs = torch.randn((2 * (T - 1), B, 1, H, W), generator=g) * 3
    pl = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0])
    flat = diffs.view(-1)
    idx = torch.arange(0, flat.numel(), 11)
    flat[idx] = pl[torch.arange(idx.numel()) % 5]
    if flat.numel() < 5:
        flat[:] = pl[(torch.arange(flat.numel()) + 3 + seed) % 5]
    dfused = torch.randn((B, T, NI, H, W), generator=g)
    return preds, diffs, dfused


# (value, S) pairs of the recursions; an operand that arrives exact has S = 0, every operation adds the magnitude it rounds
def _ms(a, s, c):
    return a[0] * s, a[1] * s + a[0].abs() * s * c + _fl(s, a[0])


def _m1(a, s, c):
    return a[0] * (1 - s), a[1] * (1 - s) + a[0].abs() * (1 + s) * c


def _add(a, b):
    return a[0] + b[0], a[1] + b[1] + a[0].abs() + b[0].abs()


def _mul(a, b):
    return a[0] * b[0], a[1] * b[0].abs() + a[0].abs() * b[1] + (a[0] * b[0]).abs()


def bifuse(preds, diffs, dfused, dt=F64, fault=None):
    """-> fused, fdiff, bdiff, fsig, bsig, dpreds, ddiffs. The backward is written out chain by chain (the host proof compares it with autograd)."""
    p, d, g = preds.to(dt), diffs.to(dt), dfused.to(dt)
    B, T, NI, H, W = p.shape
    zero = torch.zeros((B, 1, H, W), dtype=dt)
    ex = lambda v: (v, torch.zeros_like(v))           # noqa: E731

    def bslot(t):                                      # the backward logit stored at frame t
        s = 2 * T - 3 - t
        return T - 1 + (s - (T - 1) + 1) % (T - 1) if fault == 'slot_off' else s
    fd = [zero] + [d[t - 1] for t in range(1, T)]
    bd = [d[bslot(t)] for t in range(T - 1)] + [zero]
    sf, sb = [sig(v, dt) for v in fd], [sig(v, dt) for v in bd]
    cf, cb = [1 + v.abs() for v in fd], [1 + v.abs() for v in bd]
    fp, bp = [None] * T, [None] * T
    fp[0] = ex(p[:, 0])
    for t in range(1, T):
        fp[t] = _add(_m1(fp[t - 1], sf[t], cf[t]), _ms(ex(p[:, t]), sf[t], cf[t]))
    bp[T - 1] = ex(p[:, T - 1])
    for t in range(T - 2, -1, -1):
        bp[t] = _add(_m1(bp[t + 1], sb[t], cb[t]), _ms(ex(p[:, t]), sb[t], cb[t]))
    fused = []
    for t in range(T):
        if t == 0 and fault != 'avg_frame0':
            fused.append(fp[0])
        elif t == T - 1:
            fused.append(bp[t])
        else:
            v, S = _add(fp[t], bp[t])
            fused.append((v, S) if fault == 'no_half' and 0 < t else (0.5 * v, 0.5 * S))
    out = {'fused': tuple(torch.stack(q, 1) for q in zip(*fused))}
    out['fdiff'], out['bdiff'] = (torch.stack(fd, 1), None), (torch.stack(bd, 1), None)
    out['fsig'] = (torch.stack(sf, 1), torch.stack([s * c + _fl(s, torch.ones_like(s)) for s, c in zip(sf, cf)], 1))
    out['bsig'] = (torch.stack(sb, 1), torch.stack([s * c + _fl(s, torch.ones_like(s)) for s, c in zip(sb, cb)], 1))
    # backward
    z4 = ex(torch.zeros((B, NI, H, W), dtype=dt))
    dpl = [z4] * T
    gsf, gsb = [ex(zero)] * T, [ex(zero)] * T
    tot = lambda q: (q[0].sum(1, keepdim=True), q[1].sum(1, keepdim=True))       # noqa: E731  over the instances
    carry = z4
    for t in range(T - 2, 0, -1):                      # forward chain: fused[t] = (fp[t] + bp[t]) / 2 for 0 < t < T - 1
        gt = _add(ex(0.5 * g[:, t]), carry)
        dpl[t] = _add(dpl[t], _ms(gt, sf[t], cf[t]))
        dif = (p[:, t] - fp[t - 1][0], fp[t - 1][1] + p[:, t].abs() + fp[t - 1][0].abs())
        gsf[t] = _add(gsf[t], tot(_mul(gt, dif)))
        carry = z4 if fault == 'no_carry' else _m1(gt, sf[t], cf[t])
    dpl[0] = _add(dpl[0], _add(ex(g[:, 0]), carry))
    G = z4
    for t in range(1, T):                              # backward chain: G = dL / dbp[t - 1]
        gprev = G
        dpl[t - 1] = _add(dpl[t - 1], _ms(gprev, sb[t - 1], cb[t - 1]))
        dif = (p[:, t - 1] - bp[t][0], bp[t][1] + p[:, t - 1].abs() + bp[t][0].abs())
        gsb[t - 1] = _add(gsb[t - 1], tot(_mul(gprev, dif)))
        G = _add(ex(0.5 * g[:, t] if t <= T - 2 else g[:, T - 1]), _m1(gprev, sb[t - 1], cb[t - 1]))
    dpl[T - 1] = _add(dpl[T - 1], G)
    out['dpreds'] = tuple(torch.stack(q, 1) for q in zip(*dpl))

    def dlogit(q, s, c):
        return q[0] * s * (1 - s), q[1] * s * (1 - s) + q[0].abs() * s * (1 + s) * c + _fl(s * (1 - s), q[0])
    dd = [None] * (2 * (T - 1))
    for t in range(1, T):
        dd[t - 1] = dlogit(gsf[t], sf[t], cf[t])
    for t in range(T - 1):
        dd[2 * T - 3 - t] = dlogit(gsb[t], sb[t], cb[t])
    out['ddiffs'] = tuple(torch.stack(q, 0) for q in zip(*dd))
    return out


# ------------------------------------------------------------------------------------------------------------------
# loss_dtSSD (maggie/network/loss.py:7-16) and mean BCE with logits, on (B, T, 1, E) frame slices
# ------------------------------------------------------------------------------------------------------------------
LOSS_GEOMS = [(1, 2, 1), (1, 2, 255), (2, 3, 257), (2, 4, 384), (1, 3, 262444), (2, 2, 524365)]
# (sig, mask, slice, ground truth through the copy path of _frames): every option with every other at least once
LOSS_COMBOS = [(0, None, 'full', 0), (1, None, 'tail', 1), (1, None, 'head', 1), (0, '01', 'tail', 0), (1, 'frac', 'full', 0), (0, 'zero', 'head', 0),
               (1, '01', 'head', 0), (0, 'frac', 'tail', 1), (1, 'zero', 'full', 0)]
BCE_COMBOS = [(kind,) + c[1:] for c in LOSS_COMBOS[:3] for kind in (0, 1)]      # three slices; the first entry selects 0 / 1 (0) or fractional targets
GOUT = 1.7000000476837158                 # float32(1.7): the weight of the loss in the backward
K_DTSSD_TERM = 12                         # sigm 7, three differences, the square, times m
K_DTSSD_GRAD = 19                         # 2 * gout / sums[1] 3, sigm 7, three differences, times c, times m, frame difference, 1 - p, two products
K_BCE_TERM = 11                           # x * y, the difference, __expf 4, log1pf 4, the sum (fmaxf and fabsf are exact)
K_BCE_GRAD = 11                           # gout / n 2, sigm 7, - y, times c


def k_dtssd(n):
    """sums[0], sums[1], the loss (torch's division of the two device sums, counted 2) and the gradient (on top of sums[1])."""
    return {'sum0': sum_k(n) + K_DTSSD_TERM, 'sum1': sum_k(n) + 1, 'loss': sum_k(n) + K_DTSSD_TERM + 2, 'grad': sum_k(n) + 1 + K_DTSSD_GRAD}


def atomic_k(items):
    """What the atomic form of a cross-workgroup sum over `items` work items adds to k. sum_k counts a tree; with atomicAdd the per-workgroup
    partials (at most 1024 workgroups of 256 items) are added one after another in arrival order, blocks - 1 further additions on the path. They do
    not average out when the partials are alike: sums[1] over an absent mask adds 1024 equal partials and every addition rounds the same way.
    (Added after the first device run, which measured 41.6 on the atomic sums[1] at 1024 workgroups against sum_k + 1 = 29; the deterministic form
    of the same sum measured 2.0. The count had missed these additions; no other k changed.)"""
    return min(1024, -(-items // 256)) - 1


def k_bce(n):
    return {'sum': sum_k(n) + K_BCE_TERM, 'loss': sum_k(n) + K_BCE_TERM + 2, 'grad': K_BCE_GRAD}


def _sliced(parent, how):
    return parent if how == 'full' else parent[:, 1:] if how == 'tail' else parent[:, :-1]


def loss_case(B, T, E, combo, seed=0, integer=False, bce=False):
    """-> the tensors loss_views() takes: the clip, the slice spec, a two-channel ground truth and mask. The slices `tail` / `head` are [:, 1:] / [:, :-1] of a clip of T + 1 frames;
    copy: the ground truth (and the mask) is t[:, 1:, 0:1] of a two-channel tensor of T + 1 frames. integer: p, g from {0, 1, 2}, mask 0 / 1.
    bce: logits with standard deviation 4 and planted 0, +-2^-12, +-20, +-88, +-100, +-1e4."""
    sig_on, mask, how, copy = combo
    g = torch.Generator().manual_seed(4000 + seed)
    Tp = T if how == 'full' else T + 1
    if integer:
        parent = torch.randint(0, 3, (B, Tp, 1, E), generator=g).float()
    else:
        parent = torch.randn((B, Tp, 1, E), generator=g) * (4 if bce else 1.5)
    if bce:
        pl = torch.tensor([0.0, 2.0 ** -12, -2.0 ** -12, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4])
        flat = parent.view(-1)
        idx = torch.arange(0, flat.numel(), 3) if flat.numel() < 64 else torch.arange(0, flat.numel(), 23)
        flat[idx] = pl[(torch.arange(idx.numel()) + seed) % len(pl)]

    def side(kind):
        if integer:
            return torch.randint(0, 3 if kind == 'gt' else 2, (B, T + 1, 2, E), generator=g).float()
        full = torch.rand((B, T + 1, 2, E), generator=g)
        if kind == 'gt':
            return (full > 0.5).float() if bce and not sig_on else full      # BCE: 0 / 1 targets for half of the combinations, fractional for the other
        return (full > 0.3).float() if mask == '01' else full * 0 if mask == 'zero' else full
    return {'parent': parent, 'how': how, 'gt': side('gt'), 'mask': None if mask is None else side('mask'), 'copy': copy}


def loss_views(parent, how, gt, mask, copy):
    """The tensors a loss call receives, from the tensors of loss_case() (on whatever device they are): the frame slice of the clip, and
    t[:, 1:, 0:1] of the two-channel ground truth / mask (copy: that view itself, which takes the copy path of _frames; else made contiguous)."""
    view = (lambda t: t[:, 1:, 0:1]) if copy else (lambda t: t[:, 1:, 0:1].contiguous())
    return _sliced(parent, how), view(gt), None if mask is None else view(mask)


def dtssd(p, g, m, sig_on, gout=GOUT, dt=F64, fault=None):
    """p: the (B, T, 1, E) slice (a view of its clip), g, m (None: ones). -> sum0, sum1, loss, grad (same shape as p)."""
    B, T, _, E = p.shape
    if fault == 'stride_TE' and B > 1:                  # the batch stride of a slice taken as T * E instead of the clip's
        p = torch.as_strided(p, p.shape, (T * E, E, E, 1), p.storage_offset())
    raw, g = p.to(dt), g.to(dt)
    one = torch.ones((B, T, 1, E), dtype=dt)
    mm = one if m is None else m.to(dt)
    if T < 2:
        z = torch.zeros((), dtype=dt)
        return {'sum0': (z, z), 'sum1': (z, z), 'loss': (z / z, z), 'grad': (torch.zeros_like(raw), torch.zeros_like(raw))}
    pv = sig(raw, dt) if sig_on else raw
    A = pv.abs() * (1 + raw.abs()) if sig_on else pv.abs()
    sgn = 1.0 if fault == 'gp_sign' else -1.0
    dd = (pv[:, 1:] - pv[:, :-1]) - (g[:, 1:] + sgn * g[:, :-1])
    S_d = A[:, 1:] + A[:, :-1] + g[:, 1:].abs() + g[:, :-1].abs()
    mv = mm[:, 1:]
    sum0, S0 = (dd * dd * mv).sum(), (2 * dd.abs() * S_d * mv).sum()
    sum1 = ((mm if fault == 'mask_frame0' else mv) + 1e-6).sum()
    loss = sum0 / sum1
    c = 2 * gout / sum1
    D, S_D = c * dd * mv, c * S_d * mv
    zf = torch.zeros_like(D[:, :1])
    gp = torch.cat([zf, D], 1) - torch.cat([D, zf], 1)
    S_gp = torch.cat([zf, S_D], 1) + torch.cat([S_D, zf], 1)
    if sig_on:
        S_gp = S_gp * pv * (1 + pv) * (1 + raw.abs()) + _fl(pv * (1 - pv), gp)
        gp = gp * pv * (1 - pv)
    return {'sum0': (sum0, S0), 'sum1': (sum1, sum1.abs()), 'loss': (loss, S0 / sum1 + loss.abs()), 'grad': (gp, S_gp)}


def bce(x, y, gout=GOUT, dt=F64, fault=None):
    """F.binary_cross_entropy_with_logits(x, y, reduction='mean'): max(x, 0) - x y + log1p(exp(-|x|)). -> sum, loss, grad."""
    x, y = x.to(dt), y.to(dt)
    n = x.numel()
    e = torch.exp(-x.abs()) if dt == F64 else torch.exp2(-x.abs() * LOG2E)
    l = torch.log1p(e)
    xy = torch.zeros_like(x) if fault == 'no_xy' else x * y
    term = x.clamp_min(0) - xy + l
    S_t = x.clamp_min(0) + (x * y).abs() + e * (1 + x.abs()) + l + _fl(e, torch.ones_like(e))
    s, S = term.sum(), S_t.sum()
    cnt = n // x.shape[1] if fault == 'wrong_count' else n          # the mean over B * E instead of B * T * E
    sg = sig(x, dt)
    grad = gout / cnt * (sg - y)
    S_g = gout / cnt * (sg * (1 + x.abs()) + y.abs()) + _fl(sg, torch.full_like(sg, gout / cnt))
    return {'sum': (s, S), 'loss': (s / cnt, S / cnt), 'grad': (grad, S_g)}


# ------------------------------------------------------------------------------------------------------------------
# eval-time bounding-box crop, as the header of temporal2.hip states it: compared with equality
# ------------------------------------------------------------------------------------------------------------------
CROP_GEOMS = [(1, 8, 8), (3, 40, 63), (2, 33, 64), (2, 37, 65), (65, 8, 72), (32, 200, 168)]
CROP_THR, CROP_SIGMA = 0.1, 3
BOX_EMPTY = [1 << 30, -1, 1 << 30, -1]
# the coefficients on the host 10 (expf 4, the normaliser's three sums, division 2, square), horizontal pass 13 (7 products, 6 sums), 7-row sum 6,
# the scale 2 (a division), the source coordinate 3, the fraction 1, 1 - fraction 1, the inner and the outer blend 3 each (two products, one sum)
K_CROP = 42
K_COORD = 6                      # of these, the operations behind the fraction: the scale 2, the product, - 0.5, the fraction, 1 - fraction
CROP_SECOND = {'seed': 1, 'shift': 4}      # the second set of planes of a geometry (seeds chosen so that no case has an undecided pixel)
KINDS = ['nothing', 'full', 'top', 'bottom', 'left', 'right', 'pixel', 'faint', 'two']


def crop_pads(W):
    return [0, 30, W + 5]


def crop_case(P, H, W, seed=0, shift=0):
    """alpha planes (P, H, W) fp32 and boolean planes for the bits. Plane p holds KINDS[(p + offset) % 9]: nothing, foreground everywhere, a blob
    touching the top / bottom / left / right border (the bottom one lies in the last five rows), one pixel of 1.0, a faint blob that stays below the
    threshold, two blobs far apart. -> alpha, bits, kinds"""
    g = torch.Generator().manual_seed(5000 + seed)
    a = torch.zeros((P, H, W))
    off = 1 + seed + shift
    kinds = [KINDS[(p + off) % len(KINDS)] for p in range(P)]
    q = lambda n, f: max(1, int(n * f))                # noqa: E731
    blob = lambda h, w: torch.rand((h, w), generator=g) * 0.6 + 0.4      # noqa: E731
    for p, kind in enumerate(kinds):
        if kind == 'full':
            a[p] = blob(H, W)
        elif kind == 'top':
            a[p, :q(H, .3), q(W, .3):q(W, .3) + q(W, .4)] = blob(q(H, .3), q(W, .4))
        elif kind == 'bottom':
            hb = min(5, H)
            a[p, H - hb:, q(W, .2):q(W, .2) + q(W, .5)] = blob(hb, q(W, .5))
        elif kind == 'left':
            a[p, q(H, .4):q(H, .4) + q(H, .4), :q(W, .2)] = blob(q(H, .4), q(W, .2))
        elif kind == 'right':
            a[p, q(H, .1):q(H, .1) + q(H, .5), W - q(W, .25):] = blob(q(H, .5), q(W, .25))
        elif kind == 'pixel':
            a[p, H // 2, W // 3] = 1.0
        elif kind == 'faint':
            a[p, q(H, .3):q(H, .3) + q(H, .3), q(W, .5):q(W, .5) + q(W, .3)] = 0.05
        elif kind == 'two':
            h1, h2, w2 = max(3, q(H, .2)), max(3, q(H, .25)), max(3, q(W, .2))
            a[p, :h1, :q(W, .15)] = blob(h1, q(W, .15))
            a[p, H - h2:, W - w2:] = blob(h2, w2)
    bits = torch.rand((P, H, W), generator=g) > 0.4
    return a, bits, kinds


def crop_smooth(a, sigma=CROP_SIGMA, dt=F64, fault=None):
    """The smoothed, cropped and resized planes. -> val (P, H, W) and S: the four taps, plus the distance of the taps times the size of the source
    coordinate (the fp32 coordinate (y + 0.5) * (H - 6) / H - 0.5 carries a relative error, so the fraction an absolute one that grows with it)."""
    a = a.to(dt)
    P, H, W = a.shape
    j = torch.arange(7, dtype=dt) - 3
    gw = torch.exp(-j * j / (2.0 * sigma * sigma))
    gw = gw / gw.sum()
    across = gw if fault in ('g_not_sq', 'gauss2d') else gw * gw               # g2[j] = (g[j] / sum g)^2 on every row
    down = gw if fault == 'gauss2d' else torch.ones(7, dtype=dt)
    ap = F.pad(a, (3, 3, 3, 3))
    h = sum(across[k] * ap[:, :, k:k + W] for k in range(7))                  # (P, H + 6, W)
    sm = sum(down[k] * h[:, k:k + H] for k in range(7))                       # (P, H, W)
    c = sm[:, 3:H - 3, 3:W - 3]
    Hc, Wc = H - 6, W - 6

    def src(n, nc):
        f = ((torch.arange(n, dtype=dt) + 0.5) * (torch.tensor(nc, dtype=dt) / n) - 0.5).clamp_min(0)
        i0 = f.floor().long()
        return f, i0, (i0 + 1).clamp_max(nc - 1), f - i0
    fy, y0, y1, ly = src(H, Hc)
    fx, x0, x1, lx = src(W, Wc)
    ly, fy = ly[None, :, None], fy[None, :, None]
    v00, v01, v10, v11 = c[:, y0][:, :, x0], c[:, y0][:, :, x1], c[:, y1][:, :, x0], c[:, y1][:, :, x1]
    val = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
    S = v00 + v01 + v10 + v11 + (K_COORD / K_CROP) * ((fy + 1) * ((v10 - v00).abs() + (v11 - v01).abs()) + (fx + 1) * ((v01 - v00).abs() + (v11 - v10).abs()))
    return val, S


def crop_undecided(val, S, thr=CROP_THR):
    """Pixels whose decision cannot be compared across precisions: |val - thr| <= U32 K_CROP S (S >= val: no laxer than K_CROP val)."""
    return int(((val - thr).abs() <= U32 * K_CROP * S).sum())


def crop_boxes(above):
    """(P, H, W) bool -> (P, 4) int32 [ymin, ymax, xmin, xmax], BOX_EMPTY for a plane without a pixel."""
    P, H, W = above.shape
    ry, rx = above.any(2), above.any(1)
    ys, xs = torch.arange(H)[None], torch.arange(W)[None]
    big, neg = torch.tensor(1 << 30), torch.tensor(-1)
    box = torch.stack([torch.where(ry, ys, big).min(1)[0], torch.where(ry, ys, neg).max(1)[0],
                       torch.where(rx, xs, big).min(1)[0], torch.where(rx, xs, neg).max(1)[0]], 1)
    return box.to(torch.int32)


def crop_inside(box, H, W, pad, fault=None):
    """(P, H, W) bool: [ymin - pad, ymax + pad) x [xmin - pad, xmax + pad) clamped; an empty plane keeps everything."""
    P = box.shape[0]
    inside = torch.zeros((P, H, W), dtype=torch.bool)
    for p in range(P):
        ymin, ymax, xmin, xmax = (int(v) for v in box[p])
        if ymax < ymin:
            inside[p] = fault != 'empty_zeroed'
            continue
        inc = 1 if fault == 'ymax_inclusive' else 0
        if fault == 'pad_after_clamp':                 # the slice bounds of a restatement that pads the clamped box: a negative start wraps
            inside[p][slice(max(ymin, 0) - pad, min(ymax, H) + pad), slice(max(xmin, 0) - pad, min(xmax, W) + pad)] = True
        else:
            inside[p, max(ymin - pad, 0):min(ymax + pad + inc, H), max(xmin - pad, 0):min(xmax + pad, W)] = True
    return inside


def crop(alpha, bits, pad, sigma=CROP_SIGMA, thr=CROP_THR, dt=F64, fault=None, smooth=None):
    """-> box (int32, as the kernel leaves it: not padded), inside, alpha, bits (bool planes or None). smooth: a crop_smooth() result to reuse."""
    val, _ = crop_smooth(alpha, sigma, dt, fault) if smooth is None else smooth
    P, H, W = alpha.shape
    box = crop_boxes(val > thr)
    inside = crop_inside(box, H, W, pad, fault)
    return {'box': (box, None), 'inside': (inside, None), 'alpha': (alpha * inside, None), 'bits': (None if bits is None else bits & inside, None)}


def bits_words(planes):
    """bool (P, H, W) -> int64 words (P, H, ceil(W / 64)), bit b of word j = column 64 j + b."""
    P, H, W = planes.shape
    Ww = (W + 63) // 64
    a = np.zeros((P, H, Ww * 64), np.uint64)
    a[:, :, :W] = planes.numpy()
    w = (a.reshape(P, H, Ww, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return torch.from_numpy(w.view(np.int64))


def words_bits(words, W):
    a = words.cpu().numpy().view(np.uint64)
    P, H, Ww = a.shape
    b = ((a[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(P, H, Ww * 64)
    return torch.from_numpy(b.astype(bool))
