"""float64 references, case construction and comparison helpers for the device-row-count kernels of the sparse head
(tests/test_gpu_rows.py on the device, tests/test_rows_reference_cpu.py on the host). Plain torch / numpy on the CPU.

A case is a capacity `cap` and a live count `live`. A (cap, C) buffer holds `live` live rows; everything from row `live` on is
poison (NaN), rows 0 and live - 1 carry outliers (16 x the typical magnitude, exact in the case's dtype), and output buffers handed to a
kernel carry GUARD sentinel rows behind the capacity.

Every reference works on the ALREADY ROUNDED operands, in float64, over [:live], and returns the value next to S, the float64 sum of the
absolute values of the terms that form each element (condition included where a difference of large numbers feeds the element). The
comparison is element-wise:

    |got - ref| <= u_out * |ref| + floor + U32 * k * S

u_out: one rounding unit of the output dtype (2^-8 bf16, 2^-10 f16, 0 for an fp32 output), floor: 2^-24 for f16 (subnormals), U32 = 2^-23,
k: fp32 operations on the longest path to the element (the named constants K_* at the end of this file, one per kernel output)."""
import math

import numpy as np
import torch

U32 = 2.0 ** -23
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10, torch.float32: 0.0}
FLOOR = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24, torch.float32: 0.0}
GUARD = 64
OUTLIER = 16
EXACT_LIMIT = 2 ** 24
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def live_counts(cap):
    """The row-count words a case runs with (None = no word at all, must equal `cap`)."""
    return [-3, 0, 1, 5, 257, cap - 1, cap, cap + 1000]


def clamp_live(v, cap):
    return cap if v is None else max(0, min(int(v), cap))


def sum_k(live):
    """Starting k of a column sum of rounded products over `live` rows: a pairwise tree has ceil(log2 n) levels, + 8 for the per-term arithmetic."""
    return int(math.ceil(math.log2(max(live, 2)))) + 8


# ------------------------------------------------------------------------------------------------------------------
# case construction
# ------------------------------------------------------------------------------------------------------------------
def base_rows(cap, C, seed, std=1.0, offset=0.0):
    """(cap, C) float64 normal values; the live / dead split is applied by rows_input()."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((cap, C), generator=g, dtype=torch.float64) * std + offset


def base_int_rows(cap, C, seed, lim=8):
    """(cap, C) float64 integers in [-lim, lim]: exact in bf16 / f16 / f32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, (cap, C), generator=g).double()


def rows_input(base, live, dtype, outlier=OUTLIER, poison=float('nan')):
    """Round `base` to `dtype`, scale rows 0 and live - 1 by `outlier` (a power of two: still exact in dtype), poison rows >= live."""
    t = base.to(dtype).clone()
    if live > 0:
        t[0] *= outlier
        if live > 1:
            t[live - 1] *= outlier
    t[live:] = poison
    return t


def sentinel(shape, dtype):
    """A tensor filled with a fixed finite bit pattern (0x5A5A.. in every element)."""
    if dtype == torch.float32:
        return torch.full(shape, 0x5A5A5A5A, dtype=torch.int32).view(torch.float32)
    return torch.full(shape, 0x5A5A, dtype=torch.int16).view(dtype)


def bits_of(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def guarded(cap, width, dtype):
    """(cap + GUARD, width) sentinel-filled buffer; hand buf[:cap] (or a channel slice of it) to the kernel."""
    return sentinel((cap + GUARD, width), dtype)


def untouched(buf, before, live, cols=None):
    """True when every element of `buf` outside [0:live, cols] still has the bits of `before` (guard rows, dead rows and, for a
    channel slice, the columns next to it)."""
    a, b = bits_of(buf).clone(), bits_of(before).clone()
    c0, c1 = (0, a.shape[1]) if cols is None else cols
    a[:live, c0:c1] = 0
    b[:live, c0:c1] = 0
    return torch.equal(a, b)


def site_coords(cap, n_frames, n_i, seed):
    """`cap` distinct sites (p, y, x) in raster order over P = n_frames * n_i planes of an (H, W) grid, sorted by plane like the head's site
    lists, dense enough that rows of several instance planes share pixels. Pixel (H - 1, W - 1) is reserved in every plane:
    (P - 1, H - 1, W - 1) is the poison site dead rows point at. -> coords (cap, 3) int32, (P, H, W), poison site."""
    P = n_frames * n_i
    W = 16
    H = max(4, -(-int(cap * 1.4 / P + 2) // W))
    rs = np.random.RandomState(seed)
    free = np.ones((P, H, W), bool)
    free[:, H - 1, W - 1] = False
    idx = np.flatnonzero(free.reshape(-1))
    assert idx.size >= cap
    pick = np.sort(rs.choice(idx, cap, replace=False))
    p, rem = np.divmod(pick, H * W)
    y, x = np.divmod(rem, W)
    coords = np.stack([p, y, x], 1).astype(np.int32)
    return torch.from_numpy(coords), (P, H, W), (P - 1, H - 1, W - 1)


def coords_input(coords, live, poison_site):
    c = coords.clone()
    c[live:] = torch.tensor(poison_site, dtype=torch.int32)
    return c


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
MEASURED = {}            # what -> largest observed (err - u_out |ref| - floor) / (U32 * S)


def error_ratio(got, ref, S, dtype):
    """Largest err / (U32 * S) left after the output rounding allowance; inf when an element is NaN / inf or misses with S == 0."""
    got, ref, S = got.detach().cpu().double(), ref.double(), S.double().expand_as(ref)
    if ref.numel() == 0:
        return 0.0
    rest = (got - ref).abs() - U_OUT[dtype] * ref.abs() - FLOOR[dtype]
    rest = torch.where(torch.isfinite(rest), rest.clamp_min(0.0), torch.full_like(rest, float('inf')))
    ratio = torch.where(rest > 0, rest / (U32 * S), torch.zeros_like(rest))       # rest > 0 with S == 0 -> inf
    return float(ratio.max())


def close(got, ref, S, k, dtype):
    """Element-wise |got - ref| <= u_out |ref| + floor + U32 k S; False for any NaN / inf or shape mismatch."""
    if tuple(got.shape) != tuple(ref.shape):
        return False
    return error_ratio(got, ref, S, dtype) <= k


def check(got, ref, S, k, dtype, what):
    """Assert close(); the observed ratio is recorded in MEASURED[what] (and printed when it sets a new maximum) before the assertion."""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    r = error_ratio(got, ref, S, dtype)
    if r > MEASURED.get(what, -1.0):
        MEASURED[what] = r
        print('RATIO %-28s %-8s n=%-8d err/(u32*S) = %.3f (k = %s)' % (what, str(dtype).replace('torch.', ''), ref.numel(), r, k))
    assert r <= k, '%s: err / (u32 S) = %g > k = %g' % (what, r, k)


def exact(got, ref, what):
    """Bit-exact comparison of an fp32 result with a float64 reference that is exactly representable (exact-integer sums)."""
    assert float(ref.abs().max()) < EXACT_LIMIT if ref.numel() else True, what
    g = got.detach().cpu().double()
    assert torch.equal(g, ref.double()), '%s: %d of %d elements differ' % (what, int((g != ref).sum()), ref.numel())


def assert_exact_conditions(*operands, partial_bound):
    """The preconditions of an exact-integer case: every operand is an integer that bf16 and f16 represent, and the largest sum of
    absolute values any partial sum can reach stays below 2^24 -- then every fp32 partial sum is exact whatever the order."""
    for t in operands:
        t = t.double()
        t = t[torch.isfinite(t)]
        assert torch.equal(t, t.round())
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    assert float(partial_bound) < EXACT_LIMIT, partial_bound


# ------------------------------------------------------------------------------------------------------------------
# references (float64, live rows only). Operands arrive rounded; every function returns (value, S) pairs.
# ------------------------------------------------------------------------------------------------------------------
def _act(t, act, slope):
    if act == ACT_RELU:
        return torch.relu(t)
    if act == ACT_LEAKY:
        return torch.where(t > 0, t, t * slope)
    return t


def sigmoid_mul(a, g):
    """a * sigmoid(g). The fast exponential forms exp2(g * log2 e): the rounding of that product is a relative error |g| u32 / 2 of the
    result, so the condition 1 + |g| is part of S."""
    a, g = a.double(), g.double()
    out = a * torch.sigmoid(g)
    return out, out.abs() * (1 + g.abs())


def sigmoid_mul_bwd(dout, a, g):
    """da = dout * s, dg = dout * a * s * (1 - s); 1 - s is a difference of two terms of size 1 and s."""
    d, a, g = dout.double(), a.double(), g.double()
    s = torch.sigmoid(g)
    da, dg = d * s, d * a * s * (1 - s)
    return (da, da.abs() * (1 + g.abs())), (dg, (d * a * s).abs() * (1 + s) * (1 + g.abs()))


def add(a, b):
    a, b = a.double(), b.double()
    return a + b, a.abs() + b.abs()


def dropout_keep(y):
    """The keep mask a dropout output implies (the input of a case has no zeros)."""
    return y.detach().cpu().double() != 0


def layernorm(x, r, gamma, beta, eps):
    """LayerNorm(x + r) * gamma + beta per row, biased variance. -> (y, S), (mean, S), (rstd, S).
    v - mean is a difference: its absolute error is u32 (|v| + |mean|) per operation, which reaches y directly and through rstd
    (relative error of rstd ~ <|d| (|v| + |mean|)> / var), hence the factor 1 + |xhat| and S of rstd."""
    v = x.double() + r.double()
    gamma, beta = gamma.double(), beta.double()
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xh = d * rstd
    y = xh * gamma + beta
    mag = v.abs() + v.abs().mean(1, keepdim=True)
    s_var = var + 2 * (d.abs() * mag).mean(1, keepdim=True)
    s_rstd = rstd + 0.5 * rstd ** 3 * s_var
    s_y = (mag * rstd + d.abs() * s_rstd) * gamma.abs() + beta.abs()
    return (y, s_y), (mean[:, 0], v.abs().mean(1)), (rstd[:, 0], s_rstd[:, 0])


def layernorm_bwd(dy, x, r, gamma, mean, rstd):
    """-> (dz, S), (dgamma, S), (dbeta, S) with the stored row statistics (mean, rstd) taken as operands."""
    dy, v, gamma = dy.double(), x.double() + r.double(), gamma.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    C = v.shape[1]
    xh = (v - mean) * rstd
    cond = (v.abs() + mean.abs()) * rstd                       # |xhat| <= cond: the size of the terms behind xhat
    dg = dy * gamma
    s1, s2 = dg.sum(1, keepdim=True) / C, (dg * xh).sum(1, keepdim=True) / C
    dz = rstd * (dg - s1 - xh * s2)
    s_s2 = (dg.abs() * cond).sum(1, keepdim=True) / C
    s_dz = rstd * (dg.abs() + dg.abs().sum(1, keepdim=True) / C + cond * s2.abs() + xh.abs() * s_s2)
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    return (dz, s_dz), (dgamma, (dy.abs() * cond).sum(0)), (dbeta, dy.abs().sum(0))


def batchnorm(x, gamma, beta, rm, rv, momentum, eps, count_mult=1, res=None, act=ACT_NONE, slope=0.2, one_pass=False):
    """Training BatchNorm over the live rows x (n, C), n >= 1 -> dict of (value, S): scale, shift, mean, invstd, running_mean, running_var, y, and
    the plain column sums `sum`, `sumsq`, `censq` (sum of centred squares). The running variance is unbiased over n * count_mult samples.
    one_pass: S of the variance for the E[x^2] - E[x]^2 form (else the two-pass form)."""
    x, gamma, beta, rm, rv = x.double(), gamma.double(), beta.double(), rm.double(), rv.double()
    n = x.shape[0]
    mean = x.mean(0)
    d = x - mean
    var = (d * d).mean(0)
    invstd = torch.rsqrt(var + eps)
    ax = x.abs().mean(0)
    s_var = ((x * x).mean(0) + mean * mean) if one_pass else (var + 2 * (d.abs() * (x.abs() + mean.abs())).mean(0))
    s_inv = invstd + 0.5 * invstd ** 3 * s_var
    scale = gamma * invstd
    shift = beta - mean * scale
    s_scale = gamma.abs() * s_inv
    s_shift = beta.abs() + gamma.abs() * (ax * invstd + mean.abs() * s_inv)
    nu = n * count_mult
    unb = var * nu / (nu - 1) if nu > 1 else var
    out = {'mean': (mean, ax), 'invstd': (invstd, s_inv), 'scale': (scale, s_scale), 'shift': (shift, s_shift),
           'running_mean': ((1 - momentum) * rm + momentum * mean, (1 - momentum) * rm.abs() + momentum * ax),
           'running_var': ((1 - momentum) * rv + momentum * unb, (1 - momentum) * rv.abs() + momentum * s_var * (nu / (nu - 1) if nu > 1 else 1)),
           'sum': (x.sum(0), x.abs().sum(0)), 'sumsq': ((x * x).sum(0), (x * x).sum(0)), 'censq': ((d * d).sum(0), s_var * n)}
    pre = x * scale + shift + (0 if res is None else res.double())
    s_pre = x.abs() * s_scale + s_shift + (0 if res is None else res.double().abs())
    out['y'] = (_act(pre, act, slope), s_pre)
    return out


def act_grad(dy, y, act, slope):
    """g = dy * act'(y), the mask taken from the stored activation output y."""
    g = dy.double()
    if act == ACT_RELU:
        return torch.where(y.double() > 0, g, torch.zeros_like(g))
    if act == ACT_LEAKY:
        return torch.where(y.double() > 0, g, g * slope)
    return g


def batchnorm_bwd(dy, y, x, scale, mean, invstd, act=ACT_NONE, slope=0.2, n=None, sums=None):
    """BatchNorm(+activation) backward over the live rows with the stored (scale, mean, invstd) as operands: -> dict of (value, S):
    dx, dres (= g), sum_g (dbeta), sum_gx (dgamma). `n`: the divisor (live rows unless a global count is given); `sums`: (sum_g, sum_gx) to
    apply instead of the local ones (the apply-only pass of a synchronised layer)."""
    x, scale, mean, invstd = x.double(), scale.double(), mean.double(), invstd.double()
    g = act_grad(dy, y, act, slope) if y is not None else dy.double()
    n = x.shape[0] if n is None else n
    xh = (x - mean) * invstd
    cond = (x.abs() + mean.abs()) * invstd
    sg, sgx = g.sum(0), (g * xh).sum(0)
    s_sg, s_sgx = g.abs().sum(0), (g.abs() * cond).sum(0)
    if sums is not None:
        sg_a, sgx_a, s_sg_a, s_sgx_a = sums[0].double(), sums[1].double(), sums[0].double().abs(), sums[1].double().abs()
    else:
        sg_a, sgx_a, s_sg_a, s_sgx_a = sg, sgx, s_sg, s_sgx
    dx = scale * (g - sg_a / n - xh * sgx_a / n)
    s_dx = scale.abs() * (g.abs() + s_sg_a / n + cond * sgx_a.abs() / n + xh.abs() * s_sgx_a / n)
    return {'dx': (dx, s_dx), 'dres': (g, g.abs()), 'sum_g': (sg, s_sg), 'sum_gx': (sgx, s_sgx)}


def bias_act_bwd(dy, y):
    """g = dy * (y > 0) (y None: g = dy), db = g.sum(0)."""
    g = dy.double() if y is None else torch.where(y.double() > 0, dy.double(), torch.zeros_like(dy.double()))
    return g, (g.sum(0), g.abs().sum(0))


def affine_act(x, scale, shift, res, res2, act, slope):
    """act(x * scale + shift + res) + res2."""
    pre = x.double() * scale.double() + shift.double()
    s = (x.double() * scale.double()).abs() + shift.double().abs()
    if res is not None:
        pre, s = pre + res.double(), s + res.double().abs()
    out = _act(pre, act, slope)
    if res2 is not None:
        out, s = out + res2.double(), s + res2.double().abs()
    return out, s


def _site_index(coords, n_i, mul_ninst):
    c = coords.long()
    frame = c[:, 0] // n_i
    return frame, c[:, 1], c[:, 2], frame * mul_ninst + (c[:, 0] - frame * n_i)


def gather_rows(dense, coords, n_i, mul=None):
    """out[r] = dense[frame(r), y, x] * mul[frame, inst]; dense (N, Hd, Wd, C), mul (N, n_tok, C) fp32 or None."""
    frame, y, x, tok = _site_index(coords, n_i, 0 if mul is None else mul.shape[1])
    out = dense.double()[frame, y, x]
    if mul is not None:
        out = out * mul.double().reshape(-1, mul.shape[-1])[tok]
    return out, out.abs()


def gather_rows_bwd(dout, coords, n_i, dense, mul=None):
    """-> (ddense, S), (dmul, S): ddense[frame, y, x] += dout[r] * mul[frame, inst]; dmul[frame, inst] += dout[r] * dense[frame, y, x]."""
    N, Hd, Wd, C = dense.shape
    frame, y, x, tok = _site_index(coords, n_i, 0 if mul is None else mul.shape[1])
    d = dout.double()
    pix = (frame * Hd + y) * Wd + x
    gd = d if mul is None else d * mul.double().reshape(-1, C)[tok]
    ddense = torch.zeros((N * Hd * Wd, C), dtype=torch.float64).index_add_(0, pix, gd)
    s_dd = torch.zeros((N * Hd * Wd, C), dtype=torch.float64).index_add_(0, pix, gd.abs())
    if mul is None:
        return (ddense.reshape(N, Hd, Wd, C), s_dd.reshape(N, Hd, Wd, C)), None
    gm = d * dense.double().reshape(-1, C)[pix]
    dmul = torch.zeros((mul.shape[0] * mul.shape[1], C), dtype=torch.float64).index_add_(0, tok, gm)
    s_dm = torch.zeros_like(dmul).index_add_(0, tok, gm.abs())
    return (ddense.reshape(N, Hd, Wd, C), s_dd.reshape(N, Hd, Wd, C)), (dmul.reshape(mul.shape), s_dm.reshape(mul.shape))


def scatter_plane(vals, col, coords, P, H, W, fill):
    plane = torch.full((P, H, W), float(fill), dtype=torch.float64)
    c = coords.long()
    plane[c[:, 0], c[:, 1], c[:, 2]] = vals.double()[:, col]
    return plane


def gather_plane(plane, coords, like, width):
    c = coords.long()
    out = torch.zeros((c.shape[0], width), dtype=torch.float64)
    out[:, 0] = plane.double()[c[:, 0], c[:, 1], c[:, 2]].to(like).double()
    return out


def strided_neighbors(act_coarse, act_fine, ksize=3):
    """Gather table of a stride-2 sparse conv (kind 2): rows = coarse sites o, entry k = (ky, kx) is the row of the fine site
    i = 2 o - 1 + k (per axis) when it exists and is active, else -1. numpy restatement."""
    co = np.argwhere(act_coarse).astype(np.int64)
    P, Hf, Wf = act_fine.shape
    grid = np.full(act_fine.shape, -1, np.int32)
    grid[act_fine] = np.arange(int(act_fine.sum()), dtype=np.int32)
    nbr = np.full((co.shape[0], ksize * ksize), -1, np.int32)
    for ky in range(ksize):
        for kx in range(ksize):
            iy, ix = 2 * co[:, 1] - 1 + ky, 2 * co[:, 2] - 1 + kx
            ok = (iy >= 0) & (iy < Hf) & (ix >= 0) & (ix < Wf)
            nbr[:, ky * ksize + kx] = np.where(ok, grid[co[:, 0], np.where(ok, iy, 0), np.where(ok, ix, 0)], -1)
    return nbr


def patch_bits(bits, count, H, W, y0, y1, x0, x1):
    """bits (P, H, ceil(W / 64)) int64 words, bit b of word j = column 64 j + b. count > 0: unchanged; else [y0:y1, x0:x1] of every plane set."""
    out = bits.clone()
    if count > 0:
        return out
    a = out.numpy().view(np.uint64)
    for x in range(x0, x1):
        a[:, y0:y1, x >> 6] |= np.uint64(1) << np.uint64(x & 63)
    return out


# ------------------------------------------------------------------------------------------------------------------
# k: fp32 operations on the longest path to an element (__expf and rsqrtf count 4 each). Column sums of rounded products use
# sum_k(live) = ceil(log2 live) + 8 (+ the operations behind it); test_gpu_rows.py records the measured err / (u32 S) next to these.
# ------------------------------------------------------------------------------------------------------------------
K_ADD = 1                # one addition
K_SIGMUL = 8             # __expf 4, 1 + e, reciprocal 2, times a
K_SIGMUL_BWD = 12        # sigmoid 7, 1 - s, three multiplications, one spare for the fused / unfused product order
K_DROPOUT = 2            # 1 / (1 - p), times x
K_AFFINE = 5             # x * scale, + shift, + res, leaky slope, + res2
K_GATHER = 1             # times mul (0 without: a copy)
K_LN_MEAN = 16           # x + r, 8 adds in the lane, 6 butterfly steps, times 1 / C
K_LN_RSTD = 40           # mean 16, v - mean, square, 8 + 6 adds, times 1 / C, + eps, rsqrtf 4, rounded up
K_LN_Y = 44              # rstd 40, times rstd, times gamma, + beta, one spare
K_LN_DZ = 32             # xhat 3, dy * gamma, 2 x (8 + 6) adds of the row sums shared, 2 x times 1 / C, 2 multiplies, 2 subtractions, times rstd
K_BN_MEAN = 8            # on top of the column sum: / n, the momentum blend 3, rounded up to the spare of sum_k
K_BN_SHIFT = 24          # mean, invstd, gamma * invstd, mean * scale, beta - ...: measured 1.9, between the mean and the variance family
K_BN_VAR = 48            # invstd | scale | running_var on top of the sums: centring, / n, + eps, rsqrtf 4, unbiased factor 2, blend 3 = 14 by count;
                         # measured 12.4 on the one-pass running variance (E[x^2] - E[x]^2 in fp32), so 48 + sum_k(live) >= 4 x that
K_CENSQ = 16             # centred squares on top of sum_k: the mean (sum * 1/n) 2, x - mean, square; measured 5.5 -> sum_k + 16 >= 4 x that
K_SUM_GX = 12            # sum g * xhat on top of sum_k: xhat 2, times g, slope; measured 5.1 -> sum_k + 12 >= 4 x that
K_BN_Y = 4               # on top of K_BN_SHIFT: x * scale, + shift, + res, leaky slope
K_BN_DX = 12             # on top of the two sums: xhat 2, 2 x (/ n, multiply), 2 subtractions, times scale, mask
K_XHAT = 3               # (v - mean) * rstd, times dy: the product under LayerNorm's sum dy * xhat
