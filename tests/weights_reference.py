"""float64 references, case construction and comparison helpers for the spectral-norm weight kernels (csrc/spectral_norm.hip: the per-conv
mg_spectral_norm / mg_spectral_norm_bwd and the batched pipeline behind functional.SpectralNormPlan / SpectralNormBatch). Used by
tests/test_gpu_weights.py on the device and tests/test_weights_reference_cpu.py on the host. Plain numpy in float64, no device code.

The parameter W[A][B][kh][kw] is fp32 and is viewed as the matrix [A][B * taps] (nn.Conv2d: A = Cout, B = Cin; nn.ConvTranspose2d: A = Cin,
B = Cout). One power iteration (maggie/network/module/spectral_norm.py:22-35,73-80, SpectralNorm.normalized_weight):

    t = W^T u      v' = t / (|t| + 1e-12)      s = W v'      u' = s / (|s| + 1e-12)      sigma = u' . (W v')

krsc() is W / sigma in the conv kernels' (Cout, taps, pad_in) layout with zeros in the channels [Cin, pad_in); twin() its (pad_in, taps, Cout)
permutation; dW() the gradient G / sigma - <G, W> / sigma^2 * u' v'^T in the parameter's own [A][B][taps] order.

Every reference returns a Q: the value, S -- the float64 sum of the absolute values of the terms that form each element -- and C, the error
budget (in units of u32) that the element inherits from the computed quantities it is formed from. The comparison is element-wise:

    |got - ref| <= u_out * |ref| + floor + U32 * (k * S + C)   =   u_out |ref| + floor + U32 * k * S_eff,     S_eff = S + C / k

u_out: one rounding unit of the output dtype (2^-8 bf16, 2^-10 f16, 0 for fp32), floor: 2^-24 for f16 (subnormals), U32 = 2^-23, k: the fp32
operations on the longest path to the element (the k_* functions and K_* constants at the end of this file, each next to its derivation; a
sum of n rounded products counts rows_reference.sum_k(n) = ceil(log2 n) + 8). The figure recorded as `measured` is err / (U32 * S_eff)."""
import collections
import math

import numpy as np
import torch

from rows_reference import FLOOR, U32, U_OUT, sum_k

EPS = 1e-12
OUTLIER = 16.0
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def pad8(c):
    return (c + 7) // 8 * 8


class Geom(collections.namedtuple('Geom', 'A B kh kw transposed')):
    """One weight: the parameter's shape (A, B, kh, kw) and whether it belongs to a transposed convolution."""
    __slots__ = ()

    taps = property(lambda g: g.kh * g.kw)
    Wd = property(lambda g: g.B * g.kh * g.kw)
    cin = property(lambda g: g.A if g.transposed else g.B)
    cout = property(lambda g: g.B if g.transposed else g.A)
    pad_in = property(lambda g: pad8(g.A if g.transposed else g.B))
    numel = property(lambda g: g.A * g.B * g.kh * g.kw)
    n_out = property(lambda g: g.cout * g.taps * g.pad_in)

    def __str__(g):
        return '%dx%dx%dx%d%s' % (g.A, g.B, g.kh, g.kw, 'T' if g.transposed else '')


def G_(A, B, kh, kw=None, transposed=0):
    return Geom(A, B, kh, kh if kw is None else kw, int(transposed))


# ------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_weights.py (the host file proves the comparison on exactly these)
# ------------------------------------------------------------------------------------------------------------------
# A. per-conv forward and backward: (geometry, the edge it reaches)
PER_CONV = [
    (G_(1, 1, 1), 'total = 1: one dot block, its partial parked in a one-element dW'),
    (G_(7, 3, 3), 'A < 8 row lanes, Wd = 27 < 32, Cin = 3 -> pad_in = 8, A % 4 != 0'),
    (G_(9, 5, 1), 'A = 9: the four-accumulator loop does not run, stride-8 tail of 2 and 1 rows; Wd = 5; pad_in = 8'),
    (G_(33, 20, 1), 'A = 33: one round of four accumulators, then a tail of one row in lane 0; Wd = 20; pad_in = 24'),
    (G_(57, 34, 3), 'A = 57: lane 0 takes a second round (32 + 24 < 57), the others a tail; Wd = 306 = 9 * 32 + 18 = 4 * 64 + 50; pad_in = 40'),
    (G_(64, 40, 4, transposed=1), '16 taps, transposed: dW in [Cin][Cout][taps] order, Cin = 64 unpadded'),
    (G_(20, 32, 4, transposed=1), '16 taps, transposed: padding along A (20 -> 24)'),
    (G_(300, 70, 1, 3), 'non-square taps; A = 300 > 256 and Wd = 210 < 256 in sn_norms; pad_in = 72'),
    (G_(256, 256, 3), '589 824 outputs wrap the 2048-block grid of sn_finish_kernel; all 256 dot blocks run'),
]
# B. one plan over a mixed list: (geometry, plain)
BATCH_LIST = [
    (G_(7, 3, 3), 0),
    (G_(24, 8, 3), 1),
    (G_(33, 20, 1), 0),
    (G_(17, 34, 3), 0),                       # last b tile: nb = 2 -> scalar parameter load and scalar store
    (G_(20, 32, 4, transposed=1), 0),
    (G_(64, 40, 4, transposed=1), 0),
    (G_(3, 5, 1), 1),                         # numel = 15, n_out = 24: every offset rounding
    (G_(48, 64, 1), 0),                       # fully vectorised tile
]
BATCH_NO_GRAD = 2                             # the entry of BATCH_LIST whose gradient is absent
# C. more than 256 tiles in one conv
BIG = [G_(512, 512, 4, transposed=1), G_(512, 512, 3)]
# D. the two geometries of test_batched_weight_pipeline_mixes_spectral_norm_and_plain_convs (ConvWeight(40, 64, 3), ConvWeight(64, 32, 1))
AGREE = [G_(64, 40, 3), G_(32, 64, 1)]
# E. a parameter 4 bytes into a 16-byte aligned buffer, at a vector-friendly shape
MISALIGNED = G_(48, 64, 1)


def all_geoms():
    out = [g for g, _ in PER_CONV] + [g for g, p in BATCH_LIST if not p] + BIG + AGREE + [MISALIGNED]
    return list(dict.fromkeys(out))


def seed_of(g):
    return (g.A * 1000003 + g.B * 10007 + g.kh * 101 + g.kw * 11 + g.transposed) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------------
# case construction
# ------------------------------------------------------------------------------------------------------------------
def _edges(g):
    """Boolean [A][B][taps]: the last row, the last column and the last tap (each only where there is more than one)."""
    m = np.zeros((g.A, g.B, g.taps), bool)
    if g.A > 1:
        m[-1] = True
    if g.B > 1:
        m[:, -1] = True
    if g.taps > 1:
        m[:, :, -1] = True
    return m


def make_w(g, seed=None):
    """The fp32 parameter (A, B, kh, kw): normal values, edges scaled by 16."""
    rs = np.random.RandomState(seed_of(g) if seed is None else seed)
    w = rs.standard_normal((g.A, g.B, g.taps))
    w = np.where(_edges(g), w * OUTLIER, w)
    return torch.from_numpy(w.reshape(g.A, g.B, g.kh, g.kw)).float()


def make_u(g, seed=None):
    """A normalised normal vector of A entries, fp32."""
    rs = np.random.RandomState((seed_of(g) if seed is None else seed) + 1)
    u = rs.standard_normal(g.A)
    return torch.from_numpy(u / np.linalg.norm(u)).float()


def make_v(g, seed=None):
    rs = np.random.RandomState((seed_of(g) if seed is None else seed) + 2)
    v = rs.standard_normal(g.Wd)
    return torch.from_numpy(v / np.linalg.norm(v)).float()


def make_g(g, dtype, seed=None, pad=float('nan')):
    """A gradient in the (Cout, taps, pad_in) layout, rounded through `dtype`: normal values, the parameter's edges scaled by 16, the padded
    channels [Cin, pad_in) filled with `pad`."""
    rs = np.random.RandomState((seed_of(g) if seed is None else seed) + 3)
    gp = rs.standard_normal((g.A, g.B, g.taps))
    gp = np.where(_edges(g), gp * OUTLIER, gp)
    out = np.full((g.cout, g.taps, g.pad_in), pad, np.float64)
    out[:, :, :g.cin] = gp.transpose(1, 2, 0) if g.transposed else gp.transpose(0, 2, 1)
    return torch.from_numpy(out).to(dtype)


def rounded(t, dtype):
    """What a kernel that stores `dtype` sees of t."""
    return t.to(dtype).float()


def _f64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t, np.float64)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
Q = collections.namedtuple('Q', 'value S C')


def power_iteration(W, u):
    """One power iteration from the fp32 parameter W (A, B, kh, kw) and u (A). -> dict of Q: t, v, s, u, sigma.
    Budgets (units of u32), E_x = k_x S_x + C_x:
      t_j = sum_i W_ij u_i                 S = sum_i |W_ij u_i|
      v_j = t_j / (|t| + eps)              S = |v_j|, C = E_t_j / |t| + |v_j| r_t with r_t = sum_l |t_l| E_t_l / |t|^2 (the norm's inherited part)
      s_i = sum_j W_ij v_j                 S = sum_j |W_ij v_j|, C = sum_j |W_ij| E_v_j
      u_i = s_i / (|s| + eps)              S = |u_i|, C = E_s_i / |s| + |u_i| r_s with r_s = sum_l |s_l| E_s_l / |s|^2
      sigma = u . s = |s|^2 / (|s| + eps)  S = sigma, C = sigma r_s"""
    W = _f64(W)
    A = W.shape[0]
    Wm = W.reshape(A, -1)
    Wd = Wm.shape[1]
    u = _f64(u)
    aW = np.abs(Wm)
    t = Wm.T @ u
    S_t = aW.T @ np.abs(u)
    E_t = k_t(A) * S_t
    nt = math.sqrt(float(t @ t))
    v = t / (nt + EPS)
    r_t = float(np.abs(t) @ E_t) / nt ** 2
    C_v = E_t / nt + np.abs(v) * r_t
    E_v = k_v(Wd) * np.abs(v) + C_v
    s = Wm @ v
    S_s = aW @ np.abs(v)
    C_s = aW @ E_v
    E_s = k_s(Wd) * S_s + C_s
    ns = math.sqrt(float(s @ s))
    u2 = s / (ns + EPS)
    r_s = float(np.abs(s) @ E_s) / ns ** 2
    C_u = E_s / ns + np.abs(u2) * r_s
    sigma = float(u2 @ (Wm @ v))
    return {'t': Q(t, S_t, np.zeros_like(t)), 'v': Q(v, np.abs(v), C_v), 's': Q(s, S_s, C_s), 'u': Q(u2, np.abs(u2), C_u),
            'sigma': Q(np.array([sigma]), np.array([abs(sigma)]), np.array([abs(sigma) * r_s]))}


def budget(q, k):
    """E = k S + C, the allowance of q in units of u32."""
    return k * q.S + q.C


def krsc(W, sigma, transposed, pad_in, e_sigma=0.0):
    """W / sigma as (Cout, taps, pad_in), zeros in [Cin, pad_in). e_sigma: sigma's budget (units of u32): C = |W / sigma| e_sigma / sigma."""
    W = _f64(W)
    A, B = W.shape[:2]
    Wn = W.reshape(A, B, -1) / sigma
    o = Wn.transpose(1, 2, 0) if transposed else Wn.transpose(0, 2, 1)
    out = np.zeros(o.shape[:2] + (pad_in,), np.float64)
    out[:, :, :o.shape[2]] = o
    a = np.abs(out)
    return Q(out, a, a * (e_sigma / abs(sigma)))


def twin(W, sigma, transposed, pad_in, e_sigma=0.0):
    """The (pad_in, taps, Cout) permutation of krsc(): zero rows for the padded input channels."""
    q = krsc(W, sigma, transposed, pad_in, e_sigma)
    return Q(*(np.ascontiguousarray(x.transpose(2, 1, 0)) for x in q))


def plain_krsc(W, pad_in):
    """An ordinary conv weight (Cout, Cin, kh, kw) in the (Cout, taps, pad_in) layout: a permutation, no arithmetic."""
    return krsc(W, 1.0, 0, pad_in).value


def grad_to_param(G, A, B, taps, transposed, twin_layout=False):
    """G in (Cout, taps, pad_in) order -- or, twin_layout, in (pad_in, taps, Cout) order -- back to the parameter's [A][B][taps]; the padded
    channels are dropped unread."""
    G = _f64(G)
    if twin_layout:
        G = G.transpose(2, 1, 0)
    cin = A if transposed else B
    G = G[:, :, :cin]
    return np.ascontiguousarray(G.transpose(2, 0, 1) if transposed else G.transpose(0, 2, 1))


def dW(G, W, u, v, sigma, transposed, twin_layout=False, e_u=None, e_v=None, e_sigma=0.0):
    """G / sigma - <G, W> / sigma^2 * u v^T as [A][B][taps]. u, v: the vectors AFTER the power iteration.
    S = |G| / sigma + |<G, W>| |u v| / sigma^2; C = the budget of the dot product, k_dot(n) sum |G W|, times |u v| / sigma^2, plus (when the
    kernel's own u, v, sigma differ from the ones given here by e_u, e_v, e_sigma) |dot| / sigma^2 (e_u |v| + |u| e_v) + (|G| / sigma +
    2 |dot| |u v| / sigma^2) e_sigma / sigma."""
    W = _f64(W)
    A, B = W.shape[:2]
    Wp = W.reshape(A, B, -1)
    taps = Wp.shape[2]
    Gp = grad_to_param(G, A, B, taps, transposed, twin_layout)
    u, v = _f64(u), _f64(v).reshape(B, taps)
    dot = float((Gp * Wp).sum())
    s_dot = float(np.abs(Gp * Wp).sum())
    uv = u[:, None, None] * v[None]
    val = Gp / sigma - dot / sigma ** 2 * uv
    S = np.abs(Gp) / abs(sigma) + abs(dot) * np.abs(uv) / sigma ** 2
    C = k_dot(Wp.size) * s_dot * np.abs(uv) / sigma ** 2
    if e_u is not None:
        e_u, e_v = _f64(e_u), _f64(e_v).reshape(B, taps)
        C = C + abs(dot) / sigma ** 2 * (e_u[:, None, None] * np.abs(v)[None] + np.abs(u)[:, None, None] * e_v[None])
    C = C + (np.abs(Gp) / abs(sigma) + 2 * abs(dot) * np.abs(uv) / sigma ** 2) * (e_sigma / abs(sigma))
    return Q(val, S, C)


def forward_reference(W, u, transposed, pad_in):
    """Everything one forward call writes: the power iteration, the normalised weight and its twin, with the inherited budgets."""
    A = W.shape[0]
    it = power_iteration(W, u)
    sigma = float(it['sigma'].value[0])
    e_sigma = float(budget(it['sigma'], k_sigma(A))[0])
    it['out'] = krsc(W, sigma, transposed, pad_in, e_sigma)
    it['twin'] = twin(W, sigma, transposed, pad_in, e_sigma)
    return it


def backward_reference(G, W, fwd, transposed, twin_layout=False):
    """dW for a kernel that ran on its own u', v', sigma, evaluated with the reference's (`fwd` = forward_reference(...))."""
    W_ = _f64(W)
    A, Wd = W_.shape[0], W_[0].size
    return dW(G, W, fwd['u'].value, fwd['v'].value, float(fwd['sigma'].value[0]), transposed, twin_layout,
              e_u=budget(fwd['u'], k_u(A)), e_v=budget(fwd['v'], k_v(Wd)), e_sigma=float(budget(fwd['sigma'], k_sigma(A))[0]))


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
MEASURED = {}            # what -> largest observed (err - u_out |ref| - floor) / (U32 * S_eff)


def error_ratio(got, q, k, dtype):
    """Largest err / (U32 * S_eff) left after the output rounding allowance; inf for a NaN / inf element or a miss with S_eff == 0."""
    got = _f64(got)
    ref = q.value
    if ref.size == 0:
        return 0.0
    s_eff = np.broadcast_to(q.S + q.C / k, ref.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        rest = np.abs(got - ref) - U_OUT[dtype] * np.abs(ref) - FLOOR[dtype]
        rest = np.where(np.isfinite(rest), np.maximum(rest, 0.0), np.inf)
        ratio = np.where(rest > 0, rest / (U32 * s_eff), 0.0)
    return float(ratio.max())


def close(got, q, k, dtype):
    """Element-wise |got - ref| <= u_out |ref| + floor + U32 (k S + C); False for any NaN / inf or shape mismatch."""
    if tuple(got.shape) != tuple(q.value.shape):
        return False
    return error_ratio(got, q, k, dtype) <= k


def check(got, q, k, dtype, what):
    """Assert close(); the observed ratio is recorded in MEASURED[what] (and printed when it sets a new maximum) before the assertion."""
    assert tuple(got.shape) == tuple(q.value.shape), (what, tuple(got.shape), q.value.shape)
    r = error_ratio(got, q, k, dtype)
    if r > MEASURED.get(what, -1.0):
        MEASURED[what] = r
        print('RATIO %-22s %-8s n=%-8d err/(u32*S) = %.3f (k = %s)' % (what, str(dtype).replace('torch.', ''), q.value.size, r, k))
    assert r <= k, '%s: err / (u32 S) = %g > k = %g' % (what, r, k)


def bits(t):
    """The raw bits of a tensor / array as integers (numpy)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()
    t = np.ascontiguousarray(t)
    return t.view({2: np.int16, 4: np.int32, 8: np.int64}[t.dtype.itemsize])


def padding_is_zero(out, cin):
    """True when the channels [cin, pad_in) of a (Cout, taps, pad_in) weight are exactly +0 (every bit clear)."""
    return not bits(out)[:, :, cin:].any()


def twin_padding_is_zero(out_t, cin):
    """The same for the (pad_in, taps, Cout) twin: the rows [cin, pad_in)."""
    return not bits(out_t)[cin:].any()


# ------------------------------------------------------------------------------------------------------------------
# k: fp32 operations on the longest path to an element (a reciprocal or a division counts 2, sqrtf 1). A sum of n rounded products counts
# sum_k(n) = ceil(log2 n) + 8; the + 8 holds the product and the fixed-order steps between the thread's own accumulator and the result.
# ------------------------------------------------------------------------------------------------------------------
def k_t(A):
    """t_j: a sum over the A rows."""
    return sum_k(A)


def k_norm(n):
    """|x| = sqrtf(sum of n squares): the relative error of the sum, sum_k(n), is halved by the root (rounded up), + 1 for sqrtf."""
    return (sum_k(n) + 1) // 2 + 1


def k_v(Wd):
    """v_j = t_j * (1 / (|t| + eps)): the norm, + eps, the reciprocal 2, the multiplication."""
    return k_norm(Wd) + 4


def k_s(Wd):
    """s_i = (sum_j W_ij t_j) * sv: a sum over the Wd columns, then the scale that makes it W v."""
    return sum_k(Wd) + 1


def k_u(A):
    """u_i = s'_i * (sv / (|s| + eps)), |s| = sqrtf(sum s'^2) * sv: the norm, times sv, + eps, the division 2, the multiplication."""
    return k_norm(A) + 5


def k_sigma(A):
    """sigma = |s|^2 / (|s| + eps): the norm, times sv, the square, + eps, the division 2."""
    return k_norm(A) + 5


def k_dot(n):
    """<G, W>: a sum of n products."""
    return sum_k(n)


K_OUT = 3                # W * (1 / sigma): the reciprocal 2, the multiplication (sigma's own budget arrives through C)
K_DW = 8                 # 1 / sigma 2, dot * inv * inv 2, times u, times v, g * inv, the subtraction
