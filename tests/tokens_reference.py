"""float64 references, case construction and the k constants for the instance-token kernels: the token <-> feature cross attention
(csrc/attention.hip), the token-side linear layers and the token self-attention (csrc/token_side.hip) and the mask pre-processing mg_imd_prep
(tests/test_gpu_tokens.py on the device, tests/test_tokens_reference_cpu.py on the host). Plain torch / numpy on the CPU.

Every reference takes the fp32 operands of the kernel, evaluates in `dt` (float64: the reference; float32: "what plain fp32 torch gives for the
same operation on the same inputs", the yardstick of the host proof) and returns {name: (value, S)}. S is the first-order sensitivity of the fp32
evaluation: the sum of the absolute values of the terms under every sum, carried through the chain. The comparison is rows_reference's:

    |got - ref| <= U32 * k * S        (element-wise; U32 = 2^-23, all outputs fp32)

Softmax (scores s with sensitivity S_s, over the softmax dimension): E = max S_s, P = softmax(s), S_p = P (1 + 2 E + |s - max s|): the error of a
score moves P by P times that error (numerator) and by at most P times the largest such error (denominator); |s - max s| is there because the error
of __expf grows with its argument. Masked positions have P = 0 and S = 0.

The backward passes take the probabilities the forward STORED (fp32) as an operand, like the kernels do (rows_reference treats the stored LayerNorm
statistics the same way), so their S starts from exact operands.

`fault=`: a planted defect (the host proof shows that the comparison rejects each of them by 16 x k); None: the operation itself."""
import math

import numpy as np
import torch

from rows_reference import sum_k, K_LN_Y, K_LN_MEAN, K_LN_RSTD, K_LN_DZ, K_XHAT

F64 = torch.float64
T_TOK, D_ATT = 10, 128                     # the cross attention is built for 10 tokens of width 128
RPB = 64                                   # feature rows per workgroup of the backward row passes (csrc/attention.hip)

# (B, L, NID) of the cross-attention cases: one row; fewer rows than a forward workgroup (16); exactly one; one short of / exactly / one past a backward
# workgroup (64) with the widest table the host check admits (64); three workgroups and one row; sixteen workgroups, ragged
ATTN_CASES = [(1, 1, 1), (1, 15, 3), (2, 16, 11), (1, 63, 64), (3, 64, 11), (2, 65, 64), (5, 129, 2), (2, 1000, 11)]
SA_CASES = [(1, 1, 4), (1, 10, 128), (3, 7, 100), (2, 16, 128), (2, 16, 256), (3, 5, 132)]
TL_CASES = [(1, 4, 1), (3, 12, 11), (5, 96, 100), (33, 132, 128), (9, 256, 64), (4, 128, 256), (130, 64, 200)]
# (xadd, bias, res, relu, ln): the option sets of test_gpu_kernels.py::test_token_linear_matches_torch
TL_OPTIONS = [(True, True, True, False, True), (False, True, False, True, False), (False, False, False, False, False),
              (False, True, False, False, False), (False, True, False, False, True), (True, False, False, False, False)]
PAIR_K = [64, 96, 128, 132]


def _t(t, dt):
    return None if t is None else t.detach().cpu().to(dt)


# ------------------------------------------------------------------------------------------------------------------
# k: fp32 operations on the longest path to an element, written down before the device run. sum_k(n) = ceil(log2 n) + 8 for a sum of n rounded
# terms; __expf counts 4, a reciprocal 2. L: feature rows, D: the width of a dot product, T: tokens.
# ------------------------------------------------------------------------------------------------------------------
K_SCORE = 16                               # 8 multiply-adds in the lane, 4 butterfly steps, + table, * scale = 14, rounded up
K_SOFTMAX = 8                              # on top of the scores and the sum of the exponentials: s - max, __expf 4, reciprocal 2, * inv


def k_tok_p(L):
    return K_SCORE + K_SOFTMAX + sum_k(L)


def k_tok_ctx(L):
    return k_tok_p(L) + 1 + sum_k(L)       # times F, the sum over the rows


K_G = 14                                   # dCtx . F: 8 + 4, + dP, one spare


def k_rowdot(L):
    return K_G + 1 + sum_k(L)


def k_tok_ds(L):
    return k_rowdot(L) + 3                 # G - rowdot, * P, * scale


def k_tok_dfeat(L):
    return k_tok_ds(L) + 1 + sum_k(2 * T_TOK)      # 2 T products per channel


def k_tok_dqk(L):
    return k_tok_ds(L) + 1 + sum_k(L)


def k_tok_dbtab(L):
    return k_tok_ds(L) + sum_k(L)


K_FEAT_P = K_SCORE + K_SOFTMAX + sum_k(T_TOK)                  # 36
K_FEAT_OUT = K_FEAT_P + 1 + sum_k(T_TOK + 1)                   # + T products and the bias: 49
K_FEAT_DS = 12 + 1 + sum_k(T_TOK) + 3                          # dP = dout . Vp (8 + 4), the row dot, dP - dot, * P, * scale: 28
K_FEAT_DFEAT = K_FEAT_DS + 1 + sum_k(T_TOK)                    # 41


def k_feat_dkq(L):
    return K_FEAT_DS + 1 + sum_k(L)


def k_feat_dvp(L):
    return 1 + sum_k(L)


def k_feat_db2(L):
    return K_FEAT_DS + sum_k(L)


def k_feat_dob(n):
    return sum_k(n)


def k_sa_p(T, D):
    return sum_k(D) + 1 + K_SOFTMAX + sum_k(T)


def k_sa_out(T, D):
    return k_sa_p(T, D) + 1 + sum_k(T)


def k_sa_ds(T, D):
    return sum_k(D) + 1 + sum_k(T) + 3


def k_sa_dqk(T, D):
    return k_sa_ds(T, D) + 1 + sum_k(T)


def k_sa_dv(T):
    return 1 + sum_k(T)


def k_tl_lin(K):
    return sum_k(K) + 3                    # x + xadd, the K products, + bias, + res


def k_tl_y(K, ln):
    return k_tl_lin(K) + (K_LN_Y if ln else 0)


def k_tl_stat(K, which):
    return k_tl_lin(K) + (K_LN_MEAN if which == 'mean' else K_LN_RSTD)


def k_tl_dz(ln):
    return K_LN_DZ if ln else 0


def k_tl_dx(N, ln, pair_n=None):
    return k_tl_dz(ln) + 1 + sum_k(N) + (0 if pair_n is None else 1 + sum_k(pair_n))


def k_tl_dw(R, ln):
    return k_tl_dz(ln) + 2 + sum_k(R)      # x + xadd, times dz, the sum over the rows


def k_tl_db(R, ln):
    return k_tl_dz(ln) + sum_k(R)


def k_tl_dgamma(R):
    return sum_k(R) + K_XHAT


def k_tl_dbeta(R):
    return sum_k(R)


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def _softmax(s, S_s, masked=None):
    """Softmax over the last dimension -> P, S_p (see the module docstring)."""
    if masked is not None:
        s = s.masked_fill(masked, float('-inf'))
        S_s = S_s.masked_fill(masked, 0.0)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    P = e / e.sum(-1, keepdim=True)
    E = S_s.amax(-1, keepdim=True)
    gap = torch.where(P > 0, (s - m).abs(), torch.zeros_like(s))
    return P, P * (1 + 2 * E + gap)


def _keep(L, fault, dt):
    """Weights of the feature rows under a sum over l: a planted fault drops one."""
    k = torch.ones(L, dtype=dt)
    if fault == 'drop_last_row':
        k[L - 1] = 0
    if fault == 'drop_first_row_of_last_workgroup':
        k[(L - 1) // RPB * RPB] = 0
    return k


def _ids(ids, NID, fault):
    ids = ids.detach().cpu().long()
    if fault == 'id_off_by_one':
        ids = ids.clone()
        l = ids.shape[1] // 2
        ids[0, l] = (ids[0, l] + 1) % NID
    return ids


def _scale(scale, fault):
    return scale * scale if fault == 'scale_twice' else scale


# ------------------------------------------------------------------------------------------------------------------
# tokens <- features
# ------------------------------------------------------------------------------------------------------------------
def attn_tok_fwd(qk, btab, feat, ids, scale, dt=F64, fault=None):
    """s[t,l] = (Qk[t] . F[l] + Btab[t, id[l]]) scale, P = softmax_l, ctx[t] = sum_l P[t,l] F[l] -> score, p, ctx."""
    qk, btab, feat = _t(qk, dt), _t(btab, dt), _t(feat, dt)
    B, T, _ = qk.shape
    L, NID = feat.shape[1], btab.shape[2]
    idx = _ids(ids, NID, fault)[:, None, :].expand(B, T, L)
    tb = btab.gather(2, idx)
    ft = feat.transpose(1, 2)
    s = (qk @ ft + tb) * _scale(scale, fault)
    S_s = (qk.abs() @ ft.abs() + tb.abs()) * scale
    P, S_p = _softmax(s, S_s)
    ctx = (P * _keep(L, fault, dt)) @ feat
    return {'score': (s, S_s), 'p': (P, S_p), 'ctx': (ctx, S_p @ feat.abs())}


def attn_tok_bwd(p, feat, qk, ids, dctx, dp, scale, NID, dt=F64, fault=None):
    """G = dP + dCtx . F, rowdot = sum_l P G, dS = P (G - rowdot) scale -> dfeat, dqk, dbtab (p: the stored probabilities)."""
    p, feat, qk, dctx, dp = _t(p, dt), _t(feat, dt), _t(qk, dt), _t(dctx, dt), _t(dp, dt)
    B, T, L = p.shape
    idx = _ids(ids, NID, fault)[:, None, :].expand(B, T, L)
    ft = feat.transpose(1, 2)
    G, S_G = dctx @ ft, dctx.abs() @ ft.abs()
    if dp is not None:
        G, S_G = G + dp, S_G + dp.abs()
    short = torch.ones(L, dtype=dt)
    if fault == 'rowdot_short':
        short[L - 1] = 0
    rd, S_rd = (p * G * short).sum(2, keepdim=True), (p * S_G).sum(2, keepdim=True)
    dS, S_dS = p * (G - rd) * _scale(scale, fault), p * (S_G + S_rd) * scale
    dfeat = dS.transpose(1, 2) @ qk + p.transpose(1, 2) @ dctx
    S_df = S_dS.transpose(1, 2) @ qk.abs() + p.transpose(1, 2) @ dctx.abs()
    keep = _keep(L, fault, dt)
    dqk, S_dqk = (dS * keep) @ feat, S_dS @ feat.abs()
    dbtab = torch.zeros((B, T, NID), dtype=dt).scatter_add_(2, idx, dS * keep)
    S_db = torch.zeros((B, T, NID), dtype=dt).scatter_add_(2, idx, S_dS)
    return {'dfeat': (dfeat, S_df), 'dqk': (dqk, S_dqk), 'dbtab': (dbtab, S_db)}


# ------------------------------------------------------------------------------------------------------------------
# features <- tokens
# ------------------------------------------------------------------------------------------------------------------
def _table(b2, tn, T, fault):
    """The score-bias table as (B, T, NID); given as (B, NID, T), or (B, T, NID) with tn."""
    B = b2.shape[0]
    if fault == 'other_layout':            # the same memory read in the other layout
        NID = b2.shape[2] if tn else b2.shape[1]
        return b2.reshape(B, NID, T).transpose(1, 2) if tn else b2.reshape(B, T, NID)
    return b2 if tn else b2.transpose(1, 2)


def attn_feat_fwd(feat, kq, b2, vp, obias, pad, ids, scale, tn=False, dt=F64, fault=None):
    """s[l,t] = (F[l] . Kq[t] + B2[id[l], t]) scale (padded tokens: -inf), P = softmax_t, out[l] = sum_t P[l,t] Vp[t] + obias -> out, p."""
    feat, kq, b2, vp, obias = _t(feat, dt), _t(kq, dt), _t(b2.contiguous(), dt), _t(vp, dt), _t(obias, dt)
    B, L, _ = feat.shape
    T = kq.shape[1]
    table = _table(b2, tn, T, fault)
    NID = table.shape[2]
    idx = _ids(ids, NID, fault)[:, None, :].expand(B, T, L)
    tb = table.gather(2, idx).transpose(1, 2)
    kt = kq.transpose(1, 2)
    s = (feat @ kt + tb) * _scale(scale, fault)
    S_s = (feat.abs() @ kt.abs() + tb.abs()) * scale
    masked = None
    if pad is not None and fault != 'pad_ignored':
        masked = pad.detach().cpu().bool()[:, None, :].expand(B, L, T)
    P, S_p = _softmax(s, S_s, masked)
    out, S_out = P @ vp, S_p @ vp.abs()
    if obias is not None:
        out, S_out = out + obias, S_out + obias.abs()
    return {'out': (out, S_out), 'p': (P, S_p)}


def attn_feat_bwd(dout, p, feat, kq, vp, ids, scale, NID, want_bias, tn=False, dt=F64, fault=None):
    """dP = dout . Vp, dS = P (dP - sum_t P dP) scale -> dfeat, dkq, dvp, db2 ((B, NID, T), or (B, T, NID) with tn), dob (p: the stored probabilities)."""
    dout, p, feat, kq, vp = _t(dout, dt), _t(p, dt), _t(feat, dt), _t(kq, dt), _t(vp, dt)
    B, L, T = p.shape
    idx = _ids(ids, NID, fault)[:, None, :].expand(B, T, L)
    vt = vp.transpose(1, 2)
    dP, S_dP = dout @ vt, dout.abs() @ vt.abs()
    dot, S_dot = (p * dP).sum(2, keepdim=True), (p * S_dP).sum(2, keepdim=True)
    dS, S_dS = p * (dP - dot) * _scale(scale, fault), p * (S_dP + S_dot) * scale
    keep = _keep(L, fault, dt)[:, None]
    res = {'dfeat': (dS @ kq, S_dS @ kq.abs()),
           'dkq': ((dS * keep).transpose(1, 2) @ feat, S_dS.transpose(1, 2) @ feat.abs()),
           'dvp': ((p * keep).transpose(1, 2) @ dout, p.transpose(1, 2) @ dout.abs())}
    db2 = torch.zeros((B, T, NID), dtype=dt).scatter_add_(2, idx, (dS * keep).transpose(1, 2))
    S_db2 = torch.zeros((B, T, NID), dtype=dt).scatter_add_(2, idx, S_dS.transpose(1, 2))
    res['db2'] = (db2, S_db2) if tn else (db2.transpose(1, 2), S_db2.transpose(1, 2))
    if want_bias:
        d = dout[:1] if fault == 'dob_one_batch' else dout
        res['dob'] = ((d * keep).sum((0, 1)), dout.abs().sum((0, 1)))
    return res


# ------------------------------------------------------------------------------------------------------------------
# token self-attention
# ------------------------------------------------------------------------------------------------------------------
def token_sa_fwd(q, k, v, pad, dt=F64, fault=None):
    """softmax(q k^T / sqrt(D), key padding) v -> out, p."""
    q, k, v = _t(q, dt), _t(k, dt), _t(v, dt)
    B, T, D = q.shape
    scale = 1.0 / D ** 0.5
    kt = k.transpose(1, 2)
    s, S_s = (q @ kt) * _scale(scale, fault), (q.abs() @ kt.abs()) * scale
    masked = None
    if pad is not None and fault != 'pad_ignored':
        masked = pad.detach().cpu().bool()[:, None, :].expand(B, T, T)
    P, S_p = _softmax(s, S_s, masked)
    return {'out': (P @ v, S_p @ v.abs()), 'p': (P, S_p)}


def token_sa_bwd(dout, q, k, v, prob, dt=F64, fault=None):
    dout, q, k, v, p = _t(dout, dt), _t(q, dt), _t(k, dt), _t(v, dt), _t(prob, dt)
    D = q.shape[2]
    scale = 1.0 / D ** 0.5
    vt = v.transpose(1, 2)
    dP, S_dP = dout @ vt, dout.abs() @ vt.abs()
    dot, S_dot = (p * dP).sum(2, keepdim=True), (p * S_dP).sum(2, keepdim=True)
    dS, S_dS = p * (dP - dot) * _scale(scale, fault), p * (S_dP + S_dot) * scale
    return {'dq': (dS @ k, S_dS @ k.abs()), 'dk': (dS.transpose(1, 2) @ q, S_dS.transpose(1, 2) @ q.abs()),
            'dv': (p.transpose(1, 2) @ dout, p.transpose(1, 2) @ dout.abs())}


# ------------------------------------------------------------------------------------------------------------------
# token linear: y = LN( res + act( (x + xadd) W^T + b ) )
# ------------------------------------------------------------------------------------------------------------------
def token_linear_fwd(x, W, b=None, xadd=None, res=None, relu=False, gamma=None, beta=None, eps=0.0, wt=False, dt=F64, fault=None):
    """-> y (and, with a LayerNorm, z = the pre-norm values, mean, rstd). The LayerNorm follows rows_reference.layernorm, with the sensitivity of
    its input (S_v >= |v|) in the place of |v|."""
    x, W, b, xadd, res, gamma, beta = (_t(t, dt) for t in (x, W, b, xadd, res, gamma, beta))
    Wt = W if wt else W.t()                                    # (K, N)
    xs, S_x = (x, x.abs()) if xadd is None else (x + xadd, x.abs() + xadd.abs())
    v, S_v = xs @ Wt, S_x @ Wt.abs()
    if b is not None:
        v, S_v = v + b, S_v + b.abs()
    if relu:
        v = torch.relu(v)
    if res is not None:
        v, S_v = v + res, S_v + res.abs()
    if gamma is None:
        return {'y': (v, S_v)}
    N = v.shape[1]
    div = N + 1 if fault == 'ln_divisor' else N
    mean = v.sum(1, keepdim=True) / div
    d = v - mean
    var = (d * d).sum(1, keepdim=True) / div
    rstd = torch.rsqrt(var + eps)
    mag = S_v + S_v.mean(1, keepdim=True)
    s_var = var + 2 * (d.abs() * mag).mean(1, keepdim=True)
    s_rstd = rstd + 0.5 * rstd ** 3 * s_var
    y = d * rstd * gamma + beta
    s_y = (mag * rstd + d.abs() * s_rstd) * gamma.abs() + beta.abs()
    return {'y': (y, s_y), 'z': (v, S_v), 'mean': (mean[:, 0], S_v.mean(1)), 'rstd': (rstd[:, 0], s_rstd[:, 0])}


def token_linear_bwd(dy, x, W, xadd=None, has_b=False, has_res=False, yout=None, gamma=None, z=None, mean=None, rstd=None, wt=False, dt=F64):
    """-> dx, dW, db, dres, dgamma, dbeta (the ones that exist). yout: the stored output of a ReLU layer (its mask); z, mean, rstd: the stored
    pre-norm values and row statistics of a LayerNorm layer -- operands, like in the kernel."""
    dy, x, W, xadd, gamma = (_t(t, dt) for t in (dy, x, W, xadd, gamma))
    out = {}
    g, S_g = dy, dy.abs()
    if gamma is not None:
        z, mean, rstd = _t(z, dt), _t(mean, dt)[:, None], _t(rstd, dt)[:, None]
        N = z.shape[1]
        xh = (z - mean) * rstd
        cond = (z.abs() + mean.abs()) * rstd
        dg = dy * gamma
        s1, s2 = dg.sum(1, keepdim=True) / N, (dg * xh).sum(1, keepdim=True) / N
        g = rstd * (dg - s1 - xh * s2)
        s_s2 = (dg.abs() * cond).sum(1, keepdim=True) / N
        S_g = rstd * (dg.abs() + dg.abs().sum(1, keepdim=True) / N + cond * s2.abs() + xh.abs() * s_s2)
        out['dgamma'] = ((dy * xh).sum(0), (dy.abs() * cond).sum(0))
        out['dbeta'] = (dy.sum(0), dy.abs().sum(0))
    if has_res:
        out['dres'] = (g, S_g)
    if yout is not None:
        m = (_t(yout, dt) > 0).to(dt)
        g, S_g = g * m, S_g * m
    Wn = W.t() if wt else W                                    # (N, K)
    xs, S_x = (x, x.abs()) if xadd is None else (x + xadd, x.abs() + xadd.abs())
    out['dx'] = (g @ Wn, S_g @ Wn.abs())
    dW, S_dW = g.t() @ xs, S_g.t() @ S_x
    out['dW'] = (dW.t(), S_dW.t()) if wt else (dW, S_dW)
    if has_b:
        out['db'] = (g.sum(0), S_g.sum(0))
    return out


def pair_dx(dy1, W1, dy2, W2, dt=F64, fault=None):
    """The input gradient of two plain layers that read the same x: dy1 W1 + dy2 W2."""
    dy1, W1, dy2, W2 = (_t(t, dt) for t in (dy1, W1, dy2, W2))
    times = {'pair_twice': 2, 'pair_missing': 0}.get(fault, 1)
    return dy1 @ W1 + times * (dy2 @ W2), dy1.abs() @ W1.abs() + dy2.abs() @ W2.abs()


# ------------------------------------------------------------------------------------------------------------------
# mask pre-processing (numpy restatement of maggie/network/module/instance_matte_decoder.py:131-153 and utils/utils.py:16-21)
# ------------------------------------------------------------------------------------------------------------------
def imd_prep(mask, gt, h, w, n_i):
    """mask (B, NF, n_in, h s, w s) float32, gt (B, NF, n_gt, h gs, w gs) float32 or None -> feat_ids (B, NF h w) int32, guidance (B, n_i, NF h w)
    float32 or None, valid (B, n_i) uint8.
    resizeAnyShape(use_avg_pool_binary=True): avg_pool2d with kernel = stride = s, then > 0; the position (mask * [1 .. n_in]).max over the instances;
    a slot is valid when its binary mask has any cell; the guidance is the max-pooled alpha > 0, slots from n_gt on are 0."""
    mask = np.asarray(mask, np.float32)
    B, NF, n_in = mask.shape[:3]
    s = mask.shape[-1] // w
    win = mask.reshape(B, NF, n_in, h, s, w, s)
    avg = win.sum((4, 6), dtype=np.float32) / np.float32(s * s)
    m8 = (avg > 0).astype(np.float32)                                               # (B, NF, n_in, h, w)
    pos = np.arange(1, n_in + 1, dtype=np.float32)[None, None, :, None, None]
    ids = (m8 * pos).max(2) if n_in else np.zeros((B, NF, h, w), np.float32)
    feat_ids = ids.astype(np.int32).reshape(B, NF * h * w)
    valid = np.zeros((B, n_i), np.uint8)
    valid[:, :n_in] = m8.max((1, 3, 4)) > 0 if n_in else 0
    guidance = None
    if gt is not None:
        gt = np.asarray(gt, np.float32)
        n_gt, gs = gt.shape[2], gt.shape[-1] // w
        pooled = gt.reshape(B, NF, n_gt, h, gs, w, gs).max((4, 6))                   # (B, NF, n_gt, h, w)
        guidance = np.zeros((B, n_i, NF, h, w), np.float32)
        guidance[:, :n_gt] = (pooled > 0).astype(np.float32).transpose(0, 2, 1, 3, 4)[:, :n_i]
        guidance = guidance.reshape(B, n_i, NF * h * w)
    return feat_ids, guidance, valid


# (B, NF, n_in, n_gt, n_i, h, w, s, gs); n_gt None: no ground truth (the eval path)
IMD_CASES = [
    (2, 1, 5, 5, 10, 17, 19, 1, 8),        # planes form, s = 1; 323 cells a frame: no multiple of 256; n_gt < n_i: slots from n_gt on are 0
    (1, 1, 3, 3, 10, 6, 5, 2, 8),          # planes form, s = 2; B n_i = 10: no multiple of 4
    (1, 1, 4, 4, 10, 4, 5, 8, 8),          # s = 8: the generic form with 16-byte alpha reads
    (1, 1, 4, 4, 10, 5, 6, 1, 4),          # gs = 4
    (1, 1, 4, 4, 10, 5, 6, 1, 3),          # gs = 3: scalar alpha reads
    (2, 1, 5, None, 10, 9, 7, 2, 1),       # no ground truth
    (1, 1, 0, 3, 10, 4, 4, 1, 8),          # no guidance mask at all
    (1, 1, 16, 16, 16, 5, 5, 1, 8),        # n_in = n_i = 16: every register slot of the planes form
    (2, 3, 4, 2, 10, 5, 4, 1, 8),          # three frames
]


def imd_case(B, NF, n_in, n_gt, n_i, h, w, s, gs, seed):
    """Mask values from {0, 2^-10, 0.5, 1} and alphas from {0, 2^-10, 1}, mostly 0 so that empty windows, empty slots and windows with one tiny pixel occur;
    n_gt None: no ground truth."""
    rs = np.random.RandomState(seed)
    mv = np.array([0, 2.0 ** -10, 0.5, 1], np.float32)
    q = 1 - 0.7 ** (1.0 / (s * s))                                                   # three windows in ten have a pixel, whatever their size
    mask = mv[rs.choice(4, (B, NF, n_in, h * s, w * s), p=[1 - q, q / 3, q / 3, q / 3])]
    if n_in > 1:
        mask[:, :, n_in // 2] = 0                                                    # an instance slot without any mask pixel
    gt = None
    if n_gt is not None:
        gv = np.array([0, 2.0 ** -10, 1], np.float32)
        q = 1 - 0.7 ** (1.0 / (gs * gs))
        gt = gv[rs.choice(3, (B, NF, n_gt, h * gs, w * gs), p=[1 - q, q / 2, q / 2])]
    return torch.from_numpy(mask), None if gt is None else torch.from_numpy(gt)


# ------------------------------------------------------------------------------------------------------------------
# case construction (fp32 operands on the CPU)
# ------------------------------------------------------------------------------------------------------------------
def attn_case(B, L, NID, seed=0, ids_mode='random'):
    """Operands of both cross-attention directions. Feature rows 0, L - 1 and the first row of the last backward workgroup are 4 x outliers (their
    scores then carry a visible share of the softmax, so a kernel that skips one of them cannot hide). ids_mode: 'random', 'skip' (one id that no row
    uses: id NID // 2) or 'one' (all rows on id NID - 1)."""
    g = torch.Generator().manual_seed(1000 * L + 10 * NID + B + seed)
    T, D = T_TOK, D_ATT
    rn = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    feat = rn(B, L, D)
    for l in {0, L - 1, (L - 1) // RPB * RPB}:
        feat[:, l] *= 4
    ids = torch.randint(0, NID, (B, L), generator=g, dtype=torch.int32)
    if ids_mode == 'skip' and NID > 1:
        ids = torch.where(ids == NID // 2, torch.full_like(ids, NID - 1), ids)
    if ids_mode == 'one':
        ids = torch.full_like(ids, NID - 1)
    pads = [None, torch.ones(B, T, dtype=torch.uint8), torch.zeros(B, T, dtype=torch.uint8)]
    pads[1][:, 3] = 0                                            # one valid token
    for b in range(B):                                           # differs per batch element: T - 1 - b valid tokens (at least one)
        pads[2][b, T - 1 - b % (T - 1):] = 1
    return dict(qk=rn(B, T, D), btab=rn(B, T, NID), feat=feat, ids=ids, dctx=rn(B, T, D), dp=rn(B, T, L), kq=rn(B, T, D), b2=rn(B, NID, T),
                vp=rn(B, T, D), obias=rn(D), dout=rn(B, L, D), pads=pads, scale=1.0 / math.sqrt(D), B=B, L=L, NID=NID)


def sa_case(B, T, D, seed=0):
    g = torch.Generator().manual_seed(100 * T + D + B + seed)
    q, k, v, dout = (torch.randn(B, T, D, generator=g) for _ in range(4))
    pads = [None]
    if T > 1:
        one = torch.ones(B, T, dtype=torch.bool)
        one[:, T // 2] = False
        per = torch.zeros(B, T, dtype=torch.bool)
        for b in range(B):
            per[b, T - 1 - b % (T - 1):] = True
        pads += [one, per]
    return dict(q=q, k=k, v=v, dout=dout, pads=pads)


def tl_case(R, K, N, xadd, bias, res, ln, seed=0, integer=False, wt=False):
    """Operands of one token linear layer; integer: small integers (every product sum stays far below 2^24: exact in fp32 in any order)."""
    g = torch.Generator().manual_seed(10000 * R + 100 * K + N + seed)
    if integer:
        rn = lambda *s: torch.randint(-4, 5, s, generator=g).float()          # noqa: E731
        W = rn(K, N) if wt else rn(N, K)
    else:
        rn = lambda *s: torch.randn(*s, generator=g)                          # noqa: E731
        W = (rn(K, N) if wt else rn(N, K)) / K ** 0.5
    c = dict(x=rn(R, K), W=W, xadd=rn(R, K) if xadd else None, b=rn(N) if bias else None, res=rn(R, N) if res else None, dy=rn(R, N),
             gamma=None, beta=None, eps=1e-5)
    if ln:
        c['gamma'], c['beta'] = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    return c
