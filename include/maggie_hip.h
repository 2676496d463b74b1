/* maggie_hip.h -- C ABI of libmaggie_hip.so: the MI355X (gfx950) kernels behind MaGGIe's matting hot path.
 *
 * The reference (hmchuong/MaGGIe) has no FFI layer of its own: its hot path is Python `nn.Module`s calling
 * third-party native code (cuDNN through torch, spconv, OpenCV). This header is the boundary a maintainer binds
 * instead of those calls; `maggie_amd/hip.py` is that binding (ctypes) and `maggie_amd/network/` mirrors the
 * reference's module API on top of it. Every entry point cites the reference call it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), 16-byte aligned, unless the name says host;
 *   - activations are NHWC ("rows x channels": row = (n*H + h)*W + w) in `dtype` = MG_F32, MG_BF16 or MG_F16 (every `dtype` argument below);
 *     sparse feature matrices are rows x channels with row = active-site id (sorted (batch,y,x) order);
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); kernels are asynchronous;
 *   - return value 0 = launched, <0 = argument error, >0 = hipError_t.
 */
#ifndef MAGGIE_HIP_H
#define MAGGIE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MG_F32 0
#define MG_BF16 1
#define MG_F16 3 /* IEEE half storage, fp32 accumulate: the reference's `--precision 16` (torch.cuda.amp fp16 autocast + GradScaler, engine/train.py:208,227-229) */

#define MG_ACT_NONE 0
#define MG_ACT_RELU 1
#define MG_ACT_LRELU 2

#define MG_STAT_REPLICAS 32 /* BatchNorm statistic accumulators are [MG_STAT_REPLICAS][2*C]: atomics of different blocks spread over replicas */

#define MG_MODE_CONV 0   /* src(m,tap) = (n, ho*stride - pad + ky*dil, wo*stride - pad + kx*dil)                 */
#define MG_MODE_TCONV 1  /* src(m,tap) = (n, (ho + pad - ky*dil)/stride, ...) when divisible: dgrad / ConvTranspose */
#define MG_MODE_GATHER 2 /* src(m,tap) = nbr[m*taps + tap]  (-1 = no neighbour): sparse convolutions               */

int mg_abi_version(void);
/* Declare [base, base + bytes) zero-filled with every part handed to at most one accumulator (NULL, 0: no such range). Entry points that clear an
 * accumulator with a fill launch of their own skip it for buffers inside the range -- the host's per-graph zero arena (one memset node per replay). */
int mg_set_zeroed_range(void* base, long bytes);
/* The invariant is checked: an entry point asked to clear words of the range that an earlier call already claimed fails with hipErrorAlreadyMapped
 * (208) instead of silently keeping stale sums; mg_zeroed_range_conflicts() returns (and resets) how often that happened. */
int mg_zero_claim(void* p, long bytes);
int mg_zeroed_range_conflicts(void);

/* Bit-reproducible steps. The reference trains with torch.backends.cudnn.deterministic = True, benchmark = False (tools/main.py:135-136): two
 * runs of one step give the same bits, so the active-pixel index map -- a threshold of the coarse alpha (maggie/utils/utils.py:31) -- is the same
 * run to run. mg_set_deterministic(1) (the library's default) gives this library the same property: every cross-workgroup fp32 sum (BatchNorm
 * statistics and backward sums, bias / LayerNorm gradients, the token side of the attention backward, loss sums, SpectralNorm dot products, the
 * gradient norm) is formed as "one partial per workgroup, added in index order" instead of atomicAdd. mg_set_deterministic(0) restores the atomic
 * forms. The ordered sums stage their partials in a library-owned scratch that mg_det_init(bytes) allocates on the CURRENT device (call it once,
 * outside any stream capture; entry points return -7 when it is missing or too small). The scratch is shared by all launches: issue the library's
 * kernels on ONE stream at a time (stream order also holds inside a captured graph).
 * mg_stat_rows(): rows of the [rows][2C] statistics scratch the column-statistics kernels fill (MG_STAT_REPLICAS, or MG_DET_STAT_ROWS = 1024 in
 * deterministic mode: one row per row block, added in row order by mg_bn_finalize). */
#define MG_DET_STAT_ROWS 1024
int mg_set_deterministic(int on);
int mg_get_deterministic(void);
int mg_det_init(long bytes);
/* Round 5: ONE side stream per device may run this library's BatchNorm kernels concurrently with the main stream (the encoder's shortcut branches next to
 * the backbone, maggie/network/encoder/resnet.py:167-175): register it here (NULL: none) -- it gets a slot scratch of its own (`bytes`, allocated once,
 * never moved). Outside a stream capture. */
int mg_det_side_stream(void* stream, long bytes);
int mg_stat_rows(void);
/* test hook: dst[g][c] += sum_b slots[g][b][c] in the library's fixed order ([groups][nblk][nv] fp32) */
int mg_det_reduce_test(const float* slots, int nblk, int groups, int nv, float* dst, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution (MFMA):  Y[m, yoff+co] = epi( sum_{tap,ci} X[src(m,tap), ci] * W[co, tap, ci] )
 *   epi(v): if pre_act v = act(v);  v = v*scale[co] + shift[co];  v += res;  if !pre_act v = act(v);  v += res2
 *   stats (optional, fp32 [2*Cout], pre-zeroed): per-channel sum and sum of squares of the stored Y (BatchNorm).
 * Replaces: nn.Conv2d / nn.ConvTranspose2d (+ folded BatchNorm, activation, residual add) in
 *   maggie/network/encoder/resnet.py:23-39,177-200; maggie/network/decoder/resnet.py:28-45;
 *   maggie/network/module/aspp.py:34-56; maggie/network/module/instance_matte_decoder.py:81-88,290;
 *   maggie/network/module/conv_gru.py:24-29; and spconv SubMConv2d / SparseInverseConv2d
 *   (maggie/network/decoder/resnet_inst_matt_spconv.py:69-130) in MG_MODE_GATHER.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct mg_conv_params {
    const void* x;       /* [rows_in, ldx] activations                                            */
    const void* w;       /* [Cout, R*S, Cin] weights, same dtype, Cin padded like x               */
    void* y;             /* [M, ldy] output                                                       */
    const int32_t* nbr;  /* MG_MODE_GATHER: [M, R*S] source rows, -1 = none                       */
    const float* scale;  /* [Cout] or NULL                                                        */
    const float* shift;  /* [Cout] or NULL (bias / folded BN shift)                               */
    const void* res;     /* residual, [M or M/4, ldr], same dtype, or NULL                        */
    const void* res2;    /* post-activation residual, [M, ldr2] or NULL                           */
    float* stats;        /* [MG_STAT_REPLICAS][2*Cout] fp32 (pre-zeroed) or NULL                  */
    int32_t dtype, mode;
    int32_t N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil;
    int32_t M;           /* output rows (N*Hout*Wout, or active sites)                            */
    int32_t ldx, ldy, yoff, ldr, ldr2;
    int32_t act, pre_act, res_mode; /* res_mode: 1 = same rows, 2 = residual at half resolution (nearest x2) */
    float slope;
    int32_t dw_dtype;    /* mg_conv_wgrad_ws only: dtype dW is written in (MG_F32 = 0 default; MG_BF16 / MG_F16 = the activations' 16-bit type, needs a workspace) */
    int32_t stat_mode;   /* mg_conv_fprop `stats`: 0 = [MG_STAT_REPLICAS][2*Cout] sum and sum of squares (default);
                            1 = ONE row [2*Cout], column sums only (small layers: feeds the exact two-pass variance) */
    const int32_t* m_dev; /* optional DEVICE row count (sparse head): the kernels run over min(*m_dev, M) rows, M is then the
                            capacity the buffers were sized for. The launch is a fixed, persistent grid (tiles are walked
                            grid-stride), so no host code ever needs the count: the detail stage stays free of device->host
                            reads and its launches can be captured into a hipGraph. NULL: M is the row count (dense layers). */
    /* mg_conv_fprop, optional (bnb_x != NULL): this launch computes the gradient dz arriving at the OUTPUT z = act(BN(x) [+ res]) of a
     * training BatchNorm layer (maggie/network/encoder/resnet.py:28-39 backward). The epilogue then writes g = dz * act'(z) to `y` and
     * accumulates that layer's backward reductions into `stats` (stat_mode 0 layout): stats[c] += sum g, stats[Cout + c] += sum g * xhat,
     * xhat = (x - mean) * invstd -- the separate mg_bn_bwd_reduce pass disappears. bnb_y / bnb_x: [M, bnb_ld] rows of z (NULL when the
     * layer has no activation) and x in the launch dtype; bnb_act: the layer's activation (its LeakyReLU slope is `slope`). */
    const void* bnb_y;
    const void* bnb_x;
    const float* bnb_mean;
    const float* bnb_invstd;
    int32_t bnb_act, bnb_ld;
    int32_t stat_rep;    /* rows of `stats` in stat_mode 0 (0 = MG_STAT_REPLICAS): output tile t adds to row t % stat_rep. With stat_rep >= the number of
                            output tiles (mg_conv_stat_rows) every word receives ONE addition and mg_bn_finalize adds the rows in index order: the
                            statistics are then bit-reproducible run to run (the reference runs with cudnn.deterministic = True, tools/main.py:135-136) */
    int32_t reserved0;
    /* Operand transform (round 5; conv + BatchNorm + activation as one pass in TRAINING, maggie/network/encoder/resnet.py:26-37,
     * maggie/network/decoder/resnet.py:20-45): xf_scale != NULL makes every IN-IMAGE element of `x` enter the contraction as
     *     x_eff[m, ci] = act(x[m, ci] * xf_scale[ci] + xf_shift[ci]),   act = xf_act with LeakyReLU slope xf_slope,
     * rounded to the storage type -- the value mg_affine_act would have written -- while padding (out-of-image taps) stays 0. `x` is then the RAW
     * output of the producing convolution and (xf_scale, xf_shift) the folded batch statistics of the BatchNorm layer between the two
     * convolutions (mg_bn_finalize): the normalised activation is never stored. Honoured by mg_conv_fprop (MG_MODE_CONV) and by
     * mg_conv_wgrad* (the `x` operand) for the kernel forms mg_conv_xform_ok reports; other forms return -9. */
    const float* xf_scale;
    const float* xf_shift;
    int32_t xf_act;
    float xf_slope;
    /* bnb_* launches whose BatchNorm layer never stored its activation output (operand-path BatchNorm: bnb_y == NULL although bnb_act != none): the
     * sign of the activation's argument is re-formed as bnb_x * bnb_scale + bnb_shift (the layer's folded scale | shift, as in xf_*). */
    const float* bnb_scale;
    const float* bnb_shift;
} mg_conv_params;

/* 1 when the kernel form this geometry dispatches to applies the operand transform (xf_*) in flight: which = 0 mg_conv_fprop[_ws], 1 mg_conv_wgrad*. */
int mg_conv_xform_ok(const mg_conv_params* p, int which);

int mg_conv_fprop(const mg_conv_params* p, void* stream);
/* Round 6: the 3x3 / stride-1 / pad-1 layers with Cin % 32 == 0 in the 16-bit types (forward and data gradient, with the operand transform, the
 * residual / statistics epilogue and the BatchNorm-link sums) are tried first on the producer / consumer halo-tile kernel of csrc/conv_halo3.hip
 * (reference: maggie/network/encoder/resnet.py:23-39,167-175, decoder/resnet.py:20-45). These two are A/B and experiment switches, not part of the
 * path's contract: mg_set_halo3(0) restores the round-2..5 kernel forms (returns the previous setting; environment MG_HALO3),
 * mg_set_halo3_cfg(TH, BN, NS) forces one tile form (tile rows 4 | 8, channels 32 | 64, ring depth 1 | 3 | 4, or 100 + depth = the persistent ring form that walks several tiles per workgroup -- measured, not selected by the
 * dispatch: DESIGN.md 12.1; 200 | 201 = never | always the one-slab persistent form for Cin == 32, Cout <= 32 layers, which the dispatch takes from 4 096 tiles up;
 * 0, 0, 0 = the measured dispatch). */
int mg_set_halo3(int on);
int mg_set_halo3_cfg(int th, int bn, int ns);
/* Rows of a `stats` buffer (stat_mode 0) that give every output tile of any forward kernel form its own row for an [M = N * Hout * Wout] output
 * (deterministic mode; MG_STAT_REPLICAS in atomic mode): what mg_conv_params.stat_rep must be at least, else the launch fails with -8. */
int mg_conv_stat_rows(int M, int N, int Hout, int Wout);
/* *out = the sticky error word of the cooperative single-launch kernels on the current device (mg_bn_train_bwd's one-launch form: a workgroup gave up
 * waiting for its peers -- the launch's result is then invalid); 0 = none. A host read (hipMemcpy): for tests and end-of-run checks. */
int mg_coop_error(int* out);
/* Switch mg_bn_train_bwd's one-launch form (reduce + ordered sum + apply behind a flag hand-shake; measured slower than the three launches, off by
 * default, MG_BN_COOP=1) on or off; returns the previous setting. */
int mg_set_bn_coop(int on);
/* Switch the last-arriver form of mg_bn_bwd_reduce / mg_bn_train_bwd (deterministic mode: the last row block of a channel group to finish adds the
 * partial rows in row order in its own tail, with the arithmetic of the separate ordered-sum launch -> same bits, one launch less per layer; measured
 * +30 us per layer, off by default, MG_BN_BWD_TAIL=1) on or off; returns the previous setting. */
int mg_set_bn_bwd_tail(int on);
/* Same, allowed to split the K dimension over several blocks per tile for deep layers with few output rows (M <= 8192,
 * K >= ~1152, Cout >= 64): mg_conv_fprop_workspace(p) = floats of scratch that plan needs (0: no split, identical to
 * mg_conv_fprop); partial tiles go to the workspace, a second kernel sums them and applies the epilogue (deterministic). */
long mg_conv_fprop_workspace(const mg_conv_params* p);
int mg_conv_fprop_ws(const mg_conv_params* p, float* workspace, long workspace_floats, void* stream);

/* Weight gradient:  dW[co, tap, ci] (+)= sum_m dY[m, co] * X[src(m,tap), ci]   (fp32 accumulate, atomics across
 * row splits; dW must be pre-zeroed fp32 [Cout, R*S, Cin]). Same geometry struct; `y` = dY (read), `res` unused,
 * `w` unused, `stats` = dW. Replaces cuDNN wgrad / spconv's indice_conv_backward filter gradient. */
int mg_conv_wgrad(const mg_conv_params* p, void* stream);
/* Deterministic, atomic-free variant: with `workspace` >= mg_conv_wgrad_workspace(p) floats every row split writes its own
 * partial and a second kernel reduces them; dW is then OVERWRITTEN (no pre-zeroing needed). */
long mg_conv_wgrad_workspace(const mg_conv_params* p);
int mg_conv_wgrad_ws(const mg_conv_params* p, float* workspace, long workspace_floats, void* stream);
/* Parked slab reduction: mg_conv_wgrad_park runs the weight-gradient GEMM of mg_conv_wgrad_ws WITHOUT its trailing "row-split slabs -> dW"
 * kernel and returns that reduction's descriptor; the caller keeps `workspace` alive and untouched and later hands all the descriptors of a
 * backward pass to mg_wgrad_reduce_batched: one launch (per 64 layers) instead of one per layer (~80 per training step), same arithmetic per
 * element, so dW has the same bits either way. splits == 0 in a returned descriptor: nothing was parked, dW is already complete. */
typedef struct mg_wgrad_parked {
    const float* ws;     /* the slabs: [splits][n] fp32 */
    void* dw;            /* destination, n elements of dw_dtype */
    long n;
    int32_t splits, form, dw_dtype, blocks;
} mg_wgrad_parked;
int mg_conv_wgrad_park(const mg_conv_params* p, float* workspace, long workspace_floats, mg_wgrad_parked* out, void* stream);
int mg_wgrad_reduce_batched(const mg_wgrad_parked* items, int count, void* stream);

/* Which kernel forms ran (host-side bookkeeping for tests and tools; needs no GPU). Every kernel form the convolution family compiles has an id in
 * [0, mg_conv_form_count()) and a stable name: the launcher, its integer template arguments, then the mode where the kernel is templated on it and
 * the variants it was instantiated with -- "h3<8,64,3>/CONV/res/xf", "fprop<128,64,2>/TCONV/phased", "split<128>/CONV", "split_finish",
 * "wgrad<32,64>/GATHER", "reduce_tile". The storage type is not part of the name. mg_conv_form_name writes the name (NUL-terminated, truncated to
 * `cap`) and returns its length, -1 for an unknown id. mg_conv_last_forms writes the ids, in launch order, of the kernels the calling thread's most
 * recent mg_conv_fprop[_ws], mg_conv_wgrad[_ws | _park] or mg_wgrad_reduce_batched call launched (at most `cap` of them; -1 = a form missing from the
 * list) and returns how many there were; each of those calls clears the record on entry. */
int mg_conv_form_count(void);
int mg_conv_form_name(int id, char* buf, int cap);
int mg_conv_last_forms(int* ids, int cap);


/* ---------------------------------------------------------------------------------------------------------------
 * Row x channel normalisation / activation kernels (HBM-bound, 16-byte vector accesses).
 * Replace nn.BatchNorm2d / nn.BatchNorm1d (+ ReLU / LeakyReLU(0.2) / residual add) in
 *   maggie/network/encoder/resnet.py:23-39,167-175; maggie/network/decoder/resnet.py:28-45;
 *   maggie/network/module/aspp.py:34-56; maggie/network/decoder/resnet_inst_matt_spconv.py:69-130 (BatchNorm1d over
 *   the active rows), and nn.AvgPool2d(2,2) / nn.UpsamplingNearest2d(2) (encoder/resnet.py:113, decoder:143).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct mg_rowwise_params {
    const void* x;        /* [M, ldx] pre-normalisation input (conv output)                       */
    void* y;              /* [M, ldy] (+yoff) output of the forward / saved output in backward     */
    const void* dy;       /* [M, lddy] upstream gradient (backward)                                */
    void* dx;             /* [M, lddx] gradient w.r.t. x (backward) or NULL                        */
    const void* res;      /* residual added before the activation, or NULL                         */
    const void* res2;     /* residual added after the activation, or NULL                          */
    void* dres;           /* [M, lddres] gradient of `res` (= dy * act'), or NULL                   */
    const float* scale;   /* [C] gamma*invstd (forward) / (backward)                               */
    const float* shift;   /* [C] beta - mean*gamma*invstd                                          */
    const float* mean;    /* [C] (backward)                                                        */
    const float* invstd;  /* [C] (backward)                                                        */
    float* sums;          /* [2C] backward reductions: sum g, sum g*xhat                            */
    const float* count_ptr; /* optional device scalar row count (SyncBN); else `count`               */
    int32_t dtype, M, C, H, W;
    int32_t ldx, ldy, yoff, ldr, ldr2, lddy, lddx, lddres;
    int32_t act, res_mode, mask_x_pos;
    float slope, count;
    const int32_t* m_dev; /* optional DEVICE row count (see mg_conv_params.m_dev): rows = min(*m_dev, M); BatchNorm then uses it as
                             the sample count (exact two-pass variance), NULL: M rows */
    int32_t count_mult;   /* mg_bn_train_fwd: every row stands for count_mult samples in the unbiased running-variance factor n / (n - 1)
                             (0 = 1). The decoder's skip branch (UpsamplingNearest2d(2) -> 1x1 conv -> BatchNorm, maggie/network/decoder/resnet.py:
                             143-147 of the reference) is evaluated BEFORE the up-sampling here: mean and biased variance are unchanged by the 2x2
                             replication, the reference's sample count is 4x the rows (count_mult = 4) */
    int32_t mask_from_x;  /* backward of an operand-path BatchNorm layer (round 5, mg_conv_params.xf_*): the activation output was never stored -- `y` is
                             ignored and the sign of act's argument is re-formed as x * scale + shift (needs `shift`) */
} mg_rowwise_params;

/* stats[rep][c] += sum_m x[m,c], stats[rep][C+c] += sum_m x[m,c]^2 (fp32 [MG_STAT_REPLICAS][2C], pre-zeroed) */
int mg_colstats(const void* x, int dtype, int M, int C, int ld, float* stats, void* stream);
/* batch statistics (`nrep` replicas of [2C], summed here) -> scale/shift/mean/invstd, running-stat update (momentum, unbiased var) */
/* exact two-pass variant for small M: stats[0:C] += sum, stats[C:2C] += sum (x - mean)^2 (stats [2C] must arrive zeroed) */
int mg_colstats_centered(const void* x, int dtype, int M, int C, int ld, float* stats, int have_sum, void* stream);
/* `centered` != 0: stats[C:2C] holds the centred second moment (mg_colstats_centered) instead of sum x^2 */
/* out[n] = sum over the rows of stats[nrep][n] in the library's fixed order (local statistics of a SyncBatchNorm layer before the exchange) */
int mg_stat_rows_sum(const float* stats, int nrep, int n, float* out, void* stream);
int mg_bn_finalize(const float* stats, int nrep, const float* count_ptr, float count, int C, int centered, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                   float* mean_out, float* invstd_out, void* stream);
/* Training BatchNorm(+residual+activation) behind one entry point each way (same kernels as the calls above; local statistics only):
 *   mg_bn_train_fwd: p: x, y, res*, act, slope, H, W, dtype, M, C, ld*; stats_ws: statistics scratch, [2C] floats with `exact`, else
 *                    [MG_STAT_REPLICAS][2C] (ws_zeroed != 0: the caller hands it over zeroed, e.g. a slice of a per-step zero arena;
 *                    else it is zeroed here); outs: 4C floats receiving scale | shift | mean | invstd (kept for the backward);
 *                    stats_in (or NULL): statistics already accumulated by the producing conv's epilogue -- stats_in_rows replicas
 *                    of [2C], or with `exact` one row of column sums; `exact`: two-pass variance (few rows per channel).
 *                    Updates running_mean / running_var (or NULL).
 *   mg_bn_train_bwd: p: dy, y, x, scale, mean, invstd, dx, dres, sums [2C] (zeroed here unless sums_zeroed; = dbeta | dgamma after). */
int mg_bn_train_fwd(const mg_rowwise_params* p, float* stats_ws, int ws_zeroed, float* outs, const float* stats_in, int stats_in_rows,
                    int exact, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                    void* stream);
int mg_bn_train_bwd(const mg_rowwise_params* p, int sums_zeroed, void* stream);
/* eval mode: fold running statistics into scale/shift */
int mg_bn_fold(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               float eps, float* scale, float* shift, void* stream);
/* y = act(x*scale + shift + res) + res2 */
int mg_affine_act(const mg_rowwise_params* p, void* stream);
/* BatchNorm backward: reduce (sums) then apply (dx, dres) */
int mg_bn_bwd_reduce(const mg_rowwise_params* p, void* stream);
int mg_bn_bwd_apply(const mg_rowwise_params* p, void* stream);
/* apply pass for a layer whose reductions rode on the consumer conv's data-gradient epilogue (mg_conv_params.bnb_*): p->dy holds
 * g = dy * act'(y) already, sums_rep = nrep replicas of [2C] (summed here); sums_out [2C] receives dbeta | dgamma. Needs a power-of-two
 * number of 16-byte channel chunks per row (-3 otherwise). */
int mg_bn_bwd_apply_linked(const mg_rowwise_params* p, const float* sums_rep, int nrep, float* sums_out, void* stream);
/* op 0: 2x2 average pool, 1: 2x2 sum pool (out Ho x Wo from 2Ho x 2Wo); 2: 0.25*nearest-upsample, 3: nearest-upsample
 * (out Ho x Wo from Ho/2 x Wo/2) */
int mg_pool2x2(const void* in, void* out, int dtype, int op, int N, int Ho, int Wo, int C, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Region ops on bit-packed planes (uint64 words, bit b of word j <-> pixel x = 64*j + b; rows padded to whole words).
 * Replace compute_unknown (maggie/utils/utils.py:27-55: threshold + CPU cv2.dilate with MORPH_ELLIPSE + H2D copy),
 * the rule-book side of spconv (`dummy_downscale`, maggie/network/decoder/resnet_inst_matt_spconv.py:61-66,217-218)
 * and torch.nonzero (:206). Integer work: results are bit-exact w.r.t. oracle/region.py.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_U8 2
/* mode 0: bit = (lo < a < hi); mode 1: bit = (a > 0). `a` is [P,H,W] planes of dtype MG_F32 or MG_U8. */
int mg_bits_pack(const void* a, int dtype, void* bits, int P, int H, int W, int mode, float lo, float hi, void* stream);
int mg_bits_unpack_u8(const void* bits, uint8_t* out, int P, int H, int W, void* stream);
int mg_bits_unpack_f32(const void* bits, float* out, int P, int H, int W, void* stream);   /* the same as 0.f / 1.f planes (loss weights) */
/* progressive refinement blend of `fuse` (resnet_inst_matt_spconv.py:272-290): out = bit ? a : b over fp32 planes [P][H][W] (= a*w + b*(1-w)
 * for the 0/1 weight plane the bits encode), and its backward da = bit ? dy : 0, db = bit ? 0 : dy (either may be NULL) */
int mg_bits_select(const void* bits, const float* a, const float* b, float* out, int P, int H, int W, void* stream);
int mg_bits_select_bwd(const void* bits, const float* dy, float* da, float* db, int P, int H, int W, void* stream);
/* out = dilate(in, ellipse(width)) [& andmask]; `widths` = per-plane device int32[P] (train mode) or NULL + width_all */
int mg_bits_dilate(const void* in, void* out, const void* andmask, int P, int H, int W, const int32_t* widths, int width_all,
                   void* stream);
/* SparseConv2d(k3,s2,p1) output-site rule: coarse is [P, ceil(Hf/2), ceil(Wf/2)] */
int mg_bits_downsample(const void* fine, void* coarse, int P, int Hf, int Wf, void* stream);
/* per-row exclusive scan: rowoff[P*H + 1] (rowoff[P*H] = number of active sites), wordoff[P*H*Ww] = rank of each word */
int mg_bits_rank(const void* bits, int P, int H, int W, int32_t* counts_tmp, int32_t* rowoff, int32_t* wordoff, void* stream);
/* Bounded sparse-head capacity: keep at most `cap` active sites of a level in rank order (bits cleared in place, *count clamped, *overflow set to 1
 * when sites were dropped; wordoff stays valid for the kept sites). The host raises on the sticky overflow flag at its next flag read. */
int mg_bits_truncate(void* bits, const int32_t* wordoff, int P, int H, int W, int cap, int32_t* count, int32_t* overflow, void* stream);
/* coords[R,3] = (plane, y, x) of the active sites in sorted order (== torch.nonzero) */
int mg_bits_coords(const void* bits, const int32_t* wordoff, int P, int H, int W, int32_t* coords, void* stream);
/* gather tables [R, k*k] into the (src_bits, src_wordoff) level. kind 0: submanifold k x k; kind 1: inverse conv
 * (rows fine, source coarse, tap valid iff fine = 2*coarse - 1 + tap); kind 2: strided (rows coarse, source fine) */
int mg_gather_table(const int32_t* coords, int R, int ksize, int kind, const void* src_bits, const int32_t* src_wordoff, int Hs,
                    int Ws, int32_t* nbr, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Dense <-> sparse gathers, alpha-plane kernels, input packing
 * (maggie/network/decoder/resnet_inst_matt_spconv.py:161-194,221-232,247-251,264-268,303-304,360-362;
 *  maggie/network/encoder/resnet.py:211-229).
 * ------------------------------------------------------------------------------------------------------------- */
/* out[r, yoff+c] = dense[plane/n_i, y, x, c] * (mul ? mul[plane/n_i, plane%n_i, c] : 1) */
int mg_gather_rows(const void* dense, int dtype, const int32_t* coords, int R, int n_i, int Hd, int Wd, int C, const float* mul,
                   int mul_ninst, void* out, int ldo, int yoff, void* stream);
int mg_gather_rows_bwd(const void* dout, int dtype, int ldo, int yoff, const int32_t* coords, int R, int n_i, int Hd, int Wd, int C,
                       const float* mul, int mul_ninst, const void* dense, float* ddense, float* dmul, void* stream);
/* atomic-free d(dense): each dense pixel sums the rows of the instance planes active there (bits/wordoff of that level) */
/* dmul[frame, inst, c] = sum over the rows r of plane (frame, inst) of dout[r, yoff + c] * dense[frame, y_r, x_r, c] (fp32 [N, mul_ninst, C],
 * OVERWRITTEN): the token-multiplier gradient of mg_gather_rows without atomics -- per-plane row ranges (coords sorted by plane), fixed-order sums. */
int mg_gather_rows_dmul_det(const void* dout, int dtype, int ldo, int yoff, const int32_t* coords, int R, int n_i, int N, int Hd, int Wd, int C,
                            int mul_ninst, const void* dense, float* dmul, const int32_t* r_dev, void* stream);
int mg_gather_rows_bwd_dense(const void* dout, int dtype, int ldo, int yoff, const void* bits, const int32_t* wordoff, int n_i, int N,
                             int Hd, int Wd, int C, const float* mul, int mul_ninst, void* ddense, void* stream);
/* plane[P,H,W] = fill everywhere, vals[r, col] at the active sites (SparseConvTensor.dense() - 99 trick) */
int mg_scatter_plane(const void* vals, int dtype, int ldv, int col, const int32_t* coords, int R, int P, int H, int W, float fill,
                     float* plane, void* stream);
int mg_gather_plane(const float* plane, const int32_t* coords, int R, int H, int W, void* vals, int dtype, int ldv, int col,
                    void* stream);
/* x[N,H,W,8] = [RGB, mask-ID embedding (3), 0, 0] from NCHW fp32 image, (N,n_m,Hm,Wm) masks (nearest upsampled) */
int mg_mask_embed(const float* image, const float* masks, const float* table, int N, int H, int W, int n_m, int Hm, int Wm,
                  int n_embed, void* out, int dtype, void* stream);
int mg_mask_embed_bwd(const void* dx, int dtype, const float* masks, int N, int H, int W, int n_m, int Hm, int Wm, int n_embed,
                      float* dtable, void* stream);
/* out[N,C,h*s,w*s] (fp32 planes) = (tanh(bilinear_up(in)) + 1)/2 ; `in` addressed with explicit strides */
int mg_upsample_tanh(const void* in, int dtype, long sn, long sc, long sy, long sx, int N, int C, int h, int w, int scale,
                     int apply_tanh, float* out, void* stream);
int mg_upsample_tanh_bwd(const float* dout, const float* out, long sn, long sc, long sy, long sx, int N, int C, int h, int w,
                         int scale, int apply_tanh, float* din, void* stream);
/* The same with a 0 / 1 scale per output plane (`pscale` [N*C] or NULL: `x_os8 * valid_masks`, resnet_inst_matt_spconv.py:331, without a second
 * pass over the planes) and `any_nonzero` (or NULL; a pre-zeroed int32 set to 1 when any output element is non-zero: the `x_os8.sum() == 0` test
 * of :314 without a reduction over the planes). The backward masks the gradient of the planes scaled by 0. */
int mg_upsample_tanh_ex(const void* in, int dtype, long sn, long sc, long sy, long sx, int N, int C, int h, int w, int scale,
                        int apply_tanh, float* out, const float* pscale, int32_t* any_nonzero, void* stream);
int mg_upsample_tanh_bwd_ex(const float* dout, const float* out, long sn, long sc, long sy, long sx, int N, int C, int h, int w,
                            int scale, int apply_tanh, float* din, const float* pscale, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * SpectralNorm weight preparation (maggie/network/module/spectral_norm.py:22-35,73-80): one power iteration on every
 * forward (u, v updated in place), sigma = u^T W v, and W/sigma written in the conv kernels' (Cout, taps, Cin_pad) layout.
 * W: fp32 [A][B][taps] (Conv2d: A=Cout,B=Cin; ConvTranspose2d (transposed=1): A=Cin,B=Cout). work: fp32 [B*taps + A + 4].
 * ------------------------------------------------------------------------------------------------------------- */
int mg_spectral_norm(const float* W, float* u, float* v, int A, int B, int taps, int transposed, int pad_in, void* out,
                     int out_dtype, float* work, void* stream);
/* dW = G/sigma - (<G,W>/sigma^2) u v^T ; G fp32 in the (Cout, taps, pad_in) layout; u, v, work as left by the forward */
int mg_spectral_norm_bwd(const float* G, const float* W, const float* u, const float* v, int A, int B, int taps, int transposed,
                         int pad_in, float* work, float* dW, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Instance-token <-> feature cross attention (fp32, one head, D = 128, T = 10 tokens) -- replaces the
 * nn.MultiheadAttention calls of CrossAttentionLayer (maggie/network/module/mask_attention.py:63-133) inside
 * InstanceMatteDecoder.forward (maggie/network/module/instance_matte_decoder.py:170-236). The token side (Q/K/V/out
 * projections of 10 tokens, ID position table) is folded into small matrices by the caller; these kernels make one pass
 * over the (B, L, D) feature rows per direction. ids[b,l] in [0, NID) selects the ID position row of a feature pixel.
 *   tok_fwd : S[t,l] = (qk[t].F[l] + btab[t,ids[l]])*scale; p = softmax_l S (B,T,L); ctx[t] = sum_l p F[l] (B,T,D)
 *   tok_bwd : given dctx (B,T,D) and dp (B,T,L or NULL): dqk, dbtab (B,T,NID), dfeat (B,L,D); gbuf (B,T,L), rowdot (B,T) scratch
 *   feat_fwd: S[l,t] = (F[l].kq[t] + b2[ids[l],t])*scale, -inf where pad_mask[b,t]; p = softmax_t (B,L,T);
 *             out[l] = sum_t p vp[t] + obias (B,L,D)
 *   feat_bwd: given dout: dfeat, dkq, dvp (B,T,D), db2 (B,NID,T), dobias (D or NULL)
 * Accumulated outputs are zeroed by the entry points. Returns -3 for unsupported D / T.
 * ------------------------------------------------------------------------------------------------------------- */
int mg_attn_tok_fwd(const float* qk, const float* btab, const float* feat, const int32_t* ids, int B, int T, int L, int D, int NID,
                    float scale, float* p, float* ctx, void* stream);
int mg_attn_tok_bwd(const float* p, const float* feat, const float* qk, const int32_t* ids, const float* dctx, const float* dp, int B, int T,
                    int L, int D, int NID, float scale, float* gbuf, float* rowdot, float* dqk, float* dbtab, float* dfeat, void* stream);
int mg_attn_feat_fwd(const float* feat, const float* kq, const float* b2, const float* vp, const float* obias, const uint8_t* pad_mask,
                     const int32_t* ids, int B, int T, int L, int D, int NID, float scale, float* out, float* p, void* stream);
int mg_attn_feat_bwd(const float* dout, const float* p, const float* feat, const float* kq, const float* vp, const int32_t* ids, int B, int T,
                     int L, int D, int NID, float scale, float* dfeat, float* dkq, float* dvp, float* db2, float* dobias, void* stream);
/* Round 5: b2_tn != 0 -- the score-bias table b2 and its gradient db2 are laid out (B, T, NID), the layout the token-side linear that forms the table
 * writes (no transposed copy in front of / behind the kernels). */
int mg_attn_feat_fwd_ex(const float* feat, const float* kq, const float* b2, const float* vp, const float* obias, const uint8_t* pad_mask,
                        const int32_t* ids, int B, int T, int L, int Dm, int NID, float scale, float* out, float* p, int b2_tn, void* stream);
int mg_attn_feat_bwd_ex(const float* dout, const float* p, const float* feat, const float* kq, const float* vp, const int32_t* ids, int B, int T,
                        int L, int Dm, int NID, float scale, float* dfeat, float* dkq, float* dvp, float* db2, float* dobias, int b2_tn, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused matting losses on fp32 planes [P,H,W] (maggie/network/arch/maggie.py:237-266,290-346; maggie/network/loss.py:67-191):
 * weighted L1, Sobel-gradient L1, 3-level Laplacian-pyramid L1 -- forward sums and exact backward. `flags[p]` = the
 * plane has any non-zero weight (planes with all-zero weights contribute nothing and are skipped).
 * ------------------------------------------------------------------------------------------------------------- */
int mg_plane_flags(const float* w, int P, int HW, int32_t* flags, void* stream);
/* as_float != 0: flags is float[P], 0.0 / 1.0 (a per-plane scale: `valid_masks`, resnet_inst_matt_spconv.py:320) */
int mg_plane_flags_ex(const float* w, int P, int HW, void* flags, int as_float, void* stream);
/* loss weight of the OS8 prediction (arch/maggie.py:271-281): out = [plane p of gt has a positive pixel] + (reweight && (gt or a8 in
 * [1/255, 254/255])); fp32 planes [P][HW]; flags_scratch: P int32 */
int mg_os8_weight(const float* gt, const float* a8, int P, long HW, int reweight, int32_t* flags_scratch, float* out, void* stream);
/* the same with a8 standing for a8 * pvalid[plane] (pvalid: int32 [P] 0 / 1 or NULL) */
int mg_os8_weight_ex(const float* gt, const float* a8, int P, long HW, int reweight, int32_t* flags_scratch, float* out, const int32_t* pvalid,
                     void* stream);
/* sums = 32 replicas x 16 floats (512 zeroed floats; a workgroup adds to replica `its index mod 32`: same-address atomics were the kernels' bound),
 * each replica [l1, grad, w, lap0, w0, lap1, w1, lap2, w2, ...] (accumulated by mg_loss_point_fwd / mg_pyr_lap_fwd; mg_pyr_lap_fwd takes
 * `sums + 3 + 2 * level`); the replicas are summed here -> out3 = (rec, lap, grad)
 * with the reference's normalisations (arch/maggie.py:237-262: eps 1e-8 on the L1 term; loss.py:137-191: eps 1e-6, 3-fold LapLoss);
 * mg_loss_coef: upstream gradient g3 of those three -> the five per-term coefficients the backward kernels take. */
int mg_loss_finish(const float* sums, float* out3, void* stream);
int mg_loss_coef(const float* g3, const float* sums, float* coef5, void* stream);
/* d = p - t; sums[0] += w|d|, sums[1] += |sobel(p*w) - sobel(t*w)|, sums[2] += w. `pvalid` (int32 [P] or NULL): planes with pvalid == 0 are
 * evaluated with p = 0 (`pred * valid_masks`, arch/maggie.py:112-118, folded into the loss kernels; their gradient is zero) */
int mg_loss_point_fwd(const float* p, const float* t, const float* w, const int32_t* flags, int P, int H, int W, float* d,
                      float* sums, const int32_t* pvalid, void* stream);
/* out[P,h/2,w/2] = (gauss5 (reflect) * x)[::2, ::2] */
int mg_pyr_down(const float* x, const int32_t* flags, int P, int h, int w, float* out, void* stream);
/* L = x - 4*gauss5*zero_stuff(down); sums[0] += |L|*wl, sums[1] += wl, G = wl*sign(L); wl = w0[y<<lvl, x<<lvl] */
int mg_pyr_lap_fwd(const float* x, const float* down, const float* w0, int lvl, int H0, int W0, const int32_t* flags, int P, int h,
                   int w, float* G, float* sums, void* stream);
/* r[P,h/2,w/2] = add - U^T(coef*q) ;  dd[P,h,w] = coef*q + D^T(r)   (adjoints of the pyramid's up / down operators) */
int mg_pyr_upT(const float* q, const float* coef, const float* add, const int32_t* flags, int P, int h, int w, float* r, void* stream);
int mg_pyr_downT(const float* r, const float* q, const float* coef, const int32_t* flags, int P, int h, int w, float* dd, void* stream);
/* dp = coef_rec*w*sign(p-t) + dd + coef_grad*w*SobelAdjoint(...)  (A, B: [P,H,W] scratch) */
int mg_loss_point_bwd(const float* p, const float* t, const float* w, const int32_t* flags, int P, int H, int W, const float* coef_rec,
                      const float* coef_grad, const float* dd, float* A, float* B, float* dp, const int32_t* pvalid, void* stream);

/* The whole fused-loss pipeline of S (<= 3) output scales per call (alpha_os1 / os4 / os8 of arch/maggie.py:283-300 share shape and target): scale s
 * reads p[s] and w[s] ([P][H][W] fp32 each) against the shared target t; pvalid as in mg_loss_point_fwd. Scratch buffers hold S * P planes,
 * scale-major: flags [S*P], d / G0 / dd0 / A / B / dp at (H, W), down0 / G1 / r0 / dd1 at (H/2, W/2), down1 / G2 / r1 / dd2 at (H/4, W/4), down2 / r2 at
 * (H/8, W/8); sums [S][512] accumulators, out [S][3] = (rec, lap, grad) per scale, g [S][3] their upstream gradients, coef [S][5]. H, W multiples of 8. */
int mg_matting_losses_fwd(const float* const* p, const float* t, const float* const* w, const int32_t* pvalid, int S, int P, int H, int W, int32_t* flags,
                          float* d, float* down0, float* down1, float* down2, float* G0, float* G1, float* G2, float* sums, float* out, void* stream);
int mg_matting_losses_bwd(const float* g, const float* sums, const float* const* p, const float* t, const float* const* w, const int32_t* pvalid,
                          const int32_t* flags, int S, int P, int H, int W, const float* G0, const float* G1, const float* G2, float* coef, float* r2,
                          float* dd2, float* r1, float* dd1, float* r0, float* dd0, float* A, float* B, float* dp, void* stream);

/* Batched SpectralNorm: all wrapped convolutions of a model in five launches. `descs` lives in device memory. */
typedef struct mg_sn_desc {
    const float* W;      /* fp32 parameter weight_bar, [A][B][taps]                                   */
    float* u;            /* weight_u [A]  (updated in place)                                          */
    float* v;            /* weight_v [B*taps] (updated in place)                                      */
    int64_t out_off;     /* element offset of this conv's (Cout, taps, pad_in) block in the output    */
    int64_t work_off;    /* float offset of this conv's [v (B*taps) | u (A) | scratch (4)] block      */
    int64_t dw_off;      /* float offset of this conv's gradient block (backward)                     */
    int32_t A, B, taps, transposed, pad_in;
    int32_t plain;       /* != 0: an ordinary (not spectrally normalised) conv weight: converted / transposed with sigma = 1, u and v unused;
                            its gradient comes back unchanged in the parameter's layout                      */
    int32_t k3_first, k3_count; /* this conv's run of (16 x 32) parameter tiles in items_k3: the backward adds their <G, W> partials in item order */
} mg_sn_desc;
int mg_spectral_norm_batched(const mg_sn_desc* descs, int n_conv, const int32_t* items_k1, int n1, const int32_t* items_k2, int n2,
                             const int32_t* items_k3, int n3, float* work_base, long work_floats, void* out_base, void* out_t_base,
                             int out_dtype, void* stream);   /* out_t_base (or NULL): same offsets, (Cin_pad, taps, Cout) copies for dgrad */
/* items_k1: (conv, block of 32 columns of W^T u, -, -); items_k2: (conv, group of 4 rows of W v, -, -); items_k3: (conv, a tile, b tile, -).
 * Every sum of the pipeline (W^T u, the two norms, <G, W>) is formed in a fixed order: no atomics, bit-reproducible u / v / sigma.
 * dot_part: n3 floats of scratch (per-tile partials of <G, W>). */
int mg_spectral_norm_batched_bwd(const mg_sn_desc* descs, int n_conv, const int32_t* items_k3, int n3, const void* const* Gptrs,
                                 int g_dtype, float* work_base, float* dW_base, float* dot_part, void* stream);
/* Round 5: the same with (a) per-conv destinations -- dWptrs: device array of n_conv float* (NULL entries / NULL array: dW_base + dw_off), so that
 * the gradients land in the caller's own storage (the optimizer's flat buffer) without a gather copy; (b) bit 0 of a ConvTranspose weight's
 * Gptrs entry set = that gradient is laid out like the twin, (Cin_pad, taps, Cout) -- what the role-swapped weight-gradient GEMM of a
 * transposed convolution writes -- and is read as such (no permute + copy in front). mg_spectral_norm_batched now emits the twin of ConvTranspose
 * weights as well (out_t_base). */
int mg_spectral_norm_batched_bwd_to(const mg_sn_desc* descs, int n_conv, const int32_t* items_k3, int n3, const void* const* Gptrs,
                                    int g_dtype, float* work_base, float* dW_base, float* const* dWptrs, float* dot_part, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Temporal (video) elementwise kernels. Rows x channels (NHWC) in `dtype`; rz = first gate conv's output (M, 2C) = [r | z] before
 * the sigmoid, cpre = second gate conv's output (M, C) before the tanh.
 *   mg_gru_gate_fwd : xrh (M,2C) = [x | sigmoid(r) * h]                      (maggie/network/module/conv_gru.py:24-25)
 *   mg_gru_out_fwd  : hn = (1 - sigmoid(z)) * h + sigmoid(z) * tanh(cpre)    (conv_gru.py:25-26)
 *   mg_gru_out_bwd  : from dhn: drz[:, C:], dc_pre, dh_part = dhn * (1 - z)
 *   mg_gru_gate_bwd : from dxrh: dx = dxrh[:, :C], drz[:, :C], dh_part = dxrh[:, C:] * r
 *   mg_temporal_fuse: eval-time alpha-level aggregation over frames (t-1, t, t+1) of maggie/network/arch/maggie_temp.py:34-77,
 *                     in place on fp32 planes (n_frames >= 3, P, H*W; t+1 = the LAST frame, :48, frames 1 and 2 are rewritten): thresholds the difference maps at 0.5, propagates t-1 -> t and t+1 -> t,
 *                     keeps the model's own prediction where the two disagree, then propagates t -> t+1.
 * ------------------------------------------------------------------------------------------------------------- */
int mg_gru_gate_fwd(const void* rz, const void* x, const void* h, int dtype, int M, int C, void* xrh, void* stream);
int mg_gru_gate_bwd(const void* dxrh, const void* rz, const void* h, int dtype, int M, int C, void* dx, void* drz, void* dh_part, void* stream);
int mg_gru_out_fwd(const void* rz, const void* cpre, const void* h, int dtype, int M, int C, void* hn, void* stream);
int mg_gru_out_bwd(const void* dhn, const void* rz, const void* cpre, const void* h, int dtype, int M, int C, void* drz, void* dc_pre,
                   void* dh_part, void* stream);
int mg_temporal_fuse(float* alphas, const float* prev, const float* df, const float* db, long plane_elems, int n_frames, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sparse refinement head, parameter side (maggie/network/decoder/resnet_inst_matt_spconv.py:69-130: the spconv layers' weights
 * (Cout, k, k, Cin) and biases, and inst_spec_layer's two nn.Linear). One launch converts ALL of them for a step, one launch
 * brings all their gradients back:
 *   backward == 0: src fp32 parameter (cout, taps, cin) -> dst (cout_pad, taps, cin_pad) zero padded, in `dtype`;
 *                  dst_t (or NULL) (cin_pad, taps, cout_pad), taps reversed when flip_t (input-gradient operand of a
 *                  submanifold conv). A bias is an entry with cout = taps = 1.
 *   backward != 0: src (cout_pad, taps, cin_pad) in `dtype` (NULL = no gradient) -> dst fp32 (cout, taps, cin).
 * `entries` is a HOST array (n <= MG_WB_MAX_ENTRIES); it travels in the kernel arguments.
 *   mg_bias_act_bwd: backward of a "+bias, ReLU" epilogue over rows x C: g = dy * (y > 0) (y, g NULL: no activation) and
 *                  db[c] = sum_m g[m,c] (db NULL: no bias), one pass.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_WB_MAX_ENTRIES 64
typedef struct mg_wb_entry {
    const void* src;
    void* dst;
    void* dst_t;
    int32_t cout, taps, cin, cout_pad, cin_pad, flip_t, dtype, reserved;
} mg_wb_entry;
int mg_weight_bank(const mg_wb_entry* entries, int n, int backward, void* stream);
int mg_bias_act_bwd(const void* dy, const void* y, void* g, int dtype, int M, int C, float* db, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Optimizer step of the measured train step (maggie/engine/train.py:274,281: clip_grad_norm_(0.01), AdamW of engine/optim.py:110-118)
 * over ONE flat fp32 buffer holding every trainable parameter (p, g, m, v: n floats each, n % 4 == 0, 16-byte aligned).
 * sumsq_scratch != NULL: the squared gradient norm is reduced into it first (1 device double) and, with max_norm > 0, gradients
 * are scaled by min(1, max_norm / (norm + 1e-6)) inside the update (no separate scaling pass); norm_out (or NULL) receives the norm.
 * bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t) for step t (computed by the host mirror).
 * phases: bit 0 = reduce the norm of g[0:n] into sumsq_scratch, bit 1 = update [0:n] (3 = both). Parameters that got no gradient
 * this step are skipped like torch does: the host reduces the norm over the whole buffer once (phases 1), then updates each
 * contiguous run of parameters that have one (phases 2, same scratch).
 * ------------------------------------------------------------------------------------------------------------- */
int mg_adamw_flat(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float bias_correction1, float bias_correction2_sqrt, double* sumsq_scratch, float max_norm, float* norm_out, int phases,
                  void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Input side: the tensor work of the reference's DataLoader after decoding, from uint8 buffers.
 *   mg_preprocess_image : ToTensor + Normalize (maggie/dataloader/transforms.py:720-778): in uint8 [frames][HW][3] ->
 *                         out fp32 [frames][3][HW] = (x / 255 - mean[c]) / std[c]  (IEEE divisions: bit-exact). HW % 4 == 0.
 *   mg_preprocess_planes: alpha / mask planes (transforms.py:744 `alphas < 5 -> 0`; maggie/dataloader/him.py:157-173): in uint8
 *                         [frames][n_in][H][W] -> out fp32 [frames][n_slots][Ho][Wo] = v / 255 of plane src_of_slot[frame*n_slots
 *                         + slot] (device int32; < 0 = empty slot -> zeros; NULL = identity), values below `thresh` -> 0,
 *                         sampled like F.interpolate(mode="nearest") when (Ho, Wo) != (H, W).
 * ------------------------------------------------------------------------------------------------------------- */
int mg_preprocess_image(const uint8_t* in, float* out, const float* mean3, const float* std3, long frames, long HW, void* stream);
int mg_preprocess_planes(const uint8_t* in, float* out, const int32_t* src_of_slot, int frames, int n_in, int n_slots, int H, int W,
                         int Ho, int Wo, int thresh, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Ground-truth maps of the datasets on the device (csrc/morph.hip): grey-scale morphology with OpenCV's ellipse, on uint8 planes.
 *   E = getStructuringElement(MORPH_ELLIPSE, (k, k)), anchor a = k / 2; dilate: dst[y][x] = max over E[i][j] != 0 of src[y+i-a][x+j-a],
 *   erode: the same offsets with min; pixels outside the image take no part; n iterations = the filter applied n times. All n passes
 *   of a 64 x 64 tile run out of LDS in one launch (halo n*(k/2) up / left, n*(k-1-k/2) down / right): one read of the input, one write
 *   of the product. Integer work: bit-exact, deterministic, no host synchronisation (capturable once mg_morph_prepare has run).
 *   kn: DEVICE int32 [frames][2] = (k, n) of every frame, 1 <= k <= 31, n >= 1. halo_max: the caller's bound on n * (k - 1) over the
 *   frames, 0 <= halo_max <= MG_MORPH_MAX_HALO (else -2); it sizes the LDS tile, and a frame whose table entry exceeds it is computed
 *   with k and then n clamped to the bound (never out of bounds).
 *   mg_morph_prepare   : uploads the ellipse span table to the current device (implicit in the first call of the entries below; call it
 *                        before capturing a graph).
 *   mg_morph_u8        : in u8 [planes][H][W] -> dil, ero u8 [planes][H][W] (either may be NULL); frame of a plane = plane / planes_per_frame.
 *   mg_transition_gt   : in u8 [frames][n_in][H][W] -> out fp32 [frames][n_slots][H][W]; slot s of frame f shows plane src_of_slot[f*n_slots+s]
 *                        (device int32; < 0 = empty slot -> zeros; NULL = identity, n_slots == n_in); values below `thresh` read as 0
 *                        (transforms.py:744). MG_GT_TRANSITION: [dilate > erode] (gen_transition_gt, maggie/dataloader/utils.py:15-35, as
 *                        called by him.py:185-189: its `masks` branch is dead there). MG_GT_TRIMAP: 2 where v >= 128, then 1 where
 *                        dilate > erode, else 0 (him.py:190-196, vim.py:198-203).
 *   mg_diff_transition : in u8 [T][n_in][H][W] -> out fp32 [T][n_slots][H][W] (vim.py:171-183,211): frame 0 all ones; frame t >= 1 =
 *                        [n-pass dilation of the union over instances of (|a_t - a_{t-1}| > diff_thresh)] written to every slot; values
 *                        below `thresh` read as 0. kn entry 0 is not read.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_MORPH_MAX_HALO 48
#define MG_GT_TRANSITION 0
#define MG_GT_TRIMAP 1
int mg_morph_prepare(void);
int mg_morph_u8(const uint8_t* in, uint8_t* dil, uint8_t* ero, const int32_t* kn, int halo_max, long planes, int planes_per_frame, int H, int W,
                void* stream);
int mg_transition_gt(const uint8_t* in, float* out, const int32_t* src_of_slot, const int32_t* kn, int halo_max, int frames, int n_in,
                     int n_slots, int H, int W, int thresh, int mode, void* stream);
int mg_diff_transition(const uint8_t* in, float* out, const int32_t* kn, int halo_max, int T, int n_in, int n_slots, int H, int W, int thresh,
                       int diff_thresh, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Guidance-mask synthesis of the training loaders on the device (csrc/maskgen.hip; maggie/dataloader/transforms.py:388-565:
 * GenMaskFromAlpha -> RandomBinarizedMask -> DownUpMask -> CutMask -> MaskDropout). uint8 planes [planes][H][W], H * W < 2^31 (else -2);
 * every table is DEVICE int32 and is read by the kernel, so a captured launch follows draws written into it between replays. Integer
 * work: bit-exact, deterministic. No entry synchronises with the host.
 *   mg_mask_morph : out = 255 * morph(in > thr). params [planes][4] = (thr, k_dilate, k_erode, order): thr = floor of the reference's float
 *                   threshold (cv2.threshold(THRESH_BINARY) on 8-bit data is v > floor(t)); cv2.dilate / cv2.erode with np.ones((k, k)),
 *                   anchor a = k / 2: dst[y][x] = max (min) over 0 <= i, j < k of src[y+i-a][x+j-a], pixels outside the image take no part,
 *                   also between the two passes; 1 <= k <= MG_MASK_MAX_K (the host raises beyond; the kernel clamps); order MG_MASK_*
 *                   below, MG_MASK_NONE = threshold only (GenMaskFromAlpha is thr = 127 with MG_MASK_NONE). One launch for all planes;
 *                   threshold and both passes run on a bit-packed tile in LDS.
 *   mg_mask_downup: where apply[p] != 0: cv2.resize(INTER_LINEAR) to (dh, dw), cv2.resize(INTER_LINEAR) back to (H, W), then 255 * (v > 127);
 *                   other planes are copied. Any uint8 input. tab = [dw][3] | [dh][3] | [W][3] | [H][3] rows of (offset, c0, c1): the taps
 *                   `offset` and `offset + 1` (clamped to the last index) and OpenCV's coefficients scaled by 2048, for the columns and rows
 *                   of the small image and then of the output; horizontal pass row = S0 * c0 + S1 * c1 in int32, vertical pass
 *                   (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2. The offsets are non-decreasing and a 64-pixel run of the
 *                   output reads at most MG_MASK_MAX_PATCH of the small image (scale ratio <= 1; the host builds and checks the tables:
 *                   maggie_amd/utils/maskgen.py resize_tables). The small image stays in LDS. `out` must not alias `in`.
 *   mg_mask_cut   : out = in with, per plane p, the h x w rectangle at (dst_row, dst_col) replaced by the one at (src_row, src_col) of plane
 *                   src_plane of `in`. rects [planes][8] = (src_plane, dst_row, dst_col, src_row, src_col, h, w, 0); src_plane < 0 (or a
 *                   rectangle that leaves the plane) = untouched. CutMask.internal is src_plane = p; .external is two entries naming each
 *                   other with the same rectangle. Out of place (in == out: -2), so overlapping rectangles read the old values.
 *   mg_mask_stats : stats [planes][5] = (count, xmin, xmax, ymin, ymax) of the non-zero pixels; an empty plane gives (0, W, -1, H, -1).
 *   mg_mask_drop  : in place, entry e of sel [n][4] = (plane, idx, ph, pw): (x, y) = the idx-th non-zero pixel of the plane in raster order;
 *                   x = min(x, xmax - pw), y = min(y, ymax - ph) (not below 0) with this plane's row of `stats`; zero [y, y+ph) x [x, x+pw)
 *                   (MaskDropout, transforms.py:557-563). plane < 0, idx outside the plane's count, ph <= 0 or pw <= 0 = skipped. The
 *                   entries name distinct planes.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_MASK_MAX_K 31
#define MG_MASK_MAX_PATCH 66
#define MG_MASK_DILATE_ERODE 0
#define MG_MASK_ERODE_DILATE 1
#define MG_MASK_DILATE 2
#define MG_MASK_ERODE 3
#define MG_MASK_NONE 4
int mg_mask_morph(const uint8_t* in, uint8_t* out, const int32_t* params, long planes, int H, int W, void* stream);
int mg_mask_downup(const uint8_t* in, uint8_t* out, const int32_t* apply, const int32_t* tab, int dh, int dw, long planes, int H, int W,
                   void* stream);
int mg_mask_cut(const uint8_t* in, uint8_t* out, const int32_t* rects, long planes, int H, int W, void* stream);
int mg_mask_stats(const uint8_t* in, int32_t* stats, long planes, int H, int W, void* stream);
int mg_mask_drop(uint8_t* planes_u8, const int32_t* sel, const int32_t* stats, int n, long planes, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Input geometry on the device (csrc/geometry.hip; maggie/dataloader/transforms.py:104-166, ResizeShort -> PaddingMultiplyBy): cv2.resize of
 * uint8 images with the padding and the tensor stage fused into the same launch. Integer work and IEEE divisions: bit-exact.
 *   mg_resize_u8 : in uint8 [images][H][W][channels] (channels 1 or 3) -> an (Ho, Wo) output per image whose cells (y < dh, x < dw) hold
 *                  the resized image and whose other cells are the padding: the value a source pixel of 0 would have given.
 *                  interp MG_RESIZE_LINEAR : xtab [dw][3], ytab [dh][3] DEVICE int32 rows of (offset, c0, c1) as in mg_mask_downup -- taps
 *                    `offset` and `offset + 1` (clamped to the last index), OpenCV's 11-bit coefficients; the same column table for every
 *                    channel; row = S0 * c0 + S1 * c1 in int32, then (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2.
 *                  interp MG_RESIZE_NEAREST: xtab [dw], ytab [dh] DEVICE int32 source indices (cv2.INTER_NEAREST, or any composition of
 *                    index maps: the mask path folds the resize, the padding and the loaders' nearest 1/8 down-scale into one table).
 *                  The tables are built on the host (maggie_amd/utils/geometry.py); every index read from them is clamped to the source.
 *                  epilogue MG_RESIZE_RAW  : out uint8 [images][Ho][Wo][channels].
 *                           MG_RESIZE_NORM : channels 3; out fp32 [images][3][Ho][Wo] = (v / 255 - mean[c]) / std[c] (the expression of
 *                                            mg_preprocess_image, shared through csrc/pixel_norm.h); no uint8 intermediate.
 *                           MG_RESIZE_SLOTS: channels 1; `images` frames of n_in planes -> out fp32 [images][n_slots][Ho][Wo] = v / 255 of
 *                                            plane src_of_slot[frame * n_slots + slot] (DEVICE int32; < 0 = empty slot -> zeros; NULL =
 *                                            identity, n_slots == n_in), values below `thresh` -> 0: mg_preprocess_planes' contract.
 *                  regime (linear only) MG_RESIZE_SHARED_ROWS: the horizontal pass of the source rows of a MG_RESIZE_TILE_ROWS x
 *                    MG_RESIZE_TILE_COLS output tile runs once into LDS (uint16 per channel and column), the vertical pass reads it; legal
 *                    when no tile reads more than MG_RESIZE_MAX_ROWS source rows (the host checks its row table; the kernel clamps).
 *                    MG_RESIZE_DIRECT: four global taps per output pixel, four pixels per lane: any ratio. Both give the same bits.
 *                  Returns -2 for an argument error (before any launch), -3 when the launch would exceed a grid dimension.
 *   mg_resize_limits: the tile and LDS row budget of the shared-rows regime, for the host's choice.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_RESIZE_LINEAR 0
#define MG_RESIZE_NEAREST 1
#define MG_RESIZE_RAW 0
#define MG_RESIZE_NORM 1
#define MG_RESIZE_SLOTS 2
#define MG_RESIZE_SHARED_ROWS 0
#define MG_RESIZE_DIRECT 1
#define MG_RESIZE_TILE_ROWS 32
#define MG_RESIZE_TILE_COLS 64
#define MG_RESIZE_MAX_ROWS 68
int mg_resize_u8(const uint8_t* in, void* out, const int32_t* xtab, const int32_t* ytab, const int32_t* src_of_slot, long images, int n_in,
                 int n_slots, int channels, int H, int W, int dh, int dw, int Ho, int Wo, int interp, int epilogue, int regime,
                 const float* mean3, const float* std3, int thresh, void* stream);
int mg_resize_limits(int* tile_rows, int* tile_cols, int* max_rows);

/* ---------------------------------------------------------------------------------------------------------------
 * Training crop on the device (csrc/crop.hip; maggie/dataloader/transforms.py:191-305, RandomCropByAlpha -> RandomHorizontalFlip, between
 * PaddingMultiplyBy and the mask chain). uint8 in; integer work and the IEEE divisions of csrc/pixel_norm.h: bit-exact. The draws stay on the
 * host (maggie_amd/utils/crop.py); the kernels read them from DEVICE int32 tables, so a captured launch follows draws written between replays.
 *   mg_crop_bbox     : alphas uint8 [planes][H][W] -> box [5] = (count, xmin, xmax, ymin, ymax) of the pixels whose sum over all planes exceeds
 *                      127 * planes (`alphas.mean(0) > 127` as an integer test); no such pixel gives (0, W, -1, H, -1). Rows are split over
 *                      many workgroups: per-workgroup extremes in LDS, then integer atomics on the five words (which the entry initialises
 *                      on the stream first). planes <= MG_CROP_MAX_PLANES.
 *   mg_crop_hits     : hits [n] = 1 where any plane holds a value > 127 inside window k = [y0, y0 + ch) x [x0, x0 + cw), windows [n][2] =
 *                      (x0, y0), n <= MG_CROP_MAX_WINDOWS; otherwise 0. Reads the windows only.
 *   mg_crop_gather   : out pixel (y, x) of image i = in pixel (y0 + y, x0 + x), or (y0 + y, x0 + cw - 1 - x) when flip != 0; window [3] =
 *                      (x0, y0, flip), one for all images, clamped to the source. in uint8 [images][H][W][channels] (channels 1 or 3).
 *                      lut (channels 3 only, or NULL): DEVICE uint8 [3][256], v = lut[c][v] after the gather and before the epilogue.
 *                      epilogue MG_CROP_RAW : out uint8 [images][ch][cw][channels];
 *                               MG_CROP_NORM: channels 3; out fp32 [images][3][ch][cw] = (v / 255 - mean[c]) / std[c], the bits of
 *                                             mg_preprocess_image on the uint8 crop.
 *                      A lane owns MG_CROP_CHUNK pixels of one output row: 16-byte stores when cw is a multiple of it, per element otherwise.
 *   mg_crop_padresize: the padding branch: cv2.resize of the image padded with zeros by (pad_h, pad_w) on both sides to (dh, dw). The tables
 *                      are those of mg_resize_u8 (linear xtab [dw][3], ytab [dh][3]; nearest xtab [dw], ytab [dh]) in PADDED coordinates;
 *                      the kernel subtracts the pads and reads 0 outside the source. A flip is a reversed column table. Epilogues and lut as
 *                      in mg_crop_gather with (ch, cw) = (dh, dw).
 * Each returns -2 for an argument error (before any launch), -3 when the launch would exceed a grid dimension.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_CROP_RAW 0
#define MG_CROP_NORM 1
#define MG_CROP_MAX_WINDOWS 3
#define MG_CROP_MAX_PLANES (1 << 22)
#define MG_CROP_CHUNK 16
int mg_crop_bbox(const uint8_t* alphas, int32_t* box, long planes, int H, int W, void* stream);
int mg_crop_hits(const uint8_t* alphas, const int32_t* windows, int32_t* hits, int n, long planes, int H, int W, int ch, int cw, void* stream);
int mg_crop_gather(const uint8_t* in, void* out, const int32_t* window, const uint8_t* lut, long images, int channels, int H, int W, int ch,
                   int cw, int epilogue, const float* mean3, const float* std3, void* stream);
int mg_crop_padresize(const uint8_t* in, void* out, const int32_t* xtab, const int32_t* ytab, const uint8_t* lut, long images, int channels,
                      int H, int W, int pad_h, int pad_w, int dh, int dw, int interp, int epilogue, const float* mean3, const float* std3,
                      void* stream);
int mg_crop_limits(int* max_windows, int* max_planes, int* chunk);

/* ---------------------------------------------------------------------------------------------------------------
 * RandomAffine on the device (csrc/affine.hip; maggie/dataloader/transforms.py:926-963 with dataloader/utils.py:61-221: cv2.warpAffine of
 * every frame and alpha plane of an item, then the float64 channel shift of the frames). uint8 in; the warp is integer work only, the shift is
 * the reference's float64 add and clamp followed by the IEEE divisions of csrc/pixel_norm.h: bit-exact. The draws, the matrix, its inversion
 * and the tables stay on the host (maggie_amd/utils/affine.py); the kernels read DEVICE buffers, so a captured launch follows draws written
 * between replays.
 *   tab              : DEVICE int32 [adelta W | bdelta W | X0 H | Y0 H], OpenCV's AB_BITS = 10 tables of the INVERSE map for an (H, W)
 *                      destination of the source's size: adelta[x] = cvRound(M0 * x * 1024), bdelta[x] = cvRound(M3 * x * 1024),
 *                      X0[y] = cvRound((M1 * y + M2) * 1024) + round_delta, Y0[y] likewise with M4, M5; round_delta 512 (nearest) or 16
 *                      (linear). Sums wrap; every index derived from a table is range-tested: a wrong table gives zeros or wrong pixels.
 *   mg_affine_warp_planes     : INTER_NEAREST, BORDER_CONSTANT 0, in / out uint8 [planes][H][W]: out(y, x) = in(sy, sx), sx = (X0[y] +
 *                      adelta[x]) >> 10, sy = (Y0[y] + bdelta[x]) >> 10 (arithmetic shifts), 0 when the tap is outside.
 *   mg_affine_warp_frames     : INTER_LINEAR, BORDER_CONSTANT 0, in / out uint8 [frames][H][W][3]: X = (X0[y] + adelta[x]) >> 5, sx = X >> 5,
 *                      fx = X & 31 (y likewise); out = (sum of the four taps times 32 * (32 - fx) * (32 - fy) ... + 16384) >> 15, each tap
 *                      outside the image 0 on its own. minmax int32 [frames][2]: each output frame's min and max over pixels and channels
 *                      (integer atomics; the entry initialises the words on the stream first).
 *                      regime MG_AFFINE_STAGED: a MG_AFFINE_TILE_ROWS x MG_AFFINE_TILE_COLS output tile copies its source box (from the
 *                      table values at the tile's corners, cut to the image) into LDS when it fits MG_AFFINE_BOX_BYTES and reads its taps
 *                      there; other taps and larger boxes read global memory. MG_AFFINE_DIRECT: four global taps per pixel. Same bits.
 *   mg_affine_shift_normalize : in uint8 [frames][H][W][3] -> out fp32 [frames][3][H][W] = ((float)clamp((double)v + *intensity, min, max) /
 *                      255 - mean[c]) / std[c] with min / max = minmax[frame] (channel_shift in float64, ToTensor's .float(), Normalize).
 *                      intensity: DEVICE double.
 * Each returns -2 for an argument error (before any launch; H, W <= MG_AFFINE_MAX_SIDE as in OpenCV's fixed-point path), -3 when the launch
 * would exceed a grid dimension.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_AFFINE_STAGED 0
#define MG_AFFINE_DIRECT 1
#define MG_AFFINE_TILE_ROWS 32
#define MG_AFFINE_TILE_COLS 64
#define MG_AFFINE_BOX_BYTES 16384
#define MG_AFFINE_MAX_SIDE 32767
int mg_affine_warp_planes(const uint8_t* in, uint8_t* out, const int32_t* tab, long planes, int H, int W, void* stream);
int mg_affine_warp_frames(const uint8_t* in, uint8_t* out, const int32_t* tab, int32_t* minmax, long frames, int H, int W, int regime,
                          void* stream);
int mg_affine_shift_normalize(const uint8_t* in, float* out, const int32_t* minmax, const double* intensity, long frames, int H, int W,
                              const float* mean3, const float* std3, void* stream);
int mg_affine_limits(int* tile_rows, int* tile_cols, int* box_bytes, int* max_side);

/* ---------------------------------------------------------------------------------------------------------------
 * The photometric steps of the training stream on the device (csrc/photometric.hip; maggie/dataloader/transforms.py:812-924, him.py:46-48,
 * vim.py:51-54): a per-channel tone curve, additive noise, and the JPEG round trip of JpegCompression -- the lossy part of libjpeg-turbo at
 * Pillow's defaults (baseline, 4:2:0, JDCT_ISLOW, fancy upsampling) without the lossless entropy coding. uint8 in, int32 arithmetic: bit-exact.
 * Every table is a DEVICE buffer, so a captured launch follows values written between replays.
 *   lut              : uint8 [3][256] or NULL: channel c of a pixel becomes lut[c][v], first.
 *   noise            : int16 [h][w][noise_channels] or NULL, noise_channels 1 (one sample per pixel) or 3: v = clamp(v + noise, 0, 255), after
 *                      `lut`; the same plane for every frame.
 *   qtab             : int32 [2][64], the luma and chroma quantisation tables in natural order, 1..255 (other values are clamped to that).
 *   mg_jpeg_ycc      : in uint8 [frames][h][w][3] -> `planes`: the DECODED component planes Y uint8 [frames][h16][w16], then Cb, then Cr
 *                      [frames][h16 / 2][w16 / 2] (h16, w16 = h, w rounded up to 16; frames * h16 * w16 * 3 / 2 bytes, 16-byte aligned): lut,
 *                      noise, RGB -> YCbCr, the encoder's edge replication, h2v2 downsampling, forward DCT, quantisation, dequantisation,
 *                      inverse DCT, clamp. A workgroup of MG_JPEG_THREADS lanes owns a MG_JPEG_TILE_ROWS x MG_JPEG_TILE_COLS tile of MCUs.
 *   mg_jpeg_rgb      : `planes` -> out: triangle upsampling of Cb / Cr over the real ceil(h / 2) x ceil(w / 2) samples (2 x 2 replication
 *                      when ceil(w / 2) <= 2), YCbCr -> RGB, clamp. epilogue MG_PHOTO_RAW: out uint8 [frames][h][w][3]; MG_PHOTO_NORM: out fp32
 *                      [frames][3][h][w] = (v / 255 - mean[c]) / std[c], the bits of mg_preprocess_image on the raw result. A lane owns 16
 *                      pixels of a row: 16-byte stores when w is a multiple of 16 and `out` is 16-byte aligned, per element otherwise.
 *   mg_photo_noise   : `lut` and / or `noise` alone (either may be NULL), in uint8 [frames][h][w][3] -> out with the same two epilogues.
 * Each returns -2 for an argument error (before any launch; h, w <= MG_JPEG_MAX_SIDE), -3 when the launch would exceed a grid dimension.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_PHOTO_RAW 0
#define MG_PHOTO_NORM 1
#define MG_JPEG_TILE_ROWS 32
#define MG_JPEG_TILE_COLS 64
#define MG_JPEG_THREADS 384
#define MG_JPEG_MAX_SIDE 32767
int mg_jpeg_ycc(const uint8_t* in, uint8_t* planes, const uint8_t* lut, const int16_t* noise, int noise_channels, const int32_t* qtab, long frames,
                int h, int w, void* stream);
int mg_jpeg_rgb(const uint8_t* planes, void* out, long frames, int h, int w, int epilogue, const float* mean3, const float* std3, void* stream);
int mg_photo_noise(const uint8_t* in, void* out, const uint8_t* lut, const int16_t* noise, int noise_channels, long frames, int h, int w,
                   int epilogue, const float* mean3, const float* std3, void* stream);
int mg_jpeg_limits(int* tile_rows, int* tile_cols, int* threads, int* max_side);

/* ---------------------------------------------------------------------------------------------------------------
 * MotionBlur of the video training stream on the device (csrc/motion.hip; maggie/dataloader/transforms.py:965-1034, vim.py:52): the kernel
 * albumentations draws is one 8-connected line of n <= 49 ones in a ksize x ksize box (ksize odd, 3..49) divided by n, so every plane is
 *   out[y][x] = rhe( sum_k src[r101(y + dy_k, h)][r101(x + dx_k, w)] / n )
 * with (dy_k, dx_k) the offsets of the line's pixels from the anchor ksize / 2 (correlation, no flip), r101 OpenCV's BORDER_REFLECT_101
 * (0 for a length of 1; repeated for sources smaller than the reach) and rhe round-half-to-even of the exact rational: integer work only.
 *   taps             : DEVICE int32 [MG_MOTION_TABLE]: [0] = n, [1] = ksize, then n (dy, dx) pairs in the kernel's row-major order. The launch
 *                      geometry does not depend on it; the kernel clamps n to 1..MG_MOTION_MAX_TAPS and every offset to +-MG_MOTION_MAX_KSIZE / 2
 *                      and reads 2 + 2 n entries, so a captured launch follows a table rewritten between replays and no table can send a read
 *                      outside the LDS tile.
 *   mg_motion_frames : in uint8 [frames][h][w][3] -> out uint8 in the same layout (MG_PHOTO_RAW) or fp32 [frames][3][h][w] =
 *                      (v / 255 - mean[c]) / std[c] (MG_PHOTO_NORM), the bits of mg_preprocess_image on the raw result.
 *   mg_motion_planes : uint8 [planes][h][w] in and out.
 * A workgroup of MG_MOTION_THREADS lanes owns MG_MOTION_TILE_ROWS x MG_MOTION_TILE_COLS output pixels. Each returns -2 for an argument error
 * (before any launch; h, w <= MG_MOTION_MAX_SIDE, in != out), -3 when the launch would exceed a grid dimension.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_MOTION_MAX_KSIZE 49
#define MG_MOTION_MAX_TAPS 49
#define MG_MOTION_TABLE (2 + 2 * MG_MOTION_MAX_TAPS)
#define MG_MOTION_TILE_ROWS 32
#define MG_MOTION_TILE_COLS 64
#define MG_MOTION_THREADS 256
#define MG_MOTION_MAX_SIDE 32767
int mg_motion_frames(const uint8_t* in, void* out, const int32_t* taps, long frames, int h, int w, int epilogue, const float* mean3,
                     const float* std3, void* stream);
int mg_motion_planes(const uint8_t* in, uint8_t* out, const int32_t* taps, long planes, int h, int w, void* stream);
int mg_motion_limits(int* max_ksize, int* max_taps, int* tile_rows, int* tile_cols, int* table_len, int* max_side);

/* ---------------------------------------------------------------------------------------------------------------
 * Compositing (csrc/compose.hip): Pillow's Image.resize / Image.paste and the occlusion bookkeeping of tools/synthesize_image_him.py and
 * tools/synthesize_video_him.py on uint8 data, exact. `ps` = bytes per pixel: 1 (planes) or 3 (interleaved frames).
 *   mg_compose_resize    : src uint8 [n][src_h][src_w][ps], the crop (cx, cy, cw, ch) of every image -> out uint8 [n][out_h][out_w][ps]. xtab / ytab:
 *                          DEVICE int32 [out_w][MG_COMPOSE_TAB_HEADER + kx] / [out_h][.. + ky], a row = (first source index, tap count, 0, 0, taps in
 *                          2^-22 units, zeros up to kx); kx, ky multiples of 4, tables 16-byte aligned. NULL = that pass is a copy (its size must
 *                          not change). Pass: clip8((2^21 + sum in * tap) >> 22), horizontal first, a byte between the passes. regime
 *                          MG_COMPOSE_FUSED: one launch, the horizontal results of a tile's source rows as bytes in LDS (the host promises at most
 *                          MG_COMPOSE_MAX_ROWS rows per MG_COMPOSE_TILE_ROWS output rows; the kernel clamps); MG_COMPOSE_TWO_PASS: two launches
 *                          through tmp (n * ch rows of out_w * ps rounded up to 16 bytes, 16-byte aligned; unused without ytab). Same bytes. Every
 *                          table entry is clamped to the source, so a captured launch follows tables rewritten between replays.
 *   mg_compose_paste     : dst [dst_h][dst_w][ps] <- src [src_h][src_w][ps] at (x, y), clipped to dst; mask [src_h][src_w] or NULL (a copy):
 *                          t = dst (255 - m) + src m + 128, ((t >> 8) + t) >> 8.
 *   mg_compose_try_place : planes [>= n_prev][h][w] of fp32 / fp64 (dtype), a uint8 [ha][wa] placed at (x, y) (clipped), lut [256] = v / 255 in the
 *                          planes' type. Writes nothing but out, DEVICE fp64 [2 MG_COMPOSE_MAX_PLANES + 1]: [j] = sum plane_j (1 - a / 255),
 *                          [MAX_PLANES + j] = sum plane_j for j < n_prev, [2 MAX_PLANES] = sum a / 255, zeros elsewhere; the product and 1 - x in
 *                          the planes' type, the sums in fp64: MG_COMPOSE_SUM_BLOCKS partials per sum in `partial` (fp64
 *                          [2 MAX_PLANES + 2][SUM_BLOCKS]), each a fixed tree over a strided chunk, added in index order. No atomics.
 *   mg_compose_commit    : one launch: image [h][w][3] masked paste of fg [ha][wa][3] through a; canvas [h][w][3] = fg inside the box, 0 outside;
 *                          plane idx = a / 255 inside, 0 outside; planes j < idx *= 1 - a / 255. image, canvas (and fg with both) may be NULL.
 *   mg_compose_planes_u8 : out = trunc(plane * 255) (product in the planes' type), flags int32 [count] = 1 where a plane holds a non-zero value.
 *   mg_compose_alpha_box : box int32 [4] = min x, min y, max x, max y of alpha > 0 (w, h, -1, -1 for an all-zero plane).
 * Each returns -2 for an argument error before any launch (sides 1..MG_COMPOSE_MAX_SIDE), -3 when a launch would exceed a grid dimension.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_COMPOSE_TILE_ROWS 16
#define MG_COMPOSE_TILE_BYTES 192
#define MG_COMPOSE_MAX_ROWS 128
#define MG_COMPOSE_LDS_BYTES (MG_COMPOSE_MAX_ROWS * MG_COMPOSE_TILE_BYTES)
#define MG_COMPOSE_THREADS 256
#define MG_COMPOSE_TAB_HEADER 4
#define MG_COMPOSE_MAX_PLANES 10
#define MG_COMPOSE_SUM_BLOCKS 64
#define MG_COMPOSE_MAX_SIDE 32767
#define MG_COMPOSE_FUSED 0
#define MG_COMPOSE_TWO_PASS 1
#define MG_COMPOSE_F32 0
#define MG_COMPOSE_F64 1
int mg_compose_resize(const uint8_t* src, uint8_t* out, uint8_t* tmp, const int32_t* xtab, const int32_t* ytab, long n, int ps, int src_h,
                      int src_w, int cx, int cy, int cw, int ch, int out_h, int out_w, int kx, int ky, int regime, void* stream);
int mg_compose_paste(uint8_t* dst, const uint8_t* src, const uint8_t* mask, int ps, int dst_h, int dst_w, int src_h, int src_w, int x, int y,
                     void* stream);
int mg_compose_try_place(const void* planes, const uint8_t* a, const void* lut, double* partial, double* out, int dtype, int h, int w, int ha,
                         int wa, int x, int y, int n_prev, void* stream);
int mg_compose_commit(uint8_t* image, uint8_t* canvas, void* planes, const uint8_t* fg, const uint8_t* a, const void* lut, int dtype, int h, int w,
                      int ha, int wa, int x, int y, int idx, void* stream);
int mg_compose_planes_u8(const void* planes, uint8_t* out, int32_t* flags, int dtype, long count, int h, int w, void* stream);
int mg_compose_alpha_box(const uint8_t* alpha, int32_t* box, int h, int w, void* stream);
int mg_compose_limits(int* tile_rows, int* tile_bytes, int* max_rows, int* lds_bytes, int* tab_header, int* max_planes, int* sum_blocks,
                      int* max_side);

/* ---------------------------------------------------------------------------------------------------------------
 * Validation metrics on the device (maggie/utils/metric.py). fp32 planes, fp64 results. `trimap` may be NULL;
 * mask_mode: 0 = all ones, 1 = (trimap > 0) (Metric.update :47), 2 = (trimap == 1) (dtSSD.update :427).
 *   mg_metric_plane_sums: out[P][3] = per plane { sum |pred-gt| m, sum (pred-gt)^2 m, sum m }      (SAD :68-78, MSE :80-90, MAD :92-97)
 *   mg_metric_grad      : out[P] = per plane sum (|G(gt_n)| - |G(pred_n)|)^2 m, G = 9x9 Gaussian-derivative pair (filter_x81,
 *                         filter_y = its transpose, zero padding), x_n = (x - min) / (max - min + 1e-6) over the WHOLE tensor
 *                         (:388-405); scratch4: 4 int32 of device scratch
 *   mg_metric_dtssd     : pred/gt/trimap [B][T][N][HW]; out[N] = sum_{b,t<T-1,px} ((p[t+1]-p[t]) - (g[t+1]-g[t]))^2 m[t]  (:436-441)
 * ------------------------------------------------------------------------------------------------------------- */
int mg_metric_plane_sums(const float* pred, const float* gt, const float* trimap, int mask_mode, int P, long HW, double* out, void* stream);
int mg_metric_grad(const float* pred, const float* gt, const float* trimap, int mask_mode, int P, int H, int W, const float* filter_x81,
                   int32_t* scratch4, double* out, void* stream);
int mg_metric_dtssd(const float* pred, const float* gt, const float* trimap, int mask_mode, int B, int T, int N, long HW, double* out,
                    void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Inference post-path: `reverse_transform_tensor` (maggie/utils/postprocessing.py:36-64: crop the
 * bottom/right padding to (crop_h, crop_w), bilinear resize with align_corners=True to (Hout, Wout)) fused with the alpha
 * snapping of maggie/engine/test.py:139-142,229-231 (<= 1/255 -> 0, >= 254/255 -> 1 when `snap`). fp32 planes [P,Hin,Win].
 * ------------------------------------------------------------------------------------------------------------- */
int mg_postprocess_alpha(const float* in, int P, int Hin, int Win, int crop_h, int crop_w, int Hout, int Wout, int snap, float* out,
                         void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Connected components of many 2-D binary planes (csrc/ccl.hip): tile union-find in LDS, border merge, flatten. The root of a component
 * is its smallest row-major index, so every result is independent of scheduling. H * W < 2^31 (else -2); every scratch buffer comes
 * from the caller, sized by mg_cc_scratch_bytes(op, P, H, W, &bytes) for op MG_CC_OP_LABEL / _CONN / _LARGEST. No host synchronisation.
 *   mg_cc_label              : mask u8 [P][H][W] (non-zero = foreground), connectivity 1 (4-neighbours) or 2 (8-neighbours) ->
 *                              labels i32 [P][H][W] = 1..num[p] in the raster order of each component's first pixel, background 0:
 *                              skimage.measure.label's array; num i32 [P].
 *   mg_metric_conn           : out f64 [P] = per plane conn_diff of maggie/utils/metric.py:240-298 (before * 0.001): levels i = 1..10,
 *                              t_i = float32(i * 0.1), intersection_i = (gt >= t_i) & (pred >= t_i) compared in fp32 (numpy < 2),
 *                              largest 4-connected component (ties: the smallest root); round_down = t_{i-1} for the first level whose
 *                              largest component misses the pixel, else 1; term |(1 - gd [gd >= 0.15]) - (1 - pd [pd >= 0.15])| m in
 *                              fp32, summed in fp64 in a fixed order (bit-reproducible). mask_mode as for the metrics above.
 *   mg_postprocess_largest_cc: out = alpha * [pixel in the largest 8-connected component of alpha > thresh] (maggie/utils/postprocessing.py
 *                              :66-86; ties: the smallest root); a plane with no foreground is copied unchanged. Capturable in a graph.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_CC_OP_LABEL 0
#define MG_CC_OP_CONN 1
#define MG_CC_OP_LARGEST 2
int mg_cc_scratch_bytes(int op, int P, int H, int W, long* bytes);
int mg_cc_label(const uint8_t* mask, int P, int H, int W, int connectivity, int32_t* labels, int32_t* num, void* scratch, void* stream);
int mg_metric_conn(const float* pred, const float* gt, const float* trimap, int mask_mode, int P, int H, int W, void* scratch, double* out,
                   void* stream);
int mg_postprocess_largest_cc(const float* alpha, int P, int H, int W, float thresh, void* scratch, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Dense Farneback optical flow and the MESSDdt metric (csrc/flow.hip; maggie/utils/metric.py:450-531). fp32 arithmetic; every scratch
 * buffer comes from the caller; no host synchronisation and no allocation; the launch count depends on the pyramid depth only.
 *   mg_flow_levels          : pyramid levels below full size for H x W planes (0..5): halve while both sides stay >= 32
 *   mg_flow_farneback       : prev, next u8 [P][H][W] -> flow f32 [P][H][W][2] ([..][0] along columns, [..][1] along rows;
 *                             next(p + flow) ~ prev(p)). The parameters are those of cv2.calcOpticalFlowFarneback and must be the
 *                             reference's (0.5, 5, 10, 2, 7, 1.5, MG_FLOW_GAUSSIAN), else -2. scratch: mg_flow_scratch_bytes.
 *   mg_metric_messddt       : pred / gt / trimap (may be NULL; mask = trimap == 1) f32 [F][N][H][W] -> out f64 [N][2] =
 *                             { sum_t sum |error_map|, sum_t (sum m_t + 1) } with error_map = (p_t - g_t)^2 m_t - (p' - g')^2 m', the primed
 *                             sample read as the reference reads it: for pixel (row i, column j) at row clamp(j + fx, 0, H-1), column
 *                             clamp(i + fy, 0, W-1) of FRAME 1, for every t. The flow is that of the planes (uint8)(gt * 255.0f), rounded
 *                             half to even; `flow_in` (f32 [F-1][N][H][W][2], tests) replaces it, `flow_out` receives it; both may be
 *                             NULL. F < 2: zeros. scratch: mg_messddt_scratch_bytes.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_FLOW_GAUSSIAN 256       /* cv2.OPTFLOW_FARNEBACK_GAUSSIAN */
#define MG_FLOW_MAX_SIDE 32767
int mg_flow_levels(int H, int W);
int mg_flow_scratch_bytes(long P, int H, int W, long* bytes);
int mg_flow_farneback(const uint8_t* prev, const uint8_t* next, long P, int H, int W, double pyr_scale, int levels, int winsize,
                      int iterations, int poly_n, double poly_sigma, int flags, void* scratch, float* flow, void* stream);
int mg_messddt_scratch_bytes(int F, int N, int H, int W, long* bytes);
int mg_metric_messddt(const float* pred, const float* gt, const float* trimap, int F, int N, int H, int W, const float* flow_in,
                      void* scratch, float* flow_out, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sparse refinement head with a DEVICE row count (round 2).
 * The reference's detail stage (maggie/network/decoder/resnet_inst_matt_spconv.py:196-270) sizes every spconv feature matrix from
 * `torch.nonzero` (:206) -- a device->host read per forward, after which ~430 small launches are paced by the host. Here the site
 * counts of the index pyramid stay in device words (mg_bits_rank: rowoff[P*H]); feature matrices are (capacity x C) buffers and
 * every kernel below runs over min(*rows_dev, capacity) rows from a fixed grid (mg_conv_params.m_dev / mg_rowwise_params.m_dev for
 * the implicit-GEMM and BatchNorm entry points). `*_dev` = the entry point of the same name with the extra `rows_dev` argument
 * (NULL: identical to the plain one).
 * ------------------------------------------------------------------------------------------------------------- */
int mg_gather_rows_dev(const void* dense, int dtype, const int32_t* coords, int R, int n_i, int Hd, int Wd, int C, const float* mul,
                       int mul_ninst, void* out, int ldo, int yoff, const int32_t* rows_dev, void* stream);
int mg_gather_rows_bwd_dev(const void* dout, int dtype, int ldo, int yoff, const int32_t* coords, int R, int n_i, int Hd, int Wd, int C,
                           const float* mul, int mul_ninst, const void* dense, float* ddense, float* dmul, const int32_t* rows_dev, void* stream);
int mg_scatter_plane_dev(const void* vals, int dtype, int ldv, int col, const int32_t* coords, int R, int P, int H, int W, float fill,
                         float* plane, const int32_t* rows_dev, void* stream);
/* zero_rest != 0: the other ldv - 1 columns of every live row are zeroed (gradient of a 1-channel output padded to a 16-byte row) */
int mg_gather_plane_dev(const float* plane, const int32_t* coords, int R, int H, int W, void* vals, int dtype, int ldv, int col,
                        const int32_t* rows_dev, int zero_rest, void* stream);
int mg_gather_table_dev(const int32_t* coords, int R, int ksize, int kind, const void* src_bits, const int32_t* src_wordoff, int Hs,
                        int Ws, int32_t* nbr, const int32_t* rows_dev, void* stream);
int mg_colstats_dev(const void* x, int dtype, int M, int C, int ld, float* stats, const int32_t* rows_dev, void* stream);
int mg_colstats_centered_dev(const void* x, int dtype, int M, int C, int ld, float* stats, int have_sum, const int32_t* rows_dev, void* stream);
int mg_bias_act_bwd_dev(const void* dy, const void* y, void* g, int dtype, int M, int C, float* db, const int32_t* rows_dev, void* stream);
/* out = a * sigmoid(g): instance-specific guidance, `detail * guidance` of resnet_inst_matt_spconv.py:188-193 (a may be a channel slice
 * of a wider buffer: row pitch lda); backward da = dout * s, dg = dout * a * s * (1 - s) */
int mg_rows_sigmoid_mul_fwd(const void* a, int lda, const void* g, void* out, int dtype, int M, int C, const int32_t* rows_dev, void* stream);
int mg_rows_sigmoid_mul_bwd(const void* dout, const void* a, int lda, const void* g, void* da, void* dg, int dtype, int M, int C,
                            const int32_t* rows_dev, void* stream);
/* out = a + b over the live rows (gradient of a feature matrix with two consumers) */
int mg_rows_add(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int dtype, int M, int C, const int32_t* rows_dev, void* stream);
/* nn.Dropout(p) of FFNLayer (maggie/network/module/mask_attention.py:170-182) with a counter-based mask: keep = hash(state, salt, element)
 * >= p; `state` = device int64[2] (seed, step). The backward calls the same entry point on the gradient (same state and salt). */
int mg_rows_dropout(const void* x, void* y, int dtype, int M, int C, float p, const int64_t* state, int salt, const int32_t* rows_dev, void* stream);
/* y = LayerNorm(x + r) * gamma + beta per row (post-norm residual of FFNLayer, mask_attention.py:176-181); rstat [M][2] = (mean, rstd).
 * Backward: dz (= dx = dr), dgamma / dbeta [C] (zeroed here, fp32). C / (8 bf16 | 4 fp32) must be a power of two <= 64. */
int mg_rows_add_layernorm_fwd(const void* x, const void* r, const float* gamma, const float* beta, float eps, void* y, float* rstat, int dtype,
                              int M, int C, const int32_t* rows_dev, void* stream);
int mg_rows_add_layernorm_bwd(const void* dy, const void* x, const void* r, const float* gamma, const float* rstat, void* dz, float* dgamma,
                              float* dbeta, int dtype, int M, int C, const int32_t* rows_dev, void* stream);
/* resnet_inst_matt_spconv.py:347-348 ("dummy code to prevent all zeros"): if *count == 0, set bits [y0:y1, x0:x1] of every plane */
int mg_bits_patch_if_empty(void* bits, const int32_t* count, int P, int H, int W, int y0, int y1, int x0, int x1, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Temporal-consistency tail of the video model (maggie_amd/csrc/temporal2.hip), fp32 planes.
 *   mg_bifuse_fwd/_bwd : bidirectional alpha fusion of maggie/network/decoder/resnet_inst_matt_spconv_temp.py:35-79 over the T frames
 *                        of a clip. preds / fused (B,T,NI,HW); diffs (2(T-1), B, HW) = the difference logits in the reference's call
 *                        order (forward pairs, then backward pairs); fdiff / bdiff (B,T,HW) = the reference's forward_diffs /
 *                        backward_diffs (zero-padded), fsig / bsig their sigmoids. Backward: dpreds, ddiffs (summed over instances).
 *   mg_dtssd_fwd/_bwd  : loss_dtSSD (maggie/network/loss.py:7-16): sums[0] / sums[1]; p, g, m hold T frames of E elements per batch
 *                        item with batch strides *bs (frame slices of a wider tensor need no copy); sig != 0: p = sigmoid(logits)
 *                        (loss_temporal_sparsity, :183-203); m NULL = ones. Backward: dp = gout / sums[1] * d(numerator)/dp.
 *   mg_bce_logits_*    : F.binary_cross_entropy_with_logits(reduction='mean') of the difference logits (:189-190), same strides.
 *   mg_temporal_crop   : eval-time bounding-box crop (:115-142 with utils/utils.py:61-83): in place on alpha [P,H,W] and on the
 *                        detail bit planes [P,H,Ww]; scratch [P,H,W] floats, box int32[P][4].
 * ------------------------------------------------------------------------------------------------------------- */
int mg_bifuse_fwd(const float* preds, const float* diffs, int B, int T, int NI, long HW, float* fused, float* fdiff, float* bdiff, float* fsig,
                  float* bsig, void* stream);
int mg_bifuse_bwd(const float* dfused, const float* preds, const float* diffs, int B, int T, int NI, long HW, float* dpreds, float* ddiffs, void* stream);
int mg_dtssd_fwd(const float* p, long pbs, const float* g, long gbs, const float* m, long mbs, int B, int T, long E, int sig, float* sums, void* stream);
int mg_dtssd_bwd(const float* p, long pbs, const float* g, long gbs, const float* m, long mbs, int B, int T, long E, int sig, const float* sums,
                 const float* gout, float* dp, long dbs, void* stream);
int mg_bce_logits_fwd(const float* x, long xbs, const float* y, long ybs, int B, long TE, float* sum, void* stream);
int mg_bce_logits_bwd(const float* x, long xbs, const float* y, long ybs, int B, long TE, const float* gout, float* dx, long dbs, void* stream);
int mg_temporal_crop(float* alpha, void* bits, int P, int H, int W, float sigma, float thr, int pad, float* scratch, int32_t* box, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Loss bookkeeping (maggie_amd/csrc/losses.hip)
 *   mg_atten_loss_fwd/_bwd : compute_atten_loss of maggie/network/module/instance_matte_decoder.py (guidance_mask [rows, L], attention
 *                            matrix [rows, L], rows = batch * instance slots): out[0] = scale * sum_rows((sum_l gm != 0) - sum_l gm * att);
 *                            terms [rows] scratch. Backward: datt = -scale * gout[0] * gm.
 *   mg_scalar_lincomb/_bwd : out[0] = sum_i coef[i] * ptrs[i][0] over n <= 16 device scalars (ptrs / coef are HOST arrays, passed by value
 *                            into the launch): the loss sums of arch/maggie.py:283-300; backward gin[i] = coef[i] * gout[0].
 * ------------------------------------------------------------------------------------------------------------- */
int mg_atten_loss_fwd(const float* gm, const float* att, int rows, long L, float scale, float* terms, float* out, void* stream);
int mg_atten_loss_bwd(const float* gm, const float* gout, float scale, long n, float* datt, void* stream);
int mg_scalar_lincomb(const float* const* ptrs, const float* coef, int n, float* out, void* stream);
int mg_scalar_lincomb_bwd(const float* coef, int n, const float* gout, float* gin, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Token side of the instance matte decoder (maggie_amd/csrc/token_side.hip): the (batch x 10 tokens) x 128 operations of
 * maggie/network/module/mask_attention.py:9-206 -- projections, FFN / MLP layers, post-norm residual LayerNorms (SelfAttentionLayer
 * :9-60, CrossAttentionLayer :63-133 token side, FFNLayer :170-182, MLP :185-206) -- fp32, single-workgroup kernels.
 *   mg_token_linear_fwd: y[R,N] = LN( res + act( (x + xadd)[R,K] W[N,K]^T + bias ) ); xadd / bias / res / gamma,beta (LayerNorm) may be
 *                        NULL, relu 0/1. With a LayerNorm: z[R,N] (its input) and rstat[R][2] = (mean, rstd) are kept for the backward.
 *   mg_token_linear_bwd: from dy: dx[R,K] (also the gradient of xadd), dW[N,K], db[N], dres[R,N], dgamma / dbeta[N] (NULL when absent);
 *                        yout = the forward output (ReLU mask; only read when relu); dz_scratch [R,N] floats.
 *   mg_token_sa_fwd/bwd: out[b] = softmax(q[b] k[b]^T * scale, keys with pad[b][j] != 0 masked) v[b], prob [B,T,T] kept; T <= 16.
 * ------------------------------------------------------------------------------------------------------------- */
int mg_token_linear_fwd(const float* x, const float* xadd, const float* W, const float* bias, const float* res, int relu, const float* gamma,
                        const float* beta, float eps, float* y, float* z, float* rstat, int R, int K, int N, void* stream);
int mg_token_linear_bwd(const float* dy, const float* x, const float* xadd, const float* W, const float* yout, int relu, const float* gamma,
                        const float* z, const float* rstat, float* dx, float* dW, float* db, float* dres, float* dgamma, float* dbeta, float* dz_scratch,
                        int R, int K, int N, void* stream);
/* mg_token_linear_fwd / _bwd with `wt` != 0: W is given as [K][N] and y = (x + xadd) W (dW is returned as [K][N] too) -- the `x @ wk` products of
 * mask_attention.py (queries folded through the key projection) without a transposed copy of the weight each step. N % 4 == 0. */
int mg_token_linear_fwd_ex(const float* x, const float* xadd, const float* W, const float* bias, const float* res, int relu, const float* gamma,
                           const float* beta, float eps, float* y, float* z, float* rstat, int R, int K, int N, int wt, void* stream);
int mg_token_linear_bwd_ex(const float* dy, const float* x, const float* xadd, const float* W, const float* yout, int relu, const float* gamma,
                           const float* z, const float* rstat, float* dx, float* dW, float* db, float* dres, float* dgamma, float* dbeta,
                           float* dz, int R, int K, int N, int wt, void* stream);
/* Mask pre-processing of the instance matte decoder (instance_matte_decoder.py:131-153; utils.py:16-21): mask [B][NF][n_in][h*s][w*s] fp32 guidance
 * masks (s = integer factor over the OS8 map), gt (or NULL) [B][NF][n_gt][h*gs][w*gs] fp32 alphas -> feat_ids int32 [B][NF*h*w] = max_i (i+1) * [avg-pooled
 * mask_i > 0]; valid uint8 [B][n_i] padded to 4 bytes (zeroed here): 1 where slot i has a mask pixel; guidance fp32 [B][n_i][NF*h*w] = [max-pooled alpha_i > 0]
 * (only with gt). */
int mg_imd_prep(const float* mask, int n_in, int s, const float* gt, int n_gt, int gs, int B, int NF, int h, int w, int n_i, int32_t* feat_ids,
                float* guidance, unsigned char* valid, void* stream);
/* Up to 4 INDEPENDENT token linear layers per launch (the q / k / v projections of the token self-attention, the folded key / table products of a
 * cross attention: module/mask_attention.py:9-206): per layer the semantics of mg_token_linear_fwd_ex / _bwd_ex. Unused pointers are NULL. */
typedef struct mg_tok_lin {
    const float *x, *xadd, *W, *bias, *res, *gamma, *beta;   /* forward inputs ([R,K], [R,K], [N,K] or [K,N] with wt, [N], [R,N], [N], [N]) */
    float *y, *z, *rstat;                                    /* forward outputs (z: pre-LayerNorm values, rstat [R,2]: with gamma)          */
    const float *dy, *yout;                                  /* backward inputs ([R,N]; yout = y of a ReLU layer)                          */
    float *dx, *dW, *db, *dres, *dgamma, *dbeta, *dz;        /* backward outputs (dz: [R,N] scratch; = dy for a plain layer)               */
    int32_t R, K, N, relu, wt;
    float eps;
    int32_t dx_pair;                                         /* backward (round 5): 1 + index of another layer of the call that reads the SAME x (neither
                                                                has an xadd; that layer passes dx = NULL): its dz . W is added into this layer's dx --
                                                                one input gradient for the shared tensor instead of two and an add; 0: none */
} mg_tok_lin;
int mg_token_linear_multi_fwd(const mg_tok_lin* ops, int n, void* stream);
int mg_token_linear_multi_bwd(const mg_tok_lin* ops, int n, void* stream);
/* einsum('bqc,blc->blq') of the instance matte decoder (instance_matte_decoder.py:296-299): logits[b][l][q] = sum_c feat[b][l][c] tok[b][q][c] for
 * q < Q, zero up to the row pitch QP (= 16). feat / out / dlog / dfeat in `dtype` ([B][L][C] / [B][L][QP]); tok / dtok fp32 [B][Q][C] (dtok is
 * overwritten). C = 32 or 64, Q <= 16. The tokens are rounded to `dtype` first (the 1x1 convolution this replaces did the same). */
int mg_token_einsum_fwd(const void* feat, int dtype, const float* tok, int B, int L, int C, int Q, int QP, void* out, void* stream);
int mg_token_einsum_bwd(const void* dlog, const void* feat, int dtype, const float* tok, int B, int L, int C, int Q, int QP, void* dfeat,
                        float* dtok, void* stream);
/* out[i] = ((srcs[0][i] + srcs[1][i]) + srcs[2][i]) + ... : the gradient of a tensor with k <= 16 consumers in one launch and a fixed order (replaces
 * the k - 1 pairwise adds of the autograd engine; maggie/network/module/mask_attention.py:63-133 uses every token tensor several times). fp32. */
int mg_sum_k(const float* const* srcs, int k, long n, float* out, void* stream);
/* The same for tensors of `dtype` (MG_F32 / MG_BF16 / MG_F16; 16-byte aligned): 16-bit terms are added in fp32 in the given order and rounded once. */
int mg_sum_k_t(const void* const* srcs, int k, long n, void* out, int dtype, void* stream);
/* AdaptiveAvgPool2d(1) over NHWC rows (maggie/network/module/aspp.py:24-27,50-52). mode 0: x (N, HW, C) -> out (N, C), the mean of each sample's rows
 * (fp32 sums in a fixed order); mode 1: x = dy (N, C) -> out = dx (N, HW, C) = dy / HW; mode 2: like 0 without the division (the backward of broadcasting
 * the pooled row back over the map). ld: element stride between the rows of x in modes 0 / 2 (0 = C; a channel slice of a wider map is read in place). */
int mg_spatial_mean(const void* x, void* out, int dtype, int N, int HW, int C, int mode, int ld, void* stream);
/* dsts[j][0 .. bytes[j]) = srcs[j][...] for j < k <= 16 as ONE launch (replaces torch._foreach_copy_ of contiguous same-type tensors = one hipMemcpyAsync
 * each: the outputs a replayed graph hands to the caller, engine/train.py:229-241 keeps them across steps; gradient hand-over between graphs). */
int mg_copy_k(const void* const* srcs, void* const* dsts, const long* bytes, int k, void* stream);
/* Any number of copies in one launch, the job list in DEVICE memory: table = int64[4 * jobs], (src, dst, bytes, first 4 KiB block) per job with the first
 * blocks ascending from 0; nblk = total number of 4 KiB blocks. (A captured graph fills the table once, after the capture.) */
int mg_copy_table(const long* table, int jobs, long nblk, void* stream);
/* out[4] (int32, device) = [a NaN among the n fp32 tokens, nonzero[0] == 0, ovf[0] != 0, err[0]] -- NULL inputs give 0. The four words the host reads
 * between the trunk and the detail stage (maggie/network/module/mask_attention.py:95-98 raises on NaN tokens; resnet_inst_matt_spconv.py:314 switches
 * the guidance to the ground truth when the coarse alpha is zero), in one launch. */
int mg_step_flags(const float* tokens, long n, const int* nonzero, const int* ovf, const int* err, int* out, void* stream);
int mg_token_sa_fwd(const float* q, const float* k, const float* v, const unsigned char* pad, float scale, int B, int T, int D, float* out, float* prob,
                    void* stream);
int mg_token_sa_bwd(const float* dout, const float* q, const float* k, const float* v, const float* prob, float scale, int B, int T, int D, float* dq,
                    float* dk, float* dv, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mailbox all-reduce (csrc/mailbox.hip): in-place fp32 sum over the ranks of a pack of <= MG_MAILBOX_PACK floats as ONE kernel launch on `stream`
 * (capturable into hipGraphs), through peer-mapped mailboxes instead of RCCL. Replaces: the statistics all-reduce of nn.SyncBatchNorm
 * (engine/train.py:159-161) when the step is replayed from graphs. Setup: every rank calls mg_mailbox_create (-> its mailbox + a 64-byte IPC handle),
 * exchanges the handles out of band, opens the peers' with mg_mailbox_open and fills mg_mailbox.peer[] (its own pointer at peer[rank]). `seq_dev`
 * (zeroed uint32) and `err_dev` (zeroed int32; set to 1 when a peer did not arrive within `spin_ticks` of the 100 MHz wall clock) are this rank's own
 * device words. Every rank must issue the same sequence of calls.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_MAILBOX_MAX_RANKS 8
#define MG_MAILBOX_SLOTS 64
#define MG_MAILBOX_PACK 1088
typedef struct mg_mailbox {
    float* peer[MG_MAILBOX_MAX_RANKS]; /* peer[r]: rank r's mailbox as mapped into THIS process */
    int32_t world, rank;
} mg_mailbox;
long mg_mailbox_bytes(int world);
int mg_mailbox_create(int world, void** ptr, void* handle64);
int mg_mailbox_open(const void* handle64, void** ptr);
int mg_mailbox_close(void* ptr);
int mg_mailbox_free(void* ptr);
int mg_mailbox_allreduce(const mg_mailbox* mb, float* data, int n, uint32_t* seq_dev, int32_t* err_dev, long spin_ticks, void* stream);
/* out-of-place form (src is left untouched: SyncBN backward keeps the LOCAL sums for dgamma / dbeta) */
int mg_mailbox_allreduce_to(const mg_mailbox* mb, const float* src, float* dst, int n, uint32_t* seq_dev, int32_t* err_dev, long spin_ticks, void* stream);
/* SyncBN forward statistics in one launch: this rank's [nrep][2C] sums (sum x | sum x^2) and row count -> exchanged -> outs = scale | shift | mean |
 * invstd [4C], *count_out = global count, running statistics updated (the arithmetic of mg_bn_finalize on the pooled moments). 2C + 1 <= MG_MAILBOX_PACK. */
int mg_mailbox_bn_finalize(const mg_mailbox* mb, const float* stats, int nrep, float count, int C, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* outs, float* count_out,
                           uint32_t* seq_dev, int32_t* err_dev, long spin_ticks, void* stream);
/* the same with this rank's row count read from the device (count_dev: int32 [1], NULL = use `count`): BatchNorm1d over the sparse head's live rows */
int mg_mailbox_bn_finalize_dev(const mg_mailbox* mb, const float* stats, int nrep, float count, const int32_t* count_dev, int C, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* outs, float* count_out,
                               uint32_t* seq_dev, int32_t* err_dev, long spin_ticks, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Baseline JPEG decoding (csrc/jpegdec.hip): the entropy-coded segments of `frames` files of one geometry -> RGB on the device. Replaces T.Load
 * (maggie/dataloader/transforms.py:38-66: Image.open(path).convert("RGB")) for SOF0 files with one interleaved scan, in one of six layouts:
 * 4:2:0, 4:4:4, greyscale, and 4:2:2, 4:4:0 and 4:1:1. csrc/jpeg_common.h maps a layout to its geometry:
 *   luma sampling (hs, vs) = (2, 2), (1, 1), (1, 1), (2, 1), (1, 2), (4, 1) over (1, 1) Cb and Cr (greyscale: one component). An MCU is
 *   8 hs x 8 vs pixels and holds hs * vs luma blocks (row-major) then Cb then Cr: 6, 3, 1, 4, 4, 6 blocks, the slot words 912..917 of `tabs`;
 *   mcux = ceil(w / 8 hs), mcuy = ceil(h / 8 vs); coef int16 [frames][mcuy * mcux * blocks per MCU][64];
 *   planes  : Y [frames][mcuy * 8 vs][yp] then Cb, Cr [frames][mcuy * 8][cp] each, `planes` 16-byte aligned. 4:2:0, 4:4:4 and greyscale are as
 *             wide as their blocks: yp = mcux * 8 hs, cp = mcux * 8. 4:2:2, 4:4:0 and 4:1:1 are PITCHED: yp rounded up to 16, and cp too in
 *             4:4:0: a lane of mg_jpeg_rgb_hv loads 16 luma and 8 / 16 / 4 chroma bytes at once, and a pitch of that many bytes keeps each
 *             load inside its row and aligned. The bytes between a row's blocks and its pitch are never written and never used.
 *             plane_bytes = frames * mcuy * 8 * (vs * yp + 2 * cp), without the 2 * cp in greyscale.
 * The Huffman decoding is the self-synchronising parallel form: the segment is cut into subsequences of `sub_bytes` raw
 * bytes, one lane each.
 *   tabs    : int32 [frames][MG_JPEGDEC_TAB_WORDS], one record per frame: four Huffman tables (DC 0, DC 1, AC 0, AC 1) of 228 words each
 *             (look uint16[256] = len << 8 | symbol for codes of at most 8 bits, else 0; maxcode int32[18] by length, -1 = none; valoff int32[18]
 *             = index of the length's first value minus its first code; vals uint8[256]); words 912..917 the block slots of an MCU
 *             (DC table | AC table << 4); 918 the segment's offset in `data`, 919 its length, 920 the restart interval in MCUs (0 = none);
 *             928..1119 the quantisation tables of components 0, 1, 2 in natural order.
 *   mg_jpegdec_sync  : launch number `launch` (0, 1, 2, ...) of the synchronisation. exits uint64 [frames][nsub] (a subsequence's exit state:
 *             raw bit position | slot << 40 | zig-zag index << 44), counts int32 [frames][nsub] (blocks completed), entries uint64
 *             [frames][ceil(nsub / MG_JPEGDEC_THREADS)], bounds uint64 [2][frames][ceil(nsub / MG_JPEGDEC_THREADS)]; info int32 [info_words],
 *             zeroed by the caller: [0] status bits, [2 + 2 k] nonzero when launch k moved a workgroup's exit state (another launch is needed),
 *             [3 + 2 k] the rounds launch k ran inside a workgroup. nsub = ceil(longest segment / sub_bytes).
 *   mg_jpegdec_coef  : counts -> first_block int32 [frames][nsub] (exclusive sum), then coef int16 [frames][blocks][64] (zero-filled by the
 *             caller; scan order, natural order inside a block, the DC term as its difference) and the status bits.
 *   mg_jpegdec_dcsum : DC differences -> DC terms, per component within each restart interval.
 *   mg_jpegdec_idct  : coef x table -> inverse DCT -> planes uint8: 4:2:0 in mg_jpeg_rgb's layout (finish with mg_jpeg_rgb); 4:4:4 and greyscale
 *             finish with mg_jpegdec_rgb, the pitched layouts with mg_jpeg_rgb_hv.
 *   mg_jpegdec_rgb   : the 4:4:4 / greyscale planes -> out, the epilogues of mg_jpeg_rgb.
 *   mg_jpeg_rgb_hv (csrc/photometric.hip): the pitched planes, named by (hs, vs) = (2, 1), (1, 2) or (4, 1), -> out with the epilogues of
 *             mg_jpeg_rgb. Chroma is upsampled over the real ceil(h / vs) x ceil(w / hs) samples, neighbours clamped to them: 4:2:2
 *             out[2j] = (3 c[j] + c[j-1] + 1) >> 2, out[2j+1] = (3 c[j] + c[j+1] + 2) >> 2 along the row (replication when ceil(w / 2) <= 2);
 *             4:4:0 the same along the column at every width; 4:1:1 replication.
 * Each returns -2 for an argument error (before any launch), -3 when the launch would exceed a grid dimension. Sizes (`data_bytes`,
 * `coef_elems`, `plane_bytes`) are checked against the geometry and bound every access.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_JPEGDEC_420 0
#define MG_JPEGDEC_444 1
#define MG_JPEGDEC_GREY 2
#define MG_JPEGDEC_422 3
#define MG_JPEGDEC_440 4
#define MG_JPEGDEC_411 5
#define MG_JPEGDEC_THREADS 128
#define MG_JPEGDEC_TAB_WORDS 1120
#define MG_JPEGDEC_MIN_SUB 8 /* 16 code bits + 11 value bits = 4 data bytes, each of which may drag a stuffed byte */
#define MG_JPEGDEC_MAX_SUB 4096
#define MG_JPEGDEC_DEFAULT_SUB 8 /* the best of tools/jpegdec_bench.py's sweep on its 1080 x 1920 file */
#define MG_JPEGDEC_MAX_BYTES (1L << 28)
#define MG_JPEGDEC_ST_INDEX 1    /* a zig-zag index past 63 */
#define MG_JPEGDEC_ST_CODE 2     /* an unassigned code or a category above 11 */
#define MG_JPEGDEC_ST_PAST_END 4 /* the segment ended before the last block */
#define MG_JPEGDEC_ST_COUNT 8    /* the blocks decoded are not MCUs x blocks per MCU */
#define MG_JPEGDEC_ST_RESTART 16 /* a restart marker off an interval's end, out of order, or without DRI */
int mg_jpegdec_limits(int* threads, int* min_sub, int* max_sub, int* default_sub, int* tab_words);
int mg_jpegdec_sync(const uint8_t* data, long data_bytes, const int32_t* tabs, unsigned long long* exits, int32_t* counts,
                    unsigned long long* entries, unsigned long long* bounds, int32_t* info, int info_words, long frames, int nsub, int sub_bytes,
                    int layout, int launch, void* stream);
int mg_jpegdec_coef(const uint8_t* data, long data_bytes, const int32_t* tabs, const unsigned long long* exits, const int32_t* counts,
                    int32_t* first_block, int16_t* coef, long coef_elems, int32_t* info, long frames, int nsub, int sub_bytes, int h, int w, int layout,
                    void* stream);
int mg_jpegdec_dcsum(int16_t* coef, long coef_elems, const int32_t* tabs, long frames, int h, int w, int layout, void* stream);
int mg_jpegdec_idct(const int16_t* coef, long coef_elems, const int32_t* tabs, uint8_t* planes, long plane_bytes, long frames, int h, int w, int layout,
                    void* stream);
int mg_jpegdec_rgb(const uint8_t* planes, long plane_bytes, void* out, long frames, int h, int w, int layout, int epilogue, const float* mean3,
                   const float* std3, void* stream);
int mg_jpeg_rgb_hv(const uint8_t* planes, long plane_bytes, void* out, long frames, int h, int w, int hs, int vs, int epilogue, const float* mean3,
                   const float* std3, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Progressive JPEG decoding (csrc/jpegprog.hip): the scans of `frames` SOF2 files of one geometry, in any of mg_jpegdec's six layouts -> the
 * coefficient buffer of mg_jpegdec_idct (int16 [frames][blocks][64], zero-filled by the caller, DC terms final: mg_jpegdec_dcsum is NOT called). One wave per chain of scans
 * (DESIGN.md section 30): a file's DC scans, or the AC scans of one of its components, in file order.
 *   scans   : int32 [nscans][MG_JPEGPROG_SCAN_WORDS], one record per scan: two Huffman tables of 228 words each (mg_jpegdec's form; a DC scan:
 *             DC table 0 and 1, an AC scan: its one table first); word 456 the segment's offset in `data`, 457 its length, 458 the restart
 *             interval in MCUs (0 = none), 459 Ss, 460 Se, 461 Ah, 462 Al, 463 the blocks of an MCU of this scan when it is interleaved (0: one
 *             component, visited over its real blocks in raster order), 464 that one component, 466..471 the interleaved scan's blocks:
 *             slot in the frame's MCU | component << 4 | table << 8.
 *   chains  : int32 [nchains][MG_JPEGPROG_CHAIN_WORDS]: frame, first scan record, number of scan records (run in that order), 0.
 *   info    : int32 [frames], zeroed by the caller: the status bits of the frame's chains. A chain ends at its first status bit.
 * An AC chain never stores coefficient 0, a DC chain nothing else, every store is 16 bits wide: all chains may share one launch.
 * Returns -2 for an argument error (before any launch), -3 when the launch would exceed a grid dimension; `data_bytes`, `nscans`,
 * `coef_elems` and the geometry bound every access, and a record that does not fit them sets MG_JPEGPROG_ST_RECORD.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_JPEGPROG_THREADS 64
#define MG_JPEGPROG_SCAN_WORDS 480
#define MG_JPEGPROG_CHAIN_WORDS 4
#define MG_JPEGPROG_ST_REFINE 32  /* a refinement symbol whose size is not 1, or a new value past the end of the band */
#define MG_JPEGPROG_ST_EXTRA 64   /* whole bytes of a scan's segment left behind its last block */
#define MG_JPEGPROG_ST_RECORD 128 /* a scan or chain record outside the buffers or the geometry */
int mg_jpegprog_limits(int* threads, int* scan_words, int* chain_words);
int mg_jpegprog_chains(const uint8_t* data, long data_bytes, const int32_t* scans, long nscans, const int32_t* chains, long nchains, int16_t* coef,
                       long coef_elems, int32_t* info, long frames, int h, int w, int layout, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * PNG decoding (csrc/pngdec.hip): the zlib streams (concatenated IDAT payloads) of `planes` non-interlaced files of one size -> the L plane of
 * Image.open(path).convert("L") on the device. Replaces the alpha / mask half of T.Load (maggie/dataloader/transforms.py:47-50). DESIGN.md
 * section 26. Colour type 0 and 3 at depth 1, 2, 4, 8; colour type 2, 4, 6 at depth 8.
 *   recs    : int32 [planes][MG_PNGDEC_REC_WORDS], one record per file: [0] the offset of its zlib stream in `data`, [1] the stream's length
 *             (the two header bytes and the Adler-32 trailer included), [2] colour type, [3] bit depth, [4] the number of palette entries
 *             (256 for grey), [8..71] the 256-entry L table as bytes (grey: sample * 255 / (2^depth - 1); palette: L of each PLTE entry).
 *   raw     : uint8 [planes][raw_stride], the inflated bytes h x (1 + rowbytes) of each file at the start of its slice; raw_stride a multiple
 *             of 16 that holds the largest of them, `raw` 16-byte aligned, `data` 4-byte aligned.
 *   info    : int32 [planes][MG_PNGDEC_INFO_WORDS], zeroed by the caller: [0] status bits (both kernels), [1] rounds, [2] deflate blocks,
 *             [3] tokens, [4] the Adler-32 computed, [5] the Adler-32 of the trailer.
 *   mg_pngdec_inflate  : one wave per file; RFC 1951 in rounds of at most MG_PNGDEC_ROUND_TOKENS tokens (a stored block: one round per 2048 bytes).
 *   mg_pngdec_unfilter : raw -> out uint8 [planes][h][w]; skips a file whose status is not 0.
 * Each returns -2 for an argument error (before any launch), -3 when the launch would exceed a grid dimension. Every access is bounded by
 * `data_bytes`, `raw_stride` and h, w; a record that does not fit them sets MG_PNGDEC_ST_RECORD.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_PNGDEC_THREADS 64
#define MG_PNGDEC_REC_WORDS 72
#define MG_PNGDEC_INFO_WORDS 8
#define MG_PNGDEC_ROUND_TOKENS 64
#define MG_PNGDEC_FLUSH_BYTES 4096
#define MG_PNGDEC_MAX_SIDE 32767
#define MG_PNGDEC_MAX_ROWBYTES 16384 /* the row that a band hands to the next stays in LDS */
#define MG_PNGDEC_MAX_BYTES (1L << 28)
#define MG_PNGDEC_MAX_RAW (1L << 30)
#define MG_PNGDEC_ST_PAST_END 1    /* a read past the end of the stream */
#define MG_PNGDEC_ST_SIZE 2        /* more or fewer bytes than h x (1 + rowbytes) */
#define MG_PNGDEC_ST_DISTANCE 4    /* a distance beyond the bytes produced */
#define MG_PNGDEC_ST_BLOCK_TYPE 8  /* the reserved block type */
#define MG_PNGDEC_ST_STORED_LEN 16 /* LEN != ~NLEN */
#define MG_PNGDEC_ST_CODE_SET 32   /* a code set that zlib refuses */
#define MG_PNGDEC_ST_SYMBOL 64     /* an unassigned code, literal/length symbol 286 / 287 or distance symbol 30 / 31 */
#define MG_PNGDEC_ST_ADLER 128     /* the Adler-32 of the inflated bytes is not the trailer's */
#define MG_PNGDEC_ST_FILTER 256    /* a filter type above 4 */
#define MG_PNGDEC_ST_INDEX 512     /* a palette index past PLTE's last entry */
#define MG_PNGDEC_ST_RECORD 1024   /* a record outside data_bytes / raw_stride, or an unsupported colour type and depth */
int mg_pngdec_limits(int* threads, int* max_side, int* max_rowbytes, int* rec_words, int* info_words, int* round_tokens, int* flush_bytes);
int mg_pngdec_inflate(const uint8_t* data, long data_bytes, const int32_t* recs, uint8_t* raw, long raw_stride, int32_t* info, long planes, int h,
                      int w, void* stream);
int mg_pngdec_unfilter(const uint8_t* raw, long raw_stride, const int32_t* recs, uint8_t* out, int32_t* info, long planes, int h, int w,
                       void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * PNG frames and planes of every legal file (csrc/pngcolor.hip): the zlib streams of `files` files of one size -- any of the 15 (colour type,
 * bit depth) pairs, Adam7 interlaced or not, per file -- -> Image.open(path).convert("RGB") or .convert("L") on the device. Replaces the frame
 * half of T.Load for .png files (maggie/dataloader/transforms.py:47-50). DESIGN.md section 34. Grey 16 converts as min(v, 255) (Pillow's I;16),
 * every other 16-bit sample as its high byte; alpha and tRNS are dropped.
 *   recs    : int32 [files][MG_PNGCOLOR_REC_WORDS]: [0] the offset of the zlib stream in `data`, [1] its length, [2] colour type, [3] bit depth,
 *             [4] palette entries (256 without a palette), [5] interlace (0 / 1), [6] the inflated size: the sum over the non-empty passes of
 *             ph x (1 + rb), [7] 0, [_REC_PASSES + 4 k ..] pass k (7 for Adam7, else 1; the rest zero): pw, ph, rb, byte offset in the file's `raw`
 *             slice, with pw = ceil((w - x0) / dx), ph = ceil((h - y0) / dy), rb = ceil(pw x channels x depth / 8) (the kernels recompute the
 *             table and refuse a record that differs), [_REC_LTABLE ..] the L of each palette entry as 256 bytes, [_REC_PALETTE ..] 256 x 3
 *             palette bytes.
 *   raw     : uint8 [files][raw_stride] as for mg_pngdec_*; mg_pngcolor_unfilter reconstructs the scanlines IN PLACE (filter type bytes stay).
 *   info    : int32 [files][MG_PNGDEC_INFO_WORDS], zeroed by the caller; the words and the MG_PNGDEC_ST_* bits of mg_pngdec_*.
 *   mg_pngcolor_inflate  : mg_pngdec_inflate's algorithm (csrc/png_inflate.h), expecting recs[6] bytes.
 *   mg_pngcolor_unfilter : one wave per (file, pass); a filter type above 4 sets MG_PNGDEC_ST_FILTER and decodes as type 0.
 *   mg_pngcolor_convert  : raw -> out, `mode` _OUT_RGB uint8 [files][h][w][3], _OUT_L uint8 [files][h][w] (`out` at any byte), _OUT_NORM float32
 *             [files][3][h][w] = (v / 255 - mean[c]) / std[c] with IEEE divisions (`mean`, `std`: 3 host floats; `out` 4-byte aligned). Skips a
 *             file whose status is not 0; a palette index past the last entry sets MG_PNGDEC_ST_INDEX.
 * Each returns -2 for an argument error (before any launch; a destination overlapping `raw` is one), -3 when the launch would exceed a grid
 * dimension. Every access is bounded by `data_bytes`, `raw_stride` and h, w; a record that does not fit them sets MG_PNGDEC_ST_RECORD.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_PNGCOLOR_REC_WORDS 292
#define MG_PNGCOLOR_REC_PASSES 8
#define MG_PNGCOLOR_REC_LTABLE 36
#define MG_PNGCOLOR_REC_PALETTE 100
#define MG_PNGCOLOR_MAX_ROWBYTES 32768 /* RGBA 16 at 3840 pixels is 30720; the carry row of a band stays in LDS */
#define MG_PNGCOLOR_GROUP 16           /* pixels of a lane of mg_pngcolor_convert */
#define MG_PNGCOLOR_OUT_RGB 0
#define MG_PNGCOLOR_OUT_L 1
#define MG_PNGCOLOR_OUT_NORM 2
int mg_pngcolor_limits(int* threads, int* max_side, int* max_rowbytes, int* rec_words, int* info_words, int* group);
int mg_pngcolor_inflate(const uint8_t* data, long data_bytes, const int32_t* recs, uint8_t* raw, long raw_stride, int32_t* info, long files, int h,
                        int w, void* stream);
int mg_pngcolor_unfilter(uint8_t* raw, long raw_stride, const int32_t* recs, int32_t* info, long files, int h, int w, void* stream);
int mg_pngcolor_convert(const uint8_t* raw, long raw_stride, const int32_t* recs, void* out, int32_t* info, long files, int h, int w, int mode,
                        const float* mean, const float* std, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * PNG encoding (csrc/pngenc.hip): `nplanes` planes of one size [nplanes][h][w] -> the zlib streams (78 01, deflate, Adler-32) of 8-bit
 * greyscale, non-interlaced PNG files, Sub filter on every row, packed back to back. Replaces the pixel pass of the result writer
 * (maggie/engine/test.py:20-68). The host adds the signature, IHDR, the IDAT length and CRC, and IEND. DESIGN.md section 27.
 *   mode    : MG_PNGENC_MODE_U8 uint8 samples; _UNIT float32, byte = (uint8)(x * 255.0f), NaN and x < 0 -> 0, x > 1 -> 255;
 *             _THRESHOLD float32, byte = x > 0.5f ? 255 : 0. float planes 4-byte aligned.
 *   blocks  : the filtered stream of a plane, h x (1 + w) bytes, is cut into ceil(h (1 + w) / MG_PNGENC_BLOCK_BYTES) deflate blocks; one
 *             workgroup of MG_PNGENC_THREADS lanes per block. Tokens are runs (distance 1) inside a block.
 *   recs    : int32 [nplanes][blocks][MG_PNGENC_REC_WORDS], written by mg_pngenc_size: [0] 1 fixed / 2 dynamic, [1] the block's bits (header
 *             and end-of-block included), [2] its bytes, [3] its tokens, [4] sum b mod 65521, [5] sum (n - i) b_i mod 65521 (the Adler-32
 *             partials), [6] literal/length codes sent, [7] code-length codes sent, [8..80) the 286 literal/length code lengths of the dynamic
 *             construction as bytes, [80..85) the 19 code-length code lengths as bytes, the rest 0.
 *   sizes   : int64 [nplanes], written by mg_pngenc_size: the bytes of each plane's zlib stream. 8-byte aligned.
 *   mg_pngenc_emit : `out` zeroed by the caller, 16-byte aligned, `out_bytes` a multiple of 4 and at least the sum of `sizes`; plane p's
 *             stream starts at the sum of sizes[0..p). Runs after mg_pngenc_size on the same stream with the same planes, recs and sizes.
 * Each returns -2 for an argument error (before any launch: null or misaligned pointers, a mode, a side or a plane count out of range),
 * -3 when nplanes x blocks exceeds 2^31 - 1. Every access is bounded by nplanes, h, w and out_bytes.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_PNGENC_THREADS 256
#define MG_PNGENC_BLOCK_BYTES 16384
#define MG_PNGENC_REC_WORDS 88
#define MG_PNGENC_MAX_SIDE 32767             /* MG_PNGDEC_MAX_SIDE: the device decoder reads back what this writes */
#define MG_PNGENC_MAX_WIDTH 16384            /* MG_PNGDEC_MAX_ROWBYTES */
#define MG_PNGENC_MAX_RAW ((1L << 30) - 16)  /* h x (1 + w), as pngdec.parse accepts it */
#define MG_PNGENC_MAX_PLANES 65536
#define MG_PNGENC_MODE_U8 0
#define MG_PNGENC_MODE_UNIT 1
#define MG_PNGENC_MODE_THRESHOLD 2
int mg_pngenc_limits(int* threads, int* block_bytes, int* rec_words, int* max_side, int* max_width, int* max_planes);
int mg_pngenc_size(const void* planes, int mode, long nplanes, int h, int w, int32_t* recs, int64_t* sizes, void* stream);
int mg_pngenc_emit(const void* planes, int mode, long nplanes, int h, int w, const int32_t* recs, const int64_t* sizes, uint8_t* out,
                   long out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Baseline JPEG encoding (csrc/jpegenc.hip): `frames` RGB frames of one size [frames][h][w][3] uint8 -> the entropy-coded segments (stuffed,
 * with EOI) of the files Pillow's Image.save(path, quality=q) writes: 4:2:0, the Annex K Huffman tables, no optimisation, no restart markers.
 * Replaces the pixel pass behind the synthesis tools' .save('....jpg') (tools/synthesize_image_him.py:93-109, synthesize_video_him.py:189).
 * The host adds the 623 header bytes. DESIGN.md section 28. With mx = ceil(w / 16), my = ceil(h / 16): blocks = 6 mx my per frame.
 *   lut, noise, qtab : the operands of mg_jpeg_ycc (lut uint8 [3][256] or null; noise int16 [h][w][noise_channels] or null; qtab int32 [2][64]
 *             natural order, entries clamped to 1..255).
 *   coef    : int16 [frames][blocks][64], 16-byte aligned, `coef_elems` = frames x blocks x 64: MCUs row by row, y0 y1 y2 y3 cb cr in an MCU,
 *             natural order inside a block, DC terms NOT differenced -- the layout mg_jpegdec_dcsum leaves. A luma block beyond ceil(w / 8)
 *             block columns or ceil(h / 8) block rows is a dummy block: AC terms 0, DC = the DC of the block before it in the MCU.
 *   bits    : int32 [frames][blocks], the bits of each block in the scan; offs int64 [frames][blocks], their exclusive sum per frame.
 *   sizes   : int64 [4][frames]: [0] the bytes of the frame's scan in the file (stuffed, + 2 for EOI), [1] its unstuffed bytes, [2] its bits,
 *             [3] the exclusive sum of [0]: where the frame's scan starts in `out`. [1], [2] by mg_jpegenc_bits, [0], [3] by mg_jpegenc_pack.
 *   raw     : uint8 [frames][raw_stride], ZEROED by the caller, 16-byte aligned: each frame's unstuffed stream at the start of its slice, the
 *             last byte filled with 1-bits. raw_stride a multiple of 16, at least ceil(blocks x MG_JPEGENC_MAX_BLOCK_BITS / 8) + 4 rounded up to 16.
 *   ffcount : int32 [frames][chunks], choff int64 [frames][chunks], chunks = ceil(raw_stride / MG_JPEGENC_CHUNK_BYTES): the 0xFF bytes of each
 *             chunk of the unstuffed stream and their exclusive sum per frame (written for the chunks the stream reaches).
 *   mg_jpegenc_stuff : raw -> out, a 0x00 behind every 0xFF, FF D9 behind the last byte; `out_bytes` bounds every store; `grid_chunks` in
 *             1..chunks: the chunks launched per frame, at least ceil(max sizes[1] / MG_JPEGENC_CHUNK_BYTES).
 * The entries run in this order on one stream. Each returns -2 for an argument error (before any launch: null or misaligned pointers, a size or a
 * frame count out of range, a coef_elems or raw_stride that does not fit the geometry), -3 when a launch would exceed 2^31 - 1 workgroups.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_JPEGENC_THREADS 256
#define MG_JPEGENC_PACK_BLOCKS 64        /* blocks of a packing workgroup: an LDS image of 64 x 1658 bits, 13 KiB */
#define MG_JPEGENC_CHUNK_BYTES 4096      /* a stuffing chunk: 16 bytes a lane */
#define MG_JPEGENC_MAX_BLOCK_BITS 1658   /* DC 9 + 11, 63 AC terms of 16 + 10 */
#define MG_JPEGENC_MAX_FRAMES 4096
int mg_jpegenc_limits(int* threads, int* pack_blocks, int* chunk_bytes, int* max_block_bits, int* max_side, int* max_frames);
int mg_jpegenc_coef(const uint8_t* in, const uint8_t* lut, const int16_t* noise, int noise_channels, const int32_t* qtab, int16_t* coef,
                    long coef_elems, long frames, int h, int w, void* stream);
int mg_jpegenc_bits(const int16_t* coef, long coef_elems, int32_t* bits, int64_t* offs, int64_t* sizes, long frames, int h, int w, void* stream);
int mg_jpegenc_pack(const int16_t* coef, long coef_elems, const int32_t* bits, const int64_t* offs, int64_t* sizes, uint8_t* raw, long raw_stride,
                    int32_t* ffcount, int64_t* choff, long frames, int h, int w, void* stream);
int mg_jpegenc_stuff(const uint8_t* raw, long raw_stride, const int64_t* choff, const int64_t* sizes, uint8_t* out, long out_bytes, long frames,
                     int h, int w, long grid_chunks, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Matte output (csrc/matteout.hip): the pixel passes of the reference's predictor behind the forward (demo/maggie_predictor.py:35-40,62-76,
 * 121-157; demo/app.py:58-65). DESIGN.md section 29. All four are compiled without floating-point contraction; none reads anything back or
 * synchronises, so each can be captured in a graph. A lane owns MG_MATTE_GROUP consecutive pixels and moves them 16 bytes at a time; a base of
 * any alignment is accepted (the 16-byte accesses then run unaligned), except where stated.
 *   mg_matte_composite : alpha fp32 [frames * P][Hin][Win] (4-byte aligned) at the network's size -> per output pixel of [H][W] the bilinear
 *             value (align_corners) over the top-left crop_h x crop_w region, as mg_postprocess_alpha states it but with every operation
 *             rounded on its own; H == crop_h and W == crop_w copies the value bit for bit; nothing beyond the crop is read. `snap` != 0:
 *             <= 1/255 -> 0, >= 254/255 -> 1. Then per channel of frames_u8 [frames][H][W][3]: t1 = f32(v) * a, t2 = (1 - a) * f32(bg),
 *             s = t1 + t2, each rounded to fp32; out = trunc(clamp(s, 0, 255)), uint8 [frames * P][H][W][3]. The background is `bg_image`
 *             uint8 [bg_frames][H][W][3] with bg_frames 1 (shared by all frames) or `frames`, or, when bg_image is null, the colour
 *             (bg_r, bg_g, bg_b), each 0..255. `alpha_out`, when given, receives the fp32 [frames * P][H][W] alpha that was used. A frame's
 *             bytes are loaded once for its P instances. Hin x Win and 3 H W must fit 31 bits.
 *   mg_matte_overlay   : frames_u8 [frames][H][W][3], masks uint8 [frames][H][W], alpha in [0, 1] -> out [frames][H][W][3] =
 *             trunc(f32(in1) + alpha * f32(in2 - in1)) with in2 = (r, g, b) where mask > 0, else 0: PIL.Image.blend(image, palette(mask), alpha).
 *   mg_matte_label_ids : a label map of n elements, uint8 (elem_bytes 1) or int32 (elem_bytes 4) -> presence uint32
 *             [MG_MATTE_PRESENCE_WORDS], zeroed by the call: bit (id & 31) of word (id >> 5) for every id 0..255 of the map; word 8 is
 *             nonzero when an int32 label lies outside 0..255. An LDS bitmap per workgroup, ORed into the device words with atomics.
 *   mg_matte_label_planes : planes uint8 [n_ids][n], 255 where the map equals ids[k], else 0; `ids` is a HOST array of n_ids <= 256 bytes.
 * Each returns -2 for an argument error before any launch (a null pointer, a size, a crop, a colour, an alpha or an element size out of range,
 * a misaligned fp32 or int32 base), -3 for more than 65535 frames in mg_matte_composite.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_MATTE_THREADS 256
#define MG_MATTE_GROUP 16                /* pixels of a lane: 48 frame bytes, three 16-byte loads and stores */
#define MG_MATTE_MAX_BLOCKS 16384        /* workgroups along x; the kernels stride over what is left */
#define MG_MATTE_PRESENCE_WORDS 9
int mg_matte_composite(const float* alpha, long frames, int P, int Hin, int Win, int crop_h, int crop_w, int H, int W, int snap,
                       const uint8_t* frames_u8, const uint8_t* bg_image, long bg_frames, int bg_r, int bg_g, int bg_b, uint8_t* out,
                       float* alpha_out, void* stream);
int mg_matte_overlay(const uint8_t* frames_u8, const uint8_t* masks, long frames, int H, int W, int r, int g, int b, float alpha, uint8_t* out,
                     void* stream);
int mg_matte_label_ids(const void* map, int elem_bytes, long n, uint32_t* presence, void* stream);
int mg_matte_label_planes(const void* map, int elem_bytes, long n, const uint8_t* ids, int n_ids, uint8_t* planes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Background compositing (csrc/background.hip): LoadRandomBackground -> HistogramMatching -> ComposeBackground of the reference
 * (maggie/dataloader/transforms.py:307-370,841-864) on uint8 tensors. DESIGN.md section 32. The file is compiled without floating-point
 * contraction; nothing reads back or synchronises, so the chain can be captured in a graph.
 *   mg_bg_blur_crop : bg uint8 [bh][bw][3] -> out uint8 [h][w][3], the window at (x, y) of the separable integer Gaussian of the WHOLE
 *             background: horizontal sums s1 = sum_k q_k v (16 bits, <= 255 * 256), vertical sums s2 = sum_k q_k s1 (32 bits),
 *             out = (s2 + 32768) >> 16; border BORDER_REFLECT_101 on the background, repeated for sides below the reach. Only the window's
 *             pixels are computed. `win` is a DEVICE int32 [MG_BG_WIN_TABLE]: [0] = ksize (odd, 1..MG_BG_MAX_KSIZE; 1 with the tap 256 is the
 *             plain copy), [1] = x, [2] = y, [3] = 0, then ksize taps q_k >= 0 that sum to 256. The launch does not depend on the table; the
 *             kernel clamps ksize to odd 1..25, x to 0..bw - w, y to 0..bh - h and each tap to 0..256. Needs w <= bw, h <= bh.
 *   mg_bg_hist      : frames uint8 [pixels][3] -> counts uint32 [3][256] += the per-channel counts. The counts ACCUMULATE: the caller
 *             zeroes them. Per-wave bins in LDS, runs of equal bytes added at once, integer atomics into the counts. pixels < 2^31.
 *   mg_bg_match_lut : the tone curves of skimage.exposure.match_histograms (float branch) followed by the reference's blend, from the two
 *             histograms [3][256]: luts uint8 [2][3][256], [0] the foreground's curve, [1] the background's. `draw` is a DEVICE fp32 [4]:
 *             f32(ratio), f32(1. - ratio), match_bg (0 or 1), 0. The matched side is the foreground (match_bg 0: towards the background's
 *             histogram) or the background; the other side and byte values that do not occur are the identity. One workgroup.
 *   mg_bg_compose   : out[t] = uint8(clip(f64(lutF[fg]) * wt[a][0] + f64(lutB[bg]) * wt[a][1], 0, 255)), fg uint8 [frames][h][w][3], alpha
 *             uint8 [frames][h][w], bg uint8 [bg_frames][h][w][3] with bg_frames 1 (shared) or `frames`; `luts` uint8 [2][3][256] or null
 *             (identities); `wt` DEVICE fp64 [256][2] = a / 255.0, 1 - a / 255.0. `fg_out` [frames][h][w][3] and `bg_out` [bg_frames][h][w][3],
 *             when given, receive lutF[fg] and lutB[bg]. A lane owns MG_MATTE_GROUP pixels at any base alignment.
 * Each returns -2 for an argument error before any launch, -3 when the launch would exceed a grid dimension. mg_bg_limits reports the
 * constants below to a binding that mirrors them.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_BG_MAX_KSIZE 25
#define MG_BG_WIN_TABLE 32
#define MG_BG_TILE_ROWS 16
#define MG_BG_TILE_COLS 64
#define MG_BG_THREADS 256
#define MG_BG_MAX_SIDE 32767
#define MG_BG_HIST_MAX_BLOCKS 2048
int mg_bg_blur_crop(const uint8_t* bg, int bh, int bw, const int32_t* win, uint8_t* out, int h, int w, void* stream);
int mg_bg_hist(const uint8_t* frames, long pixels, uint32_t* counts, void* stream);
int mg_bg_match_lut(const uint32_t* hist_fg, const uint32_t* hist_bg, const float* draw, uint8_t* luts, void* stream);
int mg_bg_compose(const uint8_t* fg, const uint8_t* alpha, const uint8_t* bg, long bg_frames, long frames, int h, int w, const uint8_t* luts,
                  const double* wt, uint8_t* out, uint8_t* fg_out, uint8_t* bg_out, void* stream);
int mg_bg_limits(int* max_ksize, int* win_table, int* tile_rows, int* tile_cols, int* max_side);

/* ---------------------------------------------------------------------------------------------------------------
 * Colour PNG encoding (csrc/pngenc.hip): `nimages` images of one size [nimages][h][w][channels] uint8, channels 3 (colour type 2) or 4
 * (colour type 6) -> the zlib streams of 8-bit non-interlaced files, Sub filter on every row with the filter distance `channels`. Only the
 * filtered stream differs from the grey entries: a row is 01 and channels x w bytes, byte j of it minus byte j - channels (j >= channels).
 * Blocks, records, sizes, the blob and the return codes are those of mg_pngenc_size / mg_pngenc_emit with a row of channels x w bytes:
 * channels x w <= MG_PNGENC_MAX_WIDTH and h x (1 + channels x w) <= MG_PNGENC_MAX_RAW. DESIGN.md section 35.
 * ------------------------------------------------------------------------------------------------------------- */
int mg_pngenc_size_rgb(const uint8_t* images, int channels, long nimages, int h, int w, int32_t* recs, int64_t* sizes, void* stream);
int mg_pngenc_emit_rgb(const uint8_t* images, int channels, long nimages, int h, int w, const int32_t* recs, const int64_t* sizes, uint8_t* out,
                       long out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Cut-outs (csrc/cutout.hip): the foreground colour of every instance by the blur-fusion estimator (Forte & Pitie, ICIP 2021) stated on
 * bytes, two passes with the radii r0 then r1, and the straight RGBA image. DESIGN.md section 35 is the statement. The file is compiled
 * without floating-point contraction; nothing reads back or synchronises and the launches form one chain, so a call can be captured in a graph.
 *   mg_cutout_alpha_bytes : fp32 [n] (4-byte aligned) -> uint8 [n], byte = (uint8)(x * 255.0f), NaN and x < 0 -> 0, x >= 1 -> 255
 *             (MG_PNGENC_MODE_UNIT).
 *   mg_cutout_estimate : frames_u8 [frames][H][W][3], alpha_u8 [frames * P][H][W] -> out uint8 [frames * P][H][W][out_channels]:
 *             out_channels 3 the estimate F, 4 (out 4-byte aligned) the cut-out (F, a) with F = 0 where a == 0. One pass P(I, F, B, a, r):
 *             window [y - r/2, y - r/2 + r) x [x - r/2, x - r/2 + r), indices reflected without repeating the edge (period 2 (n - 1),
 *             as often as needed); SA = sum a, SFA = sum F a, SBA = sum B (255 - a), exact integers < 2^32; then in fp64, every
 *             operation rounded on its own: ba = SA / (255 r r), bF = (SFA / (65025 r r)) / (ba + 1e-5),
 *             bB = (SBA / (65025 r r)) / ((1 - ba) + 1e-5), al = a / 255, i = I / 255, f = bF + al ((i - al bF) - (1 - al) bB);
 *             F' = floor(clip(f, 0, 1) 255 + 0.5), B' = floor(clip(bB, 0, 1) 255 + 0.5). The estimate is F1, B1 = P(I, I, I, a, r0),
 *             F = P(I, F1, B1, a, r1). Scratch, all caller-owned, for `chunk` >= 1 planes at a time: rows uint32 [chunk][7][H][W]
 *             (4-byte aligned), f1 and b1 uint8 [chunk][H][W][3]. 4 launches per chunk.
 * Each returns -2 for an argument error before any launch (a null pointer, a side outside 1..MG_CUTOUT_MAX_SIDE, a radius outside
 * 1..MG_CUTOUT_MAX_RADIUS, a channel count, a misaligned base).
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_CUTOUT_THREADS 256
#define MG_CUTOUT_TILE 256               /* columns of a row-sum workgroup: 2 x 7 x (256 + 254) uint32 of LDS, 28 560 bytes */
#define MG_CUTOUT_GROUP 8                /* neighbours added first when a window has 16 taps or more */
#define MG_CUTOUT_STRIP 32               /* rows a column lane walks down; twice as many for windows of 32 rows and more */
#define MG_CUTOUT_MAX_RADIUS 255
#define MG_CUTOUT_MAX_SIDE 32767
int mg_cutout_limits(int* threads, int* tile, int* strip, int* max_radius, int* max_side);
int mg_cutout_alpha_bytes(const float* alpha, long n, uint8_t* out, void* stream);
int mg_cutout_estimate(const uint8_t* frames_u8, const uint8_t* alpha_u8, long frames, int P, int H, int W, int r0, int r1, uint32_t* rows,
                       uint8_t* f1, uint8_t* b1, long chunk, uint8_t* out, int out_channels, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Full-size mattes (csrc/refine.hip): the fast guided filter (He & Sun) stated on bytes. A local linear model alpha ~ a . I + b is fitted at
 * the network's size and its averaged coefficients, brought to full size bilinearly, are applied to the full-size frame. DESIGN.md section 36
 * is the statement, tests/refine_restatement.py the same arithmetic in NumPy and the byte-for-byte oracle. The file is compiled without
 * floating-point contraction and uses no fp32 between the sums and the bytes; nothing reads back or synchronises and the launches of an entry
 * form one chain, so both entries can be captured in a graph. No equality with a float implementation is claimed.
 *   Inputs per frame: I uint8 [H][W][3] (full size), the guide G uint8 [h][w][3] (the frame as the network saw it), per instance p uint8 [h][w].
 *   Parameters: window side r, 1..MG_REFINE_MAX_RADIUS, n = r r; eps, MG_REFINE_MIN_EPS..1, in units of the squared [0, 1] range.
 *   1. Window [y - r/2, y - r/2 + r) x [x - r/2, x - r/2 + r) (integer division), indices reflected without repeating the edge (period
 *      2 (len - 1), as often as needed; an axis of length 1 maps everything to 0).
 *   2. Window sums, exact integers < 2^32: per frame SI_c (3) and SII_cd, c <= d (6), of G_c G_d; per instance Sp and SIp_c (3) of G_c p.
 *   3. Per low-resolution pixel in fp64, every operation rounded on its own, in this order:
 *      m_c = SI_c / (255.0 n), mp = Sp / (255.0 n); s_cd = SII_cd / (65025.0 n) - m_c m_d, then s_cc = s_cc + eps;
 *      k_c = SIp_c / (65025.0 n) - m_c mp;
 *      c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11, c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12,
 *      c22 = s00 s11 - s01 s01; det = (s00 c00 + s01 c01) + s02 c02;
 *      a_0 = ((c00 k_0 + c01 k_1) + c02 k_2) / det, a_1 with the row (c01, c11, c12), a_2 with the row (c02, c12, c22);
 *      b = mp - ((a_0 m_0 + a_1 m_1) + a_2 m_2);
 *      A_c = floor(clip(a_c, -256, 256) 65536.0 + 0.5), B = floor(clip(b, -1024, 1024) 65536.0 + 0.5), integers (16 fractional bits).
 *      The model gives |a| <= 0.25 / sqrt(eps) <= 250 for eps >= 1e-6 and |b| <= 1 + 3 |a|: the two clips are guards that never act.
 *   4. The same window over A_c and B: exact integer sums, |sum| < 2^39; abar_c = (double)sum A_c / (n 65536.0), bbar likewise, one division each.
 *   5. To full size. Along x: ratio = w / W (fp64), s = (X + 0.5) ratio - 0.5 clamped to [0, w - 1], x0 = floor(s), x1 = min(x0 + 1, w - 1),
 *      fx = s - x0; the y axis likewise with h / H. For a plane v: top = v[y0][x0] (1 - fx) + v[y0][x1] fx, bot likewise on row y1,
 *      up(v) = top (1 - fy) + bot fy. q = ((up(bbar) + up(abar_0) i_0) + up(abar_1) i_1) + up(abar_2) i_2 with i_c = I_c / 255.0;
 *      byte = floor(clip(q, 0, 1) 255.0 + 0.5); with snap a byte <= 1 becomes 0 and a byte >= 254 becomes 255.
 *   mg_refine_coefficients : guide [frames][h][w][3], alpha_u8 [frames * P][h][w] -> means fp64 [frames * P][4][h][w] = (abar_0, abar_1,
 *             abar_2, bbar), steps 1-4. Scratch, all caller-owned: grows and gsums uint32 [frames][9][h][w] (planes SI_0..2, SII_00, 01, 02,
 *             11, 12, 22; 4-byte aligned), prows uint32 [frames * P][4][h][w], coef int32 [frames * P][4][h][w] (A_0..2, B), crows int64
 *             [frames * P][4][h][w] and means (8-byte aligned). 6 launches.
 *   mg_refine_apply : frames_u8 [frames][H][W][3], means -> out uint8 [frames * P][H][W] and/or outf fp32 [frames * P][H][W] = byte / 255.0f
 *             (either may be null, not both), step 5 in one launch: a lane owns MG_REFINE_LANE_PIXELS consecutive pixels of one row, loads
 *             their frame bytes once and loops over the frame's instances. xi int32 [W] / xf fp64 [W] hold x0 / fx, yi [H] / yf [H] hold
 *             y0 / fy (made on the host in fp64; an index outside the plane is clamped into it by the kernel).
 * Each returns -2 for an argument error before any launch (a null pointer, a side outside 1..MG_CUTOUT_MAX_SIDE, a side of the window outside
 * 1..MG_REFINE_MAX_RADIUS, an eps outside MG_REFINE_MIN_EPS..1, a misaligned base); frames * P == 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------------------------- */
#define MG_REFINE_THREADS 256
#define MG_REFINE_TILE 256               /* columns of a row-sum workgroup: 9 x (256 + 63) uint32 of LDS, 11 484 bytes */
#define MG_REFINE_STRIP 32               /* rows a column lane walks down */
#define MG_REFINE_MAX_RADIUS 64
#define MG_REFINE_LANE_PIXELS 4
#define MG_REFINE_MIN_EPS 1e-6
int mg_refine_limits(int* threads, int* tile, int* strip, int* max_radius, int* max_side, int* lane_pixels);
int mg_refine_coefficients(const uint8_t* guide_u8, const uint8_t* alpha_u8, long frames, int P, int h, int w, int r, double eps, uint32_t* grows,
                           uint32_t* gsums, uint32_t* prows, int32_t* coef, int64_t* crows, double* means, void* stream);
int mg_refine_apply(const uint8_t* frames_u8, const double* means, long frames, int P, int h, int w, int H, int W, const int32_t* xi,
                    const double* xf, const int32_t* yi, const double* yf, int snap, uint8_t* out, float* outf, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGGIE_HIP_H */
