// BatchNorm (training statistics, folding, apply+activation+residual, backward) and related row x channel
// elementwise kernels for NHWC / sparse-row feature matrices on gfx950. All are HBM-bound: 16-byte vector accesses,
// per-thread fixed channel group so per-channel parameters live in registers, column reductions finished with one
// atomicAdd per channel per block.
// Replaces nn.BatchNorm2d / nn.BatchNorm1d (+ReLU / LeakyReLU / residual adds) of
//   maggie/network/encoder/resnet.py:23-39,167-175; maggie/network/decoder/resnet.py:28-45;
//   maggie/network/module/aspp.py:34-56; maggie/network/decoder/resnet_inst_matt_spconv.py:69-130.
#include <stdlib.h>
#include "common.h"
#include "launch.h"
#include "../../include/maggie_hip.h"

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------------
// Column reductions over a (M x C) row-major matrix. Grid = (row blocks, channel groups): a block owns TX 16-byte channel
// chunks (<= 8, i.e. one 128-byte line of bf16) and TY = 256/TX row lanes, so deep layers (few rows, many channels) still
// fill the chip. Per-thread register partials -> LDS [TY][TX*CE*NACC] -> one global atomicAdd per channel per block.
// ---------------------------------------------------------------------------------------------------
struct ColGeom {
    int tx, ty, groups, rb, rpb;
};
static inline ColGeom col_geom(int M, int C, int ce, int max_rb, int nt = NT, int rpt = 4) {
    ColGeom g;
    const int cpr = C / ce;
    g.tx = cpr < 8 ? cpr : 8;
    g.ty = nt / g.tx;
    g.groups = (cpr + g.tx - 1) / g.tx;
    int want = 1024 / g.groups; if (want < 1) want = 1; if (want > max_rb) want = max_rb;
    int rb = (M + g.ty * rpt - 1) / (g.ty * rpt); if (rb < 1) rb = 1; if (rb > want) rb = want;
    g.rpb = (M + rb - 1) / rb;
    g.rb = (M + g.rpb - 1) / g.rpb;
    return g;
}

// `slot` (deterministic mode, csrc/det.hip): this workgroup's row [NACC][C] of the slot buffer -- the partial is STORED there (every row
// block owns its row; mg_det_reduce adds the rows in index order) instead of being added to dst0 / dst1 atomically.
template <int NV>
__device__ __forceinline__ void col_block_reduce(float* sred, const float* part, int tx, int ty, int ix, int iy, bool active,
                                                 float* __restrict__ dst0, float* __restrict__ dst1, int c_base, int C, int ce,
                                                 float* __restrict__ slot = nullptr) {
    // sred: [ty][tx*NV]; part: this thread's NV values (NV = ce * NACC, channel-major: [acc][e])
    const int width = tx * NV;
    if (active) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sred[iy * width + ix * NV + k] = part[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < width; j += (int)blockDim.x) {
        float acc = 0.f;
        for (int r = 0; r < ty; ++r) acc += sred[r * width + j];
        const int cx = j / NV, k = j - cx * NV, a = k / ce, e = k - a * ce;
        const int c = c_base + cx * ce + e;
        if (c < C) {
            if (slot) slot[a * C + c] = acc;
            else atomicAdd((a == 0 ? dst0 : dst1) + c, acc);
        }
    }
}

// the same reduction for the 1024-thread blocks (tx a power of two): rows of a wave first meet in registers (butterfly over the lanes that share a
// channel chunk), so LDS holds one row per WAVE instead of one per thread row (64 KB -> 8 KB at 1024 threads)
template <int NV>
__device__ __forceinline__ void col_block_reduce_wave(float* sred, float* part, int tx, int ix, bool active,
                                                      float* __restrict__ dst0, float* __restrict__ dst1, int c_base, int C, int ce,
                                                      float* __restrict__ slot = nullptr) {
    const int width = tx * NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    for (int off = tx; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < NV; ++k) part[k] += __shfl_xor(part[k], off);
    }
    if (lane < tx && active) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sred[wave * width + ix * NV + k] = part[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < width; j += (int)blockDim.x) {
        const int cx = j / NV, k = j - cx * NV, a = k / ce, e = k - a * ce;
        const int c = c_base + cx * ce + e;
        if (c < C) {
            float acc = 0.f;
            for (int r = 0; r < nw; ++r) acc += sred[r * width + j];
            if (slot) slot[a * C + c] = acc;
            else atomicAdd((a == 0 ? dst0 : dst1) + c, acc);
        }
    }
}

// column statistics: stats[c] += sum_m x[m,c]; stats[C+c] += sum_m x[m,c]^2
template <typename T>
__global__ __launch_bounds__(NT) void colstats_kernel(const T* __restrict__ x, int M, int C, int ld, float* __restrict__ stats,
                                                      int rows_per_block, int nrep, int only_sum, int tx, int ty, const int32_t* __restrict__ m_dev,
                                                      float* __restrict__ slots) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float sred[];
    if (m_dev) { M = dev_rows(m_dev, M); rows_per_block = (M + (int)gridDim.x - 1) / (int)gridDim.x; }
    const int ix = threadIdx.x % tx, iy = threadIdx.x / tx;
    const int cc = blockIdx.y * tx + ix;
    const bool active = iy < ty && cc * CE < C;
    float part[2 * CE];
#pragma unroll
    for (int k = 0; k < 2 * CE; ++k) part[k] = 0.f;
    const int mbeg = blockIdx.x * rows_per_block, mend = min(M, mbeg + rows_per_block);
    if (active) {
        const T* xp = x + cc * CE;
        int m = mbeg + iy;
        for (; m + ty < mend; m += 2 * ty) {                 // two independent loads in flight
            float f0[CE], f1[CE];
            TR::unpack(*(const uint4*)(xp + (long)m * ld), f0);
            TR::unpack(*(const uint4*)(xp + (long)(m + ty) * ld), f1);
#pragma unroll
            for (int e = 0; e < CE; ++e) { part[e] += f0[e] + f1[e]; part[CE + e] += f0[e] * f0[e] + f1[e] * f1[e]; }
        }
        if (m < mend) {
            float f0[CE];
            TR::unpack(*(const uint4*)(xp + (long)m * ld), f0);
#pragma unroll
            for (int e = 0; e < CE; ++e) { part[e] += f0[e]; part[CE + e] += f0[e] * f0[e]; }
        }
    }
    // nrep >= gridDim.x (deterministic mode: MG_DET_STAT_ROWS rows): every row block adds to its OWN row -- one addition per word, no order
    float* st = stats + (size_t)(blockIdx.x & (nrep - 1)) * 2 * C;
    if (only_sum) col_block_reduce<CE>(sred, part, tx, ty, ix, iy, active, st, st, blockIdx.y * tx * CE, C, CE, slots ? slots + (size_t)blockIdx.x * C : nullptr);
    else col_block_reduce<2 * CE>(sred, part, tx, ty, ix, iy, active, st, st + C, blockIdx.y * tx * CE, C, CE, slots ? slots + (size_t)blockIdx.x * 2 * C : nullptr);
}

// backward of "+ bias, ReLU" epilogues (sparse convs / linears without a BatchNorm behind them): g = dy * (y > 0) and
// db[c] = sum_m g[m,c] in one pass (the torch formulation was compare + cast + multiply + cast + sum: 5 launches)
template <typename T>
__global__ __launch_bounds__(NT) void bias_act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ g, int M, int C,
                                                          float* __restrict__ db, int rows_per_block, int tx, int ty, const int32_t* __restrict__ m_dev,
                                                          float* __restrict__ slots) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float sred[];
    if (m_dev) { M = dev_rows(m_dev, M); rows_per_block = (M + (int)gridDim.x - 1) / (int)gridDim.x; }
    const int ix = threadIdx.x % tx, iy = threadIdx.x / tx;
    const int cc = blockIdx.y * tx + ix;
    const bool active = iy < ty && cc * CE < C;
    float part[CE];
#pragma unroll
    for (int k = 0; k < CE; ++k) part[k] = 0.f;
    const int mbeg = blockIdx.x * rows_per_block, mend = min(M, mbeg + rows_per_block);
    if (active) {
        for (int m = mbeg + iy; m < mend; m += ty) {
            const long off = (long)m * C + cc * CE;
            float f[CE];
            TR::unpack(*(const uint4*)(dy + off), f);
            if (y) {
                float yv[CE];
                TR::unpack(*(const uint4*)(y + off), yv);
#pragma unroll
                for (int e = 0; e < CE; ++e) f[e] = yv[e] > 0.f ? f[e] : 0.f;
                *(uint4*)(g + off) = TR::pack(f);
            }
#pragma unroll
            for (int e = 0; e < CE; ++e) part[e] += f[e];
        }
    }
    if (db) col_block_reduce<CE>(sred, part, tx, ty, ix, iy, active, db, db, blockIdx.y * tx * CE, C, CE, slots ? slots + (size_t)blockIdx.x * C : nullptr);
}

// second pass of the exact two-pass variance: stats[C+c] += sum_m (x[m,c] - stats[c]/M)^2   (stats[0:C] = column sums)
template <typename T>
__global__ __launch_bounds__(NT) void colstats_centered_kernel(const T* __restrict__ x, int M, int C, int ld, float* __restrict__ stats,
                                                               int rows_per_block, int tx, int ty, const int32_t* __restrict__ m_dev,
                                                               float* __restrict__ slots) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float sred[];
    if (m_dev) { M = dev_rows(m_dev, M); rows_per_block = (M + (int)gridDim.x - 1) / (int)gridDim.x; }
    const int ix = threadIdx.x % tx, iy = threadIdx.x / tx;
    const int cc = blockIdx.y * tx + ix;
    const bool active = iy < ty && cc * CE < C;
    float part[CE], mu[CE];
    const float inv_m = M > 0 ? 1.f / (float)M : 0.f;
#pragma unroll
    for (int e = 0; e < CE; ++e) { part[e] = 0.f; mu[e] = active ? stats[cc * CE + e] * inv_m : 0.f; }
    const int mbeg = blockIdx.x * rows_per_block, mend = min(M, mbeg + rows_per_block);
    if (active) {
        const T* xp = x + cc * CE;
        int m = mbeg + iy;
        for (; m + ty < mend; m += 2 * ty) {
            float f0[CE], f1[CE];
            TR::unpack(*(const uint4*)(xp + (long)m * ld), f0);
            TR::unpack(*(const uint4*)(xp + (long)(m + ty) * ld), f1);
#pragma unroll
            for (int e = 0; e < CE; ++e) { float d0 = f0[e] - mu[e], d1 = f1[e] - mu[e]; part[e] += d0 * d0 + d1 * d1; }
        }
        if (m < mend) {
            float f0[CE];
            TR::unpack(*(const uint4*)(xp + (long)m * ld), f0);
#pragma unroll
            for (int e = 0; e < CE; ++e) { float d0 = f0[e] - mu[e]; part[e] += d0 * d0; }
        }
    }
    col_block_reduce<CE>(sred, part, tx, ty, ix, iy, active, stats + C, stats + C, blockIdx.y * tx * CE, C, CE, slots ? slots + (size_t)blockIdx.x * C : nullptr);
}

// ---------------------------------------------------------------------------------------------------
// finalize: batch statistics -> (scale, shift, mean, invstd) + running-stat update (momentum, unbiased var)
// ---------------------------------------------------------------------------------------------------
__global__ void bn_finalize_kernel(const float* __restrict__ stats, int nrep, const float* __restrict__ count_ptr, float count, int C, int centered,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float* running_mean,
                                   float* running_var, float momentum, float eps, float* __restrict__ scale,
                                   float* __restrict__ shift, float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                   const int32_t* __restrict__ m_dev, float nmult) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float n = count_ptr ? *count_ptr : count;
    if (m_dev) n = (float)dev_rows(m_dev, (int)count);
    if ((m_dev || count_ptr) && n <= 0.f) {               // no active row at all (on any rank, for SyncBN): identity statistics, running stats untouched
        scale[c] = gamma ? gamma[c] : 1.f; shift[c] = beta ? beta[c] : 0.f; mean_out[c] = 0.f; invstd_out[c] = 1.f;
        return;
    }
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < nrep; ++r) { s1 += stats[(size_t)r * 2 * C + c]; s2 += stats[(size_t)r * 2 * C + C + c]; }
    float mean = s1 / n;
    float var = centered ? s2 / n : s2 / n - mean * mean;
    var = var > 0.f ? var : 0.f;
    float invstd = rsqrtf(var + eps);
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    scale[c] = g * invstd;
    shift[c] = b - mean * g * invstd;
    mean_out[c] = mean;
    invstd_out[c] = invstd;
    if (running_mean) {
        const float nu = n * nmult;                           // samples the reference's BatchNorm saw (rows x count_mult)
        float unbiased = nu > 1.f ? var * nu / (nu - 1.f) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
}

// The same for MANY rows (deterministic mode: one row per row block / per output tile of the producing conv, up to tens of thousands): one
// workgroup per channel, thread t adds rows t, t + 256, ... in that order, the 256 partial sums meet in a fixed tree. The result depends on
// (nrep) only -- never on which workgroup of the producer finished first.
__global__ __launch_bounds__(NT) void bn_finalize_rows_kernel(const float* __restrict__ stats, int nrep, const float* __restrict__ count_ptr, float count, int C,
                                                             int centered, const float* __restrict__ gamma, const float* __restrict__ beta, float* running_mean,
                                                             float* running_var, float momentum, float eps, float* __restrict__ scale,
                                                             float* __restrict__ shift, float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                             const int32_t* __restrict__ m_dev, float nmult) {
    __shared__ float sh[2][NT];
    const int c = blockIdx.x, t = threadIdx.x;
    float n = count_ptr ? *count_ptr : count;
    if (m_dev) n = (float)dev_rows(m_dev, (int)count);
    if ((m_dev || count_ptr) && n <= 0.f) {
        if (t == 0) { scale[c] = gamma ? gamma[c] : 1.f; shift[c] = beta ? beta[c] : 0.f; mean_out[c] = 0.f; invstd_out[c] = 1.f; }
        return;
    }
    float a1 = 0.f, a2 = 0.f;
    int r = t;
    for (; r + 3 * NT < nrep; r += 4 * NT) {                  // four independent loads per column in flight, added in row order
        const float x0 = stats[(size_t)r * 2 * C + c], x1 = stats[(size_t)(r + NT) * 2 * C + c];
        const float x2 = stats[(size_t)(r + 2 * NT) * 2 * C + c], x3 = stats[(size_t)(r + 3 * NT) * 2 * C + c];
        const float y0 = stats[(size_t)r * 2 * C + C + c], y1 = stats[(size_t)(r + NT) * 2 * C + C + c];
        const float y2 = stats[(size_t)(r + 2 * NT) * 2 * C + C + c], y3 = stats[(size_t)(r + 3 * NT) * 2 * C + C + c];
        a1 += x0; a1 += x1; a1 += x2; a1 += x3;
        a2 += y0; a2 += y1; a2 += y2; a2 += y3;
    }
    for (; r < nrep; r += NT) { a1 += stats[(size_t)r * 2 * C + c]; a2 += stats[(size_t)r * 2 * C + C + c]; }
    sh[0][t] = a1; sh[1][t] = a2;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) { sh[0][t] += sh[0][t + o]; sh[1][t] += sh[1][t + o]; }
        __syncthreads();
    }
    if (t != 0) return;
    const float s1 = sh[0][0], s2 = sh[1][0];
    float mean = s1 / n;
    float var = centered ? s2 / n : s2 / n - mean * mean;
    var = var > 0.f ? var : 0.f;
    float invstd = rsqrtf(var + eps);
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    scale[c] = g * invstd;
    shift[c] = b - mean * g * invstd;
    mean_out[c] = mean;
    invstd_out[c] = invstd;
    if (running_mean) {
        const float nu = n * nmult;                           // samples the reference's BatchNorm saw (rows x count_mult)
        float unbiased = nu > 1.f ? var * nu / (nu - 1.f) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
}

__global__ void bn_fold_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ running_mean, const float* __restrict__ running_var, float eps,
                               float* __restrict__ scale, float* __restrict__ shift) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float invstd = rsqrtf(running_var[c] + eps);
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    scale[c] = g * invstd;
    shift[c] = b - running_mean[c] * g * invstd;
}

// ---------------------------------------------------------------------------------------------------
// y = act(x*scale + shift + res) + res2      (res optionally at half resolution, nearest x2)
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void affine_act_kernel(const mg_rowwise_params p) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    const int cpr = p.C / CE;
    const long total = (long)dev_rows(p.m_dev, p.M) * cpr;
    const T* __restrict__ x = (const T*)p.x;
    const T* __restrict__ r1 = (const T*)p.res;
    const T* __restrict__ r2 = (const T*)p.res2;
    T* __restrict__ y = (T*)p.y;
    // When the chunks-per-row count divides the block size (every power-of-two channel count), a thread keeps ONE channel chunk for
    // its whole grid-stride walk: scale / shift live in registers and the row index advances by a constant, instead of 2*CE scalar
    // parameter loads and a 64-bit division per 16-byte chunk (the 262144 x 64 layer ran at 1.9 TB/s on those).
    const bool fixed = (NT % cpr) == 0;
    float scf[CE], shf[CE];
    int m_fix = 0, cc_fix = 0, m_step = 0;
    if (fixed) {
        const long i0 = (long)blockIdx.x * NT + threadIdx.x;
        m_fix = (int)(i0 / cpr); cc_fix = (int)(i0 - (long)m_fix * cpr);
        m_step = (int)(((long)gridDim.x * NT) / cpr);
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            scf[e] = p.scale ? p.scale[cc_fix * CE + e] : 1.f;
            shf[e] = p.shift ? p.shift[cc_fix * CE + e] : 0.f;
        }
    }
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        int m, cc;
        if (fixed) { m = m_fix; cc = cc_fix; m_fix += m_step; }
        else { m = (int)(i / cpr); cc = (int)(i - (long)m * cpr); }
        int c0 = cc * CE;
        float f[CE], a[CE], b[CE];
        TR::unpack(*(const uint4*)(x + (long)m * p.ldx + c0), f);
#pragma unroll
        for (int e = 0; e < CE; ++e) { a[e] = 0.f; b[e] = 0.f; }
        if (r1) {
            long rrow = m;
            if (p.res_mode == 2) {
                int hw = p.H * p.W; int n = m / hw; int rem = m - n * hw; int ho = rem / p.W; int wo = rem - ho * p.W;
                rrow = ((long)n * (p.H >> 1) + (ho >> 1)) * (p.W >> 1) + (wo >> 1);
            }
            TR::unpack(*(const uint4*)(r1 + rrow * p.ldr + c0), a);
        }
        if (r2) TR::unpack(*(const uint4*)(r2 + (long)m * p.ldr2 + c0), b);
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            float v = f[e];
            float sc, sh;
            if (fixed) { sc = scf[e]; sh = shf[e]; }
            else { sc = p.scale ? p.scale[c0 + e] : 1.f; sh = p.shift ? p.shift[c0 + e] : 0.f; }
            v = v * sc + sh + a[e];
            v = apply_act(v, p.act, p.slope) + b[e];
            f[e] = v;
        }
        *(uint4*)(y + (long)m * p.ldy + p.yoff + c0) = TR::pack(f);
    }
}

// ---------------------------------------------------------------------------------------------------
// Training BatchNorm, last forward pass: finalize + apply in ONE launch (round 3). Every workgroup re-derives scale / shift for
// its own channels from the accumulated statistics (the replicas are summed through LDS by the first 2C threads -- at most 32
// independent L2 loads per thread, then 2 * CE LDS reads per thread), workgroup 0 also writes scale | shift | mean | invstd for the backward
// and updates the running statistics. Same arithmetic, in the same order, as bn_finalize_kernel + affine_act_kernel; what goes
// away is a 6 us launch at the latency floor per BatchNorm layer (59 per step) and its dependent boundary.
// Requires a fixed thread -> channel-chunk mapping (NT % (C / CE) == 0: every power-of-two channel count).
// ---------------------------------------------------------------------------------------------------
// Sum of `nrep` replicas of a [2C] fp32 statistics row for THIS thread's CE channels: s1[e] = sum_r st[r][c0 + e], s2[e] = sum_r st[r][C + c0 + e].
// nrep == 1 (exact two-pass layers, the sparse head): two 16-byte loads per 4 channels straight into registers, no barrier. nrep > 1 (the
// 32 replicas a conv epilogue spreads its atomics over): the WORKGROUP reads the nrep x 2C words once, every thread a few INDEPENDENT loads
// (thread -> (replica group, column); a serial `a += st[r]` loop was 32 dependent L2 round trips, and every thread reading all replicas of
// its own channels moved 2 GB through L2 per launch), partial sums meet in LDS. `lds`: 256 floats + 2C floats.
template <int CE>
__device__ __forceinline__ void replica_sums(const float* __restrict__ st, int nrep, int C, int c0, float* s1, float* s2, float* lds) {
    if (nrep == 1) {
#pragma unroll
        for (int q = 0; q < CE / 4; ++q) {
            const float4 a = *(const float4*)(st + c0 + q * 4);
            const float4 b = *(const float4*)(st + C + c0 + q * 4);
            s1[q * 4 + 0] = a.x; s1[q * 4 + 1] = a.y; s1[q * 4 + 2] = a.z; s1[q * 4 + 3] = a.w;
            s2[q * 4 + 0] = b.x; s2[q * 4 + 1] = b.y; s2[q * 4 + 2] = b.z; s2[q * 4 + 3] = b.w;
        }
        return;
    }
    // columns 2C <= 256 (every layer that accumulates replicas has C <= 128): thread t -> column t % W2, replica group t / W2
    const int W2 = 2 * C;
    float* part = lds;                // [NT]
    float* tot = lds + NT;            // [2C]
    if (W2 <= NT) {
        const int groups = NT / W2;                           // replica groups in flight (power of two: C is)
        const int col = threadIdx.x % W2, grp = threadIdx.x / W2;
        float a = 0.f;
        if (grp < groups) {
            float v[8];
            int r = grp;
            for (; r + 7 * groups < nrep; r += 8 * groups) {
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = st[(size_t)(r + u * groups) * W2 + col];
#pragma unroll
                for (int u = 0; u < 8; ++u) a += v[u];
            }
            for (; r < nrep; r += groups) a += st[(size_t)r * W2 + col];
        }
        part[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x < W2) {
            float t = 0.f;
            for (int g = 0; g < groups; ++g) t += part[g * W2 + threadIdx.x];
            tot[threadIdx.x] = t;
        }
        __syncthreads();
    } else {
        for (int j = threadIdx.x; j < W2; j += NT) {
            float t = 0.f;
            for (int r = 0; r < nrep; ++r) t += st[(size_t)r * W2 + j];
            tot[j] = t;
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < CE; ++e) { s1[e] = tot[c0 + e]; s2[e] = tot[C + c0 + e]; }
}

struct BnFin {
    const float* stats; int nrep; int centered;
    const float* gamma; const float* beta; float* running_mean; float* running_var;
    float momentum, eps; float* outs;
};

template <typename T>
__global__ __launch_bounds__(NT) void bn_apply_fused_kernel(const mg_rowwise_params p, const BnFin f) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float slds[];                           // [NT + 2C] (replica_sums)
    const int C = p.C, cpr = C / CE;
    const int Mrows = dev_rows(p.m_dev, p.M);
    const long i0 = (long)blockIdx.x * NT + threadIdx.x;
    int m = (int)(i0 / cpr);
    const int cc = (int)(i0 - (long)m * cpr), c0 = cc * CE;
    const int m_step = (int)(((long)gridDim.x * NT) / cpr);
    const T* __restrict__ x = (const T*)p.x;
    const T* __restrict__ r1 = (const T*)p.res;
    const T* __restrict__ r2 = (const T*)p.res2;
    T* __restrict__ y = (T*)p.y;
    auto res_row = [&](int mm) -> long {
        if (p.res_mode != 2) return mm;
        const int hw = p.H * p.W; const int nn = mm / hw; const int rem = mm - nn * hw; const int ho = rem / p.W; const int wo = rem - ho * p.W;
        return ((long)nn * (p.H >> 1) + (ho >> 1)) * (p.W >> 1) + (wo >> 1);
    };
    // the first row's operands are requested BEFORE the statistics are touched: most launches give a thread one or two rows, so the
    // statistics round trip (L2 miss on words just written by atomics) and the tensor round trip overlap instead of adding up
    uint4 qx = make_uint4(0, 0, 0, 0), qa = qx, qb = qx;
    if (m < Mrows) {
        qx = *(const uint4*)(x + (long)m * p.ldx + c0);
        if (r1) qa = *(const uint4*)(r1 + res_row(m) * p.ldr + c0);
        if (r2) qb = *(const uint4*)(r2 + (long)m * p.ldr2 + c0);
    }
    const float n = p.count_ptr ? *p.count_ptr : (p.m_dev ? (float)Mrows : p.count);
    float gam[CE], bet[CE], t1[CE], t2[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { gam[e] = f.gamma ? f.gamma[c0 + e] : 1.f; bet[e] = f.beta ? f.beta[c0 + e] : 0.f; }
    replica_sums<CE>(f.stats, f.nrep, C, c0, t1, t2, slds);
    const bool ident = (p.m_dev || p.count_ptr) && n <= 0.f;  // no live row anywhere: identity statistics, running stats untouched
    const bool writer = blockIdx.x == 0 && threadIdx.x < cpr;
    float sc[CE], sh[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int c = c0 + e;
        const float g = gam[e], b = bet[e];
        float mean = 0.f, invstd = 1.f, var = 0.f;
        if (!ident) {
            const float s1 = t1[e], s2 = t2[e];
            mean = s1 / n;
            var = f.centered ? s2 / n : s2 / n - mean * mean;
            var = var > 0.f ? var : 0.f;
            invstd = rsqrtf(var + f.eps);
        }
        sc[e] = ident ? g : g * invstd;
        sh[e] = ident ? b : b - mean * g * invstd;
        if (writer) {
            f.outs[c] = sc[e]; f.outs[C + c] = sh[e]; f.outs[2 * C + c] = mean; f.outs[3 * C + c] = invstd;
            if (f.running_mean && !ident) {
                const float unbiased = n > 1.f ? var * n / (n - 1.f) : var;
                f.running_mean[c] = (1.f - f.momentum) * f.running_mean[c] + f.momentum * mean;
                f.running_var[c] = (1.f - f.momentum) * f.running_var[c] + f.momentum * unbiased;
            }
        }
    }
    while (m < Mrows) {
        const int mn = m + m_step;
        uint4 nx = make_uint4(0, 0, 0, 0), na = nx, nb = nx;
        if (mn < Mrows) {                                      // next row in flight under this row's arithmetic and store
            nx = *(const uint4*)(x + (long)mn * p.ldx + c0);
            if (r1) na = *(const uint4*)(r1 + res_row(mn) * p.ldr + c0);
            if (r2) nb = *(const uint4*)(r2 + (long)mn * p.ldr2 + c0);
        }
        float v[CE], a[CE], b[CE];
        TR::unpack(qx, v);
#pragma unroll
        for (int e = 0; e < CE; ++e) { a[e] = 0.f; b[e] = 0.f; }
        if (r1) TR::unpack(qa, a);
        if (r2) TR::unpack(qb, b);
#pragma unroll
        for (int e = 0; e < CE; ++e) v[e] = apply_act(v[e] * sc[e] + sh[e] + a[e], p.act, p.slope) + b[e];
        *(uint4*)(y + (long)m * p.ldy + p.yoff + c0) = TR::pack(v);
        m = mn; qx = nx; qa = na; qb = nb;
    }
}

// ---------------------------------------------------------------------------------------------------
// BN backward, pass 1: sums[c] += sum_m g, sums[C+c] += sum_m g*xhat,  g = dy * act'(y) (y = post-activation output)
// BN backward, pass 2: dx = scale_c * (g - sum_g/n - xhat * sum_gx/n)   [ * (x > 0) for the ReLU-before-BN shortcut ]
//                      dres = g (optional, gradient of the pre-activation residual)
// ---------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load_g(const mg_rowwise_params& p, int m, int c0, float* g) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    TR::unpack(*(const uint4*)((const T*)p.dy + (long)m * p.lddy + c0), g);
    if (p.act != MG_ACT_NONE && p.mask_from_x) {
        // the activation output was never stored (round 5: the consumer convolution applies BatchNorm + activation to its operand in flight,
        // mg_conv_params.xf_*): its sign is that of x * scale + shift, re-formed from the raw input with the arithmetic of xf_apply8
        float xv[CE];
        TR::unpack(*(const uint4*)((const T*)p.x + (long)m * p.ldx + c0), xv);
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            const float z = xv[e] * p.scale[c0 + e] + p.shift[c0 + e];
            if (!(z > 0.f)) g[e] = (p.act == MG_ACT_RELU) ? 0.f : g[e] * p.slope;
        }
    } else if (p.act != MG_ACT_NONE) {
        float yv[CE];
        TR::unpack(*(const uint4*)((const T*)p.y + (long)m * p.ldy + p.yoff + c0), yv);
        if (p.res2) {                      // y = act(.) + res2  -> recover the activation output sign
            float b[CE];
            TR::unpack(*(const uint4*)((const T*)p.res2 + (long)m * p.ldr2 + c0), b);
#pragma unroll
            for (int e = 0; e < CE; ++e) yv[e] -= b[e];
        }
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            if (!(yv[e] > 0.f)) g[e] = (p.act == MG_ACT_RELU) ? 0.f : g[e] * p.slope;
        }
    }
}

template <typename T, int BT = NT>
__global__ __launch_bounds__(BT) void bn_bwd_reduce_kernel(const mg_rowwise_params p, int rows_per_block, int tx, int ty, float* __restrict__ slots, unsigned* __restrict__ tail_cnt) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float sred[];
    const int C = p.C;
    const int M = dev_rows(p.m_dev, p.M);
    if (p.m_dev) rows_per_block = (M + (int)gridDim.x - 1) / (int)gridDim.x;
    const int ix = threadIdx.x % tx, iy = threadIdx.x / tx;
    const int cc = blockIdx.y * tx + ix;
    const bool active = iy < ty && cc * CE < C;
    const int c0 = cc * CE;
    float part[2 * CE], mu[CE], is[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        part[e] = 0.f; part[CE + e] = 0.f;
        mu[e] = active ? p.mean[c0 + e] : 0.f; is[e] = active ? p.invstd[c0 + e] : 0.f;
    }
    const int mbeg = blockIdx.x * rows_per_block, mend = min(M, mbeg + rows_per_block);
    if (active) {
        int m = mbeg + iy;
        for (; m + ty < mend; m += 2 * ty) {                 // two independent row groups in flight
            float g0[CE], g1[CE], x0[CE], x1[CE];
            load_g<T>(p, m, c0, g0);
            load_g<T>(p, m + ty, c0, g1);
            TR::unpack(*(const uint4*)((const T*)p.x + (long)m * p.ldx + c0), x0);
            TR::unpack(*(const uint4*)((const T*)p.x + (long)(m + ty) * p.ldx + c0), x1);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                part[e] += g0[e] + g1[e];
                part[CE + e] += (g0[e] * (x0[e] - mu[e]) + g1[e] * (x1[e] - mu[e])) * is[e];
            }
        }
        if (m < mend) {
            float g0[CE], x0[CE];
            load_g<T>(p, m, c0, g0);
            TR::unpack(*(const uint4*)((const T*)p.x + (long)m * p.ldx + c0), x0);
#pragma unroll
            for (int e = 0; e < CE; ++e) { part[e] += g0[e]; part[CE + e] += g0[e] * (x0[e] - mu[e]) * is[e]; }
        }
    }
    float* slot = slots ? slots + (size_t)blockIdx.x * 2 * C : nullptr;
    if (BT > NT) col_block_reduce_wave<2 * CE>(sred, part, tx, ix, active, p.sums, p.sums + C, blockIdx.y * tx * CE, C, CE, slot);
    else col_block_reduce<2 * CE>(sred, part, tx, ty, ix, iy, active, p.sums, p.sums + C, blockIdx.y * tx * CE, C, CE, slot);
    if (!tail_cnt) return;
    // ---- ordered sum of the partial rows by the LAST row block of this channel group to arrive (round 6; the separate mg_det_reduce launch of this
    // layer disappears). No workgroup waits for another one: every block publishes its row (release), takes a ticket, and the one that draws the last
    // ticket adds all rows of its group IN ROW ORDER -- chunk by chunk with det_reduce_kernel's own arithmetic (det_chunk_sum), so the sums have the bits
    // the separate launch gave them, whichever block happens to be last. The ticket word returns to 0 for the next launch on the stream.
    __shared__ int s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(tail_cnt + blockIdx.y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev + 1u == gridDim.x;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int nblk = (int)gridDim.x, gw = tx * CE, ncol = 2 * gw, c_base = blockIdx.y * gw;      // columns of this group: [a][gw], a = 0: sum g, 1: sum g xhat
    const int cs = (nblk + MG_DET_CHUNKS - 1) / MG_DET_CHUNKS;
    float* sh = sred;                                          // [MG_DET_CHUNKS][ncol] <= 8 KB: inside both reduction layouts above (all reads of them are done)
    for (int j = threadIdx.x; j < MG_DET_CHUNKS * ncol; j += BT) {
        const int k = j / ncol, col = j - k * ncol, a = col / gw, c = c_base + col - a * gw;
        const int b0 = k * cs, b1 = min(nblk, b0 + cs);
        sh[j] = (c < C && b0 < b1) ? det_chunk_sum(slots + (size_t)b0 * 2 * C + a * C + c, b1 - b0, 2 * C) : 0.f;
    }
    __syncthreads();
    for (int col = threadIdx.x; col < ncol; col += BT) {
        const int a = col / gw, c = c_base + col - a * gw;
        if (c < C) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < MG_DET_CHUNKS; ++i) t += sh[i * ncol + col];
            p.sums[a * C + c] += t;
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(tail_cnt + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(const mg_rowwise_params p) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    const int cpr = p.C / CE;
    const int Mrows = dev_rows(p.m_dev, p.M);
    const long total = (long)Mrows * cpr;
    // sample count: the SyncBN global count when given, else the live rows of this rank (device word), else the host value
    const float inv_n = p.count_ptr ? (*p.count_ptr > 0.f ? 1.f / *p.count_ptr : 0.f) : (p.m_dev ? (Mrows > 0 ? 1.f / (float)Mrows : 0.f) : 1.f / p.count);
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        int m = (int)(i / cpr), cc = (int)(i - (long)m * cpr);
        int c0 = cc * CE;
        float g[CE], xv[CE], o[CE];
        load_g<T>(p, m, c0, g);
        if (p.dres) *(uint4*)((T*)p.dres + (long)m * p.lddres + c0) = TR::pack(g);
        if (p.dx) {
            TR::unpack(*(const uint4*)((const T*)p.x + (long)m * p.ldx + c0), xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                int c = c0 + e;
                float xh = (xv[e] - p.mean[c]) * p.invstd[c];
                float v = p.scale[c] * (g[e] - p.sums[c] * inv_n - xh * p.sums[p.C + c] * inv_n);
                if (p.mask_x_pos && !(xv[e] > 0.f)) v = 0.f;
                o[e] = v;
            }
            *(uint4*)((T*)p.dx + (long)m * p.lddx + c0) = TR::pack(o);
        }
    }
}

// dgamma[c] = sums[C+c], dbeta[c] = sums[c] are read directly by the host side (fp32 tensors).

// Pass 2 with a fixed thread -> channel-chunk mapping (round 3; NT % (C / CE) == 0): the per-channel constants (mean, invstd, scale, the two
// sums) live in registers for the whole grid-stride walk instead of five parameter loads and a 64-bit division per 16-byte chunk. The
// sums may arrive as `nrep` replicas of [2C] (accumulated by the consumer conv's data-gradient epilogue, mg_conv_params.bnb_*): they are
// reduced through LDS here, workgroup 0 writes the totals to `sums_out` (= dbeta | dgamma). `premasked`: p.dy already holds
// g = dy * act'(y) (written by that epilogue), so y is not read again.
template <typename T>
__global__ __launch_bounds__(NT) void bn_bwd_apply_fixed_kernel(const mg_rowwise_params p, const float* __restrict__ sums_rep, int nrep, int premasked,
                                                                float* __restrict__ sums_out) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    extern __shared__ float slds[];                           // [NT + 2C] (replica_sums)
    const int C = p.C, cpr = C / CE;
    const int Mrows = dev_rows(p.m_dev, p.M);
    const long i0 = (long)blockIdx.x * NT + threadIdx.x;
    int m = (int)(i0 / cpr);
    const int cc = (int)(i0 - (long)m * cpr), c0 = cc * CE;
    const int m_step = (int)(((long)gridDim.x * NT) / cpr);
    // first row's operands in flight before the sums are touched (see bn_apply_fused_kernel)
    float g[CE];
    uint4 qx = make_uint4(0, 0, 0, 0);
    if (m < Mrows) {
        if (premasked) TR::unpack(*(const uint4*)((const T*)p.dy + (long)m * p.lddy + c0), g);
        else load_g<T>(p, m, c0, g);
        qx = *(const uint4*)((const T*)p.x + (long)m * p.ldx + c0);
    }
    float mu[CE], is[CE], sc[CE], sg[CE], sgx[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { mu[e] = p.mean[c0 + e]; is[e] = p.invstd[c0 + e]; sc[e] = p.scale[c0 + e]; }
    replica_sums<CE>(sums_rep, nrep, C, c0, sg, sgx, slds);
    if (sums_out && blockIdx.x == 0 && threadIdx.x < cpr) {
#pragma unroll
        for (int e = 0; e < CE; ++e) { sums_out[c0 + e] = sg[e]; sums_out[C + c0 + e] = sgx[e]; }
    }
    const float inv_n = p.count_ptr ? (*p.count_ptr > 0.f ? 1.f / *p.count_ptr : 0.f) : (p.m_dev ? (Mrows > 0 ? 1.f / (float)Mrows : 0.f) : 1.f / p.count);
#pragma unroll
    for (int e = 0; e < CE; ++e) { sg[e] *= inv_n; sgx[e] *= inv_n; }
    while (m < Mrows) {
        const int mn = m + m_step;
        float gn[CE];
        uint4 nx = make_uint4(0, 0, 0, 0);
        if (mn < Mrows) {
            if (premasked) TR::unpack(*(const uint4*)((const T*)p.dy + (long)mn * p.lddy + c0), gn);
            else load_g<T>(p, mn, c0, gn);
            nx = *(const uint4*)((const T*)p.x + (long)mn * p.ldx + c0);
        }
        if (p.dres) *(uint4*)((T*)p.dres + (long)m * p.lddres + c0) = TR::pack(g);
        if (p.dx) {
            float xv[CE], o[CE];
            TR::unpack(qx, xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                const float xh = (xv[e] - mu[e]) * is[e];
                float v = sc[e] * (g[e] - sg[e] - xh * sgx[e]);
                if (p.mask_x_pos && !(xv[e] > 0.f)) v = 0.f;
                o[e] = v;
            }
            *(uint4*)((T*)p.dx + (long)m * p.lddx + c0) = TR::pack(o);
        }
        m = mn; qx = nx;
#pragma unroll
        for (int e = 0; e < CE; ++e) g[e] = gn[e];
    }
}

// ---------------------------------------------------------------------------------------------------
// 2x2 average pool (AvgPool2d(2,2), encoder/resnet.py:113), its backward, 2x2 sum (nearest-upsample backward)
// ---------------------------------------------------------------------------------------------------
template <typename T, int OP>   // OP 0: out[n,ho,wo] = mean of 2x2 of in; 1: out = sum of 2x2 of in; 2: out[n,h,w] = 0.25*in[n,h/2,w/2]; 3: out = in[n,h/2,w/2]
__global__ __launch_bounds__(NT) void pool2x2_kernel(const T* __restrict__ in, T* __restrict__ out, int N, int Ho, int Wo, int C,
                                                     int Hi, int Wi) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    const int cpr = C / CE;
    const long total = (long)N * Ho * Wo * cpr;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        int cc = (int)(i % cpr); long r = i / cpr;
        int wo = (int)(r % Wo); r /= Wo; int ho = (int)(r % Ho); int n = (int)(r / Ho);
        float o[CE];
        if (OP <= 1) {
#pragma unroll
            for (int e = 0; e < CE; ++e) o[e] = 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    float f[CE];
                    TR::unpack(*(const uint4*)(in + (((long)n * Hi + 2 * ho + dy) * Wi + 2 * wo + dx) * C + cc * CE), f);
#pragma unroll
                    for (int e = 0; e < CE; ++e) o[e] += f[e];
                }
            if (OP == 0) {
#pragma unroll
                for (int e = 0; e < CE; ++e) o[e] *= 0.25f;
            }
        } else {
            TR::unpack(*(const uint4*)(in + (((long)n * Hi + (ho >> 1)) * Wi + (wo >> 1)) * C + cc * CE), o);
            if (OP == 2) {
#pragma unroll
                for (int e = 0; e < CE; ++e) o[e] *= 0.25f;
            }
        }
        *(uint4*)(out + (((long)n * Ho + ho) * Wo + wo) * C + cc * CE) = TR::pack(o);
    }
}

inline int grid_for(long total) {
    long b = (total + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int mg_colstats_dev(const void* x, int dtype, int M, int C, int ld, float* stats, const int32_t* m_dev, void* stream) {
    if (M <= 0) return 0;
    const int ce = MG_IS16(dtype) ? 8 : 4;
    if (C % ce || ld % ce) return -3;
    const ColGeom g = col_geom(M, C, ce, 1024);
    const size_t lds = (size_t)g.ty * g.tx * 2 * ce * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    // deterministic mode: MG_DET_STAT_ROWS (1024 >= the row-block count) rows, i.e. one row per row block -- a word receives ONE addition, the
    // finalize kernel adds the rows in index order
    const int nrep = mg_det_on ? MG_DET_STAT_ROWS : MG_STAT_REPLICAS;
    MG_WITH_DTYPE(dtype, T, hipLaunchKernelGGL(colstats_kernel<T>, dim3(g.rb, g.groups), dim3(NT), lds, st, (const T*)x, M, C, ld, stats, g.rpb, nrep, 0, g.tx, g.ty, m_dev, nullptr););
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_colstats(const void* x, int dtype, int M, int C, int ld, float* stats, void* stream) {
    return mg_colstats_dev(x, dtype, M, C, ld, stats, nullptr, stream);
}

extern "C" int mg_bias_act_bwd_dev(const void* dy, const void* y, void* g, int dtype, int M, int C, float* db, const int32_t* m_dev, void* stream);
extern "C" int mg_bias_act_bwd(const void* dy, const void* y, void* g, int dtype, int M, int C, float* db, void* stream) {
    return mg_bias_act_bwd_dev(dy, y, g, dtype, M, C, db, nullptr, stream);
}
extern "C" int mg_bias_act_bwd_dev(const void* dy, const void* y, void* g, int dtype, int M, int C, float* db, const int32_t* m_dev, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (db) { hipError_t e = mg_zero_words(db, C, st); if (e != hipSuccess) return (int)e; }
    if (M <= 0) return 0;
    const int ce = MG_IS16(dtype) ? 8 : 4;
    if (C % ce) return -3;
    if (y && !g) return -3;
    const ColGeom gm = col_geom(M, C, ce, 512);          // like MG_BN_RB: enough blocks to stream at HBM rate, few enough atomics per channel
    const size_t lds = (size_t)gm.ty * gm.tx * ce * sizeof(float);
    float* slots = nullptr;
    if (db && mg_det_on && gm.rb > 1) { slots = mg_det_scratch_on((long)gm.rb * C, st); if (!slots) return MG_DET_NO_SCRATCH; }
    MG_WITH_DTYPE(dtype, T, hipLaunchKernelGGL(bias_act_bwd_kernel<T>, dim3(gm.rb, gm.groups), dim3(NT), lds, st, (const T*)dy, (const T*)y, (T*)g, M, C, db, gm.rpb, gm.tx, gm.ty, m_dev, slots););
    MG_CHECK_LAUNCH();
    if (slots) return mg_det_reduce1(slots, gm.rb, db, C, st);
    return 0;
}

extern "C" int mg_colstats_centered_dev(const void* x, int dtype, int M, int C, int ld, float* stats, int have_sum, const int32_t* m_dev, void* stream);
extern "C" int mg_colstats_centered(const void* x, int dtype, int M, int C, int ld, float* stats, int have_sum, void* stream) {
    return mg_colstats_centered_dev(x, dtype, M, C, ld, stats, have_sum, nullptr, stream);
}
extern "C" int mg_colstats_centered_dev(const void* x, int dtype, int M, int C, int ld, float* stats, int have_sum, const int32_t* m_dev, void* stream) {
    if (M <= 0) return 0;
    const int ce = MG_IS16(dtype) ? 8 : 4;
    if (C % ce || ld % ce) return -3;
    const ColGeom g = col_geom(M, C, ce, 256);
    const size_t lds = (size_t)g.ty * g.tx * 2 * ce * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    // `stats` must arrive zeroed (the caller hands out slices of a per-step zero arena): pass 1 adds the column sums only
    // (skipped when the producing conv's epilogue already did: have_sum), pass 2 the centred second moments.
    // Deterministic mode: each pass stores one partial row per row block, mg_det_reduce adds them in order (two more small launches).
    float* slots = nullptr;
    if (mg_det_on && g.rb > 1) { slots = mg_det_scratch_on((long)g.rb * C, st); if (!slots) return MG_DET_NO_SCRATCH; }
    MG_WITH_DTYPE(dtype, T,
        if (!have_sum) {
            hipLaunchKernelGGL(colstats_kernel<T>, dim3(g.rb, g.groups), dim3(NT), lds, st, (const T*)x, M, C, ld, stats, g.rpb, 1, 1, g.tx, g.ty, m_dev, slots);
            if (slots) { int rc_ = mg_det_reduce1(slots, g.rb, stats, C, st); if (rc_) return rc_; }
        }
        hipLaunchKernelGGL(colstats_centered_kernel<T>, dim3(g.rb, g.groups), dim3(NT), lds, st, (const T*)x, M, C, ld, stats, g.rpb, g.tx, g.ty, m_dev, slots);
        if (slots) { int rc_ = mg_det_reduce1(slots, g.rb, stats + C, C, st); if (rc_) return rc_; }
    );
    MG_CHECK_LAUNCH();
    return 0;
}

/* out[n] = sum over the nrep rows of stats[nrep][n], added in the library's fixed order (csrc/det.hip): the local [sum x | sum x^2] of a SyncBatchNorm
 * layer whose statistics arrive as one row per tile / row block, before they go into the cross-rank exchange. */
extern "C" int mg_stat_rows_sum(const float* stats, int nrep, int n, float* out, void* stream) {
    if (!stats || !out || nrep < 1 || n < 1) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = mg_zero_words(out, n, st);
    if (e != hipSuccess) return (int)e;
    return mg_det_reduce1(stats, nrep, out, n, st);
}

static int bn_finalize_launch(const float* stats, int nrep, const float* count_ptr, float count, int C, int centered, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                              float* mean_out, float* invstd_out, const int32_t* m_dev, void* stream, int count_mult = 1) {
    const float nmult = count_mult > 1 ? (float)count_mult : 1.f;
    if (nrep > MG_STAT_REPLICAS)
        hipLaunchKernelGGL(bn_finalize_rows_kernel, dim3(C), dim3(NT), 0, (hipStream_t)stream, stats, nrep, count_ptr, count, C, centered, gamma,
                           beta, running_mean, running_var, momentum, eps, scale, shift, mean_out, invstd_out, m_dev, nmult);
    else
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, stats, nrep, count_ptr, count, C, centered, gamma,
                           beta, running_mean, running_var, momentum, eps, scale, shift, mean_out, invstd_out, m_dev, nmult);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_bn_finalize(const float* stats, int nrep, const float* count_ptr, float count, int C, int centered, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                              float* mean_out, float* invstd_out, void* stream) {
    return bn_finalize_launch(stats, nrep, count_ptr, count, C, centered, gamma, beta, running_mean, running_var, momentum, eps, scale, shift, mean_out,
                              invstd_out, nullptr, stream);
}

extern "C" int mg_bn_fold(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, float* scale, float* shift, void* stream) {
    hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, C, gamma, beta, running_mean,
                       running_var, eps, scale, shift);
    MG_CHECK_LAUNCH();
    return 0;
}

static int rowwise_check(const mg_rowwise_params* p) {
    if (!p) return -1;
    const int ce = MG_IS16(p->dtype) ? 8 : 4;
    if (p->C % ce) return -3;
    return 0;
}

extern "C" int mg_affine_act(const mg_rowwise_params* p, void* stream) {
    int rc = rowwise_check(p); if (rc) return rc;
    if (p->M <= 0) return 0;
    const int ce = MG_IS16(p->dtype) ? 8 : 4;
    long total = (long)p->M * (p->C / ce);
    MG_WITH_DTYPE(p->dtype, T, hipLaunchKernelGGL(affine_act_kernel<T>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, *p););
    MG_CHECK_LAUNCH();
    return 0;
}

// OFF by default, measured (one lease, two runs each): 11.78 / 11.84 ms against 10.04 / 10.09 ms -- +1.75 ms over 59 layers, ~30 us per layer or ~120 ns per
// row block: the release fence + ticket of EVERY block (an L2 write-back each, 128-512 blocks per layer) costs several times the 5.4 us launch + 1.5 us
// kernel boundary it removes. Same verdict as the flag hand-shake of bn_bwd_coop_kernel: on this part a cross-workgroup meeting point
// inside a launch is dearer than a kernel boundary, with or without waiting. Kept for the tests and as the measured answer to "let the last block of
// the reduction do the ordered sum" (VERDICT round 5, item 4a): mg_set_bn_bwd_tail / MG_BN_BWD_TAIL=1.
static int g_bn_bwd_tail = (int)mg_env_long("MG_BN_BWD_TAIL", 0);
extern "C" int mg_set_bn_bwd_tail(int on) { const int was = g_bn_bwd_tail; g_bn_bwd_tail = on ? 1 : 0; return was; }

// `hand_over` (deterministic mode): when the partial rows number at most `hand_over_max`, they are NOT summed here -- *hand_over receives
// them ([*hand_over_rows][2C]) and the caller's apply pass adds them in row order itself (bn_bwd_apply_fixed_kernel: one launch less per layer).
static int bn_bwd_reduce_impl(const mg_rowwise_params* p, void* stream, float** hand_over, int* hand_over_rows, int hand_over_max) {
    int rc = rowwise_check(p); if (rc) return rc;
    if (hand_over) { *hand_over = nullptr; *hand_over_rows = 0; }
    if (p->M <= 0) return 0;
    const int ce = MG_IS16(p->dtype) ? 8 : 4;
    // row blocks: every block ends with one atomic per channel, all blocks on the same 2C addresses -- past ~256 blocks those serialise into a
    // tail longer than what the extra parallelism buys, except on the largest tensors (measured, us at 128 / 256 / 512 / 1024 row blocks:
    // 1M x 32: 109 / 60 / 45 / 52; 262144 x 64: 56 / 35 / 31 / 43; 262144 x 32: 29 / 21.5 / 24 / 36; 65536 x 64: 19 / 13 / 19 / 19)
    static const int env_rb = (int)mg_env_long("MG_BN_RB", 0);
    const int max_rb = env_rb > 0 ? env_rb : ((long)p->M * p->C >= (16l << 20) ? 512 : 256);
    ColGeom g = col_geom(p->M, p->C, ce, max_rb);
    // the row-block count is capped by the atomics, not by the work: when a block still walks >= 256 rows, 1024-thread blocks put four times the
    // waves (loads in flight) behind the same number of atomics (65536 x 64..128: 18.6 us with 4 waves per CU, the tensor is 16-32 MB)
    static const int wide_on = (int)mg_env_long("MG_BN_WIDE", 1);
    const bool wide = wide_on && !p->m_dev && max_rb == 256 && g.rpb >= 256 && (g.tx & (g.tx - 1)) == 0;      // (the >= 16 M element layers: 25 -> 36 us)
    if (wide) g = col_geom(p->M, p->C, ce, max_rb, 1024, 2);
    const size_t lds = wide ? (size_t)16 * g.tx * 2 * ce * sizeof(float) : (size_t)g.ty * g.tx * 2 * ce * sizeof(float);
    // deterministic mode: one partial row [2C] per row block in the slot scratch, added in row-block order by mg_det_reduce into p->sums
    float* slots = nullptr;
    if (mg_det_on && g.rb > 1) { slots = mg_det_scratch_on((long)g.rb * 2 * p->C, (hipStream_t)stream); if (!slots) return MG_DET_NO_SCRATCH; }
    // MG_BN_BWD_TAIL=1: the ordered sum of the partial rows rides in the tail of this launch (last-arriver form, see the kernel) instead of its own launch
    unsigned* tail = nullptr;
    if (g_bn_bwd_tail && slots && !(hand_over && g.rb <= hand_over_max) && g.groups <= MG_TAIL_WORDS && g.tx * ce * 2 * MG_DET_CHUNKS * sizeof(float) <= lds)
        tail = mg_det_tail_words((hipStream_t)stream);
    if (wide) {
        MG_WITH_DTYPE(p->dtype, T, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, 1024>), dim3(g.rb, g.groups), dim3(1024), lds, (hipStream_t)stream, *p, g.rpb, g.tx, g.ty, slots, tail););
    } else MG_WITH_DTYPE(p->dtype, T, hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(g.rb, g.groups), dim3(NT), lds, (hipStream_t)stream, *p, g.rpb, g.tx, g.ty, slots, tail););
    MG_CHECK_LAUNCH();
    if (tail) return 0;                                        // the last row block of every channel group added the rows itself
    if (slots && hand_over && g.rb <= hand_over_max) { *hand_over = slots; *hand_over_rows = g.rb; return 0; }
    if (slots) return mg_det_reduce1(slots, g.rb, p->sums, 2 * p->C, (hipStream_t)stream);
    return 0;
}
extern "C" int mg_bn_bwd_reduce(const mg_rowwise_params* p, void* stream) { return bn_bwd_reduce_impl(p, stream, nullptr, nullptr, 0); }

static bool bn_fixed_shape_ok(const mg_rowwise_params& p) {
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    const int cpr = p.C / ce;
    return p.M > 0 && cpr > 0 && cpr <= NT && (NT % cpr) == 0 && p.ldx % ce == 0 && p.lddy % ce == 0 && (!p.dx || p.lddx % ce == 0) &&
           (!p.dres || p.lddres % ce == 0);
}
static bool bn_fixed_ok(const mg_rowwise_params& p) {
    // the general apply pass stays on the simple grid-stride kernel (8.0 us average against 8.9 us for this one at nrep = 1: more registers,
    // fewer waves in flight); this kernel serves the linked path (replicated sums). MG_BN_FIXED_APPLY=1 uses it everywhere.
    static const int on = (int)mg_env_long("MG_BN_FIXED_APPLY", 0);
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    const int cpr = p.C / ce;
    return on && p.M > 0 && cpr > 0 && cpr <= NT && (NT % cpr) == 0 && p.ldx % ce == 0 && p.lddy % ce == 0 && (!p.dx || p.lddx % ce == 0) &&
           (!p.dres || p.lddres % ce == 0);
}
static int bn_bwd_apply_fixed_launch(const mg_rowwise_params& p, const float* sums_rep, int nrep, int premasked, float* sums_out, hipStream_t st) {
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    const long total = (long)p.M * (p.C / ce);
    MG_WITH_DTYPE(p.dtype, T, hipLaunchKernelGGL(bn_bwd_apply_fixed_kernel<T>, dim3(grid_for(total)), dim3(NT), (size_t)(NT + 2 * p.C) * sizeof(float), st, p, sums_rep, nrep, premasked, sums_out););
    MG_CHECK_LAUNCH();
    return 0;
}

/* BatchNorm backward, apply pass only, for a layer whose reductions were accumulated by the consumer conv's data-gradient epilogue
 * (mg_conv_params.bnb_*): p->dy = g (already dy * act'(y)), sums_rep = nrep replicas of [2C]; sums_out [2C] receives dbeta | dgamma. */
extern "C" int mg_bn_bwd_apply_linked(const mg_rowwise_params* p, const float* sums_rep, int nrep, float* sums_out, void* stream) {
    int rc = rowwise_check(p); if (rc) return rc;
    if (!sums_rep || nrep < 1 || !sums_out) return -2;
    if (!bn_fixed_shape_ok(*p)) return -3;
    return bn_bwd_apply_fixed_launch(*p, sums_rep, nrep, 1, sums_out, (hipStream_t)stream);
}

extern "C" int mg_bn_bwd_apply(const mg_rowwise_params* p, void* stream) {
    int rc = rowwise_check(p); if (rc) return rc;
    if (p->M <= 0) return 0;
    if (bn_fixed_ok(*p)) return bn_bwd_apply_fixed_launch(*p, p->sums, 1, 0, nullptr, (hipStream_t)stream);
    const int ce = MG_IS16(p->dtype) ? 8 : 4;
    long total = (long)p->M * (p->C / ce);
    MG_WITH_DTYPE(p->dtype, T, hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, *p););
    MG_CHECK_LAUNCH();
    return 0;
}

// =====================================================================================================================
// Small BatchNorm layers in ONE launch per direction (M <= 4096 rows: the OS16 / OS32 layers, ~30 of the 71 per step).
// A workgroup OWNS one 16-byte channel chunk (8 bf16 / 4 fp32 channels) over all rows: every thread keeps its <= 16 rows of the chunk in
// registers, so x is read once, the exact two-pass variance comes from registers, and -- because no other workgroup touches these
// channels -- there are no atomics, no zeroed accumulators and no cross-workgroup ordering: statistics, finalize (scale / shift / mean /
// invstd, running statistics) and apply are one kernel (were 4 launches, ~25 us at the ~5 us latency floor each); backward: reduce + apply
// in one (were 2). The strided 16-byte column reads are served from L2 (these tensors are <= 4 MB).
// =====================================================================================================================
template <int CE>
__device__ __forceinline__ void block_sum_vec(float* v, float* sred) {            // sum of v[0..CE) over the 256 threads, result in every thread
#pragma unroll
    for (int e = 0; e < CE; ++e) v[e] = wave_sum(v[e]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                                              // sred may still be read from the previous reduction
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < CE; ++e) sred[wave * CE + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < CE; ++e) v[e] = (sred[e] + sred[CE + e]) + (sred[2 * CE + e] + sred[3 * CE + e]);
}

template <typename T, int RPT>
__global__ __launch_bounds__(NT) void bn_small_fwd_kernel(const mg_rowwise_params p, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* running_mean, float* running_var, float momentum, float eps, float* __restrict__ outs) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    __shared__ float sred[4 * CE];
    const int c0 = blockIdx.x * CE, t = threadIdx.x, M = p.M, C = p.C;
    const T* __restrict__ x = (const T*)p.x;
    const T* __restrict__ r1 = (const T*)p.res;
    const T* __restrict__ r2 = (const T*)p.res2;
    // PRE (the <= 1024-row layers, RPT == 4): the residual rows are requested together with the x rows -- they do not depend on the statistics, and
    // asked for after the two block reductions they were one more exposed memory round trip in a kernel that is nothing but round trips
    constexpr bool PRE = RPT <= 4;
    uint4 q[RPT], qa[PRE ? RPT : 1], qb[PRE ? RPT : 1];
    float s[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) s[e] = 0.f;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int m = t + k * NT;
        q[k] = m < M ? *(const uint4*)(x + (long)m * p.ldx + c0) : make_uint4(0, 0, 0, 0);
    }
    if constexpr (PRE) {
#pragma unroll
        for (int k = 0; k < (PRE ? RPT : 1); ++k) { qa[k] = make_uint4(0, 0, 0, 0); qb[k] = qa[k]; }
        if (r1) {
#pragma unroll
            for (int k = 0; k < (PRE ? RPT : 1); ++k) {
                const int m = t + k * NT;
                if (m < M) {
                    long rrow = m;
                    if (p.res_mode == 2) {
                        const int hw = p.H * p.W; const int n = m / hw; const int rem = m - n * hw; const int ho = rem / p.W; const int wo = rem - ho * p.W;
                        rrow = ((long)n * (p.H >> 1) + (ho >> 1)) * (p.W >> 1) + (wo >> 1);
                    }
                    qa[k] = *(const uint4*)(r1 + rrow * p.ldr + c0);
                }
            }
        }
        if (r2) {
#pragma unroll
            for (int k = 0; k < (PRE ? RPT : 1); ++k) {
                const int m = t + k * NT;
                if (m < M) qb[k] = *(const uint4*)(r2 + (long)m * p.ldr2 + c0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        float f[CE];
        TR::unpack(q[k], f);
#pragma unroll
        for (int e = 0; e < CE; ++e) s[e] += f[e];                               // rows beyond M hold zeros
    }
    block_sum_vec<CE>(s, sred);
    const float inv_n = 1.f / (float)M;
    float mean[CE], var[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { mean[e] = s[e] * inv_n; var[e] = 0.f; }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        if (t + k * NT < M) {
            float f[CE];
            TR::unpack(q[k], f);
#pragma unroll
            for (int e = 0; e < CE; ++e) { const float d = f[e] - mean[e]; var[e] += d * d; }
        }
    }
    block_sum_vec<CE>(var, sred);
    float sc[CE], sh[CE], invstd[CE], gam[CE], bet[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { gam[e] = gamma ? gamma[c0 + e] : 1.f; bet[e] = beta ? beta[c0 + e] : 0.f; }
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        var[e] = fmaxf(var[e] * inv_n, 0.f);
        invstd[e] = rsqrtf(var[e] + eps);
        sc[e] = gam[e] * invstd[e]; sh[e] = bet[e] - mean[e] * gam[e] * invstd[e];
    }
    if (t == 0) {
        // the running statistics of the chunk are READ as one batch before anything is stored: written as load -> store per channel, the possible
        // aliasing of the four destination arrays made every load wait for the store in front of it -- 2 * CE dependent round trips in one thread
        // while the rest of the workgroup had long finished (hipcc -S: 16 of this kernel's 24 full waits)
        float rm[CE], rv[CE];
        if (running_mean) {
#pragma unroll
            for (int e = 0; e < CE; ++e) { rm[e] = running_mean[c0 + e]; rv[e] = running_var[c0 + e]; }
        }
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            const int c = c0 + e;
            outs[c] = sc[e]; outs[C + c] = sh[e]; outs[2 * C + c] = mean[e]; outs[3 * C + c] = invstd[e];
        }
        if (running_mean) {
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                const float n = (float)M * (p.count_mult > 1 ? (float)p.count_mult : 1.f), unbiased = n > 1.f ? var[e] * n / (n - 1.f) : var[e];
                running_mean[c0 + e] = (1.f - momentum) * rm[e] + momentum * mean[e];
                running_var[c0 + e] = (1.f - momentum) * rv[e] + momentum * unbiased;
            }
        }
    }
    T* __restrict__ y = (T*)p.y;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int m = t + k * NT;
        if (m >= M) continue;
        float f[CE], a[CE], b[CE];
        TR::unpack(q[k], f);
        if constexpr (PRE) {
            TR::unpack(qa[k], a);
            TR::unpack(qb[k], b);
#pragma unroll
            for (int e = 0; e < CE; ++e) f[e] = apply_act(f[e] * sc[e] + sh[e] + a[e], p.act, p.slope) + b[e];
            *(uint4*)(y + (long)m * p.ldy + p.yoff + c0) = TR::pack(f);
            continue;
        }
#pragma unroll
        for (int e = 0; e < CE; ++e) { a[e] = 0.f; b[e] = 0.f; }
        if (r1) {
            long rrow = m;
            if (p.res_mode == 2) {
                const int hw = p.H * p.W; const int n = m / hw; const int rem = m - n * hw; const int ho = rem / p.W; const int wo = rem - ho * p.W;
                rrow = ((long)n * (p.H >> 1) + (ho >> 1)) * (p.W >> 1) + (wo >> 1);
            }
            TR::unpack(*(const uint4*)(r1 + rrow * p.ldr + c0), a);
        }
        if (r2) TR::unpack(*(const uint4*)(r2 + (long)m * p.ldr2 + c0), b);
#pragma unroll
        for (int e = 0; e < CE; ++e) f[e] = apply_act(f[e] * sc[e] + sh[e] + a[e], p.act, p.slope) + b[e];
        *(uint4*)(y + (long)m * p.ldy + p.yoff + c0) = TR::pack(f);
    }
}

template <typename T, int RPT>
__global__ __launch_bounds__(NT) void bn_small_bwd_kernel(const mg_rowwise_params p) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    __shared__ float sred[4 * CE];
    const int c0 = blockIdx.x * CE, t = threadIdx.x, M = p.M, C = p.C;
    float mu[CE], is[CE], sg[CE], sgx[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { mu[e] = p.mean[c0 + e]; is[e] = p.invstd[c0 + e]; sg[e] = 0.f; sgx[e] = 0.f; }
    float g[RPT][CE];
    uint4 qx[RPT];
    if constexpr (RPT <= 4) {
        // the <= 1024-row layers: every row of dy, x and (stored-activation form) y / res2 is requested before the first is used. load_g() per row
        // compiled to load dy -> wait -> load y -> wait -> load x -> wait, row after row: 12 dependent round trips for 4 rows (hipcc -S). Rows past M
        // read row M - 1 (M > 1 here) and are zeroed after the fact, so that no load sits behind a per-lane condition.
        const bool from_x = p.act != MG_ACT_NONE && p.mask_from_x, from_y = p.act != MG_ACT_NONE && !p.mask_from_x;
        uint4 qd[RPT], qy[RPT], qr[RPT];
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int m = min(t + k * NT, M - 1);
            qd[k] = *(const uint4*)((const T*)p.dy + (long)m * p.lddy + c0);
            qx[k] = *(const uint4*)((const T*)p.x + (long)m * p.ldx + c0);
            qy[k] = make_uint4(0, 0, 0, 0); qr[k] = qy[k];
        }
        if (from_y) {
#pragma unroll
            for (int k = 0; k < RPT; ++k) qy[k] = *(const uint4*)((const T*)p.y + (long)min(t + k * NT, M - 1) * p.ldy + p.yoff + c0);
            if (p.res2) {
#pragma unroll
                for (int k = 0; k < RPT; ++k) qr[k] = *(const uint4*)((const T*)p.res2 + (long)min(t + k * NT, M - 1) * p.ldr2 + c0);
            }
        }
        float xsc[CE], xsh[CE];
#pragma unroll
        for (int e = 0; e < CE; ++e) { xsc[e] = from_x ? p.scale[c0 + e] : 0.f; xsh[e] = from_x ? p.shift[c0 + e] : 0.f; }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const bool live = t + k * NT < M;
            float xv[CE];
            TR::unpack(qd[k], g[k]);
            TR::unpack(qx[k], xv);
            if (from_x) {                                    // the arithmetic of load_g(): sign of x * scale + shift
#pragma unroll
                for (int e = 0; e < CE; ++e) {
                    const float z = xv[e] * xsc[e] + xsh[e];
                    if (!(z > 0.f)) g[k][e] = (p.act == MG_ACT_RELU) ? 0.f : g[k][e] * p.slope;
                }
            } else if (from_y) {                             // y = act(.) + res2 -> the activation output's sign
                float yv[CE], rb[CE];
                TR::unpack(qy[k], yv);
                TR::unpack(qr[k], rb);
                if (p.res2) {
#pragma unroll
                    for (int e = 0; e < CE; ++e) yv[e] -= rb[e];
                }
#pragma unroll
                for (int e = 0; e < CE; ++e) {
                    if (!(yv[e] > 0.f)) g[k][e] = (p.act == MG_ACT_RELU) ? 0.f : g[k][e] * p.slope;
                }
            }
            if (live) {
#pragma unroll
                for (int e = 0; e < CE; ++e) { sg[e] += g[k][e]; sgx[e] += g[k][e] * (xv[e] - mu[e]) * is[e]; }
            } else {
                qx[k] = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < CE; ++e) g[k][e] = 0.f;
            }
        }
    } else {
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int m = t + k * NT;
        if (m < M) {
            load_g<T>(p, m, c0, g[k]);
            qx[k] = *(const uint4*)((const T*)p.x + (long)m * p.ldx + c0);
            float xv[CE];
            TR::unpack(qx[k], xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) { sg[e] += g[k][e]; sgx[e] += g[k][e] * (xv[e] - mu[e]) * is[e]; }
        } else {
            qx[k] = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < CE; ++e) g[k][e] = 0.f;
        }
    }
    }
    block_sum_vec<CE>(sg, sred);
    block_sum_vec<CE>(sgx, sred);
    if (t == 0) {
#pragma unroll
        for (int e = 0; e < CE; ++e) { p.sums[c0 + e] = sg[e]; p.sums[C + c0 + e] = sgx[e]; }
    }
    const float inv_n = 1.f / p.count;
    float sc[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) sc[e] = p.scale[c0 + e];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int m = t + k * NT;
        if (m >= M) continue;
        if (p.dres) *(uint4*)((T*)p.dres + (long)m * p.lddres + c0) = TR::pack(g[k]);
        if (p.dx) {
            float xv[CE], o[CE];
            TR::unpack(qx[k], xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                const float xh = (xv[e] - mu[e]) * is[e];
                float v = sc[e] * (g[k][e] - sg[e] * inv_n - xh * sgx[e] * inv_n);
                if (p.mask_x_pos && !(xv[e] > 0.f)) v = 0.f;
                o[e] = v;
            }
            *(uint4*)((T*)p.dx + (long)m * p.lddx + c0) = TR::pack(o);
        }
    }
}

static bool bn_small_ok(const mg_rowwise_params& p) {
    // rows up to which the one-launch form is used: a workgroup reads its 16-byte column slice with a row stride, i.e. one cache line per
    // lane -- at 4096 rows x 32 workgroups that costs as much as the four coalesced launches it replaces (24.8 us forward, 33.7 us backward
    // against ~25 / ~17 us); at 1024 rows (64 workgroups x 4 rows per thread) it is 12 us each way. MG_BN_SMALL_ROWS=0 switches it off.
    static const int max_rows = (int)mg_env_long("MG_BN_SMALL_ROWS", 1024);
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    return !p.m_dev && !p.count_ptr && p.M > 1 && p.M <= max_rows && p.M <= 16 * NT && p.C % ce == 0 && p.ldx % ce == 0;
}
template <typename T>
static int bn_small_fwd_launch(const mg_rowwise_params& p, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                               float eps, float* outs, hipStream_t st) {
    const int ce = ElemTraits<T>::CE;
    dim3 grid(p.C / ce);
    if (p.M <= 4 * NT) hipLaunchKernelGGL((bn_small_fwd_kernel<T, 4>), grid, dim3(NT), 0, st, p, gamma, beta, running_mean, running_var, momentum, eps, outs);
    else if (p.M <= 8 * NT) hipLaunchKernelGGL((bn_small_fwd_kernel<T, 8>), grid, dim3(NT), 0, st, p, gamma, beta, running_mean, running_var, momentum, eps, outs);
    else hipLaunchKernelGGL((bn_small_fwd_kernel<T, 16>), grid, dim3(NT), 0, st, p, gamma, beta, running_mean, running_var, momentum, eps, outs);
    MG_CHECK_LAUNCH();
    return 0;
}
template <typename T>
static int bn_small_bwd_launch(const mg_rowwise_params& p, hipStream_t st) {
    const int ce = ElemTraits<T>::CE;
    dim3 grid(p.C / ce);
    if (p.M <= 4 * NT) hipLaunchKernelGGL((bn_small_bwd_kernel<T, 4>), grid, dim3(NT), 0, st, p);
    else if (p.M <= 8 * NT) hipLaunchKernelGGL((bn_small_bwd_kernel<T, 8>), grid, dim3(NT), 0, st, p);
    else hipLaunchKernelGGL((bn_small_bwd_kernel<T, 16>), grid, dim3(NT), 0, st, p);
    MG_CHECK_LAUNCH();
    return 0;
}

static bool bn_fused_ok(const mg_rowwise_params& p) {
    // off by default: 0.89 ms per step against 0.98 ms for finalize + apply in the kernel trace, but nothing on the step's wall clock (13.48 vs
    // 13.43-13.50 ms over 60-step runs): its register footprint (per-channel constants + the prefetched row) costs the streaming part what the
    // removed launch saved. MG_BN_FUSED_APPLY=1 switches it on.
    static const int on = (int)mg_env_long("MG_BN_FUSED_APPLY", 0);
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    const int cpr = p.C / ce;
    return on && p.M > 0 && cpr > 0 && cpr <= NT && (NT % cpr) == 0 && p.ldx % ce == 0;
}
static int bn_apply_fused_launch(const mg_rowwise_params& p, const float* stats, int nrep, int centered, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* outs, hipStream_t st) {
    const int ce = MG_IS16(p.dtype) ? 8 : 4;
    const long total = (long)p.M * (p.C / ce);
    BnFin f{stats, nrep, centered, gamma, beta, running_mean, running_var, momentum, eps, outs};
    MG_WITH_DTYPE(p.dtype, T, hipLaunchKernelGGL(bn_apply_fused_kernel<T>, dim3(grid_for(total)), dim3(NT), (size_t)(NT + 2 * p.C) * sizeof(float), st, p, f););
    MG_CHECK_LAUNCH();
    return 0;
}

// ---- one-call training BatchNorm (the four / two launches above behind ONE entry point: the per-call host cost of the Python
// binding -- argument marshalling, allocations, autograd bookkeeping -- is paid once instead of per kernel; this matters for the
// host-paced sparse head, where a BatchNorm forward cost 51 us of host time for ~15 us of kernels) ------------------------------
extern "C" int mg_bn_train_fwd(const mg_rowwise_params* p_in, float* stats_ws, int ws_zeroed, float* outs, const float* stats_in,
                               int stats_in_rows, int exact, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, void* stream) {
    int rc = rowwise_check(p_in); if (rc) return rc;
    mg_rowwise_params p = *p_in;
    const int C = p.C;
    hipStream_t st = (hipStream_t)stream;
    float* own = stats_ws;                               // [2C] (exact) or [MG_STAT_REPLICAS][2C] statistics scratch; outs: scale | shift | mean | invstd
    if (!stats_in && !own) return -3;
    if (exact && bn_small_ok(p) && p.y)                  // one launch: the statistics never leave the registers (stats_in / stats_ws unused)
        return p.dtype == MG_BF16 ? bn_small_fwd_launch<bf16raw>(p, gamma, beta, running_mean, running_var, momentum, eps, outs, st)
               : p.dtype == MG_F16 ? bn_small_fwd_launch<f16raw>(p, gamma, beta, running_mean, running_var, momentum, eps, outs, st)
                                   : bn_small_fwd_launch<float>(p, gamma, beta, running_mean, running_var, momentum, eps, outs, st);
    const float* stats = stats_in;
    int nrep = stats_in_rows, centered = 0;
    if (mg_det_on) {
        // deterministic mode: one-pass statistics with one row per row block / conv output tile (`own`: [MG_DET_STAT_ROWS][2C]), added in row
        // order by bn_finalize_rows_kernel. The two-pass variance needs the column sums BEFORE its second pass, i.e. a cross-workgroup sum in the
        // middle of the layer: it stays with the <= 1024-row layers, which run it inside one workgroup (bn_small, above).
        //
        // fp32 storage (round 5, ADVICE medium): the one-pass E[x^2] - E[x]^2 loses var's digits when |mean| >> std, and with fp32 storage nothing else
        // hides that (16-bit storage rounds x itself to 2^-8 |x| first). Layers the caller marks `exact` (<= EXACT_STATS_ROWS rows) and the sparse
        // head's device-row-count layers therefore keep the two-pass variance here too, in its ordered form: column sums by row blocks -> slots ->
        // ordered sum, centred second moments the same way (mg_colstats_centered_dev; four small launches, parity mode only).
        if (p.dtype == MG_F32 && (exact || p.m_dev) && !stats) {
            if (!own) return -3;
            if (!ws_zeroed) { hipError_t e = mg_zero_words(own, 2 * C, st); if (e != hipSuccess) return (int)e; }
            if (p.M > 0) { rc = mg_colstats_centered_dev(p.x, p.dtype, p.M, C, p.ldx, own, 0, p.m_dev, stream); if (rc) return rc; }
            p.count = (float)p.M;
            rc = bn_finalize_launch(own, 1, nullptr, (float)p.M, C, 1, gamma, beta, running_mean, running_var, momentum, eps, outs, outs + C, outs + 2 * C,
                                    outs + 3 * C, p.m_dev, stream, p.count_mult);
            if (rc) return rc;
            p.scale = outs; p.shift = outs + C;
            return p.y ? mg_affine_act(&p, stream) : 0;
        }
        if (!stats) {
            if (!own) return -3;
            if (!ws_zeroed) { hipError_t e = mg_zero_words(own, (long)MG_DET_STAT_ROWS * 2 * C, st); if (e != hipSuccess) return (int)e; }
            if (p.M > 0) { rc = mg_colstats_dev(p.x, p.dtype, p.M, C, p.ldx, own, p.m_dev, stream); if (rc) return rc; }
            stats = own; nrep = MG_DET_STAT_ROWS;
        } else if (exact && stats_in_rows == 1) return -3;       // a sums-only row of a conv epilogue is not reproducible: callers hand over row sets
        p.count = (float)p.M;
        rc = bn_finalize_launch(stats, nrep, nullptr, (float)p.M, C, 0, gamma, beta, running_mean, running_var, momentum, eps, outs, outs + C, outs + 2 * C,
                                outs + 3 * C, p.m_dev, stream, p.count_mult);
        if (rc) return rc;
        p.scale = outs; p.shift = outs + C;
        return p.y ? mg_affine_act(&p, stream) : 0;          // (y == NULL: the consumer applies scale | shift to its operand, mg_conv_params.xf_*)
    }
    if (p.m_dev) {
        // sparse head: the row count is a device word -> always the exact two-pass variance over min(*m_dev, M) rows (no host knowledge of
        // the count is needed to choose a path), statistics in `own` [2C]
        if (!own) return -3;
        if (!ws_zeroed) { hipError_t e = mg_zero_words(own, 2 * C, st); if (e != hipSuccess) return (int)e; }
        if (p.M > 0) { rc = mg_colstats_centered_dev(p.x, p.dtype, p.M, C, p.ldx, own, 0, p.m_dev, stream); if (rc) return rc; }
        if (bn_fused_ok(p) && p.y) return bn_apply_fused_launch(p, own, 1, 1, gamma, beta, running_mean, running_var, momentum, eps, outs, st);
        rc = bn_finalize_launch(own, 1, nullptr, (float)p.M, C, 1, gamma, beta, running_mean, running_var, momentum, eps, outs, outs + C, outs + 2 * C,
                                outs + 3 * C, p.m_dev, stream, p.count_mult);
        if (rc) return rc;
        p.scale = outs; p.shift = outs + C;
        return p.y ? mg_affine_act(&p, stream) : 0;          // (y == NULL: the consumer applies scale | shift to its operand, mg_conv_params.xf_*)
    }
    if (exact) {
        // two-pass variance; a 1-row stats_in already carries the column sums from the producing conv's epilogue
        float* row = stats_in ? (float*)stats_in : own;
        if (!stats_in && !ws_zeroed) { hipError_t e = mg_zero_words(own, 2 * C, st); if (e != hipSuccess) return (int)e; }
        rc = mg_colstats_centered(p.x, p.dtype, p.M, C, p.ldx, row, stats_in ? 1 : 0, stream); if (rc) return rc;
        stats = row; nrep = 1; centered = 1;
    } else if (!stats_in) {
        if (!ws_zeroed) { hipError_t e = mg_zero_words(own, (long)MG_STAT_REPLICAS * 2 * C, st); if (e != hipSuccess) return (int)e; }
        rc = mg_colstats(p.x, p.dtype, p.M, C, p.ldx, own, stream); if (rc) return rc;
        stats = own; nrep = MG_STAT_REPLICAS;
    }
    p.count = (float)p.M;
    if (bn_fused_ok(p) && p.y) return bn_apply_fused_launch(p, stats, nrep, centered, gamma, beta, running_mean, running_var, momentum, eps, outs, st);
    rc = bn_finalize_launch(stats, nrep, nullptr, (float)p.M, C, centered, gamma, beta, running_mean, running_var, momentum, eps, outs, outs + C,
                            outs + 2 * C, outs + 3 * C, nullptr, stream, p.count_mult);
    if (rc) return rc;
    p.scale = outs; p.shift = outs + C;
    return p.y ? mg_affine_act(&p, stream) : 0;
}


// =====================================================================================================================
// Training BatchNorm backward as ONE launch for the mid-size layers (round 5): reduce -> ordered sum -> apply used to be three launches
// (bn_bwd_reduce 10 us + det_reduce 5 us + bn_bwd_apply 8 us per layer, dz and x read twice). Here every workgroup owns a (row block, 32-channel
// group), keeps its rows of dz and x IN REGISTERS (<= 8 rows per thread: the layer fits the chip's register file), writes its partial
// sums [sum g | sum g xhat] as one 64-float row, and meets the other row blocks of its channel group in a flag hand-shake -- no atomics:
// a workgroup stores its arrival flag (release), then polls the <= 256 flags of its group with one coalesced load per round. The rows are then
// added in row-block order by every workgroup for itself (4 row lanes x 64 columns, fixed tree: the result depends on the launch geometry
// only) and the apply pass runs from the registers: dz and x are read once, dx written once.
// Generation scheme instead of a reset: the flags carry generation G + 1, G is read from a device word at kernel entry and bumped by
// workgroup (0, 0) after ITS wait -- every workgroup has read G by then (it could not have arrived otherwise) -- so a replayed graph needs no
// memset between replays. The grid is at most 256 workgroups of 256 threads (one per CU: co-resident by construction); a peer that does not
// arrive within the spin budget sets the sticky error word (mg_coop_error) instead of hanging the GPU.
// =====================================================================================================================
constexpr int COOP_TX = 4, COOP_TY = NT / COOP_TX, COOP_CH = 32;          // 4 lanes x 8 channels = one 32-channel group per workgroup

template <typename T, int KEEP>
__global__ __launch_bounds__(NT) void bn_bwd_coop_kernel(const mg_rowwise_params p, int rb, int rpb, unsigned long long* __restrict__ sync, float* __restrict__ slots) {
    using TR = ElemTraits<T>;
    constexpr int CE = TR::CE;
    static_assert(CE == 8 && KEEP <= 8, "16-bit storage, at most 8 rows per thread");
    __shared__ float sred[NT / 64][COOP_TX * 2 * CE];
    __shared__ float stot[4][2 * COOP_CH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ix = t & (COOP_TX - 1), iy = t / COOP_TX;
    const int b = blockIdx.x, g = blockIdx.y, C = p.C;
    const int c0 = g * COOP_CH + ix * CE;
    const int mbeg = b * rpb, mend = min(p.M, mbeg + rpb);
    // hand-shake words (64-bit): generation of channel group g at [8 + g], arrival flags of its row blocks at [128 + g * rb + b]. A flag carries
    // (generation + 1, group, row-block count): words left behind by other layers (another geometry maps other (g, b) pairs to the same word) or by
    // earlier launches can never compare equal.
    unsigned long long* gen_w = sync + 8 + g;
    unsigned long long* flags = sync + 128 + (size_t)g * rb;
    const unsigned long long gen = __hip_atomic_load(gen_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
    const unsigned long long want = (gen << 16) | ((unsigned long long)g << 9) | (unsigned long long)rb;
    float mu[CE], is[CE], sc[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { mu[e] = p.mean[c0 + e]; is[e] = p.invstd[c0 + e]; sc[e] = p.scale[c0 + e]; }
    const float sl = p.act == MG_ACT_RELU ? 0.f : p.slope;     // what a masked element's gradient is multiplied by
    // ---- phase 1: this thread's rows -> registers (raw dz, x, one mask bit per element), partial sums
    uint4 qd[KEEP], qx[KEEP];
    unsigned long long mk = 0ull;                             // bit (k * 8 + e): the activation passes the gradient of element e of row k unchanged
    float part[2 * CE];
#pragma unroll
    for (int e = 0; e < 2 * CE; ++e) part[e] = 0.f;
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int m = mbeg + iy + k * COOP_TY;
        qd[k] = make_uint4(0, 0, 0, 0); qx[k] = make_uint4(0, 0, 0, 0);
        if (m < mend) {
            float gv[CE], dv[CE], xv[CE];
            load_g<T>(p, m, c0, gv);                            // dz * act'(.) (mask from y, or re-formed from x: mask_from_x)
            qd[k] = *(const uint4*)((const T*)p.dy + (long)m * p.lddy + c0);
            qx[k] = *(const uint4*)((const T*)p.x + (long)m * p.ldx + c0);
            TR::unpack(qd[k], dv);
            TR::unpack(qx[k], xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
                if (gv[e] == dv[e]) mk |= 1ull << (k * 8 + e);
                part[e] += gv[e]; part[CE + e] += gv[e] * (xv[e] - mu[e]) * is[e];
            }
        }
    }
    // rows of a wave meet by butterfly over the lanes that share a channel chunk, the four waves through LDS in wave order
    for (int off = COOP_TX; off < 64; off <<= 1) {
#pragma unroll
        for (int e = 0; e < 2 * CE; ++e) part[e] += __shfl_xor(part[e], off);
    }
    if (lane < COOP_TX) {
#pragma unroll
        for (int e = 0; e < 2 * CE; ++e) sred[wave][ix * 2 * CE + e] = part[e];
    }
    __syncthreads();
    if (t < 2 * COOP_CH) {
        // column t of the row: accumulator a = t / 32 (0: sum g, 1: sum g xhat), channel ch = t % 32 -> lane cx = ch / 8, element e = ch % 8
        const int a = t / COOP_CH, ch = t - a * COOP_CH, cx = ch / CE, e = ch - cx * CE;
        const int j = cx * 2 * CE + a * CE + e;
        slots[((size_t)g * rb + b) * (2 * COOP_CH) + t] = (sred[0][j] + sred[1][j]) + (sred[2][j] + sred[3][j]);
    }
    // ---- arrival: the row is visible device-wide before the flag is; then wait for the rb flags of this channel group
    __threadfence();
    __syncthreads();
    if (t == 0) __hip_atomic_store(flags + b, want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    int ok_all = 0;
    for (int spin = 0; spin < (1 << 18); ++spin) {
        const int ok = (t >= rb) || (__hip_atomic_load(flags + t, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == want);
        ok_all = __syncthreads_and(ok);
        if (ok_all) break;
        __builtin_amdgcn_s_sleep(4);
    }
    if (!ok_all && t == 0) __hip_atomic_store((unsigned*)sync + 1, 1u + (unsigned)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (b == 0 && t == 0) __hip_atomic_store(gen_w, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // every workgroup of the group has read the old generation
    // ---- the rb rows of this channel group, added in row order: 4 row lanes x 64 columns, then a fixed combine
    {
        const int col = t & (2 * COOP_CH - 1), rl = t / (2 * COOP_CH);
        const float* base = slots + (size_t)g * rb * (2 * COOP_CH) + col;
        float a0 = 0.f;
        for (int r = rl; r < rb; r += 4) a0 += base[(size_t)r * (2 * COOP_CH)];
        stot[rl][col] = a0;
    }
    __syncthreads();
    float sg[CE], sgx[CE];
    const float inv_n = 1.f / p.count;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int c = ix * CE + e;
        sg[e] = ((stot[0][c] + stot[1][c]) + (stot[2][c] + stot[3][c])) * inv_n;
        sgx[e] = ((stot[0][COOP_CH + c] + stot[1][COOP_CH + c]) + (stot[2][COOP_CH + c] + stot[3][COOP_CH + c])) * inv_n;
    }
    if (b == 0 && t < 2 * COOP_CH) {                          // dbeta | dgamma of this channel group
        const int a = t / COOP_CH, ch = t - a * COOP_CH;
        p.sums[a * C + g * COOP_CH + ch] = (stot[0][t] + stot[1][t]) + (stot[2][t] + stot[3][t]);
    }
    // ---- phase 2: apply from the registers
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int m = mbeg + iy + k * COOP_TY;
        if (m < mend) {
            float gv[CE], xv[CE], o[CE];
            TR::unpack(qd[k], gv);
            TR::unpack(qx[k], xv);
#pragma unroll
            for (int e = 0; e < CE; ++e) gv[e] = ((mk >> (k * 8 + e)) & 1ull) ? gv[e] : gv[e] * sl;      // the arithmetic of load_g
            if (p.dres) *(uint4*)((T*)p.dres + (long)m * p.lddres + c0) = TR::pack(gv);
            if (p.dx) {
#pragma unroll
                for (int e = 0; e < CE; ++e) {
                    const float xh = (xv[e] - mu[e]) * is[e];
                    float v = sc[e] * (gv[e] - sg[e] - xh * sgx[e]);
                    if (p.mask_x_pos && !(xv[e] > 0.f)) v = 0.f;
                    o[e] = v;
                }
                *(uint4*)((T*)p.dx + (long)m * p.lddx + c0) = TR::pack(o);
            }
        }
    }
}

static int g_bn_coop = (int)mg_env_long("MG_BN_COOP", 0);
extern "C" int mg_set_bn_coop(int on) { const int was = g_bn_coop; g_bn_coop = on ? 1 : 0; return was; }
struct CoopPlan { int rb, rpb, keep, groups; };
// the one-launch form serves 16-bit layers whose rows fit the register file: C % 32 == 0, host row count, rows per thread <= 8
static bool bn_bwd_coop_plan(const mg_rowwise_params& p, CoopPlan& pl) {
    // OFF by default (measured, profiles/r05_ab_bn_coop.txt: 12.40 / 12.43 ms against 11.24 / 11.37 ms): a software hand-shake between the workgroups of one
    // launch costs ~70 ns PER WORKGROUP on this part (tools/micro_gridbar.hip: +6 / +10 / +18 us for 64 / 128 / 256 workgroups, release fence + relaxed
    // polls; 57 us with acquire polls), a kernel boundary ~1.5 us whatever the grid -- three launches beat one with a barrier inside. Kept for the record
    // and the tests (mg_set_bn_coop / MG_BN_COOP=1).
    if (!g_bn_coop || !mg_det_on || !MG_IS16(p.dtype) || p.m_dev || p.count_ptr || p.C % COOP_CH || p.M <= 1024 || !p.dx) return false;
    if (p.ldx % 8 || p.lddy % 8 || p.lddx % 8 || (p.dres && p.lddres % 8) || (p.act != MG_ACT_NONE && !p.mask_from_x && (p.ldy % 8 || p.yoff % 8))) return false;
    pl.groups = p.C / COOP_CH;
    if (pl.groups > 64) return false;
    int rb = 256 / pl.groups;
    const int by_rows = (p.M + COOP_TY - 1) / COOP_TY;        // at least one row per thread row
    if (rb > by_rows) rb = by_rows;
    if (rb < 1) rb = 1;
    pl.rpb = (p.M + rb - 1) / rb;
    pl.rb = (p.M + pl.rpb - 1) / pl.rpb;
    const int rows_per_thread = (pl.rpb + COOP_TY - 1) / COOP_TY;
    pl.keep = rows_per_thread <= 2 ? 2 : (rows_per_thread <= 4 ? 4 : (rows_per_thread <= 8 ? 8 : 0));
    return pl.keep != 0 && pl.rb <= 256 && 2 * (128 + pl.groups * pl.rb) <= MG_COOP_WORDS;
}
template <typename T>
static int bn_bwd_coop_launch(const mg_rowwise_params& p, const CoopPlan& pl, hipStream_t st) {
    unsigned long long* sync = (unsigned long long*)mg_coop_sync();
    float* slots = mg_det_scratch((long)pl.groups * pl.rb * 2 * COOP_CH);
    if (!sync || !slots) return MG_DET_NO_SCRATCH;
    dim3 grid(pl.rb, pl.groups);
    if (pl.keep == 2) hipLaunchKernelGGL((bn_bwd_coop_kernel<T, 2>), grid, dim3(NT), 0, st, p, pl.rb, pl.rpb, sync, slots);
    else if (pl.keep == 4) hipLaunchKernelGGL((bn_bwd_coop_kernel<T, 4>), grid, dim3(NT), 0, st, p, pl.rb, pl.rpb, sync, slots);
    else hipLaunchKernelGGL((bn_bwd_coop_kernel<T, 8>), grid, dim3(NT), 0, st, p, pl.rb, pl.rpb, sync, slots);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_bn_train_bwd(const mg_rowwise_params* p, int sums_zeroed, void* stream) {
    int rc = rowwise_check(p); if (rc) return rc;
    if (bn_small_ok(*p) && p->lddy % (MG_IS16(p->dtype) ? 8 : 4) == 0)
        return p->dtype == MG_BF16 ? bn_small_bwd_launch<bf16raw>(*p, (hipStream_t)stream) : p->dtype == MG_F16 ? bn_small_bwd_launch<f16raw>(*p, (hipStream_t)stream) : bn_small_bwd_launch<float>(*p, (hipStream_t)stream);
    {
        CoopPlan pl;
        if (bn_bwd_coop_plan(*p, pl))                          // mid-size 16-bit layers: reduce + ordered sum + apply in ONE launch (sums are stored, not added)
            return p->dtype == MG_BF16 ? bn_bwd_coop_launch<bf16raw>(*p, pl, (hipStream_t)stream) : bn_bwd_coop_launch<f16raw>(*p, pl, (hipStream_t)stream);
    }
    if (!sums_zeroed) {
        hipError_t e = mg_zero_words(p->sums, 2 * p->C, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    // MG_BN_BWD_HANDOVER=n: layers with <= n row blocks skip the ordered-sum launch, the apply pass adds the partial rows itself. Off by default:
    // measured 11.97 / 11.77 ms (n = 32) against 11.74 / 11.71 ms (off) on one lease, 12.05 at n = 64 -- every workgroup of the apply pass repeats
    // the row sum in front of its streaming part, which costs what the removed ~6 us launch saved.
    static const int max_rows = (int)mg_env_long("MG_BN_BWD_HANDOVER", 0);
    float* part = nullptr;
    int nrows = 0;
    const bool can = max_rows > 0 && !p->count_ptr && bn_fixed_shape_ok(*p);
    rc = bn_bwd_reduce_impl(p, stream, can ? &part : nullptr, &nrows, max_rows); if (rc) return rc;
    if (part) return bn_bwd_apply_fixed_launch(*p, part, nrows, 0, p->sums, (hipStream_t)stream);
    return mg_bn_bwd_apply(p, stream);
}

extern "C" int mg_pool2x2(const void* in, void* out, int dtype, int op, int N, int Ho, int Wo, int C, void* stream) {
    const int ce = MG_IS16(dtype) ? 8 : 4;
    if (C % ce) return -3;
    long total = (long)N * Ho * Wo * (C / ce);
    if (total <= 0) return 0;
    int Hi = (op <= 1) ? Ho * 2 : Ho / 2, Wi = (op <= 1) ? Wo * 2 : Wo / 2;
    hipStream_t st = (hipStream_t)stream;
    dim3 g(grid_for(total)), b(NT);
    if (op < 0 || op > 3) return -2;
#define POOL_CASE(OP) hipLaunchKernelGGL((pool2x2_kernel<T, OP>), g, b, 0, st, (const T*)in, (T*)out, N, Ho, Wo, C, Hi, Wi)
    MG_WITH_DTYPE(dtype, T, switch (op) { case 0: POOL_CASE(0); break; case 1: POOL_CASE(1); break; case 2: POOL_CASE(2); break; default: POOL_CASE(3); break; });
#undef POOL_CASE
    MG_CHECK_LAUNCH();
    return 0;
}

// ---- AdaptiveAvgPool2d(1) over NHWC rows (the pooled branch of ASPP, maggie/network/module/aspp.py:24-27,50-52) -----------------------------------
// out[n][c] = mean over the HW rows of sample n, summed in fp32 in a fixed order (4 row groups per workgroup, each over its rows in order, the four
// partial sums added in group order), stored in the tensor's dtype. Backward: dx[n][r][c] = dy[n][c] / HW. One launch each way (was: cast to fp32,
// a strided torch reduction, cast back: 27 us for a 1 MB tensor; expand + divide + cast on the way back).
namespace {
template <typename T>
__global__ __launch_bounds__(256) void spatial_mean_fwd_kernel(const T* __restrict__ x, int HW, int C, int ld, float mul, T* __restrict__ out) {
    __shared__ float part[4][64];
    const int n = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    float a = 0.f;
    if (c < C) {
        const T* p = x + ((long)n * HW) * ld + c;
        // sixteen rows in flight per trip (one load -> wait -> add per row was 64 dependent round trips at 16 x 16: 17 us for a 1 MB tensor); the rows
        // are added in the same order
        for (int r0 = g; r0 < HW; r0 += 64) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = ElemTraits<T>::ld(p + (long)min(r0 + 4 * u, HW - 1) * ld);      // past the end: the last row again, not added
#pragma unroll
            for (int u = 0; u < 16; ++u) { if (r0 + 4 * u < HW) a += v[u]; }
        }
    }
    part[g][threadIdx.x & 63] = a;
    __syncthreads();
    if (g == 0 && c < C) {
        const int l = threadIdx.x;
        const float sum = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
        ElemTraits<T>::st(out + (long)n * C + c, sum * mul);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void spatial_mean_bwd_kernel(const T* __restrict__ dy, int HW, int C, T* __restrict__ dx) {
    const long total = (long)HW * C;
    const int n = blockIdx.y;
    const float inv = 1.f / (float)HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256)
        ElemTraits<T>::st(dx + (long)n * total + i, ElemTraits<T>::ld(dy + (long)n * C + (i % C)) * inv);
}
}  // namespace
extern "C" int mg_spatial_mean(const void* x, void* out, int dtype, int N, int HW, int C, int mode, int ld, void* stream) {
    if (!x || !out || N <= 0 || HW <= 0 || C <= 0 || mode < 0 || mode > 2) return -2;
    if (ld <= 0) ld = C;
    if (ld < C || (mode == 1 && ld != C)) return -2;
    const int backward = mode == 1;
    const float mul = mode == 2 ? 1.f : 1.f / (float)HW;         // mode 2: the plain sum over the rows (backward of broadcasting one row to HW rows)
    hipStream_t st = (hipStream_t)stream;
    MG_WITH_DTYPE_OR(dtype, -3, T,
        if (backward) {
            long b = ((long)HW * C + 255) / 256; if (b > 1024) b = 1024;
            hipLaunchKernelGGL(spatial_mean_bwd_kernel<T>, dim3((unsigned)b, N), dim3(256), 0, st, (const T*)x, HW, C, (T*)out);
        } else hipLaunchKernelGGL(spatial_mean_fwd_kernel<T>, dim3((C + 63) / 64, N), dim3(256), 0, st, (const T*)x, HW, C, ld, mul, (T*)out);
    );
    MG_CHECK_LAUNCH();
    return 0;
}
