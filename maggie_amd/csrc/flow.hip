// Dense Farneback optical flow for batched uint8 planes and the MESSDdt metric of maggie/utils/metric.py:450-531 on the device (DESIGN.md
// section 23). The reference copies every prediction, ground truth and trimap to the host, runs cv2.calcOpticalFlowFarneback in a process pool
// and warps in torch on the CPU; here the planes stay in HBM and two doubles per instance come back.
//
// The flow is Farneback 2003 as OpenCV structures it, at the reference's parameters only (pyr_scale 0.5, levels 5, winsize 10, iterations 2,
// poly_n 7, poly_sigma 1.5, Gaussian window, no initial flow), fp32 throughout. tests/flow_restatement.py states it in NumPy. Per pyramid
// level, coarse to fine, six launches that each serve all P plane pairs (blockIdx.z):
//   level_rows_kernel   uint8 -> fp32, the smooth_sz-tap Gaussian along x at the two columns each output column's resize taps land on
//   level_cols_kernel   the same along y: the level image of both frames (the blur is never computed where the resize does not look)
//   polyexp_kernel      polynomial expansion of both frames (5 planar fp32 planes each)
//   matrices_kernel     flow from the coarser level (bilinear, x 2) or zero, and the five planes G11 G12 G22 h1 h2
//   update_kernel x 2   11-tap Gaussian of the five planes, the 2x2 solve, and (first pass) the next matrices
// Every stencil stages its tile plus halo in LDS; the matrices are point-wise gathers at data-dependent positions and read HBM (L2).
// Nothing is summed across workgroups, so a plane's result does not depend on what else is in the batch.
#include <math.h>
#include "common.h"
#include "launch.h"
#include "../../include/maggie_hip.h"

namespace {

constexpr int MAX_SMOOTH = 79;                     // taps of the level blur at scale 1/32
constexpr int POLY_N = 7, POLY_TAPS = 2 * POLY_N + 1;
constexpr int WIN_R = 5, WIN_TAPS = 2 * WIN_R + 1;
constexpr int LC = 64, LR = 4;                     // level kernels: 64 output columns x 4 output rows per workgroup
constexpr int TW = 32, TH = 16;                    // polyexp / update: 32 x 16 outputs per workgroup of 256 threads, two rows per thread

struct SmoothTaps { float g[MAX_SMOOTH]; };
struct PolyTaps { float g[POLY_TAPS], xg[POLY_TAPS], xxg[POLY_TAPS]; float ig11, ig03, ig33, ig55; };
struct WinTaps { float g[WIN_TAPS]; };

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}
__device__ __forceinline__ int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

// Bilinear resize tap of output index o: pixel centre (o + 1/2) s - 1/2 computed in fp64 and rounded to fp32, taps clamped, weight 0 where the left
// tap is clamped. No contraction: the position is the rounded product, as the restatement has it.
__device__ __forceinline__ void resize_tap(int o, double s, int n_src, int& i0, int& i1, float& w) {
#pragma clang fp contract(off)
    const double c = ((double)o + 0.5) * s;
    const float f = (float)(c - 0.5);
    const float fl = floorf(f);
    i0 = (int)fl;
    w = f - fl;
    if (i0 < 0) { i0 = 0; w = 0.f; }
    if (i0 >= n_src - 1) { i0 = n_src - 1; w = 0.f; }
    i1 = i0 + 1 < n_src ? i0 + 1 : n_src - 1;
}
// the left tap of output o and the right tap of output o: the ends of the source span a workgroup stages
__device__ __forceinline__ int resize_first(int o, double s, int n_src) { int i0, i1; float w; resize_tap(o, s, n_src, i0, i1, w); return i0; }
__device__ __forceinline__ int resize_last(int o, double s, int n_src) { int i0, i1; float w; resize_tap(o, s, n_src, i0, i1, w); return i1; }

// LDS position of element j of a staged source row: one dword of padding every 32. Neighbouring lanes read source columns 2^k apart (the level's
// scale), which unpadded is a 2^k-way bank conflict on every tap; padded, the 32 lanes of a half fall on 32 banks for every k. The tap reads are
// single dwords (ds_read_b32: bank = dword address mod 32, lanes conflict within a 32-lane half); wider reads bank mod 64 and would need another pad.
__device__ __forceinline__ int lds_pad(int j) { return j + (j >> 5); }

// ---- level image, x pass: tmp[z][y][ox] for every source row y ------------------------------------------------------------------------------------
// (NTAPS is a template argument of the two level kernels: the tap loops unroll and the taps sit in scalar registers; indexed at run time, every tap
// would be a scalar load from the kernel arguments with its own wait)
template <int NTAPS>
__global__ __launch_bounds__(LC * LR) void level_rows_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ next, int P, int H, int W, int wl,
                                                             double sx, int span, int pitch, SmoothTaps tp, float* __restrict__ tmp) {
    extern __shared__ float lds[];                                      // [LR][pitch], element j of a row at lds_pad(j)
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const uint8_t* src = (z < P ? prev + (long)z * H * W : next + (long)(z - P) * H * W);
    constexpr int r = NTAPS >> 1;
    const int ox0 = blockIdx.x * LC, oxl = min(ox0 + LC, wl) - 1, y = blockIdx.y * LR + ty;
    const int xlo = resize_first(ox0, sx, W) - r, n = min(resize_last(oxl, sx, W) + r - xlo + 1, span);
    if (y < H) {
        const uint8_t* row = src + (long)y * W;
#pragma unroll 8
        for (int i = tx; i < n; i += LC) lds[ty * pitch + lds_pad(i)] = (float)row[reflect101(xlo + i, W)];      // (unrolled: eight loads in flight, the loop is latency-bound otherwise)
    }
    __syncthreads();
    const int ox = ox0 + tx;
    if (y >= H || ox >= wl) return;
    int x0, x1;
    float wx;
    resize_tap(ox, sx, W, x0, x1, wx);
    const float* lrow = lds + ty * pitch;
    const int j0 = x0 - r - xlo;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NTAPS; ++i) a += tp.g[i] * lrow[lds_pad(j0 + i)];
    float v = a;
    if (wx != 0.f) {
        const int j1 = x1 - r - xlo;
        float b = 0.f;
#pragma unroll
        for (int i = 0; i < NTAPS; ++i) b += tp.g[i] * lrow[lds_pad(j1 + i)];
        v = a * (1.f - wx) + b * wx;
    }
    tmp[((long)z * H + y) * wl + ox] = v;
}

// ---- level image, y pass: img[z][oy][ox] ------------------------------------------------------------------------------------------------------------
template <int NTAPS>
__global__ __launch_bounds__(LC * LR) void level_cols_kernel(const float* __restrict__ tmp, int H, int hl, int wl, double sy, int span, SmoothTaps tp,
                                                             float* __restrict__ img) {
    extern __shared__ float lds[];                                      // [span][LC]
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    constexpr int r = NTAPS >> 1;
    const int oy0 = blockIdx.y * LR, oyl = min(oy0 + LR, hl) - 1, ox = blockIdx.x * LC + tx;
    const int ylo = resize_first(oy0, sy, H) - r, n = min(resize_last(oyl, sy, H) + r - ylo + 1, span);
    const float* src = tmp + (long)z * H * wl;
    if (ox < wl)
#pragma unroll 8
        for (int i = ty; i < n; i += LR) lds[i * LC + tx] = src[(long)reflect101(ylo + i, H) * wl + ox];
    __syncthreads();
    const int oy = oy0 + ty;
    if (oy >= hl || ox >= wl) return;
    int y0, y1;
    float wy;
    resize_tap(oy, sy, H, y0, y1, wy);
    const float* l0 = lds + (y0 - r - ylo) * LC + tx;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NTAPS; ++i) a += tp.g[i] * l0[i * LC];
    float v = a;
    if (wy != 0.f) {
        const float* l1 = lds + (y1 - r - ylo) * LC + tx;
        float b = 0.f;
#pragma unroll
        for (int i = 0; i < NTAPS; ++i) b += tp.g[i] * l1[i * LC];
        v = a * (1.f - wy) + b * wy;
    }
    img[((long)z * hl + oy) * wl + ox] = v;
}

// ---- polynomial expansion: R[z][5][h][w] = b_x, b_y, A_xx, A_yy, A_xy; columns first, then rows; replicate border -------------------------------------
constexpr int PIW = TW + 2 * POLY_N, PIH = TH + 2 * POLY_N;             // 46 x 30 staged pixels

__global__ __launch_bounds__(256) void polyexp_kernel(const float* __restrict__ img, int h, int w, PolyTaps tp, float* __restrict__ R) {
    __shared__ float in[PIH][PIW];
    __shared__ float v[3][TH][PIW];
    const int z = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, tid = threadIdx.x;
    const float* src = img + (long)z * h * w;
#pragma unroll
    for (int i = tid; i < PIH * PIW; i += 256) {
        const int ly = i / PIW, lx = i - ly * PIW;
        in[ly][lx] = src[(long)clampi(y0 + ly - POLY_N, 0, h - 1) * w + clampi(x0 + lx - POLY_N, 0, w - 1)];
    }
    __syncthreads();
    for (int i = tid; i < TH * PIW; i += 256) {
        const int ly = i / PIW, lx = i - ly * PIW;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < POLY_TAPS; ++k) {
            const float p = in[ly + k][lx];
            s0 += tp.g[k] * p; s1 += tp.xg[k] * p; s2 += tp.xxg[k] * p;
        }
        v[0][ly][lx] = s0; v[1][ly][lx] = s1; v[2][ly][lx] = s2;
    }
    __syncthreads();
    const int lx = tid & (TW - 1), x = x0 + lx;
    if (x >= w) return;
    const long plane = (long)h * w;
    float* dst = R + (long)z * 5 * plane;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = (tid >> 5) + half * 8, y = y0 + ly;
        if (y >= h) continue;
        float s = 0.f, bx = 0.f, by = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < POLY_TAPS; ++k) {
            const float a = v[0][ly][lx + k], b = v[1][ly][lx + k], c = v[2][ly][lx + k];
            s += tp.g[k] * a; bx += tp.xg[k] * a; xx += tp.xxg[k] * a;
            by += tp.g[k] * b; xy += tp.xg[k] * b;
            yy += tp.g[k] * c;
        }
        const long o = (long)y * w + x;
        dst[o] = tp.ig11 * bx;
        dst[plane + o] = tp.ig11 * by;
        dst[2 * plane + o] = tp.ig03 * s + tp.ig33 * xx;
        dst[3 * plane + o] = tp.ig03 * s + tp.ig33 * yy;
        dst[4 * plane + o] = tp.ig55 * xy;
    }
}

// ---- the matrices at one pixel -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float border_w(int i, int n) {
    const float b[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    float s = 1.f;
    if (i < 5) s *= b[i];
    if (n - 1 - i < 5) s *= b[n - 1 - i];
    return s;
}

__device__ __forceinline__ void matrices_at(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int x, int y, float dx, float dy,
                                            float* __restrict__ M) {
    const long plane = (long)h * w, o = (long)y * w + x;
    float fx = (float)x + dx, fy = (float)y + dy;
    const float flx = floorf(fx), fly = floorf(fy);
    fx -= flx; fy -= fly;
    float bx = 0.f, by = 0.f, axx = R0[2 * plane + o], ayy = R0[3 * plane + o], axy = R0[4 * plane + o];
    // the comparison in fp32 first: a flow that is huge or NaN never reaches the integer conversion
    if (flx >= 0.f && flx < (float)(w - 1) && fly >= 0.f && fly < (float)(h - 1)) {
        const int x1 = (int)flx, y1 = (int)fly;
        const long q = (long)y1 * w + x1;
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        float s[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float* p = R1 + c * plane + q;
            s[c] = a00 * p[0] + a01 * p[1] + a10 * p[w] + a11 * p[w + 1];
        }
        bx = (R0[o] - s[0]) * 0.5f;
        by = (R0[plane + o] - s[1]) * 0.5f;
        axx = (axx + s[2]) * 0.5f;
        ayy = (ayy + s[3]) * 0.5f;
        axy = (axy + s[4]) * 0.25f;
    } else {
        axy *= 0.5f;
    }
    const float sc = border_w(y, h) * border_w(x, w);
    bx *= sc; by *= sc; axx *= sc; ayy *= sc; axy *= sc;
    bx += axx * dx + axy * dy;
    by += axy * dx + ayy * dy;
    M[o] = axx * axx + axy * axy;
    M[plane + o] = (axx + ayy) * axy;
    M[2 * plane + o] = ayy * ayy + axy * axy;
    M[3 * plane + o] = axx * bx + axy * by;
    M[4 * plane + o] = axy * bx + ayy * by;
}

// flow of this level from the coarser one (bilinear, columns first, x 2; zero at the coarsest), and the first matrices
__global__ __launch_bounds__(256) void matrices_kernel(const float* __restrict__ R, int P, int h, int w, const float* __restrict__ coarse, int hc, int wc,
                                                       double sx, double sy, float* __restrict__ flow, float* __restrict__ M) {
    const int z = blockIdx.z, x = blockIdx.x * TW + (threadIdx.x & (TW - 1)), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    const long plane = (long)h * w;
    float dx = 0.f, dy = 0.f;
    if (coarse) {
        int x0, x1, y0, y1;
        float wx, wy;
        resize_tap(x, sx, wc, x0, x1, wx);
        resize_tap(y, sy, hc, y0, y1, wy);
        const float2* c = (const float2*)coarse + (long)z * hc * wc;
        const float2 p00 = c[(long)y0 * wc + x0], p01 = c[(long)y0 * wc + x1], p10 = c[(long)y1 * wc + x0], p11 = c[(long)y1 * wc + x1];
        const float tx0 = p00.x * (1.f - wx) + p01.x * wx, tx1 = p10.x * (1.f - wx) + p11.x * wx;
        const float ty0 = p00.y * (1.f - wx) + p01.y * wx, ty1 = p10.y * (1.f - wx) + p11.y * wx;
        dx = (tx0 * (1.f - wy) + tx1 * wy) * 2.f;
        dy = (ty0 * (1.f - wy) + ty1 * wy) * 2.f;
    }
    ((float2*)flow)[(long)z * plane + (long)y * w + x] = make_float2(dx, dy);
    matrices_at(R + (long)z * 5 * plane, R + (long)(P + z) * 5 * plane, h, w, x, y, dx, dy, M + (long)z * 5 * plane);
}

// ---- flow update: 11-tap Gaussian of the five planes (columns first, replicate border), the solve, and the next matrices ---------------------------------
constexpr int UIW = TW + 2 * WIN_R, UIH = TH + 2 * WIN_R;               // 42 x 26

__global__ __launch_bounds__(256) void update_kernel(const float* __restrict__ Min, const float* __restrict__ R, int P, int h, int w, WinTaps tp,
                                                     float* __restrict__ flow, float* __restrict__ Mout) {
    __shared__ float in[5][UIH][UIW];
    __shared__ float v[5][TH][UIW];
    const int z = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, tid = threadIdx.x;
    const long plane = (long)h * w;
    const float* src = Min + (long)z * 5 * plane;
#pragma unroll
    for (int i = tid; i < UIH * UIW; i += 256) {
        const int ly = i / UIW, lx = i - ly * UIW;
        const long o = (long)clampi(y0 + ly - WIN_R, 0, h - 1) * w + clampi(x0 + lx - WIN_R, 0, w - 1);
#pragma unroll
        for (int c = 0; c < 5; ++c) in[c][ly][lx] = src[c * plane + o];
    }
    __syncthreads();
    for (int i = tid; i < TH * UIW; i += 256) {
        const int ly = i / UIW, lx = i - ly * UIW;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < WIN_TAPS; ++k) s += tp.g[k] * in[c][ly + k][lx];
            v[c][ly][lx] = s;
        }
    }
    __syncthreads();
    const int lx = tid & (TW - 1), x = x0 + lx;
    if (x >= w) return;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = (tid >> 5) + half * 8, y = y0 + ly;
        if (y >= h) continue;
        float b[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < WIN_TAPS; ++k) s += tp.g[k] * v[c][ly][lx + k];
            b[c] = s;
        }
        const float idet = 1.f / (b[0] * b[2] - b[1] * b[1] + 1e-3f);
        const float dx = (b[2] * b[3] - b[1] * b[4]) * idet, dy = (b[0] * b[4] - b[1] * b[3]) * idet;
        ((float2*)flow)[(long)z * plane + (long)y * w + x] = make_float2(dx, dy);
        if (Mout) matrices_at(R + (long)z * 5 * plane, R + (long)(P + z) * 5 * plane, h, w, x, y, dx, dy, Mout + (long)z * 5 * plane);
    }
}

// ---- MESSDdt ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int NT = 256, MAX_BLK = 64;

// (uint8)(gt * 255.0f): one fp32 multiply, truncated (metric.py:465, :453)
__global__ __launch_bounds__(NT) void gt_u8_kernel(const float* __restrict__ gt, long n, uint8_t* __restrict__ out) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const float v = gt[i] * 255.0f;
        out[i] = (uint8_t)(v >= 255.f ? 255 : (v > 0.f ? (int)v : 0));
    }
}

// part[q][blk] = { sum |error_map|, sum m_t } of pair q = t * N + n over the pixels of this workgroup. The warped sample is read as metric.py:481-492
// reads it: pixel (row i, column j) at row clamp(j + fx, 0, H-1), column clamp(i + fy, 0, W-1) of FRAME 1 of the instance, for every t.
__global__ __launch_bounds__(NT) void messddt_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ tri,
                                                             const float* __restrict__ flow, int N, int H, int W, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sh[NT / 64][2];
    const int q = blockIdx.y, n = q % N;
    const long HW = (long)H * W, cur = (long)q * HW, one = ((long)N + n) * HW;
    const float2* fl = (const float2*)flow + cur;
    double err = 0.0, num = 0.0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        const int row = (int)(i / W), col = (int)(i - (long)row * W);
        const float2 f = fl[i];
        const float fx = fminf(fmaxf(rintf(f.x), -1e9f), 1e9f), fy = fminf(fmaxf(rintf(f.y), -1e9f), 1e9f);      // (NaN -> -1e9: clamped below)
        long r = (long)col + (long)fx, c = (long)row + (long)fy;
        r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        const long s = one + r * W + c;
        const float m0 = tri ? (tri[cur + i] == 1.f ? 1.f : 0.f) : 1.f, m1 = tri ? (tri[s] == 1.f ? 1.f : 0.f) : 1.f;
        const float d0 = pred[cur + i] - gt[cur + i], d1 = pred[s] - gt[s];
        const float e = d0 * d0 * m0 - d1 * d1 * m1;
        err += (double)fabsf(e);
        num += (double)m0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { err += __shfl_down(err, off, 64); num += __shfl_down(num, off, 64); }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = err; sh[threadIdx.x >> 6][1] = num; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = 0.0, m = 0.0;
        for (int k = 0; k < NT / 64; ++k) { e += sh[k][0]; m += sh[k][1]; }
        double* dst = part + ((long)q * gridDim.x + blockIdx.x) * 2;
        dst[0] = e; dst[1] = m;
    }
}

// out[n] = { sum_t err_t, sum_t (sum m_t + 1) }: one wave per instance, lane b holds workgroup b's partial (nblk <= 64), a fixed shuffle tree per pair,
// the pairs added in order
__global__ __launch_bounds__(64) void messddt_final_kernel(const double* __restrict__ part, int pairs_t, int N, int nblk, double* __restrict__ out) {
    const int n = blockIdx.x, b = threadIdx.x;
    double e = 0.0, m = 0.0;
    for (int t = 0; t < pairs_t; ++t) {
        const double* p = part + ((long)(t * N + n) * nblk + b) * 2;
        double pe = b < nblk ? p[0] : 0.0, pm = b < nblk ? p[1] : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { pe += __shfl_down(pe, off, 64); pm += __shfl_down(pm, off, 64); }
        e += pe; m += pm + 1.0;
    }
    if (b == 0) { out[2 * n] = e; out[2 * n + 1] = m; }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
inline int levels_of(int h, int w) {
    double scale = 1.0;
    int k = 0;
    for (; k < 5; ++k) {
        scale *= 0.5;
        if (w * scale < 32 || h * scale < 32) break;
    }
    return k;
}
inline int level_side(int n, int k) { return (int)nearbyint(n * ldexp(1.0, -k)); }      // half to even

inline void gauss_taps(int n, double sigma, float* out) {
    double g[MAX_SMOOTH], sum = 0.0;
    if (sigma <= 0.0) { out[0] = 0.25f; out[1] = 0.5f; out[2] = 0.25f; return; }
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; g[i] = exp(-x * x / (2.0 * sigma * sigma)); sum += g[i]; }
    for (int i = 0; i < n; ++i) out[i] = (float)(g[i] / sum);
}

inline bool poly_taps(PolyTaps& tp) {
    double g[POLY_TAPS], sum = 0.0;
    for (int i = 0; i < POLY_TAPS; ++i) { const double x = i - POLY_N; g[i] = exp(-x * x / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < POLY_TAPS; ++i) {
        const double x = i - POLY_N;
        g[i] /= sum;
        tp.g[i] = (float)g[i]; tp.xg[i] = (float)(x * g[i]); tp.xxg[i] = (float)(x * x * g[i]);
    }
    // Gram matrix of (1, x, y, x^2, y^2, xy) under g (x) g, inverted in fp64 (Gauss-Jordan with partial pivoting)
    double G[6][12] = {};
    for (int iy = 0; iy < POLY_TAPS; ++iy)
        for (int ix = 0; ix < POLY_TAPS; ++ix) {
            const double x = ix - POLY_N, y = iy - POLY_N, wgt = g[ix] * g[iy], b[6] = {1.0, x, y, x * x, y * y, x * y};
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) G[i][j] += wgt * b[i] * b[j];
        }
    for (int i = 0; i < 6; ++i) G[i][6 + i] = 1.0;
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(G[r][c]) > fabs(G[piv][c])) piv = r;
        if (G[piv][c] == 0.0) return false;
        for (int j = 0; j < 12; ++j) { const double t = G[c][j]; G[c][j] = G[piv][j]; G[piv][j] = t; }
        const double d = G[c][c];
        for (int j = 0; j < 12; ++j) G[c][j] /= d;
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = G[r][c];
            for (int j = 0; j < 12; ++j) G[r][j] -= f * G[c][j];
        }
    }
    tp.ig11 = (float)G[1][6 + 1]; tp.ig03 = (float)G[0][6 + 3]; tp.ig33 = (float)G[3][6 + 3]; tp.ig55 = (float)G[5][6 + 5];
    return true;
}

inline long align256(long b) { return (b + 255) & ~255L; }
constexpr long FLOW_FLOATS_PER_PIXEL = 26;          // tmp 2, img 2, R 10, M 5 + 5, the coarser level's flow 2

// staged source pixels of a level kernel: the taps of 63 (3) further outputs, the right tap, the halo on both sides, and one to spare
inline int level_span(int outs, double s, int r) { return (int)ceil((outs - 1) * s) + 2 * r + 4; }

int farneback(const uint8_t* prev, const uint8_t* next, int P, int H, int W, float* ws, float* out, hipStream_t st) {
    const long N = (long)P * H * W;
    float* tmp = ws;
    float* img = tmp + 2 * N;
    float* R = img + 2 * N;
    float* M0 = R + 10 * N;
    float* M1 = M0 + 5 * N;
    float* other = M1 + 5 * N;
    PolyTaps pt;
    if (!poly_taps(pt)) return -2;
    WinTaps wt;
    gauss_taps(WIN_TAPS, 0.3 * WIN_R, wt.g);
    const int levels = levels_of(H, W);
    const float* coarse = nullptr;
    int hc = 0, wc = 0;
    for (int k = levels; k >= 0; --k) {
        const int hl = level_side(H, k), wl = level_side(W, k);
        if (hl < 1 || wl < 1) return -2;
        const double sigma = (ldexp(1.0, k) - 1.0) * 0.5;
        SmoothTaps tp = {};
        const int n5 = (int)nearbyint(5.0 * sigma) | 1, ntaps = n5 > 3 ? n5 : 3;
        if (ntaps > MAX_SMOOTH) return -2;
        gauss_taps(ntaps, sigma, tp.g);
        const double sx = (double)W / wl, sy = (double)H / hl;
        const int span_x = level_span(LC, sx, ntaps >> 1), span_y = level_span(LR, sy, ntaps >> 1);
        const dim3 lb(LC, LR), gx((wl + LC - 1) / LC, (H + LR - 1) / LR, 2 * P), gy((wl + LC - 1) / LC, (hl + LR - 1) / LR, 2 * P);
        const int pitch_x = span_x + (span_x >> 5) + 1;
        const size_t lds_x = (size_t)LR * pitch_x * sizeof(float), lds_y = (size_t)span_y * LC * sizeof(float);
#define MG_LEVEL_TAPS(NTP)                                                                                                                  \
    case NTP:                                                                                                                               \
        MG_LAUNCH_LDS(level_rows_kernel<NTP>, gx, lb, lds_x, st, prev, next, P, H, W, wl, sx, span_x, pitch_x, tp, tmp);                         \
        MG_LAUNCH_LDS(level_cols_kernel<NTP>, gy, lb, lds_y, st, (const float*)tmp, H, hl, wl, sy, span_y, tp, img);                        \
        break;
        switch (ntaps) {                                                 // smooth_sz of the levels 0 .. 5
            MG_LEVEL_TAPS(3) MG_LEVEL_TAPS(9) MG_LEVEL_TAPS(19) MG_LEVEL_TAPS(39) MG_LEVEL_TAPS(79)
            default: return -2;
        }
#undef MG_LEVEL_TAPS
        const dim3 tiles((wl + TW - 1) / TW, (hl + TH - 1) / TH, P), tiles2(tiles.x, tiles.y, 2 * P);
        hipLaunchKernelGGL(polyexp_kernel, tiles2, dim3(256), 0, st, (const float*)img, hl, wl, pt, R);
        float* cur = (k & 1) ? other : out;                             // level 0 lands in `out`
        hipLaunchKernelGGL(matrices_kernel, dim3(tiles.x, (hl + 7) / 8, P), dim3(256), 0, st, (const float*)R, P, hl, wl, coarse, hc, wc,
                           coarse ? (double)wc / wl : 1.0, coarse ? (double)hc / hl : 1.0, cur, M0);
        hipLaunchKernelGGL(update_kernel, tiles, dim3(256), 0, st, (const float*)M0, (const float*)R, P, hl, wl, wt, cur, M1);
        hipLaunchKernelGGL(update_kernel, tiles, dim3(256), 0, st, (const float*)M1, (const float*)R, P, hl, wl, wt, cur, (float*)nullptr);
        MG_CHECK_LAUNCH();
        coarse = cur; hc = hl; wc = wl;
    }
    return 0;
}

inline int check_flow_shape(long P, int H, int W) {
    if (P < 0 || H < 1 || W < 1 || H > MG_FLOW_MAX_SIDE || W > MG_FLOW_MAX_SIDE) return -2;
    if (2 * P > 65535) return -3;
    return 0;
}
inline int messddt_blocks(long HW) {
    const long b = (HW + NT * 16 - 1) / (NT * 16);
    return (int)(b < 1 ? 1 : (b > MAX_BLK ? MAX_BLK : b));
}

}  // namespace

extern "C" int mg_flow_levels(int H, int W) { return (H < 1 || W < 1) ? -2 : levels_of(H, W); }

extern "C" int mg_flow_scratch_bytes(long P, int H, int W, long* bytes) {
    if (!bytes) return -2;
    MG_RETURN_IF(check_flow_shape(P, H, W));
    *bytes = FLOW_FLOATS_PER_PIXEL * P * H * W * (long)sizeof(float);
    return 0;
}

extern "C" int mg_flow_farneback(const uint8_t* prev, const uint8_t* next, long P, int H, int W, double pyr_scale, int levels, int winsize,
                                 int iterations, int poly_n, double poly_sigma, int flags, void* scratch, float* flow, void* stream) {
    if (pyr_scale != 0.5 || levels != 5 || winsize != 10 || iterations != 2 || poly_n != 7 || poly_sigma != 1.5 || flags != MG_FLOW_GAUSSIAN) return -2;
    MG_RETURN_IF(check_flow_shape(P, H, W));
    if (P == 0) return 0;
    if (!prev || !next || !scratch || !flow) return -2;
    return farneback(prev, next, (int)P, H, W, (float*)scratch, flow, (hipStream_t)stream);
}

// scratch of mg_metric_messddt: the uint8 planes, the flows, the partial sums, the flow's own scratch
extern "C" int mg_messddt_scratch_bytes(int F, int N, int H, int W, long* bytes) {
    if (!bytes || F < 0 || N < 0) return -2;
    const long pairs = F < 2 ? 0 : (long)(F - 1) * N;
    MG_RETURN_IF(check_flow_shape(pairs, H, W));
    const long HW = (long)H * W;
    *bytes = align256((long)F * N * HW) + align256(pairs * HW * 2 * (long)sizeof(float)) + align256(pairs * MAX_BLK * 2 * (long)sizeof(double)) +
             FLOW_FLOATS_PER_PIXEL * pairs * HW * (long)sizeof(float);
    return 0;
}

extern "C" int mg_metric_messddt(const float* pred, const float* gt, const float* trimap, int F, int N, int H, int W, const float* flow_in,
                                 void* scratch, float* flow_out, double* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (F < 0 || N < 0) return -2;
    if (N == 0) return 0;
    if (!out) return -2;
    hipError_t e = mg_zero_words(out, (long)N * 4, st);
    if (e != hipSuccess) return (int)e;
    if (F < 2) return 0;
    const long pairs = (long)(F - 1) * N, HW = (long)H * W;
    MG_RETURN_IF(check_flow_shape(pairs, H, W));
    if (!pred || !gt || !scratch) return -2;
    char* ws = (char*)scratch;
    uint8_t* u8 = (uint8_t*)ws;                       ws += align256((long)F * N * HW);
    float* flow = (float*)ws;                         ws += align256(pairs * HW * 2 * (long)sizeof(float));
    double* part = (double*)ws;                       ws += align256(pairs * MAX_BLK * 2 * (long)sizeof(double));
    if (flow_out) flow = flow_out;
    if (flow_in) {
        flow = const_cast<float*>(flow_in);
    } else {
        const long n = (long)F * N * HW;
        long blocks = (n + NT * 8 - 1) / (NT * 8);
        hipLaunchKernelGGL(gt_u8_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(NT), 0, st, gt, n, u8);
        MG_RETURN_IF(farneback(u8, u8 + (long)N * HW, (int)pairs, H, W, (float*)ws, flow, st));
    }
    const int nblk = messddt_blocks(HW);
    hipLaunchKernelGGL(messddt_partial_kernel, dim3(nblk, (unsigned)pairs), dim3(NT), 0, st, pred, gt, trimap, (const float*)flow, N, H, W, part);
    hipLaunchKernelGGL(messddt_final_kernel, dim3(N), dim3(64), 0, st, (const double*)part, F - 1, N, nblk, out);
    return (int)hipGetLastError();
}
