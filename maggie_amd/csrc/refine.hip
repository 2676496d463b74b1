// Full-size mattes on the device: the fast guided filter (He & Sun) stated on bytes. A local linear model alpha ~ a . I + b is fitted at the
//   network's size, its coefficients are rounded to 16 fractional bits, averaged over the same window, brought to full size bilinearly and applied
//   to the full-size frame. DESIGN.md section 36 and the header block of include/maggie_hip.h hold the statement; tests/refine_restatement.py
//   states the same arithmetic in NumPy and is the byte-for-byte oracle.
//   mg_refine_coefficients : guide, alpha bytes -> the fp64 means (abar_0, abar_1, abar_2, bbar) at the network's size, six launches:
//     rf_rows_kernel<true>  : a workgroup owns MG_REFINE_TILE columns of one guide row. The row's bytes over the tile and its reach (reflected
//                             without repeating the edge, as often as needed) go into LDS as the nine planes G_c, G_c G_d (c <= d), formed on the
//                             load; a lane adds the r taps of its column and stores nine uint32 row sums (at most 64 x 65025 < 2^23).
//     rf_cols_kernel<0>     : a lane owns one column over a strip of MG_REFINE_STRIP rows: the r (reflected) rows of the strip's first window,
//                             then one row in, one row out. Stores the nine window sums of the frame, which its instances share.
//     rf_rows_kernel<false> : the four planes p, G_c p of one instance, as above.
//     rf_cols_kernel<1>     : the same walk over the four; at every pixel it reads the frame's nine sums, solves the 3 x 3 system by cofactors
//                             in fp64 in the stated order and stores A_0, A_1, A_2, B as int32 (|A| <= 2^24, |B| <= 2^26).
//     rf_crows_kernel, rf_ccols_kernel : the second window over the four integer planes, int64 sums (|sum| < 2^39), and the fp64 means.
//     All sums are exact integers, so the order of adding and the wrap of a running difference change nothing.
//   mg_refine_apply : the hot path, one launch at full size. A workgroup owns a run of columns of one output row, so y0, y1, fy are uniform. A
//     lane owns MG_REFINE_LANE_PIXELS = 4 consecutive pixels: it loads their 12 frame bytes once (three 4-byte loads where the address allows),
//     keeps their x0, x1, fx, and loops over the frame's instances: four planes x four taps of the means (read through the cache: a wave's 256
//     pixels touch about 256 w / W + 1 neighbouring columns of two rows, a few cache lines an instruction), the lerps in the stated order, the
//     byte, one 4-byte store (a wave stores 256 contiguous bytes). 16 pixels a lane were tried first: the 256 loads in flight took 256 VGPRs
//     at one wave a SIMD, or 121 spilled at four. I / 255.0 comes from an LDS table of the 256 quotients (the same division, made once).
// The clips of a and b are guards that never act: the model gives |a| <= 0.25 / sqrt(eps) <= 250 for eps >= 1e-6, and |b| <= 1 + 3 |a|.
// The whole file is compiled WITHOUT floating-point contraction and holds no fp32 between the sums and the bytes.
#include "common.h"
#include "../../include/maggie_hip.h"

#pragma clang fp contract(off)

namespace {
constexpr int NT = MG_REFINE_THREADS;
constexpr int TILE = MG_REFINE_TILE;
constexpr int STRIP = MG_REFINE_STRIP;
constexpr int RMAX = MG_REFINE_MAX_RADIUS;
constexpr int LP = MG_REFINE_LANE_PIXELS;
constexpr int SPAN = TILE + RMAX - 1;                      // LDS entries of a plane: the tile and its reach
constexpr long ZMAX = 65535;                               // planes of one launch (gridDim.z)
static_assert(NT == TILE && NT == 256 && LP % 4 == 0, "one lane per column of the tile and per entry of the quotient table; whole 32-bit words a lane");

// BORDER_REFLECT_101 as often as needed: period 2 (n - 1); n == 1 maps everything to 0
__device__ __forceinline__ int reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// GUIDE: plane n is frame n0 + n, nine planes. Else plane n is instance n0 + n of frame (n0 + n) / P, four planes. rows: uint32 [planes][NQ][h][w].
template <bool GUIDE>
__global__ __launch_bounds__(NT) void rf_rows_kernel(const uint8_t* __restrict__ G, const uint8_t* __restrict__ alpha, long n0, int P, int h, int w,
                                                     int r, uint32_t* __restrict__ rows) {
    constexpr int NQ = GUIDE ? 9 : 4;
    __shared__ uint32_t pr[NQ][SPAN];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * TILE, y = (int)blockIdx.y;
    const long n = blockIdx.z;
    const long npix = (long)h * w;
    const uint8_t* g = G + (GUIDE ? n0 + n : (n0 + n) / P) * npix * 3 + (long)y * w * 3;
    const uint8_t* a = GUIDE ? nullptr : alpha + (n0 + n) * npix + (long)y * w;
    const int cols = w - x0 < TILE ? w - x0 : TILE;          // columns of this tile
    const int span = cols + r - 1;                           // <= SPAN
    const int left = x0 - r / 2;
    for (int i = tid; i < span; i += NT) {
        const int x = reflect(left + i, w);
        const uint32_t g0 = g[3 * x], g1 = g[3 * x + 1], g2 = g[3 * x + 2];
        if constexpr (GUIDE) {
            pr[0][i] = g0; pr[1][i] = g1; pr[2][i] = g2;
            pr[3][i] = g0 * g0; pr[4][i] = g0 * g1; pr[5][i] = g0 * g2;
            pr[6][i] = g1 * g1; pr[7][i] = g1 * g2; pr[8][i] = g2 * g2;
        } else {
            const uint32_t pv = a[x];
            pr[0][i] = pv; pr[1][i] = g0 * pv; pr[2][i] = g1 * pv; pr[3][i] = g2 * pv;
        }
    }
    __syncthreads();
    if (tid < cols) {
        uint32_t s[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] = 0;
        for (int k = 0; k < r; ++k) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q] += pr[q][tid + k];
        }
        uint32_t* d = rows + (n * NQ * h + y) * (long)w + x0 + tid;
#pragma unroll
        for (int q = 0; q < NQ; ++q) d[(long)q * npix] = s[q];
    }
}

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int32_t fixed16(double v, double bound) { return (int32_t)floor(clipd(v, -bound, bound) * 65536.0 + 0.5); }

// step 3 of the statement: g the frame's nine window sums, s the instance's four -> A_0, A_1, A_2, B
__device__ __forceinline__ void solve(const uint32_t* g, const uint32_t* s, double d1, double d2, double eps, int32_t* o) {
    const double m0 = (double)g[0] / d1, m1 = (double)g[1] / d1, m2 = (double)g[2] / d1, mp = (double)s[0] / d1;
    double s00 = (double)g[3] / d2 - m0 * m0;
    const double s01 = (double)g[4] / d2 - m0 * m1;
    const double s02 = (double)g[5] / d2 - m0 * m2;
    double s11 = (double)g[6] / d2 - m1 * m1;
    const double s12 = (double)g[7] / d2 - m1 * m2;
    double s22 = (double)g[8] / d2 - m2 * m2;
    s00 = s00 + eps; s11 = s11 + eps; s22 = s22 + eps;
    const double k0 = (double)s[1] / d2 - m0 * mp, k1 = (double)s[2] / d2 - m1 * mp, k2 = (double)s[3] / d2 - m2 * mp;
    const double c00 = s11 * s22 - s12 * s12;
    const double c01 = s02 * s12 - s01 * s22;
    const double c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02;
    const double c12 = s01 * s02 - s00 * s12;
    const double c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    const double a0 = ((c00 * k0 + c01 * k1) + c02 * k2) / det;
    const double a1 = ((c01 * k0 + c11 * k1) + c12 * k2) / det;
    const double a2 = ((c02 * k0 + c12 * k1) + c22 * k2) / det;
    const double b = mp - ((a0 * m0 + a1 * m1) + a2 * m2);
    o[0] = fixed16(a0, 256.0); o[1] = fixed16(a1, 256.0); o[2] = fixed16(a2, 256.0); o[3] = fixed16(b, 1024.0);
}

// MODE 0: rows uint32 [planes][9][h][w] -> sums, the same shape. MODE 1: rows uint32 [planes][4][h][w] and gsums [frames][9][h][w] (plane n
// reads frame (n0 + n) / P) -> coef int32 [planes][4][h][w].
template <int MODE>
__global__ __launch_bounds__(NT) void rf_cols_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ gsums, long n0, int P, int h, int w,
                                                     int r, double eps, uint32_t* __restrict__ sums, int32_t* __restrict__ coef) {
    constexpr int NQ = MODE == 0 ? 9 : 4;
    const int x = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (x >= w) return;
    const int y0 = (int)blockIdx.y * STRIP;
    const int y1 = y0 + STRIP < h ? y0 + STRIP : h;
    const long n = blockIdx.z;
    const long npix = (long)h * w;
    const uint32_t* src = rows + n * NQ * npix + x;
    const uint32_t* gs = MODE == 0 ? nullptr : gsums + ((n0 + n) / P) * 9 * npix;
    const int top = y0 - r / 2;
    uint32_t s[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = 0;
    for (int k = 0; k < r; ++k) {
        const long o = (long)reflect(top + k, h) * w;
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] += src[(long)q * npix + o];
    }
    const double cnt = (double)(r * r);
    const double d1 = 255.0 * cnt, d2 = 65025.0 * cnt;
    for (int y = y0; y < y1; ++y) {
        const long pix = (long)y * w + x;
        if (MODE == 0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) sums[(n * NQ + q) * npix + pix] = s[q];
        } else {
            uint32_t g[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) g[q] = gs[(long)q * npix + pix];
            int32_t o[4];
            solve(g, s, d1, d2, eps, o);
#pragma unroll
            for (int q = 0; q < 4; ++q) coef[(n * 4 + q) * npix + pix] = o[q];
        }
        if (y + 1 < y1) {                                    // the window moves down a row: wrap-around differences of exact sums
            const long oin = (long)reflect(y - r / 2 + r, h) * w, oout = (long)reflect(y - r / 2, h) * w;
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q] += src[(long)q * npix + oin] - src[(long)q * npix + oout];
        }
    }
}

// the second window, rows: coef int32 [planes][4][h][w] -> crows int64, the same shape
__global__ __launch_bounds__(NT) void rf_crows_kernel(const int32_t* __restrict__ coef, int h, int w, int r, int64_t* __restrict__ crows) {
    __shared__ int32_t pr[4][SPAN];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * TILE, y = (int)blockIdx.y;
    const long n = blockIdx.z;
    const long npix = (long)h * w;
    const int32_t* c = coef + n * 4 * npix + (long)y * w;
    const int cols = w - x0 < TILE ? w - x0 : TILE;
    const int span = cols + r - 1;
    const int left = x0 - r / 2;
    for (int i = tid; i < span; i += NT) {
        const int x = reflect(left + i, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q][i] = c[(long)q * npix + x];
    }
    __syncthreads();
    if (tid < cols) {
        int64_t s[4] = {0, 0, 0, 0};
        for (int k = 0; k < r; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += pr[q][tid + k];
        }
        int64_t* d = crows + (n * 4 * h + y) * (long)w + x0 + tid;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[(long)q * npix] = s[q];
    }
}

// the second window, columns, and step 4: crows -> means fp64 [planes][4][h][w]
__global__ __launch_bounds__(NT) void rf_ccols_kernel(const int64_t* __restrict__ crows, int h, int w, int r, double* __restrict__ means) {
    const int x = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (x >= w) return;
    const int y0 = (int)blockIdx.y * STRIP;
    const int y1 = y0 + STRIP < h ? y0 + STRIP : h;
    const long n = blockIdx.z;
    const long npix = (long)h * w;
    const int64_t* src = crows + n * 4 * npix + x;
    const int top = y0 - r / 2;
    int64_t s[4] = {0, 0, 0, 0};
    for (int k = 0; k < r; ++k) {
        const long o = (long)reflect(top + k, h) * w;
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += src[(long)q * npix + o];
    }
    const double den = (double)(r * r) * 65536.0;
    for (int y = y0; y < y1; ++y) {
        const long pix = (long)y * w + x;
#pragma unroll
        for (int q = 0; q < 4; ++q) means[(n * 4 + q) * npix + pix] = (double)s[q] / den;
        if (y + 1 < y1) {
            const long oin = (long)reflect(y - r / 2 + r, h) * w, oout = (long)reflect(y - r / 2, h) * w;
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += src[(long)q * npix + oin] - src[(long)q * npix + oout];
        }
    }
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// I: uint8 [frames][H][W][3] (the launch's first frame); means fp64 [frames * P][4][h][w]; out uint8 / outf fp32 [frames * P][H][W] (either may be null)
__global__ __launch_bounds__(NT) void rf_apply_kernel(const uint8_t* __restrict__ I, const double* __restrict__ means, int P, int h, int w, int H, int W,
                                                      const int32_t* __restrict__ xi, const double* __restrict__ xf, const int32_t* __restrict__ yi,
                                                      const double* __restrict__ yf, int snap, uint8_t* __restrict__ out, float* __restrict__ outf) {
    __shared__ double unit[256];                             // v / 255.0
    __shared__ float unitf[256];                             // v / 255.0f
    unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    unitf[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.0f);
    __syncthreads();
    const int X0 = ((int)blockIdx.x * NT + (int)threadIdx.x) * LP;
    if (X0 >= W) return;
    const int y = (int)blockIdx.y;
    const long t = blockIdx.z;
    const int cnt = W - X0 < LP ? W - X0 : LP;
    const long npix = (long)h * w;
    const int y0 = clampi(yi[y], h - 1), y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const double fy = yf[y], gy = 1.0 - fy;
    union { uint32_t v[3 * LP / 4]; uint8_t b[3 * LP]; } px;
    const uint8_t* src = I + ((t * H + y) * (long)W + X0) * 3;
    if (cnt == LP && ((uintptr_t)src & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 3 * LP / 4; ++k) px.v[k] = reinterpret_cast<const uint32_t*>(src)[k];
    } else {
#pragma unroll
        for (int j = 0; j < LP; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px.b[3 * j + c] = j < cnt ? src[3 * j + c] : (uint8_t)0;
        }
    }
    uint32_t xa[LP], xb[LP];
    double fx[LP];
#pragma unroll
    for (int j = 0; j < LP; ++j) {
        const int X = j < cnt ? X0 + j : X0;                 // a lane that reaches past the row's end repeats its first pixel there and stores nothing for it
        xa[j] = (uint32_t)clampi(xi[X], w - 1);
        xb[j] = (int)xa[j] + 1 < w ? xa[j] + 1u : xa[j];
        fx[j] = xf[X];
    }
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        const long n = t * P + p;
        const double* r0 = means + n * 4 * npix + (long)y0 * w;
        const double* r1 = means + n * 4 * npix + (long)y1 * w;
        union { uint32_t v[LP / 4]; uint8_t b[LP]; } ob;
#pragma unroll
        for (int j = 0; j < LP; ++j) {
            const double gx = 1.0 - fx[j];
            double up[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* a = r0 + (long)q * npix;
                const double* b = r1 + (long)q * npix;
                const double top = a[xa[j]] * gx + a[xb[j]] * fx[j];
                const double bot = b[xa[j]] * gx + b[xb[j]] * fx[j];
                up[q] = top * gy + bot * fy;
            }
            const double v = ((up[3] + up[0] * unit[px.b[3 * j]]) + up[1] * unit[px.b[3 * j + 1]]) + up[2] * unit[px.b[3 * j + 2]];
            uint32_t k = (uint32_t)floor(clipd(v, 0.0, 1.0) * 255.0 + 0.5);
            if (snap) k = k <= 1u ? 0u : (k >= 254u ? 255u : k);
            ob.b[j] = (uint8_t)k;
        }
        const long o = (n * H + y) * (long)W + X0;
        if (out) {
            if (cnt == LP && ((uintptr_t)(out + o) & 3) == 0) {
#pragma unroll
                for (int k = 0; k < LP / 4; ++k) reinterpret_cast<uint32_t*>(out + o)[k] = ob.v[k];
            } else {
#pragma unroll
                for (int j = 0; j < LP; ++j) {
                    if (j < cnt) out[o + j] = ob.b[j];
                }
            }
        }
        if (outf) {
#pragma unroll
            for (int j = 0; j < LP; ++j) {
                if (j < cnt) outf[o + j] = unitf[ob.b[j]];
            }
        }
    }
}

int bad_side(int v) { return v < 1 || v > MG_CUTOUT_MAX_SIDE; }
}  // namespace

extern "C" int mg_refine_limits(int* threads, int* tile, int* strip, int* max_radius, int* max_side, int* lane_pixels) {
    if (!threads || !tile || !strip || !max_radius || !max_side || !lane_pixels) return -2;
    *threads = NT; *tile = TILE; *strip = STRIP; *max_radius = RMAX; *max_side = MG_CUTOUT_MAX_SIDE; *lane_pixels = LP;
    return 0;
}

extern "C" int mg_refine_coefficients(const uint8_t* guide_u8, const uint8_t* alpha_u8, long frames, int P, int h, int w, int r, double eps,
                                      uint32_t* grows, uint32_t* gsums, uint32_t* prows, int32_t* coef, int64_t* crows, double* means, void* stream) {
    if (!guide_u8 || !alpha_u8 || !grows || !gsums || !prows || !coef || !crows || !means || frames < 0 || P < 0) return -2;
    if (bad_side(h) || bad_side(w) || r < 1 || r > RMAX || !(eps >= MG_REFINE_MIN_EPS && eps <= 1.0)) return -2;
    if (((uintptr_t)grows & 3) || ((uintptr_t)gsums & 3) || ((uintptr_t)prows & 3) || ((uintptr_t)coef & 3) || ((uintptr_t)crows & 7) ||
        ((uintptr_t)means & 7))
        return -2;
    const long planes = frames * P;
    if (planes == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)h * w;
    const unsigned gx_r = (unsigned)((w + TILE - 1) / TILE), gx_c = (unsigned)((w + NT - 1) / NT), gy_c = (unsigned)((h + STRIP - 1) / STRIP);
    for (long n0 = 0; n0 < frames; n0 += ZMAX) {
        const unsigned nz = (unsigned)(frames - n0 < ZMAX ? frames - n0 : ZMAX);
        hipLaunchKernelGGL(rf_rows_kernel<true>, dim3(gx_r, (unsigned)h, nz), dim3(NT), 0, st, guide_u8, (const uint8_t*)nullptr, n0, 1, h, w, r,
                           grows + n0 * 9 * npix);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(rf_cols_kernel<0>, dim3(gx_c, gy_c, nz), dim3(NT), 0, st, (const uint32_t*)(grows + n0 * 9 * npix), (const uint32_t*)nullptr,
                           n0, 1, h, w, r, eps, gsums + n0 * 9 * npix, (int32_t*)nullptr);
        MG_CHECK_LAUNCH();
    }
    for (long n0 = 0; n0 < planes; n0 += ZMAX) {
        const unsigned nz = (unsigned)(planes - n0 < ZMAX ? planes - n0 : ZMAX);
        const long off = n0 * 4 * npix;
        hipLaunchKernelGGL(rf_rows_kernel<false>, dim3(gx_r, (unsigned)h, nz), dim3(NT), 0, st, guide_u8, alpha_u8, n0, P, h, w, r, prows + off);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(rf_cols_kernel<1>, dim3(gx_c, gy_c, nz), dim3(NT), 0, st, (const uint32_t*)(prows + off), (const uint32_t*)gsums, n0, P, h, w,
                           r, eps, (uint32_t*)nullptr, coef + off);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(rf_crows_kernel, dim3(gx_r, (unsigned)h, nz), dim3(NT), 0, st, (const int32_t*)(coef + off), h, w, r, crows + off);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(rf_ccols_kernel, dim3(gx_c, gy_c, nz), dim3(NT), 0, st, (const int64_t*)(crows + off), h, w, r, means + off);
        MG_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int mg_refine_apply(const uint8_t* frames_u8, const double* means, long frames, int P, int h, int w, int H, int W, const int32_t* xi,
                               const double* xf, const int32_t* yi, const double* yf, int snap, uint8_t* out, float* outf, void* stream) {
    if (!frames_u8 || !means || !xi || !xf || !yi || !yf || (!out && !outf) || frames < 0 || P < 0) return -2;
    if (bad_side(h) || bad_side(w) || bad_side(H) || bad_side(W)) return -2;
    if (((uintptr_t)means & 7) || ((uintptr_t)xi & 3) || ((uintptr_t)xf & 7) || ((uintptr_t)yi & 3) || ((uintptr_t)yf & 7) || ((uintptr_t)outf & 3))
        return -2;
    if (frames * P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)h * w, NPIX = (long)H * W;
    const unsigned gx = (unsigned)((W + NT * LP - 1) / (NT * LP));
    for (long t0 = 0; t0 < frames; t0 += ZMAX) {
        const unsigned nz = (unsigned)(frames - t0 < ZMAX ? frames - t0 : ZMAX);
        hipLaunchKernelGGL(rf_apply_kernel, dim3(gx, (unsigned)H, nz), dim3(NT), 0, st, frames_u8 + t0 * NPIX * 3, means + t0 * P * 4 * npix, P, h, w, H, W,
                           xi, xf, yi, yf, snap, out ? out + t0 * P * NPIX : (uint8_t*)nullptr, outf ? outf + t0 * P * NPIX : (float*)nullptr);
        MG_CHECK_LAUNCH();
    }
    return 0;
}
