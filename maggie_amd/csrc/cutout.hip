// Cut-outs on the device: the foreground colour of every instance (blur-fusion estimator of Forte & Pitie, ICIP 2021, applied twice) stated on
//   bytes, and the straight RGBA image made from it. DESIGN.md section 35 holds the statement, the scheme and the measurements;
//   tests/cutout_restatement.py states the same arithmetic in NumPy and is the byte-for-byte oracle.
//   mg_cutout_alpha_bytes : fp32 alpha -> the byte of pngenc's 'unit' mode.
//   mg_cutout_estimate    : frames, alpha bytes -> F (3 channels) or RGBA (4 channels, RGB 0 where A == 0), two passes of P(I, F, B, a, r).
//
// One pass is two launches over seven integer planes (a, F_c a, B_c (255 - a)):
//   ct_rows_kernel : a workgroup owns MG_CUTOUT_TILE columns of one row of one plane. The row's bytes over the tile and its reach (reflected
//                    without repeating the edge, as often as needed) go into LDS as the seven products, formed on the load; a lane then adds the
//                    r taps of its column for each of the seven and stores seven uint32 row sums. Sums of at most 255 x 65025 < 2^24.
//                    From r = 16 on the taps are added in two steps: sums of MG_CUTOUT_GROUP neighbours for every entry first (a second LDS
//                    array), then r / GROUP of those and the r % GROUP entries left: 8 + 11 + 2 LDS reads a plane instead of 90 at r = 90.
//   ct_cols_kernel : a lane owns one column over a strip of MG_CUTOUT_STRIP rows (twice as many from r = 32 on, where the strip's first window
//                    costs more than the walk). It adds the r (reflected) rows of the strip's first window, then walks down: the fp64 formula
//                    on the seven window sums, the output bytes, one row in, one row out. a / 255 and I / 255 come from an LDS table of the
//                    256 quotients (the same division, made once). The sums are exact integers below 2^32 (255^2 x 65025), so the order of
//                    adding and the wrap of the running difference change nothing.
// The whole file is compiled WITHOUT floating-point contraction: the statement rounds every fp64 operation on its own.
#include "common.h"
#include "../../include/maggie_hip.h"

#pragma clang fp contract(off)

namespace {
constexpr int NT = MG_CUTOUT_THREADS;
constexpr int TILE = MG_CUTOUT_TILE;
constexpr int STRIP = MG_CUTOUT_STRIP;
constexpr int RMAX = MG_CUTOUT_MAX_RADIUS;
constexpr int GRP = MG_CUTOUT_GROUP;
constexpr int SPAN = TILE + RMAX - 1;                      // LDS entries of a plane: the tile and its reach
static_assert(NT == TILE && NT == 256, "one lane per column of the tile and per entry of the quotient table");

// BORDER_REFLECT_101 as often as needed: period 2 (n - 1); n == 1 maps everything to 0
__device__ __forceinline__ int reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

__global__ __launch_bounds__(NT) void alpha_bytes_kernel(const float* __restrict__ a, long n, uint8_t* __restrict__ out) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const float y = a[i] * 255.0f;
        out[i] = (uint8_t)(!(y >= 0.f) ? 0 : (y >= 255.f ? 255 : (int)y));          // pe_pixel of pngenc.hip, 'unit'
    }
}

// F, B: uint8 [..][H][W][3]; plane n of the chunk reads image (i0 + n) / fdiv of each (i0 = n0, fdiv = P when both are the frames; 0 and 1 for
// the chunk's own estimates) and alpha plane n0 + n. rows: uint32 [planes][7][H][W].
__global__ __launch_bounds__(NT) void ct_rows_kernel(const uint8_t* __restrict__ F, const uint8_t* __restrict__ B, const uint8_t* __restrict__ alpha,
                                                     long n0, long i0, int fdiv, int H, int W, int r, uint32_t* __restrict__ rows) {
    __shared__ uint32_t pr[7][SPAN], gr[7][SPAN];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * TILE, y = (int)blockIdx.y;
    const long n = blockIdx.z;
    const long npix = (long)H * W;
    const long img = (i0 + n) / fdiv;
    const uint8_t* f = F + img * npix * 3 + (long)y * W * 3;
    const uint8_t* b = B + img * npix * 3 + (long)y * W * 3;
    const uint8_t* a = alpha + (n0 + n) * npix + (long)y * W;
    const bool same = F == B;
    const int cols = W - x0 < TILE ? W - x0 : TILE;          // columns of this tile
    const int span = cols + r - 1;                           // <= SPAN
    const int left = x0 - r / 2;
    for (int i = tid; i < span; i += NT) {
        const int x = reflect(left + i, W);
        const uint32_t av = a[x], na = 255u - av;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t fv = f[3 * x + c];
            const uint32_t bv = same ? fv : (uint32_t)b[3 * x + c];
            pr[1 + c][i] = fv * av;
            pr[4 + c][i] = bv * na;
        }
        pr[0][i] = av;
    }
    __syncthreads();
    const int ng = r >= 2 * GRP ? r / GRP : 0;                // groups of GRP taps added from gr; the other taps from pr
    if (ng) {
        for (int i = tid; i + GRP <= span; i += NT) {
            uint32_t g[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
#pragma unroll
                for (int q = 0; q < 7; ++q) g[q] += pr[q][i + j];
            }
#pragma unroll
            for (int q = 0; q < 7; ++q) gr[q][i] = g[q];
        }
        __syncthreads();
    }
    if (tid < cols) {
        uint32_t s[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int m = 0; m < ng; ++m) {                       // tid + (m + 1) GRP <= cols - 1 + r: inside the span
#pragma unroll
            for (int q = 0; q < 7; ++q) s[q] += gr[q][tid + m * GRP];
        }
        for (int k = ng * GRP; k < r; ++k) {
#pragma unroll
            for (int q = 0; q < 7; ++q) s[q] += pr[q][tid + k];
        }
        uint32_t* d = rows + (n * 7 * H + y) * (long)W + x0 + tid;
#pragma unroll
        for (int q = 0; q < 7; ++q) d[(long)q * npix] = s[q];
    }
}

__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }
__device__ __forceinline__ uint32_t to_byte(double v) { return (uint32_t)floor(clip01(v) * 255.0 + 0.5); }

// MODE 0: outF, outB uint8 [planes][H][W][3]; 1: outF only; 2: outF uint8 [planes][H][W][4] = (F or 0 where a == 0, a)
template <int MODE>
__global__ __launch_bounds__(NT) void ct_cols_kernel(const uint32_t* __restrict__ rows, const uint8_t* __restrict__ I, const uint8_t* __restrict__ alpha,
                                                     long n0, int P, int H, int W, int r, int strip, uint8_t* __restrict__ outF, uint8_t* __restrict__ outB) {
    __shared__ double unit[256];                             // v / 255.0
    unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const int x = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (x >= W) return;
    const int y0 = (int)blockIdx.y * strip;
    const int y1 = y0 + strip < H ? y0 + strip : H;
    const long n = blockIdx.z;
    const long npix = (long)H * W;
    const uint32_t* src = rows + n * 7 * npix + x;
    const uint8_t* im = I + ((n0 + n) / P) * npix * 3;
    const uint8_t* a = alpha + (n0 + n) * npix;
    const int top = y0 - r / 2;
    uint32_t s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < r; ++k) {
        const long o = (long)reflect(top + k, H) * W;
#pragma unroll
        for (int q = 0; q < 7; ++q) s[q] += src[(long)q * npix + o];
    }
    const double cnt = (double)(r * r);
    const double da = 255.0 * cnt, dc = 65025.0 * cnt;
    for (int y = y0; y < y1; ++y) {
        const long pix = (long)y * W + x;
        const uint32_t av = a[pix];
        const double ba = (double)s[0] / da;
        const double dF = ba + 1e-5, dB = (1.0 - ba) + 1e-5;
        const double al = unit[av];
        uint32_t fo[3], bo[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double bF = ((double)s[1 + c] / dc) / dF;
            const double bB = ((double)s[4 + c] / dc) / dB;
            const double i = unit[im[pix * 3 + c]];
            const double fv = bF + al * ((i - al * bF) - (1.0 - al) * bB);
            fo[c] = to_byte(fv);
            bo[c] = to_byte(bB);
        }
        const long op = (n * npix + pix);
        if (MODE == 2) {
            const uint32_t rgb = av ? (fo[0] | fo[1] << 8 | fo[2] << 16) : 0u;
            reinterpret_cast<uint32_t*>(outF)[op] = rgb | av << 24;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) outF[op * 3 + c] = (uint8_t)fo[c];
            if (MODE == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) outB[op * 3 + c] = (uint8_t)bo[c];
            }
        }
        if (y + 1 < y1) {                                    // the window moves down a row: wrap-around differences of exact sums
            const long oin = (long)reflect(y - r / 2 + r, H) * W, oout = (long)reflect(y - r / 2, H) * W;
#pragma unroll
            for (int q = 0; q < 7; ++q) s[q] += src[(long)q * npix + oin] - src[(long)q * npix + oout];
        }
    }
}

int bad_radius(int r) { return r < 1 || r > RMAX; }
int strip_of(int r) { return r >= 32 ? 2 * STRIP : STRIP; }
}  // namespace

extern "C" int mg_cutout_limits(int* threads, int* tile, int* strip, int* max_radius, int* max_side) {
    if (!threads || !tile || !strip || !max_radius || !max_side) return -2;
    *threads = NT; *tile = TILE; *strip = STRIP; *max_radius = RMAX; *max_side = MG_CUTOUT_MAX_SIDE;
    return 0;
}

extern "C" int mg_cutout_alpha_bytes(const float* alpha, long n, uint8_t* out, void* stream) {
    if (!alpha || !out || n < 0 || ((uintptr_t)alpha & 3)) return -2;
    if (n == 0) return 0;
    long blocks = (n + NT - 1) / NT;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(alpha_bytes_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, alpha, n, out);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_cutout_estimate(const uint8_t* frames_u8, const uint8_t* alpha_u8, long frames, int P, int H, int W, int r0, int r1,
                                  uint32_t* rows, uint8_t* f1, uint8_t* b1, long chunk, uint8_t* out, int out_channels, void* stream) {
    if (!frames_u8 || !alpha_u8 || !rows || !f1 || !b1 || !out || frames < 0 || P < 0 || chunk < 1) return -2;
    if (H < 1 || W < 1 || H > MG_CUTOUT_MAX_SIDE || W > MG_CUTOUT_MAX_SIDE || bad_radius(r0) || bad_radius(r1)) return -2;
    if ((out_channels != 3 && out_channels != 4) || ((uintptr_t)rows & 3) || (out_channels == 4 && ((uintptr_t)out & 3))) return -2;
    const long planes = frames * P;
    if (planes == 0) return 0;
    if (chunk > 65535) chunk = 65535;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)H * W;
    const int s0 = strip_of(r0), s1 = strip_of(r1);
    const dim3 grid_r((unsigned)((W + TILE - 1) / TILE), (unsigned)H, 1);
    for (long n0 = 0; n0 < planes; n0 += chunk) {
        const unsigned nz = (unsigned)(planes - n0 < chunk ? planes - n0 : chunk);
        dim3 gr = grid_r;
        gr.z = nz;
        const dim3 gc0((unsigned)((W + NT - 1) / NT), (unsigned)((H + s0 - 1) / s0), nz), gc1(gc0.x, (unsigned)((H + s1 - 1) / s1), nz);
        uint8_t* o = out + n0 * npix * out_channels;
        hipLaunchKernelGGL(ct_rows_kernel, gr, dim3(NT), 0, st, frames_u8, frames_u8, alpha_u8, n0, n0, P, H, W, r0, rows);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(ct_cols_kernel<0>, gc0, dim3(NT), 0, st, (const uint32_t*)rows, frames_u8, alpha_u8, n0, P, H, W, r0, s0, f1, b1);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(ct_rows_kernel, gr, dim3(NT), 0, st, (const uint8_t*)f1, (const uint8_t*)b1, alpha_u8, n0, 0L, 1, H, W, r1, rows);
        MG_CHECK_LAUNCH();
        if (out_channels == 4)
            hipLaunchKernelGGL(ct_cols_kernel<2>, gc1, dim3(NT), 0, st, (const uint32_t*)rows, frames_u8, alpha_u8, n0, P, H, W, r1, s1, o, (uint8_t*)nullptr);
        else
            hipLaunchKernelGGL(ct_cols_kernel<1>, gc1, dim3(NT), 0, st, (const uint32_t*)rows, frames_u8, alpha_u8, n0, P, H, W, r1, s1, o, (uint8_t*)nullptr);
        MG_CHECK_LAUNCH();
    }
    return 0;
}
