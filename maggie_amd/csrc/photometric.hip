// The photometric steps of the loaders' training stream on uint8 frames (reference: maggie/dataloader/transforms.py:812-924, wired in him.py:46-48
//   and vim.py:51-54): a per-channel tone curve, additive noise and the JPEG round trip of imgaug's JpegCompression, which saves with Pillow
//   and opens the file again. What runs here is the lossy part of libjpeg-turbo at Pillow's defaults -- baseline, 4:2:0, JDCT_ISLOW, no
//   smoothing, fancy upsampling -- without the entropy coding, which is lossless. All of it is int32 work; `>>` is arithmetic. Bit-exact.
//
// jpeg_ycc_kernel   frames [T][h][w][3] -> decoded component planes Y [T][h16][w16], Cb and Cr [T][h16 / 2][w16 / 2]. A workgroup owns a
//   MG_JPEG_TILE_ROWS x MG_JPEG_TILE_COLS tile of whole 16 x 16 MCUs: 32 luma and 2 x 8 chroma blocks, 48 in all, and has 48 * 8 = 384 lanes.
//   Load: a lane owns 2 x 2 pixel quads; the source coordinates are clamped (the encoder's edge replication), the tone curve and the noise are
//   applied to the pixel read, RGB -> YCbCr, h2v2 downsampling with the alternating bias. Past the last real chroma row of an even-height image
//   the chroma comes from rows h - 2 and h - 1 (libjpeg replicates the last DOWNSAMPLED row), the luma from row h - 1.
//   Transform: one lane runs one 8-point 1-D pass, so a wave64 covers eight blocks. Forward rows; then, per column and in registers, forward
//   columns, quantise, dequantise and the inverse transform's column pass (which comes first there); then inverse rows, + 128, clamp and one
//   8-byte store per lane. The passes exchange through LDS: an int32 block is [8][9] dwords (row pitch 9) at a pitch of 72, which makes both
//   the row-wise and the column-wise ds_read_b32 / ds_write_b32 of a 32-lane half fall into 32 different banks.
//   Quantisation divides by qv = 8 t, t = 1..255 read from the DEVICE table: each workgroup derives m = floor((2^32 - 1) / qv) + 1 =
//   ceil(2^32 / qv) per entry and takes (n * m) >> 32, which equals n / qv for every n < 2^32 / 2040 (tests/test_photometric_cpu.py runs the
//   whole range the transform can produce).
// jpeg_rgb_kernel   planes -> frames: a lane owns 16 pixels of one output row; triangle upsampling of Cb / Cr from the real
//   ceil(h / 2) x ceil(w / 2) samples (neighbours clamped to them, never the padding), 2 x 2 replication when ceil(w / 2) <= 2, YCbCr -> RGB, clamp;
//   three uint4 of raw bytes, or four float4 per channel plane with the Normalize epilogue of pixel_norm.h; per element on ragged widths and
//   unaligned bases.
// jpeg_rgb_hv_kernel the same for the planes mg_jpegdec_idct leaves (luma sampling (2,1), (1,2) or (4,1) over (1,1) chroma, DESIGN.md section
//   31): 16 luma bytes and 8 / 2 x 16 / 4 chroma bytes per lane in one load each; 4:2:2 the triangle filter along the row (replication when
//   ceil(w / 2) <= 2), 4:4:0 along the column at every width, 4:1:1 replication; neighbours clamped to the real samples.
// photo_point_kernel the tone curve and / or the saturating add alone, the same 16 pixels per lane and the same two epilogues.
#ifndef MG_HOST_EMU
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"
#endif

namespace {
#include "jpeg_common.h"

constexpr int TH = MG_JPEG_TILE_ROWS, TW = MG_JPEG_TILE_COLS;
constexpr int NYB = (TH / 8) * (TW / 8), NCB = (TH / 16) * (TW / 16);      // luma blocks, chroma blocks per component
constexpr int NB = NYB + 2 * NCB;                                          // 48 blocks
constexpr int NT = MG_JPEG_THREADS;                                        // one lane per block row / column
constexpr int RP = 9, BP = 8 * RP;                                         // row and block pitch in dwords
constexpr int PT = 256;                                                    // the pointwise kernels
static_assert(TH == 32 && TW == 64 && NT == NB * 8 && NT % 64 == 0, "384 lanes: 48 blocks of 8 lines");

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(NT) void jpeg_ycc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ planes, const uint8_t* __restrict__ lut,
                                                      const int16_t* __restrict__ noise, int nc, const int32_t* __restrict__ qtab, long frames,
                                                      int h, int w, int h16, int w16, int tiles_x, int tiles) {
    __shared__ int s_blk[NB * BP];
    __shared__ int s_t[128];
    __shared__ unsigned s_m[128];
    const int tid = threadIdx.x;
    const long t = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - t * tiles);
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
    if (tid < 128) {
        const int q = min(max(qtab[tid], 1), 255);                          // a table rewritten on the device may hold anything
        s_t[tid] = q;
        s_m[tid] = 0xFFFFFFFFu / (unsigned)(8 * q) + 1u;                    // ceil(2^32 / qv)
    }
    const uint8_t* __restrict__ src = in + t * ((long)h * w * 3);
    const int g1 = (nc == 3) ? 1 : 0, g2 = (nc == 3) ? 2 : 0;

    // the pixel at (y, x), 0 <= y < h, 0 <= x < w, after the tone curve and the noise, as Y, Cb and Cr before their final shift
    auto pixel = [&](int y, int x, int& Y, int& Cb, int& Cr) {
        const long o = (long)y * w + x;
        const uint8_t* p = src + o * 3;
        int r = p[0], g = p[1], b = p[2];
        if (lut) { r = lut[r]; g = lut[256 + g]; b = lut[512 + b]; }
        if (noise) {
            const int16_t* n = noise + o * nc;
            r = clamp255(r + n[0]); g = clamp255(g + n[g1]); b = clamp255(b + n[g2]);
        }
        Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
        Cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
        Cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    };

    // ---- load, convert, downsample ----
    const int chr = (h + 1) >> 1;                                           // real chroma rows
    for (int k = tid; k < (TH / 2) * (TW / 2); k += NT) {
        const int qy = k / (TW / 2), qx = k - qy * (TW / 2);
        const int gy = (ty0 >> 1) + qy, gx = (tx0 >> 1) + qx;               // the chroma sample of this quad
        const int x0 = min(2 * gx, w - 1), x1 = min(2 * gx + 1, w - 1);
        const int y0 = min(2 * gy, h - 1), y1 = min(2 * gy + 1, h - 1);
        int Y[4], cb[4], cr[4];
        pixel(y0, x0, Y[0], cb[0], cr[0]);
        pixel(y0, x1, Y[1], cb[1], cr[1]);
        pixel(y1, x0, Y[2], cb[2], cr[2]);
        pixel(y1, x1, Y[3], cb[3], cr[3]);
        if (gy >= chr && !(h & 1)) {                                        // below an even image: the last downsampled row, rows h - 2 and h - 1
            int unused;
            pixel(h - 2, x0, unused, cb[0], cr[0]);
            pixel(h - 2, x1, unused, cb[1], cr[1]);
        }
        const int bias = 1 + (gx & 1);
        const int Cb = (cb[0] + cb[1] + cb[2] + cb[3] + bias) >> 2, Cr = (cr[0] + cr[1] + cr[2] + cr[3] + bias) >> 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ly = 2 * qy + (e >> 1), lx = 2 * qx + (e & 1);
            s_blk[((ly >> 3) * (TW / 8) + (lx >> 3)) * BP + (ly & 7) * RP + (lx & 7)] = Y[e] - 128;
        }
        const int cblk = NYB + (qy >> 3) * (TW / 16) + (qx >> 3), co = (qy & 7) * RP + (qx & 7);
        s_blk[cblk * BP + co] = Cb - 128;
        s_blk[(cblk + NCB) * BP + co] = Cr - 128;
    }
    __syncthreads();

    const int b = tid >> 3, l = tid & 7;
    int* __restrict__ blk = s_blk + b * BP;
    int d[8];
    // ---- forward rows ----
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[l * RP + k];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[l * RP + k] = d[k];
    __syncthreads();
    // ---- forward columns, quantise, dequantise, inverse columns ----
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[k * RP + l];
    fdct8<false>(d);
    const int sel = b >= NYB ? 64 : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = s_t[sel + k * 8 + l];
        const unsigned n = (unsigned)abs(d[k]) + (unsigned)(4 * q);        // |c| + qv / 2, far below 2^32 / 2040
        const int kq = (int)__umulhi(n, s_m[sel + k * 8 + l]);             // n / (8 q)
        d[k] = (d[k] < 0 ? -kq : kq) * q;
    }
    idct8<11>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[k * RP + l] = d[k];
    __syncthreads();
    // ---- inverse rows, + 128, clamp, store ----
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[l * RP + k];
    idct8<18>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)clamp255(d[k] + 128) << (8 * k);
        hi |= (uint32_t)clamp255(d[k + 4] + 128) << (8 * k);
    }
    const int hc = h16 >> 1, wc = w16 >> 1;
    if (b < NYB) {
        const int gy = ty0 + (b / (TW / 8)) * 8 + l, gx = tx0 + (b % (TW / 8)) * 8;
        if (gy < h16 && gx < w16) *(uint2*)(planes + (t * h16 + gy) * (long)w16 + gx) = make_uint2(lo, hi);
    } else {
        const int c = (b - NYB) / NCB, cb = (b - NYB) % NCB;
        const int gy = (ty0 >> 1) + (cb / (TW / 16)) * 8 + l, gx = (tx0 >> 1) + (cb % (TW / 16)) * 8;
        uint8_t* __restrict__ plane = planes + frames * (long)h16 * w16 + c * (frames * (long)hc * wc);
        if (gy < hc && gx < wc) *(uint2*)(plane + (t * hc + gy) * (long)wc + gx) = make_uint2(lo, hi);
    }
}

// 16 pixels of row y of frame t from x0 on, n of them real: raw bytes [T][h][w][3] or the normalised planes [T][3][h][w]
template <int EPI>
__device__ __forceinline__ void store16(const int (&px)[16][3], void* __restrict__ out, long t, int y, int x0, int n, int h, int w, int vec,
                                        const float (&mean)[3], const float (&std)[3]) {
    if constexpr (EPI == MG_PHOTO_RAW) {
        uint8_t* __restrict__ dst = (uint8_t*)out + ((t * h + y) * (long)w + x0) * 3;
        if (vec) {
            uint32_t wd[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                wd[q] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const int e = 4 * q + k; wd[q] |= (uint32_t)px[e / 3][e % 3] << (8 * k); }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) ((uint4*)dst)[q] = make_uint4(wd[4 * q], wd[4 * q + 1], wd[4 * q + 2], wd[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < n) { dst[3 * j] = (uint8_t)px[j][0]; dst[3 * j + 1] = (uint8_t)px[j][1]; dst[3 * j + 2] = (uint8_t)px[j][2]; }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* __restrict__ dst = (float*)out + ((t * 3 + c) * h + y) * (long)w + x0;
            float f[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) f[j] = mg_norm_u8(px[j][c], mean[c], std[c]);
            if (vec) {
#pragma unroll
                for (int q = 0; q < 4; ++q) ((float4*)dst)[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j < n) dst[j] = f[j];
            }
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(PT) void jpeg_rgb_kernel(const uint8_t* __restrict__ planes, void* __restrict__ out, long frames, int h, int w, int h16,
                                                      int w16, int groups, long units, int vec, float m0, float m1, float m2, float s0, float s1,
                                                      float s2) {
    const long u = (long)blockIdx.x * PT + threadIdx.x;
    if (u >= units) return;
    const long row = u / groups, t = row / h;
    const int y = (int)(row - t * h), x0 = (int)(u - row * groups) * 16, n = min(16, w - x0);
    const int chr = (h + 1) >> 1, cwr = (w + 1) >> 1, hc = h16 >> 1, wc = w16 >> 1;
    // 16 luma samples: x0 + 15 < w16
    const uint4 yv = *(const uint4*)(planes + (t * h16 + y) * (long)w16 + x0);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    // the chroma row of this output row and its vertical neighbour among the REAL rows; columns j0 - 1 .. j0 + 8 among the real columns
    const int i = y >> 1, inb = (y & 1) ? min(i + 1, chr - 1) : max(i - 1, 0);
    const int j0 = x0 >> 1, jl = max(j0 - 1, 0), jr = min(j0 + 8, cwr - 1);
    const bool fancy = cwr > 2;
    int c16[2][16];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* __restrict__ plane = planes + frames * (long)h16 * w16 + c * (frames * (long)hc * wc) + t * (long)hc * wc;
        const uint8_t* __restrict__ ra = plane + (long)i * wc;
        const uint8_t* __restrict__ rb = plane + (long)inb * wc;
        const uint2 a = *(const uint2*)(ra + j0), bb = *(const uint2*)(rb + j0);                    // j0 + 7 < wc
        int p[10], s[10];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            p[k + 1] = (int)(((k < 4 ? a.x : a.y) >> (8 * (k & 3))) & 255u);
            s[k + 1] = 3 * p[k + 1] + (int)(((k < 4 ? bb.x : bb.y) >> (8 * (k & 3))) & 255u);
        }
        s[0] = 3 * (int)ra[jl] + (int)rb[jl];
        s[9] = 3 * (int)ra[jr] + (int)rb[jr];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = j0 + k, cur = s[k + 1];
            const int left = j == 0 ? cur : s[k], right = j >= cwr - 1 ? cur : s[k + 2];
            c16[c][2 * k] = fancy ? (3 * cur + left + 8) >> 4 : p[k + 1];
            c16[c][2 * k + 1] = fancy ? (3 * cur + right + 7) >> 4 : p[k + 1];
        }
    }
    int px[16][3];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int Y = (int)((yw[j >> 2] >> (8 * (j & 3))) & 255u), cb = c16[0][j] - 128, cr = c16[1][j] - 128;
        px[j][0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
        px[j][1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        px[j][2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    store16<EPI>(px, out, t, y, x0, n, h, w, vec, mean, std);
}

// planes as mg_jpegdec_idct leaves them: Y [T][ph][yp], Cb and Cr [T][chh][cp]; yp is a multiple of 16 and cp of the chroma bytes a lane loads,
// so that every load below lies inside its row and is aligned to its own size
template <int EPI, int HS, int VS>
__global__ __launch_bounds__(PT) void jpeg_rgb_hv_kernel(const uint8_t* __restrict__ planes, void* __restrict__ out, long frames, int h, int w, int ph,
                                                         int yp, int chh, int cp, int groups, long units, int vec, float m0, float m1, float m2,
                                                         float s0, float s1, float s2) {
    const long u = (long)blockIdx.x * PT + threadIdx.x;
    if (u >= units) return;
    const long row = u / groups, t = row / h;
    const int y = (int)(row - t * h), x0 = (int)(u - row * groups) * 16, n = min(16, w - x0);
    const int chr = (h + VS - 1) / VS, cwr = (w + HS - 1) / HS;          // the real chroma samples
    const uint4 yv = *(const uint4*)(planes + (t * ph + y) * (long)yp + x0);                        // x0 + 15 < yp
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    int c16[2][16];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* __restrict__ plane = planes + frames * (long)ph * yp + c * (frames * (long)chh * cp) + t * (long)chh * cp;
        if constexpr (HS == 2) {                                           // 4:2:2: columns j0 - 1 .. j0 + 8 of this row among the real columns
            const uint8_t* __restrict__ ra = plane + (long)y * cp;
            const int j0 = x0 >> 1, jl = max(j0 - 1, 0), jr = min(j0 + 8, cwr - 1);
            const uint2 a = *(const uint2*)(ra + j0);                      // j0 + 7 < cp
            int p[10];
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k + 1] = (int)(((k < 4 ? a.x : a.y) >> (8 * (k & 3))) & 255u);
            p[0] = ra[jl];
            p[9] = ra[jr];
            const bool fancy = cwr > 2;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = j0 + k, cur = p[k + 1];
                const int left = j == 0 ? cur : p[k], right = j >= cwr - 1 ? cur : p[k + 2];
                c16[c][2 * k] = fancy ? (3 * cur + left + 1) >> 2 : cur;
                c16[c][2 * k + 1] = fancy ? (3 * cur + right + 2) >> 2 : cur;
            }
        } else if constexpr (VS == 2) {                                    // 4:4:0: the row's chroma row and its neighbour among the REAL rows
            const int i = y >> 1, inb = (y & 1) ? min(i + 1, chr - 1) : max(i - 1, 0), bias = 1 + (y & 1);
            const uint4 a = *(const uint4*)(plane + (long)i * cp + x0), b = *(const uint4*)(plane + (long)inb * cp + x0);      // x0 + 15 < cp
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                c16[c][k] = (3 * (int)((aw[k >> 2] >> (8 * (k & 3))) & 255u) + (int)((bw[k >> 2] >> (8 * (k & 3))) & 255u) + bias) >> 2;
        } else {                                                           // 4:1:1: four columns of this row, each four times
            const uint32_t a = *(const uint32_t*)(plane + (long)y * cp + (x0 >> 2));               // x0 / 4 + 3 < cp
#pragma unroll
            for (int k = 0; k < 16; ++k) c16[c][k] = (int)((a >> (8 * (k >> 2))) & 255u);
        }
    }
    int px[16][3];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int Y = (int)((yw[j >> 2] >> (8 * (j & 3))) & 255u), cb = c16[0][j] - 128, cr = c16[1][j] - 128;
        px[j][0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
        px[j][1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        px[j][2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    store16<EPI>(px, out, t, y, x0, n, h, w, vec, mean, std);
}

template <int EPI>
__global__ __launch_bounds__(PT) void photo_point_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, const uint8_t* __restrict__ lut,
                                                         const int16_t* __restrict__ noise, int nc, int h, int w, int groups, long units, int vin,
                                                         int vec, float m0, float m1, float m2, float s0, float s1, float s2) {
    const long u = (long)blockIdx.x * PT + threadIdx.x;
    if (u >= units) return;
    const long row = u / groups, t = row / h;
    const int y = (int)(row - t * h), x0 = (int)(u - row * groups) * 16, n = min(16, w - x0);
    const uint8_t* __restrict__ src = in + ((t * h + y) * (long)w + x0) * 3;
    int px[16][3] = {};
    if (vin) {
        uint32_t wd[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint4 v = ((const uint4*)src)[q];
            wd[4 * q] = v.x; wd[4 * q + 1] = v.y; wd[4 * q + 2] = v.z; wd[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int e = 0; e < 48; ++e) px[e / 3][e % 3] = (int)((wd[e >> 2] >> (8 * (e & 3))) & 255u);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < n) { px[j][0] = src[3 * j]; px[j][1] = src[3 * j + 1]; px[j][2] = src[3 * j + 2]; }
    }
    if (lut) {
#pragma unroll
        for (int j = 0; j < 16; ++j) { px[j][0] = lut[px[j][0]]; px[j][1] = lut[256 + px[j][1]]; px[j][2] = lut[512 + px[j][2]]; }
    }
    if (noise) {
        const int16_t* __restrict__ nz = noise + ((long)y * w + x0) * nc;
        const int g1 = (nc == 3) ? 1 : 0, g2 = (nc == 3) ? 2 : 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < n) {
                px[j][0] = clamp255(px[j][0] + nz[j * nc]);
                px[j][1] = clamp255(px[j][1] + nz[j * nc + g1]);
                px[j][2] = clamp255(px[j][2] + nz[j * nc + g2]);
            }
    }
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    store16<EPI>(px, out, t, y, x0, n, h, w, vec, mean, std);
}

bool bad_size(long frames, int h, int w) { return frames < 0 || h <= 0 || w <= 0 || h > MG_JPEG_MAX_SIDE || w > MG_JPEG_MAX_SIDE; }
bool bad_epilogue(int e) { return e != MG_PHOTO_RAW && e != MG_PHOTO_NORM; }

// 16-byte stores: whole groups of 16 pixels per row and an aligned base (a row of the raw form is 3 w bytes, of a normalised plane 4 w)
int vec_ok(const void* p, int w) { return (w % 16 == 0) && ((uintptr_t)p % 16 == 0); }

}  // namespace

extern "C" int mg_jpeg_limits(int* tile_rows, int* tile_cols, int* threads, int* max_side) {
    if (!tile_rows || !tile_cols || !threads || !max_side) return -2;
    *tile_rows = TH; *tile_cols = TW; *threads = NT; *max_side = MG_JPEG_MAX_SIDE;
    return 0;
}

extern "C" int mg_jpeg_ycc(const uint8_t* in, uint8_t* planes, const uint8_t* lut, const int16_t* noise, int noise_channels, const int32_t* qtab,
                           long frames, int h, int w, void* stream) {
    if (bad_size(frames, h, w) || (noise && noise_channels != 1 && noise_channels != 3)) return -2;
    if (frames == 0) return 0;
    if (!in || !planes || !qtab || in == planes || (uintptr_t)planes % 16 != 0) return -2;
    const int h16 = (h + 15) & ~15, w16 = (w + 15) & ~15;
    const int tiles_x = (w16 + TW - 1) / TW;
    const long tiles = (long)tiles_x * ((h16 + TH - 1) / TH);
    if (frames > 0x7fffffffL / tiles) return -3;
    hipLaunchKernelGGL(jpeg_ycc_kernel, dim3((unsigned)(frames * tiles)), dim3(NT), 0, (hipStream_t)stream, in, planes, lut, noise, noise_channels,
                       qtab, frames, h, w, h16, w16, tiles_x, (int)tiles);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_jpeg_rgb(const uint8_t* planes, void* out, long frames, int h, int w, int epilogue, const float* mean3, const float* std3,
                           void* stream) {
    if (bad_size(frames, h, w) || bad_epilogue(epilogue) || !mean3 || !std3) return -2;
    if (frames == 0) return 0;
    if (!planes || !out || (const void*)planes == out || (uintptr_t)planes % 16 != 0) return -2;
    const int h16 = (h + 15) & ~15, w16 = (w + 15) & ~15, groups = (w + 15) / 16;
    if (frames > 0x7fffffffffL / ((long)h * groups)) return -3;
    const long units = frames * h * groups, blocks = (units + PT - 1) / PT;
    if (blocks > 0x7fffffffL) return -3;
    const int vec = vec_ok(out, w);
    if (epilogue == MG_PHOTO_RAW)
        hipLaunchKernelGGL(jpeg_rgb_kernel<MG_PHOTO_RAW>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, planes, out, frames, h, w, h16, w16,
                           groups, units, vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
        hipLaunchKernelGGL(jpeg_rgb_kernel<MG_PHOTO_NORM>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, planes, out, frames, h, w, h16, w16,
                           groups, units, vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_jpeg_rgb_hv(const uint8_t* planes, long plane_bytes, void* out, long frames, int h, int w, int hs, int vs, int epilogue,
                              const float* mean3, const float* std3, void* stream) {
    if (bad_size(frames, h, w) || bad_epilogue(epilogue) || !mean3 || !std3 || !((hs == 2 && vs == 1) || (hs == 1 && vs == 2) || (hs == 4 && vs == 1)))
        return -2;
    // mg_jpegdec_idct's planes: whole MCUs, the luma pitch a multiple of 16, the 4:4:0 chroma pitch too
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int ph = mcuy * 8 * vs, yp = (mcux * 8 * hs + 15) & ~15, chh = mcuy * 8, cp = vs == 2 ? (mcux * 8 + 15) & ~15 : mcux * 8;
    if (plane_bytes != frames * ((long)ph * yp + 2L * chh * cp)) return -2;
    if (frames == 0) return 0;
    if (!planes || !out || (const void*)planes == out || (uintptr_t)planes % 16 != 0) return -2;
    const int groups = (w + 15) / 16;
    if (frames > 0x7fffffffffL / ((long)h * groups)) return -3;
    const long units = frames * h * groups, blocks = (units + PT - 1) / PT;
    if (blocks > 0x7fffffffL) return -3;
    const int vec = vec_ok(out, w);
#define MG_RGB_HV(E, H, V)                                                                                                                         \
    hipLaunchKernelGGL((jpeg_rgb_hv_kernel<E, H, V>), dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, planes, out, frames, h, w, ph, yp, \
                       chh, cp, groups, units, vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2])
    if (epilogue == MG_PHOTO_RAW) {
        if (hs == 2) MG_RGB_HV(MG_PHOTO_RAW, 2, 1);
        else if (vs == 2) MG_RGB_HV(MG_PHOTO_RAW, 1, 2);
        else MG_RGB_HV(MG_PHOTO_RAW, 4, 1);
    } else {
        if (hs == 2) MG_RGB_HV(MG_PHOTO_NORM, 2, 1);
        else if (vs == 2) MG_RGB_HV(MG_PHOTO_NORM, 1, 2);
        else MG_RGB_HV(MG_PHOTO_NORM, 4, 1);
    }
#undef MG_RGB_HV
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_photo_noise(const uint8_t* in, void* out, const uint8_t* lut, const int16_t* noise, int noise_channels, long frames, int h, int w,
                              int epilogue, const float* mean3, const float* std3, void* stream) {
    if (bad_size(frames, h, w) || bad_epilogue(epilogue) || !mean3 || !std3 || (noise && noise_channels != 1 && noise_channels != 3)) return -2;
    if (frames == 0) return 0;
    if (!in || !out || (const void*)in == out) return -2;
    const int groups = (w + 15) / 16;
    if (frames > 0x7fffffffffL / ((long)h * groups)) return -3;
    const long units = frames * h * groups, blocks = (units + PT - 1) / PT;
    if (blocks > 0x7fffffffL) return -3;
    const int vin = vec_ok(in, w), vec = vec_ok(out, w);
    if (epilogue == MG_PHOTO_RAW)
        hipLaunchKernelGGL(photo_point_kernel<MG_PHOTO_RAW>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, in, out, lut, noise,
                           noise_channels, h, w, groups, units, vin, vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
        hipLaunchKernelGGL(photo_point_kernel<MG_PHOTO_NORM>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, in, out, lut, noise,
                           noise_channels, h, w, groups, units, vin, vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MG_CHECK_LAUNCH();
    return 0;
}
