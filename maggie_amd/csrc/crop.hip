// The training crop of the loaders on uint8 images (reference: maggie/dataloader/transforms.py:191-305, RandomCropByAlpha -> RandomHorizontalFlip,
//   between PaddingMultiplyBy and the mask chain in him.py:36-65 / vim.py:43-74). The draws are the host's (maggie_amd/utils/crop.py); what runs
//   here is the data-dependent part of them and the pixels. Integer work and the IEEE divisions of pixel_norm.h: every result is bit-exact.
//
// crop_bbox_kernel       box of `alphas.mean(0) > 127` as the integer test sum_p alpha > 127 * P: a lane owns 16 consecutive pixels of a row and
//   walks the P planes with one 16-byte load each; per-workgroup count and extremes by LDS atomics, then one set of global integer atomics
//   per workgroup that found a pixel. Rows are spread over the whole grid (27 648 lanes for 576 x 768), not one workgroup per plane.
// crop_hits_kernel       `(crop_alphas > 127).sum() > 0` for up to three candidate windows: a wave per window row and plane, 16-byte chunks
//   tested with `& 0x80808080`, the ragged ends of a row byte by byte; one atomicOr per wave that saw a pixel. Reads the windows only.
// crop_gather_kernel     the crop and the flip: a lane owns 16 pixels of one output row, reads them with unaligned 16-byte loads (x0 is
//   arbitrary), reverses the pixel order in registers when flipped, and stores 16 bytes (uint8) or float4s (the Normalize epilogue). The window
//   and the flip come from a device table, so a captured launch follows new draws.
// crop_padresize_kernel  the padding branch (10 % of the items): the direct-tap form of geometry.hip's resize in padded coordinates; a tap that
//   falls into the border reads 0. Four pixels per lane.
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"

namespace {

constexpr int NT = 256;
constexpr int CK = MG_CROP_CHUNK;           // pixels per lane of the gather and the box
constexpr int PY = NT / 64, PX = 256;       // the pad-and-resize tile: one wave per output row, four pixels per lane

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- the box and the hit test ----------------------------------------------------------------------------------------------------------------
__global__ void crop_init_kernel(int32_t* __restrict__ out, int n, int H, int W) {
    // n == 0: the five words of the box (0, W, -1, H, -1); otherwise n zeroed hit words
    if (threadIdx.x == 0) {
        if (n == 0) { out[0] = 0; out[1] = W; out[2] = -1; out[3] = H; out[4] = -1; }
        else for (int k = 0; k < n; ++k) out[k] = 0;
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void crop_bbox_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ box, int P, int H, int W, int groups,
                                                       long units) {
    __shared__ int s[5];
    if (threadIdx.x == 0) { s[0] = 0; s[1] = W; s[2] = -1; s[3] = H; s[4] = -1; }
    __syncthreads();
    const long u = (long)blockIdx.x * NT + threadIdx.x;
    int cnt = 0, xmin = W, xmax = -1, y = 0;
    if (u < units) {
        y = (int)(u / groups);
        const int x0 = (int)(u - (long)y * groups) * CK, n = min(CK, W - x0);
        const long HW = (long)H * W;
        const uint8_t* __restrict__ src = in + (long)y * W + x0;
        int sum[CK] = {};
        for (int p = 0; p < P; ++p, src += HW) {
            if constexpr (VEC) {                                           // W % 16 == 0 and a 16-byte aligned base: every chunk is aligned and whole
                const uint4 v = *(const uint4*)src;
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < CK; ++j) sum[j] += (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            } else {
#pragma unroll
                for (int j = 0; j < CK; ++j)
                    if (j < n) sum[j] += (int)src[j];
            }
        }
        const int thr = 127 * P;                                           // P <= MG_CROP_MAX_PLANES: 255 * P fits
#pragma unroll
        for (int j = 0; j < CK; ++j)
            if (j < n && sum[j] > thr) { ++cnt; xmin = min(xmin, x0 + j); xmax = max(xmax, x0 + j); }
    }
    if (cnt) {                                                             // integer atomics: the result does not depend on order
        atomicAdd(&s[0], cnt); atomicMin(&s[1], xmin); atomicMax(&s[2], xmax); atomicMin(&s[3], y); atomicMax(&s[4], y);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s[0] > 0) {
        atomicAdd(&box[0], s[0]); atomicMin(&box[1], s[1]); atomicMax(&box[2], s[2]); atomicMin(&box[3], s[3]); atomicMax(&box[4], s[4]);
    }
}

__global__ __launch_bounds__(NT) void crop_hits_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ windows, int32_t* __restrict__ hits,
                                                       int P, int H, int W, int ch, int cw, int row_blocks, int aligned) {
    const long blk = blockIdx.x;
    const int rb = (int)(blk % row_blocks);
    const long kp = blk / row_blocks;
    const int p = (int)(kp % P), k = (int)(kp / P);
    const int y = rb * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= ch) return;
    const int x0 = clampi(windows[2 * k], 0, W - cw), y0 = clampi(windows[2 * k + 1], 0, H - ch);
    const long s = ((long)p * H + y0 + y) * W + x0, e = s + cw;            // the row of the window as byte offsets [s, e) into `in`
    bool hit = false;
    for (long c = (s >> 4) + lane; c * 16 < e; c += 64) {
        const long b = c * 16;
        if (aligned && b >= s && b + 16 <= e) {
            const uint4 v = *(const uint4*)(in + b);
            hit |= ((v.x | v.y | v.z | v.w) & 0x80808080u) != 0u;          // > 127 is the top bit
        } else {
            for (long a = max(b, s); a < min(b + 16, e); ++a) hit |= in[a] > 127;
        }
    }
    if (__ballot(hit) != 0ull && lane == 0) atomicOr(&hits[k], 1);
}

// ---- the pixels ------------------------------------------------------------------------------------------------------------------------------
struct Crop {
    const uint8_t* in;
    void* out;
    const int32_t* window;
    const int32_t* xtab;
    const int32_t* ytab;
    const uint8_t* lut;
    int H, W, ch, cw, pad_h, pad_w, epilogue, vec, chunks, tiles_x, tiles;
    long units;
    float mean[3], std[3];
};

// N pixels (y, x0 .. x0 + N - 1) of output image i, the first n of them inside the row, through the launch's epilogue; x0 a multiple of N
template <int C, int N>
__device__ __forceinline__ void emit(const Crop& g, long i, int y, int x0, int n, const int (&v)[N][C]) {
    const bool vec = g.vec && n == N;
    const long HWo = (long)g.ch * g.cw, pix = (long)y * g.cw + x0;
    if (g.epilogue == MG_CROP_RAW) {
        uint8_t* o = (uint8_t*)g.out + (i * HWo + pix) * C;
        if (vec) {
            uint32_t word[N * C / 4];
#pragma unroll
            for (int w = 0; w < N * C / 4; ++w) {
                word[w] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const int e = 4 * w + k; word[w] |= (uint32_t)(v[e / C][e % C] & 255) << (8 * k); }
            }
            if constexpr (N == 16) {
#pragma unroll
                for (int q = 0; q < C; ++q) ((uint4*)o)[q] = make_uint4(word[4 * q], word[4 * q + 1], word[4 * q + 2], word[4 * q + 3]);
            } else {
#pragma unroll
                for (int w = 0; w < N * C / 4; ++w) ((uint32_t*)o)[w] = word[w];
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j < n) {
#pragma unroll
                    for (int c = 0; c < C; ++c) o[j * C + c] = (uint8_t)v[j][c];
                }
        }
    } else {
        if constexpr (C == 3) {
            float* o = (float*)g.out + i * 3 * HWo + pix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float f[N];
#pragma unroll
                for (int j = 0; j < N; ++j) f[j] = mg_norm_u8(v[j][c] & 255, g.mean[c], g.std[c]);
                if (vec) {
#pragma unroll
                    for (int q = 0; q < N / 4; ++q) ((float4*)(o + c * HWo))[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
                } else {
#pragma unroll
                    for (int j = 0; j < N; ++j)
                        if (j < n) o[c * HWo + j] = f[j];
                }
            }
        }
    }
}

template <int C, int N>
__device__ __forceinline__ void tone(const uint8_t* s_lut, int (&v)[N][C]) {
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) v[j][c] = s_lut[c * 256 + (v[j][c] & 255)];
}

template <int C>
__device__ __forceinline__ bool stage_lut(const Crop& g, uint8_t* s_lut) {
    if (!g.lut) return false;                                              // the same for every thread of the launch
    for (int k = threadIdx.x; k < 256 * C; k += NT) s_lut[k] = g.lut[k];
    __syncthreads();
    return true;
}

template <int C>
__global__ __launch_bounds__(NT) void crop_gather_kernel(Crop g) {
    __shared__ uint8_t s_lut[256 * C];
    const bool lut = stage_lut<C>(g, s_lut);
    const long u = (long)blockIdx.x * NT + threadIdx.x;
    if (u >= g.units) return;
    const long t = u / g.chunks;
    const int j = (int)(u - t * g.chunks);
    const long i = t / g.ch;
    const int y = (int)(t - i * g.ch);
    const int x0 = clampi(g.window[0], 0, g.W - g.cw), y0 = clampi(g.window[1], 0, g.H - g.ch);
    const bool flip = g.window[2] != 0;
    const int n = min(CK, g.cw - CK * j);
    const uint8_t* __restrict__ row = g.in + ((i * g.H + y0 + y) * (long)g.W + x0) * C;     // the window's row: cw * C bytes, all inside the source
    int v[CK][C] = {};
    if (n == CK) {
        // 16 whole pixels: 16 * C contiguous bytes, read as unaligned words; flipped, they are the mirrored run in reverse pixel order
        const int sx = flip ? g.cw - CK * (j + 1) : CK * j;
        uint32_t w[4 * C];
        __builtin_memcpy(w, row + (long)sx * C, sizeof(w));
#pragma unroll
        for (int q = 0; q < CK; ++q)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int b = (flip ? CK - 1 - q : q) * C + c;
                v[q][c] = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u);
            }
    } else {
#pragma unroll
        for (int q = 0; q < CK; ++q)                                       // unrolled: `v` stays in registers
            if (q < n) {
                const int sx = flip ? g.cw - 1 - (CK * j + q) : CK * j + q;
#pragma unroll
                for (int c = 0; c < C; ++c) v[q][c] = row[(long)sx * C + c];
            }
    }
    if (lut) tone<C, CK>(s_lut, v);
    emit<C, CK>(g, i, y, CK * j, n, v);
}

template <int C, bool NEAREST>
__global__ __launch_bounds__(NT) void crop_padresize_kernel(Crop g) {
    __shared__ uint8_t s_lut[256 * C];
    const bool lut = stage_lut<C>(g, s_lut);
    const long blk = blockIdx.x;
    const long i = blk / g.tiles;
    const int tile = (int)(blk - i * g.tiles);
    const int y = (tile / g.tiles_x) * PY + (threadIdx.x >> 6), x0 = (tile % g.tiles_x) * PX + (threadIdx.x & 63) * 4;
    if (y >= g.ch || x0 >= g.cw) return;
    const int n = min(4, g.cw - x0);
    const int Hp = g.H + 2 * g.pad_h, Wp = g.W + 2 * g.pad_w;
    const uint8_t* __restrict__ src = g.in + i * (long)g.H * g.W * C;
    // a tap at padded coordinates (py, px): the source pixel, or the border's 0
    auto tap = [&](int py, int px, int c) -> int {
        const int sy = py - g.pad_h, sx = px - g.pad_w;
        return (sy >= 0 && sy < g.H && sx >= 0 && sx < g.W) ? (int)src[((long)sy * g.W + sx) * C + c] : 0;
    };
    int v[4][C] = {};
    if constexpr (NEAREST) {
        const int py = clampi(g.ytab[y], 0, Hp - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const int px = clampi(g.xtab[x0 + j], 0, Wp - 1);
#pragma unroll
                for (int c = 0; c < C; ++c) v[j][c] = tap(py, px, c);
            }
    } else {
        const int yo = clampi(g.ytab[3 * y], 0, Hp - 1), y1 = min(yo + 1, Hp - 1), b0 = g.ytab[3 * y + 1], b1 = g.ytab[3 * y + 2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const int gx = x0 + j;
                const int xo = clampi(g.xtab[3 * gx], 0, Wp - 1), x1 = min(xo + 1, Wp - 1);
                const int a0 = g.xtab[3 * gx + 1], a1 = g.xtab[3 * gx + 2];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int R0 = tap(yo, xo, c) * a0 + tap(yo, x1, c) * a1;
                    const int R1 = tap(y1, xo, c) * a0 + tap(y1, x1, c) * a1;
                    v[j][c] = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
                }
            }
    }
    if (lut) tone<C, 4>(s_lut, v);
    emit<C, 4>(g, i, y, x0, n, v);
}

bool bad_image(long images, int channels, int H, int W) {
    return images < 0 || (channels != 1 && channels != 3) || H <= 0 || W <= 0 || (long)H * W * channels > 0x7fffffffL;
}

bool bad_epilogue(int epilogue, int channels, const uint8_t* lut, const float* mean3, const float* std3) {
    if (epilogue != MG_CROP_RAW && epilogue != MG_CROP_NORM) return true;
    if (epilogue == MG_CROP_NORM && (channels != 3 || !mean3 || !std3)) return true;
    return lut && channels != 3;
}

void fill(Crop& g, const uint8_t* in, void* out, const uint8_t* lut, int H, int W, int ch, int cw, int epilogue, const float* mean3,
          const float* std3, int pixels_per_lane) {
    g.in = in; g.out = out; g.lut = lut; g.window = nullptr; g.xtab = nullptr; g.ytab = nullptr;
    g.H = H; g.W = W; g.ch = ch; g.cw = cw; g.pad_h = 0; g.pad_w = 0; g.epilogue = epilogue;
    g.chunks = 0; g.tiles_x = 0; g.tiles = 0; g.units = 0;
    for (int c = 0; c < 3; ++c) { g.mean[c] = mean3 ? mean3[c] : 0.f; g.std[c] = std3 ? std3[c] : 1.f; }
    // packed stores: a lane's pixels start on a 16-byte boundary (uint8 chunks of 16, fp32 groups of 4) or a 4-byte one (uint8 groups of 4)
    g.vec = (cw % pixels_per_lane == 0) && ((uintptr_t)out % 16 == 0);
}

}  // namespace

extern "C" int mg_crop_limits(int* max_windows, int* max_planes, int* chunk) {
    if (!max_windows || !max_planes || !chunk) return -2;
    *max_windows = MG_CROP_MAX_WINDOWS;
    *max_planes = MG_CROP_MAX_PLANES;
    *chunk = CK;
    return 0;
}

extern "C" int mg_crop_bbox(const uint8_t* alphas, int32_t* box, long planes, int H, int W, void* stream) {
    if (planes <= 0 || planes > MG_CROP_MAX_PLANES || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL) return -2;
    if (!alphas || !box) return -2;
    const int groups = (W + CK - 1) / CK;
    const long units = (long)H * groups, blocks = (units + NT - 1) / NT;
    if (blocks > 0x7fffffffL) return -3;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(crop_init_kernel, dim3(1), dim3(64), 0, st, box, 0, H, W);
    MG_CHECK_LAUNCH();
    if (W % CK == 0 && (uintptr_t)alphas % 16 == 0)
        hipLaunchKernelGGL(crop_bbox_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, st, alphas, box, (int)planes, H, W, groups, units);
    else
        hipLaunchKernelGGL(crop_bbox_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, st, alphas, box, (int)planes, H, W, groups, units);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_crop_hits(const uint8_t* alphas, const int32_t* windows, int32_t* hits, int n, long planes, int H, int W, int ch, int cw,
                            void* stream) {
    if (n < 0 || n > MG_CROP_MAX_WINDOWS || planes <= 0 || planes > MG_CROP_MAX_PLANES || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL) return -2;
    if (ch <= 0 || cw <= 0 || ch > H || cw > W) return -2;
    if (n == 0) return 0;
    if (!alphas || !windows || !hits) return -2;
    const int row_blocks = (ch + NT / 64 - 1) / (NT / 64);
    const long blocks = (long)n * planes * row_blocks;
    if (blocks > 0x7fffffffL) return -3;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(crop_init_kernel, dim3(1), dim3(64), 0, st, hits, n, H, W);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_hits_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, alphas, windows, hits, (int)planes, H, W, ch, cw, row_blocks,
                       (int)((uintptr_t)alphas % 16 == 0));
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_crop_gather(const uint8_t* in, void* out, const int32_t* window, const uint8_t* lut, long images, int channels, int H, int W,
                              int ch, int cw, int epilogue, const float* mean3, const float* std3, void* stream) {
    if (bad_image(images, channels, H, W) || ch <= 0 || cw <= 0 || ch > H || cw > W) return -2;
    if (bad_epilogue(epilogue, channels, lut, mean3, std3)) return -2;
    if (images == 0) return 0;
    if (!in || !out || !window) return -2;
    Crop g;
    fill(g, in, out, lut, H, W, ch, cw, epilogue, mean3, std3, CK);
    g.window = window;
    g.chunks = (cw + CK - 1) / CK;
    if (images > 0x7fffffffL / ch || images * ch > 0x7fffffffffL / g.chunks) return -3;
    g.units = images * ch * g.chunks;
    const long blocks = (g.units + NT - 1) / NT;
    if (blocks > 0x7fffffffL) return -3;
    hipStream_t st = (hipStream_t)stream;
    if (channels == 1) hipLaunchKernelGGL(crop_gather_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, st, g);
    else hipLaunchKernelGGL(crop_gather_kernel<3>, dim3((unsigned)blocks), dim3(NT), 0, st, g);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_crop_padresize(const uint8_t* in, void* out, const int32_t* xtab, const int32_t* ytab, const uint8_t* lut, long images,
                                 int channels, int H, int W, int pad_h, int pad_w, int dh, int dw, int interp, int epilogue, const float* mean3,
                                 const float* std3, void* stream) {
    if (bad_image(images, channels, H, W) || dh <= 0 || dw <= 0 || (long)dh * dw * channels > 0x7fffffffL) return -2;
    if (pad_h < 0 || pad_w < 0 || pad_h > 0x3fffffff - H || pad_w > 0x3fffffff - W) return -2;
    if (interp != MG_RESIZE_LINEAR && interp != MG_RESIZE_NEAREST) return -2;
    if (bad_epilogue(epilogue, channels, lut, mean3, std3)) return -2;
    if (images == 0) return 0;
    if (!in || !out || !xtab || !ytab) return -2;
    Crop g;
    fill(g, in, out, lut, H, W, dh, dw, epilogue, mean3, std3, 4);
    g.xtab = xtab; g.ytab = ytab; g.pad_h = pad_h; g.pad_w = pad_w;
    g.tiles_x = (dw + PX - 1) / PX;
    const long tiles = (long)g.tiles_x * ((dh + PY - 1) / PY);
    if (tiles > 0x7fffffffL || images > 0x7fffffffL / tiles) return -3;
    g.tiles = (int)tiles;
    const dim3 grid((unsigned)(images * tiles)), block(NT);
    hipStream_t st = (hipStream_t)stream;
    if (interp == MG_RESIZE_LINEAR) {
        if (channels == 1) hipLaunchKernelGGL((crop_padresize_kernel<1, false>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((crop_padresize_kernel<3, false>), grid, block, 0, st, g);
    } else {
        if (channels == 1) hipLaunchKernelGGL((crop_padresize_kernel<1, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((crop_padresize_kernel<3, true>), grid, block, 0, st, g);
    }
    MG_CHECK_LAUNCH();
    return 0;
}
