// Input geometry of the loaders on uint8 images (reference: maggie/dataloader/transforms.py:104-166, ResizeShort -> PaddingMultiplyBy, in front
//   of ToTensor / Normalize and the item assembly of him.py:157-176): a table-driven cv2.resize with the padding and the tensor stage fused into
//   the launch. Integer work and the IEEE divisions of pixel_norm.h: every result is bit-exact.
//
// Interpolation comes from host-built tables (maggie_amd/utils/geometry.py): INTER_LINEAR on 8-bit data is OpenCV's 11-bit fixed-point scheme,
//   per column and per row (offset, c0, c1), the same column table for every channel of an interleaved frame; INTER_NEAREST is one source
//   index per column and per row -- and so is any composition of index maps: the mask path folds the resize, the padding and the loaders'
//   nearest 1/8 down-scale into one table, and the full-size mask is never stored. A cell outside (dh, dw) is the padding and is written by
//   the same launch with the value a source pixel of 0 would have given: 0, (0 / 255 - mean) / std, or 0 / 255.
//
// Two kernels for the linear case, the same bits from both:
// resize_shared_kernel  the source rows of a 32 x 64 output tile are shared between its output rows (up-scaling, reductions up to ~2x: at most
//   68 of them). The horizontal pass runs once per needed source row into LDS, R >> 4 <= 32640 as uint16 per channel and column (26 KB for
//   three channels: six workgroups per CU), then the vertical pass reads two LDS rows per output pixel.
// resize_direct_kernel  larger reductions: every output pixel owns its four taps, nothing is shared and a tile's footprint does not fit in
//   LDS. A wave covers 256 consecutive pixels of ONE output row, four per lane, so its reads walk two contiguous source row segments and
//   its fp32 stores are 16 bytes per lane and channel plane. The nearest case is this kernel with one tap.
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"

namespace {

constexpr int NT = 256;
constexpr int TY = MG_RESIZE_TILE_ROWS, TX = MG_RESIZE_TILE_COLS, MAXR = MG_RESIZE_MAX_ROWS;
constexpr int DY = NT / 64, DX = 256;       // the direct tile: one wave per output row, four pixels per lane

struct Geo {
    const uint8_t* in;
    void* out;
    const int32_t* xtab;
    const int32_t* ytab;
    const int32_t* src_of_slot;
    int n_in, n_slots, H, W, dh, dw, Ho, Wo, epilogue, thresh, tiles_x, tiles, vec;
    float mean[3], std[3];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the source image of output image p (MG_RESIZE_SLOTS: through the slot table); nullptr: an empty slot
template <int C>
__device__ __forceinline__ const uint8_t* source_of(const Geo& g, long p) {
    long src = p;
    if (g.epilogue == MG_RESIZE_SLOTS) {
        const long f = p / g.n_slots;
        const int s = g.src_of_slot ? g.src_of_slot[p] : (int)(p - f * g.n_slots);
        if (s < 0 || s >= g.n_in) return nullptr;
        src = f * g.n_in + s;
    }
    return g.in + src * (long)g.H * g.W * C;
}

// four pixels (y, x0 .. x0 + 3) of output image p, x0 a multiple of 4, through the launch's epilogue
template <int C>
__device__ __forceinline__ void emit(const Geo& g, long p, int y, int x0, const int (&v)[4][C]) {
    const int n = min(4, g.Wo - x0);
    const bool vec = g.vec && n == 4;
    const long HWo = (long)g.Ho * g.Wo, pix = (long)y * g.Wo + x0;
    if (g.epilogue == MG_RESIZE_RAW) {
        uint8_t* o = (uint8_t*)g.out + (p * HWo + pix) * C;
        if (vec) {
#pragma unroll
            for (int w = 0; w < C; ++w) {
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const int e = 4 * w + k; word |= (uint32_t)(v[e / C][e % C] & 255) << (8 * k); }
                ((uint32_t*)o)[w] = word;
            }
        } else {
            for (int j = 0; j < n; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) o[j * C + c] = (uint8_t)v[j][c];
        }
    } else if (g.epilogue == MG_RESIZE_NORM) {
        if constexpr (C == 3) {
            float* o = (float*)g.out + p * 3 * HWo + pix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4 f;
                f.x = mg_norm_u8(v[0][c], g.mean[c], g.std[c]);
                f.y = mg_norm_u8(v[1][c], g.mean[c], g.std[c]);
                f.z = mg_norm_u8(v[2][c], g.mean[c], g.std[c]);
                f.w = mg_norm_u8(v[3][c], g.mean[c], g.std[c]);
                if (vec) *(float4*)(o + c * HWo) = f;
                else {
                    const float s[4] = {f.x, f.y, f.z, f.w};
                    for (int j = 0; j < n; ++j) o[c * HWo + j] = s[j];
                }
            }
        }
    } else {
        if constexpr (C == 1) {
            float* o = (float*)g.out + p * HWo + pix;
            float4 f;
            f.x = mg_scale_u8(v[0][0], g.thresh);
            f.y = mg_scale_u8(v[1][0], g.thresh);
            f.z = mg_scale_u8(v[2][0], g.thresh);
            f.w = mg_scale_u8(v[3][0], g.thresh);
            if (vec) *(float4*)o = f;
            else {
                const float s[4] = {f.x, f.y, f.z, f.w};
                for (int j = 0; j < n; ++j) o[j] = s[j];
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(NT) void resize_shared_kernel(Geo g) {
    __shared__ uint16_t rows[MAXR * TX * C];
    const long blk = blockIdx.x;
    const long p = blk / g.tiles;
    const int tile = (int)(blk - p * g.tiles);
    const int ty0 = (tile / g.tiles_x) * TY, tx0 = (tile % g.tiles_x) * TX;
    const int th = min(TY, g.Ho - ty0);
    const uint8_t* __restrict__ src = source_of<C>(g, p);
    const int vh = src ? min(ty0 + th, g.dh) - ty0 : 0;                      // rows of the tile inside the resized image
    int y_lo = 0, nrows = 0;
    if (vh > 0 && tx0 < g.dw) {
        // the source rows this tile reads (the offsets are non-decreasing); clamped to what LDS holds: the host picks this kernel only when
        // no tile needs more, and a table that breaks the promise reads wrong rows, never out of bounds
        y_lo = clampi(g.ytab[3 * ty0], 0, g.H - 1);
        const int y_hi = min(clampi(g.ytab[3 * (ty0 + vh - 1)], 0, g.H - 1) + 1, g.H - 1);
        nrows = clampi(y_hi - y_lo + 1, 1, MAXR);
        const int x = threadIdx.x & 63, gx = tx0 + x;                         // lane = column; a wave per source row
        if (gx < g.dw) {
            const int xo = clampi(g.xtab[3 * gx], 0, g.W - 1), x1 = min(xo + 1, g.W - 1);
            const int a0 = g.xtab[3 * gx + 1], a1 = g.xtab[3 * gx + 2];
            for (int r = threadIdx.x >> 6; r < nrows; r += NT / 64) {
                const uint8_t* __restrict__ row = src + (long)min(y_lo + r, g.H - 1) * g.W * C;
#pragma unroll
                for (int c = 0; c < C; ++c) rows[(r * TX + x) * C + c] = (uint16_t)(((int)row[xo * C + c] * a0 + (int)row[x1 * C + c] * a1) >> 4);
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < TY * (TX / 4); q += NT) {
        const int ry = q / (TX / 4), qx = (q % (TX / 4)) * 4;
        const int y = ty0 + ry, x0 = tx0 + qx;
        if (y >= g.Ho || x0 >= g.Wo) continue;
        int v[4][C] = {};
        if (nrows > 0 && y < g.dh) {
            const int yo = clampi(g.ytab[3 * y], 0, g.H - 1), b0 = g.ytab[3 * y + 1], b1 = g.ytab[3 * y + 2];
            const int r0 = clampi(yo - y_lo, 0, nrows - 1), r1 = clampi(min(yo + 1, g.H - 1) - y_lo, 0, nrows - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < g.dw) {
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        v[j][c] = (((b0 * (int)rows[(r0 * TX + qx + j) * C + c]) >> 16) + ((b1 * (int)rows[(r1 * TX + qx + j) * C + c]) >> 16) + 2) >> 2;
                }
        }
        emit<C>(g, p, y, x0, v);
    }
}

template <int C, bool NEAREST>
__global__ __launch_bounds__(NT) void resize_direct_kernel(Geo g) {
    const long blk = blockIdx.x;
    const long p = blk / g.tiles;
    const int tile = (int)(blk - p * g.tiles);
    const int y = (tile / g.tiles_x) * DY + (threadIdx.x >> 6), x0 = (tile % g.tiles_x) * DX + (threadIdx.x & 63) * 4;
    if (y >= g.Ho || x0 >= g.Wo) return;
    const uint8_t* __restrict__ src = source_of<C>(g, p);
    int v[4][C] = {};
    if (src && y < g.dh) {
        if constexpr (NEAREST) {
            const uint8_t* __restrict__ row = src + (long)clampi(g.ytab[y], 0, g.H - 1) * g.W * C;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < g.dw) {
                    const int sx = clampi(g.xtab[x0 + j], 0, g.W - 1);
#pragma unroll
                    for (int c = 0; c < C; ++c) v[j][c] = row[sx * C + c];
                }
        } else {
            const int yo = clampi(g.ytab[3 * y], 0, g.H - 1), b0 = g.ytab[3 * y + 1], b1 = g.ytab[3 * y + 2];
            const uint8_t* __restrict__ row0 = src + (long)yo * g.W * C;
            const uint8_t* __restrict__ row1 = src + (long)min(yo + 1, g.H - 1) * g.W * C;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < g.dw) {
                    const int gx = x0 + j;
                    const int xo = clampi(g.xtab[3 * gx], 0, g.W - 1), x1 = min(xo + 1, g.W - 1);
                    const int a0 = g.xtab[3 * gx + 1], a1 = g.xtab[3 * gx + 2];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int R0 = (int)row0[xo * C + c] * a0 + (int)row0[x1 * C + c] * a1;
                        const int R1 = (int)row1[xo * C + c] * a0 + (int)row1[x1 * C + c] * a1;
                        v[j][c] = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
                    }
                }
        }
    }
    emit<C>(g, p, y, x0, v);
}

}  // namespace

extern "C" int mg_resize_limits(int* tile_rows, int* tile_cols, int* max_rows) {
    if (!tile_rows || !tile_cols || !max_rows) return -2;
    *tile_rows = TY;
    *tile_cols = TX;
    *max_rows = MAXR;
    return 0;
}

extern "C" int mg_resize_u8(const uint8_t* in, void* out, const int32_t* xtab, const int32_t* ytab, const int32_t* src_of_slot, long images,
                            int n_in, int n_slots, int channels, int H, int W, int dh, int dw, int Ho, int Wo, int interp, int epilogue,
                            int regime, const float* mean3, const float* std3, int thresh, void* stream) {
    if (images < 0 || (channels != 1 && channels != 3) || H <= 0 || W <= 0 || dh <= 0 || dw <= 0 || Ho < dh || Wo < dw) return -2;
    if ((long)H * W * channels > 0x7fffffffL || (long)Ho * Wo * channels > 0x7fffffffL) return -2;
    if (interp != MG_RESIZE_LINEAR && interp != MG_RESIZE_NEAREST) return -2;
    if (regime != MG_RESIZE_SHARED_ROWS && regime != MG_RESIZE_DIRECT) return -2;
    if (epilogue != MG_RESIZE_RAW && epilogue != MG_RESIZE_NORM && epilogue != MG_RESIZE_SLOTS) return -2;
    if (epilogue == MG_RESIZE_NORM && (channels != 3 || !mean3 || !std3)) return -2;
    if (epilogue == MG_RESIZE_SLOTS && (channels != 1 || n_in <= 0 || n_slots <= 0 || (!src_of_slot && n_slots != n_in))) return -2;
    if (images == 0) return 0;
    if (!in || !out || !xtab || !ytab) return -2;
    Geo g;
    g.in = in; g.out = out; g.xtab = xtab; g.ytab = ytab; g.src_of_slot = src_of_slot;
    g.n_in = n_in; g.n_slots = n_slots; g.H = H; g.W = W; g.dh = dh; g.dw = dw; g.Ho = Ho; g.Wo = Wo; g.epilogue = epilogue; g.thresh = thresh;
    for (int c = 0; c < 3; ++c) { g.mean[c] = mean3 ? mean3[c] : 0.f; g.std[c] = std3 ? std3[c] : 1.f; }
    // packed stores: four pixels of a row start on a 4-byte (uint8) or 16-byte (fp32) boundary when the row length is a multiple of 4
    g.vec = (Wo % 4 == 0) && ((uintptr_t)out % 16 == 0);
    const bool shared = interp == MG_RESIZE_LINEAR && regime == MG_RESIZE_SHARED_ROWS;
    const int tw = shared ? TX : DX, th = shared ? TY : DY;
    g.tiles_x = (Wo + tw - 1) / tw;
    const long tiles = (long)g.tiles_x * ((Ho + th - 1) / th);
    const long outs = epilogue == MG_RESIZE_SLOTS ? images * n_slots : images;
    if (tiles > 0x7fffffffL || outs > 0x7fffffffL / tiles) return -3;
    g.tiles = (int)tiles;
    const dim3 grid((unsigned)(outs * tiles)), block(NT);
    hipStream_t st = (hipStream_t)stream;
    if (shared) {
        if (channels == 1) hipLaunchKernelGGL(resize_shared_kernel<1>, grid, block, 0, st, g);
        else hipLaunchKernelGGL(resize_shared_kernel<3>, grid, block, 0, st, g);
    } else if (interp == MG_RESIZE_LINEAR) {
        if (channels == 1) hipLaunchKernelGGL((resize_direct_kernel<1, false>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((resize_direct_kernel<3, false>), grid, block, 0, st, g);
    } else {
        if (channels == 1) hipLaunchKernelGGL((resize_direct_kernel<1, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((resize_direct_kernel<3, true>), grid, block, 0, st, g);
    }
    MG_CHECK_LAUNCH();
    return 0;
}
