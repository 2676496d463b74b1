// RandomAffine of the loaders on uint8 images (reference: maggie/dataloader/transforms.py:926-963 with random_transform, apply_transforms_cv and
//   channel_shift of dataloader/utils.py:61-221; wired in him.py:49 and vim.py:55). The draws, the matrix, its inversion and the four fixed-point
//   tables are the host's (maggie_amd/utils/affine.py); what runs here is cv2.warpAffine's classic uint8 path from those tables and the float64
//   channel shift with ToTensor + Normalize. The warp is integer work only: no device float decides a pixel. Every result is bit-exact.
//
// A table buffer is int32 [adelta W | bdelta W | X0 H | Y0 H] (AB_BITS = 10; X0 / Y0 carry the interpolation's round_delta). The kernels add
//   with wrap-around, so a buffer may hold anything: every index derived from it is range-tested before it addresses memory.
//
// affine_planes_kernel   INTER_NEAREST for the alphas: a lane owns 4 consecutive output pixels of a row, computes their four source indices
//   once (sx = (X0[y] + adelta[x]) >> 10, sy likewise, -1 when the tap is outside) and walks the planes of its group with them; 4-byte stores,
//   per element on ragged widths.
// affine_frames_kernel   INTER_LINEAR for the 3-channel frames: X = (X0[y] + adelta[x]) >> 5, sx = X >> 5, fx = X & 31, the four integer
//   weights 32 * (32 - fx) * (32 - fy) ... of sum 32768, (sum + 16384) >> 15, each tap outside the image 0 on its own. A workgroup owns a
//   32 x 64 output tile, a lane 4 consecutive pixels of a row in each half of it. STAGED: the tile's source box, taken from the table values at
//   the tile's corners and cut to the image, is copied to LDS with 16-byte row loads when it fits MG_AFFINE_BOX_BYTES, and taps inside it are
//   read from LDS; a tap outside the box (tables that are not monotone) or a box that does not fit reads global memory, so both regimes give
//   the same bits for any table. DIRECT: four global taps per pixel. Each frame's min and max over its pixels and channels are left in two
//   device words by integer atomics (order-free), which affine_init_kernel sets on the same stream first.
// affine_shift_kernel    channel_shift + ToTensor + Normalize: f = (float)clamp((double)v + intensity, mn, mx), then the two IEEE divisions of
//   pixel_norm.h; a lane owns 4 pixels, reads 12 bytes and writes one float4 per channel plane.
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"

namespace {

constexpr int NT = 256;
constexpr int TR = MG_AFFINE_TILE_ROWS, TC = MG_AFFINE_TILE_COLS;          // the frames' output tile
constexpr int BOX = MG_AFFINE_BOX_BYTES;
constexpr int PG = 8;                                                    // planes per workgroup of the nearest warp (at least)
static_assert(TC == 64 && TR == 32 && NT == 256, "a lane owns 4 pixels of a row: 16 lanes per row, 16 rows per pass, two passes");

// the sum of two table entries with wrap-around (a buffer rewritten on the device may hold anything)
__device__ __forceinline__ int wsum(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

__global__ void affine_init_kernel(int32_t* __restrict__ mm, int frames) {
    for (int t = threadIdx.x; t < frames; t += blockDim.x) { mm[2 * t] = 255; mm[2 * t + 1] = 0; }
}

// ---- INTER_NEAREST, planes ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void affine_planes_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ tab,
                                                           long planes, int per, int H, int W, int groups, long units, int vec) {
    const long u = (long)blockIdx.x * NT + threadIdx.x;
    if (u >= units) return;
    const int y = (int)(u / groups), x0 = (int)(u - (long)y * groups) * 4, n = min(4, W - x0);
    const int32_t *adelta = tab, *bdelta = tab + W, *X0 = tab + 2 * W, *Y0 = X0 + H;
    const int Xy = X0[y], Yy = Y0[y];
    int idx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        idx[j] = -1;
        if (j < n) {
            const int sx = wsum(Xy, adelta[x0 + j]) >> 10, sy = wsum(Yy, bdelta[x0 + j]) >> 10;       // arithmetic shifts: negative coordinates floor
            if (sx >= 0 && sx < W && sy >= 0 && sy < H) idx[j] = sy * W + sx;
        }
    }
    const long HW = (long)H * W, p0 = (long)blockIdx.y * per, p1 = min(planes, p0 + per);
    const long o = (long)y * W + x0;
    for (long p = p0; p < p1; ++p) {
        const uint8_t* __restrict__ src = in + p * HW;
        uint8_t* __restrict__ dst = out + p * HW + o;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = idx[j] >= 0 ? (uint32_t)src[idx[j]] : 0u;
        if (vec) {
            *(uint32_t*)dst = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) dst[j] = (uint8_t)v[j];
        }
    }
}

// ---- INTER_LINEAR, 3-channel frames --------------------------------------------------------------------------------------------------------------
template <bool STAGED>
__global__ __launch_bounds__(NT) void affine_frames_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ tab,
                                                           int32_t* __restrict__ mm, int H, int W, int tiles_x, int tiles, int vec) {
    __shared__ uint4 s_box[STAGED ? BOX / 16 : 1];
    __shared__ int s_mm[2];
    const long blk = blockIdx.x;
    const long t = blk / tiles;
    const int tile = (int)(blk - t * tiles);
    const int ty0 = (tile / tiles_x) * TR, tx0 = (tile % tiles_x) * TC;
    const int ty1 = min(ty0 + TR, H) - 1, tx1 = min(tx0 + TC, W) - 1;         // the tile's last row and column
    const int32_t *adelta = tab, *bdelta = tab + W, *X0 = tab + 2 * W, *Y0 = X0 + H;
    const long HW3 = (long)H * W * 3;
    const uint8_t* __restrict__ src = in + t * HW3;
    if (threadIdx.x == 0) { s_mm[0] = 255; s_mm[1] = 0; }

    // the source box of the tile: the taps of its four corners (sx .. sx + 1, sy .. sy + 1), cut to the image
    int bx0 = 0, by0 = 0, bw = 0, bh = 0, pitch = 0;
    const uint8_t* s_bytes = (const uint8_t*)s_box;
    if constexpr (STAGED) {
        const int xa = X0[ty0], xb = X0[ty1], da = adelta[tx0], db = adelta[tx1];
        const int ya = Y0[ty0], yb = Y0[ty1], ea = bdelta[tx0], eb = bdelta[tx1];
        const int sx[4] = {wsum(xa, da) >> 10, wsum(xa, db) >> 10, wsum(xb, da) >> 10, wsum(xb, db) >> 10};
        const int sy[4] = {wsum(ya, ea) >> 10, wsum(ya, eb) >> 10, wsum(yb, ea) >> 10, wsum(yb, eb) >> 10};
        bx0 = max(min(min(sx[0], sx[1]), min(sx[2], sx[3])), 0);
        by0 = max(min(min(sy[0], sy[1]), min(sy[2], sy[3])), 0);
        const int bx1 = min(max(max(sx[0], sx[1]), max(sx[2], sx[3])), W - 2) + 1;       // |sx| < 2^21: no overflow
        const int by1 = min(max(max(sy[0], sy[1]), max(sy[2], sy[3])), H - 2) + 1;
        bw = bx1 - bx0 + 1; bh = by1 - by0 + 1;
        if (bw <= 0 || bh <= 0 || bw > BOX / 3 || bh > BOX) { bw = 0; bh = 0; }           // empty, or too large to stage
        pitch = (bw * 3 + 15) & ~15;
        if ((long)bh * pitch > BOX) { bw = 0; bh = 0; }
        // bx0 >= 0, bx0 + bw - 1 <= W - 1, by0 >= 0, by0 + bh - 1 <= H - 1: the box lies inside the frame
        const int chunks = pitch >> 4;
        for (int k = threadIdx.x; k < bh * chunks; k += NT) {
            const int r = k / chunks, c16 = (k - r * chunks) * 16;
            const long g = ((long)(by0 + r) * W + bx0) * 3 + c16;                       // < HW3
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (g + 16 <= HW3) {
                __builtin_memcpy(&v, src + g, 16);                                       // past the box's row end it reads pixels nobody looks at
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};                                        // the frame's last bytes: one at a time
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (g + j < HW3) w[j >> 2] |= (uint32_t)src[g + j] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            s_box[r * chunks + (c16 >> 4)] = v;                                          // r * pitch + c16 bytes: inside BOX
        }
    }
    __syncthreads();

    // channel c of the tap at (sy, sx): 0 outside the image, LDS inside the staged box, global memory otherwise
    auto tap3 = [&](int sy, int sx, int (&v)[3]) {
        v[0] = v[1] = v[2] = 0;
        if (sx < 0 || sx >= W || sy < 0 || sy >= H) return;
        if constexpr (STAGED) {
            const int lx = sx - bx0, ly = sy - by0;
            if (lx >= 0 && lx < bw && ly >= 0 && ly < bh) {
                const uint8_t* p = s_bytes + ly * pitch + lx * 3;
                v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
                return;
            }
        }
        const uint8_t* p = src + ((long)sy * W + sx) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    };

    int mn = 255, mx = 0;
    const int lx0 = tx0 + (threadIdx.x & 15) * 4;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int y = ty0 + pass * 16 + (threadIdx.x >> 4);
        if (y >= H || lx0 >= W) continue;
        const int n = min(4, W - lx0);
        const int Xy = X0[y], Yy = Y0[y];
        uint32_t px[4][3] = {};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) continue;
            const int X = wsum(Xy, adelta[lx0 + j]) >> 5, Y = wsum(Yy, bdelta[lx0 + j]) >> 5;
            const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
            const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
            int a[3], b[3], c[3], d[3];
            tap3(sy, sx, a);
            // sx + 1 and sy + 1 cannot overflow: |sx|, |sy| < 2^21
            tap3(sy, sx + 1, b);
            tap3(sy + 1, sx, c);
            tap3(sy + 1, sx + 1, d);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int v = (w00 * a[ch] + w01 * b[ch] + w10 * c[ch] + w11 * d[ch] + 16384) >> 15;       // <= 255: the weights sum to 32768
                px[j][ch] = (uint32_t)v;
                mn = min(mn, v); mx = max(mx, v);
            }
        }
        uint8_t* __restrict__ dst = out + t * HW3 + ((long)y * W + lx0) * 3;
        if (vec && n == 4) {
            uint32_t w[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                w[q] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const int e = 4 * q + k; w[q] |= px[e / 3][e % 3] << (8 * k); }
            }
            ((uint32_t*)dst)[0] = w[0]; ((uint32_t*)dst)[1] = w[1]; ((uint32_t*)dst)[2] = w[2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) { dst[3 * j] = (uint8_t)px[j][0]; dst[3 * j + 1] = (uint8_t)px[j][1]; dst[3 * j + 2] = (uint8_t)px[j][2]; }
        }
    }
    if (mn <= mx) { atomicMin(&s_mm[0], mn); atomicMax(&s_mm[1], mx); }      // integer atomics: the result does not depend on order
    __syncthreads();
    if (threadIdx.x == 0 && s_mm[0] <= s_mm[1]) { atomicMin(&mm[2 * t], s_mm[0]); atomicMax(&mm[2 * t + 1], s_mm[1]); }
}

// ---- channel shift + ToTensor + Normalize --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void affine_shift_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, const int32_t* __restrict__ mm,
                                                          const double* __restrict__ intensity, long HW, long groups, long units, int vec,
                                                          float m0, float m1, float m2, float s0, float s1, float s2) {
    const long u = (long)blockIdx.x * NT + threadIdx.x;
    if (u >= units) return;
    const long t = u / groups, p0 = (u - t * groups) * 4;
    const int n = (int)min(4L, HW - p0);
    const double shift = *intensity, lo = (double)mm[2 * t], hi = (double)mm[2 * t + 1];
    const uint8_t* __restrict__ src = in + (t * HW + p0) * 3;
    uint32_t b[12] = {};
    if (vec) {
        const uint32_t w[3] = {((const uint32_t*)src)[0], ((const uint32_t*)src)[1], ((const uint32_t*)src)[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) b[k] = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) b[k] = src[k];
    }
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    float* __restrict__ dst = out + t * 3 * HW + p0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // np.clip(v + intensity, min, max) in float64, `.float()`, then Normalize.norm in fp32
            const double x = fmin(fmax((double)b[3 * j + c] + shift, lo), hi);
            f[j] = mg_norm_f32((float)x, mean[c], std[c]);
        }
        if (vec) {
            *(float4*)(dst + c * HW) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) dst[c * HW + j] = f[j];
        }
    }
}

bool bad_size(long images, int H, int W) {
    return images < 0 || H <= 0 || W <= 0 || H > MG_AFFINE_MAX_SIDE || W > MG_AFFINE_MAX_SIDE;       // H * W * 3 < 2^32 / 1.3: fits a long, and sy * W + sx an int
}

}  // namespace

extern "C" int mg_affine_limits(int* tile_rows, int* tile_cols, int* box_bytes, int* max_side) {
    if (!tile_rows || !tile_cols || !box_bytes || !max_side) return -2;
    *tile_rows = TR; *tile_cols = TC; *box_bytes = BOX; *max_side = MG_AFFINE_MAX_SIDE;
    return 0;
}

extern "C" int mg_affine_warp_planes(const uint8_t* in, uint8_t* out, const int32_t* tab, long planes, int H, int W, void* stream) {
    if (bad_size(planes, H, W)) return -2;
    if (planes == 0) return 0;
    if (!in || !out || !tab || in == out) return -2;
    const int groups = (W + 3) / 4;
    const long units = (long)H * groups, blocks = (units + NT - 1) / NT;
    long per = PG;
    if ((planes + per - 1) / per > 65535) per = (planes + 65534) / 65535;
    if (blocks > 0x7fffffffL || per > 0x7fffffffL) return -3;
    const int vec = (W % 4 == 0) && ((uintptr_t)out % 4 == 0);
    hipLaunchKernelGGL(affine_planes_kernel, dim3((unsigned)blocks, (unsigned)((planes + per - 1) / per)), dim3(NT), 0, (hipStream_t)stream, in, out,
                       tab, planes, (int)per, H, W, groups, units, vec);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_affine_warp_frames(const uint8_t* in, uint8_t* out, const int32_t* tab, int32_t* minmax, long frames, int H, int W, int regime,
                                     void* stream) {
    if (bad_size(frames, H, W) || (regime != MG_AFFINE_STAGED && regime != MG_AFFINE_DIRECT)) return -2;
    if (frames == 0) return 0;
    if (!in || !out || !tab || !minmax || in == out) return -2;
    const int tiles_x = (W + TC - 1) / TC;
    const long tiles = (long)tiles_x * ((H + TR - 1) / TR);
    if (frames > 0x7fffffffL / tiles) return -3;
    const int vec = (W % 4 == 0) && ((uintptr_t)out % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(affine_init_kernel, dim3(1), dim3(NT), 0, st, minmax, (int)frames);
    MG_CHECK_LAUNCH();
    const dim3 grid((unsigned)(frames * tiles)), block(NT);
    if (regime == MG_AFFINE_STAGED)
        hipLaunchKernelGGL(affine_frames_kernel<true>, grid, block, 0, st, in, out, tab, minmax, H, W, tiles_x, (int)tiles, vec);
    else
        hipLaunchKernelGGL(affine_frames_kernel<false>, grid, block, 0, st, in, out, tab, minmax, H, W, tiles_x, (int)tiles, vec);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_affine_shift_normalize(const uint8_t* in, float* out, const int32_t* minmax, const double* intensity, long frames, int H, int W,
                                         const float* mean3, const float* std3, void* stream) {
    if (bad_size(frames, H, W) || !mean3 || !std3) return -2;
    if (frames == 0) return 0;
    if (!in || !out || !minmax || !intensity) return -2;
    const long HW = (long)H * W, groups = (HW + 3) / 4;
    if (frames > 0x7fffffffffL / groups) return -3;
    const long units = frames * groups, blocks = (units + NT - 1) / NT;
    if (blocks > 0x7fffffffL) return -3;
    const int vec = (HW % 4 == 0) && ((uintptr_t)in % 4 == 0) && ((uintptr_t)out % 16 == 0);
    hipLaunchKernelGGL(affine_shift_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, in, out, minmax, intensity, HW, groups, units,
                       vec, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MG_CHECK_LAUNCH();
    return 0;
}
