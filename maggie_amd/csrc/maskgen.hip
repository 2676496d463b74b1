// Guidance-mask synthesis of the training loaders on uint8 planes (reference: maggie/dataloader/transforms.py:388-565,
//   GenMaskFromAlpha -> RandomBinarizedMask -> DownUpMask -> CutMask -> MaskDropout). Integer work throughout: every result is bit-exact.
//
// mask_morph_kernel  threshold + rectangular dilation / erosion (cv2.dilate / cv2.erode with np.ones((k, k)), anchor k / 2, k <= 31), up to two
//   passes. The image is binary after the threshold, so a 64 x 64 tile and its halo live in LDS as ONE BIT per pixel: a 128 x 128 region
//   (32 pixels of halo on every side: two passes reach at most 30) is 128 rows of two 64-bit words, 2 KB. The words come straight out of
//   `__ballot(v > t)` of a 64-pixel row segment. One pass is a k-wide OR along the row -- log2(k) shift-and-OR steps on the 128-bit row in
//   registers -- and a k-high OR down the column (k 8-byte LDS reads). Erosion is the same OR on the holes: erode(X) = inside & ~dilate(inside
//   & ~X), which also gives "pixels outside the image take no part" for both operators (outside bits are 0 in X and in the holes), before
//   and between the passes. Zeros shifted in at the edge of the region make a fringe of a / b bits inexact per pass, like the shrinking
//   region of morph.hip; the tile is 32 bits away from it. Rows and words the plane's own (k_d, k_e, order) cannot reach are not loaded.
// mask_downup_kernel cv2.resize(INTER_LINEAR) down by r and back up, then > 127, fused: a workgroup computes the patch of the small image its
//   64 x 64 output tile reads into LDS (four source taps per small pixel, through host-built (offset, c0, c1) tables of OpenCV's 11-bit
//   fixed-point coefficients), then up-samples from there. Table-driven for every size.
// mask_cut_kernel    rectangle copy inside a plane or from another plane (a swap is two entries), out of place.
// mask_stats_kernel / mask_drop_kernel  count and bounding box of the non-zero pixels; zero a rectangle anchored at the idx-th non-zero
//   pixel in raster order (row counts by ballot, a running sum over the rows, a ballot search within the row).
#include "common.h"
#include "../../include/maggie_hip.h"

namespace {

constexpr int MT = 64;             // tile side
constexpr int MH = 32;             // halo on every side of the tile inside the LDS region
constexpr int MR = MT + 2 * MH;    // region side: 128 rows of two 64-bit words
constexpr int NT = 256;
constexpr int MAXK = MG_MASK_MAX_K;

struct U128 { uint64_t lo, hi; };  // bit i of lo: column i of the region; bit i of hi: column 64 + i

__device__ __forceinline__ U128 shr(U128 v, int s) {       // r[x] = v[x + s], 0 <= s < 64
    U128 r;
    r.lo = (v.lo >> s) | (s ? v.hi << (64 - s) : 0ull);
    r.hi = v.hi >> s;
    return r;
}
__device__ __forceinline__ U128 shl(U128 v, int s) {       // r[x] = v[x - s], 0 <= s < 64
    U128 r;
    r.hi = (v.hi << s) | (s ? v.lo >> (64 - s) : 0ull);
    r.lo = v.lo << s;
    return r;
}
// r[x] = OR over 0 <= j < k of v[x + j - a]: a forward window of k bits by doubling, then moved back by the anchor
__device__ __forceinline__ U128 window_or(U128 v, int k, int a) {
    int w = 1;
    while (2 * w <= k) { const U128 t = shr(v, w); v.lo |= t.lo; v.hi |= t.hi; w *= 2; }
    if (w < k) { const U128 t = shr(v, k - w); v.lo |= t.lo; v.hi |= t.hi; }
    return shl(v, a);
}
// bits of the 64 columns starting at image column x0 that lie inside [0, W)
__device__ __forceinline__ uint64_t col_mask(int x0, int W) {
    const int lo = max(0, -x0), hi = min(64, W - x0);
    if (hi <= lo) return 0ull;
    const uint64_t upto_hi = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    return upto_hi & ~((1ull << lo) - 1ull);
}

// one rectangular pass over the whole region, cur -> cur (through tmp); thread (r, w) owns word w of row r
__device__ __forceinline__ void rect_pass(uint64_t* cur, uint64_t* tmp, int k, bool erode, int r, int w, U128 in) {
    const int a = k / 2;
    U128 v = {cur[2 * r], cur[2 * r + 1]};
    if (erode) { v.lo = in.lo & ~v.lo; v.hi = in.hi & ~v.hi; }             // the holes
    const U128 h = window_or(v, k, a);
    tmp[2 * r + w] = w ? h.hi : h.lo;
    __syncthreads();
    uint64_t acc = 0ull;
    const int i0 = max(0, a - r), i1 = min(k, MR + a - r);                 // rows r + i - a inside the region
    for (int i = i0; i < i1; ++i) acc |= tmp[2 * (r + i - a) + w];
    const uint64_t mine = w ? in.hi : in.lo;
    cur[2 * r + w] = erode ? (mine & ~acc) : (mine & acc);
    __syncthreads();
}

__global__ __launch_bounds__(NT) void mask_morph_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                        const int32_t* __restrict__ params, int H, int W, int tiles_x, int tiles) {
    __shared__ uint64_t cur[MR * 2], tmp[MR * 2];
    const long blk = blockIdx.x;
    const long p = blk / tiles;
    const int tile = (int)(blk - p * tiles);
    const int ty0 = (tile / tiles_x) * MT, tx0 = (tile % tiles_x) * MT;
    const int oy = ty0 - MH, ox = tx0 - MH;
    const long HW = (long)H * W;
    const uint8_t* __restrict__ plane = in + p * HW;

    // this plane's draws, clamped to what the region holds (the host raises before a launch; a table rewritten between graph replays is
    // clamped here, never out of bounds)
    const int thr = params[4 * p];
    const int kd = min(max(params[4 * p + 1], 1), MAXK), ke = min(max(params[4 * p + 2], 1), MAXK);
    const int order = params[4 * p + 3];
    int k1 = 0, k2 = 0;                                                     // 0: no pass
    bool e1 = false, e2 = false;
    if (order == MG_MASK_DILATE_ERODE) { k1 = kd; k2 = ke; e2 = true; }
    else if (order == MG_MASK_ERODE_DILATE) { k1 = ke; e1 = true; k2 = kd; }
    else if (order == MG_MASK_DILATE) { k1 = kd; }
    else if (order == MG_MASK_ERODE) { k1 = ke; e1 = true; }
    const int U = k1 / 2 + k2 / 2;                                          // reach up / left
    const int D = (k1 ? k1 - 1 - k1 / 2 : 0) + (k2 ? k2 - 1 - k2 / 2 : 0);  // reach down / right

    // ---- load: one ballot per 64-pixel row segment; 256 segments, 64 per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r_lo = MH - U, r_hi = MH + MT + D;                            // region rows / columns that can reach the tile
    constexpr int NW = NT / 64, LD = 4;                                     // four loads in flight per lane
    for (int it = wave; it < MR * 2; it += NW * LD) {
        int v[LD];
#pragma unroll
        for (int u = 0; u < LD; ++u) {
            const int item = it + u * NW, r = item >> 1, c = 64 * (item & 1) + lane;
            const int y = oy + r, x = ox + c;
            const bool ok = r >= r_lo && r < r_hi && c >= r_lo && c < r_hi && y >= 0 && y < H && x >= 0 && x < W;
            v[u] = ok ? (int)plane[(long)y * W + x] : INT32_MIN;            // below every threshold
        }
#pragma unroll
        for (int u = 0; u < LD; ++u) {
            const uint64_t word = __ballot(v[u] > thr);
            if (lane == 0) cur[it + u * NW] = word;
        }
    }
    __syncthreads();

    const int r = threadIdx.x >> 1, w = threadIdx.x & 1;
    U128 inside = {0ull, 0ull};
    if (oy + r >= 0 && oy + r < H) { inside.lo = col_mask(ox, W); inside.hi = col_mask(ox + 64, W); }
    if (k1 > 1) rect_pass(cur, tmp, k1, e1, r, w, inside);                  // k = 1 is the identity
    if (k2 > 1) rect_pass(cur, tmp, k2, e2, r, w, inside);

    // ---- store the tile: lane = column, 16 rows per wave
    const int c = MH + lane;
    for (int ry = wave; ry < MT; ry += NT / 64) {
        const int y = ty0 + ry, x = tx0 + lane;
        if (y < H && x < W) out[p * HW + (long)y * W + x] = ((cur[2 * (MH + ry) + (c >> 6)] >> (c & 63)) & 1ull) ? 255 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int PM = MG_MASK_MAX_PATCH;       // side of the small-image patch of one tile

// 8-bit bilinear resize of OpenCV, one pixel: horizontal taps into int32, then the vertical pass
__device__ __forceinline__ int bilinear_fixed(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int R0 = s00 * a0 + s01 * a1, R1 = s10 * a0 + s11 * a1;
    return (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
}

__global__ __launch_bounds__(NT) void mask_downup_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                         const int32_t* __restrict__ apply, const int32_t* __restrict__ tab, int dh, int dw,
                                                         int H, int W, int tiles_x, int tiles) {
    __shared__ uint8_t small[PM * PM];
    const long blk = blockIdx.x;
    const long p = blk / tiles;
    const int tile = (int)(blk - p * tiles);
    const int ty0 = (tile / tiles_x) * MT, tx0 = (tile % tiles_x) * MT;
    const int th = min(MT, H - ty0), tw = min(MT, W - tx0);
    const long HW = (long)H * W;
    const uint8_t* __restrict__ plane = in + p * HW;
    uint8_t* __restrict__ oplane = out + p * HW;
    if (apply[p] == 0) {                                                    // this plane passes through
        for (int i = threadIdx.x; i < th * MT; i += NT) {
            const int ry = i >> 6, rx = i & 63;
            if (rx < tw) oplane[(long)(ty0 + ry) * W + tx0 + rx] = plane[(long)(ty0 + ry) * W + tx0 + rx];
        }
        return;
    }
    const int32_t* __restrict__ dnx = tab;                                  // [dw][3] offset, c0, c1: small column -> source columns
    const int32_t* __restrict__ dny = dnx + 3 * dw;                         // [dh][3]
    const int32_t* __restrict__ upx = dny + 3 * dh;                         // [W][3]: output column -> small columns
    const int32_t* __restrict__ upy = upx + 3 * W;                          // [H][3]
    // the patch of the small image this tile reads (the offsets are non-decreasing)
    const int sy_lo = min(max(upy[3 * ty0], 0), dh - 1), sx_lo = min(max(upx[3 * tx0], 0), dw - 1);
    const int sy_hi = min(upy[3 * (ty0 + th - 1)] + 1, dh - 1), sx_hi = min(upx[3 * (tx0 + tw - 1)] + 1, dw - 1);
    const int ph = min(max(sy_hi - sy_lo + 1, 1), PM), pw = min(max(sx_hi - sx_lo + 1, 1), PM);
    for (int i = threadIdx.x; i < ph * pw; i += NT) {
        const int py = i / pw, px = i - py * pw;
        const int32_t* ty = dny + 3 * (sy_lo + py);
        const int32_t* tx = dnx + 3 * (sx_lo + px);
        const int y0 = min(max(ty[0], 0), H - 1), y1 = min(y0 + 1, H - 1);
        const int x0 = min(max(tx[0], 0), W - 1), x1 = min(x0 + 1, W - 1);
        const uint8_t* r0 = plane + (long)y0 * W;
        const uint8_t* r1 = plane + (long)y1 * W;
        small[py * PM + px] = (uint8_t)bilinear_fixed(r0[x0], r0[x1], r1[x0], r1[x1], tx[1], tx[2], ty[1], ty[2]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < th * MT; i += NT) {
        const int ry = i >> 6, rx = i & 63;
        if (rx >= tw) continue;
        const int32_t* ty = upy + 3 * (ty0 + ry);
        const int32_t* tx = upx + 3 * (tx0 + rx);
        const int y0 = min(max(ty[0] - sy_lo, 0), ph - 1), y1 = min(y0 + 1, ph - 1);       // the second tap is clamped at the small image's edge,
        const int x0 = min(max(tx[0] - sx_lo, 0), pw - 1), x1 = min(x0 + 1, pw - 1);       // which is the patch's edge there
        const int v = bilinear_fixed(small[y0 * PM + x0], small[y0 * PM + x1], small[y1 * PM + x0], small[y1 * PM + x1], tx[1], tx[2], ty[1], ty[2]);
        oplane[(long)(ty0 + ry) * W + tx0 + rx] = v > 127 ? 255 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int CUT_PX = 16;           // pixels per thread

__global__ __launch_bounds__(NT) void mask_cut_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ rects,
                                                      long P, int H, int W, int chunks) {
    const long blk = blockIdx.x;
    const long p = blk / chunks;
    const int chunk = (int)(blk - p * chunks);
    const long HW = (long)H * W;
    const int32_t* rc = rects + 8 * p;
    const int sp = rc[0], dr = rc[1], dc = rc[2], sr = rc[3], sc = rc[4], h = rc[5], w = rc[6];
    // an entry that is not a rectangle pair inside the planes leaves the plane untouched
    const bool on = sp >= 0 && sp < P && h > 0 && w > 0 && dr >= 0 && dc >= 0 && sr >= 0 && sc >= 0 && dr <= H - h && sr <= H - h && dc <= W - w &&
                    sc <= W - w;
    const uint8_t* __restrict__ mine = in + p * HW;
    const uint8_t* __restrict__ other = in + (on ? (long)sp : p) * HW;
    const long base = (long)chunk * (NT * CUT_PX) + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < CUT_PX; ++j) {
        const long i = base + (long)j * NT;
        if (i >= HW) break;
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        uint8_t v = mine[i];
        if (on && y >= dr && y < dr + h && x >= dc && x < dc + w) v = other[(long)(y - dr + sr) * W + (x - dc + sc)];
        out[p * HW + i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int ST = 1024;             // threads of the per-plane kernels: 16 waves, one row each per trip

__global__ __launch_bounds__(ST) void mask_stats_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ stats, int H, int W) {
    __shared__ int s[5];
    const long p = blockIdx.x;
    const uint8_t* __restrict__ plane = in + p * (long)H * W;
    if (threadIdx.x == 0) { s[0] = 0; s[1] = W; s[2] = -1; s[3] = H; s[4] = -1; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0, xmin = W, xmax = -1, ymin = H, ymax = -1;
    for (int y = wave; y < H; y += ST / 64)
        for (int x = lane; x < W; x += 64)
            if (plane[(long)y * W + x]) { ++cnt; xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); }
    if (cnt) {                                                             // integer LDS atomics: the result does not depend on order
        atomicAdd(&s[0], cnt); atomicMin(&s[1], xmin); atomicMax(&s[2], xmax); atomicMin(&s[3], ymin); atomicMax(&s[4], ymax);
    }
    __syncthreads();
    if (threadIdx.x < 5) stats[5 * p + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(ST) void mask_drop_kernel(uint8_t* __restrict__ planes, const int32_t* __restrict__ sel, const int32_t* __restrict__ stats,
                                                       long P, int H, int W) {
    __shared__ int s_cnt[ST / 64];
    __shared__ int s_x;
    const int32_t* e = sel + 4 * blockIdx.x;
    const int p = e[0], idx = e[1], ph = e[2], pw = e[3];
    if (p < 0 || p >= P || idx < 0 || ph <= 0 || pw <= 0) return;           // a skipped entry
    uint8_t* __restrict__ plane = planes + (long)p * H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_x = -1;
    // the row of the idx-th non-zero pixel: counts of 16 rows at a time, added in row order
    int base = 0, row = -1, row_base = 0;
    for (int y0 = 0; y0 < H && row < 0; y0 += ST / 64) {
        const int y = y0 + wave;
        int n = 0;
        if (y < H)
            for (int x0 = 0; x0 < W; x0 += 64) n += __popcll(__ballot(x0 + lane < W && plane[(long)y * W + x0 + lane] != 0));
        if (lane == 0) s_cnt[wave] = n;
        __syncthreads();
        for (int j = 0; j < ST / 64; ++j) {
            const int c = s_cnt[j];
            if (row < 0 && idx < base + c) { row = y0 + j; row_base = base; }
            base += c;
        }
        __syncthreads();
    }
    if (row < 0) return;                                                   // idx is not below the plane's count
    if (wave == 0) {                                                       // the (idx - row_base)-th non-zero pixel of that row
        int rem = idx - row_base;
        for (int x0 = 0; x0 < W; x0 += 64) {
            const bool bit = x0 + lane < W && plane[(long)row * W + x0 + lane] != 0;
            const uint64_t m = __ballot(bit);
            const int n = __popcll(m);
            if (rem < n) {
                if (bit && __popcll(m & ((1ull << lane) - 1ull)) == rem) s_x = x0 + lane;
                break;
            }
            rem -= n;
        }
    }
    __syncthreads();
    if (s_x < 0) return;
    const int xmax = stats[5 * p + 2], ymax = stats[5 * p + 4];
    const int x = max(min(s_x, xmax - pw), 0), y = max(min(row, ymax - ph), 0);         // transforms.py:561-562
    const int h = min(ph, H - y), w = min(pw, W - x);
    for (int i = threadIdx.x; i < h * w; i += ST) plane[(long)(y + i / w) * W + x + i % w] = 0;
}

inline bool bad_shape(long planes, int H, int W) { return planes < 0 || H < 0 || W < 0 || (long)H * W > 0x7fffffffL; }

}  // namespace

extern "C" int mg_mask_morph(const uint8_t* in, uint8_t* out, const int32_t* params, long planes, int H, int W, void* stream) {
    if (bad_shape(planes, H, W) || !params) return -2;
    if (planes == 0 || H == 0 || W == 0) return 0;
    const int tiles_x = (W + MT - 1) / MT, tiles = tiles_x * ((H + MT - 1) / MT);
    const long blocks = planes * tiles;
    if (blocks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(mask_morph_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, in, out, params, H, W, tiles_x, tiles);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_mask_downup(const uint8_t* in, uint8_t* out, const int32_t* apply, const int32_t* tab, int dh, int dw, long planes, int H, int W,
                              void* stream) {
    if (bad_shape(planes, H, W) || !apply || !tab || dh <= 0 || dw <= 0) return -2;
    if (planes == 0 || H == 0 || W == 0) return 0;
    const int tiles_x = (W + MT - 1) / MT, tiles = tiles_x * ((H + MT - 1) / MT);
    const long blocks = planes * tiles;
    if (blocks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(mask_downup_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, in, out, apply, tab, dh, dw, H, W, tiles_x, tiles);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_mask_cut(const uint8_t* in, uint8_t* out, const int32_t* rects, long planes, int H, int W, void* stream) {
    if (bad_shape(planes, H, W) || !rects || in == out) return -2;
    if (planes == 0 || H == 0 || W == 0) return 0;
    const long per = (long)NT * CUT_PX;
    const int chunks = (int)(((long)H * W + per - 1) / per);
    const long blocks = planes * chunks;
    if (blocks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(mask_cut_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, in, out, rects, planes, H, W, chunks);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_mask_stats(const uint8_t* in, int32_t* stats, long planes, int H, int W, void* stream) {
    if (bad_shape(planes, H, W) || !stats) return -2;
    if (planes == 0) return 0;
    if (planes > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)planes), dim3(ST), 0, (hipStream_t)stream, in, stats, H, W);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_mask_drop(uint8_t* planes_u8, const int32_t* sel, const int32_t* stats, int n, long planes, int H, int W, void* stream) {
    if (bad_shape(planes, H, W) || n < 0 || !sel || !stats) return -2;
    if (n == 0 || planes == 0 || H == 0 || W == 0) return 0;
    hipLaunchKernelGGL(mask_drop_kernel, dim3((unsigned)n), dim3(ST), 0, (hipStream_t)stream, planes_u8, sel, stats, planes, H, W);
    MG_CHECK_LAUNCH();
    return 0;
}
