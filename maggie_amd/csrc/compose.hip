// Compositing of the multi-instance training images and clips on uint8 data (reference: tools/synthesize_image_him.py:33-111,
//   tools/synthesize_video_him.py:157-184): Pillow's Image.resize (bicubic / bilinear) and Image.paste, the occlusion bookkeeping of the
//   accept / reject loop and the alpha bounding box. Integer work, or IEEE sub / mul without contraction: every result is exact
//   (DESIGN.md section 24).
//
// Resize. A pass of Pillow's resampler is, per output index i with the table row (lo, n, w_0 .. w_{n-1}) the host built,
//     out[i] = clip8((2^21 + sum_k in[lo + k] * w_k) >> 22)
//   horizontal pass first, then vertical, a BYTE between them. A table row is MG_COMPOSE_TAB_HEADER + K int32 (K a multiple of 4, zeros
//   after the n taps), so the taps are read four at a time on 16-byte boundaries; a pass without a table is a copy. Every table entry is
//   clamped (lo to the source, n to K and to the source, LDS rows to the staged ones): a table rewritten between the replays of a
//   captured launch cannot send a read outside the source or the tile.
//   resize_fused<PS>  a workgroup owns MG_COMPOSE_TILE_ROWS output rows x MG_COMPOSE_TILE_BYTES output bytes of a row (PS = bytes per pixel).
//     Phase 1: the source rows those output rows read (first lo .. last lo + n, at most MG_COMPOSE_MAX_ROWS) are resampled horizontally, one
//     byte per lane and step, into LDS rows of TILE_BYTES. The tap loop takes four taps (one int4) and four source bytes per trip: the
//     addresses come from lo + k alone, so the eight loads of a trip are independent and in flight together.
//     Phase 2: a lane owns 16 adjacent output bytes of one row: per vertical tap one ds_read_b128 (row pitch 192 B, a lane's unit 16-byte
//     aligned; the 12 lanes of an output row read one contiguous 192 B LDS row) and 16 integer multiply-adds; one 16-byte store when the
//     unit is whole and its address aligned, bytes otherwise.
//   hpass<PS> / vpass  the same two passes as two launches with the intermediate in global memory at a pitch rounded up to 16 bytes, for
//     geometries whose tile reads more rows than LDS holds. Same bytes.
// Paste. t = dst * (255 - m) + src * m + 128; ((t >> 8) + t) >> 8 per byte, the box clipped to the destination; a copy without a mask.
// Placement. place_partial<F> / place_final: fp64 sums of plane_j, of plane_j * (1 - a / 255) and of a / 255, one partial per workgroup
//   (lanes stride their chunk, then a fixed tree in LDS), the partials added in index order by one lane per sum. No floating-point atomics.
//   commit<F>: masked paste into the composite, unmasked paste onto the black canvas, plane idx = a / 255 (0 outside the box), planes
//   j < idx multiplied by 1 - a / 255, in one launch. a / 255 is a 256-entry table of F made on the host.
#include "common.h"
#include "../../include/maggie_hip.h"

namespace {

constexpr int TR = MG_COMPOSE_TILE_ROWS, TB = MG_COMPOSE_TILE_BYTES, MAXR = MG_COMPOSE_MAX_ROWS, NT = MG_COMPOSE_THREADS;
constexpr int HDR = MG_COMPOSE_TAB_HEADER, PREC = 22, MAXP = MG_COMPOSE_MAX_PLANES, NB = MG_COMPOSE_SUM_BLOCKS;
constexpr int UPR = TB / 16;                                                 // 16-byte units of a tile row
static_assert(TB % 48 == 0 && NT % 64 == 0 && MAXR >= TR && HDR % 4 == 0, "whole pixels of 1 and 3 bytes in 16-byte units");
static_assert(MAXR * TB == MG_COMPOSE_LDS_BYTES && MG_COMPOSE_LDS_BYTES <= 65536, "the staged rows fit the default LDS allowance");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> PREC, 0, 255); }

struct Span { int lo, n; };
// row i of a table of `k` taps a row, clamped to a source of `len`; without a table the identity
__device__ __forceinline__ Span span_of(const int32_t* __restrict__ tab, int k, int i, int len) {
    if (!tab) return {min(i, len - 1), 1};
    const int2 h = *(const int2*)(tab + (long)i * (HDR + k));
    const int lo = clampi(h.x, 0, len - 1);
    return {lo, clampi(h.y, 0, min(k, len - lo))};
}

// one byte of the horizontal pass: channel c of output pixel ox from the source row `row` of in_w pixels
template <int PS>
__device__ __forceinline__ uint8_t hbyte(const uint8_t* __restrict__ row, const int32_t* __restrict__ xtab, int kx, int ox, int c, int in_w) {
    if (!xtab) return row[min(ox, in_w - 1) * PS + c];
    const Span s = span_of(xtab, kx, ox, in_w);
    const int32_t* __restrict__ t = xtab + (long)ox * (HDR + kx) + HDR;
    const uint8_t* __restrict__ px = row + (long)s.lo * PS + c;
    const int last = s.n - 1;
    int acc = 1 << (PREC - 1);
    for (int k = 0; k < s.n; k += 4) {
        const int4 w = *(const int4*)(t + k);
        const int v0 = px[k * PS], v1 = px[min(k + 1, last) * PS], v2 = px[min(k + 2, last) * PS], v3 = px[min(k + 3, last) * PS];
        acc += v0 * w.x + (k + 1 < s.n ? v1 * w.y : 0) + (k + 2 < s.n ? v2 * w.z : 0) + (k + 3 < s.n ? v3 * w.w : 0);
    }
    return (uint8_t)clip8(acc);
}

__device__ __forceinline__ void mad16(int* acc, const uint4& v, int w) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += (int)((d[e >> 2] >> (8 * (e & 3))) & 0xffu) * w;
}

// 16 results of the vertical pass -> memory: one 16-byte store when whole and aligned, bytes otherwise
__device__ __forceinline__ void store16(uint8_t* __restrict__ dst, const int* acc, int nb) {
    uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) d[e >> 2] |= (uint32_t)clip8(acc[e]) << (8 * (e & 3));
    if (nb == 16 && ((uintptr_t)dst & 15) == 0) {
        *(uint4*)dst = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < nb) dst[e] = (uint8_t)(d[e >> 2] >> (8 * (e & 3)));
    }
}

// 16 adjacent bytes of the vertical pass for output row oy: rows of `pitch` bytes at `base` (16-byte aligned units), row `r0` of the source first
__device__ __forceinline__ void vunit(const uint8_t* __restrict__ base, int pitch, int r0, int rows, const int32_t* __restrict__ ytab, int ky, int oy,
                                      int in_h, int* acc) {
    const Span s = span_of(ytab, ky, oy, in_h);
    const int32_t* __restrict__ t = ytab ? ytab + (long)oy * (HDR + ky) + HDR : nullptr;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 1 << (PREC - 1);
#pragma unroll 2
    for (int k = 0; k < s.n; ++k) {
        const int w = t ? t[k] : (1 << PREC);
        const uint4 v = *(const uint4*)(base + (long)clampi(s.lo + k - r0, 0, rows - 1) * pitch);
        mad16(acc, v, w);
    }
}

template <int PS>
__global__ __launch_bounds__(NT) void resize_fused(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, const int32_t* __restrict__ xtab,
                                                   const int32_t* __restrict__ ytab, int kx, int ky, long src_plane, int src_pitch, int in_h,
                                                   int in_w, int out_h, int out_w, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[MAXR * TB];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const long p = blockIdx.x / (tiles_x * tiles_y);
    const int RB = out_w * PS;
    const int y0 = ty * TR, rows_out = min(TR, out_h - y0), b0 = tx * TB, tb = min(TB, RB - b0);
    const Span first = span_of(ytab, ky, y0, in_h), last = span_of(ytab, ky, y0 + rows_out - 1, in_h);
    const int r0 = first.lo, rows = clampi(last.lo + last.n - r0, 1, min(MAXR, in_h - r0));

    const uint8_t* __restrict__ sp = src + p * src_plane;
    for (int i = tid; i < rows * tb; i += NT) {
        const int r = i / tb, b = i - r * tb, gb = b0 + b, ox = gb / PS;
        s_rows[r * TB + b] = hbyte<PS>(sp + (long)(r0 + r) * src_pitch, xtab, kx, ox, gb - ox * PS, in_w);
    }
    __syncthreads();

    for (int u = tid; u < TR * UPR; u += NT) {
        const int ly = u / UPR, ub = (u - ly * UPR) * 16;
        if (ly >= rows_out || ub >= tb) continue;
        int acc[16];
        vunit(s_rows + ub, TB, r0, rows, ytab, ky, y0 + ly, in_h, acc);
        store16(out + (p * out_h + y0 + ly) * (long)RB + b0 + ub, acc, min(16, tb - ub));
    }
}

// horizontal pass alone: one byte per lane into rows of `dst_pitch` bytes
template <int PS>
__global__ __launch_bounds__(NT) void hpass(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int32_t* __restrict__ xtab, int kx,
                                            long src_plane, int src_pitch, int in_h, int in_w, int out_w, int dst_pitch, long total) {
    const int RB = out_w * PS;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long row = i / RB;
        const int gb = (int)(i - row * RB), ox = gb / PS;
        const long p = row / in_h;
        const int y = (int)(row - p * in_h);
        dst[row * dst_pitch + gb] = hbyte<PS>(src + p * src_plane + (long)y * src_pitch, xtab, kx, ox, gb - ox * PS, in_w);
    }
}

// vertical pass alone: 16 bytes per lane out of rows whose pitch is a multiple of 16
__global__ __launch_bounds__(NT) void vpass(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ out, const int32_t* __restrict__ ytab, int ky,
                                            int in_h, int out_h, int row_bytes, int tmp_pitch, long total) {
    const int upr = (row_bytes + 15) / 16;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long row = i / upr;
        const int ub = (int)(i - row * upr) * 16;
        const long p = row / out_h;
        const int oy = (int)(row - p * out_h);
        int acc[16];
        vunit(tmp + p * in_h * (long)tmp_pitch + ub, tmp_pitch, 0, in_h, ytab, ky, oy, in_h, acc);
        store16(out + row * row_bytes + ub, acc, min(16, row_bytes - ub));
    }
}

__device__ __forceinline__ int blend8(int d, int s, int m) {
    const int t = d * (255 - m) + s * m + 128;
    return ((t >> 8) + t) >> 8;
}

// box of bw x bh pixels: dst at (dx0, dy0), src and mask at (sx0, sy0)
__global__ __launch_bounds__(NT) void paste_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask,
                                                   int ps, int dw, int sw, int dx0, int dy0, int sx0, int sy0, int bw, int bh) {
    const int rb = bw * ps;
    const long total = (long)bh * rb;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int y = (int)(i / rb), b = (int)(i - (long)y * rb);
        const long so = (long)(sy0 + y) * sw + sx0;
        uint8_t* __restrict__ d = dst + ((long)(dy0 + y) * dw + dx0) * ps + b;
        const int s = src[so * ps + b];
        *d = mask ? (uint8_t)blend8(*d, s, mask[so + b / ps]) : (uint8_t)s;
    }
}

template <typename F> __device__ __forceinline__ F sub_rn(F a, F b);
template <> __device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
template <> __device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
template <typename F> __device__ __forceinline__ F mul_rn(F a, F b);
template <> __device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
template <> __device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }

// grid (NB, n_prev + 1): blockIdx.y = plane j, or n_prev for the area of a / 255. partial[(2 j + s) * NB + b], s = 0 new, 1 old.
template <typename F>
__global__ __launch_bounds__(NT) void place_partial(const F* __restrict__ planes, const uint8_t* __restrict__ a, const F* __restrict__ lut,
                                                    double* __restrict__ partial, int H, int W, int ha, int wa, int x, int y, int n_prev) {
    __shared__ double s_new[NT], s_old[NT];
    const int tid = threadIdx.x, j = blockIdx.y;
    const long HW = (long)H * W, chunk = (HW + NB - 1) / NB;
    const long lo = blockIdx.x * chunk, hi = min(HW, lo + chunk);
    const F* __restrict__ pl = planes + (long)max(min(j, n_prev - 1), 0) * HW;
    double sn = 0.0, so = 0.0;
    for (long i = lo + tid; i < hi; i += NT) {
        const int py = (int)(i / W), ax = (int)(i - (long)py * W) - x, ay = py - y;
        const bool inside = (unsigned)ax < (unsigned)wa && (unsigned)ay < (unsigned)ha;
        const F v = inside ? lut[a[(long)ay * wa + ax]] : (F)0;
        if (j < n_prev) {
            const F pv = pl[i];
            so += (double)pv;
            sn += (double)(inside ? mul_rn<F>(pv, sub_rn<F>((F)1, v)) : pv);
        } else {
            sn += (double)v;
        }
    }
    s_new[tid] = sn; s_old[tid] = so;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) { s_new[tid] += s_new[tid + o]; s_old[tid] += s_old[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        partial[(2 * j) * NB + blockIdx.x] = s_new[0];
        partial[(2 * j + 1) * NB + blockIdx.x] = s_old[0];
    }
}

// out[j] = new area of plane j, out[MAXP + j] = its present area, out[2 MAXP] = the area of a / 255; the rest 0
__global__ void place_final(const double* __restrict__ partial, double* __restrict__ out, int n_prev) {
    const int t = threadIdx.x;
    if (t > 2 * MAXP) return;
    int row = -1;
    if (t < MAXP) row = t < n_prev ? 2 * t : -1;
    else if (t < 2 * MAXP) row = t - MAXP < n_prev ? 2 * (t - MAXP) + 1 : -1;
    else row = 2 * n_prev;
    double s = 0.0;
    if (row >= 0)
        for (int b = 0; b < NB; ++b) s += partial[row * NB + b];
    out[t] = s;
}

template <typename F>
__global__ __launch_bounds__(NT) void commit_kernel(uint8_t* __restrict__ image, uint8_t* __restrict__ canvas, F* __restrict__ planes,
                                                    const uint8_t* __restrict__ fg, const uint8_t* __restrict__ a, const F* __restrict__ lut, int H,
                                                    int W, int ha, int wa, int x, int y, int idx) {
    const long HW = (long)H * W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        const int py = (int)(i / W), ax = (int)(i - (long)py * W) - x, ay = py - y;
        const bool inside = (unsigned)ax < (unsigned)wa && (unsigned)ay < (unsigned)ha;
        const long ai = inside ? (long)ay * wa + ax : 0;
        const int m = inside ? a[ai] : 0;
        if (fg) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = inside ? fg[ai * 3 + c] : 0;
                if (image && inside) image[i * 3 + c] = (uint8_t)blend8(image[i * 3 + c], s, m);
                if (canvas) canvas[i * 3 + c] = (uint8_t)s;
            }
        }
        const F v = inside ? lut[m] : (F)0;
        planes[idx * HW + i] = v;
        if (inside) {
            const F om = sub_rn<F>((F)1, v);
            F pv[MAXP];
#pragma unroll
            for (int j = 0; j < MAXP; ++j) pv[j] = j < idx ? planes[j * HW + i] : (F)0;
#pragma unroll
            for (int j = 0; j < MAXP; ++j)
                if (j < idx) planes[j * HW + i] = mul_rn<F>(pv[j], om);
        }
    }
}

template <typename F>
__global__ __launch_bounds__(NT) void planes_u8_kernel(const F* __restrict__ planes, uint8_t* __restrict__ out, int32_t* __restrict__ flags, long HW,
                                                       long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const F v = planes[i];
        out[i] = (uint8_t)clampi((int)mul_rn<F>(v, (F)255), 0, 255);
        if (v != (F)0) flags[i / HW] = 1;                                       // every writer stores the same word
    }
}

__global__ void box_init(int32_t* __restrict__ box, int H, int W) {
    if (threadIdx.x == 0) { box[0] = W; box[1] = H; box[2] = -1; box[3] = -1; }
}

// box = (min x, min y, max x, max y) of alpha > 0
__global__ __launch_bounds__(NT) void box_kernel(const uint8_t* __restrict__ alpha, int32_t* __restrict__ box, int H, int W) {
    __shared__ int s_box[4];
    if (threadIdx.x == 0) { s_box[0] = W; s_box[1] = H; s_box[2] = -1; s_box[3] = -1; }
    __syncthreads();
    const long HW = (long)H * W;
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        if (alpha[i] > 0) {
            const int py = (int)(i / W), px = (int)(i - (long)py * W);
            x0 = min(x0, px); y0 = min(y0, py); x1 = max(x1, px); y1 = max(y1, py);
        }
    }
    if (x1 >= 0) { atomicMin(&s_box[0], x0); atomicMin(&s_box[1], y0); atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1); }
    __syncthreads();
    if (threadIdx.x == 0 && s_box[2] >= 0) {
        atomicMin(&box[0], s_box[0]); atomicMin(&box[1], s_box[1]); atomicMax(&box[2], s_box[2]); atomicMax(&box[3], s_box[3]);
    }
}

unsigned blocks_for(long total) {
    const long b = (total + NT - 1) / NT;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
bool bad_side(int v) { return v <= 0 || v > MG_COMPOSE_MAX_SIDE; }

}  // namespace

extern "C" int mg_compose_limits(int* tile_rows, int* tile_bytes, int* max_rows, int* lds_bytes, int* tab_header, int* max_planes, int* sum_blocks,
                                 int* max_side) {
    if (!tile_rows || !tile_bytes || !max_rows || !lds_bytes || !tab_header || !max_planes || !sum_blocks || !max_side) return -2;
    *tile_rows = TR; *tile_bytes = TB; *max_rows = MAXR; *lds_bytes = MG_COMPOSE_LDS_BYTES; *tab_header = HDR; *max_planes = MAXP;
    *sum_blocks = NB; *max_side = MG_COMPOSE_MAX_SIDE;
    return 0;
}

extern "C" int mg_compose_resize(const uint8_t* src, uint8_t* out, uint8_t* tmp, const int32_t* xtab, const int32_t* ytab, long n, int ps,
                                 int src_h, int src_w, int cx, int cy, int cw, int ch, int out_h, int out_w, int kx, int ky, int regime,
                                 void* stream) {
    if (n < 0 || (ps != 1 && ps != 3) || bad_side(src_h) || bad_side(src_w) || bad_side(cw) || bad_side(ch) || bad_side(out_h) || bad_side(out_w))
        return -2;
    if (cx < 0 || cy < 0 || cx > src_w - cw || cy > src_h - ch) return -2;
    if (regime != MG_COMPOSE_FUSED && regime != MG_COMPOSE_TWO_PASS) return -2;
    if (xtab ? (kx <= 0 || kx % 4 != 0) : cw != out_w) return -2;
    if (ytab ? (ky <= 0 || ky % 4 != 0) : ch != out_h) return -2;
    if (n == 0) return 0;
    if (!src || !out || src == out || (regime == MG_COMPOSE_TWO_PASS && ytab && !tmp)) return -2;
    if (((uintptr_t)xtab & 15) || ((uintptr_t)ytab & 15) || ((uintptr_t)tmp & 15)) return -2;
    hipStream_t st = (hipStream_t)stream;
    const long src_plane = (long)src_h * src_w * ps;
    const int src_pitch = src_w * ps;
    const uint8_t* s0 = src + ((long)cy * src_w + cx) * ps;
    const int RB = out_w * ps;
    if (regime == MG_COMPOSE_FUSED) {
        const int tiles_x = (RB + TB - 1) / TB, tiles_y = (out_h + TR - 1) / TR;
        if (n > 0x7fffffffL / ((long)tiles_x * tiles_y)) return -3;
        const dim3 grid((unsigned)(n * tiles_x * tiles_y));
        if (ps == 1)
            hipLaunchKernelGGL((resize_fused<1>), grid, dim3(NT), 0, st, s0, out, xtab, ytab, kx, ky, src_plane, src_pitch, ch, cw, out_h, out_w,
                               tiles_x, tiles_y);
        else
            hipLaunchKernelGGL((resize_fused<3>), grid, dim3(NT), 0, st, s0, out, xtab, ytab, kx, ky, src_plane, src_pitch, ch, cw, out_h, out_w,
                               tiles_x, tiles_y);
        MG_CHECK_LAUNCH();
        return 0;
    }
    // two launches: the horizontal pass (a copy of the crop without a table) into tmp, or straight into out when there is no vertical pass
    const int tmp_pitch = ytab ? (RB + 15) / 16 * 16 : RB;
    uint8_t* hdst = ytab ? tmp : out;
    const long htotal = n * ch * (long)RB;
    if (ps == 1)
        hipLaunchKernelGGL((hpass<1>), dim3(blocks_for(htotal)), dim3(NT), 0, st, s0, hdst, xtab, kx, src_plane, src_pitch, ch, cw, out_w, tmp_pitch,
                           htotal);
    else
        hipLaunchKernelGGL((hpass<3>), dim3(blocks_for(htotal)), dim3(NT), 0, st, s0, hdst, xtab, kx, src_plane, src_pitch, ch, cw, out_w, tmp_pitch,
                           htotal);
    MG_CHECK_LAUNCH();
    if (ytab) {
        const long vtotal = n * out_h * (long)((RB + 15) / 16);
        hipLaunchKernelGGL(vpass, dim3(blocks_for(vtotal)), dim3(NT), 0, st, tmp, out, ytab, ky, ch, out_h, RB, tmp_pitch, vtotal);
        MG_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int mg_compose_paste(uint8_t* dst, const uint8_t* src, const uint8_t* mask, int ps, int dst_h, int dst_w, int src_h, int src_w, int x,
                                int y, void* stream) {
    if ((ps != 1 && ps != 3) || bad_side(dst_h) || bad_side(dst_w) || bad_side(src_h) || bad_side(src_w)) return -2;
    if (x < -MG_COMPOSE_MAX_SIDE || x > MG_COMPOSE_MAX_SIDE || y < -MG_COMPOSE_MAX_SIDE || y > MG_COMPOSE_MAX_SIDE) return -2;
    if (!dst || !src || dst == src || dst == mask) return -2;
    const int dx0 = x > 0 ? x : 0, dy0 = y > 0 ? y : 0, sx0 = dx0 - x, sy0 = dy0 - y;
    const int bw = (x + src_w < dst_w ? x + src_w : dst_w) - dx0, bh = (y + src_h < dst_h ? y + src_h : dst_h) - dy0;
    if (bw <= 0 || bh <= 0) return 0;                                        // the box lies outside the destination: nothing to paste
    hipLaunchKernelGGL(paste_kernel, dim3(blocks_for((long)bw * bh * ps)), dim3(NT), 0, (hipStream_t)stream, dst, src, mask, ps, dst_w, src_w, dx0,
                       dy0, sx0, sy0, bw, bh);
    MG_CHECK_LAUNCH();
    return 0;
}

static bool bad_place(const void* planes, const uint8_t* a, const void* lut, int dtype, int h, int w, int ha, int wa, int x, int y) {
    return !planes || !a || !lut || (dtype != MG_COMPOSE_F32 && dtype != MG_COMPOSE_F64) || bad_side(h) || bad_side(w) || bad_side(ha) ||
           bad_side(wa) || x < -MG_COMPOSE_MAX_SIDE || x > MG_COMPOSE_MAX_SIDE || y < -MG_COMPOSE_MAX_SIDE || y > MG_COMPOSE_MAX_SIDE;
}

extern "C" int mg_compose_try_place(const void* planes, const uint8_t* a, const void* lut, double* partial, double* out, int dtype, int h, int w,
                                    int ha, int wa, int x, int y, int n_prev, void* stream) {
    if (bad_place(planes, a, lut, dtype, h, w, ha, wa, x, y) || !partial || !out || n_prev < 0 || n_prev > MAXP) return -2;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(NB, n_prev + 1);
    if (dtype == MG_COMPOSE_F32)
        hipLaunchKernelGGL((place_partial<float>), grid, dim3(NT), 0, st, (const float*)planes, a, (const float*)lut, partial, h, w, ha, wa, x, y,
                           n_prev);
    else
        hipLaunchKernelGGL((place_partial<double>), grid, dim3(NT), 0, st, (const double*)planes, a, (const double*)lut, partial, h, w, ha, wa, x, y,
                           n_prev);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(place_final, dim3(1), dim3(64), 0, st, partial, out, n_prev);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_compose_commit(uint8_t* image, uint8_t* canvas, void* planes, const uint8_t* fg, const uint8_t* a, const void* lut, int dtype,
                                 int h, int w, int ha, int wa, int x, int y, int idx, void* stream) {
    if (bad_place(planes, a, lut, dtype, h, w, ha, wa, x, y) || idx < 0 || idx >= MAXP || ((image || canvas) && !fg)) return -2;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for((long)h * w));
    if (dtype == MG_COMPOSE_F32)
        hipLaunchKernelGGL((commit_kernel<float>), grid, dim3(NT), 0, st, image, canvas, (float*)planes, fg, a, (const float*)lut, h, w, ha, wa, x, y,
                           idx);
    else
        hipLaunchKernelGGL((commit_kernel<double>), grid, dim3(NT), 0, st, image, canvas, (double*)planes, fg, a, (const double*)lut, h, w, ha, wa, x,
                           y, idx);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_compose_planes_u8(const void* planes, uint8_t* out, int32_t* flags, int dtype, long count, int h, int w, void* stream) {
    if ((dtype != MG_COMPOSE_F32 && dtype != MG_COMPOSE_F64) || count < 0 || bad_side(h) || bad_side(w)) return -2;
    if (count == 0) return 0;
    if (!planes || !out || !flags) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mg_zero_words_kernel, dim3(1), dim3(256), 0, st, (uint32_t*)flags, count);
    MG_CHECK_LAUNCH();
    const long HW = (long)h * w, total = count * HW;
    if (dtype == MG_COMPOSE_F32)
        hipLaunchKernelGGL((planes_u8_kernel<float>), dim3(blocks_for(total)), dim3(NT), 0, st, (const float*)planes, out, flags, HW, total);
    else
        hipLaunchKernelGGL((planes_u8_kernel<double>), dim3(blocks_for(total)), dim3(NT), 0, st, (const double*)planes, out, flags, HW, total);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_compose_alpha_box(const uint8_t* alpha, int32_t* box, int h, int w, void* stream) {
    if (!alpha || !box || bad_side(h) || bad_side(w)) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(box_init, dim3(1), dim3(64), 0, st, box, h, w);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(box_kernel, dim3(blocks_for((long)h * w)), dim3(NT), 0, st, alpha, box, h, w);
    MG_CHECK_LAUNCH();
    return 0;
}
