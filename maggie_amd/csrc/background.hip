// Background compositing on the device: LoadRandomBackground -> HistogramMatching -> ComposeBackground of the reference
// (maggie/dataloader/transforms.py:307-370,841-864) on uint8 tensors. DESIGN.md section 32.
//   mg_bg_blur_crop : the window of the blurred background. The blur is a separable INTEGER Gaussian modelled on OpenCV's 8-bit fixed-point path
//                     (taps of 8 fractional bits that sum to 256, 16-bit horizontal sums, 32-bit vertical sums, (s + 32768) >> 16); it was NOT
//                     compared with cv2.GaussianBlur. Only the window's pixels are computed.
//   mg_bg_hist      : per-channel 256-bin counts of interleaved frames.
//   mg_bg_match_lut : the two 256-entry tone curves of skimage.exposure.match_histograms (float branch) + the reference's blend. Frames are uint8,
//                     so the matched value is a pure function of the byte value per channel: the kernel touches no pixel.
//   mg_bg_compose   : clip(fg * (a / 255.0) + bg * (1 - a / 255.0), 0, 255).astype(uint8) in fp64 through the curves.
//
// blur_crop_kernel  A workgroup owns TR x TC window pixels, i.e. rows of TB = 3 TC bytes (interleaved RGB is a byte row whose taps lie 3 bytes
//   apart). Stage: the tile's source box plus a halo of R = ksize / 2 pixels as BYTES in LDS, rows and pixels through BORDER_REFLECT_101 on the
//   whole background; LDS column 0 is the source byte column a0 = the first needed column rounded down to 4, so that an LDS dword is a source
//   dword whenever rows start on dwords (one 4-byte load), as in motion.hip. Horizontal: a lane owns 4 adjacent bytes of a staged row; per tap two
//   dwords and v_alignbyte_b32, bytes 0, 2 and 1, 3 multiplied by the tap in two registers of two 16-bit fields (the taps are >= 0 and sum to
//   256: every partial sum is <= 255 * 256 < 65536); the sums go to LDS as u16. Vertical: a lane owns 16 adjacent bytes of an output row: two
//   16-byte LDS reads per tap, sixteen 32-bit sums, one 16-byte store when the address allows.
//
// The whole file is compiled WITHOUT floating-point contraction: np.interp rounds slope * (x - xp[j]) and the sum on their own, NumPy the two
// products and the sum of the blend and of the composite.
#include "common.h"
#include "../../include/maggie_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TR = MG_BG_TILE_ROWS, TC = MG_BG_TILE_COLS, NT = MG_BG_THREADS;
constexpr int RMAX = MG_BG_MAX_KSIZE / 2;                                  // 12
constexpr int ROWS = TR + 2 * RMAX;                                        // staged rows at most
constexpr int TB = TC * 3;                                                 // output bytes of a tile row
constexpr int NEED = (3 + TB + 2 * RMAX * 3 + 3) / 4 + 1;                  // dwords from a0 to the last needed column, + 1 for the second read
constexpr int PITCH = ((NEED + 15) / 32) * 32 + 16;                        // dwords of a staged row, = 16 mod 32
constexpr int HP = TB / 2 + 4;                                             // dwords of a row of u16 sums; a multiple of 4: 16-byte reads
constexpr int GP = MG_MATTE_GROUP;                                         // pixels of a lane in the histogram and the composite
static_assert(MG_BG_MAX_KSIZE % 2 == 1 && TB % 16 == 0 && PITCH >= NEED && HP % 4 == 0, "tile geometry");
static_assert(4 + MG_BG_MAX_KSIZE <= MG_BG_WIN_TABLE && NT % 64 == 0 && NT >= MG_BG_MAX_KSIZE, "table; whole waves");

// BORDER_REFLECT_101 in closed form (period 2 (len - 1)); 0 for a length of 1
__device__ __forceinline__ int r101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * (len - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ uint4 ld16(const void* p, bool aligned) {
    if (aligned) return *(const uint4*)p;
    uint4 v;
    __builtin_memcpy(&v, p, 16);            // the address may have any alignment
    return v;
}
__device__ __forceinline__ void st16(void* p, const uint4& v, bool aligned) {
    if (aligned) *(uint4*)p = v;
    else __builtin_memcpy(p, &v, 16);
}
__device__ __forceinline__ bool is16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

// ---- window of the blurred background --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void blur_crop_kernel(const uint8_t* __restrict__ bg, int bh, int bw, const int32_t* __restrict__ win,
                                                       uint8_t* __restrict__ out, int h, int w, int tiles_x, int wide_in) {
    __shared__ uint32_t s_px[ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_h[ROWS * HP];
    __shared__ uint32_t s_q[MG_BG_MAX_KSIZE];
    const int tid = threadIdx.x;
    // the table may have been rewritten on the device: nothing below leaves the background or LDS whatever it holds
    const int ks = clampi(win[0], 1, MG_BG_MAX_KSIZE) | 1, R = ks >> 1;
    const int x0 = clampi(win[1], 0, bw - w), y0 = clampi(win[2], 0, bh - h);
    if (tid < ks) s_q[tid] = (uint32_t)clampi(win[4 + tid], 0, 256);

    const int ty0 = (blockIdx.x / tiles_x) * TR, tx0 = (blockIdx.x % tiles_x) * TC;
    const int rows_out = min(TR, h - ty0), tb = min(TB, (w - tx0) * 3);
    const int RB = bw * 3;                                                  // bytes of a background row
    const int gx = (x0 + tx0) * 3;                                          // source byte column of the tile's first output byte
    const int a0 = (gx - R * 3) & ~3;                                       // rounds down, also below zero
    const int nw = (gx + ((tb + 3) & ~3) + R * 3 - a0 + 3) >> 2;            // <= NEED - 1
    const int rows = rows_out + 2 * R;                                      // <= ROWS

    // ---- stage ----
    for (int i = tid; i < rows * nw; i += NT) {
        const int ry = i / nw, cw = i - ry * nw;
        const uint8_t* __restrict__ row = bg + (long)r101(y0 + ty0 - R + ry, bh) * RB;
        const int col = a0 + 4 * cw;
        uint32_t v = 0;
        if (wide_in && col >= 0 && col + 4 <= RB) {
            v = *(const uint32_t*)(row + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = col + e;
                const int px = c >= 0 ? c / 3 : -((2 - c) / 3);            // floor
                v |= (uint32_t)row[r101(px, bw) * 3 + (c - px * 3)] << (8 * e);
            }
        }
        s_px[ry * PITCH + cw] = v;
    }
    __syncthreads();

    // ---- horizontal: u16 sums of every staged row ----
    constexpr int UPR = TB / 4;
    for (int u = tid; u < rows * UPR; u += NT) {
        const int ry = u / UPR, bl = (u - ry * UPR) * 4;
        if (bl >= tb) continue;
        const int base = ry * (PITCH * 4) + (gx + bl - a0) - R * 3;         // >= ry * PITCH * 4
        uint32_t acc02 = 0, acc13 = 0;
        for (int k = 0; k < ks; ++k) {
            const int o = base + 3 * k;
            const uint32_t w0 = s_px[o >> 2], w1 = s_px[(o >> 2) + 1];
            const uint32_t v = __builtin_amdgcn_alignbyte(w1, w0, (unsigned)o & 3u);
            const uint32_t q = s_q[k];
            acc02 += (v & 0x00ff00ffu) * q;
            acc13 += ((v >> 8) & 0x00ff00ffu) * q;
        }
        s_h[ry * HP + (bl >> 1)] = (acc02 & 0xffffu) | (acc13 << 16);
        s_h[ry * HP + (bl >> 1) + 1] = (acc02 >> 16) | (acc13 & 0xffff0000u);
    }
    __syncthreads();

    // ---- vertical: 32-bit sums, round, store ----
    constexpr int VPR = TB / 16;
    for (int u = tid; u < TR * VPR; u += NT) {
        const int ly = u / VPR, b16 = (u - ly * VPR) * 16;
        if (ly >= rows_out || b16 >= tb) continue;
        uint32_t acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0;
        for (int k = 0; k < ks; ++k) {
            const uint4* p = (const uint4*)&s_h[(ly + k) * HP + (b16 >> 1)];
            const uint4 lo = p[0], hi = p[1];
            const uint32_t wd[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const uint32_t q = s_q[k];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[2 * e] += (wd[e] & 0xffffu) * q;
                acc[2 * e + 1] += (wd[e] >> 16) * q;
            }
        }
        uint32_t ow[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            ow[e] = ((acc[4 * e] + 32768u) >> 16) | ((acc[4 * e + 1] + 32768u) >> 16) << 8 | ((acc[4 * e + 2] + 32768u) >> 16) << 16 |
                    ((acc[4 * e + 3] + 32768u) >> 16) << 24;
        uint8_t* __restrict__ dst = out + ((long)(ty0 + ly) * w + tx0) * 3 + b16;
        if (b16 + 16 <= tb && is16(dst)) {
            *(uint4*)dst = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (b16 + e < tb) dst[e] = (uint8_t)byte_of(ow, e);
        }
    }
}

// ---- histograms ------------------------------------------------------------------------------------------------------------------------
// counts [3][256] += the bytes of `npix` interleaved pixels. A lane owns 16 pixels (three 16-byte loads; 48 = 0 mod 3, so byte k of a group is
// channel k % 3). Every wave has its own 3 x 256 bins in LDS. A lane adds a RUN of equal bytes of a channel at once, so a constant image
// costs one LDS atomic per lane, channel and group instead of sixteen to one address. Integer sums: the order does not matter.
__global__ __launch_bounds__(NT) void hist_kernel(const uint8_t* __restrict__ in, long npix, uint32_t* __restrict__ counts) {
    constexpr int NW = NT / 64;
    __shared__ uint32_t bins[NW * 768];
    for (int i = threadIdx.x; i < NW * 768; i += NT) bins[i] = 0u;
    __syncthreads();
    uint32_t* my = bins + (threadIdx.x >> 6) * 768;
    const bool al = is16(in);
    const long groups = (npix + GP - 1) / GP;
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long pix0 = grp * GP;
        if (pix0 + GP <= npix) {
            uint32_t fw[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = ld16(in + pix0 * 3 + 16 * q, al);
                fw[4 * q] = v.x; fw[4 * q + 1] = v.y; fw[4 * q + 2] = v.z; fw[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint32_t last = byte_of(fw, c), run = 1;
#pragma unroll
                for (int j = 1; j < GP; ++j) {
                    const uint32_t v = byte_of(fw, 3 * j + c);
                    if (v != last) {
                        atomicAdd(&my[c * 256 + last], run);
                        last = v;
                        run = 0;
                    }
                    ++run;
                }
                atomicAdd(&my[c * 256 + last], run);
            }
        } else {
            for (long i = pix0 * 3; i < npix * 3; ++i) atomicAdd(&my[(int)(i % 3) * 256 + in[i]], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 768; i += NT) {
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) s += bins[k * 768 + i];
        if (s != 0u) atomicAdd(&counts[i], s);
    }
}

// ---- tone curves -----------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 lanes, lane v = byte value v. Per channel, with S the histogram of the matched side and T the template's:
//   quantiles   qs[v] = cumsum(S)[v] / size(S), over the occupied bins of T  xp[j] = cumsum(T) / size(T), fp[j] = the bin's value (fp64; the
//               cumulative counts are integers below 2^31, exact in fp64, and the fp64 division is IEEE-correct);
//   np.interp   one-entry template -> fp[0]; x < xp[0] -> fp[0]; x > xp[n - 1] -> fp[n - 1]; j = the last xp[j] <= x; j == n - 1 or
//               x == xp[j] -> fp[j]; else slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]), slope * (x - xp[j]) + fp[j], each operation rounded;
//   blend       m32 = f32(result); uint8(m32 * ratio + f32(v) * (1 - ratio)) in fp32, each operation rounded, truncated.
// Bins of S that are empty, and the whole other side, are the identity.
__global__ __launch_bounds__(256) void match_lut_kernel(const uint32_t* __restrict__ hist_fg, const uint32_t* __restrict__ hist_bg,
                                                        const float* __restrict__ draw, uint8_t* __restrict__ luts) {
    __shared__ uint32_t cs[256], ct[256];
    __shared__ double xp[256], fp[256];
    const int v = threadIdx.x;
    const float ratio = draw[0], rest = draw[1];
    const bool match_bg = draw[2] != 0.f;
    const uint32_t* __restrict__ hs = match_bg ? hist_bg : hist_fg;
    const uint32_t* __restrict__ ht = match_bg ? hist_fg : hist_bg;
    uint8_t* __restrict__ lut_m = luts + (match_bg ? 768 : 0);
    uint8_t* __restrict__ lut_i = luts + (match_bg ? 0 : 768);
    for (int c = 0; c < 3; ++c) {
        cs[v] = hs[c * 256 + v];
        ct[v] = ht[c * 256 + v];
        __syncthreads();
        uint32_t sum_s = 0, sum_t = 0, tot_s = 0, tot_t = 0;
        int rank = 0, n = 0;
        for (int u = 0; u < 256; ++u) {
            const uint32_t a = cs[u], b = ct[u];
            tot_s += a; tot_t += b;
            n += b != 0u;
            if (u <= v) { sum_s += a; sum_t += b; rank += b != 0u; }
        }
        const bool occupied = cs[v] != 0u;
        if (ct[v] != 0u) {
            xp[rank - 1] = (double)sum_t / (double)tot_t;
            fp[rank - 1] = (double)v;
        }
        __syncthreads();
        uint32_t res = (uint32_t)v;
        if (occupied && n > 0) {
            const double x = (double)sum_s / (double)tot_s;
            double m;
            if (n == 1 || x < xp[0]) {
                m = fp[0];
            } else if (x > xp[n - 1]) {
                m = fp[n - 1];
            } else {
                int lo = 0, hi = n - 1;                                     // xp[lo] <= x always holds
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (xp[mid] <= x) lo = mid; else hi = mid - 1;
                }
                const int j = lo;
                if (j == n - 1 || xp[j] == x) {
                    m = fp[j];
                } else {
                    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
                    const double prod = slope * (x - xp[j]);
                    m = prod + fp[j];
                }
            }
            const float m32 = (float)m;
            const float t1 = m32 * ratio;
            const float t2 = (float)v * rest;
            const float s = t1 + t2;
            res = (uint32_t)fminf(fmaxf(s, 0.f), 255.f);
        }
        lut_m[c * 256 + v] = (uint8_t)res;
        lut_i[c * 256 + v] = (uint8_t)v;
        __syncthreads();
    }
}

// ---- composite -------------------------------------------------------------------------------------------------------------------------
// uint8(clip(f64(lutF[fg]) * wt[a][0] + f64(lutB[bg]) * wt[a][1], 0, 255)): two products and a sum, each rounded to fp64. The sum exceeds 255
// for 11 of the 256^3 triples (255.00000000000003), so the clip acts. A lane owns 16 pixels: three 16-byte loads of fg and of bg, one of alpha,
// three 16-byte stores per output.
__device__ __forceinline__ uint32_t compose_of(uint32_t f, uint32_t b, double w1, double w0) {
    const double t1 = (double)f * w1;
    const double t2 = (double)b * w0;
    double s = t1 + t2;
    s = fmin(fmax(s, 0.0), 255.0);
    return (uint32_t)s;
}

__global__ __launch_bounds__(NT) void compose_kernel(const uint8_t* __restrict__ fg, const uint8_t* __restrict__ alpha,
                                                     const uint8_t* __restrict__ bg, long bg_stride, long npix, const uint8_t* __restrict__ luts,
                                                     const double* __restrict__ wt, uint8_t* __restrict__ out, uint8_t* __restrict__ fg_out,
                                                     uint8_t* __restrict__ bg_out) {
    __shared__ double s_w[512];
    __shared__ uint8_t s_l[2 * 768];
    for (int i = threadIdx.x; i < 512; i += NT) s_w[i] = wt[i];
    for (int i = threadIdx.x; i < 2 * 768; i += NT) s_l[i] = luts ? luts[i] : (uint8_t)(i & 255);
    __syncthreads();
    const long t = blockIdx.y, n3 = npix * 3;
    const uint8_t* fr = fg + t * n3;
    const uint8_t* al = alpha + t * npix;
    const uint8_t* bgp = bg + t * bg_stride;
    uint8_t* od = out + t * n3;
    uint8_t* fo = fg_out ? fg_out + t * n3 : nullptr;
    uint8_t* bo = bg_out && (bg_stride != 0 || t == 0) ? bg_out + t * bg_stride : nullptr;      // a shared background is written by frame 0
    const bool fr_al = is16(fr), a_al = is16(al), bg_al = is16(bgp), od_al = is16(od), fo_al = is16(fo), bo_al = is16(bo);
    const long groups = (npix + GP - 1) / GP;
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long pix0 = grp * GP;
        if (pix0 + GP <= npix) {
            uint32_t fw[12], bw[12], aw[4], ow[12], fm[12], bm[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = ld16(fr + pix0 * 3 + 16 * q, fr_al);
                fw[4 * q] = v.x; fw[4 * q + 1] = v.y; fw[4 * q + 2] = v.z; fw[4 * q + 3] = v.w;
                const uint4 u = ld16(bgp + pix0 * 3 + 16 * q, bg_al);
                bw[4 * q] = u.x; bw[4 * q + 1] = u.y; bw[4 * q + 2] = u.z; bw[4 * q + 3] = u.w;
            }
            const uint4 a4 = ld16(al + pix0, a_al);
            aw[0] = a4.x; aw[1] = a4.y; aw[2] = a4.z; aw[3] = a4.w;
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                uint32_t w = 0, wf = 0, wb = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int k = 4 * q + b, ch = k % 3;
                    const uint32_t a = byte_of(aw, k / 3);
                    const uint32_t f = s_l[ch * 256 + byte_of(fw, k)], g = s_l[768 + ch * 256 + byte_of(bw, k)];
                    w |= compose_of(f, g, s_w[2 * a], s_w[2 * a + 1]) << (8 * b);
                    wf |= f << (8 * b);
                    wb |= g << (8 * b);
                }
                ow[q] = w; fm[q] = wf; bm[q] = wb;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                st16(od + pix0 * 3 + 16 * q, make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]), od_al);
                if (fo) st16(fo + pix0 * 3 + 16 * q, make_uint4(fm[4 * q], fm[4 * q + 1], fm[4 * q + 2], fm[4 * q + 3]), fo_al);
                if (bo) st16(bo + pix0 * 3 + 16 * q, make_uint4(bm[4 * q], bm[4 * q + 1], bm[4 * q + 2], bm[4 * q + 3]), bo_al);
            }
        } else {
            // the last group of a frame: fewer than GP pixels, byte by byte
            for (long i = pix0; i < npix; ++i) {
                const uint32_t a = al[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t f = s_l[c * 256 + fr[i * 3 + c]], g = s_l[768 + c * 256 + bgp[i * 3 + c]];
                    od[i * 3 + c] = (uint8_t)compose_of(f, g, s_w[2 * a], s_w[2 * a + 1]);
                    if (fo) fo[i * 3 + c] = (uint8_t)f;
                    if (bo) bo[i * 3 + c] = (uint8_t)g;
                }
            }
        }
    }
}

unsigned grid_of(long groups, long cap) {
    long blocks = (groups + NT - 1) / NT;
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int mg_bg_limits(int* max_ksize, int* win_table, int* tile_rows, int* tile_cols, int* max_side) {
    if (!max_ksize || !win_table || !tile_rows || !tile_cols || !max_side) return -2;
    *max_ksize = MG_BG_MAX_KSIZE; *win_table = MG_BG_WIN_TABLE; *tile_rows = TR; *tile_cols = TC; *max_side = MG_BG_MAX_SIDE;
    return 0;
}

extern "C" int mg_bg_blur_crop(const uint8_t* bg, int bh, int bw, const int32_t* win, uint8_t* out, int h, int w, void* stream) {
    if (!bg || !win || !out || bg == out || ((uintptr_t)win & 3)) return -2;
    if (h <= 0 || w <= 0 || h > bh || w > bw || bh > MG_BG_MAX_SIDE || bw > MG_BG_MAX_SIDE) return -2;
    const int tiles_x = (w + TC - 1) / TC;
    const long tiles = (long)tiles_x * ((h + TR - 1) / TR);
    if (tiles > 0x7fffffffL) return -3;
    const int wide_in = ((bw * 3) % 4 == 0) && ((uintptr_t)bg % 4 == 0);
    hipLaunchKernelGGL(blur_crop_kernel, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, bg, bh, bw, win, out, h, w, tiles_x, wide_in);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_bg_hist(const uint8_t* frames, long pixels, uint32_t* counts, void* stream) {
    if (!frames || !counts || pixels <= 0 || pixels > 0x7fffffffL || ((uintptr_t)counts & 3)) return -2;
    hipLaunchKernelGGL(hist_kernel, dim3(grid_of((pixels + GP - 1) / GP, MG_BG_HIST_MAX_BLOCKS)), dim3(NT), 0, (hipStream_t)stream, frames, pixels,
                       counts);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_bg_match_lut(const uint32_t* hist_fg, const uint32_t* hist_bg, const float* draw, uint8_t* luts, void* stream) {
    if (!hist_fg || !hist_bg || !draw || !luts || (((uintptr_t)hist_fg | (uintptr_t)hist_bg | (uintptr_t)draw) & 3)) return -2;
    hipLaunchKernelGGL(match_lut_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist_fg, hist_bg, draw, luts);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_bg_compose(const uint8_t* fg, const uint8_t* alpha, const uint8_t* bg, long bg_frames, long frames, int h, int w,
                             const uint8_t* luts, const double* wt, uint8_t* out, uint8_t* fg_out, uint8_t* bg_out, void* stream) {
    if (!fg || !alpha || !bg || !wt || !out || frames < 0 || h <= 0 || w <= 0 || ((uintptr_t)wt & 7)) return -2;
    if (bg_frames != 1 && bg_frames != frames) return -2;
    if ((long)h * w > 0x7fffffffL / 3) return -2;
    if (frames == 0) return 0;
    if (frames > 65535) return -3;
    const long npix = (long)h * w;
    const dim3 grid(grid_of((npix + GP - 1) / GP, MG_MATTE_MAX_BLOCKS), (unsigned)frames);
    hipLaunchKernelGGL(compose_kernel, grid, dim3(NT), 0, (hipStream_t)stream, fg, alpha, bg, bg_frames == 1 && frames != 1 ? 0L : npix * 3, npix,
                       luts, wt, out, fg_out, bg_out);
    MG_CHECK_LAUNCH();
    return 0;
}
