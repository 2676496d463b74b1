// Every legal PNG decoded on the device: all 15 (colour type, bit depth) pairs, Adam7 or not, to the RGB frame of Pillow's
//   `Image.open(path).convert("RGB")` or the L plane of `.convert("L")`. Replaces the frame half of T.Load for .png files and the host
//   fall-back of csrc/pngdec.hip for 16-bit and interlaced files (maggie/dataloader/transforms.py:47-50). The chunk walk and the per-pass table
//   are the host's (maggie_amd/utils/pngcolor.py); DESIGN.md section 34 holds the conversion table, the bounds argument and the measurements.
//
// pc_inflate_kernel   `pd_inflate_file` of png_inflate.h, ONE WAVE per file, told the byte count of the record: the sum over the passes of
//   rows x (1 + rowbytes), which the kernel checks against the geometry it derives from (h, w, colour type, depth, interlace) itself.
// pc_unfilter_kernel  grid = (7, files): one wave per pass of a file (passes 2..7 of a non-interlaced file and empty passes return at once). A pass
//   is a sub-image of its own: the prior row is zero at ITS first row. The diagonal wavefront of pd_unfilter_kernel -- lane k owns row r0 + k of
//   a 64-row band and reconstructs byte x = s - k at step s; `b` is lane k - 1's result of the step before -- with `a` and `c` taken from 64-bit
//   shift registers (hist = hist << 8 | v; a = hist >> 8 (bpp - 1)), bpp 1, 2, 3, 4, 6 or 8. The reconstructed bytes go back through the LDS
//   tile IN PLACE over the filtered ones, 64 lanes storing 64 consecutive bytes of one scanline: the tile of steps [s0, s0 + 64) is loaded whole
//   before any of its bytes is computed, its outputs are exactly the bytes it loaded, the tiles of a band are disjoint, and `a`, `b`, `c` never
//   come from global memory. The filter type bytes stay where they are.
// pc_convert_kernel   grid = (ceil(h * ceil(w / 16) / 64), files): a lane owns 16 consecutive output pixels of one row. The source of a pixel
//   is its scanline and column, or for an Adam7 file its pass from (x & 7, y & 7) and row (y - y0) / dy, column (x - x0) / dx of that pass.
//   Samples below 8 bits are MSB first; at 16 bits the high byte, or min(v, 255) for grey (Pillow's I;16 conversion). The palette and the L
//   table of the file are in LDS. Output: uint8 RGB interleaved (48 bytes a lane), uint8 L (16 bytes) or fp32 normalised planar.
#ifndef MG_HOST_EMU
#include "pixel_norm.h"
#endif
#include "png_inflate.h"

namespace {

constexpr int CRW = MG_PNGCOLOR_REC_WORDS, IW = MG_PNGDEC_INFO_WORDS;
constexpr int CMAXROW = MG_PNGCOLOR_MAX_ROWBYTES;
constexpr int PITCH = 68;                                                  // bytes of a tile row: 17 dwords, so that 32 lanes hit 32 banks
constexpr int GP = MG_PNGCOLOR_GROUP;                                      // pixels of a lane of the convert kernel
constexpr int R_PASS = MG_PNGCOLOR_REC_PASSES, R_LTAB = MG_PNGCOLOR_REC_LTABLE, R_PAL = MG_PNGCOLOR_REC_PALETTE;
static_assert(R_PASS + 28 == R_LTAB && R_LTAB + 64 == R_PAL && R_PAL + 192 == CRW, "the record: 7 passes x 4 words, 256 L bytes, 256 x 3 palette bytes");
static_assert(GP == 16 && WV == 64, "a lane converts 16 pixels; one wave per workgroup");

MG_DEVCONST uint8_t A7_X0[7] = {0, 4, 0, 2, 0, 1, 0}, A7_Y0[7] = {0, 0, 4, 0, 2, 0, 1};
MG_DEVCONST uint8_t A7_DX[7] = {8, 8, 4, 4, 2, 2, 1}, A7_DY[7] = {8, 8, 8, 4, 4, 2, 2};

struct CGeo { int ch, depth, bpp, npass, total; };
struct CPass { int pw, ph, rb, off; };

// channels, bits and the number of passes of a record; 0 for an illegal (colour type, depth, interlace)
__device__ __forceinline__ int pc_form(const int32_t* rec, CGeo& g) {
    const int ct = rec[2], depth = rec[3], lace = rec[5];
    g.ch = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
    g.depth = depth;
    const bool low = depth == 1 || depth == 2 || depth == 4;
    const bool form = (ct == 0 && (low || depth == 8 || depth == 16)) || (ct == 3 && (low || depth == 8)) ||
                      ((ct == 2 || ct == 4 || ct == 6) && (depth == 8 || depth == 16));
    g.bpp = form ? (g.ch * depth >= 8 ? (g.ch * depth) >> 3 : 1) : 1;
    g.npass = lace == 1 ? 7 : 1;
    g.total = rec[6];
    return form && (lace == 0 || lace == 1) && rec[4] >= 0 && rec[4] <= 256;
}
// pass k of an (h, w) image as the formula gives it, `off` = the bytes of the passes in front of it
__device__ __forceinline__ CPass pc_pass(const CGeo& g, int lace, int k, int h, int w, long off) {
    CPass q;
    const int x0 = lace ? A7_X0[k] : 0, y0 = lace ? A7_Y0[k] : 0, dx = lace ? A7_DX[k] : 1, dy = lace ? A7_DY[k] : 1;
    q.pw = w > x0 ? (w - x0 + dx - 1) / dx : 0;
    q.ph = h > y0 ? (h - y0 + dy - 1) / dy : 0;
    const long rb = ((long)q.pw * g.ch * g.depth + 7) >> 3;
    q.rb = (int)(rb <= CMAXROW ? rb : -1);
    q.off = (int)(off <= MG_PNGDEC_MAX_RAW ? off : -1);
    return q;
}
// The record's pass table against the formula, its sizes against raw_stride: every lane computes the same answer. Returns 0 for a record that
// does not fit; then nothing of the file is touched.
__device__ __forceinline__ int pc_check(const int32_t* rec, int h, int w, long raw_stride, CGeo& g) {
    if (!pc_form(rec, g)) return 0;
    long off = 0;
    int ok = 1;
    for (int k = 0; k < 7; ++k) {
        const int32_t* t = rec + R_PASS + 4 * k;
        if (k >= g.npass) { ok &= t[0] == 0 && t[1] == 0 && t[2] == 0 && t[3] == 0; continue; }
        const CPass q = pc_pass(g, rec[5], k, h, w, off);
        ok &= q.rb >= 0 && q.off >= 0 && t[0] == q.pw && t[1] == q.ph && t[2] == q.rb && t[3] == q.off;
        if (q.pw > 0 && q.ph > 0 && q.rb >= 0) off += (long)q.ph * (1 + q.rb);
    }
    return ok && off == g.total && off >= 1 && off <= raw_stride;
}

__global__ void __launch_bounds__(MG_PNGDEC_THREADS)
pc_inflate_kernel(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ recs, uint8_t* __restrict__ raw, long raw_stride,
                  int32_t* __restrict__ info, int h, int w) {
    const long p = blockIdx.x;
    const int32_t* rec = recs + p * CRW;
    const long off = rec[0];
    const int len = rec[1];
    int32_t* inf = info + p * IW;
    CGeo g;
    if (!pc_check(rec, h, w, raw_stride, g) || off < 0 || len < 0 || off + len > data_bytes) {
        if (threadIdx.x == 0) inf[0] = MG_PNGDEC_ST_RECORD;
        return;
    }
    pd_inflate_file(data, data_bytes, off, len, g.total, raw + p * raw_stride, inf);
}

__global__ void __launch_bounds__(MG_PNGDEC_THREADS)
pc_unfilter_kernel(uint8_t* raw, long raw_stride, const int32_t* __restrict__ recs, int32_t* info, int h, int w) {
    __shared__ __attribute__((aligned(4))) uint8_t carry[CMAXROW];
    __shared__ __attribute__((aligned(4))) uint8_t tile[WV * PITCH];
    const int lane = (int)threadIdx.x;
    const int pass = (int)blockIdx.x;
    const long p = blockIdx.y;
    const int32_t* rec = recs + p * CRW;
    int32_t* inf = info + p * IW;
    if ((inf[0] & ~MG_PNGDEC_ST_FILTER) != 0) return;                      // the inflate failed: `raw` is not a file's scanlines
    CGeo g;
    if (!pc_check(rec, h, w, raw_stride, g)) {
        if (lane == 0) atomicOr(inf, MG_PNGDEC_ST_RECORD);
        return;
    }
    if (pass >= g.npass) return;
    const int32_t* t = rec + R_PASS + 4 * pass;
    const int pw = t[0], ph = t[1], rb = t[2];
    if (pw < 1 || ph < 1) return;                                          // an empty pass has no bytes
    const int bpp = g.bpp, pitch = 1 + rb, sh = 8 * (bpp - 1);
    uint8_t* rawp = raw + p * raw_stride + t[3];                           // pc_check: t[3] + ph * pitch <= total <= raw_stride
    for (int x = lane; x < rb; x += WV) carry[x] = 0;
    int bad = 0;
    for (int r0 = 0; r0 < ph; r0 += WV) {
        const int rows = ph - r0 < WV ? ph - r0 : WV;
        const int row = r0 + lane;
        const bool rowok = lane < rows;
        int ft = rowok ? rawp[(long)row * pitch] : 0;
        if (ft > 4) { bad |= MG_PNGDEC_ST_FILTER; ft = 0; }
        unsigned long long ha = 0, hc = 0;
        int prev = 0;
        const int nsteps = rb + rows - 1;
        for (int s0 = 0; s0 < nsteps; s0 += WV) {
            __syncthreads();
#pragma unroll 8
            for (int rr = 0; rr < WV; ++rr) {                              // row rr of the tile: bytes x = s0 - rr + j, j = 0..63
                const int x = s0 - rr + lane;
                if (rr < rows && x >= 0 && x < rb) tile[rr * PITCH + lane] = rawp[(long)(r0 + rr) * pitch + 1 + x];
            }
            __syncthreads();
            const int jn = nsteps - s0 < WV ? nsteps - s0 : WV;
            for (int j = 0; j < jn; ++j) {
                const int x = s0 + j - lane;
                const bool active = rowok && x >= 0 && x < rb;
                int b = pd_shift_up(prev);
                if (lane == 0) b = active ? carry[x] : 0;
                const int f = tile[lane * PITCH + j];
                const int a = (int)((ha >> sh) & 255u), c = (int)((hc >> sh) & 255u);
                const int pa = b > c ? b - c : c - b, pb = a > c ? a - c : c - a, pq = a + b - 2 * c, pc = pq < 0 ? -pq : pq;
                const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                const int pred = ft == 0 ? 0 : (ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : paeth)));
                const int v = (f + pred) & 255;
                if (active) {
                    tile[lane * PITCH + j] = (uint8_t)v;
                    ha = (ha << 8) | (unsigned)v;
                    hc = (hc << 8) | (unsigned)b;
                    prev = v;
                    if (lane == WV - 1) carry[x] = (uint8_t)v;
                }
            }
            __syncthreads();
#pragma unroll 8
            for (int rr = 0; rr < WV; ++rr) {                              // the same bytes back, reconstructed: 64 consecutive bytes of a scanline
                const int x = s0 - rr + lane;
                if (rr < rows && x >= 0 && x < rb) rawp[(long)(r0 + rr) * pitch + 1 + x] = tile[rr * PITCH + lane];
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(inf, bad);
}

__device__ __forceinline__ bool pc_is16(const void* q) { return ((uintptr_t)q & 15) == 0; }
__device__ __forceinline__ void pc_st16(void* q, const uint4& v, bool aligned) {
    if (aligned) *(uint4*)q = v;
    else __builtin_memcpy(q, &v, 16);                                      // the address may have any alignment
}

struct Norm { float m0, m1, m2, s0, s1, s2; };

__global__ void __launch_bounds__(MG_PNGDEC_THREADS)
pc_convert_kernel(const uint8_t* __restrict__ raw, long raw_stride, const int32_t* __restrict__ recs, void* __restrict__ out, int32_t* info,
                  int h, int w, int mode, Norm nm) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[256];              // the L table (256 bytes), then the palette (256 x 3 bytes)
    __shared__ int32_t ptab[28];
    const int lane = (int)threadIdx.x;
    const long p = blockIdx.y;
    const int32_t* rec = recs + p * CRW;
    int32_t* inf = info + p * IW;
    for (int i = lane; i < 256; i += WV) tab[i] = (uint32_t)rec[R_LTAB + i];
    if (lane < 28) ptab[lane] = rec[R_PASS + lane];
    __syncthreads();
    if ((inf[0] & ~MG_PNGDEC_ST_INDEX) != 0) return;                       // not a file's scanlines
    CGeo g;
    if (!pc_check(rec, h, w, raw_stride, g)) {
        if (lane == 0) atomicOr(inf, MG_PNGDEC_ST_RECORD);
        return;
    }
    const int chunks = (w + GP - 1) / GP;
    const long idx = (long)blockIdx.x * WV + lane;
    if (idx >= (long)h * chunks) return;
    const int y = (int)(idx / chunks), x0 = (int)(idx - (long)y * chunks) * GP;
    const int n = w - x0 < GP ? w - x0 : GP;
    const int ct = rec[2], depth = g.depth, ch = g.ch, npal = rec[4], lace = rec[5];
    const uint8_t* ltab = reinterpret_cast<const uint8_t*>(tab);
    const uint8_t* pal = ltab + 256;
    const uint8_t* rawp = raw + p * raw_stride;
    const int vmask = (1 << (depth < 8 ? depth : 8)) - 1, scale = depth < 8 ? 255 / vmask : 1;
    const uint8_t* row0 = rawp + (long)y * (1 + ptab[2]) + 1;              // the scanline of a non-interlaced file
    uint32_t rgb[3 * GP / 4] = {0};                                        // 48 bytes: R G B of the 16 pixels, packed
    uint32_t lum[GP / 4] = {0};
    int bad = 0;
#pragma unroll
    for (int k = 0; k < GP; ++k) {
        if (k >= n) continue;
        const int x = x0 + k;
        const uint8_t* row = row0;
        int col = x;
        if (lace) {
            const int ps = (y & 1) ? 6 : ((x & 1) ? 5 : ((y & 2) ? 4 : ((x & 2) ? 3 : ((y & 4) ? 2 : ((x & 4) ? 1 : 0)))));
            const int32_t* t = ptab + 4 * ps;
            row = rawp + t[3] + (long)((y - A7_Y0[ps]) / A7_DY[ps]) * (1 + t[2]) + 1;
            col = (x - A7_X0[ps]) / A7_DX[ps];
        }
        int s[3];
        if (depth < 8) {                                                   // grey or palette, MSB first
            const int bit = col * depth;
            s[0] = s[1] = s[2] = (row[bit >> 3] >> (8 - depth - (bit & 7))) & vmask;
        } else if (depth == 8) {
            const uint8_t* q = row + (long)col * ch;
            s[0] = q[0];
            s[1] = ch >= 3 ? q[1] : s[0];
            s[2] = ch >= 3 ? q[2] : s[0];
        } else {
            const uint8_t* q = row + (long)col * ch * 2;
            s[0] = ct == 0 ? (q[0] ? 255 : q[1]) : q[0];                   // grey 16: min(v, 255), Pillow's I;16; else the high byte
            s[1] = ch >= 3 ? q[2] : s[0];
            s[2] = ch >= 3 ? q[4] : s[0];
        }
        int r, gg, b, L;
        if (ct == 3) {
            if (s[0] >= npal) bad |= MG_PNGDEC_ST_INDEX;
            r = pal[3 * s[0]]; gg = pal[3 * s[0] + 1]; b = pal[3 * s[0] + 2];
            L = ltab[s[0]];
        } else if (ch < 3) {
            r = gg = b = L = s[0] * scale;
        } else {
            r = s[0]; gg = s[1]; b = s[2];
            L = (19595 * r + 38470 * gg + 7471 * b + 0x8000) >> 16;
        }
        rgb[(3 * k) >> 2] |= (uint32_t)r << (8 * ((3 * k) & 3));
        rgb[(3 * k + 1) >> 2] |= (uint32_t)gg << (8 * ((3 * k + 1) & 3));
        rgb[(3 * k + 2) >> 2] |= (uint32_t)b << (8 * ((3 * k + 2) & 3));
        lum[k >> 2] |= (uint32_t)L << (8 * (k & 3));
    }
    if (bad) atomicOr(inf, bad);
    const long pix = ((long)p * h + y) * w + x0;
    if (mode == MG_PNGCOLOR_OUT_RGB) {
        uint8_t* d = reinterpret_cast<uint8_t*>(out) + 3 * pix;
        if (n == GP) {
            const bool al = pc_is16(d);
#pragma unroll
            for (int q = 0; q < 3; ++q) pc_st16(d + 16 * q, make_uint4(rgb[4 * q], rgb[4 * q + 1], rgb[4 * q + 2], rgb[4 * q + 3]), al);
        } else {
#pragma unroll
            for (int k = 0; k < 3 * GP; ++k)
                if (k < 3 * n) d[k] = (uint8_t)(rgb[k >> 2] >> (8 * (k & 3)));
        }
    } else if (mode == MG_PNGCOLOR_OUT_L) {
        uint8_t* d = reinterpret_cast<uint8_t*>(out) + pix;
        if (n == GP) {
            pc_st16(d, make_uint4(lum[0], lum[1], lum[2], lum[3]), pc_is16(d));
        } else {
#pragma unroll
            for (int k = 0; k < GP; ++k)
                if (k < n) d[k] = (uint8_t)(lum[k >> 2] >> (8 * (k & 3)));
        }
    } else {                                                               // fp32 (files, 3, h, w): (v / 255 - mean) / std, IEEE divisions
        const float mean[3] = {nm.m0, nm.m1, nm.m2}, sd[3] = {nm.s0, nm.s1, nm.s2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = reinterpret_cast<float*>(out) + ((long)p * 3 + c) * h * w + (long)y * w + x0;
            const bool al = pc_is16(d);
#pragma unroll
            for (int q = 0; q < GP / 4; ++q) {
                float f[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 3 * (4 * q + e) + c;
                    f[e] = mg_norm_u8((int)((rgb[k >> 2] >> (8 * (k & 3))) & 255u), mean[c], sd[c]);
                }
                if (4 * q + 4 <= n) {
                    uint4 v;
                    __builtin_memcpy(&v, f, 16);
                    pc_st16(d + 4 * q, v, al);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * q + e < n) d[4 * q + e] = f[e];
                }
            }
        }
    }
}

__host__ inline bool pc_bad_args(long files, int h, int w, long raw_stride) {
    return files < 1 || h < 1 || w < 1 || h > MG_PNGDEC_MAX_SIDE || w > MG_PNGDEC_MAX_SIDE || raw_stride < 16 || raw_stride % 16 != 0 ||
           raw_stride > MG_PNGDEC_MAX_RAW;
}

}  // namespace

extern "C" int mg_pngcolor_limits(int* threads, int* max_side, int* max_rowbytes, int* rec_words, int* info_words, int* group) {
    if (!threads || !max_side || !max_rowbytes || !rec_words || !info_words || !group) return -2;
    *threads = WV; *max_side = MG_PNGDEC_MAX_SIDE; *max_rowbytes = CMAXROW; *rec_words = CRW; *info_words = IW; *group = GP;
    return 0;
}

extern "C" int mg_pngcolor_inflate(const uint8_t* data, long data_bytes, const int32_t* recs, uint8_t* raw, long raw_stride, int32_t* info, long files,
                                   int h, int w, void* stream) {
    if (pc_bad_args(files, h, w, raw_stride) || data_bytes < 0 || data_bytes > MG_PNGDEC_MAX_BYTES) return -2;
    if (!data || !recs || !raw || !info || (uintptr_t)data % 4 != 0 || (uintptr_t)raw % 16 != 0 || (uintptr_t)recs % 4 != 0 || (uintptr_t)info % 4 != 0) return -2;
    if (files > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(pc_inflate_kernel, dim3((unsigned)files), dim3(WV), 0, (hipStream_t)stream, data, data_bytes, recs, raw, raw_stride, info, h, w);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_pngcolor_unfilter(uint8_t* raw, long raw_stride, const int32_t* recs, int32_t* info, long files, int h, int w, void* stream) {
    if (pc_bad_args(files, h, w, raw_stride)) return -2;
    if (!raw || !recs || !info || (uintptr_t)recs % 4 != 0 || (uintptr_t)info % 4 != 0) return -2;
    if (files > 65535) return -3;
    hipLaunchKernelGGL(pc_unfilter_kernel, dim3(7, (unsigned)files), dim3(WV), 0, (hipStream_t)stream, raw, raw_stride, recs, info, h, w);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_pngcolor_convert(const uint8_t* raw, long raw_stride, const int32_t* recs, void* out, int32_t* info, long files, int h, int w,
                                   int mode, const float* mean, const float* std, void* stream) {
    if (pc_bad_args(files, h, w, raw_stride)) return -2;
    if (!raw || !recs || !out || !info || (uintptr_t)recs % 4 != 0 || (uintptr_t)info % 4 != 0) return -2;
    if (mode != MG_PNGCOLOR_OUT_RGB && mode != MG_PNGCOLOR_OUT_L && mode != MG_PNGCOLOR_OUT_NORM) return -2;
    if (files > 65535) return -3;
    Norm nm = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
    if (mode == MG_PNGCOLOR_OUT_NORM) {
        if (!mean || !std || (uintptr_t)out % 4 != 0) return -2;
        nm = Norm{mean[0], mean[1], mean[2], std[0], std[1], std[2]};
    }
    const long out_bytes = files * (long)h * w * (mode == MG_PNGCOLOR_OUT_L ? 1 : (mode == MG_PNGCOLOR_OUT_RGB ? 3 : 12));
    const uintptr_t r0 = (uintptr_t)raw, r1 = r0 + (uintptr_t)(files * raw_stride), o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)out_bytes;
    if (o0 < r1 && r0 < o1) return -2;                                     // the destination aliases the source
    const long lanes = (long)h * ((w + GP - 1) / GP);
    hipLaunchKernelGGL(pc_convert_kernel, dim3((unsigned)((lanes + WV - 1) / WV), (unsigned)files), dim3(WV), 0, (hipStream_t)stream, raw, raw_stride,
                       recs, out, info, h, w, mode, nm);
    MG_CHECK_LAUNCH();
    return 0;
}
