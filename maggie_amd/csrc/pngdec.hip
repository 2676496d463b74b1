// PNG decoding on the device: the zlib streams (the concatenated IDAT payloads) of P non-interlaced files of one size -> the filtered
//   scanlines (`raw`) -> the L plane that Pillow's `Image.open(path).convert("L")` returns. Replaces the alpha / mask half of T.Load
//   (maggie/dataloader/transforms.py:47-50). The chunk walk, the CRCs and the two zlib header bytes are the host's (maggie_amd/utils/pngdec.py);
//   DESIGN.md section 26 holds the bounds argument, the LDS layout and the measurements.
//
// pd_inflate_kernel   RFC 1951, ONE WAVE per file, grid = P: `pd_inflate_file` of png_inflate.h (shared with csrc/pngcolor.hip), told the byte
//   count that IHDR promises.
// pd_unfilter_kernel  one wave per file, a band of 64 rows at a time: lane k owns row r0 + k and reconstructs byte x = s - k at step s, so that
//   the byte above (`b`) is lane k - 1's result of the previous step, moved by one cross-lane shift; `a` and `c` are the lane's own result
//   and its own `b` of bpp steps ago (bpp <= 4: four registers each). The filter type is per lane: the five predictors are computed and
//   selected. A band takes rowbytes + 63 steps. The filtered bytes come through a skewed LDS tile from coalesced loads; the last row of a
//   band stays in LDS for the next. The epilogue unpacks 1 / 2 / 4-bit samples, looks grey and palette samples up in the file's 256-entry L
//   table, applies (19595 R + 38470 G + 7471 B + 0x8000) >> 16 to RGB(A), takes the grey byte of LA, and stores uint8.
#include "png_inflate.h"

namespace {

constexpr int RW = MG_PNGDEC_REC_WORDS, IW = MG_PNGDEC_INFO_WORDS;
constexpr int MAXROW = MG_PNGDEC_MAX_ROWBYTES;
constexpr int PITCH = 68;                                                  // bytes of a tile row: 17 dwords, so that 32 lanes hit 32 banks

struct Geo { int ok, ch, rb, bpp, expect; };
// rowbytes, bytes per complete pixel and the inflated size of a file of colour type `ct` and `depth` bits; ok = 0 outside the supported set
__device__ __forceinline__ Geo geo_of(int ct, int depth, int h, int w, long raw_stride) {
    Geo g;
    g.ch = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
    const bool form = ((ct == 0 || ct == 3) && (depth == 1 || depth == 2 || depth == 4 || depth == 8)) || ((ct == 2 || ct == 4 || ct == 6) && depth == 8);
    const long bits = (long)w * g.ch * (form ? depth : 8);
    const long rb = (bits + 7) >> 3;
    g.rb = (int)(rb <= MAXROW ? rb : MAXROW);
    g.bpp = (g.ch * (form ? depth : 8)) >> 3;
    if (g.bpp < 1) g.bpp = 1;
    const long expect = (long)h * (1 + g.rb);
    g.ok = form && rb <= MAXROW && expect <= raw_stride;
    g.expect = (int)(g.ok ? expect : 0);
    return g;
}

__global__ void __launch_bounds__(MG_PNGDEC_THREADS)
pd_inflate_kernel(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ recs, uint8_t* __restrict__ raw, long raw_stride,
                  int32_t* __restrict__ info, int h, int w) {
    const long p = blockIdx.x;
    const int32_t* rec = recs + p * RW;
    const long off = rec[0];
    const int len = rec[1];
    const Geo g = geo_of(rec[2], rec[3], h, w, raw_stride);
    int32_t* inf = info + p * IW;
    if (!g.ok || off < 0 || len < 0 || off + len > data_bytes) {
        if (threadIdx.x == 0) inf[0] = MG_PNGDEC_ST_RECORD;
        return;
    }
    pd_inflate_file(data, data_bytes, off, len, g.expect, raw + p * raw_stride, inf);
}

__global__ void __launch_bounds__(MG_PNGDEC_THREADS)
pd_unfilter_kernel(const uint8_t* __restrict__ raw, long raw_stride, const int32_t* __restrict__ recs, uint8_t* __restrict__ out,
                   int32_t* __restrict__ info, int h, int w) {
    __shared__ __attribute__((aligned(4))) uint8_t carry[MAXROW];
    __shared__ __attribute__((aligned(4))) uint8_t tile[WV * PITCH];
    __shared__ __attribute__((aligned(4))) uint8_t lut[256];
    const int lane = (int)threadIdx.x;
    const long p = blockIdx.x;
    const int32_t* rec = recs + p * RW;
    const int ct = rec[2], depth = rec[3], npal = rec[4];
    int32_t* inf = info + p * IW;
    if (inf[0] != 0) return;                                               // the inflate failed: `raw` is not a file's scanlines
    const Geo g = geo_of(ct, depth, h, w, raw_stride);
    if (!g.ok) {
        if (lane == 0) inf[0] = MG_PNGDEC_ST_RECORD;
        return;
    }
    const int rb = g.rb, bpp = g.bpp, pitch = 1 + rb;
    const uint8_t* rawp = raw + p * raw_stride;
    uint8_t* outp = out + p * (long)h * w;
    *reinterpret_cast<uint32_t*>(lut + 4 * lane) = (uint32_t)rec[8 + lane];
    for (int x = lane; x < rb; x += WV) carry[x] = 0;
    const int ppb = depth < 8 ? 8 / depth : 1, vmask = (1 << depth) - 1;
    int bad = 0;
    for (int r0 = 0; r0 < h; r0 += WV) {
        const int rows = h - r0 < WV ? h - r0 : WV;
        const int row = r0 + lane;
        const bool rowok = lane < rows;
        int ft = rowok ? rawp[(long)row * pitch] : 0;
        if (ft > 4) { bad |= MG_PNGDEC_ST_FILTER; ft = 0; }
        int a0 = 0, a1 = 0, a2 = 0, a3 = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, prev = 0;
        uint8_t* orow = outp + (long)row * w;
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
                const int a = bpp == 1 ? a0 : (bpp == 2 ? a1 : (bpp == 3 ? a2 : a3));
                const int c = bpp == 1 ? c0 : (bpp == 2 ? c1 : (bpp == 3 ? c2 : c3));
                const int pa = b > c ? b - c : c - b, pb = a > c ? a - c : c - a, pq = a + b - 2 * c, pc = pq < 0 ? -pq : pq;
                const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                const int pred = ft == 0 ? 0 : (ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : paeth)));
                const int v = (f + pred) & 255;
                if (active) {
                    if (ct == 2) {
                        const int px = x / 3;
                        if (x - 3 * px == 2) orow[px] = (uint8_t)((19595 * a1 + 38470 * a0 + 7471 * v + 0x8000) >> 16);
                    } else if (ct == 6) {
                        if ((x & 3) == 3) orow[x >> 2] = (uint8_t)((19595 * a2 + 38470 * a1 + 7471 * a0 + 0x8000) >> 16);
                    } else if (ct == 4) {
                        if ((x & 1) == 0) orow[x >> 1] = (uint8_t)v;
                    } else if (depth == 8) {
                        if (v >= npal) bad |= MG_PNGDEC_ST_INDEX;
                        orow[x] = lut[v];
                    } else {
                        for (int i = 0; i < ppb; ++i) {
                            const int px = x * ppb + i;
                            if (px < w) {
                                const int s = (v >> (8 - depth * (i + 1))) & vmask;
                                if (s >= npal) bad |= MG_PNGDEC_ST_INDEX;
                                orow[px] = lut[s];
                            }
                        }
                    }
                    a3 = a2; a2 = a1; a1 = a0; a0 = v;
                    c3 = c2; c2 = c1; c1 = c0; c0 = b;
                    prev = v;
                    if (lane == WV - 1) carry[x] = (uint8_t)v;
                }
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(inf, bad);
}

__host__ inline bool pd_bad_args(long planes, int h, int w, long raw_stride) {
    return planes < 1 || h < 1 || w < 1 || h > MG_PNGDEC_MAX_SIDE || w > MG_PNGDEC_MAX_SIDE || raw_stride < 16 || raw_stride % 16 != 0 ||
           raw_stride > MG_PNGDEC_MAX_RAW;
}

}  // namespace

extern "C" int mg_pngdec_limits(int* threads, int* max_side, int* max_rowbytes, int* rec_words, int* info_words, int* round_tokens, int* flush_bytes) {
    if (!threads || !max_side || !max_rowbytes || !rec_words || !info_words || !round_tokens || !flush_bytes) return -2;
    *threads = WV; *max_side = MG_PNGDEC_MAX_SIDE; *max_rowbytes = MAXROW; *rec_words = RW; *info_words = IW; *round_tokens = TOK; *flush_bytes = FLUSH;
    return 0;
}

extern "C" int mg_pngdec_inflate(const uint8_t* data, long data_bytes, const int32_t* recs, uint8_t* raw, long raw_stride, int32_t* info, long planes,
                                 int h, int w, void* stream) {
    if (pd_bad_args(planes, h, w, raw_stride) || data_bytes < 0 || data_bytes > MG_PNGDEC_MAX_BYTES) return -2;
    if (!data || !recs || !raw || !info || (uintptr_t)data % 4 != 0 || (uintptr_t)raw % 16 != 0 || (uintptr_t)recs % 4 != 0 || (uintptr_t)info % 4 != 0) return -2;
    if (planes > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(pd_inflate_kernel, dim3((unsigned)planes), dim3(WV), 0, (hipStream_t)stream, data, data_bytes, recs, raw, raw_stride, info, h, w);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_pngdec_unfilter(const uint8_t* raw, long raw_stride, const int32_t* recs, uint8_t* out, int32_t* info, long planes, int h, int w,
                                  void* stream) {
    if (pd_bad_args(planes, h, w, raw_stride)) return -2;
    if (!raw || !recs || !out || !info || (const void*)raw == (const void*)out || (uintptr_t)recs % 4 != 0 || (uintptr_t)info % 4 != 0) return -2;
    if (planes > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(pd_unfilter_kernel, dim3((unsigned)planes), dim3(WV), 0, (hipStream_t)stream, raw, raw_stride, recs, out, info, h, w);
    MG_CHECK_LAUNCH();
    return 0;
}
