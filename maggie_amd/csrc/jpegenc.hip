// Baseline JPEG encoding on the device: frames [T][h][w][3] uint8 RGB -> the entropy-coded segments of the files Pillow's
//   `Image.save(path, quality=q)` writes (4:2:0, the Annex K Huffman tables, no optimisation, no restart markers), byte for byte. Replaces the
//   pixel pass behind the synthesis tools' `.save('....jpg')` (tools/synthesize_image_him.py:93-109, tools/synthesize_video_him.py:189). The 623
//   header bytes are the host's (maggie_amd/utils/jpegenc.py); DESIGN.md section 28 holds the rules, the LDS layouts and the measurements;
//   tests/jpegenc_restatement.py states the same encoder sequentially.
//
// je_coef_kernel   the load phase, the forward transform and the quantisation of photometric.hip's jpeg_ycc_kernel (restated here: the same
//   32 x 64 tile of whole MCUs, one lane per 8-point pass, the [8][9] / 72-dword LDS pitch, the __umulhi division), then the quantised terms
//   go back through LDS so that a lane stores one ROW of a block as one 16-byte word: int16 [T][blocks][64], MCUs row by row, y0 y1 y2 y3 cb cr
//   in an MCU, natural order in a block, DC terms not differenced -- what mg_jpegdec_dcsum leaves. A luma block beyond ceil(w / 8) block
//   columns or ceil(h / 8) block rows is a dummy block: zeros, and the DC of the block before it in the MCU.
// je_bits_kernel   one WAVE per block, lane z its zig-zag term z. The 64-bit ballot of "term != 0" gives every lane its run from a
//   leading-zero count; lane 0 codes the DC difference (the predecessor's DC is read from global memory), lane 63 the end-of-block when term 63
//   is zero. The wave's sum is the block's bit count.
// je_scan_kernel   per frame (one workgroup): the exclusive sum of the bit counts -> every block's bit offset; the frame's bits and bytes.
// je_pack_kernel   a workgroup ORs the codes of MG_JPEGENC_PACK_BLOCKS blocks MSB-first into an LDS image at the offsets of the scan plus a
//   wave prefix sum, then flushes it byte-swapped: interior words with plain (16-byte where aligned) stores, the first and the last word with a
//   global atomicOr on the zeroed buffer, because neighbouring workgroups share them. The frame's last block fills the last byte with 1-bits.
// je_count_kernel / je_chunk_kernel / je_base_kernel   the 0xFF bytes of every MG_JPEGENC_CHUNK_BYTES chunk of the unstuffed stream, their
//   exclusive sum per frame, each frame's final size (+ 2 for EOI) and its offset in the output.
// je_stuff_kernel  a lane copies its 16 bytes to their final place, a 0x00 behind every 0xFF; the lane with the last byte appends FF D9.
// No workgroup waits for another inside a launch.
#ifndef MG_HOST_EMU                                                        // tests/csrc/jpegenc_host.cpp compiles this file for the host
#include "common.h"
#include "../../include/maggie_hip.h"
#endif

namespace {
#include "jpeg_common.h"

// ---- the transform half: photometric.hip's tiles, jpeg_common.h's passes ----------------------------------------------------------------------
constexpr int TH = MG_JPEG_TILE_ROWS, TW = MG_JPEG_TILE_COLS;
constexpr int NYB = (TH / 8) * (TW / 8), NCB = (TH / 16) * (TW / 16);
constexpr int NB = NYB + 2 * NCB;
constexpr int NT = MG_JPEG_THREADS;
constexpr int RP = 9, BP = 8 * RP;
static_assert(TH == 32 && TW == 64 && NT == NB * 8 && NT % 64 == 0, "384 lanes: 48 blocks of 8 lines");

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(NT) void je_coef_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ lut, const int16_t* __restrict__ noise,
                                                     int nc, const int32_t* __restrict__ qtab, int16_t* __restrict__ coef, int h, int w, int mx,
                                                     int my, int tiles_x, int tiles) {
    __shared__ int s_blk[NB * BP];
    __shared__ int s_q[128];
    __shared__ unsigned s_m[128];
    const int tid = threadIdx.x;
    const long t = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - t * tiles);
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
    if (tid < 128) {
        const int q = min(max(qtab[tid], 1), 255);
        s_q[tid] = q;
        s_m[tid] = 0xFFFFFFFFu / (unsigned)(8 * q) + 1u;                    // ceil(2^32 / qv)
    }
    const uint8_t* __restrict__ src = in + t * ((long)h * w * 3);
    const int g1 = (nc == 3) ? 1 : 0, g2 = (nc == 3) ? 2 : 0;

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

    // ---- load, convert, downsample (section 19's edge rules) ----
    const int chr = (h + 1) >> 1;
    for (int k = tid; k < (TH / 2) * (TW / 2); k += NT) {
        const int qy = k / (TW / 2), qx = k - qy * (TW / 2);
        const int gy = (ty0 >> 1) + qy, gx = (tx0 >> 1) + qx;
        const int x0 = min(2 * gx, w - 1), x1 = min(2 * gx + 1, w - 1);
        const int y0 = min(2 * gy, h - 1), y1 = min(2 * gy + 1, h - 1);
        int Y[4], cb[4], cr[4];
        pixel(y0, x0, Y[0], cb[0], cr[0]);
        pixel(y0, x1, Y[1], cb[1], cr[1]);
        pixel(y1, x0, Y[2], cb[2], cr[2]);
        pixel(y1, x1, Y[3], cb[3], cr[3]);
        if (gy >= chr && !(h & 1)) {                                        // below an even image: the last downsampled row
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
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[l * RP + k];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[l * RP + k] = d[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[k * RP + l];
    fdct8<false>(d);
    const int sel = b >= NYB ? 64 : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = s_q[sel + k * 8 + l];
        const unsigned n = (unsigned)abs(d[k]) + (unsigned)(4 * q);        // |c| + qv / 2, far below 2^32 / 2040
        const int kq = (int)__umulhi(n, s_m[sel + k * 8 + l]);             // n / (8 q)
        blk[k * RP + l] = d[k] < 0 ? -kq : kq;
    }
    __syncthreads();

    // ---- one row of a block per lane -> one 16-byte store ----
    int mrow, mcol, slot, srcb = b;
    bool dummy = false;
    if (b < NYB) {
        const int brow = b / (TW / 8), bcol = b % (TW / 8);
        const int gbr = (ty0 >> 3) + brow, gbc = (tx0 >> 3) + bcol;
        const int bh = (h + 7) >> 3, bw = (w + 7) >> 3;
        mrow = gbr >> 1; mcol = gbc >> 1; slot = (gbr & 1) * 2 + (gbc & 1);
        int s = slot;
        while (s > 0 && !((2 * mrow + (s >> 1)) < bh && (2 * mcol + (s & 1)) < bw)) --s;        // slot 0 of a real MCU is real
        dummy = s != slot;
        srcb = ((brow & ~1) + (s >> 1)) * (TW / 8) + (bcol & ~1) + (s & 1);
    } else {
        const int c = (b - NYB) / NCB, cb = (b - NYB) % NCB;
        mrow = (ty0 >> 4) + cb / (TW / 16); mcol = (tx0 >> 4) + cb % (TW / 16); slot = 4 + c;
    }
    if (mrow >= my || mcol >= mx) return;
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = dummy ? 0 : blk[l * RP + k];
    if (dummy && l == 0) v[0] = s_blk[srcb * BP];
    uint4 o;
    o.x = (uint32_t)(v[0] & 0xffff) | ((uint32_t)v[1] << 16);
    o.y = (uint32_t)(v[2] & 0xffff) | ((uint32_t)v[3] << 16);
    o.z = (uint32_t)(v[4] & 0xffff) | ((uint32_t)v[5] << 16);
    o.w = (uint32_t)(v[6] & 0xffff) | ((uint32_t)v[7] << 16);
    const long gblk = (t * my + mrow) * (long)mx * 6 + (long)mcol * 6 + slot;
    *reinterpret_cast<uint4*>(coef + gblk * 64 + l * 8) = o;
}

// ---- the Huffman tables: ISO/IEC 10918-1 Annex K.3 - K.6, canonical codes (Annex C) built at compile time -------------------------------------------
struct HuffTab { uint32_t e[256]; };                                       // symbol -> code | length << 16
template <int N>
constexpr HuffTab make_tab(const uint8_t (&counts)[16], const uint8_t (&vals)[N]) {
    HuffTab t{};
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < counts[l - 1]; ++i) { t.e[vals[k]] = code | ((unsigned)l << 16); ++code; ++k; }
        code <<= 1;
    }
    return t;
}
constexpr uint8_t DC_L_N[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t DC_C_N[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t DC_V[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_L_N[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t AC_L_V[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t AC_C_N[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t AC_C_V[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr HuffTab T_DC_L = make_tab(DC_L_N, DC_V), T_AC_L = make_tab(AC_L_N, AC_L_V), T_DC_C = make_tab(DC_C_N, DC_V), T_AC_C = make_tab(AC_C_N, AC_C_V);
static_assert(T_AC_L.e[0x00] == (0xAu | (4u << 16)) && T_AC_L.e[0xF0] == (0x7F9u | (11u << 16)) && T_AC_L.e[0xFA] == (0xFFFEu | (16u << 16)), "K.5");
static_assert(T_AC_C.e[0x00] == (0x0u | (2u << 16)) && T_AC_C.e[0xF0] == (0x3FAu | (10u << 16)) && T_DC_L.e[11] == (0x1FEu | (9u << 16)) &&
              T_DC_C.e[11] == (0x7FEu | (11u << 16)), "K.3, K.4, K.6");
// DC luma, AC luma, DC chroma, AC chroma: 4 x 256 words
__device__ const HuffTab JE_TABS[4] = {T_DC_L, T_AC_L, T_DC_C, T_AC_C};

__device__ const uint8_t JE_ZIGZAG[64] = MG_JPEG_ZIGZAG;

constexpr int ET = MG_JPEGENC_THREADS;                                     // the entropy kernels: four waves
constexpr int PBK = MG_JPEGENC_PACK_BLOCKS;                                // blocks of a packing workgroup
constexpr int CH = MG_JPEGENC_CHUNK_BYTES;                                 // bytes of a stuffing chunk: 16 per lane
constexpr int MAXB = MG_JPEGENC_MAX_BLOCK_BITS;
constexpr int IMG_WORDS = (31 + PBK * MAXB + 7 + 31) / 32 + 2;             // the start inside a word, the blocks, the fill, and two words of slack
constexpr int ST = 1024, SI = 4;                                           // the scan workgroup: lanes, items per lane
static_assert(ET == 256 && PBK % (ET / 64) == 0 && CH == ET * 16 && MAXB == 20 + 63 * 26, "four waves, 16 bytes a lane");

__device__ __forceinline__ void je_load_tabs(uint32_t* tabs, int tid) {
    const uint32_t* g = &JE_TABS[0].e[0];
    for (int i = tid; i < 1024; i += ET) tabs[i] = g[i];
    __syncthreads();
}

// lane `z` of the wave that owns block `blk` of its frame (coefficients at `cf`, the frame's at `frame`): the code bits of zig-zag term z,
// at most 59 of them, right-aligned in *val -> their number. Lane 0: the DC difference; lane 63: the end-of-block when term 63 is zero.
__device__ __forceinline__ int je_lane_code(const int16_t* __restrict__ frame, long blk, int z, const uint32_t* tabs, unsigned long long* val) {
    const int16_t* __restrict__ cf = frame + blk * 64;
    int v = cf[JE_ZIGZAG[z]];
    const int slot = (int)(blk % 6);
    const uint32_t* dc = tabs + (slot < 4 ? 0 : 512);
    const uint32_t* ac = dc + 256;
    if (z == 0) {
        const long back = slot == 0 ? 3 : (slot < 4 ? 1 : 6);               // the block before it of the same component, in scan order
        const int pred = (slot >= 1 && slot <= 3) || blk >= 6 ? (int)frame[(blk - back) * 64] : 0;
        v -= pred;
    }
    const unsigned long long mask = __ballot(v != 0) | 1ull;               // bit 0 stands for the DC term: runs count from term 1
    const int a = abs(v);
    const int n = 32 - __clz(a);                                           // the category; 0 for 0
    const unsigned mag = (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
    unsigned long long code = 0;
    int nb = 0;
    if (z == 0) {
        const uint32_t e = dc[min(n, 11)];
        code = e & 0xffffu; nb = (int)(e >> 16);
        code = (code << n) | mag; nb += n;
    } else if (v != 0) {
        const unsigned long long below = mask & ((1ull << z) - 1ull);      // never 0: bit 0
        const int run = z - (63 - __clzll(below)) - 1;
        const uint32_t zrl = ac[0xF0], e = ac[((run & 15) << 4) | min(n, 10)];
        for (int k = run >> 4; k > 0; --k) { code = (code << (zrl >> 16)) | (zrl & 0xffffu); nb += (int)(zrl >> 16); }
        code = (code << (e >> 16)) | (e & 0xffffu); nb += (int)(e >> 16);
        code = (code << n) | mag; nb += n;
    } else if (z == 63) {
        const uint32_t e = ac[0x00];
        code = e & 0xffffu; nb = (int)(e >> 16);
    }
    *val = code;
    return nb;
}

__device__ __forceinline__ int je_wave_incl(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
    return x;
}

__global__ __launch_bounds__(ET) void je_bits_kernel(const int16_t* __restrict__ coef, int32_t* __restrict__ bits, long nblk, long total) {
    __shared__ uint32_t tabs[1024];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    je_load_tabs(tabs, tid);
    for (int i = wv; i < PBK; i += ET / 64) {
        const long g = (long)blockIdx.x * PBK + i;                         // wave-uniform
        if (g >= total) break;
        const long t = g / nblk, blk = g - t * nblk;
        unsigned long long val;
        const int nb = je_lane_code(coef + t * nblk * 64, blk, lane, tabs, &val);
        const int sum = je_wave_incl(nb, lane);
        if (lane == 63) bits[g] = sum;
    }
}

// the exclusive sum of n values, ST lanes with SI consecutive values each per round; every lane gets the total. `ws`: ST / 64 words of LDS.
template <typename L, typename S>
__device__ __forceinline__ long long je_scan(long n, L load, S store, long long* ws) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long carry = 0;
    for (long base = 0; base < n; base += (long)ST * SI) {
        long long v[SI], mine = 0;
#pragma unroll
        for (int k = 0; k < SI; ++k) { const long i = base + (long)tid * SI + k; v[k] = i < n ? load(i) : 0; mine += v[k]; }
        long long x = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
        __syncthreads();
        if (lane == 63) ws[wv] = x;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < ST / 64; ++k) { const long long s = ws[k]; if (k < wv) before += s; all += s; }
        long long at = carry + before + x - mine;
#pragma unroll
        for (int k = 0; k < SI; ++k) { const long i = base + (long)tid * SI + k; if (i < n) store(i, at); at += v[k]; }
        carry += all;
    }
    return carry;
}

// sizes: int64 [4][frames]: [0] the bytes of the frame's scan in the file (stuffed, with EOI), [1] its unstuffed bytes, [2] its bits, [3] its offset
__global__ __launch_bounds__(ST) void je_scan_kernel(const int32_t* __restrict__ bits, int64_t* __restrict__ offs, int64_t* __restrict__ sizes,
                                                     long nblk, long frames) {
    __shared__ long long ws[ST / 64];
    const long t = blockIdx.x;
    const int32_t* __restrict__ b = bits + t * nblk;
    int64_t* __restrict__ o = offs + t * nblk;
    const long long tot = je_scan(nblk, [&](long i) { return (long long)b[i]; }, [&](long i, long long v) { o[i] = v; }, ws);
    if (threadIdx.x == 0) { sizes[2 * frames + t] = tot; sizes[frames + t] = (tot + 7) >> 3; }
}

// `nb` bits, right-aligned in `val`, at bit `bit` of the image (bit 0 = the most significant bit of word 0)
__device__ __forceinline__ void je_put(uint32_t* img, int bit, unsigned long long val, int nb) {
    if (nb <= 0 || bit < 0) return;
    const int w = bit >> 5, sh = bit & 31;
    if (w + 2 >= IMG_WORDS) return;
    const unsigned long long V = val << (64 - nb);
    const uint32_t w0 = (uint32_t)((V >> 32) >> sh), w1 = (uint32_t)(V >> sh), w2 = sh ? (uint32_t)(V << (32 - sh)) : 0u;
    if (w0) atomicOr(&img[w], w0);
    if (w1) atomicOr(&img[w + 1], w1);
    if (w2) atomicOr(&img[w + 2], w2);
}

__global__ __launch_bounds__(ET) void je_pack_kernel(const int16_t* __restrict__ coef, const int32_t* __restrict__ bits, const int64_t* __restrict__ offs,
                                                     uint8_t* __restrict__ raw, long raw_stride, long nblk, int groups) {
    __shared__ uint32_t tabs[1024];
    __shared__ __attribute__((aligned(16))) uint32_t img[IMG_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long t = blockIdx.x / (unsigned)groups;
    const long first = (long)(blockIdx.x - (unsigned)t * (unsigned)groups) * PBK;
    const int count = (int)(nblk - first < PBK ? nblk - first : PBK);
    for (int i = tid; i < IMG_WORDS; i += ET) img[i] = 0;
    je_load_tabs(tabs, tid);                                               // its barrier also orders the zeroing
    const int64_t* __restrict__ fo = offs + t * nblk;
    const int32_t* __restrict__ fb = bits + t * nblk;
    const long long start = fo[first];
    long long end = fo[first + count - 1] + fb[first + count - 1];
    const int fill = first + count == nblk ? (int)(-end & 7) : 0;         // the frame's last byte is filled with 1-bits
    const long word0 = (long)(start >> 5);
    for (int i = wv; i < count; i += ET / 64) {
        unsigned long long val;
        const int nb = je_lane_code(coef + t * nblk * 64, first + i, lane, tabs, &val);
        const int at = (int)(fo[first + i] - (word0 << 5)) + je_wave_incl(nb, lane) - nb;
        je_put(img, at, val, nb);
    }
    if (tid == 0 && fill) je_put(img, (int)(end - (word0 << 5)), (1ull << fill) - 1ull, fill);
    end += fill;
    __syncthreads();
    int nw = (int)(((end + 31) >> 5) - word0);
    if (nw > IMG_WORDS) nw = IMG_WORDS;
    const long cap = raw_stride >> 2;                                      // words of the frame's slice
    uint32_t* outw = reinterpret_cast<uint32_t*>(raw + t * raw_stride);
    if (tid == 0 && nw > 0 && word0 < cap && img[0]) atomicOr(&outw[word0], __builtin_bswap32(img[0]));
    if (tid == 1 && nw > 1 && word0 + nw - 1 < cap && img[nw - 1]) atomicOr(&outw[word0 + nw - 1], __builtin_bswap32(img[nw - 1]));
    // the interior [1, nw - 1): single words up to the first 16-byte boundary of the output, 16-byte stores, single words again
    const int lo = 1, hi = nw - 1;
    int mid = lo + (int)((4 - ((word0 + lo) & 3)) & 3);
    if (mid > hi) mid = hi;
    const int quads = hi > mid ? (hi - mid) >> 2 : 0;
    const int tail = mid + 4 * quads;
    for (int i = lo + tid; i < mid; i += ET)
        if (word0 + i < cap) outw[word0 + i] = __builtin_bswap32(img[i]);
    for (int q = tid; q < quads; q += ET) {
        const int i = mid + 4 * q;
        if (word0 + i + 3 < cap) {
            uint4 v;
            v.x = __builtin_bswap32(img[i]); v.y = __builtin_bswap32(img[i + 1]); v.z = __builtin_bswap32(img[i + 2]); v.w = __builtin_bswap32(img[i + 3]);
            *reinterpret_cast<uint4*>(outw + word0 + i) = v;
        }
    }
    for (int i = tail + tid; i < hi; i += ET)
        if (word0 + i < cap) outw[word0 + i] = __builtin_bswap32(img[i]);
}

// the lane's 16 bytes of chunk c of frame t (zeros behind the stream's end) and how many of them belong to the stream
__device__ __forceinline__ int je_chunk_load(const uint8_t* __restrict__ raw, long raw_stride, long t, long c, long long ub, int tid, uint32_t (&wd)[4]) {
    const long long at = (long long)c * CH + (long long)tid * 16;
    wd[0] = wd[1] = wd[2] = wd[3] = 0;
    if (at >= ub || at + 16 > raw_stride) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + t * raw_stride + at);
    wd[0] = v.x; wd[1] = v.y; wd[2] = v.z; wd[3] = v.w;
    return (int)(ub - at < 16 ? ub - at : 16);
}
__device__ __forceinline__ int je_count_ff(const uint32_t (&wd)[4], int n) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) c += (k < n && ((wd[k >> 2] >> (8 * (k & 3))) & 255u) == 255u) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(ET) void je_count_kernel(const uint8_t* __restrict__ raw, long raw_stride, const int64_t* __restrict__ sizes,
                                                      int32_t* __restrict__ ffcount, long frames, long chunks) {
    __shared__ int wt[ET / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long t = blockIdx.x / chunks, c = blockIdx.x - t * chunks;
    const long long ub = sizes[frames + t];
    if ((long long)c * CH >= ub) return;                                   // uniform
    uint32_t wd[4];
    const int n = je_chunk_load(raw, raw_stride, t, c, ub, tid, wd);
    const int x = je_wave_incl(je_count_ff(wd, n), lane);
    if (lane == 63) wt[wv] = x;
    __syncthreads();
    if (tid == 0) ffcount[t * chunks + c] = wt[0] + wt[1] + wt[2] + wt[3];
}

__global__ __launch_bounds__(ST) void je_chunk_kernel(const int32_t* __restrict__ ffcount, int64_t* __restrict__ choff, int64_t* __restrict__ sizes,
                                                      long frames, long chunks) {
    __shared__ long long ws[ST / 64];
    const long t = blockIdx.x;
    const long long ub = sizes[frames + t];
    long n = (long)((ub + CH - 1) / CH);
    if (n > chunks) n = chunks;
    const int32_t* __restrict__ f = ffcount + t * chunks;
    int64_t* __restrict__ o = choff + t * chunks;
    const long long tot = je_scan(n, [&](long i) { return (long long)f[i]; }, [&](long i, long long v) { o[i] = v; }, ws);
    if (threadIdx.x == 0) sizes[t] = ub + tot + 2;
}

__global__ __launch_bounds__(ST) void je_base_kernel(int64_t* __restrict__ sizes, long frames) {
    __shared__ long long ws[ST / 64];
    je_scan(frames, [&](long i) { return (long long)sizes[i]; }, [&](long i, long long v) { sizes[3 * frames + i] = v; }, ws);
}

__global__ __launch_bounds__(ET) void je_stuff_kernel(const uint8_t* __restrict__ raw, long raw_stride, const int64_t* __restrict__ choff,
                                                      const int64_t* __restrict__ sizes, uint8_t* __restrict__ out, long out_bytes, long frames,
                                                      long chunks, long grid_chunks) {
    __shared__ int wt[ET / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long t = blockIdx.x / grid_chunks, c = blockIdx.x - t * grid_chunks;
    const long long ub = sizes[frames + t];
    if (c >= chunks || (long long)c * CH >= ub) return;                    // uniform
    uint32_t wd[4];
    const int n = je_chunk_load(raw, raw_stride, t, c, ub, tid, wd);
    const int mine = je_count_ff(wd, n);
    const int x = je_wave_incl(mine, lane);
    if (lane == 63) wt[wv] = x;
    __syncthreads();
    int before = x - mine;
    for (int k = 0; k < wv; ++k) before += wt[k];
    long long at = sizes[3 * frames + t] + choff[t * chunks + c] + (long long)c * CH + (long long)tid * 16 + before;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < n) {
            const uint8_t b = (uint8_t)((wd[k >> 2] >> (8 * (k & 3))) & 255u);
            if (at < out_bytes) out[at] = b;
            ++at;
            if (b == 255) { if (at < out_bytes) out[at] = 0; ++at; }
        }
    }
    if (n > 0 && (long long)c * CH + (long long)tid * 16 + n == ub) {      // the stream's last byte is this lane's: EOI
        if (at < out_bytes) out[at] = 0xFF;
        if (at + 1 < out_bytes) out[at + 1] = 0xD9;
    }
}

struct Geo { long mx, my, nblk; };
bool je_bad_size(long frames, int h, int w) { return frames < 1 || frames > MG_JPEGENC_MAX_FRAMES || h < 1 || w < 1 || h > MG_JPEG_MAX_SIDE || w > MG_JPEG_MAX_SIDE; }
Geo je_geo(int h, int w) { Geo g; g.mx = (w + 15) / 16; g.my = (h + 15) / 16; g.nblk = g.mx * g.my * 6; return g; }
long je_raw_stride(long nblk) { return ((nblk * MAXB + 7) / 8 + 4 + 15) / 16 * 16; }

}  // namespace

extern "C" int mg_jpegenc_limits(int* threads, int* pack_blocks, int* chunk_bytes, int* max_block_bits, int* max_side, int* max_frames) {
    if (!threads || !pack_blocks || !chunk_bytes || !max_block_bits || !max_side || !max_frames) return -2;
    *threads = ET; *pack_blocks = PBK; *chunk_bytes = CH; *max_block_bits = MAXB; *max_side = MG_JPEG_MAX_SIDE; *max_frames = MG_JPEGENC_MAX_FRAMES;
    return 0;
}

extern "C" int mg_jpegenc_coef(const uint8_t* in, const uint8_t* lut, const int16_t* noise, int noise_channels, const int32_t* qtab, int16_t* coef,
                               long coef_elems, long frames, int h, int w, void* stream) {
    if (je_bad_size(frames, h, w) || (noise && noise_channels != 1 && noise_channels != 3)) return -2;
    const Geo g = je_geo(h, w);
    if (!in || !qtab || !coef || (uintptr_t)coef % 16 != 0 || (uintptr_t)qtab % 4 != 0 || coef_elems != frames * g.nblk * 64) return -2;
    const int tiles_x = (int)((g.mx * 16 + TW - 1) / TW);
    const long tiles = (long)tiles_x * ((g.my * 16 + TH - 1) / TH);
    if (frames > 0x7fffffffL / tiles) return -3;
    hipLaunchKernelGGL(je_coef_kernel, dim3((unsigned)(frames * tiles)), dim3(NT), 0, (hipStream_t)stream, in, lut, noise, noise_channels, qtab, coef,
                       h, w, (int)g.mx, (int)g.my, tiles_x, (int)tiles);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_jpegenc_bits(const int16_t* coef, long coef_elems, int32_t* bits, int64_t* offs, int64_t* sizes, long frames, int h, int w,
                               void* stream) {
    if (je_bad_size(frames, h, w)) return -2;
    const Geo g = je_geo(h, w);
    if (!coef || !bits || !offs || !sizes || coef_elems != frames * g.nblk * 64) return -2;
    if ((uintptr_t)coef % 2 != 0 || (uintptr_t)bits % 4 != 0 || (uintptr_t)offs % 8 != 0 || (uintptr_t)sizes % 8 != 0) return -2;
    const long total = frames * g.nblk, grid = (total + PBK - 1) / PBK;
    if (grid > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(je_bits_kernel, dim3((unsigned)grid), dim3(ET), 0, (hipStream_t)stream, coef, bits, g.nblk, total);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(je_scan_kernel, dim3((unsigned)frames), dim3(ST), 0, (hipStream_t)stream, (const int32_t*)bits, offs, sizes, g.nblk, frames);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_jpegenc_pack(const int16_t* coef, long coef_elems, const int32_t* bits, const int64_t* offs, int64_t* sizes, uint8_t* raw,
                               long raw_stride, int32_t* ffcount, int64_t* choff, long frames, int h, int w, void* stream) {
    if (je_bad_size(frames, h, w)) return -2;
    const Geo g = je_geo(h, w);
    if (!coef || !bits || !offs || !sizes || !raw || !ffcount || !choff || coef_elems != frames * g.nblk * 64) return -2;
    if ((uintptr_t)coef % 2 != 0 || (uintptr_t)bits % 4 != 0 || (uintptr_t)offs % 8 != 0 || (uintptr_t)sizes % 8 != 0 || (uintptr_t)raw % 16 != 0 ||
        (uintptr_t)ffcount % 4 != 0 || (uintptr_t)choff % 8 != 0)
        return -2;
    if (raw_stride % 16 != 0 || raw_stride < je_raw_stride(g.nblk)) return -2;
    const long groups = (g.nblk + PBK - 1) / PBK, chunks = (raw_stride + CH - 1) / CH;
    if (frames * groups > 0x7fffffffL || frames * chunks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(je_pack_kernel, dim3((unsigned)(frames * groups)), dim3(ET), 0, (hipStream_t)stream, coef, bits, offs, raw, raw_stride, g.nblk,
                       (int)groups);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(je_count_kernel, dim3((unsigned)(frames * chunks)), dim3(ET), 0, (hipStream_t)stream, (const uint8_t*)raw, raw_stride,
                       (const int64_t*)sizes, ffcount, frames, chunks);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(je_chunk_kernel, dim3((unsigned)frames), dim3(ST), 0, (hipStream_t)stream, (const int32_t*)ffcount, choff, sizes, frames, chunks);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(je_base_kernel, dim3(1), dim3(ST), 0, (hipStream_t)stream, sizes, frames);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_jpegenc_stuff(const uint8_t* raw, long raw_stride, const int64_t* choff, const int64_t* sizes, uint8_t* out, long out_bytes,
                                long frames, int h, int w, long grid_chunks, void* stream) {
    if (je_bad_size(frames, h, w)) return -2;
    const Geo g = je_geo(h, w);
    if (!raw || !choff || !sizes || !out || (uintptr_t)raw % 16 != 0 || (uintptr_t)choff % 8 != 0 || (uintptr_t)sizes % 8 != 0) return -2;
    if (raw_stride % 16 != 0 || raw_stride < je_raw_stride(g.nblk) || out_bytes < 1) return -2;
    const long chunks = (raw_stride + CH - 1) / CH;
    if (grid_chunks < 1 || grid_chunks > chunks) return -2;
    if (frames * grid_chunks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(je_stuff_kernel, dim3((unsigned)(frames * grid_chunks)), dim3(ET), 0, (hipStream_t)stream, raw, raw_stride, choff, sizes, out,
                       out_bytes, frames, chunks, grid_chunks);
    MG_CHECK_LAUNCH();
    return 0;
}
