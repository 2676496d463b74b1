// Baseline JPEG decoding on the device: the entropy-coded segment of T files of one geometry, in any of the six layouts of include/maggie_hip.h
//   (jpeg_common.h maps a layout to its geometry) -> coefficients -> component planes -> RGB. The lossy half (dequantisation, JDCT_ISLOW inverse
//   transform, upsampling, YCbCr -> RGB) is photometric.hip's, pinned to Pillow; this file adds the Huffman decoding in
//   the self-synchronising parallel form of Weissenberger and Schmidt and runs jpeg_common.h's inverse passes on blocks that arrive
//   as coefficients (DESIGN.md sections 25, 31 and 33).
//
// A frame's segment is cut into subsequences of `sub_bytes` raw bytes; one lane owns one subsequence. A lane's state is (bit position, block
//   slot within the MCU, zig-zag index); the number of blocks it completed is kept next to it. Bit positions count RAW bits: a stuffed 0x00
//   (the byte after a data 0xFF) is skipped by the reader, and 0xFF 0xD0..0xD7 stops it -- a symbol that does not fit in front of a restart
//   marker can only be the padding of an interval's last byte (the all-ones code is never assigned), so the lane steps over the marker into
//   slot 0, index 0. Every loop runs under a bound from the sizes passed in; no workgroup waits for another.
//
// jd_sync_kernel   launch 0: every lane decodes its subsequence from its first bit assuming slot 0 / index 0 (right for subsequence 0). Then,
//   in every launch, rounds inside the workgroup: lane l takes the exit state of lane l - 1 as its entry and decodes again when that entry is
//   new to it; the rounds end when one changes nothing (at most MG_JPEGDEC_THREADS of them: a change travels one lane per round). Lane 0's
//   entry is the exit of the previous workgroup as the PREVIOUS launch left it (two buffers, read one, write the other: no word is read and
//   written in one launch). A launch after which no workgroup's exit moved ends the synchronisation; the host bounds the launches.
// jd_prefix_kernel exclusive sum of the per-subsequence block counts of a frame.  jd_coef_kernel the same decode once more from the now right
//   entries, writing int16 coefficients de-zig-zagged into zero-filled blocks in scan order, the DC term as its DIFFERENCE; status bits.
// jd_dcsum_kernel  per frame and component: the segmented (per restart interval) inclusive sum that turns differences into DC terms.
// jd_idct_kernel   coefficient x table, columns (descale 11), rows (descale 18), + 128, range limit; one lane per 8-point pass on [8][9]-pitch
//   LDS blocks; writes the plane layout mg_jpeg_rgb (4:2:0), jd_rgb_kernel or mg_jpeg_rgb_hv (4:2:2, 4:4:0, 4:1:1: pitched planes) reads.
// jd_rgb_kernel    4:4:4 and greyscale planes -> raw bytes or the Normalize epilogue.
#ifndef MG_HOST_EMU
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"
#define MG_DEVCONST __device__ const
#endif

namespace {
#include "jpeg_common.h"

constexpr int NT = MG_JPEGDEC_THREADS;                                     // lanes = subsequences per workgroup of the decode kernels
constexpr int TW = MG_JPEGDEC_TAB_WORDS;                                   // int32 words of a frame's record
constexpr int W_SLOT = 4 * HT, W_OFF = W_SLOT + 6, W_LEN = W_OFF + 1, W_RI = W_OFF + 2, W_QT = 928;
constexpr int PT = 256;                                                    // lanes of the other kernels
constexpr int RP = 9, BP = 8 * RP;                                         // row and block pitch in dwords (photometric.hip's)
constexpr unsigned long long INVALID = ~0ull;
static_assert(W_QT + 192 == TW && NT % 64 == 0 && NT <= PT, "record layout");

MG_DEVCONST uint8_t NATURAL[64] = MG_JPEG_ZIGZAG;

// blocks per MCU, the MCU grid, luma blocks per MCU row and column, the row pitch of the luma plane and of a chroma plane in bytes
struct Geo { int bpm, mcux, mcuy, hs, vs, yp, cp; };
// the struct of a layout and the bytes of its planes (jpeg_common.h); bad_layout: anything but the six
bool bad_layout(int layout) { JpegLayout l; return !jpeg_layout(layout, 8, 8, l); }
Geo geo_of(int layout, int h, int w) {
    JpegLayout l = {};
    jpeg_layout(layout, h, w, l);
    return Geo{l.bpm, l.mcux, l.mcuy, l.hs, l.vs, l.yp, l.cp};
}
long plane_bytes_of(long frames, int layout, const Geo& g) {
    return frames * (long)g.mcuy * 8 * ((long)g.vs * g.yp + (layout == MG_JPEGDEC_GREY ? 0L : 2L) * g.cp);
}

// ---- the bit reader and one subsequence ------------------------------------------------------------------------------------------------------
constexpr int STOP_NONE = 0, STOP_RST = 1, STOP_END = 2;
struct Reader {
    unsigned long long W;                                                  // up to 8 DATA bytes from the one that holds `pos`, big-endian; 0xFF beyond `nb`
    unsigned sm;                                                           // bit k: data byte k is a 0xFF with its stuffed 0x00 behind it
    int nb, rp, stop;                                                      // data bytes held, the next raw byte to fetch, why fetching ended
};

__device__ __forceinline__ void rd_open(Reader& r, long pos) { r.W = ~0ull; r.sm = 0; r.nb = 0; r.rp = (int)(pos >> 3); r.stop = STOP_NONE; }

__device__ __forceinline__ void rd_fill(Reader& r, const uint8_t* __restrict__ d, int len) {
    while (r.nb < 8 && r.stop == STOP_NONE) {                              // at most 8 rounds
        if (r.rp >= len) { r.stop = STOP_END; break; }
        const unsigned b = d[r.rp];
        int step = 1;
        if (b == 0xFF) {
            const unsigned n = r.rp + 1 < len ? d[r.rp + 1] : 0xD9u;
            if (n == 0) { r.sm |= 1u << r.nb; step = 2; }
            else { r.stop = (n >= 0xD0 && n <= 0xD7) ? STOP_RST : STOP_END; break; }
        }
        const int s = 56 - 8 * r.nb;
        r.W = (r.W & ~(0xFFull << s)) | ((unsigned long long)b << s);
        r.nb += 1;
        r.rp += step;
    }
}

// the first raw position at or after byte q from which a lane may start: not a stuffed byte, not inside a restart marker
__device__ __forceinline__ long canonical_start(const uint8_t* __restrict__ d, int len, long q) {
    if (q >= len) return 8L * len;
    const unsigned b = d[q], p = q > 0 ? d[q - 1] : 0u;
    if (p == 0xFF && (b == 0 || (b >= 0xD0 && b <= 0xD7))) return 8 * (q + 1);
    if (b == 0xFF && q + 1 < len && d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7) return 8 * (q + 2) > 8L * len ? 8L * len : 8 * (q + 2);
    return 8 * q;
}

__device__ __forceinline__ unsigned long long pack_state(long pos, int slot, int zz) {
    return (unsigned long long)pos | ((unsigned long long)slot << 40) | ((unsigned long long)zz << 44);
}

// Decode from `st` to the first symbol that starts at or after bit `endbit`; returns the exit state, the blocks completed in `nblk`. WRITE: the
// coefficients go to coef[(blk0 + completed) * 64 + natural index] for block indices below `nbf`, and the checks set bits of `status`.
template <bool WRITE>
__device__ __forceinline__ unsigned long long run_sub(unsigned long long st, long endbit, const uint8_t* __restrict__ d, int len,
                                                      const int* __restrict__ tab, int bpm, int maxit, int& nblk, int16_t* __restrict__ coef,
                                                      int blk0, int nbf, int ri_blocks, int& status) {
    long pos = (long)(st & ((1ull << 40) - 1));
    int slot = (int)((st >> 40) & 7), zz = (int)((st >> 44) & 63);
    nblk = 0;
    if (slot >= bpm) slot = 0;
    if (pos > 8L * len) pos = 8L * len;
    Reader r;
    rd_open(r, pos);
    for (int it = 0; it < maxit && pos < endbit; ++it) {
        if (r.nb < 5) rd_fill(r, d, len);
        const int o = (int)(pos & 7);
        const unsigned bits = (unsigned)((r.W << o) >> 32);
        const int info = tab[W_SLOT + slot];
        const int* __restrict__ tb = tab + HT * (zz == 0 ? (info & 1) : 2 + ((info >> 4) & 1));
        // first level: the leading 8 bits; then the canonical walk over lengths 9..16
        int len_c = 0, sym = 0;
        const unsigned e = ((const uint16_t*)tb)[bits >> 24];
        if (e) { len_c = (int)(e >> 8); sym = (int)(e & 255u); }
        else {
            for (int l = 9; l <= 16; ++l) {
                const int code = (int)(bits >> (32 - l));
                if (code <= tb[HT_MAXCODE + l]) {
                    const int idx = tb[HT_VALOFF + l] + code;
                    if ((unsigned)idx < 256u) { len_c = l; sym = ((const uint8_t*)(tb + HT_VALS))[idx]; }
                    break;
                }
            }
        }
        bool bad = len_c == 0;
        if (bad) len_c = 16;                                               // an unassigned code: sixteen bits of nothing (status in the output pass)
        int s = zz == 0 ? sym : (sym & 15);
        const int run = zz == 0 ? 0 : (sym >> 4);
        if (s > 11) { s = 11; bad = true; }                                // 8-bit samples: categories 0..11
        const int n = len_c + s;
        if (o + n > 8 * r.nb) {                                            // the symbol does not fit in front of where the data stops
            if (r.stop == STOP_RST) {
                if (WRITE) {
                    const int done = blk0 + nblk, m = r.rp + 1 < len ? d[r.rp + 1] & 7 : 0;
                    if (slot != 0 || zz != 0 || ri_blocks <= 0 || done % (ri_blocks > 0 ? ri_blocks : 1) != 0 ||
                        ((done / (ri_blocks > 0 ? ri_blocks : 1) - 1) & 7) != m) status |= MG_JPEGDEC_ST_RESTART;
                }
                pos = 8L * (r.rp + 2);
                if (pos > 8L * len) pos = 8L * len;
                slot = 0; zz = 0;
                rd_open(r, pos);
                continue;
            }
            if (WRITE && blk0 + nblk < nbf) status |= MG_JPEGDEC_ST_PAST_END;
            pos = 8L * len;
            break;
        }
        if (WRITE && bad) status |= MG_JPEGDEC_ST_CODE;
        int v = s ? (int)((bits << len_c) >> (32 - s)) : 0;
        if (s && v < (1 << (s - 1))) v = v - (1 << s) + 1;
        const int blk = blk0 + nblk;
        if (zz == 0) {
            if (WRITE) { if (blk < nbf) coef[(long)blk * 64] = (int16_t)v; else status |= MG_JPEGDEC_ST_COUNT; }
            zz = 1;
        } else if (s == 0) {
            zz = run == 15 ? zz + 16 : 64;
            if (WRITE && zz > 64) status |= MG_JPEGDEC_ST_INDEX;
        } else {
            zz += run;
            if (zz > 63) { if (WRITE) status |= MG_JPEGDEC_ST_INDEX; }
            else if (WRITE) { if (blk < nbf) coef[(long)blk * 64 + NATURAL[zz]] = (int16_t)v; else status |= MG_JPEGDEC_ST_COUNT; }
            zz += 1;
        }
        if (zz >= 64) { zz = 0; nblk += 1; slot = slot + 1 >= bpm ? 0 : slot + 1; }
        // consume n bits: whole data bytes leave the window, with the stuffed bytes behind them
        const int kk = (o + n) >> 3;
        pos += n + 8 * __popc(r.sm & ((1u << kk) - 1u));
        if (kk) { r.W = (r.W << (8 * kk)) | ((1ull << (8 * kk)) - 1ull); r.sm >>= kk; r.nb -= kk; }
    }
    return pack_state(pos, slot, zz);
}

// a frame's record into LDS, and its segment checked against the buffer
__device__ __forceinline__ void load_tab(int* __restrict__ s_tab, const int32_t* __restrict__ tabs, long t, int words, long data_bytes, int& off,
                                         int& len) {
    for (int k = threadIdx.x; k < words; k += blockDim.x) s_tab[k] = tabs[t * TW + k];
    __syncthreads();
    off = s_tab[W_OFF]; len = s_tab[W_LEN];
    if (off < 0 || len < 0 || (long)off + len > data_bytes) { off = 0; len = 0; }
}

__global__ __launch_bounds__(NT) void jd_sync_kernel(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ tabs,
                                                     unsigned long long* __restrict__ E, int32_t* __restrict__ cnt,
                                                     unsigned long long* __restrict__ Ein, unsigned long long* __restrict__ Eb,
                                                     int32_t* __restrict__ info, int nsub, int sub_bytes, int wgs, int bpm, long frames, int launch) {
    __shared__ int s_tab[W_QT];
    __shared__ unsigned long long s_E[NT];
    const int l = threadIdx.x;
    const long t = blockIdx.x / wgs;
    const int g = (int)(blockIdx.x - t * wgs), j = g * NT + l;
    int off, len;
    load_tab(s_tab, tabs, t, W_QT, data_bytes, off, len);
    const uint8_t* __restrict__ d = data + off;
    const bool active = j < nsub, first = launch == 0;
    const long endbit = 8L * min((long)(j + 1) * sub_bytes, (long)len);
    const int maxit = 8 * sub_bytes + 8, last = min(NT, nsub - g * NT) - 1;
    const unsigned long long* __restrict__ Eb_in = Eb + (long)(launch & 1) * frames * wgs;
    unsigned long long* __restrict__ Eb_out = Eb + (long)((launch + 1) & 1) * frames * wgs;
    unsigned long long mine = INVALID, seen = INVALID, in0 = INVALID;
    int mycnt = 0, unused = 0;
    if (active) {
        if (first) {
            const unsigned long long st = j == 0 ? 0ull : pack_state(canonical_start(d, len, (long)j * sub_bytes), 0, 0);
            mine = run_sub<false>(st, endbit, d, len, s_tab, bpm, maxit, mycnt, nullptr, 0, 0, 0, unused);
            if (j == 0) seen = 0ull;
        } else {
            mine = E[t * nsub + j]; mycnt = cnt[t * nsub + j];
            seen = j == 0 ? 0ull : (l == 0 ? Ein[t * wgs + g] : E[t * nsub + j - 1]);
            if (l == 0 && g > 0) in0 = Eb_in[t * wgs + g - 1];
        }
    }
    s_E[l] = mine;
    __syncthreads();
    int rounds = 0;
    for (int r = 0; r < NT; ++r) {                                         // a change travels one lane per round
        const unsigned long long entry = l == 0 ? in0 : s_E[l - 1];
        int ch = 0;
        if (active && j > 0 && entry != INVALID && entry != seen) {
            const unsigned long long now = run_sub<false>(entry, endbit, d, len, s_tab, bpm, maxit, mycnt, nullptr, 0, 0, 0, unused);
            seen = entry;
            ch = now != mine;
            mine = now;
        }
        if (!__syncthreads_or(ch)) break;
        s_E[l] = mine;
        __syncthreads();
        rounds += 1;
    }
    if (active) {
        E[t * nsub + j] = mine; cnt[t * nsub + j] = mycnt;
        if (l == 0) Ein[t * wgs + g] = seen;
        if (l == last) {
            Eb_out[t * wgs + g] = mine;
            if (first || mine != Eb_in[t * wgs + g]) atomicOr(&info[2 + 2 * launch], 1);
        }
        if (l == 0 && rounds) atomicMax(&info[3 + 2 * launch], rounds);
    }
}

// exclusive sum of n counts per frame: a lane sums its chunk, lane 0 walks the PT chunk sums
__global__ __launch_bounds__(PT) void jd_prefix_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ blk0, int nsub) {
    __shared__ int s_sum[PT];
    const long t = blockIdx.x;
    const int l = threadIdx.x, chunk = (nsub + PT - 1) / PT, a = min(l * chunk, nsub), b = min(a + chunk, nsub);
    int s = 0;
    for (int k = a; k < b; ++k) s += cnt[t * nsub + k];
    s_sum[l] = s;
    __syncthreads();
    if (l == 0) {
        int run = 0;
        for (int k = 0; k < PT; ++k) { const int v = s_sum[k]; s_sum[k] = run; run += v; }
    }
    __syncthreads();
    s = s_sum[l];
    for (int k = a; k < b; ++k) { blk0[t * nsub + k] = s; s += cnt[t * nsub + k]; }
}

__global__ __launch_bounds__(NT) void jd_coef_kernel(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ tabs,
                                                     const unsigned long long* __restrict__ E, const int32_t* __restrict__ blk0,
                                                     int16_t* __restrict__ coef, int32_t* __restrict__ info, int nsub, int sub_bytes, int wgs, int bpm,
                                                     int nbf) {
    __shared__ int s_tab[W_QT];
    const int l = threadIdx.x;
    const long t = blockIdx.x / wgs;
    const int g = (int)(blockIdx.x - t * wgs), j = g * NT + l;
    int off, len;
    load_tab(s_tab, tabs, t, W_QT, data_bytes, off, len);
    if (j >= nsub) return;
    const uint8_t* __restrict__ d = data + off;
    const long endbit = 8L * min((long)(j + 1) * sub_bytes, (long)len);
    const unsigned long long st = j == 0 ? 0ull : E[t * nsub + j - 1];
    int status = 0, n = 0;
    int b0 = blk0[t * nsub + j];
    if (b0 < 0 || b0 > nbf) { b0 = nbf; status |= MG_JPEGDEC_ST_COUNT; }
    const int ri = s_tab[W_RI];
    const int ri_blocks = ri > 0 && ri <= 0x7fffffff / 8 ? ri * bpm : 0;
    run_sub<true>(st, endbit, d, len, s_tab, bpm, 8 * sub_bytes + 8, n, coef + t * (long)nbf * 64, b0, nbf, ri_blocks, status);
    if (j == nsub - 1 && b0 + n != nbf) status |= MG_JPEGDEC_ST_COUNT;
    if (status) atomicOr(&info[0], status);
}

// differences -> DC terms: one workgroup per (frame, component); a lane owns a run of the component's blocks in scan order, sums it within restart
// intervals, lane 0 carries the sums across lanes, then every lane rewrites its run
__global__ __launch_bounds__(PT) void jd_dcsum_kernel(int16_t* __restrict__ coef, const int32_t* __restrict__ tabs, int bpm, int mcus, int ncomp) {
    __shared__ int s_sum[PT], s_cut[PT];
    const long t = blockIdx.x / ncomp;
    const int c = (int)(blockIdx.x - t * ncomp), l = threadIdx.x;
    const int nbc = c == 0 ? bpm - (ncomp - 1) : 1, slot0 = c == 0 ? 0 : bpm - ncomp + c;      // blocks per MCU and first slot of the component
    const int ri = tabs[t * TW + W_RI];
    const int total = mcus * nbc, chunk = (total + PT - 1) / PT, a = min(l * chunk, total), b = min(a + chunk, total);
    int16_t* __restrict__ f = coef + t * (long)mcus * bpm * 64;
    int s = 0, cut = 0;
    for (int k = a; k < b; ++k) {
        const int mcu = k / nbc, sl = k - mcu * nbc;
        if (ri > 0 && sl == 0 && mcu % ri == 0) { s = 0; cut = 1; }
        s += f[((long)mcu * bpm + slot0 + sl) * 64];
    }
    s_sum[l] = s; s_cut[l] = cut;
    __syncthreads();
    if (l == 0) {
        int run = 0;
        for (int k = 0; k < PT; ++k) { const int v = s_sum[k], ct = s_cut[k]; s_sum[k] = run; run = ct ? v : run + v; }
    }
    __syncthreads();
    s = s_sum[l];
    for (int k = a; k < b; ++k) {
        const int mcu = k / nbc, sl = k - mcu * nbc;
        if (ri > 0 && sl == 0 && mcu % ri == 0) s = 0;
        int16_t* p = f + ((long)mcu * bpm + slot0 + sl) * 64;
        s += *p;
        *p = (int16_t)s;
    }
}

__global__ __launch_bounds__(PT) void jd_idct_kernel(const int16_t* __restrict__ coef, const int32_t* __restrict__ tabs, uint8_t* __restrict__ planes,
                                                     long frames, Geo g, long nblocks) {
    __shared__ int s_blk[(PT / 8) * BP];
    const int tid = threadIdx.x, b = tid >> 3, l = tid & 7;
    const long u = (long)blockIdx.x * (PT / 8) + b;
    const bool on = u < nblocks;
    const int bpf = g.mcux * g.mcuy * g.bpm;
    const long t = on ? u / bpf : 0;
    const int rb = on ? (int)(u - t * bpf) : 0, mcu = rb / g.bpm, slot = rb - mcu * g.bpm;
    const int ny = g.hs * g.vs, c = slot < ny ? 0 : slot - ny + 1;
    int* __restrict__ blk = s_blk + b * BP;
    int d[8];
    if (on) {
        const int16_t* __restrict__ src = coef + u * 64;
        const int32_t* __restrict__ q = tabs + t * TW + W_QT + 64 * c;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)src[k * 8 + l] * q[k * 8 + l];
        idct8<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) blk[k * RP + l] = d[k];
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = blk[l * RP + k];
        idct8<18>(d);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)range_limit(d[k]) << (8 * k);
            hi |= (uint32_t)range_limit(d[k + 4]) << (8 * k);
        }
        const int my = mcu / g.mcux, mx = mcu - my * g.mcux;
        const long pw = g.yp, ph = (long)g.mcuy * 8 * g.vs;                                      // the luma plane
        uint8_t* dst;
        if (c == 0) dst = planes + (t * ph + (my * g.vs + slot / g.hs) * 8 + l) * pw + (mx * g.hs + slot % g.hs) * 8;
        else {
            const long cw = g.cp, chh = (long)g.mcuy * 8;
            dst = planes + frames * ph * pw + (c - 1) * (frames * chh * cw) + (t * chh + my * 8 + l) * cw + mx * 8;
        }
        *(uint2*)dst = make_uint2(lo, hi);
    }
}

template <int EPI>
__global__ __launch_bounds__(PT) void jd_rgb_kernel(const uint8_t* __restrict__ planes, void* __restrict__ out, long frames, int h, int w, int ph,
                                                    int pw, int grey, long pixels, float m0, float m1, float m2, float s0, float s1, float s2) {
    const long u = (long)blockIdx.x * PT + threadIdx.x;
    if (u >= pixels) return;
    const long row = u / w, t = row / h;
    const int x = (int)(u - row * w), y = (int)(row - t * h);
    const long at = (t * ph + y) * (long)pw + x, plane = frames * (long)ph * pw;
    const int Y = planes[at];
    int r = Y, gg = Y, b = Y;
    if (!grey) {
        const int cb = (int)planes[plane + at] - 128, cr = (int)planes[2 * plane + at] - 128;
        r = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
        gg = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        b = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    }
    if constexpr (EPI == MG_PHOTO_RAW) {
        uint8_t* __restrict__ dst = (uint8_t*)out + u * 3;
        dst[0] = (uint8_t)r; dst[1] = (uint8_t)gg; dst[2] = (uint8_t)b;
    } else {
        float* __restrict__ dst = (float*)out + (t * 3 * h + y) * (long)w + x;
        const long cs = (long)h * w;
        dst[0] = mg_norm_u8(r, m0, s0); dst[cs] = mg_norm_u8(gg, m1, s1); dst[2 * cs] = mg_norm_u8(b, m2, s2);
    }
}

bool bad_sub(int nsub, int sub_bytes) {
    return nsub <= 0 || sub_bytes < MG_JPEGDEC_MIN_SUB || sub_bytes > MG_JPEGDEC_MAX_SUB || (long)nsub * sub_bytes > MG_JPEGDEC_MAX_BYTES;
}

// the launches behind the entry points, the geometry given
int launch_sync(const uint8_t* data, long data_bytes, const int32_t* tabs, unsigned long long* exits, int32_t* counts, unsigned long long* entries,
                unsigned long long* bounds, int32_t* info, long frames, int nsub, int sub_bytes, int bpm, int launch, void* stream) {
    if (!data || !tabs || !exits || !counts || !entries || !bounds || !info) return -2;
    const int wgs = (nsub + NT - 1) / NT;
    if (frames > 0x7fffffffL / wgs) return -3;
    hipLaunchKernelGGL(jd_sync_kernel, dim3((unsigned)(frames * wgs)), dim3(NT), 0, (hipStream_t)stream, data, data_bytes, tabs, exits, counts, entries,
                       bounds, info, nsub, sub_bytes, wgs, bpm, frames, launch);
    MG_CHECK_LAUNCH();
    return 0;
}

int launch_coef(const uint8_t* data, long data_bytes, const int32_t* tabs, const unsigned long long* exits, const int32_t* counts,
                int32_t* first_block, int16_t* coef, long coef_elems, int32_t* info, long frames, int nsub, int sub_bytes, const Geo& g, void* stream) {
    const long nbf = (long)g.mcux * g.mcuy * g.bpm;
    if (nbf > 0x7fffffffL / 64 || coef_elems != frames * nbf * 64) return -2;
    if (frames == 0) return 0;
    if (!data || !tabs || !exits || !counts || !first_block || !coef || !info) return -2;
    const int wgs = (nsub + NT - 1) / NT;
    if (frames > 0x7fffffffL / wgs) return -3;
    hipLaunchKernelGGL(jd_prefix_kernel, dim3((unsigned)frames), dim3(PT), 0, (hipStream_t)stream, counts, first_block, nsub);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jd_coef_kernel, dim3((unsigned)(frames * wgs)), dim3(NT), 0, (hipStream_t)stream, data, data_bytes, tabs, exits, first_block,
                       coef, info, nsub, sub_bytes, wgs, g.bpm, (int)nbf);
    MG_CHECK_LAUNCH();
    return 0;
}

int launch_dcsum(int16_t* coef, long coef_elems, const int32_t* tabs, long frames, const Geo& g, void* stream) {
    const long nbf = (long)g.mcux * g.mcuy * g.bpm;
    if (nbf > 0x7fffffffL / 64 || coef_elems != frames * nbf * 64) return -2;
    if (frames == 0) return 0;
    if (!coef || !tabs) return -2;
    const int ncomp = g.bpm == 1 ? 1 : 3;
    if (frames > 0x7fffffffL / ncomp) return -3;
    hipLaunchKernelGGL(jd_dcsum_kernel, dim3((unsigned)(frames * ncomp)), dim3(PT), 0, (hipStream_t)stream, coef, tabs, g.bpm, g.mcux * g.mcuy, ncomp);
    MG_CHECK_LAUNCH();
    return 0;
}

int launch_idct(const int16_t* coef, long coef_elems, const int32_t* tabs, uint8_t* planes, long plane_bytes, long want_bytes, long frames,
                const Geo& g, void* stream) {
    const long nbf = (long)g.mcux * g.mcuy * g.bpm;
    if (nbf > 0x7fffffffL / 64 || coef_elems != frames * nbf * 64 || plane_bytes != want_bytes) return -2;
    if (frames == 0) return 0;
    if (!coef || !tabs || !planes || (uintptr_t)planes % 16 != 0) return -2;
    const long nblocks = frames * nbf, blocks = (nblocks + PT / 8 - 1) / (PT / 8);
    if (blocks > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, coef, tabs, planes, frames, g, nblocks);
    MG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int mg_jpegdec_limits(int* threads, int* min_sub, int* max_sub, int* default_sub, int* tab_words) {
    if (!threads || !min_sub || !max_sub || !default_sub || !tab_words) return -2;
    *threads = NT; *min_sub = MG_JPEGDEC_MIN_SUB; *max_sub = MG_JPEGDEC_MAX_SUB; *default_sub = MG_JPEGDEC_DEFAULT_SUB; *tab_words = TW;
    return 0;
}

extern "C" int mg_jpegdec_sync(const uint8_t* data, long data_bytes, const int32_t* tabs, unsigned long long* exits, int32_t* counts,
                               unsigned long long* entries, unsigned long long* bounds, int32_t* info, int info_words, long frames, int nsub,
                               int sub_bytes, int layout, int launch, void* stream) {
    if (frames < 0 || bad_layout(layout) || bad_sub(nsub, sub_bytes) || data_bytes < 0 || launch < 0 || info_words < 4 ||
        launch > (info_words - 4) / 2) return -2;
    if (frames == 0) return 0;
    return launch_sync(data, data_bytes, tabs, exits, counts, entries, bounds, info, frames, nsub, sub_bytes, geo_of(layout, 8, 8).bpm, launch, stream);
}

extern "C" int mg_jpegdec_coef(const uint8_t* data, long data_bytes, const int32_t* tabs, const unsigned long long* exits, const int32_t* counts,
                               int32_t* first_block, int16_t* coef, long coef_elems, int32_t* info, long frames, int nsub, int sub_bytes, int h, int w,
                               int layout, void* stream) {
    if (jpeg_bad_size(frames, h, w) || bad_layout(layout) || bad_sub(nsub, sub_bytes) || data_bytes < 0) return -2;
    return launch_coef(data, data_bytes, tabs, exits, counts, first_block, coef, coef_elems, info, frames, nsub, sub_bytes, geo_of(layout, h, w), stream);
}

extern "C" int mg_jpegdec_dcsum(int16_t* coef, long coef_elems, const int32_t* tabs, long frames, int h, int w, int layout, void* stream) {
    if (jpeg_bad_size(frames, h, w) || bad_layout(layout)) return -2;
    return launch_dcsum(coef, coef_elems, tabs, frames, geo_of(layout, h, w), stream);
}

extern "C" int mg_jpegdec_idct(const int16_t* coef, long coef_elems, const int32_t* tabs, uint8_t* planes, long plane_bytes, long frames, int h, int w,
                               int layout, void* stream) {
    if (jpeg_bad_size(frames, h, w) || bad_layout(layout)) return -2;
    const Geo g = geo_of(layout, h, w);
    return launch_idct(coef, coef_elems, tabs, planes, plane_bytes, plane_bytes_of(frames, layout, g), frames, g, stream);
}

extern "C" int mg_jpegdec_rgb(const uint8_t* planes, long plane_bytes, void* out, long frames, int h, int w, int layout, int epilogue,
                              const float* mean3, const float* std3, void* stream) {
    if (jpeg_bad_size(frames, h, w) || (layout != MG_JPEGDEC_444 && layout != MG_JPEGDEC_GREY) || (epilogue != MG_PHOTO_RAW && epilogue != MG_PHOTO_NORM) ||
        !mean3 || !std3) return -2;
    const Geo g = geo_of(layout, h, w);
    if (plane_bytes != plane_bytes_of(frames, layout, g)) return -2;
    if (frames == 0) return 0;
    if (!planes || !out || (const void*)planes == out) return -2;
    const long pixels = frames * h * w, blocks = (pixels + PT - 1) / PT;
    if (blocks > 0x7fffffffL) return -3;
    const int grey = layout == MG_JPEGDEC_GREY;
    if (epilogue == MG_PHOTO_RAW)
        hipLaunchKernelGGL(jd_rgb_kernel<MG_PHOTO_RAW>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, planes, out, frames, h, w, g.mcuy * 8,
                           g.mcux * 8, grey, pixels, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
        hipLaunchKernelGGL(jd_rgb_kernel<MG_PHOTO_NORM>, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, planes, out, frames, h, w, g.mcuy * 8,
                           g.mcux * 8, grey, pixels, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MG_CHECK_LAUNCH();
    return 0;
}
