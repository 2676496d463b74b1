// PNG encoding on the device: P planes of one size (uint8, or float32 converted on the load) -> the zlib streams of 8-bit greyscale,
//   non-interlaced PNG files with the Sub filter on every row, packed back to back in one blob. Replaces the pixel pass of the result writer
//   (maggie/engine/test.py:20-68: `(alphas * 255).astype('uint8')`, `> 0.5`, cv2.imwrite). The signature, IHDR, the IDAT length and CRC and
//   IEND are the host's (maggie_amd/utils/pngenc.py); DESIGN.md section 27 holds the algorithm, the LDS table and the measurements;
//   tests/pngenc_restatement.py states the same encoder sequentially and is its byte-for-byte oracle.
//   The colour entries (mg_pngenc_size_rgb / mg_pngenc_emit_rgb: RGB and RGBA images) run the same kernels on rows of
//   channels x w bytes with the filter distance `channels`; only pe_load_block knows the difference.
//
// The filtered stream of a plane (h x (1 + w) bytes: 01, p[0], p[1] - p[0], ...) is cut into deflate blocks of MG_PNGENC_BLOCK_BYTES; one
//   workgroup of MG_PNGENC_THREADS lanes handles one block, lane t the bytes [64 t, 64 t + 64). Tokens are runs only (distance 1) and never
//   cross a block: a byte starts a run when it differs from its left neighbour, a lane's first byte learns its run's start from a max-scan of
//   the lanes' last starts and a lane's last byte its run's end from a reverse min-scan of their first starts (in the wave by shuffles,
//   across the waves through LDS); pe_token_at() then tells from (offset in the run, run length) alone what a byte starts.
// pe_size_kernel   histogram (LDS integer atomics) -> code lengths (two-queue Huffman over the symbols ranked by (count, symbol), limited to
//   15 / 7 bits by a Kraft repair) -> the 16 / 17 / 18 coding of the length list -> fixed or dynamic by exact bit count -> the block's record
//   (type, bits, Adler-32 partials, lengths). pe_total_kernel adds a plane's bit counts into its stream size.
// pe_emit_kernel   re-derives the tokens from the pixels (a block's tokens would be up to 64 KiB of traffic each way; the pixels are read
//   once more instead), sums the bit counts of the blocks in front of it, ORs the codes into an LDS image of the block at bit offsets from a
//   prefix sum, and flushes: interior words with plain (16-byte where aligned) stores, the first and the last word with a global atomicOr
//   on the zeroed output, because neighbouring blocks share them. A plane's first block writes 78 01, its last block sets BFINAL, pads to
//   a byte and writes the Adler-32 combined from the partials.
#ifndef MG_HOST_EMU
#include "common.h"
#include "../../include/maggie_hip.h"
#define MG_DEVCONST __device__ const

namespace {
// the cross-lane scans of one workgroup of four waves (the host build of tests/csrc/pngenc_host.cpp replaces these three). `wt`: 4 words of LDS.
__device__ __forceinline__ int pe_scan_add_excl(int v, int* total, int* wt) {       // sum of v over the lanes in front; *total over all
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
    __syncthreads();
    if (lane == 63) wt[wv] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int t = wt[i]; if (i < wv) base += t; tot += t; }
    *total = tot;
    return base + x - v;
}
__device__ __forceinline__ int pe_scan_max_excl(int v, int* wt) {                   // max of v over the lanes in front, -1 for lane 0
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(x, o, 64); if (lane >= o && u > x) x = u; }
    __syncthreads();
    if (lane == 63) wt[wv] = x;
    __syncthreads();
    int r = __shfl_up(x, 1, 64);
    if (lane == 0) r = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int t = wt[i]; if (i < wv && t > r) r = t; }
    return r;
}
__device__ __forceinline__ int pe_scan_min_excl_rev(int v, int none, int* wt) {     // min of v over the lanes behind, `none` for the last
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_down(x, o, 64); if (lane + o < 64 && u < x) x = u; }
    __syncthreads();
    if (lane == 0) wt[wv] = x;
    __syncthreads();
    int r = __shfl_down(x, 1, 64);
    if (lane == 63) r = none;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int t = wt[i]; if (i > wv && t < r) r = t; }
    return r;
}
}  // namespace
#endif

namespace {

constexpr int PT = MG_PNGENC_THREADS;
constexpr int PB = MG_PNGENC_BLOCK_BYTES;
constexpr int PCH = PB / PT;                                               // bytes of a lane
constexpr int PRW = MG_PNGENC_REC_WORDS;
constexpr int IMG_WORDS = PB * 9 / 32 + 8;                                 // 31 + 16 + (9 B + 10) + 7 + 32 bits, rounded up
constexpr unsigned PADLER = 65521u;
static_assert(PT == 256 && PB % PT == 0 && PB >= 4096 && PB <= 32768, "four waves; a run length fits 16 bits");
static_assert(IMG_WORDS * 32 >= 31 + 16 + 9 * PB + 10 + 7 + 32 + 32, "the image holds a block of the fixed form, the header bytes and the trailer");

MG_DEVCONST uint8_t PE_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one sample as the byte the file stores
__device__ __forceinline__ int pe_pixel(const void* __restrict__ src, int mode, long idx) {
    if (mode == MG_PNGENC_MODE_U8) return ((const uint8_t*)src)[idx];
    const float x = ((const float*)src)[idx];
    if (mode == MG_PNGENC_MODE_THRESHOLD) return x > 0.5f ? 255 : 0;
    const float y = x * 255.0f;
    return !(y >= 0.f) ? 0 : (y >= 255.f ? 255 : (int)y);                  // NaN and negatives -> 0
}

// the bytes [k PB, k PB + n) of the plane's filtered stream -> fb. `w` is the BYTES of a row and `bpp` the filter distance: 1 for a grey
// plane, the channel count (and w = channels x width) for a colour image, whose samples are uint8
__device__ __forceinline__ void pe_load_block(const void* __restrict__ src, int mode, long plane, int h, int w, int bpp, int k, int n, uint8_t* fb, int tid) {
    const unsigned pitch = (unsigned)w + 1u;
    const long base = plane * (long)h * w;
    for (int i = tid; i < n; i += PT) {
        const unsigned g = (unsigned)k * (unsigned)PB + (unsigned)i;       // < 2^30
        const unsigned r = g / pitch, c = g - r * pitch;
        int v = 1;
        if (c >= 1) {
            const long at = base + (long)r * w + (c - 1);
            v = pe_pixel(src, mode, at);
            if (c > (unsigned)bpp) v = (v - pe_pixel(src, mode, at - bpp)) & 255;
        }
        fb[i] = (uint8_t)v;
    }
    __syncthreads();
}

// what the byte at offset o of a run of length L starts: 0 nothing, 1 a literal, else a match of that length at distance 1
__device__ __forceinline__ int pe_token_at(int o, int L) {
    if (L < 4 || o == 0) return 1;
    const int m = (L - 1) / 258, q = (o - 1) / 258, ro = (o - 1) - q * 258;
    if (q < m) return ro == 0 ? 258 : 0;
    const int rem = (L - 1) - 258 * m;
    if (rem >= 3) return ro == 0 ? rem : 0;
    return 1;
}

// a match length 3..258 -> its literal/length symbol, the number of extra bits and their value
__device__ __forceinline__ int pe_length_symbol(int len, int* eb, int* ev) {
    *eb = 0; *ev = 0;
    if (len == 258) return 285;
    const int l = len - 3;
    if (l < 8) return 257 + l;
    const int e = 29 - __builtin_clz((unsigned)l);                         // floor(log2 l) - 2
    *eb = e; *ev = l & ((1 << e) - 1);
    return 257 + 4 * e + 4 + ((l >> e) & 3);
}
__device__ __forceinline__ int pe_len_extra(int i) { return i < 8 || i == 28 ? 0 : (i >> 2) - 1; }      // extra bits of length code 257 + i
__device__ __forceinline__ int pe_fixed_len(int s) { return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)); }

// where the lane's first byte's run starts and where its last byte's run ends
struct Span { int a, e, sin, eout; };
__device__ __forceinline__ Span pe_spans(const uint8_t* fb, int n, int tid, int* wt) {
    Span s;
    s.a = tid * PCH < n ? tid * PCH : n;
    s.e = s.a + PCH < n ? s.a + PCH : n;
    int fs = n, ls = -1;
    for (int i = s.a; i < s.e; ++i)
        if (i == 0 || fb[i] != fb[i - 1]) { if (fs == n) fs = i; ls = i; }
    const int before = pe_scan_max_excl(ls, wt);
    s.eout = pe_scan_min_excl_rev(fs, n, wt);
    s.sin = fs == s.a ? s.a : before;                                      // byte 0 is a start, so `before` >= 0 wherever it is used
    if (s.sin < 0) s.sin = 0;
    return s;
}

// f(position, kind, byte) for every token that starts in the lane's bytes, in order
template <typename F>
__device__ __forceinline__ void pe_walk(const uint8_t* fb, const Span& sp, F f) {
    int i = sp.a, s = sp.sin;
    while (i < sp.e) {
        int e = i + 1;
        while (e < sp.e && fb[e] == fb[e - 1]) ++e;
        const int L = (e == sp.e ? sp.eout : e) - s;
        const int v = fb[i];
        for (int q = i; q < e; ++q) {
            const int k = pe_token_at(q - s, L);
            if (k) f(q, k, v);
        }
        i = e; s = e;
    }
}

struct HuffWork { int lw[288], iw[288], blc[16], m; uint16_t sym[288], lp[288], ip[288], idepth[288]; };

// counts of `nsym` symbols -> code lengths of at most `maxbits` (every lane calls it; lane 0 builds the tree)
__device__ __forceinline__ void pe_code_lengths(const int* hist, int nsym, int maxbits, uint8_t* lens, HuffWork& W, int tid) {
    __syncthreads();
    if (tid == 0) W.m = 0;
    for (int s = tid; s < nsym; s += PT) lens[s] = 0;
    __syncthreads();
    for (int s = tid; s < nsym; s += PT) {
        const int c = hist[s];
        if (c > 0) {
            int rank = 0;
            for (int j = 0; j < nsym; ++j) { const int cj = hist[j]; rank += (cj > 0 && (cj < c || (cj == c && j < s))) ? 1 : 0; }
            W.sym[rank] = (uint16_t)s;
            W.lw[rank] = c;
            atomicAdd(&W.m, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int m = W.m;
        if (m == 1) lens[W.sym[0]] = 1;
        if (m >= 2) {
            int li = 0, ii = 0;
            for (int k = 0; k < m - 1; ++k) {                              // two queues: the leaves in order, the nodes as they were made
                int w = 0;
                for (int t = 0; t < 2; ++t) {
                    if (li < m && (ii >= k || W.lw[li] <= W.iw[ii])) { w += W.lw[li]; W.lp[li] = (uint16_t)k; ++li; }
                    else { w += W.iw[ii]; W.ip[ii] = (uint16_t)k; ++ii; }
                }
                W.iw[k] = w;
            }
            W.idepth[m - 2] = 0;
            for (int j = m - 3; j >= 0; --j) W.idepth[j] = (uint16_t)(W.idepth[W.ip[j]] + 1);
            for (int l = 0; l < 16; ++l) W.blc[l] = 0;
            for (int i = 0; i < m; ++i) { const int d = W.idepth[W.lp[i]] + 1; W.blc[d < maxbits ? d : maxbits] += 1; }
            int total = 0;
            for (int l = 1; l <= maxbits; ++l) total += W.blc[l] << (maxbits - l);
            for (int guard = 0; total > (1 << maxbits) && guard < 288; ++guard) {      // the excess is below the number of folded codes
                W.blc[maxbits] -= 1;
                for (int l = maxbits - 1; l >= 1; --l)
                    if (W.blc[l]) { W.blc[l] -= 1; W.blc[l + 1] += 2; break; }
                total -= 1;
            }
            int i = 0;
            for (int l = maxbits; l >= 1; --l)
                for (int c = W.blc[l]; c > 0 && i < m; --c) lens[W.sym[i++]] = (uint8_t)l;
        }
    }
    __syncthreads();
}

// the 16 / 17 / 18 coding of lens[0, hlit) followed by the one distance length 1 -> tok[] = symbol | extra value << 5; counts into clhist if given
__device__ __forceinline__ int pe_rle(const uint8_t* lens, int hlit, uint16_t* tok, int* clhist) {
    int nt = 0, i = 0;
    const int n = hlit + 1;
#define PE_GET(j) ((j) < hlit ? (int)lens[j] : 1)
#define PE_TOK(s, x) do { if (nt < 288) tok[nt++] = (uint16_t)((s) | ((x) << 5)); if (clhist) clhist[s] += 1; } while (0)
    while (i < n) {
        const int v = PE_GET(i);
        int r = 1;
        while (i + r < n && PE_GET(i + r) == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int k = r < 138 ? r : 138; PE_TOK(18, k - 11); r -= k; }
            while (r >= 3) { const int k = r < 10 ? r : 10; PE_TOK(17, k - 3); r -= k; }
        } else {
            PE_TOK(v, 0);
            --r;
            while (r >= 3) { const int k = r < 6 ? r : 6; PE_TOK(16, k - 3); r -= k; }
        }
        for (; r > 0; --r) PE_TOK(v, 0);
    }
#undef PE_GET
#undef PE_TOK
    return nt;
}
__device__ __forceinline__ int pe_cl_extra(int s) { return s == 16 ? 2 : (s == 17 ? 3 : (s == 18 ? 7 : 0)); }

// RFC 1951 3.2.2, the codes bit-reversed for an LSB-first stream (one lane)
__device__ __forceinline__ void pe_codes(const uint8_t* lens, int n, uint16_t* code) {
    int blc[16], nxt[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) blc[l] = 0;
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
#pragma unroll
        for (int q = 1; q < 16; ++q) blc[q] += l == q ? 1 : 0;
    }
    int c = 0;
    nxt[0] = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) { c = (c + blc[l - 1]) << 1; nxt[l] = c; }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        int v = 0;
#pragma unroll
        for (int q = 1; q < 16; ++q)
            if (l == q) { v = nxt[q]; nxt[q] += 1; }
        int r = 0;
        for (int b = 0; b < l; ++b) { r = (r << 1) | (v & 1); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

__device__ __forceinline__ void pe_put(uint32_t* img, int bit, uint32_t v, int nb) {
    const int w = bit >> 5;
    if (nb <= 0 || bit < 0 || w + 1 >= IMG_WORDS) return;
    const unsigned long long x = (unsigned long long)v << (bit & 31);
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (lo) atomicOr(&img[w], lo);
    if (hi) atomicOr(&img[w + 1], hi);
}

__device__ __forceinline__ int pe_blocks(int h, int w) { return (int)(((long)h * (w + 1) + PB - 1) / PB); }

__global__ void __launch_bounds__(MG_PNGENC_THREADS)
pe_size_kernel(const void* __restrict__ src, int mode, int h, int w, int bpp, int32_t* __restrict__ recs) {
    __shared__ __attribute__((aligned(16))) uint8_t fb[PB];
    __shared__ int hist[288], clhist[20], wt[4], ntok;
    __shared__ unsigned long long acc[2];
    __shared__ HuffWork W;
    __shared__ __attribute__((aligned(4))) uint8_t lens[288];
    __shared__ __attribute__((aligned(4))) uint8_t cllens[20];
    __shared__ uint16_t cltok[288];
    __shared__ int hdr[8];
    const int tid = (int)threadIdx.x;
    const int nb = pe_blocks(h, w);
    const long plane = blockIdx.x / (unsigned)nb;
    const int k = (int)(blockIdx.x - (unsigned)plane * (unsigned)nb);
    const long raw = (long)h * (w + 1);
    const int n = (int)(raw - (long)k * PB < PB ? raw - (long)k * PB : PB);
    for (int s = tid; s < 288; s += PT) { hist[s] = 0; lens[s] = 0; }
    if (tid < 20) { clhist[tid] = 0; cllens[tid] = 0; }
    if (tid < 2) acc[tid] = 0;
    if (tid == 0) ntok = 0;
    pe_load_block(src, mode, plane, h, w, bpp, k, n, fb, tid);
    const Span sp = pe_spans(fb, n, tid, wt);
    unsigned long long s1 = 0, s2 = 0;
    for (int i = sp.a; i < sp.e; ++i) { const unsigned b = fb[i]; s1 += b; s2 += (unsigned long long)b * (unsigned)(n - i); }
    atomicAdd(&acc[0], s1);
    atomicAdd(&acc[1], s2);
    int mine = 0;
    pe_walk(fb, sp, [&](int, int kind, int v) {
        int eb, ev;
        atomicAdd(&hist[kind == 1 ? v : pe_length_symbol(kind, &eb, &ev)], 1);
        ++mine;
    });
    atomicAdd(&ntok, mine);
    __syncthreads();
    if (tid == 0) hist[256] = 1;
    pe_code_lengths(hist, 286, 15, lens, W, tid);
    if (tid == 0) {
        int hlit = 257;
        for (int s = 257; s < 286; ++s) if (lens[s]) hlit = s + 1;
        hdr[0] = hlit;
        hdr[1] = pe_rle(lens, hlit, cltok, clhist);
    }
    pe_code_lengths(clhist, 19, 7, cllens, W, tid);
    if (tid == 0) {
        const int hlit = hdr[0], ncl = hdr[1];
        int hclen = 4;
        for (int i = 4; i < 19; ++i) if (cllens[PE_CL_ORDER[i]]) hclen = i + 1;
        int extra = 0, nmatch = 0;
        for (int i = 0; i < 29; ++i) { extra += hist[257 + i] * pe_len_extra(i); nmatch += hist[257 + i]; }
        int fixed = 3 + extra + 5 * nmatch, dyn = 17 + 3 * hclen + extra + nmatch;
        for (int s = 0; s < 286; ++s) { fixed += hist[s] * pe_fixed_len(s); dyn += hist[s] * lens[s]; }
        for (int t = 0; t < ncl; ++t) { const int s = cltok[t] & 31; dyn += cllens[s] + pe_cl_extra(s); }
        int32_t* rec = recs + (long)blockIdx.x * PRW;
        rec[0] = dyn < fixed ? 2 : 1;
        rec[1] = dyn < fixed ? dyn : fixed;
        rec[2] = n;
        rec[3] = ntok;
        rec[4] = (int32_t)(acc[0] % PADLER);
        rec[5] = (int32_t)(acc[1] % PADLER);
        rec[6] = hlit;
        rec[7] = hclen;
        rec[85] = 0; rec[86] = 0; rec[87] = 0;
    }
    int32_t* rec = recs + (long)blockIdx.x * PRW;
    if (tid < 72) rec[8 + tid] = *reinterpret_cast<const int32_t*>(lens + 4 * tid);
    if (tid < 5) rec[80 + tid] = *reinterpret_cast<const int32_t*>(cllens + 4 * tid);
}

// sizes[p] = 2 + the bytes of the plane's blocks + 4
__global__ void __launch_bounds__(MG_PNGENC_THREADS)
pe_total_kernel(const int32_t* __restrict__ recs, int h, int w, int64_t* __restrict__ sizes) {
    __shared__ unsigned long long acc;
    const int tid = (int)threadIdx.x;
    const int nb = pe_blocks(h, w);
    if (tid == 0) acc = 0;
    __syncthreads();
    unsigned long long bits = 0;
    for (int j = tid; j < nb; j += PT) bits += (unsigned)recs[((long)blockIdx.x * nb + j) * PRW + 1];
    atomicAdd(&acc, bits);
    __syncthreads();
    if (tid == 0) sizes[blockIdx.x] = (int64_t)(6 + ((acc + 7) >> 3));
}

__global__ void __launch_bounds__(MG_PNGENC_THREADS)
pe_emit_kernel(const void* __restrict__ src, int mode, int h, int w, int bpp, const int32_t* __restrict__ recs, const int64_t* __restrict__ sizes,
               uint8_t* __restrict__ out, long out_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t fb[PB];
    __shared__ __attribute__((aligned(16))) uint32_t img[IMG_WORDS];
    __shared__ __attribute__((aligned(4))) uint8_t lens[288];
    __shared__ __attribute__((aligned(4))) uint8_t cllens[20];
    __shared__ uint16_t code[288], clcode[20], cltok[288];
    __shared__ unsigned long long acc[4];
    __shared__ int wt[4], hdr[4];
    const int tid = (int)threadIdx.x;
    const int nb = pe_blocks(h, w);
    const long plane = blockIdx.x / (unsigned)nb;
    const int k = (int)(blockIdx.x - (unsigned)plane * (unsigned)nb);
    const long raw = (long)h * (w + 1);
    const int n = (int)(raw - (long)k * PB < PB ? raw - (long)k * PB : PB);
    const bool final = k == nb - 1;
    const int32_t* rec = recs + (long)blockIdx.x * PRW;
    const int type = rec[0] == 2 ? 2 : 1;
    int hlit = rec[6], hclen = rec[7];
    hlit = hlit < 257 ? 257 : (hlit > 286 ? 286 : hlit);
    hclen = hclen < 4 ? 4 : (hclen > 19 ? 19 : hclen);
    if (tid < 72) {
        uint32_t v = (uint32_t)rec[8 + tid] & 0x0f0f0f0fu;
        if (type == 1) {
            v = 0;
            for (int b = 0; b < 4; ++b) v |= (uint32_t)pe_fixed_len(4 * tid + b) << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(lens + 4 * tid) = v;
    }
    if (tid < 5) *reinterpret_cast<uint32_t*>(cllens + 4 * tid) = (uint32_t)rec[80 + tid] & 0x07070707u;
    if (tid < 4) acc[tid] = 0;
    for (int i = tid; i < IMG_WORDS; i += PT) img[i] = 0;
    pe_load_block(src, mode, plane, h, w, bpp, k, n, fb, tid);
    // the bytes of the planes in front, the bits of this plane's blocks in front, and (the last block) the Adler-32 of the plane
    unsigned long long off = 0, pre = 0, a1 = 0, a2 = 0;
    for (long q = tid; q < plane; q += PT) off += (unsigned long long)sizes[q];
    for (int j = tid; j < (final ? nb : k); j += PT) {
        const int32_t* rj = recs + (plane * nb + j) * PRW;
        if (j < k) pre += (unsigned)rj[1];
        if (final) {
            const long end = (long)(j + 1) * PB < raw ? (long)(j + 1) * PB : raw;
            const unsigned s1 = (unsigned)rj[4] % PADLER, s2 = (unsigned)rj[5] % PADLER;
            a1 += s1;
            a2 = (a2 + s2 + (unsigned long long)s1 * (unsigned)((raw - end) % PADLER)) % PADLER;
        }
    }
    atomicAdd(&acc[0], off);
    atomicAdd(&acc[1], pre);
    atomicAdd(&acc[2], a1);
    atomicAdd(&acc[3], a2);
    const Span sp = pe_spans(fb, n, tid, wt);                                // its barriers also order the writes above
    const unsigned long long g0 = acc[0] * 8 + (k == 0 ? 0 : 16 + acc[1]);  // the blob's bit at which this block (or the header bytes) starts
    const long word0 = (long)(g0 >> 5);
    if (tid == 0) {
        pe_codes(lens, 288, code);                                           // the fixed set counts the two symbols that never occur
        int bit = (int)(g0 & 31);
        if (k == 0) { pe_put(img, bit, 0x0178u, 16); bit += 16; }
        pe_put(img, bit, (final ? 1u : 0u) | ((uint32_t)type << 1), 3);
        bit += 3;
        if (type == 2) {
            pe_codes(cllens, 19, clcode);
            const int ncl = pe_rle(lens, hlit, cltok, nullptr);
            pe_put(img, bit, (uint32_t)(hlit - 257) | ((uint32_t)(hclen - 4) << 10), 14);
            bit += 14;
            for (int i = 0; i < hclen; ++i) { pe_put(img, bit, cllens[PE_CL_ORDER[i]], 3); bit += 3; }
            for (int t = 0; t < ncl; ++t) {
                const int s = cltok[t] & 31, eb = pe_cl_extra(s), l = cllens[s < 19 ? s : 0];
                pe_put(img, bit, (uint32_t)clcode[s < 19 ? s : 0] | ((uint32_t)(cltok[t] >> 5) << l), l + eb);
                bit += l + eb;
            }
        }
        hdr[0] = bit;
    }
    __syncthreads();
    const int dbits = type == 2 ? 1 : 5;
    int mine = 0;
    pe_walk(fb, sp, [&](int, int kind, int v) {
        int eb = 0, ev = 0;
        const int s = kind == 1 ? v : pe_length_symbol(kind, &eb, &ev);
        mine += lens[s] + (kind == 1 ? 0 : eb + dbits);
    });
    int total = 0;
    int at = hdr[0] + pe_scan_add_excl(mine, &total, wt);
    pe_walk(fb, sp, [&](int, int kind, int v) {
        int eb = 0, ev = 0;
        const int s = kind == 1 ? v : pe_length_symbol(kind, &eb, &ev);
        const int l = lens[s];
        const int nbits = l + (kind == 1 ? 0 : eb + dbits);
        pe_put(img, at, (uint32_t)code[s] | ((uint32_t)ev << l), nbits);
        at += nbits;
    });
    if (tid == 0) {
        int bit = hdr[0] + total;
        pe_put(img, bit, code[256], lens[256]);
        bit += lens[256];
        if (final) {
            bit = (bit + 7) & ~7;
            const unsigned A = (unsigned)((1 + acc[2]) % PADLER), Bv = (unsigned)((acc[3] + (unsigned long long)(raw % PADLER)) % PADLER);
            const uint32_t ad = (Bv << 16) | A;
            for (int b = 0; b < 4; ++b) { pe_put(img, bit, (ad >> (24 - 8 * b)) & 255u, 8); bit += 8; }
        }
        hdr[1] = bit;
    }
    __syncthreads();
    int nw = (hdr[1] + 31) >> 5;
    if (nw > IMG_WORDS) nw = IMG_WORDS;
    const long cap = out_bytes >> 2;                                       // words of the output
    uint32_t* outw = reinterpret_cast<uint32_t*>(out);
    if (tid == 0 && word0 < cap && img[0]) atomicOr(&outw[word0], img[0]);
    if (tid == 1 && nw > 1 && word0 + nw - 1 < cap && img[nw - 1]) atomicOr(&outw[word0 + nw - 1], img[nw - 1]);
    // the interior [1, nw - 1): single words up to the first 16-byte boundary of the output, 16-byte stores, single words again
    const int lo = 1, hi = nw - 1;
    int mid = lo + (int)((4 - ((word0 + lo) & 3)) & 3);
    if (mid > hi) mid = hi;
    const int quads = hi > mid ? (hi - mid) >> 2 : 0;
    const int tail = mid + 4 * quads;
    for (int i = lo + tid; i < mid; i += PT)
        if (word0 + i < cap) outw[word0 + i] = img[i];
    for (int q = tid; q < quads; q += PT) {
        const int i = mid + 4 * q;
        if (word0 + i + 3 < cap) {
            uint4 v;
            v.x = img[i]; v.y = img[i + 1]; v.z = img[i + 2]; v.w = img[i + 3];
            *reinterpret_cast<uint4*>(outw + word0 + i) = v;
        } else {                                                           // out_bytes below the sum of the sizes: the words that still fit
            for (int j = 0; j < 4; ++j)
                if (word0 + i + j < cap) outw[word0 + i + j] = img[i + j];
        }
    }
    for (int i = tail + tid; i < hi; i += PT)
        if (word0 + i < cap) outw[word0 + i] = img[i];
}

__host__ inline int pe_bad_args(const void* planes, int mode, long nplanes, int h, int w) {
    if (!planes || mode < 0 || mode > 2 || nplanes < 1 || nplanes > MG_PNGENC_MAX_PLANES) return 1;
    if (h < 1 || w < 1 || h > MG_PNGENC_MAX_SIDE || w > MG_PNGENC_MAX_WIDTH || (long)h * (w + 1) > MG_PNGENC_MAX_RAW) return 1;
    return (uintptr_t)planes % (mode == MG_PNGENC_MODE_U8 ? 1 : 4) != 0;
}

}  // namespace

extern "C" int mg_pngenc_limits(int* threads, int* block_bytes, int* rec_words, int* max_side, int* max_width, int* max_planes) {
    if (!threads || !block_bytes || !rec_words || !max_side || !max_width || !max_planes) return -2;
    *threads = PT; *block_bytes = PB; *rec_words = PRW; *max_side = MG_PNGENC_MAX_SIDE; *max_width = MG_PNGENC_MAX_WIDTH; *max_planes = MG_PNGENC_MAX_PLANES;
    return 0;
}

// the launches of both forms: `w` the bytes of a row, `bpp` the filter distance
static int pe_size_launch(const void* planes, int mode, long nplanes, int h, int w, int bpp, int32_t* recs, int64_t* sizes, void* stream) {
    if (pe_bad_args(planes, mode, nplanes, h, w) || !recs || !sizes || (uintptr_t)recs % 4 != 0 || (uintptr_t)sizes % 8 != 0) return -2;
    const long grid = nplanes * (((long)h * (w + 1) + PB - 1) / PB);
    if (grid > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(pe_size_kernel, dim3((unsigned)grid), dim3(PT), 0, (hipStream_t)stream, planes, mode, h, w, bpp, recs);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pe_total_kernel, dim3((unsigned)nplanes), dim3(PT), 0, (hipStream_t)stream, (const int32_t*)recs, h, w, sizes);
    MG_CHECK_LAUNCH();
    return 0;
}

static int pe_emit_launch(const void* planes, int mode, long nplanes, int h, int w, int bpp, const int32_t* recs, const int64_t* sizes, uint8_t* out,
                          long out_bytes, void* stream) {
    if (pe_bad_args(planes, mode, nplanes, h, w) || !recs || !sizes || !out || (uintptr_t)recs % 4 != 0 || (uintptr_t)sizes % 8 != 0) return -2;
    if ((uintptr_t)out % 16 != 0 || out_bytes < 8 || out_bytes % 4 != 0) return -2;
    const long grid = nplanes * (((long)h * (w + 1) + PB - 1) / PB);
    if (grid > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(pe_emit_kernel, dim3((unsigned)grid), dim3(PT), 0, (hipStream_t)stream, planes, mode, h, w, bpp, recs, sizes, out, out_bytes);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_pngenc_size(const void* planes, int mode, long nplanes, int h, int w, int32_t* recs, int64_t* sizes, void* stream) {
    return pe_size_launch(planes, mode, nplanes, h, w, 1, recs, sizes, stream);
}

extern "C" int mg_pngenc_emit(const void* planes, int mode, long nplanes, int h, int w, const int32_t* recs, const int64_t* sizes, uint8_t* out,
                              long out_bytes, void* stream) {
    return pe_emit_launch(planes, mode, nplanes, h, w, 1, recs, sizes, out, out_bytes, stream);
}

// colour: [nimages][h][w][channels] uint8 is [nimages][h][channels w] bytes with the filter distance `channels`
static inline int pe_bad_colour(int channels, int w) { return (channels != 3 && channels != 4) || w < 1 || w > MG_PNGENC_MAX_WIDTH / channels; }

extern "C" int mg_pngenc_size_rgb(const uint8_t* images, int channels, long nimages, int h, int w, int32_t* recs, int64_t* sizes, void* stream) {
    if (pe_bad_colour(channels, w)) return -2;
    return pe_size_launch(images, MG_PNGENC_MODE_U8, nimages, h, channels * w, channels, recs, sizes, stream);
}

extern "C" int mg_pngenc_emit_rgb(const uint8_t* images, int channels, long nimages, int h, int w, const int32_t* recs, const int64_t* sizes,
                                  uint8_t* out, long out_bytes, void* stream) {
    if (pe_bad_colour(channels, w)) return -2;
    return pe_emit_launch(images, MG_PNGENC_MODE_U8, nimages, h, channels * w, channels, recs, sizes, out, out_bytes, stream);
}
