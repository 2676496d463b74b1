// RFC 1951 for one wave and one zlib stream: the inflate body of `mg_pngdec_inflate` (csrc/pngdec.hip) and `mg_pngcolor_inflate`
//   (csrc/pngcolor.hip), which differ only in where the expected byte count comes from. DESIGN.md section 26 holds the bounds argument.
//
// pd_inflate_file   ONE WAVE per stream. The bit reader's state (64-bit hold, bit count, next byte) is wave-uniform: every lane decodes every
//   token, lane t KEEPS token t of a round of up to MG_PNGDEC_ROUND_TOKENS tokens (a literal, or a length / distance pair).
//   An exclusive prefix sum of the token lengths gives each token's output position; the literals in front of the round's first match are
//   written first, then the matches in token order, each followed by the literals up to the next match, all 64 lanes copying one match
//   together: byte j comes from pos - dist + (dist < len ? j % dist : j), which lies in front of the match, so that no lane waits for another
//   inside a match. (All literals of a round at once would be wrong on a 32 KiB ring: a literal 32 768 - dist + k bytes behind a match
//   takes the slot of the match's source byte k.) The 32 KiB window is an LDS ring; it is flushed to `raw` in
//   16-byte stores whenever MG_PNGDEC_FLUSH_BYTES are pending, and the Adler-32 sums are taken from the ring at the same time: no lane reads
//   global memory that this launch wrote. The compressed bytes come through an LDS stage filled with coalesced dword loads. Dynamic code
//   sets are turned into a look-up table (short codes) plus the canonical count / sorted-symbol form (long codes) in LDS per block, under
//   zlib's acceptance rules. Every loop consumes at least one bit or produces at least one byte per turn and stops at the stream's last bit
//   and at the size the caller expects.
//
// A host build (tests/csrc/*_host.cpp) defines MG_HOST_EMU and supplies the four cross-lane moves and the launch shims itself.
#pragma once
#ifndef MG_HOST_EMU
#include "common.h"
#include "../../include/maggie_hip.h"
#define MG_DEVCONST __device__ const

namespace {
// the cross-lane moves of one wave (a host build replaces these four)
__device__ __forceinline__ int pd_shift_up(int v) { return __shfl_up(v, 1, 64); }                  // lane k gets lane k - 1's v (lane 0 its own)
__device__ __forceinline__ int pd_scan(int v) {                                                    // inclusive sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if ((int)(threadIdx.x & 63) >= o) v += u; }
    return v;
}
__device__ __forceinline__ unsigned long long pd_ballot(int p) { return __ballot(p); }
__device__ __forceinline__ unsigned long long pd_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
}  // namespace
#endif

namespace {

constexpr int WV = MG_PNGDEC_THREADS;                                      // one wave
constexpr int RING = 32768, RMASK = RING - 1;                              // the deflate window
constexpr int SB = 4096;                                                   // staged stream bytes
constexpr int TOK = MG_PNGDEC_ROUND_TOKENS;
constexpr int ROUND_BYTES = TOK * 6 + 8;                                   // a token is at most 15 + 5 + 15 + 13 = 48 bits; + one refill
constexpr int HEADER_BYTES = 640;                                          // 17 + 19 * 3 + 316 * (7 + 7) bits = 563 bytes, + refills
constexpr int STORED_CHUNK = 2048;                                         // bytes of a stored block copied per round
constexpr int FLUSH = MG_PNGDEC_FLUSH_BYTES;
constexpr int LLB = 10, DLB = 8;                                           // index bits of the literal/length and of the distance look-up
constexpr unsigned ADLER = 65521u;
static_assert(WV == 64 && TOK >= 1 && TOK <= 64, "one wave, lane t keeps token t");
// a round writes at most TOK * 258 bytes in front of at most FLUSH + 15 pending ones; a ring slot is overwritten 32768 positions later, so
// everything older than that must be in `raw` already
static_assert(FLUSH % 16 == 0 && FLUSH + 16 + TOK * 258 <= RING && FLUSH + 16 + STORED_CHUNK <= RING, "the ring must not overwrite pending bytes");
static_assert(STORED_CHUNK + 24 <= SB && HEADER_BYTES + 24 <= SB && ROUND_BYTES + 24 <= SB,      // 8 back + 3 alignment + what a turn consumes + 8 ahead
              "the stage holds what one turn consumes");

MG_DEVCONST uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// `next`: the stream byte the next refill takes; `pre`: the four bytes at `next`, loaded one refill ahead so that a refill does not wait for LDS
struct Bits { unsigned long long hold; int n; int next; uint32_t pre; };

__device__ __forceinline__ uint32_t pd_word(const uint8_t* sbuf, int o) {
    uint32_t w;
    __builtin_memcpy(&w, sbuf + o, 4);
    return w;
}
// at least 32 bits in `hold` afterwards. The caller keeps next - sbase + 8 <= SB (pd_ensure).
__device__ __forceinline__ void pd_refill(Bits& b, const uint8_t* sbuf, int sbase) {
    if (b.n <= 32) {
        b.hold |= (unsigned long long)b.pre << b.n;
        b.n += 32;
        b.next += 4;
        b.pre = pd_word(sbuf, b.next - sbase);
    }
}
__device__ __forceinline__ int pd_bits(Bits& b, int k) {
    const int v = (int)(b.hold & ((1ull << k) - 1));
    b.hold >>= k;
    b.n -= k;
    return v;
}
__device__ __forceinline__ long pd_consumed(const Bits& b) { return (long)b.next * 8 - b.n; }

// the stream bytes [start - ((off + start) & 3), + SB) into the stage (`start` may be negative: nothing is loaded from in front of the stream), dword loads where the whole dword lies inside the stream, zero past its end
__device__ __forceinline__ int pd_stage(const uint8_t* __restrict__ data, long data_bytes, long off, int len, int start, uint8_t* sbuf, int lane) {
    const int sbase = start - (int)((off + start) & 3);
    __syncthreads();
    for (int i = lane; i < SB / 4; i += WV) {
        const int rel = sbase + 4 * i;
        const long a = off + rel;
        uint32_t v = 0;
        if (rel >= 0 && rel + 4 <= len && a + 4 <= data_bytes) {
            v = *reinterpret_cast<const uint32_t*>(data + a);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (rel + k >= 0 && rel + k < len && a + k < data_bytes) v |= (uint32_t)data[a + k] << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(sbuf + 4 * i) = v;
    }
    __syncthreads();
    return sbase;
}
// The stage is refilled from 8 bytes in front of `next`: the hold carries up to 64 bits that lie in front of `next`, and a stored block hands
// the whole bytes among them back (next -= n >> 3), so that `next` never drops below `sbase`.
constexpr int BACK = 8;
#define pd_ensure(k) do { if (bs.next - sbase + (k) + 8 > SB) sbase = pd_stage(data, data_bytes, off, len, bs.next - BACK, sbuf, lane); } while (0)

// one symbol: the look-up for codes of at most `lb` bits, else the canonical walk (count per length, symbols sorted by code). -1: no such code.
__device__ __forceinline__ int pd_symbol(Bits& b, const uint16_t* lut, int lb, const uint16_t* cnt, const uint16_t* sorted) {
    const uint32_t e = lut[b.hold & ((1u << lb) - 1)];
    if (e) {
        const int l = (int)(e >> 9);
        b.hold >>= l;
        b.n -= l;
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;
    unsigned long long hh = b.hold;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(hh & 1);
        hh >>= 1;
        const int c = cnt[l];
        if (code - c < first) {
            b.hold = hh;
            b.n -= l;
            return sorted[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

enum { SET_CODES = 0, SET_LENS = 1, SET_DISTS = 2 };
// `n` code lengths -> cnt[16], sorted[], lut[1 << lb]. Returns nonzero for a set zlib refuses: over-subscribed; incomplete unless it is a single
// one-bit code of a literal/length or distance set; `checked` = 0 (the fixed sets) skips the test. tmp: code[320], nxt[16], offs[16].
__device__ __forceinline__ int pd_build(const uint8_t* lens, int n, int kind, int checked, uint16_t* lut, int lb, uint16_t* cnt, uint16_t* sorted,
                                        uint16_t* code, uint16_t* nxt, uint16_t* offs, int lane) {
    __syncthreads();
    if (lane < 16) {
        int c = 0;
        for (int s = 0; s < n; ++s) c += lens[s] == lane;
        cnt[lane] = (uint16_t)(lane ? c : 0);
    }
    for (int i = lane; i < (1 << lb); i += WV) lut[i] = 0;
    __syncthreads();
    int left = 1, total = 0, over = 0, maxl = 0;
    for (int l = 1; l <= 15; ++l) {
        const int c = cnt[l];
        left = (left << 1) - c;
        if (left < 0) { over = 1; left = 0; }
        total += c;
        if (c) maxl = l;
    }
    int bad = 0;
    if (checked) {
        if (over) bad = 1;
        else if (total == 0) bad = kind == SET_CODES;                      // no distance code at all is a block of literals only
        else if (left > 0 && (kind == SET_CODES || maxl != 1)) bad = 1;
    }
    if (bad) return 1;
    if (lane == 0) {
        int c = 0, o = 0;
        for (int l = 1; l <= 15; ++l) {
            c <<= 1;
            nxt[l] = (uint16_t)c;
            offs[l] = (uint16_t)o;
            c += cnt[l];
            o += cnt[l];
        }
    }
    __syncthreads();
    if (lane >= 1 && lane < 16) {
        int c = nxt[lane], o = offs[lane];
        for (int s = 0; s < n; ++s)
            if (lens[s] == lane) { code[s] = (uint16_t)c++; sorted[o++] = (uint16_t)s; }
    }
    __syncthreads();
    for (int s = lane; s < n; s += WV) {
        const int l = lens[s];
        if (l >= 1 && l <= lb) {
            int c = code[s], r = 0;
            for (int k = 0; k < l; ++k) { r = (r << 1) | (c & 1); c >>= 1; }
            for (int e = r; e < (1 << lb); e += 1 << l) lut[e] = (uint16_t)(s | (l << 9));
        }
    }
    __syncthreads();
    return 0;
}

// ring[f0, f1) -> raw, 16 bytes per lane and store (f0 is a multiple of 16), and the Adler-32 sums over them: A += sum b, B += n A + sum (n - i) b_i
__device__ __forceinline__ void pd_flush(const uint8_t* ring, uint8_t* __restrict__ rawp, int f0, int f1, unsigned& A, unsigned& B, int lane) {
    const int n = f1 - f0;
    unsigned long long s1 = 0, s2 = 0;
    __syncthreads();
    for (int q = f0 + 16 * lane; q < f1; q += 16 * WV) {
        const int valid = f1 - q < 16 ? f1 - q : 16;
        const uint4 v = *reinterpret_cast<const uint4*>(ring + (q & RMASK));
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
        const int wgt = n - (q - f0);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned byte = k < valid ? (wd[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
            s1 += byte;
            s2 += (unsigned long long)byte * (unsigned)(wgt - k);
        }
        if (valid == 16) {
            *reinterpret_cast<uint4*>(rawp + q) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < valid) rawp[q + k] = (uint8_t)((wd[k >> 2] >> (8 * (k & 3))) & 255u);
        }
    }
    s1 = pd_sum(s1);
    s2 = pd_sum(s2);
    B = (unsigned)(((unsigned long long)B + (unsigned long long)(unsigned)n * A + s2) % ADLER);
    A = (unsigned)(((unsigned long long)A + s1) % ADLER);
}

// The zlib stream data[off, off + len) -> rawp[0, expect), by the whole wave of a 64-lane workgroup. The caller has checked that the stream lies
// inside `data_bytes` and that `expect` bytes fit behind `rawp` (16-byte aligned). inf[0..5]: status, rounds, blocks, tokens, the two Adler-32s.
__device__ __forceinline__ void pd_inflate_file(const uint8_t* __restrict__ data, long data_bytes, long off, int len, int expect,
                                                uint8_t* __restrict__ rawp, int32_t* __restrict__ inf) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[SB + 8];
    __shared__ uint16_t lut_l[1 << LLB], lut_d[1 << DLB], sorted_l[288], sorted_d[32], cnt_l[16], cnt_d[16], code[320], nxt[16], offs[16];
    __shared__ __attribute__((aligned(4))) uint8_t lens[320];
    __shared__ uint8_t clen[20];
    __shared__ uint32_t tok[WV];
    __shared__ int32_t tpos[WV];
    const int lane = (int)threadIdx.x;
    const long endbit = (long)len * 8;
    Bits bs;
    bs.hold = 0; bs.n = 0; bs.next = 0;
    int sbase = pd_stage(data, data_bytes, off, len, 0, sbuf, lane);
    bs.pre = pd_word(sbuf, -sbase);
    pd_refill(bs, sbuf, sbase);
    pd_bits(bs, 16);                                                       // CMF and FLG: checked by the host
    int st = 0, pos = 0, flushed = 0, rounds = 0, blocks = 0, tokens = 0, last = 0;
    unsigned A = 1, B = 0;
    while (!st && !last) {
        pd_ensure(HEADER_BYTES);
        pd_refill(bs, sbuf, sbase);
        last = pd_bits(bs, 1);
        const int type = pd_bits(bs, 2);
        ++blocks;
        if (pd_consumed(bs) > endbit) { st |= MG_PNGDEC_ST_PAST_END; break; }
        if (type == 3) { st |= MG_PNGDEC_ST_BLOCK_TYPE; break; }
        if (type == 0) {
            pd_bits(bs, bs.n & 7);
            pd_refill(bs, sbuf, sbase);
            const int ln = pd_bits(bs, 16), nl = pd_bits(bs, 16);
            if (pd_consumed(bs) > endbit) { st |= MG_PNGDEC_ST_PAST_END; break; }
            if (ln != (~nl & 0xffff)) { st |= MG_PNGDEC_ST_STORED_LEN; break; }
            bs.next -= bs.n >> 3;                                          // n is a multiple of 8 here: give the whole bytes back
            bs.hold = 0; bs.n = 0;
            if (bs.next + ln > len) { st |= MG_PNGDEC_ST_PAST_END; break; }
            if (pos + ln > expect) { st |= MG_PNGDEC_ST_SIZE; break; }
            for (int rem = ln; rem > 0;) {
                const int c = rem < STORED_CHUNK ? rem : STORED_CHUNK;
                pd_ensure(c);
                for (int j = lane; j < c; j += WV) ring[(pos + j) & RMASK] = sbuf[bs.next - sbase + j];
                bs.next += c; pos += c; rem -= c;
                ++rounds;
                if (pos - flushed >= FLUSH) { pd_flush(ring, rawp, flushed, pos & ~15, A, B, lane); flushed = pos & ~15; }
            }
            pd_ensure(8);
            bs.pre = pd_word(sbuf, bs.next - sbase);
            continue;
        }
        if (type == 1) {
            for (int s = lane; s < 320; s += WV) lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : (s < 288 ? 8 : 5))));
            pd_build(lens, 288, SET_LENS, 0, lut_l, LLB, cnt_l, sorted_l, code, nxt, offs, lane);
            pd_build(lens + 288, 32, SET_DISTS, 0, lut_d, DLB, cnt_d, sorted_d, code, nxt, offs, lane);
        } else {
            const int hlit = pd_bits(bs, 5) + 257, hdist = pd_bits(bs, 5) + 1, hclen = pd_bits(bs, 4) + 4;
            if (hlit > 286 || hdist > 30) { st |= MG_PNGDEC_ST_CODE_SET; break; }
            __syncthreads();
            if (lane < 20) clen[lane] = 0;
            __syncthreads();
            for (int i = 0; i < hclen; ++i) {
                pd_refill(bs, sbuf, sbase);
                const int v = pd_bits(bs, 3);
                if (lane == 0) clen[CL_ORDER[i]] = (uint8_t)v;
            }
            if (pd_build(clen, 19, SET_CODES, 1, lut_d, DLB, cnt_d, sorted_d, code, nxt, offs, lane)) { st |= MG_PNGDEC_ST_CODE_SET; break; }
            const int total = hlit + hdist;
            int i = 0, prev = 0;
            while (i < total) {
                pd_refill(bs, sbuf, sbase);
                const int s = pd_symbol(bs, lut_d, DLB, cnt_d, sorted_d);
                if (s < 0 || s > 18) { st |= MG_PNGDEC_ST_CODE_SET; break; }
                int rep = 1, v = s;
                if (s == 16) {
                    if (i == 0) { st |= MG_PNGDEC_ST_CODE_SET; break; }
                    v = prev; rep = 3 + pd_bits(bs, 2);
                } else if (s == 17) { v = 0; rep = 3 + pd_bits(bs, 3); }
                else if (s == 18) { v = 0; rep = 11 + pd_bits(bs, 7); }
                if (i + rep > total) { st |= MG_PNGDEC_ST_CODE_SET; break; }
                if (lane == 0)
                    for (int k = 0; k < rep; ++k) lens[i + k] = (uint8_t)v;
                i += rep;
                prev = v;
            }
            if (st) break;
            if (pd_consumed(bs) > endbit) { st |= MG_PNGDEC_ST_PAST_END; break; }
            __syncthreads();
            if (lens[256] == 0) { st |= MG_PNGDEC_ST_CODE_SET; break; }    // no end-of-block code
            if (pd_build(lens, hlit, SET_LENS, 1, lut_l, LLB, cnt_l, sorted_l, code, nxt, offs, lane) ||
                pd_build(lens + hlit, hdist, SET_DISTS, 1, lut_d, DLB, cnt_d, sorted_d, code, nxt, offs, lane)) { st |= MG_PNGDEC_ST_CODE_SET; break; }
        }
        // the rounds of a Huffman block
        for (int eob = 0; !eob && !st;) {
            pd_ensure(ROUND_BYTES);
            int ntok = 0, produced = 0, mylen = 0;
            uint32_t mytok = 0;
            while (ntok < TOK) {
                pd_refill(bs, sbuf, sbase);
                const int s = pd_symbol(bs, lut_l, LLB, cnt_l, sorted_l);
                if (s < 0 || s >= 286) { st |= MG_PNGDEC_ST_SYMBOL; break; }
                uint32_t t;
                int tl;
                if (s < 256) { t = (uint32_t)s; tl = 1; }
                else if (s == 256) {
                    if (pd_consumed(bs) > endbit) st |= MG_PNGDEC_ST_PAST_END;
                    eob = 1;
                    break;
                } else {
                    const int li = s - 257, le = li < 8 || li == 28 ? 0 : (li >> 2) - 1;
                    tl = (li < 8 ? 3 + li : (li == 28 ? 258 : 3 + ((4 + (li & 3)) << le))) + pd_bits(bs, le);
                    pd_refill(bs, sbuf, sbase);
                    const int d = pd_symbol(bs, lut_d, DLB, cnt_d, sorted_d);
                    if (d < 0 || d >= 30) { st |= MG_PNGDEC_ST_SYMBOL; break; }
                    const int de = d < 4 ? 0 : (d >> 1) - 1;
                    const int dist = (d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << de)) + pd_bits(bs, de);
                    if (dist > pos + produced) { st |= MG_PNGDEC_ST_DISTANCE; break; }
                    t = (uint32_t)tl | ((uint32_t)dist << 16);
                }
                if (pd_consumed(bs) > endbit) { st |= MG_PNGDEC_ST_PAST_END; break; }
                if (pos + produced + tl > expect) { st |= MG_PNGDEC_ST_SIZE; break; }
                if (lane == ntok) { mytok = t; mylen = tl; }
                ++ntok;
                produced += tl;
            }
            // expansion: lane t holds token t. A literal is written before the first match behind it (so that a match may copy it) and not
            // before the matches in front of it: its slot is that of the byte 32 768 positions back, which those may still have to read.
            const int mypos = pos + pd_scan(mylen) - mylen;
            __syncthreads();
            tok[lane] = mytok;
            tpos[lane] = mypos;
            bool pending = lane < ntok && (mytok >> 16) == 0;
            unsigned long long m = pd_ballot(lane < ntok && (mytok >> 16) != 0);
            if (pending && (m == 0 || lane < __builtin_ctzll(m))) { ring[mypos & RMASK] = (uint8_t)mytok; pending = false; }
            __syncthreads();
            while (m) {
                const int t = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t tk = tok[t];
                const int ml = (int)(tk & 0xffffu), md = (int)(tk >> 16), mp = tpos[t];
                int v[5];                                                  // 5 x 64 >= 258: all source bytes read, then all bytes written
                if (md >= ml) {
#pragma unroll
                    for (int c = 0; c < 5; ++c) { const int j = c * WV + lane; v[c] = j < ml ? ring[(mp - md + j) & RMASK] : 0; }
                } else if (md == 1) {
                    const int one = ring[(mp - 1) & RMASK];
#pragma unroll
                    for (int c = 0; c < 5; ++c) v[c] = one;
                } else {
#pragma unroll
                    for (int c = 0; c < 5; ++c) { const int j = c * WV + lane; v[c] = j < ml ? ring[(mp - md + j % md) & RMASK] : 0; }
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 5; ++c) { const int j = c * WV + lane; if (j < ml) ring[(mp + j) & RMASK] = (uint8_t)v[c]; }
                if (pending && (m == 0 || lane < __builtin_ctzll(m))) { ring[mypos & RMASK] = (uint8_t)mytok; pending = false; }
                __syncthreads();
            }
            pos += produced;
            tokens += ntok;
            ++rounds;
            if (pos - flushed >= FLUSH) { pd_flush(ring, rawp, flushed, pos & ~15, A, B, lane); flushed = pos & ~15; }
        }
    }
    unsigned trailer = 0;
    if (!st) {
        if (pos != expect) st |= MG_PNGDEC_ST_SIZE;
        pd_ensure(16);
        pd_bits(bs, bs.n & 7);
        pd_refill(bs, sbuf, sbase);
        const unsigned tw = (unsigned)(bs.hold & 0xffffffffu);
        pd_bits(bs, 32);
        trailer = (tw >> 24) | ((tw >> 8) & 0xff00u) | ((tw << 8) & 0xff0000u) | (tw << 24);
        if (pd_consumed(bs) > endbit) st |= MG_PNGDEC_ST_PAST_END;
    }
    if (!st) {
        pd_flush(ring, rawp, flushed, pos, A, B, lane);
        if (((B << 16) | A) != trailer) st |= MG_PNGDEC_ST_ADLER;
    }
    if (lane == 0) {
        inf[0] = st; inf[1] = rounds; inf[2] = blocks; inf[3] = tokens;
        inf[4] = (int32_t)((B << 16) | A); inf[5] = (int32_t)trailer;
    }
}

}  // namespace
