// Progressive JPEG decoding on the device: the scans of T SOF2 files of one geometry, in any of jpegdec.hip's six layouts -> its coefficient buffer (int16
//   [frames][blocks][64], natural order, interleaved MCU order with the padding blocks, DC terms final). Everything behind the coefficients is
//   jpegdec.hip's (mg_jpegdec_idct and the colour kernels), unchanged.
//
// A refinement scan cannot be cut into subsequences: the bits a block takes depend on which of its coefficients earlier scans made non-zero, so
//   a lane that does not know its block cannot decode. What IS independent: the DC scans of a file, the AC scans of each component, and the
//   files. Each of these is a CHAIN of scans in file order, and one wave runs one chain: jp_chain_kernel, one workgroup of 64 lanes per chain.
//   Lane k holds the coefficient at zig-zag index k of the current block. The bit reader, the Huffman decoding and the cursor are computed by
//   every lane alike (wave-uniform, kept in scalar registers); what is per lane is the coefficient, its correction bit and its store:
//     DC first               lane 0 stores pred << Al.
//     DC refinement          one bit per block: up to 64 blocks a round, lane i ORs 1 << Al into the DC term of the round's block i.
//     AC first               the lane whose index is the cursor stores extend(receive(s), s) << Al; an end-of-band run skips its blocks unread.
//     AC refinement          hist = ballot(coefficient non-zero and in the band). A symbol (r, s) moves the cursor to the zero of rank r among
//                            the clear bits of hist from the cursor on; the set bits in between each take one correction bit, a lane's own
//                            being the one at its rank among them. The new value goes to the lane the cursor stopped at. A value placed in
//                            this scan lies behind the cursor, so hist is taken once per block. The coefficients of 16 blocks are read
//                            ahead into LDS at once: only a block's own turn changes its band.
//   An AC chain never stores coefficient 0 and the DC chain stores nothing else, and every store is one int16, so all chains of all files share
//   one launch. No wave waits for another. Every loop runs under a bound from the sizes passed in (blocks, 64 symbols per block, four bytes per
//   refill); a corrupt stream sets a status bit in info[frame] and ends the chain.
// The scan's Huffman words (two tables of jpeg_common.h's HT words) and a window of the segment's bytes live in LDS. The reader skips a stuffed 0x00
//   behind a data 0xFF and stops in front of any marker; a restart realigns to the byte, checks RSTn's number and resets the predictors and
//   the end-of-band run.
#ifndef MG_HOST_EMU
#include "common.h"
#include "../../include/maggie_hip.h"
#define MG_DEVCONST __device__ const
__device__ __forceinline__ unsigned long long jp_ballot(int p) { return __ballot(p); }
// what every lane read alike from LDS, moved to a scalar register: the reader's state and the cursor then live in SGPRs and run on the scalar unit
#define JP_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define JP_UNI(x) ((int)(x))
#endif

namespace {
#include "jpeg_common.h"

constexpr int NL = MG_JPEGPROG_THREADS;                                    // lanes of a chain's wave
constexpr int SW = MG_JPEGPROG_SCAN_WORDS, CW = MG_JPEGPROG_CHAIN_WORDS;
constexpr int S_OFF = 2 * HT, S_LEN = S_OFF + 1, S_RI = S_OFF + 2, S_SS = S_OFF + 3, S_SE = S_OFF + 4, S_AH = S_OFF + 5, S_AL = S_OFF + 6;
constexpr int S_NSLOT = S_OFF + 7, S_COMP = S_OFF + 8, S_SLOT = S_OFF + 10, HDR = 24;
constexpr int AHEAD = 16;                                                  // blocks a refinement scan reads ahead
constexpr int WIN = 2048;                                                  // bytes of the segment held in LDS
constexpr int STOP_NONE = 0, STOP_RST = 1, STOP_END = 2;
static_assert(NL == 64 && S_OFF + HDR == SW && S_SLOT + 6 <= SW, "record layout");

MG_DEVCONST uint8_t JP_NATURAL[64] = MG_JPEG_ZIGZAG;

// ---- the bit reader: wave-uniform, its bytes through an LDS window ------------------------------------------------------------------------------
struct Bits {
    const uint8_t* d;                                                      // the scan's segment
    uint8_t* win;                                                          // LDS, WIN bytes from raw byte `base`
    unsigned long long buf;                                                // `cnt` data bits, left-aligned, zeros behind them; a fill leaves 32 or more
    int len, cnt, rp, stop, base;
};

// the window moves to raw byte i (rounded down to a dword of the window); every lane of the wave calls with the same i
__device__ __forceinline__ void jp_refill(Bits& r, int i) {
    __syncthreads();
    r.base = i & ~3;
    for (int k = threadIdx.x; k < WIN + 4 && r.base + k < r.len; k += NL) r.win[k] = r.d[r.base + k];
    __syncthreads();
}

__device__ __forceinline__ unsigned jp_byte(Bits& r, int i) {              // 0 <= i < r.len
    if (i < r.base || i >= r.base + WIN) jp_refill(r, i);
    return (unsigned)JP_UNI(r.win[i - r.base]);
}

__device__ __forceinline__ unsigned jp_word(Bits& r, int i) {              // raw bytes i .. i + 3 (i + 4 <= r.len), the first one on top
    if (i < r.base || i + 4 > r.base + WIN) jp_refill(r, i);
    const int o = i - r.base;
    const uint32_t* w = (const uint32_t*)r.win + (o >> 2);
    const unsigned long long v = (unsigned long long)(unsigned)JP_UNI(w[0]) | ((unsigned long long)(unsigned)JP_UNI(w[1]) << 32);
    return __builtin_bswap32((unsigned)(v >> (8 * (o & 3))));
}

// the reader's state is the same in every lane; said again where a symbol starts, so that it is kept in scalar registers whatever the control
// flow in between looked like to the compiler
__device__ __forceinline__ void jp_uniform(Bits& r) {
    r.buf = (unsigned long long)(unsigned)JP_UNI((unsigned)r.buf) | ((unsigned long long)(unsigned)JP_UNI((unsigned)(r.buf >> 32)) << 32);
    r.cnt = JP_UNI(r.cnt); r.rp = JP_UNI(r.rp); r.stop = JP_UNI(r.stop); r.base = JP_UNI(r.base);
}

__device__ __forceinline__ void jp_open(Bits& r, int at) { r.buf = 0; r.cnt = 0; r.rp = at; r.stop = STOP_NONE; }

__device__ __forceinline__ void jp_fill(Bits& r) {
    if (r.cnt <= 32 && r.stop == STOP_NONE && r.rp + 4 <= r.len) {         // four bytes at once when none of them is 0xFF
        const unsigned x = jp_word(r, r.rp), y = ~x;
        if (((y - 0x01010101u) & ~y & 0x80808080u) == 0) {
            r.buf |= (unsigned long long)x << (32 - r.cnt);
            r.cnt += 32;
            r.rp += 4;
        }
    }
    for (int it = 0; it < 4 && r.cnt < 32 && r.stop == STOP_NONE; ++it) {                       // byte by byte: stuffing, markers, the tail
        if (r.rp >= r.len) { r.stop = STOP_END; break; }
        const unsigned b = jp_byte(r, r.rp);
        int step = 1;
        if (b == 0xFF) {
            const unsigned n = r.rp + 1 < r.len ? jp_byte(r, r.rp + 1) : 0xD9u;
            if (n == 0) step = 2;
            else { r.stop = (n >= 0xD0 && n <= 0xD7) ? STOP_RST : STOP_END; break; }
        }
        r.buf |= (unsigned long long)b << (56 - r.cnt);
        r.cnt += 8;
        r.rp += step;
    }
}

// receive(n), 0 <= n <= 32; a read past the data sets MG_JPEGDEC_ST_PAST_END
__device__ __forceinline__ unsigned jp_take(Bits& r, int n, int& status) {
    if (n <= 0) return 0u;
    jp_uniform(r);
    if (r.cnt < n) jp_fill(r);
    if (r.cnt < n) { status |= MG_JPEGDEC_ST_PAST_END; return 0u; }
    const unsigned v = (unsigned)(r.buf >> (64 - n));
    r.buf <<= n;
    r.cnt -= n;
    return v;
}

__device__ __forceinline__ unsigned long long jp_take_long(Bits& r, int n, int& status) {          // 0 <= n <= 64
    if (n <= 32) return jp_take(r, n, status);
    const unsigned long long hi = jp_take(r, n - 32, status);
    return (hi << 32) | jp_take(r, 32, status);
}

// one Huffman symbol from the table at `tb` (LDS): the leading 8 bits, then the canonical walk over lengths 9..16
__device__ __forceinline__ int jp_symbol(Bits& r, const int* tb, int& status) {
    jp_uniform(r);
    if (r.cnt < 32) jp_fill(r);                                            // a code and its value bits then need no second fill
    const unsigned peek = (unsigned)(r.buf >> 48);
    int len_c = 0, sym = 0;
    const unsigned e = (unsigned)JP_UNI(((const uint16_t*)tb)[peek >> 8]);
    if (e) { len_c = (int)(e >> 8); sym = (int)(e & 255u); }
    else {
        for (int l = 9; l <= 16; ++l) {
            const int code = (int)(peek >> (16 - l));
            if (code <= JP_UNI(tb[HT_MAXCODE + l])) {
                const int idx = JP_UNI(tb[HT_VALOFF + l]) + code;
                if ((unsigned)idx < 256u) { len_c = l; sym = JP_UNI(((const uint8_t*)(tb + HT_VALS))[idx]); }
                break;
            }
        }
    }
    if (len_c == 0) {                                                      // fewer bits than a code, or an unassigned one
        status |= r.cnt < 16 && r.stop != STOP_NONE ? MG_JPEGDEC_ST_PAST_END : MG_JPEGDEC_ST_CODE;
        return 0;
    }
    if (len_c > r.cnt) { status |= MG_JPEGDEC_ST_PAST_END; return 0; }
    r.buf <<= len_c;
    r.cnt -= len_c;
    return sym;
}

__device__ __forceinline__ int jp_extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// a restart in front of interval number `done` (1, 2, ...): what is left of the last byte is padding, RSTn carries (done - 1) mod 8
__device__ __forceinline__ void jp_restart(Bits& r, int done, int& status) {
    jp_fill(r);
    if (r.cnt >= 8 || r.stop != STOP_RST || r.rp + 1 >= r.len || (int)(jp_byte(r, r.rp + 1) & 7u) != ((done - 1) & 7)) {
        status |= MG_JPEGDEC_ST_RESTART;
        return;
    }
    jp_open(r, r.rp + 2);
}

struct Geo { int bpm, mcux, mcuy, ncomp, hl, vl; };                        // hl, vl: log2 of the luma blocks per MCU row and column
// the struct of a layout (jpeg_common.h); false for anything but the six
bool jp_geo(int layout, int h, int w, Geo& g) {
    JpegLayout l;
    if (!jpeg_layout(layout, h, w, l)) return false;
    g.bpm = l.bpm; g.mcux = l.mcux; g.mcuy = l.mcuy; g.ncomp = l.ncomp;
    g.hl = l.hs == 4 ? 2 : l.hs - 1;
    g.vl = l.vs == 4 ? 2 : l.vs - 1;
    return true;
}

// block (by, bx) of component `comp`, counted over the component's real blocks -> its index in the MCU-major buffer: a luma block lives in MCU
// (by / vs, bx / hs), slot (by % vs) * hs + bx % hs; the chroma slots follow the hs * vs luma slots
__device__ __forceinline__ long jp_at(int by, int bx, int comp, const Geo& g) {
    if (comp == 0)
        return ((long)(by >> g.vl) * g.mcux + (bx >> g.hl)) * g.bpm + ((by & ((1 << g.vl) - 1)) << g.hl) + (bx & ((1 << g.hl) - 1));
    return ((long)by * g.mcux + bx) * g.bpm + (1 << (g.hl + g.vl)) + comp - 1;
}
// the same for block n of the component's raster order (`bw` blocks per row)
__device__ __forceinline__ long jp_block(int n, int bw, int comp, const Geo& g) { return jp_at(n / bw, n % bw, comp, g); }

// one scan of a chain; returns its status bits. `cf`: the frame's coefficients; `s_tab` / `s_win`: LDS.
__device__ __forceinline__ int jp_scan(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ rec, int16_t* __restrict__ cf,
                                       int h, int w, const Geo& g, int* s_tab, uint8_t* s_win, int16_t* s_stage) {
    const int lane = threadIdx.x;
    __syncthreads();                                                       // the scan before is done with the LDS
    for (int k = lane; k < SW; k += NL) s_tab[k] = rec[k];
    __syncthreads();
    const int off = JP_UNI(s_tab[S_OFF]), len = JP_UNI(s_tab[S_LEN]), ri = JP_UNI(s_tab[S_RI]), Ss = JP_UNI(s_tab[S_SS]), Se = JP_UNI(s_tab[S_SE]);
    const int Ah = JP_UNI(s_tab[S_AH]), Al = JP_UNI(s_tab[S_AL]), nslot = JP_UNI(s_tab[S_NSLOT]), comp = JP_UNI(s_tab[S_COMP]);
    if (off < 0 || len < 0 || (long)off + len > data_bytes || ri < 0 || Ss < 0 || Se > 63 || Ss > Se || (Ss == 0 && Se != 0) || Ah < 0 || Ah > 13 ||
        Al < 0 || Al > 13 || nslot < 0 || nslot > g.bpm || comp < 0 || comp >= g.ncomp || (Ss > 0 && nslot != 0))
        return MG_JPEGPROG_ST_RECORD;
    for (int k = 0; k < nslot; ++k) {
        const int sl = s_tab[S_SLOT + k];
        if ((sl & 15) >= g.bpm || ((sl >> 4) & 15) >= g.ncomp || (sl >> 8) < 0 || (sl >> 8) > 1) return MG_JPEGPROG_ST_RECORD;
    }
    // the units of the scan: MCUs when it is interleaved, else the component's real blocks in raster order
    const int bw = nslot == 0 && comp == 0 ? (w + 7) / 8 : g.mcux;        // a chroma component has one block per MCU: its real blocks are the MCUs
    const int bh = nslot == 0 && comp == 0 ? (h + 7) / 8 : g.mcuy;
    const int units = bw * bh, per = nslot ? nslot : 1;
    const int nat = JP_NATURAL[lane];
    Bits r;
    r.d = data + off; r.win = s_win; r.len = len; r.base = -(1 << 30);
    jp_open(r, 0);
    int status = 0, eobrun = 0, pred0 = 0, pred1 = 0, pred2 = 0, done = 0;
    int togo = ri > 0 ? ri : 0x7fffffff;
    const int p1 = 1 << Al, m1 = -(1 << Al);
    const bool band = lane >= Ss && lane <= Se;
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;  // the lanes in front of this one
    const unsigned long long upto_se = ~0ull >> (63 - Se);
    // an AC scan walks its component's blocks with a cursor; a refinement scan reads the coefficients of AHEAD blocks at once into LDS, so that the
    // wave pays the way to memory once per AHEAD blocks (nothing but a block's own turn changes its band: what is read early is what the scans
    // before left)
    int by = 0, bx = 0, qy = 0, qx = 0, staged = 0;                        // blocks [staged - AHEAD, staged) are in s_stage
    for (int unit = 0; unit < units && status == 0;) {                     // every round advances `unit`
        if (togo == 0) {
            done += 1;
            jp_restart(r, done, status);
            if (status) break;
            pred0 = pred1 = pred2 = 0; eobrun = 0; togo = ri;
        }
        if (Ss == 0 && Ah == 0) {                                          // ---- DC first: the blocks of one unit
            for (int k = 0; k < per && status == 0; ++k) {
                const int sl = nslot ? JP_UNI(s_tab[S_SLOT + k]) : (comp << 4);
                const int c = (sl >> 4) & 15;
                const long blk = nslot ? (long)unit * g.bpm + (sl & 15) : jp_block(unit, bw, comp, g);
                const int s = jp_symbol(r, s_tab + HT * (sl >> 8), status);
                if (s > 11) status |= MG_JPEGDEC_ST_CODE;
                if (status) break;
                const int diff = jp_extend((int)jp_take(r, s, status), s);
                int& pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                pred += diff;
                if (lane == 0 && status == 0) cf[blk * 64] = (int16_t)(pred * p1);
            }
            unit += 1; togo -= 1;
        } else if (Ss == 0) {                                              // ---- DC refinement: one bit per block, a lane per block of the round
            const int m = min(min(NL / per, togo), units - unit), nb = m * per;
            const unsigned long long bits = jp_take_long(r, nb, status);
            if (status == 0 && lane < nb && ((bits >> (nb - 1 - lane)) & 1)) {
                const int u = lane / per, k = lane - u * per;
                const long blk = nslot ? (long)(unit + u) * g.bpm + (s_tab[S_SLOT + k] & 15) : jp_block(unit + u, bw, comp, g);
                cf[blk * 64] = (int16_t)(cf[blk * 64] | p1);
            }
            unit += m; togo -= m;
        } else if (Ah == 0) {                                              // ---- AC first
            if (eobrun > 0) {                                              // the run's blocks take no bits: skip them unread
                const int n = min(eobrun, min(togo, units - unit));
                eobrun -= n; unit += n; togo -= n;
                bx += n;
                if (bx >= bw) { by += bx / bw; bx %= bw; }
                continue;
            }
            int16_t* __restrict__ p = cf + jp_at(by, bx, comp, g) * 64;
            int k = Ss;
            for (int it = 0; it < 64 && k <= Se && status == 0; ++it) {
                const int rs = jp_symbol(r, s_tab, status), rr = rs >> 4, s = rs & 15;
                if (status) break;
                if (s) {
                    k += rr;
                    const int v = jp_extend((int)jp_take(r, s, status), s);
                    if (k > Se) status |= MG_JPEGDEC_ST_INDEX;
                    else if (lane == k && status == 0) p[nat] = (int16_t)(v * p1);
                    k += 1;
                } else if (rr == 15) k += 16;
                else {
                    eobrun = (1 << rr) + (int)jp_take(r, rr, status) - 1;
                    break;
                }
            }
            unit += 1; togo -= 1;
            if (++bx == bw) { bx = 0; by += 1; }
        } else {                                                           // ---- AC refinement
            int16_t* __restrict__ p = cf + jp_at(by, bx, comp, g) * 64;
            if (unit >= staged) {                                          // unit == staged: the cursor (qy, qx) is at this block
                int v[AHEAD];
                __syncthreads();
#pragma unroll
                for (int j = 0; j < AHEAD; ++j) {
                    v[j] = band && staged + j < units ? (int)cf[jp_at(qy, qx, comp, g) * 64 + nat] : 0;
                    if (++qx == bw) { qx = 0; qy += 1; }
                }
#pragma unroll
                for (int j = 0; j < AHEAD; ++j) s_stage[j * NL + lane] = (int16_t)v[j];
                staged += AHEAD;
                __syncthreads();
            }
            int c = s_stage[(unit - (staged - AHEAD)) * NL + lane];
            const int c0 = c;
            const unsigned long long hist = jp_ballot(c != 0);
            int k = Ss;
            if (eobrun == 0) {
                for (int it = 0; it < 64 && k <= Se && status == 0; ++it) {
                    const int rs = jp_symbol(r, s_tab, status), s = rs & 15;
                    int rr = rs >> 4, val = 0;
                    if (status) break;
                    if (s) {
                        if (s != 1) { status |= MG_JPEGPROG_ST_REFINE; break; }
                        val = jp_take(r, 1, status) ? p1 : m1;
                    } else if (rr < 15) {
                        eobrun = (1 << rr) + (int)jp_take(r, rr, status);
                        break;
                    }
                    const unsigned long long from = upto_se & ~((1ull << k) - 1ull);              // k..Se
                    unsigned long long z = ~hist & from;
                    for (int q = 0; q < rr; ++q) z &= z - 1;                                       // drop the rr zeros that are skipped
                    const int stop = z ? __builtin_ctzll(z) : Se + 1;
                    const unsigned long long corr = hist & from & ((stop < 64 ? 1ull << stop : 0ull) - 1ull);
                    const int n = __builtin_popcountll(corr);
                    const unsigned long long cb = jp_take_long(r, n, status);
                    if (status) break;
                    if ((corr >> lane) & 1) {
                        const int rank = __builtin_popcountll(corr & below);
                        if (((cb >> (n - 1 - rank)) & 1) && (c & p1) == 0) c += c >= 0 ? p1 : m1;
                    }
                    if (val) {
                        if (stop > Se) { status |= MG_JPEGPROG_ST_REFINE; break; }
                        if (lane == stop) c = val;
                    }
                    k = stop + 1;
                }
            }
            if (eobrun > 0 && status == 0) {                               // inside a run: every non-zero coefficient left in the band is corrected
                const unsigned long long corr = k <= Se ? hist & upto_se & ~((1ull << k) - 1ull) : 0ull;
                const int n = __builtin_popcountll(corr);
                const unsigned long long cb = jp_take_long(r, n, status);
                if (status == 0 && ((corr >> lane) & 1)) {
                    const int rank = __builtin_popcountll(corr & below);
                    if (((cb >> (n - 1 - rank)) & 1) && (c & p1) == 0) c += c >= 0 ? p1 : m1;
                }
                eobrun -= 1;
            }
            if (band && c != c0 && status == 0) p[nat] = (int16_t)c;
            unit += 1; togo -= 1;
            if (++bx == bw) { bx = 0; by += 1; }
        }
    }
    if (status == 0) {                                                     // what is left of the segment is the padding of its last byte
        jp_fill(r);
        if (r.cnt >= 8 || r.stop == STOP_RST) status |= MG_JPEGPROG_ST_EXTRA;
    }
    return status;
}

__global__ __launch_bounds__(NL) void jp_chain_kernel(const uint8_t* __restrict__ data, long data_bytes, const int32_t* __restrict__ scans, long nscans,
                                                      const int32_t* __restrict__ chains, int16_t* __restrict__ coef, int32_t* __restrict__ info,
                                                      long frames, int h, int w, Geo g) {
    __shared__ int s_tab[SW];
    __shared__ uint32_t s_win32[WIN / 4 + 2];                               // jp_word reads the dword behind the window's last
    uint8_t* s_win = (uint8_t*)s_win32;
    __shared__ int16_t s_stage[AHEAD * NL];
    const int32_t* __restrict__ ch = chains + (long)blockIdx.x * CW;
    const long t = ch[0], first = ch[1], n = ch[2];
    if (t < 0 || t >= frames) return;
    int status = 0;
    if (first < 0 || n < 0 || first + n > nscans) status = MG_JPEGPROG_ST_RECORD;
    int16_t* __restrict__ cf = coef + t * (long)g.mcux * g.mcuy * g.bpm * 64;
    for (long k = 0; k < n && status == 0; ++k) status = jp_scan(data, data_bytes, scans + (first + k) * SW, cf, h, w, g, s_tab, s_win, s_stage);
    if (status && threadIdx.x == 0) atomicOr(&info[t], status);
}

}  // namespace

extern "C" int mg_jpegprog_limits(int* threads, int* scan_words, int* chain_words) {
    if (!threads || !scan_words || !chain_words) return -2;
    *threads = NL; *scan_words = SW; *chain_words = CW;
    return 0;
}

extern "C" int mg_jpegprog_chains(const uint8_t* data, long data_bytes, const int32_t* scans, long nscans, const int32_t* chains, long nchains,
                                  int16_t* coef, long coef_elems, int32_t* info, long frames, int h, int w, int layout, void* stream) {
    Geo g;
    if (jpeg_bad_size(frames, h, w) || data_bytes < 0 || data_bytes > MG_JPEGDEC_MAX_BYTES || nscans < 0 || nchains < 0 || !jp_geo(layout, h, w, g))
        return -2;
    const long nbf = (long)g.mcux * g.mcuy * g.bpm;
    if (nbf > 0x7fffffffL / 64 || coef_elems != frames * nbf * 64) return -2;
    if (frames == 0 || nchains == 0) return 0;
    if (!data || !scans || !chains || !coef || !info) return -2;
    if (nchains > 0x7fffffffL) return -3;
    hipLaunchKernelGGL(jp_chain_kernel, dim3((unsigned)nchains), dim3(NL), 0, (hipStream_t)stream, data, data_bytes, scans, nscans, chains, coef, info,
                       frames, h, w, g);
    MG_CHECK_LAUNCH();
    return 0;
}
