// MotionBlur of the video training stream on uint8 frames and alpha planes (reference: maggie/dataloader/transforms.py:965-1034, wired in
//   vim.py:52). The kernel albumentations draws is one 8-connected line of n <= 49 ones in a ksize x ksize box divided by n, so a plane is
//     out[y][x] = rhe( sum_k src[r101(y + dy_k, h)][r101(x + dx_k, w)] / n )
//   with r101 = BORDER_REFLECT_101 and rhe = round-half-to-even of the exact rational S / n. Integer work only.
//
// motion_kernel<PS, EPI>   PS = bytes per pixel of a row: 1 for planes, 3 for interleaved frames, whose row is just a byte row with taps 3 dx
//   apart. A workgroup owns MG_MOTION_TILE_ROWS x MG_MOTION_TILE_COLS output pixels, i.e. rows of TB = TILE_COLS * PS bytes.
//   Table: every lane walks the n taps of the DEVICE table (uniform, so scalar loads), clamps n to 1..49 and each offset to +-24, and takes the
//   bounding box lo_y..hi_y, lo_x..hi_x; lane k < n keeps tap k's LDS byte offset in s_off. Nothing of the launch depends on the table.
//   Stage: the tile plus the box as BYTES in LDS, rows at a pitch of PITCH dwords. LDS column 0 is source byte column a0 = the tile's first
//   needed column rounded DOWN to 4, so a dword of LDS is a dword of the source row whenever rows start on dwords (`wide_in`: base and row
//   bytes multiples of 4): one 4-byte load and one ds_write_b32 per dword that lies inside the row; dwords that touch the border, and every
//   dword of an unaligned source, are put together from four byte loads through r101 on the pixel index. Rows come through r101 too. A source
//   byte is fetched once per tile (a reflected copy is a second LDS position, so a second fetch).
//   Sum: a lane owns 4 adjacent output bytes. Per tap it reads the two dwords around its unaligned 4 bytes, v_alignbyte_b32 brings them
//   together, and bytes 0, 2 and bytes 1, 3 are added into two registers of two 16-bit fields each (49 * 255 = 12 495 < 65 536). Lanes of a
//   row read consecutive dwords; PITCH = 16 mod 32 keeps the rows of one 32-lane half on different banks when a half spans two rows.
//   Round: q = S / n by multiplication with ceil(2^32 / n) (exact while S * n < 2^32), r = S - q n, + 1 when 2 r > n or (2 r == n and q odd).
//   Store: one dword of raw bytes when the row allows (`wide_out`), per byte otherwise; MG_PHOTO_NORM writes the fp32 planes of pixel_norm.h.
#include "common.h"
#include "../../include/maggie_hip.h"
#include "pixel_norm.h"

namespace {

constexpr int TR = MG_MOTION_TILE_ROWS, TC = MG_MOTION_TILE_COLS, NT = MG_MOTION_THREADS;
constexpr int REACH = MG_MOTION_MAX_KSIZE / 2;                             // 24
constexpr int ROWS = TR + 2 * REACH;                                       // staged rows at most
static_assert(MG_MOTION_MAX_KSIZE % 2 == 1 && MG_MOTION_MAX_TAPS * 255 < 65536, "two 16-bit sums per register");
static_assert(NT % 64 == 0 && NT >= MG_MOTION_MAX_TAPS, "whole waves; one lane per tap");

template <int PS>
struct Geo {
    static constexpr int TB = TC * PS;                                      // output bytes of a tile row
    // bytes from a0 to the last needed column: at most 3 of rounding, the tile, the box; + 1 dword for the second read of the last lane
    static constexpr int NEED = (3 + TB + 2 * REACH * PS + 3) / 4 + 1;
    static constexpr int PITCH = ((NEED + 15) / 32) * 32 + 16;              // dwords, = 16 mod 32
    static_assert(TB % 4 == 0 && PITCH >= NEED, "a lane owns 4 bytes");
};

// BORDER_REFLECT_101 in closed form: the loop `p = -p` / `p = 2 (len - 1) - p` has period 2 (len - 1)
__device__ __forceinline__ int r101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * (len - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int PS, int EPI>
__global__ __launch_bounds__(NT) void motion_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, const int32_t* __restrict__ taps, int h,
                                                    int w, int tiles_x, int tiles, int wide_in, int wide_out, float m0, float m1, float m2,
                                                    float s0, float s1, float s2) {
    using G = Geo<PS>;
    __shared__ uint32_t s_px[ROWS * G::PITCH];
    __shared__ int s_off[MG_MOTION_MAX_TAPS];
    const int tid = threadIdx.x;
    const long p = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - p * tiles);
    const int ty0 = (tile / tiles_x) * TR, bx0 = (tile % tiles_x) * G::TB;  // first output row, first output byte column
    const int RB = w * PS;                                                  // bytes of a row
    const int rows_out = min(TR, h - ty0), tb = min(G::TB, RB - bx0);

    // ---- the table: n, the box, the LDS offset of every tap ----
    const int n = clampi(taps[0], 1, MG_MOTION_MAX_TAPS);                   // a table rewritten on the device may hold anything
    int lo_y = REACH, hi_y = -REACH, lo_x = REACH, hi_x = -REACH;
    for (int k = 0; k < n; ++k) {
        const int dy = clampi(taps[2 + 2 * k], -REACH, REACH), dx = clampi(taps[3 + 2 * k], -REACH, REACH);
        lo_y = min(lo_y, dy); hi_y = max(hi_y, dy); lo_x = min(lo_x, dx); hi_x = max(hi_x, dx);
    }
    if (tid < n) {
        const int dy = clampi(taps[2 + 2 * tid], -REACH, REACH), dx = clampi(taps[3 + 2 * tid], -REACH, REACH);
        s_off[tid] = (dy - lo_y) * (G::PITCH * 4) + dx * PS;
    }

    // ---- stage rows ty0 + lo_y .. and byte columns a0 .. of plane p ----
    const int a0 = (bx0 + lo_x * PS) & ~3;                                  // rounds down, also below zero
    const int nw = (bx0 + ((tb + 3) & ~3) + hi_x * PS - a0 + 3) >> 2;       // whole 4-byte units of the last lane; <= NEED - 1
    const int rows = rows_out + hi_y - lo_y;                                // <= ROWS
    const uint8_t* __restrict__ src = in + p * ((long)h * RB);
    for (int i = tid; i < rows * nw; i += NT) {
        const int ry = i / nw, cw = i - ry * nw;
        const uint8_t* __restrict__ row = src + (long)r101(ty0 + lo_y + ry, h) * RB;
        const int col = a0 + 4 * cw;
        uint32_t v = 0;
        if (wide_in && col >= 0 && col + 4 <= RB) {
            v = *(const uint32_t*)(row + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = col + e;
                const int px = c >= 0 ? c / PS : -((PS - 1 - c) / PS);       // floor
                v |= (uint32_t)row[r101(px, w) * PS + (c - px * PS)] << (8 * e);
            }
        }
        s_px[ry * G::PITCH + cw] = v;
    }
    __syncthreads();

    // ---- n taps out of LDS, round, store ----
    const unsigned magic = 0xFFFFFFFFu / (unsigned)n + 1u;                  // ceil(2^32 / n); wraps to 0 at n = 1, where it is not used
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    constexpr int UPR = G::TB / 4;                                          // lanes' units per tile row
    for (int u = tid; u < TR * UPR; u += NT) {
        const int ly = u / UPR, bl = (u - ly * UPR) * 4;
        if (ly >= rows_out || bl >= tb) continue;
        const int base = ly * (G::PITCH * 4) + (bx0 + bl - a0);
        uint32_t acc02 = 0, acc13 = 0;
        for (int k = 0; k < n; ++k) {
            const int o = base + s_off[k];
            const uint32_t w0 = s_px[o >> 2], w1 = s_px[(o >> 2) + 1];
            const uint32_t v = __builtin_amdgcn_alignbyte(w1, w0, (unsigned)o & 3u);
            acc02 += v & 0x00ff00ffu;
            acc13 += (v >> 8) & 0x00ff00ffu;
        }
        const unsigned S[4] = {acc02 & 0xffffu, acc13 & 0xffffu, acc02 >> 16, acc13 >> 16};
        unsigned res[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned q = n == 1 ? S[e] : __umulhi(S[e], magic);
            const unsigned r2 = 2u * (S[e] - q * (unsigned)n);
            res[e] = q + ((r2 > (unsigned)n || (r2 == (unsigned)n && (q & 1u))) ? 1u : 0u);
        }
        const int y = ty0 + ly, b = bx0 + bl;
        if constexpr (EPI == MG_PHOTO_RAW) {
            uint8_t* __restrict__ dst = (uint8_t*)out + (p * h + y) * (long)RB + b;
            if (wide_out && b + 4 <= RB) {
                *(uint32_t*)dst = res[0] | (res[1] << 8) | (res[2] << 16) | (res[3] << 24);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (b + e < RB) dst[e] = (uint8_t)res[e];
            }
        } else {
            static_assert(PS == 3, "the Normalize epilogue is for frames");
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = b + e, x = c / 3, ch = c - 3 * x;
                if (c < RB) {
                    const float mu = ch == 0 ? mean[0] : (ch == 1 ? mean[1] : mean[2]), sd = ch == 0 ? std[0] : (ch == 1 ? std[1] : std[2]);
                    ((float*)out)[((p * 3 + ch) * h + y) * (long)w + x] = mg_norm_u8((int)res[e], mu, sd);
                }
            }
        }
    }
}

bool bad_size(long count, int h, int w) { return count < 0 || h <= 0 || w <= 0 || h > MG_MOTION_MAX_SIDE || w > MG_MOTION_MAX_SIDE; }

// rows start on dwords: one 4-byte access per dword of a row
int wide_ok(const void* p, int row_bytes) { return (row_bytes % 4 == 0) && ((uintptr_t)p % 4 == 0); }

template <int PS, int EPI>
int launch(const uint8_t* in, void* out, const int32_t* taps, long count, int h, int w, const float* mean3, const float* std3, void* stream) {
    const int tiles_x = (w + TC - 1) / TC;
    const long tiles = (long)tiles_x * ((h + TR - 1) / TR);
    if (count > 0x7fffffffL / tiles) return -3;
    const int wide_in = wide_ok(in, w * PS), wide_out = EPI == MG_PHOTO_RAW ? wide_ok(out, w * PS) : 0;
    hipLaunchKernelGGL((motion_kernel<PS, EPI>), dim3((unsigned)(count * tiles)), dim3(NT), 0, (hipStream_t)stream, in, out, taps, h, w, tiles_x,
                       (int)tiles, wide_in, wide_out, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int mg_motion_limits(int* max_ksize, int* max_taps, int* tile_rows, int* tile_cols, int* table_len, int* max_side) {
    if (!max_ksize || !max_taps || !tile_rows || !tile_cols || !table_len || !max_side) return -2;
    *max_ksize = MG_MOTION_MAX_KSIZE; *max_taps = MG_MOTION_MAX_TAPS; *tile_rows = TR; *tile_cols = TC; *table_len = MG_MOTION_TABLE;
    *max_side = MG_MOTION_MAX_SIDE;
    return 0;
}

extern "C" int mg_motion_frames(const uint8_t* in, void* out, const int32_t* taps, long frames, int h, int w, int epilogue, const float* mean3,
                                const float* std3, void* stream) {
    if (bad_size(frames, h, w) || (epilogue != MG_PHOTO_RAW && epilogue != MG_PHOTO_NORM) || !mean3 || !std3) return -2;
    if (frames == 0) return 0;
    if (!in || !out || !taps || (const void*)in == out) return -2;
    if (epilogue == MG_PHOTO_RAW) return launch<3, MG_PHOTO_RAW>(in, out, taps, frames, h, w, mean3, std3, stream);
    return launch<3, MG_PHOTO_NORM>(in, out, taps, frames, h, w, mean3, std3, stream);
}

extern "C" int mg_motion_planes(const uint8_t* in, uint8_t* out, const int32_t* taps, long planes, int h, int w, void* stream) {
    if (bad_size(planes, h, w)) return -2;
    if (planes == 0) return 0;
    if (!in || !out || !taps || in == out) return -2;
    const float unused[3] = {0.f, 1.f, 1.f};
    return launch<1, MG_PHOTO_RAW>(in, out, taps, planes, h, w, unused, unused, stream);
}
