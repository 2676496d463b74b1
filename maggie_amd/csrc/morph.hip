// Grey-scale morphology with OpenCV's ellipse on uint8 planes, and the dataset ground-truth maps built from it:
//   * transition = [dilate^n(alpha) > erode^n(alpha)]        (reference: maggie/dataloader/utils.py:15-35 as called by him.py:185-189)
//   * trimap     = 2 where alpha >= 128, 1 where transition  (him.py:190-196, vim.py:198-203; k = 25, one pass)
//   * video transition = [dilate^n(union over instances of |a_t - a_{t-1}| > 5) > 0], the same plane in every slot, frame 0 all ones
//                                                            (vim.py:171-183,211 with gen_diff_mask, utils.py:5-13)
// `v -> v / 255` is strictly increasing, so the reference's float comparisons are decided in the uint8 domain: everything here is integer work.
//
// One launch runs all n passes of a 64 x 64 tile out of LDS. The tile is loaded once with a halo of n * (k / 2) rows / columns up / left and
// n * (k - 1 - k / 2) down / right (even k is not symmetric about its anchor); the max image and the min image ping-pong between two LDS
// buffers each, and the region that is still exact shrinks by one element reach per pass until it is the tile. A pixel outside the image
// is "absent" in every pass: it is loaded as 0 / 255 and written back as 0 / 255 by every pass (masked by its coordinates), so a
// computed halo value never leaks in from beyond the border. The epilogue reads the two final images and writes the product.
//
// One pass: a thread owns PX horizontally adjacent pixels and walks the k rows of the element. The PX windows of a row span of length L
// overlap in L - PX + 1 bytes: that core is reduced once, the PX - 1 bytes to its left by a suffix scan and the PX - 1 to its right by a
// prefix scan (van Herk's split, in registers), and pixel q is core (+) left[q] (+) right[q - 1] -- L + PX - 1 LDS byte reads and about
// L / 2 + 2.5 PX three-operand max / min per row instead of PX * L of each. PX = 4 for k <= 8 (lanes along a row: 4-byte stride, no
// bank conflict), PX = 8 above (lanes along a column: the row stride is an odd number of words).
#include "common.h"
#include "../../include/maggie_hip.h"
#include "se_table.h"

namespace {

constexpr int TW = 64, TH = 64, NT = 512;
constexpr int PXMAX = 8;
enum { OUT_RAW = 0, OUT_TRANSITION = 1, OUT_TRIMAP = 2, OUT_DIFF = 3 };

struct MorphArgs {
    const uint8_t* in;
    uint8_t* dil;
    uint8_t* ero;
    float* out;
    const int32_t* kn;             // [frames][2]
    const int32_t* src_of_slot;    // [frames][n_out] or NULL
    int op, halo_max, n_in, n_out, n_slots, H, W, thresh, diff_thresh;
    int tiles_x, tiles_y, stride, buf_bytes;
};

__host__ __device__ inline int lds_stride(int halo_max) {
    // bytes per LDS row: the widest row + the over-read of the last pixel group, as an odd number of words
    int s = (TW + halo_max + PXMAX - 1 + 3) / 4;
    return (s | 1) * 4;
}

template <bool MAX> __device__ __forceinline__ unsigned mm(unsigned a, unsigned b) { return MAX ? max(a, b) : min(a, b); }

// acc[q] (+)= reduction of p[q .. q + L - 1], q = 0 .. PX - 1
template <int PX, bool MAX>
__device__ __forceinline__ void row_span(const uint8_t* __restrict__ p, int L, unsigned (&acc)[PX]) {
    if (L >= PX - 1) {
        unsigned left[PX - 1], right[PX - 1];
#pragma unroll
        for (int q = 0; q < PX - 1; ++q) { left[q] = p[q]; right[q] = p[L + q]; }
        unsigned core = MAX ? 0u : 255u;
        int j = PX - 1;
        for (; j + 4 <= L; j += 4) {                      // four independent reads in flight, two three-operand reductions
            const unsigned b0 = p[j], b1 = p[j + 1], b2 = p[j + 2], b3 = p[j + 3];
            core = mm<MAX>(mm<MAX>(core, mm<MAX>(b0, b1)), mm<MAX>(b2, b3));
        }
        for (; j < L; ++j) core = mm<MAX>(core, p[j]);
#pragma unroll
        for (int q = PX - 3; q >= 0; --q) left[q] = mm<MAX>(left[q], left[q + 1]);
#pragma unroll
        for (int q = 1; q < PX - 1; ++q) right[q] = mm<MAX>(right[q], right[q - 1]);
        acc[0] = mm<MAX>(acc[0], mm<MAX>(core, left[0]));
#pragma unroll
        for (int q = 1; q < PX - 1; ++q) acc[q] = mm<MAX>(acc[q], mm<MAX>(core, mm<MAX>(left[q], right[q - 1])));
        acc[PX - 1] = mm<MAX>(acc[PX - 1], mm<MAX>(core, right[PX - 2]));
    } else {
#pragma unroll
        for (int q = 0; q < PX; ++q)
            for (int j = 0; j < L; ++j) acc[q] = mm<MAX>(acc[q], p[q + j]);
    }
}

// the same for a span length known at compile time: every byte read has an immediate offset and the scans are straight-line code. The
// element rows of k <= 8 have L <= 9; the uniform switch below picks the instantiation (the run-time-L form above made the compiler build
// a nest of short loops and branches around every read).
template <int PX, bool MAX, int L>
__device__ __forceinline__ void row_span_fixed(const uint8_t* __restrict__ p, unsigned (&acc)[PX]) {
    unsigned b[L + PX - 1];
#pragma unroll
    for (int j = 0; j < L + PX - 1; ++j) b[j] = p[j];
    if constexpr (L >= PX - 1) {
        unsigned core = MAX ? 0u : 255u;
#pragma unroll
        for (int j = PX - 1; j < L; ++j) core = mm<MAX>(core, b[j]);
#pragma unroll
        for (int q = PX - 3; q >= 0; --q) b[q] = mm<MAX>(b[q], b[q + 1]);                      // suffix scan of the left edge b[0 .. PX-2]
#pragma unroll
        for (int q = 1; q < PX - 1; ++q) b[L + q] = mm<MAX>(b[L + q], b[L + q - 1]);           // prefix scan of the right edge b[L .. L+PX-2]
        acc[0] = mm<MAX>(acc[0], mm<MAX>(core, b[0]));
#pragma unroll
        for (int q = 1; q < PX - 1; ++q) acc[q] = mm<MAX>(acc[q], mm<MAX>(core, mm<MAX>(b[q], b[L + q - 1])));
        acc[PX - 1] = mm<MAX>(acc[PX - 1], mm<MAX>(core, b[L + PX - 2]));
    } else {
#pragma unroll
        for (int q = 0; q < PX; ++q)
#pragma unroll
            for (int j = 0; j < L; ++j) acc[q] = mm<MAX>(acc[q], b[q + j]);
    }
}

template <int PX, bool MAX>
__device__ __forceinline__ void row_span_any(const uint8_t* __restrict__ p, int L, unsigned (&acc)[PX]) {
    if constexpr (PX == 4) {
        switch (L) {
            case 1: row_span_fixed<PX, MAX, 1>(p, acc); return;
            case 2: row_span_fixed<PX, MAX, 2>(p, acc); return;
            case 3: row_span_fixed<PX, MAX, 3>(p, acc); return;
            case 4: row_span_fixed<PX, MAX, 4>(p, acc); return;
            case 5: row_span_fixed<PX, MAX, 5>(p, acc); return;
            case 6: row_span_fixed<PX, MAX, 6>(p, acc); return;
            case 7: row_span_fixed<PX, MAX, 7>(p, acc); return;
            case 8: row_span_fixed<PX, MAX, 8>(p, acc); return;
            case 9: row_span_fixed<PX, MAX, 9>(p, acc); return;
            default: break;
        }
    }
    row_span<PX, MAX>(p, L, acc);
}

// all n passes; returns with the final images in buffer (n & 1). oy / ox: image coordinates of LDS cell (0, 0). `span`: lane i of every wave
// holds the span of element row i as lo | hi << 8 (two signed bytes), so a row's span is one v_readlane away -- no memory access in the loop.
template <int PX, bool COLUMN_LANES, bool DO_D, bool DO_E>
__device__ __forceinline__ void run_passes(uint8_t* dbuf, uint8_t* ebuf, int buf_bytes, int S, int k, int n, int Rr, int Rc, int oy, int ox,
                                           int H, int W, int span) {
    const int a = k / 2, b = k - 1 - a;
    for (int p = 1; p <= n; ++p) {
        const int so = (p & 1) ? 0 : buf_bytes, dofs = (p & 1) ? buf_bytes : 0;
        const int r0 = p * a, r1 = Rr - p * b, c0 = p * a, c1 = Rc - p * b;
        const int nr = r1 - r0, G = (c1 - c0 + PX - 1) / PX;
        // item -> (row, group), lanes along a row (or along a column); advanced by NT items per trip without a division
        const int inner = COLUMN_LANES ? nr : G;
        const int step_hi = NT / inner, step_lo = NT - step_hi * inner;
        int hi_i = threadIdx.x / inner, lo_i = threadIdx.x - hi_i * inner;
        for (int it = threadIdx.x; it < nr * G; it += NT) {
            const int rr = COLUMN_LANES ? lo_i : hi_i, g = COLUMN_LANES ? hi_i : lo_i;
            lo_i += step_lo; hi_i += step_hi;
            if (lo_i >= inner) { lo_i -= inner; ++hi_i; }
            const int r = r0 + rr, c = c0 + g * PX;
            unsigned ad[PX], ae[PX];
#pragma unroll
            for (int q = 0; q < PX; ++q) { ad[q] = 0u; ae[q] = 255u; }
            for (int i = 0; i < k; ++i) {
                const int sp = __builtin_amdgcn_readlane(span, i);
                const int lo = (int)(int8_t)(sp & 0xff), hi = (int)(int8_t)((sp >> 8) & 0xff);
                if (lo > hi) continue;
                const int o = so + (r + i - a) * S + c + lo;
                if (DO_D) row_span_any<PX, true>(dbuf + o, hi - lo + 1, ad);
                if (DO_E) row_span_any<PX, false>(ebuf + o, hi - lo + 1, ae);
            }
            const int y = oy + r;
            const bool yin = y >= 0 && y < H;
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                if (c + q < c1) {
                    const int x = ox + c + q;
                    const bool inside = yin && x >= 0 && x < W;
                    if (DO_D) dbuf[dofs + r * S + c + q] = (uint8_t)(inside ? ad[q] : 0u);
                    if (DO_E) ebuf[dofs + r * S + c + q] = (uint8_t)(inside ? ae[q] : 255u);
                }
            }
        }
        __syncthreads();
    }
}

template <bool DO_D, bool DO_E>
__device__ __forceinline__ void run_all(uint8_t* dbuf, uint8_t* ebuf, int buf_bytes, int S, int k, int n, int Rr, int Rc, int oy, int ox, int H,
                                        int W, int span) {
    if (k <= 8) run_passes<4, false, DO_D, DO_E>(dbuf, ebuf, buf_bytes, S, k, n, Rr, Rc, oy, ox, H, W, span);
    else        run_passes<8, true, DO_D, DO_E>(dbuf, ebuf, buf_bytes, S, k, n, Rr, Rc, oy, ox, H, W, span);
}

__global__ __launch_bounds__(NT) void morph_tile_kernel(MorphArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tiles = A.tiles_x * A.tiles_y;
    const long blk = blockIdx.x;
    const int tile = (int)(blk % tiles);
    const long oplane = blk / tiles;                      // output plane: frame * n_out + j
    const int frame = (int)(oplane / A.n_out), j = (int)(oplane - (long)frame * A.n_out);
    const int ty0 = (tile / A.tiles_x) * TH, tx0 = (tile % A.tiles_x) * TW;
    const int H = A.H, W = A.W;
    const long HW = (long)H * W;
    const int th = min(TH, H - ty0), tw = min(TW, W - tx0);

    // which input plane this block shows
    int src = j;
    if (A.op == OUT_TRANSITION || A.op == OUT_TRIMAP) {
        if (A.src_of_slot) src = A.src_of_slot[oplane];
        if (src < 0 || src >= A.n_in) {                   // empty slot: zeros
            float* o = A.out + oplane * HW;
            for (int i = threadIdx.x; i < th * tw; i += NT) o[(long)(ty0 + i / tw) * W + tx0 + i % tw] = 0.f;
            return;
        }
    }
    if (A.op == OUT_DIFF && frame == 0) {                 // vim.py:182: the first frame is all ones, in every slot
        for (int s = 0; s < A.n_slots; ++s) {
            float* o = A.out + (long)s * HW;
            for (int i = threadIdx.x; i < th * tw; i += NT) o[(long)(ty0 + i / tw) * W + tx0 + i % tw] = 1.f;
        }
        return;
    }

    // this frame's element and pass count, inside the caller's bound
    int k = A.kn[2 * frame], n = A.kn[2 * frame + 1];
    k = min(max(k, 1), min(MAXK - 1, A.halo_max + 1));
    n = max(n, 1);
    n = k > 1 ? min(n, max(A.halo_max / (k - 1), 1)) : 1;      // k == 1 is the identity, however often
    const int a = k / 2, b = k - 1 - a;
    const int U = n * a, D = n * b;                       // (kept when the passes are skipped below: the tile sits at (U, U) of the buffers)
    const int Rr = TH + U + D, Rc = TW + U + D, S = A.stride;
    const int oy = ty0 - U, ox = tx0 - U;
    const bool do_d = A.op != OUT_RAW || A.dil != nullptr;
    const bool do_e = A.op == OUT_RAW ? A.ero != nullptr : A.op != OUT_DIFF;
    uint8_t* dbuf = lds;
    uint8_t* ebuf = lds + 2 * A.buf_bytes;

    // ---- load: one read of the input per cell, the `< thresh -> 0` rule and (video) the frame difference folded in. The block also learns the
    // range of what it loaded: when every in-image cell of the tile and its halo holds ONE value, every pass returns that value (the element
    // contains its anchor, absent pixels take no part), so the passes are skipped -- most tiles of a matte are plain background or interior.
    __shared__ int s_range[2];
    if (threadIdx.x == 0) { s_range[0] = 255; s_range[1] = 0; }
    __syncthreads();
    int vmin = 255, vmax = 0;
    const int thr = A.thresh;
    if (A.op == OUT_DIFF) {
        const uint8_t* cur = A.in + (long)frame * A.n_in * HW;
        const uint8_t* prv = cur - (long)A.n_in * HW;
        for (int i = threadIdx.x; i < Rr * Rc; i += NT) {
            const int r = i / Rc, c = i - r * Rc, y = oy + r, x = ox + c;
            unsigned v = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const long at = (long)y * W + x;
                for (int q = 0; q < A.n_in; ++q) {
                    int u1 = cur[q * HW + at], u0 = prv[q * HW + at];
                    u1 = u1 < thr ? 0 : u1; u0 = u0 < thr ? 0 : u0;
                    if (abs(u1 - u0) > A.diff_thresh) v = 255u;
                }
            }
            dbuf[r * S + c] = (uint8_t)v;
            if (y >= 0 && y < H && x >= 0 && x < W) { vmin = min(vmin, (int)v); vmax = max(vmax, (int)v); }
        }
    } else {
        const uint8_t* plane = A.in + ((long)frame * A.n_in + src) * HW;
        for (int i = threadIdx.x; i < Rr * Rc; i += NT) {
            const int r = i / Rc, c = i - r * Rc, y = oy + r, x = ox + c;
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
            int v = inside ? plane[(long)y * W + x] : 0;
            v = v < thr ? 0 : v;
            if (do_d) dbuf[r * S + c] = (uint8_t)v;
            if (do_e) ebuf[r * S + c] = (uint8_t)(inside ? v : 255);
            if (inside) { vmin = min(vmin, v); vmax = max(vmax, v); }
        }
    }
    if (vmin <= vmax) { atomicMin(&s_range[0], vmin); atomicMax(&s_range[1], vmax); }      // integer LDS atomics: the result does not depend on order
    __syncthreads();
    if (s_range[0] == s_range[1]) n = 0;                  // the loaded images are already the final ones (buffer 0)

    const int row = threadIdx.x & 63;                     // lane i: the span of element row i (rows >= k: empty)
    const int span = row < k ? ((int)(uint8_t)c_se.lo[k][row] | ((int)(uint8_t)c_se.hi[k][row] << 8)) : 0x0001;
    if (do_d && do_e) run_all<true, true>(dbuf, ebuf, A.buf_bytes, S, k, n, Rr, Rc, oy, ox, H, W, span);
    else if (do_d)    run_all<true, false>(dbuf, ebuf, A.buf_bytes, S, k, n, Rr, Rc, oy, ox, H, W, span);
    else              run_all<false, true>(dbuf, ebuf, A.buf_bytes, S, k, n, Rr, Rc, oy, ox, H, W, span);

    // ---- epilogue: the final images are in buffer (n & 1); one write per output pixel
    const uint8_t* fd = dbuf + ((n & 1) ? A.buf_bytes : 0);
    const uint8_t* fe = ebuf + ((n & 1) ? A.buf_bytes : 0);
    for (int i = threadIdx.x; i < th * tw; i += NT) {
        const int ry = i / tw, rx = i - ry * tw;
        const int cell = (U + ry) * S + U + rx;
        const long at = (long)(ty0 + ry) * W + tx0 + rx;
        if (A.op == OUT_RAW) {
            if (do_d) A.dil[oplane * HW + at] = fd[cell];
            if (do_e) A.ero[oplane * HW + at] = fe[cell];
        } else if (A.op == OUT_TRANSITION) {
            A.out[oplane * HW + at] = fd[cell] > fe[cell] ? 1.f : 0.f;
        } else if (A.op == OUT_TRIMAP) {
            int v = A.in[((long)frame * A.n_in + src) * HW + at];          // the centre value again: an L2 hit, the tile has just been read
            v = v < thr ? 0 : v;
            A.out[oplane * HW + at] = fd[cell] > fe[cell] ? 1.f : (v >= 128 ? 2.f : 0.f);
        } else {
            const float v = fd[cell] > 0 ? 1.f : 0.f;
            float* o = A.out + (long)frame * A.n_slots * HW + at;
            for (int s = 0; s < A.n_slots; ++s) o[(long)s * HW] = v;
        }
    }
}

int launch(MorphArgs& A, long out_planes, bool two_images, void* stream) {
    if (A.halo_max < 0 || A.halo_max > MG_MORPH_MAX_HALO) return -2;
    if (A.H <= 0 || A.W <= 0 || out_planes <= 0) return 0;
    const int rc = ensure_se_table();
    if (rc) return rc;
    A.tiles_x = (A.W + TW - 1) / TW;
    A.tiles_y = (A.H + TH - 1) / TH;
    const long blocks = out_planes * A.tiles_x * A.tiles_y;
    if (blocks > 0x7fffffffL) return -3;
    A.stride = lds_stride(A.halo_max);
    A.buf_bytes = (TH + A.halo_max) * A.stride;
    const size_t lds_bytes = (size_t)A.buf_bytes * (two_images ? 4 : 2);       // at most 4 * 112 * 124 = 55552 bytes
    hipLaunchKernelGGL(morph_tile_kernel, dim3((unsigned)blocks), dim3(NT), lds_bytes, (hipStream_t)stream, A);
    MG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int mg_morph_prepare(void) { return ensure_se_table(); }

extern "C" int mg_morph_u8(const uint8_t* in, uint8_t* dil, uint8_t* ero, const int32_t* kn, int halo_max, long planes, int planes_per_frame,
                           int H, int W, void* stream) {
    if (planes_per_frame <= 0 || !kn) return -2;
    if (!dil && !ero) return 0;
    MorphArgs A = {};
    A.in = in; A.dil = dil; A.ero = ero; A.kn = kn;
    A.op = OUT_RAW; A.halo_max = halo_max; A.n_in = planes_per_frame; A.n_out = planes_per_frame; A.n_slots = planes_per_frame;
    A.H = H; A.W = W;
    return launch(A, planes, true, stream);
}

extern "C" int mg_transition_gt(const uint8_t* in, float* out, const int32_t* src_of_slot, const int32_t* kn, int halo_max, int frames, int n_in,
                                int n_slots, int H, int W, int thresh, int mode, void* stream) {
    if ((mode != MG_GT_TRANSITION && mode != MG_GT_TRIMAP) || !kn) return -2;
    if (frames <= 0 || n_slots <= 0) return 0;
    if (n_in <= 0 || (!src_of_slot && n_slots != n_in)) return -2;
    MorphArgs A = {};
    A.in = in; A.out = out; A.kn = kn; A.src_of_slot = src_of_slot;
    A.op = mode == MG_GT_TRIMAP ? OUT_TRIMAP : OUT_TRANSITION;
    A.halo_max = halo_max; A.n_in = n_in; A.n_out = n_slots; A.n_slots = n_slots; A.H = H; A.W = W; A.thresh = thresh;
    return launch(A, (long)frames * n_slots, true, stream);
}

extern "C" int mg_diff_transition(const uint8_t* in, float* out, const int32_t* kn, int halo_max, int T, int n_in, int n_slots, int H, int W,
                                  int thresh, int diff_thresh, void* stream) {
    if (!kn) return -2;
    if (T <= 0 || n_slots <= 0) return 0;
    if (n_in <= 0) return -2;
    MorphArgs A = {};
    A.in = in; A.out = out; A.kn = kn;
    A.op = OUT_DIFF; A.halo_max = halo_max; A.n_in = n_in; A.n_out = 1; A.n_slots = n_slots; A.H = H; A.W = W;
    A.thresh = thresh; A.diff_thresh = diff_thresh;
    return launch(A, T, false, stream);
}
