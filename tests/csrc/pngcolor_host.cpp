// maggie_amd/csrc/pngcolor.hip (and the csrc/png_inflate.h it shares with pngdec.hip) compiled for the host: the kernel source itself, one thread
// per lane of the wave, a barrier for __syncthreads, the cross-lane moves through a shared array, the workgroups of a launch one after the
// other. Built with -fsanitize=address,undefined -pthread by tests/test_pngcolor_cpu.py and run on buffers of exactly the sizes the entry
// points are told, so that an access outside them stops the program. Not a GPU program: nothing here is launched.
//
//   pngcolor_host IN OUT  IN: int32 ncases, then per case int32 {h, w, files, blob_bytes, mode, raw_stride}, int32 recs[files][292], blob.
//                         OUT: per case int32 {rc_inflate, rc_unfilter, rc_convert, n_out_bytes}, int32 info[files][8],
//                         uint8 raw[files][raw_stride], the output bytes (the host sequence of maggie_amd/utils/pngcolor.py `run`).
#define MG_HOST_EMU 1
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/maggie_hip.h"

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define MG_DEVCONST static const
#define MG_CHECK_LAUNCH() do { } while (0)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int LANES = MG_PNGDEC_THREADS;
static pthread_barrier_t g_start, g_done, g_block;
static std::function<void()> g_body;
static bool g_quit = false;
static int g_x[LANES];
static unsigned long long g_y[LANES];

static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
// csrc/pixel_norm.h: (v / 255 - mean) / std with IEEE divisions
static inline float mg_norm_u8(int v, float mean, float std) { return ((float)v / 255.0f - mean) / std; }

namespace {
// the four cross-lane moves of png_inflate.h: every lane of the wave calls them together
inline int pd_shift_up(int v) {
    const int l = (int)threadIdx.x;
    g_x[l] = v;
    __syncthreads();
    const int r = l ? g_x[l - 1] : v;
    __syncthreads();
    return r;
}
inline int pd_scan(int v) {
    const int l = (int)threadIdx.x;
    g_x[l] = v;
    __syncthreads();
    int r = 0;
    for (int i = 0; i <= l; ++i) r += g_x[i];
    __syncthreads();
    return r;
}
inline unsigned long long pd_ballot(int p) {
    const int l = (int)threadIdx.x;
    g_x[l] = p != 0;
    __syncthreads();
    unsigned long long r = 0;
    for (int i = 0; i < LANES; ++i) r |= (unsigned long long)g_x[i] << i;
    __syncthreads();
    return r;
}
inline unsigned long long pd_sum(unsigned long long v) {
    const int l = (int)threadIdx.x;
    g_y[l] = v;
    __syncthreads();
    unsigned long long r = 0;
    for (int i = 0; i < LANES; ++i) r += g_y[i];
    __syncthreads();
    return r;
}
}  // namespace

static void worker(int tid) {
    for (;;) {
        pthread_barrier_wait(&g_start);
        if (g_quit) return;
        for (unsigned by = 0; by < gridDim.y; ++by)
            for (unsigned bx = 0; bx < gridDim.x; ++bx) {
                threadIdx.x = (unsigned)tid; blockIdx.x = bx; blockIdx.y = by;
                g_body();
                pthread_barrier_wait(&g_block);                         // the next workgroup reuses the `__shared__` storage
            }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(dim3 grid, dim3 block, std::function<void()> body) {
    if (block.x != (unsigned)LANES || block.y != 1) { fprintf(stderr, "emu: workgroup of %u lanes\n", block.x); exit(3); }
    g_body = body;
    blockDim = block; gridDim = grid;
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g), (b), [=]() { k(__VA_ARGS__); })

#include "../../maggie_amd/csrc/pngcolor.hip"

template <typename T> struct Exact {                                // an allocation of exactly n elements, 16-byte aligned, filled with 0xA5 (or zero)
    T* p; size_t n;
    explicit Exact(size_t n_, bool zero = false) : p(nullptr), n(n_) {
        const size_t bytes = n_ ? n_ * sizeof(T) : 1;
        if (posix_memalign((void**)&p, 16, bytes)) exit(3);
        memset(p, zero ? 0 : 0xA5, bytes);
    }
    ~Exact() { free(p); }
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: pngcolor_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, LANES + 1);
    pthread_barrier_init(&g_done, nullptr, LANES + 1);
    pthread_barrier_init(&g_block, nullptr, LANES);
    std::vector<std::thread> pool;
    for (int t = 0; t < LANES; ++t) pool.emplace_back(worker, t);
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[6];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1], mode = hd[4];
        const long F = hd[2], nbytes = hd[3], stride = hd[5];
        Exact<int32_t> recs((size_t)F * MG_PNGCOLOR_REC_WORDS);
        Exact<uint8_t> blob((size_t)nbytes);
        if (!rd(in, recs.p, recs.n * 4) || !rd(in, blob.p, blob.n)) { rc_main = 2; break; }
        const size_t per = (size_t)h * w * (mode == MG_PNGCOLOR_OUT_L ? 1 : (mode == MG_PNGCOLOR_OUT_RGB ? 3 : 12));
        Exact<uint8_t> raw((size_t)(F * stride)), dst((size_t)F * per);
        Exact<int32_t> info((size_t)F * MG_PNGDEC_INFO_WORDS, true);
        const int rc1 = mg_pngcolor_inflate(blob.p, nbytes, recs.p, raw.p, stride, info.p, F, h, w, nullptr);
        const int rc2 = rc1 ? 0 : mg_pngcolor_unfilter(raw.p, stride, recs.p, info.p, F, h, w, nullptr);
        const int rc3 = rc1 || rc2 ? 0 : mg_pngcolor_convert(raw.p, stride, recs.p, dst.p, info.p, F, h, w, mode, mean, sd, nullptr);
        const int32_t res[4] = {rc1, rc2, rc3, (int32_t)dst.n};
        fwrite(res, 4, 4, out);
        fwrite(info.p, 4, info.n, out);
        fwrite(raw.p, 1, raw.n, out);
        fwrite(dst.p, 1, dst.n, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("pngcolor_host: ok\n");
    return rc_main;
}
