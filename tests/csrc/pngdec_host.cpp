// maggie_amd/csrc/pngdec.hip compiled for the host: the kernel source itself, one thread per lane of the wave, a barrier for __syncthreads, the
// cross-lane moves through a shared array, the workgroups of a launch one after the other. Built with -fsanitize=address,undefined -pthread
// by tests/test_pngdec_cpu.py and run on buffers of exactly the sizes the entry points are told, so that an access outside them stops the
// program. Not a GPU program: nothing here is launched.
//
//   pngdec_host IN OUT    IN: int32 ncases, then per case int32 {h, w, planes, blob_bytes}, int32 recs[planes][72], blob.
//                         OUT: per case int32 {rc_inflate, rc_unfilter, raw_stride, n_out}, int32 info[planes][8], uint8 raw[planes][raw_stride],
//                         uint8 out[planes][h][w] (the host sequence of maggie_amd/utils/pngdec.py `run`).
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
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int LANES = MG_PNGDEC_THREADS;
static pthread_barrier_t g_start, g_done, g_block;
static std::function<void()> g_body;
static int g_blocks;
static bool g_quit = false;
static int g_x[LANES];
static unsigned long long g_y[LANES];

static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }

namespace {
// the four cross-lane moves of pngdec.hip: every lane of the wave calls them together
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
        for (int b = 0; b < g_blocks; ++b) {
            threadIdx.x = (unsigned)tid; blockIdx.x = (unsigned)b;
            g_body();
            pthread_barrier_wait(&g_block);                             // the next workgroup reuses the `__shared__` storage
        }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(unsigned blocks, unsigned threads, std::function<void()> body) {
    if (threads != (unsigned)LANES) { fprintf(stderr, "emu: workgroup of %u lanes\n", threads); exit(3); }
    g_body = body; g_blocks = (int)blocks;
    blockDim = dim3(threads); gridDim = dim3(blocks);
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g).x, (b).x, [=]() { k(__VA_ARGS__); })

#include "../../maggie_amd/csrc/pngdec.hip"

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
    if (argc != 3) { fprintf(stderr, "usage: pngdec_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, LANES + 1);
    pthread_barrier_init(&g_done, nullptr, LANES + 1);
    pthread_barrier_init(&g_block, nullptr, LANES);
    std::vector<std::thread> pool;
    for (int t = 0; t < LANES; ++t) pool.emplace_back(worker, t);
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[4];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1];
        const long P = hd[2], nbytes = hd[3];
        Exact<int32_t> recs((size_t)P * MG_PNGDEC_REC_WORDS);
        Exact<uint8_t> blob((size_t)nbytes);
        if (!rd(in, recs.p, recs.n * 4) || !rd(in, blob.p, blob.n)) { rc_main = 2; break; }
        long stride = 16;
        for (long p = 0; p < P; ++p) {
            const int ct = recs.p[p * MG_PNGDEC_REC_WORDS + 2], depth = recs.p[p * MG_PNGDEC_REC_WORDS + 3];
            const int ch = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
            const long size = (long)h * (1 + ((long)w * ch * depth + 7) / 8);
            stride = std::max(stride, (size + 15) / 16 * 16);
        }
        Exact<uint8_t> raw((size_t)(P * stride)), plane((size_t)(P * h * w));
        Exact<int32_t> info((size_t)P * MG_PNGDEC_INFO_WORDS, true);
        const int rc1 = mg_pngdec_inflate(blob.p, nbytes, recs.p, raw.p, stride, info.p, P, h, w, nullptr);
        const int rc2 = rc1 ? 0 : mg_pngdec_unfilter(raw.p, stride, recs.p, plane.p, info.p, P, h, w, nullptr);
        const int32_t res[4] = {rc1, rc2, (int32_t)stride, (int32_t)plane.n};
        fwrite(res, 4, 4, out);
        fwrite(info.p, 4, info.n, out);
        fwrite(raw.p, 1, raw.n, out);
        fwrite(plane.p, 1, plane.n, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("pngdec_host: ok\n");
    return rc_main;
}
