// maggie_amd/csrc/jpegprog.hip compiled for the host: the kernel source itself, one thread per lane of the wave, a barrier for __syncthreads, the
// ballot through a shared array, the workgroups (chains) of a launch one after the other. Built with -fsanitize=address,undefined -pthread by
// tests/test_jpegprog_cpu.py and run on buffers of exactly the sizes the entry point is told, so that an access outside them stops the program.
// Not a GPU program: nothing here is launched.
//
//   jpegprog_host IN OUT    IN: int32 ncases, then per case int32 {h, w, layout, frames, nscans, nchains, blob_bytes},
//                           int32 scans[nscans][480], int32 chains[nchains][4], blob.
//                           OUT: per case int32 {rc, n_coef}, int32 info[frames], int16 coef[n_coef].
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
typedef void* hipStream_t;
using std::max;
using std::min;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int LANES = MG_JPEGPROG_THREADS;
static pthread_barrier_t g_start, g_done, g_block;
static std::function<void()> g_body;
static int g_blocks;
static bool g_quit = false;
static int g_x[LANES];

static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long jp_ballot(int p) {                  // every lane of the wave calls it together
    const int l = (int)threadIdx.x;
    g_x[l] = p != 0;
    __syncthreads();
    unsigned long long r = 0;
    for (int i = 0; i < LANES; ++i) r |= (unsigned long long)g_x[i] << i;
    __syncthreads();
    return r;
}

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

#include "../../maggie_amd/csrc/jpegprog.hip"

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
    if (argc != 3) { fprintf(stderr, "usage: jpegprog_host IN OUT\n"); return 2; }
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
        int32_t hd[7];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1], layout = hd[2];
        const long frames = hd[3], nscans = hd[4], nchains = hd[5], nbytes = hd[6];
        Exact<int32_t> scans((size_t)nscans * MG_JPEGPROG_SCAN_WORDS), chains((size_t)nchains * MG_JPEGPROG_CHAIN_WORDS);
        Exact<uint8_t> blob((size_t)nbytes);
        if (!rd(in, scans.p, scans.n * 4) || !rd(in, chains.p, chains.n * 4) || !rd(in, blob.p, blob.n)) { rc_main = 2; break; }
        const int side = layout == MG_JPEGDEC_420 ? 16 : 8, bpm = layout == MG_JPEGDEC_420 ? 6 : (layout == MG_JPEGDEC_444 ? 3 : 1);
        const long nbf = (long)((w + side - 1) / side) * ((h + side - 1) / side) * bpm;
        Exact<int16_t> coef((size_t)(frames * nbf * 64), true);
        Exact<int32_t> info((size_t)frames, true);
        const int rc = mg_jpegprog_chains(blob.p, nbytes, scans.p, nscans, chains.p, nchains, coef.p, (long)coef.n, info.p, frames, h, w, layout, nullptr);
        const int32_t res[2] = {rc, (int32_t)coef.n};
        fwrite(res, 4, 2, out);
        fwrite(info.p, 4, info.n, out);
        fwrite(coef.p, 2, coef.n, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("jpegprog_host: ok\n");
    return rc_main;
}
