// The decode path of maggie_amd/utils/jpegsamp.py compiled for the host: maggie_amd/csrc/jpegdec.hip, jpegprog.hip and photometric.hip, the
// kernel sources themselves, one thread per GPU thread, a barrier for __syncthreads, the ballot through a shared array, the workgroups of a
// launch one after the other. Built with -fsanitize=address,undefined -pthread by tests/test_jpegsamp_cpu.py and run on buffers of exactly the
// sizes the entry points are told, so that an access outside them, or a wide load or store off its alignment, stops the program.
// Not a GPU program: nothing here is launched.
//
//   jpegsamp_host IN OUT   IN: int32 ncases, then per case int32 {kind (0 baseline, 1 progressive), h, w, layout (MG_JPEGDEC_422 / _440 / _411), 0,
//                          sub_bytes, frames, nscans, nchains, blob_bytes}, int32 recs[frames][1120] (jpegdec's records; a progressive case reads the quantisation tables
//                          from them), progressive: int32 scans[nscans][480], int32 chains[nchains][4]; then the blob.
//                          OUT: per case int32 {rc, status, n_coef, n_planes, n_rgb}, int16 coef, uint8 planes, uint8 rgb (raw epilogue),
//                          float norm[n_rgb] (the ToTensor + Normalize epilogue): the host loops of jpegdec.py / jpegprog.py `run`.
#define MG_HOST_EMU 1
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
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
// the vector types with the alignment the device asks of a load or store of their size
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { uint2 v; v.x = a; v.y = b; return v; }
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { uint4 v; v.x = a; v.y = b; v.z = c; v.w = d; return v; }
static inline float4 make_float4(float a, float b, float c, float d) { float4 v; v.x = a; v.y = b; v.z = c; v.w = d; return v; }
typedef void* hipStream_t;
using std::max;
using std::min;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int POOL = 256;
static pthread_barrier_t g_start, g_done, g_block[3];              // workgroups of 64, 128 and 256 lanes
static std::function<void()> g_body;
static int g_threads, g_blocks;
static std::atomic<int> g_or{0};
static bool g_quit = false;
static int g_x[64];

static inline pthread_barrier_t* block_barrier() { return &g_block[g_threads == 64 ? 0 : (g_threads == 128 ? 1 : 2)]; }
static inline void __syncthreads() { pthread_barrier_wait(block_barrier()); }
static inline int __syncthreads_or(int p) {
    if (p) g_or.store(1);
    __syncthreads();
    const int r = g_or.load();
    __syncthreads();
    if (threadIdx.x == 0) g_or.store(0);
    __syncthreads();
    return r;
}
static inline unsigned long long jp_ballot(int p) {                  // every lane of the 64-lane workgroup calls it together
    g_x[threadIdx.x] = p != 0;
    __syncthreads();
    unsigned long long r = 0;
    for (int i = 0; i < 64; ++i) r |= (unsigned long long)g_x[i] << i;
    __syncthreads();
    return r;
}
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int atomicMax(int32_t* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
// pixel_norm.h's ToTensor + Normalize.norm (IEEE divisions)
static inline float mg_norm_u8(int v, float mean, float std) { return ((float)v / 255.0f - mean) / std; }

static void worker(int tid) {
    for (;;) {
        pthread_barrier_wait(&g_start);
        if (g_quit) return;
        if (tid < g_threads)
            for (int b = 0; b < g_blocks; ++b) {
                threadIdx.x = (unsigned)tid; blockIdx.x = (unsigned)b;
                g_body();
                pthread_barrier_wait(block_barrier());              // the next workgroup reuses the `__shared__` storage
            }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(unsigned blocks, unsigned threads, std::function<void()> body) {
    if (threads != 64 && threads != 128 && threads != POOL) { fprintf(stderr, "emu: workgroup of %u lanes\n", threads); exit(3); }
    g_body = body; g_threads = (int)threads; g_blocks = (int)blocks;
    blockDim = dim3(threads); gridDim = dim3(blocks);
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g).x, (b).x, [=]() { k(__VA_ARGS__); })

// each source keeps its helpers in an unnamed namespace; a namespace of its own around each keeps the three sets apart in one program (the
// extern "C" entry points are the ones include/maggie_hip.h declares, wherever they are defined)
namespace jd {
#include "../../maggie_amd/csrc/jpegdec.hip"
}
namespace jp {
#include "../../maggie_amd/csrc/jpegprog.hip"
}
namespace ph {
#include "../../maggie_amd/csrc/photometric.hip"
}

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
    if (argc != 3) { fprintf(stderr, "usage: jpegsamp_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, POOL + 1);
    pthread_barrier_init(&g_done, nullptr, POOL + 1);
    pthread_barrier_init(&g_block[0], nullptr, 64);
    pthread_barrier_init(&g_block[1], nullptr, 128);
    pthread_barrier_init(&g_block[2], nullptr, POOL);
    std::vector<std::thread> pool;
    for (int t = 0; t < POOL; ++t) pool.emplace_back(worker, t);
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[10];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int kind = hd[0], h = hd[1], w = hd[2], layout = hd[3], S = hd[5];
        if (layout < MG_JPEGDEC_422 || layout > MG_JPEGDEC_411) { rc_main = 2; break; }
        const int hs = layout == MG_JPEGDEC_422 ? 2 : (layout == MG_JPEGDEC_411 ? 4 : 1), vs = layout == MG_JPEGDEC_440 ? 2 : 1;
        const long T = hd[6], nscans = hd[7], nchains = hd[8], nbytes = hd[9];
        Exact<int32_t> recs((size_t)T * MG_JPEGDEC_TAB_WORDS), scans((size_t)nscans * MG_JPEGPROG_SCAN_WORDS);
        Exact<int32_t> chains((size_t)nchains * MG_JPEGPROG_CHAIN_WORDS);
        Exact<uint8_t> blob((size_t)nbytes);
        if (!rd(in, recs.p, recs.n * 4) || !rd(in, scans.p, scans.n * 4) || !rd(in, chains.p, chains.n * 4) || !rd(in, blob.p, blob.n)) {
            rc_main = 2;
            break;
        }
        // the geometry of include/maggie_hip.h, said once more
        const long mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs), nbf = mcux * mcuy * (hs * vs + 2);
        const long yp = (mcux * 8 * hs + 15) / 16 * 16, cp = vs == 2 ? (mcux * 8 + 15) / 16 * 16 : mcux * 8, pb = T * mcuy * 8 * (vs * yp + 2 * cp);
        Exact<int16_t> coef((size_t)(T * nbf * 64), true);
        Exact<uint8_t> planes((size_t)pb), rgb((size_t)T * h * w * 3);
        Exact<float> norm((size_t)T * h * w * 3);
        const float mean[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
        int rc = 0, status = 0;
        auto finish = [&]() {
            int r = mg_jpegdec_idct(coef.p, (long)coef.n, recs.p, planes.p, pb, T, h, w, layout, nullptr);
            if (!r) r = mg_jpeg_rgb_hv(planes.p, pb, rgb.p, T, h, w, hs, vs, MG_PHOTO_RAW, mean, std3, nullptr);
            if (!r) r = mg_jpeg_rgb_hv(planes.p, pb, norm.p, T, h, w, hs, vs, MG_PHOTO_NORM, mean, std3, nullptr);
            return r;
        };
        if (kind == 0) {
            long longest = 0;
            for (long t = 0; t < T; ++t) longest = std::max<long>(longest, recs.p[t * MG_JPEGDEC_TAB_WORDS + 919]);
            const int nsub = (int)std::max<long>(1, (longest + S - 1) / S), wgs = (nsub + MG_JPEGDEC_THREADS - 1) / MG_JPEGDEC_THREADS;
            const int max_launches = wgs + 1, info_words = 4 + 2 * (max_launches + 1);
            Exact<unsigned long long> exits((size_t)T * nsub), entries((size_t)T * wgs), bounds((size_t)2 * T * wgs, true);
            Exact<int32_t> counts((size_t)T * nsub), first((size_t)T * nsub), info((size_t)info_words, true);
            int k = 0;
            auto sync = [&](int launch) {
                return mg_jpegdec_sync(blob.p, nbytes, recs.p, exits.p, counts.p, entries.p, bounds.p, info.p, info_words, T, nsub, S, layout, launch,
                                       nullptr);
            };
            auto output = [&]() {
                int r = mg_jpegdec_coef(blob.p, nbytes, recs.p, exits.p, counts.p, first.p, coef.p, (long)coef.n, info.p, T, nsub, S, h, w, layout,
                                        nullptr);
                if (!r) r = mg_jpegdec_dcsum(coef.p, (long)coef.n, recs.p, T, h, w, layout, nullptr);
                return r ? r : finish();
            };
            rc = sync(0);
            if (!rc && wgs > 1) { k = 1; rc = sync(1); }
            if (!rc) rc = output();
            bool again = false;
            while (!rc && k >= 1 && info.p[2 + 2 * k] != 0) {
                if (k >= max_launches) { rc = -100; break; }
                k += 1;
                rc = sync(k);
                again = true;
            }
            if (!rc && again) {
                memset(coef.p, 0, coef.n * 2);
                info.p[0] = 0;
                rc = output();
            }
            status = info.p[0];
        } else {
            Exact<int32_t> info((size_t)T, true);
            rc = mg_jpegprog_chains(blob.p, nbytes, scans.p, nscans, chains.p, nchains, coef.p, (long)coef.n, info.p, T, h, w, layout, nullptr);
            if (!rc) rc = finish();
            for (long t = 0; t < T; ++t) status |= info.p[t];
        }
        const int32_t res[5] = {rc, status, (int32_t)coef.n, (int32_t)planes.n, (int32_t)rgb.n};
        fwrite(res, 4, 5, out);
        fwrite(coef.p, 2, coef.n, out);
        fwrite(planes.p, 1, planes.n, out);
        fwrite(rgb.p, 1, rgb.n, out);
        fwrite(norm.p, 4, norm.n, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("jpegsamp_host: ok\n");
    return rc_main;
}
