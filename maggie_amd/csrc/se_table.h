// OpenCV getStructuringElement(MORPH_ELLIPSE, (k, k)) row spans, relative to the anchor k / 2, as a __constant__ table shared by the
// morphology kernels (region.hip: bit-plane dilation; morph.hip: grey-scale dilation / erosion). Each translation unit that includes this
// header owns its copy of the table (there is no relocatable device code in this build) and fills it on its first call.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <mutex>

namespace {

constexpr int MAXK = 32;

struct SeTable { int8_t lo[MAXK][MAXK]; int8_t hi[MAXK][MAXK]; };   // [k][row]; lo > hi => empty row
__constant__ SeTable c_se;
std::once_flag g_se_once;
int g_se_rc = 0;

void build_se_table(SeTable& t) {
    for (int k = 0; k < MAXK; ++k)
        for (int i = 0; i < MAXK; ++i) { t.lo[k][i] = 1; t.hi[k][i] = 0; }
    for (int k = 1; k < MAXK; ++k) {
        if (k == 1) { t.lo[1][0] = 0; t.hi[1][0] = 0; continue; }
        int r = k / 2, c = k / 2;
        double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
        for (int i = 0; i < k; ++i) {
            int dy = i - r;
            if (abs(dy) <= r) {
                int dx = (int)nearbyint(c * sqrt((r * r - dy * dy) * inv_r2));   // cvRound: round half to even
                int j1 = c - dx < 0 ? 0 : c - dx;
                int j2 = c + dx + 1 > k ? k : c + dx + 1;
                if (j2 > j1) { t.lo[k][i] = (int8_t)(j1 - c); t.hi[k][i] = (int8_t)(j2 - 1 - c); }
            }
        }
    }
}

int ensure_se_table() {
    std::call_once(g_se_once, [] {
        SeTable t;
        build_se_table(t);
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_se), &t, sizeof(t));
        g_se_rc = (int)e;
    });
    return g_se_rc;
}

}  // namespace
