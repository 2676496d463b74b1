// The convolution launch forms by name (host code only): the list of every kernel form conv_halo3.hip, conv_igemm.hip and conv_wgrad.hip
// instantiate, and the thread-local record of the forms the last public conv entry call launched. See conv_forms.h.
#include "conv_forms.h"
#include "../../include/maggie_hip.h"
#include <stdio.h>
#include <vector>

namespace {

constexpr int LAST_CAP = 32;
thread_local uint64_t g_last[LAST_CAP];
thread_local int g_last_n = 0;

struct FamInfo { const char* name; int nargs; };
const FamInfo& fam_info(int fam) {
    static const FamInfo tab[MG_FF_END] = {
        {"?", 0},          {"h3", 3},          {"h3_slab", 0},      {"h3_persist", 3}, {"halo", 3},       {"c8", 1},           {"async", 4},
        {"async_mdev", 4}, {"fprop", 3},       {"fprop_mdev", 3},   {"split", 1},      {"split_finish", 0}, {"wgrad_c8", 0},   {"wgrad_gather9", 1},
        {"wgrad_halo", 0}, {"wgrad", 2},       {"reduce", 0},       {"reduce_wave", 0}, {"reduce_tile", 0}, {"reduce_batched", 0}};
    return tab[fam > 0 && fam < MG_FF_END ? fam : 0];
}

// every form the three files compile, in a fixed order: the position is the form's id
const std::vector<uint64_t>& all_forms() {
    static const std::vector<uint64_t> forms = [] {
        std::vector<uint64_t> v;
        const int C = MG_MODE_CONV, T = MG_MODE_TCONV, G = MG_MODE_GATHER, X = MG_FORM_NOMODE;
        const int RES = MG_FORM_RES, XF = MG_FORM_XF, BNB = MG_FORM_BNB;
        // conv_halo3.hip
#define MG_ROW3(a, b, c) {a, b, c},
        static const int h3[][3] = {MG_H3_TILE_FORMS(MG_ROW3)};
        for (const auto& f : h3) {
            for (int fl : {0, RES, XF, RES | XF}) v.push_back(mg_form_code(MG_FF_H3, f[0], f[1], f[2], 0, C, fl));
            for (int fl : {0, RES, RES | BNB}) v.push_back(mg_form_code(MG_FF_H3, f[0], f[1], f[2], 0, T, fl));
        }
        for (int fl : {0, RES, XF, RES | XF}) v.push_back(mg_form_code(MG_FF_H3_SLAB, 0, 0, 0, 0, C, fl));
        for (int fl : {0, RES}) v.push_back(mg_form_code(MG_FF_H3_SLAB, 0, 0, 0, 0, T, fl));
        static const int h3p[][3] = {MG_H3_PERSIST_FORMS(MG_ROW3)};
#undef MG_ROW3
        for (const auto& f : h3p)
            for (int m : {C, T})
                for (int fl : {0, RES}) v.push_back(mg_form_code(MG_FF_H3_PERSIST, f[0], f[1], f[2], 0, m, fl));
        // conv_igemm.hip
        static const int halo[][3] = {{8, 16, 1}, {4, 16, 1}, {8, 32, 1}, {4, 32, 1}, {8, 64, 1}, {4, 64, 1}, {8, 32, 2}, {8, 64, 3}, {4, 64, 3}};
        for (const auto& f : halo) {
            v.push_back(mg_form_code(MG_FF_HALO, f[0], f[1], f[2], 0, C, 0));
            if (f[2] <= 2 && f[1] >= 32) v.push_back(mg_form_code(MG_FF_HALO, f[0], f[1], f[2], 0, C, XF));
            v.push_back(mg_form_code(MG_FF_HALO, f[0], f[1], f[2], 0, T, 0));
            v.push_back(mg_form_code(MG_FF_HALO, f[0], f[1], f[2], 0, T, BNB));
        }
        for (int th : {8, 16}) v.push_back(mg_form_code(MG_FF_C8, th, 0, 0, 0, X, 0));
        static const int as[][4] = {{128, 128, 2, 3}, {128, 64, 2, 4}, {128, 64, 2, 3}, {64, 64, 2, 4}, {64, 64, 2, 3}};
        for (const auto& f : as) {
            for (int m : {C, T, G}) v.push_back(mg_form_code(MG_FF_ASYNC, f[0], f[1], f[2], f[3], m, 0));
            v.push_back(mg_form_code(MG_FF_ASYNC, f[0], f[1], f[2], f[3], T, BNB));
            for (int m : {C, G}) v.push_back(mg_form_code(MG_FF_ASYNC_MDEV, f[0], f[1], f[2], f[3], m, 0));
        }
        static const int fp[][2] = {{128, 128}, {128, 64}, {64, 64}, {64, 32}, {128, 32}, {128, 16}};
        for (const auto& f : fp)
            for (int ks : {1, 2, 4}) {
                for (int m : {C, T, G}) v.push_back(mg_form_code(MG_FF_FPROP, f[0], f[1], ks, 0, m, 0));
                v.push_back(mg_form_code(MG_FF_FPROP, f[0], f[1], ks, 0, T, MG_FORM_PHASED));
                v.push_back(mg_form_code(MG_FF_FPROP, f[0], f[1], ks, 0, C, BNB));
                v.push_back(mg_form_code(MG_FF_FPROP, f[0], f[1], ks, 0, T, BNB));
                v.push_back(mg_form_code(MG_FF_FPROP, f[0], f[1], ks, 0, T, BNB | MG_FORM_PHASED));
                for (int m : {C, G}) {
                    v.push_back(mg_form_code(MG_FF_FPROP_MDEV, f[0], f[1], ks, 0, m, 0));
                    if (f[0] == 128 && f[1] <= 32 && ks <= 2) v.push_back(mg_form_code(MG_FF_FPROP_MDEV, f[0], f[1], ks, 0, m, XF));
                }
            }
        for (int bn : {64, 128})
            for (int m : {C, T}) v.push_back(mg_form_code(MG_FF_SPLIT, bn, 0, 0, 0, m, 0));
        v.push_back(mg_form_code(MG_FF_SPLIT_FINISH, 0, 0, 0, 0, X, 0));
        // conv_wgrad.hip
        v.push_back(mg_form_code(MG_FF_WGRAD_C8, 0, 0, 0, 0, X, 0));
        v.push_back(mg_form_code(MG_FF_WGRAD_GATHER9, 1, 0, 0, 0, X, 0));
        v.push_back(mg_form_code(MG_FF_WGRAD_GATHER9, 1, 0, 0, 0, X, XF));
        v.push_back(mg_form_code(MG_FF_WGRAD_GATHER9, 2, 0, 0, 0, X, 0));
        v.push_back(mg_form_code(MG_FF_WGRAD_HALO, 0, 0, 0, 0, X, 0));
        v.push_back(mg_form_code(MG_FF_WGRAD_HALO, 0, 0, 0, 0, X, XF));
        static const int wg[][2] = {{32, 32}, {32, 64}, {64, 32}, {64, 64}};
        for (const auto& f : wg) {
            for (int m : {C, T, G}) v.push_back(mg_form_code(MG_FF_WGRAD, f[0], f[1], 0, 0, m, 0));
            if (f[0] == 32 && f[1] == 32)
                for (int m : {C, G}) v.push_back(mg_form_code(MG_FF_WGRAD, f[0], f[1], 0, 0, m, XF));
        }
        for (int fam : {MG_FF_REDUCE, MG_FF_REDUCE_WAVE, MG_FF_REDUCE_TILE, MG_FF_REDUCE_BATCHED}) v.push_back(mg_form_code(fam, 0, 0, 0, 0, X, 0));
        return v;
    }();
    return forms;
}

int format_form(uint64_t code, char* buf, int cap) {
    const int fam = (int)(code & 0xff), mode = (int)(code >> 40 & 0xff), flags = (int)(code >> 48 & 0xff);
    const FamInfo& fi = fam_info(fam);
    char tmp[96];
    int n = snprintf(tmp, sizeof(tmp), "%s", fi.name);
    for (int i = 0; i < fi.nargs; ++i) n += snprintf(tmp + n, sizeof(tmp) - n, "%c%d", i ? ',' : '<', (int)(code >> (8 * (i + 1)) & 0xff));
    if (fi.nargs) n += snprintf(tmp + n, sizeof(tmp) - n, ">");
    if (mode != MG_FORM_NOMODE) n += snprintf(tmp + n, sizeof(tmp) - n, "/%s", mode == MG_MODE_CONV ? "CONV" : mode == MG_MODE_TCONV ? "TCONV" : "GATHER");
    if (flags & MG_FORM_RES) n += snprintf(tmp + n, sizeof(tmp) - n, "/res");
    if (flags & MG_FORM_XF) n += snprintf(tmp + n, sizeof(tmp) - n, "/xf");
    if (flags & MG_FORM_BNB) n += snprintf(tmp + n, sizeof(tmp) - n, "/bnb");
    if (flags & MG_FORM_PHASED) n += snprintf(tmp + n, sizeof(tmp) - n, "/phased");
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", tmp);
    return n;
}

}  // namespace

extern "C" void mg_conv_forms_clear(void) { g_last_n = 0; }
extern "C" void mg_conv_forms_push(uint64_t code) {
    if (g_last_n < LAST_CAP) g_last[g_last_n] = code;
    ++g_last_n;
}

extern "C" int mg_conv_form_count(void) { return (int)all_forms().size(); }

extern "C" int mg_conv_form_name(int id, char* buf, int cap) {
    const auto& f = all_forms();
    if (id < 0 || id >= (int)f.size()) return -1;
    return format_form(f[id], buf, cap);
}

extern "C" int mg_conv_last_forms(int* ids, int cap) {
    const auto& f = all_forms();
    for (int i = 0; i < g_last_n && i < LAST_CAP && i < cap; ++i) {
        int id = -1;
        for (int k = 0; k < (int)f.size(); ++k)
            if (f[k] == g_last[i]) { id = k; break; }
        if (ids) ids[i] = id;
    }
    return g_last_n;
}
