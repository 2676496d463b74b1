// Stand-alone check of maggie_amd/csrc/launch_host.h (the knob reader and the per-device once-mask), compiled from the very header the launchers
// include. Built with -fsanitize=address,undefined -pthread by tests/test_launch_host_cpu.py; exit status 0 = every case holds.
#include "../../maggie_amd/csrc/launch_host.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static long knob(const char* text, long dflt) {
    if (text) setenv("MG_LAUNCH_HOST_CHECK", text, 1); else unsetenv("MG_LAUNCH_HOST_CHECK");
    return mg_env_long("MG_LAUNCH_HOST_CHECK", dflt);
}

int main() {
    // the knob reader: atoi / atol parsing, the default only when unset
    CHECK(knob(nullptr, 41) == 41);
    CHECK(knob(nullptr, -5) == -5);
    CHECK(knob("12", 41) == 12);
    CHECK(knob("-3", 41) == -3);
    CHECK(knob("7x", 41) == 7);
    CHECK(knob("x", 41) == 0);
    CHECK(knob("", 41) == 0);
    CHECK(knob("  9", 41) == 9);                       // (leading blanks, as atoi skips them)
    CHECK(knob("123456789012", 41) == 123456789012l);  // beyond int, read as long
    static_assert(sizeof(long) == 8 && 123456789012l > INT_MAX, "the case above needs a 64-bit long");
    unsetenv("MG_LAUNCH_HOST_CHECK");
    CHECK(mg_env_str("MG_LAUNCH_HOST_CHECK") == nullptr);
    setenv("MG_LAUNCH_HOST_CHECK", "8,32,4", 1);
    CHECK(mg_env_str("MG_LAUNCH_HOST_CHECK") && !std::strcmp(mg_env_str("MG_LAUNCH_HOST_CHECK"), "8,32,4"));

    // the once-mask
    static_assert(MG_MAX_DEVICES == 16, "the mask is one 32-bit word over 16 device indices");
    {
        mg_once_mask m;
        CHECK(!m.is_done(0));
        CHECK(m.first_time(0));
        CHECK(m.is_done(0) && !m.is_done(15) && !m.is_done(-1) && !m.is_done(16));
        CHECK(!m.first_time(0));
        CHECK(m.first_time(15));                       // independent of device 0
        CHECK(!m.first_time(15));
        CHECK(!m.first_time(0));
        for (int i = 0; i < 3; ++i) { CHECK(m.first_time(-1)); CHECK(m.first_time(16)); }      // outside [0, 16): never remembered
        CHECK(m.first_time(1));                        // and they left no bit behind
        CHECK(m.done.load() == ((1u << 0) | (1u << 1) | (1u << 15)));
    }
    for (int round = 0; round < 64; ++round) {        // eight threads racing on one index: exactly one `true`
        mg_once_mask m;
        std::atomic<int> go{0}, wins{0};
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&] {
                go.fetch_add(1);
                while (go.load() < 8) {}
                if (m.first_time(round % MG_MAX_DEVICES)) wins.fetch_add(1);
            });
        for (auto& t : th) t.join();
        CHECK(wins.load() == 1);
    }
    if (fails) return 1;
    std::puts("launch_host: ok");
    return 0;
}
