// Host-side helpers of the launchers that need no HIP: the knob reader and the per-device "done once" mask. Pure C++17 (no HIP include), so
// tests/csrc/launch_host_check.cpp exercises it as a stand-alone program. launch.h adds the pieces that talk to the runtime.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdlib>

constexpr int MG_MAX_DEVICES = 16;     // the library keeps per-device state (det.hip, launch.h) for this many device indices

// An integer knob from the environment, parsed the way atoi / atol parse: the leading integer of the text, 0 when there is none, `dflt` only when the
// variable is unset. Call sites keep `static const ... = mg_env_long("MG_...", D);`: every knob is read once, at first use.
inline long mg_env_long(const char* name, long dflt) {
    const char* e = std::getenv(name);
    return e ? std::strtol(e, nullptr, 10) : dflt;
}
inline const char* mg_env_str(const char* name) { return std::getenv(name); }      // nullptr: unset

// first_time(dev) is true exactly once per device index, also under racing threads (one fetch_or decides). An index outside [0, MG_MAX_DEVICES) is
// never remembered: always true, the caller's work is simply repeated. is_done(dev) only looks: a caller whose work can fail asks it first, does the
// work, and calls first_time(dev) to remember the device once the work has succeeded (launch.h: mg_lds_opt_in).
struct mg_once_mask {
    std::atomic<uint32_t> done{0};
    bool is_done(int dev) const { return dev >= 0 && dev < MG_MAX_DEVICES && (done.load(std::memory_order_acquire) & (1u << dev)); }
    bool first_time(int dev) {
        if (dev < 0 || dev >= MG_MAX_DEVICES) return true;
        const uint32_t bit = 1u << dev;
        return !(done.fetch_or(bit, std::memory_order_acq_rel) & bit);
    }
};
