// host_util.hpp -- argument errors, environment switches and the debug stopwatch.  Plain C++ (no HIP): common.hpp includes
// it for the device side, the host-only sources (assembly_plan.cpp, mf_analysis.cpp, mf_launch_plan.hpp) include it alone.
#pragma once
#include <chrono>
#include <cstdlib>
#include <stdexcept>

namespace mgbhip {

struct InvalidArgument : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define MGB_REQUIRE(cond, msg)                                   \
    do {                                                         \
        if (!(cond)) throw ::mgbhip::InvalidArgument(msg);       \
    } while (0)

// NAME=1 in the environment.  Callers on a hot path keep the answer in a `static const bool`: read once per process.
inline bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}
// MGBHIP_DEBUG as a number, 0 when unset
inline int debug_level() {
    const char* e = getenv("MGBHIP_DEBUG");
    return e ? atoi(e) : 0;
}

// seconds since construction, for the MGBHIP_DEBUG >= 2 timing lines on stderr
struct Stopwatch {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace mgbhip
