// The library's host-worker convention for code outside jaad_capi.cpp: the same rule as its
// host_threads() (a context's worker pool), restated here so that file stays as it is.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <thread>

namespace jaad {

// Host worker threads: 16 (one GPU's CPU share on the target nodes) or fewer CPUs;
// JAAD_HOST_THREADS overrides (1..64).
inline int host_threads()
{
    if (const char* e = std::getenv("JAAD_HOST_THREADS")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64) return v;
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::min(16u, hw ? hw : 1u);
}

}  // namespace jaad
