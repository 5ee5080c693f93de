// vcfxg_env.h -- the one reader of the context's environment knobs (vcfxg_ctx.h reads them when a
// context opens).  Plain C++: tests/env_knobs_test.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace vcfxg {

inline const char *env_text(const char *name) { return getenv(name); }
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
// unset: dflt (as it stands); set: the value as strtoull / atoll read it (text that is no number
// reads as 0), clamped to [lo, hi]
inline uint64_t env_u64(const char *name, uint64_t dflt, uint64_t lo = 0, uint64_t hi = UINT64_MAX) {
    const char *e = getenv(name);
    return e ? std::min(std::max<uint64_t>(strtoull(e, nullptr, 10), lo), hi) : dflt;
}
inline int64_t env_i64(const char *name, int64_t dflt, int64_t lo = INT64_MIN, int64_t hi = INT64_MAX) {
    const char *e = getenv(name);
    return e ? std::min(std::max<int64_t>(atoll(e), lo), hi) : dflt;
}

}  // namespace vcfxg
