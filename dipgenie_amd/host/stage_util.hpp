// Small helpers shared by the host stages (anchors.cpp, expanded_graph.cpp, haploid_dp.cpp, solve.cpp, diploid.cpp,
// fast_graph.cpp): the DG_DEBUG lap timer and the message of a failed backend call.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pipeline.hpp"

namespace dg {

// DG_DEBUG lap timer: lap("what") prints "[dg::<tag>] what <seconds since the previous lap>" to stderr, `what` padded to
// the site's column width.  The environment is read once per object.
struct Lap {
    const char *tag;
    int width;
    bool on;
    double t;
    Lap(const char *tag_, int width_) : tag(tag_), width(width_), on(getenv("DG_DEBUG") != nullptr), t(now_s()) {}
    void operator()(const char *what) {
        if (!on) return;
        const double n = now_s();
        fprintf(stderr, "[dg::%s] %-*s %.3f s\n", tag, width, what, n - t);
        t = n;
    }
};

inline std::string backend_error(const Backend &be, const char *what) {
    return std::string(what) + " failed: " + (be.last_error ? be.last_error() : "?");
}

// A stage function reports failure as its message ("" = success): failed(stage(...), err) hands it to the caller's err.
inline bool failed(const std::string &message, std::string &err) {
    if (message.empty()) return false;
    err = message;
    return true;
}

}  // namespace dg
