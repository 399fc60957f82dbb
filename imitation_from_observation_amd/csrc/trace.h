// trace.h -- option "trace_launch" for the launchers outside gemm_launch.h (wconvt.hip, convt3.hip, convt3m.hip, c3conv.hip,
// c3wgrad.hip, dconv.hip, convt_product): one stderr line per distinct launch, in the style of the implicit GEMM's, `family | key value ...`.
// Host code only.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <set>
#include <string>

#include "options.h"

namespace ctx {

__attribute__((format(printf, 1, 2))) inline void trace_launch(const char* fmt, ...) {
    if (!opt(OPT_TRACE_LAUNCH)) return;
    static std::mutex mu;
    static std::set<std::string> seen;
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> g(mu);
    if (seen.insert(buf).second) fprintf(stderr, "%s\n", buf);
}

}  // namespace ctx
