// What the companion libraries (select.hip, f64.hip, query.hip, foldin.hip) share, and nothing of the main library:
// the error plumbing of a C entry point and the layouts a block of an iterate is read in.  Private and header-only:
// every name is in the anonymous namespace, so each library keeps its own message and exports nothing new.  A file
// names its library's two return codes before the include:
//     #define COMPANION_ERR_INVALID SIMRANK_QUERY_ERR_INVALID
//     #define COMPANION_ERR_HIP SIMRANK_QUERY_ERR_HIP
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#if !defined(COMPANION_ERR_INVALID) || !defined(COMPANION_ERR_HIP)
#error "define COMPANION_ERR_INVALID and COMPANION_ERR_HIP before including companion.h"
#endif

namespace {

thread_local std::string g_error;          // what the library's *_last_error() returns

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

#define REQUIRE(cond, ...)                \
    do {                                  \
        if (!(cond)) {                    \
            set_error(__VA_ARGS__);       \
            return COMPANION_ERR_INVALID; \
        }                                 \
    } while (0)

#define HIP_CHECK(call)                                               \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) {                                       \
            set_error("%s failed: %s", #call, hipGetErrorString(e_)); \
            (void)hipGetLastError();                                  \
            return COMPANION_ERR_HIP;                                 \
        }                                                             \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The layouts of a block of an iterate ("iterate_layout" of simrank_plan_get & co).  The public headers of the select,
// query and fold-in libraries each declare them under their own prefix; each of those files asserts that they are these.
enum Layout : int { PANEL_F32 = 0, ROWMAJOR_F32 = 1, PANEL_F16 = 2, ROWMAJOR_F64 = 3 };

#define COMPANION_SAME_LAYOUT(PREFIX, NAME) \
    static_assert(int(PREFIX##NAME) == NAME, "the public header's " #PREFIX #NAME " is not the shared layout code")

constexpr float kHalfScale = 1.0f / 16384.0f;          // fp16-held values are value x 2^14

// element (r, c) of a block in layout L, widened as the dense hand-back widens it
template <int L>
__device__ inline double elem(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    if constexpr (L == PANEL_F32) {
        return (double)static_cast<const float*>(S)[((c >> 5) * stride + r) * 32 + (c & 31)];
    } else if constexpr (L == ROWMAJOR_F32) {
        return (double)static_cast<const float*>(S)[r * stride + c];
    } else if constexpr (L == PANEL_F16) {
        const __half h = static_cast<const __half*>(S)[((c >> 6) * stride + r) * 64 + (c & 63)];
        return (double)(__half2float(h) * kHalfScale);
    } else {
        return static_cast<const double*>(S)[r * stride + c];
    }
}

}  // namespace
