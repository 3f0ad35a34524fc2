// creg_common.h -- host-side helpers shared by the libcreg translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <vector>
#include "../../include/creg.h"

namespace creg {

void set_error(const char* fmt, ...);

#define CREG_HIP(call)                                                                  \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess) {                                                        \
            creg::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),     \
                            __FILE__, __LINE__);                                        \
            return CREG_EHIP;                                                           \
        }                                                                               \
    } while (0)

#define CREG_REQUIRE(cond, ...)                                                         \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            creg::set_error(__VA_ARGS__);                                               \
            return CREG_EINVAL;                                                         \
        }                                                                               \
    } while (0)

#define CREG_LAUNCH_CHECK()                                                             \
    do {                                                                                \
        hipError_t e__ = hipGetLastError();                                             \
        if (e__ != hipSuccess) {                                                        \
            creg::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), \
                            __FILE__, __LINE__);                                        \
            return CREG_EHIP;                                                           \
        }                                                                               \
    } while (0)

// The first failing HIP call of a sequence that must reach its teardown (an open capture, chains to join) whatever happens:
// CREG_TRY skips every call after it; the caller reports `what` and `err` once, at the end.
struct FirstError {
    hipError_t err = hipSuccess;
    const char* what = "";
    bool ok() const { return err == hipSuccess; }
    void note(hipError_t e, const char* w) { if (ok() && e != hipSuccess) { err = e; what = w; } }
};
#define CREG_TRY(fe, call) do { if ((fe).ok()) (fe).note((call), #call); } while (0)

// Handles that live for one scope, released on every way out of it (a null handle is not the owner's yet).
struct ScopedStream { hipStream_t h = nullptr; ScopedStream() = default; ScopedStream(const ScopedStream&) = delete; ~ScopedStream() { if (h) (void)hipStreamDestroy(h); } };
struct ScopedGraph { hipGraph_t h = nullptr; ScopedGraph() = default; ScopedGraph(const ScopedGraph&) = delete; ~ScopedGraph() { if (h) (void)hipGraphDestroy(h); } };
struct ScopedEvents {
    std::vector<hipEvent_t> v;
    explicit ScopedEvents(size_t n = 0) : v(n, nullptr) {}
    ScopedEvents(const ScopedEvents&) = delete;
    ~ScopedEvents() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
    hipEvent_t& operator[](size_t i) { return v[i]; }
};

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace creg
