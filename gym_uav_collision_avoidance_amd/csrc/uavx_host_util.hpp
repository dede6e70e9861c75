// uavx_host_util.hpp -- host-side plumbing of the C ABI that both translation units use (uavx_multi.hip, uavx_uw.hip): error
// reporting into a handle, the device guard, launch-and-report, grid and slab arithmetic.  Included at file scope, behind
// uavx_device.hpp; everything in it has internal linkage except the three functions uavx_multi_handle.hpp defines for both.
#pragma once

#include <string>
#include <utility>

bool uavx_recip_division_exact(double tau);
float uavx_f32_at_or_above(double b);
float uavx_f32_at_or_below(double b);

namespace {

// H: uavx_handle or uavx_uw_handle (any handle with a `std::string err`; may be NULL)
template <class H>
int fail(H *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}
template <class H>
int hip_fail(H *h, hipError_t e, const char *what) {
    return fail(h, UAVX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define UAVX_HIP(h, call)                                   \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return hip_fail(h, e_, #call); \
    } while (0)

// Launches go to the handle's device; the caller's current device is restored afterwards.
struct DeviceGuard {
    int prev = -1, want;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) : want(device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != want) err = hipSetDevice(want);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
};
#define UAVX_ENTER(h)                                                     \
    DeviceGuard guard_((h)->device);                                      \
    if (guard_.err != hipSuccess) return hip_fail((h), guard_.err, "hipSetDevice")

// What a launch left behind, as the status of the entry point (the error text goes into the handle).
template <class H>
int launched(H *h) {
    UAVX_HIP(h, hipGetLastError());
    return UAVX_OK;
}
// Launch `kernel` without dynamic LDS and report.
template <class H, class... P, class... A>
int launch(H *h, void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, A &&...args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, std::forward<A>(args)...);
    return launched(h);
}

// workgroups of kBlock threads for n items, one thread each
inline dim3 block_grid(int64_t n) { return dim3((unsigned)((n + uavx::kBlock - 1) / uavx::kBlock)); }
// The same for a kernel of that shape: one thread per item.
template <class H, class... P, class... A>
int launch_items(H *h, void (*kernel)(P...), int64_t n, hipStream_t st, A &&...args) {
    return launch(h, kernel, block_grid(n), dim3(uavx::kBlock), st, std::forward<A>(args)...);
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace
