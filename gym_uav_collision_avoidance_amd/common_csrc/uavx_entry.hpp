// What the entry points of libuavx_clip.so, libuavx_gae.so, libuavx_ppo.so, libuavx_norm.so, libuavx_prio.so, libuavx_keywalk.so
// and libuavx_actor.so's replay unit do alike on the host: argument checks, launch-and-report in uavx_actor.h's status codes,
// and the marker of the build's source hash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "../../include/uavx_actor.h"

namespace uavx_common {

static bool aligned(const void *p, uintptr_t al) { return ((uintptr_t)p & (al - 1)) == 0; }     // true for NULL

static bool unit(double x) { return x >= 0.0 && x <= 1.0; }     // false for NaN

// what a launch left behind, as the status of the entry point
static int launched() { return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP; }

// launches `kernel` as `blocks` workgroups of `wg` threads without dynamic LDS and reports
template <class... P, class... A>
static int launch(void (*kernel)(P...), int64_t blocks, int wg, hipStream_t st, A &&...args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(wg), 0, st, std::forward<A>(args)...);
    return launched();
}

}  // namespace uavx_common

// UAVX_BUILD_MARKER(UAVX_X_SRC_HASH); leaves the bytes "UAVX_X_SRC_HASH=<hash>\0" in the library, where the loader
// (_native.up_to_date) finds them in the file without mapping it.  The Makefile defines the name: the hash, or "" for a
// hand-run make.
#define UAVX_BUILD_MARKER(NAME) __attribute__((used)) static const char kBuildInfo[] = #NAME "=" NAME
