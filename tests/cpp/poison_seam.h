// Failure seam for the CPU emulator build of the library (tests only; see pprobe_cases.build_poison): force-included in front of every source, it
// routes the library's hipMemcpyAsync calls through a wrapper that can fail ONE device-to-host copy -- the way a pfv_encoder ends up "poisoned"
// (its reference has advanced, the frame's packet was never written), which no public call can provoke.
// pfv_seam_fail_d2h = n > 0: the n-th device-to-host copy from now fails with hipErrorInvalidValue and the counter returns to 0.
#pragma once
#include <hip/hip_runtime.h>

__attribute__((visibility("default"))) inline int pfv_seam_fail_d2h = 0;

static inline hipError_t pfv_seam_memcpy_async(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t st)
{
    if (kind == hipMemcpyDeviceToHost && pfv_seam_fail_d2h > 0 && --pfv_seam_fail_d2h == 0) return hipErrorInvalidValue;
    return hipMemcpyAsync(d, s, n, kind, st);
}
#define hipMemcpyAsync pfv_seam_memcpy_async
