// antq_dispatch.h -- how a launcher of libantq turns a run-time value (dtype, a flag, vectors per lane, wavefronts per
// workgroup) into a template argument.  Host only, header only.  A launcher nests these around ONE launch expression:
//
//     return with_dtype(dtype, [&](auto tag) {
//         using T = decltype(tag);
//         return with_bool(ovp, [&](auto o) {
//             return with_value<8, 4>(one_of<8>(U, 4), [&](auto u) {
//                 launch_k(unordered, k<T, o.value, u.value>, grid, block, lds, st, args...);
//                 return launch_status();
//             });
//         });
//     });
//
// Only the listed values are instantiated.  A combination that has no kernel is excluded with `if constexpr` inside the
// innermost lambda, where the exclusion can be read next to the launch.
#ifndef ANTQ_DISPATCH_H
#define ANTQ_DISPATCH_H

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "../../include/antq.h"
#include "antq_device.h"

namespace antq {

// the status of the launches a launcher has just enqueued
static inline int launch_status() { return hipGetLastError() == hipSuccess ? ANTQ_OK : ANTQ_ERR_LAUNCH; }

// (always inlined: the lambdas' captures then stay in registers instead of a closure in memory, and the launcher compiles
//  to the code the hand-written ladders gave)
#define ANTQ_DISPATCH_INLINE static inline __attribute__((always_inline))

// f(float{}) / f(bf16_tag{}) / f(f16_tag{}); any other dtype: ANTQ_ERR_UNSUPPORTED.  (An entry point that also takes
// ANTQ_F64, or has another answer for an unknown dtype, says so at its call site.)
template <typename F>
ANTQ_DISPATCH_INLINE int with_dtype(int dtype, F &&f)
{
    switch (dtype) {
    case ANTQ_F32: return f(float{});
    case ANTQ_BF16: return f(bf16_tag{});
    case ANTQ_F16: return f(f16_tag{});
    default: return ANTQ_ERR_UNSUPPORTED;
    }
}

template <typename F>
ANTQ_DISPATCH_INLINE int with_bool(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals v.  A value that is not listed instantiates and
// launches nothing (ANTQ_ERR_UNSUPPORTED): the caller says what such a value runs with one_of.
template <int... Vs, typename F>
ANTQ_DISPATCH_INLINE int with_value(int v, F &&f)
{
    int rc = ANTQ_ERR_UNSUPPORTED;
    (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return rc;
}
// v if it is one of Vs, `otherwise` if it is not
template <int... Vs>
static inline int one_of(int v, int otherwise)
{
    return ((v == Vs) || ...) ? v : otherwise;
}

// One launch.  `unordered`: the dispatch packet goes out without the barrier bit (hipExtAnyOrderLaunch), so the kernel may
// start while the launches queued before it on the same stream are still draining -- the caller has promised that it
// does not depend on them (weights at rest).  Later ordinary launches still wait for it.
template <typename... KArgs, typename... Args>
static inline void launch_k(bool unordered, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args)
{
    if (unordered) hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, nullptr, nullptr, hipExtAnyOrderLaunch, static_cast<KArgs>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, static_cast<KArgs>(args)...);
}

}  // namespace antq

#endif  // ANTQ_DISPATCH_H
