// Host-only launch layer of libwr_mi355x: one checked kernel launch and the dispatch from run-time codes (dtype, flags,
// small integer sets) to template arguments.  Every launch of the library goes through `launch` or
// `launch_lds`, so a kernel's template list is written once per launch and a failure is reported under the name of the
// kernel that failed.
#pragma once

#include <type_traits>
#include <utility>

#include "wr_common.hpp"

namespace wr {

// Launch `kernel` and return WR_OK, or WR_ELAUNCH with the HIP error text under `name`.  The arguments convert to the
// kernel's parameter types here (a literal nullptr, a non-const pointer for a const one).
template <typename... P, typename... A>
inline int launch(const char *name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(std::forward<A>(args))...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e));
        return WR_ELAUNCH;
    }
    return WR_OK;
}

// The same for a kernel whose dynamic LDS may exceed the default 64 KiB limit: raise the limit of that same kernel first
// (the result is ignored: a refusal shows as the launch's own error).
template <typename... P, typename... A>
inline int launch_lds(const char *name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...args)
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return launch(name, kernel, grid, block, lds, st, std::forward<A>(args)...);
}

// ---- typed dispatch: call `f` with a tag whose type carries the run-time value ----
// The return types are deduced on purpose: a call then instantiates the helper and `f`'s body where it stands, so the
// kernels are instantiated -- and laid out in the code object -- in the order the source first names them.  With a
// declared `int` the bodies would wait for the end of the file, behind any kernel a later function names directly.
template <int V>
using int_c = std::integral_constant<int, V>;

// Element type of a wr_dtype code (validated by the caller; anything that is not f32 / f16 is bf16, as everywhere).
// `f` receives a value of float / _Float16 / __bf16: `using T = decltype(t);`.
template <typename F>
inline auto with_dtype(int code, F &&f)
{
    if (code == WR_F32) return f(float{});
    if (code == WR_F16) return f(_Float16{});
    return f(__bf16{});
}

// `f` receives std::true_type or std::false_type: `decltype(b)::value`.
template <typename F>
inline auto with_bool(bool b, F &&f)
{
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// `f` receives std::integral_constant<int, V> for the first V of the list equal to `v`, the last V when none is.
template <int V0, int... Vs, typename F>
inline auto with_int(int v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return with_int<Vs...>(v, std::forward<F>(f));
    }
}

// unroll depth of a streaming kernel from its tuning key: 16, 8 or 4
inline int unroll_of(int key) { return tune_get(key) >= 16 ? 16 : tune_get(key) >= 8 ? 8 : 4; }

}  // namespace wr
