// Host-side dispatch shared by the launchers: run-time (method, flag) -> template argument, method names, grid sizes.
// Plain C++17, no device code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/ivs.h"

namespace ivs {

constexpr int IVS_MAX_DEV = 64;      // devices whose CU count and kernel attributes are cached per index

// The methods a kernel family is instantiated for.  with_method calls f(std::integral_constant<int, M>{}) for the M of
// the list that equals the run-time code and returns false (f not called) when the code is not in the list: the list is
// what keeps unsupported (kernel, method) pairs from being instantiated.
template <int... M> struct Methods {};
template <int... M, class F>
inline bool with_method(int method, Methods<M...>, F&& f) {
    return ((method == M && (f(std::integral_constant<int, M>{}), true)) || ...);
}
// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// the <...> part of a kernel name reported by ivs_last_kernel()
inline const char* method_name(int method) {
    static const char* const names[] = {"linear", "cubic", "cubicspline", "slinear", "nearest", "zero", "pchip", "akima",
                                        "from_derivatives", "quadratic", "barycentric", "krogh", "pad", "bfill"};
    static_assert(sizeof(names) / sizeof(names[0]) == IVS_BFILL + 1, "one name per method code");
    return method >= 0 && method <= IVS_BFILL ? names[method] : "?";
}

// Workgroups per CU that 160 KiB of LDS admit (granted in `granule`-byte units), at least 1 and at most `cap`
inline int workgroups_per_cu(size_t lds_bytes, int cap, size_t granule = 1) {
    const int n = (int)((160 * 1024) / ((lds_bytes + granule - 1) / granule * granule));
    return n > cap ? cap : (n < 1 ? 1 : n);
}

// 1-D grid of a grid-stride kernel: one workgroup per `per_block` items, at most `per_cu` workgroups per CU
inline int64_t capped_blocks(int64_t n, int num_cu, int per_block = 256, int per_cu = 16) {
    const int64_t blocks = (n + per_block - 1) / per_block, cap = (int64_t)num_cu * per_cu;
    return blocks > cap ? cap : blocks;
}

}  // namespace ivs
