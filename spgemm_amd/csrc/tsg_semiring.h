// tsg_semiring.h -- the semirings of the plan kernels (tsg_numeric.hip,
// tsg_masked.hip): c(i,j) = (+) over k of A(i,k) (x) B(k,j).
//
// One trait struct per TSG_SEMIRING_* value (include/tsg.h).  The kernels are
// templated on it and never name an operator themselves:
//   identity()    the (+)-identity: what an entry no product reaches holds, what
//                 a sum starts from, what a lane without a source contributes
//   mul(a, b)     (x)
//   add(x, y)     (+), in registers
//   atomic(p, x)  *p := *p (+) x, on LDS and on global memory alike: the plain
//                 atomicAdd / atomicMin / atomicMax(double *) -- ds_add_f64 /
//                 ds_min_f64 / ds_max_f64 on LDS, global_atomic_{add,min,max}_f64
//                 on global memory, no compare-and-swap loop -- correct on
//                 fine-grained memory too (c_val is the caller's, its kind
//                 unknown; tsg_numeric.hip's header)
//   kValues       whether a_val / b_val are read at all (PLUS_PAIR: never, the
//                 pointers may be null -- sr_load then yields 1.0 without a read)
// min and max are exact, so the five min / max semirings give the same bits
// whatever the order of the sum; PLUS_PAIR sums small integers, exact too.
// NaN inputs and the sign of a zero result are unspecified for min / max.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/tsg.h"

namespace tsg {

struct SrAddMonoid {
    static __host__ __device__ __forceinline__ double identity() { return 0.0; }
    static __device__ __forceinline__ double add(double x, double y) { return x + y; }
    static __device__ __forceinline__ void atomic(double *p, double x) { atomicAdd(p, x); }
};
struct SrMinMonoid {
    static __host__ __device__ __forceinline__ double identity() { return __builtin_huge_val(); }
    static __device__ __forceinline__ double add(double x, double y) { return fmin(x, y); }
    static __device__ __forceinline__ void atomic(double *p, double x) { atomicMin(p, x); }
};
struct SrMaxMonoid {
    static __host__ __device__ __forceinline__ double identity() { return -__builtin_huge_val(); }
    static __device__ __forceinline__ double add(double x, double y) { return fmax(x, y); }
    static __device__ __forceinline__ void atomic(double *p, double x) { atomicMax(p, x); }
};

struct SrPlusTimes : SrAddMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return a * b; }
};
struct SrMinPlus : SrMinMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return a + b; }
};
struct SrMaxPlus : SrMaxMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return a + b; }
};
struct SrMaxTimes : SrMaxMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return a * b; }
};
struct SrMaxMin : SrMaxMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return fmin(a, b); }
};
struct SrMinMax : SrMinMonoid {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ double mul(double a, double b) { return fmax(a, b); }
};
struct SrPlusPair : SrAddMonoid {
    static constexpr bool kValues = false;
    static __device__ __forceinline__ double mul(double, double) { return 1.0; }
};

// v[q], or 1.0 without touching v where the semiring reads no values
template <class SR> __device__ __forceinline__ double sr_load(const double *v, long q) {
    if constexpr (SR::kValues) return v[q];
    else return 1.0;
}

// the one switch from a TSG_SEMIRING_* value to its traits: f(SR{}) for a known
// semiring, TSG_ERR_INVALID otherwise
template <class F> static inline int semiring_dispatch(int semiring, F f) {
    switch (semiring) {
    case TSG_SEMIRING_PLUS_TIMES: return f(SrPlusTimes{});
    case TSG_SEMIRING_MIN_PLUS: return f(SrMinPlus{});
    case TSG_SEMIRING_MAX_PLUS: return f(SrMaxPlus{});
    case TSG_SEMIRING_MAX_TIMES: return f(SrMaxTimes{});
    case TSG_SEMIRING_MAX_MIN: return f(SrMaxMin{});
    case TSG_SEMIRING_MIN_MAX: return f(SrMinMax{});
    case TSG_SEMIRING_PLUS_PAIR: return f(SrPlusPair{});
    default: return TSG_ERR_INVALID;
    }
}

// ---- the binary ops of the element-wise pass (tsg_ewise.hip): one trait struct
// per TSG_BINOP_* value.  apply(x, y) combines x = alpha a and y = beta b, each
// already rounded (ew_scale), and rounds once more: contraction is off in these
// bodies, so the product and the sum never fuse into an fma (device code is
// compiled with contraction on).  kReadsA / kReadsB: whether apply reads x / y
// at all -- the kernels then skip the load and the scaling of the other.
struct EwPlus {
    static constexpr bool kReadsA = true, kReadsB = true;
    static __device__ __forceinline__ double apply(double x, double y) {
#pragma clang fp contract(off)
        return x + y;
    }
};
struct EwTimes {
    static constexpr bool kReadsA = true, kReadsB = true;
    static __device__ __forceinline__ double apply(double x, double y) {
#pragma clang fp contract(off)
        return x * y;
    }
};
struct EwMin {
    static constexpr bool kReadsA = true, kReadsB = true;
    static __device__ __forceinline__ double apply(double x, double y) { return fmin(x, y); }
};
struct EwMax {
    static constexpr bool kReadsA = true, kReadsB = true;
    static __device__ __forceinline__ double apply(double x, double y) { return fmax(x, y); }
};
struct EwFirst {
    static constexpr bool kReadsA = true, kReadsB = false;
    static __device__ __forceinline__ double apply(double x, double) { return x; }
};
struct EwSecond {
    static constexpr bool kReadsA = false, kReadsB = true;
    static __device__ __forceinline__ double apply(double, double y) { return y; }
};
// scalar * v, rounded once (never the first half of an fma)
__device__ __forceinline__ double ew_scale(double scalar, double v) {
#pragma clang fp contract(off)
    return scalar * v;
}

// the one switch from a TSG_BINOP_* value to its traits
template <class F> static inline int binop_dispatch(int op, F f) {
    switch (op) {
    case TSG_BINOP_PLUS: return f(EwPlus{});
    case TSG_BINOP_TIMES: return f(EwTimes{});
    case TSG_BINOP_MIN: return f(EwMin{});
    case TSG_BINOP_MAX: return f(EwMax{});
    case TSG_BINOP_FIRST: return f(EwFirst{});
    case TSG_BINOP_SECOND: return f(EwSecond{});
    default: return TSG_ERR_INVALID;
    }
}

}  // namespace tsg
