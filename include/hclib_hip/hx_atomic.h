// hx_atomic.h — privatised atomics in device code (the device side of
// include/hclib_atomic.h).
//
// The reference keeps one padded copy of an atomic per worker thread, lets
// each worker update its own copy without synchronisation and folds the
// copies when the program asks for the value (inc/hclib_atomic.h:37-42,
// 81-137; src/hclib_atomic.c:34-54). A device worker is a wave
// (hx::current_worker(), hx_common.h), so here:
//
//   storage   nslots slots in device memory, each on its own 128-byte line,
//             nslots a power of two that is at least the worker count of any
//             launch this library makes (hclib_hip_atomic_create);
//   update    the active lanes of the wave combine their values in registers,
//             then the first active lane does ONE relaxed agent-scope
//             read-modify-write on slot current_worker() & (nslots - 1);
//   gather    one workgroup folds the slots in a fixed order
//             (hclib_hip_atomic_gather, csrc/atomic.hip).
//
// The slot write is an atomic, so workers that share a slot (a grid of the
// caller's own that is larger than nslots, two streams) are slower, never
// wrong. update() is correct under any set of active lanes: a full wave
// combines with a butterfly (hx::wave_sum's shape); a partial one walks the
// ballot with v_readlane, because a cross-lane shuffle would read the
// registers of lanes that are switched off.
#pragma once

#include <limits>
#include <type_traits>

#include "hx_common.h"

namespace hx {

// dtype / op codes of the C ABI (HCLIB_HIP_ATOMIC_* in include/hclib_hip.h)
template <typename T>
struct AtomicDtype;
template <>
struct AtomicDtype<int32_t> {
    static constexpr int value = 0;
};
template <>
struct AtomicDtype<uint32_t> {
    static constexpr int value = 1;
};
template <>
struct AtomicDtype<int64_t> {
    static constexpr int value = 2;
};
template <>
struct AtomicDtype<uint64_t> {
    static constexpr int value = 3;
};
template <>
struct AtomicDtype<float> {
    static constexpr int value = 4;
};
template <>
struct AtomicDtype<double> {
    static constexpr int value = 5;
};
// `long long` / `unsigned long long` are distinct types from int64_t /
// uint64_t on LP64: accept them under the same codes
template <>
struct AtomicDtype<std::conditional_t<std::is_same<int64_t, long>::value, long long, long>> {
    static constexpr int value = 2;
};
template <>
struct AtomicDtype<std::conditional_t<std::is_same<uint64_t, unsigned long>::value, unsigned long long, unsigned long>> {
    static constexpr int value = 3;
};

// The three reductions. identity(): the value that changes nothing, what a
// thread that ran no iteration contributes. combine(): the fold of two
// partial values. apply(): the read-modify-write on a slot.
struct Sum {
    static constexpr int kId = 0;
    template <typename T>
    __host__ __device__ static T identity() {
        return T(0);
    }
    template <typename T>
    __host__ __device__ static T combine(T a, T b) {
        return a + b;
    }
    template <typename T>
    __device__ static void apply(T *slot, T v) {
        __hip_atomic_fetch_add(slot, v, __ATOMIC_RELAXED, HX_AGENT);
    }
};
struct Max {
    static constexpr int kId = 1;
    template <typename T>
    __host__ __device__ static T identity() {
        if constexpr (std::is_floating_point<T>::value) return -std::numeric_limits<T>::infinity();
        else return std::numeric_limits<T>::lowest();
    }
    template <typename T>
    __host__ __device__ static T combine(T a, T b) {
        return a > b ? a : b;
    }
    // f32: the compiler expands this to a compare-and-swap loop (gfx950 has no
    // global_atomic_max_f32); the slot belongs to one wave, so the loop runs once
    template <typename T>
    __device__ static void apply(T *slot, T v) {
        __hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED, HX_AGENT);
    }
};
// logical or, as inc/hclib_atomic.h:172-186: the value is 0 or 1
struct Or {
    static constexpr int kId = 2;
    template <typename T>
    __host__ __device__ static T identity() {
        return T(0);
    }
    template <typename T>
    __host__ __device__ static T combine(T a, T b) {
        return (a != T(0) || b != T(0)) ? T(1) : T(0);
    }
    // floating types have no atomic or: swapping 1 in is the same update
    template <typename T>
    __device__ static void apply(T *slot, T v) {
        if (v == T(0)) return;
        if constexpr (std::is_integral<T>::value) __hip_atomic_fetch_or(slot, T(1), __ATOMIC_RELAXED, HX_AGENT);
        else __hip_atomic_exchange(slot, T(1), __ATOMIC_RELAXED, HX_AGENT);
    }
};

// v of lane `src` (wave-uniform) for 4- and 8-byte types
template <typename T>
__device__ __forceinline__ T wave_readlane(T v, int src) {
    if constexpr (sizeof(T) == 4) {
        int w;
        __builtin_memcpy(&w, &v, 4);
        w = __builtin_amdgcn_readlane(w, src);
        __builtin_memcpy(&v, &w, 4);
        return v;
    } else {
        static_assert(sizeof(T) == 8, "4- or 8-byte values");
        int w[2];
        __builtin_memcpy(w, &v, 8);
        w[0] = __builtin_amdgcn_readlane(w[0], src);
        w[1] = __builtin_amdgcn_readlane(w[1], src);
        __builtin_memcpy(&v, w, 8);
        return v;
    }
}

// The fold of v over the lanes of `active` (the wave's current exec mask,
// never empty here), the same value in every active lane.
template <typename Op, typename T>
__device__ __forceinline__ T wave_combine(T v, unsigned long long active) {
    if (active == ~0ull) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = Op::template combine<T>(v, __shfl_xor(v, d, 64));
        return v;
    }
    unsigned long long m = active;
    T r = wave_readlane(v, __builtin_ctzll(m));
    for (m &= m - 1; m; m &= m - 1) r = Op::template combine<T>(r, wave_readlane(v, __builtin_ctzll(m)));
    return r;
}

// The device view of one atomic: a POD passed by value in a lambda capture
// or a Kind::Ctx (hclib::hip::atomic_*_t::view(), hclib_hip_atomic_view).
template <typename T, typename Op>
struct AtomicView {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "int32/uint32/int64/uint64/float/double");
    using value_type = T;
    using op_type = Op;

    char *slots;      // nslots lines of `stride` bytes, the value at offset 0
    uint32_t nslots;  // power of two
    uint32_t stride;

    __device__ __forceinline__ T *slot() const {
        return (T *)(slots + (size_t)((uint32_t)current_worker() & (nslots - 1u)) * stride);
    }

    // Callable under any active mask; the lanes that are off contribute nothing.
    __device__ __forceinline__ void update(T v) const {
        const unsigned long long active = __ballot(1);
        if constexpr (std::is_same<Op, Or>::value) {
            // a ballot counts active lanes only: no cross-lane data needed
            const bool any = __ballot(v != T(0)) != 0ull;
            if (any && lane_id() == (int)__builtin_ctzll(active)) Op::template apply<T>(slot(), T(1));
        } else {
            const T r = wave_combine<Op, T>(v, active);
            if (lane_id() == (int)__builtin_ctzll(active)) Op::template apply<T>(slot(), r);
        }
    }
    // the reference's spellings (inc/hclib_atomic.h:147-150, 163-165, 178-181)
    __device__ __forceinline__ const AtomicView &operator+=(T v) const {
        static_assert(std::is_same<Op, Sum>::value, "+= is the sum's update");
        update(v);
        return *this;
    }
    __device__ __forceinline__ const AtomicView &operator|=(T v) const {
        static_assert(std::is_same<Op, Or>::value, "|= is the or's update");
        update(v);
        return *this;
    }
};

}  // namespace hx
