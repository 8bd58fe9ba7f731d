// ops_elem.h -- the element types of fasterrcnn_amd.ops and their one rounding, stated once for every operator family: a tensor is
// float, float16 or bfloat16 IN MEMORY and float32 in registers.  A load widens exactly, the arithmetic is the float32 kernels', and a
// store rounds to nearest even once, NaN and infinities as torch's Tensor.to(), so that op(x_T) == op(x_T.float()).to(T) bit for bit.
#pragma once
#include "common.h"

namespace frcnn {

// the 16-bit storage types (FRCNN_OPS_F16 / FRCNN_OPS_BF16 of include/frcnn_hip.h)
struct f16 { _Float16 v; };
struct bf16 { unsigned short bits; };

// widen(e): the element's value, exactly
__device__ __forceinline__ float widen(float e) { return e; }
__device__ __forceinline__ float widen(f16 e) { return (float)e.v; }
__device__ __forceinline__ float widen(bf16 e) { return __uint_as_float((unsigned)e.bits << 16); }

// The empty asm pins v (a float or a vector of them) as float32 VALUES before a conversion to float16.  Without it the compiler folds a
// preceding float32 multiply or add into the conversion (v_fma_mixlo_f16), which rounds the exact product to float16 directly: where
// the float32 product is a float16 tie that skips the float32 rounding of the contract and lands on the other neighbour (seen on an
// MI355X: one column in 21384 of deform_conv2d).
template <typename T> __device__ __forceinline__ void pin_f32(T& v) { asm volatile("" : "+v"(v)); }

// round_to(v, e): e = v rounded into the element's type.  float16 by the hardware conversion (v_cvt_f16_f32); bfloat16 by the integer
// rounding of c10::BFloat16: every NaN becomes 0x7FC0 there, which the packed hardware conversion would not give.
__device__ __forceinline__ void round_to(float v, float& e) { e = v; }
__device__ __forceinline__ void round_to(float v, f16& e)
{
    pin_f32(v);
    e.v = (_Float16)v;
}
__device__ __forceinline__ void round_to(float v, bf16& e)
{
    const unsigned b = __float_as_uint(v);
    e.bits = v != v ? (unsigned short)0x7FC0 : (unsigned short)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}
// the same as a value
template <typename E> __device__ __forceinline__ E narrow(float v)
{
    E e;
    round_to(v, e);
    return e;
}

// Elem<E>: one element in memory as E, in registers as float32
template <typename E> struct Elem {
    static __device__ __forceinline__ float load(const E* p, size_t i) { return widen(p[i]); }
    static __device__ __forceinline__ void store(E* p, size_t i, float v) { p[i] = narrow<E>(v); }
};

// what an element is to a vector load or store
template <typename E> struct ElemRaw { typedef E type; };
template <> struct ElemRaw<f16> { typedef _Float16 type; };
template <> struct ElemRaw<bf16> { typedef unsigned short type; };

// ElemRun<E, N>: N consecutive elements in memory as E (run i of p: one aligned load or store), in registers as float32 (vec).  float
// and float16 runs convert as vectors -- widen's and round_to's conversions on every element, behind the same pin -- which is the
// form the compiler keeps packed; bfloat16 runs go through widen and round_to element by element.  at: one element, widened.
template <typename E, int N> struct ElemRun {
    static constexpr int V = N;
    typedef float vec __attribute__((ext_vector_type(N)));
    typedef int ivec __attribute__((ext_vector_type(N)));
    typedef typename ElemRaw<E>::type raw __attribute__((ext_vector_type(N)));
    static __device__ __forceinline__ vec load(const E* p, size_t i)
    {
        const raw r = reinterpret_cast<const raw*>(p)[i];
        if constexpr (__is_same(E, bf16)) {
            vec v;
#pragma unroll
            for (int j = 0; j < N; ++j) v[j] = widen(bf16{r[j]});
            return v;
        } else {
            return __builtin_convertvector(r, vec);
        }
    }
    static __device__ __forceinline__ void store(E* p, size_t i, vec v)
    {
        raw r;
        if constexpr (__is_same(E, bf16)) {
#pragma unroll
            for (int j = 0; j < N; ++j) r[j] = narrow<bf16>(v[j]).bits;
        } else {
            if constexpr (__is_same(E, f16)) pin_f32(v);
            r = __builtin_convertvector(v, raw);
        }
        reinterpret_cast<raw*>(p)[i] = r;
    }
    static __device__ __forceinline__ float at(const E* p, size_t i) { return widen(p[i]); }
};
template <typename E> static constexpr int ELEM_WIDE_RUN = 16 / (int)sizeof(E);      // the run of 16 bytes

}  // namespace frcnn

// The body of a 16-bit entry point by element-type code: returns the expression that follows E, in which E names the storage type
// (variadic only so that the expression may hold commas); any other code is FRCNN_EINVAL.
#define OPS_ELEM_DISPATCH(elem_type, E, ...)                                                \
    do {                                                                                    \
        if ((elem_type) == FRCNN_OPS_F16) { typedef frcnn::f16 E; return __VA_ARGS__; }     \
        if ((elem_type) == FRCNN_OPS_BF16) { typedef frcnn::bf16 E; return __VA_ARGS__; }   \
        return FRCNN_EINVAL;                                                                \
    } while (0)
