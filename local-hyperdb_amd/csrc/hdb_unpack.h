// hdb_unpack.h -- how a stored row becomes accumulate-type values: the element traits of every stored dtype, the widening of one
// 16-byte piece (hdb_unpack) and of one element (hdb_to_f).  One text for the VALU scan (hdb_scan.hip) and the units that must
// reproduce its partial sums bit for bit (hdb_rerank.hip).
#pragma once
#include "hdb_common.h"

template <typename T> struct Elem;
template <> struct Elem<__half> { using Acc = float;  static constexpr int EPC = 8; };
template <> struct Elem<hdb_bf16> { using Acc = float; static constexpr int EPC = 8; };
template <> struct Elem<hdb_f8> { using Acc = float; static constexpr int EPC = 16; };
template <> struct Elem<hdb_i8> { using Acc = float; static constexpr int EPC = 16; };
template <> struct Elem<float>  { using Acc = float;  static constexpr int EPC = 4; };
template <> struct Elem<double> { using Acc = double; static constexpr int EPC = 2; };

__device__ __forceinline__ void hdb_unpack(const uint4& raw, float (&x)[8], __half*) {
    const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) { float2 f = __half22float2(h[i]); x[2 * i] = f.x; x[2 * i + 1] = f.y; }
}
// bfloat16 pairs: the even element is the low half of its word (a shift), the odd one the high half (a mask)
__device__ __forceinline__ void hdb_unpack(const uint4& raw, float (&x)[8], hdb_bf16*) {
    const unsigned int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = __uint_as_float(w[i] << 16); x[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
}
// float8 e4m3 (OCP): v_cvt_pk_f32_fp8 widens the two bytes of one half of a word (word select: false = bytes 0-1, true = bytes
// 2-3), exactly -- element 4 i + b of the chunk is byte b of word i
__device__ __forceinline__ void hdb_unpack(const uint4& raw, float (&x)[16], hdb_f8*) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const int w[4] = {(int)raw.x, (int)raw.y, (int)raw.z, (int)raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
        x[4 * i] = lo[0]; x[4 * i + 1] = lo[1]; x[4 * i + 2] = hi[0]; x[4 * i + 3] = hi[1];
    }
}
// int8: element 4 i + b of the chunk is byte b of word i, sign-extended and converted by one v_cvt_f32_i32 with a byte select
// (hdb_i8_cvt): 16 instructions per 16-byte load against float8's 8
__device__ __forceinline__ void hdb_unpack(const uint4& raw, float (&x)[16], hdb_i8*) {
    const int w[4] = {(int)raw.x, (int)raw.y, (int)raw.z, (int)raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[4 * i] = hdb_i8_cvt<0>(w[i]); x[4 * i + 1] = hdb_i8_cvt<1>(w[i]); x[4 * i + 2] = hdb_i8_cvt<2>(w[i]); x[4 * i + 3] = hdb_i8_cvt<3>(w[i]);
    }
}
__device__ __forceinline__ void hdb_unpack(const uint4& raw, float (&x)[4], float*) {
    x[0] = __uint_as_float(raw.x); x[1] = __uint_as_float(raw.y);
    x[2] = __uint_as_float(raw.z); x[3] = __uint_as_float(raw.w);
}
__device__ __forceinline__ void hdb_unpack(const uint4& raw, double (&x)[2], double*) {
    x[0] = __longlong_as_double(((unsigned long long)raw.y << 32) | raw.x);
    x[1] = __longlong_as_double(((unsigned long long)raw.w << 32) | raw.z);
}

__device__ __forceinline__ float hdb_to_f(__half v) { return __half2float(v); }
__device__ __forceinline__ float hdb_to_f(hdb_bf16 v) { return hdb_bf16_to_f(v); }
__device__ __forceinline__ float hdb_to_f(hdb_f8 v) { return __builtin_amdgcn_cvt_f32_fp8((int)v.bits, 0); }
__device__ __forceinline__ float hdb_to_f(hdb_i8 v) { return hdb_i8_to_f(v); }
__device__ __forceinline__ float hdb_to_f(float v) { return v; }
__device__ __forceinline__ double hdb_to_f(double v) { return v; }
