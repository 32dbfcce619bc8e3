// Small host-side helpers shared by the translation units of libnsff_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nsff_render.h"

inline thread_local hipError_t g_nsff_last_err = hipSuccess;
inline int nsff_hip_fail(hipError_t e) { g_nsff_last_err = e; return NSFF_ERR_HIP; }
inline int nsff_launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NSFF_OK : nsff_hip_fail(e);
}

// ---- the f16x3 value-domain flag (NSFF_RANGE_*, nsff_range_flags) ----
// The word itself is defined once, in field.hip (the library is not built with -fgpu-rdc: a __device__ variable per translation
// unit would be a separate word); every other kernel receives its address through its argument struct.  Null (the first launch
// of a device happened inside a stream capture, before anything resolved the address) = the launch records nothing.
uint32_t* nsff_range_word(hipStream_t st);
constexpr float NSFF_F16_MAX = 65504.f;
// one atomic per wave, issued by its first lane that saw a value outside the fp16 range (`m`: the lane's running max of |x|;
// !(m <= 65504) so that a NaN that reached it counts).  Call with the whole wave converged.
__device__ __forceinline__ void nsff_range_flag(uint32_t* word, float m, uint32_t bit, unsigned lane) {
    const unsigned long long hit = __builtin_amdgcn_ballot_w64(!(m <= NSFF_F16_MAX));
    if (hit != 0ull && word != nullptr && lane == (unsigned)__builtin_ctzll(hit)) atomicOr(word, bit);
}
__device__ __forceinline__ void nsff_range_flag(uint32_t* word, float m, uint32_t bit) { nsff_range_flag(word, m, bit, threadIdx.x & 63u); }
// m = max(m, |a|, |b|) in one instruction (v_max3 drops a NaN operand: see nsff_range_flag)
__device__ __forceinline__ float nsff_absmax3(float m, float a, float b) {
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}
