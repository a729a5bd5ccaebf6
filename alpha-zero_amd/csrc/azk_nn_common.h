// azk_nn_common.h - the vector types and small device helpers that the network kernels share (azk_nn.hip, azk_embed_tok.hip,
// azk_embed_conv.hip, azk_rows.hip, azk_nnx.hip, azk_tail.hip, azk_block.hip).  A helper lives here only if every copy that used to
// exist was textually the same function; a file pulls them in with `using namespace azk_nn;`.
// Left where they are because their copies differ: wait_vmcnt (azk_block.hip: counts 0..16, azk_tail.hip: 0..24 - the run-time
// branch tree differs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace azk_nn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// Sum over the 16 lanes of a DPP row (lanes sharing lane>>4), result in every lane: quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror - four v_add_f32 with a DPP operand instead of four ds_bpermute round trips.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// Sum over the 4 lanes of a quad, result in every lane of it.
__device__ __forceinline__ float quad_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    return v;
}

// fp32 -> bf16 (round to nearest even) as plain vector casts: hipcc lowers them to v_cvt_pk_bf16_f32
__device__ __forceinline__ uint4 pack8(const float *v) {
    f32x8 f;
#pragma unroll
    for (int q = 0; q < 8; q++) f[q] = v[q];
    union { bf16x8 b; uint4 u; } r;
    r.b = __builtin_convertvector(f, bf16x8);
    return r.u;
}

// four floats -> the 4 x bf16 operand of v_mfma_f32_16x16x16_bf16 with two v_cvt_pk_bf16_f32
__device__ __forceinline__ s16x4 pack4_bf16(f32x2 lo, f32x2 hi) {
    const u32x2 p = {__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2)), __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2))};
    return __builtin_bit_cast(s16x4, p);
}

// fp32 -> bf16 bits (round to nearest even) in integer arithmetic
__device__ __forceinline__ unsigned bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// exp(x) for x <= ~80 with float32 accuracy: x log2(e) carried as hi + lo (the plain product loses |x| ulps of the argument,
// 5e-6 relative at x = -80), v_exp_f32 on hi, first-order correction for lo.
__device__ __forceinline__ float exp_acc(float x) {
    const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.92596299112661746e-8f;
    const float hi = x * L2E_HI;
    const float lo = __builtin_fmaf(x, L2E_HI, -hi) + x * L2E_LO;
    const float r = __builtin_amdgcn_exp2f(hi);
    return __builtin_fmaf(r, lo * 0.693147180559945309f, r);
}

// nn.GELU (erf form) with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below the bf16 result's resolution):
// a dozen instructions instead of libm's erff.
__device__ __forceinline__ float gelu_erf(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float erf_abs = 1.0f - poly * __expf(-z * z);
    return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}

// nn.GELU (erf form) for the fp32-accurate tail (k_gemm_h and its LDS-staged form): libm's erff (a few float32 ulps: about 1e-7
// on erf, so |x| / 2 times that on the result, plus the two roundings of 0.5 x (1 + erf)).  The Abramowitz & Stegun 7.1.26 form with
// a true division stood here before: 1.5e-7 is the error of the FORMULA; evaluated in float32 (t = 1 / (1 + p z), whose rounding the
// polynomial's slope of 3.4 at t = 1 multiplies, the Horner chain, and the cancellation in 1 - poly exp) its erf was off by up to
// 6e-7 (largest near x = 0.035), 2.3 times the 1.5e-7 + __expf share the float64 tests allow ("What pins the fp16-plane
// tail links").  erff costs about fifty instructions on 32 values per lane of the wide link's epilogue - the 512 -> 2048 link that bench.py's
// fp32 line (`--nn-dtype fp32`, `fp32_line` of `--full`) runs on every simulation step; DESIGN.md, same place, has what that costs, measured.
__device__ __forceinline__ float gelu_erff(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}

// s_waitcnt vmcnt(N) for a compile-time N (the asm immediate wants an integer constant expression)
template <int N> __device__ __forceinline__ void wait_vmcnt_c() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// One LDS-DMA piece: 64 lanes x 16 bytes from per-lane global addresses to 1 KiB of LDS at the wave-uniform byte address lds_dst.
// As inline assembly on purpose: hipcc treats the builtin form as a pending LDS write and drains it with s_waitcnt vmcnt(0) in front of
// the next ds_read - every stage of a ring would be waited for at once.  The statement saves and restores M0 (the destination base);
// the loads are invisible to the compiler's own counters, so every wait for them is explicit (wait_vmcnt_c).
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

}  // namespace azk_nn
