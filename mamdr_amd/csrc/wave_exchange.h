// Cross-lane exchanges of a 64-lane wave on the vector ALU (gfx950), for the short dependent reduction chains that sit
// between two barriers of a step kernel.  `__shfl` / `__shfl_xor` compile to ds_bpermute_b32: every step is a round trip
// through the LDS crossbar plus an address register.  Each offset of a butterfly has a VALU form on gfx950:
//   32   v_permlane32_swap   (the two half-waves trade places)
//   16   v_permlane16_swap   (the odd rows of 16 trade places with the even ones)
//    8   DPP row_ror:8       (a row of 16 rotated by half)
//    4   two bank-masked DPP moves: banks 0 and 2 of a row read four lanes up, banks 1 and 3 four lanes down
//  2, 1  DPP quad_perm
// The helpers move VALUES only; what is added to what, and in which order of steps, is the `__shfl` form's, so a sum has
// the same bits (x + y and y + x round alike; with two different NaNs among the operands the payload that survives
// depends on which operand an instruction names first, which neither form fixes).  Every helper keeps its `__shfl` form
// beside it (`*_ref`): the documented meaning, and what tests/device/wave_exchange_check.hip compares against, bit for
// bit over all 64 lanes.
// (hazard: a VALU write of an operand needs two wait states before v_permlane*_swap reads it; for the builtins hipcc's
// hazard recogniser pads with s_nop where a write falls into that window.)
// This header includes nothing of the engine.
#pragma once
#include <hip/hip_runtime.h>

namespace mamdr {

// ---- the value of lane (l ^ O), one step
template <int CTRL, int BANKS>
__device__ __forceinline__ float wave_dpp_mov(float old, float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, x), CTRL,
                                                                 0xf, BANKS, false));
}
// v_permlane32_swap / v_permlane16_swap (vdst = x, src = y): .a is vdst afterwards -- its upper half (its odd rows of 16)
// now holds what src had in the lower half (the even rows) -- and .b is src afterwards, the other way round
struct WaveSwap {
    float a, b;
};
template <int O>
__device__ __forceinline__ WaveSwap wave_swap(float x, float y) {
    static_assert(O == 16 || O == 32, "the two swaps of gfx950");
    const unsigned ux = __builtin_bit_cast(unsigned, x), uy = __builtin_bit_cast(unsigned, y);
    const auto r = O == 32 ? __builtin_amdgcn_permlane32_swap(ux, uy, false, false)
                           : __builtin_amdgcn_permlane16_swap(ux, uy, false, false);
    const unsigned a = r[0], b = r[1];      // (scalars first: a bit cast of a vector ELEMENT reads the vector's first)
    return WaveSwap{__builtin_bit_cast(float, a), __builtin_bit_cast(float, b)};
}
template <int O>
__device__ __forceinline__ float wave_xor_get(float x) {
    static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "one butterfly step of a 64-lane wave");
    if constexpr (O == 32 || O == 16) {
        const WaveSwap r = wave_swap<O>(x, x);
        return ((threadIdx.x & 63) & O) != 0 ? r.a : r.b;
    } else if constexpr (O == 8) {
        return wave_dpp_mov<0x128, 0xf>(x, x);                     // row_ror:8
    } else if constexpr (O == 4) {
        const float up = wave_dpp_mov<0x104, 0x5>(x, x);           // row_shl:4, banks 0 and 2: lane l reads lane l + 4
        return wave_dpp_mov<0x114, 0xa>(up, x);                    // row_shr:4, banks 1 and 3: lane l reads lane l - 4
    } else if constexpr (O == 2) {
        return wave_dpp_mov<0x4e, 0xf>(x, x);                      // quad_perm:[2,3,0,1]
    } else {
        return wave_dpp_mov<0xb1, 0xf>(x, x);                      // quad_perm:[1,0,3,2]
    }
}
template <int O>
__device__ __forceinline__ float wave_xor_get_ref(float x) { return __shfl_xor(x, O); }

// ---- x + the value of lane (l ^ O): one step of a butterfly sum.  At 32 and 16 the two results of the swap are the
// lane's own value and its partner's (which is which differs between the halves): their sum needs no select
template <int O>
__device__ __forceinline__ float wave_xor_add(float x) {
    if constexpr (O == 32 || O == 16) {
        const WaveSwap r = wave_swap<O>(x, x);
        return r.a + r.b;
    } else {
        return x + wave_xor_get<O>(x);
    }
}
template <int O>
__device__ __forceinline__ float wave_xor_add_ref(float x) { return x + __shfl_xor(x, O); }

// ---- the sum over the wave in every lane: offsets 32, 16, 8, 4, 2, 1 in this order
__device__ __forceinline__ float wave_xor_sum64(float s) {
    s = wave_xor_add<32>(s);
    s = wave_xor_add<16>(s);
    s = wave_xor_add<8>(s);
    s = wave_xor_add<4>(s);
    s = wave_xor_add<2>(s);
    s = wave_xor_add<1>(s);
    return s;
}
__device__ __forceinline__ float wave_xor_sum64_ref(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// ---- the sum over the wave of a * b with the FIRST step fused: lane l starts from fma(a, b, p), p the ROUNDED product of
// lane l ^ 32.  That is what `s = a * b; s += __shfl_xor(s, 32)` compiles to under hipcc's default contraction, i.e. what
// k_tower4's output unit has always computed; written out, the bits no longer depend on what the compiler contracts
__device__ __forceinline__ float wave_xor_dot64(float a, float b) {
    float s = __builtin_fmaf(a, b, wave_xor_get<32>(a * b));
    s = wave_xor_add<16>(s);
    s = wave_xor_add<8>(s);
    s = wave_xor_add<4>(s);
    s = wave_xor_add<2>(s);
    s = wave_xor_add<1>(s);
    return s;
}
__device__ __forceinline__ float wave_xor_dot64_ref(float a, float b) {
    float s = __builtin_fmaf(a, b, __shfl_xor(a * b, 32));
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// ---- the lanes of a column (l & 15) across the four rows of 16: offsets 16, then 32
__device__ __forceinline__ float wave_xor_sum_16_32(float s) { return wave_xor_add<32>(wave_xor_add<16>(s)); }
__device__ __forceinline__ float wave_xor_sum_16_32_ref(float s) {
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return s;
}

// ---- every lane receives the values its column (l & 15) holds in the four rows of 16: g[q] = x of lane (l & 15) + 16 q.
// One 16-swap leaves (row 0 | row 0 | row 2 | row 2) and (row 1 | row 1 | row 3 | row 3); a 32-swap of each with itself
// spreads the lower half's and the upper half's row over the wave
__device__ __forceinline__ void wave_gather_rows16(float x, float (&g)[4]) {
    const WaveSwap r = wave_swap<16>(x, x);
    const WaveSwap e = wave_swap<32>(r.a, r.a), o = wave_swap<32>(r.b, r.b);
    g[0] = e.a;
    g[1] = o.a;
    g[2] = e.b;
    g[3] = o.b;
}
__device__ __forceinline__ void wave_gather_rows16_ref(float x, float (&g)[4]) {
    const int l = (int)threadIdx.x & 15;
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = __shfl(x, l + 16 * q);
}

}  // namespace mamdr
