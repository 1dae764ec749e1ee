// Lane exchanges and wave reductions without an LDS round trip, one definition for every kernel (__shfl_xor compiles to
// ds_bpermute_b32 pairs, ~100 cycles of latency each in the dependent chain of a reduction).  Inside a row of 16 lanes: DPP moves,
// one VALU instruction per 32-bit half.  Across the rows (the MFMA operand layouts keep one k-group per row): gfx950's permlane
// swaps -- v_permlane16_swap exchanges the odd rows of one register with the even rows of another, v_permlane32_swap the upper half
// of one with the lower half of the other; with both registers = v the two results are {even rows, odd rows} resp. {lower half,
// upper half} in both rows' / halves' places, one of them the lane's own value, the other the one of lane l ^ 16 resp. l ^ 32.
// Their sum has the value of `v += __shfl_xor(v, 16, 64)` / `(v, 32, 64)`.
#pragma once
#include <hip/hip_runtime.h>

template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    // (bound_ctrl: a lane whose source lies outside its row reads 0 -- the row shifts rely on it -- and no `old` operand has to
    //  be zeroed first)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void xrow_swap16(double v, double& a, double& b) {
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
    a = __hiloint2double(hi[0], lo[0]); b = __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ void xrow_swap32(double v, double& a, double& b) {
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
    a = __hiloint2double(hi[0], lo[0]); b = __hiloint2double(hi[1], lo[1]);
}
// v[l] + v[l ^ 16] and v[l] + v[l ^ 32] in every lane
__device__ __forceinline__ double xrow_sum16(double v) { double a, b; xrow_swap16(v, a, b); return a + b; }
__device__ __forceinline__ double xrow_sum32(double v) { double a, b; xrow_swap32(v, a, b); return a + b; }
// t[l] + t[l ^ 4] + t[l ^ 8] + t[l ^ 12] for the lanes of the first quad of every row (the others get another association of
// the same four values): two row rotations instead of two ds_bpermute pairs
__device__ __forceinline__ double quad4_sum(double t) {
    t += dpp_move<0x124>(t);   // row_ror:4
    t += dpp_move<0x128>(t);   // row_ror:8
    return t;
}
// op over every aligned group of SP adjacent lanes (SP a power of two), the same value in every lane of the group: a fixed butterfly,
// the same tree in every lane; all 64 lanes must be active
template <int SP, class Op>
__device__ __forceinline__ double group_reduce(double v, Op op) {
    static_assert(SP >= 1 && SP <= 64 && (SP & (SP - 1)) == 0, "power of two");
    [[maybe_unused]] double a, b;
    if constexpr (SP >= 2) v = op(v, dpp_move<0xB1>(v));     // quad_perm [1,0,3,2]
    if constexpr (SP >= 4) v = op(v, dpp_move<0x4E>(v));     // quad_perm [2,3,0,1]
    if constexpr (SP >= 8) v = op(v, dpp_move<0x141>(v));    // row_half_mirror
    if constexpr (SP >= 16) v = op(v, dpp_move<0x140>(v));   // row_mirror
    if constexpr (SP >= 32) { xrow_swap16(v, a, b); v = op(a, b); }
    if constexpr (SP >= 64) { xrow_swap32(v, a, b); v = op(a, b); }
    return v;
}
template <int SP>
__device__ __forceinline__ double group_sum(double v) { return group_reduce<SP>(v, [](double x, double y) { return x + y; }); }
// the 16 lanes of a DPP row (= the 16 points of a neuron group)
__device__ __forceinline__ double row_sum16(double v) { return group_sum<16>(v); }
// sum over the 256 threads of a workgroup, fixed order: butterfly inside each wave, the four wave sums added in wave order; every
// thread gets it.  red: four doubles of LDS; the leading barrier lets a caller use it again at once
__device__ __forceinline__ double block_sum256(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
