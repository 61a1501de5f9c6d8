// sweep_clf_fx_impl.h -- what the kernels on FIXED-POINT cached fields share: D = 2^k J s kept exactly as
// int32 | int64, an accepted row applied entry by entry in integer arithmetic.  Included by sweep_clf_fx.hip (the classical
// sweep, its seeds) and sweep_transverse_fx.hip (the transverse sweep on the same fields).
#pragma once
#include "sweep_clf_impl.h"

namespace sga {

// 2^kx x as an integer: exact (the set-time scan chose kx so that it is one, and it fits the field type)
template <typename FT, typename JT>
__device__ __forceinline__ FT fx_of(JT x, int kx) {
    if constexpr (sizeof(JT) == 1) return (FT)x;  // integer J: kx = 0
    else return (FT)ldexp((double)x, kx);
}

// D_j += mult 2^kx J_ij for the EPL = 16 / sizeof(JT) couplings x = J[i][j0 .. j0 + EPL) of one lane (mult = -2 s_i);
// wrapping unsigned arithmetic (the intermediate 2 |2^k J| may pass the signed range, the result never does)
template <typename JT, typename FT, typename VEC>
__device__ __forceinline__ void fx_apply_chunk(FT *F, const VEC &x, long long j0, int mult, int kx) {
    constexpr int EPL = 16 / (int)sizeof(JT);
    constexpr int NV = EPL * (int)sizeof(FT) / 16;  // int4 per lane: 1 | 2 | 4 | 8
    using UFT = typename std::make_unsigned<FT>::type;
    int4 *p = reinterpret_cast<int4 *>(F + j0);
    int4 t[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) t[i] = p[i];
    FT v[EPL];
    JT e[EPL];
    __builtin_memcpy(v, t, sizeof(v));
    __builtin_memcpy(e, &x, sizeof(e));
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = (FT)((UFT)v[i] + (UFT)(FT)mult * (UFT)fx_of<FT>(e[i], kx));
    __builtin_memcpy(t, v, sizeof(v));
#pragma unroll
    for (int i = 0; i < NV; ++i) p[i] = t[i];
}

}  // namespace sga
