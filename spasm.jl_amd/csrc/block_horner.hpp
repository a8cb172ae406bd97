// block_horner.hpp -- a matrix polynomial of the resident exact product applied to a block of vectors over GF(p) on gfx950, one
// block Horner step per launch round: Y[row, j] <- (M Y)[row, j] + sum_{c < B} V[row, c] * C[c, j], for V of B in {2, 4, 8, 16}
// columns and Y of K <= B columns (spasm_amd_block_poly_apply, spasm_amd_block_wiedemann_solve).  D steps give
// X = sum_t M^t V C_t, which is what a block Wiedemann solve needs from the right generator of its sequence: about n / b products
// where the scalar Horner run of horner.hpp takes up to n, and one run serves up to b right-hand sides.
//
// The step is k_spmv_step / k_spmv_step_combine of spmv_step.hpp with BlockHornerEpi<SMALL, B> (KW = spmv_kw(K) <= B columns): the
// lane that owns y[row, j] stores y = y0 + sum_c V[row, c] * C[c, j], y0 the canonical row sum (for the long rows in the combine).
// C is the B x KW slice of this step in a device table of canonical residues (the host reduces the coefficients; steps x B x KW
// words, uploaded once per call).  The lane keeps the B words of its column j in registers over all its rows: the epilogue names
// BlockCoef<B> as its coefficient type in EpiCoef, and coef(j) reads them once, before the row loop.  The B words of V[row, :] are
// read by every lane of the row (the same addresses: one request a wave and row) and reduced where they are read (zp_residue).
//
// Bound of the combination: y0 is canonical, |y0| <= halfp < 2^31.  A term is ZpAcc<SMALL>::mul_lazy of two canonical residues, the
// domain tests/test_gpu_zp.py pins.  p < 2^16: |term| <= halfp + 256 < 2^15.1, so y0 and B <= 16 terms stay below 2^20 in an i32,
// far below the zp_lazy_terms limit (65043 terms at p = 65521).  Larger p: a plain product V * C is below 2^62 and 16 of them do
// not fit an i64, so the terms are lazy residues, |term| <= 0.51 p < 2^31.1, and y0 and 16 of them stay below 2^36 in an i64.
// Both are inside the domain of zp_reduce (|x| <= min(3 * 2^51 * p, 2^62), p >= 3), which gives the canonical y.
// Field operations only: every prime 2 < p <= 0xFFFFFFFB works.
//
// Counting (cnt != nullptr): the lane that owns y[row, j] contributes (y != 0) to cnt[j] through krylov_project, exactly as
// HornerEpi does: a count is at most the number of rows, an integer sum that does not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "spmv_step.hpp"

// the B coefficients C[0 .. B, j] a lane keeps for its column j
template <int B> struct BlockCoef {
    int c[B];
};

// y0 + sum_c V[row, c] * C[c, j]: y0 canonical, v the row of V (any int32), k canonical; the bound is argued above
template <bool SMALL, int B>
__device__ __forceinline__ int block_combine(const ZpField &F, int hp, int mhp, const int *__restrict__ v, const BlockCoef<B> &k, int y0)
{
    typename ZpAcc<SMALL>::type a = y0;
#pragma unroll
    for (int c = 0; c < B; c++) a += ZpAcc<SMALL>::mul_lazy(F, zp_residue(F, hp, mhp, v[c]), k.c[c]);
    return zp_reduce(F, (int64_t)a);
}

// The first step from Y = 0 is no product: Y[r, j] <- sum_c V[r, c] * C[c, j]; one lane per (row, column), striding over the rows.
template <bool SMALL, int B, int KW>
__global__ __launch_bounds__(KRY_BS) void k_block_horner_first(int n, int kc, ZpField F, int hp, int mhp, const int *__restrict__ T,
                                                               const int *__restrict__ V, i64d ldv, int *__restrict__ Y, i64d ldy,
                                                               long long *__restrict__ cnt)
{
    static_assert(KW <= B, "at most B columns");
    constexpr int RPB = KRY_BS / KW;
    const int j = threadIdx.x % KW;
    long long t = 0;
    if (j < kc) {
        BlockCoef<B> k;
#pragma unroll
        for (int c = 0; c < B; c++) k.c[c] = T[c * KW + j];
        for (i64d r = (i64d)blockIdx.x * RPB + threadIdx.x / KW; r < n; r += (i64d)gridDim.x * RPB) {
            const int y = block_combine<SMALL, B>(F, hp, mhp, V + r * ldv, k, 0);
            Y[r * ldy + j] = y;
            t += y != 0;
        }
    }
    if (cnt) krylov_project<KW>(t, cnt);
}

// T[(i * B + c) * B + r] <- S[(i * B + r) * B + c]: every term of a block sequence transposed, one lane per word
__global__ __launch_bounds__(256) void k_block_transpose_terms(i64d total, int b, const int *__restrict__ S, int *__restrict__ T)
{
    const i64d e = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const i64d bb = (i64d)b * b, i = e / bb;
    const int w = (int)(e - i * bb), r = w / b, c = w - r * b;
    T[i * bb + (i64d)c * b + r] = S[e];
}

// the epilogue of a block Horner step (spmv_step.hpp): Y[row, j] <- y0 + sum_c V[row, c] * T[c * KW + j] and the term (y != 0) of
// cnt[j]; counted only when cnt is given.  ldt is the KW of the launch.
template <bool SMALL, int B> struct BlockHornerEpi {
    const int *T, *V;
    i64d ldv;
    int ldt;
    long long *cnt;
    __device__ BlockCoef<B> coef(int j) const
    {
        BlockCoef<B> k;
#pragma unroll
        for (int c = 0; c < B; c++) k.c[c] = T[c * ldt + j];
        return k;
    }
    __device__ long long own(const ZpField &F, int hp, int mhp, const BlockCoef<B> &k, int row, int, int y0, int *yp) const
    {
        const int y = block_combine<SMALL, B>(F, hp, mhp, V + (i64d)row * ldv, k, y0);
        *yp = y;
        return y != 0;
    }
    __device__ bool projects() const { return cnt != nullptr; }
    __device__ long long *sums() const { return cnt; }
};

template <bool SMALL, int B> struct EpiCoef<BlockHornerEpi<SMALL, B>> { typedef BlockCoef<B> type; };
