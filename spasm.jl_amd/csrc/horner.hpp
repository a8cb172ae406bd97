// horner.hpp -- a polynomial of the resident exact product applied to vectors over GF(p) on gfx950, one Horner step per launch
// round: Y[row, v] <- (A X)[row, v] + T[v] * B[row, v] (spasm_amd_poly_apply, spasm_amd_wiedemann_solve).
//
// The Horner step is k_spmv_step / k_spmv_step_combine of spmv_step.hpp with HornerEpi: the lane that owns y[row, v] stores
// zp_axpy(T[v], b[row, v], y0), y0 the canonical row sum (for the long rows in the combine).  T is the KW-wide row of this step in a
// device table of canonical residues (the host reduces the coefficients; steps x KW words, uploaded once per call); a column whose
// polynomial has a lower degree has zeros at the top of the table and stays 0 until its leading coefficient arrives, because
// A 0 + 0 b = 0.  Entries of B and of the first X (the caller's arrays) are reduced where they are read (zp_residue).
//
// Bound of the combination: the row sum r is what SPMV_TEAM_SUM leaves: for p < 2^16 the sum of at most 64 canonical residues,
// |r| < 2^21; for larger p the sum of at most 64 i64 accumulators of at most SPMV_SEG lazy terms below 2^31.1, |r| < 2^51.1; in
// the combine the sum of at most 2^31 / SPMV_SEG canonical partial sums, |s| < 2^48.  All are inside the domain of zp_reduce
// (|x| <= min(3 * 2^51 * p, 2^62), p >= 3), which gives the canonical y0.  T[v] is canonical (host), b is canonical after
// zp_residue, so y = zp_axpy(T[v], b, y0) takes three canonical residues: the domain tests/test_gpu_zp.py pins.
// Field operations only: every prime 2 < p <= 0xFFFFFFFB works.
//
// Counting (cnt != nullptr): the lane that owns y[row, v] contributes (y != 0) to cnt[v], reduced through krylov_project: lanes,
// then waves, then one 64-bit vector atomic per (workgroup, column).  A count is at most the number of rows, < 2^31, far inside
// krylov_project's |t| < 2^62; it is an integer sum, so it does not depend on scheduling.  cnt[v] == 0 says column v of Y is zero.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "krylov.hpp"

// The first step from X = 0 is no product: W[r, v] <- T[v] * B[r, v]; one lane per (row, column), striding over the rows.
template <int KW>
__global__ __launch_bounds__(KRY_BS) void k_horner_scale(int n, int kc, ZpField F, int hp, int mhp, const int *__restrict__ T,
                                                         const int *__restrict__ B, i64d ldb, int *__restrict__ Y, i64d ldy,
                                                         long long *__restrict__ cnt)
{
    constexpr int RPB = KRY_BS / KW;
    const int v = threadIdx.x % KW;
    long long t = 0;
    if (v < kc) {
        const int c = T[v];
        for (i64d r = (i64d)blockIdx.x * RPB + threadIdx.x / KW; r < n; r += (i64d)gridDim.x * RPB) {
            const int y = zp_mul(F, c, zp_residue(F, hp, mhp, B[r * ldb + v]));
            Y[r * ldy + v] = y;
            t += y != 0;
        }
    }
    if (cnt) krylov_project<KW>(t, cnt);
}

// the epilogue of a Horner step (spmv_step.hpp): Y[row, v] <- y0 + T[v] * B[row, v] and the term (y != 0) of cnt[v]; counted only
// when cnt is given
struct HornerEpi {
    const int *T, *B;
    i64d ldb;
    long long *cnt;
    __device__ int coef(int v) const { return T[v]; }
    __device__ long long own(const ZpField &F, int hp, int mhp, int c, int row, int v, int y0, int *yp) const
    {
        const int y = zp_axpy(F, c, zp_residue(F, hp, mhp, B[(i64d)row * ldb + v]), y0); // three canonical residues
        *yp = y;
        return y != 0;
    }
    __device__ bool projects() const { return cnt != nullptr; }
    __device__ long long *sums() const { return cnt; }
};
