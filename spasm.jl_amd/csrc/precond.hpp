// precond.hpp -- rank and determinant over GF(p) without elimination on gfx950: the projected Krylov sequences of the diagonally
// preconditioned operators D A (determinant) and E A^T D2 A (rank) of the resident exact product (spasm_amd_wiedemann_rank,
// spasm_amd_wiedemann_det, spasm_amd_precond_sequence).  No fill-in: memory is O(nnz + (n + m) * K).
//
// The preconditioned step is k_spmv_step / k_spmv_step_combine of spmv_step.hpp with DiagEpi: the lane that owns y[row, v] stores
// y = zp_mul(d[row], y0), y0 the canonical row sum (for the long rows in the combine), and, when U is given, contributes
// zp_mul(U[row, v], y) to acc[v] of this step (krylov_project).  One step of the rank sequence is two launch sets on the two views
// of the operator: fwd with DiagEpi{d2, no projection} writes the n x KW intermediate D2 A X, tr with DiagEpi{e, U, acc + i * KW}
// writes the next m x KW iterate E A^T (D2 A X) and its projection.  One step of the determinant's sequence is one launch set with
// DiagEpi{d, U, acc + i * KW}.  Term 0 is k_krylov_dot, the finish is k_krylov_finish, the recurrences are k_berlekamp_massey:
// those of krylov.hpp, unchanged.
//
// Bound of the scale: the row sum r is what SPMV_TEAM_SUM leaves: for p < 2^16 the sum of at most 64 canonical residues,
// |r| < 2^21; for larger p the sum of at most 64 i64 accumulators of at most SPMV_SEG lazy terms below 2^31.1, |r| < 2^51.1; in
// the combine the sum of at most 2^31 / SPMV_SEG canonical partial sums, |s| < 2^48.  All are inside the domain of zp_reduce
// (|x| <= min(3 * 2^51 * p, 2^62), p >= 3), which gives the canonical y0.  d[row] is any int32 (the caller's array, or the
// generator's balanced residue) and is canonical after zp_residue, so y = zp_mul(d, y0) takes two canonical residues and is
// canonical: the next product reads canonical X, as every step of krylov.hpp does.
// Bound of the projection: U[row, v] is canonical after zp_residue and y is canonical, so a term zp_mul(u, y) is a canonical
// residue, |term| <= halfp < 2^31; there are at most 2^31 rows, so every partial sum and the total stay below 2^31 * halfp < 2^62
// in an i64: the argument of krylov.hpp, and k_krylov_finish reduces it as there.  Without U the term is 0 and nothing is summed.
// Field operations only (zp_mul, zp_residue): every prime 2 < p <= 0xFFFFFFFB works.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "krylov.hpp"

// the epilogue of a preconditioned step (spmv_step.hpp): Y[row, v] <- d[row] * y0 and, when U is given, the term U[row, v] * y of
// acc[v]
struct DiagEpi {
    const int *d;
    const int *U;
    i64d ldu;
    long long *acc;
    __device__ int coef(int) const { return 0; }
    __device__ long long own(const ZpField &F, int hp, int mhp, int, int row, int v, int y0, int *yp) const
    {
        const int y = zp_mul(F, zp_residue(F, hp, mhp, d[row]), y0); // two canonical residues
        *yp = y;
        return U ? zp_mul(F, zp_residue(F, hp, mhp, U[(i64d)row * ldu + v]), y) : 0;
    }
    __device__ bool projects() const { return U != nullptr; }
    __device__ long long *sums() const { return acc; }
};
