// horner.hpp -- a polynomial of the resident exact product applied to vectors over GF(p) on gfx950, one Horner step per launch
// round: Y[row, v] <- (A X)[row, v] + T[v] * B[row, v] (spasm_amd_poly_apply, spasm_amd_wiedemann_solve).
//
// The Horner step.  k_horner_step is k_krylov_step on the same row classes and entry streams (SpmvView: short, medium, long in
// segments of SPMV_SEG), with the same grid cap and team striding.  Y is written and never read.  T is the KW-wide row of this
// step in a device table of canonical residues (the host reduces the coefficients; steps x KW words, uploaded once per call); a
// column whose polynomial has a lower degree has zeros at the top of the table and stays 0 until its leading coefficient arrives,
// because A 0 + 0 b = 0.  Entries of B and of the first X (the caller's arrays) are reduced where they are read (krylov_residue).
// For the long rows the row sum is complete only in k_horner_combine, so T * B enters there.
//
// Bound of the combination: the row sum r is what k_krylov_step has before its last reduction: for p < 2^16 the sum of at most 64
// canonical residues, |r| < 2^21; for larger p the sum of at most 64 i64 accumulators of at most SPMV_SEG lazy terms below 2^31.1,
// |r| < 2^51.1; in the combine the sum of at most 2^31 / SPMV_SEG canonical partial sums, |s| < 2^48.  All are inside the domain
// of zp_reduce (|x| <= min(3 * 2^51 * p, 2^62), p >= 3), which gives the canonical y0.  T[v] is canonical (host), b is canonical
// after krylov_residue, so y = zp_axpy(T[v], b, y0) takes three canonical residues: the domain tests/test_gpu_zp.py pins.
// Field operations only: every prime 2 < p <= 0xFFFFFFFB works.
//
// Counting (cnt != nullptr): the lane that owns y[row, v] contributes (y != 0) to cnt[v], reduced through krylov_project: lanes,
// then waves, then one 64-bit vector atomic per (workgroup, column).  A count is at most the number of rows, < 2^31, far inside
// krylov_project's |t| < 2^62; it is an integer sum, so it does not depend on scheduling.  cnt[v] == 0 says column v of Y is zero.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "zp.hpp"
#include "spmv.hpp"
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
            const int y = zp_mul(F, c, krylov_residue(F, hp, mhp, B[r * ldb + v]));
            Y[r * ldy + v] = y;
            t += y != 0;
        }
    }
    if (cnt) krylov_project<KW>(t, cnt);
}

// One team of TEAM lanes per work item, as in k_krylov_step.  Not PARTIAL: Y[row, v] <- the row's sum + T[v] * B[row, v] (Y is
// not read).  PARTIAL: part[it * KW + v] <- the segment's sum; T and B wait for the combine.
template <bool SMALL, int KW, int TEAM, bool PARTIAL>
__global__ __launch_bounds__(KRY_BS) void k_horner_step(int nitems, const int *__restrict__ items, const int *__restrict__ segbeg,
                                                        const i64d *__restrict__ start, const int *__restrict__ len, const int2 *__restrict__ ent,
                                                        ZpField F, int hp, int mhp, int kc, const int *__restrict__ X, i64d ldx, int *__restrict__ Y,
                                                        i64d ldy, int *__restrict__ part, const int *__restrict__ T, const int *__restrict__ B,
                                                        i64d ldb, long long *__restrict__ cnt)
{
    static_assert(TEAM % KW == 0 && 64 % TEAM == 0, "team shape");
    constexpr int E = TEAM / KW, TPB = KRY_BS / TEAM;
    typedef typename ZpAcc<SMALL>::type acc_t;
    typedef typename std::conditional<SMALL, int, long long>::type sum_t;
    const int tl = threadIdx.x % TEAM;
    const int v = tl % KW, e = tl / KW;
    const bool vok = v < kc;
    const int c = (!PARTIAL && vok) ? T[v] : 0;
    long long t = 0;
    // whole teams leave the loop together: the shuffles stay inside a team
    for (i64d it = (i64d)blockIdx.x * TPB + threadIdx.x / TEAM; it < nitems; it += (i64d)gridDim.x * TPB) {
        const int row = items ? items[it] : (int)it;
        const i64d st = start[row];
        int lo = 0, hi = len[row];
        if (PARTIAL) {
            lo = segbeg[it];
            hi = min(hi, lo + SPMV_SEG);
        }
        acc_t acc = 0;
        for (int k0 = lo + e; k0 < hi; k0 += SPMV_UNROLL * E) {
            int2 a[SPMV_UNROLL];
#pragma unroll
            for (int u = 0; u < SPMV_UNROLL; u++) {
                const int k = k0 + u * E;
                a[u] = k < hi ? ent[st + k] : make_int2(0, 0);
            }
            int xv[SPMV_UNROLL];
#pragma unroll
            for (int u = 0; u < SPMV_UNROLL; u++) xv[u] = (vok && k0 + u * E < hi) ? X[(i64d)a[u].x * ldx + v] : 0;
#pragma unroll
            for (int u = 0; u < SPMV_UNROLL; u++) acc += ZpAcc<SMALL>::mul_lazy(F, a[u].y, krylov_residue(F, hp, mhp, xv[u]));
        }
        sum_t r;
        if (SMALL) r = (sum_t)zp_reduce(F, (int64_t)acc);
        else r = (sum_t)acc;
#pragma unroll
        for (int o = KW; o < TEAM; o <<= 1) r += __shfl_xor(r, o, TEAM);
        if (e == 0 && vok) {
            const int y0 = zp_reduce(F, (int64_t)r); // |r| < 2^51.1 (the header)
            if (PARTIAL) {
                part[it * KW + v] = y0;
            } else {
                const int y = zp_axpy(F, c, krylov_residue(F, hp, mhp, B[(i64d)row * ldb + v]), y0); // three canonical residues
                Y[(i64d)row * ldy + v] = y;
                t += y != 0;
            }
        }
    }
    if (!PARTIAL && cnt) krylov_project<KW>(t, cnt);
}

// the long rows: row rows[l] owns the segments off[l] .. off[l+1]-1; one lane per (row, column); y is complete here
template <int KW>
__global__ __launch_bounds__(KRY_BS) void k_horner_combine(int nlong, const int *__restrict__ rows, const int *__restrict__ off,
                                                           const int *__restrict__ part, int kc, ZpField F, int hp, int mhp, int *__restrict__ Y,
                                                           i64d ldy, const int *__restrict__ T, const int *__restrict__ B, i64d ldb,
                                                           long long *__restrict__ cnt)
{
    constexpr int RPB = KRY_BS / KW;
    const int v = threadIdx.x % KW;
    long long t = 0;
    if (v < kc) {
        const int c = T[v];
        for (i64d l = (i64d)blockIdx.x * RPB + threadIdx.x / KW; l < nlong; l += (i64d)gridDim.x * RPB) {
            int64_t s = 0; // |s| <= (2^31 / SPMV_SEG) * 2^31 < 2^48: exact
            for (int it = off[l]; it < off[l + 1]; it++) s += part[(i64d)it * KW + v];
            const int row = rows[l];
            const int y = zp_axpy(F, c, krylov_residue(F, hp, mhp, B[(i64d)row * ldb + v]), zp_reduce(F, s));
            Y[(i64d)row * ldy + v] = y;
            t += y != 0;
        }
    }
    if (cnt) krylov_project<KW>(t, cnt);
}
