// spmv_step.hpp -- one step Y <- A X of an iteration with the resident exact product over GF(p) on gfx950, with an epilogue on
// every finished entry of Y: the kernels behind the projected Krylov sequence (krylov.hpp, KrylovEpi) and behind Horner's rule
// (horner.hpp, HornerEpi).
//
// The row sum is SPMV_TEAM_SUM of spmv.hpp, on the same row classes and entry streams as k_spmv (SpmvView: short, medium, long in
// segments of SPMV_SEG), and its bounds are argued there.  What differs from k_spmv: Y is written and never read, so there is no
// memset and no read-modify-write.  The grid is capped at KRY_WG_PER_CU workgroups per CU and a team strides over the work items of
// its class.  And the lane that owns y[row, v] hands the canonical row sum to the epilogue, which stores y and returns a term of an
// integer sum per column (a projection, a count).  That sum is taken first over the rows the lane's team walks, then over the
// lanes of the wave that hold column v (shuffles), then over the waves of the workgroup (LDS), and then ONE 64-bit integer add per
// (workgroup, column) goes to global memory (a vector atomic; skipped when the sum is 0): krylov_project.  It is an integer, so it
// does not depend on the order in which lanes, waves, workgroups and atomics add, and two runs give the same bits.  For the long
// rows y is complete only in the combine kernel, so the epilogue runs there and the segment launch never consults it.
//
// An epilogue is a trivially copyable struct passed by value:
//   int  coef(int v) const            what the lane keeps for its column over all its rows (read once, before the loop);
//   long long own(F, hp, mhp, c, row, v, y0, yp) const
//                                     y0 is the canonical (A X)[row, v] and c = coef(v): stores the entry at yp, returns its term;
//   bool projects() const             whether the terms are summed at all;
//   long long *sums() const           where: KW words, |sum| < 2^62.
// An epilogue that returns B > 1 terms per entry (the b x b projection of block_krylov.hpp) names B in EpiTerms and has instead
//   void own(F, hp, mhp, row, v, y0, yp, long long (&t)[B]) const
//                                     stores the entry at yp and adds its B terms to t[0 .. B);
//   template <int KW> void project(long long (&t)[B]) const
//                                     sums t over the workgroup and adds the sums to global memory (every lane calls it).
// The one-term epilogues do not name EpiTerms and compile to what they compiled to before it existed: the branch is taken at
// compile time (profiles/block_wiedemann_asm_diff.txt).
// A one-term epilogue whose lane keeps more than one word for its column (the B coefficients of block_horner.hpp) names the
// trivially copyable type in EpiCoef: coef(v) returns it, own takes it as c, and a lane that owns nothing holds its zero value.
// The others do not name EpiCoef, their c is the int it was, and they compile to what they compiled to before
// (profiles/block_solve_asm_diff.txt).
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "spmv.hpp"

constexpr int KRY_BS = 256;                  // lanes of a workgroup of the step kernels (KW divides it)
constexpr int KRY_WG_PER_CU = 8;             // the grid of a step is capped at this many workgroups per CU

// The workgroup's sum of t over the lanes of each column (the column of a lane is threadIdx.x % KW, KW a power of two that divides
// 64) is added to accp[column].  Every lane of the workgroup calls it, with t = 0 where it owns nothing.  |t| < 2^62.
template <int KW> __device__ __forceinline__ void krylov_project(long long t, long long *accp)
{
    constexpr int NW = KRY_BS / 64;
    __shared__ long long s_red[NW * KW];
#pragma unroll
    for (int o = KW; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < KW) s_red[wave * KW + lane] = t;
    __syncthreads();
    if (threadIdx.x < KW) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += s_red[w * KW + threadIdx.x];
        if (s != 0) atomicAdd((unsigned long long *)(accp + threadIdx.x), (unsigned long long)s);
    }
}

// the terms an epilogue returns per entry of Y: 1 unless it says otherwise
template <class Epi> struct EpiTerms { static constexpr int value = 1; };

// what a lane keeps for its column over all its rows, the result of coef(v): an int unless the epilogue says otherwise
template <class Epi> struct EpiCoef { typedef int type; };

// One team of TEAM lanes per work item (SPMV_TEAM_SUM); a team strides over the items of its class.  Not PARTIAL: the epilogue
// gets the row's sum.  PARTIAL: part[it * KW + v] <- the segment's sum, no epilogue.
template <bool SMALL, int KW, int TEAM, bool PARTIAL, class Epi>
__global__ __launch_bounds__(KRY_BS) void k_spmv_step(int nitems, const int *__restrict__ items, const int *__restrict__ segbeg,
                                                      const i64d *__restrict__ start, const int *__restrict__ len, const int2 *__restrict__ ent,
                                                      ZpField F, int hp, int mhp, int kc, const int *__restrict__ X, i64d ldx, int *__restrict__ Y,
                                                      i64d ldy, int *__restrict__ part, Epi epi)
{
    constexpr int TPB = KRY_BS / TEAM;
    constexpr int NT = EpiTerms<Epi>::value;
    const SpmvLane<KW, TEAM> L(kc);
    if constexpr (PARTIAL || NT == 1) {
        // (a segment launch never consults the epilogue, of either kind)
        typedef typename EpiCoef<Epi>::type Coef;
        Coef c = Coef();
        if constexpr (!PARTIAL) c = L.vok ? epi.coef(L.v) : Coef();
        long long t = 0;
        // whole teams leave the loop together: the shuffles stay inside a team
        for (i64d it = (i64d)blockIdx.x * TPB + threadIdx.x / TEAM; it < nitems; it += (i64d)gridDim.x * TPB) {
            SPMV_TEAM_SUM(row, r, it);
            if (L.e == 0 && L.vok) {
                const int y0 = zp_reduce(F, (int64_t)r);
                if constexpr (PARTIAL) part[it * KW + L.v] = y0;
                else t += epi.own(F, hp, mhp, c, row, L.v, y0, Y + (i64d)row * ldy + L.v);
            }
        }
        if constexpr (!PARTIAL)
            if (epi.projects()) krylov_project<KW>(t, epi.sums());
    } else {
        long long t[NT] = {};
        for (i64d it = (i64d)blockIdx.x * TPB + threadIdx.x / TEAM; it < nitems; it += (i64d)gridDim.x * TPB) {
            SPMV_TEAM_SUM(row, r, it);
            if (L.e == 0 && L.vok) epi.own(F, hp, mhp, row, L.v, zp_reduce(F, (int64_t)r), Y + (i64d)row * ldy + L.v, t);
        }
        epi.template project<KW>(t);
    }
}

// the long rows: row rows[l] owns the segments off[l] .. off[l+1]-1; one lane per (row, column); y is complete here, so the
// epilogue runs here
template <int KW, class Epi>
__global__ __launch_bounds__(KRY_BS) void k_spmv_step_combine(int nlong, const int *__restrict__ rows, const int *__restrict__ off,
                                                              const int *__restrict__ part, int kc, ZpField F, int hp, int mhp,
                                                              int *__restrict__ Y, i64d ldy, Epi epi)
{
    constexpr int RPB = KRY_BS / KW;
    constexpr int NT = EpiTerms<Epi>::value;
    const int v = threadIdx.x % KW;
    if constexpr (NT == 1) {
        long long t = 0;
        if (v < kc) {
            const typename EpiCoef<Epi>::type c = epi.coef(v);
            for (i64d l = (i64d)blockIdx.x * RPB + threadIdx.x / KW; l < nlong; l += (i64d)gridDim.x * RPB) {
                int64_t s = 0; // |s| <= (2^31 / SPMV_SEG) * 2^31 < 2^48: exact
                for (int it = off[l]; it < off[l + 1]; it++) s += part[(i64d)it * KW + v];
                const int row = rows[l];
                t += epi.own(F, hp, mhp, c, row, v, zp_reduce(F, s), Y + (i64d)row * ldy + v);
            }
        }
        if (epi.projects()) krylov_project<KW>(t, epi.sums());
    } else {
        long long t[NT] = {};
        if (v < kc) {
            for (i64d l = (i64d)blockIdx.x * RPB + threadIdx.x / KW; l < nlong; l += (i64d)gridDim.x * RPB) {
                int64_t s = 0; // as above
                for (int it = off[l]; it < off[l + 1]; it++) s += part[(i64d)it * KW + v];
                const int row = rows[l];
                epi.own(F, hp, mhp, row, v, zp_reduce(F, s), Y + (i64d)row * ldy + v, t);
            }
        }
        epi.template project<KW>(t);
    }
}
