// spmv.hpp -- exact sparse matrix x dense block products over GF(p) on gfx950: Y <- A X + Y (spasm_Axpy, spasm_xApy and the
// resident operator spasm_amd_spmv_*; reference src/SpaSM.jl:640-658).
//
// Both orientations are gather-by-row: x A is computed as A^T x over the device transpose of A, so every output entry is owned
// by one team of lanes, no atomics are used and the result does not depend on scheduling.  A team covers (entry x vector): lane
// (e, v) multiplies entry e, e + E, ... of its row by column v of the gathered row of X, so the KW values a row of X contributes
// are one contiguous read.  Rows are binned by length (host side, once per orientation):
//   short  (len <= SPMV_SHORT):          a team of min(64, 8 KW) lanes per row, several rows per wave;
//   medium (len <= SPMV_SEG):            one wave per row;
//   long   (len >  SPMV_SEG):            one wave per segment of SPMV_SEG entries, each writing its partial sum as a canonical
//                                        residue; k_spmv_combine adds a row's partials as exact i64 integers, then y.
// Accumulator bounds (zp.hpp): a lane takes at most SPMV_SEG = 16384 lazy terms.  For p < 2^16 a lazy term is at most
// p/2 + 256 < 2^15.01 in absolute value, so the i32 accumulator stays below 2^29.01; it is reduced to a canonical residue
// before the team sum (64 lanes x 2^15).  For larger p a term is below 2^31.1 and the i64 accumulator below 2^45.1, the team
// sum below 2^51.1.  Inputs need not be reduced: an entry of X outside [mhalfp, halfp] is reduced where it is gathered, and y
// enters through the final zp_reduce (|sum + y| < 2^52).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "zp.hpp"

constexpr int SPMV_SHORT = 32;    // rows up to this length go to the short-row teams
constexpr int SPMV_SEG = 16384;   // longest row one wave takes whole; longer rows are cut into segments of this length
constexpr int SPMV_UNROLL = 4;    // entries (and gathers) in flight per lane

constexpr int spmv_short_team(int kw) { return kw * 8 < 64 ? kw * 8 : 64; }

// The place of a lane in its team of TEAM lanes: it takes the entries e, e + E, .. (E = TEAM / KW) of the team's row and column v
// of the KW-wide chunk; columns v >= kc are idle.
template <int KW, int TEAM> struct SpmvLane {
    static_assert(TEAM % KW == 0 && 64 % TEAM == 0, "team shape");
    int v, e;
    bool vok;
    __device__ __forceinline__ SpmvLane(int kc) : v(threadIdx.x % TEAM % KW), e(threadIdx.x % TEAM / KW), vok(v < kc) {}
};

template <bool SMALL> using spmv_sum_t = typename std::conditional<SMALL, int, long long>::type;

// The row sum of one work item, the ONE gather loop of the resident product: k_spmv below and the step kernels of spmv_step.hpp
// (Krylov, Horner) are shells around it, and the accumulator bounds above are those of this loop.  Work item it is row items[it]
// (items == nullptr: row it), taken whole, or with PARTIAL its segment [segbeg[it], segbeg[it] + SPMV_SEG).  SPMV_TEAM_SUM(row, r, it)
// declares row and r in the scope of the kernel that names it: r is the team's sum for the lane's column, congruent to
// (A X)[row, v] and inside the domain of zp_reduce, not yet reduced; every lane of the team gets it.  A whole team comes here or
// none does: the shuffles stay inside a team.  It reads the kernel's own SMALL, KW, TEAM, PARTIAL, its view arguments (items,
// segbeg, start, len, ent), F, hp, mhp, X, ldx and its SpmvLane L.
// Besides row and r it leaves E, st, lo, hi and acc in that scope: a kernel that takes it uses those names for nothing else, and
// takes it once (a block around it would hide them, but the whole-row k_spmv then compile to other registers than before).
// It is text and not a function on purpose.  A function is optimised on its own before it is inlined, and the compiler then
// factors the four lazy terms of the loop differently (one v_mul_lo_u32 where there were four v_mul_i32_i24) and the segment
// kernels take 1-2 more VGPRs; as text every kernel compiles to the instructions it had when it carried its own copy of the loop.
#define SPMV_TEAM_SUM(row, r, it)                                                                                        \
    constexpr int E = TEAM / KW;                                                                                         \
    const int row = items ? items[it] : (int)it;                                                                         \
    const i64d st = start[row];                                                                                          \
    int lo = 0, hi = len[row];                                                                                           \
    if (PARTIAL) {                                                                                                       \
        lo = segbeg[it];                                                                                                 \
        hi = min(hi, lo + SPMV_SEG);                                                                                     \
    }                                                                                                                    \
    typename ZpAcc<SMALL>::type acc = 0;                                                                                 \
    for (int k0 = lo + L.e; k0 < hi; k0 += SPMV_UNROLL * E) {                                                            \
        int2 a[SPMV_UNROLL];                                                                                             \
        _Pragma("unroll") for (int u = 0; u < SPMV_UNROLL; u++) {                                                        \
            const int k = k0 + u * E;                                                                                    \
            a[u] = k < hi ? ent[st + k] : make_int2(0, 0);                                                               \
        }                                                                                                                \
        int xv[SPMV_UNROLL];                                                                                             \
        _Pragma("unroll") for (int u = 0; u < SPMV_UNROLL; u++)                                                          \
            xv[u] = (L.vok && k0 + u * E < hi) ? X[(i64d)a[u].x * ldx + L.v] : 0;                                        \
        _Pragma("unroll") for (int u = 0; u < SPMV_UNROLL; u++)                                                          \
            acc += ZpAcc<SMALL>::mul_lazy(F, a[u].y, zp_residue(F, hp, mhp, xv[u]));                                     \
    }                                                                                                                    \
    spmv_sum_t<SMALL> r;                                                                                                 \
    if (SMALL) r = zp_reduce(F, (int64_t)acc);                                                                           \
    else r = acc;                                                                                                        \
    _Pragma("unroll") for (int o = KW; o < TEAM; o <<= 1) r += __shfl_xor(r, o, TEAM)

// One team of TEAM lanes per work item (SPMV_TEAM_SUM).  PARTIAL: the segment's sum goes to part[it * KW + v]; otherwise
// Y[row * ldy + v] <- sum + Y[row * ldy + v].
template <bool SMALL, int KW, int TEAM, bool PARTIAL>
__global__ __launch_bounds__(256) void k_spmv(int nitems, const int *__restrict__ items, const int *__restrict__ segbeg,
                                              const i64d *__restrict__ start, const int *__restrict__ len, const int2 *__restrict__ ent, ZpField F,
                                              int hp, int mhp, int kc, const int *__restrict__ X, i64d ldx, int *__restrict__ Y, i64d ldy,
                                              int *__restrict__ part)
{
    const int it = (int)(((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM);
    if (it >= nitems) return; // whole teams leave together
    const SpmvLane<KW, TEAM> L(kc);
    SPMV_TEAM_SUM(row, r, it);
    if (L.e != 0 || !L.vok) return;
    if (PARTIAL) {
        part[(i64d)it * KW + L.v] = zp_reduce(F, (int64_t)r);
    } else {
        int *yp = Y + (i64d)row * ldy + L.v;
        *yp = zp_reduce(F, (int64_t)r + (int64_t)*yp);
    }
}

// the long rows: row rows[l] owns the segments off[l] .. off[l+1]-1 of k_spmv<.., PARTIAL>; one lane per (row, column)
__global__ void k_spmv_combine(int nlong, const int *__restrict__ rows, const int *__restrict__ off, const int *__restrict__ part, int kw, int kc,
                               ZpField F, int *__restrict__ Y, i64d ldy)
{
    const i64d g = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = (int)(g / kw), v = (int)(g % kw);
    if (l >= nlong || v >= kc) return;
    int64_t s = 0; // |s| <= (2^31 / SPMV_SEG) * 2^31 < 2^48: exact
    for (int it = off[l]; it < off[l + 1]; it++) s += part[(i64d)it * kw + v];
    int *yp = Y + (i64d)rows[l] * ldy + v;
    *yp = zp_reduce(F, s + (int64_t)*yp);
}

// transposed view: row lengths from the row pointers of the device transpose
__global__ void k_spmv_len_from_ptr(int n, const i64d *__restrict__ p, int *__restrict__ len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) len[i] = (int)(p[i + 1] - p[i]);
}
