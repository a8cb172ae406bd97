// trsolve.hpp -- exact dense triangular solves x T = b over GF(p) on gfx950, k right-hand sides at once (spasm_dense_forward_solve,
// spasm_dense_back_solve and the resident operator spasm_amd_trsolve_*; reference src/SpaSM.jl:663-692).
//
// T is n x m; participating row i has the pivot column c(i) and the diagonal d(i) = T[i][c(i)].  The pivot graph (i -> k when
// row i has an entry on c(k), k != i) is acyclic; x[k] = d(k)^-1 (b[c(k)] - sum_{i != k} x[i] T[i][c(k)]).  The operator (engine.hip)
// orders the participating rows by topological level once ("positions") and cuts that order into panels:
//   wide panel   one level of >= TRS_WIDE rows: its rows are independent, k_trs_wide_solve takes them in one grid launch;
//   chunk        at most TRS_CHUNK consecutive positions of narrower levels: one workgroup (k_trs_chunk_solve) steps through the
//                chunk's own levels with workgroup barriers, taking the dependencies inside the chunk from its diagonal block
//                D[a][b] = T[row a][c(row b)] (a before b, at most TRS_CHUNK^2 residues) held in LDS.
// After a panel is solved, k_trs_push adds x_panel T[panel rows] into acc[t] = sum x[i] T[i][c(t)] for every later position t
// that the panel touches: the panel's entries are stored gathered by target (descriptor = target, start, length), one team per
// target, so each accumulator has one owner per launch -- no atomics, no waiting between workgroups, results independent of
// scheduling.  Dependencies between panels are kernel boundaries on one stream.  Entries on columns without a pivot are pushed
// once, at the end, by k_trs_residual (gathered by column), which writes the residual b - x T (zero on pivot columns by
// construction) and clears ok[v] when it is not zero.
//
// Accumulator bounds (zp.hpp): every stored residue (T, acc, x) is canonical.  A lazy term is at most p/2 + 256 < 2^15.01 for
// p < 2^16 and below 2^31.1 otherwise.  k_trs_chunk_solve: a row takes at most TRS_CHUNK - 1 = 63 lazy terms on top of a residue,
// |r| < 2^21.1 in i32 (p < 2^16), |r| < 2^37.1 in i64.  k_trs_push / k_trs_residual: a lane folds its i32 accumulator to a
// canonical residue every TRS_FOLD = 16384 terms, so it stays below 2^29.01 (the same bound as k_spmv); the i64 accumulator of
// larger p takes fewer than 2^31 terms of 2^31.1 (a descriptor or a column has fewer than 2^31 entries), so it stays below 2^62.1.
// Every lane reduces its accumulator to a canonical residue before the team sum, so a team sum of at most 64 lanes is below 2^38.
// Inputs need not be reduced: B is reduced where it is read.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "zp.hpp"

constexpr int TRS_WIDE = 256;    // a level with at least this many rows is one panel of its own
constexpr int TRS_CHUNK = 64;    // rows of a chunk (narrow levels); its diagonal block has at most TRS_CHUNK^2 entries
constexpr int TRS_CV = 16;       // vectors per chunk workgroup: TRS_CHUNK x TRS_CV = 1024 lanes
constexpr int TRS_FOLD = 16384;  // lazy terms a lane takes between two reductions of its accumulator
constexpr int TRS_UNROLL = 4;    // entries (and gathers) in flight per lane

// x[pos][v] = d^-1 (b[c(pos)][v] - acc[pos][v]) for the positions beg .. beg + cnt - 1 (one level: independent rows)
__global__ __launch_bounds__(256) void k_trs_wide_solve(int beg, int cnt, const int *__restrict__ pcol, const int *__restrict__ pdinv, ZpField F, int kw,
                                                        int kc, const int *__restrict__ B, i64d ldb, const int *__restrict__ acc, int *__restrict__ xs)
{
    const i64d g = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(g / kc), v = (int)(g % kc);
    if (r >= cnt) return;
    const i64d pos = (i64d)beg + r;
    const int b = zp_reduce(F, (int64_t)B[(i64d)pcol[pos] * ldb + v]);
    xs[pos * kw + v] = zp_mul(F, pdinv[pos], zp_sub(F, b, acc[pos * kw + v]));
}

// One chunk of s <= TRS_CHUNK positions beg .. beg + s - 1, one workgroup per TRS_CV vectors (blockIdx.y).  Lane (a, vl): row a
// of the chunk, vector v = blockIdx.y * TRS_CV + vl.  steps[0 .. nsteps-1]: the ends of the chunk's levels (chunk-relative).
// diag: the s x s block, diag[b * s + a] = T[row b][c(row a)], zero unless b is in an earlier level than a (read only when
// nsteps > 1).
template <bool SMALL>
__global__ __launch_bounds__(TRS_CHUNK *TRS_CV) void k_trs_chunk_solve(int beg, int s, const int *__restrict__ diag, const int *__restrict__ steps, int nsteps,
                                                                      const int *__restrict__ pcol, const int *__restrict__ pdinv, ZpField F, int kw, int kc,
                                                                      const int *__restrict__ B, i64d ldb, const int *__restrict__ acc, int *__restrict__ xs)
{
    typedef typename ZpAcc<SMALL>::type acc_t;
    __shared__ int D[TRS_CHUNK * TRS_CHUNK];
    __shared__ int xl[TRS_CHUNK * TRS_CV];
    __shared__ int st[TRS_CHUNK];
    const int t = threadIdx.x;
    if (nsteps > 1) // one level: no dependency inside the chunk and no block stored
        for (int e = t; e < s * s; e += blockDim.x) D[e] = diag[e];
    if (t < nsteps) st[t] = steps[t];
    const int a = t / TRS_CV, vl = t % TRS_CV;
    const int v = blockIdx.y * TRS_CV + vl;
    const bool live = a < s && v < kc;
    const i64d pos = (i64d)beg + a;
    acc_t r = 0;
    int dinv = 0;
    if (live) {
        const int b = zp_reduce(F, (int64_t)B[(i64d)pcol[pos] * ldb + v]);
        r = zp_sub(F, b, acc[pos * kw + v]);
        dinv = pdinv[pos];
    }
    __syncthreads();
    int s0 = 0;
    for (int q = 0; q < nsteps; q++) {
        const int s1 = st[q];
        if (live && a >= s0 && a < s1) {
            const int x = zp_mul(F, dinv, zp_reduce(F, (int64_t)r));
            xl[a * TRS_CV + vl] = x;
            xs[pos * kw + v] = x;
        }
        __syncthreads(); // xl of this level is complete; each xl slot is written once, so one barrier per level suffices
        if (live && a >= s1) {
            for (int b = s0; b < s1; b++) r -= ZpAcc<SMALL>::mul_lazy(F, D[b * s + a], xl[b * TRS_CV + vl]);
        }
        s0 = s1;
    }
}

// acc[tgt[d]][v] += sum over the entries (srcpos, val) of descriptor d of x[srcpos][v] * val, one team of TEAM lanes per
// descriptor: lane (e, v) takes entries e, e + E, ... (E = TEAM / KW).  Descriptors of one launch have distinct targets.
template <bool SMALL, int KW, int TEAM>
__global__ __launch_bounds__(256) void k_trs_push(int ndesc, const int *__restrict__ tgt, const i64d *__restrict__ start, const int *__restrict__ len,
                                                  const int2 *__restrict__ ent, ZpField F, int kc, const int *__restrict__ xs, int *__restrict__ acc)
{
    static_assert(TEAM % KW == 0 && 64 % TEAM == 0, "team shape");
    constexpr int E = TEAM / KW;
    typedef typename ZpAcc<SMALL>::type acc_t;
    const int it = (int)(((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM);
    if (it >= ndesc) return; // whole teams leave together
    const int tl = threadIdx.x % TEAM;
    const int v = tl % KW, e = tl / KW;
    const bool vok = v < kc;
    const i64d st = start[it];
    const int hi = len[it];
    acc_t sacc = 0;
    int fold = 0;
    for (int k0 = e; k0 < hi; k0 += TRS_UNROLL * E) {
        int2 a[TRS_UNROLL];
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) a[u] = k0 + u * E < hi ? ent[st + k0 + u * E] : make_int2(0, 0);
        int xv[TRS_UNROLL];
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) xv[u] = vok ? xs[(i64d)a[u].x * KW + v] : 0;
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) sacc += ZpAcc<SMALL>::mul_lazy(F, a[u].y, xv[u]);
        if (SMALL && (fold += TRS_UNROLL) >= TRS_FOLD) {
            sacc = zp_reduce(F, (int64_t)sacc);
            fold = 0;
        }
    }
    long long r = zp_reduce(F, (int64_t)sacc);
#pragma unroll
    for (int o = KW; o < TEAM; o <<= 1) r += __shfl_xor(r, o, TEAM);
    if (e != 0 || !vok) return;
    int *ap = acc + (i64d)tgt[it] * KW + v;
    *ap = zp_reduce(F, r + (int64_t)*ap);
}

// B[c][v] <- b - x T on column c: 0 on pivot columns (colpos[c] >= 0), b[c][v] - sum of the column's entries (srcpos, val) times
// x[srcpos][v] elsewhere; a non-zero residual clears ok[v].  One team per column.
template <bool SMALL, int KW, int TEAM>
__global__ __launch_bounds__(256) void k_trs_residual(int m, const int *__restrict__ colpos, const i64d *__restrict__ rstart, const int2 *__restrict__ ent,
                                                      ZpField F, int kc, const int *__restrict__ xs, int *__restrict__ B, i64d ldb,
                                                      unsigned char *__restrict__ ok)
{
    static_assert(TEAM % KW == 0 && 64 % TEAM == 0, "team shape");
    constexpr int E = TEAM / KW;
    typedef typename ZpAcc<SMALL>::type acc_t;
    const int c = (int)(((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM);
    if (c >= m) return;
    const int tl = threadIdx.x % TEAM;
    const int v = tl % KW, e = tl / KW;
    const bool vok = v < kc;
    const bool piv = colpos[c] >= 0;
    const i64d st = rstart[c];
    const int hi = piv ? 0 : (int)(rstart[c + 1] - st);
    acc_t sacc = 0;
    int fold = 0;
    for (int k0 = e; k0 < hi; k0 += TRS_UNROLL * E) {
        int2 a[TRS_UNROLL];
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) a[u] = k0 + u * E < hi ? ent[st + k0 + u * E] : make_int2(0, 0);
        int xv[TRS_UNROLL];
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) xv[u] = vok ? xs[(i64d)a[u].x * KW + v] : 0;
#pragma unroll
        for (int u = 0; u < TRS_UNROLL; u++) sacc += ZpAcc<SMALL>::mul_lazy(F, a[u].y, xv[u]);
        if (SMALL && (fold += TRS_UNROLL) >= TRS_FOLD) {
            sacc = zp_reduce(F, (int64_t)sacc);
            fold = 0;
        }
    }
    long long r = zp_reduce(F, (int64_t)sacc);
#pragma unroll
    for (int o = KW; o < TEAM; o <<= 1) r += __shfl_xor(r, o, TEAM);
    if (e != 0 || !vok) return;
    int *bp = B + (i64d)c * ldb + v;
    const int res = piv ? 0 : zp_sub(F, zp_reduce(F, (int64_t)*bp), zp_reduce(F, r));
    *bp = res;
    if (res != 0) ok[v] = 0; // every writer stores the same byte
}

// X[i][v] <- x of row i (0 on rows without a pivot)
__global__ void k_trs_write_x(int n, const int *__restrict__ rowpos, int kw, int kc, const int *__restrict__ xs, int *__restrict__ X, i64d ldx)
{
    const i64d g = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(g / kc), v = (int)(g % kc);
    if (i >= n) return;
    const int pos = rowpos[i];
    X[(i64d)i * ldx + v] = pos < 0 ? 0 : xs[(i64d)pos * kw + v];
}
