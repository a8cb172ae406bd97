// block_bm.hpp -- Berlekamp-Massey over matrix sequences on gfx950: a left generator F(x) = sum_t F_t x^t of a sequence of b x b
// matrices S_0 .. S_{len-1} over GF(p), b in {2, 4, 8, 16} (spasm_amd_block_berlekamp_massey).
//
// Method: the order-by-order minimal approximant basis (the iterative sigma-basis of Beckermann and Labahn, the M-Basis of
// Giorgi, Jeannerod and Villard, Coppersmith's iteration) of the 2b x b series G(x) = [S(x); I], S(x) = sum_i S_i x^i.  The basis
// has 2b rows [g_i(x) | h_i(x)] of b + b polynomials with g_i S + h_i = 0 mod x^k at order k, and a degree
// delta_i = max(deg g_i, deg h_i + 1).  It starts at order 0 from the identity: rows i < b are [e_i | 0] with delta = 0, rows
// b + i are [0 | e_i] with delta = 1.  Step k:
//   discrepancy   D[i, :] = the coefficient of x^k of g_i S + h_i = sum_t g_i[t] S_{k-t} + h_i[k], a 2b x b matrix;
//   elimination   the rows are taken by (delta, index) ascending.  A row whose D is not zero becomes a pivot at its first non-zero
//                 column c, and c is cleared from every later row j: row j <- row j - (D[j, c] / D[i, c]) row i, in D, g and h
//                 alike.  delta_i <= delta_j, so no degree grows;
//   shift         the pivot rows are multiplied by x, delta <- delta + 1; the other rows now have D = 0.  Order k + 1 holds.
// Only g is kept.  Of h a row needs h_i[k] alone at step k, and since delta_i <= k + 1 there (by induction: a pivot's delta and k
// grow together) h_i[k + 1] is 0 for a row that was no pivot and is the eliminated h_i[k] for a pivot (the shift).  So h lives on
// as the 2b x b matrix hk, which goes through the elimination beside D.
// The row operations of a step are collected as the 2b x 2b matrix T (new row i = x^piv[i] * sum_j T[i, j] * old row j) by the
// one small workgroup that eliminates, and applied to g by a kernel spread over the coefficients, from one buffer of g into the
// other: nothing is read that the same launch writes.  g is stored coefficient-major, word (t, i, c) at (t * 2b + i) * b + c.
//
// Result.  A row of degree delta reversed, f[t] = g[delta - t], annihilates: sum_t f[t] S_{i+t} is the coefficient i + delta of
// g S + h for 0 <= i < len - delta, which is 0 as deg h < delta.  The rows are taken by (delta, index) ascending and a row joins F
// when its g(0) is independent of those already in; g(0) of the basis has rank b (e_r is g(0) of the approximant [e_r | -e_r S]),
// so b rows join and the matrix of leading row coefficients of F, their g(0), is non-singular.
//
// Launches.  A step is three ordinary launches on one stream: k_bbm_disc, k_bbm_elim, k_bbm_update; there is no grid-wide barrier
// and nothing the host waits for.  The host sizes the grids by the bound delta <= k + 1; workgroups above the largest degree
// (device memory, maxdeg) leave at once.
// Accumulator bounds.  In k_bbm_disc a lane takes at most ceil(BBM_CHUNK / slices) * b <= 64 * 16 = 1024 lazy products (ZpAcc):
// for p < 2^16 the i32 accumulator holds zp_lazy_terms(F) >= 65043 of them, whatever len is (so the i32 lazy limit refuses no len;
// the host pins 64 * 16 <= 65043 with a static_assert); for larger p an i64 accumulator below 1024 * 2^31.1.  A workgroup's sum
// is reduced to a canonical residue and added to dacc with one 64-bit integer vector atomic per entry: at most
// len / BBM_CHUNK + 1 workgroups, |sum| < 2^25 * 2^31,
// an integer that does not depend on the order of the additions.  In k_bbm_update a word sums at most 2b <= 32 lazy products.
// Field operations from zp.hpp only: every prime 2 < p <= 0xFFFFFFFB works.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"

constexpr int BBM_CHUNK = 64;  // coefficients of g one workgroup of the discrepancy takes
constexpr int BBM_DISC_BS = 512; // lanes of a discrepancy workgroup: 2 b^2 entries of D times 512 / (2 b^2) slices of the chunk
constexpr int BBM_BS = 256;    // lanes of the other kernels

// the state of one run in device memory
struct BbmState {
    int *g[2];          // the two buffers of g: (len + 2) * 2b * b words each, zero above a row's degree
    long long *dacc;    // 2b * b sums of the discrepancy, zero between steps
    int *hk;            // 2b * b: h_i[k]
    int *T;             // 2b * 2b: the row operations of the step
    int *deg;           // 2b
    int *piv;           // 2b: 1 where the row was a pivot of the step
    int *maxdeg;        // the largest degree
    int *sel;           // b: the rows of the basis that make F
};

template <int B> __global__ void k_bbm_init(BbmState st)
{
    const int tid = threadIdx.x;
    for (int e = tid; e < 2 * B * B; e += blockDim.x) {
        const int i = e / B, c = e % B;
        st.g[0][e] = (i < B && i == c) ? 1 : 0;
        st.hk[e] = (i >= B && i - B == c) ? 1 : 0;
        st.dacc[e] = 0;
    }
    for (int i = tid; i < 2 * B; i += blockDim.x) st.deg[i] = i < B ? 0 : 1;
    if (tid == 0) *st.maxdeg = 1;
}

// dacc[i * B + c] += sum over the chunk's t of sum_r g[t][i][r] * S[k - t][r][c]
template <bool SMALL, int B>
__global__ __launch_bounds__(BBM_DISC_BS) void k_bbm_disc(int k, ZpField F, const int *__restrict__ S, const int *__restrict__ g,
                                                          const int *__restrict__ maxdeg, long long *__restrict__ dacc)
{
    constexpr int O = 2 * B * B, SL = BBM_DISC_BS / O;
    __shared__ long long s_part[BBM_DISC_BS];
    const int t0 = blockIdx.x * BBM_CHUNK, md = *maxdeg;
    if (t0 > md) return; // the whole workgroup: g is zero up there
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp;
    const int tid = threadIdx.x, o = tid % O, sl = tid / O, i = o / B, c = o % B;
    const int tend = min(min(t0 + BBM_CHUNK, k + 1), md + 1);
    typename ZpAcc<SMALL>::type acc = 0;
    // (unrolled further, the i32 class keeps every product of a coefficient in flight: 256 VGPRs and scratch at B = 16)
#pragma unroll 1
    for (int t = t0 + sl; t < tend; t += SL) {
        const int *p = g + ((i64d)t * 2 * B + i) * B;
        const int *s = S + (i64d)(k - t) * B * B + c;
#pragma unroll 4
        for (int r = 0; r < B; r++) acc += ZpAcc<SMALL>::mul_lazy(F, p[r], zp_residue(F, hp, mhp, s[r * B]));
    }
    long long v = SMALL ? (long long)zp_reduce(F, (int64_t)acc) : (long long)acc;
    if (SL > 1) {
        s_part[tid] = v;
        __syncthreads();
        if (sl != 0) return;
        for (int q = 1; q < SL; q++) v += s_part[q * O + o];
    }
    const int w = zp_reduce(F, (int64_t)v);
    if (w != 0) atomicAdd((unsigned long long *)(dacc + o), (unsigned long long)(long long)w);
}

// Fixed-order elimination of the R x B matrix D in LDS (rows by ord[0 .. R)): a row that is not zero becomes a pivot at its first
// non-zero column, which is cleared from the later rows; the same operations go to the NX extra words of each row in X (row
// stride NX).  pv[i] <- 1 for a pivot.  Stops after `want` pivots.  Every lane of the workgroup calls it; returns the pivots.
template <int B, int R, int NX>
__device__ int bbm_eliminate(const ZpField &F, int *D, int *X, const int *ord, int *pv, int *fm, int *sel, int want)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    int npiv = 0;
    for (int s = 0; s < R && npiv < want; s++) {
        const int i = ord[s];
        int pc = -1;
        for (int c = 0; c < B; c++)
            if (D[i * B + c] != 0) { pc = c; break; }
        if (pc < 0) continue; // the same for every lane: D[i] is as the last barrier left it
        const int inv = zp_inverse(F, D[i * B + pc]);
        if (tid == 0) { pv[i] = 1; if (sel) sel[npiv] = i; }
        npiv++;
        // the multipliers of the later rows, then the rows
        for (int s2 = s + 1 + tid; s2 < R; s2 += nt) {
            const int v = D[ord[s2] * B + pc];
            fm[s2] = v == 0 ? 0 : zp_neg(F, zp_mul(F, v, inv));
        }
        __syncthreads();
        constexpr int W = B + NX;
        for (int e = tid; e < (R - s - 1) * W; e += nt) {
            const int s2 = s + 1 + e / W, w = e % W, f = fm[s2];
            if (f == 0) continue;
            const int j = ord[s2];
            if (w < B) D[j * B + w] = w == pc ? 0 : zp_axpy(F, f, D[i * B + w], D[j * B + w]);
            else X[j * NX + (w - B)] = zp_axpy(F, f, X[i * NX + (w - B)], X[j * NX + (w - B)]);
        }
        __syncthreads();
    }
    return npiv;
}

// ord[rank of i by (dg[i], i)] <- i for the first R lanes
template <int R> __device__ void bbm_order(const int *dg, int *ord)
{
    const int i = threadIdx.x;
    if (i < R) {
        int rank = 0;
        for (int j = 0; j < R; j++) rank += (dg[j] < dg[i] || (dg[j] == dg[i] && j < i)) ? 1 : 0;
        ord[rank] = i;
    }
}

// one workgroup: D <- dacc + hk, the elimination, T, hk, deg, piv and maxdeg of the step; dacc <- 0
template <int B> __global__ __launch_bounds__(BBM_BS) void k_bbm_elim(ZpField F, BbmState st)
{
    constexpr int R = 2 * B, NX = B + R; // beside D a row carries its hk (B words) and its row of T (R words)
    __shared__ int D[R * B], X[R * NX], dg[R], ord[R], pv[R], fm[R];
    const int tid = threadIdx.x;
    for (int e = tid; e < R * B; e += BBM_BS) {
        const int h = st.hk[e];
        D[e] = zp_reduce(F, (int64_t)st.dacc[e] + (int64_t)h);
        st.dacc[e] = 0;
        X[(e / B) * NX + e % B] = h;
    }
    for (int e = tid; e < R * R; e += BBM_BS) X[(e / R) * NX + B + e % R] = (e / R == e % R) ? 1 : 0;
    if (tid < R) { dg[tid] = st.deg[tid]; pv[tid] = 0; }
    __syncthreads();
    bbm_order<R>(dg, ord);
    __syncthreads();
    bbm_eliminate<B, R, NX>(F, D, X, ord, pv, fm, nullptr, B);
    __syncthreads();
    for (int e = tid; e < R * B; e += BBM_BS) st.hk[e] = pv[e / B] ? X[(e / B) * NX + e % B] : 0;
    for (int e = tid; e < R * R; e += BBM_BS) st.T[e] = X[(e / R) * NX + B + e % R];
    if (tid < R) {
        st.deg[tid] = dg[tid] + pv[tid];
        st.piv[tid] = pv[tid];
    }
    if (tid == 0) {
        int m = 0;
        for (int i = 0; i < R; i++) m = max(m, dg[i] + pv[i]);
        *st.maxdeg = m;
    }
}

// gn[t][i][c] <- sum_j T[i, j] * go[t - piv[i]][j][c] for 0 <= t <= k + 1; one lane per word
template <bool SMALL, int B>
__global__ __launch_bounds__(BBM_BS) void k_bbm_update(int k, ZpField F, const int *__restrict__ go, int *__restrict__ gn, const int *__restrict__ T,
                                                       const int *__restrict__ piv, const int *__restrict__ maxdeg)
{
    constexpr int R = 2 * B;
    __shared__ int sT[R * R], sp[R];
    const i64d e0 = (i64d)blockIdx.x * BBM_BS;
    // A workgroup whose words all lie above the largest degree (the new one: k_bbm_elim has written it) leaves without writing.
    // Those words of gn are zero already: gn was last written two steps ago, up to the largest degree of that step, and maxdeg
    // never decreases (a degree only grows), so whatever a buffer holds that is not zero lies at t <= maxdeg, where this launch
    // overwrites every word; above it both buffers still hold the zeros of the memset before the first step.
    if (e0 / (R * B) > *maxdeg) return;
    for (int e = threadIdx.x; e < R * R; e += BBM_BS) sT[e] = T[e];
    if (threadIdx.x < R) sp[threadIdx.x] = piv[threadIdx.x];
    __syncthreads();
    const i64d e = e0 + threadIdx.x;
    const int t = (int)(e / (R * B)), i = (int)(e / B % R), c = (int)(e % B);
    if (t > k + 1) return;
    const int ts = t - sp[i];
    typename ZpAcc<SMALL>::type acc = 0;
    if (ts >= 0) {
        const int *src = go + (i64d)ts * R * B + c;
        for (int j = 0; j < R; j++) {
            const int f = sT[i * R + j];
            if (f != 0) acc += ZpAcc<SMALL>::mul_lazy(F, f, src[j * B]);
        }
    }
    gn[e] = zp_reduce(F, (int64_t)acc);
}

// one workgroup: the b rows of F by (degree, index) with independent g(0); rowdeg, dmax
template <int B> __global__ __launch_bounds__(BBM_BS) void k_bbm_select(ZpField F, BbmState st, const int *__restrict__ g, int *__restrict__ rowdeg, int *__restrict__ dmax)
{
    constexpr int R = 2 * B;
    __shared__ int D[R * B], X[R], dg[R], ord[R], pv[R], fm[R], sl[B];
    const int tid = threadIdx.x;
    for (int e = tid; e < R * B; e += BBM_BS) D[e] = g[e];
    if (tid < R) { dg[tid] = st.deg[tid]; pv[tid] = 0; X[tid] = 0; }
    if (tid < B) sl[tid] = 0;
    __syncthreads();
    bbm_order<R>(dg, ord);
    __syncthreads();
    bbm_eliminate<B, R, 1>(F, D, X, ord, pv, fm, sl, B);
    __syncthreads();
    if (tid < B) {
        st.sel[tid] = sl[tid];
        rowdeg[tid] = dg[sl[tid]];
    }
    if (tid == 0) {
        int m = 0;
        for (int r = 0; r < B; r++) m = max(m, dg[sl[r]]);
        *dmax = m;
    }
}

// coef[(t * B + r) * B + c] <- g[delta_r - t][sel[r]][c] for t <= delta_r, else 0; 0 <= t <= len
template <int B>
__global__ __launch_bounds__(BBM_BS) void k_bbm_write(i64d total, const int *__restrict__ g, const int *__restrict__ sel, const int *__restrict__ rowdeg,
                                                      int *__restrict__ coef)
{
    const i64d e = (i64d)blockIdx.x * BBM_BS + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e / (B * B)), r = (int)(e / B % B), c = (int)(e % B);
    const int d = rowdeg[r];
    coef[e] = t <= d ? g[((i64d)(d - t) * 2 * B + sel[r]) * B + c] : 0;
}
