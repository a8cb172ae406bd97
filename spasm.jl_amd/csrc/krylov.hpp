// krylov.hpp -- the black-box route to spectral invariants over GF(p) on gfx950: projected Krylov sequences s_i = u^T A^i v of the
// resident exact product (spmv.hpp), and their shortest linear recurrences by Berlekamp-Massey (spasm_amd_krylov_sequence,
// spasm_amd_berlekamp_massey, spasm_amd_minpoly).  No elimination, no fill-in: memory is O(nnz + n * K).
//
// The Krylov step is k_spmv_step / k_spmv_step_combine of spmv_step.hpp with KrylovEpi: the lane that owns y[row, v] stores y and
// contributes zp_mul(u[row, v], y), a canonical residue, to acc[v] of this step (krylov_project; for the long rows in the combine).
//
// Bound of the projection: a term is a canonical residue, |term| <= halfp < 2^31, and there are at most 2^31 rows, so every
// partial sum and the total stay below 2^31 * halfp < 2^62 in an i64.  k_krylov_finish brings the sum to the balanced residue with
// zp_reduce, whose float quotient is within 1 because |sum| / p <= 2^30.  The bounds of the product itself are those of spmv.hpp
// (a lane takes at most SPMV_SEG lazy terms).  Unreduced entries of U and of the first X (the caller's V) are reduced where they
// are read (zp_residue).
//
// Berlekamp-Massey.  One workgroup of BM_BS lanes per sequence.  The connection polynomial C and the previous one B are two arrays
// of dmax + 1 words (dmax = len: L never exceeds the number of terms read), in LDS when 2 * (dmax + 1) <= BM_LDS_WORDS (158 KiB of
// the 160 KiB a workgroup may take on gfx950; the rest is for s_sum and whatever the compiler adds), else in device memory, by the
// same device code.  Invariant: every word above an array's degree is zero.  Step i:
//   discrepancy  d = sum_{j <= L} C[j] * s[i - j]: lane t takes j = t, t + BM_BS, .. with lazy products (ZpAcc), reduces its own
//                sum, the wave adds by shuffles, the workgroup through s_sum (two halves used in turn: one barrier).  A lane takes
//                ceil((L + 1) / BM_BS) lazy terms: for p < 2^16 the i32 accumulator holds zp_lazy_terms(F) >= 65043 of them, which
//                allows len <= 65043 * 512 (the host refuses more); for larger p the i64 accumulator is no limit (2^31.1 a term).
//                The sequence is read from global memory; a term outside [mhalfp, halfp] is reduced where it is read.
//   d == 0       m <- m + 1, nothing else, no second barrier.
//   2 L > i      C[k] <- C[k] - (d / b) * B[k - m] for m <= k <= deg B + m (<= L): a lane reads and writes its own words of C only.
//   2 L <= i     the length changes to i + 1 - L and B must become the old C.  Nothing is copied: the new C is written INTO the array
//                of B, newC[k] = C[k] - (d / b) * B[k - m] for 0 <= k <= i + 1 - L, and the two pointers are swapped.  The word
//                B[k - m] a lane reads is a word another lane overwrites, so the chunks of BM_BS words are taken from the TOP down
//                and every chunk reads, passes a barrier, then writes: a chunk writes [base, base + BM_BS), all chunks after it read
//                below base, and its own reads are done before its barrier.  Then b <- d with ONE field inverse, m <- 1.
//   barrier      after either update, before the next discrepancy reads C.
// Field operations only (zp_mul, zp_axpy, zp_inverse): every prime 2 < p <= 0xFFFFFFFB works.  The output is the monic
// f(x) = x^L * C(1 / x), f[k] = C[L - k]: the zero sequence gives f = 1, the sequence 1, 0, 0, 0 gives f = x.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "spmv_step.hpp"

constexpr int BM_BS = 512;                   // lanes of a Berlekamp-Massey workgroup
constexpr int BM_LDS_WORDS = 158 * 1024 / 4; // words C and B may take in LDS: 2 * (dmax + 1) <= 40448, dmax <= 20223

// s_0: accp[v] += sum_r U[r, v] * X[r, v]; one lane per (row, column), striding over the rows
template <int KW>
__global__ __launch_bounds__(KRY_BS) void k_krylov_dot(int n, int kc, ZpField F, int hp, int mhp, const int *__restrict__ U, i64d ldu,
                                                       const int *__restrict__ X, i64d ldx, long long *__restrict__ accp)
{
    constexpr int RPB = KRY_BS / KW;
    const int v = threadIdx.x % KW;
    long long t = 0;
    if (v < kc)
        for (i64d r = (i64d)blockIdx.x * RPB + threadIdx.x / KW; r < n; r += (i64d)gridDim.x * RPB)
            t += zp_mul(F, zp_residue(F, hp, mhp, U[r * ldu + v]), zp_residue(F, hp, mhp, X[r * ldx + v]));
    krylov_project<KW>(t, accp);
}

// the epilogue of a Krylov step (spmv_step.hpp): Y[row, v] <- y and the term U[row, v] * y of acc[v]; always projected
struct KrylovEpi {
    const int *U;
    i64d ldu;
    long long *acc;
    __device__ int coef(int) const { return 0; }
    __device__ long long own(const ZpField &F, int hp, int mhp, int, int row, int v, int y, int *yp) const
    {
        *yp = y;
        return zp_mul(F, zp_residue(F, hp, mhp, U[(i64d)row * ldu + v]), y);
    }
    __device__ bool projects() const { return true; }
    __device__ long long *sums() const { return acc; }
};

// S[i * k + c] <- the balanced residue of acc[i * kw + c]
__global__ void k_krylov_finish(i64d total, int k, int kw, ZpField F, const long long *__restrict__ acc, int *__restrict__ S)
{
    const i64d g = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    S[g] = zp_reduce(F, (int64_t)acc[(g / k) * kw + g % k]);
}

struct BmArgs {
    ZpField F;
    int len;          // terms of a sequence; also dmax, the degree bound of C and B
    const int *S;     // sequence c is S[c], S[lds + c], ..
    i64d lds;
    int *coef;        // f of sequence c: coef[c * ldc ..], ldc >= len + 1 words, zero above the degree
    i64d ldc;
    int *deg;
    int *gwork;       // the device-memory class: 2 * (len + 1) words per sequence
};

template <bool SMALL, bool LDS>
__global__ __launch_bounds__(BM_BS) void k_berlekamp_massey(BmArgs a)
{
    extern __shared__ int s_bm[];
    __shared__ long long s_sum[2][BM_BS / 64];
    typedef typename ZpAcc<SMALL>::type acc_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, len = a.len, dmax = a.len, words = dmax + 1;
    const ZpField F = a.F;
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp;
    int *P = LDS ? s_bm : a.gwork + (i64d)c * 2 * words;   // C
    int *Q = P + words;                                    // B
    const int *s = a.S + c;
    for (int k = tid; k < 2 * words; k += BM_BS) P[k] = (k == 0 || k == words) ? 1 : 0;
    __syncthreads();
    int L = 0, LB = 0, m = 1, binv = 1, par = 0;
    for (int i = 0; i < len; i++) {
        // ---- discrepancy
        acc_t acc = 0;
        for (int j = tid; j <= L; j += BM_BS) acc += ZpAcc<SMALL>::mul_lazy(F, P[j], zp_residue(F, hp, mhp, s[(i64d)(i - j) * a.lds]));
        long long r;
        if (SMALL) r = (long long)zp_reduce(F, (int64_t)acc);
        else r = (long long)acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
        if (lane == 0) s_sum[par][wave] = r;
        __syncthreads();
        long long tot = 0;
#pragma unroll
        for (int w = 0; w < BM_BS / 64; w++) tot += s_sum[par][w];
        par ^= 1;
        const int d = zp_reduce(F, (int64_t)tot);
        if (d == 0) { m++; continue; }
        const int f = zp_neg(F, zp_mul(F, d, binv));
        if (2 * L <= i) {
            // ---- the length changes: the new C goes into the array of B, from the top down, read | barrier | write
            const int Ln = i + 1 - L;
            for (int base = (Ln / BM_BS) * BM_BS; base >= 0; base -= BM_BS) {
                const int k = base + tid;
                int pv = 0, qv = 0;
                if (k <= Ln) {
                    pv = P[k];
                    if (k >= m) qv = Q[k - m];
                }
                __syncthreads();
                if (k <= Ln) Q[k] = zp_axpy(F, f, qv, pv);
            }
            int *T = P; P = Q; Q = T;
            LB = L;
            L = Ln;
            binv = zp_inverse(F, d);
            m = 1;
        } else {
            const int top = min(LB + m, dmax);
            for (int k = m + tid; k <= top; k += BM_BS) P[k] = zp_axpy(F, f, Q[k - m], P[k]);
            m++;
        }
        __syncthreads();
    }
    int *out = a.coef + (i64d)c * a.ldc;
    for (i64d k = tid; k < a.ldc; k += BM_BS) out[k] = k <= L ? P[L - k] : 0;
    if (tid == 0) a.deg[c] = L;
}
