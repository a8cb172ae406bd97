// block_krylov.hpp -- block projected Krylov sequences over GF(p) on gfx950: S_i = U^T M^i V, a b x b matrix per step, for n x b
// arrays U and V, b in {2, 4, 8, 16} (spasm_amd_block_sequence).  A block sequence of about 2 n / b terms carries
// what K independent scalar sequences of 2 n terms carry, so block Wiedemann needs about 2 n / b sparse products where the scalar
// routines of krylov.hpp and precond.hpp need 2 n.
//
// The step is k_spmv_step / k_spmv_step_combine of spmv_step.hpp with BlockEpi<B> (KW = B columns): the lane that owns y[row, c]
// stores y = d[row] * y0 (or y0 without a diagonal) and contributes the B canonical residues zp_mul(U[row, r], y), 0 <= r < B, to
// the B sums it keeps in registers over the rows its team walks.  block_project then adds each of them over the lanes of the wave
// that hold column c (shuffles), over the waves of the workgroup (LDS: (KRY_BS / 64) * B * B words of 8 bytes, 8 KiB at B = 16) and
// sends at most B * B 64-bit integer vector atomics per (workgroup, step) to acc[step * B * B + r * B + c], none where the sum is
// 0.  Term 0 is k_block_dot; the finish is k_krylov_finish of krylov.hpp over B * B words a step.
//
// Bound of the projection, as in krylov.hpp: U[row, r] is canonical after zp_residue and y is canonical, so a term is a canonical
// residue, |term| <= halfp < 2^31; an entry of S sums one term per row and there are at most 2^31 rows, so every partial sum and
// the total stay below 2^31 * halfp < 2^62 in an i64, inside the domain of zp_reduce.  The sums are integers: they do not depend
// on the order in which lanes, waves, workgroups and atomics add, and two runs give the same bytes.  The bound of the scale by d
// is that of precond.hpp (two canonical residues), the bounds of the product itself are those of spmv.hpp.
// Field operations only (zp_mul, zp_residue): every prime 2 < p <= 0xFFFFFFFB works.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "spmv_step.hpp"

// The workgroup's sums of t[r] over the lanes of each column c (the column of a lane is threadIdx.x % B) are added to
// accp[r * B + c].  Every lane of the workgroup calls it, with zeros where it owns nothing.  |t[r]| < 2^62.
template <int B> __device__ __forceinline__ void block_project(long long (&t)[B], long long *accp)
{
    static_assert(B >= 2 && B <= 16 && B * B <= KRY_BS, "block width");
    constexpr int NW = KRY_BS / 64;
    __shared__ long long s_blk[NW * B * B];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < B; r++) {
        long long x = t[r];
#pragma unroll
        for (int o = B; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
        if (lane < B) s_blk[(wave * B + r) * B + lane] = x;
    }
    __syncthreads();
    if (threadIdx.x < B * B) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += s_blk[w * B * B + threadIdx.x];
        if (s != 0) atomicAdd((unsigned long long *)(accp + threadIdx.x), (unsigned long long)s);
    }
}

// S_0: accp[r * B + c] += sum_k U[k, r] * X[k, c]; one lane per (row, column c), striding over the rows
template <int B>
__global__ __launch_bounds__(KRY_BS) void k_block_dot(int n, ZpField F, int hp, int mhp, const int *__restrict__ U, i64d ldu,
                                                      const int *__restrict__ X, i64d ldx, long long *__restrict__ accp)
{
    constexpr int RPB = KRY_BS / B;
    const int c = threadIdx.x % B;
    long long t[B] = {};
    for (i64d k = (i64d)blockIdx.x * RPB + threadIdx.x / B; k < n; k += (i64d)gridDim.x * RPB) {
        const int x = zp_residue(F, hp, mhp, X[k * ldx + c]);
        const int *u = U + k * ldu;
#pragma unroll
        for (int r = 0; r < B; r++) t[r] += zp_mul(F, zp_residue(F, hp, mhp, u[r]), x);
    }
    block_project<B>(t, accp);
}

// the epilogue of a block step (spmv_step.hpp, B terms an entry): Y[row, c] <- y = d[row] * y0 (d == NULL: y0) and the terms
// U[row, r] * y of acc[r * B + c]
template <int B> struct BlockEpi {
    const int *d;
    const int *U;
    i64d ldu;
    long long *acc;
    __device__ void own(const ZpField &F, int hp, int mhp, int row, int, int y0, int *yp, long long (&t)[B]) const
    {
        const int y = d ? zp_mul(F, zp_residue(F, hp, mhp, d[row]), y0) : y0; // two canonical residues
        *yp = y;
        const int *u = U + (i64d)row * ldu;
#pragma unroll
        for (int r = 0; r < B; r++) t[r] += zp_mul(F, zp_residue(F, hp, mhp, u[r]), y);
    }
    template <int KW> __device__ void project(long long (&t)[B]) const
    {
        static_assert(KW == B, "a block step has B columns");
        block_project<B>(t, acc);
    }
};

template <int B> struct EpiTerms<BlockEpi<B>> { static constexpr int value = B; };
