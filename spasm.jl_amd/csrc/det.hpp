// det.hpp -- the determinant mod p of many small square matrices in one launch: one workgroup per matrix, resident in LDS.
//
// The input, the descriptors, the classes and the LDS layout are those of batch.hpp (BatchDesc, BatchArgs, BatchLds,
// batch_lds_words); the elimination is batch_eliminate with the skip of rows that are pivots already, as BATCH_RANK runs it.  The
// skip does not touch a pivot: the pivot of column c is elected, and its inverse kept in pinv[], before any later step reaches the
// row.  A kernel of its own, not a mode of k_batch_elim, whose register budget has no room for one more run-time test (batch.hpp).
//
// What the elimination leaves behind when the rank is n: the k-th pivot lies on column k (every column has one, so pivcol[k] = k)
// and on image row pivrow[k], and pinv[k] is the inverse of its value at the time of its election.  Subtracting multiples of one row
// from another does not change a determinant, so
//   det = sgn(k -> pivrow[k]) * prod_k pivot_k = sgn(k -> pivrow[k]) * (prod_k pinv[k])^-1.
// The product of the n inverses costs n multiplications and ONE inversion: a strided product per lane, a butterfly over the wave,
// the wave products through the election's mailbox (free after the elimination's last barrier), combined by thread 0.  The sign is
// the parity of the inversions of pivrow: thread k counts the j < k with pivrow[j] > pivrow[k] (n <= 181 <= BS on this path: every
// lane of a wave reads the same word, which LDS broadcasts), the wave sums the parities with a ballot.
// A rank below n gives 0; n = 0 gives 1 (the empty product).  det[item] is a balanced residue, written by thread 0.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "batch.hpp"

// BatchArgs as k_batch_elim reads it; mode, rec, scratch and cnt are not looked at, and `rank` is det[], indexed like desc.
template <int BS>
__global__ __launch_bounds__(BS) void k_batch_det(BatchArgs a)
{
    extern __shared__ int s_det[];
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = a.items[blockIdx.x];
    const BatchDesc d = a.desc[item];
    const ZpField F = d.F;
    const int n = d.n, ld = d.ld;
    const BatchLds L(s_det, a.cap, a.bw, a.rmax, false);
    int *img = L.img;

    batch_lds_clear<BS>(L, n * ld, a.bw);
    __syncthreads();
    batch_load_rows<BS, false>(F, img, ld, n, n, a.P + d.row0, a.J, a.X);
    __syncthreads();

    const int r = batch_eliminate<BS, false>(F, L, ld, n, n, n, true, nullptr);
    if (r < n) {
        if (tid == 0) a.rank[item] = 0;
        return;
    }
    // (pivrow[], pinv[] of the last pivot were written before the barrier that ends the elimination; the mailbox is free)
    const int *pivrow = L.pivrow, *pinv = L.pinv;
    int prod = 1;
    unsigned odd = 0;
    for (int k = tid; k < n; k += BS) {
        prod = zp_mul(F, prod, pinv[k]);
        const int mine = pivrow[k];
        int inv = 0;
        for (int j = 0; j < k; j++) inv += pivrow[j] > mine ? 1 : 0;
        odd ^= (unsigned)inv & 1u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) prod = zp_mul(F, prod, __shfl_xor(prod, off));
    const unsigned long long b = __ballot(odd != 0);
    if (lane == 0) {
        L.wmin[wave] = prod;
        L.wmin[8 + wave] = (int)(__popcll(b) & 1);
    }
    __syncthreads();
    if (tid == 0) {
        int all = 1, sign = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            all = zp_mul(F, all, L.wmin[w]);
            sign ^= L.wmin[8 + w];
        }
        const int piv = zp_inverse(F, all);
        a.rank[item] = sign ? zp_neg(F, piv) : piv;
    }
}
