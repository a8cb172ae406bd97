// colechelon.hpp -- the reduced column echelon form over GF(p) of a tall dense block on gfx950: X is rows x K, row-major, K <= 64
// (spasm_amd_dense_column_echelon, and the basis of spasm_amd_wiedemann_kernel).  The form is unique for a column
// space: column j < rank has its first non-zero entry, a 1, in row pivots[j]; pivots ascends strictly; row pivots[j] is zero in
// every other column; the columns from rank on are zero; every word is the balanced residue.  Two blocks with the same column
// space give the same bytes.
//
// Schedule, column by column (c = 0 .. K - 1), three launches a column and no host synchronization between them:
//   k_ce_find   the first row r with X[r, c] != 0: a lane stops at its first hit, the workgroup takes the minimum (shuffles, LDS)
//               and sends one 32-bit integer vector atomicMin to piv[c] (none when it found nothing).  piv[c] starts at CE_NONE.
//   k_ce_pivot  one wave: copies row piv[c] into the column's own slice of the multiplier table (mult[j] = -X[piv, j]), inverts
//               the pivot and sets the slice's flag; piv[c] == CE_NONE clears the flag, and this launch and the next do nothing.
//   k_ce_elim   one pass over rows x K: X[r, c] <- xc = X[r, c] / pivot, X[r, j] <- X[r, j] - xc * X[piv, j] for j != c.  It reads
//               the pivot row from the table, never from X, so it reads no row another workgroup writes.  A row is held by KW lanes
//               of one wave (KW the power of two >= K); xc reaches them by a shuffle from the lane of column c, the only lane that
//               reads or writes X[r, c].
// Rows above piv[c] are zero in column c and stay as they are; row piv[c'] of an earlier pivot is zero in column c, so it stays as
// it is too, and the first non-zero word of column c' stays the 1 in row piv[c'].  After the K columns the host reads the K pivot
// rows once, sorts the columns that have one, and k_ce_permute compacts them in place (again a shuffle inside the row: every lane
// reads its own word before any word of the row is written).  Work is rows * K words read and written per pivot column,
// O(rows * K^2) in all, bound by memory.
//
// Bound of the accumulator: every word is canonical after zp_residue (any int32 is reduced where it is read).  xc = zp_mul of two
// canonical residues is canonical.  The update is zp_axpy(-m, xc, x) of three canonical residues: |(-m) * xc + x| <= halfp^2 + halfp
// < 2^62 in an i64, the double quotient is within 1 of the exact one (|a x / p| < 2^31, relative error 2^-52), so the remainder is
// below 1.5 p and the one correction of zp_normalize gives the canonical residue: the domain zp.hpp states for zp_axpy.  Nothing
// is summed lazily; there is one product a word and pass.
// Field operations only (zp_mul, zp_axpy, zp_inverse, zp_residue): every prime 2 < p <= 0xFFFFFFFB works.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "spmv_step.hpp"

constexpr int CE_BS = 256;            // lanes of a workgroup
constexpr int CE_MAXK = 64;           // a row is held by one wave
constexpr int CE_NONE = 0x7f7f7f7f;   // piv[c] of a column without a non-zero word: above every row (rows < 2^30), one memset sets it
constexpr int CE_SLICE = CE_MAXK + 2; // words of a column's slice of the table: K multipliers, the inverse, the flag
constexpr int CE_INV = CE_MAXK, CE_FLAG = CE_MAXK + 1;

__global__ __launch_bounds__(CE_BS) void k_ce_find(i64d rows, int c, ZpField F, int hp, int mhp, const int *__restrict__ X, i64d ldx, int *__restrict__ piv)
{
    __shared__ int s_min[CE_BS / 64];
    int best = CE_NONE;
    for (i64d r = (i64d)blockIdx.x * CE_BS + threadIdx.x; r < rows; r += (i64d)gridDim.x * CE_BS)
        if (zp_residue(F, hp, mhp, X[r * ldx + c]) != 0) {
            best = (int)r;
            break;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CE_BS / 64; w++) best = min(best, s_min[w]);
        if (best != CE_NONE) atomicMin(piv + c, best);
    }
}

// one wave; lane j < K
__global__ __launch_bounds__(64) void k_ce_pivot(int K, int c, ZpField F, int hp, int mhp, const int *__restrict__ X, i64d ldx, const int *__restrict__ piv,
                                                 int *__restrict__ mult)
{
    const int j = threadIdx.x, prow = piv[c];
    if (prow == CE_NONE) {
        if (j == 0) mult[CE_FLAG] = 0;
        return;
    }
    const int *row = X + (i64d)prow * ldx;
    if (j < K) mult[j] = zp_neg(F, zp_residue(F, hp, mhp, row[j]));
    if (j == 0) {
        mult[CE_INV] = zp_inverse(F, zp_residue(F, hp, mhp, row[c]));
        mult[CE_FLAG] = 1;
    }
}

// kw lanes a row (kw the power of two >= K, kw <= 64: the lanes of a row share a wave); every lane of a wave walks the same number
// of row groups, so the shuffle is taken by all of them
__global__ __launch_bounds__(CE_BS) void k_ce_elim(i64d rows, int K, int kw, int c, ZpField F, int hp, int mhp, int *__restrict__ X, i64d ldx,
                                                   const int *__restrict__ mult)
{
    if (!mult[CE_FLAG]) return;
    const int j = threadIdx.x % kw, rpb = CE_BS / kw;
    const int inv = mult[CE_INV], nm = j < K ? mult[j] : 0;
    for (i64d base = (i64d)blockIdx.x * rpb; base < rows; base += (i64d)gridDim.x * rpb) {
        const i64d r = base + threadIdx.x / kw;
        const bool mine = r < rows && j < K;
        const int x = mine ? zp_residue(F, hp, mhp, X[r * ldx + j]) : 0;
        const int xc = zp_mul(F, __shfl(x, c, kw), inv);
        if (mine) X[r * ldx + j] = j == c ? xc : zp_axpy(F, nm, xc, x);
    }
}

// the columns of the sorted order, in place: X[r, j] <- X[r, src[j]] for j < rank, 0 for rank <= j < K
struct CeOrder {
    unsigned char src[CE_MAXK];
};

__global__ __launch_bounds__(CE_BS) void k_ce_permute(i64d rows, int K, int kw, int rank, CeOrder ord, ZpField F, int hp, int mhp, int *__restrict__ X, i64d ldx)
{
    const int j = threadIdx.x % kw, rpb = CE_BS / kw;
    const int from = j < rank ? ord.src[j] : 0;
    for (i64d base = (i64d)blockIdx.x * rpb; base < rows; base += (i64d)gridDim.x * rpb) {
        const i64d r = base + threadIdx.x / kw;
        const bool mine = r < rows && j < K;
        const int x = mine ? zp_residue(F, hp, mhp, X[r * ldx + j]) : 0;
        const int y = __shfl(x, from, kw);
        if (mine) X[r * ldx + j] = j < rank ? y : 0;
    }
}

// dst[r, at + i] <- src[r, sel.c[i]], 0 <= i < count <= 16: the accepted candidates join the basis
struct CeSelect {
    int c[16];
};

__global__ __launch_bounds__(CE_BS) void k_ce_gather_columns(i64d rows, int count, CeSelect sel, const int *__restrict__ src, i64d lds, int *__restrict__ dst,
                                                             i64d ldd, int at)
{
    const i64d total = rows * count;
    for (i64d e = (i64d)blockIdx.x * CE_BS + threadIdx.x; e < total; e += (i64d)gridDim.x * CE_BS) {
        const i64d r = e / count;
        const int i = (int)(e - r * count);
        dst[r * ldd + at + i] = src[r * lds + sel.c[i]];
    }
}
