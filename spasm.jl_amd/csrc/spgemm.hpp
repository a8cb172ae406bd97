// spgemm.hpp -- exact sparse matrix algebra over GF(p) on gfx950: C = A B, C = a A + b B, C = A[r0:r1, c0:c1]
// (the resident handles spasm_amd_dcsr_* and the one-shot forms spasm_amd_csr_mul / spasm_amd_csr_lincomb).
//
// One family of kernels serves the three operations.  An output row is a sum of SEGMENTS -- a slice of stored entries, a scalar
// it is multiplied by, a window of columns it is restricted to:
//   product      row i of C = sum over the entries (k, a) of row i of A of   a * (row k of B)        (Gustavson's row-wise scatter)
//   combination  row i of C = sa * (row i of A) + sb * (row i of B)                                  (two segments, or one)
//   submatrix    row i of C = 1 * (row r0 + i of A) on the columns [c0, c1), renumbered from c0      (one segment)
// so that "sum the terms of equal column, drop what is zero mod p, sort by column" is written once.  The canonical form of a
// matrix is the combination 1 * A.
//
// Steps (host driver: spg_run in engine.hip):
//   size     k_spg_size: bound[i] = sum of the segment lengths (products of the row; an upper bound of its entries), the row's
//            slice of the scratch cap[i] = min(bound, columns), its class; rows are grouped by class with a stable radix sort.
//   numeric  by class of BOUND:
//            tiny   (bound <= 32)       k_spg_tiny: a team of 16 lanes per row, 16 rows per workgroup; the terms are ranked by
//                                       (column, position) in LDS, equal columns summed by the first of their run.  No table.
//            hash   (bound <= 64 << c,  k_spg_hash<LOGT = 7 + c>, c = 0 .. 6: one workgroup per row (one wave up to LOGT = 10, four
//                    c = 0 .. 6)        above) and an LDS table of 2^LOGT slots {column tag, accumulator}: the load factor is at most
//                                       1/2 for the row's BOUND, whatever the number of distinct columns turns out to be.  The live
//                                       slots are reduced, the non-zero ones compacted and sorted by column (bitonic, LDS).
//            global (bound > 4096)      k_spg_global: a dense accumulator of `columns` 64-bit words per workgroup in global memory,
//                                       integer atomics; read back in column order (which is the sort), cleared as it is read.
//            The segments of a row are taken batch-wise: a workgroup loads up to BS segment heads, scans their lengths, and its
//            lanes walk the concatenation of the batch (a binary search in the scanned lengths names the segment of a term).  Lanes
//            are busy whether the rows of B hold 3 entries or 30 000.
//   compact  every kernel writes its row sorted into the row's scratch slice and the count; the counts are scanned and
//            k_spg_pack copies the rows back to back.  Rows are processed in chunks whose scratch fits the memory budget.
//
// Accumulator bounds (zp.hpp).  A lazy term is below 2^15.01 in absolute value for p < 2^16 and below 2^31.1 otherwise.
//   tiny:   at most 32 terms summed in i64: below 2^36.1.
//   hash:   at most 4096 terms per row (bound of the largest class), i32 slots for p < 2^16: below 2^27.1; i64 slots otherwise: below 2^43.1.
//   global: i64 words.  Between two reductions in place (k_spg_global sweeps its accumulator whenever 2^30 terms have gone in since
//           the last one, and a batch is cut into slices of 2^30 terms) a word receives at most 2^31 terms on top of a residue:
//           below 2^31 * 2^31.1 + 2^31 < 2^62.2.  Any number of terms per output entry is therefore exact.
// Determinism: integer atomics only (addition of integers is associative), and the order of a row's entries comes from a sort
// over distinct columns or from the column-ordered read of the dense accumulator, never from the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "zp.hpp"

constexpr int SPG_TINY = 32;          // rows with at most this many products go to the team kernel
constexpr int SPG_TINY_TEAM = 16;
constexpr int SPG_LOGT_MIN = 7;       // hash classes: tables of 2^7 .. 2^13 slots, bound <= half the slots
constexpr int SPG_LOGT_MAX = 13;
constexpr int SPG_NCLASS = 10;        // 0 tiny, 1 .. 7 hash, 8 global, 9 rows without products (nothing to do)
constexpr int SPG_CLS_GLOBAL = 8;
constexpr int SPG_CLS_EMPTY = 9;
constexpr long long SPG_SWEEP = 1ll << 30;  // terms between two reductions of the global accumulator
#define SPG_NOCOL 0x7fffffff

enum { SPG_MUL = 1, SPG_LINCOMB = 2, SPG_SUBMATRIX = 3 };

struct SpgArgs {
    int mode;
    int nrows;                 // rows of C
    int ncols;                 // columns of C
    const i64d *Ap;            // first operand: row pointers and packed entries
    const int2 *Aent;
    const i64d *Bp;            // second operand (product: the rows that are scattered; combination: may be null)
    const int2 *Bent;
    int sa, sb;                // scalars of the combination (balanced residues)
    int r0, c0, c1;            // submatrix: first row, column window (other modes: 0, 0, columns)
    ZpField F;
    const i64d *off;           // per row of C: start of its scratch slice (exclusive scan of cap)
    i64d off_base;             // .. minus this (the chunk's first slice)
    int2 *scratch;
    i64d *cnt;                 // per row of C: entries written
};

__device__ __forceinline__ int spg_nseg(const SpgArgs &a, int i)
{
    if (a.mode == SPG_MUL) return (int)(a.Ap[i + 1] - a.Ap[i]);
    return (a.mode == SPG_LINCOMB && a.Bp) ? 2 : 1;
}

__device__ __forceinline__ void spg_seg(const SpgArgs &a, int i, int s, const int2 *&base, i64d &len, int &scale)
{
    if (a.mode == SPG_MUL) {
        const int2 e = a.Aent[a.Ap[i] + s];
        base = a.Bent + a.Bp[e.x];
        len = a.Bp[e.x + 1] - a.Bp[e.x];
        scale = e.y;
    } else if (a.mode == SPG_LINCOMB && s == 1) {
        base = a.Bent + a.Bp[i];
        len = a.Bp[i + 1] - a.Bp[i];
        scale = a.sb;
    } else {
        const int r = a.r0 + i;
        base = a.Aent + a.Ap[r];
        len = a.Ap[r + 1] - a.Ap[r];
        scale = a.mode == SPG_LINCOMB ? a.sa : 1;
    }
}

__host__ __device__ __forceinline__ int spg_class_of(long long bound)
{
    if (bound <= 0) return SPG_CLS_EMPTY;
    if (bound <= SPG_TINY) return 0;
    for (int c = 0; c <= SPG_LOGT_MAX - SPG_LOGT_MIN; c++)
        if (bound <= (64ll << c)) return 1 + c;
    return SPG_CLS_GLOBAL;
}

// size: one lane per row of C (the segment heads of a product row are read through A.j: rows of a few dozen entries)
__global__ void k_spg_size(SpgArgs a, i64d *__restrict__ bound, i64d *__restrict__ cap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrows) return;
    i64d b = 0;
    const int ns = spg_nseg(a, i);
    for (int s = 0; s < ns; s++) {
        const int2 *base;
        i64d len;
        int scale;
        spg_seg(a, i, s, base, len, scale);
        b += len;
    }
    bound[i] = b;
    cap[i] = b < (i64d)a.ncols ? b : (i64d)a.ncols;
}

// the product rows of a matrix with long rows: a wave per row sums the lengths of the rows of B it names (coalesced over A.j)
__global__ void k_spg_size_wave(SpgArgs a, i64d *__restrict__ bound, i64d *__restrict__ cap)
{
    const int i = (int)(((i64d)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (i >= a.nrows) return; // whole waves leave together
    const int lane = threadIdx.x & 63;
    const i64d st = a.Ap[i], n = a.Ap[i + 1] - st;
    i64d b = 0;
    for (i64d k = lane; k < n; k += 64) {
        const int r = a.Aent[st + k].x;
        b += a.Bp[r + 1] - a.Bp[r];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
    if (lane == 0) {
        bound[i] = b;
        cap[i] = b < (i64d)a.ncols ? b : (i64d)a.ncols;
    }
}

// class keys of the rows lo .. lo + n - 1 for the radix sort, and the class histogram (LDS first, then one atomic per class and workgroup)
__global__ __launch_bounds__(256) void k_spg_classify(int lo, int n, const i64d *__restrict__ bound, unsigned char *__restrict__ key, int *__restrict__ row,
                                                      int *__restrict__ hist, i64d *__restrict__ maxbound)
{
    __shared__ int s_h[SPG_NCLASS];
    __shared__ i64d s_max;
    if (threadIdx.x < SPG_NCLASS) s_h[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const i64d b = bound[lo + t];
        const int c = spg_class_of(b);
        key[t] = (unsigned char)c;
        row[t] = lo + t;
        atomicAdd(&s_h[c], 1);
        atomicMax((unsigned long long *)&s_max, (unsigned long long)b);
    }
    __syncthreads();
    if (threadIdx.x < SPG_NCLASS && s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
    if (threadIdx.x == 0 && s_max) atomicMax((unsigned long long *)maxbound, (unsigned long long)s_max);
}

// ---- tiny rows -----------------------------------------------------------------------------------------------------------
// 16 teams of 16 lanes per workgroup, one row each.  Every lane of the workgroup reaches every barrier (a team without a row
// idles through them).  Terms outside the column window keep their position with the tag SPG_NOCOL, which sorts last.
template <bool SMALL>
__global__ __launch_bounds__(256) void k_spg_tiny(SpgArgs a, int nitems, const int *__restrict__ items)
{
    constexpr int T = SPG_TINY_TEAM, TEAMS = 256 / T, CAP = SPG_TINY;
    __shared__ int s_col[TEAMS][CAP];
    __shared__ long long s_val[TEAMS][CAP];
    __shared__ int s_scol[TEAMS][CAP];
    __shared__ long long s_sval[TEAMS][CAP];
    const int team = threadIdx.x / T, tl = threadIdx.x % T;
    const int it = blockIdx.x * TEAMS + team;
    const bool active = it < nitems;
    const int row = active ? items[it] : 0;
    int n = 0;
    if (active) {
        const int ns = spg_nseg(a, row);
        for (int s = 0; s < ns; s++) {
            const int2 *base;
            i64d len;
            int scale;
            spg_seg(a, row, s, base, len, scale);
            for (int k = tl; k < (int)len; k += T) { // n + len <= bound <= CAP
                const int2 e = base[k];
                const bool in = e.x >= a.c0 && e.x < a.c1;
                s_col[team][n + k] = in ? e.x - a.c0 : SPG_NOCOL;
                s_val[team][n + k] = in ? (long long)ZpAcc<SMALL>::mul_lazy(a.F, scale, e.y) : 0;
            }
            n += (int)len;
        }
    }
    __syncthreads();
    for (int e = tl; e < n; e += T) {
        const int c = s_col[team][e];
        int rank = 0;
        for (int f = 0; f < n; f++) {
            const int d = s_col[team][f];
            rank += (d < c || (d == c && f < e)) ? 1 : 0;
        }
        s_scol[team][rank] = c;
        s_sval[team][rank] = s_val[team][e];
    }
    __syncthreads();
    // the first of a run of equal columns sums the run; s_col now holds the residue of a run at its head, 0 elsewhere
    for (int q = tl; q < n; q += T) {
        const int c = s_scol[team][q];
        int v = 0;
        if (c != SPG_NOCOL && (q == 0 || s_scol[team][q - 1] != c)) {
            long long sum = 0;
            for (int f = q; f < n && s_scol[team][f] == c; f++) sum += s_sval[team][f];
            v = zp_reduce(a.F, sum);
        }
        s_col[team][q] = v;
    }
    __syncthreads();
    if (!active) return;
    int2 *out = a.scratch + (a.off[row] - a.off_base);
    int total = 0;
    for (int q = tl; q < n; q += T) {
        const int v = s_col[team][q];
        if (v == 0) continue;
        int pos = 0;
        for (int f = 0; f < q; f++) pos += s_col[team][f] != 0 ? 1 : 0;
        out[pos] = make_int2(s_scol[team][q], v);
    }
    if (tl == 0) {
        for (int f = 0; f < n; f++) total += s_col[team][f] != 0 ? 1 : 0;
        a.cnt[row] = total;
    }
}

// ---- the terms of a row, batch-wise, for a whole workgroup -------------------------------------------------------------------
// s_pre: BS + 1 words, s_base / s_scale: BS.  term(column in C, lazy product) is called once per stored entry inside the window;
// after_slice(terms) is called by every lane (uniformly) after at most SPG_SWEEP terms, behind a barrier.
template <int BS, bool SMALL, class Term, class After>
__device__ __forceinline__ void spg_for_terms(const SpgArgs &a, int row, i64d *s_pre, const int2 **s_base, int *s_scale, Term term, After after_slice)
{
    const int tid = threadIdx.x;
    const int ns = spg_nseg(a, row);
    for (int s0 = 0; s0 < ns; s0 += BS) {
        i64d len = 0;
        if (s0 + tid < ns) {
            const int2 *base;
            int scale;
            spg_seg(a, row, s0 + tid, base, len, scale);
            s_base[tid] = base;
            s_scale[tid] = scale;
        }
        if (tid == 0) s_pre[0] = 0;
        s_pre[tid + 1] = len;
        __syncthreads();
        for (int d = 1; d < BS; d <<= 1) { // inclusive scan of the lengths
            const i64d v = tid >= d ? s_pre[tid + 1 - d] : 0;
            __syncthreads();
            s_pre[tid + 1] += v;
            __syncthreads();
        }
        const i64d total = s_pre[BS];
        for (i64d f0 = 0; f0 < total; f0 += SPG_SWEEP) {
            const i64d lim = total - f0 < SPG_SWEEP ? total : f0 + SPG_SWEEP;
            for (i64d f = f0 + tid; f < lim; f += BS) {
                int lo = 0, hi = BS; // the last segment that starts at or before f (segments of length 0 start where the next one does)
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_pre[mid] <= f) lo = mid;
                    else hi = mid;
                }
                const int2 e = s_base[lo][f - s_pre[lo]];
                if (e.x >= a.c0 && e.x < a.c1) term(e.x - a.c0, ZpAcc<SMALL>::mul_lazy(a.F, s_scale[lo], e.y));
            }
            __syncthreads();
            after_slice(lim - f0);
        }
    }
}

template <bool SMALL> constexpr size_t spg_hash_lds(int logt, int bs)
{
    // accumulators, tags, the list of live entries (half the slots), segment heads of a batch
    return ((size_t)1 << logt) * (SMALL ? 4 : 8) + ((size_t)1 << logt) * 4 + ((size_t)1 << (logt - 1)) * 8 + (size_t)(bs + 1) * 8 + (size_t)bs * 8 +
           (size_t)bs * 4 + 16;
}

// ---- hash classes: one workgroup of BS lanes per row, table of 2^LOGT slots --------------------------------------------------
template <int LOGT, int BS, bool SMALL>
__global__ __launch_bounds__(BS) void k_spg_hash(SpgArgs a, int nitems, const int *__restrict__ items)
{
    typedef typename ZpAcc<SMALL>::type acc_t;
    typedef typename std::conditional<SMALL, unsigned, unsigned long long>::type uacc_t;
    constexpr int SLOTS = 1 << LOGT, LIST = SLOTS / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char spg_lds[];
    acc_t *s_acc = (acc_t *)spg_lds;
    i64d *s_pre = (i64d *)(s_acc + SLOTS);
    const int2 **s_base = (const int2 **)(s_pre + BS + 1);
    int2 *s_list = (int2 *)(s_base + BS);
    int *s_tag = (int *)(s_list + LIST);
    int *s_scale = s_tag + SLOTS;
    int *s_n = s_scale + BS;
    const int tid = threadIdx.x;
    const int row = items[blockIdx.x]; // grid = nitems
    for (int k = tid; k < SLOTS; k += BS) {
        s_tag[k] = -1;
        s_acc[k] = 0;
    }
    if (tid == 0) *s_n = 0;
    __syncthreads();
    spg_for_terms<BS, SMALL>(
        a, row, s_pre, s_base, s_scale,
        [&](int c, acc_t t) {
            unsigned h = ((unsigned)c * 2654435761u) >> (32 - LOGT);
            for (;;) { // distinct columns <= bound <= SLOTS / 2: a free slot exists
                const int old = atomicCAS(&s_tag[h], -1, c);
                if (old == -1 || old == c) break;
                h = (h + 1) & (SLOTS - 1);
            }
            atomicAdd((uacc_t *)&s_acc[h], (uacc_t)t);
        },
        [](i64d) {});
    // live slots: reduce, keep what is not zero (in any order: the columns are distinct and sorted next)
    for (int k = tid; k < SLOTS; k += BS) {
        const int c = s_tag[k];
        if (c < 0) continue;
        const int v = zp_reduce(a.F, (int64_t)s_acc[k]);
        if (v != 0) s_list[atomicAdd(s_n, 1)] = make_int2(c, v);
    }
    __syncthreads();
    const int L = *s_n;
    int P = 1;
    while (P < L) P <<= 1; // <= LIST
    for (int q = L + tid; q < P; q += BS) s_list[q] = make_int2(SPG_NOCOL, 0);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += BS) {
                const int x = i ^ j;
                if (x > i) {
                    const int2 u = s_list[i], w = s_list[x];
                    if ((u.x > w.x) == ((i & k) == 0)) {
                        s_list[i] = w;
                        s_list[x] = u;
                    }
                }
            }
            __syncthreads();
        }
    int2 *out = a.scratch + (a.off[row] - a.off_base);
    for (int q = tid; q < L; q += BS) out[q] = s_list[q];
    if (tid == 0) a.cnt[row] = L;
}

// ---- the last resort: a dense accumulator of ncols words per workgroup, in global memory --------------------------------------
// dense: gridDim.x * ncols words, zero on entry and on exit.
__global__ __launch_bounds__(256) void k_spg_global(SpgArgs a, int nitems, const int *__restrict__ items, long long *__restrict__ dense)
{
    constexpr int BS = 256;
    __shared__ i64d s_pre[BS + 1];
    __shared__ const int2 *s_base[BS];
    __shared__ int s_scale[BS];
    __shared__ int s_wave[BS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long *acc = dense + (i64d)blockIdx.x * a.ncols;
    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int row = items[it];
        i64d since = 0;
        auto term = [&](int c, long long t) { atomicAdd((unsigned long long *)&acc[c], (unsigned long long)t); };
        auto after = [&](i64d terms) {
            since += terms; // (the same on every lane)
            if (since < SPG_SWEEP) return;
            __threadfence(); // the atomics of this lane have landed before anybody reads the words
            __syncthreads();
            for (int c = tid; c < a.ncols; c += BS) {
                const long long w = __hip_atomic_load(&acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&acc[c], (long long)zp_reduce(a.F, w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __threadfence();
            __syncthreads();
            since = 0;
        };
        if (a.F.small) spg_for_terms<BS, true>(a, row, s_pre, s_base, s_scale, [&](int c, int t) { term(c, (long long)t); }, after);
        else spg_for_terms<BS, false>(a, row, s_pre, s_base, s_scale, term, after);
        // (spg_for_terms ends behind a barrier: every atomic of the row has been issued; they are device-scope and this workgroup
        // reads its own accumulator below)
        __threadfence();
        __syncthreads();
        int2 *out = a.scratch + (a.off[row] - a.off_base);
        int run = 0; // entries written so far (the same on every lane)
        for (int c0 = 0; c0 < a.ncols; c0 += BS) {
            const int c = c0 + tid;
            int v = 0;
            if (c < a.ncols) {
                const long long w = __hip_atomic_load(&acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (w != 0) {
                    v = zp_reduce(a.F, w);
                    __hip_atomic_store(&acc[c], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const unsigned long long bal = __ballot(v != 0);
            if (lane == 0) s_wave[wave] = __popcll(bal);
            __syncthreads();
            int pos = run + __popcll(bal & ((1ull << lane) - 1));
            int tot = 0;
#pragma unroll
            for (int w = 0; w < BS / 64; w++) {
                if (w < wave) pos += s_wave[w];
                tot += s_wave[w];
            }
            if (v != 0) out[pos] = make_int2(c, v); // pos < distinct columns touched <= cap
            run += tot;
            __syncthreads();
        }
        if (tid == 0) a.cnt[row] = run;
        __threadfence();
        __syncthreads();
    }
}

// ---- compact: the rows lo .. lo + n - 1 from their scratch slices to their places; a team per row -------------------------------
template <int TEAM>
__global__ void k_spg_pack(int lo, int n, const i64d *__restrict__ off, i64d off_base, const int2 *__restrict__ scratch, const i64d *__restrict__ cnt,
                           const i64d *__restrict__ pos, int2 *__restrict__ out)
{
    const int t = (int)(((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM);
    if (t >= n) return;
    const int tl = threadIdx.x % TEAM;
    const int2 *src = scratch + (off[lo + t] - off_base);
    int2 *dst = out + pos[t];
    const i64d c = cnt[lo + t];
    for (i64d q = tl; q < c; q += TEAM) dst[q] = src[q];
}

// ---- the handle's own small kernels ----------------------------------------------------------------------------------------
// columns outside [0, m): flag (the kernels above index accumulators by column)
__global__ void k_spg_check_cols(i64d nnz, int m, const int *__restrict__ j, int *__restrict__ bad)
{
    i64d k = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const i64d stride = (i64d)gridDim.x * blockDim.x;
    for (; k < nnz; k += stride)
        if ((unsigned)j[k] >= (unsigned)m) *bad = 1;
}

__global__ void k_spg_unpack(i64d nnz, const int2 *__restrict__ ent, int *__restrict__ j, int *__restrict__ x)
{
    i64d k = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const i64d stride = (i64d)gridDim.x * blockDim.x;
    for (; k < nnz; k += stride) {
        const int2 e = ent[k];
        j[k] = e.x;
        x[k] = e.y;
    }
}

// two canonical matrices: any difference in the row pointers or the entries sets *diff
__global__ void k_spg_diff(int n, i64d nnz, const i64d *__restrict__ pa, const i64d *__restrict__ pb, const int2 *__restrict__ ea, const int2 *__restrict__ eb,
                           int *__restrict__ diff)
{
    i64d k = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const i64d stride = (i64d)gridDim.x * blockDim.x;
    for (; k < nnz || k <= n; k += stride) {
        bool d = false;
        if (k <= n) d = pa[k] != pb[k];
        if (k < nnz) d = d || ea[k].x != eb[k].x || ea[k].y != eb[k].y;
        if (d) *diff = 1;
    }
}
