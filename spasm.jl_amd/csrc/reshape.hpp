// reshape.hpp -- structural operations on resident matrices over GF(p) on gfx950: transpose, row / column permutation, vcat, hcat
// (spasm_amd_dcsr_transpose / _permute / _vcat / _hcat).  No value changes: there is no modular arithmetic in this file.
//
// All four operations are "move every entry to a computed place, then order a row where its columns no longer ascend":
//   transpose    entry (i, c, v) of A goes to row c of the result as (i, v)
//   permute      row i of the result is row p[i] of A, an entry on column c lands on column qinv[c]
//   vcat         row off_k + i of the result is row i of operand k
//   hcat         row i of the result is row i of operand 0, then of operand 1 with its columns shifted by the widths before it, ..
//
// Steps (host driver: rsh_run in engine.hip):
//   count   the length of every row of the result, exactly: k_rsh_lens reads it off the operands' row pointers (permute, vcat,
//           hcat), k_rsh_hist counts the entries of each column of A (transpose; integer atomics on counts: deterministic).  One
//           exclusive scan gives the row pointers; the result is allocated at its final size.  There is no compaction pass.
//   move    k_rsh_move<TEAM>: a team of 8 lanes or a wave per row (by the average row length, as k_spg_pack is chosen) copies the
//           row's slices to their place.  vcat, hcat and a permutation of rows alone copy slices whose columns ascend already: done.
//           transpose places (source row, value) at the column's cursor (an atomic: the order inside a row is the order of
//           arrival); a permutation with qinv writes relabelled columns in the source's order.
//   order   (transpose, permute with qinv) every row of two entries or more is sorted by column in place.  The operand is
//           canonical, so the keys of a row are distinct, the sorted row is unique and does not depend on the order of arrival.
//           Rows are grouped by length with a stable radix sort (k_rsh_classify):
//             wave   2 .. 64 entries        k_rsh_sort_wave: a wave per row, four rows per workgroup; every lane ranks its entry
//                                           against the row's keys in LDS and writes it at its rank
//             group  65 .. 512, .. 2048,    k_rsh_sort_group: a workgroup of 256 lanes per row, bitonic sort in LDS over the next
//                    .. RSH_GROUP_MAX       power of two of the length; three LDS sizes (4, 16, 64 KB: the largest leaves two
//                                           workgroups per CU inside 160 KB)
//             long   above RSH_GROUP_MAX    the rows are gathered back to back (k_rsh_long_copy), sorted as 64-bit words on their low
//                                           32 bits = the column by rocprim::segmented_radix_sort_keys, and copied back
// LDS access: lanes read and write consecutive elements (stride 1) or one common address (broadcast) everywhere; in a step of
// the bitonic sort the lanes whose partner lies above them are the active ones, and those of a half wave fall on distinct banks.
// No lane walks LDS with a power-of-two stride, so no padding is needed.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"

enum { RSH_TRANSPOSE = 4, RSH_PERMUTE = 5, RSH_VCAT = 6, RSH_HCAT = 7 };  // stats[10] of the result (1 .. 3: spgemm.hpp)

constexpr int RSH_WAVE_MAX = 64;       // rows up to this length are ordered by one wave
constexpr int RSH_GROUP_MAX = 8192;    // .. up to this one by one workgroup in LDS (8 bytes per entry: 64 KB)
constexpr int RSH_NCLASS = 6;          // 0 nothing to order, 1 wave, 2 .. 4 group (512, 2048, 8192), 5 long
constexpr int RSH_CLS_LONG = 5;
#define RSH_NOCOL 0x7fffffff

struct RshOperand {
    const i64d *p;
    const int2 *ent;
    int off;  // vcat: first row of the operand in the result; hcat: its first column
    int n;    // rows
};

struct RshArgs {
    int op;
    int nitems;                  // rows the move walks: the rows of A (transpose), the rows of the result (others)
    int count;                   // operands (1 for transpose and permute)
    const RshOperand *ops;       // device array
    const int *rowmap;           // permute: p, or null
    const int *colmap;           // permute: qinv, or null
    const i64d *Rp;              // row pointers of the result
    int2 *out;                   // its entries
    unsigned long long *cursor;  // transpose: entries placed so far in each row of the result (zero on entry)
};

__host__ __device__ __forceinline__ int rsh_class_of(long long len)
{
    if (len <= 1) return 0;
    if (len <= RSH_WAVE_MAX) return 1;
    if (len <= 512) return 2;
    if (len <= 2048) return 3;
    if (len <= RSH_GROUP_MAX) return 4;
    return RSH_CLS_LONG;
}

// the operand that holds row i of a vcat: the last one that starts at or before i (an operand without rows starts where the next does)
__device__ __forceinline__ int rsh_vcat_operand(const RshArgs &a, int i)
{
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.ops[mid].off <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- count -----------------------------------------------------------------------------------------------------------------
// permute, vcat, hcat: one lane per row of the result
__global__ void k_rsh_lens(RshArgs a, int nrows, i64d *__restrict__ len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    i64d l = 0;
    if (a.op == RSH_HCAT) {
        for (int k = 0; k < a.count; k++) l += a.ops[k].p[i + 1] - a.ops[k].p[i];
    } else if (a.op == RSH_VCAT) {
        const RshOperand o = a.ops[rsh_vcat_operand(a, i)];
        l = o.p[i - o.off + 1] - o.p[i - o.off];
    } else {
        const int r = a.rowmap ? a.rowmap[i] : i;
        l = a.ops[0].p[r + 1] - a.ops[0].p[r];
    }
    len[i] = l;
}

// transpose: the entries of each column (len: zero on entry)
__global__ void k_rsh_hist(i64d nnz, const int2 *__restrict__ ent, unsigned long long *__restrict__ len)
{
    i64d k = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const i64d stride = (i64d)gridDim.x * blockDim.x;
    for (; k < nnz; k += stride) atomicAdd(&len[ent[k].x], 1ull);
}

// ---- move: a team per row ---------------------------------------------------------------------------------------------------
template <int TEAM>
__global__ void k_rsh_move(RshArgs a)
{
    const i64d t = ((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM;
    if (t >= a.nitems) return;
    const int i = (int)t, tl = threadIdx.x % TEAM;
    if (a.op == RSH_TRANSPOSE) {
        const RshOperand o = a.ops[0];
        const i64d st = o.p[i], n = o.p[i + 1] - st;
        for (i64d q = tl; q < n; q += TEAM) {
            const int2 e = o.ent[st + q];
            const i64d pos = a.Rp[e.x] + (i64d)atomicAdd(&a.cursor[e.x], 1ull);  // below Rp[e.x + 1]: the histogram counted this entry
            a.out[pos] = make_int2(i, e.y);
        }
        return;
    }
    int2 *dst = a.out + a.Rp[i];
    if (a.op == RSH_HCAT) {
        for (int k = 0; k < a.count; k++) {
            const RshOperand o = a.ops[k];
            const i64d st = o.p[i], n = o.p[i + 1] - st;
            for (i64d q = tl; q < n; q += TEAM) {
                const int2 e = o.ent[st + q];
                dst[q] = make_int2(e.x + o.off, e.y);
            }
            dst += n;
        }
        return;
    }
    int k = 0, r = i;
    if (a.op == RSH_VCAT) {
        k = rsh_vcat_operand(a, i);
        r = i - a.ops[k].off;
    } else if (a.rowmap) {
        r = a.rowmap[i];
    }
    const RshOperand o = a.ops[k];
    const i64d st = o.p[r], n = o.p[r + 1] - st;
    for (i64d q = tl; q < n; q += TEAM) {
        const int2 e = o.ent[st + q];
        dst[q] = make_int2(a.colmap ? a.colmap[e.x] : e.x, e.y);
    }
}

// ---- order ------------------------------------------------------------------------------------------------------------------
// class keys of the rows for the radix sort, the class histogram and the longest row
__global__ __launch_bounds__(256) void k_rsh_classify(int n, const i64d *__restrict__ Rp, unsigned char *__restrict__ key, int *__restrict__ row,
                                                      int *__restrict__ hist, i64d *__restrict__ maxlen)
{
    __shared__ int s_h[RSH_NCLASS];
    __shared__ i64d s_max;
    if (threadIdx.x < RSH_NCLASS) s_h[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const i64d l = Rp[t + 1] - Rp[t];
        const int c = rsh_class_of(l);
        key[t] = (unsigned char)c;
        row[t] = t;
        atomicAdd(&s_h[c], 1);
        atomicMax((unsigned long long *)&s_max, (unsigned long long)l);
    }
    __syncthreads();
    if (threadIdx.x < RSH_NCLASS && s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
    if (threadIdx.x == 0 && s_max) atomicMax((unsigned long long *)maxlen, (unsigned long long)s_max);
}

// rows of 2 .. 64 entries: a wave per row, four rows per workgroup.  A lane keeps its entry in registers, the keys go to LDS, and
// the rank of an entry is the number of keys below it (ties, which a canonical operand does not have, go by position: the ranks
// are a permutation in any case).  Every entry is read before the barrier and written after it: in place.
__global__ __launch_bounds__(256) void k_rsh_sort_wave(int nitems, const int *__restrict__ items, const i64d *__restrict__ Rp, int2 *__restrict__ ent)
{
    __shared__ int s_key[4][RSH_WAVE_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const i64d it = (i64d)blockIdx.x * 4 + wave;
    i64d st = 0;
    int n = 0;
    if (it < nitems) {
        const int row = items[it];
        st = Rp[row];
        n = (int)(Rp[row + 1] - st);  // <= RSH_WAVE_MAX by its class
    }
    int2 e = make_int2(0, 0);
    if (lane < n) {
        e = ent[st + lane];
        s_key[wave][lane] = e.x;
    }
    __syncthreads();
    if (lane < n) {
        int rank = 0;
        for (int f = 0; f < n; f++) {
            const int d = s_key[wave][f];
            rank += (d < e.x || (d == e.x && f < lane)) ? 1 : 0;
        }
        ent[st + rank] = e;
    }
}

// rows of 65 .. RSH_GROUP_MAX entries: a workgroup per row, bitonic sort in LDS over P = the next power of two of the length.  The
// launch sizes the LDS for the class's largest row (8 bytes per entry).
__global__ __launch_bounds__(256) void k_rsh_sort_group(int nitems, const int *__restrict__ items, const i64d *__restrict__ Rp, int2 *__restrict__ ent)
{
    constexpr int BS = 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char rsh_lds[];
    int2 *s = (int2 *)rsh_lds;
    const int tid = threadIdx.x;
    const int row = items[blockIdx.x];  // grid = nitems
    const i64d st = Rp[row];
    const int n = (int)(Rp[row + 1] - st);
    int P = 128;
    while (P < n) P <<= 1;  // <= the capacity of the row's class
    for (int q = tid; q < P; q += BS) s[q] = q < n ? ent[st + q] : make_int2(RSH_NOCOL, 0);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += BS) {
                const int x = i ^ j;
                if (x > i) {
                    const int2 u = s[i], w = s[x];
                    if ((u.x > w.x) == ((i & k) == 0)) {
                        s[i] = w;
                        s[x] = u;
                    }
                }
            }
            __syncthreads();
        }
    for (int q = tid; q < n; q += BS) ent[st + q] = s[q];
}

// long rows: their lengths (for the host, which cuts them into batches), and the copy to / from the back-to-back buffer
__global__ void k_rsh_long_lens(int nitems, const int *__restrict__ items, const i64d *__restrict__ Rp, i64d *__restrict__ len)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nitems) len[t] = Rp[items[t] + 1] - Rp[items[t]];
}

// a workgroup per row; back: from the buffer to the matrix.  coff: the rows' starts in the buffer (nitems + 1)
__global__ __launch_bounds__(256) void k_rsh_long_copy(int back, const int *__restrict__ items, const i64d *__restrict__ Rp, const unsigned *__restrict__ coff,
                                                       int2 *__restrict__ ent, int2 *__restrict__ buf)
{
    const int row = items[blockIdx.x];  // grid = the rows of the batch
    const i64d st = Rp[row];
    const unsigned c0 = coff[blockIdx.x], n = coff[blockIdx.x + 1] - c0;
    for (unsigned q = threadIdx.x; q < n; q += 256) {
        if (back) ent[st + q] = buf[c0 + q];
        else buf[c0 + q] = ent[st + q];
    }
}
