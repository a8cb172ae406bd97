// charpoly.hpp -- the characteristic polynomial chi_A(x) = det(x * I - A) mod p of many small square matrices in one launch: one
// workgroup per matrix, resident in LDS; and of one larger matrix (n <= CHARPOLY_NMAX) by one workgroup on an image in global memory.
//
// Row operations keep rank, kernel and determinant but not the spectrum, so this is no epilogue of batch_eliminate: the matrix is
// brought to upper Hessenberg form by SIMILARITY (every row operation is followed by the inverse column operation), and chi is read
// off the Hessenberg matrix by a recurrence over its leading principal minors.  Both use field operations only (no division by
// 1 .. n as in Faddeev-LeVerrier or the Newton identities), so every prime the engine accepts works, p <= n included.
//
// Input, descriptors and classes are those of batch.hpp (BatchDesc, the staged concatenated CSR, the four classes); the dense
// n x n image is loaded as k_batch_det loads it (zp_reduce on every entry, odd row stride).  BatchDesc::rec is where the n + 1
// coefficients of the matrix go in coef[], BatchDesc::slice where its image starts in gimg[] (global path).
//
// Phase 1, charpoly_hessenberg.  For k = 0 .. n - 3, with s = k + 1:
//   election   the FIRST row pr > k with a[pr][k] != 0: ballot per wave, one candidate per wave in the mailbox, all read after a
//              barrier; rows are scanned in blocks of BS from s on, and the mailbox has two halves used in turn, as in
//              batch_eliminate.  No such row: column k is in Hessenberg form already, next k.
//   swap       pr != s: rows pr and s (columns >= k; left of k both rows are zero), barrier, columns pr and s (all rows), barrier.
//   factors    f_i = a[i][k] / a[s][k] for i > s, written over a[i][k]; barrier.
//   rows       row_i -= f_i * row_s on columns > k, TX lanes per row; barrier.
//   columns    the inverse operation, on ALL rows r: a[r][s] += sum_{i > s} f_i * a[r][i]; TX lanes per row form the dot product
//              (each term reduced, zp_axpy) and a butterfly of zp_add adds them up; barrier.
//   clear      a[i][k] = 0 for i > s.  No barrier: no later step reads or writes column k below the subdiagonal.
// That is 4 barriers per column (5 when the election runs into a second block of rows, 2 more with a swap), 1 where no pivot exists.
// The pivot rule fixes the sequence of operations, so two runs give the same bits; chi does not depend on it.
//
// Phase 2, charpoly_recurrence.  With p_0 = 1 and p_k the characteristic polynomial of the leading k x k block of H,
//   p_{k+1}(x) = (x - h_kk) * p_k(x) - sum_{i<k} h_ik * (prod_{j=i+1..k} h_{j,j-1}) * p_i(x).
// Step k: lane i <= k multiplies its suffix product prod[i] by h_{k,k-1} (ONE multiplication, prod[k] = 1) and posts
// g[i] = h_ik * prod[i]; barrier; lane j <= k forms coefficient j of p_{k+1} = p_k[j-1] - sum_{i=j..k} g[i] * p_i[j], every term
// reduced (zp_axpy), no lazy accumulator.  g has two halves used in turn, so ONE barrier per step is enough: step k + 1 posts into
// the other half and reads H and its own prod word only, and the half of step k is written again after the barrier of step k + 1.
//
// Where the polynomials live.  All of p_0 .. p_{n-1} stay live; the leading 1 is implicit, p_i has i words.  After phase 1 the image
// strictly below the subdiagonal is zero and never read as part of H: coefficient j of p_i (0 <= j < i <= n - 2) is the word
// img[(i + 1) * ld + j], row i + 1 <= n - 1, column j <= (i + 1) - 2.  p_{n-1} (n - 1 words) lives in last[], p_n goes to coef[].
//
// Work words besides the image: last[n - 1], prod[n], g[2][n], the mailbox (16).  The LDS kernel carves them behind the image out of
// what the shared launcher allots a class (batch_lds_words): 4 * rmax + 16 <= 2 * bw + 3 * rmax + 16 because rmax <= 2 * bw in every
// class (33 / 64, 65 / 256, 111 / 768, 182 / 2048), and n < rmax.  The global kernel keeps them in static LDS (CHARPOLY_NMAX each).
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"
#include "batch.hpp"

#define CHARPOLY_NMAX 1024   // the global path: one workgroup per matrix, an image of at most 1024 x 1025 words

struct CharpolyArgs {
    const BatchDesc *desc;
    const int *items;          // descriptors of this launch
    const i64d *P;
    const int *J;
    const int *X;
    const int2 *E;             // not NULL: packed {column, value} entries (a resident matrix) in place of J and X
    int cap, bw, rmax;         // the class, filled in by the launcher
    int *coef;
    int *gimg;                 // global path: the images
};

// the dense image of the matrix: cleared, then scattered from the CSR; ends with a barrier
template <int BS> __device__ __forceinline__ void charpoly_load(const CharpolyArgs &a, const BatchDesc &d, int *img)
{
    const int tid = threadIdx.x, n = d.n, ld = d.ld;
    const ZpField F = d.F;
    for (int e = tid; e < n * ld; e += BS) img[e] = 0;
    __syncthreads();
    // (batch_load_rows with a second arm for packed entries; the select stays inside the row loop, where the compiler has it)
    const BatchLanes<BS> t(n);
    for (int i = t.ty; i < n; i += t.TY) {
        const i64d e0 = a.P[d.row0 + i], e1 = a.P[d.row0 + i + 1];
        if (a.E) {
            for (i64d k = e0 + t.tx; k < e1; k += t.TX) {
                const int2 e = a.E[k];
                img[i * ld + e.x] = zp_reduce(F, (int64_t)e.y);
            }
        } else {
            for (i64d k = e0 + t.tx; k < e1; k += t.TX) img[i * ld + a.J[k]] = zp_reduce(F, (int64_t)a.X[k]);
        }
    }
    __syncthreads();
}

// phase 1: the image becomes an upper Hessenberg matrix similar to it; ends with a barrier
template <int BS> __device__ __forceinline__ void charpoly_hessenberg(const ZpField &F, int *img, int *wmin, int n, int ld)
{
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BatchLanes<BS> t(n);
    const int TX = t.TX, tx = t.tx, ty = t.ty, TY = t.TY;

    int par = 0;
    for (int k = 0; k + 2 < n; k++) {
        const int s = k + 1;
        // ---- election: the first row below row k that holds column k
        int pr = 0x7fffffff;
        for (int base = s; base < n; base += BS) {
            const int i = base + tid;
            const bool hit = i < n && img[i * ld + k] != 0;
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wmin[par * 8 + wave] = b ? base + wave * 64 + (__ffsll((long long)b) - 1) : 0x7fffffff;
            __syncthreads();
            int best = 0x7fffffff;
#pragma unroll
            for (int w = 0; w < NW; w++) best = min(best, wmin[par * 8 + w]);
            par ^= 1;
            if (best != 0x7fffffff) { pr = best; break; }
        }
        if (pr == 0x7fffffff) continue;
        // ---- the pivot to row s: rows pr and s, then columns pr and s
        if (pr != s) {
            for (int j = k + tid; j < n; j += BS) {
                const int u = img[s * ld + j], v = img[pr * ld + j];
                img[s * ld + j] = v;
                img[pr * ld + j] = u;
            }
            __syncthreads();
            for (int r = tid; r < n; r += BS) {
                const int u = img[r * ld + s], v = img[r * ld + pr];
                img[r * ld + s] = v;
                img[r * ld + pr] = u;
            }
            __syncthreads();
        }
        const int inv = zp_inverse(F, img[s * ld + k]);
        // ---- factors, in place on column k
        for (int i = s + 1 + tid; i < n; i += BS) {
            const int f = img[i * ld + k];
            if (f != 0) img[i * ld + k] = zp_mul(F, f, inv);
        }
        __syncthreads();
        // ---- rows: row i -= factor * row s, on the columns right of k
        for (int i = s + 1 + ty; i < n; i += TY) {
            const int f = img[i * ld + k];
            if (f == 0) continue;
            for (int j = s + tx; j < n; j += TX) {
                const int v = img[s * ld + j];
                if (v != 0) img[i * ld + j] = zp_axpy(F, -f, v, img[i * ld + j]);
            }
        }
        __syncthreads();
        // ---- columns: column s += sum of factor_i * column i, on every row (the trip count is the same for all lanes)
        for (int r0 = 0; r0 < n; r0 += TY) {
            const int r = r0 + ty;
            int acc = 0;
            if (r < n)
                for (int i = s + 1 + tx; i < n; i += TX) {
                    const int f = img[i * ld + k];
                    if (f != 0) acc = zp_axpy(F, f, img[r * ld + i], acc);
                }
            for (int off = TX >> 1; off > 0; off >>= 1) acc = zp_add(F, acc, __shfl_xor(acc, off));
            if (r < n && tx == 0 && acc != 0) img[r * ld + s] = zp_add(F, img[r * ld + s], acc);
        }
        __syncthreads();
        // ---- column k below the subdiagonal is zero again
        for (int i = s + 1 + tid; i < n; i += BS) img[i * ld + k] = 0;
    }
    __syncthreads();
}

// phase 2: out[0 .. n] = the coefficients of chi, low degree first, from the Hessenberg image; gs = words of one half of g
template <int BS>
__device__ __forceinline__ void charpoly_recurrence(const ZpField &F, int *img, int *last, int *prod, int *g, int gs, int n, int ld, int *out)
{
    const int tid = threadIdx.x;
    int par = 0;
    for (int k = 0; k < n; k++) {
        int *gk = g + par * gs;
        const int sub = k > 0 ? img[k * ld + k - 1] : 1;
        for (int i = tid; i <= k; i += BS) {
            int t = 1;
            if (i + 1 == k) t = sub;
            else if (i < k) t = zp_mul(F, prod[i], sub);
            prod[i] = t;
            gk[i] = zp_mul(F, img[i * ld + k], t);
        }
        __syncthreads();
        for (int j = tid; j <= k; j += BS) {
            // p_k: in the image while k <= n - 2, else in last[]
            int acc, pkj;
            if (k + 1 < n) {
                acc = j > 0 ? img[(k + 1) * ld + j - 1] : 0;
                pkj = j < k ? img[(k + 1) * ld + j] : 1;
            } else {
                acc = j > 0 ? last[j - 1] : 0;
                pkj = j < k ? last[j] : 1;
            }
            if (j < k) {
                acc = zp_sub(F, acc, gk[j]);   // p_j[j] = 1
                for (int i = j + 1; i < k; i++) acc = zp_axpy(F, -gk[i], img[(i + 1) * ld + j], acc);
            }
            acc = zp_axpy(F, -gk[k], pkj, acc);
            if (k + 2 < n) img[(k + 2) * ld + j] = acc;
            else if (k + 2 == n) last[j] = acc;
            else out[j] = acc;
        }
        par ^= 1;
    }
    if (tid == 0) out[n] = 1;
}

template <int BS>
__global__ __launch_bounds__(BS) void k_batch_charpoly(CharpolyArgs a)
{
    extern __shared__ int s_charpoly[];
    const int item = a.items[blockIdx.x];
    const BatchDesc d = a.desc[item];
    const ZpField F = d.F;
    int *img = s_charpoly, *last = img + a.cap, *prod = last + a.rmax, *g = prod + a.rmax, *wmin = g + 2 * a.rmax;
    charpoly_load<BS>(a, d, img);
    charpoly_hessenberg<BS>(F, img, wmin, d.n, d.ld);
    charpoly_recurrence<BS>(F, img, last, prod, g, a.rmax, d.n, d.ld, a.coef + d.rec);
}

// the same two phases on an image in global memory (a barrier orders the global accesses of a workgroup)
__global__ __launch_bounds__(512) void k_charpoly_global(CharpolyArgs a)
{
    __shared__ int s_work[4 * CHARPOLY_NMAX + 16];
    const int item = a.items[blockIdx.x];
    const BatchDesc d = a.desc[item];
    const ZpField F = d.F;
    int *img = a.gimg + d.slice, *last = s_work, *prod = last + CHARPOLY_NMAX, *g = prod + CHARPOLY_NMAX, *wmin = g + 2 * CHARPOLY_NMAX;
    charpoly_load<512>(a, d, img);
    charpoly_hessenberg<512>(F, img, wmin, d.n, d.ld);
    charpoly_recurrence<512>(F, img, last, prod, g, CHARPOLY_NMAX, d.n, d.ld, a.coef + d.rec);
}
