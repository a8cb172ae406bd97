// polyprod.hpp -- the exact product of many polynomials mod p on the device: a product tree over ONE concatenated array.
//
// Layout.  Polynomial k of the input is len[k] >= 1 words, low degree first, at off[k] = the exclusive scan of len; T = sum of len
// is below 2^31, so every offset and every word index is an int.  A level multiplies the neighbours (2k, 2k + 1) of its list into
// the OTHER of two buffers of T words each, at the offset of the left factor: a product of lengths a and b has a + b - 1 <= a + b
// words, so it fits the span of its pair (one slack word stays behind each product; it is never read, because a pair names the
// offsets of BOTH its factors: the right one begins where it began at level 0, not behind the left one).  An odd last polynomial
// is copied.  The list of the next level is (off[2k], a + b - 1).  ceil(log2 count) levels, one launch each; the lengths are known on
// the host, so all descriptors of all levels are built there and uploaded once, and no coefficient crosses the host in between.
// The result is the first T - count + 1 words of the buffer the last level wrote.
//
// Arithmetic.  Word t of u * v (lengths a <= b after a swap) is sum_{i = max(0, t-b+1) .. min(t, a-1)} u[i] * v[t-i]: every term
// goes through zp_axpy, as in charpoly.hpp.  No lazy accumulator, hence no term count to bound: every accepted prime works.  The
// operands are balanced residues: the input of the C entry is reduced once by k_pp_reduce (any int32 is allowed there), the
// factors of the characteristic polynomials are balanced already, and a level writes canonical residues only.
//
// Two walking shapes, chosen per pair by the SHORTER factor's length a (the longest sum a word of the pair can have):
//   a <  PP_WAVE   one thread per output word (a copy is such a pair with b = 0)
//   a >= PP_WAVE   one wave per output word: lane l takes the terms lo + l, lo + l + 64, .., a butterfly of zp_add adds the 64
//                  partial sums (step 4 of charpoly_hessenberg), lane 0 stores.  A wave takes PP_WPW words in turn.
// Each shape numbers the output words of ITS pairs of the level consecutively: sum[q] = words before the q-th pair of the shape
// (sum[cnt] = all of them), pair[q] = which pair that is.  A thread (a wave) finds its pair by a binary search of its word number
// in sum[].  The first tb workgroups of a launch walk the thread shape, the others the wave shape.
//
// Index bounds.  For 0 <= t <= a + b - 2: lo = max(0, t - b + 1) <= i <= hi = min(t, a - 1), so 0 <= i < a and 0 <= t - i <= b - 1:
// reads stay inside [off, off + a) and [offb, offb + b), both inside the span of the pair in the source buffer (offb >= off + a);
// the store goes to off + t <= off + a + b - 2 in the other buffer.  Pairs have disjoint spans, and a level never reads what it
// writes.  lo <= hi for every such t (a, b >= 1).
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"

#define PP_WAVE 64   // shorter factor of at least this many words: a wave per output word
#define PP_WPW 4     // output words a wave takes in turn

struct PpPair { int off, a, offb, b; };   // factors at off (a words) and offb (b words), the product at off; b == 0: a copy of a words

struct PpArgs {
    ZpField F;
    const PpPair *pair;        // the pairs of this level
    const int *tsum, *tpair;   // thread shape: tcnt + 1 sums, tcnt pairs
    const int *wsum, *wpair;   // wave shape
    int tcnt, wcnt;
    int tb;                    // workgroups of the thread shape
    const int *src;
    int *dst;
};

// the q with sum[q] <= w < sum[q + 1] (pairs have at least one word each, so it is unique); 0 <= w < sum[cnt]
__device__ __forceinline__ int pp_locate(const int *__restrict__ sum, int cnt, int w)
{
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (sum[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void k_pp_reduce(ZpField F, int words, int *__restrict__ x)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < words) x[w] = zp_reduce(F, (int64_t)x[w]);
}

__global__ __launch_bounds__(256) void k_pp_level(PpArgs g)
{
    const ZpField F = g.F;
    if ((int)blockIdx.x < g.tb) {
        const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (w >= g.tsum[g.tcnt]) return;
        const int q = pp_locate(g.tsum, g.tcnt, (int)w);
        const PpPair pr = g.pair[g.tpair[q]];
        const int t = (int)w - g.tsum[q];
        const int *u = g.src + pr.off, *v = g.src + pr.offb;
        int a = pr.a, b = pr.b;
        if (b == 0) { g.dst[pr.off + t] = u[t]; return; }
        if (a > b) { const int *x = u; u = v; v = x; a = pr.b; b = pr.a; }
        const int lo = t - b + 1 > 0 ? t - b + 1 : 0, hi = t < a - 1 ? t : a - 1;
        int acc = 0;
        for (int i = lo; i <= hi; i++) acc = zp_axpy(F, u[i], v[t - i], acc);
        g.dst[pr.off + t] = acc;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t first = (((int64_t)blockIdx.x - g.tb) * 4 + wave) * PP_WPW;
    const int total = g.wsum[g.wcnt];
    for (int r = 0; r < PP_WPW; r++) {
        const int64_t w = first + r;
        if (w >= total) return;   // the same for all lanes of the wave
        const int q = pp_locate(g.wsum, g.wcnt, (int)w);
        const PpPair pr = g.pair[g.wpair[q]];
        const int t = (int)w - g.wsum[q];
        const int *u = g.src + pr.off, *v = g.src + pr.offb;
        int a = pr.a, b = pr.b;
        if (a > b) { const int *x = u; u = v; v = x; a = pr.b; b = pr.a; }
        const int lo = t - b + 1 > 0 ? t - b + 1 : 0, hi = t < a - 1 ? t : a - 1;
        int acc = 0;
        for (int i = lo + lane; i <= hi; i += 64) acc = zp_axpy(F, u[i], v[t - i], acc);
        for (int off = 32; off > 0; off >>= 1) acc = zp_add(F, acc, __shfl_xor(acc, off));
        if (lane == 0) g.dst[pr.off + t] = acc;
    }
}
