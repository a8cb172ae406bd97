"""Times the batched echelonization of small matrices (csrc/batch.hpp) against the loop over S.echelonize on the same inputs:
(i) N = 100, 1000, 10000 random 50 x 60 matrices (synth_csr kind 0, density 0.1) at p = 65521 and p = 127, (ii) a block matrix
of 5000 connected components of mixed sizes (2..40 rows and columns) through Block, batched=True against the per-block loop.
Per case: wall ms per matrix of the batch call (median of --reps after --warmup calls) and of the loop (one pass after a warm-up
of 50 calls; over the first --loop-max matrices when N is larger -- the loop's cost per matrix does not depend on N), their
ratio, and batch_stats of the last batch call (launches, chunks, device microseconds of the LDS path).  The ranks of both sides
are compared.  One JSON line per case.  Kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402

LM = {"enable_greedy_pivot_search": False}


def timed_batch(fn, reps, warmup):
    ms, out = [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def timed_loop(mats, loop_max):
    for A in mats[:50]:
        S.echelonize(A, **LM)
    part = mats[:loop_max]
    t0 = time.perf_counter()
    ranks = [S.echelonize(A, **LM).r for A in part]
    return (time.perf_counter() - t0) * 1e3 / max(len(part), 1), ranks


def report(name, mats, batch_ms, ranks, stats, loop_ms, loop_ranks, extra=None):
    assert ranks[: len(loop_ranks)] == loop_ranks, "batch and loop disagree on a rank"
    out = {
        "case": name, "matrices": len(mats), "batch_ms_per_matrix": round(batch_ms / len(mats), 5), "loop_ms_per_matrix": round(loop_ms, 4),
        "loop_matrices": len(loop_ranks), "ratio_loop_over_batch": round(loop_ms / max(batch_ms / len(mats), 1e-9), 1), "batch_ms": round(batch_ms, 3),
        "device_us_per_matrix": round(stats["device_us"] / len(mats), 3), **stats,
    }
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def block_matrix(ncomp, seed, p):
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(2, 41)), int(rng.integers(2, 41))) for _ in range(ncomp)]
    n, m = sum(a for a, _ in shapes), sum(b for _, b in shapes)
    rperm, cperm = rng.permutation(n), rng.permutation(m)
    rows = [[] for _ in range(n)]
    r0 = c0 = 0
    for (a, b) in shapes:
        D = (rng.random((a, b)) < 0.3) * rng.integers(1, p, size=(a, b))
        for i in range(a):  # a path through the rows and columns keeps the component in one piece
            D[i, i % b] = D[i, i % b] or 7
            if i + 1 < a:
                D[i + 1, i % b] = D[i + 1, i % b] or 5
        for c in range(b):
            if not D[:, c].any():
                D[c % a, c] = 3
        for i in range(a):
            rows[rperm[r0 + i]] = [(int(cperm[c0 + c]), int(D[i, c])) for c in range(b) if D[i, c]]
        r0 += a
        c0 += b
    return S.CSR.from_rows(rows, m, prime=p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--primes", default="65521,127")
    ap.add_argument("--loop-max", type=int, default=1000)
    ap.add_argument("--components", type=int, default=5000, help="0: skip the block case")
    a = ap.parse_args()
    for p in [int(v) for v in a.primes.split(",")]:
        for N in [int(v) for v in a.sizes.split(",")]:
            mats = [S.synth_csr(0, 50, 60, density=0.1, prime=p, seed=0xBA7C0000 + k) for k in range(N)]
            batch_ms, facts = timed_batch(lambda: S.echelonize_batch(mats), a.reps, a.warmup)
            stats = S.batch_stats()
            ranks = [f.r for f in facts]
            del facts
            rank_ms, _ = timed_batch(lambda: S.rank_batch(mats), a.reps, a.warmup)
            loop_ms, loop_ranks = timed_loop(mats, a.loop_max)
            report(f"50x60_p{p}_N{N}", mats, batch_ms, ranks, stats, loop_ms, loop_ranks, {"rank_batch_ms_per_matrix": round(rank_ms / N, 5)})
    if a.components > 0:
        A = block_matrix(a.components, 0xB10C, 42013)
        B = S.Block.from_csr(A)
        batch_ms, E = timed_batch(lambda: S.blocks.echelonize(B, batched=True), a.reps, a.warmup)
        stats = S.batch_stats()
        ranks = [f.r for f in E.blocks]
        del E
        loop_ms, loop_ranks = timed_loop(B.blocks, a.loop_max)
        report(f"block_{len(B)}_components", B.blocks, batch_ms, ranks, stats, loop_ms, loop_ranks, {"shape": list(A.shape), "nnz": S.nnz(A)})


if __name__ == "__main__":
    main()
