"""Times the determinant entries (csrc/det.hpp) against the yardstick that runs the same elimination with the same skip,
rank_batch / DeviceBlocks.rank, on the same inputs: (i) N random dense n x n matrices per case (4096 of 32 x 32, 1024 of 110 x 110,
256 of 181 x 181) at each of --primes through det_batch and rank_batch, (ii) one block-diagonal matrix of 20 x 20 blocks (200 000
rows by default), scrambled by random row and column permutations, through DeviceBlocks.det and DeviceBlocks.rank on one handle.
Per case: wall ms of both calls (median of --reps after --warmup calls), the device microseconds of the LDS path that det_stats /
batch_stats report for the last call (HIP events around the launches), both ratios det / rank, and the counters of det_stats.
Both sides must agree on which inputs are singular.  One JSON line per case, printed and appended to
--out (profiles/det_timing.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spasm_jl_amd as S  # noqa: E402


def timed(fn, reps, warmup):
    ms, out = [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def dense_csr(rng, n, p):
    V = S.balanced(rng.integers(1, p, size=(n, n), dtype=np.int64), p)
    return S.CSR.from_arrays(n, n, np.arange(n + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int32), n), V.ravel(), prime=p)


def block_diagonal(rng, nblocks, bs, p):
    """nblocks dense bs x bs blocks on a diagonal; row r moves to rp[r], column c to cq[c].  A block is L * U with L unit lower
    triangular and the diagonal of U non-zero, so none is singular (among 10 000 random blocks over p = 65521 one would be, one
    time in seven, and the parities would never be reached); p < 2^31."""
    n = nblocks * bs
    L = np.tril(rng.integers(1, p, size=(nblocks, bs, bs), dtype=np.int64), -1) + np.eye(bs, dtype=np.int64)
    U = np.triu(rng.integers(1, p, size=(nblocks, bs, bs), dtype=np.int64))
    V = S.balanced(np.matmul(L, U) % p, p).reshape(n, bs)
    rp, cq = rng.permutation(n), rng.permutation(n)
    src = np.empty(n, dtype=np.int64)
    src[rp] = np.arange(n)
    cols = cq[(src // bs * bs)[:, None] + np.arange(bs)[None, :]]
    return S.CSR.from_arrays(n, n, np.arange(n + 1, dtype=np.int64) * bs, cols.ravel(), V[src].ravel(), prime=p)


def record(out_path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="4096x32,1024x110,256x181", help="N x n, comma separated; empty: skip")
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--block-rows", type=int, default=200000, help="rows of the block-diagonal matrix; 0: skip")
    ap.add_argument("--block-size", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_timing.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0xDE7)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for case in [c for c in a.cases.split(",") if c]:
            N, n = (int(v) for v in case.split("x"))
            mats = [dense_csr(rng, n, p) for _ in range(N)]
            det_ms, dets = timed(lambda: S.det_batch(mats), a.reps, a.warmup)
            dst = S.det_stats()
            rank_ms, ranks = timed(lambda: S.rank_batch(mats), a.reps, a.warmup)
            bst = S.batch_stats()
            assert [bool(d) for d in dets.tolist()] == [r == n for r in ranks], "det and rank disagree on which matrices are singular"
            record(a.out, {
                "case": f"{N}x{n}x{n}_p{p}", "matrices": N, "n": n, "prime": p, "det_ms": round(det_ms, 3), "rank_ms": round(rank_ms, 3),
                "wall_ratio_det_over_rank": round(det_ms / rank_ms, 3), "det_device_us": dst["device_us"], "rank_device_us": bst["device_us"],
                "device_ratio_det_over_rank": round(dst["device_us"] / max(bst["device_us"], 1), 3), "det_stats": dst,
            })
            del mats
    if a.block_rows > 0:
        p, bs = 65521, a.block_size
        A = block_diagonal(rng, a.block_rows // bs, bs, p)
        with S.DeviceBlocks(A) as Bk:
            det_ms, d = timed(Bk.det, a.reps, a.warmup)
            dst = S.det_stats()
            rank_ms, ranks = timed(Bk.rank, a.reps, a.warmup)
            bst = S.batch_stats()
            whole_ms, dw = timed(lambda: S.det(A), a.reps, a.warmup)   # upload and split included
            assert dw == d
            assert (d != 0) == (sum(ranks) == A.n), "det and rank disagree on whether the matrix is singular"
            record(a.out, {
                "case": f"blockdiag_{A.n}_of_{bs}x{bs}_p{p}", "blocks": len(Bk), "n": A.n, "prime": p, "det_ms": round(det_ms, 3), "rank_ms": round(rank_ms, 3),
                "wall_ratio_det_over_rank": round(det_ms / rank_ms, 3), "det_device_us": dst["device_us"], "rank_device_us": bst["device_us"],
                "device_ratio_det_over_rank": round(dst["device_us"] / max(bst["device_us"], 1), 3), "host_parity_us": dst["host_parity_us"], "det_of_csr_ms": round(whole_ms, 3), "det_stats": dst,
            })


if __name__ == "__main__":
    main()
