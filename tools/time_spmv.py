"""Times the exact products on BASELINE config 3 (1M x 1M, 20 entries per row, p = 65521): A X and x A through the resident
operator (spasm_amd_spmv_apply_dev on torch device tensors) for k = 1, 8, 32, by device events over --reps applies after a
warm-up, and the one-shot spasm_Axpy (host arrays, upload included) by the host clock.  Prints one JSON line and, with --out,
appends it to that file.

Algorithmic bytes of one apply: 8 nnz (the (j, x) entries) + 12 rows (row start and length) + 4k (cols + 2 rows) (X read once,
Y read and written); GB/s against 8 TB/s, the MI355X's HBM peak.  Kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--prime", type=int, default=65521)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = a.prime
    A = S.synth_csr(1, a.n, a.n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0003)
    nnz = S.nnz(A)
    n, m = A.shape
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = {"matrix": f"config 3: {n} x {m}, {nnz} entries, p = {p}", "reps": a.reps, "cases": []}
    with S.SpMV(A) as op:
        for trans in (False, True):
            rows, cols = (m, n) if trans else (n, m)
            for k in [int(s) for s in a.ks.split(",")]:
                X = torch.randint(-(p // 2), p // 2 + 1, (cols, k), dtype=torch.int32, device="cuda", generator=gen)
                Y = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
                for _ in range(a.warmup):
                    op.apply(X, Y, trans=trans)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    op.apply(X, Y, trans=trans)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.reps
                nbytes = 8 * nnz + 12 * rows + 4 * k * (cols + 2 * rows)
                gbs = nbytes / ms / 1e6
                out["cases"].append({"op": "x A" if trans else "A X", "k": k, "ms": round(ms, 5), "bytes": nbytes, "GB_s": round(gbs, 1),
                                     "frac_8TBs": round(gbs / 8000, 4)})
    x = S.balanced(np.random.default_rng(2).integers(0, p, size=m), p)
    walls = []
    for _ in range(3):
        y = np.zeros(n, dtype=np.int32)
        t0 = time.perf_counter()
        S.axpy(A, x, y)
        walls.append((time.perf_counter() - t0) * 1e3)
    out["one_shot_spasm_Axpy_ms"] = round(float(np.median(walls)), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
