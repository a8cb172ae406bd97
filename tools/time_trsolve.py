"""Times the dense triangular solve on the U of BASELINE config 3 at 1/SCALE (default 10: 100k x 100k, 20 entries per row,
p = 65521, factorized by S.echelonize as tools/time_c3.py does): S.TriangularSolver.from_lu (create, host clock) and
spasm_amd_trsolve_apply_dev on torch device tensors for k = 1, 8, 32 (device events over --reps applies after a warm-up).  For
comparison, spasm_amd_triangular_solve (S.sparse_triangular_solve) on the same k vectors given as CSR rows, by the host clock.
Prints one JSON line.

The traffic floor of one apply is one read of U: 8 bytes (column, value) per entry; GB/s against 8 TB/s, the MI355X's HBM peak.
Kernel times: run under `rocprofv3 --kernel-trace --stats`."""
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
    ap.add_argument("--scale", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--no-compare", action="store_true")
    a = ap.parse_args()
    n = 1_000_000 // a.scale
    p = 65521
    A = S.synth_csr(1, n, n, row_nnz=20, prime=p, seed=0x5A5A0003)
    t0 = time.perf_counter()
    fact = S.echelonize(A)
    out = {"matrix": f"config 3 at 1/{a.scale}: {n} x {n}, p = {p}", "echelonize_s": round(time.perf_counter() - t0, 2)}
    U = fact.U
    nnz = S.nnz(U)
    out.update({"rank": fact.r, "nnz_U": nnz, "reps": a.reps, "cases": []})
    t0 = time.perf_counter()
    ts = S.TriangularSolver.from_lu(fact)
    out["create_s"] = round(time.perf_counter() - t0, 2)
    out["plan"] = ts.stats()
    print(f"echelonize {out['echelonize_s']} s, create {out['create_s']} s, {out['plan']}", file=sys.stderr, flush=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    floor = 8 * nnz
    for k in [int(s) for s in a.ks.split(",")]:
        Y = torch.randint(-(p // 2), p // 2 + 1, (U.n, k), dtype=torch.int32, device="cuda", generator=gen)
        B0 = torch.from_numpy(_xT(U, Y.cpu().numpy(), p)).cuda() if k == 1 else torch.randint(-(p // 2), p // 2 + 1, (U.m, k), dtype=torch.int32,
                                                                                           device="cuda", generator=gen)
        B = B0.clone()
        for _ in range(a.warmup):
            B.copy_(B0)
            X, ok = ts.solve(B)
        torch.cuda.synchronize()
        exact = bool(ok.all()) and bool(torch.equal(X, Y)) if k == 1 else None  # b = y U: x == y
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ts.solve(B, X)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        gbs = floor / ms / 1e6
        out["cases"].append({"k": k, "ms": round(ms, 3), "floor_bytes": floor, "GB_s": round(gbs, 1), "frac_8TBs": round(gbs / 8000, 4),
                             "exact": exact})
    ts.close()
    if not a.no_compare:
        cmp = []
        for k in [int(s) for s in a.ks.split(",")]:
            rng = np.random.default_rng(k)
            Bd = rng.integers(-(p // 2), p // 2 + 1, size=(k, U.m))
            Bs = S.CSR(Bd.T.copy(), prime=p)  # stores the transpose: k rows of m entries
            try:
                t0 = time.perf_counter()
                S.api._triangular_solve(U, Bs, fact.qinv)
                cmp.append({"k": k, "s": round(time.perf_counter() - t0, 3)})
            except Exception as e:  # reported, not hidden
                cmp.append({"k": k, "failed": str(e)[:200]})
        out["spasm_amd_triangular_solve"] = cmp
    print(json.dumps(out), flush=True)


def _xT(U, Y, p):
    """b = Y^T U as m x k int32 (exact, on the device through the resident SpMV)"""
    with S.SpMV(U) as op:
        return op.apply(np.ascontiguousarray(Y), trans=True)


if __name__ == "__main__":
    main()
