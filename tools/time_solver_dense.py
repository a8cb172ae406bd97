"""Times the dense apply of the resident solver (BatchSolver.solve_dense on torch tensors that stay on the device) against
BatchSolver.solve on the same right-hand sides as host CSR, the cases of tools/time_solver.py: (i) N = 100, 1000, 10000 systems of
50 x 60 (synth_csr kind 0, density 0.1) with K = 1, 4, 64 right-hand sides each (every second one y * A, the others random) at
p = 65521 and p = 127, (ii) a block matrix of 5000 connected components of mixed sizes with 1000 right-hand sides.  Per case: wall
microseconds per call of solve_dense (the call and a synchronise) and of solve, and device microseconds of both: HIP events around
the call for solve_dense (so it contains the host's argument checks and launch, during which the device idles: an upper bound of
the kernels, loose for small cases), the figure solver_stats() reports for solve (its kernels alone).  Medians of --reps calls after --warmup.  Before anything is
timed the results are compared entry for entry.  One JSON line per case, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402
from time_batch import block_matrix  # noqa: E402
from time_solver import rhs_for, timed  # noqa: E402


def dense_of(B):
    """the K x m CSR of right-hand sides as the m x K int32 array of solve_dense"""
    K, m = B.shape
    D = np.zeros((m, K), dtype=np.int32)
    for k in range(K):
        e0, e1 = int(B.p[k]), int(B.p[k + 1])
        D[np.asarray(B.j[e0:e1]), k] = np.asarray(B.x[e0:e1])
    return D


def same(Xd, X, col0=0):
    """rows col0 .. of the dense result against the K x n CSR of solve"""
    K, n = X.shape
    D = np.zeros((n, K), dtype=np.int32)
    for k in range(K):
        e0, e1 = int(X.p[k]), int(X.p[k + 1])
        D[np.asarray(X.j[e0:e1]), k] = np.asarray(X.x[e0:e1])
    return np.array_equal(Xd[col0:col0 + n], D)


def time_dense(sv, Bt, Xt, reps, warmup):
    """(wall us, device us) of solve_dense: medians; the wall time ends with a synchronise, the device time lies between two events
    recorded around the Python call, host launch latency included"""
    wall, dev = [], []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        sv.solve_dense(Bt, X=Xt)
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            wall.append((time.perf_counter() - t0) * 1e6)
            dev.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(wall)), float(np.median(dev))


def report(out_path, line):
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")


def case(a, name, sv, rhs_list, Bd, nsys, solve):
    """compare, then time; rhs_list: what solve takes; Bd: the same right-hand sides as one dense array"""
    Bt = torch.from_numpy(Bd).cuda()
    Xt = torch.zeros((sv.dense_info()["rows"], Bd.shape[1]), dtype=torch.int32, device="cuda")
    X, ok = solve()
    Xd, okd = sv.solve_dense(Bt, X=Xt)
    Xd, okd = Xd.cpu().numpy(), okd.cpu().numpy()
    if isinstance(X, list):
        r0 = 0
        for i, x in enumerate(X):
            assert same(Xd, x, r0) and np.array_equal(okd[i], ok[i]), f"solve_dense and solve disagree on system {i}"
            r0 += x.shape[1]
    else:
        assert same(Xd, X) and np.array_equal(okd, ok), "solve_dense and solve disagree"
    dense_us, dense_dev = time_dense(sv, Bt, Xt, a.reps, a.warmup)
    sparse_us, _ = timed(solve, a.reps, a.warmup)
    st = S.solver_stats()
    info = sv.dense_info()
    report(a.out, {
        "case": name, "systems": nsys, "K": int(Bd.shape[1]), "solve_dense_wall_us": round(dense_us, 1), "solve_wall_us": round(sparse_us, 1),
        "ratio_solve_over_solve_dense": round(sparse_us / max(dense_us, 1e-9), 2), "solve_dense_device_us": round(dense_dev, 1), "solve_device_us": st["device_us"],
        "solve_dense_wall_us_per_system": round(dense_us / nsys, 3), "solve_wall_us_per_system": round(sparse_us / nsys, 3), "unsolved": int((~okd).sum()),
        "plan_jobs": info["plan_jobs"], "plan_launches": info["plan_launches"], "plans_built": info["plans_built"],
    })


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--rhs", default="1,4,64")
    ap.add_argument("--primes", default="65521,127")
    ap.add_argument("--components", type=int, default=5000, help="0: skip the block case")
    ap.add_argument("--rhs-rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "solver_dense_timing.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_solver_dense.py needs a GPU: there is nothing to time without one")
    for p in [int(v) for v in a.primes.split(",")]:
        for N in [int(v) for v in a.sizes.split(",")]:
            mats = [S.synth_csr(0, 50, 60, density=0.1, prime=p, seed=0x501E0000 + k) for k in range(N)]
            with S.BatchSolver(mats) as sv:
                for K in [int(v) for v in a.rhs.split(",")]:
                    rng = np.random.default_rng(0x501E + K)
                    rhs = [rhs_for(A, K, p, rng) for A in mats]
                    Bd = np.concatenate([dense_of(B) for B in rhs], axis=0)
                    case(a, f"50x60_p{p}_N{N}_K{K}", sv, rhs, Bd, N, lambda: sv.solve(rhs))
                    del rhs, Bd
    if a.components > 0:
        p = 42013
        A = block_matrix(a.components, 0xB10C, p)
        rng = np.random.default_rng(0xB10C)
        rows = A.rows()
        rr = []
        for k in range(a.rhs_rows):
            acc = {}
            for i in rng.integers(0, A.n, size=4):
                f = int(rng.integers(1, p))
                for c, v in rows[int(i)]:
                    acc[c] = (acc.get(c, 0) + f * v) % p
            if k % 4 == 3:
                acc[int(rng.integers(0, A.m))] = 1
            rr.append(sorted((c, v - p if 2 * v > p else v) for c, v in acc.items() if v))
        Rhs = S.CSR.from_rows(rr, A.m, prime=p)
        with S.DeviceBlocks(A) as db, db.solver() as sv:
            case(a, f"block_{len(db)}_components_rhs{a.rhs_rows}", sv, Rhs, dense_of(Rhs), len(db), lambda: sv.solve(Rhs))


if __name__ == "__main__":
    main()
