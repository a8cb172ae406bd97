"""Times the fused preconditioned steps (csrc/precond.hpp: S.precond_sequence) against the loop a caller can compose today on the
same SpMV handle, in the same run.  A rank step is two products: Y <- D2 A X, Z <- E A^T Y and the projection U^T Z; the composed
loop is a zeroing, SpMV.apply, a torch row scale, a zeroing, SpMV.apply(trans=True), a torch row scale and a torch dot per column
in int64.  A determinant step is one product: Y <- D A X and U^T Y; composed: a zeroing, SpMV.apply, a row scale, a dot.  The torch
scale and dot are stand-ins: products of two residues of a 32-bit prime overflow them, so the composed loop does not compute the
sequence, it only costs what computing it that way would.

The fused figure is the device time of the launches of one precond_sequence call (the library's HIP events, S.precond_stats:
uploads and the final copy are outside) divided by the steps; the composed figure is the time between two torch events around the
same number of steps.  Fused and composed rounds alternate; each figure is the median of `reps` rounds after `warmup` rounds.
Matrices: n rows with `row_nnz` random entries each (S.synth_csr).

Also one end-to-end S.wiedemann_rank at n = 10^4 beside S.rank of the same matrix (wall-clock seconds, one run each).

One JSON line per case, printed and appended to --out (profiles/precond_timing.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spasm_jl_amd as S  # noqa: E402


def record(out_path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def med(v, steps):
    return round(float(np.median(v)) / steps, 2), [round(min(v) / steps, 2), round(max(v) / steps, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rank-n", type=int, default=10000, help="0: leave the end-to-end rank out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precond_timing.jsonl"))
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    rng = np.random.default_rng(0x57ED)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            A = S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n)
            with S.SpMV(A) as op:
                for K in [int(v) for v in a.ks.split(",") if v]:
                    U, V = (S.balanced(rng.integers(0, p, size=(n, K), dtype=np.int64), p) for _ in range(2))
                    dl, dr = S.precond_diagonal(n, 1, 0, p), S.precond_diagonal(n, 1, 1, p)
                    tU, tV = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
                    tl, tr = torch.from_numpy(dl).cuda()[:, None], torch.from_numpy(dr).cuda()[:, None]
                    Y, Z0, Z1 = torch.zeros_like(tV), torch.zeros_like(tV), torch.zeros_like(tV)
                    acc = torch.zeros((a.steps, K), dtype=torch.int64, device=tV.device)

                    def fused(mode):
                        S.precond_sequence(op, mode, dl, dr, U, V, a.steps + 1)
                        return S.precond_stats()["sequence_device_us"]

                    def composed(mode):
                        X, Z = tV, Z0
                        for i in range(a.steps):
                            if mode:
                                Y.zero_()
                                op.apply(X, Y)
                                Y.mul_(tl)
                                Z.zero_()
                                op.apply(Y, Z, trans=True)
                                Z.mul_(tr)
                            else:
                                Z.zero_()
                                op.apply(X, Z)
                                Z.mul_(tl)
                            acc[i] = (tU * Z).sum(0, dtype=torch.int64)
                            X, Z = Z, (Z1 if Z is Z0 else Z0)

                    for mode, name in ((1, "rank"), (0, "det")):
                        for _ in range(a.warmup):
                            fused(mode)
                            composed(mode)
                        torch.cuda.synchronize()
                        tf, tc = [], []
                        for _ in range(a.reps):   # alternating, so that both see the same machine
                            tf.append(fused(mode))
                            tc.append(event_ms(torch, lambda: composed(mode)) * 1e3)
                        f, fmm = med(tf, a.steps)
                        c, cmm = med(tc, a.steps)
                        record(a.out, {"case": f"precond_{name}_n{n}_nnz{a.row_nnz}_K{K}_p{p}", "step": name, "n": n, "K": K, "prime": p,
                                       "steps": a.steps, "products_per_step": 1 + mode, "fused_us_per_step": f, "composed_us_per_step": c,
                                       "fused_min_max_us": fmm, "composed_min_max_us": cmm, "launches": S.precond_stats()["launches"]})
            del A
    if a.rank_n > 0:
        n, p = a.rank_n, 65521
        A = S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n)
        t0 = time.perf_counter()
        rw = S.wiedemann_rank(A, tries=1)
        t1 = time.perf_counter()
        st = S.precond_stats()
        re = S.rank(A)
        t2 = time.perf_counter()
        record(a.out, {"case": f"rank_end_to_end_n{n}_nnz{a.row_nnz}_p{p}", "n": n, "prime": p, "wiedemann_rank": list(rw), "rank": int(re),
                       "wiedemann_seconds": round(t1 - t0, 3), "elimination_seconds": round(t2 - t1, 3), "products": st["products"],
                       "sequence_device_us": st["sequence_device_us"], "bm_device_us": st["bm_device_us"]})


if __name__ == "__main__":
    main()
