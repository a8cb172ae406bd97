"""Times the block Wiedemann solve (csrc/block_horner.hpp) against the scalar solve of the same build, on the same matrix, in the
same run.

step     one block Horner step beside one K-column Horner step of S.poly_apply on the same SpMV handle: both run on device tensors
         on one stream, timed by events around the whole call (the upload of the coefficient table included) and divided by the
         `steps` products.  The two alternate; each figure is the median of `reps` rounds after `warmup` rounds.
solve    S.block_wiedemann_solve beside S.wiedemann_solve at the same K (the scalar route is untouched by the block solve) on a
         matrix with a non-zero diagonal and random right-hand sides: wall-clock seconds and the device microseconds of either's
         stats (sequence, recurrence, Horner + check), alternating, medians of `solve_reps` after one warm-up each.

Matrices: n rows with `row_nnz` random entries each (S.synth_csr; the diagonal is set to 1 + (i mod 7) so that the matrix is
non-singular with fair probability).  One JSON line per case, printed and appended to --out (profiles/block_solve_timing.jsonl)."""
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


def med(v, div=1.0, nd=2):
    return round(float(np.median(v)) / div, nd), [round(min(v) / div, nd), round(max(v) / div, nd)]


def with_diagonal(A, p):
    out = []
    for i, r in enumerate(A.rows()):
        out.append(sorted([(c, v) for c, v in r if c != i] + [(i, 1 + i % 7)]))
    return S.CSR.from_rows(out, A.m, prime=p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000")
    ap.add_argument("--bs", default="4,8,16")
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_solve_timing.jsonl"))
    a = ap.parse_args()
    assert S._abi.lib().spasm_amd_device_count() > 0, "no GPU: nothing is measured without one"
    import torch

    rng = np.random.default_rng(0xB10C5)
    bs = [int(v) for v in a.bs.split(",") if v]
    for p in [int(v) for v in a.primes.split(",") if v]:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            A = with_diagonal(S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n), p)
            with S.SpMV(A) as op:
                for b in bs:
                    for k in (1, b):
                        tV = torch.from_numpy(S.balanced(rng.integers(0, p, size=(n, b), dtype=np.int64), p)).cuda()
                        tVk = tV[:, :k].contiguous()
                        Cs = S.balanced(rng.integers(0, p, size=(a.steps + 1, b, k), dtype=np.int64), p)
                        polys = [S.balanced(rng.integers(1, p, size=a.steps + 1, dtype=np.int64), p) for _ in range(k)]

                        def timed(fn):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            e1.synchronize()
                            return e0.elapsed_time(e1) * 1000.0

                        block = lambda: S.block_poly_apply(op, Cs, tV)
                        scalar = lambda: S.poly_apply(op, polys, tVk)
                        for _ in range(a.warmup):
                            timed(block)
                            timed(scalar)
                        tb, ts = [], []
                        for _ in range(a.reps):   # alternating, so that both see the same machine
                            tb.append(timed(block))
                            ts.append(timed(scalar))
                        fb, bmm = med(tb, a.steps)
                        fs, smm = med(ts, a.steps)
                        record(a.out, {"case": f"block_horner_step_n{n}_nnz{a.row_nnz}_b{b}_K{k}_p{p}", "n": n, "b": b, "K": k, "prime": p,
                                       "steps": a.steps, "block_horner_us_per_step": fb, "horner_K_us_per_step": fs, "block_min_max_us": bmm,
                                       "horner_min_max_us": smm})
                for b in bs:
                    for k in (1, b):
                        B = S.balanced(rng.integers(0, p, size=(n, k), dtype=np.int64), p)
                        S.block_wiedemann_solve(op, B, b=b, tries=1)
                        S.wiedemann_solve(op, B, tries=1)
                        wb, ws, db, ds = [], [], [], []
                        for _ in range(a.solve_reps):
                            t0 = time.perf_counter()
                            Xb, sb = S.block_wiedemann_solve(op, B, b=b, tries=1)
                            t1 = time.perf_counter()
                            st = S.block_solve_stats()
                            Xs, ss = S.wiedemann_solve(op, B, tries=1)
                            t2 = time.perf_counter()
                            sw = S.wiedemann_stats()
                            wb.append(t1 - t0)
                            ws.append(t2 - t1)
                            db.append((st["sequence_device_us"], st["bm_device_us"], st["horner_device_us"]))
                            ds.append((sw["sequence_device_us"], sw["horner_device_us"]))
                        both = (sb == 1) & (ss == 1)
                        record(a.out, {"case": f"block_solve_n{n}_nnz{a.row_nnz}_b{b}_K{k}_p{p}", "n": n, "b": b, "K": k, "prime": p,
                                       "block_status": sb.tolist(), "wiedemann_status": ss.tolist(),
                                       "agree": bool(both.any() and (Xb[:, both] == Xs[:, both]).all()),
                                       "block_seconds": med(wb, nd=4)[0], "wiedemann_seconds": med(ws, nd=4)[0],
                                       "block_sequence_device_us": int(np.median([x[0] for x in db])),
                                       "block_bm_device_us": int(np.median([x[1] for x in db])),
                                       "block_horner_check_device_us": int(np.median([x[2] for x in db])),
                                       "wiedemann_sequence_bm_device_us": int(np.median([x[0] for x in ds])),
                                       "wiedemann_horner_check_device_us": int(np.median([x[1] for x in ds])),
                                       "block_products": st["products"], "wiedemann_products": sw["products"], "len": st["len"],
                                       "max_degree": st["max_degree"]})
            del A


if __name__ == "__main__":
    main()
