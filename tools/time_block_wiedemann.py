"""Times block Wiedemann (csrc/block_krylov.hpp, csrc/block_bm.hpp) against the scalar routines of the same build, on the same SpMV
handle, in the same run.

step     the device time of the launches of one S.block_sequence call (the library's HIP events, S.block_stats: uploads and the
         final copy are outside) divided by its steps, beside that of S.krylov_sequence with K = b on the same U, V
         (S.minpoly_stats).  The two alternate; each figure is the median of `reps` rounds after `warmup` rounds.
bm       the device time of S.block_berlekamp_massey on the block sequence of 2 * ceil(n / b) + 2 terms of that matrix, divided by
         the terms: one step is three launches (discrepancy, elimination, update).  Median of `bm_reps` runs after one.
det      S.block_wiedemann_det beside S.wiedemann_det(K=8) (untouched by block Wiedemann) on the same matrix with a non-zero
         diagonal: wall-clock seconds and the device microseconds of either's stats, alternating, medians of `det_reps`.

Matrices: n rows with `row_nnz` random entries each (S.synth_csr; for det the diagonal is set to 1 + (i mod 7) so that the matrix
is non-singular with fair probability).  One JSON line per case, printed and appended to --out
(profiles/block_wiedemann_timing.jsonl)."""
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
    rows = A.rows()
    out = []
    for i, r in enumerate(rows):
        r = [(c, v) for c, v in r if c != i] + [(i, 1 + i % 7)]
        out.append(sorted(r))
    return S.CSR.from_rows(out, A.m, prime=p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--bs", default="4,8,16")
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bm-reps", type=int, default=3)
    ap.add_argument("--det-sizes", default="10000", help="sizes of the end-to-end determinants (empty: none)")
    ap.add_argument("--det-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_wiedemann_timing.jsonl"))
    a = ap.parse_args()
    assert S._abi.lib().spasm_amd_device_count() > 0, "no GPU: nothing is measured without one"
    rng = np.random.default_rng(0xB10C)
    sizes = [int(v) for v in a.sizes.split(",") if v]
    det_sizes = [int(v) for v in a.det_sizes.split(",") if v]
    bs = [int(v) for v in a.bs.split(",") if v]
    for p in [int(v) for v in a.primes.split(",") if v]:
        for n in sizes:
            A = S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n)
            with S.SpMV(A) as op:
                for b in bs:
                    U, V = (S.balanced(rng.integers(0, p, size=(n, b), dtype=np.int64), p) for _ in range(2))

                    def block():
                        S.block_sequence(op, U, V, a.steps + 1)
                        return S.block_stats()["sequence_device_us"]

                    def scalar():
                        S.krylov_sequence(op, U, V, a.steps + 1)
                        return S.minpoly_stats()["sequence_device_us"]

                    for _ in range(a.warmup):
                        block()
                        scalar()
                    tb, ts = [], []
                    for _ in range(a.reps):   # alternating, so that both see the same machine
                        tb.append(block())
                        ts.append(scalar())
                    fb, bmm = med(tb, a.steps)
                    fs, smm = med(ts, a.steps)
                    record(a.out, {"case": f"block_step_n{n}_nnz{a.row_nnz}_b{b}_p{p}", "n": n, "b": b, "prime": p, "steps": a.steps,
                                   "block_us_per_step": fb, "krylov_K_eq_b_us_per_step": fs, "block_min_max_us": bmm, "krylov_min_max_us": smm,
                                   "launches": S.block_stats()["launches"]})
                    length = 2 * -(-n // b) + 2
                    seq = S.block_sequence(op, U, V, length)
                    seq_us = S.block_stats()["sequence_device_us"]
                    tm = []
                    for r in range(a.bm_reps + 1):
                        _, rowdeg = S.block_berlekamp_massey(seq, p)
                        if r:
                            tm.append(S.block_stats()["bm_device_us"])
                    fm, mmm = med(tm, length)
                    record(a.out, {"case": f"block_bm_n{n}_b{b}_p{p}", "n": n, "b": b, "prime": p, "len": length, "bm_us_per_step": fm,
                                   "bm_min_max_us": mmm, "bm_total_us": int(np.median(tm)), "sequence_total_us": seq_us,
                                   "degree_sum": int(rowdeg.sum()), "max_degree": int(rowdeg.max()), "launches": S.block_stats()["launches"]})
            if n in det_sizes:
                Ad = with_diagonal(A, p)
                want = S.wiedemann_det(Ad, K=8, tries=1)   # warm-up of the scalar route
                for b in bs:
                    S.block_wiedemann_det(Ad, b=b, tries=1)
                    wb, ws, db, ds = [], [], [], []
                    for _ in range(a.det_reps):
                        t0 = time.perf_counter()
                        got = S.block_wiedemann_det(Ad, b=b, tries=1)
                        t1 = time.perf_counter()
                        st = S.block_stats()
                        ref = S.wiedemann_det(Ad, K=8, tries=1)
                        t2 = time.perf_counter()
                        sp = S.precond_stats()
                        wb.append(t1 - t0)
                        ws.append(t2 - t1)
                        db.append((st["sequence_device_us"], st["bm_device_us"]))
                        ds.append((sp["sequence_device_us"], sp["bm_device_us"]))
                    record(a.out, {"case": f"block_det_n{n}_nnz{a.row_nnz}_b{b}_p{p}", "n": n, "b": b, "prime": p, "block_det": list(got),
                                   "wiedemann_det_K8": list(ref), "agree": bool(got[1] == 1 and ref[1] == 1 and got[0] == ref[0] and ref == want),
                                   "block_seconds": med(wb, nd=4)[0], "wiedemann_K8_seconds": med(ws, nd=4)[0],
                                   "block_sequence_device_us": int(np.median([x[0] for x in db])), "block_bm_device_us": int(np.median([x[1] for x in db])),
                                   "wiedemann_sequence_device_us": int(np.median([x[0] for x in ds])),
                                   "wiedemann_bm_device_us": int(np.median([x[1] for x in ds])), "block_steps": st["steps"],
                                   "wiedemann_products": sp["products"]})
            del A


if __name__ == "__main__":
    main()
