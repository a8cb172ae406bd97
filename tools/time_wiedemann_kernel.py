"""Times the kernel routine (csrc/colechelon.hpp) on the device of this run.

kernel   S.wiedemann_kernel on a dim x dim matrix of about `row_nnz` entries a row whose last `nullity` rows are combinations of two
         earlier rows, for nullity in --nullities and b in --bs: wall-clock seconds with and without certify and, from the
         counters of the uncertified call divided by its tries, the device microseconds per try of the sequence, the recurrence,
         Horner plus check, and the echelon form.  Medians of `reps` after one warm-up.
elim     S.kernel of the same matrix (elimination, with fill-in): wall-clock seconds, once per matrix.
solve    one try's Horner half beside S.block_wiedemann_solve at the same b on the same operator (K = b right-hand sides, tries=1):
         the Horner + check device microseconds of either.
echelon  S.column_echelon alone at rows = --echelon-rows and K in (8, 64) on a random full-rank block: device microseconds (the K
         columns, the read-back and the permutation; the copies to and from the host are outside), the bytes it must move
         (rows * K * 4 read and written per pivot column) and the fraction of --hbm-peak-gbs that this is.

One JSON line per case, printed and appended to --out (profiles/wiedemann_kernel_timing.jsonl)."""
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


def planted(n, row_nnz, nullity, p):
    """n x n, a non-zero diagonal; the last `nullity` rows are 2 * row(2 j) + 3 * row(2 j + 1)"""
    A = S.synth_csr(1, n, n, row_nnz=row_nnz, prime=p, seed=0x5A5A0000 + n)
    rows = []
    for i, r in enumerate(A.rows()):
        rows.append(sorted([(c, v) for c, v in r if c != i] + [(i, 1 + i % 7)]))
    for j in range(nullity):
        acc = {}
        for src, f in ((2 * j, 2), (2 * j + 1, 3)):
            for c, v in rows[src]:
                acc[c] = (acc.get(c, 0) + f * v) % p
        rows[n - 1 - j] = sorted((c, int(S.balanced(np.array([v]), p)[0])) for c, v in acc.items() if v)
    return S.CSR.from_rows(rows, n, prime=p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=10000)
    ap.add_argument("--row-nnz", type=int, default=10)
    ap.add_argument("--nullities", default="1,8,40")
    ap.add_argument("--bs", default="4,8,16")
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--echelon-rows", type=int, default=1000000)
    ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0)
    ap.add_argument("--skip-elimination", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiedemann_kernel_timing.jsonl"))
    a = ap.parse_args()
    assert S._abi.lib().spasm_amd_device_count() > 0, "no GPU: nothing is measured without one"
    rng = np.random.default_rng(0xB10C6)
    n = a.dim
    for p in [int(v) for v in a.primes.split(",") if v]:
        for k in (8, 64):
            X = S.balanced(rng.integers(0, p, size=(a.echelon_rows, k), dtype=np.int64), p)
            S.column_echelon(X, p)
            us = []
            for _ in range(a.reps):
                E, piv = S.column_echelon(X, p)
                us.append(S.wiedemann_kernel_stats()["echelon_device_us"])
            moved = 2.0 * a.echelon_rows * k * 4 * len(piv)
            t = float(np.median(us))
            record(a.out, {"case": f"column_echelon_rows{a.echelon_rows}_K{k}_p{p}", "rows": a.echelon_rows, "K": k, "prime": p,
                           "rank": len(piv), "device_us": t, "min_max_us": [min(us), max(us)], "bytes_moved": moved,
                           "gb_per_s": round(moved / t / 1e3, 1), "fraction_of_hbm_peak": round(moved / t / 1e3 / a.hbm_peak_gbs, 3),
                           "hbm_peak_gbs": a.hbm_peak_gbs})
            del X, E
        for nullity in [int(v) for v in a.nullities.split(",") if v]:
            A = planted(n, a.row_nnz, nullity, p)
            if not a.skip_elimination:
                t0 = time.perf_counter()
                Kr = S.kernel(S.transpose(A))   # S.kernel gives x with x B = 0: B = A^T for A x = 0
                record(a.out, {"case": f"elimination_kernel_n{n}_nullity{nullity}_p{p}", "n": n, "nullity": nullity, "prime": p,
                               "vectors": Kr.n, "seconds": round(time.perf_counter() - t0, 4)})
                del Kr
            with S.SpMV(A) as op:
                for b in [int(v) for v in a.bs.split(",") if v]:
                    S.wiedemann_kernel(op, b=b, seed=1)
                    plain, cert, per_try = [], [], []
                    for _ in range(a.reps):   # alternating, so that both see the same machine
                        t0 = time.perf_counter()
                        N, piv, _ = S.wiedemann_kernel(op, b=b, seed=1)
                        t1 = time.perf_counter()
                        st = S.wiedemann_kernel_stats()
                        Nc, _, complete = S.wiedemann_kernel(op, b=b, seed=1, certify=True)
                        t2 = time.perf_counter()
                        sc = S.wiedemann_kernel_stats()
                        plain.append(t1 - t0)
                        cert.append(t2 - t1)
                        tr = max(st["tries"], 1)
                        per_try.append([st[key] / tr for key in ("sequence_device_us", "bm_device_us", "horner_device_us", "echelon_device_us")])
                    med = [int(np.median([x[i] for x in per_try])) for i in range(4)]
                    record(a.out, {"case": f"wiedemann_kernel_n{n}_nnz{a.row_nnz}_nullity{nullity}_b{b}_p{p}", "n": n, "nullity": nullity, "b": b,
                                   "prime": p, "found": int(N.shape[1]), "tries": st["tries"], "found_certified": int(Nc.shape[1]),
                                   "tries_certified": sc["tries"], "complete": bool(complete), "seconds": round(float(np.median(plain)), 4),
                                   "seconds_certified": round(float(np.median(cert)), 4), "sequence_us_per_try": med[0],
                                   "bm_us_per_try": med[1], "horner_check_us_per_try": med[2], "echelon_us_per_try": med[3],
                                   "products": st["products"], "certify_products": sc["certify_products"], "candidates": st["candidates"],
                                   "accepted": st["accepted"], "dependent": st["dependent"]})
                    B = S.balanced(rng.integers(0, p, size=(n, b), dtype=np.int64), p)
                    S.block_wiedemann_solve(op, B, b=b, tries=1)
                    hs = []
                    for _ in range(a.reps):
                        S.block_wiedemann_solve(op, B, b=b, tries=1)
                        hs.append(S.block_solve_stats()["horner_device_us"])
                    record(a.out, {"case": f"horner_half_n{n}_b{b}_nullity{nullity}_p{p}", "n": n, "b": b, "prime": p,
                                   "kernel_horner_check_us_per_try": med[2], "block_solve_horner_check_us": int(np.median(hs))})
            del A


if __name__ == "__main__":
    main()
