"""Times the characteristic-polynomial entries (csrc/charpoly.hpp) against det_batch on the same inputs: N random dense n x n
matrices per case (4096 of 32 x 32, 1024 of 110 x 110, 256 of 181 x 181 on the LDS path; one 512 x 512 and one 1024 x 1024 on the
global path, where det_batch takes the general path of echelonize with L) at each of --primes.  Per case: wall ms of both calls
(median of --reps after --warmup calls), the device microseconds that charpoly_stats reports for the last call (HIP events around
the launches) and, on the LDS path, those of det_stats, both ratios charpoly / det, and the counters of charpoly_stats.  The
constant term must be (-1)^n times the determinant.  One JSON line per case, printed and appended to --out
(profiles/charpoly_timing.jsonl)."""
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


def record(out_path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="4096x32,1024x110,256x181,1x512,1x1024", help="N x n, comma separated")
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charpoly_timing.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0xC4A2)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for case in [c for c in a.cases.split(",") if c]:
            N, n = (int(v) for v in case.split("x"))
            mats = [dense_csr(rng, n, p) for _ in range(N)]
            cp_ms, pols = timed(lambda: S.charpoly_batch(mats), a.reps, a.warmup)
            cst = S.charpoly_stats()
            det_ms, dets = timed(lambda: S.det_batch(mats), a.reps, a.warmup)
            dst = S.det_stats()
            sign = -1 if n % 2 else 1
            assert [int(c[0]) for c in pols] == [int(S.balanced(sign * int(d), p)) for d in dets.tolist()], "constant term and determinant disagree"
            lds = cst["lds_path"] > 0
            cp_us = cst["lds_device_us"] if lds else cst["global_device_us"]
            rec = {
                "case": f"{N}x{n}x{n}_p{p}", "matrices": N, "n": n, "prime": p, "path": "lds" if lds else "global", "charpoly_ms": round(cp_ms, 3),
                "det_ms": round(det_ms, 3), "wall_ratio_charpoly_over_det": round(cp_ms / det_ms, 3), "charpoly_device_us": cp_us,
            }
            if lds:   # (the general path of det has no device figure of its own)
                rec["det_device_us"] = dst["device_us"]
                rec["device_ratio_charpoly_over_det"] = round(cp_us / max(dst["device_us"], 1), 3)
            rec["charpoly_stats"] = cst
            record(a.out, rec)
            del mats


if __name__ == "__main__":
    main()
