"""Times the exact sparse products on resident handles (csrc/spgemm.hpp): (i) BASELINE config 3 squared (n x n, 20 entries per
row, p = 65521) at 1/10 and full size, (ii) a Macaulay-like synth_csr(2, ...) times its transpose at 200k x 80k, (iii) L U of an
L = True factorization.  Per case, from DeviceCSR.stats() (HIP events inside the library) over --reps products after a warm-up:
ms of the size / numeric / compact steps (medians), products per second (flops / numeric ms), output entries per second, the
algorithm's own bytes over the time of all three steps as a fraction of 8 TB/s, rows per path; upload and download by the host
clock, apart.  Algorithmic bytes: 8 (nnz A + flops) read (entries of A, the rows of B they name) + 16 rows of A + 8 cap written
and 8 entries read and written again by the compaction.  Yardstick: scipy.sparse CSR x CSR in int64 on the host, ONE thread,
values reduced afterwards (p < 2^16) -- what the reference's host path amounts to, not a tuned competitor.  One JSON line per case.
Kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402


def host_product_ms(A, B):
    import scipy.sparse as sp

    def to_sp(M):
        k = S.nnz(M)
        return sp.csr_matrix((M.x[:k].astype(np.int64), M.j[:k].astype(np.int64), np.asarray(M.p)), shape=M.shape)

    a, b = to_sp(A), to_sp(B)
    t0 = time.perf_counter()
    c = a @ b
    c.data %= A.prime
    c.eliminate_zeros()
    c.sort_indices()
    return (time.perf_counter() - t0) * 1e3


def case(name, A, B, reps, warmup, host):
    t0 = time.perf_counter()
    a = S.DeviceCSR(A)
    b = a if B is A else S.DeviceCSR(B)
    up = (time.perf_counter() - t0) * 1e3
    sts = []
    for r in range(warmup + reps):
        c = a @ b
        if r >= warmup:
            sts.append(c.stats())
        if r < warmup + reps - 1:
            c.close()
    t0 = time.perf_counter()
    C = c.download()
    down = (time.perf_counter() - t0) * 1e3
    st = sts[-1]
    ms = {k: float(np.median([s[k] for s in sts])) for k in ("ms_size", "ms_numeric", "ms_compact")}
    total = sum(ms.values())
    nbytes = 8 * (S.nnz(A) + st["flops"]) + 16 * A.n + 8 * (st["scratch_bytes"] // 8) + 16 * st["entries"]
    out = {
        "case": name, "A": list(A.shape), "B": list(B.shape), "prime": A.prime, "nnz_A": S.nnz(A), "nnz_B": S.nnz(B), "flops": st["flops"], "entries": st["entries"],
        **{k: round(v, 3) for k, v in ms.items()},
        "Gproducts_s": round(st["flops"] / max(ms["ms_numeric"], 1e-6) / 1e6, 2), "Gentries_s": round(st["entries"] / max(total, 1e-6) / 1e6, 2),
        "bytes": nbytes, "frac_8TBs": round(nbytes / max(total, 1e-6) / 1e6 / 8000, 4),
        "rows_tiny": st["rows_tiny"], "rows_hash": st["rows_hash"], "rows_global": st["rows_global"], "chunks": st["chunks"], "max_bound": st["max_bound"],
        "upload_ms": round(up, 1), "download_ms": round(down, 1),
    }
    assert S.nnz(C) == st["entries"]
    if host and A.prime < 65536:
        out["scipy_int64_one_thread_ms"] = round(host_product_ms(A, B), 1)
    c.close()
    a.close()
    b.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="c3_tenth,c3_full,macaulay,lu")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy yardstick")
    a = ap.parse_args()
    p = 65521
    for name in a.cases.split(","):
        if name in ("c3_tenth", "c3_full"):
            n = 100_000 if name == "c3_tenth" else 1_000_000
            A = S.synth_csr(1, n, n, row_nnz=20, prime=p, seed=0x5A5A0003)
            case(name, A, A, a.reps, a.warmup, not a.no_host)
        elif name == "macaulay":
            A = S.synth_csr(2, 200_000, 80_000, row_nnz=40, prime=p, seed=0x5A5A0005)
            case(name, A, S.transpose(A), a.reps, a.warmup, not a.no_host)
        elif name == "lu":
            A = S.synth_csr(1, 5_000, 5_000, row_nnz=4, prime=p, seed=0x5A5A0009)
            fact = S.echelonize(A, L=True, enable_greedy_pivot_search=False)
            case(name, fact.L, fact.U, a.reps, a.warmup, not a.no_host)
        else:
            raise SystemExit(f"unknown case {name}")


if __name__ == "__main__":
    main()
