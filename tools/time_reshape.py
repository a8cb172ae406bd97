"""Times the structural operations on resident matrices (csrc/reshape.hpp): D.T, D.permute(p, q), hcat(D, D), vcat(D, D) on (i)
BASELINE config 3 (n x n, 20 entries per row, p = 65521) at 1/10 and full size and (ii) a Macaulay-like synth_csr(2, ...) at
200k x 80k.  Per case and operation, over --reps runs after --warmup: device microseconds of the count / move / order steps from
DeviceCSR.stats() (HIP events inside the library; medians) and the wall time of the call (median, host clock, the call returns
after the device has finished).  Yardstick: the route that exists without these operations -- download(), the host operation
(S.transpose; numpy index arithmetic on the CSR arrays for the others), DeviceCSR(...) -- by the host clock, --host-reps times
(median), with its three parts apart.  The device result is compared with the host route's (equals) once per operation.
One JSON line per case and operation, printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spasm_jl_amd as S  # noqa: E402


def arrays(A):
    k = S.nnz(A)
    return np.asarray(A.p, dtype=np.int64), A.j[:k], A.x[:k]


def host_transpose(A, P, Q):
    return S.transpose(A)


def host_permute(A, P, Q):
    ptr, j, x = arrays(A)
    lens = np.diff(ptr)
    nl = lens[P]
    nptr = np.concatenate([[0], np.cumsum(nl)])
    src = np.repeat(ptr[P] - nptr[:-1], nl) + np.arange(int(nptr[-1]))  # position in A of every entry of the result, row after row
    qinv = np.empty(A.m, dtype=np.int32)
    qinv[Q] = np.arange(A.m, dtype=np.int32)
    nj = qinv[j[src]]
    order = np.lexsort((nj, np.repeat(np.arange(A.n), nl)))
    return S.CSR.from_arrays(A.n, A.m, nptr, nj[order], x[src][order], prime=A.prime)


def host_vcat(A, P, Q):
    ptr, j, x = arrays(A)
    return S.CSR.from_arrays(2 * A.n, A.m, np.concatenate([ptr, ptr[1:] + ptr[-1]]), np.concatenate([j, j]), np.concatenate([x, x]), prime=A.prime)


def host_hcat(A, P, Q):
    ptr, j, x = arrays(A)
    row = np.repeat(np.arange(A.n), np.diff(ptr))
    order = np.argsort(np.concatenate([row, row]), kind="stable")  # row i of the left operand, then row i of the right one
    return S.CSR.from_arrays(A.n, 2 * A.m, 2 * ptr, np.concatenate([j, j + np.int32(A.m)])[order], np.concatenate([x, x])[order], prime=A.prime)


OPS = {
    "transpose": (lambda d, P, Q: d.T, host_transpose),
    "permute": (lambda d, P, Q: d.permute(P, Q), host_permute),
    "hcat": (lambda d, P, Q: S.hcat(d, d), host_hcat),
    "vcat": (lambda d, P, Q: S.vcat(d, d), host_vcat),
}


def med(v):
    return float(np.median(v))


def case(name, A, a, out):
    rng = np.random.default_rng(11)
    P, Q = rng.permutation(A.n), rng.permutation(A.m)
    d = S.DeviceCSR(A)
    for op in a.ops.split(","):
        dev, host = OPS[op]
        sts, wall = [], []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            c = dev(d, P, Q)
            t1 = time.perf_counter()
            if r >= a.warmup:
                sts.append(c.stats())
                wall.append((t1 - t0) * 1e6)
            if r < a.warmup + a.reps - 1:
                c.close()
        st = sts[-1]
        rec = {
            "case": name, "op": op, "A": list(A.shape), "prime": A.prime, "nnz_A": S.nnz(A), "result": list(c.shape), "entries": st["entries"],
            "count_us": round(med([s["ms_size"] for s in sts]) * 1e3, 1), "move_us": round(med([s["ms_numeric"] for s in sts]) * 1e3, 1),
            "order_us": round(med([s["ms_compact"] for s in sts]) * 1e3, 1), "wall_us": round(med(wall), 1),
            "rows_wave": st["rows_tiny"], "rows_group": st["rows_hash"], "rows_long": st["rows_global"], "longest_row": st["max_bound"],
            "scratch_bytes": st["scratch_bytes"],
        }
        parts = []
        for r in range(a.host_reps):
            t0 = time.perf_counter()
            H = d.download()
            t1 = time.perf_counter()
            H2 = host(H, P, Q)
            t2 = time.perf_counter()
            e = S.DeviceCSR(H2)
            t3 = time.perf_counter()
            parts.append(((t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6))
            if r < a.host_reps - 1:
                e.close()
        if parts:
            rec["same_as_host_route"] = bool(c.equals(e))
            e.close()
            rec["host_download_us"], rec["host_op_us"], rec["host_upload_us"] = (round(med([q[k] for q in parts]), 1) for k in range(3))
            rec["host_route_us"] = round(med([sum(q) for q in parts]), 1)
            rec["host_over_device"] = round(rec["host_route_us"] / max(rec["wall_us"], 1e-3), 2)
        c.close()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1, help="runs of the download / host operation / upload route (0: skip it)")
    ap.add_argument("--cases", default="c3_tenth,c3_full,macaulay")
    ap.add_argument("--ops", default="transpose,permute,hcat,vcat")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reshape_timing.jsonl"))
    a = ap.parse_args()
    p = 65521
    with open(a.out, "w") as out:
        for name in a.cases.split(","):
            if name in ("c3_tenth", "c3_full"):
                n = 100_000 if name == "c3_tenth" else 1_000_000
                A = S.synth_csr(1, n, n, row_nnz=20, prime=p, seed=0x5A5A0003)
            elif name == "macaulay":
                A = S.synth_csr(2, 200_000, 80_000, row_nnz=40, prime=p, seed=0x5A5A0005)
            else:
                raise SystemExit(f"unknown case {name}")
            case(name, A, a, out)


if __name__ == "__main__":
    main()
