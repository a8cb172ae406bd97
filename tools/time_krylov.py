"""Times the fused Krylov step (csrc/krylov.hpp: S.krylov_sequence on torch tensors, the _dev entry) against the loop a caller could
write without it, on the same SpMV handle and the same tensors, in the same run: per step one zeroing of Y, one SpMV.apply
(spasm_amd_spmv_apply_dev) and one torch dot product per column, (U * Y).sum(0) in int64 -- a stand-in: products of two residues
of a 32-bit prime overflow such a sum, so the composed loop does not compute the sequence, it only costs what computing it that way
would.  Both are enqueued on the current stream and timed with device events around `steps` steps, after `warmup` untimed rounds;
the median of `reps` rounds is divided by the steps.  Matrices: n rows with `row_nnz` random entries each (S.synth_csr).

Also times S.berlekamp_massey on the sequence of a random monic polynomial of degree d with 2 d terms, in the LDS class and in the
device-memory class (device microseconds from the library's events, S.minpoly_stats, median of `reps`; d = 10^4 is 80 KB of LDS).

One JSON line per case, printed and appended to --out (profiles/krylov_timing.jsonl)."""
import argparse
import json
import os
import sys

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


def lfsr(f, init, count, p):
    """count terms of s[i + d] = -sum_j f[j] s[i + j] (the tool's own set-up, not timed): int64 with the products of two residues
    taken in two 16-bit halves of one factor"""
    d = len(f) - 1
    s = np.zeros(count, dtype=np.int64)
    s[:d] = np.asarray(init, dtype=np.int64) % p
    nf = np.array([(-int(x)) % p for x in f[:d]], dtype=np.int64)
    hi, lo = nf >> 16, nf & 0xFFFF
    for i in range(count - d):
        w = s[i: i + d]
        s[i + d] = (((w * hi % p) * 65536 + w * lo) % p).sum() % p
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bm-degrees", default="1000,10000")
    ap.add_argument("--bm-prime", type=int, default=4294967291)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_timing.jsonl"))
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    rng = np.random.default_rng(0x57ED)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            A = S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n)
            with S.SpMV(A) as op:
                for K in [int(v) for v in a.ks.split(",") if v]:
                    U = torch.from_numpy(S.balanced(rng.integers(0, p, size=(n, K), dtype=np.int64), p)).cuda()
                    V = torch.from_numpy(S.balanced(rng.integers(0, p, size=(n, K), dtype=np.int64), p)).cuda()
                    Y0, Y1 = torch.zeros_like(V), torch.zeros_like(V)
                    acc = torch.zeros((a.steps, K), dtype=torch.int64, device=V.device)

                    def fused():
                        return S.krylov_sequence(op, U, V, a.steps + 1)

                    def composed():
                        X, Y = V, Y0
                        for i in range(a.steps):
                            Y.zero_()
                            op.apply(X, Y)
                            acc[i] = (U * Y).sum(0, dtype=torch.int64)
                            X, Y = Y, (Y1 if Y is Y0 else Y0)

                    for _ in range(a.warmup):
                        fused()
                        composed()
                    torch.cuda.synchronize()
                    tf, tc = [], []
                    for _ in range(a.reps):   # alternating, so that both see the same machine
                        tf.append(event_ms(torch, fused))
                        tc.append(event_ms(torch, composed))
                    record(a.out, {
                        "case": f"krylov_n{n}_nnz{a.row_nnz}_K{K}_p{p}", "n": n, "K": K, "prime": p, "steps": a.steps,
                        "fused_us_per_step": round(float(np.median(tf)) * 1e3 / a.steps, 2),
                        "composed_us_per_step": round(float(np.median(tc)) * 1e3 / a.steps, 2),
                        "fused_min_max_us": [round(min(tf) * 1e3 / a.steps, 2), round(max(tf) * 1e3 / a.steps, 2)],
                        "composed_min_max_us": [round(min(tc) * 1e3 / a.steps, 2), round(max(tc) * 1e3 / a.steps, 2)],
                        "launches": S.minpoly_stats()["launches"],
                    })
            del A
    p = a.bm_prime
    for d in [int(v) for v in a.bm_degrees.split(",") if v]:
        f = [int(x) for x in rng.integers(0, p, size=d)] + [1]
        s = lfsr(f, rng.integers(0, p, size=d), 2 * d, p)
        for where, name in ((1, "lds"), (2, "device_memory")):
            us, got = [], None
            for r in range(a.warmup + a.reps):
                got = S.berlekamp_massey(s, p, where=where)
                if r >= a.warmup:
                    us.append(S.minpoly_stats()["bm_device_us"])
            assert [int(x) % p for x in got] == f, "Berlekamp-Massey did not return the polynomial of the sequence"
            record(a.out, {"case": f"bm_d{d}_{name}_p{p}", "degree": d, "terms": 2 * d, "prime": p, "class": name,
                           "device_us": float(np.median(us)), "min_max_us": [min(us), max(us)]})


if __name__ == "__main__":
    main()
