"""Times the fused Horner step (csrc/horner.hpp: S.poly_apply on torch tensors, the _dev entry) against the loop a caller could write
without it, on the same SpMV handle and the same tensors, in the same run: per step Y <- c * B by torch ((B * c) % p in int64,
stored as int32) and one SpMV.apply (spasm_amd_spmv_apply_dev: Y <- A X + Y).  For a 32-bit prime the torch product of two residues
can pass 2^63, so there the composed loop is a stand-in: it costs what computing the step that way would.  Both are enqueued on the
current stream and timed with device events around a polynomial of degree `steps` (the fused run has one elementwise launch for
the leading coefficients on top of its `steps` products; the composed loop has the same first scale), after `warmup` untimed
rounds, the two variants alternating; the median of `reps` rounds is divided by the steps.  Matrices: n rows with `row_nnz` random
entries each (S.synth_csr), the shapes of tools/time_krylov.py.

Also times S.wiedemann_solve end to end on one of these matrices (--solve-n, --solve-k), split by the two timers of
S.wiedemann_stats (HIP events inside the library), with the wall time of the call beside them; median of `reps` after `warmup`.

One JSON line per case, printed and appended to --out (profiles/wiedemann_timing.jsonl)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--row-nnz", type=int, default=20)
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solve-n", type=int, default=10000)
    ap.add_argument("--solve-k", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiedemann_timing.jsonl"))
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    rng = np.random.default_rng(0x57EE)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            A = S.synth_csr(1, n, n, row_nnz=a.row_nnz, prime=p, seed=0x5A5A0000 + n)
            with S.SpMV(A) as op:
                for K in [int(v) for v in a.ks.split(",") if v]:
                    B = torch.from_numpy(S.balanced(rng.integers(0, p, size=(n, K), dtype=np.int64), p)).cuda()
                    polys = [S.balanced(rng.integers(1, p, size=a.steps + 1, dtype=np.int64), p) for _ in range(K)]
                    # the composed loop reads its coefficients from the device too: row s holds the coefficients of degree steps - s
                    T = torch.from_numpy(np.stack([f[::-1] for f in polys], axis=1).astype(np.int64)).cuda()
                    B64 = B.to(torch.int64)
                    Y0, Y1 = torch.zeros_like(B), torch.zeros_like(B)

                    def fused():
                        return S.poly_apply(op, polys, B)

                    def composed():
                        Y0.copy_((B64 * T[0]) % p)
                        X, Y = Y0, Y1
                        for i in range(1, a.steps + 1):
                            Y.copy_((B64 * T[i]) % p)
                            op.apply(X, Y)
                            X, Y = Y, X
                        return X

                    for _ in range(a.warmup):
                        fused()
                        composed()
                    torch.cuda.synchronize()
                    tf, tc = [], []
                    for _ in range(a.reps):   # alternating, so that both see the same machine
                        tf.append(event_ms(torch, fused))
                        tc.append(event_ms(torch, composed))
                    st = S.wiedemann_stats()
                    same = bool((fused() == composed()).all().item()) if p < 2**31 else None   # (exact only below 2^31)
                    record(a.out, {
                        "case": f"horner_n{n}_nnz{a.row_nnz}_K{K}_p{p}", "n": n, "K": K, "prime": p, "steps": a.steps,
                        "fused_us_per_step": round(float(np.median(tf)) * 1e3 / a.steps, 2),
                        "composed_us_per_step": round(float(np.median(tc)) * 1e3 / a.steps, 2),
                        "fused_min_max_us": [round(min(tf) * 1e3 / a.steps, 2), round(max(tf) * 1e3 / a.steps, 2)],
                        "composed_min_max_us": [round(min(tc) * 1e3 / a.steps, 2), round(max(tc) * 1e3 / a.steps, 2)],
                        "launches": st["launches"], "composed_agrees": same,
                    })
            if n == a.solve_n:
                K = a.solve_k
                Bh = S.balanced(rng.integers(0, p, size=(n, K), dtype=np.int64), p)
                with S.SpMV(A) as op:
                    seq, hor, wall, st, status = [], [], [], None, None
                    for r in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        _, status = op.wiedemann_solve(Bh)
                        t1 = time.perf_counter()
                        st = S.wiedemann_stats()
                        if r >= a.warmup:
                            seq.append(st["sequence_device_us"])
                            hor.append(st["horner_device_us"])
                            wall.append((t1 - t0) * 1e6)
                record(a.out, {
                    "case": f"wiedemann_solve_n{n}_nnz{a.row_nnz}_K{K}_p{p}", "n": n, "K": K, "prime": p, "status": status.tolist(),
                    "tries": st["tries"], "products": st["products"], "launches": st["launches"], "degree": st["degree"],
                    "sequence_bm_device_us": float(np.median(seq)), "horner_check_device_us": float(np.median(hor)),
                    "wall_us": round(float(np.median(wall)), 1),
                    "sequence_bm_min_max_us": [min(seq), max(seq)], "horner_check_min_max_us": [min(hor), max(hor)],
                })
            del A


if __name__ == "__main__":
    main()
