"""Times the characteristic polynomial by components (csrc/blocks.hpp index split, csrc/charpoly.hpp, csrc/polyprod.hpp) against a
yardstick measured in the same run: charpoly_batch of the FETCHED blocks plus the product of the factors in Python on the host.

Cases (each at every prime of --primes): N random dense n x n blocks on the diagonal, scrambled by a random simultaneous
permutation on the device (4096 of 32 x 32 and 256 of 181 x 181), and the diagonal matrix with n = 200 000 (all blocks 1 x 1:
the product tree alone).  Per case: wall ms of S.charpoly(A, split=True) from the host matrix (upload, split, kernels, product),
of DeviceBlocks.charpoly() on a handle that exists already, and of the yardstick (median of --reps after --warmup calls, host
clock); the device microseconds of charpoly_split_stats (HIP events inside the library) and of the split (blocks_info).  The
yardstick's product is a pairwise tree of numpy int64 convolutions reduced mod p at every level: directly for p < 2^16 (at most
2^18 terms below 2^32), and on the 16-bit halves of the coefficients otherwise (four convolutions of terms below 2^32, put together
in Python integers).  For p >= 2^16 it is left out (null) above --host-product-max, and the blocks are fetched for charpoly_batch
only up to --fetch-max of them (null above: one call per block).  The results must agree.  One JSON line per case, printed and
appended to --out (profiles/charpoly_split_timing.jsonl)."""
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


def block_diagonal(rng, N, n, p):
    """N dense n x n blocks on the diagonal, scrambled by a simultaneous permutation on the device; the host matrix"""
    nn = N * n
    V = S.balanced(rng.integers(1, p, size=(nn, n), dtype=np.int64), p)
    cols = (np.arange(nn, dtype=np.int64) // n * n)[:, None] + np.arange(n, dtype=np.int64)[None, :]
    A = S.CSR.from_arrays(nn, nn, np.arange(nn + 1, dtype=np.int64) * n, cols.ravel().astype(np.int32), V.ravel(), prime=p)
    if n == 1:
        return A
    q = rng.permutation(nn).astype(np.int32)
    with S.DeviceCSR(A) as D0, D0.permute(q, q) as D:
        return D.download()


def host_product(polys, p):
    level = [np.asarray(f, dtype=np.int64) % p for f in polys]
    while len(level) > 1:
        nxt = []
        for k in range(0, len(level), 2):
            if k + 1 == len(level):
                nxt.append(level[k])
            elif p < 65536:
                nxt.append(np.convolve(level[k], level[k + 1]) % p)
            else:
                u, v = level[k], level[k + 1]
                u1, u0, v1, v0 = u >> 16, u & 0xFFFF, v >> 16, v & 0xFFFF
                hi, mid, lo = np.convolve(u1, v1) % p, (np.convolve(u1, v0) + np.convolve(u0, v1)) % p, np.convolve(u0, v0) % p
                out = (hi.astype(object) * (1 << 32) + mid.astype(object) * (1 << 16) + lo.astype(object)) % p
                nxt.append(out.astype(np.int64))
        level = nxt
    return S.balanced(np.array([int(v) for v in level[0]], dtype=np.int64), p).astype(np.int32)


def record(out_path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="4096x32,256x181,200000x1", help="N blocks x n rows, comma separated")
    ap.add_argument("--primes", default="65521,4294967291")
    ap.add_argument("--host-product-max", type=int, default=50000, help="largest N * n whose host product is timed when p >= 2^16")
    ap.add_argument("--fetch-max", type=int, default=10000, help="most blocks that are fetched for the charpoly_batch yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charpoly_split_timing.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0xC4A3)
    for p in [int(v) for v in a.primes.split(",") if v]:
        for case in [c for c in a.cases.split(",") if c]:
            N, n = (int(v) for v in case.split("x"))
            A = block_diagonal(rng, N, n, p)
            split_ms, chi = timed(lambda: S.charpoly(A, split=True), a.reps, a.warmup)
            with S.DeviceBlocks(A, index=True) as B:
                info = B.info()
                handle_ms, chi2 = timed(B.charpoly, a.reps, a.warmup)
                st = S.charpoly_split_stats()
                factors, batch_ms, blocks = B.charpoly_factors(), None, None
                if len(B) <= a.fetch_max:
                    blocks = [B.fetch(b) for b in range(len(B))]
                    batch_ms, fetched = timed(lambda: S.charpoly_batch(blocks), a.reps, a.warmup)
                    assert [f.tolist() for f in fetched] == [f.tolist() for f in factors], "factors disagree"
            assert chi.tobytes() == chi2.tobytes()
            host_ms = None
            if p < 65536 or N * n <= a.host_product_max:
                host_ms, ref = timed(lambda: host_product(factors, p), 1, 0)
                assert ref.tobytes() == chi.tobytes(), "the host product disagrees"
            record(a.out, {
                "case": f"{N}x{n}x{n}_p{p}", "blocks": N, "n": N * n, "prime": p, "split_from_host_ms": round(split_ms, 3),
                "handle_charpoly_ms": round(handle_ms, 3), "yardstick_charpoly_batch_ms": None if batch_ms is None else round(batch_ms, 3),
                "yardstick_host_product_ms": None if host_ms is None else round(host_ms, 3),
                "split_device_us": info["components_us"] + info["numbering_us"] + info["split_us"], "stats": st,
            })
            del A, blocks


if __name__ == "__main__":
    main()
