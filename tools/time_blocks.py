"""Times the block split on the device (csrc/blocks.hpp) against the host split, up to the ranks of the blocks: (i) the block matrix
of tools/time_batch.py (5000 connected components of 2..40 rows and columns, 105 753 x 106 399, p = 42013), (ii) one single-component
matrix: BASELINE config 3 at 1/--scale (synth_csr kind 1, 20 entries per row, p = 65521), where every union contends for one root.
Per case, median of --reps after --warmup calls:
  host_ms     Block.from_csr(A) + blocks.rank(B, batched=True)   (host_split_ms + host_rank_ms)
  device_ms   DeviceBlocks(A).rank(), the handle built inside the timed call (device_split_ms: the constructor alone)
  components_us / numbering_us / split_us: device time of the three phases (info(), HIP events), of the last call
Both sides must agree on the rank and on the number of blocks.  One JSON line per case.  --skip-rank leaves the ranks out (the
single-component case spends seconds in the general path on either side)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spasm_jl_amd as S  # noqa: E402
from time_batch import block_matrix  # noqa: E402


def timed(fn, reps, warmup):
    ms, out = [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def run_case(name, A, reps, warmup, with_rank):
    info = {}

    def host():
        t0 = time.perf_counter()
        B = S.Block.from_csr(A)
        info["host_split_ms"] = (time.perf_counter() - t0) * 1e3
        return len(B), (S.blocks.rank(B, batched=True) if with_rank else None)

    def device():
        t0 = time.perf_counter()
        with S.DeviceBlocks(A) as D:
            info["device_split_ms"] = (time.perf_counter() - t0) * 1e3
            info.update(D.info())
            return len(D), (sum(D.rank()) if with_rank else None)

    host_ms, (hb, hr) = timed(host, reps, warmup)
    device_ms, (db, dr) = timed(device, reps, warmup)
    assert (hb, hr) == (db, dr), f"host and device disagree: {(hb, hr)} != {(db, dr)}"
    out = {"case": name, "shape": list(A.shape), "prime": A.prime, "rank": dr, "host_ms": round(host_ms, 3), "device_ms": round(device_ms, 3),
           "ratio_host_over_device": round(host_ms / max(device_ms, 1e-9), 1)}
    out.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()})
    if with_rank:
        out.update({"batch_" + k: v for k, v in S.batch_stats().items()})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--components", type=int, default=5000, help="0: skip the block case")
    ap.add_argument("--scale", type=int, default=10, help="config 3 at 1/scale; 0: skip the single-component case")
    ap.add_argument("--skip-rank", action="store_true")
    a = ap.parse_args()
    if a.components > 0:
        run_case(f"block_{a.components}_components", block_matrix(a.components, 0xB10C, 42013), a.reps, a.warmup, not a.skip_rank)
    if a.scale > 0:
        n = 1000000 // a.scale
        run_case(f"config3_1/{a.scale}_one_component", S.synth_csr(1, n, n, row_nnz=20, prime=65521, seed=0x5A5A0003), a.reps, a.warmup, not a.skip_rank)


if __name__ == "__main__":
    main()
