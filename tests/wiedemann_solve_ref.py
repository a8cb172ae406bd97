"""Host references shared by tests/test_gpu_poly_apply.py and tests/test_gpu_wiedemann_solve.py: Horner's rule through Mat.apply and
Wiedemann's solve with its certificate, seed-per-try rule and statuses, in numpy int64 and Python integers on top of
tests/wiedemann_ref.py.  The algorithm is the one include/spasm_amd.h describes for spasm_amd_wiedemann_solve; every quantity it
produces is determined by (A, b, u), so the device must give the same bytes.  Nothing here touches a device."""
import numpy as np

import wiedemann_ref as W
from wiedemann_ref import bal, mulmod

M64 = (1 << 64) - 1


def seeded_U(n, K, seed, p):
    """the U of spasm_amd_minpoly_vectors(n, K, seed): word (r, c) is splitmix64(seed + 0x9E3779B97F4A7C15 * (2 (r K + c) + 1)) mod p"""
    out = np.zeros(n * K, dtype=np.int64)
    for e in range(n * K):
        z = (seed + 0x9E3779B97F4A7C15 * (2 * e + 1)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out[e] = (z ^ (z >> 31)) % p
    return bal(out.reshape(n, K), p)


def ref_poly_apply(A, polys, V, p):
    """X[:, c] = f_c(A) V[:, c] by Horner on the common schedule of max(deg) products (a column of lower degree is zero until its
    leading coefficient arrives); polys[c] any integers, low degree first, [] the zero polynomial; balanced int32 (n, K)"""
    Vr = np.asarray(V, dtype=np.int64).reshape(A.n, -1) % p
    K = Vr.shape[1]
    assert len(polys) == K
    D = max(len(f) for f in polys) - 1
    X = np.zeros((A.n, K), dtype=np.int64)
    for s in range(D + 1):
        j = D - s
        c = np.array([int(f[j]) % p if j < len(f) else 0 for f in polys], dtype=np.int64)
        X = (A.apply(X, p) + mulmod(Vr, c[None, :], p)) % p
    return bal(X, p)


def ref_solve(M, B, p, trans=False, seed=0, tries=3, maxdeg=None, U=None):
    """(X, status, stats): the columns of B solved one by one as the device does; stats has tries, products, degree, solved,
    kernel_vectors.  Raises ValueError("degree bound too small") where the device refuses."""
    A = M.transpose() if trans else M
    n = A.n
    B = np.asarray(B, dtype=np.int64).reshape(n, -1)
    K = B.shape[1]
    md = n if maxdeg is None or maxdeg <= 0 or maxdeg > n else maxdeg
    length = 2 * md + 2 if md < n else 2 * n
    ntries = 1 if U is not None else (3 if tries <= 0 else tries)
    X = np.zeros((n, K), dtype=np.int32)
    status = np.zeros(K, dtype=np.int32)
    stats = dict(tries=0, products=0, degree=0, solved=0, kernel_vectors=0)
    act = list(range(K))
    for t in range(ntries):
        if not act:
            break
        Ut = (np.asarray(U).reshape(n, K) if U is not None else seeded_U(n, K, seed + t, p))[:, act]
        Bt = B[:, act]
        seq = W.ref_sequence(A, Ut, Bt, length, p)
        table, regular, Lmax = [], [], 0
        for a in range(len(act)):
            f, L = W.ref_bm(seq[:, a], p)
            if L > md:
                raise ValueError("degree bound too small")
            Lmax = max(Lmax, L)
            scale = (-pow(f[0], -1, p)) % p if f[0] else 1
            table.append([x * scale % p for x in f[1:]])
            regular.append(f[0] != 0)
        Xt = ref_poly_apply(A, table, Bt, p) if Lmax > 0 else np.zeros((n, len(act)), dtype=np.int32)
        r = np.array([p - 1 if g else 0 for g in regular], dtype=np.int64)
        R = (A.apply(Xt.astype(np.int64) % p, p) + mulmod(Bt % p, r[None, :], p)) % p
        stats["tries"] = t + 1
        stats["products"] += (length - 1) + max(Lmax - 1, 0) + 1
        stats["degree"] = max(stats["degree"], Lmax)
        left = []
        for a, c in enumerate(act):
            rzero, xzero = not R[:, a].any(), not Xt[:, a].any()
            if regular[a] and rzero:
                status[c] = 1
                stats["solved"] += 1
            elif not regular[a] and rzero and not xzero:
                status[c] = 2
                stats["kernel_vectors"] += 1
            else:
                left.append(c)
                continue
            X[:, c] = Xt[:, a]
        act = left
    return X, status, stats
