"""The row classes of the exact products with A (csrc/spmv.hpp; spmv_launch, SpmvView::bin and apply_dev in engine.hip) on inputs
built so that one named piece of a kernel must be right: blocks of every chunk width over rows on both sides of every bin edge,
a lane that takes a whole segment of worst-case terms, rows binned longer than they are on the device, windows of wider arrays.

The inputs and the exact integer references come from sparse_worst_cases.py; test_sparse_worst_cases_host.py proves the
constructions (row lengths, designed products, segment sums) without a GPU.  Every comparison is exact equality."""
import functools

import numpy as np
import pytest

import sparse_worst_cases as W

pytestmark = pytest.mark.gpu

PRIMES = [3, 65521, 65537, 0xFFFFFFFB]  # 65521: the last prime with F.small, 65537: the first without
KMAX = max(W.SPMV_BLOCKS)


def to_csr(S, M, p):
    return S.CSR.from_arrays(M.n, M.m, M.ptr, M.j.astype(np.int32), M.v.astype(np.int32), prime=p)


@functools.lru_cache(maxsize=None)
def designed(p):
    """the 13 x 32769 matrix of the row lengths 0, 1, 31, 32, 33, 63, 64, 65, 16383, 16384, 16385, 32768, 32769 and its transpose"""
    A = W.spmv_designed(p, np.random.default_rng(p % 1000 + 11))
    return A, W.host_transpose(A)


def window(master, k, pad_left, extra, rng):
    """the first k columns of master as a window of an array k + extra wide"""
    big = W.rand_int32(rng, (master.shape[0], k + extra))
    win = big[:, pad_left:pad_left + k]
    win[:] = master[:, :k]
    return big, win


def check_blocks(S, p, M, runs, trans_math, rng):
    """op(M) X + Y for M a Mat and op = transpose when trans_math, through every (host matrix, trans flag) of runs -- the same
    product by different kernels' rows: one reference for all of them, one one-shot product per column and run"""
    rin, rout = (M.n, M.m) if trans_math else (M.m, M.n)
    Xm, Y0 = W.rand_int32(rng, (rin, KMAX)), W.rand_int32(rng, (rout, KMAX))
    want = W.ref_apply(M.ptr, M.j, M.v, Xm, Y0, trans_math, p)
    for H, trans in runs:
        single = np.empty_like(want)
        for c in range(KMAX):
            x, y = np.ascontiguousarray(Xm[:, c]), Y0[:, c].copy()
            single[:, c] = S.xapy(x, H, y) if trans else S.axpy(H, x, y)
        assert np.array_equal(single, want), (p, trans)
        with S.SpMV(H) as op:
            for k in W.SPMV_BLOCKS:
                Xbig, X = window(Xm, k, 1, 3, rng)    # ldx = k + 3
                Ybig, Y = window(Y0, k, 2, 5, rng)    # ldy = k + 5
                Xbig0, Ybig0 = Xbig.copy(), Ybig.copy()
                assert op.apply(X, Y, trans=trans) is Y
                bad = np.argwhere(Y != want[:, :k])
                assert len(bad) == 0, (p, k, trans, H.shape, bad[:5].tolist())
                assert np.array_equal(Y, single[:, :k])  # column c of the block is the one-shot product on column c
                assert np.array_equal(Xbig, Xbig0)
                assert np.array_equal(Ybig[:, :2], Ybig0[:, :2]) and np.array_equal(Ybig[:, k + 2:], Ybig0[:, k + 2:])


@pytest.mark.parametrize("p", PRIMES)
def test_block_products_over_every_bin(S, p):
    """k = 1 .. 129 covers every kernel width full, partly filled and as a second chunk of one column (spmv_chunks); the designed
    matrix has rows in the short, the medium and the long list, none of them a range, so the short kernel runs with a row list, the
    medium and the long kernel and k_spmv_combine with every KW.  The transpose of the designed matrix brings the same lengths to
    the rows of the device transpose (trans=True)."""
    rng = np.random.default_rng(p % 1000 + 12)
    A, T = designed(p)
    a, t = to_csr(S, A, p), to_csr(S, T, p)
    check_blocks(S, p, A, [(a, False), (t, True)], False, rng)   # A X: rows of A, rows of the device transpose of T
    check_blocks(S, p, A, [(a, True), (t, False)], True, rng)    # A^T X: short rows only, both ways
    B = W.spmv_short_plus_one(p, rng)                            # short_all false with lists of a few rows
    b = to_csr(S, B, p)
    check_blocks(S, p, B, [(b, False)], False, rng)
    check_blocks(S, p, B, [(b, True)], True, rng)


@pytest.mark.parametrize("p", [65521, 32749, 65537, 0xFFFFFFFB])
def test_lane_takes_a_whole_segment_of_worst_case_terms(S, p):
    """A medium row of 16384 entries and long rows of 49153 and 81921 (three and five full segments and one of a single entry),
    every product congruent to t = target_residue(p) (and, in the twin, to -t), applied with k = 64: KW = 64, so E = 1 and one lane
    sums a whole row or segment.  Magnitudes reached by a lane's accumulator: 16384 * (p//2 - 512) = 2^28.98 for p = 65521 (i32, the
    header of spmv.hpp claims < 2^29.01) and 2^27.95 for 32749; 16384 * (p//2 - 1) = 2^29 for 65537 and 2^45 for 0xFFFFFFFB (i64).
    The row of 81921 terms sums to 2^31.3 for 65521: were it not cut into segments, a lane's i32
    would wrap.  The partials of a long row that k_spmv_combine adds are each t.  Y starts at INT32_MAX and INT32_MIN in alternate
    columns; a tenth of X is unreduced.  k = 1, 8, 65 run the same rows with E = 64, 8 and the second chunk."""
    for sign in (1, -1):
        rng = np.random.default_rng(p % 1000 + 13 + sign)
        M, x, sums = W.lane_worst_case(p, rng, sign)
        xl = W.lift(x, p, rng, 0.1).astype(np.int32)
        for H, trans in ((to_csr(S, M, p), False), (to_csr(S, W.host_transpose(M), p), True)):
            with S.SpMV(H) as op:
                for k in (64, 1, 8, 65):
                    X = np.ascontiguousarray(np.repeat(xl[:, None], k, axis=1))
                    y0 = [W.INT32_MAX if c % 2 == 0 else W.INT32_MIN for c in range(k)]
                    Y = np.array([y0] * M.n, dtype=np.int32)
                    want = [[W.bal(s + y, p) for y in y0] for s in sums]  # Python integers
                    op.apply(X, Y, trans=trans)
                    assert Y.tolist() == want, (p, sign, trans, k)


@pytest.mark.parametrize("p", PRIMES)
def test_rows_binned_longer_than_they_are(S, p):
    """Rows of 33, 16385 and 32769 stored entries of which 5 are not multiples of p: binned by the stored length (medium, long,
    long), 5 entries long on the device, so the second and third segment of a long row start past its end (lo >= hi) and their
    partials must be written as 0.  The stored values are unreduced (v + s p): the reduction at ingest."""
    rng = np.random.default_rng(p % 1000 + 14)
    M = W.binned_longer(p, rng)
    with S.SpMV(to_csr(S, M, p)) as op:
        for k in (1, 64):
            for trans in (False, True):
                rin, rout = (M.n, M.m) if trans else (M.m, M.n)
                X, Y = W.rand_int32(rng, (rin, k)), W.rand_int32(rng, (rout, k))
                want = W.ref_apply(M.ptr, M.j, M.v, X, Y, trans, p)
                op.apply(X, Y, trans=trans)
                assert np.array_equal(Y, want), (p, k, trans)


@pytest.mark.parametrize("p", PRIMES)
def test_torch_windows(S, p):
    """spasm_amd_spmv_apply_dev with X and Y as column windows of wider device tensors (stride(0) = k + 3 and k + 5 > k), on the
    designed matrix and its transpose: the result is the numpy path's, the words outside the windows keep their values"""
    import torch

    rng = np.random.default_rng(p % 1000 + 15)
    for M in designed(p):
        with S.SpMV(to_csr(S, M, p)) as op:
            for k in (3, 64, 65):
                for trans in (False, True):
                    rin, rout = (M.n, M.m) if trans else (M.m, M.n)
                    Xbig, Ybig = W.rand_int32(rng, (rin, k + 3)), W.rand_int32(rng, (rout, k + 5))
                    want = op.apply(np.ascontiguousarray(Xbig[:, 1:1 + k]), np.ascontiguousarray(Ybig[:, 2:2 + k]), trans=trans)
                    Xt, Yt = torch.from_numpy(Xbig).cuda(), torch.from_numpy(Ybig).cuda()
                    Xw, Yw = Xt[:, 1:1 + k], Yt[:, 2:2 + k]
                    assert Xw.stride(0) == k + 3 and Yw.stride(0) == k + 5
                    assert op.apply(Xw, Yw, trans=trans) is Yw
                    torch.cuda.synchronize()
                    got = Yt.cpu().numpy()
                    assert np.array_equal(got[:, 2:2 + k], want), (p, k, trans, M.n)
                    assert np.array_equal(got[:, :2], Ybig[:, :2]) and np.array_equal(got[:, k + 2:], Ybig[:, k + 2:])
                    assert np.array_equal(Xt.cpu().numpy(), Xbig)
