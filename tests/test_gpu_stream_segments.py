"""The streaming scatter cuts a row's stream BY POSITION ("Segment records"): the plan kernel writes one
record per run of W (a segment) and one for the row's own entries, and chunk g of a wave is the 64 stream positions
64 g .. 64 g + 63 whatever segments they fall into.  These matrices are built by hand so that the streams hit the edges of that
cut; every case goes through spasm_amd_schur_plan_* and is compared with the oracle entry for entry, plus the five counters.

How the matrices are made.  Row 0 is the single entry (0, 1): the pivot of column 0, and its row of W is empty.  Row j
(1 <= j < P) is (j, a_j) followed by lens[j - 1] entries on non-pivot columns: the pivot of column j, whose row of W has exactly
that many entries (no pivot row holds another pivot column, so W = -U_PN up to the pivots' inverses).  Every other row holds an
entry on column 0 -- it loses the election of its leftmost column to row 0 and is reduced --, entries on the pivot columns it
picks (one run of W each, in the order of the row's entries) and `nN` entries on non-pivot columns (its own segment).  The length
of its stream is nN + the sum of the picked lengths.  A row cannot be reduced without an entry on a pivot column (it would win
its leftmost column), so "no run at all" is a row whose only pivot column is column 0, whose run is empty.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("npiv", "applications", "nnz_reduced", "nnz_out", "rows_out")
OWN_WIDTH = 1 << 14  # non-pivot columns no pivot row touches


def run_plan(S, A, lo=0, hi=None):
    lib = S._abi.lib()
    hi = A.n if hi is None else hi
    plan = lib.spasm_amd_schur_plan_create_strided(A.data, lo, hi, 1)
    assert plan, S._abi.last_error()
    try:
        assert lib.spasm_amd_schur_plan_run(plan, None) == 0, S._abi.last_error()
        st = S._abi.RoundStats()
        assert lib.spasm_amd_schur_plan_stats(plan, C.byref(st)) == 0, S._abi.last_error()
        ptr = lib.spasm_amd_schur_plan_fetch(plan, None)
        assert ptr, S._abi.last_error()
        return S.CSR(ptr), st.as_dict()
    finally:
        lib.spasm_amd_schur_plan_free(plan)


class Builder:
    """lens[j - 1] = entries of the row of W of pivot column j.  share = {j: (i, k)}: the first k non-pivot columns of pivot row j
    are k columns of pivot row i spread over its whole length (two runs that meet on those columns)."""

    def __init__(self, prime, lens, share=None, seed=1):
        self.p = prime
        self.rng = np.random.default_rng(seed)
        self.lens = list(lens)
        self.P = 1 + len(self.lens)
        self.cols = {}
        nxt = self.P
        for j, L in enumerate(self.lens, start=1):
            mine = []
            if share and j in share:
                i, k = share[j]
                mine = [self.cols[i][(t * len(self.cols[i])) // k] for t in range(k)]
            fresh = L - len(mine)
            mine += list(range(nxt, nxt + fresh))
            nxt += fresh
            self.cols[j] = mine
        self.own0 = nxt
        self.m = nxt + OWN_WIDTH
        self.rows = [[(0, 1)]] + [[(j, self.val())] + [(c, self.val()) for c in self.cols[j]] for j in range(1, self.P)]
        self.stream = []  # stream length of every reduced row

    def val(self):
        return int(self.rng.integers(1, self.p))

    def row(self, picks, nN, own_from=None, times=1):
        """`times` rows with an entry on column 0, on every pivot column of `picks` and on nN non-pivot columns; own_from = (j, k):
        k of the nN columns are columns of pivot row j (the own segment and that run meet there)."""
        for _ in range(times):
            own = []
            if own_from:
                j, k = own_from
                own = [int(c) for c in self.rng.choice(self.cols[j], size=k, replace=False)]
            own += [self.own0 + int(c) for c in self.rng.choice(OWN_WIDTH, size=nN - len(own), replace=False)]
            body = [(j, self.val()) for j in picks] + [(c, self.val()) for c in own]
            body = [body[i] for i in self.rng.permutation(len(body))]  # own entries and runs interleaved, runs in any order
            at = int(self.rng.integers(0, len(body) + 1))
            self.rows.append(body[:at] + [(0, self.val())] + body[at:])
            self.stream.append(nN + sum(self.lens[j - 1] for j in picks))

    def finish(self, S, O):
        A = S.CSR.from_rows(self.rows, self.m, self.p)
        So, info = O.schur_round(A)
        assert info["npiv"] == self.P, (info["npiv"], self.P)  # the pivots are where the construction wants them
        return A, So, info, self.stream


def edges(S, O, prime):
    """lengths 1, 2, 3, 63, 64, 65, 128, 200, then thirty runs of 1 - 3 entries and ten of 17"""
    lens = [1, 2, 3, 63, 64, 65, 128, 200] + [1 + (i % 3) for i in range(30)] + [17] * 10
    R1, R63, R64, R65, R128, R200 = 1, 4, 5, 6, 7, 8
    short = list(range(9, 39))
    mid = list(range(39, 49))
    b = Builder(prime, lens, seed=prime % 1000)
    T = 6
    b.row([R64], 0, times=T)             # a stream of exactly 64: one full chunk, no own segment
    b.row([R128], 0, times=T)            # exactly 128
    b.row([R63], 0, times=T)             # 63
    b.row([R65], 0, times=T)             # 65: one entry in the second chunk
    b.row([R1], 0, times=T)              # 1, as a run
    b.row([], 1, times=T)                # 1, as the own segment: no run at all (column 0's is empty)
    b.row([], 100, times=T)              # own segment only, two chunks
    b.row([R64], 64, times=T)            # the run starts at lane 0 of the second chunk
    b.row([R64], 63, times=T)            # the run starts at lane 63 of the first chunk
    b.row([R1], 63, times=T)             # ... and is the last entry of the stream
    b.row(short[:25], 5, times=T)        # 26 segments in one chunk
    b.row(short, 0, times=T)             # 30 runs of 1 - 3 entries, no own segment
    b.row([R200], 10, times=T)           # one run over four chunks
    b.row([R200, R128, 3], 61, times=T)  # 392 entries: long runs, a short one and the own segment in any order
    b.row(mid, 7, times=T)               # ten runs of 17: the shape of the bench's rows
    b.row(mid + short + [R63, R65], 20, times=T)
    for _ in range(120):                 # and a crowd of whatever
        k = int(b.rng.integers(0, 12))
        picks = [int(j) for j in b.rng.choice(np.arange(1, b.P), size=k, replace=False)]
        b.row(picks, int(b.rng.integers(0, 40)))
    return b.finish(S, O)


def duplicates(S, O, prime):
    """runs that meet on columns: in one chunk, in different chunks of different waves, more often than a row's fix-up list holds"""
    #       1   2   3    4    5    6    7    8   9
    lens = [20, 20, 300, 330, 300, 200, 200, 40, 40]
    share = {2: (1, 10), 5: (3, 17), 7: (6, 100), 9: (8, 30)}
    b = Builder(prime, lens, share=share, seed=7 + prime % 1000)
    T = 10
    b.row([1, 2], 4, times=T)                     # the duplicate and its owner in the same chunk
    b.row([1, 2], 0, times=T)
    b.row([1], 30, own_from=(1, 8), times=T)      # the own segment and a run meet
    b.row([8, 9], 0, times=T)                     # 30 duplicates in a stream of 80
    b.row([3, 4, 5], 20, times=T)                 # 950 entries: two waves share the row; owner and duplicate 630 positions apart
    b.row([5, 3], 700, own_from=(3, 40), times=T) # 1300: four waves
    b.row([6, 7], 0, times=T)                     # 100 duplicates: more than the fix-up list holds, the hash-table twin takes the row
    b.row([6, 7, 1, 2], 50, own_from=(6, 20), times=T)
    for _ in range(100):
        k = int(b.rng.integers(1, 10))
        picks = [int(j) for j in b.rng.choice(np.arange(1, b.P), size=k, replace=False)]
        b.row(picks, int(b.rng.integers(0, 30)))
    return b.finish(S, O)


def boundary(S, O, prime):
    """62 - 66 entries on pivot columns (column 0 among them): 63 is the last row that streams (with its own segment: 64 records),
    64 the first that goes to the multiplier lists"""
    b = Builder(prime, [5] * 70, seed=11)
    for npick in (61, 62, 63, 64, 65, 70):
        for nN in (0, 3):
            b.row(list(range(1, npick + 1)), nN, times=8)
    return b.finish(S, O)


def long_rows(S, O, prime):
    """streams beyond one wave's rows: 2 and 4 waves per row deal the position chunks among them"""
    b = Builder(prime, [170] * 40 + [1, 2, 3, 64], seed=13)
    for npick, nN in ((4, 1), (4, 0), (5, 33), (7, 90), (9, 0), (15, 10), (20, 64), (30, 19), (40, 200)):
        for _ in range(6):
            picks = [int(j) for j in b.rng.choice(np.arange(1, 41), size=npick, replace=False)]
            b.row(picks + [41, 42, 43, 44][: npick % 5], nN)
    b.row([1, 2, 3, 44], 0, times=3)  # 574 = 8 * 64 + 62
    b.row([1, 2, 3, 44, 43], 127, times=3)  # 704 = 11 * 64: the last chunk is full
    return b.finish(S, O)


CASES = {
    "edges-65521": (edges, 65521),
    "edges-127": (edges, 127),
    "edges-2147483647": (edges, 2147483647),
    "duplicates-65521": (duplicates, 65521),
    "duplicates-7": (duplicates, 7),  # a duplicate cancels its owner once in seven
    "duplicates-2147483647": (duplicates, 2147483647),
    "boundary-65521": (boundary, 65521),
    "long-65521": (long_rows, 65521),
    "long-2147483647": (long_rows, 2147483647),
}


@functools.lru_cache(maxsize=None)
def case(S, O, name):
    make, prime = CASES[name]
    return make(S, O, prime)


def check(S, A, So, info, lo=0, hi=None):
    Sc, st = run_plan(S, A, lo, hi)
    for key in COUNTERS:
        assert st[key] == info[key], (key, st[key], info[key])
    assert Sc.n == So.n
    got, want = Sc.rows(), So.rows()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:8], w[:8])
    return st


@pytest.mark.parametrize("name", list(CASES))
def test_segment_streams_vs_oracle(S, O, name):
    A, So, info, stream = case(S, O, name)
    check(S, A, So, info)


def test_the_edges_are_where_they_should_be(S, O):
    """the streams the constructions promise (a change of the builder must not move them off the edges silently)"""
    _, _, _, stream = case(S, O, "edges-65521")
    for want in (1, 63, 64, 65, 127, 128, 210):
        assert want in stream, want
    _, _, _, stream = case(S, O, "long-65521")
    assert any(640 < s <= 1280 for s in stream) and any(1280 < s <= 2560 for s in stream) and any(5120 < s <= 10240 for s in stream)
    assert 574 in stream and 704 in stream


def test_a_shard_smaller_than_a_workgroup(S, O):
    """three rows of the edge matrix as a shard: every wave past the third clamps its descriptors to the last row"""
    A, _, _, _ = case(S, O, "edges-65521")
    make, prime = CASES["edges-65521"]
    P = 49
    for lo, hi in ((P + 6 * 7, P + 6 * 7 + 3), (P + 6 * 12, P + 6 * 12 + 1), (A.n - 2, A.n)):
        So, info = O.schur_round(A, row_lo=lo, row_hi=hi)
        check(S, A, So, info, lo, hi)
