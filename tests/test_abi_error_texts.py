"""The error texts of the C ABI, pinned: calls that fail at an argument check before any device is needed, so the return value and
the text of spasm_amd_last_error() are the same with and without a GPU.  The strings were recorded from the library as it was
before the entry points were routed through one error guard (abi_call in csrc/engine.hip) and must not change with it -- the
doubled names of the spmv family and of spasm_amd_dshard_open included: the functions below those entries put the entry's name
in front themselves, and the entry adds it again.

Every row is followed by a call that succeeds without a device, after which the text must be empty: one of the row's own family
where the family has such a call (a solver of zero systems, a batch of zero matrices, zero right-hand sides), otherwise the
solver of zero systems, which goes through the same guard.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

NULL = object()  # a NULL pointer returned (ctypes: None for void *, a false pointer object for typed pointers)
P = C.POINTER


class Ctx:
    """The arguments the rows share; built once."""

    def __init__(self, S):
        self.S = S
        self.lib = S._abi.lib()
        self.csrp = P(S._abi.CsrStruct)
        self.A = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)  # 3 x 2
        self.U = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, 1)]], 2, prime=127)
        self.x = np.zeros(4, dtype=np.int32)
        self.b = np.zeros(4, dtype=np.int32)
        self.xj = np.zeros(12, dtype=np.int32)
        self.q = np.full(2, -1, dtype=np.int32)
        self.ok = np.zeros(4, dtype=np.uint8)
        self.out1 = (self.csrp * 1)()
        self.lu1 = (P(S._abi.LuStruct) * 1)()
        self.okp1 = (P(C.c_ubyte) * 1)()
        self.rank1 = (C.c_int64 * 1)()
        self.hash = (C.c_uint8 * 32)()
        self.lu = S._abi.LuStruct()  # a factorization with U alone: no L, no qinv, no p
        self.lu.U = self.U.data
        self.h0 = self.lib.spasm_amd_solver_create(0, None)  # a solver of zero systems
        assert self.h0

    def arr(self, mats):
        return (self.csrp * max(len(mats), 1))(*[M.data if M is not None else None for M in mats])

    @staticmethod
    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def ip(a):
        return a.ctypes.data_as(P(C.c_int32))


@pytest.fixture(scope="module")
def ctx(S):
    c = Ctx(S)
    yield c
    c.lib.spasm_amd_solver_free(c.h0)


# the device-free successes
def ok_solver(c):
    h = c.lib.spasm_amd_solver_create(0, None)
    assert h
    text = c.S._abi.last_error()
    c.lib.spasm_amd_solver_free(h)
    return text


def ok_batch(c):
    assert c.lib.spasm_amd_echelonize_batch(0, None, None, None) == 0
    return c.S._abi.last_error()


def ok_solve_batch(c):
    assert c.lib.spasm_amd_solve_batch(0, None, None, None, None) == 0
    return c.S._abi.last_error()


def ok_dense(c):
    assert c.lib.spasm_amd_solver_apply_dense(c.h0, 0, None, 0, None, 0, None) == 0
    return c.S._abi.last_error()


# (id, the failing call, its return value, its text, the successful call that follows)
ROWS = [
    # resident matrices
    ("dcsr_download_null", lambda c: c.lib.spasm_amd_dcsr_download(None), NULL, "spasm_amd_dcsr_download: download: NULL matrix", ok_solver),
    ("dcsr_mul_null", lambda c: c.lib.spasm_amd_dcsr_mul(None, None), NULL, "spasm_amd_dcsr_mul: product: NULL matrix", ok_solver),
    ("dcsr_equal_null", lambda c: c.lib.spasm_amd_dcsr_equal(None, None), -1, "spasm_amd_dcsr_equal: comparison: NULL matrix", ok_solver),
    # blocks
    ("blocks_create_null", lambda c: c.lib.spasm_amd_blocks_create(None), NULL, "spasm_amd_blocks_create: NULL matrix", ok_solver),
    ("blocks_create_dcsr_null", lambda c: c.lib.spasm_amd_blocks_create_dcsr(None), NULL, "spasm_amd_blocks_create_dcsr: NULL matrix", ok_solver),
    ("blocks_shapes_null", lambda c: c.lib.spasm_amd_blocks_shapes(None, None, None, None), -1, "spasm_amd_blocks_shapes: NULL handle", ok_solver),
    ("blocks_maps_null", lambda c: c.lib.spasm_amd_blocks_maps(None, None, None, None, None, None, None, None, None), -1, "spasm_amd_blocks_maps: NULL handle", ok_solver),
    ("blocks_fetch_null", lambda c: c.lib.spasm_amd_blocks_fetch(None, 0), NULL, "spasm_amd_blocks_fetch: NULL handle", ok_solver),
    ("blocks_rank_null", lambda c: c.lib.spasm_amd_blocks_rank(None, None, c.rank1), -1, "spasm_amd_blocks_rank: NULL handle", ok_batch),
    ("blocks_solve_null", lambda c: c.lib.spasm_amd_blocks_solve(None, c.A.data, c.out1, None), -1, "spasm_amd_blocks_solve: NULL handle", ok_solve_batch),
    # the resident solver
    ("solver_create_negative_count", lambda c: c.lib.spasm_amd_solver_create(-1, c.arr([c.A])), NULL, "spasm_amd_solver_create: count < 0", ok_solver),
    ("solver_create_null_array", lambda c: c.lib.spasm_amd_solver_create(2, None), NULL, "spasm_amd_solver_create: NULL array", ok_solver),
    ("solver_create_blocks_null", lambda c: c.lib.spasm_amd_solver_create_blocks(None), NULL, "spasm_amd_solver_create_blocks: NULL handle", ok_solver),
    ("solver_apply_null", lambda c: c.lib.spasm_amd_solver_apply(None, c.arr([c.A]), c.out1, c.okp1), -1, "spasm_amd_solver_apply: NULL handle", ok_solver),
    ("solver_apply_blocks_null", lambda c: c.lib.spasm_amd_solver_apply_blocks(None, c.A.data, c.out1, None), -1, "spasm_amd_solver_apply_blocks: NULL handle", ok_solver),
    ("solver_ranks_null", lambda c: c.lib.spasm_amd_solver_ranks(None, c.rank1), -1, "spasm_amd_solver_ranks: NULL handle", ok_solver),
    ("solver_basis_null", lambda c: c.lib.spasm_amd_solver_basis(None, 0, c.ip(c.x)), -1, "spasm_amd_solver_basis: NULL handle", ok_solver),
    ("solver_basis_index", lambda c: c.lib.spasm_amd_solver_basis(c.h0, 0, None), -1, "spasm_amd_solver_basis: system index out of range", ok_solver),
    # the resident solver on dense right-hand sides
    ("solver_apply_dense_null", lambda c: c.lib.spasm_amd_solver_apply_dense(None, 1, c.vp(c.b), 1, c.vp(c.x), 1, None), -1, "spasm_amd_solver_apply_dense: NULL handle", ok_dense),
    ("solver_apply_dense_negative_K", lambda c: c.lib.spasm_amd_solver_apply_dense(c.h0, -1, c.vp(c.b), 1, c.vp(c.x), 1, c.vp(c.ok)), -1, "spasm_amd_solver_apply_dense: K < 0", ok_dense),
    ("solver_apply_dense_short_ldb", lambda c: c.lib.spasm_amd_solver_apply_dense(c.h0, 2, c.vp(c.b), 1, c.vp(c.x), 2, c.vp(c.ok)), -1, "spasm_amd_solver_apply_dense: ldb < K", ok_dense),
    ("solver_apply_dense_short_ldx", lambda c: c.lib.spasm_amd_solver_apply_dense(c.h0, 2, c.vp(c.b), 2, c.vp(c.x), 1, c.vp(c.ok)), -1, "spasm_amd_solver_apply_dense: ldx < K", ok_dense),
    ("solver_apply_dense_dev_null", lambda c: c.lib.spasm_amd_solver_apply_dense_dev(None, 1, c.vp(c.b), 1, c.vp(c.x), 1, None, None), -1, "spasm_amd_solver_apply_dense_dev: NULL handle", ok_dense),
    ("solver_apply_dense_dev_negative_K", lambda c: c.lib.spasm_amd_solver_apply_dense_dev(c.h0, -1, c.vp(c.b), 1, c.vp(c.x), 1, c.vp(c.ok), None), -1, "spasm_amd_solver_apply_dense_dev: K < 0", ok_dense),
    ("solver_apply_dense_dev_short_ldb", lambda c: c.lib.spasm_amd_solver_apply_dense_dev(c.h0, 2, c.vp(c.b), 1, c.vp(c.x), 2, c.vp(c.ok), None), -1, "spasm_amd_solver_apply_dense_dev: ldb < K", ok_dense),
    # matrix-vector products: spmv_check names the entry, and the entry names itself again
    ("spmv_apply_null", lambda c: c.lib.spasm_amd_spmv_apply(None, 0, 1, c.vp(c.x), 1, c.vp(c.b), 1), -1, "spasm_amd_spmv_apply: spasm_amd_spmv_apply: NULL operator", ok_solver),
    ("spmv_apply_dev_null", lambda c: c.lib.spasm_amd_spmv_apply_dev(None, 0, 1, c.vp(c.x), 1, c.vp(c.b), 1, None), -1, "spasm_amd_spmv_apply_dev: spasm_amd_spmv_apply_dev: NULL operator", ok_solver),
    # dense triangular solves: the name once
    ("trsolve_create_null", lambda c: c.lib.spasm_amd_trsolve_create(None, c.vp(c.q), 0), NULL, "spasm_amd_trsolve_create: NULL matrix", ok_solver),
    ("trsolve_create_kind", lambda c: c.lib.spasm_amd_trsolve_create(c.U.data, c.vp(c.q), 7), NULL, "spasm_amd_trsolve_create: kind must be 0 (forward, piv = q) or 1 (back, piv = p)", ok_solver),
    ("trsolve_apply_null", lambda c: c.lib.spasm_amd_trsolve_apply(None, 1, c.vp(c.b), 1, c.vp(c.x), 1, None), -1, "spasm_amd_trsolve_apply: NULL operator", ok_solver),
    ("trsolve_apply_dev_null", lambda c: c.lib.spasm_amd_trsolve_apply_dev(None, 1, c.vp(c.b), 1, c.vp(c.x), 1, None, None), -1, "spasm_amd_trsolve_apply_dev: NULL operator", ok_solver),
    ("dense_forward_solve_null", lambda c: c.lib.spasm_dense_forward_solve(None, c.vp(c.b), c.vp(c.x), c.vp(c.q)), False, "spasm_dense_forward_solve: NULL matrix", ok_solver),
    ("dense_back_solve_null", lambda c: c.lib.spasm_dense_back_solve(None, c.vp(c.b), c.vp(c.x), c.vp(c.q)), False, "spasm_dense_back_solve: NULL matrix", ok_solver),
    # many small matrices in one call
    ("echelonize_batch_negative_count", lambda c: c.lib.spasm_amd_echelonize_batch(-1, c.arr([c.A]), None, c.lu1), -1, "spasm_amd_echelonize_batch: count < 0", ok_batch),
    ("echelonize_batch_null_array", lambda c: c.lib.spasm_amd_echelonize_batch(1, None, None, c.lu1), -1, "spasm_amd_echelonize_batch: NULL array", ok_batch),
    ("rank_batch_null_matrix", lambda c: c.lib.spasm_amd_rank_batch(1, c.arr([None]), None, c.rank1), -1, "spasm_amd_rank_batch: matrix 0: NULL matrix", ok_batch),
    ("kernel_batch_negative_count", lambda c: c.lib.spasm_amd_kernel_batch(-3, None, None, None), -1, "spasm_amd_kernel_batch: count < 0", ok_batch),
    ("solve_batch_negative_count", lambda c: c.lib.spasm_amd_solve_batch(-1, c.arr([c.A]), c.arr([c.A]), c.out1, c.okp1), -1, "spasm_amd_solve_batch: count < 0", ok_solve_batch),
    ("solve_batch_null_array", lambda c: c.lib.spasm_amd_solve_batch(1, None, None, c.out1, c.okp1), -1, "spasm_amd_solve_batch: NULL array", ok_solve_batch),
    # the dense finish over shards, out of order
    ("dshard_open_null", lambda c: c.lib.spasm_amd_dshard_open(None, 0, 1), NULL, "spasm_amd_dshard_open: spasm_amd_dshard_open: null plan", ok_solver),
    ("dshard_open_rows_null", lambda c: c.lib.spasm_amd_dshard_open_rows(None, 0, 1), NULL, "spasm_amd_dshard_open_rows: spasm_amd_dshard_open_rows: null shard", ok_solver),
    ("dshard_flags_unopened", lambda c: c.lib.spasm_amd_dshard_flags(None, None), -1, "spasm_amd_dshard_flags: no dense shard (spasm_amd_dshard_open comes first)", ok_solver),
    ("dshard_density_unopened", lambda c: c.lib.spasm_amd_dshard_density(None, None, 0, None), -1.0, "spasm_amd_dshard_density: no dense shard (spasm_amd_dshard_open comes first)", ok_solver),
    ("dshard_build_unopened", lambda c: c.lib.spasm_amd_dshard_build(None), -1, "spasm_amd_dshard_build: no dense shard (spasm_amd_dshard_open comes first)", ok_solver),
    ("dshard_info_unbuilt", lambda c: c.lib.spasm_amd_dshard_info(None, None, None, None, None, None, None), -1,
     "spasm_amd_dshard_info: no dense shard (spasm_amd_dshard_open / _density / _build come first)", ok_solver),
    ("dshard_pack_unbuilt", lambda c: c.lib.spasm_amd_dshard_pack(None, 0, None), -1, "spasm_amd_dshard_pack: no dense shard (spasm_amd_dshard_open / _density / _build come first)", ok_solver),
    ("dshard_finish_unbuilt", lambda c: c.lib.spasm_amd_dshard_finish(None), -1, "spasm_amd_dshard_finish: no dense shard (spasm_amd_dshard_open / _density / _build come first)", ok_solver),
    ("dshard_fetch_U_unbuilt", lambda c: c.lib.spasm_amd_dshard_fetch_U(None, None, None, None), NULL,
     "spasm_amd_dshard_fetch_U: no dense shard (spasm_amd_dshard_open / _density / _build come first)", ok_solver),
    ("schur_plan_prepare_null", lambda c: c.lib.spasm_amd_schur_plan_prepare(None), -1, "spasm_amd_schur_plan_prepare: null plan", ok_solver),
    ("schur_plan_fetch_U_null", lambda c: c.lib.spasm_amd_schur_plan_fetch_U(None, None, None), NULL, "spasm_amd_schur_plan_fetch_U: null plan", ok_solver),
    # the reference's entry points
    ("sparse_triangular_solve_null", lambda c: c.lib.spasm_sparse_triangular_solve(None, c.A.data, 0, c.ip(c.xj), c.ip(c.x), c.ip(c.q)), -1, "spasm_sparse_triangular_solve: null argument", ok_solver),
    ("sparse_triangular_solve_row_past_end", lambda c: c.lib.spasm_sparse_triangular_solve(c.U.data, c.A.data, 3, c.ip(c.xj), c.ip(c.x), c.ip(c.q)), -1, "spasm_sparse_triangular_solve: row out of range", ok_solver),
    ("sparse_triangular_solve_row_negative", lambda c: c.lib.spasm_sparse_triangular_solve(c.U.data, c.A.data, -1, c.ip(c.xj), c.ip(c.x), c.ip(c.q)), -1, "spasm_sparse_triangular_solve: row out of range", ok_solver),
    ("certificate_rank_create_null_matrix", lambda c: c.lib.spasm_certificate_rank_create(None, c.hash, C.byref(c.lu)), NULL, "spasm_certificate_rank_create: null argument", ok_solver),
    ("certificate_rank_create_null_fact", lambda c: c.lib.spasm_certificate_rank_create(c.A.data, c.hash, None), NULL, "spasm_certificate_rank_create: null argument", ok_solver),
    ("certificate_rank_create_no_qinv", lambda c: c.lib.spasm_certificate_rank_create(c.A.data, c.hash, C.byref(c.lu)), NULL, "spasm_certificate_rank_create: null argument", ok_solver),
    ("solve_without_L", lambda c: c.lib.spasm_solve(C.byref(c.lu), c.vp(c.b), c.vp(c.x)), False, "spasm_solve: null argument (a factorization with L is needed)", ok_solver),
    ("solve_null", lambda c: c.lib.spasm_solve(None, c.vp(c.b), c.vp(c.x)), False, "spasm_solve: null argument (a factorization with L is needed)", ok_solver),
    ("gesv_null", lambda c: c.lib.spasm_gesv(None, None, None), NULL, "spasm_gesv: incomplete factorization (U / qinv / p missing)", ok_solver),
]


@pytest.mark.parametrize("call,ret,text,then", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_a_failing_call_returns_its_failure_value_and_text_and_the_next_success_clears_it(ctx, call, ret, text, then):
    got = call(ctx)
    if ret is NULL:
        assert not got
    else:
        assert got == ret and type(got) is type(ret)
    assert ctx.S._abi.last_error() == text
    assert then(ctx) == ""
