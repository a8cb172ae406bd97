"""spasm.jl_amd -- MI355X-native sparse GF(p) echelonization behind SpaSM.jl's CSR / echelonize / kernel surface.

The directory name carries a dot, so import it as `spasm_jl_amd` (the loader module of that name
at the repository root registers this package).
"""
from . import _abi, blocks
from .blocks import Block
from .api import (
    CSR,
    DeviceBlocks,
    DeviceCSR,
    LU,
    EchelonizeOpts,
    Field,
    SpasmError,
    SpMV,
    TriangularSolver,
    Triplet,
    ZZp,
    RankCertificate,
    axpy,
    balanced,
    batch_stats,
    dense_back_solve,
    dense_forward_solve,
    certificate_rank_create,
    certificate_rank_verify,
    rank_certificate_load,
    rank_certificate_save,
    echelonize,
    echelonize_batch,
    echelonize_multi,
    factorization_verify,
    gesv,
    kernel,
    kernel_batch,
    last_rounds,
    load,
    nnz,
    prime0,
    rank,
    rank_batch,
    rref,
    save,
    scatter,
    solve,
    sparse,
    sparse_triangular_solve,
    sparse_triangular_solve_row,
    submatrix,
    synth_csr,
    transpose,
    xapy,
)

__all__ = [
    "Block", "blocks", "CSR", "LU", "Triplet", "load", "save", "EchelonizeOpts", "Field", "SpasmError", "ZZp", "balanced", "RankCertificate", "certificate_rank_create", "certificate_rank_verify", "rank_certificate_save", "rank_certificate_load", "echelonize", "echelonize_multi", "factorization_verify", "gesv", "solve", "kernel",
    "last_rounds", "nnz", "prime0", "rank", "rref", "sparse", "sparse_triangular_solve", "sparse_triangular_solve_row", "scatter", "synth_csr", "transpose",
    "axpy", "xapy", "SpMV", "dense_forward_solve", "dense_back_solve", "TriangularSolver",
    "DeviceCSR", "submatrix",
    "echelonize_batch", "rank_batch", "kernel_batch", "batch_stats",
    "DeviceBlocks",
]
