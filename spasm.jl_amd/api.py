"""Host-side mirror of SpaSM.jl's CSR / echelonize / kernel surface over the C ABI.

Julia is absent from this image, so the host side above the C ABI is written in Python with the
reference's names, argument meaning and error behaviour (reference src/SpaSM.jl, lines cited per
item).  Everything that computes goes through libspasm_amd.so; nothing here falls back to Python.
"""
import ctypes as C

import numpy as np

from . import _abi

prime0 = 42013  # reference src/SpaSM.jl:16


class SpasmError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------
# Field / ZZp  (reference src/SpaSM.jl:51-121)
# ---------------------------------------------------------------------------------------------
class Field:
    """Field(p): the finite field Z/pZ, 2 < p <= 0xfffffffb (reference src/SpaSM.jl:73-76)."""

    def __init__(self, p=prime0):
        p = int(p)
        if not (2 < p <= 0xFFFFFFFB):
            raise AssertionError("2 < p <= 0xfffffffb")  # the @assert at :74
        self.p = p
        self.halfp = p // 2
        self.mhalfp = p // 2 - p + 1
        self.dinvp = 1.0 / p

    def __call__(self, x):
        """Balanced representative of x (reference src/SpaSM.jl:83-88, :96)."""
        x = int(x) % self.p
        return x - self.p if x > self.halfp else x

    def __eq__(self, other):
        return isinstance(other, Field) and other.p == self.p

    def __hash__(self):
        return hash(self.p)

    def __repr__(self):
        return f"Field({self.p})"


def ZZp(F, x=None):
    """ZZp(F, x) / ZZp(p, x) / ZZp(x): balanced representative (reference src/SpaSM.jl:96-98)."""
    if x is None:
        return Field(prime0)(F)
    if not isinstance(F, Field):
        F = Field(F)
    return F(x)


def balanced(values, p):
    """Vectorised ZZp: integers -> balanced residues (reference src/SpaSM.jl:955-958)."""
    v = np.mod(np.asarray(values, dtype=np.int64), p)
    return np.where(2 * v > p, v - p, v).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# CSR  (reference src/SpaSM.jl:126-167, :941-1023)
# ---------------------------------------------------------------------------------------------
class CSR:
    """Spasm matrix in Compressed Sparse Row format, owned through the C ABI.

    CSR(m, prime) with a scipy sparse matrix or a 2-D array stores the TRANSPOSE: every column of
    `m` becomes a row (reference src/SpaSM.jl:941-968, README.md:7).  `transpose=False` stores `m`
    itself (one extra spasm_transpose, :967).
    """

    def __init__(self, src, prime=prime0, transpose=True, own=True):
        self._own = own
        if isinstance(src, C.POINTER(_abi.CsrStruct)):
            if not src:
                raise SpasmError("NULL spasm_csr: " + _abi.last_error())
            self.data = src
            return
        import scipy.sparse as sp

        A = sp.csc_matrix(src)
        if A.dtype.kind not in "iu":
            raise TypeError("integer entries expected")
        A.sum_duplicates()
        nrow_j, ncol_j = A.shape
        vals = balanced(A.data, prime)
        keep = vals != 0  # zeros are dropped (:959)
        col_of = np.repeat(np.arange(ncol_j), np.diff(A.indptr))
        counts = np.bincount(col_of[keep], minlength=ncol_j).astype(np.int64)
        nnz_ = int(keep.sum())
        ptr = _abi.lib().spasm_csr_alloc(ncol_j, nrow_j, nnz_, int(prime), True)  # csr_alloc(n,m,nzmax,prime) :944
        if not ptr:
            raise SpasmError("spasm_csr_alloc failed: " + _abi.last_error())
        self.data = ptr
        st = ptr.contents
        p = np.ctypeslib.as_array(st.p, (ncol_j + 1,))
        p[0] = 0
        np.cumsum(counts, out=p[1:])
        if nnz_:
            np.ctypeslib.as_array(st.j, (nnz_,))[:] = A.indices[keep]
            np.ctypeslib.as_array(st.x, (nnz_,))[:] = vals[keep]
        if not transpose:
            t = _abi.lib().spasm_transpose(self.data)
            if not t:
                raise SpasmError("spasm_transpose failed: " + _abi.last_error())
            _abi.lib().spasm_csr_free(self.data)
            self.data = t

    @classmethod
    def from_rows(cls, rows, m, prime=prime0):
        """Build directly from libspasm-side rows: rows[i] = list of (column, value)."""
        n = len(rows)
        nnz_ = sum(len(r) for r in rows)
        ptr = _abi.lib().spasm_csr_alloc(n, m, nnz_, int(prime), True)
        if not ptr:
            raise SpasmError("spasm_csr_alloc failed: " + _abi.last_error())
        self = cls(ptr)
        p, j, x = self.p, self.j, self.x
        k = 0
        F = Field(prime)
        for i, r in enumerate(rows):
            p[i] = k
            for (c, v) in r:
                j[k] = c
                x[k] = F(v)
                k += 1
        p[n] = k
        return self

    @classmethod
    def from_arrays(cls, n, m, p, j, x, prime=prime0):
        """Copy host CSR arrays (0-based, values already balanced) into an owned spasm_csr."""
        nnz_ = int(p[n])
        ptr = _abi.lib().spasm_csr_alloc(int(n), int(m), nnz_, int(prime), True)
        if not ptr:
            raise SpasmError("spasm_csr_alloc failed: " + _abi.last_error())
        self = cls(ptr)
        self.p[:] = np.asarray(p, dtype=np.int64)[: n + 1]
        if nnz_:
            self.j[:nnz_] = np.asarray(j, dtype=np.int32)[:nnz_]
            self.x[:nnz_] = np.asarray(x, dtype=np.int32)[:nnz_]
        return self

    def __del__(self):  # finalizer(csr_free, x), reference src/SpaSM.jl:146-150
        if getattr(self, "_own", False) and getattr(self, "data", None):
            try:
                _abi.lib().spasm_csr_free(self.data)
            except Exception:
                pass
            self.data = None

    # getproperty, reference src/SpaSM.jl:154-167: views, no copies
    @property
    def _st(self):
        return self.data.contents

    @property
    def n(self):
        return int(self._st.n)

    @property
    def m(self):
        return int(self._st.m)

    @property
    def nzmax(self):
        return int(self._st.nzmax)

    @property
    def prime(self):
        return int(self._st.field.p)

    @property
    def field(self):
        return Field(self.prime)

    @property
    def p(self):
        return np.ctypeslib.as_array(self._st.p, (self.n + 1,))

    @property
    def j(self):
        return np.ctypeslib.as_array(self._st.j, (max(self.nzmax, 1),))

    @property
    def x(self):
        return np.ctypeslib.as_array(self._st.x, (max(self.nzmax, 1),))

    @property
    def shape(self):  # Base.size, :229
        return (self.n, self.m)

    def __repr__(self):  # Base.show, :195
        return f"{self.n}×{self.m} CSR matrix % {self.prime} with {nnz(self)} (maximum {self.nzmax}) non-zeros"

    def rows(self):
        """libspasm-side rows as sorted lists of (column, balanced value)."""
        p, j, x = self.p, self.j, self.x
        out = []
        for i in range(self.n):
            lo, hi = int(p[i]), int(p[i + 1])
            out.append(sorted(zip(j[lo:hi].tolist(), x[lo:hi].tolist())))
        return out

    # `ndarray @ CSR` reaches __rmatmul__ only when numpy steps aside
    __array_ufunc__ = None

    def __matmul__(self, x):
        """A @ x (reference src/SpaSM.jl:658, A * x): x of shape (m,) or (m, k), integers (reduced mod p); a new int32 array of
        shape (n,) or (n, k).  A @ B with B a CSR (reference src/SpaSM.jl:995): the product as a new CSR in canonical form."""
        if isinstance(x, CSR):
            return _csr_mul(self, x)
        return _product(self, x, trans=False)

    # Matrix algebra (reference src/SpaSM.jl:995-1004), on the device (csrc/spgemm.hpp); results are canonical: columns ascending
    # inside each row, no zero stored.  `==` stays identity: equality as matrices is equals().
    def __add__(self, other):
        return _csr_lincomb(1, self, 1, other)

    def __sub__(self, other):
        return _csr_lincomb(1, self, -1, other)

    def __neg__(self):
        return _csr_lincomb(-1, self, 0, None)

    def __mul__(self, a):
        return _csr_lincomb(_int_scalar(a), self, 0, None)

    __rmul__ = __mul__

    def equals(self, other):
        """True when both are the same matrix over the same field, whatever the order of the stored entries."""
        if not isinstance(other, CSR):
            raise TypeError("a CSR expected")
        if self.shape != other.shape or self.prime != other.prime:
            return False
        with DeviceCSR(self) as a, DeviceCSR(other) as b:
            return a.equals(b)

    def __getitem__(self, key):
        """A[r0:r1, c0:c1] (reference src/SpaSM.jl:594-603): spasm_submatrix on the host, stored order kept."""
        rows, cols = _slice_pair(key, self.shape)
        return submatrix(self, rows, cols)

    def __rmatmul__(self, x):
        """x @ A (reference src/SpaSM.jl:645, x * A): x of shape (n,) or (k, n), integers (reduced mod p); a new int32 array of
        shape (m,) or (k, m)."""
        return _product(self, x, trans=True)

    def todense(self):
        """Dense libspasm-side matrix (n x m) of balanced residues."""
        D = np.zeros((self.n, self.m), dtype=np.int64)
        p, j, x = self.p, self.j, self.x
        for i in range(self.n):
            lo, hi = int(p[i]), int(p[i + 1])
            D[i, j[lo:hi]] = x[lo:hi]
        return D


def nnz(A):
    """SparseArrays.nnz (reference src/SpaSM.jl:432)."""
    return int(_abi.lib().spasm_nnz(A.data))


def sparse(A, transpose=True):
    """SparseMatrixCSC view of a CSR: column i = row i of the CSR, sorted (reference src/SpaSM.jl:1011-1023)."""
    import scipy.sparse as sp

    n, m = A.shape
    k = nnz(A)
    mat = sp.csc_matrix((A.x[:k].astype(np.int64), A.j[:k].astype(np.int64), A.p.astype(np.int64)), shape=(m, n))
    mat.sort_indices()
    return mat if transpose else mat.T.tocsc()


def transpose(A):
    """Base.transpose(::CSR) (reference src/SpaSM.jl:589)."""
    t = _abi.lib().spasm_transpose(A.data)
    if not t:
        raise SpasmError("spasm_transpose failed: " + _abi.last_error())
    return CSR(t)


# ---------------------------------------------------------------------------------------------
# Exact products y <- A x + y, y <- x A + y  (reference src/SpaSM.jl:640-658; csrc/spmv.hpp)
# ---------------------------------------------------------------------------------------------
def _host_vec(a, n, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.int32:
        raise TypeError(f"{name} must be an int32 numpy array")
    if a.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), not {a.shape}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be contiguous")
    return a


def _check_void(who):
    err = _abi.last_error()
    if err:
        raise SpasmError(err if err.startswith(who) else f"{who} failed: {err}")


def axpy(A, x, y):
    """axpy!(A, x, y) (reference src/SpaSM.jl:653-657): y <- A x + y in place and returned.  x: int32, A.m entries; y: int32,
    A.n entries (any int32 values; y ends as balanced residues)."""
    _host_vec(x, A.m, "x")
    _host_vec(y, A.n, "y")
    if not y.flags["WRITEABLE"]:
        raise ValueError("y must be writable")
    _abi.lib().spasm_Axpy(A.data, x.ctypes.data, y.ctypes.data)
    _check_void("spasm_Axpy")
    return y


def xapy(x, A, y):
    """xapy!(x, A, y) (reference src/SpaSM.jl:640-644): y <- x A + y in place and returned.  x: int32, A.n entries; y: int32,
    A.m entries."""
    _host_vec(x, A.n, "x")
    _host_vec(y, A.m, "y")
    if not y.flags["WRITEABLE"]:
        raise ValueError("y must be writable")
    _abi.lib().spasm_xApy(x.ctypes.data, A.data, y.ctypes.data)
    _check_void("spasm_xApy")
    return y


def _product(A, x, trans):
    """A @ x (trans=False) or x @ A (trans=True) as a new int32 array."""
    x = np.asarray(x)
    if x.dtype.kind not in "iu":
        raise TypeError("integer entries expected")
    inner, outer = (A.n, A.m) if trans else (A.m, A.n)
    if x.ndim == 1:
        if x.shape[0] != inner:
            raise ValueError(f"dimension mismatch: {A.shape} matrix and vector of {x.shape[0]} entries")
        xr = balanced(x, A.prime)
        y = np.zeros(outer, dtype=np.int32)
        return xapy(xr, A, y) if trans else axpy(A, xr, y)
    if x.ndim != 2:
        raise ValueError("a vector or a matrix expected")
    # x @ A with x of shape (k, n) is the block of the k products x_i A: the operator takes it as n x k
    X = balanced(x.T if trans else x, A.prime)
    if X.shape[0] != inner:
        raise ValueError(f"dimension mismatch: {A.shape} matrix and block of shape {x.shape}")
    with SpMV(A) as op:
        Y = op.apply(np.ascontiguousarray(X), trans=trans)
    return np.ascontiguousarray(Y.T) if trans else Y


class SpMV:
    """A resident on the device for repeated exact products (spasm_amd_spmv_*; engine extension).  A is the stored CSR, n x m
    (A.shape), and may be dropped once the operator exists.

    apply(X, Y=None, trans=False): Y <- A X + Y (trans=False: X is m x k, Y is n x k) or Y <- A^T X + Y, i.e. the k products
    x_i A with x_i the columns of X (trans=True: X is n x k, Y is m x k); X of shape (rows,) is one vector.  Y is updated in place
    and returned (None: zeros).  int32 numpy arrays, or int32 torch tensors on the current device (enqueued on the current
    stream).  The transpose is built on the device by the first trans=True apply and kept."""

    def __init__(self, A):
        self.shape = A.shape
        self.prime = A.prime
        self._op = _abi.lib().spasm_amd_spmv_create(A.data)
        if not self._op:
            raise SpasmError(_abi.last_error() or "spasm_amd_spmv_create failed")

    def close(self):
        op, self._op = getattr(self, "_op", None), None
        if op:
            _abi.lib().spasm_amd_spmv_free(op)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, X, Y=None, trans=False):
        if not self._op:
            raise SpasmError("the operator is closed")
        n, m = self.shape
        rin, rout = (n, m) if trans else (m, n)
        if type(X).__module__.startswith("torch"):
            return self._apply_torch(X, Y, bool(trans), rin, rout)
        if not isinstance(X, np.ndarray) or X.dtype != np.int32:
            raise TypeError("X must be an int32 numpy array or torch tensor")
        if X.ndim not in (1, 2) or X.shape[0] != rin:
            raise ValueError(f"X must have shape ({rin},) or ({rin}, k), not {X.shape}")
        k = 1 if X.ndim == 1 else X.shape[1]
        if Y is None:
            Y = np.zeros((rout,) + X.shape[1:], dtype=np.int32)
        if not isinstance(Y, np.ndarray) or Y.dtype != np.int32:
            raise TypeError("Y must be an int32 numpy array")
        if Y.shape != (rout,) + X.shape[1:]:
            raise ValueError(f"Y must have shape {(rout,) + X.shape[1:]}, not {Y.shape}")
        if not Y.flags["WRITEABLE"]:
            raise ValueError("Y must be writable")
        Xc = _rows_view(X, "X")
        Yc = _rows_view(Y, "Y")
        ldx = k if X.ndim == 1 else max(Xc.strides[0] // 4, k)
        ldy = k if Y.ndim == 1 else max(Yc.strides[0] // 4, k)
        rc = _abi.lib().spasm_amd_spmv_apply(self._op, int(trans), int(k), Xc.ctypes.data, ldx, Yc.ctypes.data, ldy)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return Y

    def _apply_torch(self, X, Y, trans, rin, rout):
        import torch

        if X.dtype != torch.int32 or X.device.type != "cuda" or X.device.index != torch.cuda.current_device():
            raise TypeError("X must be an int32 tensor on the current device")
        if X.dim() not in (1, 2) or X.shape[0] != rin:
            raise ValueError(f"X must have shape ({rin},) or ({rin}, k), not {tuple(X.shape)}")
        k = 1 if X.dim() == 1 else X.shape[1]
        if Y is None:
            Y = torch.zeros((rout,) + tuple(X.shape[1:]), dtype=torch.int32, device=X.device)
        if Y.dtype != torch.int32 or Y.device != X.device:
            raise TypeError("Y must be an int32 tensor on the device of X")
        if tuple(Y.shape) != (rout,) + tuple(X.shape[1:]):
            raise ValueError(f"Y must have shape {(rout,) + tuple(X.shape[1:])}, not {tuple(Y.shape)}")
        for t, name in ((X, "X"), (Y, "Y")):
            if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < k):
                raise ValueError(f"{name} must have unit stride along its rows")
        if X.data_ptr() == Y.data_ptr():
            raise ValueError("X and Y must not overlap")
        ldx = k if X.dim() == 1 else max(X.stride(0), k)
        ldy = k if Y.dim() == 1 else max(Y.stride(0), k)
        stream = torch.cuda.current_stream().cuda_stream
        rc = _abi.lib().spasm_amd_spmv_apply_dev(self._op, int(trans), int(k), C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy,
                                                  C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return Y


def _rows_view(a, name):
    """a itself when its rows are unit-stride and laid out at a positive leading dimension (what the C call takes)"""
    if a.ndim == 1:
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{name} must be contiguous")
        return a
    if a.strides[1] != 4 or (a.shape[0] > 1 and a.strides[0] < 4 * a.shape[1]) or a.strides[0] % 4:
        raise ValueError(f"{name} must have unit stride along its rows")
    return a


# ---------------------------------------------------------------------------------------------
# Matrix algebra: A B, a A + b B, submatrix  (reference src/SpaSM.jl:594-603, :995-1004; csrc/spgemm.hpp)
# ---------------------------------------------------------------------------------------------
def _int_scalar(a):
    if isinstance(a, (bool, np.bool_)) or not isinstance(a, (int, np.integer)):
        raise TypeError("an integer scalar expected")
    a = int(a)
    if not -(2**63) <= a < 2**63:
        raise ValueError("the scalar must fit 64 bits")
    return a


def _same_field(A, B):
    if A.prime != B.prime:
        raise ValueError(f"the matrices are over different primes: {A.prime} and {B.prime}")


def _slice_pair(key, shape):
    """(rows, cols) as ranges from A[r, c] with step-1 slices"""
    if not isinstance(key, tuple) or len(key) != 2:
        raise TypeError("two slices expected: A[r0:r1, c0:c1]")
    out = []
    for k, size in zip(key, shape):
        if not isinstance(k, slice):
            raise TypeError("slices expected: A[r0:r1, c0:c1]")
        if k.step not in (None, 1):
            raise ValueError("slices with a step are not supported")
        lo, hi, _ = k.indices(size)
        out.append(range(lo, max(hi, lo)))
    return out[0], out[1]


def _range_bounds(r, name):
    if isinstance(r, slice):
        raise TypeError(f"{name} must be a range")
    r = range(*r) if isinstance(r, tuple) else r
    if not isinstance(r, range):
        raise TypeError(f"{name} must be a range")
    if r.step != 1:
        raise ValueError("ranges with a step are not supported")
    return r.start, r.stop  # (an inverted or outside range is the library's to refuse)


def submatrix(A, rows, cols, with_values=True):
    """submatrix(A, r, c, with_values) (reference src/SpaSM.jl:594-597) with Python ranges: rows and columns of A as a new CSR,
    columns renumbered from cols.start, the entries of each row in their stored order; without values x is NULL.  Host-side."""
    r0, r1 = _range_bounds(rows, "rows")
    c0, c1 = _range_bounds(cols, "cols")
    ptr = _abi.lib().spasm_submatrix(A.data, r0, r1, c0, c1, bool(with_values))
    if not ptr:
        raise SpasmError(_abi.last_error() or "spasm_submatrix failed")
    return CSR(ptr)


def _csr_mul(A, B):
    if A.m != B.n:
        raise ValueError(f"dimension mismatch: {A.shape} times {B.shape}")
    _same_field(A, B)
    ptr = _abi.lib().spasm_amd_csr_mul(A.data, B.data)
    if not ptr:
        raise SpasmError(_abi.last_error() or "spasm_amd_csr_mul failed")
    return CSR(ptr)


def _csr_lincomb(a, A, b, B):
    if B is not None:
        if not isinstance(B, CSR):
            raise TypeError("a CSR expected")
        if A.shape != B.shape:
            raise ValueError(f"dimension mismatch: {A.shape} and {B.shape}")
        _same_field(A, B)
    ptr = _abi.lib().spasm_amd_csr_lincomb(_int_scalar(a), A.data, _int_scalar(b), B.data if B is not None else None)
    if not ptr:
        raise SpasmError(_abi.last_error() or "spasm_amd_csr_lincomb failed")
    return CSR(ptr)


class DeviceCSR:
    """An n x m matrix over GF(p) resident on the device (spasm_amd_dcsr_*; engine extension).  DeviceCSR(A) uploads the CSR A,
    which may be dropped afterwards.  D1 @ D2, D1 + D2, D1 - D2, -D, a * D, D * a (Python int), D[r0:r1, c0:c1] make new resident
    matrices in canonical form (columns ascending inside each row, no zero stored) without crossing the host; download() gives
    a CSR; equals() compares as matrices; stats() describes the operation that made the matrix.

    D.T / D.transpose(), D.permute(p, q) (what numpy's A[np.ix_(p, q)] gives; qinv= takes the inverse column map instead),
    vcat(D1, D2, ..) / D1.vcat(D2, ..) (rows stacked) and hcat(D1, D2, ..) / D1.hcat(D2, ..) (side by side) move entries without
    touching their values (spasm_amd_dcsr_transpose / _permute / _vcat / _hcat; csrc/reshape.hpp); the results are canonical too.
    For these four, stats() reads: flops = entries = the entries moved; rows_tiny / rows_hash / rows_global = the rows whose
    columns were put in order by the one-wave, the workgroup and the long-row path (0 where nothing had to be ordered: vcat,
    hcat, a permutation of rows alone); chunks = 1; ms_size / ms_numeric / ms_compact = the count, move and order steps;
    scratch_bytes = peak scratch; op = 4 transpose, 5 permute, 6 vcat, 7 hcat; max_bound = the longest row of the result."""

    STATS = ("flops", "entries", "rows_tiny", "rows_hash", "rows_global", "chunks", "ms_size", "ms_numeric", "ms_compact", "scratch_bytes", "op", "max_bound")

    def __init__(self, A, _handle=None):
        if _handle is not None:
            self._h = _handle
        else:
            if not isinstance(A, CSR):
                raise TypeError("a CSR expected")
            self._h = _abi.lib().spasm_amd_dcsr_upload(A.data)
            if not self._h:
                raise SpasmError(_abi.last_error() or "spasm_amd_dcsr_upload failed")
        out = (C.c_int64 * 4)()
        _abi.lib().spasm_amd_dcsr_info(self._h, out)
        self.shape = (int(out[0]), int(out[1]))
        self.nnz = int(out[2])
        self.prime = int(out[3])

    @classmethod
    def _wrap(cls, handle, who):
        if not handle:
            raise SpasmError(_abi.last_error() or f"{who} failed")
        return cls(None, _handle=handle)

    def _need(self):
        if not getattr(self, "_h", None):
            raise SpasmError("the matrix is closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _abi.lib().spasm_amd_dcsr_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def download(self):
        ptr = _abi.lib().spasm_amd_dcsr_download(self._need())
        if not ptr:
            raise SpasmError(_abi.last_error() or "spasm_amd_dcsr_download failed")
        return CSR(ptr)

    def stats(self):
        out = (C.c_int64 * 12)()
        _abi.lib().spasm_amd_dcsr_stats(self._need(), out)
        d = {k: int(v) for k, v in zip(self.STATS, out)}
        for k in ("ms_size", "ms_numeric", "ms_compact"):
            d[k] = d[k] / 1000.0  # the library counts microseconds
        return d

    def _other(self, other):
        if not isinstance(other, DeviceCSR):
            raise TypeError("a DeviceCSR expected")
        h = other._need()
        _same_field(self, other)
        return h

    def __matmul__(self, other):
        if not isinstance(other, DeviceCSR):
            return NotImplemented
        me, h = self._need(), self._other(other)
        if self.shape[1] != other.shape[0]:
            raise ValueError(f"dimension mismatch: {self.shape} times {other.shape}")
        return DeviceCSR._wrap(_abi.lib().spasm_amd_dcsr_mul(me, h), "spasm_amd_dcsr_mul")

    def lincomb(self, a, b=0, other=None):
        """a * self + b * other (other None: a * self)"""
        me, h = self._need(), None
        if other is not None:
            h = self._other(other)
            if self.shape != other.shape:
                raise ValueError(f"dimension mismatch: {self.shape} and {other.shape}")
        return DeviceCSR._wrap(_abi.lib().spasm_amd_dcsr_lincomb(_int_scalar(a), me, _int_scalar(b), h), "spasm_amd_dcsr_lincomb")

    def __add__(self, other):
        return self.lincomb(1, 1, other) if isinstance(other, DeviceCSR) else NotImplemented

    def __sub__(self, other):
        return self.lincomb(1, -1, other) if isinstance(other, DeviceCSR) else NotImplemented

    def __neg__(self):
        return self.lincomb(-1)

    def __mul__(self, a):
        return self.lincomb(_int_scalar(a))

    __rmul__ = __mul__

    def __getitem__(self, key):
        me = self._need()
        rows, cols = _slice_pair(key, self.shape)
        return DeviceCSR._wrap(_abi.lib().spasm_amd_dcsr_submatrix(me, rows.start, rows.stop, cols.start, cols.stop), "spasm_amd_dcsr_submatrix")

    def equals(self, other):
        if not isinstance(other, DeviceCSR):
            raise TypeError("a DeviceCSR expected")
        rc = _abi.lib().spasm_amd_dcsr_equal(self._need(), other._need())
        if rc < 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_dcsr_equal failed")
        return bool(rc)

    def transpose(self):
        """the transpose as a new resident matrix"""
        return DeviceCSR._wrap(_abi.lib().spasm_amd_dcsr_transpose(self._need()), "spasm_amd_dcsr_transpose")

    T = property(transpose)

    def permute(self, p=None, q=None, *, qinv=None):
        """Row i of the result is row p[i]; with q, column k of the result is column q[k] (numpy's A[np.ix_(p, q)]); with qinv,
        an entry on column j lands on column qinv[j].  None is the identity."""
        me = self._need()
        if q is not None and qinv is not None:
            raise ValueError("give q or qinv, not both")
        n, m = self.shape
        p = _permutation(p, n, "p")
        if q is not None:
            q = _permutation(q, m, "q")
            qinv = np.empty(m, dtype=np.int32)
            qinv[q] = np.arange(m, dtype=np.int32)
        else:
            qinv = _permutation(qinv, m, "qinv")
        as_ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        return DeviceCSR._wrap(_abi.lib().spasm_amd_dcsr_permute(me, as_ptr(p), as_ptr(qinv)), "spasm_amd_dcsr_permute")

    def vcat(self, *others):
        return vcat(self, *others)

    def hcat(self, *others):
        return hcat(self, *others)


def _permutation(a, size, name):
    """a as a contiguous int32 array after checking that it is a permutation of range(size); None stays None"""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be an array of integers")
    if a.shape != (size,):
        raise ValueError(f"{name} must have {size} entries, it has shape {a.shape}")
    seen = np.zeros(size, dtype=bool)
    if size and (a.min() < 0 or a.max() >= size):
        raise ValueError(f"{name} is not a permutation: an index lies outside 0 .. {size - 1}")
    seen[a] = True
    if not seen.all():
        raise ValueError(f"{name} is not a permutation: an index is repeated")
    return np.ascontiguousarray(a, dtype=np.int32)


def _cat(sym, axis, Ds):
    if not Ds:
        raise ValueError("at least one DeviceCSR is needed")
    for D in Ds:
        if not isinstance(D, DeviceCSR):
            raise TypeError("a DeviceCSR expected")
    hs = [D._need() for D in Ds]
    for D in Ds[1:]:
        if D.shape[axis] != Ds[0].shape[axis]:
            raise ValueError(f"dimension mismatch: {Ds[0].shape} and {D.shape}")
        _same_field(Ds[0], D)
    arr = (C.c_void_p * len(hs))(*hs)
    return DeviceCSR._wrap(getattr(_abi.lib(), sym)(len(hs), arr), sym)


def vcat(*Ds):
    """the resident matrices stacked, rows of the first on top (equal column counts), in one pass"""
    return _cat("spasm_amd_dcsr_vcat", 1, Ds)


def hcat(*Ds):
    """the resident matrices side by side (equal row counts), in one pass"""
    return _cat("spasm_amd_dcsr_hcat", 0, Ds)


# ---------------------------------------------------------------------------------------------
# Dense triangular solves x T = b  (reference src/SpaSM.jl:663-692; csrc/trsolve.hpp)
# ---------------------------------------------------------------------------------------------
def _dense_solve(sym, T, b, x, piv, npiv):
    _host_vec(b, T.m, "b")
    _host_vec(x, T.n, "x")
    _host_vec(piv, npiv, "q" if sym == "spasm_dense_forward_solve" else "p")
    if not b.flags["WRITEABLE"] or not x.flags["WRITEABLE"]:
        raise ValueError("b and x must be writable")
    ok = getattr(_abi.lib(), sym)(T.data, b.ctypes.data, x.ctypes.data, piv.ctypes.data)
    if not ok:
        _check_void(sym)
    return bool(ok)


def dense_forward_solve(U, b, x, q):
    """dense_forward_solve(U, b, x, q) (reference src/SpaSM.jl:688-692): solves x U = b.  U: n x m with unit pivots, q[i] the
    pivot column of row i (< 0: none); b: int32, m entries, overwritten by the residual b - x U; x: int32, n entries, filled.
    True iff the residual is zero; SpasmError on a malformed U (pivot out of range or twice, non-unit pivot, cycle)."""
    return _dense_solve("spasm_dense_forward_solve", U, b, x, q, U.n)


def dense_back_solve(L, b, x, p):
    """dense_back_solve(L, b, x, p) (reference src/SpaSM.jl:673-677): solves x L = b.  L: n x m, p[j] the row whose diagonal
    entry (non-zero) is on column j (< 0: none); b: int32, m entries, overwritten by the residual; x: int32, n entries, filled.
    True iff the residual is zero; SpasmError on a malformed L (pivot out of range or twice, zero diagonal, cycle)."""
    return _dense_solve("spasm_dense_back_solve", L, b, x, p, L.m)


class TriangularSolver:
    """T resident on the device for repeated solves x T = b (spasm_amd_trsolve_*; engine extension).  kind="forward": piv = q
    (n entries, pivot column of each row, unit pivots); kind="back": piv = p (m entries, row of each column's diagonal).  T may be
    dropped once the solver exists.

    solve(B, X=None) -> (X, ok): B is m x k (the right-hand sides as columns; shape (m,) is one vector) and is overwritten by the
    residuals; X (n x k, filled) and ok (k flags, or one for a vector) are returned.  int32 numpy arrays, or int32 torch tensors
    on the current device (enqueued on the current stream; ok is then a bool tensor)."""

    def __init__(self, T, piv, kind="forward"):
        if kind not in ("forward", "back"):
            raise ValueError('kind must be "forward" or "back"')
        n, m = T.shape
        if not isinstance(piv, np.ndarray) or piv.dtype != np.int32:
            raise TypeError("piv must be an int32 numpy array")
        npiv = n if kind == "forward" else m
        if piv.shape != (npiv,):
            raise ValueError(f"piv must have shape ({npiv},), not {piv.shape}")
        piv = np.ascontiguousarray(piv)
        self.shape = (n, m)
        self.prime = T.prime
        self.kind = kind
        self._op = _abi.lib().spasm_amd_trsolve_create(T.data, piv.ctypes.data, 0 if kind == "forward" else 1)
        if not self._op:
            raise SpasmError(_abi.last_error() or "spasm_amd_trsolve_create failed")

    @classmethod
    def from_lu(cls, fact):
        """The forward solver on fact.U, with q the inverse of fact.qinv"""
        U = fact.U
        qinv = np.asarray(fact.qinv)
        q = np.full(U.n, -1, dtype=np.int32)
        cols = np.flatnonzero(qinv >= 0)
        q[qinv[cols]] = cols
        return cls(U, q, "forward")

    def stats(self):
        """n, m, participating rows, levels, wide panels, chunks, kernels per apply (k <= 64), stored entries"""
        out = (C.c_int64 * 8)()
        _abi.lib().spasm_amd_trsolve_stats(self._op, out)
        keys = ("n", "m", "rows", "levels", "wide_panels", "chunks", "launches", "entries")
        return dict(zip(keys, [int(v) for v in out]))

    def close(self):
        op, self._op = getattr(self, "_op", None), None
        if op:
            _abi.lib().spasm_amd_trsolve_free(op)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, B, X=None):
        if not self._op:
            raise SpasmError("the solver is closed")
        n, m = self.shape
        if type(B).__module__.startswith("torch"):
            return self._solve_torch(B, X, n, m)
        if not isinstance(B, np.ndarray) or B.dtype != np.int32:
            raise TypeError("B must be an int32 numpy array or torch tensor")
        if B.ndim not in (1, 2) or B.shape[0] != m:
            raise ValueError(f"B must have shape ({m},) or ({m}, k), not {B.shape}")
        if not B.flags["WRITEABLE"]:
            raise ValueError("B must be writable")
        k = 1 if B.ndim == 1 else B.shape[1]
        if X is None:
            X = np.zeros((n,) + B.shape[1:], dtype=np.int32)
        if not isinstance(X, np.ndarray) or X.dtype != np.int32:
            raise TypeError("X must be an int32 numpy array")
        if X.shape != (n,) + B.shape[1:]:
            raise ValueError(f"X must have shape {(n,) + B.shape[1:]}, not {X.shape}")
        if not X.flags["WRITEABLE"]:
            raise ValueError("X must be writable")
        if k == 0:
            return X, np.zeros(0, dtype=bool)
        Bc = _rows_view(B, "B")
        Xc = _rows_view(X, "X")
        ldb = k if B.ndim == 1 else max(Bc.strides[0] // 4, k)
        ldx = k if X.ndim == 1 else max(Xc.strides[0] // 4, k)
        ok = np.zeros(k, dtype=np.uint8)
        rc = _abi.lib().spasm_amd_trsolve_apply(self._op, int(k), Bc.ctypes.data, ldb, Xc.ctypes.data, ldx, ok.ctypes.data)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        ok = ok.astype(bool)
        return X, (bool(ok[0]) if B.ndim == 1 else ok)

    def _solve_torch(self, B, X, n, m):
        import torch

        if B.dtype != torch.int32 or B.device.type != "cuda" or B.device.index != torch.cuda.current_device():
            raise TypeError("B must be an int32 tensor on the current device")
        if B.dim() not in (1, 2) or B.shape[0] != m:
            raise ValueError(f"B must have shape ({m},) or ({m}, k), not {tuple(B.shape)}")
        k = 1 if B.dim() == 1 else B.shape[1]
        if X is None:
            X = torch.zeros((n,) + tuple(B.shape[1:]), dtype=torch.int32, device=B.device)
        if X.dtype != torch.int32 or X.device != B.device:
            raise TypeError("X must be an int32 tensor on the device of B")
        if tuple(X.shape) != (n,) + tuple(B.shape[1:]):
            raise ValueError(f"X must have shape {(n,) + tuple(B.shape[1:])}, not {tuple(X.shape)}")
        for t, name in ((B, "B"), (X, "X")):
            if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < k):
                raise ValueError(f"{name} must have unit stride along its rows")
        if n > 0 and m > 0 and B.data_ptr() == X.data_ptr():
            raise ValueError("B and X must not overlap")
        ldb = k if B.dim() == 1 else max(B.stride(0), k)
        ldx = k if X.dim() == 1 else max(X.stride(0), k)
        ok = torch.empty(max(k, 1), dtype=torch.uint8, device=B.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = _abi.lib().spasm_amd_trsolve_apply_dev(self._op, int(k), C.c_void_p(B.data_ptr()), ldb, C.c_void_p(X.data_ptr()), ldx,
                                                    C.c_void_p(ok.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        ok = ok[:k].bool()
        return X, (ok[0] if B.dim() == 1 else ok)


# ---------------------------------------------------------------------------------------------
# LU / echelonize / kernel / rank  (reference src/SpaSM.jl:262-305, :814-884, :1147-1149)
# ---------------------------------------------------------------------------------------------
class EchelonizeOpts:
    """EchelonizeOpts() filled by spasm_echelonize_init_opts (reference src/SpaSM.jl:817)."""

    def __init__(self, **kwargs):
        self.struct = _abi.EchelonizeOptsStruct()
        _abi.lib().spasm_echelonize_init_opts(C.byref(self.struct))
        for k, v in kwargs.items():  # parse_echelonize_opts, :819-824
            if not hasattr(self.struct, k):
                raise AttributeError(f"type EchelonizeOpts has no field {k}")
            setattr(self.struct, k, v)

    def __getattr__(self, k):
        return getattr(self.__dict__["struct"], k)


class LU:
    def __init__(self, ptr):
        if not ptr:
            raise SpasmError("spasm_echelonize failed: " + _abi.last_error())
        self.data = ptr

    @classmethod
    def from_parts(cls, U, qinv, p, L=None):
        """An LU from its parts (layout reference src/SpaSM.jl:262-270), e.g. assembled from the rounds of the row-sharded
        echelonize.  U (and L, when given): CSRs whose ownership passes to the LU; qinv: m entries (row of U or -1); p: max(n, m)
        entries.  Everything is malloc'ed so that spasm_lu_free releases it like an LU of spasm_echelonize."""
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]
        qinv = np.ascontiguousarray(qinv, dtype=np.int32)
        p = np.ascontiguousarray(p, dtype=np.int32)

        def dup(a):
            mem = libc.malloc(max(a.nbytes, 4))
            if not mem:
                raise MemoryError("malloc")
            C.memmove(mem, a.ctypes.data, a.nbytes)
            return C.cast(mem, C.POINTER(C.c_int32))

        mem = libc.malloc(C.sizeof(_abi.LuStruct))
        if not mem:
            raise MemoryError("malloc")
        st = C.cast(mem, C.POINTER(_abi.LuStruct))
        st.contents.r = int(U.n)
        st.contents.complete = False
        st.contents.L = L.data if L is not None else None
        if L is not None:
            L._own = False
        st.contents.U = U.data
        st.contents.qinv = dup(qinv)
        st.contents.p = dup(p)
        st.contents.Ltmp = None
        U._own = False  # now owned by the LU
        return cls(st)

    def __del__(self):  # finalizer(lu_free, x), reference src/SpaSM.jl:273-277
        if getattr(self, "data", None):
            try:
                _abi.lib().spasm_lu_free(self.data)
            except Exception:
                pass
            self.data = None

    @property
    def r(self):
        return int(self.data.contents.r)

    @property
    def complete(self):
        return bool(self.data.contents.complete)

    @property
    def U(self):
        st = self.data.contents
        if not st.U:
            raise SpasmError("M.U is null")  # :291
        return CSR(st.U, own=False)

    @property
    def L(self):
        st = self.data.contents
        if not st.L:
            raise SpasmError("M.L is null")  # :288
        return CSR(st.L, own=False)

    @property
    def qinv(self):
        st = self.data.contents
        if not st.qinv:
            raise SpasmError("M.qinv is null")
        return np.ctypeslib.as_array(st.qinv, (max(int(st.U.contents.m), 1),))[: int(st.U.contents.m)]

    @property
    def p(self):
        st = self.data.contents
        if not st.p:
            raise SpasmError("M.p is null")
        return np.ctypeslib.as_array(st.p, (max(int(st.U.contents.m), 1),))[: int(st.U.contents.m)]


def echelonize(A, opts=None, verbose=False, **kwargs):
    """echelonize(A; kwargs...) -> LU (reference src/SpaSM.jl:860-866)."""
    if opts is None:
        opts = EchelonizeOpts()
    for k, v in kwargs.items():
        if not hasattr(opts.struct, k):
            raise AttributeError(f"type EchelonizeOpts has no field {k}")
        setattr(opts.struct, k, v)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_echelonize(A.data, C.byref(opts.struct))
    return LU(ptr)


def echelonize_multi(A, nshards, opts=None, verbose=False, **kwargs):
    """echelonize over `nshards` row shards on the devices of this process (spasm_amd_echelonize_multi; engine extension): the
    LU of echelonize(A; enable_greedy_pivot_search=false) whatever nshards is -- same rank, pivot columns and kernel."""
    if opts is None:
        opts = EchelonizeOpts()
    for k, v in kwargs.items():
        if not hasattr(opts.struct, k):
            raise AttributeError(f"type EchelonizeOpts has no field {k}")
        setattr(opts.struct, k, v)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_amd_echelonize_multi(A.data, C.byref(opts.struct), int(nshards))
    return LU(ptr)


def kernel(A, verbose=False, **kwargs):
    """kernel(fact::LU) / kernel(A::CSR) (reference src/SpaSM.jl:876-882, :1147)."""
    fact = A if isinstance(A, LU) else echelonize(A, verbose=verbose, **kwargs)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_kernel(fact.data)
    if not ptr:
        raise SpasmError("spasm_kernel failed: " + _abi.last_error())
    return CSR(ptr)


def scatter(A, i, beta, x):
    """scatter(A, i, beta, x): x += beta * A[i] (reference src/SpaSM.jl:619-620; i 0-based here, as on the C side).  x: int32
    array of m balanced residues, updated in place."""
    assert x.dtype == np.int32 and x.flags["C_CONTIGUOUS"] and len(x) >= A.m and 0 <= i < A.n
    _abi.lib().spasm_scatter(A.data, int(i), int(beta), x.ctypes.data_as(C.POINTER(C.c_int32)))
    return x


def sparse_triangular_solve_row(U, B, k, xj, x, qinv, verbose=False):
    """sparse_triangular_solve(U, B, k, xj, x, qinv) (reference src/SpaSM.jl:694-722; k 0-based): solve x * U = B[k].  xj: int32,
    3 m entries, zero on entry; x: int32, m entries.  Returns top: the pattern of the solution is xj[top:m], its values x[xj[...]];
    with x_b on the pivot columns and x_a on the others, x_b * U + x_a == B[k]."""
    m = U.m
    assert m == B.m == len(qinv) and 0 <= k < B.n                     # the reference's assertions (:715-720)
    assert xj.dtype == np.int32 and len(xj) >= 3 * m and not xj.any()
    assert x.dtype == np.int32 and len(x) >= m
    q = np.ascontiguousarray(qinv, dtype=np.int32)
    with _quiet(not verbose):
        top = _abi.lib().spasm_sparse_triangular_solve(U.data, B.data, int(k), xj.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        x.ctypes.data_as(C.POINTER(C.c_int32)), q.ctypes.data_as(C.POINTER(C.c_int32)))
    if top < 0:
        raise SpasmError("spasm_sparse_triangular_solve failed: " + _abi.last_error())
    return int(top)


def sparse_triangular_solve(U, B, qinv=None, verbose=False):
    """sparse_triangular_solve(LU, B) / sparse_triangular_solve(U, B, qinv) (reference src/SpaSM.jl:725-755): solve X * U == B in
    sparse matrices; returns X (rows of B x rows of U), or None if some row of B has no solution.  One device pass over all
    rows of B (spasm_amd_triangular_solve)."""
    if isinstance(U, LU):
        U, qinv = U.U, U.qinv
    X, ok = _triangular_solve(U, B, qinv, verbose)
    return X if bool(ok.all()) else None


def _triangular_solve(U, B, qinv, verbose=False):
    """(X, ok): x_b of every row of B and whether its x_a is empty (reference src/SpaSM.jl:694-713)"""
    q = np.ascontiguousarray(qinv, dtype=np.int32)
    ok = np.zeros(max(B.n, 1), dtype=np.uint8)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_amd_triangular_solve(U.data, q.ctypes.data_as(C.POINTER(C.c_int32)), B.data, ok.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if not ptr:
        raise SpasmError("spasm_amd_triangular_solve failed: " + _abi.last_error())
    return CSR(ptr), ok[: B.n].astype(bool)


def rref(fact, verbose=False):
    """rref(fact) -> (R, Rqinv) (reference src/SpaSM.jl:871): reduced row echelon form of fact.U; Rqinv[j] = row of R whose
    pivot is column j, or -1."""
    m = fact.U.m
    rq = np.full(max(m, 1), -1, dtype=np.int32)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_rref(fact.data, rq.ctypes.data_as(C.POINTER(C.c_int32)))
    if not ptr:
        raise SpasmError("spasm_rref failed: " + _abi.last_error())
    return CSR(ptr), rq[:m]


def gesv(fact, B, verbose=False):
    """gesv(fact::LU, B::CSR) (reference src/SpaSM.jl:907-923): solve X * A == B where A has been echelonized as `fact` WITH its
    L factor (echelonize(A, L=True)).  Returns (X, ok): X is rows(B) x rows(A); ok[k] says whether row k of B has a solution."""
    ok = np.zeros(max(B.n, 1), dtype=np.uint8)
    with _quiet(not verbose):
        ptr = _abi.lib().spasm_gesv(fact.data, B.data, ok.ctypes.data)
    if not ptr:
        raise SpasmError("spasm_gesv failed: " + _abi.last_error())
    return CSR(ptr), ok[: B.n].astype(bool)


def solve(fact, b, x=None):
    """solve(fact::LU, b::Vector) (reference src/SpaSM.jl:889-905): x with x * A == b, or None when there is none.  b has one entry
    per column of A, x one per ROW OF A (the prototype sizes x by fact.U.n; see include/spasm_amd.h)."""
    st = fact.data.contents
    if not st.L:
        raise SpasmError("M.L is null")  # fact.L, :896
    m, n = int(st.U.contents.m), int(st.L.contents.n)
    b = np.ascontiguousarray(b, dtype=np.int32)
    if b.shape != (m,):
        raise ValueError(f"b must have {m} entries")
    if x is None:
        x = np.zeros(n, dtype=np.int32)
    elif x.shape != (n,) or x.dtype != np.int32:
        raise ValueError(f"x must be an int32 vector of {n} entries")
    okv = _abi.lib().spasm_solve(fact.data, b.ctypes.data, x.ctypes.data)
    if not okv and _abi.last_error():
        raise SpasmError("spasm_solve failed: " + _abi.last_error())
    return x if okv else None


def factorization_verify(A, fact, seed=0):
    """factorization_verify(A, fact, seed) (reference src/SpaSM.jl:934): probabilistic self-check, on the host, that the row
    space of A lies in the span of fact.U and that U has echelon shape (so rank(A) <= fact.r).  With L = NULL the converse
    inclusion is not checked (include/spasm_amd.h)."""
    return bool(_abi.lib().spasm_factorization_verify(A.data, fact.data, int(seed) & 0xFFFFFFFFFFFFFFFF))


def rank(A, rank_only=False, verbose=False, **kwargs):
    """rank(N::LU) = N.r; rank(A::CSR) = rank(echelonize(A)) (reference src/SpaSM.jl:305, :1149).  rank_only=True (engine extension,
    spasm_amd_rank): the rows of U are counted on the device and never assembled on the host -- for matrices whose U outgrows it."""
    if isinstance(A, LU):
        return A.r
    if not rank_only:
        return echelonize(A, verbose=verbose, **kwargs).r
    opts = EchelonizeOpts()
    for k, v in kwargs.items():
        if not hasattr(opts.struct, k):
            raise AttributeError(f"type EchelonizeOpts has no field {k}")
        setattr(opts.struct, k, v)
    with _quiet(not verbose):
        r = _abi.lib().spasm_amd_rank(A.data, C.byref(opts.struct))
    if r < 0:
        raise SpasmError("spasm_amd_rank failed: " + _abi.last_error())
    return int(r)


# ---------------------------------------------------------------------------------------------
# Many small matrices in one call  (spasm_amd_*_batch; csrc/batch.hpp; engine extension)
# ---------------------------------------------------------------------------------------------
BATCH_STATS = ("matrices", "lds_path", "general_path", "chunks", "launches", "device_us", "entries", "max_image_words")


def _batch_args(mats, opts, kwargs):
    mats = list(mats)
    for A in mats:
        if not isinstance(A, CSR):
            raise TypeError("a list of CSR expected")
    if opts is None:
        opts = EchelonizeOpts()
    for k, v in kwargs.items():
        if not hasattr(opts.struct, k):
            raise AttributeError(f"type EchelonizeOpts has no field {k}")
        setattr(opts.struct, k, v)
    arr = (C.POINTER(_abi.CsrStruct) * max(len(mats), 1))(*[A.data for A in mats])
    return mats, opts, arr


def echelonize_batch(mats, opts=None, verbose=False, **kwargs):
    """echelonize_batch([A, ...]; kwargs...) -> [LU, ...] (spasm_amd_echelonize_batch): matrices with n * m <= 32768 are
    eliminated inside LDS, one workgroup each, all in a few launches; the others, and every matrix when L=True, take the path of
    echelonize one at a time.  The LDS path elects the canonical (leftmost) pivot columns whatever the pivot-search options say."""
    mats, opts, arr = _batch_args(mats, opts, kwargs)
    out = (C.POINTER(_abi.LuStruct) * max(len(mats), 1))()
    with _quiet(not verbose):
        rc = _abi.lib().spasm_amd_echelonize_batch(len(mats), arr, C.byref(opts.struct), out)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_echelonize_batch failed")
    return [LU(out[i]) for i in range(len(mats))]


def rank_batch(mats, opts=None, verbose=False, **kwargs):
    """rank_batch([A, ...]; kwargs...) -> [rank, ...] (spasm_amd_rank_batch): only the ranks leave the device."""
    mats, opts, arr = _batch_args(mats, opts, kwargs)
    out = (C.c_int64 * max(len(mats), 1))()
    with _quiet(not verbose):
        rc = _abi.lib().spasm_amd_rank_batch(len(mats), arr, C.byref(opts.struct), out)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_rank_batch failed")
    return [int(out[i]) for i in range(len(mats))]


def kernel_batch(mats, opts=None, verbose=False, **kwargs):
    """kernel_batch([A, ...]; kwargs...) -> [K, ...] (spasm_amd_kernel_batch): K[i] = kernel(echelonize_batch(...)[i]), its
    vectors in ascending order of their free column, without the LUs ever reaching the host."""
    mats, opts, arr = _batch_args(mats, opts, kwargs)
    out = (C.POINTER(_abi.CsrStruct) * max(len(mats), 1))()
    with _quiet(not verbose):
        rc = _abi.lib().spasm_amd_kernel_batch(len(mats), arr, C.byref(opts.struct), out)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_kernel_batch failed")
    return [CSR(out[i]) for i in range(len(mats))]


def batch_stats():
    """Counters of the last batch call of this thread (spasm_amd_batch_stats), as a dict keyed by BATCH_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_batch_stats(out)
    return {k: int(v) for k, v in zip(BATCH_STATS, out)}


# ---------------------------------------------------------------------------------------------
# A matrix split into its blocks on the device  (spasm_amd_blocks_*; csrc/blocks.hpp; engine extension)
# ---------------------------------------------------------------------------------------------
BLOCKS_INFO = ("blocks", "n", "m", "nnz", "largest_rows", "largest_cols", "largest_nnz", "blocks_without_entries", "components_us", "numbering_us", "split_us")


class DeviceBlocks:
    """The connected components of the row/column graph of A, found and split off on the device (spasm_amd_blocks_*).
    DeviceBlocks(A) takes a CSR (uploaded; it may be dropped afterwards) or a DeviceCSR (no upload).  The blocks stay on the device
    as one concatenated CSR in the batch's layout: rank(), echelonize(), kernel() give what rank_batch, echelonize_batch,
    kernel_batch give for the list of blocks, without the entries crossing the host.  to_block() builds the Block that
    Block.from_csr(A) builds; maps(), shapes(), fetch(b), info() read the handle.
    index=True (a square A): the index split (spasm_amd_blocks_create_index), where row i and column i are one vertex, so that A is
    block diagonal up to a SIMULTANEOUS permutation; only such a handle has charpoly() and charpoly_factors()."""

    def __init__(self, A, index=False):
        lib = _abi.lib()
        if isinstance(A, CSR):
            self._h = (lib.spasm_amd_blocks_create_index if index else lib.spasm_amd_blocks_create)(A.data)
        elif isinstance(A, DeviceCSR):
            self._h = (lib.spasm_amd_blocks_create_index_dcsr if index else lib.spasm_amd_blocks_create_dcsr)(A._need())
        else:
            raise TypeError("a CSR or a DeviceCSR expected")
        if not self._h:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_create failed")
        i = self.info()
        self._nb = i["blocks"]
        self.shape = (i["n"], i["m"])
        self.nnz = i["nnz"]
        self.prime = A.prime

    def _need(self):
        if not getattr(self, "_h", None):
            raise SpasmError("the blocks are closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _abi.lib().spasm_amd_blocks_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._nb

    @property
    def index(self):
        """True for the index split (spasm_amd_blocks_is_index)"""
        return _abi.lib().spasm_amd_blocks_is_index(self._need()) == 1

    def charpoly(self):
        """The n + 1 coefficients of det(x * I - A) mod p of the matrix behind an index handle (spasm_amd_blocks_charpoly): the
        product of the blocks' characteristic polynomials, formed on the device."""
        out = np.zeros(self.shape[0] + 1, dtype=np.int32)
        with _quiet(True):
            rc = _abi.lib().spasm_amd_blocks_charpoly(self._need(), out.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_charpoly failed")
        return out

    def charpoly_factors(self):
        """[characteristic polynomial of block b, ...] as int32 arrays of rows_b + 1 words (spasm_amd_blocks_charpoly_factors)"""
        n, nb = self.shape[0], self._nb
        out = np.zeros(max(n + nb, 1), dtype=np.int32)
        with _quiet(True):
            rc = _abi.lib().spasm_amd_blocks_charpoly_factors(self._need(), out.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_charpoly_factors failed")
        rows = self.shapes()[0].tolist()
        start = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
        return [out[int(start[b]) + b: int(start[b]) + b + rows[b] + 1].copy() for b in range(nb)]

    def info(self):
        out = (C.c_int64 * 11)()
        _abi.lib().spasm_amd_blocks_info(self._need(), out)
        return {k: int(v) for k, v in zip(BLOCKS_INFO, out)}

    def shapes(self):
        """(rows, cols, nnz): one int32 / int32 / int64 array entry per block"""
        nb = self._nb
        rows, cols, nz = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int64)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        if _abi.lib().spasm_amd_blocks_shapes(self._need(), rows.ctypes.data_as(i32), cols.ctypes.data_as(i32), nz.ctypes.data_as(i64)) != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_shapes failed")
        return rows[:nb], cols[:nb], nz[:nb]

    def maps(self):
        """dict of row_block, row_pos, col_block, col_pos, block_rows, row_start, block_cols, col_start (numpy arrays)"""
        (n, m), nb = self.shape, self._nb
        d = {
            "row_block": np.zeros(max(n, 1), dtype=np.int32), "row_pos": np.zeros(max(n, 1), dtype=np.int32),
            "col_block": np.zeros(max(m, 1), dtype=np.int32), "col_pos": np.zeros(max(m, 1), dtype=np.int32),
            "block_rows": np.zeros(max(n, 1), dtype=np.int32), "row_start": np.zeros(nb + 1, dtype=np.int64),
            "block_cols": np.zeros(max(m, 1), dtype=np.int32), "col_start": np.zeros(nb + 1, dtype=np.int64),
        }
        args = [d[k].ctypes.data_as(C.POINTER(C.c_int64 if d[k].dtype == np.int64 else C.c_int32)) for k in d]
        if _abi.lib().spasm_amd_blocks_maps(self._need(), *args) != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_maps failed")
        size = {"row_block": n, "row_pos": n, "block_rows": n, "col_block": m, "col_pos": m, "block_cols": m, "row_start": nb + 1, "col_start": nb + 1}
        return {k: v[: size[k]] for k, v in d.items()}

    def fetch(self, b):
        ptr = _abi.lib().spasm_amd_blocks_fetch(self._need(), int(b))
        if not ptr:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_fetch failed")
        return CSR(ptr)

    def block_maps(self):
        """(row2block, col2block, block2row, block2col) as a Block holds them"""
        mp = self.maps()
        row2block = list(zip(mp["row_block"].tolist(), mp["row_pos"].tolist()))
        col2block = list(zip(mp["col_block"].tolist(), mp["col_pos"].tolist()))
        rs, cs = mp["row_start"].tolist(), mp["col_start"].tolist()
        br, bc = mp["block_rows"].tolist(), mp["block_cols"].tolist()
        block2row = [br[rs[b]:rs[b + 1]] for b in range(self._nb)]
        block2col = [bc[cs[b]:cs[b + 1]] for b in range(self._nb)]
        return row2block, col2block, block2row, block2col

    def to_block(self):
        """The Block of Block.from_csr(A): the blocks as host matrices and the four maps."""
        from .blocks import Block

        return Block([self.fetch(b) for b in range(self._nb)], *self.block_maps())

    def _opts(self, opts, kwargs):
        if opts is None:
            opts = EchelonizeOpts()
        for k, v in kwargs.items():
            if not hasattr(opts.struct, k):
                raise AttributeError(f"type EchelonizeOpts has no field {k}")
            setattr(opts.struct, k, v)
        return opts

    def rank(self, opts=None, verbose=False, **kwargs):
        """[rank of block b, ...] (spasm_amd_blocks_rank): only the ranks leave the device."""
        opts = self._opts(opts, kwargs)
        out = (C.c_int64 * max(self._nb, 1))()
        with _quiet(not verbose):
            rc = _abi.lib().spasm_amd_blocks_rank(self._need(), C.byref(opts.struct), out)
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_rank failed")
        return [int(out[i]) for i in range(self._nb)]

    def echelonize(self, opts=None, verbose=False, **kwargs):
        """[LU of block b, ...] (spasm_amd_blocks_echelonize)"""
        opts = self._opts(opts, kwargs)
        out = (C.POINTER(_abi.LuStruct) * max(self._nb, 1))()
        with _quiet(not verbose):
            rc = _abi.lib().spasm_amd_blocks_echelonize(self._need(), C.byref(opts.struct), out)
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_echelonize failed")
        return [LU(out[i]) for i in range(self._nb)]

    def kernel(self, opts=None, verbose=False, **kwargs):
        """[kernel of block b, ...] (spasm_amd_blocks_kernel)"""
        opts = self._opts(opts, kwargs)
        out = (C.POINTER(_abi.CsrStruct) * max(self._nb, 1))()
        with _quiet(not verbose):
            rc = _abi.lib().spasm_amd_blocks_kernel(self._need(), C.byref(opts.struct), out)
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_kernel failed")
        return [CSR(out[i]) for i in range(self._nb)]

    def solve(self, B, verbose=False):
        """(X, ok) with X * A == B row by row for the matrix A this handle was split from (spasm_amd_blocks_solve): the columns of B
        are dealt to the blocks on the device, every block inside the LDS limit is solved from the resident blocks, and X comes back
        assembled.  Whenever A as a whole is inside the limit this is byte for byte what solve_batch([A], [B]) returns."""
        if not isinstance(B, CSR):
            raise TypeError("a CSR expected")
        if B.m != self.shape[1]:
            raise ValueError("B needs as many columns as the matrix of the handle")
        out = C.POINTER(_abi.CsrStruct)()
        ok = np.zeros(max(B.n, 1), dtype=np.uint8)
        with _quiet(not verbose):
            rc = _abi.lib().spasm_amd_blocks_solve(self._need(), B.data, C.byref(out), ok.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_blocks_solve failed")
        return CSR(out), ok[: B.n].astype(np.bool_)

    def solver(self):
        """A BatchSolver of all blocks (spasm_amd_solver_create_blocks): the blocks are factored once, from the device, and
        solver.solve(B) returns what solve(B) returns without eliminating them again.  It outlives this handle."""
        return BatchSolver.from_blocks(self)


# ---------------------------------------------------------------------------------------------
# X * A = B for many small matrices, and block by block  (spasm_amd_solve_batch / _blocks_solve; csrc/solve_batch.hpp)
# ---------------------------------------------------------------------------------------------
SOLVE_STATS = ("systems", "lds_path", "general_path", "jobs", "launches", "device_us", "entries", "unsolved")


def solve_batch(mats, rhs, verbose=False):
    """solve_batch([A, ...], [B, ...]) -> ([X, ...], [ok, ...]) (spasm_amd_solve_batch): X[i] * A[i] == B[i] row by row, ok[i] a
    np.bool_ array with one flag per row of B[i].  Systems with m * (n + 1) <= 32768 are solved inside LDS: X[i][k] is then the
    unique solution that is zero outside the canonical row basis of A[i] (the rows that are no combination of the rows before
    them), and an empty row where ok[i][k] is False.  The others go through echelonize(L=True) + gesv one at a time."""
    mats, rhs = list(mats), list(rhs)
    for M in mats + rhs:
        if not isinstance(M, CSR):
            raise TypeError("lists of CSR expected")
    if len(mats) != len(rhs):
        raise ValueError("as many right-hand sides as matrices expected")
    cnt = len(mats)
    arr = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))(*[A.data for A in mats])
    brr = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))(*[B.data for B in rhs])
    out = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))()
    oks = [np.zeros(max(B.n, 1), dtype=np.uint8) for B in rhs]
    okp = (C.POINTER(C.c_ubyte) * max(cnt, 1))(*[o.ctypes.data_as(C.POINTER(C.c_ubyte)) for o in oks])
    with _quiet(not verbose):
        rc = _abi.lib().spasm_amd_solve_batch(cnt, arr, brr, out, okp)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_solve_batch failed")
    return [CSR(out[i]) for i in range(cnt)], [o[: B.n].astype(np.bool_) for o, B in zip(oks, rhs)]


def solve_stats():
    """Counters of the last solve_batch / DeviceBlocks.solve call of this thread (spasm_amd_solve_stats), keyed by SOLVE_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_solve_stats(out)
    return {k: int(v) for k, v in zip(SOLVE_STATS, out)}


# ---------------------------------------------------------------------------------------------
# X * A = B with A factored once  (spasm_amd_solver_*; csrc/solver.hpp)
# ---------------------------------------------------------------------------------------------
SOLVER_INFO = ("systems", "lds_path", "general_path", "operator_words", "rank_sum", "factor_jobs", "create_launches", "create_us")
SOLVER_DENSE_INFO = ("rows", "cols", "ok_rows", "general_path", "plan_k", "plan_jobs", "plan_launches", "plans_built")


class BatchSolver:
    """The systems A[i] factored once and resident on the device for repeated solves X[i] * A[i] = B[i] (spasm_amd_solver_*; engine
    extension).  BatchSolver(mats) takes a list of CSR, which may be dropped afterwards; BatchSolver.from_blocks(device_blocks) (or
    DeviceBlocks.solver()) takes the blocks of a split matrix, and the DeviceBlocks may be closed afterwards.

    solve(rhs) -> (X, ok): for a solver made from a list, rhs is a list with one CSR per system and the result is what
    solve_batch(mats, rhs) returns, byte for byte on the LDS path; for one made from blocks, rhs is one CSR and the result is what
    DeviceBlocks.solve(rhs) returns.  One solve at a time per solver.

    solve_dense(B, X=None) -> (X, ok) (spasm_amd_solver_apply_dense / _dev): the right-hand sides are the COLUMNS of a dense B, the
    layout of SpMV.apply and TriangularSolver.solve.  A solver made from blocks stands for the matrix A that was split: B is
    m x k, X is n x k and ok has k flags.  A solver made from a list stands for diag(A[0], A[1], ...): system i owns the rows
    sum(m_j, j < i) ... of B and sum(n_j, j < i) ... of X, and ok has shape (count, k).  Column v of X is the dense image of what
    solve returns for that right-hand side, and zero where ok is False; B is left as it was.  B of shape (rows,) is one vector (X and
    ok lose the axis too).  int32 numpy arrays, or int32 torch tensors on the current device (enqueued on the current stream; ok
    is then a bool tensor, and nothing touches the host).  A solver with a system over the limit of the LDS path refuses."""

    def __init__(self, mats):
        mats = list(mats)
        for M in mats:
            if not isinstance(M, CSR):
                raise TypeError("a list of CSR expected")
        cnt = len(mats)
        arr = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))(*[A.data for A in mats])
        with _quiet(True):
            self._h = _abi.lib().spasm_amd_solver_create(cnt, arr)
        if not self._h:
            raise SpasmError(_abi.last_error() or "spasm_amd_solver_create failed")
        self._blocks = False
        self._count = cnt
        self.shapes = [A.shape for A in mats]
        self.primes = [A.prime for A in mats]

    @classmethod
    def from_blocks(cls, device_blocks):
        """The solver of all blocks of a DeviceBlocks, built from the blocks on the device"""
        if not isinstance(device_blocks, DeviceBlocks):
            raise TypeError("a DeviceBlocks expected")
        self = cls.__new__(cls)
        with _quiet(True):
            self._h = _abi.lib().spasm_amd_solver_create_blocks(device_blocks._need())
        if not self._h:
            raise SpasmError(_abi.last_error() or "spasm_amd_solver_create_blocks failed")
        self._blocks = True
        self._count = len(device_blocks)
        self.shape = device_blocks.shape
        self.prime = device_blocks.prime
        return self

    def _need(self):
        if not getattr(self, "_h", None):
            raise SpasmError("the solver is closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _abi.lib().spasm_amd_solver_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._count

    def info(self):
        out = (C.c_int64 * 8)()
        _abi.lib().spasm_amd_solver_info(self._need(), out)
        return {k: int(v) for k, v in zip(SOLVER_INFO, out)}

    @property
    def ranks(self):
        """[rank of system i, ...]"""
        out = (C.c_int64 * max(self._count, 1))()
        if _abi.lib().spasm_amd_solver_ranks(self._need(), out) != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_solver_ranks failed")
        return [int(out[i]) for i in range(self._count)]

    def basis(self, i):
        """The rows of system i its solutions live on, ascending (int32 array): the canonical row basis on the LDS path, the
        factorization's pivotal rows on the general path."""
        i = int(i)
        if not 0 <= i < self._count:
            raise IndexError("system index out of range")
        h = self._need()
        n = self.shape[0] if self._blocks else self.shapes[i][0]
        rows = np.zeros(max(n, 1), dtype=np.int32)
        r = _abi.lib().spasm_amd_solver_basis(h, i, rows.ctypes.data_as(C.POINTER(C.c_int32)))
        if r < 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_solver_basis failed")
        return rows[:r].copy()

    def solve(self, rhs, verbose=False):
        h = self._need()
        if self._blocks:
            if not isinstance(rhs, CSR):
                raise TypeError("a CSR expected")
            out = C.POINTER(_abi.CsrStruct)()
            ok = np.zeros(max(rhs.n, 1), dtype=np.uint8)
            with _quiet(not verbose):
                rc = _abi.lib().spasm_amd_solver_apply_blocks(h, rhs.data, C.byref(out), ok.ctypes.data_as(C.POINTER(C.c_ubyte)))
            if rc != 0:
                raise SpasmError(_abi.last_error() or "spasm_amd_solver_apply_blocks failed")
            return CSR(out), ok[: rhs.n].astype(np.bool_)
        rhs = list(rhs)
        for M in rhs:
            if not isinstance(M, CSR):
                raise TypeError("a list of CSR expected")
        if len(rhs) != self._count:
            raise ValueError("as many right-hand sides as systems expected")
        cnt = self._count
        brr = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))(*[B.data for B in rhs])
        out = (C.POINTER(_abi.CsrStruct) * max(cnt, 1))()
        oks = [np.zeros(max(B.n, 1), dtype=np.uint8) for B in rhs]
        okp = (C.POINTER(C.c_ubyte) * max(cnt, 1))(*[o.ctypes.data_as(C.POINTER(C.c_ubyte)) for o in oks])
        with _quiet(not verbose):
            rc = _abi.lib().spasm_amd_solver_apply(h, brr, out, okp)
        if rc != 0:
            raise SpasmError(_abi.last_error() or "spasm_amd_solver_apply failed")
        return [CSR(out[i]) for i in range(cnt)], [o[: B.n].astype(np.bool_) for o, B in zip(oks, rhs)]

    def dense_info(self):
        """The shape solve_dense works on and its cached plan (spasm_amd_solver_dense_info), keyed by SOLVER_DENSE_INFO."""
        out = (C.c_int64 * 8)()
        _abi.lib().spasm_amd_solver_dense_info(self._need(), out)
        return {k: int(v) for k, v in zip(SOLVER_DENSE_INFO, out)}

    def _dense_shape(self):
        if self._blocks:
            return self.shape[0], self.shape[1], 1
        return sum(n for n, _ in self.shapes), sum(m for _, m in self.shapes), self._count

    def solve_dense(self, B, X=None):
        h = self._need()
        n, m, okrows = self._dense_shape()
        if type(B).__module__.startswith("torch"):
            return self._solve_dense_torch(h, B, X, n, m, okrows)
        if not isinstance(B, np.ndarray) or B.dtype != np.int32:
            raise TypeError("B must be an int32 numpy array or torch tensor")
        if B.ndim not in (1, 2) or B.shape[0] != m:
            raise ValueError(f"B must have shape ({m},) or ({m}, k), not {B.shape}")
        k = 1 if B.ndim == 1 else B.shape[1]
        if X is None:
            X = np.zeros((n,) + B.shape[1:], dtype=np.int32)
        if not isinstance(X, np.ndarray) or X.dtype != np.int32:
            raise TypeError("X must be an int32 numpy array")
        if X.shape != (n,) + B.shape[1:]:
            raise ValueError(f"X must have shape {(n,) + B.shape[1:]}, not {X.shape}")
        if not X.flags["WRITEABLE"]:
            raise ValueError("X must be writable")
        Bc = _rows_view(B, "B") if B.size else B   # (an array without elements has no strides to speak of)
        Xc = _rows_view(X, "X") if X.size else X
        if n > 0 and m > 0 and k > 0 and np.shares_memory(Bc, Xc):
            raise ValueError("B and X must not overlap")
        ldb = k if B.ndim == 1 else max(Bc.strides[0] // 4, k)
        ldx = k if X.ndim == 1 else max(Xc.strides[0] // 4, k)
        ok = np.ones(max(okrows * k, 1), dtype=np.uint8)
        rc = _abi.lib().spasm_amd_solver_apply_dense(h, int(k), Bc.ctypes.data, ldb, Xc.ctypes.data, ldx, ok.ctypes.data)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        ok = ok[: okrows * k].astype(bool)
        ok = ok if self._blocks else ok.reshape(okrows, k)
        return X, (ok[..., 0] if B.ndim == 1 else ok)

    def _solve_dense_torch(self, h, B, X, n, m, okrows):
        import torch

        if B.dtype != torch.int32 or B.device.type != "cuda" or B.device.index != torch.cuda.current_device():
            raise TypeError("B must be an int32 tensor on the current device")
        if B.dim() not in (1, 2) or B.shape[0] != m:
            raise ValueError(f"B must have shape ({m},) or ({m}, k), not {tuple(B.shape)}")
        k = 1 if B.dim() == 1 else B.shape[1]
        if X is None:
            X = torch.zeros((n,) + tuple(B.shape[1:]), dtype=torch.int32, device=B.device)
        if X.dtype != torch.int32 or X.device != B.device:
            raise TypeError("X must be an int32 tensor on the device of B")
        if tuple(X.shape) != (n,) + tuple(B.shape[1:]):
            raise ValueError(f"X must have shape {(n,) + tuple(B.shape[1:])}, not {tuple(X.shape)}")
        for t, name in ((B, "B"), (X, "X")):
            if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < k):
                raise ValueError(f"{name} must have unit stride along its rows")
        ldb = k if B.dim() == 1 else max(B.stride(0), k)
        ldx = k if X.dim() == 1 else max(X.stride(0), k)
        if n > 0 and m > 0 and k > 0 and _windows_overlap(B.data_ptr(), m, ldb, X.data_ptr(), n, ldx, k):
            raise ValueError("B and X must not overlap")
        ok = torch.ones(max(okrows * k, 1), dtype=torch.uint8, device=B.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = _abi.lib().spasm_amd_solver_apply_dense_dev(h, int(k), C.c_void_p(B.data_ptr()), ldb, C.c_void_p(X.data_ptr()), ldx,
                                                         C.c_void_p(ok.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        ok = ok[: okrows * k].bool()
        ok = ok if self._blocks else ok.reshape(okrows, k)
        return X, (ok[..., 0] if B.dim() == 1 else ok)


def _windows_overlap(b0, m, ldb, x0, n, ldx, k):
    """Do the windows of m rows at b0 and n rows at x0 (k int32 words a row, ldb and ldx words apart) share a byte?  Row by row, as
    the engine tests it: two windows side by side in one array interleave without sharing a word."""
    length, rowb, rowx = 4 * k, 4 * ldb, 4 * ldx
    if not (b0 < x0 + (n - 1) * rowx + length and x0 < b0 + (m - 1) * rowb + length):
        return False
    d = (b0 - x0) + rowb * np.arange(m, dtype=np.int64)    # row j of X meets a row of B iff |d - j * rowx| < length
    lo = np.maximum((d - length) // rowx + 1, 0)
    hi = np.minimum(-((-(d + length)) // rowx) - 1, n - 1)
    return bool((lo <= hi).any())


def solver_stats():
    """Counters of the last BatchSolver.solve call of this thread (spasm_amd_solver_stats), keyed by SOLVE_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_solver_stats(out)
    return {k: int(v) for k, v in zip(SOLVE_STATS, out)}


def last_rounds(max_rounds=4096):
    """Per-round records of the most recent echelonize call on this thread (engine extension)."""
    buf = (_abi.RoundStats * max_rounds)()
    n = _abi.lib().spasm_amd_last_rounds(buf, max_rounds)
    return [buf[i].as_dict() for i in range(min(n, max_rounds))]


DENSE_STATS = ("eliminations", "kind", "rows", "cols", "block", "tall_finishes", "panels_redone", "spare")
DENSE_KINDS = {0: None, 1: "i8_one_digit", 2: "i8_two_digits", 3: "f64_panels", 4: "rank1_updates"}


def dense_stats():
    """Counters of the dense eliminations of the last echelonize call of this thread (spasm_amd_dense_stats), keyed by DENSE_STATS;
    `kind` (of the last elimination) is one of DENSE_KINDS' names, None when the call reached no dense finish."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_dense_stats(out)
    d = {k: int(v) for k, v in zip(DENSE_STATS, out)}
    d["kind"] = DENSE_KINDS[d["kind"]]
    return d


# The engine's progress text goes to stderr / logcallback like libspasm's; the reference hides it
# by redirecting the process's stderr around the ccall unless verbose (src/SpaSM.jl:838-858).
_LOGFUNC = C.CFUNCTYPE(C.c_int, C.c_char_p)
_swallow = _LOGFUNC(lambda s: 0)


class _quiet:
    def __init__(self, active):
        self.active = active

    def __enter__(self):
        if self.active:
            self.slot = C.c_void_p.in_dll(_abi.lib(), "logcallback")
            self.prev = self.slot.value
            self.slot.value = C.cast(_swallow, C.c_void_p).value

    def __exit__(self, *exc):
        if self.active:
            self.slot.value = self.prev
        return False


def synth_csr(kind, n, m, density=0.0, row_nnz=0, prime=prime0, seed=0):
    """Deterministic synthetic CSR: kind 0 = Bernoulli(density), kind 1 = row_nnz per row."""
    ptr = _abi.lib().spasm_amd_synth_csr(int(kind), int(n), int(m), float(density), int(row_nnz), int(prime), int(seed))
    if not ptr:
        raise SpasmError("spasm_amd_synth_csr failed: " + _abi.last_error())
    return CSR(ptr)


# ---------------------------------------------------------------------------------------------
# Triplets and the SMS wire format  (reference src/SpaSM.jl:234-260, :482-529, :1025-1086)
# ---------------------------------------------------------------------------------------------
_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


class Triplet:
    """Spasm matrix in coordinate format; `push` then `compress` (reference src/SpaSM.jl:244-251, :482-493)."""

    def __init__(self, n=0, m=0, nzmax=16, prime=prime0, ptr=None):
        self.data = ptr if ptr is not None else _abi.lib().spasm_triplet_alloc(int(n), int(m), int(nzmax), int(prime), True)
        if not self.data:
            raise SpasmError("spasm_triplet_alloc failed: " + _abi.last_error())

    def __del__(self):
        if getattr(self, "data", None):
            try:
                _abi.lib().spasm_triplet_free(self.data)
            except Exception:
                pass
            self.data = None

    def push(self, i, j, x):
        """push!(A, (i, j, x)) with 1-based indices (reference src/SpaSM.jl:482-488)."""
        assert 1 <= i and 1 <= j
        _abi.lib().spasm_add_entry(self.data, int(i) - 1, int(j) - 1, int(x))
        return self

    def transpose_(self):
        _abi.lib().spasm_triplet_transpose(self.data)
        return self

    @property
    def nz(self):
        return int(self.data.contents.nz)

    @property
    def shape(self):
        return (int(self.data.contents.n), int(self.data.contents.m))

    def compress(self):
        ptr = _abi.lib().spasm_compress(self.data)
        if not ptr:
            raise SpasmError("spasm_compress failed: " + _abi.last_error())
        return CSR(ptr)


def load(path, prime=prime0, csr=True, get_hash=False):
    """load(File{format"SMS"}(path); prime, csr) (reference src/SpaSM.jl:498-512): Triplet, or CSR when csr=True."""
    f = _libc.fopen(str(path).encode(), b"r")
    if not f:
        raise OSError(f"cannot open {path}")
    try:
        digest = (C.c_uint8 * 32)() if get_hash else None
        ptr = _abi.lib().spasm_triplet_load(f, int(prime), digest)
    finally:
        _libc.fclose(f)
    if not ptr:
        raise SpasmError("spasm_triplet_load failed: " + _abi.last_error())
    T = Triplet(ptr=ptr)
    out = T.compress() if csr else T
    return (out, bytes(digest)) if get_hash else out


def save(path, A):
    """save(File{format"SMS"}(path), A) for a CSR or a Triplet (reference src/SpaSM.jl:514-529)."""
    f = _libc.fopen(str(path).encode(), b"w")
    if not f:
        raise OSError(f"cannot open {path}")
    try:
        if isinstance(A, Triplet):
            _abi.lib().spasm_triplet_save(A.data, f)
        else:
            _abi.lib().spasm_csr_save(A.data, f)
    finally:
        _libc.fclose(f)


# ---------------------------------------------------------------------------------------------
# Rank certificates  (reference src/SpaSM.jl:345-353, :928-933)
# ---------------------------------------------------------------------------------------------
class RankCertificate:
    """RankCertificate{F}: r rows i and r columns j of A whose submatrix is shown non-singular by y * A[i, j] == x for the
    challenge x drawn from (hash, prime, r, i, j) -- a proof that rank(A) >= r (include/spasm_amd.h)."""

    def __init__(self, ptr, own=True):
        assert ptr
        self.data = ptr
        self._own = own

    def __del__(self):
        if getattr(self, "data", None) and self._own:
            try:
                _abi.lib().spasm_rank_certificate_free(self.data)
            except Exception:
                pass
            self.data = None

    r = property(lambda s: int(s.data.contents.r))
    prime = property(lambda s: int(s.data.contents.prime))
    hash = property(lambda s: bytes(s.data.contents.hash))

    def _arr(self, name):
        r = self.r
        return np.ctypeslib.as_array(getattr(self.data.contents, name), (max(r, 1),))[:r]

    i = property(lambda s: s._arr("i"))
    j = property(lambda s: s._arr("j"))
    x = property(lambda s: s._arr("x"))
    y = property(lambda s: s._arr("y"))


def _hash_arg(h):
    h = bytes(h)
    assert len(h) == 32, "the hash is the 32-byte SHA-256 digest load(..., get_hash=True) returns"
    return (C.c_uint8 * 32).from_buffer_copy(h)


def certificate_rank_create(A, hash, fact):
    """certificate_rank_create(A, hash, fact) (reference src/SpaSM.jl:928)."""
    ptr = _abi.lib().spasm_certificate_rank_create(A.data, _hash_arg(hash), fact.data)
    if not ptr:
        raise SpasmError("spasm_certificate_rank_create failed: " + _abi.last_error())
    return RankCertificate(ptr)


def certificate_rank_verify(A, hash, proof):
    """certificate_rank_verify(A, hash, proof) -> Bool (reference src/SpaSM.jl:930): host-side, O(nnz(A))."""
    return bool(_abi.lib().spasm_certificate_rank_verify(A.data, _hash_arg(hash), proof.data))


def rank_certificate_save(proof, path):
    """rank_certificate_save(proof, file) (reference src/SpaSM.jl:931)."""
    f = _libc.fopen(str(path).encode(), b"w")
    if not f:
        raise OSError(f"cannot open {path}")
    try:
        _abi.lib().spasm_rank_certificate_save(proof.data, f)
    finally:
        _libc.fclose(f)


def rank_certificate_load(path):
    """rank_certificate_load(file, proof) (reference src/SpaSM.jl:933): a RankCertificate, or None when the file does not parse."""
    f = _libc.fopen(str(path).encode(), b"r")
    if not f:
        raise OSError(f"cannot open {path}")
    libc = C.CDLL(None)
    libc.calloc.restype = C.c_void_p
    libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
    mem = libc.calloc(1, C.sizeof(_abi.RankCertificateStruct))
    ptr = C.cast(mem, C.POINTER(_abi.RankCertificateStruct))
    try:
        ok = _abi.lib().spasm_rank_certificate_load(f, ptr)
    finally:
        _libc.fclose(f)
    if not ok:
        _abi.lib().spasm_rank_certificate_free(ptr)
        return None
    return RankCertificate(ptr)


# ---------------------------------------------------------------------------------------------
# Determinants mod p  (spasm_amd_det*; csrc/det.hpp; engine extension)
# ---------------------------------------------------------------------------------------------
DET_STATS = ("items", "lds_path", "general_path", "zero_by_structure", "launches", "device_us", "host_parity_us", "spare")


def det_batch(mats):
    """det_batch([A, ...]) -> numpy int64 array of the determinants mod p as balanced residues (spasm_amd_det_batch): square
    matrices with n * n <= 32768 are eliminated inside LDS, one workgroup each, and one int per matrix comes back; the others
    take the path of echelonize with L one at a time.  The matrices may differ in size and in prime."""
    mats = list(mats)
    for A in mats:
        if not isinstance(A, CSR):
            raise TypeError("a list of CSR expected")
    arr = (C.POINTER(_abi.CsrStruct) * max(len(mats), 1))(*[A.data for A in mats])
    out = (C.c_int32 * max(len(mats), 1))()
    with _quiet(True):
        rc = _abi.lib().spasm_amd_det_batch(len(mats), arr, out)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_det_batch failed")
    return np.array(out[: len(mats)], dtype=np.int64)


def det(A):
    """det(A) -> int, the determinant mod p as a balanced residue.  A CSR (spasm_amd_det) or a DeviceCSR (spasm_amd_dcsr_det) is
    split into its blocks on the device first; a DeviceBlocks (spasm_amd_blocks_det) is split already.  The value is the product
    of the blocks' determinants times the parities of the two permutations that bring A to block-diagonal form; 0 without any
    elimination when a block is not square."""
    lib = _abi.lib()
    out = C.c_int32(0)
    with _quiet(True):
        if isinstance(A, CSR):
            who, rc = "spasm_amd_det", lib.spasm_amd_det(A.data, C.byref(out))
        elif isinstance(A, DeviceCSR):
            who, rc = "spasm_amd_dcsr_det", lib.spasm_amd_dcsr_det(A._need(), C.byref(out))
        elif isinstance(A, DeviceBlocks):
            who, rc = "spasm_amd_blocks_det", lib.spasm_amd_blocks_det(A._need(), C.byref(out))
        else:
            raise TypeError("a CSR, a DeviceCSR or a DeviceBlocks expected")
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return int(out.value)


def det_stats():
    """Counters of the last det call of this thread (spasm_amd_det_stats), as a dict keyed by DET_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_det_stats(out)
    return {k: int(v) for k, v in zip(DET_STATS, out)}


DeviceCSR.det = det
DeviceBlocks.det = det


# ---------------------------------------------------------------------------------------------
# Characteristic polynomials mod p  (spasm_amd_charpoly*; csrc/charpoly.hpp; engine extension)
# ---------------------------------------------------------------------------------------------
CHARPOLY_STATS = ("items", "lds_path", "global_path", "launches", "lds_device_us", "global_device_us", "spare0", "spare1")


def charpoly_batch(mats):
    """charpoly_batch([A, ...]) -> list of numpy int32 arrays: the n + 1 coefficients of det(x * I - A) mod p as balanced residues,
    low degree first, the last one 1 (spasm_amd_charpoly_batch).  Square matrices with n * n <= 32768 are reduced to Hessenberg form
    inside LDS, one workgroup each; larger ones (n <= 1024) by one workgroup on an image in device memory.  The matrices may differ
    in size and in prime."""
    mats = list(mats)
    for A in mats:
        if not isinstance(A, CSR):
            raise TypeError("a list of CSR expected")
    arr = (C.POINTER(_abi.CsrStruct) * max(len(mats), 1))(*[A.data for A in mats])
    # (a matrix the entry will refuse still gets a slot, so that the refusal is the entry's)
    outs = [np.zeros(max(A.n, 0) + 1, dtype=np.int32) for A in mats]
    ptrs = (C.POINTER(C.c_int32) * max(len(mats), 1))(*[o.ctypes.data_as(C.POINTER(C.c_int32)) for o in outs])
    with _quiet(True):
        rc = _abi.lib().spasm_amd_charpoly_batch(len(mats), arr, ptrs)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_charpoly_batch failed")
    return outs


def charpoly(A, split=False):
    """charpoly(A) -> numpy int32 array of the n + 1 coefficients of det(x * I - A) mod p as balanced residues, low degree first.
    A CSR (spasm_amd_charpoly) or a DeviceCSR (spasm_amd_dcsr_charpoly: on its device, no entry crosses the host).
    split=True: A is split by the components of its index graph first and the blocks' polynomials are multiplied on the device
    (spasm_amd_charpoly_split / _dcsr_charpoly_split): no limit on n, only on the rows of a block (1024)."""
    lib = _abi.lib()
    if split:
        if isinstance(A, CSR):
            who, fn, arg, n = "spasm_amd_charpoly_split", lib.spasm_amd_charpoly_split, A.data, A.n
        elif isinstance(A, DeviceCSR):
            who, fn, arg, n = "spasm_amd_dcsr_charpoly_split", lib.spasm_amd_dcsr_charpoly_split, A._need(), A.shape[0]
        else:
            raise TypeError("a CSR or a DeviceCSR expected")
        out = np.zeros(max(n, 0) + 1, dtype=np.int32)
        with _quiet(True):
            rc = fn(arg, out.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise SpasmError(_abi.last_error() or f"{who} failed")
        return out
    if isinstance(A, CSR):
        n = A.n
    elif isinstance(A, DeviceCSR):
        A._need()
        n = A.shape[0]
    else:
        raise TypeError("a CSR or a DeviceCSR expected")
    out = np.zeros(max(n, 0) + 1, dtype=np.int32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_int32))
    with _quiet(True):
        if isinstance(A, CSR):
            who, rc = "spasm_amd_charpoly", lib.spasm_amd_charpoly(A.data, ptr)
        else:
            who, rc = "spasm_amd_dcsr_charpoly", lib.spasm_amd_dcsr_charpoly(A._need(), ptr)
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return out


def charpoly_stats():
    """Counters of the last charpoly call of this thread (spasm_amd_charpoly_stats), as a dict keyed by CHARPOLY_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_charpoly_stats(out)
    return {k: int(v) for k, v in zip(CHARPOLY_STATS, out)}


DeviceCSR.charpoly = charpoly


# ---------------------------------------------------------------------------------------------
# Characteristic polynomials by components  (spasm_amd_poly_product, _charpoly_split*; csrc/polyprod.hpp; engine extension)
# ---------------------------------------------------------------------------------------------
CHARPOLY_SPLIT_STATS = ("blocks", "lds_path", "global_path", "launches", "charpoly_device_us", "product_levels", "product_device_us", "spare")


def poly_product(polys, prime):
    """poly_product([f, ...], prime) -> numpy int32 array: the product of the polynomials mod prime as balanced residues, low
    degree first (spasm_amd_poly_product: a product tree on the device).  Every f is a non-empty sequence of integers that fit
    int32; [] gives [1]."""
    polys = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1) for f in polys]
    count = len(polys)
    lens = (C.c_int32 * max(count, 1))(*[len(f) for f in polys])
    ptrs = (C.POINTER(C.c_int32) * max(count, 1))(*[f.ctypes.data_as(C.POINTER(C.c_int32)) for f in polys])
    out = np.zeros(max(sum(len(f) for f in polys) - count + 1, 1), dtype=np.int32)
    with _quiet(True):
        rc = _abi.lib().spasm_amd_poly_product(count, lens, ptrs, int(prime), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_poly_product failed")
    return out


def charpoly_split_stats():
    """Counters of the last split charpoly call of this thread (spasm_amd_charpoly_split_stats), keyed by CHARPOLY_SPLIT_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_charpoly_split_stats(out)
    return {k: int(v) for k, v in zip(CHARPOLY_SPLIT_STATS, out)}


# ---------------------------------------------------------------------------------------------
# Minimal polynomials by Wiedemann's method  (spasm_amd_krylov_sequence, _berlekamp_massey, _poly_lcm, _minpoly*; csrc/krylov.hpp)
# ---------------------------------------------------------------------------------------------
MINPOLY_STATS = ("n", "K", "steps", "launches", "bm_class", "degree", "sequence_device_us", "bm_device_us")


def krylov_sequence(op, U, V, length, trans=False):
    """krylov_sequence(op, U, V, length, trans=False) -> S of shape (length, K): S[i, c] = sum_r U[r, c] * (A^i V)[r, c] mod p as
    balanced residues, A the square matrix of the SpMV operator op (A^T with trans=True).  U and V are n x K (or n entries: K = 1),
    1 <= K <= 64, int32 numpy arrays (spasm_amd_krylov_sequence) or int32 torch tensors on the current device (enqueued on the
    current stream without a host synchronization; S is a tensor: spasm_amd_krylov_sequence_dev).  U and V are not modified."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n = op.shape[0]
    length = int(length)
    if length < 0:
        raise ValueError("length must not be negative")
    lib = _abi.lib()
    if type(U).__module__.startswith("torch") or type(V).__module__.startswith("torch"):
        import torch

        for t, name in ((U, "U"), (V, "V")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device.type != "cuda" or t.device.index != torch.cuda.current_device():
                raise TypeError(f"{name} must be an int32 tensor on the current device")
            if t.dim() not in (1, 2) or t.shape[0] != n or tuple(t.shape) != tuple(U.shape):
                raise ValueError(f"U and V must both have shape ({n},) or ({n}, K), not {tuple(t.shape)}")
        k = 1 if U.dim() == 1 else int(U.shape[1])
        for t, name in ((U, "U"), (V, "V")):
            if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < k):
                raise ValueError(f"{name} must have unit stride along its rows")
        ldu = k if U.dim() == 1 else max(U.stride(0), k)
        ldv = k if V.dim() == 1 else max(V.stride(0), k)
        S = torch.empty((length, k), dtype=torch.int32, device=U.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.spasm_amd_krylov_sequence_dev(op._op, int(bool(trans)), k, length, C.c_void_p(U.data_ptr()), ldu, C.c_void_p(V.data_ptr()), ldv,
                                               C.c_void_p(S.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return S
    for a, name in ((U, "U"), (V, "V")):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise TypeError(f"{name} must be an int32 numpy array or torch tensor")
        if a.ndim not in (1, 2) or a.shape[0] != n or a.shape != U.shape:
            raise ValueError(f"U and V must both have shape ({n},) or ({n}, K), not {a.shape}")
    k = 1 if U.ndim == 1 else U.shape[1]
    Uc, Vc = _rows_view(U, "U"), _rows_view(V, "V")
    ldu = k if U.ndim == 1 else max(Uc.strides[0] // 4, k)
    ldv = k if V.ndim == 1 else max(Vc.strides[0] // 4, k)
    S = np.zeros((length, k), dtype=np.int32)
    rc = lib.spasm_amd_krylov_sequence(op._op, int(bool(trans)), int(k), length, Uc.ctypes.data, ldu, Vc.ctypes.data, ldv, S.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error())
    return S


def berlekamp_massey(S, prime, where=0):
    """berlekamp_massey(S, prime, where=0) -> list of numpy int32 arrays, one per column of S (len x count; a 1-d S is one
    sequence): the monic polynomial of the shortest linear recurrence of the column, low degree first, as balanced residues
    (spasm_amd_berlekamp_massey: one workgroup per sequence; where = 1 forces the LDS class, 2 the device-memory class).  The
    zero sequence gives [1]; 1, 0, 0, 0 gives x."""
    S = np.asarray(S)
    if S.dtype.kind not in "iu":
        raise TypeError("integer entries expected")
    one = S.ndim == 1
    if one:
        S = S[:, None]
    if S.ndim != 2:
        raise ValueError("a sequence or a len x count array expected")
    S = np.ascontiguousarray(balanced(S, int(prime)))
    length, count = S.shape
    ldc = length + 1
    coef = np.zeros((max(count, 1), ldc), dtype=np.int32)
    deg = np.zeros(max(count, 1), dtype=np.int32)
    rc = _abi.lib().spasm_amd_berlekamp_massey(count, length, S.ctypes.data, count, int(prime), int(where),
                                               coef.ctypes.data, ldc, deg.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_berlekamp_massey failed")
    out = [coef[c, : deg[c] + 1].copy() for c in range(count)]
    return out[0] if one else out


def poly_lcm(polys, prime):
    """poly_lcm([f, ...], prime) -> numpy int32 array: the monic lcm of the polynomials mod prime as balanced residues, low degree
    first (spasm_amd_poly_lcm: Euclid on the host, exact, no device).  Every f is a non-empty sequence of integers that fit int32
    and is not the zero polynomial; [] gives [1]."""
    polys = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1) for f in polys]
    count = len(polys)
    lens = (C.c_int32 * max(count, 1))(*[len(f) for f in polys])
    ptrs = (C.POINTER(C.c_int32) * max(count, 1))(*[f.ctypes.data_as(C.POINTER(C.c_int32)) for f in polys])
    out = np.zeros(max(sum(len(f) for f in polys) - count + 1, 1), dtype=np.int32)
    outlen = C.c_int32(0)
    rc = _abi.lib().spasm_amd_poly_lcm(count, lens, ptrs, int(prime), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(outlen))
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_poly_lcm failed")
    return out[: outlen.value].copy()


def minpoly_vectors(n, K, seed, prime):
    """(U, V): the n x K int32 arrays minpoly uses for this seed when none are given (spasm_amd_minpoly_vectors)."""
    U = np.zeros((n, K), dtype=np.int32)
    V = np.zeros((n, K), dtype=np.int32)
    rc = _abi.lib().spasm_amd_minpoly_vectors(int(n), int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(prime), U.ctypes.data, V.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_minpoly_vectors failed")
    return U, V


def _family_target(A, stem):
    """(who, function, handle, rows) of the entry point of `stem` for a CSR, an SpMV or a DeviceCSR"""
    if isinstance(A, CSR):
        who, arg, n = f"spasm_amd_{stem}", A.data, A.n
    elif isinstance(A, SpMV):
        if not A._op:
            raise SpasmError("the operator is closed")
        who, arg, n = f"spasm_amd_spmv_{stem}", A._op, A.shape[0]
    elif isinstance(A, DeviceCSR):
        who, arg, n = f"spasm_amd_dcsr_{stem}", A._need(), A.shape[0]
    else:
        raise TypeError("a CSR, an SpMV or a DeviceCSR expected")
    return who, getattr(_abi.lib(), who), arg, n


def minpoly(A, K=8, seed=0, maxdeg=None, U=None, V=None):
    """minpoly(A, K=8, seed=0, maxdeg=None, U=None, V=None) -> numpy int32 array: the lcm of the minimal polynomials of K
    projections u^T A^i v of the Krylov sequence of the square matrix A, monic, low degree first, balanced residues.  A is a CSR
    (spasm_amd_minpoly), an SpMV operator (spasm_amd_spmv_minpoly) or a DeviceCSR (spasm_amd_dcsr_minpoly: on its device).  U and V
    are n x K int32 arrays, or both None: minpoly_vectors(n, K, seed, prime).  maxdeg bounds the degree (None: n); a matrix whose
    polynomial has a larger degree is refused ("degree bound too small").
    The result always divides the minimal polynomial of A and equals it with a probability that grows with p and K.  If its
    constant term is 0, A is singular (certain).  If its degree is n, it is the characteristic polynomial."""
    who, fn, arg, n = _family_target(A, "minpoly")
    K = int(K)
    kk = 8 if K == 0 else K
    ptrs = []
    for a, name in ((U, "U"), (V, "V")):
        if a is None:
            ptrs.append(None)
            continue
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != (n, kk) or not a.flags["C_CONTIGUOUS"]:
            raise TypeError(f"{name} must be a contiguous int32 numpy array of shape ({n}, {kk})")
        ptrs.append(a.ctypes.data)
    md = 0 if maxdeg is None else int(maxdeg)
    out = np.zeros((md if 0 < md <= n else max(n, 0)) + 1, dtype=np.int32)
    deg = C.c_int32(0)
    with _quiet(True):
        rc = fn(arg, K, int(seed) & 0xFFFFFFFFFFFFFFFF, md, ptrs[0], ptrs[1], out.ctypes.data, C.byref(deg))
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return out[: deg.value + 1].copy()


def minpoly_stats():
    """Counters of the last Krylov / Berlekamp-Massey / minpoly call of this thread (spasm_amd_minpoly_stats), keyed by
    MINPOLY_STATS."""
    out = (C.c_int64 * 8)()
    _abi.lib().spasm_amd_minpoly_stats(out)
    return {k: int(v) for k, v in zip(MINPOLY_STATS, out)}


SpMV.krylov_sequence = krylov_sequence
SpMV.minpoly = minpoly
DeviceCSR.minpoly = minpoly


# ---------------------------------------------------------------------------------------------
# Polynomials of A applied to vectors, and Wiedemann's solve  (spasm_amd_poly_apply*, _wiedemann_solve*; csrc/horner.hpp)
# ---------------------------------------------------------------------------------------------
WIEDEMANN_STATS = ("n", "K", "tries", "products", "launches", "degree", "solved", "kernel_vectors", "sequence_device_us", "horner_device_us")


def _poly_table(polys, k):
    """(deg, coef, ldc) of k polynomials given low degree first; an empty one is the zero polynomial"""
    polys = [np.asarray(f).reshape(-1) for f in polys]
    if len(polys) != k:
        raise ValueError(f"{k} polynomials expected, one per column, not {len(polys)}")
    for f in polys:
        if f.size and (f.dtype.kind not in "iu" or f.min() < -2**31 or f.max() > 2**31 - 1):
            raise TypeError("the coefficients must be integers that fit int32")
    ldc = max([f.size for f in polys] + [1])
    coef = np.zeros((k, ldc), dtype=np.int32)
    for c, f in enumerate(polys):
        coef[c, : f.size] = f
    deg = np.array([f.size - 1 for f in polys], dtype=np.int32)
    return deg, coef, ldc


def poly_apply(op, polys, V, trans=False):
    """poly_apply(op, polys, V, trans=False) -> X with X[:, c] = f_c(A) V[:, c] mod p as balanced residues, A the square matrix of
    the SpMV operator op (A^T with trans=True) and f_c = polys[c], low degree first (any int32; [] is the zero polynomial).  V is
    n x K, 1 <= K <= 64, or n entries with polys one polynomial.  int32 numpy arrays (spasm_amd_poly_apply) or int32 torch tensors
    on the current device (enqueued on the current stream without a host synchronization; X is a tensor:
    spasm_amd_poly_apply_dev).  Horner's rule: max(deg) products with A.  V is not modified."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n = op.shape[0]
    is_torch = type(V).__module__.startswith("torch")
    ndim = V.dim() if is_torch else getattr(V, "ndim", 0)
    if ndim not in (1, 2) or V.shape[0] != n:
        raise ValueError(f"V must have shape ({n},) or ({n}, K)")
    k = 1 if ndim == 1 else int(V.shape[1])
    if ndim == 1 and (len(polys) == 0 or np.ndim(polys[0]) == 0):
        polys = [polys]
    deg, coef, ldc = _poly_table(polys, k)
    lib = _abi.lib()
    if is_torch:
        import torch

        if V.dtype != torch.int32 or V.device.type != "cuda" or V.device.index != torch.cuda.current_device():
            raise TypeError("V must be an int32 tensor on the current device")
        if V.stride(-1) != 1 or (ndim == 2 and V.shape[0] > 1 and V.stride(0) < k):
            raise ValueError("V must have unit stride along its rows")
        ldv = k if ndim == 1 else max(V.stride(0), k)
        X = torch.empty(tuple(V.shape), dtype=torch.int32, device=V.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.spasm_amd_poly_apply_dev(op._op, int(bool(trans)), k, deg.ctypes.data, coef.ctypes.data, ldc, C.c_void_p(V.data_ptr()), ldv,
                                          C.c_void_p(X.data_ptr()), k, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return X
    if not isinstance(V, np.ndarray) or V.dtype != np.int32:
        raise TypeError("V must be an int32 numpy array or torch tensor")
    Vc = _rows_view(V, "V")
    ldv = k if ndim == 1 else max(Vc.strides[0] // 4, k)
    X = np.zeros(V.shape, dtype=np.int32)
    rc = lib.spasm_amd_poly_apply(op._op, int(bool(trans)), k, deg.ctypes.data, coef.ctypes.data, ldc, Vc.ctypes.data, ldv, X.ctypes.data, k)
    if rc != 0:
        raise SpasmError(_abi.last_error())
    return X


def wiedemann_solve(A, B, trans=False, seed=0, tries=3, maxdeg=None, U=None):
    """wiedemann_solve(A, B, trans=False, seed=0, tries=3, maxdeg=None, U=None) -> (X, status): A x = b (x A = b with trans=True)
    for every column b of B by Wiedemann's method, without elimination or fill-in.  A is a square CSR (spasm_amd_wiedemann_solve),
    an SpMV operator (spasm_amd_spmv_wiedemann_solve) or a DeviceCSR (spasm_amd_dcsr_wiedemann_solve).  B is n x K, 1 <= K <= 64,
    or n entries: one right-hand side (X then has n entries).  X is int32, balanced residues; status is an int32 array, one per
    column:  1  solved, A x = b verified on the device;  2  the column of X is a non-zero vector of the kernel of A (A is singular:
    certain; nothing is said about b);  0  undecided after `tries` tries with the seeds seed, seed + 1, .. (the column of X is
    zero).  U (n x K) fixes the projection vectors and allows one try only.  maxdeg bounds the degree of the polynomials (None: n)."""
    who, fn, arg, n = _family_target(A, "wiedemann_solve")
    if not isinstance(B, np.ndarray) or B.dtype != np.int32 or B.ndim not in (1, 2) or B.shape[0] != n:
        raise TypeError(f"B must be an int32 numpy array of shape ({n},) or ({n}, K)")
    k = 1 if B.ndim == 1 else B.shape[1]
    Bc = _rows_view(B, "B") if n > 0 else B   # (numpy gives an array without rows strides of its own)
    ldb = k if B.ndim == 1 or n == 0 else max(Bc.strides[0] // 4, k)
    uptr = None
    if U is not None:
        if not isinstance(U, np.ndarray) or U.dtype != np.int32 or U.size != n * k or U.shape[0] != n or not U.flags["C_CONTIGUOUS"]:
            raise TypeError(f"U must be a contiguous int32 numpy array of shape ({n}, {k})")
        uptr = U.ctypes.data
    X = np.zeros(B.shape, dtype=np.int32)
    status = np.zeros(max(k, 1), dtype=np.int32)
    with _quiet(True):
        rc = fn(arg, int(bool(trans)), int(k), Bc.ctypes.data, ldb, int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), 0 if maxdeg is None else int(maxdeg),
                uptr, X.ctypes.data, max(k, 1), status.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return X, status[:k]


def wiedemann_stats():
    """Counters of the last poly_apply / wiedemann_solve call of this thread (spasm_amd_wiedemann_stats), keyed by WIEDEMANN_STATS."""
    out = (C.c_int64 * 10)()
    _abi.lib().spasm_amd_wiedemann_stats(out)
    return {k: int(v) for k, v in zip(WIEDEMANN_STATS, out)}


SpMV.poly_apply = poly_apply
SpMV.wiedemann_solve = wiedemann_solve
DeviceCSR.wiedemann_solve = wiedemann_solve


# ---------------------------------------------------------------------------------------------
# Rank and determinant by preconditioned Wiedemann  (spasm_amd_wiedemann_rank*, _wiedemann_det*, _precond_*; csrc/precond.hpp)
# ---------------------------------------------------------------------------------------------
PRECOND_STATS = ("n", "m", "K", "tries", "products", "launches", "degree", "x_multiplicity", "sequence_device_us", "bm_device_us")


def wiedemann_rank(A, K=8, seed=0, tries=3, maxdeg=None):
    """wiedemann_rank(A, K=8, seed=0, tries=3, maxdeg=None) -> (rank, certain): the rank of the n x m matrix A mod p by
    preconditioned Wiedemann, without elimination or fill-in.  A is a CSR (spasm_amd_wiedemann_rank), an SpMV operator
    (spasm_amd_spmv_wiedemann_rank) or a DeviceCSR (spasm_amd_dcsr_wiedemann_rank).  The result is a lower bound, always; it equals
    the rank with a probability that grows with p, and certain is True only when it reaches min(n, m).  `tries` seeds seed,
    seed + 1, .. are used and the largest bound is returned.  maxdeg bounds the rank looked for (None: min(n, m)); a larger one
    is refused ("degree bound too small")."""
    who, fn, arg, _ = _family_target(A, "wiedemann_rank")
    rank, certain = C.c_int64(0), C.c_int32(0)
    with _quiet(True):
        rc = fn(arg, int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), 0 if maxdeg is None else int(maxdeg), C.byref(rank), C.byref(certain))
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return int(rank.value), bool(certain.value)


def wiedemann_det(A, K=8, seed=0, tries=3):
    """wiedemann_det(A, K=8, seed=0, tries=3) -> (det, status): the determinant of the square matrix A mod p as a balanced residue
    by preconditioned Wiedemann, without elimination or fill-in.  A is a CSR (spasm_amd_wiedemann_det), an SpMV operator
    (spasm_amd_spmv_wiedemann_det) or a DeviceCSR (spasm_amd_dcsr_wiedemann_det).  status 1: det is certain; status 0: undecided
    after `tries` tries with the seeds seed, seed + 1, .. (det is 0 then and says nothing)."""
    who, fn, arg, _ = _family_target(A, "wiedemann_det")
    det, status = C.c_int32(0), C.c_int32(0)
    with _quiet(True):
        rc = fn(arg, int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), C.byref(det), C.byref(status))
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return int(det.value), int(status.value)


def precond_diagonal(length, seed, which, prime):
    """The int32 diagonal of `length` non-zero balanced residues that try `seed` of wiedemann_rank / wiedemann_det uses
    (spasm_amd_precond_diagonal): which = 0 the left one (D2, or D of the determinant), which = 1 the right one (E = D1^2)."""
    d = np.zeros(int(length), dtype=np.int32)
    rc = _abi.lib().spasm_amd_precond_diagonal(int(length), int(seed) & 0xFFFFFFFFFFFFFFFF, int(which), int(prime), d.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_precond_diagonal failed")
    return d


def precond_sequence(op, mode, d_left, d_right, U, V, length):
    """precond_sequence(op, mode, d_left, d_right, U, V, length) -> S of shape (length, K): the projected sequence
    S[i, c] = sum_r U[r, c] * (B^i V)[r, c] mod p of the preconditioned operator with the caller's diagonals
    (spasm_amd_precond_sequence).  mode 0: B = diag(d_left) A, A square (d_right may be None).  mode 1: B = diag(d_right) A^T
    diag(d_left) A for the n x m matrix A of the SpMV operator op; d_left has n words, d_right m, U and V are m x K.  All int32
    numpy arrays, any int32 is reduced where it is read."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n, m = op.shape
    length = int(length)
    if length < 0:
        raise ValueError("length must not be negative")
    for a, name in ((U, "U"), (V, "V")):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 2 or a.shape[0] != m or a.shape != U.shape:
            raise TypeError(f"{name} must be an int32 numpy array of shape ({m}, K)")
    k = U.shape[1]
    Uc, Vc = np.ascontiguousarray(U), np.ascontiguousarray(V)
    diag = []
    for a, name, size in ((d_left, "d_left", n), (d_right, "d_right", m)):
        if a is None:
            diag.append(None)
            continue
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != (size,):
            raise TypeError(f"{name} must be an int32 numpy array of {size} words")
        diag.append(np.ascontiguousarray(a))
    S = np.zeros((length, k), dtype=np.int32)
    rc = _abi.lib().spasm_amd_precond_sequence(op._op, int(mode), int(k), length, None if diag[0] is None else diag[0].ctypes.data,
                                               None if diag[1] is None else diag[1].ctypes.data, Uc.ctypes.data, k, Vc.ctypes.data, k, S.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_precond_sequence failed")
    return S


def precond_stats():
    """Counters of the last preconditioned Wiedemann call of this thread (spasm_amd_precond_stats), keyed by PRECOND_STATS."""
    out = (C.c_int64 * 10)()
    _abi.lib().spasm_amd_precond_stats(out)
    return {k: int(v) for k, v in zip(PRECOND_STATS, out)}


SpMV.wiedemann_rank = wiedemann_rank
SpMV.wiedemann_det = wiedemann_det
SpMV.precond_sequence = precond_sequence
DeviceCSR.wiedemann_rank = wiedemann_rank
DeviceCSR.wiedemann_det = wiedemann_det


# ---------------------------------------------------------------------------------------------
# Block Wiedemann  (spasm_amd_block_sequence*, _block_berlekamp_massey, _block_wiedemann_det*; csrc/block_krylov.hpp, block_bm.hpp)
# ---------------------------------------------------------------------------------------------
BLOCK_STATS = ("b", "len", "steps", "launches", "degree_sum", "tries", "sequence_device_us", "bm_device_us", "n", "max_degree")


def block_sequence(op, U, V, length, trans=False, d_left=None):
    """block_sequence(op, U, V, length, trans=False, d_left=None) -> S of shape (length, b, b):
    S[i, r, c] = sum_k U[k, r] * (M^i V)[k, c] mod p as balanced residues, M = A, the square matrix of the SpMV operator op (A^T
    with trans=True), or diag(d_left) times it.  U and V are n x b, b in (2, 4, 8, 16); d_left has n words, none zero mod p.
    int32 numpy arrays (spasm_amd_block_sequence) or int32 torch tensors on the current device (enqueued on the current stream
    without a host synchronization; S is a tensor and d_left is not checked: spasm_amd_block_sequence_dev).  Any int32 is reduced
    where it is read; U, V and d_left are not modified."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n = op.shape[0]
    length = int(length)
    lib = _abi.lib()
    if type(U).__module__.startswith("torch") or type(V).__module__.startswith("torch"):
        import torch

        tensors = [(U, "U"), (V, "V")] + ([(d_left, "d_left")] if d_left is not None else [])
        for t, name in tensors:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device.type != "cuda" or t.device.index != torch.cuda.current_device():
                raise TypeError(f"{name} must be an int32 tensor on the current device")
        for t, name in tensors[:2]:
            if t.dim() != 2 or t.shape[0] != n or tuple(t.shape) != tuple(U.shape):
                raise ValueError(f"U and V must both have shape ({n}, b), not {tuple(t.shape)}")
        b = int(U.shape[1])
        for t, name in tensors[:2]:
            if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < b):
                raise ValueError(f"{name} must have unit stride along its rows")
        if d_left is not None and (tuple(d_left.shape) != (n,) or not d_left.is_contiguous()):
            raise ValueError(f"d_left must be a contiguous tensor of {n} words")
        S = torch.empty((max(length, 0), b, b), dtype=torch.int32, device=U.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.spasm_amd_block_sequence_dev(op._op, int(bool(trans)), b, length, None if d_left is None else C.c_void_p(d_left.data_ptr()),
                                              C.c_void_p(U.data_ptr()), max(U.stride(0), b), C.c_void_p(V.data_ptr()), max(V.stride(0), b),
                                              C.c_void_p(S.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return S
    for a, name in ((U, "U"), (V, "V")):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise TypeError(f"{name} must be an int32 numpy array or torch tensor")
        if a.ndim != 2 or a.shape[0] != n or a.shape != U.shape:
            raise ValueError(f"U and V must both have shape ({n}, b), not {a.shape}")
    b = U.shape[1]
    Uc, Vc = np.ascontiguousarray(U), np.ascontiguousarray(V)
    dptr = None
    if d_left is not None:
        if not isinstance(d_left, np.ndarray) or d_left.dtype != np.int32 or d_left.shape != (n,):
            raise TypeError(f"d_left must be an int32 numpy array of {n} words")
        dl = np.ascontiguousarray(d_left)
        dptr = dl.ctypes.data
    S = np.zeros((max(length, 0), b, b), dtype=np.int32)
    rc = lib.spasm_amd_block_sequence(op._op, int(bool(trans)), int(b), length, dptr, Uc.ctypes.data, b, Vc.ctypes.data, b, S.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error())
    return S


def block_berlekamp_massey(S_, prime):
    """block_berlekamp_massey(S, prime) -> (F, rowdeg): a left generator of the matrix sequence S (len x b x b integers, b in
    (2, 4, 8, 16)) mod prime by Berlekamp-Massey over matrix sequences on the device (spasm_amd_block_berlekamp_massey).  F is an
    int32 array of shape (max(rowdeg) + 1, b, b), F[t] the coefficient of x^t, balanced residues; rowdeg[r] is the degree of row r.
    For every row r and 0 <= i < len - rowdeg[r]: sum_t F[t, r, :] @ S[i + t] = 0 mod prime; the matrix of the leading row
    coefficients F[rowdeg[r], r, :] is non-singular; the degrees are minimal.  F is unique only up to row operations: two runs give
    the same bytes, another implementation may give another F.  The zero sequence gives F = I."""
    S_ = np.asarray(S_)
    if S_.dtype.kind not in "iu":
        raise TypeError("integer entries expected")
    if S_.ndim != 3 or S_.shape[1] != S_.shape[2]:
        raise ValueError("a len x b x b array expected")
    S_ = np.ascontiguousarray(balanced(S_, int(prime)))
    length, b = int(S_.shape[0]), int(S_.shape[1])
    coef = np.zeros((length + 1, b, b), dtype=np.int32)
    rowdeg = np.zeros(max(b, 1), dtype=np.int32)
    dmax = C.c_int32(0)
    rc = _abi.lib().spasm_amd_block_berlekamp_massey(b, length, S_.ctypes.data, int(prime), coef.ctypes.data, rowdeg.ctypes.data, C.byref(dmax))
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_block_berlekamp_massey failed")
    return coef[: dmax.value + 1].copy(), rowdeg[:b].copy()


def block_wiedemann_det(A, b=8, seed=0, tries=3):
    """block_wiedemann_det(A, b=8, seed=0, tries=3) -> (det, status): the determinant of the square matrix A mod p as a balanced
    residue by block Wiedemann, without elimination or fill-in, from about 2 n / b products with A where wiedemann_det takes 2 n.
    A is a CSR (spasm_amd_block_wiedemann_det), an SpMV operator (spasm_amd_spmv_block_wiedemann_det) or a DeviceCSR
    (spasm_amd_dcsr_block_wiedemann_det); b is 2, 4, 8 or 16.  status 1: the generator of the block sequence has full degree and
    det was read off it.  This is a Monte Carlo answer, not a verified one: it is right with a probability that grows with p (and
    is poor for p = 3), and unlike wiedemann_det nothing proves it, because the block sequence has only about 2 n / b terms.
    status 0: undecided after `tries` tries with the seeds seed, seed + 1, .. (det is 0 then and says nothing)."""
    who, fn, arg, _ = _family_target(A, "block_wiedemann_det")
    det, status = C.c_int32(0), C.c_int32(0)
    with _quiet(True):
        rc = fn(arg, int(b), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), C.byref(det), C.byref(status))
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return int(det.value), int(status.value)


def block_stats():
    """Counters of the last block Wiedemann call of this thread (spasm_amd_block_stats), keyed by BLOCK_STATS."""
    out = (C.c_int64 * 10)()
    _abi.lib().spasm_amd_block_stats(out)
    return {k: int(v) for k, v in zip(BLOCK_STATS, out)}


SpMV.block_sequence = block_sequence
SpMV.block_wiedemann_det = block_wiedemann_det
DeviceCSR.block_wiedemann_det = block_wiedemann_det


# ---------------------------------------------------------------------------------------------
# Block Horner and the block Wiedemann solve  (spasm_amd_block_poly_apply*, _block_wiedemann_solve*; csrc/block_horner.hpp)
# ---------------------------------------------------------------------------------------------
BLOCK_SOLVE_STATS = ("n", "b", "K", "len", "tries", "products", "sequence_products", "horner_products", "launches", "degree_sum",
                     "max_degree", "solved", "kernel_vectors", "sequence_device_us", "bm_device_us", "horner_device_us")


def block_poly_apply(op, coef, V, trans=False):
    """block_poly_apply(op, C, V, trans=False) -> X = sum_t A^t V C[t] mod p as balanced residues, n x K: A the square matrix of
    the SpMV operator op (A^T with trans=True), V n x b with b in (2, 4, 8, 16), C an integer array of shape (D + 1, b, K) with
    1 <= K <= b (any int32; D + 1 = 0 gives X = 0).  int32 numpy arrays (spasm_amd_block_poly_apply) or V an int32 torch tensor
    on the current device (enqueued on the current stream without a host synchronization; X is a tensor:
    spasm_amd_block_poly_apply_dev).  Block Horner: D products with A, each followed by the b x K combination.  V is not modified."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n = op.shape[0]
    Cc = np.asarray(coef)
    if Cc.ndim != 3:
        raise ValueError("C must have shape (D + 1, b, K)")
    if Cc.size and (Cc.dtype.kind not in "iu" or Cc.min() < -2**31 or Cc.max() > 2**31 - 1):
        raise TypeError("the coefficients must be integers that fit int32")
    Cc = np.ascontiguousarray(Cc, dtype=np.int32)
    D, b, k = int(Cc.shape[0]) - 1, int(Cc.shape[1]), int(Cc.shape[2])
    is_torch = type(V).__module__.startswith("torch")
    ndim = V.dim() if is_torch else getattr(V, "ndim", 0)
    if ndim != 2 or tuple(V.shape) != (n, b):
        raise ValueError(f"V must have shape ({n}, {b})")
    lib = _abi.lib()
    cptr = Cc.ctypes.data if Cc.size else None
    if is_torch:
        import torch

        if V.dtype != torch.int32 or V.device.type != "cuda" or V.device.index != torch.cuda.current_device():
            raise TypeError("V must be an int32 tensor on the current device")
        if V.stride(-1) != 1 or (V.shape[0] > 1 and V.stride(0) < b):
            raise ValueError("V must have unit stride along its rows")
        X = torch.empty((n, k), dtype=torch.int32, device=V.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.spasm_amd_block_poly_apply_dev(op._op, int(bool(trans)), b, k, D, cptr, C.c_void_p(V.data_ptr()), max(V.stride(0), b),
                                                C.c_void_p(X.data_ptr()), max(k, 1), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise SpasmError(_abi.last_error())
        return X
    if not isinstance(V, np.ndarray) or V.dtype != np.int32:
        raise TypeError("V must be an int32 numpy array or torch tensor")
    Vc = np.ascontiguousarray(V)
    X = np.zeros((n, k), dtype=np.int32)
    rc = lib.spasm_amd_block_poly_apply(op._op, int(bool(trans)), b, k, D, cptr, Vc.ctypes.data, b, X.ctypes.data, max(k, 1))
    if rc != 0:
        raise SpasmError(_abi.last_error())
    return X


def block_wiedemann_solve(A, B, b=8, trans=False, seed=0, tries=3):
    """block_wiedemann_solve(A, B, b=8, trans=False, seed=0, tries=3) -> (X, status): A x = b (x A = b with trans=True) for every
    column of B by block Wiedemann, without elimination or fill-in, from about 3 n / b products with A where wiedemann_solve takes
    up to 3 n.  A is a square CSR (spasm_amd_block_wiedemann_solve), an SpMV operator (spasm_amd_spmv_block_wiedemann_solve) or a
    DeviceCSR (spasm_amd_dcsr_block_wiedemann_solve); the block width b is 2, 4, 8 or 16.  B is n x K, 1 <= K <= b, or n entries:
    one right-hand side (X then has n entries).  X is int32, balanced residues; status is an int32 array, one per column:
    1  solved, A x = b verified on the device by one more product;  2  the column of X is a non-zero vector of the kernel of A,
    verified the same way (nothing is said about b);  0  undecided after `tries` tries with the seeds seed, seed + 1, .. (the
    column of X is zero).  Statuses 1 and 2 are proofs, not Monte Carlo answers: the residual is computed."""
    who, fn, arg, n = _family_target(A, "block_wiedemann_solve")
    if not isinstance(B, np.ndarray) or B.dtype != np.int32 or B.ndim not in (1, 2) or B.shape[0] != n:
        raise TypeError(f"B must be an int32 numpy array of shape ({n},) or ({n}, K)")
    k = 1 if B.ndim == 1 else B.shape[1]
    Bc = _rows_view(B, "B") if n > 0 else B   # (numpy gives an array without rows strides of its own)
    ldb = k if B.ndim == 1 or n == 0 else max(Bc.strides[0] // 4, k)
    X = np.zeros(B.shape, dtype=np.int32)
    status = np.zeros(max(k, 1), dtype=np.int32)
    with _quiet(True):
        rc = fn(arg, int(bool(trans)), int(b), int(k), Bc.ctypes.data, ldb, int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), X.ctypes.data, max(k, 1),
                status.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return X, status[:k]


def block_solve_stats():
    """Counters of the last block_poly_apply / block_wiedemann_solve call of this thread (spasm_amd_block_solve_stats), keyed by
    BLOCK_SOLVE_STATS."""
    out = (C.c_int64 * len(BLOCK_SOLVE_STATS))()
    _abi.lib().spasm_amd_block_solve_stats(out)
    return {k: int(v) for k, v in zip(BLOCK_SOLVE_STATS, out)}


SpMV.block_poly_apply = block_poly_apply
SpMV.block_wiedemann_solve = block_wiedemann_solve
DeviceCSR.block_wiedemann_solve = block_wiedemann_solve


# ---------------------------------------------------------------------------------------------
# Kernel bases without fill-in  (spasm_amd_dense_column_echelon, _block_precond_sequence, _wiedemann_kernel*; csrc/colechelon.hpp)
# ---------------------------------------------------------------------------------------------
WIEDEMANN_KERNEL_STATS = ("n", "m", "b", "want", "tries", "products", "sequence_products", "horner_products", "check_products",
                          "certify_products", "launches", "candidates", "accepted", "dependent", "found", "sequence_device_us",
                          "bm_device_us", "horner_device_us", "echelon_device_us")


def column_echelon(X, prime):
    """column_echelon(X, prime) -> (E, pivots): the reduced column echelon form mod prime of the column space of X, an int32 numpy
    array of shape (rows, K), K <= 64 (any int32 is reduced), by column-wise elimination on the device
    (spasm_amd_dense_column_echelon).  E has the shape of X: column j < len(pivots) has its first non-zero entry, a 1, in row
    pivots[j]; pivots ascends strictly; row pivots[j] is zero in every other column; the remaining columns are zero; balanced
    residues.  The form is unique: two blocks with the same column space give the same bytes.  X is not modified."""
    if not isinstance(X, np.ndarray) or X.dtype != np.int32 or X.ndim != 2:
        raise TypeError("X must be a two-dimensional int32 numpy array")
    rows, k = X.shape
    E = np.array(X, dtype=np.int32, order="C")
    pivots = np.zeros(max(k, 1), dtype=np.int32)
    rank = C.c_int32(0)
    rc = _abi.lib().spasm_amd_dense_column_echelon(rows, k, E.ctypes.data, max(k, 1), int(prime), C.byref(rank), pivots.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_dense_column_echelon failed")
    return E, pivots[: rank.value].copy()


def block_precond_sequence(op, U, V, length, d_left, d_right=None, trans=False):
    """block_precond_sequence(op, U, V, length, d_left, d_right=None, trans=False) -> S of shape (length, b, b):
    S[i, r, c] = sum_k U[k, r] * (M^i V)[k, c] mod p as balanced residues, M = diag(d_right) op(A)^T diag(d_left) op(A) for the
    SpMV operator op of a matrix A that may be rectangular (op(A) = A^T with trans=True); d_right=None is the identity.  U and V
    are dim x b int32 numpy arrays, dim the number of columns of op(A), b in (2, 4, 8, 16); d_left has one word per row of op(A),
    d_right dim words (spasm_amd_block_precond_sequence).  Any int32 is reduced where it is read."""
    if not isinstance(op, SpMV):
        raise TypeError("an SpMV operator expected")
    if not op._op:
        raise SpasmError("the operator is closed")
    n, m = (op.shape[1], op.shape[0]) if trans else (op.shape[0], op.shape[1])
    for a, name in ((U, "U"), (V, "V")):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise TypeError(f"{name} must be an int32 numpy array")
        if a.ndim != 2 or a.shape[0] != m or a.shape != U.shape:
            raise ValueError(f"U and V must both have shape ({m}, b), not {a.shape}")
    b = int(U.shape[1])
    diag = []
    for d, name, words in ((d_left, "d_left", n), (d_right, "d_right", m)):
        if d is None and name == "d_right":
            diag.append(None)
            continue
        if not isinstance(d, np.ndarray) or d.dtype != np.int32 or d.shape != (words,):
            raise TypeError(f"{name} must be an int32 numpy array of {words} words")
        diag.append(np.ascontiguousarray(d))
    Uc, Vc = np.ascontiguousarray(U), np.ascontiguousarray(V)
    length = int(length)
    S = np.zeros((max(length, 0), b, b), dtype=np.int32)
    rc = _abi.lib().spasm_amd_block_precond_sequence(op._op, int(bool(trans)), b, length, diag[0].ctypes.data,
                                                     None if diag[1] is None else diag[1].ctypes.data, Uc.ctypes.data, b, Vc.ctypes.data, b,
                                                     S.ctypes.data)
    if rc != 0:
        raise SpasmError(_abi.last_error() or "spasm_amd_block_precond_sequence failed")
    return S


def wiedemann_kernel(A, want=None, b=8, trans=False, seed=0, tries=3, certify=False):
    """wiedemann_kernel(A, want=None, b=8, trans=False, seed=0, tries=3, certify=False) -> (N, pivots, complete): vectors x with
    A x = 0 (x A = 0 with trans=True) as the columns of N, dim x found, int32 balanced residues, by block Wiedemann on
    A^T D2 A without elimination or fill-in.  A is a CSR, rectangular or square (spasm_amd_wiedemann_kernel), an SpMV operator
    (spasm_amd_spmv_wiedemann_kernel) or a DeviceCSR (spasm_amd_dcsr_wiedemann_kernel); b is 2, 4, 8 or 16; found <= want <= 64
    and want=None means min(64, tries * b).  N is in the reduced column echelon form of column_echelon, with the pivot rows pivots.
    Every column is a proved kernel vector (its residual against A is computed on the device) and the columns are independent.
    complete is True only with certify=True and only when found equals dim minus the lower bound of the rank that wiedemann_rank's
    procedure gives (K = 8, the same seeds): then N is a basis of the whole kernel, and that is a proof, not a Monte Carlo claim.
    complete False says nothing: no certificate was asked for, the numbers did not meet, or want cut the basis short."""
    who, fn, arg, _ = _family_target(A, "wiedemann_kernel")
    n, m = (A.n, A.m) if isinstance(A, CSR) else (A.shape[0], A.shape[1])
    dim = n if trans else m
    tries = int(tries)
    b = int(b)
    if want is None:
        want = max(0, min(64, tries * b))
    want = int(want)
    N = np.zeros((dim, max(want, 0)), dtype=np.int32)
    pivots = np.zeros(max(want, 1), dtype=np.int32)
    found, complete = C.c_int32(0), C.c_int32(0)
    with _quiet(True):
        rc = fn(arg, int(bool(trans)), b, want, int(seed) & 0xFFFFFFFFFFFFFFFF, tries, int(bool(certify)), N.ctypes.data, max(want, 1),
                C.byref(found), pivots.ctypes.data, C.byref(complete))
    if rc != 0:
        raise SpasmError(_abi.last_error() or f"{who} failed")
    return np.ascontiguousarray(N[:, : found.value]), pivots[: found.value].copy(), bool(complete.value)


def wiedemann_kernel_stats():
    """Counters of the last wiedemann_kernel call of this thread (spasm_amd_wiedemann_kernel_stats), keyed by
    WIEDEMANN_KERNEL_STATS.  block_precond_sequence fills the slots of its sequence; column_echelon fills launches, found (the
    rank) and echelon_device_us."""
    out = (C.c_int64 * len(WIEDEMANN_KERNEL_STATS))()
    _abi.lib().spasm_amd_wiedemann_kernel_stats(out)
    return {k: int(v) for k, v in zip(WIEDEMANN_KERNEL_STATS, out)}


SpMV.block_precond_sequence = block_precond_sequence
SpMV.wiedemann_kernel = wiedemann_kernel
DeviceCSR.wiedemann_kernel = wiedemann_kernel
