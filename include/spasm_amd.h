/*
 * spasm_amd.h -- C ABI of the MI355X-native sparse GF(p) echelonization engine.
 *
 * This is the drop-in boundary: every `spasm_*` symbol below has the name, argument
 * order and struct layout that SpaSM.jl binds with `@ccall spasm_lib.<sym>` (reference
 * file `src/SpaSM.jl`; the line of each binding is cited next to the declaration).
 * Pointing `spasm_lib` at `libspasm_amd.so` re-routes the echelonize / kernel hot path
 * to the HIP engine without touching the Julia side.
 *
 * Conventions (all from the reference wrapper):
 *   - indices are 0-based on this side of the boundary      (src/SpaSM.jl:486,597,961)
 *   - values are balanced residues in [mhalfp, halfp], i32  (src/SpaSM.jl:79-88)
 *   - rows of a CSR need not be sorted by column            (src/SpaSM.jl:1017-1020)
 *   - returned objects are owned by the caller and released with spasm_csr_free /
 *     spasm_lu_free from an arbitrary thread                (src/SpaSM.jl:146-150,273-277)
 *
 * The `spasm_amd_*` symbols are engine extensions (device-resident handles for
 * benchmarking and multi-GPU sharding); the reference has no counterpart for them.
 */
#ifndef SPASM_AMD_H
#define SPASM_AMD_H

#include <stdint.h>
#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t i64;
typedef int32_t spasm_ZZp; /* balanced representative, src/SpaSM.jl:79-81 */

/* struct Field, src/SpaSM.jl:51-56 (32 bytes, embedded by value) */
struct spasm_field_struct {
    i64 p;
    i64 halfp;
    i64 mhalfp;
    double dinvp;
};
typedef struct spasm_field_struct spasm_field[1];

/* struct _CSR, src/SpaSM.jl:126-134 (72 bytes) */
struct spasm_csr {
    i64 nzmax;
    int n;          /* rows */
    int m;          /* columns */
    i64 *p;         /* n+1 row starts */
    int *j;         /* column indices */
    spasm_ZZp *x;   /* values (may be NULL when allocated with_values = false) */
    spasm_field field;
};

/* struct _Triplet, src/SpaSM.jl:234-243 (80 bytes) */
struct spasm_triplet {
    i64 nzmax;
    i64 nz;
    int n;
    int m;
    int *i;
    int *j;
    spasm_ZZp *x;
    spasm_field field;
};

/* struct _LU, src/SpaSM.jl:262-270 (48 bytes) */
struct spasm_lu {
    int r;                    /* rank */
    bool complete;            /* L present and complete */
    struct spasm_csr *L;      /* NULL unless opts->L */
    struct spasm_csr *U;      /* r x m, unit pivots, pivot not necessarily first in row */
    int *qinv;                /* m entries: row of U holding the pivot of column j, or -1 */
    int *p;                   /* >= m entries (Julia views it with length U->m, :300) */
    struct spasm_triplet *Ltmp;
};

/* struct EchelonizeOpts, src/SpaSM.jl:325-343 (64 bytes) */
struct echelonize_opts {
    bool enable_greedy_pivot_search;
    bool enable_tall_and_skinny;
    bool enable_dense;
    bool enable_GPLU;
    bool L;
    bool complete;
    double min_pivot_proportion;
    int max_round;
    double sparsity_threshold;
    int dense_block_size;     /* Julia declares Int (8 bytes) at :339; low 32 bits are read */
    double low_rank_ratio;
    double tall_and_skinny_ratio;
    double low_rank_start_weight;
};

/* The layouts SpaSM.jl's mirrors imply (x86-64, little-endian), checked where the header is compiled: a field that
 * moves is a build error here, not a wrong pointer in Julia. */
#if defined(__cplusplus)
#define SPASM_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define SPASM_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
SPASM_LAYOUT_ASSERT(sizeof(struct spasm_field_struct) == 32 && offsetof(struct spasm_field_struct, p) == 0 && offsetof(struct spasm_field_struct, halfp) == 8 &&
                        offsetof(struct spasm_field_struct, mhalfp) == 16 && offsetof(struct spasm_field_struct, dinvp) == 24,
                    "spasm_field: src/SpaSM.jl:51-56");
SPASM_LAYOUT_ASSERT(sizeof(struct spasm_csr) == 72 && offsetof(struct spasm_csr, nzmax) == 0 && offsetof(struct spasm_csr, n) == 8 && offsetof(struct spasm_csr, m) == 12 &&
                        offsetof(struct spasm_csr, p) == 16 && offsetof(struct spasm_csr, j) == 24 && offsetof(struct spasm_csr, x) == 32 &&
                        offsetof(struct spasm_csr, field) == 40,
                    "spasm_csr: src/SpaSM.jl:126-134");
SPASM_LAYOUT_ASSERT(sizeof(struct spasm_triplet) == 80 && offsetof(struct spasm_triplet, nz) == 8 && offsetof(struct spasm_triplet, n) == 16 &&
                        offsetof(struct spasm_triplet, m) == 20 && offsetof(struct spasm_triplet, i) == 24 && offsetof(struct spasm_triplet, j) == 32 &&
                        offsetof(struct spasm_triplet, x) == 40 && offsetof(struct spasm_triplet, field) == 48,
                    "spasm_triplet: src/SpaSM.jl:234-243");
SPASM_LAYOUT_ASSERT(sizeof(struct spasm_lu) == 48 && offsetof(struct spasm_lu, r) == 0 && offsetof(struct spasm_lu, complete) == 4 && offsetof(struct spasm_lu, L) == 8 &&
                        offsetof(struct spasm_lu, U) == 16 && offsetof(struct spasm_lu, qinv) == 24 && offsetof(struct spasm_lu, p) == 32 &&
                        offsetof(struct spasm_lu, Ltmp) == 40,
                    "spasm_lu: src/SpaSM.jl:262-270");
SPASM_LAYOUT_ASSERT(sizeof(struct echelonize_opts) == 64 && offsetof(struct echelonize_opts, enable_greedy_pivot_search) == 0 &&
                        offsetof(struct echelonize_opts, enable_tall_and_skinny) == 1 && offsetof(struct echelonize_opts, enable_dense) == 2 &&
                        offsetof(struct echelonize_opts, enable_GPLU) == 3 && offsetof(struct echelonize_opts, L) == 4 && offsetof(struct echelonize_opts, complete) == 5 &&
                        offsetof(struct echelonize_opts, min_pivot_proportion) == 8 && offsetof(struct echelonize_opts, max_round) == 16 &&
                        offsetof(struct echelonize_opts, sparsity_threshold) == 24 && offsetof(struct echelonize_opts, dense_block_size) == 32 &&
                        offsetof(struct echelonize_opts, low_rank_ratio) == 40 && offsetof(struct echelonize_opts, tall_and_skinny_ratio) == 48 &&
                        offsetof(struct echelonize_opts, low_rank_start_weight) == 56,
                    "echelonize_opts: src/SpaSM.jl:325-343");

/* ---- data symbol: SpaSM.log() stores a C callback here, src/SpaSM.jl:34-46 ---- */
extern int (*logcallback)(char *);

/* ---- spasm_util.c surface ---- */
double spasm_wtime(void);                                            /* src/SpaSM.jl:430 */
i64 spasm_nnz(const struct spasm_csr *A);                            /* src/SpaSM.jl:432 */
struct spasm_csr *spasm_csr_alloc(int n, int m, i64 nzmax, i64 prime, bool with_values); /* :441 */
void spasm_csr_realloc(struct spasm_csr *A, i64 nzmax);              /* src/SpaSM.jl:447 */
void spasm_csr_resize(struct spasm_csr *A, int n, int m);            /* src/SpaSM.jl:449 */
void spasm_csr_free(struct spasm_csr *A);                            /* src/SpaSM.jl:451 */
void spasm_lu_free(struct spasm_lu *N);                              /* src/SpaSM.jl:463 */
int spasm_get_num_threads(void);                                     /* src/SpaSM.jl:470 */
int spasm_get_thread_num(void);                                      /* src/SpaSM.jl:475 */

/* ---- spasm_triplet.c / spasm_io.c surface: the SMS wire format ("n m M" header, 1-based "i j v" lines,
 * "0 0 0" terminator; reference src/SpaSM.jl:1029-1042, :1063-1086).  Host-side I/O, no device work. ---- */
struct spasm_triplet *spasm_triplet_alloc(int n, int m, i64 nzmax, i64 prime, bool with_values); /* src/SpaSM.jl:453 */
void spasm_triplet_realloc(struct spasm_triplet *T, i64 nzmax);      /* src/SpaSM.jl:455 */
void spasm_triplet_free(struct spasm_triplet *T);                    /* src/SpaSM.jl:457 */
void spasm_add_entry(struct spasm_triplet *T, int i, int j, i64 x);  /* src/SpaSM.jl:486 */
void spasm_triplet_transpose(struct spasm_triplet *T);               /* src/SpaSM.jl:491 */
struct spasm_csr *spasm_compress(const struct spasm_triplet *T);     /* src/SpaSM.jl:493 */
struct spasm_triplet *spasm_triplet_load(void *file, i64 prime, uint8_t *hash); /* FILE*, src/SpaSM.jl:501; hash = SHA-256 of the stream or NULL */
void spasm_triplet_save(const struct spasm_triplet *T, void *file);  /* FILE*, src/SpaSM.jl:514 */
void spasm_csr_save(const struct spasm_csr *A, void *file);          /* FILE*, src/SpaSM.jl:523 */

/* ---- spasm_certificate.c: the probabilistic self-check of a factorization (src/SpaSM.jl:934).  Host-side, O(nnz).
 * Checks (a) the shape of the echelon form: every row of U holds a 1 on its pivot column qinv^-1(k) and U is (permuted)
 * triangular, so its rows are independent; (b) for random vectors x drawn from `seed`, that x*A reduces to zero modulo the rows
 * of U, i.e. that the row space of A lies in that of U (a wrong U escapes with probability <= 1/p per trial; 2 trials, 8 for
 * p < 2^16).  Together: rank(A) <= r and U spans at least the rows of A.
 * With fact->L (echelonize_opts.L) the check is two-sided, as libspasm's: (c) x*L*U == x*A for random x, i.e. A == L*U, and
 * (d) the rows p[0 .. r) of L form a triangular matrix with a non-zero diagonal, so U = L_P^-1 A_P: every row of U lies in the
 * row space of A and rank(A) == r.  Without L, (c) and (d) are skipped: a U with rows outside the row space of A passes. ---- */
bool spasm_factorization_verify(const struct spasm_csr *A, const struct spasm_lu *fact, uint64_t seed);

/* ---- spasm_certificate.c: rank certificates (src/SpaSM.jl:345-353, :928-933).  A certificate proves rank(A) >= r to somebody who
 * only has A: r rows i[] and r columns j[] whose r x r submatrix C is non-singular, shown by a vector y with y * C == x for a
 * challenge x the prover cannot choose -- x is drawn from SHA-256(hash, prime, r, i, j) (Fiat-Shamir; `hash` is the 32-byte digest
 * of the matrix file as spasm_triplet_load computes it): if C were singular a random x would lie in its row space with probability
 * <= 1/p -- PER CHALLENGE.  The struct SpaSM.jl mirrors holds one (x, y) pair, so that is all one certificate carries: a prover who
 * may retry (other rows, other columns, another order -- each choice hashes to a new x) gets a singular C accepted after about p
 * attempts, which is cheap for p = 127 or 65521.  The certificate is therefore evidence against ERRORS (a wrong rank out of a faulty
 * run), not against an adversarial prover with a small prime; that needs k challenges with p^k >= 2^64, i.e. another struct.
 * Verification is host-side and O(nnz(A)); together with spasm_factorization_verify (rank(A) <= r) it pins the rank.
 * Creation takes the pivotal rows and the pivot columns of `fact` and solves y * C == x on the device (C is echelonized with L,
 * then spasm_solve).  libspasm's on-disk format is not in the reference tree: save/load use a text format of their own
 * ("spasm-amd rank certificate v1", then r, prime, the hash in hex and r lines "i j x y"). ---- */
struct spasm_rank_certificate {      /* src/SpaSM.jl:345-353 */
    int r;
    i64 prime;
    uint8_t hash[32];
    int *i;                          /* r rows of A */
    int *j;                          /* r columns of A */
    spasm_ZZp *x;                    /* the challenge */
    spasm_ZZp *y;                    /* the response: y * A[i, j] == x */
};
struct spasm_rank_certificate *spasm_certificate_rank_create(const struct spasm_csr *A, const uint8_t *hash, const struct spasm_lu *fact); /* :928 */
bool spasm_certificate_rank_verify(const struct spasm_csr *A, const uint8_t *hash, const struct spasm_rank_certificate *proof);           /* :930 */
void spasm_rank_certificate_save(const struct spasm_rank_certificate *proof, void *file);  /* FILE*, :931 */
bool spasm_rank_certificate_load(void *file, struct spasm_rank_certificate *proof);        /* FILE*, :933; fills a caller-owned struct */
void spasm_rank_certificate_free(struct spasm_rank_certificate *proof);                    /* engine extension: the arrays and the struct */
/* the challenge a certificate with these rows and columns must answer (r balanced residues); engine extension, for verifiers and tests */
void spasm_amd_certificate_challenge(const uint8_t *hash, i64 prime, int r, const int *i, const int *j, spasm_ZZp *x);

/* ---- spasm_solve.c (src/SpaSM.jl:895-923), for a factorization that carries L (echelonize with opts->L; the sparse rounds then
 * keep their multiplier lists and the dense finish is not used).  L is n x r with A[i] == sum_k L[i][k] U[k]; the entry of row
 * p[k] on column k is the pivot U's row k was divided by.
 * spasm_gesv: X (rows of B x rows of A, zero outside the pivotal rows) with X*A == B; ok[k] tells whether row k of B is in the
 *             row space.  Two batched triangular solves on the device (Y*U == B, then X_P*L_P == Y).
 * spasm_solve: the same for one dense vector b (m entries) -> x (n = rows of A entries); false when there is no solution.
 *             NOTE the prototype wrapper allocates x with fact.U.n entries (src/SpaSM.jl:898): bind it with size(fact.L, 1). ---- */
struct spasm_csr *spasm_gesv(const struct spasm_lu *fact, const struct spasm_csr *B, bool *ok);
bool spasm_solve(const struct spasm_lu *fact, const spasm_ZZp *b, spasm_ZZp *x);

/* ---- spasm_ZZp.c surface (commented-out binding at src/SpaSM.jl:65; arithmetic restated :73-88,:383-390) ---- */
void spasm_field_init(i64 p, spasm_field F);

/* ---- spasm_scatter.c / spasm_triangular.c as SpaSM.jl binds them ---- */
void spasm_scatter(const struct spasm_csr *A, int i, spasm_ZZp beta, spasm_ZZp *x);   /* src/SpaSM.jl:620: x += beta * A[i] (host) */
/* src/SpaSM.jl:721, semantics :694-713: solve x * U = B[k]; x (m entries, need not be initialised) receives the solution
 * scattered over the columns, xj[top .. m) its pattern (xj has 3 m entries, zero on entry; only xj[top .. m) is written);
 * with x_b on the pivot columns (qinv[j] >= 0) and x_a on the others, x_b * U + x_a == B[k].  Pivots of U must be 1; they need
 * not be the first entries of their rows.  Returns top (-1 on failure).  One row through the batched device solve
 * (spasm_amd_triangular_solve does all rows of B in one pass). */
int spasm_sparse_triangular_solve(const struct spasm_csr *U, const struct spasm_csr *B, int k, int *xj, spasm_ZZp *x, const int *qinv);

/* ---- spasm_spmv.c as SpaSM.jl binds it (src/SpaSM.jl:640-658: xapy!, axpy!, x * A, A * x) ----
 * Host arrays.  spasm_Axpy: y <- A x + y, x has A->m entries, y has A->n.  spasm_xApy: y <- x A + y, x has A->n entries, y has
 * A->m.  Any int32 in x or y is accepted (reduced like the values of A); on return y holds balanced residues.  On failure (no
 * device, A->x == NULL, out of memory) y is unchanged and spasm_amd_last_error() says why.  Exact, on the device (csrc/spmv.hpp). */
void spasm_Axpy(const struct spasm_csr *A, const spasm_ZZp *x, spasm_ZZp *y);  /* src/SpaSM.jl:656 */
void spasm_xApy(const spasm_ZZp *x, const struct spasm_csr *A, spasm_ZZp *y);  /* src/SpaSM.jl:643 */

/* Engine extension: A resident on the device for repeated products (A may be freed once the operator exists).
 * spasm_amd_spmv_apply: Y <- op(A) X + Y for k vectors at once.  trans = 0: op(A) = A, X is m x k, Y is n x k; trans = 1:
 * op(A) = A^T, i.e. the k products x_i A, X is n x k, Y is m x k.  Row-major, leading dimensions ldx, ldy >= k (in entries).
 * The transpose is built on the device on the first trans = 1 apply and kept.  Returns 0, or -1 with Y unchanged.
 * spasm_amd_spmv_apply_dev: the same on device arrays (X and Y must not overlap); stream NULL: returns when Y is written, else
 * the products are enqueued on that hipStream_t.  One apply at a time per operator. */
typedef struct spasm_amd_spmv spasm_amd_spmv;
spasm_amd_spmv *spasm_amd_spmv_create(const struct spasm_csr *A);
int spasm_amd_spmv_apply(spasm_amd_spmv *op, int trans, int k, const spasm_ZZp *X, i64 ldx, spasm_ZZp *Y, i64 ldy);
int spasm_amd_spmv_apply_dev(spasm_amd_spmv *op, int trans, int k, const spasm_ZZp *X, i64 ldx, spasm_ZZp *Y, i64 ldy, void *stream);
void spasm_amd_spmv_free(spasm_amd_spmv *op);

/* ---- spasm_triangular.c, dense right-hand sides (src/SpaSM.jl:663-692: dense_back_solve, dense_forward_solve) ----
 * Solve x T = b, T n x m.  Participating row i has the pivot column c(i) and the diagonal d(i) = T[i][c(i)]:
 *   forward: c(i) = q[i] (n entries, q[i] < 0: row i does not participate), d(i) must be 1;
 *   back:    c(p[j]) = j for every j with p[j] >= 0 (m entries), d(i) must be non-zero.
 * The pivot graph (edge i -> k when row i has an entry on c(k), k != i) must be acyclic; the rows need not be stored in a
 * triangular order.  x (n entries) is 0 on the rows that do not participate and on the others the unique vector with
 * (x T)[c(k)] = b[c(k)] for every participating k.  On return b holds the residual b - x T (balanced residues); the result is
 * true iff it is zero.  Any int32 in b or x is accepted.  Errors (a NULL argument, a pivot out of range or claimed twice, a
 * non-unit pivot (forward), a zero diagonal (back), a cycle, no device): false, b and x unchanged, spasm_amd_last_error() says
 * why; after a solve the error text is empty whether or not a solution exists.  Exact, on the device (csrc/trsolve.hpp). */
bool spasm_dense_forward_solve(const struct spasm_csr *U, spasm_ZZp *b, spasm_ZZp *x, const int *q);   /* src/SpaSM.jl:691 */
bool spasm_dense_back_solve(const struct spasm_csr *L, spasm_ZZp *b, spasm_ZZp *x, const int *p);      /* src/SpaSM.jl:676 */

/* Engine extension: T resident on the device for repeated solves (T may be freed once the operator exists).
 * spasm_amd_trsolve_create: kind 0 forward (piv = q, n entries), kind 1 back (piv = p, m entries); does every structural check
 * above once (cycle included) and returns NULL with the reason on failure.
 * spasm_amd_trsolve_apply: k systems at once.  B is m x k (right-hand sides in, residuals out), X is n x k, row-major with leading
 * dimensions ldb, ldx >= k; vector v is column v; ok[v] = 1 iff residual v is zero.  Returns 0, or -1 with B and X unchanged.
 * spasm_amd_trsolve_apply_dev: the same on device arrays (ok too), enqueued on the hipStream_t stream (NULL: returns when done).
 * spasm_amd_trsolve_stats: out[8] = n, m, participating rows, levels, wide panels, chunks, kernels of one apply (k <= 64),
 * stored entries.  One apply at a time per operator. */
typedef struct spasm_amd_trsolve spasm_amd_trsolve;
spasm_amd_trsolve *spasm_amd_trsolve_create(const struct spasm_csr *T, const int *piv, int kind);
int spasm_amd_trsolve_apply(spasm_amd_trsolve *op, int k, spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok);
int spasm_amd_trsolve_apply_dev(spasm_amd_trsolve *op, int k, spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok, void *stream);
void spasm_amd_trsolve_stats(const spasm_amd_trsolve *op, i64 *out);
void spasm_amd_trsolve_free(spasm_amd_trsolve *op);

/* ---- spasm_transpose.c ---- */
struct spasm_csr *spasm_transpose(const struct spasm_csr *A);        /* src/SpaSM.jl:589 (one-argument form) */
/* src/SpaSM.jl:597 (submatrix, and the range forms of getindex at :594-603): rows [r0, r1), columns [c0, c1) of A as an
 * (r1 - r0) x (c1 - c0) matrix over the same field, columns renumbered from c0, the entries of each row in their stored order (a
 * copy, no sort); x == NULL when with_values is false.  Host-side, O(entries of the rows), needs no device.  A range that is
 * inverted or leaves the matrix: NULL, spasm_amd_last_error() says why. */
struct spasm_csr *spasm_submatrix(const struct spasm_csr *A, int r0, int r1, int c0, int c1, bool with_values);

/* ---- Engine extension: sparse matrix algebra over GF(p) on the device (csrc/spgemm.hpp) ----
 * What SpaSM.jl offers on CSR through SparseMatrixCSC on the host (src/SpaSM.jl:995-1004: a * b, a + b, a - b, -a, scalar * a) and
 * submatrix, on matrices that stay on the device: spasm_amd_dcsr is an n x m matrix over GF(p) resident there, every operation
 * returns a new handle and leaves its operands as they are, so chains of operations do not cross the host.
 *   upload     A may be freed afterwards; A->x must not be NULL; rows need not be sorted and may hold duplicate columns (they
 *              are summed), explicit zeros and any int32 as a value (reduced like the values of A elsewhere)
 *   download   a host CSR the caller frees with spasm_csr_free
 *   info       out[4] = n, m, stored entries, prime
 *   mul        A (n x k) * B (k x m)
 *   lincomb    a * A + b * B for any i64 a, b (reduced mod p); B == NULL: a * A.  lincomb(1, A, 0, NULL) is the canonical form of A
 *   submatrix  rows [r0, r1), columns [c0, c1), columns renumbered from c0
 *   equal      1 when A and B are the same matrix over the same field (canonical forms are compared; an upload is brought to
 *              canonical form first), 0 when not, < 0 on error
 *   stats      of the operation that made D (all 0 for an upload): out[12] = products (sum over the rows of their bound), entries
 *              written, rows through the tiny / the LDS hash / the global-memory path, chunks of rows, device microseconds of the
 *              size / numeric / compact steps (HIP events), peak scratch bytes, operation (1 mul, 2 lincomb, 3 submatrix),
 *              largest bound of a row
 * CONTRACT of every result (mul, lincomb, submatrix, and the one-shot forms below):
 *   exact          every entry is the true value modulo p as a balanced residue in [mhalfp, halfp], for every prime the engine
 *                  accepts (3 .. 0xFFFFFFFB) and any number of terms per entry
 *   canonical      inside each row the columns ascend, no stored entry is zero (terms that cancel mod p are dropped), and after
 *                  download nzmax == nnz == p[n]
 *   deterministic  two runs give byte-identical p, j, x
 *   errors         a NULL argument, inner dimensions or primes that differ, A->x == NULL, a column index or a range outside the
 *                  matrix, no device ("no HIP device"), out of device memory: NULL (or < 0), operands untouched,
 *                  spasm_amd_last_error() says why; after success the text is empty.
 * One operation at a time per handle as a result; handles may be shared as operands. */
typedef struct spasm_amd_dcsr spasm_amd_dcsr;
spasm_amd_dcsr *spasm_amd_dcsr_upload(const struct spasm_csr *A);
struct spasm_csr *spasm_amd_dcsr_download(const spasm_amd_dcsr *D);
void spasm_amd_dcsr_info(const spasm_amd_dcsr *D, i64 *out);
void spasm_amd_dcsr_free(spasm_amd_dcsr *D);
spasm_amd_dcsr *spasm_amd_dcsr_mul(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B);
spasm_amd_dcsr *spasm_amd_dcsr_lincomb(i64 a, const spasm_amd_dcsr *A, i64 b, const spasm_amd_dcsr *B);
spasm_amd_dcsr *spasm_amd_dcsr_submatrix(const spasm_amd_dcsr *A, int r0, int r1, int c0, int c1);
int spasm_amd_dcsr_equal(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B);
void spasm_amd_dcsr_stats(const spasm_amd_dcsr *D, i64 *out);
/* Structural operations on resident matrices (csrc/reshape.hpp; engine extension): what SpaSM.jl offers on CSR as transpose
 * (src/SpaSM.jl:589), vcat / hcat (:192-193, through the host there) and spasm_permute (:611), for matrices that stay on the device.
 *   transpose  the m x n matrix with entry (j, i) = entry (i, j) of A
 *   permute    p and qinv are HOST arrays of n and m ints, NULL = the identity.  Row i of the result is row p[i] of A, and an entry
 *              on column j of A lands on column qinv[j].  (These are the argument names of spasm_permute(A, p, qinv, with_values);
 *              libspasm's source was not at hand, so the semantics are stated here and the symbol spasm_permute is not claimed.)
 *              Both arrays are checked to be bijections on the host, O(n + m), before anything is launched.
 *   vcat       count >= 1 matrices with equal column counts, rows stacked in the order of the list, in one pass
 *   hcat       count >= 1 matrices with equal row counts, side by side: the columns of D[k] are renumbered from the sum of the
 *              widths before it
 * Every result obeys the CONTRACT above word for word (exact: values are copied, never computed; canonical; deterministic;
 * operands untouched) and is a new handle.  An operand that is not canonical yet (an upload) is first brought to canonical form,
 * as equal does.  Errors -- a NULL argument, count < 1, a NULL element, shapes or primes that differ, p or qinv not a
 * permutation, more than INT_MAX rows or columns in all, no device ("no HIP device"), out of device memory -- return NULL and
 * spasm_amd_last_error() says why.
 * spasm_amd_dcsr_stats of such a result: out[12] = entries moved, the same again, rows ordered by the one-wave / the workgroup /
 * the long-row path (0 where no ordering was needed: vcat, hcat, a permutation of rows alone), 1, device microseconds of the
 * count / move / order steps (HIP events), peak scratch bytes, operation (4 transpose, 5 permute, 6 vcat, 7 hcat), longest row of
 * the result. */
spasm_amd_dcsr *spasm_amd_dcsr_transpose(const spasm_amd_dcsr *A);                       /* m x n */
spasm_amd_dcsr *spasm_amd_dcsr_permute(const spasm_amd_dcsr *A, const int *p, const int *qinv);
spasm_amd_dcsr *spasm_amd_dcsr_vcat(int count, const spasm_amd_dcsr *const *D);          /* rows stacked */
spasm_amd_dcsr *spasm_amd_dcsr_hcat(int count, const spasm_amd_dcsr *const *D);          /* side by side */
/* one-shot forms on host matrices: upload, operate, download */
struct spasm_csr *spasm_amd_csr_mul(const struct spasm_csr *A, const struct spasm_csr *B);
struct spasm_csr *spasm_amd_csr_lincomb(i64 a, const struct spasm_csr *A, i64 b, const struct spasm_csr *B);


/* ---- spasm_echelonize.c / spasm_kernel.c : THE hot path ---- */
void spasm_echelonize_init_opts(struct echelonize_opts *opts);       /* src/SpaSM.jl:817 */
struct spasm_lu *spasm_echelonize(const struct spasm_csr *A, struct echelonize_opts *opts); /* :863 */
struct spasm_csr *spasm_kernel(const struct spasm_lu *fact);         /* src/SpaSM.jl:879 */
/* spasm_rref.c (src/SpaSM.jl:871): the reduced row echelon form of fact->U (r x m; row k = row k of U with its entries on the
 * other pivot columns eliminated, pivot 1 first); Rqinv (m entries, may be NULL) receives the pivot column -> row map.
 * Pivots must be the leftmost entries of their rows (this engine's LUs). */
struct spasm_csr *spasm_rref(const struct spasm_lu *fact, int *Rqinv);

/* ====================================================================================
 * Engine extensions (no reference counterpart): device-resident handles.
 * ==================================================================================== */

/* Per-round record written by the engine (what libspasm prints per round, README.md:19-38). */
struct spasm_amd_round_stats {
    int round;
    int rows_in;          /* rows of the matrix entering the round */
    i64 nnz_in;
    int npiv;             /* structural pivots elected this round */
    int rows_out;         /* non-empty rows of the Schur complement */
    i64 nnz_out;
    i64 nnz_reduced;      /* reference scatter trip count: sum nnz(A_i) + sum over applications nnz(U_r) */
    i64 applications;     /* (row, pivot-row) eliminations performed */
    i64 read_bytes;       /* algorithmic read bytes: 8*nnz_reduced + 16*segments + 4*m */
    double ms_pivots;     /* device time, pivot election + U build */
    double ms_solve;      /* device time, triangular-solve kernel (multipliers) */
    double ms_scatter;    /* device time, scatter/accumulate kernel (Schur rows) */
    double ms_total;
    /* scatter kernels, per size class (one launch each): device time, rows, entries streamed (the row's own
     * entries + the non-pivot part of every applied pivot row) and row segments visited.  Classes 0..6: LDS hash
     * tables of 256..16384 slots, 7: the global-memory last resort, 8..14: the streaming twins of 0..6 (rows whose
     * entries are written out directly; a row with too many duplicate columns is redone by its hash class) */
    double ms_class[16];
    int rows_class[16];
    i64 ent_class[16];
    i64 seg_class[16];
    i64 stream_fix;       /* duplicate columns the streaming kernels merged after the fact */
    i64 stream_redo;      /* rows the streaming kernels handed back to the hash-table kernels */
    /* per-round setup, wall time with its host synchronisations: ms_uinv = Uinv = (I + U_PP)^-1 (rounds that keep to the
     * multiplier lists; 0 when the round goes along W); ms_w = the levels of the pivot graph + sizing + the first build of W
     * (included in ms_pivots of an echelonize round; a plan pays them when it is created, and rebuilds W in every run: ms_wbuild) */
    double ms_uinv;
    double ms_w;
    i64 npiv_open;        /* of npiv: pivots the "Faugere-Lachartre on columns" search added to the leftmost-entry ones
                           * (echelonize rounds with enable_greedy_pivot_search; 0 for plans, which keep to leftmost entries) */
    /* W = -(I + U_PP)^-1 U_PN as the Schur step builds it, level by level of the pivot graph (csrc/wlevel.hpp): device time of
     * the build inside the last plan run (it is part of every run), levels, entries of W, rows left to the workgroup kernel */
    double ms_wbuild;
    i64 w_levels;
    i64 w_entries;
    i64 w_long_rows;
    i64 npiv_greedy;      /* of npiv: pivots the greedy cycle-free search added (reference README.md:23; csrc/greedy.hpp) */
    /* reserved, always 0 (the seven fields of a removed Schur kernel; they keep the layout of the struct) */
    double ms_fused;
    double ms_fused_fix;
    i64 rows_fused;
    i64 ent_fused;
    i64 seg_fused;
    i64 rows_rejected;
    i64 s_entries_used;
    double ms_levels;     /* the levels of the pivot graph (relaxation + sort), once per round: part of ms_w */
    double ms_w_sizing;   /* of ms_w: the device-memory query and the allocation of the buffers of the W build (wall time) */
};

typedef struct spasm_amd_schur_plan spasm_amd_schur_plan;

/* Last error text of the calling thread ("" if none). Engine calls return NULL / nonzero on failure. */
const char *spasm_amd_last_error(void);

/* Number of HIP devices visible; <= 0 when there is none (the hot path then fails loudly). */
int spasm_amd_device_count(void);
int spasm_amd_set_device(int dev);

/* Deterministic synthetic CSR (host memory, caller frees with spasm_csr_free):
 *   kind 0: every entry present with probability `density` (BASELINE config 2)
 *   kind 1: exactly `row_nnz` distinct uniform columns per row (BASELINE configs 3/4)
 *   kind 2: Macaulay-like, rows are translates of n/2500 base patterns of 10..row_nnz terms (BASELINE config 5)
 * values uniform on the nonzero balanced residues; columns unsorted. */
struct spasm_csr *spasm_amd_synth_csr(int kind, int n, int m, double density, int row_nnz,
                                      i64 prime, uint64_t seed);

/* Build a device-resident plan for ONE Schur round of A (BASELINE config 3):
 * uploads rows [row_lo,row_hi) of A as this device's shard, elects the Faugere-Lachartre
 * pivots of the WHOLE matrix (so that every shard sees the same U), builds U on the device.
 * Returns NULL on failure. */
spasm_amd_schur_plan *spasm_amd_schur_plan_create(const struct spasm_csr *A, int row_lo, int row_hi);
/* Same with the plan's rows taken as row_lo, row_lo + stride, ... < row_hi.  Strided shards (rank r of G: row_lo = r,
 * stride = G) are balanced; contiguous blocks are not when the election's tie-break puts the pivots in the first rows. */
spasm_amd_schur_plan *spasm_amd_schur_plan_create_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride);
/* Run the round once on `stream` (a hipStream_t, NULL = default): solve + scatter kernels.
 * Returns 0 on success. Safe to call repeatedly (outputs are overwritten). */
int spasm_amd_schur_plan_run(spasm_amd_schur_plan *plan, void *stream);
/* Per-class event pairs around the scatter launches (stats->ms_class) are recorded when `on` (default); they cost a
 * few microseconds of launch gap each, so throughput runs switch them off and profile one extra run with them on. */
void spasm_amd_schur_plan_class_timing(spasm_amd_schur_plan *plan, int on);
/* Block until the plan's last run has finished and fill `stats` (counters + event timings). */
int spasm_amd_schur_plan_stats(spasm_amd_schur_plan *plan, struct spasm_amd_round_stats *stats);
/* Copy the Schur complement of the last run back to host CSR (n_shard_nonpivot x m). p_out (may be
 * NULL) receives, per output row, the index of the originating row of A. */
struct spasm_csr *spasm_amd_schur_plan_fetch(spasm_amd_schur_plan *plan, int *p_out);
/* The pivot rows of the plan's round as they enter U (scaled to a unit pivot, reference src/SpaSM.jl:712), in pivot-index order
 * (= ascending pivot column for a plan); pivcol_out / row_out (npiv ints each, may be NULL) receive the pivot column and the originating
 * row of A of each.  What a row-sharded echelonization appends to U after every exchange, without rebuilding it on the host. */
struct spasm_csr *spasm_amd_schur_plan_fetch_U(spasm_amd_schur_plan *plan, int *pivcol_out, int *row_out);
void spasm_amd_schur_plan_free(spasm_amd_schur_plan *plan);

/* ---- row-sharded round with an exchange of the pivot rows (one process per GPU; the collectives are the
 * caller's: torch.distributed / RCCL all-reduce(MIN) on the keys, all-gather on the exported rows) ----
 * All `*_dev` arguments are DEVICE pointers owned by the caller.
 *   1. shard_create   uploads rows [row_lo,row_hi) of A only
 *   2. shard_elect    writes this shard's election keys, one i64 per column: (row length << 32 | global row),
 *                     INT64_MAX where the shard proposes nothing            -> caller: all-reduce(MIN)
 *   3. shard_set_keys takes the reduced keys, numbers the pivots; returns npiv (< 0 on error) and reports
 *                     how many pivot rows / entries this shard owns         -> caller: all-gather of the counts
 *   4. shard_export   packs the owned pivot rows: hdr_dev[2*k] = pivot index, hdr_dev[2*k+1] = length;
 *                     ent_dev = their {col,val} pairs back to back          -> caller: all-gather (variable length)
 *   5. shard_import   takes the concatenation over ranks (any order of parts), builds U; then plan_run /
 *                     plan_stats / plan_fetch work on the returned plan for this shard's non-pivot rows. */
typedef struct spasm_amd_shard spasm_amd_shard;
spasm_amd_shard *spasm_amd_shard_create(const struct spasm_csr *A, int row_lo, int row_hi);
spasm_amd_shard *spasm_amd_shard_create_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride);
int spasm_amd_shard_elect(spasm_amd_shard *sh, int64_t *keys_dev);
int spasm_amd_shard_set_keys(spasm_amd_shard *sh, const int64_t *keys_dev, int *n_owned, i64 *nnz_owned);
/* r04: shard_set_keys in two halves with "Faugere-Lachartre on columns" (enable_greedy_pivot_search, src/SpaSM.jl:326; README.md:23)
 * between them -- the search of the single-device round over ROW SHARDS: shard_assign numbers the leftmost pivots (returns how many);
 * shard_open_step runs one step of the search on this shard's rows: `in_dev` is the array the step before left, REDUCED over the
 * shards by the caller, `out_dev` receives the array this step leaves (m elements) for the caller to reduce --
 *   step 0 BEGIN -> closed (int32, MAX) | 1 HIST (in: closed) -> colcnt (int32, SUM) | 2 PROPOSE (in: colcnt) -> best2 (int64, MIN)
 *   3 ACCEPT (in: best2) -> newflag (int32, MAX) | 4 RECORD (in: newflag; pass = 1..4) -> closed (int32, MAX), returns the pivots the
 *   pass accepted (0: the search is over) | 5 FINISH: renumbers, returns the pivots the search added
 * (steps 1-4 once per pass, at most four passes: four m-word reductions per pass); shard_finish_keys then does the rest of
 * shard_set_keys (the shard's non-pivot rows, the pivot rows it owns).  < 0 on error. */
int spasm_amd_shard_assign(spasm_amd_shard *sh, const int64_t *keys_dev);
int spasm_amd_shard_open_step(spasm_amd_shard *sh, int step, int pass, const void *in_dev, void *out_dev);
int spasm_amd_shard_finish_keys(spasm_amd_shard *sh, int *n_owned, i64 *nnz_owned);
int spasm_amd_shard_export(spasm_amd_shard *sh, int *hdr_dev, int *ent_dev);
spasm_amd_schur_plan *spasm_amd_shard_import(spasm_amd_shard *sh, int n_rows, i64 n_entries, const int *hdr_dev, const int *ent_dev);
/* X * U = B for every row of B in one device pass: what SpaSM.jl's sparse_triangular_solve(U, B, qinv) / `B / LU`
 * (src/SpaSM.jl:733-755) obtains by looping spasm_sparse_triangular_solve over the rows of B.  Semantics of :694-713: with x_b on
 * the pivot columns and x_a on the others, x_b * U + x_a == B[k]; X (rows of B x rows of U) holds x_b indexed by the row of U;
 * ok[k] = 1 when x_a is empty, i.e. X[k] * U == B[k].  U needs unit pivots that are the leftmost entries of their rows. */
struct spasm_csr *spasm_amd_triangular_solve(const struct spasm_csr *U, const int *qinv, const struct spasm_csr *B, unsigned char *ok);
/* The kernel step of a multi-GPU run: the kernel vectors of the free columns number first, first + step, ... only (free
 * columns counted in ascending order; vector f of spasm_kernel(fact) is row (f - first) / step here). */
struct spasm_csr *spasm_amd_kernel_strided(const struct spasm_lu *fact, int first, int step);
/* Multi-round sharded echelonization (spasm.jl_amd/sharded.py: echelonize_sharded): the Schur rows of a sharded plan become the
 * shard's matrix of the next round, on the device, under the same numbering (local row i = original row lo + i * stride; this
 * round's pivot rows and empty rows are empty rows).  Runs the plan if it has not run; CONSUMES the plan (also on failure the
 * caller must not use it again); rows_out / nnz_out: non-empty rows and entries of the new matrix. */
spasm_amd_shard *spasm_amd_schur_plan_advance(spasm_amd_schur_plan *plan, int *rows_out, i64 *nnz_out);
/* the shard's current rows as a host CSR with one row per local row (empty ones included); free with spasm_csr_free */
struct spasm_csr *spasm_amd_shard_fetch(spasm_amd_shard *sh);
void spasm_amd_shard_free(spasm_amd_shard *sh);

/* spasm_echelonize over several devices of THIS process: `nshards` row shards (shard s: rows s, s + nshards, ...; device s modulo
 * the number of visible devices, so nshards = 8 on an 8-GPU node puts one shard on each), per round an election (per-column minimum
 * of the shards' keys), an exchange of the elected pivot rows (peer copies over xGMI) and the local Schur complement of every shard's
 * rows.  A remainder that is dense (or a round whose Schur complement is estimated dense: spasm_schur_estimate_density /
 * spasm_schur_dense, reference src/SpaSM.jl:763-766) is finished by ALL shards together for primes below 2^16 (csrc/dense_multi.hpp:
 * the rows stay where they are, per panel of 64 columns the candidates' panel entries go to shard 0 and the elected pivot rows to every
 * shard); a small or sparse remainder, and larger primes, by the single-device engine on device 0.  Leftmost-entry pivots throughout, so rank, pivot columns and kernel
 * equal those of spasm_echelonize with enable_greedy_pivot_search = 0 whatever nshards is.  What spasm.jl_amd/sharded.py does with
 * one process per GPU and RCCL, behind one call for hosts without torch.distributed (the Julia side: one more @ccall). */
struct spasm_lu *spasm_amd_echelonize_multi(const struct spasm_csr *A, struct echelonize_opts *opts, int nshards);
/* ---- the dense finish over row shards with ONE PROCESS PER SHARD (spasm.jl_amd/sharded.py; csrc/dense_multi.hpp states the
 * protocol).  The steps are the engine's, the exchanges between them the caller's collectives; `*_dev` are DEVICE pointers of the caller.
 *   shard_import_U      as spasm_amd_shard_import, but stops after U is built (no W / Uinv, no dry run)
 *   schur_plan_prepare  .. which this catches up on when the round stays sparse after all
 *   dshard_open         the columns this shard's Schur rows of the round can touch, as flags          -> dshard_flags -> all-reduce(MAX)
 *   dshard_density      takes the reduced flags (all shards then number the columns alike), estimates the density of the round's
 *                       Schur complement on 64 columns (spasm_schur_estimate_density); C_out = columns of the dense matrix
 *   dshard_build        this shard's Schur rows straight into its dense matrix (spasm_schur_dense), guest rows behind them
 *   per block of KB columns: dshard_block_begin; per panel of 64 (q-th of the block, columns c0 .. c0 + w):
 *     dshard_candidates   the rows this shard's own elimination of the panel elects, cand_bytes bytes   -> all-gather
 *     dshard_elect        the panel's pivots among the candidates of all shards (every rank runs it: same result); npp pivots,
 *                         cnt[k] / first[k]: how many shard k owns and the guest slot of its first
 *     dshard_pack         this shard's winners: cnt rows of (ldc - c0) elements, then nd planes of cnt x KB bytes -> one broadcast per owner
 *     dshard_unpack       an owner's buffer into the guest rows (also the owner's own)
 *     dshard_apply        the panel: elimination by the now known pivots, triangular solve of the pivot rows, update inside the block
 *   dshard_block_end(b0, b1, panels); after the last block dshard_finish = pivots found by all shards together (< 0: error), and
 *   dshard_fetch_U = the rows of U this shard owns (pivcol_out / row_out: C ints each, n_out of them used). */
typedef struct spasm_amd_dshard spasm_amd_dshard;
spasm_amd_schur_plan *spasm_amd_shard_import_U(spasm_amd_shard *sh, int n_rows, i64 n_entries, const int *hdr_dev, const int *ent_dev);
int spasm_amd_schur_plan_prepare(spasm_amd_schur_plan *plan);
spasm_amd_dshard *spasm_amd_dshard_open(spasm_amd_schur_plan *plan, int me, int nshards);
/* r04: the same finish over the shard's CURRENT rows (a remainder that is dense already; no round, no U): _flags / _density (returns 1.0)
 * / _build and the panel steps as after spasm_amd_dshard_open.  The shard stays the caller's. */
spasm_amd_dshard *spasm_amd_dshard_open_rows(spasm_amd_shard *sh, int me, int nshards);
int spasm_amd_dshard_flags(spasm_amd_dshard *ds, int *flags_dev);
double spasm_amd_dshard_density(spasm_amd_dshard *ds, const int *flags_dev, int free_cols, int *C_out);
int spasm_amd_dshard_build(spasm_amd_dshard *ds);
int spasm_amd_dshard_info(spasm_amd_dshard *ds, int *C_out, int *KB, i64 *ldc, int *elem, int *nd, int *cand_bytes);
int spasm_amd_dshard_block_begin(spasm_amd_dshard *ds);
int spasm_amd_dshard_candidates(spasm_amd_dshard *ds, int c0, int w, void *cand_dev);
int spasm_amd_dshard_elect(spasm_amd_dshard *ds, const void *stack_dev, int w, int *npp, int *cnt, int *first);
i64 spasm_amd_dshard_pack(spasm_amd_dshard *ds, int c0, void *buf_dev);
int spasm_amd_dshard_unpack(spasm_amd_dshard *ds, int q, int c0, int owner, const void *buf_dev);
int spasm_amd_dshard_apply(spasm_amd_dshard *ds, int q, int c0, int w, int b1);
int spasm_amd_dshard_block_end(spasm_amd_dshard *ds, int b0, int b1, int npan);
int spasm_amd_dshard_finish(spasm_amd_dshard *ds);
struct spasm_csr *spasm_amd_dshard_fetch_U(spasm_amd_dshard *ds, int *pivcol_out, int *row_out, int *n_out);
void spasm_amd_dshard_close(spasm_amd_dshard *ds);

/* How the most recent spasm_amd_echelonize_multi of this thread finished: 0 = remainder gathered to device 0 (or nothing left),
 * 1 = a round's Schur complement straight to dense on all shards, 2 = the dense remainder on all shards. */
int spasm_amd_multi_last_finish(void);

/* rank(A) = rank(echelonize(A)) (reference src/SpaSM.jl:1149) without materialising U on the host: the pivot rows are counted where
 * they are found.  For matrices whose U outgrows the host (BASELINE config 5: 10^10 entries and more above 1/3 scale).  Same
 * options as spasm_echelonize (L excluded); -1 on error. */
i64 spasm_amd_rank(const struct spasm_csr *A, struct echelonize_opts *opts);

/* ---- Engine extension: many small matrices in one call (csrc/batch.hpp) ----
 * spasm_echelonize pays a fixed cost per call (upload, planning of the rounds, dozens of launches, several synchronisations) that
 * dwarfs the work on a matrix of a few dozen rows.  These entries take `count` matrices A[0 .. count) at once; the matrices of one
 * batch may differ in shape and in prime.
 *   LDS path      a matrix with values, n * m <= 32768 (and opts == NULL or opts->L == 0) is eliminated by ONE workgroup in a dense
 *                 image held in LDS, all such matrices of the batch in a constant number of launches per chunk (a chunk = as many
 *                 matrices as fit the scratch budget, a third of the free device memory; SPASM_AMD_BATCH_SCRATCH_MB lowers it);
 *                 one upload of the matrices and one of their descriptors per call; per chunk one download, preceded by the
 *                 8-byte read of its size
 *   general path  every other matrix of the batch goes through spasm_echelonize / spasm_kernel as they are, one at a time;
 *                 its result is what the per-matrix call returns under `opts`
 *   echelonize    out[i] is an ordinary spasm_lu (free it with spasm_lu_free).  From the LDS path: r, U r x m with the pivot 1 as the
 *                 leftmost entry of its row and the columns ascending inside each row, qinv, p (the elected rows in election order,
 *                 then the others ascending), L == NULL, complete == false; U is the REDUCED row echelon form, and row k holds the
 *                 k-th pivot column.  spasm_kernel, spasm_rref, spasm_gesv, spasm_solve, spasm_factorization_verify and
 *                 spasm_certificate_rank_create take it like any other LU.
 *   options       the LDS path always elects the canonical pivot columns (those leftmost-entry pivots give: the pivot of a column
 *                 is the first row, not yet a pivot, that holds it), so the pivot-search options (enable_greedy_pivot_search,
 *                 enable_tall_and_skinny, enable_dense, enable_GPLU, min_pivot_proportion, max_round, sparsity_threshold, ...)
 *                 have NO EFFECT there; rank and row space are those of spasm_echelonize under any options
 *   kernel        K[i] = the vectors spasm_kernel returns for that LU (vector of the free column f: -1 on f, R[a][f] on the pivot
 *                 column of row a of the reduced form), in ascending order of their free column, columns ascending inside a vector
 *   rank          rank[i] only; nothing but the ranks is downloaded
 *   stats         of the last batch call of this thread: out[8] = matrices, matrices through the LDS path, matrices through the
 *                 general path, chunks, kernel launches of the LDS path (eliminations, scans, packs), device microseconds of the LDS
 *                 path (HIP events), entries written by the LDS path, largest image in 32-bit words
 *   exact         for every prime the engine accepts (3 .. 0xFFFFFFFB); values of A may be any int32 (reduced on load); a row must
 *                 not hold a column twice
 *   deterministic two runs give byte-identical results
 *   errors        count < 0, a NULL array, a NULL matrix, A[i]->x == NULL, a malformed matrix, a column index outside the matrix, no
 *                 device ("no HIP device"), out of memory: -1, NO output slot is written, spasm_amd_last_error() names the cause and
 *                 the index of the matrix.  count == 0 succeeds (and needs no device).  After success the error text is empty. */
int spasm_amd_echelonize_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, struct spasm_lu **out);
int spasm_amd_rank_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, i64 *rank);
int spasm_amd_kernel_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, struct spasm_csr **K);
void spasm_amd_batch_stats(i64 *out);   /* of the last batch call of this thread */

/* ---- Engine extension: a matrix split into its blocks on the device (csrc/blocks.hpp) ----
 * The blocks of A are the connected components of its row/column graph: vertices are the rows and the columns, every STORED entry
 * (i, j) joins row i and column j whatever its value (an explicit zero joins; a repeated (i, j) is harmless for the split).  This is
 * Block(A) of the reference (src/blocks.jl:35-105), computed on the device: a union-find forest with the rule "the larger root goes
 * under the smaller" gives the components, a stable sort by block number the maps, one copy the blocks.  The handle keeps them as one
 * concatenated device CSR in the layout the batch entries above read, so the three consumers below start from the descriptors.
 *   numbering     blocks in ascending order of their smallest vertex, rows before columns; an empty row is a 1 x 0 block, an empty
 *                 column a 0 x 1 block.  Inside a block the rows and the columns keep their ascending order in A, and the entries of
 *                 a row keep A's order.  row_pos / col_pos are 0-based positions inside the block.
 *   create        uploads A (values as they are: any int32) and splits it.  create_dcsr does the same from a resident matrix without
 *                 an upload, on that matrix's device; the values are the balanced residues the resident matrix holds.
 *   info          out[11] = blocks, n, m, entries, rows / columns / entries of the block with most entries, blocks without entries,
 *                 device microseconds of the components, of the numbering, of the split (HIP events)
 *   shapes        rows[b], cols[b], nnz[b] for the nblocks blocks; any pointer may be NULL
 *   maps          row_block[n], row_pos[n], col_block[m], col_pos[m], block_rows[n] (the rows of A block after block; those of block b
 *                 at row_start[b] .. row_start[b + 1]), row_start[nblocks + 1], block_cols[m], col_start[nblocks + 1]; any may be NULL
 *   fetch         block b as an ordinary spasm_csr over A's prime (free it with spasm_csr_free)
 *   rank, echelonize, kernel
 *                 rank[b], out[b], K[b] for the nblocks blocks: exactly what spasm_amd_rank_batch / _echelonize_batch / _kernel_batch
 *                 return for the list of fetched blocks under the same opts -- the same kernel on the same input -- except that no
 *                 entry of a block inside the LDS limit is downloaded or uploaded on the way.  Blocks over the limit, and every block
 *                 when opts->L is set, are fetched and take the general path.  A block without entries needs no launch.
 *                 spasm_amd_batch_stats describes the call (such a block counts with the LDS path).
 *   deterministic the components do not depend on how the races of the union-find resolve (csrc/blocks.hpp gives the argument): two
 *                 handles of one matrix hold byte-identical maps and blocks
 *   errors        a NULL argument, A->x == NULL, a prime outside 3 .. 0xFFFFFFFB, malformed row pointers ("row pointers must not
 *                 decrease"), a column index outside the matrix, n + m >= 2^31, a working set that does not fit the free device memory,
 *                 no device, a block index out of range: NULL / -1, nothing is written to the output arrays, spasm_amd_last_error()
 *                 names the cause.  spasm_amd_blocks_free(NULL) is a no-op.  A handle belongs to one process. */
typedef struct spasm_amd_blocks spasm_amd_blocks;
spasm_amd_blocks *spasm_amd_blocks_create(const struct spasm_csr *A);
spasm_amd_blocks *spasm_amd_blocks_create_dcsr(const spasm_amd_dcsr *D);
void spasm_amd_blocks_info(const spasm_amd_blocks *B, i64 *out);
int spasm_amd_blocks_shapes(const spasm_amd_blocks *B, int *rows, int *cols, i64 *nnz);
int spasm_amd_blocks_maps(const spasm_amd_blocks *B, int *row_block, int *row_pos, int *col_block, int *col_pos, int *block_rows, i64 *row_start,
                          int *block_cols, i64 *col_start);
struct spasm_csr *spasm_amd_blocks_fetch(const spasm_amd_blocks *B, int b);
int spasm_amd_blocks_rank(spasm_amd_blocks *B, struct echelonize_opts *opts, i64 *rank);
int spasm_amd_blocks_echelonize(spasm_amd_blocks *B, struct echelonize_opts *opts, struct spasm_lu **out);
int spasm_amd_blocks_kernel(spasm_amd_blocks *B, struct echelonize_opts *opts, struct spasm_csr **K);
void spasm_amd_blocks_free(spasm_amd_blocks *B);

/* ---- Engine extension: X * A = B for many small matrices, and block by block (csrc/solve_batch.hpp) ----
 * spasm_gesv / spasm_solve need a factorization that carries L, which the LDS path of the batch does not produce, and the general
 * path costs milliseconds per matrix.  These entries solve X[i] * A[i] = B[i] for `count` systems at once; the systems of one call
 * may differ in shape and in prime.  A[i] is n_i x m_i, B[i] is K_i x m_i over the same prime (K_i may be 0, rows of B[i] may be
 * empty), X[i] is K_i x n_i (free it with spasm_csr_free) and ok[i] points to K_i bytes.
 *   LDS path      a system with m * (n + 1) <= 32768 is solved by workgroups that hold the transposed image of A, augmented by a
 *                 slab of right-hand sides, in LDS, and eliminate it with the election rule of the batch.  A system with more
 *                 right-hand sides than its class holds is cut into slabs, one workgroup each; the result does not depend on where
 *                 the slabs are cut.  Chunks, uploads and downloads as for the batch entries above.
 *                   ok[i][k] = 1 iff B[i][k] lies in the row space of A[i]
 *                   ok = 1:  X[i][k] is the UNIQUE solution of x * A[i] = B[i][k] that is zero outside the CANONICAL ROW BASIS of
 *                            A[i]: row j of A[i] belongs to that basis iff it is not a combination of rows 0 .. j-1
 *                   ok = 0:  X[i][k] is an empty row
 *                 X is canonical in the sense of the dcsr contract: columns ascending inside a row, no stored zero, balanced
 *                 residues, nzmax == nnz == p[n].  Two runs are byte-identical.
 *   shapes        n = 0: ok[i][k] = 1 iff the row of B is zero mod p; m = 0: every ok = 1; X has no entries.  Neither needs a
 *                 launch (nor K = 0); such systems count with the LDS path.
 *   input         values of A and B may be any int32 (reduced on load); rows need not be sorted; a row must not hold a column
 *                 twice; an explicit zero is allowed
 *   general path  a system over the limit goes through spasm_echelonize with L set and spasm_gesv as they are.  ok has the same
 *                 meaning and X[i][k] * A[i] == B[i][k], but the support of X is that factorization's pivotal rows: the
 *                 canonical-basis guarantee DOES NOT HOLD there.  (Rows without a solution are empty, columns ascend, no stored zero.)
 *   blocks_solve  X * A = Rhs for the matrix A the handle was split from: Rhs is K x m over the handle's prime, X is K x n, ok has K
 *                 bytes.  The entries of Rhs are dealt to the blocks by col_block / col_pos on the device (Rhs is uploaded once); block
 *                 b receives, as right-hand sides, the rows of Rhs that hold an entry in its columns.  Blocks inside the limit are
 *                 solved from the resident concatenated CSR: no entry of such a block crosses the bus.  Blocks over the limit are
 *                 fetched and take the general path.  An entry of Rhs that is non-zero mod p on an empty column of A (a 0 x 1
 *                 block) makes its row unsolvable.  ok[k] is the AND over the blocks; X[k] places each block's solution on the block's
 *                 rows (block_rows), columns ascending, and is an empty row when ok[k] = 0.  X is put together on the device.
 *                 The components of A span disjoint column sets, so the union of the blocks' canonical bases is the canonical basis
 *                 of A: whenever A as a whole is inside the limit, blocks_solve returns BYTE FOR BYTE what spasm_amd_solve_batch
 *                 returns for (A, Rhs) as one system.
 *   stats         of the last solve call of this thread: out[8] = systems (blocks_solve: the blocks that received a right-hand side),
 *                 systems through the LDS path, systems through the general path, jobs (matrix-slab workgroups), kernel launches of
 *                 the LDS path (eliminations, scans, packs), device microseconds of the LDS path (HIP events; blocks_solve: the split
 *                 of Rhs, the eliminations and the assembly of X), entries of X written by the LDS path (blocks_solve: entries of X),
 *                 right-hand-side rows without a solution
 *   errors        count < 0, a NULL array, a NULL matrix, x == NULL in a matrix, primes of A[i] and B[i] that differ, B[i]->m !=
 *                 A[i]->m, a column index outside the matrix, malformed row pointers, no device ("no HIP device"), out of memory; for
 *                 blocks_solve also a NULL handle, Rhs->m != m of the handle, a prime that differs from the handle's: -1, NO output
 *                 slot is written (neither X nor ok), spasm_amd_last_error() names the function, the cause and the index of the
 *                 matrix.  count == 0 succeeds (and needs no device).  After success the error text is empty. */
int spasm_amd_solve_batch(int count, const struct spasm_csr *const *A, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok);
int spasm_amd_blocks_solve(spasm_amd_blocks *Bk, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok);
void spasm_amd_solve_stats(i64 *out);   /* of the last solve call of this thread */

/* ---- Engine extension: X * A = B with A factored once (csrc/solver.hpp) ----
 * spasm_amd_solve_batch and spasm_amd_blocks_solve eliminate A on every call.  A solver handle eliminates every system once and
 * keeps, per system of the LDS path, an operator of m * rank words on the device; an apply only multiplies the entries of a
 * right-hand side on the pivot columns of A into it.  Create once, apply many times (like spasm_amd_spmv_* / spasm_amd_trsolve_*).
 *   create        `count` systems A[i] (n_i x m_i; shapes and primes may differ).  The matrices may be dropped afterwards.
 *   create_blocks one system per block of the split, built from the handle's resident concatenated CSR (only a block over the limit
 *                 is fetched).  The solver copies the maps it needs: the blocks handle may be freed afterwards.
 *   apply         B[i] is K_i x m_i over the prime of A[i]; X[i] (K_i x n_i, free it with spasm_csr_free) and ok[i] (K_i bytes) as
 *                 for spasm_amd_solve_batch.  The input, output, ok, shape and error rules of spasm_amd_solve_batch apply word for
 *                 word, and for every system of the LDS path (m * (n + 1) <= 32768) apply returns BYTE FOR BYTE what
 *                 spasm_amd_solve_batch returns for the same (A, B): the unique solution that is zero outside the CANONICAL ROW BASIS
 *                 of A[i], an empty row where ok = 0.  Two applies of the same input are byte-identical, and an apply leaves the
 *                 handle as it was.
 *   apply_blocks  Rhs, X and ok as for spasm_amd_blocks_solve, whose rules apply word for word; returns BYTE FOR BYTE what
 *                 spasm_amd_blocks_solve returns whenever no block that meets Rhs is over the limit.
 *   general path  a system over the limit keeps its factorization with L (spasm_echelonize, once, at create); apply runs spasm_gesv
 *                 on it.  X * A == B and ok as on the LDS path, but the canonical-basis guarantee DOES NOT HOLD there.
 *   shapes        n = 0, m = 0 and rank 0 need no launch at create, and none at apply beyond the test that the row of B vanishes.
 *   info          out[8] = systems, systems on the LDS path (empty shapes included), systems on the general path, operator words
 *                 (sum of m * rank over the LDS path; the buffer has room for min(n, m) columns per system), sum of the ranks,
 *                 factor jobs (system-slab workgroups of create), kernel launches of create, device microseconds of create (HIP
 *                 events).
 *   ranks         rank[i] = rank of system i (count words)
 *   basis         rows[0 .. r) = the canonical row basis of system i, ascending: the rows of A[i] every solution lives on.  rows has
 *                 room for n_i ints; returns r, -1 on error.  For a system of the general path these are that factorization's
 *                 pivotal rows, ascending, NOT the canonical basis.
 *   stats         of the last apply of this thread, in the layout of spasm_amd_solve_stats
 *   use           one apply at a time per handle; a handle belongs to the device it was created on
 *   errors        as for spasm_amd_solve_batch / spasm_amd_blocks_solve (the prime and m of B[i] are checked against A[i]'s), and:
 *                 a NULL handle; apply on a handle made by create_blocks, apply_blocks on one made by create; a system index out of
 *                 range.  create returns NULL, the others -1; NO output slot is written; spasm_amd_last_error() names the function,
 *                 the cause and the index of the matrix; the handle stays usable.  count == 0 succeeds at create and at apply (and
 *                 needs no device).  spasm_amd_solver_free(NULL) is harmless. */
typedef struct spasm_amd_solver spasm_amd_solver;
spasm_amd_solver *spasm_amd_solver_create(int count, const struct spasm_csr *const *A);
spasm_amd_solver *spasm_amd_solver_create_blocks(const spasm_amd_blocks *Bk);
int spasm_amd_solver_apply(spasm_amd_solver *S, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok);
int spasm_amd_solver_apply_blocks(spasm_amd_solver *S, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok);
void spasm_amd_solver_info(const spasm_amd_solver *S, i64 *out);
int spasm_amd_solver_ranks(const spasm_amd_solver *S, i64 *rank);
int spasm_amd_solver_basis(const spasm_amd_solver *S, int i, int *rows);
void spasm_amd_solver_stats(i64 *out);   /* of the last apply of this thread */
void spasm_amd_solver_free(spasm_amd_solver *S);

/* ---- Engine extension: the resident solver against dense right-hand sides that stay on the device (csrc/solver.hpp) ----
 * spasm_amd_solver_apply takes and returns host CSR; this apply takes the right-hand sides as the COLUMNS of a dense row-major
 * array and returns the solutions as columns, the layout of spasm_amd_spmv_apply_dev and spasm_amd_trsolve_apply_dev, so that a
 * loop (solve, form the residual with the resident product, solve again) runs on one stream without a right-hand side on the host.
 *   matrix        one per handle.  A handle of create_blocks: A, the matrix that was split (N = its rows, M = its columns), ok has
 *                 K bytes.  A handle of create: diag(A_0 .. A_{count-1}), N = sum n_i, M = sum m_i; system i owns rows
 *                 sum_{j<i} m_j .. of B and rows sum_{j<i} n_j .. of X; ok has count * K bytes, ok[i * K + v]; every system
 *                 reduces by its own prime.
 *   B, X          B is M x K with leading dimension ldb >= K, X is N x K with ldx >= K, int32; right-hand side v is column v of B
 *                 and its solution column v of X: X[:, v]^T * A == B[:, v]^T.  Any int32 is accepted in B and reduced on load.
 *   result        column v of X, restricted to a system, is entry for entry the dense image of the row spasm_amd_solver_apply /
 *                 _apply_blocks return for the same right-hand side: the unique solution that is zero outside the canonical row
 *                 basis, as balanced residues; all zero where ok = 0.  X is overwritten in its whole N x K window; the words
 *                 outside it (ldx > K) and all of B are left as they were.
 *   apply_dense   host arrays: upload, apply_dense_dev on the NULL stream, download.
 *   _dev          device pointers for B, X and ok.  stream NULL: returns when X and ok are written; otherwise everything is
 *                 enqueued on that hipStream_t and the call does not wait for it.  The job plan of the most recent K is kept in
 *                 the handle: a second apply with the same K uploads and allocates nothing.  An apply with another K rebuilds
 *                 the plan and, before it does, WAITS FOR THE DEVICE (hipDeviceSynchronize), so that applies enqueued earlier
 *                 end on the plan they began with: applies of different K may follow each other on a stream without a
 *                 synchronise by the caller, at the price of that wait; a loop that alternates between two K pays it at every
 *                 call.  STREAM CAPTURE: an apply with the K of the plan only enqueues on `stream`; one that would
 *                 have to rebuild the plan while `stream` is capturing is refused with -1 before anything is touched, and the
 *                 capture stays valid: apply once with that K before the capture begins.
 *   general path  a handle with a system over the limit of the LDS path is REFUSED (the factorization of such a system lives on
 *                 the host and is not applied to dense device arrays): -1, nothing written, the error names the first such
 *                 system.  dense_info out[3] tells beforehand.
 *   dense_info    out[8] = N, M, rows of ok (count, or 1 for a handle of create_blocks), systems on the general path, K of the
 *                 cached plan (0: none), jobs (system-slab workgroups) of that plan, kernel launches of one apply with that plan,
 *                 plans built so far.
 *   use           one host thread at a time per handle, as for the other applies.  Applies enqueued on ONE stream need nothing
 *                 more.  Applies of a create_blocks handle enqueued on different streams share the flag words of the plan: the
 *                 caller orders them (an event, or a synchronise).
 *   errors        a NULL handle; K < 0; ldb < K or ldx < K; a NULL B, X or ok with K > 0 and a non-empty shape; B and X that
 *                 overlap (windows that share a word, tested row by row: two windows side by side in one array, which
 *                 interleave without sharing one, are accepted); a plan to rebuild on a capturing stream; no device.  -1, no output word written, spasm_amd_last_error() names the function and the cause, the
 *                 handle stays usable; after success the error text is empty.  K == 0 succeeds (also on a handle with a system
 *                 of the general path: there is nothing to refuse), and so does a handle of zero systems for any K; neither
 *                 needs a device or writes anything.  The create_blocks handle of a matrix without rows and columns has no
 *                 system either, but its ok has K bytes: they are set to 1 (apply_dense does that on the host and needs no
 *                 device; apply_dense_dev is given a device pointer and writes it there). */
int spasm_amd_solver_apply_dense(spasm_amd_solver *S, int K, const spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok);
int spasm_amd_solver_apply_dense_dev(spasm_amd_solver *S, int K, const spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok, void *stream);
void spasm_amd_solver_dense_info(const spasm_amd_solver *S, i64 *out);

/* Per-round records of the most recent spasm_echelonize call on this thread. */
int spasm_amd_last_rounds(struct spasm_amd_round_stats *out, int max_rounds);

/* The dense eliminations of the most recent spasm_echelonize call on this thread (read-only counters; all zero when the call never
 * reached a dense finish).  out[8] = eliminations run; of the LAST one: its kind (1 = int8 matrix cores, one base-256 digit, p < 2^8;
 * 2 = int8, two digits, p < 2^16; 3 = f64 panels, p <= 2^24 or forced; 4 = rank-1 updates, p > 2^24), rows, columns, block width
 * (columns updated at once: the int8 block; 64 for the f64 panels; 1 for the rank-1 updates); tall-and-skinny finishes; panels of
 * the tall panel kernel redone in place; spare.  out == NULL is ignored. */
void spasm_amd_dense_stats(i64 *out);

/* The device's field arithmetic (csrc/zp.hpp, the restatement of spasm_ZZp.c as SpaSM.jl gives it, src/SpaSM.jl:383-390) on n
 * test vectors: a, b, c are balanced residues; out receives 8 ints per vector: a*b, a*b+c, a+b, a-b, -a, a^-1 (0 for a = 0),
 * a*b through the scatter kernels' lazy product + short reduction, 64*a*b through a lazy accumulator + the same reduction.
 * Returns 0 on success. */
int spasm_amd_zp_probe(i64 prime, int n, const int *a, const int *b, const int *c, int *out);

/* The lazy accumulators of the sparse kernels over their domain: for each of n triples, count[i] >= 0 copies of the lazy product
 * a[i] * b[i] are summed in the accumulator type the kernels use for this prime (i32 for p < 2^16, i64 above) and reduced as the
 * kernels reduce a table slot; out[i] receives the balanced residue of count[i] * a[i] * b[i] as long as
 * count[i] * (p/2 + 256) < 2^31 and count[i] <= 2^20 (p < 2^16; no limit above).  Returns 0 on success; without a device
 * ("no HIP device") or with bad arguments 1, and out is not written. */
int spasm_amd_zp_sum_probe(i64 prime, int n, const int *a, const int *b, const int *count, int *out);

/* The primitives of csrc/zp.hpp one at a time, on chosen arguments (tests/test_gpu_zp.py, tests/test_zp_host.py).  All return 0 on
 * success and 1 on an error; the entries that run on the device fail without one ("no HIP device") and write nothing then.
 *   zp_reduce_probe        out[i] = zp_reduce(x[i]), the balanced residue of an i64 with |x| <= min(3 * 2^51 * p, 2^62) (the domain the
 *                          header of zp.hpp derives).  where = 0: the host compilation of the function in a plain loop, no device
 *                          needed; where = 1: one lane per value on the device.
 *   zp_field_probe_host    the first six results of spasm_amd_zp_probe (a*b, a*b+c, a+b, a-b, -a, a^-1 with 0 for a = 0), 6 ints per
 *                          vector, from the host compilation: no device needed; the device's six must be the same bits.
 *   zp_lazy_probe          out[i] = the raw, unreduced lazy product of a[i] and b[i] as the accumulators take it (i32 for p < 2^16,
 *                          widened; i64 above): congruent to a*b, |out| <= p/2 + 256 for p < 2^16 and <= 0.51 p above.
 *   zp_small_lazy_probe    p < 2^16 only: out[i] = the raw one-step reduction zp_small_lazy(x[i]) of an i32 with |x| <= 2^30 and
 *                          |x / p| < 2^22, which the lazy product applies to x = a * b.
 *   zp_small_lazy_scan     p < 2^16 only: the same function at EVERY x of [x_lo, x_hi] (same domain), in chunks of `chunk`
 *                          consecutive values, chunk k starting at x_lo + k * chunk and the last one cut at x_hi: tmax[k] and tmin[k]
 *                          receive the chunk's largest and smallest result, bad[k] its number of results not congruent to x mod p (by
 *                          integer remainder).  The three arrays have (x_hi - x_lo) / chunk + 1 entries, at most 2^24. */
int spasm_amd_zp_reduce_probe(i64 prime, int where, int n, const i64 *x, int *out);
int spasm_amd_zp_field_probe_host(i64 prime, int n, const int *a, const int *b, const int *c, int *out);
int spasm_amd_zp_lazy_probe(i64 prime, int n, const int *a, const int *b, i64 *out);
int spasm_amd_zp_small_lazy_probe(i64 prime, int n, const int *x, int *out);
int spasm_amd_zp_small_lazy_scan(i64 prime, i64 x_lo, i64 x_hi, int chunk, int *tmax, int *tmin, int *bad);

/* ---- Engine extension: determinants mod p (csrc/det.hpp) ----
 * The elimination computes every pivot and then keeps only their number; these entries return the determinant of a square matrix
 * as a balanced residue, at the three scales of the engine: many small matrices in one call, a split matrix block by block, a
 * whole matrix.  The matrices of one batch may differ in size and in prime.
 *   LDS path      a matrix with n * n <= 32768 (n <= 181) is eliminated by ONE workgroup in LDS, as spasm_amd_rank_batch does it;
 *                 det = sgn(k -> row of the k-th pivot) * product of the pivots, the product taken over the inverses the
 *                 elimination keeps and inverted once.  All such matrices of a call in at most four launches; one int per matrix
 *                 comes back.
 *   general path  every other matrix goes through spasm_echelonize with L, one at a time: 0 when the rank is below n, otherwise
 *                 sgn(p) * sgn(pivot columns) * product of the diagonal of L; the two parities are counted on the host.
 *   det_batch     det[i] for A[0 .. count)
 *   blocks_det    the matrix behind the handle: when a block is not square (a row or a column without entry is such a block) the
 *                 determinant is 0 and nothing is eliminated; otherwise it is the product of the blocks' determinants, the blocks
 *                 inside the LDS limit straight from the handle, the others fetched and sent through the general path, times the
 *                 parities of the row and of the column permutation that bring A to block-diagonal form.  Those are counted on the
 *                 host from row_block / row_pos / col_block / col_pos: 16 bytes per row are downloaded (not when the product is 0).
 *   det           spasm_amd_blocks_create + blocks_det; dcsr_det: spasm_amd_blocks_create_dcsr + blocks_det on the resident
 *                 matrix's device, no entry crosses the host
 *   values        any int32 is accepted and reduced on load; a row must not hold a column twice.  The determinant of the 0 x 0
 *                 matrix is 1.
 *   stats         of the last det call of this thread: out[8] = matrices (det_batch) or blocks, of them through the LDS path,
 *                 through the general path, blocks that make the determinant 0 by their shape, launches of the LDS path, its
 *                 device microseconds (HIP events), host microseconds spent on parities (the download of the maps included), 0.
 *                 The split of det / dcsr_det is not part of them.
 *   deterministic two runs give the same values
 *   errors        count < 0, a NULL array or result pointer, a NULL matrix or handle, A->x == NULL, a malformed matrix, a prime
 *                 outside 3 .. 0xFFFFFFFB, a column index outside the matrix, a matrix that is not square ("matrix 3: not square
 *                 (3 x 2)"), no device ("no HIP device"), out of memory: -1, NO output slot is written, spasm_amd_last_error()
 *                 names the cause (and the index of the matrix).  All but the last two are found before a device is looked for.
 *                 count == 0 succeeds (and needs no device).  After success the error text is empty. */
int spasm_amd_det_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *det);
int spasm_amd_det(const struct spasm_csr *A, spasm_ZZp *det);
int spasm_amd_blocks_det(spasm_amd_blocks *B, spasm_ZZp *det);
int spasm_amd_dcsr_det(const spasm_amd_dcsr *D, spasm_ZZp *det);
void spasm_amd_det_stats(i64 *out);   /* of the last det call of this thread */

/* ---- Engine extension: characteristic polynomials mod p (csrc/charpoly.hpp) ----
 * chi_A(x) = det(x * I - A) of a square matrix: monic of degree n, returned as n + 1 balanced residues, low degree first, the last
 * one 1 (the 0 x 0 matrix: {1}).  The matrix is brought to upper Hessenberg form by similarity (first non-zero below the diagonal
 * as pivot, row operations followed by the inverse column operations) and chi is read off by the recurrence over the leading
 * principal minors.  Field operations only: every prime 2 < p <= 0xFFFFFFFB works, p <= n included.  The matrices of one batch may
 * differ in size and in prime.
 *   LDS path      a matrix with n * n <= 32768 (n <= 181) is ONE workgroup in LDS, classed and launched like spasm_amd_rank_batch;
 *                 all such matrices of a call in at most four launches
 *   global path   a larger matrix, n <= 1024, is one workgroup of 512 on a dense image of its own in device memory (4 MiB at most),
 *                 all of them in one launch: exact, not fast.  There is no multi-workgroup reduction for large n and no split by
 *                 components.
 *   charpoly_batch  coef[i][0 .. A[i]->n] for A[0 .. count); every coef[i] has room for A[i]->n + 1 words, owned by the caller
 *   charpoly        one matrix; dcsr_charpoly: a resident matrix, on its device, no entry crosses the host
 *   values        any int32 is accepted and reduced on load; a row must not hold a column twice
 *   stats         of the last charpoly call of this thread: out[8] = matrices, of them through the LDS path, through the global
 *                 path, launches, device microseconds of the LDS path (HIP events), of the global path, 0, 0
 *   deterministic two runs give the same values
 *   errors        count < 0, a NULL array, a NULL matrix, A->x == NULL, a malformed matrix, a prime outside 3 .. 0xFFFFFFFB, a
 *                 column index outside the matrix, a matrix that is not square ("matrix 3: not square (3 x 2)"), a NULL coef[i],
 *                 n > 1024 ("matrix 3: characteristic polynomial limited to n <= 1024 (n = 1025)"), no device ("no HIP device"),
 *                 out of memory: -1, NO output slot is written, spasm_amd_last_error() names the cause (and the index of the
 *                 matrix).  All but the last two are found before a device is looked for.  count == 0 succeeds (and needs no
 *                 device).  After success the error text is empty. */
int spasm_amd_charpoly_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *const *coef);
int spasm_amd_charpoly(const struct spasm_csr *A, spasm_ZZp *coef);
int spasm_amd_dcsr_charpoly(const spasm_amd_dcsr *D, spasm_ZZp *coef);
void spasm_amd_charpoly_stats(i64 *out);   /* of the last charpoly call of this thread */

/* ---- Engine extension: characteristic polynomials by components (csrc/blocks.hpp, csrc/polyprod.hpp) ----
 * The split of spasm_amd_blocks_create pairs rows with columns freely: rank and determinant (up to sign) survive it, the spectrum
 * does not.  The INDEX split takes row i and column i as one vertex: the graph of spasm_amd_blocks_create (every stored entry
 * (i, j), explicit zeros included, joins row i and column j) plus the edge row i - column i for every i.  Its components are sets
 * S_b of indices, A is diag(A[S_0,S_0], A[S_1,S_1], ..) up to a simultaneous permutation of rows and columns, and
 * chi_A = prod_b chi_{A[S_b,S_b]}.
 *   create_index  same arguments and handle type as spasm_amd_blocks_create / _create_dcsr; n == m is required ("not square
 *                 (3 x 2)", found before a device is looked for).  Every block is square; block_rows and block_cols hold the same
 *                 indices block for block; row_pos[i] == col_pos[i] and row_block[i] == col_block[i]; blocks ascend by smallest
 *                 index; there is no 1 x 0 or 0 x 1 block (an index with neither row nor column entries is a 1 x 1 zero block);
 *                 two handles of one matrix are byte-identical.  An index handle is an ordinary handle: rank, echelonize, kernel,
 *                 solve, det, fetch, maps, shapes and spasm_amd_solver_create_blocks work on it unchanged (for det the two
 *                 parities coincide).
 *   is_index      1 for such a handle, 0 for a handle of spasm_amd_blocks_create / _create_dcsr, -1 for NULL
 *   poly_product  out[0 .. sum(len) - count] = the product of `count` polynomials mod prime as balanced residues, low degree
 *                 first.  Polynomial k is len[k] >= 1 words f[k][..]; any int32 is reduced on load; it need not be monic and a
 *                 zero leading word is allowed.  count == 0 gives {1} (and needs no device).  A product tree on the device:
 *                 ceil(log2 count) levels, one launch each, every term reduced (no lazy accumulator: every accepted prime works).
 *   blocks_charpoly_factors
 *                 coef[n + nblocks]: the polynomial of block b (rows_b + 1 words, monic) at row_start[b] + b
 *   blocks_charpoly
 *                 coef[n + 1] = chi_A.  The blocks go to the kernels of spasm_amd_charpoly_batch straight from the handle (LDS path
 *                 for rows^2 <= 32768, global path up to 1024 rows, one launch); the factors are multiplied on the device; only
 *                 the result is downloaded.  n == 0 gives {1} with no launch.
 *   charpoly_split, dcsr_charpoly_split
 *                 create_index followed by blocks_charpoly; the resident matrix on its device, no entry crosses the host.  Unlike
 *                 spasm_amd_charpoly there is no limit on n, only on the rows of a block.
 *   stats         of the last call of this thread: out[8] = blocks, of them on the LDS path, on the global path, launches of the
 *                 charpoly kernels, their device microseconds (HIP events), product levels, product device microseconds, 0.  The
 *                 split's own time is in spasm_amd_blocks_info.
 *   deterministic two runs give the same values
 *   errors        poly_product: count < 0, a NULL array, a NULL f[k] ("polynomial 3: NULL array"), len[k] < 1, a prime outside
 *                 3 .. 0xFFFFFFFB, a total length >= 2^31, no device, out of memory.  charpoly: a NULL handle, a NULL coef, a handle
 *                 that is not an index split ("spasm_amd_blocks_charpoly: the handle is not an index split
 *                 (spasm_amd_blocks_create_index)"), a block with more than 1024 rows ("block 3: characteristic polynomial limited
 *                 to n <= 1024 (n = 1025)"): both found from the handle before any elimination.  -1 (NULL for the creators), NO
 *                 output word is written, spasm_amd_last_error() names the cause and the index.  All but "no device" and "out of
 *                 memory" are found before a device is looked for. */
spasm_amd_blocks *spasm_amd_blocks_create_index(const struct spasm_csr *A);
spasm_amd_blocks *spasm_amd_blocks_create_index_dcsr(const spasm_amd_dcsr *D);
int spasm_amd_blocks_is_index(const spasm_amd_blocks *B);
int spasm_amd_poly_product(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out);
int spasm_amd_blocks_charpoly(spasm_amd_blocks *B, spasm_ZZp *coef);
int spasm_amd_blocks_charpoly_factors(spasm_amd_blocks *B, spasm_ZZp *coef);
int spasm_amd_charpoly_split(const struct spasm_csr *A, spasm_ZZp *coef);
int spasm_amd_dcsr_charpoly_split(const spasm_amd_dcsr *D, spasm_ZZp *coef);
void spasm_amd_charpoly_split_stats(i64 *out);   /* of the last split charpoly call of this thread */

/* ---- Engine extension: minimal polynomials mod p of sparse matrices by Wiedemann's method (csrc/krylov.hpp) ----
 * The black-box route: no elimination and no fill-in, memory O(nnz + n * K), no limit on n below 2^24.  The Krylov sequence
 * s_i = u^T A^i v of the resident exact product is projected on the device, its shortest linear recurrence is found by
 * Berlekamp-Massey on the device, and the lcm over K projections is taken on the host.
 *   krylov_sequence  op is a resident operator of a SQUARE n x n matrix ("not square (3 x 2)" otherwise), 1 <= K <= 64, U and V are
 *                 row-major n x K with leading dimensions ldu, ldv >= K (the layout of spasm_amd_spmv_apply; any int32 is reduced
 *                 where it is read), S is len x K, packed:  S[i * K + c] = sum_r U[r, c] * (A^i V)[r, c]  for 0 <= i < len, as
 *                 balanced residues; trans = 1 uses A^T.  V and U are not modified.  len == 0 succeeds and writes nothing.  Per
 *                 step one launch per non-empty row class of the operator (plus the combine when there are long rows): the step
 *                 writes A X into one of two buffers of the operator and folds the projection into the same launch as an exact
 *                 64-bit integer sum (|sum| < 2^62), so the result does not depend on scheduling and two runs give the same bytes.
 *   krylov_sequence_dev  the same on device arrays, enqueued on the hipStream_t stream without any host synchronization (NULL:
 *                 returns when S is written).  One sequence at a time per operator.
 *   berlekamp_massey  `count` sequences of `len` terms in one launch, one workgroup each: sequence c is S[c], S[lds + c], ..
 *                 (column c of a row-major len x lds HOST array, lds >= count; any int32 is reduced on load).  coef is count x ldc
 *                 with ldc >= len + 1: row c receives the monic f(x) = x^L * C(1 / x) of the shortest recurrence
 *                 sum_j C[j] * s[i - j] = 0 (C[0] = 1, L <= len), low degree first, deg[c] + 1 words with deg[c] = L, and the rest
 *                 of the row is zeroed.  The zero sequence gives {1}; 1, 0, 0, 0 gives x.  where = 0 chooses the class by size:
 *                 the two polynomials live in LDS while 2 * (len + 1) words fit 158 KiB (len <= 20223), else in device memory
 *                 (exact, not fast); 1 forces the LDS class ("the LDS class does not fit (len = .., at most 20223)" when it does
 *                 not); 2 forces the device-memory class.  Both classes give the same bytes.  Field operations only: every prime
 *                 2 < p <= 0xFFFFFFFB works.  count == 0 succeeds and needs no device.
 *   poly_lcm      the monic lcm of `count` polynomials mod prime (polynomial k is len[k] >= 1 words f[k][..], any int32, a zero
 *                 leading word allowed, not the zero polynomial) by Euclid on the host in exact arithmetic: *outlen words are written
 *                 to out (balanced residues, low degree first, the last one 1), which must hold sum(len) - count + 1 words.
 *                 count == 0 gives {1}.  Needs no device.
 *   minpoly_vectors  the vectors minpoly uses when U == V == NULL, as n x K packed arrays (either may be NULL): word (t, r, c), t = 0
 *                 for U and 1 for V, is w mod p as a balanced residue, w the splitmix64 output of the state
 *                 seed + 0x9E3779B97F4A7C15 * (2 * (r * K + c) + t + 1)  (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *                 z *= 0x94D049BB133111EB; z ^= z >> 31; all mod 2^64).  The same seed gives the same bytes.  Needs no device.
 *   minpoly, spmv_minpoly, dcsr_minpoly
 *                 A host matrix, a resident operator, a resident matrix (on its device; no entry crosses the host).  K == 0 means
 *                 8, maxdeg <= 0 (or > n) means n.  U and V are packed n x K host arrays or both NULL (minpoly_vectors(seed)).
 *                 coef must hold maxdeg + 1 words; *deg + 1 of them are written.  The sequence has 2 * maxdeg terms when
 *                 maxdeg = n, and 2 * maxdeg + 2 when maxdeg < n: 2 * maxdeg terms fix a recurrence of degree <= maxdeg but
 *                 cannot show that the bound was too small (Berlekamp-Massey returns L = maxdeg on them whatever the true degree);
 *                 with two more terms a larger degree shows as L > maxdeg and the call fails with "degree bound too small".
 *                 n == 0 gives {1} and needs no device.
 *   CONTRACT      the result is monic and ALWAYS divides the minimal polynomial of A; it equals it with a probability that grows
 *                 with p and K (a projection misses a factor with probability about deg / p; small primes want a larger K and
 *                 still may miss).  If x divides the result (coef[0] == 0), A is singular: that is certain.  If *deg == n, the
 *                 result is the characteristic polynomial of A.  A result of lower degree says nothing certain about rank.
 *   stats         of the last of these calls of this thread: out[8] = n, K, steps (products with A), launches, Berlekamp-Massey
 *                 class (1 LDS, 2 device memory), degree of the result, device microseconds of the sequence and of
 *                 Berlekamp-Massey (HIP events; 0 for krylov_sequence_dev).  Every call clears what it does not fill.
 *   deterministic two runs give the same bytes
 *   errors        a NULL operator / matrix / array, a matrix that is not square, K outside 1 .. 64 (0 .. 64 for minpoly:
 *                 "K out of range"), ldu or ldv < K, lds < count, "ldc < len + 1", only one of U and V given, a prime outside
 *                 3 .. 0xFFFFFFFB, n >= 2^24, no device ("no HIP device"), out of memory: -1, NO output word is written,
 *                 spasm_amd_last_error() names the cause.  All but the last two are found before a device is looked for (for a
 *                 host matrix and for berlekamp_massey; an operator or a resident matrix has one already). */
int spasm_amd_krylov_sequence(spasm_amd_spmv *op, int trans, int K, int len, const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S);
int spasm_amd_krylov_sequence_dev(spasm_amd_spmv *op, int trans, int K, int len, const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv,
                                  spasm_ZZp *S, void *stream);
int spasm_amd_berlekamp_massey(int count, int len, const spasm_ZZp *S, i64 lds, i64 prime, int where, spasm_ZZp *coef, i64 ldc, int *deg);
int spasm_amd_poly_lcm(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out, int *outlen);
int spasm_amd_minpoly_vectors(int n, int K, uint64_t seed, i64 prime, spasm_ZZp *U, spasm_ZZp *V);
int spasm_amd_minpoly(const struct spasm_csr *A, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);
int spasm_amd_spmv_minpoly(spasm_amd_spmv *op, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);
int spasm_amd_dcsr_minpoly(const spasm_amd_dcsr *D, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);
void spasm_amd_minpoly_stats(i64 *out);   /* of the last Krylov / Berlekamp-Massey / minpoly call of this thread */

/* ---- Engine extension: polynomials of A applied to vectors, and sparse solves mod p without fill-in by Wiedemann's method
 *      (csrc/horner.hpp) ----
 * The solve that stays in O(nnz + n * K) memory: no elimination, no limit on n below 2^24.  One Horner step per product,
 * Y <- op(A) X + c * B, on the row classes of the resident operator; the solve certifies every answer on the device.
 *   poly_apply    op is a resident operator of a SQUARE n x n matrix ("not square (3 x 2)" otherwise), 1 <= K <= 64.
 *                 X[:, c] <- f_c(op(A)) * V[:, c] with f_c = coef[c * ldc + 0 .. deg[c]], low degree first (any int32 is reduced on
 *                 load; deg[c] = -1 is the zero polynomial; ldc >= max(deg) + 1); trans = 1 uses A^T.  deg and coef are HOST arrays.
 *                 V and X are row-major n x K host arrays with leading dimensions ldv, ldx >= K (the layout of
 *                 spasm_amd_krylov_sequence; any int32 in V is reduced where it is read); V must not overlap X and is not
 *                 modified.  Columns of lower degree are zero-padded at the top of the schedule, so the call makes max(deg) products
 *                 with A, each one launch per non-empty row class of the operator (plus the combine when there are long rows),
 *                 after one elementwise launch for the leading coefficients.  The results are balanced residues.
 *   poly_apply_dev  the same with V and X on the device, enqueued on the hipStream_t stream without any host synchronization
 *                 (NULL: the default stream, and no synchronization either).  The coefficient table is uploaded once per call.
 *                 One call at a time per operator: it uses the operator's two Krylov buffers.
 *   wiedemann_solve, spmv_wiedemann_solve, dcsr_wiedemann_solve
 *                 A host matrix, a resident operator, a resident matrix (on its device).  trans = 0 solves A x = b, trans = 1
 *                 solves x A = b (the orientation of the library's gesv).  B and X are n x K row-major HOST arrays (ldb, ldx >= K),
 *                 status has K words, 1 <= K <= 64.  Column c is independent of the others:
 *                   1. the sequence s_i = u_c^T op(A)^i b_c is projected (2 * maxdeg terms when maxdeg = n, 2 * maxdeg + 2 when
 *                      maxdeg < n; maxdeg <= 0 or > n means n; a degree above maxdeg is refused with "degree bound too small", as
 *                      in minpoly).  u_c is column c of U (packed n x K) when U is given, else column c of the U of
 *                      minpoly_vectors(n, K, seed + t) on try t: a column's result depends only on (A, b_c, u_c);
 *                   2. Berlekamp-Massey gives its polynomial f_c;
 *                   3. with q_c = (f_c - f_c(0)) / x, one Horner run gives x_c = -q_c(op(A)) b_c / f_c(0) when f_c(0) != 0, and
 *                      z_c = q_c(op(A)) b_c when f_c(0) == 0;
 *                   4. one more step R <- op(A) X + r B (r_c = -1 or 0) with the non-zero counts of R and X certifies the column.
 *                 status[c] = 1  solved: f_c(0) != 0 and R_c == 0, so op(A) x_c = b_c holds (b_c = 0 gives x_c = 0);
 *                 status[c] = 2  kernel vector: f_c(0) == 0, R_c == 0 and X_c != 0, so X_c is a non-zero vector with
 *                                op(A) X_c = 0 and A is singular: that is certain; it says nothing about whether b_c is in the image;
 *                 status[c] = 0  undecided after every try (the projection lost a factor each time): column c of X is zero.
 *                 Undecided columns are packed into a narrower array and tried again with the next seed, `tries` tries in all
 *                 (tries <= 0 means 3; one try only when U is given).  A status is never 1 or 2 without the device check having
 *                 passed.  The return value is 0 when the call ran, whatever the statuses.  n == 0: every status is 1, no device.
 *   stats         of the last of these calls of this thread: out[10] = n, K, tries used, products with A (sequences + Horner +
 *                 checks), launches, largest degree of an f_c, columns solved, columns with a kernel vector, device microseconds
 *                 of the sequences + Berlekamp-Massey and of Horner + checks (HIP events).  poly_apply fills n, K, products,
 *                 launches.  Every call clears what it does not fill.
 *   deterministic two runs give the same bytes (the counts are integer sums)
 *   errors        a NULL operator / matrix / array, a matrix that is not square, K outside 1 .. 64 ("K out of range"), "ldb < K",
 *                 "ldx < K", "ldv < K", "polynomial 2: ldc < deg + 1 ..", "polynomial 2: a degree below -1 (-2)", "V must not
 *                 overlap X", a prime outside 3 .. 0xFFFFFFFB, n >= 2^24, "degree bound too small", no device ("no HIP device"),
 *                 out of memory: -1, NO output word is written, spasm_amd_last_error() names the cause.  The argument errors are
 *                 found before a device is looked for (for a host matrix; an operator or a resident matrix has one already). */
int spasm_amd_poly_apply(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv,
                         spasm_ZZp *X, i64 ldx);
int spasm_amd_poly_apply_dev(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv,
                             spasm_ZZp *X, i64 ldx, void *stream);
int spasm_amd_wiedemann_solve(const struct spasm_csr *A, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                              const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);
int spasm_amd_spmv_wiedemann_solve(spasm_amd_spmv *op, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                                   const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);
int spasm_amd_dcsr_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                                   const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);
void spasm_amd_wiedemann_stats(i64 *out);   /* of the last poly_apply / Wiedemann solve call of this thread */

/* ---- Engine extension: rank and determinant mod p without fill-in by preconditioned Wiedemann (csrc/precond.hpp) ----
 * A rank and a determinant that use no elimination kernel: memory O(nnz + (n + m) * K), n, m < 2^24.  A is n x m (n rows).  With
 * random diagonals D2 (n x n) and E = D1^2 (m x m), all entries non-zero, B = E A^T D2 A is m x m; for a square A, B = D A.  The
 * projected sequence of B comes from the resident product with the diagonal scale folded into the step's launch, its recurrences
 * from Berlekamp-Massey on the device, the lcm f over the K projections and the split f = x^e g, g(0) != 0, from the host.
 *   CONTRACT      rank: the result deg g is a lower bound, always: deg g <= rank(A) whatever p, K and the seed (f divides the
 *                 minimal polynomial of B; B is invertible on im B^e by Fitting's decomposition, so deg g <= dim im B^e <=
 *                 rank(B) <= rank(A)).  deg g = rank(A) is likely, with a probability that grows with p (the published bound
 *                 wants p >> n^2; over GF(3) the bound falls short often) and never certain, except that *certain = 1 when the
 *                 result equals min(n, m).  det: status 1 is certain: either deg f = n, then f is the characteristic polynomial
 *                 of D A and det A = (-1)^n f(0) / prod d_i, or x divides f, then A is singular and det A = 0.  status 0 says
 *                 nothing (the value is 0 then).
 *   precond_diagonal  the diagonals of try seed.  The words of one diagonal differ from each other as long as that is possible
 *                 (the first p - 1 of them), so that D I = D has a minimal polynomial of full degree whenever n < p: word
 *                 (which, i), 0 <= i < len, is 1 + P_b(i mod N) with N = p - 1, b = i div N and P_b a pseudo-random permutation
 *                 of 0 .. N - 1: split x into two halves of h = ceil(bits(N - 1) / 2) bits (h >= 1), x = L * 2^h + R, and run
 *                 four Feistel rounds r = 0 .. 3, (L, R) <- (R, L xor (w & (2^h - 1))), w the splitmix64 output (the mixer
 *                 of minpoly_vectors) of the state
 *                   seed + 0x9E3779B97F4A7C15 * ((which + 1) * 2^60 + b * 2^20 + r * 2^16 + R)  mod 2^64;
 *                 x <- L * 2^h + R, and the four rounds are repeated on x while x >= N.  which = 0 is D2 (and the D of the
 *                 determinant), which = 1 is E: the SQUARE mod p of that word (its words may repeat: w and p - w share a
 *                 square).  Every word lies in 1 .. p - 1 and is returned as a balanced residue.  The states differ from those
 *                 of minpoly_vectors, whose indices 2 * (r * K + c) + t + 1 stay below 2^32.  The same seed gives the same
 *                 bytes.  Needs no device.
 *   precond_sequence  op is a resident operator; d_left, d_right, U, V, S are HOST arrays (any int32 is reduced where it is read).
 *                 mode 0: op is square, S[i * K + c] = sum_r U[r, c] * ((D A)^i V)[r, c] with D = diag(d_left) (n words; d_right
 *                 is not read); one launch set per step.  mode 1: S[i * K + c] = sum_r U[r, c] * ((E A^T D2 A)^i V)[r, c] with
 *                 D2 = diag(d_left) (n words), E = diag(d_right) (m words); U and V are m x K (ldu, ldv >= K); two launch sets
 *                 per step, on the two views of the operator.  0 <= i < len, balanced residues, 1 <= K <= 64.  len == 0 writes
 *                 nothing; an operator without rows or columns needs no launch.
 *   wiedemann_rank, spmv_wiedemann_rank, dcsr_wiedemann_rank
 *                 A host matrix, a resident operator, a resident matrix (on its device; its transpose is made on the device
 *                 and lives for the call).  K == 0 means 8, tries <= 0 means 3, maxdeg <= 0 (or > min(n, m)) means min(n, m).
 *                 Try t uses U, V = minpoly_vectors(m, K, seed + t) and precond_diagonal(n, seed + t, 0), (m, seed + t, 1), and
 *                 runs 2 * maxdeg + 2 terms, that is 2 * (2 * maxdeg + 1) products with A -- not 2 * maxdeg terms as minpoly:
 *                 B may have a nilpotent part, whose factor x takes f one degree beyond deg g (deg f <= min(n, m) + 1 always,
 *                 because B = P Q with P m x n, Q n x m: its minimal polynomial divides x times that of Q P).  *rank is the largest deg g over the tries; the tries stop
 *                 once it reaches min(n, m).  A projection or an lcm with deg g > maxdeg is refused ("degree bound too
 *                 small").  n == 0 or m == 0: rank 0, certain 1, no device.
 *   wiedemann_det, spmv_wiedemann_det, dcsr_wiedemann_det
 *                 A must be square.  Try t runs the 2 * n terms (2 * n - 1 products) of D A with D = precond_diagonal(n,
 *                 seed + t, 0) and U, V = minpoly_vectors(n, K, seed + t); the first try with deg f = n or f(0) = 0 ends the
 *                 call with *status = 1; after the last try *status = 0 and *det = 0.  prod d_i and its inverse are exact host
 *                 arithmetic.  The empty matrix has determinant 1, status 1, and needs no device.
 *   stats         of the last of these calls of this thread: out[10] = n, m, K, tries used, products with A (per try
 *                 2 * (2 * maxdeg + 1) for rank, 2 * n - 1 for det; (len - 1) * (1 + mode) for precond_sequence), launches,
 *                 degree of f, multiplicity of x in f (of the try that set the result), device microseconds of the sequences
 *                 and of Berlekamp-Massey (HIP events).  Every call clears what it does not fill.
 *   deterministic two runs give the same bytes
 *   errors        a NULL operator / matrix / array, a matrix that is not square (det, mode 0: "not square (3 x 2)"), K outside
 *                 0 .. 64 (1 .. 64 for precond_sequence: "K out of range"), mode or which outside 0 .. 1, ldu or ldv < K, a
 *                 prime outside 3 .. 0xFFFFFFFB, n or m >= 2^24, "degree bound too small", no device ("no HIP device"), out of
 *                 memory: -1, NO output word is written, spasm_amd_last_error() names the cause.  The argument errors are found
 *                 before a device is looked for (for a host matrix; an operator or a resident matrix has one already). */
int spasm_amd_precond_diagonal(int len, uint64_t seed, int which, i64 prime, spasm_ZZp *d);
int spasm_amd_precond_sequence(spasm_amd_spmv *op, int mode, int K, int len, const spasm_ZZp *d_left, const spasm_ZZp *d_right,
                               const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S);
int spasm_amd_wiedemann_rank(const struct spasm_csr *A, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);
int spasm_amd_spmv_wiedemann_rank(spasm_amd_spmv *op, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);
int spasm_amd_dcsr_wiedemann_rank(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);
int spasm_amd_wiedemann_det(const struct spasm_csr *A, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);
int spasm_amd_spmv_wiedemann_det(spasm_amd_spmv *op, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);
int spasm_amd_dcsr_wiedemann_det(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);
void spasm_amd_precond_stats(i64 *out);   /* of the last preconditioned Wiedemann call of this thread */

/* ---- block Wiedemann: block Krylov sequences, Berlekamp-Massey over matrix sequences, determinant (engine extension; DESIGN
 *      section 27; csrc/block_krylov.hpp, csrc/block_bm.hpp) ----
 * A block projection U^T M^i V with U, V of b columns carries in about 2 n / b terms what the scalar routines above read off 2 n
 * terms.  b is 2, 4, 8 or 16.
 *   block_sequence    op is a resident SQUARE operator; d_left (n words or NULL), U, V (n x b, ldu, ldv >= b) and S are HOST arrays,
 *                 any int32 is reduced where it is read.  S[(i * b + r) * b + c] = sum_k U[k, r] * (M^i V)[k, c] mod p for
 *                 0 <= i < len, balanced residues, with M = A (trans 0), A^T (trans 1), and D A or D A^T when d_left is given,
 *                 D = diag(d_left), every word non-zero mod p.  One launch set per step (the step kernels of the resident
 *                 product with a b x b projection as epilogue), no host synchronization inside the run.  The diagonal of a
 *                 term is the K = b term of krylov_sequence for the same U, V.
 *   block_sequence_dev  the same on DEVICE arrays of the operator's device (S: len * b * b words), enqueued on stream (NULL: the
 *                 null stream, and the call waits); d_left is not checked for zeros.
 *   block_berlekamp_massey  S is a HOST array of len terms of b * b words.  Returns a left generator F(x) = sum_t F_t x^t:
 *                 coef[(t * b + r) * b + c] = F_t[r, c] for 0 <= t <= len (the caller gives (len + 1) * b * b words), low degree
 *                 first, balanced residues; rowdeg[r] is the degree of row r, the words of a row above its degree are zero,
 *                 *dmax is the largest row degree.
 *                   (A) for every row r and every 0 <= i < len - rowdeg[r]: sum_{t <= rowdeg[r]} F_t[r, :] S_{i+t} = 0;
 *                   (B) the b x b matrix of leading row coefficients (row r taken at x^rowdeg[r]) is non-singular;
 *                   (C) the row degrees are those of a minimal approximant basis of [S(x); I] at order len, taken by
 *                       ascending (degree, index) with independent leading rows; their sum is the rank of the block Hankel
 *                       matrix of the sequence when len covers the left and right generator degrees.
 *                 F is unique only up to row operations: it is specified by (A), (B), (C) and by being the same bytes in
 *                 two runs.  The zero sequence gives F = I, all degrees 0.  The state lives in device memory; a step is three
 *                 ordinary launches on one stream (discrepancy, elimination, update), no grid-wide barrier.
 *   block_wiedemann_det, spmv_block_wiedemann_det, dcsr_block_wiedemann_det
 *                 A host matrix, a resident operator, a resident matrix; A must be square.  tries <= 0 means 3.  Try t takes
 *                 D = precond_diagonal(n, seed + t, 0), U, V = minpoly_vectors(n, b, seed + t), the block sequence of D A with
 *                 len = 2 * ceil(n / b) + 2 terms, and its generator F.  When the row degrees sum to n:
 *                 det A = (-1)^n det F_0 / det(leading row coefficients of F) / prod d_i (0 when F_0 is singular), *status = 1;
 *                 the two b x b determinants and prod d_i are exact host arithmetic.  Otherwise the next seed is tried; after
 *                 the last try *status = 0 and *det = 0.
 *                 *status = 1 IS MONTE CARLO, unlike wiedemann_det: the proof there rests on the 2 n terms of a scalar
 *                 sequence and does not carry over to a block sequence of about 2 n / b terms.  The value is right with a
 *                 probability that grows with p (and is poor over GF(3)); nothing verifies it.
 *                 The empty matrix has determinant 1, status 1, and needs no device.
 *   stats         of the last of these calls of this thread: out[10] = b, len, steps of the sequence (products with A, summed
 *                 over the tries), launches, sum of the row degrees (last try), tries used, device microseconds of the
 *                 sequences and of Berlekamp-Massey (HIP events), n, largest row degree.  Every call clears what it does not fill.
 *   deterministic two runs give the same bytes (the projection and the discrepancy add integers)
 *   errors        "b must be 2, 4, 8 or 16", a NULL operator / matrix / array, a matrix that is not square ("not square (3 x 2)"),
 *                 len outside 1 .. 2^24 - 1 ("len out of range"), trans outside 0 .. 1, ldu or ldv < b, a word of d_left that is
 *                 zero mod p ("d_left[3] is zero mod p"), a prime outside 3 .. 0xFFFFFFFB or even ("prime must be odd"),
 *                 n >= 2^24, no device ("no HIP device"), out of memory: -1, NO output word is written,
 *                 spasm_amd_last_error() names the cause. */
int spasm_amd_block_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,
                             const spasm_ZZp *V, i64 ldv, spasm_ZZp *S);
int spasm_amd_block_sequence_dev(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,
                                 const spasm_ZZp *V, i64 ldv, spasm_ZZp *S, void *stream);
int spasm_amd_block_berlekamp_massey(int b, int len, const spasm_ZZp *S, i64 prime, spasm_ZZp *coef, int *rowdeg, int *dmax);
int spasm_amd_block_wiedemann_det(const struct spasm_csr *A, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);
int spasm_amd_spmv_block_wiedemann_det(spasm_amd_spmv *op, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);
int spasm_amd_dcsr_block_wiedemann_det(const spasm_amd_dcsr *D, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);
void spasm_amd_block_stats(i64 *out);   /* of the last block Wiedemann call of this thread */

/* ---- block Horner and the block Wiedemann solve (engine extension; csrc/block_horner.hpp) ----
 * A solve from the block sequence above: about 2 n / b products for the sequence and n / b for block Horner, where
 * spasm_amd_wiedemann_solve takes 2 n and up to n, and one run serves up to b right-hand sides.  b is 2, 4, 8 or 16.
 *   block_poly_apply  op is a resident SQUARE operator; coef, V (n x b, ldv >= b) and X (n x K, ldx >= K, 1 <= K <= b) are HOST
 *                 arrays, any int32 is reduced where it is read.  X <- sum_{t=0}^{D} op(A)^t V C_t mod p as balanced residues,
 *                 C_t[c, j] = coef[(t * b + c) * K + j] (b x K), op(A) = A (trans 0) or A^T (trans 1); -1 <= D < 2^24 and
 *                 D = -1 gives X = 0 (coef may be NULL then).  Block Horner: Y <- op(A) Y + V C_s for s = D .. 0, the first
 *                 step without a product, so D products; one launch set per step (the step kernels of the resident product
 *                 with the b x K combination as epilogue).  V must not overlap X.  n = 0 returns at once.
 *   block_poly_apply_dev  the same on DEVICE arrays V and X of the operator's device (coef stays a HOST array), enqueued on stream
 *                 (NULL: the null stream) without a host synchronization, like poly_apply_dev.
 *   block_wiedemann_solve, spmv_block_wiedemann_solve, dcsr_block_wiedemann_solve
 *                 A host matrix, a resident operator, a resident matrix; A must be square, n < 2^24.  B (n x K, ldb >= K,
 *                 1 <= K <= b) and X (n x K, ldx >= K) are HOST arrays.  Solves op(A) x = b_j for every column of B; trans = 1
 *                 solves x A = b on the transposed view.  tries <= 0 means 3.  Try t takes U, Z = minpoly_vectors(n, b,
 *                 seed + t, p), overwrites the leading columns of Z by the undecided right-hand sides (packed in their order):
 *                 V = [B | Z]; the block sequence S_i = U^T op(A)^i V of len = 2 * ceil(n / b) + 2 terms; the left generator F of
 *                 the transposed terms S_i^T (block_berlekamp_massey on the device), so sum_t S_{i+t} F_t^T = 0; Gauss-Jordan
 *                 on [F_0 | I] (host, b^3).  Column j is regular when e_j lies in the row space of F_0: lambda F_0 = e_j; else
 *                 lambda is the (j mod nullity)-th vector of the left null space of F_0 in the order the elimination leaves
 *                 them.  With h = lambda F: x_j = -sum_{s < D} op(A)^s V h_{s+1}^T, D the largest row degree, by one block
 *                 Horner run for all undecided columns.  Then ONE more product forms r_j = op(A) x_j - b_j on the regular columns
 *                 and op(A) x_j on the others, and the non-zeros of x_j and r_j are counted on the device.
 *                 status[j] = 1: regular and r_j = 0, op(A) x_j = b_j IS PROVED;  2: not regular, r_j = 0 and x_j != 0, a proved
 *                 non-zero kernel vector (A is singular; nothing is said about b_j);  0: undecided after the last try, the column
 *                 of X is zero.  Undecided columns are retried with the next seed.  Nothing is written to X or status before
 *                 the last try has run.  n = 0: status 1 everywhere, no device needed.
 *   solve_stats   of the last of these calls of this thread: out[16] = n, b, K, len, tries used, products with A (all), those of
 *                 the sequences ((len - 1) a try), those of Horner and the check (max(D - 1, 0) + 1 a try; D for block_poly_apply),
 *                 launches, sum of the row degrees (last try), largest row degree, columns solved, columns with a kernel vector,
 *                 device microseconds of the sequences, of Berlekamp-Massey, of Horner + check (HIP events).  Every call clears
 *                 what it does not fill.  spasm_amd_block_stats keeps its ten slots and is not touched by these calls.
 *   deterministic two runs give the same bytes (the counts and projections add integers)
 *   errors        "b must be 2, 4, 8 or 16", "K out of range (1 <= K <= b)", "trans must be 0 or 1", "D out of range
 *                 (-1 <= D < 2^24)", "ldv < b", "ldb < K", "ldx < K", a NULL operator / matrix / array, a matrix that is not
 *                 square ("not square (3 x 2)"), "V must not overlap X", n >= 2^24, len outside 1 .. 2^24 - 1, no device
 *                 ("no HIP device"), out of memory: -1, NO output word is written, spasm_amd_last_error() names the cause. */
int spasm_amd_block_poly_apply(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,
                               spasm_ZZp *X, i64 ldx);
int spasm_amd_block_poly_apply_dev(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,
                                   spasm_ZZp *X, i64 ldx, void *stream);
int spasm_amd_block_wiedemann_solve(const struct spasm_csr *A, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                    spasm_ZZp *X, i64 ldx, int *status);
int spasm_amd_spmv_block_wiedemann_solve(spasm_amd_spmv *op, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                         spasm_ZZp *X, i64 ldx, int *status);
int spasm_amd_dcsr_block_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                         spasm_ZZp *X, i64 ldx, int *status);
void spasm_amd_block_solve_stats(i64 *out);   /* of the last block Horner / block Wiedemann solve call of this thread */

/* ---- kernel bases without fill-in (engine extension; csrc/colechelon.hpp) ----
 * Verified kernel vectors of a sparse matrix, rectangular or square, by block Wiedemann on M = op(A)^T D2 op(A), collected in the
 * reduced column echelon form of their span; with certify the basis can be PROVED complete.  Memory is O(nnz + dim * 64).
 *   dense_column_echelon  X is a HOST array, rows x K, row-major, leading dimension ldx >= K, 0 <= K <= 64, 0 <= rows < 2^30; any
 *                 int32 is reduced where it is read.  X is replaced by the reduced column echelon form of its column space:
 *                 column j < *rank has its first non-zero entry, a 1, in row pivots[j]; pivots ascends strictly; row pivots[j] is
 *                 zero in every other column; columns *rank .. K - 1 are zero; every word is the balanced residue.  The form is
 *                 unique: two runs, and two blocks with the same column space, give the same bytes.  pivots has room for K words.
 *                 Column by column on the device: a first-non-zero search (one integer atomicMin a workgroup), a copy of the pivot
 *                 row with the inverse of the pivot, one elimination pass over rows x K; no host synchronization between columns,
 *                 one read-back of the K pivot rows, one permutation.  O(rows * K^2) words moved.  rows = 0 or K = 0: rank 0, no
 *                 device needed.
 *   block_precond_sequence  op is a resident operator, rectangular or square; op(A) = A (trans 0) or A^T (trans 1) is n x m.
 *                 S[(i * b + r) * b + c] = sum_k U[k, r] * (M^i V)[k, c] mod p, 0 <= i < len, balanced residues, with
 *                 M = diag(d_right) op(A)^T diag(d_left) op(A) (m x m); d_right = NULL means the identity.  U and V are m x b HOST
 *                 arrays (ldu, ldv >= b), d_left has n words, d_right m, S len * b * b; b is 2, 4, 8 or 16, 1 <= len < 2^24.  A
 *                 step is two launch sets of the step kernels: the forward view with the diagonal d_left, the transposed view with
 *                 the block projection.  n = 0 or m = 0: M = 0, S_0 = U^T V, no device needed.
 *   wiedemann_kernel, spmv_wiedemann_kernel, dcsr_wiedemann_kernel
 *                 A host matrix, a resident operator, a resident matrix, n x m, n, m < 2^24.  Returns vectors x with A x = 0
 *                 (trans 1: x A = 0) as the columns of N: dim x *found, dim = m (n with trans), *found <= want <= 64, a HOST array
 *                 with ldn >= want, in the reduced column echelon form above; pivots (room for want words) gets its pivot rows.
 *                 b is 2, 4, 8 or 16; tries >= 1.  Try t = 0, 1, ..: D2 = precond_diagonal(rows of op(A), seed + t, 0) and
 *                 U, Y = minpoly_vectors(dim, b, seed + t, p); V = M Y; the block sequence U^T M^i V of 2 * ceil(dim / b) + 2
 *                 terms; the left generator F of its transposed terms (block_berlekamp_massey); the candidates
 *                 W = sum_s M^s Y F_s^T (dim x b) by ONE composite block Horner pass over Y, not V; then ONE product op(A) W with
 *                 the non-zero counts of every column of W and of op(A) W.  A column is accepted only when its residual count is 0
 *                 and it is non-zero: the residual is taken against A itself, not against M, so EVERY RETURNED COLUMN IS A PROVED
 *                 KERNEL VECTOR.  At most want - *found accepted columns (the first ones) join the basis, which is brought to
 *                 echelon form on the device: a dependent column falls out.  Over a small field ker M may exceed ker A; such
 *                 candidates are rejected, never returned.  The tries stop when *found = want, when the certification closes, or
 *                 after `tries`.
 *                 certify != 0: the preconditioned rank of spasm_amd_wiedemann_rank (K = 8, the same seed and tries) runs first;
 *                 its r is ALWAYS a lower bound of rank A, so dim - r bounds the nullity from above.  *complete = 1 exactly when
 *                 *found = dim - r: then the columns of N are a basis of the WHOLE kernel, and THIS IS A PROOF, never a Monte
 *                 Carlo claim.  *complete = 0 says nothing: certify was 0, the numbers did not meet, or want cut the basis short.
 *                 dim = 0: *found = 0, *complete = 1, no device needed.  A matrix op(A) without rows: unit vectors, no device.
 *   kernel_stats  of the last of these calls of this thread: out[19] = n, m, b, want, tries used, products with A (all), those of
 *                 the sequences (2 * len a try), of Horner (2 * D a try), of the check (1 a try), of the certification, launches,
 *                 candidates formed (b a try), accepted (joined the basis), dropped as dependent, found, device microseconds of the
 *                 sequences, of Berlekamp-Massey, of Horner + check, of the echelon form (HIP events).  found = accepted - dropped;
 *                 the rejected candidates have no slot: rejected = candidates - accepted.  dense_column_echelon fills launches,
 *                 found (the rank) and the echelon microseconds; block_precond_sequence the slots of its sequence.
 *   deterministic two runs give the same bytes
 *   errors        "K out of range (0 <= K <= 64)", "ldx < K", "rows out of range (0 <= rows < 2^30)", "prime out of range (2 < p <=
 *                 0xfffffffb)", "b must be 2, 4, 8 or 16", "trans must be 0 or 1", "want out of range (0 <= want <= 64)",
 *                 "ldn < want", "tries < 1", "len out of range (1 <= len < 2^24)", "bad arguments (trans 0/1, ldu >= b, ldv >= b)",
 *                 "Wiedemann kernel limited to dim < 2^24", a NULL operator / matrix / array, no device ("no HIP device"), out of
 *                 memory: -1, NO output word is written, spasm_amd_last_error() names the cause. */
int spasm_amd_dense_column_echelon(i64 rows, int K, spasm_ZZp *X, i64 ldx, i64 prime, int *rank, int *pivots);
int spasm_amd_block_precond_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *d_right /* or NULL */,
                                     const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S);
int spasm_amd_wiedemann_kernel(const struct spasm_csr *A, int trans, int b, int want, uint64_t seed, int tries, int certify,
                               spasm_ZZp *N, i64 ldn, int *found, int *pivots, int *complete);
int spasm_amd_spmv_wiedemann_kernel(spasm_amd_spmv *op, int trans, int b, int want, uint64_t seed, int tries, int certify,
                                    spasm_ZZp *N, i64 ldn, int *found, int *pivots, int *complete);
int spasm_amd_dcsr_wiedemann_kernel(const spasm_amd_dcsr *D, int trans, int b, int want, uint64_t seed, int tries, int certify,
                                    spasm_ZZp *N, i64 ldn, int *found, int *pivots, int *complete);
void spasm_amd_wiedemann_kernel_stats(i64 *out);   /* of the last kernel-basis call of this thread */

#ifdef __cplusplus
}
#endif
#endif /* SPASM_AMD_H */
