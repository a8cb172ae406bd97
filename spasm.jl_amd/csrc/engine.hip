// engine.hip -- round driver of the MI355X echelonization engine and its C ABI entry points.
//
// spasm_echelonize / spasm_kernel / spasm_transpose keep the signatures SpaSM.jl binds (reference
// src/SpaSM.jl:863, :879, :589): host CSR in, host LU / CSR out, caller owns the result.  Inside,
// the matrix is uploaded once, every round runs on the device (kernels.hpp), and only U, qinv and
// the rank come back.  There is NO CPU fallback: without a HIP device these entry points fail.
#include "common.hpp"
#include "kernels.hpp"
#include "stream.hpp"
#include "wlevel.hpp"
#include "greedy.hpp"
#include "dense.hpp"
#include "spmv.hpp"
#include "spgemm.hpp"
#include "reshape.hpp"
#include "trsolve.hpp"
#include "batch.hpp"
#include "blocks.hpp"
#include "solve_batch.hpp"
#include "solver.hpp"
#include <cstring>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <vector>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <atomic>
#include <string>

namespace {

struct EngineError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            char _b[512];                                                                             \
            snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            throw EngineError(_b);                                                                    \
        }                                                                                             \
    } while (0)

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    void alloc(size_t count)
    {
        release();
        if (count == 0) count = 1;
        const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            (void)hipGetLastError();
            char b[256];
            snprintf(b, sizeof b, "device allocation of %.2f GiB failed: %s (%.1f of %.1f GiB free)", (double)(count * sizeof(T)) / 1073741824.0,
                     hipGetErrorString(e), (double)fr / 1073741824.0, (double)tot / 1073741824.0);
            throw EngineError(b);
        }
        n = count;
    }
    void ensure(size_t count) { if (count > n) alloc(count); }
    void zero(hipStream_t s) { if (p) HIPCHK(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
};

// the calling thread's device, put back on scope exit; given a handle, that handle's device is selected in between
struct DeviceGuard {
    int prev = 0;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    template <class H> explicit DeviceGuard(const H *h) : DeviceGuard() { if (h) HIPCHK(hipSetDevice(h->dev)); }
    DeviceGuard(const DeviceGuard &) = delete;
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// a handle that lives on a device is destroyed on that device
template <class H> void handle_free(H *h)
{
    if (!h) return;
    DeviceGuard g;
    (void)hipSetDevice(h->dev);
    delete h;
}

// The one error guard of the C ABI: every exported function that can fail is `return abi_call(name, failure value, [&] { body });`.
// The thread's error text is cleared, the body runs, and a std::exception becomes the text "<who>: <what>" and the entry's failure
// value.  ABI_NAMED_BELOW: the functions below put the entry's name in front of most of their messages themselves (the triangular
// solves), so a <what> that begins with <who> is the text as it is.
enum AbiText { ABI_PREFIX, ABI_NAMED_BELOW };

template <class R, class F> R abi_call(const char *who, R fail, F &&body, AbiText text = ABI_PREFIX)
{
    spasm_clear_error();
    try {
        return body();
    } catch (const std::exception &e) {
        if (text == ABI_NAMED_BELOW && strncmp(e.what(), who, strlen(who)) == 0) spasm_set_error("%s", e.what());
        else spasm_set_error("%s: %s", who, e.what());
        return fail;
    }
}

template <class F> void abi_call(const char *who, F &&body)
{
    (void)abi_call(who, 0, [&] { body(); return 0; });
}

inline int cdiv(i64 a, i64 b) { return (int)((a + b - 1) / b); }

// device matrix: rows are slices (start,len) of ent; lead = leftmost column; orig = row of the input matrix
struct DevMat {
    int n = 0, m = 0;
    DevBuf<i64d> start;
    DevBuf<int> len, lead, orig;
    DevBuf<int2> ent;
};

struct Scanner {
    DevBuf<unsigned char> tmp;
    // (the sums are formed in the type of the output: 32-bit counts scan into 64-bit offsets)
    template <class In, class Out> void exclusive(const In *in, Out *out, size_t n, hipStream_t s)
    {
        size_t bytes = 0;
        HIPCHK(rocprim::exclusive_scan(nullptr, bytes, in, out, Out(0), n, rocprim::plus<Out>(), s));
        tmp.ensure(bytes);
        HIPCHK(rocprim::exclusive_scan(tmp.p, bytes, in, out, Out(0), n, rocprim::plus<Out>(), s));
    }
};

// hash-table classes of the scatter kernel: log2(slots), threads per row, waves per workgroup,
// unrolled rounds of pivot rows, largest row bound (load factor <= 5/8)
struct ScatterClass { int logt, tpr, wpb, maxr; i64 cap; };
const ScatterClass kClasses[7] = {{8, 64, 4, 1, 160},  {9, 64, 4, 2, 320},   {10, 64, 4, 4, 640},  {11, 128, 2, 4, 1280},
                                  {12, 256, 4, 4, 2560}, {13, 256, 4, 5, 5120}, {14, 256, 4, 5, 10240}};
const int kNumHashClasses = 7;

inline size_t scatter_lds_bytes(const ScatterClass &c, bool small)
{
    const size_t retry = small ? RetryList<true>::BYTES : RetryList<false>::BYTES; // one list per wave
    const size_t table = ((size_t)1 << c.logt) * (small ? 8 : 12) + 32; // + s_misc
    return c.tpr == 64 ? (table + retry) * (size_t)c.wpb : table + retry * (size_t)c.wpb;
}

// function attributes (the opt-in to more than 64 KB of dynamic LDS) are per DEVICE: a process that drives several devices
// (spasm_amd_echelonize_multi) sets them on each
constexpr int kMaxDev = 64;
inline int current_device()
{
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    return dev & (kMaxDev - 1);
}

template <int LOGT, int TPR, int WPB, int MAXR, bool SMALL, int MINW = 1> void init_scatter(size_t lds)
{
    static bool attr_done[kMaxDev] = {false};
    bool &done = attr_done[current_device()];
    if (!done) {
        HIPCHK(hipFuncSetAttribute((const void *)k_scatter<LOGT, TPR, WPB, MAXR, SMALL, MINW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
}
template <int LOGT, int TPR, int WPB, int MAXR, bool SMALL, int MINW = 1> void launch_scatter(const ScatterArgs &a, int grid, size_t lds, hipStream_t s)
{
    init_scatter<LOGT, TPR, WPB, MAXR, SMALL, MINW>(lds);
    if (grid <= 0) return; // (warm-up call: attributes only)
    hipLaunchKernelGGL((k_scatter<LOGT, TPR, WPB, MAXR, SMALL, MINW>), dim3(grid), dim3(WPB * 64), lds, s, a);
    HIPCHK(hipGetLastError());
}

template <bool SMALL> void launch_scatter_class(int cls, const ScatterArgs &a, int grid, size_t lds, hipStream_t s)
{
    switch (cls) {
    case 0: launch_scatter<8, 64, 4, 1, SMALL>(a, grid, lds, s); break;
    case 1: launch_scatter<9, 64, 4, 2, SMALL>(a, grid, lds, s); break;
    case 2: launch_scatter<10, 64, 4, 4, SMALL, 4>(a, grid, lds, s); break;   // 8 KiB tables: 19 rows per CU fit, keep the registers under 96
    case 3: launch_scatter<11, 128, 2, 4, SMALL, 4>(a, grid, lds, s); break;  // 16 KiB tables: 10 workgroups of 2 waves per CU
    case 4: launch_scatter<12, 256, 4, 4, SMALL, 4>(a, grid, lds, s); break;
    case 5: launch_scatter<13, 256, 4, 5, SMALL>(a, grid, lds, s); break;
    case 6: if (SMALL) launch_scatter<14, 256, 4, 5, true>(a, grid, lds, s); break;
    default: break;
    }
}

// grid = min(rows, resident workgroups): the kernels walk their row list with a grid stride, and a workgroup that is not resident
// from the start would do its share after everybody else (the LDS bound alone can be above what the registers admit)
template <int LOGT, int TPR, int WPB, int B, bool SMALL, int MINW = 1, int EPL = 1, int QX = 0, bool BLOOM = false, bool SEG = false> void launch_wstream(const StreamArgs &a, int nrows, int num_cu, size_t lds, hipStream_t s)
{
    static int per_cu_dev[kMaxDev] = {0};
    int &per_cu = per_cu_dev[current_device()];
    if (!per_cu) {
        HIPCHK(hipFuncSetAttribute((const void *)k_wstream<LOGT, TPR, WPB, B, SMALL, MINW, EPL, QX, BLOOM, SEG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int nb = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_wstream<LOGT, TPR, WPB, B, SMALL, MINW, EPL, QX, BLOOM, SEG>, WPB * 64, lds));
        per_cu = std::max(nb, 1);
    }
    if (nrows <= 0) return; // (warm-up call: attributes and occupancy only)
    const int rows_per_block = TPR == 64 ? WPB : 1;
    const int grid = std::max(1, std::min((nrows + rows_per_block - 1) / rows_per_block, num_cu * per_cu));
    hipLaunchKernelGGL((k_wstream<LOGT, TPR, WPB, B, SMALL, MINW, EPL, QX, BLOOM, SEG>), dim3(grid), dim3(WPB * 64), lds, s, a);
    HIPCHK(hipGetLastError());
}

// chunks of the plan along W: 2^6 entries (a lane of the streaming kernel takes one entry per chunk) or 2^7 (two: one 16-byte load and,
// where the chunk is full, one 16-byte store per lane; half the per-chunk work).  SPASM_AMD_CHUNK = 64 | 128.
// Measured on config 3 (the rows of W average 170 entries): chunks of 128 are SLOWER, 3.75 ms per step against 3.33 -- a run of 170
// entries is three chunks of 64 (89 % of the lanes busy) or two of 128 (66 %), and a chunk of the two-entry kernel costs 1.7 x the
// instructions of a one-entry chunk: nothing is saved below runs of ~500 entries.  Default 64; the other stays for such matrices.
inline bool stream_bloom()
{
    const char *e = getenv("SPASM_AMD_BLOOM");
    return e && atoi(e) != 0;
}
inline int stream_chunk_log()
{
    const char *e = getenv("SPASM_AMD_CHUNK"); // (read per launch: a test sets it for one case)
    return e && atoi(e) == 128 ? 7 : 6;
}
// What the plan along W writes and the streaming kernels read (fixed by the plan: the scatter of a solve takes what its plan cut).
// Default: SEGMENT records, one per run, the stream cut by position (stream.hpp: k_wplan<.., true>, k_wstream<.., SEG>).  The two
// measured alternatives keep the chunk records they were built on: SPASM_AMD_CHUNK=128 (two entries per lane) and
// SPASM_AMD_BLOOM=1 (the filter; chunks of 64).  The streaming kernels of the segment route address the U_PN + own + W buffer by
// 32-bit BYTE offsets from its base: a buffer of 2^29 entries or more (the engine's own limit is 2^32 entries, prepare_w) also
// takes chunk records of 64 and the kernels with 64-bit addresses.
enum StreamMode { STREAM_SEG = 0, STREAM_CHUNK64 = 1, STREAM_BLOOM = 2, STREAM_CHUNK128 = 3 };
inline StreamMode stream_mode(i64 buffer_entries)
{
    if (stream_chunk_log() == 7) return STREAM_CHUNK128;
    if (stream_bloom()) return STREAM_BLOOM;
    return buffer_entries < ((i64)1 << 29) ? STREAM_SEG : STREAM_CHUNK64;
}

// the streaming twins of the hash-table classes (row bounds up to 160 << c): first table of 256 << c words (at most 5/8 full); a
// wave per row up to 640 entries, then 2 and 4 waves
const int kNumStreamClasses = 7;
inline int stream_logt(int c) { return 8 + c; }
inline int stream_tpr(int c) { return c <= 2 ? 64 : (c == 3 ? 128 : 256); }
inline int stream_wpb(int c) { return c == 3 ? 2 : 4; }
template <bool SMALL> void launch_stream_class(int cls, const StreamArgs &a, int nrows, int num_cu, size_t lds, hipStream_t s, StreamMode mode)
{
    if (mode == STREAM_SEG) { // (ring slots as for the chunk records: a slot is 64 positions now)
        switch (cls) {
        case 0: launch_wstream<8, 64, 4, 4, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 1: launch_wstream<9, 64, 4, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 2: launch_wstream<10, 64, 4, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 3: launch_wstream<11, 128, 2, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 4: launch_wstream<12, 256, 4, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 5: launch_wstream<13, 256, 4, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        case 6: launch_wstream<14, 256, 4, 8, SMALL, 1, 1, 0, false, true>(a, nrows, num_cu, lds, s); break;
        default: break;
        }
        return;
    }
    if (mode == STREAM_CHUNK128) {
        switch (cls) { // (ring slots D: chunks of 128 in flight per wave)
        case 0: launch_wstream<8, 64, 4, 2, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 1: launch_wstream<9, 64, 4, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 2: launch_wstream<10, 64, 4, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 3: launch_wstream<11, 128, 2, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 4: launch_wstream<12, 256, 4, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 5: launch_wstream<13, 256, 4, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        case 6: launch_wstream<14, 256, 4, 4, SMALL, 1, 2>(a, nrows, num_cu, lds, s); break;
        default: break;
        }
        return;
    }
    if (mode == STREAM_BLOOM) { // the duplicate check as a filter (stream.hpp: BLOOM)
        switch (cls) {
        case 0: launch_wstream<8, 64, 4, 4, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 1: launch_wstream<9, 64, 4, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 2: launch_wstream<10, 64, 4, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 3: launch_wstream<11, 128, 2, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 4: launch_wstream<12, 256, 4, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 5: launch_wstream<13, 256, 4, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        case 6: launch_wstream<14, 256, 4, 8, SMALL, 1, 1, 0, true>(a, nrows, num_cu, lds, s); break;
        default: break;
        }
        return;
    }
    // (groups of two chunks instead of four for the classes whose rows have three to six chunks, so that fewer of them take the
    // one-at-a-time path of a group that is not full: no difference, 0.1085 / 0.208 ms against 0.1083 / 0.2043; template parameter QX)
    switch (cls) {
    case 0: launch_wstream<8, 64, 4, 4, SMALL>(a, nrows, num_cu, lds, s); break;
    case 1: launch_wstream<9, 64, 4, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    case 2: launch_wstream<10, 64, 4, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    case 3: launch_wstream<11, 128, 2, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    case 4: launch_wstream<12, 256, 4, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    case 5: launch_wstream<13, 256, 4, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    case 6: launch_wstream<14, 256, 4, 8, SMALL>(a, nrows, num_cu, lds, s); break;
    default: break;
    }
}

// ------------------------------------------------------------------------------------------------
// One echelonization round on one device.
// ------------------------------------------------------------------------------------------------
struct Round {
    ZpField F;
    int m = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    Scanner scan;

    // election
    DevBuf<u64d> best;
    DevBuf<int> colflag, colscan, qinv_r, pivrow, pivcol, is_piv, rowflag, rowscan, np_rows;
    int npiv = 0, nnp = 0;
    // U of this round
    DevBuf<i64d> ulen, uoff;
    i64 utotal = 0;
    DevBuf<int2> Ufull, UPP, UPN;
    DevBuf<UHdr> uhdr;
    // Uinv = (I + U_PP)^-1, one row per pivot (built once per round when the reach is short)
    bool use_uinv = false;
    DevMat E;                       // the unit rows e_r
    DevBuf<int2> UinvPool;
    DevBuf<i64d> UinvStart, ubound;
    DevBuf<int> UinvLen;
    DevBuf<int4> colinfo;           // per column: pivot index + location of its Uinv row
    DevBuf<unsigned> pbits;         // per column: one bit, set for pivot columns
    DevBuf<i64d> rstart;            // per processed row slot: start / length of its own entries
    DevBuf<int> rlen;
    i64 uinv_nnz = 0;
    // solve
    DevBuf<int4> Lpool;
    DevBuf<int> Lidx;               // pivot index of every record (only when want_idx: kernel basis, triangular solve)
    bool want_idx = false;
    DevBuf<int> sflag;              // per row slot: the streaming scatter may take the row
    DevBuf<int2> fixbuf;            // per row slot: SFIX duplicates found by the streaming kernels, merged by k_stream_fix
    DevBuf<int> fixcnt;
    bool use_stream = true;         // SPASM_AMD_STREAM=0 turns W and the streaming scatter off
    StreamMode smode = STREAM_SEG;  // records of the last plan along W: segments, or chunks of 2^6 / 2^7 entries (stream_mode)
    // W = -(I + U_PP)^-1 U_PN (stream.hpp), built level by level of the pivot graph (wlevel.hpp).  One buffer, addressed by 32-bit
    // offsets: [U_PN | the own non-pivot entries of the rows the plan kernel takes | the rows of W]
    bool use_w = false;
    bool force_lists = false;       // keep to the multiplier lists even when W is there (exact trip counters: they count list entries)
    DevBuf<int4> wcol;              // per pivot column: {pivot index, length, offset} of its row of W
    DevBuf<int2> wrow;              // the same per pivot index: {offset, length}
    DevBuf<int> wreject_list;
    i64 wtotal = 0;                 // entries of W's region handed out by the last build
    i64 wcap = 0;                   // entries of W's region
    i64 w_entries = 0, w_long_rows = 0; // entries of W, rows the workgroup kernel built (statistics of the first build)
    i64 own_base = 0, wbase = 0;    // where the own entries / the rows of W start in the buffer
    i64 own_total = 0;              // entries of the part of the buffer that takes the rows' own non-pivot entries
    DevBuf<u64d> own_ctr;           // its bump counters
    DevBuf<u64d> wstate, wblk;      // cursor + statistics of the build; the blocks its waves carve rows from
    DevBuf<int> wmid_list, wbig_list, wbig_count; // rows the wave kernel leaves to the workgroup kernels; counts [2 * level + {0: medium, 1: large}]
    std::vector<int> wbig_at;       // rows the workgroup kernels built per level and tier (statistics: SPASM_AMD_WDEBUG, plans)
    bool want_w_row_stats = false;  // plans read them (spasm_amd_round_stats::w_long_rows)
    DevBuf<WLevRec> lev_recs;       // the pivot rows in level order, as the level kernels read them
    DevBuf<unsigned> lev0_sz, lev0_off; // level 0: lengths rounded up to 16, and their prefix sums = the rows' places in W
    DevBuf<u64d> lev0_ent;
    i64 lev0_total = 0, lev0_entries = 0;
    int wave_per_cu_blocks = 0;     // resident workgroups of k_wlevel_wave per CU
    // levels of the pivot graph: level L = lev_order[lev_start[L] .. lev_start[L + 1])
    DevBuf<int> lev, lev_keys, lev_iota, lev_order, lev_start_d, lev_flag;
    DevBuf<unsigned char> sort_tmp;
    std::vector<int> lev_start;
    int depth = -1;                 // deepest level; -1: no levels (not computed, or the graph is deeper than WMAXLEV)
    bool quiet_rejects = false;     // a plan whose dry run saw the plan kernel reject no row: later runs skip the chain-solve launches
    DevBuf<u64d> pool_ctr;          // NPOOL sharded bump counters
    int npool_active = NPOOL;       // regions in use by the current solve
    u64d region_cap = 0;
    DevBuf<i64d> Lstart, bound, sstart;
    DevBuf<int> Llen, overflow_list, overflow2_list, fail_list;
    DevBuf<long long> pmask;        // per row slot: which own entries sit on pivot columns (solve -> scatter)
    // last-resort solve (dense vector + bitmap over the pivot indices, per workgroup)
    int big_blocks = 0, big_npiv = -1;
    DevBuf<int> xdense;
    DevBuf<unsigned> bitmap;
    DevBuf<int4> bigscratch;
    DevBuf<RoundCounters> ctr;
    RoundCounters hctr;
    // scatter
    DevBuf<int> class_count, class_list;
    DevBuf<RowDesc> class_desc;
    // last-resort scatter (dense accumulator + bitmap + touched list over the columns, per workgroup)
    int bigsc_blocks = 0, bigsc_m = -1;
    DevBuf<long long> sc_xdense;
    DevBuf<unsigned> sc_bitmap;
    DevBuf<int> sc_touched;
    DevBuf<u64d> stamps;            // diagnostic build only
    DevMat S;
    i64 s_capacity = 0;      // entries S.ent can hold (sum of bounds at the time it was sized)
    i64 s_total_bound = 0;
    int free_cols = 0;
    // timing
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipStream_t side = nullptr;     // the few rows of the largest table classes run beside the others
    hipStream_t twin_s[3] = {nullptr, nullptr, nullptr}; // with `side`: the hash-table twins of the streaming classes, four abreast
    hipEvent_t twin_ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t lane_s[4] = {nullptr, nullptr, nullptr, nullptr}; // further lanes of the streaming classes (lane 0 = the round's stream)
    hipEvent_t lane_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_cls_done[NHASHMAX] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_cls[NCLASS + 1];  // one in front of every scatter launch (class_timing) and one behind the last
    int launch_cls[NCLASS];         // class id of launch i
    int nlaunch = 0;
    int hclass_count[NCLASS];
    int nhash_used = 0;
    bool class_timing = true;       // record an event pair around every scatter class (costs a few microseconds of gap each)

    Round()
    {
        memset(&hctr, 0, sizeof hctr);
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        for (auto &e : ev_cls) { e = nullptr; HIPCHK(hipEventCreate(&e)); }
        memset(hclass_count, 0, sizeof hclass_count);
        memset(launch_cls, 0, sizeof launch_cls);
        if (const char *e = getenv("SPASM_AMD_STREAM")) use_stream = atoi(e) != 0;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) num_cu = prop.multiProcessorCount;
    }
    ~Round()
    {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_cls) if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_w) if (e) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        for (auto &e : lane_ev) if (e) (void)hipEventDestroy(e);
        for (auto &l : lane_s) if (l) (void)hipStreamDestroy(l);
        for (auto &e : ev_cls_done) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        for (auto &e : twin_ev) if (e) (void)hipEventDestroy(e);
        for (auto &l : twin_s) if (l) (void)hipStreamDestroy(l);
    }

    // ---- (1a) local candidates: best[j] = min over local rows with leftmost column j of (len, global row)
    void elect_local(const DevMat &A, int row_base, int row_stride = 1)
    {
        m = A.m;
        best.ensure((size_t)m + 1);
        hipLaunchKernelGGL(k_fill_u64, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, stream, (i64d)m + 1, (u64d)NO_BEST, best.p);
        HIPCHK(hipGetLastError());
        if (A.n > 0) {
            hipLaunchKernelGGL(k_elect, dim3(cdiv(A.n, 256)), dim3(256), 0, stream, A.n, row_base, row_stride, A.len.p, A.lead.p, best.p);
            HIPCHK(hipGetLastError());
        }
    }

    // ---- (1b) number the pivots by ascending column; pivrow holds GLOBAL row ids
    void assign_pivots()
    {
        colflag.ensure((size_t)m + 1);
        colscan.ensure((size_t)m + 1);
        qinv_r.ensure((size_t)m + 1);
        hipLaunchKernelGGL(k_col_flags, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, stream, m, best.p, colflag.p);
        HIPCHK(hipGetLastError());
        scan.exclusive(colflag.p, colscan.p, (size_t)m + 1, stream);
        HIPCHK(hipMemcpyAsync(&npiv, colscan.p + m, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        pivrow.ensure((size_t)npiv + 1);
        pivcol.ensure((size_t)npiv + 1);
        if (m > 0) {
            hipLaunchKernelGGL(k_col_assign, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, best.p, colscan.p, qinv_r.p, pivrow.p, pivcol.p);
            HIPCHK(hipGetLastError());
        }
    }

    // ---- (1b') "FL on columns": after the leftmost election (best[] filled, pivots numbered), non-pivot rows take pivots on
    // columns no pivot row touches (kernels.hpp, k_close_cols ..).  Renumbers the pivots: the new ones first.  Returns how many
    // were added.  Single device only (the proposals would need a second all-reduce in a sharded round).
    DevBuf<int> closed, colcnt, prop, newflag, newscan;
    bool quiet_fallbacks = false; // a plan whose dry run sent no row past the first combine class: later runs skip those launches
    bool quiet_known = false;     // set once a plan's dry run is over: the rows and the matrix of its solves do not change any more
    DevBuf<int> pivval; // the pivot entries before scaling (the diagonal of L), filled by build_U when want_pivval
    bool want_pivval = false;
    DevBuf<u64d> best2;
    int n_leftmost = 0, n_open = 0;
    DevBuf<int> newpass, newidx, newrow_of_col, newrows;
    // The search in steps, cut where an array that describes ALL rows must be reduced over the row shards (one device: no cut).
    // (row_base, row_stride): local row i is global row row_base + i * row_stride; pivrow / newrows hold global rows.
    int open_count[OPEN_PASSES + 1] = {0};
    int open_nnew = 0, open_npass = 0;
    // -> closed[] (reduce: MAX): the columns the pivot rows THIS shard holds touch
    void open_begin(const DevMat &A, int row_base, int row_stride)
    {
        n_leftmost = npiv;
        n_open = 0;
        open_nnew = open_npass = 0;
        for (int &c : open_count) c = 0;
        closed.ensure((size_t)m + 1); colcnt.ensure((size_t)m + 1); newflag.ensure((size_t)m + 1); newscan.ensure((size_t)m + 1);
        newpass.ensure((size_t)m + 1); newidx.ensure((size_t)m + 1); newrow_of_col.ensure((size_t)m + 1); newrows.ensure((size_t)m + 1);
        best2.ensure((size_t)m + 1);
        prop.ensure((size_t)A.n + 1);
        is_piv.ensure((size_t)A.n + 1);
        HIPCHK(hipMemsetAsync(closed.p, 0, ((size_t)m + 1) * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(newpass.p, 0, ((size_t)m + 1) * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(is_piv.p, 0, ((size_t)A.n + 1) * sizeof(int), stream));
        if (npiv > 0) {
            hipLaunchKernelGGL(k_mark_rows, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, row_base, row_stride, A.n, pivrow.p, is_piv.p);
            constexpr int TEAM = 8;
            hipLaunchKernelGGL((k_close_cols<TEAM>), dim3(cdiv((i64)npiv * TEAM, 256)), dim3(256), 0, stream, npiv, pivrow.p, row_base, row_stride, A.n, A.start.p, A.len.p,
                               A.ent.p, closed.p);
            HIPCHK(hipGetLastError());
        }
    }
    // -> colcnt[] (reduce: SUM): rows that are no pivots per column
    void open_hist(const DevMat &A)
    {
        HIPCHK(hipMemsetAsync(colcnt.p, 0, ((size_t)m + 1) * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(newflag.p, 0, ((size_t)m + 1) * sizeof(int), stream));
        hipLaunchKernelGGL(k_fill_u64, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, stream, (i64d)m + 1, (u64d)NO_BEST, best2.p);
        if (A.n > 0) hipLaunchKernelGGL(k_col_histogram, dim3(cdiv((i64)A.n * 8, 256)), dim3(256), 0, stream, A.n, is_piv.p, A.start.p, A.len.p, A.ent.p, colcnt.p);
        HIPCHK(hipGetLastError());
    }
    // -> best2[] (reduce: MIN): the best proposal per column
    void open_propose(const DevMat &A, int row_base, int row_stride)
    {
        constexpr int TEAM = 8;
        if (A.n > 0)
            hipLaunchKernelGGL((k_propose_open<TEAM>), dim3(cdiv((i64)A.n * TEAM, 256)), dim3(256), 0, stream, A.n, row_base, row_stride, is_piv.p, A.start.p, A.len.p,
                               A.ent.p, closed.p, colcnt.p, prop.p, best2.p);
        HIPCHK(hipGetLastError());
    }
    // -> newflag[] (reduce: MAX): the columns whose winner holds no other proposed column
    void open_accept(const DevMat &A, int row_base, int row_stride)
    {
        constexpr int TEAM = 8;
        if (A.n > 0)
            hipLaunchKernelGGL((k_accept_open<TEAM>), dim3(cdiv((i64)A.n * TEAM, 256)), dim3(256), 0, stream, A.n, row_base, row_stride, A.start.p, A.len.p, A.ent.p,
                               prop.p, best2.p, newflag.p);
        HIPCHK(hipGetLastError());
    }
    // the accepted pivots of the pass (the same on every shard) -> closed[] (reduce: MAX); returns how many
    int open_record(const DevMat &A, int pass, int row_base, int row_stride)
    {
        scan.exclusive(newflag.p, newscan.p, (size_t)m + 1, stream);
        int nacc = 0;
        HIPCHK(hipMemcpyAsync(&nacc, newscan.p + m, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (nacc == 0) return 0;
        constexpr int TEAM = 8;
        hipLaunchKernelGGL(k_record_open, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, pass, newflag.p, newscan.p, best2.p, newpass.p, newidx.p,
                           newrow_of_col.p, newrows.p, is_piv.p, row_base, row_stride, A.n);
        hipLaunchKernelGGL((k_close_cols<TEAM>), dim3(cdiv((i64)nacc * TEAM, 256)), dim3(256), 0, stream, nacc, newrows.p, row_base, row_stride, A.n, A.start.p, A.len.p,
                           A.ent.p, closed.p);
        HIPCHK(hipGetLastError());
        open_count[pass] = nacc;
        open_nnew += nacc;
        open_npass = pass;
        return nacc;
    }
    // renumber: the open-column pivots first (last pass first), the leftmost pivots behind them (colscan still holds their ascending
    // numbering).  Returns how many pivots the search added.
    int open_finish()
    {
        const int nnew = open_nnew;
        if (nnew == 0) return 0;
        int base[OPEN_PASSES + 2] = {0};
        for (int pass = open_npass, at = 0; pass >= 1; pass--) { base[pass] = at; at += open_count[pass]; }
        static_assert(OPEN_PASSES == 4, "k_col_assign2 takes the bases of four passes");
        pivrow.ensure((size_t)npiv + nnew + 1);
        pivcol.ensure((size_t)npiv + nnew + 1);
        hipLaunchKernelGGL(k_col_assign2, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, nnew, make_int4(base[1], base[2], base[3], base[4]), best.p, newpass.p,
                           newidx.p, newrow_of_col.p, colscan.p, qinv_r.p, pivrow.p, pivcol.p);
        HIPCHK(hipGetLastError());
        npiv += nnew;
        n_open = nnew;
        return nnew;
    }
    int extend_pivots_on_open_columns(const DevMat &A)
    {
        n_leftmost = npiv;
        n_open = 0;
        if (npiv == 0 || A.n == 0) return 0;
        open_begin(A, 0, 1);
        for (int pass = 1; pass <= OPEN_PASSES; pass++) {
            open_hist(A);
            open_propose(A, 0, 1);
            open_accept(A, 0, 1);
            if (open_record(A, pass, 0, 1) == 0) break;
        }
        return open_finish();
    }

    // ---- (1b'') the greedy cycle-free search (greedy.hpp; reference README.md:23): after the leftmost election and "FL on columns",
    // non-pivot rows take pivots on columns that carry none as long as the pivots stay permutable to a triangle.  Appends the new
    // pivots, then renumbers ALL pivots of the round topologically (descending level, ascending column).  Returns how many were
    // added.  Single device only, like "FL on columns".
    DevBuf<int> gr_accept, gr_ascan, gr_lev, gr_iota, gr_order, gr_prow, gr_pcol, gr_flag;
    DevBuf<u64d> gr_keys, gr_keys2;
    int n_greedy = 0;
    int extend_pivots_cycle_free(const DevMat &A)
    {
        n_greedy = 0;
        if (npiv == 0 || A.n == 0) return 0;
        const int n = A.n;
        best2.ensure((size_t)m + 1);
        prop.ensure((size_t)n + 1);
        gr_accept.ensure((size_t)n + 1);
        gr_ascan.ensure((size_t)n + 1);
        is_piv.ensure((size_t)n + 1);
        HIPCHK(hipMemsetAsync(is_piv.p, 0, ((size_t)n + 1) * sizeof(int), stream));
        hipLaunchKernelGGL(k_mark_rows, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, 0, 1, n, pivrow.p, is_piv.p);
        HIPCHK(hipGetLastError());
        int nnew = 0;
        int reach_max = GREEDY_REACH_MAX_DEFAULT, occ_max = GREEDY_OCC_MAX_DEFAULT;
        if (const char *e = getenv("SPASM_AMD_GREEDY_REACH_MAX")) reach_max = std::min(GR_BUDGET, std::max(0, atoi(e)));
        if (const char *e = getenv("SPASM_AMD_GREEDY_OCC_MAX")) occ_max = std::max(1, atoi(e));
        colcnt.ensure((size_t)m + 1);
        for (int pass = 1; pass <= GREEDY_PASSES; pass++) {
            HIPCHK(hipMemsetAsync(colcnt.p, 0, ((size_t)m + 1) * sizeof(int), stream));
            hipLaunchKernelGGL(k_col_histogram, dim3(cdiv((i64)n * 8, 256)), dim3(256), 0, stream, n, is_piv.p, A.start.p, A.len.p, A.ent.p, colcnt.p);
            hipLaunchKernelGGL(k_fill_u64, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, stream, (i64d)m + 1, (u64d)NO_BEST, best2.p);
            hipLaunchKernelGGL((k_greedy<1>), dim3(cdiv(n, GR_WPB)), dim3(64 * GR_WPB), 0, stream, n, is_piv.p, A.start.p, A.len.p, A.ent.p, qinv_r.p, pivrow.p, best2.p,
                               prop.p, gr_accept.p, colcnt.p, occ_max, reach_max);
            hipLaunchKernelGGL((k_greedy<2>), dim3(cdiv(n, GR_WPB)), dim3(64 * GR_WPB), 0, stream, n, is_piv.p, A.start.p, A.len.p, A.ent.p, qinv_r.p, pivrow.p, best2.p,
                               prop.p, gr_accept.p, colcnt.p, occ_max, reach_max);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemsetAsync(gr_accept.p + n, 0, sizeof(int), stream));
            scan.exclusive(gr_accept.p, gr_ascan.p, (size_t)n + 1, stream);
            int nacc = 0;
            HIPCHK(hipMemcpyAsync(&nacc, gr_ascan.p + n, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (nacc == 0) break;
            // (pivrow / pivcol grow: keep what is there)
            if ((size_t)(npiv + nnew + nacc + 1) > pivrow.n) {
                DevBuf<int> r2, c2;
                r2.alloc((size_t)(npiv + nnew + nacc) + (size_t)n / 8 + 1024);
                c2.alloc(r2.n);
                HIPCHK(hipMemcpyAsync(r2.p, pivrow.p, (size_t)(npiv + nnew) * sizeof(int), hipMemcpyDeviceToDevice, stream));
                HIPCHK(hipMemcpyAsync(c2.p, pivcol.p, (size_t)(npiv + nnew) * sizeof(int), hipMemcpyDeviceToDevice, stream));
                HIPCHK(hipStreamSynchronize(stream));
                pivrow = std::move(r2);
                pivcol = std::move(c2);
            }
            hipLaunchKernelGGL(k_greedy_record, dim3(cdiv(n, 256)), dim3(256), 0, stream, n, npiv + nnew, gr_accept.p, gr_ascan.p, prop.p, pivrow.p, pivcol.p, qinv_r.p,
                               is_piv.p);
            HIPCHK(hipGetLastError());
            nnew += nacc;
        }
        if (nnew == 0) return 0;
        npiv += nnew;
        n_greedy = nnew;
        // ---- topological renumbering of all pivots of the round
        gr_lev.ensure((size_t)npiv + 1); gr_iota.ensure((size_t)npiv + 1); gr_order.ensure((size_t)npiv + 1);
        gr_prow.ensure((size_t)npiv + 1); gr_pcol.ensure((size_t)npiv + 1); gr_keys.ensure((size_t)npiv + 1); gr_keys2.ensure((size_t)npiv + 1);
        gr_flag.ensure(4);
        HIPCHK(hipMemsetAsync(gr_lev.p, 0, ((size_t)npiv + 1) * sizeof(int), stream));
        constexpr int TEAM = 8;
        for (int batch = 0;; batch++) {
            if (batch * 8 > npiv + 8) throw EngineError("greedy pivot search: the pivots do not form an acyclic graph");
            for (int it = 0; it < 8; it++) {
                if (it == 7) HIPCHK(hipMemsetAsync(gr_flag.p, 0, sizeof(int), stream));
                hipLaunchKernelGGL((k_piv_relax<TEAM>), dim3(cdiv((i64)npiv * TEAM, 256)), dim3(256), 0, stream, npiv, pivrow.p, pivcol.p, A.start.p, A.len.p, A.ent.p,
                                   qinv_r.p, gr_lev.p, it == 7 ? gr_flag.p : (int *)nullptr);
            }
            HIPCHK(hipGetLastError());
            int ch = 1;
            HIPCHK(hipMemcpyAsync(&ch, gr_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (ch == 0) break;
        }
        hipLaunchKernelGGL(k_piv_keys, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, gr_lev.p, pivcol.p, gr_keys.p, gr_iota.p);
        HIPCHK(hipGetLastError());
        {
            size_t bytes = 0;
            HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, gr_keys.p, gr_keys2.p, gr_iota.p, gr_order.p, (size_t)npiv, 0, 64, stream));
            sort_tmp.ensure(bytes);
            HIPCHK(rocprim::radix_sort_pairs(sort_tmp.p, bytes, gr_keys.p, gr_keys2.p, gr_iota.p, gr_order.p, (size_t)npiv, 0, 64, stream));
        }
        HIPCHK(hipMemcpyAsync(gr_prow.p, pivrow.p, (size_t)npiv * sizeof(int), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemcpyAsync(gr_pcol.p, pivcol.p, (size_t)npiv * sizeof(int), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(k_piv_permute, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, gr_order.p, gr_prow.p, gr_pcol.p, pivrow.p, pivcol.p, qinv_r.p);
        HIPCHK(hipGetLastError());
        return nnew;
    }

    // ---- (1c) local non-pivot, non-empty rows
    // row_stride: local row i is global row row_base + i * row_stride; (lo, hi, step): which LOCAL rows this plan reduces
    void mark_local(const DevMat &A, int row_base, int lo = 0, int hi = INT_MAX, int row_stride = 1, int step = 1)
    {
        is_piv.ensure((size_t)A.n + 1);
        rowflag.ensure((size_t)A.n + 1);
        rowscan.ensure((size_t)A.n + 1);
        np_rows.ensure((size_t)A.n + 1);
        HIPCHK(hipMemsetAsync(is_piv.p, 0, ((size_t)A.n + 1) * sizeof(int), stream));
        if (npiv > 0) {
            hipLaunchKernelGGL(k_mark_rows, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, row_base, row_stride, A.n, pivrow.p, is_piv.p);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_row_flags, dim3(cdiv((i64)A.n + 1, 256)), dim3(256), 0, stream, A.n, lo, hi, step, is_piv.p, A.len.p, rowflag.p);
        HIPCHK(hipGetLastError());
        scan.exclusive(rowflag.p, rowscan.p, (size_t)A.n + 1, stream);
        HIPCHK(hipMemcpyAsync(&nnp, rowscan.p + A.n, sizeof(int), hipMemcpyDeviceToHost, stream));
        if (A.n > 0) {
            hipLaunchKernelGGL(k_compact, dim3(cdiv(A.n, 256)), dim3(256), 0, stream, A.n, rowflag.p, rowscan.p, np_rows.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(stream));
    }

    // ---- (2) U from the pivot rows; PM holds them, rowsrc[idx] = row of PM (device array)
    void build_U(const DevMat &PM, const int *rowsrc)
    {
        ulen.ensure((size_t)npiv + 1);
        uoff.ensure((size_t)npiv + 1);
        uhdr.ensure((size_t)npiv + 1);
        hipLaunchKernelGGL(k_gather_len, dim3(cdiv((i64)npiv + 1, 256)), dim3(256), 0, stream, npiv, rowsrc, PM.len.p, ulen.p);
        HIPCHK(hipGetLastError());
        scan.exclusive(ulen.p, uoff.p, (size_t)npiv + 1, stream);
        i64d tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, uoff.p + npiv, sizeof(i64d), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        utotal = tot;
        if (utotal >= (i64)0xffffffffLL) throw EngineError("pivot rows of one round exceed 2^32 entries");
        Ufull.ensure((size_t)utotal + 1);
        UPP.ensure((size_t)utotal + 1);
        UPN.ensure((size_t)utotal + 1);
        if (npiv > 0) {
            constexpr int TEAM = 16;
            if (want_pivval) pivval.ensure((size_t)npiv + 1);
            hipLaunchKernelGGL((k_build_U<TEAM>), dim3(cdiv((i64)npiv * TEAM, 256)), dim3(256), 0, stream, npiv, F, rowsrc, pivcol.p,
                               PM.start.p, PM.len.p, PM.ent.p, qinv_r.p, uoff.p, Ufull.p, UPP.p, UPN.p, uhdr.p, want_pivval ? pivval.p : nullptr);
            HIPCHK(hipGetLastError());
        }
        free_cols = m - npiv;
    }

    // ---- (3) SOLVE for `nrows` rows of M (rows = list of local rows or NULL)
    void alloc_solve(int nrows, i64 lpool_entries)
    {
        Lstart.ensure((size_t)nrows + 1);
        Llen.ensure((size_t)nrows + 1);
        bound.ensure((size_t)nrows + 1);
        sstart.ensure((size_t)nrows + 1);
        overflow_list.ensure((size_t)nrows + 1);
        fail_list.ensure((size_t)nrows + 1);
        overflow2_list.ensure((size_t)nrows + 1);
        pmask.ensure((size_t)nrows + 1);
        sflag.ensure((size_t)nrows + 1);
        fixcnt.ensure((size_t)nrows + 1);
        if (use_stream) fixbuf.ensure(((size_t)nrows + 1) * SFIX);
        npool_active = std::min(NPOOL, std::max(1, nrows / 4));
        region_cap = ((u64d)lpool_entries + npool_active - 1) / npool_active;
        Lpool.ensure((size_t)(region_cap * npool_active) + 1);
        if (want_idx) Lidx.ensure((size_t)(region_cap * npool_active) + 1);
        pool_ctr.ensure((size_t)NPOOL * POOL_STRIDE);
        alloc_big();
        ctr.ensure(NCTR);
        class_count.ensure(NCLASS);
        class_list.ensure((size_t)NCLASS * (size_t)(nrows > 0 ? nrows : 1));
        class_desc.ensure((size_t)NCLASS * (size_t)(nrows > 0 ? nrows : 1));
        S.start.ensure((size_t)nrows + 1);
        S.len.ensure((size_t)nrows + 1);
        S.lead.ensure((size_t)nrows + 1);
        S.orig.ensure((size_t)nrows + 1);
        // (what run_solve would otherwise allocate on its first use, between two launches of a round's timed step)
        rstart.ensure((size_t)nrows + 1);
        rlen.ensure((size_t)nrows + 1);
        wreject_list.ensure((size_t)nrows + 1);
        own_ctr.ensure((size_t)NPOOL * POOL_STRIDE);
    }

    void alloc_big()
    {
        if (big_npiv == npiv && big_blocks > 0) return;
        // the dense fallback keeps npiv * 20 bytes per workgroup; stay under ~2 GB
        const i64 per = std::max<i64>((i64)npiv, 1) * 20;
        // the kernel is a chain of dependent round trips per popped pivot: rows in flight are its throughput, so as many
        // one-wave workgroups as the chip holds (32 per CU), within 16 GiB of scratch
        big_blocks = (int)std::max<i64>(1, std::min<i64>((i64)num_cu * 32, ((i64)16 << 30) / per));
        big_npiv = npiv;
        const size_t nw = ((size_t)std::max(npiv, 1) + 31) / 32;
        xdense.alloc((size_t)big_blocks * (size_t)std::max(npiv, 1));
        bitmap.alloc((size_t)big_blocks * nw);
        bigscratch.alloc((size_t)big_blocks * (size_t)std::max(npiv, 1));
        xdense.zero(stream);
        bitmap.zero(stream);
    }

    // chain solve: small teams first, then one wave per row, then the unbounded fallback
    // (only, only_count: when given, the row slots to solve -- what the plan kernel left -- instead of all of them)
    void launch_chain(SolveArgs a, int nrows, bool first_class, const int *only = nullptr, const int *only_count = nullptr)
    {
        if (first_class) {
            a.retry = only;
            a.retry_count = only_count;
            a.overflow_list = overflow_list.p;
            a.overflow_count = &ctr.p->solve_overflow;
            constexpr int TEAM = 8, CAP = 128, TPB = 256;
            const int grid = only ? std::min(cdiv((i64)nrows * TEAM, TPB), num_cu * 8) : cdiv((i64)nrows * TEAM, TPB);
            hipLaunchKernelGGL((k_solve<TEAM, CAP, TPB>), dim3(grid), dim3(TPB), 0, stream, a);
            HIPCHK(hipGetLastError());
        }
        BigSolveArgs b;
        b.npiv = std::max(npiv, 1);
        b.nwords = (std::max(npiv, 1) + 31) / 32;
        b.xdense = xdense.p;
        b.bitmap = bitmap.p;
        b.scratch = bigscratch.p;
        const size_t lds_dense = (size_t)b.npiv * 4 + (size_t)b.nwords * 4;
        if (lds_dense <= 150 * 1024) {
            // second class: one workgroup per row, dense multiplier vector + pending bitmap in LDS (unbounded reach)
            b.s = a;
            b.s.retry = overflow_list.p;
            b.s.retry_count = &ctr.p->solve_overflow;
            b.s.overflow_list = nullptr;
            b.s.overflow_count = nullptr;
            static bool attr_done[kMaxDev] = {false};
            bool &done = attr_done[current_device()];
            if (!done) {
                HIPCHK(hipFuncSetAttribute((const void *)k_solve_big<true, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
                done = true;
            }
            const int per_cu = (int)std::max<size_t>(1, (size_t)(160 * 1024) / (lds_dense + 64));
            hipLaunchKernelGGL((k_solve_big<true, 256>), dim3(std::min(big_blocks, num_cu * per_cu)), dim3(256), lds_dense, stream, b);
            HIPCHK(hipGetLastError());
            return;
        }
        a.retry = overflow_list.p;
        a.retry_count = &ctr.p->solve_overflow;
        a.overflow_list = fail_list.p;
        a.overflow_count = &ctr.p->solve_failed;
        {
            constexpr int TEAM = 64, CAP = 4096, TPB = 64;
            hipLaunchKernelGGL((k_solve<TEAM, CAP, TPB>), dim3(std::min(nrows, 5 * num_cu)), dim3(TPB), 0, stream, a);
            HIPCHK(hipGetLastError());
        }
        b.s = a;
        b.s.retry = fail_list.p;
        b.s.retry_count = &ctr.p->solve_failed;
        b.s.overflow_list = nullptr;
        b.s.overflow_count = nullptr;
        hipLaunchKernelGGL((k_solve_big<false, 64>), dim3(big_blocks), dim3(64), 0, stream, b);
        HIPCHK(hipGetLastError());
    }

    // rows of Uinv: the chain solve applied to the unit rows e_r (once per round, after build_U)
    // expected_rows = rows the solve will process: building Uinv costs npiv chain solves, so it pays only for more rows than that
    double ms_uinv = 0, ms_w = 0;   // wall time of the last prepare_uinv / prepare_w, host synchronisations included
    double ms_levels = 0;           // of ms_w: the levels of the pivot graph (build_levels)
    double ms_w_sizing = 0;         // of ms_w: sizing the [U_PN | own | W] buffer and allocating what the build needs

    void prepare_uinv(i64 expected_rows = ((i64)1 << 62))
    {
        HIPCHK(hipStreamSynchronize(stream));
        const double t0 = spasm_wtime();
        prepare_uinv_(expected_rows);
        HIPCHK(hipStreamSynchronize(stream));
        ms_uinv = 1e3 * (spasm_wtime() - t0);
    }
    void prepare_w(i64 expected_rows, i64 own_entries)
    {
        HIPCHK(hipStreamSynchronize(stream));
        const double t0 = spasm_wtime();
        prepare_w_(expected_rows, own_entries);
        HIPCHK(hipStreamSynchronize(stream));
        ms_w = 1e3 * (spasm_wtime() - t0);
    }

    void prepare_uinv_(i64 expected_rows)
    {
        use_uinv = false;
        uinv_nnz = 0;
        if (npiv == 0 || expected_rows < (i64)npiv) return;
        E.n = npiv;
        E.m = m;
        E.start.ensure((size_t)npiv + 1);
        E.len.ensure((size_t)npiv + 1);
        E.ent.ensure((size_t)npiv + 1);
        UinvStart.ensure((size_t)npiv + 1);
        UinvLen.ensure((size_t)npiv + 1);
        ubound.ensure((size_t)npiv + 1);
        overflow_list.ensure((size_t)npiv + 1);
        fail_list.ensure((size_t)npiv + 1);
        ctr.ensure(NCTR);
        alloc_big();
        hipLaunchKernelGGL(k_unit_rows, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, pivcol.p, E.start.p, E.len.p, E.ent.p);
        HIPCHK(hipGetLastError());
        i64 pool = std::max<i64>(24 * (i64)npiv, 1 << 16);
        const i64 limit = 96 * (i64)npiv + (1 << 16); // beyond this average reach the combine would cost more than the chains
        for (;;) {
            npool_active = std::min(NPOOL, std::max(1, npiv / 4));
            const u64d ucap = ((u64d)pool + npool_active - 1) / npool_active;
            UinvPool.ensure((size_t)(ucap * npool_active) + 1);
            pool_ctr.ensure((size_t)NPOOL * POOL_STRIDE);
            HIPCHK(hipMemsetAsync(ctr.p, 0, NCTR * sizeof(RoundCounters), stream));
            HIPCHK(hipMemsetAsync(pool_ctr.p, 0, (size_t)NPOOL * POOL_STRIDE * sizeof(u64d), stream));
            SolveArgs a;
            a.nrows = npiv;
            a.rows = nullptr;
            a.self_idx = nullptr;
            a.start = E.start.p;
            a.len = E.len.p;
            a.ent = E.ent.p;
            a.qinv_r = qinv_r.p;
            a.uhdr = uhdr.p;
            a.UPP = UPP.p;
            a.Lpool = nullptr;
            a.Lidx = nullptr;
            a.Lpool2 = UinvPool.p;
            a.lpool_cap = ucap;
            a.pool_ctr = pool_ctr.p;
            a.npool = npool_active;
            a.Lstart = UinvStart.p;
            a.Llen = UinvLen.p;
            a.bound = ubound.p;
            a.free_cols = free_cols;
            a.ctr = ctr.p;
            a.F = F;
            // only the LDS classes: a pivot whose own reach is beyond them makes Uinv too large anyway
            a.retry = nullptr;
            a.retry_count = nullptr;
            a.overflow_list = overflow_list.p;
            a.overflow_count = &ctr.p->solve_overflow;
            {
                constexpr int TEAM = 8, CAP = 128, TPB = 256;
                hipLaunchKernelGGL((k_solve<TEAM, CAP, TPB>), dim3(cdiv((i64)npiv * TEAM, TPB)), dim3(TPB), 0, stream, a);
                HIPCHK(hipGetLastError());
            }
            {
                // pivots whose own reach exceeds the first class (128) already account for more than the budget of Uinv:
                // do not spend seconds in the second class to find that out (Macaulay-like rounds)
                int novf = 0;
                HIPCHK(hipMemcpyAsync(&novf, &ctr.p->solve_overflow, sizeof(int), hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                if ((i64)novf * 128 > limit) return;
            }
            a.retry = overflow_list.p;
            a.retry_count = &ctr.p->solve_overflow;
            a.overflow_list = nullptr;
            a.overflow_count = &ctr.p->solve_failed;
            {
                constexpr int TEAM = 64, CAP = 4096, TPB = 64;
                hipLaunchKernelGGL((k_solve<TEAM, CAP, TPB>), dim3(std::min(npiv, 5 * num_cu)), dim3(TPB), 0, stream, a);
                HIPCHK(hipGetLastError());
            }
            RoundCounters c = read_counters();
            const u64d used = pool_used(); // synchronises
            if (c.solve_failed) return;                       // some pivot reaches > 4096 others: chains it is
            if (c.lpool_overflow) {
                if (pool >= NPOOL * (limit / NPOOL + 1)) return; // Uinv too dense
                pool = std::min<i64>(std::max<i64>(pool * 4, (i64)used + 1024), NPOOL * (limit / NPOOL + 1));
                continue;
            }
            c.lpool_used = used;
            uinv_nnz = (i64)c.lpool_used;
            use_uinv = uinv_nnz <= limit && uinv_nnz < (i64)0x7fffffff;
            if (use_uinv) {
                colinfo.ensure((size_t)m + 1);
                pbits.ensure((size_t)cdiv(m, 256) * 8 + 2);
                hipLaunchKernelGGL(k_colinfo, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, qinv_r.p, UinvStart.p, UinvLen.p, colinfo.p, pbits.p);
                HIPCHK(hipGetLastError());
            }
            return;
        }
    }

    // ---- levels of the pivot graph (wlevel.hpp): relaxation on the device, rows ordered by level with a stable radix sort (a
    // level's rows in ascending pivot index: the build is the same every time).  Part of the pivot bookkeeping of a round, like the
    // reference's topological reordering of the pivots (README.md:21-24); the Schur step proper (build_w_levels ..) has no
    // host synchronisation.
    void build_levels()
    {
        depth = -1;
        if (npiv == 0) return;
        lev.ensure((size_t)npiv + 1);
        lev_keys.ensure((size_t)npiv + 1);
        lev_iota.ensure((size_t)npiv + 1);
        lev_order.ensure((size_t)npiv + 1);
        lev_start_d.ensure(WMAXLEV + 4);
        lev_flag.ensure(4);
        HIPCHK(hipMemsetAsync(lev.p, 0, ((size_t)npiv + 1) * sizeof(int), stream));
        bool converged = false;
        // a launch moves every row at least one level on: WMAXLEV + 2 launches settle any graph that is not too deep
        for (int batch = 0; batch * 8 < WMAXLEV + 2 && !converged; batch++) {
            for (int it = 0; it < 8; it++) {
                if (it == 7) HIPCHK(hipMemsetAsync(lev_flag.p, 0, sizeof(int), stream));
                hipLaunchKernelGGL(k_lev_relax, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, uhdr.p, UPP.p, lev.p, it == 7 ? lev_flag.p : (int *)nullptr, 2);
            }
            HIPCHK(hipGetLastError());
            int ch = 1;
            HIPCHK(hipMemcpyAsync(&ch, lev_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            converged = ch == 0;
        }
        if (!converged) return;
        hipLaunchKernelGGL(k_iota, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, lev_iota.p);
        HIPCHK(hipGetLastError());
        {
            size_t bytes = 0;
            HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, lev.p, lev_keys.p, lev_iota.p, lev_order.p, (size_t)npiv, 0, 10, stream));
            sort_tmp.ensure(bytes);
            HIPCHK(rocprim::radix_sort_pairs(sort_tmp.p, bytes, lev.p, lev_keys.p, lev_iota.p, lev_order.p, (size_t)npiv, 0, 10, stream));
        }
        hipLaunchKernelGGL(k_fill_int, dim3(1), dim3(WMAXLEV + 4 <= 256 ? 256 : 512), 0, stream, WMAXLEV + 3, npiv, lev_start_d.p);
        hipLaunchKernelGGL(k_lev_starts, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, lev_keys.p, lev_start_d.p, WMAXLEV + 1);
        HIPCHK(hipGetLastError());
        // what follows needs nothing from the host: the records in level order, the places of level 0 (rows that are copied) in W --
        // ONE read-back at the end
        lev_recs.ensure((size_t)npiv + 1);
        hipLaunchKernelGGL(k_lev_recs, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, lev_order.p, uhdr.p, pivcol.p, lev_recs.p);
        lev0_sz.ensure((size_t)npiv + 2);
        lev0_off.ensure((size_t)npiv + 2);
        lev0_ent.ensure(1);
        HIPCHK(hipMemsetAsync(lev0_ent.p, 0, sizeof(u64d), stream));
        hipLaunchKernelGGL(k_lev0_sizes, dim3(cdiv((i64)npiv + 1, 256)), dim3(256), 0, stream, npiv, lev_start_d.p + 1, lev_recs.p, lev0_sz.p, lev0_ent.p);
        HIPCHK(hipGetLastError());
        scan.exclusive(lev0_sz.p, lev0_off.p, (size_t)npiv + 1, stream);
        lev_start.assign(WMAXLEV + 3, npiv);
        int deepest = 0;
        unsigned tot0 = 0;
        u64d ent0 = 0;
        HIPCHK(hipMemcpyAsync(lev_start.data(), lev_start_d.p, (WMAXLEV + 3) * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&deepest, lev_keys.p + (npiv - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&tot0, lev0_off.p + npiv, sizeof tot0, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&ent0, lev0_ent.p, sizeof ent0, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (deepest > WMAXLEV) return;
        depth = deepest;
        lev_start[(size_t)depth + 1] = npiv;
        lev0_total = tot0;
        lev0_entries = (i64)ent0;
    }

    // ---- W, level by level (kernels only: part of every Schur step).  first: the build that follows build_U -- the workgroup kernel
    // runs behind every level and the caller then notes where it had work (wbig_at); later builds of the same U skip the others.
    int wblk_slots() const { return num_cu * (16 * 4 + 8 + 1); } // waves of the wave kernel, workgroups of the medium and of the large table
    // ---- W, level by level (kernels only: part of every Schur step).  Level 0 is a copy (k_wlevel0).  A level of many rows: the
    // wave kernel, then the workgroup kernel with the medium table for the rows it left, then the one with the largest table; a level
    // of at most 2048 rows skips the wave kernel (a launch costs ~10 us whatever it does): all its rows go to the workgroup kernel
    // with the medium table -- with the largest one when the level has no more rows than the chip has CUs.
    // first: the build that follows build_U, every launch is made and the caller notes the list counts (wbig_at); later builds of
    // the same U skip the launches whose lists were empty.
    hipEvent_t ev_w[2] = {nullptr, nullptr}; // around the level launches of the last W build
    void build_w_levels()
    {
        if (!ev_w[0]) for (auto &e : ev_w) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(ev_w[0], stream));
        const int nblk_words = 2 * wblk_slots();
        const int ncount_words = 2 * (depth + 2) * WL_NSUB * WL_SUBSTRIDE;
        hipLaunchKernelGGL(k_wbuild_reset, dim3(cdiv(std::max(nblk_words, ncount_words), 256)), dim3(256), 0, stream, wstate.p, wblk.p, nblk_words,
                           wbig_count.p, ncount_words, (u64d)lev0_total);
        HIPCHK(hipGetLastError());
        constexpr int NT_MID = 256, NT_BIG = 1024; // (512 threads for the medium table were slower: its rows wait on memory, and fewer workgroups fit a CU)
        const size_t lds_mid = F.small ? wl_wg_lds_bytes<true>(wl_mid_slots(), NT_MID) : wl_wg_lds_bytes<false>(wl_mid_slots(), NT_MID);
        const int big_slots = F.small ? wl_big_slots<true>() : wl_big_slots<false>();
        const size_t lds_big = F.small ? wl_wg_lds_bytes<true>(big_slots, NT_BIG) : wl_wg_lds_bytes<false>(big_slots, NT_BIG);
        if (!wave_per_cu_blocks) {
            int nb = 0;
            if (F.small) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_wlevel_wave<true>, 256, 0));
            else HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_wlevel_wave<false>, 256, 0));
            wave_per_cu_blocks = std::min(std::max(nb, 1), 16);
            if (F.small) {
                HIPCHK(hipFuncSetAttribute((const void *)k_wlevel_wg<true, NT_BIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_big));
                HIPCHK(hipFuncSetAttribute((const void *)k_wlevel_wg<true, NT_MID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mid));
            } else {
                HIPCHK(hipFuncSetAttribute((const void *)k_wlevel_wg<false, NT_BIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_big));
                HIPCHK(hipFuncSetAttribute((const void *)k_wlevel_wg<false, NT_MID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mid));
            }
        }
        const int mid_per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / (lds_mid + 256)));
        WLevelArgs a;
        a.UPP = UPP.p;
        a.buf = UPN.p;
        a.wrow = wrow.p;
        a.wcol = wcol.p;
        a.wstate = wstate.p;
        a.wbase = (unsigned)wbase;
        a.wcap = (u64d)wcap;
        a.wblk = wblk.p;
        a.F = F;
        a.list_stride = npiv;
        auto launch_wg = [&](int tier, int grid) {
            a.tslots = tier ? big_slots : wl_mid_slots();
            a.blk_base = num_cu * 16 * 4 + (tier ? num_cu * 8 : 0);
            if (tier) {
                if (F.small) hipLaunchKernelGGL((k_wlevel_wg<true, NT_BIG>), dim3(grid), dim3(NT_BIG), lds_big, stream, a);
                else hipLaunchKernelGGL((k_wlevel_wg<false, NT_BIG>), dim3(grid), dim3(NT_BIG), lds_big, stream, a);
            } else {
                if (F.small) hipLaunchKernelGGL((k_wlevel_wg<true, NT_MID>), dim3(grid), dim3(NT_MID), lds_mid, stream, a);
                else hipLaunchKernelGGL((k_wlevel_wg<false, NT_MID>), dim3(grid), dim3(NT_MID), lds_mid, stream, a);
            }
        };
        {
            const int cnt0 = lev_start[1];
            hipLaunchKernelGGL(k_wlevel0, dim3(std::max(1, std::min(cdiv((i64)cnt0 * 16, 256), num_cu * 8))), dim3(256), 0, stream, cnt0, lev_recs.p, lev0_off.p,
                               UPN.p, wrow.p, wcol.p, (unsigned)wbase, F);
        }
        for (int L = 1; L <= depth; L++) {
            const int cnt = lev_start[(size_t)L + 1] - lev_start[(size_t)L];
            if (cnt <= 0) continue;
            int *const mid_count = wbig_count.p + (size_t)(2 * L) * WL_NSUB * WL_SUBSTRIDE, *const big_count = wbig_count.p + (size_t)(2 * L + 1) * WL_NSUB * WL_SUBSTRIDE;
            // (every tier launch is made, with the grid of a full list: how many rows a list holds is only known on the device, and the
            // build runs once per round -- a launch whose list is empty costs a few microseconds)
            const int known_mid = -1, known_big = -1;
            a.cnt = cnt;
            a.rec_base = lev_start[(size_t)L];
            a.mid_list = wmid_list.p;
            a.mid_count = mid_count;
            a.big_list = wbig_list.p;
            a.big_count = big_count;
            a.list = nullptr;
            a.count = nullptr;
            if (cnt > 2048) {
                a.recs = lev_recs.p + lev_start[(size_t)L];
                a.tslots = 0;
                a.blk_base = 0;
                const int grid = std::min(cdiv(cnt, 4), num_cu * wave_per_cu_blocks);
                if (F.small) hipLaunchKernelGGL(k_wlevel_wave<true>, dim3(grid), dim3(256), 0, stream, a);
                else hipLaunchKernelGGL(k_wlevel_wave<false>, dim3(grid), dim3(256), 0, stream, a);
                a.recs = lev_recs.p;
                if (known_mid != 0) {
                    a.list = wmid_list.p;
                    a.count = mid_count;
                    a.big_list = nullptr; // (the wave kernel sorted the rows: what is on this list fits the medium table)
                    launch_wg(0, known_mid < 0 ? num_cu * mid_per_cu : std::min(num_cu * mid_per_cu, known_mid));
                }
            } else {
                a.recs = lev_recs.p;
                if (cnt <= num_cu) {
                    a.big_list = nullptr; // all rows with the largest table: what does not fit is not available
                    launch_wg(1, cnt);
                    continue;
                }
                launch_wg(0, std::min(num_cu * mid_per_cu, cnt)); // rows beyond the medium table go on the list of the largest
            }
            if (known_big != 0) {
                a.list = wbig_list.p;
                a.count = big_count;
                a.big_list = nullptr;
                launch_wg(1, known_big < 0 ? num_cu : std::min(num_cu, known_big));
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev_w[1], stream));
    }

    // Decides whether this round goes along W, sizes the [U_PN | own | W] buffer and builds W once (synchronises: the outcome of
    // the build is read back).  Worth it when many more rows than pivots are reduced; a W much larger than U means long chains,
    // which the multiplier lists serve better.
    // own_entries: upper bound of the entries of the rows that will be reduced along W (their non-pivot entries are copied into
    // the buffer by the plan kernel)
    void prepare_w_(i64 expected_rows, i64 own_entries)
    {
        use_w = false;
        wtotal = 0;
        ms_levels = 0;
        ms_w_sizing = 0;
        if (!use_stream || force_lists || want_idx || m >= (1 << 24) || npiv == 0 || expected_rows < 2 * (i64)npiv) return;
        {
            HIPCHK(hipStreamSynchronize(stream));
            const double t0 = spasm_wtime();
            build_levels();
            HIPCHK(hipStreamSynchronize(stream));
            ms_levels = 1e3 * (spasm_wtime() - t0);
        }
        if (depth < 0) return;
        const double t_sizing0 = spasm_wtime();
        // room for the rows' own entries: what they have, half as much again for uneven regions, and a block per team of the plan kernel
        const i64 own_room = ((own_entries + own_entries / 2 + (i64)num_cu * 16 * 16 * 256 + NPOOL) + 15) & ~(i64)15;
        own_base = (utotal + 15) & ~(i64)15;
        wbase = own_base + own_room;
        // offsets into the buffer are 32-bit
        i64 cap = std::min<i64>(64 * std::max<i64>(utotal, 1 << 16), (i64)0xffffffffLL - wbase - 64);
        {
            // memory only vetoes (the route changes, not the result): half of what is free beside the buffer already there
            size_t fr = 0, totmem = 0;
            HIPCHK(hipMemGetInfo(&fr, &totmem));
            const i64 have = (i64)UPN.n;
            const i64 room = have + (i64)(fr / 2 / sizeof(int2));
            if (wbase + cap + 1 > room) cap = room - wbase - 1;
        }
        cap &= ~(i64)15;
        if (cap < 4 * std::max<i64>(utotal, 1 << 12) || cap < 2 * lev0_total) return;
        if ((i64)UPN.n < wbase + cap + 1) {
            DevBuf<int2> both;
            both.alloc((size_t)(wbase + cap) + 1);
            if (utotal > 0) HIPCHK(hipMemcpyAsync(both.p, UPN.p, (size_t)utotal * sizeof(int2), hipMemcpyDeviceToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
            UPN = std::move(both);
        }
        wcap = cap;
        wrow.ensure((size_t)npiv + 1);
        wcol.ensure((size_t)m + 1);
        wmid_list.ensure((size_t)WL_NSUB * (size_t)npiv + 1);
        wbig_list.ensure((size_t)WL_NSUB * (size_t)npiv + 1);
        wbig_count.ensure((size_t)2 * (WMAXLEV + 2) * WL_NSUB * WL_SUBSTRIDE);
        wstate.ensure(WS_WORDS);
        wblk.ensure((size_t)2 * wblk_slots());
        own_ctr.ensure((size_t)NPOOL * POOL_STRIDE);
        pbits.ensure((size_t)cdiv(m, 256) * 8 + 2);
        hipLaunchKernelGGL(k_pbits, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, qinv_r.p, pbits.p);
        HIPCHK(hipGetLastError());
        wbig_at.assign((size_t)2 * (depth + 2), 0);
        {
            // (wall time of the sizing: the device-memory query and whatever had to be allocated -- once per Round for rounds of one size)
            HIPCHK(hipStreamSynchronize(stream));
            ms_w_sizing = 1e3 * (spasm_wtime() - t_sizing0);
        }
        build_w_levels();
        hipLaunchKernelGGL(k_wstats, dim3(cdiv(npiv, 256)), dim3(256), 0, stream, npiv, wrow.p, wstate.p);
        HIPCHK(hipGetLastError());
        u64d ws[WS_WORDS];
        HIPCHK(hipMemcpyAsync(ws, wstate.p, sizeof ws, hipMemcpyDeviceToHost, stream));
        const bool wdebug = getenv("SPASM_AMD_WDEBUG") != nullptr || want_w_row_stats;
        std::vector<int> parts;
        if (wdebug) { // (how many rows the workgroup kernels built, level by level: a statistic, 280 KB over PCIe)
            parts.resize((size_t)2 * (depth + 1) * WL_NSUB * WL_SUBSTRIDE);
            HIPCHK(hipMemcpyAsync(parts.data(), wbig_count.p, parts.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        if (wdebug)
            for (int k = 0; k < 2 * (depth + 1); k++)
                for (int sb = 0; sb < WL_NSUB; sb++) wbig_at[(size_t)k] += parts[((size_t)k * WL_NSUB + sb) * WL_SUBSTRIDE];
        if (ws[WS_ERROR]) throw EngineError("a hash table of the W build filled up (internal bound violated)");
        if (getenv("SPASM_AMD_WDEBUG")) {
            fprintf(stderr, "[wlevel] npiv %d depth %d entries %llu cursor %llu unavailable %llu long rows %llu; rows per level (medium, large):", npiv, depth,
                    (unsigned long long)ws[WS_ENTRIES], (unsigned long long)ws[WS_CURSOR], (unsigned long long)ws[WS_UNAVAIL], (unsigned long long)ws[WS_BIGROWS]);
            for (int L = 0; L <= depth; L++)
                fprintf(stderr, " %d (%d, %d)", lev_start[(size_t)L + 1] - lev_start[(size_t)L], wbig_at[(size_t)2 * L], wbig_at[(size_t)2 * L + 1]);
            fprintf(stderr, "\n");
        }
        // rows that could not be built send the rows that need them to the multiplier lists: a few are fine, many mean W does not pay
        if (ws[WS_UNAVAIL] * 64 > (u64d)npiv) return;
        wtotal = (i64)std::min<u64d>(ws[WS_CURSOR], (u64d)cap);
        w_entries = (i64)ws[WS_ENTRIES] + lev0_entries;
        w_long_rows = 0;
        for (int k = 0; k < 2 * (depth + 1); k++) w_long_rows += wbig_at[(size_t)k];
        own_total = own_room;
        use_w = true;
    }

    void run_solve(const DevMat &M, const int *rows, const int *self_idx, int nrows)
    {
        // the plan along the rows of W; what it leaves (streams beyond the streaming classes, rows that are bound to be full of
        // duplicate columns, rows that need a row of W that could not be built) goes through the multiplier lists
        const bool wmode = use_w && !force_lists && !self_idx && !want_idx;
        {
            static_assert(sizeof(RoundCounters) % 4 == 0, "cleared word by word");
            const int nctr_words = (int)(NCTR * sizeof(RoundCounters) / 4), npool_words = NPOOL * POOL_STRIDE;
            const int span = std::max(std::max(nctr_words, npool_words), nrows + 1);
            // (the counters of the plan kernel's own-entry regions are cleared here as well: one launch less per step)
            if (wmode) own_ctr.ensure((size_t)NPOOL * POOL_STRIDE);
            hipLaunchKernelGGL(k_solve_reset, dim3(cdiv(span, 256)), dim3(256), 0, stream, nrows, (unsigned *)ctr.p, nctr_words, pool_ctr.p,
                               npool_words, class_count.p, (int)NCLASS, bound.p, pmask.p, sflag.p, wmode ? own_ctr.p : (u64d *)nullptr);
            HIPCHK(hipGetLastError());
        }
        if (nrows == 0) return;
        SolveArgs a;
        a.nrows = nrows;
        a.rows = rows;
        a.self_idx = self_idx;
        a.retry = nullptr;
        a.retry_count = nullptr;
        a.start = M.start.p;
        a.len = M.len.p;
        a.ent = M.ent.p;
        a.qinv_r = qinv_r.p;
        a.uhdr = uhdr.p;
        a.UPP = UPP.p;
        a.Lpool = Lpool.p;
        a.Lidx = want_idx ? Lidx.p : nullptr;
        a.Lpool2 = nullptr;
        a.lpool_cap = region_cap;
        a.pool_ctr = pool_ctr.p;
        a.npool = npool_active;
        a.Lstart = Lstart.p;
        a.Llen = Llen.p;
        a.bound = bound.p;
        a.free_cols = free_cols;
        a.overflow_list = overflow_list.p;
        a.overflow_count = &ctr.p->solve_overflow;
        a.ctr = ctr.p;
        a.F = F;
        if (!wmode && !use_uinv) {
            launch_chain(a, nrows, true);
            return;
        }
        rstart.ensure((size_t)nrows + 1);
        rlen.ensure((size_t)nrows + 1);
        // (every step: a round gathers them once, and a plan's step is a round's)
        hipLaunchKernelGGL(k_gather_rows, dim3(cdiv(nrows, 256)), dim3(256), 0, stream, nrows, rows, M.start.p, M.len.p, rstart.p, rlen.p);
        HIPCHK(hipGetLastError());
        if (wmode) {
            wreject_list.ensure((size_t)nrows + 1);
            WPlanArgs wp;
            wp.nrows = nrows;
            wp.rstart = rstart.p;
            wp.rlen = rlen.p;
            wp.ent = M.ent.p;
            wp.pbits = pbits.p;
            wp.wcol = wcol.p;
            wp.Lpool = Lpool.p;
            wp.lpool_cap = region_cap;
            wp.pool_ctr = pool_ctr.p;
            wp.npool = npool_active;
            wp.upn = UPN.p;
            wp.own_base = (unsigned)own_base;
            wp.own_cap = (u64d)own_total / (u64d)npool_active;
            wp.own_ctr = own_ctr.p;
            wp.Lstart = Lstart.p;
            wp.Llen = Llen.p;
            wp.bound = bound.p;
            wp.pmask = pmask.p;
            wp.sflag = sflag.p;
            wp.free_cols = free_cols;
            wp.max_bound = (int)kClasses[kNumStreamClasses - 1].cap;
            wp.wave_row_bound = (int)kClasses[2].cap;
            wp.overflow_list = wreject_list.p;
            wp.overflow_count = &ctr.p->wplan_reject;
            wp.ctr = ctr.p;
            wp.F = F;
            smode = stream_mode(wbase + wcap); // (the streaming kernels of this solve's scatter take what the plan cut)
            wp.chunk_log = smode == STREAM_CHUNK128 ? 7 : 6;
            constexpr int TEAM = 16, TPB = 256;
            const dim3 grid(std::min(cdiv((i64)nrows * TEAM, TPB), num_cu * 16));
            if (smode == STREAM_SEG) hipLaunchKernelGGL((k_wplan<TEAM, TPB, true>), grid, dim3(TPB), 0, stream, wp);
            else hipLaunchKernelGGL((k_wplan<TEAM, TPB, false>), grid, dim3(TPB), 0, stream, wp);
            HIPCHK(hipGetLastError());
            if (!use_uinv) {
                // no Uinv beside W: the rows the plan kernel left are solved by elimination chains
                // (a plan that has seen its rows once knows whether anybody gets this far)
                if (!quiet_rejects) launch_chain(a, nrows, true, wreject_list.p, &ctr.p->wplan_reject);
                return;
            }
        }
        CombineArgs c;
        c.nrows = nrows;
        c.self_idx = self_idx;
        c.rstart = rstart.p;
        c.rlen = rlen.p;
        c.ent = M.ent.p;
        c.colinfo = colinfo.p;
        c.pbits = pbits.p;
        c.uhdr = uhdr.p;
        c.UinvPool = UinvPool.p;
        c.Lpool = Lpool.p;
        c.Lidx = want_idx ? Lidx.p : nullptr;
        c.sflag = nullptr; // (only the plan along W marks rows for the streaming kernel)
        c.lpool_cap = region_cap;
        c.pool_ctr = pool_ctr.p;
        c.npool = npool_active;
        c.Lstart = Lstart.p;
        c.Llen = Llen.p;
        c.bound = bound.p;
        c.pmask = pmask.p;
        c.free_cols = free_cols;
        c.retry = wmode ? wreject_list.p : nullptr;
        c.retry_count = wmode ? &ctr.p->wplan_reject : nullptr;
        c.overflow_list = overflow2_list.p;
        c.overflow_count = &ctr.p->combine_overflow;
        c.ctr = ctr.p;
        {
            const char *dbg = getenv("SPASM_DBG"); // timing ablations (diagnostic builds only)
            c.dbg = dbg ? atoi(dbg) : 0;
        }
        c.F = F;
        {
            constexpr int TEAM = 16, LOGC = 8, TPB = 256; // up to 128 distinct pivots per row
            const int grid = std::min(cdiv((i64)nrows * TEAM, TPB), num_cu * 8);
            if (F.small) hipLaunchKernelGGL((k_combine<TEAM, LOGC, TPB, true>), dim3(grid), dim3(TPB), 0, stream, c);
            else hipLaunchKernelGGL((k_combine<TEAM, LOGC, TPB, false>), dim3(grid), dim3(TPB), 0, stream, c);
            HIPCHK(hipGetLastError());
        }
        // (a plan that has seen its rows once knows whether anybody gets this far: three or four launches of ~8 us each, in
        // order, are a tenth of the step of a 1/8 shard)
        if (!quiet_fallbacks) {
            c.retry = overflow2_list.p;
            c.retry_count = &ctr.p->combine_overflow;
            c.overflow_list = overflow_list.p;
            c.overflow_count = &ctr.p->solve_overflow;
            {
                constexpr int TEAM = 64, LOGC = 12, TPB = 64; // one wave per row, up to 2048 distinct pivots
                const int grid = std::min(nrows, num_cu * 4);
                if (F.small) hipLaunchKernelGGL((k_combine<TEAM, LOGC, TPB, true>), dim3(grid), dim3(TPB), 0, stream, c);
                else hipLaunchKernelGGL((k_combine<TEAM, LOGC, TPB, false>), dim3(grid), dim3(TPB), 0, stream, c);
                HIPCHK(hipGetLastError());
            }
            launch_chain(a, nrows, false); // what is left: chain classes
        }
    }

    // sum of the NCTR statistic copies (synchronises)
    // (total_bound_of: also fetch the total of the bounds of that many rows, s_total_bound, in the same round trip)
    RoundCounters read_counters(int total_bound_of = -1)
    {
        std::vector<RoundCounters> h(NCTR);
        i64d tot = 0;
        HIPCHK(hipMemcpyAsync(h.data(), ctr.p, NCTR * sizeof(RoundCounters), hipMemcpyDeviceToHost, stream));
        if (total_bound_of >= 0) HIPCHK(hipMemcpyAsync(&tot, sstart.p + total_bound_of, sizeof(i64d), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (total_bound_of >= 0) s_total_bound = tot;
        RoundCounters c = h[0];
        for (int i = 1; i < NCTR; i++) {
            c.applications += h[i].applications;
            c.nnz_reduced += h[i].nnz_reduced;
            c.segments += h[i].segments;
            c.lpool_overflow += h[i].lpool_overflow;
            c.scatter_overflow += h[i].scatter_overflow;
            c.nonempty_out += h[i].nonempty_out;
            c.nnz_out += h[i].nnz_out;
            c.stream_redo += h[i].stream_redo;
            c.stream_fix += h[i].stream_fix;
            for (int k = 0; k < 16; k++) { c.class_ent[k] += h[i].class_ent[k]; c.class_seg[k] += h[i].class_seg[k]; }
        }
        return c;
    }

    // entries handed out by the fullest region times NPOOL (what a balanced pool would need); synchronises
    u64d pool_used()
    {
        std::vector<u64d> h((size_t)NPOOL * POOL_STRIDE);
        HIPCHK(hipMemcpyAsync(h.data(), pool_ctr.p, h.size() * sizeof(u64d), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        u64d mx = 0;
        for (int r = 0; r < npool_active; r++) mx = std::max(mx, h[(size_t)r * POOL_STRIDE]);
        return mx * (u64d)npool_active;
    }

    // solve + bounds with automatic growth of the multiplier pool; returns the total bound of S
    // returns -1 when the multiplier records of these rows would need more than max_pool entries (the caller then
    // processes fewer rows at a time)
    i64 solve_phase(const DevMat &M, const int *rows, const int *self_idx, int nrows, i64 lpool_guess, i64 max_pool = ((i64)1 << 62))
    {
        i64 pool = std::min<i64>(std::max<i64>(lpool_guess, 1 << 16), max_pool);
        for (;;) {
            alloc_solve(nrows, pool);
            run_solve(M, rows, self_idx, nrows);
            run_bounds(nrows);
            const RoundCounters c = read_counters(nrows); // the counters and the total of the bounds: one round trip
            const i64 tot = s_total_bound;
            if (c.lpool_overflow) {
                if (pool >= max_pool) return -1;
                pool = std::min<i64>(std::max<i64>(pool * 2, (i64)(pool_used() * 5 / 4) + 1024), max_pool);
                continue;
            }
            return tot;
        }
    }

    // ---- (4) SCATTER.  S.ent must hold s_total_bound entries (size_S() after a solve).
    void run_bounds(int nrows)
    {
        scan.exclusive(bound.p, sstart.p, (size_t)nrows + 1, stream);
    }

    i64 fetch_total_bound(int nrows)
    {
        i64d tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, sstart.p + nrows, sizeof(i64d), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        s_total_bound = tot;
        return tot;
    }

    // ---- what the scatter needs once per Round: its streams and events, the opt-in of its kernels to large LDS, the scratch of the
    // last-resort kernel.  Done on the first scatter -- or, by a round, in front of its timed step (warm_scatter): a hipMalloc of
    // gigabytes or the creation of six streams between two launches of the step is milliseconds of an idle device.
    static int n_lanes() { static const int v = [] { const char *e = getenv("SPASM_AMD_STREAM_LANES"); return std::min(4, std::max(1, e ? atoi(e) : 2)); }(); return v; }
    static int n_twins() { static const int v = [] { const char *e = getenv("SPASM_AMD_TWIN_STREAMS"); return std::min(4, std::max(1, e ? atoi(e) : 2)); }(); return v; }
    void ensure_streams()
    {
        if (!side) {
            HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        }
        if (!ev_cls_done[0]) for (auto &e : ev_cls_done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (int l = 1; l < n_lanes(); l++)
            if (!lane_s[l]) {
                HIPCHK(hipStreamCreateWithFlags(&lane_s[l], hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&lane_ev[l], hipEventDisableTiming));
            }
        for (int t = 0; t < n_twins() - 1; t++)
            if (!twin_s[t]) {
                HIPCHK(hipStreamCreateWithFlags(&twin_s[t], hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&twin_ev[t], hipEventDisableTiming));
            }
    }
    void ensure_big_scatter(hipStream_t s)
    {
        if (bigsc_m == m) return;
        const i64 per = std::max<i64>((i64)m, 1) * 13; // bytes per workgroup: 8 accumulator + 4 list + bitmap
        // rows in flight are its throughput; its rows are the handful beyond every LDS table: 2 GiB of scratch at most
        bigsc_blocks = (int)std::max<i64>(1, std::min<i64>((i64)num_cu * 8, ((i64)2 << 30) / per));
        bigsc_m = m;
        const size_t nw = ((size_t)std::max(m, 1) + 31) / 32;
        sc_xdense.alloc((size_t)bigsc_blocks * (size_t)std::max(m, 1));
        sc_bitmap.alloc((size_t)bigsc_blocks * nw);
        sc_touched.alloc((size_t)bigsc_blocks * (size_t)std::max(m, 1));
        sc_xdense.zero(s);
        sc_bitmap.zero(s);
    }
    void warm_scatter()
    {
        ensure_streams();
        ensure_big_scatter(stream);
        ScatterArgs a;
        memset(&a, 0, sizeof a);
        StreamArgs sa;
        memset(&sa, 0, sizeof sa);
        const int nhash = F.small ? kNumHashClasses : kNumHashClasses - 1;
        for (int c = 0; c < nhash; c++) {
            const size_t lds = scatter_lds_bytes(kClasses[c], F.small);
            if (F.small) launch_scatter_class<true>(c, a, 0, lds, stream);
            else launch_scatter_class<false>(c, a, 0, lds, stream);
        }
        for (int c = 0; c < std::min(nhash, kNumStreamClasses); c++) {
            const size_t lds = stream_lds_bytes(stream_logt(c), stream_tpr(c), stream_wpb(c));
            const StreamMode mode = stream_mode(use_w ? wbase + wcap : 0);
            if (F.small) launch_stream_class<true>(c, sa, 0, num_cu, lds, stream, mode);
            else launch_stream_class<false>(c, sa, 0, num_cu, lds, stream, mode);
        }
    }

    void run_scatter(const DevMat &M, const int *rows, int nrows)
    {
        const int4 *recs = Lpool.p;
        S.n = nrows;
        S.m = m;
        nlaunch = 0;
        if (nrows == 0) return;
        // (class_count was cleared by the reset kernel of the solve that precedes every scatter)
        int nhash = F.small ? kNumHashClasses : kNumHashClasses - 1; // 12-byte slots: the 2^14 table exceeds LDS
        // the streaming kernel goes along the rows of W (the plan kernel marks the rows it can take)
        const bool streaming = use_w && !force_lists && !want_idx;
        BinArgs b;
        b.nrows = nrows;
        b.bound = bound.p;
        b.Llen = Llen.p;
        for (int c = 0; c < NCLASS; c++) b.cap[c] = -1;
        for (int c = 0; c < nhash; c++) b.cap[c] = kClasses[c].cap;
        b.lazy_terms = zp_lazy_terms(F);
        // classes nhash..NHASHMAX-2 are unused (cap -1 never matches); class NHASHMAX-1 collects what fits nowhere
        b.class_count = class_count.p;
        b.class_list = class_list.p;
        b.rows = rows;
        b.start = M.start.p;
        b.len = M.len.p;
        b.orig = M.orig.p;
        b.Lstart = Lstart.p;
        b.sstart = sstart.p;
        b.pmask = pmask.p;
        b.sflag = sflag.p;
        b.stream_classes = streaming ? std::min(nhash, kNumStreamClasses) : 0;
        b.Sorig = S.orig.p;
        b.fixcnt = fixcnt.p;
        b.desc = class_desc.p;
        hipLaunchKernelGGL(k_bin, dim3(cdiv(nrows, 1024)), dim3(256), 0, stream, b);
        HIPCHK(hipGetLastError());

        ScatterArgs a;
        a.ent = M.ent.p;
        a.qinv_r = qinv_r.p;
        a.uhdr = uhdr.p;
        a.UPN = UPN.p;
        a.Lpool = recs;
        a.Sent = S.ent.p;
        a.Slen = S.len.p;
        a.Slead = S.lead.p;
        a.ctr = ctr.p;
        a.F = F;
        {
            const char *dbg = getenv("SPASM_DBG"); // timing ablations of the scatter kernel (wrong results when set)
            a.dbg = dbg ? atoi(dbg) : 0;
        }
        a.stamps = nullptr;
#ifdef SPASM_STAMPS
        stamps.ensure(NCLASS * 2 * NSTAMP);
        HIPCHK(hipMemsetAsync(stamps.p, 0, NCLASS * 2 * NSTAMP * sizeof(u64d), stream));
        a.stamps = stamps.p;
#endif
        StreamArgs sa;
        sa.ent = M.ent.p;
        sa.qinv_r = qinv_r.p;
        sa.UPN = UPN.p;
        sa.Lpool = recs;
        sa.Sent = S.ent.p;
        sa.Slen = S.len.p;
        sa.Slead = S.lead.p;
        sa.ctr = ctr.p;
        sa.F = F;
        sa.dbg = a.dbg;
        sa.stamps = a.stamps;
        sa.fixbuf = fixbuf.p;
        sa.fixcnt = fixcnt.p;
        nhash_used = nhash;
        // The classes with the largest tables hold few rows (config 3: 7829 and 51 of 830527), each a long serial job of one
        // workgroup: launched after the others they are a tail on a nearly empty chip (0.27 of 4.1 ms; 74 of 760 us for a
        // 1/8 shard).  They go first, on a side stream, and the wide classes fill the rest of the chip meanwhile.
        const int first_side = 6;
        const bool use_side = !class_timing && (nhash > first_side || streaming);
        if (use_side) {
            ensure_streams();
            HIPCHK(hipEventRecord(ev_fork, stream));
            HIPCHK(hipStreamWaitEvent(side, ev_fork, 0));
        }
        auto mark = [&](int cls_id, hipStream_t s) { // event in front of a launch, for the per-class times
            if (!class_timing || nlaunch >= NCLASS) return;
            HIPCHK(hipEventRecord(ev_cls[nlaunch], s));
            launch_cls[nlaunch++] = cls_id;
        };
        auto launch_class = [&](int c, hipStream_t s) {
            mark(c, s);
            a.cls = c;
            a.class_count = class_count.p + c;
            a.desc = class_desc.p + (size_t)c * nrows;
            const size_t lds = scatter_lds_bytes(kClasses[c], F.small);
            int per_cu = (int)std::min<size_t>(32 / kClasses[c].wpb, (160 * 1024) / lds);
            if (per_cu < 1) per_cu = 1;
            const int rows_per_block = kClasses[c].tpr == 64 ? kClasses[c].wpb : 1;
            const int grid = std::max(1, std::min(cdiv(nrows, rows_per_block), num_cu * per_cu));
            if (F.small) launch_scatter_class<true>(c, a, grid, lds, s);
            else launch_scatter_class<false>(c, a, grid, lds, s);
        };
        // the streaming twin of hash class c; rows it gives up on land in class c's list, which therefore runs after it
        auto launch_stream_cls = [&](int c, hipStream_t s) {
            if (!streaming || c >= kNumStreamClasses) return;
            mark(NSTREAM0 + c, s);
            sa.cls = NSTREAM0 + c;
            sa.class_count = class_count.p + NSTREAM0 + c;
            sa.desc = class_desc.p + (size_t)(NSTREAM0 + c) * nrows;
            sa.redo_count = class_count.p + c;
            sa.redo_desc = class_desc.p + (size_t)c * nrows;
            const size_t lds = stream_lds_bytes(stream_logt(c), stream_tpr(c), stream_wpb(c));
            if (F.small) launch_stream_class<true>(c, sa, nrows, num_cu, lds, s, smode);
            else launch_stream_class<false>(c, sa, nrows, num_cu, lds, s, smode);
        };
        // the duplicates the streaming kernels found are merged afterwards, a wave per row that has any
        auto launch_stream_fix = [&](hipStream_t s) {
            if (!streaming) return;
            mark(NCLASS - 1, s); // (reported as class 15)
            StreamFixArgs fa;
            fa.nrows = nrows;
            fa.fixcnt = fixcnt.p;
            fa.fixbuf = fixbuf.p;
            fa.sstart = sstart.p;
            fa.Sent = S.ent.p;
            fa.Slen = S.len.p;
            fa.Slead = S.lead.p;
            fa.ctr = ctr.p;
            fa.F = F;
            hipLaunchKernelGGL(k_stream_fix, dim3(cdiv(nrows, 64)), dim3(256), 0, s, fa);
            HIPCHK(hipGetLastError());
        };
        auto launch_big = [&](hipStream_t s) {
            // rows that fit no LDS table: the last class, through the global-memory kernel
            ensure_big_scatter(s);
            mark(NHASHMAX - 1, s);
            BigScatterArgs bb;
            bb.s = a;
            bb.s.cls = NHASHMAX - 1;
            bb.s.class_count = class_count.p + (NHASHMAX - 1);
            bb.s.desc = class_desc.p + (size_t)(NHASHMAX - 1) * nrows;
            bb.m = std::max(m, 1);
            bb.nwords = (std::max(m, 1) + 31) / 32;
            bb.xdense = sc_xdense.p;
            bb.bitmap = sc_bitmap.p;
            bb.touched = sc_touched.p;
            hipLaunchKernelGGL(k_scatter_big, dim3(bigsc_blocks), dim3(256), 0, s, bb);
            HIPCHK(hipGetLastError());
        };
        if (use_side && streaming) {
            // the streaming kernels on the main stream, longest rows first; the hash-table kernel of a class -- it only gets what its
            // streaming twin hands back -- follows that twin on the side stream, beside the streaming kernels of the shorter rows
            // several lanes: the streaming kernels go round-robin over a few streams, so that the workgroups of the next classes
            // fill the chip while the last ones of a class drain (config 3: 2.68 ms per step on one lane, 2.38 on two)
            const int lanes = n_lanes();
            for (int l = 1; l < lanes; l++) HIPCHK(hipStreamWaitEvent(lane_s[l], ev_fork, 0));
            // the hash-table twins (a handful of rows each: 20 - 50 us of one or two workgroups whatever the shard size) run two
            // abreast on streams of their own: chained on one stream they were 0.15 ms of a 0.6 ms step of a 1/8 shard
            // (HIP multiplexes streams over four hardware queues: with more than four streams in play a twin waiting for its event
            // blocks the streaming kernels queued behind it -- 2.4 -> 3.0 ms per step with six streams; four it is)
            const int ntwin = n_twins();
            for (int c = nhash - 1; c >= 0; c--) {
                const int l = (nhash - 1 - c) % lanes;
                hipStream_t lane = l ? lane_s[l] : stream;
                launch_stream_cls(c, lane);
                HIPCHK(hipEventRecord(ev_cls_done[c], lane));
                const int t = (nhash - 1 - c) % ntwin;
                hipStream_t tw = t ? twin_s[t - 1] : side;
                HIPCHK(hipStreamWaitEvent(tw, ev_cls_done[c], 0));
                launch_class(c, tw);
            }
            for (int l = 1; l < lanes; l++) {
                HIPCHK(hipEventRecord(lane_ev[l], lane_s[l]));
                HIPCHK(hipStreamWaitEvent(stream, lane_ev[l], 0));
            }
            for (int t = 0; t < ntwin - 1; t++) {
                HIPCHK(hipEventRecord(twin_ev[t], twin_s[t]));
                HIPCHK(hipStreamWaitEvent(stream, twin_ev[t], 0));
            }
            launch_stream_fix(stream);
            launch_big(side);
            HIPCHK(hipEventRecord(ev_join, side));
            HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
        } else if (use_side) {
            for (int c = nhash - 1; c >= first_side; c--) launch_class(c, side); // longest rows first
            launch_big(side);
            HIPCHK(hipEventRecord(ev_join, side));
            for (int c = 0; c < first_side; c++) launch_class(c, stream);
            HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
        } else {
            for (int c = nhash - 1; c >= 0; c--) launch_stream_cls(c, stream);
            launch_stream_fix(stream);
            for (int c = 0; c < nhash; c++) launch_class(c, stream);
            launch_big(stream);
            if (class_timing) HIPCHK(hipEventRecord(ev_cls[nlaunch], stream));
        }
        hipLaunchKernelGGL(k_scatter_mark_failed, dim3(cdiv(nrows, 256)), dim3(256), 0, stream, nrows, Llen.p, S.len.p, S.lead.p);
        HIPCHK(hipGetLastError());
        // the Schur rows start where their slots start
        HIPCHK(hipMemcpyAsync(S.start.p, sstart.p, ((size_t)nrows + 1) * sizeof(i64d), hipMemcpyDeviceToDevice, stream));
    }

    void fetch_counters()
    {
        hctr = read_counters();
        int *cc = hclass_count;
        HIPCHK(hipMemcpyAsync(cc, class_count.p, NCLASS * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
#ifdef SPASM_STAMPS
        {
            std::vector<u64d> h(NCLASS * 2 * NSTAMP);
            HIPCHK(hipMemcpy(h.data(), stamps.p, h.size() * sizeof(u64d), hipMemcpyDeviceToHost));
            static const char *names[NSTAMP] = {"prologue", "issue", "wait-loads", "own", "rounds", "remainder", "sweep", "-"};
            static const char *snames[NSTAMP] = {"top+own", "chunks", "next-req", "rowend", "reset", "rotate", "-", "-"};
            for (int c = NSTREAM0; c < NCLASS; c++) {
                const double waves = (double)h[(size_t)c * 2 * NSTAMP + NSTAMP];
                if (waves == 0) continue;
                fprintf(stderr, "[stamps] stream class %d rows %d waves %.0f: cycles per wave:", c - NSTREAM0, cc[c], waves);
                for (int i = 0; i < 6; i++) fprintf(stderr, " %s=%.0f", snames[i], (double)h[(size_t)c * 2 * NSTAMP + i] / waves);
                fprintf(stderr, "\n");
            }
            for (int c = 0; c < NHASHMAX; c++) {
                const double waves = (double)h[(size_t)c * 2 * NSTAMP + NSTAMP];
                if (waves == 0) continue;
                fprintf(stderr, "[stamps] class %d rows %d waves %.0f: cycles per wave:", c, cc[c], waves);
                for (int i = 0; i < 7; i++) fprintf(stderr, " %s=%.0f", names[i], (double)h[(size_t)c * 2 * NSTAMP + i] / waves);
                fprintf(stderr, "\n");
            }
        }
#endif
        if (hctr.lpool_overflow) throw EngineError("multiplier pool exhausted");
        if (hctr.scatter_overflow) throw EngineError("a hash table of the scatter kernel filled up (internal bound violated)");
    }
};

// ------------------------------------------------------------------------------------------------
// host CSR -> device matrix
// ------------------------------------------------------------------------------------------------
void upload_csr_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride, DevMat &M, hipStream_t s);

void upload_csr(const struct spasm_csr *A, int row_lo, int row_hi, DevMat &M, hipStream_t s)
{
    const int n = row_hi - row_lo;
    const i64 base = A->p[row_lo];
    const i64 nnz = A->p[row_hi] - base;
    M.n = n;
    M.m = A->m;
    M.start.ensure((size_t)n + 1);
    M.len.ensure((size_t)n + 1);
    M.lead.ensure((size_t)n + 1);
    M.orig.ensure((size_t)n + 1);
    M.ent.ensure((size_t)nnz + 1);
    DevBuf<i64d> dp;
    DevBuf<int> dj, dx;
    dp.alloc((size_t)n + 1);
    dj.alloc((size_t)nnz + 1);
    dx.alloc((size_t)nnz + 1);
    // row pointers relative to the shard
    std::vector<i64d> hp((size_t)n + 1);
    for (int i = 0; i <= n; i++) hp[(size_t)i] = A->p[row_lo + i] - base;
    HIPCHK(hipMemcpyAsync(dp.p, hp.data(), ((size_t)n + 1) * sizeof(i64d), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(dj.p, A->j + base, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        if (A->x) HIPCHK(hipMemcpyAsync(dx.p, A->x + base, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_entries, dim3(std::min<i64>(cdiv(nnz, 256), 65536)), dim3(256), 0, s, (i64d)nnz, zp_field_make(A->field->p), dj.p,
                           A->x ? dx.p : nullptr, M.ent.p);
        HIPCHK(hipGetLastError());
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_pack_rows, dim3(cdiv(n, 256)), dim3(256), 0, s, n, row_lo, 1, dp.p, M.start.p, M.len.p, M.orig.p);
        HIPCHK(hipGetLastError());
        constexpr int TEAM = 8;
        if (A->x) hipLaunchKernelGGL((k_drop_zeros<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, M.start.p, M.len.p, M.ent.p);
        hipLaunchKernelGGL((k_row_lead<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, M.start.p, M.len.p, M.ent.p, M.lead.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s)); // hp and the staging buffers go out of scope
}

// rows row_lo, row_lo + stride, ... < row_hi of A, gathered on the host and uploaded as one matrix
void upload_csr_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride, DevMat &M, hipStream_t s)
{
    if (stride <= 1) { upload_csr(A, row_lo, row_hi, M, s); return; }
    const int n = row_hi > row_lo ? (row_hi - row_lo + stride - 1) / stride : 0;
    std::vector<i64d> hp((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) { const int g = row_lo + i * stride; hp[(size_t)i + 1] = hp[(size_t)i] + (A->p[g + 1] - A->p[g]); }
    const i64 nnz = hp[(size_t)n];
    std::vector<int> hj((size_t)nnz + 1), hx((size_t)nnz + 1);
    for (int i = 0; i < n; i++) {
        const int g = row_lo + i * stride;
        const i64 len = A->p[g + 1] - A->p[g];
        memcpy(hj.data() + hp[(size_t)i], A->j + A->p[g], sizeof(int) * (size_t)len);
        if (A->x) memcpy(hx.data() + hp[(size_t)i], A->x + A->p[g], sizeof(int) * (size_t)len);
    }
    M.n = n;
    M.m = A->m;
    M.start.ensure((size_t)n + 1);
    M.len.ensure((size_t)n + 1);
    M.lead.ensure((size_t)n + 1);
    M.orig.ensure((size_t)n + 1);
    M.ent.ensure((size_t)nnz + 1);
    DevBuf<i64d> dp;
    DevBuf<int> dj, dx;
    dp.alloc((size_t)n + 1);
    dj.alloc((size_t)nnz + 1);
    dx.alloc((size_t)nnz + 1);
    HIPCHK(hipMemcpyAsync(dp.p, hp.data(), ((size_t)n + 1) * sizeof(i64d), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(dj.p, hj.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        if (A->x) HIPCHK(hipMemcpyAsync(dx.p, hx.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_entries, dim3(std::min<i64>(cdiv(nnz, 256), 65536)), dim3(256), 0, s, (i64d)nnz, zp_field_make(A->field->p), dj.p,
                           A->x ? dx.p : nullptr, M.ent.p);
        HIPCHK(hipGetLastError());
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_pack_rows, dim3(cdiv(n, 256)), dim3(256), 0, s, n, row_lo, stride, dp.p, M.start.p, M.len.p, M.orig.p);
        HIPCHK(hipGetLastError());
        constexpr int TEAM = 8;
        if (A->x) hipLaunchKernelGGL((k_drop_zeros<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, M.start.p, M.len.p, M.ent.p);
        hipLaunchKernelGGL((k_row_lead<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, M.start.p, M.len.p, M.ent.p, M.lead.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
}

void require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) throw EngineError("no HIP device: the MI355X engine has no CPU fallback");
}

void check_input(const struct spasm_csr *A, const char *who)
{
    if (!A) throw EngineError(std::string(who) + ": NULL matrix");
    const i64 p = A->field->p;
    if (p <= 2 || p > 0xfffffffbLL) throw EngineError(std::string(who) + ": prime out of range (2 < p <= 0xfffffffb)");
    if (!A->x && A->p[A->n] > 0) throw EngineError(std::string(who) + ": matrix without values");
}

thread_local std::vector<spasm_amd_round_stats> g_last_rounds;
thread_local int g_multi_finish = 0; // how the last spasm_amd_echelonize_multi finished (spasm_amd_multi_last_finish)
// the dense eliminations of the last echelonize call of this thread (spasm_amd_dense_stats): how many, then of the LAST one its
// kind (1 int8 one digit, 2 int8 two digits, 3 f64 panels, 4 rank-1 updates), rows, columns, block width (KB; 64 for the f64
// panels, 1 for the rank-1 updates); tall-and-skinny finishes, panels the tall panels redid in place, spare
thread_local i64 g_dense_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
inline void dense_stats_note(int kind, int R, int C, int block)
{
    g_dense_stats[0]++;
    g_dense_stats[1] = kind; g_dense_stats[2] = R; g_dense_stats[3] = C; g_dense_stats[4] = block;
}

i64 read_bytes_of(const RoundCounters &c, int m) { return 8 * (i64)c.nnz_reduced + 16 * (i64)c.segments + 4 * (i64)m; }

void fill_stats(spasm_amd_round_stats &st, const Round &R, int round, int rows_in, i64 nnz_in)
{
    memset(&st, 0, sizeof st);
    st.round = round;
    st.rows_in = rows_in;
    st.nnz_in = nnz_in;
    st.npiv = R.npiv;
    st.npiv_open = R.n_open;
    st.npiv_greedy = R.n_greedy;
    st.rows_out = R.hctr.nonempty_out;
    st.nnz_out = (i64)R.hctr.nnz_out;
    st.nnz_reduced = (i64)R.hctr.nnz_reduced;
    st.applications = (i64)R.hctr.applications;
    st.read_bytes = read_bytes_of(R.hctr, R.m);
    float ms = 0;
    if (hipEventElapsedTime(&ms, R.ev[0], R.ev[1]) == hipSuccess) st.ms_pivots = ms;
    if (hipEventElapsedTime(&ms, R.ev[1], R.ev[2]) == hipSuccess) st.ms_solve = ms;
    if (hipEventElapsedTime(&ms, R.ev[2], R.ev[3]) == hipSuccess) st.ms_scatter = ms;
    if (hipEventElapsedTime(&ms, R.ev[0], R.ev[3]) == hipSuccess) st.ms_total = ms;
    for (int i = 0; i < R.nlaunch; i++)
        if (R.class_timing && hipEventElapsedTime(&ms, R.ev_cls[i], R.ev_cls[i + 1]) == hipSuccess) st.ms_class[R.launch_cls[i]] = ms;
    for (int c = 0; c < NCLASS; c++) {
        st.rows_class[c] = R.hclass_count[c];
        st.ent_class[c] = (i64)R.hctr.class_ent[c];
        st.seg_class[c] = (i64)R.hctr.class_seg[c];
    }
    st.stream_fix = R.hctr.stream_fix;
    st.stream_redo = R.hctr.stream_redo;
    st.ms_uinv = R.ms_uinv;
    st.ms_w = R.ms_w;
    st.ms_levels = R.ms_levels;
    st.ms_w_sizing = R.ms_w_sizing;
    if (R.use_w) {
        if (R.ev_w[0] && hipEventElapsedTime(&ms, R.ev_w[0], R.ev_w[1]) == hipSuccess) st.ms_wbuild = ms;
        st.w_levels = R.depth + 1;
        st.w_entries = R.w_entries;
        st.w_long_rows = R.w_long_rows;
    }
    (void)hipGetLastError(); // (an event that was never recorded makes hipEventElapsedTime fail: not an error of the engine)
}

// malloc'ed, uninitialised, geometrically growing int array whose buffer ends up in the spasm_csr the caller frees: the entries
// of U go device -> this buffer -> caller, without a value-initialising resize (a memset of gigabytes) or a final copy
struct HostInts {
    int *ptr = nullptr;
    size_t n = 0, cap = 0;
    HostInts() {}
    HostInts(const HostInts &) = delete;
    HostInts &operator=(const HostInts &) = delete;
    ~HostInts() { free(ptr); }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    int *data() { return ptr; }
    int *grow(size_t count) // room for `count` more; returns where they go
    {
        if (n + count > cap) {
            const size_t want = std::max(n + count, cap + cap / 2 + 1024);
            int *q = (int *)realloc(ptr, want * sizeof(int));
            if (!q) throw EngineError("out of host memory for U");
            ptr = q;
            cap = want;
        }
        int *at = ptr + n;
        n += count;
        return at;
    }
    int *steal() { int *q = ptr; ptr = nullptr; n = cap = 0; return q; }
};

struct HostU {
    std::vector<i64> p;      // row pointers
    HostInts j, x;
    std::vector<int> pivcol; // pivot column of each row
    std::vector<int> orig;   // originating row of the input
    // rank only (spasm_amd_rank): the rows of U are counted, their entries never leave the device -- at config 5's scale they are
    // what outgrows the host (10^10 entries and more), not anything the device holds
    bool rank_only = false;
    i64 uncollected = 0;     // pivots counted without a row of U to show for them
};

// entries of pivot rows (device, {col,val} pairs) appended to the host arrays of U: split on the device, downloaded straight
// into the tails of U.j / U.x (was: a host copy of the pairs and 2 x nnz push_backs -- a third of config 2's echelonize)
void append_entries(HostU &U, const int2 *dent, i64 count, hipStream_t s)
{
    if (count <= 0 || U.rank_only) return;
    DevBuf<int> dj, dx;
    dj.alloc((size_t)count);
    dx.alloc((size_t)count);
    hipLaunchKernelGGL(k_split_ent, dim3((unsigned)std::min<i64>((count + 255) / 256, 65536)), dim3(256), 0, s, (i64d)count, dent, dj.p, dx.p);
    HIPCHK(hipGetLastError());
    int *hj = U.j.grow((size_t)count), *hx = U.x.grow((size_t)count);
    HIPCHK(hipMemcpyAsync(hj, dj.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hx, dx.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
}

// append the pivot rows of a round (device) to the host copy of U
void append_round_U(HostU &U, const Round &R, const DevMat &A, hipStream_t s)
{
    const int np = R.npiv;
    if (np == 0) return;
    std::vector<i64d> off((size_t)np + 1);
    std::vector<int> pc((size_t)np), pr((size_t)np);
    std::vector<int> orig((size_t)A.n);
    HIPCHK(hipMemcpyAsync(off.data(), R.uoff.p, ((size_t)np + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pc.data(), R.pivcol.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pr.data(), R.pivrow.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    if (A.n > 0) HIPCHK(hipMemcpyAsync(orig.data(), A.orig.p, (size_t)A.n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 base = U.p.back();
    for (int k = 0; k < np; k++) {
        U.p.push_back(base + off[(size_t)k + 1]);
        U.pivcol.push_back(pc[(size_t)k]);
        U.orig.push_back(orig[(size_t)pr[(size_t)k]]);
    }
    append_entries(U, R.Ufull.p, R.utotal, s);
}

// ------------------------------------------------------------------------------------------------
// dense tail: leftmost-pivot elimination of the live part of `M`; its pivot rows are appended to U
// ------------------------------------------------------------------------------------------------
// cells the dense finish may hold: a third of the free device memory in bytes (beside it: the dense W of a slab of columns, the
// digit planes of a block, the rows of U it emits), at least 2^31 cells; elem = bytes per cell (dense_elem_bytes)
// The hand-off to the dense finish is decided by the SHAPE: at most 2^36 bytes of dense matrix (64 GiB: a quarter of an MI355X,
// beside the dense W of a slab of columns, the digit planes of a block and the rows of U it emits).  Free memory only vetoes
// (a shared or smaller device): the caller then stays with sparse rounds, and the veto is logged, since with "FL on columns" the
// pivot columns depend on where the sparse rounds stop.
i64 dense_max_entries(int elem = 4)
{
    const i64 by_shape = ((i64)1 << 36) / std::max(elem, 1);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return by_shape;
    const i64 by_memory = (i64)(fr / 3) / std::max(elem, 1);
    if (by_memory < by_shape) {
        static bool said = false;
        if (!said) spasm_logf("[echelonize] dense finish capped by free device memory (%.1f GiB free): %lld cells instead of %lld\n", (double)fr / 1073741824.0,
                              (long long)by_memory, (long long)by_shape);
        said = true;
        return by_memory;
    }
    return by_shape;
}

// which element type the dense matrix of a finish gets: bytes / shorts when the int8 path of dense.hpp will take it (its block
// updates are bound by reading and writing D), ints otherwise (f64 panels, rank-1 updates)
int dense_elem_bytes(const ZpField &F, i64 R)
{
    const char *force64 = getenv("SPASM_AMD_DENSE_F64"); // diagnostics: the f64 panels for every prime
    if (!F.small || (force64 && atoi(force64))) return 4;
    if ((R + 255) / 256 > 65536) return 4; // more rows than the panel kernel takes (64 per thread of 256 workgroups)
    return F.p <= 255 ? 1 : 2;
}

// The pivot rows of the dense columns [c_lo, c_hi) of an eliminated (or partly eliminated: the pivot rows of those columns are final)
// dense matrix, appended to U.  Returns how many.
// (device buffers of the extraction, kept between calls: hipFree waits for the whole device, which would end the overlap)
struct ExtractWork {
    Scanner scan;
    DevBuf<int> pflag, pscan, pivcol, porig, dj, dx;
    DevBuf<i64d> ulen, uoff;
    DevBuf<int2> Ufull;
    // Device -> pageable host memory runs at ~7 GB/s (the runtime stages it through its own pinned chunks, one host thread copying):
    // the 21 GB of U of a 73k x 73k finish took 3.1 s, longer than the elimination.  Two pinned buffers of our own instead: the DMA of
    // piece i + 1 runs while piece i is copied out by all host threads.
    static constexpr size_t PIN_BYTES = (size_t)64 << 20;
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t pev[2] = {nullptr, nullptr};
    ExtractWork() {}
    ExtractWork(const ExtractWork &) = delete;
    ~ExtractWork()
    {
        for (int b = 0; b < 2; b++) {
            if (pin[b]) (void)hipHostFree(pin[b]);
            if (pev[b]) (void)hipEventDestroy(pev[b]);
        }
    }
    void d2h(void *dst, const void *src, size_t bytes, hipStream_t s)
    {
        if (bytes < ((size_t)8 << 20)) {
            HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            return;
        }
        for (int b = 0; b < 2; b++) {
            if (!pin[b]) HIPCHK(hipHostMalloc(&pin[b], PIN_BYTES, hipHostMallocDefault));
            if (!pev[b]) HIPCHK(hipEventCreateWithFlags(&pev[b], hipEventDisableTiming));
        }
        const size_t npieces = (bytes + PIN_BYTES - 1) / PIN_BYTES;
        auto piece = [&](size_t i) { return std::min(PIN_BYTES, bytes - i * PIN_BYTES); };
        HIPCHK(hipMemcpyAsync(pin[0], src, piece(0), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(pev[0], s));
        for (size_t i = 0; i < npieces; i++) {
            const int b = (int)(i & 1);
            if (i + 1 < npieces) {
                HIPCHK(hipMemcpyAsync(pin[b ^ 1], (const char *)src + (i + 1) * PIN_BYTES, piece(i + 1), hipMemcpyDeviceToHost, s));
                HIPCHK(hipEventRecord(pev[b ^ 1], s));
            }
            HIPCHK(hipEventSynchronize(pev[b]));
            const size_t n = piece(i);
            char *out = (char *)dst + i * PIN_BYTES;
            const char *in = (const char *)pin[b];
            const size_t part = (size_t)4 << 20;
            const long long nparts = (long long)((n + part - 1) / part);
#pragma omp parallel for schedule(static) num_threads(8)
            for (long long q = 0; q < nparts; q++) memcpy(out + (size_t)q * part, in + (size_t)q * part, std::min(part, n - (size_t)q * part));
        }
    }
};

template <typename DT>
int dense_extract_range(const DT *Dp, int C, i64 ldc, const int *pivrow_of_col, int c_lo, int c_hi, const int *clist, const int *row_orig, HostU &U, ExtractWork &W,
                        hipStream_t s)
{
    const int nc = c_hi - c_lo;
    if (nc <= 0) return 0;
    Scanner &scan = W.scan;
    DevBuf<int> &pflag = W.pflag, &pscan = W.pscan;
    pflag.ensure((size_t)nc + 1); pscan.ensure((size_t)nc + 1);
    hipLaunchKernelGGL(k_flag_nonneg, dim3(cdiv((i64)nc + 1, 256)), dim3(256), 0, s, nc, pivrow_of_col + c_lo, pflag.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(pflag.p, pscan.p, (size_t)nc + 1, s);
    int npd = 0;
    HIPCHK(hipMemcpyAsync(&npd, pscan.p + nc, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (npd == 0) return 0;
    if (U.rank_only) { U.uncollected += npd; return npd; }
    DevBuf<i64d> &ulen = W.ulen, &uoff = W.uoff;
    ulen.ensure((size_t)npd + 1024); uoff.ensure((size_t)npd + 1024);
    HIPCHK(hipMemsetAsync(ulen.p, 0, ((size_t)npd + 1) * sizeof(i64d), s));
    hipLaunchKernelGGL((k_dense_count<DT>), dim3(nc), dim3(256), 0, s, C, Dp, (i64d)ldc, pivrow_of_col, pscan.p, ulen.p, c_lo);
    HIPCHK(hipGetLastError());
    scan.exclusive(ulen.p, uoff.p, (size_t)npd + 1, s);
    i64d tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, uoff.p + npd, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    DevBuf<int2> &Ufull = W.Ufull;
    DevBuf<int> &pivcol = W.pivcol, &porig = W.porig;
    // (a quarter more than asked for: a later call that needs a little more must not free -- hipFree waits for the whole device)
    if ((size_t)tot + 1 > Ufull.n) Ufull.alloc((size_t)tot + (size_t)tot / 4 + 1024);
    pivcol.ensure((size_t)npd + 1024); porig.ensure((size_t)npd + 1024);
    hipLaunchKernelGGL((k_dense_emit<DT>), dim3(nc), dim3(64), 0, s, C, Dp, (i64d)ldc, pivrow_of_col, pscan.p, uoff.p, clist, row_orig, Ufull.p, pivcol.p, porig.p, c_lo);
    HIPCHK(hipGetLastError());
    std::vector<i64d> off((size_t)npd + 1);
    std::vector<int> pc((size_t)npd), po((size_t)npd);
    HIPCHK(hipMemcpyAsync(off.data(), uoff.p, ((size_t)npd + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pc.data(), pivcol.p, (size_t)npd * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(po.data(), porig.p, (size_t)npd * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 base = U.p.back();
    for (int k = 0; k < npd; k++) {
        U.p.push_back(base + off[(size_t)k + 1]);
        U.pivcol.push_back(pc[(size_t)k]);
        U.orig.push_back(po[(size_t)k]);
    }
    if (tot > 0) {
        if ((size_t)tot > W.dj.n) { W.dj.alloc((size_t)tot + (size_t)tot / 4 + 1024); W.dx.alloc(W.dj.n); }
        hipLaunchKernelGGL(k_split_ent, dim3((unsigned)std::min<i64>(((i64)tot + 255) / 256, 65536)), dim3(256), 0, s, (i64d)tot, Ufull.p, W.dj.p, W.dx.p);
        HIPCHK(hipGetLastError());
        int *hj = U.j.grow((size_t)tot), *hx = U.x.grow((size_t)tot);
        W.d2h(hj, W.dj.p, (size_t)tot * sizeof(int), s);
        W.d2h(hx, W.dx.p, (size_t)tot * sizeof(int), s);
    }
    return npd;
}

// The rows of U of a dense elimination on their way to the host WHILE it runs: the pivot rows of a block of columns are final when
// the block is done (its pivot rows were updated right of the block last), so the block before the one the device works on is
// extracted and copied on a stream of its own (a 10^9-entry U took as long to download as the elimination took: 1.0 of 1.9 s for
// config 5 at 1/5).  The host blocks in the copies; the device has the current block's launches queued by then.
struct UStreamer {
    const void *Dp = nullptr;
    int C = 0;
    i64 ldc = 0;
    const int *pivrow_of_col = nullptr, *clist = nullptr, *row_orig = nullptr;
    HostU *U = nullptr;
    hipStream_t s2 = nullptr;
    hipEvent_t ev = nullptr;
    ExtractWork work;
    int done_to = 0, found = 0;
    double seconds = 0;
    UStreamer() {}
    UStreamer(const UStreamer &) = delete;
    ~UStreamer()
    {
        if (ev) (void)hipEventDestroy(ev);
        if (s2) (void)hipStreamDestroy(s2);
    }
    void init(const void *Dp_, int C_, i64 ldc_, const int *pc, const int *clist_, const int *row_orig_, HostU &U_)
    {
        Dp = Dp_; C = C_; ldc = ldc_; pivrow_of_col = pc; clist = clist_; row_orig = row_orig_; U = &U_;
        HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    // everything queued on `main` so far finishes the columns below c_hi: remember the point ..
    void mark(hipStream_t main) { HIPCHK(hipEventRecord(ev, main)); }
    // .. and (later, with more work queued on the main stream) take the pivot rows of [done_to, c_hi)
    template <typename DT> void take(int c_hi)
    {
        if (c_hi <= done_to) return;
        const double t0 = spasm_wtime();
        HIPCHK(hipStreamWaitEvent(s2, ev, 0));
        found += dense_extract_range((const DT *)Dp, C, ldc, pivrow_of_col, done_to, c_hi, clist, row_orig, *U, work, s2);
        done_to = c_hi;
        seconds += spasm_wtime() - t0;
    }
};

template <typename DT>
bool dense_eliminate_i8(DevBuf<DT> &D, int R, int C, i64 ldc, const ZpField &F, DevBuf<int> &pivrow_of_col, hipStream_t s, UStreamer *us = nullptr)
{
    static int num_cu = 0;
    if (!num_cu) {
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        HIPCHK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    }
    const int ND = F.p <= 255 ? 1 : 2;
    int KB = 1024;
    if (const char *e = getenv("SPASM_AMD_DENSE_KB")) KB = std::min(2048, std::max(64, atoi(e) / 64 * 64)); // tests: several blocks on small matrices
    // rows per workgroup of the panel kernel: a multiple of 64; resident in LDS when they fit (144 KB: 2304 rows of bytes for
    // p < 2^8, 1152 rows of shorts otherwise)
    int G = num_cu;
    int chunk = (int)((((i64)R + G - 1) / G + 63) / 64 * 64);
    if (chunk > 65536) return false; // (64 rows per thread at most)
    G = (int)(((i64)R + chunk - 1) / chunk);
    const int Rp = G * chunk;
    const int xbytes = ND == 1 ? 1 : 2;
    const int lds_rows = 147456 / (DP_W * xbytes);
    const char *force_global = getenv("SPASM_AMD_PANEL_GLOBAL"); // tests: the in-place variant on small matrices
    const bool inlds = chunk <= lds_rows && !(force_global && atoi(force_global));
    // more rows than fit: the first num_cu * res_chunk rows stay LDS-resident and elect the pivots, the others follow (dense.hpp,
    // k_panel_follow).  SPASM_AMD_PANEL_RES_ROWS (tests): rows per workgroup that count as fitting.
    int res_chunk = lds_rows / 64 * 64;
    if (const char *e = getenv("SPASM_AMD_PANEL_RES_ROWS")) res_chunk = std::min(res_chunk, std::max(64, atoi(e) / 64 * 64));
    const char *no_follow = getenv("SPASM_AMD_PANEL_NO_FOLLOW"); // A/B: the in-place variant for tall matrices, as before
    int G_res = num_cu;
    if (const char *e = getenv("SPASM_AMD_PANEL_RES_WGS")) G_res = std::min(num_cu, std::max(1, atoi(e))); // tests: resident workgroups
    const i64 R_res = (i64)G_res * res_chunk; // (< Rp when tall)
    const bool tall = R_res < (i64)R && !(force_global && atoi(force_global)) && !(no_follow && atoi(no_follow));
    const int fol_chunk = std::min(res_chunk, (int)((147456 - (int)sizeof(int) * (DP_W * DP_W + DP_W) - 1024) / (DP_W * xbytes) / 64 * 64));
    const int G_fol = tall ? (int)((Rp - R_res + fol_chunk - 1) / fol_chunk) : 0;
    DevBuf<int> follow_flag;
    if (tall) follow_flag.alloc(1);
    int redone = 0, npanels_done = 0;
    const int Cp = (int)ldc + 256; // (the GEMM stages whole tiles of 128 or 256 columns of Ut, starting at any multiple of 64)
    DevBuf<DT> P;
    DevBuf<int> seq, candrow, invtab;
    DevBuf<signed char> Fd, Ut;
    DevBuf<PanelInfo> info;
    DevBuf<PanelSync> sync;
    DevBuf<DenseState> st;
    const int npanel = KB / DP_W;
    const i64 fplane = (i64)Rp * KB, uplane = (i64)Cp * KB;
    P.alloc((size_t)DP_W * (size_t)Rp);
    seq.alloc((size_t)Rp);
    candrow.alloc((size_t)2 * std::max(G, num_cu) * DP_REC);
    Fd.alloc((size_t)ND * (size_t)fplane);
    Ut.alloc((size_t)ND * (size_t)uplane);
    info.alloc((size_t)npanel);
    sync.alloc(1);
    st.alloc(1);
    st.zero(s);
    DevBuf<unsigned long long> stamps; // diagnostics: phase times of the panel kernel's columns (workgroup 0), 100 MHz ticks
    if (const char *e = getenv("SPASM_AMD_PANEL_STAMPS")) if (atoi(e)) { stamps.alloc(DP_W * 8); stamps.zero(s); }
    invtab.alloc((size_t)F.p);
    hipLaunchKernelGGL(k_inv_table, dim3(cdiv(F.p, 256)), dim3(256), 0, s, (int)F.p, invtab.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(seq.p, 0xff, (size_t)Rp * sizeof(int), s));
    HIPCHK(hipMemsetAsync(pivrow_of_col.p, 0xff, ((size_t)C + 1) * sizeof(int), s));
    const size_t lds = inlds ? (size_t)chunk * DP_W * (size_t)xbytes : 0;
    static bool attr_done_dev[kMaxDev] = {false}; // (per device, and per element type: this function is a template)
    bool &attr_done = attr_done_dev[current_device()];
    if (!attr_done) {
        HIPCHK(hipFuncSetAttribute((const void *)k_panel_lu<true, 1024, DT>, hipFuncAttributeMaxDynamicSharedMemorySize, 147456));
        HIPCHK(hipFuncSetAttribute((const void *)k_panel_follow<1024, DT>, hipFuncAttributeMaxDynamicSharedMemorySize, 147456 - (int)sizeof(int) * (DP_W * DP_W + DP_W) - 1024));
        attr_done = true;
    }
    // The panel kernel's own grid barrier needs every workgroup of a launch resident at once (a plain launch does not check it, as
    // the cooperative launch did): ask the runtime how many fit and refuse cleanly instead of spinning into the barrier's timeout.
    {
        auto fits = [&](const void *fn, int wgs, size_t dyn, const char *what) {
            int per_cu = 0;
            HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 1024, dyn));
            if ((i64)wgs > (i64)per_cu * num_cu)
                throw EngineError(std::string("dense finish: the ") + what + " panel kernel needs " + std::to_string(wgs) + " resident workgroups, the device holds " +
                                  std::to_string((i64)per_cu * num_cu));
        };
        const void *fn_lds = (const void *)k_panel_lu<true, 1024, DT>, *fn_glb = (const void *)k_panel_lu<false, 1024, DT>;
        if (tall) {
            fits(fn_lds, G_res, (size_t)res_chunk * DP_W * (size_t)xbytes, "LDS-resident");
            fits(fn_glb, G, 0, "in-place");
        } else
            fits(inlds ? fn_lds : fn_glb, G, lds, inlds ? "LDS-resident" : "in-place");
    }
    const char *glds_env = getenv("SPASM_AMD_GEMM_GLDS"); // A/B: the 256 x 256 LDS-DMA kernel for the large one-digit updates
    const bool glds_tile = glds_env && atoi(glds_env) != 0;
    if constexpr (std::is_same<DT, signed char>::value) {
        if (glds_tile) HIPCHK(hipFuncSetAttribute((const void *)k_gemm_i8_glds<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, GL_LDS_BYTES));
    }
    auto gemm = [&](int ja, int jb, int k0, int K, const int *rows, int nrows) {
        if (jb <= ja || K <= 0) return;
        // (1-D grid: the kernel orders the tiles itself, in bands of row tiles; a partial last band has fewer row tiles, and its
        // tiles still number rows_in_band * ntn, so the total is simply ntm * ntn)
        const int ntm = cdiv(rows ? nrows : R, 128);
        if (ND == 1 && glds_tile && !rows && K >= 256 && jb - ja >= 1024 && R >= 4096 && std::is_same<DT, signed char>::value) {
            // the large updates of the one-digit finish: 256 x 256 tile, operands by LDS-DMA, loads in flight across barriers
            if constexpr (std::is_same<DT, signed char>::value) {
                const int ntm2 = cdiv(R, GL_BM), ntn2 = cdiv(jb - ja, GL_BN);
                hipLaunchKernelGGL((k_gemm_i8_glds<DT>), dim3((unsigned)((i64)ntm2 * ntn2)), dim3(512), GL_LDS_BYTES, s, R, ja, jb, k0, K, F, D.p, (i64d)ldc, seq.p, Fd.p, Ut.p,
                                   KB, ntm2, ntn2);
            }
        } else if (ND == 1) {
            const int ntn = cdiv(jb - ja, 128);
            hipLaunchKernelGGL((k_gemm_i8<1, 2, 2, 2, 2, DT>), dim3((unsigned)((i64)ntm * ntn)), dim3(256), 0, s, R, ja, jb, k0, K, F, D.p, (i64d)ldc, seq.p, rows, nrows,
                               Fd.p, (i64d)fplane, Ut.p, (i64d)uplane, KB, ntm, ntn);
        } else {
            const int ntn = cdiv(jb - ja, 64);
            hipLaunchKernelGGL((k_gemm_i8<2, 4, 1, 1, 2, DT>), dim3((unsigned)((i64)ntm * ntn)), dim3(256), 0, s, R, ja, jb, k0, K, F, D.p, (i64d)ldc, seq.p, rows, nrows,
                               Fd.p, (i64d)fplane, Ut.p, (i64d)uplane, KB, ntm, ntn);
        }
    };
    auto trsm = [&](int q, int ja, int jb) {
        if (jb <= ja) return;
        if (ND == 1) hipLaunchKernelGGL((k_trsm_i8<1, DT>), dim3(cdiv(jb - ja, 64)), dim3(64), 0, s, ja, jb, F, D.p, (i64d)ldc, info.p + q, Ut.p, (i64d)uplane, KB, q * DP_W);
        else hipLaunchKernelGGL((k_trsm_i8<2, DT>), dim3(cdiv(jb - ja, 64)), dim3(64), 0, s, ja, jb, F, D.p, (i64d)ldc, info.p + q, Ut.p, (i64d)uplane, KB, q * DP_W);
    };
    int marked_to = 0; // columns whose pivot rows are final once the event of the streamer has passed
    for (int b0 = 0; b0 < C; b0 += KB) {
        const int b1 = std::min(b0 + KB, C);
        HIPCHK(hipMemsetAsync(Fd.p, 0, (size_t)ND * (size_t)fplane, s));
        HIPCHK(hipMemsetAsync(Ut.p, 0, (size_t)ND * (size_t)uplane, s));
        int q = 0;
        for (int c0 = b0; c0 < b1; c0 += DP_W, q++) {
            const int c1 = std::min(c0 + DP_W, b1), w = c1 - c0;
            hipLaunchKernelGGL((k_panel_load<DT>), dim3(Rp / 64), dim3(256), 0, s, R, Rp, c0, w, D.p, (i64d)ldc, P.p, sync.p);
            {
                int a_Rp = Rp, a_chunk = tall ? res_chunk : chunk, a_w = w, a_c0 = c0;
                ZpField a_F = F;
                DT *a_P = P.p;
                int *a_seq = seq.p, *a_pc = pivrow_of_col.p, *a_cand = candrow.p;
                PanelInfo *a_info = info.p + q;
                PanelSync *a_sy = sync.p;
                DenseState *a_st = st.p;
                const int *a_inv = invtab.p;
                unsigned long long *a_stamps = stamps.p;
                void *args[] = {&a_Rp, &a_chunk, &a_w, &a_c0, &a_F, &a_P, &a_seq, &a_pc, &a_info, &a_sy, &a_cand, &a_st, &a_inv, &a_stamps};
                const void *fn_lds = (const void *)k_panel_lu<true, 1024, DT>, *fn_glb = (const void *)k_panel_lu<false, 1024, DT>;
                // A PLAIN launch: G <= one workgroup per CU (checked against the runtime's occupancy figure above), so the grid is
                // resident as a whole once it has started and the kernel's own barrier (dense.hpp: panel_grid_barrier, bounded
                // spins) is enough.  The U streamer's kernels (scan, k_dense_count, k_dense_emit, k_split_ent on its stream s2) do
                // run beside it: they are short, use no LDS to speak of and end on their own, so they can delay the start of a
                // panel workgroup, never hold one out for good; two ELIMINATIONS on one device at once can (each takes a share of
                // the CUs and waits for the rest): ranks that share a device take turns (sharded.py: the replicated finish and dshard_candidates).
                // hipLaunchCooperativeKernel bought nothing but its launch-time size check, cost ~17 us per panel, and its dedicated
                // HSA queue made every rocprofv3-profiled process die in exit(): libamdhip64's exit handler tears that queue down
                // inside libhsa-runtime64 after rocprofiler-sdk has finalised its queue interception (tools/segv_probe.sh,
                // profiles/r03_exit_sigsegv_backtrace.txt -- no frame of this library in the trace).
                // (the follow path gives up for the rest of this elimination once it has misfired four times and more often than
                // not: every misfire costs the resident kernel, the followers' pass and a read-back on top of the in-place panel --
                // residuals of a weak first slab, whose pivots sit anywhere in 2.7M rows: 639 of 648 panels redone)
                const bool follow_now = tall && !(redone >= 4 && 2 * redone > npanels_done);
                if (tall && !follow_now) a_chunk = chunk;
                if (!follow_now) {
                    HIPCHK(hipLaunchKernel(inlds ? fn_lds : fn_glb, dim3(G), dim3(1024), args, (size_t)lds, s));
                } else {
                    // the pivots among the resident rows, then the followers; a follower that should have been a pivot: redo in place
                    HIPCHK(hipMemsetAsync(follow_flag.p, 0, sizeof(int), s));
                    HIPCHK(hipLaunchKernel(fn_lds, dim3(G_res), dim3(1024), args, (size_t)res_chunk * DP_W * (size_t)xbytes, s));
                    hipLaunchKernelGGL((k_panel_follow<1024, DT>), dim3(G_fol), dim3(1024), (size_t)fol_chunk * DP_W * (size_t)xbytes, s, Rp, (int)R_res, fol_chunk, w, F, P.p,
                                       seq.p, info.p + q, follow_flag.p);
                    HIPCHK(hipGetLastError());
                    int fl = 0;
                    HIPCHK(hipMemcpyAsync(&fl, follow_flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
                    HIPCHK(hipStreamSynchronize(s));
                    npanels_done++;
                    if (fl) {
                        redone++;
                        hipLaunchKernelGGL(k_panel_undo, dim3(1), dim3(DP_W), 0, s, c0, info.p + q, seq.p, pivrow_of_col.p, st.p);
                        hipLaunchKernelGGL((k_panel_load<DT>), dim3(Rp / 64), dim3(256), 0, s, R, Rp, c0, w, D.p, (i64d)ldc, P.p, sync.p);
                        HIPCHK(hipGetLastError());
                        a_chunk = chunk;
                        HIPCHK(hipLaunchKernel(fn_glb, dim3(G), dim3(1024), args, 0, s));
                    }
                }
            }
            if (ND == 1) hipLaunchKernelGGL((k_panel_store<1, DT>), dim3(Rp / 64), dim3(256), 0, s, R, Rp, c0, w, F, P.p, seq.p, D.p, (i64d)ldc, info.p + q, Fd.p, (i64d)fplane, KB, q * DP_W);
            else hipLaunchKernelGGL((k_panel_store<2, DT>), dim3(Rp / 64), dim3(256), 0, s, R, Rp, c0, w, F, P.p, seq.p, D.p, (i64d)ldc, info.p + q, Fd.p, (i64d)fplane, KB, q * DP_W);
            // inside the block: the panel's pivot rows, then everybody else, K = 64
            trsm(q, c1, b1);
            gemm(c1, b1, q * DP_W, DP_W, nullptr, 0);
            HIPCHK(hipGetLastError());
        }
        // right of the block: the pivot rows panel by panel (those of earlier panels first applied through the GEMM), then all others
        const int npan = q;
        for (int t = 0; t < npan; t++) {
            if (t > 0) gemm(b1, C, 0, t * DP_W, (const int *)((const char *)(info.p + t) + offsetof(PanelInfo, row)), DP_W);
            trsm(t, b1, C);
        }
        gemm(b1, C, 0, npan * DP_W, nullptr, 0);
        HIPCHK(hipGetLastError());
        if (us) {
            // this block is queued as a whole: the rows of U of the block BEFORE it go to the host now (the host blocks in the copy,
            // the device works through this block meanwhile); then the event that says this block is done
            if (marked_to > us->done_to) us->template take<DT>(marked_to);
            us->mark(s);
            marked_to = b1;
        }
    }
    DenseState hst;
    HIPCHK(hipMemcpyAsync(&hst, st.p, sizeof hst, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hst.pad) throw EngineError("dense finish: a grid barrier of the panel kernel timed out (the device is shared with another process?)");
    dense_stats_note(ND, R, C, KB);
    g_dense_stats[6] += redone;
    if (tall) spasm_logf("[echelonize/dense] tall panels: %lld resident rows elect, %lld follow; %d of %d panels redone in place%s\n", (long long)R_res,
                         (long long)R - (long long)R_res, redone, npanels_done,
                         redone >= 4 && 2 * redone > npanels_done ? ", the others in place from the start" : "");
    if (stamps.p) {
        std::vector<unsigned long long> h(DP_W * 8);
        HIPCHK(hipMemcpy(h.data(), stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        double acc[6] = {0, 0, 0, 0, 0, 0};
        int n = 0;
        for (int c = 0; c + 1 < DP_W; c++) {
            if (!h[(size_t)c * 8 + 5] || !h[(size_t)(c + 1) * 8]) continue;
            for (int k = 0; k < 5; k++) acc[k] += (double)(h[(size_t)c * 8 + k + 1] - h[(size_t)c * 8 + k]);
            acc[5] += (double)(h[(size_t)(c + 1) * 8] - h[(size_t)c * 8 + 5]);
            n++;
        }
        if (n) fprintf(stderr, "[panel stamps] last panel, %d columns, us per column: scan %.2f  record %.2f  barrier %.2f  pivot row %.2f  eliminate %.2f  loop %.2f\n", n,
                       acc[0] / n / 100, acc[1] / n / 100, acc[2] / n / 100, acc[3] / n / 100, acc[4] / n / 100, acc[5] / n / 100);
    }
    return true;
}

// The pivot rows of an eliminated dense matrix (pivrow_of_col[c] = row of D that is the pivot row of its column c, -1: none), as
// sparse rows appended to U: column c of D is column clist[c] of the matrix, row r comes from row row_orig[r] of the input.
// *seconds (if given) receives the time spent.  Returns the number of rows appended.
template <typename DT>
int dense_extract_U(const DT *Dp, int C, i64 ldc, const int *pivrow_of_col, const int *clist, const int *row_orig, HostU &U, hipStream_t s)
{
    Scanner scan;
    DevBuf<int> pflag, pscan;
    pflag.alloc((size_t)C + 1); pscan.alloc((size_t)C + 1);
    hipLaunchKernelGGL(k_flag_nonneg, dim3(cdiv((i64)C + 1, 256)), dim3(256), 0, s, C, pivrow_of_col, pflag.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(pflag.p, pscan.p, (size_t)C + 1, s);
    int npd = 0;
    HIPCHK(hipMemcpyAsync(&npd, pscan.p + C, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (npd == 0) return 0;
    if (U.rank_only) { U.uncollected += npd; return npd; }
    DevBuf<i64d> ulen, uoff;
    ulen.alloc((size_t)npd + 1); uoff.alloc((size_t)npd + 1);
    ulen.zero(s);
    hipLaunchKernelGGL((k_dense_count<DT>), dim3(C), dim3(256), 0, s, C, Dp, (i64d)ldc, pivrow_of_col, pscan.p, ulen.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(ulen.p, uoff.p, (size_t)npd + 1, s);
    i64d tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, uoff.p + npd, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    DevBuf<int2> Ufull;
    DevBuf<int> pivcol, porig;
    Ufull.alloc((size_t)tot + 1); pivcol.alloc((size_t)npd + 1); porig.alloc((size_t)npd + 1);
    hipLaunchKernelGGL((k_dense_emit<DT>), dim3(C), dim3(64), 0, s, C, Dp, (i64d)ldc, pivrow_of_col, pscan.p, uoff.p, clist, row_orig,
                       Ufull.p, pivcol.p, porig.p);
    HIPCHK(hipGetLastError());
    std::vector<i64d> off((size_t)npd + 1);
    std::vector<int> pc((size_t)npd), po((size_t)npd);
    HIPCHK(hipMemcpyAsync(off.data(), uoff.p, ((size_t)npd + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pc.data(), pivcol.p, (size_t)npd * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(po.data(), porig.p, (size_t)npd * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 base = U.p.back();
    for (int k = 0; k < npd; k++) {
        U.p.push_back(base + off[(size_t)k + 1]);
        U.pivcol.push_back(pc[(size_t)k]);
        U.orig.push_back(po[(size_t)k]);
    }
    append_entries(U, Ufull.p, (i64)tot, s);
    return npd;
}

// Leftmost-pivot elimination of a dense R x C matrix D (row-major, leading dimension ldc, residues mod p) whose column c is
// column clist[c] of the matrix and whose row r comes from row row_orig[r] of the input; the pivot rows found are appended to U.
template <typename DT>
int dense_eliminate(DevBuf<DT> &D, int R, int C, i64 ldc, const int *clist, const int *row_orig, const ZpField &F, HostU &U, hipStream_t s)
{
    const double te0 = spasm_wtime();
    double te1 = te0;
    Scanner scan;
    DevBuf<int> is_piv, pivrow_of_col, prow, fcol;
    DevBuf<DenseState> st;
    is_piv.alloc((size_t)R + 1);
    pivrow_of_col.alloc((size_t)C + 1);
    prow.alloc((size_t)ldc);
    fcol.alloc((size_t)R + 1);
    st.alloc(1);
    is_piv.zero(s); st.zero(s);
    const int rc = std::max(R, C);
    UStreamer us;
    bool streamed = false;
    if constexpr (!std::is_same<DT, int>::value) {
        // narrow D: the int8 path (dense_elem_bytes has checked that it applies); pivrow_of_col is filled, D holds the echelon form.
        // The rows of U leave for the host block by block while the elimination goes on (UStreamer).
        us.init(D.p, C, ldc, pivrow_of_col.p, clist, row_orig, U);
        streamed = true;
        if (!dense_eliminate_i8(D, R, C, ldc, F, pivrow_of_col, s, &us)) throw EngineError("dense finish: shape outside the panel kernel's range");
    } else {
        if (F.p <= ((i64)1 << 24)) {
            // blocked: panels of DPB columns, f64-MFMA trailing update (exact: 64 * (p/2)^2 < 2^53)
            const i64 R64 = ((i64)R + 63) / 64 * 64, ldu = ldc;
            DevBuf<double> Lm, Upan;
            DevBuf<int> pan_row, pan_inv;
            Lm.alloc((size_t)R64 * DPB);
            Upan.alloc((size_t)DPB * (size_t)ldu);
            pan_row.alloc(DPB);
            pan_inv.alloc(DPB);
            for (int c0 = 0; c0 < C; c0 += DPB) {
                const int c1 = std::min(c0 + DPB, C);
                Lm.zero(s);
                Upan.zero(s);
                for (int c = c0; c < c1; c++) {
                    hipLaunchKernelGGL(k_panel_find, dim3(1), dim3(1024), 0, s, c, c0, c1, R, F, D.p, (i64d)ldc, is_piv.p, pivrow_of_col.p, prow.p,
                                       pan_row.p, pan_inv.p, st.p);
                    hipLaunchKernelGGL(k_panel_elim2, dim3(R), dim3(64), 0, s, c, c1, F, D.p, (i64d)ldc, is_piv.p, prow.p, fcol.p, Lm.p, st.p);
                }
                HIPCHK(hipGetLastError());
                if (c1 < C) {
                    hipLaunchKernelGGL(k_panel_trsm2, dim3(cdiv(C - c1, 64)), dim3(64), 0, s, c1, C, F, D.p, (i64d)ldc, Lm.p, pan_row.p, pan_inv.p, Upan.p,
                                       (i64d)ldu, st.p);
                    hipLaunchKernelGGL(k_dense_gemm, dim3((unsigned)(R64 / 64), cdiv(C - c1, 64)), dim3(256), 0, s, c1, R, C, F, D.p, (i64d)ldc, Lm.p,
                                       Upan.p, (i64d)ldu, is_piv.p, st.p);
                    HIPCHK(hipGetLastError());
                }
            }
            HIPCHK(hipStreamSynchronize(s)); // Lm / Upan go out of scope
            dense_stats_note(3, R, C, DPB);
        } else {
            dense_stats_note(4, R, C, 1);
            for (int c = 0; c < C; c++) {
                hipLaunchKernelGGL(k_dense_find, dim3(1), dim3(1024), 0, s, c, R, D.p, (i64d)ldc, is_piv.p, pivrow_of_col.p, st.p);
                hipLaunchKernelGGL(k_dense_scale, dim3(cdiv(rc, 256)), dim3(256), 0, s, c, R, C, F, D.p, (i64d)ldc, is_piv.p, prow.p, fcol.p, st.p);
                hipLaunchKernelGGL(k_dense_store_prow, dim3(cdiv(C, 256)), dim3(256), 0, s, c, C, D.p, (i64d)ldc, prow.p, st.p);
                hipLaunchKernelGGL(k_dense_elim, dim3(cdiv(C - c, 256), R), dim3(256), 0, s, c, R, C, F, D.p, (i64d)ldc, prow.p, fcol.p, st.p);
                if ((c & 255) == 255) HIPCHK(hipGetLastError());
            }
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    te1 = spasm_wtime();
    int npd = 0;
    if constexpr (!std::is_same<DT, int>::value) {
        if (streamed) {
            us.template take<DT>(C);
            npd = us.found;
        }
    } else {
        npd = dense_extract_U(D.p, C, ldc, pivrow_of_col.p, clist, row_orig, U, s);
    }
    if (streamed)
        spasm_logf("[echelonize/dense] %d x %d dense tail: %d pivots [elimination with the rows of U leaving block by block %.2fs, the last block's rows %.2fs; %.2fs of copies in all]\n",
                   R, C, npd, te1 - te0, spasm_wtime() - te1, us.seconds);
    else
        spasm_logf("[echelonize/dense] %d x %d dense tail: %d pivots [elimination %.2fs, rows of U to the host %.2fs]\n", R, C, npd, te1 - te0, spasm_wtime() - te1);
    return npd;
}


#include "dense_tall.hpp"

// cells of dense matrix a finish of `rows` x `cols` keeps resident: all of it, or -- tall and skinny -- the first slab and a batch
double dense_cells_resident(const struct echelonize_opts *opts, const ZpField &F, i64 rows, i64 cols)
{
    if (rows <= INT_MAX && cols <= INT_MAX && tall_applies(opts, F, rows, cols)) {
        // (the slab, and the smallest batch of other rows: batches and the dense W adapt to what memory is left)
        const i64 slab = tall_first_slab((int)rows, (int)cols);
        return ((double)slab + (double)std::min<i64>(rows - slab, 4096)) * (double)cols;
    }
    return (double)rows * (double)cols;
}

// cells the finish of `rows` x `cols` may keep resident: the shape cap of dense_max_entries, or -- tall and skinny, where the resident
// part is the slab that carries the pivots and cannot be smaller -- what 55 % of the free memory holds (config 5 at full size:
// a slab of 365k x 324k bytes = 118 GB)
double dense_cells_allowed(const struct echelonize_opts *opts, const ZpField &F, i64 rows, i64 cols, int elem)
{
    if (rows <= INT_MAX && cols <= INT_MAX && tall_applies(opts, F, rows, cols)) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) return 0.55 * (double)fr / (double)std::max(elem, 1);
    }
    return (double)dense_max_entries(elem);
}

// the live rows of a sparse matrix, a range at a time, as dense rows (RowSource of dense_tall.hpp)
template <typename DT> struct FillRowSource {
    const DevMat &M;
    const int *rows, *cmap;
    i64 ldc;
    hipStream_t s;
    void fill(int off, int cnt, DT *Dp)
    {
        if (cnt <= 0) return;
        hipLaunchKernelGGL((k_dense_fill<DT>), dim3(cdiv((i64)cnt * 64, 256)), dim3(256), 0, s, cnt, rows + off, M.start.p, M.len.p, M.ent.p, cmap, Dp, (i64d)ldc);
        HIPCHK(hipGetLastError());
    }
    int nslabs() const { return 1; }
    void slab_range(int, i64 &s0, int &w) const { s0 = 0; w = (int)ldc; }
    void prepare_slab(int) {}
    void fill_slab(int, int off, int cnt, DT *Dp, i64) { fill(off, cnt, Dp); }
    void done() {}
};

int run_dense_tail(const DevMat &M, const ZpField &F, HostU &U, hipStream_t s, const struct echelonize_opts *opts = nullptr)
{
    const int n = M.n, m = M.m;
    Scanner scan;
    // live rows and live columns
    DevBuf<int> rflag, rscan, rows, cflag, cscan, cmap, clist;
    rflag.alloc((size_t)n + 1); rscan.alloc((size_t)n + 1); rows.alloc((size_t)n + 1);
    cflag.alloc((size_t)m + 1); cscan.alloc((size_t)m + 1); cmap.alloc((size_t)m + 1); clist.alloc((size_t)m + 1);
    hipLaunchKernelGGL(k_flag_live, dim3(cdiv((i64)n + 1, 256)), dim3(256), 0, s, n, M.len.p, rflag.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(rflag.p, rscan.p, (size_t)n + 1, s);
    hipLaunchKernelGGL(k_compact, dim3(cdiv(std::max(n, 1), 256)), dim3(256), 0, s, n, rflag.p, rscan.p, rows.p);
    HIPCHK(hipGetLastError());
    cflag.zero(s);
    if (n > 0) {
        hipLaunchKernelGGL(k_flag_cols, dim3(cdiv((i64)n * 64, 256)), dim3(256), 0, s, n, M.start.p, M.len.p, M.ent.p, cflag.p);
        HIPCHK(hipGetLastError());
    }
    scan.exclusive(cflag.p, cscan.p, (size_t)m + 1, s);
    int R = 0, C = 0;
    HIPCHK(hipMemcpyAsync(&R, rscan.p + n, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&C, cscan.p + m, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (R == 0 || C == 0) return 0;
    hipLaunchKernelGGL(k_col_map, dim3(cdiv(m, 256)), dim3(256), 0, s, m, cflag.p, cscan.p, cmap.p, clist.p);
    HIPCHK(hipGetLastError());
    const i64 ldc = ((i64)C + 63) / 64 * 64;
    DevBuf<int> row_orig;
    row_orig.alloc((size_t)R + 1);
    hipLaunchKernelGGL(k_gather_int, dim3(cdiv(R, 256)), dim3(256), 0, s, R, rows.p, M.orig.p, row_orig.p);
    HIPCHK(hipGetLastError());
    auto go = [&](auto tag) {
        using DT = decltype(tag);
        if constexpr (!std::is_same<DT, int>::value) {
            if (tall_applies(opts, F, R, C)) {
                FillRowSource<DT> src{M, rows.p, cmap.p, ldc, s};
                return dense_finish_tall<DT>(src, R, C, ldc, clist.p, row_orig.p, F, U, s);
            }
        }
        DevBuf<DT> D;
        D.alloc((size_t)R * (size_t)ldc);
        D.zero(s);
        hipLaunchKernelGGL((k_dense_fill<DT>), dim3(cdiv((i64)R * 64, 256)), dim3(256), 0, s, R, rows.p, M.start.p, M.len.p, M.ent.p, cmap.p, D.p, (i64d)ldc);
        HIPCHK(hipGetLastError());
        return dense_eliminate(D, R, C, ldc, clist.p, row_orig.p, F, U, s);
    };
    switch (dense_elem_bytes(F, R)) {
    case 1: return go((signed char)0);
    case 2: return go((short)0);
    default: return go((int)0);
    }
}

// ------------------------------------------------------------------------------------------------
// The Schur complement of a round straight into a dense matrix (spasm_schur_dense, prototype reference src/SpaSM.jl:765-766),
// through a dense image of W = -(I + U_PP)^-1 U_PN (kernels.hpp, k_wd_level ..): no multiplier solve, so the cost does not
// depend on how many pivots a row reaches.
// ------------------------------------------------------------------------------------------------
struct DenseW {
    Round &R;
    const DevMat &cur;
    hipStream_t s;
    Scanner scan;
    DevBuf<int> cflag, cscan, cmap, clist, cmap_s, order;
    DevBuf<unsigned char> Wd; // the dense W of the current slab, wbytes per element
    int wbytes = 4;
    std::vector<int> lvl_off; // rows order[lvl_off[l-1] .. lvl_off[l]) make level l >= 1 (level 0 needs no combination)
    int C = 0, depth = 0;
    bool have_levels = false;

    DenseW(Round &R_, const DevMat &cur_, hipStream_t s_) : R(R_), cur(cur_), s(s_) {}

    // columns of the dense matrix: those that hold entries of the current matrix and carry no pivot of this round.  In two halves:
    // row shards OR their flags between flag_columns() and finish_columns(), so that all of them number the columns alike.
    void flag_columns()
    {
        const int m = cur.m;
        cflag.alloc((size_t)m + 1); cscan.alloc((size_t)m + 1); cmap.alloc((size_t)m + 1); clist.alloc((size_t)m + 1); cmap_s.alloc((size_t)m + 1);
        cflag.zero(s);
        if (cur.n > 0) {
            hipLaunchKernelGGL(k_flag_cols, dim3(cdiv((i64)cur.n * 64, 256)), dim3(256), 0, s, cur.n, cur.start.p, cur.len.p, cur.ent.p, cflag.p);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_mask_pivot_cols, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, s, m, R.qinv_r.p, cflag.p);
        HIPCHK(hipGetLastError());
    }
    int finish_columns()
    {
        const int m = cur.m;
        scan.exclusive(cflag.p, cscan.p, (size_t)m + 1, s);
        HIPCHK(hipMemcpyAsync(&C, cscan.p + m, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (C > 0) {
            hipLaunchKernelGGL(k_col_map, dim3(cdiv(m, 256)), dim3(256), 0, s, m, cflag.p, cscan.p, cmap.p, clist.p);
            HIPCHK(hipGetLastError());
        }
        return C;
    }
    int map_columns()
    {
        flag_columns();
        return finish_columns();
    }

    // levels of the pivot graph (pivot indices are a topological order: row q of U_PP only holds indices > q)
    void levels()
    {
        if (have_levels) return;
        have_levels = true;
        const int npiv = R.npiv;
        std::vector<UHdr> hdr((size_t)std::max(npiv, 1));
        std::vector<int2> upp((size_t)std::max<i64>(R.utotal, 1));
        HIPCHK(hipMemcpyAsync(hdr.data(), R.uhdr.p, (size_t)npiv * sizeof(UHdr), hipMemcpyDeviceToHost, s));
        if (R.utotal > 0) HIPCHK(hipMemcpyAsync(upp.data(), R.UPP.p, (size_t)R.utotal * sizeof(int2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::vector<int> lev((size_t)std::max(npiv, 1), 0);
        depth = 0;
        for (int q = npiv - 1; q >= 0; q--) {
            const UHdr &h = hdr[(size_t)q];
            int l = 0;
            for (int k = 0; k < h.npp; k++) l = std::max(l, lev[(size_t)upp[(size_t)h.off + (size_t)k].x] + 1);
            lev[(size_t)q] = l;
            depth = std::max(depth, l);
        }
        lvl_off.assign((size_t)depth + 1, 0);
        for (int q = 0; q < npiv; q++) if (lev[(size_t)q] > 0) lvl_off[(size_t)lev[(size_t)q]]++;
        // lvl_off[l] = end of level l after the prefix sum; level l starts at lvl_off[l - 1]
        for (int l = 1; l <= depth; l++) lvl_off[(size_t)l] += lvl_off[(size_t)l - 1];
        std::vector<int> h_order((size_t)std::max(lvl_off[(size_t)depth], 1)), cursor(lvl_off.begin(), lvl_off.end());
        for (int q = 0; q < npiv; q++) {
            const int l = lev[(size_t)q];
            if (l > 0) h_order[(size_t)cursor[(size_t)l - 1]++] = q;
        }
        order.alloc(h_order.size());
        HIPCHK(hipMemcpyAsync(order.p, h_order.data(), h_order.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }

    static int threads_for(int Cs) { return Cs >= 1024 ? 256 : std::max(16, Cs / 4); }

    // W on the columns cmap_s maps to 0 .. Cs-1 (Cs a multiple of 64)
    void build_w(int Cs)
    {
        levels();
        const int npiv = R.npiv;
        const i64 ldw = Cs;
        Wd.ensure((size_t)std::max(npiv, 1) * (size_t)ldw * (size_t)wbytes);
        HIPCHK(hipMemsetAsync(Wd.p, 0, (size_t)npiv * (size_t)ldw * (size_t)wbytes, s));
        const int bt = threads_for(Cs);
        const unsigned gy = (unsigned)cdiv(Cs, 4 * bt);
        auto go = [&](auto tag) {
            using WT = decltype(tag);
            WT *wd = (WT *)Wd.p;
            constexpr int TEAM = 16;
            hipLaunchKernelGGL((k_wd_seed<TEAM, WT>), dim3(cdiv((i64)npiv * TEAM, 256)), dim3(256), 0, s, npiv, R.F, R.uhdr.p, R.UPN.p, cmap_s.p, wd, (i64d)ldw);
            HIPCHK(hipGetLastError());
            // (narrow residues: 16 bytes per lane and term -- kernels.hpp, WideRow)
            constexpr bool wide = sizeof(WT) < 4;
            const int ept = 16 / (int)sizeof(WT);
            const int btw = Cs / ept >= 256 ? 256 : std::max(16, Cs / ept);
            const unsigned gyw = (unsigned)cdiv(Cs, ept * btw);
            for (int l = 1; l <= depth; l++) {
                const int lo = lvl_off[(size_t)l - 1], cnt = lvl_off[(size_t)l] - lo;
                if (cnt == 0) continue;
                if constexpr (wide) {
                    if (R.F.small) hipLaunchKernelGGL((k_wd_level_wide<WT>), dim3((unsigned)cnt, gyw), dim3(btw), 0, s, cnt, order.p + lo, R.F, R.uhdr.p, R.UPP.p, wd, (i64d)ldw, Cs);
                    else hipLaunchKernelGGL((k_wd_level<false, WT>), dim3((unsigned)cnt, gy), dim3(bt), 0, s, cnt, order.p + lo, R.F, R.uhdr.p, R.UPP.p, wd, (i64d)ldw, Cs);
                } else {
                    if (R.F.small) hipLaunchKernelGGL((k_wd_level<true, WT>), dim3((unsigned)cnt, gy), dim3(bt), 0, s, cnt, order.p + lo, R.F, R.uhdr.p, R.UPP.p, wd, (i64d)ldw, Cs);
                    else hipLaunchKernelGGL((k_wd_level<false, WT>), dim3((unsigned)cnt, gy), dim3(bt), 0, s, cnt, order.p + lo, R.F, R.uhdr.p, R.UPP.p, wd, (i64d)ldw, Cs);
                }
                if ((l & 1023) == 0) HIPCHK(hipGetLastError());
            }
        };
        switch (wbytes) {
        case 1: go((signed char)0); break;
        case 2: go((short)0); break;
        default: go((int)0); break;
        }
        HIPCHK(hipGetLastError());
    }

    // the entries of the rows on pivot columns as (pivot index, value) lists
    DevBuf<i64d> pcnt, poff;
    DevBuf<int2> plist;
    const int *prows = nullptr;
    int pn = -1;
    void row_lists(const int *rows, int nrows)
    {
        if (prows == rows && pn == nrows) return;
        prows = rows; pn = nrows;
        constexpr int TEAM = 16;
        pcnt.alloc((size_t)nrows + 1); poff.alloc((size_t)nrows + 1);
        hipLaunchKernelGGL((k_wd_pcount<TEAM>), dim3(cdiv(((i64)nrows + 1) * TEAM, 256)), dim3(256), 0, s, nrows, rows, cur.start.p, cur.len.p, cur.ent.p,
                           R.qinv_r.p, pcnt.p);
        HIPCHK(hipGetLastError());
        scan.exclusive(pcnt.p, poff.p, (size_t)nrows + 1, s);
        i64d tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, poff.p + nrows, sizeof tot, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        plist.alloc((size_t)tot + 1);
        hipLaunchKernelGGL((k_wd_pfill<TEAM>), dim3(cdiv((i64)nrows * TEAM, 256)), dim3(256), 0, s, nrows, rows, cur.start.p, cur.len.p, cur.ent.p,
                           R.qinv_r.p, poff.p, plist.p);
        HIPCHK(hipGetLastError());
    }

    // the Schur rows of `rows` (local rows, device list) on the slab's columns: Dp[t][dcol0 + j]; Dp is zero there on entry
    template <typename DT> void rows_into(const int *rows, int nrows, int Cs, DT *Dp, i64 ldc, int dcol0)
    {
        if (nrows == 0) return;
        row_lists(rows, nrows);
        constexpr int TEAM = 16;
        hipLaunchKernelGGL((k_wd_own<TEAM, DT>), dim3(cdiv((i64)nrows * TEAM, 256)), dim3(256), 0, s, nrows, rows, cur.start.p, cur.len.p, cur.ent.p, R.qinv_r.p,
                           cmap_s.p, Dp, (i64d)ldc, dcol0);
        const int bt = threads_for(Cs);
        const unsigned gy = (unsigned)cdiv(Cs, 4 * bt);
        auto go = [&](auto tag) {
            using WT = decltype(tag);
            const WT *wd = (const WT *)Wd.p;
            if constexpr (sizeof(WT) < 4 && std::is_same<WT, DT>::value) {
                if (R.F.small) { // narrow residues: 16 bytes per lane and term
                    const int ept = 16 / (int)sizeof(WT);
                    const int btw = Cs / ept >= 256 ? 256 : std::max(16, Cs / ept);
                    hipLaunchKernelGGL((k_wd_rows_wide<WT>), dim3((unsigned)nrows, (unsigned)cdiv(Cs, ept * btw)), dim3(btw), 0, s, nrows, R.F, poff.p, plist.p, wd, (i64d)Cs, Cs, Dp,
                                       (i64d)ldc, dcol0);
                    return;
                }
            }
            if (R.F.small) hipLaunchKernelGGL((k_wd_rows<true, DT, WT>), dim3((unsigned)nrows, gy), dim3(bt), 0, s, nrows, R.F, poff.p, plist.p, wd, (i64d)Cs, Cs, Dp,
                                              (i64d)ldc, dcol0);
            else hipLaunchKernelGGL((k_wd_rows<false, DT, WT>), dim3((unsigned)nrows, gy), dim3(bt), 0, s, nrows, R.F, poff.p, plist.p, wd, (i64d)Cs, Cs, Dp, (i64d)ldc,
                                    dcol0);
        };
        switch (wbytes) {
        case 1: go((signed char)0); break;
        case 2: go((short)0); break;
        default: go((int)0); break;
        }
        HIPCHK(hipGetLastError());
    }

    void slab(int s0, int Cs, int stride)
    {
        hipLaunchKernelGGL(k_slab_cmap, dim3(cdiv(cur.m, 256)), dim3(256), 0, s, cur.m, cmap.p, s0, Cs, stride, cmap_s.p);
        HIPCHK(hipGetLastError());
    }

    // spasm_schur_estimate_density (prototype reference src/SpaSM.jl:763-764) without solving a single row: the Schur complement
    // restricted to 64 of its columns, evenly spread, for ALL the non-pivot rows; density relative to `free_cols` columns
    double estimate_density(const int *rows, int nrows, int free_cols)
    {
        if (C == 0 || nrows == 0 || free_cols <= 0) return 0.0;
        const int Cs = 64, stride = std::max(1, C / Cs);
        const int sampled = std::min(Cs, (C + stride - 1) / stride);
        slab(0, Cs, stride > 1 ? stride : 0); // (stride 1: the first 64 columns, as a slab)
        build_w(Cs);
        DevBuf<int> Dsm;
        DevBuf<u64d> cnt;
        Dsm.alloc((size_t)nrows * Cs);
        Dsm.zero(s);
        cnt.alloc(1);
        cnt.zero(s);
        rows_into(rows, nrows, Cs, Dsm.p, Cs, 0);
        hipLaunchKernelGGL(k_count_nonzero, dim3(std::min(cdiv((i64)nrows * Cs, 256), R.num_cu * 16)), dim3(256), 0, s, (i64d)nrows * Cs, Dsm.p, cnt.p);
        HIPCHK(hipGetLastError());
        u64d nz = 0;
        HIPCHK(hipMemcpyAsync(&nz, cnt.p, sizeof nz, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // nz / (rows * sampled) is the density over the C live columns; the other free columns are empty
        return (double)nz / ((double)nrows * (double)sampled) * ((double)C / (double)free_cols);
    }
};

// The Schur complement of the round R has prepared (pivots elected, U built), straight into a dense matrix over the columns W has
// mapped: D gets nnp + extra_rows rows (the extra ones zero: the guest rows of the distributed finish), row_orig the input rows.
template <typename DT>
void schur_dense_build(Round &R, const DevMat &cur, int nnp, DenseW &W, int extra_rows, DevBuf<DT> &D, DevBuf<int> &row_orig, hipStream_t s)
{
    const int C = W.C;
    const double tw0 = spasm_wtime();
    const i64 ldc = ((i64)C + 63) / 64 * 64;
    D.alloc(((size_t)nnp + (size_t)extra_rows) * (size_t)ldc);
    D.zero(s);
    row_orig.alloc((size_t)nnp + 1);
    if (nnp > 0) {
        hipLaunchKernelGGL(k_gather_int, dim3(cdiv(nnp, 256)), dim3(256), 0, s, nnp, R.np_rows.p, cur.orig.p, row_orig.p);
        HIPCHK(hipGetLastError());
    }
    // W for as many columns at a time as a third of the free memory holds
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    W.wbytes = (int)sizeof(DT); // (W holds residues like D does)
    i64 budget = (i64)(fr / 3) + (i64)W.Wd.n;
    if (const char *mb = getenv("SPASM_AMD_MEM_BUDGET_MB")) budget = std::max<i64>(atoll(mb), 1) << 18; // tests: several slabs
    i64 Cs = std::min<i64>(ldc, std::max<i64>(64, budget / ((i64)std::max(R.npiv, 1) * W.wbytes) / 64 * 64));
    int nslab = 0;
    for (i64 s0 = 0; s0 < ldc && nnp > 0; s0 += Cs, nslab++) {
        const int w = (int)std::min<i64>(Cs, ldc - s0);
        W.slab((int)s0, w, 0);
        W.build_w(w);
        W.rows_into(R.np_rows.p, nnp, w, D.p, ldc, (int)s0);
    }
    HIPCHK(hipStreamSynchronize(s));
    spasm_logf("[echelonize/dense] Schur complement %d x %d through a dense W (%d pivots, %d levels, %d slab%s of columns) [%.2fs]\n", nnp, C, R.npiv,
               W.depth, nslab, nslab == 1 ? "" : "s", spasm_wtime() - tw0);
    W.Wd.release();
}

// the Schur rows of a round, a range of the non-pivot rows at a time, through the dense W (RowSource of dense_tall.hpp)
template <typename DT> struct SchurRowSource {
    Round &R;
    const DevMat &cur;
    DenseW &W;
    i64 ldc;
    hipStream_t s;
    i64 Cs = 0;
    bool built = false;
    SchurRowSource(Round &R_, const DevMat &cur_, DenseW &W_, i64 ldc_, hipStream_t s_) : R(R_), cur(cur_), W(W_), ldc(ldc_), s(s_)
    {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        W.wbytes = (int)sizeof(DT);
        i64 budget = (i64)(fr / 3) + (i64)W.Wd.n;
        if (const char *mb = getenv("SPASM_AMD_MEM_BUDGET_MB")) budget = std::max<i64>(atoll(mb), 1) << 18;
        Cs = std::min<i64>(ldc, std::max<i64>(64, budget / ((i64)std::max(R.npiv, 1) * W.wbytes) / 64 * 64));
    }
    void fill(int off, int cnt, DT *Dp)
    {
        const bool one = Cs >= ldc; // W for all columns at once: built once, kept until done()
        for (i64 s0 = 0; s0 < ldc && cnt > 0; s0 += Cs) {
            const int w = (int)std::min<i64>(Cs, ldc - s0);
            if (!(one && built)) {
                W.slab((int)s0, w, 0);
                W.build_w(w);
                built = true;
            }
            W.rows_into(R.np_rows.p + off, cnt, w, Dp, ldc, (int)s0);
        }
    }
    int nslabs() const { return (int)((ldc + Cs - 1) / Cs); }
    void slab_range(int k, i64 &s0, int &w) const { s0 = (i64)k * Cs; w = (int)std::min<i64>(Cs, ldc - s0); }
    void prepare_slab(int k)
    {
        if (Cs >= ldc && built) return;
        i64 s0;
        int w;
        slab_range(k, s0, w);
        W.slab((int)s0, w, 0);
        W.build_w(w);
        built = true;
    }
    // rows off .. off + cnt on the columns of the slab prepare_slab(k) has built: Dp[i][j], j < w, leading dimension ldw
    void fill_slab(int k, int off, int cnt, DT *Dp, i64 ldw)
    {
        i64 s0;
        int w;
        slab_range(k, s0, w);
        if (cnt > 0) W.rows_into(R.np_rows.p + off, cnt, w, Dp, ldw, 0);
    }
    void done() { W.Wd.release(); built = false; }
};

// The finish of an echelonization whose remainder is dense: the Schur complement of the round R has prepared (pivots elected, U
// built) goes straight into a dense matrix over the columns that are left, and is eliminated there.
void schur_dense_finish(Round &R, const DevMat &cur, int nnp, HostU &U, hipStream_t s, DenseW *prepared = nullptr, const struct echelonize_opts *opts = nullptr)
{
    std::unique_ptr<DenseW> own;
    if (!prepared) {
        own.reset(new DenseW(R, cur, s));
        own->map_columns();
        prepared = own.get();
    }
    DenseW &W = *prepared;
    const int C = W.C;
    if (C == 0 || nnp == 0) return;
    const i64 ldc = ((i64)C + 63) / 64 * 64;
    DevBuf<int> row_orig;
    // (element type of D: dense_elem_bytes)
    auto go = [&](auto tag) {
        using DT = decltype(tag);
        if constexpr (!std::is_same<DT, int>::value) {
            if (tall_applies(opts, R.F, nnp, C)) {
                // many more rows than columns: one slab carries the pivots, the other rows are reduced in one step (dense_tall.hpp)
                row_orig.alloc((size_t)nnp + 1);
                hipLaunchKernelGGL(k_gather_int, dim3(cdiv(nnp, 256)), dim3(256), 0, s, nnp, R.np_rows.p, cur.orig.p, row_orig.p);
                HIPCHK(hipGetLastError());
                SchurRowSource<DT> src(R, cur, W, ldc, s);
                dense_finish_tall<DT>(src, nnp, C, ldc, W.clist.p, row_orig.p, R.F, U, s);
                return;
            }
        }
        DevBuf<DT> D;
        schur_dense_build(R, cur, nnp, W, 0, D, row_orig, s);
        dense_eliminate(D, nnp, C, ldc, W.clist.p, row_orig.p, R.F, U, s);
    };
    switch (dense_elem_bytes(R.F, nnp)) {
    case 1: go((signed char)0); break;
    case 2: go((short)0); break;
    default: go((int)0); break;
    }
}

#include "dense_multi.hpp"

// the L factor on the host, as it is collected: per chunk the rows it belongs to (original row of A per slot, entries per slot),
// then the (row of U, value) pairs
struct HostL {
    std::vector<int> row;     // original row of every entry
    std::vector<int> j, x;    // row of U, value
};

// the multiplier lists of the `cnt` row slots the last solve_phase of R filled (rows np_rows[off ..]) -> HostL; ubase = rows of U
// that existed before this round
void collect_L_lists(HostL &L, Round &R, const DevMat &cur, int off, int cnt, int ubase, hipStream_t s)
{
    if (cnt == 0) return;
    DevBuf<i64d> lcnt, loff;
    lcnt.alloc((size_t)cnt + 1); loff.alloc((size_t)cnt + 1);
    hipLaunchKernelGGL(k_l_count, dim3(cdiv(((i64)cnt + 1) * 64, 256)), dim3(256), 0, s, cnt, R.Lstart.p, R.Llen.p, R.Lpool.p, lcnt.p);
    HIPCHK(hipGetLastError());
    R.scan.exclusive(lcnt.p, loff.p, (size_t)cnt + 1, s);
    std::vector<i64d> h_off((size_t)cnt + 1);
    std::vector<int> h_rows((size_t)cnt), h_orig((size_t)cur.n);
    HIPCHK(hipMemcpyAsync(h_off.data(), loff.p, ((size_t)cnt + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_rows.data(), R.np_rows.p + off, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_orig.data(), cur.orig.p, (size_t)cur.n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 tot = h_off[(size_t)cnt];
    if (tot == 0) return;
    DevBuf<int> oj, ox;
    oj.alloc((size_t)tot); ox.alloc((size_t)tot);
    hipLaunchKernelGGL(k_l_fill, dim3(cdiv((i64)cnt * 64, 256)), dim3(256), 0, s, cnt, ubase, R.Lstart.p, R.Llen.p, R.Lpool.p, R.Lidx.p, loff.p, oj.p, ox.p);
    HIPCHK(hipGetLastError());
    const size_t old = L.j.size();
    L.j.resize(old + (size_t)tot); L.x.resize(old + (size_t)tot); L.row.resize(old + (size_t)tot);
    HIPCHK(hipMemcpyAsync(L.j.data() + old, oj.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(L.x.data() + old, ox.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int t = 0; t < cnt; t++) {
        const int o = h_orig[(size_t)h_rows[(size_t)t]];
        for (i64 k = h_off[(size_t)t]; k < h_off[(size_t)t + 1]; k++) L.row[old + (size_t)k] = o;
    }
}

// the diagonal: row U.orig[ubase + k] of A is pivval[k] times row ubase + k of U (plus what its own list said in earlier rounds)
void collect_L_pivots(HostL &L, Round &R, const HostU &U, int ubase, hipStream_t s)
{
    const int np = R.npiv;
    if (np == 0) return;
    std::vector<int> pv((size_t)np);
    HIPCHK(hipMemcpyAsync(pv.data(), R.pivval.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < np; k++) {
        L.row.push_back(U.orig[(size_t)ubase + (size_t)k]);
        L.j.push_back(ubase + k);
        L.x.push_back(pv[(size_t)k]);
    }
}

struct HostL;
struct spasm_lu *assemble_lu(HostU &U, int n, int m, i64 prime, HostL *HLp);

struct spasm_lu *do_echelonize(const struct spasm_csr *A, struct echelonize_opts *opts, i64 *rank_only = nullptr)
{
    // max_round, min_pivot_proportion, enable_dense and sparsity_threshold (reference src/SpaSM.jl:329-337) decide how far the
    // sparse rounds go and what finishes.  With enable_greedy_pivot_search off every pivot is a leftmost entry, and rank, pivot
    // columns and kernel do not depend on those tunables; with it on (the reference's default) the pivot columns depend on
    // where the sparse rounds stop, the rank of course does not.
    struct echelonize_opts dflt;
    if (!opts) { spasm_echelonize_init_opts(&dflt); opts = &dflt; }
    require_device();
    check_input(A, "spasm_echelonize");
    const int n = A->n, m = A->m;
    const i64 prime = A->field->p;
    const double t0 = spasm_wtime();
    spasm_logf("[echelonize] Start on %d x %d matrix with %lld nnz\n", n, m, (long long)spasm_nnz(A));
    g_last_rounds.clear();
    memset(g_dense_stats, 0, sizeof g_dense_stats);
    // Fields of echelonize_opts (reference src/SpaSM.jl:332, :339, :340, :342) this engine has no use for say so when they are set
    // away from spasm_echelonize_init_opts' values: they tune libspasm's dense strategies (rows per dense block of its FFPACK
    // calls; when its randomized low-rank mode starts and with which row weights) and the completion of L -- the dense finish
    // here is one exact blocked elimination (panels of 64 columns, blocks of 1024), which has no such knobs, and L holds the
    // multipliers of the pivotal and the eliminated rows as the rounds produced them.  The result does not depend on them.
    {
        struct echelonize_opts d0;
        spasm_echelonize_init_opts(&d0);
        if (opts->dense_block_size != d0.dense_block_size)
            spasm_logf("[echelonize] option dense_block_size = %d ignored (the dense finish works in panels of 64 columns and blocks of 1024)\n", opts->dense_block_size);
        if (opts->low_rank_ratio != d0.low_rank_ratio || opts->low_rank_start_weight != d0.low_rank_start_weight)
            spasm_logf("[echelonize] options low_rank_ratio = %g / low_rank_start_weight = %g ignored (no randomized low-rank mode: the "
                       "tall-and-skinny finish reduces every row exactly)\n", opts->low_rank_ratio, opts->low_rank_start_weight);
        if (opts->complete != d0.complete) spasm_logf("[echelonize] option complete = %d ignored (L is returned as the rounds produced it; LU.complete stays false)\n", (int)opts->complete);
    }

    hipStream_t stream = nullptr;
    HostU U;
    U.p.push_back(0);
    U.rank_only = rank_only != nullptr;
    std::unique_ptr<DevMat> cur(new DevMat());
    upload_csr(A, 0, n, *cur, stream);
    i64 cur_nnz = spasm_nnz(A);

    std::unique_ptr<Round> R(new Round());
    R->F = zp_field_make(prime);
    R->stream = stream;
    // the trip counters of the round statistics (applications, nnz_reduced, read_bytes) count multiplier-list entries: they are
    // exact only when the rounds keep to the lists, which costs about a third more time per round
    if (const char *e = getenv("SPASM_AMD_ROUND_STATS")) R->force_lists = atoi(e) != 0;
    // (no event pair around every scatter class: with them the classes run one after the other on one stream -- the two lanes and
    // the twins' side streams are what the benchmark's step has, and a round is to cost what that step costs.  The per-class times
    // of the round statistics are then zero; SPASM_AMD_CLASS_TIMING=1 brings them back.)
    R->class_timing = false;
    if (const char *e = getenv("SPASM_AMD_CLASS_TIMING")) R->class_timing = atoi(e) != 0;
    // echelonize_opts.L (reference src/SpaSM.jl:331): keep the multipliers.  They only exist as lists on the sparse path, so the
    // rounds keep to the lists (with the pivot index of every record) and the dense finish is not used.
    const bool want_L = opts->L;
    const bool use_dense = opts->enable_dense && !want_L;
    HostL HL;
    if (want_L) { R->force_lists = true; R->want_idx = true; R->want_pivval = true; }
    int round = 0;
    i64 cur_live = n;
    bool gplu_finish = false; // the sparse rounds are over (max_round / min_pivot_proportion) and the dense finish is not an option
    bool partial = false;     // enable_GPLU = 0 and no dense finish: the factorization stops short (the reference's behaviour)
    while (cur->n > 0 && m > 0) {
        {
            const i64 cfree = (i64)m - (i64)U.pivcol.size();
            const double cells = (double)cur_live * (double)cfree;
            if (use_dense && cur_nnz > 0 && cells > 0 && dense_cells_resident(opts, R->F, cur_live, cfree) <= dense_cells_allowed(opts, R->F, cur_live, cfree, dense_elem_bytes(R->F, cur_live)) &&
                (double)cur_nnz > opts->sparsity_threshold * cells) {
                spasm_logf("[echelonize] finishing; density = %.3f; aspect ratio = %.1f\n", (double)cur_nnz / cells,
                           cfree > 0 ? (double)cur_live / (double)cfree : 0.0);
                run_dense_tail(*cur, R->F, U, stream, opts);
                break;
            }
        }
        HIPCHK(hipEventRecord(R->ev[0], stream));
        R->elect_local(*cur, 0);
        R->assign_pivots();
        if (R->npiv == 0) break; // no non-empty row left
        // enable_greedy_pivot_search (reference src/SpaSM.jl:326): off = leftmost-entry pivots only; on = also "FL on columns"
        // in the max_round sparse rounds (libspasm's third search, the cycle-free greedy one, is not reproduced).  The rounds of the
        // finish keep to leftmost entries, like the reference's GPLU and dense finishes.
        R->n_leftmost = R->npiv;
        R->n_open = 0;
        R->n_greedy = 0;
        if (opts->enable_greedy_pivot_search && !gplu_finish && round < opts->max_round) {
            R->extend_pivots_on_open_columns(*cur);
            const char *no_third = getenv("SPASM_AMD_NO_CYCLE_FREE_SEARCH"); // A/B: the round without the third search
            if (!(no_third && atoi(no_third))) R->extend_pivots_cycle_free(*cur);
        }
        if (!gplu_finish) {
            // The reference's round loop (tunables src/SpaSM.jl:333-337): at most max_round sparse rounds, and none that finds
            // fewer than min_pivot_proportion * min(rows, free columns) pivots ("not enough pivots found; stopping", README.md:32).
            // What is left then goes to the dense finish when it fits the device and may be used, else to the GPLU-style
            // finish: more leftmost-pivot rounds until nothing is left.
            const i64 cfree = (i64)m - (i64)U.pivcol.size();
            const double need = opts->min_pivot_proportion * (double)std::min<i64>(cur_live, cfree);
            const bool few = (double)R->npiv < need;
            const bool spent = round >= opts->max_round;
            if (few || spent) {
                if (few) spasm_logf("[echelonize] not enough pivots found; stopping (%d < %.0f)\n", R->npiv, need);
                const double cells = (double)cur_live * (double)cfree;
                // dense when the remainder is dense enough (the reference's rule) or small enough for the cubic work not to matter
                // (2^28 cells: a 16384 x 16384 remainder); a large sparse remainder is better served by more sparse rounds
                const bool worth = (double)cur_nnz > opts->sparsity_threshold * cells || cells <= (double)((i64)1 << 28);
                if (use_dense && cells > 0 && dense_cells_resident(opts, R->F, cur_live, cfree) <= dense_cells_allowed(opts, R->F, cur_live, cfree, dense_elem_bytes(R->F, cur_live)) && worth) {
                    spasm_logf("[echelonize] finishing; density = %.3f; aspect ratio = %.1f\n", (double)cur_nnz / cells,
                               cfree > 0 ? (double)cur_live / (double)cfree : 0.0);
                    run_dense_tail(*cur, R->F, U, stream, opts);
                    break;
                }
                if (!opts->enable_GPLU) {
                    // enable_GPLU = 0 (reference src/SpaSM.jl:330) with the dense finish off, not applicable or vetoed: no method is left
                    // to finish with.  libspasm says so and returns what the sparse rounds found ([UPSTREAM-RECALL] "Cannot finish
                    // (no valid method; enable either GPLU or dense)"): U is then a partial echelon form and r a LOWER bound of the rank.
                    spasm_logf("[echelonize] Cannot finish (no valid method; enable either GPLU or dense): stopping with %d pivots, a lower bound of the rank\n",
                               (int)U.pivcol.size());
                    partial = true;
                    break;
                }
                spasm_logf("[echelonize] finishing with GPLU-style rounds\n");
                gplu_finish = true;
            }
        }
        R->mark_local(*cur, 0);
        R->build_U(*cur, R->pivrow.p);
        // W (level by level, no Uinv) when many more rows than pivots are reduced and the pivot graph is shallow; otherwise Uinv
        // for the multiplier lists, or elimination chains when that is too dense as well
        R->prepare_w(R->nnp, cur_nnz);
        if (R->use_w) { R->use_uinv = false; R->ms_uinv = 0; }
        else R->prepare_uinv(R->nnp);
        const int nnp = R->nnp;
        // The multiplier records and the slots of the Schur rows of ALL non-pivot rows normally fit (config 3: 0.5 + 4.6 GB).
        // Rounds whose rows reach tens of thousands of pivots (Macaulay-like) can need more than the device has: the rows
        // are then reduced in batches, each appended compactly to the matrix of the next round.
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        i64 avail = (i64)mem_free + (i64)(R->Lpool.n * sizeof(int4)) + (i64)(R->S.ent.n * sizeof(int2));
        i64 floor_entries = 1 << 20;
        if (const char *mb = getenv("SPASM_AMD_MEM_BUDGET_MB")) { // tests: pretend the device is this small
            avail = std::max<i64>(atoll(mb), 1) << 20;
            floor_entries = 1 << 10;
        }
        const i64 max_pool = std::max<i64>((i64)(0.40 * (double)avail) / (i64)sizeof(int4), floor_entries);
        const i64 max_slots = std::max<i64>((i64)(0.30 * (double)avail) / (i64)sizeof(int2), floor_entries);
        std::unique_ptr<DevMat> next(new DevMat());
        next->n = nnp;
        next->m = m;
        RoundCounters acc;
        memset(&acc, 0, sizeof acc);
        int acc_class[NCLASS] = {0};
        float ms_solve = 0, ms_scatter = 0;
        i64 appended = 0; // entries of next->ent in use (batched rounds)
        int off = 0, chunk = nnp, nbatch = 0;
        float ms_pivots = 0;
        DevBuf<i64d> app_scan;
        // ---- the density of the Schur complement, estimated before it is built (reference spasm_schur_estimate_density, prototype
        // src/SpaSM.jl:763-764, log line README.md:25): the Schur rows of a sample of the non-pivot rows (every step-th, at most
        // 2048; libspasm takes 100 at random) are computed for real.  The same sample sizes the record pool and the slots.
        double rec_per_row = 4.0 * (double)cur_nnz / (double)std::max(nnp, 1), slots_per_row = 0;
        double est_density = -1;
        const int free_now = m - (int)U.pivcol.size() - R->npiv;
        const bool dense_possible = use_dense && nnp > 64 && dense_cells_resident(opts, R->F, nnp, free_now) <= dense_cells_allowed(opts, R->F, nnp, free_now, dense_elem_bytes(R->F, nnp));
        std::unique_ptr<DenseW> dw;
        if (nnp > 0 && dense_possible && !R->use_uinv && !R->use_w) {
            // No Uinv: the rows of this round reach many pivots (or there are few rows), and the row sample below would walk those
            // reaches one dependent step at a time (1.7 s for 2048 rows of the 200k x 80k Macaulay-like case).  Sample COLUMNS
            // instead: the Schur complement on 64 of its columns, all rows, through a dense W.
            dw.reset(new DenseW(*R, *cur, stream));
            dw->map_columns();
            est_density = dw->estimate_density(R->np_rows.p, nnp, free_now);
            spasm_logf("Schur complement is %d x %d, estimated density : %.2f (64 columns sampled, %d levels)\n", nnp, free_now, est_density, dw->depth);
        }
        const bool go_dense = dense_possible && est_density > opts->sparsity_threshold;
        if (nnp > 0 && !go_dense) {
            const int probe = std::min(nnp, 2048);
            const int step = nnp / probe;
            DevBuf<int> probe_rows;
            probe_rows.alloc((size_t)probe + 1);
            hipLaunchKernelGGL(k_pick_stride, dim3(cdiv(probe, 256)), dim3(256), 0, stream, probe, step, R->np_rows.p, probe_rows.p);
            HIPCHK(hipGetLastError());
            const i64 tp = R->solve_phase(*cur, probe_rows.p, nullptr, probe, 1 << 20, max_pool);
            if (tp >= 0) {
                rec_per_row = std::max(rec_per_row, 1.25 * (double)R->pool_used() / probe);
                slots_per_row = 1.25 * (double)tp / probe;
            }
            // (the sample's Schur rows are only computed where the answer can matter: the dense finish allowed and within reach)
            if (tp >= 0 && tp <= max_slots && dense_possible && est_density < 0) {
                R->S.ent.ensure((size_t)tp + 1);
                R->run_scatter(*cur, probe_rows.p, probe);
                R->fetch_counters();
                if (free_now > 0) est_density = (double)R->hctr.nnz_out / ((double)probe * (double)free_now);
                spasm_logf("Schur complement is %d x %d, estimated density : %.2f (%d rows sampled)\n", nnp, free_now, est_density, probe);
            } else if (tp < 0) {
                rec_per_row = (double)max_pool / probe;
            }
            if (nnp > 16384) {
                const double fit = std::min((double)max_pool / std::max(rec_per_row, 1.0), slots_per_row > 0 ? (double)max_slots / slots_per_row : 1e18);
                if (fit < (double)nnp) chunk = std::max(1, (int)(0.8 * fit));
            }
        }
        // ---- dense already?  Then the Schur complement goes straight into the dense matrix of the finish (spasm_schur_dense,
        // prototype src/SpaSM.jl:765-766) and is never materialised sparse.
        if (dense_possible && est_density > opts->sparsity_threshold) {
            spasm_logf("[echelonize] round %d\n[pivots] Faugère-Lachartre: %d pivots found\n", round, R->n_leftmost);
            if (R->n_open) spasm_logf("[pivots] ``Faugère-Lachartre on columns'': %d pivots found\n", R->n_open);
            if (R->n_greedy) spasm_logf("[pivots] greedy alternating cycle-free search: %d pivots found\n", R->n_greedy);
            spasm_logf("[echelonize] finishing; density = %.3f (estimated); aspect ratio = %.1f; Schur complement straight to dense\n", est_density,
                       free_now > 0 ? (double)nnp / (double)free_now : 0.0);
            append_round_U(U, *R, *cur, stream);
            schur_dense_finish(*R, *cur, nnp, U, stream, dw.get(), opts);
            spasm_amd_round_stats st;
            fill_stats(st, *R, round, cur->n, cur_nnz);
            st.nnz_out = -1; // (never counted: the rows went dense)
            g_last_rounds.push_back(st);
            break;
        }
        dw.reset();
        while (off < nnp || nnp == 0) {
            const int cnt = std::min(chunk, nnp - off);
            // (what the step allocates is allocated here, in front of the timed step: the record pool, the per-row arrays, and S as the
            // sample sized it -- a 4 GB hipMalloc between two kernels of the step is milliseconds of an idle device)
            R->alloc_solve(cnt, std::min<i64>(std::max<i64>((i64)(rec_per_row * (double)cnt), 1 << 16), max_pool));
            R->warm_scatter();
            if (slots_per_row > 0) R->S.ent.ensure((size_t)std::min<double>((double)max_slots, 1.05 * slots_per_row * (double)cnt) + 1024);
            HIPCHK(hipEventRecord(R->ev[1], stream));
            // the solve (plan or multiplier lists, bounds), then the scatter classes
            const i64 tot = R->solve_phase(*cur, R->np_rows.p + off, nullptr, cnt, std::max<i64>((i64)(rec_per_row * (double)cnt), 1 << 16), max_pool);
            if (tot < 0 || tot > max_slots) {
                if (cnt <= 1) throw EngineError("one row of the Schur complement does not fit the device memory");
                chunk = std::max(1, cnt / 2);
                spasm_logf("[echelonize] round %d: %d rows at a time do not fit the device memory, trying %d\n", round, cnt, chunk);
                continue;
            }
            HIPCHK(hipEventRecord(R->ev[2], stream));
            R->S.ent.ensure((size_t)tot + 1);
            R->run_scatter(*cur, R->np_rows.p + off, cnt);
            HIPCHK(hipEventRecord(R->ev[3], stream));
            R->fetch_counters();
            if (want_L) collect_L_lists(HL, *R, *cur, off, cnt, (int)U.pivcol.size(), stream);
            {
                float ms = 0;
                if (nbatch == 0 && hipEventElapsedTime(&ms, R->ev[0], R->ev[1]) == hipSuccess) ms_pivots = ms; // incl. the probe
                if (hipEventElapsedTime(&ms, R->ev[1], R->ev[2]) == hipSuccess) ms_solve += ms;
                if (hipEventElapsedTime(&ms, R->ev[2], R->ev[3]) == hipSuccess) ms_scatter += ms;
            }
            acc.applications += R->hctr.applications;
            acc.nnz_reduced += R->hctr.nnz_reduced;
            acc.segments += R->hctr.segments;
            acc.nonempty_out += R->hctr.nonempty_out;
            acc.nnz_out += R->hctr.nnz_out;
            acc.stream_fix += R->hctr.stream_fix;
            acc.stream_redo += R->hctr.stream_redo;
            for (int c = 0; c < 16; c++) { acc.class_ent[c] += R->hctr.class_ent[c]; acc.class_seg[c] += R->hctr.class_seg[c]; }
            for (int c = 0; c < NCLASS; c++) acc_class[c] += R->hclass_count[c];
            nbatch++;
            if (off == 0 && cnt == nnp) {
                // the whole round at once: its slots become the next matrix as they are
                next->start = std::move(R->S.start);
                next->len = std::move(R->S.len);
                next->lead = std::move(R->S.lead);
                next->orig = std::move(R->S.orig);
                next->ent = std::move(R->S.ent);
            } else {
                if (off == 0) {
                    next->start.ensure((size_t)nnp + 1);
                    next->len.ensure((size_t)nnp + 1);
                    next->lead.ensure((size_t)nnp + 1);
                    next->orig.ensure((size_t)nnp + 1);
                }
                const i64 add = (i64)R->hctr.nnz_out;
                if ((size_t)(appended + add + 1) > next->ent.n) { // grow geometrically, keep what is there
                    DevBuf<int2> bigger;
                    bigger.alloc((size_t)std::max<i64>(appended + add + 1, (i64)((double)next->ent.n * 1.5)));
                    if (appended > 0) HIPCHK(hipMemcpyAsync(bigger.p, next->ent.p, (size_t)appended * sizeof(int2), hipMemcpyDeviceToDevice, stream));
                    HIPCHK(hipStreamSynchronize(stream));
                    next->ent = std::move(bigger);
                }
                app_scan.ensure((size_t)cnt + 2);
                hipLaunchKernelGGL(k_copy_len64, dim3(cdiv((i64)cnt + 1, 256)), dim3(256), 0, stream, cnt, R->S.len.p, app_scan.p);
                HIPCHK(hipGetLastError());
                R->scan.exclusive(app_scan.p, app_scan.p, (size_t)cnt + 1, stream);
                constexpr int TEAM = 16;
                hipLaunchKernelGGL((k_append_rows<TEAM>), dim3(cdiv((i64)cnt * TEAM, 256)), dim3(256), 0, stream, cnt, R->S.start.p, R->S.len.p,
                                   R->S.lead.p, R->S.orig.p, R->S.ent.p, app_scan.p, (i64d)appended, off, next->ent.p, next->start.p,
                                   next->len.p, next->lead.p, next->orig.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(stream));
                appended += add;
            }
            off += cnt;
            if (nnp == 0) break;
        }
        if (nbatch > 1) {
            // the pools of a batched round are as large as the device allows: give them back before the next round
            R->Lpool.release();
            R->S.ent.release();
        }
        R->hctr.applications = acc.applications;
        R->hctr.nnz_reduced = acc.nnz_reduced;
        R->hctr.segments = acc.segments;
        R->hctr.nonempty_out = acc.nonempty_out;
        R->hctr.nnz_out = acc.nnz_out;
        R->hctr.stream_fix = acc.stream_fix;
        R->hctr.stream_redo = acc.stream_redo;
        for (int c = 0; c < 16; c++) { R->hctr.class_ent[c] = acc.class_ent[c]; R->hctr.class_seg[c] = acc.class_seg[c]; }
        for (int c = 0; c < NCLASS; c++) R->hclass_count[c] = acc_class[c];
        {
            const int ubase = (int)U.pivcol.size();
            append_round_U(U, *R, *cur, stream);
            if (want_L) collect_L_pivots(HL, *R, U, ubase, stream);
        }

        spasm_amd_round_stats st;
        fill_stats(st, *R, round, cur->n, cur_nnz);
        st.ms_pivots = ms_pivots;
        st.ms_solve = ms_solve;
        st.ms_scatter = ms_scatter;
        st.ms_total = ms_pivots + ms_solve + ms_scatter;
        g_last_rounds.push_back(st);
        spasm_logf("[echelonize] round %d\n[pivots] Faugère-Lachartre: %d pivots found [%.1fs]\n", round, R->n_leftmost, st.ms_pivots * 1e-3);
        if (R->n_open) spasm_logf("[pivots] ``Faugère-Lachartre on columns'': %d pivots found\n", R->n_open);
        if (R->n_greedy) spasm_logf("[pivots] greedy alternating cycle-free search: %d pivots found\n", R->n_greedy);
        spasm_logf("Schur complement: %d * %d [%lld nz / density= %.3f], %.1fs%s\n", nnp, m - (int)U.pivcol.size(),
                   (long long)st.nnz_out, nnp > 0 && m > 0 ? (double)st.nnz_out / ((double)nnp * (double)m) : 0.0,
                   (st.ms_solve + st.ms_scatter) * 1e-3, nbatch > 1 ? " (in batches of rows)" : "");

        // the Schur complement becomes the matrix of the next round
        cur = std::move(next);
        cur_nnz = st.nnz_out;
        cur_live = st.rows_out;
        round++;
        if (cur_nnz == 0) break;
    }

    if (rank_only) {
        *rank_only = (i64)U.pivcol.size() + U.uncollected;
        spasm_logf("[echelonize] Done in %.1fs. Rank %lld%s (rank only: the rows of U stayed on the device)\n", spasm_wtime() - t0, (long long)*rank_only,
                   partial ? " (not finished: a lower bound)" : "");
        return nullptr;
    }
    struct spasm_lu *N = assemble_lu(U, n, m, prime, want_L ? &HL : nullptr);
    spasm_logf("[echelonize] Done in %.1fs. Rank %d%s, %lld nz in basis\n", spasm_wtime() - t0, N->r, partial ? " (not finished: a lower bound)" : "", (long long)U.p.back());
    return N;
}

// ---- the host LU from the rows of U collected round by round (layout reference src/SpaSM.jl:262-270; ownership :273-277)
struct spasm_lu *assemble_lu(HostU &U, int n, int m, i64 prime, HostL *HLp)
{
    const bool want_L = HLp != nullptr;
    const int r = (int)U.pivcol.size();
    struct spasm_csr *Uc = spasm_csr_alloc(r, m, 0, prime, true);
    if (!Uc) throw EngineError("out of host memory for U");
    memcpy(Uc->p, U.p.data(), sizeof(i64) * ((size_t)r + 1));
    if (!U.j.empty()) { // the buffers the entries were downloaded into become the arrays of U (malloc'ed, like spasm_csr_alloc's)
        free(Uc->j);
        free(Uc->x);
        Uc->nzmax = (i64)U.j.size();
        Uc->j = U.j.steal();
        Uc->x = U.x.steal();
    }
    struct spasm_lu *N = (struct spasm_lu *)malloc(sizeof *N);
    const int plen = std::max(std::max(n, m), 1);
    int *qinv = (int *)malloc(sizeof(int) * (size_t)std::max(m, 1));
    int *p = (int *)malloc(sizeof(int) * (size_t)plen);
    for (int j = 0; j < m; j++) qinv[j] = -1;
    for (int k = 0; k < r; k++) qinv[U.pivcol[(size_t)k]] = k;
    {
        // pivotal rows first, then the others in ascending order
        std::vector<char> used((size_t)std::max(n, 1), 0);
        int w = 0;
        for (int k = 0; k < r; k++) { p[w++] = U.orig[(size_t)k]; used[(size_t)U.orig[(size_t)k]] = 1; }
        for (int i = 0; i < n; i++) if (!used[(size_t)i]) p[w++] = i;
        for (; w < plen; w++) p[w] = -1;
    }
    struct spasm_csr *Lc = nullptr;
    if (want_L) {
        // rows of L in the order of the rows of A; inside a row the entries arrive round by round, i.e. by ascending row of U
        HostL &HL = *HLp;
        const i64 lnz = (i64)HL.j.size();
        Lc = spasm_csr_alloc(n, r, lnz, prime, true);
        if (!Lc) throw EngineError("out of host memory for L");
        std::vector<i64> cntr((size_t)n + 1, 0);
        for (i64 k = 0; k < lnz; k++) cntr[(size_t)HL.row[(size_t)k] + 1]++;
        for (int i = 0; i < n; i++) cntr[(size_t)i + 1] += cntr[(size_t)i];
        memcpy(Lc->p, cntr.data(), sizeof(i64) * ((size_t)n + 1));
        for (i64 k = 0; k < lnz; k++) {
            const i64 w = cntr[(size_t)HL.row[(size_t)k]]++;
            Lc->j[w] = HL.j[(size_t)k];
            Lc->x[w] = HL.x[(size_t)k];
        }
    }
    N->r = r;
    N->complete = false;
    N->L = Lc;
    N->U = Uc;
    N->qinv = qinv;
    N->p = p;
    N->Ltmp = nullptr;
    return N;
}


// ------------------------------------------------------------------------------------------------
// device transpose: column j of M becomes an output row when keep[j] < 0 (keep == NULL: every column);
// entries are labelled label[row] (NULL: the row index); diag = 1 prepends (j,-1) to every output row
// ------------------------------------------------------------------------------------------------
struct TransposeOut {
    int nrows = 0;
    i64 nnz = 0;
    DevBuf<i64d> Tp;
    DevBuf<int2> Tent;
};

void device_transpose(const DevMat &M, int nrowsM, const int *keep, const int *label, int diag, Scanner &scan, hipStream_t s, TransposeOut &out)
{
    const int m = M.m;
    DevBuf<int> cnt, flag, rowidx, cursor;
    DevBuf<i64d> tlen, tstart;
    cnt.alloc((size_t)m + 1);
    flag.alloc((size_t)m + 1);
    rowidx.alloc((size_t)m + 1);
    cursor.alloc((size_t)m + 1);
    tlen.alloc((size_t)m + 1);
    tstart.alloc((size_t)m + 1);
    cnt.zero(s);
    constexpr int TEAM = 8;
    if (nrowsM > 0) {
        hipLaunchKernelGGL((k_count_cols<TEAM>), dim3(cdiv((i64)nrowsM * TEAM, 256)), dim3(256), 0, s, nrowsM, M.start.p, M.len.p, M.ent.p, cnt.p);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_trow_len, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, s, m, keep, cnt.p, diag, tlen.p, flag.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(tlen.p, tstart.p, (size_t)m + 1, s);
    scan.exclusive(flag.p, rowidx.p, (size_t)m + 1, s);
    i64d tot = 0;
    int nrows = 0;
    HIPCHK(hipMemcpyAsync(&tot, tstart.p + m, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nrows, rowidx.p + m, sizeof nrows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out.nrows = nrows;
    out.nnz = tot;
    out.Tp.alloc((size_t)nrows + 1);
    out.Tent.alloc((size_t)tot + 1);
    hipLaunchKernelGGL(k_trow_ptr, dim3(cdiv((i64)m + 1, 256)), dim3(256), 0, s, m, keep, rowidx.p, tstart.p, diag, out.Tp.p, out.Tent.p, cursor.p);
    HIPCHK(hipGetLastError());
    if (nrowsM > 0) {
        hipLaunchKernelGGL((k_tfill<TEAM>), dim3(cdiv((i64)nrowsM * TEAM, 256)), dim3(256), 0, s, nrowsM, M.start.p, M.len.p, M.ent.p, label, tstart.p, cursor.p, out.Tent.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
}

struct spasm_csr *transpose_out_to_host(const TransposeOut &T, int ncols, i64 prime, hipStream_t s)
{
    struct spasm_csr *K = spasm_csr_alloc(T.nrows, ncols, T.nnz, prime, true);
    if (!K) throw EngineError("out of host memory");
    std::vector<int2> ent((size_t)T.nnz);
    HIPCHK(hipMemcpyAsync(K->p, T.Tp.p, ((size_t)T.nrows + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    if (T.nnz > 0) HIPCHK(hipMemcpyAsync(ent.data(), T.Tent.p, (size_t)T.nnz * sizeof(int2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (i64 k = 0; k < T.nnz; k++) { K->j[k] = ent[(size_t)k].x; K->x[k] = ent[(size_t)k].y; }
    return K;
}

struct spasm_csr *do_transpose(const struct spasm_csr *A)
{
    require_device();
    if (!A) throw EngineError("spasm_transpose: NULL matrix");
    hipStream_t s = nullptr;
    DevMat M;
    upload_csr(A, 0, A->n, M, s);
    Scanner scan;
    TransposeOut T;
    device_transpose(M, A->n, nullptr, nullptr, 0, scan, s, T);
    struct spasm_csr *R = transpose_out_to_host(T, A->n, A->field->p, s);
    if (!A->x) { free(R->x); R->x = nullptr; }
    return R;
}

// ------------------------------------------------------------------------------------------------
// Pivot numbering for the consumers of a factorization (kernel, rref, triangular solve): a topological order of
// "row a of U has an entry on the pivot column of row b  =>  a before b", which makes U_PP strictly upper triangular in
// pivot-index space -- what the solve kernels assume.  U produced by this engine is stored in such an order already
// (rounds in sequence; inside a round the open-column pivots, then the leftmost ones by ascending column), so the check
// is one pass; any other (permuted) triangular U gets a depth-first numbering.  Pivots need not be leftmost entries
// (reference src/SpaSM.jl:712 only promises unit pivots).  Returns perm (perm[t] = row of U with pivot index t) and fills
// pc (pivot column of each row).
// ------------------------------------------------------------------------------------------------
static std::vector<int> pivot_topological_order(const struct spasm_csr *U, const int *qinv, const char *who, std::vector<int> &pc)
{
    const int r = U->n, m = U->m;
    const std::string w(who);
    pc.assign((size_t)std::max(r, 1), -1);
    int named = 0;
    for (int j = 0; j < m; j++) {
        const int a = qinv[j];
        if (a >= r) throw EngineError(w + ": qinv points outside U");
        if (a >= 0) { if (pc[(size_t)a] < 0) named++; pc[(size_t)a] = j; }
    }
    if (named != r) throw EngineError(w + ": qinv does not name one pivot column per row of U");
    // (one pass over the entries of U, on all host threads: U has 10^9 entries on the large cases)
    int bad_unit = 0, unordered = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(| : bad_unit, unordered)
    for (int a = 0; a < r; a++) {
        bool unit = false;
        const int pca = pc[(size_t)a];
        for (i64 k = U->p[a]; k < U->p[a + 1]; k++) {
            const int j = U->j[k];
            if (j == pca) { if (U->x[k] == 1) unit = true; continue; }
            const int b = qinv[j];
            if (b >= 0 && b < a) unordered = 1;
        }
        if (!unit) bad_unit = 1;
    }
    if (bad_unit) throw EngineError(w + ": pivots of U must be 1");
    std::vector<int> perm((size_t)std::max(r, 1));
    const bool ordered = !unordered;
    if (ordered) {
        for (int a = 0; a < r; a++) perm[(size_t)a] = a;
        return perm;
    }
    std::vector<char> state((size_t)r, 0);
    std::vector<int> stack, post;
    std::vector<i64> pos((size_t)r, 0);
    post.reserve((size_t)r);
    for (int root = 0; root < r; root++) {
        if (state[(size_t)root]) continue;
        stack.push_back(root);
        state[(size_t)root] = 1;
        pos[(size_t)root] = U->p[root];
        while (!stack.empty()) {
            const int a = stack.back();
            bool pushed = false;
            while (pos[(size_t)a] < U->p[a + 1]) {
                const int b = qinv[U->j[pos[(size_t)a]++]];
                if (b < 0 || b == a) continue;
                if (state[(size_t)b] == 1) throw EngineError(w + ": U is not (permuted) triangular");
                if (state[(size_t)b] == 0) {
                    state[(size_t)b] = 1;
                    pos[(size_t)b] = U->p[b];
                    stack.push_back(b);
                    pushed = true;
                    break;
                }
            }
            if (!pushed) { state[(size_t)a] = 2; post.push_back(a); stack.pop_back(); }
        }
    }
    for (int t = 0; t < r; t++) perm[(size_t)t] = post[(size_t)(r - 1 - t)];
    return perm;
}

// ------------------------------------------------------------------------------------------------
// kernel basis from an echelonized U (reference call site src/SpaSM.jl:879).
// The reduced row echelon form R of U is computed with the SAME solve + scatter kernels as a Schur
// round (each row of U is reduced by all the others); the kernel vector of free column j is then
// -e_j + sum_a R[a][j] e_{pivcol(a)}: a transpose of R's free part (known answers test/runtests.jl:20-23).
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// spasm_rref (reference src/SpaSM.jl:871): the reduced row echelon form of U.  Row k of R is row k of U minus the
// combination of the OTHER rows that clears its entries on their pivot columns -- one Schur "round" in which every row
// of U is a pivot row and, at the same time, a row to reduce with its own pivot excluded (self_idx).  The pivots are
// numbered in a topological order (pivot_topological_order), so they need not be leftmost entries.
// ------------------------------------------------------------------------------------------------
struct spasm_csr *do_rref(const struct spasm_lu *fact, int *Rqinv)
{
    require_device();
    if (!fact || !fact->U || !fact->qinv) throw EngineError("spasm_rref: incomplete factorization (U / qinv missing)");
    const struct spasm_csr *U = fact->U;
    check_input(U, "spasm_rref");
    const int r = U->n, m = U->m;
    const int *qinv = fact->qinv;
    const i64 prime = U->field->p;
    // pivots numbered in topological order: idx -> (column, row of U)
    std::vector<int> pc;
    const std::vector<int> perm = pivot_topological_order(U, qinv, "spasm_rref", pc);
    std::vector<int> h_qinv_r((size_t)std::max(m, 1), -1), h_pivcol((size_t)r), h_pivrow((size_t)r), h_self((size_t)std::max(r, 1), -1);
    for (int t = 0; t < r; t++) {
        const int k = perm[(size_t)t];
        h_qinv_r[(size_t)pc[(size_t)k]] = t;
        h_self[(size_t)k] = t;
        h_pivcol[(size_t)t] = pc[(size_t)k];
        h_pivrow[(size_t)t] = k;
    }
    struct spasm_csr *Rm = nullptr;
    std::vector<i64> sp((size_t)r + 1, 0);
    std::vector<int> sj, sx;
    if (r > 0) {
        hipStream_t s = nullptr;
        DevMat PM;
        upload_csr(U, 0, r, PM, s);
        std::unique_ptr<Round> R(new Round());
        R->F = zp_field_make(prime);
        R->stream = s;
        R->m = m;
        R->npiv = r;
        R->nnp = r;
        R->qinv_r.alloc((size_t)m + 1);
        R->pivcol.alloc((size_t)r + 1);
        R->pivrow.alloc((size_t)r + 1);
        R->np_rows.alloc((size_t)r + 1);
        DevBuf<int> self;
        self.alloc((size_t)r + 1);
        HIPCHK(hipMemcpyAsync(R->qinv_r.p, h_qinv_r.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(R->pivcol.p, h_pivcol.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(R->pivrow.p, h_pivrow.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(self.p, h_self.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_iota, dim3(cdiv(r, 256)), dim3(256), 0, s, r, R->np_rows.p);
        HIPCHK(hipGetLastError());
        R->build_U(PM, R->pivrow.p);
        R->prepare_uinv(r);
        const i64 tot = R->solve_phase(PM, R->np_rows.p, self.p, r, 4 * spasm_nnz(U));
        R->S.ent.ensure((size_t)tot + 1);
        R->run_scatter(PM, R->np_rows.p, r);
        R->fetch_counters();
        // the non-pivot parts of the reduced rows, compacted on the device
        DevBuf<i64d> len64, ostart;
        len64.alloc((size_t)r + 1);
        ostart.alloc((size_t)r + 1);
        hipLaunchKernelGGL(k_copy_len64, dim3(cdiv((i64)r + 1, 256)), dim3(256), 0, s, r, R->S.len.p, len64.p);
        HIPCHK(hipGetLastError());
        R->scan.exclusive(len64.p, ostart.p, (size_t)r + 1, s);
        HIPCHK(hipMemcpyAsync(sp.data(), ostart.p, ((size_t)r + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const i64 nz = sp[(size_t)r];
        DevBuf<int> oj, ox;
        oj.alloc((size_t)nz + 1);
        ox.alloc((size_t)nz + 1);
        constexpr int TEAM = 16;
        hipLaunchKernelGGL((k_compact_rows<TEAM>), dim3(cdiv((i64)r * TEAM, 256)), dim3(256), 0, s, r, R->S.start.p, R->S.len.p, R->S.ent.p, ostart.p, oj.p, ox.p);
        HIPCHK(hipGetLastError());
        sj.resize((size_t)nz);
        sx.resize((size_t)nz);
        if (nz > 0) {
            HIPCHK(hipMemcpyAsync(sj.data(), oj.p, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(sx.data(), ox.p, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
    }
    const i64 total = (r > 0 ? sp[(size_t)r] : 0) + r;
    Rm = spasm_csr_alloc(r, m, total, prime, true);
    if (!Rm) throw EngineError("out of host memory for R");
    i64 w = 0;
    for (int k = 0; k < r; k++) {
        Rm->p[k] = w;
        Rm->j[w] = h_pivcol[(size_t)h_self[(size_t)k]];
        Rm->x[w] = 1;
        w++;
        const i64 a = sp[(size_t)k], b = sp[(size_t)k + 1];
        if (b > a) {
            memcpy(Rm->j + w, sj.data() + a, (size_t)(b - a) * sizeof(int));
            memcpy(Rm->x + w, sx.data() + a, (size_t)(b - a) * sizeof(int));
            w += b - a;
        }
    }
    Rm->p[r] = w;
    if (Rqinv) for (int j = 0; j < m; j++) Rqinv[j] = qinv[j];
    return Rm;
}

// ------------------------------------------------------------------------------------------------
// X * U = B for every row of B at once (the reference loops spasm_sparse_triangular_solve over the rows of B,
// src/SpaSM.jl:733-755): with x_b on the pivot columns and x_a on the others, x_b * U + x_a == B[k] (:694-713).  One Schur
// "round" with U as the pivot rows and B as the rows to reduce: the multipliers ARE x_b, the Schur row IS x_a.
// Returns X (rows of B x rows of U); ok[k] = 1 when x_a is empty, i.e. row k has a solution.  Same pivot numbering as rref.
// ------------------------------------------------------------------------------------------------
// resid (may be NULL): receives x_a, the part of B[k] - x_b * U on the columns without a pivot, one row per row of B
struct spasm_csr *do_trisolve(const struct spasm_csr *U, const int *qinv, const struct spasm_csr *B, unsigned char *ok, struct spasm_csr **resid)
{
    require_device();
    if (!U || !qinv || !B) throw EngineError("spasm_amd_triangular_solve: null argument");
    check_input(U, "spasm_amd_triangular_solve");
    check_input(B, "spasm_amd_triangular_solve");
    const int r = U->n, m = U->m, nb = B->n;
    const i64 prime = U->field->p;
    if (B->m != m || B->field->p != prime) throw EngineError("spasm_amd_triangular_solve: B and U differ in columns or field");
    std::vector<int> pc;
    const std::vector<int> perm = pivot_topological_order(U, qinv, "spasm_amd_triangular_solve", pc);
    std::vector<int> h_qinv_r((size_t)std::max(m, 1), -1), h_pivcol((size_t)r), h_pivrow((size_t)r);
    for (int t = 0; t < r; t++) {
        const int k = perm[(size_t)t];
        h_qinv_r[(size_t)pc[(size_t)k]] = t;
        h_pivcol[(size_t)t] = pc[(size_t)k];
        h_pivrow[(size_t)t] = k;
    }
    std::vector<i64> xp((size_t)nb + 1, 0);
    std::vector<int> slen((size_t)std::max(nb, 1), 0);
    struct spasm_csr *X = nullptr;
    if (nb > 0 && r > 0) {
        hipStream_t s = nullptr;
        DevMat PM, BM;
        upload_csr(U, 0, r, PM, s);
        upload_csr(B, 0, nb, BM, s);
        std::unique_ptr<Round> R(new Round());
        R->F = zp_field_make(prime);
        R->stream = s;
        R->m = m;
        R->npiv = r;
        R->nnp = nb;
        R->qinv_r.alloc((size_t)m + 1);
        R->pivcol.alloc((size_t)r + 1);
        R->pivrow.alloc((size_t)r + 1);
        R->np_rows.alloc((size_t)nb + 1);
        HIPCHK(hipMemcpyAsync(R->qinv_r.p, h_qinv_r.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(R->pivcol.p, h_pivcol.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(R->pivrow.p, h_pivrow.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_iota, dim3(cdiv(nb, 256)), dim3(256), 0, s, nb, R->np_rows.p);
        HIPCHK(hipGetLastError());
        R->want_idx = true; // X is assembled from (pivot index, multiplier)
        R->build_U(PM, R->pivrow.p);
        R->prepare_uinv(nb);
        const i64 tot = R->solve_phase(BM, R->np_rows.p, nullptr, nb, 4 * (spasm_nnz(B) + spasm_nnz(U)));
        R->S.ent.ensure((size_t)tot + 1);
        R->run_scatter(BM, R->np_rows.p, nb);
        R->fetch_counters();
        DevBuf<i64d> xlen, xstart;
        xlen.alloc((size_t)nb + 1);
        xstart.alloc((size_t)nb + 1);
        hipLaunchKernelGGL(k_xcount, dim3(cdiv(((i64)nb + 1) * 64, 256)), dim3(256), 0, s, nb, R->Lstart.p, R->Llen.p, R->Lpool.p, xlen.p);
        HIPCHK(hipGetLastError());
        R->scan.exclusive(xlen.p, xstart.p, (size_t)nb + 1, s);
        HIPCHK(hipMemcpyAsync(xp.data(), xstart.p, ((size_t)nb + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(slen.data(), R->S.len.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const i64 nz = xp[(size_t)nb];
        X = spasm_csr_alloc(nb, r, nz, prime, true);
        if (!X) throw EngineError("out of host memory for X");
        if (nz > 0) {
            DevBuf<int> oj, ox;
            oj.alloc((size_t)nz);
            ox.alloc((size_t)nz);
            hipLaunchKernelGGL(k_xfill, dim3(cdiv((i64)nb * 64, 256)), dim3(256), 0, s, nb, R->pivrow.p, R->Lstart.p, R->Llen.p, R->Lpool.p, R->Lidx.p, xstart.p,
                               oj.p, ox.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(X->j, oj.p, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(X->x, ox.p, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        for (int k = 0; k <= nb; k++) X->p[k] = xp[(size_t)k];
        if (resid) {
            // x_a: the Schur rows of the rows of B, compacted (device) and copied out
            DevBuf<i64d> l64, rstart2;
            l64.alloc((size_t)nb + 1);
            rstart2.alloc((size_t)nb + 1);
            hipLaunchKernelGGL(k_copy_len64, dim3(cdiv((i64)nb + 1, 256)), dim3(256), 0, s, nb, R->S.len.p, l64.p);
            HIPCHK(hipGetLastError());
            R->scan.exclusive(l64.p, rstart2.p, (size_t)nb + 1, s);
            std::vector<i64d> hp2((size_t)nb + 1);
            HIPCHK(hipMemcpyAsync(hp2.data(), rstart2.p, ((size_t)nb + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const i64 rz = hp2[(size_t)nb];
            struct spasm_csr *Rs = spasm_csr_alloc(nb, m, rz, prime, true);
            if (!Rs) { spasm_csr_free(X); throw EngineError("out of host memory for the residual rows"); }
            for (int k = 0; k <= nb; k++) Rs->p[k] = hp2[(size_t)k];
            if (rz > 0) {
                DevBuf<int> oj2, ox2;
                oj2.alloc((size_t)rz);
                ox2.alloc((size_t)rz);
                constexpr int TEAM = 16;
                hipLaunchKernelGGL((k_compact_rows<TEAM>), dim3(cdiv((i64)nb * TEAM, 256)), dim3(256), 0, s, nb, R->S.start.p, R->S.len.p, R->S.ent.p, rstart2.p, oj2.p, ox2.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(Rs->j, oj2.p, (size_t)rz * sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHK(hipMemcpyAsync(Rs->x, ox2.p, (size_t)rz * sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
            }
            *resid = Rs;
        }
    } else {
        X = spasm_csr_alloc(nb, r, 0, prime, true);
        if (!X) throw EngineError("out of host memory for X");
        for (int k = 0; k <= nb; k++) X->p[k] = 0;
        for (int k = 0; k < nb; k++) slen[(size_t)k] = (int)(B->p[k + 1] - B->p[k]); // without pivots a row is solvable iff it is zero
        if (resid) {
            // no pivots (or no rows): x_a is the row itself
            const i64 bz = B->p[nb];
            struct spasm_csr *Rs = spasm_csr_alloc(nb, m, bz, prime, true);
            if (!Rs) { spasm_csr_free(X); throw EngineError("out of host memory for the residual rows"); }
            const ZpField F = zp_field_make(prime);
            for (int k = 0; k <= nb; k++) Rs->p[k] = B->p[k];
            for (i64 t = 0; t < bz; t++) { Rs->j[t] = B->j[t]; Rs->x[t] = zp_reduce(F, B->x[t]); }
            *resid = Rs;
        }
    }
    if (ok) for (int k = 0; k < nb; k++) ok[k] = slen[(size_t)k] == 0;
    return X;
}

// ------------------------------------------------------------------------------------------------
// spasm_gesv / spasm_solve (reference src/SpaSM.jl:895-923): X * A == B from a factorization that carries L (echelonize_opts.L).
// With A[i] = sum_k L[i][k] U[k]:  X * A = (X * L) * U, so   Y * U = B  (the batched triangular solve on the device, Y is
// nb x r), then  X_P * L_P = Y  on the pivotal rows p[0 .. r) of A, whose rows of L form a lower triangular r x r matrix with the
// pivots d_k = L[p[k]][k] on the diagonal (a row only holds multipliers of pivots elected before it).  Scaled to a unit diagonal
// this is a second triangular solve of the same kind; X is zero outside the pivotal rows.  ok[b] = 1 when row b has a solution.
// ------------------------------------------------------------------------------------------------
struct spasm_csr *do_trisolve(const struct spasm_csr *U, const int *qinv, const struct spasm_csr *B, unsigned char *ok, struct spasm_csr **resid = nullptr);

struct spasm_csr *do_gesv(const struct spasm_lu *fact, const struct spasm_csr *B, unsigned char *ok)
{
    if (!fact || !fact->U || !fact->qinv || !fact->p) throw EngineError("incomplete factorization (U / qinv / p missing)");
    if (!fact->L) throw EngineError("the factorization has no L: echelonize with L = true (reference src/SpaSM.jl:331)");
    if (!B) throw EngineError("null right-hand side");
    const struct spasm_csr *U = fact->U, *L = fact->L;
    const int r = U->n, n = L->n, nb = B->n;
    const i64 prime = U->field->p;
    if (L->m != r) throw EngineError("L must have one column per row of U");
    const ZpField F = zp_field_make(prime);
    // the pivotal rows of L, scaled to a unit diagonal
    std::vector<int> diag((size_t)std::max(r, 1), 0);
    i64 mnz = 0;
    for (int k = 0; k < r; k++) {
        const int i = fact->p[k];
        if (i < 0 || i >= n) throw EngineError("p does not name a row of A for every row of U");
        mnz += L->p[i + 1] - L->p[i];
    }
    struct spasm_csr *M = spasm_csr_alloc(r, r, mnz, prime, true);
    if (!M) throw EngineError("out of host memory");
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Mguard(M, spasm_csr_free);
    i64 w = 0;
    for (int k = 0; k < r; k++) {
        const int i = fact->p[k];
        M->p[k] = w;
        int d = 0;
        for (i64 q = L->p[i]; q < L->p[i + 1]; q++) {
            if (L->j[q] > k) throw EngineError("L is not triangular on the pivotal rows");
            if (L->j[q] == k) d = L->x[q];
        }
        if (d == 0) throw EngineError("L has a zero on its diagonal");
        diag[(size_t)k] = d;
        const int dinv = zp_inverse(F, d);
        for (i64 q = L->p[i]; q < L->p[i + 1]; q++) {
            M->j[w] = L->j[q];
            M->x[w] = L->j[q] == k ? 1 : zp_mul(F, dinv, L->x[q]);
            w++;
        }
    }
    M->p[r] = w;
    std::vector<int> ident((size_t)std::max(r, 1));
    for (int k = 0; k < r; k++) ident[(size_t)k] = k;
    std::vector<unsigned char> ok1((size_t)std::max(nb, 1), 0), ok2((size_t)std::max(nb, 1), 0);
    struct spasm_csr *Y = do_trisolve(U, fact->qinv, B, ok1.data());
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Yguard(Y, spasm_csr_free);
    struct spasm_csr *Xs = do_trisolve(M, ident.data(), Y, ok2.data());
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Xguard(Xs, spasm_csr_free);
    // X[b][p[k]] = Xs[b][k] / d_k
    struct spasm_csr *X = spasm_csr_alloc(nb, n, spasm_nnz(Xs), prime, true);
    if (!X) throw EngineError("out of host memory for X");
    std::vector<int> dinv((size_t)std::max(r, 1));
    for (int k = 0; k < r; k++) dinv[(size_t)k] = zp_inverse(F, diag[(size_t)k]);
    for (int b = 0; b <= nb; b++) X->p[b] = Xs->p[b];
    for (i64 q = 0; q < Xs->p[nb]; q++) {
        const int k = Xs->j[q];
        X->j[q] = fact->p[k];
        X->x[q] = zp_mul(F, Xs->x[q], dinv[(size_t)k]);
    }
    if (ok) for (int b = 0; b < nb; b++) ok[b] = ok1[(size_t)b] && ok2[(size_t)b];
    return X;
}

// first / step: only the free columns number first, first + step, ... (in ascending column order) get their kernel vector:
// the unit of the multi-GPU kernel step (free columns are independent)
struct spasm_csr *do_kernel_core(const struct spasm_csr *U, const int *qinv, int first, int step);

// The part of U a kernel basis needs.  The kernel vector of free column j is -e_j + sum_a y_a e_{pivcol(a)} with
//        y_a = U[a][j] - sum_{b != a} U[a][pivcol(b)] y_b,
// so y_a can only be non-zero when row a holds an entry on a (selected) free column or on the pivot column of a row b that can:
// the rows outside that closure have y = 0 for every free column and drop out, with the pivot columns they own (qinv = -2 below:
// neither free nor a pivot of what is left).  For the factorizations whose U does not fit the device as one round (config 5 at
// 1/3: 5.5e9 entries; the round's U has 32-bit offsets) the closure is what is solved instead -- a few rows when the kernel
// vectors are sparse, all of U when they are not (then the limit stands).  Host side, all threads: one pass for the free columns,
// then sweeps over the rows not yet in the closure until nothing changes.
struct KernelReduced {
    struct spasm_csr *U2 = nullptr;
    std::vector<int> qinv2;
    ~KernelReduced() { if (U2) spasm_csr_free(U2); }
};

void kernel_closure(const struct spasm_csr *U, const int *qinv, int first, int step, KernelReduced &out)
{
    const int r = U->n, m = U->m;
    std::vector<unsigned char> sel((size_t)std::max(m, 1), 0);
    {
        int f = 0;
        for (int j = 0; j < m; j++)
            if (qinv[j] < 0 && qinv[j] != -2) {
                if (f >= first && (f - first) % step == 0) sel[(size_t)j] = 1;
                f++;
            }
    }
    std::vector<unsigned char> need((size_t)std::max(r, 1), 0);
    unsigned char *nd = need.data();
    int any = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(| : any)
    for (int a = 0; a < r; a++)
        for (i64 k = U->p[a]; k < U->p[a + 1]; k++)
            if (sel[(size_t)U->j[k]] && U->x[k] != 0) { __atomic_store_n(&nd[a], 1, __ATOMIC_RELAXED); any = 1; break; }
    int sweeps = 0;
    for (int changed = any; changed; sweeps++) {
        changed = 0;
        // (descending: in a U whose rows come in elimination order a row refers to later rows, and a chain closes in one sweep)
#pragma omp parallel for schedule(static, 4096) reduction(| : changed)
        for (int i = 0; i < r; i++) {
            const int a = r - 1 - i;
            if (__atomic_load_n(&nd[a], __ATOMIC_RELAXED)) continue;
            for (i64 k = U->p[a]; k < U->p[a + 1]; k++) {
                const int b = qinv[U->j[k]];
                if (b >= 0 && b != a && U->x[k] != 0 && __atomic_load_n(&nd[b], __ATOMIC_RELAXED)) {
                    __atomic_store_n(&nd[a], 1, __ATOMIC_RELAXED);
                    changed = 1;
                    break;
                }
            }
        }
    }
    std::vector<int> newidx((size_t)std::max(r, 1), -1);
    int r2 = 0;
    for (int a = 0; a < r; a++) if (need[(size_t)a]) newidx[(size_t)a] = r2++;
    out.qinv2.assign((size_t)std::max(m, 1), -1);
    for (int j = 0; j < m; j++) {
        const int a = qinv[j];
        out.qinv2[(size_t)j] = a < 0 ? a : (newidx[(size_t)a] >= 0 ? newidx[(size_t)a] : -2);
    }
    std::vector<i64> cnt((size_t)r2 + 1, 0);
#pragma omp parallel for schedule(dynamic, 1024)
    for (int a = 0; a < r; a++) {
        if (!need[(size_t)a]) continue;
        i64 c = 0;
        for (i64 k = U->p[a]; k < U->p[a + 1]; k++) c += out.qinv2[(size_t)U->j[k]] != -2;
        cnt[(size_t)newidx[(size_t)a] + 1] = c;
    }
    for (int t = 0; t < r2; t++) cnt[(size_t)t + 1] += cnt[(size_t)t];
    out.U2 = spasm_csr_alloc(r2, m, std::max<i64>(cnt[(size_t)r2], 1), U->field->p, true);
    if (!out.U2) throw EngineError("out of host memory");
    for (int t = 0; t <= r2; t++) out.U2->p[t] = cnt[(size_t)t];
#pragma omp parallel for schedule(dynamic, 1024)
    for (int a = 0; a < r; a++) {
        if (!need[(size_t)a]) continue;
        i64 w = cnt[(size_t)newidx[(size_t)a]];
        for (i64 k = U->p[a]; k < U->p[a + 1]; k++)
            if (out.qinv2[(size_t)U->j[k]] != -2) { out.U2->j[w] = U->j[k]; out.U2->x[w] = U->x[k]; w++; }
    }
    spasm_logf("[kernel] closure of the free columns: %d of %d rows of U, %lld of %lld entries (%d sweeps)\n", r2, r, (long long)cnt[(size_t)r2], (long long)spasm_nnz(U), sweeps);
}

#include "kernel_dense.hpp"

// spasm_kernel through a dense right-hand side (kernel_dense.hpp): every free column at once, the dense tail of U on the int8 GEMM,
// the sparse rows level by level.  For primes below 2^16 (the element types of the dense finish).  dense_tail_rows < 0: chosen by
// density.  Returns NULL when Y (r x free columns) or the dense tail do not fit the device: the caller falls back.
template <typename DT>
struct spasm_csr *kernel_dense_rhs(const struct spasm_csr *U, const int *qinv, int first, int step, i64 dense_tail_rows)
{
    const int r = U->n, m = U->m;
    const i64 prime = U->field->p;
    const ZpField F = zp_field_make(prime);
    const double t_start = spasm_wtime();
    spasm_logf("[kernel] start. U is %d x %d (%lld nnz). All free columns at once: a dense right-hand side\n", r, m, (long long)spasm_nnz(U));
    std::vector<int> pc;
    const std::vector<int> perm = pivot_topological_order(U, qinv, "spasm_kernel", pc);
    std::vector<int> pos_of_row((size_t)std::max(r, 1), 0), pivcol_of_pos((size_t)std::max(r, 1), 0);
    for (int t = 0; t < r; t++) { pos_of_row[(size_t)perm[(size_t)t]] = t; pivcol_of_pos[(size_t)t] = pc[(size_t)perm[(size_t)t]]; }
    std::vector<int> h_free, fidx((size_t)std::max(m, 1), -1);
    {
        int f = 0;
        for (int j = 0; j < m; j++)
            if (qinv[j] < 0 && qinv[j] != -2) {
                if (f >= first && (f - first) % step == 0) { fidx[(size_t)j] = (int)h_free.size(); h_free.push_back(j); }
                f++;
            }
    }
    const int nf = (int)h_free.size();
    if (nf == 0) {
        struct spasm_csr *K = spasm_csr_alloc(0, m, 1, prime, true);
        if (!K) throw EngineError("out of host memory");
        K->p[0] = 0;
        return K;
    }
    const i64 ldz = ((i64)nf + 63) / 64 * 64;
    size_t fr = 0, tot_mem = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot_mem));
    if ((double)std::max(r, 1) * (double)ldz * sizeof(DT) > 0.4 * (double)fr) return nullptr;
    // ---- the dense tail: the longest run of last positions that is dense enough to be worth a dense block (any run is CORRECT: a
    // row only refers to pivots behind it, so the rows of a tail refer to the tail and to free columns only)
    int t0 = r;
    {
        const double budget = 0.35 * (double)fr;
        if (dense_tail_rows >= 0) t0 = r - (int)std::min<i64>(dense_tail_rows, r);
        else {
            // The rows of a dense finish come last in U and hold nearly all of its entries: take the shortest tail that holds 99 %
            // (then 90, 75, 50 %) of the entries of U, provided it IS dense (a twentieth of its triangle + free columns) and fits.
            // (Per-row rules fail on the residual rows of a tall finish, which are short and still belong to the tail.)
            std::vector<double> cum((size_t)r + 1, 0.0); // cum[t] = entries of the positions t .. r-1
            for (int t = r - 1; t >= 0; t--) { const int a = perm[(size_t)t]; cum[(size_t)t] = cum[(size_t)t + 1] + (double)(U->p[a + 1] - U->p[a]); }
            const double cover[4] = {0.99, 0.90, 0.75, 0.50};
            for (int q = 0; q < 4 && t0 == r; q++) {
                int lo = 0, hi = r; // the largest t with cum[t] >= cover * total (cum is non-increasing in t)
                while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (cum[(size_t)mid] >= cover[q] * cum[0]) lo = mid; else hi = mid - 1; }
                const double rows = (double)(r - lo);
                if (rows >= 256 && cum[(size_t)lo] >= 0.05 * rows * (0.5 * rows + nf) && rows * (rows + nf + 64) * sizeof(DT) <= budget) t0 = lo;
            }
        }
        const double rows = (double)(r - t0);
        if (rows * (rows + nf + 64) * sizeof(DT) > budget) return nullptr;
    }
    const int rd = r - t0;
    hipStream_t s = nullptr;
    DevBuf<DT> Y;
    Y.alloc((size_t)std::max(r, 1) * (size_t)ldz);
    Y.zero(s);
    DevBuf<int> d_qinv, d_pos, d_fidx;
    d_qinv.alloc((size_t)m + 1); d_pos.alloc((size_t)r + 1); d_fidx.alloc((size_t)m + 1);
    HIPCHK(hipMemcpyAsync(d_qinv.p, qinv, (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
    if (r > 0) HIPCHK(hipMemcpyAsync(d_pos.p, pos_of_row.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_fidx.p, fidx.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
    const double t_prep = spasm_wtime();
    double t_dense_rows = t_prep, t_z = t_prep;
    if (rd > 0) {
        // D1[k][0 .. rd) = the pivot columns of the tail in position order (the pivot of row k on column k), [rd, rd + nf) = the free columns
        const i64 ldc = ((i64)rd + nf + 63) / 64 * 64;
        DevBuf<DT> D1;
        D1.alloc((size_t)rd * (size_t)ldc);
        D1.zero(s);
        const i64 CH = (i64)1 << 28; // entries per chunk of rows on their way to the device
        std::vector<i64> hptr;
        std::vector<int> hj, hx;
        DevBuf<i64d> dptr;
        DevBuf<int> dj, dx;
        // (rows that lie one behind the other in U -- the usual case: U in elimination order -- go to the device from where they are)
        bool contig = true;
        for (int t = t0; t < r && contig; t++) contig = perm[(size_t)t] == perm[(size_t)t0] + (t - t0);
        for (int ta = t0; ta < r;) {
            int tb = ta;
            i64 ne = 0;
            while (tb < r) {
                const int a = perm[(size_t)tb];
                const i64 len = U->p[a + 1] - U->p[a];
                if (tb > ta && ne + len > CH) break;
                ne += len;
                tb++;
            }
            const int nk = tb - ta;
            hptr.assign((size_t)nk + 1, 0);
            for (int k = 0; k < nk; k++) { const int a = perm[(size_t)(ta + k)]; hptr[(size_t)k + 1] = hptr[(size_t)k] + (U->p[a + 1] - U->p[a]); }
            const int *src_j = nullptr, *src_x = nullptr;
            if (contig) {
                const i64 base = U->p[perm[(size_t)ta]];
                src_j = U->j + base; src_x = U->x + base;
            } else {
                hj.resize((size_t)std::max<i64>(ne, 1)); hx.resize((size_t)std::max<i64>(ne, 1));
#pragma omp parallel for schedule(dynamic, 64)
                for (int k = 0; k < nk; k++) {
                    const int a = perm[(size_t)(ta + k)];
                    const i64 len = U->p[a + 1] - U->p[a];
                    memcpy(hj.data() + hptr[(size_t)k], U->j + U->p[a], (size_t)len * sizeof(int));
                    memcpy(hx.data() + hptr[(size_t)k], U->x + U->p[a], (size_t)len * sizeof(int));
                }
                src_j = hj.data(); src_x = hx.data();
            }
            dptr.ensure((size_t)nk + 1); dj.ensure((size_t)std::max<i64>(ne, CH) + 1); dx.ensure((size_t)std::max<i64>(ne, CH) + 1);
            HIPCHK(hipMemcpyAsync(dptr.p, hptr.data(), ((size_t)nk + 1) * sizeof(i64), hipMemcpyHostToDevice, s));
            if (ne > 0) {
                HIPCHK(hipMemcpyAsync(dj.p, src_j, (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(dx.p, src_x, (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s));
            }
            hipLaunchKernelGGL((k_kd_dense_rows<DT>), dim3(nk), dim3(256), 0, s, nk, ta - t0, dptr.p, dj.p, dx.p, d_qinv.p, d_pos.p, d_fidx.p, t0, rd, D1.p, (i64d)ldc);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s)); // (the staging vectors are reused)
            ta = tb;
        }
        t_dense_rows = spasm_wtime();
        DevBuf<int> prow, fcol; // (prow = pcol = 0 .. rd-1)
        prow.alloc((size_t)rd + 1); fcol.alloc((size_t)nf + 1);
        hipLaunchKernelGGL(k_iota, dim3(cdiv(rd, 256)), dim3(256), 0, s, rd, prow.p);
        hipLaunchKernelGGL(k_iota_from, dim3(cdiv(nf, 256)), dim3(256), 0, s, nf, rd, fcol.p);
        HIPCHK(hipGetLastError());
        TallWork<DT> W(F, s);
        tall_reduced_form<DT>(W, D1.p, ldc, rd, prow.p, prow.p, fcol.p, nf, Y.p + (size_t)t0 * (size_t)ldz, ldz, F, s);
        HIPCHK(hipStreamSynchronize(s));
        t_z = spasm_wtime();
    }
    // ---- the sparse rows: positions [0, t0), level by level (level 0: rows that refer to no other sparse row)
    int nlev = 0;
    if (t0 > 0) {
        std::vector<int> lev((size_t)t0, 0);
        std::vector<i64> eptr((size_t)t0 + 1, 0);
        for (int t = t0 - 1; t >= 0; t--) { // (descending: a row refers to positions behind it)
            const int a = perm[(size_t)t];
            int lv = 0;
            i64 n = 0;
            for (i64 k = U->p[a]; k < U->p[a + 1]; k++) {
                const int c = U->j[k];
                const int b = qinv[c];
                if (b == a || U->x[k] == 0) continue;
                if (b >= 0) { const int pos = pos_of_row[(size_t)b]; if (pos < t0) lv = std::max(lv, lev[(size_t)pos] + 1); n++; }
                else if (fidx[(size_t)c] >= 0) n++;
            }
            lev[(size_t)t] = lv;
            eptr[(size_t)t + 1] = n;
            nlev = std::max(nlev, lv + 1);
        }
        for (int t = 0; t < t0; t++) eptr[(size_t)t + 1] += eptr[(size_t)t];
        const i64 ne = eptr[(size_t)t0];
        // (a U whose dense rows did not end up in the tail would be solved row after row here: hours.  Not this path's case.)
        if ((double)ne * (double)nf > 4e14 || (nlev > (1 << 20) && (double)ne > 1e9)) return nullptr;
        std::vector<int2> hent((size_t)std::max<i64>(ne, 1));
#pragma omp parallel for schedule(dynamic, 1024)
        for (int t = 0; t < t0; t++) {
            const int a = perm[(size_t)t];
            i64 w = eptr[(size_t)t];
            for (i64 k = U->p[a]; k < U->p[a + 1]; k++) {
                const int c = U->j[k];
                const int b = qinv[c];
                if (b == a || U->x[k] == 0) continue;
                if (b >= 0) hent[(size_t)w++] = make_int2(pos_of_row[(size_t)b], U->x[k]);
                else if (fidx[(size_t)c] >= 0) hent[(size_t)w++] = make_int2(-1 - fidx[(size_t)c], U->x[k]);
            }
        }
        std::vector<int> lstart((size_t)nlev + 1, 0), order((size_t)t0);
        for (int t = 0; t < t0; t++) lstart[(size_t)lev[(size_t)t] + 1]++;
        for (int l = 0; l < nlev; l++) lstart[(size_t)l + 1] += lstart[(size_t)l];
        {
            std::vector<int> at(lstart.begin(), lstart.end() - 1);
            for (int t = 0; t < t0; t++) order[(size_t)at[(size_t)lev[(size_t)t]]++] = t;
        }
        DevBuf<i64d> dptr;
        DevBuf<int2> dent;
        DevBuf<int> dord;
        dptr.alloc((size_t)t0 + 1); dent.alloc((size_t)ne + 1); dord.alloc((size_t)t0 + 1);
        HIPCHK(hipMemcpyAsync(dptr.p, eptr.data(), ((size_t)t0 + 1) * sizeof(i64), hipMemcpyHostToDevice, s));
        if (ne > 0) HIPCHK(hipMemcpyAsync(dent.p, hent.data(), (size_t)ne * sizeof(int2), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dord.p, order.data(), (size_t)t0 * sizeof(int), hipMemcpyHostToDevice, s));
        const int ctiles = cdiv(nf, 1024);
        for (int l = 0; l < nlev; l++) {
            const int cnt = lstart[(size_t)l + 1] - lstart[(size_t)l];
            if (cnt == 0) continue;
            hipLaunchKernelGGL((k_kd_level<DT>), dim3(cnt, ctiles), dim3(256), 0, s, cnt, dord.p + lstart[(size_t)l], dptr.p, dent.p, F, Y.p, (i64d)ldz, nf);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    const double t_sparse = spasm_wtime();
    // ---- K = Y transposed, compacted
    const int nchunks = std::max(1, cdiv(r, KD_CHUNK));
    DevBuf<i64d> cnt, off;
    DevBuf<int> d_pcp, d_free;
    const size_t ncnt = (size_t)nf * (size_t)nchunks;
    cnt.alloc(ncnt + 1); off.alloc(ncnt + 1); d_pcp.alloc((size_t)r + 1); d_free.alloc((size_t)nf + 1);
    HIPCHK(hipMemsetAsync(cnt.p + ncnt, 0, sizeof(i64d), s));
    if (r > 0) HIPCHK(hipMemcpyAsync(d_pcp.p, pivcol_of_pos.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_free.p, h_free.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL((k_kd_count<DT>), dim3(cdiv(nf, 256), nchunks), dim3(256), 0, s, r, nf, Y.p, (i64d)ldz, cnt.p, nchunks);
    HIPCHK(hipGetLastError());
    Scanner scan;
    scan.exclusive(cnt.p, off.p, ncnt + 1, s);
    std::vector<i64d> h_off(ncnt + 1);
    HIPCHK(hipMemcpyAsync(h_off.data(), off.p, (ncnt + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 ktot = h_off[ncnt];
    DevBuf<int> Kj, Kx;
    Kj.alloc((size_t)ktot + 1); Kx.alloc((size_t)ktot + 1);
    hipLaunchKernelGGL((k_kd_fill<DT>), dim3(cdiv(nf, 256), nchunks), dim3(256), 0, s, r, nf, Y.p, (i64d)ldz, off.p, nchunks, d_pcp.p, d_free.p, Kj.p, Kx.p);
    HIPCHK(hipGetLastError());
    struct spasm_csr *K = spasm_csr_alloc(nf, m, std::max<i64>(ktot, 1), prime, true);
    if (!K) throw EngineError("out of host memory");
    for (int i = 0; i <= nf; i++) K->p[i] = i < nf ? h_off[(size_t)i * (size_t)nchunks] : ktot;
    if (ktot > 0) {
        HIPCHK(hipMemcpyAsync(K->j, Kj.p, (size_t)ktot * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(K->x, Kx.p, (size_t)ktot * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    spasm_logf("[kernel] pivot order and free columns %.2fs; dense tail of %d rows: to the device %.2fs, reduced form %.2fs; %d sparse rows in %d levels %.2fs; K %.2fs\n",
               t_prep - t_start, rd, t_dense_rows - t_prep, t_z - t_dense_rows, t0, nlev, t_sparse - t_z, spasm_wtime() - t_sparse);
    spasm_logf("[kernel] done in %.1fs. NNZ(K) = %lld\n", spasm_wtime() - t_start, (long long)spasm_nnz(K));
    return K;
}

struct spasm_csr *do_kernel(const struct spasm_lu *fact, int first = 0, int step = 1)
{
    require_device();
    if (!fact || !fact->U || !fact->qinv) throw EngineError("spasm_kernel: incomplete factorization (U / qinv missing)");
    const struct spasm_csr *U = fact->U;
    check_input(U, "spasm_kernel");
    if (first < 0 || step < 1) throw EngineError("spasm_amd_kernel_strided: bad (first, step)");
    // a U too large for the device as one round goes through its closure (SPASM_AMD_KERNEL_REDUCE_NNZ, tests: the size from which)
    i64 reduce_at = (i64)1 << 31;
    if (const char *e = getenv("SPASM_AMD_KERNEL_REDUCE_NNZ")) reduce_at = atoll(e);
    // all free columns at once through a dense right-hand side (kernel_dense.hpp): primes below 2^16; SPASM_AMD_KERNEL_DENSE_RHS = 1
    // always (tests), 0 never; SPASM_AMD_KERNEL_DENSE_TAIL (tests): rows of the dense tail instead of the choice by density
    {
        const ZpField F = zp_field_make(U->field->p);
        const char *e = getenv("SPASM_AMD_KERNEL_DENSE_RHS");
        // (by default from 2^26 entries of U on: config 5 at 1/5, 2e9 entries, takes 1.3 s this way and 2.3 s with one sparse solve
        // per free column; below that the difference is noise and the sparse solves also serve the large primes)
        const bool want = e ? atoi(e) != 0 : spasm_nnz(U) >= std::min<i64>(reduce_at, (i64)1 << 26);
        if (want && F.small && dense_elem_bytes(F, 1) <= 2) {
            i64 tail = -1;
            if (const char *t = getenv("SPASM_AMD_KERNEL_DENSE_TAIL")) tail = atoll(t);
            struct spasm_csr *K = dense_elem_bytes(F, 1) == 1 ? kernel_dense_rhs<signed char>(U, fact->qinv, first, step, tail)
                                                              : kernel_dense_rhs<short>(U, fact->qinv, first, step, tail);
            if (K) return K;
            spasm_logf("[kernel] the dense right-hand side does not fit the device: one sparse solve per free column\n");
        }
    }
    if (spasm_nnz(U) >= reduce_at) {
        const double t0 = spasm_wtime();
        KernelReduced red;
        kernel_closure(U, fact->qinv, first, step, red);
        spasm_logf("[kernel] closure found in %.2fs\n", spasm_wtime() - t0);
        return do_kernel_core(red.U2, red.qinv2.data(), first, step);
    }
    return do_kernel_core(U, fact->qinv, first, step);
}

// qinv[j] = row of U with its pivot on column j, -1: free column, -2: a pivot column of a row that is not part of U (kernel_closure)
struct spasm_csr *do_kernel_core(const struct spasm_csr *U, const int *qinv, int first, int step)
{
    const int r = U->n, m = U->m;
    const i64 prime = U->field->p;
    const double t0 = spasm_wtime();
    spasm_logf("[kernel] start. U is %d x %d (%lld nnz). Transposing U\n", r, m, (long long)spasm_nnz(U));

    // pivot column of each row, unit pivots checked (reference src/SpaSM.jl:712), topological numbering
    std::vector<int> pc;
    const std::vector<int> perm = pivot_topological_order(U, qinv, "spasm_kernel", pc);
    const double t_order = spasm_wtime();
    std::vector<int> idx_of((size_t)std::max(r, 1));
    for (int t = 0; t < r; t++) idx_of[(size_t)perm[(size_t)t]] = t;

    // Transposed triangular system (what libspasm solves per free column, README.md:39 "Transposing U"):
    // unknowns y_a = k[pivcol(a)], equations y_a + sum_{b != a} U[a][pivcol(b)] y_b = U[a][j].  Numbering the
    // pivots in REVERSE topological order (ridx) makes the system strictly upper triangular for the solve kernels:
    // "pivot row" ridx(b) = column pivcol(b) of U, "right-hand side" of free column j = column j of U.
    std::vector<int> h_lab((size_t)std::max(r, 1)), h_rowsrc((size_t)std::max(r, 1)), h_free;
    for (int a = 0; a < r; a++) h_lab[(size_t)a] = r - 1 - idx_of[(size_t)a];
    for (int t = 0; t < r; t++) h_rowsrc[(size_t)(r - 1 - t)] = pc[(size_t)perm[(size_t)t]]; // column of pivot ridx
    {
        int f = 0;
        for (int j = 0; j < m; j++)
            if (qinv[j] < 0 && qinv[j] != -2) {
                if (f >= first && (f - first) % step == 0) h_free.push_back(j);
                f++;
            }
    }
    const int nfree = (int)h_free.size();

    hipStream_t s = nullptr;
    DevMat PM;
    upload_csr(U, 0, r, PM, s);
    HIPCHK(hipStreamSynchronize(s));
    const double t_upload = spasm_wtime();
    std::unique_ptr<Round> R(new Round());
    R->F = zp_field_make(prime);
    R->stream = s;
    DevBuf<int> lab, rowsrc, freecol;
    lab.alloc((size_t)r + 1);
    rowsrc.alloc((size_t)r + 1);
    freecol.alloc((size_t)nfree + 1);
    if (r > 0) {
        HIPCHK(hipMemcpyAsync(lab.p, h_lab.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(rowsrc.p, h_rowsrc.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (nfree > 0) HIPCHK(hipMemcpyAsync(freecol.p, h_free.data(), (size_t)nfree * sizeof(int), hipMemcpyHostToDevice, s));
    // Ut: row j = column j of U with entries labelled ridx(a)
    TransposeOut Ut;
    device_transpose(PM, r, nullptr, lab.p, 0, R->scan, s, Ut);
    HIPCHK(hipStreamSynchronize(s));
    const double t_transpose = spasm_wtime();
    DevMat T;
    T.n = m;
    T.m = r;
    T.start.alloc((size_t)m + 1);
    T.len.alloc((size_t)m + 1);
    T.lead.alloc(1);
    T.orig.alloc((size_t)m + 1);
    T.ent = std::move(Ut.Tent);
    if (m > 0) {
        hipLaunchKernelGGL(k_rows_from_ptr, dim3(cdiv(m, 256)), dim3(256), 0, s, m, Ut.Tp.p, T.start.p, T.len.p, T.orig.p);
        HIPCHK(hipGetLastError());
    }
    // the solve structures over the ridx space: every "column" 0..r-1 carries a pivot
    R->m = r;
    R->npiv = r;
    R->qinv_r.alloc((size_t)r + 1);
    R->pivcol.alloc((size_t)r + 1);
    if (r > 0) {
        hipLaunchKernelGGL(k_iota, dim3(cdiv(r, 256)), dim3(256), 0, s, r, R->qinv_r.p);
        hipLaunchKernelGGL(k_iota, dim3(cdiv(r, 256)), dim3(256), 0, s, r, R->pivcol.p);
        HIPCHK(hipGetLastError());
    }
    R->want_idx = true; // the kernel vectors are assembled from (pivot index, multiplier)
    HIPCHK(hipStreamSynchronize(s));
    const double t_rows = spasm_wtime();
    R->build_U(T, rowsrc.p);
    HIPCHK(hipStreamSynchronize(s));
    const double t_buildu = spasm_wtime();
    R->prepare_uinv(nfree);
    // (the record pool: a guess that grows when a solve overflows it.  4 nnz(U) was the guess -- 160 GB of pool for the U of config 5
    // at 1/5, 3.4 of the step's 4.5 s spent allocating it for kernel vectors of one or two entries)
    R->solve_phase(T, freecol.p, nullptr, nfree, std::min<i64>(4 * spasm_nnz(U), std::max<i64>((i64)1 << 24, 1024 * (i64)nfree)));
    HIPCHK(hipStreamSynchronize(s));
    const double t_solve = spasm_wtime();
    // assemble K: row f = {(free column, -1)} U {(column of pivot ridx, y_ridx)}
    DevBuf<i64d> klen, kstart;
    klen.alloc((size_t)nfree + 1);
    kstart.alloc((size_t)nfree + 1);
    hipLaunchKernelGGL(k_kcount, dim3(cdiv(((i64)nfree + 1) * 64, 256)), dim3(256), 0, s, nfree, R->Lstart.p, R->Llen.p, R->Lpool.p, klen.p);
    HIPCHK(hipGetLastError());
    R->scan.exclusive(klen.p, kstart.p, (size_t)nfree + 1, s);
    i64d ktot = 0;
    HIPCHK(hipMemcpyAsync(&ktot, kstart.p + nfree, sizeof ktot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    DevBuf<int2> Kent;
    Kent.alloc((size_t)ktot + 1);
    if (nfree > 0) {
        hipLaunchKernelGGL(k_kfill, dim3(cdiv((i64)nfree * 64, 256)), dim3(256), 0, s, nfree, freecol.p, rowsrc.p, R->Lstart.p, R->Llen.p, R->Lpool.p, R->Lidx.p,
                           kstart.p, Kent.p);
        HIPCHK(hipGetLastError());
    }
    struct spasm_csr *K = spasm_csr_alloc(nfree, m, ktot, prime, true);
    if (!K) throw EngineError("out of host memory");
    {
        std::vector<int2> ent((size_t)ktot);
        HIPCHK(hipMemcpyAsync(K->p, kstart.p, ((size_t)nfree + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
        if (ktot > 0) HIPCHK(hipMemcpyAsync(ent.data(), Kent.p, (size_t)ktot * sizeof(int2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (i64 q = 0; q < ktot; q++) { K->j[q] = ent[(size_t)q].x; K->x[q] = ent[(size_t)q].y; }
    }
    spasm_logf("[kernel] pivot order %.2fs, U to the device %.2fs, transpose %.2fs, rows of the transposed system %.2fs, its U %.2fs, solves %.2fs, K %.2fs\n", t_order - t0,
               t_upload - t_order, t_transpose - t_upload, t_rows - t_transpose, t_buildu - t_rows, t_solve - t_buildu, spasm_wtime() - t_solve);
    spasm_logf("[kernel] done in %.1fs. NNZ(K) = %lld\n", spasm_wtime() - t0, (long long)spasm_nnz(K));
    return K;
}

} // namespace

// ------------------------------------------------------------------------------------------------
// device-resident plan for ONE Schur round (bench / multi-GPU shard)
// ------------------------------------------------------------------------------------------------
struct spasm_amd_schur_plan {
    DevMat A;
    DevMat PM;          // sharded runs: the imported pivot rows
    DevBuf<int> rowsrc; // sharded runs: pivot index -> row of PM
    Round R;
    int lo = 0, hi = 0, stride = 1;  // the plan's rows: lo, lo + stride, ... < hi (global row ids)
    i64 nnz_in = 0;
    i64 prime = 0;
    bool ran = false;
    // the reference's trip counters of this round, counted once on the multiplier lists when the plan is made (the runs go
    // along the rows of W, where no list exists to count)
    u64d exact_applications = 0, exact_nnz_reduced = 0, exact_segments = 0;
};

namespace {

} // namespace

struct spasm_amd_shard {
    spasm_amd_schur_plan *plan = nullptr; // owns the shard's rows and the round; handed to the caller by shard_import
    int n_total = 0;
    int npiv = 0, nown = 0;
    i64 nnz_own = 0;
    DevBuf<int> oflag, oscan;
    DevBuf<int2> ohdr;
    DevBuf<i64d> olen, ooff;
    bool imported = false;
};

namespace {

// what a plan's round needs beside U: W when the round can go along it (rebuilt by every run: it is part of the Schur step),
// else Uinv for the multiplier lists
void plan_prepare(spasm_amd_schur_plan *P)
{
    Round &R = P->R;
    R.want_w_row_stats = true;
    R.prepare_w((i64)1 << 62, P->nnz_in);
    if (R.use_w) { R.use_uinv = false; R.ms_uinv = 0; }
    else R.prepare_uinv();
}

// dry run of the solve on the multiplier lists: sizes the record pool and the Schur slots (the bounds along W are no larger)
// and counts the reference's trip counters once
void plan_dry_run(spasm_amd_schur_plan *P, i64 pool_guess)
{
    Round &R = P->R;
    const bool fl = R.force_lists;
    R.force_lists = true;
    const i64 tot = R.solve_phase(P->A, R.np_rows.p, nullptr, R.nnp, pool_guess);
    const RoundCounters c = R.read_counters();
    P->exact_applications = c.applications;
    P->exact_nnz_reduced = c.nnz_reduced;
    P->exact_segments = c.segments;
    R.force_lists = fl;
    i64 tot2 = 0;
    // along W a row's stream is the sum of the runs of its entries on pivot columns: two runs that share pivot rows count them
    // twice, so these bounds can exceed the lists' -- size for both
    if (R.use_w && !fl) {
        tot2 = R.solve_phase(P->A, R.np_rows.p, nullptr, R.nnp, pool_guess);
        const RoundCounters c2 = R.read_counters(); // the plan runs exactly this again: the same rows take the same classes
        R.quiet_fallbacks = c2.combine_overflow == 0 && c2.solve_overflow == 0 && c2.solve_failed == 0;
        R.quiet_rejects = c2.wplan_reject == 0;
        R.quiet_known = true;
    }
    R.S.ent.ensure((size_t)std::max(tot, tot2) + 1);
}

spasm_amd_shard *shard_create(const struct spasm_csr *A, int lo, int hi, int stride = 1)
{
    require_device();
    check_input(A, "spasm_amd_shard_create");
    if (lo < 0 || hi > A->n || lo > hi || stride < 1) throw EngineError("spasm_amd_shard_create: bad row range");
    std::unique_ptr<spasm_amd_shard> S(new spasm_amd_shard());
    std::unique_ptr<spasm_amd_schur_plan> P(new spasm_amd_schur_plan());
    P->lo = lo;
    P->hi = hi;
    P->stride = stride;
    P->prime = A->field->p;
    P->nnz_in = 0;
    for (int g = lo; g < hi; g += stride) P->nnz_in += A->p[g + 1] - A->p[g];
    hipStream_t s = nullptr;
    upload_csr_strided(A, lo, hi, stride, P->A, s); // only this shard's rows; orig = global row ids
    P->R.F = zp_field_make(P->prime);
    P->R.stream = s;
    S->n_total = A->n;
    S->plan = P.release();
    return S.release();
}

void shard_elect(spasm_amd_shard *S, int64_t *keys_dev)
{
    Round &R = S->plan->R;
    R.elect_local(S->plan->A, S->plan->lo, S->plan->stride);
    HIPCHK(hipMemcpyAsync(keys_dev, R.best.p, (size_t)S->plan->A.m * sizeof(u64d), hipMemcpyDeviceToDevice, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
}

// the reduced election keys -> the leftmost pivots, numbered (the same on every shard); returns how many
int shard_assign(spasm_amd_shard *S, const int64_t *keys_dev)
{
    spasm_amd_schur_plan *P = S->plan;
    Round &R = P->R;
    const int m = P->A.m;
    R.m = m;
    R.best.ensure((size_t)m + 1);
    HIPCHK(hipMemcpyAsync(R.best.p, keys_dev, (size_t)m * sizeof(u64d), hipMemcpyDeviceToDevice, R.stream));
    R.assign_pivots();
    R.n_leftmost = R.npiv;
    R.n_open = 0;
    return R.npiv;
}

// "FL on columns" over row shards (Round::open_*): one step of the search on this shard's rows.  `in_dev`: the array the step before
// left, REDUCED over the shards by the caller (copied in first); `out_dev` receives the array this step leaves, m elements, for the
// caller to reduce: BEGIN -> closed (int32, MAX); HIST (in: closed) -> colcnt (int32, SUM); PROPOSE (in: colcnt) -> best2 (int64,
// MIN); ACCEPT (in: best2) -> newflag (int32, MAX); RECORD (in: newflag) -> closed (int32, MAX), returns the pivots the pass
// accepted (0: the search is over, nothing written); FINISH renumbers and returns the pivots the search added.
enum { OPEN_BEGIN = 0, OPEN_HIST = 1, OPEN_PROPOSE = 2, OPEN_ACCEPT = 3, OPEN_RECORD = 4, OPEN_FINISH = 5 };
int shard_open_step(spasm_amd_shard *S, int step, int pass, const void *in_dev, void *out_dev)
{
    spasm_amd_schur_plan *P = S->plan;
    Round &R = P->R;
    hipStream_t s = R.stream;
    const size_t m = (size_t)P->A.m;
    int ret = 0;
    auto take = [&](void *dst, size_t elem) { if (in_dev) HIPCHK(hipMemcpyAsync(dst, in_dev, m * elem, hipMemcpyDeviceToDevice, s)); };
    auto give = [&](const void *src, size_t elem) { if (out_dev) HIPCHK(hipMemcpyAsync(out_dev, src, m * elem, hipMemcpyDeviceToDevice, s)); };
    switch (step) {
    case OPEN_BEGIN:
        R.open_begin(P->A, P->lo, P->stride);
        give(R.closed.p, sizeof(int));
        break;
    case OPEN_HIST:
        take(R.closed.p, sizeof(int));
        R.open_hist(P->A);
        give(R.colcnt.p, sizeof(int));
        break;
    case OPEN_PROPOSE:
        take(R.colcnt.p, sizeof(int));
        R.open_propose(P->A, P->lo, P->stride);
        give(R.best2.p, sizeof(u64d));
        break;
    case OPEN_ACCEPT:
        take(R.best2.p, sizeof(u64d));
        R.open_accept(P->A, P->lo, P->stride);
        give(R.newflag.p, sizeof(int));
        break;
    case OPEN_RECORD:
        take(R.newflag.p, sizeof(int));
        ret = R.open_record(P->A, pass, P->lo, P->stride);
        if (ret > 0) give(R.closed.p, sizeof(int));
        break;
    case OPEN_FINISH:
        ret = R.open_finish();
        break;
    default:
        throw EngineError("spasm_amd_shard_open_step: unknown step");
    }
    HIPCHK(hipStreamSynchronize(s));
    return ret;
}

// the pivots are final: this shard's non-pivot rows, the pivot rows it owns (what shard_export sends); returns npiv
int shard_finish_keys(spasm_amd_shard *S, int *n_owned, i64 *nnz_owned);

int shard_set_keys(spasm_amd_shard *S, const int64_t *keys_dev, int *n_owned, i64 *nnz_owned)
{
    shard_assign(S, keys_dev);
    return shard_finish_keys(S, n_owned, nnz_owned);
}

int shard_finish_keys(spasm_amd_shard *S, int *n_owned, i64 *nnz_owned)
{
    spasm_amd_schur_plan *P = S->plan;
    Round &R = P->R;
    hipStream_t s = R.stream;
    R.mark_local(P->A, P->lo, 0, INT_MAX, P->stride, 1); // local non-pivot rows; pivrow holds global ids
    S->npiv = R.npiv;
    // owned pivot rows, in ascending pivot index
    const int np = R.npiv;
    S->oflag.alloc((size_t)np + 1);
    S->oscan.alloc((size_t)np + 1);
    hipLaunchKernelGGL(k_owned_flags, dim3(cdiv((i64)np + 1, 256)), dim3(256), 0, s, np, P->lo, P->stride, P->A.n, R.pivrow.p, S->oflag.p);
    HIPCHK(hipGetLastError());
    R.scan.exclusive(S->oflag.p, S->oscan.p, (size_t)np + 1, s);
    HIPCHK(hipMemcpyAsync(&S->nown, S->oscan.p + np, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    S->ohdr.alloc((size_t)S->nown + 1);
    S->olen.alloc((size_t)S->nown + 1);
    S->ooff.alloc((size_t)S->nown + 1);
    HIPCHK(hipMemsetAsync(S->olen.p + S->nown, 0, sizeof(i64d), s));
    if (np > 0) {
        hipLaunchKernelGGL(k_export_hdr, dim3(cdiv(np, 256)), dim3(256), 0, s, np, P->lo, P->stride, S->oflag.p, S->oscan.p, R.pivrow.p, P->A.len.p, S->ohdr.p, S->olen.p);
        HIPCHK(hipGetLastError());
    }
    R.scan.exclusive(S->olen.p, S->ooff.p, (size_t)S->nown + 1, s);
    i64d tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, S->ooff.p + S->nown, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    S->nnz_own = tot;
    if (n_owned) *n_owned = S->nown;
    if (nnz_owned) *nnz_owned = tot;
    return np;
}

void shard_export(spasm_amd_shard *S, int *hdr_dev, int *ent_dev)
{
    spasm_amd_schur_plan *P = S->plan;
    Round &R = P->R;
    hipStream_t s = R.stream;
    if (S->nown > 0) {
        HIPCHK(hipMemcpyAsync(hdr_dev, S->ohdr.p, (size_t)S->nown * sizeof(int2), hipMemcpyDeviceToDevice, s));
        constexpr int TEAM = 16;
        hipLaunchKernelGGL((k_export_rows<TEAM>), dim3(cdiv((i64)S->nown * TEAM, 256)), dim3(256), 0, s, S->nown, P->lo, P->stride, S->ohdr.p, S->ooff.p, R.pivrow.p,
                           P->A.start.p, P->A.ent.p, (int2 *)ent_dev);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
}

// what a sharded round needs after its U: W / Uinv and the dry run that sizes the pools (the second half of shard_import)
void shard_import_finish(spasm_amd_schur_plan *P)
{
    Round &R = P->R;
    plan_prepare(P);
    HIPCHK(hipEventRecord(R.ev[1], R.stream));
    plan_dry_run(P, 4 * std::max<i64>(P->nnz_in, 1 << 14));
}

// prepare = false: stop after U (the caller decides first whether the round's Schur complement goes dense; shard_import_finish otherwise)
spasm_amd_schur_plan *shard_import(spasm_amd_shard *S, int n_rows, i64 n_entries, const int *hdr_dev, const int *ent_dev, bool prepare = true)
{
    spasm_amd_schur_plan *P = S->plan;
    if (!P) throw EngineError("spasm_amd_shard_import: already imported");
    Round &R = P->R;
    hipStream_t s = R.stream;
    if (n_rows != R.npiv) throw EngineError("spasm_amd_shard_import: the parts do not add up to the elected pivots");
    DevMat &PM = P->PM;
    PM.n = n_rows;
    PM.m = P->A.m;
    PM.start.alloc((size_t)n_rows + 1);
    PM.len.alloc((size_t)n_rows + 1);
    PM.lead.alloc(1);
    PM.orig.alloc((size_t)n_rows + 1);
    PM.ent.alloc((size_t)n_entries + 1);
    P->rowsrc.alloc((size_t)n_rows + 1);
    DevBuf<i64d> l64, off;
    l64.alloc((size_t)n_rows + 1);
    off.alloc((size_t)n_rows + 1);
    hipLaunchKernelGGL(k_hdr_len64, dim3(cdiv((i64)n_rows + 1, 256)), dim3(256), 0, s, n_rows, (const int2 *)hdr_dev, l64.p);
    HIPCHK(hipGetLastError());
    R.scan.exclusive(l64.p, off.p, (size_t)n_rows + 1, s);
    i64d tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, off.p + n_rows, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (tot != n_entries) throw EngineError("spasm_amd_shard_import: header lengths do not match the entry count");
    if (n_rows > 0) {
        hipLaunchKernelGGL(k_import_rows, dim3(cdiv(n_rows, 256)), dim3(256), 0, s, n_rows, (const int2 *)hdr_dev, off.p, PM.start.p, PM.len.p, PM.orig.p, P->rowsrc.p);
        HIPCHK(hipGetLastError());
    }
    if (n_entries > 0) HIPCHK(hipMemcpyAsync(PM.ent.p, ent_dev, (size_t)n_entries * sizeof(int2), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipEventRecord(R.ev[0], s));
    R.build_U(PM, P->rowsrc.p);
    if (prepare) shard_import_finish(P);
    S->plan = nullptr; // ownership passes to the caller
    S->imported = true;
    return P;
}

void plan_run(spasm_amd_schur_plan *P, hipStream_t s);

// The round of a sharded plan becomes history: its Schur rows become the shard's matrix of the next round, on the device and
// under the same local numbering (local row i = original row lo + i * stride).  Consumes the plan.
spasm_amd_shard *plan_advance(spasm_amd_schur_plan *P, int *rows_out, i64 *nnz_out)
{
    if (!P) throw EngineError("spasm_amd_schur_plan_advance: null plan");
    if (!P->ran) plan_run(P, P->R.stream);
    Round &R = P->R;
    hipStream_t s = R.stream;
    R.fetch_counters(); // synchronises; throws on an exhausted pool / table
    const int n = P->A.n, nnp = R.nnp;
    std::unique_ptr<spasm_amd_shard> S2(new spasm_amd_shard());
    std::unique_ptr<spasm_amd_schur_plan> P2(new spasm_amd_schur_plan());
    P2->lo = P->lo;
    P2->hi = P->hi;
    P2->stride = P->stride;
    P2->prime = P->prime;
    P2->nnz_in = (i64)R.hctr.nnz_out;
    DevMat &A2 = P2->A;
    A2.n = n;
    A2.m = P->A.m;
    A2.start.alloc((size_t)n + 1);
    A2.len.alloc((size_t)n + 1);
    A2.lead.alloc((size_t)n + 1);
    A2.orig.alloc((size_t)n + 1);
    if (n > 0) {
        hipLaunchKernelGGL(k_advance_init, dim3(cdiv(n, 256)), dim3(256), 0, s, n, P->lo, P->stride, A2.start.p, A2.len.p, A2.lead.p, A2.orig.p);
        HIPCHK(hipGetLastError());
    }
    if (nnp > 0) {
        hipLaunchKernelGGL(k_advance_rows, dim3(cdiv(nnp, 256)), dim3(256), 0, s, nnp, n, P->lo, P->stride, R.S.start.p, R.S.len.p, R.S.lead.p,
                           R.S.orig.p, A2.start.p, A2.len.p, A2.lead.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    A2.ent = std::move(R.S.ent);
    P2->R.F = zp_field_make(P2->prime);
    P2->R.stream = s;
    S2->n_total = P->hi;
    if (rows_out) *rows_out = R.hctr.nonempty_out;
    if (nnz_out) *nnz_out = (i64)R.hctr.nnz_out;
    S2->plan = P2.release();
    delete P;
    return S2.release();
}

// the shard's rows as a host CSR with one row per LOCAL row (empty rows included; local row i = original row lo + i * stride)
struct spasm_csr *shard_fetch(spasm_amd_shard *S)
{
    if (!S || !S->plan) throw EngineError("spasm_amd_shard_fetch: the shard has no matrix (already imported?)");
    spasm_amd_schur_plan *P = S->plan;
    Round &R = P->R;
    hipStream_t s = R.stream;
    const int n = P->A.n;
    DevBuf<i64d> len64, ostart;
    len64.alloc((size_t)n + 1);
    ostart.alloc((size_t)n + 1);
    hipLaunchKernelGGL(k_copy_len64, dim3(cdiv((i64)n + 1, 256)), dim3(256), 0, s, n, P->A.len.p, len64.p);
    HIPCHK(hipGetLastError());
    R.scan.exclusive(len64.p, ostart.p, (size_t)n + 1, s);
    std::vector<i64d> hp((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(hp.data(), ostart.p, ((size_t)n + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64 tot = hp[(size_t)n];
    struct spasm_csr *out = spasm_csr_alloc(n, P->A.m, tot, P->prime, true);
    if (!out) throw EngineError("out of host memory for the shard's rows");
    for (int i = 0; i <= n; i++) out->p[i] = hp[(size_t)i];
    if (tot > 0) {
        DevBuf<int> oj, ox;
        oj.alloc((size_t)tot);
        ox.alloc((size_t)tot);
        constexpr int TEAM = 16;
        hipLaunchKernelGGL((k_compact_rows<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, P->A.start.p, P->A.len.p, P->A.ent.p, ostart.p, oj.p, ox.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out->j, oj.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->x, ox.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return out;
}

spasm_amd_schur_plan *plan_create(const struct spasm_csr *A, int lo, int hi, int stride = 1)
{
    require_device();
    check_input(A, "spasm_amd_schur_plan_create");
    if (lo < 0 || hi > A->n || lo > hi || stride < 1) throw EngineError("spasm_amd_schur_plan_create: bad row range");
    std::unique_ptr<spasm_amd_schur_plan> P(new spasm_amd_schur_plan());
    P->lo = lo;
    P->hi = hi;
    P->stride = stride;
    P->prime = A->field->p;
    P->nnz_in = 0;
    for (int g = lo; g < hi; g += stride) P->nnz_in += A->p[g + 1] - A->p[g];
    hipStream_t s = nullptr;
    // the whole matrix is resident on every device: the election sees all rows, so every shard builds the same U
    upload_csr(A, 0, A->n, P->A, s);
    Round &R = P->R;
    R.F = zp_field_make(P->prime);
    R.stream = s;
    HIPCHK(hipEventRecord(R.ev[0], s));
    R.elect_local(P->A, 0);
    R.assign_pivots();
    R.mark_local(P->A, 0, lo, hi, 1, stride);
    R.build_U(P->A, R.pivrow.p);
    plan_prepare(P.get());
    HIPCHK(hipEventRecord(R.ev[1], s));
    plan_dry_run(P.get(), 4 * spasm_nnz(A));
    return P.release();
}

void plan_run(spasm_amd_schur_plan *P, hipStream_t s)
{
    Round &R = P->R;
    R.stream = s;
    // the whole Schur step of the round (reference spasm_schur, src/SpaSM.jl:761-762: the per-row solve is inside it): W from
    // U, the plan of every row, the scatter.  ev[4] .. ev[1] = the W build.
    HIPCHK(hipEventRecord(R.ev[4], s));
    if (R.use_w) R.build_w_levels();
    else if (R.use_uinv) R.prepare_uinv();
    HIPCHK(hipEventRecord(R.ev[1], s));
    R.run_solve(P->A, R.np_rows.p, nullptr, R.nnp);
    R.run_bounds(R.nnp);
    HIPCHK(hipEventRecord(R.ev[2], s));
    R.run_scatter(P->A, R.np_rows.p, R.nnp);
    HIPCHK(hipEventRecord(R.ev[3], s));
    P->ran = true;
}

// the pivot rows of the plan's round as they enter U: scaled to a unit pivot, in pivot-index order (= ascending pivot column);
// pivcol_out / row_out (npiv ints each, may be NULL): pivot column and originating row (global row number) of each
struct spasm_csr *plan_fetch_U(spasm_amd_schur_plan *P, int *pivcol_out, int *row_out)
{
    Round &R = P->R;
    hipStream_t s = R.stream;
    const int np = R.npiv;
    struct spasm_csr *Uc = spasm_csr_alloc(np, R.m, R.utotal, P->prime, true);
    if (!Uc) throw EngineError("out of host memory for the round's U rows");
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> guard(Uc, spasm_csr_free); // (a HIPCHK below may throw)
    if (np > 0) HIPCHK(hipMemcpyAsync(Uc->p, R.uoff.p, ((size_t)np + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    else Uc->p[0] = 0;
    if (R.utotal > 0) {
        DevBuf<int> dj, dx;
        dj.alloc((size_t)R.utotal);
        dx.alloc((size_t)R.utotal);
        hipLaunchKernelGGL(k_split_ent, dim3((unsigned)std::min<i64>((R.utotal + 255) / 256, 65536)), dim3(256), 0, s, (i64d)R.utotal, R.Ufull.p, dj.p, dx.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(Uc->j, dj.p, (size_t)R.utotal * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(Uc->x, dx.p, (size_t)R.utotal * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (np > 0 && pivcol_out) HIPCHK(hipMemcpyAsync(pivcol_out, R.pivcol.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    if (np > 0 && row_out) HIPCHK(hipMemcpyAsync(row_out, R.pivrow.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return guard.release();
}

struct spasm_csr *plan_fetch(spasm_amd_schur_plan *P, int *p_out)
{
    Round &R = P->R;
    if (!P->ran) throw EngineError("spasm_amd_schur_plan_fetch: run the plan first");
    hipStream_t s = R.stream;
    const int n = R.nnp;
    R.fetch_counters();
    DevBuf<i64d> len64, ostart;
    len64.alloc((size_t)n + 1);
    ostart.alloc((size_t)n + 1);
    hipLaunchKernelGGL(k_copy_len64, dim3(cdiv((i64)n + 1, 256)), dim3(256), 0, s, n, R.S.len.p, len64.p);
    HIPCHK(hipGetLastError());
    R.scan.exclusive(len64.p, ostart.p, (size_t)n + 1, s);
    i64d tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, ostart.p + n, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    DevBuf<int> oj, ox;
    oj.alloc((size_t)tot + 1);
    ox.alloc((size_t)tot + 1);
    if (n > 0) {
        constexpr int TEAM = 16;
        hipLaunchKernelGGL((k_compact_rows<TEAM>), dim3(cdiv((i64)n * TEAM, 256)), dim3(256), 0, s, n, R.S.start.p, R.S.len.p, R.S.ent.p, ostart.p, oj.p, ox.p);
        HIPCHK(hipGetLastError());
    }
    struct spasm_csr *S = spasm_csr_alloc(n, R.m, tot, P->prime, true);
    if (!S) throw EngineError("out of host memory");
    HIPCHK(hipMemcpyAsync(S->p, ostart.p, ((size_t)n + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    if (tot > 0) {
        HIPCHK(hipMemcpyAsync(S->j, oj.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(S->x, ox.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (p_out && n > 0) HIPCHK(hipMemcpyAsync(p_out, R.S.orig.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return S;
}

// ------------------------------------------------------------------------------------------------
// The whole echelonization, row-sharded over the devices of ONE process (spasm_amd_echelonize_multi): what spasm.jl_amd/sharded.py
// does between processes with torch.distributed, here with the shards of one host thread and peer copies over xGMI in place of the
// collectives -- so that a Julia host reaches all GPUs of a node through one ccall.  Shard s keeps rows s, s + nshards, ... on
// device s % (devices): with fewer devices than shards several shards share a device (how the protocol is tested on one GPU).
// Per round: every shard proposes its election keys, device 0 takes the per-column minimum (all-reduce(MIN)), every shard numbers
// the pivots and exports the pivot rows it owns, all shards receive the concatenation (all-gather) and build the same U, the Schur
// rows stay where they are.  Leftmost-entry pivots only in the sharded rounds and in the finish, so the result does not depend on
// the number of shards.  When little is left, or the remainder is dense enough for the dense finish, the rows are gathered and
// the single-device engine finishes them on device 0.
// ------------------------------------------------------------------------------------------------
struct spasm_lu *do_echelonize_multi(const struct spasm_csr *A, struct echelonize_opts *opts, int nshards)
{
    struct echelonize_opts dflt;
    if (!opts) { spasm_echelonize_init_opts(&dflt); opts = &dflt; }
    require_device();
    check_input(A, "spasm_amd_echelonize_multi");
    if (nshards < 1) throw EngineError("spasm_amd_echelonize_multi: at least one shard");
    if (opts->L) throw EngineError("spasm_amd_echelonize_multi: the L factor is only kept by the single-device rounds");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    const int n = A->n, m = A->m;
    const i64 prime = A->field->p;
    const double t0 = spasm_wtime();
    spasm_logf("[echelonize] Start on %d x %d matrix with %lld nnz, %d row shards on %d device(s)\n", n, m, (long long)spasm_nnz(A), nshards, std::min(ndev, nshards));
    DeviceGuard guard;
    auto dev_of = [&](int sh) { return sh % ndev; };
    // the exchange copies device to device: directly over xGMI where the devices can see each other
    for (int a = 0; a < std::min(ndev, nshards); a++) {
        if (hipSetDevice(a) != hipSuccess) continue;
        for (int b = 0; b < std::min(ndev, nshards); b++) {
            int can = 0;
            if (a != b && hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(b, 0);
        }
    }
    (void)hipGetLastError(); // ("already enabled" is not an error of ours)
    struct ShardState {
        spasm_amd_shard *sh = nullptr;
        spasm_amd_schur_plan *plan = nullptr;
        int rows = 0;
        i64 nnz = 0;
        int n_own = 0;
        i64 nnz_own = 0;
        DevBuf<u64d> keys;
        DevBuf<int> hdr, ent, hdr_all, ent_all;
        DevBuf<int> oc_i;   // "FL on columns": the int32 array of the current step
        DevBuf<u64d> oc_q;  // .. and the proposals
    };
    std::vector<std::unique_ptr<ShardState>> st((size_t)nshards);
    auto cleanup = [&]() {
        for (size_t k = 0; k < st.size(); k++) {
            ShardState *q = st[k].get();
            if (!q) continue;
            (void)hipSetDevice(dev_of((int)k));
            if (q->plan) delete q->plan;
            if (q->sh) { delete q->sh->plan; delete q->sh; }
            q->plan = nullptr;
            q->sh = nullptr;
            st[k].reset(); // (its device buffers are released on their device)
        }
    };
    HostU U;
    U.p.push_back(0);
    try {
        for (int k = 0; k < nshards; k++) {
            HIPCHK(hipSetDevice(dev_of(k)));
            st[(size_t)k].reset(new ShardState());
            ShardState &q = *st[(size_t)k];
            q.sh = shard_create(A, k, n, nshards);
            for (int g = k; g < n; g += nshards) { const i64 l = A->p[g + 1] - A->p[g]; q.rows += l > 0; q.nnz += l; }
        }
        DevBuf<u64d> stage; // on device 0: another shard's keys, on their way into the minimum
        int round = 0;
        bool extra_round_done = false;
        i64 last_nnz = -1;
        i64 finish_nnz = (i64)1 << 22;
        if (const char *e = getenv("SPASM_AMD_MULTI_FINISH_NNZ")) finish_nnz = std::max<i64>(atoll(e), 0); // tests: small remainders sharded too
        g_multi_finish = 0;
        // ---- the dense finish over the shards (dense_multi.hpp): primes below 2^16 (the int8 path), as many shards as the election
        // workgroup holds candidates for.  SPASM_AMD_MULTI_GATHER=1 (A/B, tests): the old hand-off, everything to device 0.
        const ZpField F0 = zp_field_make(prime);
        const int elem = F0.p <= 255 ? 1 : 2;
        const char *gather_env = getenv("SPASM_AMD_MULTI_GATHER");
        const bool ddf_ok = opts->enable_dense && F0.small && nshards * DP_W <= 147456 / (DP_W * elem) && nshards <= DM_MAXSHARDS && !(gather_env && atoi(gather_env));
        // .. and remainders worth it: below 16 GiB of dense matrix one device finishes faster than the shards exchange panels
        // (a 44k x 44k remainder over two ranks: 25 s of collectives against 1 s).  SPASM_AMD_MULTI_DENSE_MIN_BYTES (tests): 0.
        double dense_min_bytes = 17179869184.0;
        if (const char *e = getenv("SPASM_AMD_MULTI_DENSE_MIN_BYTES")) dense_min_bytes = atof(e);
        std::vector<int> devs((size_t)nshards);
        for (int k = 0; k < nshards; k++) devs[(size_t)k] = dev_of(k);
        // does a dense matrix of `rows` local rows and `cols` columns fit a shard's device beside what the elimination needs?
        // (no cap by shape here: the shards finish together BECAUSE one device does not hold the remainder -- config 3 / 4 leave
        // 95k x 760k shorts = 144 GB per device of an 8-GPU node; 60 % of the free memory, beside the digit planes and the dense W)
        auto dense_fits = [&](i64 rows, i64 cols) {
            const double bytes = ((double)rows + 2048.0) * (double)((cols + 63) / 64 * 64) * (double)elem;
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
            return bytes <= 0.6 * (double)fr;
        };
        auto run_typed = [&](int C, const std::vector<const int *> &clists, auto &&build) {
            if (elem == 1) return dense_multi_run<signed char>(nshards, devs, F0, C, clists, build, U);
            return dense_multi_run<short>(nshards, devs, F0, C, clists, build, U);
        };
        // The round whose pivots have just been exchanged (every shard holds U): estimate the density of its Schur complement on 64
        // columns (spasm_schur_estimate_density, as the single-device engine does for rounds without W or Uinv); dense -> the Schur
        // complement of every shard's rows goes straight into its dense matrix and the shards eliminate them together.
        auto dense_round = [&]() -> bool {
            const int free_now = m - (int)U.pivcol.size();
            if (free_now <= 0) return false;
            std::vector<std::unique_ptr<DenseW>> dws((size_t)nshards);
            std::vector<int *> flags((size_t)nshards);
            i64 nnp_tot = 0, nnp_max = 0;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                spasm_amd_schur_plan *P = st[(size_t)k]->plan;
                dws[(size_t)k].reset(new DenseW(P->R, P->A, P->R.stream));
                dws[(size_t)k]->flag_columns();
                HIPCHK(hipStreamSynchronize(P->R.stream));
                flags[(size_t)k] = dws[(size_t)k]->cflag.p;
                nnp_tot += P->R.nnp;
                nnp_max = std::max<i64>(nnp_max, P->R.nnp);
            }
            if (nnp_tot <= 64) return false;
            or_flags_across(devs, flags, m);
            int C = 0;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                C = dws[(size_t)k]->finish_columns();
            }
            if (C == 0 || !dense_fits(nnp_max, C)) return false;
            HIPCHK(hipSetDevice(dev_of(0)));
            Round &R0 = st[0]->plan->R;
            const double est = dws[0]->estimate_density(R0.np_rows.p, R0.nnp, free_now);
            spasm_logf("Schur complement is %lld x %d, estimated density : %.2f (64 columns sampled on shard 0, %d levels)\n", (long long)nnp_tot, free_now, est, dws[0]->depth);
            if (!(est > opts->sparsity_threshold)) return false;
            spasm_logf("[echelonize] finishing; density = %.3f (estimated); aspect ratio = %.1f; Schur complement straight to dense on %d shards\n", est,
                       (double)nnp_tot / (double)free_now, nshards);
            std::vector<const int *> clists((size_t)nshards);
            for (int k = 0; k < nshards; k++) clists[(size_t)k] = dws[(size_t)k]->clist.p;
            run_typed(C, clists, [&](int k, int extra, auto &D, DevBuf<int> &row_orig, int &Rk) {
                spasm_amd_schur_plan *P = st[(size_t)k]->plan;
                Rk = P->R.nnp;
                schur_dense_build(P->R, P->A, Rk, *dws[(size_t)k], extra, D, row_orig, P->R.stream);
            });
            return true;
        };
        // the remaining rows are dense already: every shard's live rows as a dense matrix, eliminated together
        auto dense_now = [&]() -> bool {
            std::vector<std::unique_ptr<DenseFill>> fl((size_t)nshards);
            std::vector<int *> flags((size_t)nshards);
            i64 rmax = 0;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                spasm_amd_schur_plan *P = st[(size_t)k]->sh->plan;
                fl[(size_t)k].reset(new DenseFill(P->A, P->R.stream));
                fl[(size_t)k]->flag_columns();
                flags[(size_t)k] = fl[(size_t)k]->cflag.p;
                rmax = std::max<i64>(rmax, fl[(size_t)k]->R);
            }
            or_flags_across(devs, flags, m);
            int C = 0;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                C = fl[(size_t)k]->finish_columns();
            }
            if (C == 0 || !dense_fits(rmax, C)) return false;
            std::vector<const int *> clists((size_t)nshards);
            for (int k = 0; k < nshards; k++) clists[(size_t)k] = fl[(size_t)k]->clist.p;
            run_typed(C, clists, [&](int k, int extra, auto &D, DevBuf<int> &row_orig, int &Rk) {
                Rk = fl[(size_t)k]->R;
                fl[(size_t)k]->build(extra, D, row_orig);
            });
            return true;
        };
        for (;;) {
            i64 rows_left = 0, nnz_left = 0;
            for (auto &q : st) { rows_left += q->rows; nnz_left += q->nnz; }
            if (nnz_left == 0) break;
            const i64 free_cols = (i64)m - (i64)U.pivcol.size();
            const double cells = (double)rows_left * (double)std::max<i64>(free_cols, 1);
            bool dense_enough = opts->enable_dense && (double)nnz_left > opts->sparsity_threshold * cells;
            // (one round ahead as well: when the fill keeps growing at the rate of the last round the next Schur complement would
            // be dense -- it is then never built sparse; the single-device density estimate plays this role there)
            // (with the distributed finish the estimate after the election decides instead: dense_round)
            const bool ddf_now = ddf_ok && cells * (double)elem >= dense_min_bytes;
            if (!ddf_now && last_nnz > 0 && nnz_left > last_nnz)
                dense_enough = dense_enough || (opts->enable_dense && (double)nnz_left * ((double)nnz_left / (double)last_nnz) > opts->sparsity_threshold * cells);
            if (ddf_now && dense_enough && nnz_left > finish_nnz) {
                spasm_logf("[echelonize] finishing; density = %.3f; aspect ratio = %.1f; dense finish on %d shards\n", (double)nnz_left / cells,
                           free_cols > 0 ? (double)rows_left / (double)free_cols : 0.0, nshards);
                if (dense_now()) { g_multi_finish = 2; break; }
            }
            // max_round sparse rounds are over and the remainder is still sparse: the single-device engine would elect once more and
            // estimate the density of that Schur complement before choosing its finish -- so do the shards, once
            const bool spent = round >= opts->max_round;
            const bool one_more = ddf_now && spent && !extra_round_done && !dense_enough && nnz_left > finish_nnz;
            if (one_more) extra_round_done = true;
            if (!one_more && (nnz_left <= finish_nnz || spent || dense_enough)) {
                // ---- hand-off: the remaining rows, under their original numbers, to the single-device engine on device 0
                std::vector<struct spasm_csr *> parts((size_t)nshards, nullptr);
                struct spasm_csr *rest = nullptr;
                struct spasm_lu *fact = nullptr;
                try {
                    i64 tot = 0;
                    for (int k = 0; k < nshards; k++) {
                        HIPCHK(hipSetDevice(dev_of(k)));
                        parts[(size_t)k] = shard_fetch(st[(size_t)k]->sh); // one row per local row: local row i = original row k + i * nshards
                        tot += parts[(size_t)k]->p[parts[(size_t)k]->n];
                    }
                    rest = spasm_csr_alloc(n, m, tot, prime, true);
                    if (!rest) throw EngineError("out of host memory for the remaining rows");
                    i64 w = 0;
                    for (int g = 0; g < n; g++) {
                        const struct spasm_csr *P = parts[(size_t)(g % nshards)];
                        const int i = g / nshards;
                        rest->p[g] = w;
                        const i64 lo = P->p[i], len = P->p[i + 1] - lo;
                        if (len > 0) {
                            memcpy(rest->j + w, P->j + lo, sizeof(int) * (size_t)len);
                            memcpy(rest->x + w, P->x + lo, sizeof(int) * (size_t)len);
                        }
                        w += len;
                    }
                    rest->p[n] = w;
                    for (auto &pp : parts) { spasm_csr_free(pp); pp = nullptr; }
                    HIPCHK(hipSetDevice(dev_of(0)));
                    struct echelonize_opts fo = *opts;
                    fo.enable_greedy_pivot_search = false;
                    fact = do_echelonize(rest, &fo);
                    const int fr = fact->r;
                    std::vector<int> colof((size_t)std::max(fr, 1), -1);
                    for (int j = 0; j < m; j++) if (fact->qinv[j] >= 0) colof[(size_t)fact->qinv[j]] = j;
                    const i64 base = U.p.back();
                    for (int k = 0; k < fr; k++) {
                        U.p.push_back(base + fact->U->p[k + 1]);
                        U.pivcol.push_back(colof[(size_t)k]);
                        U.orig.push_back(fact->p[k]);
                    }
                    const i64 uz = fact->U->p[fr];
                    if (uz > 0) {
                        memcpy(U.j.grow((size_t)uz), fact->U->j, sizeof(int) * (size_t)uz);
                        memcpy(U.x.grow((size_t)uz), fact->U->x, sizeof(int) * (size_t)uz);
                    }
                    spasm_lu_free(fact);
                    spasm_csr_free(rest);
                } catch (...) {
                    for (auto pp : parts) if (pp) spasm_csr_free(pp);
                    if (rest) spasm_csr_free(rest);
                    if (fact) spasm_lu_free(fact);
                    throw;
                }
                break;
            }
            // ---- election: keys of every shard, minimum on device 0, back to every shard
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                st[(size_t)k]->keys.ensure((size_t)m + 1);
                shard_elect(st[(size_t)k]->sh, (int64_t *)st[(size_t)k]->keys.p);
            }
            HIPCHK(hipSetDevice(dev_of(0)));
            stage.ensure((size_t)m + 1);
            for (int k = 1; k < nshards; k++) {
                HIPCHK(hipMemcpy(stage.p, st[(size_t)k]->keys.p, (size_t)m * sizeof(u64d), hipMemcpyDeviceToDevice));
                hipLaunchKernelGGL(k_min_u64, dim3(cdiv(m, 256)), dim3(256), 0, nullptr, (i64d)m, st[0]->keys.p, stage.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipDeviceSynchronize());
            }
            int npiv = 0, n_open = 0;
            i64 tot_rows = 0, tot_ent = 0;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                if (k > 0) HIPCHK(hipMemcpy(st[(size_t)k]->keys.p, st[0]->keys.p, (size_t)m * sizeof(u64d), hipMemcpyDeviceToDevice));
                npiv = shard_assign(st[(size_t)k]->sh, (const int64_t *)st[(size_t)k]->keys.p);
            }
            // "Faugere-Lachartre on columns" over the shards (enable_greedy_pivot_search, in the max_round sparse rounds like the
            // single-device loop): the steps of shard_open_step, the array each leaves merged on device 0 and handed back -- what the
            // four all-reduces per pass do between processes (sharded.py: set_keys_open).  The third, cycle-free search is not sharded.
            if (opts->enable_greedy_pivot_search && round < opts->max_round && npiv > 0 && !getenv("SPASM_AMD_MULTI_NO_OPEN_COLUMNS")) {
                for (int k = 0; k < nshards; k++) {
                    HIPCHK(hipSetDevice(dev_of(k)));
                    st[(size_t)k]->oc_i.ensure((size_t)m + 1);
                    st[(size_t)k]->oc_q.ensure((size_t)m + 1);
                }
                HIPCHK(hipSetDevice(dev_of(0)));
                DevBuf<int> stage_i;
                stage_i.alloc((size_t)m + 1);
                stage.ensure((size_t)m + 1);
                // kind 0: int32 MAX, 1: int32 SUM, 2: u64 MIN; the merged array ends up in every shard's buffer
                auto merge = [&](int kind) {
                    HIPCHK(hipSetDevice(dev_of(0)));
                    for (int k = 1; k < nshards; k++) {
                        if (kind == 2) {
                            HIPCHK(hipMemcpy(stage.p, st[(size_t)k]->oc_q.p, (size_t)m * sizeof(u64d), hipMemcpyDeviceToDevice));
                            hipLaunchKernelGGL(k_min_u64, dim3(cdiv(m, 256)), dim3(256), 0, nullptr, (i64d)m, st[0]->oc_q.p, stage.p);
                        } else {
                            HIPCHK(hipMemcpy(stage_i.p, st[(size_t)k]->oc_i.p, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice));
                            if (kind == 0) hipLaunchKernelGGL(k_max_i32, dim3(cdiv(m, 256)), dim3(256), 0, nullptr, (i64d)m, st[0]->oc_i.p, stage_i.p);
                            else hipLaunchKernelGGL(k_add_i32, dim3(cdiv(m, 256)), dim3(256), 0, nullptr, (i64d)m, st[0]->oc_i.p, stage_i.p);
                        }
                        HIPCHK(hipGetLastError());
                        HIPCHK(hipDeviceSynchronize());
                    }
                    for (int k = 1; k < nshards; k++) {
                        HIPCHK(hipSetDevice(dev_of(k)));
                        if (kind == 2) HIPCHK(hipMemcpy(st[(size_t)k]->oc_q.p, st[0]->oc_q.p, (size_t)m * sizeof(u64d), hipMemcpyDeviceToDevice));
                        else HIPCHK(hipMemcpy(st[(size_t)k]->oc_i.p, st[0]->oc_i.p, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice));
                    }
                };
                // one step on every shard: in / out = the shard's own buffer of the kind (0: none, 1: oc_i, 2: oc_q); returns shard 0's count
                auto step_all = [&](int step, int pass, int in_kind, int out_kind) {
                    int ret = 0;
                    for (int k = 0; k < nshards; k++) {
                        HIPCHK(hipSetDevice(dev_of(k)));
                        ShardState &q = *st[(size_t)k];
                        const void *in = in_kind == 1 ? (const void *)q.oc_i.p : in_kind == 2 ? (const void *)q.oc_q.p : nullptr;
                        void *out = out_kind == 1 ? (void *)q.oc_i.p : out_kind == 2 ? (void *)q.oc_q.p : nullptr;
                        const int rc = shard_open_step(q.sh, step, pass, in, out);
                        if (k == 0) ret = rc;
                        else if (rc != ret) throw EngineError("spasm_amd_echelonize_multi: the shards disagree on the pivots of a pass");
                    }
                    return ret;
                };
                step_all(OPEN_BEGIN, 0, 0, 1);
                merge(0);
                for (int pass = 1; pass <= OPEN_PASSES; pass++) {
                    step_all(OPEN_HIST, pass, 1, 1);
                    merge(1);
                    step_all(OPEN_PROPOSE, pass, 1, 2);
                    merge(2);
                    step_all(OPEN_ACCEPT, pass, 2, 1);
                    merge(0);
                    if (step_all(OPEN_RECORD, pass, 1, 1) == 0) break;
                    merge(0);
                }
                n_open = step_all(OPEN_FINISH, 0, 0, 0);
                if (n_open) spasm_logf("[pivots] ``Faugère-Lachartre on columns'' over %d shards: %d pivots found\n", nshards, n_open);
            }
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                ShardState &q = *st[(size_t)k];
                npiv = shard_finish_keys(q.sh, &q.n_own, &q.nnz_own);
                tot_rows += q.n_own;
                tot_ent += q.nnz_own;
            }
            if (npiv == 0) break;
            if (tot_rows != npiv) throw EngineError("spasm_amd_echelonize_multi: the shards do not own the elected pivot rows between them");
            // ---- exchange: every shard exports what it owns; every shard receives the concatenation
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                ShardState &q = *st[(size_t)k];
                q.hdr.ensure((size_t)2 * (size_t)std::max(q.n_own, 1));
                q.ent.ensure((size_t)2 * (size_t)std::max<i64>(q.nnz_own, 1));
                shard_export(q.sh, q.hdr.p, q.ent.p);
            }
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                ShardState &q = *st[(size_t)k];
                q.hdr_all.ensure((size_t)2 * (size_t)std::max(npiv, 1));
                q.ent_all.ensure((size_t)2 * (size_t)std::max<i64>(tot_ent, 1));
                i64 hr = 0, he = 0;
                for (int src = 0; src < nshards; src++) {
                    const ShardState &o = *st[(size_t)src];
                    if (o.n_own > 0) HIPCHK(hipMemcpy(q.hdr_all.p + 2 * hr, o.hdr.p, (size_t)2 * (size_t)o.n_own * sizeof(int), hipMemcpyDeviceToDevice));
                    if (o.nnz_own > 0) HIPCHK(hipMemcpy(q.ent_all.p + 2 * he, o.ent.p, (size_t)2 * (size_t)o.nnz_own * sizeof(int), hipMemcpyDeviceToDevice));
                    hr += o.n_own;
                    he += o.nnz_own;
                }
            }
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                ShardState &q = *st[(size_t)k];
                spasm_amd_shard *sh = q.sh;
                q.plan = shard_import(sh, npiv, tot_ent, q.hdr_all.p, q.ent_all.p, !ddf_now); // (the shard hands its matrix to the plan)
                q.sh = nullptr;
                delete sh;
            }
            // ---- the round's rows of U, from shard 0 (identical on all)
            {
                HIPCHK(hipSetDevice(dev_of(0)));
                std::vector<int> pc((size_t)npiv), ro((size_t)npiv);
                struct spasm_csr *Uc = plan_fetch_U(st[0]->plan, pc.data(), ro.data());
                const i64 base = U.p.back();
                for (int k = 0; k < npiv; k++) {
                    U.p.push_back(base + Uc->p[k + 1]);
                    U.pivcol.push_back(pc[(size_t)k]);
                    U.orig.push_back(ro[(size_t)k]);
                }
                const i64 uz = Uc->p[npiv];
                if (uz > 0) {
                    memcpy(U.j.grow((size_t)uz), Uc->j, sizeof(int) * (size_t)uz);
                    memcpy(U.x.grow((size_t)uz), Uc->x, sizeof(int) * (size_t)uz);
                }
                spasm_csr_free(Uc);
            }
            if (ddf_now) {
                if (dense_round()) {
                    g_multi_finish = 1;
                    spasm_logf("[echelonize] round %d (sharded): %d pivots, %lld rows / %lld entries before it; its Schur complement went dense\n", round, npiv,
                               (long long)rows_left, (long long)nnz_left);
                    break;
                }
                for (int k = 0; k < nshards; k++) {
                    HIPCHK(hipSetDevice(dev_of(k)));
                    shard_import_finish(st[(size_t)k]->plan);
                }
            }
            // ---- the Schur complement of every shard's rows becomes its matrix of the next round, on its device
            last_nnz = nnz_left;
            for (int k = 0; k < nshards; k++) {
                HIPCHK(hipSetDevice(dev_of(k)));
                ShardState &q = *st[(size_t)k];
                spasm_amd_schur_plan *P = q.plan;
                q.plan = nullptr; // consumed by the call, whatever happens
                q.sh = plan_advance(P, &q.rows, &q.nnz);
            }
            spasm_logf("[echelonize] round %d (sharded): %d pivots, %lld rows / %lld entries before it\n", round, npiv, (long long)rows_left, (long long)nnz_left);
            round++;
        }
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
    struct spasm_lu *N = assemble_lu(U, n, m, prime, nullptr);
    spasm_logf("[echelonize] Done in %.1fs. Rank %d, %lld nz in basis\n", spasm_wtime() - t0, N->r, (long long)U.p.back());
    return N;
}

// ------------------------------------------------------------------------------------------------
// The dense finish over row shards with ONE PROCESS PER SHARD (spasm.jl_amd/sharded.py: torch.distributed, RCCL): the steps of
// dense_finish_multi behind the C ABI, the exchanges between them are the caller's collectives -- an all-gather of the candidate
// records (every rank then runs the election itself: deterministic, nothing is sent back) and one broadcast per owner of the
// packed winner rows.
// ------------------------------------------------------------------------------------------------
struct DShardBase {
    virtual ~DShardBase() {}
    virtual void build(spasm_amd_schur_plan *P, DenseW &W, int me, int nshards, int C) = 0;
    virtual void build_rows(spasm_amd_schur_plan *P, DenseFill &fl, int me, int nshards, int C) = 0; // the live rows of P->A instead of a round's Schur rows
    virtual void block_begin() = 0;
    virtual void candidates(int c0, int w, void *cand_dev) = 0;
    virtual void elect(const void *stack_dev, int w) = 0;
    virtual i64 pack(int c0, void *buf) = 0;
    virtual void unpack(int q, int c0, int owner, const void *buf) = 0;
    virtual void apply(int q, int c0, int w, int b1) = 0;
    virtual void block_end(int b0, int b1, int npan) = 0;
    virtual int finish() = 0;
    virtual int extract(const int *clist, HostU &U) = 0;
    virtual void info(int *KB, i64 *ldc, int *elem, int *nd) = 0;
    PanelGlob hglob;
    int nshards = 1;
};

template <typename DT> struct DShardT : DShardBase {
    DenseShard<DT> sh;
    void build(spasm_amd_schur_plan *P, DenseW &W, int me, int nsh, int C) override
    {
        nshards = nsh;
        memset(&hglob, 0, sizeof hglob);
        sh.me = me;
        sh.C = C;
        sh.ldc = ((i64)C + 63) / 64 * 64;
        sh.F = P->R.F;
        sh.KB = dense_kb();
        sh.R = P->R.nnp;
        sh.s = P->R.stream;
        schur_dense_build(P->R, P->A, sh.R, W, sh.KB, sh.D, sh.row_orig, P->R.stream);
        sh.setup(nsh, true);
    }
    void build_rows(spasm_amd_schur_plan *P, DenseFill &fl, int me, int nsh, int C) override
    {
        nshards = nsh;
        memset(&hglob, 0, sizeof hglob);
        sh.me = me;
        sh.C = C;
        sh.ldc = ((i64)C + 63) / 64 * 64;
        sh.F = P->R.F;
        sh.KB = dense_kb();
        sh.R = fl.R;
        sh.s = P->R.stream;
        fl.build(sh.KB, sh.D, sh.row_orig); // (KB guest rows behind the shard's own, as schur_dense_build leaves them)
        sh.setup(nsh, true);
    }
    void block_begin() override { sh.block_begin(); }
    void candidates(int c0, int w, void *cand_dev) override
    {
        sh.candidates(c0, w);
        HIPCHK(hipMemcpyAsync(cand_dev, sh.cand.p, sizeof(CandRec), hipMemcpyDeviceToDevice, sh.s));
        HIPCHK(hipStreamSynchronize(sh.s));
    }
    void elect(const void *stack_dev, int w) override { sh.elect_from(stack_dev, nshards, w, &hglob); }
    i64 pack(int c0, void *buf) override
    {
        sh.pack(c0, &hglob, true);
        return sh.export_to(c0, &hglob, buf);
    }
    void unpack(int q, int c0, int owner, const void *buf) override { sh.import_from(q, c0, owner, &hglob, buf); }
    void apply(int q, int c0, int w, int b1) override { sh.apply_panel(q, c0, w, b1); }
    void block_end(int b0, int b1, int npan) override { sh.block_end(b0, b1, npan); }
    int finish() override { return sh.finish(); }
    int extract(const int *clist, HostU &U) override { return dense_extract_U(sh.D.p, sh.C, sh.ldc, sh.own_pc.p, clist, sh.row_orig.p, U, sh.s); }
    void info(int *KB, i64 *ldc, int *elem, int *nd) override
    {
        if (KB) *KB = sh.KB;
        if (ldc) *ldc = sh.ldc;
        if (elem) *elem = (int)sizeof(DT);
        if (nd) *nd = sh.ND;
    }
};

} // namespace

struct spasm_amd_dshard {
    spasm_amd_schur_plan *plan = nullptr; // not owned
    std::unique_ptr<DenseW> dw;           // the Schur rows of the plan's round through the dense W ..
    std::unique_ptr<DenseFill> fl;        // .. or (spasm_amd_dshard_open_rows) the live rows of the shard's matrix as they are
    const int *cflag() const { return fl ? fl->cflag.p : dw->cflag.p; }
    const int *clist() const { return fl ? fl->clist.p : dw->clist.p; }
    std::unique_ptr<DShardBase> impl;
    int me = 0, nshards = 1, C = 0;
};

namespace {

// (a step called out of order -- no handle, or before dshard_build -- is an error, not a crash)
void dshard_built(const spasm_amd_dshard *ds)
{
    if (!ds || !ds->impl) throw EngineError("no dense shard (spasm_amd_dshard_open / _density / _build come first)");
}

void dshard_opened(const spasm_amd_dshard *ds)
{
    if (!ds || (!ds->dw && !ds->fl)) throw EngineError("no dense shard (spasm_amd_dshard_open comes first)");
}

spasm_amd_dshard *dshard_open(spasm_amd_schur_plan *P, int me, int nshards)
{
    if (!P) throw EngineError("spasm_amd_dshard_open: null plan");
    if (!P->R.F.small) throw EngineError("spasm_amd_dshard_open: the dense finish over shards takes primes below 2^16");
    const int elem = P->R.F.p <= 255 ? 1 : 2;
    if (nshards < 1 || nshards > DM_MAXSHARDS || nshards * DP_W > 147456 / (DP_W * elem)) throw EngineError("spasm_amd_dshard_open: too many shards for the election workgroup");
    if (me < 0 || me >= nshards) throw EngineError("spasm_amd_dshard_open: shard number out of range");
    std::unique_ptr<spasm_amd_dshard> ds(new spasm_amd_dshard());
    ds->plan = P;
    ds->me = me;
    ds->nshards = nshards;
    ds->dw.reset(new DenseW(P->R, P->A, P->R.stream));
    ds->dw->flag_columns();
    HIPCHK(hipStreamSynchronize(P->R.stream));
    return ds.release();
}

// the same over the shard's CURRENT rows (no round, no U): a remainder that is dense already is eliminated by all ranks together
// where it is (the one-process path's dense_now)
spasm_amd_dshard *dshard_open_rows(spasm_amd_shard *S, int me, int nshards)
{
    if (!S || !S->plan) throw EngineError("spasm_amd_dshard_open_rows: null shard");
    spasm_amd_schur_plan *P = S->plan;
    if (!P->R.F.small) throw EngineError("spasm_amd_dshard_open_rows: the dense finish over shards takes primes below 2^16");
    const int elem = P->R.F.p <= 255 ? 1 : 2;
    if (nshards < 1 || nshards > DM_MAXSHARDS || nshards * DP_W > 147456 / (DP_W * elem)) throw EngineError("spasm_amd_dshard_open_rows: too many shards for the election workgroup");
    if (me < 0 || me >= nshards) throw EngineError("spasm_amd_dshard_open_rows: shard number out of range");
    std::unique_ptr<spasm_amd_dshard> ds(new spasm_amd_dshard());
    ds->plan = P;
    ds->me = me;
    ds->nshards = nshards;
    ds->fl.reset(new DenseFill(P->A, P->R.stream));
    ds->fl->flag_columns();
    return ds.release();
}

// the rows of U this shard owns after the finish, as a host CSR; pivcol_out / row_out: their pivot columns and originating rows
struct spasm_csr *dshard_fetch_U(spasm_amd_dshard *ds, int *pivcol_out, int *row_out, int *n_out)
{
    HostU U;
    U.p.push_back(0);
    const int got = ds->impl->extract(ds->clist(), U);
    const i64 nz = U.p.back();
    struct spasm_csr *Uc = spasm_csr_alloc(got, ds->plan->A.m, nz, ds->plan->prime, true);
    if (!Uc) throw EngineError("out of host memory for the shard's rows of U");
    for (int k = 0; k <= got; k++) Uc->p[k] = U.p[(size_t)k];
    if (nz > 0) {
        memcpy(Uc->j, U.j.data(), sizeof(int) * (size_t)nz);
        memcpy(Uc->x, U.x.data(), sizeof(int) * (size_t)nz);
    }
    for (int k = 0; k < got; k++) {
        if (pivcol_out) pivcol_out[k] = U.pivcol[(size_t)k];
        if (row_out) row_out[k] = U.orig[(size_t)k];
    }
    if (n_out) *n_out = got;
    return Uc;
}

} // namespace

// ------------------------------------------------------------------------------------------------
// Exact products with A (spmv.hpp): the operator keeps A on the device, and its transpose once a product x A is asked for.
// ------------------------------------------------------------------------------------------------
namespace {

// one orientation as gather-by-row, with its rows binned by length (spmv.hpp)
struct SpmvView {
    int rows = 0, cols = 0;
    const i64d *start = nullptr;
    const int *len = nullptr;
    const int2 *ent = nullptr;
    DevBuf<int> tlen;                      // transposed view: row lengths from the row pointers
    int nshort = 0, nmid = 0, nlong = 0, nseg = 0;
    bool short_all = false;                // every row is short: the short kernel runs over 0 .. rows-1 without a list
    DevBuf<int> short_rows, mid_rows, long_rows, long_off, seg_row, seg_beg, part;

    // hlen: an upper bound of every row's length (the host CSR's, before zeros are dropped, or the transpose's)
    void bin(const std::vector<i64> &hlen, hipStream_t s)
    {
        std::vector<int> sr, mr, lr, lo, sg, sb;
        for (int i = 0; i < rows; i++) {
            const i64 l = hlen[(size_t)i];
            if (l <= SPMV_SHORT) sr.push_back(i);
            else if (l <= SPMV_SEG) mr.push_back(i);
            else {
                lr.push_back(i);
                lo.push_back((int)sg.size());
                for (i64 b = 0; b < l; b += SPMV_SEG) { sg.push_back(i); sb.push_back((int)b); }
            }
        }
        lo.push_back((int)sg.size());
        nshort = (int)sr.size();
        nmid = (int)mr.size();
        nlong = (int)lr.size();
        nseg = (int)sg.size();
        short_all = nshort == rows;
        auto up = [&](DevBuf<int> &d, const std::vector<int> &h) {
            d.alloc(h.size());
            if (!h.empty()) HIPCHK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s));
        };
        if (!short_all) up(short_rows, sr);
        up(mid_rows, mr);
        up(long_rows, lr);
        up(long_off, lo);
        up(seg_row, sg);
        up(seg_beg, sb);
        part.alloc((size_t)nseg * 64);
        HIPCHK(hipStreamSynchronize(s)); // the host vectors go out of scope
    }

    // a view of rows_ rows from device row pointers p[0 .. rows_]: they serve as starts, the lengths are their differences
    void from_row_pointers(int rows_, int cols_, const i64d *p, const int2 *ent_, hipStream_t s)
    {
        rows = rows_;
        cols = cols_;
        start = p;
        ent = ent_;
        tlen.alloc((size_t)rows + 1);
        if (rows > 0) {
            hipLaunchKernelGGL(k_spmv_len_from_ptr, dim3(cdiv(rows, 256)), dim3(256), 0, s, rows, p, tlen.p);
            HIPCHK(hipGetLastError());
        }
        len = tlen.p;
        std::vector<i64d> hp((size_t)rows + 1);
        HIPCHK(hipMemcpyAsync(hp.data(), p, hp.size() * sizeof(i64d), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::vector<i64> hl((size_t)rows);
        for (int i = 0; i < rows; i++) hl[(size_t)i] = hp[(size_t)i + 1] - hp[(size_t)i];
        bin(hl, s);
    }

    // The launches of one product with KW columns, in their order: sum(team, partial, nitems, items, segbeg, part) for each
    // non-empty class (team and partial are std::integral_constants: the TEAM and PARTIAL of SPMV_TEAM_SUM), then
    // combine(nlong, rows, off, part) after the segments of the long rows.  Returns the number of launches.
    template <int KW, class Sum, class Combine> int for_classes(Sum &&sum, Combine &&combine) const
    {
        typedef std::integral_constant<int, 64> wave;
        int launches = 0;
        if (nshort > 0) {
            sum(std::integral_constant<int, spmv_short_team(KW)>(), std::false_type(), nshort, short_all ? nullptr : short_rows.p, nullptr, nullptr);
            launches++;
        }
        if (nmid > 0) {
            sum(wave(), std::false_type(), nmid, mid_rows.p, nullptr, nullptr);
            launches++;
        }
        if (nlong > 0) {
            sum(wave(), std::true_type(), nseg, seg_row.p, seg_beg.p, part.p);
            combine(nlong, long_rows.p, long_off.p, part.p);
            launches += 2;
        }
        return launches;
    }
};

// the width KW of a chunk of k >= 1 columns: the next power of two
int spmv_kw(int k)
{
    int kw = 1;
    while (kw < k) kw <<= 1;
    return kw;
}

// f(std::integral_constant<int, KW>) for kw = KW in 1, 2, 4, .., 64
template <class Fn> auto dispatch_kw(int kw, Fn &&f)
{
    switch (kw) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return f(std::integral_constant<int, 64>());
    }
}

// Y <- A X + Y: one team per work item, 256 lanes a workgroup, no grid cap
template <bool SMALL, int KW>
void spmv_launch(const SpmvView &V, const ZpField &F, int kc, const int *X, i64 ldx, int *Y, i64 ldy, hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp;
    V.for_classes<KW>(
        [&](auto team, auto partial, int nitems, const int *items, const int *segbeg, int *part) {
            constexpr int TEAM = decltype(team)::value;
            hipLaunchKernelGGL((k_spmv<SMALL, KW, TEAM, decltype(partial)::value>), dim3(cdiv((i64)nitems * TEAM, 256)), dim3(256), 0, s, nitems, items,
                               segbeg, V.start, V.len, V.ent, F, hp, mhp, kc, X, (i64d)ldx, Y, (i64d)ldy, part);
        },
        [&](int nlong, const int *rows, const int *off, const int *part) {
            hipLaunchKernelGGL(k_spmv_combine, dim3(cdiv((i64)nlong * KW, 256)), dim3(256), 0, s, nlong, rows, off, part, KW, kc, F, Y, (i64d)ldy);
        });
    HIPCHK(hipGetLastError());
}

// the ping-pong buffers and the projection sums of one Krylov sequence (krylov.hpp; the section at the end of this file)
struct KrylovWork {
    DevBuf<int> w0, w1;
    DevBuf<int> mid;                       // the n x KW intermediate D2 A X of a composite block Horner step
    DevBuf<long long> acc;
    // the coefficient table of a Horner run (horner.hpp): the host copy lives here until its upload has completed
    DevBuf<int> tab;
    std::vector<int> htab;
    hipEvent_t tab_up = nullptr;
    KrylovWork() {}
    KrylovWork(const KrylovWork &) = delete;
    KrylovWork &operator=(const KrylovWork &) = delete;
    ~KrylovWork() { if (tab_up) (void)hipEventDestroy(tab_up); }
};

} // namespace

struct spasm_amd_spmv {
    int dev = 0;
    ZpField F;
    DevMat A;
    TransposeOut T;
    bool have_t = false;
    SpmvView fwd, tr;
    DevBuf<int> hx, hy;   // staging of the host-array applies
    KrylovWork kry;       // buffers of spasm_amd_krylov_sequence_dev (krylov.hpp)

    // the transposed view, built on the first x A: the device counting sort of the engine, then its rows binned
    void build_transpose()
    {
        if (have_t) return;
        hipStream_t s = nullptr;
        Scanner scan;
        device_transpose(A, A.n, nullptr, nullptr, 0, scan, s, T);
        tr.from_row_pointers(A.m, A.n, T.Tp.p, T.Tent.p, s);
        have_t = true;
    }

    // Y <- op(A) X + Y on device arrays, enqueued on s
    void apply_dev(int trans, int k, const int *X, i64 ldx, int *Y, i64 ldy, hipStream_t s)
    {
        if (trans) build_transpose();
        const SpmvView &V = trans ? tr : fwd;
        for (int k0 = 0; k0 < k; k0 += 64) {
            const int kc = std::min(k - k0, 64);
            dispatch_kw(spmv_kw(kc), [&](auto KW) {
                if (F.small) spmv_launch<true, KW()>(V, F, kc, X + k0, ldx, Y + k0, ldy, s);
                else spmv_launch<false, KW()>(V, F, kc, X + k0, ldx, Y + k0, ldy, s);
            });
        }
    }

    // the same on host arrays, through device copies packed with leading dimension k; Y is written only once all went well
    void apply_host(int trans, int k, const int *X, i64 ldx, int *Y, i64 ldy)
    {
        if (trans) build_transpose();
        const SpmvView &V = trans ? tr : fwd;
        const size_t xr = (size_t)V.cols, yr = (size_t)V.rows, kk = (size_t)k;
        if (k == 0 || yr == 0) return;
        hipStream_t s = nullptr;
        hx.ensure(xr * kk);
        hy.ensure(yr * kk);
        if (xr > 0) HIPCHK(hipMemcpy2DAsync(hx.p, kk * sizeof(int), X, (size_t)ldx * sizeof(int), kk * sizeof(int), xr, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpy2DAsync(hy.p, kk * sizeof(int), Y, (size_t)ldy * sizeof(int), kk * sizeof(int), yr, hipMemcpyHostToDevice, s));
        apply_dev(trans, k, hx.p, k, hy.p, k, s);
        std::vector<int> out(yr * kk);
        HIPCHK(hipMemcpyAsync(out.data(), hy.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t i = 0; i < yr; i++) memcpy(Y + i * (size_t)ldy, out.data() + i * kk, kk * sizeof(int));
    }
};

namespace {

spasm_amd_spmv *spmv_create(const struct spasm_csr *A, const char *who)
{
    require_device();
    check_input(A, who);
    if (!A->x) throw EngineError(std::string(who) + ": matrix without values (A->x == NULL)");
    std::unique_ptr<spasm_amd_spmv> op(new spasm_amd_spmv());
    HIPCHK(hipGetDevice(&op->dev));
    op->F = zp_field_make(A->field->p);
    hipStream_t s = nullptr;
    upload_csr(A, 0, A->n, op->A, s);
    SpmvView &V = op->fwd;
    V.rows = A->n;
    V.cols = A->m;
    V.start = op->A.start.p;
    V.len = op->A.len.p;
    V.ent = op->A.ent.p;
    std::vector<i64> hl((size_t)A->n);
    for (int i = 0; i < A->n; i++) hl[(size_t)i] = A->p[i + 1] - A->p[i];
    V.bin(hl, s);
    return op.release();
}

void spmv_check(const spasm_amd_spmv *op, int trans, int k, const void *X, i64 ldx, const void *Y, i64 ldy, const char *who)
{
    if (!op) throw EngineError(std::string(who) + ": NULL operator");
    if (k < 0 || ldx < k || ldy < k || (trans != 0 && trans != 1)) throw EngineError(std::string(who) + ": bad arguments (trans 0/1, k >= 0, ldx >= k, ldy >= k)");
    const int xr = trans ? op->A.n : op->A.m, yr = trans ? op->A.m : op->A.n;
    if (k > 0 && ((xr > 0 && !X) || (yr > 0 && !Y))) throw EngineError(std::string(who) + ": NULL array");
}

// spasm_Axpy / spasm_xApy: y <- op(A) x + y through a temporary operator
void spmv_once(const struct spasm_csr *A, int trans, const spasm_ZZp *x, spasm_ZZp *y, const char *who)
{
    std::unique_ptr<spasm_amd_spmv> op(spmv_create(A, who));
    spmv_check(op.get(), trans, 1, x, 1, y, 1, who);
    op->apply_host(trans, 1, x, 1, y, 1);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// Sparse matrix algebra on resident matrices (spgemm.hpp): products, linear combinations, submatrices.  A handle owns the row
// pointers and the packed {column, value} entries of one matrix; every operation makes a new handle in canonical form.
// ------------------------------------------------------------------------------------------------
struct spasm_amd_dcsr {
    int dev = 0;
    int n = 0, m = 0;
    i64 nnz = 0;
    ZpField F;
    bool canonical = false;  // rows sorted, no duplicate column, no zero: true for every result, unknown for an upload
    DevBuf<i64d> p;          // n + 1
    DevBuf<int2> ent;        // nnz
    i64 stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

template <int LOGT, int BS, bool SMALL> void spg_launch_hash(const SpgArgs &a, int nitems, const int *items, hipStream_t s)
{
    constexpr size_t lds = spg_hash_lds<SMALL>(LOGT, BS);
    static bool attr_done[kMaxDev] = {false};
    bool &done = attr_done[current_device()];
    if (!done) {
        HIPCHK(hipFuncSetAttribute((const void *)k_spg_hash<LOGT, BS, SMALL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    hipLaunchKernelGGL((k_spg_hash<LOGT, BS, SMALL>), dim3(nitems), dim3(BS), lds, s, a, nitems, items);
}

template <bool SMALL> void spg_launch_class(int cls, const SpgArgs &a, int nitems, const int *items, hipStream_t s)
{
    switch (cls) {
    case 0: hipLaunchKernelGGL((k_spg_tiny<SMALL>), dim3(cdiv(nitems, 256 / SPG_TINY_TEAM)), dim3(256), 0, s, a, nitems, items); break;
    case 1: spg_launch_hash<7, 64, SMALL>(a, nitems, items, s); break;
    case 2: spg_launch_hash<8, 64, SMALL>(a, nitems, items, s); break;
    case 3: spg_launch_hash<9, 64, SMALL>(a, nitems, items, s); break;
    case 4: spg_launch_hash<10, 64, SMALL>(a, nitems, items, s); break;
    case 5: spg_launch_hash<11, 256, SMALL>(a, nitems, items, s); break;
    case 6: spg_launch_hash<12, 256, SMALL>(a, nitems, items, s); break;
    case 7: spg_launch_hash<13, 256, SMALL>(a, nitems, items, s); break;
    default: break;
    }
    HIPCHK(hipGetLastError());
}

struct SpgEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    SpgEvents() { for (auto &x : e) HIPCHK(hipEventCreate(&x)); }
    ~SpgEvents() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
    double ms(int a, int b)
    {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, e[a], e[b]));
        return (double)t;
    }
};

// bytes of scratch one chunk of rows may use: a third of the free device memory (SPASM_AMD_SPGEMM_SCRATCH_MB: a smaller figure,
// for the tests of the chunked path)
size_t spg_budget()
{
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    size_t b = fr / 3;
    const char *e = getenv("SPASM_AMD_SPGEMM_SCRATCH_MB");
    if (e && atof(e) > 0) b = std::min(b, (size_t)(atof(e) * 1048576.0));
    return b;
}

// C = op(A, B): the driver of the three steps of spgemm.hpp.  mode SPG_MUL: A (n x k) * B (k x m); SPG_LINCOMB: sa * A + sb * B (B may
// be null); SPG_SUBMATRIX: A[r0:r1, c0:c1].  The operands have been checked by the caller.
std::unique_ptr<spasm_amd_dcsr> spg_run(int mode, const spasm_amd_dcsr &A, const spasm_amd_dcsr *B, int sa, int sb, int r0, int r1, int c0, int c1)
{
    hipStream_t s = nullptr;
    std::unique_ptr<spasm_amd_dcsr> R(new spasm_amd_dcsr());
    R->dev = A.dev;
    R->F = A.F;
    R->canonical = true;
    const int n = mode == SPG_SUBMATRIX ? r1 - r0 : A.n;
    const int m = mode == SPG_MUL ? B->m : (mode == SPG_SUBMATRIX ? c1 - c0 : A.m);
    R->n = n;
    R->m = m;
    R->p.alloc((size_t)n + 1);
    R->stats[10] = mode;
    if (n == 0 || m == 0) { // nothing to compute (and no accumulator of zero columns)
        HIPCHK(hipMemsetAsync(R->p.p, 0, ((size_t)n + 1) * sizeof(i64d), s));
        R->ent.alloc(1);
        HIPCHK(hipStreamSynchronize(s));
        return R;
    }
    int num_cu = 256;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, A.dev) == hipSuccess) num_cu = prop.multiProcessorCount;
    }
    SpgArgs a;
    memset(&a, 0, sizeof a);
    a.mode = mode;
    a.nrows = n;
    a.ncols = m;
    a.Ap = A.p.p;
    a.Aent = A.ent.p;
    a.Bp = B ? B->p.p : nullptr;
    a.Bent = B ? B->ent.p : nullptr;
    a.sa = sa;
    a.sb = sb;
    a.r0 = mode == SPG_SUBMATRIX ? r0 : 0;
    a.c0 = mode == SPG_SUBMATRIX ? c0 : 0;
    a.c1 = mode == SPG_SUBMATRIX ? c1 : m;
    a.F = A.F;

    SpgEvents ev;
    Scanner scan;
    DevBuf<i64d> bound, cap, off, cnt, tmp;
    const size_t n1 = (size_t)n + 1;
    bound.alloc(n1);
    cap.alloc(n1);
    off.alloc(n1);
    cnt.alloc(n1);
    tmp.alloc(n1);
    bound.zero(s);
    cap.zero(s);
    cnt.zero(s);
    // ---- size
    HIPCHK(hipEventRecord(ev.e[0], s));
    if (mode == SPG_MUL && A.nnz > 8 * (i64)A.n) hipLaunchKernelGGL(k_spg_size_wave, dim3(cdiv((i64)n * 64, 256)), dim3(256), 0, s, a, bound.p, cap.p);
    else hipLaunchKernelGGL(k_spg_size, dim3(cdiv(n, 256)), dim3(256), 0, s, a, bound.p, cap.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(cap.p, off.p, n1, s);
    scan.exclusive(bound.p, tmp.p, n1, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    i64d total_cap = 0, flops = 0;
    HIPCHK(hipMemcpyAsync(&total_cap, off.p + n, sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&flops, tmp.p + n, sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double ms_size = ev.ms(0, 1), ms_num = 0, ms_compact = 0;
    a.off = off.p;
    a.cnt = cnt.p;

    // ---- chunks of rows whose scratch slices fit the budget
    const size_t budget = spg_budget();
    const i64 max_ent = (i64)(budget / sizeof(int2));
    std::vector<int> cut; // chunk c = rows cut[c] .. cut[c + 1] - 1
    std::vector<i64d> hoff;
    cut.push_back(0);
    if (total_cap <= max_ent) {
        cut.push_back(n);
    } else {
        hoff.resize(n1);
        HIPCHK(hipMemcpy(hoff.data(), off.p, n1 * sizeof(i64d), hipMemcpyDeviceToHost));
        int lo = 0;
        while (lo < n) {
            int hi = lo;
            while (hi < n && hoff[(size_t)hi + 1] - hoff[(size_t)lo] <= max_ent) hi++;
            if (hi == lo) {
                char b[256];
                snprintf(b, sizeof b, "row %d alone needs %.2f GiB of scratch, %.2f GiB may be used", lo,
                         (double)(hoff[(size_t)lo + 1] - hoff[(size_t)lo]) * 8.0 / 1073741824.0, (double)budget / 1073741824.0);
                throw EngineError(b);
            }
            cut.push_back(hi);
            lo = hi;
        }
    }
    const int nchunks = (int)cut.size() - 1;

    DevBuf<unsigned char> key, key2, sort_tmp;
    DevBuf<int> rowid, rowid2, hist;
    DevBuf<i64d> maxb, pos;
    DevBuf<int2> scratch;
    DevBuf<long long> dense;
    size_t dense_rows = 0;
    hist.alloc(16);
    maxb.alloc(1);
    maxb.zero(s);
    std::vector<DevBuf<int2>> parts((size_t)nchunks);
    std::vector<i64> part_nnz((size_t)nchunks, 0);
    i64 rows_path[3] = {0, 0, 0};
    size_t peak = 0;
    for (int c = 0; c < nchunks; c++) {
        const int lo = cut[(size_t)c], hi = cut[(size_t)c + 1], nc = hi - lo;
        const i64d off_lo = nchunks == 1 ? 0 : hoff[(size_t)lo];
        const i64d chunk_cap = nchunks == 1 ? total_cap : hoff[(size_t)hi] - off_lo;
        key.ensure((size_t)nc);
        key2.ensure((size_t)nc);
        rowid.ensure((size_t)nc);
        rowid2.ensure((size_t)nc);
        pos.ensure((size_t)nc + 1);
        scratch.ensure((size_t)chunk_cap + 1);
        hist.zero(s);
        hipLaunchKernelGGL(k_spg_classify, dim3(cdiv(nc, 256)), dim3(256), 0, s, lo, nc, bound.p, key.p, rowid.p, hist.p, maxb.p);
        HIPCHK(hipGetLastError());
        {
            size_t bytes = 0;
            HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, key.p, key2.p, rowid.p, rowid2.p, (size_t)nc, 0, 4, s));
            sort_tmp.ensure(bytes);
            HIPCHK(rocprim::radix_sort_pairs(sort_tmp.p, bytes, key.p, key2.p, rowid.p, rowid2.p, (size_t)nc, 0, 4, s));
        }
        int h[16];
        HIPCHK(hipMemcpyAsync(h, hist.p, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        a.off_base = off_lo;
        a.scratch = scratch.p;
        // the global class: as many rows at a time as workgroups fit the device, and as accumulators fit the budget
        int nglobal = h[SPG_CLS_GLOBAL], gblocks = 0;
        if (nglobal > 0) {
            const size_t per_row = (size_t)m * sizeof(long long);
            const size_t fit = budget / per_row;
            if (fit == 0) {
                char b[256];
                snprintf(b, sizeof b, "a row of more than %d products needs an accumulator of %.2f GiB, %.2f GiB may be used", 64 << (SPG_LOGT_MAX - SPG_LOGT_MIN),
                         (double)per_row / 1073741824.0, (double)budget / 1073741824.0);
                throw EngineError(b);
            }
            gblocks = (int)std::min<size_t>(std::min<size_t>((size_t)nglobal, (size_t)num_cu * 2), fit);
            if ((size_t)gblocks > dense_rows) {
                dense.alloc((size_t)gblocks * (size_t)m);
                dense.zero(s); // (the kernel leaves it zero)
                dense_rows = (size_t)gblocks;
            }
        }
        peak = std::max(peak, scratch.n * sizeof(int2) + dense.n * sizeof(long long));
        // ---- numeric
        HIPCHK(hipEventRecord(ev.e[1], s));
        int first = 0;
        for (int cls = 0; cls < SPG_NCLASS; cls++) {
            const int cntc = h[cls];
            if (cntc > 0 && cls < SPG_CLS_GLOBAL) {
                if (A.F.small) spg_launch_class<true>(cls, a, cntc, rowid2.p + first, s);
                else spg_launch_class<false>(cls, a, cntc, rowid2.p + first, s);
                rows_path[cls == 0 ? 0 : 1] += cntc;
            } else if (cntc > 0 && cls == SPG_CLS_GLOBAL) {
                hipLaunchKernelGGL(k_spg_global, dim3(gblocks), dim3(256), 0, s, a, cntc, rowid2.p + first, dense.p);
                HIPCHK(hipGetLastError());
                rows_path[2] += cntc;
            }
            first += cntc;
        }
        // ---- compact
        HIPCHK(hipEventRecord(ev.e[2], s));
        scan.exclusive(cnt.p + lo, pos.p, (size_t)nc + 1, s); // (cnt[hi] is still 0: the chunks go in ascending order)
        i64d cn = 0;
        HIPCHK(hipMemcpyAsync(&cn, pos.p + nc, sizeof(i64d), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        parts[(size_t)c].alloc((size_t)cn + 1);
        part_nnz[(size_t)c] = cn;
        if (cn > 0) {
            if (chunk_cap <= 16 * (i64d)nc) hipLaunchKernelGGL((k_spg_pack<8>), dim3(cdiv((i64)nc * 8, 256)), dim3(256), 0, s, lo, nc, off.p, off_lo, scratch.p, cnt.p, pos.p, parts[(size_t)c].p);
            else hipLaunchKernelGGL((k_spg_pack<64>), dim3(cdiv((i64)nc * 64, 256)), dim3(256), 0, s, lo, nc, off.p, off_lo, scratch.p, cnt.p, pos.p, parts[(size_t)c].p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ev.e[3], s));
        HIPCHK(hipStreamSynchronize(s));
        ms_num += ev.ms(1, 2);
        ms_compact += ev.ms(2, 3);
    }
    scratch.release();
    dense.release();
    // ---- the row pointers, and the parts back to back
    scan.exclusive(cnt.p, R->p.p, n1, s);
    i64 nnz = 0;
    for (i64 v : part_nnz) nnz += v;
    R->nnz = nnz;
    if (nchunks == 1) {
        R->ent = std::move(parts[0]);
    } else {
        R->ent.alloc((size_t)nnz + 1);
        i64 at = 0;
        for (int c = 0; c < nchunks; c++) {
            if (part_nnz[(size_t)c] > 0)
                HIPCHK(hipMemcpyAsync(R->ent.p + at, parts[(size_t)c].p, (size_t)part_nnz[(size_t)c] * sizeof(int2), hipMemcpyDeviceToDevice, s));
            at += part_nnz[(size_t)c];
        }
    }
    i64d hmax = 0;
    HIPCHK(hipMemcpyAsync(&hmax, maxb.p, sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 *st = R->stats;
    st[0] = flops;
    st[1] = nnz;
    st[2] = rows_path[0];
    st[3] = rows_path[1];
    st[4] = rows_path[2];
    st[5] = nchunks;
    st[6] = (i64)(ms_size * 1000.0);
    st[7] = (i64)(ms_num * 1000.0);
    st[8] = (i64)(ms_compact * 1000.0);
    st[9] = (i64)peak;
    st[11] = hmax;
    return R;
}

spasm_amd_dcsr *dcsr_upload(const struct spasm_csr *A, const char *who)
{
    require_device();
    check_input(A, who);
    const std::string w(who);
    if (!A->x) throw EngineError(w + ": matrix without values (A->x == NULL)");
    const int n = A->n, m = A->m;
    if (n < 0 || m < 0 || !A->p || A->p[0] != 0) throw EngineError(w + ": malformed matrix");
    for (int i = 0; i < n; i++)
        if (A->p[i + 1] < A->p[i]) throw EngineError(w + ": row pointers must not decrease");
    const i64 nnz = A->p[n];
    if (nnz > 0 && !A->j) throw EngineError(w + ": malformed matrix");
    std::unique_ptr<spasm_amd_dcsr> D(new spasm_amd_dcsr());
    HIPCHK(hipGetDevice(&D->dev));
    D->F = zp_field_make(A->field->p);
    D->n = n;
    D->m = m;
    D->nnz = nnz;
    hipStream_t s = nullptr;
    D->p.alloc((size_t)n + 1);
    D->ent.alloc((size_t)nnz + 1);
    static_assert(sizeof(i64d) == sizeof(i64), "row pointers are copied as they are");
    HIPCHK(hipMemcpyAsync(D->p.p, A->p, ((size_t)n + 1) * sizeof(i64d), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        DevBuf<int> dj, dx, bad;
        dj.alloc((size_t)nnz);
        dx.alloc((size_t)nnz);
        bad.alloc(1);
        bad.zero(s);
        HIPCHK(hipMemcpyAsync(dj.p, A->j, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dx.p, A->x, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        const int grid = (int)std::min<i64>(cdiv(nnz, 256), 65536);
        hipLaunchKernelGGL(k_spg_check_cols, dim3(grid), dim3(256), 0, s, (i64d)nnz, m, dj.p, bad.p);
        hipLaunchKernelGGL(k_pack_entries, dim3(grid), dim3(256), 0, s, (i64d)nnz, D->F, dj.p, dx.p, D->ent.p);
        HIPCHK(hipGetLastError());
        int hbad = 0;
        HIPCHK(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (hbad) throw EngineError(w + ": a column index lies outside the matrix");
    }
    HIPCHK(hipStreamSynchronize(s));
    return D.release();
}

struct spasm_csr *dcsr_download(const spasm_amd_dcsr *D)
{
    hipStream_t s = nullptr;
    struct spasm_csr *R = spasm_csr_alloc(D->n, D->m, D->nnz, D->F.p, true);
    if (!R) throw EngineError("out of host memory");
    try {
        HIPCHK(hipMemcpyAsync(R->p, D->p.p, ((size_t)D->n + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
        if (D->nnz > 0) {
            DevBuf<int> dj, dx;
            dj.alloc((size_t)D->nnz);
            dx.alloc((size_t)D->nnz);
            hipLaunchKernelGGL(k_spg_unpack, dim3((int)std::min<i64>(cdiv(D->nnz, 256), 65536)), dim3(256), 0, s, (i64d)D->nnz, D->ent.p, dj.p, dx.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(R->j, dj.p, (size_t)D->nnz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(R->x, dx.p, (size_t)D->nnz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        HIPCHK(hipStreamSynchronize(s));
    } catch (...) {
        spasm_csr_free(R);
        throw;
    }
    return R;
}

int spg_scalar(const ZpField &F, i64 a)
{
    i64 r = a % F.p;
    if (r < 0) r += F.p;
    return zp_normalize(F, r);
}

void dcsr_need(const spasm_amd_dcsr *D, const char *who)
{
    if (!D) throw EngineError(std::string(who) + ": NULL matrix");
}

spasm_amd_dcsr *dcsr_mul(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B, const char *who)
{
    dcsr_need(A, who);
    dcsr_need(B, who);
    const std::string w(who);
    if (A->F.p != B->F.p) throw EngineError(w + ": the matrices are over different primes");
    if (A->m != B->n) throw EngineError(w + ": dimension mismatch (columns of A, rows of B)");
    if (A->dev != B->dev) throw EngineError(w + ": the matrices live on different devices");
    return spg_run(SPG_MUL, *A, B, 1, 1, 0, 0, 0, 0).release();
}

spasm_amd_dcsr *dcsr_lincomb(i64 a, const spasm_amd_dcsr *A, i64 b, const spasm_amd_dcsr *B, const char *who)
{
    dcsr_need(A, who);
    const std::string w(who);
    if (B) {
        if (A->F.p != B->F.p) throw EngineError(w + ": the matrices are over different primes");
        if (A->n != B->n || A->m != B->m) throw EngineError(w + ": dimension mismatch");
        if (A->dev != B->dev) throw EngineError(w + ": the matrices live on different devices");
    }
    return spg_run(SPG_LINCOMB, *A, B, spg_scalar(A->F, a), spg_scalar(A->F, b), 0, 0, 0, 0).release();
}

spasm_amd_dcsr *dcsr_submatrix(const spasm_amd_dcsr *A, int r0, int r1, int c0, int c1, const char *who)
{
    dcsr_need(A, who);
    if (r0 < 0 || r1 < r0 || r1 > A->n || c0 < 0 || c1 < c0 || c1 > A->m) throw EngineError(std::string(who) + ": range outside the matrix");
    return spg_run(SPG_SUBMATRIX, *A, nullptr, 1, 1, r0, r1, c0, c1).release();
}

int dcsr_equal(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B, const char *who)
{
    dcsr_need(A, who);
    dcsr_need(B, who);
    if (A->dev != B->dev) throw EngineError(std::string(who) + ": the matrices live on different devices");
    if (A->n != B->n || A->m != B->m || A->F.p != B->F.p) return 0;
    std::unique_ptr<spasm_amd_dcsr> ca, cb; // canonical forms of what is not canonical yet: 1 * A
    if (!A->canonical) { ca.reset(dcsr_lincomb(1, A, 0, nullptr, who)); A = ca.get(); }
    if (!B->canonical) { cb.reset(dcsr_lincomb(1, B, 0, nullptr, who)); B = cb.get(); }
    if (A->nnz != B->nnz) return 0;
    hipStream_t s = nullptr;
    DevBuf<int> diff;
    diff.alloc(1);
    diff.zero(s);
    const i64 work = std::max<i64>(A->nnz, (i64)A->n + 1);
    hipLaunchKernelGGL(k_spg_diff, dim3((int)std::min<i64>(cdiv(work, 256), 65536)), dim3(256), 0, s, A->n, (i64d)A->nnz, A->p.p, B->p.p, A->ent.p, B->ent.p, diff.p);
    HIPCHK(hipGetLastError());
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, diff.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return h ? 0 : 1;
}

// ---- transpose, permute, vcat, hcat (reshape.hpp) ----------------------------------------------------------------------------
void rsh_launch_group(int cls, int nitems, const int *items, const i64d *Rp, int2 *ent, hipStream_t s)
{
    const size_t lds = (size_t)(cls == 2 ? 512 : (cls == 3 ? 2048 : RSH_GROUP_MAX)) * sizeof(int2);
    static bool attr_done[kMaxDev] = {false};
    bool &done = attr_done[current_device()];
    if (!done) {
        HIPCHK(hipFuncSetAttribute((const void *)k_rsh_sort_group, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)RSH_GROUP_MAX * sizeof(int2))));
        done = true;
    }
    hipLaunchKernelGGL(k_rsh_sort_group, dim3(nitems), dim3(256), lds, s, nitems, items, Rp, ent);
    HIPCHK(hipGetLastError());
}

// the long rows of the list: gathered back to back in batches, sorted by column as 64-bit words {column, value} on their low half,
// copied back.  Returns the bytes of scratch it took.
size_t rsh_sort_long(int nlong, const int *items, const i64d *Rp, int2 *ent, hipStream_t s)
{
    DevBuf<i64d> dlen;
    dlen.alloc((size_t)nlong);
    hipLaunchKernelGGL(k_rsh_long_lens, dim3(cdiv(nlong, 256)), dim3(256), 0, s, nlong, items, Rp, dlen.p);
    HIPCHK(hipGetLastError());
    std::vector<i64d> hlen((size_t)nlong);
    HIPCHK(hipMemcpyAsync(hlen.data(), dlen.p, (size_t)nlong * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const i64d batch_cap = (i64d)1 << 28;  // entries per batch (a row above it goes alone; a row holds below 2^31 entries)
    DevBuf<int2> in, out;
    DevBuf<unsigned> coff;
    DevBuf<unsigned char> tmp;
    std::vector<unsigned> hoff;
    size_t peak = 0;
    int lo = 0;
    while (lo < nlong) {
        int hi = lo;
        i64d total = 0;
        while (hi < nlong && (hi == lo || total + hlen[(size_t)hi] <= batch_cap)) total += hlen[(size_t)hi++];
        const int nb = hi - lo;
        hoff.assign((size_t)nb + 1, 0u);
        for (int t = 0; t < nb; t++) hoff[(size_t)t + 1] = hoff[(size_t)t] + (unsigned)hlen[(size_t)(lo + t)];
        in.ensure((size_t)total);
        out.ensure((size_t)total);
        coff.ensure((size_t)nb + 1);
        HIPCHK(hipMemcpyAsync(coff.p, hoff.data(), ((size_t)nb + 1) * sizeof(unsigned), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_rsh_long_copy, dim3(nb), dim3(256), 0, s, 0, items + lo, Rp, coff.p, ent, in.p);
        HIPCHK(hipGetLastError());
        size_t bytes = 0;
        HIPCHK(rocprim::segmented_radix_sort_keys(nullptr, bytes, (unsigned long long *)in.p, (unsigned long long *)out.p, (unsigned)total, (unsigned)nb, coff.p,
                                                  coff.p + 1, 0, 32, s));
        tmp.ensure(bytes);
        HIPCHK(rocprim::segmented_radix_sort_keys(tmp.p, bytes, (unsigned long long *)in.p, (unsigned long long *)out.p, (unsigned)total, (unsigned)nb, coff.p,
                                                  coff.p + 1, 0, 32, s));
        hipLaunchKernelGGL(k_rsh_long_copy, dim3(nb), dim3(256), 0, s, 1, items + lo, Rp, coff.p, ent, out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));  // (hoff is reused by the next batch)
        peak = std::max(peak, (in.n + out.n) * sizeof(int2) + tmp.n + coff.n * sizeof(unsigned) + dlen.n * sizeof(i64d));
        lo = hi;
    }
    return peak;
}

// R = op(D[0 .. count - 1]): the driver of the three steps of reshape.hpp.  The operands are canonical, on one device, over one
// prime, and their shapes fit (checked by the callers below); p and qinv are HOST arrays that have been checked, or null.
std::unique_ptr<spasm_amd_dcsr> rsh_run(int op, int count, const spasm_amd_dcsr *const *D, const int *p, const int *qinv)
{
    hipStream_t s = nullptr;
    const spasm_amd_dcsr &A = *D[0];
    std::unique_ptr<spasm_amd_dcsr> R(new spasm_amd_dcsr());
    R->dev = A.dev;
    R->F = A.F;
    R->canonical = true;
    std::vector<RshOperand> hops((size_t)count);
    i64 n = 0, m = 0, nnz = 0;
    for (int k = 0; k < count; k++) {
        hops[(size_t)k].p = D[k]->p.p;
        hops[(size_t)k].ent = D[k]->ent.p;
        hops[(size_t)k].n = D[k]->n;
        hops[(size_t)k].off = op == RSH_VCAT ? (int)n : (op == RSH_HCAT ? (int)m : 0);
        nnz += D[k]->nnz;
        if (op == RSH_VCAT) n += D[k]->n;
        if (op == RSH_HCAT) m += D[k]->m;
    }
    if (op == RSH_TRANSPOSE) { n = A.m; m = A.n; }
    if (op == RSH_PERMUTE) { n = A.n; m = A.m; }
    if (op == RSH_VCAT) m = A.m;
    if (op == RSH_HCAT) n = A.n;
    R->n = (int)n;
    R->m = (int)m;
    R->nnz = nnz;
    R->stats[10] = op;
    R->stats[5] = 1;
    const size_t n1 = (size_t)n + 1;
    R->p.alloc(n1);
    R->ent.alloc((size_t)nnz + 1);
    if (nnz == 0) {
        HIPCHK(hipMemsetAsync(R->p.p, 0, n1 * sizeof(i64d), s));
        HIPCHK(hipStreamSynchronize(s));
        return R;
    }
    SpgEvents ev;
    Scanner scan;
    DevBuf<RshOperand> ops;
    DevBuf<i64d> len;
    DevBuf<int> rowmap, colmap;
    ops.alloc((size_t)count);
    len.alloc(n1);
    HIPCHK(hipMemcpyAsync(ops.p, hops.data(), (size_t)count * sizeof(RshOperand), hipMemcpyHostToDevice, s));
    if (p) {
        rowmap.alloc((size_t)A.n);
        HIPCHK(hipMemcpyAsync(rowmap.p, p, (size_t)A.n * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (qinv) {
        colmap.alloc((size_t)A.m);
        HIPCHK(hipMemcpyAsync(colmap.p, qinv, (size_t)A.m * sizeof(int), hipMemcpyHostToDevice, s));
    }
    len.zero(s);
    RshArgs a;
    memset(&a, 0, sizeof a);
    a.op = op;
    a.nitems = op == RSH_TRANSPOSE ? A.n : (int)n;
    a.count = count;
    a.ops = ops.p;
    a.rowmap = p ? rowmap.p : nullptr;
    a.colmap = qinv ? colmap.p : nullptr;
    a.Rp = R->p.p;
    a.out = R->ent.p;
    a.cursor = (unsigned long long *)len.p;
    size_t peak = ops.n * sizeof(RshOperand) + len.n * sizeof(i64d) + (rowmap.n + colmap.n) * sizeof(int);
    // ---- count
    HIPCHK(hipEventRecord(ev.e[0], s));
    if (op == RSH_TRANSPOSE) hipLaunchKernelGGL(k_rsh_hist, dim3((int)std::min<i64>(cdiv(nnz, 256), 65536)), dim3(256), 0, s, (i64d)nnz, A.ent.p, (unsigned long long *)len.p);
    else hipLaunchKernelGGL(k_rsh_lens, dim3(cdiv(n, 256)), dim3(256), 0, s, a, (int)n, len.p);
    HIPCHK(hipGetLastError());
    scan.exclusive(len.p, R->p.p, n1, s);  // (len[n] is 0)
    // ---- move
    HIPCHK(hipEventRecord(ev.e[1], s));
    if (op == RSH_TRANSPOSE) len.zero(s);  // the counts become the cursors
    if (nnz <= 16 * (i64)a.nitems) hipLaunchKernelGGL((k_rsh_move<8>), dim3(cdiv((i64)a.nitems * 8, 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_rsh_move<64>), dim3(cdiv((i64)a.nitems * 64, 256)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    // ---- order
    HIPCHK(hipEventRecord(ev.e[2], s));
    DevBuf<unsigned char> key, key2, sort_tmp;
    DevBuf<int> rowid, rowid2, hist;
    DevBuf<i64d> maxl;
    hist.alloc(16);
    maxl.alloc(1);
    hist.zero(s);
    maxl.zero(s);
    key.alloc((size_t)n);
    rowid.alloc((size_t)n);
    hipLaunchKernelGGL(k_rsh_classify, dim3(cdiv(n, 256)), dim3(256), 0, s, (int)n, R->p.p, key.p, rowid.p, hist.p, maxl.p);
    HIPCHK(hipGetLastError());
    i64 rows_path[3] = {0, 0, 0};
    if (op == RSH_TRANSPOSE || (op == RSH_PERMUTE && qinv)) {
        key2.alloc((size_t)n);
        rowid2.alloc((size_t)n);
        size_t bytes = 0;
        HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, key.p, key2.p, rowid.p, rowid2.p, (size_t)n, 0, 4, s));
        sort_tmp.ensure(bytes);
        HIPCHK(rocprim::radix_sort_pairs(sort_tmp.p, bytes, key.p, key2.p, rowid.p, rowid2.p, (size_t)n, 0, 4, s));
        int h[16];
        HIPCHK(hipMemcpyAsync(h, hist.p, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        peak += (key2.n + key.n) + (rowid.n + rowid2.n) * sizeof(int) + sort_tmp.n;
        int first = h[0];
        if (h[1] > 0) {
            hipLaunchKernelGGL(k_rsh_sort_wave, dim3(cdiv(h[1], 4)), dim3(256), 0, s, h[1], rowid2.p + first, R->p.p, R->ent.p);
            HIPCHK(hipGetLastError());
            rows_path[0] = h[1];
        }
        first += h[1];
        for (int cls = 2; cls < RSH_CLS_LONG; cls++) {
            if (h[cls] > 0) rsh_launch_group(cls, h[cls], rowid2.p + first, R->p.p, R->ent.p, s);
            rows_path[1] += h[cls];
            first += h[cls];
        }
        if (h[RSH_CLS_LONG] > 0) {
            peak += rsh_sort_long(h[RSH_CLS_LONG], rowid2.p + first, R->p.p, R->ent.p, s);
            rows_path[2] = h[RSH_CLS_LONG];
        }
    }
    HIPCHK(hipEventRecord(ev.e[3], s));
    i64d hmax = 0;
    HIPCHK(hipMemcpyAsync(&hmax, maxl.p, sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 *st = R->stats;
    st[0] = nnz;
    st[1] = nnz;
    st[2] = rows_path[0];
    st[3] = rows_path[1];
    st[4] = rows_path[2];
    st[6] = (i64)(ev.ms(0, 1) * 1000.0);
    st[7] = (i64)(ev.ms(1, 2) * 1000.0);
    st[8] = (i64)(ev.ms(2, 3) * 1000.0);
    st[9] = (i64)peak;
    st[11] = hmax;
    return R;
}

// the operands of a structural operation: not NULL, on one device, over one prime; what is not canonical yet is brought to
// canonical form (own[] keeps those copies alive)
void rsh_operands(int count, const spasm_amd_dcsr *const *D, std::vector<const spasm_amd_dcsr *> &use, std::vector<std::unique_ptr<spasm_amd_dcsr>> &own, const char *who)
{
    const std::string w(who);
    if (count < 1) throw EngineError(w + ": at least one matrix is needed");
    if (!D) throw EngineError(w + ": NULL list of matrices");
    for (int k = 0; k < count; k++) {
        dcsr_need(D[k], who);
        if (D[k]->F.p != D[0]->F.p) throw EngineError(w + ": the matrices are over different primes");
        if (D[k]->dev != D[0]->dev) throw EngineError(w + ": the matrices live on different devices");
    }
    use.assign(D, D + count);
    for (int k = 0; k < count; k++)
        if (!use[(size_t)k]->canonical) {
            own.emplace_back(dcsr_lincomb(1, use[(size_t)k], 0, nullptr, who));
            use[(size_t)k] = own.back().get();
        }
}

// host check, O(len): map is a bijection of 0 .. len - 1
void rsh_check_permutation(const int *map, int len, const char *name, const char *who)
{
    if (!map) return;
    std::vector<unsigned char> seen((size_t)len, 0);
    for (int i = 0; i < len; i++) {
        const int v = map[i];
        if (v < 0 || v >= len || seen[(size_t)v]) {
            char b[160];
            snprintf(b, sizeof b, "%s: %s is not a permutation (%s[%d] = %d is %s)", who, name, name, i, v, (v < 0 || v >= len) ? "out of range" : "repeated");
            throw EngineError(b);
        }
        seen[(size_t)v] = 1;
    }
}

spasm_amd_dcsr *dcsr_transpose(const spasm_amd_dcsr *A, const char *who)
{
    require_device();
    std::vector<const spasm_amd_dcsr *> use;
    std::vector<std::unique_ptr<spasm_amd_dcsr>> own;
    rsh_operands(1, &A, use, own, who);
    return rsh_run(RSH_TRANSPOSE, 1, use.data(), nullptr, nullptr).release();
}

spasm_amd_dcsr *dcsr_permute(const spasm_amd_dcsr *A, const int *p, const int *qinv, const char *who)
{
    require_device();
    dcsr_need(A, who);
    rsh_check_permutation(p, A->n, "p", who);
    rsh_check_permutation(qinv, A->m, "qinv", who);
    std::vector<const spasm_amd_dcsr *> use;
    std::vector<std::unique_ptr<spasm_amd_dcsr>> own;
    rsh_operands(1, &A, use, own, who);
    return rsh_run(RSH_PERMUTE, 1, use.data(), p, qinv).release();
}

spasm_amd_dcsr *dcsr_cat(int op, int count, const spasm_amd_dcsr *const *D, const char *who)
{
    require_device();
    std::vector<const spasm_amd_dcsr *> use;
    std::vector<std::unique_ptr<spasm_amd_dcsr>> own;
    const std::string w(who);
    if (count < 1) throw EngineError(w + ": at least one matrix is needed");
    if (!D) throw EngineError(w + ": NULL list of matrices");
    i64 total = 0;
    for (int k = 0; k < count; k++) {
        dcsr_need(D[k], who);
        if (op == RSH_VCAT && D[k]->m != D[0]->m) throw EngineError(w + ": dimension mismatch (the matrices must have the same number of columns)");
        if (op == RSH_HCAT && D[k]->n != D[0]->n) throw EngineError(w + ": dimension mismatch (the matrices must have the same number of rows)");
        total += op == RSH_VCAT ? D[k]->n : D[k]->m;
    }
    if (total > 0x7fffffff) throw EngineError(w + (op == RSH_VCAT ? ": more than INT_MAX rows in all" : ": more than INT_MAX columns in all"));
    rsh_operands(count, D, use, own, who);
    return rsh_run(op, count, use.data(), nullptr, nullptr).release();
}

struct spasm_csr *csr_mul_once(const struct spasm_csr *A, const struct spasm_csr *B)
{
    require_device();
    if (!A || !B) throw EngineError("NULL matrix");
    if (A->m != B->n) throw EngineError("dimension mismatch (columns of A, rows of B)");
    if (A->field->p != B->field->p) throw EngineError("the matrices are over different primes");
    std::unique_ptr<spasm_amd_dcsr> a(dcsr_upload(A, "A"));
    std::unique_ptr<spasm_amd_dcsr> b(dcsr_upload(B, "B"));
    std::unique_ptr<spasm_amd_dcsr> c(dcsr_mul(a.get(), b.get(), "product"));
    a.reset();
    b.reset();
    return dcsr_download(c.get());
}

struct spasm_csr *csr_lincomb_once(i64 sa, const struct spasm_csr *A, i64 sb, const struct spasm_csr *B)
{
    require_device();
    if (!A) throw EngineError("NULL matrix");
    if (B && (A->n != B->n || A->m != B->m)) throw EngineError("dimension mismatch");
    if (B && A->field->p != B->field->p) throw EngineError("the matrices are over different primes");
    std::unique_ptr<spasm_amd_dcsr> a(dcsr_upload(A, "A"));
    std::unique_ptr<spasm_amd_dcsr> b(B ? dcsr_upload(B, "B") : nullptr);
    std::unique_ptr<spasm_amd_dcsr> c(dcsr_lincomb(sa, a.get(), sb, b.get(), "combination"));
    a.reset();
    b.reset();
    return dcsr_download(c.get());
}

} // namespace

// ------------------------------------------------------------------------------------------------
// Dense triangular solves x T = b (trsolve.hpp): the operator keeps T on the device in the order of its pivot graph's levels,
// cut into panels, with each panel's entries gathered by the later position they feed.
// ------------------------------------------------------------------------------------------------
namespace {

struct TrsPanel {
    int beg = 0, cnt = 0;   // positions beg .. beg + cnt - 1
    bool wide = false;      // one level of >= TRS_WIDE rows; else a chunk of <= TRS_CHUNK rows
    int nsteps = 0;         // chunk: its levels, ends at steps[step_off ..]; 1: no dependency inside, no diagonal block
    i64 step_off = 0, diag_off = 0;
    i64 desc_off = 0, nent = 0;
    int ndesc = 0;
    bool long_team = false; // push with a whole wave per descriptor
};

} // namespace

struct spasm_amd_trsolve {
    int dev = 0;
    int n = 0, m = 0, kind = 0, npart = 0, nlevels = 0, nwide = 0, nchunk = 0;
    i64 stored = 0;
    ZpField F;
    std::vector<TrsPanel> panels;
    bool res_long = false;
    DevBuf<int> pcol, pdinv, rowpos, colpos, steps, diag, dtgt, dlen;
    DevBuf<i64d> dstart, rstart;
    DevBuf<int2> gent, rent;
    DevBuf<int> acc, xs;                   // per apply: npart x kw
    DevBuf<int> hb, hx;                    // staging of the host-array applies
    DevBuf<unsigned char> hok;

    // kernels of one apply of at most 64 vectors
    i64 launches() const
    {
        i64 c = 0;
        for (const TrsPanel &P : panels) c += 1 + (P.ndesc > 0);
        return c + (m > 0) + (n > 0);
    }

    template <bool SMALL, int KW>
    void run(int kc, int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok, hipStream_t s)
    {
        constexpr int TS = spmv_short_team(KW);
        if (npart > 0) {
            acc.ensure((size_t)npart * KW);
            xs.ensure((size_t)npart * KW);
            HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)npart * KW * sizeof(int), s));
            for (const TrsPanel &P : panels) {
                if (P.wide)
                    hipLaunchKernelGGL(k_trs_wide_solve, dim3(cdiv((i64)P.cnt * kc, 256)), dim3(256), 0, s, P.beg, P.cnt, pcol.p, pdinv.p, F, KW, kc, B,
                                       (i64d)ldb, acc.p, xs.p);
                else
                    hipLaunchKernelGGL(k_trs_chunk_solve<SMALL>, dim3(1, cdiv(kc, TRS_CV)), dim3(TRS_CHUNK * TRS_CV), 0, s, P.beg, P.cnt, diag.p + P.diag_off,
                                       steps.p + P.step_off, P.nsteps, pcol.p, pdinv.p, F, KW, kc, B, (i64d)ldb, acc.p, xs.p);
                if (P.ndesc > 0) {
                    if (P.long_team)
                        hipLaunchKernelGGL((k_trs_push<SMALL, KW, 64>), dim3(cdiv((i64)P.ndesc * 64, 256)), dim3(256), 0, s, P.ndesc, dtgt.p + P.desc_off,
                                           dstart.p + P.desc_off, dlen.p + P.desc_off, gent.p, F, kc, xs.p, acc.p);
                    else
                        hipLaunchKernelGGL((k_trs_push<SMALL, KW, TS>), dim3(cdiv((i64)P.ndesc * TS, 256)), dim3(256), 0, s, P.ndesc, dtgt.p + P.desc_off,
                                           dstart.p + P.desc_off, dlen.p + P.desc_off, gent.p, F, kc, xs.p, acc.p);
                }
            }
        }
        if (m > 0) {
            if (res_long)
                hipLaunchKernelGGL((k_trs_residual<SMALL, KW, 64>), dim3(cdiv((i64)m * 64, 256)), dim3(256), 0, s, m, colpos.p, rstart.p, rent.p, F, kc, xs.p,
                                   B, (i64d)ldb, ok);
            else
                hipLaunchKernelGGL((k_trs_residual<SMALL, KW, TS>), dim3(cdiv((i64)m * TS, 256)), dim3(256), 0, s, m, colpos.p, rstart.p, rent.p, F, kc, xs.p,
                                   B, (i64d)ldb, ok);
        }
        if (n > 0) hipLaunchKernelGGL(k_trs_write_x, dim3(cdiv((i64)n * kc, 256)), dim3(256), 0, s, n, rowpos.p, KW, kc, xs.p, X, (i64d)ldx);
        HIPCHK(hipGetLastError());
    }

    // X, residual in B and ok for k right-hand sides on device arrays, enqueued on s (k > 0)
    void apply_dev(int k, int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok, hipStream_t s)
    {
        HIPCHK(hipMemsetAsync(ok, 1, (size_t)k, s));
        for (int k0 = 0; k0 < k; k0 += 64) {
            const int kc = std::min(k - k0, 64);
            dispatch_kw(spmv_kw(kc), [&](auto KW) {
                if (F.small) run<true, KW()>(kc, B + k0, ldb, X + k0, ldx, ok + k0, s);
                else run<false, KW()>(kc, B + k0, ldb, X + k0, ldx, ok + k0, s);
            });
        }
    }

    // the same on host arrays, through device copies packed with leading dimension k; B, X and ok are written only once all went well
    void apply_host(int k, int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok)
    {
        if (k == 0) return;
        hipStream_t s = nullptr;
        const size_t kk = (size_t)k;
        hb.ensure((size_t)m * kk);
        hx.ensure((size_t)n * kk);
        hok.ensure(kk);
        if (m > 0) HIPCHK(hipMemcpy2DAsync(hb.p, kk * sizeof(int), B, (size_t)ldb * sizeof(int), kk * sizeof(int), (size_t)m, hipMemcpyHostToDevice, s));
        apply_dev(k, hb.p, k, hx.p, k, hok.p, s);
        std::vector<int> ob((size_t)m * kk), ox((size_t)n * kk);
        std::vector<unsigned char> ook(kk);
        if (m > 0) HIPCHK(hipMemcpyAsync(ob.data(), hb.p, ob.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        if (n > 0) HIPCHK(hipMemcpyAsync(ox.data(), hx.p, ox.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ook.data(), hok.p, kk, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < m; i++) memcpy(B + (size_t)i * (size_t)ldb, ob.data() + (size_t)i * kk, kk * sizeof(int));
        for (int i = 0; i < n; i++) memcpy(X + (size_t)i * (size_t)ldx, ox.data() + (size_t)i * kk, kk * sizeof(int));
        memcpy(ok, ook.data(), kk);
    }
};

namespace {

// All structural checks, the levels of the pivot graph, the panels and the gathered copies, on the host; then one upload.
spasm_amd_trsolve *trsolve_create(const struct spasm_csr *T, const int *piv, int kind, const char *who)
{
    const std::string w(who);
    if (!T) throw EngineError(w + ": NULL matrix");
    if (kind != 0 && kind != 1) throw EngineError(w + ": kind must be 0 (forward, piv = q) or 1 (back, piv = p)");
    require_device();
    check_input(T, who);
    const int n = T->n, m = T->m;
    if (!piv && (kind == 0 ? n : m) > 0) throw EngineError(w + ": NULL pivot array");
    std::unique_ptr<spasm_amd_trsolve> op(new spasm_amd_trsolve());
    HIPCHK(hipGetDevice(&op->dev));
    const ZpField F = zp_field_make(T->field->p);
    op->F = F;
    op->n = n;
    op->m = m;
    op->kind = kind;
    const i64 *Tp = T->p;
    const int *Tj = T->j;
    const int *Tx = T->x;
    char msg[256];

    // pivots: c(i) and its inverse
    std::vector<int> rowcol((size_t)n, -1), colrow((size_t)m, -1);
    if (kind == 0) {
        for (int i = 0; i < n; i++) {
            const int j = piv[i];
            if (j < 0) continue;
            if (j >= m) { snprintf(msg, sizeof msg, "%s: q[%d] = %d is out of range (%d columns)", who, i, j, m); throw EngineError(msg); }
            if (colrow[(size_t)j] >= 0) { snprintf(msg, sizeof msg, "%s: column %d is the pivot of rows %d and %d", who, j, colrow[(size_t)j], i); throw EngineError(msg); }
            colrow[(size_t)j] = i;
            rowcol[(size_t)i] = j;
        }
    } else {
        for (int j = 0; j < m; j++) {
            const int i = piv[j];
            if (i < 0) continue;
            if (i >= n) { snprintf(msg, sizeof msg, "%s: p[%d] = %d is out of range (%d rows)", who, j, i, n); throw EngineError(msg); }
            if (rowcol[(size_t)i] >= 0) { snprintf(msg, sizeof msg, "%s: row %d holds the pivots of columns %d and %d", who, i, rowcol[(size_t)i], j); throw EngineError(msg); }
            rowcol[(size_t)i] = j;
            colrow[(size_t)j] = i;
        }
    }

    // diagonals and in-degrees of the pivot graph (edge i -> k: row i has an entry on c(k), k != i)
    std::vector<int> dg((size_t)n, 0), indeg((size_t)n, 0);
    int badcol = -1;
#pragma omp parallel for schedule(dynamic, 1024)
    for (int i = 0; i < n; i++) {
        if (rowcol[(size_t)i] < 0) continue;
        int64_t d = 0;
        for (i64 e = Tp[i]; e < Tp[i + 1]; e++) {
            const int j = Tj[e];
            if (j < 0 || j >= m) {
#pragma omp atomic write
                badcol = i;
                continue;
            }
            const int k = colrow[(size_t)j];
            // reduced entry by entry: T is the caller's (raw ints, repeated entries are summed), and a sum of raw values can leave
            // the domain of zp_reduce (a row of p = 3 that repeats its diagonal 3 * 2^20 * p times); this one stays below 2^30 p
            if (k == i) d += zp_reduce(F, (int64_t)Tx[e]);
            else if (k >= 0) {
#pragma omp atomic
                indeg[(size_t)k]++;
            }
        }
        dg[(size_t)i] = zp_reduce(F, d);
    }
    if (badcol >= 0) { snprintf(msg, sizeof msg, "%s: row %d has a column index out of range", who, badcol); throw EngineError(msg); }
    int npart = 0;
    for (int i = 0; i < n; i++) {
        if (rowcol[(size_t)i] < 0) continue;
        npart++;
        if (kind == 0 && dg[(size_t)i] != 1) {
            snprintf(msg, sizeof msg, "%s: the pivot of row %d (column %d) is %d, not 1", who, i, rowcol[(size_t)i], dg[(size_t)i]);
            throw EngineError(msg);
        }
        if (kind == 1 && dg[(size_t)i] == 0) {
            snprintf(msg, sizeof msg, "%s: the diagonal entry of row %d (column %d) is zero", who, i, rowcol[(size_t)i]);
            throw EngineError(msg);
        }
    }
    op->npart = npart;

    // levels, frontier by frontier (Kahn): the positions are the rows in level order, by row inside a level
    std::vector<int> order, lvl_end;
    order.reserve((size_t)npart);
    for (int i = 0; i < n; i++)
        if (rowcol[(size_t)i] >= 0 && indeg[(size_t)i] == 0) order.push_back(i);
    size_t head = 0;
    while (head < order.size()) {
        const size_t end = order.size();
        lvl_end.push_back((int)end);
        for (size_t q = head; q < end; q++) {
            const int i = order[q];
            for (i64 e = Tp[i]; e < Tp[i + 1]; e++) {
                const int k = colrow[(size_t)Tj[e]];
                if (k >= 0 && k != i && --indeg[(size_t)k] == 0) order.push_back(k);
            }
        }
        std::sort(order.begin() + (i64)end, order.end());
        head = end;
    }
    if ((int)order.size() != npart) {
        int on = -1;
        for (int i = 0; i < n && on < 0; i++)
            if (rowcol[(size_t)i] >= 0 && indeg[(size_t)i] > 0) on = i;
        snprintf(msg, sizeof msg, "%s: the pivot graph has a cycle (row %d waits on itself through other rows)", who, on);
        throw EngineError(msg);
    }
    op->nlevels = (int)lvl_end.size();

    // panels: a wide level alone, narrower levels in chunks of at most TRS_CHUNK positions (a level may straddle two chunks)
    std::vector<int> hsteps;
    {
        TrsPanel cur;
        auto close = [&]() {
            if (cur.cnt == 0) return;
            cur.step_off = (i64)hsteps.size() - cur.nsteps;
            op->panels.push_back(cur);
            op->nchunk++;
            cur = TrsPanel();
        };
        int lb = 0;
        for (int le : lvl_end) {
            if (le - lb >= TRS_WIDE) {
                close();
                TrsPanel P;
                P.beg = lb;
                P.cnt = le - lb;
                P.wide = true;
                op->panels.push_back(P);
                op->nwide++;
            } else {
                for (int q = lb; q < le;) {
                    if (cur.cnt == 0) cur.beg = q;
                    const int take = std::min(le - q, TRS_CHUNK - cur.cnt);
                    cur.cnt += take;
                    cur.nsteps++;
                    hsteps.push_back(cur.cnt);
                    q += take;
                    if (cur.cnt == TRS_CHUNK) close();
                }
            }
            lb = le;
        }
        close();
    }
    const int npan = (int)op->panels.size();
    std::vector<int> pos_of((size_t)n, -1), panel_of((size_t)npart, 0), hpcol((size_t)npart), hdinv((size_t)npart);
    for (int a = 0; a < npart; a++) {
        const int i = order[(size_t)a];
        pos_of[(size_t)i] = a;
        hpcol[(size_t)a] = rowcol[(size_t)i];
        hdinv[(size_t)a] = kind == 0 ? 1 : zp_inverse(F, dg[(size_t)i]);
    }
    i64 ndiag = 0;
    for (int P = 0; P < npan; P++) {
        TrsPanel &Q = op->panels[(size_t)P];
        for (int a = Q.beg; a < Q.beg + Q.cnt; a++) panel_of[(size_t)a] = P;
        if (!Q.wide && Q.nsteps > 1) {
            Q.diag_off = ndiag;
            ndiag += (i64)Q.cnt * Q.cnt;
        }
    }

    // gathered copies.  Entries of row pos a on column j: no pivot on j -> the residual's column j; the own pivot -> (the diagonal);
    // the pivot of a position t of the same chunk -> its diagonal block; of a later panel -> the push of a's panel, target t.
    std::vector<i64> rcnt((size_t)m + 1, 0);
    std::vector<i64> pent((size_t)npan, 0);
    std::vector<int> pdesc((size_t)npan, 0);
#pragma omp parallel
    {
        std::vector<int> cnt((size_t)npart, 0), touched;
#pragma omp for schedule(dynamic, 1)
        for (int P = 0; P < npan; P++) {
            const TrsPanel &Q = op->panels[(size_t)P];
            i64 ne = 0;
            touched.clear();
            for (int a = Q.beg; a < Q.beg + Q.cnt; a++) {
                const int i = order[(size_t)a];
                for (i64 e = Tp[i]; e < Tp[i + 1]; e++) {
                    const int j = Tj[e];
                    const int k = colrow[(size_t)j];
                    if (k < 0) {
#pragma omp atomic
                        rcnt[(size_t)j + 1]++;
                    } else if (k != i) {
                        const int t = pos_of[(size_t)k];
                        if (panel_of[(size_t)t] == P) continue;
                        ne++;
                        if (cnt[(size_t)t]++ == 0) touched.push_back(t);
                    }
                }
            }
            for (int t : touched) cnt[(size_t)t] = 0;
            pent[(size_t)P] = ne;
            pdesc[(size_t)P] = (int)touched.size();
        }
    }
    i64 nent = 0, ndesc = 0;
    for (int P = 0; P < npan; P++) {
        TrsPanel &Q = op->panels[(size_t)P];
        Q.desc_off = ndesc;
        Q.ndesc = pdesc[(size_t)P];
        Q.nent = pent[(size_t)P];
        Q.long_team = Q.ndesc > 0 && Q.nent > (i64)32 * Q.ndesc;
        ndesc += Q.ndesc;
        nent += Q.nent;
    }
    for (int j = 0; j < m; j++) rcnt[(size_t)j + 1] += rcnt[(size_t)j];
    const i64 nres = m > 0 ? rcnt[(size_t)m] : 0;
    op->res_long = m > 0 && nres > (i64)32 * m;
    std::vector<int2> hgent((size_t)std::max<i64>(nent, 1)), hrent((size_t)std::max<i64>(nres, 1));
    std::vector<int> hdtgt((size_t)std::max<i64>(ndesc, 1)), hdlen((size_t)std::max<i64>(ndesc, 1)), hdiag((size_t)std::max<i64>(ndiag, 1), 0);
    std::vector<i64d> hdstart((size_t)std::max<i64>(ndesc, 1));
    std::vector<i64> rcur(rcnt.begin(), rcnt.end());
    i64 eoff = 0;
    std::vector<i64> pent_off((size_t)npan, 0);
    for (int P = 0; P < npan; P++) {
        pent_off[(size_t)P] = eoff;
        eoff += op->panels[(size_t)P].nent;
    }
#pragma omp parallel
    {
        std::vector<int> cnt((size_t)npart, 0), touched;
        std::vector<i64> cur;
#pragma omp for schedule(dynamic, 1)
        for (int P = 0; P < npan; P++) {
            const TrsPanel &Q = op->panels[(size_t)P];
            touched.clear();
            for (int a = Q.beg; a < Q.beg + Q.cnt; a++) {
                const int i = order[(size_t)a];
                for (i64 e = Tp[i]; e < Tp[i + 1]; e++) {
                    const int k = colrow[(size_t)Tj[e]];
                    if (k < 0 || k == i) continue;
                    const int t = pos_of[(size_t)k];
                    if (panel_of[(size_t)t] == P) continue;
                    if (cnt[(size_t)t]++ == 0) touched.push_back(t);
                }
            }
            std::sort(touched.begin(), touched.end());
            // descriptors in target order; cnt[t] becomes the fill cursor of target t
            i64 o = pent_off[(size_t)P];
            for (size_t q = 0; q < touched.size(); q++) {
                const int t = touched[q];
                const size_t d = (size_t)(Q.desc_off + (i64)q);
                hdtgt[d] = t;
                hdstart[d] = o;
                hdlen[d] = cnt[(size_t)t];
                o += cnt[(size_t)t];
                cnt[(size_t)t] = (int)q;
            }
            cur.assign(touched.size(), 0);
            for (int a = Q.beg; a < Q.beg + Q.cnt; a++) {
                const int i = order[(size_t)a];
                for (i64 e = Tp[i]; e < Tp[i + 1]; e++) {
                    const int j = Tj[e];
                    const int k = colrow[(size_t)j];
                    const int v = zp_reduce(F, (int64_t)Tx[e]);
                    if (k < 0) {
                        i64 slot;
#pragma omp atomic capture
                        slot = rcur[(size_t)j]++;
                        hrent[(size_t)slot] = make_int2(a, v);
                    } else if (k != i) {
                        const int t = pos_of[(size_t)k];
                        if (panel_of[(size_t)t] == P) {
                            if (Q.nsteps > 1) {
                                int &dd = hdiag[(size_t)(Q.diag_off + (i64)(a - Q.beg) * Q.cnt + (t - Q.beg))];
                                dd = zp_add(F, dd, v);
                            }
                            continue;
                        }
                        const int q = cnt[(size_t)t];
                        const size_t d = (size_t)(Q.desc_off + (i64)q);
                        hgent[(size_t)(hdstart[d] + cur[(size_t)q]++)] = make_int2(a, v);
                    }
                }
            }
            for (int t : touched) cnt[(size_t)t] = 0;
        }
    }
    op->stored = nent + nres + ndiag;

    hipStream_t s = nullptr;
    auto up = [&](auto &d, const auto &h) {
        d.alloc(h.size());
        if (!h.empty()) HIPCHK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice, s));
    };
    std::vector<int> hcolpos((size_t)m, -1);
    for (int a = 0; a < npart; a++) hcolpos[(size_t)hpcol[(size_t)a]] = a;
    std::vector<i64d> hrstart(rcnt.begin(), rcnt.end());
    up(op->pcol, hpcol);
    up(op->pdinv, hdinv);
    up(op->rowpos, pos_of);
    up(op->colpos, hcolpos);
    up(op->steps, hsteps);
    up(op->diag, hdiag);
    up(op->dtgt, hdtgt);
    up(op->dlen, hdlen);
    up(op->dstart, hdstart);
    up(op->rstart, hrstart);
    up(op->gent, hgent);
    up(op->rent, hrent);
    HIPCHK(hipStreamSynchronize(s)); // the host vectors go out of scope
    return op.release();
}

void trsolve_check(const spasm_amd_trsolve *op, int k, const void *B, i64 ldb, const void *X, i64 ldx, const void *ok, const char *who)
{
    if (!op) throw EngineError(std::string(who) + ": NULL operator");
    if (k < 0 || ldb < k || ldx < k) throw EngineError(std::string(who) + ": bad arguments (k >= 0, ldb >= k, ldx >= k)");
    if (k > 0 && ((op->m > 0 && !B) || (op->n > 0 && !X) || !ok)) throw EngineError(std::string(who) + ": NULL array");
}

// spasm_dense_forward_solve / spasm_dense_back_solve (`who`): a temporary operator, one right-hand side
bool trsolve_once(const struct spasm_csr *T, spasm_ZZp *b, spasm_ZZp *x, const int *piv, int kind, const char *who)
{
    return abi_call(who, false, [&] {
        std::unique_ptr<spasm_amd_trsolve> op(trsolve_create(T, piv, kind, who));
        unsigned char ok = 0;
        trsolve_check(op.get(), 1, b, 1, x, 1, &ok, who);
        op->apply_host(1, b, 1, x, 1, &ok);
        return ok != 0;
    }, ABI_NAMED_BELOW);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// Many small matrices in one call (batch.hpp): every matrix whose dense image fits LDS is eliminated by one workgroup; the others,
// and every matrix of a call that asks for L, go through do_echelonize / do_kernel one at a time.  batch_run stages host matrices
// (one upload of the concatenated row pointers, columns, values) and hands over to batch_fast, which starts from the descriptors
// and is shared with the blocks of a split matrix that lie on the device already (blocks.hpp); per chunk of matrices whose
// scratch fits the budget: at most BATCH_NCLASS elimination launches, one scan, one pack, the 8-byte read of the chunk's
// entry count and one download.
//
// The first part of the section is the driver that the solve (solve_batch.hpp, further down) shares: the check and the staging of
// host matrices, the launch of a list of jobs class by class, the cut into chunks and the scan that ends a chunk's eliminations.
// ------------------------------------------------------------------------------------------------
namespace {

thread_local i64 g_batch_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

struct BatchClass { int cap, bs; };
// image words -> threads: small images get small workgroups and several of them per CU (LDS per workgroup: 5, 18, 53, 147 KiB)
constexpr BatchClass kBatchClass[BATCH_NCLASS] = {{1024, 64}, {4096, 128}, {12288, 256}, {BATCH_PAD_CAP, 512}};

void batch_layout(int cls, int &bw, int &rmax)
{
    const int lim = std::min(kBatchClass[cls].cap, BATCH_LIMIT);
    bw = lim / 32;
    rmax = 1; // min(n, m) <= sqrt(n * m) < rmax
    while ((i64)rmax * rmax <= lim) rmax++;
}

// the checks of a host matrix that need no device; NULL when it is well formed
const char *batch_check(const struct spasm_csr *M)
{
    if (!M) return "NULL matrix";
    if (M->field->p <= 2 || M->field->p > 0xfffffffbLL) return "prime out of range (2 < p <= 0xfffffffb)";
    if (M->n < 0 || M->m < 0 || !M->p || M->p[0] != 0) return "malformed matrix";
    if (!M->x) return "matrix without values (x == NULL)";
    for (int t = 0; t < M->n; t++)
        if (M->p[t + 1] < M->p[t]) return "row pointers must not decrease";
    const i64 nz = M->p[M->n];
    if (nz > 0 && !M->j) return "malformed matrix";
    const unsigned um = (unsigned)M->m;
    for (i64 k = 0; k < nz; k++)
        if ((unsigned)M->j[k] >= um) return "a column index lies outside the matrix";
    return nullptr;
}

// batch_check of matrix i of a list, and of a whole list in order
void batch_check_at(int i, const struct spasm_csr *M)
{
    const char *bad = batch_check(M);
    if (!bad) return;
    char msg[160];
    snprintf(msg, sizeof msg, "matrix %d: %s", i, bad);
    throw EngineError(msg);
}

void batch_check_list(int count, const struct spasm_csr *const *A)
{
    for (int i = 0; i < count; i++) batch_check_at(i, A[i]);
}

// i >= 0: matrix i of a list; i < 0: the one matrix, operator or handle of the call
void require_square(int i, int n, int m)
{
    if (n == m) return;
    char msg[96];
    if (i >= 0) snprintf(msg, sizeof msg, "matrix %d: not square (%d x %d)", i, n, m);
    else snprintf(msg, sizeof msg, "not square (%d x %d)", n, m);
    throw EngineError(msg);
}

inline size_t batch_align(size_t x) { return (x + 15) & ~(size_t)15; }

// host matrices on the device as one concatenated CSR: row pointers (global entry offsets) | columns | values in one buffer;
// row0[f] = where the n + 1 pointers of list[f] start in P
struct BatchStaged {
    DevBuf<unsigned char> buf;
    const i64d *P = nullptr;
    const int *J = nullptr, *X = nullptr;
    std::vector<i64> row0;
};

void batch_stage(const std::vector<const struct spasm_csr *> &list, BatchStaged &out)
{
    i64 rows_total = 0, nnz_total = 0;
    out.row0.assign(list.size(), 0);
    for (size_t f = 0; f < list.size(); f++) {
        out.row0[f] = rows_total;
        rows_total += (i64)list[f]->n + 1;
        nnz_total += list[f]->p[list[f]->n];
    }
    const size_t o_j = batch_align((size_t)rows_total * sizeof(i64d));
    const size_t o_x = batch_align(o_j + (size_t)nnz_total * sizeof(int));
    const size_t in_bytes = batch_align(o_x + (size_t)nnz_total * sizeof(int));
    std::vector<unsigned char> stage(in_bytes);
    i64d *P = (i64d *)stage.data();
    int *J = (int *)(stage.data() + o_j), *X = (int *)(stage.data() + o_x);
    i64 e0 = 0, r0 = 0;
    for (const struct spasm_csr *M : list) {
        const i64 nz = M->p[M->n];
        for (int t = 0; t <= M->n; t++) P[r0 + t] = (i64d)(e0 + M->p[t]);
        if (nz > 0) {
            memcpy(J + e0, M->j, (size_t)nz * sizeof(int));
            memcpy(X + e0, M->x, (size_t)nz * sizeof(int));
        }
        r0 += (i64)M->n + 1;
        e0 += nz;
    }
    out.buf.alloc(in_bytes);
    HIPCHK(hipMemcpy(out.buf.p, stage.data(), in_bytes, hipMemcpyHostToDevice)); // (blocking: stage ends with this scope)
    out.P = (const i64d *)out.buf.p;
    out.J = (const int *)(out.buf.p + o_j);
    out.X = (const int *)(out.buf.p + o_x);
}

// A matrix of the LDS path as the descriptors need it: its shape, its prime, and where its n + 1 row pointers start in P.
struct BatchItem { int n, m; i64 row0; i64 prime; };

// the matrices A[i], i in pick, staged in that order; returns what describes them
std::vector<BatchItem> batch_stage_items(const struct spasm_csr *const *A, const std::vector<int> &pick, BatchStaged &in)
{
    std::vector<const struct spasm_csr *> list;
    for (int i : pick) list.push_back(A[i]);
    batch_stage(list, in);
    std::vector<BatchItem> item;
    for (size_t f = 0; f < list.size(); f++) item.push_back(BatchItem{list[f]->n, list[f]->m, in.row0[f], list[f]->field->p});
    return item;
}

// The descriptor of an item as every kernel over the batch's image reads it (n, m, ld, F, row0; the rest zero), and its class.
// Here and nowhere else: the row stride (batch.hpp, "Row stride") and the smallest class that holds the padded image.
int batch_describe(const BatchItem &M, BatchDesc &d)
{
    memset(&d, 0, sizeof d);
    d.n = M.n;
    d.m = M.m;
    d.ld = (M.m % 2 == 0 && (i64)M.n * (M.m + 1) <= BATCH_PAD_CAP) ? M.m + 1 : M.m;
    d.F = zp_field_make(M.prime);
    d.row0 = M.row0;
    const i64 key = std::max<i64>((i64)d.n * d.ld, std::max(d.n, d.m));
    int c = 0;
    while (key > kBatchClass[c].cap) c++;
    return c;
}

// The kernels of a path, one per class: k[c] is the instance for kBatchClass[c].bs threads.  Every Args carries items and the LDS
// layout (cap, bw, rmax), which the launcher fills in.  attr_done: the classes of THIS table whose dynamic-LDS attribute is set,
// per device; two tables over one Args type each keep their own.
template <class Args> struct ElimKernels {
    void (*k[BATCH_NCLASS])(Args);
    mutable bool attr_done[kMaxDev][BATCH_NCLASS] = {};
};
const ElimKernels<BatchArgs> kBatchElim = {{k_batch_elim<64>, k_batch_elim<128>, k_batch_elim<256>, k_batch_elim<512>}};
const ElimKernels<SolveBatchArgs> kSolveElim = {{k_solve_elim<64>, k_solve_elim<128>, k_solve_elim<256>, k_solve_elim<512>}};

// one class of jobs; the dynamic-LDS attribute of a kernel is set once per device
template <class Args> void batch_launch_class(const ElimKernels<Args> &kern, int cls, Args a, const int *items, int nitems, hipStream_t s)
{
    a.items = items;
    a.cap = kBatchClass[cls].cap;
    batch_layout(cls, a.bw, a.rmax);
    const size_t lds = (size_t)batch_lds_words(a.cap, a.bw, a.rmax) * sizeof(int);
    bool &done = kern.attr_done[current_device()][cls];
    if (!done) {
        HIPCHK(hipFuncSetAttribute((const void *)kern.k[cls], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    void *args[] = {&a};
    HIPCHK(hipLaunchKernel((const void *)kern.k[cls], dim3(nitems), dim3(kBatchClass[cls].bs), args, lds, s));
}

// Jobs lo .. hi - 1 by class (a stable counting sort into items[lo .. hi), which must live until the stream has passed the
// upload), the items to the device, one launch per class that occurs.  `started`, when given, is recorded between the upload and
// the first launch.  Returns the launches.
template <class Args>
int batch_launch_jobs(const ElimKernels<Args> &kern, const std::vector<unsigned char> &cls, int lo, int hi, std::vector<int> &items, int *d_items, const Args &a,
                      hipEvent_t started, hipStream_t s)
{
    int hist[BATCH_NCLASS] = {0, 0, 0, 0}, at[BATCH_NCLASS], sum = lo, launches = 0;
    for (int q = lo; q < hi; q++) hist[cls[(size_t)q]]++;
    for (int k = 0; k < BATCH_NCLASS; k++) { at[k] = sum; sum += hist[k]; }
    for (int q = lo; q < hi; q++) items[(size_t)at[cls[(size_t)q]]++] = q;
    HIPCHK(hipMemcpyAsync(d_items + lo, items.data() + lo, (size_t)(hi - lo) * sizeof(int), hipMemcpyHostToDevice, s));
    if (started) HIPCHK(hipEventRecord(started, s));
    int first = lo;
    for (int k = 0; k < BATCH_NCLASS; k++) {
        if (hist[k] > 0) { batch_launch_class(kern, k, a, d_items + first, hist[k], s); launches++; }
        first += hist[k];
    }
    return launches;
}

// One word per item (a rank, a determinant): the descriptors up, the launches of `kern` between two events, out[f] = the word
// the workgroup of item f left in BatchArgs::rank, one synchronize.  Returns the launches and the device time between the events.
struct BatchTimed { int launches; double ms; };
BatchTimed batch_one_word(const ElimKernels<BatchArgs> &kern, const std::vector<BatchDesc> &desc, const std::vector<unsigned char> &cls, const i64d *dP, const int *dJ,
                          const int *dX, int *out)
{
    const int nf = (int)desc.size();
    hipStream_t s = nullptr;
    DevBuf<BatchDesc> d_desc;
    DevBuf<int> d_items, d_word;
    d_desc.alloc((size_t)nf);
    d_items.alloc((size_t)nf);
    d_word.alloc((size_t)nf);
    HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nf * sizeof(BatchDesc), hipMemcpyHostToDevice, s));
    std::vector<int> items((size_t)nf);
    BatchArgs a;
    memset(&a, 0, sizeof a);
    a.desc = d_desc.p;
    a.P = dP;
    a.J = dJ;
    a.X = dX;
    a.mode = BATCH_RANK;
    a.rank = d_word.p;
    SpgEvents ev;
    const int launches = batch_launch_jobs(kern, cls, 0, nf, items, d_items.p, a, ev.e[0], s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    HIPCHK(hipMemcpyAsync(out, d_word.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BatchTimed{launches, ev.ms(0, 1)};
}

// bytes of device buffers one chunk may use: a third of the free device memory (SPASM_AMD_BATCH_SCRATCH_MB: a smaller figure, for
// the tests of the chunked path; read once per call)
size_t batch_budget()
{
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    size_t b = fr / 3;
    const char *e = getenv("SPASM_AMD_BATCH_SCRATCH_MB");
    if (e && atof(e) > 0) b = std::min(b, (size_t)(atof(e) * 1048576.0));
    return b;
}

// chunks of consecutive jobs whose needs (bytes, need(q)) fit the budget together; a job over the budget is a chunk of its own.
// Chunk c = jobs cut[c] .. cut[c + 1] - 1.
template <class Need> std::vector<int> batch_cut(int njobs, size_t budget, Need need)
{
    std::vector<int> cut(1, 0);
    size_t used = 0;
    for (int q = 0; q < njobs; q++) {
        const size_t bytes = need(q);
        if (used > 0 && used + bytes > budget) { cut.push_back(q); used = 0; }
        used += bytes;
    }
    cut.push_back(njobs);
    return cut;
}

// The end of a chunk's eliminations: rowstart[0 .. slots] = exclusive scan of the row counts cnt[0 .. slots] (cnt[slots] is the
// scan's sentinel, which the caller has zeroed before the timed span).  Returns the entries of the chunk, read back from
// rowstart[slots]; they must fit the slices (ents).
i64 batch_chunk_entries(const int *cnt, i64 slots, i64 ents, DevBuf<i64d> &rowstart, Scanner &scan, hipStream_t s)
{
    rowstart.ensure((size_t)slots + 1);
    scan.exclusive(cnt, rowstart.p, (size_t)slots + 1, s);
    i64d total = 0;
    HIPCHK(hipMemcpyAsync(&total, rowstart.p + slots, sizeof total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total < 0 || total > ents) throw EngineError("internal error: a chunk wrote more entries than its slices hold");
    return total;
}

// nrows x m matrix from the lengths of its rows and the packed entries ent[at ..] (of which there are `total`); advances at
struct spasm_csr *batch_rows_to_csr(int nrows, int m, i64 prime, const int *len, const int2 *ent, i64 total, i64 &at)
{
    i64 nz = 0;
    for (int k = 0; k < nrows; k++) nz += len[k];
    if (at + nz > total) throw EngineError("internal error: row counts and entry count disagree");
    struct spasm_csr *R = spasm_csr_alloc(nrows, m, nz, prime, true);
    if (!R) throw EngineError("out of host memory");
    R->p[0] = 0;
    for (int k = 0; k < nrows; k++) R->p[k + 1] = R->p[k] + len[k];
    for (i64 e = 0; e < nz; e++) { R->j[e] = ent[at + e].x; R->x[e] = ent[at + e].y; }
    at += nz;
    return R;
}

// most entries of the output of an n x m matrix: U of rank r has r rows of at most m - r + 1 entries, K has m - r rows of at most
// r + 1, r <= min(n, m); both products peak where the factors meet
i64 batch_entry_cap(int mode, int n, int m)
{
    const i64 rm = std::min(n, m);
    if (mode == BATCH_LU) {
        const i64 r = std::min<i64>(rm, (m + 1) / 2);
        return r * (m - r + 1);
    }
    const i64 r = std::min<i64>(rm, m / 2);
    return (m - r) * (r + 1);
}

// what a call returns, owned until it is handed over: lu (BATCH_LU) or K (BATCH_KERNEL) per matrix, and every rank
struct BatchResults {
    std::vector<struct spasm_lu *> lu;
    std::vector<struct spasm_csr *> K;
    std::vector<i64> ranks;
    BatchResults(int mode, int count) : lu(mode == BATCH_LU ? (size_t)count : 0, nullptr), K(mode == BATCH_KERNEL ? (size_t)count : 0, nullptr), ranks((size_t)count, 0) {}
    ~BatchResults()
    {
        for (auto *x : lu) spasm_lu_free(x);
        for (auto *x : K) spasm_csr_free(x);
    }
    // to the caller's array of the mode, all at once
    void hand_over(int mode, struct spasm_lu **lu_out, struct spasm_csr **k_out, i64 *rank_out)
    {
        if (mode == BATCH_LU) { memcpy(lu_out, lu.data(), sizeof(struct spasm_lu *) * lu.size()); lu.clear(); }
        else if (mode == BATCH_KERNEL) { memcpy(k_out, K.data(), sizeof(struct spasm_csr *) * K.size()); K.clear(); }
        else memcpy(rank_out, ranks.data(), sizeof(i64) * ranks.size());
    }
};

// The LDS path from the descriptors on.  fast[f] = place, in the call's list, of the f-th matrix; item[f] describes it; P, J, X: the
// concatenated CSR on the device (P holds global entry offsets).  Results go to res at fast[f]; g_batch_stats[3 .. 7] are filled.
void batch_fast(int mode, const std::vector<int> &fast, const std::vector<BatchItem> &item, const i64d *dP, const int *dJ, const int *dX, BatchResults &res)
{
    i64 *st = g_batch_stats;
    const int nf = (int)fast.size();
    if (nf == 0) return;
    hipStream_t s = nullptr;
    const size_t budget = batch_budget();
    // ---- descriptors, classes, chunks
    std::vector<BatchDesc> desc((size_t)nf);
    std::vector<unsigned char> cls((size_t)nf);
    std::vector<i64> ecap((size_t)nf), recw((size_t)nf);
    for (int f = 0; f < nf; f++) {
        BatchDesc &d = desc[(size_t)f];
        cls[(size_t)f] = (unsigned char)batch_describe(item[(size_t)f], d);
        d.nslots = mode == BATCH_LU ? std::min(d.n, d.m) : d.m;
        ecap[(size_t)f] = mode == BATCH_RANK ? 0 : batch_entry_cap(mode, d.n, d.m);
        recw[(size_t)f] = mode == BATCH_LU ? ((2 + (i64)d.m + d.n + 1) & ~(i64)1) : 2;
        st[7] = std::max<i64>(st[7], (i64)d.n * d.ld);
    }
    // per matrix: scratch + packed entries, record, row counts and their scan; the ranks alone need none of them
    const std::vector<int> cut = batch_cut(nf, budget, [&](int f) {
        return mode == BATCH_RANK ? (size_t)0 : (size_t)ecap[(size_t)f] * 2 * sizeof(int2) + (size_t)recw[(size_t)f] * sizeof(int) + (size_t)desc[(size_t)f].nslots * (sizeof(int) + sizeof(i64d));
    });
    const int nchunks = (int)cut.size() - 1;
    // slots, records and slices of a chunk, laid out in batch order
    struct ChunkPlan { i64 slots, recs, ents; };
    std::vector<ChunkPlan> plan((size_t)nchunks, ChunkPlan{0, 0, 0});
    for (int c = 0; c < nchunks; c++) {
        ChunkPlan &pl = plan[(size_t)c];
        for (int f = cut[(size_t)c]; f < cut[(size_t)c + 1]; f++) {
            BatchDesc &d = desc[(size_t)f];
            d.slot0 = pl.slots;
            d.rec = pl.recs;
            d.slice = pl.ents;
            pl.slots += d.nslots;
            pl.recs += recw[(size_t)f];
            pl.ents += ecap[(size_t)f];
        }
    }
    i64 launches = 0, entries = 0;
    double ms = 0;

    if (mode == BATCH_RANK) {
        std::vector<int> hr((size_t)nf);
        const BatchTimed t = batch_one_word(kBatchElim, desc, cls, dP, dJ, dX, hr.data());
        launches += t.launches;
        ms += t.ms;
        for (int f = 0; f < nf; f++) res.ranks[(size_t)fast[(size_t)f]] = hr[(size_t)f];
    } else {
        // ---- descriptors to the device (the row pointers, columns and values are there already)
        DevBuf<BatchDesc> d_desc;
        DevBuf<int> d_items;
        d_desc.alloc((size_t)nf);
        d_items.alloc((size_t)nf);
        HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nf * sizeof(BatchDesc), hipMemcpyHostToDevice, s));
        std::vector<int> items((size_t)nf);
        BatchArgs a;
        memset(&a, 0, sizeof a);
        a.desc = d_desc.p;
        a.P = dP;
        a.J = dJ;
        a.X = dX;
        a.mode = mode;
        SpgEvents ev;
        DevBuf<int2> scratch;
        DevBuf<unsigned char> out;
        DevBuf<i64d> rowstart;
        Scanner scan;
        std::vector<unsigned char> host;
        for (int c = 0; c < nchunks; c++) {
            const ChunkPlan &pl = plan[(size_t)c];
            const int lo = cut[(size_t)c], hi = cut[(size_t)c + 1];
            // the chunk's output buffer: row counts (+ 1 for the scan) | records | packed entries
            const size_t o_rec = batch_align((size_t)(pl.slots + 1) * sizeof(int));
            const size_t o_ent = batch_align(o_rec + (size_t)pl.recs * sizeof(int));
            scratch.ensure((size_t)pl.ents + 1);
            out.ensure(o_ent + (size_t)pl.ents * sizeof(int2) + 16);
            a.cnt = (int *)out.p;
            a.rec = (int *)(out.p + o_rec);
            a.scratch = scratch.p;
            HIPCHK(hipMemsetAsync(a.cnt + pl.slots, 0, sizeof(int), s));
            launches += batch_launch_jobs(kBatchElim, cls, lo, hi, items, d_items.p, a, ev.e[0], s);
            const i64 total = batch_chunk_entries(a.cnt, pl.slots, pl.ents, rowstart, scan, s);
            launches++;
            if (total > 0) {
                hipLaunchKernelGGL(k_batch_pack, dim3(hi - lo), dim3(64), 0, s, a.desc, (const int *)d_items.p + lo, mode, (const int *)a.rec, (const int *)a.cnt,
                                   (const i64d *)rowstart.p, (const int2 *)scratch.p, (int2 *)(out.p + o_ent));
                HIPCHK(hipGetLastError());
                launches++;
            }
            HIPCHK(hipEventRecord(ev.e[1], s));
            const size_t out_bytes = o_ent + (size_t)total * sizeof(int2);
            if (host.size() < out_bytes) host.resize(out_bytes);
            HIPCHK(hipMemcpyAsync(host.data(), out.p, out_bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            ms += ev.ms(0, 1);
            entries += total;
            // ---- the chunk's results, in the order of its slices
            const int *h_cnt = (const int *)host.data();
            const int *h_rec = (const int *)(host.data() + o_rec);
            const int2 *h_ent = (const int2 *)(host.data() + o_ent);
            i64 at = 0;
            for (int f = lo; f < hi; f++) {
                const int i = fast[(size_t)f];
                const BatchDesc &d = desc[(size_t)f];
                const int *rec = h_rec + d.rec;
                const int r = rec[0], n = d.n, m = d.m;
                if (r < 0 || r > std::min(n, m)) throw EngineError("internal error: rank outside its bounds");
                struct spasm_csr *R = batch_rows_to_csr(mode == BATCH_LU ? r : m - r, m, d.F.p, h_cnt + d.slot0, h_ent, total, at);
                res.ranks[(size_t)i] = r;
                if (mode == BATCH_KERNEL) { res.K[(size_t)i] = R; continue; }
                struct spasm_lu *N = (struct spasm_lu *)malloc(sizeof *N);
                const int plen = std::max(std::max(n, m), 1);
                int *qinv = (int *)malloc(sizeof(int) * (size_t)std::max(m, 1));
                int *p = (int *)malloc(sizeof(int) * (size_t)plen);
                if (!N || !qinv || !p) { free(N); free(qinv); free(p); spasm_csr_free(R); throw EngineError("out of host memory"); }
                if (m > 0) memcpy(qinv, rec + 2, sizeof(int) * (size_t)m);
                if (n > 0) memcpy(p, rec + 2 + m, sizeof(int) * (size_t)n);
                for (int w = n; w < plen; w++) p[w] = -1;
                N->r = r;
                N->complete = false;
                N->L = nullptr;
                N->U = R;
                N->qinv = qinv;
                N->p = p;
                N->Ltmp = nullptr;
                res.lu[(size_t)i] = N;
            }
        }
    }
    st[3] = nchunks;
    st[4] = launches;
    st[5] = (i64)(ms * 1000.0);
    st[6] = entries;
}

// one matrix through the general path
void batch_slow(int mode, int i, const struct spasm_csr *M, struct echelonize_opts *opts, BatchResults &res)
{
    if (mode == BATCH_RANK) {
        i64 r = -1;
        if (opts && opts->L) {
            struct spasm_lu *N = do_echelonize(M, opts);
            r = N->r;
            spasm_lu_free(N);
        } else {
            (void)do_echelonize(M, opts, &r);
        }
        res.ranks[(size_t)i] = r;
    } else if (mode == BATCH_LU) {
        res.lu[(size_t)i] = do_echelonize(M, opts);
    } else {
        struct spasm_lu *N = do_echelonize(M, opts);
        try {
            res.K[(size_t)i] = do_kernel(N);
        } catch (...) {
            spasm_lu_free(N);
            throw;
        }
        spasm_lu_free(N);
    }
}

// mode BATCH_LU: lu_out[count]; BATCH_KERNEL: k_out[count]; BATCH_RANK: rank_out[count].  Nothing is written before all is done.
void batch_run(int mode, int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, struct spasm_lu **lu_out, struct spasm_csr **k_out, i64 *rank_out)
{
    memset(g_batch_stats, 0, sizeof g_batch_stats);
    if (count < 0) throw EngineError("count < 0");
    if (count == 0) return;
    if (!A || (mode == BATCH_LU && !lu_out) || (mode == BATCH_KERNEL && !k_out) || (mode == BATCH_RANK && !rank_out)) throw EngineError("NULL array");
    batch_check_list(count, A);
    require_device();
    const bool fast_ok = !opts || !opts->L;
    std::vector<int> fast, slow;
    for (int i = 0; i < count; i++) {
        const struct spasm_csr *M = A[i];
        if (fast_ok && M->n <= BATCH_LIMIT && M->m <= BATCH_LIMIT && (i64)M->n * M->m <= BATCH_LIMIT) fast.push_back(i);
        else slow.push_back(i);
    }
    BatchResults res(mode, count);
    i64 *st = g_batch_stats;
    st[0] = count;
    st[1] = (i64)fast.size();
    st[2] = (i64)slow.size();
    if (!fast.empty()) {
        BatchStaged in;
        const std::vector<BatchItem> item = batch_stage_items(A, fast, in);
        batch_fast(mode, fast, item, in.P, in.J, in.X, res);
    }
    // ---- the others through the general path, one at a time
    for (int i : slow) batch_slow(mode, i, A[i], opts, res);
    res.hand_over(mode, lu_out, k_out, rank_out);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// A matrix split into the connected components of its row/column graph, on the device (blocks.hpp).  The handle owns the maps and
// the blocks as ONE concatenated CSR in the layout the batch reads, so rank / echelonize / kernel of all blocks start from the
// descriptors: no entry crosses the host on the way.
// ------------------------------------------------------------------------------------------------
struct spasm_amd_blocks {
    int dev = 0;
    int n = 0, m = 0, nb = 0;
    int index = 0;                                                                 // 1: the index split (row i tied to column i)
    i64 nnz = 0;
    i64 prime = 0;
    DevBuf<int> row_block, row_pos, col_block, col_pos, block_rows, block_cols;   // n, n, m, m, n, m
    DevBuf<i64d> row_start, col_start;                                             // nb + 1 each
    DevBuf<i64d> P;                                                                // n + nb: rows + 1 pointers per block
    DevBuf<int> J, X;                                                              // nnz each
    std::vector<i64> h_row_start, h_col_start, h_nnz, h_ent0;                      // nb + 1, nb + 1, nb, nb + 1 (first entry of a block)
    i64 us[3] = {0, 0, 0};                                                         // device time: components, numbering, split
    i64 big[3] = {0, 0, 0};                                                        // the block with most entries: rows, columns, entries
    i64 empty = 0;                                                                 // blocks without entries
};

namespace {

template <int PH> void blk_launch_rows(const BlkArgs &a, i64 nnz, hipStream_t s)
{
    if (a.n == 0 || nnz == 0) return;
    const i64 avg = nnz / a.n;
    if (avg <= 3) hipLaunchKernelGGL((k_blk_rows<PH, 1>), dim3(cdiv(a.n, 256)), dim3(256), 0, s, a);
    else if (avg <= 24) hipLaunchKernelGGL((k_blk_rows<PH, 8>), dim3(cdiv((i64)a.n * 8, 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_blk_rows<PH, 64>), dim3(cdiv((i64)a.n * 64, 256)), dim3(256), 0, s, a);
    // the long rows: at most nnz / BLK_LONG of them; the list is complete when phase (a)'s row kernel has ended
    const int grid = (int)std::min<i64>(std::max<i64>(nnz / BLK_LONG, 1), 4096);
    hipLaunchKernelGGL((k_blk_long<PH>), dim3(grid), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
}

// sort (block, index) pairs by block, stable; end_bit covers nb - 1
void blk_sort(DevBuf<unsigned char> &tmp, const int *key, int *key_out, const int *val, int *val_out, int cnt, int nb, hipStream_t s)
{
    if (cnt == 0) return;
    int bits = 1;
    while (bits < 31 && ((i64)1 << bits) < nb) bits++;
    size_t bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, key, key_out, val, val_out, (size_t)cnt, 0, bits, s));
    tmp.ensure(bytes);
    HIPCHK(rocprim::radix_sort_pairs(tmp.p, bytes, key, key_out, val, val_out, (size_t)cnt, 0, bits, s));
}

// components, numbering and split of the n x m matrix (dP, dJ, dX) that lies on the current device; index: the index split
// (n == m, row i and column i are one vertex: the tie phase of blocks.hpp)
spasm_amd_blocks *blocks_build(int n, int m, i64 nnz, i64 prime, const i64d *dP, const int *dJ, const int *dX, bool index)
{
    hipStream_t s = nullptr;
    std::unique_ptr<spasm_amd_blocks> B(new spasm_amd_blocks());
    HIPCHK(hipGetDevice(&B->dev));
    if (index && n != m) throw EngineError("internal error: an index split of a matrix that is not square");
    B->index = index ? 1 : 0;
    B->n = n;
    B->m = m;
    B->nnz = nnz;
    B->prime = prime;
    const int nv = n + m;
    {
        // what the build holds at its peak, next to the matrix: the forest and the flags, two maps and two sort buffers per vertex,
        // the lengths and their scan (at most n + m blocks), the split entries, the temporaries of rocprim (a key/value copy at most)
        const double need = 4.0 * nv * 9 + 8.0 * (2.0 * nv + n) * 2 + 8.0 * (double)nnz + 4.0 * (nnz / BLK_LONG + 1) + (double)(1 << 20);
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        if (need > (double)fr) {
            char b[200];
            snprintf(b, sizeof b, "the working set of %.2f GiB does not fit the free device memory (%.2f GiB)", need / 1073741824.0, (double)fr / 1073741824.0);
            throw EngineError(b);
        }
    }
    SpgEvents ev;
    Scanner scan;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<int> parent, root, num, nlong, longrows, iota, key_sorted;
    parent.alloc((size_t)nv);
    root.alloc((size_t)nv + 1);
    num.alloc((size_t)nv + 1);
    nlong.alloc(1);
    longrows.alloc((size_t)(nnz / BLK_LONG) + 1);
    nlong.zero(s);
    BlkArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    a.m = m;
    a.P = dP;
    a.J = dJ;
    a.X = dX;
    a.parent = parent.p;
    a.nlong = nlong.p;
    a.longrows = longrows.p;
    // ---- components
    HIPCHK(hipEventRecord(ev.e[0], s));
    if (nv > 0) {
        hipLaunchKernelGGL(k_blk_init, dim3(cdiv(nv, 256)), dim3(256), 0, s, nv, parent.p);
        blk_launch_rows<BLK_MINCOL>(a, nnz, s);
        blk_launch_rows<BLK_UNITE>(a, nnz, s);
        if (index) hipLaunchKernelGGL(k_blk_tie, dim3(cdiv(n, 256)), dim3(256), 0, s, n, parent.p);
        hipLaunchKernelGGL(k_blk_flatten, dim3(cdiv(nv, 256)), dim3(256), 0, s, nv, parent.p, root.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev.e[1], s));
    // ---- numbering
    HIPCHK(hipMemsetAsync(root.p + nv, 0, sizeof(int), s));
    scan.exclusive<int>(root.p, num.p, (size_t)nv + 1, s);
    int nb = 0;
    HIPCHK(hipMemcpyAsync(&nb, num.p + nv, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nb < 0 || nb > nv) throw EngineError("internal error: block count outside its bounds");
    B->nb = nb;
    B->row_block.alloc((size_t)n);
    B->row_pos.alloc((size_t)n);
    B->block_rows.alloc((size_t)n);
    B->col_block.alloc((size_t)m);
    B->col_pos.alloc((size_t)m);
    B->block_cols.alloc((size_t)m);
    B->row_start.alloc((size_t)nb + 1);
    B->col_start.alloc((size_t)nb + 1);
    B->P.alloc((size_t)n + nb);
    B->J.alloc((size_t)nnz);
    B->X.alloc((size_t)nnz);
    DevBuf<i64d> len, bnnz;
    len.alloc((size_t)n + nb);
    bnnz.alloc((size_t)nb);
    len.zero(s);
    iota.alloc((size_t)std::max(n, m));
    key_sorted.alloc((size_t)std::max(n, m));
    if (nv > 0) {
        hipLaunchKernelGGL(k_blk_label, dim3(cdiv(nv, 256)), dim3(256), 0, s, n, m, (const int *)parent.p, (const int *)num.p, B->row_block.p, B->col_block.p, iota.p);
        HIPCHK(hipGetLastError());
    }
    // columns first: key_sorted is reused, and the rows' pass also fills the row lengths
    blk_sort(sort_tmp, B->col_block.p, key_sorted.p, iota.p, B->block_cols.p, m, nb, s);
    hipLaunchKernelGGL(k_blk_starts, dim3(cdiv((i64)nb + 1, 256)), dim3(256), 0, s, nb, m, (const int *)key_sorted.p, B->col_start.p);
    if (m > 0)
        hipLaunchKernelGGL(k_blk_pos, dim3(cdiv(m, 256)), dim3(256), 0, s, m, (const int *)key_sorted.p, (const int *)B->block_cols.p, (const i64d *)B->col_start.p, B->col_pos.p,
                           (const i64d *)nullptr, (i64d *)nullptr);
    blk_sort(sort_tmp, B->row_block.p, key_sorted.p, iota.p, B->block_rows.p, n, nb, s);
    hipLaunchKernelGGL(k_blk_starts, dim3(cdiv((i64)nb + 1, 256)), dim3(256), 0, s, nb, n, (const int *)key_sorted.p, B->row_start.p);
    if (n > 0)
        hipLaunchKernelGGL(k_blk_pos, dim3(cdiv(n, 256)), dim3(256), 0, s, n, (const int *)key_sorted.p, (const int *)B->block_rows.p, (const i64d *)B->row_start.p, B->row_pos.p, dP,
                           len.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[2], s));
    // ---- split
    if (n + nb > 0) scan.exclusive<i64d>(len.p, B->P.p, (size_t)n + nb, s);
    a.row_block = B->row_block.p;
    a.row_pos = B->row_pos.p;
    a.col_pos = B->col_pos.p;
    a.row_start = B->row_start.p;
    a.cP = B->P.p;
    a.cJ = B->J.p;
    a.cX = B->X.p;
    blk_launch_rows<BLK_COPY>(a, nnz, s);
    if (nb > 0) hipLaunchKernelGGL(k_blk_nnz, dim3(cdiv(nb, 256)), dim3(256), 0, s, nb, (const i64d *)B->row_start.p, (const i64d *)B->P.p, bnnz.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[3], s));
    B->h_row_start.assign((size_t)nb + 1, 0);
    B->h_col_start.assign((size_t)nb + 1, 0);
    B->h_nnz.assign((size_t)nb, 0);
    B->h_ent0.assign((size_t)nb + 1, 0);
    static_assert(sizeof(i64d) == sizeof(i64), "starts are copied as they are");
    HIPCHK(hipMemcpyAsync(B->h_row_start.data(), B->row_start.p, ((size_t)nb + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(B->h_col_start.data(), B->col_start.p, ((size_t)nb + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    if (nb > 0) HIPCHK(hipMemcpyAsync(B->h_nnz.data(), bnnz.p, (size_t)nb * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) B->us[k] = (i64)(ev.ms(k, k + 1) * 1000.0);
    if (B->h_row_start[(size_t)nb] != n || B->h_col_start[(size_t)nb] != m) throw EngineError("internal error: the blocks do not cover the matrix");
    for (int b = 0; b < nb; b++) {
        const i64 z = B->h_nnz[(size_t)b], r = B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b], c = B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b];
        if (z < 0 || r < 0 || c < 0) throw EngineError("internal error: a block of negative size");
        B->h_ent0[(size_t)b + 1] = B->h_ent0[(size_t)b] + z;
        if (z == 0) B->empty++;
        if (b == 0 || z > B->big[2]) { B->big[0] = r; B->big[1] = c; B->big[2] = z; }
    }
    if (B->h_ent0[(size_t)nb] != nnz) throw EngineError("internal error: the blocks do not hold the entries of the matrix");
    if (index && B->h_row_start != B->h_col_start) throw EngineError("internal error: a block of an index split is not square");
    return B.release();
}

// the checks that need no device; who names the entry's argument
void blocks_check_host(const struct spasm_csr *A)
{
    if (!A) throw EngineError("NULL matrix");
    if (!A->x) throw EngineError("matrix without values (A->x == NULL)");
    if (A->field->p <= 2 || A->field->p > 0xfffffffbLL) throw EngineError("prime out of range (2 < p <= 0xfffffffb)");
    if (A->n < 0 || A->m < 0) throw EngineError("malformed matrix");
    if ((i64)A->n + (i64)A->m >= ((i64)1 << 31)) throw EngineError("n + m must be below 2^31");
    if (!A->p || A->p[0] != 0) throw EngineError("malformed matrix");
    for (int i = 0; i < A->n; i++)
        if (A->p[i + 1] < A->p[i]) throw EngineError("row pointers must not decrease");
    if (A->p[A->n] > 0 && !A->j) throw EngineError("malformed matrix");
}

spasm_amd_blocks *blocks_create(const struct spasm_csr *A, bool index = false)
{
    blocks_check_host(A);
    if (index) require_square(-1, A->n, A->m);
    require_device();
    hipStream_t s = nullptr;
    const int n = A->n, m = A->m;
    const i64 nnz = A->p[n];
    DevBuf<i64d> dp;
    DevBuf<int> dj, dx, bad;
    dp.alloc((size_t)n + 1);
    dj.alloc((size_t)nnz);
    dx.alloc((size_t)nnz);
    bad.alloc(1);
    bad.zero(s);
    HIPCHK(hipMemcpyAsync(dp.p, A->p, ((size_t)n + 1) * sizeof(i64d), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(dj.p, A->j, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dx.p, A->x, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        // before anything indexes the forest by a column
        hipLaunchKernelGGL(k_spg_check_cols, dim3((int)std::min<i64>(cdiv(nnz, 256), 65536)), dim3(256), 0, s, (i64d)nnz, m, (const int *)dj.p, bad.p);
        HIPCHK(hipGetLastError());
        int hbad = 0;
        HIPCHK(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (hbad) throw EngineError("a column index lies outside the matrix");
    }
    return blocks_build(n, m, nnz, A->field->p, dp.p, dj.p, dx.p, index);
}

spasm_amd_blocks *blocks_create_dcsr(const spasm_amd_dcsr *D, bool index = false)
{
    if (!D) throw EngineError("NULL matrix");
    if (D->F.p <= 2 || D->F.p > 0xfffffffbLL) throw EngineError("prime out of range (2 < p <= 0xfffffffb)");
    if ((i64)D->n + (i64)D->m >= ((i64)1 << 31)) throw EngineError("n + m must be below 2^31");
    if (index) require_square(-1, D->n, D->m);
    hipStream_t s = nullptr;
    DevBuf<int> dj, dx;
    dj.alloc((size_t)D->nnz);
    dx.alloc((size_t)D->nnz);
    if (D->nnz > 0) {
        hipLaunchKernelGGL(k_spg_unpack, dim3((int)std::min<i64>(cdiv(D->nnz, 256), 65536)), dim3(256), 0, s, (i64d)D->nnz, (const int2 *)D->ent.p, dj.p, dx.p);
        HIPCHK(hipGetLastError());
    }
    return blocks_build(D->n, D->m, D->nnz, D->F.p, D->p.p, dj.p, dx.p, index);
}

void blocks_need(const spasm_amd_blocks *B)
{
    if (!B) throw EngineError("NULL handle");
}

// block b as the LDS path reads it from the handle's concatenated CSR (every block has rows + 1 pointers of its own)
BatchItem blocks_item(const spasm_amd_blocks *B, int b)
{
    const i64 r0 = B->h_row_start[(size_t)b], c0 = B->h_col_start[(size_t)b];
    return BatchItem{(int)(B->h_row_start[(size_t)b + 1] - r0), (int)(B->h_col_start[(size_t)b + 1] - c0), r0 + b, B->prime};
}

// block b as a host matrix (the caller frees it)
struct spasm_csr *blocks_fetch(const spasm_amd_blocks *B, int b)
{
    blocks_need(B);
    if (b < 0 || b >= B->nb) throw EngineError("block index out of range");
    hipStream_t s = nullptr;
    const i64 r0 = B->h_row_start[(size_t)b], rn = B->h_row_start[(size_t)b + 1] - r0, cn = B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b];
    const i64 e0 = B->h_ent0[(size_t)b], nz = B->h_nnz[(size_t)b];
    struct spasm_csr *R = spasm_csr_alloc((int)rn, (int)cn, nz, B->prime, true);
    if (!R) throw EngineError("out of host memory");
    try {
        HIPCHK(hipMemcpyAsync(R->p, B->P.p + r0 + b, ((size_t)rn + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
        if (nz > 0) {
            HIPCHK(hipMemcpyAsync(R->j, B->J.p + e0, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(R->x, B->X.p + e0, (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        for (i64 t = 0; t <= rn; t++) R->p[t] -= e0;
        if (R->p[0] != 0 || R->p[rn] != nz) throw EngineError("internal error: the row pointers of a block disagree with its size");
    } catch (...) {
        spasm_csr_free(R);
        throw;
    }
    return R;
}

// what the batch returns for an n x m matrix without entries: rank 0; U 0 x m, qinv = -1, p = the rows ascending; the kernel is the
// whole space, vector t = -1 on column t
void blocks_empty_result(int mode, int i, int n, int m, i64 prime, BatchResults &res)
{
    res.ranks[(size_t)i] = 0;
    if (mode == BATCH_RANK) return;
    if (mode == BATCH_KERNEL) {
        struct spasm_csr *K = spasm_csr_alloc(m, m, m, prime, true);
        if (!K) throw EngineError("out of host memory");
        for (int t = 0; t < m; t++) { K->p[t + 1] = t + 1; K->j[t] = t; K->x[t] = -1; }
        res.K[(size_t)i] = K;
        return;
    }
    struct spasm_csr *U = spasm_csr_alloc(0, m, 0, prime, true);
    struct spasm_lu *N = (struct spasm_lu *)malloc(sizeof *N);
    const int plen = std::max(std::max(n, m), 1);
    int *qinv = (int *)malloc(sizeof(int) * (size_t)std::max(m, 1));
    int *p = (int *)malloc(sizeof(int) * (size_t)plen);
    if (!U || !N || !qinv || !p) { free(N); free(qinv); free(p); spasm_csr_free(U); throw EngineError("out of host memory"); }
    for (int c = 0; c < std::max(m, 1); c++) qinv[c] = -1;
    for (int w = 0; w < plen; w++) p[w] = w < n ? w : -1;
    N->r = 0;
    N->complete = false;
    N->L = nullptr;
    N->U = U;
    N->qinv = qinv;
    N->p = p;
    N->Ltmp = nullptr;
    res.lu[(size_t)i] = N;
}

// rank / echelonize / kernel of every block: the batch with its input on the device already
void blocks_run(int mode, spasm_amd_blocks *B, struct echelonize_opts *opts, struct spasm_lu **lu_out, struct spasm_csr **k_out, i64 *rank_out)
{
    memset(g_batch_stats, 0, sizeof g_batch_stats);
    blocks_need(B);
    if ((mode == BATCH_LU && !lu_out) || (mode == BATCH_KERNEL && !k_out) || (mode == BATCH_RANK && !rank_out)) throw EngineError("NULL array");
    const int count = B->nb;
    if (count == 0) return;
    const bool fast_ok = !opts || !opts->L;
    std::vector<int> fast, slow, none;
    std::vector<BatchItem> item;
    for (int b = 0; b < count; b++) {
        const i64 rn = B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b], cn = B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b];
        if (!(fast_ok && rn <= BATCH_LIMIT && cn <= BATCH_LIMIT && rn * cn <= BATCH_LIMIT)) slow.push_back(b);
        else if (B->h_nnz[(size_t)b] == 0) none.push_back(b);
        else {
            fast.push_back(b);
            item.push_back(blocks_item(B, b));
        }
    }
    BatchResults res(mode, count);
    i64 *st = g_batch_stats;
    st[0] = count;
    st[1] = (i64)(fast.size() + none.size()); // (a block without entries belongs to the LDS path, which has nothing to do for it)
    st[2] = (i64)slow.size();
    batch_fast(mode, fast, item, B->P.p, B->J.p, B->X.p, res);
    for (int b : none)
        blocks_empty_result(mode, b, (int)(B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b]), (int)(B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b]), B->prime, res);
    for (int b : slow) {
        struct spasm_csr *M = blocks_fetch(B, b);
        try {
            batch_slow(mode, b, M, opts, res);
        } catch (...) {
            spasm_csr_free(M);
            throw;
        }
        spasm_csr_free(M);
    }
    res.hand_over(mode, lu_out, k_out, rank_out);
}

template <class T> void blocks_copy_out(T *dst, const DevBuf<T> &src, size_t cnt, hipStream_t s)
{
    if (dst && cnt > 0) HIPCHK(hipMemcpyAsync(dst, src.p, cnt * sizeof(T), hipMemcpyDeviceToHost, s));
}

} // namespace

// ------------------------------------------------------------------------------------------------
// X * A = B for many small matrices in one call, and block by block for a split matrix (solve_batch.hpp).  A system whose
// transposed image with one right-hand side fits LDS (m * (n + 1) <= BATCH_LIMIT) is cut into jobs, one per slab of right-hand sides;
// a job is one workgroup of k_solve_elim.  Per chunk of jobs whose scratch fits the budget: at most BATCH_NCLASS elimination
// launches, one scan, one pack, the 8-byte read of the chunk's entry count and one download.  The other systems go through
// do_echelonize with L and do_gesv one at a time.
// ------------------------------------------------------------------------------------------------
namespace {

thread_local i64 g_solve_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// a system of the LDS path (n, m, K >= 1): where its row pointers and those of its right-hand sides start, and its first slot
struct SolveSys { int n, m, K; i64 row0, brow0, slot0; i64 prime; };

inline bool solve_fits(i64 n, i64 m) { return n <= BATCH_LIMIT && m <= BATCH_LIMIT && m * (n + 1) <= BATCH_LIMIT; }

// Class, slab width and stride of a system.  The smallest class that holds all K right-hand sides next to A in one slab; when none
// does, the largest class and as many as it holds (a job repeats the elimination of A, so wide slabs are what saves work).  Stride:
// solve_batch.hpp, "Row stride".
void solve_shape(int n, int m, int K, int &cls, int &w, int &ld)
{
    int c = 0;
    i64 fit = 0;
    for (;; c++) {
        fit = kBatchClass[c].cap / m - n; // right-hand sides the class holds next to A (>= 1 in the last class: solve_fits)
        if (fit >= K || c == BATCH_NCLASS - 1) break;
    }
    w = (int)std::min<i64>(K, fit);
    const int W = n + w;
    ld = W;
    if (W % 2 == 0) {
        if ((i64)m * (W + 1) <= kBatchClass[c].cap) ld = W + 1;
        else if (w < K && w > 1) { w--; ld = n + w; }
    }
    cls = c;
}

// the jobs of the systems, in (system, slab) order; slots and slices are global here (solve_chunks makes them relative to a chunk)
void solve_jobs(const std::vector<SolveSys> &sys, std::vector<SolveDesc> &desc, std::vector<unsigned char> &cls, std::vector<i64> &ecap)
{
    for (const SolveSys &S : sys) {
        int c = 0, w = 0, ld = 0;
        solve_shape(S.n, S.m, S.K, c, w, ld);
        for (int t0 = 0; t0 < S.K; t0 += w) {
            SolveDesc d;
            memset(&d, 0, sizeof d);
            d.row0 = S.row0;
            d.brow0 = S.brow0 + t0;
            d.slot0 = S.slot0 + t0;
            d.n = S.n;
            d.m = S.m;
            d.w = std::min(w, S.K - t0);
            d.ld = ld;
            d.F = zp_field_make(S.prime);
            desc.push_back(d);
            cls.push_back((unsigned char)c);
            ecap.push_back((i64)d.w * (std::min(S.n, S.m) + 1));
        }
    }
}

// The chunks of a list of jobs (Desc carries slot0, slice, w; Args carries desc, cnt, src, ok, scratch), shared by solve_fast and the
// resident solver: consecutive jobs whose scratch fits the budget (per job: scratch + packed entries, and per slot: count, its scan,
// source, ok), slots and slices made relative to the chunk; per chunk the launches of `kern`, the scan, k_solve_pack and one
// download.  h_cnt / h_ok per slot, h_ent the rows of X back to back in slot order; st[4 .. 6] are filled.
template <class Desc, class Args>
void solve_chunks(const ElimKernels<Args> &kern, std::vector<Desc> &desc, const std::vector<unsigned char> &cls, const std::vector<i64> &ecap, Args a, i64 nslots,
                  std::vector<int> &h_cnt, std::vector<unsigned char> &h_ok, std::vector<int2> &h_ent, i64 *st)
{
    hipStream_t s = nullptr;
    const size_t budget = batch_budget();
    const int nj = (int)desc.size();
    const std::vector<int> cut = batch_cut(nj, budget, [&](int q) { return (size_t)ecap[(size_t)q] * 2 * sizeof(int2) + (size_t)desc[(size_t)q].w * (sizeof(int) + 2 * sizeof(i64d) + 1); });
    const int nchunks = (int)cut.size() - 1;
    std::vector<i64> c_slot0((size_t)nchunks), c_slots((size_t)nchunks), c_ents((size_t)nchunks);
    for (int c = 0; c < nchunks; c++) {
        const int lo = cut[(size_t)c], hi = cut[(size_t)c + 1];
        const i64 s0 = desc[(size_t)lo].slot0;
        i64 ents = 0;
        for (int q = lo; q < hi; q++) {
            desc[(size_t)q].slot0 -= s0;
            desc[(size_t)q].slice = ents;
            ents += ecap[(size_t)q];
        }
        c_slot0[(size_t)c] = s0;
        c_slots[(size_t)c] = desc[(size_t)hi - 1].slot0 + desc[(size_t)hi - 1].w;
        c_ents[(size_t)c] = ents;
    }
    DevBuf<Desc> d_desc;
    DevBuf<int> d_items, d_cnt;
    DevBuf<i64d> d_src, rowstart;
    DevBuf<unsigned char> d_ok;
    DevBuf<int2> scratch, out;
    Scanner scan;
    d_desc.alloc((size_t)nj);
    d_items.alloc((size_t)nj);
    HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nj * sizeof(Desc), hipMemcpyHostToDevice, s));
    std::vector<int> items((size_t)nj);
    a.desc = d_desc.p;
    SpgEvents ev;
    i64 launches = 0, entries = 0;
    double ms = 0;
    h_cnt.assign((size_t)nslots, 0);
    h_ok.assign((size_t)nslots, 0);
    h_ent.clear();
    for (int c = 0; c < nchunks; c++) {
        const int lo = cut[(size_t)c], hi = cut[(size_t)c + 1];
        const i64 slots = c_slots[(size_t)c], ents = c_ents[(size_t)c], s0 = c_slot0[(size_t)c];
        d_cnt.ensure((size_t)slots + 1);
        d_src.ensure((size_t)slots);
        d_ok.ensure((size_t)slots);
        scratch.ensure((size_t)ents + 1);
        a.cnt = d_cnt.p;
        a.src = d_src.p;
        a.ok = d_ok.p;
        a.scratch = scratch.p;
        HIPCHK(hipMemsetAsync(d_cnt.p + slots, 0, sizeof(int), s));
        launches += batch_launch_jobs(kern, cls, lo, hi, items, d_items.p, a, ev.e[0], s);
        const i64 total = batch_chunk_entries(d_cnt.p, slots, ents, rowstart, scan, s);
        launches++;
        if (total > 0) {
            out.ensure((size_t)total);
            hipLaunchKernelGGL(k_solve_pack, dim3((unsigned)slots), dim3(64), 0, s, (const int *)d_cnt.p, (const i64d *)d_src.p, (const i64d *)rowstart.p,
                               (const int2 *)scratch.p, out.p);
            HIPCHK(hipGetLastError());
            launches++;
        }
        HIPCHK(hipEventRecord(ev.e[1], s));
        const size_t at = h_ent.size();
        h_ent.resize(at + (size_t)total);
        HIPCHK(hipMemcpyAsync(h_cnt.data() + s0, d_cnt.p, (size_t)slots * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_ok.data() + s0, d_ok.p, (size_t)slots, hipMemcpyDeviceToHost, s));
        if (total > 0) HIPCHK(hipMemcpyAsync(h_ent.data() + at, out.p, (size_t)total * sizeof(int2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ms += ev.ms(0, 1);
        entries += total;
    }
    st[4] = launches;
    st[5] = (i64)(ms * 1000.0);
    st[6] = entries;
}

// The LDS path of spasm_amd_solve_batch from the systems on: h_cnt / h_ok per slot, h_ent the rows of X back to back in slot order.
void solve_fast(const std::vector<SolveSys> &sys, i64 nslots, const BatchStaged &A, const BatchStaged &B, std::vector<int> &h_cnt, std::vector<unsigned char> &h_ok,
                std::vector<int2> &h_ent)
{
    i64 *st = g_solve_stats;
    if (sys.empty()) return;
    std::vector<SolveDesc> desc;
    std::vector<unsigned char> cls;
    std::vector<i64> ecap;
    solve_jobs(sys, desc, cls, ecap);
    st[3] = (i64)desc.size();
    SolveBatchArgs a;
    memset(&a, 0, sizeof a);
    a.P = A.P; a.J = A.J; a.X = A.X;
    a.BP = B.P; a.BJ = B.J; a.BX = B.X;
    solve_chunks(kSolveElim, desc, cls, ecap, a, nslots, h_cnt, h_ok, h_ent, st);
}

struct CsrList {
    std::vector<struct spasm_csr *> v;
    ~CsrList() { for (auto *x : v) spasm_csr_free(x); }
};

// One system through the general path from its factorization N (with L) on: do_gesv.  Rows without a solution are emptied; the
// others get their columns in ascending order and lose their stored zeros.  n = the rows of A; ok[K].
struct spasm_csr *solve_slow_with(const struct spasm_lu *N, int n, i64 prime, const struct spasm_csr *B, unsigned char *ok)
{
    const ZpField F = zp_field_make(prime);
    const int K = B->n;
    // the right-hand side with reduced values
    struct spasm_csr *Bn = spasm_csr_alloc(K, B->m, B->p[K], prime, true);
    if (!Bn) throw EngineError("out of host memory");
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Bguard(Bn, spasm_csr_free);
    for (int k = 0; k <= K; k++) Bn->p[k] = B->p[k];
    for (i64 e = 0; e < B->p[K]; e++) { Bn->j[e] = B->j[e]; Bn->x[e] = zp_reduce(F, (int64_t)B->x[e]); }
    struct spasm_csr *Xs = do_gesv(N, Bn, ok);
    std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Xguard(Xs, spasm_csr_free);
    std::vector<std::pair<int, int>> row;
    i64 nz = 0;
    for (int k = 0; k < K; k++)
        if (ok[k])
            for (i64 e = Xs->p[k]; e < Xs->p[k + 1]; e++) nz += Xs->x[e] != 0;
    struct spasm_csr *X = spasm_csr_alloc(K, n, nz, prime, true);
    if (!X) throw EngineError("out of host memory");
    i64 w = 0;
    for (int k = 0; k < K; k++) {
        X->p[k] = w;
        if (!ok[k]) continue;
        row.clear();
        for (i64 e = Xs->p[k]; e < Xs->p[k + 1]; e++)
            if (Xs->x[e] != 0) row.push_back({Xs->j[e], Xs->x[e]});
        std::sort(row.begin(), row.end());
        for (auto &cv : row) { X->j[w] = cv.first; X->x[w] = cv.second; w++; }
    }
    X->p[K] = w;
    return X;
}

// the factorization of the general path: A echelonized with L
struct spasm_lu *solve_slow_factor(const struct spasm_csr *A)
{
    struct echelonize_opts o;
    spasm_echelonize_init_opts(&o);
    o.L = 1;
    return do_echelonize(A, &o);
}

// One system through the general path: A echelonized with L, then solve_slow_with.
struct spasm_csr *solve_slow(const struct spasm_csr *A, const struct spasm_csr *B, unsigned char *ok)
{
    struct spasm_lu *N = solve_slow_factor(A);
    std::unique_ptr<struct spasm_lu, void (*)(struct spasm_lu *)> Nguard(N, spasm_lu_free);
    return solve_slow_with(N, A->n, A->field->p, B, ok);
}

// Nothing is written to X / ok before all is done.
void solve_batch_run(int count, const struct spasm_csr *const *A, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok)
{
    memset(g_solve_stats, 0, sizeof g_solve_stats);
    if (count < 0) throw EngineError("count < 0");
    if (count == 0) return;
    if (!A || !B || !X || !ok) throw EngineError("NULL array");
    char msg[200];
    for (int i = 0; i < count; i++) {
        const char *bad = batch_check(A[i]);
        const char *which = "A";
        if (!bad) { bad = batch_check(B[i]); which = "B"; }
        if (!bad && A[i]->field->p != B[i]->field->p) { bad = "the primes of A and B differ"; which = "B"; }
        if (!bad && B[i]->m != A[i]->m) { bad = "B->m != A->m"; which = "B"; }
        if (!bad && B[i]->n > 0 && !ok[i]) { bad = "NULL array (ok)"; which = "B"; }
        if (bad) {
            snprintf(msg, sizeof msg, "matrix %d (%s): %s", i, which, bad);
            throw EngineError(msg);
        }
    }
    i64 *st = g_solve_stats;
    st[0] = count;
    CsrList res;
    res.v.assign((size_t)count, nullptr);
    std::vector<std::vector<unsigned char>> oks((size_t)count);
    std::vector<int> fast, slow;
    for (int i = 0; i < count; i++) {
        const int n = A[i]->n, m = A[i]->m, K = B[i]->n;
        oks[(size_t)i].assign((size_t)K, 1);
        if (n == 0 || m == 0 || K == 0) {
            // no launch: without rows only the zero row is reachable, without columns everything is
            const ZpField F = zp_field_make(A[i]->field->p);
            for (int k = 0; k < K && n == 0; k++)
                for (i64 e = B[i]->p[k]; e < B[i]->p[k + 1]; e++)
                    if (zp_reduce(F, (int64_t)B[i]->x[e]) != 0) oks[(size_t)i][(size_t)k] = 0;
            res.v[(size_t)i] = spasm_csr_alloc(K, n, 0, A[i]->field->p, true);
            if (!res.v[(size_t)i]) throw EngineError("out of host memory");
            for (int k = 0; k <= K; k++) res.v[(size_t)i]->p[k] = 0;
            st[1]++;
        } else if (solve_fits(n, m)) fast.push_back(i);
        else slow.push_back(i);
    }
    if (!fast.empty() || !slow.empty()) require_device();
    st[1] += (i64)fast.size();
    st[2] = (i64)slow.size();
    if (!fast.empty()) {
        BatchStaged ina, inb;
        const std::vector<BatchItem> ia = batch_stage_items(A, fast, ina), ib = batch_stage_items(B, fast, inb);
        std::vector<SolveSys> sys;
        i64 nslots = 0;
        for (size_t f = 0; f < fast.size(); f++) {
            sys.push_back(SolveSys{ia[f].n, ia[f].m, ib[f].n, ia[f].row0, ib[f].row0, nslots, ia[f].prime});
            nslots += ib[f].n;
        }
        std::vector<int> h_cnt;
        std::vector<unsigned char> h_ok;
        std::vector<int2> h_ent;
        solve_fast(sys, nslots, ina, inb, h_cnt, h_ok, h_ent);
        i64 at = 0;
        for (size_t f = 0; f < fast.size(); f++) {
            const int i = fast[f], K = sys[f].K;
            res.v[(size_t)i] = batch_rows_to_csr(K, sys[f].n, sys[f].prime, h_cnt.data() + sys[f].slot0, h_ent.data(), (i64)h_ent.size(), at);
            memcpy(oks[(size_t)i].data(), h_ok.data() + sys[f].slot0, (size_t)K);
        }
    }
    for (int i : slow) res.v[(size_t)i] = solve_slow(A[i], B[i], oks[(size_t)i].data());
    for (int i = 0; i < count; i++)
        for (unsigned char v : oks[(size_t)i]) st[7] += v ? 0 : 1;
    for (int i = 0; i < count; i++)
        if (!oks[(size_t)i].empty()) memcpy(ok[i], oks[(size_t)i].data(), oks[(size_t)i].size());
    memcpy(X, res.v.data(), sizeof(struct spasm_csr *) * (size_t)count);
    res.v.clear();
}

// 64-bit keys with 32-bit values, stable, on the low `bits` bits
void solve_sort(DevBuf<unsigned char> &tmp, const unsigned long long *key, unsigned long long *key_out, const int *val, int *val_out, i64 cnt, int bits, hipStream_t s)
{
    if (cnt == 0) return;
    size_t bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, key, key_out, val, val_out, (size_t)cnt, 0, bits, s));
    tmp.ensure(bytes);
    HIPCHK(rocprim::radix_sort_pairs(tmp.p, bytes, key, key_out, val, val_out, (size_t)cnt, 0, bits, s));
}

inline int solve_bits(i64 v)
{
    int bits = 1;
    while (bits < 32 && ((i64)1 << bits) < v) bits++;
    return bits;
}

// what solve_blocks_rows reads of a split: the maps on the device and the starts of the blocks on the host
struct BlocksView {
    int nb;
    i64 prime;
    const int *col_block, *col_pos, *block_rows;
    const i64d *row_start;
    const std::vector<i64> *h_row_start, *h_col_start;
};

// how the blocks that meet a right-hand side are solved
struct BlocksSolveOps {
    virtual ~BlocksSolveOps() {}
    // does block b (rn x cn, rn > 0) take the LDS path?
    virtual bool fits(int b, i64 rn, i64 cn) = 0;
    // the jobs of the LDS-path blocks (sys[f] is block blk[f]; brow0 = slot0 = its first run): returns the words (int2) of entry
    // scratch they need, slices laid out from 0, and their number
    virtual i64 plan(const std::vector<SolveSys> &sys, const std::vector<int> &blk, int &njobs) = 0;
    // a block over the limit against its runs Rb, on the general path
    virtual struct spasm_csr *slow(int b, const struct spasm_csr *Rb, unsigned char *okb) = 0;
    // the planned jobs: right-hand sides (run_start, sj, sx), outputs per run; returns the launches, with the stream drained
    virtual i64 launch(const i64d *run_start, const int *sj, const int *sx, int *cnt, i64d *src, unsigned char *ok, int2 *scratch, hipStream_t s) = 0;
};

// spasm_amd_blocks_solve: every call eliminates the blocks it meets (k_solve_elim from the resident concatenated CSR)
struct BlocksElimOps : BlocksSolveOps {
    spasm_amd_blocks *B;
    std::vector<SolveDesc> desc;
    std::vector<unsigned char> cls;
    explicit BlocksElimOps(spasm_amd_blocks *B_) : B(B_) {}
    bool fits(int, i64 rn, i64 cn) override { return solve_fits(rn, cn); }
    i64 plan(const std::vector<SolveSys> &sys, const std::vector<int> &, int &njobs) override
    {
        std::vector<i64> ecap;
        desc.clear();
        cls.clear();
        solve_jobs(sys, desc, cls, ecap);
        njobs = (int)desc.size();
        i64 ents = 0;
        for (int q = 0; q < njobs; q++) { desc[(size_t)q].slice = ents; ents += ecap[(size_t)q]; }
        return ents;
    }
    struct spasm_csr *slow(int b, const struct spasm_csr *Rb, unsigned char *okb) override
    {
        struct spasm_csr *M = blocks_fetch(B, b);
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Mguard(M, spasm_csr_free);
        return solve_slow(M, Rb, okb);
    }
    i64 launch(const i64d *run_start, const int *sj, const int *sx, int *cnt, i64d *src, unsigned char *ok, int2 *scratch, hipStream_t s) override
    {
        const int nj = (int)desc.size();
        DevBuf<SolveDesc> d_desc;
        DevBuf<int> d_items;
        d_desc.alloc((size_t)nj);
        d_items.alloc((size_t)nj);
        HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nj * sizeof(SolveDesc), hipMemcpyHostToDevice, s));
        std::vector<int> items((size_t)nj);
        SolveBatchArgs a;
        memset(&a, 0, sizeof a);
        a.desc = d_desc.p;
        a.P = B->P.p; a.J = B->J.p; a.X = B->X.p;
        a.BP = run_start; a.BJ = sj; a.BX = sx;
        a.cnt = cnt;
        a.src = src;
        a.ok = ok;
        a.scratch = scratch;
        const i64 launches = batch_launch_jobs(kSolveElim, cls, 0, nj, items, d_items.p, a, nullptr, s);
        HIPCHK(hipStreamSynchronize(s)); // (items and the buffers belong to this scope)
        return launches;
    }
};

inline BlocksView blocks_view(const spasm_amd_blocks *B)
{
    return BlocksView{B->nb, B->prime, B->col_block.p, B->col_pos.p, B->block_rows.p, B->row_start.p, &B->h_row_start, &B->h_col_start};
}

// Rows k0 .. k1 of Rhs (on the device as rp / rj / rx) against the blocks of the handle.  Appends to xp (row lengths become
// pointers at the caller), xj, xx and writes ok[k0 .. k1).  The pipeline, every step on the device unless it says otherwise:
//   keys      (block of the entry's column, row) per entry; a stable sort; the runs of equal keys = the right-hand sides of the blocks
//   plan      where the runs of each block start comes to the host (nb + 1 words): jobs for the blocks inside the limit; the blocks
//             over it are fetched with their runs and solved by solve_slow, their rows of X uploaded behind the jobs' slices
//   solve     k_solve_elim from the resident concatenated CSR; a run of a block without rows is solvable iff it vanishes
//   assemble  the runs by row (a second stable sort), ok[k] = AND over the runs of row k, the entries of the solvable rows as
//             (row, row of A) keys through block_rows, one sort, row pointers by bisection, one download
// The maps of the split come as a BlocksView and the solve of the blocks as a BlocksSolveOps, so that the resident solver, which
// holds copies of the maps and its own operators, runs the same pipeline.
void solve_blocks_rows(const BlocksView &B, BlocksSolveOps &ops, i64 *st, int k0, int k1, const i64d *rp, const i64 *h_rp, const int *rj, const int *rx,
                       std::vector<i64> &xlen, std::vector<int> &xj, std::vector<int> &xx, unsigned char *ok)
{
    hipStream_t s = nullptr;
    const int K = k1 - k0, nb = B.nb;
    const i64 e0 = h_rp[k0], ne = h_rp[k1] - e0;
    const ZpField F = zp_field_make(B.prime);
    if (ne == 0) {
        for (int k = 0; k < K; k++) { ok[k0 + k] = 1; xlen[(size_t)(k0 + k)] = 0; }
        return;
    }
    Scanner scan;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<unsigned long long> key, skey;
    DevBuf<int> val, sval, head, runid, sj, sx;
    key.alloc((size_t)ne);
    skey.alloc((size_t)ne);
    val.alloc((size_t)ne);
    sval.alloc((size_t)ne);
    head.alloc((size_t)ne + 1);
    runid.alloc((size_t)ne + 1);
    sj.alloc((size_t)ne);
    sx.alloc((size_t)ne);
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    hipLaunchKernelGGL(k_sv_keys, dim3(cdiv(ne, 256)), dim3(256), 0, s, K, (i64d)e0, (i64d)ne, rp + k0, rj, B.col_block, key.p, val.p);
    HIPCHK(hipGetLastError());
    solve_sort(sort_tmp, key.p, skey.p, val.p, sval.p, ne, 32 + solve_bits(nb), s);
    hipLaunchKernelGGL(k_sv_heads, dim3(cdiv(ne + 1, 256)), dim3(256), 0, s, (i64d)ne, (const unsigned long long *)skey.p, head.p);
    HIPCHK(hipGetLastError());
    scan.exclusive<int>(head.p, runid.p, (size_t)ne + 1, s);
    int nruns = 0;
    HIPCHK(hipMemcpyAsync(&nruns, runid.p + ne, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nruns <= 0 || nruns > ne) throw EngineError("internal error: run count outside its bounds");
    DevBuf<i64d> run_start, brun, d_src, krun, off;
    DevBuf<int> run_block, run_row, d_cnt, iota, byrow, krow, len;
    DevBuf<unsigned char> d_ok, rowok;
    run_start.alloc((size_t)nruns + 1);
    run_block.alloc((size_t)nruns);
    run_row.alloc((size_t)nruns);
    brun.alloc((size_t)nb + 1);
    d_cnt.alloc((size_t)nruns);
    d_src.alloc((size_t)nruns);
    d_ok.alloc((size_t)nruns);
    iota.alloc((size_t)nruns);
    hipLaunchKernelGGL(k_sv_runs, dim3(cdiv(ne + 1, 256)), dim3(256), 0, s, (i64d)e0, (i64d)ne, (const unsigned long long *)skey.p, (const int *)sval.p, (const int *)head.p,
                       (const int *)runid.p, rj, rx, B.col_pos, run_start.p, run_block.p, run_row.p, sj.p, sx.p);
    hipLaunchKernelGGL(k_blk_starts, dim3(cdiv((i64)nb + 1, 256)), dim3(256), 0, s, nb, nruns, (const int *)run_block.p, brun.p);
    hipLaunchKernelGGL(k_sv_init, dim3(cdiv(nruns, 256)), dim3(256), 0, s, nruns, F, (const i64d *)run_start.p, (const int *)run_block.p, B.row_start,
                       (const int *)sx.p, d_cnt.p, d_src.p, d_ok.p, iota.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<i64> h_brun((size_t)nb + 1);
    HIPCHK(hipMemcpyAsync(h_brun.data(), brun.p, ((size_t)nb + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // ---- plan (host: one step per block)
    std::vector<SolveSys> sys;
    std::vector<int> sysb, slow;
    for (int b = 0; b < nb; b++) {
        const i64 Kb = h_brun[(size_t)b + 1] - h_brun[(size_t)b];
        if (Kb == 0) continue;
        const i64 rn = (*B.h_row_start)[(size_t)b + 1] - (*B.h_row_start)[(size_t)b], cn = (*B.h_col_start)[(size_t)b + 1] - (*B.h_col_start)[(size_t)b];
        st[0]++;
        if (rn == 0) st[1]++;
        else if (ops.fits(b, rn, cn)) {
            st[1]++;
            sys.push_back(SolveSys{(int)rn, (int)cn, (int)Kb, (*B.h_row_start)[(size_t)b] + b, h_brun[(size_t)b], h_brun[(size_t)b], B.prime});
            sysb.push_back(b);
        } else {
            st[2]++;
            slow.push_back(b);
        }
    }
    int nj = 0;
    const i64 ents = ops.plan(sys, sysb, nj);
    st[3] += nj;
    // ---- the blocks over the limit, on the host; their rows of X go behind the slices
    std::vector<int2> slow_ent;
    std::vector<int> slow_cnt;
    std::vector<i64> slow_src, slow_run;
    std::vector<unsigned char> slow_ok;
    for (int b : slow) {
        const i64 q0 = h_brun[(size_t)b], Kb = h_brun[(size_t)b + 1] - q0;
        const int cn = (int)((*B.h_col_start)[(size_t)b + 1] - (*B.h_col_start)[(size_t)b]);
        std::vector<i64> rs((size_t)Kb + 1);
        HIPCHK(hipMemcpy(rs.data(), run_start.p + q0, ((size_t)Kb + 1) * sizeof(i64d), hipMemcpyDeviceToHost));
        const i64 z0 = rs[0], z = rs[(size_t)Kb] - z0;
        struct spasm_csr *Rb = spasm_csr_alloc((int)Kb, cn, z, B.prime, true);
        if (!Rb) throw EngineError("out of host memory");
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Rguard(Rb, spasm_csr_free);
        for (i64 t = 0; t <= Kb; t++) Rb->p[t] = rs[(size_t)t] - z0;
        if (z > 0) {
            HIPCHK(hipMemcpy(Rb->j, sj.p + z0, (size_t)z * sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(Rb->x, sx.p + z0, (size_t)z * sizeof(int), hipMemcpyDeviceToHost));
        }
        std::vector<unsigned char> okb((size_t)Kb, 0);
        struct spasm_csr *Xb = ops.slow(b, Rb, okb.data());
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Xguard(Xb, spasm_csr_free);
        for (i64 t = 0; t < Kb; t++) {
            slow_run.push_back(q0 + t);
            slow_ok.push_back(okb[(size_t)t]);
            slow_cnt.push_back((int)(Xb->p[t + 1] - Xb->p[t]));
            slow_src.push_back(ents + (i64)slow_ent.size());
            for (i64 e = Xb->p[t]; e < Xb->p[t + 1]; e++) slow_ent.push_back(make_int2(Xb->j[e], Xb->x[e]));
        }
    }
    DevBuf<int2> scratch;
    scratch.alloc((size_t)ents + slow_ent.size() + 1);
    if (!slow_ent.empty()) HIPCHK(hipMemcpy(scratch.p + ents, slow_ent.data(), slow_ent.size() * sizeof(int2), hipMemcpyHostToDevice));
    for (size_t t = 0; t < slow_run.size(); t++) {
        HIPCHK(hipMemcpy(d_cnt.p + slow_run[t], &slow_cnt[t], sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_src.p + slow_run[t], &slow_src[t], sizeof(i64d), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ok.p + slow_run[t], &slow_ok[t], 1, hipMemcpyHostToDevice));
    }
    // ---- solve
    i64 launches = 0;
    HIPCHK(hipEventRecord(ev.e[2], s));
    if (nj > 0) launches += ops.launch(run_start.p, sj.p, sx.p, d_cnt.p, d_src.p, d_ok.p, scratch.p, s);
    // ---- assemble
    byrow.alloc((size_t)nruns);
    krow.alloc((size_t)nruns);
    krun.alloc((size_t)K + 1);
    len.alloc((size_t)nruns + 1);
    off.alloc((size_t)nruns + 1);
    rowok.alloc((size_t)K);
    blk_sort(sort_tmp, run_row.p, krow.p, iota.p, byrow.p, nruns, K, s);
    hipLaunchKernelGGL(k_blk_starts, dim3(cdiv((i64)K + 1, 256)), dim3(256), 0, s, K, nruns, (const int *)krow.p, krun.p);
    HIPCHK(hipMemsetAsync(len.p + nruns, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_sv_rowok, dim3(cdiv(K, 256)), dim3(256), 0, s, K, (const i64d *)krun.p, (const int *)byrow.p, (const unsigned char *)d_ok.p, (const int *)d_cnt.p,
                       rowok.p, len.p);
    HIPCHK(hipGetLastError());
    scan.exclusive((const int *)len.p, off.p, (size_t)nruns + 1, s);
    i64d total = 0;
    HIPCHK(hipMemcpyAsync(&total, off.p + nruns, sizeof total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total < 0 || total > ents + (i64)slow_ent.size()) throw EngineError("internal error: the rows of X hold more entries than the slices");
    std::vector<i64> h_p((size_t)K + 1, 0);
    const size_t at = xj.size();
    xj.resize(at + (size_t)total);
    xx.resize(at + (size_t)total);
    DevBuf<unsigned long long> xkey, xskey;
    DevBuf<int> xval, xsval, outj;
    DevBuf<i64d> outp;
    outp.alloc((size_t)K + 1);
    xkey.alloc((size_t)total);
    xskey.alloc((size_t)total);
    xval.alloc((size_t)total);
    xsval.alloc((size_t)total);
    outj.alloc((size_t)total);
    if (total > 0) {
        hipLaunchKernelGGL(k_sv_emit, dim3((unsigned)nruns), dim3(64), 0, s, (const int *)len.p, (const i64d *)off.p, (const i64d *)d_src.p, (const int *)run_block.p,
                           (const int *)run_row.p, B.row_start, B.block_rows, (const int2 *)scratch.p, xkey.p, xval.p);
        HIPCHK(hipGetLastError());
        solve_sort(sort_tmp, xkey.p, xskey.p, xval.p, xsval.p, total, 32 + solve_bits(K), s);
    }
    hipLaunchKernelGGL(k_sv_finish, dim3(cdiv(std::max<i64>(total, (i64)K + 1), 256)), dim3(256), 0, s, K, total, (const unsigned long long *)xskey.p, outp.p, outj.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[3], s));
    HIPCHK(hipMemcpyAsync(h_p.data(), outp.p, ((size_t)K + 1) * sizeof(i64d), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ok + k0, rowok.p, (size_t)K, hipMemcpyDeviceToHost, s));
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(xj.data() + at, outj.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(xx.data() + at, xsval.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (h_p[0] != 0 || h_p[(size_t)K] != total) throw EngineError("internal error: the row pointers of X disagree with its entries");
    for (int k = 0; k < K; k++) xlen[(size_t)(k0 + k)] = h_p[(size_t)k + 1] - h_p[(size_t)k];
    st[4] += launches;
    st[5] += (i64)((ev.ms(0, 1) + ev.ms(2, 3)) * 1000.0);
    st[6] += total;
}

// Rhs against the split (n x m, on device dev) that V views: the checks of Rhs, its upload, the rows in chunks, X and ok.
void solve_blocks_apply(const BlocksView &V, int n, int m, int dev, BlocksSolveOps &ops, i64 *st, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok)
{
    const std::vector<i64> &h_row_start = *V.h_row_start, &h_col_start = *V.h_col_start;
    if (!Rhs) throw EngineError("NULL matrix");
    if (Rhs->m != m) throw EngineError("Rhs->m differs from the columns of the handle's matrix");
    if (Rhs->field->p != V.prime) throw EngineError("the prime of Rhs differs from the handle's");
    const char *bad = batch_check(Rhs);
    if (bad) throw EngineError(bad);
    if (!X || (Rhs->n > 0 && !ok)) throw EngineError("NULL array");
    HIPCHK(hipSetDevice(dev));
    hipStream_t s = nullptr;
    const int K = Rhs->n;
    const i64 nnz = Rhs->p[K];
    std::vector<i64> xlen((size_t)K, 0);
    std::vector<int> xj, xx;
    std::vector<unsigned char> hok((size_t)K, 1);
    if (K > 0 && nnz > 0) {
        DevBuf<i64d> rp;
        DevBuf<int> rj, rx;
        rp.alloc((size_t)K + 1);
        rj.alloc((size_t)nnz);
        rx.alloc((size_t)nnz);
        static_assert(sizeof(i64d) == sizeof(i64), "row pointers are copied as they are");
        HIPCHK(hipMemcpyAsync(rp.p, Rhs->p, ((size_t)K + 1) * sizeof(i64d), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(rj.p, Rhs->j, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(rx.p, Rhs->x, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        // chunks of rows: an entry of Rhs opens at most one run, a run holds at most min(rows, cols) + 1 entries of its block, and
        // every such entry is held about five times on the way (scratch, key and value twice, column)
        i64 rmax = 1;
        for (int b = 0; b < V.nb; b++)
            rmax = std::max(rmax, std::min(h_row_start[(size_t)b + 1] - h_row_start[(size_t)b], h_col_start[(size_t)b + 1] - h_col_start[(size_t)b]) + 1);
        const double per = 64.0 + 48.0 * (double)rmax;
        const i64 cap = std::min<i64>((i64)std::max(1.0, (double)batch_budget() / per), ((i64)1 << 31) - 2);
        int k0 = 0;
        while (k0 < K) {
            int k1 = k0 + 1;
            while (k1 < K && Rhs->p[k1 + 1] - Rhs->p[k0] <= cap) k1++;
            if (Rhs->p[k1] - Rhs->p[k0] > ((i64)1 << 31) - 2) throw EngineError("a row of Rhs holds 2^31 entries or more");
            solve_blocks_rows(V, ops, st, k0, k1, rp.p, Rhs->p, rj.p, rx.p, xlen, xj, xx, hok.data());
            k0 = k1;
        }
    }
    struct spasm_csr *R = spasm_csr_alloc(K, n, (i64)xj.size(), V.prime, true);
    if (!R) throw EngineError("out of host memory");
    R->p[0] = 0;
    for (int k = 0; k < K; k++) R->p[k + 1] = R->p[k] + xlen[(size_t)k];
    if (R->p[K] != (i64)xj.size()) { spasm_csr_free(R); throw EngineError("internal error: the rows of X disagree with its entries"); }
    if (!xj.empty()) {
        memcpy(R->j, xj.data(), xj.size() * sizeof(int));
        memcpy(R->x, xx.data(), xx.size() * sizeof(int));
    }
    for (int k = 0; k < K; k++) st[7] += hok[(size_t)k] ? 0 : 1;
    if (K > 0) memcpy(ok, hok.data(), (size_t)K);
    *X = R;
}

void solve_blocks_run(spasm_amd_blocks *B, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok)
{
    memset(g_solve_stats, 0, sizeof g_solve_stats);
    blocks_need(B);
    BlocksElimOps ops(B);
    solve_blocks_apply(blocks_view(B), B->n, B->m, B->dev, ops, g_solve_stats, Rhs, X, ok);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// X * A = B with A factored once (solver.hpp): spasm_amd_solver_*.  create eliminates every system of the LDS path once (one
// workgroup of k_solver_factor per slab of identity columns) and keeps the operators G, the pivots and the ranks on the device;
// a system over the limit keeps its factorization with L.  apply is solve_batch with k_solver_apply in place of k_solve_elim, on
// the same chunk driver (solve_chunks), and apply_blocks is blocks_solve on the same pipeline (solve_blocks_rows).
// ------------------------------------------------------------------------------------------------
enum { SOLVER_LDS = 0, SOLVER_GENERAL = 1, SOLVER_EMPTY = 2 };

struct SolverSys {
    int n = 0, m = 0, kind = SOLVER_EMPTY, r = 0;
    i64 prime = 0;
    i64 goff = 0, pivoff = 0;        // SOLVER_LDS: its operator (room for min(n, m) columns of m words) and its pivots
    int ldg = 1, cls = 0, q = 1;     // LDS layout of an apply job (solver_shape)
    struct spasm_lu *lu = nullptr;   // SOLVER_GENERAL
    std::vector<int> basis;          // the rows of A the solutions live on, ascending
};

struct spasm_amd_solver {
    int dev = 0;
    bool blocks = false;
    std::vector<SolverSys> sys;
    DevBuf<int> G, pivrow, pivcol;
    i64 info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // a handle made from a split: system b = block b, and copies of the maps the assembly reads
    int n = 0, m = 0, nb = 0;
    i64 prime = 0;
    DevBuf<int> col_block, col_pos, block_rows;
    DevBuf<i64d> row_start;
    std::vector<i64> h_row_start, h_col_start;
    // the dense apply: the global columns of every block (a handle made from a split) and the job plan of the most recent K
    DevBuf<int> block_cols;
    struct DensePlan {
        int K = 0, njobs = 0, launches = 0;
        int hist[BATCH_NCLASS] = {0, 0, 0, 0};
        DevBuf<SolverDenseDesc> desc;
        DevBuf<int> items;
        DevBuf<unsigned> flag;
    } dense;
    i64 dense_built = 0;
    ~spasm_amd_solver()
    {
        for (SolverSys &Y : sys) spasm_lu_free(Y.lu);
    }
};

namespace {

thread_local i64 g_solver_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

const ElimKernels<SolverFactorArgs> kSolverFactor = {{k_solver_factor<64>, k_solver_factor<128>, k_solver_factor<256>, k_solver_factor<512>}};
const ElimKernels<SolverApplyArgs> kSolverApply = {{k_solver_apply<64>, k_solver_apply<128>, k_solver_apply<256>, k_solver_apply<512>}};
const ElimKernels<SolverDenseArgs> kSolverDense = {{k_solver_apply_dense<64>, k_solver_apply_dense<128>, k_solver_apply_dense<256>, k_solver_apply_dense<512>}};

// rounds of q right-hand sides a job of k_solver_apply works through: what staging G once is spread over
constexpr int kSolverRounds = 8;

// Class, stride and right-hand sides in flight of an operator of m x r words (solver.hpp, "Row stride").  The smallest class that
// holds G and one vector of m + r words; q = the vectors that fit beside G, at most one per group of whole waves that covers m.
void solver_shape(int m, int r, int &cls, int &ldg, int &q)
{
    ldg = std::max(r, 1);
    if (ldg % 2 == 0 && (i64)m * (ldg + 1) + m + r <= kBatchClass[BATCH_NCLASS - 1].cap) ldg++;
    const i64 need = (i64)m * ldg + m + r;
    int c = 0;
    while (c < BATCH_NCLASS - 1 && need > kBatchClass[c].cap) c++;
    if (need > kBatchClass[c].cap) throw EngineError("internal error: an operator does not fit the largest class");
    const int mp = (m + 63) & ~63, bs = kBatchClass[c].bs;
    const i64 room = (kBatchClass[c].cap - (i64)m * ldg) / (m + r);
    q = mp <= bs ? (int)std::min<i64>(bs / mp, room) : 1;
    cls = c;
}

// The operators of the LDS-path systems list[f] (places in S->sys; n, m > 0) from the concatenated CSR on the device; row0[f] =
// where the n + 1 row pointers of list[f] start in P.  Adds to info[5 .. 7].
void solver_factor(spasm_amd_solver *S, const std::vector<int> &list, const std::vector<i64> &row0, const i64d *dP, const int *dJ, const int *dX)
{
    const int nf = (int)list.size();
    if (nf == 0) return;
    hipStream_t s = nullptr;
    i64 gwords = 0, pwords = 0;
    for (int i : list) {
        SolverSys &Y = S->sys[(size_t)i];
        const i64 cap = std::min(Y.n, Y.m);
        Y.goff = gwords;
        Y.pivoff = pwords;
        gwords += (i64)Y.m * cap;
        pwords += cap;
    }
    S->G.alloc((size_t)gwords);
    S->pivrow.alloc((size_t)pwords);
    S->pivcol.alloc((size_t)pwords);
    DevBuf<int> drank;
    drank.alloc((size_t)nf);
    // ---- jobs: one per slab of the m identity columns, by the rules of the right-hand sides (solve_shape)
    std::vector<SolverFactorDesc> desc;
    std::vector<unsigned char> cls;
    for (int f = 0; f < nf; f++) {
        const SolverSys &Y = S->sys[(size_t)list[(size_t)f]];
        int c = 0, w = 0, ld = 0;
        solve_shape(Y.n, Y.m, Y.m, c, w, ld);
        for (int t0 = 0; t0 < Y.m; t0 += w) {
            SolverFactorDesc d;
            memset(&d, 0, sizeof d);
            d.row0 = row0[(size_t)f];
            d.goff = Y.goff;
            d.pivoff = Y.pivoff;
            d.sys = f;
            d.n = Y.n;
            d.m = Y.m;
            d.ld = ld;
            d.t0 = t0;
            d.w = std::min(w, Y.m - t0);
            d.F = zp_field_make(Y.prime);
            desc.push_back(d);
            cls.push_back((unsigned char)c);
        }
    }
    const int nj = (int)desc.size();
    DevBuf<SolverFactorDesc> d_desc;
    DevBuf<int> d_items;
    d_desc.alloc((size_t)nj);
    d_items.alloc((size_t)nj);
    HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nj * sizeof(SolverFactorDesc), hipMemcpyHostToDevice, s));
    std::vector<int> items((size_t)nj);
    SolverFactorArgs a;
    memset(&a, 0, sizeof a);
    a.desc = d_desc.p;
    a.P = dP; a.J = dJ; a.X = dX;
    a.G = S->G.p;
    a.pivrow = S->pivrow.p;
    a.pivcol = S->pivcol.p;
    a.rank = drank.p;
    SpgEvents ev;
    const i64 launches = batch_launch_jobs(kSolverFactor, cls, 0, nj, items, d_items.p, a, ev.e[0], s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> hrank((size_t)nf), hpivcol((size_t)std::max<i64>(pwords, 1));
    HIPCHK(hipMemcpyAsync(hrank.data(), drank.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost, s));
    if (pwords > 0) HIPCHK(hipMemcpyAsync(hpivcol.data(), S->pivcol.p, (size_t)pwords * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int f = 0; f < nf; f++) {
        SolverSys &Y = S->sys[(size_t)list[(size_t)f]];
        const int r = hrank[(size_t)f];
        if (r < 0 || r > std::min(Y.n, Y.m)) throw EngineError("internal error: rank outside its bounds");
        Y.r = r;
        Y.basis.assign(hpivcol.begin() + Y.pivoff, hpivcol.begin() + Y.pivoff + r);
        for (int k = 0; k < r; k++)
            if (Y.basis[(size_t)k] < 0 || Y.basis[(size_t)k] >= Y.n || (k > 0 && Y.basis[(size_t)k] <= Y.basis[(size_t)k - 1])) throw EngineError("internal error: the pivot columns do not ascend");
        solver_shape(Y.m, r, Y.cls, Y.ldg, Y.q);
    }
    S->info[5] += nj;
    S->info[6] += launches;
    S->info[7] += (i64)(ev.ms(0, 1) * 1000.0);
}

// the general path of a system: its factorization with L, the pivotal rows of which carry the solutions
void solver_factor_slow(SolverSys &Y, const struct spasm_csr *A)
{
    Y.lu = solve_slow_factor(A);
    Y.r = (int)Y.lu->r;
    Y.basis.assign(Y.lu->p, Y.lu->p + Y.r);
    std::sort(Y.basis.begin(), Y.basis.end());
}

void solver_finish_info(spasm_amd_solver *S)
{
    i64 *v = S->info;
    v[0] = (i64)S->sys.size();
    for (const SolverSys &Y : S->sys) {
        if (Y.kind == SOLVER_GENERAL) v[2]++;
        else v[1]++;
        if (Y.kind == SOLVER_LDS) v[3] += (i64)Y.m * Y.r;
        v[4] += Y.r;
    }
}

spasm_amd_solver *solver_create(int count, const struct spasm_csr *const *A)
{
    if (count < 0) throw EngineError("count < 0");
    std::unique_ptr<spasm_amd_solver> S(new spasm_amd_solver());
    if (count == 0) return S.release();
    if (!A) throw EngineError("NULL array");
    batch_check_list(count, A);
    S->sys.resize((size_t)count);
    std::vector<int> fast, slow;
    for (int i = 0; i < count; i++) {
        SolverSys &Y = S->sys[(size_t)i];
        Y.n = A[i]->n;
        Y.m = A[i]->m;
        Y.prime = A[i]->field->p;
        if (Y.n == 0 || Y.m == 0) Y.kind = SOLVER_EMPTY;
        else if (solve_fits(Y.n, Y.m)) { Y.kind = SOLVER_LDS; fast.push_back(i); }
        else { Y.kind = SOLVER_GENERAL; slow.push_back(i); }
    }
    if (!fast.empty() || !slow.empty()) {
        require_device();
        HIPCHK(hipGetDevice(&S->dev));
    }
    if (!fast.empty()) {
        BatchStaged in;
        batch_stage_items(A, fast, in);
        solver_factor(S.get(), fast, in.row0, in.P, in.J, in.X);
    }
    for (int i : slow) solver_factor_slow(S->sys[(size_t)i], A[i]);
    solver_finish_info(S.get());
    return S.release();
}

template <class T> void solver_copy_map(DevBuf<T> &dst, const DevBuf<T> &src, size_t cnt, hipStream_t s)
{
    dst.alloc(cnt);
    if (cnt > 0) HIPCHK(hipMemcpyAsync(dst.p, src.p, cnt * sizeof(T), hipMemcpyDeviceToDevice, s));
}

// the operators of all blocks from the resident concatenated CSR; only a block over the limit is fetched
spasm_amd_solver *solver_create_blocks(const spasm_amd_blocks *B)
{
    blocks_need(B);
    HIPCHK(hipSetDevice(B->dev));
    hipStream_t s = nullptr;
    std::unique_ptr<spasm_amd_solver> S(new spasm_amd_solver());
    S->blocks = true;
    S->dev = B->dev;
    S->n = B->n;
    S->m = B->m;
    S->nb = B->nb;
    S->prime = B->prime;
    S->h_row_start = B->h_row_start;
    S->h_col_start = B->h_col_start;
    solver_copy_map(S->col_block, B->col_block, (size_t)B->m, s);
    solver_copy_map(S->col_pos, B->col_pos, (size_t)B->m, s);
    solver_copy_map(S->block_rows, B->block_rows, (size_t)B->n, s);
    solver_copy_map(S->row_start, B->row_start, (size_t)B->nb + 1, s);
    // the dense apply reads B through the columns of a block in the block's order: the inverse of (col_block, col_pos)
    S->block_cols.alloc((size_t)B->m);
    if (B->m > 0) {
        hipLaunchKernelGGL(k_solver_block_cols, dim3(cdiv(B->m, 256)), dim3(256), 0, s, B->m, S->col_block.p, S->col_pos.p, B->col_start.p, S->block_cols.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    S->sys.resize((size_t)B->nb);
    std::vector<int> fast, slow;
    std::vector<i64> row0;
    for (int b = 0; b < B->nb; b++) {
        SolverSys &Y = S->sys[(size_t)b];
        Y.n = (int)(B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b]);
        Y.m = (int)(B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b]);
        Y.prime = B->prime;
        if (Y.n == 0 || Y.m == 0) Y.kind = SOLVER_EMPTY;
        else if (solve_fits(Y.n, Y.m)) {
            Y.kind = SOLVER_LDS;
            fast.push_back(b);
            row0.push_back(B->h_row_start[(size_t)b] + b);
        } else {
            Y.kind = SOLVER_GENERAL;
            slow.push_back(b);
        }
    }
    solver_factor(S.get(), fast, row0, B->P.p, B->J.p, B->X.p);
    for (int b : slow) {
        struct spasm_csr *M = blocks_fetch(B, b);
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Mguard(M, spasm_csr_free);
        solver_factor_slow(S->sys[(size_t)b], M);
    }
    solver_finish_info(S.get());
    return S.release();
}

// The apply jobs of the systems sys[f] (K right-hand sides each, from brow0 / slot0) of the handle's systems which[f]: slabs of
// kSolverRounds * q right-hand sides.  A slot holds at most r + 1 entries.
void solver_jobs(const spasm_amd_solver *S, const std::vector<SolveSys> &sys, const std::vector<int> &which, std::vector<SolverApplyDesc> &desc,
                 std::vector<unsigned char> &cls, std::vector<i64> &ecap)
{
    for (size_t f = 0; f < sys.size(); f++) {
        const SolverSys &Y = S->sys[(size_t)which[f]];
        const int w = kSolverRounds * Y.q;
        for (int t0 = 0; t0 < sys[f].K; t0 += w) {
            SolverApplyDesc d;
            memset(&d, 0, sizeof d);
            d.goff = Y.goff;
            d.pivoff = Y.pivoff;
            d.brow0 = sys[f].brow0 + t0;
            d.slot0 = sys[f].slot0 + t0;
            d.m = Y.m;
            d.r = Y.r;
            d.ldg = Y.ldg;
            d.w = std::min(w, sys[f].K - t0);
            d.q = Y.q;
            d.F = zp_field_make(Y.prime);
            desc.push_back(d);
            cls.push_back((unsigned char)Y.cls);
            ecap.push_back((i64)d.w * (Y.r + 1));
        }
    }
}

SolverApplyArgs solver_args(const spasm_amd_solver *S, const i64d *BP, const int *BJ, const int *BX)
{
    SolverApplyArgs a;
    memset(&a, 0, sizeof a);
    a.G = S->G.p;
    a.pivrow = S->pivrow.p;
    a.pivcol = S->pivcol.p;
    a.BP = BP; a.BJ = BJ; a.BX = BX;
    return a;
}

void solver_need(const spasm_amd_solver *S, bool blocks)
{
    if (!S) throw EngineError("NULL handle");
    if (S->blocks != blocks) throw EngineError(blocks ? "the handle was made by spasm_amd_solver_create: use spasm_amd_solver_apply" : "the handle was made by spasm_amd_solver_create_blocks: use spasm_amd_solver_apply_blocks");
}

// Nothing is written to X / ok before all is done, and the handle is only read.
void solver_apply_run(spasm_amd_solver *S, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok)
{
    memset(g_solver_stats, 0, sizeof g_solver_stats);
    solver_need(S, false);
    const int count = (int)S->sys.size();
    if (count == 0) return;
    if (!B || !X || !ok) throw EngineError("NULL array");
    char msg[200];
    for (int i = 0; i < count; i++) {
        const SolverSys &Y = S->sys[(size_t)i];
        const char *bad = batch_check(B[i]);
        if (!bad && Y.prime != B[i]->field->p) bad = "the primes of A and B differ";
        if (!bad && B[i]->m != Y.m) bad = "B->m != A->m";
        if (!bad && B[i]->n > 0 && !ok[i]) bad = "NULL array (ok)";
        if (bad) {
            snprintf(msg, sizeof msg, "matrix %d (B): %s", i, bad);
            throw EngineError(msg);
        }
    }
    i64 *st = g_solver_stats;
    st[0] = count;
    CsrList res;
    res.v.assign((size_t)count, nullptr);
    std::vector<std::vector<unsigned char>> oks((size_t)count);
    std::vector<int> fast, slow;
    for (int i = 0; i < count; i++) {
        const SolverSys &Y = S->sys[(size_t)i];
        const int K = B[i]->n;
        oks[(size_t)i].assign((size_t)K, 1);
        if (Y.kind == SOLVER_GENERAL && K > 0) { slow.push_back(i); continue; }
        if (Y.kind == SOLVER_LDS && Y.r > 0 && K > 0) { fast.push_back(i); continue; }
        // no launch: without rows, or with rows that vanish, only the zero row is reachable; without columns everything is
        const ZpField F = zp_field_make(Y.prime);
        for (int k = 0; k < K && Y.m > 0; k++)
            for (i64 e = B[i]->p[k]; e < B[i]->p[k + 1]; e++)
                if (zp_reduce(F, (int64_t)B[i]->x[e]) != 0) oks[(size_t)i][(size_t)k] = 0;
        res.v[(size_t)i] = spasm_csr_alloc(K, Y.n, 0, Y.prime, true);
        if (!res.v[(size_t)i]) throw EngineError("out of host memory");
        for (int k = 0; k <= K; k++) res.v[(size_t)i]->p[k] = 0;
        st[Y.kind == SOLVER_GENERAL ? 2 : 1]++;
    }
    if (!fast.empty() || !slow.empty()) HIPCHK(hipSetDevice(S->dev));
    st[1] += (i64)fast.size();
    st[2] += (i64)slow.size();
    if (!fast.empty()) {
        BatchStaged inb;
        const std::vector<BatchItem> ib = batch_stage_items(B, fast, inb);
        std::vector<SolveSys> sys;
        i64 nslots = 0;
        for (size_t f = 0; f < fast.size(); f++) {
            const SolverSys &Y = S->sys[(size_t)fast[f]];
            sys.push_back(SolveSys{Y.n, Y.m, ib[f].n, 0, ib[f].row0, nslots, Y.prime});
            nslots += ib[f].n;
        }
        std::vector<SolverApplyDesc> desc;
        std::vector<unsigned char> cls;
        std::vector<i64> ecap;
        solver_jobs(S, sys, fast, desc, cls, ecap);
        st[3] = (i64)desc.size();
        std::vector<int> h_cnt;
        std::vector<unsigned char> h_ok;
        std::vector<int2> h_ent;
        solve_chunks(kSolverApply, desc, cls, ecap, solver_args(S, inb.P, inb.J, inb.X), nslots, h_cnt, h_ok, h_ent, st);
        i64 at = 0;
        for (size_t f = 0; f < fast.size(); f++) {
            const int i = fast[f], K = sys[f].K;
            res.v[(size_t)i] = batch_rows_to_csr(K, sys[f].n, sys[f].prime, h_cnt.data() + sys[f].slot0, h_ent.data(), (i64)h_ent.size(), at);
            memcpy(oks[(size_t)i].data(), h_ok.data() + sys[f].slot0, (size_t)K);
        }
    }
    for (int i : slow) res.v[(size_t)i] = solve_slow_with(S->sys[(size_t)i].lu, S->sys[(size_t)i].n, S->sys[(size_t)i].prime, B[i], oks[(size_t)i].data());
    for (int i = 0; i < count; i++)
        for (unsigned char v : oks[(size_t)i]) st[7] += v ? 0 : 1;
    for (int i = 0; i < count; i++)
        if (!oks[(size_t)i].empty()) memcpy(ok[i], oks[(size_t)i].data(), oks[(size_t)i].size());
    memcpy(X, res.v.data(), sizeof(struct spasm_csr *) * (size_t)count);
    res.v.clear();
}

// spasm_amd_solver_apply_blocks: the blocks a right-hand side meets are applied, not eliminated.  A block whose entries all vanish
// mod p (rank 0) is launched like the others: its job is the zero test.
struct BlocksApplyOps : BlocksSolveOps {
    const spasm_amd_solver *S;
    std::vector<SolverApplyDesc> desc;
    std::vector<unsigned char> cls;
    explicit BlocksApplyOps(const spasm_amd_solver *S_) : S(S_) {}
    bool fits(int b, i64, i64) override { return S->sys[(size_t)b].kind == SOLVER_LDS; }
    i64 plan(const std::vector<SolveSys> &sys, const std::vector<int> &blk, int &njobs) override
    {
        std::vector<i64> ecap;
        desc.clear();
        cls.clear();
        solver_jobs(S, sys, blk, desc, cls, ecap);
        njobs = (int)desc.size();
        i64 ents = 0;
        for (int q = 0; q < njobs; q++) { desc[(size_t)q].slice = ents; ents += ecap[(size_t)q]; }
        return ents;
    }
    struct spasm_csr *slow(int b, const struct spasm_csr *Rb, unsigned char *okb) override
    {
        const SolverSys &Y = S->sys[(size_t)b];
        return solve_slow_with(Y.lu, Y.n, Y.prime, Rb, okb);
    }
    i64 launch(const i64d *run_start, const int *sj, const int *sx, int *cnt, i64d *src, unsigned char *ok, int2 *scratch, hipStream_t s) override
    {
        const int nj = (int)desc.size();
        DevBuf<SolverApplyDesc> d_desc;
        DevBuf<int> d_items;
        d_desc.alloc((size_t)nj);
        d_items.alloc((size_t)nj);
        HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nj * sizeof(SolverApplyDesc), hipMemcpyHostToDevice, s));
        std::vector<int> items((size_t)nj);
        SolverApplyArgs a = solver_args(S, run_start, sj, sx);
        a.desc = d_desc.p;
        a.cnt = cnt;
        a.src = src;
        a.ok = ok;
        a.scratch = scratch;
        const i64 launches = batch_launch_jobs(kSolverApply, cls, 0, nj, items, d_items.p, a, nullptr, s);
        HIPCHK(hipStreamSynchronize(s)); // (items and the buffers belong to this scope)
        return launches;
    }
};

void solver_apply_blocks_run(spasm_amd_solver *S, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok)
{
    memset(g_solver_stats, 0, sizeof g_solver_stats);
    solver_need(S, true);
    BlocksApplyOps ops(S);
    const BlocksView V{S->nb, S->prime, S->col_block.p, S->col_pos.p, S->block_rows.p, S->row_start.p, &S->h_row_start, &S->h_col_start};
    solve_blocks_apply(V, S->n, S->m, S->dev, ops, g_solver_stats, Rhs, X, ok);
}

// ---- the dense apply (solver.hpp, "The dense apply"): spasm_amd_solver_apply_dense / _dev.  One matrix per handle: A of the split,
// or diag(A_0 .. A_{count-1}) of a list, system i on rows sum_{j<i} m_j .. of B and sum_{j<i} n_j .. of X.
void solver_dense_dims(const spasm_amd_solver *S, i64 &N, i64 &M)
{
    N = S->n;
    M = S->m;
    if (S->blocks) return;
    for (const SolverSys &Y : S->sys) { N += Y.n; M += Y.m; }
}

// Class, stride and tiles in flight of the dense apply of an m x r operator: G, the m words of the order of the rows and q tiles
// of r * T words, each part rounded up to 16 bytes.  The odd stride where it fits the largest class; q = at most one tile per group
// of whole waves that covers m.  Without rank nothing lies in LDS.
void solver_dense_shape(int m, int r, int &cls, int &ldg, int &q)
{
    constexpr int T = SOLVER_DENSE_T;
    const int mp = m > 64 ? (m + 63) & ~63 : 64;
    if (r == 0) {
        cls = 0;
        ldg = 1;
        q = std::max(kBatchClass[0].bs / mp, 1);
        return;
    }
    auto fixed = [&](int ld) { return (((i64)m * ld + 3) & ~(i64)3) + (((i64)m + 3) & ~(i64)3); };
    const i64 tile = (i64)r * T;
    ldg = r;
    if (ldg % 2 == 0 && fixed(ldg + 1) + tile <= kBatchClass[BATCH_NCLASS - 1].cap) ldg++;
    const i64 need = fixed(ldg) + tile;
    int c = 0;
    while (c < BATCH_NCLASS - 1 && need > kBatchClass[c].cap) c++;
    if (need > kBatchClass[c].cap) throw EngineError("internal error: an operator and a tile of right-hand sides do not fit the largest class");
    const int bs = kBatchClass[c].bs;
    q = mp <= bs ? (int)std::min<i64>(bs / mp, (kBatchClass[c].cap - fixed(ldg)) / tile) : 1;
    cls = c;
}

// The plan of an apply of K columns: one job per (system, slab of kSolverRounds * q tiles), sorted by class, on the device.  Kept in
// the handle until another K comes: an apply with the K of the plan uploads and allocates nothing.  Another K overwrites the
// buffers of the plan in place, and an earlier apply may still be queued on a stream that the copies below do not wait for (a
// non-blocking stream): the rebuild therefore waits for the device first, so that an apply in flight ends on the plan it began with.
void solver_dense_plan(spasm_amd_solver *S, int K, hipStream_t s)
{
    spasm_amd_solver::DensePlan &P = S->dense;
    if (P.K == K) return;
    // (a capture can neither wait for the device nor take the blocking copies below: refused before anything is touched)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
        char msg[200];
        snprintf(msg, sizeof msg, "the stream is capturing and the handle holds no plan for K = %d: apply once with this K before the capture", K);
        throw EngineError(msg);
    }
    P.K = 0;
    if (S->dense_built > 0) HIPCHK(hipDeviceSynchronize());
    std::vector<SolverDenseDesc> desc;
    std::vector<unsigned char> cls;
    i64 brow = 0, xrow = 0;
    for (size_t i = 0; i < S->sys.size(); i++) {
        const SolverSys &Y = S->sys[i];
        if (S->blocks) {
            brow = S->h_col_start[i];
            xrow = S->h_row_start[i];
        }
        int c = 0, ldg = 1, q = 1;
        solver_dense_shape(Y.m, Y.r, c, ldg, q);
        const i64 w = (i64)kSolverRounds * q * SOLVER_DENSE_T;
        for (i64 v0 = 0; v0 < K; v0 += w) {
            SolverDenseDesc d;
            memset(&d, 0, sizeof d);
            d.goff = Y.goff;
            d.pivoff = Y.pivoff;
            d.brow = brow;
            d.xrow = xrow;
            d.okoff = (i64)i * K;
            d.n = Y.n;
            d.m = Y.m;
            d.r = Y.r;
            d.ldg = ldg;
            d.v0 = (int)v0;
            d.w = (int)std::min<i64>(w, K - v0);
            d.q = q;
            d.F = zp_field_make(Y.prime);
            desc.push_back(d);
            cls.push_back((unsigned char)c);
        }
        brow += Y.m;
        xrow += Y.n;
    }
    const int nj = (int)desc.size();
    int at[BATCH_NCLASS], sum = 0;
    for (int k = 0; k < BATCH_NCLASS; k++) P.hist[k] = 0;
    for (int j = 0; j < nj; j++) P.hist[cls[(size_t)j]]++;
    for (int k = 0; k < BATCH_NCLASS; k++) { at[k] = sum; sum += P.hist[k]; }
    std::vector<int> items((size_t)nj);
    for (int j = 0; j < nj; j++) items[(size_t)at[cls[(size_t)j]]++] = j;
    P.desc.ensure((size_t)nj);
    P.items.ensure((size_t)nj);
    if (S->blocks) P.flag.ensure((size_t)K);
    if (nj > 0) {
        HIPCHK(hipMemcpy(P.desc.p, desc.data(), (size_t)nj * sizeof(SolverDenseDesc), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(P.items.p, items.data(), (size_t)nj * sizeof(int), hipMemcpyHostToDevice));
    }
    P.njobs = nj;
    P.launches = S->blocks ? 1 : 0; // (the finishing kernel)
    for (int k = 0; k < BATCH_NCLASS; k++) P.launches += P.hist[k] > 0 ? 1 : 0;
    P.K = K;
    S->dense_built++;
}

// Do the windows of B (M rows of K words, ldb apart) and X (N rows, ldx apart) share a byte?  Row by row, not by their extents:
// two windows side by side in one array (ldb, ldx > K) interleave without sharing a word.  The rows are walked only where the
// extents meet.
bool solver_dense_overlap(const void *B, i64 M, i64 ldb, const void *X, i64 N, i64 ldx, i64 K)
{
    const i64 len = K * (i64)sizeof(int), rowb = ldb * (i64)sizeof(int), rowx = ldx * (i64)sizeof(int);
    const uintptr_t b0 = (uintptr_t)B, b1 = b0 + (uintptr_t)((M - 1) * rowb + len);
    const uintptr_t x0 = (uintptr_t)X, x1 = x0 + (uintptr_t)((N - 1) * rowx + len);
    if (!(b0 < x1 && x0 < b1)) return false;
    auto floordiv = [](i64 a, i64 b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); };
    for (i64 i = 0; i < M; i++) {
        // row j of X meets row i of B iff |d - j * rowx| < len, d = the distance of row i of B from the first word of X
        const i64 d = (i64)(b0 - x0) + i * rowb;
        const i64 lo = std::max<i64>(floordiv(d - len, rowx) + 1, 0), hi = std::min<i64>(-floordiv(-(d + len), rowx) - 1, N - 1);
        if (lo <= hi) return true;
    }
    return false;
}

// The checks that need no device, in the order of the header.  false: nothing to do (no system, or no column).
bool solver_dense_check(const spasm_amd_solver *S, int K, const void *B, i64 ldb, const void *X, i64 ldx, const void *ok)
{
    if (!S) throw EngineError("NULL handle");
    if (K < 0) throw EngineError("K < 0");
    if (ldb < K) throw EngineError("ldb < K");
    if (ldx < K) throw EngineError("ldx < K");
    if (K == 0 || (S->sys.empty() && !S->blocks)) return false;
    for (size_t i = 0; i < S->sys.size(); i++)
        if (S->sys[i].kind == SOLVER_GENERAL) {
            char msg[200];
            snprintf(msg, sizeof msg, "system %zu is over the limit of the LDS path (general path): the dense apply does not take it", i);
            throw EngineError(msg);
        }
    i64 N = 0, M = 0;
    solver_dense_dims(S, N, M);
    if ((M > 0 && !B) || (N > 0 && !X) || !ok) throw EngineError("NULL array");
    if (M > 0 && N > 0 && solver_dense_overlap(B, M, ldb, X, N, ldx, K)) throw EngineError("B and X overlap");
    return true;
}

// everything on stream s: the flags (a blocks handle), one launch per class that occurs, the finishing kernel (a blocks handle)
void solver_dense_enqueue(spasm_amd_solver *S, int K, const int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok, hipStream_t s)
{
    solver_dense_plan(S, K, s);
    const spasm_amd_solver::DensePlan &P = S->dense;
    SolverDenseArgs a;
    memset(&a, 0, sizeof a);
    a.desc = P.desc.p;
    a.G = S->G.p;
    a.pivrow = S->pivrow.p;
    a.pivcol = S->pivcol.p;
    a.B = B;
    a.ldb = ldb;
    a.X = X;
    a.ldx = ldx;
    if (S->blocks) {
        a.colmap = S->block_cols.p;
        a.rowmap = S->block_rows.p;
        a.flag = P.flag.p;
        HIPCHK(hipMemsetAsync(P.flag.p, 0, (size_t)K * sizeof(unsigned), s));
    } else a.ok = ok;
    int first = 0;
    for (int k = 0; k < BATCH_NCLASS; k++) {
        if (P.hist[k] > 0) batch_launch_class(kSolverDense, k, a, P.items.p + first, P.hist[k], s);
        first += P.hist[k];
    }
    if (S->blocks) {
        const i64 words = (i64)std::max(S->n, 1) * K;
        hipLaunchKernelGGL(k_solver_dense_finish, dim3(cdiv(words, 256)), dim3(256), 0, s, S->n, K, P.flag.p, ok, X, (i64d)ldx);
        HIPCHK(hipGetLastError());
    }
}

void solver_apply_dense_dev(spasm_amd_solver *S, int K, const int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok, hipStream_t s)
{
    if (!solver_dense_check(S, K, B, ldb, X, ldx, ok)) return;
    require_device();
    HIPCHK(hipSetDevice(S->dev));
    solver_dense_enqueue(S, K, B, ldb, X, ldx, ok, s);
    if (!s) HIPCHK(hipStreamSynchronize(s));
}

// host arrays: upload the window of B, the apply on the NULL stream, download the window of X and ok
void solver_apply_dense_host(spasm_amd_solver *S, int K, const int *B, i64 ldb, int *X, i64 ldx, unsigned char *ok)
{
    if (!solver_dense_check(S, K, B, ldb, X, ldx, ok)) return;
    if (S->sys.empty()) { // the split of a matrix without rows and columns: 0 = 0 holds for every column, and no device is needed
        memset(ok, 1, (size_t)K);
        return;
    }
    require_device();
    HIPCHK(hipSetDevice(S->dev));
    i64 N = 0, M = 0;
    solver_dense_dims(S, N, M);
    const size_t nok = S->blocks ? (size_t)K : S->sys.size() * (size_t)K, line = (size_t)K * sizeof(int);
    DevBuf<int> dB, dX;
    DevBuf<unsigned char> dok;
    dB.alloc((size_t)M * K);
    dX.alloc((size_t)N * K);
    dok.alloc(nok);
    if (M > 0) HIPCHK(hipMemcpy2D(dB.p, line, B, (size_t)ldb * sizeof(int), line, (size_t)M, hipMemcpyHostToDevice));
    solver_dense_enqueue(S, K, dB.p, K, dX.p, K, dok.p, nullptr);
    HIPCHK(hipStreamSynchronize(nullptr));
    std::vector<unsigned char> hok(nok);
    HIPCHK(hipMemcpy(hok.data(), dok.p, nok, hipMemcpyDeviceToHost));
    if (N > 0) HIPCHK(hipMemcpy2D(X, (size_t)ldx * sizeof(int), dX.p, line, line, (size_t)N, hipMemcpyDeviceToHost));
    memcpy(ok, hok.data(), nok);
}

} // namespace

// ================================================================================================
// C ABI: every entry point that can fail is one abi_call (above, beside HIPCHK)
// ================================================================================================

extern "C" {

SPASM_API int spasm_amd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

SPASM_API int spasm_amd_set_device(int dev)
{
    if (hipSetDevice(dev) != hipSuccess) { spasm_set_error("hipSetDevice(%d) failed", dev); return 1; }
    return 0;
}

// engine extension of spasm_echelonize (reference src/SpaSM.jl:863): the same result from `nshards` row shards on the devices of
// this process (include/spasm_amd.h)
SPASM_API struct spasm_lu *spasm_amd_echelonize_multi(const struct spasm_csr *A, struct echelonize_opts *opts, int nshards)
{
    return abi_call<struct spasm_lu *>("spasm_amd_echelonize_multi", nullptr, [&] { return do_echelonize_multi(A, opts, nshards); });
}

// reference src/SpaSM.jl:863
SPASM_API struct spasm_lu *spasm_echelonize(const struct spasm_csr *A, struct echelonize_opts *opts)
{
    return abi_call<struct spasm_lu *>("spasm_echelonize", nullptr, [&] { return do_echelonize(A, opts); });
}

// rank(A) = rank(echelonize(A)) (reference src/SpaSM.jl:1149) without the rows of U ever leaving the device; -1 on error
SPASM_API i64 spasm_amd_rank(const struct spasm_csr *A, struct echelonize_opts *opts)
{
    return abi_call<i64>("spasm_amd_rank", -1, [&] {
        struct echelonize_opts o;
        if (opts) o = *opts;
        else spasm_echelonize_init_opts(&o);
        if (o.L) throw EngineError("the L factor needs the rows of U");
        i64 r = -1;
        (void)do_echelonize(A, &o, &r);
        return r;
    });
}

// reference src/SpaSM.jl:879
SPASM_API struct spasm_csr *spasm_kernel(const struct spasm_lu *fact)
{
    return abi_call<struct spasm_csr *>("spasm_kernel", nullptr, [&] { return do_kernel(fact); });
}

SPASM_API struct spasm_csr *spasm_amd_kernel_strided(const struct spasm_lu *fact, int first, int step)
{
    return abi_call<struct spasm_csr *>("spasm_amd_kernel_strided", nullptr, [&] { return do_kernel(fact, first, step); });
}

// reference src/SpaSM.jl:694-722: x * U = B[k] for ONE row.  The row goes through the batched device solve (do_trisolve: the Schur
// machinery with U as the pivot rows), then the solution is laid out as libspasm does: x scattered over the m columns (x_b on the
// pivot columns, x_a on the others; only the entries of the pattern are written), the pattern in xj[top .. m), top returned.
// Pattern order: the pivot columns reached, then the columns of x_a, each ascending.  xj[0 .. top) and xj[m .. 3m) (libspasm's
// DFS stacks and marks, "it remains OK", :700) are left as they are.  -1 on failure.
SPASM_API int spasm_sparse_triangular_solve(const struct spasm_csr *U, const struct spasm_csr *B, int k, int *xj, spasm_ZZp *x, const int *qinv)
{
    return abi_call("spasm_sparse_triangular_solve", -1, [&] {
        if (!U || !B || !xj || !x || !qinv) throw EngineError("spasm_sparse_triangular_solve: null argument");
        if (k < 0 || k >= B->n) throw EngineError("spasm_sparse_triangular_solve: row out of range");
        const int m = U->m;
        // row k of B as a matrix of its own (borrowed arrays)
        i64 rp[2] = {0, B->p[k + 1] - B->p[k]};
        struct spasm_csr one = *B;
        one.n = 1;
        one.nzmax = rp[1];
        one.p = rp;
        one.j = B->j + B->p[k];
        one.x = B->x + B->p[k];
        struct spasm_csr *resid = nullptr; // (set by do_trisolve as its last step)
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> X(do_trisolve(U, qinv, &one, nullptr, &resid), spasm_csr_free);
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Rs(resid, spasm_csr_free);
        std::vector<int> colof((size_t)std::max(U->n, 1), -1);
        for (int j = 0; j < m; j++) if (qinv[j] >= 0 && qinv[j] < U->n) colof[(size_t)qinv[j]] = j;
        std::vector<int> pat;
        for (i64 t = X->p[0]; t < X->p[1]; t++) { const int j = colof[(size_t)X->j[t]]; x[j] = X->x[t]; pat.push_back(j); }
        std::sort(pat.begin(), pat.end());
        const size_t npiv_pat = pat.size();
        for (i64 t = Rs->p[0]; t < Rs->p[1]; t++) { x[Rs->j[t]] = Rs->x[t]; pat.push_back(Rs->j[t]); }
        std::sort(pat.begin() + (long)npiv_pat, pat.end());
        const int top = m - (int)pat.size();
        for (size_t t = 0; t < pat.size(); t++) xj[(size_t)top + t] = pat[t];
        return top;
    }, ABI_NAMED_BELOW);
}

SPASM_API struct spasm_csr *spasm_amd_triangular_solve(const struct spasm_csr *U, const int *qinv, const struct spasm_csr *B, unsigned char *ok)
{
    return abi_call<struct spasm_csr *>("spasm_amd_triangular_solve", nullptr, [&] { return do_trisolve(U, qinv, B, ok); });
}

// reference src/SpaSM.jl:915-923
SPASM_API struct spasm_csr *spasm_gesv(const struct spasm_lu *fact, const struct spasm_csr *B, bool *ok)
{
    static_assert(sizeof(bool) == 1, "ok is an array of bytes");
    return abi_call<struct spasm_csr *>("spasm_gesv", nullptr, [&] { return do_gesv(fact, B, (unsigned char *)ok); });
}

// reference src/SpaSM.jl:895-905: x (n = rows of A entries) with x * A == b (m entries); false when there is no solution
// reference src/SpaSM.jl:928: the certificate of rank(A) >= fact->r (include/spasm_amd.h): rows = the pivotal rows, columns = the
// pivot columns, x = the Fiat-Shamir challenge, y with y * A[rows, columns] == x solved on the device (the r x r submatrix is
// echelonized with L, then the two triangular solves of spasm_solve).  NULL on failure (e.g. when U is not of full rank r on A).
SPASM_API struct spasm_rank_certificate *spasm_certificate_rank_create(const struct spasm_csr *A, const uint8_t *hash, const struct spasm_lu *fact)
{
    return abi_call<struct spasm_rank_certificate *>("spasm_certificate_rank_create", nullptr, [&] {
        // (the temporaries are freed while the exception unwinds, so the error text is set after spasm_solve and the frees)
        std::unique_ptr<struct spasm_rank_certificate, void (*)(struct spasm_rank_certificate *)> P(nullptr, spasm_rank_certificate_free);
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Cm(nullptr, spasm_csr_free);
        std::unique_ptr<struct spasm_lu, void (*)(struct spasm_lu *)> fc(nullptr, spasm_lu_free);
        if (!A || !hash || !fact || !fact->U || !fact->qinv || !fact->p) throw EngineError("null argument");
        const int r = fact->r, n = A->n, m = A->m;
        const i64 prime = A->field->p;
        if (fact->U->m != m || r > n || r > m) throw EngineError("the factorization does not belong to this matrix");
        P.reset((struct spasm_rank_certificate *)calloc(1, sizeof *P));
        if (!P) throw EngineError("out of host memory");
        P->r = r;
        P->prime = prime;
        memcpy(P->hash, hash, 32);
        P->i = (int *)malloc(sizeof(int) * (size_t)std::max(r, 1));
        P->j = (int *)malloc(sizeof(int) * (size_t)std::max(r, 1));
        P->x = (spasm_ZZp *)calloc((size_t)std::max(r, 1), sizeof(spasm_ZZp));
        P->y = (spasm_ZZp *)calloc((size_t)std::max(r, 1), sizeof(spasm_ZZp));
        if (!P->i || !P->j || !P->x || !P->y) throw EngineError("out of host memory");
        std::vector<int> pos((size_t)std::max(m, 1), -1);
        for (int j = 0; j < m; j++) {
            const int k = fact->qinv[j];
            if (k >= 0) { if (k >= r) throw EngineError("qinv names a row beyond the rank"); P->j[k] = j; pos[(size_t)j] = k; }
        }
        i64 cz = 0;
        for (int k = 0; k < r; k++) {
            const int i = fact->p[k];
            if (i < 0 || i >= n) throw EngineError("fact->p does not list the pivotal rows");
            P->i[k] = i;
            for (i64 t = A->p[i]; t < A->p[i + 1]; t++) cz += pos[(size_t)A->j[t]] >= 0;
        }
        spasm_cert_challenge(hash, prime, r, P->i, P->j, P->x);
        if (r == 0) return P.release();
        // C = A[rows, columns], r x r
        Cm.reset(spasm_csr_alloc(r, r, cz, prime, true));
        if (!Cm) throw EngineError("out of host memory");
        i64 w = 0;
        for (int k = 0; k < r; k++) {
            Cm->p[k] = w;
            const int i = P->i[k];
            for (i64 t = A->p[i]; t < A->p[i + 1]; t++) {
                const int c = pos[(size_t)A->j[t]];
                if (c >= 0) { Cm->j[w] = c; Cm->x[w] = A->x[t]; w++; }
            }
        }
        Cm->p[r] = w;
        struct echelonize_opts o;
        spasm_echelonize_init_opts(&o);
        o.L = true;
        o.enable_greedy_pivot_search = false;
        fc.reset(do_echelonize(Cm.get(), &o));
        if (!fc || fc->r != r) throw EngineError("the pivotal rows and pivot columns do not span a non-singular submatrix");
        if (!spasm_solve(fc.get(), P->x, P->y)) throw EngineError("the challenge has no solution (singular submatrix)");
        return P.release();
    });
}

SPASM_API bool spasm_solve(const struct spasm_lu *fact, const spasm_ZZp *b, spasm_ZZp *x)
{
    return abi_call("spasm_solve", false, [&] {
        if (!fact || !fact->U || !fact->L || !b || !x) throw EngineError("null argument (a factorization with L is needed)");
        const int m = fact->U->m, n = fact->L->n;
        const i64 prime = fact->U->field->p;
        const ZpField F = zp_field_make(prime);
        i64 nz = 0;
        for (int j = 0; j < m; j++) nz += zp_reduce(F, (int64_t)b[j]) != 0;
        struct spasm_csr *B = spasm_csr_alloc(1, m, nz, prime, true);
        if (!B) throw EngineError("out of host memory");
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> Bguard(B, spasm_csr_free);
        i64 w = 0;
        B->p[0] = 0;
        for (int j = 0; j < m; j++) {
            const int v = zp_reduce(F, (int64_t)b[j]);
            if (v != 0) { B->j[w] = j; B->x[w] = v; w++; }
        }
        B->p[1] = w;
        unsigned char ok = 0;
        struct spasm_csr *X = do_gesv(fact, B, &ok);
        for (int i = 0; i < n; i++) x[i] = 0;
        for (i64 q = X->p[0]; q < X->p[1]; q++) x[X->j[q]] = X->x[q];
        spasm_csr_free(X);
        return ok != 0;
    });
}

SPASM_API struct spasm_csr *spasm_rref(const struct spasm_lu *fact, int *Rqinv)
{
    return abi_call<struct spasm_csr *>("spasm_rref", nullptr, [&] { return do_rref(fact, Rqinv); });
}

// reference src/SpaSM.jl:589
SPASM_API struct spasm_csr *spasm_transpose(const struct spasm_csr *A)
{
    return abi_call<struct spasm_csr *>("spasm_transpose", nullptr, [&] { return do_transpose(A); });
}

SPASM_API spasm_amd_schur_plan *spasm_amd_schur_plan_create(const struct spasm_csr *A, int row_lo, int row_hi)
{
    return abi_call<spasm_amd_schur_plan *>("spasm_amd_schur_plan_create", nullptr, [&] { return plan_create(A, row_lo, row_hi); });
}

SPASM_API spasm_amd_schur_plan *spasm_amd_schur_plan_create_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride)
{
    return abi_call<spasm_amd_schur_plan *>("spasm_amd_schur_plan_create_strided", nullptr, [&] { return plan_create(A, row_lo, row_hi, stride); });
}

SPASM_API spasm_amd_shard *spasm_amd_shard_create_strided(const struct spasm_csr *A, int row_lo, int row_hi, int stride)
{
    return abi_call<spasm_amd_shard *>("spasm_amd_shard_create_strided", nullptr, [&] { return shard_create(A, row_lo, row_hi, stride); });
}

SPASM_API int spasm_amd_schur_plan_run(spasm_amd_schur_plan *plan, void *stream)
{
    return abi_call("spasm_amd_schur_plan_run", 1, [&] { plan_run(plan, (hipStream_t)stream); return 0; });
}

SPASM_API void spasm_amd_schur_plan_class_timing(spasm_amd_schur_plan *plan, int on)
{
    if (plan) plan->R.class_timing = on != 0;
}

SPASM_API int spasm_amd_schur_plan_stats(spasm_amd_schur_plan *plan, struct spasm_amd_round_stats *stats)
{
    return abi_call("spasm_amd_schur_plan_stats", 1, [&] {
        if (!plan->ran) throw EngineError("run the plan first");
        plan->R.fetch_counters();
        plan->R.hctr.applications = plan->exact_applications;
        plan->R.hctr.nnz_reduced = plan->exact_nnz_reduced;
        plan->R.hctr.segments = plan->exact_segments;
        fill_stats(*stats, plan->R, 0, plan->hi > plan->lo ? (plan->hi - plan->lo + plan->stride - 1) / plan->stride : 0, plan->nnz_in);
        return 0;
    });
}

SPASM_API struct spasm_csr *spasm_amd_schur_plan_fetch(spasm_amd_schur_plan *plan, int *p_out)
{
    return abi_call<struct spasm_csr *>("spasm_amd_schur_plan_fetch", nullptr, [&] { return plan_fetch(plan, p_out); });
}

SPASM_API struct spasm_csr *spasm_amd_schur_plan_fetch_U(spasm_amd_schur_plan *plan, int *pivcol_out, int *row_out)
{
    return abi_call<struct spasm_csr *>("spasm_amd_schur_plan_fetch_U", nullptr, [&] {
        if (!plan) throw EngineError("null plan");
        return plan_fetch_U(plan, pivcol_out, row_out);
    });
}

SPASM_API void spasm_amd_schur_plan_free(spasm_amd_schur_plan *plan) { delete plan; }

SPASM_API spasm_amd_shard *spasm_amd_shard_create(const struct spasm_csr *A, int row_lo, int row_hi)
{
    return abi_call<spasm_amd_shard *>("spasm_amd_shard_create", nullptr, [&] { return shard_create(A, row_lo, row_hi); });
}

SPASM_API int spasm_amd_shard_elect(spasm_amd_shard *sh, int64_t *keys_dev)
{
    return abi_call("spasm_amd_shard_elect", 1, [&] { shard_elect(sh, keys_dev); return 0; });
}

SPASM_API int spasm_amd_shard_set_keys(spasm_amd_shard *sh, const int64_t *keys_dev, int *n_owned, i64 *nnz_owned)
{
    return abi_call("spasm_amd_shard_set_keys", -1, [&] { return shard_set_keys(sh, keys_dev, n_owned, nnz_owned); });
}

SPASM_API int spasm_amd_shard_assign(spasm_amd_shard *sh, const int64_t *keys_dev)
{
    return abi_call("spasm_amd_shard_assign", -1, [&] { return shard_assign(sh, keys_dev); });
}

SPASM_API int spasm_amd_shard_open_step(spasm_amd_shard *sh, int step, int pass, const void *in_dev, void *out_dev)
{
    return abi_call("spasm_amd_shard_open_step", -1, [&] { return shard_open_step(sh, step, pass, in_dev, out_dev); });
}

SPASM_API int spasm_amd_shard_finish_keys(spasm_amd_shard *sh, int *n_owned, i64 *nnz_owned)
{
    return abi_call("spasm_amd_shard_finish_keys", -1, [&] { return shard_finish_keys(sh, n_owned, nnz_owned); });
}

SPASM_API int spasm_amd_shard_export(spasm_amd_shard *sh, int *hdr_dev, int *ent_dev)
{
    return abi_call("spasm_amd_shard_export", 1, [&] { shard_export(sh, hdr_dev, ent_dev); return 0; });
}

SPASM_API spasm_amd_schur_plan *spasm_amd_shard_import(spasm_amd_shard *sh, int n_rows, i64 n_entries, const int *hdr_dev, const int *ent_dev)
{
    return abi_call<spasm_amd_schur_plan *>("spasm_amd_shard_import", nullptr, [&] { return shard_import(sh, n_rows, n_entries, hdr_dev, ent_dev); });
}

SPASM_API spasm_amd_shard *spasm_amd_schur_plan_advance(spasm_amd_schur_plan *plan, int *rows_out, i64 *nnz_out)
{
    return abi_call<spasm_amd_shard *>("spasm_amd_schur_plan_advance", nullptr, [&] { return plan_advance(plan, rows_out, nnz_out); });
}

SPASM_API struct spasm_csr *spasm_amd_shard_fetch(spasm_amd_shard *sh)
{
    return abi_call<struct spasm_csr *>("spasm_amd_shard_fetch", nullptr, [&] { return shard_fetch(sh); });
}

SPASM_API void spasm_amd_shard_free(spasm_amd_shard *sh)
{
    if (!sh) return;
    delete sh->plan;
    delete sh;
}

// the device's field arithmetic on n test vectors (canonical residues a, b, c in; 8 results per vector out): see k_zp_probe
SPASM_API int spasm_amd_zp_probe(i64 prime, int n, const int *a, const int *b, const int *c, int *out)
{
    return abi_call("spasm_amd_zp_probe", 1, [&] {
        require_device();
        if (prime <= 2 || prime > 0xfffffffbLL || n < 0) throw EngineError("bad arguments");
        const ZpField F = zp_field_make(prime);
        DevBuf<int> da, db, dc, dout;
        da.alloc((size_t)n + 1); db.alloc((size_t)n + 1); dc.alloc((size_t)n + 1); dout.alloc((size_t)8 * n + 1);
        hipStream_t s = nullptr;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(da.p, a, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(db.p, b, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(dc.p, c, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            if (F.small) hipLaunchKernelGGL(k_zp_probe<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, da.p, db.p, dc.p, dout.p);
            else hipLaunchKernelGGL(k_zp_probe<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, da.p, db.p, dc.p, dout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)8 * n * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// count[i] lazy products a[i] * b[i] summed and reduced as the kernels do it (one result per triple): see k_zp_sum_probe
SPASM_API int spasm_amd_zp_sum_probe(i64 prime, int n, const int *a, const int *b, const int *count, int *out)
{
    return abi_call("spasm_amd_zp_sum_probe", 1, [&] {
        require_device();
        if (prime <= 2 || prime > 0xfffffffbLL || n < 0) throw EngineError("bad arguments");
        for (int i = 0; i < n; i++)
            if (count[i] < 0) throw EngineError("bad arguments (negative count)");
        const ZpField F = zp_field_make(prime);
        DevBuf<int> da, db, dc, dout;
        da.alloc((size_t)n + 1); db.alloc((size_t)n + 1); dc.alloc((size_t)n + 1); dout.alloc((size_t)n + 1);
        hipStream_t s = nullptr;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(da.p, a, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(db.p, b, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(dc.p, count, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            if (F.small) hipLaunchKernelGGL(k_zp_sum_probe<true>, dim3(cdiv(n, 64)), dim3(64), 0, s, F, n, da.p, db.p, dc.p, dout.p);
            else hipLaunchKernelGGL(k_zp_sum_probe<false>, dim3(cdiv(n, 64)), dim3(64), 0, s, F, n, da.p, db.p, dc.p, dout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// zp_reduce on chosen i64 values: where = 0 the host compilation of zp.hpp in a plain loop (no device needed), where = 1 k_zp_reduce_probe
SPASM_API int spasm_amd_zp_reduce_probe(i64 prime, int where, int n, const i64 *x, int *out)
{
    return abi_call("spasm_amd_zp_reduce_probe", 1, [&] {
        if (prime <= 2 || prime > 0xfffffffbLL || n < 0 || (where != 0 && where != 1)) throw EngineError("bad arguments");
        const ZpField F = zp_field_make(prime);
        if (where == 0) {
            for (int i = 0; i < n; i++) out[i] = zp_reduce(F, x[i]);
            return 0;
        }
        require_device();
        DevBuf<long long> dx;
        DevBuf<int> dout;
        dx.alloc((size_t)n + 1); dout.alloc((size_t)n + 1);
        hipStream_t s = nullptr;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_zp_reduce_probe, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, dx.p, dout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// the first six columns of spasm_amd_zp_probe (mul, axpy, add, sub, neg, inverse) from the host compilation of zp.hpp: no device needed
SPASM_API int spasm_amd_zp_field_probe_host(i64 prime, int n, const int *a, const int *b, const int *c, int *out)
{
    return abi_call("spasm_amd_zp_field_probe_host", 1, [&] {
        if (prime <= 2 || prime > 0xfffffffbLL || n < 0) throw EngineError("bad arguments");
        const ZpField F = zp_field_make(prime);
        for (int i = 0; i < n; i++) {
            const int x = a[i], y = b[i], z = c[i];
            int *o = out + (size_t)6 * i;
            o[0] = zp_mul(F, x, y);
            o[1] = zp_axpy(F, x, y, z);
            o[2] = zp_add(F, x, y);
            o[3] = zp_sub(F, x, y);
            o[4] = zp_neg(F, x);
            o[5] = x != 0 ? zp_inverse(F, x) : 0;
        }
        return 0;
    });
}

// the raw lazy products of n pairs, unreduced: see k_zp_lazy_probe
SPASM_API int spasm_amd_zp_lazy_probe(i64 prime, int n, const int *a, const int *b, i64 *out)
{
    return abi_call("spasm_amd_zp_lazy_probe", 1, [&] {
        require_device();
        if (prime <= 2 || prime > 0xfffffffbLL || n < 0) throw EngineError("bad arguments");
        const ZpField F = zp_field_make(prime);
        DevBuf<int> da, db;
        DevBuf<long long> dout;
        da.alloc((size_t)n + 1); db.alloc((size_t)n + 1); dout.alloc((size_t)n + 1);
        hipStream_t s = nullptr;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(da.p, a, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(db.p, b, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            if (F.small) hipLaunchKernelGGL(k_zp_lazy_probe<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, da.p, db.p, dout.p);
            else hipLaunchKernelGGL(k_zp_lazy_probe<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, da.p, db.p, dout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// the domain of zp_small_lazy as the kernels call it: p < 2^16, |x| <= 2^30 (a product of two 24-bit operands of ZpAcc<true>) and |x / p| < 2^22
static void zp_small_lazy_domain(i64 prime, i64 x_lo, i64 x_hi)
{
    if (prime <= 2 || prime >= 65536) throw EngineError("bad arguments (2 < p < 2^16 needed)");
    const i64 top = std::min<i64>((i64)1 << 30, (prime << 22) - 1);
    if (x_lo < -top || x_hi > top) throw EngineError("bad arguments (x outside the domain of zp_small_lazy)");
}

// the raw zp_small_lazy(x[i]) for p < 2^16: see k_zp_small_lazy_probe
SPASM_API int spasm_amd_zp_small_lazy_probe(i64 prime, int n, const int *x, int *out)
{
    return abi_call("spasm_amd_zp_small_lazy_probe", 1, [&] {
        require_device();
        if (n < 0) throw EngineError("bad arguments");
        i64 lo = 0, hi = 0;
        for (int i = 0; i < n; i++) { lo = std::min<i64>(lo, x[i]); hi = std::max<i64>(hi, x[i]); }
        zp_small_lazy_domain(prime, lo, hi);
        const ZpField F = zp_field_make(prime);
        DevBuf<int> dx, dout;
        dx.alloc((size_t)n + 1); dout.alloc((size_t)n + 1);
        hipStream_t s = nullptr;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_zp_small_lazy_probe, dim3(cdiv(n, 256)), dim3(256), 0, s, F, n, dx.p, dout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// zp_small_lazy over every x of [x_lo, x_hi], one record per chunk of consecutive values: see k_zp_small_lazy_scan
SPASM_API int spasm_amd_zp_small_lazy_scan(i64 prime, i64 x_lo, i64 x_hi, int chunk, int *tmax, int *tmin, int *bad)
{
    return abi_call("spasm_amd_zp_small_lazy_scan", 1, [&] {
        require_device();
        if (chunk <= 0 || x_hi < x_lo) throw EngineError("bad arguments");
        zp_small_lazy_domain(prime, x_lo, x_hi);
        const ZpField F = zp_field_make(prime);
        const i64 nchunks = (x_hi - x_lo) / chunk + 1;
        if (nchunks > ((i64)1 << 24)) throw EngineError("bad arguments (more than 2^24 chunks)");
        DevBuf<int> dmax, dmin, dbad;
        dmax.alloc((size_t)nchunks); dmin.alloc((size_t)nchunks); dbad.alloc((size_t)nchunks);
        hipStream_t s = nullptr;
        const int grid = (int)std::min<i64>(nchunks, 16384);
        hipLaunchKernelGGL(k_zp_small_lazy_scan, dim3(grid), dim3(64), 0, s, F, (long long)x_lo, (long long)x_hi, chunk, (int)nchunks, dmax.p, dmin.p, dbad.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tmax, dmax.p, (size_t)nchunks * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(tmin, dmin.p, (size_t)nchunks * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(bad, dbad.p, (size_t)nchunks * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

SPASM_API int spasm_amd_multi_last_finish(void) { return g_multi_finish; }

// ---- the dense finish over row shards, one process per shard (include/spasm_amd.h); no entry here switches the device
SPASM_API spasm_amd_schur_plan *spasm_amd_shard_import_U(spasm_amd_shard *sh, int n_rows, i64 n_entries, const int *hdr_dev, const int *ent_dev)
{
    return abi_call<spasm_amd_schur_plan *>("spasm_amd_shard_import_U", nullptr, [&] { return shard_import(sh, n_rows, n_entries, hdr_dev, ent_dev, false); });
}
SPASM_API int spasm_amd_schur_plan_prepare(spasm_amd_schur_plan *plan)
{
    return abi_call("spasm_amd_schur_plan_prepare", -1, [&] {
        if (!plan) throw EngineError("null plan");
        shard_import_finish(plan);
        return 0;
    });
}
SPASM_API spasm_amd_dshard *spasm_amd_dshard_open(spasm_amd_schur_plan *plan, int me, int nshards)
{
    return abi_call<spasm_amd_dshard *>("spasm_amd_dshard_open", nullptr, [&] { return dshard_open(plan, me, nshards); });
}
SPASM_API spasm_amd_dshard *spasm_amd_dshard_open_rows(spasm_amd_shard *sh, int me, int nshards)
{
    return abi_call<spasm_amd_dshard *>("spasm_amd_dshard_open_rows", nullptr, [&] { return dshard_open_rows(sh, me, nshards); });
}
SPASM_API int spasm_amd_dshard_flags(spasm_amd_dshard *ds, int *flags_dev)
{
    return abi_call("spasm_amd_dshard_flags", -1, [&] {
        dshard_opened(ds);
        HIPCHK(hipMemcpy(flags_dev, ds->cflag(), ((size_t)ds->plan->A.m + 1) * sizeof(int), hipMemcpyDeviceToDevice));
        return 0;
    });
}
SPASM_API double spasm_amd_dshard_density(spasm_amd_dshard *ds, const int *flags_dev, int free_cols, int *C_out)
{
    return abi_call("spasm_amd_dshard_density", -1.0, [&] {
        dshard_opened(ds);
        if (ds->fl) { // the rows as they are: the density is the matrix's own, which the caller knows; 1.0 = "dense, as you said"
            HIPCHK(hipMemcpy(ds->fl->cflag.p, flags_dev, ((size_t)ds->plan->A.m + 1) * sizeof(int), hipMemcpyDeviceToDevice));
            ds->C = ds->fl->finish_columns();
            if (C_out) *C_out = ds->C;
            return 1.0;
        }
        HIPCHK(hipMemcpy(ds->dw->cflag.p, flags_dev, ((size_t)ds->plan->A.m + 1) * sizeof(int), hipMemcpyDeviceToDevice));
        ds->C = ds->dw->finish_columns();
        if (C_out) *C_out = ds->C;
        Round &R = ds->plan->R;
        return ds->dw->estimate_density(R.np_rows.p, R.nnp, free_cols);
    });
}
SPASM_API int spasm_amd_dshard_build(spasm_amd_dshard *ds)
{
    return abi_call("spasm_amd_dshard_build", -1, [&] {
        dshard_opened(ds);
        if (ds->C <= 0) throw EngineError("no column left (call spasm_amd_dshard_density first)");
        if (ds->plan->R.F.p <= 255) ds->impl.reset(new DShardT<signed char>());
        else ds->impl.reset(new DShardT<short>());
        if (ds->fl) ds->impl->build_rows(ds->plan, *ds->fl, ds->me, ds->nshards, ds->C);
        else ds->impl->build(ds->plan, *ds->dw, ds->me, ds->nshards, ds->C);
        return 0;
    });
}
SPASM_API int spasm_amd_dshard_info(spasm_amd_dshard *ds, int *C_out, int *KB, i64 *ldc, int *elem, int *nd, int *cand_bytes)
{
    return abi_call("spasm_amd_dshard_info", -1, [&] {
        dshard_built(ds);
        if (C_out) *C_out = ds->C;
        ds->impl->info(KB, ldc, elem, nd);
        if (cand_bytes) *cand_bytes = (int)sizeof(CandRec);
        return 0;
    });
}
SPASM_API int spasm_amd_dshard_block_begin(spasm_amd_dshard *ds)
{
    return abi_call("spasm_amd_dshard_block_begin", -1, [&] { dshard_built(ds); ds->impl->block_begin(); return 0; });
}
SPASM_API int spasm_amd_dshard_candidates(spasm_amd_dshard *ds, int c0, int w, void *cand_dev)
{
    return abi_call("spasm_amd_dshard_candidates", -1, [&] { dshard_built(ds); ds->impl->candidates(c0, w, cand_dev); return 0; });
}
SPASM_API int spasm_amd_dshard_elect(spasm_amd_dshard *ds, const void *stack_dev, int w, int *npp, int *cnt, int *first)
{
    return abi_call("spasm_amd_dshard_elect", -1, [&] {
        dshard_built(ds);
        ds->impl->elect(stack_dev, w);
        if (npp) *npp = ds->impl->hglob.npp;
        for (int k = 0; k < ds->nshards; k++) {
            if (cnt) cnt[k] = ds->impl->hglob.cnt[k];
            if (first) first[k] = ds->impl->hglob.first[k];
        }
        return 0;
    });
}
SPASM_API i64 spasm_amd_dshard_pack(spasm_amd_dshard *ds, int c0, void *buf_dev)
{
    return abi_call<i64>("spasm_amd_dshard_pack", -1, [&] { dshard_built(ds); return ds->impl->pack(c0, buf_dev); });
}
SPASM_API int spasm_amd_dshard_unpack(spasm_amd_dshard *ds, int q, int c0, int owner, const void *buf_dev)
{
    return abi_call("spasm_amd_dshard_unpack", -1, [&] { dshard_built(ds); ds->impl->unpack(q, c0, owner, buf_dev); return 0; });
}
SPASM_API int spasm_amd_dshard_apply(spasm_amd_dshard *ds, int q, int c0, int w, int b1)
{
    return abi_call("spasm_amd_dshard_apply", -1, [&] { dshard_built(ds); ds->impl->apply(q, c0, w, b1); return 0; });
}
SPASM_API int spasm_amd_dshard_block_end(spasm_amd_dshard *ds, int b0, int b1, int npan)
{
    return abi_call("spasm_amd_dshard_block_end", -1, [&] { dshard_built(ds); ds->impl->block_end(b0, b1, npan); return 0; });
}
SPASM_API int spasm_amd_dshard_finish(spasm_amd_dshard *ds)
{
    return abi_call("spasm_amd_dshard_finish", -1, [&] { dshard_built(ds); return ds->impl->finish(); });
}
SPASM_API struct spasm_csr *spasm_amd_dshard_fetch_U(spasm_amd_dshard *ds, int *pivcol_out, int *row_out, int *n_out)
{
    return abi_call<struct spasm_csr *>("spasm_amd_dshard_fetch_U", nullptr, [&] { dshard_built(ds); return dshard_fetch_U(ds, pivcol_out, row_out, n_out); });
}
SPASM_API void spasm_amd_dshard_close(spasm_amd_dshard *ds) { delete ds; }

// reference src/SpaSM.jl:640-658 (axpy!, xapy!, A * x, x * A): host arrays; on failure y is left as it was
SPASM_API void spasm_Axpy(const struct spasm_csr *A, const spasm_ZZp *x, spasm_ZZp *y)
{
    abi_call("spasm_Axpy", [&] { spmv_once(A, 0, x, y, "spasm_Axpy"); });
}

SPASM_API void spasm_xApy(const spasm_ZZp *x, const struct spasm_csr *A, spasm_ZZp *y)
{
    abi_call("spasm_xApy", [&] { spmv_once(A, 1, x, y, "spasm_xApy"); });
}

SPASM_API spasm_amd_spmv *spasm_amd_spmv_create(const struct spasm_csr *A)
{
    return abi_call<spasm_amd_spmv *>("spasm_amd_spmv_create", nullptr, [&] { return spmv_create(A, "spasm_amd_spmv_create"); });
}

SPASM_API int spasm_amd_spmv_apply(spasm_amd_spmv *op, int trans, int k, const spasm_ZZp *X, i64 ldx, spasm_ZZp *Y, i64 ldy)
{
    return abi_call("spasm_amd_spmv_apply", -1, [&] {
        spmv_check(op, trans, k, X, ldx, Y, ldy, "spasm_amd_spmv_apply");
        DeviceGuard g(op);
        op->apply_host(trans, k, X, ldx, Y, ldy);
        return 0;
    });
}

SPASM_API int spasm_amd_spmv_apply_dev(spasm_amd_spmv *op, int trans, int k, const spasm_ZZp *X, i64 ldx, spasm_ZZp *Y, i64 ldy, void *stream)
{
    return abi_call("spasm_amd_spmv_apply_dev", -1, [&] {
        spmv_check(op, trans, k, X, ldx, Y, ldy, "spasm_amd_spmv_apply_dev");
        DeviceGuard g(op);
        hipStream_t s = (hipStream_t)stream;
        if (k > 0) op->apply_dev(trans, k, X, ldx, Y, ldy, s);
        if (!stream) HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

SPASM_API void spasm_amd_spmv_free(spasm_amd_spmv *op) { handle_free(op); }

// ---- sparse matrix algebra on resident matrices (spgemm.hpp; engine extension) ----
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_upload(const struct spasm_csr *A)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_upload", nullptr, [&] { return dcsr_upload(A, "upload"); });
}
SPASM_API struct spasm_csr *spasm_amd_dcsr_download(const spasm_amd_dcsr *D)
{
    return abi_call<struct spasm_csr *>("spasm_amd_dcsr_download", nullptr, [&] { dcsr_need(D, "download"); DeviceGuard g(D); return dcsr_download(D); });
}
SPASM_API void spasm_amd_dcsr_info(const spasm_amd_dcsr *D, i64 *out)
{
    if (!D || !out) return;
    out[0] = D->n;
    out[1] = D->m;
    out[2] = D->nnz;
    out[3] = D->F.p;
}
SPASM_API void spasm_amd_dcsr_stats(const spasm_amd_dcsr *D, i64 *out)
{
    if (!D || !out) return;
    memcpy(out, D->stats, sizeof D->stats);
}
SPASM_API void spasm_amd_dcsr_free(spasm_amd_dcsr *D) { handle_free(D); }
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_mul(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_mul", nullptr, [&] { DeviceGuard g(A); return dcsr_mul(A, B, "product"); });
}
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_lincomb(i64 a, const spasm_amd_dcsr *A, i64 b, const spasm_amd_dcsr *B)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_lincomb", nullptr, [&] { DeviceGuard g(A); return dcsr_lincomb(a, A, b, B, "combination"); });
}
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_submatrix(const spasm_amd_dcsr *A, int r0, int r1, int c0, int c1)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_submatrix", nullptr, [&] { DeviceGuard g(A); return dcsr_submatrix(A, r0, r1, c0, c1, "submatrix"); });
}
SPASM_API int spasm_amd_dcsr_equal(const spasm_amd_dcsr *A, const spasm_amd_dcsr *B)
{
    return abi_call("spasm_amd_dcsr_equal", -1, [&] { DeviceGuard g(A); return dcsr_equal(A, B, "comparison"); });
}
// transpose, permutation, concatenation of resident matrices (reshape.hpp)
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_transpose(const spasm_amd_dcsr *A)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_transpose", nullptr, [&] { DeviceGuard g(A); return dcsr_transpose(A, "transpose"); });
}
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_permute(const spasm_amd_dcsr *A, const int *p, const int *qinv)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_permute", nullptr, [&] { DeviceGuard g(A); return dcsr_permute(A, p, qinv, "permutation"); });
}
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_vcat(int count, const spasm_amd_dcsr *const *D)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_vcat", nullptr, [&] { DeviceGuard g((count > 0 && D) ? D[0] : nullptr); return dcsr_cat(RSH_VCAT, count, D, "vcat"); });
}
SPASM_API spasm_amd_dcsr *spasm_amd_dcsr_hcat(int count, const spasm_amd_dcsr *const *D)
{
    return abi_call<spasm_amd_dcsr *>("spasm_amd_dcsr_hcat", nullptr, [&] { DeviceGuard g((count > 0 && D) ? D[0] : nullptr); return dcsr_cat(RSH_HCAT, count, D, "hcat"); });
}
// one-shot forms on host matrices: upload, operate, download
SPASM_API struct spasm_csr *spasm_amd_csr_mul(const struct spasm_csr *A, const struct spasm_csr *B)
{
    return abi_call<struct spasm_csr *>("spasm_amd_csr_mul", nullptr, [&] { return csr_mul_once(A, B); });
}
SPASM_API struct spasm_csr *spasm_amd_csr_lincomb(i64 a, const struct spasm_csr *A, i64 b, const struct spasm_csr *B)
{
    return abi_call<struct spasm_csr *>("spasm_amd_csr_lincomb", nullptr, [&] { return csr_lincomb_once(a, A, b, B); });
}

// reference src/SpaSM.jl:663-692 (dense_back_solve, dense_forward_solve): host arrays; on an error b and x are left as they were
SPASM_API bool spasm_dense_forward_solve(const struct spasm_csr *U, spasm_ZZp *b, spasm_ZZp *x, const int *q)
{
    return trsolve_once(U, b, x, q, 0, "spasm_dense_forward_solve");
}

SPASM_API bool spasm_dense_back_solve(const struct spasm_csr *L, spasm_ZZp *b, spasm_ZZp *x, const int *p)
{
    return trsolve_once(L, b, x, p, 1, "spasm_dense_back_solve");
}

SPASM_API spasm_amd_trsolve *spasm_amd_trsolve_create(const struct spasm_csr *T, const int *piv, int kind)
{
    return abi_call<spasm_amd_trsolve *>("spasm_amd_trsolve_create", nullptr, [&] { return trsolve_create(T, piv, kind, "spasm_amd_trsolve_create"); }, ABI_NAMED_BELOW);
}

SPASM_API int spasm_amd_trsolve_apply(spasm_amd_trsolve *op, int k, spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok)
{
    return abi_call("spasm_amd_trsolve_apply", -1, [&] {
        trsolve_check(op, k, B, ldb, X, ldx, ok, "spasm_amd_trsolve_apply");
        DeviceGuard g(op);
        op->apply_host(k, B, ldb, X, ldx, ok);
        return 0;
    }, ABI_NAMED_BELOW);
}

SPASM_API int spasm_amd_trsolve_apply_dev(spasm_amd_trsolve *op, int k, spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok, void *stream)
{
    return abi_call("spasm_amd_trsolve_apply_dev", -1, [&] {
        trsolve_check(op, k, B, ldb, X, ldx, ok, "spasm_amd_trsolve_apply_dev");
        DeviceGuard g(op);
        hipStream_t s = (hipStream_t)stream;
        if (k > 0) op->apply_dev(k, B, ldb, X, ldx, ok, s);
        if (!stream) HIPCHK(hipStreamSynchronize(s));
        return 0;
    }, ABI_NAMED_BELOW);
}

SPASM_API void spasm_amd_trsolve_stats(const spasm_amd_trsolve *op, i64 *out)
{
    if (!op || !out) return;
    const i64 v[8] = {op->n, op->m, op->npart, op->nlevels, op->nwide, op->nchunk, op->launches(), op->stored};
    memcpy(out, v, sizeof v);
}

SPASM_API void spasm_amd_trsolve_free(spasm_amd_trsolve *op) { handle_free(op); }

// ---- many small matrices in one call (batch.hpp; engine extension): the caller's device is put back, none is selected ----
SPASM_API int spasm_amd_echelonize_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, struct spasm_lu **out)
{
    return abi_call("spasm_amd_echelonize_batch", -1, [&] { DeviceGuard g; batch_run(BATCH_LU, count, A, opts, out, nullptr, nullptr); return 0; });
}

SPASM_API int spasm_amd_rank_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, i64 *rank)
{
    return abi_call("spasm_amd_rank_batch", -1, [&] { DeviceGuard g; batch_run(BATCH_RANK, count, A, opts, nullptr, nullptr, rank); return 0; });
}

SPASM_API int spasm_amd_kernel_batch(int count, const struct spasm_csr *const *A, struct echelonize_opts *opts, struct spasm_csr **K)
{
    return abi_call("spasm_amd_kernel_batch", -1, [&] { DeviceGuard g; batch_run(BATCH_KERNEL, count, A, opts, nullptr, K, nullptr); return 0; });
}

SPASM_API void spasm_amd_batch_stats(i64 *out)
{
    if (out) memcpy(out, g_batch_stats, sizeof g_batch_stats);
}

// ---- a matrix split into its connected components on the device (blocks.hpp; engine extension) ----
SPASM_API spasm_amd_blocks *spasm_amd_blocks_create(const struct spasm_csr *A)
{
    return abi_call<spasm_amd_blocks *>("spasm_amd_blocks_create", nullptr, [&] { DeviceGuard g; return blocks_create(A); });
}

SPASM_API spasm_amd_blocks *spasm_amd_blocks_create_dcsr(const spasm_amd_dcsr *D)
{
    return abi_call<spasm_amd_blocks *>("spasm_amd_blocks_create_dcsr", nullptr, [&] { DeviceGuard g(D); return blocks_create_dcsr(D); });
}

// the index split: row i and column i are one vertex (n == m); an ordinary handle otherwise
SPASM_API spasm_amd_blocks *spasm_amd_blocks_create_index(const struct spasm_csr *A)
{
    return abi_call<spasm_amd_blocks *>("spasm_amd_blocks_create_index", nullptr, [&] { DeviceGuard g; return blocks_create(A, true); });
}

SPASM_API spasm_amd_blocks *spasm_amd_blocks_create_index_dcsr(const spasm_amd_dcsr *D)
{
    return abi_call<spasm_amd_blocks *>("spasm_amd_blocks_create_index_dcsr", nullptr, [&] { DeviceGuard g(D); return blocks_create_dcsr(D, true); });
}

SPASM_API int spasm_amd_blocks_is_index(const spasm_amd_blocks *B) { return B ? B->index : -1; }

SPASM_API void spasm_amd_blocks_info(const spasm_amd_blocks *B, i64 *out)
{
    if (!B || !out) return;
    const i64 v[11] = {B->nb, B->n, B->m, B->nnz, B->big[0], B->big[1], B->big[2], B->empty, B->us[0], B->us[1], B->us[2]};
    memcpy(out, v, sizeof v);
}

SPASM_API int spasm_amd_blocks_shapes(const spasm_amd_blocks *B, int *rows, int *cols, i64 *nnz)
{
    return abi_call("spasm_amd_blocks_shapes", -1, [&] {
        DeviceGuard g;
        blocks_need(B);
        for (int b = 0; b < B->nb; b++) {
            if (rows) rows[b] = (int)(B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b]);
            if (cols) cols[b] = (int)(B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b]);
            if (nnz) nnz[b] = B->h_nnz[(size_t)b];
        }
        return 0;
    });
}

SPASM_API int spasm_amd_blocks_maps(const spasm_amd_blocks *B, int *row_block, int *row_pos, int *col_block, int *col_pos, int *block_rows, i64 *row_start,
                                    int *block_cols, i64 *col_start)
{
    return abi_call("spasm_amd_blocks_maps", -1, [&] {
        DeviceGuard g(B);
        blocks_need(B);
        hipStream_t s = nullptr;
        blocks_copy_out(row_block, B->row_block, (size_t)B->n, s); blocks_copy_out(row_pos, B->row_pos, (size_t)B->n, s);
        blocks_copy_out(col_block, B->col_block, (size_t)B->m, s); blocks_copy_out(col_pos, B->col_pos, (size_t)B->m, s);
        blocks_copy_out(block_rows, B->block_rows, (size_t)B->n, s); blocks_copy_out(block_cols, B->block_cols, (size_t)B->m, s);
        HIPCHK(hipStreamSynchronize(s));
        if (row_start) memcpy(row_start, B->h_row_start.data(), sizeof(i64) * ((size_t)B->nb + 1));
        if (col_start) memcpy(col_start, B->h_col_start.data(), sizeof(i64) * ((size_t)B->nb + 1));
        return 0;
    });
}

SPASM_API struct spasm_csr *spasm_amd_blocks_fetch(const spasm_amd_blocks *B, int b)
{
    return abi_call<struct spasm_csr *>("spasm_amd_blocks_fetch", nullptr, [&] { DeviceGuard g(B); blocks_need(B); return blocks_fetch(B, b); });
}

SPASM_API int spasm_amd_blocks_rank(spasm_amd_blocks *B, struct echelonize_opts *opts, i64 *rank)
{
    return abi_call("spasm_amd_blocks_rank", -1, [&] { DeviceGuard g(B); blocks_need(B); blocks_run(BATCH_RANK, B, opts, nullptr, nullptr, rank); return 0; });
}

SPASM_API int spasm_amd_blocks_echelonize(spasm_amd_blocks *B, struct echelonize_opts *opts, struct spasm_lu **out)
{
    return abi_call("spasm_amd_blocks_echelonize", -1, [&] { DeviceGuard g(B); blocks_need(B); blocks_run(BATCH_LU, B, opts, out, nullptr, nullptr); return 0; });
}

SPASM_API int spasm_amd_blocks_kernel(spasm_amd_blocks *B, struct echelonize_opts *opts, struct spasm_csr **K)
{
    return abi_call("spasm_amd_blocks_kernel", -1, [&] { DeviceGuard g(B); blocks_need(B); blocks_run(BATCH_KERNEL, B, opts, nullptr, K, nullptr); return 0; });
}

SPASM_API void spasm_amd_blocks_free(spasm_amd_blocks *B) { handle_free(B); }

// ---- X * A = B for many small matrices, and block by block (solve_batch.hpp; engine extension) ----
SPASM_API int spasm_amd_solve_batch(int count, const struct spasm_csr *const *A, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok)
{
    return abi_call("spasm_amd_solve_batch", -1, [&] { DeviceGuard g; solve_batch_run(count, A, B, X, ok); return 0; });
}

SPASM_API int spasm_amd_blocks_solve(spasm_amd_blocks *B, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok)
{
    return abi_call("spasm_amd_blocks_solve", -1, [&] { DeviceGuard g; solve_blocks_run(B, Rhs, X, ok); return 0; });
}

SPASM_API void spasm_amd_solve_stats(i64 *out)
{
    if (out) memcpy(out, g_solve_stats, sizeof g_solve_stats);
}

// ---- X * A = B with A factored once (solver.hpp; engine extension): the functions called select the solver's device ----
SPASM_API spasm_amd_solver *spasm_amd_solver_create(int count, const struct spasm_csr *const *A)
{
    return abi_call<spasm_amd_solver *>("spasm_amd_solver_create", nullptr, [&] { DeviceGuard g; return solver_create(count, A); });
}

SPASM_API spasm_amd_solver *spasm_amd_solver_create_blocks(const spasm_amd_blocks *Bk)
{
    return abi_call<spasm_amd_solver *>("spasm_amd_solver_create_blocks", nullptr, [&] { DeviceGuard g; return solver_create_blocks(Bk); });
}

SPASM_API int spasm_amd_solver_apply(spasm_amd_solver *S, const struct spasm_csr *const *B, struct spasm_csr **X, unsigned char *const *ok)
{
    return abi_call("spasm_amd_solver_apply", -1, [&] { DeviceGuard g; solver_apply_run(S, B, X, ok); return 0; });
}

SPASM_API int spasm_amd_solver_apply_blocks(spasm_amd_solver *S, const struct spasm_csr *Rhs, struct spasm_csr **X, unsigned char *ok)
{
    return abi_call("spasm_amd_solver_apply_blocks", -1, [&] { DeviceGuard g; solver_apply_blocks_run(S, Rhs, X, ok); return 0; });
}

SPASM_API int spasm_amd_solver_apply_dense(spasm_amd_solver *S, int K, const spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok)
{
    return abi_call("spasm_amd_solver_apply_dense", -1, [&] { DeviceGuard g; solver_apply_dense_host(S, K, B, ldb, X, ldx, ok); return 0; });
}

SPASM_API int spasm_amd_solver_apply_dense_dev(spasm_amd_solver *S, int K, const spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok, void *stream)
{
    return abi_call("spasm_amd_solver_apply_dense_dev", -1, [&] { DeviceGuard g; solver_apply_dense_dev(S, K, B, ldb, X, ldx, ok, (hipStream_t)stream); return 0; });
}

SPASM_API void spasm_amd_solver_dense_info(const spasm_amd_solver *S, i64 *out)
{
    if (!S || !out) return;
    i64 N = 0, M = 0, general = 0;
    solver_dense_dims(S, N, M);
    for (const SolverSys &Y : S->sys) general += Y.kind == SOLVER_GENERAL ? 1 : 0;
    const i64 v[8] = {N, M, S->blocks ? 1 : (i64)S->sys.size(), general, S->dense.K, S->dense.K ? S->dense.njobs : 0, S->dense.K ? S->dense.launches : 0, S->dense_built};
    memcpy(out, v, sizeof v);
}

SPASM_API void spasm_amd_solver_info(const spasm_amd_solver *S, i64 *out)
{
    if (S && out) memcpy(out, S->info, sizeof S->info);
}

SPASM_API int spasm_amd_solver_ranks(const spasm_amd_solver *S, i64 *rank)
{
    return abi_call("spasm_amd_solver_ranks", -1, [&] {
        DeviceGuard g;
        if (!S) throw EngineError("NULL handle");
        if (!S->sys.empty() && !rank) throw EngineError("NULL array");
        for (size_t i = 0; i < S->sys.size(); i++) rank[i] = S->sys[i].r;
        return 0;
    });
}

SPASM_API int spasm_amd_solver_basis(const spasm_amd_solver *S, int i, int *rows)
{
    return abi_call("spasm_amd_solver_basis", -1, [&] {
        DeviceGuard g;
        if (!S) throw EngineError("NULL handle");
        if (i < 0 || (size_t)i >= S->sys.size()) throw EngineError("system index out of range");
        const std::vector<int> &b = S->sys[(size_t)i].basis;
        if (!b.empty() && !rows) throw EngineError("NULL array");
        if (!b.empty()) memcpy(rows, b.data(), b.size() * sizeof(int));
        return (int)b.size();
    });
}

SPASM_API void spasm_amd_solver_stats(i64 *out)
{
    if (out) memcpy(out, g_solver_stats, sizeof g_solver_stats);
}

SPASM_API void spasm_amd_solver_free(spasm_amd_solver *S) { handle_free(S); }

SPASM_API int spasm_amd_last_rounds(struct spasm_amd_round_stats *out, int max_rounds)
{
    const int n = (int)g_last_rounds.size();
    for (int i = 0; i < n && i < max_rounds; i++) out[i] = g_last_rounds[(size_t)i];
    return n;
}

SPASM_API void spasm_amd_dense_stats(i64 *out)
{
    if (out) memcpy(out, g_dense_stats, sizeof g_dense_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Determinants mod p (det.hpp): of many small matrices in one call, of a split matrix block by block, of a whole matrix.  A
// matrix whose image fits LDS (n * n <= BATCH_LIMIT) is one workgroup of k_batch_det, staged, classed and launched by the batch's
// driver; the others go through do_echelonize with L one at a time, where
//   det = sgn(k -> p[k]) * sgn(k -> column with qinv == k) * prod_k L[p[k]][k]:
// A = L * U; the rows p[0 .. n) of L form a lower triangle whose diagonal holds the unscaled pivots (what
// spasm_factorization_verify checks under (d)), and U, with a 1 on column pivcol[k] of row k and no cycle among its other entries,
// has that one transversal.  Both parities are counted on the host, cycle by cycle.
// ------------------------------------------------------------------------------------------------
#include "det.hpp"

namespace {

// count, LDS items, general-path items, items zero by structure, launches, device us, host-parity us, spare
thread_local i64 g_det_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

const ElimKernels<BatchArgs> kBatchDet = {{k_batch_det<64>, k_batch_det<128>, k_batch_det<256>, k_batch_det<512>}};

// 0 for an even permutation of 0 .. n - 1, 1 for an odd one: n - cycles mod 2
int det_perm_parity(const std::vector<i64> &perm)
{
    const size_t n = perm.size();
    std::vector<char> seen(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (perm[i] < 0 || (size_t)perm[i] >= n || seen[(size_t)perm[i]]) throw EngineError("internal error: a map of the determinant is no permutation");
        seen[(size_t)perm[i]] = 1;
    }
    size_t cycles = 0;
    for (size_t i = 0; i < n; i++) {
        if (seen[i] == 2) continue;
        cycles++;
        for (size_t k = i; seen[k] != 2; k = (size_t)perm[k]) seen[k] = 2;
    }
    return (int)((n - cycles) & 1);
}

// The LDS path from the descriptors on: batch_one_word over k_batch_det.  item[f] describes the f-th matrix of the concatenated
// CSR on the device; out[f] = its determinant.  g_det_stats[4], [5] are added to.
void det_fast(const std::vector<BatchItem> &item, const i64d *dP, const int *dJ, const int *dX, std::vector<int> &out)
{
    const int nf = (int)item.size();
    out.assign((size_t)nf, 0);
    if (nf == 0) return;
    std::vector<BatchDesc> desc((size_t)nf);
    std::vector<unsigned char> cls((size_t)nf);
    for (int f = 0; f < nf; f++) cls[(size_t)f] = (unsigned char)batch_describe(item[(size_t)f], desc[(size_t)f]);
    const BatchTimed t = batch_one_word(kBatchDet, desc, cls, dP, dJ, dX, out.data());
    g_det_stats[4] += t.launches;
    g_det_stats[5] += (i64)(t.ms * 1000.0);
}

// one square matrix through the general path
int det_general(const struct spasm_csr *M)
{
    const int n = M->n;
    const ZpField F = zp_field_make(M->field->p);
    std::unique_ptr<struct spasm_lu, void (*)(struct spasm_lu *)> N(solve_slow_factor(M), spasm_lu_free);
    if (N->r < n) return 0;
    const struct spasm_csr *Lf = N->L;
    if (N->r != n || !Lf || !N->p || !N->qinv || Lf->n != n || Lf->m != n) throw EngineError("internal error: the factorization of a determinant has no square L");
    const double t0 = spasm_wtime();
    int prod = 1;
    std::vector<i64> rows((size_t)n), cols((size_t)n, -1);
    for (int k = 0; k < n; k++) {
        const int i = N->p[k];
        if (i < 0 || i >= n) throw EngineError("internal error: a map of the determinant is no permutation");
        rows[(size_t)k] = i;
        int diag = 0;
        for (i64 q = Lf->p[i]; q < Lf->p[i + 1]; q++)
            if (Lf->j[q] == k) diag = zp_add(F, diag, zp_reduce(F, (int64_t)Lf->x[q]));
        if (diag == 0) throw EngineError("internal error: L without a pivot on its diagonal");
        prod = zp_mul(F, prod, diag);
    }
    for (int j = 0; j < n; j++) {
        const int k = N->qinv[j];
        if (k < 0 || k >= n || cols[(size_t)k] != -1) throw EngineError("internal error: a map of the determinant is no permutation");
        cols[(size_t)k] = j;
    }
    const int odd = det_perm_parity(rows) ^ det_perm_parity(cols);
    g_det_stats[6] += (i64)((spasm_wtime() - t0) * 1e6);
    return odd ? zp_neg(F, prod) : prod;
}

void det_stats_reset() { memset(g_det_stats, 0, sizeof g_det_stats); }

// det[i] of every A[i].  Nothing is written before all is done.
void det_run(int count, const struct spasm_csr *const *A, spasm_ZZp *det)
{
    det_stats_reset();
    if (count < 0) throw EngineError("count < 0");
    if (count == 0) return;
    if (!A || !det) throw EngineError("NULL array");
    for (int i = 0; i < count; i++) {
        batch_check_at(i, A[i]);
        require_square(i, A[i]->n, A[i]->m);
    }
    require_device();
    std::vector<int> fast, slow;
    for (int i = 0; i < count; i++) {
        if ((i64)A[i]->n * A[i]->n <= BATCH_LIMIT) fast.push_back(i);
        else slow.push_back(i);
    }
    i64 *st = g_det_stats;
    st[0] = count;
    st[1] = (i64)fast.size();
    st[2] = (i64)slow.size();
    std::vector<int> res((size_t)count, 0);
    if (!fast.empty()) {
        BatchStaged in;
        const std::vector<BatchItem> item = batch_stage_items(A, fast, in);
        std::vector<int> d;
        det_fast(item, in.P, in.J, in.X, d);
        for (size_t f = 0; f < fast.size(); f++) res[(size_t)fast[f]] = d[f];
    }
    for (int i : slow) res[(size_t)i] = det_general(A[i]);
    for (int i = 0; i < count; i++) det[i] = res[(size_t)i];
}

// The determinant of the matrix behind the handle: the product of its blocks' determinants times the parities of the row and the
// column permutation that bring it to block-diagonal form (row i to row_start[row_block[i]] + row_pos[i], columns alike).  A block
// that is not square, or a row or column without entry (a block of its own, 1 x 0 or 0 x 1), makes it 0 and nothing is eliminated.
void blocks_det(spasm_amd_blocks *B, spasm_ZZp *det)
{
    det_stats_reset();
    blocks_need(B);
    if (!det) throw EngineError("NULL array");
    require_square(-1, B->n, B->m);
    i64 *st = g_det_stats;
    const int count = B->nb;
    const ZpField F = zp_field_make(B->prime);
    st[0] = count;
    std::vector<int> fast, slow;
    std::vector<BatchItem> item;
    for (int b = 0; b < count; b++) {
        const i64 rn = B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b], cn = B->h_col_start[(size_t)b + 1] - B->h_col_start[(size_t)b];
        if (rn != cn || B->h_nnz[(size_t)b] == 0) st[3]++;
        else if (rn * rn <= BATCH_LIMIT) {
            fast.push_back(b);
            item.push_back(blocks_item(B, b));
        } else slow.push_back(b);
    }
    if (st[3] > 0) { *det = 0; return; }
    st[1] = (i64)fast.size();
    st[2] = (i64)slow.size();
    int prod = 1;
    std::vector<int> d;
    det_fast(item, B->P.p, B->J.p, B->X.p, d);
    for (int v : d) prod = zp_mul(F, prod, v);
    for (int b : slow) {
        if (prod == 0) break;
        std::unique_ptr<struct spasm_csr, void (*)(struct spasm_csr *)> M(blocks_fetch(B, b), spasm_csr_free);
        prod = zp_mul(F, prod, det_general(M.get()));
    }
    if (prod != 0 && B->n > 0) {
        // the four maps come to the host for the two parities: 16 bytes per row of A
        const double t0 = spasm_wtime();
        hipStream_t s = nullptr;
        const size_t n = (size_t)B->n;
        std::vector<int> blk(n), pos(n);
        std::vector<i64> perm(n);
        int odd = 0;
        for (int side = 0; side < 2; side++) {
            blocks_copy_out(blk.data(), side ? B->col_block : B->row_block, n, s);
            blocks_copy_out(pos.data(), side ? B->col_pos : B->row_pos, n, s);
            HIPCHK(hipStreamSynchronize(s));
            const std::vector<i64> &start = side ? B->h_col_start : B->h_row_start;
            for (size_t i = 0; i < n; i++) {
                if (blk[i] < 0 || blk[i] >= count) throw EngineError("internal error: a map of the determinant is no permutation");
                perm[i] = start[(size_t)blk[i]] + pos[i];
            }
            odd ^= det_perm_parity(perm);
        }
        if (odd) prod = zp_neg(F, prod);
        st[6] += (i64)((spasm_wtime() - t0) * 1e6);
    }
    *det = prod;
}

// split, then blocks_det on a handle that lives for the call (the split is not part of the stats; the handle's info has it)
template <class Make> void det_split(Make &&make, spasm_ZZp *det)
{
    std::unique_ptr<spasm_amd_blocks> B(make());
    blocks_det(B.get(), det);
}

} // namespace

extern "C" {

// ---- determinants mod p (det.hpp; engine extension): the caller's device is put back, none is selected ----
SPASM_API int spasm_amd_det_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *det)
{
    return abi_call("spasm_amd_det_batch", -1, [&] { DeviceGuard g; det_run(count, A, det); return 0; });
}

SPASM_API int spasm_amd_det(const struct spasm_csr *A, spasm_ZZp *det)
{
    return abi_call("spasm_amd_det", -1, [&] {
        DeviceGuard g;
        det_stats_reset();
        if (const char *bad = batch_check(A)) throw EngineError(bad);
        if (!det) throw EngineError("NULL array");
        require_square(-1, A->n, A->m);
        det_split([&] { return blocks_create(A); }, det);
        return 0;
    });
}

SPASM_API int spasm_amd_blocks_det(spasm_amd_blocks *B, spasm_ZZp *det)
{
    return abi_call("spasm_amd_blocks_det", -1, [&] { DeviceGuard g(B); blocks_det(B, det); return 0; });
}

SPASM_API int spasm_amd_dcsr_det(const spasm_amd_dcsr *D, spasm_ZZp *det)
{
    return abi_call("spasm_amd_dcsr_det", -1, [&] {
        DeviceGuard g(D);
        det_stats_reset();
        if (!D) throw EngineError("NULL matrix");
        if (!det) throw EngineError("NULL array");
        require_square(-1, D->n, D->m);
        det_split([&] { return blocks_create_dcsr(D); }, det);
        return 0;
    });
}

SPASM_API void spasm_amd_det_stats(i64 *out)
{
    if (out) memcpy(out, g_det_stats, sizeof g_det_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Characteristic polynomials mod p (charpoly.hpp): chi_A(x) = det(x * I - A) of many small matrices in one call, of one matrix, of
// a resident matrix.  A matrix whose image fits LDS (n * n <= BATCH_LIMIT) is one workgroup of k_batch_charpoly, staged, classed
// and launched by the batch's driver; a larger one (n <= CHARPOLY_NMAX) is one workgroup of k_charpoly_global on an image of its
// own in device memory, all of them in one launch.  The n + 1 coefficients of every matrix come back in one download.
// ------------------------------------------------------------------------------------------------
#include "charpoly.hpp"

namespace {

// matrices, of them LDS path, of them global path, launches, device us of the LDS path, of the global path, 0, 0
thread_local i64 g_charpoly_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

const ElimKernels<CharpolyArgs> kBatchCharpoly = {{k_batch_charpoly<64>, k_batch_charpoly<128>, k_batch_charpoly<256>, k_batch_charpoly<512>}};

void charpoly_stats_reset() { memset(g_charpoly_stats, 0, sizeof g_charpoly_stats); }

void charpoly_check_size(int i, int n)
{
    if (n <= CHARPOLY_NMAX) return;
    char msg[160];
    if (i >= 0) snprintf(msg, sizeof msg, "matrix %d: characteristic polynomial limited to n <= %d (n = %d)", i, CHARPOLY_NMAX, n);
    else snprintf(msg, sizeof msg, "characteristic polynomial limited to n <= %d (n = %d)", CHARPOLY_NMAX, n);
    throw EngineError(msg);
}

// What the launches of one call hold until the stream has passed them: descriptors, item lists, the images of the global path, the
// events around the two paths.  order[q] = which item descriptor q describes (the LDS items first, then the global ones).
struct CharpolyJob {
    std::vector<int> order, items;
    std::vector<BatchDesc> desc;
    DevBuf<BatchDesc> d_desc;
    DevBuf<int> d_items, d_img;
    SpgEvents ev;
    int nl = 0, ng = 0, launches = 0;
    // after the stream was synchronized: st[0 .. 5] as spasm_amd_charpoly_stats documents them
    void stats(i64 *st)
    {
        st[0] = nl + ng;
        st[1] = nl;
        st[2] = ng;
        st[3] = launches;
        if (nl > 0) st[4] = (i64)(ev.ms(0, 1) * 1000.0);
        if (ng > 0) st[5] = (i64)(ev.ms(2, 3) * 1000.0);
    }
};

// item[f] describes the f-th matrix (m = n) of a concatenated CSR on the device, its entries as columns dJ and values dX or packed
// as dE.  Its n + 1 coefficients go to d_coef[rec[f] ..] (rec == NULL: back to back in the order of `order`; `words` = their sum).
// Launches only: the caller synchronizes the stream.
void charpoly_launch(CharpolyJob &job, const std::vector<BatchItem> &item, const i64 *rec, const i64d *dP, const int *dJ, const int *dX, const int2 *dE, int *d_coef,
                     hipStream_t s)
{
    const int nf = (int)item.size();
    for (int c = 0; c < BATCH_NCLASS; c++) {
        int bw, rmax;
        batch_layout(c, bw, rmax);
        if (rmax > 2 * bw) throw EngineError("internal error: the work words of a characteristic polynomial do not fit a class");
    }
    std::vector<int> &order = job.order;
    for (int f = 0; f < nf; f++)
        if ((i64)item[(size_t)f].n * item[(size_t)f].n <= BATCH_LIMIT) order.push_back(f);
    const int nl = (int)order.size();
    for (int f = 0; f < nf; f++)
        if ((i64)item[(size_t)f].n * item[(size_t)f].n > BATCH_LIMIT) order.push_back(f);
    job.nl = nl;
    job.ng = nf - nl;
    std::vector<BatchDesc> &desc = job.desc;
    desc.resize((size_t)nf);
    std::vector<unsigned char> cls((size_t)nf, 0);
    std::vector<int> &items = job.items;
    items.resize((size_t)nf);
    i64 words = 0, image = 0;
    for (int q = 0; q < nf; q++) {
        const BatchItem &M = item[(size_t)order[(size_t)q]];
        BatchDesc &d = desc[(size_t)q];
        if (q < nl) {
            cls[(size_t)q] = (unsigned char)batch_describe(M, d);
        } else {
            memset(&d, 0, sizeof d);
            d.n = d.m = M.n;
            d.F = zp_field_make(M.prime);
            d.row0 = M.row0;
            d.ld = M.n | 1;
            d.slice = image;
            image += (i64)M.n * d.ld;
            items[(size_t)q] = q;
        }
        d.rec = rec ? rec[order[(size_t)q]] : words;
        words += (i64)M.n + 1;
    }
    job.d_desc.alloc((size_t)nf);
    job.d_items.alloc((size_t)nf);
    if (image > 0) job.d_img.alloc((size_t)image);
    HIPCHK(hipMemcpyAsync(job.d_desc.p, desc.data(), (size_t)nf * sizeof(BatchDesc), hipMemcpyHostToDevice, s));
    CharpolyArgs a;
    memset(&a, 0, sizeof a);
    a.desc = job.d_desc.p;
    a.P = dP;
    a.J = dJ;
    a.X = dX;
    a.E = dE;
    a.coef = d_coef;
    a.gimg = job.d_img.p;
    SpgEvents &ev = job.ev;
    if (nl > 0) {
        job.launches += batch_launch_jobs(kBatchCharpoly, cls, 0, nl, items, job.d_items.p, a, ev.e[0], s);
        HIPCHK(hipEventRecord(ev.e[1], s));
    }
    if (nf > nl) {
        HIPCHK(hipMemcpyAsync(job.d_items.p + nl, items.data() + nl, (size_t)(nf - nl) * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev.e[2], s));
        a.items = job.d_items.p + nl;
        hipLaunchKernelGGL(k_charpoly_global, dim3(nf - nl), dim3(512), 0, s, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[3], s));
        job.launches++;
    }
}

// out[f] = the n + 1 coefficients of the f-th matrix of charpoly_launch.  The counters are set here.
void charpoly_device(const std::vector<BatchItem> &item, const i64d *dP, const int *dJ, const int *dX, const int2 *dE, std::vector<std::vector<int>> &out)
{
    const int nf = (int)item.size();
    out.assign((size_t)nf, std::vector<int>());
    i64 *st = g_charpoly_stats;
    st[0] = nf;
    if (nf == 0) return;
    hipStream_t s = nullptr;
    i64 words = 0;
    for (const BatchItem &M : item) words += (i64)M.n + 1;
    DevBuf<int> d_coef;
    d_coef.alloc((size_t)words);
    CharpolyJob job;
    charpoly_launch(job, item, nullptr, dP, dJ, dX, dE, d_coef.p, s);
    std::vector<int> coef((size_t)words);
    HIPCHK(hipMemcpyAsync(coef.data(), d_coef.p, (size_t)words * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    job.stats(st);
    for (int q = 0; q < nf; q++) {
        const BatchDesc &d = job.desc[(size_t)q];
        out[(size_t)job.order[(size_t)q]].assign(coef.begin() + d.rec, coef.begin() + d.rec + d.n + 1);
    }
}

// coef[i][0 .. n_i] of every A[i].  Nothing is written before all is done.
void charpoly_run(int count, const struct spasm_csr *const *A, spasm_ZZp *const *coef)
{
    charpoly_stats_reset();
    if (count < 0) throw EngineError("count < 0");
    if (count == 0) return;
    if (!A || !coef) throw EngineError("NULL array");
    for (int i = 0; i < count; i++) {
        batch_check_at(i, A[i]);
        require_square(i, A[i]->n, A[i]->m);
        if (!coef[i]) {
            char msg[160];
            snprintf(msg, sizeof msg, "matrix %d: NULL array", i);
            throw EngineError(msg);
        }
        charpoly_check_size(i, A[i]->n);
    }
    require_device();
    std::vector<int> all;
    for (int i = 0; i < count; i++) all.push_back(i);
    BatchStaged in;
    const std::vector<BatchItem> item = batch_stage_items(A, all, in);
    std::vector<std::vector<int>> res;
    charpoly_device(item, in.P, in.J, in.X, nullptr, res);
    for (int i = 0; i < count; i++) memcpy(coef[i], res[(size_t)i].data(), res[(size_t)i].size() * sizeof(int));
}

} // namespace

extern "C" {

// ---- characteristic polynomials mod p (charpoly.hpp; engine extension): the caller's device is put back, none is selected ----
SPASM_API int spasm_amd_charpoly_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *const *coef)
{
    return abi_call("spasm_amd_charpoly_batch", -1, [&] { DeviceGuard g; charpoly_run(count, A, coef); return 0; });
}

SPASM_API int spasm_amd_charpoly(const struct spasm_csr *A, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_charpoly", -1, [&] {
        DeviceGuard g;
        charpoly_stats_reset();
        if (const char *bad = batch_check(A)) throw EngineError(bad);
        if (!coef) throw EngineError("NULL array");
        require_square(-1, A->n, A->m);
        charpoly_check_size(-1, A->n);
        charpoly_run(1, &A, &coef);
        return 0;
    });
}

SPASM_API int spasm_amd_dcsr_charpoly(const spasm_amd_dcsr *D, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_dcsr_charpoly", -1, [&] {
        DeviceGuard g(D);
        charpoly_stats_reset();
        if (!D) throw EngineError("NULL matrix");
        if (!coef) throw EngineError("NULL array");
        require_square(-1, D->n, D->m);
        charpoly_check_size(-1, D->n);
        std::vector<BatchItem> item(1, BatchItem{D->n, D->m, 0, D->F.p});
        std::vector<std::vector<int>> res;
        charpoly_device(item, D->p.p, nullptr, nullptr, D->ent.p, res);
        memcpy(coef, res[0].data(), res[0].size() * sizeof(int));
        return 0;
    });
}

SPASM_API void spasm_amd_charpoly_stats(i64 *out)
{
    if (out) memcpy(out, g_charpoly_stats, sizeof g_charpoly_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Characteristic polynomials by components (blocks.hpp: the index split; polyprod.hpp: the product tree).  The blocks of an index
// handle go to the kernels of charpoly.hpp straight from the handle's concatenated CSR; the kernels write the factors into one
// concatenated array (the polynomial of block b at row_start[b] + b), which the product tree reduces on the device.
// ------------------------------------------------------------------------------------------------
#include "polyprod.hpp"

namespace {

// blocks, of them LDS path, of them global path, launches of the charpoly kernels, their device us, product levels, product device us, 0
thread_local i64 g_charpoly_split_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

void charpoly_split_stats_reset() { memset(g_charpoly_split_stats, 0, sizeof g_charpoly_split_stats); }

// The descriptors of all levels of a product tree, from the lengths alone, and its launches.
struct PolyProduct {
    struct Level { size_t pair0, t0, w0; int tcnt, wcnt, tb, wb; };
    std::vector<Level> level;
    std::vector<PpPair> pair;          // level after level
    std::vector<int> tsum, tpair, wsum, wpair;
    DevBuf<PpPair> d_pair;
    DevBuf<int> d_tsum, d_tpair, d_wsum, d_wpair;
    i64 total = 0, out_words = 0;

    // len[k] >= 1 words at the exclusive scan of len; the sum is below 2^31 (the callers have checked both)
    void plan(const std::vector<int> &len)
    {
        std::vector<int> off(len.size()), cur(len);
        for (size_t k = 0; k < len.size(); k++) { off[k] = (int)total; total += len[k]; }
        out_words = total - (i64)len.size() + 1;
        while (cur.size() > 1) {
            Level L;
            L.pair0 = pair.size();
            L.t0 = tsum.size();
            L.w0 = wsum.size();
            L.tcnt = L.wcnt = 0;
            const size_t c = cur.size(), np = (c + 1) / 2;
            std::vector<int> noff(np), nlen(np);
            i64 tw = 0, ww = 0;
            std::vector<int> ts, tp, ws, wp;
            for (size_t k = 0; k < np; k++) {
                const int a = cur[2 * k], b = 2 * k + 1 < c ? cur[2 * k + 1] : 0;
                const int outlen = b ? a + b - 1 : a;
                pair.push_back(PpPair{off[2 * k], a, b ? off[2 * k + 1] : 0, b});
                if (b && std::min(a, b) >= PP_WAVE) { ws.push_back((int)ww); wp.push_back((int)k); ww += outlen; }
                else { ts.push_back((int)tw); tp.push_back((int)k); tw += outlen; }
                noff[k] = off[2 * k];
                nlen[k] = outlen;
            }
            ts.push_back((int)tw);
            ws.push_back((int)ww);
            L.tcnt = (int)tp.size();
            L.wcnt = (int)wp.size();
            L.tb = cdiv(tw, 256);
            L.wb = cdiv(ww, 4 * PP_WPW);
            tsum.insert(tsum.end(), ts.begin(), ts.end());
            wsum.insert(wsum.end(), ws.begin(), ws.end());
            // the pair lists are padded to the length of the sums, so that one base serves both arrays of a shape
            tp.push_back(0);
            wp.push_back(0);
            tpair.insert(tpair.end(), tp.begin(), tp.end());
            wpair.insert(wpair.end(), wp.begin(), wp.end());
            level.push_back(L);
            off.swap(noff);
            cur.swap(nlen);
        }
    }

    void upload(hipStream_t s)
    {
        if (level.empty()) return;
        d_pair.alloc(pair.size());
        d_tsum.alloc(tsum.size());
        d_tpair.alloc(tpair.size());
        d_wsum.alloc(wsum.size());
        d_wpair.alloc(wpair.size());
        HIPCHK(hipMemcpyAsync(d_pair.p, pair.data(), pair.size() * sizeof(PpPair), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_tsum.p, tsum.data(), tsum.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_tpair.p, tpair.data(), tpair.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_wsum.p, wsum.data(), wsum.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_wpair.p, wpair.data(), wpair.size() * sizeof(int), hipMemcpyHostToDevice, s));
    }

    // x0 holds the factors (balanced residues), x1 is the other buffer of `total` words; returns the one that holds the product
    int *run(const ZpField &F, int *x0, int *x1, hipStream_t s)
    {
        int *src = x0, *dst = x1;
        for (const Level &L : level) {
            PpArgs g;
            memset(&g, 0, sizeof g);
            g.F = F;
            g.pair = d_pair.p + L.pair0;
            g.tsum = d_tsum.p + L.t0;
            g.tpair = d_tpair.p + L.t0;
            g.wsum = d_wsum.p + L.w0;
            g.wpair = d_wpair.p + L.w0;
            g.tcnt = L.tcnt;
            g.wcnt = L.wcnt;
            g.tb = L.tb;
            g.src = src;
            g.dst = dst;
            hipLaunchKernelGGL(k_pp_level, dim3(L.tb + L.wb), dim3(256), 0, s, g);
            HIPCHK(hipGetLastError());
            std::swap(src, dst);
        }
        return src;
    }
};

// out[0 .. sum(len) - count] = the product of the count polynomials f[k] (len[k] words, any int32).  Nothing is written before all
// is done.
void poly_product(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out)
{
    if (count < 0) throw EngineError("count < 0");
    if (!out) throw EngineError("NULL array");
    if (count > 0 && (!len || !f)) throw EngineError("NULL array");
    if (prime <= 2 || prime > 0xfffffffbLL) throw EngineError("prime out of range (2 < p <= 0xfffffffb)");
    i64 total = 0;
    for (int k = 0; k < count; k++) {
        char msg[96];
        if (len[k] < 1) {
            snprintf(msg, sizeof msg, "polynomial %d: a length below 1 (%d)", k, len[k]);
            throw EngineError(msg);
        }
        if (!f[k]) {
            snprintf(msg, sizeof msg, "polynomial %d: NULL array", k);
            throw EngineError(msg);
        }
        total += len[k];
        if (total >= ((i64)1 << 31)) {
            snprintf(msg, sizeof msg, "polynomial %d: the total length must be below 2^31", k);
            throw EngineError(msg);
        }
    }
    if (count == 0) { out[0] = 1; return; }
    require_device();
    hipStream_t s = nullptr;
    const ZpField F = zp_field_make(prime);
    PolyProduct pp;
    pp.plan(std::vector<int>(len, len + count));
    std::vector<int> host((size_t)total);
    {
        size_t at = 0;
        for (int k = 0; k < count; k++) { memcpy(host.data() + at, f[k], (size_t)len[k] * sizeof(int)); at += (size_t)len[k]; }
    }
    DevBuf<int> x0, x1;
    x0.alloc((size_t)total);
    if (count > 1) x1.alloc((size_t)total);
    HIPCHK(hipMemcpyAsync(x0.p, host.data(), (size_t)total * sizeof(int), hipMemcpyHostToDevice, s));
    pp.upload(s);
    hipLaunchKernelGGL(k_pp_reduce, dim3(cdiv(total, 256)), dim3(256), 0, s, F, (int)total, x0.p);
    HIPCHK(hipGetLastError());
    const int *res = pp.run(F, x0.p, x1.p, s);
    std::vector<int> got((size_t)pp.out_words);
    HIPCHK(hipMemcpyAsync(got.data(), res, (size_t)pp.out_words * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out, got.data(), (size_t)pp.out_words * sizeof(int));
}

// The characteristic polynomial of the matrix behind an index handle: coef[0 .. n] = the product of the blocks' polynomials, or
// (factors) coef[row_start[b] + b ..] = the polynomial of block b.  Both refusals come from the handle's metadata.
void blocks_charpoly(spasm_amd_blocks *B, spasm_ZZp *coef, bool factors)
{
    charpoly_split_stats_reset();
    blocks_need(B);
    if (!coef) throw EngineError("NULL array");
    if (!B->index) throw EngineError("the handle is not an index split (spasm_amd_blocks_create_index)");
    const int nb = B->nb;
    for (int b = 0; b < nb; b++) {
        const i64 rn = B->h_row_start[(size_t)b + 1] - B->h_row_start[(size_t)b];
        if (rn > CHARPOLY_NMAX) {
            char msg[160];
            snprintf(msg, sizeof msg, "block %d: characteristic polynomial limited to n <= %d (n = %lld)", b, CHARPOLY_NMAX, (long long)rn);
            throw EngineError(msg);
        }
    }
    i64 *st = g_charpoly_split_stats;
    st[0] = nb;
    if (B->n == 0) {
        if (!factors) coef[0] = 1;
        return;
    }
    hipStream_t s = nullptr;
    const i64 total = (i64)B->n + nb;   // below 2^31: n + m is
    std::vector<BatchItem> item((size_t)nb);
    std::vector<i64> rec((size_t)nb);
    std::vector<int> len((size_t)nb);
    for (int b = 0; b < nb; b++) {
        item[(size_t)b] = blocks_item(B, b);   // (square: the row and the column starts of an index split are the same)
        rec[(size_t)b] = item[(size_t)b].row0;
        len[(size_t)b] = item[(size_t)b].n + 1;
    }
    PolyProduct pp;
    DevBuf<int> x0, x1;
    x0.alloc((size_t)total);
    if (!factors) {
        pp.plan(len);
        if (nb > 1) x1.alloc((size_t)total);
        pp.upload(s);
    }
    CharpolyJob job;
    charpoly_launch(job, item, rec.data(), B->P.p, B->J.p, B->X.p, nullptr, x0.p, s);
    SpgEvents ev;
    const int *res = x0.p;
    if (!factors) {
        HIPCHK(hipEventRecord(ev.e[0], s));
        res = pp.run(zp_field_make(B->prime), x0.p, x1.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
    }
    const size_t words = factors ? (size_t)total : (size_t)B->n + 1;
    std::vector<int> got(words);
    HIPCHK(hipMemcpyAsync(got.data(), res, words * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    job.stats(cs);
    st[1] = cs[1];
    st[2] = cs[2];
    st[3] = cs[3];
    st[4] = cs[4] + cs[5];
    if (!factors) {
        st[5] = (i64)pp.level.size();
        st[6] = (i64)(ev.ms(0, 1) * 1000.0);
    }
    memcpy(coef, got.data(), words * sizeof(int));
}

// index split, then blocks_charpoly on a handle that lives for the call
template <class Make> void charpoly_split(Make &&make, spasm_ZZp *coef)
{
    std::unique_ptr<spasm_amd_blocks> B(make());
    blocks_charpoly(B.get(), coef, false);
}

} // namespace

extern "C" {

// ---- product of polynomials mod p (polyprod.hpp) and characteristic polynomials by components (engine extension) ----
SPASM_API int spasm_amd_poly_product(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out)
{
    return abi_call("spasm_amd_poly_product", -1, [&] { DeviceGuard g; poly_product(count, len, f, prime, out); return 0; });
}

SPASM_API int spasm_amd_blocks_charpoly(spasm_amd_blocks *B, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_blocks_charpoly", -1, [&] { DeviceGuard g(B); blocks_charpoly(B, coef, false); return 0; });
}

SPASM_API int spasm_amd_blocks_charpoly_factors(spasm_amd_blocks *B, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_blocks_charpoly_factors", -1, [&] { DeviceGuard g(B); blocks_charpoly(B, coef, true); return 0; });
}

SPASM_API int spasm_amd_charpoly_split(const struct spasm_csr *A, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_charpoly_split", -1, [&] {
        DeviceGuard g;
        charpoly_split_stats_reset();
        blocks_check_host(A);
        if (!coef) throw EngineError("NULL array");
        require_square(-1, A->n, A->m);
        charpoly_split([&] { return blocks_create(A, true); }, coef);
        return 0;
    });
}

SPASM_API int spasm_amd_dcsr_charpoly_split(const spasm_amd_dcsr *D, spasm_ZZp *coef)
{
    return abi_call("spasm_amd_dcsr_charpoly_split", -1, [&] {
        DeviceGuard g(D);
        charpoly_split_stats_reset();
        if (!D) throw EngineError("NULL matrix");
        if (!coef) throw EngineError("NULL array");
        require_square(-1, D->n, D->m);
        charpoly_split([&] { return blocks_create_dcsr(D, true); }, coef);
        return 0;
    });
}

SPASM_API void spasm_amd_charpoly_split_stats(i64 *out)
{
    if (out) memcpy(out, g_charpoly_split_stats, sizeof g_charpoly_split_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Minimal polynomials of sparse matrices by Wiedemann's method (krylov.hpp): the projected Krylov sequence of the resident exact
// product, Berlekamp-Massey on the device, and the lcm over the K projections on the host.
// ------------------------------------------------------------------------------------------------
#include "krylov.hpp"
#include "precond.hpp"
#include "block_krylov.hpp"
#include "block_bm.hpp"

namespace {

// n, K, steps, launches, BM class (1 LDS, 2 device memory), degree, sequence device us, BM device us
thread_local i64 g_minpoly_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

void minpoly_stats_reset() { memset(g_minpoly_stats, 0, sizeof g_minpoly_stats); }

// the grid of a step kernel: KRY_BS lanes a workgroup, at most cap workgroups (its teams stride)
dim3 step_grid(i64 lanes, int cap) { return dim3((unsigned)std::max(1, std::min(cdiv(lanes, KRY_BS), cap))); }

int step_grid_cap()
{
    int dev = 0, cu = 256;
    HIPCHK(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
    return cu * KRY_WG_PER_CU;
}

// Y <- A X with the epilogue epi on every entry of Y (spmv_step.hpp); Y is not read.  Returns the launches.
template <bool SMALL, int KW, class Epi>
int spmv_step_launch(const SpmvView &V, const ZpField &F, int kc, const int *X, i64d ldx, int *Y, i64d ldy, const Epi &epi, int cap, hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp;
    const int launches = V.for_classes<KW>(
        [&](auto team, auto partial, int nitems, const int *items, const int *segbeg, int *part) {
            constexpr int TEAM = decltype(team)::value;
            hipLaunchKernelGGL((k_spmv_step<SMALL, KW, TEAM, decltype(partial)::value, Epi>), step_grid((i64)nitems * TEAM, cap), dim3(KRY_BS), 0, s, nitems,
                               items, segbeg, V.start, V.len, V.ent, F, hp, mhp, kc, X, ldx, Y, ldy, part, epi);
        },
        [&](int nlong, const int *rows, const int *off, const int *part) {
            hipLaunchKernelGGL((k_spmv_step_combine<KW, Epi>), step_grid((i64)nlong * KW, cap), dim3(KRY_BS), 0, s, nlong, rows, off, part, kc, F, hp, mhp,
                               Y, ldy, epi);
        });
    HIPCHK(hipGetLastError());
    return launches;
}

// The operator B of a projected sequence.  No diagonal: B = A, fwd the view of a square matrix.  dl alone: B = D A, dl the n words
// of D.  tr: B = E A^T D2 A, fwd and tr the two views of the n x m matrix, dl = D2 (n words), dr = E (m words).
// block: the sequence is the b x b projection U^T B^i X of block_krylov.hpp (b = K in {2, 4, 8, 16}; b * b words a term) and not
// its diagonal.  block with tr: B = E A^T D2 A as above, dr == NULL for E = I.
struct SeqOperator {
    const SpmvView *fwd = nullptr, *tr = nullptr;
    const int *dl = nullptr, *dr = nullptr;
    bool block = false;
    int dim() const { return tr ? fwd->cols : fwd->rows; }
};

// One step is one launch set (KrylovEpi, or DiagEpi with dl) whose iterates ping-pong in W.w0 / W.w1, or with tr two sets: W.w0
// holds the n x KW intermediate and W.w1 the m x KW iterate.  A block step with tr is fwd with DiagEpi{d2, no projection}, then
// tr with BlockEpi<B>{dr or NULL, U, ldu, acc}: the existing epilogues on the other view.
template <bool SMALL, int KW>
int sequence_launch(const SeqOperator &op, const ZpField &F, int kc, i64 len, const int *U, i64 ldu, const int *X0, i64 ldx0, KrylovWork &W, int *S, int cap,
                    hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp, dim = op.dim();
    constexpr bool BLOCKW = KW >= 2 && KW <= 16; // the widths a block sequence has
    const i64 aw = op.block ? (i64)KW * KW : KW; // sums a term
    int launches = 0;
    HIPCHK(hipMemsetAsync(W.acc.p, 0, (size_t)len * aw * sizeof(long long), s));
    if (dim > 0) {
        if (op.block) {
            if constexpr (BLOCKW)
                hipLaunchKernelGGL((k_block_dot<KW>), step_grid((i64)dim * KW, cap), dim3(KRY_BS), 0, s, dim, F, hp, mhp, U, (i64d)ldu, X0, (i64d)ldx0, W.acc.p);
        } else {
            hipLaunchKernelGGL((k_krylov_dot<KW>), step_grid((i64)dim * KW, cap), dim3(KRY_BS), 0, s, dim, kc, F, hp, mhp, U, (i64d)ldu, X0, (i64d)ldx0,
                               W.acc.p);
        }
        launches++;
    }
    const int *X = X0;
    i64d ldx = (i64d)ldx0;
    int *Y = W.w0.p;
    for (i64 i = 1; i < len && dim > 0; i++) {
        long long *acc = W.acc.p + i * aw;
        if (op.block && op.tr) {
            launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, W.w0.p, (i64d)KW, DiagEpi{op.dl, nullptr, 0, nullptr}, cap, s);
            if constexpr (BLOCKW)
                launches += spmv_step_launch<SMALL, KW>(*op.tr, F, kc, W.w0.p, (i64d)KW, W.w1.p, (i64d)KW, BlockEpi<KW>{op.dr, U, (i64d)ldu, acc}, cap, s);
            X = W.w1.p;
        } else if (op.block) {
            if constexpr (BLOCKW) launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, Y, (i64d)KW, BlockEpi<KW>{op.dl, U, (i64d)ldu, acc}, cap, s);
            X = Y;
            Y = Y == W.w0.p ? W.w1.p : W.w0.p;
        } else if (op.tr) {
            launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, W.w0.p, (i64d)KW, DiagEpi{op.dl, nullptr, 0, nullptr}, cap, s);
            launches += spmv_step_launch<SMALL, KW>(*op.tr, F, kc, W.w0.p, (i64d)KW, W.w1.p, (i64d)KW, DiagEpi{op.dr, U, (i64d)ldu, acc}, cap, s);
            X = W.w1.p;
        } else {
            if (op.dl) launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, Y, (i64d)KW, DiagEpi{op.dl, U, (i64d)ldu, acc}, cap, s);
            else launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, Y, (i64d)KW, KrylovEpi{U, (i64d)ldu, acc}, cap, s);
            X = Y;
            Y = Y == W.w0.p ? W.w1.p : W.w0.p;
        }
        ldx = KW;
    }
    const i64 total = op.block ? len * aw : len * kc;
    hipLaunchKernelGGL(k_krylov_finish, dim3(cdiv(total, 256)), dim3(256), 0, s, (i64d)total, op.block ? (int)aw : kc, (int)aw, F, W.acc.p, S);
    HIPCHK(hipGetLastError());
    return launches + 1;
}

// S[i * K + c] = sum_r U[r, c] * (B^i X)[r, c], 0 <= i < len, on device arrays, enqueued on s; no host synchronization.
// 1 <= K <= 64, len >= 1.  With op.block: S[(i * K + r) * K + c] = sum_k U[k, r] * (B^i X)[k, c].  Returns the launches.
int sequence_run(const SeqOperator &op, const ZpField &F, int K, i64 len, const int *U, i64 ldu, const int *X, i64 ldx, KrylovWork &W, int *S, hipStream_t s)
{
    const int kw = spmv_kw(K), cap = step_grid_cap();
    if (len > 1) {
        W.w0.ensure((size_t)op.fwd->rows * kw);
        if (op.tr || len > 2) W.w1.ensure((size_t)op.dim() * kw);
    }
    W.acc.ensure((size_t)len * kw * (op.block ? kw : 1));
    return dispatch_kw(kw, [&](auto KW) {
        return F.small ? sequence_launch<true, KW()>(op, F, K, len, U, ldu, X, ldx, W, S, cap, s)
                       : sequence_launch<false, KW()>(op, F, K, len, U, ldu, X, ldx, W, S, cap, s);
    });
}

void krylov_check(const spasm_amd_spmv *op, int trans, int K, i64 len, const void *U, i64 ldu, const void *V, i64 ldv, const void *S)
{
    if (!op) throw EngineError("NULL operator");
    require_square(-1, op->A.n, op->A.m);
    if (K < 1 || K > 64) throw EngineError("K out of range (1 <= K <= 64)");
    if (len < 0 || len * 64 >= ((i64)1 << 31) || ldu < K || ldv < K || (trans != 0 && trans != 1))
        throw EngineError("bad arguments (trans 0/1, 0 <= len < 2^25, ldu >= K, ldv >= K)");
    if (len > 0 && (!S || (op->A.n > 0 && (!U || !V)))) throw EngineError("NULL array");
}

// the class of a Berlekamp-Massey launch: 1 LDS, 2 device memory
int bm_class(int len, int where)
{
    if (where < 0 || where > 2) throw EngineError("where must be 0 (by size), 1 (LDS) or 2 (device memory)");
    const bool fits = 2 * ((i64)len + 1) <= BM_LDS_WORDS;
    if (where == 1 && !fits) {
        char msg[128];
        snprintf(msg, sizeof msg, "the LDS class does not fit (len = %d, at most %d)", len, BM_LDS_WORDS / 2 - 1);
        throw EngineError(msg);
    }
    return where == 2 || !fits ? 2 : 1;
}

void check_prime(i64 prime)
{
    if (prime <= 2 || prime > 0xfffffffbLL) throw EngineError("prime out of range (2 < p <= 0xfffffffb)");
}

void bm_check_len(const ZpField &F, i64 len)
{
    if (len < 0 || len >= ((i64)1 << 30)) throw EngineError("len out of range (0 <= len < 2^30)");
    if (len > (i64)zp_lazy_terms(F) * BM_BS) throw EngineError("len beyond the lazy accumulator of the discrepancy for this prime");
}

// count sequences on the device (sequence c is column c of S, leading dimension lds) -> d_coef (count x ldc), d_deg; enqueued on s
void bm_device(const ZpField &F, int count, int len, const int *dS, i64 lds, int cls, int *d_coef, i64 ldc, int *d_deg, DevBuf<int> &gwork, hipStream_t s)
{
    BmArgs a;
    a.F = F;
    a.len = len;
    a.S = dS;
    a.lds = (i64d)lds;
    a.coef = d_coef;
    a.ldc = (i64d)ldc;
    a.deg = d_deg;
    a.gwork = nullptr;
    if (cls == 1) {
        static bool attr_done[kMaxDev] = {false};
        bool &done = attr_done[current_device()];
        if (!done) {
            HIPCHK(hipFuncSetAttribute((const void *)k_berlekamp_massey<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, BM_LDS_WORDS * 4));
            HIPCHK(hipFuncSetAttribute((const void *)k_berlekamp_massey<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, BM_LDS_WORDS * 4));
            done = true;
        }
        const size_t lds_bytes = 2 * ((size_t)len + 1) * sizeof(int);
        if (F.small) hipLaunchKernelGGL((k_berlekamp_massey<true, true>), dim3(count), dim3(BM_BS), lds_bytes, s, a);
        else hipLaunchKernelGGL((k_berlekamp_massey<false, true>), dim3(count), dim3(BM_BS), lds_bytes, s, a);
    } else {
        gwork.ensure((size_t)count * 2 * ((size_t)len + 1));
        a.gwork = gwork.p;
        if (F.small) hipLaunchKernelGGL((k_berlekamp_massey<true, false>), dim3(count), dim3(BM_BS), 0, s, a);
        else hipLaunchKernelGGL((k_berlekamp_massey<false, false>), dim3(count), dim3(BM_BS), 0, s, a);
    }
    HIPCHK(hipGetLastError());
}

void berlekamp_massey(int count, int len, const spasm_ZZp *S, i64 lds, i64 prime, int where, spasm_ZZp *coef, i64 ldc, int *deg)
{
    minpoly_stats_reset();
    if (count < 0) throw EngineError("count < 0");
    check_prime(prime);
    const ZpField F = zp_field_make(prime);
    bm_check_len(F, len);
    if (lds < count) throw EngineError("lds < count");
    if (ldc < (i64)len + 1) throw EngineError("ldc < len + 1");
    if ((i64)count * ldc >= ((i64)1 << 40)) throw EngineError("count * ldc too large");
    const int cls = bm_class(len, where);
    if (count == 0) return;
    if (!coef || !deg || (len > 0 && !S)) throw EngineError("NULL array");
    require_device();
    hipStream_t s = nullptr;
    DevBuf<int> dS, d_coef, d_deg, gwork;
    dS.alloc((size_t)len * (size_t)count);
    d_coef.alloc((size_t)count * (size_t)ldc);
    d_deg.alloc((size_t)count);
    if (len > 0)
        HIPCHK(hipMemcpy2DAsync(dS.p, (size_t)count * sizeof(int), S, (size_t)lds * sizeof(int), (size_t)count * sizeof(int), (size_t)len, hipMemcpyHostToDevice, s));
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    bm_device(F, count, len, dS.p, count, cls, d_coef.p, ldc, d_deg.p, gwork, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> hc((size_t)count * (size_t)ldc), hd((size_t)count);
    HIPCHK(hipMemcpyAsync(hc.data(), d_coef.p, hc.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hd.data(), d_deg.p, hd.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 *st = g_minpoly_stats;
    st[1] = count;
    st[3] = 1;
    st[4] = cls;
    st[7] = (i64)(ev.ms(0, 1) * 1000.0);
    memcpy(coef, hc.data(), hc.size() * sizeof(int));
    memcpy(deg, hd.data(), hd.size() * sizeof(int));
}

// ---- Berlekamp-Massey over matrix sequences (block_bm.hpp)
int block_width(int b)
{
    if (b != 2 && b != 4 && b != 8 && b != 16) throw EngineError("b must be 2, 4, 8 or 16");
    return b;
}

// Nothing in k_bbm_disc counts lazy terms, and no len can overrun them: a lane takes at most BBM_CHUNK * 16 of them whatever len
// is, below the 65043 the i32 accumulator of the largest p < 2^16 holds (zp_lazy_terms; more for smaller primes).  So the i32 lazy
// limit refuses no len here, unlike bm_check_len; len is bounded by the words of g alone.
static_assert(BBM_CHUNK * 16 <= 65043, "a lane of k_bbm_disc stays inside the i32 lazy accumulator");
void block_bm_check_len(i64 len)
{
    if (len < 1 || len >= ((i64)1 << 24)) throw EngineError("len out of range (1 <= len < 2^24)");
}

// the device state of one matrix Berlekamp-Massey run, kept from one try to the next
struct BlockBmWork {
    DevBuf<int> g0, g1, small;
    DevBuf<long long> dacc;
    BbmState st;
    void ensure(int b, int len)
    {
        const size_t r = 2 * (size_t)b, words = ((size_t)len + 2) * r * b;
        g0.ensure(words);
        g1.ensure(words);
        dacc.ensure(r * b);
        small.ensure(r * b + r * r + 2 * r + 1 + b);
        st.g[0] = g0.p;
        st.g[1] = g1.p;
        st.dacc = dacc.p;
        st.hk = small.p;
        st.T = st.hk + r * b;
        st.deg = st.T + r * r;
        st.piv = st.deg + r;
        st.maxdeg = st.piv + r;
        st.sel = st.maxdeg + 1;
    }
};

template <bool SMALL, int B>
int block_bm_launch(const ZpField &F, int len, const int *dS, BlockBmWork &W, int *d_coef, int *d_rowdeg, int *d_dmax, hipStream_t s)
{
    constexpr int R = 2 * B;
    const size_t words = ((size_t)len + 2) * R * B;
    HIPCHK(hipMemsetAsync(W.st.g[0], 0, words * sizeof(int), s));
    HIPCHK(hipMemsetAsync(W.st.g[1], 0, words * sizeof(int), s));
    hipLaunchKernelGGL((k_bbm_init<B>), dim3(1), dim3(BBM_BS), 0, s, W.st);
    int cur = 0;
    for (int k = 0; k < len; k++) {
        hipLaunchKernelGGL((k_bbm_disc<SMALL, B>), dim3(cdiv((i64)k + 1, BBM_CHUNK)), dim3(BBM_DISC_BS), 0, s, k, F, dS, W.st.g[cur], W.st.maxdeg, W.st.dacc);
        hipLaunchKernelGGL((k_bbm_elim<B>), dim3(1), dim3(BBM_BS), 0, s, F, W.st);
        hipLaunchKernelGGL((k_bbm_update<SMALL, B>), dim3(cdiv(((i64)k + 2) * R * B, BBM_BS)), dim3(BBM_BS), 0, s, k, F, W.st.g[cur], W.st.g[cur ^ 1], W.st.T,
                           W.st.piv, W.st.maxdeg);
        cur ^= 1;
    }
    hipLaunchKernelGGL((k_bbm_select<B>), dim3(1), dim3(BBM_BS), 0, s, F, W.st, W.st.g[cur], d_rowdeg, d_dmax);
    const i64 total = ((i64)len + 1) * B * B;
    hipLaunchKernelGGL((k_bbm_write<B>), dim3(cdiv(total, BBM_BS)), dim3(BBM_BS), 0, s, (i64d)total, W.st.g[cur], W.st.sel, d_rowdeg, d_coef);
    HIPCHK(hipGetLastError());
    return 3 * len + 3;
}

// The left generator of the len terms dS (b * b words a term) -> d_coef ((len + 1) * b * b words, F_t at t * b * b), d_rowdeg (b),
// d_dmax (1), all on the device; enqueued on s, no host synchronization.  Returns the launches.
int block_bm_device(const ZpField &F, int b, int len, const int *dS, BlockBmWork &W, int *d_coef, int *d_rowdeg, int *d_dmax, hipStream_t s)
{
    W.ensure(b, len);
    auto go = [&](auto B) {
        return F.small ? block_bm_launch<true, B()>(F, len, dS, W, d_coef, d_rowdeg, d_dmax, s)
                       : block_bm_launch<false, B()>(F, len, dS, W, d_coef, d_rowdeg, d_dmax, s);
    };
    switch (b) {
    case 2: return go(std::integral_constant<int, 2>());
    case 4: return go(std::integral_constant<int, 4>());
    case 8: return go(std::integral_constant<int, 8>());
    default: return go(std::integral_constant<int, 16>());
    }
}

// b, len, steps of the sequence, launches, sum of the row degrees, tries used, device us of the sequence, device us of
// Berlekamp-Massey, n, largest row degree
thread_local i64 g_block_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void block_stats_reset() { memset(g_block_stats, 0, sizeof g_block_stats); }

void block_berlekamp_massey(int b, int len, const spasm_ZZp *S, i64 prime, spasm_ZZp *coef, int *rowdeg, int *dmax)
{
    block_stats_reset();
    block_width(b);
    check_prime(prime);
    if ((prime & 1) == 0) throw EngineError("prime must be odd");
    const ZpField F = zp_field_make(prime);
    block_bm_check_len(len);
    if (!S || !coef || !rowdeg || !dmax) throw EngineError("NULL array");
    require_device();
    hipStream_t s = nullptr;
    const size_t bb = (size_t)b * b;
    DevBuf<int> dS, d_coef, d_small;
    BlockBmWork W;
    dS.alloc((size_t)len * bb);
    d_coef.alloc(((size_t)len + 1) * bb);
    d_small.alloc((size_t)b + 1);
    HIPCHK(hipMemcpyAsync(dS.p, S, (size_t)len * bb * sizeof(int), hipMemcpyHostToDevice, s));
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    const int launches = block_bm_device(F, b, len, dS.p, W, d_coef.p, d_small.p, d_small.p + b, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> hc(((size_t)len + 1) * bb), hs((size_t)b + 1);
    HIPCHK(hipMemcpyAsync(hc.data(), d_coef.p, hc.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hs.data(), d_small.p, hs.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(coef, hc.data(), hc.size() * sizeof(int));
    memcpy(rowdeg, hs.data(), (size_t)b * sizeof(int));
    *dmax = hs[(size_t)b];
    i64 *st = g_block_stats;
    st[0] = b;
    st[1] = len;
    st[3] = launches;
    for (int r = 0; r < b; r++) st[4] += rowdeg[r];
    st[7] = (i64)(ev.ms(0, 1) * 1000.0);
    st[9] = *dmax;
}

// ---- polynomials over GF(p) on the host, as residues in [0, p), low degree first, no zero leading word (the zero polynomial is empty)
typedef std::vector<uint64_t> HPoly;

// any int32 -> its residue in [0, p); a residue in [0, p) -> the balanced one
inline uint64_t hresidue(int x, uint64_t p)
{
    const int64_t r = (int64_t)x % (int64_t)p;
    return (uint64_t)(r < 0 ? r + (int64_t)p : r);
}

inline int hbalanced(uint64_t w, uint64_t p) { return (int)(w > p / 2 ? (int64_t)w - (int64_t)p : (int64_t)w); }

HPoly hpoly_load(const int *f, int len, uint64_t p)
{
    HPoly a((size_t)len);
    for (int k = 0; k < len; k++) a[(size_t)k] = hresidue(f[k], p);
    while (!a.empty() && a.back() == 0) a.pop_back();
    return a;
}

// the multiplicity of x in f (not zero: its leading word ends the loop)
size_t hpoly_valuation(const HPoly &f)
{
    size_t e = 0;
    while (f[e] == 0) e++;
    return e;
}

uint64_t hinv(uint64_t a, uint64_t p)
{
    int64_t r0 = (int64_t)a, r1 = (int64_t)p, s0 = 1, s1 = 0;
    while (r1 != 0) {
        const int64_t q = r0 / r1;
        int64_t t = r0 - q * r1; r0 = r1; r1 = t;
        t = s0 - q * s1; s0 = s1; s1 = t;
    }
    int64_t r = s0 % (int64_t)p;
    return (uint64_t)(r < 0 ? r + (int64_t)p : r);
}

// a <- a mod b (b not zero); quo (may be NULL) <- the quotient.  Products of two residues fit a u64 (p < 2^32).
void hpoly_divrem(HPoly &a, const HPoly &b, uint64_t p, HPoly *quo)
{
    const size_t db = b.size() - 1;
    if (quo) quo->assign(a.size() > db ? a.size() - db : 0, 0);
    const uint64_t ib = hinv(b.back(), p);
    while (a.size() > db) {
        const size_t sh = a.size() - 1 - db;
        const uint64_t q = a.back() * ib % p;
        if (quo) (*quo)[sh] = q;
        const uint64_t nq = p - q; // q != 0: a has no zero leading word
        for (size_t k = 0; k <= db; k++) a[sh + k] = (a[sh + k] + nq * b[k]) % p;
        while (!a.empty() && a.back() == 0) a.pop_back();
    }
}

void hpoly_monic(HPoly &a, uint64_t p)
{
    if (a.empty() || a.back() == 1) return;
    const uint64_t i = hinv(a.back(), p);
    for (uint64_t &w : a) w = w * i % p;
}

// the monic lcm of two non-zero polynomials: a * (b / gcd(a, b))
HPoly hpoly_lcm(HPoly a, HPoly b, uint64_t p)
{
    hpoly_monic(a, p);
    hpoly_monic(b, p);
    if (a == b) return a;
    HPoly g = a, h = b;
    while (!h.empty()) {
        hpoly_divrem(g, h, p, nullptr);
        g.swap(h);
    }
    HPoly q, r = b;
    hpoly_divrem(r, g, p, &q);
    HPoly out(a.size() + q.size() - 1, 0);
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] == 0) continue;
        for (size_t j = 0; j < q.size(); j++) out[i + j] = (out[i + j] + a[i] * q[j]) % p;
    }
    hpoly_monic(out, p);
    return out;
}

void hpoly_store(const HPoly &a, uint64_t p, int *out)
{
    for (size_t k = 0; k < a.size(); k++) out[k] = hbalanced(a[k], p);
}

void poly_lcm(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out, int *outlen)
{
    if (count < 0) throw EngineError("count < 0");
    if (!out || !outlen) throw EngineError("NULL array");
    if (count > 0 && (!len || !f)) throw EngineError("NULL array");
    check_prime(prime);
    const uint64_t p = (uint64_t)prime;
    std::vector<HPoly> poly;
    i64 total = 0;
    for (int k = 0; k < count; k++) {
        char msg[96];
        if (len[k] < 1) {
            snprintf(msg, sizeof msg, "polynomial %d: a length below 1 (%d)", k, len[k]);
            throw EngineError(msg);
        }
        if (!f[k]) {
            snprintf(msg, sizeof msg, "polynomial %d: NULL array", k);
            throw EngineError(msg);
        }
        total += len[k];
        if (total >= ((i64)1 << 31)) {
            snprintf(msg, sizeof msg, "polynomial %d: the total length must be below 2^31", k);
            throw EngineError(msg);
        }
        poly.push_back(hpoly_load(f[k], len[k], p));
        if (poly.back().empty()) {
            snprintf(msg, sizeof msg, "polynomial %d: the zero polynomial has no lcm", k);
            throw EngineError(msg);
        }
    }
    HPoly r(1, 1);
    for (const HPoly &g : poly) r = hpoly_lcm(r, g, p);
    hpoly_store(r, p, out);
    *outlen = (int)r.size();
}

// The vectors of spasm_amd_minpoly when the caller gives none: word (t, r, c) -- t = 0 for U, 1 for V -- is the splitmix64 output
// of the state seed + 0x9E3779B97F4A7C15 * (2 * (r * K + c) + t + 1), reduced mod p to the balanced residue.
uint64_t minpoly_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

void minpoly_vectors(int n, int K, uint64_t seed, i64 prime, int *U, int *V)
{
    const uint64_t p = (uint64_t)prime;
    for (int t = 0; t < 2; t++) {
        int *dst = t ? V : U;
        if (!dst) continue;
        for (i64 e = 0; e < (i64)n * K; e++) {
            dst[e] = hbalanced(minpoly_mix(seed + 0x9E3779B97F4A7C15ULL * (2 * (uint64_t)e + (uint64_t)t + 1)) % p, p);
        }
    }
}

int minpoly_K(int K)
{
    if (K < 0 || K > 64) throw EngineError("K out of range (0 <= K <= 64, 0 means 8)");
    return K == 0 ? 8 : K;
}

// the degree bound of a caller: maxdeg where it lies in 1 .. n, else n
int degree_bound(int maxdeg, int n) { return (maxdeg <= 0 || maxdeg > n) ? n : maxdeg; }

// 2 * md terms determine a recurrence of degree <= md; two more terms show a degree above md as L > md (see the header)
int sequence_terms(int md, int n) { return md < n ? 2 * md + 2 : 2 * n; }

// The stage every Wiedemann driver shares: the projected sequence of len terms, Berlekamp-Massey on its K columns, and the K
// polynomials on the host.  The buffers are kept from one try to the next.
struct SeqRecurrences {
    DevBuf<int> dS, d_coef, d_deg, gwork;
    KrylovWork W;
    SpgEvents ev;
    std::vector<int> deg, coef; // the K degrees; K rows of ldh words
    size_t ldh = 0;
    struct Run {
        int launches, bm_class; // the launches include Berlekamp-Massey's one
        i64 sequence_us, bm_us;
    };

    // U and X are packed n x K device arrays.  Synchronizes s.  The polynomials come back in one copy of K rows by
    // (largest degree + 1) words.
    Run run(const SeqOperator &op, const ZpField &F, int K, int len, const int *U, const int *X, hipStream_t s)
    {
        const i64 ldc = (i64)len + 1;
        const int cls = bm_class(len, 0);
        dS.ensure((size_t)len * K);
        d_coef.ensure((size_t)K * (size_t)ldc);
        d_deg.ensure((size_t)K);
        HIPCHK(hipEventRecord(ev.e[0], s));
        const int launches = sequence_run(op, F, K, len, U, K, X, K, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        bm_device(F, K, len, dS.p, K, cls, d_coef.p, ldc, d_deg.p, gwork, s);
        HIPCHK(hipEventRecord(ev.e[2], s));
        deg.resize((size_t)K);
        HIPCHK(hipMemcpyAsync(deg.data(), d_deg.p, deg.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ldh = (size_t)*std::max_element(deg.begin(), deg.end()) + 1;
        coef.resize((size_t)K * ldh);
        HIPCHK(hipMemcpy2D(coef.data(), ldh * sizeof(int), d_coef.p, (size_t)ldc * sizeof(int), ldh * sizeof(int), (size_t)K, hipMemcpyDeviceToHost));
        return {launches + 1, cls, (i64)(ev.ms(0, 1) * 1000.0), (i64)(ev.ms(1, 2) * 1000.0)};
    }

    // the polynomial of projection c: monic, of degree deg[c]
    HPoly poly(int c, uint64_t p) const { return hpoly_load(coef.data() + (size_t)c * ldh, deg[(size_t)c] + 1, p); }
};

// The lcm of the minimal polynomials of the K projected sequences of the square matrix behind view V.
void minpoly_run(const SpmvView &V, const ZpField &F, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *X, spasm_ZZp *coef, int *deg)
{
    const int n = V.rows, md = degree_bound(maxdeg, n);
    const uint64_t p = (uint64_t)F.p;
    if (n >= (1 << 24)) throw EngineError("minimal polynomial limited to n < 2^24");
    const int len = sequence_terms(md, n);
    bm_check_len(F, len);
    hipStream_t s = nullptr;
    std::vector<int> hu, hv;
    if (!U) {
        hu.resize((size_t)n * K);
        hv.resize((size_t)n * K);
        minpoly_vectors(n, K, seed, F.p, hu.data(), hv.data());
        U = hu.data();
        X = hv.data();
    }
    DevBuf<int> dU, dV;
    const size_t nk = (size_t)n * K;
    dU.alloc(nk);
    dV.alloc(nk);
    HIPCHK(hipMemcpyAsync(dU.p, U, nk * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dV.p, X, nk * sizeof(int), hipMemcpyHostToDevice, s));
    SeqRecurrences R;
    const SeqRecurrences::Run run = R.run({&V}, F, K, len, dU.p, dV.p, s);
    i64 *st = g_minpoly_stats;
    st[0] = n;
    st[1] = K;
    st[2] = len - 1;
    st[3] = run.launches;
    st[4] = run.bm_class;
    st[6] = run.sequence_us;
    st[7] = run.bm_us;
    for (int c = 0; c < K; c++)
        if (R.deg[(size_t)c] > md) {
            char msg[128];
            snprintf(msg, sizeof msg, "degree bound too small (projection %d has degree %d, maxdeg %d)", c, R.deg[(size_t)c], md);
            throw EngineError(msg);
        }
    HPoly r(1, 1);
    for (int c = 0; c < K; c++) {
        r = hpoly_lcm(r, R.poly(c, p), p);
        if ((i64)r.size() - 1 > md) throw EngineError("degree bound too small (the lcm of the projections exceeds maxdeg)");
    }
    st[5] = (i64)r.size() - 1;
    hpoly_store(r, p, coef);
    *deg = (int)r.size() - 1;
}

// the view of a resident matrix (n, m > 0): the row pointers serve as starts, the lengths are their differences
void dcsr_view(const spasm_amd_dcsr *D, SpmvView &view, hipStream_t s) { view.from_row_pointers(D->n, D->m, D->p.p, D->ent.p, s); }

// The matrix of a family entry: a host CSR, an SpMV operator or a resident matrix.  check() reads n, m and F without a device;
// views() takes the device (put back when this goes) and builds the views that are asked for.  It owns what it had to make:
// the temporary operator of a CSR, the transpose of a resident matrix, the views of a resident matrix.
struct Operand {
    std::unique_ptr<DeviceGuard> guard; // first: whatever lives on the device goes before it
    const spasm_csr *A = nullptr;
    spasm_amd_spmv *op = nullptr;
    const spasm_amd_dcsr *D = nullptr;
    const char *who = nullptr; // the entry's name, for the messages of the temporary operator
    enum { CSR, SPMV, DCSR } kind;
    std::unique_ptr<spasm_amd_spmv> tmp;
    std::unique_ptr<spasm_amd_dcsr> T;
    SpmvView vf, vt;
    int n = 0, m = 0;
    ZpField F;
    const SpmvView *fwd = nullptr, *tr = nullptr;

    Operand(const spasm_csr *A_, const char *who_) : A(A_), who(who_), kind(CSR) {}
    Operand(spasm_amd_spmv *op_) : op(op_), kind(SPMV) {}
    Operand(const spasm_amd_dcsr *D_) : D(D_), kind(DCSR) {}

    void check()
    {
        if (kind == CSR) {
            if (const char *bad = batch_check(A)) throw EngineError(bad);
            n = A->n, m = A->m, F = zp_field_make(A->field->p);
        } else if (kind == SPMV) {
            if (!op) throw EngineError("NULL operator");
            n = op->A.n, m = op->A.m, F = op->F;
        } else {
            if (!D) throw EngineError("NULL matrix");
            n = D->n, m = D->m, F = D->F;
        }
    }

    void views(bool forward, bool transposed)
    {
        if (kind == CSR) {
            guard.reset(new DeviceGuard());
            tmp.reset(spmv_create(A, who));
            op = tmp.get();
        } else if (kind == SPMV) {
            guard.reset(new DeviceGuard(op));
        } else {
            guard.reset(new DeviceGuard(D));
            // the transpose stays on the device for the length of the call
            if (transposed) T.reset(dcsr_transpose(D, "transpose"));
            if (forward) dcsr_view(D, vf, nullptr);
            if (transposed) dcsr_view(T.get(), vt, nullptr);
            fwd = &vf, tr = &vt;
            return;
        }
        if (transposed) op->build_transpose();
        fwd = &op->fwd, tr = &op->tr;
    }
};

int minpoly_entry(Operand &&o, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *X, spasm_ZZp *coef, int *deg)
{
    minpoly_stats_reset();
    o.check();
    require_square(-1, o.n, o.m);
    K = minpoly_K(K);
    if (!coef || !deg) throw EngineError("NULL array");
    if ((U == nullptr) != (X == nullptr)) throw EngineError("U and V must both be given or both be NULL");
    if (o.n == 0) { coef[0] = 1; *deg = 0; return 0; }
    o.views(true, false);
    minpoly_run(*o.fwd, o.F, K, seed, maxdeg, U, X, coef, deg);
    return 0;
}

} // namespace

extern "C" {

// ---- Krylov sequences, Berlekamp-Massey and minimal polynomials (krylov.hpp; engine extension) ----
SPASM_API int spasm_amd_krylov_sequence(spasm_amd_spmv *op, int trans, int K, int len, const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    return abi_call("spasm_amd_krylov_sequence", -1, [&] {
        minpoly_stats_reset();
        krylov_check(op, trans, K, len, U, ldu, V, ldv, S);
        if (len == 0) return 0;
        DeviceGuard g(op);
        if (trans) op->build_transpose();
        const SpmvView &view = trans ? op->tr : op->fwd;
        const size_t n = (size_t)op->A.n, kk = (size_t)K;
        hipStream_t s = nullptr;
        DevBuf<int> dU, dV, dS;
        KrylovWork W;
        dU.alloc(n * kk);
        dV.alloc(n * kk);
        dS.alloc((size_t)len * kk);
        if (n > 0) {
            HIPCHK(hipMemcpy2DAsync(dU.p, kk * sizeof(int), U, (size_t)ldu * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpy2DAsync(dV.p, kk * sizeof(int), V, (size_t)ldv * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
        }
        SpgEvents ev;
        HIPCHK(hipEventRecord(ev.e[0], s));
        const int launches = sequence_run({&view}, op->F, K, len, dU.p, K, dV.p, K, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        std::vector<int> out((size_t)len * kk);
        HIPCHK(hipMemcpyAsync(out.data(), dS.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        i64 *st = g_minpoly_stats;
        st[0] = (i64)n;
        st[1] = K;
        st[2] = len - 1;
        st[3] = launches;
        st[6] = (i64)(ev.ms(0, 1) * 1000.0);
        memcpy(S, out.data(), out.size() * sizeof(int));
        return 0;
    });
}

SPASM_API int spasm_amd_krylov_sequence_dev(spasm_amd_spmv *op, int trans, int K, int len, const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv,
                                            spasm_ZZp *S, void *stream)
{
    return abi_call("spasm_amd_krylov_sequence_dev", -1, [&] {
        minpoly_stats_reset();
        krylov_check(op, trans, K, len, U, ldu, V, ldv, S);
        if (len == 0) return 0;
        DeviceGuard g(op);
        if (trans) op->build_transpose();
        hipStream_t s = (hipStream_t)stream;
        const int launches = sequence_run({trans ? &op->tr : &op->fwd}, op->F, K, len, U, ldu, V, ldv, op->kry, S, s);
        if (!stream) HIPCHK(hipStreamSynchronize(s));
        i64 *st = g_minpoly_stats;
        st[0] = op->A.n;
        st[1] = K;
        st[2] = len - 1;
        st[3] = launches;
        return 0;
    });
}

SPASM_API int spasm_amd_berlekamp_massey(int count, int len, const spasm_ZZp *S, i64 lds, i64 prime, int where, spasm_ZZp *coef, i64 ldc, int *deg)
{
    return abi_call("spasm_amd_berlekamp_massey", -1, [&] { DeviceGuard g; berlekamp_massey(count, len, S, lds, prime, where, coef, ldc, deg); return 0; });
}

SPASM_API int spasm_amd_poly_lcm(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out, int *outlen)
{
    return abi_call("spasm_amd_poly_lcm", -1, [&] { poly_lcm(count, len, f, prime, out, outlen); return 0; });
}

SPASM_API int spasm_amd_minpoly_vectors(int n, int K, uint64_t seed, i64 prime, spasm_ZZp *U, spasm_ZZp *V)
{
    return abi_call("spasm_amd_minpoly_vectors", -1, [&] {
        if (n < 0 || K < 1 || K > 64) throw EngineError("bad arguments (n >= 0, 1 <= K <= 64)");
        check_prime(prime);
        minpoly_vectors(n, K, seed, prime, U, V);
        return 0;
    });
}

SPASM_API int spasm_amd_minpoly(const struct spasm_csr *A, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg)
{
    return abi_call("spasm_amd_minpoly", -1, [&] { return minpoly_entry(Operand(A, "spasm_amd_minpoly"), K, seed, maxdeg, U, V, coef, deg); });
}

SPASM_API int spasm_amd_spmv_minpoly(spasm_amd_spmv *op, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg)
{
    return abi_call("spasm_amd_spmv_minpoly", -1, [&] { return minpoly_entry(Operand(op), K, seed, maxdeg, U, V, coef, deg); });
}

SPASM_API int spasm_amd_dcsr_minpoly(const spasm_amd_dcsr *D, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg)
{
    return abi_call("spasm_amd_dcsr_minpoly", -1, [&] { return minpoly_entry(Operand(D), K, seed, maxdeg, U, V, coef, deg); });
}

SPASM_API void spasm_amd_minpoly_stats(i64 *out)
{
    if (out) memcpy(out, g_minpoly_stats, sizeof g_minpoly_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Polynomials of the resident exact product applied to vectors (Horner's rule, horner.hpp), and on top of them sparse solves
// without fill-in by Wiedemann's method that certify their own answers.
// ------------------------------------------------------------------------------------------------
#include "horner.hpp"

namespace {

// n, K, tries used, products with A, launches, largest degree, columns solved, columns with a kernel vector, device us of the
// sequences + Berlekamp-Massey, device us of Horner + check
thread_local i64 g_wied_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void wied_stats_reset() { memset(g_wied_stats, 0, sizeof g_wied_stats); }

// the steps of table rows T[0 .. rows) (KW words each).  X0 == NULL: the run starts from X = 0, so its first step is the plain
// scale and rows - 1 products follow; else every row is a product and the first one reads X0.  The last step writes Yout (leading
// dimension ldyo) and, when cnt is given, adds its non-zero counts to cnt[0 .. KW); the steps between ping-pong in W.
template <bool SMALL, int KW>
int horner_launch(const SpmvView &V, const ZpField &F, int kc, int rows, const int *T, const int *B, i64 ldb, const int *X0, i64 ldx0, int *Yout, i64 ldyo,
                  KrylovWork &W, long long *cnt, int cap, hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp, n = V.rows;
    int launches = 0;
    const int *X = X0;
    i64d ldx = (i64d)ldx0;
    for (int i = 0; i < rows && n > 0; i++) {
        const bool last = i == rows - 1;
        int *Y = last ? Yout : (X == W.w0.p ? W.w1.p : W.w0.p);
        const i64d ldy = last ? (i64d)ldyo : (i64d)KW;
        long long *cp = last ? cnt : nullptr;
        const int *Ti = T + (size_t)i * KW;
        if (!X) {
            hipLaunchKernelGGL((k_horner_scale<KW>), step_grid((i64)n * KW, cap), dim3(KRY_BS), 0, s, n, kc, F, hp, mhp, Ti, B, (i64d)ldb, Y, ldy, cp);
            launches++;
        } else {
            launches += spmv_step_launch<SMALL, KW>(V, F, kc, X, ldx, Y, ldy, HornerEpi{Ti, B, (i64d)ldb, cp}, cap, s);
        }
        HIPCHK(hipGetLastError());
        X = Y;
        ldx = ldy;
    }
    return launches;
}

// rows >= 1 Horner steps on device arrays, enqueued on s; no host synchronization.  T is the device table, rows x spmv_kw(K)
// canonical residues.  Returns the launches.
int horner_run(const SpmvView &V, const ZpField &F, int K, int rows, const int *T, const int *B, i64 ldb, const int *X0, i64 ldx0, int *Yout, i64 ldyo,
               KrylovWork &W, long long *cnt, hipStream_t s)
{
    const int kw = spmv_kw(K), cap = step_grid_cap();
    const size_t words = (size_t)V.rows * kw;
    if (rows > 1) {
        W.w0.ensure(words);
        if (rows > 2) W.w1.ensure(words);
    }
    return dispatch_kw(kw, [&](auto KW) {
        return F.small ? horner_launch<true, KW()>(V, F, K, rows, T, B, ldb, X0, ldx0, Yout, ldyo, W, cnt, cap, s)
                       : horner_launch<false, KW()>(V, F, K, rows, T, B, ldb, X0, ldx0, Yout, ldyo, W, cnt, cap, s);
    });
}

// the table of spasm_amd_poly_apply in W.htab: row s holds the coefficients of degree D - s, D = max(deg); zeros above a
// column's degree.  Returns D (-1: every polynomial is zero).
int poly_table(const ZpField &F, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, std::vector<int> &tab)
{
    int D = -1;
    for (int c = 0; c < K; c++) D = std::max(D, deg[c]);
    const int kw = spmv_kw(K);
    tab.assign((size_t)(D + 1) * kw, 0);
    const uint64_t p = (uint64_t)F.p;
    for (int c = 0; c < K; c++)
        for (int j = 0; j <= deg[c]; j++) tab[(size_t)(D - j) * kw + c] = hbalanced(hresidue(coef[(i64)c * ldc + j], p), p);
    return D;
}

void poly_apply_check(const spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv,
                      const spasm_ZZp *X, i64 ldx)
{
    if (!op) throw EngineError("NULL operator");
    require_square(-1, op->A.n, op->A.m);
    if (K < 1 || K > 64) throw EngineError("K out of range (1 <= K <= 64)");
    if (trans != 0 && trans != 1) throw EngineError("trans must be 0 or 1");
    if (ldv < K) throw EngineError("ldv < K");
    if (ldx < K) throw EngineError("ldx < K");
    if (!deg || !coef) throw EngineError("NULL array");
    for (int c = 0; c < K; c++) {
        char msg[112];
        if (deg[c] < -1) {
            snprintf(msg, sizeof msg, "polynomial %d: a degree below -1 (%d)", c, deg[c]);
            throw EngineError(msg);
        }
        if (deg[c] >= (1 << 24)) {
            snprintf(msg, sizeof msg, "polynomial %d: degree limited to < 2^24 (%d)", c, deg[c]);
            throw EngineError(msg);
        }
        if (ldc < (i64)deg[c] + 1) {
            snprintf(msg, sizeof msg, "polynomial %d: ldc < deg + 1 (ldc = %lld, deg = %d)", c, (long long)ldc, deg[c]);
            throw EngineError(msg);
        }
    }
    const i64 n = op->A.n;
    if (n > 0) {
        if (!V || !X) throw EngineError("NULL array");
        const uintptr_t v0 = (uintptr_t)V, v1 = v0 + (size_t)((n - 1) * ldv + K) * sizeof(int);
        const uintptr_t x0 = (uintptr_t)X, x1 = x0 + (size_t)((n - 1) * ldx + K) * sizeof(int);
        if (v0 < x1 && x0 < v1) throw EngineError("V must not overlap X");
    }
}

// X <- f_c(op(A)) V on device arrays, enqueued on s: the table goes up once, then max(deg) products.  Returns the launches.
int poly_apply_dev(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const int *dV, i64 ldv, int *dX, i64 ldx,
                   hipStream_t s, int *products)
{
    if (trans) op->build_transpose();
    const SpmvView &view = trans ? op->tr : op->fwd;
    KrylovWork &W = op->kry;
    const size_t n = (size_t)op->A.n;
    // the host copy of the previous call's table may still be on its way up
    if (W.tab_up) HIPCHK(hipEventSynchronize(W.tab_up));
    else HIPCHK(hipEventCreateWithFlags(&W.tab_up, hipEventDisableTiming));
    const int D = poly_table(op->F, K, deg, coef, ldc, W.htab);
    *products = std::max(D, 0);
    if (D < 0) {
        HIPCHK(hipMemset2DAsync(dX, (size_t)ldx * sizeof(int), 0, (size_t)K * sizeof(int), n, s));
        return 0;
    }
    W.tab.ensure(W.htab.size());
    HIPCHK(hipMemcpyAsync(W.tab.p, W.htab.data(), W.htab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(W.tab_up, s));
    return horner_run(view, op->F, K, D + 1, W.tab.p, dV, ldv, nullptr, 0, dX, ldx, W, nullptr, s);
}

void wied_check(int n, int m, int trans, int K, const void *B, i64 ldb, const void *X, i64 ldx, const int *status)
{
    require_square(-1, n, m);
    if (K < 1 || K > 64) throw EngineError("K out of range (1 <= K <= 64)");
    if (trans != 0 && trans != 1) throw EngineError("trans must be 0 or 1");
    if (ldb < K) throw EngineError("ldb < K");
    if (ldx < K) throw EngineError("ldx < K");
    if (!status || (n > 0 && (!B || !X))) throw EngineError("NULL array");
    if (n >= (1 << 24)) throw EngineError("Wiedemann solve limited to n < 2^24");
}

// the system with no unknown: the empty x solves it
void wied_empty(int K, int *status)
{
    for (int c = 0; c < K; c++) status[c] = 1;
    g_wied_stats[1] = K;
    g_wied_stats[6] = K;
}

// The solve behind the three entries: V is the view of op(A), square, n > 0; the arguments have been checked.  Nothing is written
// to X or status before every try has run.
void wied_run(const SpmvView &V, const ZpField &F, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg, const spasm_ZZp *U,
              spasm_ZZp *X, i64 ldx, int *status)
{
    const int n = V.rows, md = degree_bound(maxdeg, n), len = sequence_terms(md, n);
    const uint64_t p = (uint64_t)F.p;
    bm_check_len(F, len);
    const int ntries = U ? 1 : (tries <= 0 ? 3 : tries);
    hipStream_t s = nullptr;
    std::vector<int> outX((size_t)n * K, 0), outS((size_t)K, 0), act((size_t)K);
    for (int c = 0; c < K; c++) act[(size_t)c] = c;
    std::vector<int> hu, pu, pb, hx, tab;
    std::vector<long long> hcnt;
    std::vector<char> regular;
    DevBuf<int> dU, dB, dX, dR, dT;
    DevBuf<long long> dcnt;
    SeqRecurrences R;
    KrylovWork &W = R.W;
    SpgEvents ev;
    i64 *st = g_wied_stats;
    st[0] = n;
    st[1] = K;
    for (int t = 0; t < ntries && !act.empty(); t++) {
        const int ka = (int)act.size(), kw = spmv_kw(ka);
        const size_t nk = (size_t)n * ka;
        // the undecided columns, packed; a column keeps the u of its original index
        const int *Us = U;
        if (!U) {
            hu.resize((size_t)n * K);
            minpoly_vectors(n, K, seed + (uint64_t)t, F.p, hu.data(), nullptr);
            Us = hu.data();
        }
        pu.resize(nk);
        pb.resize(nk);
        for (int r = 0; r < n; r++)
            for (int a = 0; a < ka; a++) {
                pu[(size_t)r * ka + a] = Us[(size_t)r * K + act[(size_t)a]];
                pb[(size_t)r * ka + a] = B[(i64)r * ldb + act[(size_t)a]];
            }
        dU.ensure(nk);
        dB.ensure(nk);
        dX.ensure(nk);
        dR.ensure((size_t)n * kw);
        dcnt.ensure((size_t)2 * kw);
        HIPCHK(hipMemcpyAsync(dU.p, pu.data(), nk * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dB.p, pb.data(), nk * sizeof(int), hipMemcpyHostToDevice, s));
        const SeqRecurrences::Run run = R.run({&V}, F, ka, len, dU.p, dB.p, s);
        st[2] = t + 1;
        st[3] += len - 1;
        st[4] += run.launches;
        st[8] += run.sequence_us + run.bm_us;
        int Lmax = 0;
        for (int a = 0; a < ka; a++) {
            const int L = R.deg[(size_t)a];
            if (L > md) {
                char msg[128];
                snprintf(msg, sizeof msg, "degree bound too small (projection %d has degree %d, maxdeg %d)", act[(size_t)a], L, md);
                throw EngineError(msg);
            }
            Lmax = std::max(Lmax, L);
        }
        st[5] = std::max(st[5], (i64)Lmax);
        // the table: column a carries q = (f - f(0)) / x, scaled by -1 / f(0) when f(0) != 0, zero-padded at the top; one more row
        // for the check: -1 where x is expected to solve the system, 0 where it is expected to lie in the kernel
        const int rows = Lmax; // max deg q + 1
        tab.assign((size_t)(rows + 1) * kw, 0);
        regular.assign((size_t)ka, 0);
        for (int a = 0; a < ka; a++) {
            const HPoly f = R.poly(a, p);
            const int L = (int)f.size() - 1;
            const uint64_t f0 = f[0], scale = f0 ? (p - hinv(f0, p)) % p : 1;
            regular[(size_t)a] = f0 != 0;
            for (int j = 0; j < L; j++) tab[(size_t)(rows - 1 - j) * kw + a] = hbalanced(f[(size_t)j + 1] * scale % p, p);
            tab[(size_t)rows * kw + a] = f0 ? -1 : 0;
        }
        dT.ensure(tab.size());
        HIPCHK(hipMemcpyAsync(dT.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dcnt.p, 0, (size_t)2 * kw * sizeof(long long), s));
        HIPCHK(hipEventRecord(ev.e[0], s));
        int launches = 0;
        if (rows == 0) HIPCHK(hipMemsetAsync(dX.p, 0, nk * sizeof(int), s));
        else launches += horner_run(V, F, ka, rows, dT.p, dB.p, ka, nullptr, 0, dX.p, ka, W, dcnt.p, s);
        // the certificate: R <- op(A) X + r B, with the non-zero counts of X (above) and of R
        launches += horner_run(V, F, ka, 1, dT.p + (size_t)rows * kw, dB.p, ka, dX.p, ka, dR.p, kw, W, dcnt.p + kw, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        hcnt.resize((size_t)2 * kw);
        hx.resize(nk);
        HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt.p, hcnt.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hx.data(), dX.p, nk * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        st[3] += std::max(rows - 1, 0) + 1;
        st[4] += launches;
        st[9] += (i64)(ev.ms(0, 1) * 1000.0);
        std::vector<int> left;
        for (int a = 0; a < ka; a++) {
            const int c = act[(size_t)a];
            const bool rzero = hcnt[(size_t)kw + a] == 0, xzero = hcnt[(size_t)a] == 0;
            int verdict = 0;
            if (regular[(size_t)a] && rzero) verdict = 1;
            else if (!regular[(size_t)a] && rzero && !xzero) verdict = 2;
            if (!verdict) {
                left.push_back(c);
                continue;
            }
            outS[(size_t)c] = verdict;
            st[5 + verdict]++;
            for (int r = 0; r < n; r++) outX[(size_t)r * K + c] = hx[(size_t)r * ka + a];
        }
        act.swap(left);
    }
    for (int r = 0; r < n; r++) memcpy(X + (i64)r * ldx, outX.data() + (size_t)r * K, (size_t)K * sizeof(int));
    memcpy(status, outS.data(), (size_t)K * sizeof(int));
}

int wied_entry(Operand &&o, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg, const spasm_ZZp *U, spasm_ZZp *X, i64 ldx,
               int *status)
{
    wied_stats_reset();
    o.check();
    wied_check(o.n, o.m, trans, K, B, ldb, X, ldx, status);
    if (o.n == 0) { wied_empty(K, status); return 0; }
    o.views(!trans, trans != 0); // x A = b is A^T x = b
    wied_run(trans ? *o.tr : *o.fwd, o.F, K, B, ldb, seed, tries, maxdeg, U, X, ldx, status);
    return 0;
}

} // namespace

extern "C" {

// ---- polynomials of A applied to vectors, and Wiedemann's solve (horner.hpp; engine extension) ----
SPASM_API int spasm_amd_poly_apply(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv,
                                   spasm_ZZp *X, i64 ldx)
{
    return abi_call("spasm_amd_poly_apply", -1, [&] {
        wied_stats_reset();
        poly_apply_check(op, trans, K, deg, coef, ldc, V, ldv, X, ldx);
        const size_t n = (size_t)op->A.n, kk = (size_t)K;
        if (n == 0) return 0;
        DeviceGuard g(op);
        hipStream_t s = nullptr;
        DevBuf<int> dV, dX;
        dV.alloc(n * kk);
        dX.alloc(n * kk);
        HIPCHK(hipMemcpy2DAsync(dV.p, kk * sizeof(int), V, (size_t)ldv * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
        int products = 0;
        const int launches = poly_apply_dev(op, trans, K, deg, coef, ldc, dV.p, K, dX.p, K, s, &products);
        std::vector<int> out(n * kk);
        HIPCHK(hipMemcpyAsync(out.data(), dX.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        i64 *st = g_wied_stats;
        st[0] = (i64)n;
        st[1] = K;
        st[3] = products;
        st[4] = launches;
        for (size_t r = 0; r < n; r++) memcpy(X + (i64)r * ldx, out.data() + r * kk, kk * sizeof(int));
        return 0;
    });
}

SPASM_API int spasm_amd_poly_apply_dev(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv,
                                       spasm_ZZp *X, i64 ldx, void *stream)
{
    return abi_call("spasm_amd_poly_apply_dev", -1, [&] {
        wied_stats_reset();
        poly_apply_check(op, trans, K, deg, coef, ldc, V, ldv, X, ldx);
        if (op->A.n == 0) return 0;
        DeviceGuard g(op);
        int products = 0;
        const int launches = poly_apply_dev(op, trans, K, deg, coef, ldc, V, ldv, X, ldx, (hipStream_t)stream, &products);
        i64 *st = g_wied_stats;
        st[0] = op->A.n;
        st[1] = K;
        st[3] = products;
        st[4] = launches;
        return 0;
    });
}

SPASM_API int spasm_amd_wiedemann_solve(const struct spasm_csr *A, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                                        const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_wiedemann_solve", -1,
                    [&] { return wied_entry(Operand(A, "spasm_amd_wiedemann_solve"), trans, K, B, ldb, seed, tries, maxdeg, U, X, ldx, status); });
}

SPASM_API int spasm_amd_spmv_wiedemann_solve(spasm_amd_spmv *op, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                                             const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_spmv_wiedemann_solve", -1, [&] { return wied_entry(Operand(op), trans, K, B, ldb, seed, tries, maxdeg, U, X, ldx, status); });
}

SPASM_API int spasm_amd_dcsr_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg,
                                             const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_dcsr_wiedemann_solve", -1, [&] { return wied_entry(Operand(D), trans, K, B, ldb, seed, tries, maxdeg, U, X, ldx, status); });
}

SPASM_API void spasm_amd_wiedemann_stats(i64 *out)
{
    if (out) memcpy(out, g_wied_stats, sizeof g_wied_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Rank and determinant without fill-in by preconditioned Wiedemann (precond.hpp): the projected sequences of D A and of
// E A^T D2 A, Berlekamp-Massey on the device, the lcm over the K projections and the factor x^e on the host.
// ------------------------------------------------------------------------------------------------
namespace {

// n, m, K, tries used, products with A, launches, degree of f, multiplicity of x in f, device us of the sequences, device us of
// Berlekamp-Massey
thread_local i64 g_precond_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void precond_stats_reset() { memset(g_precond_stats, 0, sizeof g_precond_stats); }

// The diagonals of the preconditioners.  The words of one diagonal differ from each other as long as that is possible (the
// first p - 1 of them): D I = D must have a minimal polynomial of full degree for the determinant of the identity to be certain,
// and independent words repeat with the probability of the birthday problem (64 of 126: all but certainly).  So word (which, i)
// is 1 + P_b(i mod N), N = p - 1, b = i div N, with P_b a pseudo-random permutation of 0 .. N - 1: four Feistel rounds on two
// halves of h = ceil(bits(N - 1) / 2) bits, (L, R) <- (R, L xor (w & (2^h - 1))), w the splitmix64 output of the state
// seed + 0x9E3779B97F4A7C15 * ((which + 1) * 2^60 + b * 2^20 + r * 2^16 + R) in round r, repeated while the result is >= N (a
// permutation of 0 .. 2^(2h) - 1 walked along its cycle back into 0 .. N - 1: a permutation of these; 2^(2h) < 4 N).  which = 1
// squares the word mod p.  The multiplier is odd, so distinct indices give distinct states, and the indices of minpoly_vectors
// stay below 2^32 (2 * n * K + 1 <= 2^31 + 1 for n < 2^24, K <= 64) while these start at 2^60.
void precond_diagonal(int len, uint64_t seed, int which, i64 prime, int *d)
{
    const uint64_t p = (uint64_t)prime, N = p - 1;
    int bits = 0;
    while (bits < 32 && ((N - 1) >> bits) != 0) bits++;
    const int h = std::max(1, (bits + 1) / 2);
    const uint64_t mask = ((uint64_t)1 << h) - 1;
    for (int i = 0; i < len; i++) {
        const uint64_t base = (((uint64_t)which + 1) << 60) + (((uint64_t)i / N) << 20);
        uint64_t x = (uint64_t)i % N;
        do {
            uint64_t L = x >> h, R = x & mask;
            for (uint64_t r = 0; r < 4; r++) {
                const uint64_t t = L ^ (minpoly_mix(seed + 0x9E3779B97F4A7C15ULL * (base + (r << 16) + R)) & mask);
                L = R;
                R = t;
            }
            x = (L << h) | R;
        } while (x >= N);
        uint64_t w = 1 + x;
        if (which == 1) w = w * w % p;
        d[i] = hbalanced(w, p);
    }
}

// what the tries of rank or determinant keep from one to the next
struct PrecondTry {
    DevBuf<int> dU, dV, dl, dr;
    std::vector<int> hu, hv, diag;
    SeqRecurrences R;
};

// One try with the seed `seed`: the diagonals and vectors of the seed go up, the sequence of len terms and Berlekamp-Massey run,
// and the lcm over K comes back.  Tr == NULL: D A on the view Fw of a square matrix; else E A^T D2 A on the two views of the
// n x m matrix.  g (may be NULL) receives the left diagonal as residues in [0, p).  A projection whose polynomial has more than
// md roots away from 0 is refused, and so is such an lcm.
HPoly precond_try(PrecondTry &T, const SpmvView &Fw, const SpmvView *Tr, const ZpField &F, int K, uint64_t seed, int len, int md, std::vector<uint64_t> *g)
{
    const int n = Fw.rows, dim = Tr ? Fw.cols : Fw.rows;
    const uint64_t p = (uint64_t)F.p;
    hipStream_t s = nullptr;
    const size_t nk = (size_t)dim * K;
    T.hu.resize(nk);
    T.hv.resize(nk);
    minpoly_vectors(dim, K, seed, F.p, T.hu.data(), T.hv.data());
    T.dU.ensure(nk);
    T.dV.ensure(nk);
    T.dl.ensure((size_t)n);
    HIPCHK(hipMemcpyAsync(T.dU.p, T.hu.data(), nk * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(T.dV.p, T.hv.data(), nk * sizeof(int), hipMemcpyHostToDevice, s));
    T.diag.resize((size_t)n + (size_t)(Tr ? dim : 0));
    precond_diagonal(n, seed, 0, F.p, T.diag.data());
    HIPCHK(hipMemcpyAsync(T.dl.p, T.diag.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if (g) {
        g->resize((size_t)n);
        for (int i = 0; i < n; i++) (*g)[(size_t)i] = hresidue(T.diag[(size_t)i], p);
    }
    if (Tr) {
        precond_diagonal(dim, seed, 1, F.p, T.diag.data() + n);
        T.dr.ensure((size_t)dim);
        HIPCHK(hipMemcpyAsync(T.dr.p, T.diag.data() + n, (size_t)dim * sizeof(int), hipMemcpyHostToDevice, s));
    }
    const SeqRecurrences::Run run = T.R.run({&Fw, Tr, T.dl.p, T.dr.p}, F, K, len, T.dU.p, T.dV.p, s);
    i64 *st = g_precond_stats;
    st[3]++;
    st[4] += (i64)(len - 1) * (Tr ? 2 : 1);
    st[5] += run.launches;
    st[8] += run.sequence_us;
    st[9] += run.bm_us;
    HPoly r(1, 1);
    for (int c = 0; c < K; c++) {
        const HPoly f = T.R.poly(c, p);
        const size_t e = hpoly_valuation(f);
        if ((i64)f.size() - 1 - (i64)e > md) {
            char msg[160];
            snprintf(msg, sizeof msg, "degree bound too small (projection %d has degree %d with x^%d, maxdeg %d)", c, T.R.deg[(size_t)c], (int)e, md);
            throw EngineError(msg);
        }
        r = hpoly_lcm(r, f, p);
    }
    if ((i64)r.size() - 1 - (i64)hpoly_valuation(r) > md) throw EngineError("degree bound too small (the lcm of the projections exceeds maxdeg)");
    return r;
}

int precond_tries(int tries) { return tries <= 0 ? 3 : tries; }

void precond_limits(int n, int m)
{
    if (n >= (1 << 24) || m >= (1 << 24)) throw EngineError("preconditioned Wiedemann limited to n, m < 2^24");
}

// The rank behind the three entries: Fw and Tr are the two views of the n x m matrix, n > 0, m > 0.
void precond_rank_run(const SpmvView &Fw, const SpmvView &Tr, const ZpField &F, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain)
{
    const int n = Fw.rows, m = Fw.cols, mn = std::min(n, m);
    const int md = degree_bound(maxdeg, mn);
    // 2 * md + 2 terms: f = x^e g may have one more degree than its g (see the header)
    const int len = 2 * md + 2;
    bm_check_len(F, len);
    i64 *st = g_precond_stats;
    st[0] = n;
    st[1] = m;
    st[2] = K;
    PrecondTry T;
    i64 best = -1;
    const int ntries = precond_tries(tries);
    for (int t = 0; t < ntries && best < mn; t++) {
        const HPoly f = precond_try(T, Fw, &Tr, F, K, seed + (uint64_t)t, len, md, nullptr);
        const size_t e = hpoly_valuation(f);
        const i64 bound = (i64)f.size() - 1 - (i64)e;
        if (bound > best) {
            best = bound;
            st[6] = (i64)f.size() - 1;
            st[7] = (i64)e;
        }
    }
    *rank = best;
    *certain = best == mn;
}

// The determinant behind the three entries: V is the view of the square matrix, n > 0.
void precond_det_run(const SpmvView &V, const ZpField &F, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    const int n = V.rows;
    const uint64_t p = (uint64_t)F.p;
    const int len = 2 * n;
    bm_check_len(F, len);
    i64 *st = g_precond_stats;
    st[0] = n;
    st[1] = n;
    st[2] = K;
    PrecondTry T;
    std::vector<uint64_t> d;
    const int ntries = precond_tries(tries);
    for (int t = 0; t < ntries; t++) {
        const HPoly f = precond_try(T, V, nullptr, F, K, seed + (uint64_t)t, len, n, &d);
        const size_t e = hpoly_valuation(f);
        st[6] = (i64)f.size() - 1;
        st[7] = (i64)e;
        if (e > 0) { // x divides a divisor of the minimal polynomial of D A: A is singular
            *det = 0;
            *status = 1;
            return;
        }
        if ((int)f.size() - 1 == n) { // f is the characteristic polynomial of D A: det(D A) = (-1)^n f(0)
            uint64_t prod = 1;
            for (uint64_t w : d) prod = prod * w % p;
            uint64_t v = f[0] * hinv(prod, p) % p;
            if (n & 1) v = (p - v) % p;
            *det = hbalanced(v, p);
            *status = 1;
            return;
        }
    }
    *det = 0;
    *status = 0;
}

void precond_sequence(spasm_amd_spmv *op, int mode, int K, int len, const spasm_ZZp *dl, const spasm_ZZp *dr, const spasm_ZZp *U, i64 ldu,
                      const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    if (!op) throw EngineError("NULL operator");
    if (mode != 0 && mode != 1) throw EngineError("mode must be 0 (D A) or 1 (E A^T D2 A)");
    const int n = op->A.n, m = op->A.m;
    if (mode == 0) require_square(-1, n, m);
    if (K < 1 || K > 64) throw EngineError("K out of range (1 <= K <= 64)");
    if (len < 0 || (i64)len * 64 >= ((i64)1 << 31) || ldu < K || ldv < K) throw EngineError("bad arguments (0 <= len < 2^25, ldu >= K, ldv >= K)");
    if (len == 0) return;
    if (!S || (m > 0 && (!U || !V)) || (n > 0 && !dl) || (mode == 1 && m > 0 && !dr)) throw EngineError("NULL array");
    const uint64_t p = (uint64_t)op->F.p;
    if (n == 0 || m == 0) { // the operator is zero: s_0 = U^T V on the host, every later term is 0
        memset(S, 0, (size_t)len * K * sizeof(int));
        for (int c = 0; c < K; c++) {
            uint64_t a = 0;
            for (i64 r = 0; r < m; r++) a = (a + hresidue(U[r * ldu + c], p) * hresidue(V[r * ldv + c], p)) % p;
            S[c] = hbalanced(a, p);
        }
        return;
    }
    DeviceGuard g(op);
    if (mode == 1) op->build_transpose();
    const size_t dim = (size_t)m, kk = (size_t)K;
    hipStream_t s = nullptr;
    DevBuf<int> dU, dV, dS, ddl, ddr;
    KrylovWork W;
    dU.alloc(dim * kk);
    dV.alloc(dim * kk);
    dS.alloc((size_t)len * kk);
    ddl.alloc((size_t)n);
    HIPCHK(hipMemcpy2DAsync(dU.p, kk * sizeof(int), U, (size_t)ldu * sizeof(int), kk * sizeof(int), dim, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpy2DAsync(dV.p, kk * sizeof(int), V, (size_t)ldv * sizeof(int), kk * sizeof(int), dim, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ddl.p, dl, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if (mode == 1) {
        ddr.alloc(dim);
        HIPCHK(hipMemcpyAsync(ddr.p, dr, dim * sizeof(int), hipMemcpyHostToDevice, s));
    }
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    const int launches = sequence_run({&op->fwd, mode == 1 ? &op->tr : nullptr, ddl.p, ddr.p}, op->F, K, len, dU.p, K, dV.p, K, W, dS.p, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> out((size_t)len * kk);
    HIPCHK(hipMemcpyAsync(out.data(), dS.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 *st = g_precond_stats;
    st[0] = n;
    st[1] = m;
    st[2] = K;
    st[4] = (i64)(len - 1) * (mode == 1 ? 2 : 1);
    st[5] = launches;
    st[8] = (i64)(ev.ms(0, 1) * 1000.0);
    memcpy(S, out.data(), out.size() * sizeof(int));
}

int rank_entry(Operand &&o, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain)
{
    precond_stats_reset();
    o.check();
    K = minpoly_K(K);
    if (!rank || !certain) throw EngineError("NULL array");
    precond_limits(o.n, o.m);
    if (o.n == 0 || o.m == 0) { *rank = 0; *certain = 1; return 0; }
    o.views(true, true);
    i64 r = 0;
    int c = 0;
    precond_rank_run(*o.fwd, *o.tr, o.F, K, seed, tries, maxdeg, &r, &c);
    *rank = r;
    *certain = c;
    return 0;
}

int det_entry(Operand &&o, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    precond_stats_reset();
    o.check();
    require_square(-1, o.n, o.m);
    K = minpoly_K(K);
    if (!det || !status) throw EngineError("NULL array");
    precond_limits(o.n, o.m);
    if (o.n == 0) { *det = 1; *status = 1; return 0; }
    o.views(true, false);
    spasm_ZZp v = 0;
    int st = 0;
    precond_det_run(*o.fwd, o.F, K, seed, tries, &v, &st);
    *det = v;
    *status = st;
    return 0;
}

} // namespace

extern "C" {

// ---- rank and determinant by preconditioned Wiedemann (precond.hpp; engine extension) ----
SPASM_API int spasm_amd_precond_diagonal(int len, uint64_t seed, int which, i64 prime, spasm_ZZp *d)
{
    return abi_call("spasm_amd_precond_diagonal", -1, [&] {
        precond_stats_reset();
        if (len < 0 || (which != 0 && which != 1)) throw EngineError("bad arguments (len >= 0, which 0 or 1)");
        check_prime(prime);
        if (len > 0 && !d) throw EngineError("NULL array");
        precond_diagonal(len, seed, which, prime, d);
        return 0;
    });
}

SPASM_API int spasm_amd_precond_sequence(spasm_amd_spmv *op, int mode, int K, int len, const spasm_ZZp *d_left, const spasm_ZZp *d_right,
                                         const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    return abi_call("spasm_amd_precond_sequence", -1, [&] {
        precond_stats_reset();
        precond_sequence(op, mode, K, len, d_left, d_right, U, ldu, V, ldv, S);
        return 0;
    });
}

SPASM_API int spasm_amd_wiedemann_rank(const struct spasm_csr *A, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain)
{
    return abi_call("spasm_amd_wiedemann_rank", -1, [&] { return rank_entry(Operand(A, "spasm_amd_wiedemann_rank"), K, seed, tries, maxdeg, rank, certain); });
}

SPASM_API int spasm_amd_spmv_wiedemann_rank(spasm_amd_spmv *op, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain)
{
    return abi_call("spasm_amd_spmv_wiedemann_rank", -1, [&] { return rank_entry(Operand(op), K, seed, tries, maxdeg, rank, certain); });
}

SPASM_API int spasm_amd_dcsr_wiedemann_rank(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain)
{
    return abi_call("spasm_amd_dcsr_wiedemann_rank", -1, [&] { return rank_entry(Operand(D), K, seed, tries, maxdeg, rank, certain); });
}

SPASM_API int spasm_amd_wiedemann_det(const struct spasm_csr *A, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_wiedemann_det", -1, [&] { return det_entry(Operand(A, "spasm_amd_wiedemann_det"), K, seed, tries, det, status); });
}

SPASM_API int spasm_amd_spmv_wiedemann_det(spasm_amd_spmv *op, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_spmv_wiedemann_det", -1, [&] { return det_entry(Operand(op), K, seed, tries, det, status); });
}

SPASM_API int spasm_amd_dcsr_wiedemann_det(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_dcsr_wiedemann_det", -1, [&] { return det_entry(Operand(D), K, seed, tries, det, status); });
}

SPASM_API void spasm_amd_precond_stats(i64 *out)
{
    if (out) memcpy(out, g_precond_stats, sizeof g_precond_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Block Wiedemann (block_krylov.hpp, block_bm.hpp): the b x b projected sequence of A, A^T or D A, its left generator by
// Berlekamp-Massey over matrix sequences, and the determinant from the generator.
// ------------------------------------------------------------------------------------------------
namespace {

// what a block sequence adds to the terms the generic case needs (2 * ceil(n / b)): the two terms of sequence_terms
constexpr int BLOCK_SLACK = 2;

int block_terms(int n, int b) { return 2 * ((n + b - 1) / b) + BLOCK_SLACK; }

void block_sequence_check(const spasm_amd_spmv *op, int trans, int b, i64 len, const void *U, i64 ldu, const void *V, i64 ldv, const void *S)
{
    if (!op) throw EngineError("NULL operator");
    block_width(b);
    require_square(-1, op->A.n, op->A.m);
    if (len < 1 || len >= ((i64)1 << 24)) throw EngineError("len out of range (1 <= len < 2^24)");
    if (ldu < b || ldv < b || (trans != 0 && trans != 1)) throw EngineError("bad arguments (trans 0/1, ldu >= b, ldv >= b)");
    if (!S || (op->A.n > 0 && (!U || !V))) throw EngineError("NULL array");
}

// a zero word (mod p) of the caller's diagonal is refused: D must be invertible
void block_diagonal_check(const int *d, int n, i64 prime)
{
    for (int i = 0; i < n; i++)
        if ((i64)d[i] % prime == 0) {
            char msg[96];
            snprintf(msg, sizeof msg, "d_left[%d] is zero mod p", i);
            throw EngineError(msg);
        }
}

// the b x b determinant mod p of residues in [0, p), by elimination on the host (exact: products of two residues fit a u64)
uint64_t hdet_small(std::vector<uint64_t> a, int b, uint64_t p)
{
    uint64_t det = 1;
    for (int c = 0; c < b; c++) {
        int piv = -1;
        for (int r = c; r < b && piv < 0; r++)
            if (a[(size_t)r * b + c] != 0) piv = r;
        if (piv < 0) return 0;
        if (piv != c) {
            for (int k = 0; k < b; k++) std::swap(a[(size_t)piv * b + k], a[(size_t)c * b + k]);
            det = (p - det) % p;
        }
        const uint64_t pv = a[(size_t)c * b + c], inv = hinv(pv, p);
        det = det * pv % p;
        for (int r = c + 1; r < b; r++) {
            const uint64_t f = a[(size_t)r * b + c] * inv % p;
            if (f == 0) continue;
            const uint64_t nf = p - f;
            for (int k = c; k < b; k++) a[(size_t)r * b + k] = (a[(size_t)r * b + k] + nf * a[(size_t)c * b + k]) % p;
        }
    }
    return det;
}

// The determinant behind the three entries: V is the view of the square matrix, n > 0.  Per try: D and U, V of the seed, the
// block sequence of D A with block_terms(n, b) terms, its generator F; when the row degrees sum to n,
// det A = (-1)^n det F_0 / det(leading row coefficients) / prod d_i.  Monte Carlo: see the header.
void block_det_run(const SpmvView &V, const ZpField &F, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    const int n = V.rows;
    const uint64_t p = (uint64_t)F.p;
    const int len = block_terms(n, b);
    block_bm_check_len(len);
    hipStream_t s = nullptr;
    const size_t nb = (size_t)n * b, bb = (size_t)b * b;
    std::vector<int> hu(nb), hv(nb), diag((size_t)n), hdeg((size_t)b + 1), row((size_t)b);
    DevBuf<int> dU, dV, dl, dS, d_coef, d_small;
    KrylovWork W;
    BlockBmWork BW;
    SpgEvents ev;
    dU.alloc(nb);
    dV.alloc(nb);
    dl.alloc((size_t)n);
    dS.alloc((size_t)len * bb);
    d_coef.alloc(((size_t)len + 1) * bb);
    d_small.alloc((size_t)b + 1);
    i64 *st = g_block_stats;
    st[0] = b;
    st[1] = len;
    st[8] = n;
    const int ntries = precond_tries(tries);
    *det = 0;
    *status = 0;
    for (int t = 0; t < ntries; t++) {
        const uint64_t sd = seed + (uint64_t)t;
        minpoly_vectors(n, b, sd, F.p, hu.data(), hv.data());
        precond_diagonal(n, sd, 0, F.p, diag.data());
        HIPCHK(hipMemcpyAsync(dU.p, hu.data(), nb * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dV.p, hv.data(), nb * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dl.p, diag.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev.e[0], s));
        SeqOperator op{&V, nullptr, dl.p, nullptr};
        op.block = true;
        int launches = sequence_run(op, F, b, len, dU.p, b, dV.p, b, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        launches += block_bm_device(F, b, len, dS.p, BW, d_coef.p, d_small.p, d_small.p + b, s);
        HIPCHK(hipEventRecord(ev.e[2], s));
        HIPCHK(hipMemcpyAsync(hdeg.data(), d_small.p, hdeg.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        i64 sum = 0;
        for (int r = 0; r < b; r++) sum += hdeg[(size_t)r];
        st[2] += len - 1;
        st[3] += launches;
        st[4] = sum;
        st[5]++;
        st[6] += (i64)(ev.ms(0, 1) * 1000.0);
        st[7] += (i64)(ev.ms(1, 2) * 1000.0);
        st[9] = hdeg[(size_t)b];
        if (sum != n) continue;
        // F_0 is term 0 of coef; the leading coefficient of row r is row r of term rowdeg[r]
        std::vector<uint64_t> f0(bb), lc(bb);
        std::vector<int> h0(bb);
        HIPCHK(hipMemcpy(h0.data(), d_coef.p, bb * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < bb; e++) f0[e] = hresidue(h0[e], p);
        for (int r = 0; r < b; r++) {
            HIPCHK(hipMemcpy(row.data(), d_coef.p + ((size_t)hdeg[(size_t)r] * b + r) * b, (size_t)b * sizeof(int), hipMemcpyDeviceToHost));
            for (int c = 0; c < b; c++) lc[(size_t)r * b + c] = hresidue(row[(size_t)c], p);
        }
        const uint64_t dlc = hdet_small(lc, b, p);
        if (dlc == 0) continue; // cannot happen (the generator is row-reduced); try the next seed rather than divide by it
        uint64_t prod = 1;
        for (int i = 0; i < n; i++) prod = prod * hresidue(diag[(size_t)i], p) % p;
        uint64_t v = hdet_small(f0, b, p) * hinv(dlc, p) % p * hinv(prod, p) % p;
        if (n & 1) v = (p - v) % p;
        *det = hbalanced(v, p);
        *status = 1;
        return;
    }
}

int block_det_entry(Operand &&o, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    block_stats_reset();
    o.check();
    require_square(-1, o.n, o.m);
    block_width(b);
    if (!det || !status) throw EngineError("NULL array");
    precond_limits(o.n, o.m);
    if (o.n == 0) { *det = 1; *status = 1; return 0; }
    o.views(true, false);
    spasm_ZZp v = 0;
    int st = 0;
    block_det_run(*o.fwd, o.F, b, seed, tries, &v, &st);
    *det = v;
    *status = st;
    return 0;
}

} // namespace

extern "C" {

// ---- block Wiedemann (block_krylov.hpp, block_bm.hpp; engine extension) ----
SPASM_API int spasm_amd_block_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,
                                       const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    return abi_call("spasm_amd_block_sequence", -1, [&] {
        block_stats_reset();
        block_sequence_check(op, trans, b, len, U, ldu, V, ldv, S);
        const size_t n = (size_t)op->A.n, kk = (size_t)b, bb = kk * kk;
        if (d_left) block_diagonal_check(d_left, (int)n, op->F.p);
        if (n == 0) { memset(S, 0, (size_t)len * bb * sizeof(int)); return 0; }
        DeviceGuard g(op);
        if (trans) op->build_transpose();
        hipStream_t s = nullptr;
        DevBuf<int> dU, dV, dS, dl;
        KrylovWork W;
        dU.alloc(n * kk);
        dV.alloc(n * kk);
        dS.alloc((size_t)len * bb);
        HIPCHK(hipMemcpy2DAsync(dU.p, kk * sizeof(int), U, (size_t)ldu * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpy2DAsync(dV.p, kk * sizeof(int), V, (size_t)ldv * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
        if (d_left) {
            dl.alloc(n);
            HIPCHK(hipMemcpyAsync(dl.p, d_left, n * sizeof(int), hipMemcpyHostToDevice, s));
        }
        SpgEvents ev;
        HIPCHK(hipEventRecord(ev.e[0], s));
        SeqOperator sq{trans ? &op->tr : &op->fwd, nullptr, d_left ? dl.p : nullptr, nullptr};
        sq.block = true;
        const int launches = sequence_run(sq, op->F, b, len, dU.p, b, dV.p, b, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        std::vector<int> out((size_t)len * bb);
        HIPCHK(hipMemcpyAsync(out.data(), dS.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        i64 *st = g_block_stats;
        st[0] = b;
        st[1] = len;
        st[2] = len - 1;
        st[3] = launches;
        st[6] = (i64)(ev.ms(0, 1) * 1000.0);
        st[8] = (i64)n;
        memcpy(S, out.data(), out.size() * sizeof(int));
        return 0;
    });
}

SPASM_API int spasm_amd_block_sequence_dev(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,
                                           const spasm_ZZp *V, i64 ldv, spasm_ZZp *S, void *stream)
{
    return abi_call("spasm_amd_block_sequence_dev", -1, [&] {
        block_stats_reset();
        block_sequence_check(op, trans, b, len, U, ldu, V, ldv, S);
        DeviceGuard g(op);
        hipStream_t s = (hipStream_t)stream;
        if (op->A.n == 0) {
            HIPCHK(hipMemsetAsync(S, 0, (size_t)len * b * b * sizeof(int), s));
            return 0;
        }
        if (trans) op->build_transpose();
        SeqOperator sq{trans ? &op->tr : &op->fwd, nullptr, d_left, nullptr};
        sq.block = true;
        const int launches = sequence_run(sq, op->F, b, len, U, ldu, V, ldv, op->kry, S, s);
        if (!stream) HIPCHK(hipStreamSynchronize(s));
        i64 *st = g_block_stats;
        st[0] = b;
        st[1] = len;
        st[2] = len - 1;
        st[3] = launches;
        st[8] = op->A.n;
        return 0;
    });
}

SPASM_API int spasm_amd_block_berlekamp_massey(int b, int len, const spasm_ZZp *S, i64 prime, spasm_ZZp *coef, int *rowdeg, int *dmax)
{
    return abi_call("spasm_amd_block_berlekamp_massey", -1, [&] { DeviceGuard g; block_berlekamp_massey(b, len, S, prime, coef, rowdeg, dmax); return 0; });
}

SPASM_API int spasm_amd_block_wiedemann_det(const struct spasm_csr *A, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_block_wiedemann_det", -1,
                    [&] { return block_det_entry(Operand(A, "spasm_amd_block_wiedemann_det"), b, seed, tries, det, status); });
}

SPASM_API int spasm_amd_spmv_block_wiedemann_det(spasm_amd_spmv *op, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_spmv_block_wiedemann_det", -1, [&] { return block_det_entry(Operand(op), b, seed, tries, det, status); });
}

SPASM_API int spasm_amd_dcsr_block_wiedemann_det(const spasm_amd_dcsr *D, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status)
{
    return abi_call("spasm_amd_dcsr_block_wiedemann_det", -1, [&] { return block_det_entry(Operand(D), b, seed, tries, det, status); });
}

SPASM_API void spasm_amd_block_stats(i64 *out)
{
    if (out) memcpy(out, g_block_stats, sizeof g_block_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Block Wiedemann solve (block_horner.hpp): a matrix polynomial applied to a block of vectors by block Horner steps, and on top of
// it sparse solves from the right generator of a block sequence that certify their own answers.
// ------------------------------------------------------------------------------------------------
#include "block_horner.hpp"

namespace {

// n, b, K, len, tries used, products with A, those of the sequences, those of Horner and the check, launches, sum of the row
// degrees (last try), largest row degree, columns solved, columns with a kernel vector, device us of the sequences, of
// Berlekamp-Massey, of Horner + check
constexpr int BLOCK_SOLVE_NSTATS = 16;
thread_local i64 g_block_solve_stats[BLOCK_SOLVE_NSTATS] = {0};

void block_solve_stats_reset() { memset(g_block_solve_stats, 0, sizeof g_block_solve_stats); }

// the steps of table slices T[0 .. rows) (B x KW words each) from Y = 0: the first is the plain combination, rows - 1 products
// follow.  The last step writes Yout (leading dimension ldyo) and, when cnt is given, adds its non-zero counts to cnt[0 .. KW); the
// steps between ping-pong in W.  With op.tr a product is two launch sets, M = A^T D2 A: fwd with DiagEpi{d2} writes W.mid, tr with
// BlockHornerEpi reads it (BlockHornerEpi has no diagonal: E = I).
template <bool SMALL, int B, int KW>
int block_horner_launch(const SeqOperator &op, const ZpField &F, int kc, int rows, const int *T, const int *Vb, i64 ldv, int *Yout, i64 ldyo, KrylovWork &W,
                        long long *cnt, int cap, hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp, n = op.dim();
    int launches = 0;
    const int *X = nullptr;
    i64d ldx = 0;
    for (int i = 0; i < rows && n > 0; i++) {
        const bool last = i == rows - 1;
        int *Y = last ? Yout : (X == W.w0.p ? W.w1.p : W.w0.p);
        const i64d ldy = last ? (i64d)ldyo : (i64d)KW;
        long long *cp = last ? cnt : nullptr;
        const int *Ti = T + (size_t)i * B * KW;
        if (!X) {
            hipLaunchKernelGGL((k_block_horner_first<SMALL, B, KW>), step_grid((i64)n * KW, cap), dim3(KRY_BS), 0, s, n, kc, F, hp, mhp, Ti, Vb, (i64d)ldv, Y,
                               ldy, cp);
            launches++;
        } else if (op.tr) {
            launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, W.mid.p, (i64d)KW, DiagEpi{op.dl, nullptr, 0, nullptr}, cap, s);
            launches += spmv_step_launch<SMALL, KW>(*op.tr, F, kc, W.mid.p, (i64d)KW, Y, ldy, BlockHornerEpi<SMALL, B>{Ti, Vb, (i64d)ldv, KW, cp}, cap, s);
        } else {
            launches += spmv_step_launch<SMALL, KW>(*op.fwd, F, kc, X, ldx, Y, ldy, BlockHornerEpi<SMALL, B>{Ti, Vb, (i64d)ldv, KW, cp}, cap, s);
        }
        HIPCHK(hipGetLastError());
        X = Y;
        ldx = ldy;
    }
    return launches;
}

// rows >= 1 block Horner steps on device arrays, enqueued on s; no host synchronization.  Vb is dim x b (leading dimension ldv), T
// the device table, rows x b x spmv_kw(K) canonical residues; Yout gets K columns.  op is A (fwd alone) or A^T D2 A (fwd, tr and
// dl = D2; dr is not applied).  Returns the launches.
int block_horner_run(const SeqOperator &op, const ZpField &F, int b, int K, int rows, const int *T, const int *Vb, i64 ldv, int *Yout, i64 ldyo,
                     KrylovWork &W, long long *cnt, hipStream_t s)
{
    const int kw = spmv_kw(K), cap = step_grid_cap();
    const size_t words = (size_t)op.dim() * kw;
    if (rows > 1) {
        W.w0.ensure(words);
        if (rows > 2) W.w1.ensure(words);
        if (op.tr) W.mid.ensure((size_t)op.fwd->rows * kw);
    }
    auto go = [&](auto B) {
        return dispatch_kw(kw, [&](auto KW) -> int {
            if constexpr (KW() <= B()) {
                return F.small ? block_horner_launch<true, B(), KW()>(op, F, K, rows, T, Vb, ldv, Yout, ldyo, W, cnt, cap, s)
                               : block_horner_launch<false, B(), KW()>(op, F, K, rows, T, Vb, ldv, Yout, ldyo, W, cnt, cap, s);
            } else {
                throw EngineError("K out of range (1 <= K <= b)");
            }
        });
    };
    switch (b) {
    case 2: return go(std::integral_constant<int, 2>());
    case 4: return go(std::integral_constant<int, 4>());
    case 8: return go(std::integral_constant<int, 8>());
    default: return go(std::integral_constant<int, 16>());
    }
}

void block_poly_check(const spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv, const spasm_ZZp *X,
                      i64 ldx)
{
    if (!op) throw EngineError("NULL operator");
    block_width(b);
    require_square(-1, op->A.n, op->A.m);
    if (K < 1 || K > b) throw EngineError("K out of range (1 <= K <= b)");
    if (trans != 0 && trans != 1) throw EngineError("trans must be 0 or 1");
    if (D < -1 || D >= (1 << 24)) throw EngineError("D out of range (-1 <= D < 2^24)");
    if (ldv < b) throw EngineError("ldv < b");
    if (ldx < K) throw EngineError("ldx < K");
    if (D >= 0 && !coef) throw EngineError("NULL array");
    const i64 n = op->A.n;
    if (n > 0) {
        if (!V || !X) throw EngineError("NULL array");
        const uintptr_t v0 = (uintptr_t)V, v1 = v0 + (size_t)((n - 1) * ldv + b) * sizeof(int);
        const uintptr_t x0 = (uintptr_t)X, x1 = x0 + (size_t)((n - 1) * ldx + K) * sizeof(int);
        if (v0 < x1 && x0 < v1) throw EngineError("V must not overlap X");
    }
}

// X <- sum_{t <= D} op(A)^t V C_t on device arrays, enqueued on s: the table goes up once (slice i holds C_{D - i}), then D
// products.  Returns the launches.
int block_poly_apply_dev(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const int *dV, i64 ldv, int *dX, i64 ldx, hipStream_t s)
{
    const size_t n = (size_t)op->A.n;
    if (D < 0) {
        HIPCHK(hipMemset2DAsync(dX, (size_t)ldx * sizeof(int), 0, (size_t)K * sizeof(int), n, s));
        return 0;
    }
    if (trans) op->build_transpose();
    const SpmvView &view = trans ? op->tr : op->fwd;
    KrylovWork &W = op->kry;
    // the host copy of the previous call's table may still be on its way up
    if (W.tab_up) HIPCHK(hipEventSynchronize(W.tab_up));
    else HIPCHK(hipEventCreateWithFlags(&W.tab_up, hipEventDisableTiming));
    const int kw = spmv_kw(K);
    const uint64_t p = (uint64_t)op->F.p;
    W.htab.assign((size_t)(D + 1) * b * kw, 0);
    for (int i = 0; i <= D; i++)
        for (int c = 0; c < b; c++)
            for (int j = 0; j < K; j++)
                W.htab[((size_t)i * b + c) * kw + j] = hbalanced(hresidue(coef[((size_t)(D - i) * b + c) * K + j], p), p);
    W.tab.ensure(W.htab.size());
    HIPCHK(hipMemcpyAsync(W.tab.p, W.htab.data(), W.htab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(W.tab_up, s));
    return block_horner_run({&view}, op->F, b, K, D + 1, W.tab.p, dV, ldv, dX, ldx, W, nullptr, s);
}

void block_poly_stats(i64 n, int b, int K, int D, int launches)
{
    i64 *st = g_block_solve_stats;
    st[0] = n;
    st[1] = b;
    st[2] = K;
    st[5] = st[7] = std::max(D, 0);
    st[8] = launches;
}

void block_wied_check(int n, int m, int trans, int b, int K, const void *B, i64 ldb, const void *X, i64 ldx, const int *status)
{
    require_square(-1, n, m);
    block_width(b);
    if (K < 1 || K > b) throw EngineError("K out of range (1 <= K <= b)");
    if (trans != 0 && trans != 1) throw EngineError("trans must be 0 or 1");
    if (ldb < K) throw EngineError("ldb < K");
    if (ldx < K) throw EngineError("ldx < K");
    if (!status || (n > 0 && (!B || !X))) throw EngineError("NULL array");
    if (n >= (1 << 24)) throw EngineError("Wiedemann solve limited to n < 2^24");
}

// Gauss-Jordan on [G | I] over GF(p), G b x b residues in [0, p): column by column, the first row at or below the rank with a
// non-zero word is swapped up, scaled to 1 and cleared from every other row.  Leaves R = T G reduced, T in t; returns the rank and
// in pivrow[c] the row whose pivot is column c (-1: none).  Rows rank .. b - 1 of R are zero: those rows of T span the left null
// space of G, in this order.
int block_reduce_g(std::vector<uint64_t> &g, std::vector<uint64_t> &t, int b, uint64_t p, std::vector<int> &pivrow)
{
    t.assign((size_t)b * b, 0);
    for (int r = 0; r < b; r++) t[(size_t)r * b + r] = 1;
    pivrow.assign((size_t)b, -1);
    int rank = 0;
    for (int c = 0; c < b && rank < b; c++) {
        int piv = -1;
        for (int r = rank; r < b && piv < 0; r++)
            if (g[(size_t)r * b + c] != 0) piv = r;
        if (piv < 0) continue;
        if (piv != rank)
            for (int k = 0; k < b; k++) {
                std::swap(g[(size_t)piv * b + k], g[(size_t)rank * b + k]);
                std::swap(t[(size_t)piv * b + k], t[(size_t)rank * b + k]);
            }
        const uint64_t inv = hinv(g[(size_t)rank * b + c], p);
        for (int k = 0; k < b; k++) {
            g[(size_t)rank * b + k] = g[(size_t)rank * b + k] * inv % p;
            t[(size_t)rank * b + k] = t[(size_t)rank * b + k] * inv % p;
        }
        for (int r = 0; r < b; r++) {
            const uint64_t f = g[(size_t)r * b + c];
            if (r == rank || f == 0) continue;
            const uint64_t nf = p - f;
            for (int k = 0; k < b; k++) {
                g[(size_t)r * b + k] = (g[(size_t)r * b + k] + nf * g[(size_t)rank * b + k] % p) % p;
                t[(size_t)r * b + k] = (t[(size_t)r * b + k] + nf * t[(size_t)rank * b + k] % p) % p;
            }
        }
        pivrow[(size_t)c] = rank++;
    }
    return rank;
}

// The solve behind the three entries: V is the view of op(A), square, n > 0; the arguments have been checked.  Per try: U and
// [B | Z] of the seed, the block sequence, the left generator F of its transposed terms (a right generator of the sequence), the
// reduction of [F_0 | I], one combination h = lambda F per undecided column, the block Horner run and the residual with its counts.
// Nothing is written to X or status before every try has run.
void block_wied_run(const SpmvView &V, const ZpField &F, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, spasm_ZZp *X, i64 ldx,
                    int *status)
{
    const int n = V.rows, len = block_terms(n, b);
    const uint64_t p = (uint64_t)F.p;
    block_bm_check_len(len);
    const int ntries = tries <= 0 ? 3 : tries;
    hipStream_t s = nullptr;
    const size_t nb = (size_t)n * b, bb = (size_t)b * b;
    std::vector<int> outX((size_t)n * K, 0), outS((size_t)K, 0), act((size_t)K);
    for (int c = 0; c < K; c++) act[(size_t)c] = c;
    std::vector<int> hu(nb), hv(nb), hdeg((size_t)b + 1), hcoef, tab, hx, pivrow;
    std::vector<uint64_t> g, tg, lam((size_t)b);
    std::vector<long long> hcnt;
    std::vector<char> regular;
    DevBuf<int> dU, dV, dS, dSt, d_coef, d_small, dX, dR, dT;
    DevBuf<long long> dcnt;
    KrylovWork W;
    BlockBmWork BW;
    SpgEvents ev, evh;
    dU.alloc(nb);
    dV.alloc(nb);
    dS.alloc((size_t)len * bb);
    dSt.alloc((size_t)len * bb);
    d_coef.alloc(((size_t)len + 1) * bb);
    d_small.alloc((size_t)b + 1);
    i64 *st = g_block_solve_stats;
    st[0] = n;
    st[1] = b;
    st[2] = K;
    st[3] = len;
    for (int t = 0; t < ntries && !act.empty(); t++) {
        const int ka = (int)act.size(), kw = spmv_kw(ka);
        const size_t nk = (size_t)n * ka;
        // V = [B | Z]: the undecided right-hand sides, packed, over the leading columns of the seed's V
        minpoly_vectors(n, b, seed + (uint64_t)t, F.p, hu.data(), hv.data());
        for (int r = 0; r < n; r++)
            for (int a = 0; a < ka; a++) hv[(size_t)r * b + a] = B[(i64)r * ldb + act[(size_t)a]];
        HIPCHK(hipMemcpyAsync(dU.p, hu.data(), nb * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dV.p, hv.data(), nb * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev.e[0], s));
        SeqOperator op{&V};
        op.block = true;
        int launches = sequence_run(op, F, b, len, dU.p, b, dV.p, b, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        const i64 total = (i64)len * (i64)bb;
        hipLaunchKernelGGL(k_block_transpose_terms, dim3(cdiv(total, 256)), dim3(256), 0, s, (i64d)total, b, dS.p, dSt.p);
        HIPCHK(hipGetLastError());
        launches += 1 + block_bm_device(F, b, len, dSt.p, BW, d_coef.p, d_small.p, d_small.p + b, s);
        HIPCHK(hipEventRecord(ev.e[2], s));
        HIPCHK(hipMemcpyAsync(hdeg.data(), d_small.p, hdeg.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int D = hdeg[(size_t)b];
        hcoef.resize(((size_t)D + 1) * bb);
        HIPCHK(hipMemcpy(hcoef.data(), d_coef.p, hcoef.size() * sizeof(int), hipMemcpyDeviceToHost));
        i64 sum = 0;
        for (int r = 0; r < b; r++) sum += hdeg[(size_t)r];
        st[4] = t + 1;
        st[5] += len - 1;
        st[6] += len - 1;
        st[8] += launches;
        st[9] = sum;
        st[10] = std::max(st[10], (i64)D);
        st[13] += (i64)(ev.ms(0, 1) * 1000.0);
        st[14] += (i64)(ev.ms(1, 2) * 1000.0);
        // lambda_a F_0 = e_a where e_a lies in the row space of F_0 (column a is regular), else lambda_a F_0 = 0
        g.resize(bb);
        for (size_t e = 0; e < bb; e++) g[e] = hresidue(hcoef[e], p);
        const int rank = block_reduce_g(g, tg, b, p, pivrow), nullity = b - rank;
        // slice i of the table is C_{D - 1 - i} = -(h_{D - i} of the ka columns)^T; one more row for the check: -1 where x is
        // expected to solve the system, 0 where it is expected to lie in the kernel
        tab.assign((size_t)D * b * kw + kw, 0);
        regular.assign((size_t)ka, 0);
        for (int a = 0; a < ka; a++) {
            int lr = -1;
            const int pr = pivrow[(size_t)a];
            if (pr >= 0) {
                bool unit = true;
                for (int k = 0; k < b && unit; k++) unit = g[(size_t)pr * b + k] == (k == a ? 1u : 0u);
                if (unit) lr = pr;
            }
            regular[(size_t)a] = lr >= 0;
            if (lr < 0) lr = rank + a % nullity; // (a column that is not regular leaves nullity > 0)
            for (int k = 0; k < b; k++) lam[(size_t)k] = tg[(size_t)lr * b + k];
            for (int d = 1; d <= D; d++) {
                const int *Fd = hcoef.data() + (size_t)d * bb;
                for (int c = 0; c < b; c++) {
                    uint64_t h = 0;
                    for (int r = 0; r < b; r++) h += lam[(size_t)r] * hresidue(Fd[(size_t)r * b + c], p) % p;
                    tab[((size_t)(D - d) * b + c) * kw + a] = hbalanced((p - h % p) % p, p);
                }
            }
            tab[(size_t)D * b * kw + a] = regular[(size_t)a] ? -1 : 0;
        }
        dX.ensure(nk);
        dR.ensure((size_t)n * kw);
        dcnt.ensure((size_t)2 * kw);
        dT.ensure(tab.size());
        HIPCHK(hipMemcpyAsync(dT.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dcnt.p, 0, (size_t)2 * kw * sizeof(long long), s));
        HIPCHK(hipEventRecord(evh.e[0], s));
        launches = 0;
        if (D == 0) HIPCHK(hipMemsetAsync(dX.p, 0, nk * sizeof(int), s));
        else launches += block_horner_run({&V}, F, b, ka, D, dT.p, dV.p, b, dX.p, ka, W, dcnt.p, s);
        // the certificate: R <- op(A) X + r B, with the non-zero counts of X (above) and of R
        launches += horner_run(V, F, ka, 1, dT.p + (size_t)D * b * kw, dV.p, b, dX.p, ka, dR.p, kw, W, dcnt.p + kw, s);
        HIPCHK(hipEventRecord(evh.e[1], s));
        hcnt.resize((size_t)2 * kw);
        hx.resize(nk);
        HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt.p, hcnt.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hx.data(), dX.p, nk * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int hp_ = std::max(D - 1, 0) + 1;
        st[5] += hp_;
        st[7] += hp_;
        st[8] += launches;
        st[15] += (i64)(evh.ms(0, 1) * 1000.0);
        std::vector<int> left;
        for (int a = 0; a < ka; a++) {
            const int c = act[(size_t)a];
            const bool rzero = hcnt[(size_t)kw + a] == 0, xzero = hcnt[(size_t)a] == 0;
            int verdict = 0;
            if (regular[(size_t)a] && rzero) verdict = 1;
            else if (!regular[(size_t)a] && rzero && !xzero) verdict = 2;
            if (!verdict) {
                left.push_back(c);
                continue;
            }
            outS[(size_t)c] = verdict;
            st[10 + verdict]++;
            for (int r = 0; r < n; r++) outX[(size_t)r * K + c] = hx[(size_t)r * ka + a];
        }
        act.swap(left);
    }
    for (int r = 0; r < n; r++) memcpy(X + (i64)r * ldx, outX.data() + (size_t)r * K, (size_t)K * sizeof(int));
    memcpy(status, outS.data(), (size_t)K * sizeof(int));
}

int block_wied_entry(Operand &&o, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, spasm_ZZp *X, i64 ldx, int *status)
{
    block_solve_stats_reset();
    o.check();
    block_wied_check(o.n, o.m, trans, b, K, B, ldb, X, ldx, status);
    if (o.n == 0) {
        for (int c = 0; c < K; c++) status[c] = 1;
        g_block_solve_stats[1] = b;
        g_block_solve_stats[2] = g_block_solve_stats[11] = K;
        return 0;
    }
    block_bm_check_len(block_terms(o.n, b));
    o.views(!trans, trans != 0); // x A = b is A^T x = b
    block_wied_run(trans ? *o.tr : *o.fwd, o.F, b, K, B, ldb, seed, tries, X, ldx, status);
    return 0;
}

} // namespace

extern "C" {

// ---- block Horner and the block Wiedemann solve (block_horner.hpp; engine extension) ----
SPASM_API int spasm_amd_block_poly_apply(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,
                                         spasm_ZZp *X, i64 ldx)
{
    return abi_call("spasm_amd_block_poly_apply", -1, [&] {
        block_solve_stats_reset();
        block_poly_check(op, trans, b, K, D, coef, V, ldv, X, ldx);
        const size_t n = (size_t)op->A.n, kk = (size_t)K, wb = (size_t)b;
        if (n == 0) return 0;
        DeviceGuard g(op);
        hipStream_t s = nullptr;
        DevBuf<int> dV, dX;
        dV.alloc(n * wb);
        dX.alloc(n * kk);
        HIPCHK(hipMemcpy2DAsync(dV.p, wb * sizeof(int), V, (size_t)ldv * sizeof(int), wb * sizeof(int), n, hipMemcpyHostToDevice, s));
        const int launches = block_poly_apply_dev(op, trans, b, K, D, coef, dV.p, b, dX.p, K, s);
        std::vector<int> out(n * kk);
        HIPCHK(hipMemcpyAsync(out.data(), dX.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        block_poly_stats((i64)n, b, K, D, launches);
        for (size_t r = 0; r < n; r++) memcpy(X + (i64)r * ldx, out.data() + r * kk, kk * sizeof(int));
        return 0;
    });
}

SPASM_API int spasm_amd_block_poly_apply_dev(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,
                                             spasm_ZZp *X, i64 ldx, void *stream)
{
    return abi_call("spasm_amd_block_poly_apply_dev", -1, [&] {
        block_solve_stats_reset();
        block_poly_check(op, trans, b, K, D, coef, V, ldv, X, ldx);
        if (op->A.n == 0) return 0;
        DeviceGuard g(op);
        const int launches = block_poly_apply_dev(op, trans, b, K, D, coef, V, ldv, X, ldx, (hipStream_t)stream);
        block_poly_stats(op->A.n, b, K, D, launches);
        return 0;
    });
}

SPASM_API int spasm_amd_block_wiedemann_solve(const struct spasm_csr *A, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                              spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_block_wiedemann_solve", -1,
                    [&] { return block_wied_entry(Operand(A, "spasm_amd_block_wiedemann_solve"), trans, b, K, B, ldb, seed, tries, X, ldx, status); });
}

SPASM_API int spasm_amd_spmv_block_wiedemann_solve(spasm_amd_spmv *op, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                                   spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_spmv_block_wiedemann_solve", -1,
                    [&] { return block_wied_entry(Operand(op), trans, b, K, B, ldb, seed, tries, X, ldx, status); });
}

SPASM_API int spasm_amd_dcsr_block_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,
                                                   spasm_ZZp *X, i64 ldx, int *status)
{
    return abi_call("spasm_amd_dcsr_block_wiedemann_solve", -1,
                    [&] { return block_wied_entry(Operand(D), trans, b, K, B, ldb, seed, tries, X, ldx, status); });
}

SPASM_API void spasm_amd_block_solve_stats(i64 *out)
{
    if (out) memcpy(out, g_block_solve_stats, sizeof g_block_solve_stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Kernel bases without fill-in (colechelon.hpp): the reduced column echelon form of a tall dense block, the block sequence of the
// composite operator A^T D2 A, and on top of them verified kernel vectors by block Wiedemann whose basis can be proved complete.
// ------------------------------------------------------------------------------------------------
#include "colechelon.hpp"

namespace {

// n, m, b, want, tries used, products with A, those of the sequences, of Horner, of the check, of the certification, launches,
// candidates formed, accepted, dropped as dependent, found, device us of the sequences, of Berlekamp-Massey, of Horner + check, of
// the echelon form
constexpr int WKER_NSTATS = 19;
thread_local i64 g_wker_stats[WKER_NSTATS] = {0};

void wker_stats_reset() { memset(g_wker_stats, 0, sizeof g_wker_stats); }

struct CeWork {
    DevBuf<int> piv, mult;
};

// The reduced column echelon form of the rows x K block X on the device (0 < K <= 64, 0 < rows < 2^30), in place: 3 K launches
// enqueued on s, one read-back of the K pivot rows, one permutation.  hpiv gets the rank pivot rows, ascending.  Returns the rank.
int column_echelon_dev(i64 rows, int K, int *X, i64 ldx, const ZpField &F, CeWork &W, int *hpiv, int *launches, hipStream_t s)
{
    const int hp = (int)F.halfp, mhp = (int)F.mhalfp, kw = spmv_kw(K), cap = step_grid_cap();
    W.piv.ensure(CE_MAXK);
    W.mult.ensure((size_t)CE_MAXK * CE_SLICE);
    HIPCHK(hipMemsetAsync(W.piv.p, 0x7f, (size_t)K * sizeof(int), s));
    const dim3 gfind = step_grid(rows, cap), gelim = step_grid(rows * kw, cap);
    for (int c = 0; c < K; c++) {
        int *mult = W.mult.p + (size_t)c * CE_SLICE;
        hipLaunchKernelGGL(k_ce_find, gfind, dim3(CE_BS), 0, s, (i64d)rows, c, F, hp, mhp, X, (i64d)ldx, W.piv.p);
        hipLaunchKernelGGL(k_ce_pivot, dim3(1), dim3(64), 0, s, K, c, F, hp, mhp, X, (i64d)ldx, W.piv.p, mult);
        hipLaunchKernelGGL(k_ce_elim, gelim, dim3(CE_BS), 0, s, (i64d)rows, K, kw, c, F, hp, mhp, X, (i64d)ldx, mult);
    }
    HIPCHK(hipGetLastError());
    int piv[CE_MAXK];
    HIPCHK(hipMemcpyAsync(piv, W.piv.p, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<std::pair<int, int>> order;
    for (int c = 0; c < K; c++)
        if (piv[c] != CE_NONE) order.push_back({piv[c], c});
    std::sort(order.begin(), order.end());
    const int rank = (int)order.size();
    CeOrder ord;
    memset(&ord, 0, sizeof ord);
    for (int j = 0; j < rank; j++) {
        ord.src[j] = (unsigned char)order[(size_t)j].second;
        hpiv[j] = order[(size_t)j].first;
    }
    hipLaunchKernelGGL(k_ce_permute, gelim, dim3(CE_BS), 0, s, (i64d)rows, K, kw, rank, ord, F, hp, mhp, X, (i64d)ldx);
    HIPCHK(hipGetLastError());
    if (launches) *launches += 3 * K + 1;
    return rank;
}

void dense_column_echelon(i64 rows, int K, spasm_ZZp *X, i64 ldx, i64 prime, int *rank, int *pivots)
{
    if (K < 0 || K > CE_MAXK) throw EngineError("K out of range (0 <= K <= 64)");
    if (ldx < K) throw EngineError("ldx < K");
    if (rows < 0 || rows >= ((i64)1 << 30)) throw EngineError("rows out of range (0 <= rows < 2^30)");
    check_prime(prime);
    if (!rank || (K > 0 && !pivots) || (rows > 0 && K > 0 && !X)) throw EngineError("NULL array");
    if (rows == 0 || K == 0) {
        *rank = 0;
        return;
    }
    require_device();
    DeviceGuard g;
    const ZpField F = zp_field_make(prime);
    hipStream_t s = nullptr;
    const size_t kk = (size_t)K, n = (size_t)rows;
    DevBuf<int> dX;
    CeWork W;
    dX.alloc(n * kk);
    HIPCHK(hipMemcpy2DAsync(dX.p, kk * sizeof(int), X, (size_t)ldx * sizeof(int), kk * sizeof(int), n, hipMemcpyHostToDevice, s));
    int hpiv[CE_MAXK], launches = 0;
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    const int r = column_echelon_dev(rows, K, dX.p, K, F, W, hpiv, &launches, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> out(n * kk);
    HIPCHK(hipMemcpyAsync(out.data(), dX.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    g_wker_stats[10] = launches;
    g_wker_stats[14] = r;
    g_wker_stats[18] = (i64)(ev.ms(0, 1) * 1000.0); // the K columns, the read-back of the pivot rows and the permutation
    for (size_t i = 0; i < n; i++) memcpy(X + (i64)i * ldx, out.data() + i * kk, kk * sizeof(int));
    memcpy(pivots, hpiv, (size_t)r * sizeof(int));
    *rank = r;
}

// Y <- d * (A X) on device arrays (K columns, Y of leading dimension spmv_kw(K)): one launch set with DiagEpi and no projection
int diag_step_run(const SpmvView &V, const ZpField &F, int K, const int *d, const int *X, i64 ldx, int *Y, hipStream_t s)
{
    const int kw = spmv_kw(K), cap = step_grid_cap();
    return dispatch_kw(kw, [&](auto KW) {
        return F.small ? spmv_step_launch<true, KW()>(V, F, K, X, (i64d)ldx, Y, (i64d)KW(), DiagEpi{d, nullptr, 0, nullptr}, cap, s)
                       : spmv_step_launch<false, KW()>(V, F, K, X, (i64d)ldx, Y, (i64d)KW(), DiagEpi{d, nullptr, 0, nullptr}, cap, s);
    });
}

void block_precond_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *dl, const spasm_ZZp *dr, const spasm_ZZp *U, i64 ldu,
                            const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    if (!op) throw EngineError("NULL operator");
    block_width(b);
    if (len < 1 || len >= (1 << 24)) throw EngineError("len out of range (1 <= len < 2^24)");
    if (ldu < b || ldv < b || (trans != 0 && trans != 1)) throw EngineError("bad arguments (trans 0/1, ldu >= b, ldv >= b)");
    // op(A) is n x m: M = diag(d_right) op(A)^T diag(d_left) op(A) is m x m
    const int n = trans ? op->A.m : op->A.n, m = trans ? op->A.n : op->A.m;
    if (!S || (m > 0 && (!U || !V)) || (n > 0 && !dl)) throw EngineError("NULL array");
    const uint64_t p = (uint64_t)op->F.p;
    const size_t kk = (size_t)b, bb = kk * kk, dim = (size_t)m;
    if (n == 0 || m == 0) { // M is zero: S_0 = U^T V on the host, every later term is 0
        memset(S, 0, (size_t)len * bb * sizeof(int));
        for (int r = 0; r < b; r++)
            for (int c = 0; c < b; c++) {
                uint64_t a = 0;
                for (i64 k = 0; k < m; k++) a = (a + hresidue(U[k * ldu + r], p) * hresidue(V[k * ldv + c], p)) % p;
                S[(size_t)r * kk + c] = hbalanced(a, p);
            }
        return;
    }
    DeviceGuard g(op);
    op->build_transpose();
    hipStream_t s = nullptr;
    DevBuf<int> dU, dV, dS, ddl, ddr;
    KrylovWork W;
    dU.alloc(dim * kk);
    dV.alloc(dim * kk);
    dS.alloc((size_t)len * bb);
    ddl.alloc((size_t)n);
    HIPCHK(hipMemcpy2DAsync(dU.p, kk * sizeof(int), U, (size_t)ldu * sizeof(int), kk * sizeof(int), dim, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpy2DAsync(dV.p, kk * sizeof(int), V, (size_t)ldv * sizeof(int), kk * sizeof(int), dim, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ddl.p, dl, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if (dr) {
        ddr.alloc(dim);
        HIPCHK(hipMemcpyAsync(ddr.p, dr, dim * sizeof(int), hipMemcpyHostToDevice, s));
    }
    SpgEvents ev;
    HIPCHK(hipEventRecord(ev.e[0], s));
    SeqOperator sq{trans ? &op->tr : &op->fwd, trans ? &op->fwd : &op->tr, ddl.p, dr ? ddr.p : nullptr};
    sq.block = true;
    const int launches = sequence_run(sq, op->F, b, len, dU.p, b, dV.p, b, W, dS.p, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    std::vector<int> out((size_t)len * bb);
    HIPCHK(hipMemcpyAsync(out.data(), dS.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    i64 *st = g_wker_stats;
    st[0] = n;
    st[1] = m;
    st[2] = b;
    st[5] = st[6] = (i64)(len - 1) * 2;
    st[10] = launches;
    st[15] = (i64)(ev.ms(0, 1) * 1000.0);
    memcpy(S, out.data(), out.size() * sizeof(int));
}

void wker_check(int trans, int b, int want, int tries, const void *N, i64 ldn, const int *found, const int *pivots, const int *complete, int dim)
{
    block_width(b);
    if (trans != 0 && trans != 1) throw EngineError("trans must be 0 or 1");
    if (want < 0 || want > CE_MAXK) throw EngineError("want out of range (0 <= want <= 64)");
    if (ldn < want) throw EngineError("ldn < want");
    if (tries < 1) throw EngineError("tries < 1");
    if (!found || !complete || (want > 0 && !pivots) || (want > 0 && dim > 0 && !N)) throw EngineError("NULL array");
    if (dim >= (1 << 24)) throw EngineError("Wiedemann kernel limited to dim < 2^24");
}

// The kernel of B = op(A) behind the three entries: Fw and Tr are the views of B (nr x dim) and of its transpose, nr > 0, dim > 0,
// 0 <= want <= 64; the arguments have been checked.  Per try: D2, U and Y of the seed, V = M Y with M = B^T D2 B, the block sequence
// of M on U, V, the left generator F of its transposed terms, the candidates W = sum_s M^s Y F_s^T by one composite block Horner
// pass, the residual B W with its counts, and the echelon form of the basis with the accepted columns.  The basis stays on the
// device; nothing is written to the caller's arrays before every try has run.
void wker_run(const SpmvView &Fw, const SpmvView &Tr, const ZpField &F, int b, int want, uint64_t seed, int tries, int certify, spasm_ZZp *N, i64 ldn,
              int *found, int *pivots, int *complete)
{
    const int nr = Fw.rows, dim = Fw.cols, len = block_terms(dim, b);
    const uint64_t p = (uint64_t)F.p;
    block_bm_check_len(len);
    i64 *st = g_wker_stats;
    hipStream_t s = nullptr;
    // the lower bound of the rank first: a full-rank matrix is decided without a try
    i64 target = -1; // dim - r once r is known
    if (certify) {
        precond_stats_reset(); // spasm_amd_precond_stats describes the certification run
        i64 r = 0;
        int certain = 0;
        precond_rank_run(Fw, Tr, F, 8, seed, tries, 0, &r, &certain);
        st[9] = g_precond_stats[4];
        st[10] += g_precond_stats[5];
        target = (i64)dim - r;
    }
    const size_t db = (size_t)dim * b, bb = (size_t)b * b;
    std::vector<int> hu(db), hy(db), diag((size_t)nr), hdeg((size_t)b + 1), hcoef, tab;
    std::vector<long long> hcnt((size_t)2 * b);
    DevBuf<int> dU, dY, dV, dl, dS, dSt, d_coef, d_small, dW, dR, dT, dZ, dN;
    DevBuf<long long> dcnt;
    KrylovWork W;
    BlockBmWork BW;
    CeWork CW;
    SpgEvents ev, evh;
    dU.alloc(db);
    dY.alloc(db);
    dV.alloc(db);
    dl.alloc((size_t)nr);
    dS.alloc((size_t)len * bb);
    dSt.alloc((size_t)len * bb);
    d_coef.alloc(((size_t)len + 1) * bb);
    d_small.alloc((size_t)b + 1);
    dW.alloc(db);
    dR.alloc((size_t)nr * b);
    dZ.alloc(std::max(db, (size_t)nr * b));
    W.mid.ensure((size_t)nr * b); // the intermediate of V = M Y is that of the composite Horner steps
    dN.alloc((size_t)dim * CE_MAXK);
    dcnt.alloc((size_t)2 * b);
    dZ.zero(s);
    int have = 0;
    int hpiv[CE_MAXK];
    bool ech_pending = false;
    auto echelon_time = [&] { // after a wait on the stream
        if (ech_pending) st[18] += (i64)(evh.ms(2, 3) * 1000.0);
        ech_pending = false;
    };
    for (int t = 0; t < tries && have < want && have != target; t++) {
        const uint64_t sd = seed + (uint64_t)t;
        precond_diagonal(nr, sd, 0, F.p, diag.data());
        minpoly_vectors(dim, b, sd, F.p, hu.data(), hy.data());
        HIPCHK(hipMemcpyAsync(dU.p, hu.data(), db * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dY.p, hy.data(), db * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dl.p, diag.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev.e[0], s));
        // V = M Y: fwd with the diagonal, then the plain product by tr (a Horner step with the coefficient 0)
        int launches = diag_step_run(Fw, F, b, dl.p, dY.p, b, W.mid.p, s);
        launches += horner_run(Tr, F, b, 1, dZ.p, dZ.p, b, W.mid.p, b, dV.p, b, W, nullptr, s);
        SeqOperator sq{&Fw, &Tr, dl.p, nullptr};
        sq.block = true;
        launches += sequence_run(sq, F, b, len, dU.p, b, dV.p, b, W, dS.p, s);
        HIPCHK(hipEventRecord(ev.e[1], s));
        const i64 total = (i64)len * (i64)bb;
        hipLaunchKernelGGL(k_block_transpose_terms, dim3(cdiv(total, 256)), dim3(256), 0, s, (i64d)total, b, dS.p, dSt.p);
        HIPCHK(hipGetLastError());
        launches += 1 + block_bm_device(F, b, len, dSt.p, BW, d_coef.p, d_small.p, d_small.p + b, s);
        HIPCHK(hipEventRecord(ev.e[2], s));
        HIPCHK(hipMemcpyAsync(hdeg.data(), d_small.p, hdeg.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        echelon_time();
        const int D = hdeg[(size_t)b];
        hcoef.resize(((size_t)D + 1) * bb);
        HIPCHK(hipMemcpy(hcoef.data(), d_coef.p, hcoef.size() * sizeof(int), hipMemcpyDeviceToHost));
        st[4] = t + 1;
        st[6] += (i64)len * 2;
        st[15] += (i64)(ev.ms(0, 1) * 1000.0);
        st[16] += (i64)(ev.ms(1, 2) * 1000.0);
        // slice i of the table is C_{D - i}, C_s[c][j] = F_s[j][c]: column j of W is the relation of row j of the generator
        tab.assign(((size_t)D + 1) * bb, 0);
        for (int i = 0; i <= D; i++) {
            const int *Fs = hcoef.data() + (size_t)(D - i) * bb;
            for (int c = 0; c < b; c++)
                for (int j = 0; j < b; j++) tab[((size_t)i * b + c) * b + j] = hbalanced(hresidue(Fs[(size_t)j * b + c], p), p);
        }
        dT.ensure(tab.size());
        HIPCHK(hipMemcpyAsync(dT.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dcnt.p, 0, (size_t)2 * b * sizeof(long long), s));
        HIPCHK(hipEventRecord(evh.e[0], s));
        launches += block_horner_run(sq, F, b, b, D + 1, dT.p, dY.p, b, dW.p, b, W, dcnt.p, s);
        // the certificate: R <- B W with its non-zero counts, against B itself and not against M
        launches += horner_run(Fw, F, b, 1, dZ.p, dZ.p, b, dW.p, b, dR.p, b, W, dcnt.p + b, s);
        HIPCHK(hipEventRecord(evh.e[1], s));
        HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt.p, hcnt.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        st[7] += (i64)D * 2;
        st[8] += 1;
        st[11] += b;
        st[17] += (i64)(evh.ms(0, 1) * 1000.0);
        CeSelect sel;
        memset(&sel, 0, sizeof sel);
        int take = 0;
        for (int j = 0; j < b && have + take < want; j++)
            if (hcnt[(size_t)b + j] == 0 && hcnt[(size_t)j] != 0) sel.c[take++] = j;
        if (take > 0) {
            HIPCHK(hipEventRecord(evh.e[2], s));
            hipLaunchKernelGGL(k_ce_gather_columns, step_grid((i64)dim * take, step_grid_cap()), dim3(CE_BS), 0, s, (i64d)dim, take, sel, dW.p, (i64d)b, dN.p,
                               (i64d)CE_MAXK, have);
            HIPCHK(hipGetLastError());
            int el = 1;
            const int rank = column_echelon_dev(dim, have + take, dN.p, CE_MAXK, F, CW, hpiv, &el, s);
            HIPCHK(hipEventRecord(evh.e[3], s));
            ech_pending = true; // its time is read at the next wait on the stream: the rank is here already
            launches += el;
            st[12] += take;
            st[13] += have + take - rank;
            have = rank;
        }
        st[10] += launches;
    }
    HIPCHK(hipStreamSynchronize(s));
    echelon_time();
    st[5] = st[6] + st[7] + st[8] + st[9];
    st[14] = have;
    if (have > 0) {
        std::vector<int> out((size_t)dim * have);
        HIPCHK(hipMemcpy2D(out.data(), (size_t)have * sizeof(int), dN.p, (size_t)CE_MAXK * sizeof(int), (size_t)have * sizeof(int), (size_t)dim,
                           hipMemcpyDeviceToHost));
        for (int r = 0; r < dim; r++) memcpy(N + (i64)r * ldn, out.data() + (size_t)r * have, (size_t)have * sizeof(int));
        memcpy(pivots, hpiv, (size_t)have * sizeof(int));
    }
    *found = have;
    *complete = certify && have == target;
}

int wker_entry(Operand &&o, int trans, int b, int want, uint64_t seed, int tries, int certify, spasm_ZZp *N, i64 ldn, int *found, int *pivots, int *complete)
{
    wker_stats_reset();
    o.check();
    const int nr = trans ? o.m : o.n, dim = trans ? o.n : o.m;
    wker_check(trans, b, want, tries, N, ldn, found, pivots, complete, dim);
    i64 *st = g_wker_stats;
    st[0] = o.n;
    st[1] = o.m;
    st[2] = b;
    st[3] = want;
    if (dim == 0) {
        *found = 0;
        *complete = 1;
        return 0;
    }
    if (nr == 0) { // no equation: the unit vectors, as many as are wanted
        const int have = std::min(want, dim);
        for (int r = 0; r < dim && have > 0; r++)
            for (int c = 0; c < have; c++) N[(i64)r * ldn + c] = r == c;
        for (int c = 0; c < have; c++) pivots[c] = c;
        *found = have;
        *complete = certify && have == dim;
        st[14] = have;
        return 0;
    }
    if (o.n >= (1 << 24) || o.m >= (1 << 24)) throw EngineError("Wiedemann kernel limited to dim < 2^24");
    block_bm_check_len(block_terms(dim, b));
    o.views(true, true);
    wker_run(trans ? *o.tr : *o.fwd, trans ? *o.fwd : *o.tr, o.F, b, want, seed, tries, certify, N, ldn, found, pivots, complete);
    return 0;
}

} // namespace

extern "C" {

// ---- kernel bases without fill-in (colechelon.hpp; engine extension) ----
SPASM_API int spasm_amd_dense_column_echelon(i64 rows, int K, spasm_ZZp *X, i64 ldx, i64 prime, int *rank, int *pivots)
{
    return abi_call("spasm_amd_dense_column_echelon", -1, [&] {
        wker_stats_reset();
        dense_column_echelon(rows, K, X, ldx, prime, rank, pivots);
        return 0;
    });
}

SPASM_API int spasm_amd_block_precond_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *d_right,
                                               const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S)
{
    return abi_call("spasm_amd_block_precond_sequence", -1, [&] {
        wker_stats_reset();
        block_precond_sequence(op, trans, b, len, d_left, d_right, U, ldu, V, ldv, S);
        return 0;
    });
}

SPASM_API int spasm_amd_wiedemann_kernel(const struct spasm_csr *A, int trans, int b, int want, uint64_t seed, int tries, int certify, spasm_ZZp *N, i64 ldn,
                                         int *found, int *pivots, int *complete)
{
    return abi_call("spasm_amd_wiedemann_kernel", -1, [&] {
        return wker_entry(Operand(A, "spasm_amd_wiedemann_kernel"), trans, b, want, seed, tries, certify, N, ldn, found, pivots, complete);
    });
}

SPASM_API int spasm_amd_spmv_wiedemann_kernel(spasm_amd_spmv *op, int trans, int b, int want, uint64_t seed, int tries, int certify, spasm_ZZp *N, i64 ldn,
                                              int *found, int *pivots, int *complete)
{
    return abi_call("spasm_amd_spmv_wiedemann_kernel", -1,
                    [&] { return wker_entry(Operand(op), trans, b, want, seed, tries, certify, N, ldn, found, pivots, complete); });
}

SPASM_API int spasm_amd_dcsr_wiedemann_kernel(const spasm_amd_dcsr *D, int trans, int b, int want, uint64_t seed, int tries, int certify, spasm_ZZp *N,
                                              i64 ldn, int *found, int *pivots, int *complete)
{
    return abi_call("spasm_amd_dcsr_wiedemann_kernel", -1,
                    [&] { return wker_entry(Operand(D), trans, b, want, seed, tries, certify, N, ldn, found, pivots, complete); });
}

SPASM_API void spasm_amd_wiedemann_kernel_stats(i64 *out)
{
    if (out) memcpy(out, g_wker_stats, sizeof g_wker_stats);
}

} // extern "C"
