// spk_internal.hpp -- private declarations shared by the libspk.so sources.
//
// Layering (MI355X-first, not PETSc's):
//   spk_api.cpp      C ABI entry points, argument checks, error strings
//   spk_solver.cpp   the products, PCApply and the device-resident FGMRES: the host only ENQUEUES a
//                    restart cycle; Hessenberg/Givens/convergence live on the device
//   spk_operator.cpp KSPSetOperators / KSPSetUp, the device half: uploads, blocked copies, dictionary rounds,
//                    collectives of the halo plan, Schur diagonal
//   spk_host.hpp/.cpp the host-pure half of the set-up (no HIP; compiles without ROCm): errors, host arrays, row-slab
//                    split, ghost numbering, halo plan, dictionary field layout, windows and transpose of B
//   spk_k_*.hip      hand-written gfx950 kernels (HBM-bound, FP64, no MFMA): spmv (+ set-up, FP32 sweeps), vec (MDot,
//                    MAXPY, PC pieces), krylov (scalar work, head kernels), iter (fused iteration), comm (peer-store
//                    launches); spk_device.hpp = the device helpers they share
//   spk_comm.cpp     collectives: peer-store windows over xGMI on top of RCCL (one process per
//                    GPU); host-callback and in-process backends for 1-GPU rehearsals
//   spk_partition.cpp C entry points of the row-slab partition and split
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include <hip/hip_ext.h>

#include "spk_host.hpp"
#include "spk_amg.hpp"
#include "spk_lanczos_core.hpp"
#include "spk_gs_launch.hpp"

namespace spk {

#define SPK_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            ::spk::fail(SPK_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                           \
    } while (0)

// ---------------------------------------------------------------------------
// device memory
// ---------------------------------------------------------------------------
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; n = o.n;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // allocates `count` (+pad) elements, zero-filled
    void alloc(size_t count, size_t pad = 0)
    {
        release();
        n = count;
        size_t bytes = (count + pad) * sizeof(T);
        if (bytes == 0) bytes = sizeof(T);
        SPK_HIP(hipMalloc((void **)&p, bytes));
        SPK_HIP(hipMemset(p, 0, bytes));
    }
    // allocates without clearing (the caller writes every element it reads; only the pad is zeroed)
    void alloc_raw(size_t count, size_t pad = 0)
    {
        release();
        n = count;
        size_t bytes = (count + pad) * sizeof(T);
        if (bytes == 0) bytes = sizeof(T);
        SPK_HIP(hipMalloc((void **)&p, bytes));
        if (pad) SPK_HIP(hipMemset(p + count, 0, pad * sizeof(T)));
    }
    void upload(const T *h, size_t count, size_t pad = 0)
    {
        alloc(count, pad);
        if (count) SPK_HIP(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
    }
};

// CSR block on the device, prepared for the row-tiled stream kernel.
struct CsrDev {
    int32_t nrows = 0, ncols = 0;
    int64_t nnz = 0;
    DevBuf<int32_t> rowptr, colidx;
    DevBuf<double> val;
    // stream tiling: tile t covers rows [tile_row[t], tile_row[t+1])
    DevBuf<int32_t> tile_row;
    int32_t ntiles = 0;
};

// 2x2-blocked copy of the diagonal part of A (dof-2 DMDA matrices: rows 2k, 2k+1 share
// their column pattern, columns come in pairs 2c, 2c+1 -- PETSc exploits the same fact
// with BAIJ / inodes).  One int32 block column + 4 values per block: 36 B per 4 stored
// non-zeros instead of 48.  Values are kept as two planes so every load is 16 B/lane.
struct BcsrDev {
    int32_t nbrows = 0;
    int64_t nblocks = 0;
    DevBuf<int32_t> browptr, bcol;
    DevBuf<double> vtop, vbot;  // (a00,a01) and (a10,a11) per block
    DevBuf<float> vtop32, vbot32;  // the same in single precision, for the FP32 inner sweeps (spk_pc_setup with sweeps)
    DevBuf<int32_t> tile_brow;
    int32_t ntiles = 0;
    bool ok = false;
};

// 3x3-blocked copy (dof-3 grids): one block column index per nine values; plane k (stride ldp) = entry (k / 3, k % 3) of
// every block.  v32: the same planes in single precision for the FP32 inner sweeps (spk_pc_setup with inner sweeps).
struct Bcsr3Dev {
    int32_t nbrows = 0;
    int64_t nblocks = 0, ldp = 0;
    DevBuf<int32_t> browptr, bcol, tile_brow;
    DevBuf<double> v;
    DevBuf<float> v32;
    int32_t ntiles = 0;
    bool ok = false;
};

// Row types + deviation codes of a blocked matrix (bs = 2 or 3; spk_k_dict.hip).  The reference assembles the same
// element matrix for every element of a uniform grid (/root/reference/src/Discretization.c:25, :293-332) -- up to the
// rounding of a Jacobian formed from node coordinates (:96-128): the entries of A scatter by a few hundred ulps around a
// handful of ideal values.  So A has a few dozen block CLASSES (blocks equal up to that noise) and a few dozen ROW TYPES
// (sequences of (column offset, class) along a block row).  Stored per block row: one 16-bit type; per stored value: a
// two's-complement bit field k of the width its class entry needs with  value = base[class][entry] + k 2^g[class][entry]
// exactly, a block's fields packed into one (2x2) / two (3x3) 64-bit words.
// The small tables sit in LDS.  A product streams x, y and ~1.8 B per stored non-zero instead of 9 (blocked) / 12
// (CSR) and forms the same products in the same order: bit-identical sums.  Found in the caller's CSR at KSPSetOperators
// (hashing on the device, then EVERY value decoded and compared bit by bit); a matrix that does not fit (too many classes
// or types, a row beyond kDictMaxK blocks, deviations that are not small multiples of one power of two or do not fit the
// words, tables beyond the LDS budget) keeps the plain blocked layout.
struct DictDev {
    int bs = 0;
    int32_t nbrows = 0, ntype = 0, nclass = 0, kmax = 0;
    int64_t nblocks = 0;
    DevBuf<uint16_t> tid;          // type of every block row
    DevBuf<int32_t> tab;           // [ntype] lengths (padded to an even count), then ntype x kmax x {column offset, class}
    DevBuf<double> cls;            // (nclass + 1) x bs*bs x {base, 2^g}: the last one is the NULL class (base 0, scale 0: decodes to +0)
    DevBuf<int32_t> fld;           // (nclass + 1) x bs*bs bit fields of the codes (spk_dict.hpp: dict_field / dict_field2)
    DevBuf<double> zpad;           // zeros: the x a position beyond a row's length gathers in the pipelined product
    DevBuf<unsigned char> codes;   // bs = 2: one 64-bit word per block, positions 2p / 2p+1 side by side in plane p (16 B per block
                                   // row; an odd last position: 8 B); bs = 3: two words per block, plane k = position k
    int64_t plane_off[kDictMaxK] = {};
    int64_t code_bytes = 0;        // bytes of codes a product reads (the planes without their padding rows)
    int32_t lds_bytes = 0;         // tables as laid out in LDS
    // 2x2: every class has the SAME field layout (the widest need of any class per entry still fits: entries 0, 1 in the
    // low half of the word, 2, 3 in the high half): the product kernel extracts without reading the field table
    bool uniform = false;
    int32_t uw[4] = {1, 1, 1, 1};
    bool straddle = false;         // 2x2: some class has a field across the halves of its word (spk_dict.hpp)
    int uniform3 = 0;              // 3x3: one field layout for all classes; 1..3 = which entries sit in the second word
    int32_t u3l[9] = {}, u3r[9] = {};   // its shifts (dict_field3u)
    bool ok = false;
};

// Short-and-wide block (B: m rows x n_local cols) cut into column windows so
// that x is streamed once for all m rows.
struct WideDev {
    int32_t m = 0, ncols = 0, nwin = 0, win = 0;
    int64_t nnz = 0;
    DevBuf<int32_t> colidx;  // nnz, rows concatenated, ascending in a row
    DevBuf<double> val;
    DevBuf<int32_t> winptr;  // (nwin+1) x m : start of window w in row r
};

// ---------------------------------------------------------------------------
// peer-store windows (one-shot collectives over xGMI, spk_comm.cpp / spk_device.hpp, spk_k_comm.hip)
// ---------------------------------------------------------------------------
namespace k {
struct SendRanges;
constexpr int kPeerMax = 8;        // ranks of one node
constexpr int kArSlots = 4;        // all-reduce slots in flight (a rank is never more than one ahead)
constexpr int kArGranules = 128;   // 8-byte {seq, half} granules per rank and slot = 64 doubles
// One-shot all-reduce: every rank stores its values as tagged granules into EVERY rank's window
// (win[p] = rank p's window as mapped here) and sums what arrived in its own, in rank order.
// Device-side diagnostics of the peer-store backend (spk_comm_get_info): accumulated by ONE lane per
// collective / waiting workgroup.  stats[2k] = 100 MHz ticks between "my stores are issued" and "every
// rank's contribution has arrived", stats[2k+1] = number of such waits; k = kStatArDots (all-reduce in
// the finish of MDot), kStatArNorm (the one after MAXPY), kStatArOther (stand-alone launches),
// kStatHalo (ghost rows).
enum { kStatArDots = 0, kStatArNorm = 1, kStatArOther = 2, kStatHalo = 3, kStatCount = 8 };
struct PeerAR {
    int P, me;                     // P == 0: off
    uint32_t seq, timeout_ms;
    unsigned long long *win[kPeerMax];
    int32_t *err;                  // set to 1 by a poll that timed out
    unsigned long long *stats;     // nullptr: no accounting
    int kind;                      // kStatAr*
};
// Halo exchange in the same style: my segment for peer i goes to remote[i] (the place in that
// rank's staging window where it expects my rows), what I expect arrives in `mine`.
struct PeerHalo {
    int npeers;                    // 0: off
    uint32_t seq, timeout_ms;
    unsigned long long *remote[4];
    const unsigned long long *mine;
    int64_t send_off[5], recv_off[5];
    int32_t *err;
    unsigned long long *stats;
};
// The same exchange for segments that are bandwidth-bound (a node PLANE of a 3-D slab): the payload
// goes as plain doubles in chunks of kBulkChunk, each followed -- after a system-scope release -- by
// ONE flag store; the receiver waits on the flag of a chunk, then copies it out of its staging.
constexpr int kBulkChunk = 2048;
struct PeerBulk {
    int npeers;
    uint32_t seq, timeout_ms;
    double *rdata[4];                 // where my segment for peer i starts in its staging
    unsigned long long *rflag[4];     // that staging's flag of element 0 of my segment (one flag per chunk, at its first element)
    const double *mdata;              // my staging (this parity)
    const unsigned long long *mflag;
    int64_t send_off[5], recv_off[5];
    int32_t send_chunk0[5], recv_chunk0[5];  // prefix sums of the chunk counts
    int32_t *err;
    unsigned long long *stats;
};
}  // namespace k

// ---------------------------------------------------------------------------
// collectives
// ---------------------------------------------------------------------------
struct HaloPlan;
class Comm {
public:
    virtual ~Comm() {}
    virtual int rank() const { return 0; }
    virtual int size() const { return 1; }
    // called once the halo plan of the (0,0) block is known (collective)
    virtual void setup_halo(int32_t n_ghost, const std::vector<int> &peers, const std::vector<int64_t> &send_off,
                            const std::vector<int64_t> &recv_off)
    { (void)n_ghost; (void)peers; (void)send_off; (void)recv_off; }
    // all-reduce performed INSIDE the reducing kernel's finish (peer-store backend): returns the
    // window set for the next all-reduce of `count` values, or P == 0 when the backend cannot
    // (the caller then calls allreduce_sum after the kernel)
    virtual k::PeerAR fused_allreduce(int count, int kind = k::kStatArOther) { (void)count; (void)kind; return k::PeerAR{}; }
    // what the first multi-GPU run needs to be diagnosable from its own output (spk_comm_get_info): a plain backend
    // reports how many all-reduces / halo exchanges it carried; the peer-store wrapper overrides with its own split
    virtual void info(spk_comm_info *out)
    {
        out->n_allreduce_inner = n_ar_calls_;
        out->n_halo_inner = n_ex_calls_;
    }
    // halo exchange performed INSIDE the kernel that produces the vector (contiguous send ranges
    // only): fills the peer fields of sr for the next exchange and returns true, or returns false
    // (the caller then calls exchange())
    virtual bool fused_halo(k::SendRanges &sr, double *xghost) { (void)sr; (void)xghost; return false; }
    // The resident restart-cycle kernel runs a whole cycle's collectives inside ONE launch: n_ar all-reduces and n_halo
    // halo exchanges with consecutive sequence numbers.  Fills the window set of the first all-reduce and the send ranges
    // of the first two exchanges (the two staging parities; sr0 / sr1 come in as copies of the context's ranges) and
    // reserves the numbers; false when this backend cannot (the caller keeps the launch-by-launch form)
    virtual bool resident_plan(int n_ar, int n_halo, k::PeerAR &ar, k::SendRanges &sr0, k::SendRanges &sr1, double *xghost)
    { (void)n_ar; (void)n_halo; (void)ar; (void)sr0; (void)sr1; (void)xghost; return false; }
    // throws SPK_ERR_COMM when a device-side wait of this backend has timed out (call after a sync)
    virtual void check(hipStream_t s) { (void)s; }
    virtual const char *name() const { return "self"; }
    // true when the Krylov all-reduces ride in the finish of the reducing kernels (fused_allreduce returns windows)
    virtual bool fuses() const { return false; }
    // device address of the backend's sticky error word (nullptr: none): the solver reads it with its own per-cycle
    // state copy and calls check() only when it is set
    virtual const int32_t *error_dev() const { return nullptr; }
    // in-place sum over ranks of `count` doubles in device memory, stream-ordered
    virtual void allreduce_sum(double *dev, int count, hipStream_t s) { (void)dev; (void)count; (void)s; }
    // exchange of packed halo segments: sendbuf[send_off[p]..] -> peer p,
    // peer p's segment lands in recvbuf[recv_off[p]..]
    virtual void exchange(const double *sendbuf, const std::vector<int> &peers,
                          const std::vector<int64_t> &send_off, double *recvbuf,
                          const std::vector<int64_t> &recv_off, hipStream_t s)
    { (void)sendbuf; (void)peers; (void)send_off; (void)recvbuf; (void)recv_off; (void)s; }
    // host-side exchange of small setup data (sizes, index lists)
    virtual void host_allgather(const void *in, void *out, size_t bytes_each) { memcpy_self(in, out, bytes_each); }
    virtual void host_allgatherv(const void *in, size_t bytes_in, std::vector<std::vector<char>> &out)
    {
        out.assign(1, std::vector<char>((const char *)in, (const char *)in + bytes_in));
    }
protected:
    static void memcpy_self(const void *in, void *out, size_t b);
    int64_t n_ar_calls_ = 0, n_ex_calls_ = 0;
};
Comm *make_self_comm();
Comm *make_rccl_comm(int rank, int nranks, const void *id128, int device);
Comm *make_local_comm(spk_local_group *grp, int rank);
Comm *make_host_comm(int rank, int nranks, const spk_host_comm &cb);
// wraps `inner` (kept for set-up traffic and as the fallback) with the peer-store backend when every
// rank can map every other rank's window; returns `inner` itself otherwise (*why says why)
Comm *make_peer_comm(Comm *inner, int device, std::string *why);

// ---------------------------------------------------------------------------
// Krylov state that lives in device memory (one per context)
// ---------------------------------------------------------------------------
struct KrylovState {
    int32_t its, reason, done, loc_done;
    int32_t max_it, restart, hapend, skip_refine;
    // what the kernels of an ITERATION are gated by: set together with `done`, and alone when the
    // rest of the restart cycle is to be skipped (single-reduction mode: a convergence seen by the
    // recurrence is only tentative and is confirmed on the true residual of the restart)
    int32_t skip_iter, guess_nonzero;
    double rnorm, rnorm0, ttol, abstol, dtol, bnorm;
    double rtol;    // -ksp_rtol: ttol is fixed at iteration 0 (KSPConvergedDefault)
    double cnorm0;  // the norm the relative and the divergence tests refer to (||b|| or the initial residual)
    double inv_tt;  // 1/||w|| of the last orthogonalised vector (or 1/||r||)
    double tt;
    double beta;    // the residual norm this restart cycle started from (the early-restart test of an FP32 basis)
};

// What the states of MINRES and pipelined CG share: the convergence words of KrylovState (converged_default) and the
// start / confirmation bookkeeping of the shared frame (spk_device.hpp)
struct SolverHead {
    KrylovState ks;
    int32_t norm;     // SPK_NORM_*
    int32_t tent;     // ks.reason was set by the recurrence alone: confirmed on b - K x
    int32_t starts;   // recurrence (re)starts
    int32_t started;  // rnorm0 / ttol fixed
};

// MINRES state (spk_minres): the shared head and the scalar recurrence
struct MinresState : SolverHead {
    int32_t first;    // first iteration of a recurrence (v_0 = 0)
    int32_t pend;     // reason to end with once the pending update is applied (happy breakdown)
    double gam, gam_prev, delta, eta, c0, c1, s0, s1;
    double vz_ig, vz_dg, vz_gg;                 // v_{j+1} = ig p - dg v_j - gg v_{j-1}   (p = K z_j, z_j not scaled)
    double wx_ig, wx_a2, wx_a3, wx_ia1, wx_cx;  // w_{j+1} = (ig z_j - a3 w_{j-1} - a2 w_j) ia1 ;  x += cx w_{j+1}
};

// pipelined CG state (spk_pipecg): the shared head and the scalar recurrence
struct PipecgState : SolverHead {
    int32_t first;    // the next pass is the first of a recurrence (z = n, s = w, p = u, q = m)
    int32_t rr_idle;  // pipecgrr: 0 while a replacement asked for by the gap check is pending (the gate of its launches)
    double alpha, beta;   // step lengths of the next pass
    double gamma;         // <r, u> of the pass before it (gamma_old)
    double alpha_old, gamma_old;   // alpha and gamma before the last iteration step (pipecgrr's replacement step)
    double tau;                    // pipecgrr: replace when ||(b - K x) - r|| > tau ||r||
    int32_t replacements;          // pipecgrr: residual replacements so far
    int32_t rr_above;              // pipecgrr: the last gap check of this recurrence found the gap above tau ||r||
};

// Workspace of MINRES or pipelined CG (one each in the context, allocated on first use; nothing of FGMRES's or of the
// other solver's is touched): the solver's vectors, the reduced sums, the residual history, the state and its read-back
struct SolverWork {
    DevBuf<double> vec;                    // the solver's vectors, stride ld, zero-filled: the pad entries stay zero
    DevBuf<double> out, hist;              // reduced sums, residual history
    DevBuf<unsigned char> state;           // MinresState / PipecgState
    void *pin = nullptr;                   // pinned landing place of the state read-back (two slots)
    hipEvent_t ev[2] = {nullptr, nullptr}; // behind the copy into each slot
    void ensure(int64_t ld, int nvec, int32_t hist_cap, size_t state_bytes);
    ~SolverWork();
};

// kernel launch wrappers (spk_k_*.hip)
namespace k {
constexpr int kMaxNv = 64;       // max vectors in one mdot/maxpy launch; restart <= 62 takes the fused kernels
constexpr int kBigNv = 1024;     // restart lengths up to kBigNv - 2 run Gram-Schmidt in chunks of <= 40 vectors
constexpr int kPartialLd = 64;   // leading dimension of block partials
constexpr int kMaxBlocks = 2048; // cap for grid-stride vector kernels
constexpr int kBTile = 512;      // 2x2 blocks per tile of the blocked SpMV kernels

void build_tiles(const int32_t *rowptr, int32_t nrows, std::vector<int32_t> &tile_row);
// arms the block-partials buffer of the cross-workgroup finish (spk_k_vec.hip)
void arm_partials(double *p, size_t n, hipStream_t s);
// test hook: a reduction with a partial that never arrives (see spk_debug_finish_timeout)
struct Finish;
void finish_probe(const Finish &f, hipStream_t s);
// test hook: the wave sums of na x 512 values by wave_sum and by wave_sum_multi (see spk_debug_wave_sums)
void wave_sums_probe(int na, const double *in, double *out, hipStream_t s);
// test hook: the launch shapes mdot / maxpy pick for n entries and the two knobs they read (see spk_debug_vec_shape)
void vec_shapes_probe(int64_t n, int32_t *out);

// where a reducing kernel leaves its result: block partials (armed with the sentinel of the
// "last block reduces" protocol, spk_device.hpp) and the output slot
struct Finish {
    double *partials;
    double *out;
    PeerAR ar;  // P != 0 (mdot, maxpy only): the finishing workgroup also sums over the ranks
    // sticky execution-error word of the context (bit 0: a partial never arrived within fin_ticks);
    // fgmres / the API calls turn it into SPK_ERR_HIP and re-arm the partials
    int32_t *err = nullptr;
    uint32_t fin_ticks = 400000000u;  // bound of the reducer's wait, 100 MHz ticks (4 s)
};

// off-rank part folded into the SpMV epilogue (rowptr over ALL local rows; nullptr: none)
struct OffDiag {
    const int32_t *rowptr, *colidx;
    const double *val, *xg;
};
// packed halo values written by the producer of a vector instead of a gather launch: up to four
// contiguous row ranges (slab partitions send whole node lines / planes)
struct SendRanges {
    int n;  // 0: none
    int32_t r0[4], len[4], off[4];
    double *buf;
    // peer-store backend (Comm::fused_halo): the rows go as granules straight into the neighbours'
    // staging instead of buf, and extra workgroups at the end of the grid wait for MY ghost rows and
    // unpack them into xghost -- the halo exchange costs no launch of its own
    int peer;  // 0: off
    uint32_t seq, timeout_ms;
    unsigned long long *remote[4];
    const unsigned long long *mine;
    int32_t nrecv;
    double *xghost;
    int32_t *err;
    unsigned long long *stats;
};

// y = A x  (+ Bt-rows * lam when bt != nullptr; y += when accumulate); CSR stream kernel.
// rider: one extra workgroup of the launch runs a pending Givens step beside the row tiles (GivensRider below)
struct GivensRider;
void spmv(const CsrDev &A, const double *x, double *y, const CsrDev *bt, const double *lam,
          const int32_t *done, hipStream_t s, bool accumulate = false, const OffDiag *od = nullptr,
          const GivensRider *rider = nullptr);
// same product from the 2x2-blocked copy (bitwise the same sums: CSR order is kept)
void spmv_bcsr(const BcsrDev &A, const double *x, double *y, const CsrDev *bt, const double *lam,
               const int32_t *done, hipStream_t s, bool accumulate = false, const OffDiag *od = nullptr,
               const GivensRider *rider = nullptr);
void build_btiles(const int32_t *browptr, int32_t nbrows, std::vector<int32_t> &tile_brow);
// ... and from the 3x3-blocked copy (same sums again)
constexpr int kB3Tile = 256;  // blocks per tile: one per thread
void spmv_bcsr3(const Bcsr3Dev &A, const double *x, double *y, const CsrDev *bt, const double *lam,
                const int32_t *done, hipStream_t s, bool accumulate = false, const OffDiag *od = nullptr,
                const GivensRider *rider = nullptr);
void build_b3tiles(const int32_t *browptr, int32_t nbrows, std::vector<int32_t> &tile_brow);
// ... and from row types + deviation codes (spk_k_dict.hip; same sums once more)
constexpr int kDictMaxPat = 1024, kDictMaxBlk = 1024, kDictSlots = 8192, kDictLdsMax = 48 * 1024;
void spmv_dict(const DictDev &A, const double *x, double *y, const CsrDev *bt, const double *lam, const int32_t *done,
               hipStream_t s, bool accumulate = false, const OffDiag *od = nullptr, const GivensRider *rider = nullptr);
void jacobi_sweep_f32_dict(const DictDev &A, const float *d32, float omega, const float *x32, const float *yin, float *yout,
                           const int32_t *done, hipStream_t s);
// set-up passes: classes by hashing (keys/rep: kDictSlots entries, zero / INT32_MAX before the call; slot: the table
// slot of every item; ctl[0] = number of distinct keys, ctl[1] = 1 when there are too many)
void dict_hash_blocks(int bs, const double *v0, const double *v1, int64_t ldp, int64_t nblocks, unsigned long long *keys,
                      int32_t *rep, int32_t *slot, int32_t *ctl, int maxkeys, hipStream_t s);
// cls[(id, e)] = {entry e of block rep_of_id[id], 1}; slot[q] -> class number; gexp / dmax: per (class, entry) the finest
// bit and the largest magnitude of value - base (INT32_MAX / 0 before the call); *bad: a deviation that is not exact
// Measurement (spk_debug_time_products): a product launch takes the kernel's OWN start / stop time stamps into a pair of events
// (hipExtLaunchKernelGGL) when the calling thread has set them -- a_mult around the iteration's product launch
struct LaunchTimer {
    hipEvent_t start = nullptr, stop = nullptr;
};
LaunchTimer &launch_timer();
#define SPK_LAUNCH_PRODUCT(kern, grid, block, lds, stream, ...)                                                                 \
    do {                                                                                                                        \
        const spk::k::LaunchTimer &lt_ = spk::k::launch_timer();                                                                \
        if (lt_.start) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)(lds), stream, lt_.start, lt_.stop, 0, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                                   \
    } while (0)
// spk_k_dict3.hip: the pipelined forms for 3x3 blocks (27-point row types, DictDev::uniform3); false: not applicable
bool spmv_dict3(const DictDev &A, const double *x, double *y, const CsrDev *bt, const double *lam, const int32_t *done, hipStream_t s,
                bool accumulate, const OffDiag *od, const GivensRider *rider);
bool jacobi_sweep_f32_dict3(const DictDev &A, const float *d32, float omega, const float *x32, const float *yin, float *yout,
                            const int32_t *done, hipStream_t s);
bool dict3_pipelined(const DictDev &A);     // the predicate of both
int dict_product_kernel(const DictDev &A);   // 0 plain, 1 pipelined 2x2, 2 pipelined 3x3 (single rank, no off-rank columns)
int dict_chunks_per_wg(const DictDev &A);
void dict_class_stats(int bs, const double *v0, const double *v1, int64_t ldp, int64_t nblocks, const int32_t *rep_of_id, int nid,
                      const int32_t *slot2id, int32_t *slot, double *cls, int32_t *gexp, unsigned long long *dmax, int32_t *bad,
                      hipStream_t s);
void dict_hash_rows(const int32_t *browptr, const int32_t *bcol, const int32_t *blkid, int32_t nbrows, unsigned long long *keys,
                    int32_t *rep, int32_t *slot, int32_t *ctl, int maxkeys, int kmax, hipStream_t s);
void dict_fill_rows(const int32_t *browptr, const int32_t *bcol, const int32_t *blkid, int32_t nbrows, const int32_t *rep_of_id,
                    int nid, int kmax, const int32_t *slot2id, const int32_t *slot, int32_t *tab, uint16_t *tid, int32_t *bad,
                    hipStream_t s);
// writes the code planes of A (tables, plane offsets and widths set), then decodes every value and compares its bits
void dict_encode_verify(const DictDev &A, const int32_t *browptr, const int32_t *bcol, const int32_t *blkid, const double *v0,
                        const double *v1, int64_t ldp, int32_t *bad, hipStream_t s);
void bcsr3_fill(const int32_t *rp, const int32_t *ci, const double *va, int nbr, int32_t *browptr, int32_t *bcol, double *v,
                int64_t ldp, int32_t *fail, hipStream_t s);
void jacobi_sweep_f32_b2(const BcsrDev &A, const float *d32, float omega, const float *x32, const float *yin, float *yout,
                         const int32_t *done, hipStream_t s);
void jacobi_sweep_f32_b3(const Bcsr3Dev &A, const float *d32, float omega, const float *x32, const float *yin, float *yout,
                         const int32_t *done, hipStream_t s);
// KSPSetOperators on the device: count off-rank entries per row, exclusive scan, split, 2x2 blocking
void csr_count_off(const int32_t *rowptr, const int32_t *colidx, int nrows, int64_t lo, int64_t hi, int64_t ncols, int32_t *cnt,
                   int32_t *bad, hipStream_t s);
void exclusive_scan_i32(const int32_t *in, int64_t n, int32_t *out, int32_t *scratch, hipStream_t s);  // out[0..n]; scratch: n/2048 + 2 ints
void csr_split(const int32_t *rowptr, const int32_t *colidx, const double *val, int nrows, int64_t lo, int64_t hi,
               const int32_t *orp, int32_t *d_rowptr, int32_t *d_col, double *d_val, int32_t *o_col, double *o_val, hipStream_t s);
void bcsr_fill(const int32_t *rp, const int32_t *ci, const double *va, int nbr, int32_t *browptr, int32_t *bcol, double *vtop,
               double *vbot, int32_t *fail, hipStream_t s);
// spk_k_assembly.hip: the CSR slab and f (may be null) of node lines [j0, j1) of the mx x my grid, bit for bit the host
// assembler's; kappa: one value per element of the whole grid on the device, or null for ones.  rowptr: 2 mx (j1 - j0) + 1.
// _grid: the workgroups it launches.
void assemble_laplace(int mx, int my, int j0, int j1, const double *kappa, int apply_bc, int32_t *rowptr, int32_t *colidx, double *val,
                      double *f, hipStream_t s);
int64_t assemble_laplace_grid(int mx, int j0, int j1);
// spk_k_assembly3d.hip: the same for the node planes [k0, k1) of the mx x my x mz grid of the 3-D generator (dof 3); kappa: one
// value per hexahedron of the whole grid.  rowptr: 3 mx my (k1 - k0) + 1.
void assemble_laplace3d(int mx, int my, int mz, int k0, int k1, const double *kappa, int apply_bc, int32_t *rowptr, int32_t *colidx,
                        double *val, double *f, hipStream_t s);
int64_t assemble_laplace3d_grid(int mx, int my, int k0, int k1);
void kappa_check(const double *kappa, int64_t ne, int32_t *flag, hipStream_t s);   // flag[0] := 1 for an entry not finite and > 0
// spk_k_constraints.hip: the constraint block of node lines (mz == 0) or planes [u0, u1) of the grid, bit for bit the host
// chain's: B by rows with localised columns (bcol, bval), B^T by rows (trp: local rows + 1, tci, tv) and the window
// pointers ((nwin + 1) x m, m = 4 or 6) for windows of `win` columns.
void assemble_constraints(int mx, int my, int mz, int u0, int u1, int32_t *bcol, double *bval, int32_t *trp, int32_t *tci, double *tv,
                          int32_t win, int32_t nwin, int32_t *winptr, hipStream_t s);
// f.out[r] = B_r . x, r < m
void wide_dot(const WideDev &B, const double *x, const Finish &f, const int32_t *done, hipStream_t s,
              const int32_t *rowmap = nullptr);
// shat[r] = sum_k B_rk^2 dinv[col_k], one wave per CSR row
void schur_diag_rows(const CsrDev &B, const double *dinv, double *shat, hipStream_t s);
// same with x replaced by x .* dinv (the B D x0 step of the Schur PC, no stored D x0)
void wide_dot_jacobi(const WideDev &B, const double *x, const double *dinv, const Finish &f,
                     const int32_t *done, hipStream_t s);
// dense[col] = val*dinv[col] over entries [k0,k1) of B (dinv == nullptr: dense[col] = 0)
void scatter_row(const int32_t *colidx, const double *val, int k0, int k1, const double *dinv,
                 double *dense, hipStream_t s);
// out[i] = sum_r slots[r*ld + i] in rank order (local-group all-reduce)
void sum_slots(const double *slots, int nslots, int ld, int count, double *out, hipStream_t s);
// VecMDot over an FP32 basis (one rank, nv2 <= 8; basis vectors beyond 40 in a launch of their own): V holds floats of stride ldv floats, the
// planes V2 (stride ld2 doubles) and w stay FP64; results as mdot's.  Always the streaming form.
void mdot_f32(const float *V, int64_t ldv, int nv, const double *w, int64_t n, int64_t n_dot, const Finish &f,
              const int32_t *done, hipStream_t s, const double *V2, int64_t ld2, int nv2, int split);
// dst = float(src), n entries (V~_0 of a cycle on an FP32 basis)
void cvt_basis_f32(const double *src, float *dst, int64_t n, const int32_t *done, hipStream_t s);
// f.out[i] = V_i . w for i < nv, then V2_i . w for i < nv2 (second slab, same stride), then w.w
void mdot(const double *V, int64_t ldv, int nv, const double *w, int64_t n, int64_t n_dot,
          const Finish &f, const int32_t *done, hipStream_t s, const double *V2 = nullptr, int nv2 = 0,
          int v2_split = 0);
// single-reduction Gram-Schmidt: scalars derived by workgroup 0 of the MAXPY kernel
struct PythArgs {
    int m;               // < 0: off
    const double *dots;  // [h_0..h_{nv-1}, q_0..q_{m-1}, w.w]  (reduced)
    double *tb;          // (restart+2) x 8: B D v_i per basis vector
    double *nrm_out;     // [||w'||^2, B D w' (m)]
};
// w += sign * sum_i a[i] * V_i ; f.out[0] = ||w_new||^2 over the first n_dot entries
// (f.out == nullptr: no norm)
// with bd != nullptr also f.out[1+r] = sum_i bd[i*MP + r] * w_new[i], i < n_bd (fused Schur path)
void maxpy(const double *V, int64_t ldv, int nv, const int32_t *nv_dev, const double *a,
           double coef_sign, double *w, int64_t n, int64_t n_dot, const Finish &f,
           const int32_t *done, hipStream_t s, const double *bd = nullptr, int64_t ldb = 0, int64_t n_bd = 0, int m = 0,
           double *w1side = nullptr, const PythArgs *pyth = nullptr, int bd_packed = 0);
void build_bd(const CsrDev &Bt, const double *dinv, int m, int64_t ldb, double *bd, hipStream_t s);
// rows 2q, 2q+1 of B D interleaved by parity into one plane each (bd_packed = 1 in the kernels that
// stream them); *bad != 0: the rows do not have that structure
void pack_bd(const double *bd, int64_t ldb, int64_t n, int m, double *bdp, int32_t *bad, hipStream_t s);
// (sa != nullptr: x = sa - sb is formed and stored in the same pass)
void sqnorm_bd(double *x, int64_t n, int64_t n_dot, const double *bd, int64_t ldb, int64_t n_bd, int m,
               double *w1side, const Finish &f, const int32_t *done, hipStream_t s, const double *sa = nullptr,
               const double *sb = nullptr);
// x *= *alpha_dev
void scale_dev(double *x, int64_t n, const double *alpha_dev, const int32_t *done, hipStream_t s);
// y = a*x + b*y with host scalars (b = 0: y = a*x without reading y)
void axpby(double a, const double *x, double b, double *y, int64_t n, const int32_t *done, hipStream_t s);
// f.out[0] = x.x over the first n_dot entries
void sqnorm(const double *x, int64_t n_dot, const Finish &f, const int32_t *done, hipStream_t s);
// x[0..n) = sa - sb and f.out[0] = x.x over the first n_dot entries, one pass
void sqnorm_sub(const double *sa, const double *sb, double *x, int64_t n, int64_t n_dot, const Finish &f, const int32_t *done,
                hipStream_t s);
// gather x[idx[i]] -> out[i]
void gather(const double *x, const int32_t *idx, int64_t n, double *out, const int32_t *done, hipStream_t s);
// peer-store collectives (stand-alone launches; the fused forms live in the reducing kernels)
void peer_allreduce(const PeerAR &a, double *buf, int count, hipStream_t s);
void peer_allreduce_loopback(const PeerAR &a, double *buf, int count, hipStream_t s);  // test hook: workgroup r = rank r
void peer_exchange(const PeerHalo &h, const double *sendbuf, double *recvbuf, hipStream_t s);
void peer_exchange_bulk(const PeerBulk &h, const double *sendbuf, double *recvbuf, hipStream_t s);
// Jacobi / Schur pieces
void jacobi(const double *dinv, const double *x, double *y, int64_t n, const int32_t *done, hipStream_t s);
void extract_diag_inv(const CsrDev &A, double *dinv, hipStream_t s);
// y0 = dinv .* (x0 - Bt y1)            (mode 0, UPPER)
// y0 = dinv .* x0 - dinv .* (Bt y1)    (mode 1, FULL third step, recomputing D x0)
// scratch != nullptr and Bt tiled (general blocks): Bt y1 by the stream kernel into scratch, then the combination
void bt_update(int mode, const CsrDev &Bt, const double *dinv, const double *x0, const double *y1,
               double *y0, const int32_t *done, hipStream_t s, double *scratch = nullptr);
// FP32 inner solve (damped-Jacobi Richardson sweeps on the diagonal block of A)
void cvt_scale_f32(const double *x, const float *d32, float omega, float *x32, float *y32, int64_t n,
                   const int32_t *done, hipStream_t s);                       // x32 = (float)x ; y32 = omega d32 x32
void jacobi_sweep_f32(const CsrDev &A, const float *val32, const float *d32, float omega, const float *x32,
                      const float *yin, float *yout, const int32_t *done, hipStream_t s);
void sweep_offdiag_f32(const CsrDev &Ao, const int32_t *rows, const float *d32, float omega, const double *xg,
                       float *y, const int32_t *done, hipStream_t s);        // y[row] -= omega d (Ao_row . xg)
void gather_f32(const float *x, const int32_t *idx, int64_t n, double *out, const int32_t *done, hipStream_t s);
// y = (double)y32  (mode 0)  |  y -= (double)y32  (mode 1)
void cvt_f32_out(const float *y32, double *y, int mode, int64_t n, const int32_t *done, hipStream_t s);
void cvt_vals_f32(const double *v, float *v32, int64_t n, hipStream_t s);
// c = x0 - Bt y1 (mode 2) | c = Bt y1 (mode 3): the vector handed to the inner solve
// small scalar kernels
void schur_y1(int fact, int m, const double *x1, const double *t, const double *shat, double *y1,
              const int32_t *done, hipStream_t s);
void copy_small(const double *src, double *dst, int n, const int32_t *done, hipStream_t s);
// The exact Schur complement of m <= 8 constraint rows (spk_k_schurw.hip; spk_pc_set_schur_pre): W = the m dense columns
// of A^ ^-1 B^T as planes of stride ldw (zero beyond the local rows), L = the Cholesky factor of S = B W (lower, row-major)
struct SchurW {
    const double *W;
    int64_t ldw;
    int m;
    const double *L;
};
// y1 = S^-1 (W^T x0 - x1) in one pass over x0 and the m planes (fact LOWER / FULL; the signs are schur_y1's); the
// finishing workgroup solves with L.  f.out is not used
void schur_w_dot(const SchurW &w, const double *x0, int64_t nl, const double *x1, double *y1, const Finish &f,
                 const int32_t *done, hipStream_t s);
// y1 = S^-1 x1 (DIAG) | -S^-1 x1 (UPPER): one wave
void schur_w_y1(const SchurW &w, int fact, const double *x1, double *y1, const int32_t *done, hipStream_t s);
// y0 = src - sum_r y1_r W_r over nl entries (dinv != nullptr: dinv .* src stands for src)
void schur_w_out(const SchurW &w, const double *src, const double *dinv, const double *y1, double *y0, int64_t nl,
                 const int32_t *done, hipStream_t s);

// Krylov scalar kernels (single wave)
// where krylov_cycle_begin reports the solve's state to the host (pinned, device-visible memory)
struct StateReport {
    KrylovState *host_state;
    int32_t *host_words;            // [0] reduction error word, [1] communicator error word
    const int32_t *errw, *commerr;  // device words (nullptr: none)
};
struct KrylovArrays {
    KrylovState *st;
    double *H, *cc, *ss, *rs, *nrs, *hcol, *hist, *tb;
    int32_t hist_cap, ldh;
    int32_t tentative;  // 1: the recurrence may end a cycle, only a true residual may end the solve
    // > 0 (an FP32 basis, with tentative): -ksp_max_it seen by the recurrence is tentative too, and a cycle also ends once
    // the recurrence residual is <= theta times the residual the cycle started from (kBasisTheta)
    double theta;
};
// Early restart of a solve on an FP32 basis: FP32's unit round-off 2^-24 with 16x head-room.  Below theta * beta the stored
// vectors carry rounding noise only (a strong preconditioner stalls near 1e-7 beta): the cycle ends, the true residual
// of the restart takes over.  A named constant, not an option.
constexpr double kBasisTheta = 1.0 / 1048576.0;   // 2^-20
// where a reducer reports a partial that never arrived (execution failure, not a numerical one): the
// context's sticky error word; the bound of the wait in 100 MHz ticks
struct FinErr {
    int32_t *err;
    uint32_t ticks;
};
// The Givens step of iteration `loc` (Hessenberg column h[0..loc], ||w'||^2 in *nrm2), carried by workgroup 0 of a
// product launch: the serial chain runs beside the row tiles instead of at the tail of the MAXPY launch's reducer.
// The tiles of that launch read the gate words BEFORE the step may set them (they compute a product nobody uses when
// the step converges: no reduction in the launch depends on them).
struct GivensRider {
    KrylovArrays ka;
    int32_t loc;     // < 0: no rider
    const double *h;
    double *nrm2;
    double *sc;      // un-normalised basis: sc[loc + 1] = 1 / sqrt(*nrm2) is set first (nullptr: not)
    // fin_n > 0: *nrm2 is first REDUCED here from the fin_n partial rows the MAXPY launch published (+ the row behind
    // them: the multiplier entries' share), then all-reduced across ranks when ar.P != 0
    double *fin_partials;
    int32_t fin_n;
    FinErr fe;
    PeerAR ar;
};
// kernel B (forms 5 and 7, spk_k_iter.hip): w' = s_w w~ - V~ (h .* sc), ||w'||^2, and the next iteration's PC / B^T product
struct IterB {
    const double *V;
    int64_t ldv;
    int nv;
    const double *dots;  // reduced [h, q]
    double *tb;
    double *w;           // V_{loc+1}: in w, out w'
    const double *dinv, *bd;
    int64_t ldb;
    const double *shat, *gram;
    int fact;
    int64_t nl;
    int m, packed;
    double *zun;         // out: z~
    double *c;           // out: c~ = pre-load of the next product (V_{loc+2}); nullptr with m = 0
    const double *wl_in;
    int lam_in_dot;
    double *partials, *out;  // out[0] = ||w'||^2
    PeerAR ar;
    int32_t *err;
    uint32_t fin_ticks;
    SendRanges sr;
    int gmain;           // set by the launcher
    const int32_t *done;
    // un-normalised basis, sc required: dots are RAW inner products of V~_i with w~, the scale factors
    // sc[i] = 1 / ||w'_i|| are applied to the scalars here (h_i = sc_i s_w dots_i, MAXPY coefficient h_i sc_i,
    // w = s_w w~); zun is Z_{loc+1} itself; the reducer stores the scaled Hessenberg column (hbuf).  sc[nv] and the
    // Givens step of THIS iteration follow in the rider of the next product launch (GivensRider).  No vector is ever
    // normalised, no pass exists for it.
    double *sc, *hbuf, *wl_out;
    KrylovArrays ka;
    int loc;
    // an FP32 basis (iter_maxpy_uhead with b.w32): V points at floats (stride ldv floats), w~ stays FP64 in w and
    // float(w') goes to w32 -- ||w'||^2 is taken from the ROUNDED values, z~ and c~ from the unrounded ones
    float *w32;
    int defer_fin;       // publish the partials of ||w'||^2 and leave: the rider of the next product launch reduces them
    int dead_out;        // the cycle's last iteration: nobody reads w', z~, c~ (x += Z y takes Z_0 .. Z_{mk-1}, r comes from x): not stored
};
// Form 7: VecMDot and kernel B in one launch (gs_fused_kernel).  b as for iter_maxpy_uhead (dots unused; defer_fin set except behind a cycle's last iteration,
// one rank); MDot's operands below.  Returns the number of partial rows of ||w'||^2 (GivensRider::fin_n).
struct GsArgs {
    const double *V2;    // planes of B D (parity-interleaved when split)
    int cnt, split;      // cnt = nv + m values (<= 40), w.w after them
    int variant, pad;    // the GsVariant launched (set by the launcher; no kernel reads it: the fields behind it stay where they are)
    int64_t n2, n_dot;   // MDot's length in double2 (the multiplier entries included), entries that count
    double *partials;    // MDot's partial rows (column offset 1 of the context's partials)
    double *out;         // the reduced [h, q, w.w] (as mdot's Finish::out)
    double *tot, *tot_next;   // the armed totals line of this launch, the line it arms for the next one
    FinErr fe;
};
static_assert(sizeof(GsArgs) == 88 && offsetof(GsArgs, V2) == 0 && offsetof(GsArgs, cnt) == 8 && offsetof(GsArgs, split) == 12 &&
              offsetof(GsArgs, n2) == 24 && offsetof(GsArgs, n_dot) == 32 && offsetof(GsArgs, partials) == 40 &&
              offsetof(GsArgs, out) == 48 && offsetof(GsArgs, tot) == 56 && offsetof(GsArgs, tot_next) == 64 &&
              offsetof(GsArgs, fe) == 72, "GsArgs is a kernel argument: the kernels read these fields at these offsets");
// launches the instantiation v names (gs_fused_variant in spk_gs_launch.hpp resolves it from the knobs and the shape)
int gs_fused(IterB b, GsArgs g, GsVariant v, hipStream_t s);
int gs_fused_occupancy(int ng, int m, bool keep);   // workgroups of the fused kernel (with / without its keep set) that fit one CU
// GS_STAMPS=1 builds: the launches' phase time stamps, 64 iterations x 256 workgroups x 8 (spk_gs_stamps.hpp); false otherwise
bool gs_stamps(unsigned long long *out);
// Resident restart cycle (spk_k_resident.hip): ONE launch runs iterations 0 .. mk-1 of a cycle with the basis in registers
// (single rank, row-type layout with 2x2 blocks, <= 512 block rows per CU, restart <= 30, <= 4 planes of B D).  On entry
// V0 = v_0 (normalised), V1 = K z_0; Z_1.. are written; the Krylov scalars end up where krylov_cycle_end expects them.
struct ResidentArgs {
    int mk, m, packed, fact, lam_in_dot;
    int64_t nl, ld;
    const double *V0, *V1;
    double *Z;
    const double *dinv, *bd;
    int64_t ldb;
    const double *shat, *gram;
    double *P;             // resident_scratch_doubles() doubles
    KrylovArrays ka;
    double *sc_out;
    int32_t *err;
    uint32_t ticks;
    PeerAR ar;             // several ranks: Comm::resident_plan (P <= 1: single rank)
    SendRanges sr0, sr1;
    OffDiag od;
};
bool cycle_resident(const DictDev &A, int num_cus, ResidentArgs r, const int32_t *done, hipStream_t s);   // false: shape does not fit
int64_t resident_scratch_doubles(int num_cus, int mk);
bool resident_fits(const DictDev &A, int num_cus, int mk, int planes);   // planes: dense planes of B D the iteration streams
int iter_maxpy_uhead(IterB b, hipStream_t s);   // returns the number of partial rows (GivensRider::fin_n)
// MINRES and pipelined CG: a scalar step of the state S, run by the finishing workgroup of the pass that reduces its sums
// (one rank) or by state_scalar after the all-reduce
template <class S>
struct Step {
    S *state;
    int mode;            // kMr* / kPc*, < 0: no step in the kernel (several ranks)
    double *hist;
    int32_t hist_cap;
};
// the state before the first start (S = PipecgState: tau, pipecgrr's threshold); the scalar step after the all-reduce
// (the iteration steps are gated like the passes).  One kernel each for both states (spk_device.hpp)
template <class S, class... Tau>
void state_init(S *state, const spk_opts &o, int norm, hipStream_t s, Tau... tau);
template <class S>
void state_scalar(Step<S> step, const double *sums, const int32_t *done, hipStream_t s);
// MINRES (spk_k_minres.hip).  sums = [<.,.>, ||.||^2]
enum { kMrBnorm = 0, kMrBegin = 1, kMrDelta = 2, kMrTest = 3, kMrRecur = 4 };
// v pass: v_{j+1} = ig p - dg v_j - gg v_{j-1} into vm (resid != 0: vm = r = p - vj, vj == nullptr: vm = p, r2 a
// second copy); z = M^-1 v (z == nullptr: no PC in the pass); sums = [<z, v>, v.v (sq)] over the first n_dot entries
void minres_vz(const double *p, const double *vj, double *vm, double *r2, double *z, const double *dinv, const double *shat,
               int64_t nl, int64_t n, int64_t n_dot, int resid, int sq, const MinresState *ms, Step<MinresState> step,
               const Finish &f, const int32_t *done, hipStream_t s);
// lagged pass: (wx) w_{j+1} = (ig z_j - a3 w_{j-1} - a2 w_j) ia1 into wm, x += cx w_{j+1}; (kwm) the same for K w with
// p_j, r -= cx K w_{j+1}; sums = [<da, db>, r.r (kwm) | db.db (sq)]
void minres_wd(int wx, const double *zp, const double *pp, double *wm, const double *w, double *x, double *kwm,
               const double *kw, double *r, const double *da, const double *db, int sq, int64_t n, int64_t n_dot,
               const MinresState *ms, Step<MinresState> step, const Finish &f, const int32_t *done, hipStream_t s);
// pipelined CG (spk_k_pipecg.hip).  sums = [<r, u>, <w, u>, r.r]
// pipecgrr adds kPcGap (sums = [||(b - K x) - r||^2, 0, r.r]: a replacement when the gap crosses tau ||r||, rr_idle = 0) and kPcReplace (the sums of the replaced
// vectors: the next pass's scalars from gamma_old, alpha_old)
enum { kPcBnorm = 0, kPcBegin = 1, kPcStart = 2, kPcIter = 3, kPcGap = 4, kPcReplace = 5 };
// r = b - kx (kx == nullptr: r = b; b is read without its pad); u = uin, or D r (dinv; nullptr: r) written to uout when
// given; sums (sums != 0) = [<r, u>, 0, r.r] over the first n_dot entries.  Not gated.
void pipecg_begin(const double *b, const double *kx, double *r, const double *uin, double *uout, const double *dinv, int sums,
                  int64_t n, int64_t n_dot, const PipecgState *ps, Step<PipecgState> step, const Finish &f, hipStream_t s);
// upd: z = n + b z, s = w + b s, p = u + b p, x += a p, r -= a s, w -= a z (first: no old z / s / p / q read), with urec
// also q = m + b q, u -= a q; u == nullptr: u = D r (dinv; nullptr: u = r) in the pass; mout: D w written.  upd = 0:
// only the sums (and mout) of the vectors as they are.  sums = [<r, u>, <w, u>, r.r]
void pipecg_pass(int upd, int urec, int sums, const double *nv, double *z, double *s_, double *p, double *x, double *r,
                 double *w, double *u, double *q, const double *m, double *mout, const double *dinv, int64_t n, int64_t n_dot,
                 const PipecgState *ps, Step<PipecgState> step, const Finish &f, const int32_t *done, hipStream_t s);
// pipecgrr's gap check: sums = [||(b - t) - r||^2, 0, r.r] (t = K x; b read without its pad), then the step kPcGap.
// Gated by done
void pipecgrr_gap(const double *b, const double *t, const double *r, int64_t n, int64_t n_dot, const PipecgState *ps,
                  Step<PipecgState> step, const Finish &f, const int32_t *done, hipStream_t s);
// pipecgrr's replacement fills, gated by gate: t != nullptr: r = a - t (a read without its pad); t == nullptr: r = a as it
// is (not written).  Then uout = D r (dinv; nullptr: r) when uout is given
void pipecgrr_fill(const double *a, const double *t, double *r, double *uout, const double *dinv, int64_t n,
                   const int32_t *gate, hipStream_t s);
void krylov_init(const KrylovArrays &ka, const spk_opts &o, const double *bnorm2, hipStream_t s);
void krylov_cycle_begin(const KrylovArrays &ka, const double *nrm2, hipStream_t s, double *tb = nullptr, int m = 0,
                        double *sc = nullptr, const StateReport *report = nullptr);
void krylov_givens(const KrylovArrays &ka, int loc, const double *dots, const double *nrm2, hipStream_t s);
// head of a fused Schur iteration: VecScale + PCApply + B^T part of MatMult in one pass, plus the
// previous iteration's Givens step in workgroup 0 (loc_prev < 0: none)
void fused_head(double *v, const double *nrm, const double *w1raw, const double *dinv, const double *bd, int64_t ldb,
                const double *shat, const double *gram, int fact, int64_t nl, int m, double *z, double *c,
                const KrylovArrays &ka, int loc_prev, const double *dots_prev, const int32_t *done, hipStream_t s,
                const SendRanges *sr = nullptr, int bd_packed = 0, double *wl_out = nullptr);
// single-reduction mode: MAXPY of iteration loc + head of iteration loc+1 + Givens of iteration loc
// in one pass (dots = reduced [h, B D w, w.w]; tb = B D v_i per basis vector, (restart+2) x 8)
void maxpy_head(const double *V, int64_t ldv, int nv, const double *dots, double *tb, double *nrm_out, double *w,
                const double *dinv, const double *bd, int64_t ldb, const double *shat, const double *gram, int fact,
                int64_t nl, int m, double *z, double *c, double *w1side, const double *wl_in, double *wl_out,
                const KrylovArrays &ka, int loc, const int32_t *done, hipStream_t s, const SendRanges *sr = nullptr,
                int bd_packed = 0);
// sc: y_i *= sc[i] (un-normalised Z); restart > kMaxNv - 2: the triangle stays in global memory
// pending: the Givens step of the cycle's last iteration, run first in the same launch (ka, loc, h, nrm2 are read)
void krylov_cycle_end(const KrylovArrays &ka, hipStream_t s, const double *sc = nullptr, int restart = 0,
                      const GivensRider *pending = nullptr);
// CGS refinement: decide (device side) whether the second pass runs, then fold its results
// (h2 into h, norm/traw of the refined vector over the first pass's)
void krylov_refine_decide(const KrylovArrays &ka, int loc, int mode, const double *dots, const double *nrm2,
                          double *dots2, hipStream_t s);
void krylov_refine_merge(const KrylovArrays &ka, int loc, double *dots, const double *dots2, double *nrm,
                         const double *nrm_b, int nn, hipStream_t s);
// one transfer of a grid-coarsened level (SPK_AMG_COARSEN_GRID): the node grids on both sides and the node size
struct AmgGrid {
    int32_t fd[3] = {0, 0, 0}, cd[3] = {0, 0, 0};   // fine and coarse nodes per side; cd[a] != fd[a]: the direction halves
    int32_t bs = 0;
    bool on = false;            // the level was built by the grid rule
    bool matrix_free = false;   // ... and the V-cycle applies P and R without reading them
    void set(const int32_t *f, const int32_t *c, int b, int transfer)
    {
        for (int a = 0; a < 3; ++a) fd[a] = f[a], cd[a] = c[a];
        bs = b;
        on = true;
        matrix_free = transfer == SPK_AMG_TRANSFER_MATRIX_FREE;
    }
};
// what the matrix-free transfer kernels take of an AmgGrid
struct GridArgs {
    int32_t fx, fy, cx, cy, cz;   // fine nodes in x, y; coarse nodes per side
    int32_t hx, hy, hz;           // 1: the direction halves
    int32_t ex, ey, ez;           // 1: ... and its fine side is even
};
inline GridArgs grid_args(const AmgGrid &a)
{
    const int32_t hx = a.cd[0] != a.fd[0], hy = a.cd[1] != a.fd[1], hz = a.cd[2] != a.fd[2];
    return GridArgs{a.fd[0], a.fd[1], a.cd[0], a.cd[1], a.cd[2], hx, hy, hz, hx && !(a.fd[0] & 1), hy && !(a.fd[1] & 1), hz && !(a.fd[2] & 1)};
}
// The fused tail (amg_tail_kernel): what one workgroup needs of the levels >= first, device-resident, written at every
// set-up.  The matrices, D^-1 and the coarse inverse are read-only in the launch; b, ya and yb are written and read by
// other waves behind a workgroup barrier -- plain pointers.
// T: the scalar type of the tail's levels -- double, or float under SPK_AMG_PRECISION_SINGLE (the tail never contains
// level 0, so it is FP32 throughout: av is the level's FP32 value array, the index arrays and pv, rv are not read)
constexpr int kAmgMaxSmooth = 64;   // amg_check_opts: smooth_its <= 64
template <typename T>
struct AmgTailLevelT {
    const int32_t *arp, *aci, *prp, *pci, *rrp, *rci;   // CSR of A_l, and of P_l, R_l to level l + 1 (stored transfers)
    const T *av, *pv, *rv, *dinv;
    T *b, *ya, *yb;
    int32_t n, nc;                  // rows of the level and of level l + 1
    int32_t nu, bs, matrix_free, fz;   // smoothing steps; node size; the transfers are the grid rule's; fine nodes in z
    int32_t stencil, nd[3];         // A_l is applied from av alone (SPK_AMG_OPERATOR_STENCIL); the level's node grid
    GridArgs g;
    T alpha[kAmgMaxSmooth], beta[kAmgMaxSmooth];
};
using AmgTailLevel = AmgTailLevelT<double>;
// one step as the kernel reads it: sel / sel_next = which buffer (0: ya, 1: yb) holds the iterate of the step's level /
// of the level below it when the step begins, resolved on the host (smooth()'s rule) so that no thread chooses
struct AmgTailStep { int32_t kind, level, sel, sel_next; };
template <typename T>
struct AmgTailDescT {
    const T *cinv;              // the coarse inverse (level `levels` - 1), dense row-major
    const AmgTailStep *steps;   // the whole cycle's list (a launch takes a range of it)
    int32_t first, levels;
    AmgTailLevelT<T> lv[SPK_AMG_MAX_LEVELS];   // by level; those below `first` are not filled
};
using AmgTailDesc = AmgTailDescT<double>;
using AmgTailDescF32 = AmgTailDescT<float>;
constexpr int kAmgTailThreads = 1024;   // one workgroup, 16 waves: 128 CSR rows or 16 dense rows per sweep
// steps [s0, s1) of d->steps -- one tail run -- in one launch of one workgroup; stencil: a level of the tail has its
// `stencil` flag set (the kernel that knows the value-array route; without, the kernel is the one of the CSR route alone)
void amg_tail(const AmgTailDesc *d, bool stencil, int32_t s0, int32_t s1, const int32_t *done, hipStream_t s);
void amg_tail(const AmgTailDescF32 *d, bool stencil, int32_t s0, int32_t s1, const int32_t *done, hipStream_t s);   // (one kernel: it knows both routes)
// smoothed-aggregation multigrid (spk_k_amg.hip): CSR levels, eight lanes per row
void amg_spmv(const CsrDev &A, const double *x, double *out, const int32_t *done, hipStream_t s);              // out = A x
void amg_cheb_csr(const CsrDev &A, const double *dinv, const double *b, const double *y, const double *yo, double *out,
                  double alpha, double beta, const int32_t *done, hipStream_t s);   // out = y + a D^-1 (b - A y) + b (y - yo)
// the same two on an n-row level with the grid stencil's closed-form pattern (nd: its node grid, bs its node size), from its
// value array `val` alone -- rowptr and colidx are not read (SPK_AMG_OPERATOR_STENCIL; spk_stencil_op_core.hpp states the
// sums).  mode 0: out = A x; mode 1: out = x + alpha dinv (b - A x) + beta (x - yo).  stencil_op_rows: the rows of one workgroup
struct StencilOpArgs { int32_t nx, ny, nz, n; };   // the level's node grid and its rows
int stencil_op_rows(const int32_t nd[3], int bs, size_t elem = sizeof(double));   // elem: sizeof of the scalar type
void amg_stencil_op(int32_t n, const double *val, const int32_t nd[3], int bs, int mode, const double *x, const double *dinv,
                    const double *b, const double *yo, double *out, double alpha, double beta, const int32_t *done, hipStream_t s);
// The FP32 forms of SPK_AMG_PRECISION_SINGLE, overloads on the vectors' types.  The level operator from the FP32 copy `val`
// of the level's value array (the rows of a workgroup keep the byte budget of stencil_op_rows, so a float workgroup
// takes up to twice the rows);  the vector step (amg_cheb_vec below);  the dense product;
// the transfers float -> float between FP32 levels, and at the level 0 / level 1 boundary R (b - t) summed in FP64 and
// rounded once on the store, y += P e with every e widened and the sums in FP64
void amg_stencil_op(int32_t n, const float *val, const int32_t nd[3], int bs, int mode, const float *x, const float *dinv,
                    const float *b, const float *yo, float *out, float alpha, float beta, const int32_t *done, hipStream_t s);
void amg_cheb_vec(int64_t n, const float *dinv, const float *b, const float *t, const float *y, const float *yo, float *out,
                  float alpha, float beta, const int32_t *done, hipStream_t s);
void amg_dense(const float *C, int32_t n, const float *b, float *y, const int32_t *done, hipStream_t s);
void amg_restrict_grid(const AmgGrid &g, const float *b, const float *t, float *out, const int32_t *done, hipStream_t s);
void amg_restrict_grid(const AmgGrid &g, const double *b, const double *t, float *out, const int32_t *done, hipStream_t s);
void amg_prolong_add_grid(const AmgGrid &g, const float *e, float *y, const int32_t *done, hipStream_t s);
void amg_prolong_add_grid(const AmgGrid &g, const float *e, double *y, const int32_t *done, hipStream_t s);
// dst[i] = (float)src[i], one rounding to nearest (the FP32 copies of a set-up; no `done` gate)
void amg_round_f32(int64_t n, const double *src, float *dst, hipStream_t s);
void amg_restrict(const CsrDev &R, const double *b, const double *t, double *out, const int32_t *done, hipStream_t s);   // out = R (b - t)
void amg_prolong_add(const CsrDev &P, const double *e, double *y, const int32_t *done, hipStream_t s);          // y += P e
// y == nullptr: out = alpha dinv b (zero initial guess); else out = y + alpha dinv (b - t) + beta (y - yo) (yo null: 0)
// the same two on a grid-coarsened level without reading P or R: the weights are powers of two, the sums run in
// ascending column order from the first product
void amg_restrict_grid(const AmgGrid &g, const double *b, const double *t, double *out, const int32_t *done, hipStream_t s);
void amg_prolong_add_grid(const AmgGrid &g, const double *e, double *y, const int32_t *done, hipStream_t s);
void amg_cheb_vec(int64_t n, const double *dinv, const double *b, const double *t, const double *y, const double *yo,
                  double *out, double alpha, double beta, const int32_t *done, hipStream_t s);
// the fine level's fused step on the 2x2 row-type layout (false: A is not that layout, nothing launched)
bool amg_cheb_dict2(const DictDev &A, const double *dinv, const double *b, const double *y, const double *yo, double *out,
                    double alpha, double beta, const int32_t *done, hipStream_t s);
void amg_dense(const double *C, int32_t n, const double *b, double *y, const int32_t *done, hipStream_t s);     // y = C b
void amg_out(int mode, int64_t n, const double *src, double *dst, const int32_t *done, hipStream_t s);          // = / -=
// the multigrid set-up on the device (spk_k_amg_setup.hip); no launch takes the `done` gate
void amgs_rows_sorted(const int32_t *rp, const int32_t *ci, int32_t n, int32_t *flag, hipStream_t s);   // *flag |= 1: a row descends
void amgs_sort_rows(const int32_t *rp, int32_t *ci, double *v, int32_t n, hipStream_t s);
void amgs_node_norms(const int32_t *rp, const int32_t *ci, const double *v, int32_t nn, int bs, double *dn, hipStream_t s);
// gp null: out[I] = strong neighbours of node I; else the neighbours at out[gp[I]..), ascending
void amgs_graph(const int32_t *rp, const int32_t *ci, const double *v, int32_t nn, int bs, double theta, const double *dn,
                const int32_t *gp, int32_t *out, hipStream_t s);
void amgs_grid_prolongator(const AmgGrid &g, int32_t *rp, int32_t *ci, double *v, hipStream_t s);   // P of g: row pointers, columns, weights
// the grid-stencil Galerkin product (SPK_AMG_GALERKIN_STENCIL; spk_galerkin_core.hpp): row pointers, columns and values
// of N = A_{l+1} from the sorted CSR of A = A_l over the node grids of g, in two launches (gather, symmetrise in place); N's
// buffers hold gs_nnz(g.cd, g.bs) entries.  check: *bad = min(*bad, row << 32 | column) over A's entries outside the stencil
void amgs_galerkin_stencil(const AmgGrid &g, const CsrDev &A, CsrDev &N, hipStream_t s);
void amgs_galerkin_stencil_check(const AmgGrid &g, const CsrDev &A, unsigned long long *bad, hipStream_t s);
void amgs_tent_count(const int32_t *agg, int32_t nrows, int bs, int32_t *cnt, hipStream_t s);
void amgs_tent_fill(const int32_t *agg, const double *inv, int32_t nrows, int bs, const int32_t *rp, int32_t *ci, double *v,
                    hipStream_t s);
// C = A B: bound[i] = slots row i may need, *total += their sum; expand into the slices at off[i]; compact behind rp
void amgs_spgemm_bound(const CsrDev &A, const CsrDev &B, int32_t *bound, unsigned long long *total, hipStream_t s);
void amgs_spgemm_expand(const CsrDev &A, const CsrDev &B, const int32_t *off, int32_t *sc, double *sv, int32_t *cnt, hipStream_t s);
void amgs_compact(int32_t n, const int32_t *off, const int32_t *rp, const int32_t *sc, const double *sv, int32_t *ci, double *v,
                  hipStream_t s);
// C = a A + b diag(scale) B over the union pattern (scale null: 1); crp null: cnt[i] = length of row i, else the fill
void amgs_add(double a, const CsrDev &A, double b, const CsrDev &B, const double *scale, const int32_t *crp, int32_t *cci,
              double *cv, int32_t *cnt, hipStream_t s);
void amgs_col_count(const int32_t *ci, int64_t nnz, int32_t *cnt, hipStream_t s);
void amgs_transpose_fill(const CsrDev &A, int32_t *pos, int32_t *tci, double *tv, hipStream_t s);   // rows unsorted: amgs_sort_rows
// the refresh: *flag |= 1 where a and b differ; the values of C = A B and of N = (Ac + Ac^T) / 2 on their kept sorted
// patterns in the build's summation order (*err |= 1: a product without a slot; nothing is written outside the row)
void amgs_pattern_equal(const int32_t *a, const int32_t *b, int64_t n, int32_t *flag, hipStream_t s);
void amgs_spgemm_numeric(const CsrDev &A, const CsrDev &B, CsrDev &C, int32_t *err, hipStream_t s);
void amgs_symmetrise_numeric(const CsrDev &Ac, CsrDev &N, int32_t *err, hipStream_t s);
// dscale, ascale: powers of two (1 on a build) -- sv = sqrt|dinv dscale|, w = sv (aw ascale): the steps on ascale A
void amgs_lz_init(int64_t n, const double *dinv, double dscale, double *sv, double *q, const Finish &f, hipStream_t s);
void amgs_abs_sum(int64_t n, const double *x, const Finish &f, hipStream_t s);   // f.out[0] = sum |x|
void amgs_lz_scale(int64_t n, double nb, const double *w, const double *sv, double *q, double *t, hipStream_t s);
void amgs_lz_dot(int64_t n, const double *sv, const double *aw, double ascale, double *w, const double *q, const Finish &f, hipStream_t s);
void amgs_lz_update(int64_t n, double a, double be, const double *q, const double *qp, double *w, const Finish &f, hipStream_t s);
// the same four passes under SPK_AMG_LANCZOS_RESIDENT: the scalars come from and go to the state block st on the device
// (spk_lanczos_core.hpp; f.out is not written), and a pass behind the stop returns at its entry.  scale: jb < 0 divides by
// st->nq, else by st->be[jb];  dot of step j: st->al[j];  update of step j of kk: reads al[j], be[j], keeps the break rule
void amgs_lz_init_resident(int64_t n, const double *dinv, double dscale, double *sv, double *q, const Finish &f,
                           lanczos_core::LzState *st, hipStream_t s);
void amgs_lz_scale_resident(int64_t n, int jb, const double *w, const double *sv, double *q, double *t, const lanczos_core::LzState *st,
                            hipStream_t s);
void amgs_lz_dot_resident(int64_t n, int j, const double *sv, const double *aw, double ascale, double *w, const double *q,
                          const Finish &f, lanczos_core::LzState *st, hipStream_t s);
void amgs_lz_update_resident(int64_t n, int j, int kk, const double *q, const double *qp, double *w, const Finish &f,
                             lanczos_core::LzState *st, hipStream_t s);
}  // namespace k

// what the cycle reads and writes of one level in the scalar type T of its vectors (AmgLevelDev::view)
template <typename T>
struct AmgLevelView {
    const T *val, *dinv;                  // the operator's value array and D^-1 (levels >= 1)
    T *b, *ya, *yb;
    const std::vector<T> &alpha, &beta;
};
// the device copy of the hierarchy (spk_amg_setup.cpp): level 0 keeps the context's A layout and diag(A)^-1
struct AmgLevelDev {
    int32_t n = 0;
    CsrDev A, P, R;                    // A: levels >= 1; P, R: all but the coarsest
    CsrDev Ptent;                      // device-built hierarchies only (test hook)
    CsrDev AP, Ac;                     // device-built with reuse on: A_l P_l and R_l A_l P_l, patterns and the refresh's value buffers (empty under SPK_AMG_GALERKIN_STENCIL)
    std::vector<int32_t> agg;          // device-built hierarchies only: the aggregates the host step returned
    DevBuf<double> dinv;               // levels >= 1
    DevBuf<double> b, ya, yb, t;       // right-hand side, two iterates, the fine level's product
    std::vector<double> alpha, beta;   // smoothing steps: y+ = y + alpha D^-1 (b - A y) + beta (y - y-)
    k::AmgGrid grid;                    // grid coarsening: the transfer to level l+1
    bool stencil_op = false;           // the cycle applies A from A.val alone (SPK_AMG_OPERATOR_STENCIL; amg_plan_cycle sets it)
    // SPK_AMG_PRECISION_SINGLE, levels >= 1: the same in FP32 -- val and dinv the copies of A.val and dinv (amg_round_levels,
    // behind every build and refresh), the cycle vectors in float (b, ya, yb above stay empty there) and the smoothing
    // coefficients rounded
    struct F32 {
        DevBuf<float> val, dinv, b, ya, yb;
        std::vector<float> alpha, beta;
    } f32;
    // double: what the set-up owns above; float: the copies
    template <typename T>
    AmgLevelView<T> view()
    {
        if constexpr (std::is_same<T, double>::value) return {A.val.p, dinv.p, b.p, ya.p, yb.p, alpha, beta};
        else return {f32.val.p, f32.dinv.p, f32.b.p, f32.ya.p, f32.yb.p, f32.alpha, f32.beta};
    }
};
// what a set-up with reuse on (spk_pc_set_amg_reuse) keeps beside the hierarchy, so that the next one can refresh it
struct AmgReuse {
    spk_amg_opts o{};                  // as spk_pc_set_amg gave them
    int bs = 0;                        // the node size the context resolved (0: detected from the pattern)
    int32_t n = 0;
    int64_t nnz = 0, ld = 0;
    DevBuf<int32_t> rowptr, colidx;    // the diagonal block's pattern the hierarchy was built on, as the context stores it
    DevBuf<int32_t> flag;              // [0]: the patterns differ; [1]: a numeric kernel of the refresh missed a slot
    // the device route's level 0: the sorted copy of the context's CSR where its rows do not ascend, and D_0^-1
    CsrDev sorted;
    bool use_sorted = false;
    DevBuf<double> dinv0;
    double dinv_sum = 0.0;             // sum |D_0^-1| at the build (its binade: by which power of two A00 was rescaled since)
    DevBuf<double> sum;                // where the kernel leaves that sum
};
struct AmgDev {
    std::vector<AmgLevelDev> lv;
    DevBuf<double> cinv;
    spk_amg_info info{};         // what spk_get_amg_info returns, on both routes
    std::unique_ptr<AmgReuse> reuse;   // null unless built with reuse on
    // the application's plan (amg_plan_cycle, at every set-up): the steps in order, the buffer each one finds its
    // iterate in, the tail runs as ranges of steps, and the tail kernel's descriptor and step list on the device
    std::vector<AmgStep> steps;
    std::vector<k::AmgTailStep> tsteps;
    std::vector<std::pair<int64_t, int64_t>> runs;
    std::vector<int32_t> run_sel;   // per run: the buffer (0: ya, 1: yb) it leaves the iterate of level tail_first in
    bool tail_stencil = false;      // a level inside the tail applies A from its value array alone
    DevBuf<k::AmgTailDesc> tail_desc;
    DevBuf<k::AmgTailStep> tail_steps;
    // SPK_AMG_PRECISION_SINGLE: the levels >= 1 run in FP32 (the vectors were allocated so); the coarse inverse rounded, and
    // the tail's descriptor over the float buffers (tail_desc stays empty)
    bool single = false;
    struct F32 {
        DevBuf<float> cinv;
        DevBuf<k::AmgTailDescF32> tail_desc;
    } f32;
    // the coarse inverse and the tail's descriptor of the cycle whose levels >= 1 are T
    template <typename T>
    auto &coarse_inv() { if constexpr (std::is_same<T, double>::value) return cinv; else return f32.cinv; }
    template <typename T>
    auto &tail() { if constexpr (std::is_same<T, double>::value) return tail_desc; else return f32.tail_desc; }
};

}  // namespace spk

// ---------------------------------------------------------------------------
// the context
// ---------------------------------------------------------------------------
struct spk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    mutable std::string err;
    std::string peer_why;  // why the peer-store backend is off (spk_comm_get_info)
    std::unique_ptr<spk::Comm> comm;

    // sizes
    int64_t n_global = 0, row_begin = 0;
    int32_t n_local = 0, m = 0, n_ghost = 0;
    int64_t ld = 0;  // padded vector length (n_local + m rounded up)

    // (0,0) block: diagonal part, compressed off-rank part
    spk::CsrDev Ad, Ao;
    spk::BcsrDev Ab;               // 2x2-blocked copy of Ad when the structure allows
    int spmv_format = 0;           // 0 = CSR stream kernel, 1 = 2x2 blocks (Ab), 2 = 3x3 blocks (Ab3)
    spk::Bcsr3Dev Ab3;             // 3x3-blocked copy (dof-3 grids)
    spk::DictDev Adict;            // row types + deviation codes over the blocked copy (uniform grids); Adict.ok: the products use it
    spk::DevBuf<int32_t> ao_rows;  // local row of each compressed Ao row
    spk::DevBuf<int32_t> ao_rowptr_full;  // Ao row pointers over all local rows (SpMV epilogue form)
    spk::k::SendRanges send_ranges{};     // halo rows as contiguous ranges, when they are
    spk::k::OffDiag offdiag() const { return spk::k::OffDiag{ao_rowptr_full.p, Ao.colidx.p, Ao.val.p, xghost.p}; }
    bool have_A = false, have_B = false;

    // constraint block: B^T (n_local x m) by rows, always; B itself
    //   m <= 8        : every row in column windows (WideDev) -- the long-row kernel, and the fused dense-plane path
    //   m  > 8        : a general sparse block: CSR by rows (Bc, the stream kernel) with up to 8 LONG rows (more than
    //                   kWideRowNnz local entries) taken out into the windowed form (B, rows listed in wide_rows)
    spk::WideDev B;
    spk::CsrDev Bt, Bc;
    bool b_general = false;
    int m_wide = 0;
    spk::DevBuf<int32_t> wide_rows;
    std::vector<int32_t> wide_rows_h;
    spk::DevBuf<double> tmpb;  // scratch vector of the general block's D x0 / B^T y1 products
    const double *bt_cached = nullptr;   // the multiplier vector whose B^T product tmpb holds (op_pc_apply -> op_mult)

    // halo plan
    std::vector<int> peers;
    std::vector<int64_t> send_off, recv_off;  // per peer offsets (+ total at end)
    spk::DevBuf<int32_t> send_idx;
    spk::DevBuf<double> send_buf, xghost;

    // preconditioner
    int pc_type = SPK_PC_NONE, schur_fact = SPK_SCHUR_FULL;
    // agreed over the ranks at KSPSetUp: every rank's local size is even / non-zero.  The head-kernel paths need an even
    // local size, and all ranks must take the SAME path (their collective sequences differ): decided collectively, not
    // from rank-local facts
    bool even_all = false, nonempty_all = false;
    bool res_fit_all = false;   // every rank's slab fits the resident restart-cycle kernel
    bool pc_ready = false;
    spk::DevBuf<double> dinv, shat, gram;  // n_local, m, m*m
    spk::DevBuf<double> bd;                // the m rows of B D as dense vectors of stride ld (fused Schur path)
    spk::DevBuf<double> bdpk;              // the same as m/2 parity-interleaved planes, when the rows allow
    bool bd_packed = false;
    // the exact Schur complement of a few rows (spk_pc_set_schur_pre): asked for / built by the last set-up.  W = A^ ^-1 B^T:
    // the V-cycle's columns in sw, or -- A^ = diag(A) -- the planes of bd (then built for every factorisation)
    int schur_pre = SPK_SCHUR_PRE_SELFP_DIAG;
    bool schur_dense = false;
    spk::DevBuf<double> sw, sfac;          // m planes of stride ld; the Cholesky factor of S (m x m, lower)
    std::vector<double> schur_S;           // S as factored (host, m x m)
    double schur_setup_seconds = 0.0;      // what W, S and the factor added to the last set-up
    double assembly_seconds = 0.0;         // the kernels of the last device assembly, up to a device synchronise
    double constraints_seconds = 0.0;      // the same of the last set_block_constraints
    spk::k::SchurW schur_w() const { return spk::k::SchurW{amg_d ? sw.p : bd.p, ld, m, sfac.p}; }
    // FP32 inner solve (0 sweeps = plain diag(A)^-1)
    int inner_sweeps = 0;
    double inner_omega = 1.0;
    spk::DevBuf<float> a32, d32, x32, y32a, y32b;
    // smoothed-aggregation multigrid standing for A^-1 (spk_pc_set_amg; built at spk_pc_setup)
    bool amg_on = false;
    spk_amg_opts amg_opts{};
    std::unique_ptr<spk_amg_hier> amg_h;
    std::unique_ptr<spk::AmgDev> amg_d;
    // spk_pc_set_amg_reuse: a set-up on an unchanged pattern refreshes the hierarchy's values instead of building it;
    // what the last set-up did, and its wall time (spk_get_amg_reuse_info)
    bool amg_reuse = false, amg_refreshed = false;
    double amg_reuse_seconds = 0.0;
    spk::DevBuf<double> bigdots;   // Gram-Schmidt coefficients of restart lengths beyond the fused kernels' 62

    // scratch
    spk::DevBuf<double> partials;  // kMaxBlocks * kPartialLd
    spk::DevBuf<double> small;     // reduced scalars (256 doubles)
    spk::DevBuf<int32_t> errw;     // sticky device-side execution-error word (Finish::err)
    uint32_t fin_ticks = 400000000u;
    // measurement (spk_debug_time_products): HIP events on the solver's stream around the product launches of the
    // iterations (the launch with the Givens rider), read by spk_get_product_timing
    bool time_products = false;
    std::vector<hipEvent_t> tp_ev;   // pairs
    size_t tp_used = 0;
    spk::k::Finish fin(double *out) { return spk::k::Finish{partials.p, out, spk::k::PeerAR{}, errw.p, fin_ticks}; }
    spk::k::Finish fin(double *out, const spk::k::PeerAR &ar) { return spk::k::Finish{partials.p, out, ar, errw.p, fin_ticks}; }
    // throws SPK_ERR_HIP when a device-side wait of a cross-workgroup reduction has timed out (call after a
    // sync); re-arms the partials so that the context stays usable
    void check_device_error();
    spk::DevBuf<double> y1tmp, ttmp;

    // how the last spk_fgmres launched its iterations (spk_get_iteration_form): SPK_ITER_* actually run, -1 for the
    // step-by-step path (PCApply and MatMult as launches of their own); single-reduction mode beside it
    int last_form = -1, last_single = 0;
    // form 7's launches of the last spk_fgmres (spk_get_gs_launch): those that staged their remainder tile in LDS
    int last_gs_launches = 0, last_gs_tail = 0;

    // Krylov workspace (sized by restart)
    int ws_restart = -1, ws_basis = -1;   // what V (or Vf and Vw) and Z are sized for
    spk::DevBuf<float> Vf;       // the FP32 basis of a -spk_basis_precision single solve: restart + 1 vectors of ld floats
    spk::DevBuf<double> Vw;      // its two FP64 work vectors: w~ and c~ in turn (and r at the restart)
    int last_basis = -1;         // spk_get_basis_info
    int64_t last_basis_bytes = 0;
    spk::DevBuf<double> V, Z, xsol, rhs, tmp;
    spk::DevBuf<double> basis_sc;    // scale factors of the un-normalised basis (forms 5, 6, 7)
    spk::DevBuf<double> res_P;       // resident cycle kernel: all-to-all buffer of the inner products
    int num_cus = 0;                 // compute units of the device (grid of the resident cycle kernel)
    spk::DevBuf<double> gs_tot;      // form 7: two armed lines of MDot totals (the launch reads one, arms the other)
    uint32_t gs_seq = 0;
    int gs_occ[6] = {-1, -1, -1, -1, -1, -1};   // form 7: workgroups of the fused kernel per CU (none / <= 4 / <= 8 planes; 3..5: with its keep set), -1 unknown
    bool gs_fused_fits(int64_t nl, int m, bool keep);   // fat vectors and every workgroup of the fused launch resident at once
    spk::SolverWork minres_work, pipecg_work;   // spk_minres; spk_pipecg and spk_pipecgrr
    double pc_tau = SPK_PIPECGRR_TAU_DEFAULT;   // spk_pipecgrr_set_tau
    spk::DevBuf<double> kry_d;  // H, cc, ss, rs, nrs, hcol, hist
    spk::DevBuf<spk::KrylovState> kst;
    spk::k::KrylovArrays ka{};

    // staging for host-pointer entry points
    spk::DevBuf<double> stage_x, stage_y;

    void ensure_scratch();
    void ensure_vectors();
    // pageable host memory -> device through two pinned staging buffers (KSPSetOperators)
    void upload_staged(void *dst, const void *src, size_t bytes);
    void *pin_state = nullptr;     // pinned landing place of the per-cycle state read-back (KrylovState + error words)
    hipEvent_t state_ev = nullptr; // ... and the event behind its copies
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
};

namespace spk {
// solver pieces used by the API layer (spk_solver.cpp)
// y (+)= Ad x in the layout the context holds: row types + codes, 2x2 / 3x3 blocks or CSR (same sums in all of them)
void a_mult(spk_ctx *c, const double *x, double *y, const CsrDev *bt, const double *lam, const int32_t *done, bool accumulate,
            const k::OffDiag *od, const k::GivensRider *rider = nullptr);
void op_mult(spk_ctx *c, const double *x, double *y, const int32_t *done, bool halo_done = false, bool reuse_bt = false);
void op_pc_apply(spk_ctx *c, const double *x, double *y, const int32_t *done);
// out[r] = B_r . (x .* scale) over this rank's columns (scale == nullptr: B_r . x); no all-reduce
void apply_B(spk_ctx *c, const double *x, const double *scale, double *out, const int32_t *done);
void pc_setup(spk_ctx *c, int pc_type, int schur_fact);   // (spk_operator.cpp, like set_block below)
// multigrid set-up (spk_amg_setup.cpp): the host hierarchy from the context's A00 (single rank) and its upload
std::unique_ptr<spk_amg_hier> amg_build_ctx(spk_ctx *c);
void amg_upload(spk_ctx *c, std::unique_ptr<spk_amg_hier> h);
// the same hierarchy built on the device from c->Ad (-spk_gamg_setup device); touches nothing of the context but its
// reduction scratch and leaves c->amg_h null: "built on the device" is c->amg_d && !c->amg_h
std::unique_ptr<AmgDev> amg_build_device(spk_ctx *c);
// reuse (spk_pc_set_amg_reuse).  amg_can_refresh: reuse is on and the context's hierarchy was built with it, from these
// options, on this size and this pattern (one kernel compares).  amg_refresh_ctx: new values on every kept pattern, on the
// route that built; throws what the build would, the hierarchy is then half-refreshed and the caller drops it.
// amg_drop_reuse: releases what only a refresh needs.
bool amg_can_refresh(spk_ctx *c);
void amg_refresh_ctx(spk_ctx *c);
void amg_drop_reuse(spk_ctx *c);
// the test hooks on either route: the host hierarchy's copy, or a download from the device-built levels
void amg_ctx_level(spk_ctx *c, int l, int which, const CsrOut &out);
void amg_ctx_aggregates(spk_ctx *c, int l, int32_t *nnodes, int32_t *agg);
void amg_debug_lanczos(spk_ctx *c, int l, int resident, int32_t *steps, double *al, double *be);
// the multigrid cycle (spk_amg_cycle.cpp).  What every set-up ends in: the cycle's vectors (ld: the context's padded
// length) and the application's plan from the options and the levels as they are
void alloc_cycle_vectors(AmgDev &d, int64_t ld, bool single);
void amg_plan_cycle(AmgDev &d, const spk_amg_opts &o, int64_t ld, hipStream_t s);
void amg_debug_transfer(spk_ctx *c, int l, int which, int stored, int64_t fine_len, const double *a, const double *b, double *out);
void amg_debug_operator_f32(spk_ctx *c, int l, int which, float alpha, float beta, const float *x, const float *xo, const float *b,
                            float *out);
void amg_debug_transfer_f32(spk_ctx *c, int l, int which, int64_t fine_len, const void *a, const void *b, void *out);
void amg_debug_operator(spk_ctx *c, int l, int which, int stencil, double alpha, double beta, const double *x, const double *xo,
                        const double *b, double *out);
// one cycle, mode 0: y = V x, mode 1: y -= V x; last != nullptr: y is not written, *last = the buffer of the hierarchy that holds V x
void amg_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done, const double **last = nullptr);
void fgmres(spk_ctx *c, const double *b_dev, double *x_dev, const spk_opts &o, spk_result *res,
            double *history, int32_t history_cap);
void minres(spk_ctx *c, const double *b_dev, double *x_dev, const spk_opts &o, int norm, spk_result *res,
            double *history, int32_t history_cap);
void pipecg(spk_ctx *c, const double *b_dev, double *x_dev, const spk_opts &o, int norm, spk_result *res,
            double *history, int32_t history_cap);
// pipelined CG with residual replacement: pipecg plus the gap check at every chunk boundary (tau > 0 or 0: always)
void pipecgrr(spk_ctx *c, const double *b_dev, double *x_dev, const spk_opts &o, int norm, double tau, spk_result *res,
              double *history, int32_t history_cap, int32_t *replacements);
// what the two drivers share: the checks they start with (an operator, KSPSetUp done) ...
void require_setup(spk_ctx *c, const char *who);
// ... and their end: drain the stream, raise a communicator or device error, fill res, copy the history (hist: device)
void finish_solve(spk_ctx *c, const KrylovState &st, int32_t cycles, std::chrono::steady_clock::time_point t0,
                  const double *hist, int32_t hist_cap, spk_result *res, double *history, int32_t history_cap);
void set_block(spk_ctx *c, int which, int64_t row_begin, int32_t nrows_local, int64_t ncols_global,
               const int32_t *rowptr, const int32_t *colidx, const double *val);
// A00 of the reference's own discretisation assembled on the device, then set_block's chain.  mz == 0: the 2-D grid
// (spk_k_assembly.hip, whole node lines), else the 3-D generator's (spk_k_assembly3d.hip, whole node planes);
// laplace_mz3: the mz of a 3-D entry point, where 0 is no grid.  assemble_laplace_csr: the slab back on the host (a test hook).
void set_block_laplace(spk_ctx *c, int mx, int my, int mz, const double *kappa, int kappa_mem, int apply_bc, double *f_dev);
void assemble_laplace_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, const double *kappa, int kappa_mem,
                          int apply_bc, int32_t *rowptr, int32_t *colidx, double *val, double *f);
int laplace_mz3(int mx, int my, int mz);
// A10 of the reference's own discretisation (SpkAssembleOperator_Constraints[3D]) written on the device for the rows A00
// gave this rank, then set_block(A10)'s chain; g into g_dev (m values, or null).  mz == 0: the 2-D block.
// assemble_constraints_csr: the kernels' arrays of any slab back on the host (a test hook); host_constraints_csr: the same
// arrays by the host chain, without a GPU.
void set_block_constraints(spk_ctx *c, int mx, int my, int mz, double *g_dev);
void assemble_constraints_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                              int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                              int64_t winptr_cap);
void host_constraints_csr(int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                          int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                          int64_t winptr_cap);

// The host side of the frame MINRES and pipelined CG share (spk_minres.cpp, spk_pipecg.cpp).  The host only ENQUEUES
// iterations, each gated by the state's `done` word; the scalar steps run on the device.  The state is copied into a
// pinned slot behind that slot's event and looked at once per chunk of iterations while the next chunk is already queued.
template <class S>
struct SolverFrame {
    spk_ctx *c;
    SolverWork &w;
    int ns;                  // sums of a pass
    S *st;                   // the state (device)
    double *out, *hist;      // reduced sums, residual history (device)
    int32_t hist_cap;
    bool one;                // one rank: the scalar step runs in the finishing workgroup of the pass
    bool look_now;           // opts.check_every > 0: a chunk's verdict is read at its end
    int64_t chunk;           // iterations per look at the state
    int64_t pending = -1;    // the slot whose verdict is still to be read
    std::chrono::steady_clock::time_point t0;

    SolverFrame(spk_ctx *c_, SolverWork &w_, int nvec, int ns_, const spk_opts &o, int64_t default_chunk)
        : c(c_), w(w_), ns(ns_), look_now(o.check_every > 0), chunk(o.check_every > 0 ? o.check_every : default_chunk)
    {
        c->ensure_scratch();
        c->ensure_vectors();
        hist_cap = (int32_t)std::min<int64_t>((int64_t)std::max(o.max_it, 0) + 2, 1 << 22);
        w.ensure(c->ld, nvec, hist_cap, sizeof(S));
        st = (S *)w.state.p;
        out = w.out.p;
        hist = w.hist.p;
        one = c->comm->size() == 1;
        SPK_HIP(hipStreamSynchronize(c->stream));
        t0 = std::chrono::steady_clock::now();
    }
    double *vec(int i) const { return w.vec.p + (size_t)c->ld * i; }
    const int32_t *done() const { return &st->ks.done; }
    // the step `mode` in the kernel of a pass (one rank; several: after); mode < 0: none
    k::Step<S> step(int mode) const { return k::Step<S>{st, one ? mode : -1, hist, hist_cap}; }
    // several ranks: the all-reduce of the pass's sums (default: out), then the step `mode`
    void after(int mode, const int32_t *gate, double *sums = nullptr) const
    {
        if (one) return;
        if (!sums) sums = out;
        c->comm->allreduce_sum(sums, ns, c->stream);
        k::state_scalar(k::Step<S>{st, mode, hist, hist_cap}, sums, gate, c->stream);
    }
    // a (re)start: the state as it is now
    S start()
    {
        pending = -1;
        report(0);
        return look(0);
    }
    // after iteration j of a recurrence of at most cap iterations: at a chunk boundary the state is reported and a verdict
    // read (look_now: this chunk's; otherwise the previous chunk's, while this one runs).  true: the solve is done
    bool chunk_end(int64_t j, int64_t cap)
    {
        if (j % chunk != 0 && j != cap) return false;
        const int slot = (int)((j / chunk) & 1);
        report(slot);
        if (look_now) return look(slot).ks.done != 0;
        const bool seen = pending >= 0 && look((int)pending).ks.done != 0;
        pending = slot;
        return seen;
    }
    void finish(const S &s, spk_result *res, double *history, int32_t history_cap) const
    {
        finish_solve(c, s.ks, s.starts, t0, hist, hist_cap, res, history, history_cap);
    }

private:
    void report(int slot)
    {
        SPK_HIP(hipMemcpyAsync((S *)w.pin + slot, st, sizeof(S), hipMemcpyDeviceToHost, c->stream));
        SPK_HIP(hipEventRecord(w.ev[slot], c->stream));
    }
    S look(int slot)
    {
        SPK_HIP(hipEventSynchronize(w.ev[slot]));
        return ((S *)w.pin)[slot];
    }
};
}  // namespace spk
