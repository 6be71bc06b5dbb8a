// spk_ksp.cpp -- KSP-shaped host facade over the C ABI (see include/spk_ksp.h):
// the call sequence of /root/reference/src/SaddlePointProblem.c:65-72 with the
// option names KSPSetFromOptions (:67) would read.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spk_ksp.h"

namespace {
// -ksp_type: an index into kKspTypes (pipecgrr is pipecg's rules plus residual replacement)
enum { kFgmres, kMinres, kPipecg, kPipecgrr };
const char *const kKspTypes[] = {"fgmres", "minres", "pipecg", "pipecgrr"};
}  // namespace

struct SpkKSP_s {
    spk_ctx *ctx = nullptr;  // created on first use so that option handling needs no GPU
    int device = 0;
    spk_opts opts;
    int32_t pc_type = SPK_PC_NONE, schur_fact = SPK_SCHUR_FULL;
    int32_t inner_sweeps = 0;  // -fieldsplit_0_ksp_max_it with -fieldsplit_0_ksp_type richardson
    double inner_omega = 1.0;  // -fieldsplit_0_ksp_richardson_scale
    bool inner_richardson = false;
    // smoothed-aggregation multigrid: -pc_type gamg (K = A) and -fieldsplit_0_pc_type gamg (the Schur split's A^-1),
    // each with its own options (amg[0]: -pc_gamg_* / -pc_mg_* / -mg_levels_*, amg[1]: the same with -fieldsplit_0_)
    bool pc_gamg = false, split0_gamg = false;
    int32_t schur_pre = SPK_SCHUR_PRE_SELFP_DIAG;   // -pc_fieldsplit_schur_precondition selfp | full
    int split1_pc = -1;                             // -fieldsplit_1_pc_type: 0 jacobi, 1 cholesky | lu, -1 follows schur_pre
    spk_amg_opts amg[2];
    bool amg_reuse[2] = {false, false};             // -pc_gamg_reuse_interpolation, plain and with -fieldsplit_0_
    // -pc_type mg / -fieldsplit_0_pc_type mg: the same slots and option sets with amg[].coarsening = SPK_AMG_COARSEN_GRID;
    // the node grid comes from SpkKSPSetOperatorsLaplace / ...3D or SpkKSPSetGrid (mz = 1 in 2-D; 0: not known)
    int32_t grid[3] = {0, 0, 0};
    bool have_ops = false, is_setup = false, has_B = false;
    bool ops_device = false;   // the last KSPSetOperators assembled A00 on the device (-ksp_view)
    bool ops_device_3d = false;   // ... with the 3-D generator's kernel
    bool ops_device_B = false;    // ... and wrote the constraint block there too (SpkKSPSetOperatorsLaplaceConstrained[3D])
    int32_t n_rows_B = 0;   // m (-ksp_view)
    // PETSc's own defaults (-ksp_type gmres with left preconditioning, -pc_type ilu / bjacobi+ilu) are
    // not implemented here: a run that leaves them unset must be refused, not silently changed
    int ksp_type = -1;                            // -ksp_type (kFgmres ...), -1: not given
    bool pc_type_given = false;
    double rr_tau = SPK_PIPECGRR_TAU_DEFAULT;     // -spk_pipecgrr_tau
    int32_t replacements = 0;                     // of the last pipecgrr solve (-ksp_view)
    bool pc_side_right = false;                   // -ksp_pc_side right was given
    int32_t norm_type = SPK_NORM_UNPRECONDITIONED;   // -ksp_norm_type
    bool monitor = false, print_reason = false, view = false;
    spk_result result;
    std::vector<double> history;
    std::string err;
};

namespace {
int set_err(SpkKSP k, int code, const std::string &m)
{
    k->err = m;
    return code;
}
int from_ctx(SpkKSP k, int code)
{
    if (code != SPK_OK) k->err = spk_last_error(k->ctx);
    return code;
}
bool parse_double(const char *s, double *v)
{
    char *e = nullptr;
    *v = std::strtod(s, &e);
    return e && e != s && *e == 0;
}
bool parse_int(const char *s, int32_t *v)
{
    char *e = nullptr;
    const long l = std::strtol(s, &e, 10);
    *v = (int32_t)l;
    return e && e != s && *e == 0;
}
bool parse_bool(const char *s, bool *v)
{
    const std::string t(s);
    if (t == "1" || t == "true" || t == "yes" || t == "on") { *v = true; return true; }
    if (t == "0" || t == "false" || t == "no" || t == "off") { *v = false; return true; }
    return false;
}
// the multigrid options (key without its -fieldsplit_0_ prefix); *handled = false: not one of them
int parse_amg(SpkKSP k, spk_amg_opts &o, bool &reuse, const std::string &full, const std::string &key, const char *val, bool *handled)
{
    *handled = true;
    auto need = [&](const char *what) -> int { return set_err(k, SPK_ERR_ARG, "option " + full + " needs " + what); };
    int32_t iv = 0;
    double dv = 0.0;
    if (key == "-pc_gamg_threshold") {
        if (!val || !parse_double(val, &dv) || !(dv >= 0.0)) return need("a real >= 0");
        o.threshold = dv;
    } else if (key == "-pc_gamg_agg_nsmooths") {
        if (!val || !parse_int(val, &iv) || iv < 0 || iv > 4) return need("an integer 0..4");
        o.nsmooths = iv;
    } else if (key == "-pc_gamg_coarse_eq_limit") {
        if (!val || !parse_int(val, &iv) || iv < 1) return need("an integer >= 1");
        o.coarse_eq_limit = iv;
    } else if (key == "-pc_gamg_reuse_interpolation") {
        bool b = true;   // (given without a value: on)
        if (val && !parse_bool(val, &b)) return need("a boolean");
        reuse = b;
    } else if (key == "-pc_mg_levels") {
        if (!val || !parse_int(val, &iv) || iv < 1 || iv > SPK_AMG_MAX_LEVELS) return need("an integer 1..16");
        o.max_levels = iv;
    } else if (key == "-mg_levels_ksp_type") {
        if (!val) return need("a type");
        const std::string v(val);
        if (v == "chebyshev") o.smoother = SPK_AMG_CHEBYSHEV;
        else if (v == "richardson") o.smoother = SPK_AMG_RICHARDSON;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (chebyshev | richardson)");
    } else if (key == "-mg_levels_ksp_max_it") {
        if (!val || !parse_int(val, &iv) || iv < 1 || iv > 64) return need("an integer 1..64");
        o.smooth_its = iv;
    } else if (key == "-mg_levels_ksp_richardson_scale") {
        if (!val || !parse_double(val, &dv) || !(dv > 0.0)) return need("a real > 0");
        o.richardson_scale = dv;
    } else if (key == "-mg_levels_ksp_chebyshev_esteig") {
        double e[4];
        const char *p = val;
        for (int i = 0; i < 4; ++i) {
            char *end = nullptr;
            e[i] = p ? std::strtod(p, &end) : 0.0;
            if (!p || end == p || !std::isfinite(e[i]) || (i < 3 ? *end != ',' : *end != 0)) return need("four reals a,b,c,d");
            p = end + 1;
        }
        std::memcpy(o.esteig, e, sizeof e);
    } else if (key == "-spk_gamg_setup") {
        if (!val) return need("host or device");
        const std::string v(val);
        if (v == "host") o.setup = SPK_AMG_SETUP_HOST;
        else if (v == "device") o.setup = SPK_AMG_SETUP_DEVICE;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (host | device)");
    } else if (key == "-pc_mg_galerkin") {   // Galerkin is the only coarse operator here
        if (val && std::string(val) != "both" && std::string(val) != "pmat")
            return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + val + " is not supported (no value | both | pmat: every "
                                                   "coarse operator is the Galerkin product)");
    } else if (key == "-spk_mg_transfer") {
        if (!val) return need("matrixfree or stored");
        const std::string v(val);
        if (v == "matrixfree") o.transfer = SPK_AMG_TRANSFER_MATRIX_FREE;
        else if (v == "stored") o.transfer = SPK_AMG_TRANSFER_STORED;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (matrixfree | stored)");
    } else if (key == "-spk_mg_sides") {
        if (!val) return need("odd or any");
        const std::string v(val);
        if (v == "odd") o.sides = SPK_AMG_SIDES_ODD;
        else if (v == "any") o.sides = SPK_AMG_SIDES_ANY;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (odd | any)");
    } else if (key == "-spk_mg_galerkin") {
        if (!val) return need("products or stencil");
        const std::string v(val);
        if (v == "products") o.galerkin = SPK_AMG_GALERKIN_PRODUCTS;
        else if (v == "stencil") o.galerkin = SPK_AMG_GALERKIN_STENCIL;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (products | stencil)");
    } else if (key == "-spk_mg_operator") {
        if (!val) return need("csr or stencil");
        const std::string v(val);
        if (v == "csr") o.op = SPK_AMG_OPERATOR_CSR;
        else if (v == "stencil") o.op = SPK_AMG_OPERATOR_STENCIL;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (csr | stencil)");
    } else if (key == "-spk_amg_lanczos") {
        if (!val) return need("stepwise or resident");
        const std::string v(val);
        if (v == "stepwise") o.lanczos = SPK_AMG_LANCZOS_STEPWISE;
        else if (v == "resident") o.lanczos = SPK_AMG_LANCZOS_RESIDENT;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (stepwise | resident)");
    } else if (key == "-spk_mg_precision") {
        if (!val) return need("double or single");
        const std::string v(val);
        if (v == "double") o.precision = SPK_AMG_PRECISION_DOUBLE;
        else if (v == "single") o.precision = SPK_AMG_PRECISION_SINGLE;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (double | single)");
    } else if (key == "-spk_mg_cycle") {
        if (!val) return need("v or w");
        const std::string v(val);
        if (v == "v") o.cycle = SPK_AMG_CYCLE_V;
        else if (v == "w") o.cycle = SPK_AMG_CYCLE_W;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (v | w)");
    } else if (key == "-spk_mg_tail") {
        if (!val) return need("auto, launches or fused");
        const std::string v(val);
        if (v == "auto") o.tail = SPK_AMG_TAIL_AUTO;
        else if (v == "launches") o.tail = SPK_AMG_TAIL_LAUNCHES;
        else if (v == "fused") o.tail = SPK_AMG_TAIL_FUSED;
        else return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + v + " is not supported (auto | launches | fused)");
    } else if (key == "-spk_mg_tail_rows") {
        if (!val || !parse_int(val, &iv) || iv < 0) return need("an integer >= 0 (0: the default)");
        o.tail_rows = iv;
    } else if (key == "-pc_mg_cycle_type") {   // PETSc's name: v is what runs anyway; the W-cycle is -spk_mg_cycle w
        if (!val) return need("v (the W-cycle is -spk_mg_cycle w)");
        if (std::string(val) != "v")
            return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + val + " is not supported (v) -- the W-cycle is " +
                                                   (full.rfind("-fieldsplit_0_", 0) == 0 ? "-fieldsplit_0_spk_mg_cycle w" : "-spk_mg_cycle w"));
    } else if (key == "-mg_levels_pc_type") {
        if (!val) return need("a type");
        if (std::string(val) != "jacobi") return set_err(k, SPK_ERR_UNSUPPORTED, "option " + full + " " + val + " is not supported (jacobi)");
    } else if (key.rfind("-mg_", 0) == 0) {
        return set_err(k, SPK_ERR_UNSUPPORTED, "unknown solver option " + full);
    } else {
        *handled = false;
    }
    return SPK_OK;
}
}  // namespace

extern "C" {

const char *SpkKSPConvergedReasonName(int32_t r)
{
    switch (r) {
    case SPK_CONVERGED_RTOL: return "CONVERGED_RTOL";
    case SPK_CONVERGED_ATOL: return "CONVERGED_ATOL";
    case SPK_CONVERGED_ITS: return "CONVERGED_ITS";
    case SPK_CONVERGED_HAPPY_BREAKDOWN: return "CONVERGED_HAPPY_BREAKDOWN";
    case SPK_DIVERGED_NULL: return "DIVERGED_NULL";
    case SPK_DIVERGED_ITS: return "DIVERGED_ITS";
    case SPK_DIVERGED_DTOL: return "DIVERGED_DTOL";
    case SPK_DIVERGED_BREAKDOWN: return "DIVERGED_BREAKDOWN";
    case SPK_DIVERGED_INDEFINITE_PC: return "DIVERGED_INDEFINITE_PC";
    case SPK_DIVERGED_NANORINF: return "DIVERGED_NANORINF";
    case SPK_DIVERGED_INDEFINITE_MAT: return "DIVERGED_INDEFINITE_MAT";
    case SPK_ITERATING: return "CONVERGED_ITERATING";
    default: return "UNKNOWN";
    }
}

int SpkKSPCreate(int device, SpkKSP *out)
{
    if (!out) return SPK_ERR_ARG;
    *out = nullptr;
    SpkKSP k = new SpkKSP_s();
    spk_default_opts(&k->opts);
    spk_default_amg_opts(&k->amg[0]);
    spk_default_amg_opts(&k->amg[1]);
    std::memset(&k->result, 0, sizeof k->result);
    k->device = device;
    *out = k;
    return SPK_OK;
}

static int ensure_ctx(SpkKSP k)
{
    if (k->ctx) return SPK_OK;
    const int rc = spk_create(&k->ctx, k->device);
    if (rc != SPK_OK) k->err = spk_last_error(nullptr);
    return rc;
}

int SpkKSPDestroy(SpkKSP *k)
{
    if (!k || !*k) return SPK_OK;
    if ((*k)->ctx) spk_destroy((*k)->ctx);
    delete *k;
    *k = nullptr;
    return SPK_OK;
}

const char *SpkKSPGetError(SpkKSP k) { return k ? k->err.c_str() : "null KSP"; }

int SpkKSPSetCommRCCL(SpkKSP k, int rank, int nranks, const void *id128)
{
    if (!k) return SPK_ERR_ARG;
    if (const int rc = ensure_ctx(k)) return rc;
    if (const int rc = spk_comm_init_rccl(k->ctx, rank, nranks, id128)) return from_ctx(k, rc);
    // peer-store collectives on top (falls back to RCCL collectively; see include/spk.h)
    return from_ctx(k, spk_comm_enable_peer(k->ctx, nullptr));
}

// what follows A00 in KSPSetOperators on either route: the constraint block, then the facade's state
static int set_operators_tail(SpkKSP k, const SpkMatCSR *B, bool device, int device_B_rows = 0)
{
    int rc = SPK_OK;
    k->ops_device = device;
    k->ops_device_B = device_B_rows > 0;
    k->has_B = false;
    k->n_rows_B = 0;
    if (device_B_rows > 0) {   // (spk_set_block_constraints has run)
        k->has_B = true;
        k->n_rows_B = device_B_rows;
    } else if (B) {
        rc = spk_set_block(k->ctx, SPK_BLOCK_A10, 0, B->nrows_local, B->ncols_global, B->rowptr, B->colidx, B->val);
        if (rc != SPK_OK) return from_ctx(k, rc);
        k->has_B = B->nrows_local > 0;
        k->n_rows_B = B->nrows_local;
    }
    k->have_ops = true;
    k->is_setup = false;
    return SPK_OK;
}

int SpkKSPSetOperators(SpkKSP k, const SpkMatCSR *A, const SpkMatCSR *B)
{
    if (!k) return SPK_ERR_ARG;
    if (!A) return set_err(k, SPK_ERR_ARG, "KSPSetOperators: null operator");
    int rc = ensure_ctx(k);
    if (rc != SPK_OK) return rc;
    rc = spk_set_block(k->ctx, SPK_BLOCK_A00, A->row_begin, A->nrows_local, A->ncols_global, A->rowptr, A->colidx, A->val);
    if (rc != SPK_OK) return from_ctx(k, rc);
    return set_operators_tail(k, B, false);
}

// A00 assembled on the device, mz == 0: the 2-D grid (spk_set_block_laplace), else the 3-D generator's
// device_B: the generator's constraint block written on the device as well (spk_set_block_constraints), g behind f in f_host
static int set_operators_device(SpkKSP k, int mx, int my, int mz, const double *kappa, const SpkMatCSR *B, double *f_host,
                                bool device_B = false)
{
    if (!k) return SPK_ERR_ARG;
    int rc = ensure_ctx(k);
    if (rc != SPK_OK) return rc;
    double *fd = nullptr;
    const bool sane = mx >= 2 && my >= 2 && (mz == 0 || mz >= 2);
    const int64_t cap = sane ? (mz ? (int64_t)3 * mx * my * mz : (int64_t)2 * mx * my) : 0;   // (the rank's rows are at most all of them)
    if (f_host && cap > 0 && cap <= INT32_MAX) {
        rc = spk_vec_create(k->ctx, cap, &fd);
        if (rc != SPK_OK) return from_ctx(k, rc);
    }
    rc = mz ? spk_set_block_laplace3d(k->ctx, mx, my, mz, kappa, SPK_MEM_HOST, 1, fd)
            : spk_set_block_laplace(k->ctx, mx, my, kappa, SPK_MEM_HOST, 1, fd);
    if (rc == SPK_OK && fd) {
        int32_t nl = 0;
        spk_get_sizes(k->ctx, nullptr, &nl, nullptr, nullptr, nullptr);
        rc = spk_vec_get(k->ctx, fd, f_host, nl);
    }
    int32_t nl = 0;
    if (rc == SPK_OK && device_B) {
        const int m = mz ? 6 : 4;
        spk_get_sizes(k->ctx, nullptr, &nl, nullptr, nullptr, nullptr);
        // (fd holds at least m values: a grid the block accepts has more rows than that; g overwrites f there once f is out)
        rc = spk_set_block_constraints(k->ctx, mx, my, mz, fd);
        if (rc == SPK_OK && fd) rc = spk_vec_get(k->ctx, fd, f_host + nl, m);
    }
    if (rc != SPK_OK) from_ctx(k, rc);   // (the message, before the clean-up can replace it)
    if (fd) spk_vec_destroy(k->ctx, fd);
    if (rc != SPK_OK) return rc;
    rc = set_operators_tail(k, B, true, device_B ? (mz ? 6 : 4) : 0);
    if (rc == SPK_OK) k->ops_device_3d = mz != 0;
    if (rc == SPK_OK) k->grid[0] = mx, k->grid[1] = my, k->grid[2] = mz ? mz : 1;
    return rc;
}

int SpkKSPSetGrid(SpkKSP k, int mx, int my, int mz)
{
    if (!k) return SPK_ERR_ARG;
    if (mx < 2 || my < 2 || mz < 0)
        return set_err(k, SPK_ERR_ARG, "KSPSetGrid: " + std::to_string(mx) + " x " + std::to_string(my) + " x " + std::to_string(mz) +
                                       " nodes (at least 2 x 2; mz = 1, or 0, in 2-D)");
    k->grid[0] = mx, k->grid[1] = my, k->grid[2] = mz ? mz : 1;
    k->is_setup = false;
    return SPK_OK;
}

int SpkKSPSetOperatorsLaplace(SpkKSP k, int mx, int my, const double *kappa, const SpkMatCSR *B, double *f_host)
{
    return set_operators_device(k, mx, my, 0, kappa, B, f_host);
}

int SpkKSPSetOperatorsLaplace3D(SpkKSP k, int mx, int my, int mz, const double *kappa, const SpkMatCSR *B, double *f_host)
{
    if (k && mz == 0) return set_err(k, SPK_ERR_ARG, "KSPSetOperatorsLaplace3D: mz = 0 (at least 2 x 2 x 2 nodes)");
    return set_operators_device(k, mx, my, mz, kappa, B, f_host);
}

int SpkKSPSetOperatorsLaplaceConstrained(SpkKSP k, int mx, int my, const double *kappa, double *rhs_host)
{
    return set_operators_device(k, mx, my, 0, kappa, nullptr, rhs_host, true);
}

int SpkKSPSetOperatorsLaplaceConstrained3D(SpkKSP k, int mx, int my, int mz, const double *kappa, double *rhs_host)
{
    if (k && mz == 0) return set_err(k, SPK_ERR_ARG, "KSPSetOperatorsLaplaceConstrained3D: mz = 0 (at least 3 x 3 x 3 nodes)");
    return set_operators_device(k, mx, my, mz, kappa, nullptr, rhs_host, true);
}

int SpkKSPSetFromOptions(SpkKSP k, int argc, const char *const *argv)
{
    if (!k) return SPK_ERR_ARG;
    if (argc > 0 && !argv) return set_err(k, SPK_ERR_ARG, "KSPSetFromOptions: null argv");
    for (int i = 0; i < argc; ++i) {
        const std::string key = argv[i] ? argv[i] : "";
        if (key.empty() || key[0] != '-') continue;
        const bool has_val = (i + 1 < argc) && argv[i + 1] && !(argv[i + 1][0] == '-' && !(argv[i + 1][1] >= '0' && argv[i + 1][1] <= '9') && argv[i + 1][1] != '.');
        const char *val = has_val ? argv[i + 1] : nullptr;
        auto need = [&](const char *what) -> int {
            return set_err(k, SPK_ERR_ARG, "option " + key + " needs " + what);
        };
        auto bad = [&]() -> int { return set_err(k, SPK_ERR_UNSUPPORTED, "option " + key + " " + (val ? val : "") + " is not supported"); };
        bool flag = true;
        {   // multigrid options, plain or with the first split's prefix
            const bool split0 = key.rfind("-fieldsplit_0_", 0) == 0;
            const std::string sub = split0 ? "-" + key.substr(14) : key;
            bool handled = false;
            const int rc = parse_amg(k, k->amg[split0 ? 1 : 0], k->amg_reuse[split0 ? 1 : 0], key, sub, val, &handled);
            if (rc != SPK_OK) return rc;
            if (handled) continue;
        }
        if (key == "-ksp_type") {
            if (!val) return need("a type");
            int t = kFgmres;
            while (t <= kPipecgrr && std::strcmp(val, kKspTypes[t]) != 0) ++t;
            if (t > kPipecgrr) return bad();
            k->ksp_type = t;
        } else if (key == "-spk_pipecgrr_tau") {
            double dv = 0.0;
            if (!val || !parse_double(val, &dv) || !(dv >= 0.0) || !std::isfinite(dv)) return need("a finite real >= 0");
            k->rr_tau = dv;
        } else if (key == "-ksp_rtol") {
            if (!val || !parse_double(val, &k->opts.rtol)) return need("a real");
        } else if (key == "-ksp_atol") {
            if (!val || !parse_double(val, &k->opts.abstol)) return need("a real");
        } else if (key == "-ksp_divtol") {
            if (!val || !parse_double(val, &k->opts.dtol)) return need("a real");
        } else if (key == "-ksp_max_it") {
            if (!val || !parse_int(val, &k->opts.max_it)) return need("an integer");
        } else if (key == "-ksp_gmres_restart") {
            if (!val || !parse_int(val, &k->opts.restart)) return need("an integer");
        } else if (key == "-ksp_initial_guess_nonzero") {
            if (val && !parse_bool(val, &flag)) return need("a boolean");
            k->opts.guess_nonzero = flag;
        } else if (key == "-ksp_gmres_classicalgramschmidt") {
            k->opts.orthog = SPK_ORTHOG_CGS;
        } else if (key == "-ksp_gmres_modifiedgramschmidt") {
            k->opts.orthog = SPK_ORTHOG_MGS;
        } else if (key == "-ksp_gmres_cgs_refinement_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "never" || v == "refine_never") k->opts.cgs_refine = SPK_REFINE_NEVER;
            else if (v == "ifneeded" || v == "refine_ifneeded") k->opts.cgs_refine = SPK_REFINE_IFNEEDED;
            else if (v == "always" || v == "refine_always") k->opts.cgs_refine = SPK_REFINE_ALWAYS;
            else return bad();
        } else if (key == "-ksp_pc_side") {
            if (!val) return need("a side");
            if (std::string(val) != "right") return bad();
            k->pc_side_right = true;   // fgmres's side; pipecg refuses it at KSPSetUp
        } else if (key == "-ksp_norm_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "unpreconditioned") k->norm_type = SPK_NORM_UNPRECONDITIONED;
            else if (v == "natural") k->norm_type = SPK_NORM_NATURAL;   // minres / pipecg only (checked at KSPSetUp)
            else return bad();
        } else if (key == "-ksp_monitor" || key == "-ksp_monitor_true_residual") {
            k->monitor = true;
        } else if (key == "-ksp_converged_reason") {
            k->print_reason = true;
        } else if (key == "-ksp_view") {
            k->view = true;
        } else if (key == "-pc_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "none") k->pc_type = SPK_PC_NONE;
            else if (v == "jacobi") k->pc_type = SPK_PC_JACOBI;
            else if (v == "fieldsplit") k->pc_type = SPK_PC_SCHUR;
            else if (v == "gamg" || v == "mg") k->pc_type = SPK_PC_JACOBI;   // Jacobi's slot, M^-1 = one V-cycle (K = A only)
            else return bad();
            k->pc_gamg = v == "gamg" || v == "mg";
            if (k->pc_gamg) k->amg[0].coarsening = v == "mg" ? SPK_AMG_COARSEN_GRID : SPK_AMG_COARSEN_AGGREGATION;
            k->pc_type_given = true;
        } else if (key == "-pc_fieldsplit_type") {
            if (!val) return need("a type");
            if (std::string(val) != "schur") return bad();
        } else if (key == "-pc_fieldsplit_schur_fact_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "diag") k->schur_fact = SPK_SCHUR_DIAG;
            else if (v == "lower") k->schur_fact = SPK_SCHUR_LOWER;
            else if (v == "upper") k->schur_fact = SPK_SCHUR_UPPER;
            else if (v == "full") k->schur_fact = SPK_SCHUR_FULL;
            else return bad();
        } else if (key == "-pc_fieldsplit_schur_precondition") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "selfp") k->schur_pre = SPK_SCHUR_PRE_SELFP_DIAG;
            else if (v == "full") k->schur_pre = SPK_SCHUR_PRE_FULL;   // the exact S of a few rows, dense (checked at KSPSetUp)
            else return bad();
        } else if (key == "-pc_fieldsplit_detect_saddle_point") {
            /* implied by the nest */
        } else if (key == "-fieldsplit_0_ksp_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "richardson") k->inner_richardson = true;   // FP32 Jacobi-Richardson inner solve
            else if (v == "preonly") k->inner_richardson = false;
            else return bad();
        } else if (key == "-fieldsplit_0_ksp_max_it" || key == "-spk_inner_sweeps") {
            if (!val || !parse_int(val, &k->inner_sweeps)) return need("an integer");
            if (key == "-spk_inner_sweeps") k->inner_richardson = k->inner_sweeps > 0;
        } else if (key == "-fieldsplit_0_ksp_richardson_scale" || key == "-spk_inner_omega") {
            if (!val || !parse_double(val, &k->inner_omega)) return need("a real");
        } else if (key == "-fieldsplit_1_ksp_type") {
            if (!val) return need("a type");
            if (std::string(val) != "preonly") return bad();
        } else if (key == "-fieldsplit_0_pc_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "jacobi") k->split0_gamg = false;
            else if (v == "gamg" || v == "mg") k->split0_gamg = true;
            else return bad();
            if (k->split0_gamg) k->amg[1].coarsening = v == "mg" ? SPK_AMG_COARSEN_GRID : SPK_AMG_COARSEN_AGGREGATION;
        } else if (key == "-fieldsplit_1_pc_type") {
            if (!val) return need("a type");
            const std::string v(val);
            if (v == "jacobi") k->split1_pc = 0;
            else if (v == "cholesky" || v == "lu") k->split1_pc = 1;   // both: the dense factor of S
            else return bad();
        } else if (key == "-spk_single_reduce") {
            if (!val || !parse_int(val, &k->opts.single_reduce)) return need("an integer (0 off, 1 on)");
        } else if (key == "-spk_iteration_form") {
            if (!val || !parse_int(val, &k->opts.iteration_form) || k->opts.iteration_form < 0 || k->opts.iteration_form > SPK_ITER_LAST)
                return need("an integer 0..7 (0 automatic, 1 four launches per iteration, 5 three launches on an un-normalised basis, "
                            "6 one launch per restart cycle, 7 as 5 with MDot and MAXPY in one launch; 2..4 are accepted and run as 5)");
        } else if (key == "-spk_basis_precision") {
            // how fgmres stores its Krylov basis (spk_opts.basis_precision); the solve refuses what single cannot run
            const std::string v(val ? val : "");
            if (v == "double") k->opts.basis_precision = SPK_BASIS_DOUBLE;
            else if (v == "single") k->opts.basis_precision = SPK_BASIS_SINGLE;
            else return need("double | single");
        } else if (key == "-spk_check_every") {
            if (!val || !parse_int(val, &k->opts.check_every)) return need("an integer");
        } else if (key.rfind("-ksp_", 0) == 0 || key.rfind("-pc_", 0) == 0 || key.rfind("-fieldsplit_", 0) == 0) {
            return set_err(k, SPK_ERR_UNSUPPORTED, "unknown solver option " + key);
        }
    }
    k->is_setup = false;
    return SPK_OK;
}

// -fieldsplit_1_pc_type as it resolves: given, or following -pc_fieldsplit_schur_precondition
static int split1_dense(SpkKSP k) { return k->split1_pc >= 0 ? k->split1_pc : (k->schur_pre == SPK_SCHUR_PRE_FULL ? 1 : 0); }

// which multigrid option set the selected preconditioner uses: 0 (-pc_type gamg), 1 (-fieldsplit_0_pc_type gamg), -1 none
static int amg_active(SpkKSP k)
{
    if (k->pc_type == SPK_PC_JACOBI && k->pc_gamg) return 0;
    if (k->pc_type == SPK_PC_SCHUR && k->split0_gamg) return 1;
    return -1;
}

int SpkKSPSetUp(SpkKSP k)
{
    if (!k) return SPK_ERR_ARG;
    if (k->ksp_type < 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: no -ksp_type given; PETSc's default (gmres, left preconditioning) is "
                                               "not implemented -- pass -ksp_type fgmres (or -ksp_type minres for a symmetric "
                                               "preconditioner)");
    if (!k->pc_type_given)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: no -pc_type given; PETSc's default (ilu, bjacobi+ilu in parallel) is "
                                               "not implemented -- pass -pc_type jacobi | fieldsplit | gamg | mg | none");
    // KSP / PC compatibility: option checks only, no GPU needed
    const bool minres = k->ksp_type == kMinres, pipecgrr = k->ksp_type == kPipecgrr;
    const bool pipecg = k->ksp_type == kPipecg || pipecgrr;
    if (k->ksp_type == kFgmres && k->norm_type == SPK_NORM_NATURAL)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_norm_type natural is for -ksp_type minres / pipecg; fgmres tests "
                                               "the unpreconditioned norm -- drop -ksp_norm_type natural or pass -ksp_type minres");
    const std::string pt = kKspTypes[k->ksp_type];
    if (pipecg && k->pc_type == SPK_PC_SCHUR)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type " + pt + " is for K = A and takes -pc_type none | jacobi | "
                                               "gamg; the Schur fieldsplit belongs to the saddle matrix, which is indefinite -- "
                                               "pass -ksp_type minres (diag) or fgmres");
    if (pipecg && k->inner_richardson && k->inner_sweeps > 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type " + pt + " needs a symmetric preconditioner and the FP32 "
                                               "inner sweeps are not -- drop -fieldsplit_0_ksp_type richardson / "
                                               "-spk_inner_sweeps, or pass -ksp_type fgmres");
    if (pipecg && k->pc_side_right)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type " + pt + " preconditions from the left only (as PETSc's "
                                               "KSP" + (pipecgrr ? "PIPECGRR" : "PIPECG") + ") -- drop -ksp_pc_side right");
    if (minres && k->pc_type == SPK_PC_SCHUR && k->schur_fact != SPK_SCHUR_DIAG)
        return set_err(k, SPK_ERR_UNSUPPORTED, std::string("KSPSetUp: -ksp_type minres needs a symmetric positive definite "
                       "preconditioner and the Schur ") + (k->schur_fact == SPK_SCHUR_LOWER ? "lower" : k->schur_fact == SPK_SCHUR_UPPER ?
                       "upper" : "full") + " factorisation is not symmetric -- pass -pc_fieldsplit_schur_fact_type diag, or -ksp_type fgmres");
    if (minres && k->pc_type != SPK_PC_NONE && k->inner_richardson && k->inner_sweeps > 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type minres needs a symmetric preconditioner and the FP32 inner "
                                               "sweeps are not -- drop -fieldsplit_0_ksp_type richardson / -spk_inner_sweeps, or "
                                               "pass -ksp_type fgmres");
    if (k->pc_type == SPK_PC_SCHUR && k->schur_pre == SPK_SCHUR_PRE_FULL && !split1_dense(k))
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -pc_fieldsplit_schur_precondition full keeps the exact Schur complement "
                                               "as a dense matrix and -fieldsplit_1_pc_type jacobi would use its diagonal only "
                                               "-- pass -fieldsplit_1_pc_type cholesky (or lu), or "
                                               "-pc_fieldsplit_schur_precondition selfp");
    if (k->pc_type == SPK_PC_SCHUR && k->schur_pre == SPK_SCHUR_PRE_SELFP_DIAG && split1_dense(k))
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -fieldsplit_1_pc_type cholesky | lu factors a dense Schur complement "
                                               "and -pc_fieldsplit_schur_precondition selfp keeps diag(B diag(A)^-1 B^T) only "
                                               "-- pass -pc_fieldsplit_schur_precondition full, or -fieldsplit_1_pc_type jacobi");
    if (k->pc_type == SPK_PC_SCHUR && k->schur_pre == SPK_SCHUR_PRE_FULL && k->inner_richardson && k->inner_sweeps > 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -pc_fieldsplit_schur_precondition full needs a linear A^-1 and the FP32 "
                                               "inner sweeps are not one in FP64 -- drop -fieldsplit_0_ksp_type richardson / "
                                               "-spk_inner_sweeps, or pass -pc_fieldsplit_schur_precondition selfp");
    const int amg_slot = amg_active(k);
    const bool mg = amg_slot >= 0 && k->amg[amg_slot].coarsening == SPK_AMG_COARSEN_GRID;
    const std::string mgname = mg ? "mg" : "gamg";
    if (minres && amg_slot >= 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type minres with the multigrid preconditioner (" + mgname + ") is not "
                                               "implemented -- pass -ksp_type fgmres");
    if (pipecg && amg_slot >= 0 && k->amg[amg_slot].precision == SPK_AMG_PRECISION_SINGLE)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type " + pt + " needs a symmetric preconditioner and the cycle of "
                                               "-spk_mg_precision single, rounded to FP32 on its levels >= 1, is not exactly one "
                                               "-- pass -ksp_type fgmres, or -spk_mg_precision double");
    if (amg_slot >= 0 && k->inner_richardson && k->inner_sweeps > 0)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: " + mgname + " and the FP32 inner sweeps both stand for A^-1 -- drop "
                                               "-fieldsplit_0_ksp_type richardson / -spk_inner_sweeps, or the " + mgname + " option");
    if (mg && k->grid[0] == 0)
        return set_err(k, SPK_ERR_STATE, std::string("KSPSetUp: ") + (amg_slot ? "-fieldsplit_0_pc_type mg" : "-pc_type mg") +
                       " coarsens a node grid and none is known -- call SpkKSPSetGrid(ksp, mx, my, mz) (the role of KSPSetDM), or "
                       "set the operator with SpkKSPSetOperatorsLaplace / SpkKSPSetOperatorsLaplace3D");
    if (mg) std::memcpy(k->amg[amg_slot].grid, k->grid, sizeof k->grid);
    for (int slot = 0; slot < 2; ++slot)
        if (k->amg_reuse[slot] && slot != amg_slot)
            return set_err(k, SPK_ERR_UNSUPPORTED, std::string("KSPSetUp: ") + (slot ? "-fieldsplit_0_pc_gamg_reuse_interpolation" :
                           "-pc_gamg_reuse_interpolation") + " keeps the prolongators of a multigrid hierarchy and " +
                           (slot ? "-fieldsplit_0_pc_type gamg inside -pc_type fieldsplit" : "-pc_type gamg") +
                           " is not selected -- select it, or drop the option");
    if (!k->have_ops) return set_err(k, SPK_ERR_STATE, "KSPSetUp: KSPSetOperators has not been called");
    if (pipecg && k->has_B)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -ksp_type " + pt + " is for K = A (symmetric positive definite); "
                                               "the saddle matrix [A B^T; B 0] is indefinite -- pass -ksp_type minres");
    if (k->pc_type == SPK_PC_SCHUR && !k->has_B)
        return set_err(k, SPK_ERR_STATE, "KSPSetUp: -pc_type fieldsplit (schur) needs the constraint block B");
    if (k->pc_type == SPK_PC_JACOBI && k->pc_gamg && k->has_B)
        return set_err(k, SPK_ERR_UNSUPPORTED, "KSPSetUp: -pc_type " + mgname + " is for K = A alone; the saddle matrix [A B^T; B 0] "
                                               "(indefinite, zero (1,1) block) is not a multigrid target -- pass -pc_type "
                                               "fieldsplit -fieldsplit_0_pc_type " + mgname);
    int rc = amg_slot >= 0 ? SPK_OK : spk_pc_set_amg(k->ctx, nullptr);
    if (rc != SPK_OK) return from_ctx(k, rc);
    rc = spk_pc_set_inner(k->ctx, k->inner_richardson ? k->inner_sweeps : 0, k->inner_omega);
    if (rc != SPK_OK) return from_ctx(k, rc);
    if (amg_slot >= 0) rc = spk_pc_set_amg(k->ctx, &k->amg[amg_slot]);
    if (rc != SPK_OK) return from_ctx(k, rc);
    rc = spk_pc_set_amg_reuse(k->ctx, amg_slot >= 0 && k->amg_reuse[amg_slot] ? 1 : 0);
    if (rc != SPK_OK) return from_ctx(k, rc);
    rc = spk_pc_set_schur_pre(k->ctx, k->schur_pre);
    if (rc != SPK_OK) return from_ctx(k, rc);
    rc = spk_pc_setup(k->ctx, k->pc_type, k->schur_fact);
    if (rc != SPK_OK) return from_ctx(k, rc);
    k->is_setup = true;
    return SPK_OK;
}

int SpkKSPSolve(SpkKSP k, const double *b, double *x)
{
    if (!k) return SPK_ERR_ARG;
    if (!k->have_ops) return set_err(k, SPK_ERR_STATE, "KSPSolve: KSPSetOperators has not been called");
    if (!b || !x) return set_err(k, SPK_ERR_ARG, "KSPSolve: null vector");
    if (!k->is_setup) {  // KSPSolve calls KSPSetUp itself when needed
        const int rc = SpkKSPSetUp(k);
        if (rc != SPK_OK) return rc;
    }
    const int64_t cap = (int64_t)k->opts.max_it + 2;
    k->history.assign((size_t)(cap > (1 << 22) ? (1 << 22) : cap), 0.0);
    if (k->ksp_type == kPipecgrr) {
        const int rc = spk_pipecgrr_set_tau(k->ctx, k->rr_tau);
        if (rc != SPK_OK) return from_ctx(k, rc);
    }
    double *h = k->history.data();
    const int32_t hn = (int32_t)k->history.size();
    int rc = SPK_OK;
    switch (k->ksp_type) {
    case kMinres: rc = spk_minres(k->ctx, b, x, SPK_MEM_HOST, &k->opts, k->norm_type, &k->result, h, hn); break;
    case kPipecg: rc = spk_pipecg(k->ctx, b, x, SPK_MEM_HOST, &k->opts, k->norm_type, &k->result, h, hn); break;
    case kPipecgrr:
        rc = spk_pipecgrr(k->ctx, b, x, SPK_MEM_HOST, &k->opts, k->norm_type, &k->result, h, hn, &k->replacements);
        break;
    default: rc = spk_fgmres(k->ctx, b, x, SPK_MEM_HOST, &k->opts, &k->result, h, hn);
    }
    if (rc != SPK_OK) return from_ctx(k, rc);
    k->history.resize((size_t)k->result.hist_len);
    if (k->monitor)
        for (size_t i = 0; i < k->history.size(); ++i) std::printf("%3zu KSP Residual norm %.12e\n", i, k->history[i]);
    if (k->print_reason)
        std::printf("Linear solve %s due to %s iterations %d\n", k->result.reason > 0 ? "converged" : "did not converge",
                    SpkKSPConvergedReasonName(k->result.reason), k->result.its);
    if (k->view) {
        std::printf("KSP Object: type %s (MI355X device-resident), ", kKspTypes[k->ksp_type]);
        if (k->ksp_type == kFgmres)
            std::printf("restart=%d, classical Gram-Schmidt, basis stored in %s precision (-spk_basis_precision), ", k->opts.restart,
                        k->opts.basis_precision == SPK_BASIS_SINGLE ? "single" : "double");
        else
            std::printf("%s norm, ", k->norm_type == SPK_NORM_NATURAL ? "natural" : "unpreconditioned");
        std::printf("rtol=%g atol=%g divtol=%g max_it=%d, ", k->opts.rtol, k->opts.abstol, k->opts.dtol, k->opts.max_it);
        const char *pc = k->pc_gamg ? (k->amg[0].coarsening == SPK_AMG_COARSEN_GRID ? "mg" : "gamg") :
                         k->pc_type == SPK_PC_JACOBI ? "jacobi" : "none";
        switch (k->ksp_type) {
        case kFgmres: std::printf("right preconditioning, pc=%d schur_fact=%d\n", k->pc_type, k->schur_fact); break;
        case kMinres: std::printf("pc=%d schur_fact=%d\n", k->pc_type, k->schur_fact); break;
        case kPipecg: std::printf("left preconditioning, pc=%s\n", pc); break;
        default:
            std::printf("left preconditioning, pc=%s, residual replacement tau=%g, replacements=%d\n", pc, k->rr_tau,
                        k->replacements);
        }
    }
    if (k->view) {
        double secs = 0.0;
        spk_get_assembly_seconds(k->ctx, &secs);
        if (k->ops_device && k->ops_device_3d) std::printf("  A00: assembled on the device (SpkKSPSetOperatorsLaplace3D), kernels %.6f s\n", secs);
        else if (k->ops_device) std::printf("  A00: assembled on the device (-spk_assembly device), kernels %.6f s\n", secs);
        else std::printf("  A00: the caller's host arrays (-spk_assembly host)\n");
        if (k->ops_device_B) {
            spk_get_constraints_seconds(k->ctx, &secs);
            std::printf("  A10: written on the device (-spk_constraints device), kernels %.6f s\n", secs);
        }
    }
    if (k->view && k->pc_type == SPK_PC_SCHUR) {
        double secs = 0.0;
        const bool full = k->schur_pre == SPK_SCHUR_PRE_FULL;
        spk_get_schur_setup_seconds(k->ctx, &secs);
        if (full)
            std::printf("  PC fieldsplit: schur_precondition full, m = %d constraint rows, S = B A^-1 B^T dense (%s), "
                        "fieldsplit_1 cholesky, set-up %.6f s\n", (int)k->n_rows_B, amg_active(k) >= 0 ? "A^-1 = the V-cycle" :
                        "A^-1 = diag(A)^-1", secs);
        else
            std::printf("  PC fieldsplit: schur_precondition selfp, m = %d constraint rows, S^ = diag(B diag(A)^-1 B^T), "
                        "fieldsplit_1 jacobi\n", (int)k->n_rows_B);
    }
    if (k->view && amg_active(k) >= 0) {
        spk_amg_info ai;
        if (spk_get_amg_info(k->ctx, &ai) == SPK_OK) {
            const spk_amg_opts &o = k->amg[amg_active(k)];
            const bool grid = ai.coarsening == SPK_AMG_COARSEN_GRID;
            std::printf("  PC %s, %s): %d levels, block size %d, operator complexity %.4f, set-up %.3f s on the %s\n",
                        grid ? "mg (grid coarsening, Galerkin" : "gamg (smoothed aggregation",
                        amg_active(k) ? "fieldsplit_0" : "K = A", ai.levels, ai.block_size, ai.operator_complexity, ai.setup_seconds,
                        ai.setup == SPK_AMG_SETUP_DEVICE ? "device" : "host");
            if (grid)
                std::printf("    smoother %s x %d, transfers %s, sides %s, coarse_eq_limit %d\n",
                            o.smoother == SPK_AMG_CHEBYSHEV ? "chebyshev/jacobi" : "richardson/jacobi", o.smooth_its,
                            o.transfer == SPK_AMG_TRANSFER_STORED ? "stored (CSR)" : "matrix-free",
                            ai.sides == SPK_AMG_SIDES_ANY ? "any (even sides halve too)" : "odd", o.coarse_eq_limit);
            else
                std::printf("    smoother %s x %d, threshold %g, nsmooths %d, coarse_eq_limit %d\n",
                            o.smoother == SPK_AMG_CHEBYSHEV ? "chebyshev/jacobi" : "richardson/jacobi", o.smooth_its, o.threshold,
                            o.nsmooths, o.coarse_eq_limit);
            if (grid)
                std::printf("    coarse operators: %s (-spk_mg_galerkin %s)\n",
                            ai.galerkin == SPK_AMG_GALERKIN_STENCIL ? "the gather on the grid stencil, closed-form patterns"
                                                                    : "the generic sparse products",
                            ai.galerkin == SPK_AMG_GALERKIN_STENCIL ? "stencil" : "products");
            if (grid && ai.op == SPK_AMG_OPERATOR_STENCIL && ai.levels > 2)
                std::printf("    level operators: stencil (-spk_mg_operator stencil): levels 1..%d apply A from their value arrays "
                            "alone, no row pointers or column indices read\n", ai.levels - 2);
            else if (grid && ai.op == SPK_AMG_OPERATOR_STENCIL)
                std::printf("    level operators: stencil (-spk_mg_operator stencil): no level between level 0 and the coarsest\n");
            else if (grid)
                std::printf("    level operators: csr (-spk_mg_operator csr): levels >= 1 as sparse matrices\n");
            if (ai.precision == SPK_AMG_PRECISION_SINGLE)
                std::printf("    precision: single (-spk_mg_precision single): levels 1..%d run in FP32 on rounded copies of their "
                            "values, level 0 and the hierarchy stay FP64\n", ai.levels - 1);
            if (ai.setup == SPK_AMG_SETUP_DEVICE)
                std::printf("    set-up Lanczos: %s (-spk_amg_lanczos %s): %s, %d read-backs in the last set-up\n",
                            ai.lanczos == SPK_AMG_LANCZOS_RESIDENT ? "resident" : "stepwise",
                            ai.lanczos == SPK_AMG_LANCZOS_RESIDENT ? "resident" : "stepwise",
                            ai.lanczos == SPK_AMG_LANCZOS_RESIDENT ? "the scalars stay on the device, one read per level"
                                                                   : "the host reads two sums per step", (int)ai.ritz_readbacks);
            const int tail = ai.tail_first >= 0 ? SPK_AMG_TAIL_FUSED : SPK_AMG_TAIL_LAUNCHES;   // as it resolved on these levels
            std::printf("    cycle %s (-spk_mg_cycle), tail %s (-spk_mg_tail %s), tail_first %d, tail_rows %d%s, tail launches per application %d\n",
                        ai.cycle == SPK_AMG_CYCLE_W ? "w" : "v", tail == SPK_AMG_TAIL_FUSED ? "fused" : "launches",
                        o.tail == SPK_AMG_TAIL_AUTO ? "auto" : o.tail == SPK_AMG_TAIL_FUSED ? "fused" : "launches", ai.tail_first,
                        o.tail_rows > 0 ? o.tail_rows : SPK_AMG_TAIL_ROWS_DEFAULT, o.tail_rows > 0 ? "" : " (default)", ai.tail_launches);
            int32_t refreshed = 0;
            double secs = 0.0;
            if (k->amg_reuse[amg_active(k)] && spk_get_amg_reuse_info(k->ctx, &refreshed, &secs) == SPK_OK)
                std::printf("    reuse_interpolation: the last set-up %s the hierarchy in %.3f s\n", refreshed ? "refreshed" : "built", secs);
            for (int l = 0; l < ai.levels; ++l) {
                char dims[64] = "";
                if (grid) std::snprintf(dims, sizeof dims, " grid %d x %d x %d", ai.dims[l][0], ai.dims[l][1], ai.dims[l][2]);
                std::printf("    level %d:%s rows %d nnz %lld lambda_max %.6g%s\n", l, dims, ai.rows[l], (long long)ai.nnz[l],
                            ai.lambda_max[l], l + 1 == ai.levels ? " (coarse: dense Cholesky inverse)" : "");
            }
        }
    }
    return SPK_OK;
}

int SpkKSPGetIterationNumber(SpkKSP k, int32_t *its) { if (!k || !its) return SPK_ERR_ARG; *its = k->result.its; return SPK_OK; }
int SpkKSPGetConvergedReason(SpkKSP k, int32_t *r) { if (!k || !r) return SPK_ERR_ARG; *r = k->result.reason; return SPK_OK; }
int SpkKSPGetResidualNorm(SpkKSP k, double *v) { if (!k || !v) return SPK_ERR_ARG; *v = k->result.rnorm; return SPK_OK; }
int SpkKSPGetSolveTime(SpkKSP k, double *v) { if (!k || !v) return SPK_ERR_ARG; *v = k->result.solve_seconds; return SPK_OK; }
int SpkKSPGetResidualHistory(SpkKSP k, const double **h, int32_t *n)
{
    if (!k || !h || !n) return SPK_ERR_ARG;
    *h = k->history.data();
    *n = (int32_t)k->history.size();
    return SPK_OK;
}
int SpkKSPGetOptions(SpkKSP k, spk_opts *o, int32_t *pc, int32_t *sf)
{
    if (!k) return SPK_ERR_ARG;
    if (o) *o = k->opts;
    if (pc) *pc = k->pc_type;
    if (sf) *sf = k->schur_fact;
    return SPK_OK;
}
int SpkKSPGetAMGOptions(SpkKSP k, int fieldsplit0, spk_amg_opts *o, int32_t *selected)
{
    if (!k || fieldsplit0 < 0 || fieldsplit0 > 1) return SPK_ERR_ARG;
    if (o) *o = k->amg[fieldsplit0];
    if (selected) *selected = fieldsplit0 ? k->split0_gamg : k->pc_gamg;
    return SPK_OK;
}
int SpkKSPGetAMGReuse(SpkKSP k, int fieldsplit0, int32_t *reuse)
{
    if (!k || !reuse || fieldsplit0 < 0 || fieldsplit0 > 1) return SPK_ERR_ARG;
    *reuse = k->amg_reuse[fieldsplit0] ? 1 : 0;
    return SPK_OK;
}
int SpkKSPGetType(SpkKSP k, const char **type, int32_t *norm_type)
{
    if (!k) return SPK_ERR_ARG;
    if (type) *type = k->ksp_type < 0 ? "" : kKspTypes[k->ksp_type];
    if (norm_type) *norm_type = k->norm_type;
    return SPK_OK;
}
int SpkKSPGetSchurPre(SpkKSP k, int32_t *pre, int32_t *dense_split1)
{
    if (!k) return SPK_ERR_ARG;
    if (pre) *pre = k->schur_pre;
    if (dense_split1) *dense_split1 = split1_dense(k);
    return SPK_OK;
}
int SpkKSPGetContext(SpkKSP k, spk_ctx **c) { if (!k || !c) return SPK_ERR_ARG; *c = k->ctx; return SPK_OK; }

}  // extern "C"
