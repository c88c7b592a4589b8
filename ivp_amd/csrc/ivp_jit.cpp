// ivp_jit.cpp -- user-defined right-hand sides compiled at run time with hiprtc.
//
// The reference lets a user implement `trait IVP { fn ode(&self, x, y, dydx) }` (src/ivp.rs:27-29)
// in host Rust.  On the GPU the right-hand side has to be device code, so the analogue is a HIP
// source snippet defining
//     __device__ void ode(double x, const double* y, double* dydx, const double* p);
// which is spliced in front of the very same kernel templates the built-in functors use
// (ivp_kargs.h + rk_core.h + rk_global.h are embedded in the library as text) and compiled for the
// context's gfx target.  One module per (method, output mode, fp mode) is built on first use.
//
// Jacobian sparsity (ivp_rhs_compile_sparse, 8 < n <= 512): the declared pattern is grouped on the host with the
// reference's first-fit rule (src/python/sparsity.rs:110-154) and travels to the kernel INSIDE the generated source, as
// constant tables next to the problem's functor -- IvpKArgs does not change.  The BDF modules of such a problem carry
//     n_groups, group_of[n] (int16) and hit[n_groups * n] (int16: the column of group g that declares `row`, or -1),
// which BdfG::fd_jac_sparse (bdf_group.h) reads.  Size: 2 n (n_groups + 1) bytes of constant data per code object --
// 3 KB for a tridiagonal system at n = 512, 512 KB in the worst case (n = 512, every column its own group).  The
// on-disk cache keys on the generated source, so two patterns never share an entry.
//
// Banded storage (IVP_RHS_BANDED, ivp_rhs_compile_sparse only): the bandwidths ml = max(row - col), mu = max(col - row) of
// the declared pattern travel the same way, as `enum { SP_ML, SP_MU }` in the functor, and bdf_band.h is spliced in
// behind bdf_group.h.  J and the factors of (I - cJ) are then stored by bands (ivp_rhs_jac_layout), and the BDF chunk
// kernel exists in two residencies -- factors in LDS for the whole launch, or in global memory -- chosen per launch by
// the host (IvpKArgs.lds_lu) and kept as separate modules.  A problem without the flag generates the functor text it
// always did.
// The banded Radau call (ivp_radau_solve_banded*) gets a Radau group module of its own for such a problem: the same tables
// and bandwidths in the functor, bdf_band.h and radau_band.h behind radau_group.h.  The call marks its argument block
// (IVP_RAD_BAND_CALL, ivp_ctx.h); every other Radau module generates the text it always did.
#include "ivp_jit.h"

#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ivp_hip.h"
#include "rk_launch.h"
#include "ivp_ctx.h"
#include "ivp_jit_sources.inc"

#ifndef IVP_MAX_GROUP_N
#define IVP_MAX_GROUP_N 512   // largest n of the wave-per-trajectory kernels (ivp_capi.cpp)
#endif

namespace {

struct JitModule {
    hipModule_t mod = nullptr;
    hipFunction_t init = nullptr, chunk = nullptr, coop = nullptr;   // coop: lane-cooperative chunk kernel (rk_coop.h), optional
    hipFunction_t events = nullptr;   // deferred event refinement (rk_global.h event_kernel_body): full modules of problems with event functions
};

struct JitRhs {
    int device, n, np, ne;
    bool has_jac = false;   // the snippet defines jac(): IVP::jac override (src/ivp.rs:67-107)
    bool has_mass = false;  // the snippet defines mass(): IVP::mass (src/ivp.rs:111-120), read by the Radau DAE call only
    bool has_mass_col = false;   // ... or mass_col(), its column form for the group Radau kernels (8 < n <= 64, radau_group.h)
    std::string ode_source;
    std::string sparsity_source;   // the pattern's tables as device code (empty: no pattern, or the snippet has its own jac_col)
    int n_groups = 0;
    bool banded = false;   // IVP_RHS_BANDED: J and the factors by bands (bdf_band.h)
    int band_ml = 0, band_mu = 0;
    std::string arch;
    std::mutex mu;
    // (device, method, fp_mode, full, ctl): hipModuleLoadData binds a module to the device that is current when it is
    // loaded, so a handle shared by contexts on several GPUs keeps one module per device
    std::map<std::tuple<int, int, int, int, bool, bool, bool, bool>, JitModule> modules;   // ... , lane-cooperative module, banded factors in LDS, banded Radau
    std::string log;
    // the code object of the compile-only check of ivp_jit_compile (key: options + source), kept for the first launch that
    // needs exactly that module: a problem with a mass matrix checks its Radau module, which is also the one it runs
    std::string checked_key;
    std::vector<char> checked_code;
};

std::string join(const char *const *parts)
{
    std::string s;
    for (; *parts; ++parts) s += *parts;
    return s;
}

// The reference's group_columns (src/python/sparsity.rs:110-154), exactly: columns in index order, each into the FIRST
// group none of whose used rows it touches, else into a new group (a column without rows lands in group 0).  The order
// decides which perturbations alias when a caller declares too little, so it is part of the contract.
// Returns IVP_OK, or IVP_ERR_BAD_ARGUMENT with *why set.  hit (optional) receives [n_groups * n].
int group_columns(int n, const int32_t *col_ptr, const int32_t *row_idx, std::vector<int32_t> &groups, int *n_groups,
                  std::vector<int16_t> *hit, const char **why)
{
    static const char *dummy;
    if (!why) why = &dummy;
    if (n <= IVP_MAX_N || n > IVP_MAX_GROUP_N) { *why = "jac_sparsity needs 8 < n <= 512"; return IVP_ERR_BAD_ARGUMENT; }
    if (!col_ptr || col_ptr[0] != 0) { *why = "jac_sparsity: col_ptr[0] must be 0"; return IVP_ERR_BAD_ARGUMENT; }
    for (int c = 0; c < n; ++c)
        if (col_ptr[c + 1] < col_ptr[c]) { *why = "jac_sparsity: col_ptr must be non-decreasing"; return IVP_ERR_BAD_ARGUMENT; }
    if (col_ptr[n] > 0 && !row_idx) { *why = "jac_sparsity: row_idx is NULL"; return IVP_ERR_BAD_ARGUMENT; }
    for (int32_t e = 0; e < col_ptr[n]; ++e)
        if (row_idx[e] < 0 || row_idx[e] >= n) { *why = "jac_sparsity: row index out of range"; return IVP_ERR_BAD_ARGUMENT; }
    groups.assign((size_t)n, 0);
    std::vector<std::vector<int16_t>> used;   // per group: the column that uses the row, or -1
    for (int c = 0; c < n; ++c) {
        const int32_t *rows = row_idx + col_ptr[c];
        const int32_t nr = col_ptr[c + 1] - col_ptr[c];
        size_t g = 0;
        for (; g < used.size(); ++g) {
            bool fits = true;
            for (int32_t e = 0; e < nr && fits; ++e) fits = used[g][(size_t)rows[e]] < 0;
            if (fits) break;
        }
        if (g == used.size()) used.emplace_back((size_t)n, (int16_t)-1);
        groups[(size_t)c] = (int32_t)g;
        for (int32_t e = 0; e < nr; ++e) used[g][(size_t)rows[e]] = (int16_t)c;   // duplicate rows of a column collapse here
    }
    *n_groups = (int)used.size();
    if (hit) {
        hit->clear();
        for (const auto &u : used) hit->insert(hit->end(), u.begin(), u.end());
    }
    return IVP_OK;
}

std::string sparsity_tables(int n, const std::vector<int32_t> &groups, int n_groups, const std::vector<int16_t> &hit)
{
    std::string s = "namespace ivp_jit {\n__device__ const short ivp_sp_group_of[" + std::to_string(n) + "] = {";
    for (int c = 0; c < n; ++c) { s += std::to_string(groups[(size_t)c]); s += c + 1 < n ? "," : ""; }
    s += "};\n__device__ const short ivp_sp_hit[" + std::to_string((size_t)n_groups * n) + "] = {";
    for (size_t e = 0; e < hit.size(); ++e) { s += std::to_string((int)hit[e]); s += (e + 1) % 32 == 0 ? ",\n" : ","; }
    s += "};\n}\n";
    return s;
}

// LDS a banded BDF chunk kernel allocates when its factors are resident (BdfBand::lds_bytes() in bdf_band.h is the same
// formula, and the kernel asserts it): per trajectory of the wavefront the factors, the pivots, the KJ + 1 = 9 state
// copies of fd_jac_sparse, the group vector and, with event functions, the event stage.
constexpr int kBandLdsBudget = 65536;   // IVP_BAND_LDS_BUDGET
bool band_lds_fits(int n, int ml, int mu, int ne)
{
    const long ngroup = IVP_WAVE / ivp_group_width(n);
    const long w = 2L * ml + mu + 1;
    return ngroup * n * (8 * (w + 9 + 1 + (ne > 0 ? 1 : 0)) + 4) <= kBandLdsBudget;
}

// bandwidths of a validated pattern
void pattern_bandwidth(int n, const int32_t *col_ptr, const int32_t *row_idx, int *ml, int *mu)
{
    *ml = 0; *mu = 0;
    for (int c = 0; c < n; ++c)
        for (int32_t e = col_ptr[c]; e < col_ptr[c + 1]; ++e) {
            if (row_idx[e] - c > *ml) *ml = row_idx[e] - c;
            if (c - row_idx[e] > *mu) *mu = c - row_idx[e];
        }
}

std::string build_source(const JitRhs &r, int method, int full_in, bool ctl, bool coop_only, bool band_lds = false, bool radau_band = false)
{
    // kernel flavour (rk_launch.h): 2 = log-only exists for the adaptive explicit methods of problems without event functions
    const int flavour = (full_in == 2 && r.ne == 0 && (method == IVP_RK23 || method == IVP_DOPRI5 || method == IVP_DOP853)) ? 2 : (full_in ? 1 : 0);
    const char *full = flavour == 2 ? "2" : (flavour ? "1" : "0");
    std::string s;
    s += "typedef unsigned int uint32_t;\ntypedef int int32_t;\ntypedef unsigned long long uint64_t;\ntypedef long long int64_t;\n";
    s += "#define IVP_HD __device__ __forceinline__\n";
    s += "#define IVP_NS ivp_jit\n";
    s += "#define IVP_USER_NE " + std::to_string(r.ne) + "\n";
    s += std::string("#define IVP_USER_JAC ") + (r.has_jac ? "1" : "0") + "\n";
    const bool group = r.n > IVP_MAX_N;   // wave-per-trajectory kernels (rk_group.h): user code defines ode_comp()
    const bool radau = method == IVP_RADAU;   // radau_core.h: thread per trajectory, n <= 8, built like rk_radau.hip; radau_group.h beyond
    // a wave that owns its SIMD: coefficients pinned in registers (rk_core.h KC) -- but not the group Radau kernels, which
    // would spill to scratch (rk_radau_group.hip)
    if ((group || coop_only || radau) && !(group && radau)) s += "#define IVP_HOIST 2\n";
    if (radau && !group) s += "#define IVP_MIN_WAVES 1\n";
    const bool mass = radau && r.has_mass;   // only the Radau modules of a problem with the hook: every other module's source stays what it was
    if (mass) s += "#define IVP_USER_MASS 1\n";
    s += join(k_src_ivp_kargs_h);
    s += "\n// ---- user right-hand side ----\n";
    s += r.ode_source;
    s += "\n// ---- integrator ----\n";
    s += join(k_src_rk_core_h);
    char buf[4096];
    if (group) {
        s += join(k_src_bdf_core_h);
        s += join(k_src_rk_global_h);   // compact_append
        s += join(k_src_rk_group_h);
        s += join(k_src_bdf_group_h);
        if (radau) {   // radau_group.h: 8 < n <= 64 with G >= n lanes per trajectory, 64 < n <= 512 with G = 64 and several rows per lane
            s += join(k_src_radau_core_h);
            s += join(k_src_radau_group_h);
            // the banded call (ivp_radau_solve_banded*, IVP_RHS_BANDED problems only): the pattern's tables and bandwidths in the
            // functor, as in the BDF modules below, and bdf_band.h / radau_band.h behind radau_group.h.  Every other Radau
            // module generates the text it always did.
            std::string sp;
            if (radau_band) {
                s += r.sparsity_source;
                s += join(k_src_bdf_band_h);
                s += join(k_src_radau_band_h);
                sp = "  enum { SP_NGROUPS = " + std::to_string(r.n_groups) + " };\n"
                     "  static __device__ __forceinline__ int sp_group_of(int c) { return ivp_sp_group_of[c]; }\n"
                     "  static __device__ __forceinline__ int sp_hit(int e) { return ivp_sp_hit[e]; }\n"
                     "  enum { SP_ML = " + std::to_string(r.band_ml) + ", SP_MU = " + std::to_string(r.band_mu) + " };\n";
            }
            std::snprintf(buf, sizeof buf,
                          "namespace ivp_jit { struct RhsUser { enum { N = %d, P = %d, NE = IVP_USER_NE };\n"
                          "  static __device__ __forceinline__ double ode_comp(int i, double x, const double* y, const double* p) { return ::ode_comp(i, x, y, p); }\n"
                          "#if IVP_USER_JAC\n"
                          "  static __device__ __forceinline__ void jac_col(int col, double x, const double* y, double* column, const double* p) { ::jac_col(col, x, y, column, p); }\n"
                          "#endif\n"
                          "%s%s%s"
                          "}; }\n"
                          "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_init(const IvpKArgs a) { ivp_jit::group_init_body<ivp_jit::M_RADAU, ivp_jit::RhsUser, %s, %d>(a); }\n"
                          "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_chunk(const IvpKArgs a) { ivp_jit::group_chunk_body<ivp_jit::M_RADAU, ivp_jit::RhsUser, %s, %d>(a); }\n",
                          r.n, r.np,
                          // Event functions (ivp_radau_solve_events*; only modules of such problems get the line).  GroupRhs::events
                          // has barriers inside so_events' root search, which the 64 / G groups of a wavefront enter and leave
                          // independently: safe because these kernels' workgroup is ONE wavefront (__launch_bounds__(IVP_WAVE), one
                          // block of IVP_WAVE lanes per launch -- bdf_group.h:31-32 states the rule).  Never a multi-wave workgroup here.
                          r.ne > 0 ? "  static __device__ __forceinline__ void events(double x, const double* y, double* g, const double* p) { ::events(x, y, g, p); }\n" : "",
                          r.has_mass_col ? "  static __device__ __forceinline__ void mass_col(int col, double* column, const double* p) { ::mass_col(col, column, p); }\n" : "",
                          sp.c_str(),
                          flavour ? "1" : "0", ivp_group_width(r.n), flavour ? "1" : "0", ivp_group_width(r.n));
            s += buf;
            return s;
        }
        // the pattern is read by BDF only (the explicit methods never call jac): other modules compile to what they were
        const bool sparse = method == IVP_BDF && !r.sparsity_source.empty();
        std::string sp;
        if (sparse) {
            s += r.sparsity_source;
            sp = "  enum { SP_NGROUPS = " + std::to_string(r.n_groups) + " };\n"
                 "  static __device__ __forceinline__ int sp_group_of(int c) { return ivp_sp_group_of[c]; }\n"
                 "  static __device__ __forceinline__ int sp_hit(int e) { return ivp_sp_hit[e]; }\n";
            if (r.banded) sp += "  enum { SP_ML = " + std::to_string(r.band_ml) + ", SP_MU = " + std::to_string(r.band_mu) + " };\n";
        }
        const bool band = sparse && r.banded;
        if (band) s += join(k_src_bdf_band_h);
        const std::string lds_arg = (band && band_lds) ? ", true" : "";
        std::snprintf(buf, sizeof buf,
                      "namespace ivp_jit { struct RhsUser { enum { N = %d, P = %d, NE = IVP_USER_NE };\n"
                      "  static __device__ __forceinline__ double ode_comp(int i, double x, const double* y, const double* p) { return ::ode_comp(i, x, y, p); }\n"
                      "#if IVP_USER_NE > 0\n"
                      "  static __device__ __forceinline__ void events(double x, const double* y, double* g, const double* p) { ::events(x, y, g, p); }\n"
                      "#endif\n"
                      "#if IVP_USER_JAC\n"
                      "  static __device__ __forceinline__ void jac_col(int col, double x, const double* y, double* column, const double* p) { ::jac_col(col, x, y, column, p); }\n"
                      "#endif\n"
                      "%s"
                      "}; }\n"
                      "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_init(const IvpKArgs a) { ivp_jit::group_init_body<%d, ivp_jit::RhsUser, %s, %d>(a); }\n"
                      "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_chunk(const IvpKArgs a) { ivp_jit::group_chunk_body<%d, ivp_jit::RhsUser, %s, %d%s>(a); }\n",
                      r.n, r.np, sp.c_str(), method, full, ivp_group_width(r.n), method, full, ivp_group_width(r.n), lds_arg.c_str());
        s += buf;
        return s;
    }
    s += join(k_src_bdf_core_h);
    if (radau) s += join(k_src_radau_core_h);   // only the Radau modules: every other module's source stays what it was
    s += join(k_src_rk_global_h);
    std::snprintf(buf, sizeof buf,
                  "namespace ivp_jit { struct RhsUser { enum { N = %d, P = %d, NE = IVP_USER_NE };\n"
                  "  static IVP_HD void ode(double x, const double* y, double* d, const double* p) { ::ode(x, y, d, p); }\n"
                  "#if IVP_USER_NE > 0\n"
                  "  static IVP_HD void events(double x, const double* y, double* g, const double* p) { ::events(x, y, g, p); }\n"
                  "#endif\n"
                  "#if IVP_USER_JAC\n"
                  "  static IVP_HD void jac(double x, const double* y, double (&j)[N][N], const double* p) { ::jac(x, y, &j[0][0], p); }\n"
                  "#endif\n"
                  "%s"
                  "}; }\n", r.n, r.np,
                  mass ? "  static IVP_HD void mass(double (&m)[N][N], const double* p) { ::mass(&m[0][0], p); }\n" : "");
    s += buf;
    if (coop_only) {   // eight lanes per trajectory for the tail of a batch: its own module, pinned coefficients
        s += join(k_src_rk_coop_h);
        std::snprintf(buf, sizeof buf,
                      "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_coop(const IvpKArgs a)\n"
                      "{ ivp_jit::coop_chunk_body<%d, ivp_jit::RhsUser, %s>(a); }\n", method, full);
        s += buf;
        return s;
    }
    std::snprintf(buf, sizeof buf,
                  "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_init(const IvpKArgs a)\n"
                  "{ const uint32_t i = blockIdx.x * IVP_WAVE + threadIdx.x; if (i < a.B) ivp_jit::any_init_body<%d, ivp_jit::RhsUser, %s>(a, i); }\n"
                  "extern \"C\" __global__ __launch_bounds__(IVP_WAVE, IVP_MIN_WAVES) void ivp_jit_chunk(const IvpKArgs a)\n"
                  "{ ivp_jit::chunk_kernel_body<%d, ivp_jit::RhsUser, %s, %s>(a); }\n",
                  method, full, method, full,
                  (ctl && (method == IVP_RK23 || method == IVP_DOPRI5 || method == IVP_DOP853)) ? "true" : "false");
    s += buf;
    if (r.ne > 0 && flavour == 1 && method != IVP_BDF && method != IVP_RADAU) {   // deferred refinement: the explicit methods only
        std::snprintf(buf, sizeof buf,
                      "extern \"C\" __global__ __launch_bounds__(IVP_WAVE) void ivp_jit_events(const IvpKArgs a)\n"
                      "{ ivp_jit::event_kernel_body<%d, ivp_jit::RhsUser>(a); }\n", method);
        s += buf;
    }
    return s;
}

// Optional on-disk cache of compiled code objects (hiprtc takes 1-2 s per module): set IVP_JIT_CACHE_DIR to an
// existing directory.  Key = FNV-1a of the complete generated source, the compile options and the hiprtc version.
// The directory must be PRIVATE to the user and trusted: entries are GPU code objects that are loaded and run as they
// are found (the 64-bit key locates an entry, it does not authenticate it).
std::string cache_path(const std::string &src, const std::string &opts)
{
    const char *dir = std::getenv("IVP_JIT_CACHE_DIR");
    if (!dir || !*dir) return std::string();
    int major = 0, minor = 0;
    (void)hiprtcVersion(&major, &minor);
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const std::string &t) { for (unsigned char ch : t) { h ^= ch; h *= 1099511628211ull; } };
    mix(src); mix(opts); mix(std::to_string(major) + "." + std::to_string(minor));
    char name[64];
    std::snprintf(name, sizeof name, "/ivp_jit_%016llx.hsaco", (unsigned long long)h);
    return std::string(dir) + name;
}

int load_module(JitRhs &r, const std::vector<char> &code, JitModule *out, bool coop_only)
{
    if (hipModuleLoadData(&out->mod, code.data()) != hipSuccess) { r.log = "hipModuleLoadData failed"; return IVP_ERR_HIP; }
    if (coop_only) {
        if (hipModuleGetFunction(&out->coop, out->mod, "ivp_jit_coop") != hipSuccess) { r.log = "kernel lookup failed"; return IVP_ERR_HIP; }
        return IVP_OK;
    }
    if (hipModuleGetFunction(&out->init, out->mod, "ivp_jit_init") != hipSuccess ||
        hipModuleGetFunction(&out->chunk, out->mod, "ivp_jit_chunk") != hipSuccess) {
        r.log = "kernel lookup failed";
        return IVP_ERR_HIP;
    }
    if (hipModuleGetFunction(&out->events, out->mod, "ivp_jit_events") != hipSuccess) { out->events = nullptr; (void)hipGetLastError(); }   // only full modules with event functions have it
    return IVP_OK;
}

int compile_module(JitRhs &r, int method, int fp_mode, int full, bool ctl, JitModule *out, bool coop_only = false, bool band_lds = false, bool radau_band = false)
{
    const std::string src = build_source(r, method, full, ctl, coop_only, band_lds, radau_band);
    const std::string opt_key = r.arch + (fp_mode == IVP_FP_FAST ? "|fast" : "|strict");
    const std::string cpath = cache_path(src, opt_key);
    if (!cpath.empty()) {
        std::ifstream in(cpath, std::ios::binary);
        if (in) {
            std::vector<char> code((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            if (!code.empty()) {
                if (!out) return IVP_OK;
                if (load_module(r, code, out, coop_only) == IVP_OK) return IVP_OK;
                (void)hipGetLastError();   // unreadable cache entry: fall through and compile
            }
        }
    }
    if (out && !r.checked_code.empty() && r.checked_key == opt_key + "\n" + src) {
        std::vector<char> code;
        code.swap(r.checked_code);
        r.checked_key.clear();
        if (load_module(r, code, out, coop_only) == IVP_OK) return IVP_OK;
        (void)hipGetLastError();   // fall through and compile
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "ivp_user_rhs.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        r.log = "hiprtcCreateProgram failed";
        return IVP_ERR_JIT;
    }
    const std::string arch = "--offload-arch=" + r.arch;
    std::vector<const char *> opts = {arch.c_str(), "-O3", "-std=c++17"};
    opts.push_back("-ffp-contract=off");   // both arithmetic modes: the FMA mode's fused operations are written out (IVP_MA)
    opts.push_back(fp_mode == IVP_FP_FAST ? "-DIVP_FAST=1" : "-DIVP_FAST=0");
    const hiprtcResult cr = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    if (ls) hiprtcGetProgramLog(prog, &log[0]);
    if (cr != HIPRTC_SUCCESS) {
        r.log = "hiprtc: " + log;
        hiprtcDestroyProgram(&prog);
        return IVP_ERR_JIT;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    std::vector<char> code(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    if (!cpath.empty()) {   // best effort: write to a temporary name, then rename (atomic on POSIX)
        const std::string tmp = cpath + ".tmp" + std::to_string((unsigned long long)(uintptr_t)&r);
        std::ofstream o(tmp, std::ios::binary);
        if (o) {
            o.write(code.data(), (std::streamsize)code.size());
            o.close();
            if (!o || std::rename(tmp.c_str(), cpath.c_str()) != 0) std::remove(tmp.c_str());
        }
    }
    if (!out) {   // compile-only check
        if (r.has_mass || r.has_mass_col) { r.checked_key = opt_key + "\n" + src; r.checked_code.swap(code); }
        return IVP_OK;
    }
    return load_module(r, code, out, coop_only);
}

}  // namespace

int ivp_jit_n_events(void *handle) { return handle ? ((JitRhs *)handle)->ne : 0; }
bool ivp_jit_has_mass(void *handle) { return handle && (((JitRhs *)handle)->has_mass || ((JitRhs *)handle)->has_mass_col); }

int ivp_jit_compile(int device, const char *ode_source, int n, int n_params, int n_events, unsigned flags, void **handle, std::string *log,
                    const int32_t *col_ptr, const int32_t *row_idx)
{
    std::string sparsity_source;
    int n_groups = 0, ml = 0, mu = 0;
    const bool banded = (flags & IVP_RHS_BANDED) != 0;
    if (banded && !col_ptr) { if (log) *log = "IVP_RHS_BANDED needs a jac_sparsity pattern"; return IVP_ERR_BAD_ARGUMENT; }
    if (banded && (flags & IVP_RHS_HAS_JAC)) {
        if (log) *log = "IVP_RHS_BANDED with IVP_RHS_HAS_JAC: an analytic jac_col in band storage is not supported";
        return IVP_ERR_BAD_ARGUMENT;
    }
    if (col_ptr) {
        std::vector<int32_t> groups;
        std::vector<int16_t> hit;
        const char *why = "";
        const int rc = group_columns(n, col_ptr, row_idx, groups, &n_groups, &hit, &why);
        if (rc != IVP_OK) { if (log) *log = why; return rc; }
        // a snippet with its own jac_col keeps it and the pattern is dropped (ivp_wrapper.rs:245-258)
        if (!(flags & IVP_RHS_HAS_JAC)) sparsity_source = sparsity_tables(n, groups, n_groups, hit);
        if (banded) {
            pattern_bandwidth(n, col_ptr, row_idx, &ml, &mu);
            if (2 * ml + mu + 1 >= n) {
                if (log) *log = "IVP_RHS_BANDED: the band (ml = " + std::to_string(ml) + ", mu = " + std::to_string(mu) + ") is as wide as the matrix (2 ml + mu + 1 >= n)";
                return IVP_ERR_BAD_ARGUMENT;
            }
        }
    }
    JitRhs *r = new JitRhs();
    r->sparsity_source = sparsity_source;
    r->n_groups = n_groups;
    r->banded = banded;
    r->band_ml = ml;
    r->band_mu = mu;
    r->device = device;
    r->has_jac = (flags & IVP_RHS_HAS_JAC) != 0;
    r->has_mass = (flags & IVP_RHS_HAS_MASS) != 0;
    r->has_mass_col = (flags & IVP_RHS_HAS_MASS_COL) != 0;
    r->n = n;
    r->np = n_params;
    r->ne = n_events;
    r->ode_source = ode_source;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.gcnArchName[0]) {
        r->arch = prop.gcnArchName;
        const size_t colon = r->arch.find(':');  // "gfx950:sramecc+:xnack-" -> "gfx950"
        if (colon != std::string::npos) r->arch.resize(colon);
    } else {
        r->arch = "gfx950";
    }
    // compile the default configuration now so that syntax errors surface at ivp_rhs_compile() time -- for a problem with a
    // mass matrix that is the Radau module, the only one any entry point launches and the only one that instantiates mass()
    // ... or, with the column hook, the group Radau module (ivp_rhs_compile_ex has checked its bounds)
    // (a mass matrix with event functions: ivp_radau_solve_events* is the one call that runs it, with this module)
    const bool radau_only = (r->has_mass && n <= IVP_MAX_N) || r->has_mass_col;
    int rc = compile_module(*r, radau_only ? IVP_RADAU : IVP_DOPRI5, IVP_FP_STRICT, n_events > 0, false, nullptr);
    if (rc == IVP_OK && r->has_jac && !r->has_mass_col) rc = compile_module(*r, IVP_BDF, IVP_FP_STRICT, n_events > 0, false, nullptr);   // jac() is only instantiated by BDF
    if (rc != IVP_OK) {
        if (log) *log = r->log;
        delete r;
        return rc;
    }
    *handle = r;
    return IVP_OK;
}

void ivp_jit_free(void *handle)
{
    JitRhs *r = (JitRhs *)handle;
    if (!r) return;
    for (auto &kv : r->modules)
        if (kv.second.mod) (void)hipModuleUnload(kv.second.mod);
    delete r;
}

const char *ivp_jit_last_log(void *handle) { return handle ? ((JitRhs *)handle)->log.c_str() : ""; }

bool ivp_jit_band(void *handle, int *ml, int *mu, bool *lds_fits)
{
    JitRhs *r = (JitRhs *)handle;
    if (!r || !r->banded) return false;
    if (ml) *ml = r->band_ml;
    if (mu) *mu = r->band_mu;
    if (lds_fits) *lds_fits = band_lds_fits(r->n, r->band_ml, r->band_mu, r->ne);
    return true;
}

bool ivp_jit_has_sparsity(void *handle) { return handle && ((JitRhs *)handle)->n_groups > 0; }

void ivp_jit_dims(void *handle, int *n, int *np)
{
    JitRhs *r = (JitRhs *)handle;
    *n = r->n;
    *np = r->np;
}

hipError_t ivp_jit_launch(void *handle, int what, int method, int fp_mode, int full, const IvpKArgs &a, uint32_t lanes,
                          hipStream_t s)
{
    JitRhs *r = (JitRhs *)handle;
    JitModule m;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        const bool ctl = a.has_ctl != 0;
        const bool coop = what == IVP_LAUNCH_COOP;   // the cooperative kernel reads the controller fields at run time anyway
        if (coop && !((r->ne == 0 || full) && (method == IVP_DOPRI5 || method == IVP_DOP853) && r->n <= IVP_MAX_N)) return hipErrorInvalidValue;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
        // banded problems: the BDF chunk kernel with LDS-resident factors is a module of its own (init kernels are the same in both)
        const bool band_lds = r->banded && method == IVP_BDF && a.lds_lu != 0 && band_lds_fits(r->n, r->band_ml, r->band_mu, r->ne);
        // the banded Radau call (ivp_radau_solve_banded*) marks its argument block: a module of its own, in band storage
        const bool radau_band = r->banded && method == IVP_RADAU && (a.ctl_nstiff & ivp_host::IVP_RAD_BAND_CALL) != 0;
        auto key = std::make_tuple(dev, method, fp_mode, full, coop ? false : ctl, coop, band_lds, radau_band);
        auto it = r->modules.find(key);
        if (it == r->modules.end()) {
            JitModule nm;
            if (compile_module(*r, method, fp_mode, full, coop ? false : ctl, &nm, coop, band_lds, radau_band) != IVP_OK) return hipErrorInvalidValue;   // r->log says why (ivp_jit_last_log)
            it = r->modules.emplace(key, nm).first;
        }
        m = it->second;
    }
    unsigned grid = (lanes + IVP_WAVE - 1) / IVP_WAVE;
    if (what == IVP_LAUNCH_CHUNK && a.lpw && r->n <= IVP_MAX_N) grid = (lanes + a.lpw - 1) / a.lpw;   // thin waves (ivp_kargs.h)
    if (r->n > IVP_MAX_N) {   // large n: a group of G lanes per trajectory, 64 / G trajectories per wave
        const unsigned per_wave = IVP_WAVE / (unsigned)ivp_group_width(r->n);
        grid = (lanes + per_wave - 1) / per_wave;
    }
    hipFunction_t fn = what == IVP_LAUNCH_INIT ? m.init : m.chunk;
    unsigned grid_y = 1;
    if (what == IVP_LAUNCH_EVENTS) {   // one lane per noted step: grid.y strides over a trajectory's noted steps
        if (!m.events) return hipErrorInvalidValue;
        fn = m.events;
        grid = (lanes + IVP_WAVE - 1) / IVP_WAVE;
        grid_y = 4;
    }
    if (what == IVP_LAUNCH_COOP) {
        if (!m.coop) return hipErrorInvalidValue;
        fn = m.coop;
        grid = (lanes + 7) / 8;
    }
    if (grid == 0) return hipSuccess;
    IvpKArgs ka = a;
    void *args[] = {&ka};
    return hipModuleLaunchKernel(fn, grid, grid_y, 1, IVP_WAVE, 1, 1, 0, s, args, nullptr);
}

extern "C" {

int ivp_jac_sparsity_groups(int32_t n, const int32_t *col_ptr, const int32_t *row_idx, int32_t *groups_out, int32_t *n_groups_out)
{
    if (!groups_out || !n_groups_out) return IVP_ERR_BAD_ARGUMENT;
    std::vector<int32_t> groups;
    int n_groups = 0;
    const int rc = group_columns(n, col_ptr, row_idx, groups, &n_groups, nullptr, nullptr);
    if (rc != IVP_OK) return rc;
    for (int32_t c = 0; c < n; ++c) groups_out[c] = groups[(size_t)c];
    *n_groups_out = n_groups;
    return IVP_OK;
}

int ivp_jac_sparsity_bandwidth(int32_t n, const int32_t *col_ptr, const int32_t *row_idx, int32_t *ml_out, int32_t *mu_out)
{
    if (!ml_out || !mu_out) return IVP_ERR_BAD_ARGUMENT;
    std::vector<int32_t> groups;
    int n_groups = 0;
    const int rc = group_columns(n, col_ptr, row_idx, groups, &n_groups, nullptr, nullptr);   // the validation of ivp_jac_sparsity_groups
    if (rc != IVP_OK) return rc;
    int ml = 0, mu = 0;
    pattern_bandwidth(n, col_ptr, row_idx, &ml, &mu);
    *ml_out = ml;
    *mu_out = mu;
    return IVP_OK;
}

int ivp_rhs_jac_layout(const void *handle, int32_t *banded, int32_t *ml, int32_t *mu, uint64_t *jac_doubles, uint64_t *lu_doubles)
{
    if (!handle) return IVP_ERR_BAD_ARGUMENT;
    const JitRhs *r = (const JitRhs *)handle;
    const uint64_t n = (uint64_t)r->n;
    if (banded) *banded = r->banded ? 1 : 0;
    if (ml) *ml = r->banded ? r->band_ml : 0;
    if (mu) *mu = r->banded ? r->band_mu : 0;
    if (jac_doubles) *jac_doubles = r->banded ? (uint64_t)(r->band_ml + r->band_mu + 1) * n : n * n;
    if (lu_doubles) *lu_doubles = r->banded ? (uint64_t)(2 * r->band_ml + r->band_mu + 1) * n : n * n;
    return IVP_OK;
}

int ivp_rhs_compile_sparse(ivp_ctx_t *ctx, const char *source, int32_t n, int32_t n_params, int32_t n_events, uint32_t flags,
                           const int32_t *col_ptr, const int32_t *row_idx, void **handle)
{
    using ivp_host::fail;
    if (!ctx || !source || !handle) return IVP_ERR_BAD_ARGUMENT;
    if (n < 1 || n > IVP_MAX_GROUP_N || n_params < 0 || n_params > IVP_MAX_P || n_events < 0 || n_events > 64)
        return fail(ctx, IVP_ERR_BAD_ARGUMENT, "unsupported dimensions");
    if (flags & ~(IVP_RHS_HAS_JAC | IVP_RHS_BANDED)) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "unknown flags 0x%x", flags);
    if ((flags & IVP_RHS_BANDED) && n <= IVP_MAX_N) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "IVP_RHS_BANDED needs 8 < n <= 512");
    if (!col_ptr) return fail(ctx, IVP_ERR_BAD_ARGUMENT, "jac_sparsity: col_ptr is NULL");
    std::string log;
    const int rc = ivp_jit_compile(ctx->device, source, n, n_params, n_events, flags, handle, &log, col_ptr, row_idx);
    if (rc != IVP_OK) ctx->err = log;
    return rc;
}

}  // extern "C"
