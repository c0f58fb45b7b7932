// r3g_api.cpp -- C ABI (include/r3g.h) over the HIP kernels.  Compiled with hipcc.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/r3g.h"
#include "r3g_ctx.h"
#include "mesh_kernels.h"
#include "meshfit_core.h"
#include "surf_common.h"
#include "tex_kernels.h"

namespace r3g {
static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(R3G_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// "meshdist_fill", "meshinside pairs": a step's or a buffer's name for the error text, with the user's name in it
struct Named {
    char s[64];
    Named(const char* fmt, const char* who) { snprintf(s, sizeof s, fmt, who); }
    operator const char*() const { return s; }
};

// the read-back of a tiny device result: n bytes through a pinned buffer into *out, behind everything queued on the stream
static int read_back(const DevBuf& pinned, const char* dev, void* out, size_t n, const char* name, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(pinned.p, dev, n, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return hip_fail(e, Named("hipMemcpyAsync(%s)", name));
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, Named("hipStreamSynchronize(%s)", name));
    memcpy(out, pinned.p, n);
    return R3G_OK;
}

// ---- hierarchical volume decoder: planner (model-free) -------------------------------------------------------------
int hier_select(Ctx* c, const float* d_coarse, int n_coarse, double level, double band, int is_finest, int64_t* count, hipStream_t s) {
    c->hier_selected = false;
    if (n_coarse < 2 || n_coarse > 645) return fail(R3G_ERR_INVALID, "r3g_hier_select: n_coarse outside [2, 645] (int32 indices of the fine lattice)");
    if (!(band >= 0.0)) return fail(R3G_ERR_INVALID, "r3g_hier_select: band must be >= 0");
    HierLayout lay;
    const size_t need = hier_workspace_bytes(n_coarse, &lay);
    int rc = c->hier_ws.grow(need, s, "hier workspace");
    if (rc) return rc;
    hipError_t e = hier_select_launch(d_coarse, level, band, is_finest, c->hier_ws.p, lay, s);
    if (e != hipSuccess) return hip_fail(e, "hier_select_launch");
    unsigned long long n = 0;
    if ((rc = read_back(c->h_small, c->hier_ws.p + lay.off_small, &n, 8, "hier select", s))) return rc;    // the level's one read-back
    c->hier_lay = lay;
    c->hier_count = (int64_t)n;
    c->hier_selected = true;
    *count = c->hier_count;
    return R3G_OK;
}

int hier_indices(Ctx* c, int32_t* d_idx_out, hipStream_t s) {
    if (!c->hier_selected) return fail(R3G_ERR_STATE, "r3g_hier_indices: no successful r3g_hier_select precedes this call");
    if (c->hier_count == 0) return R3G_OK;
    if (!d_idx_out) return fail(R3G_ERR_INVALID, "r3g_hier_indices: null argument");
    hipError_t e = hier_indices_launch(c->hier_ws.p, c->hier_lay, d_idx_out, s);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "hier_indices_launch");
}

int hier_merge(Ctx* c, const float* d_coarse, const float* d_values, float* d_fine_out, hipStream_t s) {
    if (!c->hier_selected) return fail(R3G_ERR_STATE, "r3g_hier_merge: no successful r3g_hier_select precedes this call");
    if (!d_coarse || !d_fine_out || (c->hier_count && !d_values)) return fail(R3G_ERR_INVALID, "r3g_hier_merge: null argument");
    if ((uintptr_t)d_fine_out % 16) return fail(R3G_ERR_INVALID, "r3g_hier_merge: d_fine_out must be 16-byte aligned");
    hipError_t e = hier_merge_launch(c->hier_ws.p, c->hier_lay, d_coarse, d_values, d_fine_out, s);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "hier_merge_launch");
}

int hier_unsafe_cells(Ctx* c, const float* d_fine, double level, int64_t* count, hipStream_t s) {
    if (!c->hier_selected) return fail(R3G_ERR_STATE, "hier_unsafe_cells: no successful select precedes this call");
    hipError_t e = hier_unsafe_launch(c->hier_ws.p, c->hier_lay, d_fine, level, s);
    if (e != hipSuccess) return hip_fail(e, "hier_unsafe_launch");
    unsigned long long n = 0;
    if (const int rc = read_back(c->h_small, c->hier_ws.p + c->hier_lay.off_small + 8, &n, 8, "hier unsafe cells", s)) return rc;
    *count = (int64_t)n;
    return R3G_OK;
}

// ---- grids in CSR form: the mesh distance's cells and the point-in-mesh columns ----------------------
static int grid_small(Ctx* c, const char* ws, const GridCsrLayout& lay, const char* who, hipStream_t s, GridCsrSmall* out) {
    return read_back(c->h_small, ws + lay.off_small, out, sizeof(GridCsrSmall), who, s);
}

// what the build driver needs to know of its user; `records` launches the user's records kernel
struct MeshdistBuild {
    static constexpr int D = 3, kMaxRes = r3g_md::kMaxRes;
    static constexpr size_t record_bytes = sizeof(r3g_md::Tri);
    static constexpr const char *who = "meshdist", *no_face = "the target mesh has no face", *cell = "cell";
    static int initial_resolution(int64_t nf) { return r3g_md::initial_resolution(nf); }
    const char* check() const { return nullptr; }
    hipError_t records(char* ws, const GridCsrLayout& lay, const float* v, int64_t nv, const int32_t* f, int64_t nf, hipStream_t s) const {
        return meshdist_records(ws, lay, v, nv, f, nf, s);
    }
};

struct MeshinsideBuild {
    static constexpr int D = 2, kMaxRes = r3g_mi::kMaxRes;
    static constexpr size_t record_bytes = sizeof(r3g_mi::Rec);
    static constexpr const char *who = "meshinside", *no_face = "the mesh has no face", *cell = "column";
    static int initial_resolution(int64_t nf) { return r3g_mi::initial_resolution(nf); }
    int axis;
    const char* check() const { return axis < 0 || axis > 2 ? "axis outside 0..2" : nullptr; }
    hipError_t records(char* ws, const GridCsrLayout& lay, const float* v, int64_t nv, const int32_t* f, int64_t nf, hipStream_t s) const {
        return meshinside_records(ws, lay, v, nv, f, nf, axis, s);
    }
};

// validate, reserve, records, read-back and checks, box, resolution, pairs reserve, fill, sync
template <class U>
static int grid_csr_build(Ctx* c, GridCsrState<U::D>* st, const U& user, const float* d_verts, int64_t n_verts, const int32_t* d_faces,
                          int64_t n_faces, int resolution, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out, hipStream_t s) {
    constexpr int D = U::D;
    const char* who = U::who;
    st->built = false;
    if (n_verts < 0 || n_verts >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 30))
        return fail(R3G_ERR_INVALID, "r3g_%s_build: mesh size out of range", who);
    if (n_faces == 0) return fail(R3G_ERR_INVALID, "r3g_%s_build: %s", who, U::no_face);
    if (!d_faces || (n_verts && !d_verts)) return fail(R3G_ERR_INVALID, "r3g_%s_build: null buffer", who);
    if (const char* bad = user.check()) return fail(R3G_ERR_INVALID, "r3g_%s_build: %s", who, bad);
    if (resolution < 0 || resolution > U::kMaxRes)
        return fail(R3G_ERR_INVALID, "r3g_%s_build: resolution outside [0, %d] (0 = automatic)", who, U::kMaxRes);
    const int initial = U::initial_resolution(n_faces);
    GridCsrLayout lay;
    const size_t need = grid_csr_workspace_bytes(n_faces, U::record_bytes, r3g_grid::cells<D>(resolution ? resolution : initial), &lay);
    int rc = st->ws.grow(need, s, Named("%s workspace", who));
    if (rc) return rc;
    st->lay = lay;
    hipError_t e = user.records(st->ws.p, lay, d_verts, n_verts, d_faces, n_faces, s);
    if (e != hipSuccess) return hip_fail(e, Named("%s_records", who));
    GridCsrSmall sm;
    if ((rc = grid_small(c, st->ws.p, lay, who, s, &sm))) return rc;
    // (-2 by the contract of include/r3g.h: found on the device, before anything is read through the index)
    if (sm.bad_index) return fail(-2, "r3g_%s_build: a face index lies outside [0, %lld)", who, (long long)n_verts);
    if ((int64_t)sm.skipped >= n_faces)
        return fail(R3G_ERR_INVALID, "r3g_%s_build: every face has a non-finite vertex (%lld skipped)", who, (long long)sm.skipped);
    float lo[D], hi[D];
    for (int a = 0; a < D; ++a) lo[a] = r3g_grid::dec_float(sm.box[a]), hi[a] = r3g_grid::dec_float(sm.box[D + a]);
    r3g_grid::GridN<D> g;
    int64_t pairs = 0;
    rc = r3g_grid::choose_resolution(lo, hi, resolution, initial, n_faces, [&](const r3g_grid::GridN<D>& cand, int64_t* n) {
        e = grid_csr_count_pairs(st->ws.p, lay, n_faces, cand, s);
        if (e != hipSuccess) return hip_fail(e, Named("%s_count_pairs", who));
        const int r = grid_small(c, st->ws.p, lay, who, s, &sm);
        *n = (int64_t)sm.pairs;
        return r;
    }, &g, &pairs);
    if (rc) return rc;
    if (pairs >= (1ll << 31))
        return fail(R3G_ERR_INVALID, "r3g_%s_build: %lld (face, %s) pairs at resolution %d; force a lower one", who, (long long)pairs, U::cell, g.res);
    if ((rc = st->pairs.grow(4 * (size_t)pairs, s, Named("%s pairs", who)))) return rc;
    e = grid_csr_fill(st->ws.p, lay, n_faces, g, (int32_t*)st->pairs.p, s);
    if (e != hipSuccess) return hip_fail(e, Named("%s_fill", who));
    e = hipStreamSynchronize(s);      // the caller may free its mesh buffers, and a fault would surface here
    if (e != hipSuccess) return hip_fail(e, Named("hipStreamSynchronize(%s_fill)", who));
    st->grid = g;
    st->built = true;
    if (resolution_out) *resolution_out = g.res;
    if (pairs_out) *pairs_out = pairs;
    if (skipped_out) *skipped_out = (int64_t)sm.skipped;
    return R3G_OK;
}

// the point cloud's grid (DESIGN.md sections 4k, 4m): its resolution argument, and the one build
static int cloud_resolution_check(const char* who, int resolution) {
    if (resolution >= 0 && resolution <= r3g_cl::kMaxRes) return R3G_OK;
    return fail(R3G_ERR_INVALID, "%s: resolution outside [0, %d] (0 = automatic)", who, r3g_cl::kMaxRes);
}

// The grid of c->cloud for r3g_cloud_build and r3g_cloud_dbscan: workspace for the most cells, before(), records, read-back (under
// `name`), box, resolution, grid, points reserve, fill.  The automatic resolution is choose(lo, hi, usable) and at most res_most: it
// can only fall when points are skipped, so the workspace sized for all of them is enough.  before() is DBSCAN's first event and
// launch, queued directly in front of the records (the event's interval holds no host work but the launches).  -> *skipped; when
// that is every point, nothing past the read-back has run and what it means is the caller's to say.  The caller has checked its
// arguments and cleared c->cloud.built, and sets it behind a sync of its own.
template <class Choose, class Before>
static int cloud_grid_build(Ctx* c, const char* name, const float* d_points, int64_t n_points, int resolution, int res_most, Choose choose,
                            Before before, int64_t* skipped, hipStream_t s) {
    GridCsrState<3>* st = &c->cloud;
    const size_t need = grid_csr_workspace_bytes(n_points, sizeof(r3g_cl::Pt), r3g_grid::cells<3>(resolution ? resolution : res_most), &st->lay);
    const GridCsrLayout& lay = st->lay;
    int rc = st->ws.grow(need, s, "cloud workspace");
    if (rc || (rc = before())) return rc;
    hipError_t e = cloud_records(st->ws.p, lay, d_points, n_points, s);
    if (e != hipSuccess) return hip_fail(e, "cloud_records");
    GridCsrSmall sm;
    if ((rc = grid_small(c, st->ws.p, lay, name, s, &sm))) return rc;
    *skipped = (int64_t)sm.skipped;
    const int64_t usable = n_points - *skipped;
    if (usable <= 0) return R3G_OK;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = r3g_grid::dec_float(sm.box[a]), hi[a] = r3g_grid::dec_float(sm.box[3 + a]);
    st->grid = r3g_grid::make_grid(lo, hi, resolution ? resolution : choose(lo, hi, usable));
    if ((rc = st->pairs.grow(sizeof(r3g_cl::Pt) * (size_t)usable, s, "cloud points"))) return rc;
    e = cloud_fill(st->ws.p, lay, n_points, st->grid, st->pairs.as<r3g_cl::Pt>(), s);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "cloud_fill");
}

// ---- surface extractors: marching cubes and dual marching cubes (one count and one emit driver) -----------------------------
// what the drivers need to know of their extractor
struct McExtract {
    static constexpr const char* who = "mc";
    static constexpr uint64_t ids_per_node = 3;      // a vertex lives on one of a node's three edges: ids stay inside int32
    static constexpr int faces_per_item = 1;         // totals[1] counts triangles
    static bool no_surface(unsigned long long nv, unsigned long long) { return nv == 0; }
    static constexpr auto workspace_bytes = mc_workspace_bytes;
    static constexpr auto count_launch = mc_count_launch;
    static constexpr auto emit_launch = mc_emit_launch;
};

struct DmcExtract {
    static constexpr const char* who = "dmc";
    static constexpr uint64_t ids_per_node = 6;      // at most 4 vertices and 6 triangles per cell: ids and triangle counts stay inside int32
    static constexpr int faces_per_item = 2;         // totals[1] counts quads
    static bool no_surface(unsigned long long, unsigned long long nq) { return nq == 0; }
    static constexpr auto workspace_bytes = dmc_workspace_bytes;
    static constexpr auto count_launch = dmc_count_launch;
    static constexpr auto emit_launch = dmc_emit_launch;
};

// validate, reserve, classify + scan, 64 B read-back, status / level-range / no-surface decode, state capture
template <class U>
static int surf_count(Ctx* c, SurfState* st, const float* d_grid, int n0, int n1, int n2, double level, int flag,
                      int64_t* n_verts, int64_t* n_faces, hipStream_t s) {
    const char* who = U::who;
    if (n0 < 2 || n1 < 2 || n2 < 2) return fail(R3G_ERR_INVALID, "Input array must be at least 2x2x2.");
    const uint64_t nnodes = (uint64_t)n0 * n1 * n2;
    if (nnodes * U::ids_per_node >= (1ull << 31)) return fail(R3G_ERR_INVALID, "r3g_%s_count: grid too large for int32 vertex ids", who);
    st->counted = false;
    SurfWorkspaceLayout lay;
    const size_t need = U::workspace_bytes(n0, n1, n2, &lay);
    int rc = st->ws.grow(need, s, Named("%s workspace", who));
    if (rc) return rc;
    hipError_t e = U::count_launch(d_grid, n0, n1, n2, level, flag, st->ws.p, lay, s);
    if (e != hipSuccess) return hip_fail(e, Named("%s_count_launch", who));
    unsigned long long small[8];
    if ((rc = read_back(c->h_small, st->ws.p + lay.off_small, small, 64, Named("%s count", who), s))) return rc;
    unsigned status;                                     // @0
    memcpy(&status, small, sizeof status);
    const unsigned long long* totals = small + 2;        // {vertices, triangles or quads, non-empty blocks} @16
    *n_verts = (int64_t)totals[0];
    *n_faces = (int64_t)(U::faces_per_item * totals[1]);
    // numpy: level < vol.min() or level > vol.max(); a NaN anywhere makes both comparisons false
    if (!(status & R3G_SURF_FLAG_NAN) && (!(status & R3G_SURF_FLAG_LE) || !(status & R3G_SURF_FLAG_GE)))
        return fail(R3G_ERR_LEVEL_RANGE, "Surface level must be within volume data range.");
    if (U::no_surface(totals[0], totals[1])) return fail(R3G_ERR_NO_SURFACE, "No surface found at the given iso value.");
    st->lay = lay;
    st->lay.nnz = (uint32_t)totals[2];
    st->grid = d_grid;
    st->n[0] = n0; st->n[1] = n1; st->n[2] = n2;
    st->level = level;
    st->counted = true;
    return R3G_OK;
}

template <class U>
static int surf_emit(SurfState* st, float* d_verts, int32_t* d_faces, const double* xform, int reverse_faces, hipStream_t s) {
    const char* who = U::who;
    if (!st->counted) return fail(R3G_ERR_STATE, "r3g_%s_emit: no successful r3g_%s_count precedes this call", who, who);
    hipError_t e = U::emit_launch(st->grid, st->n[0], st->n[1], st->n[2], st->level, st->ws.p, st->lay, d_verts, d_faces, xform,
                                  reverse_faces, s);
    if (e != hipSuccess) return hip_fail(e, Named("%s_emit_launch", who));
    return R3G_OK;
}
}  // namespace r3g

using namespace r3g;

extern "C" {

int r3g_version(void) { return R3G_VERSION; }
const char* r3g_last_error(void) { return g_err; }

int r3g_create(int device, r3g_ctx** out) {
    if (!out) return fail(R3G_ERR_INVALID, "r3g_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(R3G_ERR_NO_DEVICE, "r3g_create: no HIP device visible (%s); libr3g has no CPU path",
                    e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(R3G_ERR_INVALID, "r3g_create: device %d out of range [0,%d)", device, n);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(R3G_ERR_NO_DEVICE, "r3g_create: device %d is %s, libr3g is built for gfx950 only", device,
                    prop.gcnArchName);
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return fail(R3G_ERR_HIP, "out of host memory");
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    (void)option_store("gemm_num_cu", c->num_cu);      // (ignored unless positive)
    if (const int rc = c->h_small.grow(64, nullptr, "read-back buffer")) {
        delete c;
        return rc;
    }
    *out = reinterpret_cast<r3g_ctx*>(c);
    return R3G_OK;
}

void r3g_destroy(r3g_ctx* ctx) {
    if (!ctx) return;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    (void)hipSetDevice(c->device);      // before anything is freed: the buffers and events below belong to this device
    c->release_model();
    c->release_unet();
    delete c;                           // every buffer and event of the context goes with its DevBuf or PassTimer member
}

int r3g_mc_count(r3g_ctx* ctx, const float* d_grid, int n0, int n1, int n2, double level, int use_classic,
                 int64_t* n_verts, int64_t* n_faces, void* stream) {
    if (!ctx || !d_grid || !n_verts || !n_faces) return fail(R3G_ERR_INVALID, "r3g_mc_count: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return surf_count<McExtract>(c, &c->mc, d_grid, n0, n1, n2, level, use_classic, n_verts, n_faces, (hipStream_t)stream);
}

int r3g_mc_emit(r3g_ctx* ctx, float* d_verts, int32_t* d_faces, const double* xform, int reverse_faces,
                void* stream) {
    if (!ctx || !d_verts || !d_faces) return fail(R3G_ERR_INVALID, "r3g_mc_emit: null argument");
    return surf_emit<McExtract>(&reinterpret_cast<Ctx*>(ctx)->mc, d_verts, d_faces, xform, reverse_faces, (hipStream_t)stream);
}

// ---- dual marching cubes ----------------------------------------------------------------
int r3g_dmc_count(r3g_ctx* ctx, const float* d_grid, int n0, int n1, int n2, double level, int manifold,
                  int64_t* n_verts, int64_t* n_faces, void* stream) {
    if (!ctx || !d_grid || !n_verts || !n_faces) return fail(R3G_ERR_INVALID, "r3g_dmc_count: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return surf_count<DmcExtract>(c, &c->dmc, d_grid, n0, n1, n2, level, manifold, n_verts, n_faces, (hipStream_t)stream);
}

int r3g_dmc_emit(r3g_ctx* ctx, float* d_verts, int32_t* d_faces, const double* xform, int reverse_faces,
                 void* stream) {
    if (!ctx || !d_verts || !d_faces) return fail(R3G_ERR_INVALID, "r3g_dmc_emit: null argument");
    return surf_emit<DmcExtract>(&reinterpret_cast<Ctx*>(ctx)->dmc, d_verts, d_faces, xform, reverse_faces, (hipStream_t)stream);
}

// ---- hierarchical volume decoder: the planner steps on their own ----------------------------------------------
int r3g_hier_select(r3g_ctx* ctx, const float* d_coarse, int n_coarse, double level, double band, int is_finest, int64_t* count,
                    void* stream) {
    if (!ctx || !d_coarse || !count) return fail(R3G_ERR_INVALID, "r3g_hier_select: null argument");
    return hier_select(reinterpret_cast<Ctx*>(ctx), d_coarse, n_coarse, level, band, is_finest, count, (hipStream_t)stream);
}

int r3g_hier_indices(r3g_ctx* ctx, int32_t* d_idx_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_hier_indices: null argument");
    return hier_indices(reinterpret_cast<Ctx*>(ctx), d_idx_out, (hipStream_t)stream);
}

int r3g_hier_merge(r3g_ctx* ctx, const float* d_coarse, const float* d_values, float* d_fine_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_hier_merge: null argument");
    return hier_merge(reinterpret_cast<Ctx*>(ctx), d_coarse, d_values, d_fine_out, (hipStream_t)stream);
}

// ---- mesh cleaners -------------------------------------------------------------------------------------------
static int mesh_args(const char* who, r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces,
                     int64_t* n_faces) {
    if (!ctx || !n_verts || !n_faces) return fail(R3G_ERR_INVALID, "%s: null argument", who);
    if (*n_verts < 0 || *n_faces < 0 || *n_verts >= (1ll << 31) || *n_faces >= (1ll << 30))
        return fail(R3G_ERR_INVALID, "%s: mesh size out of range", who);
    if ((*n_verts && !d_verts) || (*n_faces && !d_faces)) return fail(R3G_ERR_INVALID, "%s: null buffer", who);
    return R3G_OK;
}

int r3g_mesh_remove_floaters(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                             double min_ratio, void* stream) {
    int rc = mesh_args("r3g_mesh_remove_floaters", ctx, d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    rc = c->mesh_ws.grow(mesh_workspace_bytes(*n_verts, *n_faces, 0), (hipStream_t)stream, "mesh workspace");
    if (rc) return rc;
    hipError_t e = mesh_remove_floaters(c->mesh_ws.p, c->mesh_ws.bytes, c->h_small.as<unsigned>(), d_verts, n_verts, d_faces,
                                        n_faces, min_ratio, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "mesh_remove_floaters");
}

int r3g_mesh_remove_degenerate(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                               void* stream) {
    int rc = mesh_args("r3g_mesh_remove_degenerate", ctx, d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    rc = c->mesh_ws.grow(mesh_workspace_bytes(*n_verts, *n_faces, 0), (hipStream_t)stream, "mesh workspace");
    if (rc) return rc;
    hipError_t e = mesh_remove_degenerate(c->mesh_ws.p, c->mesh_ws.bytes, c->h_small.as<unsigned>(), d_verts, n_verts, d_faces,
                                          n_faces, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "mesh_remove_degenerate");
}

int r3g_mesh_reduce_faces(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                          int64_t max_faces, void* stream) {
    int rc = mesh_args("r3g_mesh_reduce_faces", ctx, d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    if (max_faces < 1 || max_faces > 200000000) return fail(R3G_ERR_INVALID, "r3g_mesh_reduce_faces: max_faces out of range");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    rc = c->mesh_ws.grow(mesh_workspace_bytes(*n_verts, *n_faces, 0), (hipStream_t)stream, "mesh workspace");
    if (rc) return rc;
    hipError_t e = mesh_reduce_faces(c->mesh_ws.p, c->mesh_ws.bytes, c->h_small.as<unsigned>(), d_verts, n_verts, d_faces,
                                     n_faces, max_faces, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "mesh_reduce_faces");
}

int r3g_mesh_cluster_faces(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                           int64_t max_faces, void* stream) {
    int rc = mesh_args("r3g_mesh_cluster_faces", ctx, d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    if (max_faces < 1 || max_faces > 200000000) return fail(R3G_ERR_INVALID, "r3g_mesh_cluster_faces: max_faces out of range");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const int64_t r = mesh_reduce_initial_res(max_faces);
    rc = c->mesh_ws.grow(mesh_workspace_bytes(*n_verts, *n_faces, r * r * r), (hipStream_t)stream, "mesh workspace");
    if (rc) return rc;
    hipError_t e = mesh_cluster_faces(c->mesh_ws.p, c->mesh_ws.bytes, c->h_small.as<unsigned>(), d_verts, n_verts, d_faces,
                                      n_faces, max_faces, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "mesh_cluster_faces");
}

// ---- mesh distance ------------------------------------------------------------------------------------------------
int r3g_meshdist_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces,
                       int resolution, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshdist_build: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return grid_csr_build(c, &c->meshdist, MeshdistBuild{}, d_verts, n_verts, d_faces, n_faces, resolution, resolution_out, pairs_out,
                          skipped_out, (hipStream_t)stream);
}

int r3g_meshdist_query(r3g_ctx* ctx, const float* d_points, int64_t n_points, float* d_dist2, int32_t* d_face, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshdist_query: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshdist.built) return fail(R3G_ERR_STATE, "r3g_meshdist_query: no successful r3g_meshdist_build on this context");
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_meshdist_query: n_points out of range");
    if (n_points == 0) return R3G_OK;
    if (!d_points || !d_dist2 || !d_face) return fail(R3G_ERR_INVALID, "r3g_meshdist_query: null buffer");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = meshdist_query(c->meshdist.ws.p, c->meshdist.lay, c->meshdist.grid, c->meshdist.pairs.as<const int32_t>(), d_points,
                                  n_points, d_dist2, d_face, s);
    if (e != hipSuccess) return hip_fail(e, "meshdist_query");
    GridCsrSmall sm;
    int rc = grid_small(c, c->meshdist.ws.p, c->meshdist.lay, "meshdist", s, &sm);
    if (rc) return rc;
    counter_add(LC_MESHDIST_TESTS, (int64_t)sm.tests);
    return R3G_OK;
}

// ---- point clouds ----------------------------------------------------------------------------------------
int r3g_cloud_build(r3g_ctx* ctx, const float* d_points, int64_t n_points, int resolution, int* resolution_out, int64_t* skipped_out,
                    void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_build: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    c->cloud.built = false;
    if (n_points <= 0 || n_points > 0x7fffffffll) return fail(R3G_ERR_INVALID, "r3g_cloud_build: n_points outside [1, 2^31 - 1]");
    if (!d_points) return fail(R3G_ERR_INVALID, "r3g_cloud_build: null buffer");
    if (const int rc = cloud_resolution_check("r3g_cloud_build", resolution)) return rc;
    auto res = [](int64_t n) { return r3g_cl::auto_resolution(n, r3g_cl::kPointsPerCell); };
    int64_t skipped = 0;
    auto choose = [&](const float*, const float*, int64_t usable) { return res(usable); };
    if (const int rc = cloud_grid_build(c, "cloud", d_points, n_points, resolution, res(n_points), choose, [] { return 0; }, &skipped, s)) return rc;
    if (skipped >= n_points)
        return fail(R3G_ERR_INVALID, "r3g_cloud_build: every point has a non-finite coordinate (%lld skipped)", (long long)skipped);
    hipError_t e = hipStreamSynchronize(s);      // the caller may free its points, and a fault would surface here
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(cloud_fill)");
    c->cloud.built = true;
    if (resolution_out) *resolution_out = c->cloud.grid.res;
    if (skipped_out) *skipped_out = skipped;
    return R3G_OK;
}

int r3g_cloud_knn(r3g_ctx* ctx, const float* d_queries, int64_t n_queries, int k, float* d_dist2, int32_t* d_index, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_knn: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->cloud.built) return fail(R3G_ERR_STATE, "r3g_cloud_knn: no successful r3g_cloud_build on this context");
    if (k < 1 || k > r3g_cl::kMaxK) return fail(R3G_ERR_INVALID, "r3g_cloud_knn: k outside [1, %d]", r3g_cl::kMaxK);
    if (n_queries < 0 || n_queries >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_cloud_knn: n_queries out of range");
    if (n_queries == 0) return R3G_OK;
    if (!d_queries || !d_dist2 || !d_index) return fail(R3G_ERR_INVALID, "r3g_cloud_knn: null buffer");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = cloud_knn(c->cloud.ws.p, c->cloud.lay, c->cloud.grid, c->cloud.pairs.as<const r3g_cl::Pt>(), d_queries, n_queries, k, d_dist2,
                             d_index, s);
    if (e != hipSuccess) return hip_fail(e, "cloud_knn");
    GridCsrSmall sm;
    int rc = grid_small(c, c->cloud.ws.p, c->cloud.lay, "cloud", s, &sm);
    if (rc) return rc;
    counter_add(LC_CLOUD_TESTS, (int64_t)sm.tests);
    return R3G_OK;
}

// ---- normal orientation over the k-NN graph -------------------------------------------------------------
int r3g_cloud_orient(r3g_ctx* ctx, const float* d_points, const float* d_normals, int64_t n_points, int k, int resolution, int8_t* d_sign,
                     int32_t* d_tree, int64_t* report, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_orient: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (n_points <= 0 || n_points > 0x7fffffffll) return fail(R3G_ERR_INVALID, "r3g_cloud_orient: n_points outside [1, 2^31 - 1]");
    if (k < r3g_or::kMinK || k > r3g_or::kMaxK) return fail(R3G_ERR_INVALID, "r3g_cloud_orient: k outside [%d, %d]", r3g_or::kMinK, r3g_or::kMaxK);
    if (const int rc = cloud_resolution_check("r3g_cloud_orient", resolution)) return rc;
    if (!d_points || !d_normals || !d_sign || !d_tree) return fail(R3G_ERR_INVALID, "r3g_cloud_orient: null buffer");
    OrientLayout lay;
    int rc = c->orient_ws.grow(orient_workspace_bytes(n_points, k, &lay), s, "orient workspace");
    if (rc) return rc;
    char* ws = c->orient_ws.p;
    auto small = [&](OrientSmall* out) { return read_back(c->h_small, ws + lay.off_small, out, sizeof(OrientSmall), "orient", s); };
    static_assert(sizeof(OrientSmall) <= 64, "the pinned read-back buffer");
    hipError_t e = orient_prepare(ws, lay, d_points, d_normals, n_points, s);
    if (e != hipSuccess) return hip_fail(e, "orient_prepare");
    OrientSmall sm;
    if ((rc = small(&sm))) return rc;
    int64_t rounds = 0;
    if (sm.usable > 0) {
        // the cloud of the usable points alone (the others are NaN, which the build leaves out): indices stay those of d_points
        const float* q = (const float*)(ws + lay.off_q);
        if ((rc = r3g_cloud_build(ctx, q, n_points, resolution, nullptr, nullptr, stream))) return rc;
        if ((rc = r3g_cloud_knn(ctx, q, n_points, k + 1, (float*)(ws + lay.off_d2), (int32_t*)(ws + lay.off_idx), stream))) return rc;
        for (;;) {
            if (rounds >= 64) return fail(R3G_ERR_INVALID, "r3g_cloud_orient: 64 rounds without an end");
            if ((e = orient_round(ws, lay, n_points, k, s)) != hipSuccess) return hip_fail(e, "orient_round");
            ++rounds;
            if ((rc = small(&sm))) return rc;
            if (sm.merged == 0) break;
        }
    }
    if ((e = orient_finish(ws, lay, d_normals, n_points, k, d_sign, d_tree, s)) != hipSuccess) return hip_fail(e, "orient_finish");
    if ((rc = small(&sm))) return rc;
    counter_add(LC_ORIENT_ROUNDS, rounds);
    if (report) {
        const int64_t r[r3g_or::kReport] = {(int64_t)sm.usable, (int64_t)sm.trees, (int64_t)sm.flipped, rounds, (int64_t)sm.frustrated, 0, 0, 0};
        memcpy(report, r, sizeof r);
    }
    return R3G_OK;
}

// ---- DBSCAN on a point cloud ---------------------------------------------------------------------------
int r3g_cloud_dbscan(r3g_ctx* ctx, const float* d_points, int64_t n_points, double eps, int min_samples, int resolution, int32_t* d_label,
                     uint32_t* d_count, int64_t* report, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    GridCsrState<3>* st = &c->cloud;
    hipStream_t s = (hipStream_t)stream;
    if (!(eps > 0.0) || !(eps - eps == 0.0)) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan: eps must be finite and > 0");
    if (min_samples < 1) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan: min_samples must be >= 1");
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan: n_points outside [0, 2^31 - 1]");
    int rc = cloud_resolution_check("r3g_cloud_dbscan", resolution);
    if (rc) return rc;
    int64_t rep[r3g_db::kReport] = {0, 0, 0, 0, 0, -1, 0, 0};
    auto done = [&]() {
        if (report) memcpy(report, rep, sizeof rep);
        return R3G_OK;
    };
    st->built = false;              // the call replaces the context's cloud
    c->dbscan_timed = false;
    if (n_points == 0) return done();
    if (!d_points || !d_label) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan: null buffer");
    if ((rc = c->dbscan_ev.make("dbscan"))) return rc;
    DbscanLayout dl;
    if ((rc = c->dbscan_ws.grow(dbscan_workspace_bytes(n_points, &dl), s, "dbscan workspace"))) return rc;
    hipError_t e;
    auto begin = [&]() -> int {
        if (const int r = c->dbscan_ev.mark(0, s)) return r;
        e = dbscan_begin(c->dbscan_ws.p, dl, n_points, d_label, d_count, s);
        return e == hipSuccess ? R3G_OK : hip_fail(e, "dbscan_begin");
    };
    auto choose = [&](const float* lo, const float* hi, int64_t usable) { return r3g_db::auto_resolution(lo, hi, eps, usable); };
    int64_t skipped = 0;
    rc = cloud_grid_build(c, "dbscan", d_points, n_points, resolution, r3g_db::auto_resolution_most(n_points), choose, begin, &skipped, s);
    if (rc) return rc;
    int64_t launches = 2;           // begin, records
    const int64_t usable = n_points - skipped;
    if (usable <= 0) {              // nothing to cluster: every label is -1 already
        counter_add(LC_DBSCAN_LAUNCHES, launches);
        return done();
    }
    launches += 5;                  // count, the scan's three, fill
    const r3g_cl::Grid& g = st->grid;
    int run = 0;
    e = dbscan_run(c->dbscan_ws.p, dl, g, st->pairs.as<const r3g_cl::Pt>(), (const unsigned*)(st->ws.p + st->lay.off_starts), usable, n_points, eps,
                   (uint32_t)min_samples, d_label, d_count, c->dbscan_ev.ev + 1, &run, s);
    if (e != hipSuccess) return hip_fail(e, "dbscan_run");
    launches += run;
    static_assert(sizeof(DbscanSmall) <= 64, "the pinned read-back buffer");
    DbscanSmall ds;      // (its sync: the caller may free its points, and a fault would surface here)
    if ((rc = read_back(c->h_small, c->dbscan_ws.p + dl.off_small, &ds, sizeof ds, "dbscan", s))) return rc;
    st->built = true;
    c->dbscan_timed = true;
    counter_add(LC_DBSCAN_LAUNCHES, launches);
    counter_add(LC_DBSCAN_TESTS, (int64_t)ds.tests);
    rep[0] = usable, rep[1] = (int64_t)ds.n_core, rep[2] = (int64_t)ds.n_border, rep[3] = usable - rep[1] - rep[2];
    rep[4] = (int64_t)ds.n_clusters, rep[5] = r3g_db::best_label(ds.best), rep[6] = r3g_db::best_size(ds.best), rep[7] = g.res;
    return done();
}

int r3g_cloud_dbscan_times(r3g_ctx* ctx, double* ms) {
    if (!ctx || !ms) return fail(R3G_ERR_INVALID, "r3g_cloud_dbscan_times: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->dbscan_timed) return fail(R3G_ERR_STATE, "r3g_cloud_dbscan_times: no complete r3g_cloud_dbscan on this context");
    for (int p = 0; p <= kDbscanPasses; ++p)
        if (const int rc = c->dbscan_ev.elapsed(p, &ms[p])) return rc;
    return R3G_OK;
}

// ---- plane fit: batched RANSAC and the moments of a masked set -----------------------------------------
static int plane_reserve(Ctx* c, int64_t n_points, int64_t n_hyp, bool own_count, bool own_mask, PlaneLayout* lay, hipStream_t s) {
    if (const int rc = c->h_plane.grow(sizeof(PlaneSmall), s, "plane read-back buffer")) return rc;
    return c->plane_ws.grow(plane_workspace_bytes(n_points, n_hyp, own_count, own_mask, lay), s, "plane workspace");
}

// out[0..5]: centroid and the "up" normal; val: the eigenvalues ascending; *few: fewer than 3 rows in the set
static void plane_solve(const r3g_pl::Moments& m, double centroid[3], double normal[3], double val[3], int* few) {
    for (int a = 0; a < 3; ++a) centroid[a] = m.c[a];
    r3g_pl::plane_of(m, val, normal, few);
}

int r3g_plane_ransac(r3g_ctx* ctx, const float* d_points, int64_t n_points, const int32_t* d_triples, int n_hyp, double threshold,
                     uint32_t* d_count, uint8_t* d_mask, int64_t* report, double* plane, void* stream) {
    if (!(threshold > 0.0) || !(threshold - threshold == 0.0)) return fail(R3G_ERR_INVALID, "r3g_plane_ransac: threshold must be finite and > 0");
    if (n_hyp < 0 || n_hyp > r3g_pl::kMaxHyp) return fail(R3G_ERR_INVALID, "r3g_plane_ransac: n_hyp outside [0, %d]", r3g_pl::kMaxHyp);
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_plane_ransac: n_points outside [0, 2^31 - 1]");
    if (!report || !plane || (n_points && !d_points) || (n_hyp && !d_triples)) return fail(R3G_ERR_INVALID, "r3g_plane_ransac: null buffer");
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_plane_ransac: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    c->plane_timed = false;
    auto& ev = c->plane_ev;
    int rc = ev.make("plane");
    if (rc) return rc;
    PlaneLayout lay;
    if ((rc = plane_reserve(c, n_points, n_hyp, !d_count, !d_mask, &lay, s))) return rc;
    char* ws = c->plane_ws.p;
    uint32_t* count = d_count ? d_count : (uint32_t*)(ws + lay.off_count);
    uint8_t* mask = d_mask ? d_mask : (uint8_t*)(ws + lay.off_mask);
    hipError_t e;
    if ((rc = ev.mark(0, s))) return rc;
    if ((e = plane_table(ws, lay, d_points, n_points, d_triples, n_hyp, count, s)) != hipSuccess) return hip_fail(e, "plane_table");
    if ((rc = ev.mark(1, s))) return rc;
    if ((e = plane_count(ws, lay, d_points, n_points, n_hyp, threshold, count, c->num_cu, s)) != hipSuccess) return hip_fail(e, "plane_count");
    if ((rc = ev.mark(2, s))) return rc;
    if ((e = plane_winner(ws, lay, d_points, n_points, n_hyp, threshold, count, mask, s)) != hipSuccess) return hip_fail(e, "plane_winner");
    if ((rc = ev.mark(3, s))) return rc;
    if ((e = plane_moments(ws, lay, d_points, n_points, mask, s)) != hipSuccess) return hip_fail(e, "plane_moments");
    if ((rc = ev.mark(4, s))) return rc;
    PlaneSmall sm;      // (its sync: the caller may free its buffers, and a fault would surface here)
    if ((rc = read_back(c->h_plane, ws + lay.off_small, &sm, sizeof sm, "plane", s))) return rc;
    c->plane_timed = true;
    int few = 0;
    double centroid[3], normal[3], val[3];
    plane_solve(sm.mom, centroid, normal, val, &few);
    const int64_t rep[r3g_pl::kReport] = {(int64_t)sm.usable, (int64_t)sm.valid, r3g_pl::key_h(sm.key), (int64_t)r3g_pl::key_count(sm.key), few, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    for (int a = 0; a < 3; ++a) {
        plane[a] = sm.best.p0[a], plane[3 + a] = sm.best.n[a];
        plane[6 + a] = centroid[a], plane[9 + a] = normal[a], plane[12 + a] = val[a];
    }
    plane[15] = 0.0;
    return R3G_OK;
}

int r3g_plane_moments(r3g_ctx* ctx, const float* d_points, int64_t n_points, const uint8_t* d_mask, double* out, int64_t* report, void* stream) {
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_plane_moments: n_points outside [0, 2^31 - 1]");
    if (!out || !report || (n_points && !d_points)) return fail(R3G_ERR_INVALID, "r3g_plane_moments: null buffer");
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_plane_moments: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    PlaneLayout lay;
    if (const int rc = plane_reserve(c, n_points, 0, false, false, &lay, s)) return rc;
    char* ws = c->plane_ws.p;
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, sizeof(PlaneSmall), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(plane)");
    if ((e = plane_moments(ws, lay, d_points, n_points, d_mask, s)) != hipSuccess) return hip_fail(e, "plane_moments");
    PlaneSmall sm;
    if (const int rc = read_back(c->h_plane, ws + lay.off_small, &sm, sizeof sm, "plane moments", s)) return rc;
    int few = 0;
    double centroid[3], normal[3], val[3];
    plane_solve(sm.mom, centroid, normal, val, &few);
    out[0] = (double)sm.mom.n;
    for (int a = 0; a < 3; ++a) out[1 + a] = centroid[a], out[10 + a] = val[a], out[13 + a] = normal[a];
    for (int a = 0; a < 6; ++a) out[4 + a] = sm.mom.s[a];
    const int64_t rep[r3g_pl::kMomReport] = {(int64_t)sm.mom.n, (int64_t)sm.mom.skipped, few, 0};
    memcpy(report, rep, sizeof rep);
    return R3G_OK;
}

int r3g_plane_times(r3g_ctx* ctx, double* ms) {
    if (!ctx || !ms) return fail(R3G_ERR_INVALID, "r3g_plane_times: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->plane_timed) return fail(R3G_ERR_STATE, "r3g_plane_times: no complete r3g_plane_ransac on this context");
    for (int p = 0; p < r3g_pl::kPasses; ++p)
        if (const int rc = c->plane_ev.elapsed(p, &ms[p])) return rc;
    return R3G_OK;
}

// ---- soft silhouette: K-nearest soft rasteriser and its gradient to the vertices -------------------------
static int softras_args(const char* who, int64_t n_verts, int64_t n_faces, int height, int width, int K, double sigma, double blur_radius,
                        SoftrasGeom* g) {
    if (K < 1 || K > r3g_sr::kMaxK) return fail(R3G_ERR_INVALID, "%s: K outside [1, %d]", who, r3g_sr::kMaxK);
    const float sg = (float)sigma, br = (float)blur_radius;
    if (!(sg > 0.0f) || !(sg - sg == 0.0f)) return fail(R3G_ERR_INVALID, "%s: sigma must be finite and > 0 in float32", who);
    if (!(br >= 0.0f)) return fail(R3G_ERR_INVALID, "%s: blur_radius must be >= 0", who);
    if (height < 1 || width < 1 || height > r3g_sr::kMaxSide || width > r3g_sr::kMaxSide)
        return fail(R3G_ERR_INVALID, "%s: height and width must lie in [1, %d]", who, r3g_sr::kMaxSide);
    if (n_verts < 0 || n_verts >= (1ll << 31) || n_faces < 0 || n_faces > (1ll << 29)) return fail(R3G_ERR_INVALID, "%s: mesh sizes out of range", who);
    g->height = height, g->width = width, g->K = K;
    g->tiles_x = (width + r3g_sr::kTile - 1) / r3g_sr::kTile, g->tiles_y = (height + r3g_sr::kTile - 1) / r3g_sr::kTile;
    g->sigma = sg, g->blur_radius = br, g->blur_reach = sqrtf(br);
    return R3G_OK;
}

int r3g_softras_forward(r3g_ctx* ctx, const float* d_pos, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height, int width, int K,
                        double sigma, double blur_radius, float* d_alpha, int32_t* d_face, float* d_dist, float* d_zbuf, int64_t* report,
                        void* stream) {
    SoftrasGeom g;
    if (const int rc = softras_args("r3g_softras_forward", n_verts, n_faces, height, width, K, sigma, blur_radius, &g)) return rc;
    if (!d_alpha || !d_face || !d_dist || !d_zbuf || !report || (n_faces && !d_tri) || (n_verts && !d_pos))
        return fail(R3G_ERR_INVALID, "r3g_softras_forward: null buffer");
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_softras_forward: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    c->softras_fwd_timed = false;
    auto& ev = c->softras_ev;
    if (const int rc = ev.make("softras")) return rc;
    SoftrasLayout lay;
    if (const int rc = c->softras_ws.grow(softras_workspace_bytes(height, width, &lay), s, "softras workspace")) return rc;
    char* ws = c->softras_ws.p;
    hipError_t e;
    if (const int rc = ev.mark(0, s)) return rc;
    if ((e = softras_bin_count(ws, lay, g, d_pos, n_verts, d_tri, n_faces, s)) != hipSuccess) return hip_fail(e, "softras_bin_count");
    static_assert(sizeof(SoftrasSmall) <= 64, "the pinned read-back buffer");
    SoftrasSmall sm;      // (the call's one sync: the pair list is sized from it, and it is the report)
    if (const int rc = read_back(c->h_small, ws + lay.off_small, &sm, sizeof sm, "softras", s)) return rc;
    if (sm.pairs > 0x7fffffffull) return fail(R3G_ERR_INVALID, "r3g_softras_forward: %llu (face, tile) pairs, more than 2^31 - 1", sm.pairs);
    if (const int rc = c->softras_pairs.grow(4 * (size_t)sm.pairs, s, "softras pairs")) return rc;
    if ((e = softras_bin_fill(ws, lay, g, d_pos, n_verts, d_tri, n_faces, c->softras_pairs.as<int32_t>(), (unsigned)sm.pairs, s)) != hipSuccess)
        return hip_fail(e, "softras_bin_fill");
    if (const int rc = ev.mark(1, s)) return rc;
    if ((e = softras_forward(ws, lay, g, d_pos, n_verts, d_tri, n_faces, c->softras_pairs.as<const int32_t>(), d_alpha, d_face, d_dist, d_zbuf, s)) !=
        hipSuccess)
        return hip_fail(e, "softras_forward");
    if (const int rc = ev.mark(2, s)) return rc;
    c->softras_fwd_timed = true;
    const int64_t rep[r3g_sr::kFwdReport] = {(int64_t)sm.pairs, (int64_t)sm.used, (int64_t)sm.skipped, lay.tiles, 0, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    return R3G_OK;
}

int r3g_softras_backward(r3g_ctx* ctx, const float* d_pos, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height, int width, int K,
                         double sigma, double blur_radius, const int32_t* d_face, const float* d_dist, const float* d_grad_alpha,
                         const int32_t* d_corner_start, const int32_t* d_corner_ids, float* d_grad_face, float* d_grad_pos, int64_t* report,
                         void* stream) {
    SoftrasGeom g;
    if (const int rc = softras_args("r3g_softras_backward", n_verts, n_faces, height, width, K, sigma, blur_radius, &g)) return rc;
    if (!d_face || !d_dist || !d_grad_alpha || !report || (n_faces && (!d_tri || !d_grad_face || !d_corner_ids)) ||
        (n_verts && (!d_pos || !d_grad_pos || !d_corner_start)))
        return fail(R3G_ERR_INVALID, "r3g_softras_backward: null buffer");
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_softras_backward: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    c->softras_bwd_timed = false;
    auto& ev = c->softras_ev;
    if (const int rc = ev.make("softras")) return rc;
    SoftrasLayout lay;
    if (const int rc = c->softras_ws.grow(softras_workspace_bytes(height, width, &lay), s, "softras workspace")) return rc;
    char* ws = c->softras_ws.p;
    hipError_t e;
    if (const int rc = ev.mark(3, s)) return rc;
    if ((e = softras_backward(ws, lay, g, d_pos, n_verts, d_tri, n_faces, d_face, d_dist, d_grad_alpha, d_grad_face, s)) != hipSuccess)
        return hip_fail(e, "softras_backward");
    if (const int rc = ev.mark(4, s)) return rc;
    if ((e = softras_gather(d_grad_face, d_corner_start, d_corner_ids, n_verts, n_faces, d_grad_pos, s)) != hipSuccess)
        return hip_fail(e, "softras_gather");
    if (const int rc = ev.mark(5, s)) return rc;
    SoftrasSmall sm;      // (its sync: the caller may free its buffers, and a fault would surface here)
    if (const int rc = read_back(c->h_small, ws + lay.off_small, &sm, sizeof sm, "softras backward", s)) return rc;
    c->softras_bwd_timed = true;
    const int64_t rep[r3g_sr::kBwdReport] = {(int64_t)sm.found, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    return R3G_OK;
}

int r3g_softras_times(r3g_ctx* ctx, double* ms) {
    if (!ctx || !ms) return fail(R3G_ERR_INVALID, "r3g_softras_times: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->softras_fwd_timed) return fail(R3G_ERR_STATE, "r3g_softras_times: no complete r3g_softras_forward on this context");
    if (const int rc = c->softras_ev.sync(2)) return rc;      // (the forward returns before its last kernel has run)
    for (int p = 0; p < r3g_sr::kPasses; ++p) {
        ms[p] = -1.0;
        if (p >= 2 && !c->softras_bwd_timed) continue;
        if (const int rc = c->softras_ev.elapsed(p < 2 ? p : p + 1, &ms[p])) return rc;      // (no pass between events 2 and 3)
    }
    return R3G_OK;
}

// ---- point clouds: every triangle's nearest point ---------------------------------------------------------
static int facecloud_sizes(const char* who, int64_t n_verts, int64_t n_faces) {
    if (n_verts < 0 || n_faces < 0) return fail(R3G_ERR_INVALID, "%s: negative size", who);
    if (n_verts > 0x7fffffffll) return fail(R3G_ERR_INVALID, "%s: n_verts above 2^31 - 1", who);
    if (n_faces > r3g_fc::kMaxFaces) return fail(R3G_ERR_INVALID, "%s: n_faces above 2^29", who);
    return R3G_OK;
}

int r3g_cloud_faces(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, float* d_dist2,
                    int32_t* d_index, float* d_weights, float* d_diff, int64_t* report, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_faces: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = facecloud_sizes("r3g_cloud_faces", n_verts, n_faces)) return rc;
    if (!report || (n_faces && (!d_tri || !d_dist2 || !d_index || !d_weights || !d_diff)) || (n_verts && !d_verts))
        return fail(R3G_ERR_INVALID, "r3g_cloud_faces: null buffer");
    if (!c->cloud.built) return fail(R3G_ERR_STATE, "r3g_cloud_faces: no cloud on this context (r3g_cloud_build, _orient or _dbscan)");
    int64_t rep[r3g_fc::kReport] = {0, 0, 0, 0};
    if (n_faces == 0) {
        memcpy(report, rep, sizeof rep);
        return R3G_OK;
    }
    c->facecloud_fwd_timed = false;
    auto& ev = c->facecloud_ev;
    if (const int rc = ev.make("facecloud")) return rc;
    FacecloudLayout lay;
    if (const int rc = c->facecloud_ws.grow(facecloud_workspace_bytes(n_faces, &lay), s, "facecloud workspace")) return rc;
    char* ws = c->facecloud_ws.p;
    const GridCsrState<3>& cl = c->cloud;
    const r3g_cl::Pt* sorted = cl.pairs.as<const r3g_cl::Pt>();
    const unsigned* starts = (const unsigned*)(cl.ws.p + cl.lay.off_starts);
    hipError_t e;
    if (const int rc = ev.mark(0, s)) return rc;
    if ((e = facecloud_classify(ws, lay, cl.grid, d_verts, n_verts, d_tri, n_faces, s)) != hipSuccess) return hip_fail(e, "facecloud_classify");
    if (const int rc = ev.mark(1, s)) return rc;
    if ((e = facecloud_narrow(ws, lay, cl.grid, sorted, starts, n_faces, d_dist2, d_index, d_weights, d_diff, s)) != hipSuccess)
        return hip_fail(e, "facecloud_narrow");
    if (const int rc = ev.mark(2, s)) return rc;
    if ((e = facecloud_wide(ws, lay, cl.grid, sorted, starts, n_faces, d_dist2, d_index, d_weights, d_diff, s)) != hipSuccess)
        return hip_fail(e, "facecloud_wide");
    if (const int rc = ev.mark(3, s)) return rc;
    static_assert(sizeof(FacecloudSmall) <= 64, "the pinned read-back buffer");
    FacecloudSmall sm;      // (the call's one sync)
    if (const int rc = read_back(c->h_small, ws + lay.off_small, &sm, sizeof sm, "facecloud", s)) return rc;
    c->facecloud_fwd_timed = true;
    rep[0] = (int64_t)sm.usable, rep[1] = (int64_t)sm.tests, rep[2] = (int64_t)sm.wide, rep[3] = (int64_t)sm.max_ring;
    memcpy(report, rep, sizeof rep);
    return R3G_OK;
}

int r3g_cloud_faces_backward(r3g_ctx* ctx, int64_t n_verts, int64_t n_faces, const float* d_grad_dist2, const int32_t* d_index,
                             const float* d_weights, const float* d_diff, const int32_t* d_corner_start, const int32_t* d_corner_ids,
                             float* d_grad_verts, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_cloud_faces_backward: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = facecloud_sizes("r3g_cloud_faces_backward", n_verts, n_faces)) return rc;
    if ((n_faces && (!d_grad_dist2 || !d_index || !d_weights || !d_diff || !d_corner_ids)) || (n_verts && (!d_corner_start || !d_grad_verts)))
        return fail(R3G_ERR_INVALID, "r3g_cloud_faces_backward: null buffer");
    c->facecloud_bwd_timed = false;
    if (n_verts == 0) return R3G_OK;
    auto& ev = c->facecloud_ev;
    if (const int rc = ev.make("facecloud")) return rc;
    if (const int rc = ev.mark(4, s)) return rc;
    const hipError_t e = facecloud_gather(d_grad_dist2, d_index, d_weights, d_diff, d_corner_start, d_corner_ids, n_verts, n_faces, d_grad_verts, s);
    if (e != hipSuccess) return hip_fail(e, "facecloud_gather");
    if (const int rc = ev.mark(5, s)) return rc;
    c->facecloud_bwd_timed = true;
    return R3G_OK;
}

int r3g_cloud_faces_times(r3g_ctx* ctx, double* ms) {
    if (!ctx || !ms) return fail(R3G_ERR_INVALID, "r3g_cloud_faces_times: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->facecloud_fwd_timed) return fail(R3G_ERR_STATE, "r3g_cloud_faces_times: no complete r3g_cloud_faces on this context");
    for (int p = 0; p < 3; ++p)
        if (const int rc = c->facecloud_ev.elapsed(p, &ms[p])) return rc;
    ms[3] = -1.0;
    if (!c->facecloud_bwd_timed) return R3G_OK;
    if (const int rc = c->facecloud_ev.sync(5)) return rc;      // (the backward returns before its kernel has run)
    return c->facecloud_ev.elapsed(4, &ms[3]);
}

// ---- Poisson surface on a uniform lattice ---------------------------------------------------------------
static int recon_small(Ctx* c, ReconState* st, const char* what, hipStream_t s, ReconSmall* out) {
    return read_back(c->h_small, st->channels.p + recon_small_offset(st->lat.depth), out, sizeof(ReconSmall), what, s);
}

int r3g_recon_splat(r3g_ctx* ctx, const float* d_points, const float* d_normals, int64_t n_points, int depth, const double* centre,
                    double side, int64_t* d_channels_out, int64_t* usable_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_recon_splat: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    ReconState* st = &c->recon;
    hipStream_t s = (hipStream_t)stream;
    st->splatted = st->solved = false;
    if (n_points <= 0 || n_points > 0x7fffffffll) return fail(R3G_ERR_INVALID, "r3g_recon_splat: n_points outside [1, 2^31 - 1]");
    if (!d_points || !d_normals || !centre) return fail(R3G_ERR_INVALID, "r3g_recon_splat: null buffer");
    if (depth < r3g_rc::kMinDepth || depth > r3g_rc::kMaxDepth)
        return fail(R3G_ERR_INVALID, "r3g_recon_splat: depth outside [%d, %d]", r3g_rc::kMinDepth, r3g_rc::kMaxDepth);
    const r3g_rc::Lattice L = r3g_rc::make_lattice(depth, centre, side);
    bool ok = side > 0.0 && side - side == 0.0 && L.inv_h > 0.0f && L.inv_2h > 0.0f && L.inv_h - L.inv_h == 0.0f;
    for (int a = 0; a < 3; ++a) ok = ok && L.lo[a] - L.lo[a] == 0.0f;
    if (!ok) return fail(R3G_ERR_INVALID, "r3g_recon_splat: the box (centre, side) is not finite and positive in float32");
    int rc = st->channels.grow(recon_channels_bytes(depth), s, "recon channels");
    if (rc) return rc;
    if ((rc = st->levels.grow(recon_levels_bytes(depth), s, "recon levels"))) return rc;
    st->lat = L;
    st->side = side;
    hipError_t e = recon_splat(st, d_points, d_normals, n_points, s);
    if (e != hipSuccess) return hip_fail(e, "recon_splat");
    if (d_channels_out && (e = hipMemcpyAsync(d_channels_out, st->channels.p, recon_small_offset(depth), hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return hip_fail(e, "hipMemcpyAsync(recon channels)");
    ReconSmall sm;
    if ((rc = recon_small(c, st, "recon splat", s, &sm))) return rc;
    if (sm.usable == 0) return fail(R3G_ERR_INVALID, "r3g_recon_splat: no usable point (finite coordinates, finite non-zero normal)");
    st->splatted = true;
    if (usable_out) *usable_out = (int64_t)sm.usable;
    return R3G_OK;
}

int r3g_recon_solve(r3g_ctx* ctx, int cycles, float* d_b_out, float* d_chi_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_recon_solve: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    ReconState* st = &c->recon;
    if (!st->splatted) return fail(R3G_ERR_STATE, "r3g_recon_solve: no successful r3g_recon_splat on this context");
    if (cycles < 0 || cycles > 1000) return fail(R3G_ERR_INVALID, "r3g_recon_solve: cycles outside [0, 1000]");
    hipStream_t s = (hipStream_t)stream;
    st->solved = false;
    hipError_t e = recon_solve(st, cycles, s);
    if (e != hipSuccess) return hip_fail(e, "recon_solve");
    const int depth = st->lat.depth;
    const size_t bytes = (size_t)recon_nodes(depth) * 4;
    const float* lv = st->levels.as<const float>();
    if (d_b_out && (e = hipMemcpyAsync(d_b_out, lv + recon_level_offset(depth, depth, 2), bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return hip_fail(e, "hipMemcpyAsync(recon b)");
    if (d_chi_out && (e = hipMemcpyAsync(d_chi_out, lv + recon_level_offset(depth, depth, 0), bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return hip_fail(e, "hipMemcpyAsync(recon chi)");
    e = hipStreamSynchronize(s);      // a fault would surface here, before the state counts as solved
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(recon_solve)");
    st->solved = true;
    counter_add(LC_RECON_SOLVES), counter_add(LC_RECON_CYCLES, cycles);
    return R3G_OK;
}

int r3g_recon_sample(r3g_ctx* ctx, int field, const float* d_points, const float* d_normals, int64_t n_points, float* d_values_out,
                     int64_t* sum_out, int64_t* count_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_recon_sample: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    ReconState* st = &c->recon;
    if (field != 0 && field != 1) return fail(R3G_ERR_INVALID, "r3g_recon_sample: field is 0 (density) or 1 (chi)");
    if (!st->splatted) return fail(R3G_ERR_STATE, "r3g_recon_sample: no successful r3g_recon_splat on this context");
    if (field == 1 && !st->solved) return fail(R3G_ERR_STATE, "r3g_recon_sample: field 1 needs a successful r3g_recon_solve on this context");
    if (n_points <= 0 || n_points > 0x7fffffffll) return fail(R3G_ERR_INVALID, "r3g_recon_sample: n_points outside [1, 2^31 - 1]");
    if (!d_points) return fail(R3G_ERR_INVALID, "r3g_recon_sample: null buffer");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = recon_sample(st, field, d_points, d_normals, n_points, d_values_out, s);
    if (e != hipSuccess) return hip_fail(e, "recon_sample");
    ReconSmall sm;
    int rc = recon_small(c, st, "recon sample", s, &sm);
    if (rc) return rc;
    if (sum_out) *sum_out = (int64_t)sm.sum;
    if (count_out) *count_out = (int64_t)sm.usable;
    return R3G_OK;
}

int r3g_meshdist_closest(r3g_ctx* ctx, const float* d_points, int64_t n_points, float* d_dist2, int32_t* d_face, float* d_closest,
                         void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshdist_closest: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshdist.built) return fail(R3G_ERR_STATE, "r3g_meshdist_closest: no successful r3g_meshdist_build on this context");
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_meshdist_closest: n_points out of range");
    if (n_points == 0) return R3G_OK;
    if (!d_points || !d_dist2 || !d_face || !d_closest) return fail(R3G_ERR_INVALID, "r3g_meshdist_closest: null buffer");
    hipError_t e = meshfit_closest(c->meshdist.ws.p, c->meshdist.lay, c->meshdist.grid, c->meshdist.pairs.as<const int32_t>(), d_points,
                                   n_points, d_dist2, d_face, d_closest, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "meshfit_closest");
}

// one accumulation under x -> the record in c->h_fit
static int meshfit_accumulate(Ctx* c, const float* d_points, int64_t n, const float* d_weights, const r3g_md::Sim& x, int mode,
                              double max_dist, hipStream_t s, MeshfitRecord* out) {
    int rc = c->meshfit_ws.grow(meshfit_workspace_bytes(), s, "meshfit workspace");
    if (rc) return rc;
    if ((rc = c->h_fit.grow(sizeof(MeshfitRecord), s, "meshfit read-back buffer"))) return rc;
    const float md2 = (float)(max_dist * max_dist);
    hipError_t e = meshfit_step(c->meshfit_ws.p, c->meshdist.ws.p, c->meshdist.lay, c->meshdist.grid, c->meshdist.pairs.as<const int32_t>(),
                                d_points, n, d_weights, x, mode, md2, s);
    if (e != hipSuccess) return hip_fail(e, "meshfit_step");
    if ((rc = read_back(c->h_fit, c->meshfit_ws.p, out, sizeof(MeshfitRecord), "meshfit", s))) return rc;
    counter_add(LC_MESHFIT_STEPS);
    counter_add(LC_MESHDIST_TESTS, (int64_t)out->tests);
    return R3G_OK;
}

static int meshfit_check(const char* who, Ctx* c, const float* d_points, int64_t n, int mode, double max_dist) {
    if (!c->meshdist.built) return fail(R3G_ERR_STATE, "%s: no successful r3g_meshdist_build on this context", who);
    if (n < 0 || n >= (1ll << 31)) return fail(R3G_ERR_INVALID, "%s: n_points out of range", who);
    if (mode != r3g_md::kFitPoint && mode != r3g_md::kFitPlane) return fail(R3G_ERR_INVALID, "%s: mode must be 0 (point) or 1 (plane)", who);
    if (!(max_dist >= 0.0)) return fail(R3G_ERR_INVALID, "%s: max_dist must be >= 0 (+inf: no limit)", who);
    if (n && !d_points) return fail(R3G_ERR_INVALID, "%s: null buffer", who);
    return R3G_OK;
}

int r3g_meshfit_step(r3g_ctx* ctx, const float* d_points, int64_t n_points, const float* d_weights, const double* xform, int mode,
                     double max_dist, double* sums_out, int64_t* used_out, void* stream) {
    if (!ctx || !xform || !sums_out || !used_out) return fail(R3G_ERR_INVALID, "r3g_meshfit_step: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = meshfit_check("r3g_meshfit_step", c, d_points, n_points, mode, max_dist);
    if (rc) return rc;
    for (int i = 0; i < r3g_md::kFitMaxTerms; ++i) sums_out[i] = 0.0;
    *used_out = 0;
    if (n_points == 0) return R3G_OK;
    r3g_md::Sim x;
    x.s = xform[0];
    for (int i = 0; i < 9; ++i) x.r[i] = xform[1 + i];
    for (int i = 0; i < 3; ++i) x.t[i] = xform[10 + i];
    MeshfitRecord rec;
    if ((rc = meshfit_accumulate(c, d_points, n_points, d_weights, x, mode, max_dist, (hipStream_t)stream, &rec))) return rc;
    for (int i = 0; i < r3g_md::fit_terms(mode); ++i) sums_out[i] = rec.sums[i];
    *used_out = (int64_t)rec.used;
    return R3G_OK;
}

int r3g_meshfit(r3g_ctx* ctx, const float* d_points, int64_t n_points, const float* d_weights, const double* init, int mode,
                int with_scale, int max_iterations, double tolerance, double max_dist, double* matrix_out, double* info_out,
                void* stream) {
    if (!ctx || !matrix_out || !info_out) return fail(R3G_ERR_INVALID, "r3g_meshfit: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = meshfit_check("r3g_meshfit", c, d_points, n_points, mode, max_dist);
    if (rc) return rc;
    if (max_iterations < 0) return fail(R3G_ERR_INVALID, "r3g_meshfit: max_iterations must be >= 0");
    if (!(tolerance == tolerance)) return fail(R3G_ERR_INVALID, "r3g_meshfit: tolerance is NaN");
    r3g_md::Sim cur = r3g_mf::identity();
    if (init && !r3g_mf::from_matrix(init, &cur))
        return fail(R3G_ERR_INVALID, "r3g_meshfit: init is not a similarity [s R | t; 0 0 0 1] with s > 0 and det R = +1");
    double rms = 0.0, rms_prev = 0.0;
    int64_t used = 0;
    int updates = 0, converged = 0;
    if (n_points > 0) {
        double centre[3];
        r3g_md::fit_centre(c->meshdist.grid, centre);
        const int iw = mode == r3g_md::kFitPlane ? 35 : 0, id = mode == r3g_md::kFitPlane ? 36 : 17;
        for (int it = 0;; ++it) {
            MeshfitRecord rec;
            if ((rc = meshfit_accumulate(c, d_points, n_points, d_weights, cur, mode, max_dist, (hipStream_t)stream, &rec))) return rc;
            if (rec.used < 3 || !(rec.sums[iw] > 0.0))
                return fail(R3G_ERR_INVALID, "r3g_meshfit: too few points: %lld of %lld within max_dist in iteration %d (3 needed, with positive weight)",
                            (long long)rec.used, (long long)n_points, it);
            used = (int64_t)rec.used;
            rms = sqrt(rec.sums[id] / rec.sums[iw]);
            if (it > 0 && fabs(rms_prev - rms) < tolerance) {
                converged = 1;
                break;
            }
            if (it >= max_iterations) break;
            r3g_md::Sim delta;
            const bool ok = mode == r3g_md::kFitPlane ? r3g_mf::solve_plane(rec.sums, with_scale != 0, centre, &delta)
                                                      : r3g_mf::solve_point(rec.sums, with_scale != 0, centre, &delta);
            if (!ok) return fail(R3G_ERR_INVALID, "r3g_meshfit: non-finite sums in iteration %d (a non-finite weight?)", it);
            cur = r3g_mf::compose(delta, cur);
            ++updates;
            rms_prev = rms;
        }
    }
    r3g_mf::to_matrix(cur, matrix_out);
    info_out[0] = (double)updates;
    info_out[1] = (double)converged;
    info_out[2] = rms;
    info_out[3] = (double)used;
    info_out[4] = cur.s;
    return R3G_OK;
}

// ---- point in mesh ------------------------------------------------------------------------------------------------
int r3g_meshinside_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces, int axis,
                         int resolution, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshinside_build: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const int rc = grid_csr_build(c, &c->meshinside, MeshinsideBuild{axis}, d_verts, n_verts, d_faces, n_faces, resolution, resolution_out,
                                  pairs_out, skipped_out, (hipStream_t)stream);
    if (rc == R3G_OK) c->meshinside_axis = axis;
    return rc;
}

int r3g_meshinside_query(r3g_ctx* ctx, const float* d_points, int64_t n_points, int32_t* d_count, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshinside_query: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshinside.built) return fail(R3G_ERR_STATE, "r3g_meshinside_query: no successful r3g_meshinside_build on this context");
    if (n_points < 0 || n_points >= (1ll << 31)) return fail(R3G_ERR_INVALID, "r3g_meshinside_query: n_points out of range");
    if (n_points == 0) return R3G_OK;
    if (!d_points || !d_count) return fail(R3G_ERR_INVALID, "r3g_meshinside_query: null buffer");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = meshinside_query(c->meshinside.ws.p, c->meshinside.lay, c->meshinside.grid, c->meshinside_axis,
                                    c->meshinside.pairs.as<const int32_t>(), d_points, n_points, d_count, s);
    if (e != hipSuccess) return hip_fail(e, "meshinside_query");
    GridCsrSmall sm;
    int rc = grid_small(c, c->meshinside.ws.p, c->meshinside.lay, "meshinside", s, &sm);
    if (rc) return rc;
    counter_add(LC_MESHINSIDE_TESTS, (int64_t)sm.tests);
    return R3G_OK;
}

// ---- mesh topology ------------------------------------------------------------------------------------------------
static int meshtopo_small(Ctx* c, hipStream_t s, r3g_mt::Small* out) {
    return read_back(c->h_topo, c->meshtopo_ws.p + c->meshtopo_lay.off_small, out, sizeof(r3g_mt::Small), "meshtopo", s);
}

// the build behind r3g_meshtopo_build and r3g_meshtopo_orient (arguments checked by the caller)
static int meshtopo_build(Ctx* c, const char* who, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces,
                          hipStream_t s) {
    c->meshtopo_built = false;
    int rc = c->h_topo.grow(256, s, "meshtopo read-back buffer");
    if (rc) return rc;
    MeshtopoLayout lay;
    if ((rc = c->meshtopo_ws.grow(meshtopo_workspace_bytes(n_verts, n_faces, &lay), s, "meshtopo workspace"))) return rc;
    c->meshtopo_lay = lay;
    hipError_t e = meshtopo_check(c->meshtopo_ws.p, lay, d_verts, n_verts, d_faces, n_faces, s);
    if (e != hipSuccess) return hip_fail(e, "meshtopo_check");
    r3g_mt::Small sm;
    if ((rc = meshtopo_small(c, s, &sm))) return rc;
    // (-2 by the contract of include/r3g.h: found on the device, before anything is read through the index)
    if (sm.bad_index) return fail(-2, "%s: a face index lies outside [0, %lld)", who, (long long)n_verts);
    e = meshtopo_edges(c->meshtopo_ws.p, lay, d_faces, n_faces, s);
    if (e != hipSuccess) return hip_fail(e, "meshtopo_edges");
    int rounds = 0;
    for (;;) {
        if (rounds == r3g_mt::kMaxRounds) {
            counter_add(LC_MESHTOPO_ROUNDS, rounds);
            return fail(R3G_ERR_INVALID, "%s: the body labels still move after %d rounds; no labelling is returned", who, rounds);
        }
        e = meshtopo_round(c->meshtopo_ws.p, lay, n_faces, s);
        if (e != hipSuccess) return hip_fail(e, "meshtopo_round");
        ++rounds;
        if ((rc = meshtopo_small(c, s, &sm))) return rc;
        if (!sm.changed) break;
    }
    e = meshtopo_finish(c->meshtopo_ws.p, lay, d_verts, d_faces, n_faces, s);
    if (e != hipSuccess) return hip_fail(e, "meshtopo_finish");
    if ((rc = meshtopo_small(c, s, &sm))) return rc;      // (also: the caller may free its buffers, a fault would surface here)
    counter_add(LC_MESHTOPO_BUILDS), counter_add(LC_MESHTOPO_ROUNDS, rounds);
    int64_t* r = c->meshtopo_report;
    r[0] = (int64_t)sm.usable, r[1] = (int64_t)sm.skipped, r[2] = (int64_t)sm.vref, r[3] = (int64_t)sm.edges;
    r[4] = (int64_t)sm.boundary, r[5] = (int64_t)sm.clash, r[6] = (int64_t)sm.nonmanifold;
    r[7] = (int64_t)sm.bodies, r[8] = (int64_t)sm.unorientable;
    r[9] = r[2] - r[3] + r[0];
    r[10] = (int64_t)sm.nonfinite;
    r[11] = sm.six_volume_q, r[12] = r3g_mt::vol_scale(sm.max_bits);
    r[13] = sm.two_area_q, r[14] = r3g_mt::area_scale(sm.max_bits);
    r[15] = d_verts ? 1 : 0;
    c->meshtopo_nf = n_faces;
    c->meshtopo_built = true;
    return R3G_OK;
}

static int meshtopo_args(const char* who, const float* d_verts, int64_t n_verts, const void* d_faces, int64_t n_faces) {
    if (n_verts < 0 || n_verts >= (1ll << 31) || n_faces < 0 || n_faces > r3g_mt::kMaxFaces)
        return fail(R3G_ERR_INVALID, "%s: mesh size out of range (at most 2^29 faces)", who);
    if (n_faces == 0) return fail(R3G_ERR_INVALID, "%s: the mesh has no face", who);
    if (!d_faces) return fail(R3G_ERR_INVALID, "%s: null buffer", who);
    (void)d_verts;
    return R3G_OK;
}

int r3g_meshtopo_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces, int64_t* report,
                       void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshtopo_build: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    c->meshtopo_built = false;
    int rc = meshtopo_args("r3g_meshtopo_build", d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    if ((rc = meshtopo_build(c, "r3g_meshtopo_build", d_verts, n_verts, d_faces, n_faces, (hipStream_t)stream))) return rc;
    if (report) memcpy(report, c->meshtopo_report, sizeof c->meshtopo_report);
    return R3G_OK;
}

int r3g_meshtopo_report(r3g_ctx* ctx, int64_t* report) {
    if (!ctx || !report) return fail(R3G_ERR_INVALID, "r3g_meshtopo_report: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshtopo_built) return fail(R3G_ERR_STATE, "r3g_meshtopo_report: no successful r3g_meshtopo_build on this context");
    memcpy(report, c->meshtopo_report, sizeof c->meshtopo_report);
    return R3G_OK;
}

int r3g_meshtopo_mates(r3g_ctx* ctx, int32_t* d_mate, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshtopo_mates: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshtopo_built) return fail(R3G_ERR_STATE, "r3g_meshtopo_mates: no successful r3g_meshtopo_build on this context");
    if (!d_mate) return fail(R3G_ERR_INVALID, "r3g_meshtopo_mates: null buffer");
    hipError_t e = hipMemcpyAsync(d_mate, c->meshtopo_ws.p + c->meshtopo_lay.off_mate, 12 * (size_t)c->meshtopo_nf, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(meshtopo mates)");
    return R3G_OK;
}

int r3g_meshtopo_bodies(r3g_ctx* ctx, int32_t* d_body, uint8_t* d_flip, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshtopo_bodies: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshtopo_built) return fail(R3G_ERR_STATE, "r3g_meshtopo_bodies: no successful r3g_meshtopo_build on this context");
    hipError_t e = hipSuccess;
    if (d_body) e = hipMemcpyAsync(d_body, c->meshtopo_ws.p + c->meshtopo_lay.off_body, 4 * (size_t)c->meshtopo_nf, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess && d_flip)
        e = hipMemcpyAsync(d_flip, c->meshtopo_ws.p + c->meshtopo_lay.off_flip, (size_t)c->meshtopo_nf, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(meshtopo bodies)");
    return R3G_OK;
}

int r3g_meshtopo_orient(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, int32_t* d_faces, int64_t n_faces, int outward,
                        int64_t* faces_reversed, int64_t* bodies_reversed, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshtopo_orient: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    c->meshtopo_built = false;
    int rc = meshtopo_args("r3g_meshtopo_orient", d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    if (outward < 0 || outward > 2) return fail(R3G_ERR_INVALID, "r3g_meshtopo_orient: outward must be 0, 1 or 2");
    if (outward && !d_verts) return fail(R3G_ERR_INVALID, "r3g_meshtopo_orient: outward != 0 needs the vertices");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = meshtopo_build(c, "r3g_meshtopo_orient", d_verts, n_verts, d_faces, n_faces, s))) return rc;
    c->meshtopo_built = false;                    // until the state describes the faces as this call leaves them
    hipError_t e = meshtopo_apply(c->meshtopo_ws.p, c->meshtopo_lay, d_faces, n_faces, outward, s);
    if (e != hipSuccess) return hip_fail(e, "meshtopo_apply");
    r3g_mt::Small sm;
    if ((rc = meshtopo_small(c, s, &sm))) return rc;
    if (sm.faces_reversed) {
        if ((rc = meshtopo_build(c, "r3g_meshtopo_orient", d_verts, n_verts, d_faces, n_faces, s))) return rc;
    } else {
        c->meshtopo_built = true;
    }
    if (faces_reversed) *faces_reversed = (int64_t)sm.faces_reversed;
    if (bodies_reversed) *bodies_reversed = (int64_t)sm.bodies_reversed;
    return R3G_OK;
}

// ---- mesh fill ----------------------------------------------------------------------------------------------------
int r3g_meshfill_plan(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces, int64_t max_loop,
                      int mode, int64_t* report, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshfill_plan: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    c->meshfill_planned = false;
    c->meshtopo_built = false;
    int rc = meshtopo_args("r3g_meshfill_plan", d_verts, n_verts, d_faces, n_faces);
    if (rc) return rc;
    if (max_loop < r3g_mf::kMinLoop) return fail(R3G_ERR_INVALID, "r3g_meshfill_plan: max_loop must be at least 3");
    if (mode != r3g_mf::kModeFan && mode != r3g_mf::kModeCentroid) return fail(R3G_ERR_INVALID, "r3g_meshfill_plan: mode must be 0 (fan) or 1 (centroid)");
    if (mode == r3g_mf::kModeCentroid && !d_verts) return fail(R3G_ERR_INVALID, "r3g_meshfill_plan: mode 1 needs the vertices");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = meshtopo_build(c, "r3g_meshfill_plan", d_verts, n_verts, d_faces, n_faces, s))) return rc;
    const int64_t boundary = c->meshtopo_report[4];
    const int rounds = r3g_mf::rounds_for(boundary);
    r3g_mf::Small sm{};
    MeshfillLayout lay{};
    if (boundary > 0) {
        if ((rc = c->meshfill_ws.grow(meshfill_workspace_bytes(n_verts, n_faces, boundary, &lay), s, "meshfill workspace"))) return rc;
        hipError_t e = meshfill_plan(c->meshfill_ws.p, &lay, (const int32_t*)(c->meshtopo_ws.p + c->meshtopo_lay.off_mate), d_verts, n_verts,
                                     d_faces, rounds, max_loop, mode, s);
        if (e != hipSuccess) return hip_fail(e, "meshfill_plan");
        if ((rc = read_back(c->h_small, c->meshfill_ws.p + lay.off_small, &sm, sizeof sm, "meshfill", s))) return rc;
    }
    counter_add(LC_MESHFILL_PLANS), counter_add(LC_MESHFILL_ROUNDS, 2 * (int64_t)rounds);
    const int64_t verts_added = mode == r3g_mf::kModeCentroid ? (int64_t)sm.filled : 0;
    if (n_verts + verts_added >= (1ll << 31))
        return fail(R3G_ERR_INVALID, "r3g_meshfill_plan: the added vertices do not fit an int32 index");
    int64_t* r = c->meshfill_report;
    memset(r, 0, sizeof c->meshfill_report);
    r[r3g_mf::kRepBoundary] = boundary, r[r3g_mf::kRepLoops] = (int64_t)sm.loops;
    r[r3g_mf::kRepTangled] = boundary - (int64_t)sm.loop_edges, r[r3g_mf::kRepFilled] = (int64_t)sm.filled;
    r[r3g_mf::kRepOversize] = (int64_t)(sm.loops - sm.filled), r[r3g_mf::kRepLongest] = sm.longest;
    r[r3g_mf::kRepLoopEdges] = (int64_t)sm.loop_edges, r[r3g_mf::kRepFacesAdded] = (int64_t)sm.faces_added;
    r[r3g_mf::kRepVertsAdded] = verts_added, r[r3g_mf::kRepRounds] = rounds;
    r[r3g_mf::kRepMaxLoop] = max_loop, r[r3g_mf::kRepMode] = mode, r[r3g_mf::kRepFaces] = n_faces, r[r3g_mf::kRepVerts] = n_verts;
    c->meshfill_lay = lay;
    c->meshfill_planned = true;
    if (report) memcpy(report, r, sizeof c->meshfill_report);
    return R3G_OK;
}

int r3g_meshfill_emit(r3g_ctx* ctx, int32_t* d_new_faces, float* d_new_verts, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshfill_emit: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshfill_planned) return fail(R3G_ERR_STATE, "r3g_meshfill_emit: no successful r3g_meshfill_plan on this context");
    const int64_t* r = c->meshfill_report;
    if (r[r3g_mf::kRepFacesAdded] == 0) return R3G_OK;
    if (!d_new_faces) return fail(R3G_ERR_INVALID, "r3g_meshfill_emit: null buffer");
    hipError_t e = meshfill_emit(c->meshfill_ws.p, c->meshfill_lay, r[r3g_mf::kRepVerts], r[r3g_mf::kRepMaxLoop], (int)r[r3g_mf::kRepMode],
                                 r[r3g_mf::kRepFilled], r[r3g_mf::kRepFacesAdded], d_new_faces, d_new_verts, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "meshfill_emit");
    return R3G_OK;
}

int r3g_meshfill_loops(r3g_ctx* ctx, int64_t* d_loop_start, int32_t* d_loop_verts, int32_t* d_loop_status, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_meshfill_loops: null argument");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c->meshfill_planned) return fail(R3G_ERR_STATE, "r3g_meshfill_loops: no successful r3g_meshfill_plan on this context");
    const int64_t* r = c->meshfill_report;
    if (!d_loop_start || (r[r3g_mf::kRepLoops] && (!d_loop_verts || !d_loop_status)))
        return fail(R3G_ERR_INVALID, "r3g_meshfill_loops: null buffer");
    hipError_t e = meshfill_loops(c->meshfill_ws.p, c->meshfill_lay, r[r3g_mf::kRepMaxLoop], r[r3g_mf::kRepLoops], r[r3g_mf::kRepLoopEdges],
                                  d_loop_start, d_loop_verts, d_loop_status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "meshfill_loops");
    return R3G_OK;
}

// ---- texture stage ------------------------------------------------------------------------------------------------
int r3g_tex_rasterize(r3g_ctx* ctx, const float* d_pos_clip, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height,
                      int width, int32_t* d_findices, float* d_bary, void* stream) {
    if (!ctx || !d_findices || !d_bary) return fail(R3G_ERR_INVALID, "r3g_tex_rasterize: null argument");
    if (height < 1 || width < 1 || height > 16384 || width > 16384)
        return fail(R3G_ERR_INVALID, "r3g_tex_rasterize: image size out of range");
    if (n_verts < 0 || n_faces < 0 || n_faces >= (1ll << 30) || (n_faces && (!d_pos_clip || !d_tri)))
        return fail(R3G_ERR_INVALID, "r3g_tex_rasterize: bad mesh arguments");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = c->tex_ws.grow(8 * (size_t)height * width, (hipStream_t)stream, "z-buffer");
    if (rc) return rc;
    hipError_t e = tex_rasterize(d_pos_clip, d_tri, (int)n_faces, height, width, c->tex_ws.as<unsigned long long>(), d_findices,
                                 d_bary, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_rasterize");
}

int r3g_tex_interpolate(r3g_ctx* ctx, const float* d_attr, int channels, const int32_t* d_tri, const int32_t* d_findices,
                        const float* d_bary, int64_t n_pixels, float* d_out, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_tex_interpolate: null argument");
    if (channels < 1 || channels > 64 || n_pixels < 0) return fail(R3G_ERR_INVALID, "r3g_tex_interpolate: bad sizes");
    if (n_pixels == 0) return R3G_OK;      // nothing to do and no launch; an empty image may come with null buffers
    if (!d_attr || !d_tri || !d_findices || !d_bary || !d_out) return fail(R3G_ERR_INVALID, "r3g_tex_interpolate: null argument");
    hipError_t e = tex_interpolate(d_attr, channels, d_tri, d_findices, d_bary, n_pixels, d_out, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_interpolate");
}

int r3g_tex_view_weight(r3g_ctx* ctx, const int32_t* d_findices, const float* d_depth, const float* d_normal, int height,
                        int width, float cos_threshold, float depth_edge, float view_weight, float power, float* d_weight,
                        void* stream) {
    if (!ctx || !d_findices || !d_depth || !d_normal || !d_weight) return fail(R3G_ERR_INVALID, "r3g_tex_view_weight: null argument");
    if (height < 1 || width < 1) return fail(R3G_ERR_INVALID, "r3g_tex_view_weight: bad sizes");
    hipError_t e = tex_view_weight(d_findices, d_depth, d_normal, height, width, cos_threshold, depth_edge, view_weight, power,
                                   d_weight, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_view_weight");
}

int r3g_tex_bake(r3g_ctx* ctx, const float* d_image, const float* d_weight, const int32_t* d_findices, const float* d_bary,
                 const float* d_uv, const int32_t* d_uv_tri, int64_t n_pixels, int tex_size, uint64_t* d_acc, void* stream) {
    if (!ctx) return fail(R3G_ERR_INVALID, "r3g_tex_bake: null argument");
    if (tex_size < 1 || tex_size > 16384 || n_pixels < 0) return fail(R3G_ERR_INVALID, "r3g_tex_bake: bad sizes");
    if (n_pixels == 0) return R3G_OK;      // nothing to do and no launch; an empty view may come with null buffers
    if (!d_image || !d_weight || !d_findices || !d_bary || !d_uv || !d_uv_tri || !d_acc)
        return fail(R3G_ERR_INVALID, "r3g_tex_bake: null argument");
    hipError_t e = tex_bake(d_image, d_weight, d_findices, d_bary, d_uv, d_uv_tri, n_pixels, tex_size, (unsigned long long*)d_acc,
                            (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_bake");
}

int r3g_tex_bake_gather(r3g_ctx* ctx, const int32_t* d_findices_uv, const float* d_bary_uv, const float* d_clip_uv,
                        const int32_t* d_uv_tri, int tex_size, const float* d_image, const float* d_weight,
                        const int32_t* d_findices, const float* d_depth, int height, int width, float depth_eps, uint64_t* d_acc,
                        void* stream) {
    if (!ctx || !d_findices_uv || !d_bary_uv || !d_clip_uv || !d_uv_tri || !d_image || !d_weight || !d_findices || !d_depth || !d_acc)
        return fail(R3G_ERR_INVALID, "r3g_tex_bake_gather: null argument");
    if (tex_size < 1 || tex_size > 16384 || height < 1 || width < 1) return fail(R3G_ERR_INVALID, "r3g_tex_bake_gather: bad sizes");
    hipError_t e = tex_bake_gather(d_findices_uv, d_bary_uv, d_clip_uv, d_uv_tri, tex_size, d_image, d_weight, d_findices, d_depth,
                                   height, width, depth_eps, (unsigned long long*)d_acc, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_bake_gather");
}

int r3g_tex_bake_finalize(r3g_ctx* ctx, const uint64_t* d_acc, int tex_size, float* d_texture, uint8_t* d_mask, void* stream) {
    if (!ctx || !d_acc || !d_texture || !d_mask) return fail(R3G_ERR_INVALID, "r3g_tex_bake_finalize: null argument");
    if (tex_size < 1 || tex_size > 16384) return fail(R3G_ERR_INVALID, "r3g_tex_bake_finalize: bad sizes");
    hipError_t e = tex_bake_finalize((const unsigned long long*)d_acc, tex_size, d_texture, d_mask, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_bake_finalize");
}

int r3g_tex_inpaint(r3g_ctx* ctx, float* d_texture, uint8_t* d_mask, int tex_size, const int32_t* d_findices_uv,
                    const float* d_bary_uv, const float* d_verts, int64_t n_verts, const int32_t* d_pos_tri, const float* d_uv,
                    const int32_t* d_uv_tri, int64_t n_faces, int dilate_iters, int* rounds_out, void* stream) {
    if (!ctx || !d_texture || !d_mask || !d_findices_uv || !d_bary_uv || !d_verts || !d_pos_tri || !d_uv || !d_uv_tri)
        return fail(R3G_ERR_INVALID, "r3g_tex_inpaint: null argument");
    if (tex_size < 1 || tex_size > 16384 || n_verts < 1 || n_faces < 1 || n_verts >= (1ll << 31) || n_faces >= (1ll << 30) ||
        dilate_iters < 0 || dilate_iters > 4096)
        return fail(R3G_ERR_INVALID, "r3g_tex_inpaint: bad sizes");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = c->tex_ws.grow(tex_inpaint_workspace(n_verts, tex_size), (hipStream_t)stream, "inpaint workspace");
    if (rc) return rc;
    hipError_t e = tex_inpaint(c->tex_ws.p, c->h_small.as<unsigned>(), d_texture, d_mask, tex_size, d_findices_uv, d_bary_uv, d_verts,
                               n_verts, d_pos_tri, d_uv, d_uv_tri, n_faces, dilate_iters, rounds_out, (hipStream_t)stream);
    return e == hipSuccess ? R3G_OK : hip_fail(e, "tex_inpaint");
}

}  // extern "C"
