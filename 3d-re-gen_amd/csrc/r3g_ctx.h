// r3g_ctx.h -- per-device context behind the opaque r3g_ctx of include/r3g.h
#ifndef R3G_CTX_H
#define R3G_CTX_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cloud_kernels.h"
#include "dbscan_kernels.h"
#include "dev_buf.h"
#include "dmc_kernels.h"
#include "events.h"
#include "facecloud_kernels.h"
#include "hier_kernels.h"
#include "kernels.h"
#include "mc_kernels.h"
#include "meshdist_kernels.h"
#include "meshfill_kernels.h"
#include "meshfit_kernels.h"
#include "meshinside_kernels.h"
#include "meshtopo_kernels.h"
#include "orient_kernels.h"
#include "plane_kernels.h"
#include "recon_kernels.h"
#include "softras_kernels.h"

namespace r3g {

// Every buffer below is a DevBuf (dev_buf.h) and every event a PassTimer's (events.h): they go with the context, and none of them is
// released by hand.
struct Ctx {
    int device = 0;
    int num_cu = 0;
    DevBuf h_small{true};     // pinned, 64 B: read-back of tiny device results
    // marching cubes and dual marching cubes (SurfState: surf_compact_kernels.h): a caller may hold a counted state of each at once
    SurfState mc, dmc;
    // mesh cleaners
    DevBuf mesh_ws;
    // mesh distance: the grid of the last r3g_meshdist_build (records, CSR starts; the pair list has its own buffer)
    GridCsrState<3> meshdist;
    // mesh registration: the partial records of a fit step, and the pinned buffer its result is read back through (the sums
    // do not fit h_small); both made on first use
    DevBuf meshfit_ws, h_fit{true};
    // point in mesh: the columns of the last r3g_meshinside_build (separate from the distance grid: both may be held at once)
    GridCsrState<2> meshinside;
    int meshinside_axis = 0;
    // point clouds: the grid of the last r3g_cloud_build; its `pairs` buffer holds the packed points in cell order (r3g_cl::Pt),
    // not ids.  Independent of the two grids above: all three may be held at once
    GridCsrState<3> cloud;
    // Poisson surface: the int64 channels of the last r3g_recon_splat and the solver's float32 lattices (recon_kernels.h)
    ReconState recon;
    // normal orientation: the rows, labels and parities of one r3g_cloud_orient (nothing is kept between calls but the buffer)
    DevBuf orient_ws;
    // DBSCAN: the flags, roots, numbers and sizes of one r3g_cloud_dbscan (nothing is kept between calls but the buffer), and the
    // events around the passes of the last call (events.h; made on first use; dbscan_timed: they bracket a complete run)
    DevBuf dbscan_ws;
    PassTimer<kDbscanPasses + 2> dbscan_ev;
    bool dbscan_timed = false;
    // plane fit: the table, counts, mask and partial sums of one r3g_plane_ransac / r3g_plane_moments (nothing is kept between calls
    // but the buffer); h_plane is the pinned buffer its record is read back through (it does not fit h_small), made on first use;
    // the events bracket the passes of the last r3g_plane_ransac (plane_timed: a complete run)
    DevBuf plane_ws, h_plane{true};
    PassTimer<r3g_pl::kPasses + 1> plane_ev;
    bool plane_timed = false;
    // soft silhouette: the record, per-tile counts, starts and cursors of one r3g_softras_forward / _backward, and the (face, tile)
    // pairs of the forward (nothing is kept between calls but the buffers); events [0..2] bracket the bin and forward passes of the
    // last forward, [3..5] the backward and gather passes of the last backward (softras_fwd_timed / _bwd_timed: a complete call)
    DevBuf softras_ws, softras_pairs;
    PassTimer<6> softras_ev;
    bool softras_fwd_timed = false, softras_bwd_timed = false;
    // face-to-cloud distance: the record, face records and wide list of one r3g_cloud_faces (nothing is kept between calls but the
    // buffer; the cloud it reads is `cloud` above, which it leaves alone); events [0..3] bracket the classify, narrow and wide passes
    // of the last forward, [4..5] the gather of the last backward (facecloud_fwd_timed / _bwd_timed: a complete call)
    DevBuf facecloud_ws;
    PassTimer<6> facecloud_ev;
    bool facecloud_fwd_timed = false, facecloud_bwd_timed = false;
    // mesh topology: mates, bodies, flips and sums of the last r3g_meshtopo_build (a state of its own: the distance grid and the
    // columns above may be held at the same time); h_topo is the pinned buffer its counts are read back through (they do not
    // fit h_small), made on first use
    DevBuf meshtopo_ws, h_topo{true};
    MeshtopoLayout meshtopo_lay{};
    int64_t meshtopo_nf = 0;
    int64_t meshtopo_report[16] = {0};
    bool meshtopo_built = false;
    // mesh fill: the slots, loops and scans of the last r3g_meshfill_plan (a state of its own again; the plan also leaves the
    // topology state above describing its input mesh)
    DevBuf meshfill_ws;
    MeshfillLayout meshfill_lay{};
    int64_t meshfill_report[16] = {0};
    bool meshfill_planned = false;
    // texture stage (z-buffer / inpainting workspace)
    DevBuf tex_ws;

    // hierarchical volume decoder: mask / prefix of the last r3g_hier_select
    DevBuf hier_ws;
    HierLayout hier_lay{};
    int64_t hier_count = 0;
    bool hier_selected = false;

    // 3 x 3 convolutions: 256 bytes of zeros, where conv_gemm_kernel points the taps that lie outside the image.  Made on first use
    // (r3g_unet_create, r3g_op_conv3x3), never written afterwards
    DevBuf conv_zero;

    void* model = nullptr;  // r3g::Model (model.cpp)
    void release_model();
    void* unet = nullptr;   // r3g::Unet (unet.cpp)
    void release_unet();
};

// the planner steps behind r3g_hier_select / _indices / _merge (r3g_api.cpp); r3g_grid_query_hier drives them too
int hier_select(Ctx* c, const float* d_coarse, int n_coarse, double level, double band, int is_finest, int64_t* count, hipStream_t s);
int hier_indices(Ctx* c, int32_t* d_idx_out, hipStream_t s);
int hier_merge(Ctx* c, const float* d_coarse, const float* d_values, float* d_fine_out, hipStream_t s);
int hier_unsafe_cells(Ctx* c, const float* d_fine, double level, int64_t* count, hipStream_t s);

}  // namespace r3g
#endif
