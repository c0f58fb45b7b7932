// surf_common.h -- what the per-cell headers of the two surface extractors (mc_cell.h, dmc_cell.h) have in common: the range
// flags of the count pass and the output transform of a vertex.  Shared by the HIP kernels (device) and by tests/emu (host
// emulation of the launch structure, test-only).  Compile with -ffp-contract=off: the transform is fixed to the bit.
#ifndef R3G_SURF_COMMON_H
#define R3G_SURF_COMMON_H

#ifndef R3G_DEV
#define R3G_DEV static inline
#endif
#ifndef R3G_HOSTDEV
#if defined(__HIPCC__)
#define R3G_HOSTDEV static __host__ __device__ __forceinline__
#else
#define R3G_HOSTDEV static inline
#endif
#endif

// status word of the count pass: the C ABI's level-range test reads it back
#define R3G_SURF_FLAG_LE 1u   // some sample <= level
#define R3G_SURF_FLAG_GE 2u   // some sample >= level
#define R3G_SURF_FLAG_NAN 4u  // some sample is NaN

namespace r3g_surf {

// Output transform, per OUTPUT column (axis0, axis1, axis2).  It is the upstream hy3dgen rescale, applied on the float32
// value in double:  v / grid_size * bbox_size + bbox_min   (surface_extractors.MCSurfaceExtractor.run)
struct Xform {
    double grid_size[3];
    double bbox_size[3];
    double bbox_min[3];
};

// xf9 = {grid_size[3], bbox_size[3], bbox_min[3]} or null (the identity; store_vertex is then called with use_xf = false)
R3G_HOSTDEV Xform xform_from(const double* xf9) {
    Xform xf;
    for (int a = 0; a < 3; ++a) {
        xf.grid_size[a] = xf9 ? xf9[a] : 1.0;
        xf.bbox_size[a] = xf9 ? xf9[3 + a] : 1.0;
        xf.bbox_min[a] = xf9 ? xf9[6 + a] : 0.0;
    }
    return xf;
}

// one vertex from the values of its three output columns: rounded to float32 once, then transformed
R3G_DEV void store_vertex(float* dst, double p0, double p1, double p2, const Xform& xf, bool use_xf) {
    const float o0 = (float)p0, o1 = (float)p1, o2 = (float)p2;
    if (use_xf) {
        dst[0] = (float)((double)o0 / xf.grid_size[0] * xf.bbox_size[0] + xf.bbox_min[0]);
        dst[1] = (float)((double)o1 / xf.grid_size[1] * xf.bbox_size[1] + xf.bbox_min[1]);
        dst[2] = (float)((double)o2 / xf.grid_size[2] * xf.bbox_size[2] + xf.bbox_min[2]);
    } else {
        dst[0] = o0; dst[1] = o1; dst[2] = o2;
    }
}

}  // namespace r3g_surf
#endif
