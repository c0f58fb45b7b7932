// plane_kernels.h -- launchers of the plane fit (the definition is plane_core.h)
#ifndef R3G_PLANE_KERNELS_H
#define R3G_PLANE_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef R3G_PL_HD
#define R3G_PL_HD static inline
#endif
#include "plane_core.h"

namespace r3g {

// what a call reads back: 192 bytes behind everything it queued
struct PlaneSmall {
    unsigned long long usable;     // rows with three finite coordinates
    unsigned long long key;        // r3g_pl::winner_key of the winner, 0 without one
    unsigned valid;                // valid hypotheses
    unsigned pad;
    r3g_pl::Hyp best;              // the winner's entry of the table (valid = 0 without one)
    r3g_pl::Moments mom;
};

// one chunk's sums (plane_core.h, summation order)
struct PlanePartial {
    unsigned long long n, skipped;
    double v[6];
};

struct PlaneLayout {
    size_t off_small, off_hyp, off_count, off_mask, off_partial, total;
};

// own_count / own_mask: the call has no buffer of the caller's for the counts / the mask and keeps them in the workspace (the
// regions are empty otherwise: the mask alone is n_points bytes)
size_t plane_workspace_bytes(int64_t n_points, int64_t n_hyp, bool own_count, bool own_mask, PlaneLayout* lay);

// zeroes the small record (a memset, no kernel), then the table and the zeroed counts: one launch (none when n_hyp == 0)
hipError_t plane_table(char* ws, const PlaneLayout& lay, const float* points, int64_t n, const int32_t* triples, int n_hyp, uint32_t* count,
                       hipStream_t s);
// the count pass: count[h] and the usable rows; one launch (none when n == 0)
hipError_t plane_count(char* ws, const PlaneLayout& lay, const float* points, int64_t n, int n_hyp, double threshold, uint32_t* count,
                       int num_cu, hipStream_t s);
// arg-max over the table (one block) and the winner's mask over the rows: two launches
hipError_t plane_winner(char* ws, const PlaneLayout& lay, const float* points, int64_t n, int n_hyp, double threshold, const uint32_t* count,
                        uint8_t* mask, hipStream_t s);
// the moments of the rows selected by mask (all rows when NULL) into small->mom: four launches (sums, their tree, scatter, its tree)
hipError_t plane_moments(char* ws, const PlaneLayout& lay, const float* points, int64_t n, const uint8_t* mask, hipStream_t s);

}  // namespace r3g
#endif
