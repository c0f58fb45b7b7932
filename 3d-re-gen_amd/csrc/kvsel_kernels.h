// kvsel_kernels.h -- adaptive top-k selection of the geo decoder's cross-attention keys (kvsel_kernels.hip).  The algorithm is
// defined in DESIGN.md section 4d: per group of consecutive query points and per head, the keys are scored by the dot product
// with the mean of the group's sampled query rows, the k best are kept in ascending key index, and the attention of the group
// runs over their gathered K / V^T.  Head dimension 64 throughout; every tensor is bf16 unless it says otherwise.
#ifndef R3G_KVSEL_KERNELS_H
#define R3G_KVSEL_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace r3g {

// the rule behind option "geo_kv_topk" = -1 ([UPSTREAM-RECALLED]): 1024 of 3072 latents, 256 of 512, otherwise a third
inline int kvsel_upstream_topk(int num_latents) {
    return num_latents == 3072 ? 1024 : num_latents == 512 ? 256 : num_latents / 3;
}

// the cut of n consecutive rows into groups of `group`: `full` complete groups and a tail of `tail` rows (0: none) whose slab
// has tail_pad = rup(tail, 128) rows
struct KvselCut {
    int full, tail, tail_pad, groups;
};
inline KvselCut kvsel_cut(int n, int group) {
    KvselCut c;
    c.full = n / group;
    c.tail = n % group;
    c.tail_pad = (c.tail + 127) / 128 * 128;
    c.groups = c.full + (c.tail ? 1 : 0);
    return c;
}
// elements of the grouped Q of n rows: [full][H][group][64] followed by the tail's [H][tail_pad][64]
inline int64_t kvsel_grouped_elems(int n, int group, int heads) {
    const KvselCut c = kvsel_cut(n, group);
    return ((int64_t)c.full * group + c.tail_pad) * heads * 64;
}

// Q [H][lq_pad][64] -> [full][H][group][64] | [H][tail_pad][64] (16-byte copies; rows of the tail's slab past lq_pad are zero)
hipError_t kvsel_regroup_launch(const uint16_t* q, int heads, int lq, int lq_pad, int group, uint16_t* out, hipStream_t s);
// idx int32 [groups][H][topk]: per (group, head) the topk keys of largest score, ascending.  Q in the [H][lq_pad][64] layout, K
// [H][lk_pad][64].  1 <= topk <= lk, group % 256 == 0, stride >= 1, lk * 4 + 2 KiB of LDS (lk <= 15360).
hipError_t kvsel_select_launch(const uint16_t* q, int lq, int lq_pad, const uint16_t* k, int lk, int lk_pad, int heads, int group,
                               int stride, int topk, int32_t* idx, hipStream_t s);
// V [H][lk][64] (row-major) from V^T [H][64][lk_pad] in the attention kernel's key order (kernels.h vt_key_pos)
hipError_t kvsel_vrows_launch(const uint16_t* vt, int lk, int lk_pad, int heads, uint16_t* v, hipStream_t s);
// K_out [groups][H][kpad][64] = K[idx], Vt_out [groups][H][64][kpad] = V[idx] transposed, compact key j at vt_key_pos(j);
// kpad = rup(topk, 64), padded keys zero.  v: the row-major copy kvsel_vrows_launch made.
hipError_t kvsel_gather_launch(const uint16_t* k, const uint16_t* v, int lk, int lk_pad, int heads, const int32_t* idx, int groups,
                               int topk, uint16_t* k_out, uint16_t* vt_out, hipStream_t s);

}  // namespace r3g
#endif
