// geo_narrow.h -- the fused tail of a NARROW geo decoder (geo_narrow.hip): for a decoder of width 256 everything
// behind the cross-attention -- c_proj + residual, ln_3, mlp.c_fc, GELU, mlp.c_proj + residual, ln_post, output_proj -- is one launch
// per pass.  At that width the chain is HBM traffic and launches, not MFMA work; its intermediate results stay in registers.
#ifndef R3G_GEO_NARROW_H
#define R3G_GEO_NARROW_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace r3g {

constexpr int GEO_TAIL_WIDTH = 256;

// the shapes the fused tail exists for: width 256, hidden 256 | 512 | 1024
inline bool geo_tail_supported(int width, int hidden) {
    return width == GEO_TAIL_WIDTH && (hidden == 256 || hidden == 512 || hidden == 1024);
}

// The three weight matrices in the order and lane layout in which the kernel consumes them: a stream of 1 KiB MFMA operand
// fragments (64 lanes x 8 bf16), 128 for c_proj, then per 32 hidden units 16 of mlp.c_fc and 16 of mlp.c_proj.
inline size_t geo_tail_packed_bytes(int hidden) { return (size_t)(128 + hidden) * 1024; }

// c_proj [256][256], mlp.c_fc [hidden][256], mlp.c_proj [256][hidden] (bf16, row-major with the given leading dimensions) -> packed
hipError_t geo_tail_pack_launch(const uint16_t* w_proj, int64_t ld_proj, const uint16_t* w_fc, int64_t ld_fc, const uint16_t* w_fp,
                                int64_t ld_fp, int hidden, void* packed, hipStream_t s);

struct GeoTailArgs {
    const uint16_t* cat; int64_t ld_cat;      // attention output, bf16 [n][256]
    const uint16_t* x0; int64_t ld_x0;        // start of the residual stream, bf16 [n][256]
    const void* packed;                       // geo_tail_pack_launch's result
    const float *b_proj, *ln3_w, *ln3_b, *b_fc, *b_fp;   // f32 [256] | [256] | [256] | [hidden] | [256]
    const float *lnp_w, *lnp_b;               // ln_post f32 [256] each, or both null: no ln_post
    const float* out_w; float out_b;          // output_proj f32 [256] and its bias
    int hidden, n;
    float* out;                               // f32 [n]
};
// logits of rows [0, n): rows past n are neither read nor stored
hipError_t geo_tail_launch(const GeoTailArgs& p, hipStream_t s);

}  // namespace r3g
#endif
