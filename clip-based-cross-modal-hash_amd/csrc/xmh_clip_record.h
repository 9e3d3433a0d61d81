// The per-layer record of xmh_clip_blocks_forward_saved (include/xmh.h, xmh_clip_saved) and the shape of a CLIP residual block, stated
// once for the forward that writes the record (xmh_forward.hip) and the backward that reads it (xmh_block_grad.hip).  Python cannot
// include this: xmh/models/clip.py restates the field order as Transformer.SAVED_FIELDS.
//
// What a backward pass of ResidualAttentionBlock (models/CLIP/model.py:167-197) needs from the forward, per layer and in this order
// (M = B L tokens, D = width):
//   x_in [M,D] | ln1 [M,D] | qkv [M,3D] | attn [M,D] | x_mid [M,D] | ln2 [M,D] | fc_pre [M,4D] | fc_act [M,4D]
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/xmh.h"

namespace xmh {

constexpr int kSavedFloatsPerElement = 16;           // per (token, channel): 1 + 1 + 3 + 1 + 1 + 1 + 4 + 4

inline size_t saved_record_bytes(int layers, int64_t M, int D) { return (size_t)layers * kSavedFloatsPerElement * (size_t)M * D * sizeof(float); }

template <typename T>                                // float (the forward writes) or const float (the backward reads)
struct SavedRecord {
    T *x_in, *ln1, *qkv, *attn, *x_mid, *ln2, *fc_pre, *fc_act;
};

template <typename T>
inline SavedRecord<T> saved_record(T* base, int layer, int64_t M, int D) {
    const size_t md = (size_t)M * D;
    T* p = base + (size_t)layer * kSavedFloatsPerElement * md;
    return {p, p + md, p + 2 * md, p + 5 * md, p + 6 * md, p + 7 * md, p + 8 * md, p + 12 * md};
}

// in_proj [3D, D], out_proj [D, D], c_fc [4D, D], c_proj [D, 4D]
inline bool block_fits(const xmh_clip_block& b, int D) {
    return b.qkv.n == 3 * D && b.qkv.k == D && b.out.n == D && b.out.k == D && b.fc.k == D && b.fc.n == 4 * D && b.proj.n == D && b.proj.k == b.fc.n;
}

}  // namespace xmh
