// Baked clips: the flat tables of a clip and the arithmetic of its evaluation, shared by the host rule (clip_host.cpp) and the
// device kernels (clip_pose.hip, clip_weights.hip, clip_blend.hip, clip_spline_weights.hip, clip_layers.hip, clip_layer_weights.hip). The arithmetic restates GltfLoader::sample_channel, trs_matrix, mul and invert_affine
// (gltf_load.cpp) term for term; host and device are built with -ffp-contract=off, so +, -, *, / and sqrt give the same bits on
// both. atan2 and sin (LINEAR rotations between two keys only) come from each side's own libm; a CUBICSPLINE sample (clip_hermite)
// needs neither, so it is bit equal between host and device without exception.
// No HIP here beyond the function qualifiers.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SR_CLIP_HD __host__ __device__ inline
#else
#define SR_CLIP_HD inline
#endif

namespace srd {

constexpr uint32_t kClipMaxNodes = 384;     // SR_CLIP_MAX_NODES: clip_pose_kernel keeps 12 + 16 floats a node in static LDS (42 KiB)
constexpr uint32_t kClipNoNode = 0xFFFFFFFFu;
constexpr uint32_t kClipTranslation = 0, kClipRotation = 1, kClipScale = 2;
constexpr uint32_t kClipLinear = 0, kClipStep = 1, kClipCubic = 2;   // kClipCubic: a key is three rows, in-tangent, value, out-tangent
constexpr uint32_t kClipTrsWords = 12;      // SrNodeTrs: t[3] q[4] s[3] animated reserved

// One block, as the device holds it: the header, then the tables at the header's byte offsets (each 16-byte aligned).
struct ClipHeader {
    uint32_t n_nodes, n_levels, n_channels, n_skins;
    uint32_t n_joints, n_instances, n_keys, n_values;
    uint32_t nodes, levels, channels, skins;            // ClipNode[n_nodes]; uint32_t[n_levels + 1]: first node of a level; ClipChannel[]; ClipSkin[]
    uint32_t joint_nodes, joint_skins, inverse_bind, instances;   // per joint: clip node, skin (position in `skins`), 12 floats; per instance: clip node
    uint32_t times, values, bytes, reserved;            // float[n_keys], float[n_values]
};
static_assert(sizeof(ClipHeader) == 80, "five 16-byte pieces");
struct ClipNode {
    uint32_t parent, gltf_node, animated, level;        // parent: clip node or kClipNoNode; animated: bit 0 translation, 1 rotation, 2 scale
    float trs[kClipTrsWords];                           // node_trs of the file: t[3] q[4] s[3], then the animated mask's bits and 0
    float matrix[16];                                   // node_matrix of the file, row-major (a node no channel animates composes from it)
};
static_assert(sizeof(ClipNode) == 128, "eight 16-byte pieces");
// first_value: n_keys x COMPS floats (3, or 4 for a rotation); kClipCubic: n_keys x 3 x COMPS, per key in-tangent, value, out-tangent
struct ClipChannel { uint32_t node, path, interpolation, n_keys, first_time, first_value, reserved[2]; };
static_assert(sizeof(ClipChannel) == 32, "two 16-byte pieces");
struct ClipSkin { uint32_t skin, mesh_node, n_joints, first_joint; };   // the file's skin index; clip node; its slice of the joint list
static_assert(sizeof(ClipSkin) == 16, "one 16-byte piece");

// One actor of a call as clip_pose_kernel reads it, at wave-uniform addresses.
struct ClipActorRow {
    const void* clip;           // device: the clip's block
    float time_seconds;
    uint32_t flags;             // bit 0: placement given; bit 1: its instance rows are rows[rows_base + i], else instance_base + i
    uint32_t matrix_base;       // first of its n_joints matrices, in matrices of 48 bytes from the kernel's `matrices`
    uint32_t instance_base, rows_base;
    uint32_t node_base;         // first of its n_nodes records in the kept-nodes buffers
    float placement[12];
};
static_assert(sizeof(ClipActorRow) == 80, "five 16-byte pieces");

// The morph sets of a clip: a second header at ClipHeader.reserved (0: the clip has no set) and its tables, in the same block.
// A set is what morph_weights (gltf_load.cpp) derives for one blas with morph targets, flattened.
constexpr uint32_t kClipMorphAvailable = 0, kClipMorphUnavailable = 1;
struct ClipMorphHeader {
    uint32_t n_sets, n_times, n_values, n_defaults;
    uint32_t sets, times, values, defaults;             // ClipMorphSet[n_sets]; float[n_times]; float[n_values]; float[n_defaults]
};
static_assert(sizeof(ClipMorphHeader) == 32, "two 16-byte pieces");
struct ClipMorphSet {
    uint32_t blas, gltf_node, n_targets, n_keys;        // n_keys 0: no `weights` channel on the node, the defaults
    uint32_t interpolation, first_time, first_value, first_default;   // n_keys times; n_keys x n_targets values, key-major; n_targets defaults
                                                        // kClipCubic: n_keys x 3 x n_targets, per key n_targets in-tangents, values, out-tangents
    uint32_t state, status, reserved[2];                // kClipMorphUnavailable: the loader refused the set with `status`; never sampled
};
static_assert(sizeof(ClipMorphSet) == 48, "three 16-byte pieces");

// One clip-weighted item of a call as clip_weights_kernel reads it, at wave-uniform addresses.
struct ClipWeightRow {
    const void* clip;           // device: the clip's block
    float time_seconds;
    uint32_t set;               // position in the clip's morph sets
    uint32_t active_base;       // the item's slot of n_targets entries in the active arrays
    uint32_t item;              // its PoseBatchItem, whose n_active the kernel writes
    uint32_t check_word;        // the word of the check area that takes the count as well
    uint32_t reserved;
};
static_assert(sizeof(ClipWeightRow) == 32, "two 16-byte pieces");

// One actor of a blended call as clip_blend_kernel reads it, at wave-uniform addresses: two compatible clips (equal tables but
// the channels and the animated masks), each at its own time, and the share of B.
struct ClipBlendActorRow {
    const void* clip_a;         // device: the blocks of the two sources
    const void* clip_b;
    float time_a, time_b, weight;
    uint32_t flags;             // as ClipActorRow.flags
    uint32_t matrix_base, instance_base, rows_base, node_base;      // as ClipActorRow's
    float placement[12];
};
static_assert(sizeof(ClipBlendActorRow) == 96, "six 16-byte pieces");

// One clip-weighted item of a blended call as clip_blend_weights_kernel reads it, at wave-uniform addresses.
struct ClipBlendWeightRow {
    const void* clip_a;         // device: the blocks of the two sources
    const void* clip_b;
    float time_a, time_b, weight;
    uint32_t set_a;             // position in A's morph sets
    uint32_t set_b;             // position in B's morph sets (equal n_targets)
    uint32_t active_base, item, check_word;                         // as ClipWeightRow's
};
static_assert(sizeof(ClipBlendWeightRow) == 48, "three 16-byte pieces");

// One clip-weighted item with a kClipCubic set among its sources as clip_spline_weights_kernel reads it, at wave-uniform
// addresses: an item of a plain call (clip_b is null; time_b, weight and set_b are 0) or of a blended one.
struct ClipSplineWeightRow {
    const void* clip_a;         // device: the block of the source, or of source A
    const void* clip_b;         // device: the block of source B; null for an item of a plain call
    float time_a, time_b, weight;                                   // weight: the share of B
    uint32_t set_a;             // position in A's morph sets
    uint32_t set_b;             // position in B's morph sets (equal n_targets)
    uint32_t active_base, item, check_word;                         // as ClipWeightRow's
};
static_assert(sizeof(ClipSplineWeightRow) == 48, "three 16-byte pieces");

// A layer stack (sr_scene_pose_actors_layered): an actor has 1..kClipMaxLayers layers over compatible clips, applied in order
// onto one accumulated record per node (the rule: clip_additive_record below and clip_blend_record).
constexpr uint32_t kClipMaxLayers = 8;      // SR_CLIP_MAX_LAYERS
constexpr uint32_t kClipLayerOverride = 0, kClipLayerAdditive = 1;   // SR_LAYER_OVERRIDE, SR_LAYER_ADDITIVE
// One layer as clip_layers_kernel reads it, at wave-uniform addresses.
struct ClipLayerRow {
    const void* clip;           // device: the layer's clip block
    const float* mask;          // device: one float per clip node in [0, 1], or null: 1 everywhere
    float time_seconds, ref_time_seconds, weight;      // ref_time_seconds: an additive layer's reference time
    uint32_t mode;              // kClipLayerOverride / kClipLayerAdditive
};
static_assert(sizeof(ClipLayerRow) == 32, "two 16-byte pieces");
// One actor of a layered call: its slice of the call's layer table, and what ClipActorRow holds beside the clip and the time.
struct ClipLayerActorRow {
    uint32_t first_layer, n_layers;                    // layers[first_layer .. first_layer + n_layers); layer 0 is the base
    uint32_t flags;             // as ClipActorRow.flags
    uint32_t matrix_base, instance_base, rows_base, node_base;      // as ClipActorRow's
    uint32_t layer_node_base;   // first of its n_layers x n_nodes records in the kept-layers buffers, layer-major
    float placement[12];
};
static_assert(sizeof(ClipLayerActorRow) == 80, "five 16-byte pieces");
// Where a layered call's results go: one per call, in the upload like the rows, read at wave-uniform addresses where each is
// needed (ten pointers as kernel arguments would stay in scalar registers through the whole sampling loop).
struct ClipLayerTargets {
    const uint32_t* rows;       // the instance rows of the actors that gave some
    void* matrices;             // 48 bytes a matrix: what clip_pose_kernel's `matrices` is
    void* instance_transforms;  // or null: none are written
    uint32_t* check;            // one word per actor
    void* keep_trs;             // or null; SrNodeTrs per node: the final records
    void* keep_globals;         // or null, with keep_trs; 64 bytes per node
    void* keep_cur;             // or null; SrNodeTrs per layer and node: every layer's sampled records
    void* keep_ref;             // or null, with keep_cur; an additive layer's records at its reference time
};
static_assert(sizeof(ClipLayerTargets) == 64, "four 16-byte pieces");

// The key search of sample_channel / morph_weights: the key `i` at or before `time` (clamped to the first / last key) and the
// fraction `u` towards key i + 1 (0: take key i as it is).
SR_CLIP_HD void clip_key_search(const float* times, uint32_t n, uint32_t interpolation, double time, uint32_t* key, double* fraction) {
    uint32_t i = 0;
    double u = 0.0;
    if (time <= (double)times[0]) i = 0;
    else if (time >= (double)times[n - 1]) i = n - 1;
    else {
        uint32_t lo = 0, hi = n - 1;                                              // times[lo] <= time < times[hi]
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if ((double)times[mid] <= time) lo = mid; else hi = mid; }
        i = lo;
        if (interpolation == kClipLinear) u = (time - (double)times[i]) / ((double)times[i + 1] - (double)times[i]);
    }
    *key = i; *fraction = u;
}
// One weight of morph_weights from its two keys: in double from the fp32 keys, rounded once.
SR_CLIP_HD float clip_weight(float key_a, float key_b, double u) {
    const double a = key_a, b = key_b;
    return (float)(u > 0.0 ? a + u * (b - a) : a);
}
// Target k of a set at key i and fraction u; `values` is the set's own slice.
SR_CLIP_HD float clip_weight_at(const float* values, uint32_t n_targets, uint32_t i, double u, uint32_t k) {
    return clip_weight(values[(size_t)i * n_targets + k], values[(size_t)(u > 0.0 ? i + 1 : i) * n_targets + k], u);
}


// CUBICSPLINE (glTF 2.0, appendix C) between key i (value v0, out-tangent b0) and key i + 1 (in-tangent a1, value v1) at the
// fraction u, 0 < u < 1, with td = t[i + 1] - t[i]: the Hermite form in double with exactly this grouping, + - * only. The
// caller rounds the sum once.
SR_CLIP_HD double clip_hermite(double v0, double b0, double v1, double a1, double u, double td) {
    const double u2 = u * u, u3 = u2 * u;
    const double h00 = (2.0 * u3 - 3.0 * u2) + 1.0, h10 = (u3 - 2.0 * u2) + u, h01 = 3.0 * u2 - 2.0 * u3, h11 = u3 - u2;
    return ((h00 * v0 + h10 * (td * b0)) + h01 * v1) + h11 * (td * a1);
}
// clip_key_search for a kClipCubic channel: the same key and fraction as a LINEAR one, and the keys' distance `td`.
SR_CLIP_HD void clip_spline_key_search(const float* times, uint32_t n, double time, uint32_t* key, double* fraction, double* distance) {
    clip_key_search(times, n, kClipLinear, time, key, fraction);
    *distance = *fraction > 0.0 ? (double)times[*key + 1] - (double)times[*key] : 0.0;
}
// One weight of a kClipCubic set from the two keys' rows: u == 0 is the key's value.
SR_CLIP_HD float clip_spline_weight(float v0, float b0, float v1, float a1, double u, double td) {
    return u > 0.0 ? (float)clip_hermite((double)v0, (double)b0, (double)v1, (double)a1, u, td) : v0;
}
// Target k of a kClipCubic set at key i, fraction u and distance td; `values` is the set's own slice, per key n_targets
// in-tangents, values, out-tangents.
SR_CLIP_HD float clip_spline_weight_at(const float* values, uint32_t n_targets, uint32_t i, double u, double td, uint32_t k) {
    const float* key = values + (size_t)i * 3 * n_targets;
    const float* next = u > 0.0 ? key + (size_t)3 * n_targets : key;
    return clip_spline_weight(key[(size_t)n_targets + k], key[(size_t)2 * n_targets + k], next[(size_t)n_targets + k], next[k], u, td);
}

// sample_channel: one channel at `time` (clamped to the first / last key), in double from the fp32 keys, rounded once.
// COMPS 3: translation / scale. COMPS 4: a rotation, slerp along the shorter arc between the normalised keys, normalised.
// kClipCubic: clip_hermite per component of the keys as the file gives them (neither normalised nor sign-flipped); a rotation is
// normalised afterwards in every case, at a key too, and a zero sum stays zero (clip_trs_matrix makes it the identity rotation).
SR_CLIP_HD void clip_normalise(double* q) {
    const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (len > 0.0) for (int c = 0; c < 4; c++) q[c] /= len;
}
template <int COMPS>
SR_CLIP_HD void clip_sample_channel(const float* times, const float* values, uint32_t n, uint32_t interpolation, double time, float* out) {
    uint32_t i = 0;
    double u = 0.0, td = 0.0;
    if (time <= (double)times[0]) i = 0;
    else if (time >= (double)times[n - 1]) i = n - 1;
    else {
        uint32_t lo = 0, hi = n - 1;                                              // times[lo] <= time < times[hi]
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if ((double)times[mid] <= time) lo = mid; else hi = mid; }
        i = lo;
        if (interpolation != kClipStep) { td = (double)times[i + 1] - (double)times[i]; u = (time - (double)times[i]) / td; }
    }
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}, r[4];
    if (interpolation == kClipCubic) {
        const float* key = values + (size_t)i * 3 * COMPS;                        // in-tangent, value, out-tangent
        const float* next = u > 0.0 ? key + 3 * COMPS : key;                      // never past the channel's last key
        for (int c = 0; c < 4; c++) r[c] = 0.0;
        for (int c = 0; c < COMPS; c++)
            r[c] = u > 0.0 ? clip_hermite((double)key[COMPS + c], (double)key[2 * COMPS + c], (double)next[COMPS + c], (double)next[c], u, td) : (double)key[COMPS + c];
        if (COMPS == 4) clip_normalise(r);
        for (int c = 0; c < COMPS; c++) out[c] = (float)r[c];
        return;
    }
    for (int c = 0; c < COMPS; c++) { a[c] = values[(size_t)i * COMPS + c]; b[c] = values[(size_t)(u > 0.0 ? i + 1 : i) * COMPS + c]; }
    if (COMPS == 3) {
        for (int c = 0; c < 3; c++) out[c] = (float)(u > 0.0 ? a[c] + u * (b[c] - a[c]) : a[c]);
        return;
    }
    clip_normalise(a);
    for (int c = 0; c < 4; c++) r[c] = a[c];
    if (u > 0.0) {
        clip_normalise(b);
        if (a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] < 0.0) for (int c = 0; c < 4; c++) b[c] = -b[c];
        double d2 = 0.0, s2 = 0.0;
        for (int c = 0; c < 4; c++) { d2 += (a[c] - b[c]) * (a[c] - b[c]); s2 += (a[c] + b[c]) * (a[c] + b[c]); }
        const double theta = 2.0 * atan2(sqrt(d2), sqrt(s2));
        if (theta < 1e-9) for (int c = 0; c < 4; c++) r[c] = a[c] + u * (b[c] - a[c]);
        else {
            const double wa = sin((1.0 - u) * theta) / sin(theta), wb = sin(u * theta) / sin(theta);
            for (int c = 0; c < 4; c++) r[c] = wa * a[c] + wb * b[c];
        }
        clip_normalise(r);
    }
    for (int c = 0; c < 4; c++) out[c] = (float)r[c];
}

// The cross-fade of two sampled records (SrNodeTrs as twelve words: t[3] q[4] s[3], the animated mask, 0) at the share `w` of B,
// 0 <= w <= 1. Only + - * / and sqrt, in double from the fp32 values and rounded once: no libm, so host and device give the
// same bits without exception.
//   w == 0: A's record, whole, its mask included; w == 1: B's record, whole. Otherwise the mask is A's | B's; where that is 0 the
//   record is A's and the node keeps composing from the file's matrix. Where it is not, each of translation, rotation and scale
//   is taken whole: a part whose bytes are equal in both records is copied (a clip blended with itself at one time is the
//   identity at every weight); otherwise translation and scale are (float)(a + w * (b - a)), and the rotation is a normalised
//   lerp along the shorter arc: b negated where dot(a, b) < 0, r = a + w * (b - a), clip_normalise(r). nlerp and not slerp, on
//   purpose: it keeps atan2 and sin out of the stage.
// A node's local matrix comes from its TRS where the record's mask is not 0 and from the file's matrix otherwise. A node the file
// gives by `matrix` that only one of the clips animates therefore jumps between that matrix and the glTF default TRS at the end
// weights; glTF forbids animating such nodes.
SR_CLIP_HD float clip_word_float(uint32_t v) { float f; __builtin_memcpy(&f, &v, 4); return f; }
SR_CLIP_HD uint32_t clip_float_word(float f) { uint32_t v; __builtin_memcpy(&v, &f, 4); return v; }
SR_CLIP_HD void clip_blend_record(const uint32_t* a, const uint32_t* b, double w, uint32_t* out) {
    const uint32_t mask = a[10] | b[10];
    if (w == 0.0 || w == 1.0 || mask == 0u) {
        const uint32_t* src = w == 1.0 ? b : a;
        for (int i = 0; i < 12; i++) out[i] = src[i];
        return;
    }
    const int first[3] = {0, 3, 7}, count[3] = {3, 4, 3};
    for (int part = 0; part < 3; part++) {
        const int at = first[part], n = count[part];
        bool equal = true;
        for (int c = 0; c < n; c++) equal = equal && a[at + c] == b[at + c];
        if (equal) { for (int c = 0; c < n; c++) out[at + c] = a[at + c]; continue; }
        double x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0}, r[4];
        for (int c = 0; c < n; c++) { x[c] = (double)clip_word_float(a[at + c]); y[c] = (double)clip_word_float(b[at + c]); }
        if (part == 1 && x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3] < 0.0) for (int c = 0; c < 4; c++) y[c] = -y[c];
        for (int c = 0; c < 4; c++) r[c] = x[c] + w * (y[c] - x[c]);
        if (part == 1) clip_normalise(r);
        for (int c = 0; c < n; c++) out[at + c] = clip_float_word((float)r[c]);
    }
    out[10] = mask; out[11] = a[11];
}
// One morph weight of a cross-fade from the two sources' weights: the same form.
SR_CLIP_HD float clip_blend_weight(float wa, float wb, double w) {
    if (w == 0.0 || clip_float_word(wa) == clip_float_word(wb)) return wa;
    if (w == 1.0) return wb;
    return (float)((double)wa + w * ((double)wb - (double)wa));
}

// Layers. An actor has n_layers layers, 1 <= n_layers <= kClipMaxLayers, applied in order onto one accumulated record per node.
// All arithmetic is + - * / and sqrt in double from the fp32 values, rounded once per part, in the grouping written here: no
// libm, so host and device give the same bits without exception, as for clip_blend_record.
//   Effective weight: node n of layer l has w = (double)weight_l * (double)mask_l[n]; the product of two fp32 values is exact in
//   double. mask_l[n] is 1 where the layer has no mask.
//   Layer 0 is the base: its sampled records are the accumulator (override, no mask, weight 1).
//   Override layer: acc[n] = clip_blend_record(acc[n], cur[n], w); cur is the layer's clip sampled at its time.
//   Additive layer: acc[n] = clip_additive_record(acc[n], cur[n], ref[n], w); ref is the same clip sampled at the layer's
//   reference time.
//     1. Where w == 0 or (cur[10] | ref[10]) == 0, out is acc, whole.
//     2. Otherwise each of translation, rotation and scale is taken whole. A part whose bytes are equal in cur and ref is copied
//        from acc: an additive layer at its own reference time is the identity at every weight.
//     3. Translation and scale: (float)(acc + w * (cur - ref)) per component. Additive scale is a sum on purpose: no division,
//        so a zero reference scale is harmless.
//     4. Rotation, q = (x, y, z, w), Hamilton product p (x) q with each component's four terms summed left to right
//        (clip_quat_mul): d = conj(ref) (x) cur; d is negated where d.w < 0; e = (w d.x, w d.y, w d.z, 1 + w (d.w - 1)),
//        clip_normalise(e); out = acc (x) e, clip_normalise(out), rounded to float once.
//     5. out[10] = acc[10] | cur[10] | ref[10]; out[11] = acc[11].
//   A clip's channels never share a node and path, and a part without a channel has equal bytes in cur and ref; so applying
//   clip_additive_part3 / clip_additive_rotation channel by channel onto the accumulator (clip_layers_kernel) gives the node-wise
//   rule's bytes.
// Morph weights. Without SR_ACTORS_LAYER_WEIGHTS they are not layered: an item with SR_ACTOR_CLIP_WEIGHTS(blas) takes its weights
// from the base layer's clip at the base layer's time (clip_weights_kernel / clip_spline_weights_kernel, from rows the host builds
// from layer 0). With the flag they go through the stack (clip_layer_weights_kernel, sr_clip_weights_layers_host), per morph set
// (per blas) and per target k, on fp32 weights, in double in exactly this grouping, each layer's result rounded to fp32 once:
//   Sampling: cur_l[k] is layer l's clip's set for the blas at time_seconds: clip_key_search + clip_weight_at (LINEAR / STEP),
//   clip_spline_key_search + clip_spline_weight_at (cubic), the defaults where n_keys == 0. An additive layer also has ref_l[k],
//   sampled the same way at ref_time_seconds.
//   Effective weight: w_l = (double)weight_l * (double)m, exact; m is layer l's mask value at the clip node whose gltf_node is the
//   set's gltf_node, and 1.0f where the layer has no mask or the clip holds no such node. The host resolves the node once per
//   row (ClipLayerWeightEntry.mask_node); the kernel reads mask[node] only.
//   Base: acc = cur_0. Override layer: acc[k] = clip_blend_weight(acc[k], cur_l[k], w_l). Additive layer: acc[k] =
//   clip_additive_weight(acc[k], cur_l[k], ref_l[k], w_l): acc where w == 0 or the words of cur and ref are equal (an additive
//   layer at its own reference time is the identity at every weight, as for nodes), (float)(acc + w * (cur - ref)) otherwise.
//   Compaction: after the last layer the targets whose weight is +0 or -0 are left out; the rest in ascending target order.
SR_CLIP_HD float clip_additive_weight(float acc, float cur, float ref, double w) {
    if (w == 0.0 || clip_float_word(cur) == clip_float_word(ref)) return acc;
    return (float)((double)acc + w * ((double)cur - (double)ref));
}
// The effective weight of a morph set of a layer from the mask value at the set's node.
SR_CLIP_HD double clip_layer_set_weight(float weight, float mask_value) { return (double)weight * (double)mask_value; }
// One clip-weighted item of a layered call with SR_ACTORS_LAYER_WEIGHTS as clip_layer_weights_kernel reads it, at wave-uniform
// addresses: its actor's slice of the call's ClipLayerRow table and, per layer, an entry of a second table.
struct ClipLayerWeightRow {
    uint32_t first_layer, n_layers;                    // layers[first_layer .. first_layer + n_layers), the actor's
    uint32_t first_entry;                              // entries[first_entry + l] is layer l's
    uint32_t active_base, item, check_word;            // as ClipWeightRow's
    uint32_t reserved[2];
};
static_assert(sizeof(ClipLayerWeightRow) == 32, "two 16-byte pieces");
struct ClipLayerWeightEntry {
    uint32_t set;               // position in the layer's clip's morph sets
    uint32_t mask_node;         // the clip node whose mask value weighs the set, or kClipNoNode: 1
    uint32_t reserved[2];
};
static_assert(sizeof(ClipLayerWeightEntry) == 16, "one 16-byte piece");
SR_CLIP_HD void clip_quat_mul(const double* p, const double* q, double* r) {
    r[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
    r[1] = ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0];
    r[2] = ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3];
    r[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}
// Translation or scale of an additive layer: three words each; w != 0.
SR_CLIP_HD void clip_additive_part3(const uint32_t* acc, const uint32_t* cur, const uint32_t* ref, double w, uint32_t* out) {
    if (cur[0] == ref[0] && cur[1] == ref[1] && cur[2] == ref[2]) { for (int c = 0; c < 3; c++) out[c] = acc[c]; return; }
    for (int c = 0; c < 3; c++)
        out[c] = clip_float_word((float)((double)clip_word_float(acc[c]) + w * ((double)clip_word_float(cur[c]) - (double)clip_word_float(ref[c]))));
}
// The rotation of an additive layer: four words each; w != 0.
SR_CLIP_HD void clip_additive_rotation(const uint32_t* acc, const uint32_t* cur, const uint32_t* ref, double w, uint32_t* out) {
    if (cur[0] == ref[0] && cur[1] == ref[1] && cur[2] == ref[2] && cur[3] == ref[3]) { for (int c = 0; c < 4; c++) out[c] = acc[c]; return; }
    double a[4], conj[4], now[4], d[4], e[4], r[4];
    for (int c = 0; c < 4; c++) { a[c] = (double)clip_word_float(acc[c]); now[c] = (double)clip_word_float(cur[c]); }
    for (int c = 0; c < 3; c++) conj[c] = -(double)clip_word_float(ref[c]);
    conj[3] = (double)clip_word_float(ref[3]);
    clip_quat_mul(conj, now, d);
    if (d[3] < 0.0) for (int c = 0; c < 4; c++) d[c] = -d[c];
    e[0] = w * d[0]; e[1] = w * d[1]; e[2] = w * d[2]; e[3] = 1.0 + w * (d[3] - 1.0);
    clip_normalise(e);
    clip_quat_mul(a, e, r);
    clip_normalise(r);
    for (int c = 0; c < 4; c++) out[c] = clip_float_word((float)r[c]);
}
SR_CLIP_HD void clip_additive_record(const uint32_t* acc, const uint32_t* cur, const uint32_t* ref, double w, uint32_t* out) {
    const uint32_t mask = cur[10] | ref[10];
    if (w == 0.0 || mask == 0u) { for (int i = 0; i < 12; i++) out[i] = acc[i]; return; }
    clip_additive_part3(acc, cur, ref, w, out);
    clip_additive_rotation(acc + 3, cur + 3, ref + 3, w, out + 3);
    clip_additive_part3(acc + 7, cur + 7, ref + 7, w, out + 7);
    out[10] = acc[10] | mask; out[11] = acc[11];
}
// The effective weight of a node of a layer.
SR_CLIP_HD double clip_layer_weight(float weight, const float* mask, uint32_t node) { return (double)weight * (double)(mask ? mask[node] : 1.0f); }

// trs_matrix: translation * rotation * scale, fp32, row-major 4x4.
SR_CLIP_HD void clip_trs_matrix(const float* t, const float* q, const float* s, float* m) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx2 = x2 * x, xy2 = x2 * y, xz2 = x2 * z, yy2 = y2 * y, yz2 = y2 * z, zz2 = z2 * z;
    const float sy2 = y2 * w, sz2 = z2 * w, sx2 = x2 * w;
    const float R[9] = {1.0f - yy2 - zz2, xy2 - sz2, xz2 + sy2,
                        xy2 + sz2, 1.0f - xx2 - zz2, yz2 - sx2,
                        xz2 - sy2, yz2 + sx2, 1.0f - xx2 - yy2};
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m[i * 4 + j] = R[i * 3 + j] * s[j]; m[i * 4 + 3] = t[i]; }
    m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
}

// One row of mul(a, b): the loader's expression on 4x4, k = 0..3 in order.
SR_CLIP_HD void clip_mul_row(const float* a_row, const float* b, float* out) {
    for (int j = 0; j < 4; j++) out[j] = ((a_row[0] * b[j] + a_row[1] * b[4 + j]) + a_row[2] * b[8 + j]) + a_row[3] * b[12 + j];
}
SR_CLIP_HD void clip_mul(const float* a, const float* b, float* out) {
    for (int i = 0; i < 4; i++) clip_mul_row(a + 4 * i, b, out + 4 * i);
}
SR_CLIP_HD void clip_identity(float* m) {
    for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}
// A 3x4 transform as the 4x4 the loader multiplies: the rows, then (0, 0, 0, 1).
SR_CLIP_HD void clip_widen(const float* m12, float* m16) {
    for (int i = 0; i < 12; i++) m16[i] = m12[i];
    m16[12] = 0.0f; m16[13] = 0.0f; m16[14] = 0.0f; m16[15] = 1.0f;
}

// invert_affine: cofactors and determinant in double, rounded once to fp32; the three rows of the inverse. false: singular or
// not finite.
SR_CLIP_HD bool clip_finite(double v) { return v - v == 0.0; }
SR_CLIP_HD bool clip_finite(float v) { return v - v == 0.0f; }
SR_CLIP_HD bool clip_invert_affine(const float* M, float* inv) {
    const double a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double id = 1.0 / det;
    const double R[9] = {c00 * id, (a02 * a21 - a01 * a22) * id, (a01 * a12 - a02 * a11) * id,
                         c01 * id, (a00 * a22 - a02 * a20) * id, (a02 * a10 - a00 * a12) * id,
                         c02 * id, (a01 * a20 - a00 * a21) * id, (a00 * a11 - a01 * a10) * id};
    const double T[3] = {M[3], M[7], M[11]};
    bool finite = clip_finite(id) && det != 0.0;
    for (int row = 0; row < 3; row++) {
        for (int c = 0; c < 3; c++) inv[4 * row + c] = (float)R[3 * row + c];
        inv[4 * row + 3] = (float)(-(R[3 * row] * T[0] + R[3 * row + 1] * T[1] + R[3 * row + 2] * T[2]));
        for (int c = 0; c < 4; c++) finite = finite && clip_finite(inv[4 * row + c]);
    }
    return finite;
}

}  // namespace srd
