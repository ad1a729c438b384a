// Baked clips: the read-outs and the host rule (sr_clip_sample_host, sr_clip_compose_host, sr_clip_pose_host), which
// restates sr_gltf_pose over the flat tables with the arithmetic of clip_rule.h, and the host rule of cross-fades between two clips
// (sr_clip_blend_compatible, sr_clip_blend_host, sr_clip_compose_records_host, sr_clip_pose_blend_host, sr_clip_blend_weights_host),
// and the host rule of layer stacks (sr_clip_subtree_mask, sr_clip_layers_host, sr_clip_pose_layers_host) and of their morph
// weights (sr_clip_layer_weights_host, sr_clip_weights_layers_host).
// No HIP in this file.
#include "clip.h"

#include <cmath>
#include <cstring>

extern "C" {

int sr_clip_destroy(SrClip* clip) { delete clip; return SR_OK; }

int sr_clip_info(const SrClip* clip, SrClipInfo* out) {
    if (!clip || !out) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_info: null argument");
    const srd::ClipHeader& h = clip->header();
    *out = SrClipInfo{clip->animation, h.n_nodes, h.n_levels, h.n_channels, h.n_skins, h.n_joints, h.n_instances, h.n_keys, clip->duration, h.bytes};
    return SR_OK;
}

int sr_clip_skin(const SrClip* clip, uint32_t skin, uint32_t* first_matrix, uint32_t* n_joints) {
    if (!clip) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_skin: null argument");
    for (uint32_t k = 0; k < clip->header().n_skins; k++) {
        const srd::ClipSkin& s = clip->skins()[k];
        if (s.skin != skin) continue;
        if (first_matrix) *first_matrix = s.first_joint;
        if (n_joints) *n_joints = s.n_joints;
        return SR_OK;
    }
    return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_skin: no instanced mesh uses this skin");
}

int sr_clip_layout(const SrClip* clip, SrClipNodeInfo* nodes, SrClipChannelInfo* channels, uint32_t* instance_nodes) {
    if (!clip) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_layout: null argument");
    const srd::ClipHeader& h = clip->header();
    for (uint32_t n = 0; nodes && n < h.n_nodes; n++) { const srd::ClipNode& c = clip->nodes()[n]; nodes[n] = SrClipNodeInfo{c.parent, c.gltf_node, c.animated, c.level}; }
    for (uint32_t k = 0; channels && k < h.n_channels; k++) { const srd::ClipChannel& c = clip->channels()[k]; channels[k] = SrClipChannelInfo{c.node, c.path, c.interpolation, c.n_keys}; }
    if (instance_nodes && h.n_instances) memcpy(instance_nodes, clip->instances(), 4 * (size_t)h.n_instances);
    return SR_OK;
}

int sr_clip_channel_keys(const SrClip* clip, uint32_t channel, const float** times, const float** values) {
    if (!clip) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_channel_keys: null argument");
    if (channel >= clip->header().n_channels) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_channel_keys: channel index out of range");
    const srd::ClipChannel& c = clip->channels()[channel];
    if (times) *times = clip->times() + c.first_time;
    if (values) *values = clip->values() + c.first_value;
    return SR_OK;
}

int sr_clip_morph_count(const SrClip* clip, uint32_t* n_sets) {
    if (!clip || !n_sets) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_morph_count: null argument");
    *n_sets = clip->n_morph_sets();
    return SR_OK;
}

int sr_clip_morph(const SrClip* clip, uint32_t blas, SrClipMorphInfo* out) {
    if (!clip || !out) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_morph: null argument");
    const int k = clip->find_morph_set(blas);
    if (k < 0) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_morph: the clip has no morph set for this blas (it has no morph targets)");
    const srd::ClipMorphSet& s = clip->morph_sets()[k];
    const bool unavailable = s.state == srd::kClipMorphUnavailable;
    *out = SrClipMorphInfo{s.blas, s.gltf_node, s.n_targets, s.n_keys, s.interpolation,
                           unavailable ? SR_CLIP_MORPH_UNAVAILABLE : s.n_keys ? SR_CLIP_MORPH_CHANNEL : SR_CLIP_MORPH_DEFAULTS, unavailable ? (int32_t)s.status : SR_OK, 0};
    if (unavailable) srh::set_error((int32_t)s.status, clip->morph_errors[k]);      // the words, for whoever asks; the call itself succeeds
    return SR_OK;
}

int sr_clip_morph_keys(const SrClip* clip, uint32_t blas, const float** times, const float** values, const float** default_weights) {
    if (!clip) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_morph_keys: null argument");
    const int k = clip->find_morph_set(blas);
    if (k < 0) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_morph_keys: the clip has no morph set for this blas (it has no morph targets)");
    const srd::ClipMorphSet& s = clip->morph_sets()[k];
    if (s.state == srd::kClipMorphUnavailable) return srh::set_error((int32_t)s.status, "sr_clip_morph_keys: " + clip->morph_errors[k]);
    if (times) *times = s.n_keys ? clip->morph_times() + s.first_time : nullptr;
    if (values) *values = s.n_keys ? clip->morph_values() + s.first_value : nullptr;
    if (default_weights) *default_weights = clip->morph_defaults() + s.first_default;
    return SR_OK;
}

// sr_gltf_morph_weights restated over the baked set: its checks in its order, its statuses and its words.
static int weights_of(const SrClip* clip, float time_seconds, uint32_t blas, float* weights_out, uint32_t n_targets, const std::string& who) {
    if (!clip || (!weights_out && n_targets)) return srh::set_error(SR_ERR_INVALID_ARG, who + ": null argument");
    const int k = clip->find_morph_set(blas);
    if (k < 0) return srh::set_error(SR_ERR_INVALID_ARG, who + ": the clip has no morph set for this blas (it has no morph targets)");
    const srd::ClipMorphSet& s = clip->morph_sets()[k];
    const bool unavailable = s.state == srd::kClipMorphUnavailable;
    if (unavailable && s.n_targets == 0) return srh::set_error((int32_t)s.status, who + ": " + clip->morph_errors[k]);    // the morph parse itself
    if (n_targets != s.n_targets) return srh::set_error(SR_ERR_INVALID_ARG, who + ": gltf: another number of weights asked for than the blas has morph targets");
    if (clip->animation >= 0 && !std::isfinite(time_seconds)) return srh::set_error(SR_ERR_INVALID_ARG, who + ": gltf: the time of a pose must be finite");
    if (unavailable) return srh::set_error((int32_t)s.status, who + ": " + clip->morph_errors[k]);
    if (s.n_keys == 0) { memcpy(weights_out, clip->morph_defaults() + s.first_default, 4 * (size_t)n_targets); return SR_OK; }
    uint32_t i = 0;
    double u = 0.0, td = 0.0;
    const float* values = clip->morph_values() + s.first_value;
    if (s.interpolation == srd::kClipCubic) {
        srd::clip_spline_key_search(clip->morph_times() + s.first_time, s.n_keys, (double)time_seconds, &i, &u, &td);
        for (uint32_t t = 0; t < n_targets; t++) weights_out[t] = srd::clip_spline_weight_at(values, n_targets, i, u, td, t);
        return SR_OK;
    }
    srd::clip_key_search(clip->morph_times() + s.first_time, s.n_keys, s.interpolation, (double)time_seconds, &i, &u);
    for (uint32_t t = 0; t < n_targets; t++) weights_out[t] = srd::clip_weight_at(values, n_targets, i, u, t);
    return SR_OK;
}

int sr_clip_weights_host(const SrClip* clip, float time_seconds, uint32_t blas, float* weights_out, uint32_t n_targets) {
    return weights_of(clip, time_seconds, blas, weights_out, n_targets, "sr_clip_weights_host");
}

int sr_clip_sample_host(const SrClip* clip, float time_seconds, SrNodeTrs* out) {
    if (!clip || !out) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_sample_host: null argument");
    if (clip->animation >= 0 && !std::isfinite(time_seconds)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_sample_host: gltf: the time of a pose must be finite");
    const srd::ClipHeader& h = clip->header();
    for (uint32_t n = 0; n < h.n_nodes; n++) memcpy(&out[n], clip->nodes()[n].trs, sizeof(SrNodeTrs));
    for (uint32_t k = 0; k < h.n_channels; k++) {
        const srd::ClipChannel& c = clip->channels()[k];
        SrNodeTrs& t = out[c.node];
        const float* times = clip->times() + c.first_time;
        const float* values = clip->values() + c.first_value;
        if (c.path == srd::kClipRotation) srd::clip_sample_channel<4>(times, values, c.n_keys, c.interpolation, (double)time_seconds, t.rotation);
        else srd::clip_sample_channel<3>(times, values, c.n_keys, c.interpolation, (double)time_seconds, c.path == srd::kClipTranslation ? t.translation : t.scale);
    }
    return SR_OK;
}

// The composition of both sr_clip_compose_host (a node composes from its TRS where the clip animates it) and
// sr_clip_compose_records_host (where the record's own mask says so).
static int compose(const SrClip* clip, const SrNodeTrs* trs, const SrTransform* placement, SrTransform* joint_matrices, SrTransform* instance_transforms,
                   uint32_t* singular_skin, bool record_masks, const std::string& who) {
    if (!clip || !trs) return srh::set_error(SR_ERR_INVALID_ARG, who + ": null argument");
    const srd::ClipHeader& h = clip->header();
    if (singular_skin) *singular_skin = 0xFFFFFFFFu;
    std::vector<float> global(16 * (size_t)h.n_nodes);
    float ident[16], local[16];
    srd::clip_identity(ident);
    for (uint32_t n = 0; n < h.n_nodes; n++) {                  // parents come first, level by level
        const srd::ClipNode& c = clip->nodes()[n];
        if (record_masks ? trs[n].animated : c.animated) srd::clip_trs_matrix(trs[n].translation, trs[n].rotation, trs[n].scale, local);
        else memcpy(local, c.matrix, 64);
        srd::clip_mul(c.parent == srd::kClipNoNode ? ident : &global[16 * (size_t)c.parent], local, &global[16 * (size_t)n]);
    }
    if (instance_transforms) {
        float place[16], m[16];
        if (placement) srd::clip_widen(placement->m, place);
        for (uint32_t i = 0; i < h.n_instances; i++) {
            const float* g = &global[16 * (size_t)clip->instances()[i]];
            if (placement) { srd::clip_mul(place, g, m); g = m; }
            memcpy(instance_transforms[i].m, g, 48);
        }
    }
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t k = 0; joint_matrices && k < h.n_skins; k++) {       // as sr_gltf_pose: nobody inverts where no joint matrices are asked for
        const srd::ClipSkin& s = clip->skins()[k];
        float inv[16], ibm[16], a[16], j[16];
        srd::clip_identity(inv);
        if (!srd::clip_invert_affine(&global[16 * (size_t)s.mesh_node], inv)) { if (bad == 0xFFFFFFFFu) bad = k; continue; }
        for (uint32_t q = 0; q < s.n_joints; q++) {
            srd::clip_widen(clip->inverse_bind() + 12 * (size_t)(s.first_joint + q), ibm);
            srd::clip_mul(inv, &global[16 * (size_t)clip->joint_nodes()[s.first_joint + q]], a);
            srd::clip_mul(a, ibm, j);
            memcpy(joint_matrices[s.first_joint + q].m, j, 48);
        }
    }
    if (singular_skin) *singular_skin = bad;
    if (bad != 0xFFFFFFFFu) return srh::set_error(SR_ERR_UNSUPPORTED, who + ": gltf: the transform of the skinned mesh's node is singular");
    return SR_OK;
}

int sr_clip_compose_host(const SrClip* clip, const SrNodeTrs* trs, const SrTransform* placement, SrTransform* joint_matrices, SrTransform* instance_transforms,
                         uint32_t* singular_skin) {
    return compose(clip, trs, placement, joint_matrices, instance_transforms, singular_skin, false, "sr_clip_compose_host");
}

int sr_clip_compose_records_host(const SrClip* clip, const SrNodeTrs* trs, const SrTransform* placement, SrTransform* joint_matrices,
                                 SrTransform* instance_transforms, uint32_t* singular_skin) {
    return compose(clip, trs, placement, joint_matrices, instance_transforms, singular_skin, true, "sr_clip_compose_records_host");
}

int sr_clip_pose_host(const SrClip* clip, float time_seconds, const SrTransform* placement, SrTransform* joint_matrices, SrTransform* instance_transforms) {
    if (!clip) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_host: null argument");
    if (clip->animation >= 0 && !std::isfinite(time_seconds)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_host: gltf: the time of a pose must be finite");
    std::vector<SrNodeTrs> trs(clip->header().n_nodes);
    int rc = sr_clip_sample_host(clip, time_seconds, trs.data());
    if (rc != SR_OK) return rc;
    rc = sr_clip_compose_host(clip, trs.data(), placement, joint_matrices, instance_transforms, nullptr);
    if (rc == SR_ERR_UNSUPPORTED) return srh::set_error(rc, "sr_clip_pose_host: gltf: the transform of the skinned mesh's node is singular");
    return rc;
}

// ---- cross-fades: the host rule of sr_scene_pose_actors_blended ---------------------------------------------------------------------
// Two clips blend where everything but their channels and animated masks is equal: in practice, bakes of one file.
int sr_clip_blend_compatible(const SrClip* a, const SrClip* b) {
    if (!a || !b) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_blend_compatible: null argument");
    const auto differ = [](const char* table) { return srh::set_error(SR_ERR_INVALID_ARG, std::string("sr_clip_blend_compatible: the clips differ in ") + table); };
    const srd::ClipHeader& ha = a->header();
    const srd::ClipHeader& hb = b->header();
    if (ha.n_nodes != hb.n_nodes) return differ("the number of nodes");
    if (ha.n_levels != hb.n_levels || memcmp(a->levels(), b->levels(), 4 * ((size_t)ha.n_levels + 1)) != 0) return differ("the level table");
    if (ha.n_instances != hb.n_instances || memcmp(a->instances(), b->instances(), 4 * (size_t)ha.n_instances) != 0) return differ("the instance table");
    for (uint32_t n = 0; n < ha.n_nodes; n++) {
        const srd::ClipNode& x = a->nodes()[n];
        const srd::ClipNode& y = b->nodes()[n];
        if (x.parent != y.parent || x.gltf_node != y.gltf_node || x.level != y.level || memcmp(x.trs, y.trs, 40) != 0 || memcmp(x.matrix, y.matrix, 64) != 0)
            return differ("the node table");
    }
    if (ha.n_skins != hb.n_skins || memcmp(a->skins(), b->skins(), sizeof(srd::ClipSkin) * (size_t)ha.n_skins) != 0) return differ("the skin table");
    if (ha.n_joints != hb.n_joints || memcmp(a->joint_nodes(), b->joint_nodes(), 4 * (size_t)ha.n_joints) != 0) return differ("the joint nodes");
    if (memcmp(a->joint_skins(), b->joint_skins(), 4 * (size_t)ha.n_joints) != 0) return differ("the joint skins");
    if (memcmp(a->inverse_bind(), b->inverse_bind(), 48 * (size_t)ha.n_joints) != 0) return differ("the inverse bind matrices");
    return SR_OK;
}

static bool blend_weight_ok(float weight) { return weight >= 0.0f && weight <= 1.0f; }     // false for a NaN

int sr_clip_blend_host(const SrNodeTrs* trs_a, const SrNodeTrs* trs_b, uint32_t n_nodes, float weight, SrNodeTrs* out) {
    if (n_nodes && (!trs_a || !trs_b || !out)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_blend_host: null argument");
    if (!blend_weight_ok(weight)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_blend_host: the weight is not in [0, 1]");
    for (uint32_t n = 0; n < n_nodes; n++) {
        uint32_t a[srd::kClipTrsWords], b[srd::kClipTrsWords], r[srd::kClipTrsWords];
        memcpy(a, &trs_a[n], sizeof(a)); memcpy(b, &trs_b[n], sizeof(b));
        srd::clip_blend_record(a, b, (double)weight, r);
        memcpy(&out[n], r, sizeof(r));
    }
    return SR_OK;
}

int sr_clip_pose_blend_host(const SrClip* a, float time_a, const SrClip* b, float time_b, float weight, const SrTransform* placement,
                            SrTransform* joint_matrices, SrTransform* instance_transforms) {
    if (!a || !b) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_blend_host: null argument");
    if ((a->animation >= 0 && !std::isfinite(time_a)) || (b->animation >= 0 && !std::isfinite(time_b)))
        return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_blend_host: gltf: the time of a pose must be finite");
    if (!blend_weight_ok(weight)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_blend_host: the weight is not in [0, 1]");
    int rc = sr_clip_blend_compatible(a, b);
    if (rc != SR_OK) return rc;
    const uint32_t n = a->header().n_nodes;
    std::vector<SrNodeTrs> ta(n), tb(n), blended(n);
    if ((rc = sr_clip_sample_host(a, time_a, ta.data())) != SR_OK || (rc = sr_clip_sample_host(b, time_b, tb.data())) != SR_OK) return rc;
    if ((rc = sr_clip_blend_host(ta.data(), tb.data(), n, weight, blended.data())) != SR_OK) return rc;
    return compose(a, blended.data(), placement, joint_matrices, instance_transforms, nullptr, true, "sr_clip_pose_blend_host");
}

int sr_clip_blend_weights_host(const SrClip* a, float time_a, const SrClip* b, float time_b, float weight, uint32_t blas, float* weights_out, uint32_t n_targets) {
    if (!a || !b || (!weights_out && n_targets)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_blend_weights_host: null argument");
    if (!blend_weight_ok(weight)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_blend_weights_host: the weight is not in [0, 1]");
    std::vector<float> wa(n_targets), wb(n_targets);
    int rc;
    if ((rc = weights_of(a, time_a, blas, wa.data(), n_targets, "sr_clip_blend_weights_host")) != SR_OK) return rc;
    if ((rc = weights_of(b, time_b, blas, wb.data(), n_targets, "sr_clip_blend_weights_host")) != SR_OK) return rc;
    for (uint32_t t = 0; t < n_targets; t++) weights_out[t] = srd::clip_blend_weight(wa[t], wb[t], (double)weight);
    return SR_OK;
}

// ---- layers: the host rule of sr_scene_pose_actors_layered -----------------------------------------------------------------------
static_assert(SR_CLIP_MAX_LAYERS == srd::kClipMaxLayers && SR_LAYER_OVERRIDE == srd::kClipLayerOverride && SR_LAYER_ADDITIVE == srd::kClipLayerAdditive,
              "the header states the rule's constants");
static_assert(sizeof(SrClipLayer) == 32 && sizeof(SrClipLayerRule) == 16 && sizeof(SrClipLayerActor) == 40 && sizeof(SrLayerPoseInfo) == 32, "the header states these sizes");

int sr_clip_subtree_mask(const SrClip* clip, uint32_t gltf_node, float inside, float outside, float* out, uint32_t n_nodes) {
    if (!clip || !out) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_subtree_mask: null argument");
    const srd::ClipHeader& h = clip->header();
    if (n_nodes != h.n_nodes) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_subtree_mask: room for another number of nodes than the clip has");
    bool found = false;
    std::vector<char> in(h.n_nodes, 0);
    for (uint32_t n = 0; n < h.n_nodes; n++) {                  // parents come first
        const srd::ClipNode& c = clip->nodes()[n];
        in[n] = c.gltf_node == gltf_node || (c.parent != srd::kClipNoNode && in[c.parent]);
        found = found || c.gltf_node == gltf_node;
    }
    if (!found) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_subtree_mask: the clip does not hold this glTF node");
    for (uint32_t n = 0; n < h.n_nodes; n++) out[n] = in[n] ? inside : outside;
    return SR_OK;
}

// What a stack's rule refuses, wherever the stack comes from: `who` names the caller, `layer` the words in front of a layer's refusal.
static int check_layer_rule(uint32_t l, float weight, uint32_t mode, bool masked, const std::string& who) {
    if (!blend_weight_ok(weight)) return srh::set_error(SR_ERR_INVALID_ARG, who + "the weight is not in [0, 1]");
    if (mode != SR_LAYER_OVERRIDE && mode != SR_LAYER_ADDITIVE) return srh::set_error(SR_ERR_INVALID_ARG, who + "unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)");
    if (l == 0 && (mode != SR_LAYER_OVERRIDE || masked || weight != 1.0f))
        return srh::set_error(SR_ERR_INVALID_ARG, who + "the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1");
    return SR_OK;
}
static bool mask_values_ok(const float* mask, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) if (!blend_weight_ok(mask[i])) return false;
    return true;
}

int sr_clip_layers_host(const SrNodeTrs* const* cur, const SrNodeTrs* const* ref, const SrClipLayerRule* rule, uint32_t n_layers, uint32_t n_nodes, SrNodeTrs* out) {
    if (!cur || !rule || (n_nodes && !out)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_layers_host: null argument");
    if (n_layers == 0 || n_layers > SR_CLIP_MAX_LAYERS) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_layers_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]");
    for (uint32_t l = 0; l < n_layers; l++) {
        const std::string who = "sr_clip_layers_host: layer " + std::to_string(l) + ": ";
        const int rc = check_layer_rule(l, rule[l].weight, rule[l].mode, rule[l].mask != nullptr, who);
        if (rc != SR_OK) return rc;
        if (n_nodes && (!cur[l] || (rule[l].mode == SR_LAYER_ADDITIVE && (!ref || !ref[l])))) return srh::set_error(SR_ERR_INVALID_ARG, who + "null argument (the sampled records)");
        if (rule[l].mask && !mask_values_ok(rule[l].mask, n_nodes)) return srh::set_error(SR_ERR_INVALID_ARG, who + "the mask has a value that is not in [0, 1]");
    }
    for (uint32_t n = 0; n < n_nodes; n++) {
        uint32_t acc[srd::kClipTrsWords], c[srd::kClipTrsWords], r[srd::kClipTrsWords], next[srd::kClipTrsWords];
        memcpy(acc, &cur[0][n], sizeof(acc));
        for (uint32_t l = 1; l < n_layers; l++) {
            const double w = srd::clip_layer_weight(rule[l].weight, rule[l].mask, n);
            memcpy(c, &cur[l][n], sizeof(c));
            if (rule[l].mode == SR_LAYER_ADDITIVE) { memcpy(r, &ref[l][n], sizeof(r)); srd::clip_additive_record(acc, c, r, w, next); }
            else srd::clip_blend_record(acc, c, w, next);
            memcpy(acc, next, sizeof(acc));
        }
        memcpy(&out[n], acc, sizeof(acc));
    }
    return SR_OK;
}

int sr_clip_pose_layers_host(const SrClip* const* clips, const SrClipLayer* layers, const float* const* masks, uint32_t n_layers, const SrTransform* placement,
                             SrTransform* joint_matrices, SrTransform* instance_transforms) {
    if (!clips || !layers) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_layers_host: null argument");
    if (n_layers == 0 || n_layers > SR_CLIP_MAX_LAYERS) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_layers_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]");
    for (uint32_t l = 0; l < n_layers; l++) if (!clips[l]) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_pose_layers_host: null argument");
    const uint32_t n = clips[0]->header().n_nodes;
    std::vector<std::vector<SrNodeTrs>> cur(n_layers), ref(n_layers);
    std::vector<const SrNodeTrs*> cur_at(n_layers), ref_at(n_layers, nullptr);
    std::vector<SrClipLayerRule> rule(n_layers);
    int rc;
    for (uint32_t l = 0; l < n_layers; l++) {
        const std::string who = "sr_clip_pose_layers_host: layer " + std::to_string(l) + ": ";
        const SrClipLayer& ly = layers[l];
        const float* mask = masks ? masks[l] : nullptr;
        if ((rc = check_layer_rule(l, ly.weight, ly.mode, mask != nullptr, who)) != SR_OK) return rc;
        const bool additive = ly.mode == SR_LAYER_ADDITIVE;
        if (clips[l]->animation >= 0 && (!std::isfinite(ly.time_seconds) || (additive && !std::isfinite(ly.ref_time_seconds))))
            return srh::set_error(SR_ERR_INVALID_ARG, who + "gltf: the time of a pose must be finite");
        if (l && clips[l] != clips[0] && (rc = sr_clip_blend_compatible(clips[0], clips[l])) != SR_OK) return rc;      // in that function's words
        if (mask && !mask_values_ok(mask, n)) return srh::set_error(SR_ERR_INVALID_ARG, who + "the mask has a value that is not in [0, 1]");
        cur[l].resize(n);
        if ((rc = sr_clip_sample_host(clips[l], ly.time_seconds, cur[l].data())) != SR_OK) return rc;
        if (additive) { ref[l].resize(n); if ((rc = sr_clip_sample_host(clips[l], ly.ref_time_seconds, ref[l].data())) != SR_OK) return rc; ref_at[l] = ref[l].data(); }
        cur_at[l] = cur[l].data();
        rule[l] = SrClipLayerRule{ly.weight, ly.mode, mask};
    }
    std::vector<SrNodeTrs> stacked(n);
    if ((rc = sr_clip_layers_host(cur_at.data(), ref_at.data(), rule.data(), n_layers, n, stacked.data())) != SR_OK) return rc;
    return compose(clips[0], stacked.data(), placement, joint_matrices, instance_transforms, nullptr, true, "sr_clip_pose_layers_host");
}

// ---- layered morph weights: the host rule of sr_scene_pose_actors_layered with SR_ACTORS_LAYER_WEIGHTS ----------------------------
static_assert(SR_ACTORS_LAYER_WEIGHTS == 8u && sizeof(SrLayerWeightsInfo) == 32, "the header states these");

int sr_clip_layer_weights_host(const float* const* cur, const float* const* ref, const float* weight, const uint32_t* mode, const float* mask_value,
                               uint32_t n_layers, uint32_t n_targets, float* out) {
    if (!cur || !weight || !mode || (n_targets && !out)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_layer_weights_host: null argument");
    if (n_layers == 0 || n_layers > SR_CLIP_MAX_LAYERS) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_layer_weights_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]");
    for (uint32_t l = 0; l < n_layers; l++) {
        const std::string who = "sr_clip_layer_weights_host: layer " + std::to_string(l) + ": ";
        // a mask value of 1 is what a layer without a mask has: the base layer may state it
        const int rc = check_layer_rule(l, weight[l], mode[l], l == 0 && mask_value && mask_value[0] != 1.0f, who);
        if (rc != SR_OK) return rc;
        if (n_targets && (!cur[l] || (mode[l] == SR_LAYER_ADDITIVE && (!ref || !ref[l])))) return srh::set_error(SR_ERR_INVALID_ARG, who + "null argument (the sampled weights)");
        if (mask_value && !blend_weight_ok(mask_value[l])) return srh::set_error(SR_ERR_INVALID_ARG, who + "the mask value is not in [0, 1]");
    }
    for (uint32_t k = 0; k < n_targets; k++) {
        float acc = cur[0][k];
        for (uint32_t l = 1; l < n_layers; l++) {
            const double w = srd::clip_layer_set_weight(weight[l], mask_value ? mask_value[l] : 1.0f);
            acc = mode[l] == SR_LAYER_ADDITIVE ? srd::clip_additive_weight(acc, cur[l][k], ref[l][k], w) : srd::clip_blend_weight(acc, cur[l][k], w);
        }
        out[k] = acc;
    }
    return SR_OK;
}

int sr_clip_weights_layers_host(const SrClip* const* clips, const SrClipLayer* layers, const float* const* masks, uint32_t n_layers, uint32_t blas,
                                float* weights_out, uint32_t n_targets) {
    if (!clips || !layers || (!weights_out && n_targets)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_weights_layers_host: null argument");
    if (n_layers == 0 || n_layers > SR_CLIP_MAX_LAYERS) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_weights_layers_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]");
    for (uint32_t l = 0; l < n_layers; l++) if (!clips[l]) return srh::set_error(SR_ERR_INVALID_ARG, "sr_clip_weights_layers_host: null argument");
    std::vector<std::vector<float>> cur(n_layers), ref(n_layers);
    std::vector<const float*> cur_at(n_layers), ref_at(n_layers, nullptr);
    std::vector<float> weight(n_layers), mask_value(n_layers, 1.0f);
    std::vector<uint32_t> mode(n_layers);
    int rc;
    for (uint32_t l = 0; l < n_layers; l++) {
        const std::string who = "sr_clip_weights_layers_host: layer " + std::to_string(l);
        const SrClipLayer& ly = layers[l];
        const SrClip& clip = *clips[l];
        const float* mask = masks ? masks[l] : nullptr;
        if ((rc = check_layer_rule(l, ly.weight, ly.mode, mask != nullptr, who + ": ")) != SR_OK) return rc;
        const bool additive = ly.mode == SR_LAYER_ADDITIVE;
        if (clip.animation >= 0 && (!std::isfinite(ly.time_seconds) || (additive && !std::isfinite(ly.ref_time_seconds))))
            return srh::set_error(SR_ERR_INVALID_ARG, who + ": gltf: the time of a pose must be finite");
        if (l && clips[l] != clips[0] && (rc = sr_clip_blend_compatible(clips[0], clips[l])) != SR_OK) return rc;      // in that function's words
        if (mask && !mask_values_ok(mask, clip.header().n_nodes)) return srh::set_error(SR_ERR_INVALID_ARG, who + ": the mask has a value that is not in [0, 1]");
        const int k = clip.find_morph_set(blas);
        if (l && k >= 0 && clip.morph_sets()[k].state != srd::kClipMorphUnavailable && clip.morph_sets()[k].n_targets != n_targets)
            return srh::set_error(SR_ERR_INVALID_ARG, who + ": the set has " + std::to_string(clip.morph_sets()[k].n_targets) + " targets, the base layer's " + std::to_string(n_targets));
        cur[l].resize(n_targets);
        if ((rc = weights_of(&clip, ly.time_seconds, blas, cur[l].data(), n_targets, who)) != SR_OK) return rc;
        if (additive) { ref[l].resize(n_targets); if ((rc = weights_of(&clip, ly.ref_time_seconds, blas, ref[l].data(), n_targets, who)) != SR_OK) return rc; ref_at[l] = ref[l].data(); }
        cur_at[l] = cur[l].data();
        weight[l] = ly.weight; mode[l] = ly.mode;
        if (mask) {                                              // the clip node of the set's glTF node; a clip without it: 1
            const uint32_t node = clip.find_node(clip.morph_sets()[k].gltf_node);
            if (node != srd::kClipNoNode) mask_value[l] = mask[node];
        }
    }
    return sr_clip_layer_weights_host(cur_at.data(), ref_at.data(), weight.data(), mode.data(), mask_value.data(), n_layers, n_targets, weights_out);
}

}  // extern "C"
