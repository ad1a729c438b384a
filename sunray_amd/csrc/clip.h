// A baked clip on the host (sr_gltf_bake_clip): the block of clip_rule.h, which is also what sr_scene_attach_clip uploads.
// No HIP here: a stand-alone program links gltf_load.cpp and clip_host.cpp and brings srh::set_error.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sunray_hip.h"
#include "clip_rule.h"

static_assert(srd::kClipMaxNodes == SR_CLIP_MAX_NODES, "the header states the kernel's cap");
static_assert(sizeof(SrNodeTrs) == 4 * srd::kClipTrsWords, "a node's TRS is three 16-byte pieces");

struct SrClip {
    int32_t animation = -1;
    float duration = 0.0f;
    std::vector<uint32_t> block;        // ClipHeader, then the tables

    const srd::ClipHeader& header() const { return *(const srd::ClipHeader*)block.data(); }
    template <class T> const T* table(uint32_t offset) const { return (const T*)((const unsigned char*)block.data() + offset); }
    const srd::ClipNode* nodes() const { return table<srd::ClipNode>(header().nodes); }
    const uint32_t* levels() const { return table<uint32_t>(header().levels); }
    const srd::ClipChannel* channels() const { return table<srd::ClipChannel>(header().channels); }
    const srd::ClipSkin* skins() const { return table<srd::ClipSkin>(header().skins); }
    const uint32_t* joint_nodes() const { return table<uint32_t>(header().joint_nodes); }
    const uint32_t* joint_skins() const { return table<uint32_t>(header().joint_skins); }
    const float* inverse_bind() const { return table<float>(header().inverse_bind); }
    const uint32_t* instances() const { return table<uint32_t>(header().instances); }
    const float* times() const { return table<float>(header().times); }
    const float* values() const { return table<float>(header().values); }

    // the morph sets (the second header, at ClipHeader.reserved; none where that is 0) and, host only, the loader's words for
    // every unavailable set, by position
    std::vector<std::string> morph_errors;
    uint32_t n_morph_sets() const { return header().reserved ? morph_header().n_sets : 0u; }
    const srd::ClipMorphHeader& morph_header() const { return *table<srd::ClipMorphHeader>(header().reserved); }
    const srd::ClipMorphSet* morph_sets() const { return table<srd::ClipMorphSet>(morph_header().sets); }
    const float* morph_times() const { return table<float>(morph_header().times); }
    const float* morph_values() const { return table<float>(morph_header().values); }
    const float* morph_defaults() const { return table<float>(morph_header().defaults); }
    // the set of a blas -> its position, or -1
    int find_morph_set(uint32_t blas) const {
        for (uint32_t k = 0; k < n_morph_sets(); k++) if (morph_sets()[k].blas == blas) return (int)k;
        return -1;
    }
    // the clip node of a glTF node (the first in clip-node order), or kClipNoNode
    uint32_t find_node(uint32_t gltf_node) const {
        for (uint32_t n = 0; n < header().n_nodes; n++) if (nodes()[n].gltf_node == gltf_node) return n;
        return srd::kClipNoNode;
    }
};

namespace srh {

int set_error(int code, const std::string& msg);   // the library's error slot (api.cpp); returns `code`

// The parts of a clip as the bake collects them.
struct ClipParts {
    std::vector<srd::ClipNode> nodes;               // parent before child, grouped by level
    std::vector<uint32_t> levels;                   // n_levels + 1 entries
    std::vector<srd::ClipChannel> channels;         // first_time / first_value index `times` / `values`
    std::vector<float> times, values;
    std::vector<srd::ClipSkin> skins;
    std::vector<uint32_t> joint_nodes, joint_skins, instances;
    std::vector<SrTransform> inverse_bind;
    std::vector<srd::ClipMorphSet> morph_sets;      // first_time / first_value / first_default index the three tables below
    std::vector<float> morph_times, morph_values, morph_defaults;
    std::vector<std::string> morph_errors;          // one per set; empty where the set is available
};

// One block from the parts: the header, then every table at a 16-byte boundary. Inline: the loader (gltf_load.cpp) links alone.
inline uint32_t clip_align16(size_t n) { return (uint32_t)((n + 15u) & ~(size_t)15u); }
template <class T> uint32_t clip_place(std::vector<unsigned char>& bytes, const std::vector<T>& v) {
    const uint32_t at = (uint32_t)bytes.size();
    bytes.resize(at + clip_align16(sizeof(T) * v.size()), 0);
    if (!v.empty()) memcpy(bytes.data() + at, v.data(), sizeof(T) * v.size());
    return at;
}
inline void clip_assemble(const ClipParts& p, SrClip& clip) {
    std::vector<unsigned char> bytes(sizeof(srd::ClipHeader), 0);
    srd::ClipHeader h{};
    h.n_nodes = (uint32_t)p.nodes.size(); h.n_levels = (uint32_t)p.levels.size() - 1; h.n_channels = (uint32_t)p.channels.size(); h.n_skins = (uint32_t)p.skins.size();
    h.n_joints = (uint32_t)p.joint_nodes.size(); h.n_instances = (uint32_t)p.instances.size(); h.n_keys = (uint32_t)p.times.size(); h.n_values = (uint32_t)p.values.size();
    h.nodes = clip_place(bytes, p.nodes); h.levels = clip_place(bytes, p.levels); h.channels = clip_place(bytes, p.channels); h.skins = clip_place(bytes, p.skins);
    h.joint_nodes = clip_place(bytes, p.joint_nodes); h.joint_skins = clip_place(bytes, p.joint_skins); h.inverse_bind = clip_place(bytes, p.inverse_bind);
    h.instances = clip_place(bytes, p.instances); h.times = clip_place(bytes, p.times); h.values = clip_place(bytes, p.values);
    if (!p.morph_sets.empty()) {                    // a clip without morph sets is the block it has always been
        srd::ClipMorphHeader m{};
        m.n_sets = (uint32_t)p.morph_sets.size(); m.n_times = (uint32_t)p.morph_times.size(); m.n_values = (uint32_t)p.morph_values.size(); m.n_defaults = (uint32_t)p.morph_defaults.size();
        h.reserved = (uint32_t)bytes.size();
        bytes.resize(bytes.size() + sizeof(m), 0);
        m.sets = clip_place(bytes, p.morph_sets); m.times = clip_place(bytes, p.morph_times); m.values = clip_place(bytes, p.morph_values); m.defaults = clip_place(bytes, p.morph_defaults);
        memcpy(bytes.data() + h.reserved, &m, sizeof(m));
    }
    clip.morph_errors = p.morph_errors;
    h.bytes = (uint32_t)bytes.size();
    memcpy(bytes.data(), &h, sizeof(h));
    clip.block.assign(bytes.size() / 4, 0u);
    memcpy(clip.block.data(), bytes.data(), bytes.size());
}

}  // namespace srh
