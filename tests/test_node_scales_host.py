"""The host collapser's node bytes (sr_host_bvh_build / sr_host_bvh_get, no GPU): dwords 3, 10 and 11 of a node hold its three
grid scales as fp32 numbers — pure powers of two 2^e, where e is the exponent the builder derives from the node's extent on
that axis (bvh_build.cpp: the smallest e >= -126 with 2^e >= extent / 255, one more where rounding the planes outward needs
it), so that 255 grid cells span the node. An axis without extent gets the smallest scale, 2^-126."""
import numpy as np
import pytest

from sunray_amd import runtime as rt, scenes


def world_tris(desc):
    out = []
    for key, xs in desc.instances:
        m = next(m for m in desc.meshes if m.key == key)
        p = m.vertices["position"].astype(np.float64)[m.indices.reshape(-1, 3)]
        for x in xs:
            M = np.asarray(x, dtype=np.float64).reshape(3, 4)
            w = (p @ M[:, :3].T + M[:, 3]).astype(np.float32)
            out.append(np.concatenate([w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]], axis=1))
    return np.concatenate(out).astype(np.float32)


def extreme():
    """Extents from 1e-18 to 1e15 and a flat quad (see test_gpu_node_scales.py, which traces this scene on the device)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_node_scales import extreme_scene
    return extreme_scene()


def flat_quad():
    s = scenes.SceneDesc("flat_quad")
    from sunray_amd import abi
    qv, qi = scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(1, qv, qi, abi.material()))
    s.instances = [(1, [abi.IDENTITY_TRANSFORM.copy()])]
    return s


@pytest.mark.parametrize("scene_fn", [scenes.cornell_glass_mirror, lambda: scenes.heightfield(n=48, n_lights=2), extreme, flat_quad])
def test_host_nodes_carry_their_scales_as_powers_of_two_of_their_extent(scene_fn):
    w = world_tris(scene_fn())
    nodes, tris, _, _ = rt.host_bvh(w)
    W, _, po, co = rt.bvh_layout()
    assert W == 4 and po == 4 and co == 12                       # dwords 10, 11 lie between the six plane dwords and the children
    p0 = tris[:, 0:3]
    corners = np.stack([p0, p0 + tris[:, 3:6], p0 + tris[:, 6:9]], axis=1)       # fp32, as the builder bounds a triangle

    def geometry_hi(node):
        """Upper corner of the geometry below `node` (fp32 maxima: exact)."""
        hi = np.full(3, -np.inf, dtype=np.float32)
        for ref in nodes[node, co:co + W].view(np.int32):
            if ref >= 0:
                hi = np.maximum(hi, geometry_hi(int(ref)))
            else:
                v = (~int(ref)) & 0xFFFFFFFF
                first, cnt = v >> 3, v & 7
                if cnt:
                    hi = np.maximum(hi, corners[first:first + cnt].reshape(-1, 3).max(0))
        return hi

    smallest = 0
    for i in range(len(nodes)):
        bits = nodes[i, [3, 10, 11]]
        biased = (bits >> 23).astype(np.int64)
        assert ((bits & 0x807FFFFF) == 0).all() and (biased >= 1).all() and (biased <= 254).all(), (i, bits)   # +2^e, a normal number
        scale = bits.view(np.float32)
        origin = nodes[i, 0:3].view(np.float32)
        lo4, hi4, ch = rt.decode_node(nodes[i])                  # decode_node reads the same three dwords
        hi = geometry_hi(i)
        for a in range(3):
            ext = np.float32(hi[a] - origin[a])
            assert ext > 0                                       # the origin lies strictly below the node's minimum
            q = np.float32(ext / np.float32(255.0))
            fe = int(np.frexp(q)[1]) if q > 0 else -126          # 2^fe > q >= 2^(fe - 1)
            e = int(biased[a]) - 127
            assert max(fe, -126) <= e <= max(fe, -126) + 1, (i, a, ext, fe, e)
            assert scale[a] == np.ldexp(np.float32(1.0), e)
            real = np.array([c >= 0 or ((~int(c)) & 7) != 0 for c in ch])
            assert hi4[real, a].max() >= hi[a] and np.float32(255.0) * scale[a] + origin[a] >= hi[a]   # the byte grid spans the node
            smallest += e == -126
    if scene_fn is flat_quad:
        assert smallest == 1 and len(nodes) == 1                 # the y axis of the quad's only node
