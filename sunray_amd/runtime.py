"""Thin Python harness over the C ABI (include/sunray_hip.h) for tests and bench.py.

PyTorch is used only as plumbing: device memory (torch tensors as frame buffers), the current HIP
stream, and torch.distributed for the multi-GPU gather. Every compute call goes through
libsunray_hip.so; there is no CPU or torch fallback.
"""
import ctypes as C

import numpy as np

from . import abi
from ._lib import SunrayError, check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _device_vertices(tensor, device_index):
    """(address, vertex count) of a torch tensor that holds abi.VERTEX records on cuda:`device_index`; ValueError for anything
    the library would have to refuse or could not read (a CPU tensor, another device, gaps, a size that is no whole vertices)."""
    if not getattr(tensor, "is_cuda", False):
        raise ValueError("update_mesh_device: the vertices must be a tensor on the scene's GPU, not host memory")
    if tensor.device.index != device_index:
        raise ValueError("update_mesh_device: the tensor is on %s, the scene on cuda:%d" % (tensor.device, device_index))
    if not tensor.is_contiguous():
        raise ValueError("update_mesh_device: the tensor must be contiguous")
    nbytes = tensor.numel() * tensor.element_size()
    if nbytes == 0 or nbytes % abi.VERTEX.itemsize:
        raise ValueError("update_mesh_device: %d bytes are not a whole number of %d-byte vertices" % (nbytes, abi.VERTEX.itemsize))
    return C.c_void_p(tensor.data_ptr()), nbytes // abi.VERTEX.itemsize


def _device_transforms(layout, tensor, device_index):
    """(keys, counts, address) of an instance list whose transforms are a torch tensor on cuda:`device_index`: `layout` is
    [(key, count), ...], `tensor` contiguous float32 with sum(counts) x 12 elements (row-major 3x4); ValueError for anything the
    library would have to refuse or could not read."""
    keys = np.array([k for k, _ in layout], dtype=np.uint64)
    counts = np.array([c for _, c in layout], dtype=np.uint32)
    n = int(counts.sum())
    if not getattr(tensor, "is_cuda", False):
        raise ValueError("set_instances_device: the transforms must be a tensor on the scene's GPU, not host memory")
    if tensor.device.index != device_index:
        raise ValueError("set_instances_device: the tensor is on %s, the scene on cuda:%d" % (tensor.device, device_index))
    if str(tensor.dtype) != "torch.float32" or not tensor.is_contiguous():
        raise ValueError("set_instances_device: the tensor must be contiguous float32")
    if tensor.numel() != n * 12:
        raise ValueError("set_instances_device: %d elements are not %d transforms of 12" % (tensor.numel(), n))
    return keys, counts, C.c_void_p(tensor.data_ptr() if n else 0)


def _frame_flags(normals, tangents):
    """abi.FRAME_* of set_mesh_frame's two switches; ValueError for tangents without normals (the library would refuse it)."""
    if tangents and not normals:
        raise ValueError("set_mesh_frame: tangents need normals (the tangent is made orthogonal to the new normal)")
    return (abi.FRAME_NORMALS if normals else 0) | (abi.FRAME_TANGENTS if tangents else 0)


def _mesh_positions(positions, device_index):
    """The positions of update_mesh_positions -> (on_device, address, vertex count, stream or None, what keeps the memory alive):
    a contiguous float32 [n, 3] torch tensor on cuda:`device_index` goes to the device call (with torch's current stream), a
    float32 [n, 3] numpy array to the host call. ValueError for anything else: another dtype (no silent narrowing of float64),
    another shape, gaps, a CPU tensor, another device."""
    who = "update_mesh_positions"
    if isinstance(positions, np.ndarray):
        if positions.dtype != np.dtype(np.float32):
            raise ValueError("%s: the positions must be float32 (%s given)" % (who, positions.dtype))
        if positions.ndim != 2 or positions.shape[1] != 3 or len(positions) == 0:
            raise ValueError("%s: the positions must have shape (n_vertices, 3) (shape %s given)" % (who, positions.shape))
        a = np.ascontiguousarray(positions)
        return False, _p(a), len(a), None, a
    if not hasattr(positions, "data_ptr") or not hasattr(positions, "is_cuda"):
        raise ValueError("%s: the positions must be a torch tensor on the scene's GPU or a numpy array" % who)
    import torch
    if positions.dtype != torch.float32:
        raise ValueError("%s: the positions must be float32 (%s given)" % (who, positions.dtype))
    if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] == 0:
        raise ValueError("%s: the positions must have shape (n_vertices, 3) (shape %s given)" % (who, tuple(positions.shape)))
    if not positions.is_cuda:
        raise ValueError("%s: a torch tensor must be on the scene's GPU (a numpy array goes to the host call)" % who)
    if positions.device.index != device_index:
        raise ValueError("%s: the tensor is on %s, the scene on cuda:%d" % (who, positions.device, device_index))
    if not positions.is_contiguous():
        raise ValueError("%s: the tensor must be contiguous" % who)
    return True, C.c_void_p(positions.data_ptr()), positions.shape[0], C.c_void_p(torch.cuda.current_stream(positions.device).cuda_stream), positions


def mesh_frame_adjacency(vertices, indices):
    """The smoothing groups of a mesh as the runs set_mesh_frame uploads -> (offsets [n + 1] uint32, entries uint32, side [n]
    float32) (sr_mesh_frame_adjacency). Host only."""
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
    i = np.ascontiguousarray(indices, dtype=np.uint32)
    n = C.c_uint32()
    check(lib().sr_mesh_frame_adjacency(_p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), None, None, None, C.byref(n)))
    offsets, entries, side = np.zeros(len(v) + 1, dtype=np.uint32), np.zeros(max(n.value, 1), dtype=np.uint32), np.zeros(max(len(v), 1), dtype=np.float32)
    check(lib().sr_mesh_frame_adjacency(_p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(offsets), _p(entries), _p(side), C.byref(n)))
    return offsets, entries[: n.value], side[: len(v)]


def mesh_frame_host(vertices, indices, positions, normals=True, tangents=False):
    """update_mesh_positions on the host: the records a mesh with `vertices` as reference records takes from `positions` (float32
    [n, 3]), byte for byte the device's (sr_mesh_frame_host). Host only."""
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
    i = np.ascontiguousarray(indices, dtype=np.uint32)
    if not isinstance(positions, np.ndarray) or positions.dtype != np.dtype(np.float32) or positions.shape != (len(v), 3):
        raise ValueError("mesh_frame_host: the positions must be a float32 numpy array of shape (%d, 3)" % len(v))
    p = np.ascontiguousarray(positions)
    out = np.zeros(len(v), dtype=abi.VERTEX)
    check(lib().sr_mesh_frame_host(_p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(p), C.c_uint32(_frame_flags(normals, tangents)), _p(out), None))
    return out


def _skin_influences(influences):
    """The influences of set_mesh_skin as a contiguous abi.SKIN_INFLUENCE array; ValueError for anything else (no conversion: a
    float array read as records would attach nonsense)."""
    if not isinstance(influences, np.ndarray) or influences.dtype != abi.SKIN_INFLUENCE:
        raise ValueError("set_mesh_skin: the influences must be a numpy array of abi.SKIN_INFLUENCE records")
    if influences.ndim != 1 or len(influences) == 0:
        raise ValueError("set_mesh_skin: the influences must be one record per vertex, in one dimension (shape %s given)" % (influences.shape,))
    return np.ascontiguousarray(influences)


def _joint_matrices(matrices):
    """The joint matrices of skin_mesh as a contiguous float32 array of n_joints rows of 3x4 -> (array, n_joints); ValueError for
    another dtype (no silent narrowing of float64) or shape."""
    if not isinstance(matrices, np.ndarray) or matrices.dtype not in (np.dtype(np.float32), abi.TRANSFORM):
        raise ValueError("skin_mesh: the joint matrices must be a numpy float32 array (or abi.TRANSFORM records)")
    if matrices.dtype == abi.TRANSFORM:
        ok = matrices.ndim == 1
    else:
        ok = (matrices.ndim == 2 and matrices.shape[1] == 12) or (matrices.ndim == 3 and matrices.shape[1:] == (3, 4))
    if not ok or len(matrices) == 0:
        raise ValueError("skin_mesh: the joint matrices must be (n_joints, 12) or (n_joints, 3, 4), row-major 3x4 (shape %s given)" % (matrices.shape,))
    return np.ascontiguousarray(matrices), len(matrices)


def _morph_deltas(deltas):
    """The deltas of set_mesh_morph as a contiguous abi.MORPH_DELTA array of shape (n_targets, n_vertices) -> (array, n_targets,
    n_vertices); ValueError for anything else (no conversion: a float array read as records would attach nonsense)."""
    if not isinstance(deltas, np.ndarray) or deltas.dtype != abi.MORPH_DELTA:
        raise ValueError("set_mesh_morph: the deltas must be a numpy array of abi.MORPH_DELTA records")
    if deltas.ndim != 2 or deltas.shape[0] == 0 or deltas.shape[1] == 0:
        raise ValueError("set_mesh_morph: the deltas must be target-major, shape (n_targets, n_vertices) (shape %s given)" % (deltas.shape,))
    return np.ascontiguousarray(deltas), deltas.shape[0], deltas.shape[1]


def _morph_weights(weights):
    """The weights of pose_mesh as a contiguous float32 array, one per target -> (array, n_targets); ValueError for another dtype
    (no silent narrowing of float64) or shape."""
    if not isinstance(weights, np.ndarray) or weights.dtype != np.dtype(np.float32):
        raise ValueError("pose_mesh: the weights must be a numpy float32 array")
    if weights.ndim != 1 or len(weights) == 0:
        raise ValueError("pose_mesh: the weights must be one per target, in one dimension (shape %s given)" % (weights.shape,))
    return np.ascontiguousarray(weights), len(weights)


def _pose_args(weights, joint_matrices):
    """(weights pointer, n_targets, matrices pointer, n_joints, the arrays kept alive) of a pose_mesh call; either may be None."""
    if weights is None and joint_matrices is None:
        raise ValueError("pose_mesh: neither weights nor joint matrices given")
    w, nt = _morph_weights(weights) if weights is not None else (None, 0)
    m, nj = _joint_matrices(joint_matrices) if joint_matrices is not None else (None, 0)
    return (None if w is None else _p(w)), C.c_uint32(nt), (None if m is None else _p(m)), C.c_uint32(nj), (w, m)


def _pose_items(items):
    """The items of pose_meshes, a sequence of (key, weights or None, joint matrices or None), as an abi.SrPoseItem array ->
    (array, n_items, the arrays kept alive); each item goes through _pose_args, whose ValueErrors name the item."""
    try:
        items = [tuple(it) for it in items]
    except TypeError:
        raise ValueError("pose_meshes: the items must be a sequence of (key, weights, joint_matrices)")
    rows, keep = (abi.SrPoseItem * max(len(items), 1))(), []
    for i, it in enumerate(items):
        if len(it) != 3:
            raise ValueError("pose_meshes: item %d: an item is (key, weights, joint_matrices), %d values given" % (i, len(it)))
        try:
            wp, nt, mp, nj, arrays = _pose_args(it[1], it[2])
        except ValueError as e:
            raise ValueError("pose_meshes: item %d: %s" % (i, e))
        rows[i].key = int(it[0])
        rows[i].weights = None if wp is None else wp.value
        rows[i].joint_matrices = None if mp is None else mp.value
        rows[i].n_targets, rows[i].n_joints = nt.value, nj.value
        keep.append(arrays)
    return rows, C.c_uint32(len(items)), keep


class ClipWeights:
    """The fourth element of a pose_actors item whose morph weights come from its actor's clip, evaluated on the GPU: morph set
    `blas` of that clip at the actor's time (SR_ACTOR_CLIP_WEIGHTS)."""

    def __init__(self, blas):
        self.blas = int(blas)
        if self.blas < 0:
            raise ValueError("ClipWeights: the blas is an index")


class ActorArgs:
    """The arguments of pose_actors packed once (abi.SrClipActor / abi.SrActorPoseItem arrays and the numpy arrays they point
    into): `actors` is a sequence of (clip id, time in seconds, placement [12] float32 or None, instance rows uint32 or None,
    instance base), `items` one of (key, actor index, skin index or None, weights or ClipWeights(blas) or None; the actor index
    may be None where neither a skin nor ClipWeights names it). set_times() rewrites the times in place, so a crowd's per-frame
    work on the host is that and the call."""

    WHO, ROW = "pose_actors", abi.SrClipActor

    def __init__(self, actors, items):
        actors, items = [tuple(a) for a in actors], [tuple(i) for i in items]
        self.actors, self.items, self.keep = (self.ROW * max(len(actors), 1))(), (abi.SrActorPoseItem * max(len(items), 1))(), []
        self.n_actors, self.n_items = len(actors), len(items)
        for a, ac in enumerate(actors):
            self._actor(a, ac, self.actors[a])
        self._items(items)

    def _actor(self, a, ac, row):
        if len(ac) != 5:
            raise ValueError("pose_actors: actor %d: an actor is (clip id, time, placement, instance rows, instance base), %d values given" % (a, len(ac)))
        row.clip_id, row.time_seconds, row.instance_base = int(ac[0]), float(ac[1]), int(ac[4])
        self._placed(a, row, ac[2], ac[3])

    def _placed(self, a, row, placement, rows):
        if placement is not None:
            m = np.ascontiguousarray(placement)
            if m.dtype not in (np.dtype(np.float32), abi.TRANSFORM) or m.nbytes != 48:
                raise ValueError("%s: actor %d: the placement must be 12 float32 (row-major 3x4)" % (self.WHO, a))
            self.keep.append(m)
            row.placement = m.ctypes.data
        if rows is not None:
            r = np.ascontiguousarray(rows)
            if r.dtype != np.dtype(np.uint32) or r.ndim != 1:
                raise ValueError("%s: actor %d: the instance rows must be a one-dimensional numpy uint32 array" % (self.WHO, a))
            self.keep.append(r)
            row.instance_rows = r.ctypes.data if len(r) else None

    def _items(self, items):
        for i, it in enumerate(items):
            if len(it) != 4:
                raise ValueError("%s: item %d: an item is (key, actor, skin, weights), %d values given" % (self.WHO, i, len(it)))
            row = self.items[i]
            row.key, row.actor, row.skin = int(it[0]), 0 if it[1] is None else int(it[1]), abi.ACTOR_NO_SKIN if it[2] is None else int(it[2])
            if isinstance(it[3], ClipWeights):
                row.morph = abi.actor_clip_weights(it[3].blas)
            elif it[3] is not None:
                try:
                    w, nt = _morph_weights(it[3])
                except ValueError as e:
                    raise ValueError("%s: item %d: %s" % (self.WHO, i, e))
                self.keep.append(w)
                row.weights, row.n_targets = w.ctypes.data, nt

    def set_times(self, times):
        for a, t in enumerate(times):
            self.actors[a].time_seconds = float(t)


class BlendedActorArgs(ActorArgs):
    """The arguments of pose_actors_blended packed once: ActorArgs with `actors` a sequence of (clip id a, time a, clip id b,
    time b, weight: the share of b in [0, 1], placement, instance rows, instance base). set_times() rewrites A's times,
    set_fades() B's times and the weights."""
    WHO, ROW = "pose_actors_blended", abi.SrClipBlendActor

    def _actor(self, a, ac, row):
        if len(ac) != 8:
            raise ValueError("pose_actors_blended: actor %d: an actor is (clip id a, time a, clip id b, time b, weight, placement, instance rows, instance base), "
                             "%d values given" % (a, len(ac)))
        row.clip_id, row.time_seconds, row.clip_id_b, row.time_seconds_b, row.weight, row.instance_base = int(ac[0]), float(ac[1]), int(ac[2]), float(ac[3]), float(ac[4]), int(ac[7])
        self._placed(a, row, ac[5], ac[6])

    def set_fades(self, times_b, weights):
        for a, (t, w) in enumerate(zip(times_b, weights)):
            self.actors[a].time_seconds_b, self.actors[a].weight = float(t), float(w)


class LayeredActorArgs(ActorArgs):
    """The arguments of pose_actors_layered packed once: ActorArgs with `actors` a sequence of (layers, placement, instance rows,
    instance base), `layers` a sequence of 1..abi.CLIP_MAX_LAYERS of (clip id, time, weight in [0, 1], mode: "override" /
    "additive" or abi.LAYER_*, mask id or None, reference time of an additive layer); the first is the base. The layers of all
    actors lie in one array; set_times() rewrites every layer's time in place (one sequence per actor, one time per layer),
    set_layer() one layer's time, weight and reference time."""
    WHO, ROW = "pose_actors_layered", abi.SrClipLayerActor
    MODES = {"override": abi.LAYER_OVERRIDE, "additive": abi.LAYER_ADDITIVE}

    def __init__(self, actors, items):
        actors = [tuple(a) for a in actors]
        for a, ac in enumerate(actors):
            if len(ac) != 4:
                raise ValueError("pose_actors_layered: actor %d: an actor is (layers, placement, instance rows, instance base), %d values given" % (a, len(ac)))
        stacks = [[tuple(ly) for ly in ac[0]] for ac in actors]
        self.layers = (abi.SrClipLayer * max(sum(len(st) for st in stacks), 1))()
        self.first_layer, at = [], 0
        for a, st in enumerate(stacks):
            self.first_layer.append(at)
            for l, ly in enumerate(st):
                if len(ly) != 6:
                    raise ValueError("pose_actors_layered: actor %d: layer %d: a layer is (clip id, time, weight, mode, mask id, reference time), %d values given"
                                     % (a, l, len(ly)))
                row = self.layers[at + l]
                row.clip_id, row.time_seconds, row.weight = int(ly[0]), float(ly[1]), float(ly[2])
                row.mode = self.MODES[ly[3]] if isinstance(ly[3], str) else int(ly[3])
                row.mask_id, row.ref_time_seconds = abi.LAYER_NO_MASK if ly[4] is None else int(ly[4]), float(ly[5])
            at += len(st)
        self.n_layers = [len(st) for st in stacks]
        super().__init__(actors, items)

    def _actor(self, a, ac, row):
        row.layers = C.addressof(self.layers) + C.sizeof(abi.SrClipLayer) * self.first_layer[a]
        row.n_layers, row.instance_base = self.n_layers[a], int(ac[3])
        self._placed(a, row, ac[1], ac[2])

    def set_times(self, times):
        for a, per_layer in enumerate(times):
            for l, t in enumerate(per_layer):
                self.layers[self.first_layer[a] + l].time_seconds = float(t)

    def set_layer(self, actor, layer, time_seconds=None, weight=None, ref_time_seconds=None):
        row = self.layers[self.first_layer[actor] + layer]
        if time_seconds is not None:
            row.time_seconds = float(time_seconds)
        if weight is not None:
            row.weight = float(weight)
        if ref_time_seconds is not None:
            row.ref_time_seconds = float(ref_time_seconds)


def _actor_call(fn, handle, actors, items, tensor, keep_nodes, device_index, keep_sources=False, packed=ActorArgs, keep_layers=False, layer_weights=False):
    if isinstance(actors, ActorArgs) and type(actors) is not packed:
        raise ValueError("%s: the packed arguments are those of another entry point (%s)" % (packed.WHO, type(actors).__name__))
    args = actors if isinstance(actors, packed) else packed(actors, items)
    ptr, stream = None, None
    if tensor is not None:
        import torch
        if not getattr(tensor, "is_cuda", False) or tensor.device.index != device_index:
            raise ValueError("%s: the instance transforms must be a tensor on cuda:%d" % (packed.WHO, device_index))
        if str(tensor.dtype) != "torch.float32" or not tensor.is_contiguous() or tensor.numel() % 12:
            raise ValueError("%s: the instance transforms must be contiguous float32, 12 a transform" % packed.WHO)
        ptr, stream = C.c_void_p(tensor.data_ptr()), C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)
    check(fn(handle, args.actors, C.c_uint32(args.n_actors), args.items, C.c_uint32(args.n_items), ptr,
             C.c_uint32((abi.ACTORS_KEEP_NODES if keep_nodes else 0) | (abi.ACTORS_KEEP_SOURCES if keep_sources else 0) |
                        (abi.ACTORS_KEEP_LAYERS if keep_layers else 0) | (abi.ACTORS_LAYER_WEIGHTS if layer_weights else 0)), stream))


class Clip:
    """A baked clip (sr_gltf_bake_clip): one animation of a file, or its static pose, as flat tables. Immutable; it does not
    refer to the Gltf afterwards."""

    def __init__(self, handle):
        self._h = handle
        self.info = self._info()

    def close(self):
        if getattr(self, "_h", None):
            lib().sr_clip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self):
        info = abi.SrClipInfo()
        check(lib().sr_clip_info(self._h, C.byref(info)))
        return info

    def skin(self, skin):
        """-> (first matrix in the clip's concatenated joint list, joint count) of the file's skin `skin` (sr_clip_skin)."""
        first, n = C.c_uint32(), C.c_uint32()
        check(lib().sr_clip_skin(self._h, C.c_uint32(skin), C.byref(first), C.byref(n)))
        return first.value, n.value

    def layout(self):
        """-> (abi.CLIP_NODE_INFO [n_nodes], abi.CLIP_CHANNEL_INFO [n_channels], clip node of every instance uint32) (sr_clip_layout)."""
        i = self.info
        nodes, chans = np.zeros(max(i.n_nodes, 1), abi.CLIP_NODE_INFO), np.zeros(max(i.n_channels, 1), abi.CLIP_CHANNEL_INFO)
        inst = np.zeros(max(i.n_instances, 1), np.uint32)
        check(lib().sr_clip_layout(self._h, _p(nodes), _p(chans), _p(inst)))
        return nodes[:i.n_nodes], chans[:i.n_channels], inst[:i.n_instances]

    def channel_keys(self, channel):
        """-> (key times [n_keys], values [n_keys, 3 or 4]) of a channel, the file's float32; a CUBICSPLINE channel's values
        are [3 * n_keys, 3 or 4]: per key its in-tangent, value and out-tangent (sr_clip_channel_keys)."""
        c = self.layout()[1][channel]
        tp, vp = C.c_void_p(), C.c_void_p()
        check(lib().sr_clip_channel_keys(self._h, C.c_uint32(channel), C.byref(tp), C.byref(vp)))
        comps = 4 if c["path"] == 1 else 3
        rows = int(c["n_keys"]) * (3 if c["interpolation"] == abi.CLIP_CUBICSPLINE else 1)
        return _np_from(tp, int(c["n_keys"]), np.float32), _np_from(vp, rows * comps, np.float32).reshape(-1, comps)

    def morph_count(self):
        """-> the number of morph sets: one for every blas of the file that has morph targets (sr_clip_morph_count)."""
        n = C.c_uint32()
        check(lib().sr_clip_morph_count(self._h, C.byref(n)))
        return n.value

    def morph(self, blas):
        """-> dict(blas, gltf_node, n_targets, n_keys, interpolation, state (abi.CLIP_MORPH_*), status, error) of the blas's morph
        set; error: the loader's words where the set is unavailable, else None (sr_clip_morph)."""
        info = abi.SrClipMorphInfo()
        check(lib().sr_clip_morph(self._h, C.c_uint32(blas), C.byref(info)))
        out = {name: getattr(info, name) for name, _ in abi.SrClipMorphInfo._fields_ if name != "reserved"}
        out["error"] = lib().sr_last_error().decode("utf-8", "replace") if info.state == abi.CLIP_MORPH_UNAVAILABLE else None
        return out

    def morph_keys(self, blas):
        """-> (key times [n_keys], values [n_keys, n_targets], default weights [n_targets]) of the blas's morph set, the file's
        float32; without a channel the first two are empty; a CUBICSPLINE set's values are [3 * n_keys, n_targets]: per key its
        in-tangents, values and out-tangents (sr_clip_morph_keys)."""
        m = self.morph(blas)
        tp, vp, dp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sr_clip_morph_keys(self._h, C.c_uint32(blas), C.byref(tp), C.byref(vp), C.byref(dp)))
        nk, nt = m["n_keys"], m["n_targets"]
        rows = nk * (3 if m["interpolation"] == abi.CLIP_CUBICSPLINE else 1)
        return _np_from(tp, nk, np.float32), _np_from(vp, rows * nt, np.float32).reshape(rows, nt), _np_from(dp, nt, np.float32)

    def weights_host(self, time_seconds, blas, n_targets=None):
        """-> the weights [n_targets] float32 of the blas's morph set at `time_seconds`: sr_gltf_morph_weights restated over the
        clip, bit for bit. n_targets: the set's own unless given (sr_clip_weights_host)."""
        nt = self.morph(blas)["n_targets"] if n_targets is None else int(n_targets)
        w = np.zeros(max(nt, 1), dtype=np.float32)
        check(lib().sr_clip_weights_host(self._h, C.c_float(time_seconds), C.c_uint32(blas), _p(w), C.c_uint32(nt)))
        return w[:nt]

    def sample_host(self, time_seconds):
        """-> abi.NODE_TRS [n_nodes]: every clip node's TRS at `time_seconds` (sr_clip_sample_host)."""
        trs = np.zeros(max(self.info.n_nodes, 1), abi.NODE_TRS)
        check(lib().sr_clip_sample_host(self._h, C.c_float(time_seconds), _p(trs)))
        return trs[:self.info.n_nodes]

    def compose_host(self, trs, placement=None, fn=None):
        """abi.NODE_TRS records -> (joint matrices of all skins [n_joints, 12], instance transforms [n_instances, 12], the lowest
        singular skin or None). A singular skin is reported, not raised (sr_clip_compose_host)."""
        i = self.info
        trs = np.ascontiguousarray(trs, dtype=abi.NODE_TRS)
        if len(trs) != i.n_nodes:
            raise ValueError("compose_host: %d records given, the clip has %d nodes" % (len(trs), i.n_nodes))
        joints, xf, bad = np.zeros((max(i.n_joints, 1), 12), np.float32), np.zeros((max(i.n_instances, 1), 12), np.float32), C.c_uint32()
        pl = None if placement is None else np.ascontiguousarray(placement, dtype=np.float32).reshape(12)
        rc = (fn or lib().sr_clip_compose_host)(self._h, _p(trs), None if pl is None else _p(pl), _p(joints), _p(xf), C.byref(bad))
        if rc != 0 and bad.value == 0xFFFFFFFF:
            check(rc)
        return joints[:i.n_joints], xf[:i.n_instances], (None if bad.value == 0xFFFFFFFF else bad.value)

    def blend_compatible(self, other):
        """Raises unless this clip and `other` may be cross-faded: equal tables but the channels and the animated masks, in
        practice bakes of one file (sr_clip_blend_compatible)."""
        check(lib().sr_clip_blend_compatible(self._h, other._h))
        return True

    def compose_records_host(self, trs, placement=None):
        """compose_host with each node's TRS-or-matrix decision taken from the record's own `animated` word, as blended records
        need it (sr_clip_compose_records_host)."""
        return self.compose_host(trs, placement, fn=lib().sr_clip_compose_records_host)

    def pose_blend_host(self, time_seconds, other, time_other, weight, placement=None, joints=True):
        """-> (joint matrices or None, instance transforms) of the cross-fade from this clip at `time_seconds` to `other` at
        `time_other`, at the share `weight` of `other`: sample, sample, blend, compose (sr_clip_pose_blend_host)."""
        i = self.info
        jm = np.zeros((max(i.n_joints, 1), 12), np.float32) if joints else None
        xf = np.zeros((max(i.n_instances, 1), 12), np.float32)
        pl = None if placement is None else np.ascontiguousarray(placement, dtype=np.float32).reshape(12)
        check(lib().sr_clip_pose_blend_host(self._h, C.c_float(time_seconds), other._h, C.c_float(time_other), C.c_float(weight), None if pl is None else _p(pl),
                                            None if jm is None else _p(jm), _p(xf)))
        return (None if jm is None else jm[:i.n_joints]), xf[:i.n_instances]

    def blend_weights_host(self, time_seconds, other, time_other, weight, blas, n_targets=None):
        """-> the blended weights [n_targets] float32 of the blas's morph set, which both clips must have
        (sr_clip_blend_weights_host)."""
        nt = self.morph(blas)["n_targets"] if n_targets is None else int(n_targets)
        w = np.zeros(max(nt, 1), dtype=np.float32)
        check(lib().sr_clip_blend_weights_host(self._h, C.c_float(time_seconds), other._h, C.c_float(time_other), C.c_float(weight), C.c_uint32(blas), _p(w), C.c_uint32(nt)))
        return w[:nt]

    def subtree_mask(self, gltf_node, inside=1.0, outside=0.0):
        """-> a node mask float32 [n_nodes]: `inside` for the clip node of glTF node `gltf_node` and everything below it in the
        clip's parent table, `outside` elsewhere (sr_clip_subtree_mask)."""
        out = np.zeros(max(self.info.n_nodes, 1), np.float32)
        check(lib().sr_clip_subtree_mask(self._h, C.c_uint32(gltf_node), C.c_float(inside), C.c_float(outside), _p(out), C.c_uint32(self.info.n_nodes)))
        return out[:self.info.n_nodes]

    def pose_layers_host(self, layers, placement=None, joints=True):
        """-> (joint matrices or None, instance transforms) of a stack of layers whose base is this clip: `layers` is a sequence
        of (clip, time, weight, mode: "override" / "additive" or abi.LAYER_*, host mask float32 [n_nodes] or None, reference
        time); the first is the base and names this clip: sample, stack, compose (sr_clip_pose_layers_host)."""
        layers = [tuple(ly) for ly in layers]
        n = len(layers)
        clips, rows, masks, keep = (C.c_void_p * max(n, 1))(), (abi.SrClipLayer * max(n, 1))(), (C.c_void_p * max(n, 1))(), []
        for l, ly in enumerate(layers):
            if len(ly) != 6:
                raise ValueError("pose_layers_host: layer %d: a layer is (clip, time, weight, mode, mask, reference time), %d values given" % (l, len(ly)))
            clips[l] = ly[0]._h if isinstance(ly[0], Clip) else ly[0]
            rows[l].time_seconds, rows[l].weight, rows[l].ref_time_seconds, rows[l].mask_id = float(ly[1]), float(ly[2]), float(ly[5]), abi.LAYER_NO_MASK
            rows[l].mode = LayeredActorArgs.MODES[ly[3]] if isinstance(ly[3], str) else int(ly[3])
            if ly[4] is not None:
                m = _node_mask(ly[4], "pose_layers_host: layer %d" % l)
                keep.append(m)
                masks[l] = m.ctypes.data
        i = self.info
        jm = np.zeros((max(i.n_joints, 1), 12), np.float32) if joints else None
        xf = np.zeros((max(i.n_instances, 1), 12), np.float32)
        pl = None if placement is None else np.ascontiguousarray(placement, dtype=np.float32).reshape(12)
        check(lib().sr_clip_pose_layers_host(clips, rows, masks, C.c_uint32(n), None if pl is None else _p(pl), None if jm is None else _p(jm), _p(xf)))
        return (None if jm is None else jm[:i.n_joints]), xf[:i.n_instances]

    def pose_host(self, time_seconds, placement=None, joints=True):
        """-> (joint matrices of all skins [n_joints, 12] or None, instance transforms [n_instances, 12]) at `time_seconds`:
        sr_gltf_pose restated over the clip, bit for bit (sr_clip_pose_host)."""
        i = self.info
        jm = np.zeros((max(i.n_joints, 1), 12), np.float32) if joints else None
        xf = np.zeros((max(i.n_instances, 1), 12), np.float32)
        pl = None if placement is None else np.ascontiguousarray(placement, dtype=np.float32).reshape(12)
        check(lib().sr_clip_pose_host(self._h, C.c_float(time_seconds), None if pl is None else _p(pl), None if jm is None else _p(jm), _p(xf)))
        return (None if jm is None else jm[:i.n_joints]), xf[:i.n_instances]


def clip_blend_host(trs_a, trs_b, weight):
    """abi.NODE_TRS records of two sources -> the blended records at the share `weight` of the second (sr_clip_blend_host)."""
    a, b = np.ascontiguousarray(trs_a, dtype=abi.NODE_TRS), np.ascontiguousarray(trs_b, dtype=abi.NODE_TRS)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("clip_blend_host: the two sources must hold the same number of records")
    out = np.zeros(max(len(a), 1), abi.NODE_TRS)
    check(lib().sr_clip_blend_host(_p(a) if len(a) else None, _p(b) if len(b) else None, C.c_uint32(len(a)), C.c_float(weight), _p(out)))
    return out[:len(a)]


def _node_mask(mask, who):
    """A node mask as a contiguous one-dimensional float32 array; ValueError for another dtype (no silent narrowing) or shape."""
    if not isinstance(mask, np.ndarray) or mask.dtype != np.dtype(np.float32) or mask.ndim != 1 or len(mask) == 0:
        raise ValueError("%s: a node mask must be a one-dimensional numpy float32 array, one value per clip node" % who)
    return np.ascontiguousarray(mask)


def clip_layers_host(cur, rules, ref=None):
    """The layer rule over sampled records: `cur` a sequence of abi.NODE_TRS arrays, one per layer (the first is the base), `rules`
    one (weight, mode: "override" / "additive" or abi.LAYER_*, host mask float32 [n_nodes] or None) per layer, `ref` a sequence
    with an additive layer's records at its reference time (None elsewhere), or None -> the final records
    (sr_clip_layers_host)."""
    cur = [np.ascontiguousarray(c, dtype=abi.NODE_TRS) for c in cur]
    rules = [tuple(r) for r in rules]
    n = len(cur)
    if len(rules) != n or (ref is not None and len(ref) != n):
        raise ValueError("clip_layers_host: one rule (and, where given, one reference entry) per layer")
    n_nodes = len(cur[0]) if n else 0
    if any(c.ndim != 1 or len(c) != n_nodes for c in cur):
        raise ValueError("clip_layers_host: every layer must hold the same number of records")
    refs = [None if ref is None or r is None else np.ascontiguousarray(r, dtype=abi.NODE_TRS) for r in (ref or [None] * n)]
    if any(r is not None and (r.ndim != 1 or len(r) != n_nodes) for r in refs):
        raise ValueError("clip_layers_host: every layer must hold the same number of records")
    cp, rp, rows, keep = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))(), (abi.SrClipLayerRule * max(n, 1))(), []
    for l in range(n):
        if len(rules[l]) != 3:
            raise ValueError("clip_layers_host: layer %d: a rule is (weight, mode, mask), %d values given" % (l, len(rules[l])))
        cp[l] = cur[l].ctypes.data if n_nodes else None
        rp[l] = refs[l].ctypes.data if refs[l] is not None and n_nodes else None
        rows[l].weight = float(rules[l][0])
        rows[l].mode = LayeredActorArgs.MODES[rules[l][1]] if isinstance(rules[l][1], str) else int(rules[l][1])
        if rules[l][2] is not None:
            m = _node_mask(rules[l][2], "clip_layers_host: layer %d" % l)
            if len(m) != n_nodes:
                raise ValueError("clip_layers_host: layer %d: the mask has %d values, the layers %d records" % (l, len(m), n_nodes))
            keep.append(m)
            rows[l].mask = m.ctypes.data
    out = np.zeros(max(n_nodes, 1), abi.NODE_TRS)
    check(lib().sr_clip_layers_host(cp, rp, rows, C.c_uint32(n), C.c_uint32(n_nodes), _p(out)))
    return out[:n_nodes]


def clip_layer_weights_host(cur, rules, ref=None):
    """The layer rule over sampled morph weights: `cur` a sequence of float32 arrays [n_targets], one per layer (the first is the
    base), `rules` one (weight, mode: "override" / "additive" or abi.LAYER_*, mask value in [0, 1] or None: 1) per layer, `ref`
    a sequence with an additive layer's weights at its reference time (None elsewhere), or None -> the stacked weights, zeros
    included (sr_clip_layer_weights_host)."""
    cur = [np.ascontiguousarray(c, dtype=np.float32) for c in cur]
    rules = [tuple(r) for r in rules]
    n = len(cur)
    if len(rules) != n or (ref is not None and len(ref) != n):
        raise ValueError("clip_layer_weights_host: one rule (and, where given, one reference entry) per layer")
    n_targets = len(cur[0]) if n else 0
    refs = [None if ref is None or r is None else np.ascontiguousarray(r, dtype=np.float32) for r in (ref or [None] * n)]
    if any(c.ndim != 1 or len(c) != n_targets for c in cur) or any(r is not None and (r.ndim != 1 or len(r) != n_targets) for r in refs):
        raise ValueError("clip_layer_weights_host: every layer must hold the same number of weights")
    if any(len(r) != 3 for r in rules):
        raise ValueError("clip_layer_weights_host: a rule is (weight, mode, mask value)")
    cp, rp = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    for l in range(n):
        cp[l] = cur[l].ctypes.data if n_targets else None
        rp[l] = refs[l].ctypes.data if refs[l] is not None and n_targets else None
    weight, mode, mask_value = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint32), np.ones(max(n, 1), np.float32)
    for l, r in enumerate(rules):
        weight[l], mode[l] = r[0], LayeredActorArgs.MODES[r[1]] if isinstance(r[1], str) else int(r[1])
        mask_value[l] = 1.0 if r[2] is None else r[2]
    masked = any(r[2] is not None for r in rules)
    out = np.zeros(max(n_targets, 1), np.float32)
    check(lib().sr_clip_layer_weights_host(cp, rp, _p(weight), _p(mode), _p(mask_value) if masked else None,
                                           C.c_uint32(n), C.c_uint32(n_targets), _p(out)))
    return out[:n_targets]


def clip_weights_layers_host(layers, blas, n_targets=None):
    """-> the weights [n_targets] float32, zeros included, of the blas's morph set through a stack of layers: `layers` as
    Clip.pose_layers_host takes them, (clip, time, weight, mode, host mask float32 [n_nodes] or None, reference time), the first
    the base: sample every layer's set, resolve each mask at the set's node, stack (sr_clip_weights_layers_host)."""
    layers = [tuple(ly) for ly in layers]
    n = len(layers)
    clips, rows, masks, keep = (C.c_void_p * max(n, 1))(), (abi.SrClipLayer * max(n, 1))(), (C.c_void_p * max(n, 1))(), []
    for l, ly in enumerate(layers):
        if len(ly) != 6:
            raise ValueError("clip_weights_layers_host: layer %d: a layer is (clip, time, weight, mode, mask, reference time), %d values given" % (l, len(ly)))
        clips[l] = ly[0]._h if isinstance(ly[0], Clip) else ly[0]
        rows[l].time_seconds, rows[l].weight, rows[l].ref_time_seconds, rows[l].mask_id = float(ly[1]), float(ly[2]), float(ly[5]), abi.LAYER_NO_MASK
        rows[l].mode = LayeredActorArgs.MODES[ly[3]] if isinstance(ly[3], str) else int(ly[3])
        if ly[4] is not None:
            m = _node_mask(ly[4], "clip_weights_layers_host: layer %d" % l)
            keep.append(m)
            masks[l] = m.ctypes.data
    nt = layers[0][0].morph(blas)["n_targets"] if n_targets is None else int(n_targets)
    w = np.zeros(max(nt, 1), dtype=np.float32)
    check(lib().sr_clip_weights_layers_host(clips, rows, masks, C.c_uint32(n), C.c_uint32(blas), _p(w), C.c_uint32(nt)))
    return w[:nt]


def pose_batch_plan(n_vertices):
    """The layout of a batch of meshes of these vertex counts -> (first_block uint32[n], vertex_base uint64[n], n_blocks): host
    only (sr_pose_batch_plan)."""
    counts = np.ascontiguousarray(n_vertices, dtype=np.uint32)
    first, base, blocks = np.zeros(len(counts), np.uint32), np.zeros(len(counts), np.uint64), C.c_uint32(0)
    check(lib().sr_pose_batch_plan(_p(counts), C.c_uint32(len(counts)), _p(first), _p(base), C.byref(blocks)))
    return first, base, blocks.value


def camera_matrices(pos, target, fov_y, width, height, prev_view_proj=None):
    """Camera::as_matrices + transposed upload (camera.rs:33-63, lib.rs:1017-1048). Host only."""
    m = abi.SrMatrices()
    prev = None
    if prev_view_proj is not None:
        prev = (C.c_float * 16)(*[float(x) for x in prev_view_proj])
    check(lib().sr_camera_matrices(_f3(pos), _f3(target), C.c_float(fov_y), C.c_uint32(width), C.c_uint32(height), prev, C.byref(m)))
    return m


def material_new(base_color, metallic, roughness, emissive_factor, emissive_strength, transmission, ior):
    m = np.zeros((), dtype=abi.MATERIAL)
    check(lib().sr_material_new((C.c_float * 4)(*base_color), C.c_float(metallic), C.c_float(roughness), _f3(emissive_factor),
                                C.c_float(emissive_strength), C.c_float(transmission), C.c_float(ior), _p(m)))
    return m


def decode_image(data):
    """The glTF loader's image decoder on its own (8-bit PNG, JPEG) -> (h, w, channels) uint8."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    w, h, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().sr_decode_image(buf, C.c_size_t(len(data)), C.byref(w), C.byref(h), C.byref(c), None, C.c_size_t(0)))
    out = np.zeros((h.value, w.value, c.value), dtype=np.uint8)
    check(lib().sr_decode_image(buf, C.c_size_t(len(data)), C.byref(w), C.byref(h), C.byref(c), _p(out), C.c_size_t(out.size)))
    return out


def decode_image_rgba8(data):
    """image::load_from_memory(..).to_rgba8() (lib.rs:281-283): PNG (8- and 16-bit) / JPEG -> (h, w, 4) uint8."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    w, h = C.c_uint32(), C.c_uint32()
    check(lib().sr_decode_image_rgba8(buf, C.c_size_t(len(data)), C.byref(w), C.byref(h), None, C.c_size_t(0)))
    out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    check(lib().sr_decode_image_rgba8(buf, C.c_size_t(len(data)), C.byref(w), C.byref(h), _p(out), C.c_size_t(out.size)))
    return out


def emissive_triangles_from_mesh(vertices, indices, material):
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
    i = np.ascontiguousarray(indices, dtype=np.uint32)
    m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
    out = np.zeros(max(len(i) // 3, 1), dtype=abi.EMISSIVE_TRIANGLE)
    n = C.c_uint32()
    check(lib().sr_emissive_triangles_from_mesh(_p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m), _p(out), C.c_uint32(len(out)), C.byref(n)))
    return out[: n.value].copy()


def light_table(transforms, entries, triangles):
    """The host arithmetic of the frame's light table (sr_light_table): transforms (n, 12) float32, entries abi.EMISSIVE_INDIRECTION,
    triangles abi.EMISSIVE_TRIANGLE -> (len(entries), 16) float32 in the order Scene.read_lights documents."""
    t = np.asarray(transforms)
    t = np.ascontiguousarray(t["m"] if t.dtype.names else t, dtype=np.float32).reshape(-1, 12)
    e = np.ascontiguousarray(entries, dtype=abi.EMISSIVE_INDIRECTION)
    tr = np.ascontiguousarray(triangles, dtype=abi.EMISSIVE_TRIANGLE)
    out = np.zeros((len(e), 16), dtype=np.float32)
    check(lib().sr_light_table(_p(t), C.c_uint32(len(t)), _p(e), C.c_uint32(len(e)), _p(tr), C.c_uint32(len(tr)), _p(out)))
    return out


def bvh_layout():
    """(children per node, dwords per node, first plane dword, first child dword) of this build's BVH (csrc/bvh_layout.h)."""
    w, nd, po, co = (C.c_uint32() for _ in range(4))
    check(lib().sr_bvh_layout(C.byref(w), C.byref(nd), C.byref(po), C.byref(co)))
    return w.value, nd.value, po.value, co.value


def tree_build_limits(kind, n_prims):
    """(primitives per leaf, stack floor of the collapse before the build's cap bounds it) of a device-built tree of `n_prims`
    primitives of one abi.TREE_KIND_* (sr_tree_build_limits)."""
    leaf_max, floor = C.c_uint32(), C.c_uint32()
    check(lib().sr_tree_build_limits(C.c_uint32(kind), C.c_uint64(n_prims), C.byref(leaf_max), C.byref(floor)))
    return leaf_max.value, floor.value


def host_bvh(v0_e1_e2):
    """Host-only BVH build (no GPU): returns (nodes[n, node_dwords] u32, tris[n,12] f32, max_depth, max_stack)."""
    v = np.ascontiguousarray(v0_e1_e2, dtype=np.float32).reshape(-1, 9)
    h = C.c_void_p()
    check(lib().sr_host_bvh_build(_p(v), C.c_uint32(len(v)), C.byref(h)))
    try:
        np_, tp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
        nn, nt, md, ms = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().sr_host_bvh_get(h, C.byref(np_), C.byref(nn), C.byref(tp), C.byref(nt), C.byref(md), C.byref(ms)))
        nodes = np.ctypeslib.as_array(np_, shape=(nn.value, bvh_layout()[1])).copy()
        tris = np.ctypeslib.as_array(tp, shape=(nt.value, 12)).copy() if nt.value else np.zeros((0, 12), np.float32)
    finally:
        lib().sr_host_bvh_destroy(h)
    return nodes, tris, md.value, ms.value


def decode_node(node):
    """Child boxes of one quantised node as the kernel decodes them: plane = fmaf(q, 2^e, origin).
    Returns (lo[W,3], hi[W,3], child[W]) in float32 / int32."""
    W, _, po, co = bvh_layout()
    n = np.asarray(node, dtype=np.uint32)
    origin = n[0:3].view(np.float32)
    scale = n[[3, 10, 11]].view(np.float32)      # the grid scales 2^e per axis, stored as fp32 (csrc/bvh_layout.h)
    pd = W // 4                      # dwords per plane; planes LX LY LZ HX HY HZ
    lo = np.zeros((W, 3), np.float32)
    hi = np.zeros((W, 3), np.float32)
    for c in range(W):
        for a in range(3):
            ql = np.float32((int(n[po + a * pd + c // 4]) >> (8 * (c % 4))) & 0xFF)
            qh = np.float32((int(n[po + (3 + a) * pd + c // 4]) >> (8 * (c % 4))) & 0xFF)
            # one rounding, like v_fma_f32: the product q * 2^e is exact in float64
            lo[c, a] = np.float32(np.float64(ql) * np.float64(scale[a]) + np.float64(origin[a]))
            hi[c, a] = np.float32(np.float64(qh) * np.float64(scale[a]) + np.float64(origin[a]))
    return lo, hi, n[co:co + W].view(np.int32)


class DeviceFrame:
    """Frame buffers in HBM with the layouts of SrRtParams (torch tensors on one device)."""

    def __init__(self, width, height, blue_noise, device="cuda:0", primary=None):
        """`primary`: allocate the primary-hit hand-off buffer (SrRtParams.primary_payload). Default: yes, unless
        SUNRAY_PRIMARY_REUSE=0 is set in the environment (A/B switch of tests and scripts)."""
        import os
        import torch
        self.width, self.height = width, height
        n = width * height
        self.device = torch.device(device)
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=self.device)
        self.raw_color = z(n, 4, dtype=torch.float32)
        self.depth = z(n, dtype=torch.int16)       # R16_SFLOAT bits
        self.normal = z(n, dtype=torch.int32)      # R8G8B8A8_SNORM
        self.diffuse = z(n, dtype=torch.int32)     # B10G11R11_UFLOAT
        self.motion = z(n, dtype=torch.int32)      # R16G16_SFLOAT
        self.reservoirs = [z(n, 12, dtype=torch.int32), z(n, 12, dtype=torch.int32)]      # 48 B records
        self.reservoirs_gi = [z(n, 12, dtype=torch.int32), z(n, 12, dtype=torch.int32)]
        # post-RT chain images (B10G11R11 ping-pongs, RGBA8 output)
        self.accum = [z(n, dtype=torch.int32), z(n, dtype=torch.int32)]
        self.denoise = [z(n, dtype=torch.int32), z(n, dtype=torch.int32)]
        self.output = z(n, dtype=torch.int32)
        if primary is None:
            primary = os.environ.get("SUNRAY_PRIMARY_REUSE", "1") != "0"
        self.primary = z(n, 8, dtype=torch.int32) if primary else None      # 32-B RayPayload of the camera ray (RIS -> final hand-off)
        bn = np.ascontiguousarray(blue_noise, dtype=np.uint8)
        self.blue_noise_shape = bn.shape[:2]
        self.blue_noise = torch.from_numpy(bn.copy()).to(self.device)

    # host copies in the oracle's dtypes
    def host(self):
        out = {
            "raw_color": self.raw_color.cpu().numpy(),
            "depth": self.depth.cpu().numpy().view(np.uint16),
            "normal": self.normal.cpu().numpy().view(np.uint32),
            "diffuse": self.diffuse.cpu().numpy().view(np.uint32),
            "motion": self.motion.cpu().numpy().view(np.uint32),
            "reservoirs": [r.cpu().numpy().view(np.uint32).reshape(-1).view(abi.RESERVOIR) for r in self.reservoirs],
            "reservoirs_gi": [r.cpu().numpy().view(np.uint32).reshape(-1).view(abi.RESERVOIR_GI) for r in self.reservoirs_gi],
            "accum": [a.cpu().numpy().view(np.uint32) for a in self.accum],
            "denoise": [a.cpu().numpy().view(np.uint32) for a in self.denoise],
            "output": self.output.cpu().numpy().view(np.uint32),
        }
        return out


class Scene:
    """ResourceManager + acceleration structures of one GPU (sr_scene_*)."""

    def __init__(self, device_index=0, instancing=None):
        self._h = C.c_void_p()
        check(lib().sr_scene_create(C.c_int(device_index), C.byref(self._h)))
        self.device_index = device_index
        if instancing is not None:
            self.set_instancing(instancing)

    def close(self):
        if getattr(self, "_h", None):
            lib().sr_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # Renderer::load_mesh (lib.rs:873-954)
    def add_mesh(self, key, vertices, indices, material):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
        slot = C.c_uint32()
        check(lib().sr_scene_add_mesh(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m), C.byref(slot)))
        return slot.value

    def add_blas(self, key, vertices, indices, material, emissive):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
        e = np.ascontiguousarray(emissive, dtype=abi.EMISSIVE_TRIANGLE)
        slot = C.c_uint32()
        check(lib().sr_scene_add_blas(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m),
                                      _p(e) if len(e) else None, C.c_uint32(len(e)), C.byref(slot)))
        return slot.value

    def remove(self, key):
        check(lib().sr_scene_remove(self._h, C.c_uint64(key)))

    # Blas::update (acceleration_structure/blas.rs:285-310)
    def update_mesh(self, key, vertices):
        """New vertex contents for a loaded mesh (same count, indices and material); the next set_instances applies it."""
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        check(lib().sr_scene_update_mesh(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v))))

    def update_mesh_device(self, key, tensor):
        """update_mesh for vertices that are on the GPU already: a contiguous torch tensor on the scene's device, of any dtype,
        whose bytes are the mesh's abi.VERTEX records, produced on torch's current stream (sr_scene_update_mesh_device)."""
        import torch
        ptr, n = _device_vertices(tensor, self.device_index)
        check(lib().sr_scene_update_mesh_device(self._h, C.c_uint64(key), ptr, C.c_uint32(n),
                                                C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)))

    def mesh_vertex_info(self, key):
        """-> abi.SrMeshVertexInfo: whether the library's host copy of the mesh's vertices is behind its device buffer, how
        often it was fetched, and the times of the last update_mesh_device."""
        info = abi.SrMeshVertexInfo()
        check(lib().sr_scene_mesh_vertex_info(self._h, C.c_uint64(key), C.byref(info)))
        return info

    def set_mesh_skin(self, key, influences, n_joints):
        """Attaches a rig to a loaded mesh: `influences` is one abi.SKIN_INFLUENCE record per vertex; the mesh's current vertices
        become the bind pose. influences=None detaches it (sr_scene_set_mesh_skin)."""
        if influences is None:
            check(lib().sr_scene_set_mesh_skin(self._h, C.c_uint64(key), None, C.c_uint32(0), C.c_uint32(0)))
            return
        a = _skin_influences(influences)
        check(lib().sr_scene_set_mesh_skin(self._h, C.c_uint64(key), _p(a), C.c_uint32(len(a)), C.c_uint32(int(n_joints))))

    def skin_mesh(self, key, joint_matrices):
        """Poses a skinned mesh on the GPU from its bind pose: `joint_matrices` is a float32 array of the skin's n_joints 3x4
        matrices. From there on it is an update_mesh_device: the next set_instances applies it (sr_scene_skin_mesh)."""
        m, n = _joint_matrices(joint_matrices)
        check(lib().sr_scene_skin_mesh(self._h, C.c_uint64(key), _p(m), C.c_uint32(n), self._stream()))

    def set_mesh_morph(self, key, deltas):
        """Attaches morph targets to a loaded mesh: `deltas` is a numpy array of abi.MORPH_DELTA records of shape (n_targets,
        n_vertices); the mesh's current vertices become the morph base. deltas=None detaches them (sr_scene_set_mesh_morph)."""
        if deltas is None:
            check(lib().sr_scene_set_mesh_morph(self._h, C.c_uint64(key), None, C.c_uint32(0), C.c_uint32(0)))
            return
        a, nt, nv = _morph_deltas(deltas)
        check(lib().sr_scene_set_mesh_morph(self._h, C.c_uint64(key), _p(a), C.c_uint32(nv), C.c_uint32(nt)))

    def pose_mesh(self, key, weights=None, joint_matrices=None):
        """Poses a mesh on the GPU: its morph targets blended with `weights` (float32, one per target; None: no morph stage), then
        skinned with `joint_matrices` (as skin_mesh; None: no skin stage). From there on it is an update_mesh_device: the next
        set_instances applies it (sr_scene_pose_mesh)."""
        wp, nt, mp, nj, keep = _pose_args(weights, joint_matrices)
        check(lib().sr_scene_pose_mesh(self._h, C.c_uint64(key), wp, nt, mp, nj, self._stream()))

    def pose_meshes(self, items):
        """Poses many meshes at once: `items` is a sequence of (key, weights or None, joint matrices or None), each what pose_mesh
        takes. One upload, one launch and one read-back for the whole batch; all or nothing (sr_scene_pose_meshes)."""
        rows, n, keep = _pose_items(items)
        check(lib().sr_scene_pose_meshes(self._h, rows, n, self._stream()))

    def pose_batch_info(self):
        """-> abi.SrPoseBatchInfo: the last pose_meshes that reached the device (sr_scene_pose_batch_info)."""
        info = abi.SrPoseBatchInfo()
        check(lib().sr_scene_pose_batch_info(self._h, C.byref(info)))
        return info

    def attach_clip(self, clip):
        """Uploads a baked clip's tables once -> its id on this scene (sr_scene_attach_clip)."""
        cid = C.c_uint32()
        check(lib().sr_scene_attach_clip(self._h, clip._h, C.byref(cid)))
        return cid.value

    def detach_clip(self, clip_id):
        check(lib().sr_scene_detach_clip(self._h, C.c_uint32(clip_id)))

    def pose_actors(self, actors, items=(), tensor=None, keep_nodes=False):
        """pose_meshes with the joint matrices evaluated on the GPU from attached clips: `actors` and `items` as ActorArgs takes
        them (or an ActorArgs), `tensor` a float32 torch tensor on the scene's device that takes the instance transforms at the
        actors' rows, or None (sr_scene_pose_actors)."""
        _actor_call(lib().sr_scene_pose_actors, self._h, actors, items, tensor, keep_nodes, self.device_index)

    def pose_actors_blended(self, actors, items=(), tensor=None, keep_nodes=False, keep_sources=False):
        """pose_actors for actors that cross-fade between two attached clips: `actors` as BlendedActorArgs takes them (or a
        BlendedActorArgs), the rest as pose_actors; keep_sources also stores both sources' sampled TRS for read_actor_sources
        (sr_scene_pose_actors_blended)."""
        _actor_call(lib().sr_scene_pose_actors_blended, self._h, actors, items, tensor, keep_nodes, self.device_index, keep_sources, BlendedActorArgs)

    def attach_node_mask(self, weights):
        """Uploads a node mask once, one float32 in [0, 1] per clip node in clip-node order -> its id on this scene
        (sr_scene_attach_node_mask)."""
        m, mid = _node_mask(weights, "attach_node_mask"), C.c_uint32()
        check(lib().sr_scene_attach_node_mask(self._h, _p(m), C.c_uint32(len(m)), C.byref(mid)))
        return mid.value

    def detach_node_mask(self, mask_id):
        check(lib().sr_scene_detach_node_mask(self._h, C.c_uint32(mask_id)))

    def pose_actors_layered(self, actors, items=(), tensor=None, keep_nodes=False, keep_layers=False, layer_weights=False):
        """pose_actors for actors that are stacks of layers over attached clips: `actors` as LayeredActorArgs takes them (or a
        LayeredActorArgs), the rest as pose_actors; keep_layers also stores every layer's sampled records for read_actor_layer;
        layer_weights has every clip-weighted item take the stack's morph weights, not the base layer's
        (sr_scene_pose_actors_layered, SR_ACTORS_LAYER_WEIGHTS)."""
        _actor_call(lib().sr_scene_pose_actors_layered, self._h, actors, items, tensor, keep_nodes, self.device_index, False, LayeredActorArgs, keep_layers,
                    layer_weights)

    def layer_weights_info(self):
        """-> abi.SrLayerWeightsInfo: the rows, set samples, cubic samples, table bytes and kernel time of the clip-weighted items
        of the last pose_actors_layered that reached the device (sr_scene_layer_weights_info)."""
        info = abi.SrLayerWeightsInfo()
        check(lib().sr_scene_layer_weights_info(self._h, C.byref(info)))
        return info

    def read_actor_layer(self, actor, layer, n_nodes):
        """-> (abi.NODE_TRS [n_nodes], abi.NODE_TRS [n_nodes]): layer `layer`'s sampled records of an actor of the last
        pose_actors_layered with keep_layers, and those at its reference time (zeros for an override layer)
        (sr_scene_read_actor_layer)."""
        cur, ref = np.zeros(max(n_nodes, 1), abi.NODE_TRS), np.zeros(max(n_nodes, 1), abi.NODE_TRS)
        check(lib().sr_scene_read_actor_layer(self._h, C.c_uint32(actor), C.c_uint32(layer), _p(cur), _p(ref)))
        return cur[:n_nodes], ref[:n_nodes]

    def layer_pose_info(self):
        """-> abi.SrLayerPoseInfo: the layers, additive layers, masked layers and layer-table bytes of the last
        pose_actors_layered that reached the device (sr_scene_layer_pose_info)."""
        info = abi.SrLayerPoseInfo()
        check(lib().sr_scene_layer_pose_info(self._h, C.byref(info)))
        return info

    def read_actor_sources(self, actor, n_nodes):
        """-> (abi.NODE_TRS [n_nodes], abi.NODE_TRS [n_nodes]): both sources' sampled TRS of an actor of the last
        pose_actors_blended with keep_sources (sr_scene_read_actor_sources)."""
        a, b = np.zeros(max(n_nodes, 1), abi.NODE_TRS), np.zeros(max(n_nodes, 1), abi.NODE_TRS)
        check(lib().sr_scene_read_actor_sources(self._h, C.c_uint32(actor), _p(a), _p(b)))
        return a[:n_nodes], b[:n_nodes]

    def actor_pose_info(self):
        """-> abi.SrActorPoseInfo: the last pose_actors that reached the device (sr_scene_actor_pose_info)."""
        info = abi.SrActorPoseInfo()
        check(lib().sr_scene_actor_pose_info(self._h, C.byref(info)))
        return info

    def spline_pose_info(self):
        """-> abi.SrSplinePoseInfo: the cubic side of the last pose_actors / pose_actors_blended that reached the device: rows
        of each weights kernel, CUBICSPLINE channels, the spline weights kernel's time (sr_scene_spline_pose_info)."""
        info = abi.SrSplinePoseInfo()
        check(lib().sr_scene_spline_pose_info(self._h, C.byref(info)))
        return info

    def read_actor_nodes(self, actor, n_nodes):
        """-> (abi.NODE_TRS [n_nodes], global matrices [n_nodes, 16] float32) of an actor of the last pose_actors with keep_nodes
        (sr_scene_read_actor_nodes)."""
        trs, g = np.zeros(max(n_nodes, 1), abi.NODE_TRS), np.zeros((max(n_nodes, 1), 16), np.float32)
        check(lib().sr_scene_read_actor_nodes(self._h, C.c_uint32(actor), _p(trs), _p(g)))
        return trs[:n_nodes], g[:n_nodes]

    def read_item_active(self, item, n_targets=65536):
        """-> (target indices uint32 [n_active], weights float32 [n_active]): item `item`'s active list of the last pose_actors
        as the posing kernel read it; n_targets: room for that many (sr_scene_read_item_active)."""
        idx, w, n = np.zeros(max(n_targets, 1), np.uint32), np.zeros(max(n_targets, 1), np.float32), C.c_uint32()
        check(lib().sr_scene_read_item_active(self._h, C.c_uint32(item), _p(idx), _p(w), C.byref(n)))
        return idx[:n.value].copy(), w[:n.value].copy()

    def read_actor_matrices(self, actor, n_joints):
        """-> the joint matrices [n_joints, 12] float32 the posing kernel read for an actor of the last pose_actors
        (sr_scene_read_actor_matrices)."""
        m = np.zeros((max(n_joints, 1), 12), np.float32)
        check(lib().sr_scene_read_actor_matrices(self._h, C.c_uint32(actor), _p(m)))
        return m[:n_joints]

    def mesh_morph_info(self, key):
        """-> abi.SrMeshMorphInfo: the targets of the mesh's morph (0: none), the poses taken, the active targets, the refusal and
        the kernel time of the last one."""
        info = abi.SrMeshMorphInfo()
        check(lib().sr_scene_mesh_morph_info(self._h, C.c_uint64(key), C.byref(info)))
        return info

    def set_mesh_frame(self, key, normals=True, tangents=False):
        """Attaches a frame to a loaded mesh: from then on update_mesh_positions recomputes its normals (and its tangents where
        asked) from new positions alone; the mesh's current vertices become the reference records. normals=False detaches it
        (sr_scene_set_mesh_frame)."""
        flags = _frame_flags(normals, tangents)
        check(lib().sr_scene_set_mesh_frame(self._h, C.c_uint64(key), C.c_uint32(flags)))

    def update_mesh_positions(self, key, positions):
        """New positions for a mesh with a frame, float32 [n_vertices, 3]: a torch tensor on the scene's GPU, produced on torch's
        current stream, stays on the device (sr_scene_update_mesh_positions_device); a numpy array is uploaded, 12 bytes a vertex
        (sr_scene_update_mesh_positions). From there on it is an update_mesh_device: the next set_instances applies it."""
        on_device, ptr, n, stream, keep = _mesh_positions(positions, self.device_index)
        if on_device:
            check(lib().sr_scene_update_mesh_positions_device(self._h, C.c_uint64(key), ptr, C.c_uint32(n), stream))
        else:
            check(lib().sr_scene_update_mesh_positions(self._h, C.c_uint64(key), ptr, C.c_uint32(n), self._stream()))

    def mesh_frame_info(self, key):
        """-> abi.SrMeshFrameInfo: the flags of the mesh's frame (0: none), its groups, entries and longest run, the updates
        taken, the last refusal and kernel time."""
        info = abi.SrMeshFrameInfo()
        check(lib().sr_scene_mesh_frame_info(self._h, C.c_uint64(key), C.byref(info)))
        return info

    def mesh_skin_info(self, key):
        """-> abi.SrMeshSkinInfo: the joints of the mesh's skin (0: none), the poses taken, the last refusal and kernel time."""
        info = abi.SrMeshSkinInfo()
        check(lib().sr_scene_mesh_skin_info(self._h, C.c_uint64(key), C.byref(info)))
        return info

    def mesh_update_info(self):
        """-> abi.SrMeshUpdateInfo of the last update_mesh and of the set_instances that applied it."""
        info = abi.SrMeshUpdateInfo()
        check(lib().sr_scene_mesh_update_info(self._h, C.byref(info)))
        return info

    def set_mesh_build_type(self, key, build_type):
        """abi.BUILD_* of one mesh's tree: an updatable mesh (not BUILD_STATIC, the default) is refitted on the device by the
        set_instances that applies its update_mesh in the two-level form (sr_scene_set_mesh_build_type)."""
        check(lib().sr_scene_set_mesh_build_type(self._h, C.c_uint64(key), C.c_uint32(build_type)))
        return self

    def set_mesh_tree_build(self, mode):
        """Where an updatable mesh's tree is built when its state asks for the fast build: "auto" | "host" | "device"
        (sr_scene_set_mesh_tree_build)."""
        check(lib().sr_scene_set_mesh_tree_build(self._h, C.c_uint32({"auto": 0, "host": 1, "device": 2}[mode])))
        return self

    def set_mesh_tree_batch(self, mode):
        """"on" | "off": whether pending meshes of at most abi.BLAS_BATCH_MAX_TRIS triangles that ask for a fast build are built by one
        batched device launch, a workgroup per mesh (sr_scene_set_mesh_tree_batch). Off by default."""
        check(lib().sr_scene_set_mesh_tree_batch(self._h, C.c_uint32({"off": 0, "on": 1}[mode])))
        return self

    def mesh_tree_batch_info(self):
        """-> abi.SrMeshTreeBatchInfo: the batched mesh-tree builds of the last set_instances (built, passed on, launches, milliseconds)."""
        info = abi.SrMeshTreeBatchInfo()
        check(lib().sr_scene_mesh_tree_batch_info(self._h, C.byref(info)))
        return info

    def mesh_tree_info(self):
        """-> abi.SrMeshTreeInfo: the mesh-tree builds of the last set_instances (device / host counts, reason, milliseconds)."""
        info = abi.SrMeshTreeInfo()
        check(lib().sr_scene_mesh_tree_info(self._h, C.byref(info)))
        return info

    def set_tree_height_bound(self, mode, cap=0):
        """What a device fast build does with a tree taller than its stack cap: "refuse" (the host builds) | "rebalance" (the
        device makes it fit); cap: 0 = the library's 26, or 1..26 for device-built mesh trees (sr_scene_set_tree_height_bound)."""
        check(lib().sr_scene_set_tree_height_bound(self._h, C.c_uint32({"refuse": 0, "rebalance": 1}[mode]), C.c_uint32(cap)))
        return self

    def tree_height_info(self, kind):
        """-> abi.SrTreeHeightInfo of the last device fast build of one abi.TREE_KIND_*."""
        info = abi.SrTreeHeightInfo()
        check(lib().sr_scene_tree_height_info(self._h, C.c_uint32(kind), C.byref(info)))
        return info

    def mesh_as_state(self, key):
        """-> (build type, SrAsState, last op) of one mesh's tree."""
        bt, st, op = C.c_uint32(), abi.SrAsState(), C.c_uint32()
        check(lib().sr_scene_mesh_as_state(self._h, C.c_uint64(key), C.byref(bt), C.byref(st), C.byref(op)))
        return bt.value, st, op.value

    def read_mesh_tree(self, key):
        """-> dict of one mesh's part of the device arrays of a two-level scene: nodes [n_nodes, 16] uint32 (references local to the
        mesh), tris / shade [n_tris, 12] float32, shade_tex [n_tris, 24] float32 (leaf order), slot_of_prim [n_tris] uint32."""
        nn, nt = C.c_uint32(), C.c_uint32()
        check(lib().sr_scene_read_mesh_tree(self._h, C.c_uint64(key), C.byref(nn), C.byref(nt), None, None, None, None, None))
        nodes = np.zeros((max(nn.value, 1), bvh_layout()[1]), dtype=np.uint32)
        tris, shade = np.zeros((max(nt.value, 1), 12), dtype=np.float32), np.zeros((max(nt.value, 1), 12), dtype=np.float32)
        shade_tex, slot_of_prim = np.zeros((max(nt.value, 1), 24), dtype=np.float32), np.zeros(max(nt.value, 1), dtype=np.uint32)
        check(lib().sr_scene_read_mesh_tree(self._h, C.c_uint64(key), None, None, _p(nodes), _p(tris), _p(shade), _p(shade_tex), _p(slot_of_prim)))
        return {"nodes": nodes[:nn.value], "tris": tris[:nt.value], "shade": shade[:nt.value], "shade_tex": shade_tex[:nt.value],
                "slot_of_prim": slot_of_prim[:nt.value]}

    # Image::new_from_data (image/mod.rs:82-111) / Sampler::new (image/sampler.rs:44-67)
    def add_image(self, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        h, w = a.shape[0], a.shape[1]
        ch = 1 if a.ndim == 2 else a.shape[2]
        slot = C.c_uint32()
        check(lib().sr_scene_add_image(self._h, _p(a), C.c_uint32(w), C.c_uint32(h), C.c_uint32(ch), C.byref(slot)))
        return slot.value

    def add_sampler(self, min_filter, mag_filter, address_mode_u, address_mode_v):
        d = abi.SrSamplerDesc(min_filter, mag_filter, address_mode_u, address_mode_v)
        slot = C.c_uint32()
        check(lib().sr_scene_add_sampler(self._h, C.byref(d), C.byref(slot)))
        return slot.value

    # frame_instance_data (resource_manager.rs:216-267) + TLAS build
    def set_instances(self, instances):
        keys = np.array([k for k, _ in instances], dtype=np.uint64)
        counts = np.array([len(t) for _, t in instances], dtype=np.uint32)
        xf = np.array([np.asarray(t, dtype=np.float32).reshape(12) for _, ts in instances for t in ts], dtype=np.float32).reshape(-1, 12)
        if len(xf) == 0:
            xf = np.zeros((1, 12), dtype=np.float32)
        check(lib().sr_scene_set_instances(self._h, _p(keys), _p(counts), C.c_uint32(len(keys)), _p(np.ascontiguousarray(xf))))

    def set_instances_device(self, layout, tensor):
        """set_instances for transforms that are on the GPU already: `layout` is [(key, count), ...], `tensor` a contiguous
        float32 torch tensor on the scene's device with sum(counts) x 12 elements (row-major 3x4 each), produced on torch's
        current stream (sr_scene_set_instances_device)."""
        import torch
        keys, counts, ptr = _device_transforms(layout, tensor, self.device_index)
        check(lib().sr_scene_set_instances_device(self._h, _p(keys), _p(counts), C.c_uint32(len(keys)), ptr,
                                                  C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)))

    def instance_update_info(self):
        """-> abi.SrInstanceUpdateInfo: where the last instance list came from, whether the library's host copy of the transforms
        is behind the device tables, the fetches since and why, and the kernel's milliseconds."""
        info = abi.SrInstanceUpdateInfo()
        check(lib().sr_scene_instance_update_info(self._h, C.byref(info)))
        return info

    def read_instance_tables(self):
        """-> (abi.DEV_INSTANCE [n], abi.FLAT_INSTANCE [n]): the per-instance device tables, whichever path wrote them."""
        n = self.instance_update_info().n_instances
        dev, flat = np.zeros(max(n, 1), dtype=abi.DEV_INSTANCE), np.zeros(max(n, 1), dtype=abi.FLAT_INSTANCE)
        check(lib().sr_scene_read_instance_tables(self._h, _p(dev), _p(flat)))
        return dev[:n], flat[:n]

    def tile_row_costs(self, which, width, y0, rows):
        """Measured cycles per 8-pixel tile row of the last launch of pass `which` (0 ris, 1 final) with this geometry."""
        out = np.zeros((rows + 7) // 8 + 1, dtype=np.float64)
        n = C.c_uint32()
        check(lib().sr_scene_read_tile_row_costs(self._h, C.c_int(which), C.c_uint32(width), C.c_uint32(y0), C.c_uint32(rows), _p(out),
                                                 C.c_uint32(len(out)), C.byref(n)))
        return out[:n.value]

    def tile_costs(self, which, width, y0, rows):
        """Measured cycles of every 8x8 tile (row-major, ty * tiles_x + tx) of the last full-width launch of pass `which`."""
        out = np.zeros(((width + 7) // 8) * ((rows + 7) // 8), dtype=np.uint32)
        n = C.c_uint32()
        check(lib().sr_scene_read_tile_costs(self._h, C.c_int(which), C.c_uint32(width), C.c_uint32(y0), C.c_uint32(rows), _p(out),
                                             C.c_uint32(len(out)), C.byref(n)))
        return out[:n.value]

    def set_tile_costs(self, which, x0, width, y0, rows, costs):
        """Test hook: injects per-tile costs (uint32, row-major, one per 8x8 tile) for pass `which` and the launch rectangle of
        `width` columns from x0 and `rows` rows from y0; the next launch of that geometry runs in the order derived from them
        (sr_scene_set_tile_costs)."""
        c = None if costs is None else np.ascontiguousarray(costs, dtype=np.uint32).reshape(-1)
        check(lib().sr_scene_set_tile_costs(self._h, C.c_int(which), C.c_uint32(x0), C.c_uint32(width), C.c_uint32(y0), C.c_uint32(rows),
                                            None if c is None else _p(c), C.c_uint32(0 if c is None else len(c))))
        return self

    def tile_order(self, which, x0, width, y0, rows):
        """Test hook -> ([8, order_cap] uint32, order_cap): the tile lists of the eight column bands the next launch of that
        geometry would read, abi.TILE_ORDER_NONE after a list's last tile (sr_scene_read_tile_order)."""
        tiles_x, tiles_y = (width + 7) // 8, (rows + 7) // 8
        out = np.zeros(8 * max(tiles_x, 1) * max(tiles_y, 1), dtype=np.uint32)      # a band is never wider than the rectangle
        cap = C.c_uint32()
        check(lib().sr_scene_read_tile_order(self._h, C.c_int(which), C.c_uint32(x0), C.c_uint32(width), C.c_uint32(y0), C.c_uint32(rows),
                                             _p(out), C.c_uint32(len(out)), C.byref(cap)))
        return out[:8 * cap.value].reshape(8, cap.value).copy(), cap.value

    def light_stage_capacity(self):
        """Test hook: the longest light table a wave of the RIS pass keeps in its LDS for the candidate loop, in lights
        (sr_scene_light_stage_capacity); longer tables are read from global memory."""
        n = C.c_uint32()
        check(lib().sr_scene_light_stage_capacity(self._h, C.byref(n)))
        return n.value

    def set_instancing(self, mode):
        """Form of the acceleration structure at the next set_instances: "auto" | "flat" | "two_level" (sr_scene_set_instancing)."""
        check(lib().sr_scene_set_instancing(self._h, C.c_uint32({"auto": 0, "flat": 1, "two_level": 2}[mode])))
        return self

    def two_level(self):
        """True while the structure is built in the two-level form."""
        now = C.c_uint32()
        check(lib().sr_scene_instancing(self._h, None, C.byref(now)))
        return bool(now.value)

    def set_top_level_build(self, mode):
        """Where a changed instance list of a two-level scene gets its top-level tree: "auto" | "host" | "device"
        (sr_scene_set_top_level_build)."""
        check(lib().sr_scene_set_top_level_build(self._h, C.c_uint32({"auto": 0, "host": 1, "device": 2}[mode])))
        return self

    def top_level_info(self):
        """-> abi.SrTopLevelInfo of the last top-level build (path taken, reason, counts, stack, milliseconds)."""
        info = abi.SrTopLevelInfo()
        check(lib().sr_scene_top_level_info(self._h, C.byref(info)))
        return info

    def read_top_level(self):
        """-> (nodes [n_nodes, 16] uint32, tl_inst [n_boxes] uint32, records [n_instances] abi.TL_INSTANCE, boxes [n_instances, 6]
        float32, a NaN row where the instance has no box) of a scene built in the two-level form."""
        info = self.top_level_info()
        nodes = np.zeros((max(info.n_nodes, 1), bvh_layout()[1]), dtype=np.uint32)
        tl_inst = np.zeros(max(info.n_boxes, 1), dtype=np.uint32)
        records = np.zeros(max(info.n_instances, 1), dtype=abi.TL_INSTANCE)
        boxes = np.zeros((max(info.n_instances, 1), 6), dtype=np.float32)
        check(lib().sr_scene_read_top_level(self._h, _p(nodes), _p(tl_inst), _p(records), _p(boxes)))
        return nodes[:info.n_nodes], tl_inst[:info.n_boxes], records[:info.n_instances], boxes[:info.n_instances]

    def force_next_op(self, op):
        check(lib().sr_scene_force_next_op(self._h, C.c_uint32(op)))

    def end_frame(self):
        check(lib().sr_scene_end_frame(self._h))

    def as_state(self):
        """-> (SrAsState, last op) of the scene's acceleration structure."""
        st, op = abi.SrAsState(), C.c_uint32()
        check(lib().sr_scene_as_state(self._h, C.byref(st), C.byref(op)))
        return st, op.value

    def read_bvh(self):
        st = self.bvh_stats()
        nodes = np.zeros((st.n_nodes, bvh_layout()[1]), dtype=np.uint32)
        tris = np.zeros((max(st.n_triangles, 1), 12), dtype=np.float32)
        check(lib().sr_scene_read_bvh(self._h, _p(nodes), _p(tris)))
        return nodes, tris[:st.n_triangles]

    def set_light_table_build(self, mode):
        """Where set_instances builds the light table: "host" (default) | "device" (sr_scene_set_light_table_build)."""
        check(lib().sr_scene_set_light_table_build(self._h, C.c_uint32({"host": abi.LIGHTS_HOST, "device": abi.LIGHTS_DEVICE}[mode])))
        return self

    def light_table_info(self):
        """-> abi.SrLightTableInfo: the light table of the last set_instances (where it was built, uploads, fetches, milliseconds)."""
        info = abi.SrLightTableInfo()
        check(lib().sr_scene_light_table_info(self._h, C.byref(info)))
        return info

    def read_lights(self):
        """The device light table, (num_lights, 16) float32: world v0 + area, v1 + normal x, v2 + normal y, emission + normal z."""
        n = C.c_uint32()
        check(lib().sr_scene_read_lights(self._h, None, C.c_uint32(0), C.byref(n)))
        out = np.zeros((n.value, 16), dtype=np.float32)
        check(lib().sr_scene_read_lights(self._h, _p(out), C.c_uint32(n.value), C.byref(n)))
        return out

    def load(self, desc):
        for img in desc.images:
            self.add_image(img)
        for smp in desc.samplers:
            self.add_sampler(*smp)
        for m in desc.meshes:
            self.add_mesh(m.key, m.vertices, m.indices, m.material)
        self.set_instances(desc.instances)
        return self

    def tables(self):
        tp, ip, ep, mp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nt, nl, ne, nm = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().sr_scene_get_tables(self._h, C.byref(tp), C.byref(nt), C.byref(ip), C.byref(nl), C.byref(ep), C.byref(ne), C.byref(mp), C.byref(nm)))

        def arr(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (n * dt.itemsize)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=dt).copy()
        return {"transforms": arr(tp, nt.value, abi.TRANSFORM), "indirection": arr(ip, nl.value, abi.EMISSIVE_INDIRECTION),
                "emissive_triangles": arr(ep, ne.value, abi.EMISSIVE_TRIANGLE), "num_lights": nl.value,
                "meshes_info": arr(mp, nm.value, abi.MESH_INFO)}

    def bvh_stats(self):
        s = abi.SrBvhStats()
        check(lib().sr_scene_bvh_stats(self._h, C.byref(s)))
        return s

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # TraceRay test hooks: torch uint8/any tensors holding abi.RAY records
    def trace_closest(self, rays_t, n):
        import torch
        hits = torch.empty(n, 4, dtype=torch.float32, device=rays_t.device)
        check(lib().sr_trace_closest(self._h, C.c_void_p(rays_t.data_ptr()), C.c_uint32(n), C.c_void_p(hits.data_ptr()), self._stream()))
        return hits

    def trace_any(self, rays_t, n):
        import torch
        occ = torch.empty(n, dtype=torch.int32, device=rays_t.device)
        check(lib().sr_trace_any(self._h, C.c_void_p(rays_t.data_ptr()), C.c_uint32(n), C.c_void_p(occ.data_ptr()), self._stream()))
        return occ

    def shade_closest_hit(self, hits_t, n):
        import torch
        out = torch.empty(n, 8, dtype=torch.int32, device=hits_t.device)
        check(lib().sr_shade_closest_hit(self._h, C.c_void_p(hits_t.data_ptr()), C.c_uint32(n), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def any_hit_ignores(self, hits_t, n):
        import torch
        out = torch.empty(n, dtype=torch.int32, device=hits_t.device)
        check(lib().sr_any_hit_ignores(self._h, C.c_void_p(hits_t.data_ptr()), C.c_uint32(n), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def params(self, frame, matrices, frame_count, config=None, tile=None):
        p = abi.SrRtParams()
        p.scene = self._h
        p.raw_color = frame.raw_color.data_ptr()
        p.depth_img = frame.depth.data_ptr()
        p.normal_img = frame.normal.data_ptr()
        p.diffuse_img = frame.diffuse.data_ptr()
        p.motion_vec_img = frame.motion.data_ptr()
        self._m = matrices
        p.matrices = C.pointer(matrices)
        p.blue_noise_tex = frame.blue_noise.data_ptr()
        p.blue_noise_h, p.blue_noise_w = frame.blue_noise_shape
        p.reservoirs[0], p.reservoirs[1] = frame.reservoirs[0].data_ptr(), frame.reservoirs[1].data_ptr()
        p.reservoirs_gi[0], p.reservoirs_gi[1] = frame.reservoirs_gi[0].data_ptr(), frame.reservoirs_gi[1].data_ptr()
        prim = getattr(frame, "primary", None)
        p.primary_payload = prim.data_ptr() if prim is not None else None
        p.frame_count = frame_count
        p.use_srgb = 0
        p.width, p.height = frame.width, frame.height
        if tile:                      # (y0, h) rows, or (y0, h, x0, w) rows x columns; h == 0 / w == 0: all of them
            p.tile_y0, p.tile_h = tile[0], tile[1]
            if len(tile) == 4:
                p.tile_x0, p.tile_w = tile[2], tile[3]
        p.config = config or abi.SrTraceConfig.reference()
        return p

    def trace_ris(self, frame, matrices, frame_count, config=None, tile=None):
        p = self.params(frame, matrices, frame_count, config, tile)
        check(lib().sr_trace_ris(C.byref(p), self._stream()))

    def trace_final(self, frame, matrices, frame_count, config=None, tile=None):
        p = self.params(frame, matrices, frame_count, config, tile)
        check(lib().sr_trace_final(C.byref(p), self._stream()))

    def reset_counters(self):
        check(lib().sr_scene_reset_counters(self._h, self._stream()))

    def counters(self):
        c = abi.SrRayCounters()
        check(lib().sr_scene_read_counters(self._h, self._stream(), C.byref(c)))
        return c

    def set_instrumented(self, on):
        check(lib().sr_scene_set_instrumented(self._h, C.c_int(1 if on else 0)))

    def enable_timing(self, on):
        check(lib().sr_scene_enable_timing(self._h, C.c_int(1 if on else 0)))

    def read_timing(self, kind):
        ms, n = C.c_double(), C.c_uint32()
        check(lib().sr_scene_read_timing(self._h, C.c_int(kind), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def probe_helper_layout(fn):
    """(input dwords, output dwords) of one row of helper `fn` (abi.PROBE_HELPERS index); raises for an unknown id. Host only."""
    i, o = C.c_uint32(), C.c_uint32()
    check(lib().sr_probe_helper_layout(C.c_uint32(fn), C.byref(i), C.byref(o)))
    return i.value, o.value


def probe_helper(fn, rows, out):
    """sr_probe_helper on the current stream: helper `fn` on the first len(rows) / width rows of the int32 device tensor `rows`,
    results into the int32 device tensor `out` (test hook: tests/test_gpu_helper_probe.py)."""
    iw, ow = probe_helper_layout(fn)
    n = rows.numel() // iw
    assert out.numel() >= n * ow
    check(lib().sr_probe_helper(C.c_uint32(fn), C.c_void_p(rows.data_ptr()), C.c_uint32(n), C.c_void_p(out.data_ptr()), _stream()))
    return n


def probe_node_step(kind, rows):
    """sr_probe_node_step: the traversal of kind abi.NODE_PROBE_* on the host rows `rows` (abi.NODE_PROBE_ROW), one hand-made
    node per ray -> abi.NODE_PROBE_OUT per row (test hook: tests/test_gpu_node_step.py)."""
    rows = np.ascontiguousarray(rows, dtype=abi.NODE_PROBE_ROW)
    out = np.zeros(len(rows), dtype=abi.NODE_PROBE_OUT)
    check(lib().sr_probe_node_step(C.c_uint32(kind), _p(rows), C.c_uint32(len(rows)), _p(out)))
    return out


def probe_tl_record(o2w, mesh_lo, mesh_hi, max_abs_vertex=0.0, max_edge_sum=0.0):
    """sr_probe_tl_record: (record as one abi.TL_INSTANCE, abi.TL_RECORD_* result) of the instance transform `o2w` (3 x 4) over a
    mesh with the root box mesh_lo .. mesh_hi. Host only."""
    m = np.ascontiguousarray(o2w, dtype=np.float32).reshape(12)
    lo, hi = np.ascontiguousarray(mesh_lo, dtype=np.float32).reshape(3), np.ascontiguousarray(mesh_hi, dtype=np.float32).reshape(3)
    rec = np.zeros(1, dtype=abi.TL_INSTANCE)
    res = C.c_uint32()
    check(lib().sr_probe_tl_record(_p(m), _p(lo), _p(hi), C.c_float(max_abs_vertex), C.c_float(max_edge_sum), _p(rec), C.byref(res)))
    return rec[0], res.value


def post_chain(frame, frame_count, exposure=1.0, denoise_passes=4):
    """temporal_accumulation -> denoise_0..N-1 -> postprocess on the current stream (lib.rs:1576-1615)."""
    p = abi.post_params(frame, frame_count, lambda t: t.data_ptr(), exposure, denoise_passes)
    check(lib().sr_post_temporal(C.byref(p), _stream()))
    check(lib().sr_post_denoise(C.byref(p), _stream()))
    check(lib().sr_post_tonemap(C.byref(p), _stream()))


def _addr(x):
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)


def _strip_planes(planes):
    """[(tensor or device address, bytes per pixel)] -> SrStripPlane array."""
    arr = (abi.SrStripPlane * max(len(planes), 1))()
    for i, (img, bpp) in enumerate(planes):
        arr[i].img, arr[i].bpp = _addr(img), bpp
    return arr


def strip_packed_bytes(bpps, w, h):
    """Size of the packed form of a w x h rectangle of planes with these bytes per pixel (sr_strip_packed_bytes)."""
    n = C.c_uint64()
    check(lib().sr_strip_packed_bytes(_strip_planes([(0, b) for b in bpps]), C.c_uint32(len(bpps)), C.c_uint32(w), C.c_uint32(h), C.byref(n)))
    return n.value


def _strip_copy(fn, planes, size, rect, packed, stream):
    (W, H), (x0, w, y0, h) = size, rect
    check(fn(_strip_planes(planes), C.c_uint32(len(planes)), C.c_uint32(W), C.c_uint32(H), C.c_uint32(x0), C.c_uint32(w),
             C.c_uint32(y0), C.c_uint32(h), _addr(packed), _stream() if stream is None else C.c_void_p(stream)))


def strip_pack(planes, size, rect, packed, stream=None):
    """sr_strip_pack: rectangle (x0, w, y0, h) of the planes [(tensor or address, bpp)] of (W, H) images -> packed."""
    _strip_copy(lib().sr_strip_pack, planes, size, rect, packed, stream)


def strip_unpack(planes, size, rect, packed, stream=None):
    """sr_strip_unpack: packed -> rectangle (x0, w, y0, h) of the planes."""
    _strip_copy(lib().sr_strip_unpack, planes, size, rect, packed, stream)


def history_reach_check(motion, size, axis, rect, held, counter, stream=None):
    """sr_history_reach_check: adds to the device uint64 at `counter` the pixels of rectangle (x0, w, y0, h) whose history read
    may leave held = (lo, hi) along `axis` (abi.AXIS_COLS / AXIS_ROWS)."""
    (W, H), (x0, w, y0, h) = size, rect
    check(lib().sr_history_reach_check(_addr(motion), C.c_uint32(W), C.c_uint32(H), C.c_uint32(axis), C.c_uint32(x0), C.c_uint32(w),
                                       C.c_uint32(y0), C.c_uint32(h), C.c_uint32(held[0]), C.c_uint32(held[1]), _addr(counter),
                                       _stream() if stream is None else C.c_void_p(stream)))


def _instance_arrays(instances):
    keys = np.array([k for k, _ in instances], dtype=np.uint64)
    counts = np.array([len(t) for _, t in instances], dtype=np.uint32)
    xf = np.array([np.asarray(t, dtype=np.float32).reshape(12) for _, ts in instances for t in ts], dtype=np.float32).reshape(-1, 12)
    if len(xf) == 0:
        xf = np.zeros((1, 12), dtype=np.float32)
    return keys, counts, np.ascontiguousarray(xf)


def default_noise_texture(w=128, h=128, seed=7):
    out = np.zeros((h, w, 4), dtype=np.uint8)
    check(lib().sr_default_noise_texture(C.c_uint32(w), C.c_uint32(h), C.c_uint32(seed), _p(out)))
    return out


def _np_from(ptr, n, dt):
    if n == 0:
        return np.zeros(0, dtype=dt)
    buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr.value)
    return np.frombuffer(buf, dtype=dt).copy()


def gltf_parse(path):
    """sr_gltf_open + accessors -> dict(blases=[dict(vertices, indices, material (unresolved), emissive)], instances=[(blas, 3x4)],
    images=[(h,w,c) uint8], samplers=[(min, mag, u, v)], textures=[(sampler or -1, source)])."""
    g = C.c_void_p()
    check(lib().sr_gltf_open(path.encode(), C.byref(g)))
    try:
        nb, ni, nim, ns, nt = (C.c_uint32() for _ in range(5))
        check(lib().sr_gltf_counts(g, C.byref(nb), C.byref(ni), C.byref(nim), C.byref(ns), C.byref(nt)))
        out = dict(blases=[], instances=[], images=[], samplers=[], textures=[])
        for i in range(nb.value):
            vp, ip, ep = C.c_void_p(), C.c_void_p(), C.c_void_p()
            nv, nx, ne = C.c_uint32(), C.c_uint32(), C.c_uint32()
            m = np.zeros((), dtype=abi.MATERIAL)
            check(lib().sr_gltf_blas(g, C.c_uint32(i), C.byref(vp), C.byref(nv), C.byref(ip), C.byref(nx), _p(m), C.byref(ep), C.byref(ne)))
            out["blases"].append(dict(vertices=_np_from(vp, nv.value, abi.VERTEX), indices=_np_from(ip, nx.value, np.uint32), material=m,
                                      emissive=_np_from(ep, ne.value, abi.EMISSIVE_TRIANGLE)))
        for i in range(ni.value):
            b = C.c_uint32()
            t = np.zeros(12, dtype=np.float32)
            check(lib().sr_gltf_instance(g, C.c_uint32(i), C.byref(b), _p(t)))
            out["instances"].append((b.value, t))
        for i in range(nim.value):
            pp = C.c_void_p()
            w, h, ch = C.c_uint32(), C.c_uint32(), C.c_uint32()
            check(lib().sr_gltf_image(g, C.c_uint32(i), C.byref(pp), C.byref(w), C.byref(h), C.byref(ch)))
            out["images"].append(_np_from(pp, w.value * h.value * ch.value, np.uint8).reshape(h.value, w.value, ch.value))
        for i in range(ns.value):
            d = abi.SrSamplerDesc()
            check(lib().sr_gltf_sampler(g, C.c_uint32(i), C.byref(d)))
            out["samplers"].append((d.min_filter, d.mag_filter, d.address_mode_u, d.address_mode_v))
        for i in range(nt.value):
            sm, src = C.c_int32(), C.c_uint32()
            check(lib().sr_gltf_texture(g, C.c_uint32(i), C.byref(sm), C.byref(src)))
            out["textures"].append((sm.value, src.value))
        return out
    finally:
        lib().sr_gltf_close(g)


class Gltf:
    """An open glTF file (sr_gltf_open) for the calls that need it beyond the load: the rig read-outs and pose()."""

    def __init__(self, path):
        self._h = C.c_void_p()
        check(lib().sr_gltf_open(path.encode(), C.byref(self._h)))
        nb, ni = C.c_uint32(), C.c_uint32()
        check(lib().sr_gltf_counts(self._h, C.byref(nb), C.byref(ni), None, None, None))
        self.n_blases, self.n_instances = nb.value, ni.value

    def close(self):
        if getattr(self, "_h", None):
            lib().sr_gltf_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rig_counts(self):
        """-> (skins, animations) of the file."""
        ns, na = C.c_uint32(), C.c_uint32()
        check(lib().sr_gltf_rig_counts(self._h, C.byref(ns), C.byref(na)))
        return ns.value, na.value

    def blas_skin(self, blas):
        """-> (skin index or -1, abi.SKIN_INFLUENCE array with one record per vertex of the blas, or None)."""
        sk, ip, nv = C.c_int32(), C.c_void_p(), C.c_uint32()
        check(lib().sr_gltf_blas_skin(self._h, C.c_uint32(blas), C.byref(sk), C.byref(ip), C.byref(nv)))
        return sk.value, (_np_from(ip, nv.value, abi.SKIN_INFLUENCE) if sk.value >= 0 else None)

    def skin(self, i):
        """-> (inverse bind matrices [n_joints, 12] float32, joint node indices [n_joints] uint32)."""
        nj, mp, jp = C.c_uint32(), C.c_void_p(), C.c_void_p()
        check(lib().sr_gltf_skin(self._h, C.c_uint32(i), C.byref(nj), C.byref(mp), C.byref(jp)))
        return _np_from(mp, nj.value * 12, np.float32).reshape(-1, 12), _np_from(jp, nj.value, np.uint32)

    def blas_morph(self, blas):
        """-> (abi.MORPH_DELTA array of shape (n_targets, n_vertices), default weights [n_targets] float32) of the blas's morph
        targets, or (None, None) where it has none (sr_gltf_blas_morph)."""
        nt, dp, nv, wp = C.c_uint32(), C.c_void_p(), C.c_uint32(), C.c_void_p()
        check(lib().sr_gltf_blas_morph(self._h, C.c_uint32(blas), C.byref(nt), C.byref(dp), C.byref(nv), C.byref(wp)))
        if nt.value == 0:
            return None, None
        return _np_from(dp, nt.value * nv.value, abi.MORPH_DELTA).reshape(nt.value, nv.value), _np_from(wp, nt.value, np.float32)

    def morph_weights(self, animation, time_seconds, blas):
        """-> the weights [n_targets] float32 of the blas's morph targets at `time_seconds` of `animation` (-1: the file's default
        weights) (sr_gltf_morph_weights)."""
        nt = C.c_uint32()
        check(lib().sr_gltf_blas_morph(self._h, C.c_uint32(blas), C.byref(nt), None, None, None))
        w = np.zeros(max(nt.value, 1), dtype=np.float32)
        check(lib().sr_gltf_morph_weights(self._h, C.c_int32(animation), C.c_float(time_seconds), C.c_uint32(blas), _p(w), nt))
        return w[:nt.value]

    def animation(self, i):
        """-> (name, duration in seconds, channels the file lists, of which `weights` channels that are not sampled)."""
        name, dur, nc, nw = C.c_char_p(), C.c_float(), C.c_uint32(), C.c_uint32()
        check(lib().sr_gltf_animation(self._h, C.c_uint32(i), C.byref(name), C.byref(dur), C.byref(nc)))
        check(lib().sr_gltf_animation_ignored_channels(self._h, C.c_uint32(i), C.byref(nw)))
        return (name.value or b"").decode("utf-8", "replace"), dur.value, nc.value, nw.value

    def set_cubicspline(self, sample):
        """CUBICSPLINE samplers of this file: True samples them (SR_CUBICSPLINE_SAMPLE), False refuses them as ever
        (SR_CUBICSPLINE_REFUSE, the default). Read by pose, sample_node, morph_weights and bake_clip when they meet one; a clip
        keeps what it was baked with (sr_gltf_set_cubicspline)."""
        check(lib().sr_gltf_set_cubicspline(self._h, C.c_uint32(abi.CUBICSPLINE_SAMPLE if sample else abi.CUBICSPLINE_REFUSE)))

    @property
    def cubicspline(self):
        """True while CUBICSPLINE samplers are sampled (sr_gltf_cubicspline)."""
        mode = C.c_uint32()
        check(lib().sr_gltf_cubicspline(self._h, C.byref(mode)))
        return mode.value == abi.CUBICSPLINE_SAMPLE

    def animation_cubic(self, i):
        """-> (translation / rotation / scale channels, `weights` channels) of animation i that name a CUBICSPLINE sampler, in
        either mode: (0, 0) where the animation does not need set_cubicspline (sr_gltf_animation_cubic)."""
        nc, nw = C.c_uint32(), C.c_uint32()
        check(lib().sr_gltf_animation_cubic(self._h, C.c_uint32(i), C.byref(nc), C.byref(nw)))
        return nc.value, nw.value

    def pose(self, animation, time_seconds, skin=None):
        """The file at `time_seconds` of `animation` (-1: its static pose) -> (instance transforms [n_instances, 12] float32, joint
        matrices [n_joints, 12] float32 of `skin`, or None without one) (sr_gltf_pose)."""
        xf = np.zeros((max(self.n_instances, 1), 12), dtype=np.float32)
        joints = None
        if skin is not None:
            joints = np.zeros((len(self.skin(skin)[1]), 12), dtype=np.float32)
        check(lib().sr_gltf_pose(self._h, C.c_int32(animation), C.c_float(time_seconds), _p(xf), C.c_uint32(skin or 0),
                                 None if joints is None else _p(joints)))
        return xf[:self.n_instances], joints


    def bake_clip(self, animation):
        """Animation `animation` of the file (-1: its static pose) as a baked Clip (sr_gltf_bake_clip)."""
        h = C.c_void_p()
        check(lib().sr_gltf_bake_clip(self._h, C.c_int32(animation), C.byref(h)))
        return Clip(h)

    def instance_blases(self):
        """-> the blas index of every instance, in sr_gltf_instance order (uint32)."""
        out, b = np.zeros(self.n_instances, np.uint32), C.c_uint32()
        for i in range(self.n_instances):
            check(lib().sr_gltf_instance(self._h, C.c_uint32(i), C.byref(b), None))
            out[i] = b.value
        return out

    def sample_node(self, animation, time_seconds, node):
        """-> (translation [3], rotation [4], scale [3] float32, mask of the animated channels) node `node` composes from in pose()."""
        t, q, s, m = np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32), C.c_uint32()
        check(lib().sr_gltf_sample_node(self._h, C.c_int32(animation), C.c_float(time_seconds), C.c_uint32(node), _p(t), _p(q), _p(s), C.byref(m)))
        return t, q, s, m.value


class LoadedScene:
    """What Renderer.load_scene returns (sr_renderer_load_scene): .group, .instances = [(key, [3x4 transforms])]; kept for
    Renderer.attach_skins / pose_scene."""

    def __init__(self, handle):
        self._h = handle
        group, nk, nt = C.c_uint64(), C.c_uint32(), C.c_uint32()
        kp, cp, tp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sr_loaded_scene_get(self._h, C.byref(group), C.byref(kp), C.byref(cp), C.byref(nk), C.byref(tp), C.byref(nt)))
        self.group = group.value
        self.keys, self.counts = _np_from(kp, nk.value, np.uint64), _np_from(cp, nk.value, np.uint32)
        self.n_transforms = nt.value
        self.instance_blas = None
        self.instances =self.grouped(_np_from(tp, nt.value * 12, np.float32).reshape(-1, 12))

    def grouped(self, transforms):
        """[n_transforms, 12] in the loaded scene's order -> [(key, [3x4 transforms])], what Renderer.render takes."""
        inst, o = [], 0
        for k, c in zip(self.keys, self.counts):
            inst.append((int(k), [transforms[o + j].copy() for j in range(int(c))]))
            o += int(c)
        return inst

    def instance_rows(self, base=0):
        """-> uint32 [n_transforms]: for every instance in sr_gltf_instance order, its row in the order grouped() takes (by blas,
        the file's order kept within one), counted from `base`: what an actor's instance_rows are when a crowd's transforms lie
        copy after copy. Needs the scene to come from Renderer.load_scene, which notes the file's blas of every instance."""
        if self.instance_blas is None:
            raise ValueError("instance_rows: the loaded scene does not know the file's instance order (Renderer.load_scene notes it)")
        order = np.argsort(self.instance_blas, kind="stable")
        rows = np.zeros(len(order), np.uint32)
        rows[order] = np.arange(len(order), dtype=np.uint32)
        return (rows + np.uint32(base)).astype(np.uint32)

    def layout(self):
        """-> [(key, count), ...]: what set_instances_device / render_device_transforms take beside the tensor."""
        return [(int(k), int(c)) for k, c in zip(self.keys, self.counts)]

    def close(self):
        if getattr(self, "_h", None):
            lib().sr_loaded_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SceneView(Scene):
    """A scene owned by someone else (a renderer's replica): the Scene methods without destroying it."""

    def __init__(self, handle, device_index):
        self._h = handle
        self.device_index = device_index

    def close(self):
        self._h = None

    @staticmethod
    def _stream():
        return None         # the null stream of the scene's own device (the library binds it): slots may sit on other devices


class Renderer:
    """The reference's `Renderer<K>` surface for the built path (src/lib.rs:212-446, 586-639, 873-954,
    984-1238, 1908-1934), over sr_renderer_*. `camera` = (position, target, fov_y_degrees) — the
    reference's Camera (camera.rs:11-44); `instances` = [(mesh key, [3x4 row-major transform, ...]), ...]."""

    def __init__(self, size, device_index=0, devices=None, axis="cols", bounds=None, motion_halo=None):
        """`devices` (a list of device indices, repeats allowed) renders every frame across that many device slots
        (sr_renderer_create_multi): column or row strips (`axis`), cut equally or at `bounds` (len(devices) + 1 cuts), with
        temporal-history bands of `motion_halo` pixels exchanged after every RIS pass (default 32). Output on devices[0]."""
        self._h = C.c_void_p()
        self.size = (int(size[0]), int(size[1]))
        if devices is None:
            if bounds is not None or motion_halo is not None or axis != "cols":
                raise ValueError("axis, bounds and motion_halo need devices")
            check(lib().sr_renderer_create(C.c_int(device_index), C.c_uint32(self.size[0]), C.c_uint32(self.size[1]), C.byref(self._h)))
            self.devices = [int(device_index)]
            return
        if axis not in ("cols", "rows"):
            raise ValueError("axis must be 'cols' or 'rows'")
        devs = [int(d) for d in devices]
        if bounds is not None and len(bounds) != len(devs) + 1:
            raise ValueError("bounds must be %d cuts (one more than the devices)" % (len(devs) + 1))
        arr = (C.c_int * max(len(devs), 1))(*devs)
        check(lib().sr_renderer_create_multi(arr, C.c_uint32(len(devs)), C.c_uint32(self.size[0]), C.c_uint32(self.size[1]),
                                             C.c_uint32(0 if axis == "cols" else 1), C.byref(self._h)))
        self.devices = devs
        if bounds is not None:
            self.set_strip_bounds(bounds)
        if motion_halo is not None:
            self.set_motion_halo(motion_halo)

    def set_strip_bounds(self, bounds):
        b = [int(v) for v in bounds]
        if len(b) != len(self.devices) + 1 or any(v < 0 for v in b):
            raise ValueError("bounds must be %d increasing cuts" % (len(self.devices) + 1))
        check(lib().sr_renderer_set_strip_bounds(self._h, (C.c_uint32 * len(b))(*b)))

    def set_motion_halo(self, pixels):
        if int(pixels) < 0:
            raise ValueError("motion_halo must not be negative")
        check(lib().sr_renderer_set_motion_halo(self._h, C.c_uint32(int(pixels))))

    def replica_scene(self, i):
        """A non-owning view of slot i's scene (ray counters, stats): valid while the renderer lives."""
        h = C.c_void_p()
        check(lib().sr_renderer_replica_scene(self._h, C.c_uint32(int(i)), C.byref(h)))
        return _SceneView(h, self.devices[int(i)])

    def history_overflow(self):
        """Pixels, since create / resize, whose temporal-history read may have left what their slot held (synchronising).
        0 means every frame so far equals the single-device frame."""
        n = C.c_uint64()
        check(lib().sr_renderer_read_history_overflow(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            lib().sr_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resize(self, size):
        check(lib().sr_renderer_resize(self._h, C.c_uint32(int(size[0])), C.c_uint32(int(size[1]))))
        self.size = (int(size[0]), int(size[1]))

    # Frame / resize callbacks (lib.rs:537-554). The ctypes thunks are kept alive for the renderer's lifetime.
    _FRAME_CB = C.CFUNCTYPE(None, C.c_void_p)
    _RESIZE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32)

    def _keep(self, thunk):
        self.__dict__.setdefault("_thunks", []).append(thunk)
        return thunk

    def add_start_of_frame_callback(self, fn):
        check(lib().sr_renderer_add_start_of_frame_callback(self._h, self._keep(self._FRAME_CB(lambda _u: fn())), None))

    def add_end_of_frame_callback(self, fn):
        check(lib().sr_renderer_add_end_of_frame_callback(self._h, self._keep(self._FRAME_CB(lambda _u: fn())), None))

    def add_resize_callback(self, fn):
        check(lib().sr_renderer_add_resize_callback(self._h, self._keep(self._RESIZE_CB(lambda _u, w, h: fn((w, h)))), None))

    def set_blue_noise(self, rgba8):
        """Replaces the built-in noise texture (lib.rs:281-309): (h, w, 4) uint8, e.g. decode_image_rgba8 of the crate's PNG."""
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("set_blue_noise: expected (h, w, 4) uint8")
        check(lib().sr_renderer_set_blue_noise(self._h, _p(a), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0])))

    def load_mesh(self, key, vertices, indices, material):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
        check(lib().sr_renderer_load_mesh(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m)))

    def update_mesh(self, key, vertices):
        """New vertex contents for a loaded mesh on every device slot; the next render applies it."""
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        check(lib().sr_renderer_update_mesh(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v))))

    def update_mesh_device(self, key, tensor):
        """update_mesh for a torch tensor on the first slot's GPU (Scene.update_mesh_device): validated once there, copied
        device to device into every slot's replica (sr_renderer_update_mesh_device)."""
        import torch
        ptr, n = _device_vertices(tensor, self.devices[0])
        check(lib().sr_renderer_update_mesh_device(self._h, C.c_uint64(key), ptr, C.c_uint32(n),
                                                   C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)))

    def set_mesh_skin(self, key, influences, n_joints):
        """Scene.set_mesh_skin on the first device slot's scene, which poses for every slot (sr_renderer_set_mesh_skin)."""
        if influences is None:
            check(lib().sr_renderer_set_mesh_skin(self._h, C.c_uint64(key), None, C.c_uint32(0), C.c_uint32(0)))
            return
        a = _skin_influences(influences)
        check(lib().sr_renderer_set_mesh_skin(self._h, C.c_uint64(key), _p(a), C.c_uint32(len(a)), C.c_uint32(int(n_joints))))

    def skin_mesh(self, key, joint_matrices):
        """Scene.skin_mesh on the first device slot; every further slot takes the posed vertices by a device copy; the next render
        applies them (sr_renderer_skin_mesh)."""
        m, n = _joint_matrices(joint_matrices)
        check(lib().sr_renderer_skin_mesh(self._h, C.c_uint64(key), _p(m), C.c_uint32(n), None))

    def set_mesh_morph(self, key, deltas):
        """Scene.set_mesh_morph on the first device slot's scene, which poses for every slot (sr_renderer_set_mesh_morph)."""
        if deltas is None:
            check(lib().sr_renderer_set_mesh_morph(self._h, C.c_uint64(key), None, C.c_uint32(0), C.c_uint32(0)))
            return
        a, nt, nv = _morph_deltas(deltas)
        check(lib().sr_renderer_set_mesh_morph(self._h, C.c_uint64(key), _p(a), C.c_uint32(nv), C.c_uint32(nt)))

    def pose_mesh(self, key, weights=None, joint_matrices=None):
        """Scene.pose_mesh on the first device slot; every further slot takes the posed vertices by a device copy; the next render
        applies them (sr_renderer_pose_mesh)."""
        wp, nt, mp, nj, keep = _pose_args(weights, joint_matrices)
        check(lib().sr_renderer_pose_mesh(self._h, C.c_uint64(key), wp, nt, mp, nj, None))

    def set_mesh_frame(self, key, normals=True, tangents=False):
        """Scene.set_mesh_frame on the first device slot's scene, which produces for every slot (sr_renderer_set_mesh_frame)."""
        flags = _frame_flags(normals, tangents)
        check(lib().sr_renderer_set_mesh_frame(self._h, C.c_uint64(key), C.c_uint32(flags)))

    def update_mesh_positions(self, key, positions):
        """Scene.update_mesh_positions on the first device slot (a torch tensor lives on its GPU); every further slot takes the
        records by a device copy; the next render applies them (sr_renderer_update_mesh_positions_device /
        sr_renderer_update_mesh_positions)."""
        on_device, ptr, n, stream, keep = _mesh_positions(positions, self.devices[0])
        if on_device:
            check(lib().sr_renderer_update_mesh_positions_device(self._h, C.c_uint64(key), ptr, C.c_uint32(n), stream))
        else:
            check(lib().sr_renderer_update_mesh_positions(self._h, C.c_uint64(key), ptr, C.c_uint32(n), None))

    def mesh_frame_info(self, key):
        """Scene.mesh_frame_info of the first device slot's scene, where the frame lives."""
        return self.replica_scene(0).mesh_frame_info(key)

    def set_mesh_build_type(self, key, build_type):
        """abi.BUILD_* of a loaded mesh's tree on every device slot (sr_renderer_set_mesh_build_type)."""
        check(lib().sr_renderer_set_mesh_build_type(self._h, C.c_uint64(key), C.c_uint32(build_type)))

    def set_mesh_tree_build(self, mode):
        """Scene.set_mesh_tree_build on every device slot (sr_renderer_set_mesh_tree_build)."""
        check(lib().sr_renderer_set_mesh_tree_build(self._h, C.c_uint32({"auto": 0, "host": 1, "device": 2}[mode])))

    def set_tree_height_bound(self, mode, cap=0):
        """Scene.set_tree_height_bound on every device slot (sr_renderer_set_tree_height_bound)."""
        check(lib().sr_renderer_set_tree_height_bound(self._h, C.c_uint32({"refuse": 0, "rebalance": 1}[mode]), C.c_uint32(cap)))
        return self

    def set_light_table_build(self, mode):
        """Scene.set_light_table_build on every device slot (sr_renderer_set_light_table_build)."""
        check(lib().sr_renderer_set_light_table_build(self._h, C.c_uint32({"host": abi.LIGHTS_HOST, "device": abi.LIGHTS_DEVICE}[mode])))
        return self

    def light_table_info(self, slot=0):
        """Scene.light_table_info of one device slot's scene (sr_renderer_light_table_info)."""
        info = abi.SrLightTableInfo()
        check(lib().sr_renderer_light_table_info(self._h, C.c_uint32(int(slot)), C.byref(info)))
        return info

    def pose_meshes(self, items):
        """Scene.pose_meshes on the first device slot; every further slot takes each item's posed vertices by a device copy; the
        next render applies them (sr_renderer_pose_meshes)."""
        rows, n, keep = _pose_items(items)
        check(lib().sr_renderer_pose_meshes(self._h, rows, n, None))

    def attach_clip(self, clip):
        """Scene.attach_clip on the first device slot's scene, which evaluates the clips (sr_renderer_attach_clip)."""
        cid = C.c_uint32()
        check(lib().sr_renderer_attach_clip(self._h, clip._h, C.byref(cid)))
        return cid.value

    def detach_clip(self, clip_id):
        check(lib().sr_renderer_detach_clip(self._h, C.c_uint32(clip_id)))

    def pose_actors(self, actors, items=(), tensor=None, keep_nodes=False):
        """Scene.pose_actors on the first device slot; every further slot takes each item's posed vertices by a device copy.
        `tensor` lives on the first slot's GPU: render_device_transforms takes it from there (sr_renderer_pose_actors)."""
        _actor_call(lib().sr_renderer_pose_actors, self._h, actors, items, tensor, keep_nodes, self.devices[0])

    def pose_actors_blended(self, actors, items=(), tensor=None, keep_nodes=False, keep_sources=False):
        """Scene.pose_actors_blended on the first device slot, as pose_actors (sr_renderer_pose_actors_blended)."""
        _actor_call(lib().sr_renderer_pose_actors_blended, self._h, actors, items, tensor, keep_nodes, self.devices[0], keep_sources, BlendedActorArgs)

    def attach_node_mask(self, weights):
        """Scene.attach_node_mask on the first device slot's scene (sr_renderer_attach_node_mask)."""
        m, mid = _node_mask(weights, "attach_node_mask"), C.c_uint32()
        check(lib().sr_renderer_attach_node_mask(self._h, _p(m), C.c_uint32(len(m)), C.byref(mid)))
        return mid.value

    def detach_node_mask(self, mask_id):
        check(lib().sr_renderer_detach_node_mask(self._h, C.c_uint32(mask_id)))

    def pose_actors_layered(self, actors, items=(), tensor=None, keep_nodes=False, keep_layers=False, layer_weights=False):
        """Scene.pose_actors_layered on the first device slot, as pose_actors (sr_renderer_pose_actors_layered)."""
        _actor_call(lib().sr_renderer_pose_actors_layered, self._h, actors, items, tensor, keep_nodes, self.devices[0], False, LayeredActorArgs, keep_layers,
                    layer_weights)

    def layer_weights_info(self):
        """Scene.layer_weights_info of the first device slot (sr_renderer_layer_weights_info)."""
        info = abi.SrLayerWeightsInfo()
        check(lib().sr_renderer_layer_weights_info(self._h, C.byref(info)))
        return info

    def actor_pose_info(self):
        info = abi.SrActorPoseInfo()
        check(lib().sr_renderer_actor_pose_info(self._h, C.byref(info)))
        return info

    def spline_pose_info(self):
        """Scene.spline_pose_info of the first device slot (sr_renderer_spline_pose_info)."""
        info = abi.SrSplinePoseInfo()
        check(lib().sr_renderer_spline_pose_info(self._h, C.byref(info)))
        return info

    def set_pose_batch(self, on):
        """Whether pose_scene poses the file's rigged and morphed meshes by one pose_meshes (sr_renderer_set_pose_batch). Off by
        default; SR_POSE_BATCH=on in the environment turns it on at creation."""
        check(lib().sr_renderer_set_pose_batch(self._h, C.c_uint32(abi.POSE_BATCH_ON if on else abi.POSE_BATCH_OFF)))

    def set_mesh_tree_batch(self, mode):
        """Scene.set_mesh_tree_batch on every device slot (sr_renderer_set_mesh_tree_batch)."""
        check(lib().sr_renderer_set_mesh_tree_batch(self._h, C.c_uint32({"off": 0, "on": 1}[mode])))
        return self

    def mesh_tree_info(self, slot=0):
        """Scene.mesh_tree_info of one device slot's scene."""
        return self.replica_scene(slot).mesh_tree_info()

    def set_config(self, config):
        check(lib().sr_renderer_set_config(self._h, C.byref(config)))

    def load_gltf(self, path):
        """Renderer::load_gltf (lib.rs:779-786) -> (group, [(key, [3x4 transforms])])."""
        ls = C.c_void_p()
        check(lib().sr_renderer_load_gltf(self._h, path.encode(), C.byref(ls)))
        try:
            group, nk, nt = C.c_uint64(), C.c_uint32(), C.c_uint32()
            kp, cp, tp = C.c_void_p(), C.c_void_p(), C.c_void_p()
            check(lib().sr_loaded_scene_get(ls, C.byref(group), C.byref(kp), C.byref(cp), C.byref(nk), C.byref(tp), C.byref(nt)))
            keys, counts = _np_from(kp, nk.value, np.uint64), _np_from(cp, nk.value, np.uint32)
            xf = _np_from(tp, nt.value * 12, np.float32).reshape(-1, 12)
            inst, o = [], 0
            for k, c in zip(keys, counts):
                inst.append((int(k), [xf[o + j].copy() for j in range(int(c))]))
                o += int(c)
            return group.value, inst
        finally:
            lib().sr_loaded_scene_destroy(ls)

    def load_scene(self, gltf):
        """Renderer::load_scene for an open Gltf -> LoadedScene (sr_renderer_load_scene)."""
        ls = C.c_void_p()
        check(lib().sr_renderer_load_scene(self._h, gltf._h, C.byref(ls)))
        loaded = LoadedScene(ls)
        loaded.instance_blas = gltf.instance_blases()
        return loaded

    def attach_skins(self, gltf, loaded):
        """Attaches the rig of every skinned mesh of a loaded scene and makes those meshes BUILD_RAPIDLY_CHANGING
        (sr_renderer_attach_skins)."""
        check(lib().sr_renderer_attach_skins(self._h, gltf._h, loaded._h))

    def attach_morphs(self, gltf, loaded):
        """Attaches the morph targets of every mesh of a loaded scene that has some and makes those meshes
        BUILD_RAPIDLY_CHANGING; pose_scene then plays their weight animations too (sr_renderer_attach_morphs)."""
        check(lib().sr_renderer_attach_morphs(self._h, gltf._h, loaded._h))

    def pose_scene(self, gltf, loaded, animation, time_seconds):
        """Poses every skinned mesh of a loaded scene at `time_seconds` of `animation` on the GPU and returns the posed instances,
        [(key, [3x4 transforms])], for the next render (sr_renderer_pose_scene)."""
        xf = np.zeros((max(loaded.n_transforms, 1), 12), dtype=np.float32)
        check(lib().sr_renderer_pose_scene(self._h, gltf._h, loaded._h, C.c_int32(animation), C.c_float(time_seconds), _p(xf), None))
        return loaded.grouped(xf[:loaded.n_transforms])

    def unload_scene(self, group):
        check(lib().sr_renderer_unload_scene(self._h, C.c_uint64(group)))

    def unload_mesh(self, key):
        check(lib().sr_renderer_unload_mesh(self._h, C.c_uint64(key)))

    def render(self, camera, instances):
        pos, tgt, fov = camera
        keys, counts, xf = _instance_arrays(instances)
        frame = C.c_uint64()
        check(lib().sr_renderer_render(self._h, _f3(pos), _f3(tgt), C.c_float(fov), _p(keys), _p(counts), C.c_uint32(len(keys)), _p(xf),
                                       None, C.byref(frame)))
        return frame.value

    def render_device_transforms(self, camera, layout, tensor):
        """render with the instance list taken from the GPU: `layout` is [(key, count), ...], `tensor` as for
        Scene.set_instances_device, on the first device slot's GPU (sr_renderer_render_device_transforms)."""
        import torch
        pos, tgt, fov = camera
        keys, counts, ptr = _device_transforms(layout, tensor, self.devices[0])
        frame = C.c_uint64()
        check(lib().sr_renderer_render_device_transforms(self._h, _f3(pos), _f3(tgt), C.c_float(fov), _p(keys), _p(counts), C.c_uint32(len(keys)), ptr,
                                                         C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream), C.byref(frame)))
        return frame.value

    def wait_frame(self, frame):
        check(lib().sr_renderer_wait_frame(self._h, C.c_uint64(frame)))

    def render_to_host_memory(self, camera, instances):
        pos, tgt, fov = camera
        keys, counts, xf = _instance_arrays(instances)
        out = np.zeros((self.size[1], self.size[0], 4), dtype=np.uint8)
        check(lib().sr_renderer_render_to_host_memory(self._h, _f3(pos), _f3(tgt), C.c_float(fov), _p(keys), _p(counts), C.c_uint32(len(keys)),
                                                      _p(xf), _p(out)))
        return out

    @property
    def relative_frame_count(self):
        n = C.c_uint32()
        check(lib().sr_renderer_get(self._h, None, None, None, C.byref(n)))
        return n.value


def rays_to_device(rays_np, device="cuda:0"):
    import torch
    a = np.ascontiguousarray(rays_np, dtype=abi.RAY)
    return torch.from_numpy(a.view(np.float32).reshape(-1, 8).copy()).to(device)


def hits_from_device(hits_t):
    return hits_t.cpu().numpy().reshape(-1).view(abi.HIT)
